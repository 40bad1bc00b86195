"""The Groth16 prover on the device (pa_groth16_*, include/pairing_amd.h): witness in,
proof out, k proofs per call.  Affine coordinates are canonical, so the device's
(k, 51) proof rows are compared bit for bit with tests/groth16_ref.py, whose key
points are known multiples of the generators: its proofs are the four formulas
of create_proof on integers mod r and three g{1,2}_mul_generator calls, with no
multiexp and no curve addition from the code under test.  A real setup from a
tiny trapdoor checks the formulas themselves against the pairing equation."""
import ctypes
import os
import re

import numpy as np
import pytest

import decode_cases as D
import groth16_ref as G
from helpers import R_ORDER, rng
from test_fr_ntt import mont_rows

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
HEADER = os.path.join(ROOT, "include", "pairing_amd.h")
P, N, U = ctypes.c_void_p, ctypes.c_size_t, ctypes.c_uint
NEW_SIGS = {
    "pa_groth16_pk_create": [P, U, ctypes.POINTER(P)],
    "pa_groth16_pk_in_subgroup": [P],
    "pa_groth16_prove_workspace_bytes": [P, P, N],
    "pa_groth16_prove_device": [P, P, P, P, P, P, N, P, P, N, P],
    "pa_groth16_prove": [P, P, P, P, P, P, N, P],
}
NV, NPUB, NROWS, LOGN = 40, 3, 50, 6


def rows_of(vals):
    return mont_rows(vals) if vals else np.zeros((0, 4), np.uint64)


def flat(ws):
    return rows_of([v for w in ws for v in w])


@pytest.fixture(scope="module")
def real(oracle):
    """the real-setup system at log_n = 5: 30 rows, 12 variables, 3 public; four satisfying proofs' inputs"""
    mats, w = G.satisfied_system(4100, 30, 12)
    key, gamma, ic = G.real_setup(4101, mats, 12, 3, 5)
    g = rng(4102)
    rs, ss = G.rand_fr(g, 4), G.rand_fr(g, 4)
    return mats, w, key, gamma, ic, rs, ss


# ---------------- CPU ----------------

def test_reference_proof_of_a_real_setup_verifies(oracle, real):
    mats, w, key, gamma, ic, rs, ss = real
    a, b, c = G.eval_ints(mats, [w], 5)
    assert all(x * y % R_ORDER == z for x, y, z in zip(a, b, c)) and any(a) and any(c)
    h = G.quotient_ints(oracle, mats, [w], 5)[0]
    assert h[31] == 0 and any(h)
    proof = G.ref_proofs(oracle, key, mats, [w], rs[:1], ss[:1])[0]
    assert G.pairing_product_is_one(oracle, *G.verify_pairs(oracle, key, gamma, ic, w[:3], proof))
    # one witness entry changed (a private one): the same public input no longer verifies
    bad = list(w)
    bad[7] = (bad[7] + 1) % R_ORDER
    a, b, c = G.eval_ints(mats, [bad], 5)
    assert any(x * y % R_ORDER != z for x, y, z in zip(a, b, c))
    proof = G.ref_proofs(oracle, key, mats, [bad], rs[:1], ss[:1])[0]
    assert not G.pairing_product_is_one(oracle, *G.verify_pairs(oracle, key, gamma, ic, w[:3], proof))


def test_groth16_symbols_are_declared_and_bound():
    from pairing_amd import _native
    with open(HEADER) as f:
        src = f.read()
    declared = set(re.findall(r"^\s*(?:const\s+)?\w+\s*\*?\s*(pa_\w+)\s*\(", src, flags=re.M))
    for name, sig in NEW_SIGS.items():
        assert name in declared, name
        assert _native._SIGS[name] == sig, name
        assert getattr(_native._lib, name).argtypes == sig
    assert "pa_groth16_pk_free" in declared and _native._lib.pa_groth16_pk_free.restype is None
    assert _native._lib.pa_groth16_prove_workspace_bytes.restype is N
    assert _native._lib.pa_groth16_prove.restype is ctypes.c_int
    for decl in ("} pa_groth16_key;", "} pa_groth16_proof;", "typedef struct pa_groth16_pk pa_groth16_pk;"):
        assert decl in src, decl
    # the ctypes mirror of pa_groth16_key: three G1 and two G2 records, two sizes, five pointers, a size
    assert ctypes.sizeof(_native.Groth16Key) == 3 * 104 + 2 * 200 + 8 * 8
    assert _native.W_PROOF == 51
    import pairing_amd
    import pairing_amd.device as pdev
    for name in ("Groth16Pk", "groth16_pk", "groth16_prove"):
        assert name in pairing_amd.__all__ and hasattr(pairing_amd, name), name
    assert hasattr(pdev, "groth16_prove") and hasattr(pdev, "groth16_prove_workspace")
    with open(os.path.join(ROOT, "include", "pairing_amd.hpp")) as f:
        hpp = f.read()
    assert re.search(r"class Groth16Prover\b", hpp) and re.search(r"\bprove\(", hpp)
    lib = _native._lib
    assert lib.pa_groth16_pk_create(None, 3, ctypes.byref(P(0))) == -1
    assert lib.pa_groth16_pk_in_subgroup(None) == 0
    assert lib.pa_groth16_prove_workspace_bytes(None, None, 1) == 0
    assert lib.pa_groth16_prove(None, None, None, None, None, None, 1, None) == -1
    assert lib.pa_groth16_prove_device(None, None, None, None, None, None, 0, None, None, 0, None) == -1
    lib.pa_groth16_pk_free(None)
    # creation errors that come before any device call
    key = _native.Groth16Key()
    for n_vars, n_public, h_len, log_n in ((2, 3, 0, 2), (0, 0, 5, 2), (0, 0, 0, 29)):
        key.n_vars, key.n_public, key.h_len = n_vars, n_public, h_len
        h = P(0x1234)
        assert lib.pa_groth16_pk_create(ctypes.byref(key), log_n, ctypes.byref(h)) == -1 and h.value is None


def test_python_layers_check_arguments_without_a_device():
    import torch
    import pairing_amd as pa
    import pairing_amd.device as pdev
    from pairing_amd._native import FrNttDomain, Groth16Pk, R1cs
    z = lambda *s: np.zeros(s, np.uint64)  # noqa: E731
    g1, g2 = z(1, 13), z(1, 25)
    ok = dict(alpha_g1=g1, beta_g1=g1, delta_g1=g1, beta_g2=g2, delta_g2=g2, a_query=z(4, 13), b_g1_query=z(4, 13),
              b_g2_query=z(4, 25), l_query=z(3, 13), h_query=z(3, 13), n_public=1, log_n=2)
    for change, what in ((dict(alpha_g1=z(2, 13)), "alpha_g1"), (dict(beta_g2=g1), "beta_g2"),
                         (dict(b_g1_query=z(3, 13)), "n_vars"), (dict(b_g2_query=z(4, 13)), "b_g2_query"),
                         (dict(l_query=z(4, 13)), "l_query"), (dict(n_public=5), "l_query"),
                         (dict(h_query=z(5, 13)), "h_query"), (dict(log_n=29), "log_n")):
        with pytest.raises(ValueError, match=what):
            pa.groth16_pk(**dict(ok, **change))
    pk = Groth16Pk(P(1), 3, 5, 2, 7, owns=False)   # live-looking handles: every error comes before a native call
    sysm, dom = R1cs(P(1), 6, 5, owns=False), FrNttDomain(P(1), 3, owns=False)
    w, r = z(10, 4), z(2, 4)
    for args, what in (((object(), sysm, dom, w, r, r), "groth16_pk"), ((pk, object(), dom, w, r, r), "r1cs"),
                       ((pk, sysm, object(), w, r, r), "fr_ntt_domain"),
                       ((pk, sysm, FrNttDomain(P(1), 4, owns=False), w, r, r), "log_n"),
                       ((pk, R1cs(P(1), 6, 4, owns=False), dom, w, r, r), "columns"),
                       ((pk, R1cs(P(1), 9, 5, owns=False), dom, w, r, r), "rows"),
                       ((pk, sysm, dom, z(9, 4), r, r), "k proofs"), ((pk, sysm, dom, w, r, z(3, 4)), "k proofs"),
                       ((pk, sysm, dom, z(10, 5), r, r), "shape")):
        with pytest.raises(ValueError, match=what):
            pa.groth16_prove(*args)
    t = lambda *s: torch.zeros(*s, dtype=torch.int64)  # noqa: E731
    out, ws = t(2, 51), torch.zeros(8, dtype=torch.uint8)
    for args, what in (((object(), sysm, dom, t(10, 4), t(2, 4), t(2, 4), out, ws), "groth16_pk"),
                       ((pk, sysm, dom, t(9, 4), t(2, 4), t(2, 4), out, ws), "k proofs"),
                       ((pk, sysm, dom, t(10, 4), t(2, 4), t(2, 4), t(1, 51), ws), "needs 2")):
        with pytest.raises(ValueError, match=what):
            pdev.groth16_prove(*args)
    with pytest.raises(ValueError, match="groth16_pk"):
        pdev.groth16_prove_workspace(object(), sysm, 1, "cpu")
    with pytest.raises(ValueError, match="r1cs"):
        pdev.groth16_prove_workspace(pk, object(), 1, "cpu")
    with pytest.raises(ValueError, match="negative"):
        pdev.groth16_prove_workspace(pk, sysm, -1, "cpu")
    pk.close()
    with pytest.raises(ValueError, match="close"):
        pa.groth16_prove(pk, sysm, dom, w, r, r)


# ---------------- GPU ----------------

class Case:
    """a key, a system, and the device objects over them"""

    def __init__(self, gpu, oracle, key, mats, n_rows, points=None):
        self.gpu, self.oracle, self.key, self.mats = gpu, oracle, key, mats
        self.pk = gpu.groth16_pk(*(points or key.points(oracle)))
        self.sysm = gpu.r1cs(*(G.csr(m) for m in mats), n_rows, key.n_vars)
        self.dom = gpu.fr_ntt_domain(key.log_n)

    def close(self):
        for x in (self.pk, self.sysm, self.dom):
            x.close()

    def check(self, ws, rs, ss):
        got = self.gpu.groth16_prove(self.pk, self.sysm, self.dom, flat(ws), rows_of(rs), rows_of(ss))
        want = G.ref_proofs(self.oracle, self.key, self.mats, ws, rs, ss)
        assert got.shape == (len(ws), 51)
        np.testing.assert_array_equal(got, want)
        return got


@pytest.fixture(scope="module")
def small(oracle):
    """n_vars = 40, n_public = 3, n_rows = 50, log_n = 6: a satisfied system and its witness, another witness
    that does not satisfy it, and keys with h_len = n - 1 and h_len = n over the same other points"""
    mats, w = G.satisfied_system(4000, NROWS, NV)
    key = G.random_key(4001, NV, NPUB, LOGN, (1 << LOGN) - 1)
    full = G.Key(key.alpha, key.beta, key.delta, key.a, key.b, key.l, key.h + G.rand_fr(rng(4002), 1), NPUB, LOGN)
    g = rng(4003)
    other = [1] + G.rand_fr(g, NV - 1)
    return mats, w, other, key, full


@pytest.mark.gpu
def test_small_system_bit_exact(gpu, oracle, small):
    mats, w, other, key, full = small
    g = rng(4010)
    c = Case(gpu, oracle, key, mats, NROWS)
    try:
        assert c.pk.in_subgroup and (c.pk.n_vars, c.pk.n_public, c.pk.h_len, c.pk.log_n) == (NV, NPUB, 63, LOGN)
        one = c.check([w], G.rand_fr(g, 1), G.rand_fr(g, 1))                       # k = 1
        rs, ss = G.rand_fr(g, 3), G.rand_fr(g, 3)
        three = c.check([w, other, w], rs, ss)                                      # k = 3, the middle one unsatisfied
        assert not (three[0] == three[2]).all() and not (one[0] == three[0]).all()
        c.check([w, other], [0, 0], [0, 0])                                         # r = s = 0
        c.check([w, other], [R_ORDER - 1, 0], [R_ORDER - 1, R_ORDER - 1])           # r = r_order - 1
        c.check([[1] + [0] * (NV - 1)], G.rand_fr(g, 1), G.rand_fr(g, 1))           # only the constant one
        c.check([[1] + [0] * (NV - 1)], [0], [0])
        c.check([], [], [])                                                         # k = 0
        # the unsatisfied witness has a top quotient row, which h_len = n - 1 drops
        assert G.quotient_ints(oracle, mats, [other], LOGN)[0][63] != 0
        assert G.quotient_ints(oracle, mats, [w], LOGN)[0][63] == 0
    finally:
        c.close()


@pytest.mark.gpu
def test_h_len_n_and_the_last_base(gpu, oracle, small):
    mats, w, other, key, full = small
    g = rng(4020)
    rs, ss = G.rand_fr(g, 2), G.rand_fr(g, 2)
    c = Case(gpu, oracle, full, mats, NROWS)
    try:
        assert c.pk.h_len == 64
        got = c.check([w, other], rs, ss)
    finally:
        c.close()
    # for the satisfied witness the last base does not matter; for the other one it does
    short = G.ref_proofs(oracle, key, mats, [w, other], rs, ss)
    np.testing.assert_array_equal(got[0], short[0])
    assert not (got[1] == short[1]).all()


@pytest.mark.gpu
def test_a_query_point_outside_the_subgroup(gpu, oracle, small):
    """one a_query point on the curve but outside G1: the key reports it, the multiexps take the 257-bit
    path over that set, and the proof is the reference's (the witness is zero at that variable, so the
    reference, which knows points only as multiples of the generator, still applies)"""
    mats, w, other, key, full = small
    pts, truth = D.subgroup_points(1, seed=4030, n=1)
    assert not truth[0]
    points = list(key.points(oracle))
    a_query = points[5].copy()
    a_query[17] = np.array(D.aff_record(1, pts[0]), np.uint64)
    points[5] = a_query
    ws = [list(other), [1] + [0] * (NV - 1)]
    ws[0][17] = 0
    g = rng(4031)
    c = Case(gpu, oracle, key, mats, NROWS, points=points)
    try:
        assert not c.pk.in_subgroup
        c.check(ws, G.rand_fr(g, 2), G.rand_fr(g, 2))
    finally:
        c.close()


@pytest.mark.gpu
def test_two_pass_domain(gpu, oracle):
    """log_n = 11, n_rows = 1500, n_vars = 300, k = 2: the quotient runs as several passes"""
    n_vars, n_rows, log_n = 300, 1500, 11
    mats, w = G.satisfied_system(4040, n_rows, n_vars)
    key = G.random_key(4041, n_vars, 5, log_n, (1 << log_n) - 1)
    g = rng(4042)
    c = Case(gpu, oracle, key, mats, n_rows)
    try:
        assert c.dom.passes > 1
        c.check([w, [1] + G.rand_fr(g, n_vars - 1)], G.rand_fr(g, 2), G.rand_fr(g, 2))
    finally:
        c.close()


@pytest.mark.gpu
def test_real_setup_proofs_verify_on_the_device(gpu, oracle, real):
    mats, w, key, gamma, ic, rs, ss = real
    c = Case(gpu, oracle, key, mats, 30)
    try:
        good = c.check([w] * 4, rs, ss)
        spoiled = list(w)
        spoiled[9] = (spoiled[9] + 5) % R_ORDER
        bad = c.check([w, w, spoiled, w], rs, ss)
    finally:
        c.close()
    for proofs, want in ((good, [True] * 4), (bad, [True, True, False, True])):
        pairs = [G.verify_pairs(oracle, key, gamma, ic, w[:3], pr) for pr in proofs]
        p = np.concatenate([x[0] for x in pairs])
        q = np.concatenate([x[1] for x in pairs])
        _, ok, is_one = gpu.multi_pairing_batch(p, q, pairs_per_product=4)
        assert ok.all() and is_one.astype(bool).tolist() == want


def _dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a).view(np.int64)).to("cuda:0")


@pytest.mark.gpu
def test_device_entry_on_a_stream_and_every_prove_error(gpu, oracle, small):
    import torch
    import pairing_amd.device as pdev
    from pairing_amd import _native
    mats, w, other, key, full = small
    g = rng(4050)
    k = 2
    rs, ss = G.rand_fr(g, k), G.rand_fr(g, k)
    want = G.ref_proofs(oracle, key, mats, [w, other], rs, ss)
    s = torch.cuda.Stream()
    c = Case(gpu, oracle, key, mats, NROWS)
    try:
        ws = pdev.groth16_prove_workspace(c.pk, c.sysm, k, "cuda:0")
        assert ws.numel() == c.pk.prove_workspace_bytes(c.sysm, k)    # exactly the queried size
        W, R, S = _dev(flat([w, other])), _dev(rows_of(rs)), _dev(rows_of(ss))
        out = _dev(np.full((k + 1, 51), 0x5a5a5a5a5a5a5a5a, np.uint64))
        torch.cuda.synchronize()
        with torch.cuda.stream(s):
            pdev.groth16_prove(c.pk, c.sysm, c.dom, W, R, S, out, ws, stream=s)
        s.synchronize()
        host = out.cpu().numpy().view(np.uint64)
        np.testing.assert_array_equal(host[:k], want)
        assert (host[k] == 0x5a5a5a5a5a5a5a5a).all()
        np.testing.assert_array_equal(W.cpu().numpy().view(np.uint64), flat([w, other]))
        with pytest.raises(ValueError, match="workspace"):
            pdev.groth16_prove(c.pk, c.sysm, c.dom, W, R, S, out, ws[:-1], stream=s)
        with pytest.raises(ValueError, match="split"):
            pdev.groth16_prove_workspace(c.pk, c.sysm, 1 << 40, "cuda:0")

        # what the C entries refuse before anything runs
        lib = _native._lib
        fresh = _dev(np.full((k, 51), 0x5a5a5a5a5a5a5a5a, np.uint64))
        p = lambda t: ctypes.c_void_p(t.data_ptr())  # noqa: E731
        sp = ctypes.c_void_p(s.cuda_stream)
        h, hr, hd = c.pk.handle(), c.sysm.handle(), c.dom.handle()
        with gpu.fr_ntt_domain(LOGN + 1) as d7, gpu.r1cs(*(G.csr(m) for m in mats), NROWS, NV + 1) as wide, \
                gpu.r1cs(*(G.csr(m + [[]] * 20) for m in mats), NROWS + 20, NV) as tall:
            tail = (p(W), p(R), p(S), k, p(fresh), p(ws), ws.numel(), sp)
            cases = {
                "the domain's log_n differs": (h, hr, d7.handle()) + tail,
                "cols != n_vars": (h, wide.handle(), hd) + tail,
                "rows > n": (h, tall.handle(), hd) + tail,
                "workspace one byte short": (h, hr, hd) + tail[:6] + (ws.numel() - 1, sp),
                "a batch over the limit": (h, hr, hd, p(W), p(R), p(S), 1 << 40, p(fresh), p(ws), ws.numel(), sp),
                "no key": (None, hr, hd) + tail,
            }
            if torch.cuda.device_count() > 1:
                other_stream = torch.cuda.Stream(device="cuda:1")
                cases["a stream on another device"] = (h, hr, hd) + tail[:7] + (ctypes.c_void_p(other_stream.cuda_stream),)
            for what, args in cases.items():
                assert lib.pa_groth16_prove_device(*args) == -1, what
                assert lib.pa_last_error(), what
            assert lib.pa_groth16_prove_workspace_bytes(h, wide.handle(), k) == 0
            assert lib.pa_groth16_prove_workspace_bytes(h, hr, 1 << 40) == 0
        torch.cuda.synchronize()
        assert (fresh.cpu().numpy().view(np.uint64) == 0x5a5a5a5a5a5a5a5a).all()
    finally:
        c.close()
