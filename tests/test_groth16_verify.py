"""The Groth16 verifier on the device (pa_groth16_vk*, pa_groth16_verify*,
include/pairing_amd.h): k proofs per call over a prepared verifying key.  The
public-input sum (affine records), gt (final-exponentiation output) and valid
are canonical, so everything is compared bit for bit with
tests/groth16_verify_ref.py: the oracle's CurveAffine::mul / add_assign /
into_affine for the sum, its pairing and Fq12 product for the verdict.

The verify tests draw their proofs from one pool of nine distinct cases whose
reference is computed once; a batch of k proofs tiles the pool, so a k of a
thousand costs the oracle nothing more."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

import decode_cases as D
import groth16_ref as G
import groth16_verify_ref as V
from helpers import R_ORDER, rng, set_infinity, small_scalars
from test_fr_ntt import mont_rows

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
HEADER = os.path.join(ROOT, "include", "pairing_amd.h")
P, N, U = ctypes.c_void_p, ctypes.c_size_t, ctypes.c_uint
NEW_SIGS = {
    "pa_groth16_vk_create": [P, ctypes.POINTER(P)],
    "pa_groth16_vk_n_public": [P],
    "pa_groth16_vk_bytes": [P],
    "pa_groth16_vk_input_sum_workspace_bytes": [P, N],
    "pa_groth16_verify_workspace_bytes": [P, N],
    "pa_groth16_vk_input_sum_device": [P, P, N, U, N, P, P, N, P],
    "pa_groth16_vk_input_sum": [P, P, N, U, N, P],
    "pa_groth16_verify_device": [P, P, P, N, U, N, P, P, P, N, P],
    "pa_groth16_verify": [P, P, P, N, U, N, P, P],
    "pa_groth16_verify_encoded_device": [P, P, P, N, U, N, P, P, P, P, N, P],
    "pa_groth16_verify_encoded": [P, P, P, N, U, N, P, P, P],
}
SIZE_T_RESULTS = ("pa_groth16_vk_n_public", "pa_groth16_vk_bytes", "pa_groth16_vk_input_sum_workspace_bytes",
                  "pa_groth16_verify_workspace_bytes")
KNOB = "PA_G16V_SHARED_MIN"


def rows_of(vals):
    return mont_rows(vals) if vals else np.zeros((0, 4), np.uint64)


@pytest.fixture(scope="module")
def real(oracle):
    """the real-setup system at log_n = 5: 30 rows, 12 variables, 3 public (l = 2); the key's points"""
    mats, w = G.satisfied_system(5100, 30, 12)
    key, gamma, ic = G.real_setup(5101, mats, 12, 3, 5)
    return mats, w, key, V.real_vk(oracle, key, gamma, ic)


class Pool:
    """distinct proofs over the real setup's key with their inputs and the reference's (gt, valid)"""

    def __init__(self, vk, proofs, inputs, gt, valid):
        self.vk, self.proofs, self.inputs, self.gt, self.valid = vk, proofs, inputs, gt, valid
        flat = [x for row in inputs for x in row]
        self.mont = mont_rows(flat).reshape(len(inputs), vk.n_inputs, 4)
        self.repr = small_scalars(flat).reshape(len(inputs), vk.n_inputs, 4)

    def batch(self, k, shift=0):
        """(proofs (k, 51), Montgomery rows, repr rows, gt, valid) of k proofs tiling the pool from `shift`"""
        idx = (np.arange(k) + shift) % self.proofs.shape[0]
        return (np.ascontiguousarray(self.proofs[idx]), np.ascontiguousarray(self.mont[idx].reshape(-1, 4)),
                np.ascontiguousarray(self.repr[idx].reshape(-1, 4)), self.gt[idx], self.valid[idx])


@pytest.fixture(scope="module")
def pool(oracle, real):
    mats, w, key, vk = real
    g = rng(5110)
    rs, ss = G.rand_fr(g, 3), G.rand_fr(g, 3)
    spoiled = list(w)
    spoiled[9] = (spoiled[9] + 5) % R_ORDER
    good = G.ref_proofs(oracle, key, mats, [w, w, spoiled], rs, ss)
    other = V.proof_rows(oracle, *[G.rand_fr(g, 1) for _ in range(3)])[0]
    twist, truth = D.subgroup_points(2, seed=5111, n=1)
    assert not truth[0]
    proofs = [good[0], good[1], good[2]]
    for lo, hi in ((0, 13), (13, 38), (38, 51)):       # one of A, B, C replaced
        pr = good[0].copy()
        pr[lo:hi] = other[lo:hi]
        proofs.append(pr)
    proofs.append(good[1].copy())                         # a wrong public input (below)
    a_inf = good[0].copy()
    a_inf[:13] = set_infinity(np.zeros((1, 13), np.uint64), [0])[0]
    proofs.append(a_inf)                                  # A at infinity
    b_out = good[0].copy()
    b_out[13:38] = np.array(D.aff_record(2, twist[0]), np.uint64)
    proofs.append(b_out)                                  # B on the twist, outside G2
    inputs = [list(w[1:3]) for _ in proofs]
    inputs[6][0] = (inputs[6][0] + 1) % R_ORDER
    proofs = np.ascontiguousarray(np.stack(proofs))
    gt, valid = V.ref_verify(oracle, vk, proofs, inputs)
    assert valid.tolist() == [True, True] + [False] * 7
    return Pool(vk, proofs, inputs, gt, valid)


# ---------------- CPU ----------------

def test_reference_helper_accepts_a_real_proof_and_rejects_a_spoiled_witness(oracle, real):
    mats, w, key, vk = real
    g = rng(5120)
    spoiled = list(w)
    spoiled[7] = (spoiled[7] + 1) % R_ORDER
    proofs = G.ref_proofs(oracle, key, mats, [w, spoiled], G.rand_fr(g, 2), G.rand_fr(g, 2))
    gt, valid = V.ref_verify(oracle, vk, proofs, [w[1:3], w[1:3]])
    assert valid.tolist() == [True, False]
    assert (gt[0] == oracle.pairing(vk.alpha_g1, vk.beta_g2)[0]).all() and gt[1].any()
    # a wrong public input with the right proof
    assert not V.ref_verify(oracle, vk, proofs[:1], [[w[1], (w[2] + 1) % R_ORDER]])[1][0]
    # the wire form decodes back to the records
    enc = V.encode_proofs(proofs)
    assert enc.shape == (2, 192) and not V.decode_status(oracle, enc).any()
    np.testing.assert_array_equal(oracle.decode(2, np.ascontiguousarray(enc[:, 48:144]), True)[0], proofs[:, 13:38])
    np.testing.assert_array_equal(oracle.decode(1, np.ascontiguousarray(enc[:, 144:]), True)[0], proofs[:, 38:])


def test_verifier_symbols_are_declared_exported_and_bound():
    from pairing_amd import _native
    with open(HEADER) as f:
        src = f.read()
    declared = set(re.findall(r"^\s*(?:const\s+)?\w+\s*\*?\s*(pa_\w+)\s*\(", src, flags=re.M))
    lib = _native._lib
    for name, sig in NEW_SIGS.items():
        assert name in declared, name
        assert _native._SIGS[name] == sig, name
        assert getattr(lib, name).argtypes == sig
        assert getattr(lib, name).restype is (N if name in SIZE_T_RESULTS else ctypes.c_int), name
    assert "pa_groth16_vk_free" in declared and lib.pa_groth16_vk_free.restype is None
    for decl in ("} pa_groth16_vkey;", "typedef struct pa_groth16_vk pa_groth16_vk;", "#define PA_GROTH16_VK_MAX_INPUTS",
                 "#define PA_GROTH16_VERIFY_SHARED_MIN", "#define PA_GROTH16_ENCODED_PROOF_BYTES 192"):
        assert decl in src, decl
    assert _native.GROTH16_VK_MAX_INPUTS == int(re.search(r"#define PA_GROTH16_VK_MAX_INPUTS (\d+)", src).group(1))
    import pairing_amd
    import pairing_amd.device as pdev
    for name in ("Groth16Vk", "groth16_vk", "groth16_verify", "groth16_verify_encoded", "groth16_input_sum"):
        assert name in pairing_amd.__all__ and hasattr(pairing_amd, name), name
    for name in ("groth16_verify_workspace", "groth16_verify", "groth16_verify_encoded"):
        assert hasattr(pdev, name), name
    with open(os.path.join(ROOT, "include", "pairing_amd.hpp")) as f:
        hpp = f.read()
    assert re.search(r"class Groth16Verifier\b", hpp)
    for method in ("verify", "verify_encoded", "input_sum", "verifier"):
        assert re.search(r"\b%s\(" % method, hpp), method
    with open(os.path.join(ROOT, "pairing_amd", "Makefile")) as f:
        assert "lib/kernels_groth16_verify.o" in f.read()
    # what the entries refuse before any device call
    assert lib.pa_groth16_vk_create(None, ctypes.byref(P(0))) == -1 and lib.pa_last_error()
    assert lib.pa_groth16_vk_n_public(None) == 0 and lib.pa_groth16_vk_bytes(None) == 0
    assert lib.pa_groth16_verify_workspace_bytes(None, 1) == 0
    assert lib.pa_groth16_vk_input_sum_workspace_bytes(None, 1) == 0
    assert lib.pa_groth16_verify(None, None, None, 0, 0, 1, None, None) == -1
    assert lib.pa_groth16_verify_device(None, None, None, 0, 0, 1, None, None, None, 0, None) == -1
    assert lib.pa_groth16_verify_encoded(None, None, None, 0, 0, 1, None, None, None) == -1
    assert lib.pa_groth16_verify_encoded_device(None, None, None, 0, 0, 1, None, None, None, None, 0, None) == -1
    assert lib.pa_groth16_vk_input_sum(None, None, 0, 0, 1, None) == -1
    assert lib.pa_groth16_vk_input_sum_device(None, None, 0, 0, 1, None, None, 0, None) == -1
    lib.pa_groth16_vk_free(None)
    key = _native.Groth16VKey()
    ic = (ctypes.c_uint64 * 13)()
    for n_public, ic_ptr in ((0, ctypes.addressof(ic)), (_native.GROTH16_VK_MAX_INPUTS + 2, ctypes.addressof(ic)), (1, None)):
        key.n_public, key.ic = n_public, ic_ptr
        h = P(0x1234)
        assert lib.pa_groth16_vk_create(ctypes.byref(key), ctypes.byref(h)) == -1 and h.value is None


def test_vkey_struct_layout_matches_the_header(tmp_path):
    from pairing_amd import _native
    src = tmp_path / "layout.c"
    src.write_text('#include <stddef.h>\n#include <stdio.h>\n#include "pairing_amd.h"\n'
                   "int main(void) {\n"
                   '    printf("%zu %zu %zu %zu %zu %zu %zu\\n", sizeof(pa_groth16_vkey), offsetof(pa_groth16_vkey, alpha_g1),\n'
                   "           offsetof(pa_groth16_vkey, beta_g2), offsetof(pa_groth16_vkey, gamma_g2),\n"
                   "           offsetof(pa_groth16_vkey, delta_g2), offsetof(pa_groth16_vkey, ic),\n"
                   "           offsetof(pa_groth16_vkey, n_public));\n    return 0;\n}\n")
    exe = str(tmp_path / "layout")
    subprocess.run(["gcc", "-std=c11", "-Wall", "-Werror", "-I" + os.path.join(ROOT, "include"), str(src), "-o", exe],
                   check=True, capture_output=True, text=True, timeout=120)
    got = [int(x) for x in subprocess.run([exe], check=True, capture_output=True, text=True, timeout=60).stdout.split()]
    K = _native.Groth16VKey
    assert got == [ctypes.sizeof(K)] + [getattr(K, f).offset for f in
                                        ("alpha_g1", "beta_g2", "gamma_g2", "delta_g2", "ic", "n_public")]
    assert got == [104 + 3 * 200 + 16, 0, 104, 304, 504, 704, 712]


def test_python_layers_check_arguments_without_a_device():
    import torch
    import pairing_amd as pa
    import pairing_amd.device as pdev
    from pairing_amd._native import Groth16Pk, Groth16Vk
    z = lambda *s: np.zeros(s, np.uint64)  # noqa: E731
    ok = dict(alpha_g1=z(1, 13), beta_g2=z(1, 25), gamma_g2=z(1, 25), delta_g2=z(1, 25), ic=z(3, 13))
    for change, what in ((dict(alpha_g1=z(2, 13)), "alpha_g1"), (dict(beta_g2=z(1, 13)), "beta_g2"),
                         (dict(gamma_g2=z(2, 25)), "gamma_g2"), (dict(delta_g2=z(1, 24)), "delta_g2"),
                         (dict(ic=z(3, 12)), "ic"), (dict(ic=z(0, 13)), "n_public"),
                         (dict(ic=z(pa._native.GROTH16_VK_MAX_INPUTS + 2, 13)), "n_public")):
        with pytest.raises(ValueError, match=what):
            pa.groth16_vk(**dict(ok, **change))
    vk = Groth16Vk(P(1), 3, owns=False)   # a live-looking handle: every error comes before a native call
    pk = Groth16Pk(P(1), 3, 5, 2, 7, owns=False)
    assert vk.n_inputs == 2
    proofs, x = z(2, 51), z(4, 4)
    for args, kw, what in (((pk, proofs, x), {}, "groth16_vk"), ((object(), proofs, x), {}, "groth16_vk"),
                           ((vk, z(2, 50), x), {}, "shape"), ((vk, proofs, z(4, 5)), {}, "shape"),
                           ((vk, proofs, z(3, 4)), {}, "input rows"), ((vk, proofs, x), dict(stride=1), "stride"),
                           ((vk, proofs, z(4, 4)), dict(stride=3), "input rows"),
                           ((vk, proofs, x), dict(montgomery=1), "montgomery")):
        with pytest.raises(ValueError, match=what):
            pa.groth16_verify(*args, **kw)
    for args, kw, what in (((pk, z(2, 192).astype(np.uint8), x), {}, "groth16_vk"),
                           ((vk, np.zeros((2, 191), np.uint8), x), {}, "192"),
                           ((vk, np.zeros((2, 192), np.uint8), z(3, 4)), {}, "input rows"),
                           ((vk, np.zeros((2, 192), np.uint8), x), dict(stride=0), "stride")):
        with pytest.raises(ValueError, match=what):
            pa.groth16_verify_encoded(*args, **kw)
    for args, kw, what in (((pk, x), {}, "groth16_vk"), ((vk, z(4, 3)), {}, "shape"), ((vk, x), dict(k=3), "input rows"),
                           ((vk, x), dict(stride=1), "stride"), ((vk, x), dict(k=-1), "negative")):
        with pytest.raises(ValueError, match=what):
            pa.groth16_input_sum(*args, **kw)
    t = lambda *s: torch.zeros(*s, dtype=torch.int64)  # noqa: E731
    b = lambda n: torch.zeros(n, dtype=torch.uint8)  # noqa: E731
    for args, kw, what in (((pk, t(2, 51), t(4, 4), b(2), b(8)), {}, "groth16_vk"),
                           ((vk, t(2, 51), t(3, 4), b(2), b(8)), {}, "input rows"),
                           ((vk, t(2, 51), t(4, 4), b(2), b(8)), dict(stride=1), "stride"),
                           ((vk, t(2, 51), t(4, 4), b(1), b(8)), {}, "needs 2"),
                           ((vk, t(2, 51), t(4, 4), b(2), b(8)), dict(gt=t(1, 72)), "needs 2")):
        with pytest.raises(ValueError, match=what):
            pdev.groth16_verify(*args, **kw)
    with pytest.raises(ValueError, match="192"):
        pdev.groth16_verify_encoded(vk, torch.zeros(2, 191, dtype=torch.uint8), t(4, 4), b(2), b(6), b(8))
    with pytest.raises(ValueError, match="groth16_vk"):
        pdev.groth16_verify_workspace(pk, 1, "cpu")
    with pytest.raises(ValueError, match="negative"):
        pdev.groth16_verify_workspace(vk, -1, "cpu")
    with pytest.raises(ValueError, match="needs 3"):
        pdev.groth16_input_sum(vk, t(6, 4), 3, t(2, 13))
    vk.close()
    with pytest.raises(ValueError, match="close"):
        pa.groth16_verify(vk, proofs, x)


# ---------------- GPU: the public-input sum alone ----------------

def _sum_inputs(g, l, k=5):
    """k = 5 input vectors: all 0, all 1, all r - 1, two random"""
    return [[0] * l, [1] * l, [R_ORDER - 1] * l] + [G.rand_fr(g, l) for _ in range(k - 3)]


def _check_sum(gpu, oracle, ic, inputs):
    """both input formats, end to end and at a larger stride with junk between the vectors"""
    k, l = len(inputs), ic.shape[0] - 1
    want = V.ref_input_sum(oracle, ic, inputs)
    flat = [x for row in inputs for x in row]
    zero = np.zeros((1, 13), np.uint64)
    with gpu.groth16_vk(zero, np.zeros((1, 25), np.uint64), np.zeros((1, 25), np.uint64), np.zeros((1, 25), np.uint64),
                        ic) as vk:
        assert (vk.n_public, vk.n_inputs) == (l + 1, l) and vk.bytes > l * 480000
        for montgomery, rows in ((True, rows_of(flat)), (False, small_scalars(flat))):
            got = gpu.groth16_input_sum(vk, rows, k=k, montgomery=montgomery)
            np.testing.assert_array_equal(got, want)
            if l:
                stride = l + 3
                wide = np.full((k * stride, 4), 0xfeedfacecafebeef, np.uint64)
                for j in range(k):
                    wide[j * stride:j * stride + l] = rows[j * l:(j + 1) * l]
                # the last vector's junk is not part of the buffer: the call needs (k - 1) stride + l rows only
                wide = np.ascontiguousarray(wide[:(k - 1) * stride + l])
                np.testing.assert_array_equal(gpu.groth16_input_sum(vk, wide, k=k, stride=stride, montgomery=montgomery),
                                              want)
    return want


@pytest.mark.gpu
@pytest.mark.parametrize("l", [0, 1, 3, 17])
def test_input_sum_bit_exact(gpu, oracle, l):
    g = rng(5200 + l)
    ic = oracle.g1_mul_generator(small_scalars(G.rand_fr(g, l + 1)))
    want = _check_sum(gpu, oracle, ic, _sum_inputs(g, l))
    if l == 0:
        assert (want == ic[0]).all()


@pytest.mark.gpu
def test_input_sum_special_bases(gpu, oracle):
    g = rng(5210)
    base = oracle.g1_mul_generator(small_scalars(G.rand_fr(g, 4)))
    inf = set_infinity(np.zeros((1, 13), np.uint64), [0])
    # an ic entry at infinity
    ic = base.copy()
    ic[2] = inf[0]
    _check_sum(gpu, oracle, ic, _sum_inputs(g, 3))
    # an ic entry on the curve but outside G1
    pts, truth = D.subgroup_points(1, seed=5211, n=1)
    assert not truth[0]
    ic = base.copy()
    ic[1] = np.array(D.aff_record(1, pts[0]), np.uint64)
    _check_sum(gpu, oracle, ic, _sum_inputs(g, 3))
    # ic[0] at infinity, ic[1] == ic[2], equal inputs: the second addition doubles
    same = [[x, x, y] for x, y in zip([1, R_ORDER - 1] + G.rand_fr(g, 3), [0] + G.rand_fr(g, 4))]
    ic = base.copy()
    ic[0], ic[2] = inf[0], base[1]
    _check_sum(gpu, oracle, ic, same)
    # ic[2] == -ic[1], equal inputs: the sum passes through infinity before the third term
    ic = base.copy()
    ic[0], ic[2] = inf[0], G.negate_g1(base[1:2])[0]
    want = _check_sum(gpu, oracle, ic, same)
    np.testing.assert_array_equal(want[0], inf[0])    # x_3 = 0 there: infinity is also the result
    # all inputs zero and ic[0] at infinity
    ic = base.copy()
    ic[0] = inf[0]
    want = _check_sum(gpu, oracle, ic, [[0, 0, 0]] * 5)
    np.testing.assert_array_equal(want, np.repeat(inf, 5, axis=0))


# ---------------- GPU: verify ----------------

# (k, PA_G16V_SHARED_MIN or None for the library's own).  Below the bound all 3 k pairs run through the e(P, Q)
# Miller loops, whose kernels change where 3 k crosses 768 and 4096 pairs (k = 256 | 257 and 1365 | 1366), and the
# final exponentiation's where k crosses 768; from the bound on the (A, B) loops change at k = 768 | 769.  The
# bound itself is forced down to 4 (one below, at, one above); 65 is one proof past a wave.
VERIFY_CASES = [(1, None), (2, None), (3, None), (65, None), (255, None), (256, None), (257, None), (768, None),
                (769, None), (1365, None), (1366, None),
                (3, 4), (4, 4), (5, 4),
                (1, 1), (2, 1), (65, 1), (767, 1), (768, 1), (769, 1)]


@pytest.mark.gpu
@pytest.mark.parametrize("k,shared_min", VERIFY_CASES)
def test_verify_valid_and_gt_bit_exact(gpu, pool, monkeypatch, k, shared_min):
    if shared_min is None:
        monkeypatch.delenv(KNOB, raising=False)
        with open(HEADER) as f:   # the library's own bound is above every k here: these run the 3 k-pair path
            assert k < int(re.search(r"#define PA_GROTH16_VERIFY_SHARED_MIN (\d+)", f.read()).group(1))
    else:
        monkeypatch.setenv(KNOB, str(shared_min))
    proofs, mont, repr_rows, gt, valid = pool.batch(k, shift=k)
    with gpu.groth16_vk(*pool.vk.args()) as vk:
        got_valid, got_gt = gpu.groth16_verify(vk, proofs, mont, return_gt=True)
        assert got_valid.dtype == bool and got_valid.shape == (k,) and got_gt.shape == (k, 72)
        np.testing.assert_array_equal(got_valid, valid)
        np.testing.assert_array_equal(got_gt, gt)
        # no gt requested, and repr inputs
        np.testing.assert_array_equal(gpu.groth16_verify(vk, proofs, repr_rows, montgomery=False), valid)
    if k >= 9:
        assert valid.any() and not valid.all()


@pytest.mark.gpu
def test_both_paths_agree_and_k_zero(gpu, pool, monkeypatch):
    proofs, mont, _, gt, valid = pool.batch(9)
    with gpu.groth16_vk(*pool.vk.args()) as vk:
        out = []
        for bound in ("1000000", "1"):
            monkeypatch.setenv(KNOB, bound)
            out.append(gpu.groth16_verify(vk, proofs, mont, return_gt=True))
        np.testing.assert_array_equal(out[0][0], out[1][0])
        np.testing.assert_array_equal(out[0][1], out[1][1])
        np.testing.assert_array_equal(out[0][1], gt)
        assert gpu.groth16_verify(vk, proofs[:0], mont[:0]).shape == (0,)
        v, st = gpu.groth16_verify_encoded(vk, np.zeros((0, 192), np.uint8), mont[:0])
        assert v.shape == (0,) and st.shape == (0, 3)


def _dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a).view(np.int64)).to("cuda:0")


@pytest.mark.gpu
def test_the_knob_selects_the_miller_loop_composition(gpu, pool, monkeypatch):
    """gt and valid cannot tell the two compositions apart, the workspace can: its Q array (at the first
    multiple of 256 bytes behind the 3 k G1 records of P, include/pairing_amd.h) gets -gamma and -delta k
    times behind B only on the 3 k-pair path"""
    import torch
    import pairing_amd.device as pdev
    k = 5
    proofs, mont, _, gt, valid = pool.batch(k)
    q_at = (3 * k * 104 + 255) // 256 * 256
    neg = np.concatenate([np.repeat(V.negate_g2(pool.vk.gamma_g2), k, axis=0),
                          np.repeat(V.negate_g2(pool.vk.delta_g2), k, axis=0)])
    with gpu.groth16_vk(*pool.vk.args()) as vk:
        Pr, X = _dev(proofs), _dev(mont)
        for bound, pairs3k in ((None, True), (str(k + 1), True), (str(k), False), ("1", False)):
            if bound is None:
                monkeypatch.delenv(KNOB, raising=False)
            else:
                monkeypatch.setenv(KNOB, bound)
            ws = pdev.groth16_verify_workspace(vk, k, "cuda:0")
            ws.fill_(0x5a)
            out = torch.zeros(k, dtype=torch.uint8, device="cuda:0")
            pdev.groth16_verify(vk, Pr, X, out, ws)
            torch.cuda.synchronize()
            assert out.cpu().tolist() == valid.astype(int).tolist()
            q = ws[q_at:q_at + 3 * k * 200].cpu().numpy().view(np.uint64).reshape(3 * k, 25)
            np.testing.assert_array_equal(q[:k], proofs[:, 13:38])
            if pairs3k:
                np.testing.assert_array_equal(q[k:], neg)
            else:
                assert (q[k:] == 0x5a5a5a5a5a5a5a5a).all()


@pytest.mark.gpu
def test_prove_then_verify_on_the_device_from_the_witness_buffer(gpu, oracle, real):
    """groth16_prove and groth16_verify back to back in HBM, no oracle in between: the verifier reads its
    inputs from the prover's witness buffer (witness + 1, stride n_vars)"""
    import torch
    import pairing_amd.device as pdev
    mats, w, key, vkp = real
    g = rng(5300)
    k, n_vars = 4, key.n_vars
    spoiled = list(w)
    spoiled[9] = (spoiled[9] + 5) % R_ORDER
    ws = [w, w, spoiled, w]
    pk = gpu.groth16_pk(*key.points(oracle))
    sysm = gpu.r1cs(*(G.csr(m) for m in mats), 30, n_vars)
    dom = gpu.fr_ntt_domain(key.log_n)
    vk = gpu.groth16_vk(*vkp.args())
    try:
        W = _dev(rows_of([v for x in ws for v in x]))
        R, S = _dev(rows_of(G.rand_fr(g, k))), _dev(rows_of(G.rand_fr(g, k)))
        proofs = pdev.empty_records(k, 51, "cuda:0")
        valid = torch.full((k + 1,), 7, dtype=torch.uint8, device="cuda:0")
        pdev.groth16_prove(pk, sysm, dom, W, R, S, proofs, pdev.groth16_prove_workspace(pk, sysm, k, "cuda:0"))
        pdev.groth16_verify(vk, proofs, W[1:], valid, pdev.groth16_verify_workspace(vk, k, "cuda:0"), stride=n_vars)
        torch.cuda.synchronize()
        assert valid.cpu().tolist() == [1, 1, 0, 1, 7]
    finally:
        for x in (pk, sysm, dom, vk):
            x.close()


@pytest.mark.gpu
def test_encoded_proofs_status_and_valid(gpu, oracle, pool):
    # the pool's proofs whose points are all in their groups, then three records spoiled on the wire
    idx = [0, 1, 2, 3, 4, 5, 6, 7]
    enc = V.encode_proofs(pool.proofs[idx])
    good = enc[0]
    flipped = None
    for bit in range(8):                              # a bit of A's x that leaves no point on the curve
        t = good.copy()
        t[47] ^= 1 << bit
        if oracle.decode(1, t[None, :48].copy(), True)[1][0] == D.NOT_ON_CURVE:
            flipped = t
            break
    assert flipped is not None
    b_out = good.copy()
    b_out[48:144] = np.frombuffer([c for c in D.g2_cases(True) if c[1] == D.NOT_IN_SUBGROUP][0][0], np.uint8)
    no_flag = good.copy()
    no_flag[0] &= 0x7f
    data = np.ascontiguousarray(np.concatenate([enc, flipped[None], b_out[None], no_flag[None]]))
    k = data.shape[0]
    inputs = np.ascontiguousarray(np.concatenate([pool.mont[idx].reshape(-1, 4)] + [pool.mont[0]] * 3))
    want_status = V.decode_status(oracle, data)
    assert not want_status[:8].any()
    assert want_status[8:].tolist() == [[D.NOT_ON_CURVE, 0, 0], [0, D.NOT_IN_SUBGROUP, 0], [D.COMPRESSION_MODE, 0, 0]]
    with gpu.groth16_vk(*pool.vk.args()) as vk:
        valid, status, gt = gpu.groth16_verify_encoded(vk, data, inputs, return_gt=True)
        np.testing.assert_array_equal(status, want_status)
        np.testing.assert_array_equal(valid, np.concatenate([pool.valid[idx], [False] * 3]))
        np.testing.assert_array_equal(gt[:8], pool.gt[idx])
        v2, s2 = gpu.groth16_verify_encoded(vk, data, inputs)
        np.testing.assert_array_equal(v2, valid)
        np.testing.assert_array_equal(s2, status)
    assert k == 11


@pytest.mark.gpu
def test_device_entries_on_a_stream_and_every_verify_error(gpu, oracle, pool, monkeypatch):
    import torch
    import pairing_amd.device as pdev
    from pairing_amd import _native
    monkeypatch.delenv(KNOB, raising=False)
    k = 5
    proofs, mont, _, gt, valid = pool.batch(k)
    s = torch.cuda.Stream()
    vk = gpu.groth16_vk(*pool.vk.args())
    try:
        sizes = [vk.verify_workspace_bytes(n) for n in (0, 1, 2, 3, 64, 65, 1000, 1001, 1 << 14)]
        assert sizes == sorted(sizes) and sizes[0] > 0 and sizes[1] < sizes[-1]     # monotone in k
        ws = pdev.groth16_verify_workspace(vk, k, "cuda:0")
        assert ws.numel() == vk.verify_workspace_bytes(k)
        Pr, X = _dev(proofs), _dev(mont)
        fill = 0x5a5a5a5a5a5a5a5a
        out_gt = _dev(np.full((k + 1, 72), fill, np.uint64))
        out_valid = torch.full((k + 1,), 9, dtype=torch.uint8, device="cuda:0")
        torch.cuda.synchronize()
        with torch.cuda.stream(s):
            pdev.groth16_verify(vk, Pr, X, out_valid, ws, gt=out_gt, stream=s)
        s.synchronize()
        host = out_gt.cpu().numpy().view(np.uint64)
        np.testing.assert_array_equal(host[:k], gt)
        assert (host[k] == fill).all()
        assert out_valid.cpu().tolist() == valid.astype(int).tolist() + [9]
        np.testing.assert_array_equal(Pr.cpu().numpy().view(np.uint64), proofs)
        # the encoded entry and the sum alone, on the same stream
        data = _dev_bytes(V.encode_proofs(proofs[:k]))
        st = torch.full((k, 3), 9, dtype=torch.uint8, device="cuda:0")
        v2 = torch.zeros(k, dtype=torch.uint8, device="cuda:0")
        sums = pdev.empty_records(k, 13, "cuda:0")
        sum_ws = torch.empty(vk.input_sum_workspace_bytes(k), dtype=torch.uint8, device="cuda:0")
        with torch.cuda.stream(s):
            pdev.groth16_verify_encoded(vk, data, X, v2, st, ws, stream=s)
            pdev.groth16_input_sum(vk, X, k, sums, sum_ws, stream=s)
        s.synchronize()
        # proof 8 of the pool (B outside G2) is not among the first five: all decode
        assert not st.cpu().numpy().any() and v2.cpu().tolist() == valid.astype(int).tolist()
        np.testing.assert_array_equal(sums.cpu().numpy().view(np.uint64),
                                      V.ref_input_sum(oracle, pool.vk.ic, [pool.inputs[j] for j in range(k)]))
        with pytest.raises(ValueError, match="workspace"):
            pdev.groth16_verify(vk, Pr, X, out_valid, ws[:-1], stream=s)

        # what the C entries refuse before anything runs
        lib = _native._lib
        fresh = torch.full((k,), 9, dtype=torch.uint8, device="cuda:0")
        p = lambda t: ctypes.c_void_p(t.data_ptr())  # noqa: E731
        sp = ctypes.c_void_p(s.cuda_stream)
        h = vk.handle()
        good = (h, p(Pr), p(X), 2, 1, k, p(fresh), None, p(ws), ws.numel(), sp)

        def change(**kw):
            names = ("vk", "proofs", "inputs", "stride", "flags", "k", "valid", "gt", "ws", "ws_bytes", "stream")
            return tuple(kw.get(n, v) for n, v in zip(names, good))
        # pa_last_error names each case: the message of this very call, not one left by an earlier failure
        NULL, STRIDE, FLAGS, WS, BATCH = "null pointer", "input_stride", "flag", "workspace smaller", "split"

        def refused(entry, args, message, what):
            assert entry(*args) == -1, what
            assert message in lib.pa_last_error().decode(), (what, lib.pa_last_error())
        cases = {
            "no key": (change(vk=None), NULL), "no proofs": (change(proofs=None), NULL),
            "no inputs": (change(inputs=None), NULL), "no valid": (change(valid=None), NULL),
            "no workspace": (change(ws=None), NULL),
            "input_stride below l": (change(stride=1), STRIDE), "unknown flag bits": (change(flags=2), FLAGS),
            "workspace one byte short": (change(ws_bytes=ws.numel() - 1), WS + " than pa_groth16_verify_workspace_bytes"),
            "a batch over the limit": (change(k=(1 << 24) + 1), BATCH),
        }
        if torch.cuda.device_count() > 1:
            cases["a stream on another device"] = (change(
                stream=ctypes.c_void_p(torch.cuda.Stream(device="cuda:1").cuda_stream)), "another device")
        for what, (args, message) in cases.items():
            refused(lib.pa_groth16_verify_device, args, message, what)
        enc_good = (h, p(data), p(X), 2, 1, k, p(fresh), p(st), None, p(ws), ws.numel(), sp)
        for what, i, v, message in (("no key", 0, None, NULL), ("no records", 1, None, NULL), ("no inputs", 2, None, NULL),
                                    ("stride", 3, 0, STRIDE), ("flags", 4, 4, FLAGS), ("no valid", 6, None, NULL),
                                    ("no status", 7, None, NULL), ("no workspace", 9, None, NULL),
                                    ("short workspace", 10, ws.numel() - 1, WS)):
            refused(lib.pa_groth16_verify_encoded_device, enc_good[:i] + (v,) + enc_good[i + 1:], message, what)
        sum_good = (h, p(X), 2, 1, k, p(sums), p(sum_ws), sum_ws.numel(), sp)
        for what, i, v, message in (("no key", 0, None, NULL), ("no inputs", 1, None, NULL), ("stride", 2, 1, STRIDE),
                                    ("flags", 3, 8, FLAGS), ("no out", 5, None, NULL), ("no workspace", 6, None, NULL),
                                    ("short workspace", 7, sum_ws.numel() - 1,
                                     WS + " than pa_groth16_vk_input_sum_workspace_bytes")):
            refused(lib.pa_groth16_vk_input_sum_device, sum_good[:i] + (v,) + sum_good[i + 1:], message, what)
        assert lib.pa_groth16_verify_workspace_bytes(h, (1 << 24) + 1) == 0
        assert lib.pa_groth16_verify_device(*change(k=0, proofs=None, valid=None, ws=None, ws_bytes=0)) == 0   # k = 0
        torch.cuda.synchronize()
        assert (fresh.cpu().numpy() == 9).all()
    finally:
        vk.close()


def _dev_bytes(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a, np.uint8)).to("cuda:0")
