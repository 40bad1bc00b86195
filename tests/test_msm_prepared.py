"""G1 multiexp over prepared bases (pa_g1_msm_bases, include/pairing_amd.h).

The bases are checked for G1 membership and converted once; with every base
in G1 a multiexp splits each scalar s = q x^2 + rem (glv_split.h) and runs the
Pippenger pipeline over the 2m virtual terms rem * P_i + q * (-phi(P_i)) in
ceil(130 / c) windows (kernels_msm.hip, k_msm_digits_glv), otherwise the
257-bit pipeline over the prepared rows.  Either way the sum is compared as a
point (PartialEq, ec.rs:45-85) with the oracle's sum of CurveAffine::mul terms,
and at 2^14 terms with the identity sum s_i (a_i G) = ((sum s_i a_i) mod r) G."""
import ctypes
import os
import re

import numpy as np
import pytest

import decode_cases as D
from helpers import R_ORDER, from_limbs, random_scalars, rng, set_infinity, small_scalars

NT = 8
ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
HEADER = os.path.join(ROOT, "include", "pairing_amd.h")
SPLIT_SRC = os.path.join(ROOT, "pairing_amd", "csrc", "glv_split.h")
X2 = 0xd201000000010000 ** 2

NEW_SYMBOLS = ("pa_g1_msm_bases_prepare", "pa_g1_msm_bases_prepare_device", "pa_g1_msm_bases_len",
               "pa_g1_msm_bases_in_subgroup", "pa_g1_msm_bases_free", "pa_g1_multiexp_prepared_workspace_bytes",
               "pa_g1_multiexp_prepared_device", "pa_g1_multiexp_prepared")


def edge_scalars():
    return small_scalars([0, 1, 2, 3, R_ORDER - 1, R_ORDER, R_ORDER + 1, (1 << 256) - 1, 1 << 255, 0xffff])


def wide_scalars(g, n):
    """n 256-bit FrRepr values with the top bit set: all >= r"""
    return small_scalars([int.from_bytes(g.bytes(32), "little") | 1 << 255 for _ in range(n)])


def dressed(oracle, n, seed):
    """test_g1_multiexp_matches_oracle's inputs: from 17 terms up the ten edge
    scalars, an infinity base, two equal bases with equal scalars, P with -P"""
    g = rng(seed)
    p = oracle.g1_mul_generator(random_scalars(g, n), NT)
    s = random_scalars(g, n)
    if n >= 17:
        s[:10] = edge_scalars()
        set_infinity(p, [11])
        p[12] = p[13]
        s[12] = s[13]
        p[14] = p[15]
        p[14, 6:12] = oracle.fq_sub(np.zeros((1, 6), np.uint64), p[15:16, 6:12])[0]
        s[14] = s[15]
    return p, s


# ---------------- CPU: the surface ----------------

def test_new_symbols_are_declared_and_bound():
    from pairing_amd import _native
    with open(HEADER) as f:
        declared = set(re.findall(r"^\s*(?:const\s+)?\w+\s*\*?\s*(pa_\w+)\s*\(", f.read(), flags=re.M))
    for name in NEW_SYMBOLS:
        assert name in declared, name
        assert name in _native._SIGS, name
        assert getattr(_native._lib, name).argtypes == _native._SIGS[name]
    # size_t travels as c_size_t, not ctypes' default int
    assert _native._lib.pa_g1_msm_bases_len.restype is ctypes.c_size_t
    assert _native._lib.pa_g1_multiexp_prepared_workspace_bytes.restype is ctypes.c_size_t
    assert _native._SIGS["pa_g1_multiexp_prepared_device"][2] is ctypes.c_size_t
    assert _native._SIGS["pa_g1_msm_bases_prepare"][1] is ctypes.c_size_t


def borrowed(length):
    """a live-looking object over a handle nobody may dereference (the checks
    under test come before any native call) and nobody frees"""
    from pairing_amd import G1MsmBases
    return G1MsmBases(ctypes.c_void_p(8), length, True, owns=False)


def test_python_layer_rejects_bad_shapes():
    import pairing_amd as pa
    with pytest.raises(ValueError):
        pa.g1_msm_prepare(np.zeros((3, 12), np.uint64))
    with pytest.raises(ValueError):
        pa.g1_multiexp_prepared(borrowed(5), np.zeros((3, 5), np.uint64))
    with pytest.raises(ValueError):
        pa.g1_multiexp_prepared(object(), np.zeros((3, 4), np.uint64))


def test_python_layer_rejects_too_many_scalars_and_closed_objects():
    import pairing_amd as pa
    b = borrowed(5)
    assert b.len == 5 and len(b) == 5 and b.in_subgroup and not b.closed
    with pytest.raises(ValueError):
        pa.g1_multiexp_prepared(b, np.zeros((6, 4), np.uint64))
    b.close()
    b.close()   # idempotent
    assert b.closed
    with pytest.raises(ValueError):
        pa.g1_multiexp_prepared(b, np.zeros((5, 4), np.uint64))
    with pytest.raises(ValueError):
        b.handle()
    with pytest.raises(ValueError):
        b.check_terms(0)


# ---------------- CPU: the digits of both halves ----------------

def _barrett_m():
    with open(SPLIT_SRC) as f:
        m = re.search(r"kGlvBarrett\[3\]\s*=\s*\{([^}]*)\}", f.read())
    ws = [int(t.strip().rstrip("ull").rstrip("u"), 0) for t in m.group(1).split(",")]
    return sum(w << (64 * i) for i, w in enumerate(ws))


def _split(s, m):
    q = ((s >> 127) * m) >> 129
    return q, s - q * X2


def _digits(v, c):
    """k_msm_digits_glv's recoding: ceil(130 / c) signed c-bit digits, |d| <= 2^(c-1)"""
    windows = (130 + c - 1) // c
    half = 1 << (c - 1)
    out, carry = [], 0
    for w in range(windows):
        raw = carry + ((v >> (c * w)) & ((1 << c) - 1))
        carry = 1 if raw > half else 0
        out.append(raw - (1 << c) if raw > half else raw)
    return out, carry


def test_barrett_halves_recode_into_130_bit_windows():
    m = _barrett_m()
    assert m == (1 << 256) // X2
    edges = [0, 1, X2 - 1, X2, X2 + 1, 2 * X2 - 1, (1 << 128) - 1, 1 << 128, (1 << 129) * X2 // 2,
             R_ORDER - 1, R_ORDER, (1 << 255) - 1, (1 << 256) - 1, ((1 << 256) - 1) // X2 * X2,
             ((1 << 256) - 1) // X2 * X2 - 1]
    g = np.random.default_rng(182)
    rand = [int.from_bytes(g.bytes(32), "little") for _ in range(3000)]
    for s in edges + rand:
        q, rem = _split(s, m)
        assert q * X2 + rem == s
        assert 0 <= rem < (1 << 129) and 0 <= q < (1 << 129)
        for c in range(4, 17):
            for v in (q, rem):
                ds, carry = _digits(v, c)
                assert carry == 0 and len(ds) == -(-130 // c)
                assert all(abs(d) <= 1 << (c - 1) for d in ds)
                assert sum(d << (c * w) for w, d in enumerate(ds)) == v


# ---------------- GPU ----------------

@pytest.fixture(scope="module")
def base300(oracle):
    """300 dressed subgroup bases and three scalar sets with the oracle's sums"""
    p, s0 = dressed(oracle, 300, 350)
    g = rng(351)
    sets = [s0, random_scalars(g, 300), random_scalars(g, 300)]
    sets[2][:10] = edge_scalars()[::-1]
    sets[2][100:200] = wide_scalars(g, 100)
    return p, sets, [oracle.g1_multiexp(p, s, NT) for s in sets]


@pytest.mark.gpu
@pytest.mark.parametrize("n", [0, 1, 2, 3, 17, 300, 4099])
def test_prepared_multiexp_matches_oracle(gpu, oracle, n):
    # 4099: 8198 virtual terms, c = 10, the bucketing sort's second pass
    p, s = dressed(oracle, n, 250 + n)
    with gpu.g1_msm_prepare(p) as b:
        assert b.len == n and b.in_subgroup
        got = gpu.g1_multiexp_prepared(b, s)
    assert oracle.g1_eq(got, oracle.g1_multiexp(p, s, NT)).all()


@pytest.mark.gpu
def test_one_object_many_scalar_sets_and_prefixes(gpu, oracle, base300):
    p, sets, sums = base300
    b = gpu.g1_msm_prepare(p)
    try:
        assert b.in_subgroup
        for s, exp in zip(sets, sums):
            assert oracle.g1_eq(gpu.g1_multiexp_prepared(b, s), exp).all()
        got = gpu.g1_multiexp_prepared(b, sets[1][:200])
        assert oracle.g1_eq(got, oracle.g1_multiexp(p[:200], sets[1][:200], NT)).all()
        zero = gpu.g1_multiexp_prepared(b, sets[1][:0])
        assert oracle.g1_eq(zero, oracle.g1_multiexp(p[:0], sets[1][:0])).all()
    finally:
        b.close()
    with pytest.raises(ValueError):
        gpu.g1_multiexp_prepared(b, sets[0])


@pytest.mark.gpu
def test_prepared_multiexp_deterministic(gpu, oracle):
    g = rng(380)
    n = 5000
    p = oracle.g1_mul_generator(random_scalars(g, n), NT)
    s = random_scalars(g, n)
    s[100:300] = s[7]
    with gpu.g1_msm_prepare(p) as b:
        a1 = gpu.g1_multiexp_prepared(b, s)
        a2 = gpu.g1_multiexp_prepared(b, s)
    np.testing.assert_array_equal(a1, a2)
    assert oracle.g1_eq(a1, oracle.g1_multiexp(p, s, NT)).all()


@pytest.mark.gpu
def test_prepared_multiexp_crowded_buckets(gpu, oracle):
    """Every scalar equal but a short run: both halves crowd one bucket per
    window (9000 items over more than 128 chunks: k_msm_long_fix)"""
    g = rng(395)
    n = 9000
    p = oracle.g1_mul_generator(random_scalars(g, n), NT)
    s = np.repeat(random_scalars(g, 1), n, axis=0)
    s[n // 3:n // 3 + 50] = random_scalars(g, 1)
    set_infinity(p, [5, n // 2])
    with gpu.g1_msm_prepare(p) as b:
        assert b.in_subgroup
        got = gpu.g1_multiexp_prepared(b, s)
    assert oracle.g1_eq(got, oracle.g1_multiexp(p, s, NT)).all()


@pytest.mark.gpu
@pytest.mark.parametrize("kind", ["curve_point", "subgroup_plus_torsion"])
def test_fallback_for_a_base_outside_g1(gpu, oracle, base300, kind):
    pts, truth = D.subgroup_points(1, seed=371, n=1)   # [R, h R, r R, h R + r R, ...]
    idx = 0 if kind == "curve_point" else 3
    assert not truth[idx] and truth[1]
    p = base300[0].copy()
    p[137] = np.array(D.aff_record(1, pts[idx]), np.uint64)
    with gpu.g1_msm_prepare(p) as b:
        assert b.len == 300 and not b.in_subgroup
        for s in base300[1][:2]:
            assert oracle.g1_eq(gpu.g1_multiexp_prepared(b, s), oracle.g1_multiexp(p, s, NT)).all()
            assert oracle.g1_eq(gpu.g1_multiexp_prepared(b, s), gpu.g1_multiexp(p, s)).all()


@pytest.mark.gpu
def test_prepared_multiexp_identity_through_the_device_layer(gpu, oracle):
    # 2^14 terms: sum s_i (a_i G) == ((sum s_i a_i) mod r) G, a block of scalars >= r
    import torch
    import pairing_amd.device as pdev
    g = rng(390)
    n = 1 << 14
    a = random_scalars(g, n)
    s = random_scalars(g, n)
    s[500:600] = wide_scalars(g, 100)
    s[600:610] = small_scalars([R_ORDER + k for k in range(5)] + [(1 << 256) - 1 - k for k in range(5)])
    assert all(from_limbs(x) >= R_ORDER for x in s[500:610])
    # the bases a_i G made on the device (fixed-base comb + batch normalization, both checked elsewhere)
    gen = oracle.g1_from_affine(oracle.g1_mul_generator(small_scalars([1])))
    jac = pdev.empty_records(n, 18, "cuda")
    table, _ = pdev.g1_fixed_base_table(torch.from_numpy(gen.view(np.int64)).cuda())
    pdev.g1_fixed_base_mul(table, torch.from_numpy(a.view(np.int64)).cuda(), jac)
    pdev.g1_batch_normalization(jac)
    bases = torch.zeros((n, 13), dtype=torch.int64, device="cuda")
    bases[:, :12] = jac[:, :12]
    b = pdev.msm_prepare(bases)
    del bases, jac, table
    assert b.len == n and b.in_subgroup
    out = pdev.empty_records(1, 18, "cuda")
    pdev.multiexp_prepared(b, torch.from_numpy(s.view(np.int64)).cuda(), out,
                           pdev.multiexp_prepared_workspace(b, n, "cuda"))
    torch.cuda.synchronize()
    b.close()
    tot = sum(from_limbs(x) * from_limbs(y) for x, y in zip(a, s)) % R_ORDER
    np.testing.assert_array_equal(oracle.g1_into_affine(out.cpu().numpy().view(np.uint64)),
                                  oracle.g1_mul_generator(small_scalars([tot])))


@pytest.mark.gpu
def test_device_entry_errors_are_codes_not_aborts(gpu, oracle, base300):
    import torch
    import pairing_amd.device as pdev
    from pairing_amd._native import _lib
    p, sets, sums = base300
    b = pdev.msm_prepare(torch.from_numpy(p.view(np.int64)).cuda())
    n = b.len
    s = torch.from_numpy(np.concatenate([sets[0], sets[0][:1]]).view(np.int64)).cuda()
    out = pdev.empty_records(1, 18, "cuda")
    ws = pdev.multiexp_prepared_workspace(b, n, "cuda")
    need = int(_lib.pa_g1_multiexp_prepared_workspace_bytes(b.handle(), n))
    assert 0 < need <= ws.numel()
    assert int(_lib.pa_g1_multiexp_prepared_workspace_bytes(b.handle(), n + 1)) == 0
    stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    args = (b.handle(), ctypes.c_void_p(s.data_ptr()))
    tail = (ctypes.c_void_p(out.data_ptr()), ctypes.c_void_p(ws.data_ptr()))
    assert _lib.pa_g1_multiexp_prepared_device(*args, n, *tail, need - 1, stream) < 0
    assert b"workspace" in _lib.pa_last_error()
    assert _lib.pa_g1_multiexp_prepared_device(*args, n + 1, *tail, ws.numel(), stream) < 0
    assert b"prepared bases" in _lib.pa_last_error()
    host_out = np.zeros((1, 18), np.uint64)
    hs = np.zeros((n + 1, 4), np.uint64)
    assert _lib.pa_g1_multiexp_prepared(b.handle(), hs.ctypes.data_as(ctypes.c_void_p), n + 1,
                                        host_out.ctypes.data_as(ctypes.c_void_p)) < 0
    # and the object still works
    pdev.multiexp_prepared(b, s[:n], out, ws)
    torch.cuda.synchronize()
    assert oracle.g1_eq(out.cpu().numpy().view(np.uint64), sums[0]).all()
    b.close()
