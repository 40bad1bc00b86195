"""The Groth16 aggregate check on the device (pa_groth16_verify_aggregate*,
pa_g1_multiexp_u128*, include/pairing_amd.h): k proofs under one key in one
randomised pairing product.  The P array (affine records), gt and valid are
canonical, so everything is compared bit for bit with
tests/groth16_aggregate_ref.py: Python integers for the weight sums, the
oracle's CurveAffine::mul / add_assign / into_affine for the points, its
pairing and Fq12 product for gt.

The verdict tests draw their proofs from test_groth16_verify's pool over the
real setup; a batch tiles the pool's proofs, each slot with its own weight."""
import ctypes
import os
import re

import numpy as np
import pytest

import decode_cases as D
import groth16_aggregate_ref as A
import groth16_ref as G
import groth16_verify_ref as V
import small_order_cases as SO
from helpers import R_ORDER, fq12_one, rng, set_infinity, small_scalars
from test_groth16_verify import pool, real, rows_of  # noqa: F401  (fixtures)

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
HEADER = os.path.join(ROOT, "include", "pairing_amd.h")
P, N, U = ctypes.c_void_p, ctypes.c_size_t, ctypes.c_uint
NEW_SIGS = {
    "pa_g1_multiexp_u128_workspace_bytes": [N],
    "pa_g1_multiexp_u128_device": [P, P, N, P, P, N, P],
    "pa_g1_multiexp_u128": [P, P, N, P],
    "pa_groth16_verify_aggregate_workspace_bytes": [P, N],
    "pa_groth16_verify_aggregate_device": [P, P, P, N, U, P, N, P, P, P, N, P],
    "pa_groth16_verify_aggregate": [P, P, P, N, U, P, N, P, P],
    "pa_groth16_verify_aggregate_encoded_device": [P, P, P, N, U, P, N, P, P, P, P, N, P],
    "pa_groth16_verify_aggregate_encoded": [P, P, P, N, U, P, N, P, P, P],
    "pa_groth16_verify_aggregate_points_device": [P, P, P, N, U, P, N, P, P, N, P],
    "pa_groth16_verify_aggregate_points": [P, P, P, N, U, P, N, P],
}
SIZE_T_RESULTS = ("pa_g1_multiexp_u128_workspace_bytes", "pa_groth16_verify_aggregate_workspace_bytes")
# rows per block of the weight sums' first stage (kGroth16WeightBlock, launch_groth16_aggregate.h)
WEIGHT_BLOCK = 256
INF1 = set_infinity(np.zeros((1, 13), np.uint64), [0])


# ---------------- CPU: the reference helper ----------------

def _valid_batch(pool, k):  # noqa: F811
    """k valid proofs (the pool's two, tiled) with their input lists"""
    idx = [j % 2 for j in range(k)]
    return np.ascontiguousarray(pool.proofs[idx]), [pool.inputs[j] for j in idx]


def test_reference_gives_one_on_valid_proofs_and_the_weighted_product(oracle, pool):  # noqa: F811
    """gt == one on real valid proofs, and gt == prod_j (gt_j / e(alpha, beta))^z_j with gt_j from ref_verify on a
    batch that holds a spoiled proof (every point of these proofs is in its group)"""
    g = rng(7100)
    proofs, inputs = _valid_batch(pool, 3)
    z = A.rand_z(g, 3)
    gt, valid = A.ref_aggregate(oracle, pool.vk, proofs, inputs, z)
    assert valid and (gt == fq12_one()).all()
    proofs = np.ascontiguousarray(pool.proofs[[0, 2, 1, 3]])
    inputs = [pool.inputs[j] for j in (0, 2, 1, 3)]
    z = [A.rand_z(g, 1)[0], 5, (1 << 128) - 1, 1 << 64]
    gt, valid = A.ref_aggregate(oracle, pool.vk, proofs, inputs, z)
    each, _ = V.ref_verify(oracle, pool.vk, proofs, inputs)
    inv_ab, ok = oracle.fq12_inverse(oracle.pairing(pool.vk.alpha_g1, pool.vk.beta_g2))
    assert ok[0]
    want = fq12_one()
    for j in range(4):
        want = oracle.fq12_mul(want, A.fq12_pow_int(oracle, oracle.fq12_mul(each[j:j + 1], inv_ab), z[j]))
    np.testing.assert_array_equal(gt, want)
    assert not valid


def test_reference_rejects_one_spoiled_proof(oracle, pool):  # noqa: F811
    g = rng(7101)
    proofs, inputs = _valid_batch(pool, 4)
    proofs[2] = pool.proofs[2]           # a spoiled witness
    z = [v | 1 for v in A.rand_z(g, 4)]
    gt, valid = A.ref_aggregate(oracle, pool.vk, proofs, inputs, z)
    assert not valid and gt.any() and not (gt == fq12_one()).all()
    z[2] = 0                             # dropped from the check
    assert A.ref_aggregate(oracle, pool.vk, proofs, inputs, z)[1]
    gt, valid = A.ref_aggregate(oracle, pool.vk, proofs[:0], [], [])
    assert valid and (gt == fq12_one()).all()


# ---------------- CPU: symbols and the Python layers ----------------

def test_aggregate_symbols_are_declared_exported_and_bound():
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
    import pairing_amd
    import pairing_amd.device as pdev
    for name in ("groth16_verify_aggregate", "groth16_verify_aggregate_encoded", "groth16_aggregate_points",
                 "g1_multiexp_u128"):
        assert name in pairing_amd.__all__ and hasattr(pairing_amd, name), name
    for name in ("groth16_verify_aggregate_workspace", "groth16_verify_aggregate", "groth16_verify_aggregate_encoded",
                 "groth16_aggregate_points", "multiexp_u128", "multiexp_u128_workspace"):
        assert hasattr(pdev, name), name
    with open(os.path.join(ROOT, "include", "pairing_amd.hpp")) as f:
        hpp = f.read()
    for method in ("verify_aggregate", "verify_aggregate_encoded", "aggregate_points", "g1_multiexp_u128"):
        assert re.search(r"\b%s\(" % method, hpp), method
    with open(os.path.join(ROOT, "pairing_amd", "Makefile")) as f:
        assert "lib/kernels_groth16_aggregate.o" in f.read()
    # what the entries refuse before any device call
    assert lib.pa_groth16_verify_aggregate_workspace_bytes(None, 1) == 0
    assert lib.pa_g1_multiexp_u128_workspace_bytes(0) == 0
    assert lib.pa_groth16_verify_aggregate(None, None, None, 0, 0, None, 1, None, None) == -1
    assert lib.pa_groth16_verify_aggregate_device(None, None, None, 0, 0, None, 1, None, None, None, 0, None) == -1
    assert lib.pa_groth16_verify_aggregate_encoded(None, None, None, 0, 0, None, 1, None, None, None) == -1
    assert lib.pa_groth16_verify_aggregate_encoded_device(None, None, None, 0, 0, None, 1, None, None, None, None, 0,
                                                          None) == -1
    assert lib.pa_groth16_verify_aggregate_points(None, None, None, 0, 0, None, 1, None) == -1
    assert lib.pa_groth16_verify_aggregate_points_device(None, None, None, 0, 0, None, 1, None, None, 0, None) == -1
    assert lib.pa_g1_multiexp_u128(None, None, 1, None) == -1
    assert lib.pa_g1_multiexp_u128_device(None, None, 1, None, None, 0, None) == -1


def test_multiexp_u128_workspace_never_decreases_with_n():
    """The aggregate entry's workspace query is monotone in k because every term of its layout is; the only
    term that is not linear in k is this one, which needs no device.  The plan of a single n shrinks in two
    places: where the window width changes (powers of two: fewer windows) and where the accumulation's chunk
    rises by one (every 65536 x parts items: with 10 windows of 13 bits and two parts first between n = 104857
    and 104858, then at 117965, 144180, 157287, ...).  The sweep crosses every width step up to 2^24 and the
    chunk steps below 160000 one n at a time."""
    from pairing_amd import _native
    f = _native._lib.pa_g1_multiexp_u128_workspace_bytes
    assert f(0) == 0 and f(1) > 0
    dense = list(range(1, 20000)) + list(range(100000, 160000))
    edges = [n for lg in range(14, 25) for n in range((1 << lg) - 3, (1 << lg) + 4)]
    coarse = list(range(160000, (1 << 24) + 5000, 4099))
    ns = sorted(set(dense + edges + coarse))
    sizes = [int(f(n)) for n in ns]
    drops = [(a, b) for a, b, x, y in zip(ns, ns[1:], sizes, sizes[1:]) if y < x]
    assert not drops, drops[:10]
    assert sizes[-1] > sizes[0]
    for n in (104857, 117965, 144180, 157287, (1 << 12) - 1, (1 << 20) - 1):
        assert f(n + 1) >= f(n), n


def test_python_layers_check_aggregate_arguments_without_a_device():
    import torch
    import pairing_amd as pa
    import pairing_amd.device as pdev
    from pairing_amd._native import Groth16Pk, Groth16Vk
    z = lambda *s: np.zeros(s, np.uint64)  # noqa: E731
    vk = Groth16Vk(P(1), 3, owns=False)   # a live-looking handle: every error comes before a native call
    pk = Groth16Pk(P(1), 3, 5, 2, 7, owns=False)
    proofs, x, w = z(2, 51), z(4, 4), z(2, 2)
    for args, kw, what in (((pk, proofs, x, w), {}, "groth16_vk"), ((vk, z(2, 50), x, w), {}, "shape"),
                           ((vk, proofs, z(4, 5), w), {}, "shape"), ((vk, proofs, z(3, 4), w), {}, "input rows"),
                           ((vk, proofs, x, w), dict(stride=1), "stride"),
                           ((vk, proofs, x, z(2, 4)), {}, "128-bit"), ((vk, proofs, x, z(3, 2)), {}, "128-bit"),
                           ((vk, proofs, x, z(4)), {}, "128-bit"),
                           ((vk, proofs, x, w), dict(montgomery=1), "montgomery")):
        with pytest.raises(ValueError, match=what):
            pa.groth16_verify_aggregate(*args, **kw)
        with pytest.raises(ValueError, match=what):
            pa.groth16_aggregate_points(*args, **kw)
    enc = np.zeros((2, 192), np.uint8)
    for args, kw, what in (((pk, enc, x, w), {}, "groth16_vk"), ((vk, np.zeros((2, 191), np.uint8), x, w), {}, "192"),
                           ((vk, enc, z(3, 4), w), {}, "input rows"), ((vk, enc, x, w), dict(stride=0), "stride"),
                           ((vk, enc, x, z(2, 3)), {}, "128-bit")):
        with pytest.raises(ValueError, match=what):
            pa.groth16_verify_aggregate_encoded(*args, **kw)
    for bases, scalars, what in ((z(2, 12), z(2, 2), "shape"), (z(2, 13), z(2, 4), "shape"),
                                 (z(2, 13), z(3, 2), "differ in length")):
        with pytest.raises(ValueError, match=what):
            pa.g1_multiexp_u128(bases, scalars)
    t = lambda *s: torch.zeros(*s, dtype=torch.int64)  # noqa: E731
    b = lambda n: torch.zeros(n, dtype=torch.uint8)  # noqa: E731
    for args, kw, what in (((pk, t(2, 51), t(4, 4), t(2, 2), b(1), b(8)), {}, "groth16_vk"),
                           ((vk, t(2, 51), t(3, 4), t(2, 2), b(1), b(8)), {}, "input rows"),
                           ((vk, t(2, 51), t(4, 4), t(2, 2), b(1), b(8)), dict(stride=1), "stride"),
                           ((vk, t(2, 51), t(4, 4), t(2, 4), b(1), b(8)), {}, "128-bit"),
                           ((vk, t(2, 51), t(4, 4), t(3, 2), b(1), b(8)), {}, "128-bit"),
                           ((vk, t(2, 51), t(4, 4), t(4), b(1), b(8)), {}, "128-bit")):
        with pytest.raises(ValueError, match=what):
            pdev.groth16_verify_aggregate(*args, **kw)
    with pytest.raises(ValueError, match="128-bit"):
        pdev.groth16_aggregate_points(vk, t(2, 51), t(4, 4), t(2, 3), t(5, 13), b(8))
    with pytest.raises(ValueError, match="192"):
        pdev.groth16_verify_aggregate_encoded(vk, torch.zeros(2, 191, dtype=torch.uint8), t(4, 4), t(2, 2), b(1), b(6),
                                              b(8))
    with pytest.raises(ValueError, match="groth16_vk"):
        pdev.groth16_verify_aggregate_workspace(pk, 1, "cpu")
    with pytest.raises(ValueError, match="negative"):
        pdev.groth16_verify_aggregate_workspace(vk, -1, "cpu")
    vk.close()
    for fn, args in ((pa.groth16_verify_aggregate, (vk, proofs, x, w)), (pa.groth16_aggregate_points, (vk, proofs, x, w)),
                     (pa.groth16_verify_aggregate_encoded, (vk, enc, x, w))):
        with pytest.raises(ValueError, match="close"):
            fn(*args)


# ---------------- GPU: the short-scalar multiexp ----------------

def _ref_msm(oracle, bases, z):
    """(1, 13): into_affine(sum_i z_i * bases[i]) from the oracle's CurveAffine::mul"""
    if len(z) == 0:
        return oracle.g1_into_affine(A.g1_zero(oracle))
    return oracle.g1_into_affine(A.sum_rows(oracle, oracle.g1_affine_mul(bases, small_scalars(z), 8)))


def _check_msm(gpu, oracle, bases, z, against_plain=False):
    bases = np.ascontiguousarray(bases)
    got = gpu.g1_multiexp_u128(bases, A.z_rows(z))
    assert got.shape == (1, 18)
    np.testing.assert_array_equal(gpu.g1_into_affine(got), _ref_msm(oracle, bases, z))
    if against_plain:
        assert gpu.g1_eq(got, gpu.g1_multiexp(bases, small_scalars(z)))[0]


# 4097: one item past a sort tile of 4096; 4095 | 4099: the window width changes at 4096 terms (8 and 9 bits)
@pytest.mark.gpu
@pytest.mark.parametrize("n", [0, 1, 2, 33, 4095, 4097, 4099])
def test_multiexp_u128_bit_exact(gpu, oracle, n):
    g = rng(7200 + n)
    bases = oracle.g1_mul_generator(small_scalars(G.rand_fr(g, n)), 8) if n else np.zeros((0, 13), np.uint64)
    z = A.rand_z(g, n)
    for i, v in enumerate(A.Z_EDGES[:n]):
        z[(5 * i + 1) % n] = v
    _check_msm(gpu, oracle, bases, z, against_plain=True)
    if n:
        _check_msm(gpu, oracle, bases, [(1 << 128) - 1] * n)   # every top window carries


@pytest.mark.gpu
def test_multiexp_u128_special_bases(gpu, oracle):
    g = rng(7210)
    n = 33
    base = oracle.g1_mul_generator(small_scalars(G.rand_fr(g, n)), 8)
    z = A.rand_z(g, n)
    z[:6] = A.Z_EDGES
    # all bases equal and all scalars equal: every bucket addition doubles
    _check_msm(gpu, oracle, np.repeat(base[:1], n, axis=0), [z[7]] * n)
    _check_msm(gpu, oracle, np.repeat(base[:1], n, axis=0), z)
    # P with -P under the same scalar: cancellation, the whole sum is zero for an even count
    pm = base.copy()
    pm[1::2] = G.negate_g1(base[0:n - 1:2])
    zz = list(z)
    for i in range(1, n, 2):
        zz[i] = zz[i - 1]
    zz[n - 1] = 0
    _check_msm(gpu, oracle, pm, zz)
    # infinity among the bases
    some_inf = base.copy()
    set_infinity(some_inf, [0, 5, n - 1])
    _check_msm(gpu, oracle, some_inf, z)
    _check_msm(gpu, oracle, np.repeat(INF1, 3, axis=0), [1, 2, (1 << 128) - 1])
    # bases of order 3, 11 and 33 (on the curve, outside G1), alone and between subgroup points
    for name, m in SO.G1_ORDERS.items():
        T = SO.aff(1, SO.point(1, name))
        zs = [0, 1, m - 1, m, m + 1, 3 * m, (1 << 128) - 1, 1 << 127] + A.rand_z(g, 8)
        _check_msm(gpu, oracle, np.repeat(T[None], len(zs), axis=0), zs)
        mixed = base[:16].copy()
        mixed[::3] = T
        _check_msm(gpu, oracle, mixed, zs)


# ---------------- GPU: the P array ----------------

def _key(oracle, g, l, ic0_inf=False, alpha_inf=False):
    vals = [x or 1 for x in G.rand_fr(g, 4)]
    vk = V.vk_from_ints(oracle, *vals, G.rand_fr(g, l + 1))
    if ic0_inf:
        vk.ic[0] = INF1[0]
    if alpha_inf:
        vk.alpha_g1[0] = INF1[0]
    return vk


def _check_points(gpu, oracle, vkp, proofs, inputs, z):
    """both input formats, end to end and at a larger stride with junk between the vectors"""
    k, l = proofs.shape[0], vkp.n_inputs
    want = A.ref_points(oracle, vkp, proofs, inputs, z)
    # an FrRepr row is taken mod r, so it goes in as it is (values of r and above included); a Montgomery row
    # holds the value below r
    flat = [x for row in inputs for x in row]
    zr = A.z_rows(z)
    with gpu.groth16_vk(*vkp.args()) as vk:
        for montgomery, rows in ((True, rows_of([x % R_ORDER for x in flat])), (False, small_scalars(flat))):
            got = gpu.groth16_aggregate_points(vk, proofs, rows, zr, montgomery=montgomery)
            assert got.shape == (k + 3, 13)
            np.testing.assert_array_equal(got, want)
            if l and k:
                stride = l + 3
                wide = np.full((k * stride, 4), 0xfeedfacecafebeef, np.uint64)
                for j in range(k):
                    wide[j * stride:j * stride + l] = rows[j * l:(j + 1) * l]
                wide = np.ascontiguousarray(wide[:(k - 1) * stride + l])
                np.testing.assert_array_equal(
                    gpu.groth16_aggregate_points(vk, proofs, wide, zr, montgomery=montgomery, stride=stride), want)
    return want


def _inputs(g, k, l):
    """k input vectors: all 0, all r - 1, all 2^256 - 1, r and r + 1 alternating (the last two kinds are not below r:
    an FrRepr row is taken mod r), then random"""
    rows = [[0] * l, [R_ORDER - 1] * l, [(1 << 256) - 1] * l, [R_ORDER + (i & 1) for i in range(l)]]
    rows += [G.rand_fr(g, l) for _ in range(max(k - 4, 0))]
    return rows[:k]


# 2 * WEIGHT_BLOCK + 2: three blocks in the weight sums' first stage, the last with two rows
@pytest.mark.gpu
@pytest.mark.parametrize("l,k", [(0, 1), (0, 65), (1, 2), (1, 64), (3, 3), (3, 65), (3, 2 * WEIGHT_BLOCK + 2),
                                 (17, 1), (17, 3), (17, 64), (0, 0), (3, 0)])
def test_aggregate_points_bit_exact(gpu, oracle, l, k):
    g = rng(7300 + 1000 * l + k)
    vkp = _key(oracle, g, l)
    proofs = V.proof_rows(oracle, *[G.rand_fr(g, k) for _ in range(3)]) if k else np.zeros((0, 51), np.uint64)
    z = A.rand_z(g, k)
    for i, v in enumerate(A.Z_EDGES[:k]):
        z[(3 * i + 1) % k] = v
    want = _check_points(gpu, oracle, vkp, proofs, _inputs(g, k, l), z)
    if k == 0:
        np.testing.assert_array_equal(want, np.repeat(INF1, 3, axis=0))


@pytest.mark.gpu
def test_aggregate_points_special_cases(gpu, oracle):
    g = rng(7310)
    l, k = 3, 12
    proofs = V.proof_rows(oracle, *[G.rand_fr(g, k) for _ in range(3)])
    z = A.Z_EDGES + A.rand_z(g, k - 6)
    # A at infinity, A of order 3 under weights that are and are not multiples of 3, C of order 11
    proofs[6, :13] = INF1[0]
    o3, o11 = SO.aff(1, SO.point(1, "O3")), SO.aff(1, SO.point(1, "O11"))
    for j, zj in ((7, 3 * (z[7] >> 2)), (8, 3 * (z[8] >> 2) + 1), (9, 3), (10, 2)):
        proofs[j, :13] = o3
        z[j] = zj
    assert z[7] % 3 == 0 and z[8] % 3 == 1 and all(v < 1 << 128 for v in z)
    proofs[11, 38:51] = o11
    inputs = _inputs(g, k, l)
    want = _check_points(gpu, oracle, _key(oracle, g, l), proofs, inputs, z)
    np.testing.assert_array_equal(want[[0, 6, 7, 9]], np.repeat(INF1, 4, axis=0))   # z = 0, A = 0, 3 | z on order 3
    assert not want[8, 12] and not want[10, 12]
    # ic[0] and alpha at infinity; then every weight zero: the whole array is infinity
    vkp = _key(oracle, g, l, ic0_inf=True, alpha_inf=True)
    want = _check_points(gpu, oracle, vkp, proofs, inputs, z)
    np.testing.assert_array_equal(want[k + 2], INF1[0])
    want = _check_points(gpu, oracle, vkp, proofs, inputs, [0] * k)
    np.testing.assert_array_equal(want, np.repeat(INF1, k + 3, axis=0))
    # an ic entry of order 3 and alpha of order 11: the comb tables of points outside G1
    vkp = _key(oracle, g, l)
    vkp.ic[0], vkp.ic[2], vkp.alpha_g1[0] = o3, o3, o11
    _check_points(gpu, oracle, vkp, proofs, inputs, z)


# ---------------- GPU: verdict and gt ----------------

@pytest.mark.gpu
@pytest.mark.parametrize("k", [1, 3, 67, 300])
def test_aggregate_verdict_and_gt_bit_exact(gpu, oracle, pool, k):  # noqa: F811
    g = rng(7400 + k)
    good, inputs = _valid_batch(pool, k)
    z = [v | 1 for v in A.rand_z(g, k)]
    for i, v in enumerate(A.Z_EDGES[1:1 + k]):
        z[(7 * i + 2) % k] = v

    def check(vk, proofs, inp, zz, want_valid):
        gt, valid = A.ref_aggregate(oracle, pool.vk, proofs, inp, zz)
        assert valid == want_valid
        flat = [x for row in inp for x in row]
        got_valid, got_gt = gpu.groth16_verify_aggregate(vk, proofs, rows_of(flat), A.z_rows(zz), return_gt=True)
        assert got_valid is want_valid and got_gt.shape == (1, 72)
        np.testing.assert_array_equal(got_gt, gt)
        # no gt requested, and repr inputs
        assert gpu.groth16_verify_aggregate(vk, proofs, small_scalars(flat), A.z_rows(zz),
                                            montgomery=False) is want_valid
        return gt

    with gpu.groth16_vk(*pool.vk.args()) as vk:
        gt = check(vk, good, inputs, z, True)
        np.testing.assert_array_equal(gt, fq12_one())
        for at in sorted({0, k // 2, k - 1}):
            bad = good.copy()
            bad[at] = pool.proofs[2]                  # a spoiled witness
            zz = list(z)
            zz[at] |= 1
            check(vk, bad, inputs, zz, False)
            zz[at] = 0                                # dropped from the check
            check(vk, bad, inputs, zz, True)
        wrong = [list(x) for x in inputs]
        wrong[k // 2][0] = (wrong[k // 2][0] + 1) % R_ORDER
        check(vk, good, wrong, z, False)
        # weights drawn by the layer
        flat = rows_of([x for row in inputs for x in row])
        assert gpu.groth16_verify_aggregate(vk, good, flat) is True
        bad = good.copy()
        bad[k - 1] = pool.proofs[2]
        assert gpu.groth16_verify_aggregate(vk, bad, flat) is False


@pytest.mark.gpu
def test_aggregate_gt_none_gives_not_valid_and_a_zero_gt(gpu, oracle, pool):  # noqa: F811
    """A B of pure small order off E' (pairing_domain_cases.SMALL_ORDER_Q) whose Miller value is zero makes the
    product zero and the final exponentiation None: valid 0 and gt a zero record.  The reference here is the
    oracle's Miller loops, Fq12 product and final exponentiation over the reference's own P and Q arrays."""
    import pairing_domain_cases as PD
    good, inputs = _valid_batch(pool, 3)
    z = [1, 5, (1 << 128) - 1]
    found = None
    for kind in PD.SMALL_ORDER_Q:
        bad = good.copy()
        bad[1, 13:38] = np.array(D.aff_record(2, PD.points()["q"][kind]), np.uint64)
        p, q = A.ref_points(oracle, pool.vk, bad, inputs, z), A.q_array(pool.vk, bad)
        ml = oracle.miller_loop_batch(p, oracle.g2_prepare(q))
        if not oracle.final_exponentiation(A.fq12_product(oracle, ml))[1][0]:
            found = bad
            break
    assert found is not None
    flat = rows_of([x for row in inputs for x in row])
    with gpu.groth16_vk(*pool.vk.args()) as vk:
        valid, gt = gpu.groth16_verify_aggregate(vk, found, flat, A.z_rows(z), return_gt=True)
        assert valid is False and gt.shape == (1, 72) and not gt.any()
        assert gpu.groth16_verify_aggregate(vk, found, flat, A.z_rows(z)) is False


@pytest.mark.gpu
def test_aggregate_k_zero(gpu, pool):  # noqa: F811
    with gpu.groth16_vk(*pool.vk.args()) as vk:
        none = np.zeros((0, 4), np.uint64)
        valid, gt = gpu.groth16_verify_aggregate(vk, np.zeros((0, 51), np.uint64), none, return_gt=True)
        assert valid is True
        np.testing.assert_array_equal(gt, fq12_one())
        assert gpu.groth16_verify_aggregate(vk, np.zeros((0, 51), np.uint64), none, np.zeros((0, 2), np.uint64)) is True
        valid, status, gt = gpu.groth16_verify_aggregate_encoded(vk, np.zeros((0, 192), np.uint8), none, return_gt=True)
        assert valid is True and status.shape == (0, 3)
        np.testing.assert_array_equal(gt, fq12_one())


# ---------------- GPU: the encoded entry ----------------

@pytest.mark.gpu
def test_aggregate_encoded_round_trip_and_statuses(gpu, oracle, pool):  # noqa: F811
    g = rng(7500)
    k = 6
    good, inputs = _valid_batch(pool, k)
    flat = rows_of([x for row in inputs for x in row])
    enc = V.encode_proofs(good)
    z = [v | 1 for v in A.rand_z(g, k)]
    with gpu.groth16_vk(*pool.vk.args()) as vk:
        valid, status, gt = gpu.groth16_verify_aggregate_encoded(vk, enc, flat, A.z_rows(z), return_gt=True)
        assert valid is True and status.shape == (k, 3) and not status.any()
        np.testing.assert_array_equal(gt, fq12_one())
        # a spoiled proof that decodes: statuses clean, the verdict and gt are the reference's
        bad = good.copy()
        bad[4] = pool.proofs[2]
        want_gt, want_valid = A.ref_aggregate(oracle, pool.vk, bad, inputs, z)
        valid, status, gt = gpu.groth16_verify_aggregate_encoded(vk, V.encode_proofs(bad), flat, A.z_rows(z),
                                                                 return_gt=True)
        assert valid is False and not want_valid and not status.any()
        np.testing.assert_array_equal(gt, want_gt)
        # one record per status class: that status, valid = 0, the others' statuses untouched
        flipped = None
        for bit in range(8):                              # a bit of A's x that leaves no point on the curve
            t = enc[1].copy()
            t[47] ^= 1 << bit
            if oracle.decode(1, t[None, :48].copy(), True)[1][0] == D.NOT_ON_CURVE:
                flipped = t
                break
        assert flipped is not None
        b_out = enc[3].copy()
        b_out[48:144] = np.frombuffer([c for c in D.g2_cases(True) if c[1] == D.NOT_IN_SUBGROUP][0][0], np.uint8)
        for at, rec, col, code in ((1, flipped, 0, D.NOT_ON_CURVE), (3, b_out, 1, D.NOT_IN_SUBGROUP)):
            data = enc.copy()
            data[at] = rec
            want_status = V.decode_status(oracle, data)
            assert want_status[at, col] == code and np.count_nonzero(want_status) == 1
            valid, status = gpu.groth16_verify_aggregate_encoded(vk, data, flat, A.z_rows(z))
            assert valid is False
            np.testing.assert_array_equal(status, want_status)
            # the failed record decodes to infinity, which drops out of the product: the other five still give one,
            # and only the status makes the batch invalid
            valid, status, gt = gpu.groth16_verify_aggregate_encoded(vk, data, flat, A.z_rows(z), return_gt=True)
            assert valid is False and gt.shape == (1, 72)
        # 3 k = 300 status bytes: two blocks of the kernel that interleaves them, the failed record in the second
        big = np.ascontiguousarray(np.tile(enc, (17, 1))[:100])
        big_flat = np.ascontiguousarray(np.tile(flat.reshape(k, -1, 4), (17, 1, 1))[:100].reshape(-1, 4))
        zz = A.z_rows([v | 1 for v in A.rand_z(g, 100)])
        valid, status = gpu.groth16_verify_aggregate_encoded(vk, big, big_flat, zz)
        assert valid is True and status.shape == (100, 3) and not status.any()
        big[97] = flipped
        want_status = V.decode_status(oracle, big)
        assert want_status[97, 0] == D.NOT_ON_CURVE and np.count_nonzero(want_status) == 1
        valid, status = gpu.groth16_verify_aggregate_encoded(vk, big, big_flat, zz)
        assert valid is False
        np.testing.assert_array_equal(status, want_status)


# ---------------- GPU: the device entries ----------------

def _dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a).view(np.int64)).to("cuda:0")


def _dev_bytes(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a, np.uint8)).to("cuda:0")


@pytest.mark.gpu
def test_aggregate_device_entries_on_a_stream_and_every_error(gpu, oracle, pool):  # noqa: F811
    import torch
    import pairing_amd.device as pdev
    from pairing_amd import _native
    g = rng(7600)
    k = 5
    proofs, inputs = _valid_batch(pool, k)
    mont = rows_of([x for row in inputs for x in row])
    z = [v | 1 for v in A.rand_z(g, k)]
    s = torch.cuda.Stream()
    vk = gpu.groth16_vk(*pool.vk.args())
    try:
        sizes = [vk.verify_aggregate_workspace_bytes(n) for n in
                 (0, 1, 2, 3, 15, 16, 17, 64, 65, 255, 256, 257, 1000, 1001, 4095, 4096, 4097, 1 << 14,
                  # where the MSM's plan of a single n shrinks (test_multiexp_u128_workspace_never_decreases_with_n)
                  104857, 104858, 117965, 117966, (1 << 17) - 1, 1 << 17, 144180, 144181, 1 << 20, 1 << 24)]
        assert sizes == sorted(sizes) and sizes[0] > 0 and sizes[1] < sizes[-1]     # monotone in k
        ws = pdev.groth16_verify_aggregate_workspace(vk, k, "cuda:0")
        assert ws.numel() == vk.verify_aggregate_workspace_bytes(k)
        Pr, X, Z = _dev(proofs), _dev(mont), _dev(A.z_rows(z))
        fill = 0x5a5a5a5a5a5a5a5a
        out_gt = _dev(np.full((2, 72), fill, np.uint64))
        out_valid = torch.full((2,), 9, dtype=torch.uint8, device="cuda:0")
        out_pts = _dev(np.full((k + 4, 13), fill, np.uint64))
        torch.cuda.synchronize()
        with torch.cuda.stream(s):
            pdev.groth16_verify_aggregate(vk, Pr, X, Z, out_valid, ws, gt=out_gt, stream=s)
            pdev.groth16_aggregate_points(vk, Pr, X, Z, out_pts, ws, stream=s)
        s.synchronize()
        host = out_gt.cpu().numpy().view(np.uint64)
        np.testing.assert_array_equal(host[:1], fq12_one())
        assert (host[1] == fill).all()
        assert out_valid.cpu().tolist() == [1, 9]
        pts = out_pts.cpu().numpy().view(np.uint64)
        want_pts = A.ref_points(oracle, pool.vk, proofs, inputs, z)
        np.testing.assert_array_equal(pts[:k + 3], want_pts)
        assert (pts[k + 3] == fill).all()
        for t, a in ((Pr, proofs), (X, mont), (Z, A.z_rows(z))):                   # inputs untouched
            np.testing.assert_array_equal(t.cpu().numpy().view(np.uint64), a)
        # the workspace begins with the P array and, at the next multiple of 256 bytes, the Q array
        q_at = ((k + 3) * 104 + 255) // 256 * 256
        np.testing.assert_array_equal(ws[:(k + 3) * 104].cpu().numpy().view(np.uint64).reshape(k + 3, 13), want_pts)
        np.testing.assert_array_equal(ws[q_at:q_at + (k + 3) * 200].cpu().numpy().view(np.uint64).reshape(k + 3, 25),
                                      A.q_array(pool.vk, proofs))
        # the encoded entry on the same stream
        data = _dev_bytes(V.encode_proofs(proofs))
        st = torch.full((k + 1, 3), 9, dtype=torch.uint8, device="cuda:0")
        v2 = torch.full((2,), 9, dtype=torch.uint8, device="cuda:0")
        with torch.cuda.stream(s):
            pdev.groth16_verify_aggregate_encoded(vk, data, X, Z, v2, st, ws, stream=s)
        s.synchronize()
        assert v2.cpu().tolist() == [1, 9]
        assert not st[:k].cpu().numpy().any() and (st[k].cpu().numpy() == 9).all()
        with pytest.raises(ValueError, match="workspace"):
            pdev.groth16_verify_aggregate(vk, Pr, X, Z, out_valid, ws[:-1], stream=s)

        # what the C entries refuse before anything runs
        lib = _native._lib
        fresh = torch.full((4,), 9, dtype=torch.uint8, device="cuda:0")
        p = lambda t: ctypes.c_void_p(t.data_ptr())  # noqa: E731
        sp = ctypes.c_void_p(s.cuda_stream)
        h = vk.handle()
        NULL, STRIDE, FLAGS, BATCH = "null pointer", "input_stride", "flag", "split"
        WS = "workspace smaller than pa_groth16_verify_aggregate_workspace_bytes"

        def refused(entry, args, message, what):
            assert entry(*args) == -1, what
            assert message in lib.pa_last_error().decode(), (what, lib.pa_last_error())

        def sweep(entry, good, cases):
            for what, i, v, message in cases:
                refused(entry, good[:i] + (v,) + good[i + 1:], message, what)
        common = [("no key", 0, None, NULL), ("no inputs", 2, None, NULL), ("stride below l", 3, 1, STRIDE),
                  ("unknown flag bits", 4, 2, FLAGS), ("no weights", 5, None, NULL),
                  ("a batch over the limit", 6, (1 << 24) + 1, BATCH)]
        good = (h, p(Pr), p(X), 2, 1, p(Z), k, p(fresh), None, p(ws), ws.numel(), sp)
        sweep(lib.pa_groth16_verify_aggregate_device, good, common + [
            ("no proofs", 1, None, NULL), ("no valid", 7, None, NULL), ("no workspace", 9, None, NULL),
            ("workspace one byte short", 10, ws.numel() - 1, WS)])
        enc_good = (h, p(data), p(X), 2, 1, p(Z), k, p(fresh), p(st), None, p(ws), ws.numel(), sp)
        sweep(lib.pa_groth16_verify_aggregate_encoded_device, enc_good, common + [
            ("no records", 1, None, NULL), ("no valid", 7, None, NULL), ("no status", 8, None, NULL),
            ("no workspace", 10, None, NULL), ("workspace one byte short", 11, ws.numel() - 1, WS)])
        pts_good = (h, p(Pr), p(X), 2, 1, p(Z), k, p(out_pts), p(ws), ws.numel(), sp)
        sweep(lib.pa_groth16_verify_aggregate_points_device, pts_good, common + [
            ("no proofs", 1, None, NULL), ("no out", 7, None, NULL), ("no workspace", 8, None, NULL),
            ("workspace one byte short", 9, ws.numel() - 1, WS)])
        if torch.cuda.device_count() > 1:
            other = ctypes.c_void_p(torch.cuda.Stream(device="cuda:1").cuda_stream)
            refused(lib.pa_groth16_verify_aggregate_device, good[:11] + (other,), "another device", "stream")
        assert lib.pa_groth16_verify_aggregate_workspace_bytes(h, (1 << 24) + 1) == 0
        mws = pdev.multiexp_u128_workspace(k, "cuda:0")
        out = pdev.empty_records(1, 18, "cuda:0")
        msm_good = (p(Pr), p(Z), k, p(out), p(mws), mws.numel(), sp)
        sweep(lib.pa_g1_multiexp_u128_device, msm_good, [
            ("no bases", 0, None, NULL), ("no scalars", 1, None, NULL), ("no out", 3, None, NULL),
            ("no workspace", 4, None, NULL),
            ("short workspace", 5, mws.numel() - 1, "workspace smaller than pa_g1_multiexp_u128_workspace_bytes"),
            ("too many terms", 2, 1 << 31, "2^31"),
            ("misaligned scalars", 1, ctypes.c_void_p(Z.data_ptr() + 8), "16-byte aligned")])
        off = ctypes.c_void_p(Z.data_ptr() + 8)
        for entry, args in ((lib.pa_groth16_verify_aggregate_device, good), (lib.pa_groth16_verify_aggregate_encoded_device,
                                                                            enc_good),
                            (lib.pa_groth16_verify_aggregate_points_device, pts_good)):
            refused(entry, args[:5] + (off,) + args[6:], "16-byte aligned", "misaligned z")
        torch.cuda.synchronize()
        assert (fresh.cpu().numpy() == 9).all()
        # k = 0 on the device: valid = 1, gt = one, nothing else written
        one_gt = _dev(np.full((2, 72), fill, np.uint64))
        assert lib.pa_groth16_verify_aggregate_device(h, None, None, 2, 1, None, 0, p(fresh), p(one_gt), p(ws),
                                                      ws.numel(), sp) == 0
        s.synchronize()
        assert fresh.cpu().tolist() == [1, 9, 9, 9]
        host = one_gt.cpu().numpy().view(np.uint64)
        np.testing.assert_array_equal(host[:1], fq12_one())
        assert (host[1] == fill).all()
        # the torch layer's multiexp on the stream
        C = _dev(proofs[:, 38:51])
        with torch.cuda.stream(s):
            pdev.multiexp_u128(C, Z, out, mws, stream=s)
        s.synchronize()
        np.testing.assert_array_equal(gpu.g1_into_affine(out.cpu().numpy().view(np.uint64)), want_pts[k + 1:k + 2])
    finally:
        vk.close()


@pytest.mark.gpu
def test_prove_then_aggregate_verify_from_the_witness_buffer(gpu, oracle, real):  # noqa: F811
    """groth16_prove and groth16_verify_aggregate back to back in HBM, no oracle in between: the inputs are read
    from the prover's witness buffer (witness + 1, stride n_vars)"""
    import torch
    import pairing_amd.device as pdev
    mats, w, key, vkp = real
    g = rng(7700)
    k, n_vars = 4, key.n_vars
    spoiled = list(w)
    spoiled[9] = (spoiled[9] + 5) % R_ORDER
    pk = gpu.groth16_pk(*key.points(oracle))
    sysm = gpu.r1cs(*(G.csr(m) for m in mats), 30, n_vars)
    dom = gpu.fr_ntt_domain(key.log_n)
    vk = gpu.groth16_vk(*vkp.args())
    try:
        Z = _dev(A.z_rows([v | 1 for v in A.rand_z(g, k)]))
        agg_ws = pdev.groth16_verify_aggregate_workspace(vk, k, "cuda:0")
        prove_ws = pdev.groth16_prove_workspace(pk, sysm, k, "cuda:0")
        verdicts = []
        for ws_list in ([w, w, w, w], [w, w, spoiled, w]):
            W = _dev(rows_of([v for x in ws_list for v in x]))
            R, S = _dev(rows_of(G.rand_fr(g, k))), _dev(rows_of(G.rand_fr(g, k)))
            proofs = pdev.empty_records(k, 51, "cuda:0")
            valid = torch.full((2,), 7, dtype=torch.uint8, device="cuda:0")
            pdev.groth16_prove(pk, sysm, dom, W, R, S, proofs, prove_ws)
            pdev.groth16_verify_aggregate(vk, proofs, W[1:], Z, valid, agg_ws, stride=n_vars)
            torch.cuda.synchronize()
            verdicts.append(valid.cpu().tolist())
        assert verdicts == [[1, 7], [0, 7]]
    finally:
        for x in (pk, sysm, dom, vk):
            x.close()
