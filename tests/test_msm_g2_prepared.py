"""G2 multiexp over prepared bases (pa_g2_msm_bases, include/pairing_amd.h).

The bases are checked for G2 membership and converted once; with every base
in G2 a multiexp splits each scalar s = q x^2 + rem (glv_split.h) and runs the
Pippenger pipeline over the 2m virtual terms rem * Q_i + q * (x^2 Q_i) in
ceil(130 / c) windows, where x^2 Q = (beta^2 x, -y) (kernels_msm.hip,
kMsmBeta2, k_msm_bases_prepare_g2); otherwise the 257-bit pipeline runs over
the prepared rows.  A batch of k vectors is one pipeline of k W windows.
Sums are compared as points (PartialEq, ec.rs:45-85) with the oracle's sum of
CurveAffine::mul terms; a batch of one vector, a repeated call and the
Montgomery form of the same scalars are compared word for word."""
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
MSM_SRC = os.path.join(ROOT, "pairing_amd", "csrc", "kernels_msm.hip")
X2 = 0xd201000000010000 ** 2

NEW_SYMBOLS = ("pa_g2_msm_bases_prepare", "pa_g2_msm_bases_prepare_device", "pa_g2_msm_bases_len",
               "pa_g2_msm_bases_in_subgroup", "pa_g2_msm_bases_free", "pa_g2_multiexp_prepared_workspace_bytes",
               "pa_g2_multiexp_prepared_device", "pa_g2_multiexp_prepared",
               "pa_g2_multiexp_prepared_batch_workspace_bytes", "pa_g2_multiexp_prepared_batch_device",
               "pa_g2_multiexp_prepared_batch")

# The GLV path's window bits are lg(2n) - 3 up to 13 for both groups
# (msm_window_bits_glv), and the bucketing sort takes a second pass from
# c - 1 > 8, c = 10: 2n >= 2^13, n >= 4096.  4096 is that smallest size; 4099
# (8198 virtual terms, a ragged third sort tile) is the odd size just above it.
SECOND_PASS = 4096
SECOND_PASS_ODD = 4099


def edge_scalars():
    return small_scalars([0, 1, 2, 3, R_ORDER - 1, R_ORDER, R_ORDER + 1, (1 << 256) - 1, 1 << 255, 0xffff])


def wide_scalars(g, n):
    """n 256-bit FrRepr values with the top bit set: all >= r"""
    return small_scalars([int.from_bytes(g.bytes(32), "little") | 1 << 255 for _ in range(n)])


def neg_y(oracle, rec):
    """the G2 affine records with y negated"""
    out = rec.copy()
    zero = np.zeros((rec.shape[0], 6), np.uint64)
    out[:, 12:18] = oracle.fq_sub(zero, np.ascontiguousarray(rec[:, 12:18]))
    out[:, 18:24] = oracle.fq_sub(zero, np.ascontiguousarray(rec[:, 18:24]))
    return out


def dressed(oracle, n, seed):
    """from 17 terms up the ten edge scalars, an infinity base, two equal bases
    with equal scalars, Q with -Q"""
    g = rng(seed)
    p = oracle.g2_mul_generator(random_scalars(g, n), NT)
    s = random_scalars(g, n)
    if n >= 17:
        s[:10] = edge_scalars()
        set_infinity(p, [11])
        p[12] = p[13]
        s[12] = s[13]
        p[14] = neg_y(oracle, p[15:16])[0]
        s[14] = s[15]
    return p, s


# ---------------- CPU: the surface ----------------

def test_new_symbols_are_declared_and_bound():
    from pairing_amd import _native
    with open(HEADER) as f:
        text = f.read()
    declared = set(re.findall(r"^\s*(?:const\s+)?\w+\s*\*?\s*(pa_\w+)\s*\(", text, flags=re.M))
    assert re.search(r"typedef\s+struct\s+pa_g2_msm_bases\s+pa_g2_msm_bases\s*;", text)
    for name in NEW_SYMBOLS:
        assert name in declared, name
        assert name in _native._SIGS, name
        assert getattr(_native._lib, name).argtypes == _native._SIGS[name]
    sz, p, u = ctypes.c_size_t, ctypes.c_void_p, ctypes.c_uint
    # size_t travels as c_size_t, not ctypes' default int
    for name in ("pa_g2_msm_bases_len", "pa_g2_multiexp_prepared_workspace_bytes",
                 "pa_g2_multiexp_prepared_batch_workspace_bytes"):
        assert getattr(_native._lib, name).restype is sz, name
    # the G1 block's signatures, one for one
    for name in NEW_SYMBOLS:
        assert _native._SIGS[name] == _native._SIGS[name.replace("pa_g2_", "pa_g1_")], name
    assert _native._SIGS["pa_g2_multiexp_prepared_device"] == [p, p, sz, p, p, sz, p]
    assert _native._SIGS["pa_g2_multiexp_prepared_batch_workspace_bytes"] == [p, sz, sz]
    assert _native._SIGS["pa_g2_multiexp_prepared_batch_device"] == [p, p, sz, sz, u, p, p, sz, p]
    assert _native._SIGS["pa_g2_multiexp_prepared_batch"] == [p, p, sz, sz, u, p]


def borrowed(length, group=2):
    """a live-looking object over a handle nobody may dereference (the checks
    under test come before any native call) and nobody frees"""
    import pairing_amd as pa
    cls = pa.G2MsmBases if group == 2 else pa.G1MsmBases
    return cls(ctypes.c_void_p(8), length, True, owns=False)


def z(*shape):
    return np.zeros(shape, np.uint64)


def test_python_layer_rejects_bad_shapes():
    import pairing_amd as pa
    for name in ("G2MsmBases", "g2_msm_prepare", "g2_multiexp_prepared", "g2_multiexp_prepared_batch"):
        assert name in pa.__all__, name
    with pytest.raises(ValueError):
        pa.g2_msm_prepare(z(3, 24))
    with pytest.raises(ValueError):
        pa.g2_msm_prepare(z(3, 13))                                     # G1 records
    with pytest.raises(ValueError):
        pa.g2_multiexp_prepared(borrowed(5), z(3, 5))
    with pytest.raises(ValueError):
        pa.g2_multiexp_prepared(object(), z(3, 4))
    with pytest.raises(ValueError):
        pa.g2_multiexp_prepared_batch(borrowed(5), z(3, 4, 5))          # rows of five words
    with pytest.raises(ValueError):
        pa.g2_multiexp_prepared_batch(borrowed(5), z(10, 4), count=3)   # 10 rows are not 3 vectors
    with pytest.raises(ValueError):
        pa.g2_multiexp_prepared_batch(borrowed(5), z(10, 4))            # flat rows need a count
    with pytest.raises(ValueError):
        pa.g2_multiexp_prepared_batch(object(), z(2, 3, 4))
    with pytest.raises(ValueError):
        pa.g2_multiexp_prepared_batch(borrowed(5), z(2, 3, 4), montgomery=2)


def test_python_layer_rejects_too_many_scalars_and_closed_objects():
    import pairing_amd as pa
    b = borrowed(5)
    assert b.len == 5 and len(b) == 5 and b.in_subgroup and not b.closed
    with pytest.raises(ValueError):
        pa.g2_multiexp_prepared(b, z(6, 4))
    with pytest.raises(ValueError):
        pa.g2_multiexp_prepared_batch(b, z(2, 6, 4))            # m > len
    with pytest.raises(ValueError):
        pa.g2_multiexp_prepared_batch(b, z(12, 4), count=2)     # m > len, flat form
    b.close()
    b.close()   # idempotent
    assert b.closed
    with pytest.raises(ValueError):
        pa.g2_multiexp_prepared(b, z(5, 4))
    with pytest.raises(ValueError):
        pa.g2_multiexp_prepared_batch(b, z(2, 3, 4))
    with pytest.raises(ValueError):
        b.handle()
    with pytest.raises(ValueError):
        b.check_terms(0)


class _NoNativeCall:
    """stands in for the library: any entry reached is a failure"""
    def __getattr__(self, name):
        raise AssertionError("native entry %s reached" % name)


def test_a_handle_of_the_other_group_is_rejected_before_any_native_call(monkeypatch):
    import pairing_amd as pa
    from pairing_amd import _native
    g1, g2 = borrowed(5, group=1), borrowed(5, group=2)
    assert not isinstance(g1, pa.G2MsmBases) and not isinstance(g2, pa.G1MsmBases)
    monkeypatch.setattr(_native, "_lib", _NoNativeCall())
    with pytest.raises(ValueError):
        pa.g2_multiexp_prepared(g1, z(3, 4))
    with pytest.raises(ValueError):
        pa.g2_multiexp_prepared_batch(g1, z(2, 3, 4))
    with pytest.raises(ValueError):
        pa.g1_multiexp_prepared(g2, z(3, 4))
    with pytest.raises(ValueError):
        pa.g1_multiexp_prepared_batch(g2, z(2, 3, 4))


def test_device_layer_rejects_the_other_group_and_closed_objects(monkeypatch):
    import torch
    import pairing_amd.device as pdev
    from pairing_amd import _native
    monkeypatch.setattr(_native, "_lib", _NoNativeCall())
    monkeypatch.setattr(pdev, "_lib", _NoNativeCall())
    g1, g2 = borrowed(5, group=1), borrowed(5, group=2)
    s = torch.zeros((6, 4), dtype=torch.int64)
    o1, o2 = torch.zeros((2, 18), dtype=torch.int64), torch.zeros((2, 36), dtype=torch.int64)
    ws = torch.zeros(16, dtype=torch.uint8)
    for bad in (g1, object()):
        with pytest.raises(ValueError):
            pdev.g2_multiexp_prepared_workspace(bad, 3, "cpu")
        with pytest.raises(ValueError):
            pdev.g2_multiexp_prepared(bad, s[:3], o2[:1], ws)
        with pytest.raises(ValueError):
            pdev.g2_multiexp_prepared_batch_workspace(bad, 3, 2, "cpu")
        with pytest.raises(ValueError):
            pdev.g2_multiexp_prepared_batch(bad, s, 3, 2, o2, ws)
    with pytest.raises(ValueError):
        pdev.multiexp_prepared_workspace(g2, 3, "cpu")
    with pytest.raises(ValueError):
        pdev.multiexp_prepared(g2, s[:3], o1[:1], ws)
    with pytest.raises(ValueError):
        pdev.multiexp_prepared_batch_workspace(g2, 3, 2, "cpu")
    with pytest.raises(ValueError):
        pdev.multiexp_prepared_batch(g2, s, 3, 2, o1, ws)
    with pytest.raises(ValueError):
        pdev.g2_multiexp_prepared_workspace(g2, 6, "cpu")           # too many terms
    with pytest.raises(ValueError):
        pdev.g2_multiexp_prepared_batch_workspace(g2, 6, 2, "cpu")
    g2.close()
    with pytest.raises(ValueError):
        pdev.g2_multiexp_prepared(g2, s[:3], o2[:1], ws)
    with pytest.raises(ValueError):
        pdev.g2_multiexp_prepared_batch(g2, s, 3, 2, o2, ws)


# ---------------- CPU: the relation x^2 Q = (beta^2 x, -y) ----------------

def _constant(name):
    with open(MSM_SRC) as f:
        m = re.search(r"\b%s\[6\]\s*=\s*\{([^}]*)\}" % name, f.read())
    assert m, name
    ws = [int(t.strip().rstrip("ULul"), 0) for t in m.group(1).split(",")]
    assert len(ws) == 6
    return np.array([ws], np.uint64)


def test_beta2_is_the_square_of_beta(oracle):
    beta, beta2 = _constant("kMsmBeta"), _constant("kMsmBeta2")
    np.testing.assert_array_equal(oracle.fq_square(beta), beta2)
    assert not np.array_equal(beta, beta2)


def test_x2_times_q_is_beta2_x_minus_y(oracle):
    """What row n + i of the prepared rows holds, against the oracle's scalar
    multiplication, word for word in affine form: 8 random subgroup points and
    the generator.  With beta in place of beta^2 the comparison fails (checked
    below: that is the G1 relation)."""
    beta, beta2 = _constant("kMsmBeta"), _constant("kMsmBeta2")
    q = oracle.g2_mul_generator(np.concatenate([random_scalars(rng(501), 8), small_scalars([1])]), NT)
    n = q.shape[0]
    assert X2 % R_ORDER == X2
    want = oracle.g2_into_affine(oracle.g2_affine_mul(q, small_scalars([X2] * n), NT))

    def endo(b):
        out = neg_y(oracle, q)
        bb = np.repeat(b, n, axis=0)
        out[:, 0:6] = oracle.fq_mul(np.ascontiguousarray(q[:, 0:6]), bb)
        out[:, 6:12] = oracle.fq_mul(np.ascontiguousarray(q[:, 6:12]), bb)
        return out

    np.testing.assert_array_equal(endo(beta2), want)
    assert not (endo(beta)[:, :12] == want[:, :12]).all(axis=1).any()


# ---------------- GPU ----------------

@pytest.fixture(scope="module")
def base300(oracle):
    """300 dressed subgroup bases and three scalar sets with the oracle's sums"""
    p, s0 = dressed(oracle, 300, 550)
    g = rng(551)
    sets = [s0, random_scalars(g, 300), random_scalars(g, 300)]
    sets[2][:10] = edge_scalars()[::-1]
    sets[2][100:200] = wide_scalars(g, 100)
    return p, sets, [oracle.g2_multiexp(p, s, NT) for s in sets]


@pytest.fixture(scope="module")
def outside_g2():
    """a curve point outside G2 and a subgroup point plus torsion, as affine records"""
    pts, truth = D.subgroup_points(2, seed=571, n=1)   # [R, h R, r R, h R + r R, ...]
    assert not truth[0] and truth[1] and not truth[3]
    return {"curve_point": np.array(D.aff_record(2, pts[0]), np.uint64),
            "subgroup_plus_torsion": np.array(D.aff_record(2, pts[3]), np.uint64)}


def batch_scalars(s0, k, seed):
    """k vectors of len(s0) scalars: s0, then random ones with a block of values >= r"""
    m = s0.shape[0]
    g = rng(seed)
    s = np.zeros((k, m, 4), np.uint64)
    if k:
        s[0] = s0
    for j in range(1, k):
        s[j] = random_scalars(g, m)
        w = min(m // 3, 40)
        s[j, m // 2:m // 2 + w] = wide_scalars(g, w)
    return s


@pytest.mark.gpu
@pytest.mark.parametrize("n", [0, 1, 2, 3, 17, 300, SECOND_PASS, SECOND_PASS_ODD])
def test_prepared_multiexp_matches_oracle(gpu, oracle, n):
    p, s = dressed(oracle, n, 500 + n)
    with gpu.g2_msm_prepare(p) as b:
        assert b.len == n and b.in_subgroup
        got = gpu.g2_multiexp_prepared(b, s)
    assert got.shape == (1, 36)
    assert oracle.g2_eq(got, oracle.g2_multiexp(p, s, NT)).all()


@pytest.mark.gpu
def test_one_object_many_scalar_sets_and_prefixes(gpu, oracle, base300):
    p, sets, sums = base300
    b = gpu.g2_msm_prepare(p)
    try:
        assert b.in_subgroup
        for s, exp in zip(sets, sums):
            assert oracle.g2_eq(gpu.g2_multiexp_prepared(b, s), exp).all()
        got = gpu.g2_multiexp_prepared(b, sets[1][:200])
        assert oracle.g2_eq(got, oracle.g2_multiexp(p[:200], sets[1][:200], NT)).all()
        zero = gpu.g2_multiexp_prepared(b, sets[1][:0])
        assert oracle.g2_eq(zero, oracle.g2_multiexp(p[:0], sets[1][:0])).all()
    finally:
        b.close()
    with pytest.raises(ValueError):
        gpu.g2_multiexp_prepared(b, sets[0])


@pytest.mark.gpu
def test_prepared_multiexp_deterministic(gpu, oracle):
    g = rng(580)
    n = 5000
    p = oracle.g2_mul_generator(random_scalars(g, n), NT)
    s = random_scalars(g, n)
    s[100:300] = s[7]
    with gpu.g2_msm_prepare(p) as b:
        a1 = gpu.g2_multiexp_prepared(b, s)
        a2 = gpu.g2_multiexp_prepared(b, s)
    np.testing.assert_array_equal(a1, a2)
    assert oracle.g2_eq(a1, oracle.g2_multiexp(p, s, NT)).all()


@pytest.mark.gpu
def test_prepared_multiexp_crowded_buckets(gpu, oracle):
    """Every scalar equal but a short run: both halves crowd one bucket per
    window.  9000 terms are 18000 virtual ones, c = 11 and 8 items per lane:
    a crowded bucket spans ~1100 chunks, far over the GLV path's threshold of
    8 (msm_long_span_glv, the same for G2): k_msm_long_fix<2> folds it."""
    g = rng(595)
    n = 9000
    p = oracle.g2_mul_generator(random_scalars(g, n), NT)
    s = np.repeat(random_scalars(g, 1), n, axis=0)
    s[n // 3:n // 3 + 50] = random_scalars(g, 1)
    set_infinity(p, [5, n // 2])
    with gpu.g2_msm_prepare(p) as b:
        assert b.in_subgroup
        got = gpu.g2_multiexp_prepared(b, s)
    assert oracle.g2_eq(got, oracle.g2_multiexp(p, s, NT)).all()


@pytest.mark.gpu
@pytest.mark.parametrize("kind", ["curve_point", "subgroup_plus_torsion"])
def test_fallback_for_a_base_outside_g2(gpu, oracle, base300, outside_g2, kind):
    p = base300[0].copy()
    p[137] = outside_g2[kind]
    with gpu.g2_msm_prepare(p) as b:
        assert b.len == 300 and not b.in_subgroup
        for s in base300[1][:2]:
            got = gpu.g2_multiexp_prepared(b, s)
            assert oracle.g2_eq(got, oracle.g2_multiexp(p, s, NT)).all()
            assert oracle.g2_eq(got, gpu.g2_multiexp(p, s)).all()
        s = np.stack(base300[1][:2])
        rows = gpu.g2_multiexp_prepared_batch(b, s)
    for j in range(2):
        assert oracle.g2_eq(rows[j:j + 1], gpu.g2_multiexp(p, s[j])).all()


@pytest.mark.gpu
@pytest.mark.parametrize("m,k", [(300, 1), (300, 2), (300, 3), (300, 5), (SECOND_PASS_ODD, 3)])
def test_batch_rows_are_the_single_entry_points(gpu, oracle, m, k):
    """k = 2 fills a Horner wave (two groups of 8 quads), 3 and 5 leave its
    second half empty, 1 is the single entry's job: the same words"""
    p, s0 = dressed(oracle, m, 600 + m)
    s = batch_scalars(s0, k, 630 + m + k)
    with gpu.g2_msm_prepare(p) as b:
        assert b.in_subgroup
        got = gpu.g2_multiexp_prepared_batch(b, s)
        flat = gpu.g2_multiexp_prepared_batch(b, s.reshape(-1, 4), count=k)
        singles = [gpu.g2_multiexp_prepared(b, s[j]) for j in range(k)]
    assert got.shape == (k, 36)
    np.testing.assert_array_equal(got, flat)
    for j in range(k):
        assert oracle.g2_eq(got[j:j + 1], singles[j]).all(), "vector %d" % j
    if k == 1:
        np.testing.assert_array_equal(got, singles[0])
    # the oracle on the first and last vectors (the singles tie the rest to it
    # through test_prepared_multiexp_matches_oracle)
    for j in {0, k - 1}:
        assert oracle.g2_eq(got[j:j + 1], oracle.g2_multiexp(p, s[j], NT)).all(), "vector %d" % j


def reduced(oracle, s):
    """the scalars mod r as FrRepr rows, and their Montgomery form"""
    r = small_scalars([from_limbs(x) % R_ORDER for x in s.reshape(-1, 4)])
    mont, ok = oracle.fr_from_repr(r)
    assert ok.all()
    return r, mont


@pytest.mark.gpu
def test_montgomery_scalars_give_the_same_points(gpu, oracle, base300):
    p, sets, _ = base300
    k = 3
    s, mont = reduced(oracle, np.stack(sets))
    with gpu.g2_msm_prepare(p) as b:
        want = gpu.g2_multiexp_prepared_batch(b, s, count=k)
        got = gpu.g2_multiexp_prepared_batch(b, mont, count=k, montgomery=True)
    np.testing.assert_array_equal(got, want)   # the same digits: the same words
    for j in range(k):
        assert oracle.g2_eq(got[j:j + 1], oracle.g2_multiexp(p, s[j * 300:(j + 1) * 300], NT)).all(), j


@pytest.mark.gpu
def test_zero_sizes(gpu, oracle, base300):
    p, sets, _ = base300
    zero = oracle.g2_multiexp(p[:0], sets[0][:0])
    with gpu.g2_msm_prepare(p) as b:
        none = gpu.g2_multiexp_prepared_batch(b, z(0, 300, 4))              # k = 0
        assert none.shape == (0, 36)
        assert gpu.g2_multiexp_prepared_batch(b, z(0, 4), count=0).shape == (0, 36)
        empty = gpu.g2_multiexp_prepared_batch(b, z(3, 0, 4))               # m = 0: k zero points
        assert empty.shape == (3, 36)
        assert oracle.g2_eq(empty, np.repeat(zero, 3, axis=0)).all()
    with gpu.g2_msm_prepare(p[:0]) as b0:                                   # no bases at all
        assert b0.len == 0 and b0.in_subgroup
        assert oracle.g2_eq(gpu.g2_multiexp_prepared(b0, sets[0][:0]), zero).all()


@pytest.mark.gpu
def test_device_layer_on_a_side_stream_with_the_callers_workspace(gpu, oracle, base300):
    import torch
    import pairing_amd.device as pdev
    p, sets, sums = base300
    k, m = 3, 300
    s = np.stack(sets)
    dev_s = torch.from_numpy(s.reshape(-1, 4).view(np.int64)).cuda()
    stream = torch.cuda.Stream()
    torch.cuda.synchronize()
    with torch.cuda.stream(stream):
        b = pdev.g2_msm_prepare(torch.from_numpy(p.view(np.int64)).cuda(), stream=stream)
        assert isinstance(b, gpu.G2MsmBases) and b.len == m and b.in_subgroup
        one = pdev.empty_records(1, 36, "cuda")
        rows = pdev.empty_records(k, 36, "cuda")
        ws1 = pdev.g2_multiexp_prepared_workspace(b, m, "cuda")
        wsk = pdev.g2_multiexp_prepared_batch_workspace(b, m, k, "cuda")
        pdev.g2_multiexp_prepared(b, dev_s[m:2 * m], one, ws1, stream=stream)
        pdev.g2_multiexp_prepared_batch(b, dev_s, m, k, rows, wsk, stream=stream)
    stream.synchronize()
    b.close()
    with gpu.g2_msm_prepare(p) as hb:
        np.testing.assert_array_equal(one.cpu().numpy().view(np.uint64), gpu.g2_multiexp_prepared(hb, s[1]))
        np.testing.assert_array_equal(rows.cpu().numpy().view(np.uint64), gpu.g2_multiexp_prepared_batch(hb, s))
    assert oracle.g2_eq(one.cpu().numpy().view(np.uint64), sums[1]).all()


@pytest.mark.gpu
def test_device_entry_errors_are_codes_not_aborts(gpu, oracle, base300):
    import torch
    import pairing_amd.device as pdev
    from pairing_amd._native import _lib
    p, sets, sums = base300
    b = pdev.g2_msm_prepare(torch.from_numpy(p.view(np.int64)).cuda())
    n, k = b.len, 3
    s = torch.from_numpy(np.concatenate(sets + [sets[0][:3]]).view(np.int64)).cuda()   # 3 n + 3 rows
    out = pdev.empty_records(k, 36, "cuda")
    stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    args = (b.handle(), ctypes.c_void_p(s.data_ptr()))
    host_out = np.zeros((k, 36), np.uint64)
    hs = np.zeros((n + 1, 4), np.uint64)
    hptr = (hs.ctypes.data_as(ctypes.c_void_p), host_out.ctypes.data_as(ctypes.c_void_p))

    # the single entry
    ws = pdev.g2_multiexp_prepared_workspace(b, n, "cuda")
    tail = (ctypes.c_void_p(out.data_ptr()), ctypes.c_void_p(ws.data_ptr()))
    need = int(_lib.pa_g2_multiexp_prepared_workspace_bytes(b.handle(), n))
    assert 0 < need <= ws.numel()
    assert int(_lib.pa_g2_multiexp_prepared_workspace_bytes(b.handle(), n + 1)) == 0
    assert _lib.pa_g2_multiexp_prepared_device(*args, n, *tail, need - 1, stream) < 0
    assert b"workspace" in _lib.pa_last_error()
    assert _lib.pa_g2_multiexp_prepared_device(*args, n + 1, *tail, ws.numel(), stream) < 0
    assert b"prepared bases" in _lib.pa_last_error()
    assert _lib.pa_g2_multiexp_prepared(b.handle(), hptr[0], n + 1, hptr[1]) < 0

    # the batch entry
    wsk = pdev.g2_multiexp_prepared_batch_workspace(b, n, k, "cuda")
    tailk = (ctypes.c_void_p(out.data_ptr()), ctypes.c_void_p(wsk.data_ptr()))
    query = _lib.pa_g2_multiexp_prepared_batch_workspace_bytes
    entry = _lib.pa_g2_multiexp_prepared_batch_device
    needk = int(query(b.handle(), n, k))
    assert 0 < needk <= wsk.numel()
    assert int(query(b.handle(), n + 1, k)) == 0
    assert entry(*args, n, k, 0, *tailk, needk - 1, stream) < 0
    assert b"workspace" in _lib.pa_last_error()
    assert entry(*args, n + 1, k, 0, *tailk, wsk.numel(), stream) < 0
    assert b"prepared bases" in _lib.pa_last_error()
    assert entry(*args, n, k, 2, *tailk, wsk.numel(), stream) < 0
    assert b"flag" in _lib.pa_last_error()
    # over the 32-bit item limit: a window has at least n items in either
    # pipeline (n or 2 n terms), so k n > 2^32 - 1 puts k W nt over it
    big = (1 << 32) // n + 1
    assert int(query(b.handle(), n, big)) == 0
    assert entry(*args, n, big, 0, *tailk, wsk.numel(), stream) < 0
    assert b"limit" in _lib.pa_last_error()
    with pytest.raises(ValueError):
        pdev.g2_multiexp_prepared_batch_workspace(b, n, big, "cuda")
    host = _lib.pa_g2_multiexp_prepared_batch
    assert host(b.handle(), hptr[0], n + 1, k, 0, hptr[1]) < 0
    assert host(b.handle(), hptr[0], n, big, 0, hptr[1]) < 0

    # and the object still computes both
    pdev.g2_multiexp_prepared(b, s[:n], out[:1], ws)
    torch.cuda.synchronize()
    assert oracle.g2_eq(out[:1].cpu().numpy().view(np.uint64), sums[0]).all()
    pdev.g2_multiexp_prepared_batch(b, s, n, k, out, wsk)
    torch.cuda.synchronize()
    got = out.cpu().numpy().view(np.uint64)
    for j in range(k):
        assert oracle.g2_eq(got[j:j + 1], sums[j]).all()
    b.close()
