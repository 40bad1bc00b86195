"""Batched G1 multiexp over prepared bases (pa_g1_multiexp_prepared_batch,
include/pairing_amd.h): k scalar vectors end to end over the same prepared
bases run as one Pippenger pipeline of k W windows (kernels_msm.hip: vector
j's window w is window j W + w, the parts are ranges of vectors,
k_msm_horner_batch_q finishes every vector side by side).  Every output row is
compared as a point (PartialEq, ec.rs:45-85) with the oracle's sum of
CurveAffine::mul terms for that vector; a batch of one vector, a repeated call
and the Montgomery form of the same scalars are compared word for word."""
import ctypes
import os
import re

import numpy as np
import pytest

import decode_cases as D
from helpers import R_ORDER, from_limbs, random_scalars, rng, set_infinity, small_scalars
from test_msm_prepared import base300, borrowed, dressed, wide_scalars  # noqa: F401  (base300 is a fixture)

NT = 8
ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
HEADER = os.path.join(ROOT, "include", "pairing_amd.h")

NEW_SYMBOLS = ("pa_g1_multiexp_prepared_batch_workspace_bytes", "pa_g1_multiexp_prepared_batch_device",
               "pa_g1_multiexp_prepared_batch")


# ---------------- CPU: the surface ----------------

def test_batch_symbols_are_declared_and_bound():
    from pairing_amd import _native
    with open(HEADER) as f:
        text = f.read()
    declared = set(re.findall(r"^\s*(?:const\s+)?\w+\s*\*?\s*(pa_\w+)\s*\(", text, flags=re.M))
    for name in NEW_SYMBOLS:
        assert name in declared, name
        assert name in _native._SIGS, name
        assert getattr(_native._lib, name).argtypes == _native._SIGS[name]
    assert re.search(r"#define\s+PA_MSM_SCALARS_REPR\s+0u", text)
    assert re.search(r"#define\s+PA_MSM_SCALARS_MONTGOMERY\s+1u", text)
    sz, p, u = ctypes.c_size_t, ctypes.c_void_p, ctypes.c_uint
    assert _native._lib.pa_g1_multiexp_prepared_batch_workspace_bytes.restype is sz
    assert _native._SIGS["pa_g1_multiexp_prepared_batch_workspace_bytes"] == [p, sz, sz]
    assert _native._SIGS["pa_g1_multiexp_prepared_batch_device"] == [p, p, sz, sz, u, p, p, sz, p]
    assert _native._SIGS["pa_g1_multiexp_prepared_batch"] == [p, p, sz, sz, u, p]
    assert _native.msm_scalars(False) == 0 and _native.msm_scalars(True) == 1
    with pytest.raises(ValueError):
        _native.msm_scalars(2)


def test_python_layer_rejects_bad_batches():
    import pairing_amd as pa
    assert "g1_multiexp_prepared_batch" in pa.__all__
    z = lambda *shape: np.zeros(shape, np.uint64)   # noqa: E731
    with pytest.raises(ValueError):
        pa.g1_multiexp_prepared_batch(borrowed(5), z(3, 4, 5))          # rows of five words
    with pytest.raises(ValueError):
        pa.g1_multiexp_prepared_batch(borrowed(5), z(10, 4), count=3)   # 10 rows are not 3 vectors
    with pytest.raises(ValueError):
        pa.g1_multiexp_prepared_batch(borrowed(5), z(10, 4))            # flat rows need a count
    with pytest.raises(ValueError):
        pa.g1_multiexp_prepared_batch(borrowed(5), z(2, 6, 4))          # m > len
    with pytest.raises(ValueError):
        pa.g1_multiexp_prepared_batch(borrowed(5), z(12, 4), count=2)   # m > len, flat form
    with pytest.raises(ValueError):
        pa.g1_multiexp_prepared_batch(object(), z(2, 3, 4))             # not a G1MsmBases
    with pytest.raises(ValueError):
        pa.g1_multiexp_prepared_batch(borrowed(5), z(2, 3, 4), montgomery=2)
    b = borrowed(5)
    b.close()
    with pytest.raises(ValueError):
        pa.g1_multiexp_prepared_batch(b, z(2, 3, 4))                    # closed


# ---------------- GPU ----------------

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


def assert_rows_match_oracle(oracle, got, p, s):
    assert got.shape == (s.shape[0], 18)
    for j in range(s.shape[0]):
        assert oracle.g1_eq(got[j:j + 1], oracle.g1_multiexp(p, s[j], NT)).all(), "vector %d" % j


@pytest.mark.gpu
@pytest.mark.parametrize("m,k", [(0, 3), (5, 0), (1, 1), (3, 2), (17, 3), (300, 3), (5, 37), (4099, 3)])
def test_batch_matches_oracle(gpu, oracle, m, k):
    # (5, 37): c = 4, 33 GLV windows per vector, 1221 windows in all (the prefix
    # lookup, the Horner grid); (4099, 3): 8198 virtual terms, c = 10, the sort's
    # second pass, and an odd vector count across the parts
    n = max(m, 1)
    p, s0 = dressed(oracle, n, 400 + m)
    s = batch_scalars(s0[:m], k, 430 + m)
    with gpu.g1_msm_prepare(p) as b:
        assert b.in_subgroup
        got = gpu.g1_multiexp_prepared_batch(b, s)
        flat = gpu.g1_multiexp_prepared_batch(b, s.reshape(-1, 4), count=k)
    np.testing.assert_array_equal(got, flat)
    assert_rows_match_oracle(oracle, got, p[:m], s)
    if m == 0:
        assert oracle.g1_eq(got, np.repeat(oracle.g1_multiexp(p[:0], s0[:0]), k, axis=0)).all()


@pytest.mark.gpu
def test_batch_uneven_neighbours(gpu, oracle):
    """An all-zero vector (every digit dropped: its windows are empty and its
    row is the zero point) beside the crowded-bucket input of
    test_prepared_multiexp_crowded_buckets (k_msm_long_fix inside a part that
    also holds ordinary buckets) and a random vector"""
    g = rng(395)
    n = 9000
    p = oracle.g1_mul_generator(random_scalars(g, n), NT)
    crowded = np.repeat(random_scalars(g, 1), n, axis=0)
    crowded[n // 3:n // 3 + 50] = random_scalars(g, 1)
    set_infinity(p, [5, n // 2])
    s = np.stack([np.zeros((n, 4), np.uint64), crowded, random_scalars(g, n)])
    with gpu.g1_msm_prepare(p) as b:
        assert b.in_subgroup
        got = gpu.g1_multiexp_prepared_batch(b, s)
    zero = oracle.g1_multiexp(p[:0], s[0][:0])
    assert oracle.g1_eq(got[0:1], zero).all()
    assert_rows_match_oracle(oracle, got[1:], p, s[1:])


@pytest.mark.gpu
@pytest.mark.parametrize("kind", ["curve_point", "subgroup_plus_torsion"])
def test_batch_fallback_for_a_base_outside_g1(gpu, oracle, base300, kind):
    pts, truth = D.subgroup_points(1, seed=371, n=1)   # [R, h R, r R, h R + r R, ...]
    idx = 0 if kind == "curve_point" else 3
    assert not truth[idx] and truth[1]
    p = base300[0].copy()
    p[137] = np.array(D.aff_record(1, pts[idx]), np.uint64)
    s = np.stack(base300[1])
    with gpu.g1_msm_prepare(p) as b:
        assert b.len == 300 and not b.in_subgroup
        got = gpu.g1_multiexp_prepared_batch(b, s)
    assert_rows_match_oracle(oracle, got, p, s)
    for j in range(3):
        assert oracle.g1_eq(got[j:j + 1], gpu.g1_multiexp(p, s[j])).all()


@pytest.mark.gpu
def test_batch_over_a_prefix_of_the_bases(gpu, oracle, base300):
    p, sets, _ = base300
    s = np.stack([x[:200] for x in sets])
    with gpu.g1_msm_prepare(p) as b:
        got = gpu.g1_multiexp_prepared_batch(b, s)
    assert_rows_match_oracle(oracle, got, p[:200], s)


@pytest.mark.gpu
@pytest.mark.parametrize("n", [300, 5000])
def test_batch_of_one_vector_is_the_single_entry(gpu, oracle, n):
    # the same job (window bits, parts, addition order): the same words
    g = rng(440 + n)
    p = oracle.g1_mul_generator(random_scalars(g, n), NT)
    s = random_scalars(g, n)
    s[n // 2:n // 2 + 20] = wide_scalars(g, 20)
    with gpu.g1_msm_prepare(p) as b:
        one = gpu.g1_multiexp_prepared(b, s)
        got = gpu.g1_multiexp_prepared_batch(b, s[None])
    np.testing.assert_array_equal(got, one)
    assert oracle.g1_eq(got, oracle.g1_multiexp(p, s, NT)).all()


@pytest.mark.gpu
def test_batch_deterministic(gpu, oracle):
    g = rng(450)
    n, k = 5000, 4
    p = oracle.g1_mul_generator(random_scalars(g, n), NT)
    s = np.stack([random_scalars(g, n) for _ in range(k)])
    s[1, 100:300] = s[1, 7]
    with gpu.g1_msm_prepare(p) as b:
        a1 = gpu.g1_multiexp_prepared_batch(b, s)
        a2 = gpu.g1_multiexp_prepared_batch(b, s)
    np.testing.assert_array_equal(a1, a2)
    assert oracle.g1_eq(a1[1:2], oracle.g1_multiexp(p, s[1], NT)).all()


@pytest.mark.gpu
@pytest.mark.parametrize("parts,chunk", [("2", "8"), ("3", "64"), ("8", "16")])
def test_batch_parts_are_ranges_of_vectors(gpu, oracle, base300, parts, chunk):
    """PA_MSM_BATCH_PARTS (read once per process, hence a subprocess): five
    vectors in 2, 3 or 5 parts of unequal vector counts, their reductions and
    Horner grids on the side streams; small chunks put most buckets across
    several chunks and cut chunks at the parts' boundaries.  Same points."""
    import subprocess
    import sys
    import tempfile
    p, sets, sums = base300
    g = rng(455)
    s = np.stack(sets + [random_scalars(g, 300), np.zeros((300, 4), np.uint64)])
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    code = ("import sys, numpy as np; sys.path.insert(0, %r); import pairing_amd as pa; d = sys.argv[1]; "
            "b = pa.g1_msm_prepare(np.load(d + '/p.npy')); "
            "np.save(d + '/o.npy', pa.g1_multiexp_prepared_batch(b, np.load(d + '/s.npy'))); b.close()" % root)
    with tempfile.TemporaryDirectory() as d:
        np.save(os.path.join(d, "p.npy"), p)
        np.save(os.path.join(d, "s.npy"), s)
        env = dict(os.environ, PA_MSM_BATCH_PARTS=parts, PA_MSM_CHUNK=chunk)
        r = subprocess.run([sys.executable, "-c", code, d], env=env, capture_output=True, text=True, timeout=240)
        assert r.returncode == 0, r.stderr[-3000:]
        got = np.load(os.path.join(d, "o.npy"))
    assert got.shape == (5, 18)
    for j in range(3):
        assert oracle.g1_eq(got[j:j + 1], sums[j]).all(), j
    assert oracle.g1_eq(got[3:4], oracle.g1_multiexp(p, s[3], NT)).all()
    assert oracle.g1_eq(got[4:5], oracle.g1_multiexp(p[:0], s[4][:0])).all()


def reduced(oracle, s):
    """the scalars mod r as FrRepr rows, and their Montgomery form"""
    r = small_scalars([from_limbs(x) % R_ORDER for x in s.reshape(-1, 4)])
    mont, ok = oracle.fr_from_repr(r)
    assert ok.all()
    return r, mont


@pytest.mark.gpu
@pytest.mark.parametrize("m,k", [(300, 3), (4099, 2)])
def test_montgomery_scalars_give_the_same_words(gpu, oracle, m, k):
    p, s0 = dressed(oracle, m, 460 + m)
    s, mont = reduced(oracle, batch_scalars(s0, k, 465 + m))
    with gpu.g1_msm_prepare(p) as b:
        want = gpu.g1_multiexp_prepared_batch(b, s, count=k)
        got = gpu.g1_multiexp_prepared_batch(b, mont, count=k, montgomery=True)
    np.testing.assert_array_equal(got, want)
    assert oracle.g1_eq(want[k - 1:k], oracle.g1_multiexp(p, s[(k - 1) * m:], NT)).all()


@pytest.mark.gpu
def test_ntt_to_commit_chain_stays_on_the_device(gpu, oracle, base300):
    """What the flag exists for: pdev.fr_ntt writes Montgomery rows, and the
    batch commits to them where they lie"""
    import torch
    import pairing_amd.device as pdev
    p = base300[0]
    log_n, k = 8, 3
    m = 1 << log_n
    _, coeffs = reduced(oracle, random_scalars(rng(480), k * m))
    dom = gpu.fr_ntt_domain(log_n)
    evals = gpu.fr_ntt(dom, coeffs, "forward")
    b = pdev.msm_prepare(torch.from_numpy(p.view(np.int64)).cuda())
    a = torch.from_numpy(coeffs.view(np.int64)).cuda()
    dev_evals = torch.empty_like(a)
    words = pdev.fr_ntt_workspace_words(dom, k)
    nws = torch.empty(max(words, 1), dtype=torch.int64, device="cuda")
    pdev.fr_ntt(dom, a, dev_evals, "forward", nws if words else None)
    out = pdev.empty_records(k, 18, "cuda")
    ws = pdev.multiexp_prepared_batch_workspace(b, m, k, "cuda")
    pdev.multiexp_prepared_batch(b, dev_evals, m, k, out, ws, montgomery=True)
    torch.cuda.synchronize()
    b.close()
    dom.close()
    np.testing.assert_array_equal(dev_evals.cpu().numpy().view(np.uint64), evals)
    s = oracle.fr_into_repr(evals).reshape(k, m, 4)
    assert_rows_match_oracle(oracle, out.cpu().numpy().view(np.uint64), p[:m], s)


@pytest.mark.gpu
def test_batch_device_entry_errors_are_codes_not_aborts(gpu, oracle, base300):
    import torch
    import pairing_amd.device as pdev
    from pairing_amd._native import _lib
    p, sets, sums = base300
    b = pdev.msm_prepare(torch.from_numpy(p.view(np.int64)).cuda())
    n, k = b.len, 3
    s = torch.from_numpy(np.concatenate(sets + [sets[0][:3]]).view(np.int64)).cuda()   # 3 n + 3 rows
    out = pdev.empty_records(k, 18, "cuda")
    ws = pdev.multiexp_prepared_batch_workspace(b, n, k, "cuda")
    query = _lib.pa_g1_multiexp_prepared_batch_workspace_bytes
    entry = _lib.pa_g1_multiexp_prepared_batch_device
    need = int(query(b.handle(), n, k))
    assert 0 < need <= ws.numel()
    assert int(query(b.handle(), n + 1, k)) == 0
    stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    args = (b.handle(), ctypes.c_void_p(s.data_ptr()))
    tail = (ctypes.c_void_p(out.data_ptr()), ctypes.c_void_p(ws.data_ptr()))
    assert entry(*args, n, k, 0, *tail, need - 1, stream) < 0
    assert b"workspace" in _lib.pa_last_error()
    assert entry(*args, n + 1, k, 0, *tail, ws.numel(), stream) < 0
    assert b"prepared bases" in _lib.pa_last_error()
    assert entry(*args, n, k, 2, *tail, ws.numel(), stream) < 0
    assert b"flag" in _lib.pa_last_error()
    # over the 32-bit item limit: a window has at least n items in either
    # pipeline (n or 2 n terms), so k n > 2^32 - 1 puts k W nt over it
    big = (1 << 32) // n + 1
    assert int(query(b.handle(), n, big)) == 0
    assert entry(*args, n, big, 0, *tail, ws.numel(), stream) < 0
    assert b"limit" in _lib.pa_last_error()
    with pytest.raises(ValueError):
        pdev.multiexp_prepared_batch_workspace(b, n, big, "cuda")
    host_out = np.zeros((k, 18), np.uint64)
    hs = np.zeros((4, 4), np.uint64)
    host = _lib.pa_g1_multiexp_prepared_batch
    assert host(b.handle(), hs.ctypes.data_as(ctypes.c_void_p), n + 1, k, 0,
                host_out.ctypes.data_as(ctypes.c_void_p)) < 0
    assert host(b.handle(), hs.ctypes.data_as(ctypes.c_void_p), n, big, 0,
                host_out.ctypes.data_as(ctypes.c_void_p)) < 0
    # and the object still computes a correct batch
    pdev.multiexp_prepared_batch(b, s, n, k, out, ws)
    torch.cuda.synchronize()
    got = out.cpu().numpy().view(np.uint64)
    for j in range(k):
        assert oracle.g1_eq(got[j:j + 1], sums[j]).all()
    b.close()
