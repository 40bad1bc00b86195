"""pa_multi_pairing_batch[_device]: m independent pairing products per call
(Miller loops over all pairs, the segmented Fq12 product of
kernels_segprod.hip, m final exponentiations, the is_one compare).

The expected value of product j is the oracle's
final_exponentiation(miller_loop(p[seg], g2_prepare(q[seg]))) (mod.rs:40-160),
compared bit for bit; inputs are bench.make_pairs' (an infinity P every 128
rows) with a few Q rows set to infinity.  The argument checks of the Python
layers run without a device."""
import os
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import pytest

from helpers import Q, fq12_one, from_limbs, limbs

gpu_test = pytest.mark.gpu

# short/long threshold of the segmented product (kernels_segprod.hip segprod_serial_max)
SERIAL_MAX = 4
RAGGED = [0, 1, 2, 0] + list(range(3, 21)) + [33, 64, 65, 129, 300, 1, 0]
assert {SERIAL_MAX - 1, SERIAL_MAX, SERIAL_MAX + 1} <= set(RAGGED)


def _threads():
    try:
        n = len(os.sched_getaffinity(0))
    except AttributeError:
        n = os.cpu_count() or 1
    return max(1, min(n, int(os.environ.get("OMP_NUM_THREADS", "16")), 16))


def _dev(a):
    import torch
    return torch.from_numpy(np.array(a, dtype=np.uint64, order="C").view(np.int64)).to("cuda:0")


def _host(t):
    return t.cpu().numpy().view(np.uint64)


def _offsets(lengths):
    return np.concatenate([[0], np.cumsum(lengths)]).astype(np.uint64)


def _pairs(n, seed):
    """bench.make_pairs' rows (an infinity P every 128) with a few Q at infinity too"""
    import bench
    p, q = bench.make_pairs(max(n, 1), 0, seed=seed)
    p, q = p[:n], q[:n]
    q[5::31, :24] = 0
    q[5::31, 12:18] = limbs(pow(2, 384, Q))
    q[5::31, 24] = 1
    return p, q


def _expected(oracle, p, q, offsets):
    """(out, ok, is_one) of every product from the oracle, one miller_loop call per segment"""
    m = len(offsets) - 1
    prep = oracle.g2_prepare(q, _threads()) if len(q) else None

    def miller(j):
        lo, hi = int(offsets[j]), int(offsets[j + 1])
        if lo == hi:
            return fq12_one()[0]
        return oracle.miller_loop(p[lo:hi], prep[lo:hi])

    with ThreadPoolExecutor(_threads()) as ex:
        f = np.stack(list(ex.map(miller, range(m))))
    out, ok = oracle.final_exponentiation(f, _threads())
    is_one = (ok != 0) & (out == fq12_one()).all(axis=1)
    return out, ok, is_one.astype(np.uint8)


_uniform_cache = {}


def _uniform(oracle, k, m=67):
    """k pairs per product, m products: inputs, offsets and the oracle's answer, computed once"""
    if (k, m) not in _uniform_cache:
        p, q = _pairs(k * m, seed=11 + k)
        offsets = _offsets([k] * m)
        for a in (p, q, offsets):
            a.setflags(write=False)
        _uniform_cache[k, m] = (p, q, offsets, _expected(oracle, p, q, offsets))
    return _uniform_cache[k, m]


def _run_device(p, q, offsets, guard=0):
    """the device entry on a workspace of exactly the reported size; with guard > 0 the
    buffer continues past it with a pattern that must survive"""
    import torch
    import pairing_amd.device as pdev
    n, m = p.shape[0], len(offsets) - 1
    dp = _dev(p) if n else torch.zeros((0, 13), dtype=torch.int64, device="cuda:0")
    dq = _dev(q) if n else torch.zeros((0, 25), dtype=torch.int64, device="cuda:0")
    out = pdev.empty_records(m, 72, "cuda:0")
    ok = torch.full((m,), 7, dtype=torch.uint8, device="cuda:0")
    is_one = torch.full((m,), 7, dtype=torch.uint8, device="cuda:0")
    need = pdev.multi_pairing_batch_workspace_words(n, m)
    buf = torch.full((need + guard,), 0x5A5A5A5A5A5A5A5A, dtype=torch.int64, device="cuda:0")
    pdev.multi_pairing_batch(dp, dq, offsets, out, ok, is_one, buf[:need])
    torch.cuda.synchronize()
    if guard:
        assert bool((buf[need:] == 0x5A5A5A5A5A5A5A5A).all()), "the call wrote past the reported workspace size"
    return _host(out), ok.cpu().numpy(), is_one.cpu().numpy(), (_host(dp), _host(dq))


def _check(got, want):
    np.testing.assert_array_equal(got[1], want[1])   # ok
    np.testing.assert_array_equal(got[0], want[0])   # out
    np.testing.assert_array_equal(got[2], want[2])   # is_one


@gpu_test
@pytest.mark.parametrize("k", [1, 2, 3, 4])
def test_uniform_products_match_oracle(gpu, oracle, k):
    """m = 67 products of k pairs: a partial last block past the 64-lane boundary"""
    p, q, offsets, want = _uniform(oracle, k)
    _check(_run_device(p, q, offsets), want)
    assert want[1].all()


@gpu_test
def test_ragged_products_match_oracle(gpu, oracle):
    """empty products first, in the middle and last, every length 1..20 (the short/long
    threshold and its neighbours among them) and a few long ones"""
    offsets = _offsets(RAGGED)
    p, q = _pairs(int(offsets[-1]), seed=5)
    got = _run_device(p, q, offsets)
    _check(got, _expected(oracle, p, q, offsets))
    for j in np.nonzero(np.array(RAGGED) == 0)[0]:
        np.testing.assert_array_equal(got[0][j], fq12_one()[0])
        assert got[1][j] == 1 and got[2][j] == 1


@gpu_test
def test_one_long_product_among_short_ones(gpu, oracle):
    """3001 pairs in one product: the halving levels; equal to the oracle and to
    pa_multi_pairing_device over the same pairs"""
    import torch
    import pairing_amd.device as pdev
    offsets = _offsets([2, 3001, 2])
    p, q = _pairs(3005, seed=17)
    got = _run_device(p, q, offsets)
    _check(got, _expected(oracle, p, q, offsets))
    out = pdev.empty_records(1, 72, "cuda:0")
    ok = torch.zeros(1, dtype=torch.uint8, device="cuda:0")
    work = pdev.empty_records(3001, 72, "cuda:0")
    pdev.multi_pairing(_dev(p[2:3003]), _dev(q[2:3003]), out, ok, work)
    torch.cuda.synchronize()
    assert int(ok.item()) == 1
    np.testing.assert_array_equal(got[0][1], _host(out)[0])


@gpu_test
def test_regime_edges(gpu, oracle):
    """k = 2, m = 2049: 4098 Miller loops (past the lane-group window) and 2049 final
    exponentiations (past one round of the lane groups)"""
    offsets = _offsets([2] * 2049)
    p, q = _pairs(4098, seed=23)
    _check(_run_device(p, q, offsets), _expected(oracle, p, q, offsets))


def _negated(p_row):
    """-P of an affine G1 record: y -> q - y, valid on the Montgomery words too"""
    r = p_row.copy()
    r[6:12] = limbs(Q - from_limbs(p_row[6:12]))
    return r


def _verdict_pairs():
    """(P, Q), (-P, Q): the product is one; and the same with the second Q swapped: it is not"""
    d = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "bench_points.npz"))
    g1, g2 = d["g1"], d["g2"]
    p = np.stack([g1[3], _negated(g1[3])])
    return (p, np.stack([g2[9], g2[9]])), (p, np.stack([g2[9], g2[10]]))


@gpu_test
def test_verdict_single_products(gpu, oracle):
    """e(P, Q) e(-P, Q) == one gives is_one = 1; with another Q it gives is_one = 0, ok = 1"""
    offsets = _offsets([2])
    for (p, q), verdict in zip(_verdict_pairs(), (1, 0)):
        got = _run_device(p, q, offsets)
        _check(got, _expected(oracle, p, q, offsets))
        assert got[1][0] == 1 and got[2][0] == verdict


@gpu_test
@pytest.mark.parametrize("case", ["cancelling", "swapped"])
def test_verdict_inside_a_batch(gpu, oracle, case):
    """the two verdict cases at positions 0, 63, 64 and m - 1 of 130 otherwise random products"""
    m, spots = 130, [0, 63, 64, 129]
    p, q = _pairs(2 * m, seed=41)
    vp, vq = _verdict_pairs()[0 if case == "cancelling" else 1]
    for j in spots:
        p[2 * j:2 * j + 2], q[2 * j:2 * j + 2] = vp, vq
    offsets = _offsets([2] * m)
    got = _run_device(p, q, offsets)
    _check(got, _expected(oracle, p, q, offsets))
    want_one = np.zeros(m, np.uint8)
    if case == "cancelling":
        want_one[spots] = 1
    np.testing.assert_array_equal(got[2], want_one)
    assert got[1].all()


@gpu_test
def test_host_entry_with_and_without_values(gpu, oracle):
    """pairing_amd.multi_pairing_batch on numpy arrays; want_values=False returns the same flags alone"""
    p, q, offsets, want = _uniform(oracle, 3)
    out, ok, is_one = gpu.multi_pairing_batch(p, q, offsets=offsets)
    _check((out, ok.astype(np.uint8), is_one.astype(np.uint8)), want)
    out2, ok2, is_one2 = gpu.multi_pairing_batch(p, q, pairs_per_product=3, want_values=False)
    assert out2 is None
    np.testing.assert_array_equal(ok2, ok)
    np.testing.assert_array_equal(is_one2, is_one)
    vp, vq = _verdict_pairs()[0]
    out3, ok3, is_one3 = gpu.multi_pairing_batch(np.concatenate([vp, p[:3]]), np.concatenate([vq, q[:3]]),
                                                 offsets=[0, 2, 2, 5], want_values=False)
    assert out3 is None and ok3.tolist() == [True, True, True]
    assert is_one3.tolist() == [True, True, bool(want[2][0])]


@gpu_test
def test_inputs_unchanged_and_workspace_exact(gpu, oracle):
    """p and q are bit-identical after the call, and the call stays inside a workspace of
    exactly multi_pairing_batch_workspace_words(n, m)"""
    p, q, offsets, want = _uniform(oracle, 3)
    got = _run_device(p, q, offsets, guard=4096)
    _check(got, want)
    np.testing.assert_array_equal(got[3][0], p)
    np.testing.assert_array_equal(got[3][1], q)


# ---- without a device ----
def test_native_signatures_cover_the_new_entries():
    import ctypes
    from pairing_amd import _native
    for name in ("pa_multi_pairing_batch", "pa_multi_pairing_batch_device",
                 "pa_multi_pairing_batch_workspace_bytes"):
        assert name in _native._SIGS
    assert _native._SIGS["pa_multi_pairing_batch_workspace_bytes"] == [ctypes.c_size_t, ctypes.c_size_t]
    assert _native._lib.pa_multi_pairing_batch_workspace_bytes.restype is ctypes.c_size_t
    assert _native._SIGS["pa_multi_pairing_batch"][3] is ctypes.c_size_t
    assert _native._SIGS["pa_multi_pairing_batch_device"][3] is ctypes.c_size_t


def test_workspace_bytes_exact_and_monotone():
    from pairing_amd._native import _lib
    ws = _lib.pa_multi_pairing_batch_workspace_bytes
    # the Miller values, the products and the m + 1 staged offsets
    assert ws(10, 4) == 576 * 10 + 576 * 4 + 8 * 5
    assert ws(1 << 33, 1 << 32) == 576 * (1 << 33) + 576 * (1 << 32) + 8 * ((1 << 32) + 1)
    for n, m in ((0, 0), (0, 3), (7, 1), (1000, 1000)):
        assert ws(n + 1, m) > ws(n, m) and ws(n, m + 1) > ws(n, m)


@pytest.mark.parametrize("offsets,what", [([1, 2, 4], r"offsets\[0\]"), ([0, 3, 2, 4], "non-decreasing")])
def test_c_abi_rejects_bad_offsets_before_any_launch(offsets, what):
    """both C entries validate the host offsets first (PA_ERR_INVALID_ARGUMENT = -1 with a
    message), so this needs no device; the buffers are host arrays nothing dereferences"""
    from pairing_amd._native import PairingError, call, ptr
    o = np.array(offsets, np.uint64)
    m = len(o) - 1
    p, q = np.zeros((4, 13), np.uint64), np.zeros((4, 25), np.uint64)
    out, ok, is_one = np.zeros((m, 72), np.uint64), np.zeros(m, np.uint8), np.zeros(m, np.uint8)
    with pytest.raises(PairingError, match=r"\(-1\).*" + what):
        call("pa_multi_pairing_batch", ptr(p), ptr(q), ptr(o), m, ptr(out), ptr(ok), ptr(is_one))
    with pytest.raises(PairingError, match=r"\(-1\).*" + what):
        call("pa_multi_pairing_batch_device", ptr(p), ptr(q), ptr(o), m, ptr(out), ptr(ok), ptr(is_one),
             ptr(np.zeros(8, np.uint64)), None)


BAD_OFFSETS = [
    ([1, 2, 4], "start at 0"),
    ([0, 3, 2, 4], "non-decreasing"),
    ([0, 2, 3], "last offset"),
    ([0, 2, 5], "last offset"),
    ([[0, 2], [2, 4]], "1-d"),
    ([0.0, 2.0, 4.0], "integer"),
    ([0, -1, 4], "negative"),
]


@pytest.mark.parametrize("offsets,what", BAD_OFFSETS)
def test_host_layer_rejects_bad_offsets(offsets, what):
    import pairing_amd
    p, q = np.zeros((4, 13), np.uint64), np.zeros((4, 25), np.uint64)
    with pytest.raises(ValueError, match=what):
        pairing_amd.multi_pairing_batch(p, q, offsets=np.array(offsets))


def test_host_layer_offsets_or_uniform_k():
    import pairing_amd
    p, q = np.zeros((4, 13), np.uint64), np.zeros((4, 25), np.uint64)
    with pytest.raises(ValueError, match="exactly one"):
        pairing_amd.multi_pairing_batch(p, q)
    with pytest.raises(ValueError, match="exactly one"):
        pairing_amd.multi_pairing_batch(p, q, offsets=[0, 4], pairs_per_product=2)
    with pytest.raises(ValueError, match="do not split"):
        pairing_amd.multi_pairing_batch(p, q, pairs_per_product=3)
    with pytest.raises(ValueError, match="do not split"):
        pairing_amd.multi_pairing_batch(p, q, pairs_per_product=0)


@pytest.mark.parametrize("offsets,what", BAD_OFFSETS)
def test_device_layer_rejects_bad_offsets(offsets, what):
    import torch
    import pairing_amd.device as pdev
    z = lambda *s, dt=torch.int64: torch.zeros(*s, dtype=dt)  # noqa: E731
    for off in (np.array(offsets), torch.tensor(offsets)):
        with pytest.raises(ValueError, match=what):
            pdev.multi_pairing_batch(z(4, 13), z(4, 25), off, z(2, 72), z(2, dt=torch.uint8),
                                     z(2, dt=torch.uint8), z(1 << 12))


def test_device_layer_rejects_undersized_buffers():
    import torch
    import pairing_amd.device as pdev
    z = lambda *s, dt=torch.int64: torch.zeros(*s, dtype=dt)  # noqa: E731
    off = torch.tensor([0, 1, 4, 4])
    need = pdev.multi_pairing_batch_workspace_words(4, 3)
    assert need == (576 * 7 + 8 * 4) // 8
    flags = lambda k: z(k, dt=torch.uint8)  # noqa: E731
    with pytest.raises(ValueError, match="work"):
        pdev.multi_pairing_batch(z(4, 13), z(4, 25), off, z(3, 72), flags(3), flags(3), z(need - 1))
    with pytest.raises(ValueError, match="out"):
        pdev.multi_pairing_batch(z(4, 13), z(4, 25), off, z(2, 72), flags(3), flags(3), z(need))
    with pytest.raises(ValueError, match="ok"):
        pdev.multi_pairing_batch(z(4, 13), z(4, 25), off, z(3, 72), flags(2), flags(3), z(need))
    with pytest.raises(ValueError, match="is_one"):
        pdev.multi_pairing_batch(z(4, 13), z(4, 25), off, z(3, 72), flags(3), flags(2), z(need))
    with pytest.raises(ValueError, match="q"):
        pdev.multi_pairing_batch(z(4, 13), z(3, 25), off, z(3, 72), flags(3), flags(3), z(need))
    # well-sized host tensors pass the size checks and stop at the device-pointer check
    with pytest.raises(ValueError, match="CUDA"):
        pdev.multi_pairing_batch(z(4, 13), z(4, 25), off, z(3, 72), flags(3), flags(3), z(need))
