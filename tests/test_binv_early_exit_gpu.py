"""GPU tests of the binary-GCD inversions' early exit (the generated kernels'
wave-uniform exit, emit.Emitter.emit_binv; bgcd.h's per-lane exit): waves
whose lanes converge at different rounds, all-zero waves, a lone active
lane, and the library entry points that run the inversions, bit for bit
against the DSL model and the oracle."""
import functools
import os
import random
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (os.path.join(ROOT, "tools", "pgen"), os.path.join(ROOT, "tools")):
    if p not in sys.path:
        sys.path.insert(0, p)

import unit_progs  # noqa: E402

pytestmark = pytest.mark.gpu


@functools.lru_cache(maxsize=None)
def _sample():
    import test_binv_early_exit as te
    return te.sample_rows(unit_progs.unit_prog())


def _mixed_wave(g, slow_lane):
    """64 records: one highest-round value at slow_lane, zeros (both inversions
    see 0) at the even and lowest-round values at the odd other lanes"""
    import test_binv_early_exit as te
    s = _sample()
    rows = [te._zero_row(g) if k % 2 == 0 else list(s["lo"][1]) for k in range(64)]
    rows[slow_lane] = list(s["hi"][1])
    return rows


@pytest.mark.parametrize("n", [64, 65, 128])
def test_tunit_waves_with_one_slow_lane(n):
    """tunit (two inversions per lane).  64 rows: the slow value at lane 0;
    65: at lane 63, and the 65th row alone in its wave (a slow value: the
    inactive lanes neither hold the loop open nor end it early); 128: a wave
    of zeros, then a wave with the slow value at lane 63"""
    import test_binv_early_exit as te
    from test_gen_units import _run
    g = random.Random(n)
    if n == 64:
        rows = _mixed_wave(g, 0)
    elif n == 65:
        rows = _mixed_wave(g, 63) + [list(_sample()["hi"][1])]
    else:
        rows = [te._zero_row(g) for _ in range(64)] + _mixed_wave(g, 63)
    assert len(rows) == n
    gpu, model = _run("tunit", unit_progs.unit_prog(), rows)
    for k in range(n):
        assert gpu[k] == model[k], "row %d" % k


@functools.lru_cache(maxsize=None)
def _elements():
    import pymodel as pm
    import test_pgen as tp
    return [tp._abi_words(f) for f in [tp._cyclotomic(s) for s in range(30, 38)] + [tp._b0_zero_element(), pm.F12ONE]]


@pytest.mark.parametrize("n", [32, 33])
def test_tdec2_lane_pairs_full_wave_and_lone_pair(n):
    """tdec2 (lane pairs, 32 rows per wave): random cyclotomic elements, the
    b0 = 0 element and the identity (inversion input 0) mixed in one wave, and
    a 33rd row alone in its wave; each row is itself after decompression"""
    from test_gen_units import _run
    el = _elements()
    rows = [list(el[(3 * k + n) % len(el)]) for k in range(n)]
    gpu, model = _run("tdec2", unit_progs.dec_prog(lanes=2), rows, lanes=2, ws_slots=64)
    for k in range(n):
        assert gpu[k] == rows[k], "row %d" % k
    assert model == rows


@pytest.mark.parametrize("n,variant", [(2305, 0), (2305, 1), (4099, 0)],
                         ids=["2305_default_lane_groups", "2305_lane_pairs", "4099_default_lane_pairs"])
def test_final_exponentiation_apart_and_in_place(gpu, oracle, n, variant):
    """pa_final_exponentiation, zero records included (ok = 0, zero out), equal
    to the oracle with out apart from in and in place.  The default selection
    runs the lane-group kernels (pair_quad.h, a bgcd.h user) at 2 305 and the
    generated lane-pair kernel from 4 097 on; variant 1 is the lane-pair
    kernel at 2 305 too."""
    import torch
    import pairing_amd.device as pdev
    from test_bench_sizes import FQ_TOP, _dev, _field_rows, _host, _threads
    f = _field_rows(70 + n % 13, n * 12, 6, FQ_TOP, [1]).reshape(n, 72)
    zeros = [0, 63, 64, n // 2, n - 1]
    f[zeros] = 0
    exp, ok_exp = oracle.final_exponentiation(f, _threads())
    d_in = _dev(f)
    out = pdev.empty_records(n, 72, "cuda:0")
    ok = torch.empty(n, dtype=torch.uint8, device="cuda:0")
    d_same = _dev(f)
    ok2 = torch.empty(n, dtype=torch.uint8, device="cuda:0")
    gpu.set_pairing_kernel(variant)
    try:
        pdev.final_exponentiation(d_in, out, ok)
        pdev.final_exponentiation(d_same, d_same, ok2)
        torch.cuda.synchronize()
    finally:
        gpu.set_pairing_kernel(0)
    np.testing.assert_array_equal(_host(out), exp)
    np.testing.assert_array_equal(_host(d_in), f)
    np.testing.assert_array_equal(_host(d_same), exp)
    okh = ok.cpu().numpy()
    np.testing.assert_array_equal(okh, np.asarray(ok_exp, np.uint8))
    np.testing.assert_array_equal(ok2.cpu().numpy(), okh)
    assert (okh[zeros] == 0).all() and okh.sum() == n - len(zeros)


def test_g1_batch_normalization_uses_the_early_exit(gpu, oracle):
    """one bgcd.h user: G1 batch normalization at 4 099 points (zeros and
    already normalized points mixed in) against the oracle"""
    from test_gpu_parity import _jacobian_points
    n = 4099
    v = _jacobian_points(oracle, 77, n)
    np.testing.assert_array_equal(gpu.g1_batch_normalization(v), oracle.g1_batch_normalization(v))
