"""GPU tests of the lane-pair final exponentiation whose Fq4 squarings keep
their Fq2 squares double-width (tools/pgen/tower2.py: w_sqr2 / w_xi, one
reduction per output): pa_final_exponentiation and pa_pairing_batch under
pa_set_pairing_kernel(1) -- the lane-pair kernels at every size -- bit for
bit against the oracle.  A wave holds 32 pairings, so the sizes are a lone
pair (1), a partly filled second wave (33) and an odd tail (97)."""
import numpy as np
import pytest

from helpers import fq12_one, random_scalars, rng, set_infinity

pytestmark = pytest.mark.gpu


def _records(n, kind):
    """n Fq12 records: random field values with a zero record (f == 0: ok = 0,
    zero output) and the identity mixed in; n = 1: the one record `kind` names"""
    from test_bench_sizes import FQ_TOP, _field_rows
    f = _field_rows(500 + n, n * 12, 6, FQ_TOP, [1]).reshape(n, 72)
    if n == 1:
        if kind == "zero":
            f[0] = 0
        elif kind == "identity":
            f[0] = fq12_one()[0]
        return f, ([0] if kind == "zero" else [])
    zeros = [0, n // 2, n - 1]
    f[zeros] = 0
    f[[1, n - 2]] = fq12_one()
    return f, zeros


@pytest.mark.parametrize("n,kind", [(1, "random"), (1, "zero"), (1, "identity"), (33, "mixed"), (97, "mixed")])
def test_final_exponentiation_lane_pairs_apart_and_in_place(gpu, oracle, n, kind):
    import torch
    import pairing_amd.device as pdev
    from test_bench_sizes import _dev, _host
    f, zeros = _records(n, kind)
    exp, ok_exp = oracle.final_exponentiation(f)
    d_in = _dev(f)
    out = pdev.empty_records(n, 72, "cuda:0")
    ok = torch.empty(n, dtype=torch.uint8, device="cuda:0")
    d_same = _dev(f)
    ok2 = torch.empty(n, dtype=torch.uint8, device="cuda:0")
    gpu.set_pairing_kernel(1)
    try:
        pdev.final_exponentiation(d_in, out, ok)
        pdev.final_exponentiation(d_same, d_same, ok2)
        torch.cuda.synchronize()
    finally:
        gpu.set_pairing_kernel(0)
    got = _host(out)
    np.testing.assert_array_equal(got, exp)
    np.testing.assert_array_equal(_host(d_in), f)
    np.testing.assert_array_equal(_host(d_same), exp)
    okh = ok.cpu().numpy()
    np.testing.assert_array_equal(okh, np.asarray(ok_exp, np.uint8))
    np.testing.assert_array_equal(ok2.cpu().numpy(), okh)
    assert (okh[zeros] == 0).all() and okh.sum() == n - len(zeros)
    assert not got[zeros].any()
    if kind == "identity":
        np.testing.assert_array_equal(got, fq12_one().reshape(1, 72))
    if kind == "mixed":
        np.testing.assert_array_equal(got[[1, n - 2]], np.repeat(fq12_one().reshape(1, 72), 2, axis=0))


def test_pairing_lane_pairs_odd_tail(gpu, oracle):
    """e(P, Q) at 97 pairs on the lane-pair kernels (pairing-only Miller loop,
    then this final exponentiation), a pair at infinity included"""
    n = 97
    g = rng(97)
    p = oracle.g1_mul_generator(random_scalars(g, n), 4)
    q = oracle.g2_mul_generator(random_scalars(g, n), 4)
    set_infinity(p, [n - 1])
    gpu.set_pairing_kernel(1)
    try:
        got = gpu.pairing(p, q)
    finally:
        gpu.set_pairing_kernel(0)
    np.testing.assert_array_equal(got, oracle.pairing(p, q, 4))
