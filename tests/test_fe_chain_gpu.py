"""GPU tests of the final exponentiation's exponent chain: the top of |x| as
7 * 15 inside exp_by_x and the hard part as one sequential chain
(tools/pgen/kernels.py exp_by_x_karabina / hard_part_seq for the generated
kernels, pairing_amd/csrc/pair_quad.h for the lane groups).  The result is the
same power of the same element, so outputs and ok bytes are the oracle's bit
for bit: pa_final_exponentiation on the lane-pair (variant 1) and the one-lane
(variant 3) kernels, apart and in place, and e(P, Q) on those and on the lane
groups (variant 5).  A lane-pair wave holds 32 records, a one-lane wave 64:
the sizes are a lone record (1), a partly filled second lane-pair wave (33)
and an odd tail (97)."""
import numpy as np
import pytest

from helpers import fq12_one, random_scalars, rng, set_infinity

pytestmark = pytest.mark.gpu


def _records(n):
    """n Fq12 records: random field values; from 33 up, all inside the first
    wave, a zero record (f == 0: ok = 0, zero output), the identity and an
    element of the subfield Fq6 (c1 = 0: the easy part gives 1, so every
    exp_by_x squares and decompresses the identity), and a zero record last"""
    from test_bench_sizes import FQ_TOP, _field_rows
    f = _field_rows(700 + n, n * 12, 6, FQ_TOP, [1]).reshape(n, 72)
    if n == 1:
        return f, [], []
    zeros, ones = [0, 7, n - 1], [1, 5, 30]
    f[zeros] = 0
    f[1] = fq12_one().reshape(72)
    f[[5, 30], 36:] = 0          # Fq6 elements
    return f, zeros, ones


@pytest.fixture(scope="module")
def expected(oracle):
    """n -> (records, the oracle's outputs, its ok bytes, zero rows, rows that give one); computed once"""
    out = {}
    for n in (1, 33, 97):
        f, zeros, ones = _records(n)
        exp, ok = oracle.final_exponentiation(f)
        f.setflags(write=False)
        out[n] = (f, exp, np.asarray(ok, np.uint8), zeros, ones)
    return out


@pytest.mark.parametrize("n", [1, 33, 97])
@pytest.mark.parametrize("variant", [1, 3])
def test_final_exponentiation_apart_and_in_place(gpu, expected, variant, n):
    import torch
    import pairing_amd.device as pdev
    from test_bench_sizes import _dev, _host
    f, exp, ok_exp, zeros, ones = expected[n]
    d_in = _dev(f.copy())
    out = pdev.empty_records(n, 72, "cuda:0")
    ok = torch.empty(n, dtype=torch.uint8, device="cuda:0")
    d_same = _dev(f.copy())
    ok2 = torch.empty(n, dtype=torch.uint8, device="cuda:0")
    gpu.set_pairing_kernel(variant)
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
    np.testing.assert_array_equal(okh, ok_exp)
    np.testing.assert_array_equal(ok2.cpu().numpy(), ok_exp)
    assert (okh[zeros] == 0).all() and okh.sum() == n - len(zeros)
    assert not got[zeros].any()
    np.testing.assert_array_equal(got[ones], np.repeat(fq12_one().reshape(1, 72), len(ones), axis=0))


def _pairs(oracle, n):
    g = rng(900 + n)
    p = oracle.g1_mul_generator(random_scalars(g, n), 4)
    q = oracle.g2_mul_generator(random_scalars(g, n), 4)
    set_infinity(p, [n - 1])
    return p, q


@pytest.mark.parametrize("variant,n", [(1, 97), (3, 97), (5, 21), (5, 2100)])
def test_pairing_matches_oracle(gpu, oracle, variant, n):
    """e(P, Q) with one pair at infinity: lane pairs and one lane per pairing
    at an odd tail; the lane groups at 21 pairs (one wave per SIMD) and at
    2100, past the 2048 of one round, which takes their two-wave kernel"""
    p, q = _pairs(oracle, n)
    gpu.set_pairing_kernel(variant)
    try:
        got = gpu.pairing(p, q)
    finally:
        gpu.set_pairing_kernel(0)
    exp = oracle.pairing(p, q, 4)
    np.testing.assert_array_equal(got, exp)
    np.testing.assert_array_equal(got[n - 1:], fq12_one().reshape(1, 72))
