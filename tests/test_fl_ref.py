"""The big-integer restatements of tests/fl_ref.py (group law, line steps, ell,
Frobenius, Granger-Scott) checked once against the C oracle on canonical
inputs, so that tests/test_fl_unit.py compares the lazy kernels with a
reference that is itself pinned.  CPU only."""
import random

import numpy as np

import fl_ref as R
import pymodel as pm
from helpers import Q, mont, random_scalars, rng, unmont


def _f2(ws):
    return (unmont(ws[:6]), unmont(ws[6:12]))


def _g1j(row):
    return tuple(unmont(row[6 * k:6 * k + 6]) for k in range(3))


def _g2j(row):
    return tuple(_f2(row[12 * k:12 * k + 12]) for k in range(3))


def _g1row(p):
    return sum((mont(c) for c in p), [])


def _g2row(p):
    return sum((mont(c) for f in p for c in f), [])


def test_group_law_restatement_matches_oracle(oracle):
    g = rng(5)
    s = random_scalars(g, 6)
    a1 = oracle.g1_mul_generator(s)
    j1 = oracle.g1_mul_generator_jacobian(s)
    a2 = oracle.g2_mul_generator(s)
    j2 = oracle.g2_from_affine(a2)
    j2 = oracle.g2_add(j2, oracle.g2_double(j2))     # z != 1
    for F, jac, aff, dbl, add, madd, frow, fjac, w in (
            (R.Fp, j1, a1, oracle.g1_double, oracle.g1_add, oracle.g1_add_mixed, _g1row, _g1j, 6),
            (R.Fp2, j2, a2, oracle.g2_double, oracle.g2_add, oracle.g2_add_mixed, _g2row, _g2j, 12)):
        pts = [fjac(r) for r in jac]
        affs = [fjac(np.concatenate([r[:2 * w], r[:w]]))[:2] for r in aff]     # (x, y) of an affine record
        got = dbl(jac)
        for k, p in enumerate(pts):
            assert fjac(got[k]) == R.jac_double(F, p)
        rot = np.roll(jac, 1, axis=0)
        got = add(jac, rot)
        for k, p in enumerate(pts):
            assert fjac(got[k]) == R.jac_add(F, p, pts[k - 1])
        got = add(jac, jac)                            # equal points double
        for k, p in enumerate(pts):
            assert fjac(got[k]) == R.jac_add(F, p, p) == R.jac_double(F, p)
        got = madd(jac, np.roll(aff, 1, axis=0))
        for k, p in enumerate(pts):
            assert fjac(got[k]) == R.jac_add_mixed(F, p, affs[k - 1])
        # P + (-P): z = 0
        neg = np.array([frow((p[0], F.neg(p[1]), p[2])) for p in pts], np.uint64)
        got = add(jac, neg)
        for k, p in enumerate(pts):
            want = R.jac_add(F, p, (p[0], F.neg(p[1]), p[2]))
            assert fjac(got[k]) == want and want[2] == F.zero


def test_line_steps_and_ell_restatement_match_oracle(oracle):
    g = rng(6)
    s = random_scalars(g, 2)
    q = oracle.g2_mul_generator(s)
    p = oracle.g1_mul_generator(s[::-1].copy())
    prep = oracle.g2_prepare(q)
    fs = oracle.miller_loop_batch(p, prep)
    for k in range(2):
        qa = (_f2(q[k, :12]), _f2(q[k, 12:24]))
        coeffs = R.g2_prepare(qa)
        assert len(coeffs) == 68
        want = [tuple(_f2(prep[k, 36 * i + 12 * j:36 * i + 12 * j + 12]) for j in range(3)) for i in range(68)]
        assert coeffs == want
        pa = (unmont(p[k, :6]), unmont(p[k, 6:12]))
        assert R.miller_loop(pa, coeffs) == pm.fq12_from_limbs(fs[k])


def test_frobenius_and_granger_scott_restatements(oracle):
    g = random.Random(8)
    f = tuple(tuple((g.randrange(Q), g.randrange(Q)) for _ in range(3)) for _ in range(2))
    row = np.array([pm.fq12_to_limbs(f)], np.uint64)
    for power in range(12):
        assert R.f12frob(f, power) == pm.fq12_from_limbs(oracle.fq12_frobenius(row, power)[0])
    assert R.f12frob(f, 1) == pm.f12pow(f, Q)          # from the definition
    c = R.cyclotomic(f)
    assert R.gs_sqr(c) == pm.f12sqr(c)
    assert R.gs_sqr(f) != pm.f12sqr(f)
    c0, c1, c4 = ((g.randrange(Q), g.randrange(Q)) for _ in range(3))
    lim = lambda a: np.array([mont(a[0]) + mont(a[1])], np.uint64)  # noqa: E731
    assert R.mul_by_014(f, c0, c1, c4) == pm.fq12_from_limbs(oracle.fq12_mul_by_014(row, lim(c0), lim(c1), lim(c4))[0])
