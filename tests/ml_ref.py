"""A big-integer model of G2Prepared::from_affine and Bls12::miller_loop for one
pair, written formula by formula from the reference (src/bls12_381/mod.rs:
40-102 the loop and ell, 176-245 doubling_step, 247-333 addition_step): plain
residues mod q, no Montgomery form and no lazy reduction, the Fq12 part on
the schoolbook tower of pymodel.  It pins the C oracle where the reference's
known-answer vectors do not reach: points outside the subgroups and field
elements that are no curve point at all (tests/test_pairing_domain.py).

Points are (x, y) with Fq ints (G1) or Fq2 pairs (G2), or None for infinity.
"""
import numpy as np

from helpers import Q, R_ORDER, mont
from pymodel import (F2ONE, F2ZERO, F12ONE, f2add, f2mul, f2neg, f2sub, f12conj, f12mul, f12pow, f12sqr,
                     fq12_to_limbs)

BLS_X = 0xd201000000010000          # mod.rs:23; BLS_X_IS_NEGATIVE
X_BITS = bin(BLS_X >> 1)[3:]         # the bits of BLS_X >> 1 below its leading one
NUM_COEFFS = 68


def _sq(a):
    return f2mul(a, a)


def _dbl(a):
    return f2add(a, a)


def doubling_step(r):
    """mod.rs:176-245; r = [x, y, z] is updated in place"""
    tmp0 = _sq(r[0])
    tmp1 = _sq(r[1])
    tmp2 = _sq(tmp1)
    tmp3 = _dbl(f2sub(f2sub(_sq(f2add(tmp1, r[0])), tmp0), tmp2))
    tmp4 = f2add(_dbl(tmp0), tmp0)
    tmp6 = f2add(r[0], tmp4)
    tmp5 = _sq(tmp4)
    zsquared = _sq(r[2])
    r[0] = f2sub(f2sub(tmp5, tmp3), tmp3)
    r[2] = f2sub(f2sub(_sq(f2add(r[2], r[1])), tmp1), zsquared)
    r[1] = f2mul(f2sub(tmp3, r[0]), tmp4)
    tmp2 = _dbl(_dbl(_dbl(tmp2)))
    r[1] = f2sub(r[1], tmp2)
    tmp3 = f2neg(_dbl(f2mul(tmp4, zsquared)))
    tmp6 = f2sub(f2sub(_sq(tmp6), tmp0), tmp5)
    tmp1 = _dbl(_dbl(tmp1))
    tmp6 = f2sub(tmp6, tmp1)
    tmp0 = _dbl(f2mul(r[2], zsquared))
    return (tmp0, tmp3, tmp6)


def addition_step(r, q):
    """mod.rs:247-333; q = (x, y) affine"""
    qx, qy = q
    zsquared = _sq(r[2])
    ysquared = _sq(qy)
    t0 = f2mul(zsquared, qx)
    t1 = f2mul(f2sub(f2sub(_sq(f2add(qy, r[2])), ysquared), zsquared), zsquared)
    t2 = f2sub(t0, r[0])
    t3 = _sq(t2)
    t4 = _dbl(_dbl(t3))
    t5 = f2mul(t4, t2)
    t6 = f2sub(f2sub(t1, r[1]), r[1])
    t9 = f2mul(t6, qx)
    t7 = f2mul(t4, r[0])
    r[0] = f2sub(f2sub(f2sub(_sq(t6), t5), t7), t7)
    r[2] = f2sub(f2sub(_sq(f2add(r[2], t2)), zsquared), t3)
    t10 = f2add(qy, r[2])
    t8 = f2mul(f2sub(t7, r[0]), t6)
    t0 = _dbl(f2mul(r[1], t5))
    r[1] = f2sub(t8, t0)
    t10 = f2sub(_sq(t10), ysquared)
    ztsquared = _sq(r[2])
    t10 = f2sub(t10, ztsquared)
    t9 = f2sub(_dbl(t9), t10)
    t10 = _dbl(r[2])
    t6 = f2neg(t6)
    t1 = _dbl(t6)
    return (t10, t1, t9)


def g2_prepare(q):
    """G2Prepared::from_affine (mod.rs:168-358): the 68 line coefficients, or
    None for the point at infinity"""
    if q is None:
        return None
    r = [q[0], q[1], F2ONE]
    coeffs = []
    for bit in X_BITS:
        coeffs.append(doubling_step(r))
        if bit == "1":
            coeffs.append(addition_step(r, q))
    coeffs.append(doubling_step(r))
    assert len(coeffs) == NUM_COEFFS
    return coeffs


def _ell(f, c, p):
    """mod.rs:57-69: f.mul_by_014(c2, c1 * p.x, c0 * p.y), the sparse factor
    written out as a full Fq12 element (c0 + c1 v) + (c4 v) w"""
    c0 = (c[0][0] * p[1] % Q, c[0][1] * p[1] % Q)
    c1 = (c[1][0] * p[0] % Q, c[1][1] * p[0] % Q)
    return f12mul(f, ((c[2], c1, F2ZERO), (F2ZERO, c0, F2ZERO)))


def miller_loop(p, coeffs):
    """Bls12::miller_loop([(p, prepared)]) (mod.rs:40-102)"""
    if p is None or coeffs is None:
        return F12ONE
    it = iter(coeffs)
    f = F12ONE
    for bit in X_BITS:
        f = _ell(f, next(it), p)
        if bit == "1":
            f = _ell(f, next(it), p)
        f = f12sqr(f)
    f = _ell(f, next(it), p)
    return f12conj(f)


def final_exponentiation(f):
    """mod.rs:104-160 by its meaning: None for 0, else f^(3 (q^12 - 1) / r)
    (tests/test_oracle.py test_final_exponentiation_is_the_fixed_power)"""
    if f == (((0, 0),) * 3,) * 2:
        return None
    return f12pow(f, 3 * (Q ** 12 - 1) // R_ORDER)


def prepared_record(coeffs):
    """the ABI pa_g2_prepared record (68 x 36 Montgomery words + the infinity word)"""
    if coeffs is None:
        return np.array([0] * (NUM_COEFFS * 36) + [1], np.uint64)
    ws = []
    for c in coeffs:
        for f2 in c:
            ws += mont(f2[0]) + mont(f2[1])
    return np.array(ws + [0], np.uint64)


def fq12_record(f):
    return np.array(fq12_to_limbs(f), np.uint64)
