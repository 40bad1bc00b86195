"""Plain big-integer references of the Miller loop's steps, one function per
unit program of tools/pgen/unit_progs.ml_step_prog (tests/test_ml_steps.py,
tests/test_ml_steps_gpu.py).  Pure Python over tests/pymodel.py.

A record is 12 canonical ABI integers (Montgomery, R = 2^384): Fq2 number k
is (record[2k], record[2k + 1]).  `reference(which, record, pairing_only)`
maps the record to the plain residues, runs the step and maps the 12 results
back, so it compares with dsl.evaluate and with the GPU word for word.

The reference-form steps and ell are fl_ref's restatements of mod.rs
(doubling_step, addition_step, ell).  The homogeneous steps of the
pairing-only kernels (kernels.doubling_step_h / addition_step_h) have no
counterpart in the reference: they are written here from the closed formulas
of their docstrings (Costello-Lange-Naehrig, eprint 2009/615, on
E': y^2 = x^3 + b', b' = 4 (1 + u), scaled by 4), not from the kernels'
operation order; tests/test_ml_steps.py ties them to the reference forms on
curve points.
"""
import fl_ref
import pymodel as pm
from helpers import Q, RINV, RMONT

B_TWIST = (4, 4)                      # b' = 4 (1 + u)
ITER_TRIPS = 3
ITER_ADD = (False, True, False)       # the addition step: skipped, taken, skipped


def _k(a, k):
    return fl_ref.f2scale(a, k % Q)


def doubling_step_h(r):
    """(X, Y, Z) homogeneous on E' -> (2 R, the tangent's (c0, c1, c2)):
        X3 = 2 X Y (Y^2 - 9 b' Z^2)       c0 = 2 Y Z
        Y3 = (Y^2 + 9 b' Z^2)^2 - 108 b'^2 Z^4      c1 = -3 X^2
        Z3 = 8 Y^3 Z                       c2 = Y^2 - 3 b' Z^2"""
    m, sq = pm.f2mul, fl_ref.f2sqr
    x, y, z = r
    yy, bzz = sq(y), m(B_TWIST, sq(z))
    x3 = _k(m(m(x, y), pm.f2sub(yy, _k(bzz, 9))), 2)
    y3 = pm.f2sub(sq(pm.f2add(yy, _k(bzz, 9))), _k(sq(bzz), 108))
    z3 = _k(m(m(yy, y), z), 8)
    return (x3, y3, z3), (_k(m(y, z), 2), _k(sq(x), -3), pm.f2sub(yy, _k(bzz, 3)))


def addition_step_h(r, q):
    """(X1, Y1, Z1) homogeneous, q = (x2, y2) affine -> (R + Q, the chord's
    (c0, c1, c2)), theta = Y1 - y2 Z1, lambda = X1 - x2 Z1:
        X3 = lambda H,  H = lambda^3 + Z1 theta^2 - 2 X1 lambda^2
        Y3 = theta (X1 lambda^2 - H) - Y1 lambda^3
        Z3 = Z1 lambda^3
        c0 = lambda, c1 = -theta, c2 = theta x2 - lambda y2"""
    m, sq = pm.f2mul, fl_ref.f2sqr
    (x1, y1, z1), (x2, y2) = r, q
    th = pm.f2sub(y1, m(y2, z1))
    la = pm.f2sub(x1, m(x2, z1))
    la2 = sq(la)
    la3 = m(la2, la)
    h = pm.f2sub(pm.f2add(la3, m(z1, sq(th))), _k(m(x1, la2), 2))
    x3 = m(la, h)
    y3 = pm.f2sub(m(th, pm.f2sub(m(x1, la2), h)), m(y1, la3))
    return (x3, y3, m(z1, la3)), (la, pm.f2neg(th), pm.f2sub(m(th, x2), m(la, y2)))


def steps(pairing_only):
    """(doubling step, addition step), each returning (r', (c0, c1, c2))"""
    return (doubling_step_h, addition_step_h) if pairing_only else (fl_ref.doubling_step, fl_ref.addition_step)


# ---- records ----
def plain(record):
    """the six Fq2 of a record as plain residues"""
    xs = [x * RINV % Q for x in record]
    return [(xs[2 * k], xs[2 * k + 1]) for k in range(6)]


def record_of(f2s):
    """six plain Fq2 -> the 12 ABI integers"""
    return [c % Q * RMONT % Q for x in f2s for c in x]


def _f12(xs):
    return ((xs[0], xs[1], xs[2]), (xs[3], xs[4], xs[5]))


def _flat12(f):
    return [x for c6 in f for x in c6]


def reference(which, record, pairing_only=False):
    """the 12 ABI integers unit_progs.ml_step_prog(which, pairing_only=...)
    stores for this record (its slot map is in that function's docstring)"""
    xs = plain(record)
    dbl, add = steps(pairing_only)
    if which == "dbl":
        r, c = dbl((xs[0], xs[1], xs[2]))
        out = list(c) + list(r)
    elif which == "add":
        r, c = add((xs[0], xs[1], xs[2]), (xs[3], xs[4]))
        out = list(c) + list(r)
    elif which == "ell":
        c = (pm.f2add(xs[3], xs[2]), xs[4], xs[5])
        out = _flat12(fl_ref.ell(_f12(xs), c, xs[0]))
    elif which == "sqr12":
        out = _flat12(pm.f12sqr(_f12(xs)))
    elif which == "mul12":
        out = _flat12(pm.f12mul(_f12(xs), _f12(xs[1:] + xs[:1])))
    elif which == "iter":
        p, q, r, f = xs[0], (xs[1], xs[2]), (xs[3], xs[4], xs[5]), _f12(xs)
        for taken in ITER_ADD:
            r, c = dbl(r)
            f = fl_ref.ell(f, c, p)
            if taken:
                r, c = add(r, q)
                f = fl_ref.ell(f, c, p)
            f = pm.f12sqr(f)
        r, c = dbl(r)
        out = _flat12(pm.f12conj(fl_ref.ell(f, c, p)))
    else:
        raise ValueError(which)
    return record_of(out)
