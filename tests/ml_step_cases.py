"""The records the Miller loop's unit programs run on (tests/test_ml_steps.py,
tests/test_ml_steps_gpu.py): one deterministic list of labelled structured
records plus seeded random ones, every program taking every record.

A record is 12 canonical ABI integers (Montgomery, R = 2^384; R mod q stands
for 1), Fq2 number k = (record[2k], record[2k + 1]); over lane pairs lane 0
holds the even and lane 1 the odd coordinate.  What the six Fq2 mean depends
on the program (unit_progs.ml_step_prog):

    dbl   R = (Fq2 0, 1, 2)
    add   R = (Fq2 0, 1, 2), Q = (Fq2 3, 4)
    ell   f = all, P packed in Fq2 0, c0 = Fq2 3 + Fq2 2, c1 = Fq2 4, c2 = Fq2 5
    iter  P packed in Fq2 0, Q = (Fq2 1, 2), R = (Fq2 3, 4, 5), f = all

so the cases built for one layout are just further operands to the others.
The all-zero record is the kernel config's "None" input (the epilogue
writes zeros over the result) and is never in the list.  Pure Python ints.
"""
import functools
import random

import decode_cases as D
import pymodel as pm
from helpers import Q, RMONT

# coefficients a carry, a select or a zero test can get wrong: the ends of the
# range, the middle, Montgomery one, and every limb full (2^380 - 1 < q)
COEFFS = (0, 1, 2, Q - 1, Q - 2, (Q - 1) // 2, RMONT, (1 << 380) - 1)
assert all(0 <= c < Q for c in COEFFS)


def _m(x):
    return x % Q * RMONT % Q


def _rec(f2s):
    """six plain Fq2 -> record"""
    return [_m(c) for x in f2s for c in x]


def _rand2(g):
    return (g.randrange(Q), g.randrange(Q))


def _jac(pt, z):
    """the affine point as Jacobian (x z^2, y z^3, z)"""
    zz = pm.f2mul(z, z)
    return (pm.f2mul(pt[0], zz), pm.f2mul(pt[1], pm.f2mul(zz, z)), z)


def _hom(pt, z):
    """the affine point as homogeneous (x z, y z, z)"""
    return (pm.f2mul(pt[0], z), pm.f2mul(pt[1], z), z)


def _neg(pt):
    return (pt[0], pm.f2neg(pt[1]))


@functools.lru_cache(maxsize=None)
def curve_points():
    """on-curve G2 material: the named points of pairing_domain_cases (in the
    subgroup, a plain curve point, small order) and a G1 point for P"""
    import pairing_domain_cases as pdc
    pts = pdc.points()
    return {"q": pts["q"]["subgroup"], "q_curve": pts["q"]["curve"], "q13": pts["q"]["order13"],
            "p": pts["p"]["subgroup"]}


@functools.lru_cache(maxsize=None)
def _structured():
    g = random.Random(20240)
    out = []

    def add(label, rec):
        rec = [int(x) for x in rec]
        assert len(rec) == 12 and all(0 <= x < Q for x in rec) and any(rec), label
        out.append((label, rec))

    # ---- raw coefficients (record integers, whatever they stand for) ----
    for c in COEFFS[1:]:
        add("all coeff %d" % COEFFS.index(c), [c] * 12)
    for c in COEFFS:
        add("c0 = coeff %d" % COEFFS.index(c), [c if i % 2 == 0 else g.randrange(Q) for i in range(12)])
        add("c1 = coeff %d" % COEFFS.index(c), [c if i % 2 == 1 else g.randrange(Q) for i in range(12)])
    for s in range(0, 8, 2):
        add("coeffs rotated by %d" % s, [COEFFS[(i + s) % 8] for i in range(12)])
    xs = [g.randrange(Q) for _ in range(6)]
    add("c0 = c1 (equal lanes)", [xs[i // 2] for i in range(12)])
    add("c0 = -c1", [xs[i // 2] if i % 2 == 0 else Q - xs[i // 2] for i in range(12)])
    x = g.randrange(Q)
    add("one value everywhere (equal lanes)", [x] * 12)
    add("one Fq2 everywhere", [x, g.randrange(Q)] * 6)
    # ---- f ----
    add("f = 1", _rec([(1, 0)] + [(0, 0)] * 5))
    for k in range(6):
        add("f sparse: Fq2 %d only" % k, _rec([_rand2(g) if i == k else (0, 0) for i in range(6)]))
    add("P = (0, 0)", _rec([(0, 0)] + [_rand2(g) for _ in range(5)]))
    add("P = (0, 0), equal lanes", [0, 0] + [xs[i // 2] for i in range(2, 12)])

    cp = curve_points()
    qa, qc, q13 = cp["q"], cp["q_curve"], cp["q13"]
    one, zero = (1, 0), (0, 0)
    # ---- dbl layout: R = (Fq2 0, 1, 2) ----
    tail = lambda: [_rand2(g) for _ in range(3)]  # noqa: E731
    add("dbl: y = 0", _rec([_rand2(g), zero, _rand2(g)] + tail()))
    add("dbl: x = 0", _rec([zero, _rand2(g), _rand2(g)] + tail()))
    add("dbl: Z = 0", _rec([_rand2(g), _rand2(g), zero] + tail()))
    add("dbl: x = y = 0", _rec([zero, zero, _rand2(g)] + tail()))
    add("dbl: R on E', Z = 1", _rec(list(_jac(qa, one)) + tail()))
    z = _rand2(g)
    add("dbl: R on E', Jacobian", _rec(list(_jac(qc, z)) + tail()))
    add("dbl: R on E', homogeneous", _rec(list(_hom(qc, z)) + tail()))
    # ---- add layout: R = (Fq2 0, 1, 2), Q = (Fq2 3, 4) ----
    for name, q in (("Q", qa), ("-Q", _neg(qa))):
        add("add: R = %s, Z = 1" % name, _rec(list(_jac(q, one)) + list(qa) + [_rand2(g)]))
        add("add: R = %s, Jacobian" % name, _rec(list(_jac(q, z)) + list(qa) + [_rand2(g)]))
        add("add: R = %s, homogeneous" % name, _rec(list(_hom(q, z)) + list(qa) + [_rand2(g)]))
    rq = _rand2(g), _rand2(g)
    add("add: R = Q off the curve, Z = 1", _rec([rq[0], rq[1], one, rq[0], rq[1], _rand2(g)]))
    add("add: R = -Q off the curve, Z = 1", _rec([rq[0], pm.f2neg(rq[1]), one, rq[0], rq[1], _rand2(g)]))
    add("add: Z = 0", _rec([_rand2(g), _rand2(g), zero, qa[0], qa[1], _rand2(g)]))
    add("add: Q = (0, 0)", _rec([_rand2(g), _rand2(g), _rand2(g), zero, zero, _rand2(g)]))
    r2 = D._ec_add(D._f2(), qa, qa)
    add("add: R = 2 Q on E', Jacobian", _rec(list(_jac(r2, z)) + list(qa) + [_rand2(g)]))
    add("add: R = 2 Q on E', homogeneous", _rec(list(_hom(r2, z)) + list(qa) + [_rand2(g)]))
    add("add: R = 12 Q = -Q, order 13", _rec(list(_hom(_neg(q13), z)) + list(q13) + [_rand2(g)]))
    # ---- iter layout: P = Fq2 0, Q = (Fq2 1, 2), R = (Fq2 3, 4, 5); f = all ----
    p = cp["p"]
    add("iter: R = Q, Z = 1 (the loop's start)", _rec([p, qa[0], qa[1]] + list(_jac(qa, one))))
    add("iter: R = Q curve point, Z = 1", _rec([p, qc[0], qc[1]] + list(_jac(qc, one))))
    add("iter: R = -Q, Z = 1", _rec([p, qa[0], qa[1]] + list(_jac(_neg(qa), one))))
    add("iter: Z = 0", _rec([p, qa[0], qa[1], qa[0], qa[1], zero]))
    add("iter: P = (0, 0), R = Q", _rec([zero, qa[0], qa[1]] + list(_jac(qa, one))))
    add("iter: P = (0, 0), R random", _rec([zero] + [_rand2(g) for _ in range(5)]))
    add("iter: R = Q off the curve, Z = 1", _rec([_rand2(g), rq[0], rq[1], rq[0], rq[1], one]))
    # the addition step runs on 4 R: Q = 4 R and Q = -4 R meet it with theta = lambda = 0 / lambda = 0
    r4 = D._ec_mul(D._f2(), qc, 4)
    add("iter: Q = 4 R at the addition, Jacobian", _rec([p, r4[0], r4[1]] + list(_jac(qc, z))))
    add("iter: Q = 4 R at the addition, homogeneous", _rec([p, r4[0], r4[1]] + list(_hom(qc, z))))
    add("iter: Q = -4 R at the addition, Jacobian", _rec([p, r4[0], pm.f2neg(r4[1])] + list(_jac(qc, z))))
    add("iter: Q = -4 R at the addition, homogeneous", _rec([p, r4[0], pm.f2neg(r4[1])] + list(_hom(qc, z))))
    add("iter: order 13, homogeneous", _rec([p, q13[0], q13[1]] + list(_hom(q13, z))))
    y = g.randrange(Q)
    add("iter: equal lanes", [y, y] + [xs[i // 2] for i in range(2, 12)])
    add("iter: equal lanes, R = Q, Z = (1, 1)", [y, y, xs[1], xs[1], xs[2], xs[2], xs[1], xs[1], xs[2], xs[2],
                                                   RMONT, RMONT])
    assert len({label for label, _ in out}) == len(out)
    return tuple((label, tuple(rec)) for label, rec in out)


def structured():
    """[(label, record)]: fresh lists each call"""
    return [(label, list(rec)) for label, rec in _structured()]


def by_label(label):
    return next(list(rec) for lb, rec in _structured() if lb == label)


def iter_sim_labels():
    """the structured records the two iter programs take through the
    simulator: every "iter:" case (R = Q, Z = 0, a zero P and equal lanes
    among them) and some of the plain edges"""
    labels = [lb for lb, _ in _structured() if lb.startswith("iter:")]
    labels += ["f = 1", "c0 = c1 (equal lanes)", "c0 = -c1", "all coeff 3", "c0 = coeff 0", "c1 = coeff 7"]
    assert all(any(lb == x for x, _ in _structured()) for lb in labels)
    return labels


def random_records(seed, n):
    g = random.Random(seed)
    return [[g.randrange(Q) for _ in range(12)] for _ in range(n)]


def gpu_records(n=1000, nrand=32, seed=77):
    """n records for one launch: the structured records tiled (their count is
    no multiple of a wave's 32 pairs, so every tile puts a record on other
    lanes of another wave; the last wave is partly filled), seeded random ones
    in the middle"""
    s = [rec for _, rec in structured()]
    assert len(s) % 32 and n % 32
    tiled = [list(s[i % len(s)]) for i in range(n - nrand)]
    half = len(tiled) // 2
    return tiled[:half] + random_records(seed, nrand) + tiled[half:]
