"""The domain of the e(P, Q) entries as one deterministic list of cases, shared
by the CPU and GPU tests of tests/test_pairing_domain.py.

Engine::pairing (lib.rs:101-109) and miller_loop (mod.rs:40-102) state no
precondition on their points and check none: into_affine_unchecked
(ec.rs:686-740, 1333-1395) hands them whatever field elements an encoding
holds.  So the cases leave the prime-order subgroups and the curves:

  Q (G2 side)  on E': in the subgroup, a random curve point, an r-multiple
               (order divides h2), subgroup + torsion;
               of small odd order 13 and 23, alone and added to a subgroup
               point; order 13 is also the case where R = -Q inside the loop
               (see r_meets_q);
               off E': four random Fq values, a curve point with y + 1 and
               y - 1, x = 0, y = 0, small x and y on a twist with another b.
  P (G1 side)  the same four on-curve kinds, a point of order 3, random values
               off the curve, x = 0, y = 0.
  infinity     on either side, on both, and beside off-curve values.

`cases()` returns (label, p_record, q_record) triples in ABI form (13 / 25
u64 words, Montgomery coordinates, infinity word last); `KINDS[label]` names
what a test may need to know about a case.  Pure Python ints: independent of
the oracle and of the product.
"""
import functools
import math

import numpy as np

import decode_cases as D
from helpers import Q, RMONT, limbs
from ml_ref import BLS_X

F1, F2 = D._f1(), D._f2()
V = BLS_X >> 1


def r_meets_q(m):
    """the addition steps of the loop (the set bits of |x| >> 1 below its
    leading one) at which R = -Q or R = +Q for a Q of exact order m: before
    the addition at bit b, R = ((V >> b) - 1) Q.  Returns [(b, sign)]."""
    out = []
    for b in range(V.bit_length() - 2, -1, -1):
        if (V >> b) & 1:
            k = (V >> b) - 1
            if (k + 1) % m == 0:
                out.append((b, -1))
            elif (k - 1) % m == 0:
                out.append((b, +1))
    return out


def _order_is(F, P, m):
    """P has exact order m (m prime)"""
    return P is not None and D._ec_mul(F, P, m) is None


def _small_order_g2(m, seed):
    """a point of E'(Fq2) of exact prime order m | h2, from the r-multiple of
    a random curve point (decode_cases.subgroup_points' h // small
    construction); further seeds until one is not trivial"""
    assert D.H2 % m == 0
    for s in range(seed, seed + 32):
        g = np.random.default_rng(s)
        T = D._ec_mul(F2, D._random_point(2, g), D.R_ORDER)
        e = D.H2
        while e % m == 0:
            e //= m
        Ts = D._ec_mul(F2, T, e)            # order a power of m
        while Ts is not None and not _order_is(F2, Ts, m):
            Ts = D._ec_mul(F2, Ts, m)
        if Ts is not None:
            assert _order_is(F2, Ts, m)
            return Ts
    raise AssertionError("no point of order %d found" % m)


def _rand_fq(g):
    return int.from_bytes(g.bytes(64), "big") % Q


@functools.lru_cache(maxsize=None)
def points():
    """the named points: {'p': {kind: point}, 'q': {kind: point}}"""
    g1 = np.random.default_rng(9301)
    g2 = np.random.default_rng(9401)
    # ---- G1 ----
    R1 = D._random_point(1, g1)
    S1 = D._ec_mul(F1, R1, D.H1)
    T1 = D._ec_mul(F1, R1, D.R_ORDER)
    O3 = (0, 2)                                            # 2^2 = 0^3 + 4
    assert _order_is(F1, O3, 3) and D._ec_mul(F1, S1, D.R_ORDER) is None and T1 is not None
    P2 = D._ec_mul(F1, D._random_point(1, g1), D.H1)       # a second subgroup point
    p = {
        "subgroup": S1,
        "curve": R1,
        "r_multiple": T1,
        "subgroup+torsion": D._ec_add(F1, S1, T1),
        "order3": O3,
        "off_random": (_rand_fq(g1), _rand_fq(g1)),
        "x=0": (0, S1[1]),
        "y=0": (S1[0], 0),
        "subgroup2": P2,
    }
    for k in ("off_random", "x=0", "y=0"):
        assert D.rhs1(p[k][0]) != p[k][1] * p[k][1] % Q
    # ---- G2 ----
    R2 = D._random_point(2, g2)
    S2 = D._ec_mul(F2, R2, D.H2)
    T2 = D._ec_mul(F2, R2, D.R_ORDER)
    assert D._ec_mul(F2, S2, D.R_ORDER) is None and T2 is not None
    O13 = _small_order_g2(13, 9413)
    O23 = _small_order_g2(23, 9423)
    # order 13: R = 12 Q = -Q at the loop's second addition step (bit 59,
    # V >> 59 = 13), so R + Q is infinity there; no order dividing #E'(Fq2)
    # gives R = +Q (V >> b - 2 is 1, 11, 103, 53759, ... : coprime to h2 r)
    assert (59, -1) in r_meets_q(13) and not r_meets_q(23)
    order = D.H2 * D.R_ORDER
    assert all(math.gcd(order, (V >> b) - 2) == 1 for b in range(V.bit_length() - 1) if (V >> b) & 1)
    S2b = D._ec_mul(F2, D._random_point(2, g2), D.H2)
    one = (1, 0)
    q = {
        "subgroup": S2,
        "curve": R2,
        "r_multiple": T2,
        "subgroup+torsion": D._ec_add(F2, S2, T2),
        "order13": O13,
        "order23": O23,
        "subgroup+order13": D._ec_add(F2, S2, O13),
        "subgroup+order23": D._ec_add(F2, S2, O23),
        "off_random": ((_rand_fq(g2), _rand_fq(g2)), (_rand_fq(g2), _rand_fq(g2))),
        "off_random2": ((_rand_fq(g2), _rand_fq(g2)), (_rand_fq(g2), _rand_fq(g2))),
        "y+1": (S2[0], D.f2add(S2[1], one)),
        "y-1": (S2[0], D.f2add(S2[1], (Q - 1, 0))),
        "x=0": ((0, 0), S2[1]),
        "y=0": (S2[0], (0, 0)),
        "other_b": ((1, 2), (3, 4)),
        "subgroup2": S2b,
    }
    for k in OFF_CURVE_Q:
        assert D.rhs2(q[k][0]) != D.f2mul(q[k][1], q[k][1]), k
    for k in q:
        if k not in OFF_CURVE_Q:
            assert D.rhs2(q[k][0]) == D.f2mul(q[k][1], q[k][1]), k
    return {"p": p, "q": q}


OFF_CURVE_Q = ("off_random", "off_random2", "y+1", "y-1", "x=0", "y=0", "other_b")
OFF_CURVE_P = ("off_random", "x=0", "y=0")
# Q kinds of pure small order, at which the loop's R may pass through
# infinity or +-Q.  The reference's steps never use the curve constant, so
# (0, y) off E' is to them a point of order 3 on y^2 = x^3 + y_Q^2 (R = 2 Q
# = -Q at the first addition step) and (x, 0) one of order 2 (2 Q is
# infinity at the first doubling): both belong here as well as to OFF_CURVE_Q.
SMALL_ORDER_Q = ("order13", "order23", "x=0", "y=0")


def _inf(group, garbage=None):
    """G*Affine::zero() (ec.rs:158-164: x = 0, y = one, infinity set), or an
    infinity-flagged record that holds `garbage` coordinates: the flag decides"""
    if garbage is not None:
        rec = D.aff_record(group, garbage)
        rec[-1] = 1
        return rec
    w = 13 if group == 1 else 25
    fw = (w - 1) // 2
    rec = [0] * w
    rec[fw:fw + 6] = limbs(RMONT)
    rec[-1] = 1
    return rec


@functools.lru_cache(maxsize=None)
def _cases():
    pts = points()
    p, q = pts["p"], pts["q"]
    P = lambda k: D.aff_record(1, p[k])   # noqa: E731
    Qr = lambda k: D.aff_record(2, q[k])  # noqa: E731
    out = []
    # every Q kind against a subgroup P
    for k in q:
        out.append(("P subgroup x Q " + k, P("subgroup"), Qr(k)))
    # every P kind against a subgroup Q
    for k in p:
        if k != "subgroup":
            out.append(("P " + k + " x Q subgroup", P(k), Qr("subgroup")))
    # both sides outside: torsion x torsion, small orders, off curve x off curve
    out += [
        ("P r_multiple x Q r_multiple", P("r_multiple"), Qr("r_multiple")),
        ("P order3 x Q order13", P("order3"), Qr("order13")),
        ("P curve x Q off_random", P("curve"), Qr("off_random")),
        ("P off_random x Q off_random", P("off_random"), Qr("off_random")),
        ("P y=0 x Q y+1", P("y=0"), Qr("y+1")),
        ("P x=0 x Q x=0", P("x=0"), Qr("x=0")),
        ("P off_random x Q order13", P("off_random"), Qr("order13")),
        ("P subgroup2 x Q off_random2", P("subgroup2"), Qr("off_random2")),
    ]
    # infinity
    out += [
        ("P infinity x Q subgroup", _inf(1), Qr("subgroup")),
        ("P subgroup x Q infinity", P("subgroup"), _inf(2)),
        ("P infinity x Q infinity", _inf(1), _inf(2)),
        ("P infinity x Q off_random", _inf(1), Qr("off_random")),
        ("P off_random x Q infinity", P("off_random"), _inf(2)),
        ("P subgroup x Q infinity flag over off_random", P("subgroup"), _inf(2, q["off_random"])),
        ("P infinity flag over off_random x Q y+1", _inf(1, p["off_random"]), Qr("y+1")),
    ]
    assert len({c[0] for c in out}) == len(out)
    return tuple((label, np.array(pr, np.uint64), np.array(qr, np.uint64)) for label, pr, qr in out)


def cases():
    """[(label, p_record (13,), q_record (25,))]; fresh arrays each call"""
    return [(label, pr.copy(), qr.copy()) for label, pr, qr in _cases()]


def arrays():
    """(labels, p (n, 13), q (n, 25))"""
    cs = _cases()
    return [c[0] for c in cs], np.stack([c[1] for c in cs]), np.stack([c[2] for c in cs])


def _q_kind(label):
    return label.split(" x Q ")[1]


def q_off_curve(label):
    """the case's Q is not on E' and neither side is infinity: the pairs the
    pairing-only Miller loops cannot take"""
    k = _q_kind(label)
    return "infinity" not in label and k in OFF_CURVE_Q


def q_degenerate(label):
    """the case's Q has pure small order -- the small-order and R = +-Q cases,
    the only ones whose reference Miller value may be 0"""
    return "infinity" not in label and _q_kind(label) in SMALL_ORDER_Q


def has_infinity(label):
    return "infinity" in label


def as_points(p_rec, q_rec):
    """the ABI records back as canonical points (None for infinity), for ml_ref"""
    from helpers import unmont
    pt = None if int(p_rec[12]) & 0xff else (unmont(p_rec[0:6]), unmont(p_rec[6:12]))
    qt = None if int(q_rec[24]) & 0xff else ((unmont(q_rec[0:6]), unmont(q_rec[6:12])),
                                             (unmont(q_rec[12:18]), unmont(q_rec[18:24])))
    return pt, qt
