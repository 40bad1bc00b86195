"""Bases of small order for the group-law tests (tests/test_small_order.py).

E(Fq) has points of order 3, 11 and 33 (h1 = 3 * 11^2 * ...), E'(Fq2) points
of order 13 and 23 (h2 = 13^2 * 23^2 * ...).  On such a base every partial
sum of a scalar multiplication lives in a group of m elements, so the
exceptional branches of the group law (P + P, P + (-P), 0 + P, a table row
d * B = 0) are met at about every m-th step instead of never.

Everything here is decode_cases' affine arithmetic on Python ints, computed
once and cached: independent of the oracle and of the product.  Records are
in ABI form (Montgomery words); `comb_digits` and `branch_witness` restate the
signed base-256 recoding of the fixed-base comb in integers mod m.
"""
import functools

import numpy as np

import decode_cases as D
from helpers import Q, R_ORDER, limbs, mont, random_scalars, rng

F1, F2 = D._f1(), D._f2()
COMB_WINDOWS = 33
G1_ORDERS = {"O3": 3, "O11": 11, "O33": 33}
G2_ORDERS = {"O13": 13, "O23": 23}
ORDERS = dict(G1_ORDERS, **G2_ORDERS)


def field(group):
    return F1 if group == 1 else F2


def ec_neg(group, P):
    if P is None:
        return None
    if group == 1:
        return (P[0], (Q - P[1]) % Q)
    return (P[0], ((Q - P[1][0]) % Q, (Q - P[1][1]) % Q))


def _small_order_g1(m, seed):
    """a point of E(Fq) of exact prime order m | h1: the m-primary part of the
    r-multiple of a random curve point; further seeds until it is not trivial"""
    assert D.H1 % m == 0
    for s in range(seed, seed + 32):
        T = D._ec_mul(F1, D._random_point(1, np.random.default_rng(s)), D.R_ORDER)
        e = D.H1
        while e % m == 0:
            e //= m
        Ts = D._ec_mul(F1, T, e)
        while Ts is not None and D._ec_mul(F1, Ts, m) is not None:
            Ts = D._ec_mul(F1, Ts, m)
        if Ts is not None:
            return Ts
    raise AssertionError("no point of order %d found" % m)


@functools.lru_cache(maxsize=None)
def points():
    """{1: {name: point}, 2: {name: point}}: the small-order bases, subgroup
    points S (S2 in G2, and a second one S') and their sums with torsion"""
    import pairing_domain_cases as PD
    g = np.random.default_rng(9501)
    O3 = (0, 2)
    O11 = _small_order_g1(11, 9511)
    S = D._ec_mul(F1, D._random_point(1, g), D.H1)
    Sp = D._ec_mul(F1, D._random_point(1, g), D.H1)
    q = PD.points()["q"]
    return {
        1: {"O3": O3, "O11": O11, "O33": D._ec_add(F1, O3, O11), "S": S, "S'": Sp, "S+O3": D._ec_add(F1, S, O3)},
        2: {"O13": q["order13"], "O23": q["order23"], "S": q["subgroup"], "S+O13": q["subgroup+order13"]},
    }


def point(group, name):
    return points()[group][name]


# ---- records ----
def aff(group, P):
    """(13,) / (25,) uint64: the affine ABI record of P (None: infinity as G*Affine::zero())"""
    if P is None:
        w = 13 if group == 1 else 25
        rec = [0] * w
        rec[(w - 1) // 2:(w - 1) // 2 + 6] = limbs(pow(2, 384, Q))
        rec[-1] = 1
        return np.array(rec, np.uint64)
    return np.array(D.aff_record(group, P), np.uint64)


def aff_rows(group, pts):
    return np.ascontiguousarray(np.stack([aff(group, P) for P in pts]))


def jac(group, P, z):
    """(18,) / (36,) uint64: the Jacobian record (x z^2, y z^3, z) of P for a
    nonzero z (an int in G1, a pair in G2); None gives (1, 1, 0) scaled alike"""
    F = field(group)
    zz = F["mul"](z, z)
    zzz = F["mul"](zz, z)
    if P is None:
        x, y, z = zz, zzz, F["zero"]
    else:
        x, y = F["mul"](P[0], zz), F["mul"](P[1], zzz)
    if group == 1:
        return np.array(mont(x) + mont(y) + mont(z), np.uint64)
    return np.array(sum((mont(c) for c in (*x, *y, *z)), []), np.uint64)


def z_of(group, k):
    """the k-th of a fixed run of nonzero, non-one z values"""
    a = (0x5eed0000 + 7919 * k) * 0x1000000000000001f % Q
    return a if group == 1 else (a, (a * 31 + k + 1) % Q)


def jac_rows(group, pts, z0=0):
    return np.ascontiguousarray(np.stack([jac(group, P, z_of(group, z0 + k)) for k, P in enumerate(pts)]))


@functools.lru_cache(maxsize=None)
def multiples(group, name):
    """(0 T, 1 T, ..., (m - 1) T) of the small-order base `name`"""
    T, m = point(group, name), ORDERS[name]
    out = [None]
    for _ in range(m - 1):
        out.append(D._ec_add(field(group), out[-1], T))
    assert D._ec_add(field(group), out[-1], T) is None
    return tuple(out)


# ---- the comb's recoding, in integers ----
def wraps(s, window):
    """the reference's wnaf_form wrap (wnaf.rs:24-35): an odd s whose bits window..255 are all ones"""
    return bool(window) and 0 < window < 64 and s & 1 == 1 and (s >> window) == (1 << (256 - window)) - 1


def wnaf_value(s, window):
    """the integer the reference's wNAF digits of window `window` spell for a 256-bit repr s"""
    return s - (1 << 256) if wraps(s, window) else s


def comb_digits(s):
    """the signed base-256 digits of a 256-bit s, 33 windows: d > 128 becomes d - 256 with a carry"""
    out, carry = [], 0
    for win in range(COMB_WINDOWS):
        d = carry + ((s >> (8 * win)) & 0xff if win < 32 else 0)
        carry = 1 if d > 128 else 0
        out.append(d - 256 if d > 128 else d)
    assert carry == 0 and sum(d << (8 * i) for i, d in enumerate(out)) == s
    return out


def branch_witness(s, m, window=0):
    """what the comb multiply meets on a base of exact order m (odd), in
    integers mod m: the windows whose table row |d| B_win is zero (m | d), whose
    addition finds the accumulator equal to the row (a doubling), equal to its
    negative (a cancellation to zero), and whose addition starts from a zero
    accumulator after the first.  `window`: apply the wNAF wrap of that window
    first, as the entries do."""
    sign = 1
    if wraps(s, window):
        s, sign = (1 << 256) - s, -1
    acc, started = 0, False
    w = {"zero_row": 0, "doubling": 0, "cancellation": 0, "restart": 0}
    for win, d in enumerate(comb_digits(s)):
        if d == 0:
            continue
        if d % m == 0:
            w["zero_row"] += 1
            continue
        v = sign * d * pow(256, win, m) % m
        if acc == 0:
            w["restart"] += started
        elif acc == v:
            w["doubling"] += 1
        elif (acc + v) % m == 0:
            w["cancellation"] += 1
        acc, started = (acc + v) % m, True
    assert acc == sign * s % m
    return w


# ---- scalars ----
# chosen on the CPU so that test_scalar_list_reaches_every_branch's counts hold for every order
SCALAR_SEED = {3: 9703, 11: 9611, 33: 9633, 13: 9613, 23: 9623}


@functools.lru_cache(maxsize=None)
def scalar_ints(m):
    """64 256-bit reprs for a base of order m: the small multiples, m in single
    windows and in all of them, the 128 / 129 digit edges, the wNAF wrap's edges
    for windows 4 and 16 and random rows"""
    from test_bench_sizes import _wrap_scalars
    top = 1 << 256
    vals = [0, 1, m - 1, m, m + 1]
    vals += [m << (8 * i) for i in (1, 8, 31)]
    vals += [sum(m << (8 * i) for i in range(32))]
    vals += [128, 129, 128 + 256 * 128, 0x81 << 128, 128 << 248, 129 << 248]
    g = rng(SCALAR_SEED[m])
    # the wrap set of window 4 (r - 1, 2^256 - 1, 0 and 1 among its eleven) and what window 16 adds to it
    for w, pick in ((4, range(11)), (16, (2, 3, 4, 5, 7))):
        rows = _wrap_scalars(w, g)
        vals += [sum(int(x) << (64 * k) for k, x in enumerate(rows[i])) for i in pick]
    assert R_ORDER - 1 in vals and top - 1 in vals and top - (1 << 16) + 1 in vals
    rest = random_scalars(g, 64 - len(vals), bits=256)
    vals += [sum(int(x) << (64 * k) for k, x in enumerate(r)) for r in rest]
    assert len(vals) == 64
    return tuple(vals)


def scalars(m):
    """scalar_ints(m) as (64, 4) FrRepr rows"""
    return np.array([limbs(v, 4) for v in scalar_ints(m)], np.uint64)
