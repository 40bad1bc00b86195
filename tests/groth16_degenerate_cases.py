"""Degenerate inputs of the Groth16 prover (tests/test_groth16_degenerate.py).

Part A: keys inside G1/G2 as groth16_ref.Key (every point a known multiple of
its generator), with zeros -- points at infinity -- in the queries and in
alpha, beta, delta, and with one number solved mod r so that one operation of
the assembly kernel meets an exceptional branch of the group law.  `quantities`
names every intermediate point of the kernel by its discrete logarithm; each
case carries the equality it was built for, asserted on those integers.

Part B: keys whose alpha, beta and query points are multiples of a base of
small order (small_order_cases), delta a subgroup point.  The reference proof
there is the header's four formulas on decode_cases' affine integer arithmetic,
scalars acting as integers in [0, r): independent of the oracle and of the
product.  `census` replays the kernel's two double-and-add chains and its C
additions in integers mod m and counts the exceptional branches they meet.

Nothing here touches the device."""
import functools
import types

import numpy as np

import decode_cases as D
import groth16_ref as G
import small_order_cases as C
from helpers import R_ORDER, rng

R = R_ORDER
NV, NPUB, NROWS, LOGN = 8, 2, 6, 3
N = 1 << LOGN
inv = lambda v: pow(v % R, -1, R)   # noqa: E731


# ---------------- the tiny system ----------------

@functools.lru_cache(maxsize=None)
def tiny():
    """(mats, w, other): n_vars = 8, n_public = 2, n_rows = 6; w satisfies it and has no zero entry,
    other does not satisfy it"""
    mats, w = G.satisfied_system(6000, NROWS, NV)
    other = [1] + [x or 1 for x in G.rand_fr(rng(6001), NV - 1)]
    assert all(w) and all(other)
    return mats, w, other


_QUOTIENTS = {}


def quotient(oracle, mats, w, log_n, tag):
    """the n quotient integers of one witness, cached under (tag, w)"""
    key = (tag, tuple(w))
    if key not in _QUOTIENTS:
        _QUOTIENTS[key] = G.quotient_ints(oracle, mats, [list(w)], log_n)[0]
    return _QUOTIENTS[key]


def dot(x, y):
    return sum(p * q for p, q in zip(x, y)) % R


def quantities(key, w, h, r, s):
    """every point the assembly kernel forms, as its discrete logarithm, in the kernel's order"""
    q = types.SimpleNamespace()
    q.S_a, q.S_b = dot(w, key.a), dot(w, key.b)
    q.S_l, q.S_h = dot(w[key.n_public:], key.l), dot(h[:len(key.h)], key.h)
    q.A0, q.B0 = (key.alpha + q.S_a) % R, (key.beta + q.S_b) % R
    q.rd, q.sd, q.rsd = r * key.delta % R, s * key.delta % R, r * s % R * key.delta % R
    q.sA0, q.rB0 = s * q.A0 % R, r * q.B0 % R
    q.A = (q.A0 + q.rd) % R
    q.sd_Sb = (q.sd + q.S_b) % R
    q.B = (q.sd_Sb + key.beta) % R
    q.T1 = (q.S_l + q.S_h) % R
    q.T2 = (q.T1 + q.sA0) % R
    q.T3 = (q.T2 + q.rB0) % R
    q.C = (q.T3 + q.rsd) % R
    assert (q.A, q.B, q.C) == G.proof_scalars(key, w, h, r, s)
    return q


def neg(v):
    return (R - v) % R


def clone(key, **kw):
    f = dict(alpha=key.alpha, beta=key.beta, delta=key.delta, a=list(key.a), b=list(key.b), l=list(key.l),
             h=list(key.h), n_public=key.n_public, log_n=key.log_n)
    f.update(kw)
    return G.Key(**f)


def zeros(key):
    """how many points of each query are the point at infinity"""
    return {name: sum(v == 0 for v in getattr(key, name)) for name in "ablh"}


# ---------------- Part A 1: sparse keys ----------------

def _zero_at(vals, idx):
    return [0 if i in idx else v for i, v in enumerate(vals)]


@functools.lru_cache(maxsize=None)
def generic_key():
    return G.random_key(6010, NV, NPUB, LOGN, N)


@functools.lru_cache(maxsize=None)
def sparse_cases():
    """{name: (key, mats, n_rows, [witnesses], expected zero counts)}"""
    mats, w, other = tiny()
    k = generic_key()
    ws = [w, other, w]
    out = {
        "scattered": (clone(k, a=_zero_at(k.a, {0, 3, 7}), b=_zero_at(k.b, {0, 5, 7}), l=_zero_at(k.l, {0, 2, 5}),
                            h=_zero_at(k.h, {0, 4, 7})), mats, NROWS, ws, dict(a=3, b=3, l=3, h=3)),
        "a_zero": (clone(k, a=[0] * NV), mats, NROWS, ws, dict(a=NV)),
        "b_zero": (clone(k, b=[0] * NV), mats, NROWS, ws, dict(b=NV)),
        "l_zero": (clone(k, l=[0] * (NV - NPUB)), mats, NROWS, ws, dict(l=NV - NPUB)),
        "h_zero": (clone(k, h=[0] * N), mats, NROWS, ws, dict(h=N)),
        "h_len_0": (clone(k, h=[]), mats, NROWS, ws, dict(h=0)),
        "no_private_variable": (clone(k, l=[], n_public=NV), mats, NROWS, ws, dict(l=0)),
    }
    # log_n = 0: a domain of one point, one row or none
    one_row, w1 = G.satisfied_system(6020, 1, NV)
    g = rng(6021)
    other1 = [1] + G.rand_fr(g, NV - 1)
    k0 = G.random_key(6022, NV, NPUB, 0, 1)
    sparse0 = clone(k0, a=_zero_at(k0.a, {0, 7}), b=_zero_at(k0.b, {1, 7}), l=_zero_at(k0.l, {0, 5}))
    out["log_n_0_one_row"] = (sparse0, one_row, 1, [w1, other1, w1], dict(a=2, b=2, l=2, h=0))
    out["log_n_0_h_zero"] = (clone(sparse0, h=[0]), one_row, 1, [w1, other1, w1], dict(h=1))
    out["log_n_0_no_row"] = (clone(sparse0, h=[]), ([], [], []), 0, [w1, other1, w1], dict(h=0))
    return out


@functools.lru_cache(maxsize=None)
def large_case():
    """n_vars = 300, log_n = 9, 400 rows, about two thirds of every query at infinity, the first and the last
    entry of each among them: (key, mats, n_rows, [w, other])"""
    n_vars, n_rows, log_n = 300, 400, 9
    mats, w = G.satisfied_system(6030, n_rows, n_vars)
    k = G.random_key(6031, n_vars, 5, log_n, (1 << log_n) - 1)
    g = rng(6032)

    def thin(vals):
        keep = g.random(len(vals)) < 1 / 3
        keep[0] = keep[-1] = False
        return [v if t else 0 for v, t in zip(vals, keep)]
    key = clone(k, a=thin(k.a), b=thin(k.b), l=thin(k.l), h=thin(k.h))
    other = [1] + G.rand_fr(g, n_vars - 1)
    return key, mats, n_rows, [w, other]


# ---------------- Part A 2: alpha, beta, delta at infinity ----------------

@functools.lru_cache(maxsize=None)
def abd_cases():
    k = generic_key()
    return {"alpha": clone(k, alpha=0), "beta": clone(k, beta=0), "delta": clone(k, delta=0),
            "alpha_beta_delta": clone(k, alpha=0, beta=0, delta=0)}


# ---------------- Part A 3: one collision per operation of the assembly ----------------

COLLISION_R, COLLISION_S = G.rand_fr(rng(6040), 2)

# (id, what is solved, the equality the case is for, on quantities(); further facts that must hold with it)
_SOLVE = [
    # the mixed addition of alpha onto S_a (wave 2, lane 0)
    ("alpha:S_a=0", "a", lambda q, k: q.S_a == 0 and k.alpha != 0 and q.A0 == k.alpha),
    ("alpha:S_a=alpha", "alpha", lambda q, k: q.S_a == k.alpha != 0),
    ("alpha:S_a=-alpha", "alpha", lambda q, k: q.S_a == neg(k.alpha) != 0 and q.A0 == 0 and q.sA0 == 0 and q.A == q.rd),
    # of beta onto S_b, in G1 (wave 2, lane 1) and in G2 (wave 0, lane 0) at once
    ("beta:S_b=0", "b", lambda q, k: q.S_b == 0 and k.beta != 0 and q.B0 == k.beta),
    ("beta:S_b=beta", "beta", lambda q, k: q.S_b == k.beta != 0),
    ("beta:S_b=-beta", "beta", lambda q, k: q.S_b == neg(k.beta) != 0 and q.B0 == 0 and q.rB0 == 0 and q.B == q.sd),
    # A = A0 + r delta
    ("A:r.delta=A0", "r", lambda q, k: q.rd == q.A0 != 0),
    ("A:r.delta=-A0", "r", lambda q, k: q.rd == neg(q.A0) != 0 and q.A == 0),
    # B = s delta + S_b + beta
    ("B:s.delta=S_b", "s", lambda q, k: q.sd == q.S_b != 0),
    ("B:s.delta=-S_b", "s", lambda q, k: q.sd == neg(q.S_b) != 0 and q.sd_Sb == 0 and q.B == k.beta),
    ("B:s.delta+S_b=beta", "s", lambda q, k: q.sd_Sb == k.beta != 0),
    ("B:s.delta+S_b=-beta", "s", lambda q, k: q.sd_Sb == neg(k.beta) != 0 and q.B == 0),
    # C = S_l + S_h + s A0 + r B0 + (r s) delta
    ("C:S_l=S_h", "l", lambda q, k: q.S_l == q.S_h != 0),
    ("C:S_l=-S_h", "l", lambda q, k: q.S_l == neg(q.S_h) != 0 and q.T1 == 0),
    ("C:S_l+S_h=s.A0", "l", lambda q, k: q.T1 == q.sA0 != 0),
    ("C:S_l+S_h=-s.A0", "l", lambda q, k: q.T1 == neg(q.sA0) != 0 and q.T2 == 0),
    ("C:S_l+S_h+s.A0=r.B0", "l", lambda q, k: q.T2 == q.rB0 != 0),
    ("C:S_l+S_h+s.A0=-r.B0", "l", lambda q, k: q.T2 == neg(q.rB0) != 0 and q.T3 == 0),
    ("C:S_l+S_h+s.A0+r.B0=rs.delta", "l", lambda q, k: q.T3 == q.rsd != 0),
    ("C:S_l+S_h+s.A0+r.B0=-rs.delta", "l", lambda q, k: q.T3 == neg(q.rsd) != 0 and q.C == 0),
]
COLLISION_IDS = [c[0] for c in _SOLVE]
SHARED_IDS = [c[0] for c in _SOLVE if c[1] in "rs"]       # the generic key, one batched call
INFINITY_IDS = {"A:r.delta=-A0": "A", "B:s.delta+S_b=-beta": "B", "C:S_l+S_h+s.A0+r.B0=-rs.delta": "C"}


def free_number(cid):
    """which number the case solves for: r, s, alpha, beta, or the query (a, b, l) with one changed entry"""
    return _SOLVE[COLLISION_IDS.index(cid)][1]


def collision(oracle, cid):
    """(key, w, r, s, q): the case `cid`, one free number solved mod r, and its quantities with the equality
    asserted.  The free number is r or s over generic_key(), or one entry of the key (alpha, beta, the a or b
    entry of variable 3, the l entry of variable 4)."""
    _, free, holds = _SOLVE[COLLISION_IDS.index(cid)]
    mats, w, _ = tiny()
    h = quotient(oracle, mats, w, LOGN, "tiny")
    k = generic_key()
    r, s = COLLISION_R, COLLISION_S
    q = quantities(k, w, h, r, s)
    assert all(v != 0 for v in vars(q).values())        # the generic key meets none of the equalities
    dinv = inv(k.delta)
    if free == "a":
        k = clone(k, a=[v if i != 3 else (v - q.S_a * inv(w[3])) % R for i, v in enumerate(k.a)])
    elif free == "b":
        k = clone(k, b=[v if i != 3 else (v - q.S_b * inv(w[3])) % R for i, v in enumerate(k.b)])
    elif free == "alpha":
        k = clone(k, alpha=q.S_a if cid.endswith("=alpha") else neg(q.S_a))
    elif free == "beta":
        k = clone(k, beta=q.S_b if cid.endswith("=beta") else neg(q.S_b))
    elif free == "r":
        r = (q.A0 if cid.endswith("=A0") else neg(q.A0)) * dinv % R
    elif free == "s":
        target = {"B:s.delta=S_b": q.S_b, "B:s.delta=-S_b": neg(q.S_b), "B:s.delta+S_b=beta": k.beta - q.S_b,
                  "B:s.delta+S_b=-beta": -k.beta - q.S_b}[cid]
        s = target * dinv % R
    else:
        sign = neg if "=-" in cid else (lambda v: v)
        lhs, rhs = cid[2:].replace("=-", "=").split("=")
        partial = {"S_l": 0, "S_l+S_h": q.S_h, "S_l+S_h+s.A0": q.S_h + q.sA0, "S_l+S_h+s.A0+r.B0": q.S_h + q.sA0 + q.rB0}
        other = {"S_h": q.S_h, "s.A0": q.sA0, "r.B0": q.rB0, "rs.delta": q.rsd}[rhs]
        target = (sign(other) - partial[lhs]) % R       # the S_l that makes the equality hold
        var = 4
        k = clone(k, l=[v if i != var - NPUB else (v + (target - q.S_l) * inv(w[var])) % R for i, v in enumerate(k.l)])
    q = quantities(k, w, h, r, s)
    assert holds(q, k), cid
    return k, w, r, s, q


# ---------------- Part A 4: blinding scalars at the lane boundaries of the table sums ----------------

BOUNDARY_BITS = (0, 3, 4, 7, 8, 31, 32, 127, 128, 251, 252, 253, 254)


@functools.lru_cache(maxsize=None)
def boundary_scalars():
    """[(r, s)]: a single bit of r, of s, of both and of r s at every boundary; the top lane's patterns"""
    g = rng(6050)
    x, y = G.rand_fr(g, 2)
    out = []
    for i in BOUNDARY_BITS:
        b = 1 << i
        out += [(b, x), (y, b), (b, b), (x, b * inv(x) % R)]      # the last: r s = 2^i, the (r s) delta half
    top = [R - 1, (1 << 254) + (1 << 253), (1 << 254) + (1 << 253) + (1 << 252), 0x73ed << 240, 0x73eda753 << 224,
           (1 << 252) - 1, (1 << 254) - 1, R - (1 << 32)]
    assert all(0 < t < R for t in top) and all(b < R for b in (1 << i for i in BOUNDARY_BITS))
    out += [(t, t) for t in top] + [(t, x) for t in top[:4]] + [(y, t) for t in top[:4]]
    out += [(x, t * inv(x) % R) for t in top[:4]]                  # r s fills the top lane
    out += [(1, 1), (x, inv(x)), (R - 1, R - 1), (R - 1, 1), (0, x), (y, 0), (0, 0)]
    assert all(0 <= r < R and 0 <= s < R for r, s in out)
    return out


# ---------------- Part A 5: a realistic key ----------------

ONLY_A, ONLY_B, ONLY_C, NOWHERE = 3, 4, 5, 7


@functools.lru_cache(maxsize=None)
def occurrence_system():
    """(mats, w): 6 rows over 8 variables; variable 3 occurs only in A, 4 only in B, 5 only in C, 7 nowhere;
    w satisfies it"""
    g = rng(6060)
    w = [1] + [x or 1 for x in G.rand_fr(g, NV - 1)]
    a_cols = [(0, 3), (1, 6), (3, 2), (6,), (3, 1, 0), (2,)]
    b_cols = [(4, 1), (0,), (6, 4), (2, 4), (1,), (4, 6, 0)]
    c_col = [5, 6, 0, 1, 5, 2]
    coeff = lambda cols: [(c, v or 1) for c, v in zip(cols, G.rand_fr(g, len(cols)))]   # noqa: E731
    a, b = [coeff(c) for c in a_cols], [coeff(c) for c in b_cols]
    c = []
    for ra, rb, col in zip(a, b, c_col):
        va, vb = (sum(v * w[j] for j, v in row) % R for row in (ra, rb))
        assert va and vb
        c.append([(col, va * vb * inv(w[col]) % R)])
    mats = (a, b, c)
    used = [{j for row in m for j, _ in row} for m in mats]
    assert ONLY_A in used[0] and ONLY_A not in used[1] | used[2]
    assert ONLY_B in used[1] and ONLY_B not in used[0] | used[2]
    assert ONLY_C in used[2] and ONLY_C not in used[0] | used[1]
    assert NOWHERE not in used[0] | used[1] | used[2]
    return mats, w


# ---------------- Part B: keys on bases of small order ----------------

G1_GEN, G2_GEN = (D.G1_X, D.G1_Y), (D.G2_X, D.G2_Y)
# (G1 base, G2 base): one key per small-order base, and one on the mixed bases
TORSION_KEYS = [("O3", "O13"), ("O11", "O23"), ("O33", "O13"), ("S+O3", "S+O13")]
TORSION_OF = {"S+O3": "O3", "S+O13": "O13"}
_MUL = {}


def ec_add(group, P, Q):
    return D._ec_add(C.field(group), P, Q)


def ec_mul(group, P, k):
    """k P for an integer k >= 0, by double-and-add on the affine integers"""
    if P is None or k == 0:
        return None
    key = (group, P, k)
    if key not in _MUL:
        _MUL[key] = D._ec_mul(C.field(group), P, k)
    return _MUL[key]


def combo(group, pts, scalars):
    """sum_i scalars[i] pts[i], the scalars acting as plain integers: equal points share one multiplication
    by the integer sum of their scalars (nothing is reduced by a group order)"""
    tot = {}
    for P, k in zip(pts, scalars):
        if P is not None and k:
            tot[P] = tot.get(P, 0) + k
    acc = None
    for P, k in tot.items():
        acc = ec_add(group, acc, ec_mul(group, P, k))
    return acc


def order(name):
    return C.ORDERS[TORSION_OF.get(name, name)]


class PointKey:
    """a proving key as affine integer points: alpha, beta and the queries the multiples `mult` of one base
    per group, delta = d G, d H"""

    def __init__(self, P1, P2, mult, d, n_public, log_n, names=(None, None)):
        self.mult, self.d, self.n_public, self.log_n = mult, d, n_public, log_n
        self.g1, self.g2 = names
        pts = lambda grp, P, ks: [ec_mul(grp, P, k) for k in ks]   # noqa: E731
        self.alpha, self.beta1 = ec_mul(1, P1, mult["alpha"]), ec_mul(1, P1, mult["beta1"])
        self.beta2 = ec_mul(2, P2, mult["beta2"])
        self.delta1, self.delta2 = ec_mul(1, G1_GEN, d), ec_mul(2, G2_GEN, d)
        self.a, self.b1, self.l, self.h = (pts(1, P1, mult[n]) for n in ("a", "b1", "l", "h"))
        self.b2 = pts(2, P2, mult["b2"])
        self.n_vars = len(self.a)

    def points(self):
        """the arguments of pairing_amd.groth16_pk, in its order"""
        one = lambda grp, P: C.aff(grp, P)[None]   # noqa: E731
        return (one(1, self.alpha), one(1, self.beta1), one(1, self.delta1), one(2, self.beta2), one(2, self.delta2),
                C.aff_rows(1, self.a), C.aff_rows(1, self.b1), C.aff_rows(2, self.b2), C.aff_rows(1, self.l),
                C.aff_rows(1, self.h), self.n_public, self.log_n)


def int_proof(key, w, h, r, s):
    """(A, B, C) of include/pairing_amd.h's four formulas, as affine integer points (None: infinity)"""
    z = key.n_public
    A = ec_add(1, ec_add(1, key.alpha, combo(1, key.a, w)), ec_mul(1, key.delta1, r))
    B = ec_add(2, ec_add(2, key.beta2, combo(2, key.b2, w)), ec_mul(2, key.delta2, s))
    B1 = ec_add(1, ec_add(1, key.beta1, combo(1, key.b1, w)), ec_mul(1, key.delta1, s))
    Cp = ec_add(1, combo(1, key.l, w[z:]), combo(1, key.h, h[:len(key.h)]))
    Cp = ec_add(1, Cp, ec_mul(1, A, s))
    Cp = ec_add(1, Cp, ec_mul(1, B1, r))
    Cp = ec_add(1, Cp, C.ec_neg(1, ec_mul(1, key.delta1, r * s % R)))
    return A, B, Cp


def proof_row(proof):
    A, B, Cp = proof
    return np.concatenate([C.aff(1, A), C.aff(2, B), C.aff(1, Cp)])


# seeds chosen on the CPU so that the census (test_branch_census_of_the_small_order_keys) holds for every base
TORSION_SEED = {"O3": 7000, "O11": 7000, "O33": 7035, "S+O3": 7090}


def _picks(m):
    return sorted({0, 1, 2, m // 2, m - 1})


@functools.lru_cache(maxsize=None)
def torsion_key(g1, g2):
    """(PointKey, r, s): every multiplier from a few residues mod the base's order, zero among them in every
    query (the first entry of a and b, the last of l and h); alpha and beta not zero"""
    g = rng(TORSION_SEED[g1])
    p1, p2 = _picks(order(g1)), _picks(order(g2))[:4]
    draw = lambda picks, n: [picks[int(i)] for i in g.integers(0, len(picks), size=n)]   # noqa: E731
    nz = lambda picks: picks[1 + int(g.integers(0, len(picks) - 1))]                     # noqa: E731
    mult = dict(alpha=nz(p1), beta1=nz(p1), beta2=nz(p2), a=[0] + draw(p1, NV - 1), b1=[0] + draw(p1, NV - 1),
                b2=[0] + draw(p2, NV - 1), l=draw(p1, NV - NPUB - 1) + [0], h=draw(p1, N - 1) + [0])
    d, r, s = (x or 1 for x in G.rand_fr(g, 3))
    return PointKey(C.point(1, g1), C.point(2, g2), mult, d, NPUB, LOGN, names=(g1, g2)), r, s


def torsion_witnesses(g1, g2):
    """the witnesses proved over torsion_key(g1, g2): the satisfying one, two that do not satisfy, and on a
    pure small-order G2 base one more for which beta_g2 + S_b2 is the point at infinity"""
    mats, w, other = tiny()
    key, _, _ = torsion_key(g1, g2)
    ws = [list(w), list(other), [1] + [x or 1 for x in G.rand_fr(rng(TORSION_SEED[g1] + 1), NV - 1)]]
    if g2 not in TORSION_OF:
        m, mult = order(g2), key.mult
        wb = list(other)
        var = next(i for i in range(NPUB, NV) if mult["b2"][i] % m)
        tot = (mult["beta2"] + sum(x * k for x, k in zip(wb, mult["b2"]))) % m
        wb[var] += (-tot * pow(mult["b2"][var], -1, m)) % m
        assert wb[var] < R and (mult["beta2"] + sum(x * k for x, k in zip(wb, mult["b2"]))) % m == 0
        ws.append(wb)
    return ws


def blindings(r, s):
    return [(0, 0), (0, s), (r, 0), (r, s)]


# ---- the branch census, in integers mod m ----
def chain_census(base, scalar, m, cnt):
    """jac_mul_repr's 256 steps, most significant bit first, on the multiple `base` of a point of odd order m"""
    acc = 0
    started = False
    for bit in range(255, -1, -1):
        acc = 2 * acc % m
        if (scalar >> bit) & 1:
            _add_census(acc, base, m, cnt, started)
            acc, started = (acc + base) % m, True
    return acc


def _add_census(acc, v, m, cnt, count_zero_plus=True):
    if v == 0:
        cnt["P+0"] += 1
    elif acc == 0:
        cnt["0+P"] += count_zero_plus
    elif acc == v:
        cnt["P+P"] += 1
    elif (acc + v) % m == 0:
        cnt["P+(-P)"] += 1
        cnt["infinity"] += 1
    if v == 0 and acc == 0:
        cnt["infinity"] += 1


def new_count():
    return {"0+P": 0, "P+0": 0, "P+P": 0, "P+(-P)": 0, "infinity": 0}


def census(key, ws, hs, rss):
    """(chains, c_adds): what s A0, r B0 (a first 0 + P of a chain is not counted) and the C additions that
    stay in <T> meet over all witnesses and blinding pairs, for a key on a pure small-order G1 base"""
    m, mult = order(key.g1), key.mult
    assert key.g1 not in TORSION_OF
    chains, c_adds = new_count(), new_count()
    red = lambda ks, xs: sum(k * x for k, x in zip(ks, xs)) % m   # noqa: E731
    seen = set()
    for w, h in zip(ws, hs):
        A0, B0 = (mult["alpha"] + red(mult["a"], w)) % m, (mult["beta1"] + red(mult["b1"], w)) % m
        S_l, S_h = red(mult["l"], w[key.n_public:]), red(mult["h"], h)
        for r, s in rss:
            for base, e in ((A0, s), (B0, r)):
                if (base, e) not in seen:           # the same chain twice reaches nothing new
                    seen.add((base, e))
                    chain_census(base, e, m, chains)
            sA0, rB0 = s * A0 % m, r * B0 % m
            acc = S_l
            for v in (S_h, sA0, rB0):
                _add_census(acc, v, m, c_adds)
                acc = (acc + v) % m
            if r * s % R == 0:                      # (r s) delta = 0: the last addition stays in <T> too
                _add_census(acc, 0, m, c_adds)
            elif acc == 0:
                c_adds["0+P"] += 1
    return chains, c_adds
