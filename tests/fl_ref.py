"""Big-integer references and operand generators for the tests of the lazy
field layer (tests/test_fl_unit.py, tests/test_fl_ref.py).  Pure Python.

A lazy value of bound U (fl.h) is 14 limbs, each <= U (2^28 - 1), of value
< U 2q (<= where a neg of zero produced it); it stands for value / R' mod q,
R' = 2^392.  Everything here computes on those plain residues: the tower with
tests/pymodel.py, the group law and the line steps restated from the
reference formulas (ec.rs dbl-2009-l / add-2007-bl / madd-2007-bl, mod.rs
doubling_step / addition_step / ell)."""
import os
import re

import pymodel as pm
from helpers import Q

LB, NL = 28, 14
M = (1 << LB) - 1
RP = 1 << (LB * NL)
RINV = pow(RP, -1, Q)
TOP = LB * (NL - 1)
BLS_X = 0xd201000000010000

_ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def sub_tables():
    """(FL_SUB_C, FL_SUB_CU) of the committed fl_gen.h: sub's / neg's constant per
    subtrahend bound B (row B - 1) and that constant's own bound"""
    with open(os.path.join(_ROOT, "pairing_amd", "csrc", "fl_gen.h")) as f:
        src = f.read()
    cu = [int(t) for t in re.search(r"FL_SUB_CU\[14\] = \{([^}]*)\}", src).group(1).split(",")]
    body = re.search(r"FL_SUB_C\[14\]\[14\] = \{(.*?)\};", src, re.S).group(1)
    rows = [[int(t.rstrip("u"), 16) for t in r.split(",")] for r in re.findall(r"\{([^{}]*)\}", body)]
    assert len(rows) == 14 and all(len(r) == NL for r in rows) and len(cu) == 14
    return rows, cu


def val(limbs):
    return sum(int(w) << (LB * i) for i, w in enumerate(limbs[:NL]))


def digits(v):
    """normalized digits, the excess in the top limb"""
    return [(v >> (LB * i)) & M for i in range(NL - 1)] + [v >> TOP]


def plain(limbs):
    return val(limbs) * RINV % Q


def lazy_of(x):
    """the canonical lazy value of the residue x"""
    return x % Q * RP % Q


# ---- operand classes of a bound U ----
def limb_max(U):
    low = [U * M] * (NL - 1)
    return low + [(U * 2 * Q - 1 - val(low)) >> TOP]


def value_max(U):
    return digits(U * 2 * Q - 1)


def denorm(g, limbs, U, full=False):
    """the same integer with limbs pushed up (at most to U (2^28 - 1)) by
    borrowing from the limb above; a no-op for U = 1"""
    x = list(limbs)
    for i in range(NL - 2, -1, -1):
        t = min(x[i + 1], (U * M - x[i]) >> LB)
        if not full:
            t = g.randint(0, t)
        x[i] += t << LB
        x[i + 1] -= t
    return x


def rand_lazy(g, U):
    """limb-wise sum of U random normalized values below 2q"""
    x = [0] * NL
    for _ in range(U):
        for i, d in enumerate(digits(g.randrange(2 * Q))):
            x[i] += d
    return x


def lift(g, x, U, k=None):
    """a lazy value of bound U of the residue x (plain): x R' + k q, random k and limbs unless k is given"""
    v = lazy_of(x)
    kmax = (U * 2 * Q - 1 - v) // Q
    if k is None:
        return denorm(g, digits(v + g.randint(0, kmax) * Q), U)
    return digits(v + min(k, kmax) * Q)


def zeros(g, U):
    """every multiple of q below U 2q, normalized and with raised limbs"""
    out = []
    for k in range(2 * U):
        out.append(digits(k * Q))
        if U > 1 and k:
            out.append(denorm(g, digits(k * Q), U))
            out.append(denorm(g, digits(k * Q), U, full=True))
    return out


def edge_operands(g, U):
    """the classes every routine sees: limb-max, value-max, the non-canonical zeros,
    q +- 1, 2q - 1, Montgomery one (and one + q)"""
    one = RP % Q
    out = [limb_max(U), value_max(U)] + zeros(g, U)
    out += [digits(v) for v in (Q - 1, Q + 1, 2 * Q - 1, one, one + Q, 1)]
    if U > 1:
        out += [denorm(g, value_max(U), U, full=True), digits(U * 2 * Q - Q), digits(U * 2 * Q - Q + 1)]
    for x in out:
        assert all(0 <= w <= U * M for w in x) and val(x) < U * 2 * Q
    return out


def core_operands(U):
    return [limb_max(U), value_max(U), digits(0), digits(Q), digits(RP % Q)]


def operands(g, U, nrand):
    out = edge_operands(g, U)
    for i in range(nrand):
        x = rand_lazy(g, U)
        out.append(denorm(g, x, U) if i & 1 else x)
    return out


def pairs(g, UA, UB, nrand):
    """operand pairs: every edge of one side against the core of the other, then random pairs"""
    ea, eb = edge_operands(g, UA), edge_operands(g, UB)
    out = [(a, b) for a in ea for b in core_operands(UB)] + [(a, b) for a in core_operands(UA) for b in eb]
    out += [(rand_lazy(g, UA), rand_lazy(g, UB)) for _ in range(nrand)]
    return out


# ---- tower elements as lists of coefficient limb vectors ----
def tower_cases(g, ncoef, U, nrand):
    """structured and random elements of ncoef Fq coefficients (Fq2 pairs in order), bound U"""
    one = RP % Q
    cases = [[limb_max(U)] * ncoef, [value_max(U)] * ncoef, [digits(0)] * ncoef, [digits(Q)] * ncoef,
             [digits(Q - 1)] * ncoef, [digits(2 * Q - 1)] * ncoef,
             [digits(one)] + [digits(0)] * (ncoef - 1), [digits(one + Q)] + [digits(Q)] * (ncoef - 1)]
    cases.append([lift(g, Q - 1, U, 0)] * ncoef)                      # every coefficient -1
    cases.append([lift(g, Q - 1, U, 1 << 30)] * ncoef)                # ... at the top of the bound
    x = g.randrange(Q)
    cases.append([lift(g, x, U) for _ in range(ncoef)])               # all coefficients equal, different lifts
    cases.append([lift(g, x, U, 0)] * ncoef)
    for _ in range(4):                                                # c0 = c1 and c0 = -c1 in every Fq2
        xs = [g.randrange(Q) for _ in range(ncoef // 2)]
        cases.append([lift(g, xs[i // 2], U) for i in range(ncoef)])
        cases.append([lift(g, xs[i // 2] if i % 2 == 0 else Q - xs[i // 2], U) for i in range(ncoef)])
        cases.append([lift(g, xs[i // 2], U, i % 2) for i in range(ncoef)])         # x and x + q
        cases.append([lift(g, xs[i // 2] if i % 2 == 0 else Q - xs[i // 2], U, 1 - i % 2) for i in range(ncoef)])
    for pos in range(ncoef):                                          # sparse, the zeros in every form
        zs = zeros(g, U)
        cases.append([lift(g, g.randrange(1, Q), U) if i == pos else g.choice(zs) for i in range(ncoef)])
    cases.append([lift(g, g.randrange(Q), U, 1) for _ in range(ncoef)])            # every coefficient x + q
    cases.append([lift(g, g.randrange(Q), U, 1 << 30) for _ in range(ncoef)])      # ... x + the most q's
    edges = edge_operands(g, U)
    for _ in range(nrand):
        kind = g.randrange(4)
        if kind == 0:
            cases.append([rand_lazy(g, U) for _ in range(ncoef)])
        elif kind == 1:
            cases.append([denorm(g, rand_lazy(g, U), U) for _ in range(ncoef)])
        else:
            cases.append([g.choice(edges) if g.randrange(3) == 0 else rand_lazy(g, U) for _ in range(ncoef)])
    return cases


def f2_of(cs):
    return (plain(cs[0]), plain(cs[1]))


def f6_of(cs):
    return (f2_of(cs[0:2]), f2_of(cs[2:4]), f2_of(cs[4:6]))


def f12_of(cs):
    return (f6_of(cs[0:6]), f6_of(cs[6:12]))


def flat(e):
    """the Fq coefficients of a tower element in storage order"""
    if isinstance(e, int):
        return [e]
    return [x for c in e for x in flat(c)]


# ---- tower operations pymodel lacks ----
def f2sqr(a): return pm.f2mul(a, a)
def f2conj(a): return (a[0], (-a[1]) % Q)
def f2dbl(a): return pm.f2add(a, a)
def f2scale(a, k): return (a[0] * k % Q, a[1] * k % Q)


def f2pow(a, e):
    r = pm.F2ONE
    while e:
        if e & 1:
            r = pm.f2mul(r, a)
        a = pm.f2mul(a, a)
        e >>= 1
    return r


_XI = (1, 1)
_FROB = {}


def _frob_consts(power):
    """xi^((q^p - 1) / 3), xi^(2 (q^p - 1) / 3), xi^((q^p - 1) / 6): from the tower's definition"""
    if power not in _FROB:
        e = Q ** power - 1
        _FROB[power] = (f2pow(_XI, e // 3), f2pow(_XI, 2 * e // 3), f2pow(_XI, e // 6))
    return _FROB[power]


def f2frob(a, power):
    return f2conj(a) if power & 1 else a


def f6frob(a, power):
    c1, c2, _ = _frob_consts(power % 6)
    return (f2frob(a[0], power), pm.f2mul(f2frob(a[1], power), c1), pm.f2mul(f2frob(a[2], power), c2))


def f12frob(a, power):
    k = _frob_consts(power % 12)[2]
    c1 = f6frob(a[1], power)
    return (f6frob(a[0], power), tuple(pm.f2mul(c, k) for c in c1))


def f6sqr(a): return pm.f6mul(a, a)


def fq4_sqr(a, b):
    """(a + b s)^2 in Fq2[s] / (s^2 - xi)"""
    return pm.f2add(f2sqr(a), pm.f2xi(f2sqr(b))), f2dbl(pm.f2mul(a, b))


def gs_sqr(f):
    """Granger-Scott squaring (equals the square on the cyclotomic subgroup only)"""
    (a0, a1, a2), (b0, b1, b2) = f
    t0, t1 = fq4_sqr(a0, b1)
    t2, t3 = fq4_sqr(b0, a2)
    t4, t5 = fq4_sqr(a1, b2)
    m3 = lambda t, a: pm.f2sub(f2scale(t, 3), f2dbl(a))  # noqa: E731
    p3 = lambda t, b: pm.f2add(f2scale(t, 3), f2dbl(b))  # noqa: E731
    return ((m3(t0, a0), m3(t2, a1), m3(t4, a2)), (p3(pm.f2xi(t5), b0), p3(t1, b1), p3(t3, b2)))


def cyclotomic(f):
    """f^((q^6 - 1)(q^2 + 1))"""
    r = pm.f12mul(pm.f12conj(f), pm.f12inv(f))
    return pm.f12mul(f12frob(r, 2), r)


def mul_by_014(f, c0, c1, c4):
    return pm.f12mul(f, ((c0, c1, pm.F2ZERO), (pm.F2ZERO, c4, pm.F2ZERO)))


# ---- group law over Fq (ints) or Fq2 (pairs), restated from ec.rs ----
class Fp:
    zero, one = 0, 1
    add = staticmethod(lambda a, b: (a + b) % Q)
    sub = staticmethod(lambda a, b: (a - b) % Q)
    mul = staticmethod(lambda a, b: a * b % Q)
    neg = staticmethod(lambda a: -a % Q)


class Fp2:
    zero, one = pm.F2ZERO, pm.F2ONE
    add = staticmethod(pm.f2add)
    sub = staticmethod(pm.f2sub)
    mul = staticmethod(pm.f2mul)
    neg = staticmethod(pm.f2neg)


def jac_double(F, p):
    """dbl-2009-l (ec.rs double), z != 0"""
    x, y, z = p
    a = F.mul(x, x)
    b = F.mul(y, y)
    c = F.mul(b, b)
    d = F.add(x, b)
    d = F.sub(F.sub(F.mul(d, d), a), c)
    d = F.add(d, d)
    e = F.add(F.add(a, a), a)
    f = F.mul(e, e)
    z3 = F.mul(z, y)
    z3 = F.add(z3, z3)
    x3 = F.sub(F.sub(f, d), d)
    c8 = F.add(c, c)
    c8 = F.add(c8, c8)
    c8 = F.add(c8, c8)
    y3 = F.sub(F.mul(F.sub(d, x3), e), c8)
    return (x3, y3, z3)


def jac_add(F, s, o):
    """add-2007-bl (ec.rs add_assign): zero is z == 0, equal points double"""
    if s[2] == F.zero:
        return o
    if o[2] == F.zero:
        return s
    z1z1, z2z2 = F.mul(s[2], s[2]), F.mul(o[2], o[2])
    u1, u2 = F.mul(s[0], z2z2), F.mul(o[0], z1z1)
    s1, s2 = F.mul(F.mul(s[1], o[2]), z2z2), F.mul(F.mul(o[1], s[2]), z1z1)
    if u1 == u2 and s1 == s2:
        return jac_double(F, s)
    h = F.sub(u2, u1)
    i = F.add(h, h)
    i = F.mul(i, i)
    j = F.mul(h, i)
    r = F.sub(s2, s1)
    r = F.add(r, r)
    v = F.mul(u1, i)
    x3 = F.sub(F.sub(F.sub(F.mul(r, r), j), v), v)
    s1j = F.mul(s1, j)
    y3 = F.sub(F.mul(F.sub(v, x3), r), F.add(s1j, s1j))
    z3 = F.add(s[2], o[2])
    z3 = F.mul(F.sub(F.sub(F.mul(z3, z3), z1z1), z2z2), h)
    return (x3, y3, z3)


def jac_add_mixed(F, s, o):
    """madd-2007-bl (ec.rs add_assign_mixed), o = (x, y) a nonzero affine point"""
    if s[2] == F.zero:
        return (o[0], o[1], F.one)
    z1z1 = F.mul(s[2], s[2])
    u2 = F.mul(o[0], z1z1)
    s2 = F.mul(F.mul(o[1], s[2]), z1z1)
    if s[0] == u2 and s[1] == s2:
        return jac_double(F, s)
    h = F.sub(u2, s[0])
    hh = F.mul(h, h)
    i = F.add(hh, hh)
    i = F.add(i, i)
    j = F.mul(h, i)
    r = F.sub(s2, s[1])
    r = F.add(r, r)
    v = F.mul(s[0], i)
    x3 = F.sub(F.sub(F.sub(F.mul(r, r), j), v), v)
    jy = F.mul(j, s[1])
    y3 = F.sub(F.mul(F.sub(v, x3), r), F.add(jy, jy))
    z3 = F.add(s[2], h)
    z3 = F.sub(F.sub(F.mul(z3, z3), z1z1), hh)
    return (x3, y3, z3)


# ---- line steps, restated from mod.rs ----
def doubling_step(r):
    """mod.rs doubling_step: returns (r', (c0, c1, c2))"""
    F = Fp2
    x, y, z = r
    t0 = F.mul(x, x)
    t1 = F.mul(y, y)
    t2 = F.mul(t1, t1)
    t3 = F.add(t1, x)
    t3 = F.sub(F.sub(F.mul(t3, t3), t0), t2)
    t3 = F.add(t3, t3)
    t4 = F.add(F.add(t0, t0), t0)
    t6 = F.add(x, t4)
    t5 = F.mul(t4, t4)
    zsq = F.mul(z, z)
    x3 = F.sub(F.sub(t5, t3), t3)
    z3 = F.add(z, y)
    z3 = F.sub(F.sub(F.mul(z3, z3), t1), zsq)
    y3 = F.mul(F.sub(t3, x3), t4)
    t2 = f2scale(t2, 8)
    y3 = F.sub(y3, t2)
    c1 = F.neg(f2dbl(F.mul(t4, zsq)))
    c2 = F.sub(F.sub(F.sub(F.mul(t6, t6), t0), t5), f2scale(t1, 4))
    c0 = f2dbl(F.mul(z3, zsq))
    return (x3, y3, z3), (c0, c1, c2)


def addition_step(r, q):
    """mod.rs addition_step, q = (x, y) affine: returns (r', (c0, c1, c2))"""
    F = Fp2
    x, y, z = r
    qx, qy = q
    zsq = F.mul(z, z)
    ysq = F.mul(qy, qy)
    t0 = F.mul(zsq, qx)
    t1 = F.add(qy, z)
    t1 = F.mul(F.sub(F.sub(F.mul(t1, t1), ysq), zsq), zsq)
    t2 = F.sub(t0, x)
    t3 = F.mul(t2, t2)
    t4 = f2scale(t3, 4)
    t5 = F.mul(t4, t2)
    t6 = F.sub(F.sub(t1, y), y)
    t9 = F.mul(t6, qx)
    t7 = F.mul(t4, x)
    x3 = F.sub(F.sub(F.sub(F.mul(t6, t6), t5), t7), t7)
    z3 = F.add(z, t2)
    z3 = F.sub(F.sub(F.mul(z3, z3), zsq), t3)
    t10 = F.add(qy, z3)
    t8 = F.mul(F.sub(t7, x3), t6)
    t0 = f2dbl(F.mul(y, t5))
    y3 = F.sub(t8, t0)
    t10 = F.sub(F.sub(F.mul(t10, t10), ysq), F.mul(z3, z3))
    t9 = F.sub(f2dbl(t9), t10)
    return (x3, y3, z3), (f2dbl(z3), f2dbl(F.neg(t6)), t9)


def ell(f, coeffs, p):
    """mod.rs ell: f * (c2 + c1 p.x v + c0 p.y v w)"""
    c0, c1, c2 = coeffs
    return mul_by_014(f, c2, f2scale(c1, p[0]), f2scale(c0, p[1]))


def _x_bits():
    bits = [(BLS_X >> 1 >> i) & 1 for i in range(63, -1, -1)]
    return bits[bits.index(1) + 1:]


def g2_prepare(q):
    """G2Prepared::from_affine for a nonzero affine q: the 68 line coefficients"""
    coeffs = []
    r = (q[0], q[1], pm.F2ONE)
    for bit in _x_bits():
        r, c = doubling_step(r)
        coeffs.append(c)
        if bit:
            r, c = addition_step(r, q)
            coeffs.append(c)
    r, c = doubling_step(r)
    coeffs.append(c)
    return coeffs


def miller_loop(p, coeffs):
    """Engine::miller_loop for one pair (BLS_X is negative: conjugate at the end)"""
    it = iter(coeffs)
    f = pm.F12ONE
    for bit in _x_bits():
        f = ell(f, next(it), p)
        if bit:
            f = ell(f, next(it), p)
        f = pm.f12sqr(f)
    f = ell(f, next(it), p)
    return pm.f12conj(f)
