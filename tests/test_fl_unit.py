"""GPU unit tests of the hand-written lazy layer -- fl.h, tower_fl.h,
curve_fl.h, curve_fl2.h, pairing_fl.h -- one routine per launch on RAW
operands at the bounds its type F<U> allows: limbs at U (2^28 - 1), values
just under (and, where a neg of zero can produce it, exactly) U 2q,
non-canonical zeros, x given as x + q, Jacobian points with a rescaled Z.
The reference is Python big integers (tests/fl_ref.py, pinned against the C
oracle by tests/test_fl_ref.py).  Every result must be congruent to the
reference mod q AND respect the bound of its own type, which the kernel
writes next to it: every limb <= U_out (2^28 - 1), value < U_out 2q.
Test-only code object: tests/hip/fl_unit.hip -> pairing_amd/lib/test/fl_unit.hsaco."""
import ctypes
import os
import random

import numpy as np
import pytest

import fl_ref as R
import pymodel as pm
from fl_ref import M, NL, RINV, RP, digits, lazy_of, plain, val
from helpers import Q, RMONT, mont

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CO = os.path.join(ROOT, "pairing_amd", "lib", "test", "fl_unit.hsaco")
IN_SLOTS, OUT_SLOTS = 24, 16
SUB_C, SUB_CU = R.sub_tables()
# neg<B>(0) = FL_SUB_C[B-1] is exactly FL_SUB_CU[B-1] 2q for these B (tests/test_fl_model.py)
AT_BOUND = [B for B in range(1, 14) if val(SUB_C[B - 1]) == SUB_CU[B - 1] * 2 * Q]
RED_U = [1, 2, 3, 4, 6, 8, 12, 16]


def cu(b):
    return SUB_CU[b - 1]


_launch_failed = []


def run(kernel, op, p, cases, raw=None, lanes=1):
    """cases[i] = operand slots (limb lists, None = zeros); raw[i] = (word offset, words) written on top;
    lanes = lanes per case (64-lane blocks).
    After a launch that raised (a HIP error), nothing more is launched from this module."""
    import torch
    import hipmod
    if _launch_failed:
        pytest.fail("an earlier launch failed (%s): not launching again" % _launch_failed[0])
    n = len(cases)
    assert 0 < n <= 4096
    buf = np.zeros((n, IN_SLOTS * 16), dtype=np.uint32)
    for i, slots in enumerate(cases):
        assert len(slots) <= IN_SLOTS
        for k, s in enumerate(slots):
            if s is not None:
                buf[i, 16 * k:16 * k + len(s)] = s
        if raw is not None:
            off, words = raw[i]
            buf[i, off:off + len(words)] = words
    src = torch.from_numpy(buf.view(np.int32)).cuda()
    out = torch.zeros((n, OUT_SLOTS, 16), dtype=torch.int32, device="cuda")
    try:
        hipmod.launch_kernel(CO, kernel,
                             [(ctypes.c_uint64, src.data_ptr()), (ctypes.c_uint64, out.data_ptr()),
                              (ctypes.c_uint32, n), (ctypes.c_uint32, op), (ctypes.c_uint32, p)],
                             (n * lanes + 63) // 64, 64)
        res = out.cpu().numpy().view(np.uint32)
    except BaseException as e:
        _launch_failed.append("%s op %d p %d: %r" % (kernel, op, p, e))
        raise
    return res


def check(rec, want, u=None, eq_ok=False, ctx=None):
    """rec = 16 words of a result slot; want = any integer congruent to the lazy result"""
    limbs = [int(w) for w in rec[:NL]]
    U = int(rec[14])
    assert 1 <= U <= 16 and (u is None or U == u), (ctx, U, u)
    assert all(w <= U * M for w in limbs), (ctx, U, [hex(w) for w in limbs])
    v = val(limbs)
    assert v < U * 2 * Q or (eq_ok and v == U * 2 * Q), (ctx, U, hex(v))
    assert v % Q == want % Q, (ctx, hex(v % Q), hex(want % Q))
    return v


def words_of(v, n=12):
    return [(v >> (32 * j)) & 0xffffffff for j in range(n)]


def abi_of(rec):
    assert not rec[12:].any()
    return sum(int(w) << (32 * j) for j, w in enumerate(rec[:12]))


def at_bound(U):
    """operands of value exactly U 2q (what neg of a zero hands on), normalized and with raised limbs"""
    g = random.Random(U)
    top = digits(U * 2 * Q)
    return [top] if U == 1 else [top, R.denorm(g, top, U), R.denorm(g, top, U, full=True)]


# =========================================================== fl.h ==========
@pytest.mark.parametrize("p,ua,ub", [(0, 1, 1), (1, 8, 8), (2, 15, 1), (3, 3, 4)])
def test_add(p, ua, ub):
    g = random.Random(10 + p)
    cases = R.pairs(g, ua, ub, 100)
    out = run("fl_unit_base", 0, p, [[a, b] for a, b in cases])
    for i, (a, b) in enumerate(cases):
        v = check(out[i, 0], val(a) + val(b), u=ua + ub, ctx=("add", p, i))
        assert v == val(a) + val(b)


@pytest.mark.parametrize("u", [1, 8])
def test_dbl(u):
    ops = R.operands(random.Random(20 + u), u, 100)
    out = run("fl_unit_base", 1, u, [[a] for a in ops])
    for i, a in enumerate(ops):
        assert check(out[i, 0], 2 * val(a), u=2 * u, ctx=("dbl", u, i)) == 2 * val(a)


@pytest.mark.parametrize("b", range(1, 13))
def test_sub(b):
    """a + C_B - b never borrows in a limb, whatever a value of bound B looks like,
    and lands inside the bound A + FL_SUB_CU[B-1] of its type"""
    g = random.Random(30 + b)
    for op, ua in ((2, 1), (3, 16 - cu(b))):
        cases = R.pairs(g, ua, b, 100)
        cases += [(a, t) for a in R.core_operands(ua) for t in at_bound(b) if b > 1]   # subtrahend of value B 2q
        out = run("fl_unit_base", op, b, [[a, t] for a, t in cases])
        for i, (a, t) in enumerate(cases):
            v = check(out[i, 0], val(a) - val(t), u=ua + cu(b), ctx=("sub", ua, b, i))
            assert v == val(a) + val(SUB_C[b - 1]) - val(t)
            assert all(int(out[i, 0, k]) == a[k] + SUB_C[b - 1][k] - t[k] for k in range(NL))


@pytest.mark.parametrize("b", range(1, 14))
def test_neg(b):
    """neg<B>: for B in AT_BOUND, neg(0) has the value FL_SUB_CU[B-1] 2q exactly --
    the one place a lazy value meets its bound with equality"""
    g = random.Random(50 + b)
    ops = R.operands(g, b, 100) + (at_bound(b) if b > 1 else [])
    out = run("fl_unit_base", 4, b, [[a] for a in ops])
    hit = False
    for i, a in enumerate(ops):
        v = check(out[i, 0], -val(a), u=cu(b), eq_ok=True, ctx=("neg", b, i))
        assert v == val(SUB_C[b - 1]) - val(a)
        if v == cu(b) * 2 * Q:
            assert val(a) == 0
            hit = True
    assert hit == (b in AT_BOUND)


@pytest.mark.parametrize("u", RED_U)
def test_red(u):
    """one pass to F<1>: value < 2q, limbs 0..12 < 2^28 -- also from exactly U 2q"""
    g = random.Random(70 + u)
    ops = R.operands(g, u, 200) + (at_bound(u) if u > 1 else [])   # red(F<1>) is the identity
    out = run("fl_unit_base", 5, u, [[a] for a in ops])
    for i, a in enumerate(ops):
        v = check(out[i, 0], val(a), u=1, ctx=("red", u, i))
        assert (val(a) - v) // Q in (val(a) // Q, val(a) // Q - 1)


def _with_bound_cases(g, ua, ub, nrand):
    cases = R.pairs(g, ua, ub, nrand)
    cases += [(a, b) for a in at_bound(ua) if ua > 1 for b in R.core_operands(ub)]
    cases += [(a, b) for b in at_bound(ub) if ub > 1 for a in R.core_operands(ua)]
    cases += [(a, b) for a in at_bound(ua) if ua > 1 for b in at_bound(ub) if ub > 1]
    return cases


@pytest.mark.parametrize("p,ua,ub", [(0, 1, 1), (1, 1, 16), (2, 16, 1), (3, 4, 4), (4, 2, 8)])
def test_mul_leaf_at_the_column_limit(p, ua, ub):
    g = random.Random(90 + p)
    cases = _with_bound_cases(g, ua, ub, 150)
    out = run("fl_unit_base", 6, p, [[a, b] for a, b in cases])
    for i, (a, b) in enumerate(cases):
        check(out[i, 0], val(a) * val(b) * RINV, u=1, ctx=("mul", p, i))


@pytest.mark.parametrize("u", [1, 2, 3])
def test_sqr_leaf(u):
    g = random.Random(100 + u)
    ops = R.operands(g, u, 150) + (at_bound(u) if u > 1 else [])
    out = run("fl_unit_base", 7, u, [[a] for a in ops])
    for i, a in enumerate(ops):
        check(out[i, 0], val(a) ** 2 * RINV, u=1, ctx=("sqr", u, i))


@pytest.mark.parametrize("p,bounds", [(0, (1, 1, 1, 1)), (1, (4, 4, 1, 1)), (2, (8, 2, 1, 1)), (3, (3, 3, 2, 4))])
def test_sop_leaf_at_the_column_limit(p, bounds):
    g = random.Random(110 + p)
    cases = [[R.limb_max(u) for u in bounds], [R.value_max(u) for u in bounds],
             [at_bound(u)[-1] if u > 1 else R.limb_max(u) for u in bounds],
             [at_bound(u)[0] if u > 1 else R.value_max(u) for u in bounds], [digits(0)] * 4, [digits(Q)] * 4]
    edges = [R.edge_operands(g, u) + (at_bound(u) if u > 1 else []) for u in bounds]
    for _ in range(300):
        cases.append([g.choice(edges[k]) if g.randrange(3) == 0 else R.rand_lazy(g, u) for k, u in enumerate(bounds)])
    out = run("fl_unit_base", 8, p, cases)
    for i, (a, b, c, d) in enumerate(cases):
        check(out[i, 0], (val(a) * val(b) + val(c) * val(d)) * RINV, u=1, ctx=("sop", p, i))


def test_canon_pack_split():
    g = random.Random(120)
    ops = R.operands(g, 1, 200)
    for i, rec in enumerate(run("fl_unit_base", 9, 0, [[a] for a in ops])):       # fl_canon: the unique value < q
        assert [int(w) for w in rec[0, :NL]] == digits(val(ops[i]) % Q) and rec[0, 14] == 1
    for i, rec in enumerate(run("fl_unit_base", 17, 0, [[a] for a in ops])):      # fl_pack: the same integer
        assert abi_of(rec[0]) == val(ops[i])
    for i, rec in enumerate(run("fl_unit_base", 11, 0, [[a] for a in ops])):      # fl_pack_canon
        assert abi_of(rec[0]) == val(ops[i]) % Q
    vals = [0, 1, Q - 1, Q, 2 * Q - 1, (1 << 384) - 1, RMONT, (1 << 364) - 1, 1 << 364] + \
        [g.randrange(1 << 384) for _ in range(100)]
    out = run("fl_unit_base", 10, 0, [[words_of(v)] for v in vals])               # fl_split, and fl_pack back
    for i, v in enumerate(vals):
        assert [int(w) for w in out[i, 0, :NL]] == digits(v) and all(int(w) <= M for w in out[i, 0, :NL])
        assert abi_of(out[i, 1]) == v


def test_from_abi():
    g = random.Random(130)
    vals = [0, 1, 2, Q - 1, Q - 2, (Q - 1) // 2, RMONT, ((1 << 380) - 1) % Q] + [g.randrange(Q) for _ in range(200)]
    out = run("fl_unit_base", 12, 0, [[words_of(v)] for v in vals])
    for i, v in enumerate(vals):
        check(out[i, 0], v << 8, u=1, ctx=("from_abi", i))    # x 2^400 / 2^392


@pytest.mark.parametrize("u", RED_U)
def test_to_abi_and_store(u):
    """the 12 ABI words are value R'^-1 2^384 mod q, canonical, from any lazy form"""
    g = random.Random(140 + u)
    ops = R.operands(g, u, 150) + (at_bound(u) if u > 1 else [])
    for op in (13, 15):
        out = run("fl_unit_base", op, u, [[a] for a in ops])
        for i, a in enumerate(ops):
            assert abi_of(out[i, 0]) == (val(a) * RINV << 384) % Q, (op, u, i)


@pytest.mark.parametrize("u", RED_U)
def test_is_zero_exactly_on_multiples_of_q(u):
    g = random.Random(160 + u)
    ops = R.operands(g, u, 100) + (at_bound(u) if u > 1 else [])
    for k in range(2 * u):
        ops += [digits(k * Q + 1)] + ([digits(k * Q - 1)] if k else [])
        ops += [R.denorm(g, digits(k * Q + 1), u)]
    out = run("fl_unit_base", 14, u, [[a] for a in ops])
    nz = 0
    for i, a in enumerate(ops):
        assert int(out[i, 0, 15]) == (1 if val(a) % Q == 0 else 0), (u, i, hex(val(a)))
        nz += val(a) % Q == 0
    assert nz >= 2 * u


def test_fl_inv():
    g = random.Random(170)
    one = RP % Q
    ops = [digits(0), digits(Q), digits(one), digits(one + Q), digits(Q - 1), digits(2 * Q - 1), digits(1),
           digits(Q + 1), R.limb_max(1), lazy_digits(Q - 1)] + [R.rand_lazy(g, 1) for _ in range(54)]
    out = run("fl_unit_base", 16, 0, [[a] for a in ops])
    for i, a in enumerate(ops):
        x = plain(a)
        assert int(out[i, 0, 15]) == (0 if x == 0 else 1), i
        check(out[i, 0], lazy_of(pow(x, Q - 2, Q)), u=1, ctx=("inv", i))
    assert not out[0, 0, 15] and not out[1, 0, 15]


def lazy_digits(x):
    return digits(lazy_of(x))


# ====================================================== tower_fl.h ==========
def check_elem(recs, want, u=None, ctx=None):
    """recs = result slots, want = tower element (plain residues)"""
    for k, w in enumerate(R.flat(want)):
        check(recs[k], lazy_of(w), u=u, ctx=(ctx, k))


def two(g, na, ua, nb, ub, nrand):
    """operand pairs of two tower elements: structured against structured, then shuffled"""
    a, b = R.tower_cases(g, na, ua, nrand), R.tower_cases(g, nb, ub, nrand)
    n = min(len(a), len(b))
    out = [(a[i], b[i]) for i in range(n)] + [(a[i], b[(7 * i + 3) % n]) for i in range(n)]
    if na == nb and ua == ub:
        out += [(a[i], a[i]) for i in range(0, n, 3)]
    return out


@pytest.mark.parametrize("p,ua,ub", [(0, 1, 1), (1, 1, 2), (2, 2, 1), (3, 2, 2), (4, 4, 1), (5, 1, 4), (6, 3, 1)])
def test_f2_mul(p, ua, ub):
    """both operand orders of the neg branch; a zero c1 of bound 3 makes neg hand a
    value of exactly 4 2q to the sum-of-products leaf"""
    g = random.Random(200 + p)
    assert (cu(ua) * ub <= ua * cu(ub)) == (p in (0, 2, 3, 4, 6))
    cases = two(g, 2, ua, 2, ub, 60)
    out = run("fl_unit_tower", 0, p, [a + b for a, b in cases])
    for i, (a, b) in enumerate(cases):
        check_elem(out[i], pm.f2mul(R.f2_of(a), R.f2_of(b)), u=1, ctx=("f2mul", p, i))


@pytest.mark.parametrize("u", [1, 2])
def test_f2_sqr(u):
    """(a0 + a1)(a0 - a1) for U = 1, the sum-of-products form for U = 2; c0 = +-c1 included"""
    cases = R.tower_cases(random.Random(210 + u), 2, u, 150)
    out = run("fl_unit_tower", 1, u, cases)
    for i, a in enumerate(cases):
        check_elem(out[i], R.f2sqr(R.f2_of(a)), u=1, ctx=("f2sqr", u, i))


@pytest.mark.parametrize("op,u,name", [(2, 1, "mul_xi"), (2, 2, "mul_xi"), (2, 4, "mul_xi"), (3, 1, "conj"), (3, 2, "conj")])
def test_f2_linear(op, u, name):
    cases = R.tower_cases(random.Random(220 + 10 * op + u), 2, u, 100)
    out = run("fl_unit_tower", op, u, cases)
    for i, a in enumerate(cases):
        x = R.f2_of(a)
        if op == 2:
            check_elem(out[i], pm.f2xi(x), u=u + cu(u), ctx=(name, u, i))
        else:
            check_elem(out[i], R.f2conj(x), u=max(u, cu(u)), ctx=(name, u, i))


@pytest.mark.parametrize("p,u", [(0, 1), (1, 4)])
def test_f2_mul_by_fq(p, u):
    g = random.Random(230 + p)
    a, b = R.tower_cases(g, 2, u, 80), R.operands(g, u, 80)
    cases = [(a[i % len(a)], b[(3 * i + 1) % len(b)]) for i in range(max(len(a), len(b)))]
    cases += [(a[i], c) for i in range(2) for c in R.core_operands(u) + (at_bound(u) if u > 1 else [])]
    out = run("fl_unit_tower", 4, p, [x + [c] for x, c in cases])
    for i, (x, c) in enumerate(cases):
        check_elem(out[i], R.f2scale(R.f2_of(x), plain(c)), u=1, ctx=("mul_by_fq", p, i))


@pytest.mark.parametrize("p,ua,ub", [(0, 1, 1), (1, 1, 2), (2, 2, 1), (3, 2, 2)])
def test_f6_mul(p, ua, ub):
    g = random.Random(240 + p)
    cases = two(g, 6, ua, 6, ub, 50)
    out = run("fl_unit_tower", 5, p, [a + b for a, b in cases])
    for i, (a, b) in enumerate(cases):
        check_elem(out[i], pm.f6mul(R.f6_of(a), R.f6_of(b)), u=1, ctx=("f6mul", p, i))


@pytest.mark.parametrize("p,uc", [(0, 1), (1, 2)])
def test_f6_sparse_products(p, uc):
    g = random.Random(250 + p)
    cases = two(g, 6, 1, 2, uc, 50)
    out = run("fl_unit_tower", 6, p, [a + c for a, c in cases])                    # mul_by_1
    for i, (a, c) in enumerate(cases):
        want = pm.f6mul(R.f6_of(a), (pm.F2ZERO, R.f2_of(c), pm.F2ZERO))
        check_elem(out[i], want, u=1, ctx=("mul_by_1", p, i))
    c0s = R.tower_cases(g, 2, 1, 50)
    trip = [(a, c0s[(5 * i + 1) % len(c0s)], c) for i, (a, c) in enumerate(cases)]
    out = run("fl_unit_tower", 7, p, [a + c0 + c1 for a, c0, c1 in trip])           # mul_by_01
    for i, (a, c0, c1) in enumerate(trip):
        want = pm.f6mul(R.f6_of(a), (R.f2_of(c0), R.f2_of(c1), pm.F2ZERO))
        check_elem(out[i], want, u=1, ctx=("mul_by_01", p, i))


@pytest.mark.parametrize("u", [1, 2])
def test_f6_mul_v(u):
    cases = R.tower_cases(random.Random(260 + u), 6, u, 60)
    out = run("fl_unit_tower", 8, u, cases)
    for i, a in enumerate(cases):
        check_elem(out[i], pm.f6v(R.f6_of(a)), u=u + cu(u), ctx=("mul_v", u, i))


@pytest.fixture(scope="module")
def f6_cases():
    return R.tower_cases(random.Random(270), 6, 1, 60)


@pytest.fixture(scope="module")
def f12_cases():
    return R.tower_cases(random.Random(280), 12, 1, 60)


@pytest.mark.parametrize("power", range(6))
def test_f6_frobenius(f6_cases, power):
    out = run("fl_unit_tower", 9, power, f6_cases)
    for i, a in enumerate(f6_cases):
        check_elem(out[i], R.f6frob(R.f6_of(a), power), u=1, ctx=("f6frob", power, i))


@pytest.mark.parametrize("power", range(12))
def test_f12_frobenius(f12_cases, power):
    out = run("fl_unit_tower", 13, power, f12_cases)
    for i, a in enumerate(f12_cases):
        check_elem(out[i], R.f12frob(R.f12_of(a), power), u=1, ctx=("f12frob", power, i))


def test_f12_mul_sqr_conj(f12_cases):
    g = random.Random(290)
    n = len(f12_cases)
    other = R.tower_cases(g, 12, 1, 60)
    cases = [(f12_cases[i], other[i]) for i in range(n)] + [(f12_cases[i], other[(7 * i + 3) % n]) for i in range(n)]
    out = run("fl_unit_tower", 10, 0, [a + b for a, b in cases])
    for i, (a, b) in enumerate(cases):
        check_elem(out[i], pm.f12mul(R.f12_of(a), R.f12_of(b)), u=1, ctx=("f12mul", i))
    out = run("fl_unit_tower", 11, 0, f12_cases)
    for i, a in enumerate(f12_cases):
        check_elem(out[i], pm.f12sqr(R.f12_of(a)), u=1, ctx=("f12sqr", i))
    out = run("fl_unit_tower", 14, 0, f12_cases)
    for i, a in enumerate(f12_cases):
        check_elem(out[i], pm.f12conj(R.f12_of(a)), u=2, ctx=("f12conj", i))


def test_f12_mul_by_014(f12_cases):
    g = random.Random(300)
    cs = R.tower_cases(g, 6, 1, 80)
    cases = [(f12_cases[i % len(f12_cases)], cs[i]) for i in range(len(cs))]
    out = run("fl_unit_tower", 12, 0, [a + c for a, c in cases])
    for i, (a, c) in enumerate(cases):
        want = R.mul_by_014(R.f12_of(a), R.f2_of(c[0:2]), R.f2_of(c[2:4]), R.f2_of(c[4:6]))
        check_elem(out[i], want, u=1, ctx=("mul_by_014", i))


def test_fq4_and_cyclotomic_sqr(f12_cases):
    g = random.Random(310)
    cases = R.tower_cases(g, 4, 1, 100)
    out = run("fl_unit_tower", 15, 0, cases)
    for i, a in enumerate(cases):
        r0, r1 = R.fq4_sqr(R.f2_of(a[0:2]), R.f2_of(a[2:4]))
        check_elem(out[i], (r0, r1), u=1, ctx=("fq4_sqr", i))
    # on the cyclotomic subgroup Granger-Scott IS the square (every coefficient as x or x + q) ...
    cyc = []
    for _ in range(24):
        f = tuple(tuple((g.randrange(Q), g.randrange(Q)) for _ in range(3)) for _ in range(2))
        c = R.cyclotomic(f)
        assert R.gs_sqr(c) == pm.f12sqr(c)
        cyc.append([R.lift(g, x, 1) for x in R.flat(c)])
    out = run("fl_unit_tower", 16, 0, cyc)
    for i, a in enumerate(cyc):
        check_elem(out[i], pm.f12sqr(R.f12_of(a)), u=1, ctx=("cyclotomic_sqr", i))
    # ... and off it the same formula, restated, carries the edge operands
    out = run("fl_unit_tower", 16, 0, f12_cases)
    for i, a in enumerate(f12_cases):
        check_elem(out[i], R.gs_sqr(R.f12_of(a)), u=1, ctx=("granger_scott", i))


@pytest.mark.parametrize("op,ncoef,of,inv", [(17, 2, R.f2_of, pm.f2inv), (18, 6, R.f6_of, pm.f6inv),
                                              (19, 12, R.f12_of, pm.f12inv)], ids=["f2", "f6", "f12"])
def test_tower_inverse(op, ncoef, of, inv):
    """zero in any form (0, q, mixed) reports ok == 0; everything else inverts"""
    g = random.Random(320 + op)
    cases = R.tower_cases(g, ncoef, 1, 30)
    cases += [[digits(Q if (i + k) % 2 else 0) for i in range(ncoef)] for k in range(2)]
    out = run("fl_unit_tower", op, 0, cases)
    zeros = 0
    for i, a in enumerate(cases):
        x = of(a)
        if not any(R.flat(x)):
            assert not out[i, :ncoef, 15].any(), i
            zeros += 1
            continue
        assert out[i, :ncoef, 15].all(), i
        check_elem(out[i], inv(x), u=1, ctx=("inverse", ncoef, i))
    assert zeros >= 4


# ============================================ curve_fl.h, curve_fl2.h ==========
class G1:
    F, n, kernel_ops = R.Fp, 1, (0, 1, 2)

    @staticmethod
    def rand(g):
        return g.randrange(1, Q)

    @staticmethod
    def lift(g, x, u=1, k=None):
        return [R.lift(g, x, u, k)]

    @staticmethod
    def of(cs):
        return plain(cs[0])


class G2:
    F, n, kernel_ops = R.Fp2, 2, (3, 4, 5)

    @staticmethod
    def rand(g):
        return (g.randrange(1, Q), g.randrange(1, Q))

    @staticmethod
    def lift(g, x, u=1, k=None):
        return [R.lift(g, x[0], u, k), R.lift(g, x[1], u, None if k is None else (k + 1) % 2 if k < 2 else k)]

    @staticmethod
    def of(cs):
        return R.f2_of(cs)


def _scale(F, p, lam):
    l2 = F.mul(lam, lam)
    return (F.mul(p[0], l2), F.mul(p[1], F.mul(l2, lam)), F.mul(p[2], lam))


def _lift_pt(G, g, p, k=None, u=(1, 1, 1)):
    return sum((G.lift(g, c, uu, k) for c, uu in zip(p, u)), [])


def _pt_of(G, cs):
    n = G.n
    return tuple(G.of(cs[n * k:n * k + n]) for k in range(len(cs) // n))


def _check_pt(G, recs, want, flag, ctx):
    for k, c in enumerate(want):
        for j, w in enumerate(R.flat(c)):
            rec = recs[G.n * k + j]
            check(rec, lazy_of(w), u=1, ctx=(ctx, k, j))
            assert int(rec[15]) == flag, ctx


def _raw_edges(G, g):
    """a 'point' whose coordinates are the extreme F<1> operands (the formulas are polynomial identities)"""
    e = [R.limb_max(1), R.value_max(1), digits(Q - 1), digits(Q + 1), digits(RP % Q)]
    return [g.choice(e) for _ in range(3 * G.n)]


@pytest.mark.parametrize("G", [G1, G2], ids=["g1", "g2"])
def test_jac_double(G):
    g = random.Random(400 + G.n)
    cases = [_lift_pt(G, g, tuple(G.rand(g) for _ in range(3))) for _ in range(100)]
    cases += [_raw_edges(G, g) for _ in range(40)]
    out = run("fl_unit_curve", G.kernel_ops[0], 0, cases)
    for i, s in enumerate(cases):
        _check_pt(G, out[i], R.jac_double(G.F, _pt_of(G, s)), 0, ("double", G.n, i))


def _add_cases(G, seed):
    """(kind, s limbs + o limbs): equality of lazy values decides between add, double and
    zero -- the same point as x and x + q, or with a rescaled Z, must take the doubling branch"""
    g = random.Random(seed)
    F = G.F
    cases, kinds = [], []

    def put(kind, s, o):
        cases.append(s + o)
        kinds.append(kind)
    for _ in range(24):
        p = tuple(G.rand(g) for _ in range(3))
        o = tuple(G.rand(g) for _ in range(3))
        neg = (p[0], F.neg(p[1]), p[2])
        lam = G.rand(g)
        put("same", _lift_pt(G, g, p, 0), _lift_pt(G, g, p, 0))
        put("same", _lift_pt(G, g, p, 0), _lift_pt(G, g, p, 1))                 # coordinates shifted by q
        put("same", _lift_pt(G, g, p, 1), _lift_pt(G, g, p))
        put("same", _lift_pt(G, g, p), _lift_pt(G, g, _scale(F, p, lam)))       # rescaled Z
        put("neg", _lift_pt(G, g, p), _lift_pt(G, g, neg))
        put("neg", _lift_pt(G, g, p, 1), _lift_pt(G, g, _scale(F, neg, lam), 0))
        for zk in (0, 1):                                                       # z given as 0 and as q
            zero = (p[0], p[1], F.zero)
            put("szero", _lift_pt(G, g, zero, zk), _lift_pt(G, g, o))
            put("ozero", _lift_pt(G, g, o), _lift_pt(G, g, zero, zk))
            put("zeros", _lift_pt(G, g, zero, zk), _lift_pt(G, g, (o[0], o[1], F.zero), 1 - zk))
        put("add", _lift_pt(G, g, p), _lift_pt(G, g, o))
        put("add", _lift_pt(G, g, p), _lift_pt(G, g, (p[0], o[1], p[2])))      # same x, other y
        put("add", _raw_edges(G, g), _raw_edges(G, g))
    return cases, kinds


def _add_want(G, c, kind):
    h = 3 * G.n
    s, o = _pt_of(G, c[:h]), _pt_of(G, c[h:])
    want = R.jac_add(G.F, s, o)
    if kind == "same":
        assert want == R.jac_double(G.F, s) and want[2] != G.F.zero
    if kind == "neg":
        assert want[2] == G.F.zero
    return want


@pytest.mark.parametrize("G", [G1, G2], ids=["g1", "g2"])
def test_jac_add(G):
    cases, kinds = _add_cases(G, 410 + G.n)
    out = run("fl_unit_curve", G.kernel_ops[2], 0, cases)
    for i, c in enumerate(cases):
        _check_pt(G, out[i], _add_want(G, c, kinds[i]), 0, ("add", kinds[i], G.n, i))


def test_jac_add_and_double_on_lane_quads():
    """fl_jac_add_q / fl_jac_double_q spread the products of the one-lane forms over
    the four lanes of a quad: the same cases, the same values, in every lane"""
    cases, kinds = _add_cases(G1, 430)
    assert len(cases) % 16        # the last block holds a partial set of quads
    out = run("fl_unit_curve_quad", 0, 0, cases, lanes=4)
    for i, c in enumerate(cases):
        want = _add_want(G1, c, kinds[i])
        for q in range(4):
            _check_pt(G1, out[i, 3 * q:], want, 0, ("add_q", kinds[i], i, q))
    g = random.Random(431)
    cases = [_lift_pt(G1, g, tuple(G1.rand(g) for _ in range(3))) for _ in range(60)] + \
        [_raw_edges(G1, g) for _ in range(30)]
    out = run("fl_unit_curve_quad", 1, 0, cases, lanes=4)
    for i, s in enumerate(cases):
        want = R.jac_double(R.Fp, _pt_of(G1, s))
        for q in range(4):
            _check_pt(G1, out[i, 3 * q:], want, 0, ("double_q", i, q))


@pytest.mark.parametrize("G", [G1, G2], ids=["g1", "g2"])
def test_jac_add_mixed(G):
    g = random.Random(420 + G.n)
    F = G.F
    cases, kinds, flags = [], [], []

    def put(kind, s, o, untouched=0):
        cases.append(s + o + [None] * (5 * G.n - len(s) - len(o)) + [[untouched]])
        kinds.append(kind)
        flags.append(untouched)

    def aff(g_, o, k=None):
        return _lift_pt(G, g_, o, k, u=(1, 2))
    for _ in range(24):
        p = tuple(G.rand(g) for _ in range(3))
        o = (G.rand(g), G.rand(g))
        lam = G.rand(g)
        put("same", _lift_pt(G, g, (o[0], o[1], F.one), 0), aff(g, o, 0))
        put("same", _lift_pt(G, g, (o[0], o[1], F.one), 1), aff(g, o, 0))
        put("same", _lift_pt(G, g, (o[0], o[1], F.one), 0), aff(g, o))
        put("same", _lift_pt(G, g, _scale(F, (o[0], o[1], F.one), lam)), aff(g, o))
        put("neg", _lift_pt(G, g, _scale(F, (o[0], F.neg(o[1]), F.one), lam)), aff(g, o))
        for zk in (0, 1):
            put("szero", _lift_pt(G, g, (p[0], p[1], F.zero), zk), aff(g, o))
        put("untouched", _lift_pt(G, g, p), aff(g, o), 1)
        put("untouched", _raw_edges(G, g), aff(g, o, 3), 1)
        put("add", _lift_pt(G, g, p), aff(g, o))
        put("add", _raw_edges(G, g), [x for c in range(G.n) for x in [g.choice([R.limb_max(1), R.value_max(1)])]]
            + [g.choice([R.limb_max(2), R.value_max(2), R.rand_lazy(g, 2)]) for _ in range(G.n)])
    assert 16 * 5 * G.n == {1: 16 * 5, 2: 16 * 10}[G.n]     # the kernel reads `untouched` from slot 5 / slot 10
    out = run("fl_unit_curve", G.kernel_ops[1], 0, cases)
    for i, c in enumerate(cases):
        s, o = _pt_of(G, c[:3 * G.n]), _pt_of(G, c[3 * G.n:5 * G.n])
        if flags[i]:
            s = (s[0], s[1], F.zero)        # the initial identity, whatever the registers hold
        want = R.jac_add_mixed(F, s, o)
        if kinds[i] == "same":
            assert want == R.jac_double(F, s) and want[2] != F.zero
        if kinds[i] == "neg":
            assert want[2] == F.zero
        _check_pt(G, out[i], want, 0, ("add_mixed", kinds[i], G.n, i))     # `untouched` is cleared


# ======================================================= pairing_fl.h ==========
def test_line_steps():
    g = random.Random(500)
    cases = R.tower_cases(g, 6, 1, 100)
    out = run("fl_unit_pairing", 0, 0, cases)
    for i, c in enumerate(cases):
        r, line = R.doubling_step(_pt_of(G2, c))
        check_elem(out[i], (r, line), u=1, ctx=("dbl_step", i))
    cases = R.tower_cases(g, 10, 1, 100)
    out = run("fl_unit_pairing", 1, 0, cases)
    for i, c in enumerate(cases):
        r, line = R.addition_step(_pt_of(G2, c[:6]), (R.f2_of(c[6:8]), R.f2_of(c[8:10])))
        check_elem(out[i], (r, line), u=1, ctx=("add_step", i))


def test_ell(f12_cases):
    """ell_fl reads the line record's canonical ABI words and folds the conversion of
    c0, c1 into the products by kx = P.x 2^400, ky = P.y 2^400"""
    g = random.Random(510)
    k400 = pow(pow(2, 400, Q), -1, Q)
    edge = [0, 1, Q - 1, (Q - 1) // 2]
    cases, raw, want = [], [], []
    ks = R.edge_operands(g, 1)
    for i, f in enumerate(f12_cases):
        rec = [g.choice(edge) if g.randrange(4) == 0 else g.randrange(Q) for _ in range(6)]
        if i == 0:
            rec = [0] * 6
        if i == 1:
            rec = [Q - 1] * 6
        kx, ky = (g.choice(ks) if i % 3 == 0 else R.rand_lazy(g, 1) for _ in range(2))
        cases.append(f + [None] * 5 + [kx, ky])
        words = []
        for c in rec:
            for w64 in mont(c):
                words += [w64 & 0xffffffff, w64 >> 32]
        raw.append((16 * 12, words))
        p = (val(kx) * k400 % Q, val(ky) * k400 % Q)
        want.append(R.ell(R.f12_of(f), ((rec[0], rec[1]), (rec[2], rec[3]), (rec[4], rec[5])), p))
    assert len(cases[0]) == 19
    out = run("fl_unit_pairing", 2, 0, cases, raw)
    for i in range(len(cases)):
        check_elem(out[i], want[i], u=1, ctx=("ell", i))
