"""CPU model of the lazy base field (pairing_amd/csrc/fl.h, fl_gen.h): the
constants the kernels compile against, an exact integer model of the one-pass
`red`, and a big-integer replay of the product leaves' column scan at the
column limit.  The constants are read out of the committed fl_gen.h (and the
two shifts of `red` out of fl.h) with regular expressions -- not imported from
the generator -- so that what is checked is what the kernels are built from.

Conversion constants, derived from fl.h:
  fl_from_abi(x) = mul(fl_split(x), FL_TO) = x FL_TO / R' with R' = 2^392.  The
  ABI word x holds a 2^384 (Montgomery, R = 2^384) and the lazy form of a is
  a 2^392, so FL_TO = 2^392 2^392 / 2^384 = 2^400 mod q.
  fl_to_abi(y) = mul(red(y), FL_FROM) = y FL_FROM / R'.  y = a 2^392 and the
  ABI wants a 2^384, so FL_FROM = 2^384 mod q.
"""
import os
import random
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "pairing_amd", "csrc")
Q = 0x1a0111ea397fe69a4b1ba7b6434bacd764774b84f38512bf6730d2a0f6b0f6241eabfffeb153ffffb9feffffffffaaab
LB, NL = 28, 14
M = (1 << LB) - 1
RP = 1 << (LB * NL)   # R' = 2^392

# rows B of FL_SUB_C whose value is exactly FL_SUB_CU[B-1] * 2q: neg<B>(0) meets the
# value bound of its result type with equality (fl.h states the bound as <=)
SUB_C_AT_BOUND = [3, 4, 7, 8, 11, 12, 13]


def _read(name):
    with open(os.path.join(CSRC, name)) as f:
        return f.read()


def _ints(text):
    return [int(t.rstrip("u"), 16) if t.startswith("0x") else int(t) for t in re.findall(r"0x[0-9a-fA-F]+u?|\d+", text)]


@pytest.fixture(scope="module")
def K():
    """the constants of fl_gen.h and the shifts of fl.h's red"""
    src = _read("fl_gen.h")
    c = {}
    for name in ("Q", "TO", "FROM", "ONE"):
        m = re.search(r"FL_%s\[14\] = \{([^}]*)\}" % name, src)
        c[name] = _ints(m.group(1))
        assert len(c[name]) == NL
    c["KQ"] = int(re.search(r"FL_KQ = (0x[0-9a-f]+)u;", src).group(1), 16)
    c["MASK"] = int(re.search(r"FL_MASK = (0x[0-9a-f]+)u;", src).group(1), 16)
    c["QINV"] = int(re.search(r"FL_QINV = (0x[0-9a-f]+)u;", src).group(1), 16)
    body = re.search(r"FL_SUB_C\[14\]\[14\] = \{(.*?)\};", src, re.S).group(1)
    c["SUB_C"] = [_ints(r) for r in re.findall(r"\{([^{}]*)\}", body)]
    assert len(c["SUB_C"]) == 14 and all(len(r) == NL for r in c["SUB_C"])
    c["SUB_CU"] = _ints(re.search(r"FL_SUB_CU\[14\] = \{([^}]*)\}", src).group(1))
    assert len(c["SUB_CU"]) == 14
    m = re.search(r"k = \(uint32_t\)\(\(p2 \+ \(p1 >> (\d+)\)\) >> (\d+)\);", _read("fl.h"))
    assert m, "red(): the quotient estimate is no longer where this model reads it"
    c["SH1"], c["SH2"] = int(m.group(1)), int(m.group(2))
    return c


def val(limbs):
    return sum(int(w) << (LB * i) for i, w in enumerate(limbs))


def digits(v):
    return [(v >> (LB * i)) & M for i in range(NL - 1)] + [v >> (LB * (NL - 1))]


def test_basic_constants(K):
    assert K["MASK"] == M
    assert all(w <= M for n in ("Q", "TO", "FROM", "ONE") for w in K[n])
    assert val(K["Q"]) == Q
    assert K["KQ"] == (1 << 400) // Q
    assert val(K["ONE"]) == RP % Q
    assert val(K["TO"]) == pow(2, 400, Q)       # docstring: 2^392 2^392 / 2^384
    assert val(K["FROM"]) == pow(2, 384, Q)
    assert K["QINV"] == (-pow(Q, -1, 1 << LB)) % (1 << LB)
    # the round trip the two constants exist for
    a = 0x123456789abcdef % Q
    lazy = (a << 384) % Q * val(K["TO"]) * pow(RP, -1, Q) % Q
    assert lazy == (a << 392) % Q
    assert lazy * val(K["FROM"]) * pow(RP, -1, Q) % Q == (a << 384) % Q


def test_sub_constants(K):
    """FL_SUB_C[B-1] = k q dominates, limb by limb, every value of bound B, and
    FL_SUB_CU[B-1] bounds it in turn (limbs and value, the value with <=)"""
    at_bound = []
    for B in range(1, 15):
        c, cu = K["SUB_C"][B - 1], K["SUB_CU"][B - 1]
        v = val(c)
        assert v % Q == 0, B
        assert all(c[i] >= B * M for i in range(NL - 1)), B
        # top limb of any value < B 2q (equality of the value bound included: B 2q >> 364 is the same)
        assert c[NL - 1] >= (B * 2 * Q - 1) >> (LB * (NL - 1)), B
        assert c[NL - 1] >= (B * 2 * Q) >> (LB * (NL - 1)), B
        assert all(w <= cu * M for w in c), B
        assert all(w < (1 << 32) for w in c), B
        assert v <= cu * 2 * Q, B
        if v == cu * 2 * Q:
            at_bound.append(B)
    assert at_bound == SUB_C_AT_BOUND
    # the bounds the types are built from: results up to 16 exist for B = 1..13 only
    assert [B for B in range(1, 15) if K["SUB_CU"][B - 1] <= 16] == list(range(1, 14))
    assert K["SUB_CU"] == sorted(K["SUB_CU"])


# ---------------------------------------------------------------- red ----
def red_model(K, x):
    """fl.h red() on 14 u32 limbs, every machine operation with its width:
    returns (k, result limbs); asserts that no u64 / i64 operation wraps"""
    assert len(x) == NL and all(0 <= w < (1 << 32) for w in x)
    p1 = x[12] * K["KQ"]
    p2 = x[13] * K["KQ"]
    assert p1 < (1 << 64) and p2 < (1 << 64)
    s = p2 + (p1 >> K["SH1"])
    assert s < (1 << 64)
    k = s >> K["SH2"]
    assert k < (1 << 32)
    r = []
    acc = 0
    for i in range(NL - 1):
        kq = k * K["Q"][i]
        assert kq < (1 << 63)
        acc += x[i] - kq
        assert -(1 << 63) <= acc < (1 << 63)
        r.append(acc & M)          # (uint32_t)acc & FL_MASK
        acc >>= LB                 # arithmetic shift of an int64_t
    acc += x[13] - k * K["Q"][13]
    assert -(1 << 63) <= acc < (1 << 63)
    r.append(acc & 0xffffffff)     # (uint32_t)acc
    return k, r, acc


def check_red(K, x):
    v = val(x)
    k, r, top = red_model(K, x)
    assert k in (v // Q, v // Q - 1) and k >= 0, (hex(v), k)
    assert top == r[13], "top limb went negative or past 32 bits"
    assert all(w <= M for w in r[:13])
    assert val(r) == v - k * Q
    assert 0 <= val(r) < 2 * Q
    assert r[13] <= (2 * Q - 1) >> (LB * (NL - 1))
    return k, r


def pushed(x, g=None):
    """the same integer with limbs 0..12 pushed towards 2^32 - 1 by borrowing
    from the limb above (top down, so that every limb finds something to
    borrow); with g, a random amount per limb"""
    x = list(x)
    for i in range(NL - 2, -1, -1):
        t = min(x[i + 1], ((1 << 32) - 1 - x[i]) >> LB)
        if g is not None:
            t = g.randint(0, t)
        x[i] += t << LB
        x[i + 1] -= t
    return x


def test_red_model_quotient_and_range(K):
    """k = floor(V / q) or one less and V - k q in [0, 2q) with limbs 0..12 below
    2^28, for every V < 2^388 around a multiple of q, whatever the limbs"""
    assert (K["SH1"], K["SH2"]) == (28, 36)
    g = random.Random(1)
    n = 0
    seen_q = False
    m = 0
    while m * Q < (1 << 388):
        for v in (m * Q - 1, m * Q, m * Q + 1):
            if v < 0 or v >= (1 << 388):
                continue
            d = digits(v)
            forms = [d, pushed(d), pushed(d, g), pushed(d, g)]
            assert all(val(f) == v for f in forms)
            assert d[13] < 15 or min(pushed(d)[:13]) >= (1 << 32) - (1 << 28) - 15
            for f in forms:
                k, r = check_red(K, f)
                n += 1
                if v == m * Q and m and val(r) == Q:
                    seen_q = True
        m += 1
    assert m > 150 and n > 1500
    # red alone leaves a multiple of q as 0 OR q: fl_is_zero needs its fl_canon
    assert seen_q
    for _ in range(4000):
        v = g.randrange(1 << 388)
        d = digits(v)
        check_red(K, d)
        check_red(K, pushed(d, g))


def test_red_model_at_the_type_bounds(K):
    """operands of every bound U at their limits: limb-maximal, value-maximal
    (U 2q - 1) and the value U 2q itself, which neg of a zero produces"""
    for U in range(1, 17):
        top = U * 2 * Q
        low = [U * M] * (NL - 1)
        limbmax = low + [(top - 1 - val(low)) >> (LB * (NL - 1))]
        assert limbmax[13] <= U * M and val(limbmax) < top
        for x in (limbmax, digits(top - 1), digits(top), pushed(digits(top))):
            check_red(K, x)
    for B in SUB_C_AT_BOUND:
        k, r = check_red(K, K["SUB_C"][B - 1])
        assert val(r) in (0, Q)


# ------------------------------------------------- the product leaves ----
def leaf_replay(K, prods, square=False):
    """the column scan of pa_fl_sop<K> / pa_fl_sqr (tools/gen_fl.py) with exact
    integers: prods = [(a, b), ...] limb vectors.  Returns (result limbs, the
    largest value the 64-bit accumulator held)."""
    q, qinv = K["Q"], K["QINV"]
    acc, peak = 0, 0
    mdig = []
    out = [0] * NL
    for k in range(2 * NL - 1):
        for a, b in prods:
            for i in range(max(0, k - (NL - 1)), min(k, NL - 1) + 1):
                j = k - i
                if square:
                    if i < j:
                        a2 = a[j] << 1
                        assert a2 < (1 << 32)
                        acc += a[i] * a2
                    elif i == j:
                        acc += a[i] * a[i]
                    else:
                        continue
                else:
                    acc += a[i] * b[j]
                peak = max(peak, acc)
        for i in range(max(0, k - (NL - 1)), min(k - 1, NL - 1) + 1):
            acc += mdig[i] * q[k - i]
            peak = max(peak, acc)
        if k < NL:
            mk = ((acc & 0xffffffff) * qinv) & 0xffffffff & M
            mdig.append(mk)
            acc += mk * q[0]
            peak = max(peak, acc)
            assert acc & M == 0
        else:
            out[k - NL] = acc & M
        acc >>= LB
    assert acc < (1 << 32)
    out[NL - 1] = acc
    return out, peak


def limb_max(U):
    low = [U * M] * (NL - 1)
    return low + [(U * 2 * Q - 1 - val(low)) >> (LB * (NL - 1))]


@pytest.mark.parametrize("bounds", [(1, 16), (16, 1), (4, 4), (2, 8), (4, 4, 1, 1), (8, 2, 1, 1), (3, 3, 2, 4),
                                    (16, 1, 1, 1), (1, 1, 4, 4), (3,)],
                         ids=lambda b: "x".join(map(str, b)))
def test_leaf_columns_fit_64_bits(K, bounds):
    """sum(U_x U_y) <= 17 (fl.h's static_assert) keeps every running column sum,
    the Montgomery m q terms included, below 2^64 -- with limb-maximal operands,
    value-maximal ones and operands of value exactly U 2q"""
    rinv = pow(RP, -1, Q)
    g = random.Random(7)
    kinds = [limb_max, lambda U: digits(U * 2 * Q - 1), lambda U: digits(U * 2 * Q),
             lambda U: [g.randrange(U * M + 1) for _ in range(NL - 1)] + [g.randrange((U * 2 * Q) >> 364)]]
    for kind in kinds:
        ops = [kind(U) for U in bounds]
        if len(bounds) == 1:
            assert bounds[0] <= 3
            r, peak = leaf_replay(K, [(ops[0], ops[0])], square=True)
            want = val(ops[0]) ** 2
        else:
            assert sum(bounds[i] * bounds[i + 1] for i in range(0, len(bounds), 2)) <= 17
            prods = [(ops[i], ops[i + 1]) for i in range(0, len(ops), 2)]
            r, peak = leaf_replay(K, prods)
            want = sum(val(a) * val(b) for a, b in prods)
        assert peak < (1 << 64), hex(peak)
        assert all(w <= M for w in r[:13])
        assert val(r) < 2 * Q
        assert val(r) % Q == want * rinv % Q
