"""The group law on bases of small order (tests/small_order_cases.py).

On the bases the rest of the suite uses, a running sum meets the exceptional
branches of the group law -- P + P, P + (-P), 0 + P, a table row d * B that is
the identity -- with probability about 2^-255.  A base of order m meets them at
about every m-th step.  E(Fq) has points of order 3, 11 and 33, E'(Fq2) points
of order 13 and 23; every entry here takes any on-curve point, so these are
plain inputs.

CPU part: the points are what they claim to be; the oracle agrees with the
affine integer arithmetic on them (before the GPU tests lean on it); the fixed
scalar list reaches every branch (small_order_cases.branch_witness).

GPU part: the G1 and G2 fixed-base entries, the Groth16 verifying key, the
per-item scalar multiplications, the per-op group law over all pairs (k T, j T)
and the MSM entries on such bases.  Fixed-base and MSM outputs are compared as
points with the oracle (zero results as zero), the nonzero ones bit for bit
after batch_normalization, and with the integers; Jacobian words of the
per-item entries bit for bit."""
import numpy as np
import pytest

import decode_cases as D
import groth16_ref as G
import groth16_verify_ref as V
import small_order_cases as C
from helpers import R_ORDER, limbs, random_scalars, rng, small_scalars, unmont

NT = 8
N = 64
G1_BASES = ["O3", "O11", "O33", "S+O3"]
G2_BASES = ["O13", "O23", "S+O13"]
TORSION_OF = {"S+O3": "O3", "S+O13": "O13"}      # the small-order part of the mixed bases
G1_WINDOWS = (None, 4, 16)
G2_WINDOWS = (None, 4, 15)


def _order(name):
    return C.ORDERS[TORSION_OF.get(name, name)]


def _int_mul(group, name, v):
    """v * base for any integer v, on Python ints: a table look-up for a
    small-order base, S-part by double-and-add plus the torsion part otherwise"""
    t = TORSION_OF.get(name, name)
    T = C.multiples(group, t)[v % C.ORDERS[t]]
    if name not in TORSION_OF:
        return T
    F = C.field(group)
    return D._ec_add(F, D._ec_mul(F, C.point(group, "S"), v % R_ORDER) if v % R_ORDER else None, T)


def _o(oracle, group, name):
    return getattr(oracle, "g%d_%s" % (group, name))


def _default_window(oracle, group, n):
    return getattr(oracle.lib(), "o_g%d_recommended_wnaf_for_num_scalars" % group)(n)


def _nonzero(group, v):
    fw = 6 if group == 1 else 12
    return v[:, 2 * fw:3 * fw].any(axis=1)


# ---------------- CPU: the points ----------------

@pytest.mark.parametrize("group,name", [(1, n) for n in C.G1_ORDERS] + [(2, n) for n in C.G2_ORDERS])
def test_points_have_the_stated_order_and_lie_outside_the_r_torsion(group, name):
    F, m = C.field(group), C.ORDERS[name]
    P = C.point(group, name)
    x, y = P
    assert F["mul"](y, y) == (D.rhs1(x) if group == 1 else D.rhs2(x))
    mult = C.multiples(group, name)              # asserts m P == 0
    assert len(mult) == m and all(M is not None for M in mult[1:]) and len(set(mult)) == m
    assert D._ec_mul(F, P, m) is None
    for p in (3, 11, 13, 23):
        if m % p == 0 and m != p:
            assert D._ec_mul(F, P, m // p) is not None
    # r P = (r mod m) P is not zero
    assert R_ORDER % m != 0
    if group == 1:
        assert D._ec_mul(F, P, R_ORDER) == mult[R_ORDER % m]


def test_mixed_bases_are_a_subgroup_point_plus_torsion():
    for group, name in ((1, "S+O3"), (2, "S+O13")):
        F, t = C.field(group), TORSION_OF[name]
        P, S = C.point(group, name), C.point(group, "S")
        assert D._ec_mul(F, S, R_ORDER) is None and S is not None
        assert D._ec_mul(F, P, R_ORDER) == C.multiples(group, t)[R_ORDER % C.ORDERS[t]]
        x, y = P
        assert F["mul"](y, y) == (D.rhs1(x) if group == 1 else D.rhs2(x))
    Sp = C.point(1, "S'")
    assert D._ec_mul(C.F1, Sp, R_ORDER) is None and Sp != C.point(1, "S")
    assert C.point(1, "O33") == D._ec_add(C.F1, C.point(1, "O3"), C.point(1, "O11"))


def test_jacobian_records_are_the_same_points(oracle):
    for group, name in ((1, "O11"), (2, "O23")):
        pts = list(C.multiples(group, name))
        j = C.jac_rows(group, pts)
        assert not _nonzero(group, j)[0] and _nonzero(group, j)[1:].all()
        assert not (j[1:, -6:] == j[1, -6:]).all()            # the z differ
        np.testing.assert_array_equal(_o(oracle, group, "into_affine")(j), C.aff_rows(group, pts))


# ---------------- CPU: the recoding and the branches ----------------

def test_comb_digits_edges():
    assert C.comb_digits(0) == [0] * 33
    assert C.comb_digits(128)[:2] == [128, 0] and C.comb_digits(129)[:2] == [-127, 1]
    assert C.comb_digits((1 << 256) - 1) == [-1] + [0] * 31 + [1]
    assert C.comb_digits(128 + 256 * 128)[:3] == [128, 128, 0]
    for v in C.scalar_ints(11):
        d = C.comb_digits(v)
        assert len(d) == 33 and all(-127 <= x <= 128 for x in d)
    top = 1 << 256
    assert C.wraps(top - 1, 4) and C.wraps(top - 15, 4) and not C.wraps(top - 17, 4) and C.wraps(top - 17, 16)
    assert not C.wraps(top - 2, 4) and not C.wraps(R_ORDER - 1, 16) and not C.wraps(top - 1, 0)
    assert C.branch_witness(3, 3) == {"zero_row": 1, "doubling": 0, "cancellation": 0, "restart": 0}
    assert C.branch_witness(1 + 256 * 256, 3)["doubling"] == 1             # 1 B, then 65536 B = 1 B
    w = C.branch_witness(1 + 2 * 256 * 256 + 256 ** 3, 3)                  # 1, then -1, then 1 again
    assert (w["cancellation"], w["restart"]) == (1, 1)


@pytest.mark.parametrize("m", sorted(C.ORDERS.values()))
def test_scalar_list_reaches_every_branch(oracle, m):
    vals = C.scalar_ints(m)
    assert len(vals) == 64 and all(0 <= v < 1 << 256 for v in vals)
    group = 1 if m in C.G1_ORDERS.values() else 2
    windows = [0] + [w or _default_window(oracle, group, N) for w in (G1_WINDOWS if group == 1 else G2_WINDOWS)]
    for window in windows:
        wit = [C.branch_witness(v, m, window) for v in vals]
        assert sum(w["zero_row"] > 0 for w in wit) >= 8, window
        assert sum(w["doubling"] > 0 for w in wit) >= 4, window
        assert sum(w["cancellation"] > 0 for w in wit) >= 4, window
        assert sum(w["restart"] > 0 for w in wit) >= 1, window
        # what the fixed-base tests ask for: at least half of the products are not zero
        assert not window or sum(C.wnaf_value(v, window) % m != 0 for v in vals) >= N // 2, window
    assert any(C.wraps(v, 4) for v in vals) and any(C.wraps(v, 16) and not C.wraps(v, 4) for v in vals)


# ---------------- CPU: the oracle against the integers ----------------

@pytest.mark.parametrize("group,name", [(1, n) for n in G1_BASES] + [(2, n) for n in G2_BASES])
def test_oracle_matches_the_integers(oracle, group, name):
    m = _order(name)
    vals = C.scalar_ints(m)[::4]                 # 16 of the list, the small multiples and wrap edges among them
    s = np.array([limbs(v, 4) for v in vals], np.uint64)
    P = C.point(group, name)
    into = _o(oracle, group, "into_affine")
    base = np.ascontiguousarray(np.repeat(C.aff(group, P)[None], len(vals), axis=0))
    want = C.aff_rows(group, [_int_mul(group, name, v) for v in vals])
    np.testing.assert_array_equal(into(_o(oracle, group, "affine_mul")(base, s)), want)
    if group == 1 and name not in TORSION_OF:    # the look-up against the full double-and-add
        assert [D._ec_mul(C.F1, P, v) if v else None for v in vals] == [_int_mul(group, name, v) for v in vals]
    j = C.jac(group, P, C.z_of(group, 3))[None]
    for window in (G1_WINDOWS if group == 1 else G2_WINDOWS):
        w = window or _default_window(oracle, group, len(vals))
        got = _o(oracle, group, "wnaf_fixed_base")(j, s, 1, window)
        want = C.aff_rows(group, [_int_mul(group, name, C.wnaf_value(v, w)) for v in vals])
        np.testing.assert_array_equal(into(got), want)
    if name not in TORSION_OF:
        ks = [1 + (7 * i + 3) % (m - 1) for i in range(len(vals))]
        bases = C.aff_rows(group, [C.multiples(group, name)[k] for k in ks])
        tot = sum(k * v for k, v in zip(ks, vals)) % m
        got = into(_o(oracle, group, "multiexp")(bases, s, 2))
        np.testing.assert_array_equal(got[0], C.aff(group, C.multiples(group, name)[tot]))


# ---------------- GPU: fixed base ----------------

def _check_fixed(oracle, group, name, got, exp, window):
    """equal as points, zeros included; the nonzero ones (at least half) bit for
    bit after batch_normalization; a pure small-order base also against the integers"""
    assert _o(oracle, group, "eq")(got, exp).all(), (name, window)
    nz = _nonzero(group, exp)
    assert nz.sum() >= N // 2 and not nz.all()
    norm = _o(oracle, group, "batch_normalization")
    np.testing.assert_array_equal(norm(np.ascontiguousarray(got[nz])), norm(np.ascontiguousarray(exp[nz])))
    if name not in TORSION_OF:
        m = C.ORDERS[name]
        want = C.aff_rows(group, [C.multiples(group, name)[C.wnaf_value(v, window) % m] for v in C.scalar_ints(m)])
        np.testing.assert_array_equal(_o(oracle, group, "into_affine")(got), want)


@pytest.mark.gpu
@pytest.mark.parametrize("name", G1_BASES)
def test_g1_fixed_base_entries_on_small_order_bases(gpu, oracle, name):
    """plain table + multiply, GLV table + multiply (its membership flag sends
    these bases wherever phi(P) == -[x^2] P decides) and the fused entry at the
    default window, 4 and 16"""
    import torch
    import pairing_amd.device as pdev
    from test_bench_sizes import _dev, _host
    s = C.scalars(_order(name))
    base_np = C.jac(1, C.point(1, name), C.z_of(1, 5))[None]
    wd = _default_window(oracle, 1, N)
    exp = {w: oracle.g1_wnaf_fixed_base(base_np, s, NT, window=w) for w in G1_WINDOWS}
    b, sc = _dev(base_np), _dev(s)
    table, ws = pdev.fixed_base_buffers("cuda:0")
    outs = {k: pdev.empty_records(N, 18, "cuda:0") for k in ("plain", "glv") + G1_WINDOWS}
    table2, _ = pdev.g1_fixed_base_table(b)
    pdev.g1_fixed_base_mul(table2, sc, outs["plain"])
    pdev.g1_fixed_base_glv_table(b, table, ws)
    pdev.g1_fixed_base_glv_mul(b, table, ws, sc, outs["glv"])
    torch.cuda.synchronize()
    for w in G1_WINDOWS:
        pdev.g1_wnaf_fixed_base(b, sc, outs[w], table, ws, window=w)
        torch.cuda.synchronize()
    for k, out in outs.items():
        w = None if k in ("plain", "glv") else k
        _check_fixed(oracle, 1, name, _host(out), exp[w], w or wd)
        got_dev = out.clone()
        pdev.g1_batch_normalization(got_dev)
        torch.cuda.synchronize()
        nz = _nonzero(1, exp[w])
        np.testing.assert_array_equal(_host(got_dev)[nz], oracle.g1_batch_normalization(exp[w])[nz])
    # the host entry
    np.testing.assert_array_equal(gpu.g1_wnaf_fixed_base(base_np, s), _host(outs[None]))


@pytest.mark.gpu
@pytest.mark.parametrize("name", G2_BASES)
def test_g2_fixed_base_on_small_order_bases(gpu, oracle, name):
    s = C.scalars(_order(name))
    base = C.jac(2, C.point(2, name), C.z_of(2, 6))[None]
    wd = _default_window(oracle, 2, N)
    for w in G2_WINDOWS:
        got = gpu.g2_wnaf_fixed_base(base, s, window=w)
        exp = oracle.g2_wnaf_fixed_base(base, s, NT, window=w)
        _check_fixed(oracle, 2, name, got, exp, w or wd)
        nz = _nonzero(2, exp)
        np.testing.assert_array_equal(gpu.g2_batch_normalization(got)[nz], oracle.g2_batch_normalization(exp)[nz])


# ---------------- GPU: the verifying key ----------------

IC_DLOG = (0x1d2c3b4a59687766554433221100ffeeddccbbaa99887766554433221100f0e1 % R_ORDER, 0x7a5b)


def _small_order_ic(oracle):
    """ic = [S, O3, S', O11, O33] with S, S' the IC_DLOG multiples of the generator"""
    sub = oracle.g1_mul_generator(small_scalars(list(IC_DLOG)))
    return np.ascontiguousarray(np.stack([sub[0], C.aff(1, C.point(1, "O3")), sub[1], C.aff(1, C.point(1, "O11")),
                                          C.aff(1, C.point(1, "O33"))]))


@pytest.mark.gpu
def test_input_sum_over_small_order_ic(gpu, oracle):
    from test_groth16_verify import _check_sum
    g = rng(9700)
    ic = _small_order_ic(oracle)
    inputs = [[v] * 4 for v in (0, 1, 2, 3, 11, 33, R_ORDER - 1)] + [G.rand_fr(g, 4) for _ in range(6)]
    inputs += [[3, 5, 11, 33], [1, 7, 22, 66], [R_ORDER - 3, 0, R_ORDER - 11, R_ORDER - 33]]
    want = _check_sum(gpu, oracle, ic, inputs)
    # the reference sum, from the integers: x_1 O3 and x_3 O11 + x_4 O33 are looked up, the G1 part is a generator multiple
    for row, x in zip(want, inputs):
        sub = oracle.g1_mul_generator(small_scalars([(IC_DLOG[0] + x[1] * IC_DLOG[1]) % R_ORDER]))[0]
        P = None if sub[12] else (unmont(sub[0:6]), unmont(sub[6:12]))
        for name, k in (("O3", x[0]), ("O11", x[2]), ("O33", x[3])):
            P = D._ec_add(C.F1, P, C.multiples(1, name)[k % C.ORDERS[name]])
        np.testing.assert_array_equal(row, C.aff(1, P))


@pytest.mark.gpu
def test_verify_over_a_key_with_small_order_ic(gpu, oracle):
    """k = 3 proofs over such a key.  The torsion part of the input sum pairs to
    one, so a proof that satisfies a b = alpha beta + acc gamma + c delta on the
    G1 part of acc verifies; the second proof is that one with another input,
    the third has another C"""
    g = rng(9710)
    alpha, beta, gamma, delta, a, b = G.rand_fr(g, 6)
    ic = _small_order_ic(oracle)
    gen1 = lambda v: oracle.g1_mul_generator(small_scalars(v))     # noqa: E731
    gen2 = lambda v: oracle.g2_mul_generator(small_scalars(v))     # noqa: E731
    vk = V.VkPoints(gen1([alpha]), gen2([beta]), gen2([gamma]), gen2([delta]), ic)
    x = [3, G.rand_fr(g, 1)[0], 11, 34]
    acc = (IC_DLOG[0] + x[1] * IC_DLOG[1]) % R_ORDER
    c = (a * b - alpha * beta - acc * gamma) * pow(delta, -1, R_ORDER) % R_ORDER
    proofs = V.proof_rows(oracle, [a, a, a], [b, b, b], [c, c, (c + 1) % R_ORDER])
    inputs = [x, [x[0], (x[1] + 1) % R_ORDER, x[2], x[3]], x]
    gt, valid = V.ref_verify(oracle, vk, proofs, inputs)
    assert valid.tolist() == [True, False, False]
    flat = [v for row in inputs for v in row]
    from test_groth16_verify import rows_of
    with gpu.groth16_vk(*vk.args()) as h:
        got_valid, got_gt = gpu.groth16_verify(h, proofs, rows_of(flat), return_gt=True)
        np.testing.assert_array_equal(got_valid, valid)
        np.testing.assert_array_equal(got_gt, gt)
        np.testing.assert_array_equal(gpu.groth16_verify(h, proofs, small_scalars(flat), montgomery=False), valid)


# ---------------- GPU: per-item scalar multiplication ----------------

@pytest.mark.gpu
@pytest.mark.parametrize("group,name", [(1, n) for n in G1_BASES] + [(2, n) for n in G2_BASES])
def test_scalar_mul_bit_exact_on_small_order_bases(gpu, oracle, group, name):
    s = C.scalars(_order(name))
    P = C.point(group, name)
    p = np.ascontiguousarray(np.repeat(C.aff(group, P)[None], N, axis=0))
    pj = C.jac_rows(group, [P] * N, z0=10)
    got = getattr(gpu, "g%d_affine_mul" % group)(p, s)
    np.testing.assert_array_equal(got, _o(oracle, group, "affine_mul")(p, s, NT))
    got_j = getattr(gpu, "g%d_mul_assign" % group)(pj, s)
    np.testing.assert_array_equal(got_j, _o(oracle, group, "mul")(pj, s))
    if name not in TORSION_OF:
        m = C.ORDERS[name]
        want = C.aff_rows(group, [C.multiples(group, name)[v % m] for v in C.scalar_ints(m)])
        np.testing.assert_array_equal(_o(oracle, group, "into_affine")(got), want)
        np.testing.assert_array_equal(_o(oracle, group, "into_affine")(got_j), want)
        assert (~_nonzero(group, got)).sum() >= 9


# ---------------- GPU: the group law over all pairs ----------------

@pytest.mark.gpu
@pytest.mark.parametrize("group,name", [(1, "O3"), (1, "O11"), (2, "O13")])
def test_group_law_on_all_pairs_of_a_small_group(gpu, oracle, group, name):
    """(k T, j T) for all k, j < m in Jacobian forms with different z (zero:
    z = 0 under nonzero x, y): add, add_mixed, sub, double, eq, into_affine bit
    for bit with the oracle, and as points (k +- j) T on the integers"""
    from test_group import _neg_rows_nonzero
    m = C.ORDERS[name]
    mult = C.multiples(group, name)
    ks, js = np.divmod(np.arange(m * m), m)
    a = C.jac_rows(group, [mult[k] for k in ks], z0=100)
    b = C.jac_rows(group, [mult[j] for j in js], z0=100 + m * m)
    b_aff = C.aff_rows(group, [mult[j] for j in js])
    fw = 6 if group == 1 else 12
    Gp = lambda op: getattr(gpu, "g%d_%s" % (group, op))       # noqa: E731
    O = lambda op: _o(oracle, group, op)                       # noqa: E731
    res = {}
    for op, args, want in (("add", (a, b), O("add")(a, b)), ("add_mixed", (a, b_aff), O("add_mixed")(a, b_aff)),
                           ("sub", (a, b), O("add")(a, _neg_rows_nonzero(b, fw))), ("double", (a,), O("double")(a)),
                           ("into_affine", (a,), O("into_affine")(a))):
        res[op] = Gp(op)(*args)
        np.testing.assert_array_equal(res[op], want, err_msg=op)
    eq = Gp("eq")(a, b)
    np.testing.assert_array_equal(eq, O("eq")(a, b))
    np.testing.assert_array_equal(eq, ks == js)
    rows = lambda idx: C.aff_rows(group, [mult[i] for i in idx])   # noqa: E731
    into = O("into_affine")
    np.testing.assert_array_equal(into(res["add"]), rows((ks + js) % m))
    np.testing.assert_array_equal(into(res["add_mixed"]), rows((ks + js) % m))
    np.testing.assert_array_equal(into(res["sub"]), rows((ks - js) % m))
    np.testing.assert_array_equal(into(res["double"]), rows(2 * ks % m))
    np.testing.assert_array_equal(res["into_affine"], rows(ks))
    # the GPU's own into_affine on its own sums
    np.testing.assert_array_equal(Gp("into_affine")(res["add"]), rows((ks + js) % m))


# ---------------- GPU: MSM ----------------

def _msm_case(oracle, group, name, n, mixed, seed):
    """(bases (n | n + 8, 13 | 25), scalars (3, n | n + 8, 4), the multipliers
    k_i): n bases k_i T with k_i != 0 mod m; `mixed` puts eight subgroup points
    among them, at random places"""
    g = rng(seed)
    m = C.ORDERS[name]
    mult = C.multiples(group, name)
    ks = [int(k) for k in g.integers(1, m, size=n)]
    bases = C.aff_rows(group, [mult[k] for k in ks])
    if mixed:
        sub = _o(oracle, group, "mul_generator")(random_scalars(g, 8))
        order = g.permutation(n + 8)
        bases = np.ascontiguousarray(np.concatenate([bases, sub])[order])
        n += 8
    s = random_scalars(g, 3 * n, bits=256).reshape(3, n, 4)
    edge = small_scalars([0, 1, m, m - 1, R_ORDER - 1, (1 << 256) - 1, 1 << 255, R_ORDER])
    s[0, :min(n, 8)] = edge[:min(n, 8)]
    if n >= 64:
        s[1, 20:40] = s[1, 20]               # crowded buckets: equal digits over a small group
        s[2, :, 1:] = 0                      # 64-bit scalars: the upper windows are empty
    return bases, ks, np.ascontiguousarray(s)


@pytest.mark.gpu
@pytest.mark.parametrize("mixed", [False, True], ids=["torsion", "mixed"])
@pytest.mark.parametrize("n", [1, 5, 64, 300])
@pytest.mark.parametrize("group,name", [(1, "O3"), (1, "O11"), (2, "O13")])
def test_multiexp_entries_on_small_order_bases(gpu, oracle, group, name, n, mixed):
    """every base in <T>: each bucket, chunk, segment and window sum lives in a
    group of m elements, so the accumulation doubles, cancels and restarts all
    the time; the plain entry, the prepared one and the batch entry with k = 3
    against the oracle as points and, for pure torsion, against
    (sum s_i k_i mod m) T on the integers"""
    bases, ks, s = _msm_case(oracle, group, name, n, mixed, 9800 + 10 * n + group)
    n = bases.shape[0]
    m, mult = C.ORDERS[name], C.multiples(group, name)
    eq, into, ref = _o(oracle, group, "eq"), _o(oracle, group, "into_affine"), _o(oracle, group, "multiexp")
    exp = [ref(bases, s[j], NT) for j in range(3)]
    plain = getattr(gpu, "g%d_multiexp" % group)
    with getattr(gpu, "g%d_msm_prepare" % group)(bases) as prep:
        assert prep.len == n and not prep.in_subgroup
        one = getattr(gpu, "g%d_multiexp_prepared" % group)
        got = {"plain": [plain(bases, s[j]) for j in range(3)], "prepared": [one(prep, s[j]) for j in range(3)],
               "batch": list(getattr(gpu, "g%d_multiexp_prepared_batch" % group)(prep, s)[:, None, :])}
    for entry, rows in got.items():
        for j in range(3):
            assert eq(rows[j], exp[j]).all(), (entry, j)
            if not mixed:
                tot = sum(k * sum(int(x) << (64 * i) for i, x in enumerate(r)) for k, r in zip(ks, s[j])) % m
                np.testing.assert_array_equal(into(np.ascontiguousarray(rows[j]))[0], C.aff(group, mult[tot]),
                                              err_msg="%s %d" % (entry, j))
