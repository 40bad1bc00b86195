"""The Groth16 prover on degenerate keys, sums and blinding scalars
(tests/groth16_degenerate_cases.py).

tests/test_groth16.py proves over dense random keys, where every key point
and every intermediate sum is a generic point.  A real key is full of points at
infinity, and the assembly kernel is a chain of group operations of which each
has exceptional branches: 0 + P, P + 0, P + P, P + (-P), and an infinity result
written as an affine record.  Here every one of them is reached on purpose.

Part A keeps the key inside G1/G2, so the reference is groth16_ref's: discrete
logarithms mod r and three generator multiplications of the oracle.  Zeros and
collisions are chosen on those integers and asserted there before the device
runs.  Part B puts alpha, beta and the queries on bases of small order, outside
the subgroups; the reference is then the header's four formulas on affine
Python integers, and a census in integers mod m shows which branches the
kernel's double-and-add chains and C additions meet.

Every comparison is bit for bit on the (k, 51) proof rows."""
import os

import numpy as np
import pytest

import groth16_aggregate_ref as A
import groth16_degenerate_cases as X
import groth16_ref as G
import groth16_verify_ref as V
import small_order_cases as C
from helpers import R_ORDER, rng, small_scalars
from test_groth16 import Case, flat, rows_of

R = R_ORDER
ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
PURE = [pair for pair in X.TORSION_KEYS if pair[0] not in X.TORSION_OF]


def _infinity(rows, width):
    return (rows[:, width - 1] & 0xff).astype(bool)


# ---------------- CPU: the inputs are what they claim to be ----------------

def test_oracle_zero_multiple_is_the_infinity_record_of_into_affine(oracle):
    for group, gen, into, width in ((1, oracle.g1_mul_generator, oracle.g1_into_affine, 13),
                                    (2, oracle.g2_mul_generator, oracle.g2_into_affine, 25)):
        zero = gen(small_scalars([0, 5, 0]))
        np.testing.assert_array_equal(zero[0], C.aff(group, None))
        np.testing.assert_array_equal(zero[2], C.aff(group, None))
        assert _infinity(zero, width).tolist() == [True, False, True]
        # into_affine of a Jacobian zero, whatever its x and y
        jz = C.jac(group, None, C.z_of(group, 1))[None]
        np.testing.assert_array_equal(into(jz)[0], C.aff(group, None))
        # r G = 0 as well
        np.testing.assert_array_equal(gen(small_scalars([R]))[0], C.aff(group, None))


@pytest.mark.parametrize("name", list(X.sparse_cases()))
def test_sparse_keys_hold_the_stated_zeros(oracle, name):
    key, mats, n_rows, ws, want = X.sparse_cases()[name]
    got = X.zeros(key)
    for query, count in want.items():
        assert got[query] == count and len(getattr(key, query)) >= count, (name, query)
    if name == "scattered":
        for query in "ablh":
            vals = getattr(key, query)
            assert vals[0] == 0 and vals[-1] == 0 and any(vals)
    assert len(mats[0]) == n_rows <= 1 << key.log_n
    tag = "tiny" if key.log_n else "one_point_%d" % n_rows
    hs = [X.quotient(oracle, mats, w, key.log_n, tag) for w in ws]
    q = [X.quantities(key, w, h, 5, 7) for w, h in zip(ws, hs)]
    # the sums that a whole zero query, or none at all, makes the zero point handed to the assembly
    for query, attr in (("a", "S_a"), ("b", "S_b"), ("l", "S_l"), ("h", "S_h")):
        vals = getattr(key, query)
        if not any(vals):
            assert all(getattr(x, attr) == 0 for x in q), (name, query)
    if key.log_n:
        # the witnesses: one satisfies (no top quotient row), one does not
        assert hs[0][-1] == 0 and hs[1][-1] != 0 and any(hs[0])


def test_large_sparse_key_is_two_thirds_infinity():
    key, mats, n_rows, ws = X.large_case()
    for query, count in X.zeros(key).items():
        vals = getattr(key, query)
        assert 0.55 * len(vals) < count < 0.78 * len(vals) and vals[0] == 0 and vals[-1] == 0, query
    assert key.n_vars == 300 and key.log_n == 9 and len(key.h) == 511 and n_rows == 400


def test_alpha_beta_delta_keys_hold_the_stated_zeros():
    want = {"alpha": (True, False, False), "beta": (False, True, False), "delta": (False, False, True),
            "alpha_beta_delta": (True, True, True)}
    for name, key in X.abd_cases().items():
        assert (key.alpha == 0, key.beta == 0, key.delta == 0) == want[name]
        assert all(key.a) and all(key.b) and all(key.l) and all(key.h)


@pytest.mark.parametrize("cid", X.COLLISION_IDS)
def test_collision_case_meets_its_equality_on_the_integers(oracle, cid):
    key, w, r, s, q = X.collision(oracle, cid)       # asserts the equality the case is named for
    g = X.generic_key()
    changed = [n for n in ("alpha", "beta", "delta", "a", "b", "l", "h") if getattr(key, n) != getattr(g, n)]
    free = X.free_number(cid)
    assert changed == ([] if free in "rs" else [free])
    assert (cid in X.SHARED_IDS) == (key is g)
    if free in "abl":
        assert sum(x != y for x, y in zip(getattr(key, free), getattr(g, free))) == 1
    # exactly the proof points the id promises are the point at infinity
    assert [n for n in "ABC" if getattr(q, n) == 0] == ([X.INFINITY_IDS[cid]] if cid in X.INFINITY_IDS else [])


def test_boundary_scalars_cover_every_lane_boundary():
    pairs = X.boundary_scalars()
    rs, ss = [p[0] for p in pairs], [p[1] for p in pairs]
    prod = [r * s % R for r, s in pairs]
    for i in X.BOUNDARY_BITS:
        for vals in (rs, ss, prod):
            assert 1 << i in vals, i
    assert X.BOUNDARY_BITS == (0, 3, 4, 7, 8, 31, 32, 127, 128, 251, 252, 253, 254)
    # the table has 255 rows: the last lane of wave 0 holds bits 252..254, of each half of wave 1 bits 248..254
    for vals in (rs, ss, prod):
        assert any(v >> 252 == 7 for v in vals) and any(v >> 248 == 0x73 for v in vals) and R - 1 in vals
    assert (1, 1) in pairs and (0, 0) in pairs and any(p == 1 and r > 1 for p, (r, _) in zip(prod, pairs))
    assert len(pairs) <= 96


def test_realistic_key_has_infinity_where_a_variable_does_not_occur(oracle):
    mats, w = X.occurrence_system()
    key, gamma, ic = G.real_setup(6061, mats, X.NV, X.NPUB, X.LOGN)
    zero = lambda vals: [i for i, v in enumerate(vals) if v == 0]   # noqa: E731
    assert zero(key.a) == [X.ONLY_B, X.ONLY_C, X.NOWHERE]
    assert zero(key.b) == [X.ONLY_A, X.ONLY_C, X.NOWHERE]
    assert zero(key.l) == [X.NOWHERE - X.NPUB] and not zero(key.h) and len(key.h) == X.N - 1
    a, b, c = G.eval_ints(mats, [w], X.LOGN)
    assert all(x * y % R == z for x, y, z in zip(a, b, c)) and any(c)


# ---- Part B ----

def test_integer_reference_agrees_with_the_discrete_log_reference(oracle):
    """int_proof on multiples of the generators against groth16_ref.ref_proofs: ties the integer formulas, the
    integer generators and C.aff's records to the reference every other prover test uses"""
    mats, w, other = X.tiny()
    g = rng(6200)
    pick = lambda n: [int(v) for v in g.choice([0, 1, 2, 5], size=n)]   # noqa: E731
    b = pick(X.NV)
    mult = dict(alpha=3, beta1=7, beta2=7, a=pick(X.NV), b1=b, b2=b, l=pick(X.NV - X.NPUB), h=pick(X.N))
    d, r, s = G.rand_fr(g, 3)
    pkey = X.PointKey(X.G1_GEN, X.G2_GEN, mult, d, X.NPUB, X.LOGN)
    key = G.Key(3, 7, d, mult["a"], b, mult["l"], mult["h"], X.NPUB, X.LOGN)
    for got, want in zip(pkey.points()[:10], key.points(oracle)[:10]):
        np.testing.assert_array_equal(got, want)
    h = X.quotient(oracle, mats, other, X.LOGN, "tiny")
    for rr, ss in ((r, s), (0, 0)):
        row = X.proof_row(X.int_proof(pkey, other, h, rr, ss))
        np.testing.assert_array_equal(row, G.ref_proofs(oracle, key, mats, [other], [rr], [ss])[0])


def _torsion_inputs(oracle, g1, g2):
    key, r, s = X.torsion_key(g1, g2)
    mats = X.tiny()[0]
    ws = X.torsion_witnesses(g1, g2)
    hs = [X.quotient(oracle, mats, w, X.LOGN, "tiny") for w in ws]
    return key, mats, ws, hs, X.blindings(r, s)


@pytest.mark.parametrize("g1,g2", X.TORSION_KEYS)
def test_small_order_keys_are_multiples_of_their_bases_zero_among_them(g1, g2):
    key, r, s = X.torsion_key(g1, g2)
    assert r and s and key.d
    for group, name, queries in ((1, g1, ("a", "b1", "l", "h")), (2, g2, ("b2",))):
        m = X.order(name)
        for qn in queries:
            ks, pts = key.mult[qn], getattr(key, qn)
            assert 0 in ks and any(k % m for k in ks)
            assert [P is None for P in pts] == [k % m == 0 for k in ks] or name in X.TORSION_OF
            if name not in X.TORSION_OF:
                assert pts == [C.multiples(group, name)[k] for k in ks]
    assert key.alpha is not None and key.beta1 is not None and key.beta2 is not None
    # delta is a subgroup point
    assert X.ec_mul(1, key.delta1, R) is None and key.delta1 is not None


@pytest.mark.parametrize("g1,g2", PURE)
def test_branch_census_of_the_small_order_keys(oracle, g1, g2):
    """a condition on the inputs, not a measurement: on integers mod m, the scalar list and the witnesses
    make the two double-and-add chains and the C additions meet every exceptional branch"""
    key, mats, ws, hs, rss = _torsion_inputs(oracle, g1, g2)
    chains, c_adds = X.census(key, ws, hs, rss)
    for what, cnt in (("chains", chains), ("C", c_adds)):
        for branch in ("0+P", "P+0", "P+P", "P+(-P)", "infinity"):
            assert cnt[branch] > 0, (g1, what, branch, cnt)
    # the G2 side: with s = 0, B = beta_g2 + S_b2 stays in <T>, and is the point at infinity for the last witness
    m2 = X.order(g2)
    tot = [(key.mult["beta2"] + sum(x * k for x, k in zip(w, key.mult["b2"]))) % m2 for w in ws]
    assert tot[-1] == 0 and any(tot[:-1])


def test_census_counts_on_known_chains():
    cnt = X.new_count()
    assert X.chain_census(1, 3, 3, cnt) == 0          # 1, then 2 + 1 = 0
    assert (cnt["P+(-P)"], cnt["infinity"], cnt["P+P"], cnt["0+P"]) == (1, 1, 0, 0)
    cnt = X.new_count()
    assert X.chain_census(1, 0b1011, 3, cnt) == 2     # 1; 2; 4 + 1 = 2 (P + P); 4 + 1 = 2 (P + P)
    assert (cnt["P+P"], cnt["P+(-P)"]) == (2, 0)
    cnt = X.new_count()
    assert X.chain_census(1, 0b1101, 3, cnt) == 1     # 1; 2 + 1 = 0; 0; 0 + 1 (a restart)
    assert (cnt["P+(-P)"], cnt["0+P"]) == (1, 1)
    cnt = X.new_count()
    assert X.chain_census(0, 5, 3, cnt) == 0 and cnt["P+0"] == 2 and cnt["infinity"] == 2


def test_delta_of_small_order_breaks_the_identity_the_kernel_uses():
    """C's s A + r B1 - (rs) delta equals s A0 + r B0 + (rs) delta, rs reduced mod r, only when r delta = 0:
    for delta = O11 the header's expression is s A0 + r B0 + (2 r s - (rs mod r)) delta.  The header therefore
    leaves delta outside G1/G2 undefined for the prover."""
    d11 = C.point(1, "O11")
    A0, B0 = C.multiples(1, "O11")[3], C.multiples(1, "O11")[7]
    g = rng(6300)
    differ = 0
    for _ in range(4):
        r, s = G.rand_fr(g, 2)
        rs = r * s % R
        header_mult, kernel_mult = (2 * r * s - rs) % 11, rs % 11
        a = X.ec_add(1, A0, X.ec_mul(1, d11, r))
        b1 = X.ec_add(1, B0, X.ec_mul(1, d11, s))
        header = X.ec_add(1, X.ec_add(1, X.ec_mul(1, a, s), X.ec_mul(1, b1, r)), C.ec_neg(1, X.ec_mul(1, d11, rs)))
        shared = X.ec_add(1, X.ec_mul(1, A0, s), X.ec_mul(1, B0, r))
        kernel = X.ec_add(1, shared, X.ec_mul(1, d11, rs))
        assert header == X.ec_add(1, shared, C.multiples(1, "O11")[header_mult])
        assert (header == kernel) == (header_mult == kernel_mult)
        differ += header != kernel
        # on a subgroup point the two agree
        dg = X.ec_mul(1, X.G1_GEN, 12345)
        a, b1 = X.ec_mul(1, dg, r), X.ec_mul(1, dg, s)
        assert X.ec_add(1, X.ec_add(1, X.ec_mul(1, a, s), X.ec_mul(1, b1, r)), C.ec_neg(1, X.ec_mul(1, dg, rs))) \
            == X.ec_mul(1, dg, rs)
    assert differ >= 3
    for path in ("include/pairing_amd.h", "INTEGRATION.md"):
        with open(os.path.join(ROOT, path)) as f:
            text = " ".join(f.read().split())
        assert "outside G1/G2 are undefined for the prover" in text.replace(" * ", " "), path


# ---------------- GPU ----------------

def _blind(seed, k):
    g = rng(seed)
    return G.rand_fr(g, k), G.rand_fr(g, k)


def _check_part_a(gpu, oracle, key, mats, n_rows, calls):
    """prove each (witnesses, rs, ss) of `calls` over one key object; bit for bit against ref_proofs"""
    c = Case(gpu, oracle, key, mats, n_rows)
    try:
        assert c.pk.in_subgroup          # infinity passes membership: the GLV multiexp path
        assert (c.pk.n_vars, c.pk.n_public, c.pk.h_len, c.pk.log_n) == (key.n_vars, key.n_public, len(key.h), key.log_n)
        return [c.check(ws, rs, ss) for ws, rs, ss in calls]
    finally:
        c.close()


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(X.sparse_cases()))
def test_sparse_key(gpu, oracle, name):
    key, mats, n_rows, ws, want = X.sparse_cases()[name]
    assert all(X.zeros(key)[query] == count for query, count in want.items())
    rs, ss = _blind(6400, 4)
    three, one, plain = _check_part_a(gpu, oracle, key, mats, n_rows,
                                      [(ws, rs[:3], ss[:3]), (ws[1:2], rs[3:], ss[3:]), (ws[:2], [0, 0], [0, 0])])
    assert not (three[0] == three[2]).all()          # the same witness under other blinding scalars
    if name == "a_zero":                             # r = s = 0: A is alpha itself
        np.testing.assert_array_equal(plain[0, :13], key.points(oracle)[0][0])


@pytest.mark.gpu
def test_large_sparse_key(gpu, oracle):
    key, mats, n_rows, ws = X.large_case()
    assert all(2 * count > len(getattr(key, query)) for query, count in X.zeros(key).items())
    rs, ss = _blind(6410, 4)
    _check_part_a(gpu, oracle, key, mats, n_rows, [([ws[0], ws[1], ws[0]], rs[:3], ss[:3]), (ws[1:], rs[3:], ss[3:])])


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(X.abd_cases()))
def test_alpha_beta_delta_at_infinity(gpu, oracle, name):
    key = X.abd_cases()[name]
    mats, w, other = X.tiny()
    rs, ss = _blind(6420, 3)
    got, _ = _check_part_a(gpu, oracle, key, mats, X.NROWS,
                           [([w, other, w], rs, ss), ([w, other], [0, R - 1], [R - 1, 0])])
    assert not _infinity(got[:, :13], 13).any()


@pytest.fixture(scope="module")
def shared_collisions(gpu, oracle):
    """the cases whose free number is r or s: the generic key, one batched call"""
    cases = [X.collision(oracle, cid) for cid in X.SHARED_IDS]
    key, mats = X.generic_key(), X.tiny()[0]
    assert all(c[0] is key for c in cases)
    ws, rs, ss = [c[1] for c in cases], [c[2] for c in cases], [c[3] for c in cases]
    c = Case(gpu, oracle, key, mats, X.NROWS)
    try:
        assert c.pk.in_subgroup
        got = gpu.groth16_prove(c.pk, c.sysm, c.dom, flat(ws), rows_of(rs), rows_of(ss))
    finally:
        c.close()
    return got, G.ref_proofs(oracle, key, mats, ws, rs, ss)


@pytest.mark.gpu
@pytest.mark.parametrize("cid", X.COLLISION_IDS)
def test_collision_in_the_assembly(gpu, oracle, shared_collisions, cid):
    key, w, r, s, q = X.collision(oracle, cid)
    mats = X.tiny()[0]
    if cid in X.SHARED_IDS:
        i = X.SHARED_IDS.index(cid)
        got, want = shared_collisions[0][i], shared_collisions[1][i]
        np.testing.assert_array_equal(got, want, err_msg=cid)
    else:
        got = _check_part_a(gpu, oracle, key, mats, X.NROWS, [([w], [r], [s])])[0][0]
    inf = [bool(got[12] & 0xff), bool(got[37] & 0xff), bool(got[50] & 0xff)]
    assert inf == [q.A == 0, q.B == 0, q.C == 0], cid
    assert any(inf) == (cid in X.INFINITY_IDS)


@pytest.mark.gpu
def test_blinding_scalars_at_the_lane_boundaries(gpu, oracle):
    pairs = X.boundary_scalars()
    mats, w, other = X.tiny()
    ws = [w if i % 2 else other for i in range(len(pairs))]
    _check_part_a(gpu, oracle, X.generic_key(), mats, X.NROWS, [(ws, [p[0] for p in pairs], [p[1] for p in pairs])])


@pytest.mark.gpu
def test_realistic_key_round_trip(gpu, oracle):
    """prove over a setup whose key has infinity points where bellman's has them, then verify: each proof on
    the device, the batch in one aggregate check, and each on the oracle's pairing"""
    mats, w = X.occurrence_system()
    key, gamma, ic = G.real_setup(6061, mats, X.NV, X.NPUB, X.LOGN)
    spoiled, unused = list(w), list(w)
    spoiled[X.ONLY_A] = (spoiled[X.ONLY_A] + 1) % R
    unused[X.NOWHERE] = (unused[X.NOWHERE] + 1) % R       # a variable that occurs nowhere changes nothing
    rs, ss = _blind(6430, 3)
    rs[2], ss[2] = rs[0], ss[0]
    proofs, = _check_part_a(gpu, oracle, key, mats, X.NROWS, [([w, spoiled, unused], rs, ss)])
    np.testing.assert_array_equal(proofs[2], proofs[0])
    want = [True, False, True]
    vkp = V.real_vk(oracle, key, gamma, ic)
    inputs = [w[1:X.NPUB]] * 3
    ref_gt, ref_valid = V.ref_verify(oracle, vkp, proofs, inputs)
    assert ref_valid.tolist() == want
    for pr, ok in zip(proofs, want):
        assert G.pairing_product_is_one(oracle, *G.verify_pairs(oracle, key, gamma, ic, w[:X.NPUB], pr)) == ok
    z = A.rand_z(rng(6431), 3)
    x = rows_of([v for row in inputs for v in row])
    with gpu.groth16_vk(*vkp.args()) as vk:
        valid, gt = gpu.groth16_verify(vk, proofs, x, return_gt=True)
        np.testing.assert_array_equal(valid, ref_valid)
        np.testing.assert_array_equal(gt, ref_gt)
        for rows, zz, xs, ok in ((proofs, z, x, False), (proofs[::2], z[::2], x[::2], True)):
            agg_gt, agg_valid = A.ref_aggregate(oracle, vkp, rows, inputs[:len(zz)], zz)
            got_valid, got_gt = gpu.groth16_verify_aggregate(vk, rows, xs, A.z_rows(zz), return_gt=True)
            assert got_valid is agg_valid is ok
            np.testing.assert_array_equal(got_gt, agg_gt)


@pytest.mark.gpu
def test_proofs_with_a_point_at_infinity_through_the_verifier(gpu, oracle):
    """the Part A proofs whose A, B or C is the point at infinity (the reference rows, which the device's
    equal), and a generic one, under a key with their alpha, beta and delta: valid and gt as the reference"""
    mats = X.tiny()[0]
    rows = []
    for cid, which in X.INFINITY_IDS.items():
        key, w, r, s, q = X.collision(oracle, cid)
        rows.append(G.ref_proofs(oracle, key, mats, [w], [r], [s])[0])
        assert bool(rows[-1][{"A": 12, "B": 37, "C": 50}[which]] & 0xff)
    k = X.generic_key()
    w = X.tiny()[1]
    rows.append(G.ref_proofs(oracle, k, mats, [w], [X.COLLISION_R], [X.COLLISION_S])[0])
    proofs = np.ascontiguousarray(np.stack(rows))
    assert [_infinity(proofs[:, :lo + wd], lo + wd).tolist() for lo, wd in ((0, 13), (13, 25), (38, 13))] == \
        [[True, False, False, False], [False, True, False, False], [False, False, True, False]]
    g = rng(6440)
    gamma, ic0, ic1 = G.rand_fr(g, 3)
    vkp = V.vk_from_ints(oracle, k.alpha, k.beta, gamma, k.delta, [ic0, ic1])
    inputs = [G.rand_fr(g, 1) for _ in range(4)]
    ref_gt, ref_valid = V.ref_verify(oracle, vkp, proofs, inputs)
    with gpu.groth16_vk(*vkp.args()) as vk:
        valid, gt = gpu.groth16_verify(vk, proofs, rows_of([v for row in inputs for v in row]), return_gt=True)
    np.testing.assert_array_equal(valid, ref_valid)
    np.testing.assert_array_equal(gt, ref_gt)
    assert not valid.any()


@pytest.mark.gpu
@pytest.mark.parametrize("g1,g2", X.TORSION_KEYS)
def test_key_on_small_order_bases(gpu, oracle, g1, g2):
    """alpha, beta and every query point a multiple of a base outside the subgroups (the 257-bit multiexp
    path), delta in them; r, s in {0, random}^2 for every witness, one call; against the integer reference"""
    key, mats, ws, hs, rss = _torsion_inputs(oracle, g1, g2)
    batch = [(w, h, r, s) for w, h in zip(ws, hs) for r, s in rss]
    ref = [X.int_proof(key, *item) for item in batch]
    want = np.stack([X.proof_row(p) for p in ref])
    c = Case(gpu, oracle, key, mats, X.NROWS, points=key.points())
    try:
        assert not c.pk.in_subgroup
        got = gpu.groth16_prove(c.pk, c.sysm, c.dom, flat([b[0] for b in batch]), rows_of([b[2] for b in batch]),
                                rows_of([b[3] for b in batch]))
    finally:
        c.close()
    np.testing.assert_array_equal(got, want)
    if g2 not in X.TORSION_OF:
        # s = 0 keeps B in <T>: the last witness gives B at infinity, with r zero and not
        b_inf = [p[1] is None for p in ref]
        assert b_inf[-4] and b_inf[-2] and not b_inf[-1] and not b_inf[-3]
        mult = C.multiples(2, g2)
        assert all(p[1] in mult for p, item in zip(ref, batch) if item[3] == 0)
    if g1 not in X.TORSION_OF:
        # r = s = 0: the whole proof stays in groups of m elements
        mult = C.multiples(1, g1)
        assert all(p[0] in mult and p[2] in mult for p, item in zip(ref, batch) if item[2] == 0 and item[3] == 0)
