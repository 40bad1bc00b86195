"""CPU references of the R1CS product and the Groth16 prover (no device, nothing
from the code under test): matrices and witnesses as Python integers mod r,
points as known multiples of the generators, so a proof is three
g{1,2}_mul_generator calls of the oracle.

A system here is `mats` = (A, B, C), each a list of n_rows rows, each row a list
of (column, coefficient) pairs with integer coefficients in [0, r)."""
import numpy as np

from helpers import R_ORDER, rng, small_scalars
from test_fr import fr_val
from test_fr_ntt import GEN, mont_rows, omega
from test_fr_ntt_quotient import ref_quotient

W_PROOF = 51


def rand_fr(gen, n):
    return [int.from_bytes(gen.bytes(32), "little") % R_ORDER for _ in range(n)]


def csr(rows):
    """(row_ptr, col, val) of one matrix: uint64, uint32 and Montgomery (nnz, 4) rows"""
    row_ptr = np.zeros(len(rows) + 1, np.uint64)
    cols, vals = [], []
    for i, row in enumerate(rows):
        for c, v in row:
            cols.append(c)
            vals.append(v)
        row_ptr[i + 1] = len(cols)
    val = mont_rows(vals) if vals else np.zeros((0, 4), np.uint64)
    return row_ptr, np.array(cols, np.uint32), val


def eval_ints(mats, witnesses, log_n):
    """[A, B, C] -> per matrix the k * n integers sum_t val[t] w_j[col[t]], zero from n_rows on"""
    n = 1 << log_n
    out = []
    for rows in mats:
        assert len(rows) <= n
        vals = []
        for w in witnesses:
            vals += [sum(v * w[c] for c, v in row) % R_ORDER for row in rows] + [0] * (n - len(rows))
        out.append(vals)
    return out


def ref_eval(mats, witnesses, log_n):
    """the three (k * n, 4) Montgomery arrays pa_r1cs_eval must write"""
    n = 1 << log_n
    return tuple(mont_rows(v) if v else np.zeros((0, 4), np.uint64) for v in eval_ints(mats, witnesses, log_n)) \
        if witnesses and n else tuple(np.zeros((0, 4), np.uint64) for _ in range(3))


def random_system(seed, n_rows, n_cols, terms=3):
    """a random sparse system of about `terms` terms per row (no relation between A, B and C)"""
    g = rng(seed)
    mats = []
    for _ in range(3):
        rows = []
        for _ in range(n_rows):
            t = int(g.integers(0, terms + 1))
            rows.append([(int(g.integers(0, n_cols)), v) for v in rand_fr(g, t)] if n_cols else [])
        mats.append(rows)
    return mats


def satisfied_system(seed, n_rows, n_cols):
    """(mats, w): A, B and w random with w_0 = 1, each row of C one term on a variable with w != 0 such that
    (A w)_i (B w)_i = (C w)_i"""
    g = rng(seed)
    w = [1] + [x or 1 for x in rand_fr(g, n_cols - 1)]
    a, b, _ = random_system(seed + 1, n_rows, n_cols)
    c = []
    for ra, rb in zip(a, b):
        va = sum(v * w[col] for col, v in ra) % R_ORDER
        vb = sum(v * w[col] for col, v in rb) % R_ORDER
        col = int(g.integers(0, n_cols))
        c.append([(col, va * vb * pow(w[col], -1, R_ORDER) % R_ORDER)])
    return (a, b, c), w


class Key:
    """a proving key whose every point is a known multiple of its generator:
    alpha, beta, delta integers, a, b, l, h lists of integers (b serves both b_g1_query and b_g2_query)"""

    def __init__(self, alpha, beta, delta, a, b, l, h, n_public, log_n):
        self.alpha, self.beta, self.delta = alpha, beta, delta
        self.a, self.b, self.l, self.h = a, b, l, h
        self.n_vars, self.n_public, self.log_n = len(a), n_public, log_n
        assert len(b) == len(a) and len(l) == len(a) - n_public and len(h) <= 1 << log_n

    def points(self, oracle, nthreads=8):
        """the arguments of pairing_amd.groth16_pk, in its order"""
        g1 = lambda v: oracle.g1_mul_generator(small_scalars(v), nthreads) if v else np.zeros((0, 13), np.uint64)
        g2 = lambda v: oracle.g2_mul_generator(small_scalars(v), nthreads) if v else np.zeros((0, 25), np.uint64)
        return (g1([self.alpha]), g1([self.beta]), g1([self.delta]), g2([self.beta]), g2([self.delta]),
                g1(self.a), g1(self.b), g2(self.b), g1(self.l), g1(self.h), self.n_public, self.log_n)


def random_key(seed, n_vars, n_public, log_n, h_len):
    g = rng(seed)
    al, be, de = rand_fr(g, 3)
    return Key(al, be, de, rand_fr(g, n_vars), rand_fr(g, n_vars), rand_fr(g, n_vars - n_public), rand_fr(g, h_len),
               n_public, log_n)


def quotient_ints(oracle, mats, witnesses, log_n):
    """per witness the n integers of h = (A B - C) / Z from ref_quotient"""
    n = 1 << log_n
    a, b, c = ref_eval(mats, witnesses, log_n)
    h = [fr_val(x) for x in ref_quotient(oracle, a, b, c, log_n)]
    return [h[j * n:(j + 1) * n] for j in range(len(witnesses))]


def proof_scalars(key, w, h, r, s):
    """the discrete logarithms (a, b, c) of one proof: the four formulas of create_proof on integers mod r;
    h rows from key.h's length on meet no base"""
    dot = lambda x, y: sum(p * q for p, q in zip(x, y)) % R_ORDER
    a = (key.alpha + dot(w, key.a) + r * key.delta) % R_ORDER
    b = (key.beta + dot(w, key.b) + s * key.delta) % R_ORDER
    c = (dot(w[key.n_public:], key.l) + dot(h[:len(key.h)], key.h) + s * a + r * b - r * s * key.delta) % R_ORDER
    return a, b, c


def ref_proofs(oracle, key, mats, witnesses, rs, ss):
    """(k, 51) rows: the affine records of a G, b H, c G for each proof"""
    k = len(witnesses)
    if k == 0:
        return np.zeros((0, W_PROOF), np.uint64)
    hs = quotient_ints(oracle, mats, witnesses, key.log_n)
    sc = [proof_scalars(key, w, h, r, s) for w, h, r, s in zip(witnesses, hs, rs, ss)]
    a = oracle.g1_mul_generator(small_scalars([x[0] for x in sc]))
    b = oracle.g2_mul_generator(small_scalars([x[1] for x in sc]))
    c = oracle.g1_mul_generator(small_scalars([x[2] for x in sc]))
    return np.concatenate([a, b, c], axis=1)


def real_setup(seed, mats, n_vars, n_public, log_n):
    """(Key, gamma, ic): a Groth16 setup from a tiny trapdoor (tau, alpha, beta, gamma, delta) over the domain of
    2^log_n points, as bellman's generate_parameters computes it: with u_i, v_i, w_i the column polynomials of A, B, C
    at tau (Lagrange basis), a_query[i] = u_i, b_query[i] = v_i, ic[i] = (beta u_i + alpha v_i + w_i) / gamma for
    public i, l_query the same over delta for the rest, h_query[i] = tau^i (tau^n - 1) / delta for i < n - 1"""
    g = rng(seed)
    tau, alpha, beta, gamma, delta = (x or 1 for x in rand_fr(g, 5))
    n = 1 << log_n
    w = omega(log_n)
    z = (pow(tau, n, R_ORDER) - 1) % R_ORDER
    assert z
    # L_j(tau) = z w^j / (n (tau - w^j))
    ninv = pow(n, -1, R_ORDER)
    lag = [z * pow(w, j, R_ORDER) * ninv * pow(tau - pow(w, j, R_ORDER), -1, R_ORDER) % R_ORDER for j in range(n)]
    cols = []
    for rows in mats:
        acc = [0] * n_vars
        for j, row in enumerate(rows):
            for c, v in row:
                acc[c] = (acc[c] + v * lag[j]) % R_ORDER
        cols.append(acc)
    u, v, ww = cols
    mix = [(beta * u[i] + alpha * v[i] + ww[i]) % R_ORDER for i in range(n_vars)]
    ginv, dinv = pow(gamma, -1, R_ORDER), pow(delta, -1, R_ORDER)
    ic = [x * ginv % R_ORDER for x in mix[:n_public]]
    l = [x * dinv % R_ORDER for x in mix[n_public:]]
    h = [pow(tau, i, R_ORDER) * z * dinv % R_ORDER for i in range(n - 1)]
    return Key(alpha, beta, delta, u, v, l, h, n_public, log_n), gamma, ic


def verify_pairs(oracle, key, gamma, ic, w_public, proof):
    """(p (4, 13), q (4, 25)): the four pairs whose product is one for a valid proof,
    e(A, B) e(-alpha, beta) e(-sum_i w_i IC_i, gamma) e(-C, delta) = 1"""
    acc = sum(x * y for x, y in zip(w_public, ic)) % R_ORDER
    neg = lambda v: (R_ORDER - v) % R_ORDER
    p = np.concatenate([proof[None, :13], oracle.g1_mul_generator(small_scalars([neg(key.alpha), neg(acc)])),
                        negate_g1(proof[None, 38:51])])
    q = np.concatenate([proof[None, 13:38], oracle.g2_mul_generator(small_scalars([key.beta, gamma, key.delta]))])
    return np.ascontiguousarray(p), np.ascontiguousarray(q)


def negate_g1(aff):
    """-P of (n, 13) affine records, on the canonical integers"""
    from helpers import Q, from_limbs, limbs
    out = aff.copy()
    for row in out:
        if not int(row[12]) & 0xff:
            y = from_limbs(row[6:12])
            row[6:12] = limbs((Q - y) % Q)
    return out


def pairing_product_is_one(oracle, p, q):
    """prod_i e(p_i, q_i) == 1 under the oracle's pairing and fq12_mul"""
    from helpers import fq12_one
    e = oracle.pairing(p, q, 4)
    acc = e[:1]
    for i in range(1, e.shape[0]):
        acc = oracle.fq12_mul(acc, e[i:i + 1])
    return bool((acc == fq12_one()).all())


__all__ = [name for name in dir() if not name.startswith("_")]
assert GEN == 7
