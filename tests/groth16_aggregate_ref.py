"""CPU reference of the Groth16 aggregate check (no device, nothing from the code
under test).  For k proofs (A_j, B_j, C_j), inputs x_{j,i}, weights z_j and a key:

    s_0 = sum_j z_j mod r,   s_{i+1} = sum_j z_j x_{j,i} mod r
    A'_j = into_affine(z_j A_j)
    accS = into_affine(s_0 ic[0] + sum_i s_{i+1} ic[i+1])
    CS = into_affine(sum_j z_j C_j),   alphaS = into_affine(s_0 alpha)
    gt = prod_j e(A'_j, B_j) e(accS, -gamma) e(CS, -delta) e(alphaS, -beta),  valid = gt == one

The weight sums are Python integers; the points are the oracle's CurveAffine::mul,
add_assign and into_affine; gt is the Fq12 product of the oracle's pairings (the
final exponentiation is a homomorphism, so it equals the final exponentiation
of the product of the Miller values wherever that is not None)."""
import numpy as np

from groth16_verify_ref import negate_g2
from helpers import R_ORDER, fq12_one, set_infinity, small_scalars

MASK64 = (1 << 64) - 1
# the weights every test mixes in: zero, one, the word boundary, the top bit and the top window's carry
Z_EDGES = [0, 1, (1 << 64) - 1, 1 << 64, 1 << 127, (1 << 128) - 1]


def z_rows(z):
    """(k, 2) uint64 little-endian rows of 128-bit integers"""
    assert all(0 <= v < 1 << 128 for v in z)
    return np.array([[v & MASK64, v >> 64] for v in z], np.uint64).reshape(len(z), 2)


def rand_z(gen, n):
    return [int(gen.integers(0, 1 << 63)) | (int(gen.integers(0, 1 << 63)) << 63) | (int(gen.integers(0, 4)) << 126)
            for _ in range(n)]


def g1_zero(oracle):
    return oracle.g1_from_affine(set_infinity(np.zeros((1, 13), np.uint64), [0]))


def sum_rows(oracle, jac):
    """(1, 18): the sum of (n, 18) Jacobian rows, pairwise; zero for none"""
    if jac.shape[0] == 0:
        return g1_zero(oracle)
    while jac.shape[0] > 1:
        half = jac.shape[0] // 2
        head = oracle.g1_add(np.ascontiguousarray(jac[:half]), np.ascontiguousarray(jac[half:2 * half]))
        jac = np.concatenate([head, jac[2 * half:]])
    return np.ascontiguousarray(jac)


def weight_sums(inputs, z, l):
    """[s_0, .., s_l] as integers mod r; inputs: k lists of l integers (any 256-bit value)"""
    return [sum(z) % R_ORDER] + [sum(zj * x[i] for zj, x in zip(z, inputs)) % R_ORDER for i in range(l)]


def ref_points(oracle, vk, proofs, inputs, z):
    """(k + 3, 13) affine records A'_0 .. A'_{k-1} | accS | CS | alphaS"""
    k, l = proofs.shape[0], vk.n_inputs
    assert len(z) == k and len(inputs) == k
    s = weight_sums(inputs, z, l)
    zs = small_scalars(z)
    scaled = oracle.g1_affine_mul(np.ascontiguousarray(proofs[:, :13]), zs) if k else np.zeros((0, 18), np.uint64)
    acc = sum_rows(oracle, oracle.g1_affine_mul(np.ascontiguousarray(vk.ic), small_scalars(s)))
    csum = sum_rows(oracle, oracle.g1_affine_mul(np.ascontiguousarray(proofs[:, 38:51]), zs)) if k else g1_zero(oracle)
    asum = oracle.g1_affine_mul(np.ascontiguousarray(vk.alpha_g1), small_scalars(s[:1]))
    return oracle.g1_into_affine(np.ascontiguousarray(np.concatenate([scaled, acc, csum, asum])))


def q_array(vk, proofs):
    """(k + 3, 25): B_0 .. | -gamma | -delta | -beta"""
    return np.ascontiguousarray(np.concatenate([proofs[:, 13:38], negate_g2(vk.gamma_g2), negate_g2(vk.delta_g2),
                                                negate_g2(vk.beta_g2)]))


def fq12_product(oracle, rows):
    """(1, 72): the product of (n, 72) Fq12 rows, n >= 1, pairwise"""
    while rows.shape[0] > 1:
        half = rows.shape[0] // 2
        head = oracle.fq12_mul(np.ascontiguousarray(rows[:half]), np.ascontiguousarray(rows[half:2 * half]))
        rows = np.concatenate([head, rows[2 * half:]])
    return np.ascontiguousarray(rows)


def ref_aggregate(oracle, vk, proofs, inputs, z, nthreads=8):
    """(gt (1, 72), valid) of the aggregate check; k = 0 gives (one, True)"""
    if proofs.shape[0] == 0:
        return fq12_one(), True
    p = ref_points(oracle, vk, proofs, inputs, z)
    gt = fq12_product(oracle, oracle.pairing(p, q_array(vk, proofs), nthreads))
    return gt, bool((gt == fq12_one()).all())


def fq12_pow_int(oracle, a, e):
    """a^e for a (1, 72) row and a non-negative integer below 2^256"""
    return oracle.fq12_pow(a, small_scalars([e]))
