"""CPU references of the Groth16 verifier (no device, nothing from the code under
test): the public-input sum from the oracle's CurveAffine::mul, add_assign and
into_affine, the verdict from the oracle's pairing and Fq12 product, and the
192-byte wire form of a proof from decode_cases' encoders.

A verifying key here is a `VkPoints`: the affine records the library takes."""
import numpy as np

import decode_cases as D
import groth16_ref as G
from helpers import Q, from_limbs, limbs, small_scalars, unmont

ENCODED_PROOF_BYTES = 192


class VkPoints:
    """alpha_g1 (1, 13), beta_g2, gamma_g2, delta_g2 (1, 25), ic (n_public, 13) affine records"""

    def __init__(self, alpha_g1, beta_g2, gamma_g2, delta_g2, ic):
        self.alpha_g1, self.beta_g2, self.gamma_g2, self.delta_g2, self.ic = alpha_g1, beta_g2, gamma_g2, delta_g2, ic
        self.n_public = ic.shape[0]
        self.n_inputs = self.n_public - 1

    def args(self):
        """the arguments of pairing_amd.groth16_vk, in its order"""
        return self.alpha_g1, self.beta_g2, self.gamma_g2, self.delta_g2, self.ic


def vk_from_ints(oracle, alpha, beta, gamma, delta, ic):
    """the key whose points are these multiples of the generators"""
    g1 = lambda v: oracle.g1_mul_generator(small_scalars(v))   # noqa: E731
    g2 = lambda v: oracle.g2_mul_generator(small_scalars(v))   # noqa: E731
    return VkPoints(g1([alpha]), g2([beta]), g2([gamma]), g2([delta]), g1(list(ic)))


def real_vk(oracle, key, gamma, ic):
    """the verifying key of groth16_ref.real_setup's (key, gamma, ic)"""
    return vk_from_ints(oracle, key.alpha, key.beta, gamma, key.delta, ic)


def negate_g2(aff):
    """-Q of (n, 25) affine records, on the canonical integers"""
    out = aff.copy()
    for row in out:
        if not int(row[24]) & 0xff:
            for lo in (12, 18):
                y = from_limbs(row[lo:lo + 6])
                row[lo:lo + 6] = limbs((Q - y) % Q)
    return out


def ref_input_sum(oracle, ic, inputs):
    """(k, 13): into_affine(ic[0] + sum_i x[j][i] * ic[i + 1]) for the k input vectors of `inputs` (lists of
    l = n_public - 1 integers, any 256-bit value), the terms added in index order"""
    k, l = len(inputs), ic.shape[0] - 1
    if k == 0:
        return np.zeros((0, 13), np.uint64)
    acc = oracle.g1_from_affine(np.ascontiguousarray(np.repeat(ic[:1], k, axis=0)))
    for i in range(l):
        base = np.ascontiguousarray(np.repeat(ic[i + 1:i + 2], k, axis=0))
        term = oracle.g1_affine_mul(base, small_scalars([x[i] for x in inputs]))
        acc = oracle.g1_add(acc, term)
    return oracle.g1_into_affine(acc)


def ref_verify(oracle, vk, proofs, inputs, nthreads=8):
    """(gt (k, 72), valid (k,) bool) of verify_proof for (k, 51) proof rows: gt = e(A, B) e(acc, -gamma)
    e(C, -delta), valid = gt == e(alpha, beta)"""
    k = proofs.shape[0]
    if k == 0:
        return np.zeros((0, 72), np.uint64), np.zeros(0, bool)
    acc = ref_input_sum(oracle, vk.ic, inputs)
    p = np.ascontiguousarray(np.concatenate([proofs[:, :13], acc, proofs[:, 38:51]]))
    q = np.ascontiguousarray(np.concatenate([proofs[:, 13:38], np.repeat(negate_g2(vk.gamma_g2), k, axis=0),
                                             np.repeat(negate_g2(vk.delta_g2), k, axis=0)]))
    e = oracle.pairing(p, q, nthreads)
    gt = oracle.fq12_mul(oracle.fq12_mul(e[:k], e[k:2 * k]), e[2 * k:])
    want = oracle.pairing(vk.alpha_g1, vk.beta_g2)
    return gt, (gt == want).all(axis=1)


def proof_rows(oracle, a, b, c):
    """(n, 51) proofs a_i G, b_i H, c_i G from integers"""
    return np.ascontiguousarray(np.concatenate([oracle.g1_mul_generator(small_scalars(a)),
                                                oracle.g2_mul_generator(small_scalars(b)),
                                                oracle.g1_mul_generator(small_scalars(c))], axis=1))


# ---- the wire form: A (48), B (96), C (48) compressed, bellman's Proof::write ----
def _enc_g1(rec):
    if int(rec[12]) & 0xff:
        return D.zero_enc(48, True)
    x, y = unmont(rec[0:6]), unmont(rec[6:12])
    return D.enc_g1(x, y, True, greatest=y > (Q - y) % Q)


def _enc_g2(rec):
    if int(rec[24]) & 0xff:
        return D.zero_enc(96, True)
    x = (unmont(rec[0:6]), unmont(rec[6:12]))
    y = (unmont(rec[12:18]), unmont(rec[18:24]))
    ny = ((Q - y[0]) % Q, (Q - y[1]) % Q)
    return D.enc_g2(x, y, True, greatest=(y[1], y[0]) > (ny[1], ny[0]))


def encode_proofs(proofs):
    """(k, 192) uint8: the compressed records of (k, 51) proof rows whose points are on their curves"""
    out = b"".join(_enc_g1(r[:13]) + _enc_g2(r[13:38]) + _enc_g1(r[38:51]) for r in proofs)
    return np.frombuffer(out, np.uint8).reshape(-1, ENCODED_PROOF_BYTES).copy()


def decode_status(oracle, data):
    """(k, 3) uint8: the oracle's checked, compressed decode status of A, B and C of each record"""
    data = np.ascontiguousarray(data, np.uint8)
    a = oracle.decode(1, np.ascontiguousarray(data[:, :48]), True, True)[1]
    b = oracle.decode(2, np.ascontiguousarray(data[:, 48:144]), True, True)[1]
    c = oracle.decode(1, np.ascontiguousarray(data[:, 144:]), True, True)[1]
    return np.stack([a, b, c], axis=1)


__all__ = [name for name in dir() if not name.startswith("_")]
assert G.W_PROOF == 51
