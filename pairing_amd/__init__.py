"""pairing_amd -- MI355X-native batched BLS12-381 engine.

The batched counterpart of the Rust crate `pairing` v0.14.2 hot path
(dignifiedquire/pairing): Fq Montgomery multiply, the Fq2/Fq6/Fq12 tower,
G2 line precomputation (`G2Prepared`), `miller_loop` and
`final_exponentiation`, all as hand-written HIP kernels for gfx950 behind
the C ABI of include/pairing_amd.h.

Two layers:
  * batch functions over numpy arrays in the ABI layout (this module), e.g.
    `pairing(p, q)` for n independent pairs;
  * include/pairing_amd.hpp: the C++ mirror of the reference's trait surface
    (`Bls12::pairing`, `Bls12::miller_loop`, `G1Affine::prepare`,
    `G1Compressed::into_affine`, `Wnaf`, ...) over the same C ABI.
Device-resident entry points for torch tensors live in `pairing_amd.device`.
"""
import numpy as np

from ._native import (W_FQ, W_FQ2, W_FQ6, W_FQ12, W_FR, W_G1A, W_G1, W_G2A, W_G2, W_G2P, NTT_MAX_LOG_N, FrNttDomain, G1MsmBases, G2MsmBases,
                      FrCsr, Groth16Key, Groth16Pk, Groth16VKey, Groth16Vk, GROTH16_VK_MAX_INPUTS, GROTH16_ENCODED_PROOF_BYTES,
                      R1cs, R1CS_CHUNK_LEN, W_PROOF, Groth16Circuit, Groth16Params, trapdoor_rows,
                      PairingError, _lib, as_rows, batch_shape, call, csr_offsets, device_count, msm_bases, msm_scalars, ntt_mode, ptr, set_decode_kernel, set_device, set_pairing_kernel, version)

__all__ = [
    "PairingError", "version", "device_count", "set_device", "set_pairing_kernel", "set_decode_kernel",
    "fq_mul", "fq_square", "fq_add", "fq_sub", "fq_inverse", "fq_from_repr", "fq_into_repr",
    "fq2_mul", "fq2_square", "fq6_mul", "fq12_mul", "fq12_square", "fq12_inverse",
    "fq12_frobenius_map", "fq12_cyclotomic_square", "fq12_mul_by_014",
    "fq2_inverse", "fq2_frobenius_map", "fq6_square", "fq6_inverse", "fq6_frobenius_map", "fq_pow", "fq12_pow",
    "g1_batch_normalization", "g1_wnaf_fixed_base",
    "g2_prepare", "miller_loop_batch", "miller_loop_shared_prepared", "multi_miller_loop", "final_exponentiation", "pairing",
    "multi_miller_loop_affine", "multi_pairing", "multi_pairing_batch", "pairing_multi_gpu",
    "fq_sqrt", "fq2_sqrt", "g1_decode", "g2_decode", "g1_encode", "g2_encode", "DECODE_STATUS",
    "g1_subgroup_check", "g2_subgroup_check",
    "fr_mul", "fr_square", "fr_add", "fr_sub", "fr_double", "fr_negate", "fr_inverse",
    "fr_from_repr", "fr_into_repr", "fr_pow", "fr_legendre", "fr_sqrt",
    "g1_affine_mul", "g2_affine_mul", "g1_mul_assign", "g2_mul_assign", "g1_multiexp", "g2_multiexp",
    "G1MsmBases", "g1_msm_prepare", "g1_multiexp_prepared", "g1_multiexp_prepared_batch",
    "G2MsmBases", "g2_msm_prepare", "g2_multiexp_prepared", "g2_multiexp_prepared_batch",
    "FrNttDomain", "fr_ntt_domain", "fr_ntt", "fr_ntt_quotient",
    "R1cs", "r1cs", "r1cs_eval", "R1CS_CHUNK_LEN", "Groth16Pk", "groth16_pk", "groth16_prove",
    "Groth16Vk", "groth16_vk", "groth16_verify", "groth16_verify_encoded", "groth16_input_sum",
    "groth16_verify_aggregate", "groth16_verify_aggregate_encoded", "groth16_aggregate_points", "g1_multiexp_u128",
    "Groth16Circuit", "Groth16Params", "groth16_circuit", "groth16_generate", "groth16_generate_scalars",
    "g1_eq", "g2_eq", "g1_double", "g2_double", "g1_add", "g2_add", "g1_add_mixed", "g2_add_mixed", "g1_negate", "g2_negate",
    "g1_sub", "g2_sub", "g1_into_affine", "g2_into_affine", "g1_into_projective", "g2_into_projective",
    "g2_batch_normalization", "g2_wnaf_fixed_base",
    "g1_wnaf_fixed_base_exact", "g2_wnaf_fixed_base_exact", "g1_wnaf_fixed_scalar_exact", "g2_wnaf_fixed_scalar_exact",
    "g1_recommended_wnaf_for_scalar", "g2_recommended_wnaf_for_scalar",
    "g1_recommended_wnaf_for_num_scalars", "g2_recommended_wnaf_for_num_scalars",
]


def _binary(name, a, b, width):
    a = as_rows(a, width, "a")
    b = as_rows(b, width, "b")
    if a.shape != b.shape:
        raise ValueError("operand shapes differ: %s vs %s" % (a.shape, b.shape))
    out = np.empty_like(a)
    call(name, ptr(a), ptr(b), ptr(out), a.shape[0])
    return out


def _unary(name, a, width):
    a = as_rows(a, width, "a")
    out = np.empty_like(a)
    call(name, ptr(a), ptr(out), a.shape[0])
    return out


def _inverse(name, a, width):
    a = as_rows(a, width, "a")
    out = np.empty_like(a)
    ok = np.zeros(a.shape[0], np.uint8)
    call(name, ptr(a), ptr(out), ptr(ok), a.shape[0])
    return out, ok.astype(bool)


# ---- Fq: src/bls12_381/fq.rs ----
def fq_mul(a, b):
    """Fq::mul_assign (fq.rs:909-960) elementwise."""
    return _binary("pa_fq_mul_batch", a, b, W_FQ)


def fq_square(a):
    """Fq::square (fq.rs:962-1016)."""
    return _unary("pa_fq_square_batch", a, W_FQ)


def fq_add(a, b):
    return _binary("pa_fq_add_batch", a, b, W_FQ)


def fq_sub(a, b):
    return _binary("pa_fq_sub_batch", a, b, W_FQ)


def fq_inverse(a):
    """Fq::inverse (fq.rs:849-902): (values, ok) with ok False where the reference returns None."""
    return _inverse("pa_fq_inverse_batch", a, W_FQ)


def fq_from_repr(repr_rows):
    """PrimeField::from_repr (fq.rs:747-756): (values, ok), ok False = Err(NotInField) (repr >= q)."""
    r = as_rows(repr_rows, W_FQ, "repr")
    out = np.empty_like(r)
    ok = np.zeros(r.shape[0], np.uint8)
    call("pa_fq_from_repr_batch", ptr(r), ptr(out), ptr(ok), r.shape[0])
    return out, ok.astype(bool)


def fq_into_repr(a):
    """PrimeField::into_repr (fq.rs:758-775): canonical FqRepr rows."""
    return _unary("pa_fq_into_repr_batch", a, W_FQ)


# ---- tower ----
def fq2_mul(a, b):
    return _binary("pa_fq2_mul_batch", a, b, W_FQ2)


def fq2_square(a):
    return _unary("pa_fq2_square_batch", a, W_FQ2)


def fq6_mul(a, b):
    return _binary("pa_fq6_mul_batch", a, b, W_FQ6)


def fq12_mul(a, b):
    return _binary("pa_fq12_mul_batch", a, b, W_FQ12)


def fq12_square(a):
    return _unary("pa_fq12_square_batch", a, W_FQ12)


def fq12_cyclotomic_square(a):
    """Granger-Scott squaring; equals fq12_square for elements of the cyclotomic subgroup."""
    return _unary("pa_fq12_cyclotomic_square_batch", a, W_FQ12)


def fq12_inverse(a):
    return _inverse("pa_fq12_inverse_batch", a, W_FQ12)


def fq2_inverse(a):
    """Fq2::inverse (fq2.rs:138-155): (values, ok)."""
    return _inverse("pa_fq2_inverse_batch", a, W_FQ2)


def fq2_frobenius_map(a, power):
    """Fq2::frobenius_map (fq2.rs:157-159)."""
    return _frob("pa_fq2_frobenius_map_batch", a, W_FQ2, power)


def fq6_square(a):
    """Fq6::square (fq6.rs:166-197)."""
    return _unary("pa_fq6_square_batch", a, W_FQ6)


def fq6_inverse(a):
    """Fq6::inverse (fq6.rs:250-301): (values, ok)."""
    return _inverse("pa_fq6_inverse_batch", a, W_FQ6)


def fq6_frobenius_map(a, power):
    """Fq6::frobenius_map (fq6.rs:157-164)."""
    return _frob("pa_fq6_frobenius_map_batch", a, W_FQ6, power)


def _frob(name, a, width, power):
    a = as_rows(a, width, "a")
    out = np.empty_like(a)
    call(name, ptr(a), ptr(out), a.shape[0], int(power))
    return out


def _pow(name, a, width, exp_limbs):
    a = as_rows(a, width, "a")
    e = np.ascontiguousarray(np.asarray(exp_limbs, dtype=np.uint64).reshape(-1))
    out = np.empty_like(a)
    call(name, ptr(a), ptr(e), e.size, ptr(out), a.shape[0])
    return out


def fq_pow(a, exp_limbs):
    """Field::pow (lib.rs:306-324) for Fq, one exponent (u64 LE limbs) for every element."""
    return _pow("pa_fq_pow_batch", a, W_FQ, exp_limbs)


def fq12_pow(a, exp_limbs):
    """Field::pow (lib.rs:306-324) for Fq12."""
    return _pow("pa_fq12_pow_batch", a, W_FQ12, exp_limbs)


def fq12_frobenius_map(a, power):
    a = as_rows(a, W_FQ12, "a")
    out = np.empty_like(a)
    call("pa_fq12_frobenius_map_batch", ptr(a), ptr(out), a.shape[0], int(power))
    return out


def fq12_mul_by_014(a, c0, c1, c4):
    """Fq12::mul_by_014 (fq12.rs:34-48)."""
    a = as_rows(a, W_FQ12, "a")
    c0, c1, c4 = (as_rows(c, W_FQ2, "c") for c in (c0, c1, c4))
    out = np.empty_like(a)
    call("pa_fq12_mul_by_014_batch", ptr(a), ptr(c0), ptr(c1), ptr(c4), ptr(out), a.shape[0])
    return out


# ---- engine: src/bls12_381/mod.rs ----
def g2_prepare(q):
    """G2Prepared::from_affine (mod.rs:168-358) for each G2 affine point."""
    q = as_rows(q, W_G2A, "q")
    out = np.empty((q.shape[0], W_G2P), np.uint64)
    call("pa_g2_prepare_batch", ptr(q), ptr(out), q.shape[0])
    return out


def miller_loop_batch(p, q_prepared):
    """out[i] = Bls12::miller_loop([(p[i], q[i])]) -- n independent loops."""
    p = as_rows(p, W_G1A, "p")
    q = as_rows(q_prepared, W_G2P, "q_prepared")
    if p.shape[0] != q.shape[0]:
        raise ValueError("p and q_prepared lengths differ")
    out = np.empty((p.shape[0], W_FQ12), np.uint64)
    call("pa_miller_loop_batch", ptr(p), ptr(q), ptr(out), p.shape[0])
    return out


def miller_loop_shared_prepared(p, q_prepared):
    """out[i] = Bls12::miller_loop([(p[i], q)]) for ONE prepared q shared by every
    p[i] (lib.rs:88-96 called with the same &G2Prepared; mod.rs:40-102): the
    verifier's fixed-key shape.  q_prepared: one record, shape (W_G2P,) or (1, W_G2P)."""
    p = as_rows(p, W_G1A, "p")
    q = as_rows(q_prepared, W_G2P, "q_prepared")
    if q.shape[0] != 1:
        raise ValueError("q_prepared must be ONE G2Prepared record")
    out = np.empty((p.shape[0], W_FQ12), np.uint64)
    call("pa_miller_loop_shared_prepared", ptr(p), p.shape[0], ptr(q), ptr(out))
    return out


def multi_miller_loop(p, q_prepared):
    """Engine::miller_loop over all pairs: the product (mod.rs:40-102)."""
    p = as_rows(p, W_G1A, "p") if len(p) else np.zeros((0, W_G1A), np.uint64)
    q = as_rows(q_prepared, W_G2P, "q_prepared") if len(q_prepared) else np.zeros((0, W_G2P), np.uint64)
    if p.shape[0] != q.shape[0]:
        raise ValueError("p and q_prepared lengths differ")
    out = np.empty((1, W_FQ12), np.uint64)
    call("pa_multi_miller_loop", ptr(p), ptr(q), p.shape[0], ptr(out))
    return out[0]


def final_exponentiation(f):
    """Engine::final_exponentiation (mod.rs:104-160): (values, ok); ok False iff f == 0."""
    f = as_rows(f, W_FQ12, "f")
    out = np.empty_like(f)
    ok = np.zeros(f.shape[0], np.uint8)
    call("pa_final_exponentiation_batch", ptr(f), ptr(out), ptr(ok), f.shape[0])
    return out, ok.astype(bool)


def pairing(p, q, out=None):
    """Engine::pairing (lib.rs:101-109) for n independent (G1Affine, G2Affine) pairs.
    `out`: an optional (n, 72) uint64 C-contiguous array to write into -- a caller
    that reuses it saves the first-touch page faults of a fresh 37.7 MB result
    per 2^16 pairs (tools/pcie_rate.py measures both)."""
    p = as_rows(p, W_G1A, "p")
    q = as_rows(q, W_G2A, "q")
    if p.shape[0] != q.shape[0]:
        raise ValueError("p and q lengths differ")
    if out is None:
        out = np.empty((p.shape[0], W_FQ12), np.uint64)
    elif (not isinstance(out, np.ndarray) or out.dtype != np.uint64 or out.shape != (p.shape[0], W_FQ12)
          or not out.flags.c_contiguous or not out.flags.writeable):
        raise ValueError("out must be a writeable C-contiguous (%d, %d) uint64 array" % (p.shape[0], W_FQ12))
    call("pa_pairing_batch", ptr(p), ptr(q), ptr(out), p.shape[0])
    return out


# ---- G1 parameter-generation path (config 3) ----
def g1_batch_normalization(v):
    """CurveProjective::batch_normalization (ec.rs:246-294); returns the normalized copy."""
    v = as_rows(v, W_G1, "v").copy()
    call("pa_g1_batch_normalization", ptr(v), v.shape[0])
    return v


def g1_wnaf_fixed_base(base, scalars, window=None):
    """Wnaf::new().base(base, n).scalar(s) for each FrRepr scalar (wnaf.rs:93-107,
    169-178): Jacobian points equal to the reference's wNAF products -- s_i *
    base, or (s_i - 2^256) * base where its wnaf_form wraps (wnaf.rs:30-35).
    `window`: the table's window (default recommended_wnaf_for_num_scalars(n))."""
    b = as_rows(base, W_G1, "base")
    s = as_rows(scalars, 4, "scalars")
    out = np.empty((s.shape[0], W_G1), np.uint64)
    if window is None:
        call("pa_g1_wnaf_fixed_base", ptr(b), ptr(s), s.shape[0], ptr(out))
    else:
        call("pa_g1_wnaf_fixed_base_window", ptr(b), ptr(s), s.shape[0], int(window), ptr(out))
    return out


def _wnaf_exact(group, fixed_scalar, bases, scalars, window):
    wj = W_G1 if group == 1 else W_G2
    b = as_rows(bases, wj, "base" if not fixed_scalar else "bases")
    s = as_rows(scalars, 4, "scalar" if fixed_scalar else "scalars")
    # the fixed operand is ONE record (Wnaf::base(g, ..) / Wnaf::scalar(s)); a
    # second row would be ignored silently, so refuse it
    if fixed_scalar and s.shape[0] != 1:
        raise ValueError("scalar: expected exactly one record, got %d" % s.shape[0])
    if not fixed_scalar and b.shape[0] != 1:
        raise ValueError("base: expected exactly one record, got %d" % b.shape[0])
    n = b.shape[0] if fixed_scalar else s.shape[0]
    out = np.empty((n, wj), np.uint64)
    w = 0 if window is None else int(window)
    if fixed_scalar:
        call("pa_g%d_wnaf_fixed_scalar_exact" % group, ptr(b), n, ptr(s), w, ptr(out))
    else:
        call("pa_g%d_wnaf_fixed_base_exact" % group, ptr(b), ptr(s), n, w, ptr(out))
    return out


def g1_wnaf_fixed_base_exact(base, scalars, window=None):
    """Wnaf::new().base(base, n).scalar(s_i) with the reference's exact table chain,
    wnaf_form and wnaf_exp (wnaf.rs:1-179): Jacobian words bit-identical to the
    reference's.  `window`: 1..20 (default recommended_wnaf_for_num_scalars(n))."""
    return _wnaf_exact(1, False, base, scalars, window)


def g2_wnaf_fixed_base_exact(base, scalars, window=None):
    """G2 form of g1_wnaf_fixed_base_exact."""
    return _wnaf_exact(2, False, base, scalars, window)


def g1_wnaf_fixed_scalar_exact(bases, scalar, window=None):
    """Wnaf::new().scalar(s).base(g_i) (wnaf.rs:111-128, 156-166) for every Jacobian
    base, bit-identical Jacobian words.  `window`: 1..12 (default
    recommended_wnaf_for_scalar(s))."""
    return _wnaf_exact(1, True, bases, scalar, window)


def g2_wnaf_fixed_scalar_exact(bases, scalar, window=None):
    """G2 form of g1_wnaf_fixed_scalar_exact."""
    return _wnaf_exact(2, True, bases, scalar, window)


# ---- multi-pairing (SURVEY.md §8 f rank 2) and in-process multi-device ----
def _pairs(p, q):
    p = as_rows(p, W_G1A, "p") if len(p) else np.zeros((0, W_G1A), np.uint64)
    q = as_rows(q, W_G2A, "q") if len(q) else np.zeros((0, W_G2A), np.uint64)
    if p.shape[0] != q.shape[0]:
        raise ValueError("p and q lengths differ")
    return p, q


def multi_miller_loop_affine(p, q):
    """Engine::miller_loop over (G1Affine, G2Affine) pairs, prepare fused on device:
    the product of the per-pair loops (mod.rs:40-102)."""
    p, q = _pairs(p, q)
    out = np.empty((1, W_FQ12), np.uint64)
    call("pa_multi_miller_loop_affine", ptr(p), ptr(q), p.shape[0], ptr(out))
    return out[0]


def multi_pairing(p, q):
    """final_exponentiation(miller_loop(pairs)) -- the batch-verification product
    e(P_1,Q_1)...e(P_n,Q_n); returns (Fq12, ok)."""
    p, q = _pairs(p, q)
    out = np.empty((1, W_FQ12), np.uint64)
    ok = np.zeros(1, np.uint8)
    call("pa_multi_pairing", ptr(p), ptr(q), p.shape[0], ptr(out), ptr(ok))
    return out[0], bool(ok[0])


def multi_pairing_batch(p, q, offsets=None, pairs_per_product=None, want_values=True):
    """m independent multi_pairing products in one call -- a batch of signature or
    proof checks.  Product j covers pairs offsets[j] .. offsets[j+1] (CSR: m + 1
    entries from 0 to n, non-decreasing); or give pairs_per_product = k for m = n / k
    products of k pairs each.  Returns (out, ok, is_one): out (m, 72) as multi_pairing
    gives for each segment, or None with want_values=False (then only the flags
    come back from the device); ok and is_one (m,) bool, is_one[j] = ok[j] and
    out[j] == one."""
    p, q = _pairs(p, q)
    n = p.shape[0]
    if (offsets is None) == (pairs_per_product is None):
        raise ValueError("give exactly one of offsets and pairs_per_product")
    if pairs_per_product is not None:
        k = int(pairs_per_product)
        if k < 1 or n % k:
            raise ValueError("%d pairs do not split into products of %d" % (n, k))
        offsets = np.arange(n // k + 1, dtype=np.uint64) * np.uint64(k)
    o = csr_offsets(offsets, n)
    m = o.shape[0] - 1
    out = np.empty((m, W_FQ12), np.uint64) if want_values else None
    ok = np.zeros(m, np.uint8)
    is_one = np.zeros(m, np.uint8)
    call("pa_multi_pairing_batch", ptr(p), ptr(q), ptr(o), m, ptr(out) if want_values else None, ptr(ok),
         ptr(is_one))
    return out, ok.astype(bool), is_one.astype(bool)


def pairing_multi_gpu(p, q, ndev):
    """pairing(p, q) split over devices 0..ndev-1 of this process."""
    p, q = _pairs(p, q)
    out = np.empty((p.shape[0], W_FQ12), np.uint64)
    call("pa_pairing_batch_multi_gpu", ptr(p), ptr(q), ptr(out), p.shape[0], int(ndev))
    return out


# ---- square roots and point encodings (SURVEY.md §8 f rank 1) ----
# status byte -> GroupDecodingError (lib.rs:469-481)
DECODE_STATUS = {
    0: "Ok", 1: "NotOnCurve", 2: "NotInSubgroup",
    3: "CoordinateDecodingError(x / x.c0)", 4: "CoordinateDecodingError(x.c1)",
    5: "CoordinateDecodingError(y / y.c0)", 6: "CoordinateDecodingError(y.c1)",
    7: "UnexpectedCompressionMode", 8: "UnexpectedInformation",
}
ENCODED_SIZE = {(1, False): 96, (1, True): 48, (2, False): 192, (2, True): 96}


def fq_sqrt(a):
    """SqrtField::sqrt for Fq (fq.rs:1147-1170): (roots, ok); ok False for non-residues."""
    return _inverse("pa_fq_sqrt_batch", a, W_FQ)


def fq2_sqrt(a):
    """SqrtField::sqrt for Fq2 (fq2.rs:167-220): (roots, ok)."""
    return _inverse("pa_fq2_sqrt_batch", a, W_FQ2)


def _decode(group, enc, compressed, checked):
    size = ENCODED_SIZE[(group, bool(compressed))]
    enc = np.ascontiguousarray(np.asarray(enc, dtype=np.uint8))
    if enc.ndim == 1:
        enc = enc.reshape(-1, size)
    if enc.ndim != 2 or enc.shape[1] != size:
        raise ValueError("encodings must have shape (n, %d), got %s" % (size, enc.shape))
    n = enc.shape[0]
    out = np.empty((n, W_G1A if group == 1 else W_G2A), np.uint64)
    status = np.zeros(n, np.uint8)
    call("pa_g%d_decode_batch" % group, ptr(enc), n, int(bool(compressed)), int(bool(checked)), ptr(out),
         ptr(status))
    return out, status


def g1_decode(enc, compressed, checked=True):
    """G1Uncompressed / G1Compressed ::into_affine (checked) or ::into_affine_unchecked
    (ec.rs:662-837) for (n, 96|48) uint8 records: (affine points, status bytes)."""
    return _decode(1, enc, compressed, checked)


def g2_decode(enc, compressed, checked=True):
    """G2Uncompressed / G2Compressed ::into_affine[_unchecked] (ec.rs:1322-1509)."""
    return _decode(2, enc, compressed, checked)


def _subgroup(group, pts):
    pts = as_rows(pts, W_G1A if group == 1 else W_G2A, "points")
    ok = np.zeros(pts.shape[0], np.uint8)
    call("pa_g%d_subgroup_check_batch" % group, ptr(pts), pts.shape[0], ptr(ok))
    return ok.astype(bool)


def g1_subgroup_check(pts):
    """is_in_correct_subgroup_assuming_on_curve (ec.rs:142-144) for (n, 13) affine
    rows: True where r * P == 0 (infinity included); unspecified off the curve."""
    return _subgroup(1, pts)


def g2_subgroup_check(pts):
    """is_in_correct_subgroup_assuming_on_curve for (n, 25) G2 affine rows."""
    return _subgroup(2, pts)


def _encode(group, pts, compressed):
    pts = as_rows(pts, W_G1A if group == 1 else W_G2A, "points")
    size = ENCODED_SIZE[(group, bool(compressed))]
    enc = np.zeros((pts.shape[0], size), np.uint8)
    call("pa_g%d_encode_batch" % group, ptr(pts), pts.shape[0], int(bool(compressed)), ptr(enc))
    return enc


def g1_encode(pts, compressed):
    """EncodedPoint::from_affine for G1 (ec.rs:737-752, 839-867)."""
    return _encode(1, pts, compressed)


def g2_encode(pts, compressed):
    """EncodedPoint::from_affine for G2 (ec.rs:1398-1415, 1510-1539)."""
    return _encode(2, pts, compressed)


# ---- Fr: src/bls12_381/fr.rs (rows (n,4): Montgomery Fr or canonical FrRepr) ----
def fr_mul(a, b):
    """Fr::mul_assign (fr.rs:438-465) elementwise."""
    return _binary("pa_fr_mul_batch", a, b, W_FR)


def fr_square(a):
    """Fr::square (fr.rs:467-500)."""
    return _unary("pa_fr_square_batch", a, W_FR)


def fr_add(a, b):
    """Fr::add_assign (fr.rs:341-348)."""
    return _binary("pa_fr_add_batch", a, b, W_FR)


def fr_sub(a, b):
    """Fr::sub_assign (fr.rs:359-367)."""
    return _binary("pa_fr_sub_batch", a, b, W_FR)


def fr_double(a):
    """Fr::double (fr.rs:350-357)."""
    return _unary("pa_fr_double_batch", a, W_FR)


def fr_negate(a):
    """Fr::negate (fr.rs:369-375)."""
    return _unary("pa_fr_negate_batch", a, W_FR)


def fr_inverse(a):
    """Fr::inverse (fr.rs:377-431): (values, ok), ok False where the reference returns None."""
    return _inverse("pa_fr_inverse_batch", a, W_FR)


def fr_from_repr(repr_rows):
    """PrimeField::from_repr (fr.rs:279-288): (values, ok), ok False = Err(NotInField)."""
    r = as_rows(repr_rows, W_FR, "repr")
    out = np.empty_like(r)
    ok = np.zeros(r.shape[0], np.uint8)
    call("pa_fr_from_repr_batch", ptr(r), ptr(out), ptr(ok), r.shape[0])
    return out, ok.astype(bool)


def fr_into_repr(a):
    """PrimeField::into_repr (fr.rs:290-303): canonical FrRepr rows."""
    return _unary("pa_fr_into_repr_batch", a, W_FR)


def fr_pow(a, exp_limbs):
    """Field::pow (lib.rs:306-324) of every element by one exponent (u64 LE limbs)."""
    a = as_rows(a, W_FR, "a")
    e = np.ascontiguousarray(np.asarray(exp_limbs, dtype=np.uint64).reshape(-1))
    out = np.empty_like(a)
    call("pa_fr_pow_batch", ptr(a), ptr(e), e.size, ptr(out), a.shape[0])
    return out


def fr_legendre(a):
    """SqrtField::legendre (fr.rs:575-590): int8 0 Zero, 1 QuadraticResidue, -1 QuadraticNonResidue."""
    a = as_rows(a, W_FR, "a")
    out = np.zeros(a.shape[0], np.int8)
    call("pa_fr_legendre_batch", ptr(a), ptr(out), a.shape[0])
    return out


def fr_sqrt(a):
    """SqrtField::sqrt (fr.rs:592-646): (roots, ok), ok False where the reference returns None."""
    return _inverse("pa_fr_sqrt_batch", a, W_FR)


# ---- variable-base scalar multiplication and MSM (ec.rs:88-95, 174-177, 534-553) ----
def _scalar_mul(name, p, scalars, in_width, out_width):
    p = as_rows(p, in_width, "points")
    s = as_rows(scalars, 4, "scalars")
    if p.shape[0] != s.shape[0]:
        raise ValueError("points and scalars differ in length: %d vs %d" % (p.shape[0], s.shape[0]))
    out = np.zeros((p.shape[0], out_width), np.uint64)
    call(name, ptr(p), ptr(s), ptr(out), p.shape[0])
    return out


def g1_affine_mul(p, scalars):
    """CurveAffine::mul (ec.rs:174-177): Jacobian s_i * P_i, bit-exact with the reference."""
    return _scalar_mul("pa_g1_affine_mul_batch", p, scalars, W_G1A, W_G1)


def g2_affine_mul(p, scalars):
    return _scalar_mul("pa_g2_affine_mul_batch", p, scalars, W_G2A, W_G2)


def g1_mul_assign(p, scalars):
    """CurveProjective::mul_assign (ec.rs:534-553) on Jacobian points, bit-exact."""
    return _scalar_mul("pa_g1_mul_assign_batch", p, scalars, W_G1, W_G1)


def g2_mul_assign(p, scalars):
    return _scalar_mul("pa_g2_mul_assign_batch", p, scalars, W_G2, W_G2)


def _multiexp(name, bases, scalars, in_width, out_width):
    b = as_rows(bases, in_width, "bases") if len(bases) else np.zeros((0, in_width), np.uint64)
    s = as_rows(scalars, 4, "scalars") if len(scalars) else np.zeros((0, 4), np.uint64)
    if b.shape[0] != s.shape[0]:
        raise ValueError("bases and scalars differ in length: %d vs %d" % (b.shape[0], s.shape[0]))
    out = np.zeros((1, out_width), np.uint64)
    call(name, ptr(b), ptr(s), b.shape[0], ptr(out))
    return out


def g1_multiexp(bases, scalars):
    """sum_i s_i * P_i over G1 affine bases (Pippenger on the device): one Jacobian row,
    equal as a point to the reference's sum of CurveAffine::mul results."""
    return _multiexp("pa_g1_multiexp", bases, scalars, W_G1A, W_G1)


def g2_multiexp(bases, scalars):
    return _multiexp("pa_g2_multiexp", bases, scalars, W_G2A, W_G2)


def g1_multiexp_u128(bases, scalars):
    """sum_i s_i * P_i for 128-bit scalars, (n, 2) uint64 rows (little-endian), over G1 affine
    bases (pa_g1_multiexp_u128): one Jacobian row, the same point as g1_multiexp over the
    zero-extended scalars for any on-curve bases, in about half the windows."""
    b = as_rows(bases, W_G1A, "bases") if len(bases) else np.zeros((0, W_G1A), np.uint64)
    s = as_rows(scalars, 2, "scalars") if len(scalars) else np.zeros((0, 2), np.uint64)
    if b.shape[0] != s.shape[0]:
        raise ValueError("bases and scalars differ in length: %d vs %d" % (b.shape[0], s.shape[0]))
    out = np.zeros((1, W_G1), np.uint64)
    call("pa_g1_multiexp_u128", ptr(b), ptr(s), b.shape[0], ptr(out))
    return out


# the prepared entries of both groups: (handle class, affine width, Jacobian width)
_MSM_GROUPS = {1: (G1MsmBases, W_G1A, W_G1), 2: (G2MsmBases, W_G2A, W_G2)}


def _msm_prepare(group, bases):
    import ctypes
    cls, in_width, _ = _MSM_GROUPS[group]
    b = as_rows(bases, in_width, "bases") if len(bases) else np.zeros((0, in_width), np.uint64)
    h = ctypes.c_void_p(0)
    call("pa_g%d_msm_bases_prepare" % group, ptr(b), b.shape[0], ctypes.byref(h))
    return cls._adopt(h)


def _multiexp_prepared(group, prepared, scalars):
    cls, _, out_width = _MSM_GROUPS[group]
    msm_bases(prepared, cls, "g%d_msm_prepare" % group)
    s = as_rows(scalars, 4, "scalars") if len(scalars) else np.zeros((0, 4), np.uint64)
    h = prepared.check_terms(s.shape[0])
    out = np.zeros((1, out_width), np.uint64)
    call("pa_g%d_multiexp_prepared" % group, h, ptr(s), s.shape[0], ptr(out))
    return out


def _multiexp_prepared_batch(group, prepared, scalars, count, montgomery):
    cls, _, out_width = _MSM_GROUPS[group]
    msm_bases(prepared, cls, "g%d_msm_prepare" % group)
    flags = msm_scalars(montgomery)
    s, k, m = batch_shape(scalars, count)
    h = prepared.check_terms(m)
    out = np.zeros((k, out_width), np.uint64)
    call("pa_g%d_multiexp_prepared_batch" % group, h, ptr(s), m, k, flags, ptr(out))
    return out


def g1_msm_prepare(bases):
    """Prepare G1 affine bases ((n, 13) rows) for repeated multiexps: checked for G1
    membership and converted once, kept on the current device.  Returns a G1MsmBases
    (len, in_subgroup, close()); free it with close() or let it be collected."""
    return _msm_prepare(1, bases)


def g1_multiexp_prepared(prepared, scalars):
    """sum_i s_i * P_i over the first len(scalars) prepared bases: one Jacobian row, the
    same point as g1_multiexp over those bases (any 256-bit FrRepr)."""
    return _multiexp_prepared(1, prepared, scalars)


def g1_multiexp_prepared_batch(prepared, scalars, count=None, montgomery=False):
    """k multiexps over the same prepared bases in one call: scalars (k, m, 4), or
    (k * m, 4) rows with count=k vectors end to end; row j of the (k, 18) result is
    sum_i s[j][i] * P_i over the first m prepared bases, the same point as
    g1_multiexp_prepared(prepared, s[j]).  The rows are FrRepr (any 256-bit value),
    or with montgomery=True Montgomery Fr below r (what fr_ntt returns)."""
    return _multiexp_prepared_batch(1, prepared, scalars, count, montgomery)


def g2_msm_prepare(bases):
    """g1_msm_prepare for G2 affine bases ((n, 25) rows): returns a G2MsmBases.  A G1
    object is not a G2 one: each group's functions take only their own (ValueError)."""
    return _msm_prepare(2, bases)


def g2_multiexp_prepared(prepared, scalars):
    """sum_i s_i * Q_i over the first len(scalars) prepared G2 bases: one Jacobian row
    (1, 36), the same point as g2_multiexp over those bases (any 256-bit FrRepr)."""
    return _multiexp_prepared(2, prepared, scalars)


def g2_multiexp_prepared_batch(prepared, scalars, count=None, montgomery=False):
    """g1_multiexp_prepared_batch over prepared G2 bases: a (k, 36) result, row j the
    same point as g2_multiexp_prepared(prepared, s[j])."""
    return _multiexp_prepared_batch(2, prepared, scalars, count, montgomery)


# ---- batched Fr NTT over radix-2 evaluation domains ----
def fr_ntt_domain(log_n):
    """The evaluation domain of 2^log_n points on the current device: its power
    tables are built there once.  Returns an FrNttDomain (log_n, len, close());
    free it with close() or let it be collected.  PA_NTT_TILE_LOG is read here."""
    import ctypes
    log_n = int(log_n)
    if log_n < 0 or log_n > NTT_MAX_LOG_N:
        raise ValueError("log_n must be 0..%d, got %d" % (NTT_MAX_LOG_N, log_n))
    h = ctypes.c_void_p(0)
    call("pa_fr_ntt_domain_create", log_n, ctypes.byref(h))
    return FrNttDomain._adopt(h)


def fr_ntt(domain, a, mode="forward"):
    """The domain's transform of each polynomial of `a` ((batch * n, 4) Montgomery
    Fr rows, polynomial b in rows b n .. b n + n - 1, natural order in and out)
    as a new array.  mode: "forward" out[j] = sum_i a[i] w^(ij); "inverse" its
    inverse; "coset_forward" the forward transform of a[i] g^i (g = 7);
    "coset_inverse" the inverse transform, then out[i] g^-i."""
    if not isinstance(domain, FrNttDomain):
        raise ValueError("domain must come from fr_ntt_domain")
    domain.handle()   # a closed object is rejected first
    m = ntt_mode(mode)
    a = as_rows(a, W_FR, "a") if len(a) else np.zeros((0, W_FR), np.uint64)
    h, batch = domain.check_rows(a.shape[0])
    out = np.zeros_like(a)
    if batch:
        call("pa_fr_ntt", h, m, ptr(a), ptr(out), batch)
    return out


def fr_ntt_quotient(domain, a, b, c):
    """The quotient of a proof over the domain, as a new (batch * n, 4) array: from
    the evaluations a, b, c of each polynomial triple (three arrays laid out as
    fr_ntt's), the n coefficient rows of h = (A B - C) / (X^n - 1), that is
    coset_inverse((coset_forward(inverse(a)) * coset_forward(inverse(b))
    - coset_forward(inverse(c))) / (g^n - 1)), bit for bit.  Where c = a * b on
    the domain, row n - 1 of every polynomial is zero."""
    if not isinstance(domain, FrNttDomain):
        raise ValueError("domain must come from fr_ntt_domain")
    domain.handle()   # a closed object is rejected first
    a, b, c = (as_rows(x, W_FR, name) if len(x) else np.zeros((0, W_FR), np.uint64)
               for x, name in ((a, "a"), (b, "b"), (c, "c")))
    if a.shape != b.shape or a.shape != c.shape:
        raise ValueError("a, b and c must have the same shape, got %s, %s and %s" % (a.shape, b.shape, c.shape))
    h, batch = domain.check_rows(a.shape[0])
    out = np.zeros_like(a)
    if batch:
        call("pa_fr_ntt_quotient", h, ptr(a), ptr(b), ptr(c), ptr(out), batch)
    return out


# ---- R1CS matrices on the device and the Groth16 prover ----
def _csr(m, n_rows, n_cols, name):
    """(FrCsr, the arrays it points into) of one (row_ptr, col, val) triple, checked as pa_r1cs_create checks it"""
    import ctypes
    try:
        row_ptr, col, val = m
    except (TypeError, ValueError):
        raise ValueError("%s must be a (row_ptr, col, val) triple" % name) from None
    rp = np.asarray(row_ptr)
    co = np.asarray(col)
    if rp.ndim != 1 or rp.shape[0] != n_rows + 1 or (rp.size and rp.dtype.kind not in "iu"):
        raise ValueError("%s: row_ptr must be a 1-d integer array of n_rows + 1 = %d entries" % (name, n_rows + 1))
    if rp.dtype.kind == "i" and (rp < 0).any():
        raise ValueError("%s: row_ptr must not be negative" % name)
    rp = np.ascontiguousarray(rp, dtype=np.uint64)
    if int(rp[0]) != 0 or (rp[1:] < rp[:-1]).any():
        raise ValueError("%s: row_ptr must start at 0 and be non-decreasing" % name)
    nnz = int(rp[-1])
    if nnz >= 1 << 32:
        raise ValueError("%s: nnz must be below 2^32" % name)
    if co.ndim != 1 or co.shape[0] != nnz or (nnz and co.dtype.kind not in "iu"):
        raise ValueError("%s: col must be a 1-d integer array of nnz = %d entries" % (name, nnz))
    if nnz and (int(co.min()) < 0 or int(co.max()) >= n_cols):
        raise ValueError("%s: a column index is not below n_cols = %d" % (name, n_cols))
    co = np.ascontiguousarray(co, dtype=np.uint32)
    va = as_rows(val, W_FR, name + " val") if nnz else np.zeros((0, W_FR), np.uint64)
    if va.shape[0] != nnz:
        raise ValueError("%s: val must have nnz = %d rows, got %d" % (name, nnz, va.shape[0]))
    keep = (rp, co, va)
    return FrCsr(ctypes.c_void_p(rp.ctypes.data), ctypes.c_void_p(co.ctypes.data), ctypes.c_void_p(va.ctypes.data)), keep


def r1cs(a, b, c, n_rows, n_cols):
    """The matrices of a constraint system on the current device: a, b, c are CSR
    triples (row_ptr (n_rows + 1,), col (nnz,), val (nnz, 4) Montgomery Fr below r).
    Returns an R1cs (rows, cols, bytes, close()).  A value >= r is refused by the
    library (PairingError); everything else is a ValueError here."""
    import ctypes
    n_rows, n_cols = int(n_rows), int(n_cols)
    if n_rows < 0 or n_cols < 0 or n_rows > 1 << NTT_MAX_LOG_N:
        raise ValueError("n_rows must be 0..2^%d and n_cols >= 0" % NTT_MAX_LOG_N)
    ms = [_csr(m, n_rows, n_cols, name) for m, name in ((a, "a"), (b, "b"), (c, "c"))]
    h = ctypes.c_void_p(0)
    call("pa_r1cs_create", *(ctypes.byref(m[0]) for m in ms), n_rows, n_cols, ctypes.byref(h))
    return R1cs._adopt(h)


def r1cs_eval(system, witness, log_n, count=None):
    """(a, b, c), each (k * 2^log_n, 4): the products of the system's matrices with k
    witnesses ((k * cols, 4) Montgomery Fr rows end to end; count=k is needed only
    for a system of no columns), laid out as fr_ntt_quotient takes them; rows from
    the system's rows up to 2^log_n are zero."""
    if not isinstance(system, R1cs):
        raise ValueError("system must come from r1cs()")
    system.handle()   # a closed object is rejected first
    w = as_rows(witness, W_FR, "witness") if len(witness) else np.zeros((0, W_FR), np.uint64)
    h, k, log_n = system.check_eval(w.shape[0], count, log_n)
    outs = tuple(np.zeros((k << log_n, W_FR), np.uint64) for _ in range(3))
    if k:
        call("pa_r1cs_eval", h, ptr(w), k, log_n, *(ptr(o) for o in outs))
    return outs


def groth16_pk(alpha_g1, beta_g1, delta_g1, beta_g2, delta_g2, a_query, b_g1_query, b_g2_query, l_query, h_query,
               n_public, log_n):
    """A proving key on the current device (pa_groth16_pk_create): alpha_g1, beta_g1,
    delta_g1 (1, 13) and beta_g2, delta_g2 (1, 25) affine records; a_query, b_g1_query
    (n_vars, 13), b_g2_query (n_vars, 25), l_query (n_vars - n_public, 13) and h_query
    (h_len <= 2^log_n, 13).  n_public counts the constant one.  Returns a Groth16Pk."""
    import ctypes
    def rows(x, width, name):
        return as_rows(x, width, name) if len(x) else np.zeros((0, width), np.uint64)
    singles = [rows(x, w, name) for x, w, name in ((alpha_g1, W_G1A, "alpha_g1"), (beta_g1, W_G1A, "beta_g1"),
                                                   (delta_g1, W_G1A, "delta_g1"), (beta_g2, W_G2A, "beta_g2"),
                                                   (delta_g2, W_G2A, "delta_g2"))]
    for x, name in zip(singles, ("alpha_g1", "beta_g1", "delta_g1", "beta_g2", "delta_g2")):
        if x.shape[0] != 1:
            raise ValueError("%s must be one affine record, got %d" % (name, x.shape[0]))
    aq, b1q, lq, hq = (rows(x, W_G1A, name) for x, name in ((a_query, "a_query"), (b_g1_query, "b_g1_query"),
                                                             (l_query, "l_query"), (h_query, "h_query")))
    b2q = rows(b_g2_query, W_G2A, "b_g2_query")
    n_vars, n_public, log_n = aq.shape[0], int(n_public), int(log_n)
    if log_n < 0 or log_n > NTT_MAX_LOG_N:
        raise ValueError("log_n must be 0..%d, got %d" % (NTT_MAX_LOG_N, log_n))
    if b1q.shape[0] != n_vars or b2q.shape[0] != n_vars:
        raise ValueError("a_query, b_g1_query and b_g2_query must have n_vars rows each, got %d, %d and %d"
                         % (n_vars, b1q.shape[0], b2q.shape[0]))
    if n_public < 0 or n_public > n_vars or lq.shape[0] != n_vars - n_public:
        raise ValueError("l_query must have n_vars - n_public = %d rows, got %d" % (n_vars - n_public, lq.shape[0]))
    if hq.shape[0] > 1 << log_n:
        raise ValueError("h_query has %d rows, the domain %d points" % (hq.shape[0], 1 << log_n))
    key = Groth16Key()
    for field, x in zip(("alpha_g1", "beta_g1", "delta_g1", "beta_g2", "delta_g2"), singles):
        ctypes.memmove(getattr(key, field), x.ctypes.data, x.nbytes)
    key.n_vars, key.n_public, key.h_len = n_vars, n_public, hq.shape[0]
    for field, x in (("a_query", aq), ("b_g1_query", b1q), ("b_g2_query", b2q), ("l_query", lq), ("h_query", hq)):
        setattr(key, field, x.ctypes.data)
    h = ctypes.c_void_p(0)
    call("pa_groth16_pk_create", ctypes.byref(key), log_n, ctypes.byref(h))
    h = ctypes.c_void_p(h.value)
    return Groth16Pk(h, log_n, n_vars, n_public, hq.shape[0], _lib.pa_groth16_pk_in_subgroup(h))


def groth16_prove(pk, system, domain, witness, r, s):
    """k Groth16 proofs in one call (pa_groth16_prove): witness (k * n_vars, 4), r and s
    (k, 4) Montgomery Fr rows below r.  Returns (k, 51) uint64 rows, one
    pa_groth16_proof each: the affine records A (words 0..12), B (13..37) and C
    (38..50), bit for bit what into_affine of bellman's create_proof points gives."""
    if not isinstance(pk, Groth16Pk):
        raise ValueError("pk must come from groth16_pk")
    pk.handle()   # a closed object is rejected first
    w, r, s = (as_rows(x, W_FR, name) if len(x) else np.zeros((0, W_FR), np.uint64)
               for x, name in ((witness, "witness"), (r, "r"), (s, "s")))
    (h, hr, hd), k = pk.check_prove(system, domain, w.shape[0], r.shape[0], s.shape[0])
    out = np.zeros((k, W_PROOF), np.uint64)
    if k:
        call("pa_groth16_prove", h, hr, hd, ptr(w), ptr(r), ptr(s), k, ptr(out))
    return out


def groth16_circuit(a, b, c, n_rows, n_cols, n_public):
    """The constraint system as parameter generation reads it, on the current device
    (pa_groth16_circuit_create): a, b, c CSR triples as r1cs() takes them, n_cols variables of
    which the first n_public (counting the constant one) are public.  Returns a Groth16Circuit
    (rows, cols, n_public, bytes, close())."""
    import ctypes
    n_rows, n_cols, n_public = int(n_rows), int(n_cols), int(n_public)
    if n_rows < 0 or n_cols < 0 or n_rows > 1 << NTT_MAX_LOG_N or n_cols > 1 << NTT_MAX_LOG_N:
        raise ValueError("n_rows and n_cols must be 0..2^%d" % NTT_MAX_LOG_N)
    if n_public < 0 or n_public > n_cols:
        raise ValueError("n_public must be 0..n_cols = %d, got %d" % (n_cols, n_public))
    ms = [_csr(m, n_rows, n_cols, name) for m, name in ((a, "a"), (b, "b"), (c, "c"))]
    h = ctypes.c_void_p(0)
    call("pa_groth16_circuit_create", *(ctypes.byref(m[0]) for m in ms), n_rows, n_cols, n_public, ctypes.byref(h))
    return Groth16Circuit._adopt(h)


def groth16_generate(circuit, domain, trapdoor, g1, g2):
    """bellman's generate_parameters for the given trapdoor (pa_groth16_generate): trapdoor
    (5, 4) Montgomery Fr rows tau, alpha, beta, gamma, delta (below r; gamma, delta not zero),
    g1 (1, 13) and g2 (1, 25) affine base points.  Returns a Groth16Params: the named arrays of
    the proving and the verifying key as affine records, bit for bit what into_affine gives for
    them, with pk_args() for groth16_pk and vk_args() for groth16_vk."""
    if not isinstance(circuit, Groth16Circuit):
        raise ValueError("circuit must come from groth16_circuit")
    (h, hd), log_n = circuit.check_generate(domain)
    t = trapdoor_rows(trapdoor)
    p1, p2 = as_rows(g1, W_G1A, "g1"), as_rows(g2, W_G2A, "g2")
    if p1.shape[0] != 1 or p2.shape[0] != 1:
        raise ValueError("g1 and g2 must be one affine record each, got %d and %d" % (p1.shape[0], p2.shape[0]))
    o1 = np.zeros((circuit.g1_len(log_n), W_G1A), np.uint64)
    o2 = np.zeros((circuit.g2_len(), W_G2A), np.uint64)
    call("pa_groth16_generate", h, hd, ptr(p1), ptr(p2), ptr(t), ptr(o1), ptr(o2))
    return Groth16Params(o1, o2, circuit.cols, circuit.n_public, log_n)


def groth16_generate_scalars(circuit, domain, trapdoor):
    """The discrete logarithms of groth16_generate's G1 array in the same order, as
    (3 n_vars + 2^log_n + 2, 4) Montgomery Fr rows: u, v, the mixed rows (ic then l_query), the
    h rows, then alpha, beta, delta (pa_groth16_generate_scalars)."""
    if not isinstance(circuit, Groth16Circuit):
        raise ValueError("circuit must come from groth16_circuit")
    (h, hd), log_n = circuit.check_generate(domain)
    t = trapdoor_rows(trapdoor)
    out = np.zeros((circuit.g1_len(log_n), W_FR), np.uint64)
    call("pa_groth16_generate_scalars", h, hd, ptr(t), ptr(out))
    return out


def groth16_vk(alpha_g1, beta_g2, gamma_g2, delta_g2, ic):
    """A verifying key prepared on the current device (pa_groth16_vk_create): alpha_g1 (1, 13),
    beta_g2, gamma_g2, delta_g2 (1, 25) affine records and ic (n_public, 13), n_public >= 1
    counting the constant one.  Returns a Groth16Vk."""
    import ctypes
    singles = [as_rows(x, w, name) for x, w, name in ((alpha_g1, W_G1A, "alpha_g1"), (beta_g2, W_G2A, "beta_g2"),
                                                      (gamma_g2, W_G2A, "gamma_g2"), (delta_g2, W_G2A, "delta_g2"))]
    for x, name in zip(singles, ("alpha_g1", "beta_g2", "gamma_g2", "delta_g2")):
        if x.shape[0] != 1:
            raise ValueError("%s must be one affine record, got %d" % (name, x.shape[0]))
    icq = as_rows(ic, W_G1A, "ic") if len(ic) else np.zeros((0, W_G1A), np.uint64)
    if icq.shape[0] < 1 or icq.shape[0] - 1 > GROTH16_VK_MAX_INPUTS:
        raise ValueError("ic must have n_public = 1..%d rows, got %d" % (GROTH16_VK_MAX_INPUTS + 1, icq.shape[0]))
    key = Groth16VKey()
    for field, x in zip(("alpha_g1", "beta_g2", "gamma_g2", "delta_g2"), singles):
        ctypes.memmove(getattr(key, field), x.ctypes.data, x.nbytes)
    key.ic, key.n_public = icq.ctypes.data, icq.shape[0]
    h = ctypes.c_void_p(0)
    call("pa_groth16_vk_create", ctypes.byref(key), ctypes.byref(h))
    return Groth16Vk._adopt(h)


def _vk_inputs(vk, inputs, k, stride, montgomery):
    """(handle, input rows, stride, flag) of a call over k proofs; k None: as many as the rows hold"""
    if not isinstance(vk, Groth16Vk):
        raise ValueError("vk must come from groth16_vk")
    vk.handle()   # a closed object is rejected first
    flag = msm_scalars(montgomery)
    x = as_rows(inputs, W_FR, "inputs") if inputs is not None and len(inputs) else np.zeros((0, W_FR), np.uint64)
    if k is None:
        if vk.n_inputs == 0:
            raise ValueError("a key without inputs needs k")
        per = vk.n_inputs if stride is None else int(stride)
        if per < vk.n_inputs:
            raise ValueError("input stride %d is below the key's %d inputs" % (per, vk.n_inputs))
        k = (x.shape[0] + per - vk.n_inputs) // per if x.shape[0] >= vk.n_inputs else 0
    h, stride = vk.check_inputs(x.shape[0], k, stride)
    return h, x, int(k), stride, flag


def groth16_input_sum(vk, inputs, k=None, stride=None, montgomery=True):
    """The public-input sums of k proofs (pa_groth16_vk_input_sum): (k, 13) affine records
    ic[0] + sum_i x_i ic[i].  inputs: (rows, 4) rows, Montgomery Fr (montgomery=True) or FrRepr,
    row i of proof j at j * stride + i (stride None: n_inputs rows per proof, end to end)."""
    h, x, k, stride, flag = _vk_inputs(vk, inputs, k, stride, montgomery)
    out = np.zeros((k, W_G1A), np.uint64)
    if k:
        call("pa_groth16_vk_input_sum", h, ptr(x), stride, flag, k, ptr(out))
    return out


def groth16_verify(vk, proofs, inputs, montgomery=True, return_gt=False, stride=None):
    """k Groth16 proofs checked in one call (pa_groth16_verify): proofs (k, 51) rows as
    groth16_prove writes them, inputs as for groth16_input_sum.  Returns a (k,) bool array, or
    (valid, gt) with return_gt=True: gt (k, 72) = final_exponentiation(ML(A, B) ML(acc, -gamma)
    ML(C, -delta)), a zero row where that is None."""
    pr = as_rows(proofs, W_PROOF, "proofs") if len(proofs) else np.zeros((0, W_PROOF), np.uint64)
    h, x, k, stride, flag = _vk_inputs(vk, inputs, pr.shape[0], stride, montgomery)
    valid = np.zeros(k, np.uint8)
    gt = np.zeros((k, W_FQ12), np.uint64) if return_gt else None
    if k:
        call("pa_groth16_verify", h, ptr(pr), ptr(x), stride, flag, k, ptr(valid), ptr(gt) if return_gt else None)
    return (valid.astype(bool), gt) if return_gt else valid.astype(bool)


def groth16_verify_encoded(vk, data, inputs, montgomery=True, return_gt=False, stride=None):
    """groth16_verify for proofs off the wire (pa_groth16_verify_encoded): data (k, 192) uint8, A, B
    and C compressed in bellman's Proof::write order, through the checked decoders.  Returns
    (valid, status) or (valid, status, gt): status (k, 3) uint8 DECODE_STATUS codes of A, B, C;
    a proof with a nonzero status is not valid and its gt is meaningless."""
    enc = np.ascontiguousarray(np.asarray(data, dtype=np.uint8))
    if enc.ndim == 1:
        enc = enc.reshape(-1, GROTH16_ENCODED_PROOF_BYTES) if enc.size % GROTH16_ENCODED_PROOF_BYTES == 0 else enc
    if enc.ndim != 2 or enc.shape[1] != GROTH16_ENCODED_PROOF_BYTES:
        raise ValueError("encoded proofs must have shape (k, %d), got %s" % (GROTH16_ENCODED_PROOF_BYTES, enc.shape))
    h, x, k, stride, flag = _vk_inputs(vk, inputs, enc.shape[0], stride, montgomery)
    valid = np.zeros(k, np.uint8)
    status = np.zeros((k, 3), np.uint8)
    gt = np.zeros((k, W_FQ12), np.uint64) if return_gt else None
    if k:
        call("pa_groth16_verify_encoded", h, ptr(enc), ptr(x), stride, flag, k, ptr(valid), ptr(status),
             ptr(gt) if return_gt else None)
    return (valid.astype(bool), status, gt) if return_gt else (valid.astype(bool), status)


def _weights(z, k):
    """the (k, 2) uint64 weights of an aggregate call; None draws 16 bytes per proof from os.urandom"""
    if z is None:
        import os
        return np.frombuffer(os.urandom(16 * k), dtype="<u8").astype(np.uint64).reshape(k, 2)
    w = np.ascontiguousarray(z, dtype=np.uint64)
    if w.ndim != 2 or w.shape[1] != 2 or w.shape[0] != k:
        raise ValueError("z must have shape (%d, 2): one 128-bit weight per proof, got %s" % (k, w.shape))
    return w


def groth16_verify_aggregate(vk, proofs, inputs, z=None, montgomery=True, return_gt=False, stride=None):
    """k Groth16 proofs under one key checked by ONE randomised pairing product
    (pa_groth16_verify_aggregate; bellman's verify_proofs_batch): k + 3 Miller loops and one final
    exponentiation instead of 3 k and k.  proofs and inputs as for groth16_verify; z: (k, 2)
    uint64 rows, the 128-bit weights (little-endian), or None to draw them from os.urandom.
    Returns one bool for the batch, or (valid, gt) with return_gt=True: gt (1, 72), one when
    valid, a zero row where the final exponentiation is None.

    The points are taken as they are: the verdict equals "every proof passes groth16_verify"
    (up to a 2^-128 chance over random z of accepting a bad batch) only for points in G1 and
    G2; groth16_verify_aggregate_encoded checks that.  z_j = 0 drops proof j.  When a batch
    fails, run groth16_verify on it to find the bad proofs.  Up to 2^10 proofs groth16_verify
    is the faster call (device-resident on one MI355X: 5.6 ms against 7.5 at 2^10), at 2^14
    and above this one is (10.2 against 12.3, 19.6 against 29.1 at 2^16; README.md); there is
    no automatic choice, because the two return different things."""
    pr = as_rows(proofs, W_PROOF, "proofs") if len(proofs) else np.zeros((0, W_PROOF), np.uint64)
    h, x, k, stride, flag = _vk_inputs(vk, inputs, pr.shape[0], stride, montgomery)
    w = _weights(z, k)
    valid = np.zeros(1, np.uint8)
    gt = np.zeros((1, W_FQ12), np.uint64) if return_gt else None
    call("pa_groth16_verify_aggregate", h, ptr(pr), ptr(x), stride, flag, ptr(w), k, ptr(valid),
         ptr(gt) if return_gt else None)
    return (bool(valid[0]), gt) if return_gt else bool(valid[0])


def groth16_verify_aggregate_encoded(vk, data, inputs, z=None, montgomery=True, return_gt=False, stride=None):
    """groth16_verify_aggregate for proofs off the wire (pa_groth16_verify_aggregate_encoded): data
    (k, 192) uint8 as for groth16_verify_encoded, through the checked decoders, which enforce
    curve and subgroup membership.  Returns (valid, status) or (valid, status, gt): status (k, 3)
    uint8 DECODE_STATUS codes per proof; any nonzero status makes the batch not valid."""
    enc = np.ascontiguousarray(np.asarray(data, dtype=np.uint8))
    if enc.ndim == 1:
        enc = enc.reshape(-1, GROTH16_ENCODED_PROOF_BYTES) if enc.size % GROTH16_ENCODED_PROOF_BYTES == 0 else enc
    if enc.ndim != 2 or enc.shape[1] != GROTH16_ENCODED_PROOF_BYTES:
        raise ValueError("encoded proofs must have shape (k, %d), got %s" % (GROTH16_ENCODED_PROOF_BYTES, enc.shape))
    h, x, k, stride, flag = _vk_inputs(vk, inputs, enc.shape[0], stride, montgomery)
    w = _weights(z, k)
    valid = np.zeros(1, np.uint8)
    status = np.zeros((k, 3), np.uint8)
    gt = np.zeros((1, W_FQ12), np.uint64) if return_gt else None
    call("pa_groth16_verify_aggregate_encoded", h, ptr(enc), ptr(x), stride, flag, ptr(w), k, ptr(valid),
         ptr(status), ptr(gt) if return_gt else None)
    return (bool(valid[0]), status, gt) if return_gt else (bool(valid[0]), status)


def groth16_aggregate_points(vk, proofs, inputs, z, montgomery=True, stride=None):
    """The G1 side of the aggregate check (pa_groth16_verify_aggregate_points): (k + 3, 13) affine
    records z_0 A_0 .. z_{k-1} A_{k-1} | s_0 ic[0] + sum_i s_{i+1} ic[i+1] | sum_j z_j C_j | s_0 alpha
    with s_0 = sum_j z_j and s_{i+1} = sum_j z_j x_{j,i} mod r."""
    pr = as_rows(proofs, W_PROOF, "proofs") if len(proofs) else np.zeros((0, W_PROOF), np.uint64)
    h, x, k, stride, flag = _vk_inputs(vk, inputs, pr.shape[0], stride, montgomery)
    w = _weights(z, k)
    out = np.zeros((k + 3, W_G1A), np.uint64)
    call("pa_groth16_verify_aggregate_points", h, ptr(pr), ptr(x), stride, flag, ptr(w), k, ptr(out))
    return out


# ---- CurveProjective / CurveAffine surface for G1 and G2 (ec.rs:1-621) ----
_JW = {1: W_G1, 2: W_G2}
_AW = {1: W_G1A, 2: W_G2A}


def _group_unary(group, op, a, in_width, out_width):
    a = as_rows(a, in_width, "points")
    out = np.zeros((a.shape[0], out_width), np.uint64)
    call("pa_g%d_%s_batch" % (group, op), ptr(a), ptr(out), a.shape[0])
    return out


def _group_binary(group, op, a, b, b_width):
    a = as_rows(a, _JW[group], "a")
    b = as_rows(b, b_width, "b")
    if a.shape[0] != b.shape[0]:
        raise ValueError("operand lengths differ: %d vs %d" % (a.shape[0], b.shape[0]))
    out = np.zeros_like(a)
    call("pa_g%d_%s_batch" % (group, op), ptr(a), ptr(b), ptr(out), a.shape[0])
    return out


def _group_eq(group, a, b):
    a = as_rows(a, _JW[group], "a")
    b = as_rows(b, _JW[group], "b")
    if a.shape[0] != b.shape[0]:
        raise ValueError("operand lengths differ: %d vs %d" % (a.shape[0], b.shape[0]))
    out = np.zeros(a.shape[0], np.uint8)
    call("pa_g%d_eq_batch" % group, ptr(a), ptr(b), ptr(out), a.shape[0])
    return out.astype(bool)


def g1_eq(a, b):
    """PartialEq for G1 (ec.rs:45-85): a[i] == b[i] as points, per item."""
    return _group_eq(1, a, b)


def g2_eq(a, b):
    """PartialEq for G2 (ec.rs:45-85): a[i] == b[i] as points, per item."""
    return _group_eq(2, a, b)


def g1_double(a):
    """CurveProjective::double (dbl-2009-l, ec.rs:296-354), Jacobian words bit-exact."""
    return _group_unary(1, "double", a, W_G1, W_G1)


def g2_double(a):
    return _group_unary(2, "double", a, W_G2, W_G2)


def g1_add(a, b):
    """CurveProjective::add_assign (add-2007-bl, ec.rs:356-444)."""
    return _group_binary(1, "add", a, b, W_G1)


def g2_add(a, b):
    return _group_binary(2, "add", a, b, W_G2)


def g1_add_mixed(a, b):
    """CurveProjective::add_assign_mixed (madd-2007-bl, ec.rs:446-526), b affine."""
    return _group_binary(1, "add_mixed", a, b, W_G1A)


def g2_add_mixed(a, b):
    return _group_binary(2, "add_mixed", a, b, W_G2A)


def g1_negate(a):
    """CurveProjective::negate (ec.rs:528-532)."""
    return _group_unary(1, "negate", a, W_G1, W_G1)


def g2_negate(a):
    return _group_unary(2, "negate", a, W_G2, W_G2)


def g1_sub(a, b):
    """CurveProjective::sub_assign = negate + add_assign (lib.rs:156-160)."""
    return _group_binary(1, "sub", a, b, W_G1)


def g2_sub(a, b):
    return _group_binary(2, "sub", a, b, W_G2)


def g1_into_affine(a):
    """CurveProjective::into_affine (ec.rs:586-619)."""
    return _group_unary(1, "into_affine", a, W_G1, W_G1A)


def g2_into_affine(a):
    return _group_unary(2, "into_affine", a, W_G2, W_G2A)


def g1_into_projective(a):
    """CurveAffine::into_projective (ec.rs:570-582)."""
    return _group_unary(1, "into_projective", a, W_G1A, W_G1)


def g2_into_projective(a):
    return _group_unary(2, "into_projective", a, W_G2A, W_G2)


def g2_batch_normalization(v):
    """G2 CurveProjective::batch_normalization (ec.rs:246-294); returns the normalized copy."""
    v = as_rows(v, W_G2, "v").copy()
    call("pa_g2_batch_normalization", ptr(v), v.shape[0])
    return v


def g2_wnaf_fixed_base(base, scalars, window=None):
    """G2 Wnaf::new().base(base, n).scalar(s) (wnaf.rs:93-107, 169-178): points
    equal to the reference's wNAF products (see g1_wnaf_fixed_base)."""
    b = as_rows(base, W_G2, "base")
    s = as_rows(scalars, 4, "scalars")
    out = np.empty((s.shape[0], W_G2), np.uint64)
    if window is None:
        call("pa_g2_wnaf_fixed_base", ptr(b), ptr(s), s.shape[0], ptr(out))
    else:
        call("pa_g2_wnaf_fixed_base_window", ptr(b), ptr(s), s.shape[0], int(window), ptr(out))
    return out


def _window(name, arg):
    w = getattr(_lib, name)(arg)
    if w <= 0:
        raise PairingError("%s failed (%d)" % (name, w))
    return w


def g1_recommended_wnaf_for_scalar(scalar):
    """CurveProjective::recommended_wnaf_for_scalar for G1 (ec.rs:895-905), scalar a FrRepr row."""
    s = as_rows(scalar, 4, "scalar")
    return _window("pa_g1_recommended_wnaf_for_scalar", ptr(s))


def g2_recommended_wnaf_for_scalar(scalar):
    s = as_rows(scalar, 4, "scalar")
    return _window("pa_g2_recommended_wnaf_for_scalar", ptr(s))


def g1_recommended_wnaf_for_num_scalars(n):
    """CurveProjective::recommended_wnaf_for_num_scalars for G1 (ec.rs:907-921)."""
    return _window("pa_g1_recommended_wnaf_for_num_scalars", int(n))


def g2_recommended_wnaf_for_num_scalars(n):
    return _window("pa_g2_recommended_wnaf_for_num_scalars", int(n))
