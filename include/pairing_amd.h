/*
 * pairing_amd -- MI355X-native batched BLS12-381 engine, C ABI.
 *
 * This is the drop-in boundary for the hot path of the Rust crate `pairing`
 * v0.14.2 (dignifiedquire/pairing).  The reference has no FFI of its own: its
 * interface is the Rust trait surface in src/lib.rs.  Each entry point below
 * names the trait method (reference file:line) it replaces, batched over n
 * independent items.  INTEGRATION.md shows the Rust `extern "C"` block a
 * maintainer would add to bind it.
 *
 * Data layout (host and device) is the Rust in-memory order of the reference
 * types, so a `&[G1Affine]` can be passed by pointer:
 *   Fq        = 6 x u64, little-endian limbs, Montgomery form (R = 2^384), < q
 *               (src/bls12_381/fq.rs:699-700)
 *   Fq2       = {c0, c1}            Fq6 = {c0, c1, c2}       Fq12 = {c0, c1}
 *   G1Affine  = {Fq x, Fq y, u8 infinity, 7 pad}   (104 B)   ec.rs:13-18
 *   G2Affine  = {Fq2 x, Fq2 y, u8 infinity, 7 pad} (200 B)
 *   G1 / G2   = Jacobian {x, y, z}, zero iff z == 0 (144 B / 288 B) ec.rs:31-36
 *   FrRepr    = 4 x u64 little-endian, canonical (not Montgomery) fr.rs:58
 *   G2Prepared= 68 x (Fq2, Fq2, Fq2) line coefficients + u8 infinity + 7 pad
 *               (ec.rs:1615-1619, built by mod.rs:168-358) = 19 592 B
 *
 * Conventions
 *   - Every function returns 0 (PA_OK) or a negative PA_ERR_* code; nothing
 *     aborts across the ABI.  pa_last_error() describes the last failure on
 *     the calling thread.
 *   - Per-item Option results (reference returns None) are reported through a
 *     caller-provided u8 `ok` array: 1 = Some, 0 = None.
 *   - Host-pointer functions (no suffix) are synchronous: they copy inputs to
 *     the current device, run, and copy outputs back.  The caller owns all
 *     buffers; nothing is retained after return.  `out` may alias an input of
 *     the same type (giving the reference's *_assign in-place semantics).
 *   - `_device` functions take device pointers and a hipStream_t (as void*,
 *     NULL = default stream) and return after enqueueing; inputs must stay
 *     valid until the stream reaches the work.
 *   - Thread safety: all entry points are reentrant (the reference traits are
 *     Send + Sync, lib.rs:114-121, 185-186).  The device used is the calling
 *     thread's current HIP device (pa_set_device).
 */
#ifndef PAIRING_AMD_H
#define PAIRING_AMD_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define PA_OK 0
#define PA_ERR_INVALID_ARGUMENT (-1)
#define PA_ERR_HIP (-2)
#define PA_ERR_OUT_OF_MEMORY (-3)
#define PA_ERR_NO_DEVICE (-4)

#define PA_G2_PREPARED_COEFFS 68

typedef struct { uint64_t l[6]; } pa_fq;
typedef struct { pa_fq c0, c1; } pa_fq2;
typedef struct { pa_fq2 c0, c1, c2; } pa_fq6;
typedef struct { pa_fq6 c0, c1; } pa_fq12;
typedef struct { uint64_t l[4]; } pa_fr_repr;   /* canonical scalar, fr.rs:58 */
typedef struct { uint64_t l[6]; } pa_fq_repr;   /* canonical base-field words, FqRepr fq.rs:699-700 */
typedef struct { uint64_t l[4]; } pa_fr;        /* Montgomery form (R = 2^256), < r, fr.rs:247 */
typedef struct { pa_fq x, y; uint8_t infinity; uint8_t _pad[7]; } pa_g1_affine;
typedef struct { pa_fq2 x, y; uint8_t infinity; uint8_t _pad[7]; } pa_g2_affine;
typedef struct { pa_fq x, y, z; } pa_g1;
typedef struct { pa_fq2 x, y, z; } pa_g2;
typedef struct {
    pa_fq2 coeffs[PA_G2_PREPARED_COEFFS][3];
    uint8_t infinity;
    uint8_t _pad[7];
} pa_g2_prepared;

/* ---- runtime ---- */
const char *pa_version(void);
const char *pa_last_error(void);
int pa_device_count(int *count);
int pa_set_device(int device);
int pa_synchronize(void);
/* Tuning knob: which kernels run the Miller loop / final exponentiation
 * (identical results):
 *   0 = default, by batch size n: n <= PA_PQ_MIN (768) on the
 *       cooperative kernels (a four-wave quad-VM workgroup per pairing,
 *       kernels_coop.hip: the verifier shape, ~1.6 ms), n <= PA_PQ_MAX
 *       (4096) on the lane-group kernels (round 6, kernels_pair_quad.hip:
 *       one pairing per 32 lanes, rounds of up to 2048 pairings at ~3.8 ms;
 *       with PA_PQ_MAX = 0 the cooperative kernels run up to PA_COOP_MAX
 *       = 2304), n <= PA_PAIR_MAX
 *       (32768) on the generated kernels with a lane pair per pairing
 *       (~8.6-9.3 ms), n <= PA_PAIR_MAX + PA_TAIL_MAX (34816; round 6)
 *       as the first 32768 on lane pairs and the tail on a stream forked
 *       from the caller's -- on the cooperative kernels up to 832 tail
 *       pairings, the lane-group kernels above (32769 pairs in ~10.8 ms,
 *       34816 in ~13.0; not under stream capture, where the
 *       one-pairing-per-lane kernels run up to 34048, ~15.7 ms), larger
 *       batches on lane
 *       pairs again, two waves per SIMD (2^16 in ~15.7 ms; tools/pgen: own
 *       register allocation, code objects lib/pa_gen_*.hsaco, each loaded
 *       at its first use).  e(P, Q) entries (pa_pairing_batch, multi_pairing)
 *       run the pairing-only Miller loops (lane pairs and, round 6, one lane
 *       per pairing); the Miller-loop entries keep the reference's values and
 *       switch from one lane to lane pairs above 38912 (PA_ML_ONE_MAX)
 *   1 = generated kernels with a lane pair per pairing, every size (A/B)
 *   2 = cooperative kernels for every size (A/B, tests)
 *   3 = generated one-pairing-per-lane kernels for every size (A/B, tests)
 *   4 = cooperative kernels for every size on the round-2 one-wave VM
 *       (A/B, tests; added in round 3 -- 0 and 2 now run batches of up to
 *       PA_COOP_QUAD_MAX items on the four-wave quad VM, same results)
 *   5 = lane-group kernels for every size (round 6: one pairing per 32
 *       lanes, the tower's products batched into levels over 8 lane quads,
 *       kernels_pair_quad.hip; the Miller values are the reference's)
 * Process-wide; not part of the reference interface.
 * Behavior change in round 2: the numbering was 0 = hipcc lazy core,
 * 1 / 2 = hipcc 32-bit word kernels (one lane / two lanes), 3 = generated,
 * 4 / 5 = generated lane pairs / lazy reduction.  Those kernels are gone; the
 * values above now mean what is listed and anything outside 0..4 returns
 * PA_ERR_INVALID_ARGUMENT (4 was "lazy reduction" before round 2 and is the
 * one-wave cooperative VM since round 3). */
int pa_set_pairing_kernel(int variant);
/* Point-decoding kernel selection (A/B, tests): 0 = by batch size (default:
 * up to PA_DECODE_QUAD_MAX records, 8192 unless the environment says
 * otherwise, one record per group of lane quads -- the verifier's latency
 * form; larger batches one lane per record), 1 = one lane per record, 2 =
 * quad groups for every size.  Same statuses and outputs.  Process-wide; not
 * part of the reference interface. */
int pa_set_decode_kernel(int variant);

/* ---- Fq (src/bls12_381/fq.rs, Field trait src/lib.rs:267-325) ---- */
/* Field::mul_assign, fq.rs:909-960 + mont_reduce fq.rs:1036-1122 */
int pa_fq_mul_batch(const pa_fq *a, const pa_fq *b, pa_fq *out, size_t n);
/* Field::square, fq.rs:962-1016 */
int pa_fq_square_batch(const pa_fq *a, pa_fq *out, size_t n);
/* Field::add_assign / sub_assign, fq.rs:812-838 */
int pa_fq_add_batch(const pa_fq *a, const pa_fq *b, pa_fq *out, size_t n);
int pa_fq_sub_batch(const pa_fq *a, const pa_fq *b, pa_fq *out, size_t n);
/* Field::inverse, fq.rs:849-902 (ok[i] = 0 for a zero input) */
int pa_fq_inverse_batch(const pa_fq *a, pa_fq *out, uint8_t *ok, size_t n);
/* PrimeField::from_repr, fq.rs:747-756: ok[i] = 0 = Err(NotInField) when repr >= q (out[i] = 0);
 * otherwise out[i] = repr * R^2 (Montgomery form) */
int pa_fq_from_repr_batch(const pa_fq_repr *repr, pa_fq *out, uint8_t *ok, size_t n);
/* PrimeField::into_repr, fq.rs:758-775: the canonical words (mont_reduce of a) */
int pa_fq_into_repr_batch(const pa_fq *a, pa_fq_repr *out, size_t n);

/* ---- tower (fq2.rs, fq6.rs, fq12.rs) ---- */
int pa_fq2_mul_batch(const pa_fq2 *a, const pa_fq2 *b, pa_fq2 *out, size_t n);     /* fq2.rs:123-136 */
int pa_fq2_square_batch(const pa_fq2 *a, pa_fq2 *out, size_t n);                   /* fq2.rs:87-101 */
int pa_fq6_mul_batch(const pa_fq6 *a, const pa_fq6 *b, pa_fq6 *out, size_t n);     /* fq6.rs:199-248 */
int pa_fq12_mul_batch(const pa_fq12 *a, const pa_fq12 *b, pa_fq12 *out, size_t n); /* fq12.rs:116-130 */
int pa_fq12_square_batch(const pa_fq12 *a, pa_fq12 *out, size_t n);                /* fq12.rs:99-114 */
int pa_fq12_inverse_batch(const pa_fq12 *a, pa_fq12 *out, uint8_t *ok, size_t n);  /* fq12.rs:132-148 */
int pa_fq12_frobenius_map_batch(const pa_fq12 *a, pa_fq12 *out, size_t n, size_t power); /* fq12.rs:90-97 */
int pa_fq2_inverse_batch(const pa_fq2 *a, pa_fq2 *out, uint8_t *ok, size_t n);    /* fq2.rs:138-155 */
int pa_fq2_frobenius_map_batch(const pa_fq2 *a, pa_fq2 *out, size_t n, size_t power); /* fq2.rs:157-159 */
int pa_fq6_square_batch(const pa_fq6 *a, pa_fq6 *out, size_t n);                   /* fq6.rs:166-197 */
int pa_fq6_inverse_batch(const pa_fq6 *a, pa_fq6 *out, uint8_t *ok, size_t n);    /* fq6.rs:250-301 */
int pa_fq6_frobenius_map_batch(const pa_fq6 *a, pa_fq6 *out, size_t n, size_t power); /* fq6.rs:157-164 */
/* Field::pow, lib.rs:306-324, one exponent (exp_words u64, little-endian) for every element */
int pa_fq_pow_batch(const pa_fq *a, const uint64_t *exp, size_t exp_words, pa_fq *out, size_t n);
int pa_fq12_pow_batch(const pa_fq12 *a, const uint64_t *exp, size_t exp_words, pa_fq12 *out, size_t n);
/* Fq12::mul_by_014, fq12.rs:34-48 */
int pa_fq12_mul_by_014_batch(const pa_fq12 *a, const pa_fq2 *c0, const pa_fq2 *c1, const pa_fq2 *c4,
                             pa_fq12 *out, size_t n);

/* ---- G2 line precomputation: G2Prepared::from_affine, mod.rs:168-358 ---- */
int pa_g2_prepare_batch(const pa_g2_affine *q, pa_g2_prepared *out, size_t n);

/* ---- Engine (src/lib.rs:34-110, src/bls12_381/mod.rs:30-161) ---- */
/* n independent single-pair loops: out[i] = Bls12::miller_loop([(p[i], q[i])]) (mod.rs:40-102) */
int pa_miller_loop_batch(const pa_g1_affine *p, const pa_g2_prepared *q, pa_fq12 *out, size_t n);
/* One G2Prepared shared by every pair -- Engine::miller_loop takes &G2Prepared
 * references (lib.rs:88-96, Prepared: Clone lib.rs:192), so a caller may pass the
 * same prepared Q for each P (a verifying key's prepared gamma / delta):
 * out[i] = Bls12::miller_loop([(p[i], q)]) (mod.rs:40-102) for i < n, where `q`
 * is ONE record.  Its lines are staged once per call; no G2 arithmetic per pair.
 * Same bits as pa_miller_loop_batch with q repeated n times. */
int pa_miller_loop_shared_prepared(const pa_g1_affine *p, size_t n, const pa_g2_prepared *q, pa_fq12 *out);
/* Engine::miller_loop over n pairs: the product semantics of mod.rs:40-102 */
int pa_multi_miller_loop(const pa_g1_affine *p, const pa_g2_prepared *q, size_t n, pa_fq12 *out);
/* Engine::final_exponentiation, mod.rs:104-160; ok[i] = 0 iff in[i] == 0 */
int pa_final_exponentiation_batch(const pa_fq12 *in, pa_fq12 *out, uint8_t *ok, size_t n);
/* Engine::pairing, lib.rs:101-109: out[i] = e(p[i], q[i]) (prepare fused on device).
 * Like the reference, no precondition on the points: p[i] and q[i] may be any
 * field elements (outside the subgroups, of small order, or no curve point at
 * all, as the unchecked decoders hand them on), and out[i] is the reference's
 * value for them at every batch size -- a zero record where it is None (Miller
 * value 0).  Cost of a Q off E': the batches the pairing-only Miller loops
 * serve (above PA_PQ_MAX pairs) test every Q against the curve in one more
 * launch (k_pairing_ml_fixup: within run-to-run noise at 2^16 pairs, 15.3 ms)
 * and recompute an off-curve pair in reference form on one lane -- one serial
 * Miller loop for the call, 8 to 12 ms whether it holds one such pair or 64
 * (profiles/pairing_domain/).  The same
 * holds for pa_multi_pairing*, pa_pairing_batch_device and
 * pa_pairing_miller_loop_batch_device. */
int pa_pairing_batch(const pa_g1_affine *p, const pa_g2_affine *q, pa_fq12 *out, size_t n);

/* ---- G1 (config 3: parameter generation) ---- */
/* CurveProjective::batch_normalization, ec.rs:246-294, in place.  Zero and
 * already-normalized points are left untouched; others get z = 1. */
int pa_g1_batch_normalization(pa_g1 *v, size_t n);
/* Wnaf::new().base(*base, n).scalar(scalars[i]) for every i (wnaf.rs:93-107,
 * 169-178): out[i] = the reference's wNAF product of scalars[i] and base as a
 * Jacobian point (equal as a point to the reference's; representation-
 * independent PartialEq, ec.rs:45-85).  That is scalars[i] * base for every
 * 256-bit FrRepr except where the reference's wnaf_form wraps in add_nocarry
 * (wnaf.rs:30-35: s odd with bits w..255 all ones, w the window
 * recommended_wnaf_for_num_scalars(n)); there it is (s - 2^256) * base, which
 * these entries reproduce. */
int pa_g1_wnaf_fixed_base(const pa_g1 *base, const pa_fr_repr *scalars, size_t n, pa_g1 *out);
/* the same with the window given: Wnaf::new().base(*base, num_scalars) picks
 * window = recommended_wnaf_for_num_scalars(num_scalars) and .shared() copies
 * may then multiply any number n of scalars (wnaf.rs:93-107, 131-154);
 * window in 1..62 */
int pa_g1_wnaf_fixed_base_window(const pa_g1 *base, const pa_fr_repr *scalars, size_t n, int window, pa_g1 *out);

/* ---- CurveProjective / CurveAffine per-op batches, G1 and G2 ----
 * The `curve_impl!` group law (ec.rs:1-621) for both groups, one item per
 * lane, replaying the reference's formula sequence: Jacobian outputs equal
 * the reference's X, Y, Z words bit for bit (zero = z == 0; a zero produced
 * by P + (-P) keeps the x, y words the formulas leave, ec.rs:398, 477). */
/* CurveProjective::double, dbl-2009-l, ec.rs:296-354 */
int pa_g1_double_batch(const pa_g1 *a, pa_g1 *out, size_t n);
int pa_g2_double_batch(const pa_g2 *a, pa_g2 *out, size_t n);
/* CurveProjective::add_assign, add-2007-bl, ec.rs:356-444: out[i] = a[i] + b[i] */
int pa_g1_add_batch(const pa_g1 *a, const pa_g1 *b, pa_g1 *out, size_t n);
int pa_g2_add_batch(const pa_g2 *a, const pa_g2 *b, pa_g2 *out, size_t n);
/* CurveProjective::add_assign_mixed, madd-2007-bl, ec.rs:446-526 */
int pa_g1_add_mixed_batch(const pa_g1 *a, const pa_g1_affine *b, pa_g1 *out, size_t n);
int pa_g2_add_mixed_batch(const pa_g2 *a, const pa_g2_affine *b, pa_g2 *out, size_t n);
/* CurveProjective::negate, ec.rs:528-532 */
int pa_g1_negate_batch(const pa_g1 *a, pa_g1 *out, size_t n);
int pa_g2_negate_batch(const pa_g2 *a, pa_g2 *out, size_t n);
/* CurveProjective::sub_assign = negate + add_assign, lib.rs:156-160 */
int pa_g1_sub_batch(const pa_g1 *a, const pa_g1 *b, pa_g1 *out, size_t n);
int pa_g2_sub_batch(const pa_g2 *a, const pa_g2 *b, pa_g2 *out, size_t n);
/* CurveProjective::into_affine, ec.rs:586-619 (zero -> the point at infinity) */
int pa_g1_into_affine_batch(const pa_g1 *a, pa_g1_affine *out, size_t n);
int pa_g2_into_affine_batch(const pa_g2 *a, pa_g2_affine *out, size_t n);
/* CurveAffine::into_projective, ec.rs:570-582 */
int pa_g1_into_projective_batch(const pa_g1_affine *a, pa_g1 *out, size_t n);
int pa_g2_into_projective_batch(const pa_g2_affine *a, pa_g2 *out, size_t n);
/* PartialEq for the projective types, ec.rs:45-85 (representation independent:
 * X1 Z2^2 == X2 Z1^2 and Y1 Z2^3 == Y2 Z1^3; zero equals only zero):
 * eq[i] = 1 if a[i] == b[i], else 0 */
int pa_g1_eq_batch(const pa_g1 *a, const pa_g1 *b, uint8_t *eq, size_t n);
int pa_g2_eq_batch(const pa_g2 *a, const pa_g2 *b, uint8_t *eq, size_t n);
/* G2 CurveProjective::batch_normalization, ec.rs:246-294, in place */
int pa_g2_batch_normalization(pa_g2 *v, size_t n);
/* G2 Wnaf::new().base(*base, n).scalar(scalars[i]) (wnaf.rs:93-107, 169-178):
 * out[i] = the reference's wNAF product, equal as a point to the reference's
 * (PartialEq, ec.rs:45-85), including its add_nocarry wrap (wnaf.rs:30-35; see
 * pa_g1_wnaf_fixed_base); _window: the window given, 1..62 */
int pa_g2_wnaf_fixed_base(const pa_g2 *base, const pa_fr_repr *scalars, size_t n, pa_g2 *out);
int pa_g2_wnaf_fixed_base_window(const pa_g2 *base, const pa_fr_repr *scalars, size_t n, int window, pa_g2 *out);
/* Bit-exact Wnaf (wnaf.rs:1-179): the reference's window table chain
 * (wnaf_table, wnaf.rs:3-15), wnaf_form (:18-43) and wnaf_exp (:45-71), so the
 * Jacobian X, Y, Z words equal the reference's -- not only the point, as the
 * comb behind pa_g{1,2}_wnaf_fixed_base gives.  Slower than the comb (the
 * table is 2^(w-1) Jacobian entries, the multiply 256 doublings per scalar).
 * Fixed base: Wnaf::new().base(*base, num).scalar(scalars[i]) for every i
 * (wnaf.rs:93-107, 169-178); window 1..20, or 0 for
 * recommended_wnaf_for_num_scalars(n).  The table is rebuilt in parallel from
 * the chain's closed form (kernels_wnaf_exact.hip); a base whose chain takes a
 * special branch (outside G1) gets the serial chain. */
int pa_g1_wnaf_fixed_base_exact(const pa_g1 *base, const pa_fr_repr *scalars, size_t n, int window, pa_g1 *out);
int pa_g2_wnaf_fixed_base_exact(const pa_g2 *base, const pa_fr_repr *scalars, size_t n, int window, pa_g2 *out);
/* Fixed scalar: Wnaf::new().scalar(*scalar).base(bases[i]) for every i
 * (wnaf.rs:111-128, 156-166); window 1..12, or 0 for
 * recommended_wnaf_for_scalar(*scalar) */
int pa_g1_wnaf_fixed_scalar_exact(const pa_g1 *bases, size_t n, const pa_fr_repr *scalar, int window, pa_g1 *out);
int pa_g2_wnaf_fixed_scalar_exact(const pa_g2 *bases, size_t n, const pa_fr_repr *scalar, int window, pa_g2 *out);
/* device forms: `workspace` holds pa_wnaf_exact_workspace_bytes(group, n,
 * window, fixed_scalar) bytes (window as resolved: 1..20 / 1..12; the fixed-
 * scalar device form takes its window explicitly, its scalar being device memory) */
size_t pa_wnaf_exact_workspace_bytes(int group, size_t n, int window, int fixed_scalar);
int pa_g1_wnaf_fixed_base_exact_device(const pa_g1 *base, const pa_fr_repr *scalars, pa_g1 *out, size_t n,
                                       int window, void *workspace, size_t workspace_bytes, void *stream);
int pa_g2_wnaf_fixed_base_exact_device(const pa_g2 *base, const pa_fr_repr *scalars, pa_g2 *out, size_t n,
                                       int window, void *workspace, size_t workspace_bytes, void *stream);
int pa_g1_wnaf_fixed_scalar_exact_device(const pa_g1 *bases, size_t n, const pa_fr_repr *scalar, pa_g1 *out,
                                         int window, void *workspace, size_t workspace_bytes, void *stream);
int pa_g2_wnaf_fixed_scalar_exact_device(const pa_g2 *bases, size_t n, const pa_fr_repr *scalar, pa_g2 *out,
                                         int window, void *workspace, size_t workspace_bytes, void *stream);
/* CurveProjective::recommended_wnaf_for_scalar / _for_num_scalars
 * (lib.rs:166-174; G1 ec.rs:895-921, G2 ec.rs:1586-1612): the window the
 * reference's Wnaf would pick (returned as a positive int).  The GPU
 * fixed-base path does not depend on it (signed base-256 comb). */
int pa_g1_recommended_wnaf_for_scalar(const pa_fr_repr *scalar);
int pa_g2_recommended_wnaf_for_scalar(const pa_fr_repr *scalar);
int pa_g1_recommended_wnaf_for_num_scalars(size_t num_scalars);
int pa_g2_recommended_wnaf_for_num_scalars(size_t num_scalars);

/* ---- point encodings and square roots (SURVEY.md §8 f, rank 1) ----
 * Wire format of src/bls12_381/README.md "Serialization": big-endian
 * coordinates (G2: x.c1, x.c0, y.c1, y.c0), flag bits in byte 0 (bit 7
 * compressed, bit 6 infinity, bit 5 lexicographically largest y).  Record
 * sizes: G1 uncompressed 96 B, compressed 48 B; G2 192 B / 96 B.
 * status[i] is the GroupDecodingError (lib.rs:469-481) of record i: */
#define PA_DECODE_OK 0
#define PA_DECODE_NOT_ON_CURVE 1
#define PA_DECODE_NOT_IN_SUBGROUP 2
#define PA_DECODE_COORDINATE_X_C0 3   /* G1: "x coordinate"; G2: "x coordinate (c0)" */
#define PA_DECODE_COORDINATE_X_C1 4   /* G2: "x coordinate (c1)" */
#define PA_DECODE_COORDINATE_Y_C0 5   /* G1: "y coordinate"; G2: "y coordinate (c0)" */
#define PA_DECODE_COORDINATE_Y_C1 6   /* G2: "y coordinate (c1)" */
#define PA_DECODE_UNEXPECTED_COMPRESSION_MODE 7
#define PA_DECODE_UNEXPECTED_INFORMATION 8
/* EncodedPoint::into_affine (checked = 1: on-curve + subgroup checks,
 * ec.rs:662-668, 785-792, 1322-1332, 1448-1455) or into_affine_unchecked
 * (checked = 0).  Records that fail get status != 0 and out[i] = the point at
 * infinity. */
int pa_g1_decode_batch(const uint8_t *enc, size_t n, int compressed, int checked, pa_g1_affine *out,
                       uint8_t *status);
int pa_g2_decode_batch(const uint8_t *enc, size_t n, int compressed, int checked, pa_g2_affine *out,
                       uint8_t *status);
/* is_in_correct_subgroup_assuming_on_curve (ec.rs:142-144, r * P == 0) for
 * affine points: ok[i] = 1 in the subgroup (infinity included), 0 not.
 * into_affine = into_affine_unchecked + is_on_curve + this check (ec.rs:676-684,
 * 786-793, 1323-1331, 1449-1457); for compressed encodings the unchecked
 * decode already rejects points off the curve, so decode(checked) ==
 * decode(unchecked) followed by this check (a failing point: status
 * PA_DECODE_NOT_IN_SUBGROUP, output the point at infinity).  Apart, a verifier
 * can start its pairing on the unchecked points while the check runs beside it
 * (bench.py --workload verify --decode).  Points off the curve: unspecified
 * (the reference's "assuming on curve"). */
int pa_g1_subgroup_check_batch(const pa_g1_affine *p, size_t n, uint8_t *ok);
int pa_g2_subgroup_check_batch(const pa_g2_affine *p, size_t n, uint8_t *ok);
/* EncodedPoint::from_affine (ec.rs:737-752, 839-867, 1398-1415, 1510-1539) */
int pa_g1_encode_batch(const pa_g1_affine *in, size_t n, int compressed, uint8_t *enc);
int pa_g2_encode_batch(const pa_g2_affine *in, size_t n, int compressed, uint8_t *enc);
/* SqrtField::sqrt, fq.rs:1147-1170 / fq2.rs:167-220; ok[i] = 0 for a non-residue */
int pa_fq_sqrt_batch(const pa_fq *a, pa_fq *out, uint8_t *ok, size_t n);
int pa_fq2_sqrt_batch(const pa_fq2 *a, pa_fq2 *out, uint8_t *ok, size_t n);

/* ---- multi-pairing and multi-device (SURVEY.md §8 b, e, f rank 2) ---- */
/* Engine::miller_loop over n (G1Affine, G2Affine) pairs -- prepare fused on
 * device -- = the product of the per-pair loops (mod.rs:40-102); then, for
 * pa_multi_pairing, Engine::final_exponentiation (mod.rs:104-160): the
 * batch-verification shape e(P_1,Q_1)...e(P_n,Q_n).  ok = 0 iff the product
 * Miller value is zero (None).  The points may be any field elements, as for
 * pa_pairing_batch (a Q off E' costs what it costs there). */
int pa_multi_miller_loop_affine(const pa_g1_affine *p, const pa_g2_affine *q, size_t n, pa_fq12 *out);
int pa_multi_pairing(const pa_g1_affine *p, const pa_g2_affine *q, size_t n, pa_fq12 *out, uint8_t *ok);
/* m independent pa_multi_pairing products in one call -- a batch of signature
 * or proof checks: n Miller loops, a segmented product, m final
 * exponentiations.  `offsets` is CSR over the pairs, in host memory: m + 1
 * entries, offsets[0] == 0, non-decreasing, n = offsets[m]; product j covers
 * pairs [offsets[j], offsets[j+1]).  (out[j], ok[j]) are bit-identical to
 * pa_multi_pairing on that segment alone (an empty product is one with
 * ok = 1); is_one[j] = ok[j] && out[j] == one, the verifier's answer.  `out`
 * may be NULL if `is_one` is not (then only the 2 m flag bytes come back);
 * `is_one` may be NULL.  Offsets that are not CSR give PA_ERR_INVALID_ARGUMENT
 * before anything is launched.  m == 0 is a no-op. */
int pa_multi_pairing_batch(const pa_g1_affine *p, const pa_g2_affine *q, const uint64_t *offsets, size_t m,
                           pa_fq12 *out, uint8_t *ok, uint8_t *is_one);
/* pa_pairing_batch split over devices 0..ndev-1 of this process (contiguous
 * shards, one host thread per device); ndev <= pa_device_count.  The
 * environment variable PA_DEVICE_MAP (a comma list of device ordinals) maps
 * shard d to its d-th entry instead, e.g. "4,5,6,7"; then ndev <= its length. */
int pa_pairing_batch_multi_gpu(const pa_g1_affine *p, const pa_g2_affine *q, pa_fq12 *out, size_t n, int ndev);

/* ---- variable-base scalar multiplication and MSM (SURVEY.md §8 f, rank 3) ----
 * Scalars are FrRepr (canonical 4 x u64 LE; any 256-bit value, as the
 * reference's BitIterator takes).  Per-item outputs are Jacobian and equal
 * the reference's X, Y, Z words bit for bit. */
/* CurveAffine::mul, ec.rs:174-177 (mul_bits ec.rs:88-95): out[i] = s[i] * p[i] */
int pa_g1_affine_mul_batch(const pa_g1_affine *p, const pa_fr_repr *s, pa_g1 *out, size_t n);
int pa_g2_affine_mul_batch(const pa_g2_affine *p, const pa_fr_repr *s, pa_g2 *out, size_t n);
/* CurveProjective::mul_assign, ec.rs:534-553: out[i] = s[i] * p[i] (p Jacobian) */
int pa_g1_mul_assign_batch(const pa_g1 *p, const pa_fr_repr *s, pa_g1 *out, size_t n);
int pa_g2_mul_assign_batch(const pa_g2 *p, const pa_fr_repr *s, pa_g2 *out, size_t n);
/* Multi-scalar multiplication: *out = sum_i s[i] * bases[i] (Pippenger buckets
 * on the device), the prover's multiexp over CurveAffine::mul + add_assign.
 * The Jacobian result is equal as a point (PartialEq, ec.rs:45-85) to the
 * reference's sum; n = 0 gives the zero point.  n < 2^31. */
int pa_g1_multiexp(const pa_g1_affine *bases, const pa_fr_repr *s, size_t n, pa_g1 *out);
int pa_g2_multiexp(const pa_g2_affine *bases, const pa_fr_repr *s, size_t n, pa_g2 *out);
/* device workspace bytes for pa_g{1,2}_multiexp_device (group 1 or 2) */
size_t pa_multiexp_workspace_bytes(int group, size_t n);

/* ---- G1 multiexp over prepared bases ----
 * A prover's bases are its proving key: fixed across calls.  pa_g1_msm_bases
 * holds them on one device in the form the bucket accumulation gathers
 * (converted once, not per call) together with one flag: whether every base
 * passed the G1 membership test phi(P) == -[x^2] P at preparation (infinity
 * passes).  With the flag set, a multiexp splits each scalar s = q x^2 + rem
 * (integers, any 256-bit s) and sums rem P_i + q (-phi(P_i)) over half as many
 * windows; with it clear, the same 257-bit pipeline as pa_g1_multiexp runs over
 * the prepared rows and phi is never used.  Either way the result is equal as
 * a point (PartialEq, ec.rs:45-85) to the reference's sum of CurveAffine::mul
 * terms, for every 256-bit FrRepr (values >= r included).  Bases off the curve
 * are unspecified, as for pa_g1_multiexp.
 * Preparation runs once and synchronizes the stream; n < 2^30, n = 0 allowed.
 * The object is tied to the device it was prepared on (the current device, or
 * the stream's), may be used from any host thread, and lives until
 * pa_g1_msm_bases_free (NULL is a no-op); work that reads it must have
 * completed before it is freed. */
typedef struct pa_g1_msm_bases pa_g1_msm_bases;
int pa_g1_msm_bases_prepare(const pa_g1_affine *host_bases, size_t n, pa_g1_msm_bases **out);
int pa_g1_msm_bases_prepare_device(const pa_g1_affine *dev_bases, size_t n, void *stream, pa_g1_msm_bases **out);
size_t pa_g1_msm_bases_len(const pa_g1_msm_bases *bases);
int pa_g1_msm_bases_in_subgroup(const pa_g1_msm_bases *bases);   /* 1 or 0 */
int pa_g1_msm_bases_free(pa_g1_msm_bases *bases);
/* *out = sum_{i < m} s[i] * P_i over the first m <= len prepared bases; m = 0
 * gives the zero point.  Errors (m > len, a workspace smaller than
 * pa_g1_multiexp_prepared_workspace_bytes(bases, m), a stream on another
 * device than the object's) return a code before anything is launched. */
size_t pa_g1_multiexp_prepared_workspace_bytes(const pa_g1_msm_bases *bases, size_t m);
int pa_g1_multiexp_prepared_device(const pa_g1_msm_bases *bases, const pa_fr_repr *dev_scalars, size_t m,
                                   pa_g1 *dev_out, void *workspace, size_t workspace_bytes, void *stream);
int pa_g1_multiexp_prepared(const pa_g1_msm_bases *bases, const pa_fr_repr *host_scalars, size_t m, pa_g1 *out);
/* A batch of k scalar vectors over the same prepared bases, in one pipeline:
 *   out[j] = sum_{i < m} s[j * m + i] * P_i   for j < k,
 * the vectors end to end (the layout of pa_fr_ntt's `batch` polynomials), each
 * result equal as a point to pa_g1_multiexp_prepared over that vector.  k = 0
 * writes nothing and returns PA_OK; m = 0 writes k zero points.  k = 1 with
 * PA_MSM_SCALARS_REPR runs the job of pa_g1_multiexp_prepared_device.
 * flags: PA_MSM_SCALARS_REPR, rows are pa_fr_repr (any 256-bit value), or
 * PA_MSM_SCALARS_MONTGOMERY, rows are pa_fr (Montgomery, what pa_fr_ntt
 * writes) and are taken through into_repr on the device; in that mode the
 * result for a row that is not below r is unspecified.
 * Item positions and bucket keys are 32-bit.  With W windows of c bits and B =
 * 2^(c-1) buckets per window over nt terms (2m and 130 bits when the bases are
 * in the subgroup, else m and 257 bits), a batch is valid while k * W * nt <=
 * 2^32 - 1 and k * W * B < 2^32.  Beyond that ..._workspace_bytes returns 0
 * and the entries return PA_ERR_INVALID_ARGUMENT; the caller splits the batch.
 * Errors (m > len, unknown flag bits, a batch over the limit, a workspace
 * smaller than ..._batch_workspace_bytes(bases, m, k), a stream on another
 * device than the object's) return a code before anything is launched. */
#define PA_MSM_SCALARS_REPR        0u
#define PA_MSM_SCALARS_MONTGOMERY  1u
size_t pa_g1_multiexp_prepared_batch_workspace_bytes(const pa_g1_msm_bases *bases, size_t m, size_t k);
int pa_g1_multiexp_prepared_batch_device(const pa_g1_msm_bases *bases, const void *dev_scalars, size_t m, size_t k,
                                         unsigned flags, pa_g1 *dev_out, void *workspace, size_t workspace_bytes,
                                         void *stream);
int pa_g1_multiexp_prepared_batch(const pa_g1_msm_bases *bases, const void *host_scalars, size_t m, size_t k,
                                  unsigned flags, pa_g1 *out);

/* ---- G2 multiexp over prepared bases ----
 * The G1 block above, one for one, over pa_g2_affine bases and pa_g2 results:
 * the same object rules, error codes, flags, zero sizes (k = 0 writes
 * nothing, m = 0 writes k zero points) and 32-bit item limit, and one vector
 * with PA_MSM_SCALARS_REPR runs the job of pa_g2_multiexp_prepared_device.
 * The flag is the G2 membership test of pa_g2_subgroup_check_batch.  With it
 * set, the scalar splits s = q x^2 + rem as for G1 and the second half runs
 * over x^2 Q_i, which costs one Fq product per coordinate word: with beta the
 * cube root of unity of the G1 path and Q = (x, y) in G2,
 *     x^2 Q = (beta^2 x, -y)        (x = 0xd201000000010000; beta^2 scales
 *                                    both Fq components of the Fq2 coordinate)
 * and not (beta x, -y), which is the G1 relation and fails on G2.  With the
 * flag clear the 257-bit pipeline of pa_g2_multiexp runs over the prepared
 * rows; nothing is converted per call either way.  Results are equal as
 * points to the reference's sum for every 256-bit FrRepr. */
typedef struct pa_g2_msm_bases pa_g2_msm_bases;
int pa_g2_msm_bases_prepare(const pa_g2_affine *host_bases, size_t n, pa_g2_msm_bases **out);
int pa_g2_msm_bases_prepare_device(const pa_g2_affine *dev_bases, size_t n, void *stream, pa_g2_msm_bases **out);
size_t pa_g2_msm_bases_len(const pa_g2_msm_bases *bases);
int pa_g2_msm_bases_in_subgroup(const pa_g2_msm_bases *bases);   /* 1 or 0 */
int pa_g2_msm_bases_free(pa_g2_msm_bases *bases);
size_t pa_g2_multiexp_prepared_workspace_bytes(const pa_g2_msm_bases *bases, size_t m);
int pa_g2_multiexp_prepared_device(const pa_g2_msm_bases *bases, const pa_fr_repr *dev_scalars, size_t m,
                                   pa_g2 *dev_out, void *workspace, size_t workspace_bytes, void *stream);
int pa_g2_multiexp_prepared(const pa_g2_msm_bases *bases, const pa_fr_repr *host_scalars, size_t m, pa_g2 *out);
size_t pa_g2_multiexp_prepared_batch_workspace_bytes(const pa_g2_msm_bases *bases, size_t m, size_t k);
int pa_g2_multiexp_prepared_batch_device(const pa_g2_msm_bases *bases, const void *dev_scalars, size_t m, size_t k,
                                         unsigned flags, pa_g2 *dev_out, void *workspace, size_t workspace_bytes,
                                         void *stream);
int pa_g2_multiexp_prepared_batch(const pa_g2_msm_bases *bases, const void *host_scalars, size_t m, size_t k,
                                  unsigned flags, pa_g2 *out);

/* ---- scalar field Fr (src/bls12_381/fr.rs; SURVEY.md §8 f, rank 4) ----
 * pa_fr = 4 x u64 LE limbs, Montgomery form with R = 2^256, < r: the
 * reference's `Fr` in memory.  Every result is canonical, so it equals the
 * reference's bit for bit. */
int pa_fr_mul_batch(const pa_fr *a, const pa_fr *b, pa_fr *out, size_t n);  /* mul_assign fr.rs:438-465 */
int pa_fr_square_batch(const pa_fr *a, pa_fr *out, size_t n);              /* square fr.rs:467-500 */
int pa_fr_add_batch(const pa_fr *a, const pa_fr *b, pa_fr *out, size_t n);  /* add_assign fr.rs:341-348 */
int pa_fr_sub_batch(const pa_fr *a, const pa_fr *b, pa_fr *out, size_t n);  /* sub_assign fr.rs:359-367 */
int pa_fr_double_batch(const pa_fr *a, pa_fr *out, size_t n);              /* double fr.rs:350-357 */
int pa_fr_negate_batch(const pa_fr *a, pa_fr *out, size_t n);              /* negate fr.rs:369-375 */
/* inverse fr.rs:377-431; ok[i] = 0 (None) for zero */
int pa_fr_inverse_batch(const pa_fr *a, pa_fr *out, uint8_t *ok, size_t n);
/* PrimeField::from_repr fr.rs:279-288; ok[i] = 0 = Err(NotInField) when repr >= r (out[i] = 0) */
int pa_fr_from_repr_batch(const pa_fr_repr *repr, pa_fr *out, uint8_t *ok, size_t n);
/* PrimeField::into_repr fr.rs:290-303 */
int pa_fr_into_repr_batch(const pa_fr *a, pa_fr_repr *out, size_t n);
/* Field::pow lib.rs:306-324 with one exponent (exp_words u64, LE) for every element */
int pa_fr_pow_batch(const pa_fr *a, const uint64_t *exp, size_t exp_words, pa_fr *out, size_t n);
/* SqrtField::legendre fr.rs:575-590: out[i] = 0 Zero, 1 QuadraticResidue, -1 QuadraticNonResidue */
int pa_fr_legendre_batch(const pa_fr *a, int8_t *out, size_t n);
/* SqrtField::sqrt fr.rs:592-646 (the reference's Tonelli-Shanks root); ok[i] = 0 (None) for a non-residue */
int pa_fr_sqrt_batch(const pa_fr *a, pa_fr *out, uint8_t *ok, size_t n);

/* ---- batched Fr NTT: radix-2 evaluation domains ----
 * For n = 2^log_n: w = ROOT_OF_UNITY^(2^(32 - log_n)) (fr.rs:51-56), g = 7 the
 * GENERATOR (fr.rs:41-46); rows are Montgomery pa_fr, natural order in and out:
 *   PA_NTT_FORWARD        out[j] = sum_i in[i] w^(ij)
 *   PA_NTT_INVERSE        out[j] = n^-1 sum_i in[i] w^(-ij)
 *   PA_NTT_COSET_FORWARD  forward of in[i] g^i
 *   PA_NTT_COSET_INVERSE  inverse, then out[i] g^-i
 * the fft / ifft / coset_fft / icoset_fft of a prover's evaluation domain.
 * Results are canonical, so they equal any correct transform bit for bit.
 * `batch` polynomials of n rows each are transformed per call, polynomial b in
 * rows b n .. b n + n - 1; batch = 0 is a no-op and log_n = 0 the identity.
 *
 * A domain owns the power tables of its size on the device that was current
 * at creation (creation builds them there and waits for that).  log_n up to
 * PA_NTT_MAX_LOG_N = 28 (pa_fr_ntt_max_log_n()); above it creation returns
 * PA_ERR_INVALID_ARGUMENT.  The environment variable PA_NTT_TILE_LOG (1..12,
 * clamped, default 10; a value that is not a number leaves the default) is
 * read at creation: a transform runs as ceil(log_n / tile_log) passes over HBM,
 * one launch each.  A pass may have at most 2^24 - 1 workgroups: with the
 * default tile log (2^11 rows per workgroup) that allows batch * 2^log_n just
 * under 2^35 rows, with tile logs 1 and 2 (measurement only; as few as 4 and 8
 * rows per workgroup) 2^26 and 2^27; a larger batch is refused.  The object may be
 * used from any host thread and lives until pa_fr_ntt_domain_free (NULL is a
 * no-op); work that reads it must have completed before it is freed.
 *
 * in == out (in place) is allowed; with in != out the input is only read.
 * A NULL domain, an unknown mode, input and output that overlap partly, a
 * workspace smaller than pa_fr_ntt_workspace_bytes(d, batch) (which is linear
 * in batch and 0 for a one-pass domain), or a stream on another device than
 * the domain's return a code before anything is launched.  The workspace must
 * not overlap in or out.  pa_fr_ntt_device allocates nothing, does not
 * synchronize, reads nothing back and can be captured into a HIP graph. */
#define PA_NTT_FORWARD 0
#define PA_NTT_INVERSE 1
#define PA_NTT_COSET_FORWARD 2
#define PA_NTT_COSET_INVERSE 3
#define PA_NTT_MAX_LOG_N 28
typedef struct pa_fr_ntt_domain pa_fr_ntt_domain;
int pa_fr_ntt_domain_create(unsigned log_n, pa_fr_ntt_domain **out);
void pa_fr_ntt_domain_free(pa_fr_ntt_domain *d);
unsigned pa_fr_ntt_domain_log_n(const pa_fr_ntt_domain *d);
size_t pa_fr_ntt_domain_bytes(const pa_fr_ntt_domain *d);   /* device memory it holds */
unsigned pa_fr_ntt_domain_passes(const pa_fr_ntt_domain *d);     /* launches per transform (0 for log_n = 0) */
unsigned pa_fr_ntt_domain_tile_log(const pa_fr_ntt_domain *d);   /* PA_NTT_TILE_LOG as clamped */
/* polynomials that share a workgroup in a one-pass domain (2^11 rows per
 * workgroup, 2^12 at tile log 12: 2^(11 - log_n)); 0 for a domain of several passes */
size_t pa_fr_ntt_polys_per_workgroup(const pa_fr_ntt_domain *d);
unsigned pa_fr_ntt_max_log_n(void);
size_t pa_fr_ntt_workspace_bytes(const pa_fr_ntt_domain *d, size_t batch);
int pa_fr_ntt(const pa_fr_ntt_domain *d, int mode, const pa_fr *in, pa_fr *out, size_t batch);   /* host memory */
int pa_fr_ntt_device(const pa_fr_ntt_domain *d, int mode, const pa_fr *in, pa_fr *out, size_t batch,
                     void *workspace, size_t workspace_bytes, void *stream);

/* The quotient of a Groth16 proof over the domain: from the evaluations of A, B
 * and C the coefficients of h = (A B - C) / Z, Z = X^n - 1, as
 *   h_j = coset_inverse( (coset_forward(inverse(a_j)) * coset_forward(inverse(b_j))
 *                         - coset_forward(inverse(c_j))) * (g^n - 1)^-1 )
 * for each of `batch` triples: a, b and c are three arrays laid out as the
 * transforms lay out polynomials, out gets n Montgomery coefficient rows per
 * polynomial, canonical, natural order, bit-identical to that composition of
 * pa_fr_ntt, pa_fr_mul_batch and pa_fr_sub_batch (for any input; where c = a * b
 * on the domain, row n - 1 is zero).  It runs as 3 x passes launches: a pass of
 * the first two transforms covers a, b and c in one grid, the last transform
 * forms A B - C as it loads, and the inverse transforms' n^-1 and 1 / Z ride on
 * the coset factors of a's and c's forward transforms (two multiplications
 * per point fewer than the seven transforms on their own).
 * log_n = 0 is one elementwise launch of (a b - c) / 6.
 *
 * out may be exactly a, b or c; a, b and c may be one another (a == b gives
 * a^2 - c); inputs that out does not alias are only read.  A NULL domain, a
 * NULL pointer with batch > 0, out overlapping an input partly, a workspace
 * smaller than pa_fr_ntt_quotient_workspace_bytes(d, batch), or a stream on
 * another device return a code before anything is launched; batch = 0 is a
 * no-op.  The workspace is 3 batch n 32 bytes for a one-pass domain (the coset
 * evaluations), 6 batch n 32 for several passes, 0 for log_n = 0, and must not
 * overlap a, b, c or out.  The query returns 0 for a NULL domain and when the
 * 3 batch polynomials of a pass do not fit a grid: the entries then return
 * PA_ERR_INVALID_ARGUMENT and the caller splits the batch.  The device entry
 * allocates nothing, does not synchronize, reads nothing back and can be
 * captured into a HIP graph (one chain of launches). */
size_t pa_fr_ntt_quotient_workspace_bytes(const pa_fr_ntt_domain *d, size_t batch);
int pa_fr_ntt_quotient(const pa_fr_ntt_domain *d, const pa_fr *a, const pa_fr *b, const pa_fr *c, pa_fr *out,
                       size_t batch);   /* host memory */
int pa_fr_ntt_quotient_device(const pa_fr_ntt_domain *d, const pa_fr *a, const pa_fr *b, const pa_fr *c, pa_fr *out,
                              size_t batch, void *workspace, size_t workspace_bytes, void *stream);

/* ---- R1CS matrices on the device: A w, B w, C w over the domain ----
 * The three arrays the quotient takes are the products of a constraint
 * system's matrices with the witness.  pa_r1cs holds the three matrices on one
 * device; an evaluation multiplies them with k witnesses in one call.
 *   witness: k vectors of n_cols Montgomery pa_fr rows, end to end;
 *   a, b, c: k polynomials of n = 2^log_n rows each, end to end (the layout
 *            of pa_fr_ntt and pa_fr_ntt_quotient); for witness j and i < n_rows
 *            a[j n + i] = sum_t val[t] w_j[col[t]] over row i of A, likewise b
 *            and c; rows n_rows .. n - 1 are written as zero.
 * Every value is canonical, so the results are bit-exact whatever the order of
 * summation.  A column may occur more than once in a row (the terms add); empty
 * rows, an empty matrix, n_rows = 0, k = 0 (writes nothing) and log_n = 0 are
 * valid.  A witness row that is not below r is undefined.
 *
 * Creation copies the matrices (host CSR) into a device image and waits for
 * the copy; the host arrays may be released afterwards.  It cuts every row into
 * chunks of at most pa_r1cs_chunk_len() terms: one lane sums one chunk, a row of
 * one chunk stores its sum, a row of several gets its partial sums added by a
 * second, small launch (no atomics), so a row of thousands of terms among rows
 * of one to three does not set the kernel's time.  Errors at creation
 * (PA_ERR_INVALID_ARGUMENT, nothing allocated): row_ptr[0] != 0 or decreasing,
 * a column >= n_cols, a value >= r, nnz >= 2^32 in one matrix, n_rows >
 * 2^PA_NTT_MAX_LOG_N.  The object belongs to the device that was current at
 * creation, may be used from any host thread and lives until pa_r1cs_free (NULL
 * is a no-op); work that reads it must have completed before it is freed.
 *
 * Errors at evaluation (PA_ERR_INVALID_ARGUMENT, before any launch): 2^log_n <
 * n_rows, log_n > PA_NTT_MAX_LOG_N, a workspace smaller than
 * pa_r1cs_eval_workspace_bytes(r, k) (k times 32 bytes per chunk of the rows of
 * several chunks; 0 if there are none, then workspace may be NULL), a stream on
 * another device than the object's.  a, b, c, the witness and the workspace
 * must not overlap.  The device entry allocates nothing, does not synchronize
 * and reads nothing back. */
typedef struct pa_r1cs pa_r1cs;
/* host CSR: row_ptr[n_rows + 1] (row_ptr[0] = 0, non-decreasing), col[nnz] < n_cols, val[nnz] Montgomery pa_fr < r */
typedef struct { const uint64_t *row_ptr; const uint32_t *col; const pa_fr *val; } pa_fr_csr;
int pa_r1cs_create(const pa_fr_csr *a, const pa_fr_csr *b, const pa_fr_csr *c, size_t n_rows, size_t n_cols,
                   pa_r1cs **out);
void pa_r1cs_free(pa_r1cs *r);
size_t pa_r1cs_rows(const pa_r1cs *r);
size_t pa_r1cs_cols(const pa_r1cs *r);
size_t pa_r1cs_bytes(const pa_r1cs *r);   /* device memory it holds */
size_t pa_r1cs_chunk_len(void);
size_t pa_r1cs_eval_workspace_bytes(const pa_r1cs *r, size_t k);
int pa_r1cs_eval_device(const pa_r1cs *r, const pa_fr *dev_witness, size_t k, unsigned log_n, pa_fr *a, pa_fr *b,
                        pa_fr *c, void *workspace, size_t workspace_bytes, void *stream);
int pa_r1cs_eval(const pa_r1cs *r, const pa_fr *host_witness, size_t k, unsigned log_n, pa_fr *a, pa_fr *b,
                 pa_fr *c);   /* host memory */

/* ---- Groth16 prover: witness in, proof out, k proofs per call ----
 * The proving key as one object on one device (the current one at creation),
 * built on pa_g{1,2}_msm_bases_prepare.  n_public counts the constant one:
 * variables [0, n_public) have no L entry.  The L query is stored with n_public
 * points at infinity in front and the H query with points at infinity up to
 * 2^log_n, so the multiexps read the witness at stride n_vars and the quotient
 * at stride n as they lie (a consequence: the top row of h, nonzero only for an
 * unsatisfied witness, meets infinity when h_len < n and drops out, as it does
 * in bellman, which gives h_len = n - 1).  Creation fails with
 * PA_ERR_INVALID_ARGUMENT for n_public > n_vars, h_len > 2^log_n or log_n >
 * PA_NTT_MAX_LOG_N.  pa_groth16_pk_in_subgroup is 1 if all five query sets
 * passed their membership test (the multiexps then take the GLV path); the
 * proof is the same either way.  alpha, beta and delta are not tested: alpha,
 * beta and the query points may be any curve points, infinity included, and
 * the proof is bit-exact for them, but delta_g1 / delta_g2 outside G1/G2 are
 * undefined for the prover (the assembly forms C from s A0 + r B0 + (r s) delta
 * with A0 = A - r delta_g1, B0 = B1 - s delta_g1 and r s reduced mod the group
 * order, which is the formula below only for a delta whose order divides it;
 * no verifier could use another key).  For delta the key also holds
 * 2^i delta, i < 255, in both groups (109 KiB), which the assembly sums instead
 * of doubling.
 *
 * pa_groth16_prove*: for proof j with witness w (n_vars rows), z = n_public, h
 * the n rows of pa_fr_ntt_quotient over pa_r1cs_eval of w, and r, s its
 * blinding scalars (one Montgomery row each per proof, supplied by the caller)
 *   A  = alpha_g1 + sum_i w_i a_query[i]    + r delta_g1
 *   B  = beta_g2  + sum_i w_i b_g2_query[i] + s delta_g2
 *   B1 = beta_g1  + sum_i w_i b_g1_query[i] + s delta_g1
 *   C  = sum_{i >= z} w_i l_query[i - z] + sum_i h_i h_query[i] + s A + r B1 - (r s) delta_g1
 * (bellman's create_proof), written as the affine records that
 * pa_g{1,2}_into_affine_batch write for those points, infinity included:
 * affine coordinates are canonical, so a proof is bit-exact.  The device entry
 * runs pa_r1cs_eval_device, pa_fr_ntt_quotient_device, four G1 and one G2
 * pa_g*_multiexp_prepared_batch_device with PA_MSM_SCALARS_MONTGOMERY and one
 * assembly kernel on `stream`: it allocates nothing, forks no stream and does
 * not synchronize.  The workspace holds a, b, c, the five sums and one region
 * that the steps use one after the other; ..._workspace_bytes returns 0 when
 * the batch is over a multiexp's 32-bit item limit or the quotient's grid
 * limit, and the entries then return PA_ERR_INVALID_ARGUMENT: split the batch.
 * Errors, all PA_ERR_INVALID_ARGUMENT before anything runs: the domain's log_n
 * differs from the key's, pa_r1cs_cols(r1cs) != n_vars, pa_r1cs_rows(r1cs) >
 * 2^log_n, objects or stream on different devices, a batch over the limit, a
 * workspace that is too small.  k = 0 writes nothing.  A witness, r or s row
 * that is not below r is undefined. */
typedef struct {
    pa_g1_affine alpha_g1, beta_g1, delta_g1;
    pa_g2_affine beta_g2, delta_g2;
    size_t n_vars, n_public;
    const pa_g1_affine *a_query, *b_g1_query;   /* n_vars each; infinity where a variable does not occur */
    const pa_g2_affine *b_g2_query;             /* n_vars */
    const pa_g1_affine *l_query;                /* n_vars - n_public */
    const pa_g1_affine *h_query;                /* h_len <= 2^log_n */
    size_t h_len;
} pa_groth16_key;   /* host memory */
typedef struct pa_groth16_pk pa_groth16_pk;
typedef struct { pa_g1_affine a; pa_g2_affine b; pa_g1_affine c; } pa_groth16_proof;   /* 51 u64 */
int pa_groth16_pk_create(const pa_groth16_key *key, unsigned log_n, pa_groth16_pk **out);
void pa_groth16_pk_free(pa_groth16_pk *pk);   /* NULL is a no-op */
int pa_groth16_pk_in_subgroup(const pa_groth16_pk *pk);
size_t pa_groth16_prove_workspace_bytes(const pa_groth16_pk *pk, const pa_r1cs *r1cs, size_t k);
int pa_groth16_prove_device(const pa_groth16_pk *pk, const pa_r1cs *r1cs, const pa_fr_ntt_domain *d,
                            const pa_fr *dev_witness, const pa_fr *dev_r, const pa_fr *dev_s, size_t k,
                            pa_groth16_proof *dev_proofs, void *workspace, size_t workspace_bytes, void *stream);
int pa_groth16_prove(const pa_groth16_pk *pk, const pa_r1cs *r1cs, const pa_fr_ntt_domain *d,
                     const pa_fr *host_witness, const pa_fr *host_r, const pa_fr *host_s, size_t k,
                     pa_groth16_proof *proofs);   /* host memory */

/* ---- Groth16 parameter generation: trapdoor in, keys out ----
 * bellman's generate_parameters for a trapdoor (tau, alpha, beta, gamma, delta)
 * that the caller sampled, over base points g1 and g2.  With n = 2^log_n the
 * domain's size, L_j(tau) its Lagrange coefficients at tau, variable i in
 * [0, n_vars) and n_public counting the constant one:
 *   u_i = sum_j A[j][i] L_j(tau)   v_i = sum_j B[j][i] L_j(tau)   w_i = sum_j C[j][i] L_j(tau)
 *   mix_i = (beta u_i + alpha v_i + w_i) / gamma   for i <  n_public   (ic[i])
 *   mix_i = (beta u_i + alpha v_i + w_i) / delta   for i >= n_public   (l_query[i - n_public])
 *   h_i   = tau^i (tau^n - 1) / delta              for i <  n - 1      (h_query, h_len = n - 1)
 *   a_query[i] = u_i g1   b_g1_query[i] = v_i g1   b_g2_query[i] = v_i g2
 *   alpha_g1, beta_g1, delta_g1 = alpha g1, beta g1, delta g1
 *   beta_g2, gamma_g2, delta_g2 = beta g2, gamma g2, delta g2
 * L is the inverse transform of the powers 1, tau, .., tau^(n-1), L_j = n^-1
 * sum_i tau^i w^(-ij): no inversion, right for every tau (tau = w^m gives L_m = 1,
 * the other L_j = 0 and every h_i = 0; tau = 0 gives L_j = n^-1).  The outputs
 * are the affine records pa_g{1,2}_into_affine_batch write, so they are
 * bit-exact; a zero scalar gives the record of the point at infinity, e.g.
 * a_query[i] for a variable that occurs in no row of A.  The query arrays stay
 * dense (bellman's filtering of zero points and its density trackers are not
 * reproduced).  The matrices are taken as given: bellman's extra rows
 * input_i * 0 = 0 are the caller's to include.  g1 and g2 may be any on-curve
 * points, infinity included; off-curve bases are undefined.
 *
 * pa_groth16_circuit holds the transposed matrices (rows = variables, columns =
 * constraints) as a pa_r1cs image on the device current at creation, so a
 * variable of thousands of occurrences (the constant one) is a row of many
 * chunks there.  Creation errors are those of pa_r1cs_create, plus n_public >
 * n_cols and n_cols > 2^PA_NTT_MAX_LOG_N.  Lifetime rules as for pa_r1cs.
 *
 * Output layout (pa_groth16_generate_offsets returns it; a pa_groth16_key and a
 * pa_groth16_vkey can point straight into the arrays):
 *   g1_out = a_query (n_vars) | b_g1_query (n_vars) | ic (n_public) | l_query (n_vars - n_public)
 *            | h_query (n - 1) | alpha_g1 | beta_g1 | delta_g1          3 n_vars + n + 2 records
 *   g2_out = b_g2_query (n_vars) | beta_g2 | gamma_g2 | delta_g2       n_vars + 3 records
 * pa_groth16_generate_scalars* write the discrete logarithms of g1_out in the
 * same order as Montgomery rows (the last three are alpha, beta, delta): the Fr
 * half of the call without any curve arithmetic.
 *
 * The trapdoor is host memory in every entry (160 bytes; it travels as kernel
 * arguments).  The device entries take device pointers, run in stream order on
 * `stream` (the G1 multiply orders its side streams with events, as
 * pa_g1_wnaf_fixed_base_device does), allocate nothing and read nothing back:
 * a powers kernel, pa_fr_ntt_device (inverse), the chunked product of the
 * transposed image with L, a scalar kernel, one pa_g1_wnaf_fixed_base_device
 * and one pa_g2_wnaf_fixed_base_device over the whole vectors, the two batch
 * normalizations and a pack kernel each.  workspace:
 * pa_groth16_generate_workspace_bytes(circuit, log_n) bytes for either device
 * entry (0 for a NULL circuit or 2^log_n < rows).  Errors, all
 * PA_ERR_INVALID_ARGUMENT before anything runs: a NULL pointer, 2^log_n < rows
 * (log_n is the domain's), a trapdoor value >= r, gamma = 0 or delta = 0
 * (bellman's UnexpectedIdentity), circuit, domain and stream on different
 * devices, a workspace that is too small. */
typedef struct pa_groth16_circuit pa_groth16_circuit;
typedef struct { pa_fr tau, alpha, beta, gamma, delta; } pa_groth16_trapdoor;   /* host memory, Montgomery, < r */
typedef struct {
    size_t a_query, b_g1_query, ic, l_query, h_query, alpha_g1, beta_g1, delta_g1, g1_len;   /* records into g1_out */
    size_t b_g2_query, beta_g2, gamma_g2, delta_g2, g2_len;                                  /* records into g2_out */
    size_t h_len;                                                                            /* n - 1 */
} pa_groth16_generate_layout;
static inline pa_groth16_generate_layout pa_groth16_generate_offsets(size_t n_vars, size_t n_public, unsigned log_n) {
    pa_groth16_generate_layout o;
    o.h_len = ((size_t)1 << log_n) - 1;
    o.a_query = 0;
    o.b_g1_query = n_vars;
    o.ic = 2 * n_vars;
    o.l_query = 2 * n_vars + n_public;
    o.h_query = 3 * n_vars;
    o.alpha_g1 = o.h_query + o.h_len;
    o.beta_g1 = o.alpha_g1 + 1;
    o.delta_g1 = o.alpha_g1 + 2;
    o.g1_len = o.alpha_g1 + 3;
    o.b_g2_query = 0;
    o.beta_g2 = n_vars;
    o.gamma_g2 = n_vars + 1;
    o.delta_g2 = n_vars + 2;
    o.g2_len = n_vars + 3;
    return o;
}
int pa_groth16_circuit_create(const pa_fr_csr *a, const pa_fr_csr *b, const pa_fr_csr *c, size_t n_rows, size_t n_cols,
                              size_t n_public, pa_groth16_circuit **out);
void pa_groth16_circuit_free(pa_groth16_circuit *circuit);   /* NULL is a no-op */
size_t pa_groth16_circuit_rows(const pa_groth16_circuit *circuit);
size_t pa_groth16_circuit_cols(const pa_groth16_circuit *circuit);       /* n_vars */
size_t pa_groth16_circuit_n_public(const pa_groth16_circuit *circuit);
size_t pa_groth16_circuit_bytes(const pa_groth16_circuit *circuit);      /* device memory it holds */
size_t pa_groth16_generate_g1_len(const pa_groth16_circuit *circuit, unsigned log_n);   /* 3 n_vars + n + 2 */
size_t pa_groth16_generate_g2_len(const pa_groth16_circuit *circuit);                   /* n_vars + 3 */
size_t pa_groth16_generate_workspace_bytes(const pa_groth16_circuit *circuit, unsigned log_n);
int pa_groth16_generate_device(const pa_groth16_circuit *circuit, const pa_fr_ntt_domain *d,
                               const pa_g1_affine *dev_g1, const pa_g2_affine *dev_g2,
                               const pa_groth16_trapdoor *host_trapdoor, pa_g1_affine *dev_g1_out,
                               pa_g2_affine *dev_g2_out, void *workspace, size_t workspace_bytes, void *stream);
int pa_groth16_generate(const pa_groth16_circuit *circuit, const pa_fr_ntt_domain *d, const pa_g1_affine *g1,
                        const pa_g2_affine *g2, const pa_groth16_trapdoor *trapdoor, pa_g1_affine *g1_out,
                        pa_g2_affine *g2_out);   /* host memory */
int pa_groth16_generate_scalars_device(const pa_groth16_circuit *circuit, const pa_fr_ntt_domain *d,
                                       const pa_groth16_trapdoor *host_trapdoor, pa_fr *dev_out, void *workspace,
                                       size_t workspace_bytes, void *stream);
int pa_groth16_generate_scalars(const pa_groth16_circuit *circuit, const pa_fr_ntt_domain *d,
                                const pa_groth16_trapdoor *trapdoor, pa_fr *out);   /* host memory */

/* ---- Groth16 verifier: k proofs per call over a prepared verifying key ----
 * bellman's prepare_verifying_key and verify_proof.  For proof j with public
 * inputs x_1 .. x_l, l = n_public - 1 (n_public counts the constant one, as in
 * pa_groth16_key):
 *   acc_j   = ic[0] + sum_{i = 1..l} x_{j,i} ic[i]
 *   gt_j    = final_exponentiation(ML(A_j, B_j) ML(acc_j, -gamma) ML(C_j, -delta))
 *   valid_j = (the final exponentiation is not None) && gt_j == e(alpha, beta)
 * gt and valid are canonical, so they are bit-exact whichever kernels run.
 *
 * The key object lives on the device that was current at creation.  It holds
 * e(alpha, beta), -gamma and -delta as affine and as pa_g2_prepared records,
 * ic[0], and for each of ic[1..l] one fixed-base comb table
 * (pa_g1_fixed_base_table_words() u64, about 0.49 MB; exact digits), and for
 * the aggregate check below two more tables (ic[0], alpha) and -beta.  l is at
 * most PA_GROTH16_VK_MAX_INPUTS (the l + 2 tables then take 251 MB); creation above
 * it, with n_public == 0 or with a NULL pointer returns
 * PA_ERR_INVALID_ARGUMENT.  Creation waits for the tables.  alpha, beta, gamma
 * and delta are taken as they are (no curve or subgroup test).  ic points may
 * be the point at infinity, and may lie on the curve outside G1: the comb
 * assumes no subgroup and no order.  The table holds d ic[i] for d <= 128;
 * for an ic point of order below 129 (E(Fq) has such points, of order 3, 11,
 * 33 and 121, none of them in G1) some of these are the identity, which the
 * table marks and the sum skips, so the sum is the reference's for them too.
 * ic points off the curve are undefined.  The object may be used from any host thread and lives
 * until pa_groth16_vk_free (NULL is a no-op); work that reads it must have
 * completed before it is freed.
 *
 * Inputs are rows of 4 u64: pa_fr_repr with PA_MSM_SCALARS_REPR, pa_fr
 * (Montgomery, the prover's witness format) with PA_MSM_SCALARS_MONTGOMERY.
 * Row i of proof j is inputs[j * input_stride + i], i < l, input_stride >= l:
 * with inputs = witness + 1 and input_stride = n_vars the proofs of
 * pa_groth16_prove_device are verified from the witness buffer as it lies.  A
 * row that is not below r is undefined.  With l = 0 inputs may be NULL.
 *
 * pa_groth16_vk_input_sum*: acc_j alone, k affine records (what into_affine
 * gives for the reference's sum, infinity included).
 *
 * pa_groth16_verify*: proofs are the 51-word records the prover writes; the
 * points are taken as they are, like pa_pairing_batch takes its points.
 * valid: k bytes, 1 or 0.  gt may be NULL; where the final exponentiation is
 * None, gt_j is a zero record and valid_j = 0.
 *
 * pa_groth16_verify_encoded*: k records of 192 bytes, A (48), B (96) and C
 * (48) compressed as bellman's Proof::write lays them out, through the checked
 * decoders (pa_g{1,2}_decode_batch, compressed = 1, checked = 1).  status: 3 k
 * bytes, the PA_DECODE_* codes of A, B and C of proof j at status[3 j ..
 * 3 j + 2].  A proof with a nonzero status has valid = 0; its gt is what the
 * chain gives for the decoders' output (the point at infinity for a failed
 * record) and is meaningful only where all three statuses are PA_DECODE_OK.
 *
 * The device entries take device pointers, enqueue everything on `stream`,
 * allocate nothing (the generated kernels' workspace pool is theirs), stage
 * nothing from the host and do not synchronize.  Up to
 * PA_GROTH16_VERIFY_SHARED_MIN - 1 proofs all 3 k pairs run through the
 * e(P, Q) Miller loops against the affine -gamma and -delta (the cooperative
 * and lane-group kernels then serve a small batch); from there on (acc, -gamma)
 * and (C, -delta) run on the shared-prepared Miller loop, which does no G2
 * arithmetic per pair but is one launch of one lane per pairing for each of
 * the two points (measured: slower at 32768 proofs, faster at 65536, nothing
 * between; profiles/groth16_verify/).  The environment variable
 * PA_G16V_SHARED_MIN overrides the bound (read at every call; tests and
 * measurements).  The workspace begins with the P array (3 k pa_g1_affine:
 * A | acc | C) and, at the next multiple of 256 bytes, the Q array (3 k
 * pa_g2_affine: B, then -gamma and -delta k times each, which only the
 * 3 k-pair path writes); the rest is scratch.  workspace:
 * pa_groth16_verify_workspace_bytes(vk, k) bytes for either verify entry
 * (monotone in k; 0 for a NULL key or k above PA_GROTH16_VERIFY_MAX_BATCH, which
 * the entries refuse: split the batch), pa_groth16_vk_input_sum_workspace_bytes
 * for the sum alone (k l Jacobian records; with l = 0 workspace may be NULL).
 * Errors, all PA_ERR_INVALID_ARGUMENT before anything runs: a NULL pointer,
 * input_stride < l, unknown flag bits, key and stream on different devices, a
 * batch over the limit, a workspace that is too small.  k = 0 writes nothing. */
#define PA_GROTH16_VK_MAX_INPUTS 512
#define PA_GROTH16_VERIFY_MAX_BATCH ((size_t)1 << 24)
#define PA_GROTH16_VERIFY_SHARED_MIN 65536
#define PA_GROTH16_ENCODED_PROOF_BYTES 192
typedef struct {
    pa_g1_affine alpha_g1;
    pa_g2_affine beta_g2, gamma_g2, delta_g2;
    const pa_g1_affine *ic;   /* n_public records */
    size_t n_public;
} pa_groth16_vkey;   /* host memory */
typedef struct pa_groth16_vk pa_groth16_vk;
int pa_groth16_vk_create(const pa_groth16_vkey *key, pa_groth16_vk **out);
void pa_groth16_vk_free(pa_groth16_vk *vk);   /* NULL is a no-op */
size_t pa_groth16_vk_n_public(const pa_groth16_vk *vk);
size_t pa_groth16_vk_bytes(const pa_groth16_vk *vk);   /* device memory it holds */
size_t pa_groth16_vk_input_sum_workspace_bytes(const pa_groth16_vk *vk, size_t k);
int pa_groth16_vk_input_sum_device(const pa_groth16_vk *vk, const pa_fr *dev_inputs, size_t input_stride,
                                   unsigned flags, size_t k, pa_g1_affine *dev_out, void *workspace,
                                   size_t workspace_bytes, void *stream);
int pa_groth16_vk_input_sum(const pa_groth16_vk *vk, const pa_fr *host_inputs, size_t input_stride, unsigned flags,
                            size_t k, pa_g1_affine *out);   /* host memory */
size_t pa_groth16_verify_workspace_bytes(const pa_groth16_vk *vk, size_t k);
int pa_groth16_verify_device(const pa_groth16_vk *vk, const pa_groth16_proof *dev_proofs, const pa_fr *dev_inputs,
                             size_t input_stride, unsigned flags, size_t k, uint8_t *dev_valid, pa_fq12 *dev_gt,
                             void *workspace, size_t workspace_bytes, void *stream);
int pa_groth16_verify(const pa_groth16_vk *vk, const pa_groth16_proof *proofs, const pa_fr *inputs,
                      size_t input_stride, unsigned flags, size_t k, uint8_t *valid, pa_fq12 *gt);   /* host memory */
int pa_groth16_verify_encoded_device(const pa_groth16_vk *vk, const uint8_t *dev_enc, const pa_fr *dev_inputs,
                                     size_t input_stride, unsigned flags, size_t k, uint8_t *dev_valid,
                                     uint8_t *dev_status, pa_fq12 *dev_gt, void *workspace, size_t workspace_bytes,
                                     void *stream);
int pa_groth16_verify_encoded(const pa_groth16_vk *vk, const uint8_t *enc, const pa_fr *inputs, size_t input_stride,
                              unsigned flags, size_t k, uint8_t *valid, uint8_t *status,
                              pa_fq12 *gt);   /* host memory */

/* ---- Groth16 aggregate check: k proofs in one randomised pairing product ----
 * bellman's verify_proofs_batch over a pa_groth16_vk.  With weights z_j (any
 * 128-bit integers; draw them from a cryptographic generator, fresh per call
 * and unknown to whoever made the proofs):
 *   s_0     = sum_j z_j mod r,   s_{i+1} = sum_j z_j x_{j,i} mod r   (i < l)
 *   A'_j    = into_affine(z_j A_j)
 *   accS    = into_affine(s_0 ic[0] + sum_i s_{i+1} ic[i+1])
 *   CS      = into_affine(sum_j z_j C_j)
 *   alphaS  = into_affine(s_0 alpha)
 *   gt      = final_exponentiation(prod_j ML(A'_j, B_j) ML(accS, -gamma)
 *                                  ML(CS, -delta) ML(alphaS, -beta))
 *   valid   = (the final exponentiation is not None) && gt == Fq12::one
 * k + 3 Miller loops (one launch) and one final exponentiation, against 3 k
 * and k of pa_groth16_verify.  One verdict for the batch: when it is 0, run
 * pa_groth16_verify on the same proofs to find the bad ones.  The two entries
 * compute different things, so neither falls back to the other.  Measured on
 * one MI355X (profiles/groth16_verify_aggregate/, l = 4): up to 2^10 proofs
 * pa_groth16_verify_device is the faster call (k = 1: 2.4 ms against 4.6;
 * 2^10: 5.6 against 7.5 -- the G1 side costs 3 to 4.6 ms at any k), at 2^14
 * and above this one is (2^14: 10.2 ms against 12.3, 15.9 at l = 32; 2^16:
 * 19.6 against 29.1); nothing between 2^10 and 2^14 was measured.
 *
 * When every A_j and C_j is in G1 and every B_j in G2, bilinearity gives
 * gt = prod_j (gt_j / e(alpha, beta))^z_j with gt_j of pa_groth16_verify: all
 * proofs valid gives one, and a batch with an invalid proof gives one with
 * probability about 2^-128 over random z.  Both statements need subgroup
 * membership.  pa_groth16_verify_aggregate and _points take the points as they
 * are, like every records entry; pa_groth16_verify_aggregate_encoded enforces
 * membership through the checked decoders.  z_j = 0 drops proof j from the
 * check.  No scalar multiplication here uses the endomorphism: z P and the
 * sums are the group law of E(Fq), well defined for any on-curve point, points
 * of small order included; points off the curve are undefined.  FrRepr inputs
 * are taken mod r; a Montgomery row not below r is undefined.
 *
 * z: k rows of two u64, little-endian (on the device 16-byte aligned, like
 * the scalars of pa_g1_multiexp_u128_device: a pointer that is not is
 * refused with PA_ERR_INVALID_ARGUMENT).  valid: one byte.  gt: one pa_fq12 or
 * NULL; where the final exponentiation is None it is zeroed and valid = 0.
 * _encoded: records and statuses as pa_groth16_verify_encoded (3 k status
 * bytes, per proof); any nonzero status forces valid = 0.  _points: the P
 * array alone, k + 3 affine records A'_0 .. A'_{k-1} | accS | CS | alphaS.
 * k = 0: valid = 1, gt = one, nothing else is launched or written (_points
 * writes three points at infinity).
 *
 * pa_groth16_vk_create builds for these entries two more comb tables (ic[0]
 * and alpha, any on-curve point) and the affine -beta; pa_groth16_vk_bytes
 * counts them.  The device entries follow pa_groth16_verify_device: device
 * pointers, everything on `stream` (the MSM orders its side streams with
 * events), no allocation, no staging, no synchronisation, the same errors
 * (PA_ERR_INVALID_ARGUMENT before anything runs).  workspace:
 * pa_groth16_verify_aggregate_workspace_bytes(vk, k) bytes for all three
 * (never 0 for a key, also at k = 0; monotone in k; 0 for a NULL key or k
 * above PA_GROTH16_VERIFY_MAX_BATCH).  It begins with the P array and, at the
 * next multiple of 256 bytes, the Q array (k + 3 pa_g2_affine: B_0 .. |
 * -gamma | -delta | -beta).
 *
 * pa_g1_multiexp_u128*: sum_i s_i P_i for 128-bit scalars (rows of two u64,
 * little-endian) over per-call bases, a Jacobian record: the same point as
 * pa_g1_multiexp over the zero-extended scalars, for any on-curve bases (no
 * endomorphism, no membership assumption), in ceil(130 / c) windows instead of
 * ceil(257 / c).  n < 2^31; n = 0 gives zero.
 * pa_g1_multiexp_u128_workspace_bytes(n) is the largest plan of any n' <= n,
 * so it never decreases with n (the plan of one n does: fewer windows after a
 * width change, a shorter continuation array after a chunk step) and a
 * workspace sized for the largest call serves every smaller one. */
size_t pa_g1_multiexp_u128_workspace_bytes(size_t n);
int pa_g1_multiexp_u128_device(const pa_g1_affine *dev_bases, const uint64_t *dev_scalars, size_t n, pa_g1 *dev_out,
                               void *workspace, size_t workspace_bytes, void *stream);
int pa_g1_multiexp_u128(const pa_g1_affine *bases, const uint64_t *scalars, size_t n, pa_g1 *out);   /* host memory */
size_t pa_groth16_verify_aggregate_workspace_bytes(const pa_groth16_vk *vk, size_t k);
int pa_groth16_verify_aggregate_device(const pa_groth16_vk *vk, const pa_groth16_proof *dev_proofs,
                                       const pa_fr *dev_inputs, size_t input_stride, unsigned flags,
                                       const uint64_t *dev_z, size_t k, uint8_t *dev_valid, pa_fq12 *dev_gt,
                                       void *workspace, size_t workspace_bytes, void *stream);
int pa_groth16_verify_aggregate(const pa_groth16_vk *vk, const pa_groth16_proof *proofs, const pa_fr *inputs,
                                size_t input_stride, unsigned flags, const uint64_t *z, size_t k, uint8_t *valid,
                                pa_fq12 *gt);   /* host memory */
int pa_groth16_verify_aggregate_encoded_device(const pa_groth16_vk *vk, const uint8_t *dev_enc,
                                               const pa_fr *dev_inputs, size_t input_stride, unsigned flags,
                                               const uint64_t *dev_z, size_t k, uint8_t *dev_valid,
                                               uint8_t *dev_status, pa_fq12 *dev_gt, void *workspace,
                                               size_t workspace_bytes, void *stream);
int pa_groth16_verify_aggregate_encoded(const pa_groth16_vk *vk, const uint8_t *enc, const pa_fr *inputs,
                                        size_t input_stride, unsigned flags, const uint64_t *z, size_t k,
                                        uint8_t *valid, uint8_t *status, pa_fq12 *gt);   /* host memory */
int pa_groth16_verify_aggregate_points_device(const pa_groth16_vk *vk, const pa_groth16_proof *dev_proofs,
                                              const pa_fr *dev_inputs, size_t input_stride, unsigned flags,
                                              const uint64_t *dev_z, size_t k, pa_g1_affine *dev_out,
                                              void *workspace, size_t workspace_bytes, void *stream);
int pa_groth16_verify_aggregate_points(const pa_groth16_vk *vk, const pa_groth16_proof *proofs, const pa_fr *inputs,
                                       size_t input_stride, unsigned flags, const uint64_t *z, size_t k,
                                       pa_g1_affine *out);   /* host memory */

/* ---- device-resident variants (pointers are device memory) ---- */
int pa_g1_decode_batch_device(const uint8_t *enc, size_t n, int compressed, int checked, pa_g1_affine *out,
                              uint8_t *status, void *stream);
int pa_g2_decode_batch_device(const uint8_t *enc, size_t n, int compressed, int checked, pa_g2_affine *out,
                              uint8_t *status, void *stream);
int pa_g1_subgroup_check_batch_device(const pa_g1_affine *p, size_t n, uint8_t *ok, void *stream);
int pa_g2_subgroup_check_batch_device(const pa_g2_affine *p, size_t n, uint8_t *ok, void *stream);
int pa_g1_batch_normalization_device(pa_g1 *v, size_t n, void *stream);
/* u64 words of the fixed-base table and of the scratch used to build it.  The
 * multiply stages below give the reference's wNAF point for the window
 * recommended_wnaf_for_num_scalars(n) (its add_nocarry wrap included, see
 * pa_g1_wnaf_fixed_base).  The fixed-base entries and the Groth16 verifying
 * key (pa_groth16_vk_create's ic) take any on-curve point, of any order: a
 * table row d * B that is the identity (a base of order 3, 11, 33, ...) is
 * marked and skipped like a zero base's. */
size_t pa_g1_fixed_base_table_words(void);
size_t pa_g1_fixed_base_workspace_words(void);
int pa_g1_fixed_base_table_device(const pa_g1 *base, uint64_t *table, uint64_t *workspace, void *stream);
int pa_g1_fixed_base_mul_device(const uint64_t *table, const pa_fr_repr *scalars, pa_g1 *out, size_t n,
                                void *stream);
/* The same product in its GLV form as two stream-ordered stages (s = q x^2 + rem, s P = rem P - q phi(P) when
 * phi(P) == -[x^2] P; the table's 17 base rows plus their phi images and a membership flag in `workspace`); the
 * multiply stage falls back to a double-and-add from `base` when the flag says the base failed the check.  Equal as points to pa_g1_fixed_base_table_device + pa_g1_fixed_base_mul_device. */
int pa_g1_fixed_base_glv_table_device(const pa_g1 *base, uint64_t *table, uint64_t *workspace, void *stream);
int pa_g1_fixed_base_glv_mul_device(const pa_g1 *base, const uint64_t *table, const uint64_t *workspace,
                                    const pa_fr_repr *scalars, pa_g1 *out, size_t n, void *stream);
/* Wnaf::new().base(base, n).scalar(s_i) for every i (wnaf.rs:93-107, 169-178) in one call: the GLV table build
 * and multiply with the table's serial base chain overlapped (per-device side streams, ordered after `stream` by
 * events); equal as points to pa_g1_fixed_base_table_device + pa_g1_fixed_base_mul_device. */
int pa_g1_wnaf_fixed_base_device(const pa_g1 *base, const pa_fr_repr *scalars, pa_g1 *out, size_t n,
                                 uint64_t *table, uint64_t *workspace, void *stream);
int pa_g1_wnaf_fixed_base_window_device(const pa_g1 *base, const pa_fr_repr *scalars, pa_g1 *out, size_t n,
                                        int window, uint64_t *table, uint64_t *workspace, void *stream);
int pa_fq_mul_batch_device(const pa_fq *a, const pa_fq *b, pa_fq *out, size_t n, void *stream);
/* Fq::mul_assign (fq.rs:909-960) on the SoA device layout of SURVEY.md 8(d) config 2: u64 word j
 * (0..5, little-endian, Montgomery, < q) of element i at a[j * n + i]; same bits as the AoS form */
int pa_fq_mul_batch_soa_device(const uint64_t *a, const uint64_t *b, uint64_t *out, size_t n, void *stream);
int pa_fr_mul_batch_device(const pa_fr *a, const pa_fr *b, pa_fr *out, size_t n, void *stream);
int pa_g1_multiexp_device(const pa_g1_affine *bases, const pa_fr_repr *s, size_t n, pa_g1 *out, void *workspace,
                          size_t workspace_bytes, void *stream);
int pa_g2_multiexp_device(const pa_g2_affine *bases, const pa_fr_repr *s, size_t n, pa_g2 *out, void *workspace,
                          size_t workspace_bytes, void *stream);
/* G2 batch_normalization and fixed-base multiply on device memory; the G2
 * table / workspace hold pa_g2_fixed_base_table_words() /
 * pa_g2_fixed_base_workspace_words() u64 */
int pa_g2_batch_normalization_device(pa_g2 *v, size_t n, void *stream);
size_t pa_g2_fixed_base_table_words(void);
size_t pa_g2_fixed_base_workspace_words(void);
int pa_g2_wnaf_fixed_base_device(const pa_g2 *base, const pa_fr_repr *scalars, pa_g2 *out, size_t n,
                                 uint64_t *table, uint64_t *workspace, void *stream);
int pa_g2_wnaf_fixed_base_window_device(const pa_g2 *base, const pa_fr_repr *scalars, pa_g2 *out, size_t n,
                                        int window, uint64_t *table, uint64_t *workspace, void *stream);
/* group law on device memory (see the host batches above) */
int pa_g1_double_batch_device(const pa_g1 *a, pa_g1 *out, size_t n, void *stream);
int pa_g2_double_batch_device(const pa_g2 *a, pa_g2 *out, size_t n, void *stream);
int pa_g1_add_batch_device(const pa_g1 *a, const pa_g1 *b, pa_g1 *out, size_t n, void *stream);
int pa_g2_add_batch_device(const pa_g2 *a, const pa_g2 *b, pa_g2 *out, size_t n, void *stream);
int pa_g1_add_mixed_batch_device(const pa_g1 *a, const pa_g1_affine *b, pa_g1 *out, size_t n, void *stream);
int pa_g2_add_mixed_batch_device(const pa_g2 *a, const pa_g2_affine *b, pa_g2 *out, size_t n, void *stream);
int pa_g1_into_affine_batch_device(const pa_g1 *a, pa_g1_affine *out, size_t n, void *stream);
int pa_g2_into_affine_batch_device(const pa_g2 *a, pa_g2_affine *out, size_t n, void *stream);
int pa_g1_eq_batch_device(const pa_g1 *a, const pa_g1 *b, uint8_t *eq, size_t n, void *stream);
int pa_g2_eq_batch_device(const pa_g2 *a, const pa_g2 *b, uint8_t *eq, size_t n, void *stream);
int pa_miller_loop_fused_batch_device(const pa_g1_affine *p, const pa_g2_affine *q, pa_fq12 *out, size_t n,
                                      void *stream);
/* The first stage of pa_pairing_batch_device, on its own (so a caller can time
 * or overlap the two stages): Miller values from which
 * pa_final_exponentiation_batch_device gives exactly e(p[i], q[i]).  They equal
 * the reference's miller_loop values only up to an Fq2 factor per pair (the
 * lane-pair kernel's G2 steps use homogeneous coordinates and their own line
 * scaling; the final exponentiation removes any Fq2 factor, since
 * (q^12 - 1) / r is a multiple of q^2 - 1), so do not use them as Miller
 * values -- pa_miller_loop_fused_batch_device gives those.  The inputs may be
 * any field elements: the Fq2-factor argument needs q[i] on E', so a pair
 * whose q[i] is off the curve (neither point at infinity) holds the
 * reference's own Miller value instead, recomputed on one lane by a launch
 * behind the pairing-only kernel. */
int pa_pairing_miller_loop_batch_device(const pa_g1_affine *p, const pa_g2_affine *q, pa_fq12 *out, size_t n,
                                        void *stream);
/* final_exponentiation (mod.rs:104-160) on device records: one kernel launch
 * on `stream` (the cooperative kernel up to PA_COOP_MAX records, the generated
 * one above); `out` may equal `in` (in place) or lie apart from it, in which
 * case `in` is left unchanged.  ok[i] = 0 iff in[i] == 0 (None). */
int pa_final_exponentiation_batch_device(const pa_fq12 *in, pa_fq12 *out, uint8_t *ok, size_t n, void *stream);
/* pa_multi_pairing on device memory (the verifier's check without host copies); `work` holds n
 * pa_fq12 (the per-pair Miller values, reduced in place to their product) */
int pa_multi_pairing_device(const pa_g1_affine *p, const pa_g2_affine *q, size_t n, pa_fq12 *out, uint8_t *ok,
                            pa_fq12 *work, void *stream);
/* pa_multi_pairing_batch on device memory: p, q (n = host_offsets[m] records),
 * out (m records), ok and is_one (m bytes; is_one may be NULL) and `workspace`
 * (pa_multi_pairing_batch_workspace_bytes(n, m) bytes: the Miller values, the
 * products and the staged offsets; exact, monotone in both arguments) are
 * device pointers; `host_offsets` is host memory (call metadata, like n) and
 * is not read after the call returns.  Everything is enqueued on `stream`; the
 * call waits only until the offsets have been staged, not for the kernels, and
 * never allocates device memory.  Not for stream capture. */
size_t pa_multi_pairing_batch_workspace_bytes(size_t n_pairs, size_t m);
int pa_multi_pairing_batch_device(const pa_g1_affine *p, const pa_g2_affine *q, const uint64_t *host_offsets,
                                  size_t m, pa_fq12 *out, uint8_t *ok, uint8_t *is_one, void *workspace,
                                  void *stream);
/* G2Prepared::from_affine (mod.rs:168-358) and miller_loop over (G1Affine,
 * G2Prepared) pairs (mod.rs:40-102) on device records: the north-star form
 * whose line coefficients are materialized in HBM (19 592 B per point).
 * Same records and bits as pa_g2_prepare_batch / pa_miller_loop_batch. */
int pa_g2_prepare_batch_device(const pa_g2_affine *q, pa_g2_prepared *out, size_t n, void *stream);
int pa_miller_loop_batch_device(const pa_g1_affine *p, const pa_g2_prepared *q, pa_fq12 *out, size_t n,
                                void *stream);
/* pa_miller_loop_shared_prepared on device records (p: n records, q: one) */
int pa_miller_loop_shared_prepared_device(const pa_g1_affine *p, size_t n, const pa_g2_prepared *q,
                                          pa_fq12 *out, void *stream);
/* e(p[i], q[i]); `scratch` must hold n pa_fq12 (the Miller-loop values) */
int pa_pairing_batch_device(const pa_g1_affine *p, const pa_g2_affine *q, pa_fq12 *out, pa_fq12 *scratch,
                            size_t n, void *stream);

#ifdef __cplusplus
}
#endif
#endif /* PAIRING_AMD_H */
