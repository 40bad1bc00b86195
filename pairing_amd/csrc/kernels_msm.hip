// Variable-base scalar multiplication and multi-scalar multiplication (MSM)
// for G1 and G2 (SURVEY.md §8 f, rank 3).
//
// Per-lane scalar multiplication, bit-exact Jacobian output:
//   CurveAffine::mul (ec.rs:174-177 -> mul_bits ec.rs:88-95): for every one of
//     the 256 scalar bits, MSB first: double, then add_assign_mixed(base) if set.
//   CurveProjective::mul_assign (ec.rs:534-553): double-and-add with full
//     add_assign(self), doubling only after the first set bit.
// Both replay the reference's exact formula sequence (curve.h), so the X, Y, Z
// words equal the reference's, not just the point.
//
// MSM  sum_i s_i * P_i  (affine bases, FrRepr scalars: the shape of the
// downstream provers' multiexp over `CurveAffine::mul` + `add_assign`).  The
// result is equal *as a point* to the reference's sum (PartialEq, ec.rs:45-85);
// Jacobian words differ because the addition chain is Pippenger's:
//   1. k_msm_digits: signed c-bit digits per window (|d| <= 2^(c-1)); item
//      (window, |d|) -> sort key, (i | sign<<31) -> value.   c*W >= 257 so any
//      256-bit FrRepr (also >= r, as the reference's BitIterator allows) fits.
//   2. a stable LSD counting sort of the items by bucket, 8 bits per pass
//      (k_sort_hist / k_sort_scan / k_sort_scatter, ceil((c-1)/8) passes):
//      each bucket's points become contiguous in term order, windows stay
//      apart, zero digits are dropped.  Same order as a stable sort of the
//      (w*B + |d|-1) keys, so the result is deterministic.
//   3. k_msm_bucket_bounds: [start, end) per bucket from the sorted keys.
//   4. k_msm_chunk_acc_fl / _fl2: one lane per 64 sorted items, mixed additions
//      (madd-2007-bl) of the bases gathered from HBM as lazy rows (y negated
//      for negative digits), run by run; k_msm_bucket_fix folds the pieces of
//      buckets that span chunks and zeroes empty buckets (k_msm_long_fix: the
//      buckets that span many).
//   5. k_msm_segments<G>: per window, sum_m m*B_m by running sums over
//      segments of L buckets (T += B_m; S += T, top down), plus a*T for the
//      segment offset.
//   6. k_msm_group_sum_fl / _fl2 (repeated): segment results -> one sum per window.
//   7. k_msm_horner_q: one group of lane quads, sum_w 2^(c*w) S_w.
// Steps 4-6 run on the lazy 28-bit core for both groups, written once over
// curve_fl.h / curve_fl2.h's shared names; MsmKernels<G> names the kernels
// that differ by group on purpose.
// Steps 4-7 run per part of the windows (top windows first, msm_run): a part's
// reduction (4's fix-up, 5, 6) and its Horner leg run on side streams while
// the next part accumulates, so only the last part's tail is exposed.
// Work: n*W mixed additions + ~2*W*2^(c-1) additions + ~256 doublings.
//
// MSM over prepared G1 bases (launch_msm_prepare / launch_msm_prepared, group 1):
// the bases are converted to the lazy rows once, row n + i = -phi(P_i) =
// (beta x_i, -y_i) beside row i = P_i, and checked for G1 membership once.
// When every base is in G1, k_msm_digits_glv splits each scalar s = q x^2 + rem
// (glv_split.h) into the two virtual terms rem * P_i + q * (-phi(P_i)), both
// below 2^129, and steps 2-7 run over 2m virtual terms and ceil(130 / c)
// windows: the same msm_run with another digit kernel, term count and window
// count (MsmJob).  Otherwise the 257-bit pipeline runs over rows [0, m).
//
// MSM over prepared G2 bases (group 2):
// the same over 56-word rows, with row n + i = (beta^2 x_i, -y_i) = x^2 Q_i
// (kMsmBeta2): the split, the digit kernels and every stage are the G1 path's.
//
// A batch of k scalar vectors over the same prepared bases
// (launch_msm_prepared with k > 1) is the same pipeline over k W windows: vector
// j's window w is window j W + w, its items gather the same rows, the window
// parts are ranges of vectors and k_msm_horner_batch_q runs every vector's
// Horner chain side by side.  The digit kernels take Montgomery Fr rows too.
//
// 128-bit scalars over per-call G1 bases (launch_msm_u128_g1): a third plan,
// k_msm_digits_u128 over 16-byte rows in the GLV plan's ceil(130 / c) windows
// with n real terms -- no split, no endomorphism, no membership assumption; the
// bases are converted per call as in the plain entry.

#include <vector>

#include "curve_fl.h"
#include "curve_fl2.h"
#include "dec_quad.h"
#include "env.h"
#include "fr.h"
#include "glv_split.h"
#include "launch_msm.h"

#include <cstdlib>
#include <mutex>
#include <utility>

namespace pa {

// ---------------- per-lane scalar multiplication ----------------
template <int G>
__global__ void __launch_bounds__(64) k_affine_mul(const uint64_t* __restrict__ p, const uint64_t* __restrict__ s,
                                                   uint64_t* __restrict__ out, size_t n) {
    using F = typename Grp<G>::F;
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    Aff<F> a;
    load_aff(a, p + (size_t)Grp<G>::AW * i);
    uint64_t k[4];
#pragma unroll
    for (int w = 0; w < 4; w++) k[w] = s[4 * i + w];
    Jac<F> acc;
    jac_zero(acc);
#pragma unroll 1
    for (int bit = 255; bit >= 0; bit--) {  // mul_bits, ec.rs:88-95
        jac_double(acc);
        if ((k[bit >> 6] >> (bit & 63)) & 1) jac_add_mixed(acc, a);
    }
    store_jac(out + (size_t)Grp<G>::JW * i, acc);
}

template <int G>
__global__ void __launch_bounds__(64) k_proj_mul(const uint64_t* __restrict__ p, const uint64_t* __restrict__ s,
                                                 uint64_t* __restrict__ out, size_t n) {
    using F = typename Grp<G>::F;
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    Jac<F> base, acc;
    load_jac(base, p + (size_t)Grp<G>::JW * i);
    uint64_t k[4];
#pragma unroll
    for (int w = 0; w < 4; w++) k[w] = s[4 * i + w];
    jac_zero(acc);
    bool found_one = false;
#pragma unroll 1
    for (int bit = 255; bit >= 0; bit--) {  // mul_assign, ec.rs:534-553
        const bool b = (k[bit >> 6] >> (bit & 63)) & 1;
        if (found_one) jac_double(acc);
        else found_one = b;
        if (b) jac_add(acc, base);
    }
    store_jac(out + (size_t)Grp<G>::JW * i, acc);
}

// ---------------- MSM ----------------
struct MsmPlan {
    uint32_t c, W, B, L;        // window bits, windows, buckets per window, segment length
    uint32_t passes;            // counting-sort passes over the c-1 magnitude bits
    uint32_t T;                 // items per lane of the bucket accumulation
    uint32_t tpw;               // sort tiles per window
    size_t k;                   // scalar vectors (a batch: window j W + w is vector j's window w)
    size_t WT;                  // k * W windows in all
    bool fits;                  // 32-bit item positions and keys: WT n <= 2^32 - 1 and WT B < 2^32
    size_t items;               // WT * nt
    size_t off_keys_in, off_keys_out, off_vals_in, off_vals_out, off_start, off_end;
    size_t off_buckets, off_segs, off_tmp, off_hist, off_wtot, off_cont, off_basefl, off_hacc, off_long, off_wpre;
    size_t total;
};

static inline uint32_t msm_window_bits(size_t n) {
    int lg = 0;
    while (lg < 40 && ((size_t)1 << (lg + 1)) <= n) lg++;
    int c = lg - 3;
    static const int cmax = (int)env_clamp("PA_MSM_CMAX", 16, 4, 20);   // A/B knob
    if (c < 4) c = 4;
    if (c > cmax) c = cmax;
    return (uint32_t)c;
}

// The GLV path's window bits for nt = 2m virtual terms of 130 bits each
// (PA_MSM_GLV_C to A/B an absolute value), chosen by A/B at 2^16 / 2^18 / 2^20
// terms (profiles/msm_prepared/): the plain rule lg(nt) - 3 up to 13, where
// 10 windows cover the 130 bits exactly and the top window's digits are as
// spread as the others'; 13 up to 2^19 virtual terms (2^18 terms: 2.76 ms
// against 2.97 / 3.09 / 3.09 / 3.03 for c = 14 .. 17); then 15 (9 windows) and
// from 2^21 virtual terms 17 (8 windows: 8 x 2^21 items against the plain
// path's 17 x 2^20; 16 has 9 windows of 2^16 / 2 buckets, 6.75 ms against 6.03).
// G2 keeps the rule: its additions cost three of G1's in the accumulation and
// in the reduction alike, and the A/B of absolute values found the same optimum
// (profiles/msm_g2_prepared/ab_single.txt), c = 10 / 11 / 12 / 13 / 14 / 15 / 16:
// 2^14 terms 4.01 / 3.92 / 3.79 / 3.78 / 4.17 / 4.24 / 4.70 ms (the rule: 12),
// 2^16 terms 5.78 / 5.06 / 4.85 / 4.12 / 4.98 / 4.95 / 6.14 ms (13),
// 2^18 terms 10.41 / 8.27 / 8.76 / 6.85 / 7.78 / 8.29 / 8.78 ms (13).
static inline uint32_t msm_window_bits_glv(size_t nt) {
    static const int env = (int)env_within("PA_MSM_GLV_C", 0, 4, 20);
    if (env) return (uint32_t)env;
    int lg = 0;
    while (lg < 40 && ((size_t)1 << (lg + 1)) <= nt) lg++;
    if (lg >= 21) return 17;
    if (lg >= 20) return 15;
    const int c = lg - 3;
    return (uint32_t)(c < 4 ? 4 : (c > 13 ? 13 : c));
}

// A batch's window bits (PA_MSM_BATCH_C to A/B an absolute value).  The
// bucket reduction of k W windows is throughput work beside the k W nt mixed
// additions, which moves the optimum little: the single call's rule measured
// within its neighbours' spread at the batch shapes (profiles/msm_prepared_batch/):
// 16 vectors of 2^16 terms, c = 11 / 12 / 13 / 14 / 15: 7.92 / 7.81 / 8.01 /
// 9.17 / 10.38 ms (64 vectors: 26.3 / 25.5 / 25.6 / 29.1 / 33.3); 256 vectors of
// 2^12 terms, c = 8 / 9 / 10 / 11: 12.4 / 11.1 / 11.3 / 10.6 ms; 8 vectors of
// 2^18 terms, c = 12 / 13 / 14 / 15: 12.6 / 11.8 / 11.7 / 13.0 ms.  So the rule
// is the single call's, which also makes a batch of one vector its job.
// G2 batches keep it too (profiles/msm_g2_prepared/ab_batch.txt, one part):
// against c = 9 / 10 / 11 / 13 the rule measured, k x terms,
//   2 x 2^18 (13): 11.84 ms against 15.65 / 14.36 / 12.07 / 11.86,
//   2 x 2^16 (13): 5.03 against 5.77 / 5.32 / 5.29 / 5.03,
//   4 x 2^16 (13): 8.21 against 8.52 / 8.28 / 8.82 / 8.28,
//   8 x 2^16 (13): 12.74 against 13.74 / 13.41 / 12.47 / 12.73,
//   4 x 2^14 (12): 4.00 against 4.14 / 4.01 / 4.12 / 3.60,
//   16 x 2^14 (12): 9.91 against 8.21 / 8.61 / 8.82 / 10.98,
//   16 x 2^12 (10): 3.74 against 3.91 / 3.73 / 4.19 / 6.78,
//   64 x 2^12 (10): 8.95 against 9.06 / 9.34 / 11.31 / 21.92.
// One shape, 16 x 2^14, would gain 17 % from c = 9 while 4 x 2^14 wants 13: no
// rule in nt or k separates them, so none is added.
static inline uint32_t msm_window_bits_batch(size_t nt) {
    static const int env = (int)env_within("PA_MSM_BATCH_C", 0, 4, 20);
    return env ? (uint32_t)env : msm_window_bits_glv(nt);
}

// items (sorted (bucket, term) pairs) per lane of the bucket accumulation
// (PA_MSM_CHUNK to A/B, 8..512): 32 / 48 / 64 / 96 / 128 measured 167 / 162 /
// 170 / 159 / 171 M terms/s at 2^20 with one part, 64 with two parts 175-177
// (profiles/r04_msm_parts.txt)
constexpr uint32_t kMsmChunk = 64;
// Below 64 items per lane the chunk shrinks until a part's accumulation has
// one lane for each of the chip's 256 CUs x 4 SIMDs x 64 (G2 at 2^16: 20 x 2^16
// items, 320 waves at 64 per lane)
constexpr size_t kMsmFillLanes = 65536;
static uint32_t msm_chunk(size_t items, uint32_t parts) {
    static const int env = (int)env_clamp("PA_MSM_CHUNK", 0, -1, 512);   // 0: unset; else 8..512
    if (env) return (uint32_t)(env < 8 ? 8 : env);
    const size_t t = (items + kMsmFillLanes * parts - 1) / (kMsmFillLanes * parts);
    return (uint32_t)(t < 8 ? 8 : (t > kMsmChunk ? kMsmChunk : t));
}
// window parts (msm_run): at most this many, each with a Horner accumulator slot
constexpr uint32_t kMsmMaxParts = 8;
// a bucket whose items span more chunks than this has its continuation pieces
// summed by a block (k_msm_long_fix), not serially by one lane of
// k_msm_bucket_fix.  A block costs ~span/256 + 8 additions per bucket with at
// most kMsmLongBlocks buckets at a time, a lane `span` additions with every
// bucket at once: above 128 chunks the block is never the slower choice, even
// when every bucket of every window is that long (at most ~2 100 of them at
// 2^20 terms)
constexpr size_t kMsmLongSpan = 128;
// The GLV path's threshold (PA_MSM_GLV_LONGSPAN to A/B).  Its top window holds
// the 8-10 leading bits of halves below 2^129: a few hundred buckets of
// thousands of items each, 20-128 chunks apiece, which one lane of
// k_msm_bucket_fix folded in 1-2.3 ms (2^18 terms at c = 15: 2.27 ms against
// 0.56 ms for the part's whole accumulation; profiles/msm_prepared/).  128 /
// 32 / 16 / 8 / 4 measured 6.32 / 6.06 / 6.18 / 6.03 / 6.07 ms at 2^20 terms and
// 2.36 / 2.37 / 1.90 / 1.90 / 2.14 ms at 2^16: 8, and never below twice an
// evenly filled bucket's span (msm_run), so that large MSMs whose every
// bucket spans several chunks keep the one-lane fold.  G2 shares it: 4 / 8 /
// 16 / 32 / 128 measured 3.69 / 3.78 / 4.11 / 4.66 / 8.02 ms at 2^14 G2 terms,
// 4.08 / 4.10 / 4.12 / 5.49 / 5.42 at 2^16 and 6.85 / 6.86 / 6.87 / 8.27 / 8.08
// at 2^18 (profiles/msm_g2_prepared/ab_single.txt): 4 and 8 within the spread.
static size_t msm_long_span_glv() {
    static const size_t v = (size_t)env_within("PA_MSM_GLV_LONGSPAN", 8, 1, 4096);
    return v;
}
constexpr unsigned kMsmLongBlocks = 256;
// counting sort: a tile is 16 rounds of one item per thread of a 256-thread block
constexpr uint32_t kSortIpt = 16;
constexpr uint32_t kSortTile = 256 * kSortIpt;

static inline size_t align256(size_t x) { return (x + 255) & ~(size_t)255; }

// window parts of one MSM (PA_MSM_PARTS, default 2; 1 = every kernel on the
// caller's stream in order; 3 and 4 measured slower: the tails compete with the
// next part's accumulation for SIMDs, profiles/r04_msm_parts.txt)
static uint32_t msm_parts(uint32_t W) {
    static const uint32_t parts = (uint32_t)env_clamp("PA_MSM_PARTS", 2, 1, kMsmMaxParts);
    return parts < W ? parts : W;
}

// A batch's parts are ranges of vectors (PA_MSM_BATCH_PARTS to A/B, default 1).
// A single MSM hides its upper parts' latency-bound tails under the next part's
// accumulation; a batch's reduction and Horner grid are wide enough to fill
// the chip themselves, and on side streams they only compete with the
// accumulation: 1 / 2 / 4 / 8 parts measured 7.45 / 8.01 / 9.42 / 10.81 ms at
// 16 vectors of 2^16 terms, 10.92 / 11.33 / 11.47 / 11.99 ms at 256 of 2^12 and
// 11.35 / 11.85 / 12.76 / 15.57 ms at 8 of 2^18 (profiles/msm_prepared_batch/).
// G2: 1 / 2 parts measured 11.84 / 13.57 ms at 2 vectors of 2^18 terms, 5.03 /
// 5.24 at 2 of 2^16, 8.21 / 7.17 at 4 of 2^16, 12.74 / 13.75 at 8 of 2^16, 4.00 /
// 4.39 at 4 of 2^14, 9.91 / 8.17 at 16 of 2^14, 3.74 / 4.01 at 16 of 2^12 and
// 8.95 / 7.86 at 64 of 2^12; 3 and 4 parts never won
// (profiles/msm_g2_prepared/ab_batch.txt).  Two parts win three shapes and
// lose five with no pattern in k or the size: G2 stays at one.
static uint32_t msm_parts_batch(size_t k) {
    static const uint32_t parts = (uint32_t)env_clamp("PA_MSM_BATCH_PARTS", 1, 1, kMsmMaxParts);
    return parts < k ? parts : (uint32_t)k;
}

// `n` terms per window; the windows cover 257 bits for the plain entries (a
// 256-bit FrRepr and the last carry), 130 for the GLV halves (glv; < 2^129)
// and for 128-bit scalars over n real terms (the u128 entry passes glv too:
// the same window rule, no endomorphism, bases converted per call).
// own_basefl: the workspace holds the per-call converted bases.
// k > 1: a batch of k scalar vectors over the same bases, k W windows.
static hipError_t msm_plan(MsmPlan& p, int group, size_t n, bool glv = false, bool own_basefl = true, size_t k = 1) {
    p.c = glv ? (k > 1 ? msm_window_bits_batch(n) : msm_window_bits_glv(n)) : msm_window_bits(n);
    p.W = ((glv ? 130 : 257) + p.c - 1) / p.c;
    p.B = 1u << (p.c - 1);
    p.k = k;
    p.fits = k <= 0xffffffffull / p.W && k * p.W <= 0xffffffffull / n && k * p.W <= 0xffffffffull / p.B;
    if (k > 1 && !p.fits) return hipErrorInvalidValue;
    p.WT = k * p.W;
    // A/B knob: PA_MSM_SEG; default 8 buckets per segment for G1, 4 for G2 (G2
    // at 2^16 / 2^18: 5.91 / 9.13 ms with 8, 5.73 / 8.90 with 4; G1 at 2^20: 173
    // vs 163 M terms/s; profiles/r04_msm_g2_lazy.txt)
    static const uint32_t seg_env = (uint32_t)env_within("PA_MSM_SEG", 0, 2, 32);   // a power of two, or ignored
    const uint32_t seg = seg_env && !(seg_env & (seg_env - 1)) ? seg_env : (group == 1 ? 8u : 4u);
    p.L = p.B < seg ? p.B : seg;  // short segments: the running sums are a latency chain per lane
    p.items = p.WT * n;
    p.passes = (p.c - 1 + 7) / 8;
    p.tpw = (uint32_t)((n + kSortTile - 1) / kSortTile);
    const size_t jw = 8 * (size_t)(group == 1 ? Grp<1>::JW : Grp<2>::JW);
    const size_t nb = p.WT * p.B;
    const size_t nseg = p.WT * (p.B / p.L);
    size_t off = 0;
    p.off_keys_in = off; off = align256(off + 4 * p.items);
    p.off_keys_out = off; off = align256(off + 4 * p.items);
    p.off_vals_in = off; off = align256(off + 4 * p.items);
    p.off_vals_out = off; off = align256(off + 4 * p.items);
    p.off_start = off; off = align256(off + 4 * nb);
    p.off_end = off; off = align256(off + 4 * nb);
    p.off_buckets = off; off = align256(off + jw * nb);
    p.off_segs = off; off = align256(off + jw * nseg);
    p.off_tmp = off; off = align256(off + jw * nseg);
    p.T = msm_chunk(p.items, k > 1 ? msm_parts_batch(k) : msm_parts(p.W));
    p.off_cont = off; off = align256(off + jw * ((p.items + p.T - 1) / p.T + 1));
    p.off_basefl = off; off = align256(off + (own_basefl ? 4 * (group == 1 ? 28 : 56) * n : 0));
    p.off_hist = off; off = align256(off + 4 * p.WT * 256 * p.tpw);
    p.off_wtot = off; off = align256(off + 4 * p.WT);
    p.off_hacc = off; off = align256(off + jw * kMsmMaxParts);
    p.off_long = off; off = align256(off + 4 * (nb + kMsmMaxParts));   // long-bucket lists + counts
    p.off_wpre = off; off = align256(off + 4 * (p.WT + 1));            // exclusive prefix of wtot
    p.total = off;
    return hipSuccess;
}

// A scalar row as the digit kernels read it: the canonical words, or with
// mont the Montgomery form of a value below r taken through into_repr.
PA_DEV void msm_load_scalar(uint64_t (&k)[4], const uint64_t* __restrict__ row, bool mont) {
#pragma unroll
    for (int w = 0; w < 4; w++) k[w] = row[w];
    if (mont) {
        Fr a, r;
#pragma unroll
        for (int w = 0; w < 4; w++) {
            a.w[2 * w] = (uint32_t)k[w];
            a.w[2 * w + 1] = (uint32_t)(k[w] >> 32);
        }
        fr_into_repr(r, a);
#pragma unroll
        for (int w = 0; w < 4; w++) k[w] = (uint64_t)r.w[2 * w] | ((uint64_t)r.w[2 * w + 1] << 32);
    }
}

// `vectors` scalar vectors of n rows end to end; vector j's window w is window
// j W + w of the pipeline (win0 = j W), over the same n terms.
__global__ void __launch_bounds__(256) k_msm_digits(const uint64_t* __restrict__ scalars, size_t n, size_t vectors,
                                                    bool mont, uint32_t c, uint32_t W, uint32_t B, uint32_t sentinel,
                                                    uint32_t* __restrict__ keys, uint32_t* __restrict__ vals) {
    const size_t t = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= n * vectors) return;
    const size_t vec = t / n, i = t - vec * n;
    const uint32_t win0 = (uint32_t)vec * W;
    uint64_t k[4];
    msm_load_scalar(k, scalars + 4 * t, mont);
    const uint32_t mask = (1u << c) - 1;
    uint32_t carry = 0;
    for (uint32_t w = 0; w < W; w++) {
        const uint32_t bit = w * c;
        uint32_t raw = 0;
        if (bit < 256) {
            const uint32_t word = bit >> 6, sh = bit & 63;
            uint64_t v = k[word] >> sh;
            if (sh + c > 64 && word < 3) v |= k[word + 1] << (64 - sh);
            raw = (uint32_t)v & mask;
        }
        raw += carry;
        int d;
        if (raw > B) {
            d = (int)raw - (int)(1u << c);
            carry = 1;
        } else {
            d = (int)raw;
            carry = 0;
        }
        const size_t at = (size_t)(win0 + w) * n + i;
        if (d == 0) {
            keys[at] = sentinel;
            vals[at] = (uint32_t)i;
        } else {
            const uint32_t mag = (uint32_t)(d < 0 ? -d : d);
            keys[at] = (win0 + w) * B + (mag - 1);
            vals[at] = (uint32_t)i | (d < 0 ? 0x80000000u : 0u);
        }
    }
}

// The GLV path's digits: scalar i = q x^2 + rem gives virtual term i (rem,
// row i of the prepared bases) and virtual term m + i (q, row row_off + i =
// -phi(P_i)); same items as k_msm_digits, nt = 2m terms per window.  Both
// halves are below 2^129 and c W >= 130, so the top window's raw digit is
// below 2^(c-1): with the carry at most B, never a carry out.
__global__ void __launch_bounds__(256) k_msm_digits_glv(const uint64_t* __restrict__ scalars, size_t m,
                                                        size_t vectors, bool mont, uint32_t row_off, uint32_t c,
                                                        uint32_t W, uint32_t B, uint32_t sentinel,
                                                        uint32_t* __restrict__ keys, uint32_t* __restrict__ vals) {
    const size_t t = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= m * vectors) return;
    const size_t vec = t / m, i = t - vec * m;
    const uint32_t win0 = (uint32_t)vec * W;
    uint64_t k[4], half[2][3];
    msm_load_scalar(k, scalars + 4 * t, mont);
    glv_split(k, half[0], half[1]);
    const uint32_t mask = (1u << c) - 1;
    const size_t nt = 2 * m;
#pragma unroll
    for (int h = 0; h < 2; h++) {
        const uint64_t v0 = half[h][0], v1 = half[h][1], v2 = half[h][2];
        const size_t term = h ? m + i : i;
        const uint32_t row = (uint32_t)(h ? row_off + i : i);
        uint32_t carry = 0;
        for (uint32_t w = 0; w < W; w++) {
            const uint32_t bit = w * c;
            uint32_t raw = 0;
            if (bit < 192) {
                const uint32_t word = bit >> 6, sh = bit & 63;
                const uint64_t lo = word == 0 ? v0 : (word == 1 ? v1 : v2);
                const uint64_t hi = word == 0 ? v1 : (word == 1 ? v2 : 0);
                uint64_t v = lo >> sh;
                if (sh + c > 64) v |= hi << (64 - sh);
                raw = (uint32_t)v & mask;
            }
            raw += carry;
            int d;
            if (raw > B) {
                d = (int)raw - (int)(1u << c);
                carry = 1;
            } else {
                d = (int)raw;
                carry = 0;
            }
            const size_t at = (size_t)(win0 + w) * nt + term;
            if (d == 0) {
                keys[at] = sentinel;
                vals[at] = row;
            } else {
                const uint32_t mag = (uint32_t)(d < 0 ? -d : d);
                keys[at] = (win0 + w) * B + (mag - 1);
                vals[at] = row | (d < 0 ? 0x80000000u : 0u);
            }
        }
    }
}

// 128-bit scalars in 16-byte rows (two u64, little-endian) over n real terms:
// the items of k_msm_digits in the 130-bit plan's windows.  c W >= 130 and the
// scalar is below 2^128, so the top window's raw digit is below 2^(c-2): with
// the carry at most 2^(c-2) <= B, never a carry out (2^128 - 1 recodes to -1
// and a 1 at bit 128, inside the top window).
__global__ void __launch_bounds__(256) k_msm_digits_u128(const uint64_t* __restrict__ scalars, size_t n, uint32_t c,
                                                         uint32_t W, uint32_t B, uint32_t sentinel,
                                                         uint32_t* __restrict__ keys, uint32_t* __restrict__ vals) {
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const uint4 row = reinterpret_cast<const uint4*>(scalars)[i];
    const uint64_t v0 = (uint64_t)row.x | ((uint64_t)row.y << 32), v1 = (uint64_t)row.z | ((uint64_t)row.w << 32);
    const uint32_t mask = (1u << c) - 1;
    uint32_t carry = 0;
    for (uint32_t w = 0; w < W; w++) {
        const uint32_t bit = w * c;
        uint32_t raw = 0;
        if (bit < 128) {
            const uint32_t word = bit >> 6, sh = bit & 63;
            uint64_t v = (word == 0 ? v0 : v1) >> sh;
            if (sh + c > 64 && word == 0) v |= v1 << (64 - sh);
            raw = (uint32_t)v & mask;
        }
        raw += carry;
        int d;
        if (raw > B) {
            d = (int)raw - (int)(1u << c);
            carry = 1;
        } else {
            d = (int)raw;
            carry = 0;
        }
        const size_t at = (size_t)w * n + i;
        if (d == 0) {
            keys[at] = sentinel;
            vals[at] = (uint32_t)i;
        } else {
            const uint32_t mag = (uint32_t)(d < 0 ? -d : d);
            keys[at] = w * B + (mag - 1);
            vals[at] = (uint32_t)i | (d < 0 ? 0x80000000u : 0u);
        }
    }
}

__global__ void __launch_bounds__(256) k_msm_bucket_bounds(const uint32_t* __restrict__ keys, size_t items,
                                                           uint32_t sentinel, uint32_t* __restrict__ start,
                                                           uint32_t* __restrict__ end) {
    const size_t j = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (j >= items) return;
    const uint32_t k = keys[j];
    if (k >= sentinel) return;
    if (j == 0 || keys[j - 1] != k) start[k] = (uint32_t)j;
    if (j + 1 == items || keys[j + 1] != k) end[k] = (uint32_t)(j + 1);
}

// ---- the bucketing sort (step 2) ----
// Items are (key, value) = (w*B + |d|-1, term | sign<<31).  Pass k orders the
// items of each window by the 8-bit digit ((key & (B-1)) >> 8k), stably; the
// first pass reads the window-major digit output (window w at [w*n, w*n + n),
// zero digits carry key >= sentinel and are skipped), every pass writes the
// windows compacted (window w at [wpre[w], wpre[w] + wtot[w])).  A window's
// source range is cut in tiles of kSortTile items; hist[w][digit][tile] holds
// the tile's digit counts, and after k_sort_scan the exclusive prefix over
// (digit, tile) in that order -- where the tile's run of each digit starts.

// Window w's first item in the compacted layout is wpre[w], the exclusive
// prefix of wtot (wpre[windows] = every window's items).  A pass moves every
// nonzero item, so wtot and its prefix are the same after each pass: the
// prefix is written once, after the first pass's k_sort_scan.  One block.
__global__ void __launch_bounds__(1024) k_sort_wprefix(const uint32_t* __restrict__ wtot, uint32_t windows,
                                                       uint32_t* __restrict__ wpre) {
    __shared__ uint32_t s[2][1024];
    const uint32_t tid = threadIdx.x, nt = blockDim.x;
    uint32_t carry = 0;
    for (uint32_t seg = 0; seg < windows; seg += nt) {
        const uint32_t idx = seg + tid;
        const uint32_t v = idx < windows ? wtot[idx] : 0u;
        s[0][tid] = v;
        __syncthreads();
        int cur = 0;
        for (uint32_t d = 1; d < nt; d <<= 1) {  // inclusive Hillis-Steele scan
            s[cur ^ 1][tid] = s[cur][tid] + (tid >= d ? s[cur][tid - d] : 0u);
            cur ^= 1;
            __syncthreads();
        }
        if (idx < windows) wpre[idx] = carry + s[cur][tid] - v;
        carry += s[cur][nt - 1];
        __syncthreads();  // s is rewritten by the next segment
    }
    if (tid == 0) wpre[windows] = carry;
}

struct SortPass {
    uint32_t shift, bmask, sentinel, tpw, first;
    size_t n;
};

// window w's source range [base, base + count); tile t is its items
// [t kSortTile, (t + 1) kSortTile) clipped to count
PA_DEV void sort_window(const SortPass& sp, const uint32_t* __restrict__ wtot, const uint32_t* __restrict__ wpre,
                        uint32_t w, size_t& base, uint32_t& count) {
    if (sp.first) {
        base = (size_t)w * sp.n;
        count = (uint32_t)sp.n;
    } else {
        base = wpre[w];
        count = wtot[w];
    }
}

__global__ void __launch_bounds__(256) k_sort_hist(const uint32_t* __restrict__ keys, const uint32_t* __restrict__ wtot,
                                                   const uint32_t* __restrict__ wpre, SortPass sp,
                                                   uint32_t* __restrict__ hist) {
    __shared__ uint32_t h[256];
    const uint32_t tid = threadIdx.x, w = blockIdx.x / sp.tpw, t = blockIdx.x % sp.tpw;
    h[tid] = 0;
    __syncthreads();
    size_t base;
    uint32_t count;
    sort_window(sp, wtot, wpre, w, base, count);
    const uint32_t lo = t * kSortTile;
    uint32_t key[kSortIpt];  // the whole tile's loads in flight at once
#pragma unroll
    for (uint32_t r = 0; r < kSortIpt; r++) {
        const uint32_t k = lo + r * 256 + tid;
        key[r] = k < count ? keys[base + k] : 0xffffffffu;
    }
#pragma unroll
    for (uint32_t r = 0; r < kSortIpt; r++)
        if (key[r] < sp.sentinel) atomicAdd(&h[((key[r] & sp.bmask) >> sp.shift) & 0xff], 1u);
    __syncthreads();
    hist[((size_t)w * 256 + tid) * sp.tpw + t] = h[tid];
}

// exclusive prefix over one window's 256 x tpw counts (digit-major), in place;
// the window's item count into wtot[w].  One 1024-thread block per window,
// segments of 1024 x 64 counters: each thread's 64 as 16 uint4 loads in
// flight, a block scan of the 1024 thread sums, then the prefixed writes.
__global__ void __launch_bounds__(1024) k_sort_scan(uint32_t* __restrict__ hist, uint32_t tpw,
                                                    uint32_t* __restrict__ wtot) {
    __shared__ uint32_t s[2][1024];
    const uint32_t tid = threadIdx.x;
    uint32_t* a = hist + (size_t)blockIdx.x * 256 * tpw;
    const uint32_t len = 256 * tpw;  // a multiple of 4
    uint32_t carry = 0;
    for (uint32_t seg = 0; seg < len; seg += 1024 * 64) {
        const uint32_t b0 = seg + tid * 64;
        uint4 v[16];
#pragma unroll
        for (int q = 0; q < 16; q++)
            v[q] = b0 + 4 * q < len ? *reinterpret_cast<const uint4*>(a + b0 + 4 * q) : make_uint4(0, 0, 0, 0);
        uint32_t sum = 0;
#pragma unroll
        for (int q = 0; q < 16; q++) sum += v[q].x + v[q].y + v[q].z + v[q].w;
        s[0][tid] = sum;
        __syncthreads();
        int cur = 0;
        for (uint32_t d = 1; d < 1024; d <<= 1) {  // inclusive Hillis-Steele scan
            s[cur ^ 1][tid] = s[cur][tid] + (tid >= d ? s[cur][tid - d] : 0u);
            cur ^= 1;
            __syncthreads();
        }
        uint32_t run = carry + s[cur][tid] - sum;
#pragma unroll
        for (int q = 0; q < 16; q++) {
            uint4 o;
            o.x = run;
            o.y = (run += v[q].x);
            o.z = (run += v[q].y);
            o.w = (run += v[q].z);
            run += v[q].w;
            if (b0 + 4 * q < len) *reinterpret_cast<uint4*>(a + b0 + 4 * q) = o;
        }
        carry += s[cur][1023];
        __syncthreads();  // s is rewritten by the next segment
    }
    if (tid == 0) wtot[blockIdx.x] = carry;
}

// One block per tile: rank the tile's items by digit, stably, stage them
// digit-sorted in LDS, then write each digit's run to its place --
// consecutive threads write consecutive addresses of a few runs instead of
// one scattered word each.  Wave q owns the tile's items [q 1024, (q+1) 1024),
// 64 consecutive ones per round, and counts digits in its own LDS row, so the
// ranking needs no block barrier: source order = (wave, round, lane).
__global__ void __launch_bounds__(256) k_sort_scatter(const uint32_t* __restrict__ keys_in,
                                                      const uint32_t* __restrict__ vals_in,
                                                      const uint32_t* __restrict__ hist,
                                                      const uint32_t* __restrict__ wtot,
                                                      const uint32_t* __restrict__ wpre, SortPass sp,
                                                      uint32_t* __restrict__ keys_out, uint32_t* __restrict__ vals_out) {
    __shared__ uint32_t gbase[256], loff[256], wcnt[4][256], scan[2][256];
    __shared__ uint32_t sk[kSortTile], sv[kSortTile];
    __shared__ uint32_t wb_s;
    const uint32_t tid = threadIdx.x, w = blockIdx.x / sp.tpw, t = blockIdx.x % sp.tpw;
    const uint32_t wave = tid >> 6, lane = tid & 63;
    size_t base;
    uint32_t count;
    sort_window(sp, wtot, wpre, w, base, count);
    const uint32_t lo = t * kSortTile + wave * (64 * kSortIpt);
    uint32_t keyr[kSortIpt], valr[kSortIpt];  // the wave's loads in flight at once
#pragma unroll
    for (uint32_t r = 0; r < kSortIpt; r++) {
        const uint32_t k = lo + r * 64 + lane;
        keyr[r] = 0xffffffffu;
        valr[r] = 0;
        if (k < count) {
            keyr[r] = keys_in[base + k];
            valr[r] = vals_in[base + k];
        }
    }
    if (tid == 0) wb_s = wpre[w];
    // this tile's digit counts from the prefix: next entry (digit-major) minus this one
    const size_t flat = (size_t)tid * sp.tpw + t, len = (size_t)256 * sp.tpw;
    const uint32_t* hw = hist + (size_t)w * len;
    const uint32_t off = hw[flat];
    const uint32_t cnt = (flat + 1 < len ? hw[flat + 1] : wtot[w]) - off;
    scan[0][tid] = cnt;
#pragma unroll
    for (int q = 0; q < 4; q++) wcnt[q][tid] = 0;
    __syncthreads();
    const uint64_t lt = (1ull << lane) - 1;
    uint32_t slot[kSortIpt];  // rank among the wave's items of the same digit
#pragma unroll
    for (uint32_t r = 0; r < kSortIpt; r++) {
        const bool valid = keyr[r] < sp.sentinel;
        const uint32_t d = valid ? ((keyr[r] & sp.bmask) >> sp.shift) & 0xff : 0;
        // lanes of this wave holding the same digit (8 ballots)
        uint64_t peers = __ballot(valid);
#pragma unroll
        for (int b = 0; b < 8; b++) {
            const uint64_t m = __ballot((d >> b) & 1);
            peers &= ((d >> b) & 1) ? m : ~m;
        }
        const uint32_t rank = (uint32_t)__popcll(peers & lt);
        const uint32_t before = valid ? wcnt[wave][d] : 0;  // read by all peers before the leader's write
        slot[r] = before + rank;
        if (valid && rank == 0) wcnt[wave][d] = before + (uint32_t)__popcll(peers);
    }
    int cur = 0;
    for (uint32_t d = 1; d < 256; d <<= 1) {  // tile-local digit starts (the barrier also publishes wcnt)
        scan[cur ^ 1][tid] = scan[cur][tid] + (tid >= d ? scan[cur][tid - d] : 0u);
        cur ^= 1;
        __syncthreads();
    }
    const uint32_t tile_items = scan[cur][255];
    loff[tid] = scan[cur][tid] - cnt;
    gbase[tid] = wb_s + off;
    {  // wave q's run of digit d starts after waves < q's
        uint32_t run = scan[cur][tid] - cnt;
#pragma unroll
        for (int q = 0; q < 4; q++) {
            const uint32_t c = wcnt[q][tid];  // column tid is this thread's alone here
            wcnt[q][tid] = run;
            run += c;
        }
    }
    __syncthreads();
#pragma unroll
    for (uint32_t r = 0; r < kSortIpt; r++) {
        if (keyr[r] < sp.sentinel) {
            const uint32_t d = ((keyr[r] & sp.bmask) >> sp.shift) & 0xff;
            const uint32_t pos = wcnt[wave][d] + slot[r];
            sk[pos] = keyr[r];
            sv[pos] = valr[r];
        }
    }
    __syncthreads();
    for (uint32_t k = tid; k < tile_items; k += 256) {
        const uint32_t key = sk[k];
        const uint32_t d = ((key & sp.bmask) >> sp.shift) & 0xff;
        const size_t pos = (size_t)gbase[d] + (k - loff[d]);
        keys_out[pos] = key;
        vals_out[pos] = sv[k];
    }
}

// Bucket accumulation, load-balanced: lane k owns the sorted items
// [k T, (k+1) T) (T = MsmPlan::T) and adds their bases run by run.  A run whose
// bucket starts inside the chunk is written to the bucket; the chunk's first
// run, when its bucket started in an earlier chunk, goes to cont[k] and is
// folded in by k_msm_bucket_fix.  Every lane does at most T mixed additions
// whatever the digit distribution (a window whose digits crowd into few
// buckets -- the top window of scalars < r -- no longer makes a few lanes
// walk hundreds of terms).
// chunk k0 + i of the window part [w0, w1): its items [k T, (k+1) T) clipped to
// the part's items [jlo, jhi) of the sorted (window-compacted) array, k0 =
// floor(jlo / T).  A window's items start with a new bucket, so a chunk
// straddling two parts is split cleanly (its second piece never writes cont[k]).
PA_DEV bool chunk_range(size_t i, const uint32_t* __restrict__ wpre, uint32_t w0, uint32_t w1, uint32_t T,
                        size_t& k, size_t& j0, size_t& j1) {
    const size_t jlo = wpre[w0], jhi = wpre[w1];
    k = jlo / T + i;
    j0 = k * T;
    j1 = j0 + T;
    if (j0 < jlo) j0 = jlo;
    if (j1 > jhi) j1 = jhi;
    return j0 < j1;
}

// The affine bases converted once per MSM to lazy rows (curve_fl.h's
// fl_pack_row for G1: x, y -> 28 u32, the infinity flag inside, so a bucket
// item gathers ONE 112-byte record; G2: x.c0, x.c1, y.c0, y.c1 -> 56 u32, the
// flag in bit 31 of x.c0's top limb, below 2^18 for F<1>) ...
// The G2 conversion and both prepare kernels keep their own store loops: through
// a shared pack helper the compiler schedules their loads and stores differently.
template <int G> constexpr int kMsmRowWords = 28 * G;
__global__ void __launch_bounds__(256) k_msm_bases_fl(const uint64_t* __restrict__ bases, size_t n,
                                                      uint32_t* __restrict__ fl) {
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    Aff<Fq> a;
    load_aff(a, bases + (size_t)Grp<1>::AW * i);
    fl_pack_row(fl + kMsmRowWords<1> * i, fl_from_abi(a.x), fl_from_abi(a.y), a.inf);
}
__global__ void __launch_bounds__(256) k_msm_bases_fl2(const uint64_t* __restrict__ bases, size_t n,
                                                       uint32_t* __restrict__ fl) {
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    Aff<Fq2> a;
    load_aff(a, bases + (size_t)Grp<2>::AW * i);
    const F<1> v[4] = {fl_from_abi(a.x.c0), fl_from_abi(a.x.c1), fl_from_abi(a.y.c0), fl_from_abi(a.y.c1)};
    uint32_t* d = fl + kMsmRowWords<2> * i;
#pragma unroll
    for (int c = 0; c < 4; c++)
#pragma unroll
        for (int k = 0; k < 14; k++) d[14 * c + k] = v[c].w[k] | (c == 0 && k == 13 && a.inf ? 0x80000000u : 0u);
}

// The prepared rows (launch_msm_prepare, group 1): row i as k_msm_bases_fl writes
// it, row n + i = -phi(P_i) = (beta x_i, -y_i), an infinity base flagged in
// both; the membership flags ok[i] (launch_subgroup_check) counted into *bad.
// beta: kernels_curve.hip's kGlvBeta, the decode kernel's kBeta (Montgomery words)
__constant__ const uint64_t kMsmBeta[6] = {0x30f1361b798a64e8ULL, 0xf3b8ddab7ece5a2aULL, 0x16a8ca3ac61577f7ULL,
                                           0xc26a2ff874fd029bULL, 0x3636b76660701c6eULL, 0x051ba4ab241b6160ULL};
__global__ void __launch_bounds__(256) k_msm_bases_prepare(const uint64_t* __restrict__ bases,
                                                           const uint8_t* __restrict__ ok, size_t n,
                                                           uint32_t* __restrict__ rows, uint32_t* __restrict__ bad) {
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    Aff<Fq> a;
    load_aff(a, bases + (size_t)Grp<1>::AW * i);
    Fq beta, bx, ny;
    fq_load(beta, kMsmBeta);
    mul(bx, a.x, beta);
    neg(ny, a.y);
    const F<1> x = fl_from_abi(a.x), y = fl_from_abi(a.y), px = fl_from_abi(bx), py = fl_from_abi(ny);
    const uint32_t inf = a.inf ? 0x80000000u : 0u;
    uint32_t* d = rows + kMsmRowWords<1> * i;
    uint32_t* e = rows + kMsmRowWords<1> * (n + i);
#pragma unroll
    for (int k = 0; k < 14; k++) {
        d[k] = x.w[k] | (k == 13 ? inf : 0u);
        d[14 + k] = y.w[k];
        e[k] = px.w[k] | (k == 13 ? inf : 0u);
        e[14 + k] = py.w[k];
    }
    if (!ok[i]) atomicAdd(bad, 1u);
}

// The prepared G2 rows (launch_msm_prepare, group 2): row i as k_msm_bases_fl2
// writes it, row n + i = x^2 Q_i = (beta^2 x_i, -y_i) with beta^2 scaling both Fq
// components of x; an infinity base flagged in both; the membership flags
// ok[i] (launch_subgroup_check) counted into *bad.
// kMsmBeta2 is the square of kMsmBeta (Montgomery words), the other primitive
// cube root of unity in Fq.  On G1 (x, y) -> (beta x, y) multiplies by -x^2,
// one root of l^2 + l + 1 = 0 mod r; on the twist's subgroup G2 the same map
// multiplies by the other root, (-x^2)^2 = x^2 - 1, so the map that multiplies
// by -x^2 there, the one the split s = q x^2 + rem needs, is the one with
// beta^2 (tests/test_msm_g2_prepared.py checks it against the oracle).
__constant__ const uint64_t kMsmBeta2[6] = {0xcd03c9e48671f071ULL, 0x5dab22461fcda5d2ULL, 0x587042afd3851b95ULL,
                                            0x8eb60ebe01bacb9eULL, 0x03f97d6e83d050d2ULL, 0x18f0206554638741ULL};
__global__ void __launch_bounds__(256) k_msm_bases_prepare_g2(const uint64_t* __restrict__ bases,
                                                              const uint8_t* __restrict__ ok, size_t n,
                                                              uint32_t* __restrict__ rows,
                                                              uint32_t* __restrict__ bad) {
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    Aff<Fq2> a;
    load_aff(a, bases + (size_t)Grp<2>::AW * i);
    Fq beta2, bx0, bx1, ny0, ny1;
    fq_load(beta2, kMsmBeta2);
    mul(bx0, a.x.c0, beta2);
    mul(bx1, a.x.c1, beta2);
    neg(ny0, a.y.c0);
    neg(ny1, a.y.c1);
    const F<1> v[4] = {fl_from_abi(a.x.c0), fl_from_abi(a.x.c1), fl_from_abi(a.y.c0), fl_from_abi(a.y.c1)};
    const F<1> p[4] = {fl_from_abi(bx0), fl_from_abi(bx1), fl_from_abi(ny0), fl_from_abi(ny1)};
    const uint32_t inf = a.inf ? 0x80000000u : 0u;
    uint32_t* d = rows + kMsmRowWords<2> * i;
    uint32_t* e = rows + kMsmRowWords<2> * (n + i);
#pragma unroll
    for (int c = 0; c < 4; c++)
#pragma unroll
        for (int k = 0; k < 14; k++) {
            const uint32_t flag = c == 0 && k == 13 ? inf : 0u;
            d[14 * c + k] = v[c].w[k] | flag;
            e[14 * c + k] = p[c].w[k] | flag;
        }
    if (!ok[i]) atomicAdd(bad, 1u);
}

// a finished run of one bucket: to the bucket when it starts inside the chunk, else to cont[k]
template <int G>
PA_DEV void msm_flush(uint32_t key, const FlPoint<G>& acc, bool untouched, size_t j0, size_t k,
                      const uint32_t* __restrict__ start, uint64_t* __restrict__ buckets,
                      uint64_t* __restrict__ cont) {
    constexpr int JW = Grp<G>::JW;
    fl_store_jac_or_zero(start[key] >= j0 ? buckets + (size_t)JW * key : cont + (size_t)JW * k, acc, untouched);
}

// ... and the bucket accumulation with the lazy mixed addition (curve_fl.h);
// bucket pieces leave in the ABI form the later phases read.  One wave per SIMD
// (256 VGPRs + 75 AGPRs): the next item's base is gathered while the current
// addition runs (two waves per SIMD spilled 42-84 registers and measured 1-10 %
// slower).
PA_DEV void chunk_acc_fl_body(const uint32_t* __restrict__ basefl, const uint32_t* __restrict__ keys,
                              const uint32_t* __restrict__ vals, const uint32_t* __restrict__ start,
                              const uint32_t* __restrict__ wpre, uint32_t w0, uint32_t w1, uint32_t T,
                              uint32_t sentinel, uint64_t* __restrict__ buckets, uint64_t* __restrict__ cont) {
    size_t k, j0, j1;
    if (!chunk_range((size_t)blockIdx.x * blockDim.x + threadIdx.x, wpre, w0, w1, T, k, j0, j1)) return;
    uint32_t cur = keys[j0];
    if (cur >= sentinel) return;
    FlJac acc = FlJac::zero();
    bool untouched = true;
    // software pipeline: the (key, value) pair two items ahead and the base
    // of the next item are in flight while the current mixed addition runs
    // (the bucket phase is bound by these dependent random gathers)
    auto fetch = [&](size_t jj, uint32_t& kk, uint32_t& vv) {
        kk = sentinel;
        vv = 0;
        if (jj < j1) {
            kk = keys[jj];
            vv = vals[jj];
        }
    };
    auto gather = [&](uint32_t kk, uint32_t vv, F<1>& x, F<1>& y, bool& inf) {
        inf = true;
        if (kk < sentinel) fl_gather_row(basefl + kMsmRowWords<1> * (size_t)(vv & 0x7fffffffu), x, y, inf);
    };
    uint32_t key0, v0, key1, v1;
    fetch(j0, key0, v0);
    fetch(j0 + 1, key1, v1);
    F<1> tx, ty;
    bool inf;
    gather(key0, v0, tx, ty, inf);
#pragma unroll 1
    for (size_t j = j0; j < j1; j++) {
        if (key0 >= sentinel) break;
        uint32_t key2, v2;
        fetch(j + 2, key2, v2);
        F<1> nx, ny;
        bool ninf;
        gather(key1, v1, nx, ny, ninf);
        if (key0 != cur) {
            msm_flush<1>(cur, acc, untouched, j0, k, start, buckets, cont);
            untouched = true;
            cur = key0;
        }
        if (!inf) {  // an infinity base is add_assign_mixed's no-op
            const F<2> oy = (v0 >> 31) ? neg(ty) : relax<2>(ty);
            fl_jac_add_mixed(acc, untouched, tx, oy);
        }
        key0 = key1;
        v0 = v1;
        key1 = key2;
        v1 = v2;
        tx = nx;
        ty = ny;
        inf = ninf;
    }
    msm_flush<1>(cur, acc, untouched, j0, k, start, buckets, cont);
}
__global__ void __launch_bounds__(64) k_msm_chunk_acc_fl(const uint32_t* __restrict__ basefl,
                                                         const uint32_t* __restrict__ keys,
                                                         const uint32_t* __restrict__ vals,
                                                         const uint32_t* __restrict__ start,
                                                         const uint32_t* __restrict__ wpre, uint32_t w0, uint32_t w1,
                                                         uint32_t T, uint32_t sentinel,
                                                         uint64_t* __restrict__ buckets, uint64_t* __restrict__ cont) {
    chunk_acc_fl_body(basefl, keys, vals, start, wpre, w0, w1, T, sentinel, buckets, cont);
}

// One lane per bucket: empty buckets become the identity; a bucket spanning
// several chunks adds the continuation pieces of the chunks after its first.
template <int G>
__global__ void __launch_bounds__(64) k_msm_bucket_fix(const uint32_t* __restrict__ start,
                                                       const uint32_t* __restrict__ end, size_t b0, size_t b1,
                                                       uint32_t T, const uint64_t* __restrict__ cont,
                                                       uint64_t* __restrict__ buckets,
                                                       uint32_t* __restrict__ long_list,
                                                       uint32_t* __restrict__ long_count, size_t long_span) {
    using F = typename Grp<G>::F;
    constexpr int JW = Grp<G>::JW;
    const size_t b = b0 + (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (b >= b1) return;
    const uint32_t s = start[b], e = end[b];
    if (s == e) {
        Jac<F> z;
        jac_zero(z);
        store_jac(buckets + (size_t)JW * b, z);
        return;
    }
    const size_t first = s / T, last = (e - 1) / T;
    if (first == last) return;
    if (long_list && last - first > long_span) {   // k_msm_long_fix folds it, a block per bucket
        long_list[atomicAdd(long_count, 1u)] = (uint32_t)b;
        return;
    }
    FlPoint<G> acc = fl_load_jac<G>(buckets + (size_t)JW * b);   // lazy core, same formulas and values
#pragma unroll 1
    for (size_t k = first + 1; k <= last; k++) fl_jac_add(acc, fl_load_jac<G>(cont + (size_t)JW * k));
    fl_store_jac(buckets + (size_t)JW * b, acc);
}

// out[w*stride + g] = sum_{k<group} in[w*stride + g*group + k]  (indices < count),
// windows [w0, w1); the fixed per-window stride keeps the window parts' levels
// apart.  G1: one quad per output (fl_jac_add_q).
__global__ void __launch_bounds__(64) k_msm_group_sum_fl(const uint64_t* __restrict__ in, uint32_t count,
                                                         uint32_t group, uint32_t gpw, uint32_t w0, uint32_t w1,
                                                         uint32_t stride, uint64_t* __restrict__ out) {
    constexpr int JW = Grp<1>::JW;
    const size_t t = (size_t)w0 * gpw + (((size_t)blockIdx.x * blockDim.x + threadIdx.x) >> 2);
    const int q = threadIdx.x & 3;
    if (t >= (size_t)w1 * gpw) return;
    const size_t w = t / gpw;
    const uint32_t g = (uint32_t)(t % gpw);
    FlJac acc = FlJac::zero();
#pragma unroll 1
    for (uint32_t k = 0; k < group; k++) {
        const uint32_t idx = g * group + k;
        if (idx >= count) break;
        fl_jac_add_q(acc, fl_load_jac(in + (size_t)JW * (w * stride + idx)), q);
    }
    if (q == 0) fl_store_jac(out + (size_t)JW * (w * stride + g), acc);
}

// Horner on a group of lane quads (dec_quad.h; G1: 4 quads, G2: 8 quads): each
// doubling is three levels of side-by-side products (one per quad, G2 one
// Fq2 coordinate per quad) instead of the three-lane doubling's chain, and a
// quad product is ~2.5x shorter than a one-lane leaf: the 256 doublings of the
// top window are the MSM's longest dependent chain.  Same sum as a point.
PA_DEV void load_jac_q(dq::Jq<dq::Q>& r, const uint64_t* p, const dq::Lc& l) {
    Fq x, y, z;
    fq_load(x, p);
    fq_load(y, p + 6);
    fq_load(z, p + 12);
    r = {dq::from_abi(x, l), dq::from_abi(y, l), dq::from_abi(z, l)};
}
PA_DEV void load_jac_q(dq::Jq<dq::Q2>& r, const uint64_t* p, const dq::Lc& l) {
    Fq v[6];
#pragma unroll
    for (int k = 0; k < 6; k++) fq_load(v[k], p + 6 * k);
    r.x = {dq::from_abi(v[0], l), dq::from_abi(v[1], l)};
    r.y = {dq::from_abi(v[2], l), dq::from_abi(v[3], l)};
    r.z = {dq::from_abi(v[4], l), dq::from_abi(v[5], l)};
}
PA_DEV void store_jac_q(uint64_t* p, const dq::Jq<dq::Q>& a, bool lead) {
    const Fq x = dq::to_abi(a.x), y = dq::to_abi(a.y), z = dq::to_abi(a.z);
    if (lead) {
        fq_store(p, x);
        fq_store(p + 6, y);
        fq_store(p + 12, z);
    }
}
PA_DEV void store_jac_q(uint64_t* p, const dq::Jq<dq::Q2>& a, bool lead) {
    const Fq v[6] = {dq::to_abi(a.x.c0), dq::to_abi(a.x.c1), dq::to_abi(a.y.c0),
                     dq::to_abi(a.y.c1), dq::to_abi(a.z.c0), dq::to_abi(a.z.c1)};
    if (lead)
#pragma unroll
        for (int k = 0; k < 6; k++) fq_store(p + 6 * k, v[k]);
}
// Windows [wlo, whi) top down: from acc_in (the part above, doubled c times
// first) or, without one, from S_(whi-1).
template <int G>
__global__ void __launch_bounds__(64) k_msm_horner_q(const uint64_t* __restrict__ wsum, uint32_t stride, int whi,
                                                     int wlo, uint32_t c, const uint64_t* __restrict__ acc_in,
                                                     uint64_t* __restrict__ out) {
    constexpr int NQ = G == 1 ? 4 : 8;
    constexpr int JW = Grp<G>::JW;
    using E = typename std::conditional<G == 1, dq::Jq<dq::Q>, dq::Jq<dq::Q2>>::type;
    const int lane = threadIdx.x;
    if (blockIdx.x != 0 || lane >= 4 * NQ) return;   // one group
    const dq::Lc l = dq::lctx(lane, NQ);
    E acc;
    int w = whi - 1;
    if (acc_in) {
        load_jac_q(acc, acc_in, l);
    } else {
        load_jac_q(acc, wsum + (size_t)JW * stride * w, l);
        w--;
    }
#pragma unroll 1
    for (; w >= wlo; w--) {
        if (!dq::is_zero(acc.z)) {
#pragma unroll 1
            for (uint32_t k = 0; k < c; k++) dq::jdbl<NQ>(acc, l);
        }
        E x;
        load_jac_q(x, wsum + (size_t)JW * stride * w, l);
        if (!dq::is_zero(x.z)) dq::jadd<NQ>(acc, dq::make_fixed<NQ>(x, l), l);
    }
    store_jac_q(out, acc, lane == 0);
}

// The batch's Horner: vector j of [j0, j1) on its own group of quads (G1: 4
// quads, four groups per wave; G2: 8 quads, two per wave), over its windows
// j W + w from the top down as k_msm_horner_q does; the point goes to
// out + JW j.  A vector whose window sums are all zero keeps the zero point
// it loaded.
template <int G> constexpr unsigned kHornerPerWave = G == 1 ? 4 : 2;
template <int G>
__global__ void __launch_bounds__(64) k_msm_horner_batch_q(const uint64_t* __restrict__ wsum, uint32_t stride,
                                                           uint32_t W, uint32_t c, size_t j0, size_t j1,
                                                           uint64_t* __restrict__ out) {
    constexpr int NQ = G == 1 ? 4 : 8, L = 4 * NQ, JW = Grp<G>::JW;
    using E = typename std::conditional<G == 1, dq::Jq<dq::Q>, dq::Jq<dq::Q2>>::type;
    static_assert(64 / L == kHornerPerWave<G>, "groups per wave");
    const int lane = threadIdx.x;
    const size_t j = j0 + (size_t)blockIdx.x * kHornerPerWave<G> + lane / L;
    if (j >= j1) return;   // whole groups leave together
    const dq::Lc l = dq::lctx(lane, NQ);
    const uint64_t* ws = wsum + (size_t)JW * stride * (j * W);
    E acc;
    load_jac_q(acc, ws + (size_t)JW * stride * (W - 1), l);
#pragma unroll 1
    for (int w = (int)W - 2; w >= 0; w--) {
        if (!dq::is_zero(acc.z)) {
#pragma unroll 1
            for (uint32_t k = 0; k < c; k++) dq::jdbl<NQ>(acc, l);
        }
        E x;
        load_jac_q(x, ws + (size_t)JW * stride * w, l);
        if (!dq::is_zero(x.z)) dq::jadd<NQ>(acc, dq::make_fixed<NQ>(x, l), l);
    }
    store_jac_q(out + (size_t)JW * j, acc, lane % L == 0);
}

// One lane per segment of L buckets of one window: sum_m m * B_m over the
// segment, by running sums top down (T += B_m; S += T) plus a * T for the
// segment's offset a.
template <int G>
__global__ void __launch_bounds__(64) k_msm_segments(const uint64_t* __restrict__ buckets, uint32_t B, uint32_t L,
                                                     size_t t0, size_t t1, uint64_t* __restrict__ segs) {
    // one lane per segment: the kernel is throughput bound (4 k waves); a G1 quad
    // per segment (fl_jac_add_q) measured 0.57 -> 1.29 ms (profiles/r03_msm_quad_ab.txt)
    constexpr int JW = Grp<G>::JW;
    const size_t t = t0 + (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= t1) return;
    const uint32_t spw = B / L;
    const size_t w = t / spw;
    const uint32_t j = (uint32_t)(t % spw);
    const uint64_t* bw = buckets + (size_t)JW * (w * B);
    FlPoint<G> T = FlPoint<G>::zero(), S = T;
#pragma unroll 1
    for (uint32_t m = (j + 1) * L; m > j * L; m--) {  // magnitudes (j*L, (j+1)*L], top down
        fl_jac_add(T, fl_load_jac<G>(bw + (size_t)JW * (m - 1)));
        fl_jac_add(S, T);
    }
    const uint32_t a = j * L;  // S = sum (m - a) B_m; add a * T
    if (a && !fl_is_zero(T.z)) {
        FlPoint<G> aT = T;  // top set bit of a
        const int top = 31 - __clz(a);
#pragma unroll 1
        for (int bit = top - 1; bit >= 0; bit--) {
            fl_jac_double(aT);
            if ((a >> bit) & 1) fl_jac_add(aT, T);
        }
        fl_jac_add(S, aT);
    }
    fl_store_jac(segs + (size_t)JW * t, S);
}


// ---- G2's own bucket phases on the lazy core's Fq2 (curve_fl2.h) ----
// The bucket accumulation with the lazy mixed addition; the (key, value) pair
// of the next item in flight while the current addition runs (a prefetched
// 224-byte base would not fit beside the Fq2 temporaries)
__global__ void __launch_bounds__(64) k_msm_chunk_acc_fl2(const uint32_t* __restrict__ basefl,
                                                          const uint32_t* __restrict__ keys,
                                                          const uint32_t* __restrict__ vals,
                                                          const uint32_t* __restrict__ start,
                                                          const uint32_t* __restrict__ wpre, uint32_t w0, uint32_t w1,
                                                          uint32_t T, uint32_t sentinel,
                                                          uint64_t* __restrict__ buckets, uint64_t* __restrict__ cont) {
    size_t k, j0, j1;
    if (!chunk_range((size_t)blockIdx.x * blockDim.x + threadIdx.x, wpre, w0, w1, T, k, j0, j1)) return;
    uint32_t cur = keys[j0];
    if (cur >= sentinel) return;
    FlJac2 acc = FlJac2::zero();
    bool untouched = true;
    uint32_t key = cur, v = vals[j0];
#pragma unroll 1
    for (size_t j = j0; j < j1; j++) {
        if (key >= sentinel) break;
        uint32_t nkey = sentinel, nv = 0;
        if (j + 1 < j1) {
            nkey = keys[j + 1];
            nv = vals[j + 1];
        }
        if (key != cur) {
            msm_flush<2>(cur, acc, untouched, j0, k, start, buckets, cont);
            untouched = true;
            cur = key;
        }
        // the row as k_msm_bases_fl2 wrote it, gathered inline (as k_comb_mul_fl2 does): through a
        // shared helper this kernel's registers are allocated differently
        const uint2* src = reinterpret_cast<const uint2*>(basefl + kMsmRowWords<2> * (size_t)(v & 0x7fffffffu));
        F<1> c[4];
#pragma unroll
        for (int q = 0; q < 28; q++) {
            const uint2 t = src[q];
            c[q / 7].w[2 * (q % 7)] = t.x;
            c[q / 7].w[2 * (q % 7) + 1] = t.y;
        }
        const bool inf = (c[0].w[13] >> 31) != 0;
        c[0].w[13] &= 0x7fffffffu;
        if (!inf) {  // an infinity base is add_assign_mixed's no-op
            const F2<1> y = {c[2], c[3]};
            const F2<2> oy = (v >> 31) ? neg(y) : relax<2>(y);
            fl_jac_add_mixed(acc, untouched, F2<1>{c[0], c[1]}, oy);
        }
        key = nkey;
        v = nv;
    }
    msm_flush<2>(cur, acc, untouched, j0, k, start, buckets, cont);
}

// k_msm_group_sum_fl over Fq2, one lane per output
__global__ void __launch_bounds__(64) k_msm_group_sum_fl2(const uint64_t* __restrict__ in, uint32_t count,
                                                          uint32_t group, uint32_t gpw, uint32_t w0, uint32_t w1,
                                                          uint32_t stride, uint64_t* __restrict__ out) {
    constexpr int JW = Grp<2>::JW;
    const size_t t = (size_t)w0 * gpw + (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= (size_t)w1 * gpw) return;
    const size_t w = t / gpw;
    const uint32_t g = (uint32_t)(t % gpw);
    FlJac2 acc = FlJac2::zero();
#pragma unroll 1
    for (uint32_t k = 0; k < group; k++) {
        const uint32_t idx = g * group + k;
        if (idx >= count) break;
        fl_jac_add(acc, fl_load_jac<2>(in + (size_t)JW * (w * stride + idx)));
    }
    fl_store_jac(out + (size_t)JW * (w * stride + g), acc);
}

// Buckets spanning more than kMsmLongSpan chunks (crowded digits: equal
// scalars, the carry-only top window of c-bit windows above bit 255): one
// block per bucket, each thread summing a strided share of the continuation
// pieces, then a tree through LDS; the bucket's own piece is added last.  The
// list comes from k_msm_bucket_fix; without long buckets the blocks exit at
// once.  Without it one lane walked every piece (G2 at 2^18: 46 ms).
template <int G> constexpr int kMsmLongFixThreads = G == 1 ? 256 : 128;
template <int G>
__global__ void __launch_bounds__(kMsmLongFixThreads<G>) k_msm_long_fix(const uint32_t* __restrict__ start,
                                                                        const uint32_t* __restrict__ end, uint32_t T,
                                                                        const uint64_t* __restrict__ cont,
                                                                        uint64_t* __restrict__ buckets,
                                                                        const uint32_t* __restrict__ long_list,
                                                                        const uint32_t* __restrict__ long_count) {
    using P = FlPoint<G>;
    constexpr int NT = kMsmLongFixThreads<G>, JW = Grp<G>::JW, PW = sizeof(P) / 4;
    __shared__ uint32_t sh[(NT / 2) * PW];
    const int t = threadIdx.x;
    const uint32_t count = *long_count;
#pragma unroll 1
    for (uint32_t idx = blockIdx.x; idx < count; idx += gridDim.x) {
        const uint32_t b = long_list[idx];
        const size_t first = start[b] / T, last = (end[b] - 1) / T;
        P acc = P::zero();
#pragma unroll 1
        for (size_t k = first + 1 + t; k <= last; k += NT) fl_jac_add(acc, fl_load_jac<G>(cont + (size_t)JW * k));
#pragma unroll 1
        for (int h = NT / 2; h >= 1; h >>= 1) {
            if (t >= h && t < 2 * h) {
                const uint32_t* src = reinterpret_cast<const uint32_t*>(&acc);
#pragma unroll
                for (int q = 0; q < PW; q++) sh[(t - h) * PW + q] = src[q];
            }
            __syncthreads();
            if (t < h) {
                P o;
                uint32_t* dst = reinterpret_cast<uint32_t*>(&o);
#pragma unroll
                for (int q = 0; q < PW; q++) dst[q] = sh[t * PW + q];
                fl_jac_add(acc, o);
            }
            __syncthreads();
        }
        if (t == 0) {
            P bk = fl_load_jac<G>(buckets + (size_t)JW * b);
            fl_jac_add(bk, acc);
            fl_store_jac(buckets + (size_t)JW * b, bk);
        }
    }
}

template <int G>
__global__ void __launch_bounds__(64) k_jac_zero_out(uint64_t* __restrict__ out, size_t count) {
    using F = typename Grp<G>::F;
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= count) return;
    Jac<F> z;
    jac_zero(z);
    store_jac(out + (size_t)Grp<G>::JW * i, z);
}

static inline unsigned msm_blocks(size_t n, unsigned bs) { return (unsigned)((n + bs - 1) / bs); }

size_t msm_workspace_bytes(int group, size_t n) {
    if (n == 0) return 0;
    MsmPlan p;
    if (msm_plan(p, group, n) != hipSuccess) return 0;
    return p.total;
}
size_t msm_prepared_rows_bytes(size_t n, int group) { return 2 * n * (group == 1 ? 28 : 56) * sizeof(uint32_t); }
size_t msm_prepared_workspace_bytes(size_t m, bool glv, int group) {
    if (m == 0) return 0;
    MsmPlan p;
    if (msm_plan(p, group, glv ? 2 * m : m, glv, false) != hipSuccess) return 0;
    return p.total;
}
bool msm_prepared_batch_fits(size_t m, size_t k, bool glv, int group) {
    if (m == 0 || k == 0) return true;
    MsmPlan p;
    return msm_plan(p, group, glv ? 2 * m : m, glv, false, k) == hipSuccess && p.fits;
}
size_t msm_prepared_batch_workspace_bytes(size_t m, size_t k, bool glv, int group) {
    if (m == 0 || k == 0) return 0;
    MsmPlan p;
    if (msm_plan(p, group, glv ? 2 * m : m, glv, false, k) != hipSuccess || !p.fits) return 0;
    return p.total;
}

// two non-blocking side streams per device (bucket reduction, Horner legs),
// created on the device of the caller's stream.  They are shared by every
// caller on that device, so MSMs issued concurrently from several host threads
// serialize their window-part tails through them (results are unaffected: each
// call orders its own work with events).
static hipError_t msm_side_streams(hipStream_t caller, hipStream_t out[2]) {
    int dev = 0;
    hipError_t e = hipStreamGetDevice(caller, &dev);
    if (e != hipSuccess) return e;
    if (dev < 0 || dev >= 64) return hipErrorInvalidDevice;
    static std::mutex mu;
    static hipStream_t side[64][2] = {};
    std::lock_guard<std::mutex> g(mu);
    // the side streams at the highest priority: a part's reduction waves are
    // dispatched as the next part's accumulation frees SIMDs
    int lo = 0, hi = 0;
    if ((e = hipDeviceGetStreamPriorityRange(&lo, &hi)) != hipSuccess) return e;
    if (!side[dev][0] || !side[dev][1]) {
        // streams belong to the current device: create them on the caller's
        int cur = 0;
        if ((e = hipGetDevice(&cur)) != hipSuccess) return e;
        if (cur != dev && (e = hipSetDevice(dev)) != hipSuccess) return e;
        for (int k = 0; k < 2 && e == hipSuccess; k++)
            if (!side[dev][k]) e = hipStreamCreateWithPriority(&side[dev][k], hipStreamNonBlocking, hi);
        if (cur != dev) (void)hipSetDevice(cur);
        if (e != hipSuccess) return e;
    }
    out[0] = side[dev][0];
    out[1] = side[dev][1];
    return hipSuccess;
}

// What one MSM sums: `terms` scalars over affine ABI records converted per call
// (bases; the plain entries), or over prepared lazy rows (rows): the
// 257-bit digits over rows [0, terms), or with glv the two virtual terms per
// scalar over rows i and row_off + i.
struct MsmJob {
    const uint64_t* bases;
    const uint32_t* rows;
    const uint64_t* scalars;
    size_t terms;
    size_t row_off;
    bool glv;
    size_t vectors = 1;   // scalar vectors of `terms` rows end to end, one output each
    bool mont = false;    // the scalar rows are Montgomery Fr (< r), not FrRepr
    bool u128 = false;    // the scalar rows are 16 bytes (< 2^128): the 130-bit plan over `terms` real terms
};

// The kernels that differ by group: the base conversions (their store loops),
// of steps 4-6 the accumulation (G1: a two-deep prefetch) and the group sum
// (G1: a quad per output), and the lanes that group_sum spends per output
template <int G> struct MsmKernels;
template <> struct MsmKernels<1> {
    static constexpr auto bases_fl = k_msm_bases_fl;
    static constexpr auto bases_prepare = k_msm_bases_prepare;
    static constexpr auto chunk_acc = k_msm_chunk_acc_fl;
    static constexpr auto group_sum = k_msm_group_sum_fl;
    static constexpr unsigned kGroupSumLanes = 4;
};
template <> struct MsmKernels<2> {
    static constexpr auto bases_fl = k_msm_bases_fl2;
    static constexpr auto bases_prepare = k_msm_bases_prepare_g2;
    static constexpr auto chunk_acc = k_msm_chunk_acc_fl2;
    static constexpr auto group_sum = k_msm_group_sum_fl2;
    static constexpr unsigned kGroupSumLanes = 1;
};

// segment sums -> one per window, two at a time: shallow chains, 2 additions per
// level; a fan-in of 2 / 3 / 4 / 8 measured 141.6 / 140.2 / 138.1 / 133.5 M terms/s
// at 2^20 (profiles/r02_msm_tuning.txt)
constexpr uint32_t kMsmGroup = 2;

// The plan's workspace as the stages address it.  keys / vals: the sorted items
// (msm_sort_items); basefl: the lazy base rows, the job's prepared ones or the
// workspace's own.
struct MsmWs {
    uint32_t *keys_in, *keys_out, *vals_in, *vals_out, *start, *end, *hist, *wtot, *wpre;
    uint64_t *buckets, *segs, *tmp, *cont, *hacc;
    uint32_t *long_list, *long_count;   // part q: its list at long_list + b0, its count at long_count[q]
    uint32_t* own_basefl;
    const uint32_t *keys, *vals, *basefl;
};
static MsmWs msm_ws(const MsmPlan& p, const MsmJob& job, void* ws) {
    char* base = static_cast<char*>(ws);
    auto u32 = [&](size_t off) { return reinterpret_cast<uint32_t*>(base + off); };
    auto u64 = [&](size_t off) { return reinterpret_cast<uint64_t*>(base + off); };
    MsmWs w{};
    w.keys_in = u32(p.off_keys_in);
    w.keys_out = u32(p.off_keys_out);
    w.vals_in = u32(p.off_vals_in);
    w.vals_out = u32(p.off_vals_out);
    w.start = u32(p.off_start);
    w.end = u32(p.off_end);
    w.hist = u32(p.off_hist);
    w.wtot = u32(p.off_wtot);
    w.wpre = u32(p.off_wpre);
    w.buckets = u64(p.off_buckets);
    w.segs = u64(p.off_segs);
    w.tmp = u64(p.off_tmp);
    w.cont = u64(p.off_cont);
    w.hacc = u64(p.off_hacc);
    w.long_list = u32(p.off_long);
    w.long_count = w.long_list + p.WT * p.B;
    w.own_basefl = u32(p.off_basefl);
    w.basefl = job.rows ? job.rows : w.own_basefl;
    return w;
}

// Steps 1-2: the digits of every window, then the bucketing sort, ping-pong
// between the _in and _out arrays; the last destination's tail past the nonzero
// items is set to sentinel keys first.  n: items per window.
static hipError_t msm_sort_items(const MsmJob& job, const MsmPlan& p, size_t n, MsmWs& w, hipStream_t s) {
    const uint32_t WT = (uint32_t)p.WT, sentinel = WT * p.B;
    if (job.u128)
        hipLaunchKernelGGL(k_msm_digits_u128, dim3(msm_blocks(n, 256)), dim3(256), 0, s, job.scalars, n, p.c, p.W, p.B,
                           sentinel, w.keys_in, w.vals_in);
    else if (job.glv)
        hipLaunchKernelGGL(k_msm_digits_glv, dim3(msm_blocks(job.terms * job.vectors, 256)), dim3(256), 0, s,
                           job.scalars, job.terms, job.vectors, job.mont, (uint32_t)job.row_off, p.c, p.W, p.B,
                           sentinel, w.keys_in, w.vals_in);
    else
        hipLaunchKernelGGL(k_msm_digits, dim3(msm_blocks(n * job.vectors, 256)), dim3(256), 0, s, job.scalars, n,
                           job.vectors, job.mont, p.c, p.W, p.B, sentinel, w.keys_in, w.vals_in);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
    uint32_t *ksrc = w.keys_in, *vsrc = w.vals_in, *kdst = w.keys_out, *vdst = w.vals_out;
    const unsigned tiles = WT * p.tpw;
    for (uint32_t pass = 0; pass < p.passes; pass++) {
        const SortPass sp{8 * pass, p.B - 1, sentinel, p.tpw, pass == 0 ? 1u : 0u, n};
        hipLaunchKernelGGL(k_sort_hist, dim3(tiles), dim3(256), 0, s, ksrc, w.wtot, w.wpre, sp, w.hist);
        hipLaunchKernelGGL(k_sort_scan, dim3(WT), dim3(1024), 0, s, w.hist, p.tpw, w.wtot);
        if (pass == 0)   // the same totals after every pass
            hipLaunchKernelGGL(k_sort_wprefix, dim3(1), dim3(WT <= 64 ? 64 : 1024), 0, s, w.wtot, WT, w.wpre);
        if (pass + 1 == p.passes && (e = hipMemsetAsync(kdst, 0xff, 4 * p.items, s)) != hipSuccess) return e;
        hipLaunchKernelGGL(k_sort_scatter, dim3(tiles), dim3(256), 0, s, ksrc, vsrc, w.hist, w.wtot, w.wpre, sp, kdst,
                           vdst);
        std::swap(ksrc, kdst);
        std::swap(vsrc, vdst);
    }
    w.keys = ksrc;   // the last pass's output
    w.vals = vsrc;
    return hipSuccess;
}

// Step 3, and the plain entries' bases converted to lazy rows
template <int G>
static hipError_t msm_bounds_and_bases(const MsmJob& job, const MsmPlan& p, size_t n, const MsmWs& w, hipStream_t s) {
    const size_t nb = p.WT * p.B;
    hipError_t e;
    if ((e = hipMemsetAsync(w.start, 0, 4 * nb, s)) != hipSuccess) return e;
    if ((e = hipMemsetAsync(w.end, 0, 4 * nb, s)) != hipSuccess) return e;
    hipLaunchKernelGGL(k_msm_bucket_bounds, dim3(msm_blocks(p.items, 256)), dim3(256), 0, s, w.keys, p.items,
                       (uint32_t)(p.WT * p.B), w.start, w.end);
    if (!job.rows)
        hipLaunchKernelGGL(MsmKernels<G>::bases_fl, dim3(msm_blocks(n, 256)), dim3(256), 0, s, job.bases, n,
                           w.own_basefl);
    return hipGetLastError();
}

// Steps 4-6 over the windows [w0, w1) of one part, as both schedulers launch them
template <int G>
struct MsmStages {
    using K = MsmKernels<G>;
    const MsmPlan& p;
    const MsmWs& w;
    size_t n;           // items per window
    uint32_t sentinel, spw;
    size_t long_span;   // chunks above which k_msm_long_fix folds a bucket
    uint64_t* wsum;     // where the last group-sum level leaves the window sums

    MsmStages(const MsmPlan& plan, const MsmWs& ws, size_t items_per_window, bool glv)
        : p(plan), w(ws), n(items_per_window), sentinel((uint32_t)(plan.WT * plan.B)), spw(plan.B / plan.L),
          long_span(kMsmLongSpan), wsum(ws.segs) {
        if (glv) {
            const size_t even = 2 * (n / ((size_t)p.B * p.T) + 1);
            long_span = msm_long_span_glv() > even ? msm_long_span_glv() : even;
        }
        // every part takes the same number of levels (ping-pong segs <-> tmp), so
        // the window sums of all of them land in the same buffer
        for (uint32_t count = spw; count > 1; count = (count + kMsmGroup - 1) / kMsmGroup)
            wsum = wsum == w.segs ? w.tmp : w.segs;
    }

    // the part's item range is on the device (wpre): lanes for the most it can hold
    hipError_t accumulate(uint32_t w0, uint32_t w1, hipStream_t st) const {
        const size_t chunks = ((size_t)(w1 - w0) * n + p.T - 1) / p.T + 1;
        hipLaunchKernelGGL(K::chunk_acc, dim3(msm_blocks(chunks, 64)), dim3(64), 0, st, w.basefl, w.keys, w.vals,
                           w.start, w.wpre, w0, w1, p.T, sentinel, w.buckets, w.cont);
        return hipGetLastError();
    }

    // buckets -> window sums; q: the part's slot for its long-bucket count
    hipError_t reduce(uint32_t w0, uint32_t w1, uint32_t q, hipStream_t st) const {
        const size_t b0 = (size_t)w0 * p.B, b1 = (size_t)w1 * p.B;
        hipError_t r;
        if ((r = hipMemsetAsync(w.long_count + q, 0, 4, st)) != hipSuccess) return r;
        hipLaunchKernelGGL(k_msm_bucket_fix<G>, dim3(msm_blocks(b1 - b0, 64)), dim3(64), 0, st, w.start, w.end, b0, b1,
                           p.T, w.cont, w.buckets, w.long_list + b0, w.long_count + q, long_span);
        hipLaunchKernelGGL(k_msm_long_fix<G>, dim3(kMsmLongBlocks), dim3(kMsmLongFixThreads<G>), 0, st, w.start, w.end,
                           p.T, w.cont, w.buckets, w.long_list + b0, w.long_count + q);
        const size_t t0 = (size_t)w0 * spw, t1 = (size_t)w1 * spw;
        hipLaunchKernelGGL(k_msm_segments<G>, dim3(msm_blocks(t1 - t0, 64)), dim3(64), 0, st, w.buckets, p.B, p.L, t0,
                           t1, w.segs);
        uint64_t *src = w.segs, *dst = w.tmp;
        for (uint32_t count = spw; count > 1;) {
            const uint32_t gpw = (count + kMsmGroup - 1) / kMsmGroup;
            const size_t outs = (size_t)(w1 - w0) * gpw;
            hipLaunchKernelGGL(K::group_sum, dim3(msm_blocks(K::kGroupSumLanes * outs, 64)), dim3(64), 0, st, src,
                               count, kMsmGroup, gpw, w0, w1, spw, dst);
            count = gpw;
            std::swap(src, dst);
        }
        return hipGetLastError();
    }
};

// The events of one scheduled call, the first error of its launch sequence, and
// what a failed sequence owes the caller before it returns
struct MsmEvents {
    hipEvent_t ev[2 * kMsmMaxParts + 1] = {};
    int made = 0;
    hipError_t err = hipSuccess;

    explicit MsmEvents(int count) {
        for (; made < count; made++)
            if (!ck(hipEventCreateWithFlags(&ev[made], hipEventDisableTiming))) break;
    }
    ~MsmEvents() {
        for (int k = 0; k < made; k++) (void)hipEventDestroy(ev[k]);
    }
    MsmEvents(const MsmEvents&) = delete;
    MsmEvents& operator=(const MsmEvents&) = delete;

    // latches the first error; false from then on
    bool ck(hipError_t x) {
        if (err == hipSuccess) err = x;
        return err == hipSuccess;
    }
    // After a failed launch sequence, let this call's work already queued on
    // the side streams drain before the caller may release the workspace (an
    // event recorded now waits for that work only, not for what other callers
    // queue on the shared side streams later).  Returns the first error.
    hipError_t finish(const hipStream_t (&side)[2]) {
        if (err != hipSuccess)
            for (hipStream_t x : side) {
                hipEvent_t done = nullptr;
                if (hipEventCreateWithFlags(&done, hipEventDisableTiming) == hipSuccess &&
                    hipEventRecord(done, x) == hipSuccess)
                    (void)hipEventSynchronize(done);
                else
                    (void)hipStreamSynchronize(x);
                if (done) (void)hipEventDestroy(done);
            }
        return err;
    }
};

// A batch: parts are ranges of vectors, [v0, v1) = windows [v0 W, v1 W), so
// every vector's Horner chain completes inside its part (k_msm_horner_batch_q
// writes out + JW j) and nothing is carried between parts.  One part by
// default (msm_parts_batch).  With more, the caller's stream accumulates part
// after part; the reduction and Horner grid of every part but the last run
// behind it on the side streams, in turn.
template <int G>
static hipError_t msm_schedule_batch(const MsmStages<G>& st, size_t k, uint64_t* out, hipStream_t s) {
    const MsmPlan& p = st.p;
    const uint32_t parts = msm_parts_batch(k);
    auto horner = [&](size_t v0, size_t v1, hipStream_t hs) {
        hipLaunchKernelGGL(k_msm_horner_batch_q<G>, dim3(msm_blocks(v1 - v0, kHornerPerWave<G>)), dim3(64), 0, hs,
                           st.wsum, st.spw, p.W, p.c, v0, v1, out);
        return hipGetLastError();
    };
    hipError_t e;
    if (parts == 1) {
        const uint32_t WT = (uint32_t)p.WT;
        if ((e = st.accumulate(0, WT, s)) != hipSuccess || (e = st.reduce(0, WT, 0, s)) != hipSuccess) return e;
        return horner(0, k, s);
    }
    hipStream_t side[2];
    if ((e = msm_side_streams(s, side)) != hipSuccess) return e;
    MsmEvents ev(2 * (int)(parts - 1));   // ev[2q]: part q accumulated; ev[2q + 1]: its outputs written
    for (uint32_t q = 0; q < parts && ev.err == hipSuccess; q++) {
        const size_t v0 = k * q / parts, v1 = k * (q + 1) / parts;
        const uint32_t w0 = (uint32_t)v0 * p.W, w1 = (uint32_t)v1 * p.W;
        if (!ev.ck(st.accumulate(w0, w1, s))) break;
        if (q + 1 == parts) {
            if (ev.ck(st.reduce(w0, w1, q, s))) ev.ck(horner(v0, v1, s));
            break;
        }
        hipStream_t qs = side[q & 1];
        if (!ev.ck(hipEventRecord(ev.ev[2 * q], s)) || !ev.ck(hipStreamWaitEvent(qs, ev.ev[2 * q], 0)) ||
            !ev.ck(st.reduce(w0, w1, q, qs)) || !ev.ck(horner(v0, v1, qs)))
            break;
        ev.ck(hipEventRecord(ev.ev[2 * q + 1], qs));
    }
    for (uint32_t q = 0; q + 1 < parts && ev.err == hipSuccess; q++) ev.ck(hipStreamWaitEvent(s, ev.ev[2 * q + 1], 0));
    return ev.finish(side);
}

// A single MSM: window parts, top windows first.  The caller's stream runs
// every part's bucket accumulation back to back; part q's reduction runs on a
// side stream behind it and its Horner leg (windows [w0, w1), continuing the
// part above) on a third, so the latency-bound tails (segment-sum levels,
// the 16 doublings per window of the Horner chain) of the upper parts
// hide under the next parts' accumulation.  Only the last part's reduction
// and Horner leg are exposed.  Same window sums, same Horner: same point.
template <int G>
static hipError_t msm_schedule_windows(const MsmStages<G>& st, uint64_t* out, hipStream_t s) {
    constexpr int JW = Grp<G>::JW;
    const MsmPlan& p = st.p;
    const uint32_t parts = msm_parts(p.W);
    auto horner = [&](uint32_t w0, uint32_t w1, const uint64_t* leg_in, uint64_t* leg_out, hipStream_t hs) {
        hipLaunchKernelGGL(k_msm_horner_q<G>, dim3(1), dim3(64), 0, hs, st.wsum, st.spw, (int)w1, (int)w0, p.c, leg_in,
                           leg_out);
        return hipGetLastError();
    };
    hipError_t e;
    if (parts == 1) {
        if ((e = st.accumulate(0, p.W, s)) != hipSuccess || (e = st.reduce(0, p.W, 0, s)) != hipSuccess) return e;
        return horner(0, p.W, nullptr, out, s);
    }
    hipStream_t side[2];
    if ((e = msm_side_streams(s, side)) != hipSuccess) return e;
    const hipStream_t red_s = side[0], hor_s = side[1];
    // ev[2q]: part q accumulated; ev[2q + 1]: part q reduced; ev[2 parts]: the upper Horner legs done
    MsmEvents ev(2 * (int)parts + 1);
    // part q covers windows [wlo(q), wlo(q - 1)); PA_MSM_WLO="b0,b1,..." (descending
    // lower bounds, A/B of unequal parts) overrides the even split
    static const std::vector<uint32_t> wlo_env = [] {
        std::vector<uint32_t> v;
        if (const char* e = getenv("PA_MSM_WLO"))
            for (const char* c = e; *c;) {
                v.push_back((uint32_t)strtoul(c, const_cast<char**>(&c), 10));
                if (*c == ',') c++;
                else break;
            }
        return v;
    }();
    // the override is taken whole or not at all: exactly parts - 1 bounds, strictly
    // descending, each in (0, W) -- otherwise windows would be summed twice or skipped
    bool use_env = wlo_env.size() + 1 == parts;
    for (size_t k = 0; use_env && k < wlo_env.size(); k++)
        use_env = wlo_env[k] > 0 && wlo_env[k] < p.W && (k == 0 || wlo_env[k] < wlo_env[k - 1]);
    auto wlo = [&](uint32_t q) {
        if (use_env && q + 1 < parts) return wlo_env[q];
        return q + 1 == parts ? 0u : (uint32_t)(((uint64_t)p.W * (parts - 1 - q)) / parts);
    };
    for (uint32_t q = 0; q < parts && ev.err == hipSuccess; q++) {
        const uint32_t w1 = q == 0 ? p.W : wlo(q - 1), w0 = wlo(q);
        if (!ev.ck(st.accumulate(w0, w1, s))) break;
        uint64_t* leg_out = q + 1 == parts ? out : st.w.hacc + (size_t)JW * q;
        const uint64_t* leg_in = q == 0 ? nullptr : st.w.hacc + (size_t)JW * (q - 1);
        if (q + 1 == parts) {
            if (ev.ck(st.reduce(w0, w1, q, s)) && ev.ck(hipStreamWaitEvent(s, ev.ev[2 * parts], 0)))
                ev.ck(horner(w0, w1, leg_in, leg_out, s));
            break;
        }
        if (!ev.ck(hipEventRecord(ev.ev[2 * q], s)) || !ev.ck(hipStreamWaitEvent(red_s, ev.ev[2 * q], 0)) ||
            !ev.ck(st.reduce(w0, w1, q, red_s)) || !ev.ck(hipEventRecord(ev.ev[2 * q + 1], red_s)) ||
            !ev.ck(hipStreamWaitEvent(hor_s, ev.ev[2 * q + 1], 0)) || !ev.ck(horner(w0, w1, leg_in, leg_out, hor_s)))
            break;
        if (q + 2 == parts) ev.ck(hipEventRecord(ev.ev[2 * parts], hor_s));
    }
    return ev.finish(side);
}

template <int G>
static hipError_t msm_run(const MsmJob& job, uint64_t* out, void* ws, size_t ws_bytes, hipStream_t s) {
    if (job.vectors == 0) return hipSuccess;
    if (job.terms == 0) {
        hipLaunchKernelGGL(k_jac_zero_out<G>, dim3(msm_blocks(job.vectors, 64)), dim3(64), 0, s, out, job.vectors);
        return hipGetLastError();
    }
    const size_t n = job.glv ? 2 * job.terms : job.terms;   // items per window
    MsmPlan p;
    const bool short_plan = job.glv || job.u128;   // 130-bit windows
    hipError_t e = msm_plan(p, G, n, short_plan, job.rows == nullptr, job.vectors);
    if (e != hipSuccess) return e;
    if (ws_bytes < p.total || !ws) return hipErrorInvalidValue;
    if (!p.fits || p.items > 0xffffffffull) return hipErrorInvalidValue;  // 32-bit item positions and keys
    if (p.WT * p.tpw > 0x7fffffffull) return hipErrorInvalidValue;        // the sort's grid
    MsmWs w = msm_ws(p, job, ws);
    if ((e = msm_sort_items(job, p, n, w, s)) != hipSuccess) return e;
    if ((e = msm_bounds_and_bases<G>(job, p, n, w, s)) != hipSuccess) return e;
    const MsmStages<G> st(p, w, n, short_plan);
    if (job.vectors > 1) return msm_schedule_batch<G>(st, job.vectors, out, s);
    return msm_schedule_windows<G>(st, out, s);
}

hipError_t launch_msm(int group, const uint64_t* bases, const uint64_t* scalars, size_t n, uint64_t* out, void* ws,
                      size_t ws_bytes, hipStream_t stream) {
    if (n >= 0x80000000ull) return hipErrorInvalidValue;
    const MsmJob job{bases, nullptr, scalars, n, 0, false};
    return group == 1 ? msm_run<1>(job, out, ws, ws_bytes, stream) : msm_run<2>(job, out, ws, ws_bytes, stream);
}

// The largest plan of any n' <= n, so that the size never decreases with n: a
// workspace sized for the largest batch serves every smaller one.  The plan
// of one n is not monotone in two places.  The window width changes at
// powers of two (fewer windows: fewer items), and inside one width the chunk
// T = msm_chunk(items) rises by one each time W n' passes a multiple of
// kMsmFillLanes * parts, which shortens the continuation array by 1 / T.
// Between those points every array grows with n', so the maximum is at n, at
// the last n' of a width, or at the last n' before a step of T.
size_t msm_u128_workspace_bytes(size_t n) {
    if (n == 0) return 0;
    size_t best = 0;
    auto probe = [&](size_t m, MsmPlan& p) {
        if (msm_plan(p, 1, m, true) == hipSuccess && p.total > best) best = p.total;
    };
    for (size_t lo = 1; lo <= n; lo <<= 1) {
        const size_t hi = n < 2 * lo - 1 ? n : 2 * lo - 1;   // the width's terms are [lo, hi]
        MsmPlan p{};
        probe(hi, p);
        if (!p.W) return 0;
        const size_t step = kMsmFillLanes * msm_parts(p.W);   // T = ceil(W n' / step), within 8 .. kMsmChunk
        for (size_t j = 8 > p.W * lo / step ? 8 : p.W * lo / step; j < kMsmChunk && j * step / p.W < hi; j++) {
            MsmPlan q;
            if (j * step / p.W >= lo) probe(j * step / p.W, q);
        }
    }
    return best;
}
hipError_t launch_msm_u128_g1(const uint64_t* bases, const uint64_t* scalars, size_t n, uint64_t* out, void* ws,
                              size_t ws_bytes, hipStream_t stream) {
    if (n >= 0x80000000ull) return hipErrorInvalidValue;
    MsmJob job{bases, nullptr, scalars, n, 0, false};
    job.u128 = true;
    return msm_run<1>(job, out, ws, ws_bytes, stream);
}

hipError_t launch_msm_prepare(int group, const uint64_t* bases, const uint8_t* ok, size_t n, uint32_t* rows,
                              uint32_t* bad, hipStream_t stream) {
    if (n >= kMsmPreparedMax) return hipErrorInvalidValue;
    hipError_t e = hipMemsetAsync(bad, 0, sizeof(uint32_t), stream);
    if (e != hipSuccess || n == 0) return e;
    const auto prepare = group == 1 ? MsmKernels<1>::bases_prepare : MsmKernels<2>::bases_prepare;
    hipLaunchKernelGGL(prepare, dim3(msm_blocks(n, 256)), dim3(256), 0, stream, bases, ok, n, rows, bad);
    return hipGetLastError();
}

// k vectors over the prepared rows of either group; k = 1 without mont is a single MSM's job
hipError_t launch_msm_prepared(int group, const uint32_t* rows, size_t len, bool glv, const uint64_t* scalars,
                               size_t m, size_t k, bool mont, uint64_t* out, void* ws, size_t ws_bytes,
                               hipStream_t stream) {
    if (len >= kMsmPreparedMax || m > len) return hipErrorInvalidValue;
    MsmJob job{nullptr, rows, scalars, m, len, glv};
    job.vectors = k;
    job.mont = mont;
    return group == 1 ? msm_run<1>(job, out, ws, ws_bytes, stream) : msm_run<2>(job, out, ws, ws_bytes, stream);
}

hipError_t launch_scalar_mul(int group, int projective, const uint64_t* p, const uint64_t* scalars, size_t n,
                             uint64_t* out, hipStream_t stream) {
    if (n == 0) return hipSuccess;
    const dim3 g(msm_blocks(n, 64)), b(64);
    if (group == 1) {
        if (projective) hipLaunchKernelGGL(k_proj_mul<1>, g, b, 0, stream, p, scalars, out, n);
        else hipLaunchKernelGGL(k_affine_mul<1>, g, b, 0, stream, p, scalars, out, n);
    } else {
        if (projective) hipLaunchKernelGGL(k_proj_mul<2>, g, b, 0, stream, p, scalars, out, n);
        else hipLaunchKernelGGL(k_affine_mul<2>, g, b, 0, stream, p, scalars, out, n);
    }
    return hipGetLastError();
}

}  // namespace pa
