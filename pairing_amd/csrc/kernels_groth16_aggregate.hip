// The randomised batch check of k Groth16 proofs under one key (bellman's
// verify_proofs_batch), with 128-bit weights z_j:
//     s_0 = sum_j z_j,  s_{i+1} = sum_j z_j x_{j,i}  (mod r)
//     A'_j = z_j A_j,  accS = s_0 ic[0] + sum_i s_{i+1} ic[i+1],  CS = sum_j z_j C_j,  alphaS = s_0 alpha
//     gt = final_exponentiation(prod_j ML(A'_j, B_j) ML(accS, -gamma) ML(CS, -delta) ML(alphaS, -beta))
//     valid = gt is Some && gt == one
// k + 3 Miller loops and one final exponentiation instead of 3 k and k.  CS is
// the 130-bit MSM plan of kernels_msm.hip; the kernels here are the rest:
//   k_g16a_weight_partials / _fold   the k x (l + 1) column sums in Fr, two stages, no atomics
//   k_g16a_scale                     one lane per proof: z_j A_j over z_j's non-adjacent form
//   k_g16a_comb_partials / _sum      l + 2 comb multiplies over the key's tables, one lane
//                                    each, and their sum (strided chains, then a tree)
//   k_g16a_split                     proof records -> A, B and C arrays
//   k_g16a_status                    the decoders' 3 k statuses interleaved per proof, any nonzero flagged
//   k_g16a_finish                    the one gt against one, the statuses' flag folded in
// No scalar multiplication here uses the endomorphism: every step is the group
// law of E(Fq) with its equal / opposite / zero branches, so any on-curve point
// gives the point the reference's double-and-add gives.
#include "comb.h"
#include "fr.h"
#include "launch_groth16_aggregate.h"

namespace pa {
namespace {

constexpr int kG1Aff = 13, kG2Aff = 25, kProofWords = kG1Aff + kG2Aff + kG1Aff, kF12 = 72;
constexpr size_t kCombTableWords = (size_t)kFlPair * kTableRows * kCombEntries;
constexpr unsigned kSumLanes = 64;

PA_DEV void g16a_load_z(Fr& z, const uint64_t* __restrict__ rows, size_t j) {
    const uint4 v = reinterpret_cast<const uint4*>(rows)[j];
    z.w[0] = v.x; z.w[1] = v.y; z.w[2] = v.z; z.w[3] = v.w;
#pragma unroll
    for (int w = 4; w < 8; w++) z.w[w] = 0;
}

// partials[col nblk + blk] = sum over the block's rows j of z_j (col 0) or z_j x_{j, col-1}, canonical.
// z_j < 2^128 < r is its own canonical value; fr_mul(z, x R) = z x for a Montgomery row, and
// fr_mul(z R, x) = z x mod r for an FrRepr row of any value below 2^256.
__global__ void __launch_bounds__(kGroth16WeightBlock)
    k_g16a_weight_partials(const uint64_t* __restrict__ z, const uint64_t* __restrict__ inputs, size_t stride,
                           int montgomery, size_t k, uint64_t* __restrict__ partials) {
    __shared__ Fr sh[kGroth16WeightBlock];
    const unsigned tid = threadIdx.x, col = blockIdx.y;
    Fr acc;
    fr_zero(acc);
    for (size_t j = (size_t)blockIdx.x * kGroth16WeightBlock + tid; j < k;
         j += (size_t)gridDim.x * kGroth16WeightBlock) {
        Fr zj, term;
        g16a_load_z(zj, z, j);
        if (col == 0) {
            term = zj;
        } else {
            Fr x;
            fr_load(x, inputs + 4 * (j * stride + (col - 1)));
            if (!montgomery) {
                Fr r2;
                fr_r2(r2);
                fr_mul(zj, zj, r2);
            }
            fr_mul(term, zj, x);
        }
        fr_add(acc, acc, term);
    }
    sh[tid] = acc;
    __syncthreads();
    for (unsigned half = kGroth16WeightBlock / 2; half > 0; half >>= 1) {
        if (tid < half) {
            fr_add(acc, acc, sh[tid + half]);
            sh[tid] = acc;
        }
        __syncthreads();
    }
    if (tid == 0) fr_store(partials + 4 * ((size_t)col * gridDim.x + blockIdx.x), acc);
}

// s[col] = the column's partials added in block order
__global__ void __launch_bounds__(64) k_g16a_weight_fold(const uint64_t* __restrict__ partials, unsigned nblk,
                                                         size_t cols, uint64_t* __restrict__ s) {
    const size_t col = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (col >= cols) return;
    Fr acc;
    fr_zero(acc);
    for (unsigned b = 0; b < nblk; b++) {
        Fr t;
        fr_load(t, partials + 4 * (col * nblk + b));
        fr_add(acc, acc, t);
    }
    fr_store(s + 4 * col, acc);
}

// bit n of the value in three words (n < 192)
PA_DEV int g16a_bit(const uint64_t (&v)[3], int n) {
    const uint64_t w = n < 64 ? v[0] : (n < 128 ? v[1] : v[2]);   // selects: the words stay in registers
    return (int)((w >> (n & 63)) & 1);
}

// out[j] = z_j a[j].  Non-adjacent form, top digit first: with h = 3 z the digit of 2^i is
// bit_{i+1}(h) - bit_{i+1}(z), i = 128 .. 0 (h < 2^130), at most 65 of them nonzero.
__global__ void __launch_bounds__(64) k_g16a_scale(const uint64_t* __restrict__ a, const uint64_t* __restrict__ z,
                                                   size_t k, uint64_t* __restrict__ out) {
    const size_t j = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (j >= k) return;
    Aff<Fq> p;
    load_aff(p, a + (size_t)kG1Aff * j);
    const uint4 v = reinterpret_cast<const uint4*>(z)[j];
    const uint64_t zw[3] = {(uint64_t)v.x | ((uint64_t)v.y << 32), (uint64_t)v.z | ((uint64_t)v.w << 32), 0};
    uint64_t* o = out + (size_t)kG1Jac * j;
    if (p.inf || (zw[0] | zw[1]) == 0) {
        Jac<Fq> zero_pt;
        jac_zero(zero_pt);
        store_jac(o, zero_pt);
        return;
    }
    uint64_t h[3];   // 3 z = z + 2 z
    {
        const uint64_t d0 = zw[0] << 1, d1 = (zw[1] << 1) | (zw[0] >> 63), d2 = zw[1] >> 63;
        h[0] = zw[0] + d0;
        const uint64_t c0 = h[0] < d0 ? 1 : 0;
        const uint64_t t1 = zw[1] + d1;
        h[1] = t1 + c0;
        h[2] = d2 + (t1 < d1 ? 1 : 0) + (h[1] < t1 ? 1 : 0);
    }
    const F<1> px = fl_from_abi(p.x), py = fl_from_abi(p.y);
    FlJac acc = FlJac::zero();
    bool untouched = true;
#pragma unroll 1
    for (int i = 128; i >= 0; i--) {
        if (!untouched && !fl_is_zero(acc.z)) fl_jac_double(acc);
        const int d = g16a_bit(h, i + 1) - g16a_bit(zw, i + 1);
        if (d != 0) {
            const F<2> oy = d < 0 ? neg(py) : relax<2>(py);
            fl_jac_add_mixed(acc, untouched, px, oy);
        }
    }
    fl_store_jac(o, acc);   // z_j != 0: the top digit was added, and a sum that cancelled has z = 0
}

// partial[t] = s[t + 1] ic[t + 1] for t < l, s[0] ic[0] for t = l, s[0] alpha for t = l + 1
__global__ void __launch_bounds__(64) k_g16a_comb_partials(const uint64_t* __restrict__ tables,
                                                           const uint64_t* __restrict__ s, size_t l,
                                                           uint64_t* __restrict__ partials) {
    const size_t t = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= l + 2) return;
    const uint64_t* row = s + 4 * (t < l ? t + 1 : 0);
    uint64_t w[4];
#pragma unroll
    for (int i = 0; i < 4; i++) w[i] = row[i];
    FlJac acc;
    bool untouched;
    comb_mul_repr(acc, untouched, tables + kCombTableWords * t, w);
    fl_store_jac_or_zero(partials + (size_t)kG1Jac * t, acc, untouched);
}

// out_acc = partial[0] + .. + partial[l] (one block of kSumLanes lanes: lane i adds partials i, i + 64, .. in
// sequence, then six tree levels through LDS); out_alpha = partial[l + 1]
__global__ void __launch_bounds__(kSumLanes) k_g16a_comb_sum(const uint64_t* __restrict__ partials, size_t l,
                                                             uint64_t* __restrict__ out_acc,
                                                             uint64_t* __restrict__ out_alpha) {
    __shared__ FlJac sh[kSumLanes];
    const unsigned tid = threadIdx.x;
    if (tid < (unsigned)kG1Jac) out_alpha[tid] = partials[(size_t)kG1Jac * (l + 1) + tid];
    FlJac acc = FlJac::zero();
#pragma unroll 1
    for (size_t t = tid; t <= l; t += kSumLanes) fl_jac_add(acc, fl_load_jac(partials + (size_t)kG1Jac * t));
    sh[tid] = acc;
    __syncthreads();
#pragma unroll 1
    for (unsigned half = kSumLanes / 2; half > 0; half >>= 1) {
        if (tid < half) {
            fl_jac_add(acc, sh[tid + half]);
            sh[tid] = acc;
        }
        __syncthreads();
    }
    if (tid == 0) fl_store_jac_or_zero(out_acc, acc, fl_is_zero(acc.z));
}

// one lane per word of a proof record; only the flag byte of a record's last word is defined
__global__ void __launch_bounds__(256) k_g16a_split(const uint64_t* __restrict__ proofs, size_t k,
                                                    uint64_t* __restrict__ a, uint64_t* __restrict__ q,
                                                    uint64_t* __restrict__ c) {
    const size_t t = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= k * kProofWords) return;
    const size_t j = t / kProofWords;
    const int w = (int)(t % kProofWords);
    uint64_t v = proofs[t];
    if (w == kG1Aff - 1 || w == kG1Aff + kG2Aff - 1 || w == kProofWords - 1) v &= 0xff;
    if (w < kG1Aff)
        a[kG1Aff * j + w] = v;
    else if (w < kG1Aff + kG2Aff)
        q[kG2Aff * j + (w - kG1Aff)] = v;
    else
        c[kG1Aff * j + (w - kG1Aff - kG2Aff)] = v;
}

// The decoders' statuses (A, B and C: k bytes each, end to end) interleaved per proof, one lane per byte over
// the whole grid; *bad (zeroed before the launch) becomes 1 if any is nonzero.  Every lane that stores to *bad
// stores the same 1, so no atomic is needed.
__global__ void __launch_bounds__(256) k_g16a_status(const uint8_t* __restrict__ status_abc, size_t k,
                                                     uint8_t* __restrict__ status_out, uint8_t* __restrict__ bad) {
    const size_t t = (size_t)blockIdx.x * blockDim.x + threadIdx.x;   // t = c k + j
    uint8_t st = 0;
    if (t < 3 * k) {
        st = status_abc[t];
        status_out[3 * (t % k) + t / k] = st;
    }
    if (__syncthreads_or(st != 0) && threadIdx.x == 0) *bad = 1;
}

// word w of Fq12 one in the ABI's words: Fq one (R mod q, fq_one) and 66 zero words
PA_DEV uint64_t g16a_one_word(unsigned w) {
    Fq one;
    fq_one(one);
    uint64_t v = 0;
#pragma unroll
    for (unsigned i = 0; i < 6; i++)
        if (w == i) v = (uint64_t)one.w[2 * i] | ((uint64_t)one.w[2 * i + 1] << 32);
    return v;
}

// one block of at least 72 lanes; bad: k_g16a_status' byte or null
__global__ void __launch_bounds__(128) k_g16a_finish(uint64_t* __restrict__ gt, const uint8_t* __restrict__ ok,
                                                     const uint8_t* __restrict__ bad, uint8_t* __restrict__ valid,
                                                     int trivial) {
    const unsigned tid = threadIdx.x;
    if (trivial) {
        if (gt && tid < (unsigned)kF12) gt[tid] = g16a_one_word(tid);
        if (tid == 0) *valid = 1;
        return;
    }
    const bool some = *ok != 0;
    int differs = 0;
    if (tid < (unsigned)kF12) {
        if (some)
            differs = gt[tid] != g16a_one_word(tid);
        else
            gt[tid] = 0;
    }
    differs = __syncthreads_or(differs);
    if (tid == 0) *valid = some && !differs && !(bad && *bad) ? 1 : 0;
}

inline unsigned blocks_for(size_t n, unsigned bs) { return (unsigned)((n + bs - 1) / bs); }

}  // namespace

unsigned groth16_weight_blocks(size_t k) {
    const size_t b = (k + kGroth16WeightBlock - 1) / kGroth16WeightBlock;
    return (unsigned)(b < 1 ? 1 : (b > kGroth16WeightMaxBlocks ? kGroth16WeightMaxBlocks : b));
}

hipError_t launch_groth16_weight_sums(const uint64_t* z, const uint64_t* inputs, size_t stride, int montgomery,
                                      size_t l, size_t k, uint64_t* partials, uint64_t* s, hipStream_t stream) {
    const unsigned nblk = groth16_weight_blocks(k);
    hipLaunchKernelGGL(k_g16a_weight_partials, dim3(nblk, (unsigned)(l + 1)), dim3(kGroth16WeightBlock), 0, stream, z,
                       inputs, stride, montgomery, k, partials);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(k_g16a_weight_fold, dim3(blocks_for(l + 1, 64)), dim3(64), 0, stream, partials, nblk, l + 1, s);
    return hipGetLastError();
}

hipError_t launch_groth16_scale(const uint64_t* a, const uint64_t* z, size_t k, uint64_t* out, hipStream_t stream) {
    if (k == 0) return hipSuccess;
    hipLaunchKernelGGL(k_g16a_scale, dim3(blocks_for(k, 64)), dim3(64), 0, stream, a, z, k, out);
    return hipGetLastError();
}

hipError_t launch_groth16_comb_sum(const uint64_t* tables, const uint64_t* s, size_t l, uint64_t* partials,
                                   uint64_t* out_acc, uint64_t* out_alpha, hipStream_t stream) {
    hipLaunchKernelGGL(k_g16a_comb_partials, dim3(blocks_for(l + 2, 64)), dim3(64), 0, stream, tables, s, l, partials);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(k_g16a_comb_sum, dim3(1), dim3(kSumLanes), 0, stream, partials, l, out_acc, out_alpha);
    return hipGetLastError();
}

hipError_t launch_groth16_split3(const uint64_t* proofs, size_t k, uint64_t* a, uint64_t* q, uint64_t* c,
                                 hipStream_t stream) {
    if (k == 0) return hipSuccess;
    hipLaunchKernelGGL(k_g16a_split, dim3(blocks_for(k * kProofWords, 256)), dim3(256), 0, stream, proofs, k, a, q, c);
    return hipGetLastError();
}

hipError_t launch_groth16_aggregate_finish(uint64_t* gt, const uint8_t* ok, const uint8_t* status_abc,
                                           uint8_t* status_out, uint8_t* bad, uint8_t* valid, size_t k, int trivial,
                                           hipStream_t stream) {
    const bool statuses = !trivial && status_abc && k;
    if (statuses) {
        hipError_t e = hipMemsetAsync(bad, 0, 1, stream);
        if (e != hipSuccess) return e;
        hipLaunchKernelGGL(k_g16a_status, dim3(blocks_for(3 * k, 256)), dim3(256), 0, stream, status_abc, k, status_out,
                           bad);
        if ((e = hipGetLastError()) != hipSuccess) return e;
    }
    hipLaunchKernelGGL(k_g16a_finish, dim3(1), dim3(128), 0, stream, gt, ok, statuses ? bad : nullptr, valid, trivial);
    return hipGetLastError();
}

}  // namespace pa
