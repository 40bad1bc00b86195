// The steps of a Groth16 verifier (bellman's verify_proof, k proofs per call)
// that the pairing, decoding and comb-table kernels leave open:
//     acc_j = ic[0] + sum_{i = 1..l} x_{j,i} ic[i]
//     gt_j  = final_exponentiation(ML(A_j, B_j) ML(acc_j, -gamma) ML(C_j, -delta))
//     valid_j = gt_j is Some && gt_j == e(alpha, beta)
//
// The public-input sum is k l scalar multiplications over only l bases, each
// with its own fixed-base comb table in the key (comb.h: signed 8-bit digits,
// at most 33 mixed additions on the lazy 28-bit core, no doubling):
//   k_g16v_partials   one lane per (proof, input): the comb multiply over table
//                     i, the body of k_g1_comb_mul; a Jacobian partial per lane,
//                     so a small k is not l x 33 additions in sequence on a lane
//   k_g16v_sum        one lane per proof: ic[0] and the l partials added with the
//                     full group law (add-2007-bl: equal operands double, opposite
//                     ones give zero), into_affine with the in-kernel inversion,
//                     the record written where the Miller loops read their P
// Affine coordinates are canonical, so the record is the reference's whatever
// the order of the additions.
//
// Around the Miller loops and the final exponentiation (capi.hip chains them):
//   k_g16v_split      proof records -> the P array (A | acc | C) and the Q array (B)
//   k_g16v_fill_q     -gamma and -delta repeated behind B (the path that runs all
//                     3 k pairs through the e(P, Q) Miller loops)
//   k_fq12_product3   the three Miller values of a proof multiplied: the segments
//                     have length 3, so no offsets are staged
//   k_g16v_compare    gt against the key's e(alpha, beta), the decoders' statuses
//                     folded in -> valid
//   k_g16v_gather     192-byte wire records -> three arrays for the decoders
#include "comb.h"
#include "fr.h"
#include "launch_groth16_verify.h"
#include "pairing_fl.h"

namespace pa {
namespace {

constexpr int kG1Aff = 13, kG2Aff = 25, kProofWords = kG1Aff + kG2Aff + kG1Aff, kF12 = 72;
constexpr size_t kCombTableWords = (size_t)kFlPair * kTableRows * kCombEntries;

// partial[j l + i] = x[j stride + i] * ic[i + 1], Jacobian; zero (ec.rs:224-230) when nothing was added
__global__ void __launch_bounds__(64) k_g16v_partials(const uint64_t* __restrict__ tables,
                                                      const uint64_t* __restrict__ inputs, size_t stride,
                                                      int montgomery, size_t l, size_t k,
                                                      uint64_t* __restrict__ partials) {
    const size_t t = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= k * l) return;
    const size_t j = t / l, i = t % l;
    const uint64_t* row = inputs + 4 * (j * stride + i);
    uint64_t s[4];
#pragma unroll
    for (int w = 0; w < 4; w++) s[w] = row[w];
    if (montgomery) {
        Fr a, r;
#pragma unroll
        for (int w = 0; w < 4; w++) {
            a.w[2 * w] = (uint32_t)s[w];
            a.w[2 * w + 1] = (uint32_t)(s[w] >> 32);
        }
        fr_into_repr(r, a);
#pragma unroll
        for (int w = 0; w < 4; w++) s[w] = (uint64_t)r.w[2 * w] | ((uint64_t)r.w[2 * w + 1] << 32);
    }
    const uint64_t* table = tables + kCombTableWords * i;
    FlJac acc;
    bool untouched;
    comb_mul_repr(acc, untouched, table, s);
    fl_store_jac_or_zero(partials + (size_t)kG1Jac * t, acc, untouched);
}

// out[j] = into_affine(ic0 + partial[j l] + ... + partial[j l + l - 1])
__global__ void __launch_bounds__(64) k_g16v_sum(const uint64_t* __restrict__ ic0,
                                                 const uint64_t* __restrict__ partials, size_t l, size_t k,
                                                 uint64_t* __restrict__ out) {
    const size_t j = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (j >= k) return;
    Aff<Fq> a;
    load_aff(a, ic0);
    Jac<Fq> acc;
    jac_from_affine(acc, a);
#pragma unroll 1
    for (size_t i = 0; i < l; i++) {
        Jac<Fq> t;
        load_jac(t, partials + (size_t)kG1Jac * (j * l + i));
        jac_add(acc, t);
    }
    jac_to_affine(a, acc);
    store_aff(out + (size_t)kG1Aff * j, a);
}

// one lane per word of a proof record; only the flag byte of a record's last word is defined
__global__ void __launch_bounds__(256) k_g16v_split(const uint64_t* __restrict__ proofs, size_t k,
                                                    uint64_t* __restrict__ p, uint64_t* __restrict__ q) {
    const size_t t = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= k * kProofWords) return;
    const size_t j = t / kProofWords;
    const int w = (int)(t % kProofWords);
    uint64_t v = proofs[t];
    if (w == kG1Aff - 1 || w == kG1Aff + kG2Aff - 1 || w == kProofWords - 1) v &= 0xff;
    if (w < kG1Aff)
        p[kG1Aff * j + w] = v;
    else if (w < kG1Aff + kG2Aff)
        q[kG2Aff * j + (w - kG1Aff)] = v;
    else
        p[kG1Aff * (2 * k + j) + (w - kG1Aff - kG2Aff)] = v;
}

__global__ void __launch_bounds__(256) k_g16v_fill_q(const uint64_t* __restrict__ neg_gamma,
                                                     const uint64_t* __restrict__ neg_delta, size_t k,
                                                     uint64_t* __restrict__ q) {
    const size_t t = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= 2 * k * kG2Aff) return;
    const int w = (int)(t % kG2Aff);
    q[(size_t)kG2Aff * k + t] = t < k * kG2Aff ? neg_gamma[w] : neg_delta[w];
}

__global__ void __launch_bounds__(64) k_fq12_product3(const uint64_t* __restrict__ ml, size_t k,
                                                      uint64_t* __restrict__ prod) {
    const size_t j = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (j >= k) return;
    F12<1> f = load12(ml + kF12 * j);
#pragma unroll 1   // one inlined product, as k_fq12_seg_product: two of them spill
    for (size_t t = 1; t < 3; t++) f = mul(f, load12(ml + kF12 * (t * k + j)));
    store12(prod + kF12 * j, f);
}

__global__ void __launch_bounds__(64) k_g16v_compare(uint64_t* __restrict__ gt, const uint8_t* __restrict__ ok,
                                                     const uint64_t* __restrict__ expected,
                                                     const uint8_t* __restrict__ status_abc,
                                                     uint8_t* __restrict__ status_out, uint8_t* __restrict__ valid,
                                                     size_t k) {
    const size_t j = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (j >= k) return;
    uint64_t* v = gt + kF12 * j;
    bool good = ok[j] != 0;
    if (good) {
        uint64_t diff = 0;
        for (int w = 0; w < kF12; w++) diff |= v[w] ^ expected[w];
        good = diff == 0;
    } else {
        for (int w = 0; w < kF12; w++) v[w] = 0;
    }
    if (status_abc) {
        for (int c = 0; c < 3; c++) {
            const uint8_t st = status_abc[(size_t)c * k + j];
            status_out[3 * j + c] = st;
            good = good && st == 0;
        }
    }
    valid[j] = good ? 1 : 0;
}

__global__ void __launch_bounds__(256) k_g16v_gather(const uint8_t* __restrict__ enc, size_t k,
                                                     uint8_t* __restrict__ enc_a, uint8_t* __restrict__ enc_b,
                                                     uint8_t* __restrict__ enc_c) {
    const size_t t = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= k * kGroth16EncodedProofBytes) return;
    const size_t j = t / kGroth16EncodedProofBytes;
    const int b = (int)(t % kGroth16EncodedProofBytes);
    const uint8_t v = enc[t];
    if (b < 48)
        enc_a[48 * j + b] = v;
    else if (b < 144)
        enc_b[96 * j + (b - 48)] = v;
    else
        enc_c[48 * j + (b - 144)] = v;
}

inline unsigned blocks_for(size_t n, unsigned bs) { return (unsigned)((n + bs - 1) / bs); }

}  // namespace

hipError_t launch_groth16_input_sum(const uint64_t* tables, const uint64_t* ic0, const uint64_t* inputs, size_t stride,
                                    int montgomery, size_t l, size_t k, uint64_t* partials, uint64_t* out,
                                    hipStream_t stream) {
    if (k == 0) return hipSuccess;
    if (l) {
        hipLaunchKernelGGL(k_g16v_partials, dim3(blocks_for(k * l, 64)), dim3(64), 0, stream, tables, inputs, stride,
                           montgomery, l, k, partials);
        const hipError_t e = hipGetLastError();
        if (e != hipSuccess) return e;
    }
    hipLaunchKernelGGL(k_g16v_sum, dim3(blocks_for(k, 64)), dim3(64), 0, stream, ic0, partials, l, k, out);
    return hipGetLastError();
}

hipError_t launch_groth16_split(const uint64_t* proofs, size_t k, uint64_t* p, uint64_t* q, hipStream_t stream) {
    if (k == 0) return hipSuccess;
    hipLaunchKernelGGL(k_g16v_split, dim3(blocks_for(k * kProofWords, 256)), dim3(256), 0, stream, proofs, k, p, q);
    return hipGetLastError();
}

hipError_t launch_groth16_fill_q(const uint64_t* neg_gamma, const uint64_t* neg_delta, size_t k, uint64_t* q,
                                 hipStream_t stream) {
    if (k == 0) return hipSuccess;
    hipLaunchKernelGGL(k_g16v_fill_q, dim3(blocks_for(2 * k * kG2Aff, 256)), dim3(256), 0, stream, neg_gamma,
                       neg_delta, k, q);
    return hipGetLastError();
}

hipError_t launch_fq12_product3(const uint64_t* ml, size_t k, uint64_t* prod, hipStream_t stream) {
    if (k == 0) return hipSuccess;
    hipLaunchKernelGGL(k_fq12_product3, dim3(blocks_for(k, 64)), dim3(64), 0, stream, ml, k, prod);
    return hipGetLastError();
}

hipError_t launch_groth16_compare(uint64_t* gt, const uint8_t* ok, const uint64_t* expected, const uint8_t* status_abc,
                                  uint8_t* status_out, uint8_t* valid, size_t k, hipStream_t stream) {
    if (k == 0) return hipSuccess;
    hipLaunchKernelGGL(k_g16v_compare, dim3(blocks_for(k, 64)), dim3(64), 0, stream, gt, ok, expected, status_abc,
                       status_out, valid, k);
    return hipGetLastError();
}

hipError_t launch_groth16_gather(const uint8_t* enc, size_t k, uint8_t* enc_a, uint8_t* enc_b, uint8_t* enc_c,
                                 hipStream_t stream) {
    if (k == 0) return hipSuccess;
    hipLaunchKernelGGL(k_g16v_gather, dim3(blocks_for(k * kGroth16EncodedProofBytes, 256)), dim3(256), 0, stream, enc,
                       k, enc_a, enc_b, enc_c);
    return hipGetLastError();
}

}  // namespace pa
