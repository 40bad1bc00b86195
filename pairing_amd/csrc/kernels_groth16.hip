// Proof assembly of a Groth16 prover (bellman's create_proof after its
// multiexps): from the five multiexp sums of proof j, the key's alpha, beta,
// delta and the blinding scalars r, s
//     A  = alpha_g1 + S_a  + r delta_g1
//     B  = beta_g2  + S_b2 + s delta_g2
//     B1 = beta_g1  + S_b1 + s delta_g1
//     C  = S_l + S_h + s A + r B1 - (r s) delta_g1
// as affine records.  With A0 = alpha_g1 + S_a and B0 = beta_g1 + S_b1,
//     s A + r B1 - r s delta_g1 = s A0 + r B0 + (r s) delta_g1,
// so a proof is five scalar multiplications that do not depend on one another:
// r delta_g1, (r s) delta_g1 and s delta_g2 over bases the key fixes, s A0 and
// r B0 over bases of the proof.  Affine coordinates are canonical, so the
// records equal into_affine of the reference's points bit for bit whatever the
// order of the group operations.
//
// For one proof the kernel is pure latency, so the work is spread over lanes.
// The key holds 2^i delta for i < 255 in both groups (k_groth16_table, once per
// key): a fixed-base product is the sum of the table rows at the scalar's set
// bits, no doubling, and the rows are shared out over a wave.  A block is one
// proof and three waves:
//   wave 0  s delta_g2: lane l adds the rows of bits 4 l .. 4 l + 3, then a tree
//           over LDS; lane 0 finishes B (nothing in G1 waits for it)
//   wave 1  r delta_g1 on lanes 0..31 and (r s) delta_g1 on lanes 32..63, bits
//           8 l .. 8 l + 7 each, a tree per half
//   wave 2  lane 0: s A0, lane 1: r B0, the two 255-step double-and-add chains
//           that bound the kernel; then lane 0 finishes A and lane 1 C
// (a one-lane double-and-add for s delta_g2 alone took 22 ms at k = 1:
// profiles/groth16_prove/v1_default.txt).
#include "curve.h"
#include "fr.h"
#include "launch_groth16.h"

namespace pa {
namespace {

PA_DEV void lds_put(uint32_t* o, const Fq& a) {
#pragma unroll
    for (int i = 0; i < 12; i++) o[i] = a.w[i];
}
PA_DEV void lds_get(Fq& a, const uint32_t* o) {
#pragma unroll
    for (int i = 0; i < 12; i++) a.w[i] = o[i];
}
PA_DEV void lds_put(uint32_t* o, const Fq2& a) { lds_put(o, a.c0); lds_put(o + 12, a.c1); }
PA_DEV void lds_get(Fq2& a, const uint32_t* o) { lds_get(a.c0, o); lds_get(a.c1, o + 12); }
template <class F>
PA_DEV void lds_put(uint32_t* o, const Jac<F>& p) {
    constexpr int W = 2 * FieldWords<F>::n;   // u32 words per coordinate
    lds_put(o, p.x);
    lds_put(o + W, p.y);
    lds_put(o + 2 * W, p.z);
}
template <class F>
PA_DEV void lds_get(Jac<F>& p, const uint32_t* o) {
    constexpr int W = 2 * FieldWords<F>::n;
    lds_get(p.x, o);
    lds_get(p.y, o + W);
    lds_get(p.z, o + 2 * W);
}

// out = scalar * base, scalar = 8 x u32 LE (an FrRepr below r: 255 bits), MSB first
template <class F>
PA_DEV void jac_mul_repr(Jac<F>& out, const Jac<F>& base, const uint32_t* scalar) {
    jac_zero(out);
    for (int wi = 7; wi >= 0; wi--) {
        const uint32_t e = scalar[wi];
        for (int bit = 31; bit >= 0; bit--) {
            jac_double(out);
            if ((e >> bit) & 1) jac_add(out, base);
        }
    }
}

// the sum of the table rows (Jacobian 2^i base) at the set bits first .. first + count - 1 of the scalar
template <class F>
PA_DEV void table_sum(Jac<F>& acc, const uint64_t* table, const uint32_t* scalar, int first, int count) {
    constexpr int JW = 3 * FieldWords<F>::n;
    jac_zero(acc);
    for (int b = first; b < first + count && b < (int)kGroth16TableRows; b++)
        if ((scalar[b >> 5] >> (b & 31)) & 1) {
            Jac<F> t;
            load_jac(t, table + (size_t)JW * b);
            jac_add(acc, t);
        }
}

// table[i] = 2^i base for i < kGroth16TableRows, Jacobian records; one lane
template <class F>
__global__ void __launch_bounds__(64) k_groth16_table(const uint64_t* __restrict__ base, uint64_t* __restrict__ table) {
    if (threadIdx.x != 0 || blockIdx.x != 0) return;
    constexpr int JW = 3 * FieldWords<F>::n;
    Aff<F> a;
    load_aff(a, base);
    Jac<F> p;
    jac_from_affine(p, a);
    for (size_t i = 0; i < kGroth16TableRows; i++) {
        store_jac(table + JW * i, p);
        jac_double(p);
    }
}

__global__ void __launch_bounds__(192) k_groth16_assemble(const uint64_t* __restrict__ consts,
                                                           const uint64_t* __restrict__ sum_a,
                                                           const uint64_t* __restrict__ sum_b1,
                                                           const uint64_t* __restrict__ sum_l,
                                                           const uint64_t* __restrict__ sum_h,
                                                           const uint64_t* __restrict__ sum_b2,
                                                           const uint64_t* __restrict__ r, const uint64_t* __restrict__ s,
                                                           uint64_t* __restrict__ proofs) {
    __shared__ uint32_t sh2[64 * 72];   // wave 0's partial sums in G2
    __shared__ uint32_t sh1[64 * 36];   // wave 1's in G1: [0] ends as r delta_g1, [32] as (r s) delta_g1
    __shared__ uint32_t shp[2 * 36];    // s A0 and r B0
    const unsigned wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const size_t j = blockIdx.x;
    const uint64_t *alpha1 = consts, *beta1 = consts + 13, *beta2 = consts + 39;
    const uint64_t *tab1 = consts + kGroth16Table1, *tab2 = consts + kGroth16Table2;
    Fr fr_r, fr_s, repr;
    fr_load(fr_r, r + 4 * j);
    fr_load(fr_s, s + 4 * j);
    Jac<Fq> acc1;    // waves 1 and 2
    Jac<Fq2> acc2;   // wave 0
    jac_zero(acc1);
    jac_zero(acc2);
    if (wave == 0) {
        fr_into_repr(repr, fr_s);
        table_sum(acc2, tab2, repr.w, 4 * (int)lane, 4);
        lds_put(sh2 + 72 * lane, acc2);
    } else if (wave == 1) {
        Fr e = fr_r;
        if (lane >= 32) fr_mul(e, fr_r, fr_s);
        fr_into_repr(repr, e);
        table_sum(acc1, tab1, repr.w, 8 * (int)(lane & 31), 8);
        lds_put(sh1 + 36 * lane, acc1);
    } else if (lane < 2) {
        // lane 0: s (alpha_g1 + S_a), lane 1: r (beta_g1 + S_b1); lane 0 keeps A0 for A
        fr_into_repr(repr, lane == 0 ? fr_s : fr_r);
        Aff<Fq> t;
        load_jac(acc1, (lane == 0 ? sum_a : sum_b1) + 18 * j);
        load_aff(t, lane == 0 ? alpha1 : beta1);
        jac_add_mixed(acc1, t);
        Jac<Fq> prod;
        jac_mul_repr(prod, acc1, repr.w);
        lds_put(shp + 36 * lane, prod);
    }
    __syncthreads();
    // the trees: wave 0 over 64 lanes, wave 1 over each half of 32
    for (unsigned half = 32; half > 0; half >>= 1) {
        if (wave == 0 && lane < half) {
            Jac<Fq2> t;
            lds_get(t, sh2 + 72 * (lane + half));
            jac_add(acc2, t);
            lds_put(sh2 + 72 * lane, acc2);
        } else if (wave == 1 && half < 32 && (lane & 31) < half) {
            Jac<Fq> t;
            lds_get(t, sh1 + 36 * (lane + half));
            jac_add(acc1, t);
            lds_put(sh1 + 36 * lane, acc1);
        }
        __syncthreads();
    }
    if (wave == 0 && lane == 0) {
        // B = s delta_g2 + S_b2 + beta_g2
        Jac<Fq2> t;
        Aff<Fq2> a, out;
        load_jac(t, sum_b2 + 36 * j);
        jac_add(acc2, t);
        load_aff(a, beta2);
        jac_add_mixed(acc2, a);
        jac_to_affine(out, acc2);
        store_aff(proofs + kGroth16ProofWords * j + 13, out);
    } else if (wave == 2 && lane < 2) {
        Jac<Fq> t;
        if (lane == 0) {
            // A = A0 + r delta_g1
            lds_get(t, sh1);
            jac_add(acc1, t);
        } else {
            // C = S_l + S_h + s A0 + r B0 + (r s) delta_g1
            load_jac(acc1, sum_l + 18 * j);
            load_jac(t, sum_h + 18 * j);
            jac_add(acc1, t);
            lds_get(t, shp);
            jac_add(acc1, t);
            lds_get(t, shp + 36);
            jac_add(acc1, t);
            lds_get(t, sh1 + 36 * 32);
            jac_add(acc1, t);
        }
        Aff<Fq> out;
        jac_to_affine(out, acc1);
        store_aff(proofs + kGroth16ProofWords * j + (lane == 0 ? 0 : 38), out);
    }
}

}  // namespace

hipError_t launch_groth16_tables(uint64_t* consts, hipStream_t stream) {
    hipLaunchKernelGGL(k_groth16_table<Fq>, dim3(1), dim3(64), 0, stream, consts + 26, consts + kGroth16Table1);
    hipLaunchKernelGGL(k_groth16_table<Fq2>, dim3(1), dim3(64), 0, stream, consts + 64, consts + kGroth16Table2);
    return hipGetLastError();
}

hipError_t launch_groth16_assemble(const uint64_t* consts, const uint64_t* sum_a, const uint64_t* sum_b1,
                                   const uint64_t* sum_l, const uint64_t* sum_h, const uint64_t* sum_b2,
                                   const uint64_t* r, const uint64_t* s, size_t k, uint64_t* proofs,
                                   hipStream_t stream) {
    if (k == 0) return hipSuccess;
    hipLaunchKernelGGL(k_groth16_assemble, dim3((unsigned)k), dim3(192), 0, stream, consts, sum_a, sum_b1, sum_l, sum_h,
                       sum_b2, r, s, proofs);
    return hipGetLastError();
}

}  // namespace pa
