// Groth16 parameter generation (pa_groth16_generate*, include/pairing_amd.h):
// the three small steps between the existing heavy ones.
//
//   k_setup_powers    tau^i for i < n, one lane per i: the product of the
//                     tau^(2^b) of the set bits of i (at most log_n <= 28
//                     multiplications, no serial chain).  The inverse NTT of
//                     this vector is L_j(tau) = n^-1 sum_i tau^i w^(-ij), with
//                     no inversion and right for every tau, tau in the domain
//                     and tau = 0 included (bellman's generate_parameters).
//   k_setup_scalars   from u = A^T L, v = B^T L, w = C^T L (k_r1cs_chunks over
//                     the transposed image) the discrete logarithms of every
//                     G1 and G2 point of the key, one lane per G1 row.
//   k_setup_pack      batch_normalization's output as affine records.
//
// The trapdoor arrives by value (Groth16SetupConsts): 1/gamma, 1/delta and
// (tau^n - 1)/delta are formed once on the host.
#include "curve.h"
#include "fr.h"
#include "launch_groth16_setup.h"

namespace pa {
namespace {

inline unsigned blocks_for(size_t n, unsigned bs) { return (unsigned)((n + bs - 1) / bs); }

PA_DEV void fr_from_u64(Fr& r, const uint64_t* p) {
#pragma unroll
    for (int i = 0; i < 4; i++) {
        r.w[2 * i] = (uint32_t)p[i];
        r.w[2 * i + 1] = (uint32_t)(p[i] >> 32);
    }
}

__global__ void __launch_bounds__(256) k_setup_powers(Groth16SetupConsts k, unsigned log_n, uint64_t* __restrict__ pow) {
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (i >> log_n) return;
    Fr acc;
    fr_one(acc);
    for (unsigned b = 0; b < log_n; b++) {   // b is uniform: the table row is one load for the wave
        if ((i >> b) & 1) {
            Fr p;
            fr_from_u64(p, k.tau_pow2[b]);
            fr_mul(acc, acc, p);
        }
    }
    fr_store(pow + 4 * i, acc);
}

__global__ void __launch_bounds__(256) k_setup_scalars(Groth16SetupConsts k, const uint64_t* __restrict__ u,
                                                       const uint64_t* __restrict__ v, const uint64_t* __restrict__ w,
                                                       const uint64_t* __restrict__ pow, size_t nv, size_t n_public,
                                                       size_t n, int montgomery, uint64_t* __restrict__ g1,
                                                       uint64_t* __restrict__ g2) {
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    const size_t h0 = 3 * nv, c0 = h0 + n - 1;
    if (i >= c0 + 3) return;
    Fr x;
    if (i < nv) {
        fr_load(x, u + 4 * i);
    } else if (i < 2 * nv) {
        fr_load(x, v + 4 * (i - nv));
        if (g2) {
            Fr y;
            fr_into_repr(y, x);
            fr_store(g2 + 4 * (i - nv), y);
        }
    } else if (i < h0) {
        const size_t j = i - 2 * nv;
        Fr a, b, t;
        fr_load(a, u + 4 * j);
        fr_from_u64(t, k.beta);
        fr_mul(a, a, t);
        fr_load(b, v + 4 * j);
        fr_from_u64(t, k.alpha);
        fr_mul(b, b, t);
        fr_add(a, a, b);
        fr_load(b, w + 4 * j);
        fr_add(a, a, b);
        fr_from_u64(t, j < n_public ? k.gamma_inv : k.delta_inv);
        fr_mul(x, a, t);
    } else if (i < c0) {
        Fr t;
        fr_load(x, pow + 4 * (i - h0));
        fr_from_u64(t, k.h_scale);
        fr_mul(x, x, t);
    } else {
        const size_t c = i - c0;   // alpha, beta, delta in G1; beta, gamma, delta in G2
        fr_from_u64(x, c == 0 ? k.alpha : (c == 1 ? k.beta : k.delta));
        if (g2) {
            Fr y;
            fr_from_u64(y, c == 0 ? k.beta : (c == 1 ? k.gamma : k.delta));
            fr_into_repr(y, y);
            fr_store(g2 + 4 * (nv + c), y);
        }
    }
    if (!montgomery) fr_into_repr(x, x);
    fr_store(g1 + 4 * i, x);
}

template <int G>
__global__ void __launch_bounds__(64) k_setup_pack(const uint64_t* __restrict__ jac, uint64_t* __restrict__ aff,
                                                   size_t n) {
    using F = typename Grp<G>::F;
    const size_t i = (size_t)blockIdx.x * 64 + threadIdx.x;
    if (i >= n) return;
    Jac<F> p;
    load_jac(p, jac + (size_t)Grp<G>::JW * i);
    Aff<F> a;
    a.inf = jac_is_zero(p);
    if (a.inf) {   // into_affine of the identity, ec.rs:586-590
        zero(a.x);
        one(a.y);
    } else {
        a.x = p.x;
        a.y = p.y;
    }
    store_aff(aff + (size_t)Grp<G>::AW * i, a);
}

}  // namespace

void r1cs_transpose(const R1csCsr& m, size_t n_rows, size_t n_cols, R1csCsrOwned& t) {
    const uint64_t nnz = m.row_ptr[n_rows];
    t.row_ptr.assign(n_cols + 1, 0);
    t.col.assign(nnz, 0);
    t.val.assign(4 * nnz, 0);
    for (uint64_t e = 0; e < nnz; e++) t.row_ptr[m.col[e] + 1]++;
    for (size_t i = 0; i < n_cols; i++) t.row_ptr[i + 1] += t.row_ptr[i];
    std::vector<uint64_t> at(t.row_ptr.begin(), t.row_ptr.end() - 1);
    for (size_t r = 0; r < n_rows; r++)
        for (uint64_t e = m.row_ptr[r]; e < m.row_ptr[r + 1]; e++) {
            const uint64_t d = at[m.col[e]]++;
            t.col[d] = (uint32_t)r;
            for (int q = 0; q < 4; q++) t.val[4 * d + q] = m.val[4 * e + q];
        }
}

hipError_t launch_groth16_setup_powers(const Groth16SetupConsts& k, unsigned log_n, uint64_t* pow, hipStream_t stream) {
    const size_t n = (size_t)1 << log_n;
    hipLaunchKernelGGL(k_setup_powers, dim3(blocks_for(n, 256)), dim3(256), 0, stream, k, log_n, pow);
    return hipGetLastError();
}

hipError_t launch_groth16_setup_scalars(const Groth16SetupConsts& k, const uint64_t* u, const uint64_t* v,
                                        const uint64_t* w, const uint64_t* pow, size_t n_vars, size_t n_public,
                                        size_t n, bool montgomery, uint64_t* g1, uint64_t* g2, hipStream_t stream) {
    const size_t rows = 3 * n_vars + n + 2;
    hipLaunchKernelGGL(k_setup_scalars, dim3(blocks_for(rows, 256)), dim3(256), 0, stream, k, u, v, w, pow, n_vars,
                       n_public, n, montgomery ? 1 : 0, g1, g2);
    return hipGetLastError();
}

hipError_t launch_groth16_setup_pack(int group, const uint64_t* jac, uint64_t* aff, size_t n, hipStream_t stream) {
    if (n == 0) return hipSuccess;
    if (group == 1)
        hipLaunchKernelGGL(k_setup_pack<1>, dim3(blocks_for(n, 64)), dim3(64), 0, stream, jac, aff, n);
    else
        hipLaunchKernelGGL(k_setup_pack<2>, dim3(blocks_for(n, 64)), dim3(64), 0, stream, jac, aff, n);
    return hipGetLastError();
}

}  // namespace pa
