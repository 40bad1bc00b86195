// Host-side launchers of kernels_groth16_setup.hip: the steps of Groth16
// parameter generation (bellman's generate_parameters for a given trapdoor)
// that the NTT, the chunked sparse product and the fixed-base multiplies leave
// open.  Device pointers, asynchronous on `stream`.
#pragma once
#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>

#include <vector>

#include "launch_groth16.h"

namespace pa {

// What the kernels take of the trapdoor, by value (Montgomery rows of 4 u64, all below r).  The host
// forms them once per call: no lane inverts or raises anything to the n-th power.
struct Groth16SetupConsts {
    uint64_t tau_pow2[28][4];   // tau^(2^b), b < 28 = kNttMaxLogN
    uint64_t alpha[4], beta[4], gamma[4], delta[4];
    uint64_t gamma_inv[4], delta_inv[4];
    uint64_t h_scale[4];        // (tau^n - 1) / delta
};

// The transpose of one host CSR matrix (n_rows x n_cols) as a CSR of n_cols rows, by a counting sort
// that keeps the terms of a variable in row order; a column that occurs twice in a row stays two terms.
struct R1csCsrOwned {
    std::vector<uint64_t> row_ptr;
    std::vector<uint32_t> col;
    std::vector<uint64_t> val;
};
void r1cs_transpose(const R1csCsr& m, size_t n_rows, size_t n_cols, R1csCsrOwned& t);

// pow[i] = tau^i for i < 2^log_n: lane i multiplies the tau^(2^b) of its set bits
hipError_t launch_groth16_setup_powers(const Groth16SetupConsts& k, unsigned log_n, uint64_t* pow, hipStream_t stream);

// The scalar vectors of the key from u, v, w (n_vars Montgomery rows each) and the powers of tau (n rows):
//   g1[0 .. nv)           u_i                        g1[nv .. 2 nv)   v_i
//   g1[2 nv .. 3 nv)      (beta u_i + alpha v_i + w_i) / gamma for i < n_public, / delta from there on
//   g1[3 nv .. 3 nv + n - 1)   tau^i (tau^n - 1) / delta           then alpha, beta, delta
//   g2[0 .. nv)           v_i                        then beta, gamma, delta
// montgomery = false: canonical FrRepr rows (what the fixed-base multiplies read); true: Montgomery rows.
// g2 may be null (nothing of it is written).
hipError_t launch_groth16_setup_scalars(const Groth16SetupConsts& k, const uint64_t* u, const uint64_t* v,
                                        const uint64_t* w, const uint64_t* pow, size_t n_vars, size_t n_public,
                                        size_t n, bool montgomery, uint64_t* g1, uint64_t* g2, hipStream_t stream);

// Normalized Jacobian records (z = 1, or z = 0 for the identity: what batch_normalization leaves) to the
// affine records into_affine writes for them: (x, y, 0), and (0, 1, 1) for the identity.
hipError_t launch_groth16_setup_pack(int group, const uint64_t* jac, uint64_t* aff, size_t n, hipStream_t stream);

}  // namespace pa
