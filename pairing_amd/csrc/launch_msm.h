// Host-side launchers of kernels_msm.hip (variable-base scalar multiplication
// and MSM, SURVEY.md §8 f rank 3).  Device pointers, asynchronous on `stream`.
#pragma once
#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>

namespace pa {

// out[i] = scalars[i] * p[i] (group 1: G1, 2: G2), Jacobian, bit-exact with
// CurveAffine::mul (projective = 0, p = affine records, ec.rs:174-177, 88-95)
// or CurveProjective::mul_assign (projective = 1, p = Jacobian, ec.rs:534-553).
hipError_t launch_scalar_mul(int group, int projective, const uint64_t* p, const uint64_t* scalars, size_t n,
                             uint64_t* out, hipStream_t stream);
// out[0] = sum_i scalars[i] * bases[i] (Jacobian; equal as a point to the
// reference's sum).  `ws` must hold msm_workspace_bytes(group, n) bytes.
size_t msm_workspace_bytes(int group, size_t n);
hipError_t launch_msm(int group, const uint64_t* bases, const uint64_t* scalars, size_t n, uint64_t* out, void* ws,
                      size_t ws_bytes, hipStream_t stream);
// G1 only: out[0] = sum_i scalars[i] * bases[i] for 128-bit scalars in 16-byte
// rows (two u64, little-endian): ceil(130 / c) windows over the n real terms
// with the GLV plan's window rule, the bases converted per call.  No
// endomorphism and no membership assumption: the same point as launch_msm
// over the zero-extended scalars for any on-curve bases.  The workspace size
// is the largest plan of any n' <= n: it never decreases with n.
size_t msm_u128_workspace_bytes(size_t n);
hipError_t launch_msm_u128_g1(const uint64_t* bases, const uint64_t* scalars, size_t n, uint64_t* out, void* ws,
                              size_t ws_bytes, hipStream_t stream);

// ---- MSM over prepared bases ----
// Prepared rows, G1: 2n records of 28 u32 (the lazy 14 x 28-bit x, y the bucket
// accumulation gathers; infinity in bit 31 of x's top limb), row i = P_i, row
// n + i = -phi(P_i) = (beta x_i, -y_i).  G2: 2n records of 56 u32 (x.c0, x.c1,
// y.c0, y.c1; infinity in bit 31 of x.c0's top limb), row i = Q_i, row n + i =
// x^2 Q_i = (beta^2 x_i, -y_i).  n < kMsmPreparedMax: a row index and a sign
// share 32 bits.  `group` (1: G1, 2: G2) sizes the rows and the workspaces.
constexpr size_t kMsmPreparedMax = (size_t)1 << 30;
size_t msm_prepared_rows_bytes(size_t n, int group = 1);
// rows from the affine records; *bad = number of i with ok[i] == 0 (the
// membership flags of launch_subgroup_check over the same records)
hipError_t launch_msm_prepare(int group, const uint64_t* bases, const uint8_t* ok, size_t n, uint32_t* rows,
                              uint32_t* bad, hipStream_t stream);
// out[0] = sum_{i < m} scalars[i] * P_i over the rows of `len` prepared bases.
// (launch_msm_prepared with k = 1, mont = false.)
// glv (every base in the subgroup): s = q x^2 + rem, the two halves over rows i
// and len + i in ceil(130 / c) windows; otherwise the 257-bit pipeline over rows
// [0, m).  `ws` holds msm_prepared_workspace_bytes(m, glv, group) bytes.
size_t msm_prepared_workspace_bytes(size_t m, bool glv, int group = 1);

// out[j] = sum_{i < m} scalars[j m + i] * P_i for j < k: k vectors end to end
// through one pipeline of k W windows.  mont: the rows are Montgomery Fr below
// r (what the NTT writes) and pass through into_repr first.  Item positions
// and keys are 32-bit: msm_prepared_batch_fits says whether k W nt <= 2^32 - 1
// and k W B < 2^32 hold for the plan of (m, k); a batch that does not fit has
// workspace size 0 and is refused.
bool msm_prepared_batch_fits(size_t m, size_t k, bool glv, int group = 1);
size_t msm_prepared_batch_workspace_bytes(size_t m, size_t k, bool glv, int group = 1);
hipError_t launch_msm_prepared(int group, const uint32_t* rows, size_t len, bool glv, const uint64_t* scalars,
                               size_t m, size_t k, bool mont, uint64_t* out, void* ws, size_t ws_bytes,
                               hipStream_t stream);

}  // namespace pa
