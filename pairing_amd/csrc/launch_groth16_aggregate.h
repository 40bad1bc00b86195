// Host-side launchers of kernels_groth16_aggregate.hip: the steps of the
// randomised batch check of k Groth16 proofs (bellman's verify_proofs_batch)
// that the MSM, the Miller loops and the final exponentiation leave open.
// Device pointers, asynchronous on `stream`.
#pragma once
#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>

namespace pa {

// rows per block of the weight sums' first stage, and its block count for k proofs (at least 1, at most
// kGroth16WeightMaxBlocks: beyond that a block strides over the rows)
constexpr unsigned kGroth16WeightBlock = 256, kGroth16WeightMaxBlocks = 256;
unsigned groth16_weight_blocks(size_t k);

// s[0] = sum_j z_j, s[i + 1] = sum_j z_j x[j * stride + i] mod r for i < l, written as FrRepr rows (4 u64).
// z: k rows of two u64 (little-endian, any 128-bit value); inputs as launch_groth16_input_sum takes them, an
// FrRepr row taken mod r.  partials: groth16_weight_blocks(k) * (l + 1) rows of 4 u64 of scratch.  Stage one
// leaves one partial per block and column, stage two folds a column's partials in block order: no atomics, the
// same bits every run.  k = 0 writes zeros.
hipError_t launch_groth16_weight_sums(const uint64_t* z, const uint64_t* inputs, size_t stride, int montgomery,
                                      size_t l, size_t k, uint64_t* partials, uint64_t* s, hipStream_t stream);
// out[j] = z_j * a[j] (Jacobian records, 18 u64; a: affine records, 13 u64): one lane per point, at most 128 doublings
// and the at most 65 additions of z_j's non-adjacent form on the lazy core with the full group law (an addition of equal
// operands doubles, of opposite ones gives zero), so any on-curve point is multiplied as the reference's
// double-and-add multiplies it, as a point.  Infinity or z_j = 0 gives zero.
hipError_t launch_groth16_scale(const uint64_t* a, const uint64_t* z, size_t k, uint64_t* out, hipStream_t stream);
// out_acc = s[0] ic[0] + sum_{i < l} s[i + 1] ic[i + 1], out_alpha = s[0] alpha (Jacobian records).  tables: l + 2
// comb tables in the order ic[1..l], ic[0], alpha; s: l + 1 FrRepr rows; partials: l + 2 Jacobian records of
// scratch (one comb multiply per lane).  The sum: 64 lanes each add every 64th partial in sequence, then a tree
// of 6 levels over the lanes.
hipError_t launch_groth16_comb_sum(const uint64_t* tables, const uint64_t* s, size_t l, uint64_t* partials,
                                   uint64_t* out_acc, uint64_t* out_alpha, hipStream_t stream);
// proofs (k records of 51 u64) into three arrays: a[j] = A_j, c[j] = C_j (13 u64), q[j] = B_j (25 u64)
hipError_t launch_groth16_split3(const uint64_t* proofs, size_t k, uint64_t* a, uint64_t* q, uint64_t* c,
                                 hipStream_t stream);
// The end of the chain, one record: where *ok == 0 (the final exponentiation's None) gt is zeroed;
// *valid = *ok && gt == one && every status is 0.  status_abc: the decoders' statuses of A, B and C (k bytes each,
// end to end) or null; status_out (3 k bytes, proof-major) gets them interleaved by a kernel of one lane per
// byte, which leaves "any nonzero" in *bad (one byte of scratch; unused without statuses).  trivial != 0
// (k = 0): writes gt = one (gt may be null) and *valid = 1, reads nothing.
hipError_t launch_groth16_aggregate_finish(uint64_t* gt, const uint8_t* ok, const uint8_t* status_abc,
                                           uint8_t* status_out, uint8_t* bad, uint8_t* valid, size_t k, int trivial,
                                           hipStream_t stream);

}  // namespace pa
