// Host-side launchers of kernels_groth16_verify.hip: the steps of a Groth16
// verifier that the pairing, decoding and comb-table entries leave open.
// Device pointers, asynchronous on `stream`.
#pragma once
#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>

namespace pa {

constexpr size_t kGroth16EncodedProofBytes = 48 + 96 + 48;   // A, B, C compressed, bellman's Proof::write order

// The public-input sum of k proofs over the key's l = n_public - 1 bases:
//   out[j] = ic0 + sum_{i < l} x[j * stride + i] * ic[i + 1]      (affine records, 13 u64, canonical)
// tables: l fixed-base comb tables of g1_comb_table_words() u64 each (launch_g1_comb_table over ic[1..l]);
// ic0: one affine record; inputs: rows of 4 u64, FrRepr or (montgomery != 0) Montgomery Fr, row i of proof j at
// (j * stride + i) * 4; partials: k * l Jacobian records (18 u64) of scratch.  l = 0 writes ic0 k times and reads
// neither inputs nor partials.
hipError_t launch_groth16_input_sum(const uint64_t* tables, const uint64_t* ic0, const uint64_t* inputs, size_t stride,
                                    int montgomery, size_t l, size_t k, uint64_t* partials, uint64_t* out,
                                    hipStream_t stream);
// proofs (k records of 51 u64: A 13, B 25, C 13) into the arrays the Miller loops read: p[j] = A_j,
// p[2 k + j] = C_j (13 u64 each; p[k + j] is the input sum's), q[j] = B_j (25 u64)
hipError_t launch_groth16_split(const uint64_t* proofs, size_t k, uint64_t* p, uint64_t* q, hipStream_t stream);
// q[k + j] = *neg_gamma and q[2 k + j] = *neg_delta for j < k (25 u64 affine records): the Q array of the path
// that runs all 3 k pairs through the e(P, Q) Miller loops
hipError_t launch_groth16_fill_q(const uint64_t* neg_gamma, const uint64_t* neg_delta, size_t k, uint64_t* q,
                                 hipStream_t stream);
// prod[j] = ml[j] * ml[k + j] * ml[2 k + j] (Fq12, 72 u64 each): the segmented product at fixed length 3
hipError_t launch_fq12_product3(const uint64_t* ml, size_t k, uint64_t* prod, hipStream_t stream);
// valid[j] = ok[j] && gt[j] == *expected && (no status given || the three statuses of proof j are 0); where
// ok[j] == 0 (the final exponentiation's None) gt[j] is written as zero.  status_abc: the decoders' status arrays
// of A, B and C (k bytes each, end to end) or null; status_out (3 k bytes, proof-major) gets them interleaved.
hipError_t launch_groth16_compare(uint64_t* gt, const uint8_t* ok, const uint64_t* expected, const uint8_t* status_abc,
                                  uint8_t* status_out, uint8_t* valid, size_t k, hipStream_t stream);
// k encoded proofs (192 bytes: A 48, B 96, C 48) into three contiguous arrays for the decoders
hipError_t launch_groth16_gather(const uint8_t* enc, size_t k, uint8_t* enc_a, uint8_t* enc_b, uint8_t* enc_c,
                                 hipStream_t stream);

}  // namespace pa
