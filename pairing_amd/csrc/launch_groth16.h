// Host-side launchers of kernels_r1cs.hip and kernels_groth16.hip: the two
// steps of a Groth16 prover that the NTT and multiexp entries leave open.
// Device pointers, asynchronous on `stream`.
#pragma once
#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>

#include <vector>

namespace pa {

// ---- R1CS matrices times k witnesses (kernels_r1cs.hip) ----
// A chunk is what one lane sums.  32: a 2^16-term row becomes 2048 chunks = 32
// waves' worth, and a slab of one-term rows that holds the tail chunk of a long
// row is padded to at most 32 terms per lane.
constexpr size_t kR1csChunkLen = 32;

struct R1csCsr {   // host CSR of one matrix, val as 4 u64 per term
    const uint64_t* row_ptr;
    const uint32_t* col;
    const uint64_t* val;
};
struct R1csSlabs {
    size_t first[4];   // first slab of A, B, C; [3] = slabs in all
};
struct R1csImage {   // host copy of the device image
    std::vector<uint64_t> val;          // 4 u64 per entry, term-major within a slab
    std::vector<uint32_t> col;
    std::vector<uint64_t> slab_off;     // first entry of the slab
    std::vector<uint32_t> slab_len;     // terms of its longest chunk
    std::vector<uint32_t> chunk_len;    // 64 per slab
    std::vector<uint32_t> chunk_dst;    // row, or bit 31 | partial-sum slot; 0xffffffff = no chunk
    std::vector<uint32_t> fold;         // per row of several chunks: first slot, slots, matrix, row
    R1csSlabs slabs{};
    size_t entries = 0, n_partial = 0, n_fold = 0;
};
struct R1csDevLayout {   // byte offsets of the arrays in the one device allocation
    size_t val, col, slab_off, slab_len, chunk_len, chunk_dst, fold, bytes;
};
struct R1csDev {
    const void* image;
    R1csDevLayout layout;
    R1csSlabs slabs;
    size_t n_rows, n_cols, n_partial, n_fold;
};
// the CSR must have been validated (row_ptr, columns) by the caller
void r1cs_build(const R1csCsr m[3], size_t n_rows, R1csImage& img);
R1csDevLayout r1cs_dev_layout(const R1csImage& img);
// a, b, c: k polynomials of 2^log_n rows; workspace: k * n_partial rows of 32 bytes
hipError_t launch_r1cs_eval(const R1csDev& r, const uint64_t* witness, size_t k, unsigned log_n, uint64_t* a,
                            uint64_t* b, uint64_t* c, void* workspace, hipStream_t stream);
// the same over outputs of n >= n_rows rows each, n any count (n = n_rows: nothing is padded)
hipError_t launch_r1cs_eval(const R1csDev& r, const uint64_t* witness, size_t k, size_t n, uint64_t* a, uint64_t* b,
                            uint64_t* c, void* workspace, hipStream_t stream);

// ---- proof assembly (kernels_groth16.hip) ----
// consts: alpha_g1, beta_g1, delta_g1 (13 u64 affine records each), then beta_g2, delta_g2 (25 u64 each).
// sums: the five multiexp results, k Jacobian records each: a_query, b_g1_query, l_query, h_query (G1, 18 u64) and
// b_g2_query (G2, 36 u64).  r, s: k Montgomery Fr rows.  proofs: k records of 51 u64 (A 13, B 25, C 13).
// After the five records (padded to 96 words) the key's fixed-base tables: 2^i delta_g1 and 2^i delta_g2 for
// i < 255 as Jacobian records (18 and 36 u64), built on the device by launch_groth16_tables from the records.
constexpr size_t kGroth16ConstWords = 3 * 13 + 2 * 25;
constexpr size_t kGroth16TableRows = 255;
constexpr size_t kGroth16Table1 = 96;
constexpr size_t kGroth16Table2 = kGroth16Table1 + kGroth16TableRows * 18;
constexpr size_t kGroth16KeyWords = kGroth16Table2 + kGroth16TableRows * 36;
constexpr size_t kGroth16ProofWords = 13 + 25 + 13;
hipError_t launch_groth16_tables(uint64_t* consts, hipStream_t stream);
hipError_t launch_groth16_assemble(const uint64_t* consts, const uint64_t* sum_a, const uint64_t* sum_b1,
                                   const uint64_t* sum_l, const uint64_t* sum_h, const uint64_t* sum_b2,
                                   const uint64_t* r, const uint64_t* s, size_t k, uint64_t* proofs,
                                   hipStream_t stream);

}  // namespace pa
