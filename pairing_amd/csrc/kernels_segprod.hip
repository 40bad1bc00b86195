// Segmented Fq12 products for the batched multi-pairing
// (pa_multi_pairing_batch[_device]): m independent products over one array of
// per-pair Miller values, the segments given as CSR offsets, one lane per
// Fq12 product on the lazy 28-bit core (pairing_fl.h).
//
//   k_fq12_seg_level     one halving level inside every segment still longer
//                        than `cap`: work[lo + i] *= work[lo + i + ceil(L/2)]
//   k_fq12_seg_product   prod[j] = the (at most cap) values left in segment j,
//                        multiplied in sequence; one for an empty segment
//   k_fq12_is_one        is_one[j] = ok[j] && out[j] == one  (the verdict byte)
//
// Fq12 multiplication is exact and commutative and the final exponentiation
// behind these kernels gives canonical words, so the order inside a segment is
// free.
#include "launch.h"
#include "pairing_fl.h"

namespace pa {

// Fq12 one in the ABI's Montgomery words: c0.c0.c0 = R mod q, the other 66 zero
__device__ constexpr uint64_t kMontOne[6] = {0x760900000002fffdULL, 0xebf4000bc40c0002ULL, 0x5f48985753c758baULL,
                                             0x77ce585370525745ULL, 0x5c071a97a256ec6dULL, 0x15f65ec3fa80e493ULL};

// values left in a segment of `len` after `levels` halving levels (a segment
// stops halving once it is at or below cap; cap >= 1)
__host__ __device__ inline size_t seg_len_after(size_t len, int levels, size_t cap) {
    for (int t = 0; t < levels && len > cap; t++) len = (len + 1) / 2;
    return len;
}

// Level `level` (0-based) over all n values: thread g finds its segment j
// (offsets[j] <= g < offsets[j + 1], binary search: empty segments repeat an
// offset and are never found) and its index i in it.  Reads touch i + half >=
// half and writes i < L / 2 <= half, so a level needs no second buffer.
__global__ void __launch_bounds__(64) k_fq12_seg_level(uint64_t* __restrict__ work,
                                                       const uint64_t* __restrict__ offsets, size_t m, size_t n,
                                                       int level, size_t cap) {
    const size_t g = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (g >= n) return;
    size_t lo = 0, hi = m;   // offsets[lo] <= g < offsets[hi]
    while (hi - lo > 1) {
        const size_t mid = lo + (hi - lo) / 2;
        if (offsets[mid] <= g) lo = mid; else hi = mid;
    }
    const size_t base = offsets[lo];
    const size_t len = seg_len_after(offsets[lo + 1] - base, level, cap);
    const size_t i = g - base, half = (len + 1) / 2;
    if (len <= cap || i >= len / 2) return;
    uint64_t* dst = work + 72 * g;
    store12(dst, mul(load12(dst), load12(dst + 72 * half)));
}

// the values the levels left at the front of segment j, multiplied in sequence
__global__ void __launch_bounds__(64) k_fq12_seg_product(const uint64_t* __restrict__ work,
                                                         const uint64_t* __restrict__ offsets,
                                                         uint64_t* __restrict__ prod, size_t m, int levels,
                                                         size_t cap) {
    const size_t j = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (j >= m) return;
    const size_t base = offsets[j];
    const size_t len = seg_len_after(offsets[j + 1] - base, levels, cap);
    uint64_t* dst = prod + 72 * j;
    if (len == 0) {   // the empty product
        for (int w = 0; w < 72; w++) dst[w] = w < 6 ? kMontOne[w] : 0;
        return;
    }
    const uint64_t* src = work + 72 * base;
    F12<1> f = load12(src);
#pragma unroll 1
    for (size_t i = 1; i < len; i++) f = mul(f, load12(src + 72 * i));
    store12(dst, f);
}

__global__ void __launch_bounds__(64) k_fq12_is_one(const uint64_t* __restrict__ out, const uint8_t* __restrict__ ok,
                                                    uint8_t* __restrict__ is_one, size_t m) {
    const size_t j = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (j >= m) return;
    const uint64_t* v = out + 72 * j;
    uint64_t diff = 0;
    for (int w = 0; w < 72; w++) diff |= v[w] ^ (w < 6 ? kMontOne[w] : 0);
    is_one[j] = ok[j] != 0 && diff == 0;
}

static inline unsigned blocks_for(size_t n, unsigned bs) { return (unsigned)((n + bs - 1) / bs); }

// Segments of at most this many values go to the sequential kernel as they
// are; longer ones are halved first.  4: the k = 2..4 of signature and Groth16
// checks never pays a level (a chain of at most 3 dependent products, ~0.1 ms
// each in one lane), and longer segments trade chain length for levels, each
// one launch as wide as the segments allow.  Measured at 8 / 4 / 2
// (profiles/multi_pairing_batch/): with many products the total number of
// multiplications decides and the threshold does not show; with few (k = 8,
// m = 64) product + compare cost 0.63 / 0.45 / 0.42 ms, while at 2 a k = 3
// product pays a level for nothing (0.26 against 0.20 ms).
// PA_SEGPROD_SERIAL_MAX overrides (A/B measurements).
size_t segprod_serial_max() {
    static const size_t v = (size_t)env_clamp("PA_SEGPROD_SERIAL_MAX", 4, 1, LLONG_MAX);
    return v;
}

hipError_t launch_fq12_segmented_product(uint64_t* work, const uint64_t* offsets, size_t n, size_t m, size_t max_len,
                                         uint64_t* prod, hipStream_t stream) {
    if (m == 0) return hipSuccess;
    const size_t cap = segprod_serial_max();
    int levels = 0;
    for (size_t len = max_len; len > cap; len = (len + 1) / 2) {
        hipLaunchKernelGGL(k_fq12_seg_level, dim3(blocks_for(n, 64)), dim3(64), 0, stream, work, offsets, m, n, levels,
                           cap);
        hipError_t e = hipGetLastError();
        if (e != hipSuccess) return e;
        levels++;
    }
    hipLaunchKernelGGL(k_fq12_seg_product, dim3(blocks_for(m, 64)), dim3(64), 0, stream, work, offsets, prod, m, levels,
                       cap);
    return hipGetLastError();
}

hipError_t launch_fq12_is_one(const uint64_t* out, const uint8_t* ok, uint8_t* is_one, size_t m, hipStream_t stream) {
    if (m == 0) return hipSuccess;
    hipLaunchKernelGGL(k_fq12_is_one, dim3(blocks_for(m, 64)), dim3(64), 0, stream, out, ok, is_one, m);
    return hipGetLastError();
}

}  // namespace pa
