// R1CS matrices on the device and their product with k witness vectors: the
// evaluations of A, B and C over the domain that the quotient of a Groth16
// proof starts from (pa_r1cs_*, include/pairing_amd.h).
//
// Image (built once on the host by r1cs_build): every row of the three
// matrices is cut into chunks of at most kR1csChunkLen terms, an empty row is
// one chunk of no terms.  64 consecutive chunks form a slab, the work of one
// wave: lane l sums chunk 64 s + l.  A slab stores its terms term-major,
//     val[(off_s + 64 t + l)]  (32 B)     col[off_s + 64 t + l]  (4 B)
// for t < len_s = the longest chunk of the slab, so the wave's loads of term t
// are 2 KiB and 256 B of consecutive bytes; shorter chunks are padded with
// zero terms that their lanes skip.  The slabs of A, B and C follow one
// another and run in one launch; blockIdx.y is the witness.
//
// A chunk that is its row's only one stores the sum to the row (every row below
// n_rows is written by exactly one lane, with no atomics).  The chunks of a row
// of several store partial sums to the workspace; k_r1cs_fold then adds a row's
// partial sums, one wave per such row (Fr addition is exact: any order gives
// the same canonical value).  Rows n_rows .. n - 1 are zeroed by the tail
// blocks of the first launch.
#include "fr.h"
#include "launch_groth16.h"

namespace pa {

constexpr uint32_t kR1csPartial = 0x80000000u;   // chunk_dst: a partial-sum slot, not a row

// One lane per chunk.  sl.first[m] = first slab of matrix m (A, B, C), sl.first[3] = slabs in all.
__global__ void __launch_bounds__(256) k_r1cs_chunks(const uint64_t* __restrict__ val, const uint32_t* __restrict__ col,
                                                     const uint64_t* __restrict__ slab_off,
                                                     const uint32_t* __restrict__ slab_len,
                                                     const uint32_t* __restrict__ chunk_len,
                                                     const uint32_t* __restrict__ chunk_dst, R1csSlabs sl,
                                                     const uint64_t* __restrict__ witness, size_t n_cols,
                                                     size_t n_rows, size_t n, uint64_t* __restrict__ a,
                                                     uint64_t* __restrict__ b, uint64_t* __restrict__ c,
                                                     uint64_t* __restrict__ partial, size_t n_partial,
                                                     unsigned slab_blocks) {
    const size_t j = blockIdx.y;   // witness
    if (blockIdx.x >= slab_blocks) {
        // zero rows n_rows .. n - 1 of the three outputs
        const size_t pad = n - n_rows;
        const size_t i = (size_t)(blockIdx.x - slab_blocks) * 256 + threadIdx.x;
        if (i >= 3 * pad) return;
        const size_t m = i / pad, row = n_rows + (i - m * pad);
        uint64_t* out = m == 0 ? a : (m == 1 ? b : c);
        Fr z;
        fr_zero(z);
        fr_store(out + 4 * (j * n + row), z);
        return;
    }
    const size_t slab = (size_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (slab >= sl.first[3]) return;
    const unsigned lane = threadIdx.x & 63;
    const size_t chunk = slab * 64 + lane;
    const uint32_t len = chunk_len[chunk];   // padded to whole slabs: 0 and no destination past the last chunk
    const uint32_t dst = chunk_dst[chunk];
    const size_t off = slab_off[slab] + lane;
    const uint64_t* w = witness + 4 * j * n_cols;
    Fr acc;
    fr_zero(acc);
    const uint32_t slen = slab_len[slab];
    for (uint32_t t = 0; t < slen; t++) {
        if (t < len) {
            const size_t e = off + (size_t)t * 64;
            Fr v, x, p;
            fr_load(v, val + 4 * e);
            fr_load(x, w + 4 * (size_t)col[e]);
            fr_mul(p, v, x);
            fr_add(acc, acc, p);
        }
    }
    if (dst == 0xffffffffu) return;   // the padding of the last slab of a matrix
    if (dst & kR1csPartial) {
        fr_store(partial + 4 * (j * n_partial + (dst & ~kR1csPartial)), acc);
    } else {
        uint64_t* out = slab < sl.first[1] ? a : (slab < sl.first[2] ? b : c);
        fr_store(out + 4 * (j * n + dst), acc);
    }
}

// One wave per row of several chunks: fold[4 i] = first partial slot, [4 i + 1] = slots, [4 i + 2] = matrix,
// [4 i + 3] = row.
__global__ void __launch_bounds__(64) k_r1cs_fold(const uint32_t* __restrict__ fold, const uint64_t* __restrict__ partial,
                                                  size_t n_partial, size_t n, uint64_t* __restrict__ a,
                                                  uint64_t* __restrict__ b, uint64_t* __restrict__ c) {
    __shared__ uint32_t sh[64 * 8];
    const size_t j = blockIdx.y;
    const uint32_t first = fold[4 * blockIdx.x], cnt = fold[4 * blockIdx.x + 1], m = fold[4 * blockIdx.x + 2],
                   row = fold[4 * blockIdx.x + 3];
    const unsigned lane = threadIdx.x;
    const uint64_t* p = partial + 4 * (j * n_partial + first);
    Fr acc;
    fr_zero(acc);
    for (uint32_t t = lane; t < cnt; t += 64) {
        Fr x;
        fr_load(x, p + 4 * (size_t)t);
        fr_add(acc, acc, x);
    }
#pragma unroll
    for (int i = 0; i < 8; i++) sh[i * 64 + lane] = acc.w[i];
    __syncthreads();
    for (unsigned half = 32; half > 0; half >>= 1) {
        if (lane < half) {
            Fr x;
#pragma unroll
            for (int i = 0; i < 8; i++) x.w[i] = sh[i * 64 + lane + half];
            fr_add(acc, acc, x);
#pragma unroll
            for (int i = 0; i < 8; i++) sh[i * 64 + lane] = acc.w[i];
        }
        __syncthreads();
    }
    if (lane == 0) {
        uint64_t* out = m == 0 ? a : (m == 1 ? b : c);
        fr_store(out + 4 * (j * n + row), acc);
    }
}

// ---- the image, built on the host ----
namespace {
inline size_t align_up(size_t v, size_t a) { return (v + a - 1) / a * a; }
}  // namespace

void r1cs_build(const R1csCsr m[3], size_t n_rows, R1csImage& img) {
    constexpr size_t L = kR1csChunkLen;
    img = R1csImage{};
    // pass 1: chunks per matrix, partial slots, rows to fold
    size_t chunks_total = 0;
    for (int mi = 0; mi < 3; mi++) {
        img.slabs.first[mi] = chunks_total / 64;
        size_t chunks = 0;
        for (size_t r = 0; r < n_rows; r++) {
            const size_t len = m[mi].row_ptr[r + 1] - m[mi].row_ptr[r];
            const size_t rc = len ? (len + L - 1) / L : 1;
            chunks += rc;
            if (rc > 1) {
                img.n_partial += rc;
                img.n_fold++;
            }
        }
        chunks_total += align_up(chunks, 64);
    }
    img.slabs.first[3] = chunks_total / 64;
    const size_t n_slabs = chunks_total / 64;
    img.chunk_len.assign(chunks_total, 0);
    img.chunk_dst.assign(chunks_total, 0xffffffffu);
    img.slab_off.assign(n_slabs, 0);
    img.slab_len.assign(n_slabs, 0);
    img.fold.reserve(4 * img.n_fold);
    // pass 2: chunk descriptors
    std::vector<uint64_t> chunk_src(chunks_total, 0);   // first term of the chunk in its matrix's CSR
    uint32_t slot = 0;
    for (int mi = 0; mi < 3; mi++) {
        size_t ch = img.slabs.first[mi] * 64;
        for (size_t r = 0; r < n_rows; r++) {
            const uint64_t lo = m[mi].row_ptr[r], hi = m[mi].row_ptr[r + 1];
            const size_t len = hi - lo;
            const size_t rc = len ? (len + L - 1) / L : 1;
            if (rc > 1) {
                img.fold.push_back(slot);
                img.fold.push_back((uint32_t)rc);
                img.fold.push_back((uint32_t)mi);
                img.fold.push_back((uint32_t)r);
            }
            for (size_t q = 0; q < rc; q++, ch++) {
                const size_t cl = len - q * L < L ? len - q * L : L;
                img.chunk_len[ch] = (uint32_t)cl;
                img.chunk_dst[ch] = rc > 1 ? (kR1csPartial | slot++) : (uint32_t)r;
                chunk_src[ch] = lo + q * L;
            }
        }
    }
    // pass 3: slab extents and the term-major term arrays
    size_t entries = 0;
    for (size_t s = 0; s < n_slabs; s++) {
        uint32_t mx = 0;
        for (size_t l = 0; l < 64; l++) mx = img.chunk_len[s * 64 + l] > mx ? img.chunk_len[s * 64 + l] : mx;
        img.slab_off[s] = entries;
        img.slab_len[s] = mx;
        entries += (size_t)mx * 64;
    }
    img.entries = entries;
    img.val.assign(4 * entries, 0);
    img.col.assign(entries, 0);
    for (int mi = 0; mi < 3; mi++)
        for (size_t s = img.slabs.first[mi]; s < img.slabs.first[mi + 1]; s++)
            for (size_t l = 0; l < 64; l++) {
                const size_t ch = s * 64 + l;
                for (uint32_t t = 0; t < img.chunk_len[ch]; t++) {
                    const size_t e = img.slab_off[s] + (size_t)t * 64 + l, src = chunk_src[ch] + t;
                    img.col[e] = m[mi].col[src];
                    for (int q = 0; q < 4; q++) img.val[4 * e + q] = m[mi].val[4 * src + q];
                }
            }
}

R1csDevLayout r1cs_dev_layout(const R1csImage& img) {
    R1csDevLayout d{};
    size_t o = 0;
    d.val = o;       o = align_up(o + img.val.size() * 8, 256);
    d.col = o;       o = align_up(o + img.col.size() * 4, 256);
    d.slab_off = o;  o = align_up(o + img.slab_off.size() * 8, 256);
    d.slab_len = o;  o = align_up(o + img.slab_len.size() * 4, 256);
    d.chunk_len = o; o = align_up(o + img.chunk_len.size() * 4, 256);
    d.chunk_dst = o; o = align_up(o + img.chunk_dst.size() * 4, 256);
    d.fold = o;      o = align_up(o + img.fold.size() * 4, 256);
    d.bytes = o;
    return d;
}

hipError_t launch_r1cs_eval(const R1csDev& r, const uint64_t* witness, size_t k, unsigned log_n, uint64_t* a,
                            uint64_t* b, uint64_t* c, void* workspace, hipStream_t stream) {
    return launch_r1cs_eval(r, witness, k, (size_t)1 << log_n, a, b, c, workspace, stream);
}

hipError_t launch_r1cs_eval(const R1csDev& r, const uint64_t* witness, size_t k, size_t n, uint64_t* a, uint64_t* b,
                            uint64_t* c, void* workspace, hipStream_t stream) {
    if (k == 0) return hipSuccess;
    const uint8_t* base = static_cast<const uint8_t*>(r.image);
    const unsigned slab_blocks = (unsigned)((r.slabs.first[3] + 3) / 4);
    const size_t pad_blocks = (3 * (n - r.n_rows) + 255) / 256;
    uint64_t* partial = static_cast<uint64_t*>(workspace);
    // blockIdx.y is the witness: a launch covers at most 65535 of them
    for (size_t j0 = 0; j0 < k; j0 += 65535) {
        const size_t kk = k - j0 < 65535 ? k - j0 : 65535;
        const uint64_t* w = witness + 4 * j0 * r.n_cols;
        uint64_t *aj = a + 4 * j0 * n, *bj = b + 4 * j0 * n, *cj = c + 4 * j0 * n;
        uint64_t* pj = partial ? partial + 4 * j0 * r.n_partial : nullptr;
        if (slab_blocks + pad_blocks) {
            hipLaunchKernelGGL(k_r1cs_chunks, dim3((unsigned)(slab_blocks + pad_blocks), (unsigned)kk), dim3(256), 0,
                               stream, (const uint64_t*)(base + r.layout.val), (const uint32_t*)(base + r.layout.col),
                               (const uint64_t*)(base + r.layout.slab_off), (const uint32_t*)(base + r.layout.slab_len),
                               (const uint32_t*)(base + r.layout.chunk_len),
                               (const uint32_t*)(base + r.layout.chunk_dst), r.slabs, w, r.n_cols, r.n_rows, n, aj, bj,
                               cj, pj, r.n_partial, slab_blocks);
            if (hipError_t e = hipGetLastError(); e != hipSuccess) return e;
        }
        if (r.n_fold) {
            hipLaunchKernelGGL(k_r1cs_fold, dim3((unsigned)r.n_fold, (unsigned)kk), dim3(64), 0, stream,
                               (const uint32_t*)(base + r.layout.fold), pj, r.n_partial, n, aj, bj, cj);
            if (hipError_t e = hipGetLastError(); e != hipSuccess) return e;
        }
    }
    return hipSuccess;
}

}  // namespace pa
