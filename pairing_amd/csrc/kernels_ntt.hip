// Batched number-theoretic transforms over Fr: the four transforms of a
// radix-2 evaluation domain (forward, inverse and their coset forms, natural
// order in and out), bit-exact because every value is canonical Fr.
//
// A transform of n = 2^k points runs as ceil(k / T) passes over HBM, T the
// tile log (PA_NTT_TILE_LOG, default 10).  With k = t_1 + ... + t_p (every
// t_q = T but the last) and N_q = 2^t_q, pass q sees the data as blocks of
// M_q = n / (N_1 ... N_(q-1)) rows and does, for every block and every
// r < S_q = M_q / N_q, the N_q-point transform of the rows r + a S_q, then
// multiplies output j by w_(M_q)^(r j) and stores it where input row j was
// (Cooley-Tukey decimation in frequency over digits instead of bits).  The
// last pass has S = 1 and no twiddle; it writes row (j_1, ..., j_p) of the
// in-place order to its natural index j_1 + N_1 j_2 + ... (digit reversal), so
// it cannot run in place: passes go in -> workspace -> ... -> out.
//
// A workgroup of 256 threads holds 2^11 rows (2^12, 128 KiB of LDS, at T = 12):
// one tile of N_q rows for each of C = 2^11 / N_q columns.  Columns are what
// makes the HBM accesses wide:
//   - one launch (k <= T): the columns are C whole polynomials of the batch;
//   - a strided pass: C adjacent values of r, so each gathered piece is C x 32
//     contiguous bytes (C = 2 at T = 10, 4 at T = 9);
//   - the last of several passes: C adjacent values of j_1, contiguous in the
//     output.
// Inside a tile the t stages run in rounds of up to three: a thread keeps 2^R
// rows that differ in R index bits in registers (8 rows = 64 VGPRs), does the R
// stages on them and exchanges through LDS only between rounds.  The first
// round loads from HBM and the last stores to HBM straight from registers.
// LDS holds the rows as eight word planes, row p of a plane at p ^ (p >> 3):
// ds_read_b32 / ds_write_b32 serve 32 lanes per cycle over 32 banks, and with
// that swizzle the 32 rows of a half wave fall in distinct banks for a
// three-bit window at any position (two-way for the one- and two-bit windows
// of the leftover round).  The one exchange that is read bit-reversed (into
// the last round of a one-launch transform) would be 4- to 16-way under it
// from 2^8 points up and has a swizzle of its own (ntt_swz): two-way at worst.
// Every exchange of every tile shape is enumerated in DESIGN.md, "Fr NTT".
//
// The quotient of a proof, h = (A B - C) / Z from evaluations (launch_ntt_quotient),
// is seven of these transforms in 3 x passes launches: k_ntt_pass3 runs a pass
// over a, b and c in one grid, and its fused form loads A B - C as the first
// round of the last transform; the constants ride on coset tables.
#include "fr.h"
#include "launch.h"

namespace pa {
namespace {

constexpr unsigned kNttThreads = 256;

struct NttPass {
    const uint64_t* in;
    uint64_t* out;
    const uint64_t *tw, *lo, *hi, *glo, *ghi, *scale;
    size_t batch;
    uint32_t log_n, split, t, cbits, tw_shift;
    uint32_t kind;        // 0 one launch (columns = polynomials), 1 strided pass, 2 last of several passes
    uint32_t m;           // kind 1: log2 of the block M_q
    uint32_t t1;          // kind 2: log2 of N_1
    uint32_t digits, digit_bits;   // kind 2: the digits j_2 .. j_(p-1) between j_1 and this pass
    uint32_t pre_coset, post_tw, post_coset, post_scale;
};

// One copy of the multiply in the kernel: the butterflies, the pass twiddles
// and the coset factors call it (operands and result travel in VGPRs).
// Inlined at every site, and with a stage's twiddles loaded ahead of its
// products, the kernel measured 1.3-1.6 x slower ("Fr NTT").
__device__ __noinline__ Fr ntt_mul(Fr a, Fr b) {
    Fr r;
    fr_mul(r, a, b);
    return r;
}

PA_DEV uint32_t ntt_bitrev(uint32_t x, uint32_t bits) { return bits ? __brev(x) >> (32 - bits) : 0u; }
// Where row p (of 2^len rows, the low cb bits its column) sits in an LDS word
// plane.  Every exchange but one uses p ^ (p >> 3).  The exchange before the
// last round of a one-launch transform (`fin`) is read with the rows
// bit-reversed: the lanes of a half wave then differ in the column bits and in
// the top 5 - cb row bits, which that swizzle leaves out of the bank; there
// those top bits, reversed, are folded in above the column bits as well.
// The fold depends on the top row bits only, which no window of these two
// rounds reaches (len >= 11, windows below bit cb + 6): one value per group.
PA_DEV uint32_t ntt_swz_fold(uint32_t p, bool fin, uint32_t len, uint32_t cb) {
    return fin && cb < 5 ? ntt_bitrev(p >> (len - (5 - cb)), 5 - cb) << cb : 0u;
}
PA_DEV uint32_t ntt_swz(uint32_t p, uint32_t fold) { return p ^ (p >> 3) ^ fold; }

// base^e from the two-level tables: lo[e mod 2^split] * hi[e >> split]
PA_DEV Fr ntt_power(const uint64_t* lo, const uint64_t* hi, uint32_t e, uint32_t split, bool two) {
    Fr r;
    fr_load(r, lo + 4 * (size_t)(e & ((1u << split) - 1)));
    if (two) {
        Fr h;
        fr_load(h, hi + 4 * (size_t)(e >> split));
        r = ntt_mul(r, h);
    }
    return r;
}

struct NttTile {
    size_t in_base, out_base, sa_in, sc_in, sa_out, sc_out;
    uint32_t r0;        // kind 1: r of column 0
    uint32_t cols;      // live columns (the batch's tail in a one-launch transform)
};

// One round: the stages of row-index bits [lo, lo + R) on the 2^R rows a
// thread holds, for every group of rows of the workgroup.
// F (the quotient's last transform): the first round loads in * fb - fc, the
// rows of three arrays at one index, where the plain pass loads `in`.
template <int R, bool F>
PA_DEV void ntt_round(const NttPass& a, const NttTile& tile, uint32_t* lds, uint32_t lo, bool first, bool last,
                      const uint64_t* fb, const uint64_t* fc) {
    constexpr int M = 1 << R;
    const uint32_t t = a.t, cb = a.cbits;
    const uint32_t elems = 1u << (t + cb);
    const uint32_t groups = elems >> R;
    const uint32_t nmask = (1u << a.log_n) - 1;
    const bool two = a.log_n > a.split;
    // the exchange into the bit-reversed last round (the round after a window at lo <= 3 is the last)
    const bool fin_read = last && a.kind == 0, fin_write = !last && lo <= 3 && a.kind == 0;
    for (uint32_t g = threadIdx.x; g < groups; g += kNttThreads) {
        const uint32_t c = g & ((1u << cb) - 1);
        const uint32_t gr = g >> cb;   // the t - R row bits outside the window
        // the last round of a one-launch transform takes its rows bit-reversed, so
        // that consecutive lanes store consecutive output rows
        const bool rev = last && a.kind == 0;
        const uint32_t rows = rev ? ntt_bitrev(gr, t - R) : gr;
        const uint32_t x0 = ((rows >> lo) << (lo + R)) | (rows & ((1u << lo) - 1));
        const bool live = c < tile.cols;
        const uint32_t fold = ntt_swz_fold(x0 << cb, fin_read || fin_write, t + cb, cb);
        Fr v[M];
        if (first) {
#pragma unroll
            for (int m = 0; m < M; m++) {
                const uint32_t x = x0 | ((uint32_t)m << lo);
                const size_t idx = tile.in_base + (size_t)x * tile.sa_in + (size_t)c * tile.sc_in;
                if (live) {
                    fr_load(v[m], a.in + 4 * idx);
                    if constexpr (F) {
                        Fr y;
                        fr_load(y, fb + 4 * idx);
                        v[m] = ntt_mul(v[m], y);
                        fr_load(y, fc + 4 * idx);
                        fr_sub(v[m], v[m], y);
                    }
                    if (a.pre_coset) v[m] = ntt_mul(v[m], ntt_power(a.glo, a.ghi, (uint32_t)idx & nmask, a.split, two));
                } else {
                    fr_zero(v[m]);
                }
            }
        } else {
#pragma unroll
            for (int m = 0; m < M; m++) {
                const uint32_t q = ntt_swz(((x0 | ((uint32_t)m << lo)) << cb) | c, fin_read ? fold : 0u);
#pragma unroll
                for (int w = 0; w < 8; w++) v[m].w[w] = lds[w * elems + q];
            }
        }
#pragma unroll
        for (int i = R - 1; i >= 0; i--) {
            const uint32_t b = lo + i;   // pairs (x, x + 2^b), twiddle w_N^((x mod 2^b) 2^(t-1-b))
#pragma unroll
            for (int m = 0; m < M; m++) {
                if ((m >> i) & 1) continue;
                const Fr u = v[m], w = v[m | (1 << i)];
                Fr d;
                fr_add(v[m], u, w);
                fr_sub(d, u, w);
                if (b != 0) {   // the last stage's twiddles are all one
                    const uint32_t xl = (x0 & ((1u << lo) - 1)) | (((uint32_t)m & ((1u << i) - 1)) << lo);
                    Fr tw;
                    fr_load(tw, a.tw + 4 * (size_t)((xl << (t - 1 - b)) << a.tw_shift));
                    d = ntt_mul(d, tw);
                }
                v[m | (1 << i)] = d;
            }
        }
        if (last) {
            // lo = 0: row x0 | m holds output bitrev_t(x0 | m)
            const uint32_t jl = rev ? gr : ntt_bitrev(gr, t - R);
#pragma unroll
            for (int m = 0; m < M; m++) {
                if (!live) continue;
                const uint32_t j = jl | (ntt_bitrev((uint32_t)m, R) << (t - R));
                const size_t idx = tile.out_base + (size_t)j * tile.sa_out + (size_t)c * tile.sc_out;
                Fr o = v[m];
                if (a.post_tw)
                    o = ntt_mul(o, ntt_power(a.lo, a.hi, ((tile.r0 + c) * j) << (a.log_n - a.m), a.split, two));
                if (a.post_coset) {
                    o = ntt_mul(o, ntt_power(a.glo, a.ghi, (uint32_t)idx & nmask, a.split, two));
                } else if (a.post_scale) {
                    Fr s;
                    fr_load(s, a.scale);
                    o = ntt_mul(o, s);
                }
                fr_store(a.out + 4 * idx, o);
            }
        } else {
#pragma unroll
            for (int m = 0; m < M; m++) {
                const uint32_t q = ntt_swz(((x0 | ((uint32_t)m << lo)) << cb) | c, fin_write ? fold : 0u);
#pragma unroll
                for (int w = 0; w < 8; w++) lds[w * elems + q] = v[m].w[w];
            }
        }
    }
}

// One workgroup's tile of a pass: `wg` counts the tiles of one array.
template <bool F>
PA_DEV void ntt_pass_tile(const NttPass& a, size_t wg, uint32_t* ntt_lds, const uint64_t* fb, const uint64_t* fc) {
    const uint32_t t = a.t, cb = a.cbits;
    NttTile tile;
    tile.r0 = 0;
    tile.cols = 1u << cb;
    if (a.kind == 0) {
        const size_t p0 = wg << cb;
        tile.in_base = tile.out_base = p0 << t;
        tile.sa_in = tile.sa_out = 1;
        tile.sc_in = tile.sc_out = (size_t)1 << t;
        if (a.batch - p0 < tile.cols) tile.cols = (uint32_t)(a.batch - p0);
    } else if (a.kind == 1) {
        const uint32_t tb = a.m - t - cb;   // log2 of the tiles in a block
        tile.r0 = (uint32_t)(wg & (((size_t)1 << tb) - 1)) << cb;
        tile.in_base = tile.out_base = ((wg >> tb) << a.m) + tile.r0;
        tile.sa_in = tile.sa_out = (size_t)1 << (a.m - t);
        tile.sc_in = tile.sc_out = 1;
    } else {
        const uint32_t rest_bits = a.digits * a.digit_bits;
        const uint32_t cw = a.t1 - cb;   // log2 of the column chunks of j_1
        const size_t poly = wg >> (cw + rest_bits);
        const uint32_t w = (uint32_t)(wg & (((size_t)1 << (cw + rest_bits)) - 1));
        const uint32_t j1 = (w & ((1u << cw) - 1)) << cb;
        uint32_t rest = w >> cw, rrev = 0;
        tile.in_base = (poly << a.log_n) + ((((size_t)j1 << rest_bits) + rest) << t);
        for (uint32_t d = 0; d < a.digits; d++) {
            rrev = (rrev << a.digit_bits) | (rest & ((1u << a.digit_bits) - 1));
            rest >>= a.digit_bits;
        }
        tile.sa_in = 1;
        tile.sc_in = (size_t)1 << (rest_bits + t);
        tile.out_base = (poly << a.log_n) + j1 + ((size_t)rrev << a.t1);
        tile.sa_out = (size_t)1 << (a.log_n - t);
        tile.sc_out = 1;
    }
    uint32_t rem = t;
    bool first = true;
    while (rem) {
        const uint32_t r = rem == 4 ? 2u : (rem < 3 ? rem : 3u);
        const uint32_t lo = rem - r;
        if (r == 3)
            ntt_round<3, F>(a, tile, ntt_lds, lo, first, lo == 0, fb, fc);
        else if (r == 2)
            ntt_round<2, F>(a, tile, ntt_lds, lo, first, lo == 0, fb, fc);
        else
            ntt_round<1, F>(a, tile, ntt_lds, lo, first, lo == 0, fb, fc);
        rem = lo;
        first = false;
        if (rem) __syncthreads();
    }
}

__global__ void __launch_bounds__(kNttThreads, 2) k_ntt_pass(const NttPass a) {
    extern __shared__ uint32_t ntt_lds[];
    ntt_pass_tile<false>(a, blockIdx.x, ntt_lds, nullptr, nullptr);
}

// The quotient's launches (launch_ntt_quotient): the pass `p` over the arrays
// in[i] -> out[i], each with its own tiles (a batch tail per array in a
// one-launch transform) and its own low table of coset factors (which is
// where each array's constant rides).
struct NttPass3 {
    NttPass p;   // in, out and glo are taken from the arrays below
    const uint64_t* in[3];
    uint64_t* out[3];
    const uint64_t* glo[3];
    uint32_t tiles;   // workgroups per array
};

// F = false: three arrays, a grid of 3 x tiles.  F = true: one transform whose
// first round loads in[0] * in[1] - in[2] and writes out[0], a grid of `tiles`.
template <bool F>
__global__ void __launch_bounds__(kNttThreads, 2) k_ntt_pass3(const NttPass3 q) {
    extern __shared__ uint32_t ntt_lds[];
    NttPass a = q.p;
    uint32_t wg = blockIdx.x;
    if constexpr (F) {
        a.in = q.in[0], a.out = q.out[0], a.glo = q.glo[0];
    } else {
        const uint32_t arr = wg / q.tiles;   // the same for the whole workgroup: selects, no indexed copy of q
        wg -= arr * q.tiles;
        a.in = arr == 0 ? q.in[0] : (arr == 1 ? q.in[1] : q.in[2]);
        a.out = arr == 0 ? q.out[0] : (arr == 1 ? q.out[1] : q.out[2]);
        a.glo = arr == 0 ? q.glo[0] : (arr == 1 ? q.glo[1] : q.glo[2]);
    }
    ntt_pass_tile<F>(a, wg, ntt_lds, q.in[1], q.in[2]);
}

// log_n = 0, where the transforms are the identity: out = (a b - c) s, s = (g - 1)^-1
__global__ void __launch_bounds__(256) k_ntt_quotient_point(const uint64_t* a, const uint64_t* b, const uint64_t* c,
                                                            uint64_t* out, const uint64_t* s, size_t count) {
    Fr z;
    fr_load(z, s);
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < count; i += (size_t)gridDim.x * blockDim.x) {
        Fr x, y;
        fr_load(x, a + 4 * i);
        fr_load(y, b + 4 * i);
        fr_mul(x, x, y);
        fr_load(y, c + 4 * i);
        fr_sub(x, x, y);
        fr_mul(x, x, z);
        fr_store(out + 4 * i, x);
    }
}

// ---- the tables of a domain ----
PA_DEV void ntt_pow_u32(Fr& r, const Fr& base, uint32_t e) {
    Fr acc;
    fr_one(acc);
    for (int bit = 31; bit >= 0; bit--) {
        fr_sqr(acc, acc);
        if ((e >> bit) & 1) fr_mul(acc, acc, base);
    }
    r = acc;
}
PA_DEV void ntt_from_u32(Fr& r, uint32_t v) {
    Fr c;
    fr_zero(c);
    c.w[0] = v;
    fr_from_repr(r, c);
}

// 1 / Z on the coset, Z = X^n - 1: (g^n - 1)^-1
PA_DEV void ntt_zinv(Fr& r, uint32_t log_n) {
    Fr g, one;
    ntt_from_u32(g, 7);
    ntt_pow_u32(r, g, 1u << log_n);
    fr_one(one);
    fr_sub(r, r, one);   // g has order r - 1 > 2^28: never zero
    fr_inv(r, r);
}

// kind 0: out[i] = w_n^(+-(i << shift)); kind 1: out[i] = g^(+-(i << shift)), times n^-1 if `scaled`, and
// times 1 / Z as well if `scaled` is 2; kind 2: out[0] = n^-1; kind 3: out[0] = n^-1 / Z
__global__ void __launch_bounds__(64) k_ntt_table(uint64_t* out, uint32_t count, uint32_t kind, uint32_t log_n,
                                                  uint32_t shift, uint32_t inverse, uint32_t scaled) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= count) return;
    Fr r, ninv;
    if (kind != 0 && (kind >= 2 || scaled)) {
        Fr n;
        ntt_from_u32(n, 1u << log_n);
        fr_inv(ninv, n);
    }
    if (kind == 0) {
        Fr w;
        fr_root_of_unity(w);
        for (uint32_t s = log_n; s < 32; s++) fr_sqr(w, w);
        const uint32_t nmask = (1u << log_n) - 1;
        uint32_t e = (i << shift) & nmask;
        if (inverse) e = ((1u << log_n) - e) & nmask;
        ntt_pow_u32(r, w, e);
    } else if (kind == 1) {
        Fr g;
        ntt_from_u32(g, 7);   // GENERATOR, fr.rs:41-46
        if (inverse) fr_inv(g, g);
        ntt_pow_u32(r, g, i << shift);
        if (scaled) fr_mul(r, r, ninv);
        if (scaled == 2) {
            Fr z;
            ntt_zinv(z, log_n);
            fr_mul(r, r, z);
        }
    } else if (kind == 2) {
        r = ninv;
    } else {
        ntt_zinv(r, log_n);
        fr_mul(r, r, ninv);
    }
    fr_store(out + 4 * (size_t)i, r);
}

struct NttPlan {
    NttPass pass[kNttMaxLogN];
    size_t tiles[kNttMaxLogN];
    unsigned passes;
};

unsigned min_u(unsigned a, unsigned b) { return a < b ? a : b; }

// the passes of one call, without pointers
void ntt_plan(const NttLayout& l, size_t batch, NttPlan& plan) {
    const unsigned k = l.log_n, tl = l.tile_log, glog = ntt_group_log(l);
    plan.passes = l.passes;
    for (unsigned q = 0; q < l.passes; q++) {
        NttPass& p = plan.pass[q];
        p = NttPass{};
        p.batch = batch;
        p.log_n = k;
        p.split = l.split_log;
        const bool last = q + 1 == l.passes;
        p.t = last ? k - q * tl : tl;
        p.tw_shift = min_u(k, tl) - p.t;
        if (l.passes == 1) {
            p.kind = 0;
            p.cbits = glog - p.t;
            plan.tiles[q] = (batch + ((size_t)1 << p.cbits) - 1) >> p.cbits;
        } else if (!last) {
            p.kind = 1;
            p.m = k - q * tl;
            p.cbits = min_u(glog - p.t, p.m - p.t);
            p.post_tw = 1;
            plan.tiles[q] = (batch << k) >> (p.t + p.cbits);
        } else {
            p.kind = 2;
            p.t1 = tl;
            p.digits = l.passes - 2;
            p.digit_bits = tl;
            p.cbits = min_u(glog - p.t, p.t1);
            plan.tiles[q] = (batch << k) >> (p.t + p.cbits);
        }
    }
}

}  // namespace

NttLayout ntt_layout(unsigned log_n, unsigned tile_log) {
    NttLayout l{};
    l.log_n = log_n;
    l.tile_log = tile_log < 1 ? 1 : (tile_log > kNttMaxTileLog ? kNttMaxTileLog : tile_log);
    l.split_log = log_n < kNttSplitLog ? log_n : kNttSplitLog;
    l.passes = log_n == 0 ? 0 : (log_n + l.tile_log - 1) / l.tile_log;
    const unsigned tmax = log_n < l.tile_log ? log_n : l.tile_log;
    l.tile_rows = log_n == 0 ? 0 : (size_t)1 << (tmax - 1);
    l.lo_rows = (size_t)1 << l.split_log;
    l.hi_rows = (size_t)1 << (log_n - l.split_log);
    size_t at = 0;
    for (int d = 0; d < 2; d++) {
        l.tile[d] = at, at += l.tile_rows;
        l.lo[d] = at, at += l.lo_rows;
        l.hi[d] = at, at += l.hi_rows;
        l.glo[d] = at, at += l.lo_rows;
        l.ghi[d] = at, at += l.hi_rows;
    }
    l.ninv = at++;
    // the quotient's constants, after every row the transforms use
    l.qscale = at++;
    for (int i = 0; i < 2; i++) l.qglo[i] = at, at += l.lo_rows;
    l.rows = at;
    return l;
}

size_t ntt_polys_per_workgroup(const NttLayout& l) {
    return l.passes == 1 ? (size_t)1 << (ntt_group_log(l) - l.log_n) : 0;
}

size_t ntt_workspace_bytes(const NttLayout& l, size_t batch) { return l.passes > 1 ? (batch << l.log_n) * 32 : 0; }

bool ntt_batch_fits(const NttLayout& l, size_t batch) {
    if (batch > (((size_t)1 << 40) >> l.log_n)) return false;
    NttPlan plan;
    ntt_plan(l, batch, plan);
    for (unsigned q = 0; q < plan.passes; q++)
        if (plan.tiles[q] > 0xffffffull) return false;   // a grid holds fewer than 2^32 threads: 2^24 - 1 workgroups of 256
    return true;
}

hipError_t launch_ntt_build(const NttLayout& l, uint64_t* tables, hipStream_t stream) {
    struct Job {
        size_t at, count;
        uint32_t kind, shift, inverse, scaled;
    };
    const unsigned tmax = l.log_n < l.tile_log ? l.log_n : l.tile_log;
    if (ntt_group_log(l) > kNttGroupLog) {   // more than the 64 KiB a kernel may use unasked
        const void* kernels[3] = {reinterpret_cast<const void*>(k_ntt_pass),
                                  reinterpret_cast<const void*>(k_ntt_pass3<false>),
                                  reinterpret_cast<const void*>(k_ntt_pass3<true>)};
        for (const void* k : kernels) {
            const hipError_t e =
                hipFuncSetAttribute(k, hipFuncAttributeMaxDynamicSharedMemorySize, 32 << ntt_group_log(l));
            if (e != hipSuccess) return e;
        }
    }
    Job jobs[14];
    int nj = 0;
    for (uint32_t d = 0; d < 2; d++) {
        jobs[nj++] = {l.tile[d], l.tile_rows, 0, l.log_n - tmax, d, 0};
        jobs[nj++] = {l.lo[d], l.lo_rows, 0, 0, d, 0};
        jobs[nj++] = {l.hi[d], l.hi_rows, 0, l.split_log, d, 0};
        jobs[nj++] = {l.glo[d], l.lo_rows, 1, 0, d, d};   // the inverse low table carries n^-1
        jobs[nj++] = {l.ghi[d], l.hi_rows, 1, l.split_log, d, 0};
    }
    jobs[nj++] = {l.ninv, 1, 2, 0, 0, 0};
    jobs[nj++] = {l.qscale, 1, 3, 0, 0, 0};
    jobs[nj++] = {l.qglo[0], l.lo_rows, 1, 0, 0, 2};   // g^i n^-1 / Z
    jobs[nj++] = {l.qglo[1], l.lo_rows, 1, 0, 0, 1};   // g^i n^-1
    for (int j = 0; j < nj; j++) {
        if (!jobs[j].count) continue;
        hipLaunchKernelGGL(k_ntt_table, dim3((unsigned)((jobs[j].count + 63) / 64)), dim3(64), 0, stream,
                           tables + 4 * jobs[j].at, (uint32_t)jobs[j].count, jobs[j].kind, l.log_n, jobs[j].shift,
                           jobs[j].inverse, jobs[j].scaled);
        const hipError_t e = hipGetLastError();
        if (e != hipSuccess) return e;
    }
    return hipSuccess;
}

hipError_t launch_ntt(const NttLayout& l, const uint64_t* tables, int mode, const uint64_t* in, uint64_t* out,
                      size_t batch, void* workspace, hipStream_t stream) {
    if (batch == 0) return hipSuccess;
    if (mode < NTT_FORWARD || mode > NTT_COSET_INVERSE) return hipErrorInvalidValue;
    if (l.log_n == 0)   // one point: every mode is the identity (g^0 = n^-1 = 1)
        return in == out ? hipSuccess : hipMemcpyAsync(out, in, batch * 32, hipMemcpyDeviceToDevice, stream);
    if (!ntt_batch_fits(l, batch)) return hipErrorInvalidValue;
    NttPlan plan;
    ntt_plan(l, batch, plan);
    const int d = (mode == NTT_INVERSE || mode == NTT_COSET_INVERSE) ? 1 : 0;
    uint64_t* ws = static_cast<uint64_t*>(workspace);
    for (unsigned q = 0; q < plan.passes; q++) {
        NttPass& p = plan.pass[q];
        const bool first = q == 0, last = q + 1 == plan.passes;
        p.in = first ? in : ws;
        p.out = last ? out : ws;
        p.tw = tables + 4 * l.tile[d];
        p.lo = tables + 4 * l.lo[d];
        p.hi = tables + 4 * l.hi[d];
        p.glo = tables + 4 * l.glo[d];
        p.ghi = tables + 4 * l.ghi[d];
        p.scale = tables + 4 * l.ninv;
        p.pre_coset = first && mode == NTT_COSET_FORWARD;
        p.post_coset = last && mode == NTT_COSET_INVERSE;
        p.post_scale = last && mode == NTT_INVERSE;
        const size_t lds = (size_t)32 << (p.t + p.cbits);
        hipLaunchKernelGGL(k_ntt_pass, dim3((unsigned)plan.tiles[q]), dim3(kNttThreads), lds, stream, p);
        const hipError_t e = hipGetLastError();
        if (e != hipSuccess) return e;
    }
    return hipSuccess;
}

// ---- the quotient h = (A B - C) / Z of a proof, coefficients from evaluations ----
size_t ntt_quotient_workspace_bytes(const NttLayout& l, size_t batch) {
    if (l.log_n == 0) return 0;
    return (l.passes > 1 ? 6 : 3) * (batch << l.log_n) * 32;   // three coset evaluations, and a pass workspace for three arrays
}

bool ntt_quotient_fits(const NttLayout& l, size_t batch) {
    if (batch > (((size_t)1 << 40) / 3) || !ntt_batch_fits(l, 3 * batch)) return false;
    NttPlan plan;
    ntt_plan(l, batch, plan);
    for (unsigned q = 0; q < plan.passes; q++)
        if (3 * plan.tiles[q] > 0xffffffull) return false;   // each array has a batch tail of its own
    return true;
}

hipError_t launch_ntt_quotient(const NttLayout& l, const uint64_t* tables, const uint64_t* a, const uint64_t* b,
                               const uint64_t* c, uint64_t* out, size_t batch, void* workspace, hipStream_t stream) {
    if (batch == 0) return hipSuccess;
    if (!ntt_quotient_fits(l, batch)) return hipErrorInvalidValue;
    const uint64_t* ninv = tables + 4 * l.ninv;
    const uint64_t* qscale = tables + 4 * l.qscale;
    if (l.log_n == 0) {
        size_t blocks = (batch + 255) / 256;
        if (blocks > stream_cfg().max_blocks) blocks = stream_cfg().max_blocks;
        hipLaunchKernelGGL(k_ntt_quotient_point, dim3((unsigned)blocks), dim3(256), 0, stream, a, b, c, out, qscale,
                           batch);
        return hipGetLastError();
    }
    NttPlan plan;
    ntt_plan(l, batch, plan);
    const size_t words = (batch << l.log_n) * 4;   // u64 words of one array
    uint64_t* ev = static_cast<uint64_t*>(workspace);
    uint64_t* pw = ev + 3 * words;   // touched only by domains of several passes
    const uint64_t* src[3] = {a, b, c};
    // stage 0: the inverse transforms of a, b and c, left unscaled; stage 1: their coset forward transforms in
    // place, whose coset factors g^i carry the n^-1 stage 0 left out and, for a and c, 1 / Z as well
    // ((A B - C) / Z = (A / Z) B - C / Z); stage 2: the coset inverse transform of that product minus C / Z
    for (int stage = 0; stage < 3; stage++) {
        const int d = stage == 1 ? 0 : 1;
        for (unsigned q = 0; q < plan.passes; q++) {
            const bool first = q == 0, last = q + 1 == plan.passes;
            NttPass3 k{};
            NttPass& p = k.p;
            p = plan.pass[q];
            p.tw = tables + 4 * l.tile[d];
            p.lo = tables + 4 * l.lo[d];
            p.hi = tables + 4 * l.hi[d];
            p.glo = tables + 4 * l.glo[d];
            p.ghi = tables + 4 * l.ghi[d];
            p.pre_coset = first && stage == 1;
            p.post_coset = last && stage == 2;
            p.scale = ninv;   // not read: no stage has a post_scale
            k.tiles = (uint32_t)plan.tiles[q];
            for (int i = 0; i < 3; i++) {
                k.in[i] = first ? (stage == 0 ? src[i] : ev + i * words) : pw + i * words;
                k.out[i] = last ? ev + i * words : pw + i * words;
                k.glo[i] = stage == 1 ? tables + 4 * l.qglo[i == 1] : p.glo;
            }
            const size_t lds = (size_t)32 << (p.t + p.cbits);
            if (stage < 2) {
                hipLaunchKernelGGL(k_ntt_pass3<false>, dim3(3 * k.tiles), dim3(kNttThreads), lds, stream, k);
            } else if (first) {
                k.out[0] = last ? out : pw;
                hipLaunchKernelGGL(k_ntt_pass3<true>, dim3(k.tiles), dim3(kNttThreads), lds, stream, k);
            } else {
                p.in = pw;
                p.out = last ? out : pw;
                hipLaunchKernelGGL(k_ntt_pass, dim3(k.tiles), dim3(kNttThreads), lds, stream, p);
            }
            const hipError_t e = hipGetLastError();
            if (e != hipSuccess) return e;
        }
    }
    return hipSuccess;
}

}  // namespace pa
