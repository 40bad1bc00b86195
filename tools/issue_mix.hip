// Issue cost per instruction class on the MI355X, for the generated pairing
// kernels' two classes: v_mad_u64_u32 (one dependent accumulator chain, carry
// to VCC, as tools/pgen/emit.py emits a product column) and the cheap VALU
// around it (v_add_u32 / v_cndmask_b32 on other registers), mixed at
// mad : cheap = 1:0, 2:1, 1:1 and 0:1, at 1 and 2 waves per SIMD.
//
// Every wave runs ITERS x 24 instructions of the mix; the shader clock is read
// with s_memtime against s_memrealtime (100 MHz) around the loop, the kernel
// time with HIP events.  1024 x w one-wave blocks put w waves on each of the
// 1024 SIMDs (256 CUs x 4).  Output per configuration: clocks per instruction
// per SIMD (a wave's clocks / its instructions / w), and the cost of a cheap
// instruction implied by the mix when a mad costs what the 1:0 stream says:
// (clk of the mix - mads x clk per mad) / cheap instructions.
//
// Build: hipcc -O3 --offload-arch=gfx950 tools/issue_mix.hip -o tools/issue_mix
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdio.h>

#define M "v_mad_u64_u32 %[x], vcc, %[a], %[b], %[x]\n"
#define C0 "v_add_u32 %[y0], %[y0], %[a]\n"
#define C1 "v_cndmask_b32_e64 %[y1], %[y1], %[b], %[m]\n"
#define C2 "v_add_u32 %[y2], %[y2], %[b]\n"
#define C3 "v_cndmask_b32_e64 %[y3], %[y3], %[a], %[m]\n"
#define M4 M M M M
#define C4 C0 C1 C2 C3

// MODE 0: 24 mads; 1: 16 mads + 8 cheap (M M C); 2: 12 + 12 (M C); 3: 24 cheap
template <int MODE>
__global__ void __launch_bounds__(64) k(uint64_t* out, int iters, uint32_t seed) {
    uint64_t t0, r0, t1, r1;
    asm volatile("s_memtime %0\n s_memrealtime %1\n s_waitcnt lgkmcnt(0)" : "=s"(t0), "=s"(r0));
    uint32_t a = threadIdx.x ^ seed, b = blockIdx.x + seed;
    uint64_t x = a;
    const uint64_t mask = 0x5555555555555555ull;  // the cndmasks' lane mask (the odd lanes of lane pairs)
    uint32_t y0 = a, y1 = a + 1, y2 = a + 2, y3 = a + 3;
    for (int it = 0; it < iters; it++) {
        if (MODE == 0) {
            asm volatile(M4 M4 M4 M4 M4 M4
                         : [x] "+v"(x), [y0] "+v"(y0), [y1] "+v"(y1), [y2] "+v"(y2), [y3] "+v"(y3)
                         : [a] "v"(a), [b] "v"(b), [m] "s"(mask) : "vcc");
        } else if (MODE == 1) {
            asm volatile(M M C0 M M C1 M M C2 M M C3 M M C0 M M C1 M M C2 M M C3
                         : [x] "+v"(x), [y0] "+v"(y0), [y1] "+v"(y1), [y2] "+v"(y2), [y3] "+v"(y3)
                         : [a] "v"(a), [b] "v"(b), [m] "s"(mask) : "vcc");
        } else if (MODE == 2) {
            asm volatile(M C0 M C1 M C2 M C3 M C0 M C1 M C2 M C3 M C0 M C1 M C2 M C3
                         : [x] "+v"(x), [y0] "+v"(y0), [y1] "+v"(y1), [y2] "+v"(y2), [y3] "+v"(y3)
                         : [a] "v"(a), [b] "v"(b), [m] "s"(mask) : "vcc");
        } else {
            asm volatile(C4 C4 C4 C4 C4 C4
                         : [x] "+v"(x), [y0] "+v"(y0), [y1] "+v"(y1), [y2] "+v"(y2), [y3] "+v"(y3)
                         : [a] "v"(a), [b] "v"(b), [m] "s"(mask) : "vcc");
        }
    }
    asm volatile("s_memtime %0\n s_memrealtime %1\n s_waitcnt lgkmcnt(0)" : "=s"(t1), "=s"(r1));
    if (threadIdx.x == 0) {
        out[3 * blockIdx.x] = t1 - t0;
        out[3 * blockIdx.x + 1] = r1 - r0;
        out[3 * blockIdx.x + 2] = x ^ y0 ^ y1 ^ y2 ^ y3;
    }
}

struct Result {
    double clk_per_instr;  // per SIMD
    double ms, mhz;
};

template <int MODE>
Result run(uint64_t* d, uint64_t* h, int w, int iters) {
    const int blocks = 1024 * w;
    k<MODE><<<blocks, 64>>>(d, iters, 1);  // warm-up (clock ramp)
    hipEvent_t e0, e1;
    (void)hipEventCreate(&e0);
    (void)hipEventCreate(&e1);
    (void)hipEventRecord(e0);
    k<MODE><<<blocks, 64>>>(d, iters, 2);
    (void)hipEventRecord(e1);
    (void)hipEventSynchronize(e1);
    Result r;
    float ms;
    (void)hipEventElapsedTime(&ms, e0, e1);
    (void)hipMemcpy(h, d, 3 * 8 * blocks, hipMemcpyDeviceToHost);
    double clk = 0, rt = 0;
    for (int b = 0; b < blocks; b++) {
        clk += h[3 * b];
        rt += h[3 * b + 1];
    }
    r.ms = ms;
    r.mhz = clk / rt * 100.0;
    r.clk_per_instr = (clk / blocks) / (24.0 * iters) / w;
    (void)hipEventDestroy(e0);
    (void)hipEventDestroy(e1);
    return r;
}

int main() {
    const int maxb = 1024 * 2;
    uint64_t* d;
    if (hipMalloc(&d, 3 * 8 * maxb) != hipSuccess) return 1;
    static uint64_t h[3 * maxb];
    const int iters = 20000;
    static const char* const name[4] = {"1:0", "2:1", "1:1", "0:1"};
    static const double mad_share[4] = {1.0, 2.0 / 3.0, 0.5, 0.0};
    for (int w : {1, 2}) {
        Result r[4] = {run<0>(d, h, w, iters / w), run<1>(d, h, w, iters / w), run<2>(d, h, w, iters / w),
                       run<3>(d, h, w, iters / w)};
        for (int m = 0; m < 4; m++) {
            printf("waves/SIMD=%d mad:cheap=%s: %8.3f ms, clock %4.0f MHz, %5.2f clk/instr/SIMD", w, name[m], r[m].ms,
                   r[m].mhz, r[m].clk_per_instr);
            if (m)
                printf(", cheap at the 1:0 mad cost: %5.2f clk",
                       (r[m].clk_per_instr - mad_share[m] * r[0].clk_per_instr) / (1.0 - mad_share[m]));
            printf("\n");
        }
    }
    (void)hipFree(d);
    return 0;
}
