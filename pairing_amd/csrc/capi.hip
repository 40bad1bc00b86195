// C ABI of pairing_amd (include/pairing_amd.h): argument checking, device
// buffers for the host-pointer entry points, error reporting.  No compute
// happens here; every entry point ends in a HIP kernel from
// the kernels_*.hip files or a generated code object (gen_launch.hip).
#include <atomic>
#include <hip/hip_runtime.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <chrono>
#include <mutex>
#include <string>
#include <thread>
#include <utility>
#include <vector>

#include "../../include/pairing_amd.h"
#include "env.h"
#include "launch.h"
#include "launch_groth16.h"
#include "launch_groth16_aggregate.h"
#include "launch_groth16_setup.h"
#include "launch_groth16_verify.h"
#include "launch_msm.h"

namespace {

thread_local std::string g_last_error;
// Pairing kernel selection (pa_set_pairing_kernel).  0 (default) by batch
// size, each where it is fastest (round 5, profiles/r05_regimes.txt):
//   n <= pq_min() (768): the cooperative kernels (kernels_coop.hip, a
//      quad-VM workgroup per pairing, ~270 k pairings/s from 1.6 ms);
//   n <= pq_max() (4096; round 6): the lane-group kernels
//      (kernels_pair_quad.hip: one pairing per 32 lanes, rounds of 2048 at
//      ~3.8 ms -- 2048 pairs 3.78 ms, 4096 6.45, where the quad VM took 7.63 /
//      the lane pairs 8.41);
//   n <= pair_max() (32768): the generated kernels with a lane pair per
//      pairing, at most one wave per SIMD: 8.4-9.3 ms whatever n (the
//      cooperative kernels up to coop_max() = 2304 when lane groups are off);
//   n <= pair_max() + tail_max() (34816; round 6): the first 32768 on lane
//      pairs and the tail on a forked stream, on the cooperative kernels up
//      to 832 tail pairings and the lane groups above (split_head below;
//      32769: 10.8 ms, 34816: 13.0, instead of 15.7);
//   n <= one_max() (34048): one lane per pairing (one wave per SIMD at most:
//      ~15.7 ms, where a second lane-pair wave on a few SIMDs costs 15.6-16.7;
//      with the pairing-only lane-pair Miller loop lane pairs win from ~34 000
//      pairs, profiles/r05_regimes_after_ml2p.txt -- 38912 before it, and
//      still 38912 for the Miller-loop-only entries, ml_one_max(), which the
//      tail split leaves alone);
//   larger: lane pairs again, two or more waves per SIMD (2^16: 16.7 ms
//      against 17.2 ms one lane; 2^17: 33.0 vs 34.1 ms).  Round 5 gave the
//      lane-pair final exponentiation the Karabina squarings and the
//      in-kernel binary GCD (8.7 ms at 2^16 instead of 12.3 ms).
// 1 -> lane pairs for every batch size; 2 -> cooperative for every batch
// size; 3 -> one lane per pairing for every batch size; 4 -> cooperative for
// every batch size on the round-2 one-wave VM (A/B against the quad VM).
// written by pa_set_pairing_kernel and read by launches from any host thread
std::atomic<int> g_pairing_variant{0};
int pairing_variant() { return g_pairing_variant.load(std::memory_order_relaxed); }

// the regime bounds: any count, for A/B measurements
size_t coop_max() {
    static const size_t v = pa::env_count("PA_COOP_MAX", 2304);
    return v;
}
size_t pair_max() {
    static const size_t v = pa::env_count("PA_PAIR_MAX", 32768);
    return v;
}
size_t one_max() {
    static const size_t v = pa::env_count("PA_ONE_MAX", 34048);
    return v;
}
// the same window's upper edge for the reference-form Miller loop alone (the
// Miller-loop entries: pa_miller_loop_fused_batch_device, pa_multi_miller_loop_affine):
// its lane-pair kernel is slower than the pairing-only one, so one lane per pairing
// wins up to 38912 pairs there (profiles/r05_regimes.txt)
size_t ml_one_max() {
    static const size_t v = pa::env_count("PA_ML_ONE_MAX", 38912);
    return v;
}
bool use_coop(size_t n) {
    const int v = pairing_variant();
    return v == 2 || v == 4 || (v == 0 && n <= coop_max());
}
// the lane-group kernels (kernels_pair_quad.hip, one pairing per 32 lanes):
// variant 5 every size; the default in (PA_PQ_MIN, PA_PQ_MAX] = (768, 4096]:
// a round of them (at most 2048 pairings at one wave per SIMD) takes ~3.8 ms,
// against the quad VM's ~270 k pairings/s (800: 3.70 vs 3.94 ms, 2048: 3.78
// vs 7.63; the quad VM steps up after 768 pairings) and the lane pairs'
// ~8.4 ms (4096: 6.45 vs 8.41, both kernels at two waves per SIMD above 2048);
// profiles/r06_lane_groups.txt
size_t pq_min() {
    static const size_t v = pa::env_count("PA_PQ_MIN", 768);
    return v;
}
size_t pq_max() {
    static const size_t v = pa::env_count("PA_PQ_MAX", 4096);
    return v;
}
bool use_pq(size_t n) {
    const int v = pairing_variant();
    return v == 5 || (v == 0 && n > pq_min() && n <= pq_max());
}
int coop_vm() { return pairing_variant() == 4 ? 1 : 0; }
// lanes per pairing of the generated kernels; ml_only: the reference-form Miller
// loop without a final exponentiation behind it (its own crossover, ml_one_max)
int gen_lanes(size_t n, bool ml_only = false) {
    const int v = pairing_variant();
    if (v == 1) return 2;
    if (v == 3) return 1;
    return n <= pair_max() || n > (ml_only ? ml_one_max() : one_max()) ? 2 : 1;
}
// multi-pairings of at most this many pairs multiply their Miller values inside
// the cooperative final exponentiation (sequential mul12 macros); larger ones
// use the log-depth product tree first
constexpr size_t kCoopProductMax = 16;
// largest wNAF window the explicit-window fixed-base entries accept (the
// reference's heuristics pick 2..16 for G1, 2..15 for G2; its wnaf_form keeps
// a digit mod 2^(w+1) in a u64)
constexpr int kMaxWnafWindow = 62;

// Batches just above pair_max(): n <= pair_max() + tail_max() pairings run as
// the first pair_max() on lane pairs (one wave per SIMD, ~9.3 ms) and the tail
// on the cooperative kernels (a workgroup per pairing, latency-bound), the tail
// on a second stream forked from and joined back into the caller's, so its
// workgroups run beside the lane-pair waves -- instead of a second lane-pair
// wave on a few SIMDs (~15.7 ms whatever the tail).  Values are the same
// whichever kernels run a pairing (final exponentiation output; the
// pairing-only Miller values differ from the cooperative Miller loop's by Fq2
// factors, as pa_pairing_miller_loop_batch_device documents).  Not under
// stream capture (the side stream would join the graph); PA_TAIL_MAX=0 turns
// it off.
size_t tail_max() {
    // profiles/r06_tail/: the forked tail beats a second lane-pair wave (15.6-15.7
    // ms) up to ~2000 tail pairs: 32769 10.8 ms, 33024 10.6, 33792 13.1 (the
    // cooperative kernels), 34048 12.9, 34816 13.0 (the lane groups); 35840
    // 15.7 -- no better than no split
    static const size_t v = pa::env_count("PA_TAIL_MAX", 2048);
    return v;
}
// the tail's kernels: the cooperative ones up to 832 tail pairings, the lane
// groups above (33536: 12.3 vs 13.1 ms; 33664: 13.2 vs 12.9; 34816: 17.1 vs
// 13.0; profiles/r06_tail/); PA_TAIL_KIND=coop / pq forces one (A/B)
bool tail_pq(size_t tail) {
    static const int v = [] {
        const char* e = getenv("PA_TAIL_KIND");
        return !e ? 0 : strcmp(e, "pq") == 0 ? 1 : strcmp(e, "coop") == 0 ? 2 : 0;
    }();
    return v == 1 || (v == 0 && tail > 832);
}
struct TailFork {
    int dev = -1;
    hipStream_t side = nullptr;
    hipEvent_t fork = nullptr, join = nullptr;
};
// a process-wide pool: a call takes a fork, enqueues the fork wait, the tail and
// the join wait, and gives it back (a wait holds the event's state at the time it
// is enqueued, so the next call may record the events again)
std::mutex g_tail_mu;
std::vector<TailFork*> g_tail_free;
size_t split_head(size_t n, hipStream_t s) {
    if (pairing_variant() != 0 || n <= pair_max() || n - pair_max() > tail_max()) return 0;
    hipStreamCaptureStatus st = hipStreamCaptureStatusNone;
    if (hipStreamIsCapturing(s, &st) != hipSuccess || st != hipStreamCaptureStatusNone) return 0;
    return pair_max();
}
// a fork whose side stream is ordered after everything enqueued on s
hipError_t tail_begin(hipStream_t s, TailFork** out) {
    *out = nullptr;
    int dev = 0;
    hipError_t e = hipGetDevice(&dev);
    if (e != hipSuccess) return e;
    TailFork* f = nullptr;
    {
        std::lock_guard<std::mutex> lock(g_tail_mu);
        for (size_t i = 0; i < g_tail_free.size(); i++)
            if (g_tail_free[i]->dev == dev) {
                f = g_tail_free[i];
                g_tail_free.erase(g_tail_free.begin() + i);
                break;
            }
    }
    if (!f) {
        f = new TailFork;
        f->dev = dev;
        if ((e = hipStreamCreateWithFlags(&f->side, hipStreamNonBlocking)) != hipSuccess ||
            (e = hipEventCreateWithFlags(&f->fork, hipEventDisableTiming)) != hipSuccess ||
            (e = hipEventCreateWithFlags(&f->join, hipEventDisableTiming)) != hipSuccess) {
            if (f->join) (void)hipEventDestroy(f->join);
            if (f->fork) (void)hipEventDestroy(f->fork);
            if (f->side) (void)hipStreamDestroy(f->side);
            delete f;
            return e;
        }
    }
    if ((e = hipEventRecord(f->fork, s)) == hipSuccess) e = hipStreamWaitEvent(f->side, f->fork, 0);
    if (e != hipSuccess) {
        std::lock_guard<std::mutex> lock(g_tail_mu);
        g_tail_free.push_back(f);
        return e;
    }
    *out = f;
    return hipSuccess;
}
// s waits for the tail; the fork goes back to the pool
hipError_t tail_end(hipStream_t s, TailFork* f) {
    if (!f) return hipSuccess;
    hipError_t e = hipEventRecord(f->join, f->side);
    if (e == hipSuccess) e = hipStreamWaitEvent(s, f->join, 0);
    std::lock_guard<std::mutex> lock(g_tail_mu);
    g_tail_free.push_back(f);
    return e;
}
constexpr size_t kG1Words = sizeof(pa_g1_affine) / 8, kG2Words = sizeof(pa_g2_affine) / 8,
                 kF12Words = sizeof(pa_fq12) / 8;

hipError_t ml_launch(const uint64_t* p, const uint64_t* q, uint64_t* out, size_t n, hipStream_t s) {
    if (use_pq(n)) return pa::launch_pq_miller_loop(p, q, out, n, s);
    if (use_coop(n)) return pa::launch_coop_miller_loop(p, q, out, n, s, coop_vm());
    return pa::launch_miller_loop_gen(gen_lanes(n, true), p, q, out, n, s);
}
// The Miller loop in front of a final exponentiation (pa_pairing_batch[_device],
// pa_multi_pairing_device): on lane pairs the pairing-only kernel, whose Miller
// values differ from the reference's by Fq2 factors that the final
// exponentiation removes ((q^12 - 1) / r is a multiple of q^2 - 1) -- 3.5 %
// fewer instructions (tools/pgen/kernels.py doubling_step_h); round 6: one lane
// per pairing too (pa_gen_miller_loop1p).  The Miller-loop entries themselves
// keep ml_launch.
//
// Domain: the Fq2-factor argument needs Q on E' (doubling_step_h's tangent uses
// b'); P is free, and so is the order of a curve point Q.  The reference's own
// steps never use b, so for a Q off E' the two loops walk different curves and
// no final exponentiation reconciles them.  pairing_gen_launch therefore puts
// k_pairing_ml_fixup behind every pairing-only launch: it tests each Q against
// E' exactly and recomputes the off-curve pairs in reference form, so every
// e(P, Q) entry returns the reference's value for any field elements at every
// batch size.
hipError_t pairing_gen_launch(int lanes, const uint64_t* p, const uint64_t* q, uint64_t* out, size_t n,
                              hipStream_t s) {
    hipError_t e = pa::launch_miller_loop_pairing_gen(lanes, p, q, out, n, s);
    if (e == hipSuccess) e = pa::launch_pairing_ml_fixup(p, q, out, n, s);
    return e;
}
hipError_t pairing_ml_launch(const uint64_t* p, const uint64_t* q, uint64_t* out, size_t n, hipStream_t s) {
    if (use_coop(n) || use_pq(n)) return ml_launch(p, q, out, n, s);
    if (const size_t h = split_head(n, s)) {
        TailFork* f = nullptr;
        hipError_t e = pairing_gen_launch(2, p, q, out, h, s);
        if (e == hipSuccess) e = tail_begin(s, &f);
        if (e == hipSuccess)
            e = tail_pq(n - h) ? pa::launch_pq_miller_loop(p + h * kG1Words, q + h * kG2Words, out + h * kF12Words, n - h,
                                                      f->side)
                          : pa::launch_coop_miller_loop(p + h * kG1Words, q + h * kG2Words, out + h * kF12Words,
                                                        n - h, f->side, coop_vm());
        const hipError_t j = tail_end(s, f);
        return e != hipSuccess ? e : j;
    }
    return pairing_gen_launch(gen_lanes(n), p, q, out, n, s);
}
hipError_t fe_launch(const uint64_t* in, uint64_t* out, uint8_t* ok, size_t n, hipStream_t s) {
    if (use_pq(n)) return pa::launch_pq_final_exp(in, out, ok, n, s);
    if (use_coop(n)) return pa::launch_coop_final_exp(in, out, ok, n, s, coop_vm());
    if (const size_t h = split_head(n, s)) {
        TailFork* f = nullptr;
        hipError_t e = pa::launch_final_exp_gen(2, in, out, ok, h, s);
        if (e == hipSuccess) e = tail_begin(s, &f);
        if (e == hipSuccess)
            e = tail_pq(n - h) ? pa::launch_pq_final_exp(in + h * kF12Words, out + h * kF12Words, ok ? ok + h : nullptr,
                                                    n - h, f->side)
                          : pa::launch_coop_final_exp(in + h * kF12Words, out + h * kF12Words, ok ? ok + h : nullptr,
                                                      n - h, f->side, coop_vm());
        const hipError_t j = tail_end(s, f);
        return e != hipSuccess ? e : j;
    }
    return pa::launch_final_exp_gen(gen_lanes(n), in, out, ok, n, s);
}

int fail(int code, const char* what, hipError_t e = hipSuccess) {
    char buf[1024];
    const char* detail = pa::gen_error_detail();
    if (e != hipSuccess && detail[0])
        snprintf(buf, sizeof buf, "%s: %s (%d) [%s]", what, hipGetErrorString(e), (int)e, detail);
    else if (e != hipSuccess)
        snprintf(buf, sizeof buf, "%s: %s (%d)", what, hipGetErrorString(e), (int)e);
    else
        snprintf(buf, sizeof buf, "%s", what);
    g_last_error = buf;
    return code;
}

int hip_code(hipError_t e) {
    if (e == hipErrorOutOfMemory || e == hipErrorMemoryAllocation) return PA_ERR_OUT_OF_MEMORY;
    if (e == hipErrorNoDevice || e == hipErrorInvalidDevice) return PA_ERR_NO_DEVICE;
    return PA_ERR_HIP;
}

#define PA_TRY(expr, what)                                          \
    do {                                                            \
        hipError_t _e = (expr);                                     \
        if (_e != hipSuccess) return fail(hip_code(_e), what, _e);  \
    } while (0)

// ---- per-thread device context of the host-pointer entry points ----
// Every host-pointer call runs on its calling thread's own context for the
// current device: a non-blocking compute stream, a copy stream for the
// pipelined pairing path, grow-only device scratch slots and grow-only pinned
// staging buffers.  So a call never hipMallocs in steady state, waits only
// for its own stream (no device-wide synchronize), and calls from different
// host threads run concurrently (the reference traits are Send + Sync,
// lib.rs:120-121).  A thread's contexts go back to a process-wide pool when
// the thread exits (no HIP call at that point) and are reused by new threads.
struct HostCtx {
    int dev = -1;
    hipStream_t compute = nullptr, copy = nullptr, copy_out = nullptr;
    std::vector<std::pair<void*, size_t>> slots;     // device scratch, used as a stack by DevBuf
    size_t depth = 0;
    std::pair<void*, size_t> pinned[4] = {};          // pinned host staging (pipelined pairing)
    std::pair<void*, size_t> pipe[8] = {};            // device buffers of the pipelined pairing
    hipEvent_t ev[16] = {};
    size_t full_batch = 0;                            // pairings that fill the device once (one wave per SIMD)
};

struct CtxPool {
    std::mutex mu;
    std::vector<HostCtx*> free_ctx;
};
CtxPool& ctx_pool() {
    static CtxPool* p = new CtxPool;   // never destroyed: thread exits may return contexts late
    return *p;
}

struct ThreadCtxs {
    HostCtx* by_dev[64] = {};
    ~ThreadCtxs() {
        CtxPool& pool = ctx_pool();
        std::lock_guard<std::mutex> g(pool.mu);
        for (HostCtx* c : by_dev)
            if (c) {
                c->depth = 0;
                pool.free_ctx.push_back(c);
            }
    }
};
thread_local ThreadCtxs t_ctxs;

hipError_t thread_ctx(HostCtx** out) {
    int dev = 0;
    hipError_t e = hipGetDevice(&dev);
    if (e != hipSuccess) return e;
    if (dev < 0 || dev >= 64) return hipErrorInvalidDevice;
    if (HostCtx* c = t_ctxs.by_dev[dev]) {
        *out = c;
        return hipSuccess;
    }
    {
        CtxPool& pool = ctx_pool();
        std::lock_guard<std::mutex> g(pool.mu);
        for (size_t k = 0; k < pool.free_ctx.size(); k++)
            if (pool.free_ctx[k]->dev == dev) {
                *out = t_ctxs.by_dev[dev] = pool.free_ctx[k];
                pool.free_ctx.erase(pool.free_ctx.begin() + k);
                return hipSuccess;
            }
    }
    HostCtx* c = new HostCtx;
    c->dev = dev;
    if ((e = hipStreamCreateWithFlags(&c->compute, hipStreamNonBlocking)) != hipSuccess ||
        (e = hipStreamCreateWithFlags(&c->copy, hipStreamNonBlocking)) != hipSuccess ||
        (e = hipStreamCreateWithFlags(&c->copy_out, hipStreamNonBlocking)) != hipSuccess) {
        delete c;   // (a stream created before the failure is leaked: rare, bounded)
        return e;
    }
    for (auto& ev : c->ev)
        if ((e = hipEventCreateWithFlags(&ev, hipEventDisableTiming)) != hipSuccess) return e;
    *out = t_ctxs.by_dev[dev] = c;
    return hipSuccess;
}

// grow-only buffer: reuse `b` if large enough (its last use has completed --
// every call synchronizes its streams before returning)
hipError_t grow(std::pair<void*, size_t>& b, size_t bytes, bool pinned) {
    if (b.second >= bytes && b.first) return hipSuccess;
    hipError_t e;
    if (b.first && (e = pinned ? hipHostFree(b.first) : hipFree(b.first)) != hipSuccess) return e;
    b = {nullptr, 0};
    bytes = bytes < 4096 ? 4096 : bytes + bytes / 8;   // headroom: fewer regrowths for slowly rising sizes
    if ((e = pinned ? hipHostMalloc(&b.first, bytes, hipHostMallocDefault) : hipMalloc(&b.first, bytes)) !=
        hipSuccess) {
        b.first = nullptr;
        return e;
    }
    b.second = bytes;
    return hipSuccess;
}

// One stream per device for the pipelined pairing kernels of every host
// thread: two batches' kernels running at once on one GPU share its SIMDs
// worse than back to back (each wave holds a whole SIMD), so the kernels of
// concurrent callers queue on this stream while their copies overlap them.
hipError_t pairing_stream(int dev, hipStream_t* out) {
    static std::mutex mu;
    static hipStream_t streams[64] = {};
    std::lock_guard<std::mutex> g(mu);
    if (!streams[dev]) {
        hipError_t e = hipStreamCreateWithFlags(&streams[dev], hipStreamNonBlocking);
        if (e != hipSuccess) return e;
    }
    *out = streams[dev];
    return hipSuccess;
}

// The calling thread's compute stream on the current device (host entries).
hipStream_t call_stream() {
    HostCtx* c = nullptr;
    return thread_ctx(&c) == hipSuccess ? c->compute : nullptr;
}
hipError_t call_sync() {
    HostCtx* c = nullptr;
    hipError_t e = thread_ctx(&c);
    return e != hipSuccess ? e : hipStreamSynchronize(c->compute);
}

// A device scratch buffer for a host-pointer entry point: the next slot of
// the thread's context, released (not freed) when it goes out of scope.
struct DevBuf {
    void* p = nullptr;
    HostCtx* ctx = nullptr;
    hipError_t alloc(size_t bytes) {
        hipError_t e = thread_ctx(&ctx);
        if (e != hipSuccess) return e;
        if (ctx->slots.size() <= ctx->depth) ctx->slots.resize(ctx->depth + 1, {nullptr, 0});
        if ((e = grow(ctx->slots[ctx->depth], bytes ? bytes : 1, false)) != hipSuccess) {
            ctx = nullptr;
            return e;
        }
        p = ctx->slots[ctx->depth++].first;
        return hipSuccess;
    }
    ~DevBuf() {
        if (ctx) ctx->depth--;
    }
    template <class T>
    T* as() const { return static_cast<T*>(p); }
};

int upload(DevBuf& d, const void* host, size_t bytes) {
    PA_TRY(d.alloc(bytes), "device scratch");
    if (bytes) PA_TRY(hipMemcpyAsync(d.p, host, bytes, hipMemcpyHostToDevice, d.ctx->compute), "H2D copy");
    return PA_OK;
}
int download(void* host, const DevBuf& d, size_t bytes) {
    if (bytes) {
        PA_TRY(hipMemcpyAsync(host, d.p, bytes, hipMemcpyDeviceToHost, d.ctx->compute), "D2H copy");
        PA_TRY(hipStreamSynchronize(d.ctx->compute), "D2H copy");
    }
    return PA_OK;
}

bool op_needs_b(int op) {
    return op == pa::OP_FQ_MUL || op == pa::OP_FQ_ADD || op == pa::OP_FQ_SUB || op == pa::OP_FQ2_MUL ||
           op == pa::OP_FQ6_MUL || op == pa::OP_FQ12_MUL;
}

// Elementwise field op on host buffers: out = op(a, b).
int host_field_op(int op, const void* a, const void* b, void* out, uint8_t* ok, size_t n, size_t in_bytes,
                  size_t out_bytes, int param) {
    if (n == 0) return PA_OK;
    if (!a || !out || (op_needs_b(op) && !b)) return fail(PA_ERR_INVALID_ARGUMENT, "null pointer");
    DevBuf da, db, dout, dok;
    int rc;
    if ((rc = upload(da, a, in_bytes * n))) return rc;
    if (b && (rc = upload(db, b, in_bytes * n))) return rc;
    PA_TRY(dout.alloc(out_bytes * n), "device scratch");
    if (ok) PA_TRY(dok.alloc(n), "device scratch");
    PA_TRY(pa::launch_field_op(op, da.as<uint64_t>(), db.as<uint64_t>(), dout.as<uint64_t>(), dok.as<uint8_t>(), n,
                               param, call_stream()),
           "kernel launch");
    PA_TRY(call_sync(), "kernel execution");
    if ((rc = download(out, dout, out_bytes * n))) return rc;
    if (ok && (rc = download(ok, dok, n))) return rc;
    return PA_OK;
}

}  // namespace

extern "C" {

const char* pa_version(void) { return "pairing_amd 0.1.0 (gfx950)"; }
const char* pa_last_error(void) { return g_last_error.c_str(); }

int pa_device_count(int* count) {
    if (!count) return fail(PA_ERR_INVALID_ARGUMENT, "null pointer");
    hipError_t e = hipGetDeviceCount(count);
    if (e != hipSuccess) {
        *count = 0;
        return fail(PA_ERR_NO_DEVICE, "hipGetDeviceCount", e);
    }
    return PA_OK;
}
int pa_set_device(int device) {
    PA_TRY(hipSetDevice(device), "hipSetDevice");
    return PA_OK;
}
int pa_set_pairing_kernel(int variant) {
    if (variant < 0 || variant > 5) return fail(PA_ERR_INVALID_ARGUMENT, "kernel variant must be 0..5");
    g_pairing_variant.store(variant, std::memory_order_relaxed);
    return PA_OK;
}
int pa_set_decode_kernel(int variant) {
    if (variant < 0 || variant > 2) return fail(PA_ERR_INVALID_ARGUMENT, "decode kernel variant must be 0..2");
    pa::set_decode_variant(variant);
    return PA_OK;
}
int pa_synchronize(void) {
    PA_TRY(hipDeviceSynchronize(), "hipDeviceSynchronize");
    return PA_OK;
}

int pa_fq_mul_batch(const pa_fq* a, const pa_fq* b, pa_fq* out, size_t n) {
    return host_field_op(pa::OP_FQ_MUL, a, b, out, nullptr, n, 48, 48, 0);
}
int pa_fq_square_batch(const pa_fq* a, pa_fq* out, size_t n) {
    return host_field_op(pa::OP_FQ_SQR, a, nullptr, out, nullptr, n, 48, 48, 0);
}
int pa_fq_add_batch(const pa_fq* a, const pa_fq* b, pa_fq* out, size_t n) {
    return host_field_op(pa::OP_FQ_ADD, a, b, out, nullptr, n, 48, 48, 0);
}
int pa_fq_sub_batch(const pa_fq* a, const pa_fq* b, pa_fq* out, size_t n) {
    return host_field_op(pa::OP_FQ_SUB, a, b, out, nullptr, n, 48, 48, 0);
}
int pa_fq_inverse_batch(const pa_fq* a, pa_fq* out, uint8_t* ok, size_t n) {
    if (n && !ok) return fail(PA_ERR_INVALID_ARGUMENT, "null ok");
    return host_field_op(pa::OP_FQ_INV, a, nullptr, out, ok, n, 48, 48, 0);
}
int pa_fq_from_repr_batch(const pa_fq_repr* repr, pa_fq* out, uint8_t* ok, size_t n) {
    if (n && !ok) return fail(PA_ERR_INVALID_ARGUMENT, "null ok");
    return host_field_op(pa::OP_FQ_FROM_REPR, repr, nullptr, out, ok, n, 48, 48, 0);
}
int pa_fq_into_repr_batch(const pa_fq* a, pa_fq_repr* out, size_t n) {
    return host_field_op(pa::OP_FQ_INTO_REPR, a, nullptr, out, nullptr, n, 48, 48, 0);
}
int pa_fq2_mul_batch(const pa_fq2* a, const pa_fq2* b, pa_fq2* out, size_t n) {
    return host_field_op(pa::OP_FQ2_MUL, a, b, out, nullptr, n, 96, 96, 0);
}
int pa_fq2_square_batch(const pa_fq2* a, pa_fq2* out, size_t n) {
    return host_field_op(pa::OP_FQ2_SQR, a, nullptr, out, nullptr, n, 96, 96, 0);
}
int pa_fq6_mul_batch(const pa_fq6* a, const pa_fq6* b, pa_fq6* out, size_t n) {
    return host_field_op(pa::OP_FQ6_MUL, a, b, out, nullptr, n, 288, 288, 0);
}
int pa_fq12_mul_batch(const pa_fq12* a, const pa_fq12* b, pa_fq12* out, size_t n) {
    return host_field_op(pa::OP_FQ12_MUL, a, b, out, nullptr, n, 576, 576, 0);
}
int pa_fq12_square_batch(const pa_fq12* a, pa_fq12* out, size_t n) {
    return host_field_op(pa::OP_FQ12_SQR, a, nullptr, out, nullptr, n, 576, 576, 0);
}
int pa_fq12_inverse_batch(const pa_fq12* a, pa_fq12* out, uint8_t* ok, size_t n) {
    if (n && !ok) return fail(PA_ERR_INVALID_ARGUMENT, "null ok");
    return host_field_op(pa::OP_FQ12_INV, a, nullptr, out, ok, n, 576, 576, 0);
}
int pa_fq12_frobenius_map_batch(const pa_fq12* a, pa_fq12* out, size_t n, size_t power) {
    return host_field_op(pa::OP_FQ12_FROB, a, nullptr, out, nullptr, n, 576, 576, (int)(power % 12));
}
int pa_fq2_inverse_batch(const pa_fq2* a, pa_fq2* out, uint8_t* ok, size_t n) {
    if (n && !ok) return fail(PA_ERR_INVALID_ARGUMENT, "null ok");
    return host_field_op(pa::OP_FQ2_INV, a, nullptr, out, ok, n, 96, 96, 0);
}
int pa_fq2_frobenius_map_batch(const pa_fq2* a, pa_fq2* out, size_t n, size_t power) {
    return host_field_op(pa::OP_FQ2_FROB, a, nullptr, out, nullptr, n, 96, 96, (int)(power % 2));
}
int pa_fq6_square_batch(const pa_fq6* a, pa_fq6* out, size_t n) {
    return host_field_op(pa::OP_FQ6_SQR, a, nullptr, out, nullptr, n, 288, 288, 0);
}
int pa_fq6_inverse_batch(const pa_fq6* a, pa_fq6* out, uint8_t* ok, size_t n) {
    if (n && !ok) return fail(PA_ERR_INVALID_ARGUMENT, "null ok");
    return host_field_op(pa::OP_FQ6_INV, a, nullptr, out, ok, n, 288, 288, 0);
}
int pa_fq6_frobenius_map_batch(const pa_fq6* a, pa_fq6* out, size_t n, size_t power) {
    return host_field_op(pa::OP_FQ6_FROB, a, nullptr, out, nullptr, n, 288, 288, (int)(power % 6));
}
namespace {
int host_field_pow(int op, const void* a, const uint64_t* exp, size_t exp_words, void* out, size_t n,
                   size_t bytes) {
    if (n == 0) return PA_OK;
    if (!a || !out || (exp_words && !exp)) return fail(PA_ERR_INVALID_ARGUMENT, "null pointer");
    if (exp_words > (1u << 20)) return fail(PA_ERR_INVALID_ARGUMENT, "exponent too long");
    DevBuf da, de, dout;
    int rc;
    if ((rc = upload(da, a, bytes * n)) || (rc = upload(de, exp, 8 * exp_words))) return rc;
    PA_TRY(dout.alloc(bytes * n), "device scratch");
    PA_TRY(pa::launch_field_op(op, da.as<uint64_t>(), de.as<uint64_t>(), dout.as<uint64_t>(), nullptr, n,
                               (int)exp_words, call_stream()),
           "kernel launch");
    PA_TRY(call_sync(), "kernel execution");
    return download(out, dout, bytes * n);
}
}  // namespace
int pa_fq_pow_batch(const pa_fq* a, const uint64_t* exp, size_t exp_words, pa_fq* out, size_t n) {
    return host_field_pow(pa::OP_FQ_POW, a, exp, exp_words, out, n, 48);
}
int pa_fq12_pow_batch(const pa_fq12* a, const uint64_t* exp, size_t exp_words, pa_fq12* out, size_t n) {
    return host_field_pow(pa::OP_FQ12_POW, a, exp, exp_words, out, n, 576);
}
// not in the public header: cyclotomic squaring, exposed for the parity tests
int pa_fq12_cyclotomic_square_batch(const pa_fq12* a, pa_fq12* out, size_t n) {
    return host_field_op(pa::OP_FQ12_CYC_SQR, a, nullptr, out, nullptr, n, 576, 576, 0);
}

int pa_fq12_mul_by_014_batch(const pa_fq12* a, const pa_fq2* c0, const pa_fq2* c1, const pa_fq2* c4,
                             pa_fq12* out, size_t n) {
    if (n == 0) return PA_OK;
    if (!a || !c0 || !c1 || !c4 || !out) return fail(PA_ERR_INVALID_ARGUMENT, "null pointer");
    DevBuf da, d0, d1, d4, dout;
    int rc;
    if ((rc = upload(da, a, 576 * n)) || (rc = upload(d0, c0, 96 * n)) || (rc = upload(d1, c1, 96 * n)) ||
        (rc = upload(d4, c4, 96 * n)))
        return rc;
    PA_TRY(dout.alloc(576 * n), "device scratch");
    PA_TRY(pa::launch_fq12_mul_by_014(da.as<uint64_t>(), d0.as<uint64_t>(), d1.as<uint64_t>(), d4.as<uint64_t>(),
                                      dout.as<uint64_t>(), n, call_stream()),
           "kernel launch");
    PA_TRY(call_sync(), "kernel execution");
    return download(out, dout, 576 * n);
}

int pa_g2_prepare_batch(const pa_g2_affine* q, pa_g2_prepared* out, size_t n) {
    if (n == 0) return PA_OK;
    if (!q || !out) return fail(PA_ERR_INVALID_ARGUMENT, "null pointer");
    DevBuf dq, dout;
    int rc;
    if ((rc = upload(dq, q, sizeof(pa_g2_affine) * n))) return rc;
    PA_TRY(dout.alloc(sizeof(pa_g2_prepared) * n), "device scratch");
    PA_TRY(pa::launch_g2_prepare(dq.as<uint64_t>(), dout.as<uint64_t>(), n, call_stream()), "kernel launch");
    PA_TRY(call_sync(), "kernel execution");
    return download(out, dout, sizeof(pa_g2_prepared) * n);
}

int pa_miller_loop_batch(const pa_g1_affine* p, const pa_g2_prepared* q, pa_fq12* out, size_t n) {
    if (n == 0) return PA_OK;
    if (!p || !q || !out) return fail(PA_ERR_INVALID_ARGUMENT, "null pointer");
    DevBuf dp, dq, dout;
    int rc;
    if ((rc = upload(dp, p, sizeof(pa_g1_affine) * n)) || (rc = upload(dq, q, sizeof(pa_g2_prepared) * n)))
        return rc;
    PA_TRY(dout.alloc(576 * n), "device scratch");
    PA_TRY(pa::launch_miller_loop_prepared_gen(dp.as<uint64_t>(), dq.as<uint64_t>(), dout.as<uint64_t>(), n,
                                               call_stream()),
           "kernel launch");
    PA_TRY(call_sync(), "kernel execution");
    return download(out, dout, 576 * n);
}

int pa_miller_loop_shared_prepared(const pa_g1_affine* p, size_t n, const pa_g2_prepared* q, pa_fq12* out) {
    if (n == 0) return PA_OK;
    if (!p || !q || !out) return fail(PA_ERR_INVALID_ARGUMENT, "null pointer");
    DevBuf dp, dq, dout;
    int rc;
    if ((rc = upload(dp, p, sizeof(pa_g1_affine) * n)) || (rc = upload(dq, q, sizeof(pa_g2_prepared))))
        return rc;
    PA_TRY(dout.alloc(576 * n), "device scratch");
    PA_TRY(pa::launch_miller_loop_shared_gen(dp.as<uint64_t>(), dq.as<uint64_t>(), dout.as<uint64_t>(), n,
                                             call_stream()),
           "kernel launch");
    PA_TRY(call_sync(), "kernel execution");
    return download(out, dout, 576 * n);
}

int pa_multi_miller_loop(const pa_g1_affine* p, const pa_g2_prepared* q, size_t n, pa_fq12* out) {
    if (!out) return fail(PA_ERR_INVALID_ARGUMENT, "null pointer");
    if (n == 0) {
        // empty product: Fq12::one() (mod.rs:71 with no pairs), conjugated = one
        memset(out, 0, sizeof(pa_fq12));
        const uint64_t r[6] = {0x760900000002fffdULL, 0xebf4000bc40c0002ULL, 0x5f48985753c758baULL,
                               0x77ce585370525745ULL, 0x5c071a97a256ec6dULL, 0x15f65ec3fa80e493ULL};
        memcpy(out->c0.c0.c0.l, r, sizeof r);
        return PA_OK;
    }
    if (!p || !q) return fail(PA_ERR_INVALID_ARGUMENT, "null pointer");
    DevBuf dp, dq, dwork, dout;
    int rc;
    if ((rc = upload(dp, p, sizeof(pa_g1_affine) * n)) || (rc = upload(dq, q, sizeof(pa_g2_prepared) * n)))
        return rc;
    PA_TRY(dwork.alloc(576 * n), "device scratch");
    PA_TRY(dout.alloc(576), "device scratch");
    PA_TRY(pa::launch_miller_loop_prepared_gen(dp.as<uint64_t>(), dq.as<uint64_t>(), dwork.as<uint64_t>(), n,
                                               call_stream()),
           "kernel launch");
    PA_TRY(pa::launch_fq12_product(dwork.as<uint64_t>(), n, dout.as<uint64_t>(), call_stream()), "kernel launch");
    PA_TRY(call_sync(), "kernel execution");
    return download(out, dout, 576);
}

int pa_final_exponentiation_batch(const pa_fq12* in, pa_fq12* out, uint8_t* ok, size_t n) {
    if (n == 0) return PA_OK;
    if (!in || !out || !ok) return fail(PA_ERR_INVALID_ARGUMENT, "null pointer");
    DevBuf din, dout, dok;
    int rc;
    if ((rc = upload(din, in, 576 * n))) return rc;
    PA_TRY(dout.alloc(576 * n), "device scratch");
    PA_TRY(dok.alloc(n), "device scratch");
    PA_TRY(fe_launch(din.as<uint64_t>(), dout.as<uint64_t>(), dok.as<uint8_t>(), n, call_stream()),
           "kernel launch");
    PA_TRY(call_sync(), "kernel execution");
    if ((rc = download(out, dout, 576 * n))) return rc;
    return download(ok, dok, n);
}

}  // extern "C"

namespace {

// Host copy into / out of pinned staging, split over up to 8 threads for
// large buffers (a single thread's memcpy would be slower than the DMA it
// feeds).
void pcopy(void* dst, const void* src, size_t bytes) {
    constexpr size_t kPiece = 2u << 20;
    unsigned t = std::thread::hardware_concurrency();
    t = t < 1 ? 1 : (t > 8 ? 8 : t);
    if (bytes / kPiece < t) t = (unsigned)(bytes / kPiece);
    if (t <= 1) {
        memcpy(dst, src, bytes);
        return;
    }
    const size_t per = (bytes + t - 1) / t;
    std::vector<std::thread> th;
    for (unsigned k = 1; k < t; k++) {
        const size_t lo = per * k, len = lo >= bytes ? 0 : (bytes - lo < per ? bytes - lo : per);
        if (len) th.emplace_back([=] { memcpy((char*)dst + lo, (const char*)src + lo, len); });
    }
    memcpy(dst, src, per < bytes ? per : bytes);
    for (auto& x : th) x.join();
}

}  // namespace

extern "C" {

// Engine::pairing over host buffers, pipelined: the batch is cut into chunks
// of one device-filling wave count (one pairing per lane, one wave per SIMD:
// multiProcessorCount x 4 x 64 = 65 536 on MI355X); chunk k's inputs are
// staged into pinned memory and copied on the copy stream while chunk k-1
// computes on the compute stream, and chunk k-1's results travel back while
// chunk k computes.  Two pinned / device buffer sets alternate.
int pa_pairing_batch(const pa_g1_affine* p, const pa_g2_affine* q, pa_fq12* out, size_t n) {
    if (n == 0) return PA_OK;
    if (!p || !q || !out) return fail(PA_ERR_INVALID_ARGUMENT, "null pointer");
    HostCtx* c = nullptr;
    PA_TRY(thread_ctx(&c), "device context");
    hipStream_t ks = nullptr;   // kernels: the device's shared pairing stream
    PA_TRY(pairing_stream(c->dev, &ks), "pairing stream");
    if (!c->full_batch) {
        int cus = 0;
        PA_TRY(hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, c->dev), "device attribute");
        c->full_batch = (size_t)(cus > 0 ? cus : 1) * 4 * 64;
    }
    size_t chunk = c->full_batch;
    if (const char* e = getenv("PA_PIPELINE_CHUNK")) {   // tests: exercise the pipeline at small n
        const long v = strtol(e, nullptr, 10);
        if (v > 0) chunk = (size_t)v;
    }
    const size_t nchunks = (n + chunk - 1) / chunk;
    const size_t cap = n < chunk ? n : chunk;
    constexpr size_t P1 = sizeof(pa_g1_affine), P2 = sizeof(pa_g2_affine), F12 = sizeof(pa_fq12);
    const int bufs = nchunks > 1 ? 2 : 1;
    for (int k = 0; k < bufs; k++) {
        PA_TRY(grow(c->pinned[2 * k], cap * (P1 + P2), true), "pinned staging");
        PA_TRY(grow(c->pinned[2 * k + 1], cap * F12, true), "pinned staging");
        PA_TRY(grow(c->pipe[4 * k], cap * (P1 + P2), false), "device scratch");   // p | q
        PA_TRY(grow(c->pipe[4 * k + 1], cap * F12, false), "device scratch");     // Miller values
        PA_TRY(grow(c->pipe[4 * k + 2], cap * F12, false), "device scratch");     // e(p, q)
    }
    // PA_PIPELINE_TRACE=1: per-phase host timestamps on stderr (measurement only)
    static const bool trace = getenv("PA_PIPELINE_TRACE") && getenv("PA_PIPELINE_TRACE")[0] == '1';
    const auto t0 = std::chrono::steady_clock::now();
    auto stamp = [&](const char* what, size_t ci) {
        if (trace)
            fprintf(stderr, "[pipeline] chunk %zu %-10s %8.3f ms\n", ci, what,
                    std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count());
    };
    // Within a chunk the staging copies and the DMA run in kPieces pieces
    // (PA_PIPELINE_PIECES, 1..4, default 2), so the host copy of piece j
    // overlaps the DMA of piece j - 1 (in) / j + 1 (out): one caller at 2^16,
    // reused result buffer, 19.19 ms with 1 piece, 18.89 with 2, 18.84 with 4
    // (profiles/r03_host_boundary.txt).
    static const size_t kPieces = (size_t)pa::env_clamp("PA_PIPELINE_PIECES", 2, 1, 4);
    hipEvent_t* h2d = c->ev;        // [k]: chunk's inputs copied (pinned in[k] free again)
    hipEvent_t* done = c->ev + 2;   // [k]: chunk's kernels finished (device in[k], ml[k] free)
    hipEvent_t* d2h = c->ev + 4;    // [k * kPieces + j]: piece j of the chunk's results in pinned out[k]
    hipEvent_t* outk = c->ev + 12;  // [k]: every piece of the chunk's results copied (device out[k] free);
                                    // recorded after the piece loop, so an empty last piece cannot leave it stale
    auto piece = [&](size_t cnt, size_t j, size_t* lo) {
        const size_t per = (cnt + kPieces - 1) / kPieces;
        *lo = per * j < cnt ? per * j : cnt;
        return (per * (j + 1) < cnt ? per * (j + 1) : cnt) - *lo;
    };
    auto drain = [&](size_t ci) -> int {
        const int k = (int)(ci & 1);
        const size_t lo = ci * chunk, cnt = n - lo < chunk ? n - lo : chunk;
        for (size_t j = 0; j < kPieces; j++) {
            size_t a;
            const size_t m = piece(cnt, j, &a);
            if (!m) continue;
            PA_TRY(hipEventSynchronize(d2h[k * kPieces + j]), "D2H copy");
            pcopy(out + lo + a, (pa_fq12*)c->pinned[2 * k + 1].first + a, m * F12);
        }
        stamp("copied out", ci);
        return PA_OK;
    };
    for (size_t ci = 0; ci < nchunks; ci++) {
        const int k = (int)(ci & 1);
        const size_t lo = ci * chunk, cnt = n - lo < chunk ? n - lo : chunk;
        char* pin_p = (char*)c->pinned[2 * k].first;
        char* pin_q = pin_p + cnt * P1;
        char* dev_p = (char*)c->pipe[4 * k].first;
        char* dev_q = dev_p + cnt * P1;
        uint64_t* dev_ml = (uint64_t*)c->pipe[4 * k + 1].first;
        uint64_t* dev_out = (uint64_t*)c->pipe[4 * k + 2].first;
        if (ci >= 2) {
            PA_TRY(hipEventSynchronize(h2d[k]), "H2D copy");
            PA_TRY(hipStreamWaitEvent(c->copy, done[k], 0), "stream wait");
        }
        for (size_t j = 0; j < kPieces; j++) {
            size_t a;
            const size_t m = piece(cnt, j, &a);
            if (!m) continue;
            pcopy(pin_p + a * P1, p + lo + a, m * P1);
            pcopy(pin_q + a * P2, q + lo + a, m * P2);
            PA_TRY(hipMemcpyAsync(dev_p + a * P1, pin_p + a * P1, m * P1, hipMemcpyHostToDevice, c->copy), "H2D copy");
            PA_TRY(hipMemcpyAsync(dev_q + a * P2, pin_q + a * P2, m * P2, hipMemcpyHostToDevice, c->copy), "H2D copy");
        }
        PA_TRY(hipEventRecord(h2d[k], c->copy), "event");
        stamp("staged in", ci);
        PA_TRY(hipStreamWaitEvent(ks, h2d[k], 0), "stream wait");
        if (ci >= 2) PA_TRY(hipStreamWaitEvent(ks, outk[k], 0), "stream wait");
        PA_TRY(pairing_ml_launch((const uint64_t*)dev_p, (const uint64_t*)dev_q, dev_ml, cnt, ks), "kernel launch");
        // Engine::pairing unwraps: a Miller-loop value is never zero, ok is not reported
        PA_TRY(fe_launch(dev_ml, dev_out, nullptr, cnt, ks), "kernel launch");
        PA_TRY(hipEventRecord(done[k], ks), "event");
        PA_TRY(hipStreamWaitEvent(c->copy_out, done[k], 0), "stream wait");
        for (size_t j = 0; j < kPieces; j++) {
            size_t a;
            const size_t m = piece(cnt, j, &a);
            if (!m) continue;
            PA_TRY(hipMemcpyAsync((pa_fq12*)c->pinned[2 * k + 1].first + a, (const pa_fq12*)dev_out + a, m * F12,
                                  hipMemcpyDeviceToHost, c->copy_out),
                   "D2H copy");
            PA_TRY(hipEventRecord(d2h[k * kPieces + j], c->copy_out), "event");
        }
        PA_TRY(hipEventRecord(outk[k], c->copy_out), "event");
        stamp("enqueued", ci);
        if (ci >= 1) {
            const int rc = drain(ci - 1);
            if (rc) return rc;
        }
    }
    const int rc = drain(nchunks - 1);
    if (rc) return rc;
    return PA_OK;   // the last chunk's D2H event has completed: so has everything before it
}

int pa_pairing_batch_multi_gpu(const pa_g1_affine* p, const pa_g2_affine* q, pa_fq12* out, size_t n, int ndev) {
    int count = 0;
    PA_TRY(hipGetDeviceCount(&count), "hipGetDeviceCount");
    // shard d runs on device d, or on the d-th entry of PA_DEVICE_MAP (a comma
    // list of device ordinals, e.g. "2,3,6,7" to use a subset of the node, or
    // "0,0" to run two shards' workers on one device)
    std::vector<int> dev_of;
    if (const char* m = getenv("PA_DEVICE_MAP")) {
        for (const char* c = m; *c;) {
            char* end = nullptr;
            const long v = strtol(c, &end, 10);
            if (end == c || v < 0 || v >= count) return fail(PA_ERR_INVALID_ARGUMENT, "bad PA_DEVICE_MAP");
            dev_of.push_back((int)v);
            c = *end == ',' ? end + 1 : end;
            if (*end && *end != ',') return fail(PA_ERR_INVALID_ARGUMENT, "bad PA_DEVICE_MAP");
        }
    } else {
        for (int d = 0; d < count; d++) dev_of.push_back(d);
    }
    if (ndev < 1 || ndev > (int)dev_of.size()) return fail(PA_ERR_INVALID_ARGUMENT, "ndev out of range");
    if (n == 0) return PA_OK;
    if (!p || !q || !out) return fail(PA_ERR_INVALID_ARGUMENT, "null pointer");
    // contiguous shards (SURVEY.md §8 e); each worker thread owns one device
    std::vector<int> rcs(ndev, PA_OK);
    std::vector<std::string> errs(ndev);
    std::vector<std::thread> workers;
    const size_t base = n / ndev, extra = n % ndev;
    size_t lo = 0;
    for (int d = 0; d < ndev; d++) {
        const size_t cnt = base + ((size_t)d < extra ? 1 : 0);
        const int dv = dev_of[d];
        workers.emplace_back([=, &rcs, &errs] {
            hipError_t e = hipSetDevice(dv);
            if (e != hipSuccess) {
                rcs[d] = fail(hip_code(e), "hipSetDevice", e);
            } else {
                rcs[d] = pa_pairing_batch(p + lo, q + lo, out + lo, cnt);
            }
            if (rcs[d] != PA_OK) errs[d] = g_last_error;
        });
        lo += cnt;
    }
    for (auto& t : workers) t.join();
    for (int d = 0; d < ndev; d++)
        if (rcs[d] != PA_OK) {
            g_last_error = "device " + std::to_string(d) + ": " + errs[d];
            return rcs[d];
        }
    return PA_OK;
}

int pa_multi_miller_loop_affine(const pa_g1_affine* p, const pa_g2_affine* q, size_t n, pa_fq12* out) {
    if (!out) return fail(PA_ERR_INVALID_ARGUMENT, "null pointer");
    if (n == 0) return pa_multi_miller_loop(nullptr, nullptr, 0, out);
    if (!p || !q) return fail(PA_ERR_INVALID_ARGUMENT, "null pointer");
    DevBuf dp, dq, dwork, dout;
    int rc;
    if ((rc = upload(dp, p, sizeof(pa_g1_affine) * n)) || (rc = upload(dq, q, sizeof(pa_g2_affine) * n)))
        return rc;
    PA_TRY(dwork.alloc(576 * n), "device scratch");
    PA_TRY(dout.alloc(576), "device scratch");
    // per-pair loops (infinity pairs give one, as mod.rs:50-54 skips them), then the product tree
    PA_TRY(ml_launch(dp.as<uint64_t>(), dq.as<uint64_t>(), dwork.as<uint64_t>(), n, call_stream()), "kernel launch");
    PA_TRY(pa::launch_fq12_product(dwork.as<uint64_t>(), n, dout.as<uint64_t>(), call_stream()), "kernel launch");
    PA_TRY(call_sync(), "kernel execution");
    return download(out, dout, 576);
}

int pa_multi_pairing_device(const pa_g1_affine* p, const pa_g2_affine* q, size_t n, pa_fq12* out, uint8_t* ok,
                            pa_fq12* work, void* stream) {
    if (!out || !ok || (n && (!p || !q || !work))) return fail(PA_ERR_INVALID_ARGUMENT, "null pointer");
    const hipStream_t s = (hipStream_t)stream;
    if (n == 0) {   // empty product: one, final_exponentiation(one) = one
        pa_fq12 one;
        memset(&one, 0, sizeof one);
        const uint64_t r[6] = {0x760900000002fffdULL, 0xebf4000bc40c0002ULL, 0x5f48985753c758baULL,
                               0x77ce585370525745ULL, 0x5c071a97a256ec6dULL, 0x15f65ec3fa80e493ULL};
        memcpy(one.c0.c0.c0.l, r, sizeof r);
        const uint8_t k = 1;
        PA_TRY(hipMemcpyAsync(out, &one, sizeof one, hipMemcpyHostToDevice, s), "H2D copy");
        PA_TRY(hipMemcpyAsync(ok, &k, 1, hipMemcpyHostToDevice, s), "H2D copy");
        PA_TRY(hipStreamSynchronize(s), "H2D copy");   // the host sources go out of scope
        return PA_OK;
    }
    PA_TRY(pairing_ml_launch((const uint64_t*)p, (const uint64_t*)q, (uint64_t*)work, n, s), "kernel launch");
    if (n <= kCoopProductMax && use_coop(1)) {
        // the product of a few Miller values inside the cooperative final
        // exponentiation (mul12 macros, ~6 us each) instead of the one-lane
        // product-tree kernel (~117 us per level)
        PA_TRY(pa::launch_coop_final_exp((const uint64_t*)work, (uint64_t*)out, ok, 1, s, coop_vm(), n),
               "kernel launch");
        return PA_OK;
    }
    PA_TRY(pa::launch_fq12_product((uint64_t*)work, n, (uint64_t*)work, s), "kernel launch");
    PA_TRY(fe_launch((const uint64_t*)work, (uint64_t*)out, ok, 1, s), "kernel launch");
    return PA_OK;
}

int pa_multi_pairing(const pa_g1_affine* p, const pa_g2_affine* q, size_t n, pa_fq12* out, uint8_t* ok) {
    if (!out || !ok) return fail(PA_ERR_INVALID_ARGUMENT, "null pointer");
    if (n && (!p || !q)) return fail(PA_ERR_INVALID_ARGUMENT, "null pointer");
    if (n == 0) {   // the empty product: final_exponentiation(one) = one
        pa_fq12 ml;
        int rc = pa_multi_miller_loop_affine(p, q, 0, &ml);
        if (rc) return rc;
        return pa_final_exponentiation_batch(&ml, out, ok, 1);
    }
    // one stream round trip: the pairs up, the device entry (Miller loops,
    // product, final exponentiation), the result down
    DevBuf dp, dq, dwork, dout, dok;
    int rc;
    if ((rc = upload(dp, p, sizeof(pa_g1_affine) * n)) || (rc = upload(dq, q, sizeof(pa_g2_affine) * n)))
        return rc;
    PA_TRY(dwork.alloc(576 * n), "device scratch");
    PA_TRY(dout.alloc(576), "device scratch");
    PA_TRY(dok.alloc(1), "device scratch");
    if ((rc = pa_multi_pairing_device(dp.as<pa_g1_affine>(), dq.as<pa_g2_affine>(), n, dout.as<pa_fq12>(),
                                      dok.as<uint8_t>(), dwork.as<pa_fq12>(), call_stream())))
        return rc;
    if ((rc = download(out, dout, 576))) return rc;
    return download(ok, dok, 1);
}

// ---- batched multi-pairing: m independent products in one call ----
// Workspace of the device entry: the n per-pair Miller values, the m products
// (contiguous, what the final exponentiation reads) and the m + 1 staged offsets.
namespace {
struct MpbLayout {
    size_t miller, prod, offsets, bytes;
};
MpbLayout mpb_layout(size_t n, size_t m) {
    MpbLayout l;
    l.miller = 0;
    l.prod = sizeof(pa_fq12) * n;
    l.offsets = l.prod + sizeof(pa_fq12) * m;
    l.bytes = l.offsets + sizeof(uint64_t) * (m + 1);
    return l;
}
// CSR check of host offsets; the longest segment through *max_len
const char* mpb_check_offsets(const uint64_t* offsets, size_t m, size_t* max_len) {
    if (offsets[0] != 0) return "multi_pairing_batch: offsets[0] must be 0";
    size_t longest = 0;
    for (size_t j = 0; j < m; j++) {
        if (offsets[j + 1] < offsets[j]) return "multi_pairing_batch: offsets must be non-decreasing";
        const uint64_t len = offsets[j + 1] - offsets[j];
        if (len > longest) longest = (size_t)len;
    }
    if (offsets[m] > SIZE_MAX / sizeof(pa_g2_affine)) return "multi_pairing_batch: too many pairs";
    *max_len = longest;
    return nullptr;
}
}  // namespace

size_t pa_multi_pairing_batch_workspace_bytes(size_t n_pairs, size_t m) { return mpb_layout(n_pairs, m).bytes; }

int pa_multi_pairing_batch_device(const pa_g1_affine* p, const pa_g2_affine* q, const uint64_t* host_offsets, size_t m,
                                  pa_fq12* out, uint8_t* ok, uint8_t* is_one, void* workspace, void* stream) {
    if (m == 0) return PA_OK;
    if (!host_offsets || !out || !ok || !workspace) return fail(PA_ERR_INVALID_ARGUMENT, "null pointer");
    size_t max_len = 0;
    if (const char* bad = mpb_check_offsets(host_offsets, m, &max_len)) return fail(PA_ERR_INVALID_ARGUMENT, bad);
    const size_t n = (size_t)host_offsets[m];
    if (n && (!p || !q)) return fail(PA_ERR_INVALID_ARGUMENT, "null pointer");
    const hipStream_t s = (hipStream_t)stream;
    const MpbLayout l = mpb_layout(n, m);
    uint64_t* miller = (uint64_t*)((char*)workspace + l.miller);
    uint64_t* prod = (uint64_t*)((char*)workspace + l.prod);
    uint64_t* dev_offsets = (uint64_t*)((char*)workspace + l.offsets);
    if (m == 1 && n) {
        // one product: the single-product entry, with its cooperative product paths
        int rc = pa_multi_pairing_device(p, q, n, out, ok, (pa_fq12*)miller, stream);
        if (rc) return rc;
        if (is_one) PA_TRY(pa::launch_fq12_is_one((const uint64_t*)out, ok, is_one, 1, s), "kernel launch");
        return PA_OK;
    }
    // The offsets go up first and the kernels are enqueued behind them; the host
    // then waits for that copy alone (host_offsets may be pageable and is the
    // caller's again on return), not for the kernels.
    hipEvent_t staged = nullptr;
    PA_TRY(hipEventCreateWithFlags(&staged, hipEventDisableTiming), "event");
    hipError_t e = hipMemcpyAsync(dev_offsets, host_offsets, sizeof(uint64_t) * (m + 1), hipMemcpyHostToDevice, s);
    if (e == hipSuccess) e = hipEventRecord(staged, s);
    if (e == hipSuccess && n) e = pairing_ml_launch((const uint64_t*)p, (const uint64_t*)q, miller, n, s);
    if (e == hipSuccess) e = pa::launch_fq12_segmented_product(miller, dev_offsets, n, m, max_len, prod, s);
    if (e == hipSuccess) e = fe_launch(prod, (uint64_t*)out, ok, m, s);
    if (e == hipSuccess && is_one) e = pa::launch_fq12_is_one((const uint64_t*)out, ok, is_one, m, s);
    const hipError_t w = hipEventSynchronize(staged);
    (void)hipEventDestroy(staged);
    if (e != hipSuccess) return fail(hip_code(e), "kernel launch", e);
    if (w != hipSuccess) return fail(hip_code(w), "H2D copy", w);
    return PA_OK;
}

int pa_multi_pairing_batch(const pa_g1_affine* p, const pa_g2_affine* q, const uint64_t* offsets, size_t m,
                           pa_fq12* out, uint8_t* ok, uint8_t* is_one) {
    if (m == 0) return PA_OK;
    if (!offsets || !ok || (!out && !is_one)) return fail(PA_ERR_INVALID_ARGUMENT, "null pointer");
    size_t max_len = 0;
    if (const char* bad = mpb_check_offsets(offsets, m, &max_len)) return fail(PA_ERR_INVALID_ARGUMENT, bad);
    const size_t n = (size_t)offsets[m];
    if (n && (!p || !q)) return fail(PA_ERR_INVALID_ARGUMENT, "null pointer");
    // one stream round trip: the pairs up, the device entry, the flags (and the
    // values, when asked for) down
    DevBuf dp, dq, dout, dflags, dws;
    int rc;
    if ((rc = upload(dp, p, sizeof(pa_g1_affine) * n)) || (rc = upload(dq, q, sizeof(pa_g2_affine) * n)))
        return rc;
    PA_TRY(dout.alloc(sizeof(pa_fq12) * m), "device scratch");
    PA_TRY(dflags.alloc(2 * m), "device scratch");   // ok, then is_one
    PA_TRY(dws.alloc(mpb_layout(n, m).bytes), "device scratch");
    uint8_t* dev_ok = dflags.as<uint8_t>();
    const hipStream_t s = call_stream();
    if ((rc = pa_multi_pairing_batch_device(dp.as<pa_g1_affine>(), dq.as<pa_g2_affine>(), offsets, m,
                                            dout.as<pa_fq12>(), dev_ok, is_one ? dev_ok + m : nullptr, dws.p, s)))
        return rc;
    PA_TRY(hipMemcpyAsync(ok, dev_ok, m, hipMemcpyDeviceToHost, s), "D2H copy");
    if (is_one) PA_TRY(hipMemcpyAsync(is_one, dev_ok + m, m, hipMemcpyDeviceToHost, s), "D2H copy");
    if (out) PA_TRY(hipMemcpyAsync(out, dout.p, sizeof(pa_fq12) * m, hipMemcpyDeviceToHost, s), "D2H copy");
    PA_TRY(hipStreamSynchronize(s), "kernel execution");
    return PA_OK;
}

// ---- point encodings ----
namespace {
constexpr size_t enc_size(int group, int compressed) { return (group == 1 ? 48 : 96) * (compressed ? 1 : 2); }
int host_decode(int group, const uint8_t* enc, size_t n, int compressed, int checked, void* out, uint8_t* status) {
    if (n == 0) return PA_OK;
    if (!enc || !out || !status) return fail(PA_ERR_INVALID_ARGUMENT, "null pointer");
    const size_t rec = group == 1 ? sizeof(pa_g1_affine) : sizeof(pa_g2_affine);
    DevBuf de, dout, dst;
    int rc;
    if ((rc = upload(de, enc, enc_size(group, compressed) * n))) return rc;
    PA_TRY(dout.alloc(rec * n), "device scratch");
    PA_TRY(dst.alloc(n), "device scratch");
    PA_TRY(pa::launch_decode(group, compressed, checked, de.as<uint8_t>(), n, dout.as<uint64_t>(),
                             dst.as<uint8_t>(), call_stream()),
           "kernel launch");
    PA_TRY(call_sync(), "kernel execution");
    if ((rc = download(out, dout, rec * n))) return rc;
    return download(status, dst, n);
}
int host_subgroup(int group, const void* pts, size_t n, uint8_t* ok) {
    if (n == 0) return PA_OK;
    if (!pts || !ok) return fail(PA_ERR_INVALID_ARGUMENT, "null pointer");
    const size_t rec = group == 1 ? sizeof(pa_g1_affine) : sizeof(pa_g2_affine);
    DevBuf dp, dok;
    int rc;
    if ((rc = upload(dp, pts, rec * n))) return rc;
    PA_TRY(dok.alloc(n), "device scratch");
    PA_TRY(pa::launch_subgroup_check(group, dp.as<uint64_t>(), n, dok.as<uint8_t>(), call_stream()), "kernel launch");
    PA_TRY(call_sync(), "kernel execution");
    return download(ok, dok, n);
}
int host_encode(int group, const void* in, size_t n, int compressed, uint8_t* enc) {
    if (n == 0) return PA_OK;
    if (!in || !enc) return fail(PA_ERR_INVALID_ARGUMENT, "null pointer");
    const size_t rec = group == 1 ? sizeof(pa_g1_affine) : sizeof(pa_g2_affine);
    DevBuf din, de;
    int rc;
    if ((rc = upload(din, in, rec * n))) return rc;
    PA_TRY(de.alloc(enc_size(group, compressed) * n), "device scratch");
    PA_TRY(pa::launch_encode(group, compressed, din.as<uint64_t>(), n, de.as<uint8_t>(), call_stream()), "kernel launch");
    PA_TRY(call_sync(), "kernel execution");
    return download(enc, de, enc_size(group, compressed) * n);
}
int host_sqrt(int degree, const void* a, void* out, uint8_t* ok, size_t n) {
    if (n == 0) return PA_OK;
    if (!a || !out || !ok) return fail(PA_ERR_INVALID_ARGUMENT, "null pointer");
    const size_t bytes = 48 * (size_t)degree * n;
    DevBuf da, dout, dok;
    int rc;
    if ((rc = upload(da, a, bytes))) return rc;
    PA_TRY(dout.alloc(bytes), "device scratch");
    PA_TRY(dok.alloc(n), "device scratch");
    PA_TRY(pa::launch_sqrt(degree, da.as<uint64_t>(), n, dout.as<uint64_t>(), dok.as<uint8_t>(), call_stream()),
           "kernel launch");
    PA_TRY(call_sync(), "kernel execution");
    if ((rc = download(out, dout, bytes))) return rc;
    return download(ok, dok, n);
}
}  // namespace

int pa_g1_decode_batch(const uint8_t* enc, size_t n, int compressed, int checked, pa_g1_affine* out,
                       uint8_t* status) {
    return host_decode(1, enc, n, compressed != 0, checked != 0, out, status);
}
int pa_g2_decode_batch(const uint8_t* enc, size_t n, int compressed, int checked, pa_g2_affine* out,
                       uint8_t* status) {
    return host_decode(2, enc, n, compressed != 0, checked != 0, out, status);
}
int pa_g1_subgroup_check_batch(const pa_g1_affine* p, size_t n, uint8_t* ok) { return host_subgroup(1, p, n, ok); }
int pa_g2_subgroup_check_batch(const pa_g2_affine* p, size_t n, uint8_t* ok) { return host_subgroup(2, p, n, ok); }
int pa_g1_encode_batch(const pa_g1_affine* in, size_t n, int compressed, uint8_t* enc) {
    return host_encode(1, in, n, compressed != 0, enc);
}
int pa_g2_encode_batch(const pa_g2_affine* in, size_t n, int compressed, uint8_t* enc) {
    return host_encode(2, in, n, compressed != 0, enc);
}
int pa_fq_sqrt_batch(const pa_fq* a, pa_fq* out, uint8_t* ok, size_t n) { return host_sqrt(1, a, out, ok, n); }
int pa_fq2_sqrt_batch(const pa_fq2* a, pa_fq2* out, uint8_t* ok, size_t n) { return host_sqrt(2, a, out, ok, n); }

int pa_g1_batch_normalization(pa_g1* v, size_t n) {
    if (n == 0) return PA_OK;
    if (!v) return fail(PA_ERR_INVALID_ARGUMENT, "null pointer");
    DevBuf dv;
    int rc;
    if ((rc = upload(dv, v, sizeof(pa_g1) * n))) return rc;
    PA_TRY(pa::launch_g1_batch_normalize(dv.as<uint64_t>(), n, call_stream()), "kernel launch");
    PA_TRY(call_sync(), "kernel execution");
    return download(v, dv, sizeof(pa_g1) * n);
}

int pa_g1_wnaf_fixed_base(const pa_g1* base, const pa_fr_repr* scalars, size_t n, pa_g1* out) {
    return pa_g1_wnaf_fixed_base_window(base, scalars, n, pa_g1_recommended_wnaf_for_num_scalars(n), out);
}
int pa_g1_wnaf_fixed_base_window(const pa_g1* base, const pa_fr_repr* scalars, size_t n, int window, pa_g1* out) {
    if (n == 0) return PA_OK;
    if (!base || !scalars || !out) return fail(PA_ERR_INVALID_ARGUMENT, "null pointer");
    if (window < 1 || window > kMaxWnafWindow) return fail(PA_ERR_INVALID_ARGUMENT, "wnaf window out of range");
    DevBuf db, ds, dt, dw, dout;
    int rc;
    if ((rc = upload(db, base, sizeof(pa_g1))) || (rc = upload(ds, scalars, sizeof(pa_fr_repr) * n))) return rc;
    PA_TRY(dt.alloc(8 * pa::g1_comb_table_words()), "device scratch");
    PA_TRY(dw.alloc(8 * pa::g1_comb_workspace_words()), "device scratch");
    PA_TRY(dout.alloc(sizeof(pa_g1) * n), "device scratch");
    PA_TRY(pa::launch_g1_fixed_base(db.as<uint64_t>(), ds.as<uint64_t>(), dout.as<uint64_t>(), n, dt.as<uint64_t>(),
                                    dw.as<uint64_t>(), window, call_stream()),
           "kernel launch");
    PA_TRY(call_sync(), "kernel execution");
    return download(out, dout, sizeof(pa_g1) * n);
}

// ---- bit-exact Wnaf (kernels_wnaf_exact.hip) ----
namespace {
// window 0 -> the reference's recommendation; else checked against the limit
int wx_window(int window, int dflt, int max) { return window == 0 ? dflt : (window < 1 || window > max ? -1 : window); }

int wx_host(int group, bool fixed_scalar, const void* base_or_bases, size_t n, const pa_fr_repr* s, size_t ns,
            int window, void* out) {
    if (n == 0) return PA_OK;
    const size_t jb = group == 1 ? sizeof(pa_g1) : sizeof(pa_g2);
    DevBuf db, ds, dw, dout;
    int rc;
    if ((rc = upload(db, base_or_bases, jb * (fixed_scalar ? n : 1))) ||
        (rc = upload(ds, s, sizeof(pa_fr_repr) * ns)))
        return rc;
    const size_t bytes = fixed_scalar ? pa::wx_scalar_layout(group, n, window).bytes
                                      : pa::wx_layout(group, n, window).bytes;
    PA_TRY(dw.alloc(bytes), "device scratch");
    PA_TRY(dout.alloc(jb * n), "device scratch");
    if (fixed_scalar)
        PA_TRY(pa::launch_wnaf_exact_fixed_scalar(group, db.as<uint64_t>(), n, ds.as<uint64_t>(), dout.as<uint64_t>(),
                                                  window, dw.p, call_stream()),
               "kernel launch");
    else
        PA_TRY(pa::launch_wnaf_exact_fixed_base(group, db.as<uint64_t>(), ds.as<uint64_t>(), dout.as<uint64_t>(), n,
                                                window, dw.p, call_stream()),
               "kernel launch");
    PA_TRY(call_sync(), "kernel execution");
    return download(out, dout, jb * n);
}
int wx_device(int group, bool fixed_scalar, const void* base_or_bases, size_t n, const pa_fr_repr* s, int window,
              void* out, void* workspace, size_t workspace_bytes, void* stream) {
    if (n == 0) return PA_OK;
    if (!base_or_bases || !s || !out || !workspace) return fail(PA_ERR_INVALID_ARGUMENT, "null pointer");
    const size_t need = fixed_scalar ? pa::wx_scalar_layout(group, n, window).bytes
                                     : pa::wx_layout(group, n, window).bytes;
    if (workspace_bytes < need) return fail(PA_ERR_INVALID_ARGUMENT, "wnaf exact workspace too small");
    if (fixed_scalar)
        PA_TRY(pa::launch_wnaf_exact_fixed_scalar(group, (const uint64_t*)base_or_bases, n, (const uint64_t*)s,
                                                  (uint64_t*)out, window, workspace, (hipStream_t)stream),
               "kernel launch");
    else
        PA_TRY(pa::launch_wnaf_exact_fixed_base(group, (const uint64_t*)base_or_bases, (const uint64_t*)s,
                                                (uint64_t*)out, n, window, workspace, (hipStream_t)stream),
               "kernel launch");
    return PA_OK;
}
}  // namespace

int pa_g1_wnaf_fixed_base_exact(const pa_g1* base, const pa_fr_repr* scalars, size_t n, int window, pa_g1* out) {
    if (n && (!base || !scalars || !out)) return fail(PA_ERR_INVALID_ARGUMENT, "null pointer");
    const int w = wx_window(window, pa_g1_recommended_wnaf_for_num_scalars(n), pa::kWxMaxWindow);
    if (w < 0) return fail(PA_ERR_INVALID_ARGUMENT, "wnaf window out of range (exact: 1..20)");
    return wx_host(1, false, base, n, scalars, n, w, out);
}
int pa_g2_wnaf_fixed_base_exact(const pa_g2* base, const pa_fr_repr* scalars, size_t n, int window, pa_g2* out) {
    if (n && (!base || !scalars || !out)) return fail(PA_ERR_INVALID_ARGUMENT, "null pointer");
    const int w = wx_window(window, pa_g2_recommended_wnaf_for_num_scalars(n), pa::kWxMaxWindow);
    if (w < 0) return fail(PA_ERR_INVALID_ARGUMENT, "wnaf window out of range (exact: 1..20)");
    return wx_host(2, false, base, n, scalars, n, w, out);
}
int pa_g1_wnaf_fixed_scalar_exact(const pa_g1* bases, size_t n, const pa_fr_repr* scalar, int window, pa_g1* out) {
    if (n && (!bases || !scalar || !out)) return fail(PA_ERR_INVALID_ARGUMENT, "null pointer");
    const int w = n ? wx_window(window, pa_g1_recommended_wnaf_for_scalar(scalar), pa::kWxMaxScalarWindow) : 1;
    if (w < 0) return fail(PA_ERR_INVALID_ARGUMENT, "wnaf window out of range (exact fixed scalar: 1..12)");
    return wx_host(1, true, bases, n, scalar, 1, w, out);
}
int pa_g2_wnaf_fixed_scalar_exact(const pa_g2* bases, size_t n, const pa_fr_repr* scalar, int window, pa_g2* out) {
    if (n && (!bases || !scalar || !out)) return fail(PA_ERR_INVALID_ARGUMENT, "null pointer");
    const int w = n ? wx_window(window, pa_g2_recommended_wnaf_for_scalar(scalar), pa::kWxMaxScalarWindow) : 1;
    if (w < 0) return fail(PA_ERR_INVALID_ARGUMENT, "wnaf window out of range (exact fixed scalar: 1..12)");
    return wx_host(2, true, bases, n, scalar, 1, w, out);
}
size_t pa_wnaf_exact_workspace_bytes(int group, size_t n, int window, int fixed_scalar) {
    const int max = fixed_scalar ? pa::kWxMaxScalarWindow : pa::kWxMaxWindow;
    if ((group != 1 && group != 2) || window < 1 || window > max) return 0;
    return fixed_scalar ? pa::wx_scalar_layout(group, n, window).bytes : pa::wx_layout(group, n, window).bytes;
}
int pa_g1_wnaf_fixed_base_exact_device(const pa_g1* base, const pa_fr_repr* scalars, pa_g1* out, size_t n,
                                       int window, void* workspace, size_t workspace_bytes, void* stream) {
    const int w = wx_window(window, pa_g1_recommended_wnaf_for_num_scalars(n), pa::kWxMaxWindow);
    if (w < 0) return fail(PA_ERR_INVALID_ARGUMENT, "wnaf window out of range (exact: 1..20)");
    return wx_device(1, false, base, n, scalars, w, out, workspace, workspace_bytes, stream);
}
int pa_g2_wnaf_fixed_base_exact_device(const pa_g2* base, const pa_fr_repr* scalars, pa_g2* out, size_t n,
                                       int window, void* workspace, size_t workspace_bytes, void* stream) {
    const int w = wx_window(window, pa_g2_recommended_wnaf_for_num_scalars(n), pa::kWxMaxWindow);
    if (w < 0) return fail(PA_ERR_INVALID_ARGUMENT, "wnaf window out of range (exact: 1..20)");
    return wx_device(2, false, base, n, scalars, w, out, workspace, workspace_bytes, stream);
}
// the scalar is device memory here: the window must be given (1..12)
int pa_g1_wnaf_fixed_scalar_exact_device(const pa_g1* bases, size_t n, const pa_fr_repr* scalar, pa_g1* out,
                                         int window, void* workspace, size_t workspace_bytes, void* stream) {
    if (window < 1 || window > pa::kWxMaxScalarWindow)
        return fail(PA_ERR_INVALID_ARGUMENT, "wnaf window out of range (exact fixed scalar, device: 1..12)");
    return wx_device(1, true, bases, n, scalar, window, out, workspace, workspace_bytes, stream);
}
int pa_g2_wnaf_fixed_scalar_exact_device(const pa_g2* bases, size_t n, const pa_fr_repr* scalar, pa_g2* out,
                                         int window, void* workspace, size_t workspace_bytes, void* stream) {
    if (window < 1 || window > pa::kWxMaxScalarWindow)
        return fail(PA_ERR_INVALID_ARGUMENT, "wnaf window out of range (exact fixed scalar, device: 1..12)");
    return wx_device(2, true, bases, n, scalar, window, out, workspace, workspace_bytes, stream);
}

// ---- device-resident variants ----
int pa_g1_subgroup_check_batch_device(const pa_g1_affine* p, size_t n, uint8_t* ok, void* stream) {
    if (n && (!p || !ok)) return fail(PA_ERR_INVALID_ARGUMENT, "null pointer");
    PA_TRY(pa::launch_subgroup_check(1, (const uint64_t*)p, n, ok, (hipStream_t)stream), "kernel launch");
    return PA_OK;
}
int pa_g2_subgroup_check_batch_device(const pa_g2_affine* p, size_t n, uint8_t* ok, void* stream) {
    if (n && (!p || !ok)) return fail(PA_ERR_INVALID_ARGUMENT, "null pointer");
    PA_TRY(pa::launch_subgroup_check(2, (const uint64_t*)p, n, ok, (hipStream_t)stream), "kernel launch");
    return PA_OK;
}
int pa_g1_decode_batch_device(const uint8_t* enc, size_t n, int compressed, int checked, pa_g1_affine* out,
                              uint8_t* status, void* stream) {
    if (n && (!enc || !out || !status)) return fail(PA_ERR_INVALID_ARGUMENT, "null pointer");
    PA_TRY(pa::launch_decode(1, compressed != 0, checked != 0, enc, n, (uint64_t*)out, status, (hipStream_t)stream),
           "kernel launch");
    return PA_OK;
}
int pa_g2_decode_batch_device(const uint8_t* enc, size_t n, int compressed, int checked, pa_g2_affine* out,
                              uint8_t* status, void* stream) {
    if (n && (!enc || !out || !status)) return fail(PA_ERR_INVALID_ARGUMENT, "null pointer");
    PA_TRY(pa::launch_decode(2, compressed != 0, checked != 0, enc, n, (uint64_t*)out, status, (hipStream_t)stream),
           "kernel launch");
    return PA_OK;
}
int pa_g1_batch_normalization_device(pa_g1* v, size_t n, void* stream) {
    if (n && !v) return fail(PA_ERR_INVALID_ARGUMENT, "null pointer");
    PA_TRY(pa::launch_g1_batch_normalize((uint64_t*)v, n, (hipStream_t)stream), "kernel launch");
    return PA_OK;
}
size_t pa_g1_fixed_base_table_words(void) { return pa::g1_comb_table_words(); }
size_t pa_g1_fixed_base_workspace_words(void) { return pa::g1_comb_workspace_words(); }
int pa_g1_fixed_base_table_device(const pa_g1* base, uint64_t* table, uint64_t* workspace, void* stream) {
    if (!base || !table || !workspace) return fail(PA_ERR_INVALID_ARGUMENT, "null pointer");
    PA_TRY(pa::launch_g1_comb_table((const uint64_t*)base, table, workspace, (hipStream_t)stream), "kernel launch");
    return PA_OK;
}
int pa_g1_fixed_base_mul_device(const uint64_t* table, const pa_fr_repr* scalars, pa_g1* out, size_t n,
                                void* stream) {
    if (n && (!table || !scalars || !out)) return fail(PA_ERR_INVALID_ARGUMENT, "null pointer");
    PA_TRY(pa::launch_g1_comb_mul(table, (const uint64_t*)scalars, (uint64_t*)out, n,
                                  pa_g1_recommended_wnaf_for_num_scalars(n), (hipStream_t)stream),
           "kernel launch");
    return PA_OK;
}
int pa_g1_fixed_base_glv_table_device(const pa_g1* base, uint64_t* table, uint64_t* workspace, void* stream) {
    if (!base || !table || !workspace) return fail(PA_ERR_INVALID_ARGUMENT, "null pointer");
    PA_TRY(pa::launch_g1_glv_table((const uint64_t*)base, table, workspace, (hipStream_t)stream), "kernel launch");
    return PA_OK;
}
int pa_g1_fixed_base_glv_mul_device(const pa_g1* base, const uint64_t* table, const uint64_t* workspace,
                                    const pa_fr_repr* scalars, pa_g1* out, size_t n, void* stream) {
    if (n && (!base || !table || !workspace || !scalars || !out)) return fail(PA_ERR_INVALID_ARGUMENT, "null pointer");
    PA_TRY(pa::launch_g1_glv_mul((const uint64_t*)base, table, workspace,
                                 (const uint64_t*)scalars, (uint64_t*)out, n, pa_g1_recommended_wnaf_for_num_scalars(n),
                                 (hipStream_t)stream),
           "kernel launch");
    return PA_OK;
}
int pa_g1_wnaf_fixed_base_device(const pa_g1* base, const pa_fr_repr* scalars, pa_g1* out, size_t n,
                                 uint64_t* table, uint64_t* workspace, void* stream) {
    return pa_g1_wnaf_fixed_base_window_device(base, scalars, out, n, pa_g1_recommended_wnaf_for_num_scalars(n), table,
                                               workspace, stream);
}
int pa_g1_wnaf_fixed_base_window_device(const pa_g1* base, const pa_fr_repr* scalars, pa_g1* out, size_t n,
                                        int window, uint64_t* table, uint64_t* workspace, void* stream) {
    if (n && (!base || !scalars || !out || !table || !workspace)) return fail(PA_ERR_INVALID_ARGUMENT, "null pointer");
    if (window < 1 || window > kMaxWnafWindow) return fail(PA_ERR_INVALID_ARGUMENT, "wnaf window out of range");
    PA_TRY(pa::launch_g1_fixed_base((const uint64_t*)base, (const uint64_t*)scalars, (uint64_t*)out, n, table,
                                    workspace, window, (hipStream_t)stream),
           "kernel launch");
    return PA_OK;
}
int pa_fq_mul_batch_device(const pa_fq* a, const pa_fq* b, pa_fq* out, size_t n, void* stream) {
    if (n && (!a || !b || !out)) return fail(PA_ERR_INVALID_ARGUMENT, "null pointer");
    PA_TRY(pa::launch_fq_mul_batch((const uint64_t*)a, (const uint64_t*)b, (uint64_t*)out, n, (hipStream_t)stream),
           "kernel launch");
    return PA_OK;
}
int pa_fq_mul_batch_soa_device(const uint64_t* a, const uint64_t* b, uint64_t* out, size_t n, void* stream) {
    if (n && (!a || !b || !out)) return fail(PA_ERR_INVALID_ARGUMENT, "null pointer");
    PA_TRY(pa::launch_fq_mul_batch_soa(a, b, out, n, (hipStream_t)stream), "kernel launch");
    return PA_OK;
}
int pa_miller_loop_fused_batch_device(const pa_g1_affine* p, const pa_g2_affine* q, pa_fq12* out, size_t n,
                                      void* stream) {
    if (n && (!p || !q || !out)) return fail(PA_ERR_INVALID_ARGUMENT, "null pointer");
    PA_TRY(ml_launch((const uint64_t*)p, (const uint64_t*)q, (uint64_t*)out, n, (hipStream_t)stream),
           "kernel launch");
    return PA_OK;
}
int pa_pairing_miller_loop_batch_device(const pa_g1_affine* p, const pa_g2_affine* q, pa_fq12* out, size_t n,
                                        void* stream) {
    if (n && (!p || !q || !out)) return fail(PA_ERR_INVALID_ARGUMENT, "null pointer");
    PA_TRY(pairing_ml_launch((const uint64_t*)p, (const uint64_t*)q, (uint64_t*)out, n, (hipStream_t)stream),
           "kernel launch");
    return PA_OK;
}
int pa_final_exponentiation_batch_device(const pa_fq12* in, pa_fq12* out, uint8_t* ok, size_t n, void* stream) {
    if (n && (!in || !out)) return fail(PA_ERR_INVALID_ARGUMENT, "null pointer");
    PA_TRY(fe_launch((const uint64_t*)in, (uint64_t*)out, ok, n, (hipStream_t)stream), "kernel launch");
    return PA_OK;
}
int pa_g2_prepare_batch_device(const pa_g2_affine* q, pa_g2_prepared* out, size_t n, void* stream) {
    if (n && (!q || !out)) return fail(PA_ERR_INVALID_ARGUMENT, "null pointer");
    PA_TRY(pa::launch_g2_prepare((const uint64_t*)q, (uint64_t*)out, n, (hipStream_t)stream), "kernel launch");
    return PA_OK;
}
int pa_miller_loop_batch_device(const pa_g1_affine* p, const pa_g2_prepared* q, pa_fq12* out, size_t n,
                                void* stream) {
    if (n && (!p || !q || !out)) return fail(PA_ERR_INVALID_ARGUMENT, "null pointer");
    PA_TRY(pa::launch_miller_loop_prepared_gen((const uint64_t*)p, (const uint64_t*)q, (uint64_t*)out, n,
                                               (hipStream_t)stream),
           "kernel launch");
    return PA_OK;
}
int pa_miller_loop_shared_prepared_device(const pa_g1_affine* p, size_t n, const pa_g2_prepared* q, pa_fq12* out,
                                          void* stream) {
    if (n && (!p || !q || !out)) return fail(PA_ERR_INVALID_ARGUMENT, "null pointer");
    PA_TRY(pa::launch_miller_loop_shared_gen((const uint64_t*)p, (const uint64_t*)q, (uint64_t*)out, n,
                                             (hipStream_t)stream),
           "kernel launch");
    return PA_OK;
}
int pa_pairing_batch_device(const pa_g1_affine* p, const pa_g2_affine* q, pa_fq12* out, pa_fq12* scratch,
                            size_t n, void* stream) {
    if (n && (!p || !q || !out || !scratch)) return fail(PA_ERR_INVALID_ARGUMENT, "null pointer");
    PA_TRY(pairing_ml_launch((const uint64_t*)p, (const uint64_t*)q, (uint64_t*)scratch, n, (hipStream_t)stream),
           "kernel launch");
    PA_TRY(fe_launch((const uint64_t*)scratch, (uint64_t*)out, nullptr, n, (hipStream_t)stream), "kernel launch");
    return PA_OK;
}

// ---- scalar field Fr (fr.rs) ----
namespace {
bool fr_op_needs_b(int op) { return op == pa::FR_MUL || op == pa::FR_ADD || op == pa::FR_SUB; }
int host_fr_op(int op, const void* a, const void* b, void* out, uint8_t* flag, const uint64_t* exp, size_t exp_words,
               size_t n) {
    if (n == 0) return PA_OK;
    const bool has_out = op != pa::FR_LEGENDRE;
    const bool has_flag = op == pa::FR_INV || op == pa::FR_FROM_REPR || op == pa::FR_SQRT || op == pa::FR_LEGENDRE;
    if (!a || (has_out && !out) || (fr_op_needs_b(op) && !b) || (has_flag && !flag) ||
        (op == pa::FR_POW && exp_words && !exp))
        return fail(PA_ERR_INVALID_ARGUMENT, "null pointer");
    if (exp_words > (1u << 20)) return fail(PA_ERR_INVALID_ARGUMENT, "exponent too long");
    DevBuf da, db, dout, dflag, dexp;
    int rc;
    const size_t bytes = 32 * n;
    if ((rc = upload(da, a, bytes))) return rc;
    if (fr_op_needs_b(op) && (rc = upload(db, b, bytes))) return rc;
    if (op == pa::FR_POW && (rc = upload(dexp, exp, 8 * exp_words))) return rc;
    PA_TRY(dout.alloc(bytes), "device scratch");
    if (has_flag) PA_TRY(dflag.alloc(n), "device scratch");
    PA_TRY(pa::launch_fr_op(op, da.as<uint64_t>(), db.as<uint64_t>(), dout.as<uint64_t>(), dflag.as<uint8_t>(),
                            dexp.as<uint64_t>(), (int)exp_words, n, call_stream()),
           "kernel launch");
    PA_TRY(call_sync(), "kernel execution");
    if (has_out && (rc = download(out, dout, bytes))) return rc;
    if (has_flag && (rc = download(flag, dflag, n))) return rc;
    return PA_OK;
}
}  // namespace

int pa_fr_mul_batch(const pa_fr* a, const pa_fr* b, pa_fr* out, size_t n) {
    return host_fr_op(pa::FR_MUL, a, b, out, nullptr, nullptr, 0, n);
}
int pa_fr_square_batch(const pa_fr* a, pa_fr* out, size_t n) {
    return host_fr_op(pa::FR_SQR, a, nullptr, out, nullptr, nullptr, 0, n);
}
int pa_fr_add_batch(const pa_fr* a, const pa_fr* b, pa_fr* out, size_t n) {
    return host_fr_op(pa::FR_ADD, a, b, out, nullptr, nullptr, 0, n);
}
int pa_fr_sub_batch(const pa_fr* a, const pa_fr* b, pa_fr* out, size_t n) {
    return host_fr_op(pa::FR_SUB, a, b, out, nullptr, nullptr, 0, n);
}
int pa_fr_double_batch(const pa_fr* a, pa_fr* out, size_t n) {
    return host_fr_op(pa::FR_DBL, a, nullptr, out, nullptr, nullptr, 0, n);
}
int pa_fr_negate_batch(const pa_fr* a, pa_fr* out, size_t n) {
    return host_fr_op(pa::FR_NEG, a, nullptr, out, nullptr, nullptr, 0, n);
}
int pa_fr_inverse_batch(const pa_fr* a, pa_fr* out, uint8_t* ok, size_t n) {
    return host_fr_op(pa::FR_INV, a, nullptr, out, ok, nullptr, 0, n);
}
int pa_fr_from_repr_batch(const pa_fr_repr* repr, pa_fr* out, uint8_t* ok, size_t n) {
    return host_fr_op(pa::FR_FROM_REPR, repr, nullptr, out, ok, nullptr, 0, n);
}
int pa_fr_into_repr_batch(const pa_fr* a, pa_fr_repr* out, size_t n) {
    return host_fr_op(pa::FR_INTO_REPR, a, nullptr, out, nullptr, nullptr, 0, n);
}
int pa_fr_pow_batch(const pa_fr* a, const uint64_t* exp, size_t exp_words, pa_fr* out, size_t n) {
    return host_fr_op(pa::FR_POW, a, nullptr, out, nullptr, exp, exp_words, n);
}
int pa_fr_legendre_batch(const pa_fr* a, int8_t* out, size_t n) {
    return host_fr_op(pa::FR_LEGENDRE, a, nullptr, nullptr, (uint8_t*)out, nullptr, 0, n);
}
int pa_fr_sqrt_batch(const pa_fr* a, pa_fr* out, uint8_t* ok, size_t n) {
    return host_fr_op(pa::FR_SQRT, a, nullptr, out, ok, nullptr, 0, n);
}
int pa_fr_mul_batch_device(const pa_fr* a, const pa_fr* b, pa_fr* out, size_t n, void* stream) {
    if (n && (!a || !b || !out)) return fail(PA_ERR_INVALID_ARGUMENT, "null pointer");
    PA_TRY(pa::launch_fr_mul_batch((const uint64_t*)a, (const uint64_t*)b, (uint64_t*)out, n, (hipStream_t)stream),
           "kernel launch");
    return PA_OK;
}

// ---- variable-base scalar multiplication and MSM (kernels_msm.hip) ----
namespace {
int host_scalar_mul(int group, int projective, const void* p, const pa_fr_repr* s, void* out, size_t n) {
    if (n == 0) return PA_OK;
    if (!p || !s || !out) return fail(PA_ERR_INVALID_ARGUMENT, "null pointer");
    const size_t in_rec = projective ? (group == 1 ? sizeof(pa_g1) : sizeof(pa_g2))
                                     : (group == 1 ? sizeof(pa_g1_affine) : sizeof(pa_g2_affine));
    const size_t out_rec = group == 1 ? sizeof(pa_g1) : sizeof(pa_g2);
    DevBuf dp, ds, dout;
    int rc;
    if ((rc = upload(dp, p, in_rec * n)) || (rc = upload(ds, s, sizeof(pa_fr_repr) * n))) return rc;
    PA_TRY(dout.alloc(out_rec * n), "device scratch");
    PA_TRY(pa::launch_scalar_mul(group, projective, dp.as<uint64_t>(), ds.as<uint64_t>(), n, dout.as<uint64_t>(),
                                 call_stream()),
           "kernel launch");
    PA_TRY(call_sync(), "kernel execution");
    return download(out, dout, out_rec * n);
}
int host_multiexp(int group, const void* bases, const pa_fr_repr* s, size_t n, void* out) {
    if (!out || (n && (!bases || !s))) return fail(PA_ERR_INVALID_ARGUMENT, "null pointer");
    if (n >= 0x80000000ull) return fail(PA_ERR_INVALID_ARGUMENT, "multiexp supports n < 2^31");
    const size_t in_rec = group == 1 ? sizeof(pa_g1_affine) : sizeof(pa_g2_affine);
    const size_t out_rec = group == 1 ? sizeof(pa_g1) : sizeof(pa_g2);
    DevBuf db, ds, dout, dws;
    int rc;
    if ((rc = upload(db, bases, in_rec * n)) || (rc = upload(ds, s, sizeof(pa_fr_repr) * n))) return rc;
    PA_TRY(dout.alloc(out_rec), "device scratch");
    const size_t ws = pa::msm_workspace_bytes(group, n);
    PA_TRY(dws.alloc(ws), "device scratch");
    PA_TRY(pa::launch_msm(group, db.as<uint64_t>(), ds.as<uint64_t>(), n, dout.as<uint64_t>(), dws.p, ws, call_stream()),
           "kernel launch");
    PA_TRY(call_sync(), "kernel execution");
    return download(out, dout, out_rec);
}
}  // namespace

int pa_g1_affine_mul_batch(const pa_g1_affine* p, const pa_fr_repr* s, pa_g1* out, size_t n) {
    return host_scalar_mul(1, 0, p, s, out, n);
}
int pa_g2_affine_mul_batch(const pa_g2_affine* p, const pa_fr_repr* s, pa_g2* out, size_t n) {
    return host_scalar_mul(2, 0, p, s, out, n);
}
int pa_g1_mul_assign_batch(const pa_g1* p, const pa_fr_repr* s, pa_g1* out, size_t n) {
    return host_scalar_mul(1, 1, p, s, out, n);
}
int pa_g2_mul_assign_batch(const pa_g2* p, const pa_fr_repr* s, pa_g2* out, size_t n) {
    return host_scalar_mul(2, 1, p, s, out, n);
}
int pa_g1_multiexp(const pa_g1_affine* bases, const pa_fr_repr* scalars, size_t n, pa_g1* out) {
    return host_multiexp(1, bases, scalars, n, out);
}
int pa_g2_multiexp(const pa_g2_affine* bases, const pa_fr_repr* scalars, size_t n, pa_g2* out) {
    return host_multiexp(2, bases, scalars, n, out);
}
size_t pa_multiexp_workspace_bytes(int group, size_t n) {
    return (group == 1 || group == 2) ? pa::msm_workspace_bytes(group, n) : 0;
}
int pa_g1_multiexp_device(const pa_g1_affine* bases, const pa_fr_repr* scalars, size_t n, pa_g1* out,
                          void* workspace, size_t workspace_bytes, void* stream) {
    if (!out || (n && (!bases || !scalars || !workspace))) return fail(PA_ERR_INVALID_ARGUMENT, "null pointer");
    if (n && workspace_bytes < pa::msm_workspace_bytes(1, n))
        return fail(PA_ERR_INVALID_ARGUMENT, "workspace smaller than pa_multiexp_workspace_bytes");
    PA_TRY(pa::launch_msm(1, (const uint64_t*)bases, (const uint64_t*)scalars, n, (uint64_t*)out, workspace,
                          workspace_bytes, (hipStream_t)stream),
           "kernel launch");
    return PA_OK;
}
int pa_g2_multiexp_device(const pa_g2_affine* bases, const pa_fr_repr* scalars, size_t n, pa_g2* out,
                          void* workspace, size_t workspace_bytes, void* stream) {
    if (!out || (n && (!bases || !scalars || !workspace))) return fail(PA_ERR_INVALID_ARGUMENT, "null pointer");
    if (n && workspace_bytes < pa::msm_workspace_bytes(2, n))
        return fail(PA_ERR_INVALID_ARGUMENT, "workspace smaller than pa_multiexp_workspace_bytes");
    PA_TRY(pa::launch_msm(2, (const uint64_t*)bases, (const uint64_t*)scalars, n, (uint64_t*)out, workspace,
                          workspace_bytes, (hipStream_t)stream),
           "kernel launch");
    return PA_OK;
}

// 128-bit scalars over per-call bases: the 130-bit window plan, no endomorphism (kernels_msm.hip)
size_t pa_g1_multiexp_u128_workspace_bytes(size_t n) { return pa::msm_u128_workspace_bytes(n); }
int pa_g1_multiexp_u128_device(const pa_g1_affine* bases, const uint64_t* scalars, size_t n, pa_g1* out,
                               void* workspace, size_t workspace_bytes, void* stream) {
    if (!out || (n && (!bases || !scalars || !workspace))) return fail(PA_ERR_INVALID_ARGUMENT, "null pointer");
    if (n >= 0x80000000ull) return fail(PA_ERR_INVALID_ARGUMENT, "multiexp supports n < 2^31");
    if ((uintptr_t)scalars & 15) return fail(PA_ERR_INVALID_ARGUMENT, "scalars are not 16-byte aligned");
    if (n && workspace_bytes < pa::msm_u128_workspace_bytes(n))
        return fail(PA_ERR_INVALID_ARGUMENT, "workspace smaller than pa_g1_multiexp_u128_workspace_bytes");
    PA_TRY(pa::launch_msm_u128_g1((const uint64_t*)bases, scalars, n, (uint64_t*)out, workspace, workspace_bytes,
                                  (hipStream_t)stream),
           "kernel launch");
    return PA_OK;
}
int pa_g1_multiexp_u128(const pa_g1_affine* bases, const uint64_t* scalars, size_t n, pa_g1* out) {
    if (!out || (n && (!bases || !scalars))) return fail(PA_ERR_INVALID_ARGUMENT, "null pointer");
    if (n >= 0x80000000ull) return fail(PA_ERR_INVALID_ARGUMENT, "multiexp supports n < 2^31");
    DevBuf db, ds, dout, dws;
    int rc;
    if ((rc = upload(db, bases, sizeof(pa_g1_affine) * n)) || (rc = upload(ds, scalars, 16 * n))) return rc;
    PA_TRY(dout.alloc(sizeof(pa_g1)), "device scratch");
    const size_t ws = pa::msm_u128_workspace_bytes(n);
    PA_TRY(dws.alloc(ws), "device scratch");
    if ((rc = pa_g1_multiexp_u128_device(db.as<pa_g1_affine>(), ds.as<uint64_t>(), n, dout.as<pa_g1>(), dws.p, ws,
                                         call_stream())))
        return rc;
    PA_TRY(call_sync(), "kernel execution");
    return download(out, dout, sizeof(pa_g1));
}

// ---- MSM over prepared bases, G1 and G2 (kernels_msm.hip) ----
// The object owns the 2n lazy rows on one device and remembers whether every
// base passed the group's membership test: the host picks the GLV pipeline
// (flag 1) or the 257-bit one over the same rows (flag 0) from it.  Both
// groups' entries are the same code over MsmAbi<G>.
struct MsmBasesObj {
    int dev = 0;
    size_t n = 0;
    int in_subgroup = 0;
    uint32_t* rows = nullptr;
};
struct pa_g1_msm_bases : MsmBasesObj {};
struct pa_g2_msm_bases : MsmBasesObj {};

extern "C++" {   // templates
namespace {
// the current device switched to `dev` for a scope (allocations belong to the current device)
struct DeviceScope {
    int prev = -1;
    bool switched = false;
    hipError_t enter(int dev) {
        hipError_t e = hipGetDevice(&prev);
        if (e != hipSuccess || prev == dev) return e;
        if ((e = hipSetDevice(dev)) == hipSuccess) switched = true;
        return e;
    }
    ~DeviceScope() {
        if (switched) (void)hipSetDevice(prev);
    }
};

// the group's records and the entry names its messages quote
template <int G> struct MsmAbi;
template <> struct MsmAbi<1> {
    using Bases = pa_g1_msm_bases;
    using Affine = pa_g1_affine;
    using Point = pa_g1;
    static constexpr const char* small_ws = "workspace smaller than pa_g1_multiexp_prepared_workspace_bytes";
    static constexpr const char* small_batch_ws =
        "workspace smaller than pa_g1_multiexp_prepared_batch_workspace_bytes";
};
template <> struct MsmAbi<2> {
    using Bases = pa_g2_msm_bases;
    using Affine = pa_g2_affine;
    using Point = pa_g2;
    static constexpr const char* small_ws = "workspace smaller than pa_g2_multiexp_prepared_workspace_bytes";
    static constexpr const char* small_batch_ws =
        "workspace smaller than pa_g2_multiexp_prepared_batch_workspace_bytes";
};

template <int G>
int msm_bases_prepare_device(const typename MsmAbi<G>::Affine* bases, size_t n, void* stream,
                             typename MsmAbi<G>::Bases** out) {
    using Bases = typename MsmAbi<G>::Bases;
    if (!out) return fail(PA_ERR_INVALID_ARGUMENT, "null pointer");
    *out = nullptr;
    if (n && !bases) return fail(PA_ERR_INVALID_ARGUMENT, "null pointer");
    if (n >= pa::kMsmPreparedMax) return fail(PA_ERR_INVALID_ARGUMENT, "prepared multiexp bases support n < 2^30");
    hipStream_t s = (hipStream_t)stream;
    int dev = 0;
    PA_TRY(hipStreamGetDevice(s, &dev), "stream device");
    DeviceScope scope;
    PA_TRY(scope.enter(dev), "set device");
    Bases* b = new Bases;
    b->dev = dev;
    b->n = n;
    b->in_subgroup = 1;
    if (n == 0) {
        *out = b;
        return PA_OK;
    }
    // scratch: the per-base membership flags, then the count of failed ones
    const size_t bad_off = (n + 255) & ~(size_t)255;
    uint8_t* scratch = nullptr;
    uint32_t bad = 0;
    hipError_t e = hipMalloc((void**)&b->rows, pa::msm_prepared_rows_bytes(n, G));
    if (e == hipSuccess) e = hipMalloc((void**)&scratch, bad_off + sizeof(uint32_t));
    uint32_t* dbad = reinterpret_cast<uint32_t*>(scratch + bad_off);
    if (e == hipSuccess) e = pa::launch_subgroup_check(G, (const uint64_t*)bases, n, scratch, s);
    if (e == hipSuccess) e = pa::launch_msm_prepare(G, (const uint64_t*)bases, scratch, n, b->rows, dbad, s);
    if (e == hipSuccess) e = hipMemcpyAsync(&bad, dbad, sizeof bad, hipMemcpyDeviceToHost, s);
    const hipError_t sync = hipStreamSynchronize(s);   // also before the scratch goes, whatever failed above
    if (e == hipSuccess) e = sync;
    if (scratch) (void)hipFree(scratch);
    if (e != hipSuccess) {
        if (b->rows) (void)hipFree(b->rows);
        delete b;
        return fail(hip_code(e), "prepare multiexp bases", e);
    }
    b->in_subgroup = bad == 0 ? 1 : 0;
    *out = b;
    return PA_OK;
}
template <int G>
int msm_bases_prepare(const typename MsmAbi<G>::Affine* bases, size_t n, typename MsmAbi<G>::Bases** out) {
    if (!out) return fail(PA_ERR_INVALID_ARGUMENT, "null pointer");
    *out = nullptr;
    if (n && !bases) return fail(PA_ERR_INVALID_ARGUMENT, "null pointer");
    if (n >= pa::kMsmPreparedMax) return fail(PA_ERR_INVALID_ARGUMENT, "prepared multiexp bases support n < 2^30");
    DevBuf db;
    int rc;
    if ((rc = upload(db, bases, sizeof(typename MsmAbi<G>::Affine) * n))) return rc;
    return msm_bases_prepare_device<G>(db.as<typename MsmAbi<G>::Affine>(), n, call_stream(), out);
}
template <class Bases>
int msm_bases_free(Bases* b) {
    if (!b) return PA_OK;
    const hipError_t e = b->rows ? hipFree(b->rows) : hipSuccess;
    delete b;
    if (e != hipSuccess) return fail(hip_code(e), "free multiexp bases", e);
    return PA_OK;
}
template <int G>
int msm_prepared_device(const typename MsmAbi<G>::Bases* b, const pa_fr_repr* scalars, size_t m,
                        typename MsmAbi<G>::Point* out, void* workspace, size_t workspace_bytes, void* stream) {
    if (!b || !out || (m && (!scalars || !workspace))) return fail(PA_ERR_INVALID_ARGUMENT, "null pointer");
    if (m > b->n) return fail(PA_ERR_INVALID_ARGUMENT, "more scalars than prepared bases");
    if (m && workspace_bytes < pa::msm_prepared_workspace_bytes(m, b->in_subgroup != 0, G))
        return fail(PA_ERR_INVALID_ARGUMENT, MsmAbi<G>::small_ws);
    int dev = 0;
    PA_TRY(hipStreamGetDevice((hipStream_t)stream, &dev), "stream device");
    if (dev != b->dev) return fail(PA_ERR_INVALID_ARGUMENT, "stream is on another device than the prepared bases");
    PA_TRY(pa::launch_msm_prepared(G, b->rows, b->n, b->in_subgroup != 0, (const uint64_t*)scalars, m, 1, false,
                                   (uint64_t*)out, workspace, workspace_bytes, (hipStream_t)stream),
           "kernel launch");
    return PA_OK;
}
template <int G>
int msm_prepared_host(const typename MsmAbi<G>::Bases* b, const pa_fr_repr* scalars, size_t m,
                      typename MsmAbi<G>::Point* out) {
    using Point = typename MsmAbi<G>::Point;
    if (!b || !out || (m && !scalars)) return fail(PA_ERR_INVALID_ARGUMENT, "null pointer");
    if (m > b->n) return fail(PA_ERR_INVALID_ARGUMENT, "more scalars than prepared bases");
    DevBuf ds, dout, dws;
    int rc;
    if ((rc = upload(ds, scalars, sizeof(pa_fr_repr) * m))) return rc;
    PA_TRY(dout.alloc(sizeof(Point)), "device scratch");
    const size_t ws = pa::msm_prepared_workspace_bytes(m, b->in_subgroup != 0, G);
    PA_TRY(dws.alloc(ws), "device scratch");
    if ((rc = msm_prepared_device<G>(b, ds.as<pa_fr_repr>(), m, dout.as<Point>(), dws.p, ws, call_stream())))
        return rc;
    PA_TRY(call_sync(), "kernel execution");
    return download(out, dout, sizeof(Point));
}

// k scalar vectors over the same prepared bases in one pipeline
// what both batch entries refuse before touching memory; 0 = go on
int batch_args(const MsmBasesObj* b, int group, size_t m, size_t k, unsigned flags) {
    if (flags & ~PA_MSM_SCALARS_MONTGOMERY) return fail(PA_ERR_INVALID_ARGUMENT, "unknown PA_MSM_SCALARS_* flag bits");
    if (m > b->n) return fail(PA_ERR_INVALID_ARGUMENT, "more scalars than prepared bases");
    if (!pa::msm_prepared_batch_fits(m, k, b->in_subgroup != 0, group))
        return fail(PA_ERR_INVALID_ARGUMENT,
                    "batch over the 32-bit item limit (k * windows * terms <= 2^32 - 1, k * windows * buckets < 2^32): "
                    "split it");
    return PA_OK;
}
template <int G>
int msm_prepared_batch_device(const typename MsmAbi<G>::Bases* b, const void* scalars, size_t m, size_t k,
                              unsigned flags, typename MsmAbi<G>::Point* out, void* workspace, size_t workspace_bytes,
                              void* stream) {
    if (!b) return fail(PA_ERR_INVALID_ARGUMENT, "null pointer");
    int rc;
    if ((rc = batch_args(b, G, m, k, flags))) return rc;
    if (k == 0) return PA_OK;
    if (!out || (m && (!scalars || !workspace))) return fail(PA_ERR_INVALID_ARGUMENT, "null pointer");
    if (m && workspace_bytes < pa::msm_prepared_batch_workspace_bytes(m, k, b->in_subgroup != 0, G))
        return fail(PA_ERR_INVALID_ARGUMENT, MsmAbi<G>::small_batch_ws);
    int dev = 0;
    PA_TRY(hipStreamGetDevice((hipStream_t)stream, &dev), "stream device");
    if (dev != b->dev) return fail(PA_ERR_INVALID_ARGUMENT, "stream is on another device than the prepared bases");
    PA_TRY(pa::launch_msm_prepared(G, b->rows, b->n, b->in_subgroup != 0, (const uint64_t*)scalars, m, k,
                                   (flags & PA_MSM_SCALARS_MONTGOMERY) != 0, (uint64_t*)out, workspace,
                                   workspace_bytes, (hipStream_t)stream),
           "kernel launch");
    return PA_OK;
}
template <int G>
int msm_prepared_batch_host(const typename MsmAbi<G>::Bases* b, const void* scalars, size_t m, size_t k,
                            unsigned flags, typename MsmAbi<G>::Point* out) {
    using Point = typename MsmAbi<G>::Point;
    if (!b) return fail(PA_ERR_INVALID_ARGUMENT, "null pointer");
    int rc;
    if ((rc = batch_args(b, G, m, k, flags))) return rc;
    if (k == 0) return PA_OK;
    if (!out || (m && !scalars)) return fail(PA_ERR_INVALID_ARGUMENT, "null pointer");
    DevBuf ds, dout, dws;
    // k m rows fit: a batch within the item limit has k * m < 2^32
    if ((rc = upload(ds, scalars, sizeof(pa_fr_repr) * m * k))) return rc;
    PA_TRY(dout.alloc(sizeof(Point) * k), "device scratch");
    const size_t ws = pa::msm_prepared_batch_workspace_bytes(m, k, b->in_subgroup != 0, G);
    PA_TRY(dws.alloc(ws), "device scratch");
    if ((rc = msm_prepared_batch_device<G>(b, ds.p, m, k, flags, dout.as<Point>(), dws.p, ws, call_stream())))
        return rc;
    PA_TRY(call_sync(), "kernel execution");
    return download(out, dout, sizeof(Point) * k);
}
}  // namespace
}  // extern "C++"

#define PA_MSM_PREPARED_ENTRIES(G)                                                                                     \
    int pa_g##G##_msm_bases_prepare_device(const pa_g##G##_affine* bases, size_t n, void* stream,                      \
                                           pa_g##G##_msm_bases** out) {                                                \
        return msm_bases_prepare_device<G>(bases, n, stream, out);                                                     \
    }                                                                                                                  \
    int pa_g##G##_msm_bases_prepare(const pa_g##G##_affine* bases, size_t n, pa_g##G##_msm_bases** out) {              \
        return msm_bases_prepare<G>(bases, n, out);                                                                    \
    }                                                                                                                  \
    size_t pa_g##G##_msm_bases_len(const pa_g##G##_msm_bases* b) { return b ? b->n : 0; }                              \
    int pa_g##G##_msm_bases_in_subgroup(const pa_g##G##_msm_bases* b) { return b ? b->in_subgroup : 0; }               \
    int pa_g##G##_msm_bases_free(pa_g##G##_msm_bases* b) { return msm_bases_free(b); }                                 \
    size_t pa_g##G##_multiexp_prepared_workspace_bytes(const pa_g##G##_msm_bases* b, size_t m) {                       \
        return b && m <= b->n ? pa::msm_prepared_workspace_bytes(m, b->in_subgroup != 0, G) : 0;                       \
    }                                                                                                                  \
    int pa_g##G##_multiexp_prepared_device(const pa_g##G##_msm_bases* b, const pa_fr_repr* scalars, size_t m,          \
                                           pa_g##G* out, void* workspace, size_t workspace_bytes, void* stream) {      \
        return msm_prepared_device<G>(b, scalars, m, out, workspace, workspace_bytes, stream);                         \
    }                                                                                                                  \
    int pa_g##G##_multiexp_prepared(const pa_g##G##_msm_bases* b, const pa_fr_repr* scalars, size_t m, pa_g##G* out) { \
        return msm_prepared_host<G>(b, scalars, m, out);                                                               \
    }                                                                                                                  \
    size_t pa_g##G##_multiexp_prepared_batch_workspace_bytes(const pa_g##G##_msm_bases* b, size_t m, size_t k) {       \
        return b && m <= b->n ? pa::msm_prepared_batch_workspace_bytes(m, k, b->in_subgroup != 0, G) : 0;              \
    }                                                                                                                  \
    int pa_g##G##_multiexp_prepared_batch_device(const pa_g##G##_msm_bases* b, const void* scalars, size_t m,          \
                                                 size_t k, unsigned flags, pa_g##G* out, void* workspace,              \
                                                 size_t workspace_bytes, void* stream) {                               \
        return msm_prepared_batch_device<G>(b, scalars, m, k, flags, out, workspace, workspace_bytes, stream);         \
    }                                                                                                                  \
    int pa_g##G##_multiexp_prepared_batch(const pa_g##G##_msm_bases* b, const void* scalars, size_t m, size_t k,       \
                                          unsigned flags, pa_g##G* out) {                                              \
        return msm_prepared_batch_host<G>(b, scalars, m, k, flags, out);                                               \
    }
PA_MSM_PREPARED_ENTRIES(1)
PA_MSM_PREPARED_ENTRIES(2)
#undef PA_MSM_PREPARED_ENTRIES

// ---- batched Fr NTT over a radix-2 evaluation domain (kernels_ntt.hip) ----
// The object owns the power tables of its size on one device; the tile log
// (PA_NTT_TILE_LOG) is read when it is created and fixes the pass structure.
struct pa_fr_ntt_domain {
    int dev = 0;
    pa::NttLayout layout{};
    uint64_t* tables = nullptr;
};

int pa_fr_ntt_domain_create(unsigned log_n, pa_fr_ntt_domain** out) {
    if (!out) return fail(PA_ERR_INVALID_ARGUMENT, "null pointer");
    *out = nullptr;
    if (log_n > pa::kNttMaxLogN) return fail(PA_ERR_INVALID_ARGUMENT, "NTT domains support log_n <= 28");
    unsigned tile_log = pa::kNttDefaultTileLog;
    if (const char* e = getenv("PA_NTT_TILE_LOG")) {
        char* end = nullptr;
        const long v = strtol(e, &end, 10);
        if (end != e && *end == '\0')   // anything that is not a number leaves the default
            tile_log = v < 1 ? 1u : (v > (long)pa::kNttMaxTileLog ? pa::kNttMaxTileLog : (unsigned)v);
    }
    pa_fr_ntt_domain* d = new pa_fr_ntt_domain;
    d->layout = pa::ntt_layout(log_n, tile_log);
    hipError_t e = hipGetDevice(&d->dev);
    if (e == hipSuccess) e = hipMalloc((void**)&d->tables, d->layout.rows * 32);
    if (e == hipSuccess) e = pa::launch_ntt_build(d->layout, d->tables, call_stream());
    if (e == hipSuccess) e = call_sync();
    if (e != hipSuccess) {
        if (d->tables) (void)hipFree(d->tables);
        delete d;
        return fail(hip_code(e), "create NTT domain", e);
    }
    *out = d;
    return PA_OK;
}
void pa_fr_ntt_domain_free(pa_fr_ntt_domain* d) {
    if (!d) return;
    if (d->tables) (void)hipFree(d->tables);
    delete d;
}
unsigned pa_fr_ntt_domain_log_n(const pa_fr_ntt_domain* d) { return d ? d->layout.log_n : 0; }
size_t pa_fr_ntt_domain_bytes(const pa_fr_ntt_domain* d) { return d ? d->layout.rows * 32 : 0; }
unsigned pa_fr_ntt_domain_passes(const pa_fr_ntt_domain* d) { return d ? d->layout.passes : 0; }
unsigned pa_fr_ntt_domain_tile_log(const pa_fr_ntt_domain* d) { return d ? d->layout.tile_log : 0; }
size_t pa_fr_ntt_polys_per_workgroup(const pa_fr_ntt_domain* d) {
    return d ? pa::ntt_polys_per_workgroup(d->layout) : 0;
}
unsigned pa_fr_ntt_max_log_n(void) { return pa::kNttMaxLogN; }
size_t pa_fr_ntt_workspace_bytes(const pa_fr_ntt_domain* d, size_t batch) {
    return d && pa::ntt_batch_fits(d->layout, batch) ? pa::ntt_workspace_bytes(d->layout, batch) : 0;
}

namespace {
// the checks of both transform entries; `in` / `out` are only compared
int ntt_check(const pa_fr_ntt_domain* d, int mode, const pa_fr* in, pa_fr* out, size_t batch) {
    if (!d) return fail(PA_ERR_INVALID_ARGUMENT, "null pointer");
    if (mode < PA_NTT_FORWARD || mode > PA_NTT_COSET_INVERSE) return fail(PA_ERR_INVALID_ARGUMENT, "unknown NTT mode");
    if (batch == 0) return PA_OK;
    if (!in || !out) return fail(PA_ERR_INVALID_ARGUMENT, "null pointer");
    if (!pa::ntt_batch_fits(d->layout, batch))
        return fail(PA_ERR_INVALID_ARGUMENT, "NTT batch too large (a pass of the domain's tile log would exceed a grid)");
    const uintptr_t a = (uintptr_t)in, b = (uintptr_t)out;
    const size_t bytes = (batch << d->layout.log_n) * sizeof(pa_fr);
    if (a != b && a < b + bytes && b < a + bytes)
        return fail(PA_ERR_INVALID_ARGUMENT, "NTT input and output overlap partially");
    return PA_OK;
}
}  // namespace

int pa_fr_ntt_device(const pa_fr_ntt_domain* d, int mode, const pa_fr* in, pa_fr* out, size_t batch, void* workspace,
                     size_t workspace_bytes, void* stream) {
    if (int rc = ntt_check(d, mode, in, out, batch)) return rc;
    if (batch == 0) return PA_OK;
    const size_t need = pa::ntt_workspace_bytes(d->layout, batch);
    if (need && (!workspace || workspace_bytes < need))
        return fail(PA_ERR_INVALID_ARGUMENT, "workspace smaller than pa_fr_ntt_workspace_bytes");
    int dev = 0;
    PA_TRY(hipStreamGetDevice((hipStream_t)stream, &dev), "stream device");
    if (dev != d->dev) return fail(PA_ERR_INVALID_ARGUMENT, "stream is on another device than the NTT domain");
    PA_TRY(pa::launch_ntt(d->layout, d->tables, mode, (const uint64_t*)in, (uint64_t*)out, batch, workspace,
                          (hipStream_t)stream),
           "kernel launch");
    return PA_OK;
}
int pa_fr_ntt(const pa_fr_ntt_domain* d, int mode, const pa_fr* in, pa_fr* out, size_t batch) {
    if (int rc = ntt_check(d, mode, in, out, batch)) return rc;
    if (batch == 0) return PA_OK;
    DevBuf da, dws;
    int rc;
    const size_t bytes = (batch << d->layout.log_n) * sizeof(pa_fr);
    if ((rc = upload(da, in, bytes))) return rc;
    const size_t ws = pa::ntt_workspace_bytes(d->layout, batch);
    PA_TRY(dws.alloc(ws), "device scratch");
    if ((rc = pa_fr_ntt_device(d, mode, da.as<pa_fr>(), da.as<pa_fr>(), batch, dws.p, ws, call_stream()))) return rc;
    PA_TRY(call_sync(), "kernel execution");
    return download(out, da, bytes);
}

// the quotient h = (A B - C) / Z of a proof over the domain (launch_ntt_quotient)
size_t pa_fr_ntt_quotient_workspace_bytes(const pa_fr_ntt_domain* d, size_t batch) {
    return d && pa::ntt_quotient_fits(d->layout, batch) ? pa::ntt_quotient_workspace_bytes(d->layout, batch) : 0;
}

namespace {
// the checks of both quotient entries; the pointers are only compared
int ntt_quotient_check(const pa_fr_ntt_domain* d, const pa_fr* a, const pa_fr* b, const pa_fr* c, pa_fr* out,
                       size_t batch) {
    if (!d) return fail(PA_ERR_INVALID_ARGUMENT, "null pointer");
    if (batch == 0) return PA_OK;
    if (!a || !b || !c || !out) return fail(PA_ERR_INVALID_ARGUMENT, "null pointer");
    if (!pa::ntt_quotient_fits(d->layout, batch))
        return fail(PA_ERR_INVALID_ARGUMENT,
                    "NTT quotient batch too large (a pass over a, b and c would exceed a grid): split the batch");
    const size_t bytes = (batch << d->layout.log_n) * sizeof(pa_fr);
    const uintptr_t o = (uintptr_t)out;
    const pa_fr* ins[3] = {a, b, c};
    for (const pa_fr* in : ins) {
        const uintptr_t i = (uintptr_t)in;
        if (i != o && i < o + bytes && o < i + bytes)
            return fail(PA_ERR_INVALID_ARGUMENT, "NTT quotient output overlaps an input partially");
    }
    return PA_OK;
}
}  // namespace

int pa_fr_ntt_quotient_device(const pa_fr_ntt_domain* d, const pa_fr* a, const pa_fr* b, const pa_fr* c, pa_fr* out,
                              size_t batch, void* workspace, size_t workspace_bytes, void* stream) {
    if (int rc = ntt_quotient_check(d, a, b, c, out, batch)) return rc;
    if (batch == 0) return PA_OK;
    const size_t need = pa::ntt_quotient_workspace_bytes(d->layout, batch);
    if (need && (!workspace || workspace_bytes < need))
        return fail(PA_ERR_INVALID_ARGUMENT, "workspace smaller than pa_fr_ntt_quotient_workspace_bytes");
    int dev = 0;
    PA_TRY(hipStreamGetDevice((hipStream_t)stream, &dev), "stream device");
    if (dev != d->dev) return fail(PA_ERR_INVALID_ARGUMENT, "stream is on another device than the NTT domain");
    PA_TRY(pa::launch_ntt_quotient(d->layout, d->tables, (const uint64_t*)a, (const uint64_t*)b, (const uint64_t*)c,
                                   (uint64_t*)out, batch, workspace, (hipStream_t)stream),
           "kernel launch");
    return PA_OK;
}
int pa_fr_ntt_quotient(const pa_fr_ntt_domain* d, const pa_fr* a, const pa_fr* b, const pa_fr* c, pa_fr* out,
                       size_t batch) {
    if (int rc = ntt_quotient_check(d, a, b, c, out, batch)) return rc;
    if (batch == 0) return PA_OK;
    DevBuf da, db, dc, dws;
    int rc;
    const size_t bytes = (batch << d->layout.log_n) * sizeof(pa_fr);
    if ((rc = upload(da, a, bytes))) return rc;
    if ((rc = upload(db, b, bytes))) return rc;
    if ((rc = upload(dc, c, bytes))) return rc;
    const size_t ws = pa::ntt_quotient_workspace_bytes(d->layout, batch);
    PA_TRY(dws.alloc(ws), "device scratch");
    if ((rc = pa_fr_ntt_quotient_device(d, da.as<pa_fr>(), db.as<pa_fr>(), dc.as<pa_fr>(), da.as<pa_fr>(), batch, dws.p,
                                        ws, call_stream())))
        return rc;
    PA_TRY(call_sync(), "kernel execution");
    return download(out, da, bytes);
}

// ---- R1CS matrices on the device (kernels_r1cs.hip) ----
// The object owns one allocation on one device: the chunked image of the three
// matrices (launch_groth16.h).
struct pa_r1cs {
    int dev = 0;
    void* image = nullptr;
    pa::R1csDev d{};
};

namespace {
// r, 4 x u64 LE (fr.rs:4-10)
const uint64_t kFrModulus[4] = {0xffffffff00000001ull, 0x53bda402fffe5bfeull, 0x3339d80809a1d805ull,
                                0x73eda753299d7d48ull};
bool fr_below_r(const uint64_t* v) {
    for (int i = 3; i >= 0; i--)
        if (v[i] != kFrModulus[i]) return v[i] < kFrModulus[i];
    return false;
}
// 0, or the code of what is wrong with one host CSR matrix
int r1cs_csr_check(const pa_fr_csr* m, size_t n_rows, size_t n_cols) {
    if (!m) return fail(PA_ERR_INVALID_ARGUMENT, "null pointer");
    if (!m->row_ptr) return fail(PA_ERR_INVALID_ARGUMENT, "null pointer");
    if (m->row_ptr[0] != 0) return fail(PA_ERR_INVALID_ARGUMENT, "R1CS row_ptr must start at 0");
    for (size_t r = 0; r < n_rows; r++)
        if (m->row_ptr[r + 1] < m->row_ptr[r]) return fail(PA_ERR_INVALID_ARGUMENT, "R1CS row_ptr decreases");
    const uint64_t nnz = m->row_ptr[n_rows];
    if (nnz >> 32) return fail(PA_ERR_INVALID_ARGUMENT, "R1CS matrices support nnz < 2^32");
    if (nnz && (!m->col || !m->val)) return fail(PA_ERR_INVALID_ARGUMENT, "null pointer");
    for (uint64_t t = 0; t < nnz; t++) {
        if (m->col[t] >= n_cols) return fail(PA_ERR_INVALID_ARGUMENT, "R1CS column index >= n_cols");
        if (!fr_below_r(m->val[t].l)) return fail(PA_ERR_INVALID_ARGUMENT, "R1CS coefficient >= r");
    }
    return PA_OK;
}
size_t align256(size_t v) { return (v + 255) & ~(size_t)255; }

// the chunked image of three validated CSR matrices of n_rows x n_cols on the current device, copied and waited for
int r1cs_image_create(const pa::R1csCsr csr[3], size_t n_rows, size_t n_cols, pa_r1cs** out) {
    pa::R1csImage img;
    pa::r1cs_build(csr, n_rows, img);
    const pa::R1csDevLayout lay = pa::r1cs_dev_layout(img);
    pa_r1cs* r = new pa_r1cs;
    hipError_t e = hipGetDevice(&r->dev);
    if (e == hipSuccess) e = hipMalloc(&r->image, lay.bytes ? lay.bytes : 256);
    uint8_t* base = static_cast<uint8_t*>(r->image);
    hipStream_t s = call_stream();
    auto put = [&](size_t off, const void* src, size_t bytes) {
        if (e == hipSuccess && bytes) e = hipMemcpyAsync(base + off, src, bytes, hipMemcpyHostToDevice, s);
    };
    put(lay.val, img.val.data(), img.val.size() * 8);
    put(lay.col, img.col.data(), img.col.size() * 4);
    put(lay.slab_off, img.slab_off.data(), img.slab_off.size() * 8);
    put(lay.slab_len, img.slab_len.data(), img.slab_len.size() * 4);
    put(lay.chunk_len, img.chunk_len.data(), img.chunk_len.size() * 4);
    put(lay.chunk_dst, img.chunk_dst.data(), img.chunk_dst.size() * 4);
    put(lay.fold, img.fold.data(), img.fold.size() * 4);
    if (e == hipSuccess) e = call_sync();   // the image's host vectors go out of scope below
    if (e != hipSuccess) {
        (void)hipStreamSynchronize(s);
        if (r->image) (void)hipFree(r->image);
        delete r;
        return fail(hip_code(e), "create R1CS image", e);
    }
    r->d = pa::R1csDev{r->image, lay, img.slabs, n_rows, n_cols, img.n_partial, img.n_fold};
    *out = r;
    return PA_OK;
}
}  // namespace

int pa_r1cs_create(const pa_fr_csr* a, const pa_fr_csr* b, const pa_fr_csr* c, size_t n_rows, size_t n_cols,
                   pa_r1cs** out) {
    if (!out) return fail(PA_ERR_INVALID_ARGUMENT, "null pointer");
    *out = nullptr;
    if (n_rows > ((size_t)1 << pa::kNttMaxLogN))
        return fail(PA_ERR_INVALID_ARGUMENT, "R1CS systems support n_rows <= 2^28");
    const pa_fr_csr* ms[3] = {a, b, c};
    pa::R1csCsr csr[3];
    for (int i = 0; i < 3; i++) {
        if (int rc = r1cs_csr_check(ms[i], n_rows, n_cols)) return rc;
        csr[i] = {ms[i]->row_ptr, ms[i]->col, (const uint64_t*)ms[i]->val};
    }
    return r1cs_image_create(csr, n_rows, n_cols, out);
}
void pa_r1cs_free(pa_r1cs* r) {
    if (!r) return;
    if (r->image) (void)hipFree(r->image);
    delete r;
}
size_t pa_r1cs_rows(const pa_r1cs* r) { return r ? r->d.n_rows : 0; }
size_t pa_r1cs_cols(const pa_r1cs* r) { return r ? r->d.n_cols : 0; }
size_t pa_r1cs_bytes(const pa_r1cs* r) { return r ? r->d.layout.bytes : 0; }
size_t pa_r1cs_chunk_len(void) { return pa::kR1csChunkLen; }
size_t pa_r1cs_eval_workspace_bytes(const pa_r1cs* r, size_t k) { return r ? k * r->d.n_partial * sizeof(pa_fr) : 0; }

namespace {
// the checks of both evaluation entries that need no pointer
int r1cs_eval_check(const pa_r1cs* r, unsigned log_n) {
    if (!r) return fail(PA_ERR_INVALID_ARGUMENT, "null pointer");
    if (log_n > pa::kNttMaxLogN) return fail(PA_ERR_INVALID_ARGUMENT, "R1CS evaluation supports log_n <= 28");
    if (((size_t)1 << log_n) < r->d.n_rows)
        return fail(PA_ERR_INVALID_ARGUMENT, "2^log_n is smaller than the R1CS system's rows");
    return PA_OK;
}
}  // namespace

int pa_r1cs_eval_device(const pa_r1cs* r, const pa_fr* witness, size_t k, unsigned log_n, pa_fr* a, pa_fr* b, pa_fr* c,
                        void* workspace, size_t workspace_bytes, void* stream) {
    if (int rc = r1cs_eval_check(r, log_n)) return rc;
    if (k == 0) return PA_OK;
    if (!a || !b || !c || (r->d.n_cols && !witness)) return fail(PA_ERR_INVALID_ARGUMENT, "null pointer");
    const size_t need = pa_r1cs_eval_workspace_bytes(r, k);
    if (need && (!workspace || workspace_bytes < need))
        return fail(PA_ERR_INVALID_ARGUMENT, "workspace smaller than pa_r1cs_eval_workspace_bytes");
    int dev = 0;
    PA_TRY(hipStreamGetDevice((hipStream_t)stream, &dev), "stream device");
    if (dev != r->dev) return fail(PA_ERR_INVALID_ARGUMENT, "stream is on another device than the R1CS object");
    PA_TRY(pa::launch_r1cs_eval(r->d, (const uint64_t*)witness, k, log_n, (uint64_t*)a, (uint64_t*)b, (uint64_t*)c,
                                need ? workspace : nullptr, (hipStream_t)stream),
           "kernel launch");
    return PA_OK;
}
int pa_r1cs_eval(const pa_r1cs* r, const pa_fr* witness, size_t k, unsigned log_n, pa_fr* a, pa_fr* b, pa_fr* c) {
    if (int rc = r1cs_eval_check(r, log_n)) return rc;
    if (k == 0) return PA_OK;
    if (!a || !b || !c || (r->d.n_cols && !witness)) return fail(PA_ERR_INVALID_ARGUMENT, "null pointer");
    DevBuf dw, dabc, dws;
    int rc;
    const size_t bytes = (k << log_n) * sizeof(pa_fr);
    if ((rc = upload(dw, witness, k * r->d.n_cols * sizeof(pa_fr)))) return rc;
    PA_TRY(dabc.alloc(3 * bytes), "device scratch");
    const size_t ws = pa_r1cs_eval_workspace_bytes(r, k);
    PA_TRY(dws.alloc(ws), "device scratch");
    pa_fr* da = dabc.as<pa_fr>();
    pa_fr *db = da + (k << log_n), *dc = db + (k << log_n);
    if ((rc = pa_r1cs_eval_device(r, dw.as<pa_fr>(), k, log_n, da, db, dc, dws.p, ws, call_stream()))) return rc;
    PA_TRY(call_sync(), "kernel execution");
    pa_fr* outs[3] = {a, b, c};
    for (int i = 0; i < 3; i++) {
        PA_TRY(hipMemcpyAsync(outs[i], da + i * (k << log_n), bytes, hipMemcpyDeviceToHost, dabc.ctx->compute),
               "D2H copy");
    }
    PA_TRY(call_sync(), "D2H copy");
    return PA_OK;
}

// ---- Groth16 prover: the proving key as one object, and witness -> proof (kernels_groth16.hip) ----
struct pa_groth16_pk {
    int dev = 0;
    unsigned log_n = 0;
    size_t n_vars = 0, n_public = 0, h_len = 0;
    pa_g1_msm_bases *a = nullptr, *b1 = nullptr, *l = nullptr, *h = nullptr;
    pa_g2_msm_bases* b2 = nullptr;
    uint64_t* consts = nullptr;   // alpha_g1, beta_g1, delta_g1, beta_g2, delta_g2, the 2^i delta tables (launch_groth16.h)
};

void pa_groth16_pk_free(pa_groth16_pk* pk) {
    if (!pk) return;
    (void)pa_g1_msm_bases_free(pk->a);
    (void)pa_g1_msm_bases_free(pk->b1);
    (void)pa_g1_msm_bases_free(pk->l);
    (void)pa_g1_msm_bases_free(pk->h);
    (void)pa_g2_msm_bases_free(pk->b2);
    if (pk->consts) (void)hipFree(pk->consts);
    delete pk;
}

int pa_groth16_pk_create(const pa_groth16_key* key, unsigned log_n, pa_groth16_pk** out) {
    if (!out) return fail(PA_ERR_INVALID_ARGUMENT, "null pointer");
    *out = nullptr;
    if (!key) return fail(PA_ERR_INVALID_ARGUMENT, "null pointer");
    if (log_n > pa::kNttMaxLogN) return fail(PA_ERR_INVALID_ARGUMENT, "Groth16 keys support log_n <= 28");
    const size_t n = (size_t)1 << log_n, nv = key->n_vars, np = key->n_public;
    if (np > nv) return fail(PA_ERR_INVALID_ARGUMENT, "n_public exceeds n_vars");
    if (key->h_len > n) return fail(PA_ERR_INVALID_ARGUMENT, "h_len exceeds 2^log_n");
    if (nv >= pa::kMsmPreparedMax) return fail(PA_ERR_INVALID_ARGUMENT, "prepared multiexp bases support n < 2^30");
    if ((nv && (!key->a_query || !key->b_g1_query || !key->b_g2_query)) || (nv > np && !key->l_query) ||
        (key->h_len && !key->h_query))
        return fail(PA_ERR_INVALID_ARGUMENT, "null pointer");
    // the point at infinity as into_affine writes it: (0, 1), flag set
    pa_g1_affine inf;
    memset(&inf, 0, sizeof inf);
    const uint64_t fq_one[6] = {0x760900000002fffdull, 0xebf4000bc40c0002ull, 0x5f48985753c758baull,
                                0x77ce585370525745ull, 0x5c071a97a256ec6dull, 0x15f65ec3fa80e493ull};
    memcpy(inf.y.l, fq_one, sizeof fq_one);
    inf.infinity = 1;
    std::vector<pa_g1_affine> lq(nv, inf), hq(n, inf);
    if (nv > np) memcpy(lq.data() + np, key->l_query, (nv - np) * sizeof(pa_g1_affine));
    if (key->h_len) memcpy(hq.data(), key->h_query, key->h_len * sizeof(pa_g1_affine));

    pa_groth16_pk* pk = new pa_groth16_pk;
    pk->log_n = log_n;
    pk->n_vars = nv;
    pk->n_public = np;
    pk->h_len = key->h_len;
    int rc = PA_OK;
    hipError_t e = hipGetDevice(&pk->dev);
    if (e != hipSuccess) rc = fail(hip_code(e), "current device", e);
    if (!rc) rc = pa_g1_msm_bases_prepare(key->a_query, nv, &pk->a);
    if (!rc) rc = pa_g1_msm_bases_prepare(key->b_g1_query, nv, &pk->b1);
    if (!rc) rc = pa_g2_msm_bases_prepare(key->b_g2_query, nv, &pk->b2);
    if (!rc) rc = pa_g1_msm_bases_prepare(lq.data(), nv, &pk->l);
    if (!rc) rc = pa_g1_msm_bases_prepare(hq.data(), n, &pk->h);
    if (!rc) {
        uint64_t host[pa::kGroth16ConstWords];
        memcpy(host, &key->alpha_g1, 13 * 8);
        memcpy(host + 13, &key->beta_g1, 13 * 8);
        memcpy(host + 26, &key->delta_g1, 13 * 8);
        memcpy(host + 39, &key->beta_g2, 25 * 8);
        memcpy(host + 64, &key->delta_g2, 25 * 8);
        // only the flag byte of a record's last word is defined
        for (size_t w : {12, 25, 38, 63, 88}) host[w] &= 0xff;
        e = hipMalloc((void**)&pk->consts, pa::kGroth16KeyWords * sizeof(uint64_t));
        if (e == hipSuccess) e = hipMemcpy(pk->consts, host, sizeof host, hipMemcpyHostToDevice);
        if (e == hipSuccess) e = pa::launch_groth16_tables(pk->consts, call_stream());
        if (e == hipSuccess) e = call_sync();
        if (e != hipSuccess) rc = fail(hip_code(e), "create Groth16 key", e);
    }
    if (rc) {
        pa_groth16_pk_free(pk);
        return rc;
    }
    *out = pk;
    return PA_OK;
}
int pa_groth16_pk_in_subgroup(const pa_groth16_pk* pk) {
    return pk && pk->a->in_subgroup && pk->b1->in_subgroup && pk->b2->in_subgroup && pk->l->in_subgroup &&
                   pk->h->in_subgroup
               ? 1
               : 0;
}

namespace {
// the prove call's workspace: a, b, c (the quotient overwrites a), the five
// sums, and one region that the evaluation, the quotient and the multiexps use
// in turn.  bytes = 0: a batch that one of the steps refuses.
struct ProveLayout {
    size_t abc, sums, shared, shared_bytes, msm_bytes[5], bytes;
};
ProveLayout prove_layout(const pa_groth16_pk* pk, const pa_r1cs* r, size_t k) {
    ProveLayout p{};
    const size_t n = (size_t)1 << pk->log_n, nv = pk->n_vars;
    // the quotient's workspace for any tile log: 6 arrays of k polynomials cover one pass and several
    const pa::NttLayout dflt = pa::ntt_layout(pk->log_n, pa::kNttDefaultTileLog);
    if (k && !pa::ntt_quotient_fits(dflt, k)) return p;
    const MsmBasesObj* bases[5] = {pk->a, pk->b1, pk->l, pk->h, pk->b2};
    size_t shared = pa_r1cs_eval_workspace_bytes(r, k);
    const size_t quot = pk->log_n ? 6 * k * n * sizeof(pa_fr) : 0;
    shared = shared > quot ? shared : quot;
    for (int i = 0; i < 5; i++) {
        const int g = i == 4 ? 2 : 1;
        const size_t m = i == 3 ? n : nv;
        const bool glv = bases[i]->in_subgroup != 0;
        if (k && !pa::msm_prepared_batch_fits(m, k, glv, g)) return p;
        p.msm_bytes[i] = m && k ? pa::msm_prepared_batch_workspace_bytes(m, k, glv, g) : 0;
        shared = shared > p.msm_bytes[i] ? shared : p.msm_bytes[i];
    }
    size_t o = 0;
    p.abc = o;    o = align256(o + 3 * k * n * sizeof(pa_fr));
    p.sums = o;   o = align256(o + k * (4 * sizeof(pa_g1) + sizeof(pa_g2)));
    p.shared = o; o = align256(o + shared);
    p.shared_bytes = shared;
    p.bytes = o ? o : 256;
    return p;
}
// what both prove entries refuse before touching memory
int prove_check(const pa_groth16_pk* pk, const pa_r1cs* r, const pa_fr_ntt_domain* d, size_t k) {
    if (!pk || !r || !d) return fail(PA_ERR_INVALID_ARGUMENT, "null pointer");
    if (d->layout.log_n != pk->log_n)
        return fail(PA_ERR_INVALID_ARGUMENT, "the NTT domain's log_n differs from the Groth16 key's");
    if (r->d.n_cols != pk->n_vars)
        return fail(PA_ERR_INVALID_ARGUMENT, "the R1CS system's columns differ from the Groth16 key's n_vars");
    if (r->d.n_rows > ((size_t)1 << pk->log_n))
        return fail(PA_ERR_INVALID_ARGUMENT, "the R1CS system has more rows than the domain has points");
    if (r->dev != pk->dev || d->dev != pk->dev)
        return fail(PA_ERR_INVALID_ARGUMENT, "the Groth16 key, the R1CS object and the NTT domain are on different devices");
    if (k && (prove_layout(pk, r, k).bytes == 0 || !pa::ntt_quotient_fits(d->layout, k)))
        return fail(PA_ERR_INVALID_ARGUMENT,
                    "Groth16 batch over a multiexp's 32-bit item limit or the quotient's grid limit: split it");
    return PA_OK;
}
}  // namespace

size_t pa_groth16_prove_workspace_bytes(const pa_groth16_pk* pk, const pa_r1cs* r1cs, size_t k) {
    if (!pk || !r1cs || r1cs->d.n_cols != pk->n_vars || r1cs->d.n_rows > ((size_t)1 << pk->log_n)) return 0;
    return prove_layout(pk, r1cs, k).bytes;
}

int pa_groth16_prove_device(const pa_groth16_pk* pk, const pa_r1cs* r1cs, const pa_fr_ntt_domain* d,
                            const pa_fr* witness, const pa_fr* dev_r, const pa_fr* dev_s, size_t k,
                            pa_groth16_proof* proofs, void* workspace, size_t workspace_bytes, void* stream) {
    if (int rc = prove_check(pk, r1cs, d, k)) return rc;
    if (k == 0) return PA_OK;
    if (!dev_r || !dev_s || !proofs || !workspace || (pk->n_vars && !witness))
        return fail(PA_ERR_INVALID_ARGUMENT, "null pointer");
    const ProveLayout p = prove_layout(pk, r1cs, k);
    if (workspace_bytes < p.bytes || pa::ntt_quotient_workspace_bytes(d->layout, k) > p.shared_bytes)
        return fail(PA_ERR_INVALID_ARGUMENT, "workspace smaller than pa_groth16_prove_workspace_bytes");
    int dev = 0;
    PA_TRY(hipStreamGetDevice((hipStream_t)stream, &dev), "stream device");
    if (dev != pk->dev) return fail(PA_ERR_INVALID_ARGUMENT, "stream is on another device than the Groth16 key");
    const size_t n = (size_t)1 << pk->log_n, nv = pk->n_vars;
    uint8_t* ws = static_cast<uint8_t*>(workspace);
    pa_fr* a = reinterpret_cast<pa_fr*>(ws + p.abc);
    pa_fr *b = a + k * n, *c = b + k * n;
    pa_g1* sums = reinterpret_cast<pa_g1*>(ws + p.sums);   // S_a, S_b1, S_l, S_h (k each), then S_b2
    pa_g2* sum_b2 = reinterpret_cast<pa_g2*>(sums + 4 * k);
    void* shared = ws + p.shared;
    int rc;
    if ((rc = pa_r1cs_eval_device(r1cs, witness, k, pk->log_n, a, b, c, shared, p.shared_bytes, stream))) return rc;
    if ((rc = pa_fr_ntt_quotient_device(d, a, b, c, a, k, shared, p.shared_bytes, stream))) return rc;
    const unsigned mont = PA_MSM_SCALARS_MONTGOMERY;
    if ((rc = pa_g1_multiexp_prepared_batch_device(pk->a, witness, nv, k, mont, sums, shared, p.shared_bytes, stream)))
        return rc;
    if ((rc = pa_g1_multiexp_prepared_batch_device(pk->b1, witness, nv, k, mont, sums + k, shared, p.shared_bytes,
                                                   stream)))
        return rc;
    if ((rc = pa_g1_multiexp_prepared_batch_device(pk->l, witness, nv, k, mont, sums + 2 * k, shared, p.shared_bytes,
                                                   stream)))
        return rc;
    if ((rc = pa_g1_multiexp_prepared_batch_device(pk->h, a, n, k, mont, sums + 3 * k, shared, p.shared_bytes, stream)))
        return rc;
    if ((rc = pa_g2_multiexp_prepared_batch_device(pk->b2, witness, nv, k, mont, sum_b2, shared, p.shared_bytes,
                                                   stream)))
        return rc;
    PA_TRY(pa::launch_groth16_assemble(pk->consts, (const uint64_t*)sums, (const uint64_t*)(sums + k),
                                       (const uint64_t*)(sums + 2 * k), (const uint64_t*)(sums + 3 * k),
                                       (const uint64_t*)sum_b2, (const uint64_t*)dev_r, (const uint64_t*)dev_s, k,
                                       (uint64_t*)proofs, (hipStream_t)stream),
           "kernel launch");
    return PA_OK;
}

int pa_groth16_prove(const pa_groth16_pk* pk, const pa_r1cs* r1cs, const pa_fr_ntt_domain* d, const pa_fr* witness,
                     const pa_fr* host_r, const pa_fr* host_s, size_t k, pa_groth16_proof* proofs) {
    if (int rc = prove_check(pk, r1cs, d, k)) return rc;
    if (k == 0) return PA_OK;
    if (!host_r || !host_s || !proofs || (pk->n_vars && !witness)) return fail(PA_ERR_INVALID_ARGUMENT, "null pointer");
    DevBuf dw, dr, ds, dout, dws;
    int rc;
    if ((rc = upload(dw, witness, k * pk->n_vars * sizeof(pa_fr)))) return rc;
    if ((rc = upload(dr, host_r, k * sizeof(pa_fr)))) return rc;
    if ((rc = upload(ds, host_s, k * sizeof(pa_fr)))) return rc;
    PA_TRY(dout.alloc(k * sizeof(pa_groth16_proof)), "device scratch");
    const size_t ws = prove_layout(pk, r1cs, k).bytes;
    PA_TRY(dws.alloc(ws), "device scratch");
    if ((rc = pa_groth16_prove_device(pk, r1cs, d, dw.as<pa_fr>(), dr.as<pa_fr>(), ds.as<pa_fr>(), k,
                                      dout.as<pa_groth16_proof>(), dws.p, ws, call_stream())))
        return rc;
    PA_TRY(call_sync(), "kernel execution");
    return download(proofs, dout, k * sizeof(pa_groth16_proof));
}

// ---- Groth16 parameter generation: trapdoor -> proving and verifying key (kernels_groth16_setup.hip) ----
// The circuit object is the pa_r1cs image of the transposed matrices: rows = variables, columns = constraints.
struct pa_groth16_circuit {
    pa_r1cs* t = nullptr;
    size_t n_rows = 0, n_cols = 0, n_public = 0;
};

int pa_groth16_circuit_create(const pa_fr_csr* a, const pa_fr_csr* b, const pa_fr_csr* c, size_t n_rows, size_t n_cols,
                              size_t n_public, pa_groth16_circuit** out) {
    if (!out) return fail(PA_ERR_INVALID_ARGUMENT, "null pointer");
    *out = nullptr;
    if (n_rows > ((size_t)1 << pa::kNttMaxLogN))
        return fail(PA_ERR_INVALID_ARGUMENT, "R1CS systems support n_rows <= 2^28");
    if (n_cols > ((size_t)1 << pa::kNttMaxLogN))
        return fail(PA_ERR_INVALID_ARGUMENT, "Groth16 circuits support n_cols <= 2^28");
    if (n_public > n_cols) return fail(PA_ERR_INVALID_ARGUMENT, "n_public exceeds n_cols");
    const pa_fr_csr* ms[3] = {a, b, c};
    pa::R1csCsrOwned tr[3];
    pa::R1csCsr csr[3];
    for (int i = 0; i < 3; i++) {
        if (int rc = r1cs_csr_check(ms[i], n_rows, n_cols)) return rc;
        pa::r1cs_transpose({ms[i]->row_ptr, ms[i]->col, (const uint64_t*)ms[i]->val}, n_rows, n_cols, tr[i]);
        csr[i] = {tr[i].row_ptr.data(), tr[i].col.data(), tr[i].val.data()};
    }
    pa_r1cs* t = nullptr;
    if (int rc = r1cs_image_create(csr, n_cols, n_rows, &t)) return rc;
    pa_groth16_circuit* ci = new pa_groth16_circuit;
    ci->t = t;
    ci->n_rows = n_rows;
    ci->n_cols = n_cols;
    ci->n_public = n_public;
    *out = ci;
    return PA_OK;
}
void pa_groth16_circuit_free(pa_groth16_circuit* ci) {
    if (!ci) return;
    pa_r1cs_free(ci->t);
    delete ci;
}
size_t pa_groth16_circuit_rows(const pa_groth16_circuit* ci) { return ci ? ci->n_rows : 0; }
size_t pa_groth16_circuit_cols(const pa_groth16_circuit* ci) { return ci ? ci->n_cols : 0; }
size_t pa_groth16_circuit_n_public(const pa_groth16_circuit* ci) { return ci ? ci->n_public : 0; }
size_t pa_groth16_circuit_bytes(const pa_groth16_circuit* ci) { return ci ? pa_r1cs_bytes(ci->t) : 0; }
size_t pa_groth16_generate_g1_len(const pa_groth16_circuit* ci, unsigned log_n) {
    return ci && log_n <= pa::kNttMaxLogN ? 3 * ci->n_cols + ((size_t)1 << log_n) + 2 : 0;
}
size_t pa_groth16_generate_g2_len(const pa_groth16_circuit* ci) { return ci ? ci->n_cols + 3 : 0; }

namespace {
// Host Fr for the handful of trapdoor constants of a call: Montgomery rows of 4 x u64 below r (fr.rs:438-572).
const uint64_t kFrOne[4] = {0x00000001fffffffeull, 0x5884b7fa00034802ull, 0x998c4fefecbc4ff5ull,
                            0x1824b159acc5056full};
void fr_host_mul(uint64_t* out, const uint64_t* a, const uint64_t* b) {
    typedef unsigned __int128 u128;
    const uint64_t inv = 0xfffffffeffffffffull;   // -r^-1 mod 2^64 (fr.rs:37)
    uint64_t t[6] = {0, 0, 0, 0, 0, 0};
    for (int i = 0; i < 4; i++) {
        u128 c = 0;
        for (int j = 0; j < 4; j++) {
            c += (u128)a[j] * b[i] + t[j];
            t[j] = (uint64_t)c;
            c >>= 64;
        }
        c += t[4];
        t[4] = (uint64_t)c;
        t[5] = (uint64_t)(c >> 64);
        const uint64_t m = t[0] * inv;
        c = ((u128)m * kFrModulus[0] + t[0]) >> 64;
        for (int j = 1; j < 4; j++) {
            c += (u128)m * kFrModulus[j] + t[j];
            t[j - 1] = (uint64_t)c;
            c >>= 64;
        }
        c += t[4];
        t[3] = (uint64_t)c;
        t[4] = t[5] + (uint64_t)(c >> 64);
    }
    // below 2 r < 2^256: t[4] is zero
    if (!fr_below_r(t)) {
        u128 br = 0;
        for (int j = 0; j < 4; j++) {
            const u128 d = (u128)t[j] - kFrModulus[j] - (uint64_t)br;
            t[j] = (uint64_t)d;
            br = (d >> 64) & 1;
        }
    }
    memcpy(out, t, 32);
}
void fr_host_sub_one(uint64_t* out, const uint64_t* a) {   // a - 1
    typedef unsigned __int128 u128;
    uint64_t t[4];
    u128 br = 0;
    for (int j = 0; j < 4; j++) {
        const u128 d = (u128)a[j] - kFrOne[j] - (uint64_t)br;
        t[j] = (uint64_t)d;
        br = (d >> 64) & 1;
    }
    if (br) {
        u128 c = 0;
        for (int j = 0; j < 4; j++) {
            c += (u128)t[j] + kFrModulus[j];
            t[j] = (uint64_t)c;
            c >>= 64;
        }
    }
    memcpy(out, t, 32);
}
void fr_host_inv(uint64_t* out, const uint64_t* a) {   // a^(r - 2)
    const uint64_t e[4] = {0xfffffffeffffffffull, 0x53bda402fffe5bfeull, 0x3339d80809a1d805ull, 0x73eda753299d7d48ull};
    uint64_t acc[4];
    memcpy(acc, kFrOne, 32);
    for (int w = 3; w >= 0; w--)
        for (int bit = 63; bit >= 0; bit--) {
            fr_host_mul(acc, acc, acc);
            if ((e[w] >> bit) & 1) fr_host_mul(acc, acc, a);
        }
    memcpy(out, acc, 32);
}
bool fr_host_is_zero(const uint64_t* a) { return !(a[0] | a[1] | a[2] | a[3]); }

// the call's workspace: byte offsets, every region a multiple of 256
struct GenLayout {
    size_t pow, lag, uvw, partial, ntt, s1, s2, base1, base2, jac1, jac2, tab1, cws1, tab2, cws2, fr_bytes, bytes;
};
GenLayout gen_layout(const pa_groth16_circuit* ci, unsigned log_n) {
    GenLayout g{};
    const size_t n = (size_t)1 << log_n, nv = ci->n_cols, n1 = 3 * nv + n + 2, n2 = nv + 3;
    size_t o = 0;
    g.pow = o;      o = align256(o + n * sizeof(pa_fr));
    g.lag = o;      o = align256(o + n * sizeof(pa_fr));
    g.uvw = o;      o = align256(o + 3 * nv * sizeof(pa_fr));
    g.partial = o;  o = align256(o + pa_r1cs_eval_workspace_bytes(ci->t, 1));
    g.ntt = o;      o = align256(o + n * sizeof(pa_fr));   // a transform of several passes, whatever the tile log
    g.fr_bytes = o;   // what the scalars entries use
    g.s1 = o;       o = align256(o + n1 * sizeof(pa_fr_repr));
    g.s2 = o;       o = align256(o + n2 * sizeof(pa_fr_repr));
    g.base1 = o;    o = align256(o + sizeof(pa_g1));
    g.base2 = o;    o = align256(o + sizeof(pa_g2));
    g.jac1 = o;     o = align256(o + n1 * sizeof(pa_g1));
    g.jac2 = o;     o = align256(o + n2 * sizeof(pa_g2));
    g.tab1 = o;     o = align256(o + 8 * pa::g1_comb_table_words());
    g.cws1 = o;     o = align256(o + 8 * pa::g1_comb_workspace_words());
    g.tab2 = o;     o = align256(o + 8 * pa::g2_comb_table_words());
    g.cws2 = o;     o = align256(o + 8 * pa::g2_comb_workspace_words());
    g.bytes = o;
    return g;
}

// what every generation entry refuses before touching memory; fills the kernels' constants
int gen_check(const pa_groth16_circuit* ci, const pa_fr_ntt_domain* d, const pa_groth16_trapdoor* td,
              pa::Groth16SetupConsts* k) {
    if (!td) return fail(PA_ERR_INVALID_ARGUMENT, "null pointer");
    // the trapdoor first: it is host memory and needs no object to be judged
    const pa_fr* vals[5] = {&td->tau, &td->alpha, &td->beta, &td->gamma, &td->delta};
    for (const pa_fr* v : vals)
        if (!fr_below_r(v->l)) return fail(PA_ERR_INVALID_ARGUMENT, "trapdoor value >= r");
    if (fr_host_is_zero(td->gamma.l) || fr_host_is_zero(td->delta.l))
        return fail(PA_ERR_INVALID_ARGUMENT, "gamma and delta must not be zero");
    if (!ci || !d) return fail(PA_ERR_INVALID_ARGUMENT, "null pointer");
    const unsigned log_n = d->layout.log_n;
    if (((size_t)1 << log_n) < ci->n_rows)
        return fail(PA_ERR_INVALID_ARGUMENT, "2^log_n is smaller than the circuit's rows");
    if (ci->t->dev != d->dev)
        return fail(PA_ERR_INVALID_ARGUMENT, "the circuit and the NTT domain are on different devices");
    uint64_t p[4], tau_n[4];
    memcpy(p, td->tau.l, 32);
    for (unsigned b = 0; b <= 28; b++) {   // p = tau^(2^b)
        if (b == log_n) memcpy(tau_n, p, 32);
        if (b < 28) memcpy(k->tau_pow2[b], p, 32);
        fr_host_mul(p, p, p);
    }
    memcpy(k->alpha, td->alpha.l, 32);
    memcpy(k->beta, td->beta.l, 32);
    memcpy(k->gamma, td->gamma.l, 32);
    memcpy(k->delta, td->delta.l, 32);
    fr_host_inv(k->gamma_inv, td->gamma.l);
    fr_host_inv(k->delta_inv, td->delta.l);
    fr_host_sub_one(p, tau_n);
    fr_host_mul(k->h_scale, p, k->delta_inv);
    return PA_OK;
}

// powers, L, u v w and the scalar vectors on `stream`: g1 rows as Montgomery (g2 null) or both as FrRepr
int gen_scalars(const pa_groth16_circuit* ci, const pa_fr_ntt_domain* d, const pa::Groth16SetupConsts& k,
                const GenLayout& g, uint8_t* ws, bool montgomery, uint64_t* s1, uint64_t* s2, void* stream) {
    const unsigned log_n = d->layout.log_n;
    const size_t n = (size_t)1 << log_n, nv = ci->n_cols;
    hipStream_t s = (hipStream_t)stream;
    pa_fr* pow = reinterpret_cast<pa_fr*>(ws + g.pow);
    pa_fr* lag = reinterpret_cast<pa_fr*>(ws + g.lag);
    uint64_t* u = reinterpret_cast<uint64_t*>(ws + g.uvw);
    uint64_t *v = u + 4 * nv, *w = v + 4 * nv;
    PA_TRY(pa::launch_groth16_setup_powers(k, log_n, (uint64_t*)pow, s), "kernel launch");
    if (int rc = pa_fr_ntt_device(d, PA_NTT_INVERSE, pow, lag, 1, ws + g.ntt, n * sizeof(pa_fr), stream)) return rc;
    PA_TRY(pa::launch_r1cs_eval(ci->t->d, (const uint64_t*)lag, 1, nv, u, v, w,
                                ci->t->d.n_partial ? ws + g.partial : nullptr, s),
           "kernel launch");
    PA_TRY(pa::launch_groth16_setup_scalars(k, u, v, w, (const uint64_t*)pow, nv, ci->n_public, n, montgomery, s1, s2,
                                            s),
           "kernel launch");
    return PA_OK;
}
int gen_stream_check(const pa_groth16_circuit* ci, void* stream) {
    int dev = 0;
    PA_TRY(hipStreamGetDevice((hipStream_t)stream, &dev), "stream device");
    if (dev != ci->t->dev) return fail(PA_ERR_INVALID_ARGUMENT, "stream is on another device than the circuit");
    return PA_OK;
}
}  // namespace

size_t pa_groth16_generate_workspace_bytes(const pa_groth16_circuit* ci, unsigned log_n) {
    if (!ci || log_n > pa::kNttMaxLogN || ((size_t)1 << log_n) < ci->n_rows) return 0;
    return gen_layout(ci, log_n).bytes;
}

int pa_groth16_generate_scalars_device(const pa_groth16_circuit* ci, const pa_fr_ntt_domain* d,
                                       const pa_groth16_trapdoor* td, pa_fr* out, void* workspace,
                                       size_t workspace_bytes, void* stream) {
    pa::Groth16SetupConsts k;
    if (int rc = gen_check(ci, d, td, &k)) return rc;
    if (!out || !workspace) return fail(PA_ERR_INVALID_ARGUMENT, "null pointer");
    const GenLayout g = gen_layout(ci, d->layout.log_n);
    if (workspace_bytes < g.bytes)
        return fail(PA_ERR_INVALID_ARGUMENT, "workspace smaller than pa_groth16_generate_workspace_bytes");
    if (int rc = gen_stream_check(ci, stream)) return rc;
    return gen_scalars(ci, d, k, g, static_cast<uint8_t*>(workspace), true, (uint64_t*)out, nullptr, stream);
}

int pa_groth16_generate_device(const pa_groth16_circuit* ci, const pa_fr_ntt_domain* d, const pa_g1_affine* g1,
                               const pa_g2_affine* g2, const pa_groth16_trapdoor* td, pa_g1_affine* g1_out,
                               pa_g2_affine* g2_out, void* workspace, size_t workspace_bytes, void* stream) {
    pa::Groth16SetupConsts k;
    if (int rc = gen_check(ci, d, td, &k)) return rc;
    if (!g1 || !g2 || !g1_out || !g2_out || !workspace) return fail(PA_ERR_INVALID_ARGUMENT, "null pointer");
    const unsigned log_n = d->layout.log_n;
    const GenLayout g = gen_layout(ci, log_n);
    if (workspace_bytes < g.bytes)
        return fail(PA_ERR_INVALID_ARGUMENT, "workspace smaller than pa_groth16_generate_workspace_bytes");
    if (int rc = gen_stream_check(ci, stream)) return rc;
    const size_t n1 = pa_groth16_generate_g1_len(ci, log_n), n2 = pa_groth16_generate_g2_len(ci);
    uint8_t* ws = static_cast<uint8_t*>(workspace);
    hipStream_t s = (hipStream_t)stream;
    uint64_t *s1 = (uint64_t*)(ws + g.s1), *s2 = (uint64_t*)(ws + g.s2);
    pa_g1 *base1 = (pa_g1*)(ws + g.base1), *jac1 = (pa_g1*)(ws + g.jac1);
    pa_g2 *base2 = (pa_g2*)(ws + g.base2), *jac2 = (pa_g2*)(ws + g.jac2);
    int rc;
    if ((rc = gen_scalars(ci, d, k, g, ws, false, s1, s2, stream))) return rc;
    PA_TRY(pa::launch_group_op(1, pa::GROUP_FROM_AFFINE, (const uint64_t*)g1, nullptr, (uint64_t*)base1, 1, s),
           "kernel launch");
    PA_TRY(pa::launch_group_op(2, pa::GROUP_FROM_AFFINE, (const uint64_t*)g2, nullptr, (uint64_t*)base2, 1, s),
           "kernel launch");
    if ((rc = pa_g1_wnaf_fixed_base_device(base1, (const pa_fr_repr*)s1, jac1, n1, (uint64_t*)(ws + g.tab1),
                                           (uint64_t*)(ws + g.cws1), stream)))
        return rc;
    if ((rc = pa_g2_wnaf_fixed_base_device(base2, (const pa_fr_repr*)s2, jac2, n2, (uint64_t*)(ws + g.tab2),
                                           (uint64_t*)(ws + g.cws2), stream)))
        return rc;
    PA_TRY(pa::launch_g1_batch_normalize((uint64_t*)jac1, n1, s), "kernel launch");
    PA_TRY(pa::launch_groth16_setup_pack(1, (const uint64_t*)jac1, (uint64_t*)g1_out, n1, s), "kernel launch");
    PA_TRY(pa::launch_g2_batch_normalize((uint64_t*)jac2, n2, s), "kernel launch");
    PA_TRY(pa::launch_groth16_setup_pack(2, (const uint64_t*)jac2, (uint64_t*)g2_out, n2, s), "kernel launch");
    return PA_OK;
}

int pa_groth16_generate_scalars(const pa_groth16_circuit* ci, const pa_fr_ntt_domain* d, const pa_groth16_trapdoor* td,
                                pa_fr* out) {
    pa::Groth16SetupConsts k;
    if (int rc = gen_check(ci, d, td, &k)) return rc;
    if (!out) return fail(PA_ERR_INVALID_ARGUMENT, "null pointer");
    const size_t n1 = pa_groth16_generate_g1_len(ci, d->layout.log_n);
    const size_t ws = gen_layout(ci, d->layout.log_n).bytes;
    DevBuf dout, dws;
    PA_TRY(dout.alloc(n1 * sizeof(pa_fr)), "device scratch");
    PA_TRY(dws.alloc(ws), "device scratch");
    if (int rc = pa_groth16_generate_scalars_device(ci, d, td, dout.as<pa_fr>(), dws.p, ws, call_stream())) return rc;
    PA_TRY(call_sync(), "kernel execution");
    return download(out, dout, n1 * sizeof(pa_fr));
}

int pa_groth16_generate(const pa_groth16_circuit* ci, const pa_fr_ntt_domain* d, const pa_g1_affine* g1,
                        const pa_g2_affine* g2, const pa_groth16_trapdoor* td, pa_g1_affine* g1_out,
                        pa_g2_affine* g2_out) {
    pa::Groth16SetupConsts k;
    if (int rc = gen_check(ci, d, td, &k)) return rc;
    if (!g1 || !g2 || !g1_out || !g2_out) return fail(PA_ERR_INVALID_ARGUMENT, "null pointer");
    const size_t n1 = pa_groth16_generate_g1_len(ci, d->layout.log_n), n2 = pa_groth16_generate_g2_len(ci);
    const size_t ws = gen_layout(ci, d->layout.log_n).bytes;
    DevBuf dg1, dg2, do1, do2, dws;
    int rc;
    if ((rc = upload(dg1, g1, sizeof(pa_g1_affine))) || (rc = upload(dg2, g2, sizeof(pa_g2_affine)))) return rc;
    PA_TRY(do1.alloc(n1 * sizeof(pa_g1_affine)), "device scratch");
    PA_TRY(do2.alloc(n2 * sizeof(pa_g2_affine)), "device scratch");
    PA_TRY(dws.alloc(ws), "device scratch");
    if ((rc = pa_groth16_generate_device(ci, d, dg1.as<pa_g1_affine>(), dg2.as<pa_g2_affine>(), td,
                                         do1.as<pa_g1_affine>(), do2.as<pa_g2_affine>(), dws.p, ws, call_stream())))
        return rc;
    PA_TRY(call_sync(), "kernel execution");
    if ((rc = download(g1_out, do1, n1 * sizeof(pa_g1_affine)))) return rc;
    return download(g2_out, do2, n2 * sizeof(pa_g2_affine));
}

// ---- Groth16 verifier: the prepared verifying key, and proofs -> valid (kernels_groth16_verify.hip) ----
struct pa_groth16_vk {
    int dev = 0;
    size_t n_public = 0, bytes = 0;
    // one allocation: e(alpha, beta), -gamma and -delta (affine, next to each other), ic[0], the two
    // pa_g2_prepared records (-gamma, then -delta), the l comb tables of ic[1..l]; for the aggregate check the
    // comb tables of ic[0] and alpha behind them (tables l and l + 1) and -gamma, -delta, -beta (affine, next to
    // each other: the tail of its Q array)
    uint64_t* mem = nullptr;
    const uint64_t *e_ab = nullptr, *neg_gamma = nullptr, *neg_delta = nullptr, *ic0 = nullptr, *prep_gamma = nullptr,
                   *prep_delta = nullptr, *tables = nullptr, *q_tail = nullptr;
    size_t inputs() const { return n_public - 1; }
};

namespace {
// Fq one in the ABI's Montgomery words (R mod q)
constexpr uint64_t kFqOne[6] = {0x760900000002fffdull, 0xebf4000bc40c0002ull, 0x5f48985753c758baull,
                                0x77ce585370525745ull, 0x5c071a97a256ec6dull, 0x15f65ec3fa80e493ull};
// -y of an affine G2 record, as CurveAffine::negate (ec.rs:182-187): q - c for each nonzero Fq component
void g2_affine_negate(pa_g2_affine& p) {
    static const uint64_t q[6] = {0xb9feffffffffaaabull, 0x1eabfffeb153ffffull, 0x6730d2a0f6b0f624ull,
                                  0x64774b84f38512bfull, 0x4b1ba7b6434bacd7ull, 0x1a0111ea397fe69aull};
    if (p.infinity) return;
    for (pa_fq* c : {&p.y.c0, &p.y.c1}) {
        uint64_t any = 0;
        for (uint64_t w : c->l) any |= w;
        if (!any) continue;
        uint64_t borrow = 0;
        for (int i = 0; i < 6; i++) {
            const uint64_t a = q[i], b = c->l[i];
            const uint64_t d = a - b - borrow;
            borrow = (a < b || (a == b && borrow)) ? 1 : 0;
            c->l[i] = d;
        }
    }
}
// above this many proofs per call, (acc, -gamma) and (C, -delta) run on the shared-prepared Miller loop; below,
// all 3 k pairs run through pairing_ml_launch.  Measured (profiles/groth16_verify/default.txt): forced, the shared
// composition loses at 32768 proofs (three launches of at most one wave per SIMD, one after the other) and wins
// at 65536; nothing between was measured, so the bound is 65536.  Unlike the regime bounds
// above, PA_G16V_SHARED_MIN is read at every call, so one process can run both paths (tests, measurements).
size_t g16v_shared_min() { return pa::env_count("PA_G16V_SHARED_MIN", PA_GROTH16_VERIFY_SHARED_MIN); }
// the verify call's workspace: the P array (A | acc | C), the Q array (B, then -gamma and -delta k times for the
// 3 k-pair path), the 3 k Miller values, the k products (the final exponentiation runs in place there when the
// caller wants no gt), the ok bytes, the input sum's partials and the encoded entry's staging (the three byte
// arrays and their statuses)
struct VerifyLayout {
    size_t p, q, miller, prod, ok, partials, enc_a, enc_b, enc_c, status, bytes;
};
VerifyLayout verify_layout(const pa_groth16_vk* vk, size_t k) {
    VerifyLayout v{};
    size_t o = 0;
    v.p = o;        o = align256(o + 3 * k * sizeof(pa_g1_affine));
    v.q = o;        o = align256(o + 3 * k * sizeof(pa_g2_affine));
    v.miller = o;   o = align256(o + 3 * k * sizeof(pa_fq12));
    v.prod = o;     o = align256(o + k * sizeof(pa_fq12));
    v.ok = o;       o = align256(o + k);
    v.partials = o; o = align256(o + k * vk->inputs() * sizeof(pa_g1));
    v.enc_a = o;    o = align256(o + k * 48);
    v.enc_b = o;    o = align256(o + k * 96);
    v.enc_c = o;    o = align256(o + k * 48);
    v.status = o;   o = align256(o + 3 * k);
    v.bytes = o ? o : 256;
    return v;
}
// what every entry over a key refuses before touching memory; *mont gets the input format
int vk_call_check(const pa_groth16_vk* vk, const void* inputs, size_t input_stride, unsigned flags, size_t k,
                  int* mont) {
    if (!vk) return fail(PA_ERR_INVALID_ARGUMENT, "null pointer");
    if (flags & ~PA_MSM_SCALARS_MONTGOMERY) return fail(PA_ERR_INVALID_ARGUMENT, "unknown flag bits");
    if (k > PA_GROTH16_VERIFY_MAX_BATCH)
        return fail(PA_ERR_INVALID_ARGUMENT, "Groth16 verify batch over PA_GROTH16_VERIFY_MAX_BATCH: split it");
    if (input_stride < vk->inputs())
        return fail(PA_ERR_INVALID_ARGUMENT, "input_stride is smaller than the key's n_public - 1 inputs");
    if (k && vk->inputs() && !inputs) return fail(PA_ERR_INVALID_ARGUMENT, "null pointer");
    *mont = (flags & PA_MSM_SCALARS_MONTGOMERY) ? 1 : 0;
    return PA_OK;
}
int vk_stream_check(const pa_groth16_vk* vk, void* stream) {
    int dev = 0;
    PA_TRY(hipStreamGetDevice((hipStream_t)stream, &dev), "stream device");
    if (dev != vk->dev) return fail(PA_ERR_INVALID_ARGUMENT, "stream is on another device than the Groth16 key");
    return PA_OK;
}
// rows a host caller's input array holds: the last proof's row ends at its l-th input
size_t input_rows(const pa_groth16_vk* vk, size_t input_stride, size_t k) {
    return k && vk->inputs() ? (k - 1) * input_stride + vk->inputs() : 0;
}
// The chain behind the P and Q arrays (A and C, B in place; dev_status_abc: the decoders' statuses or null):
// input sum, Miller loops, product of three, final exponentiation, compare.
int verify_chain(const pa_groth16_vk* vk, const VerifyLayout& v, uint8_t* ws, const uint64_t* inputs,
                 size_t input_stride, int mont, size_t k, uint8_t* valid, const uint8_t* status_abc,
                 uint8_t* status_out, pa_fq12* gt, hipStream_t s) {
    uint64_t *p = (uint64_t*)(ws + v.p), *q = (uint64_t*)(ws + v.q), *ml = (uint64_t*)(ws + v.miller),
             *prod = (uint64_t*)(ws + v.prod);
    uint8_t* ok = ws + v.ok;
    PA_TRY(pa::launch_groth16_input_sum(vk->tables, vk->ic0, inputs, input_stride, mont, vk->inputs(), k,
                                        (uint64_t*)(ws + v.partials), p + kG1Words * k, s),
           "kernel launch");
    if (k < g16v_shared_min()) {
        PA_TRY(pa::launch_groth16_fill_q(vk->neg_gamma, vk->neg_delta, k, q, s), "kernel launch");
        PA_TRY(pairing_ml_launch(p, q, ml, 3 * k, s), "kernel launch");
    } else {
        // the (A, B) values differ from the reference's Miller values by an Fq2 factor per pair, which the final
        // exponentiation of the product removes as it does for one pair (pa_pairing_miller_loop_batch_device)
        PA_TRY(pairing_ml_launch(p, q, ml, k, s), "kernel launch");
        PA_TRY(pa::launch_miller_loop_shared_gen(p + kG1Words * k, vk->prep_gamma, ml + kF12Words * k, k, s),
               "kernel launch");
        PA_TRY(pa::launch_miller_loop_shared_gen(p + kG1Words * 2 * k, vk->prep_delta, ml + kF12Words * 2 * k, k, s),
               "kernel launch");
    }
    PA_TRY(pa::launch_fq12_product3(ml, k, prod, s), "kernel launch");
    uint64_t* out = gt ? (uint64_t*)gt : prod;
    PA_TRY(fe_launch(prod, out, ok, k, s), "kernel launch");
    PA_TRY(pa::launch_groth16_compare(out, ok, vk->e_ab, status_abc, status_out, valid, k, s), "kernel launch");
    return PA_OK;
}
}  // namespace

void pa_groth16_vk_free(pa_groth16_vk* vk) {
    if (!vk) return;
    if (vk->mem) (void)hipFree(vk->mem);
    delete vk;
}

int pa_groth16_vk_create(const pa_groth16_vkey* key, pa_groth16_vk** out) {
    if (!out) return fail(PA_ERR_INVALID_ARGUMENT, "null pointer");
    *out = nullptr;
    if (!key || !key->ic) return fail(PA_ERR_INVALID_ARGUMENT, "null pointer");
    if (key->n_public == 0) return fail(PA_ERR_INVALID_ARGUMENT, "n_public counts the constant one: it is at least 1");
    if (key->n_public - 1 > PA_GROTH16_VK_MAX_INPUTS)
        return fail(PA_ERR_INVALID_ARGUMENT, "Groth16 verifying keys support n_public - 1 <= PA_GROTH16_VK_MAX_INPUTS");
    const size_t l = key->n_public - 1, table_words = pa::g1_comb_table_words();
    // e(alpha, beta) once, with the pairing entry
    pa_fq12 e_ab;
    if (int rc = pa_pairing_batch(&key->alpha_g1, &key->beta_g2, &e_ab, 1)) return rc;
    constexpr size_t kHead = 72 + 2 * kG2Words + kG1Words;
    uint64_t head[kHead];
    pa_g2_affine neg[2] = {key->gamma_g2, key->delta_g2};
    g2_affine_negate(neg[0]);
    g2_affine_negate(neg[1]);
    memcpy(head, &e_ab, sizeof e_ab);
    memcpy(head + 72, neg, sizeof neg);
    memcpy(head + 72 + 2 * kG2Words, &key->ic[0], sizeof(pa_g1_affine));
    // only the flag byte of a record's last word is defined
    for (size_t w : {72 + kG2Words - 1, 72 + 2 * kG2Words - 1, kHead - 1}) head[w] &= 0xff;
    // -gamma, -delta, -beta: the last three Q records of the aggregate check
    constexpr size_t kTail = 3 * kG2Words;
    uint64_t tail[kTail];
    pa_g2_affine neg_beta = key->beta_g2;
    g2_affine_negate(neg_beta);
    memcpy(tail, neg, sizeof neg);
    memcpy(tail + 2 * kG2Words, &neg_beta, sizeof neg_beta);
    for (size_t w : {kG2Words - 1, 2 * kG2Words - 1, 3 * kG2Words - 1}) tail[w] &= 0xff;
    // ic[1..l], then ic[0] and alpha, as the Jacobian records the table builder reads
    std::vector<pa_g1> bases(l + 2);
    for (size_t i = 0; i < l + 2; i++) {
        const pa_g1_affine& a = i < l ? key->ic[i + 1] : (i == l ? key->ic[0] : key->alpha_g1);
        memset(&bases[i], 0, sizeof(pa_g1));
        if (a.infinity) {
            memcpy(bases[i].y.l, kFqOne, sizeof kFqOne);
        } else {
            bases[i].x = a.x;
            bases[i].y = a.y;
            memcpy(bases[i].z.l, kFqOne, sizeof kFqOne);
        }
    }
    const size_t prep_at = align256(kHead * 8), tables_at = align256(prep_at + 2 * sizeof(pa_g2_prepared));
    pa_groth16_vk* vk = new pa_groth16_vk;
    vk->n_public = key->n_public;
    const size_t tail_at = align256(tables_at + (l + 2) * table_words * 8);
    vk->bytes = tail_at + kTail * 8;
    int rc = PA_OK;
    DevBuf dbases, dws;
    hipError_t e = hipGetDevice(&vk->dev);
    if (e == hipSuccess) e = hipMalloc((void**)&vk->mem, vk->bytes);
    if (e != hipSuccess) rc = fail(hip_code(e), "create Groth16 verifying key", e);
    if (!rc) rc = upload(dbases, bases.data(), (l + 2) * sizeof(pa_g1));
    if (!rc && (e = dws.alloc(pa::g1_comb_workspace_words() * 8)) != hipSuccess)
        rc = fail(hip_code(e), "device scratch", e);
    if (!rc) {
        uint8_t* m = (uint8_t*)vk->mem;
        vk->e_ab = vk->mem;
        vk->neg_gamma = vk->mem + 72;
        vk->neg_delta = vk->neg_gamma + kG2Words;
        vk->ic0 = vk->neg_delta + kG2Words;
        vk->prep_gamma = (const uint64_t*)(m + prep_at);
        vk->prep_delta = (const uint64_t*)(m + prep_at + sizeof(pa_g2_prepared));
        vk->tables = (const uint64_t*)(m + tables_at);
        vk->q_tail = (const uint64_t*)(m + tail_at);
        const hipStream_t s = call_stream();
        e = hipMemcpyAsync(vk->mem, head, sizeof head, hipMemcpyHostToDevice, s);
        if (e == hipSuccess) e = hipMemcpyAsync(m + tail_at, tail, sizeof tail, hipMemcpyHostToDevice, s);
        if (e == hipSuccess) e = pa::launch_g2_prepare(vk->neg_gamma, (uint64_t*)(m + prep_at), 2, s);
        // one table per base, the builder's scratch reused in stream order
        for (size_t i = 0; i < l + 2 && e == hipSuccess; i++)
            e = pa::launch_g1_comb_table(dbases.as<uint64_t>() + 18 * i, (uint64_t*)(m + tables_at) + table_words * i,
                                         dws.as<uint64_t>(), s);
        if (e == hipSuccess) e = call_sync();   // `head` and the scratch go out of scope
        if (e != hipSuccess) rc = fail(hip_code(e), "create Groth16 verifying key", e);
    }
    if (rc) {
        pa_groth16_vk_free(vk);
        return rc;
    }
    *out = vk;
    return PA_OK;
}
size_t pa_groth16_vk_n_public(const pa_groth16_vk* vk) { return vk ? vk->n_public : 0; }
size_t pa_groth16_vk_bytes(const pa_groth16_vk* vk) { return vk ? vk->bytes : 0; }

size_t pa_groth16_vk_input_sum_workspace_bytes(const pa_groth16_vk* vk, size_t k) {
    return vk && k <= PA_GROTH16_VERIFY_MAX_BATCH ? k * vk->inputs() * sizeof(pa_g1) : 0;
}

int pa_groth16_vk_input_sum_device(const pa_groth16_vk* vk, const pa_fr* inputs, size_t input_stride, unsigned flags,
                                   size_t k, pa_g1_affine* out, void* workspace, size_t workspace_bytes,
                                   void* stream) {
    int mont = 0;
    if (int rc = vk_call_check(vk, inputs, input_stride, flags, k, &mont)) return rc;
    if (k == 0) return PA_OK;
    const size_t need = pa_groth16_vk_input_sum_workspace_bytes(vk, k);
    if (!out || (need && !workspace)) return fail(PA_ERR_INVALID_ARGUMENT, "null pointer");
    if (workspace_bytes < need)
        return fail(PA_ERR_INVALID_ARGUMENT, "workspace smaller than pa_groth16_vk_input_sum_workspace_bytes");
    if (int rc = vk_stream_check(vk, stream)) return rc;
    PA_TRY(pa::launch_groth16_input_sum(vk->tables, vk->ic0, (const uint64_t*)inputs, input_stride, mont, vk->inputs(),
                                        k, (uint64_t*)workspace, (uint64_t*)out, (hipStream_t)stream),
           "kernel launch");
    return PA_OK;
}

int pa_groth16_vk_input_sum(const pa_groth16_vk* vk, const pa_fr* inputs, size_t input_stride, unsigned flags, size_t k,
                            pa_g1_affine* out) {
    int mont = 0;
    if (int rc = vk_call_check(vk, inputs, input_stride, flags, k, &mont)) return rc;
    if (k == 0) return PA_OK;
    if (!out) return fail(PA_ERR_INVALID_ARGUMENT, "null pointer");
    DevBuf din, dout, dws;
    int rc;
    if ((rc = upload(din, inputs, input_rows(vk, input_stride, k) * sizeof(pa_fr)))) return rc;
    PA_TRY(dout.alloc(k * sizeof(pa_g1_affine)), "device scratch");
    const size_t ws = pa_groth16_vk_input_sum_workspace_bytes(vk, k);
    PA_TRY(dws.alloc(ws), "device scratch");
    if ((rc = pa_groth16_vk_input_sum_device(vk, din.as<pa_fr>(), input_stride, flags, k, dout.as<pa_g1_affine>(),
                                             dws.p, ws, call_stream())))
        return rc;
    return download(out, dout, k * sizeof(pa_g1_affine));
}

size_t pa_groth16_verify_workspace_bytes(const pa_groth16_vk* vk, size_t k) {
    return vk && k <= PA_GROTH16_VERIFY_MAX_BATCH ? verify_layout(vk, k).bytes : 0;
}

int pa_groth16_verify_device(const pa_groth16_vk* vk, const pa_groth16_proof* proofs, const pa_fr* inputs,
                             size_t input_stride, unsigned flags, size_t k, uint8_t* valid, pa_fq12* gt,
                             void* workspace, size_t workspace_bytes, void* stream) {
    int mont = 0;
    if (int rc = vk_call_check(vk, inputs, input_stride, flags, k, &mont)) return rc;
    if (k == 0) return PA_OK;
    if (!proofs || !valid || !workspace) return fail(PA_ERR_INVALID_ARGUMENT, "null pointer");
    const VerifyLayout v = verify_layout(vk, k);
    if (workspace_bytes < v.bytes)
        return fail(PA_ERR_INVALID_ARGUMENT, "workspace smaller than pa_groth16_verify_workspace_bytes");
    if (int rc = vk_stream_check(vk, stream)) return rc;
    uint8_t* ws = static_cast<uint8_t*>(workspace);
    const hipStream_t s = (hipStream_t)stream;
    PA_TRY(pa::launch_groth16_split((const uint64_t*)proofs, k, (uint64_t*)(ws + v.p), (uint64_t*)(ws + v.q), s),
           "kernel launch");
    return verify_chain(vk, v, ws, (const uint64_t*)inputs, input_stride, mont, k, valid, nullptr, nullptr, gt, s);
}

int pa_groth16_verify_encoded_device(const pa_groth16_vk* vk, const uint8_t* enc, const pa_fr* inputs,
                                     size_t input_stride, unsigned flags, size_t k, uint8_t* valid, uint8_t* status,
                                     pa_fq12* gt, void* workspace, size_t workspace_bytes, void* stream) {
    int mont = 0;
    if (int rc = vk_call_check(vk, inputs, input_stride, flags, k, &mont)) return rc;
    if (k == 0) return PA_OK;
    if (!enc || !valid || !status || !workspace) return fail(PA_ERR_INVALID_ARGUMENT, "null pointer");
    const VerifyLayout v = verify_layout(vk, k);
    if (workspace_bytes < v.bytes)
        return fail(PA_ERR_INVALID_ARGUMENT, "workspace smaller than pa_groth16_verify_workspace_bytes");
    if (int rc = vk_stream_check(vk, stream)) return rc;
    uint8_t* ws = static_cast<uint8_t*>(workspace);
    const hipStream_t s = (hipStream_t)stream;
    uint64_t *p = (uint64_t*)(ws + v.p), *q = (uint64_t*)(ws + v.q);
    uint8_t* st = ws + v.status;
    PA_TRY(pa::launch_groth16_gather(enc, k, ws + v.enc_a, ws + v.enc_b, ws + v.enc_c, s), "kernel launch");
    // the checked decoders write the P and Q arrays themselves (the point at infinity for a record that fails)
    PA_TRY(pa::launch_decode(1, 1, 1, ws + v.enc_a, k, p, st, s), "kernel launch");
    PA_TRY(pa::launch_decode(2, 1, 1, ws + v.enc_b, k, q, st + k, s), "kernel launch");
    PA_TRY(pa::launch_decode(1, 1, 1, ws + v.enc_c, k, p + kG1Words * 2 * k, st + 2 * k, s), "kernel launch");
    return verify_chain(vk, v, ws, (const uint64_t*)inputs, input_stride, mont, k, valid, st, status, gt, s);
}

namespace {
// both host entries: one stream round trip, like pa_multi_pairing_batch
int verify_host(const pa_groth16_vk* vk, const pa_groth16_proof* proofs, const uint8_t* enc, const pa_fr* inputs,
                size_t input_stride, unsigned flags, size_t k, uint8_t* valid, uint8_t* status, pa_fq12* gt) {
    int mont = 0;
    if (int rc = vk_call_check(vk, inputs, input_stride, flags, k, &mont)) return rc;
    if (k == 0) return PA_OK;
    if ((!proofs && !enc) || !valid || (enc && !status)) return fail(PA_ERR_INVALID_ARGUMENT, "null pointer");
    DevBuf dproofs, din, dflags, dgt, dws;
    int rc;
    if ((rc = enc ? upload(dproofs, enc, k * PA_GROTH16_ENCODED_PROOF_BYTES)
                  : upload(dproofs, proofs, k * sizeof(pa_groth16_proof))))
        return rc;
    if ((rc = upload(din, inputs, input_rows(vk, input_stride, k) * sizeof(pa_fr)))) return rc;
    PA_TRY(dflags.alloc(4 * k), "device scratch");   // valid, then the 3 k statuses
    if (gt) PA_TRY(dgt.alloc(k * sizeof(pa_fq12)), "device scratch");
    const size_t ws = verify_layout(vk, k).bytes;
    PA_TRY(dws.alloc(ws), "device scratch");
    const hipStream_t s = call_stream();
    uint8_t* dvalid = dflags.as<uint8_t>();
    pa_fq12* dg = gt ? dgt.as<pa_fq12>() : nullptr;
    rc = enc ? pa_groth16_verify_encoded_device(vk, dproofs.as<uint8_t>(), din.as<pa_fr>(), input_stride, flags, k,
                                                dvalid, dvalid + k, dg, dws.p, ws, s)
             : pa_groth16_verify_device(vk, dproofs.as<pa_groth16_proof>(), din.as<pa_fr>(), input_stride, flags, k,
                                        dvalid, dg, dws.p, ws, s);
    if (rc) return rc;
    PA_TRY(hipMemcpyAsync(valid, dvalid, k, hipMemcpyDeviceToHost, s), "D2H copy");
    if (enc) PA_TRY(hipMemcpyAsync(status, dvalid + k, 3 * k, hipMemcpyDeviceToHost, s), "D2H copy");
    if (gt) PA_TRY(hipMemcpyAsync(gt, dgt.p, k * sizeof(pa_fq12), hipMemcpyDeviceToHost, s), "D2H copy");
    PA_TRY(hipStreamSynchronize(s), "kernel execution");
    return PA_OK;
}
}  // namespace

int pa_groth16_verify(const pa_groth16_vk* vk, const pa_groth16_proof* proofs, const pa_fr* inputs, size_t input_stride,
                      unsigned flags, size_t k, uint8_t* valid, pa_fq12* gt) {
    if (k && !proofs) return fail(PA_ERR_INVALID_ARGUMENT, "null pointer");
    return verify_host(vk, proofs, nullptr, inputs, input_stride, flags, k, valid, nullptr, gt);
}

int pa_groth16_verify_encoded(const pa_groth16_vk* vk, const uint8_t* enc, const pa_fr* inputs, size_t input_stride,
                              unsigned flags, size_t k, uint8_t* valid, uint8_t* status, pa_fq12* gt) {
    if (k && !enc) return fail(PA_ERR_INVALID_ARGUMENT, "null pointer");
    return verify_host(vk, nullptr, enc, inputs, input_stride, flags, k, valid, status, gt);
}

// ---- Groth16 aggregate check: k proofs in one randomised pairing product (kernels_groth16_aggregate.hip) ----
namespace {
// The workspace: the P array (A'_0.. | accS | CS | alphaS, k + 3 affine records) first, at the next multiple of 256
// bytes the Q array (B_0.. | -gamma | -delta | -beta); then the Jacobian rows that become P, the A and C arrays,
// the Miller values (the product runs in place), the one gt and ok byte, the weight sums and their partials, the
// comb partials, the MSM's workspace and the encoded entry's staging.
constexpr size_t kG1JacWords = sizeof(pa_g1) / 8;
struct AggLayout {
    size_t p, q, jac, a, c, miller, gt, ok, s, wpart, comb, msm, msm_bytes, enc_a, enc_b, enc_c, status, bytes;
};
AggLayout agg_layout(const pa_groth16_vk* vk, size_t k) {
    AggLayout v{};
    const size_t l = vk->inputs();
    size_t o = 0;
    v.p = o;      o = align256(o + (k + 3) * sizeof(pa_g1_affine));
    v.q = o;      o = align256(o + (k + 3) * sizeof(pa_g2_affine));
    v.jac = o;    o = align256(o + (k + 3) * sizeof(pa_g1));
    v.a = o;      o = align256(o + k * sizeof(pa_g1_affine));
    v.c = o;      o = align256(o + k * sizeof(pa_g1_affine));
    v.miller = o; o = align256(o + (k + 3) * sizeof(pa_fq12));
    v.gt = o;     o = align256(o + sizeof(pa_fq12));
    v.ok = o;     o = align256(o + 2);   // the final exponentiation's ok byte, then the statuses' any-nonzero byte
    v.s = o;      o = align256(o + (l + 1) * sizeof(pa_fr));
    v.wpart = o;  o = align256(o + (size_t)pa::kGroth16WeightMaxBlocks * (l + 1) * sizeof(pa_fr));
    v.comb = o;   o = align256(o + (l + 2) * sizeof(pa_g1));
    v.msm_bytes = pa::msm_u128_workspace_bytes(k);   // never decreases with k, like every other term here
    v.msm = o;    o = align256(o + v.msm_bytes);
    v.enc_a = o;  o = align256(o + k * 48);
    v.enc_b = o;  o = align256(o + k * 96);
    v.enc_c = o;  o = align256(o + k * 48);
    v.status = o; o = align256(o + 3 * k);
    v.bytes = o;
    return v;
}
// what the three device entries refuse before anything runs; fills the layout
int agg_check(const pa_groth16_vk* vk, const void* inputs, size_t input_stride, unsigned flags, const void* z,
              size_t k, const void* workspace, size_t workspace_bytes, void* stream, int* mont, AggLayout* v) {
    if (int rc = vk_call_check(vk, inputs, input_stride, flags, k, mont)) return rc;
    if (!workspace || (k && !z)) return fail(PA_ERR_INVALID_ARGUMENT, "null pointer");
    if ((uintptr_t)z & 15) return fail(PA_ERR_INVALID_ARGUMENT, "z is not 16-byte aligned");
    *v = agg_layout(vk, k);
    if (workspace_bytes < v->bytes)
        return fail(PA_ERR_INVALID_ARGUMENT, "workspace smaller than pa_groth16_verify_aggregate_workspace_bytes");
    return vk_stream_check(vk, stream);
}
// Behind the A, B and C arrays: the weight sums, A' = z A, the comb sums, the MSM, into_affine of the k + 3
// Jacobian rows into the P array, the Q array's tail.
int agg_points(const pa_groth16_vk* vk, const AggLayout& v, uint8_t* ws, const uint64_t* inputs, size_t input_stride,
               int mont, const uint64_t* z, size_t k, hipStream_t s) {
    const size_t l = vk->inputs();
    uint64_t *jac = (uint64_t*)(ws + v.jac), *sums = (uint64_t*)(ws + v.s);
    PA_TRY(pa::launch_groth16_weight_sums(z, inputs, input_stride, mont, l, k, (uint64_t*)(ws + v.wpart), sums, s),
           "kernel launch");
    PA_TRY(pa::launch_groth16_scale((const uint64_t*)(ws + v.a), z, k, jac, s), "kernel launch");
    PA_TRY(pa::launch_groth16_comb_sum(vk->tables, sums, l, (uint64_t*)(ws + v.comb), jac + kG1JacWords * k,
                                       jac + kG1JacWords * (k + 2), s),
           "kernel launch");
    PA_TRY(pa::launch_msm_u128_g1((const uint64_t*)(ws + v.c), z, k, jac + kG1JacWords * (k + 1), ws + v.msm,
                                  v.msm_bytes, s),
           "kernel launch");
    PA_TRY(pa::launch_group_op(1, pa::GROUP_INTO_AFFINE, jac, nullptr, (uint64_t*)(ws + v.p), k + 3, s),
           "kernel launch");
    PA_TRY(hipMemcpyAsync((uint64_t*)(ws + v.q) + kG2Words * k, vk->q_tail, 3 * sizeof(pa_g2_affine),
                          hipMemcpyDeviceToDevice, s),
           "device copy");
    return PA_OK;
}
// k + 3 Miller loops in one launch, their product, one final exponentiation, the compare with one
int agg_pairing(const AggLayout& v, uint8_t* ws, size_t k, uint8_t* valid, const uint8_t* status_abc,
                uint8_t* status_out, pa_fq12* gt, hipStream_t s) {
    uint64_t* ml = (uint64_t*)(ws + v.miller);
    uint64_t* out = gt ? (uint64_t*)gt : (uint64_t*)(ws + v.gt);
    PA_TRY(pairing_ml_launch((const uint64_t*)(ws + v.p), (const uint64_t*)(ws + v.q), ml, k + 3, s), "kernel launch");
    PA_TRY(pa::launch_fq12_product(ml, k + 3, ml, s), "kernel launch");
    PA_TRY(fe_launch(ml, out, ws + v.ok, 1, s), "kernel launch");
    PA_TRY(pa::launch_groth16_aggregate_finish(out, ws + v.ok, status_abc, status_out, ws + v.ok + 1, valid, k, 0, s),
           "kernel launch");
    return PA_OK;
}
}  // namespace

size_t pa_groth16_verify_aggregate_workspace_bytes(const pa_groth16_vk* vk, size_t k) {
    return vk && k <= PA_GROTH16_VERIFY_MAX_BATCH ? agg_layout(vk, k).bytes : 0;
}

int pa_groth16_verify_aggregate_points_device(const pa_groth16_vk* vk, const pa_groth16_proof* proofs,
                                              const pa_fr* inputs, size_t input_stride, unsigned flags,
                                              const uint64_t* z, size_t k, pa_g1_affine* out, void* workspace,
                                              size_t workspace_bytes, void* stream) {
    int mont = 0;
    AggLayout v;
    if (int rc = agg_check(vk, inputs, input_stride, flags, z, k, workspace, workspace_bytes, stream, &mont, &v))
        return rc;
    if (!out || (k && !proofs)) return fail(PA_ERR_INVALID_ARGUMENT, "null pointer");
    uint8_t* ws = static_cast<uint8_t*>(workspace);
    const hipStream_t s = (hipStream_t)stream;
    PA_TRY(pa::launch_groth16_split3((const uint64_t*)proofs, k, (uint64_t*)(ws + v.a), (uint64_t*)(ws + v.q),
                                     (uint64_t*)(ws + v.c), s),
           "kernel launch");
    if (int rc = agg_points(vk, v, ws, (const uint64_t*)inputs, input_stride, mont, z, k, s)) return rc;
    PA_TRY(hipMemcpyAsync(out, ws + v.p, (k + 3) * sizeof(pa_g1_affine), hipMemcpyDeviceToDevice, s), "device copy");
    return PA_OK;
}

int pa_groth16_verify_aggregate_device(const pa_groth16_vk* vk, const pa_groth16_proof* proofs, const pa_fr* inputs,
                                       size_t input_stride, unsigned flags, const uint64_t* z, size_t k,
                                       uint8_t* valid, pa_fq12* gt, void* workspace, size_t workspace_bytes,
                                       void* stream) {
    int mont = 0;
    AggLayout v;
    if (int rc = agg_check(vk, inputs, input_stride, flags, z, k, workspace, workspace_bytes, stream, &mont, &v))
        return rc;
    if (!valid || (k && !proofs)) return fail(PA_ERR_INVALID_ARGUMENT, "null pointer");
    uint8_t* ws = static_cast<uint8_t*>(workspace);
    const hipStream_t s = (hipStream_t)stream;
    if (k == 0) {   // the empty product
        PA_TRY(pa::launch_groth16_aggregate_finish((uint64_t*)gt, nullptr, nullptr, nullptr, nullptr, valid, 0, 1, s),
               "kernel launch");
        return PA_OK;
    }
    PA_TRY(pa::launch_groth16_split3((const uint64_t*)proofs, k, (uint64_t*)(ws + v.a), (uint64_t*)(ws + v.q),
                                     (uint64_t*)(ws + v.c), s),
           "kernel launch");
    if (int rc = agg_points(vk, v, ws, (const uint64_t*)inputs, input_stride, mont, z, k, s)) return rc;
    return agg_pairing(v, ws, k, valid, nullptr, nullptr, gt, s);
}

int pa_groth16_verify_aggregate_encoded_device(const pa_groth16_vk* vk, const uint8_t* enc, const pa_fr* inputs,
                                               size_t input_stride, unsigned flags, const uint64_t* z, size_t k,
                                               uint8_t* valid, uint8_t* status, pa_fq12* gt, void* workspace,
                                               size_t workspace_bytes, void* stream) {
    int mont = 0;
    AggLayout v;
    if (int rc = agg_check(vk, inputs, input_stride, flags, z, k, workspace, workspace_bytes, stream, &mont, &v))
        return rc;
    if (!valid || (k && (!enc || !status))) return fail(PA_ERR_INVALID_ARGUMENT, "null pointer");
    uint8_t* ws = static_cast<uint8_t*>(workspace);
    const hipStream_t s = (hipStream_t)stream;
    if (k == 0) {
        PA_TRY(pa::launch_groth16_aggregate_finish((uint64_t*)gt, nullptr, nullptr, nullptr, nullptr, valid, 0, 1, s),
               "kernel launch");
        return PA_OK;
    }
    uint8_t* st = ws + v.status;
    PA_TRY(pa::launch_groth16_gather(enc, k, ws + v.enc_a, ws + v.enc_b, ws + v.enc_c, s), "kernel launch");
    // the checked decoders write the A, B and C arrays themselves (the point at infinity for a record that fails)
    PA_TRY(pa::launch_decode(1, 1, 1, ws + v.enc_a, k, (uint64_t*)(ws + v.a), st, s), "kernel launch");
    PA_TRY(pa::launch_decode(2, 1, 1, ws + v.enc_b, k, (uint64_t*)(ws + v.q), st + k, s), "kernel launch");
    PA_TRY(pa::launch_decode(1, 1, 1, ws + v.enc_c, k, (uint64_t*)(ws + v.c), st + 2 * k, s), "kernel launch");
    if (int rc = agg_points(vk, v, ws, (const uint64_t*)inputs, input_stride, mont, z, k, s)) return rc;
    return agg_pairing(v, ws, k, valid, st, status, gt, s);
}

namespace {
// the host entries: one stream round trip.  what: 0 verify, 1 encoded, 2 points
int agg_host(int what, const pa_groth16_vk* vk, const void* proofs, const pa_fr* inputs, size_t input_stride,
             unsigned flags, const uint64_t* z, size_t k, uint8_t* valid, uint8_t* status, pa_fq12* gt,
             pa_g1_affine* points) {
    int mont = 0;
    if (int rc = vk_call_check(vk, inputs, input_stride, flags, k, &mont)) return rc;
    if ((what == 2 ? !points : !valid) || (k && (!proofs || !z || (what == 1 && !status))))
        return fail(PA_ERR_INVALID_ARGUMENT, "null pointer");
    DevBuf dproofs, din, dz, dflags, dgt, dpts, dws;
    int rc;
    if ((rc = upload(dproofs, proofs, k * (what == 1 ? PA_GROTH16_ENCODED_PROOF_BYTES : sizeof(pa_groth16_proof)))))
        return rc;
    if ((rc = upload(din, inputs, input_rows(vk, input_stride, k) * sizeof(pa_fr)))) return rc;
    if ((rc = upload(dz, z, 16 * k))) return rc;
    PA_TRY(dflags.alloc(1 + 3 * k), "device scratch");   // valid, then the 3 k statuses
    if (gt) PA_TRY(dgt.alloc(sizeof(pa_fq12)), "device scratch");
    if (what == 2) PA_TRY(dpts.alloc((k + 3) * sizeof(pa_g1_affine)), "device scratch");
    const size_t ws = agg_layout(vk, k).bytes;
    PA_TRY(dws.alloc(ws), "device scratch");
    const hipStream_t s = call_stream();
    uint8_t* dvalid = dflags.as<uint8_t>();
    pa_fq12* dg = gt ? dgt.as<pa_fq12>() : nullptr;
    if (what == 0)
        rc = pa_groth16_verify_aggregate_device(vk, dproofs.as<pa_groth16_proof>(), din.as<pa_fr>(), input_stride,
                                                flags, dz.as<uint64_t>(), k, dvalid, dg, dws.p, ws, s);
    else if (what == 1)
        rc = pa_groth16_verify_aggregate_encoded_device(vk, dproofs.as<uint8_t>(), din.as<pa_fr>(), input_stride,
                                                        flags, dz.as<uint64_t>(), k, dvalid, dvalid + 1, dg, dws.p,
                                                        ws, s);
    else
        rc = pa_groth16_verify_aggregate_points_device(vk, dproofs.as<pa_groth16_proof>(), din.as<pa_fr>(),
                                                       input_stride, flags, dz.as<uint64_t>(), k,
                                                       dpts.as<pa_g1_affine>(), dws.p, ws, s);
    if (rc) return rc;
    if (what == 2) {
        PA_TRY(hipMemcpyAsync(points, dpts.p, (k + 3) * sizeof(pa_g1_affine), hipMemcpyDeviceToHost, s), "D2H copy");
    } else {
        PA_TRY(hipMemcpyAsync(valid, dvalid, 1, hipMemcpyDeviceToHost, s), "D2H copy");
        if (what == 1 && k) PA_TRY(hipMemcpyAsync(status, dvalid + 1, 3 * k, hipMemcpyDeviceToHost, s), "D2H copy");
        if (gt) PA_TRY(hipMemcpyAsync(gt, dgt.p, sizeof(pa_fq12), hipMemcpyDeviceToHost, s), "D2H copy");
    }
    PA_TRY(hipStreamSynchronize(s), "kernel execution");
    return PA_OK;
}
}  // namespace

int pa_groth16_verify_aggregate(const pa_groth16_vk* vk, const pa_groth16_proof* proofs, const pa_fr* inputs,
                                size_t input_stride, unsigned flags, const uint64_t* z, size_t k, uint8_t* valid,
                                pa_fq12* gt) {
    return agg_host(0, vk, proofs, inputs, input_stride, flags, z, k, valid, nullptr, gt, nullptr);
}
int pa_groth16_verify_aggregate_encoded(const pa_groth16_vk* vk, const uint8_t* enc, const pa_fr* inputs,
                                        size_t input_stride, unsigned flags, const uint64_t* z, size_t k,
                                        uint8_t* valid, uint8_t* status, pa_fq12* gt) {
    return agg_host(1, vk, enc, inputs, input_stride, flags, z, k, valid, status, gt, nullptr);
}
int pa_groth16_verify_aggregate_points(const pa_groth16_vk* vk, const pa_groth16_proof* proofs, const pa_fr* inputs,
                                       size_t input_stride, unsigned flags, const uint64_t* z, size_t k,
                                       pa_g1_affine* out) {
    return agg_host(2, vk, proofs, inputs, input_stride, flags, z, k, nullptr, nullptr, nullptr, out);
}

// ---- CurveProjective / CurveAffine surface, G1 and G2 (kernels_group.hip) ----
namespace {
constexpr size_t jac_bytes(int group) { return group == 1 ? sizeof(pa_g1) : sizeof(pa_g2); }
constexpr size_t aff_bytes(int group) { return group == 1 ? sizeof(pa_g1_affine) : sizeof(pa_g2_affine); }
size_t op_in_bytes(int group, int op) { return op == pa::GROUP_FROM_AFFINE ? aff_bytes(group) : jac_bytes(group); }
size_t op_b_bytes(int group, int op) {
    if (op == pa::GROUP_ADD || op == pa::GROUP_SUB || op == pa::GROUP_EQ) return jac_bytes(group);
    return op == pa::GROUP_ADD_MIXED ? aff_bytes(group) : 0;
}
size_t op_out_bytes(int group, int op) {
    if (op == pa::GROUP_EQ) return 1;
    return op == pa::GROUP_INTO_AFFINE ? aff_bytes(group) : jac_bytes(group);
}

int host_group_op(int group, int op, const void* a, const void* b, void* out, size_t n) {
    if (n == 0) return PA_OK;
    const size_t ib = op_in_bytes(group, op), bb = op_b_bytes(group, op), ob = op_out_bytes(group, op);
    if (!a || !out || (bb && !b)) return fail(PA_ERR_INVALID_ARGUMENT, "null pointer");
    DevBuf da, db, dout;
    int rc;
    if ((rc = upload(da, a, ib * n))) return rc;
    if (bb && (rc = upload(db, b, bb * n))) return rc;
    PA_TRY(dout.alloc(ob * n), "device scratch");
    PA_TRY(pa::launch_group_op(group, op, da.as<uint64_t>(), db.as<uint64_t>(), dout.as<uint64_t>(), n, call_stream()),
           "kernel launch");
    PA_TRY(call_sync(), "kernel execution");
    return download(out, dout, ob * n);
}
int device_group_op(int group, int op, const void* a, const void* b, void* out, size_t n, void* stream) {
    if (n && (!a || !out || (op_b_bytes(group, op) && !b))) return fail(PA_ERR_INVALID_ARGUMENT, "null pointer");
    PA_TRY(pa::launch_group_op(group, op, (const uint64_t*)a, (const uint64_t*)b, (uint64_t*)out, n,
                               (hipStream_t)stream),
           "kernel launch");
    return PA_OK;
}

// FrRepr::num_bits (fr.rs:58 via the repr macro): 256 minus leading zeros
int repr_num_bits(const pa_fr_repr* s) {
    for (int w = 3; w >= 0; w--)
        if (s->l[w]) return 64 * w + 64 - __builtin_clzll(s->l[w]);
    return 0;
}
int window_for_count(size_t n, const size_t* rec, int m) {
    int ret = 4;
    for (int k = 0; k < m && n > rec[k]; k++) ret++;
    return ret;
}
}  // namespace

#define PA_GROUP_ENTRIES(G, JAC, AFF)                                                                            \
    int pa_g##G##_double_batch(const JAC* a, JAC* out, size_t n) {                                              \
        return host_group_op(G, pa::GROUP_DOUBLE, a, nullptr, out, n);                                          \
    }                                                                                                           \
    int pa_g##G##_add_batch(const JAC* a, const JAC* b, JAC* out, size_t n) {                                    \
        return host_group_op(G, pa::GROUP_ADD, a, b, out, n);                                                   \
    }                                                                                                           \
    int pa_g##G##_add_mixed_batch(const JAC* a, const AFF* b, JAC* out, size_t n) {                              \
        return host_group_op(G, pa::GROUP_ADD_MIXED, a, b, out, n);                                             \
    }                                                                                                           \
    int pa_g##G##_negate_batch(const JAC* a, JAC* out, size_t n) {                                              \
        return host_group_op(G, pa::GROUP_NEGATE, a, nullptr, out, n);                                          \
    }                                                                                                           \
    int pa_g##G##_sub_batch(const JAC* a, const JAC* b, JAC* out, size_t n) {                                    \
        return host_group_op(G, pa::GROUP_SUB, a, b, out, n);                                                   \
    }                                                                                                           \
    int pa_g##G##_into_affine_batch(const JAC* a, AFF* out, size_t n) {                                         \
        return host_group_op(G, pa::GROUP_INTO_AFFINE, a, nullptr, out, n);                                     \
    }                                                                                                           \
    int pa_g##G##_into_projective_batch(const AFF* a, JAC* out, size_t n) {                                     \
        return host_group_op(G, pa::GROUP_FROM_AFFINE, a, nullptr, out, n);                                     \
    }                                                                                                           \
    int pa_g##G##_double_batch_device(const JAC* a, JAC* out, size_t n, void* stream) {                         \
        return device_group_op(G, pa::GROUP_DOUBLE, a, nullptr, out, n, stream);                                \
    }                                                                                                           \
    int pa_g##G##_add_batch_device(const JAC* a, const JAC* b, JAC* out, size_t n, void* stream) {              \
        return device_group_op(G, pa::GROUP_ADD, a, b, out, n, stream);                                         \
    }                                                                                                           \
    int pa_g##G##_add_mixed_batch_device(const JAC* a, const AFF* b, JAC* out, size_t n, void* stream) {        \
        return device_group_op(G, pa::GROUP_ADD_MIXED, a, b, out, n, stream);                                   \
    }                                                                                                           \
    int pa_g##G##_into_affine_batch_device(const JAC* a, AFF* out, size_t n, void* stream) {                    \
        return device_group_op(G, pa::GROUP_INTO_AFFINE, a, nullptr, out, n, stream);                           \
    }                                                                                                           \
    int pa_g##G##_eq_batch(const JAC* a, const JAC* b, uint8_t* eq, size_t n) {                                 \
        return host_group_op(G, pa::GROUP_EQ, a, b, eq, n);                                                     \
    }                                                                                                           \
    int pa_g##G##_eq_batch_device(const JAC* a, const JAC* b, uint8_t* eq, size_t n, void* stream) {            \
        return device_group_op(G, pa::GROUP_EQ, a, b, eq, n, stream);                                           \
    }

PA_GROUP_ENTRIES(1, pa_g1, pa_g1_affine)
PA_GROUP_ENTRIES(2, pa_g2, pa_g2_affine)
#undef PA_GROUP_ENTRIES

int pa_g2_batch_normalization(pa_g2* v, size_t n) {
    if (n == 0) return PA_OK;
    if (!v) return fail(PA_ERR_INVALID_ARGUMENT, "null pointer");
    DevBuf dv;
    int rc;
    if ((rc = upload(dv, v, sizeof(pa_g2) * n))) return rc;
    PA_TRY(pa::launch_g2_batch_normalize(dv.as<uint64_t>(), n, call_stream()), "kernel launch");
    PA_TRY(call_sync(), "kernel execution");
    return download(v, dv, sizeof(pa_g2) * n);
}
int pa_g2_batch_normalization_device(pa_g2* v, size_t n, void* stream) {
    if (n && !v) return fail(PA_ERR_INVALID_ARGUMENT, "null pointer");
    PA_TRY(pa::launch_g2_batch_normalize((uint64_t*)v, n, (hipStream_t)stream), "kernel launch");
    return PA_OK;
}
size_t pa_g2_fixed_base_table_words(void) { return pa::g2_comb_table_words(); }
size_t pa_g2_fixed_base_workspace_words(void) { return pa::g2_comb_workspace_words(); }
int pa_g2_wnaf_fixed_base_device(const pa_g2* base, const pa_fr_repr* scalars, pa_g2* out, size_t n,
                                 uint64_t* table, uint64_t* workspace, void* stream) {
    return pa_g2_wnaf_fixed_base_window_device(base, scalars, out, n, pa_g2_recommended_wnaf_for_num_scalars(n), table,
                                               workspace, stream);
}
int pa_g2_wnaf_fixed_base_window_device(const pa_g2* base, const pa_fr_repr* scalars, pa_g2* out, size_t n,
                                        int window, uint64_t* table, uint64_t* workspace, void* stream) {
    if (n == 0) return PA_OK;
    if (!base || !scalars || !out || !table || !workspace) return fail(PA_ERR_INVALID_ARGUMENT, "null pointer");
    if (window < 1 || window > kMaxWnafWindow) return fail(PA_ERR_INVALID_ARGUMENT, "wnaf window out of range");
    PA_TRY(pa::launch_g2_comb_table((const uint64_t*)base, table, workspace, (hipStream_t)stream), "kernel launch");
    PA_TRY(pa::launch_g2_comb_mul(table, (const uint64_t*)scalars, (uint64_t*)out, n, window, (hipStream_t)stream),
           "kernel launch");
    return PA_OK;
}
int pa_g2_wnaf_fixed_base(const pa_g2* base, const pa_fr_repr* scalars, size_t n, pa_g2* out) {
    return pa_g2_wnaf_fixed_base_window(base, scalars, n, pa_g2_recommended_wnaf_for_num_scalars(n), out);
}
int pa_g2_wnaf_fixed_base_window(const pa_g2* base, const pa_fr_repr* scalars, size_t n, int window, pa_g2* out) {
    if (n == 0) return PA_OK;
    if (!base || !scalars || !out) return fail(PA_ERR_INVALID_ARGUMENT, "null pointer");
    if (window < 1 || window > kMaxWnafWindow) return fail(PA_ERR_INVALID_ARGUMENT, "wnaf window out of range");
    DevBuf db, ds, dt, dw, dout;
    int rc;
    if ((rc = upload(db, base, sizeof(pa_g2))) || (rc = upload(ds, scalars, sizeof(pa_fr_repr) * n))) return rc;
    PA_TRY(dt.alloc(8 * pa::g2_comb_table_words()), "device scratch");
    PA_TRY(dw.alloc(8 * pa::g2_comb_workspace_words()), "device scratch");
    PA_TRY(dout.alloc(sizeof(pa_g2) * n), "device scratch");
    if ((rc = pa_g2_wnaf_fixed_base_window_device(db.as<pa_g2>(), ds.as<pa_fr_repr>(), dout.as<pa_g2>(), n, window,
                                                  dt.as<uint64_t>(), dw.as<uint64_t>(), call_stream())))
        return rc;
    PA_TRY(call_sync(), "kernel execution");
    return download(out, dout, sizeof(pa_g2) * n);
}

// window heuristics (ec.rs:895-921 for G1, 1586-1612 for G2)
int pa_g1_recommended_wnaf_for_scalar(const pa_fr_repr* s) {
    if (!s) return fail(PA_ERR_INVALID_ARGUMENT, "null pointer");
    const int b = repr_num_bits(s);
    return b >= 130 ? 4 : b >= 34 ? 3 : 2;
}
int pa_g2_recommended_wnaf_for_scalar(const pa_fr_repr* s) {
    if (!s) return fail(PA_ERR_INVALID_ARGUMENT, "null pointer");
    const int b = repr_num_bits(s);
    return b >= 103 ? 4 : b >= 37 ? 3 : 2;
}
int pa_g1_recommended_wnaf_for_num_scalars(size_t num_scalars) {
    static const size_t rec[12] = {1, 3, 7, 20, 43, 120, 273, 563, 1630, 3128, 7933, 62569};
    return window_for_count(num_scalars, rec, 12);
}
int pa_g2_recommended_wnaf_for_num_scalars(size_t num_scalars) {
    static const size_t rec[11] = {1, 3, 8, 20, 47, 126, 260, 826, 1501, 4555, 84071};
    return window_for_count(num_scalars, rec, 11);
}

}  // extern "C"
