#!/usr/bin/env python3
"""Fr NTT: device-resident transforms against their two floors, one session.

Times pa_fr_ntt_device with device events on one stream after warm-up (as
tools/msm_prepared_bench.py does), for forward and coset-inverse transforms at
the sizes of --cases (log_n:batch), under each tile log of --tiles
(PA_NTT_TILE_LOG is read when a domain is created, so one process can compare
them; 1 is one butterfly stage per launch, the naive comparison).  Every
(size, tile) result is first compared with the default tile's, and the default
round trip inverse(forward(a)) == a is checked, before anything is timed.

Beside each figure, from the same session:
  memory floor      passes x 2 x 32 B x n x batch over the device-to-device copy
                    bandwidth (a 256 MiB torch copy, read + write counted)
  arithmetic floor  (n / 2) log_n batch products at the rate of a register-
                    resident multiply loop: pa_fr_pow_batch over 2^20 elements
                    with two all-ones exponent lengths, the difference of the
                    two times (which cancels the copies) over the difference
                    of the product counts

  python tools/fr_ntt_bench.py --out profiles/fr_ntt --tag default
"""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

R_ORDER = 0x73eda753299d7d483339d80809a1d80553bda402fffe5bfeffffffff00000001
TOP = 0x73eda753299d7d48   # rows with a top limb below r's are below r


def fr_rows(seed, n):
    g = np.random.default_rng(seed)
    a = g.integers(0, 1 << 63, size=(n, 4), dtype=np.uint64) * np.uint64(2) + g.integers(0, 2, size=(n, 4), dtype=np.uint64)
    a[:, 3] %= np.uint64(TOP)
    return a


def copy_bandwidth(torch, stream):
    """bytes moved per second (read + write) by a 256 MiB device-to-device copy"""
    src = torch.empty(256 << 20, dtype=torch.uint8, device="cuda")
    dst = torch.empty_like(src)
    for _ in range(3):
        dst.copy_(src)
    best = None
    for _ in range(5):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(stream)
        for _ in range(4):
            dst.copy_(src)
        e1.record(stream)
        e1.synchronize()
        ms = e0.elapsed_time(e1) / 4
        best = ms if best is None else min(best, ms)
    return 2.0 * src.numel() / (best * 1e-3)


def mul_rate(pa):
    """products per second of a register-resident Fr multiply loop"""
    n = 1 << 20
    a = fr_rows(5, n)
    times = {}
    for words in (16, 48):
        exp = np.full(words, 0xffffffffffffffff, np.uint64)   # a square and a multiply per bit
        pa.fr_pow(a, exp)
        best = None
        for _ in range(4):
            t0 = time.perf_counter()
            pa.fr_pow(a, exp)
            dt = time.perf_counter() - t0
            best = dt if best is None else min(best, dt)
        times[words] = best
    products = n * 2 * 64 * (48 - 16)
    return products / (times[48] - times[16]), times


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--cases", default="12:1,16:1,20:1,24:1,12:256,8:4096", help="log_n:batch, comma separated")
    ap.add_argument("--tiles", default="10,1,8,9,11,12", help="tile logs; the first is the one the others are checked against")
    ap.add_argument("--modes", default="forward,coset_inverse")
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--rounds", type=int, default=8)
    ap.add_argument("--calls", type=int, default=8, help="timed calls per round")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "fr_ntt"))
    ap.add_argument("--tag", default="default")
    args = ap.parse_args()

    import torch
    import pairing_amd as pa
    import pairing_amd.device as pdev
    if pa.device_count() < 1:
        sys.exit("fr_ntt_bench: no HIP device (there is no CPU path to time)")
    dev = "cuda"
    stream = torch.cuda.current_stream()
    tiles = [int(t) for t in args.tiles.split(",")]
    modes = args.modes.split(",")
    bw = copy_bandwidth(torch, stream)
    rate, pow_times = mul_rate(pa)
    result = {"tag": args.tag, "device": torch.cuda.get_device_name(0), "version": pa.version(),
              "copy_bytes_per_s": bw, "fr_mul_per_s": rate, "fr_pow_seconds": {str(k): v for k, v in pow_times.items()},
              "warmup": args.warmup, "rounds": args.rounds, "calls": args.calls, "cases": []}
    lines = ["fr_ntt_bench %s  %s" % (args.tag, result["device"]),
             "device-to-device copy %.0f GB/s (read + write)   register-resident fr_mul %.1f G products/s" %
             (bw / 1e9, rate / 1e9)]
    print("\n".join(lines), flush=True)

    def emit(line):
        lines.append(line)
        print(line, flush=True)

    for case in args.cases.split(","):
        lg, batch = (int(x) for x in case.split(":"))
        n = 1 << lg
        a = torch.from_numpy(fr_rows(100 + lg, n * batch).view(np.int64)).to(dev)
        out = torch.empty_like(a)
        back = torch.empty_like(a)
        want = {}
        arith_ms = (n // 2) * lg * batch / rate * 1e3
        for tile in tiles:
            os.environ["PA_NTT_TILE_LOG"] = str(tile)
            d = pa.fr_ntt_domain(lg)
            words = pdev.fr_ntt_workspace_words(d, batch)
            ws = torch.empty(max(words, 1), dtype=torch.int64, device=dev)
            entry = {"log_n": lg, "batch": batch, "tile_log": d.tile_log, "passes": d.passes,
                     "domain_bytes": d.bytes, "workspace_bytes": words * 8, "ms": {}}
            mem_ms = d.passes * 2 * 32 * n * batch / bw * 1e3
            entry["memory_floor_ms"], entry["arithmetic_floor_ms"] = mem_ms, arith_ms
            for mode in modes:
                pdev.fr_ntt(d, a, out, mode, workspace=ws, stream=stream)
                torch.cuda.synchronize()
                if mode not in want:
                    want[mode] = out.clone()
                    if mode == "forward":
                        pdev.fr_ntt(d, out, back, "inverse", workspace=ws, stream=stream)
                        torch.cuda.synchronize()
                        if not torch.equal(back, a):
                            sys.exit("fr_ntt_bench: inverse(forward(a)) != a at 2^%d" % lg)
                elif not torch.equal(out, want[mode]):
                    sys.exit("fr_ntt_bench: tile log %d differs from tile log %d at 2^%d %s" % (tile, tiles[0], lg, mode))
                for _ in range(args.warmup):
                    pdev.fr_ntt(d, a, out, mode, workspace=ws, stream=stream)
                torch.cuda.synchronize()
                per_round = []
                for _ in range(args.rounds):
                    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    e0.record(stream)
                    for _ in range(args.calls):
                        pdev.fr_ntt(d, a, out, mode, workspace=ws, stream=stream)
                    e1.record(stream)
                    e1.synchronize()
                    per_round.append(e0.elapsed_time(e1) / args.calls)
                r = sorted(per_round)
                med = statistics.median(r)
                entry["ms"][mode] = {"median": med, "min": r[0], "max": r[-1], "rounds": per_round}
                floor = max(mem_ms, arith_ms)
                emit("2^%-2d x %-4d tile %-2d passes %-2d %-13s %9.4f ms median [%9.4f, %9.4f]  floors: memory %8.4f"
                             " arithmetic %8.4f  -> %5.2f x the %s floor" %
                             (lg, batch, d.tile_log, d.passes, mode, med, r[0], r[-1], mem_ms, arith_ms, med / floor,
                              "memory" if mem_ms >= arith_ms else "arithmetic"))
            result["cases"].append(entry)
            d.close()
            del ws
        del a, out, back, want

    os.makedirs(args.out, exist_ok=True)
    text = "\n".join(lines) + "\n"
    with open(os.path.join(args.out, args.tag + ".txt"), "w") as f:
        f.write(text)
    with open(os.path.join(args.out, args.tag + ".json"), "w") as f:
        json.dump(result, f, indent=1)


if __name__ == "__main__":
    main()
