#!/usr/bin/env python3
"""Batched multi-pairing (m products of k pairs in one call) against what a
caller had before it, one session.

Per shape (k, m), n = k m pairs from bench.make_pairs resident in HBM, timed with
device events on one stream in alternating rounds so that the variants see the
same machine state:
  batch     pa_multi_pairing_batch_device: n Miller loops, the segmented
            product, m final exponentiations, the is_one compare
  pairing   pa_pairing_batch_device over the same n pairs (n final
            exponentiations; the per-check products would still be the caller's)
  ml        pa_pairing_miller_loop_batch_device over n, alone
  fe        pa_final_exponentiation_batch_device over m, alone
ml + fe is the floor of `batch`; batch - (ml + fe) is what the segmented product,
the compare and the offsets staging cost.  Before anything is timed the first and
last product are compared with pa_multi_pairing_device on the same pairs.

Every shape runs in a child process of its own under `timeout`; the first
non-zero status ends the run.  PA_SEGPROD_SERIAL_MAX (the short/long threshold
of kernels_segprod.hip) is read once per process and recorded.

  python tools/multi_pairing_batch_bench.py --out profiles/multi_pairing_batch --tag default
"""
import argparse
import json
import os
import statistics
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SHAPES = "2x32768,4x16384,2x1024,3x64"
KNOBS = ("PA_SEGPROD_SERIAL_MAX", "PA_PAIRING_KERNEL", "PA_PQ_MIN", "PA_PQ_MAX", "PA_COOP_MAX", "PA_PAIR_MAX")
VARIANTS = ("batch", "pairing", "ml", "fe")


def run_shape(k, m, args):
    """one shape in this process; returns its result entry"""
    import torch
    import bench
    import pairing_amd as pa
    import pairing_amd.device as pdev
    if pa.device_count() < 1:
        sys.exit("multi_pairing_batch_bench: no HIP device (there is no CPU path to time)")
    dev = "cuda"
    n = k * m
    stream = torch.cuda.current_stream()
    p_np, q_np = bench.make_pairs(n, 0)
    p = torch.from_numpy(p_np.view(np.int64)).to(dev)
    q = torch.from_numpy(q_np.view(np.int64)).to(dev)
    offsets = np.arange(m + 1, dtype=np.uint64) * np.uint64(k)
    out = pdev.empty_records(m, 72, dev)
    ok = torch.zeros(m, dtype=torch.uint8, device=dev)
    is_one = torch.zeros(m, dtype=torch.uint8, device=dev)
    work = torch.empty(pdev.multi_pairing_batch_workspace_words(n, m), dtype=torch.int64, device=dev)
    pair_out, scratch = pdev.empty_records(n, 72, dev), pdev.empty_records(n, 72, dev)
    fe_in, fe_out = pdev.empty_records(m, 72, dev), pdev.empty_records(m, 72, dev)
    pdev.pairing_miller_loop(p[:m], q[:m], fe_in, stream)
    run = {"batch": lambda: pdev.multi_pairing_batch(p, q, offsets, out, ok, is_one, work, stream),
           "pairing": lambda: pdev.pairing(p, q, pair_out, scratch, stream),
           "ml": lambda: pdev.pairing_miller_loop(p, q, scratch, stream),
           "fe": lambda: pdev.final_exponentiation(fe_in, fe_out, None, stream)}

    # same values as the single-product entry first
    run["batch"]()
    one_out, one_ok = pdev.empty_records(1, 72, dev), torch.zeros(1, dtype=torch.uint8, device=dev)
    one_work = pdev.empty_records(k, 72, dev)
    for j in (0, m - 1):
        pdev.multi_pairing(p[j * k:(j + 1) * k], q[j * k:(j + 1) * k], one_out, one_ok, one_work, stream)
        torch.cuda.synchronize()
        if not (torch.equal(one_out[0], out[j]) and int(one_ok[0]) == int(ok[j])):
            sys.exit("multi_pairing_batch_bench: product %d differs from pa_multi_pairing_device" % j)

    for v in VARIANTS:
        for _ in range(args.warmup):
            run[v]()
    torch.cuda.synchronize()
    per_round = {v: [] for v in VARIANTS}
    for _ in range(args.rounds):
        for v in VARIANTS:
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(stream)
            for _ in range(args.calls):
                run[v]()
            e1.record(stream)
            e1.synchronize()
            per_round[v].append(e0.elapsed_time(e1) / args.calls)
    entry = {"k": k, "m": m, "n": n, "device": torch.cuda.get_device_name(0), "version": pa.version(),
             "steps": args.rounds * args.calls, "warmup": args.warmup, "ok_all": bool(ok.all()),
             "is_one_count": int(is_one.sum()), "ms": {}}
    for v in VARIANTS:
        r = sorted(per_round[v])
        med = statistics.median(r)
        entry["ms"][v] = {"median": med, "min": r[0], "max": r[-1], "rounds": per_round[v],
                          "spread_pct": 100.0 * (r[-1] - r[0]) / med}
    ms = {v: entry["ms"][v]["median"] for v in VARIANTS}
    entry["floor_ms"] = ms["ml"] + ms["fe"]
    entry["product_and_compare_ms"] = ms["batch"] - entry["floor_ms"]
    entry["batch_vs_pairing"] = ms["pairing"] / ms["batch"]
    entry["checks_per_s"] = m / ms["batch"] * 1e3
    return entry


def lines_of(e):
    ms = e["ms"]
    out = ["k=%d m=%-6d %-8s %8.3f ms median  [%7.3f, %7.3f]  spread %4.1f %%" %
           (e["k"], e["m"], v, ms[v]["median"], ms[v]["min"], ms[v]["max"], ms[v]["spread_pct"]) for v in VARIANTS]
    out.append("k=%d m=%-6d floor ml + fe %.3f ms; product + compare %+.3f ms; batch is %.2fx pairing over the "
               "same %d pairs; %.0f checks/s" % (e["k"], e["m"], e["floor_ms"], e["product_and_compare_ms"],
                                                 e["batch_vs_pairing"], e["n"], e["checks_per_s"]))
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--shapes", default=SHAPES, help="comma list of KxM (pairs per product x products)")
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--rounds", type=int, default=5, help="alternating rounds per shape")
    ap.add_argument("--calls", type=int, default=5, help="timed calls per variant and round")
    ap.add_argument("--timeout", type=int, default=150, help="seconds per shape (its own child process)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "multi_pairing_batch"))
    ap.add_argument("--tag", default="default")
    ap.add_argument("--child", help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.rounds * args.calls < 20:
        sys.exit("multi_pairing_batch_bench: rounds x calls must give at least 20 timed steps")

    if args.child:
        k, m = (int(x) for x in args.child.split("x"))
        json.dump(run_shape(k, m, args), sys.stdout)
        return

    result = {"tag": args.tag, "knobs": {k: os.environ[k] for k in KNOBS if k in os.environ}, "shapes": []}
    lines = []
    for shape in args.shapes.split(","):
        cmd = ["timeout", "-k", "10", str(args.timeout), sys.executable, os.path.abspath(__file__), "--child", shape,
               "--warmup", str(args.warmup), "--rounds", str(args.rounds), "--calls", str(args.calls)]
        r = subprocess.run(cmd, stdout=subprocess.PIPE, text=True)
        if r.returncode != 0:
            sys.stderr.write(r.stdout)
            sys.exit("multi_pairing_batch_bench: shape %s ended with status %d; stopping" % (shape, r.returncode))
        entry = json.loads(r.stdout.strip().splitlines()[-1])
        result["shapes"].append(entry)
        result["device"], result["version"] = entry["device"], entry["version"]
        lines += lines_of(entry)
        print("\n".join(lines_of(entry)), flush=True)

    os.makedirs(args.out, exist_ok=True)
    head = "multi_pairing_batch_bench %s  %s  knobs %s" % (args.tag, result["device"], result["knobs"] or "{}")
    with open(os.path.join(args.out, args.tag + ".txt"), "w") as f:
        f.write("\n".join([head] + lines) + "\n")
    with open(os.path.join(args.out, args.tag + ".json"), "w") as f:
        json.dump(result, f, indent=1)


if __name__ == "__main__":
    main()
