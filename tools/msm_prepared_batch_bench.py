#!/usr/bin/env python3
"""Batched G1 multiexp over prepared bases against a loop of single calls.

For each shape (m, k): k scalar vectors of m terms over the same m prepared
bases, timed with device events on one stream and in alternating rounds so
that the variants see the same machine state:
  batch   one pa_g1_multiexp_prepared_batch_device call
  loop    k back-to-back pa_g1_multiexp_prepared_device calls over the same
          vectors, one workspace
Inputs are msm_prepared_bench.py's: distinct bases k_i G made on the device,
random scalars below 2^252.  Every row of the batch is compared as a point
with the loop's before anything is timed.

--root DIR takes the package (and its library) from another checkout of this
project, e.g. the parent commit's build: where that package has no batched
entry only the loop is timed, which separates a change of the loop's own time
from the batch's gain.  k = 1 rows time the single call at that size; the
(2^20, 1) row is the throughput bound a batch of 2^20 terms in all aims at.

The A/B knobs of kernels_msm.hip (PA_MSM_BATCH_C, PA_MSM_BATCH_PARTS,
PA_MSM_GLV_C, PA_MSM_PARTS, ...) are read once per process: run the tool once
per setting; the settings in effect are recorded in the output.

  python tools/msm_prepared_batch_bench.py --out profiles/msm_prepared_batch --tag default
"""
import argparse
import json
import os
import statistics
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KNOBS = ("PA_MSM_BATCH_C", "PA_MSM_BATCH_PARTS", "PA_MSM_GLV_C", "PA_MSM_GLV_LONGSPAN", "PA_MSM_PARTS",
         "PA_MSM_CHUNK", "PA_MSM_WLO", "PA_MSM_CMAX", "PA_MSM_SEG", "PA_LIB_PATH")
SHAPES = "12x1,12x256,16x1,16x4,16x16,16x64,18x1,18x8,20x1,20x4"


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--shapes", default=SHAPES, help="LOG2_M x K, comma separated")
    ap.add_argument("--root", default=ROOT, help="the checkout whose pairing_amd package is timed")
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--rounds", type=int, default=8, help="alternating rounds per shape")
    ap.add_argument("--calls", type=int, default=4, help="timed repeats per variant and round (fewer for large k)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "msm_prepared_batch"))
    ap.add_argument("--tag", default="default")
    args = ap.parse_args()

    sys.path.insert(0, os.path.abspath(args.root))
    import torch
    import pairing_amd as pa
    import pairing_amd.device as pdev
    if pa.device_count() < 1:
        sys.exit("msm_prepared_batch_bench: no HIP device (there is no CPU path to time)")
    has_batch = hasattr(pdev, "multiexp_prepared_batch")
    dev = "cuda"
    d = np.load(os.path.join(ROOT, "tests", "golden", "bench_points.npz"))
    base_np = np.zeros((1, 18), np.uint64)
    base_np[0, :12] = d["g1"][0, :12]
    base_np[0, 12:18] = np.array([0x760900000002fffd, 0xebf4000bc40c0002, 0x5f48985753c758ba,
                                  0x77ce585370525745, 0x5c071a97a256ec6d, 0x15f65ec3fa80e493], np.uint64)
    stream = torch.cuda.current_stream()
    shapes = [tuple(int(v) for v in x.split("x")) for x in args.shapes.split(",")]
    result = {"tag": args.tag, "device": torch.cuda.get_device_name(0), "version": pa.version(),
              "root": os.path.relpath(os.path.abspath(args.root), ROOT), "has_batch_entry": has_batch,
              "knobs": {k: os.environ[k] for k in KNOBS if k in os.environ},
              "warmup": args.warmup, "rounds": args.rounds, "calls": args.calls, "shapes": {}}
    lines = []
    prepared = {}   # log2 m -> (object, single-call workspace)

    def bases_for(lg):
        if lg not in prepared:
            n = 1 << lg
            g = np.random.default_rng(1234)
            k_np = g.integers(0, 1 << 63, size=(n, 4), dtype=np.uint64)
            k_np[:, 0] ^= np.arange(n, dtype=np.uint64)
            k_np[:, 3] &= np.uint64(0x0fffffffffffffff)
            base = torch.from_numpy(base_np.view(np.int64)).to(dev)
            jac = pdev.empty_records(n, 18, dev)
            table, _ = pdev.g1_fixed_base_table(base, stream)
            pdev.g1_fixed_base_mul(table, torch.from_numpy(k_np.view(np.int64)).to(dev), jac, stream)
            pdev.g1_batch_normalization(jac, stream)
            bases = torch.zeros((n, 13), dtype=torch.int64, device=dev)
            bases[:, :12] = jac[:, :12]
            obj = pdev.msm_prepare(bases, stream)
            assert obj.in_subgroup
            prepared[lg] = (obj, pdev.multiexp_prepared_workspace(obj, n, dev))
        return prepared[lg]

    for lg, k in shapes:
        m = 1 << lg
        obj, ws1 = bases_for(lg)
        g = np.random.default_rng(4321 + 1000 * lg + k)
        s_np = g.integers(0, 1 << 63, size=(k * m, 4), dtype=np.uint64)
        s_np[:, 3] &= np.uint64(0x0fffffffffffffff)
        scal = torch.from_numpy(s_np.view(np.int64)).to(dev)
        del s_np
        rows = [scal[j * m:(j + 1) * m] for j in range(k)]
        out_loop = pdev.empty_records(k, 18, dev)
        out_rows = [out_loop[j:j + 1] for j in range(k)]

        def loop():
            for j in range(k):
                pdev.multiexp_prepared(obj, rows[j], out_rows[j], ws1, stream)

        run = {"loop": loop}
        entry = {"m": m, "k": k, "ms": {}}
        if has_batch:
            out_batch = pdev.empty_records(k, 18, dev)
            wsb = pdev.multiexp_prepared_batch_workspace(obj, m, k, dev)
            entry["workspace_bytes"] = int(wsb.numel())
            run["batch"] = lambda: pdev.multiexp_prepared_batch(obj, scal, m, k, out_batch, wsb, stream=stream)
        # same sums first
        for v in run:
            run[v]()
        torch.cuda.synchronize()
        if has_batch:
            same = bool(pa.g1_eq(out_batch.cpu().numpy().view(np.uint64), out_loop.cpu().numpy().view(np.uint64)).all())
            entry["batch_rows_equal_loop_rows_as_points"] = same
            if not same:
                sys.exit("msm_prepared_batch_bench: (2^%d, %d): the batch's rows differ from the loop's" % (lg, k))

        calls = max(1, min(args.calls, 32 // k))
        for v in run:
            for _ in range(args.warmup):
                run[v]()
        torch.cuda.synchronize()
        per_round = {v: [] for v in run}
        for _ in range(args.rounds):
            for v in run:
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record(stream)
                for _ in range(calls):
                    run[v]()
                e1.record(stream)
                e1.synchronize()
                per_round[v].append(e0.elapsed_time(e1) / calls)
        entry["calls"] = calls
        for v in run:
            r = sorted(per_round[v])
            med = statistics.median(r)
            entry["ms"][v] = {"median": med, "min": r[0], "max": r[-1], "rounds": per_round[v],
                              "spread_ms": r[-1] - r[0], "spread_pct": 100.0 * (r[-1] - r[0]) / med,
                              "mterms_per_s": k * m / med / 1e3}
            lines.append("2^%-2d x %-3d %-5s %9.3f ms median  [%8.3f, %8.3f]  spread %6.3f ms (%4.1f %%)  %7.1f M terms/s" %
                         (lg, k, v, med, r[0], r[-1], r[-1] - r[0], entry["ms"][v]["spread_pct"], k * m / med / 1e3))
        if has_batch:
            entry["loop_over_batch"] = entry["ms"]["loop"]["median"] / entry["ms"]["batch"]["median"]
            lines.append("2^%-2d x %-3d loop / batch = %.2f" % (lg, k, entry["loop_over_batch"]))
        result["shapes"]["%dx%d" % (lg, k)] = entry
        del scal, rows, out_loop, out_rows, run
        if has_batch:
            del out_batch, wsb
        torch.cuda.empty_cache()

    # a batch of 2^16 x 16 against the same 2^20 terms in one call
    sh = result["shapes"]
    if has_batch and "16x16" in sh and "20x1" in sh:
        ratio = sh["16x16"]["ms"]["batch"]["median"] / sh["20x1"]["ms"]["loop"]["median"]
        result["batch_16x16_over_single_2^20"] = ratio
        lines.append("2^16 x 16 batch / 2^20 single call = %.2f" % ratio)
    for obj, _ in prepared.values():
        obj.close()

    os.makedirs(args.out, exist_ok=True)
    head = "msm_prepared_batch_bench %s  %s  root %s  knobs %s" % (
        args.tag, result["device"], result["root"], result["knobs"] or "{}")
    text = "\n".join([head] + lines) + "\n"
    with open(os.path.join(args.out, args.tag + ".txt"), "w") as f:
        f.write(text)
    with open(os.path.join(args.out, args.tag + ".json"), "w") as f:
        json.dump(result, f, indent=1)
    sys.stdout.write(text)


if __name__ == "__main__":
    main()
