#!/usr/bin/env python3
"""G2 multiexp over prepared bases against the plain entry, single calls and batches.

For each shape (m, k): k scalar vectors of m terms over the same m G2 bases,
timed with device events on one stream and in alternating rounds so that the
variants see the same machine state:
  plain     k back-to-back pa_g2_multiexp_device calls over the affine records
            (the entry that converts the bases per call and walks 257 bits):
            what the prepared entries are compared with
  prepared  k = 1: one pa_g2_multiexp_prepared_device call
            k > 1: k back-to-back such calls, one workspace
  batch     k > 1: one pa_g2_multiexp_prepared_batch_device call
Inputs: distinct bases k_i Q made on the device (fixed-base wNAF and batch
normalization), random scalars below 2^252.  Every result is compared as a
point with the plain entry's before anything is timed.  The time of
pa_g2_msm_bases_prepare_device (membership check, conversion, the stream
synchronized) is recorded per size: host clock around the call, median of
--prepare-reps.  --time batch (a comma list) times only some variants, for
A/B runs; all of them are still run and compared once.

The A/B knobs of kernels_msm.hip (PA_MSM_GLV_C, PA_MSM_BATCH_C,
PA_MSM_GLV_LONGSPAN, ...) are read once per process: run the tool once per
setting; the settings in effect are recorded in the output.

  python tools/msm_g2_prepared_bench.py --out profiles/msm_g2_prepared --tag default
"""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KNOBS = ("PA_MSM_BATCH_C", "PA_MSM_BATCH_PARTS", "PA_MSM_GLV_C", "PA_MSM_GLV_LONGSPAN", "PA_MSM_PARTS",
         "PA_MSM_CHUNK", "PA_MSM_WLO", "PA_MSM_CMAX", "PA_MSM_SEG", "PA_LIB_PATH")
SHAPES = "14x1,16x1,18x1,16x4,14x16,12x64"
# Fq one in Montgomery form: Z = (1, 0) of the Jacobian base record
FQ_ONE = [0x760900000002fffd, 0xebf4000bc40c0002, 0x5f48985753c758ba,
          0x77ce585370525745, 0x5c071a97a256ec6d, 0x15f65ec3fa80e493]


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--shapes", default=SHAPES, help="LOG2_M x K, comma separated")
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--rounds", type=int, default=8, help="alternating rounds per shape")
    ap.add_argument("--calls", type=int, default=4, help="timed repeats per variant and round (fewer for large k)")
    ap.add_argument("--prepare-reps", type=int, default=5)
    ap.add_argument("--time", default="plain,prepared,batch",
                    help="the variants to time (all of them are run and compared once first)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "msm_g2_prepared"))
    ap.add_argument("--tag", default="default")
    args = ap.parse_args()

    sys.path.insert(0, ROOT)
    import torch
    import pairing_amd as pa
    import pairing_amd.device as pdev
    if pa.device_count() < 1:
        sys.exit("msm_g2_prepared_bench: no HIP device (there is no CPU path to time)")
    dev = "cuda"
    d = np.load(os.path.join(ROOT, "tests", "golden", "bench_points.npz"))
    base_np = np.zeros((1, 36), np.uint64)
    base_np[0, :24] = d["g2"][0, :24]
    base_np[0, 24:30] = np.array(FQ_ONE, np.uint64)
    stream = torch.cuda.current_stream()
    shapes = [tuple(int(v) for v in x.split("x")) for x in args.shapes.split(",")]
    result = {"tag": args.tag, "device": torch.cuda.get_device_name(0), "version": pa.version(),
              "knobs": {k: os.environ[k] for k in KNOBS if k in os.environ},
              "warmup": args.warmup, "rounds": args.rounds, "calls": args.calls, "prepare_ms": {}, "shapes": {}}
    lines = []
    sizes = {}   # log2 m -> (affine records, prepared object, prepared workspace, plain workspace)

    def bases_for(lg):
        if lg not in sizes:
            n = 1 << lg
            g = np.random.default_rng(1234)
            k_np = g.integers(0, 1 << 63, size=(n, 4), dtype=np.uint64)
            k_np[:, 0] ^= np.arange(n, dtype=np.uint64)
            k_np[:, 3] &= np.uint64(0x0fffffffffffffff)
            base = torch.from_numpy(base_np.view(np.int64)).to(dev)
            jac = pdev.empty_records(n, 36, dev)
            table, tws = pdev.g2_fixed_base_buffers(dev)
            pdev.g2_wnaf_fixed_base(base, torch.from_numpy(k_np.view(np.int64)).to(dev), jac, table, tws, stream)
            pdev.g2_batch_normalization(jac, stream)
            bases = torch.zeros((n, 25), dtype=torch.int64, device=dev)
            bases[:, :24] = jac[:, :24]
            del jac, table, tws
            reps = []
            for _ in range(args.prepare_reps + 1):   # the first one warms up
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                obj = pdev.g2_msm_prepare(bases, stream)
                reps.append(1e3 * (time.perf_counter() - t0))
                obj.close()
            reps = sorted(reps[1:])
            result["prepare_ms"][str(lg)] = {"median": statistics.median(reps), "min": reps[0], "max": reps[-1]}
            lines.append("2^%-2d prepare   %9.3f ms median  [%8.3f, %8.3f]  (host clock, stream synchronized)" %
                         (lg, statistics.median(reps), reps[0], reps[-1]))
            obj = pdev.g2_msm_prepare(bases, stream)
            assert obj.in_subgroup
            sizes[lg] = (bases, obj, pdev.g2_multiexp_prepared_workspace(obj, n, dev),
                         pdev.multiexp_workspace(2, n, dev))
        return sizes[lg]

    for lg, k in shapes:
        m = 1 << lg
        bases, obj, ws1, wsp = bases_for(lg)
        g = np.random.default_rng(4321 + 1000 * lg + k)
        s_np = g.integers(0, 1 << 63, size=(k * m, 4), dtype=np.uint64)
        s_np[:, 3] &= np.uint64(0x0fffffffffffffff)
        scal = torch.from_numpy(s_np.view(np.int64)).to(dev)
        del s_np
        rows = [scal[j * m:(j + 1) * m] for j in range(k)]
        outs = {v: pdev.empty_records(k, 36, dev) for v in ("plain", "prepared", "batch")}

        def plain():
            for j in range(k):
                pdev.multiexp(2, bases, rows[j], outs["plain"][j:j + 1], wsp, stream)

        def prepared():
            for j in range(k):
                pdev.g2_multiexp_prepared(obj, rows[j], outs["prepared"][j:j + 1], ws1, stream)

        run = {"plain": plain, "prepared": prepared}
        entry = {"m": m, "k": k, "ms": {}}
        if k > 1:
            wsb = pdev.g2_multiexp_prepared_batch_workspace(obj, m, k, dev)
            entry["workspace_bytes"] = int(wsb.numel())
            run["batch"] = lambda: pdev.g2_multiexp_prepared_batch(obj, scal, m, k, outs["batch"], wsb, stream=stream)
        # same sums first
        for v in run:
            run[v]()
        torch.cuda.synchronize()
        want = outs["plain"].cpu().numpy().view(np.uint64)
        for v in run:
            if not bool(pa.g2_eq(outs[v].cpu().numpy().view(np.uint64), want).all()):
                sys.exit("msm_g2_prepared_bench: (2^%d, %d): %s differs from the plain entry" % (lg, k, v))
        entry["equal_to_plain_as_points"] = True

        run = {v: run[v] for v in run if v in args.time.split(",")}
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
            lines.append("2^%-2d x %-3d %-8s %9.3f ms median  [%8.3f, %8.3f]  spread %6.3f ms (%4.1f %%)  %7.1f M terms/s" %
                         (lg, k, v, med, r[0], r[-1], r[-1] - r[0], entry["ms"][v]["spread_pct"], k * m / med / 1e3))
        best = "batch" if k > 1 else "prepared"
        if "plain" in run and best in run:
            entry["plain_over_" + best] = entry["ms"]["plain"]["median"] / entry["ms"][best]["median"]
            lines.append("2^%-2d x %-3d plain / %s = %.2f" % (lg, k, best, entry["plain_over_" + best]))
        result["shapes"]["%dx%d" % (lg, k)] = entry
        del scal, rows, outs, run
        torch.cuda.empty_cache()

    for _, obj, _, _ in sizes.values():
        obj.close()

    os.makedirs(args.out, exist_ok=True)
    head = "msm_g2_prepared_bench %s  %s  knobs %s" % (args.tag, result["device"], result["knobs"] or "{}")
    text = "\n".join([head] + lines) + "\n"
    with open(os.path.join(args.out, args.tag + ".txt"), "w") as f:
        f.write(text)
    with open(os.path.join(args.out, args.tag + ".json"), "w") as f:
        json.dump(result, f, indent=1)
    sys.stdout.write(text)


if __name__ == "__main__":
    main()
