#!/usr/bin/env python3
"""G1 multiexp: the plain entry against the prepared-bases entry, one session.

Times, with device events on one stream and in alternating rounds so that the
variants see the same machine state:
  plain     pa_g1_multiexp_device (bases converted per call, 257-bit windows)
  glv       pa_g1_multiexp_prepared_device, every base in G1 (two 130-bit
            halves per scalar over the prepared rows)
  fallback  pa_g1_multiexp_prepared_device with one base outside G1 (257-bit
            windows over the prepared rows)
and the one-off preparation (host clock; it synchronizes).  Inputs are
bench.py --workload msm's: distinct bases k_i G made on the device, random
scalars below 2^252.  Every variant's sum is compared as a point with the
plain entry's before anything is timed.

The A/B knobs of kernels_msm.hip (PA_MSM_GLV_C, PA_MSM_PARTS, PA_MSM_CHUNK, ...)
are read once per process: run the tool once per setting; the settings in
effect are recorded in the output.

  python tools/msm_prepared_bench.py --out profiles/msm_prepared --tag default
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

Q = 0x1a0111ea397fe69a4b1ba7b6434bacd764774b84f38512bf6730d2a0f6b0f6241eabfffeb153ffffb9feffffffffaaab
R_ORDER = 0x73eda753299d7d483339d80809a1d80553bda402fffe5bfeffffffff00000001
KNOBS = ("PA_MSM_GLV_C", "PA_MSM_GLV_LONGSPAN", "PA_MSM_PARTS", "PA_MSM_CHUNK", "PA_MSM_WLO", "PA_MSM_CMAX", "PA_MSM_SEG")


def point_outside_g1():
    """an affine record of a curve point y^2 = x^3 + 4 outside G1 (q = 3 mod 4 roots)"""
    def mul(P, k):
        acc = None
        for bit in bin(k)[2:]:
            acc = add(acc, acc)
            if bit == "1":
                acc = add(acc, P)
        return acc

    def add(P, S):
        if P is None or S is None:
            return S if P is None else P
        (x1, y1), (x2, y2) = P, S
        if x1 == x2:
            if (y1 + y2) % Q == 0:
                return None
            lam = 3 * x1 * x1 * pow(2 * y1, -1, Q) % Q
        else:
            lam = (y2 - y1) * pow(x2 - x1, -1, Q) % Q
        x3 = (lam * lam - x1 - x2) % Q
        return x3, (lam * (x1 - x3) - y1) % Q

    x = 5
    while True:
        rhs = (x * x * x + 4) % Q
        y = pow(rhs, (Q + 1) // 4, Q)
        if y * y % Q == rhs and mul((x, y), R_ORDER) is not None:
            mont = lambda v: [(v << 384) % Q >> (64 * i) & 0xffffffffffffffff for i in range(6)]
            return np.array(mont(x) + mont(y) + [0], np.uint64)
        x += 1


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--sizes", default="16,18,20", help="log2 term counts")
    ap.add_argument("--variants", default="plain,glv,fallback")
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--rounds", type=int, default=12, help="alternating rounds per size")
    ap.add_argument("--calls", type=int, default=8, help="timed calls per variant and round")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "msm_prepared"))
    ap.add_argument("--tag", default="default")
    args = ap.parse_args()

    import torch
    import pairing_amd as pa
    import pairing_amd.device as pdev
    if pa.device_count() < 1:
        sys.exit("msm_prepared_bench: no HIP device (there is no CPU path to time)")
    dev = "cuda"
    variants = args.variants.split(",")
    d = np.load(os.path.join(ROOT, "tests", "golden", "bench_points.npz"))
    base_np = np.zeros((1, 18), np.uint64)
    base_np[0, :12] = d["g1"][0, :12]
    base_np[0, 12:18] = np.array([0x760900000002fffd, 0xebf4000bc40c0002, 0x5f48985753c758ba,
                                  0x77ce585370525745, 0x5c071a97a256ec6d, 0x15f65ec3fa80e493], np.uint64)
    outside = torch.from_numpy(point_outside_g1().view(np.int64)).to(dev)
    stream = torch.cuda.current_stream()
    result = {"tag": args.tag, "device": torch.cuda.get_device_name(0), "version": pa.version(),
              "knobs": {k: os.environ[k] for k in KNOBS if k in os.environ},
              "warmup": args.warmup, "rounds": args.rounds, "calls": args.calls, "sizes": {}}
    lines = []
    for lg in [int(x) for x in args.sizes.split(",")]:
        n = 1 << lg
        g = np.random.default_rng(1234)
        k_np = g.integers(0, 1 << 63, size=(n, 4), dtype=np.uint64)
        s_np = g.integers(0, 1 << 63, size=(n, 4), dtype=np.uint64)
        k_np[:, 0] ^= np.arange(n, dtype=np.uint64)
        k_np[:, 3] &= np.uint64(0x0fffffffffffffff)
        s_np[:, 3] &= np.uint64(0x0fffffffffffffff)
        base = torch.from_numpy(base_np.view(np.int64)).to(dev)
        jac = pdev.empty_records(n, 18, dev)
        table, _ = pdev.g1_fixed_base_table(base, stream)
        pdev.g1_fixed_base_mul(table, torch.from_numpy(k_np.view(np.int64)).to(dev), jac, stream)
        pdev.g1_batch_normalization(jac, stream)
        bases = torch.zeros((n, 13), dtype=torch.int64, device=dev)
        bases[:, :12] = jac[:, :12]
        del jac, table
        bases_out = bases.clone()
        bases_out[n // 2] = outside
        scal = torch.from_numpy(s_np.view(np.int64)).to(dev)
        torch.cuda.synchronize()

        prep_ms = []
        objs = {}
        for name, src in (("glv", bases), ("fallback", bases_out)):
            for _ in range(3):
                if name in objs:
                    objs[name].close()
                t0 = time.perf_counter()
                objs[name] = pdev.msm_prepare(src, stream)
                prep_ms.append((name, (time.perf_counter() - t0) * 1e3))
        assert objs["glv"].in_subgroup and not objs["fallback"].in_subgroup

        outs = {v: pdev.empty_records(1, 18, dev) for v in ("plain", "plain_out", "glv", "fallback")}
        ws = {"plain": pdev.multiexp_workspace(1, n, dev),
              "glv": pdev.multiexp_prepared_workspace(objs["glv"], n, dev),
              "fallback": pdev.multiexp_prepared_workspace(objs["fallback"], n, dev)}
        run = {"plain": lambda: pdev.multiexp(1, bases, scal, outs["plain"], ws["plain"], stream),
               "glv": lambda: pdev.multiexp_prepared(objs["glv"], scal, outs["glv"], ws["glv"], stream),
               "fallback": lambda: pdev.multiexp_prepared(objs["fallback"], scal, outs["fallback"], ws["fallback"],
                                                          stream)}
        # same sums first
        pdev.multiexp(1, bases_out, scal, outs["plain_out"], ws["plain"], stream)
        for v in run:
            run[v]()
        torch.cuda.synchronize()
        host = {k: t.cpu().numpy().view(np.uint64) for k, t in outs.items()}
        same = {"glv": bool(pa.g1_eq(host["glv"], host["plain"]).all()),
                "fallback": bool(pa.g1_eq(host["fallback"], host["plain_out"]).all())}
        if not all(same.values()):
            sys.exit("msm_prepared_bench: sums differ from the plain entry's: %r" % same)

        for v in variants:
            for _ in range(args.warmup):
                run[v]()
        torch.cuda.synchronize()
        per_round = {v: [] for v in variants}
        for _ in range(args.rounds):
            for v in variants:
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record(stream)
                for _ in range(args.calls):
                    run[v]()
                e1.record(stream)
                e1.synchronize()
                per_round[v].append(e0.elapsed_time(e1) / args.calls)
        entry = {"n": n, "same_point_as_plain": same, "ms": {},
                 "workspace_bytes": {k: int(t.numel()) for k, t in ws.items()},
                 "prepare_ms": {name: min(t for k, t in prep_ms if k == name) for name in ("glv", "fallback")}}
        for v in variants:
            r = sorted(per_round[v])
            med = statistics.median(r)
            entry["ms"][v] = {"median": med, "min": r[0], "max": r[-1], "rounds": per_round[v],
                              "spread_pct": 100.0 * (r[-1] - r[0]) / med, "mterms_per_s": n / med / 1e3}
            lines.append("2^%d %-8s %8.3f ms median  [%7.3f, %7.3f]  spread %4.1f %%  %7.1f M terms/s" %
                         (lg, v, med, r[0], r[-1], entry["ms"][v]["spread_pct"], n / med / 1e3))
        if "plain" in variants:
            for v in variants:
                if v != "plain":
                    rel = 100.0 * (entry["ms"]["plain"]["median"] / entry["ms"][v]["median"] - 1.0)
                    entry["ms"][v]["faster_than_plain_pct"] = rel
                    lines.append("2^%d %-8s %+5.1f %% against plain" % (lg, v, rel))
        lines.append("2^%d prepare  %8.3f ms (all in G1)  %8.3f ms (one base outside)" %
                     (lg, entry["prepare_ms"]["glv"], entry["prepare_ms"]["fallback"]))
        result["sizes"][str(lg)] = entry
        for o in objs.values():
            o.close()
        del bases, bases_out, scal, ws, outs

    os.makedirs(args.out, exist_ok=True)
    head = "msm_prepared_bench %s  %s  knobs %s" % (args.tag, result["device"], result["knobs"] or "{}")
    text = "\n".join([head] + lines) + "\n"
    with open(os.path.join(args.out, args.tag + ".txt"), "w") as f:
        f.write(text)
    with open(os.path.join(args.out, args.tag + ".json"), "w") as f:
        json.dump(result, f, indent=1)
    sys.stdout.write(text)


if __name__ == "__main__":
    main()
