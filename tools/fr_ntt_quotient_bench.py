#!/usr/bin/env python3
"""Fr NTT quotient: pa_fr_ntt_quotient_device against the transforms alone, one session.

Device-resident, timed with device events on one stream after warm-up (as
tools/fr_ntt_bench.py does): median and max - min over --rounds rounds of
--calls calls, for k polynomial triples of 2^log_n points (--cases log_n:k).

  baseline  the seven transforms from entries every build has: a | b | c staged
            end to end once, outside the timing, then pa_fr_ntt_device inverse
            with batch 3k, coset_forward with batch 3k (in place) and
            coset_inverse with batch k.  The pointwise step (A B - C) / Z is left
            out: a lower bound on any composition of those entries.
  quotient  pa_fr_ntt_quotient_device on a, b, c as three arrays, where the
            library has it.  Before it is timed its result is compared with the
            composition: the baseline's coset evaluations, the host entries
            pa_fr_mul_batch / pa_fr_sub_batch for the pointwise step, and the
            coset-inverse transform of that.

The library is loaded by path (--lib), not through the package, so that the
same tool times a build without the quotient: there the quotient is skipped.

  python tools/fr_ntt_quotient_bench.py --out profiles/fr_ntt_quotient --tag default
  python tools/fr_ntt_quotient_bench.py --lib <parent build's libpairing_amd.so> --tag parent
"""
import argparse
import ctypes
import json
import os
import statistics
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
R_ORDER = 0x73eda753299d7d483339d80809a1d80553bda402fffe5bfeffffffff00000001
TOP = 0x73eda753299d7d48   # rows with a top limb below r's are below r
INVERSE, COSET_FORWARD, COSET_INVERSE = 1, 2, 3   # PA_NTT_* of the header


def fr_rows(seed, n):
    g = np.random.default_rng(seed)
    a = g.integers(0, 1 << 63, size=(n, 4), dtype=np.uint64) * np.uint64(2) + g.integers(0, 2, size=(n, 4), dtype=np.uint64)
    a[:, 3] %= np.uint64(TOP)
    return a


def load(path):
    lib = ctypes.CDLL(path)
    p, n = ctypes.c_void_p, ctypes.c_size_t
    lib.pa_last_error.restype = ctypes.c_char_p
    lib.pa_fr_ntt_domain_create.argtypes = [ctypes.c_uint, ctypes.POINTER(p)]
    lib.pa_fr_ntt_domain_free.argtypes = [p]
    lib.pa_fr_ntt_domain_free.restype = None
    lib.pa_fr_ntt_domain_passes.argtypes = [p]
    lib.pa_fr_ntt_domain_passes.restype = ctypes.c_uint
    lib.pa_fr_ntt_workspace_bytes.argtypes = [p, n]
    lib.pa_fr_ntt_workspace_bytes.restype = n
    lib.pa_fr_ntt_device.argtypes = [p, ctypes.c_int, p, p, n, p, n, p]
    lib.pa_fr_mul_batch.argtypes = [p, p, p, n]
    lib.pa_fr_sub_batch.argtypes = [p, p, p, n]
    has_quotient = hasattr(lib, "pa_fr_ntt_quotient_device")
    if has_quotient:
        lib.pa_fr_ntt_quotient_workspace_bytes.argtypes = [p, n]
        lib.pa_fr_ntt_quotient_workspace_bytes.restype = n
        lib.pa_fr_ntt_quotient_device.argtypes = [p, p, p, p, p, n, p, n, p]
    return lib, has_quotient


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--lib", default=os.path.join(ROOT, "pairing_amd", "lib", "libpairing_amd.so"))
    ap.add_argument("--cases", default="20:1,16:16,12:256", help="log_n:k, comma separated")
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--rounds", type=int, default=8)
    ap.add_argument("--calls", type=int, default=8, help="timed calls per round")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "fr_ntt_quotient"))
    ap.add_argument("--tag", default="default")
    ap.add_argument("--against", help="the .json of an earlier run (the parent build's, same session): the bound is "
                    "taken from its baseline instead of this run's")
    args = ap.parse_args()

    import torch
    if not torch.cuda.is_available():
        sys.exit("fr_ntt_quotient_bench: no HIP device (there is no CPU path to time)")
    lib, has_quotient = load(args.lib)
    against = {}
    if args.against:
        with open(args.against) as f:
            against = {(c["log_n"], c["k"]): c["ms"]["baseline"] for c in json.load(f)["cases"]}
    dev = "cuda"
    stream = torch.cuda.current_stream()
    sp = ctypes.c_void_p(stream.cuda_stream)

    def ok(rc, what):
        if rc != 0:
            sys.exit("fr_ntt_quotient_bench: %s failed (%d): %s" % (what, rc, lib.pa_last_error().decode()))

    def ptr(t, row=0):
        return ctypes.c_void_p(t.data_ptr() + 32 * row)

    def timed(fn):
        for _ in range(args.warmup):
            fn()
        torch.cuda.synchronize()
        per_round = []
        for _ in range(args.rounds):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(stream)
            for _ in range(args.calls):
                fn()
            e1.record(stream)
            e1.synchronize()
            per_round.append(e0.elapsed_time(e1) / args.calls)
        r = sorted(per_round)
        return {"median": statistics.median(r), "min": r[0], "max": r[-1], "spread": r[-1] - r[0], "rounds": per_round}

    result = {"tag": args.tag, "device": torch.cuda.get_device_name(0), "lib": os.path.basename(args.lib),
              "has_quotient": has_quotient, "warmup": args.warmup, "rounds": args.rounds, "calls": args.calls,
              "cases": []}
    lines = ["fr_ntt_quotient_bench %s  %s  quotient entry: %s" %
             (args.tag, result["device"], "yes" if has_quotient else "absent (baseline only)")]
    print(lines[0], flush=True)

    def emit(line):
        lines.append(line)
        print(line, flush=True)

    for case in args.cases.split(","):
        lg, k = (int(x) for x in case.split(":"))
        n = 1 << lg
        rows = k * n
        h = ctypes.c_void_p(0)
        ok(lib.pa_fr_ntt_domain_create(lg, ctypes.byref(h)), "pa_fr_ntt_domain_create")
        passes = lib.pa_fr_ntt_domain_passes(h)
        staged = torch.from_numpy(fr_rows(300 + lg, 3 * rows).view(np.int64)).to(dev)   # a | b | c
        ev = torch.empty_like(staged)
        out = torch.empty((rows, 4), dtype=torch.int64, device=dev)
        nws_bytes = lib.pa_fr_ntt_workspace_bytes(h, 3 * k)
        nws = torch.empty(max(nws_bytes // 8, 1), dtype=torch.int64, device=dev)

        def baseline():
            ok(lib.pa_fr_ntt_device(h, INVERSE, ptr(staged), ptr(ev), 3 * k, ptr(nws), nws_bytes, sp), "inverse")
            ok(lib.pa_fr_ntt_device(h, COSET_FORWARD, ptr(ev), ptr(ev), 3 * k, ptr(nws), nws_bytes, sp), "coset_forward")
            ok(lib.pa_fr_ntt_device(h, COSET_INVERSE, ptr(ev), ptr(out), k, ptr(nws), nws_bytes, sp), "coset_inverse")

        entry = {"log_n": lg, "k": k, "passes": passes, "launches": {"baseline": 3 * passes}, "ms": {}}
        entry["ms"]["baseline"] = base = timed(baseline)
        emit("%4d x 2^%-2d passes %d  baseline (7 transforms, no pointwise step) %9.4f ms median, max - min %7.4f" %
             (k, lg, passes, base["median"], base["spread"]))
        if has_quotient:
            qws_bytes = lib.pa_fr_ntt_quotient_workspace_bytes(h, k)
            qws = torch.empty(max(qws_bytes // 8, 1), dtype=torch.int64, device=dev)
            hq = torch.empty_like(out)

            def quotient():
                ok(lib.pa_fr_ntt_quotient_device(h, ptr(staged), ptr(staged, rows), ptr(staged, 2 * rows), ptr(hq), k,
                                                 ptr(qws), qws_bytes, sp), "pa_fr_ntt_quotient_device")

            # the composition, its pointwise step through the host entries
            baseline()
            torch.cuda.synchronize()
            e = np.ascontiguousarray(ev.cpu().numpy().view(np.uint64))
            zinv = pow(pow(7, n, R_ORDER) - 1, -1, R_ORDER) * (1 << 256) % R_ORDER
            z = np.tile(np.array([(zinv >> (64 * i)) & (2 ** 64 - 1) for i in range(4)], np.uint64), (rows, 1))
            t = np.empty((rows, 4), np.uint64)
            hp = lambda x: x.ctypes.data_as(ctypes.c_void_p)  # noqa: E731
            ea, eb, ec = (np.ascontiguousarray(e[i * rows:(i + 1) * rows]) for i in range(3))
            ok(lib.pa_fr_mul_batch(hp(ea), hp(eb), hp(t), rows), "pa_fr_mul_batch")
            ok(lib.pa_fr_sub_batch(hp(t), hp(ec), hp(t), rows), "pa_fr_sub_batch")
            ok(lib.pa_fr_mul_batch(hp(t), hp(z), hp(t), rows), "pa_fr_mul_batch")
            td = torch.from_numpy(t.view(np.int64)).to(dev)
            ok(lib.pa_fr_ntt_device(h, COSET_INVERSE, ptr(td), ptr(out), k, ptr(nws), nws_bytes, sp), "coset_inverse")
            quotient()
            torch.cuda.synchronize()
            if not torch.equal(hq, out):
                sys.exit("fr_ntt_quotient_bench: the quotient differs from the composition at %d x 2^%d" % (k, lg))
            entry["launches"]["quotient"] = 3 * passes if lg else 1
            entry["workspace_bytes"] = qws_bytes
            entry["ms"]["quotient"] = q = timed(quotient)
            ref = against.get((lg, k), base)   # the expectation: no worse than the baseline's median plus the larger spread
            bound = ref["median"] + max(ref["spread"], q["spread"])
            entry["bound_ms"], entry["bound_from"] = bound, args.against if (lg, k) in against else "this run"
            entry["within_bound"] = q["median"] <= bound
            emit("%4d x 2^%-2d passes %d  quotient (checked against the composition)  %9.4f ms median, max - min %7.4f"
                 "  -> %.3f x the baseline, bound %9.4f: %s" %
                 (k, lg, passes, q["median"], q["spread"], q["median"] / ref["median"], bound,
                  "within" if entry["within_bound"] else "MISSES"))
            del qws, hq
        result["cases"].append(entry)
        lib.pa_fr_ntt_domain_free(h)
        del staged, ev, out, nws

    os.makedirs(args.out, exist_ok=True)
    with open(os.path.join(args.out, args.tag + ".txt"), "w") as f:
        f.write("\n".join(lines) + "\n")
    with open(os.path.join(args.out, args.tag + ".json"), "w") as f:
        json.dump(result, f, indent=1)


if __name__ == "__main__":
    main()
