#!/usr/bin/env python3
"""Groth16 parameter generation: pa_groth16_generate_device, its stages, and what a build without it can do.

Device-resident, timed with device events on one stream after warm-up: median
and max - min over --rounds rounds of --calls calls, for a system of n = 2^log_n
rows and n variables with three terms per row in each matrix and n_public = 4
(--cases log_n, comma separated).

  baseline  entries every build has, over scalars staged outside the timing:
            pa_g1_wnaf_fixed_base_device over 3 n_vars + n + 2 scalars,
            pa_g2_wnaf_fixed_base_device over n_vars + 3, and the two batch
            normalizations.  No Fr work and no affine records: a lower bound on
            any composition.
  generate  pa_groth16_generate_device, where the library has it, and its stages
            through the entries that reach them: the Fr half as one call
            (pa_groth16_generate_scalars_device), of which the inverse transform
            (pa_fr_ntt_device) and the transposed product (pa_r1cs_eval_device
            over a pa_r1cs of the transposed matrices) are timed alone and the
            powers and scalar kernels are the rest; the two multiplies; and the
            affine output (normalizations + pack) as the call minus the Fr half
            and the multiplies.

The library is loaded by path (--lib), so the same tool times the parent build.

  python tools/groth16_setup_bench.py --lib <parent build's libpairing_amd.so> --tag parent
  python tools/groth16_setup_bench.py --tag default --against profiles/groth16_setup/parent.json
"""
import argparse
import ctypes
import json
import os
import statistics
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TOP = 0x73eda753299d7d48   # rows with a top limb below r's are below r
FQ_ONE = [0x760900000002fffd, 0xebf4000bc40c0002, 0x5f48985753c758ba,
          0x77ce585370525745, 0x5c071a97a256ec6d, 0x15f65ec3fa80e493]
P, N, U = ctypes.c_void_p, ctypes.c_size_t, ctypes.c_uint


def fr_rows(seed, n):
    g = np.random.default_rng(seed)
    a = g.integers(0, 1 << 63, size=(n, 4), dtype=np.uint64) * np.uint64(2) + g.integers(0, 2, size=(n, 4), dtype=np.uint64)
    a[:, 3] %= np.uint64(TOP)
    return a


class Csr(ctypes.Structure):
    _fields_ = [("row_ptr", P), ("col", P), ("val", P)]


def load(path):
    lib = ctypes.CDLL(path)
    lib.pa_last_error.restype = ctypes.c_char_p
    lib.pa_fr_ntt_domain_create.argtypes = [U, ctypes.POINTER(P)]
    lib.pa_fr_ntt_domain_free.argtypes = [P]
    lib.pa_fr_ntt_domain_free.restype = None
    lib.pa_fr_ntt_workspace_bytes.argtypes = [P, N]
    lib.pa_fr_ntt_workspace_bytes.restype = N
    lib.pa_fr_ntt_device.argtypes = [P, ctypes.c_int, P, P, N, P, N, P]
    lib.pa_r1cs_create.argtypes = [P, P, P, N, N, ctypes.POINTER(P)]
    lib.pa_r1cs_free.argtypes = [P]
    lib.pa_r1cs_free.restype = None
    lib.pa_r1cs_eval_workspace_bytes.argtypes = [P, N]
    lib.pa_r1cs_eval_workspace_bytes.restype = N
    lib.pa_r1cs_eval_device.argtypes = [P, P, N, U, P, P, P, P, N, P]
    for g in (1, 2):
        getattr(lib, "pa_g%d_fixed_base_table_words" % g).restype = N
        getattr(lib, "pa_g%d_fixed_base_workspace_words" % g).restype = N
        getattr(lib, "pa_g%d_wnaf_fixed_base_device" % g).argtypes = [P, P, P, N, P, P, P]
        getattr(lib, "pa_g%d_batch_normalization_device" % g).argtypes = [P, N, P]
    has = hasattr(lib, "pa_groth16_generate_device")
    if has:
        lib.pa_groth16_circuit_create.argtypes = [P, P, P, N, N, N, ctypes.POINTER(P)]
        lib.pa_groth16_circuit_free.argtypes = [P]
        lib.pa_groth16_circuit_free.restype = None
        lib.pa_groth16_circuit_bytes.argtypes = [P]
        lib.pa_groth16_circuit_bytes.restype = N
        lib.pa_groth16_generate_workspace_bytes.argtypes = [P, U]
        lib.pa_groth16_generate_workspace_bytes.restype = N
        lib.pa_groth16_generate_device.argtypes = [P, P, P, P, P, P, P, P, N, P]
        lib.pa_groth16_generate_scalars_device.argtypes = [P, P, P, P, P, N, P]
    return lib, has


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--lib", default=os.path.join(ROOT, "pairing_amd", "lib", "libpairing_amd.so"))
    ap.add_argument("--cases", default="16,20", help="log_n, comma separated")
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--rounds", type=int, default=8)
    ap.add_argument("--calls", type=int, default=1, help="timed calls per round")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "groth16_setup"))
    ap.add_argument("--tag", default="default")
    ap.add_argument("--against", help="the .json of the parent build's run in the same session")
    args = ap.parse_args()

    import torch
    if not torch.cuda.is_available():
        sys.exit("groth16_setup_bench: no HIP device (there is no CPU path to time)")
    lib, has = load(args.lib)
    against = {}
    if args.against:
        with open(args.against) as f:
            against = {c["log_n"]: c["ms"]["baseline"] for c in json.load(f)["cases"]}
    dev = "cuda"
    stream = torch.cuda.current_stream()
    sp = P(stream.cuda_stream)

    def ok(rc, what):
        if rc != 0:
            sys.exit("groth16_setup_bench: %s failed (%d): %s" % (what, rc, lib.pa_last_error().decode()))

    def ptr(t, byte=0):
        return P(t.data_ptr() + byte)

    def up(a):
        return torch.from_numpy(np.ascontiguousarray(a).view(np.int64)).to(dev)

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

    d = np.load(os.path.join(ROOT, "tests", "golden", "bench_points.npz"))

    def system(n, seed):
        """three host CSR matrices of n rows and n columns, three terms per row, and their transposes"""
        g = np.random.default_rng(seed)
        mats, trans = [], []
        for i in range(3):
            row_ptr = np.arange(n + 1, dtype=np.uint64) * np.uint64(3)
            col = g.integers(0, n, size=3 * n, dtype=np.uint32)
            val = fr_rows(seed + 10 + i, 3 * n)
            mats.append((row_ptr, col, val))
            order = np.argsort(col, kind="stable")
            t_ptr = np.zeros(n + 1, np.uint64)
            np.cumsum(np.bincount(col, minlength=n), out=t_ptr[1:])
            trans.append((t_ptr, (order // 3).astype(np.uint32), np.ascontiguousarray(val[order])))
        return mats, trans

    def csrs(mats):
        return [Csr(P(m[0].ctypes.data), P(m[1].ctypes.data), P(m[2].ctypes.data)) for m in mats]

    result = {"tag": args.tag, "device": torch.cuda.get_device_name(0), "lib": os.path.basename(args.lib),
              "has_generate": has, "warmup": args.warmup, "rounds": args.rounds, "calls": args.calls, "cases": []}
    lines = []

    def emit(line):
        lines.append(line)
        print(line, flush=True)

    emit("groth16_setup_bench %s  %s  generate entry: %s" %
         (args.tag, result["device"], "yes" if has else "absent (baseline only)"))
    for case in args.cases.split(","):
        lg = int(case)
        n = nv = 1 << lg
        n1, n2 = 3 * nv + n + 2, nv + 3
        bases = {}
        for group, (jw, fw) in ((1, (18, 6)), (2, (36, 12))):
            b = np.zeros((1, jw), np.uint64)
            b[0, :2 * fw] = d["g%d" % group][0, :2 * fw]
            b[0, 2 * fw:2 * fw + 6] = np.array(FQ_ONE, np.uint64)
            bases[group] = up(b)
        # staged scalars: canonical rows below r, as the call's scalar kernel leaves them
        s1, s2 = up(fr_rows(700 + lg, n1)), up(fr_rows(701 + lg, n2))
        jac1 = torch.empty((n1, 18), dtype=torch.int64, device=dev)
        jac2 = torch.empty((n2, 36), dtype=torch.int64, device=dev)
        tabs = {g: (torch.empty(getattr(lib, "pa_g%d_fixed_base_table_words" % g)(), dtype=torch.int64, device=dev),
                    torch.empty(getattr(lib, "pa_g%d_fixed_base_workspace_words" % g)(), dtype=torch.int64, device=dev))
                for g in (1, 2)}

        def mul1():
            ok(lib.pa_g1_wnaf_fixed_base_device(ptr(bases[1]), ptr(s1), ptr(jac1), n1, ptr(tabs[1][0]), ptr(tabs[1][1]), sp),
               "G1 fixed base")

        def mul2():
            ok(lib.pa_g2_wnaf_fixed_base_device(ptr(bases[2]), ptr(s2), ptr(jac2), n2, ptr(tabs[2][0]), ptr(tabs[2][1]), sp),
               "G2 fixed base")

        def norm():
            ok(lib.pa_g1_batch_normalization_device(ptr(jac1), n1, sp), "G1 batch normalization")
            ok(lib.pa_g2_batch_normalization_device(ptr(jac2), n2, sp), "G2 batch normalization")

        def baseline():
            mul1()
            mul2()
            norm()

        entry = {"log_n": lg, "n_vars": nv, "n_public": 4, "g1_len": n1, "g2_len": n2, "ms": {}}
        entry["ms"]["baseline"] = base = timed(baseline)
        emit("2^%-2d  baseline (two fixed-base multiplies + two normalizations, scalars staged)  %9.3f ms median, "
             "max - min %7.3f" % (lg, base["median"], base["spread"]))
        entry["ms"]["g1_multiply"], entry["ms"]["g2_multiply"] = m1, m2 = timed(mul1), timed(mul2)
        if has:
            mats, trans = system(n, 800 + lg)
            circ, sysm, dom = P(0), P(0), P(0)
            ok(lib.pa_groth16_circuit_create(*(ctypes.byref(c) for c in csrs(mats)), n, nv, 4, ctypes.byref(circ)),
               "pa_groth16_circuit_create")
            ok(lib.pa_r1cs_create(*(ctypes.byref(c) for c in csrs(trans)), nv, n, ctypes.byref(sysm)), "pa_r1cs_create")
            ok(lib.pa_fr_ntt_domain_create(lg, ctypes.byref(dom)), "pa_fr_ntt_domain_create")
            td = fr_rows(900 + lg, 5)
            tp = P(td.ctypes.data)
            aff1 = bases[1].new_zeros((1, 13))
            aff1[0, :12] = bases[1][0, :12]
            aff2 = bases[2].new_zeros((1, 25))
            aff2[0, :24] = bases[2][0, :24]
            wb = lib.pa_groth16_generate_workspace_bytes(circ, lg)
            ws = torch.empty(wb, dtype=torch.uint8, device=dev)
            o1 = torch.empty((n1, 13), dtype=torch.int64, device=dev)
            o2 = torch.empty((n2, 25), dtype=torch.int64, device=dev)
            osc = torch.empty((n1, 4), dtype=torch.int64, device=dev)
            lag, pw = up(fr_rows(901 + lg, n)), up(fr_rows(902 + lg, n))
            uvw = torch.empty((3 * nv, 4), dtype=torch.int64, device=dev)
            nb = lib.pa_fr_ntt_workspace_bytes(dom, 1)
            nws = torch.empty(max(nb, 8), dtype=torch.uint8, device=dev)
            eb = lib.pa_r1cs_eval_workspace_bytes(sysm, 1)
            ews = torch.empty(max(eb, 8), dtype=torch.uint8, device=dev)

            def generate():
                ok(lib.pa_groth16_generate_device(circ, dom, ptr(aff1), ptr(aff2), tp, ptr(o1), ptr(o2), ptr(ws), wb, sp),
                   "pa_groth16_generate_device")

            def scalars():
                ok(lib.pa_groth16_generate_scalars_device(circ, dom, tp, ptr(osc), ptr(ws), wb, sp),
                   "pa_groth16_generate_scalars_device")

            def ntt():
                ok(lib.pa_fr_ntt_device(dom, 1, ptr(pw), ptr(lag), 1, ptr(nws), nb, sp), "pa_fr_ntt_device")

            def product():
                ok(lib.pa_r1cs_eval_device(sysm, ptr(lag), 1, lg, ptr(uvw), ptr(uvw, 32 * nv), ptr(uvw, 64 * nv), ptr(ews),
                                           eb, sp), "pa_r1cs_eval_device")

            entry["ms"]["generate"] = gen = timed(generate)
            entry["ms"]["fr_half"], entry["ms"]["inverse_transform"] = fr, nt = timed(scalars), timed(ntt)
            entry["ms"]["transposed_product"] = pr = timed(product)
            entry["powers_and_scalar_kernels_ms"] = fr["median"] - nt["median"] - pr["median"]
            entry["affine_output_ms"] = gen["median"] - fr["median"] - m1["median"] - m2["median"]
            entry["workspace_bytes"], entry["circuit_bytes"] = wb, lib.pa_groth16_circuit_bytes(circ)
            ref = against.get(lg, base)
            whose = "parent's" if lg in against else "own"
            emit("2^%-2d  generate (trapdoor -> keys, one call)  %9.3f ms median, max - min %7.3f  -> %.3f x the %s "
                 "baseline (+ %.3f ms)" % (lg, gen["median"], gen["spread"], gen["median"] / ref["median"], whose,
                                           gen["median"] - ref["median"]))
            emit("      stages: Fr half %.3f (inverse transform %.3f, transposed product %.3f, powers + scalar kernels "
                 "%.3f)  G1 multiply %.3f  G2 multiply %.3f  affine output (call - rest) %.3f" %
                 (fr["median"], nt["median"], pr["median"], entry["powers_and_scalar_kernels_ms"], m1["median"],
                  m2["median"], entry["affine_output_ms"]))
            over = gen["median"] - ref["median"]
            if over > max(gen["spread"], ref["spread"]):
                parts = {"Fr half": fr["median"], "affine output beyond the baseline's normalizations":
                         entry["affine_output_ms"] - (ref["median"] - m1["median"] - m2["median"])}
                emit("      over the bound by more than the spread; accounted for by: " +
                     ", ".join("%s %.3f ms" % kv for kv in sorted(parts.items(), key=lambda kv: -kv[1])))
            lib.pa_groth16_circuit_free(circ)
            lib.pa_r1cs_free(sysm)
            lib.pa_fr_ntt_domain_free(dom)
            del ws, o1, o2, osc, lag, pw, uvw, nws, ews
        else:
            emit("      G1 multiply %.3f  G2 multiply %.3f" % (m1["median"], m2["median"]))
        result["cases"].append(entry)
        del s1, s2, jac1, jac2, tabs

    os.makedirs(args.out, exist_ok=True)
    with open(os.path.join(args.out, args.tag + ".txt"), "w") as f:
        f.write("\n".join(lines) + "\n")
    with open(os.path.join(args.out, args.tag + ".json"), "w") as f:
        json.dump(result, f, indent=1)


if __name__ == "__main__":
    main()
