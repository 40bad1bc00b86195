#!/usr/bin/env python3
"""Groth16 prover: pa_groth16_prove_device, its steps, and what a build without it can do.

Device-resident, timed with device events on one stream after warm-up: median
and max - min over --rounds rounds of --calls calls, for k proofs over a system
of n = 2^log_n rows and n variables with three terms per row in each matrix
(--cases log_n:k).  The bases are generated on the device with the fixed-base
entries (one G1 set serves the four G1 queries, one G2 set the fifth).

  baseline  entries every build has: pa_fr_ntt_quotient_device on a, b, c staged
            outside the timing, then four G1 and one G2
            pa_g*_multiexp_prepared_batch_device with Montgomery scalars.  No
            evaluation and no assembly: a lower bound on any composition.
  prove     pa_groth16_prove_device, where the library has it, and the same chain
            entry by entry with an event after each step (eval, quotient, the
            five multiexps, and the assembly as the call's time minus the rest).
  eval      pa_r1cs_eval_device alone on the first case's matrices, and on the same
            matrices with one row of 2^16 terms added to A.

The library is loaded by path (--lib), so the same tool times the parent build.

  python tools/groth16_prove_bench.py --lib <parent build's libpairing_amd.so> --tag parent
  python tools/groth16_prove_bench.py --tag default --against profiles/groth16_prove/parent.json
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


class Key(ctypes.Structure):
    _fields_ = [("alpha_g1", ctypes.c_uint64 * 13), ("beta_g1", ctypes.c_uint64 * 13), ("delta_g1", ctypes.c_uint64 * 13),
                ("beta_g2", ctypes.c_uint64 * 25), ("delta_g2", ctypes.c_uint64 * 25), ("n_vars", N), ("n_public", N),
                ("a_query", P), ("b_g1_query", P), ("b_g2_query", P), ("l_query", P), ("h_query", P), ("h_len", N)]


def load(path):
    lib = ctypes.CDLL(path)
    lib.pa_last_error.restype = ctypes.c_char_p
    lib.pa_fr_ntt_domain_create.argtypes = [U, ctypes.POINTER(P)]
    lib.pa_fr_ntt_domain_free.argtypes = [P]
    lib.pa_fr_ntt_domain_free.restype = None
    lib.pa_fr_ntt_quotient_workspace_bytes.argtypes = [P, N]
    lib.pa_fr_ntt_quotient_workspace_bytes.restype = N
    lib.pa_fr_ntt_quotient_device.argtypes = [P, P, P, P, P, N, P, N, P]
    for g in (1, 2):
        getattr(lib, "pa_g%d_fixed_base_table_words" % g).restype = N
        getattr(lib, "pa_g%d_fixed_base_workspace_words" % g).restype = N
        getattr(lib, "pa_g%d_wnaf_fixed_base_device" % g).argtypes = [P, P, P, N, P, P, P]
        getattr(lib, "pa_g%d_batch_normalization_device" % g).argtypes = [P, N, P]
        getattr(lib, "pa_g%d_msm_bases_prepare_device" % g).argtypes = [P, N, P, ctypes.POINTER(P)]
        getattr(lib, "pa_g%d_msm_bases_free" % g).argtypes = [P]
        f = getattr(lib, "pa_g%d_multiexp_prepared_batch_workspace_bytes" % g)
        f.argtypes, f.restype = [P, N, N], N
        getattr(lib, "pa_g%d_multiexp_prepared_batch_device" % g).argtypes = [P, P, N, N, U, P, P, N, P]
    has_prove = hasattr(lib, "pa_groth16_prove_device")
    if has_prove:
        lib.pa_r1cs_create.argtypes = [P, P, P, N, N, ctypes.POINTER(P)]
        lib.pa_r1cs_free.argtypes = [P]
        lib.pa_r1cs_free.restype = None
        lib.pa_r1cs_bytes.argtypes = [P]
        lib.pa_r1cs_bytes.restype = N
        lib.pa_r1cs_chunk_len.restype = N
        lib.pa_r1cs_eval_workspace_bytes.argtypes = [P, N]
        lib.pa_r1cs_eval_workspace_bytes.restype = N
        lib.pa_r1cs_eval_device.argtypes = [P, P, N, U, P, P, P, P, N, P]
        lib.pa_groth16_pk_create.argtypes = [P, U, ctypes.POINTER(P)]
        lib.pa_groth16_pk_free.argtypes = [P]
        lib.pa_groth16_pk_free.restype = None
        lib.pa_groth16_prove_workspace_bytes.argtypes = [P, P, N]
        lib.pa_groth16_prove_workspace_bytes.restype = N
        lib.pa_groth16_prove_device.argtypes = [P, P, P, P, P, P, N, P, P, N, P]
    return lib, has_prove


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--lib", default=os.path.join(ROOT, "pairing_amd", "lib", "libpairing_amd.so"))
    ap.add_argument("--cases", default="20:1,16:16,12:256", help="log_n:k, comma separated")
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--rounds", type=int, default=8)
    ap.add_argument("--calls", type=int, default=2, help="timed calls per round")
    ap.add_argument("--long-row", type=int, default=1 << 16, help="terms of the row added for the eval comparison")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "groth16_prove"))
    ap.add_argument("--tag", default="default")
    ap.add_argument("--against", help="the .json of the parent build's run in the same session")
    args = ap.parse_args()

    import torch
    if not torch.cuda.is_available():
        sys.exit("groth16_prove_bench: no HIP device (there is no CPU path to time)")
    lib, has_prove = load(args.lib)
    against = {}
    if args.against:
        with open(args.against) as f:
            against = {(c["log_n"], c["k"]): c["ms"]["baseline"] for c in json.load(f)["cases"]}
    dev = "cuda"
    stream = torch.cuda.current_stream()
    sp = P(stream.cuda_stream)

    def ok(rc, what):
        if rc != 0:
            sys.exit("groth16_prove_bench: %s failed (%d): %s" % (what, rc, lib.pa_last_error().decode()))

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

    def split(steps):
        """median ms of each step of a chain, from an event after each, over the rounds"""
        for _ in range(args.warmup):
            for _, fn in steps:
                fn()
        torch.cuda.synchronize()
        acc = {name: [] for name, _ in steps}
        for _ in range(args.rounds):
            evs = [torch.cuda.Event(enable_timing=True) for _ in range(len(steps) + 1)]
            evs[0].record(stream)
            for i, (_, fn) in enumerate(steps):
                fn()
                evs[i + 1].record(stream)
            evs[-1].synchronize()
            for i, (name, _) in enumerate(steps):
                acc[name].append(evs[i].elapsed_time(evs[i + 1]))
        return {name: {"median": statistics.median(v), "spread": max(v) - min(v)} for name, v in acc.items()}

    d = np.load(os.path.join(ROOT, "tests", "golden", "bench_points.npz"))

    def gen_bases(group, n):
        """n affine records k_i * base on the device, through the fixed-base entries"""
        jw, aw, fw = (18, 13, 6) if group == 1 else (36, 25, 12)
        base_np = np.zeros((1, jw), np.uint64)
        base_np[0, :2 * fw] = d["g%d" % group][0, :2 * fw]
        base_np[0, 2 * fw:2 * fw + 6] = np.array(FQ_ONE, np.uint64)
        g = np.random.default_rng(1234 + group)
        k_np = g.integers(0, 1 << 63, size=(n, 4), dtype=np.uint64)
        k_np[:, 0] ^= np.arange(n, dtype=np.uint64)
        k_np[:, 3] &= np.uint64(0x0fffffffffffffff)
        base, ks = up(base_np), up(k_np)
        jac = torch.empty((n, jw), dtype=torch.int64, device=dev)
        table = torch.empty(getattr(lib, "pa_g%d_fixed_base_table_words" % group)(), dtype=torch.int64, device=dev)
        tws = torch.empty(getattr(lib, "pa_g%d_fixed_base_workspace_words" % group)(), dtype=torch.int64, device=dev)
        ok(getattr(lib, "pa_g%d_wnaf_fixed_base_device" % group)(ptr(base), ptr(ks), ptr(jac), n, ptr(table), ptr(tws),
                                                                  sp), "fixed base")
        ok(getattr(lib, "pa_g%d_batch_normalization_device" % group)(ptr(jac), n, sp), "batch normalization")
        aff = torch.zeros((n, aw), dtype=torch.int64, device=dev)
        aff[:, :2 * fw] = jac[:, :2 * fw]
        torch.cuda.synchronize()
        return aff

    def system(n, seed, long_row=0):
        """three host CSR matrices of n rows and n columns, three terms per row; A's last row gets `long_row` terms"""
        g = np.random.default_rng(seed)
        mats = []
        for i in range(3):
            lens = np.full(n, 3, np.uint64)
            if i == 0 and long_row:
                lens[n - 1] = long_row
            row_ptr = np.zeros(n + 1, np.uint64)
            np.cumsum(lens, out=row_ptr[1:])
            nnz = int(row_ptr[-1])
            mats.append((row_ptr, g.integers(0, n, size=nnz, dtype=np.uint32), fr_rows(seed + 10 + i, nnz)))
        return mats

    def r1cs_create(mats, n):
        cs = [Csr(P(m[0].ctypes.data), P(m[1].ctypes.data), P(m[2].ctypes.data)) for m in mats]
        h = P(0)
        ok(lib.pa_r1cs_create(*(ctypes.byref(c) for c in cs), n, n, ctypes.byref(h)), "pa_r1cs_create")
        return h

    result = {"tag": args.tag, "device": torch.cuda.get_device_name(0), "lib": os.path.basename(args.lib),
              "has_prove": has_prove, "warmup": args.warmup, "rounds": args.rounds, "calls": args.calls, "cases": []}
    lines = []

    def emit(line):
        lines.append(line)
        print(line, flush=True)

    emit("groth16_prove_bench %s  %s  prove entry: %s" %
         (args.tag, result["device"], "yes" if has_prove else "absent (baseline only)"))
    first = True
    for case in args.cases.split(","):
        lg, k = (int(x) for x in case.split(":"))
        n = 1 << lg
        g1, g2 = gen_bases(1, n), gen_bases(2, n)
        dom = P(0)
        ok(lib.pa_fr_ntt_domain_create(lg, ctypes.byref(dom)), "pa_fr_ntt_domain_create")
        b1, b2 = P(0), P(0)
        ok(lib.pa_g1_msm_bases_prepare_device(ptr(g1), n, sp, ctypes.byref(b1)), "prepare G1")
        ok(lib.pa_g2_msm_bases_prepare_device(ptr(g2), n, sp, ctypes.byref(b2)), "prepare G2")
        w_np, r_np, s_np = fr_rows(500 + lg, k * n), fr_rows(501 + lg, k), fr_rows(502 + lg, k)
        w_np.reshape(k, n, 4)[:, 0] = np.array([0x00000001fffffffe, 0x5884b7fa00034802, 0x998c4fefecbc4ff5,
                                                0x1824b159acc5056f], np.uint64)   # w_0 = 1
        W, R, S = up(w_np), up(r_np), up(s_np)
        abc = up(fr_rows(503 + lg, 3 * k * n))
        h_out = torch.empty((k * n, 4), dtype=torch.int64, device=dev)
        qb = lib.pa_fr_ntt_quotient_workspace_bytes(dom, k)
        m1 = lib.pa_g1_multiexp_prepared_batch_workspace_bytes(b1, n, k)
        m2 = lib.pa_g2_multiexp_prepared_batch_workspace_bytes(b2, n, k)
        ws = torch.empty(max(qb, m1, m2, 8), dtype=torch.uint8, device=dev)
        sums = torch.empty((4 * k, 18), dtype=torch.int64, device=dev)
        sum2 = torch.empty((k, 36), dtype=torch.int64, device=dev)
        rows = 32 * k * n

        def quotient(a=abc, out=h_out):
            ok(lib.pa_fr_ntt_quotient_device(dom, ptr(a), ptr(a, rows), ptr(a, 2 * rows), ptr(out), k, ptr(ws), qb, sp),
               "quotient")

        def msm1(i, scalars):
            ok(lib.pa_g1_multiexp_prepared_batch_device(b1, ptr(scalars), n, k, 1, ptr(sums, 144 * k * i), ptr(ws), m1,
                                                        sp), "G1 multiexp")

        def msm2():
            ok(lib.pa_g2_multiexp_prepared_batch_device(b2, ptr(W), n, k, 1, ptr(sum2), ptr(ws), m2, sp), "G2 multiexp")

        def baseline():
            quotient()
            msm1(0, W)
            msm1(1, W)
            msm1(2, W)
            msm1(3, h_out)
            msm2()

        entry = {"log_n": lg, "k": k, "ms": {}}
        entry["ms"]["baseline"] = base = timed(baseline)
        emit("%4d x 2^%-2d  baseline (quotient + 5 multiexps, a b c staged)  %9.3f ms median, max - min %7.3f" %
             (k, lg, base["median"], base["spread"]))
        if has_prove:
            mats = system(n, 600 + lg)
            sysm = r1cs_create(mats, n)
            g1h, g2h = g1.cpu().numpy(), g2.cpu().numpy()
            key = Key()
            for i, f in enumerate(("alpha_g1", "beta_g1", "delta_g1")):
                ctypes.memmove(getattr(key, f), g1h[i + 1].ctypes.data, 104)
            for i, f in enumerate(("beta_g2", "delta_g2")):
                ctypes.memmove(getattr(key, f), g2h[i + 1].ctypes.data, 200)
            key.n_vars, key.n_public, key.h_len = n, 1, n - 1
            key.a_query = key.b_g1_query = key.h_query = g1h.ctypes.data
            key.l_query = g1h.ctypes.data + 104
            key.b_g2_query = g2h.ctypes.data
            pk = P(0)
            ok(lib.pa_groth16_pk_create(ctypes.byref(key), lg, ctypes.byref(pk)), "pa_groth16_pk_create")
            pb = lib.pa_groth16_prove_workspace_bytes(pk, sysm, k)
            pws = torch.empty(pb, dtype=torch.uint8, device=dev)
            proofs = torch.empty((k, 51), dtype=torch.int64, device=dev)
            eb = lib.pa_r1cs_eval_workspace_bytes(sysm, k)
            ews = torch.empty(max(eb, 8), dtype=torch.uint8, device=dev)
            ev = torch.empty((3 * k * n, 4), dtype=torch.int64, device=dev)

            def prove():
                ok(lib.pa_groth16_prove_device(pk, sysm, dom, ptr(W), ptr(R), ptr(S), k, ptr(proofs), ptr(pws), pb, sp),
                   "pa_groth16_prove_device")

            def evaluate(h=sysm, w=ews, b=eb):
                ok(lib.pa_r1cs_eval_device(h, ptr(W), k, lg, ptr(ev), ptr(ev, rows), ptr(ev, 2 * rows), ptr(w), b, sp),
                   "pa_r1cs_eval_device")

            entry["ms"]["prove"] = pr = timed(prove)
            steps = [("eval", evaluate), ("quotient", lambda: quotient(ev, h_out)), ("msm_a", lambda: msm1(0, W)),
                     ("msm_b_g1", lambda: msm1(1, W)), ("msm_l", lambda: msm1(2, W)), ("msm_h", lambda: msm1(3, h_out)),
                     ("msm_b_g2", msm2)]
            entry["split_ms"] = sp_ms = split(steps)
            rest = sum(v["median"] for v in sp_ms.values())
            entry["assembly_ms"] = pr["median"] - rest
            entry["workspace_bytes"], entry["r1cs_bytes"] = pb, lib.pa_r1cs_bytes(sysm)
            ref = against.get((lg, k), base)
            emit("%4d x 2^%-2d  prove (witness -> proof, one call)               %9.3f ms median, max - min %7.3f"
                 "  -> %.3f x the %s baseline (+ %.3f ms)" %
                 (k, lg, pr["median"], pr["spread"], pr["median"] / ref["median"],
                  "parent's" if (lg, k) in against else "own", pr["median"] - ref["median"]))
            emit("               split: " + "  ".join("%s %.3f" % (name, v["median"]) for name, v in sp_ms.items()) +
                 "  assembly (call - steps) %.3f" % entry["assembly_ms"])
            if first:
                ev_plain = timed(evaluate)
                skew = r1cs_create(system(n, 600 + lg, args.long_row), n)
                sb = lib.pa_r1cs_eval_workspace_bytes(skew, k)
                sws = torch.empty(max(sb, 8), dtype=torch.uint8, device=dev)
                ev_skew = timed(lambda: evaluate(skew, sws, sb))
                entry["eval_ms"] = {"plain": ev_plain, "with_long_row": ev_skew, "long_row_terms": args.long_row,
                                    "chunk_len": lib.pa_r1cs_chunk_len()}
                emit("               eval alone %9.4f ms (max - min %.4f); with one row of %d terms %9.4f ms (max - min "
                     "%.4f); chunk length %d" % (ev_plain["median"], ev_plain["spread"], args.long_row,
                                                 ev_skew["median"], ev_skew["spread"], lib.pa_r1cs_chunk_len()))
                lib.pa_r1cs_free(skew)
                del sws
            lib.pa_groth16_pk_free(pk)
            lib.pa_r1cs_free(sysm)
            del pws, proofs, ews, ev
        first = False
        result["cases"].append(entry)
        lib.pa_g1_msm_bases_free(b1)
        lib.pa_g2_msm_bases_free(b2)
        lib.pa_fr_ntt_domain_free(dom)
        del g1, g2, W, R, S, abc, h_out, ws, sums, sum2

    os.makedirs(args.out, exist_ok=True)
    with open(os.path.join(args.out, args.tag + ".txt"), "w") as f:
        f.write("\n".join(lines) + "\n")
    with open(os.path.join(args.out, args.tag + ".json"), "w") as f:
        json.dump(result, f, indent=1)


if __name__ == "__main__":
    main()
