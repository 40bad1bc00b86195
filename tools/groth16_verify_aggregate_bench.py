#!/usr/bin/env python3
"""Groth16 aggregate check: pa_groth16_verify_aggregate_device against the per-proof verifier.

Device-resident, timed with device events on one stream after warm-up: median
and max - min over --rounds rounds of --calls calls, for k proofs over a key of
l public inputs (--cases k:l).  Points come from tests/golden/bench_points.npz
(the proofs do not verify: no stage's time depends on the verdict), inputs are
random Montgomery rows, weights random 128-bit rows.

  verify      pa_groth16_verify_device (gt = NULL): the per-proof entry.  Run with
              --lib on the parent build's library this is the baseline.
  aggregate   pa_groth16_verify_aggregate_device (gt = NULL)
  points      pa_groth16_verify_aggregate_points_device: weight sums, z A, comb sums,
              short MSM, into_affine -- the G1 side alone
  msm_u128    pa_g1_multiexp_u128_device over the k C points (the short MSM alone)
  miller      pa_pairing_miller_loop_batch_device over k + 3 pairs
  final_exp   pa_final_exponentiation_batch_device over one value
  encoded     pa_groth16_verify_aggregate_encoded_device over the same proofs compressed
  (--msm n,..) pa_g1_multiexp_u128_device against pa_g1_multiexp_device over the
              zero-extended scalars at n terms

The kernels that have no entry of their own (weight sums, scaling, comb sum,
product) are read from a kernel trace of this tool at one shape, e.g.
  rocprofv3 --kernel-trace --stats -d <dir> -- python tools/groth16_verify_aggregate_bench.py --cases 16384:4 \\
      --encoded "" --msm "" --rounds 2 --tag trace

  python tools/groth16_verify_aggregate_bench.py --lib <parent build's libpairing_amd.so> --tag parent
  python tools/groth16_verify_aggregate_bench.py --tag default --against profiles/groth16_verify_aggregate/parent.json
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
P, N, U = ctypes.c_void_p, ctypes.c_size_t, ctypes.c_uint
G1A, G2A, F12 = 104, 200, 576   # bytes of pa_g1_affine, pa_g2_affine, pa_fq12


def fr_rows(seed, n):
    g = np.random.default_rng(seed)
    a = g.integers(0, 1 << 63, size=(n, 4), dtype=np.uint64) * np.uint64(2) + g.integers(0, 2, size=(n, 4), dtype=np.uint64)
    a[:, 3] %= np.uint64(TOP)
    return a


def u128_rows(seed, n):
    g = np.random.default_rng(seed)
    return g.integers(0, 1 << 63, size=(n, 2), dtype=np.uint64) * np.uint64(2) + g.integers(0, 2, size=(n, 2), dtype=np.uint64)


class VKey(ctypes.Structure):
    _fields_ = [("alpha_g1", ctypes.c_uint64 * 13), ("beta_g2", ctypes.c_uint64 * 25), ("gamma_g2", ctypes.c_uint64 * 25),
                ("delta_g2", ctypes.c_uint64 * 25), ("ic", P), ("n_public", N)]


def load(path):
    lib = ctypes.CDLL(path)
    lib.pa_last_error.restype = ctypes.c_char_p
    lib.pa_pairing_miller_loop_batch_device.argtypes = [P, P, P, N, P]
    lib.pa_final_exponentiation_batch_device.argtypes = [P, P, P, N, P]
    lib.pa_g1_encode_batch.argtypes = [P, N, ctypes.c_int, P]
    lib.pa_g2_encode_batch.argtypes = [P, N, ctypes.c_int, P]
    lib.pa_groth16_vk_create.argtypes = [P, ctypes.POINTER(P)]
    lib.pa_groth16_vk_free.argtypes = [P]
    lib.pa_groth16_vk_free.restype = None
    lib.pa_groth16_vk_bytes.argtypes, lib.pa_groth16_vk_bytes.restype = [P], N
    lib.pa_groth16_verify_workspace_bytes.argtypes, lib.pa_groth16_verify_workspace_bytes.restype = [P, N], N
    lib.pa_groth16_verify_device.argtypes = [P, P, P, N, U, N, P, P, P, N, P]
    lib.pa_multiexp_workspace_bytes.argtypes, lib.pa_multiexp_workspace_bytes.restype = [ctypes.c_int, N], N
    lib.pa_g1_multiexp_device.argtypes = [P, P, N, P, P, N, P]
    has = hasattr(lib, "pa_groth16_verify_aggregate_device")
    if has:
        f = lib.pa_groth16_verify_aggregate_workspace_bytes
        f.argtypes, f.restype = [P, N], N
        f = lib.pa_g1_multiexp_u128_workspace_bytes
        f.argtypes, f.restype = [N], N
        lib.pa_g1_multiexp_u128_device.argtypes = [P, P, N, P, P, N, P]
        lib.pa_groth16_verify_aggregate_device.argtypes = [P, P, P, N, U, P, N, P, P, P, N, P]
        lib.pa_groth16_verify_aggregate_encoded_device.argtypes = [P, P, P, N, U, P, N, P, P, P, P, N, P]
        lib.pa_groth16_verify_aggregate_points_device.argtypes = [P, P, P, N, U, P, N, P, P, N, P]
    return lib, has


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--lib", default=os.path.join(ROOT, "pairing_amd", "lib", "libpairing_amd.so"))
    ap.add_argument("--cases", default="1:4,64:4,1024:4,16384:4,16384:32,65536:4", help="k:l, comma separated")
    ap.add_argument("--encoded", default="16384:4", help="k:l cases that also time the encoded entry")
    ap.add_argument("--msm", default="16384,65536,262144", help="term counts of the short MSM against the plain one")
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--rounds", type=int, default=8)
    ap.add_argument("--calls", type=int, default=2, help="timed calls per round")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "groth16_verify_aggregate"))
    ap.add_argument("--tag", default="default")
    ap.add_argument("--against", help="the .json of the parent build's run in the same session")
    args = ap.parse_args()

    import torch
    if not torch.cuda.is_available():
        sys.exit("groth16_verify_aggregate_bench: no HIP device (there is no CPU path to time)")
    lib, has = load(args.lib)
    against = {}
    if args.against:
        with open(args.against) as f:
            against = {(c["k"], c["l"]): c["ms"]["verify"] for c in json.load(f)["cases"]}
    dev = "cuda"
    stream = torch.cuda.current_stream()
    sp = P(stream.cuda_stream)

    def ck(rc, what):
        if rc:
            sys.exit("%s failed (%d): %s" % (what, rc, lib.pa_last_error().decode()))

    def to_dev(a):
        return torch.from_numpy(np.ascontiguousarray(a).view(np.int64)).to(dev)

    def dp(t):
        return P(t.data_ptr())

    def timed(fn):
        """[median, max - min] in ms of one call, over rounds of `calls` calls"""
        for _ in range(args.warmup):
            fn()
        torch.cuda.synchronize()
        per = []
        for _ in range(args.rounds):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(stream)
            for _ in range(args.calls):
                fn()
            e1.record(stream)
            e1.synchronize()
            per.append(e0.elapsed_time(e1) / args.calls)
        return [statistics.median(per), max(per) - min(per)]

    def show(ms):
        for name, v in ms.items():
            print("    %-16s %9.3f (%.3f) ms" % (name, v[0], v[1]))
        sys.stdout.flush()

    pts = np.load(os.path.join(ROOT, "tests", "golden", "bench_points.npz"))
    g1, g2 = pts["g1"], pts["g2"]
    encoded_cases = {tuple(int(x) for x in c.split(":")) for c in args.encoded.split(",") if c}
    results = []
    for case in (c for c in args.cases.split(",") if c):
        k, l = (int(x) for x in case.split(":"))
        idx = np.arange(k, dtype=np.int64)
        a, b, c = g1[(idx * 3 + 40) % 256], g2[(idx * 5 + 3) % 256], g1[(idx * 7 + 90) % 256]
        ms = {}
        key = VKey()
        ic = np.ascontiguousarray(g1[(np.arange(l + 1) * 13 + 7) % 256])
        ctypes.memmove(key.alpha_g1, g1[0].ctypes.data, G1A)
        for field, rec in (("beta_g2", g2[0]), ("gamma_g2", g2[1]), ("delta_g2", g2[2])):
            ctypes.memmove(getattr(key, field), np.ascontiguousarray(rec).ctypes.data, G2A)
        key.ic, key.n_public = ic.ctypes.data, l + 1
        h = P(0)
        ck(lib.pa_groth16_vk_create(ctypes.byref(key), ctypes.byref(h)), "vk_create")
        row = {"k": k, "l": l, "ms": ms, "vk_bytes": int(lib.pa_groth16_vk_bytes(h))}
        proofs = np.ascontiguousarray(np.concatenate([a, b, c], axis=1))
        PR, X, Z = to_dev(proofs), to_dev(fr_rows(k + l, max(k * l, 1))), to_dev(u128_rows(k + 7 * l, k))
        valid = torch.empty(k, dtype=torch.uint8, device=dev)
        ws = torch.empty(lib.pa_groth16_verify_workspace_bytes(h, k), dtype=torch.uint8, device=dev)
        ms["verify"] = timed(lambda: ck(lib.pa_groth16_verify_device(
            h, dp(PR), dp(X), l, 1, k, dp(valid), None, dp(ws), ws.numel(), sp), "verify"))
        del ws
        if has:
            aws = torch.empty(lib.pa_groth16_verify_aggregate_workspace_bytes(h, k), dtype=torch.uint8, device=dev)
            row["workspace_bytes"] = aws.numel()
            ms["aggregate"] = timed(lambda: ck(lib.pa_groth16_verify_aggregate_device(
                h, dp(PR), dp(X), l, 1, dp(Z), k, dp(valid), None, dp(aws), aws.numel(), sp), "aggregate"))
            out_pts = torch.empty((k + 3, 13), dtype=torch.int64, device=dev)
            ms["points"] = timed(lambda: ck(lib.pa_groth16_verify_aggregate_points_device(
                h, dp(PR), dp(X), l, 1, dp(Z), k, dp(out_pts), dp(aws), aws.numel(), sp), "points"))
            C = to_dev(c)
            mws = torch.empty(max(lib.pa_g1_multiexp_u128_workspace_bytes(k), 8), dtype=torch.uint8, device=dev)
            jac = torch.empty((1, 18), dtype=torch.int64, device=dev)
            ms["msm_u128"] = timed(lambda: ck(lib.pa_g1_multiexp_u128_device(
                dp(C), dp(Z), k, dp(jac), dp(mws), mws.numel(), sp), "msm_u128"))
            SP = to_dev(np.concatenate([a, g1[:3]]))
            SQ = to_dev(np.concatenate([b, g2[:3]]))
            ml = torch.empty((k + 3, 72), dtype=torch.int64, device=dev)
            ms["miller"] = timed(lambda: ck(lib.pa_pairing_miller_loop_batch_device(dp(SP), dp(SQ), dp(ml), k + 3, sp),
                                            "miller loops"))
            fe_out = torch.empty((1, 72), dtype=torch.int64, device=dev)
            fe_ok = torch.empty(1, dtype=torch.uint8, device=dev)
            ms["final_exp"] = timed(lambda: ck(lib.pa_final_exponentiation_batch_device(
                dp(ml), dp(fe_out), dp(fe_ok), 1, sp), "final exponentiation"))
            if (k, l) in encoded_cases:
                enc = np.empty((k, 192), np.uint8)
                for lo, hi, fn, recs in ((0, 48, lib.pa_g1_encode_batch, a), (48, 144, lib.pa_g2_encode_batch, b),
                                         (144, 192, lib.pa_g1_encode_batch, c)):
                    part = np.empty((k, hi - lo), np.uint8)
                    recs = np.ascontiguousarray(recs)
                    ck(fn(recs.ctypes.data_as(P), k, 1, part.ctypes.data_as(P)), "encode")
                    enc[:, lo:hi] = part
                E = torch.from_numpy(enc).to(dev)
                status = torch.empty(3 * k, dtype=torch.uint8, device=dev)
                ms["encoded"] = timed(lambda: ck(lib.pa_groth16_verify_aggregate_encoded_device(
                    h, dp(E), dp(X), l, 1, dp(Z), k, dp(valid), dp(status), None, dp(aws), aws.numel(), sp), "encoded"))
                torch.cuda.synchronize()
                row["encoded_status_nonzero"] = int((status != 0).sum())
        torch.cuda.synchronize()
        lib.pa_groth16_vk_free(h)
        if (k, l) in against:
            ms["parent_verify"] = against[(k, l)]
        results.append(row)
        print("k = %6d  l = %3d" % (k, l))
        show(ms)
    msm = []
    for n in (int(x) for x in args.msm.split(",") if x):
        if not has:
            break
        idx = np.arange(n, dtype=np.int64)
        B = to_dev(g1[(idx * 7 + 90) % 256])
        z = u128_rows(n, n)
        Z, ZX = to_dev(z), to_dev(np.concatenate([z, np.zeros((n, 2), np.uint64)], axis=1))
        jac = torch.empty((1, 18), dtype=torch.int64, device=dev)
        w0 = torch.empty(lib.pa_g1_multiexp_u128_workspace_bytes(n), dtype=torch.uint8, device=dev)
        w1 = torch.empty(lib.pa_multiexp_workspace_bytes(1, n), dtype=torch.uint8, device=dev)
        ms = {"msm_u128": timed(lambda: ck(lib.pa_g1_multiexp_u128_device(dp(B), dp(Z), n, dp(jac), dp(w0), w0.numel(), sp),
                                           "msm_u128")),
              "msm_zero_extended": timed(lambda: ck(lib.pa_g1_multiexp_device(dp(B), dp(ZX), n, dp(jac), dp(w1), w1.numel(),
                                                                              sp), "msm"))}
        msm.append({"n": n, "ms": ms})
        print("msm n = %d" % n)
        show(ms)
    os.makedirs(args.out, exist_ok=True)
    path = os.path.join(args.out, args.tag + ".json")
    with open(path, "w") as f:
        json.dump({"lib": os.path.relpath(args.lib, ROOT), "device": torch.cuda.get_device_name(0), "rounds": args.rounds,
                   "calls": args.calls, "warmup": args.warmup, "unit": "ms: [median, max - min]", "cases": results,
                   "msm": msm}, f, indent=1)
    print("wrote", os.path.relpath(path, ROOT))


if __name__ == "__main__":
    main()
