#!/usr/bin/env python3
"""Groth16 verifier: pa_groth16_verify_device, its stages, and what a build without it can do.

Device-resident, timed with device events on one stream after warm-up: median
and max - min over --rounds rounds of --calls calls, for k proofs over a key of
l public inputs (--cases k:l).  Points come from tests/golden/bench_points.npz
(the proofs do not verify: no stage's time depends on the verdict), inputs are
random Montgomery rows.

  baseline  what every build has: pa_multi_pairing_batch_device over three pairs
            per proof, (A, B), (acc, -gamma), (C, -delta), with the acc points
            staged outside the timing -- no input sum, which flatters it.
  verify    pa_groth16_verify_device (gt = NULL) as the library dispatches it, and
            with PA_G16V_SHARED_MIN forcing each of its two Miller-loop
            compositions: `pairs3k` (all 3 k pairs through the e(P, Q) loops) and
            `shared` ((acc, -gamma), (C, -delta) on the shared-prepared loop).
  stages    entry by entry: the input sum (pa_groth16_vk_input_sum_device), the
            Miller loops of either composition from the public entries, the final
            exponentiation over k values.  `rest_*` is derived, not timed: the
            median of the forced call minus the medians of those separately timed
            entries (what is left for split, product of three and compare, and
            any gap between launches), so it carries their spreads.
  encoded   pa_groth16_verify_encoded_device over the same proofs compressed.

The library is loaded by path (--lib), so the same tool times the parent build
(baseline only there).

  python tools/groth16_verify_bench.py --lib <parent build's libpairing_amd.so> --tag parent
  python tools/groth16_verify_bench.py --tag default --against profiles/groth16_verify/parent.json
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
Q_LIMBS = [0xb9feffffffffaaab, 0x1eabfffeb153ffff, 0x6730d2a0f6b0f624, 0x64774b84f38512bf, 0x4b1ba7b6434bacd7,
           0x1a0111ea397fe69a]
P, N, U = ctypes.c_void_p, ctypes.c_size_t, ctypes.c_uint
KNOB = "PA_G16V_SHARED_MIN"
G1A, G2A, F12, G2P = 104, 200, 576, 19592   # bytes of pa_g1_affine, pa_g2_affine, pa_fq12, pa_g2_prepared


def fr_rows(seed, n):
    g = np.random.default_rng(seed)
    a = g.integers(0, 1 << 63, size=(n, 4), dtype=np.uint64) * np.uint64(2) + g.integers(0, 2, size=(n, 4), dtype=np.uint64)
    a[:, 3] %= np.uint64(TOP)
    return a


def negate_g2(rec):
    """-Q of one (25,) affine record that is not the point at infinity"""
    q = sum(w << (64 * i) for i, w in enumerate(Q_LIMBS))
    out = rec.copy()
    for lo in (12, 18):
        y = sum(int(w) << (64 * i) for i, w in enumerate(rec[lo:lo + 6]))
        out[lo:lo + 6] = [((q - y) % q >> (64 * i)) & (2**64 - 1) for i in range(6)]
    return out


class VKey(ctypes.Structure):
    _fields_ = [("alpha_g1", ctypes.c_uint64 * 13), ("beta_g2", ctypes.c_uint64 * 25), ("gamma_g2", ctypes.c_uint64 * 25),
                ("delta_g2", ctypes.c_uint64 * 25), ("ic", P), ("n_public", N)]


def load(path):
    lib = ctypes.CDLL(path)
    lib.pa_last_error.restype = ctypes.c_char_p
    lib.pa_multi_pairing_batch_workspace_bytes.argtypes = [N, N]
    lib.pa_multi_pairing_batch_workspace_bytes.restype = N
    lib.pa_multi_pairing_batch_device.argtypes = [P, P, P, N, P, P, P, P, P]
    lib.pa_pairing_miller_loop_batch_device.argtypes = [P, P, P, N, P]
    lib.pa_miller_loop_shared_prepared_device.argtypes = [P, N, P, P, P]
    lib.pa_g2_prepare_batch_device.argtypes = [P, P, N, P]
    lib.pa_final_exponentiation_batch_device.argtypes = [P, P, P, N, P]
    lib.pa_g1_encode_batch.argtypes = [P, N, ctypes.c_int, P]
    lib.pa_g2_encode_batch.argtypes = [P, N, ctypes.c_int, P]
    has_verify = hasattr(lib, "pa_groth16_verify_device")
    if has_verify:
        lib.pa_groth16_vk_create.argtypes = [P, ctypes.POINTER(P)]
        lib.pa_groth16_vk_free.argtypes = [P]
        lib.pa_groth16_vk_free.restype = None
        for name in ("pa_groth16_vk_bytes",):
            getattr(lib, name).argtypes, getattr(lib, name).restype = [P], N
        for name in ("pa_groth16_verify_workspace_bytes", "pa_groth16_vk_input_sum_workspace_bytes"):
            getattr(lib, name).argtypes, getattr(lib, name).restype = [P, N], N
        lib.pa_groth16_vk_input_sum_device.argtypes = [P, P, N, U, N, P, P, N, P]
        lib.pa_groth16_verify_device.argtypes = [P, P, P, N, U, N, P, P, P, N, P]
        lib.pa_groth16_verify_encoded_device.argtypes = [P, P, P, N, U, N, P, P, P, P, N, P]
    return lib, has_verify


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--lib", default=os.path.join(ROOT, "pairing_amd", "lib", "libpairing_amd.so"))
    ap.add_argument("--cases", default="1:4,64:4,1024:4,16384:4,16384:32", help="k:l, comma separated")
    ap.add_argument("--encoded", default="16384:4", help="k:l cases that also time the encoded entry")
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--rounds", type=int, default=8)
    ap.add_argument("--calls", type=int, default=2, help="timed calls per round")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "groth16_verify"))
    ap.add_argument("--tag", default="default")
    ap.add_argument("--against", help="the .json of the parent build's run in the same session")
    args = ap.parse_args()

    import torch
    if not torch.cuda.is_available():
        sys.exit("groth16_verify_bench: no HIP device (there is no CPU path to time)")
    lib, has_verify = load(args.lib)
    against = {}
    if args.against:
        with open(args.against) as f:
            against = {(c["k"], c["l"]): c["ms"]["baseline"] for c in json.load(f)["cases"]}
    dev = "cuda"
    stream = torch.cuda.current_stream()
    sp = P(stream.cuda_stream)
    os.environ.pop(KNOB, None)

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

    pts = np.load(os.path.join(ROOT, "tests", "golden", "bench_points.npz"))
    g1, g2 = pts["g1"], pts["g2"]
    encoded_cases = {tuple(int(x) for x in c.split(":")) for c in args.encoded.split(",") if c}
    results = []
    for case in args.cases.split(","):
        k, l = (int(x) for x in case.split(":"))
        idx = np.arange(k, dtype=np.int64)
        a, b, c = g1[(idx * 3 + 40) % 256], g2[(idx * 5 + 3) % 256], g1[(idx * 7 + 90) % 256]
        acc = g1[(idx * 11 + 150) % 256]
        neg_gamma, neg_delta = negate_g2(g2[1]), negate_g2(g2[2])
        ms = {}
        # ---- baseline: three pairs per proof through the batched multi-pairing ----
        bp = np.empty((3 * k, 13), np.uint64)
        bq = np.empty((3 * k, 25), np.uint64)
        bp[0::3], bp[1::3], bp[2::3] = a, acc, c
        bq[0::3], bq[1::3], bq[2::3] = b, neg_gamma, neg_delta
        BP, BQ = to_dev(bp), to_dev(bq)
        offsets = np.arange(k + 1, dtype=np.uint64) * np.uint64(3)
        b_out = torch.empty((k, 72), dtype=torch.int64, device=dev)
        b_flags = torch.empty(2 * k, dtype=torch.uint8, device=dev)
        b_ws = torch.empty(lib.pa_multi_pairing_batch_workspace_bytes(3 * k, k), dtype=torch.uint8, device=dev)

        def baseline():
            ck(lib.pa_multi_pairing_batch_device(dp(BP), dp(BQ), offsets.ctypes.data_as(P), k, dp(b_out), dp(b_flags),
                                                 P(b_flags.data_ptr() + k), dp(b_ws), sp), "multi_pairing_batch")
        ms["baseline"] = timed(baseline)
        row = {"k": k, "l": l, "ms": ms}
        if has_verify:
            key = VKey()
            ic = np.ascontiguousarray(g1[(np.arange(l + 1) * 13 + 7) % 256])
            ctypes.memmove(key.alpha_g1, g1[0].ctypes.data, G1A)
            for field, rec in (("beta_g2", g2[0]), ("gamma_g2", g2[1]), ("delta_g2", g2[2])):
                ctypes.memmove(getattr(key, field), np.ascontiguousarray(rec).ctypes.data, G2A)
            key.ic, key.n_public = ic.ctypes.data, l + 1
            h = P(0)
            ck(lib.pa_groth16_vk_create(ctypes.byref(key), ctypes.byref(h)), "vk_create")
            row["vk_bytes"] = int(lib.pa_groth16_vk_bytes(h))
            proofs = np.ascontiguousarray(np.concatenate([a, b, c], axis=1))
            PR, X = to_dev(proofs), to_dev(fr_rows(k + l, max(k * l, 1)))
            valid = torch.empty(k, dtype=torch.uint8, device=dev)
            ws = torch.empty(lib.pa_groth16_verify_workspace_bytes(h, k), dtype=torch.uint8, device=dev)

            def verify():
                ck(lib.pa_groth16_verify_device(h, dp(PR), dp(X), l, 1, k, dp(valid), None, dp(ws), ws.numel(), sp),
                   "verify")
            ms["verify"] = timed(verify)
            for name, bound in (("verify_pairs3k", str(1 << 40)), ("verify_shared", "1")):
                os.environ[KNOB] = bound
                ms[name] = timed(verify)
            os.environ.pop(KNOB, None)
            # ---- stages ----
            sums = torch.empty((k, 13), dtype=torch.int64, device=dev)
            s_ws = torch.empty(max(lib.pa_groth16_vk_input_sum_workspace_bytes(h, k), 8), dtype=torch.uint8, device=dev)
            ms["input_sum"] = timed(lambda: ck(lib.pa_groth16_vk_input_sum_device(
                h, dp(X), l, 1, k, dp(sums), dp(s_ws), s_ws.numel(), sp), "input_sum"))
            SP = to_dev(np.concatenate([a, acc, c]))
            SQ = to_dev(np.concatenate([b, np.repeat(neg_gamma[None], k, 0), np.repeat(neg_delta[None], k, 0)]))
            ml = torch.empty((3 * k, 72), dtype=torch.int64, device=dev)
            ms["ml_pairs3k"] = timed(lambda: ck(lib.pa_pairing_miller_loop_batch_device(dp(SP), dp(SQ), dp(ml), 3 * k, sp),
                                                "miller loops"))
            prep = torch.empty((2, G2P // 8), dtype=torch.int64, device=dev)
            ck(lib.pa_g2_prepare_batch_device(P(SQ.data_ptr() + G2A * k), dp(prep), 1, sp), "prepare")
            ck(lib.pa_g2_prepare_batch_device(P(SQ.data_ptr() + G2A * 2 * k), P(prep.data_ptr() + G2P), 1, sp), "prepare")

            def ml_shared():
                ck(lib.pa_pairing_miller_loop_batch_device(dp(SP), dp(SQ), dp(ml), k, sp), "miller loops")
                ck(lib.pa_miller_loop_shared_prepared_device(P(SP.data_ptr() + G1A * k), k, dp(prep),
                                                             P(ml.data_ptr() + F12 * k), sp), "shared miller loop")
                ck(lib.pa_miller_loop_shared_prepared_device(P(SP.data_ptr() + G1A * 2 * k), k, P(prep.data_ptr() + G2P),
                                                             P(ml.data_ptr() + F12 * 2 * k), sp), "shared miller loop")
            ms["ml_shared"] = timed(ml_shared)
            fe_out = torch.empty((k, 72), dtype=torch.int64, device=dev)
            fe_ok = torch.empty(k, dtype=torch.uint8, device=dev)
            ms["final_exp"] = timed(lambda: ck(lib.pa_final_exponentiation_batch_device(dp(ml), dp(fe_out), dp(fe_ok), k, sp),
                                               "final exponentiation"))
            for comp in ("pairs3k", "shared"):
                ms["rest_" + comp] = [ms["verify_" + comp][0] - ms["input_sum"][0] - ms["ml_" + comp][0]
                                      - ms["final_exp"][0], None]
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
                ms["verify_encoded"] = timed(lambda: ck(lib.pa_groth16_verify_encoded_device(
                    h, dp(E), dp(X), l, 1, k, dp(valid), dp(status), None, dp(ws), ws.numel(), sp), "verify_encoded"))
                torch.cuda.synchronize()
                row["encoded_status_nonzero"] = int((status != 0).sum())
            torch.cuda.synchronize()
            lib.pa_groth16_vk_free(h)
        if (k, l) in against:
            row["parent_baseline_ms"] = against[(k, l)]
        results.append(row)
        fmt = lambda v: "%9.3f (%.3f)" % (v[0], v[1]) if v[1] is not None else "%9.3f        " % v[0]  # noqa: E731
        print("k = %6d  l = %3d" % (k, l))
        for name, v in ms.items():
            print("    %-16s %s ms" % (name, fmt(v)))
        if (k, l) in against:
            print("    %-16s %s ms" % ("parent baseline", fmt(against[(k, l)])))
        sys.stdout.flush()
    os.makedirs(args.out, exist_ok=True)
    path = os.path.join(args.out, args.tag + ".json")
    with open(path, "w") as f:
        json.dump({"lib": os.path.relpath(args.lib, ROOT), "device": torch.cuda.get_device_name(0), "rounds": args.rounds,
                   "calls": args.calls, "warmup": args.warmup, "unit": "ms: [median, max - min]", "cases": results},
                  f, indent=1)
    print("wrote", os.path.relpath(path, ROOT))


if __name__ == "__main__":
    main()
