"""The aggregate check of the C++ mirror's Groth16Verifier (include/pairing_amd.hpp):
tests/cpp/test_groth16_aggregate.cpp compiles with g++ against the C ABI, and on
the device its k = 3 verdicts, gt, P array and decode statuses equal what
tests/groth16_aggregate_ref.py computes with the oracle."""
import os
import subprocess

import numpy as np
import pytest

import groth16_aggregate_ref as A
import groth16_ref as G
import groth16_verify_ref as V
from helpers import R_ORDER, rng
from test_fr_ntt import mont_rows

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIBDIR = os.path.join(ROOT, "pairing_amd", "lib")
SRC = os.path.join(ROOT, "tests", "cpp", "test_groth16_aggregate.cpp")


def _compile(out):
    cmd = ["g++", "-std=c++17", "-O1", "-Wall", "-Wextra", "-Werror", "-I" + os.path.join(ROOT, "include"), SRC,
           "-o", out, "-L" + LIBDIR, "-lpairing_amd", "-Wl,-rpath," + LIBDIR, "-Wl,-rpath-link,/opt/rocm/lib"]
    subprocess.run(cmd, check=True, capture_output=True, text=True, timeout=300)


def test_cpp_groth16_aggregate_probe_compiles_and_links(tmp_path):
    out = str(tmp_path / "test_groth16_aggregate")
    _compile(out)
    assert os.path.getsize(out) > 0


@pytest.mark.gpu
def test_cpp_groth16_aggregate_on_gpu(oracle, tmp_path):
    k = 3
    mats, w = G.satisfied_system(7800, 30, 12)
    key, gamma, ic = G.real_setup(7801, mats, 12, 3, 5)
    vk = V.real_vk(oracle, key, gamma, ic)
    g = rng(7802)
    spoiled = list(w)
    spoiled[8] = (spoiled[8] + 1) % R_ORDER
    good = G.ref_proofs(oracle, key, mats, [w, w, w], G.rand_fr(g, k), G.rand_fr(g, k))
    bad = good.copy()
    bad[1] = G.ref_proofs(oracle, key, mats, [spoiled], G.rand_fr(g, 1), G.rand_fr(g, 1))[0]
    inputs = [list(w[1:3]) for _ in range(k)]
    z = [v | 1 for v in A.rand_z(g, k)]
    assert A.ref_aggregate(oracle, vk, good, inputs, z)[1]
    gt, valid = A.ref_aggregate(oracle, vk, bad, inputs, z)
    assert not valid
    enc = V.encode_proofs(good)
    enc[2, 0] &= 0x7f                      # the third record's A without its compression flag
    status = V.decode_status(oracle, enc)
    assert status.tolist() == [[0, 0, 0], [0, 0, 0], [7, 0, 0]]
    exe = str(tmp_path / "test_groth16_aggregate")
    _compile(exe)
    data = str(tmp_path / "data.bin")
    with open(data, "wb") as f:
        f.write(np.array([vk.n_public, k], np.uint64).tobytes())
        for arr in vk.args() + (good, bad, mont_rows([x for row in inputs for x in row]), A.z_rows(z), gt,
                                A.ref_points(oracle, vk, bad, inputs, z)):
            f.write(np.ascontiguousarray(arr, np.uint64).tobytes())
        for arr in (enc, status):
            f.write(np.ascontiguousarray(arr, np.uint8).tobytes())
    r = subprocess.run([exe, data], capture_output=True, text=True, timeout=300)
    print(r.stdout, r.stderr)
    assert r.returncode == 0, r.stdout + r.stderr
    assert r.stdout.count("ok  ") == 3 and "FAIL" not in r.stdout
