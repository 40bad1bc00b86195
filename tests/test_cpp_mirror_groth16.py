"""R1cs and Groth16Prover of the C++ mirror (include/pairing_amd.hpp):
tests/cpp/test_groth16.cpp compiles with g++ against the C ABI, and on the
device its evaluation and its k = 2 proofs equal the words that
tests/groth16_ref.py computes from Python integers and the oracle."""
import os
import subprocess

import numpy as np
import pytest

import groth16_ref as G
from helpers import rng
from test_fr_ntt import mont_rows

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIBDIR = os.path.join(ROOT, "pairing_amd", "lib")
SRC = os.path.join(ROOT, "tests", "cpp", "test_groth16.cpp")


def _compile(out):
    cmd = ["g++", "-std=c++17", "-O1", "-Wall", "-Wextra", "-Werror", "-I" + os.path.join(ROOT, "include"), SRC,
           "-o", out, "-L" + LIBDIR, "-lpairing_amd", "-Wl,-rpath," + LIBDIR, "-Wl,-rpath-link,/opt/rocm/lib"]
    subprocess.run(cmd, check=True, capture_output=True, text=True, timeout=300)


def test_cpp_groth16_probe_compiles_and_links(tmp_path):
    out = str(tmp_path / "test_groth16")
    _compile(out)
    assert os.path.getsize(out) > 0


@pytest.mark.gpu
def test_cpp_groth16_prover_on_gpu(oracle, tmp_path):
    n_rows, n_vars, n_public, log_n, k = 50, 40, 3, 6, 2
    mats, w = G.satisfied_system(4200, n_rows, n_vars)
    key = G.random_key(4201, n_vars, n_public, log_n, (1 << log_n) - 1)
    g = rng(4202)
    ws = [w, [1] + G.rand_fr(g, n_vars - 1)]
    rs, ss = G.rand_fr(g, k), G.rand_fr(g, k)
    points = key.points(oracle)
    exe = str(tmp_path / "test_groth16")
    _compile(exe)
    data = str(tmp_path / "data.bin")
    with open(data, "wb") as f:
        f.write(np.array([n_rows, n_vars, n_public, log_n, len(key.h), k], np.uint64).tobytes())
        for arr in points[:10]:
            f.write(np.ascontiguousarray(arr, np.uint64).tobytes())
        for m in mats:
            row_ptr, col, val = G.csr(m)
            f.write(np.array([len(col)], np.uint64).tobytes())
            for arr in (row_ptr, col.astype(np.uint64), val):
                f.write(np.ascontiguousarray(arr, np.uint64).tobytes())
        for vals in ([v for x in ws for v in x], rs, ss):
            f.write(mont_rows(vals).tobytes())
        for arr in G.ref_eval(mats, ws, log_n):
            f.write(np.ascontiguousarray(arr, np.uint64).tobytes())
        f.write(G.ref_proofs(oracle, key, mats, ws, rs, ss).tobytes())
    r = subprocess.run([exe, data], capture_output=True, text=True, timeout=300)
    print(r.stdout, r.stderr)
    assert r.returncode == 0, r.stdout + r.stderr
    assert r.stdout.count("ok  ") == 2 and "FAIL" not in r.stdout
