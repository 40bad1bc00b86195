"""Groth16Circuit and generate_parameters of the C++ mirror (include/pairing_amd.hpp):
tests/cpp/test_groth16_setup.cpp compiles with g++ against the C ABI, and on the
device its named vectors and its key() / vkey() views equal what
tests/groth16_setup_ref.py computes with the oracle for the log_n = 5 system."""
import os
import subprocess

import numpy as np
import pytest

import groth16_ref as G
import groth16_setup_ref as S
from helpers import small_scalars

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIBDIR = os.path.join(ROOT, "pairing_amd", "lib")
SRC = os.path.join(ROOT, "tests", "cpp", "test_groth16_setup.cpp")


def _compile(out):
    cmd = ["g++", "-std=c++17", "-O1", "-Wall", "-Wextra", "-Werror", "-I" + os.path.join(ROOT, "include"), SRC,
           "-o", out, "-L" + LIBDIR, "-lpairing_amd", "-Wl,-rpath," + LIBDIR, "-Wl,-rpath-link,/opt/rocm/lib"]
    subprocess.run(cmd, check=True, capture_output=True, text=True, timeout=300)


def test_cpp_groth16_setup_probe_compiles_and_links(tmp_path):
    out = str(tmp_path / "test_groth16_setup")
    _compile(out)
    assert os.path.getsize(out) > 0


@pytest.mark.gpu
def test_cpp_generate_parameters_on_gpu(oracle, tmp_path):
    mats, _ = G.satisfied_system(7300, 30, 12)
    st = S.Setup(mats, 12, 3, 5, S.trapdoor_of(7301))
    exe = str(tmp_path / "test_groth16_setup")
    _compile(exe)
    data = str(tmp_path / "data.bin")
    with open(data, "wb") as f:
        f.write(np.array([30, 12, 3, 5], np.uint64).tobytes())
        for m in mats:
            row_ptr, col, val = G.csr(m)
            f.write(np.array([len(col)], np.uint64).tobytes())
            f.write(row_ptr.tobytes())
            f.write(np.ascontiguousarray(col, np.uint32).tobytes())
            f.write(np.ascontiguousarray(val, np.uint64).tobytes())
        for arr in (oracle.g1_mul_generator(small_scalars([1]), 1), oracle.g2_mul_generator(small_scalars([1]), 1),
                    st.trapdoor_rows(), st.g1_points(oracle), st.g2_points(oracle)):
            f.write(np.ascontiguousarray(arr, np.uint64).tobytes())
    r = subprocess.run([exe, data], capture_output=True, text=True, timeout=300)
    print(r.stdout, r.stderr)
    assert r.returncode == 0, r.stdout + r.stderr
    assert r.stdout.count("ok  ") == 3 and "FAIL" not in r.stdout
