"""G2MsmBases of the C++ mirror (include/pairing_amd.hpp):
tests/cpp/test_msm_g2.cpp compiles with g++ against the C ABI, and on the
device its prepare, multiexp and multiexp_batch (FrRepr and Montgomery rows)
at (17, 3) equal the C entry's words, the plain G2 multiexp's point and the
oracle's sums."""
import os
import subprocess

import numpy as np
import pytest

from helpers import R_ORDER, from_limbs, random_scalars, rng, small_scalars
from test_msm_g2_prepared import dressed

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIBDIR = os.path.join(ROOT, "pairing_amd", "lib")
SRC = os.path.join(ROOT, "tests", "cpp", "test_msm_g2.cpp")


def _compile(out):
    cmd = ["g++", "-std=c++17", "-O1", "-Wall", "-Wextra", "-Werror", "-I" + os.path.join(ROOT, "include"), SRC,
           "-o", out, "-L" + LIBDIR, "-lpairing_amd", "-Wl,-rpath," + LIBDIR, "-Wl,-rpath-link,/opt/rocm/lib"]
    subprocess.run(cmd, check=True, capture_output=True, text=True, timeout=300)


def test_cpp_g2_msm_probe_compiles_and_links(tmp_path):
    out = str(tmp_path / "test_msm_g2")
    _compile(out)
    assert os.path.getsize(out) > 0


@pytest.mark.gpu
def test_cpp_g2_msm_bases_on_gpu(oracle, tmp_path):
    m, k = 17, 3
    p, s0 = dressed(oracle, m, 670)
    s = np.concatenate([s0, random_scalars(rng(671), (k - 1) * m)])
    s = small_scalars([from_limbs(x) % R_ORDER for x in s])   # below r: the Montgomery overload's domain
    mont, ok = oracle.fr_from_repr(s)
    assert ok.all()
    exe = str(tmp_path / "test_msm_g2")
    _compile(exe)
    data, res = str(tmp_path / "data.bin"), str(tmp_path / "out.bin")
    with open(data, "wb") as f:
        f.write(np.array([m, k], np.uint64).tobytes())
        for arr in (p, s, mont):
            f.write(np.ascontiguousarray(arr, np.uint64).tobytes())
    r = subprocess.run([exe, data, res], capture_output=True, text=True, timeout=300)
    print(r.stdout, r.stderr)
    assert r.returncode == 0, r.stdout + r.stderr
    got = np.fromfile(res, np.uint64).reshape(k + 1, 36)
    for j in range(k):
        assert oracle.g2_eq(got[j:j + 1], oracle.g2_multiexp(p, s[j * m:(j + 1) * m], 8)).all(), j
    assert oracle.g2_eq(got[k:], oracle.g2_multiexp(p, s[:m], 8)).all()
