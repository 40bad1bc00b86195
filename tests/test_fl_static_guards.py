"""fl.h: "a formula that would overflow does not compile".  Three tiny
translation units that break a column or subtrahend bound must each stop at
the static_assert that names it, and a legal one must compile (device-only
cross-compilation for gfx950, no GPU needed).  Skipped where hipcc is absent."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "pairing_amd", "csrc")

UNIT = """#include "fl.h"
using namespace pa;
extern "C" __global__ void guard_unit(const uint32_t* in, uint32_t* out) {
    F<%(A)d> a;
    F<%(B)d> b;
    for (int i = 0; i < 14; i++) { a.w[i] = in[i]; b.w[i] = in[16 + i]; }
    const auto r = %(EXPR)s;
    for (int i = 0; i < 14; i++) out[i] = r.w[i];
}
"""


def _hipcc():
    for cand in (os.environ.get("HIPCC"), "/opt/rocm/bin/hipcc", shutil.which("hipcc")):
        if cand and os.path.exists(cand):
            return cand
    return None


def _compile(tmp_path, name, a, b, expr):
    hipcc = _hipcc()
    if hipcc is None:
        pytest.skip("hipcc not found")
    src = tmp_path / (name + ".hip")
    src.write_text(UNIT % {"A": a, "B": b, "EXPR": expr})
    return subprocess.run([hipcc, "-O1", "--offload-arch=gfx950", "-std=c++17", "--cuda-device-only",
                           "--no-gpu-bundle-output", "-I", CSRC, "-c", str(src), "-o", str(tmp_path / (name + ".o"))],
                          capture_output=True, text=True, timeout=300)


@pytest.mark.parametrize("name,a,b,expr,message", [
    ("mul_4_5", 4, 5, "mul(a, b)", "product column bound"),
    ("sqr_4", 4, 1, "sqr(a)", "square column bound"),
    ("neg_14", 14, 1, "neg(a)", "lazy bound out of range"),
    ("sop_24", 4, 4, "sop(a, b, add(b, b), relax<1>(red(a)))", "sum-of-products column bound"),
])
def test_overflowing_formula_does_not_compile(tmp_path, name, a, b, expr, message):
    r = _compile(tmp_path, name, a, b, expr)
    assert r.returncode != 0, "%s compiled" % expr
    assert "static assertion failed" in r.stderr and message in r.stderr, r.stderr[-2000:]


def test_formula_at_the_bound_compiles(tmp_path):
    r = _compile(tmp_path, "legal", 4, 4, "sop(a, b, red(a), relax<1>(red(b)))")   # 4*4 + 1*1 = 17
    assert r.returncode == 0, r.stderr[-2000:]
    r = _compile(tmp_path, "legal_neg", 13, 3, "sqr(add(red(neg(a)), red(dbl(b))))")
    assert r.returncode == 0, r.stderr[-2000:]
