"""The quotient of a proof on the device (pa_fr_ntt_quotient*, include/pairing_amd.h):

    h_j = coset_inverse((coset_forward(inverse(a_j)) * coset_forward(inverse(b_j))
                         - coset_forward(inverse(c_j))) * (g^n - 1)^-1)

Every value is canonical Fr, so every check is bit-exact.  The reference composes
tests/test_fr_ntt.py's reference transform with the oracle's fr_mul / fr_sub.
CPU: that reference against the definition on Python integers, the identity
h(x) (x^n - 1) = a(x) b(x) - c(x) for a satisfied system, and the checks of the
Python layers that need no device.  GPU (-m gpu): every size, batch shape and
pass structure (PA_NTT_TILE_LOG), aliasing and stream use, a satisfied system,
the chain into the batched multiexp, and a replay from a captured graph."""
import ctypes
import os
import re

import numpy as np
import pytest

from helpers import R_ORDER, rng
from test_fr import fr_val
from test_fr_ntt import GEN, big_int_ntt, inputs, mont_rows, omega, ref_ntt
from test_msm_prepared import base300  # noqa: F401  (a fixture)

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
HEADER = os.path.join(ROOT, "include", "pairing_amd.h")
NEW_SYMBOLS = ("pa_fr_ntt_quotient_workspace_bytes", "pa_fr_ntt_quotient_device", "pa_fr_ntt_quotient")


def zinv_row(k):
    return mont_rows([pow(pow(GEN, 1 << k, R_ORDER) - 1, -1, R_ORDER)])


def ref_quotient(oracle, a, b, c, k):
    """the quotient of each triple of polynomials ((batch * n, 4) rows each) from the reference transform
    and the oracle's fr_mul / fr_sub"""
    if a.shape[0] == 0:
        return np.zeros((0, 4), np.uint64)
    A, B, C = (ref_ntt(oracle, ref_ntt(oracle, x, k, "inverse"), k, "coset_forward") for x in (a, b, c))
    t = oracle.fr_sub(oracle.fr_mul(A, B), C)
    t = oracle.fr_mul(t, np.tile(zinv_row(k), (t.shape[0], 1)))
    return ref_ntt(oracle, t, k, "coset_inverse")


def triple(seed, nrows):
    return inputs(seed, nrows), inputs(seed + 50, nrows), inputs(seed + 100, nrows)


def horner(coeffs, x):
    acc = 0
    for v in reversed(coeffs):
        acc = (acc * x + v) % R_ORDER
    return acc


def assert_divides(oracle, a, b, c, h, k, seed):
    """h(x) (x^n - 1) = a(x) b(x) - c(x) at a random x, on Python integers, for every polynomial; a, b, c are
    evaluations over the domain (their coefficients: the reference's inverse transform), h coefficients"""
    n = 1 << k
    x = int.from_bytes(rng(seed).bytes(32), "little") % R_ORDER
    ca, cb, cc = ([fr_val(r) for r in ref_ntt(oracle, v, k, "inverse")] for v in (a, b, c))
    hv = [fr_val(r) for r in h]
    for j in range(a.shape[0] // n):
        s = slice(j * n, (j + 1) * n)
        lhs = horner(hv[s], x) * (pow(x, n, R_ORDER) - 1) % R_ORDER
        assert lhs == (horner(ca[s], x) * horner(cb[s], x) - horner(cc[s], x)) % R_ORDER, j


# ---------------- CPU ----------------

@pytest.mark.parametrize("k", range(6))
def test_reference_quotient_matches_big_integer_definition(oracle, k):
    n = 1 << k
    a, b, c = triple(2000 + k, n)
    va, vb, vc = ([fr_val(r) for r in x] for x in (a, b, c))
    A, B, C = (big_int_ntt(big_int_ntt(v, k, "inverse"), k, "coset_forward") for v in (va, vb, vc))
    zinv = pow(pow(GEN, n, R_ORDER) - 1, -1, R_ORDER)
    want = big_int_ntt([(x * y - z) * zinv % R_ORDER for x, y, z in zip(A, B, C)], k, "coset_inverse")
    got = ref_quotient(oracle, a, b, c, k)
    assert [fr_val(r) for r in got] == want
    assert (got == mont_rows(want)).all()   # canonical rows
    assert pow(GEN, n, R_ORDER) != 1
    # batched: polynomial by polynomial
    a3, b3, c3 = triple(2010 + k, 3 * n)
    got3 = ref_quotient(oracle, a3, b3, c3, k)
    for j in range(3):
        s = slice(j * n, (j + 1) * n)
        np.testing.assert_array_equal(got3[s], ref_quotient(oracle, a3[s], b3[s], c3[s], k))


@pytest.mark.parametrize("k", range(6))
def test_reference_quotient_of_a_satisfied_system(oracle, k):
    n = 1 << k
    a, b, _ = triple(2020 + k, 2 * n)
    c = oracle.fr_mul(a, b)
    h = ref_quotient(oracle, a, b, c, k)
    assert not h.reshape(2, n, 4)[:, n - 1].any()   # degree <= n - 2
    assert_divides(oracle, a, b, c, h, k, 2030 + k)
    assert h.any() or k == 0


def test_quotient_symbols_are_declared_and_bound():
    from pairing_amd import _native
    with open(HEADER) as f:
        src = f.read()
    declared = set(re.findall(r"^\s*(?:const\s+)?\w+\s*\*?\s*(pa_\w+)\s*\(", src, flags=re.M))
    for name in NEW_SYMBOLS:
        assert name in declared, name
        assert name in _native._SIGS, name
        assert getattr(_native._lib, name).argtypes == _native._SIGS[name]
    sz, p = ctypes.c_size_t, ctypes.c_void_p
    assert _native._lib.pa_fr_ntt_quotient_workspace_bytes.restype is sz
    assert _native._lib.pa_fr_ntt_quotient.restype is ctypes.c_int
    assert _native._lib.pa_fr_ntt_quotient_device.restype is ctypes.c_int
    assert _native._SIGS["pa_fr_ntt_quotient_workspace_bytes"] == [p, sz]
    assert _native._SIGS["pa_fr_ntt_quotient"] == [p, p, p, p, p, sz]
    assert _native._SIGS["pa_fr_ntt_quotient_device"] == [p, p, p, p, p, sz, p, sz, p]
    import pairing_amd
    import pairing_amd.device as pdev
    assert "fr_ntt_quotient" in pairing_amd.__all__ and hasattr(pairing_amd, "fr_ntt_quotient")
    assert hasattr(pdev, "fr_ntt_quotient") and hasattr(pdev, "fr_ntt_quotient_workspace_words")
    with open(os.path.join(ROOT, "include", "pairing_amd.hpp")) as f:
        assert re.search(r"std::vector<pa_fr> quotient\(", f.read())


def borrowed(log_n, ws_per_poly=0):
    """test_fr_ntt.py's borrowed handle (nobody may dereference it: the checks under test come before any
    native call), whose quotient workspace query answers as ws_per_poly bytes per polynomial triple would"""
    from pairing_amd import FrNttDomain

    class Borrowed(FrNttDomain):
        def quotient_workspace_bytes(self, batch):
            self.handle()
            return ws_per_poly * int(batch)

    return Borrowed(ctypes.c_void_p(8), log_n, owns=False)


def test_python_layer_checks_need_no_device():
    import pairing_amd as pa
    from pairing_amd import _native
    d = borrowed(3)
    z = lambda *s: np.zeros(s, np.uint64)  # noqa: E731
    for bad_rows in (1, 7, 9, 12):
        with pytest.raises(ValueError, match="multiple"):
            pa.fr_ntt_quotient(d, z(bad_rows, 4), z(bad_rows, 4), z(bad_rows, 4))
    for shapes in (((8, 4), (16, 4), (8, 4)), ((8, 4), (8, 4), (16, 4)), ((16, 4), (8, 4), (8, 4)),
                   ((8, 4), (0, 4), (8, 4))):
        with pytest.raises(ValueError, match="same shape"):
            pa.fr_ntt_quotient(d, *(z(*s) for s in shapes))
    with pytest.raises(ValueError):
        pa.fr_ntt_quotient(d, z(8, 5), z(8, 5), z(8, 5))
    with pytest.raises(ValueError, match="fr_ntt_domain"):
        pa.fr_ntt_quotient(object(), z(8, 4), z(8, 4), z(8, 4))
    out = pa.fr_ntt_quotient(d, z(0, 4), z(0, 4), z(0, 4))   # batch = 0: an empty array, no native call
    assert out.shape == (0, 4) and out.dtype == np.uint64
    # a NULL domain: a code from both entries, zero from the query
    lib = _native._lib
    assert lib.pa_fr_ntt_quotient(None, None, None, None, None, 1) == -1
    assert lib.pa_fr_ntt_quotient(None, None, None, None, None, 0) == -1
    assert lib.pa_fr_ntt_quotient_device(None, None, None, None, None, 1, None, 0, None) == -1
    assert lib.pa_fr_ntt_quotient_workspace_bytes(None, 4) == 0
    assert lib.pa_fr_ntt_quotient_workspace_bytes(None, 0) == 0
    d.close()
    with pytest.raises(ValueError, match="close"):
        pa.fr_ntt_quotient(d, z(8, 4), z(8, 4), z(8, 4))
    with pytest.raises(ValueError, match="close"):
        d.quotient_workspace_bytes(1)


def test_device_layer_rejects_bad_buffers_without_device():
    import torch
    import pairing_amd.device as pdev

    class FakeCuda:
        """shape/dtype/contiguity of a tensor, reporting is_cuda (tests/test_abi.py)"""
        def __init__(self, t):
            self.t = t
            self.is_cuda = True
            self.shape, self.dtype = t.shape, t.dtype

        def is_contiguous(self):
            return True

        def dim(self):
            return self.t.dim()

        def numel(self):
            return self.t.numel()

        def data_ptr(self):
            return 0

    f = lambda *s: FakeCuda(torch.zeros(*s, dtype=torch.int64))  # noqa: E731
    point, one_pass = borrowed(0), borrowed(3, ws_per_poly=3 * 8 * 32)
    assert pdev.fr_ntt_quotient_workspace_words(point, 5) == 0
    assert pdev.fr_ntt_quotient_workspace_words(one_pass, 5) == 5 * 3 * 8 * 4
    with pytest.raises(ValueError, match="out"):
        pdev.fr_ntt_quotient(point, f(16, 4), f(16, 4), f(16, 4), f(15, 4))
    with pytest.raises(ValueError, match="b has"):
        pdev.fr_ntt_quotient(point, f(16, 4), f(15, 4), f(16, 4), f(16, 4))
    with pytest.raises(ValueError, match="c has"):
        pdev.fr_ntt_quotient(point, f(16, 4), f(16, 4), f(8, 4), f(16, 4))
    with pytest.raises(ValueError, match="multiple"):
        pdev.fr_ntt_quotient(one_pass, f(12, 4), f(12, 4), f(12, 4), f(12, 4))
    with pytest.raises(ValueError, match="workspace"):
        pdev.fr_ntt_quotient(one_pass, f(16, 4), f(16, 4), f(16, 4), f(16, 4))
    with pytest.raises(ValueError, match="workspace"):
        pdev.fr_ntt_quotient(one_pass, f(16, 4), f(16, 4), f(16, 4), f(16, 4), workspace=f(2 * 3 * 8 * 4 - 1))
    with pytest.raises(ValueError, match="shape"):
        pdev.fr_ntt_quotient(point, f(16, 4), f(16, 5), f(16, 4), f(16, 4))
    with pytest.raises(ValueError, match="fr_ntt_domain"):
        pdev.fr_ntt_quotient(object(), f(16, 4), f(16, 4), f(16, 4), f(16, 4))
    with pytest.raises(ValueError, match="CUDA"):   # a CPU tensor, before any device call
        pdev.fr_ntt_quotient(point, *(torch.zeros(4, 4, dtype=torch.int64) for _ in range(4)))
    one_pass.close()
    with pytest.raises(ValueError, match="close"):
        pdev.fr_ntt_quotient(one_pass, f(16, 4), f(16, 4), f(16, 4), f(16, 4))
    with pytest.raises(ValueError, match="close"):
        pdev.fr_ntt_quotient_workspace_words(one_pass, 1)


CPP_SRC = os.path.join(ROOT, "tests", "cpp", "test_fr_ntt_quotient.cpp")
LIBDIR = os.path.join(ROOT, "pairing_amd", "lib")


def _compile_cpp(out):
    import subprocess
    cmd = ["g++", "-std=c++17", "-O1", "-Wall", "-Wextra", "-Werror", "-I" + os.path.join(ROOT, "include"), CPP_SRC,
           "-o", out, "-L" + LIBDIR, "-lpairing_amd", "-Wl,-rpath," + LIBDIR, "-Wl,-rpath-link,/opt/rocm/lib"]
    subprocess.run(cmd, check=True, capture_output=True, text=True, timeout=300)


def test_cpp_wrapper_compiles_and_links(tmp_path):
    out = str(tmp_path / "test_fr_ntt_quotient")
    _compile_cpp(out)
    assert os.path.getsize(out) > 0


# ---------------- GPU ----------------

@pytest.mark.gpu
def test_cpp_wrapper_on_gpu(oracle, tmp_path):
    """pairing_amd::FrNttDomain::quotient against the reference quotient at k = 7, batch 3"""
    import subprocess
    k, batch = 7, 3
    a, b, c = triple(2100, batch << k)
    data = str(tmp_path / "data.bin")
    with open(data, "wb") as f:
        f.write(np.array([k, batch], np.uint64).tobytes())
        for x in (a, b, c, ref_quotient(oracle, a, b, c, k), np.tile(zinv_row(k), (batch << k, 1))):
            f.write(np.ascontiguousarray(x).tobytes())
    exe = str(tmp_path / "test_fr_ntt_quotient")
    _compile_cpp(exe)
    r = subprocess.run([exe, data], capture_output=True, text=True, timeout=120)
    print(r.stdout, r.stderr)
    assert r.returncode == 0, r.stdout + r.stderr
    assert r.stdout.count("ok  ") == 6 and "FAIL" not in r.stdout


def _dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a).view(np.int64)).to("cuda:0")


def _host(t):
    return t.cpu().numpy().view(np.uint64)


def _workspace(pdev, d, batch):
    """exactly the queried size"""
    import torch
    words = pdev.fr_ntt_quotient_workspace_words(d, batch)
    assert words * 8 == d.quotient_workspace_bytes(batch)
    return torch.empty(words, dtype=torch.int64, device="cuda:0") if words else None


@pytest.mark.gpu
@pytest.mark.parametrize("k", range(13))
def test_every_size_matches_reference(gpu, oracle, k):
    n = 1 << k
    a, b, c = triple(2200 + k, n)
    with gpu.fr_ntt_domain(k) as d:
        np.testing.assert_array_equal(gpu.fr_ntt_quotient(d, a, b, c), ref_quotient(oracle, a, b, c, k))
        # the workspace: three coset evaluations, and a pass workspace for three arrays beside them
        want = 0 if k == 0 else (3 if d.passes == 1 else 6) * n * 32
        assert d.quotient_workspace_bytes(1) == want and d.quotient_workspace_bytes(5) == 5 * want
        assert d.quotient_workspace_bytes(0) == 0
        assert d.quotient_workspace_bytes(1 << 40) == 0   # no grid holds it: the entries refuse, the query says 0


@pytest.mark.gpu
@pytest.mark.parametrize("k,batch", [(0, 5), (1, 3), (6, 7), (8, 33), (10, 3)])
def test_batched(gpu, oracle, k, batch):
    a, b, c = triple(2300 + 16 * k + batch, batch << k)
    with gpu.fr_ntt_domain(k) as d:
        np.testing.assert_array_equal(gpu.fr_ntt_quotient(d, a, b, c), ref_quotient(oracle, a, b, c, k))


@pytest.mark.gpu
def test_batches_at_the_workgroup_sharing_boundaries(gpu, oracle):
    """a one-pass domain puts polys_per_workgroup polynomials in a workgroup; the grid over three arrays has
    a tail of columns for each array: that many fill an array's last workgroup exactly, one more starts another"""
    seen = set()
    for k in range(1, 13):
        with gpu.fr_ntt_domain(k) as d:
            ppw = d.polys_per_workgroup
            if d.passes != 1:
                continue
            seen.add(ppw)
            for batch in (ppw, ppw + 1):
                a, b, c = triple(2400 + 2 * k + (batch - ppw), batch << k)
                np.testing.assert_array_equal(gpu.fr_ntt_quotient(d, a, b, c), ref_quotient(oracle, a, b, c, k),
                                              err_msg="%d %d" % (k, batch))
    assert len(seen) >= 5


@pytest.fixture(scope="module")
def pass_case(oracle):
    """one k = 12 and one k = 9 triple, two polynomials each, with the reference quotient"""
    out = {}
    for k in (12, 9):
        a, b, c = triple(2500 + k, 2 << k)
        out[k] = (a, b, c, ref_quotient(oracle, a, b, c, k))
    return out


@pytest.mark.gpu
@pytest.mark.parametrize("k,tile,passes", [(12, 12, 1), (12, 6, 2), (12, 5, 3), (9, 4, 3), (9, 1, 9), (12, 0, 12)])
def test_pass_structure(gpu, pass_case, monkeypatch, k, tile, passes):
    a, b, c, want = pass_case[k]
    monkeypatch.delenv("PA_NTT_TILE_LOG", raising=False)
    with gpu.fr_ntt_domain(k) as d:
        default = gpu.fr_ntt_quotient(d, a, b, c)
        assert d.tile_log == 10
    monkeypatch.setenv("PA_NTT_TILE_LOG", str(tile))
    with gpu.fr_ntt_domain(k) as d:
        assert d.passes == passes and 1 <= d.tile_log <= 12
        assert d.quotient_workspace_bytes(2) == (3 if passes == 1 else 6) * (2 << k) * 32
        got = gpu.fr_ntt_quotient(d, a, b, c)
    np.testing.assert_array_equal(got, want)
    np.testing.assert_array_equal(got, default)


@pytest.mark.gpu
@pytest.mark.parametrize("k", [9, 12])
def test_aliasing_streams_and_untouched_rows(gpu, oracle, k):
    import torch
    import pairing_amd.device as pdev
    from pairing_amd import _native
    batch, n = 2, 1 << k
    rows = batch * n
    a, b, c = triple(2600 + k, rows)
    guard = np.full((3, 4), 0x5a5a5a5a5a5a5a5a, np.uint64)
    want = ref_quotient(oracle, a, b, c, k)
    want_sq = ref_quotient(oracle, a, a, c, k)
    s = torch.cuda.Stream()
    with gpu.fr_ntt_domain(k) as d:
        ws = _workspace(pdev, d, batch)
        assert ws is not None

        def run(A, B, C, out):
            torch.cuda.synchronize()
            with torch.cuda.stream(s):
                pdev.fr_ntt_quotient(d, A, B, C, out, workspace=ws, stream=s)
            s.synchronize()

        # a fresh output, over the first rows of a longer tensor
        A, B, C = _dev(a), _dev(b), _dev(c)
        out = _dev(np.concatenate([np.zeros_like(a), guard]))
        run(A, B, C, out)
        np.testing.assert_array_equal(_host(out)[:rows], want)
        np.testing.assert_array_equal(_host(out)[rows:], guard)
        for t, x in ((A, a), (B, b), (C, c)):
            np.testing.assert_array_equal(_host(t), x)   # the inputs are only read
        # out = a, b, c in turn
        for alias in range(3):
            src = [a, b, c]
            t = [_dev(x) for x in src]
            t[alias] = _dev(np.concatenate([src[alias], guard]))
            ins = [x[:rows] for x in t]
            run(ins[0], ins[1], ins[2], t[alias])
            np.testing.assert_array_equal(_host(t[alias])[:rows], want, err_msg="out = %s" % "abc"[alias])
            np.testing.assert_array_equal(_host(t[alias])[rows:], guard)
            for i in range(3):
                if i != alias:
                    np.testing.assert_array_equal(_host(t[i]), src[i], err_msg="input %d, out = %d" % (i, alias))
        # a = b: a^2 - c, into a fresh output and into a itself
        A, C = _dev(a), _dev(c)
        out = _dev(np.concatenate([np.zeros_like(a), guard]))
        run(A, A, C, out)
        np.testing.assert_array_equal(_host(out)[:rows], want_sq)
        np.testing.assert_array_equal(_host(out)[rows:], guard)
        np.testing.assert_array_equal(_host(A), a)
        np.testing.assert_array_equal(_host(C), c)
        run(A, A, C, A)
        np.testing.assert_array_equal(_host(A), want_sq)
        assert not np.array_equal(want_sq, want)
        # what the C entry refuses before a launch: partial overlap with any input, a short workspace
        A, B, C = _dev(a), _dev(b), _dev(c)
        big = _dev(np.concatenate([a, a]))
        p = lambda t, off=0: ctypes.c_void_p(t.data_ptr() + off)  # noqa: E731
        sp = ctypes.c_void_p(s.cuda_stream)
        wsb = ws.numel() * 8
        dev = _native._lib.pa_fr_ntt_quotient_device
        h = d.handle()
        assert dev(h, p(big), p(B), p(C), p(big, 32), batch, p(ws), wsb, sp) == -1
        assert dev(h, p(A), p(big, 32 * rows - 32), p(C), p(big), batch, p(ws), wsb, sp) == -1
        assert dev(h, p(A), p(B), p(big, 64), p(big), batch, p(ws), wsb, sp) == -1
        assert dev(h, p(A), p(B), p(C), p(A), batch, p(ws), wsb - 1, sp) == -1
        assert dev(h, p(A), p(B), p(C), p(A), batch, None, 0, sp) == -1
        assert dev(h, None, p(B), p(C), p(A), batch, p(ws), wsb, sp) == -1
        assert dev(h, p(A), p(B), p(C), None, batch, p(ws), wsb, sp) == -1
        assert dev(h, None, None, None, None, 0, None, 0, sp) == 0   # batch = 0: a no-op
        torch.cuda.synchronize()
        for t, x in ((A, a), (B, b), (C, c)):
            np.testing.assert_array_equal(_host(t), x)   # nothing was launched


@pytest.mark.gpu
def test_satisfied_system(gpu, oracle):
    k, batch = 10, 3
    n = 1 << k
    a, b, _ = triple(2700, batch * n)
    c = oracle.fr_mul(a, b)
    with gpu.fr_ntt_domain(k) as d:
        h = gpu.fr_ntt_quotient(d, a, b, c)
    np.testing.assert_array_equal(h, ref_quotient(oracle, a, b, c, k))
    assert not h.reshape(batch, n, 4)[:, n - 1].any()   # degree <= n - 2
    assert h.reshape(batch, n, 4)[:, n - 2].any(axis=1).all()
    assert_divides(oracle, a, b, c, h, k, 2710)


@pytest.mark.gpu
def test_quotient_to_h_query_chain_stays_on_the_device(gpu, oracle, base300):
    """a proof's H term: the quotient's Montgomery rows go into the batched multiexp where they lie"""
    import torch
    import pairing_amd.device as pdev
    k, batch = 8, 4
    n = 1 << k
    p = np.ascontiguousarray(base300[0][:n])
    a, b, _ = triple(2800, batch * n)
    c = oracle.fr_mul(a, b)
    c[n:] = inputs(2801, (batch - 1) * n)   # one satisfied system, three arbitrary triples
    with gpu.fr_ntt_domain(k) as d:
        prepared = pdev.msm_prepare(_dev(p))
        h = pdev.empty_records(batch * n, 4, "cuda:0")
        pdev.fr_ntt_quotient(d, _dev(a), _dev(b), _dev(c), h, workspace=_workspace(pdev, d, batch))
        out = pdev.empty_records(batch, 18, "cuda:0")
        ws = pdev.multiexp_prepared_batch_workspace(prepared, n, batch, "cuda:0")
        pdev.multiexp_prepared_batch(prepared, h, n, batch, out, ws, montgomery=True)
        torch.cuda.synchronize()
        prepared.close()
    hh = _host(h)
    np.testing.assert_array_equal(hh, ref_quotient(oracle, a, b, c, k))
    got = _host(out)
    with gpu.g1_msm_prepare(p) as bases:
        for j in range(batch):
            s = oracle.fr_into_repr(np.ascontiguousarray(hh[j * n:(j + 1) * n]))
            assert oracle.g1_eq(got[j:j + 1], gpu.g1_multiexp_prepared(bases, s)).all(), "vector %d" % j


def _hip_runtime():
    """the HIP runtime this process already runs on, by the path it was loaded from"""
    with open("/proc/self/maps") as f:
        paths = {line.split()[-1] for line in f if "libamdhip64" in line}
    assert len(paths) == 1, paths
    return ctypes.CDLL(paths.pop())


@pytest.mark.gpu
def test_replays_from_a_graph(gpu, oracle):
    """one k = 10 quotient captured on a side stream (test_fr_ntt.py's pattern) and replayed twice on fresh
    inputs; captured on its own, the call is 3 x passes kernel nodes in one linear chain"""
    import torch
    import pairing_amd.device as pdev
    k, n = 10, 1 << 10
    sets = [triple(2900 + i, n) for i in range(3)]
    with gpu.fr_ntt_domain(k) as d:
        A, B, C = (_dev(x) for x in sets[0])
        out = pdev.empty_records(n, 4, "cuda:0")
        ws = _workspace(pdev, d, 1)
        s = torch.cuda.Stream()
        s.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(s):
            pdev.fr_ntt_quotient(d, A, B, C, out, workspace=ws)
        torch.cuda.synchronize()
        np.testing.assert_array_equal(_host(out), ref_quotient(oracle, *sets[0], k))
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g, stream=s, capture_error_mode="relaxed"):
            pdev.fr_ntt_quotient(d, A, B, C, out, workspace=ws)
        torch.cuda.synchronize()
        for fresh in sets[1:]:
            for t, x in zip((A, B, C), fresh):
                t.copy_(_dev(x))
            out.zero_()
            g.replay()
            torch.cuda.synchronize()
            np.testing.assert_array_equal(_host(out), ref_quotient(oracle, *fresh, k))
        # the shape of the capture: nodes and edges of the call alone
        hip = _hip_runtime()
        vp, sz = ctypes.c_void_p, ctypes.c_size_t
        hip.hipStreamBeginCapture.argtypes = [vp, ctypes.c_int]
        hip.hipStreamEndCapture.argtypes = [vp, ctypes.POINTER(vp)]
        hip.hipGraphGetNodes.argtypes = [vp, ctypes.POINTER(vp), ctypes.POINTER(sz)]
        hip.hipGraphGetEdges.argtypes = [vp, ctypes.POINTER(vp), ctypes.POINTER(vp), ctypes.POINTER(sz)]
        hip.hipGraphDestroy.argtypes = [vp]
        graph = vp(0)
        assert hip.hipStreamBeginCapture(vp(s.cuda_stream), 2) == 0   # hipStreamCaptureModeRelaxed
        try:
            pdev.fr_ntt_quotient(d, A, B, C, out, workspace=ws, stream=s)
        finally:
            assert hip.hipStreamEndCapture(vp(s.cuda_stream), ctypes.byref(graph)) == 0
        nodes, edges = sz(0), sz(0)
        assert hip.hipGraphGetNodes(graph, None, ctypes.byref(nodes)) == 0
        assert hip.hipGraphGetEdges(graph, None, None, ctypes.byref(edges)) == 0
        assert nodes.value == 3 * d.passes
        src, dst = (vp * edges.value)(), (vp * edges.value)()
        assert hip.hipGraphGetEdges(graph, src, dst, ctypes.byref(edges)) == 0
        assert edges.value == nodes.value - 1
        assert len(set(src)) == len(set(dst)) == edges.value   # no node has two successors or two predecessors
        assert hip.hipGraphDestroy(graph) == 0
        torch.cuda.synchronize()
