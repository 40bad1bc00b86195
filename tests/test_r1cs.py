"""R1CS matrices on the device and their product with k witnesses (pa_r1cs_*,
include/pairing_amd.h): a[j n + i] = sum_t val[t] w_j[col[t]] over row i of A,
likewise b and c, rows from n_rows up to n = 2^log_n zero.  Every value is
canonical, so the device's rows are compared bit for bit with Python integers
(tests/groth16_ref.py).  The rows of more than pa_r1cs_chunk_len() terms go
through the partial sums and the fold launch; the lengths around multiples of
that constant are read from the library at run time."""
import ctypes
import os
import re

import numpy as np
import pytest

import groth16_ref as G
from helpers import R_ORDER, rng
from test_fr_ntt import mont_rows

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
HEADER = os.path.join(ROOT, "include", "pairing_amd.h")
P, N, U = ctypes.c_void_p, ctypes.c_size_t, ctypes.c_uint
NEW_SIGS = {
    "pa_r1cs_create": [P, P, P, N, N, ctypes.POINTER(P)],
    "pa_r1cs_eval_device": [P, P, N, U, P, P, P, P, N, P],
    "pa_r1cs_eval": [P, P, N, U, P, P, P],
    "pa_r1cs_rows": [P], "pa_r1cs_cols": [P], "pa_r1cs_bytes": [P],
    "pa_r1cs_eval_workspace_bytes": [P, N],
}
SIZE_T = ("pa_r1cs_rows", "pa_r1cs_cols", "pa_r1cs_bytes", "pa_r1cs_eval_workspace_bytes", "pa_r1cs_chunk_len")
SENTINEL = 0x5a5a5a5a5a5a5a5a


def log_for(n_rows):
    return max(n_rows - 1, 0).bit_length()


# ---------------- CPU ----------------

def test_reference_product_on_a_hand_example():
    # A = [[2 w0 + 3 w2], [], [w1 + w1]]; w = (5, 7, 11)
    mats = ([[(0, 2), (2, 3)], [], [(1, 1), (1, 1)]], [[], [], []], [[(0, R_ORDER - 1)], [(1, 0)], [(2, 1)]])
    a, b, c = G.eval_ints(mats, [[5, 7, 11]], 2)
    assert a == [43, 0, 14, 0] and b == [0, 0, 0, 0] and c == [R_ORDER - 5, 0, 11, 0]
    rp, col, val = G.csr(mats[0])
    assert rp.tolist() == [0, 2, 2, 4] and col.tolist() == [0, 2, 1, 1] and val.shape == (4, 4)
    assert (G.ref_eval(mats, [[5, 7, 11]], 2)[0] == mont_rows([43, 0, 14, 0])).all()


def test_r1cs_symbols_are_declared_and_bound():
    from pairing_amd import _native
    with open(HEADER) as f:
        src = f.read()
    declared = set(re.findall(r"^\s*(?:const\s+)?\w+\s*\*?\s*(pa_\w+)\s*\(", src, flags=re.M))
    for name, sig in NEW_SIGS.items():
        assert name in declared, name
        assert _native._SIGS[name] == sig, name
        assert getattr(_native._lib, name).argtypes == sig
    for name in ("pa_r1cs_free", "pa_r1cs_chunk_len"):
        assert name in declared and hasattr(_native._lib, name), name
    for name in SIZE_T:
        assert getattr(_native._lib, name).restype is N, name
    assert _native._lib.pa_r1cs_free.restype is None
    assert _native._lib.pa_r1cs_eval.restype is ctypes.c_int
    assert re.search(r"typedef\s+struct\s+pa_r1cs\s+pa_r1cs\s*;", src) and "} pa_fr_csr;" in src
    import pairing_amd
    import pairing_amd.device as pdev
    for name in ("R1cs", "r1cs", "r1cs_eval", "R1CS_CHUNK_LEN"):
        assert name in pairing_amd.__all__ and hasattr(pairing_amd, name), name
    assert hasattr(pdev, "r1cs_eval") and hasattr(pdev, "r1cs_eval_workspace_words")
    assert pairing_amd.R1CS_CHUNK_LEN == _native._lib.pa_r1cs_chunk_len() >= 2
    with open(os.path.join(ROOT, "include", "pairing_amd.hpp")) as f:
        hpp = f.read()
    assert re.search(r"class R1cs\b", hpp) and re.search(r"\beval\(", hpp)


def _raw_csr(rp, col, val):
    from pairing_amd._native import FrCsr
    rp, col, val = (np.ascontiguousarray(x, t) for x, t in ((rp, np.uint64), (col, np.uint32), (val, np.uint64)))
    return FrCsr(P(rp.ctypes.data), P(col.ctypes.data), P(val.ctypes.data)), (rp, col, val)


def test_create_refuses_bad_matrices_before_touching_a_device():
    """every listed creation error, through the C entry (its checks come before the first HIP call)"""
    from pairing_amd import _native
    lib = _native._lib
    one = mont_rows([1, 2])
    good, keep0 = _raw_csr([0, 1, 2], [0, 1], one)
    r_row = np.array([[R_ORDER >> (64 * i) & (2**64 - 1) for i in range(4)]], np.uint64)
    bad = {
        "row_ptr[0] != 0": _raw_csr([1, 1, 2], [0, 1], one),
        "row_ptr decreases": _raw_csr([0, 2, 1], [0, 1], one),
        "column >= n_cols": _raw_csr([0, 1, 2], [0, 2], one),
        "value = r": _raw_csr([0, 1, 2], [0, 1], np.concatenate([one[:1], r_row])),
        "value = 2^256 - 1": _raw_csr([0, 1, 2], [0, 1], np.full((2, 4), 2**64 - 1, np.uint64)),
        "nnz = 2^32": _raw_csr([0, 1, 1 << 32], [0, 1], one),
    }
    for what, (m, _keep) in bad.items():
        for pos in range(3):
            ms = [good, good, good]
            ms[pos] = m
            h = P(0x1234)
            rc = lib.pa_r1cs_create(*(ctypes.byref(x) for x in ms), 2, 2, ctypes.byref(h))
            assert rc == -1 and h.value is None, (what, pos)
            assert lib.pa_last_error()
    assert lib.pa_r1cs_create(None, None, None, 0, 0, ctypes.byref(P(0))) == -1
    assert lib.pa_r1cs_create(ctypes.byref(good), ctypes.byref(good), ctypes.byref(good), 2, 2, None) == -1
    # NULL objects
    assert lib.pa_r1cs_rows(None) == lib.pa_r1cs_cols(None) == lib.pa_r1cs_bytes(None) == 0
    assert lib.pa_r1cs_eval_workspace_bytes(None, 3) == 0
    assert lib.pa_r1cs_eval(None, None, 1, 0, None, None, None) == -1
    assert lib.pa_r1cs_eval_device(None, None, 1, 0, None, None, None, None, 0, None) == -1
    lib.pa_r1cs_free(None)
    del keep0


def test_python_layers_check_arguments_without_a_device():
    import torch
    import pairing_amd as pa
    import pairing_amd.device as pdev
    from pairing_amd._native import R1cs
    v = mont_rows([1, 2])
    ok = ([0, 1, 2], [0, 1], v)
    for a, what in ((([1, 1, 2], [0, 1], v), "row_ptr"), (([0, 2, 1], [0, 1], v), "row_ptr"),
                    (([0, 1], [0], v[:1]), "row_ptr"), (([0, 1, 2], [0, 2], v), "column"),
                    (([0, 1, 2], [0, -1], v), "column"), (([0, 1, 2], [0], v), "col"),
                    (([0, 1, 2], [0, 1], v[:1]), "val"), (([0, 1, 2], [0, 1], np.zeros((2, 5), np.uint64)), "val"),
                    (([0.0, 1.0, 2.0], [0, 1], v), "row_ptr"), (5, "triple")):
        with pytest.raises(ValueError, match=what):
            pa.r1cs(a, ok, ok, 2, 2)
        with pytest.raises(ValueError, match=what):
            pa.r1cs(ok, ok, a, 2, 2)
    with pytest.raises(ValueError):
        pa.r1cs(ok, ok, ok, -1, 2)
    with pytest.raises(ValueError, match="r1cs"):
        pa.r1cs_eval(object(), np.zeros((2, 4), np.uint64), 1)
    fake = R1cs(P(1), 5, 3, owns=False)   # a live-looking handle: every error below comes before a native call
    z = np.zeros
    with pytest.raises(ValueError, match="rows"):
        pa.r1cs_eval(fake, z((3, 4), np.uint64), 2)        # 4 points for 5 rows
    with pytest.raises(ValueError, match="log_n"):
        pa.r1cs_eval(fake, z((3, 4), np.uint64), 29)
    with pytest.raises(ValueError, match="vectors"):
        pa.r1cs_eval(fake, z((4, 4), np.uint64), 3)        # not a multiple of cols
    with pytest.raises(ValueError, match="vectors"):
        pa.r1cs_eval(fake, z((6, 4), np.uint64), 3, count=3)
    with pytest.raises(ValueError, match="shape"):
        pa.r1cs_eval(fake, z((3, 5), np.uint64), 3)
    t = lambda *s: torch.zeros(*s, dtype=torch.int64)  # noqa: E731  (CPU tensors: refused as such)
    with pytest.raises(ValueError, match="r1cs"):
        pdev.r1cs_eval(object(), t(3, 4), 3, t(8, 4), t(8, 4), t(8, 4))
    with pytest.raises(ValueError, match="rows"):
        pdev.r1cs_eval(fake, t(3, 4), 2, t(8, 4), t(8, 4), t(8, 4))
    with pytest.raises(ValueError, match="vectors"):
        pdev.r1cs_eval(fake, t(4, 4), 3, t(8, 4), t(8, 4), t(8, 4))
    with pytest.raises(ValueError, match="needs 16"):
        pdev.r1cs_eval(fake, t(6, 4), 3, t(16, 4), t(15, 4), t(16, 4))
    with pytest.raises(ValueError, match="CUDA"):
        pdev.r1cs_eval(fake, t(3, 4), 3, t(8, 4), t(8, 4), t(8, 4))
    fake.close()
    with pytest.raises(ValueError, match="close"):
        pa.r1cs_eval(fake, z((3, 4), np.uint64), 3)
    with pytest.raises(ValueError, match="close"):
        pdev.r1cs_eval_workspace_words(fake, 1)


# ---------------- GPU ----------------

def witnesses(seed, k, n_cols):
    g = rng(seed)
    return [G.rand_fr(g, n_cols) for _ in range(k)]


def flat(ws):
    vals = [v for w in ws for v in w]
    return mont_rows(vals) if vals else np.zeros((0, 4), np.uint64)


def check_host(gpu, mats, n_rows, n_cols, ws, log_n):
    want = G.ref_eval(mats, ws, log_n)
    with gpu.r1cs(*(G.csr(m) for m in mats), n_rows, n_cols) as sysm:
        assert (sysm.rows, sysm.cols) == (n_rows, n_cols) and sysm.bytes >= 0
        got = gpu.r1cs_eval(sysm, flat(ws), log_n, count=len(ws))
    for g, w, name in zip(got, want, "abc"):
        np.testing.assert_array_equal(g, w, err_msg=name)


@pytest.mark.gpu
@pytest.mark.parametrize("n_cols", [1, 7, 300])
@pytest.mark.parametrize("n_rows", [0, 1, 5, 64, 65, 300])
def test_sizes_match_python_integers(gpu, n_rows, n_cols):
    mats = G.random_system(3000 + 7 * n_rows + n_cols, n_rows, n_cols)
    for k in (1, 3):
        check_host(gpu, mats, n_rows, n_cols, witnesses(3100 + k, k, n_cols), log_for(n_rows))


@pytest.mark.gpu
def test_padding_exact_size_and_a_single_point(gpu):
    from pairing_amd import _native
    # 5 rows into 8 points, the outputs pre-filled: rows 5..7 must come back zero
    mats = G.random_system(3200, 5, 7)
    ws = witnesses(3201, 2, 7)
    want = G.ref_eval(mats, ws, 3)
    with gpu.r1cs(*(G.csr(m) for m in mats), 5, 7) as sysm:
        outs = [np.full((16, 4), SENTINEL, np.uint64) for _ in range(3)]
        w = flat(ws)
        rc = _native._lib.pa_r1cs_eval(sysm.handle(), _native.ptr(w), 2, 3, *(_native.ptr(o) for o in outs))
        assert rc == 0
        for o, x in zip(outs, want):
            np.testing.assert_array_equal(o, x)
            assert not o.reshape(2, 8, 4)[:, 5:].any()
        # k = 0 writes nothing
        rc = _native._lib.pa_r1cs_eval(sysm.handle(), None, 0, 3, None, None, None)
        assert rc == 0
        assert all(x.shape == (0, 4) for x in gpu.r1cs_eval(sysm, np.zeros((0, 4), np.uint64), 3))
        assert sysm.eval_workspace_bytes(5) == 0   # no row of several chunks
    # n_rows = 2^log_n exactly, and a larger domain than needed
    mats = G.random_system(3210, 64, 7)
    check_host(gpu, mats, 64, 7, witnesses(3211, 2, 7), 6)
    check_host(gpu, mats, 64, 7, witnesses(3212, 1, 7), 9)
    # log_n = 0: one row, and no row
    check_host(gpu, G.random_system(3220, 1, 7, terms=5), 1, 7, witnesses(3221, 3, 7), 0)
    check_host(gpu, ([], [], []), 0, 7, witnesses(3222, 2, 7), 0)
    check_host(gpu, ([], [], []), 0, 0, [[], []], 2)   # no columns: count=k says how many witnesses


def long_row(g, length, n_cols):
    return [(int(g.integers(0, n_cols)), v) for v in G.rand_fr(g, length)]


@pytest.mark.gpu
@pytest.mark.parametrize("where", ["first", "last", "alone", "mixed"])
def test_rows_around_the_chunk_length(gpu, where):
    """rows of 0, 1, L - 1, L, L + 1, 2 L + 1 and 64 L + 3 terms among one-term rows: one chunk, a full
    chunk, one term over, a fold over more partial sums than a wave has lanes; 300 columns, so the long rows
    repeat columns.  B has another sparsity, C is empty."""
    L = gpu.R1CS_CHUNK_LEN
    assert L == gpu._native._lib.pa_r1cs_chunk_len()
    g = rng(3300)
    n_cols = 300
    big = long_row(g, 64 * L + 3, n_cols)
    ones = lambda m: [long_row(g, 1, n_cols) for _ in range(m)]  # noqa: E731
    if where == "alone":
        a = [big]
    elif where == "first":
        a = [big] + ones(70)
    elif where == "last":
        a = ones(70) + [big]
    else:
        a = ones(3)
        for length in (0, 1, L - 1, L, L + 1, 2 * L + 1, 64 * L + 3, 0, 2 * L, 3 * L):
            a += [long_row(g, length, n_cols)] + ones(2)
    n_rows = len(a)
    b = [long_row(g, (7 * i) % (L + 2), n_cols) for i in range(n_rows)]
    c = [[] for _ in range(n_rows)]
    mats = (a, b, c)
    ws = witnesses(3301, 3, n_cols)
    check_host(gpu, mats, n_rows, n_cols, ws, log_for(n_rows))
    check_host(gpu, (c, a, b), n_rows, n_cols, ws[:1], log_for(n_rows) + 1)
    with gpu.r1cs(*(G.csr(m) for m in mats), n_rows, n_cols) as sysm:
        assert sysm.eval_workspace_bytes(1) > 0 and sysm.eval_workspace_bytes(3) == 3 * sysm.eval_workspace_bytes(1)


@pytest.mark.gpu
def test_repeated_columns_and_edge_values(gpu):
    e = [0, 1, R_ORDER - 1]
    # every pair of edge coefficient and edge witness value, a row that repeats one column five times, and a
    # row whose terms cancel
    a = [[(i, v)] for i in range(3) for v in e]
    a += [[(1, 5)] * 5, [(2, 1), (2, R_ORDER - 1)], [(0, R_ORDER - 1), (1, R_ORDER - 1), (2, R_ORDER - 1)]]
    b = [[(c, v) for c in range(3) for v in e]] + [[] for _ in range(len(a) - 1)]
    c = [[(2, R_ORDER - 1)] * 3 for _ in range(len(a))]
    ws = [e, [R_ORDER - 1] * 3, [0, 0, 0], [1, 1, 1]]
    check_host(gpu, (a, b, c), len(a), 3, ws, 4)


def _dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a).view(np.int64)).to("cuda:0")


def _host(t):
    return t.cpu().numpy().view(np.uint64)


@pytest.mark.gpu
def test_device_entry_on_a_stream_and_every_evaluation_error(gpu):
    import torch
    import pairing_amd.device as pdev
    from pairing_amd import _native
    L = gpu.R1CS_CHUNK_LEN
    g = rng(3400)
    n_cols, k, log_n = 40, 3, 4
    a = [long_row(g, t, n_cols) for t in (1, 2 * L + 1, 0, 1, L + 1, 3, 1, 1, 5 * L, 2, 1)]
    mats = (a, [long_row(g, 2, n_cols) for _ in a], [long_row(g, 1, n_cols) for _ in a])
    n_rows, n = len(a), 1 << log_n
    ws = witnesses(3401, k, n_cols)
    want = G.ref_eval(mats, ws, log_n)
    guard = np.full((2, 4), SENTINEL, np.uint64)
    s = torch.cuda.Stream()
    with gpu.r1cs(*(G.csr(m) for m in mats), n_rows, n_cols) as sysm:
        words = pdev.r1cs_eval_workspace_words(sysm, k)
        assert words * 8 == sysm.eval_workspace_bytes(k) == k * 32 * (3 + 2 + 5)   # the chunks of the three long rows
        work = torch.empty(words, dtype=torch.int64, device="cuda:0")              # exactly the queried size
        W = _dev(flat(ws))
        outs = [_dev(np.concatenate([np.full((k * n, 4), SENTINEL, np.uint64), guard])) for _ in range(3)]
        torch.cuda.synchronize()
        with torch.cuda.stream(s):
            pdev.r1cs_eval(sysm, W, log_n, *outs, workspace=work, stream=s)
        s.synchronize()
        for o, x, name in zip(outs, want, "abc"):
            np.testing.assert_array_equal(_host(o)[:k * n], x, err_msg=name)
            np.testing.assert_array_equal(_host(o)[k * n:], guard)     # rows past the batch are left alone
        np.testing.assert_array_equal(_host(W), flat(ws))              # the witness is only read
        with pytest.raises(ValueError, match="workspace"):
            pdev.r1cs_eval(sysm, W, log_n, *outs, stream=s)
        with pytest.raises(ValueError, match="workspace"):
            pdev.r1cs_eval(sysm, W, log_n, *outs, workspace=work[:-1], stream=s)

        # what the C entries refuse, each with its code and nothing written
        lib = _native._lib
        h = sysm.handle()
        fresh = [_dev(np.full((k * n, 4), SENTINEL, np.uint64)) for _ in range(3)]
        p = lambda t: ctypes.c_void_p(t.data_ptr())  # noqa: E731
        sp = ctypes.c_void_p(s.cuda_stream)
        o = [p(t) for t in fresh]
        wsb = words * 8
        cases = {
            "2^log_n < n_rows": (h, p(W), k, 3, *o, p(work), wsb, sp),
            "log_n over the maximum": (h, p(W), k, 29, *o, p(work), wsb, sp),
            "workspace one byte short": (h, p(W), k, log_n, *o, p(work), wsb - 1, sp),
            "no workspace": (h, p(W), k, log_n, *o, None, 0, sp),
            "no object": (None, p(W), k, log_n, *o, p(work), wsb, sp),
        }
        if torch.cuda.device_count() > 1:
            other = torch.cuda.Stream(device="cuda:1")
            cases["a stream on another device"] = (h, p(W), k, log_n, *o, p(work), wsb,
                                                   ctypes.c_void_p(other.cuda_stream))
        for what, args in cases.items():
            assert lib.pa_r1cs_eval_device(*args) == -1, what
            assert lib.pa_last_error(), what
        torch.cuda.synchronize()
        for t in fresh:
            assert (_host(t) == SENTINEL).all()
        host_out = [np.full((k * n, 4), SENTINEL, np.uint64) for _ in range(3)]
        w = flat(ws)
        for bad_log in (3, 29):
            assert lib.pa_r1cs_eval(h, _native.ptr(w), k, bad_log, *(_native.ptr(x) for x in host_out)) == -1
        assert all((x == SENTINEL).all() for x in host_out)
        with pytest.raises(ValueError):
            gpu.r1cs_eval(sysm, w, 3)
    with pytest.raises(ValueError, match="close"):
        gpu.r1cs_eval(sysm, w, log_n)
    # a coefficient that is not below r reaches the library through the numpy layer
    rp, col, val = G.csr(a)
    val[0] = [R_ORDER >> (64 * i) & (2**64 - 1) for i in range(4)]
    with pytest.raises(gpu.PairingError, match="coefficient"):
        gpu.r1cs((rp, col, val), G.csr(mats[1]), G.csr(mats[2]), n_rows, n_cols)
