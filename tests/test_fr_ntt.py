"""Batched Fr NTT over radix-2 evaluation domains (pa_fr_ntt*, include/pairing_amd.h).

The four transforms of a prover's evaluation domain (forward, inverse and their
coset forms, natural order in and out) are canonical Fr, so every check is
bit-exact.  The reference is built here from the oracle's Fr operations: the
rows bit-reversed, then per stage one vectorised fr_mul by the stage's twiddles
and one fr_add / fr_sub; the twiddles, g^(+-i) and n^-1 come from Python `pow`.
CPU: that reference against the O(n^2) big-integer definition, and the checks of
the Python layers that need no device.  GPU (-m gpu): every size, batch shape,
pass structure (PA_NTT_TILE_LOG), in-place and stream use, round trips, a
polynomial product and a replay from a captured graph."""
import ctypes
import os
import re

import numpy as np
import pytest

from helpers import R_ORDER, rng
from test_fr import FR_R, fr_mont, fr_val, random_fr, rows

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
HEADER = os.path.join(ROOT, "include", "pairing_amd.h")
MODES = ("forward", "inverse", "coset_forward", "coset_inverse")
GEN = 7                                          # GENERATOR, fr.rs:41-46
ROOT_OF_UNITY = pow(GEN, (R_ORDER - 1) >> 32, R_ORDER)   # fr.rs:51-56

NEW_SYMBOLS = ("pa_fr_ntt_domain_create", "pa_fr_ntt_domain_free", "pa_fr_ntt_domain_log_n", "pa_fr_ntt_domain_bytes",
               "pa_fr_ntt_domain_passes", "pa_fr_ntt_domain_tile_log", "pa_fr_ntt_polys_per_workgroup",
               "pa_fr_ntt_max_log_n", "pa_fr_ntt_workspace_bytes", "pa_fr_ntt", "pa_fr_ntt_device")


def omega(k):
    return pow(ROOT_OF_UNITY, 1 << (32 - k), R_ORDER)


def mont_rows(vals):
    return rows([v * FR_R % R_ORDER for v in vals])


_TABLES = {}


def _tables(k, inverse):
    """(w^i for i < max(n / 2, 1), g^(+-i) for i < n, n^-1) as Montgomery rows, w and g inverted for `inverse`"""
    if (k, inverse) not in _TABLES:
        n = 1 << k
        w, g = omega(k), GEN
        if inverse:
            w, g = pow(w, -1, R_ORDER), pow(g, -1, R_ORDER)
        wp, gp = [1], [1]
        for _ in range(max(n // 2, 1) - 1):
            wp.append(wp[-1] * w % R_ORDER)
        for _ in range(n - 1):
            gp.append(gp[-1] * g % R_ORDER)
        _TABLES[(k, inverse)] = (mont_rows(wp), mont_rows(gp), mont_rows([pow(n, -1, R_ORDER)]))
    return _TABLES[(k, inverse)]


def _bitrev(k):
    idx = np.arange(1 << k)
    out = np.zeros_like(idx)
    for b in range(k):
        out |= ((idx >> b) & 1) << (k - 1 - b)
    return out


def ref_ntt(oracle, a, k, mode):
    """the transform of each polynomial of `a` ((batch * n, 4) rows) from the oracle's fr_mul / fr_add / fr_sub"""
    n = 1 << k
    batch = a.shape[0] // n
    inverse = mode in ("inverse", "coset_inverse")
    wp, gp, ninv = _tables(k, inverse)
    x = np.ascontiguousarray(a, dtype=np.uint64)
    if batch == 0:
        return x.copy()
    if mode == "coset_forward":
        x = oracle.fr_mul(x, np.tile(gp, (batch, 1)))
    x = np.ascontiguousarray(x.reshape(batch, n, 4)[:, _bitrev(k)].reshape(-1, 4))
    for s in range(k):
        half = 1 << s
        v = x.reshape(-1, 2, half, 4)
        lo = np.ascontiguousarray(v[:, 0].reshape(-1, 4))
        hi = np.ascontiguousarray(v[:, 1].reshape(-1, 4))
        tw = np.ascontiguousarray(wp[::n // (2 * half)][:half])
        t = oracle.fr_mul(hi, np.tile(tw, (hi.shape[0] // half, 1)))
        x = np.stack([oracle.fr_add(lo, t).reshape(-1, half, 4), oracle.fr_sub(lo, t).reshape(-1, half, 4)],
                     axis=1).reshape(-1, 4)
    x = np.ascontiguousarray(x)
    if inverse:
        x = oracle.fr_mul(x, np.tile(ninv, (batch * n, 1)))
    if mode == "coset_inverse":
        x = oracle.fr_mul(x, np.tile(gp, (batch, 1)))
    return x


def big_int_ntt(vals, k, mode):
    """the definition, on Python integers"""
    n = 1 << k
    w = omega(k)
    x = list(vals)
    if mode == "coset_forward":
        x = [x[i] * pow(GEN, i, R_ORDER) % R_ORDER for i in range(n)]
    if mode in ("inverse", "coset_inverse"):
        w = pow(w, -1, R_ORDER)
    y = [sum(x[i] * pow(w, i * j, R_ORDER) for i in range(n)) % R_ORDER for j in range(n)]
    if mode in ("inverse", "coset_inverse"):
        y = [v * pow(n, -1, R_ORDER) % R_ORDER for v in y]
    if mode == "coset_inverse":
        y = [y[i] * pow(GEN, -i, R_ORDER) % R_ORDER for i in range(n)]
    return y


def edge_rows():
    """0, 1, r - 1 and R as values, and the largest canonical limb pattern"""
    return np.concatenate([mont_rows([0, 1, R_ORDER - 1, FR_R]), rows([R_ORDER - 1])])


def inputs(seed, nrows):
    """seeded random_fr rows with the edge rows mixed in where there is room"""
    a = random_fr(rng(seed), nrows)
    e = edge_rows()
    if nrows >= 4 * len(e):
        at = rng(seed + 1).choice(nrows, size=len(e), replace=False)
        a[at] = e
    elif nrows >= 1:
        a[0] = e[seed % len(e)]
    return a


# ---------------- CPU ----------------

@pytest.mark.parametrize("k", range(7))
def test_reference_transform_matches_big_integer_definition(oracle, k):
    n = 1 << k
    w = omega(k)
    assert pow(w, n, R_ORDER) == 1 and (k == 0 or pow(w, n // 2, R_ORDER) != 1)   # order exactly 2^k
    a = inputs(700 + k, n)
    vals = [fr_val(r) for r in a]
    for mode in MODES:
        got = ref_ntt(oracle, a, k, mode)
        assert [fr_val(r) for r in got] == big_int_ntt(vals, k, mode), mode
        assert (got == mont_rows([fr_val(r) for r in got])).all()   # canonical rows
    # the transforms invert exactly, batched
    b = inputs(710 + k, 3 * n)
    np.testing.assert_array_equal(ref_ntt(oracle, ref_ntt(oracle, b, k, "forward"), k, "inverse"), b)
    np.testing.assert_array_equal(ref_ntt(oracle, ref_ntt(oracle, b, k, "coset_forward"), k, "coset_inverse"), b)


def test_root_of_unity_is_the_oracles(oracle):
    """7^((r - 1) / 2^32): the constant both sides build their twiddles from (fr.rs:51-56)"""
    root = mont_rows([ROOT_OF_UNITY])
    np.testing.assert_array_equal(root, rows([0xb9b58d8c5f0e466a + (0x5b1b4c801819d7ec << 64) +
                                              (0x0af53ae352a31e64 << 128) + (0x5bf3adda19e9b27b << 192)]))
    x = root
    for _ in range(32):
        last = x
        x = oracle.fr_square(x)
    np.testing.assert_array_equal(x, mont_rows([1]))
    np.testing.assert_array_equal(last, mont_rows([R_ORDER - 1]))   # order exactly 2^32


def test_new_symbols_are_declared_and_bound():
    from pairing_amd import _native
    with open(HEADER) as f:
        src = f.read()
    declared = set(re.findall(r"^\s*(?:const\s+)?\w+\s*\*?\s*(pa_\w+)\s*\(", src, flags=re.M))
    for name in NEW_SYMBOLS:
        assert name in declared, name
        assert name in _native._SIGS, name
        assert getattr(_native._lib, name).argtypes == _native._SIGS[name]
    for name in ("pa_fr_ntt_domain_bytes", "pa_fr_ntt_workspace_bytes", "pa_fr_ntt_polys_per_workgroup"):
        assert getattr(_native._lib, name).restype is ctypes.c_size_t
    assert _native._lib.pa_fr_ntt_domain_free.restype is None
    assert _native._SIGS["pa_fr_ntt_device"][4] is ctypes.c_size_t
    for i, mode in enumerate(("PA_NTT_FORWARD", "PA_NTT_INVERSE", "PA_NTT_COSET_FORWARD", "PA_NTT_COSET_INVERSE")):
        assert re.search(r"#define %s %d\b" % (mode, i), src), mode
        assert _native.NTT_MODES[MODES[i]] == i
    import pairing_amd
    for name in ("FrNttDomain", "fr_ntt_domain", "fr_ntt"):
        assert name in pairing_amd.__all__ and hasattr(pairing_amd, name)


def borrowed(log_n, ws_per_poly=0):
    """a live-looking domain over a handle nobody may dereference (the checks
    under test come before any native call) and nobody frees; the one query
    that would read the handle, the workspace size, answers as a domain of
    ws_per_poly bytes per polynomial would"""
    from pairing_amd import FrNttDomain

    class Borrowed(FrNttDomain):
        def workspace_bytes(self, batch):
            self.handle()
            return ws_per_poly * int(batch)

    return Borrowed(ctypes.c_void_p(8), log_n, owns=False)


def test_python_layer_checks_need_no_device():
    import pairing_amd as pa
    d = borrowed(3)
    assert d.log_n == 3 and d.len == 8 and len(d) == 8 and not d.closed
    for bad_rows in (1, 7, 9, 12):
        with pytest.raises(ValueError, match="multiple"):
            pa.fr_ntt(d, np.zeros((bad_rows, 4), np.uint64))
    with pytest.raises(ValueError):
        pa.fr_ntt(d, np.zeros((8, 5), np.uint64))
    for bad_mode in ("backward", "", None, 0):
        with pytest.raises(ValueError, match="mode"):
            pa.fr_ntt(d, np.zeros((8, 4), np.uint64), mode=bad_mode)
    with pytest.raises(ValueError):
        pa.fr_ntt(object(), np.zeros((8, 4), np.uint64))
    # batch = 0: an empty array, no native call
    for mode in MODES:
        out = pa.fr_ntt(d, np.zeros((0, 4), np.uint64), mode=mode)
        assert out.shape == (0, 4) and out.dtype == np.uint64
    # log_n above the maximum: the Python layer and the C entry (before any device call)
    from pairing_amd import _native
    assert _native.NTT_MAX_LOG_N >= 24
    for bad in (_native.NTT_MAX_LOG_N + 1, 64, -1):
        with pytest.raises(ValueError, match="log_n"):
            pa.fr_ntt_domain(bad)
    h = ctypes.c_void_p(1)
    assert _native._lib.pa_fr_ntt_domain_create(_native.NTT_MAX_LOG_N + 1, ctypes.byref(h)) == -1
    assert not h.value
    assert _native._lib.pa_fr_ntt_domain_create(3, None) == -1
    # a NULL domain: a code from both entries, zero from the queries
    assert _native._lib.pa_fr_ntt(None, 0, None, None, 1) == -1
    assert _native._lib.pa_fr_ntt_device(None, 0, None, None, 1, None, 0, None) == -1
    assert _native._lib.pa_fr_ntt_workspace_bytes(None, 4) == 0 and _native._lib.pa_fr_ntt_domain_bytes(None) == 0
    _native._lib.pa_fr_ntt_domain_free(None)
    # a closed domain
    d.close()
    d.close()   # idempotent
    assert d.closed
    with pytest.raises(ValueError, match="close"):
        pa.fr_ntt(d, np.zeros((8, 4), np.uint64))
    with pytest.raises(ValueError, match="close"):
        d.handle()
    with pytest.raises(ValueError, match="close"):
        d.workspace_bytes(1)


def test_device_layer_rejects_undersized_buffers_without_device():
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
    one_pass, two_pass = borrowed(3), borrowed(4, ws_per_poly=16 * 32)
    assert pdev.fr_ntt_workspace_words(one_pass, 5) == 0
    assert pdev.fr_ntt_workspace_words(two_pass, 5) == 5 * 16 * 4
    with pytest.raises(ValueError, match="out"):
        pdev.fr_ntt(one_pass, f(16, 4), f(15, 4), "forward")
    with pytest.raises(ValueError, match="multiple"):
        pdev.fr_ntt(one_pass, f(12, 4), f(12, 4), "forward")
    with pytest.raises(ValueError, match="mode"):
        pdev.fr_ntt(one_pass, f(16, 4), f(16, 4), "fft")
    with pytest.raises(ValueError, match="workspace"):
        pdev.fr_ntt(two_pass, f(32, 4), f(32, 4), "inverse")
    with pytest.raises(ValueError, match="workspace"):
        pdev.fr_ntt(two_pass, f(32, 4), f(32, 4), "inverse", workspace=f(2 * 16 * 4 - 1))
    one_pass.close()
    with pytest.raises(ValueError, match="close"):
        pdev.fr_ntt(one_pass, f(16, 4), f(16, 4), "forward")
    with pytest.raises(ValueError, match="close"):
        pdev.fr_ntt_workspace_words(one_pass, 1)


def _rev(x, bits):
    return int(format(x, "0%db" % bits)[::-1], 2) if bits else 0


def _exchange_ways(t, cb, lo, width, reversed_rows, fin):
    """kernels_ntt.hip's LDS addressing restated: the most rows of one half wave (32 lanes, one
    register slot) that fall into one of the 32 banks of a word plane, for the round whose
    window is row bits [lo, lo + width) of a tile of 2^t rows x 2^cb columns"""
    length = t + cb
    worst, seen = 1, set()
    for g0 in range(0, (1 << length) >> width, 32):
        for m in range(1 << width):
            banks = {}
            for g in range(g0, min(g0 + 32, (1 << length) >> width)):
                c, gr = g & ((1 << cb) - 1), g >> cb
                rows = _rev(gr, t - width) if reversed_rows else gr
                x0 = ((rows >> lo) << (lo + width)) | (rows & ((1 << lo) - 1))
                p = ((x0 | (m << lo)) << cb) | c
                fold = _rev((x0 << cb) >> (length - (5 - cb)), 5 - cb) << cb if fin and cb < 5 else 0
                q = p ^ (p >> 3) ^ fold
                seen.add(q)
                banks.setdefault(q & 31, set()).add(q)
            worst = max(worst, max(len(s) for s in banks.values()))
    assert len(seen) == 1 << length and max(seen) < 1 << length   # the layout is a permutation of the rows
    return worst


def test_lds_exchanges_are_two_way_at_worst():
    """every exchange of every tile shape the launcher can produce: the write side of the round
    before and the read side of the round after, with the swizzle each uses (ntt_swz: the
    exchange into the bit-reversed last round of a one-launch transform has its own)"""
    def rounds(t):
        out, rem = [], t
        while rem:
            width = 2 if rem == 4 else min(rem, 3)
            out.append((rem - width, width))
            rem -= width
        return out

    worst = {}
    for group_log in (11, 12):
        for t in range(1, group_log + 1):
            for cb in range(0, group_log - t + 1):
                for one_launch in (False, True):
                    if one_launch and t + cb != group_log:
                        continue   # a one-launch transform always fills the workgroup
                    rs = rounds(t)
                    for i in range(len(rs) - 1):
                        final = one_launch and i == len(rs) - 2
                        w = _exchange_ways(t, cb, rs[i][0], rs[i][1], False, final)
                        r = _exchange_ways(t, cb, rs[i + 1][0], rs[i + 1][1], final, final)
                        assert w <= 2 and r <= 2, (t, cb, one_launch, i, w, r)
                        if rs[i][1] == 3 and rs[i + 1][1] == 3 and not final:
                            assert w == 1 and r == 1, (t, cb, i)   # three-bit windows: conflict-free
                        worst[(t, cb, one_launch)] = max(w, r, worst.get((t, cb, one_launch), 1))
    assert len(worst) > 50


CPP_SRC = os.path.join(ROOT, "tests", "cpp", "test_fr_ntt.cpp")
LIBDIR = os.path.join(ROOT, "pairing_amd", "lib")


def _compile_cpp(out):
    import subprocess
    cmd = ["g++", "-std=c++17", "-O1", "-Wall", "-Wextra", "-Werror", "-I" + os.path.join(ROOT, "include"), CPP_SRC,
           "-o", out, "-L" + LIBDIR, "-lpairing_amd", "-Wl,-rpath," + LIBDIR, "-Wl,-rpath-link,/opt/rocm/lib"]
    subprocess.run(cmd, check=True, capture_output=True, text=True, timeout=300)


def test_cpp_wrapper_compiles_and_links(tmp_path):
    out = str(tmp_path / "test_fr_ntt")
    _compile_cpp(out)
    assert os.path.getsize(out) > 0


# ---------------- GPU ----------------

@pytest.mark.gpu
def test_cpp_wrapper_on_gpu(oracle, tmp_path):
    """pairing_amd::FrNttDomain's fft / ifft / coset_fft / icoset_fft against the reference transform"""
    import subprocess
    k, batch = 7, 3
    a = inputs(1600, batch << k)
    data = str(tmp_path / "data.bin")
    with open(data, "wb") as f:
        f.write(np.array([k, batch], np.uint64).tobytes())
        f.write(a.tobytes())
        for mode in MODES:
            f.write(ref_ntt(oracle, a, k, mode).tobytes())
    exe = str(tmp_path / "test_fr_ntt")
    _compile_cpp(exe)
    r = subprocess.run([exe, data], capture_output=True, text=True, timeout=120)
    print(r.stdout, r.stderr)
    assert r.returncode == 0, r.stdout + r.stderr
    assert r.stdout.count("ok  ") == 10 and "FAIL" not in r.stdout


def _dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a).view(np.int64)).to("cuda:0")


def _host(t):
    return t.cpu().numpy().view(np.uint64)


def _workspace(pdev, d, batch):
    import torch
    words = pdev.fr_ntt_workspace_words(d, batch)
    return torch.empty(words, dtype=torch.int64, device="cuda:0") if words else None


@pytest.mark.gpu
@pytest.mark.parametrize("k", range(15))
def test_every_size_and_mode_matches_reference(gpu, oracle, k):
    a = inputs(800 + k, 1 << k)
    with gpu.fr_ntt_domain(k) as d:
        assert d.log_n == k and d.len == 1 << k and d.bytes > 0
        assert d.passes == (0 if k == 0 else -(-k // d.tile_log))
        for mode in MODES:
            np.testing.assert_array_equal(gpu.fr_ntt(d, a, mode), ref_ntt(oracle, a, k, mode), err_msg=mode)


@pytest.mark.gpu
def test_structured_inputs(gpu, oracle):
    k, n = 10, 1 << 10
    zero = np.zeros((n, 4), np.uint64)
    const = np.tile(mont_rows([0x1234567]), (n, 1))
    delta = zero.copy()
    delta[1] = mont_rows([1])[0]
    with gpu.fr_ntt_domain(k) as d:
        for mode in MODES:
            np.testing.assert_array_equal(gpu.fr_ntt(d, zero, mode), zero, err_msg=mode)
            for a in (const, delta):
                np.testing.assert_array_equal(gpu.fr_ntt(d, a, mode), ref_ntt(oracle, a, k, mode), err_msg=mode)
        # the forward transform of the delta at index 1 is the twiddle sequence itself
        w = omega(k)
        seq, x = [], 1
        for _ in range(n):
            seq.append(x)
            x = x * w % R_ORDER
        np.testing.assert_array_equal(gpu.fr_ntt(d, delta, "forward"), mont_rows(seq))


@pytest.mark.gpu
@pytest.mark.parametrize("k,batch", [(0, 5), (1, 3), (6, 7), (8, 33), (10, 3)])
def test_batched(gpu, oracle, k, batch):
    a = inputs(900 + 16 * k + batch, batch << k)
    with gpu.fr_ntt_domain(k) as d:
        for mode in MODES:
            np.testing.assert_array_equal(gpu.fr_ntt(d, a, mode), ref_ntt(oracle, a, k, mode), err_msg=mode)


@pytest.mark.gpu
def test_batches_at_the_workgroup_sharing_boundaries(gpu, oracle):
    """a one-pass domain puts pa_fr_ntt_polys_per_workgroup polynomials in a workgroup, a different
    number at every size: that many fill one workgroup exactly, one more starts the next"""
    seen = set()
    for k in range(0, 14):
        with gpu.fr_ntt_domain(k) as d:
            ppw = d.polys_per_workgroup
            if d.passes != 1:
                assert ppw == 0
                continue
            assert ppw >= 1 and ppw not in seen
            seen.add(ppw)
            for batch in (ppw, ppw + 1):
                a = inputs(1000 + 2 * k + (batch - ppw), batch << k)
                for mode in ("forward", "coset_inverse"):
                    np.testing.assert_array_equal(gpu.fr_ntt(d, a, mode), ref_ntt(oracle, a, k, mode),
                                                  err_msg="%d %d %s" % (k, batch, mode))
    assert len(seen) >= 2


@pytest.fixture(scope="module")
def pass_case(oracle):
    """one k = 12 and one k = 9 input, two polynomials each, with the reference's four transforms"""
    out = {}
    for k in (12, 9):
        a = inputs(1100 + k, 2 << k)
        out[k] = (a, {mode: ref_ntt(oracle, a, k, mode) for mode in MODES})
    return out


@pytest.mark.gpu
@pytest.mark.parametrize("k,tile,passes", [(12, 12, 1), (12, 6, 2), (12, 11, 2), (12, 5, 3), (12, 4, 3), (9, 4, 3),
                                           (9, 3, 3), (9, 1, 9), (12, 99, 1), (12, 0, 12)])
def test_pass_structure(gpu, pass_case, monkeypatch, k, tile, passes):
    a, want = pass_case[k]
    monkeypatch.delenv("PA_NTT_TILE_LOG", raising=False)
    with gpu.fr_ntt_domain(k) as d:
        default = {mode: gpu.fr_ntt(d, a, mode) for mode in MODES}
        assert d.tile_log == 10
    monkeypatch.setenv("PA_NTT_TILE_LOG", str(tile))
    with gpu.fr_ntt_domain(k) as d:
        assert d.passes == passes and 1 <= d.tile_log <= 12
        assert (d.workspace_bytes(2) == 0) == (passes == 1)
        for mode in MODES:
            got = gpu.fr_ntt(d, a, mode)
            np.testing.assert_array_equal(got, want[mode], err_msg=mode)
            np.testing.assert_array_equal(got, default[mode], err_msg=mode)


@pytest.mark.gpu
def test_tile_knob_that_is_no_number_leaves_the_default(gpu, monkeypatch):
    for bad in ("", "abc", "9x", " "):
        monkeypatch.setenv("PA_NTT_TILE_LOG", bad)
        with gpu.fr_ntt_domain(12) as d:
            assert d.tile_log == 10 and d.passes == 2, repr(bad)
            assert d.workspace_bytes(3) == 3 * 32 * 4096 and d.workspace_bytes(0) == 0
    monkeypatch.setenv("PA_NTT_TILE_LOG", " 6")   # strtol's own leading blanks
    with gpu.fr_ntt_domain(12) as d:
        assert d.tile_log == 6


@pytest.mark.gpu
@pytest.mark.parametrize("k", [9, 12])
def test_in_place_streams_and_untouched_rows(gpu, oracle, k):
    import torch
    import pairing_amd.device as pdev
    batch, n = 2, 1 << k
    a = inputs(1200 + k, batch * n)
    guard = np.full((3, 4), 0x5a5a5a5a5a5a5a5a, np.uint64)
    s = torch.cuda.Stream()
    with gpu.fr_ntt_domain(k) as d:
        ws = _workspace(pdev, d, batch)
        for mode in MODES:
            A = _dev(a)
            out = _dev(np.concatenate([np.zeros_like(a), guard]))
            inplace = _dev(np.concatenate([a, guard]))
            torch.cuda.synchronize()
            with torch.cuda.stream(s):
                pdev.fr_ntt(d, A, out, mode, workspace=ws, stream=s)
                # in == out, over the first batch * n rows of a longer tensor
                pdev.fr_ntt(d, inplace[:batch * n], inplace, mode, workspace=ws, stream=s)
            s.synchronize()
            want = ref_ntt(oracle, a, k, mode)
            np.testing.assert_array_equal(_host(A), a, err_msg=mode)               # the input is only read
            np.testing.assert_array_equal(_host(out)[:batch * n], want, err_msg=mode)
            np.testing.assert_array_equal(_host(out)[batch * n:], guard, err_msg=mode)   # rows past the end
            np.testing.assert_array_equal(_host(inplace)[:batch * n], want, err_msg=mode)
            np.testing.assert_array_equal(_host(inplace)[batch * n:], guard, err_msg=mode)
        # what the C entry refuses before a launch: partial overlap, a short workspace, an unknown mode
        from pairing_amd import _native
        A = _dev(a)
        big = _dev(np.concatenate([a, a]))
        sp = ctypes.c_void_p(s.cuda_stream)
        wsp = ctypes.c_void_p(ws.data_ptr() if ws is not None else 0)
        wsb = ws.numel() * 8 if ws is not None else 0
        dev = _native._lib.pa_fr_ntt_device
        assert dev(d.handle(), 0, ctypes.c_void_p(big.data_ptr()), ctypes.c_void_p(big.data_ptr() + 32), batch,
                   wsp, wsb, sp) == -1
        assert dev(d.handle(), 4, ctypes.c_void_p(A.data_ptr()), ctypes.c_void_p(A.data_ptr()), batch, wsp, wsb,
                   sp) == -1
        if wsb:
            assert dev(d.handle(), 0, ctypes.c_void_p(A.data_ptr()), ctypes.c_void_p(A.data_ptr()), batch, wsp,
                       wsb - 1, sp) == -1
        assert dev(d.handle(), 0, None, None, 0, None, 0, sp) == 0   # batch = 0: a no-op
        torch.cuda.synchronize()
        np.testing.assert_array_equal(_host(A), a)


@pytest.mark.gpu
def test_round_trip_at_2_16(gpu):
    k, batch = 16, 2
    a = inputs(1300, batch << k)
    with gpu.fr_ntt_domain(k) as d:
        f = gpu.fr_ntt(d, a, "forward")
        assert not np.array_equal(f, a)
        np.testing.assert_array_equal(gpu.fr_ntt(d, f, "inverse"), a)
        c = gpu.fr_ntt(d, a, "coset_forward")
        assert not np.array_equal(c, f)
        np.testing.assert_array_equal(gpu.fr_ntt(d, c, "coset_inverse"), a)


@pytest.mark.gpu
def test_polynomial_product_as_a_prover_would(gpu):
    k, n = 6, 64
    g = rng(1400)
    pa_, pb_ = ([int.from_bytes(g.bytes(32), "little") % R_ORDER for _ in range(32)] for _ in range(2))
    pa_[31] = R_ORDER - 1
    pb_[0] = 0
    prod = [0] * n
    for i, x in enumerate(pa_):
        for j, y in enumerate(pb_):
            prod[i + j] = (prod[i + j] + x * y) % R_ORDER
    a = mont_rows(pa_ + [0] * 32)
    b = mont_rows(pb_ + [0] * 32)
    with gpu.fr_ntt_domain(k) as d:
        ea, eb = gpu.fr_ntt(d, a, "forward"), gpu.fr_ntt(d, b, "forward")
        got = gpu.fr_ntt(d, gpu.fr_mul(ea, eb), "inverse")
        np.testing.assert_array_equal(got, mont_rows(prod))
        # and over the coset, as the quotient of a proof is computed
        ca, cb = gpu.fr_ntt(d, a, "coset_forward"), gpu.fr_ntt(d, b, "coset_forward")
        np.testing.assert_array_equal(gpu.fr_ntt(d, gpu.fr_mul(ca, cb), "coset_inverse"), mont_rows(prod))


@pytest.mark.gpu
def test_replays_from_a_graph(gpu, oracle):
    """one k = 10 forward transform captured on a side stream (tests/test_graph_capture.py's
    pattern; a single linear chain of launches) and replayed twice on fresh input"""
    import torch
    import pairing_amd.device as pdev
    k, n = 10, 1 << 10
    a0, a1, a2 = (inputs(1500 + i, n) for i in range(3))
    with gpu.fr_ntt_domain(k) as d:
        A = _dev(a0)
        out = pdev.empty_records(n, 4, "cuda:0")
        ws = _workspace(pdev, d, 1)
        s = torch.cuda.Stream()
        s.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(s):
            pdev.fr_ntt(d, A, out, "forward", workspace=ws)
        torch.cuda.synchronize()
        np.testing.assert_array_equal(_host(out), ref_ntt(oracle, a0, k, "forward"))
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g, stream=s, capture_error_mode="relaxed"):
            pdev.fr_ntt(d, A, out, "forward", workspace=ws)
        torch.cuda.synchronize()
        for fresh in (a1, a2):
            A.copy_(_dev(fresh))
            out.zero_()
            g.replay()
            torch.cuda.synchronize()
            np.testing.assert_array_equal(_host(out), ref_ntt(oracle, fresh, k, "forward"))
