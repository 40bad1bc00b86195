"""Device-resident entry points over torch tensors (HBM in, HBM out).

torch is plumbing here: it owns the device allocations and the stream; the
work is the C ABI's `_device` functions (HIP kernels) enqueued on that
stream.  Tensors hold the raw ABI records as int64 words (torch has no full
uint64 support), shape (n, words) exactly as the numpy layer.
"""
import ctypes

import torch

from ._native import W_FQ, W_FQ12, W_G1, W_G1A, W_G2, W_G2A, W_G2P, W_PROOF, FrNttDomain, G1MsmBases, G2MsmBases, Groth16Circuit, Groth16Pk, Groth16Vk, R1cs, _lib, call, csr_offsets, msm_bases, msm_scalars, ntt_mode, trapdoor_rows


def _stream_ptr(stream):
    s = stream if stream is not None else torch.cuda.current_stream()
    return ctypes.c_void_p(s.cuda_stream)


def _dptr(t, width, name):
    if not t.is_cuda or not t.is_contiguous() or t.dtype != torch.int64:
        raise ValueError("%s must be a contiguous int64 CUDA tensor" % name)
    if t.dim() != 2 or t.shape[1] != width:
        raise ValueError("%s must have shape (n, %d), got %s" % (name, width, tuple(t.shape)))
    return ctypes.c_void_p(t.data_ptr())


def _rows(t, n, name):
    """t holds at least the n records the call writes or reads"""
    if t.shape[0] < n:
        raise ValueError("%s has %d rows, the call needs %d" % (name, t.shape[0], n))


def _flags(ok, n, name="ok"):
    """a contiguous uint8 CUDA tensor of at least n flags, or None"""
    if ok is None:
        return ctypes.c_void_p(0)
    if not ok.is_cuda or not ok.is_contiguous() or ok.dtype != torch.uint8 or ok.numel() < n:
        raise ValueError("%s must be a contiguous uint8 CUDA tensor of >= %d elements" % (name, n))
    return ctypes.c_void_p(ok.data_ptr())


def _words(t, need, name):
    """a contiguous int64 CUDA buffer of at least `need` 8-byte words"""
    if not t.is_cuda or not t.is_contiguous() or t.dtype != torch.int64 or t.numel() < need:
        raise ValueError("%s must be a contiguous int64 CUDA tensor of >= %d words" % (name, need))
    return ctypes.c_void_p(t.data_ptr())


def _fb_table(table, ws):
    return (_words(table, int(_lib.pa_g1_fixed_base_table_words()), "table"),
            _words(ws, int(_lib.pa_g1_fixed_base_workspace_words()), "ws"))


def empty_records(n, width, device):
    return torch.empty((n, width), dtype=torch.int64, device=device)


def fq_mul(a, b, out, stream=None):
    """Fq::mul_assign over a batch resident in HBM (BASELINE config 2)."""
    n = a.shape[0]
    args = (_dptr(a, W_FQ, "a"), _dptr(b, W_FQ, "b"), _dptr(out, W_FQ, "out"))
    _rows(b, n, "b")
    _rows(out, n, "out")
    call("pa_fq_mul_batch_device", *args, n, _stream_ptr(stream))


def fq_mul_soa(a, b, out, stream=None):
    """Fq::mul_assign on the SoA device layout: (6, n) int64 planes, word j of
    element i at [j, i]."""
    for t, name in ((a, "a"), (b, "b"), (out, "out")):
        if not t.is_cuda or not t.is_contiguous() or t.dtype != torch.int64 or t.dim() != 2 or t.shape[0] != 6:
            raise ValueError("%s must be a contiguous (6, n) int64 CUDA tensor" % name)
    n = a.shape[1]
    if b.shape[1] != n or out.shape[1] != n:
        raise ValueError("operand lengths differ")
    call("pa_fq_mul_batch_soa_device", ctypes.c_void_p(a.data_ptr()), ctypes.c_void_p(b.data_ptr()),
         ctypes.c_void_p(out.data_ptr()), n, _stream_ptr(stream))


def miller_loop(p, q, out, stream=None):
    """Fused-prepare single-pair Miller loops: out[i] = miller_loop([(p[i], q[i].prepare())])."""
    n = p.shape[0]
    args = (_dptr(p, W_G1A, "p"), _dptr(q, W_G2A, "q"), _dptr(out, W_FQ12, "out"))
    _rows(q, n, "q")
    _rows(out, n, "out")
    call("pa_miller_loop_fused_batch_device", *args, n, _stream_ptr(stream))


def pairing_miller_loop(p, q, out, stream=None):
    """The Miller-loop stage of pairing(): final_exponentiation(out) = e(p[i], q[i]);
    out equals the reference's Miller values only up to Fq2 factors (see
    pa_pairing_miller_loop_batch_device)."""
    n = p.shape[0]
    args = (_dptr(p, W_G1A, "p"), _dptr(q, W_G2A, "q"), _dptr(out, W_FQ12, "out"))
    _rows(q, n, "q")
    _rows(out, n, "out")
    call("pa_pairing_miller_loop_batch_device", *args, n, _stream_ptr(stream))


def g2_prepare(q, out, stream=None):
    """G2Prepared::from_affine over a batch (mod.rs:168-358): out (n, W_G2P) int64 records."""
    n = q.shape[0]
    args = (_dptr(q, W_G2A, "q"), _dptr(out, W_G2P, "out"))
    _rows(out, n, "out")
    call("pa_g2_prepare_batch_device", *args, n, _stream_ptr(stream))


def miller_loop_prepared(p, qp, out, stream=None):
    """out[i] = miller_loop([(p[i], qp[i])]) over materialized G2Prepared records (mod.rs:40-102)."""
    n = p.shape[0]
    args = (_dptr(p, W_G1A, "p"), _dptr(qp, W_G2P, "qp"), _dptr(out, W_FQ12, "out"))
    _rows(qp, n, "qp")
    _rows(out, n, "out")
    call("pa_miller_loop_batch_device", *args, n, _stream_ptr(stream))


def miller_loop_shared_prepared(p, qp, out, stream=None):
    """out[i] = miller_loop([(p[i], qp[0])]): one G2Prepared record shared by the
    batch, its lines staged once (lib.rs:88-96, mod.rs:40-102)."""
    n = p.shape[0]
    args = (_dptr(p, W_G1A, "p"), _dptr(qp, W_G2P, "qp"), _dptr(out, W_FQ12, "out"))
    _rows(qp, 1, "qp")
    _rows(out, n, "out")
    call("pa_miller_loop_shared_prepared_device", args[0], n, args[1], args[2], _stream_ptr(stream))


def final_exponentiation(f, out, ok=None, stream=None):
    n = f.shape[0]
    args = (_dptr(f, W_FQ12, "f"), _dptr(out, W_FQ12, "out"), _flags(ok, n))
    _rows(out, n, "out")
    call("pa_final_exponentiation_batch_device", *args, n, _stream_ptr(stream))


def pairing(p, q, out, scratch, stream=None):
    """out[i] = e(p[i], q[i]) for a batch resident in HBM (BASELINE config 4)."""
    n = p.shape[0]
    args = (_dptr(p, W_G1A, "p"), _dptr(q, W_G2A, "q"), _dptr(out, W_FQ12, "out"), _dptr(scratch, W_FQ12, "scratch"))
    for t, name in ((q, "q"), (out, "out"), (scratch, "scratch")):
        _rows(t, n, name)
    call("pa_pairing_batch_device", *args, n, _stream_ptr(stream))


def multi_pairing(p, q, out, ok, work, stream=None):
    """final_exponentiation(miller_loop(pairs)) over pairs resident in HBM (the verifier's
    batch check, mod.rs:40-160): out (1, 72), ok (1,) uint8, work (n, 72) scratch."""
    n = p.shape[0]
    args = (_dptr(p, W_G1A, "p"), _dptr(q, W_G2A, "q"))
    _rows(q, n, "q")
    _rows(out, 1, "out")
    _rows(work, n, "work")   # the per-pair Miller values and the product tree
    call("pa_multi_pairing_device", *args, n, _dptr(out, W_FQ12, "out"), _flags(ok, 1),
         _dptr(work, W_FQ12, "work"), _stream_ptr(stream))


def multi_pairing_batch_workspace_words(n, m):
    """int64 words of `work` for multi_pairing_batch over n pairs in m products."""
    return (int(_lib.pa_multi_pairing_batch_workspace_bytes(int(n), int(m))) + 7) // 8


def multi_pairing_batch(p, q, offsets, out, ok, is_one, work, stream=None):
    """m independent multi_pairing products over pairs resident in HBM (a batch of
    signature or proof checks): product j covers pairs offsets[j] .. offsets[j+1].
    offsets: CSR, m + 1 entries from 0 to n, a CPU int64/uint64 tensor or numpy
    array (host metadata, staged by the call); out (m, 72), ok (m,) uint8, is_one
    (m,) uint8 or None (is_one[j] = ok[j] and out[j] == one), work an int64 buffer
    of multi_pairing_batch_workspace_words(n, m).  Sizes and offsets are checked
    before anything touches the device."""
    n = p.shape[0]
    o = csr_offsets(offsets, n)
    m = o.shape[0] - 1
    _rows(q, n, "q")
    _rows(out, m, "out")
    for t, name in ((ok, "ok"), (is_one, "is_one")):
        if t is not None and t.numel() < m:
            raise ValueError("%s has %d flags, the call needs %d" % (name, t.numel(), m))
    need = multi_pairing_batch_workspace_words(n, m)
    if work.numel() < need:
        raise ValueError("work has %d words, the call needs %d" % (work.numel(), need))
    if ok is None:
        raise ValueError("ok must be a contiguous uint8 CUDA tensor of >= %d elements" % m)
    args = (_dptr(p, W_G1A, "p"), _dptr(q, W_G2A, "q"), ctypes.c_void_p(o.ctypes.data), m,
            _dptr(out, W_FQ12, "out"), _flags(ok, m), _flags(is_one, m, "is_one"), _words(work, need, "work"))
    call("pa_multi_pairing_batch_device", *args, _stream_ptr(stream))


def g1_fixed_base_table(base, stream=None):
    """Build the fixed-base table for `base` (a (1,18) Jacobian record) in HBM."""
    dev = base.device
    table = torch.empty(int(_lib.pa_g1_fixed_base_table_words()), dtype=torch.int64, device=dev)
    ws = torch.empty(int(_lib.pa_g1_fixed_base_workspace_words()), dtype=torch.int64, device=dev)
    call("pa_g1_fixed_base_table_device", _dptr(base, W_G1, "base"), ctypes.c_void_p(table.data_ptr()),
         ctypes.c_void_p(ws.data_ptr()), _stream_ptr(stream))
    return table, ws


def g1_fixed_base_mul(table, scalars, out, stream=None):
    """out[i] = scalars[i] * base (config 3), scalars (n,4) int64 FrRepr."""
    n = scalars.shape[0]
    args = (_words(table, int(_lib.pa_g1_fixed_base_table_words()), "table"), _dptr(scalars, 4, "scalars"),
            _dptr(out, W_G1, "out"))
    _rows(out, n, "out")
    call("pa_g1_fixed_base_mul_device", *args, n, _stream_ptr(stream))


def g1_fixed_base_glv_table(base, table, ws, stream=None):
    """GLV stage 1: table rows, their phi images and the membership flag (ws)."""
    call("pa_g1_fixed_base_glv_table_device", _dptr(base, W_G1, "base"), *_fb_table(table, ws),
         _stream_ptr(stream))


def g1_fixed_base_glv_mul(base, table, ws, scalars, out, stream=None):
    """GLV stage 2: out[i] = scalars[i] * base (for a base outside G1 the
    double-and-add ladder k_g1_fixed_base_ladder takes over inside)."""
    n = scalars.shape[0]
    args = (_dptr(base, W_G1, "base"), *_fb_table(table, ws), _dptr(scalars, 4, "scalars"), _dptr(out, W_G1, "out"))
    _rows(out, n, "out")
    call("pa_g1_fixed_base_glv_mul_device", *args, n, _stream_ptr(stream))


def g1_wnaf_fixed_base(base, scalars, out, table, ws, stream=None, window=None):
    """out[i] = the reference's wNAF product scalars[i] * base (its wnaf_form
    wrap included; `window` default recommended_wnaf_for_num_scalars(n)) with
    the table built in the same call (its serial base chain overlapped with the
    multiply); table / ws as returned by fixed_base_buffers()."""
    n = scalars.shape[0]
    args = (_dptr(base, W_G1, "base"), _dptr(scalars, 4, "scalars"), _dptr(out, W_G1, "out"))
    _rows(out, n, "out")
    if window is None:
        call("pa_g1_wnaf_fixed_base_device", *args, n, *_fb_table(table, ws), _stream_ptr(stream))
    else:
        call("pa_g1_wnaf_fixed_base_window_device", *args, n, int(window), *_fb_table(table, ws),
             _stream_ptr(stream))


def fixed_base_buffers(dev):
    """(table, workspace) device buffers for g1_wnaf_fixed_base."""
    table = torch.empty(int(_lib.pa_g1_fixed_base_table_words()), dtype=torch.int64, device=dev)
    ws = torch.empty(int(_lib.pa_g1_fixed_base_workspace_words()), dtype=torch.int64, device=dev)
    return table, ws


def g1_batch_normalization(v, stream=None):
    call("pa_g1_batch_normalization_device", _dptr(v, W_G1, "v"), v.shape[0], _stream_ptr(stream))


def g2_batch_normalization(v, stream=None):
    call("pa_g2_batch_normalization_device", _dptr(v, W_G2, "v"), v.shape[0], _stream_ptr(stream))


def g2_fixed_base_buffers(dev):
    """(table, workspace) device buffers for g2_wnaf_fixed_base."""
    table = torch.empty(int(_lib.pa_g2_fixed_base_table_words()), dtype=torch.int64, device=dev)
    ws = torch.empty(int(_lib.pa_g2_fixed_base_workspace_words()), dtype=torch.int64, device=dev)
    return table, ws


def g2_wnaf_fixed_base(base, scalars, out, table, ws, stream=None, window=None):
    """out[i] = the reference's wNAF product scalars[i] * base for G2 (base a
    (1,36) Jacobian record; `window` as in g1_wnaf_fixed_base)."""
    n = scalars.shape[0]
    args = (_dptr(base, W_G2, "base"), _dptr(scalars, 4, "scalars"), _dptr(out, W_G2, "out"))
    _rows(out, n, "out")
    tw = (_words(table, int(_lib.pa_g2_fixed_base_table_words()), "table"),
          _words(ws, int(_lib.pa_g2_fixed_base_workspace_words()), "ws"))
    if window is None:
        call("pa_g2_wnaf_fixed_base_device", *args, n, *tw, _stream_ptr(stream))
    else:
        call("pa_g2_wnaf_fixed_base_window_device", *args, n, int(window), *tw, _stream_ptr(stream))


def group_add(group, a, b, out, stream=None):
    """CurveProjective::add_assign over Jacobian rows in HBM: out = a + b (group 1 or 2)."""
    w = W_G1 if group == 1 else W_G2
    args = (_dptr(a, w, "a"), _dptr(b, w, "b"), _dptr(out, w, "out"))
    _rows(b, a.shape[0], "b")
    _rows(out, a.shape[0], "out")
    call("pa_g%d_add_batch_device" % group, *args, a.shape[0], _stream_ptr(stream))


def subgroup_check(group, pts, ok, stream=None):
    """is_in_correct_subgroup_assuming_on_curve (ec.rs:142-144) over affine rows in HBM
    (n, 13|25) int64: ok (n,) uint8 = 1 in the subgroup (infinity included), 0 not."""
    n = pts.shape[0]
    args = (_dptr(pts, W_G1A if group == 1 else W_G2A, "pts"),)
    call("pa_g%d_subgroup_check_batch_device" % group, *args, n, _flags(ok, n), _stream_ptr(stream))


def decode(group, enc, compressed, checked, out, status, stream=None):
    """EncodedPoint::into_affine[_unchecked] over records resident in HBM:
    enc (n, 48|96|192) uint8, out (n, 13|25) int64 affine records, status (n,) uint8."""
    size = (48 if group == 1 else 96) * (1 if compressed else 2)
    if not enc.is_cuda or not enc.is_contiguous() or enc.dtype != torch.uint8 or enc.dim() != 2 \
            or enc.shape[1] != size:
        raise ValueError("enc must be a contiguous (n, %d) uint8 CUDA tensor" % size)
    if not status.is_cuda or status.dtype != torch.uint8 or status.numel() != enc.shape[0]:
        raise ValueError("status must be an (n,) uint8 CUDA tensor")
    width = W_G1A if group == 1 else W_G2A
    call("pa_g%d_decode_batch_device" % group, ctypes.c_void_p(enc.data_ptr()), enc.shape[0],
         int(bool(compressed)), int(bool(checked)), _dptr(out, width, "out"), ctypes.c_void_p(status.data_ptr()),
         _stream_ptr(stream))



def fr_mul(a, b, out, stream=None):
    """Fr::mul_assign (fr.rs:438-465) over a batch resident in HBM, rows (n, 4)."""
    args = (_dptr(a, 4, "a"), _dptr(b, 4, "b"), _dptr(out, 4, "out"))
    _rows(b, a.shape[0], "b")
    _rows(out, a.shape[0], "out")
    call("pa_fr_mul_batch_device", *args, a.shape[0], _stream_ptr(stream))


def fr_ntt_workspace_words(domain, batch):
    """int64 words of `workspace` for fr_ntt over `batch` polynomials (0 for a one-pass domain)."""
    return (domain.workspace_bytes(batch) + 7) // 8


def fr_ntt(domain, a, out, mode, workspace=None, stream=None):
    """The domain's transform of the batch * n Montgomery Fr rows of `a` into the same
    rows of `out` ((rows, 4) int64, natural order; out may be a itself, and rows of
    out past the batch are left alone).  mode "forward", "inverse", "coset_forward"
    or "coset_inverse"; workspace: an int64 buffer of fr_ntt_workspace_words(domain,
    batch), not needed where that is 0.  Nothing is allocated or read back."""
    if not isinstance(domain, FrNttDomain):
        raise ValueError("domain must come from fr_ntt_domain")
    domain.handle()   # a closed object is rejected first
    m = ntt_mode(mode)
    h, batch = domain.check_rows(a.shape[0])
    _rows(out, a.shape[0], "out")
    need = fr_ntt_workspace_words(domain, batch)
    if need and workspace is None:
        raise ValueError("workspace must be a contiguous int64 CUDA tensor of >= %d words" % need)
    ws = _words(workspace, need, "workspace") if need else ctypes.c_void_p(0)
    args = (_dptr(a, 4, "a"), _dptr(out, 4, "out"))
    call("pa_fr_ntt_device", h, m, *args, batch, ws, need * 8, _stream_ptr(stream))


def fr_ntt_quotient_workspace_words(domain, batch):
    """int64 words of `workspace` for fr_ntt_quotient over `batch` polynomial triples (0 for log_n = 0)."""
    return (domain.quotient_workspace_bytes(batch) + 7) // 8


def fr_ntt_quotient(domain, a, b, c, out, workspace=None, stream=None):
    """The quotient of a proof: from the evaluations a, b, c of each of batch polynomial
    triples ((rows, 4) int64 Montgomery Fr, laid out as fr_ntt's) the coefficients of
    h = (A B - C) / (X^n - 1) into the first batch * n rows of `out`, which may be a, b or
    c itself; the other inputs are only read and rows of out past the batch are left
    alone.  workspace: an int64 buffer of fr_ntt_quotient_workspace_words(domain, batch),
    not needed where that is 0.  Nothing is allocated or read back; `out` is what
    multiexp_prepared_batch(..., montgomery=True) takes."""
    if not isinstance(domain, FrNttDomain):
        raise ValueError("domain must come from fr_ntt_domain")
    domain.handle()   # a closed object is rejected first
    h, batch = domain.check_rows(a.shape[0])
    _rows(b, a.shape[0], "b")
    _rows(c, a.shape[0], "c")
    _rows(out, a.shape[0], "out")
    need = fr_ntt_quotient_workspace_words(domain, batch)
    if need and workspace is None:
        raise ValueError("workspace must be a contiguous int64 CUDA tensor of >= %d words" % need)
    ws = _words(workspace, need, "workspace") if need else ctypes.c_void_p(0)
    args = (_dptr(a, 4, "a"), _dptr(b, 4, "b"), _dptr(c, 4, "c"), _dptr(out, 4, "out"))
    call("pa_fr_ntt_quotient_device", h, *args, batch, ws, need * 8, _stream_ptr(stream))


def r1cs_eval_workspace_words(system, k):
    """int64 words of `workspace` for r1cs_eval over k witnesses (0 for a system without rows of several chunks)."""
    if not isinstance(system, R1cs):
        raise ValueError("system must come from r1cs()")
    return (system.eval_workspace_bytes(k) + 7) // 8


def r1cs_eval(system, witness, log_n, a, b, c, workspace=None, stream=None):
    """The products of the system's matrices with the k witnesses of `witness` ((k * cols, 4)
    int64 Montgomery Fr rows end to end) into the first k * 2^log_n rows of a, b and c
    ((rows, 4) int64, the layout fr_ntt_quotient takes); rows from the system's rows up to
    2^log_n are written as zero.  workspace: an int64 buffer of
    r1cs_eval_workspace_words(system, k), not needed where that is 0.  Nothing is
    allocated or read back."""
    if not isinstance(system, R1cs):
        raise ValueError("system must come from r1cs()")
    system.handle()   # a closed object is rejected first
    if system.cols == 0:
        raise ValueError("a system of no columns has no device witness: use the host entry")
    h, k, log_n = system.check_eval(witness.shape[0], None, log_n)
    for t, name in ((a, "a"), (b, "b"), (c, "c")):
        _rows(t, k << log_n, name)
    args = (_dptr(witness, 4, "witness"), k, log_n, _dptr(a, 4, "a"), _dptr(b, 4, "b"), _dptr(c, 4, "c"))
    need = r1cs_eval_workspace_words(system, k)
    if need and workspace is None:
        raise ValueError("workspace must be a contiguous int64 CUDA tensor of >= %d words" % need)
    ws = _words(workspace, need, "workspace") if need else ctypes.c_void_p(0)
    call("pa_r1cs_eval_device", h, *args, ws, need * 8, _stream_ptr(stream))


def groth16_prove_workspace(pk, system, k, device):
    """A device workspace sized for groth16_prove over k proofs.  A batch over a multiexp's
    32-bit item limit (include/pairing_amd.h) is a ValueError: split it."""
    if not isinstance(pk, Groth16Pk):
        raise ValueError("pk must come from groth16_pk")
    return torch.empty(pk.prove_workspace_bytes(system, k), dtype=torch.uint8, device=device)


def groth16_prove(pk, system, domain, witness, r, s, out, workspace, stream=None):
    """k Groth16 proofs into the first k rows of `out` ((rows, 51) int64: the affine records
    A, B, C of pa_groth16_proof): witness (k * n_vars, 4), r and s (k, 4) int64 Montgomery
    Fr rows in HBM, workspace from groth16_prove_workspace.  The evaluation, the quotient,
    the five multiexps and the assembly are enqueued on the stream; nothing is allocated,
    synchronized or read back."""
    if not isinstance(pk, Groth16Pk):
        raise ValueError("pk must come from groth16_pk")
    pk.handle()   # a closed object is rejected first
    (h, hr, hd), k = pk.check_prove(system, domain, witness.shape[0], r.shape[0], s.shape[0])
    _rows(out, k, "out")
    need = pk.prove_workspace_bytes(system, k)
    if not workspace.is_cuda or not workspace.is_contiguous() or workspace.dtype != torch.uint8 \
            or workspace.numel() < need:
        raise ValueError("workspace must be a contiguous uint8 CUDA tensor of >= %d bytes" % need)
    args = (_dptr(witness, 4, "witness"), _dptr(r, 4, "r"), _dptr(s, 4, "s"))
    call("pa_groth16_prove_device", h, hr, hd, *args, k, _dptr(out, W_PROOF, "out"),
         ctypes.c_void_p(workspace.data_ptr()), workspace.numel(), _stream_ptr(stream))


def groth16_generate_workspace(circuit, log_n, device):
    """A device workspace sized for groth16_generate and groth16_generate_scalars over a domain
    of 2^log_n points (pa_groth16_generate_workspace_bytes)."""
    if not isinstance(circuit, Groth16Circuit):
        raise ValueError("circuit must come from groth16_circuit")
    return torch.empty(circuit.generate_workspace_bytes(log_n), dtype=torch.uint8, device=device)


def _generate_args(circuit, domain, trapdoor, workspace):
    """(handles, log_n, trapdoor rows, workspace pointer, bytes) after the checks that need no device"""
    if not isinstance(circuit, Groth16Circuit):
        raise ValueError("circuit must come from groth16_circuit")
    (h, hd), log_n = circuit.check_generate(domain)
    if getattr(trapdoor, "is_cuda", False):
        raise ValueError("trapdoor must be host memory (a numpy array or a CPU tensor)")
    t = trapdoor_rows(trapdoor.numpy().view("uint64") if isinstance(trapdoor, torch.Tensor) else trapdoor)
    need = circuit.generate_workspace_bytes(log_n)
    if not workspace.is_cuda or not workspace.is_contiguous() or workspace.dtype != torch.uint8 \
            or workspace.numel() < need:
        raise ValueError("workspace must be a contiguous uint8 CUDA tensor of >= %d bytes" % need)
    return (h, hd), log_n, t, ctypes.c_void_p(workspace.data_ptr()), workspace.numel()


def groth16_generate(circuit, domain, g1, g2, trapdoor, g1_out, g2_out, workspace, stream=None):
    """bellman's generate_parameters for the given trapdoor into g1_out ((rows, 13) int64, the
    first 3 n_vars + 2^log_n + 2 rows: a_query | b_g1_query | ic | l_query | h_query | alpha_g1,
    beta_g1, delta_g1) and g2_out ((rows, 25), the first n_vars + 3: b_g2_query | beta_g2,
    gamma_g2, delta_g2), affine records.  g1 (1, 13) and g2 (1, 25) are the base points in HBM;
    trapdoor is host memory, (5, 4) Montgomery rows tau, alpha, beta, gamma, delta; workspace
    from groth16_generate_workspace.  Everything is enqueued on the stream; nothing is
    allocated, synchronized or read back."""
    (h, hd), log_n, t, ws, ws_bytes = _generate_args(circuit, domain, trapdoor, workspace)
    _rows(g1, 1, "g1")
    _rows(g2, 1, "g2")
    _rows(g1_out, circuit.g1_len(log_n), "g1_out")
    _rows(g2_out, circuit.g2_len(), "g2_out")
    call("pa_groth16_generate_device", h, hd, _dptr(g1, W_G1A, "g1"), _dptr(g2, W_G2A, "g2"),
         ctypes.c_void_p(t.ctypes.data), _dptr(g1_out, W_G1A, "g1_out"), _dptr(g2_out, W_G2A, "g2_out"), ws, ws_bytes,
         _stream_ptr(stream))


def groth16_generate_scalars(circuit, domain, trapdoor, out, workspace, stream=None):
    """The discrete logarithms of groth16_generate's G1 array, in its order, into the first
    3 n_vars + 2^log_n + 2 rows of `out` ((rows, 4) int64 Montgomery Fr rows)."""
    (h, hd), log_n, t, ws, ws_bytes = _generate_args(circuit, domain, trapdoor, workspace)
    _rows(out, circuit.g1_len(log_n), "out")
    call("pa_groth16_generate_scalars_device", h, hd, ctypes.c_void_p(t.ctypes.data), _dptr(out, 4, "out"), ws,
         ws_bytes, _stream_ptr(stream))


def groth16_verify_workspace(vk, k, device):
    """A device workspace sized for groth16_verify or groth16_verify_encoded over k proofs
    (pa_groth16_verify_workspace_bytes)."""
    if not isinstance(vk, Groth16Vk):
        raise ValueError("vk must come from groth16_vk")
    return torch.empty(vk.verify_workspace_bytes(k), dtype=torch.uint8, device=device)


def _verify_args(vk, k, inputs, stride, montgomery, valid, gt, workspace):
    """the arguments both verify entries share, after the checks that need no device"""
    if not isinstance(vk, Groth16Vk):
        raise ValueError("vk must come from groth16_vk")
    vk.handle()   # a closed object is rejected first
    flag = msm_scalars(montgomery)
    h, stride = vk.check_inputs(inputs.shape[0] if inputs is not None else 0, k, stride)
    if gt is not None:
        _rows(gt, k, "gt")
    if valid.numel() < k:
        raise ValueError("valid has %d elements, the call needs %d" % (valid.numel(), k))
    need = vk.verify_workspace_bytes(k)
    if not workspace.is_cuda or not workspace.is_contiguous() or workspace.dtype != torch.uint8 \
            or workspace.numel() < need:
        raise ValueError("workspace must be a contiguous uint8 CUDA tensor of >= %d bytes" % need)
    x = _dptr(inputs, 4, "inputs") if vk.n_inputs and k else ctypes.c_void_p(0)
    g = _dptr(gt, W_FQ12, "gt") if gt is not None else ctypes.c_void_p(0)
    return h, x, stride, flag, _flags(valid, k, "valid"), g, ctypes.c_void_p(workspace.data_ptr()), workspace.numel()


def groth16_verify(vk, proofs, inputs, valid, workspace, gt=None, stride=None, montgomery=True, stream=None):
    """k = proofs.shape[0] Groth16 proofs checked in HBM (pa_groth16_verify_device): proofs (k, 51)
    int64 as groth16_prove writes them; inputs (rows, 4) int64, row i of proof j at j * stride + i
    (stride None: n_inputs rows per proof; a view `witness[1:]` with stride = n_vars reads the
    prover's witness buffer as it lies), Montgomery Fr or (montgomery=False) FrRepr; valid (k,)
    uint8; gt None or (k, 72) int64; workspace from groth16_verify_workspace.  Everything is
    enqueued on the stream; nothing is allocated, synchronized or read back."""
    k = proofs.shape[0]
    h, x, stride, flag, v, g, ws, ws_bytes = _verify_args(vk, k, inputs, stride, montgomery, valid, gt, workspace)
    call("pa_groth16_verify_device", h, _dptr(proofs, W_PROOF, "proofs"), x, stride, flag, k, v, g, ws, ws_bytes,
         _stream_ptr(stream))


def groth16_verify_encoded(vk, data, inputs, valid, status, workspace, gt=None, stride=None, montgomery=True,
                           stream=None):
    """groth16_verify for k = data.shape[0] proofs off the wire (pa_groth16_verify_encoded_device):
    data (k, 192) uint8, A, B and C compressed; status (k, 3) uint8 gets the decoders' codes.  A
    proof with a nonzero status is not valid and its gt is meaningless."""
    if not data.is_cuda or not data.is_contiguous() or data.dtype != torch.uint8 or data.dim() != 2 \
            or data.shape[1] != 192:
        raise ValueError("data must be a contiguous (k, 192) uint8 CUDA tensor")
    k = data.shape[0]
    h, x, stride, flag, v, g, ws, ws_bytes = _verify_args(vk, k, inputs, stride, montgomery, valid, gt, workspace)
    call("pa_groth16_verify_encoded_device", h, ctypes.c_void_p(data.data_ptr()), x, stride, flag, k, v,
         _flags(status, 3 * k, "status"), g, ws, ws_bytes, _stream_ptr(stream))


def groth16_input_sum(vk, inputs, k, out, workspace=None, stride=None, montgomery=True, stream=None):
    """The public-input sums of k proofs into the first k rows of `out` ((rows, 13) int64 affine
    records; pa_groth16_vk_input_sum_device).  workspace: a uint8 buffer of
    vk.input_sum_workspace_bytes(k), not needed for a key without inputs."""
    if not isinstance(vk, Groth16Vk):
        raise ValueError("vk must come from groth16_vk")
    vk.handle()   # a closed object is rejected first
    flag = msm_scalars(montgomery)
    h, stride = vk.check_inputs(inputs.shape[0] if inputs is not None else 0, k, stride)
    _rows(out, k, "out")
    need = vk.input_sum_workspace_bytes(k)
    if need and (workspace is None or not workspace.is_cuda or not workspace.is_contiguous()
                 or workspace.dtype != torch.uint8 or workspace.numel() < need):
        raise ValueError("workspace must be a contiguous uint8 CUDA tensor of >= %d bytes" % need)
    x = _dptr(inputs, 4, "inputs") if vk.n_inputs and k else ctypes.c_void_p(0)
    call("pa_groth16_vk_input_sum_device", h, x, stride, flag, int(k), _dptr(out, W_G1A, "out"),
         ctypes.c_void_p(workspace.data_ptr()) if need else ctypes.c_void_p(0), need, _stream_ptr(stream))


def groth16_verify_aggregate_workspace(vk, k, device):
    """A device workspace sized for the three aggregate entries over k proofs
    (pa_groth16_verify_aggregate_workspace_bytes)."""
    if not isinstance(vk, Groth16Vk):
        raise ValueError("vk must come from groth16_vk")
    return torch.empty(vk.verify_aggregate_workspace_bytes(k), dtype=torch.uint8, device=device)


def _aggregate_args(vk, k, inputs, stride, montgomery, z, workspace):
    """the arguments the aggregate entries share, after the checks that need no device"""
    if not isinstance(vk, Groth16Vk):
        raise ValueError("vk must come from groth16_vk")
    vk.handle()   # a closed object is rejected first
    flag = msm_scalars(montgomery)
    h, stride = vk.check_inputs(inputs.shape[0] if inputs is not None else 0, k, stride)
    if z.dim() != 2 or tuple(z.shape) != (k, 2):
        raise ValueError("z must have shape (%d, 2): one 128-bit weight per proof, got %s" % (k, tuple(z.shape)))
    zp = _dptr(z, 2, "z")
    need = vk.verify_aggregate_workspace_bytes(k)
    if not workspace.is_cuda or not workspace.is_contiguous() or workspace.dtype != torch.uint8 \
            or workspace.numel() < need:
        raise ValueError("workspace must be a contiguous uint8 CUDA tensor of >= %d bytes" % need)
    x = _dptr(inputs, 4, "inputs") if vk.n_inputs and k else ctypes.c_void_p(0)
    return h, x, stride, flag, zp, ctypes.c_void_p(workspace.data_ptr()), workspace.numel()


def groth16_verify_aggregate(vk, proofs, inputs, z, valid, workspace, gt=None, stride=None, montgomery=True,
                             stream=None):
    """k = proofs.shape[0] Groth16 proofs checked in HBM by one randomised pairing product
    (pa_groth16_verify_aggregate_device): proofs and inputs as for groth16_verify; z (k, 2) int64,
    the 128-bit weights (little-endian words), which the caller draws from a cryptographic
    generator; valid: one uint8; gt None or (1, 72) int64; workspace from
    groth16_verify_aggregate_workspace.  Everything is enqueued on the stream.  One verdict for the
    batch: when it is 0, groth16_verify finds the bad proofs.  Up to 2^10 proofs groth16_verify is
    the faster call (5.6 ms against 7.5 at 2^10), at 2^14 and above this one is (10.2 against
    12.3; 19.6 against 29.1 at 2^16; README.md)."""
    k = proofs.shape[0]
    h, x, stride, flag, zp, ws, ws_bytes = _aggregate_args(vk, k, inputs, stride, montgomery, z, workspace)
    g = _dptr(gt, W_FQ12, "gt") if gt is not None else ctypes.c_void_p(0)
    if gt is not None:
        _rows(gt, 1, "gt")
    call("pa_groth16_verify_aggregate_device", h, _dptr(proofs, W_PROOF, "proofs"), x, stride, flag, zp, k,
         _flags(valid, 1, "valid"), g, ws, ws_bytes, _stream_ptr(stream))


def groth16_verify_aggregate_encoded(vk, data, inputs, z, valid, status, workspace, gt=None, stride=None,
                                     montgomery=True, stream=None):
    """groth16_verify_aggregate for k = data.shape[0] proofs off the wire
    (pa_groth16_verify_aggregate_encoded_device): data (k, 192) uint8; status (k, 3) uint8 gets the
    decoders' codes, and any nonzero one makes the batch not valid."""
    if not data.is_cuda or not data.is_contiguous() or data.dtype != torch.uint8 or data.dim() != 2 \
            or data.shape[1] != 192:
        raise ValueError("data must be a contiguous (k, 192) uint8 CUDA tensor")
    k = data.shape[0]
    h, x, stride, flag, zp, ws, ws_bytes = _aggregate_args(vk, k, inputs, stride, montgomery, z, workspace)
    g = _dptr(gt, W_FQ12, "gt") if gt is not None else ctypes.c_void_p(0)
    if gt is not None:
        _rows(gt, 1, "gt")
    call("pa_groth16_verify_aggregate_encoded_device", h, ctypes.c_void_p(data.data_ptr()), x, stride, flag, zp, k,
         _flags(valid, 1, "valid"), _flags(status, 3 * k, "status"), g, ws, ws_bytes, _stream_ptr(stream))


def groth16_aggregate_points(vk, proofs, inputs, z, out, workspace, stride=None, montgomery=True, stream=None):
    """The G1 side of the aggregate check into the first k + 3 rows of `out` ((rows, 13) int64 affine
    records: z_j A_j | the weighted input sum | sum_j z_j C_j | s_0 alpha;
    pa_groth16_verify_aggregate_points_device)."""
    k = proofs.shape[0]
    h, x, stride, flag, zp, ws, ws_bytes = _aggregate_args(vk, k, inputs, stride, montgomery, z, workspace)
    _rows(out, k + 3, "out")
    call("pa_groth16_verify_aggregate_points_device", h, _dptr(proofs, W_PROOF, "proofs"), x, stride, flag, zp, k,
         _dptr(out, W_G1A, "out"), ws, ws_bytes, _stream_ptr(stream))


def multiexp_u128_workspace(n, device):
    """A device workspace sized for multiexp_u128 over n terms (pa_g1_multiexp_u128_workspace_bytes)."""
    nbytes = int(_lib.pa_g1_multiexp_u128_workspace_bytes(int(n)))
    return torch.empty(max(nbytes, 1), dtype=torch.uint8, device=device)


def multiexp_u128(bases, scalars, out, workspace, stream=None):
    """out (1, 18) = sum_i scalars[i] * bases[i] over G1 affine records (n, 13) and 128-bit scalars
    (n, 2) int64, little-endian words (pa_g1_multiexp_u128_device)."""
    if scalars.shape[0] != bases.shape[0]:
        raise ValueError("bases and scalars differ in length: %d vs %d" % (bases.shape[0], scalars.shape[0]))
    call("pa_g1_multiexp_u128_device", _dptr(bases, W_G1A, "bases"), _dptr(scalars, 2, "scalars"), bases.shape[0],
         _dptr(out, W_G1, "out"), ctypes.c_void_p(workspace.data_ptr()), workspace.numel(), _stream_ptr(stream))


def multiexp_workspace(group, n, device):
    """A device workspace sized for pa_g{group}_multiexp_device over n terms."""
    nbytes = int(_lib.pa_multiexp_workspace_bytes(int(group), int(n)))
    return torch.empty(max(nbytes, 1), dtype=torch.uint8, device=device)


def multiexp(group, bases, scalars, out, workspace, stream=None):
    """out (1, 18|36) = sum_i scalars[i] * bases[i] (affine records (n, 13|25), FrRepr (n, 4))."""
    aw, jw = (W_G1A, W_G1) if group == 1 else (W_G2A, 36)
    call("pa_g%d_multiexp_device" % group, _dptr(bases, aw, "bases"), _dptr(scalars, 4, "scalars"),
         bases.shape[0], _dptr(out, jw, "out"), ctypes.c_void_p(workspace.data_ptr()), workspace.numel(),
         _stream_ptr(stream))


# the prepared entries of both groups: (handle class, affine width, Jacobian width, the preparing function)
_MSM_GROUPS = {1: (G1MsmBases, W_G1A, W_G1, "msm_prepare"), 2: (G2MsmBases, W_G2A, W_G2, "g2_msm_prepare")}


def _msm_prepare(group, bases, stream):
    cls, aw, _, _ = _MSM_GROUPS[group]
    n = bases.shape[0]
    h = ctypes.c_void_p(0)
    call("pa_g%d_msm_bases_prepare_device" % group, _dptr(bases, aw, "bases"), n, _stream_ptr(stream),
         ctypes.byref(h))
    return cls._adopt(h)


def _msm_handle(group, prepared, m):
    """the handle of this group's live object, after checking that m terms fit"""
    cls, _, _, maker = _MSM_GROUPS[group]
    return msm_bases(prepared, cls, maker).check_terms(m)


def _multiexp_prepared_workspace(group, prepared, m, device):
    m = int(m)
    h = _msm_handle(group, prepared, m)
    nbytes = int(getattr(_lib, "pa_g%d_multiexp_prepared_workspace_bytes" % group)(h, m))
    return torch.empty(max(nbytes, 1), dtype=torch.uint8, device=device)


def _multiexp_prepared(group, prepared, scalars, out, workspace, stream):
    m = scalars.shape[0]
    h = _msm_handle(group, prepared, m)
    _rows(out, 1, "out")
    call("pa_g%d_multiexp_prepared_device" % group, h, _dptr(scalars, 4, "scalars"), m,
         _dptr(out, _MSM_GROUPS[group][2], "out"), ctypes.c_void_p(workspace.data_ptr()), workspace.numel(),
         _stream_ptr(stream))


def _multiexp_prepared_batch_workspace(group, prepared, m, k, device):
    m, k = int(m), int(k)
    if k < 0:
        raise ValueError("k must not be negative, got %d" % k)
    h = _msm_handle(group, prepared, m)
    nbytes = int(getattr(_lib, "pa_g%d_multiexp_prepared_batch_workspace_bytes" % group)(h, m, k))
    if nbytes == 0 and m and k:
        raise ValueError("a batch of %d vectors of %d terms is over the 32-bit item limit: split it" % (k, m))
    return torch.empty(max(nbytes, 1), dtype=torch.uint8, device=device)


def _multiexp_prepared_batch(group, prepared, scalars, m, k, out, workspace, montgomery, stream):
    m, k = int(m), int(k)
    cls, _, _, maker = _MSM_GROUPS[group]
    msm_bases(prepared, cls, maker)
    flags = msm_scalars(montgomery)
    h = prepared.check_terms(m)
    if k < 0:
        raise ValueError("k must not be negative, got %d" % k)
    _rows(scalars, k * m, "scalars")
    _rows(out, k, "out")
    call("pa_g%d_multiexp_prepared_batch_device" % group, h, _dptr(scalars, 4, "scalars"), m, k, flags,
         _dptr(out, _MSM_GROUPS[group][2], "out"), ctypes.c_void_p(workspace.data_ptr()), workspace.numel(),
         _stream_ptr(stream))


def msm_prepare(bases, stream=None):
    """Prepare G1 multiexp bases resident in HBM ((n, 13) affine records) once:
    the membership check and the conversion the plain multiexp repeats per call.
    Synchronizes the stream.  Returns a G1MsmBases (len, in_subgroup, close())
    tied to the tensor's device; `bases` may be released afterwards."""
    return _msm_prepare(1, bases, stream)


def multiexp_prepared_workspace(prepared, m, device):
    """A device workspace sized for multiexp_prepared over the first m prepared bases."""
    return _multiexp_prepared_workspace(1, prepared, m, device)


def multiexp_prepared(prepared, scalars, out, workspace, stream=None):
    """out (1, 18) = sum_i scalars[i] * P_i over the first m = len(scalars) prepared
    bases (FrRepr (m, 4)), equal as a point to multiexp(1, ...) over the same bases."""
    _multiexp_prepared(1, prepared, scalars, out, workspace, stream)


def multiexp_prepared_batch_workspace(prepared, m, k, device):
    """A device workspace sized for multiexp_prepared_batch: k vectors over the first m
    prepared bases.  A batch over the 32-bit item limit (include/pairing_amd.h) is a
    ValueError: split it."""
    return _multiexp_prepared_batch_workspace(1, prepared, m, k, device)


def multiexp_prepared_batch(prepared, scalars, m, k, out, workspace, montgomery=False, stream=None):
    """out[j] (k, 18) = sum_i scalars[j * m + i] * P_i over the first m prepared bases:
    k vectors end to end in `scalars` ((k * m, 4); FrRepr rows, or with montgomery=True
    the Montgomery Fr rows fr_ntt writes), each equal as a point to multiexp_prepared
    over that vector.  Nothing is allocated or read back."""
    _multiexp_prepared_batch(1, prepared, scalars, m, k, out, workspace, montgomery, stream)


def g2_msm_prepare(bases, stream=None):
    """msm_prepare for G2 bases ((n, 25) affine records): returns a G2MsmBases.  The G1
    and G2 functions take only their own group's object (ValueError otherwise)."""
    return _msm_prepare(2, bases, stream)


def g2_multiexp_prepared_workspace(prepared, m, device):
    """A device workspace sized for g2_multiexp_prepared over the first m prepared bases."""
    return _multiexp_prepared_workspace(2, prepared, m, device)


def g2_multiexp_prepared(prepared, scalars, out, workspace, stream=None):
    """out (1, 36) = sum_i scalars[i] * Q_i over the first m = len(scalars) prepared G2
    bases (FrRepr (m, 4)), equal as a point to multiexp(2, ...) over the same bases."""
    _multiexp_prepared(2, prepared, scalars, out, workspace, stream)


def g2_multiexp_prepared_batch_workspace(prepared, m, k, device):
    """multiexp_prepared_batch_workspace for prepared G2 bases."""
    return _multiexp_prepared_batch_workspace(2, prepared, m, k, device)


def g2_multiexp_prepared_batch(prepared, scalars, m, k, out, workspace, montgomery=False, stream=None):
    """multiexp_prepared_batch over prepared G2 bases: out (k, 36)."""
    _multiexp_prepared_batch(2, prepared, scalars, m, k, out, workspace, montgomery, stream)


def wnaf_exact_workspace(group, n, window, fixed_scalar, device):
    """A device workspace for the bit-exact Wnaf device entries (window as resolved)."""
    nbytes = int(_lib.pa_wnaf_exact_workspace_bytes(int(group), int(n), int(window), int(bool(fixed_scalar))))
    if nbytes == 0:
        raise ValueError("wnaf exact: group %r / window %r out of range" % (group, window))
    return torch.empty(nbytes, dtype=torch.uint8, device=device)


def wnaf_fixed_base_exact(group, base, scalars, out, window, workspace, stream=None):
    """Wnaf::new().base(base, n).scalar(s_i) with the reference's Jacobian words
    (pa_g{1,2}_wnaf_fixed_base_exact_device); base (1, 18|36), scalars (n, 4)."""
    jw = W_G1 if group == 1 else W_G2
    n = scalars.shape[0]
    _rows(out, n, "out")
    _rows(base, 1, "base")
    if base.shape[0] != 1:
        raise ValueError("base: expected exactly one record, got %d" % base.shape[0])
    call("pa_g%d_wnaf_fixed_base_exact_device" % group, _dptr(base, jw, "base"), _dptr(scalars, 4, "scalars"),
         _dptr(out, jw, "out"), n, int(window), ctypes.c_void_p(workspace.data_ptr()), workspace.numel(),
         _stream_ptr(stream))


def wnaf_fixed_scalar_exact(group, bases, scalar, out, window, workspace, stream=None):
    """Wnaf::new().scalar(s).base(g_i) with the reference's Jacobian words
    (pa_g{1,2}_wnaf_fixed_scalar_exact_device); bases (n, 18|36), scalar (1, 4)."""
    jw = W_G1 if group == 1 else W_G2
    n = bases.shape[0]
    _rows(out, n, "out")
    _rows(scalar, 1, "scalar")
    if scalar.shape[0] != 1:
        raise ValueError("scalar: expected exactly one record, got %d" % scalar.shape[0])
    call("pa_g%d_wnaf_fixed_scalar_exact_device" % group, _dptr(bases, jw, "bases"), n,
         _dptr(scalar, 4, "scalar"), _dptr(out, jw, "out"), int(window), ctypes.c_void_p(workspace.data_ptr()),
         workspace.numel(), _stream_ptr(stream))
