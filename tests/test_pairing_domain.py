"""The e(P, Q) entries on their whole domain: Engine::pairing (lib.rs:101-109)
and miller_loop (mod.rs:40-102) take any field elements -- points outside the
prime-order subgroups, of small order, and values that are no curve point at
all (into_affine_unchecked, ec.rs:686-740, 1333-1395) -- and every entry here
must return the reference's value for them at every batch size, whichever
kernels serve the batch (tests/pairing_domain_cases.py lists the cases).

CPU: the big-integer model (tests/ml_ref.py) pins the oracle on every case;
the generated programs' DSL equals the oracle; the pairing-only programs
(kernels.doubling_step_h uses the curve constant) are followed along the
library's route (capi.hip pairing_gen_launch: the curve test, then the
reference form for a Q off E').

GPU (-m gpu): every e(P, Q) entry and every Miller-loop entry on every kernel
family, the sizes at which the default selection changes kernels, the fix-up
kernel on its own, the decode -> pairing flow and a captured graph.

What the reference computes at the degenerate Qs, as the oracle and the model
both give it:
  * Q of order 13: R = 12 Q = -Q at the loop's second addition step, R + Q is
    infinity (z = 0), and the Miller value is 0 for every P: pairing = None.
  * Q of order 23: R never meets +-Q or infinity before the last doubling;
    the Miller value is non-zero and the pairing an ordinary Fq12 value.
  * Q = (0, y) off E' behaves as a point of order 3 on y^2 = x^3 + y_Q^2
    (R = 2 Q = -Q at the first addition step) and Q = (x, 0) as one of order 2
    (2 Q is infinity at the first doubling): Miller value 0, pairing None.
  * no order dividing #E'(Fq2) gives R = +Q at an addition step
    (pairing_domain_cases.points asserts it).
The pairing-only programs give 0 exactly where the reference does, and the
reference's pairing on every other case with Q on E'; on the cases with Q off
E' and a non-zero value they differ -- the defect the fix-up closes.
"""
import ctypes
import os
import sys

import numpy as np
import pytest

import decode_cases as D
import ml_ref
import pairing_domain_cases as C
import pymodel as pm
from helpers import random_scalars, rng, unmont

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for _p in (os.path.join(ROOT, "tools", "pgen"), os.path.join(ROOT, "tools")):
    if _p not in sys.path:
        sys.path.insert(0, _p)

FAMILIES = [0, 1, 2, 3, 4, 5]       # pa_set_pairing_kernel: default, lane pairs, coop, one lane, one-wave VM, lane groups


def _threads():
    try:
        n = len(os.sched_getaffinity(0))
    except AttributeError:
        n = os.cpu_count() or 1
    return max(1, min(n, int(os.environ.get("OMP_NUM_THREADS", "16")), 16))


def _words(a, k):
    return sum(int(w) << (64 * i) for i, w in enumerate(a[6 * k:6 * k + 6]))


def _row(vals):
    from helpers import limbs
    return np.array([limbs(vals[k]) for k in range(12)], np.uint64).reshape(-1)


def _reference(oracle, p, q):
    """(prepared, miller, pairing, ok) of the oracle for each pair; pairing rows
    are zero where ok = 0 (None)"""
    prep = oracle.g2_prepare(q, _threads())
    ml = oracle.miller_loop_batch(p, prep, _threads())
    fe, ok = oracle.final_exponentiation(ml, _threads())
    return prep, ml, fe, np.asarray(ok, np.uint8)


@pytest.fixture(scope="module")
def ref(oracle):
    labels, p, q = C.arrays()
    prep, ml, fe, ok = _reference(oracle, p, q)
    for a in (p, q, prep, ml, fe, ok):
        a.setflags(write=False)
    return {"labels": labels, "p": p, "q": q, "prep": prep, "ml": ml, "fe": fe, "ok": ok}


# ======================= CPU: the model pins the oracle =======================
def test_case_list_covers_the_domain():
    labels, p, q = C.arrays()
    assert 35 <= len(labels) <= 45 and p.shape == (len(labels), 13) and q.shape == (len(labels), 25)
    assert sum(C.q_off_curve(x) for x in labels) >= 8
    assert sum(C.q_degenerate(x) for x in labels) >= 4
    assert sum(C.has_infinity(x) for x in labels) >= 5


def test_model_pins_oracle_prepare_and_miller_loop(oracle, ref):
    """oracle.g2_prepare and oracle.miller_loop_batch equal the big-integer
    model bit for bit on every domain case and on two random subgroup pairs"""
    g = rng(95)
    p = np.concatenate([ref["p"], oracle.g1_mul_generator(random_scalars(g, 2))])
    q = np.concatenate([ref["q"], oracle.g2_mul_generator(random_scalars(g, 2))])
    prep, ml, _, _ = _reference(oracle, p, q)
    bad = []
    for i in range(p.shape[0]):
        pt, qt = C.as_points(p[i], q[i])
        co = ml_ref.g2_prepare(qt)
        if not np.array_equal(ml_ref.prepared_record(co), prep[i]):
            bad.append(("prepare", i))
        if not np.array_equal(ml_ref.fq12_record(ml_ref.miller_loop(pt, co)), ml[i]):
            bad.append(("miller_loop", i))
    assert not bad, [(w, (ref["labels"] + ["random", "random"])[i]) for w, i in bad]


def test_model_pins_oracle_final_exponentiation_on_the_domain_values(oracle, ref):
    """the final exponentiation takes any Fq12: the domain cases' Miller values
    (the zero ones included: None) against f^(3 (q^12 - 1) / r) in the model"""
    seen = {}
    for i, label in enumerate(ref["labels"]):
        key = ref["ml"][i].tobytes()
        if key in seen:
            continue
        seen[key] = label
        want = ml_ref.final_exponentiation(pm.fq12_from_limbs(ref["ml"][i]))
        if want is None:
            assert ref["ok"][i] == 0 and not ref["fe"][i].any(), label
        else:
            assert ref["ok"][i] == 1 and np.array_equal(ml_ref.fq12_record(want), ref["fe"][i]), label
    assert any(not ref["ml"][i].any() for i in range(len(ref["labels"])))
    # Engine::pairing is the composition (lib.rs:101-109)
    np.testing.assert_array_equal(oracle.pairing(ref["p"], ref["q"], _threads()), ref["fe"])


def test_zero_miller_values_only_at_degenerate_q(ref):
    """the cap on what a pairing comparison may treat apart: only cases whose
    reference Miller value is 0, no more of them than the list has small-order
    / R = +-Q cases, each of them one of those, and ok = 1 everywhere else"""
    labels, ok = ref["labels"], ref["ok"]
    zero = [i for i in range(len(labels)) if not ref["ml"][i].any()]
    assert [i for i in range(len(labels)) if ok[i] == 0] == zero
    assert 0 < len(zero) <= sum(C.q_degenerate(x) for x in labels)
    assert all(C.q_degenerate(labels[i]) for i in zero)
    assert all(ok[i] == 1 for i in range(len(labels)) if i not in zero)


# ======================= CPU: the generated programs =======================
def _pgen():
    import build_gen  # noqa: F401
    import dsl
    import kernels
    import tower2
    return dsl, kernels, tower2


def _ins(p_rec, q_rec):
    ins = {k: _words(p_rec, k) for k in range(2)}
    ins.update({2 + k: _words(q_rec, k) for k in range(4)})
    return ins


def _coeff_ints(rec):
    return [[_words(rec, 6 * line + j) for j in range(6)] for line in range(68)]


@pytest.mark.parametrize("which", ["one_lane", "lane_pairs", "lazy", "prepared", "shared_prepared"])
def test_dsl_reference_form_miller_loops_on_the_domain(ref, which):
    """miller_loop_prog on one lane, on lane pairs and lazy, and the prepared and
    shared-prepared programs equal the oracle's Miller value on every
    non-infinity case (infinity is the kernels' lane select, outside the DSL)"""
    dsl, kernels, _ = _pgen()
    prog = {"one_lane": lambda: kernels.miller_loop_prog(lanes=1),
            "lane_pairs": lambda: kernels.miller_loop_prog(lanes=2),
            "lazy": lambda: kernels.miller_loop_prog(lanes=1, lazy=True),
            "prepared": kernels.miller_loop_prepared_prog,
            "shared_prepared": kernels.miller_loop_shared_prog}[which]()
    bad, ran = [], 0
    for i, label in enumerate(ref["labels"]):
        if C.has_infinity(label):
            continue
        ins = _ins(ref["p"][i], ref["q"][i])
        if which == "prepared":
            ins = {0: ins[0], 1: ins[1], "lines": kernels.prepared_table_lines(_coeff_ints(ref["prep"][i]))}
        elif which == "shared_prepared":
            ins = {0: ins[0], 1: ins[1], "lines": kernels.shared_table_lines(_coeff_ints(ref["prep"][i]))}
        got = dsl.evaluate(prog, ins)
        ran += 1
        if not np.array_equal(_row(got), ref["ml"][i]):
            bad.append(label)
    assert not bad and ran == sum(not C.has_infinity(x) for x in ref["labels"])


_fe_cache = {}


def _dsl_final_exp(dsl, kernels, f):
    """final_exp_prog on the 12 ABI integers f, or None for f == 0 (the
    kernels' zero select, as the reference's None)"""
    key = tuple(f)
    if key not in _fe_cache:
        if not any(key):
            _fe_cache[key] = None
        else:
            out = dsl.evaluate(kernels.final_exp_prog(), {k: key[k] for k in range(12)})
            _fe_cache[key] = [out[k] for k in range(12)]
    return _fe_cache[key]


def _q_on_curve(q_rec):
    """the fix-up's test (pairing_fl.h g2_on_curve_fl): y^2 == x^3 + 4 (1 + u)
    on canonical values"""
    x = (unmont(q_rec[0:6]), unmont(q_rec[6:12]))
    y = (unmont(q_rec[12:18]), unmont(q_rec[18:24]))
    return D.f2mul(y, y) == D.rhs2(x)


@pytest.mark.parametrize("lanes", [1, 2])
def test_dsl_pairing_only_route_gives_the_pairing_on_the_domain(ref, lanes):
    """the library's route for e(P, Q) above PA_PQ_MAX pairs (capi.hip
    pairing_gen_launch): the pairing-only program (pa_gen_miller_loop1p / 2p),
    then the fix-up -- a Q off E' has its value replaced by the reference-form
    Miller value (ml_ref is its specification; the GPU test of the fix-up
    kernel pins the kernel to it) -- then final_exp_prog.  Equal to
    oracle.pairing on every case whose reference Miller value is non-zero; 0
    and None where it is 0.  The pairing-only value alone misses the reference
    on the off-curve Qs with a non-zero value: the defect the fix-up closes."""
    dsl, kernels, tower2 = _pgen()
    if lanes == 1:
        prog = kernels.miller_loop_prog(pairing_only=True)
    else:
        prog = tower2.two_pass(lambda: kernels.miller_loop_prog(lanes=2, pairing_only=True), xi_dpp=False)()
    labels = ref["labels"]
    bad, compared, zero, replaced, shown_defect = [], 0, 0, 0, False
    for i, label in enumerate(labels):
        if C.has_infinity(label):
            continue
        got = dsl.evaluate(prog, _ins(ref["p"][i], ref["q"][i]))
        f = [got[k] for k in range(12)]
        if not _q_on_curve(ref["q"][i]):
            assert C.q_off_curve(label)
            if ref["ml"][i].any():
                assert not np.array_equal(_row(f), ref["ml"][i]), label
                if not shown_defect:     # one final exponentiation shows that it does not reconcile them
                    assert not np.array_equal(_row(_dsl_final_exp(dsl, kernels, f)), ref["fe"][i]), label
                    shown_defect = True
            pt, qt = C.as_points(ref["p"][i], ref["q"][i])
            f = [_words(ml_ref.fq12_record(ml_ref.miller_loop(pt, ml_ref.g2_prepare(qt))), k) for k in range(12)]
            replaced += 1
        if not ref["ml"][i].any():
            zero += 1
            if any(f) or _dsl_final_exp(dsl, kernels, f) is not None or ref["ok"][i] != 0:
                bad.append(label)
            continue
        compared += 1
        assert ref["ok"][i] == 1
        out = _dsl_final_exp(dsl, kernels, f)
        if out is None or not np.array_equal(_row(out), ref["fe"][i]):
            bad.append(label)
    assert not bad
    assert shown_defect and replaced == sum(C.q_off_curve(x) for x in labels)
    assert zero <= sum(C.q_degenerate(x) for x in labels)
    assert compared + zero == sum(not C.has_infinity(x) for x in labels)


# ======================= GPU =======================
def _dev(a):
    import torch
    return torch.from_numpy(np.array(a, dtype=np.uint64, order="C").view(np.int64)).to("cuda:0")   # a copy: fixtures are read-only


def _host(t):
    return t.cpu().numpy().view(np.uint64)


@pytest.fixture
def family(gpu, request):
    gpu.set_pairing_kernel(request.param)
    yield request.param
    gpu.set_pairing_kernel(0)


_by_family = pytest.mark.parametrize("family", FAMILIES, indirect=True)

N = 130                                         # two full waves and a ragged one
WAVE_FIRST = (0, 32, 64, 96, 128)               # first pair of a wave: lane pairs (32 a wave) and one lane (64)
WAVE_LAST = (31, 63, 95, 127, 129)
LIVE_OFF_Q = ("off_random", "off_random2", "y+1", "y-1", "other_b")   # off E' with a non-zero value


def _domain_batch():
    """the n = 130 batch: subgroup filler pairs (bench.make_pairs, an infinity P
    among them), every off-curve Q kind with a non-zero value once as the first
    pair of a wave (even index) and once as the last (odd), x = 0 and y = 0
    once on an even and once on an odd index, and every domain case in between"""
    import bench
    p, q = bench.make_pairs(N, 0, seed=61)
    pts = C.points()
    for k, kind in enumerate(LIVE_OFF_Q):
        for idx in (WAVE_FIRST[k], WAVE_LAST[(k + 2) % 5]):
            q[idx] = D.aff_record(2, pts["q"][kind])
            p[idx] = D.aff_record(1, pts["p"]["subgroup" if idx % 2 else "subgroup2"])
    labels, cp, cq = C.arrays()
    free = [i for i in range(1, N) if i not in WAVE_FIRST and i not in WAVE_LAST]
    where = free[:len(labels)]
    p[where], q[where] = cp, cq
    for idx, kind in zip(free[len(labels):len(labels) + 4], ("x=0", "x=0", "y=0", "y=0")):
        q[idx] = D.aff_record(2, pts["q"][kind])
    off = [i for i in range(N) if not (int(p[i, 12]) & 0xff or int(q[i, 24]) & 0xff) and not _q_on_curve(q[i])]
    return p, q, off


@pytest.fixture(scope="module")
def batch(oracle):
    p, q, off = _domain_batch()
    assert {i % 2 for i in off} == {0, 1} and set(WAVE_FIRST) <= set(off) and set(WAVE_LAST) <= set(off)
    prep, ml, fe, ok = _reference(oracle, p, q)
    assert ok[list(WAVE_FIRST + WAVE_LAST)].all() and not ok.all()
    for a in (p, q, prep, ml, fe, ok):
        a.setflags(write=False)
    return {"p": p, "q": q, "prep": prep, "ml": ml, "fe": fe, "ok": ok, "off": off}


def _assert_rows(got, want, what):
    diff = np.nonzero((got != want).any(axis=1))[0]
    assert diff.size == 0, "%s: %d rows differ from the oracle: %s" % (what, diff.size, diff.tolist()[:40])


@pytest.mark.gpu
@_by_family
def test_pairing_host_and_device_on_the_domain(gpu, batch, family):
    """pa_pairing_batch and pa_pairing_batch_device: the oracle's pairing bit
    for bit, zero rows where it is None"""
    import torch
    import pairing_amd.device as pdev
    _assert_rows(gpu.pairing(batch["p"], batch["q"]), batch["fe"], "pairing")
    out = pdev.empty_records(N, 72, "cuda:0")
    scratch = pdev.empty_records(N, 72, "cuda:0")
    pdev.pairing(_dev(batch["p"]), _dev(batch["q"]), out, scratch)
    torch.cuda.synchronize()
    _assert_rows(_host(out), batch["fe"], "device.pairing")


@pytest.mark.gpu
@_by_family
def test_pairing_stages_on_the_domain(gpu, batch, family):
    """pa_pairing_miller_loop_batch_device, then the final exponentiation: values and ok"""
    import torch
    import pairing_amd.device as pdev
    f = pdev.empty_records(N, 72, "cuda:0")
    pdev.pairing_miller_loop(_dev(batch["p"]), _dev(batch["q"]), f)
    out = pdev.empty_records(N, 72, "cuda:0")
    ok = torch.zeros(N, dtype=torch.uint8, device="cuda:0")
    pdev.final_exponentiation(f, out, ok)
    torch.cuda.synchronize()
    np.testing.assert_array_equal(ok.cpu().numpy(), batch["ok"])
    _assert_rows(_host(out), batch["fe"], "stages")
    # a pair off E' holds the reference's own Miller value whichever kernels ran
    _assert_rows(_host(f)[batch["off"]], batch["ml"][batch["off"]], "stage values off the curve")


def _product(oracle, p, prep, idx):
    f = oracle.miller_loop(np.ascontiguousarray(p[idx]), np.ascontiguousarray(prep[idx]))
    fe, ok = oracle.final_exponentiation(f[None, :].copy())
    return fe[0], bool(ok[0])


@pytest.mark.gpu
@_by_family
def test_multi_pairing_with_an_off_curve_pair(gpu, oracle, batch, family):
    """pa_multi_pairing over products that hold one pair off E' (and one that
    holds a zero Miller value: ok = 0)"""
    zero = int(np.nonzero(batch["ok"] == 0)[0][0])
    for idx in ([1, WAVE_FIRST[1], 2], [WAVE_LAST[0]], list(range(60, 70)), [3, zero, WAVE_FIRST[2]]):
        got, ok = gpu.multi_pairing(batch["p"][idx], batch["q"][idx])
        want, want_ok = _product(oracle, batch["p"], batch["prep"], idx)
        assert ok == want_ok and np.array_equal(np.asarray(got).reshape(-1), want), idx


@pytest.mark.gpu
@_by_family
@pytest.mark.parametrize("k", [2, 3])
def test_multi_pairing_batch_with_domain_cases(gpu, oracle, batch, family, k):
    """pa_multi_pairing_batch: m = 20 products of k pairs over the head of the
    batch, which holds wave-edge off-curve pairs and the domain cases"""
    m = 20
    p, q = batch["p"][:m * k], batch["q"][:m * k]
    assert any(i < m * k for i in batch["off"]) and not batch["ok"][:m * k].all()
    out, ok, is_one = gpu.multi_pairing_batch(p, q, pairs_per_product=k)
    want = [_product(oracle, batch["p"], batch["prep"], list(range(j * k, j * k + k))) for j in range(m)]
    np.testing.assert_array_equal(ok, np.array([w[1] for w in want]))
    _assert_rows(out, np.stack([w[0] for w in want]), "multi_pairing_batch k=%d" % k)
    assert not is_one[~ok].any()


@pytest.mark.gpu
@_by_family
def test_miller_loop_entries_on_the_domain(gpu, batch, family):
    """the reference-form entries: the fused Miller loop, g2_prepare, the Miller
    loop over prepared records and over one shared prepared record, bit for bit"""
    import torch
    import pairing_amd.device as pdev
    p, q = _dev(batch["p"]), _dev(batch["q"])
    f = pdev.empty_records(N, 72, "cuda:0")
    pdev.miller_loop(p, q, f)
    prep = pdev.empty_records(N, 2449, "cuda:0")
    pdev.g2_prepare(q, prep)
    g = pdev.empty_records(N, 72, "cuda:0")
    pdev.miller_loop_prepared(p, prep, g)
    torch.cuda.synchronize()
    _assert_rows(_host(f), batch["ml"], "device.miller_loop")
    _assert_rows(_host(prep), batch["prep"], "g2_prepare")
    _assert_rows(_host(g), batch["ml"], "miller_loop_prepared")
    _assert_rows(gpu.g2_prepare(batch["q"]), batch["prep"], "host g2_prepare")
    _assert_rows(gpu.miller_loop_batch(batch["p"], batch["prep"]), batch["ml"], "host miller_loop_batch")


@pytest.mark.gpu
@_by_family
def test_shared_prepared_on_the_domain(gpu, oracle, batch, family):
    """one prepared Q off E', one of order 13 and one with torsion, each shared by every P of the batch"""
    labels, _, cq = C.arrays()
    for label in ("P subgroup x Q off_random", "P subgroup x Q order13", "P subgroup x Q subgroup+torsion"):
        one = oracle.g2_prepare(cq[labels.index(label)][None, :].copy())
        want = oracle.miller_loop_batch(batch["p"], np.repeat(one, N, axis=0), _threads())
        _assert_rows(gpu.miller_loop_shared_prepared(batch["p"], one), want, "shared " + label)


def _big_batch(n, at, seed):
    import bench
    p, q = bench.make_pairs(n, 0, seed=seed)
    pts = C.points()
    for k, idx in enumerate(at):
        q[idx] = D.aff_record(2, pts["q"][LIVE_OFF_Q[k % len(LIVE_OFF_Q)]])
        p[idx] = D.aff_record(1, pts["p"]["subgroup"])
    return p, q


def _device_pairing(p, q):
    import torch
    import pairing_amd.device as pdev
    n = p.shape[0]
    out = pdev.empty_records(n, 72, "cuda:0")
    scratch = pdev.empty_records(n, 72, "cuda:0")
    pdev.pairing(_dev(p), _dev(q), out, scratch)
    torch.cuda.synchronize()
    return _host(out)


@pytest.mark.gpu
def test_default_selection_first_size_on_the_pairing_only_kernels(gpu, oracle):
    """PA_PQ_MAX + 1 pairs: the first size the default selection gives to the
    pairing-only kernels; Qs off E' at the first, the middle and the last index"""
    n = int(os.environ.get("PA_PQ_MAX", "4096")) + 1
    p, q = _big_batch(n, (0, n // 2, n - 1), seed=62)
    _assert_rows(_device_pairing(p, q), oracle.pairing(p, q, _threads()), "n = %d" % n)
    _assert_rows(gpu.pairing(p, q), oracle.pairing(p, q, _threads()), "host, n = %d" % n)


@pytest.mark.gpu
def test_split_head_and_tail_with_off_curve_pairs(gpu, oracle):
    """PA_PAIR_MAX + 1 pairs: the head on lane pairs (pairing-only), the tail on
    a forked stream; Qs off E' at the head's first and last index and in the
    tail.  Those rows and 64 sampled ones against the oracle."""
    head = int(os.environ.get("PA_PAIR_MAX", "32768"))
    n = head + 1
    at = (0, head - 1, head)
    p, q = _big_batch(n, at, seed=63)
    rows = np.array(sorted(set(at) | set(np.random.default_rng(64).choice(n, 64, replace=False).tolist())))
    want = oracle.pairing(np.ascontiguousarray(p[rows]), np.ascontiguousarray(q[rows]), _threads())
    _assert_rows(_device_pairing(p, q)[rows], want, "n = %d rows %s" % (n, rows.tolist()))


@pytest.mark.gpu
@pytest.mark.parametrize("variant", [0, 1, 3])
def test_unchecked_decode_then_pairing(gpu, oracle, variant):
    """the verifier's flow: g2_decode(compressed = 0, checked = 0) hands on an
    off-curve point, and pairing of it equals oracle.decode -> oracle.pairing"""
    pts = C.points()
    qs = [pts["q"][k] for k in ("off_random", "subgroup", "y+1", "other_b", "curve")]
    enc = np.frombuffer(b"".join(D.enc_g2(x, y, False) for x, y in qs), np.uint8).reshape(-1, 192).copy()
    got_q, st = gpu.g2_decode(enc, False, checked=False)
    want_q, want_st = oracle.decode(2, enc, False, checked=False)
    assert not st.any() and not want_st.any()
    np.testing.assert_array_equal(got_q, want_q)
    p = np.array([D.aff_record(1, pts["p"]["subgroup"])] * len(qs), np.uint64)
    gpu.set_pairing_kernel(variant)
    try:
        got = gpu.pairing(p, got_q)
    finally:
        gpu.set_pairing_kernel(0)
    _assert_rows(got, oracle.pairing(p, want_q), "decode -> pairing")


@pytest.mark.gpu
def test_fixup_kernel_on_its_own(gpu, oracle, ref):
    """pairing_fl.h g2_on_curve_fl and pairing_ml_fixup_lane (the body of
    k_pairing_ml_fixup) against Python: the curve test decides exactly on
    curve points in non-trivial form, y +- 1, x = 0, y = 0, whatever the
    infinity words say; the fix-up overwrites exactly the pairs with Q off E'
    and no infinity side, with the oracle's Miller value, and leaves the rest"""
    import torch
    import hipmod
    co = os.path.join(hipmod.TEST_LIB, "pairing_fixup_unit.hsaco")
    p, q, labels = ref["p"], ref["q"], ref["labels"]
    n = len(labels)
    on = np.array([_q_on_curve(q[i]) for i in range(n)], np.uint8)
    assert on.any() and not on.all()
    dq, dp = _dev(q), _dev(p)
    flags = torch.full((n,), 7, dtype=torch.uint8, device="cuda:0")
    hipmod.launch_kernel(co, "pairing_fixup_unit_on_curve",
                         [(ctypes.c_uint64, dq.data_ptr()), (ctypes.c_uint64, flags.data_ptr()),
                          (ctypes.c_uint32, n)], (n + 63) // 64, 64)
    np.testing.assert_array_equal(flags.cpu().numpy(), on)
    sentinel = np.full((n, 72), 0x5a5a5a5a5a5a5a5a, np.uint64)
    out = _dev(sentinel)
    wrote = torch.full((n,), 7, dtype=torch.uint8, device="cuda:0")
    hipmod.launch_kernel(co, "pairing_fixup_unit_run",
                         [(ctypes.c_uint64, dp.data_ptr()), (ctypes.c_uint64, dq.data_ptr()),
                          (ctypes.c_uint64, out.data_ptr()), (ctypes.c_uint64, wrote.data_ptr()),
                          (ctypes.c_uint32, n)], (n + 63) // 64, 64)
    want_wrote = np.array([C.q_off_curve(x) for x in labels], np.uint8)
    assert want_wrote.sum() >= 8
    np.testing.assert_array_equal(wrote.cpu().numpy(), want_wrote)
    want = np.where(want_wrote[:, None] == 1, ref["ml"], sentinel)
    _assert_rows(_host(out), want, "fix-up")


@pytest.mark.gpu
def test_off_curve_pair_through_a_captured_graph(gpu, oracle):
    """pa_pairing_batch_device on the pairing-only kernels, captured and
    replayed on new inputs with a Q off E' (tests/test_graph_capture.py): the
    fix-up is one more stream-ordered launch, no host synchronisation"""
    import torch
    import pairing_amd.device as pdev
    n = int(os.environ.get("PA_PQ_MAX", "4096")) + 1
    p1, q1 = _big_batch(n, (), seed=65)
    p2, q2 = _big_batch(n, (0, 77, n - 1), seed=66)
    P, Qd = _dev(p1), _dev(q1)
    out = pdev.empty_records(n, 72, "cuda:0")
    scratch = pdev.empty_records(n, 72, "cuda:0")
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        pdev.pairing(P, Qd, out, scratch)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=s, capture_error_mode="relaxed"):
        pdev.pairing(P, Qd, out, scratch)
    torch.cuda.synchronize()
    P.copy_(_dev(p2))
    Qd.copy_(_dev(q2))
    out.zero_()
    g.replay()
    torch.cuda.synchronize()
    _assert_rows(_host(out), oracle.pairing(p2, q2, _threads()), "graph replay")
