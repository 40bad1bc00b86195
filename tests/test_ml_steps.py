"""CPU tests of the Miller loop's pieces as unit programs
(tools/pgen/unit_progs.ml_step_prog): the G2 doubling and addition steps in
reference and homogeneous form, ell with its packed P broadcast, sqr12,
mul12, and three trips of the loop itself on miller_loop_prog's variables and
homes -- each as the lane-pair program the build makes (build_gen.PROGRAMS,
pairing_amd/lib/test/), against its one-lane twin and a plain big-integer
reference (tests/ml_step_ref.py), on the records of tests/ml_step_cases.py.

What each level reaches:

  * the DSL model (dsl.evaluate) checks the mathematics of the lane-pair
    tower and EVERY DECLARED BOUND (limb and value bounds of every
    operation), on the edge records and, through `raw`, on state at the
    variables' value bound -- which no load can produce; it knows nothing of
    registers, exchanges' encodings or storage slots;
  * the simulator runs the EMITTED instructions of both lanes in lockstep
    and compares every operation's registers with the model's trace: carries,
    selects, DPP exchanges, LDS / workspace homes, and in "iter" the second
    and third trips on the state the first left in those homes; inputs are
    loads, so values are canonical on entry;
  * the GPU (tests/test_ml_steps_gpu.py) runs the same code objects on about
    a thousand records per launch: what the assembler, the hardware's DPP and
    LDS behaviour and whole waves add to the simulator's one pair.
"""
import functools
import os
import random
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (os.path.join(ROOT, "tools", "pgen"), os.path.join(ROOT, "tools")):
    if p not in sys.path:
        sys.path.insert(0, p)

import build_gen  # noqa: E402
import dsl  # noqa: E402
import kcfg  # noqa: E402
import sim_check  # noqa: E402
import unit_progs  # noqa: E402

import ml_step_cases as cases  # noqa: E402
import ml_step_ref as ref  # noqa: E402
from test_pgen_lazy2 import STATE_VB, _edge_limbs, _raw  # noqa: E402

# object (build_gen.PROGRAMS key, pairing_amd/lib/test/pa_gen_<key>.hsaco) ->
# (which, lanes, pairing_only, workspace slots per wave).  The GPU tests size
# the workspace from the last column; test_workspace_slots holds it to the build.
OBJECTS = {
    "tml2_dbl": ("dbl", 2, False, 1),
    "tml2_dblh": ("dbl", 2, True, 1),
    "tml2_add": ("add", 2, False, 1),
    "tml2_addh": ("add", 2, True, 1),
    "tml2_ell": ("ell", 2, False, 1),
    "tml2_sqr12": ("sqr12", 2, False, 1),
    "tml2_mul12": ("mul12", 2, False, 1),
    "tml2_iter": ("iter", 2, False, 7),
    "tml2_iterh": ("iter", 2, True, 7),
    "tml1_iterh": ("iter", 1, True, 5),
}
PAIR_OBJECTS = [k for k, v in OBJECTS.items() if v[1] == 2]
STEP_OBJECTS = [k for k in PAIR_OBJECTS if OBJECTS[k][0] != "iter"]
ITER_OBJECTS = [k for k in PAIR_OBJECTS if OBJECTS[k][0] == "iter"]
NRAND = 8


def built(key):
    """the program exactly as the build makes it, and its workspace slot count"""
    prog, _, _, nmem = build_gen.PROGRAMS[key]()
    return prog, nmem


@functools.lru_cache(maxsize=None)
def one_lane(which, pairing_only):
    prog = unit_progs.ml_step_prog(which, lanes=1, pairing_only=pairing_only)
    dsl.check_scopes(prog)
    return prog


def run(prog, rec, stats=None, trace=None):
    out = dsl.evaluate(prog, {k: rec[k] for k in range(12)}, stats, trace)
    return [out[k] for k in range(12)]


def all_cases():
    return cases.structured() + [("random %d" % i, r) for i, r in enumerate(cases.random_records(31, NRAND))]


def iter_setvars(taken):
    """setvar operations of the lane-pair "iter" program with `taken` addition
    steps: 12 to take the state from the record, 9 per line (R and f), 6 per sqr12"""
    return 12 + 9 * (unit_progs.ITER_TRIPS + 1 + taken) + 6 * unit_progs.ITER_TRIPS


def test_objects_are_registered():
    assert set(OBJECTS) == set(build_gen.ML_STEP_OBJS)
    for key, (which, lanes, h, _) in OBJECTS.items():
        assert build_gen.ML_STEP_OBJS[key] == (which, lanes, h)
        assert build_gen.FILES[key] == "test/pa_gen_%s.hsaco" % key
    with open(os.path.join(ROOT, "pairing_amd", "Makefile")) as f:
        mk = f.read().replace("\\\n", " ")
    keys = next(line for line in mk.splitlines() if line.startswith("GEN_TEST_KEYS")).split("=")[1].split()
    assert set(OBJECTS) <= set(keys)


def test_case_list():
    recs = all_cases()
    # the all-zero record (the kernel config's None) never reaches a program
    assert len(cases.structured()) >= 40 and all(any(r) for _, r in recs) and all(any(r) for r in cases.gpu_records())
    assert all(len(r) == 12 and all(0 <= x < dsl.Q for x in r) for _, r in recs)
    labels = cases.iter_sim_labels()
    assert len(labels) >= 12
    for need in ("R = Q", "Z = 0", "P = (0, 0)", "equal lanes"):
        assert any(need in lb for lb in labels), need


@pytest.mark.parametrize("key", list(OBJECTS))
def test_workspace_slots(key):
    """the table the GPU tests size the workspace from is the build's count"""
    assert built(key)[1] == OBJECTS[key][3]


def test_h_steps_match_the_reference_steps_on_curve_points():
    """the homogeneous steps against the reference's, independently of the
    kernels: for R, Q on E' -- R as a Jacobian and as a homogeneous triple of
    the same affine point -- the new point is the same affine point, and the
    three coefficients are the reference's times ONE non-zero Fq2 factor; all
    by cross-multiplication"""
    import decode_cases as D
    import fl_ref
    import pymodel as pm
    m = pm.f2mul
    F2 = D._f2()
    g = random.Random(77)
    cp = cases.curve_points()

    def same_point(rj, rh):
        (xj, yj, zj), (xh, yh, zh) = rj, rh
        assert zj != pm.F2ZERO and zh != pm.F2ZERO
        zj2 = m(zj, zj)
        assert m(xj, zh) == m(xh, zj2) and m(yj, zh) == m(yh, m(zj2, zj))

    def same_line(cr, ch):
        assert all(c != pm.F2ZERO for c in cr + ch)
        for i in range(3):
            for j in range(i + 1, 3):
                assert m(ch[i], cr[j]) == m(ch[j], cr[i])

    pts = [cp["q"], cp["q_curve"], cp["q13"]] + [D._random_point(2, np.random.default_rng(s)) for s in (1, 2)]
    for a in pts:
        for k in (1, 2, 5):
            r = D._ec_mul(F2, a, k)
            zj, zh = (g.randrange(1, dsl.Q), g.randrange(dsl.Q)), (g.randrange(dsl.Q), g.randrange(1, dsl.Q))
            rj, rh = cases._jac(r, zj), cases._hom(r, zh)
            nj, cj = fl_ref.doubling_step(rj)
            nh, ch = ref.doubling_step_h(rh)
            same_point(nj, nh)
            same_line(cj, ch)
            same_point(cases._jac(D._ec_add(F2, r, r), (1, 0)), nh)        # and it is 2 R
            if k != 1:       # R = Q has no chord: both forms give the zero line there (cases "add: R = Q")
                nj, cj = fl_ref.addition_step(rj, a)
                nh, ch = ref.addition_step_h(rh, a)
                same_point(nj, nh)
                same_line(cj, ch)
                same_point(cases._jac(D._ec_add(F2, r, a), (1, 0)), nh)    # and it is R + Q


@pytest.mark.parametrize("key", PAIR_OBJECTS)
def test_model_matches_one_lane_and_reference(key):
    """dsl.evaluate asserts every declared bound on the way"""
    which, _, h, _ = OBJECTS[key]
    prog = built(key)[0]
    for label, rec in all_cases():
        st = dsl.Stats()
        got = run(prog, rec, st)
        assert got == ref.reference(which, rec, h), (key, label)
        assert got == run(one_lane(which, h), rec), (key, label, "one lane")
        if which == "iter":      # one of the three trips took the addition step, two skipped it
            assert st.counts["setvar"] == iter_setvars(1), label


@pytest.mark.parametrize("kind", ["max", "rand"])
@pytest.mark.parametrize("key", PAIR_OBJECTS)
def test_loop_carried_bounds(key, kind):
    """the state at the variables' value bound (limbs 2^28 - 1, value just
    below STATE_VB x 2q; `arg` values, model only): the lane pair equals the
    one-lane tower, every declared bound holding on the way"""
    import tower2
    which, _, h, _ = OBJECTS[key]
    assert STATE_VB == 5
    g = random.Random(5)
    ins = {(0, j): _edge_limbs(g, kind) for j in range(12)}
    pair = dsl.evaluate(tower2.two_pass(lambda: unit_progs.ml_step_prog(which, 2, h, raw=_raw(2)), xi_dpp=False)(), ins)
    one = dsl.evaluate(unit_progs.ml_step_prog(which, 1, h, raw=_raw(1)), ins)
    assert [pair[k] for k in range(12)] == [one[k] for k in range(12)]


# ---- the emitted code ----
@functools.lru_cache(maxsize=None)
def debug_code(key):
    prog = built(key)[0]
    cfg = kcfg.FinalExpCfg2()
    cfg.name = "pa_gen_" + key
    code, em = kcfg.build(prog, cfg, debug=True)
    assert max(len(em.mslot), 1) == OBJECTS[key][3]
    return prog, code


def simulate(key, rec, lane=3):
    """both lanes of pair `lane` through the emitted code: sim.run_lane checks
    every operation's registers against the model's trace; returns (stored
    record, model record, statistics of the model run)"""
    import sim
    prog, code = debug_code(key)
    trace, st = [], dsl.Stats()
    want = run(prog, rec, st, trace)
    IN, OUT, AUX, WS = 0x100000, 0x200000, 0x300000, 0x400000
    sm = sim.run_lane(code, [IN, OUT, AUX, lane + 1, WS], {IN: [0] * (72 * lane) + sim_check.words(rec)},
                      lane=2 * lane, trace=trace, pair=True)
    got = [sum(sm.mem.get(OUT + 576 * lane + 48 * k + 4 * j, 0) << (32 * j) for j in range(12)) for k in range(12)]
    slice_end = WS + OBJECTS[key][3] * 3584
    assert all(a < slice_end for a in sm.mem if a >= WS), "access past the wave's slice of the workspace"
    return got, want, st


@pytest.mark.parametrize("key", STEP_OBJECTS)
def test_sim_steps(key):
    which, _, h, _ = OBJECTS[key]
    for label, rec in cases.structured():
        got, want, _ = simulate(key, rec)
        assert got == want == ref.reference(which, rec, h), (key, label)


@pytest.mark.parametrize("key", ITER_OBJECTS)
def test_sim_iter(key):
    """three trips and the final doubling in emitted code: the second and
    third trips read the state the first left in the LDS and workspace homes"""
    which, _, h, _ = OBJECTS[key]
    labels = cases.iter_sim_labels()
    for label in labels:
        rec = cases.by_label(label)
        got, want, st = simulate(key, rec)
        assert got == want == ref.reference(which, rec, h), (key, label)
        assert st.counts["setvar"] == iter_setvars(1), label     # the addition step taken once, skipped twice
