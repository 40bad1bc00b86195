"""CPU tests of the lane-pair final exponentiation's lazy Fq4 squarings
(tools/pgen/tower2.py FE2_LAZY: the three Fq2 squares of Tower.fq4_sqr and of
each half of Tower.ksqr stay double-width, one Montgomery reduction per
output; dsl.Prog.wxi is the one partner exchange, emit.Emitter.emit_wxi its
code):

  * the DSL program equals the C oracle's final exponentiation bit for bit --
    random inputs, 1, and the cyclotomic element with b0 = 0 of
    tests/golden/karabina_b0zero.json;
  * the squarings alone, on state at the loop-carried bounds (limbs
    2^28 - 1, value just below the variables' 5 x 2q), equal Tower.ksqr /
    Tower.fq4_sqr on one lane (every declared bound asserted by dsl.evaluate);
  * the emitted code of the new ops, both lanes of a pair simulated in
    lockstep, reproduces the DSL value of every operation;
  * FE2_LAZY = 0 gives the former program, operation for operation, and
    FE2_LAZY = 1 the work the change is for.
"""
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
import kernels  # noqa: E402
import sim_check  # noqa: E402
import tower2  # noqa: E402
import unit_progs  # noqa: E402
from helpers import limbs  # noqa: E402


def _fe2(monkeypatch, lazy):
    monkeypatch.setattr(tower2, "FE2_LAZY", lazy)
    return tower2.two_pass(lambda: kernels.final_exp_prog(lanes=2))()


@pytest.fixture(scope="module")
def fe2_lazy():
    mp = pytest.MonkeyPatch()
    try:
        prog = _fe2(mp, True)
    finally:
        mp.undo()
    dsl.check_scopes(prog)
    return prog


def _inputs(which):
    import pymodel as pm
    import test_pgen as tp
    if which == "one":
        return tp._abi_words(pm.F12ONE)
    if which == "b0_zero":
        return tp._abi_words(tp._b0_zero_element())
    g = random.Random(which)
    return [g.randrange(dsl.Q) for _ in range(12)]


@pytest.mark.parametrize("which", [21, 22, "one", "b0_zero"])
def test_dsl_lazy_final_exp_matches_oracle(oracle, fe2_lazy, which):
    ins = _inputs(which)
    rec = np.array([sum((limbs(x) for x in ins), [])], dtype=np.uint64)
    exp, ok = oracle.final_exponentiation(rec)
    assert ok[0]
    st = dsl.Stats()
    out = dsl.evaluate(fe2_lazy, {k: ins[k] for k in range(12)}, st)
    assert st.counts["wsop1"] == 1322 and st.counts["wxi"] == 1322 and st.counts["sopmw"] == 661
    assert [out[k] for k in range(12)] == [sum(int(w) << (64 * i) for i, w in enumerate(exp[0][6 * k:6 * k + 6]))
                                           for k in range(12)]
    if which == "one":
        assert [out[k] for k in range(12)] == ins


# ---- the squarings alone, at the loop-carried bounds ----
STATE_VB = 5          # dsl.Prog.var: a lane-pair variable holds a value below 5 x 2q


def _edge_limbs(g, kind):
    """14 limbs of a state value: "max": limbs 0..12 = 2^28 - 1 and the top limb
    as large as the value bound STATE_VB x 2q allows; "rand": a random value
    below that bound, normalized limbs"""
    top_all = STATE_VB * 2 * dsl.Q - 1
    if kind == "max":
        low = [dsl.MASK] * (dsl.NL - 1)
        return tuple(low + [(top_all - dsl.val_of(low)) >> (dsl.LB * (dsl.NL - 1))])
    return tuple(dsl.gen_fl.limbs(g.randrange(top_all + 1)))


def _raw(lanes):
    """Fq2 number k of the input as values of the state's bounds (u = 1,
    vb = STATE_VB), read as exact limbs from inputs[(0, 2k + c)]"""
    def raw(p, k):
        vs = []
        for c in (0, 1):
            v = p._val(1, vb=STATE_VB)
            p.cur.items.append(dsl.Op("arg", v, [], imm=(0, 2 * k + c)))
            vs.append(v)
        return tuple(vs) if lanes == 1 else p.sel(vs[0], vs[1])
    return raw


@pytest.mark.parametrize("kind", ["max", "rand"])
@pytest.mark.parametrize("which", ["fq4", "ksqr"])
def test_lazy_squarings_at_the_loop_carried_bounds(monkeypatch, which, kind):
    monkeypatch.setattr(tower2, "FE2_LAZY", True)
    g = random.Random(5)
    ins = {(0, j): _edge_limbs(g, kind) for j in range(12)}
    st = dsl.Stats()
    lazy = dsl.evaluate(unit_progs.sqr4_prog(which, lanes=2, raw=_raw(2)), ins, st)
    n = 3 if which == "fq4" else 2           # Fq4 squarings: two wide squares, xi on both halves, two reductions each
    assert st.counts["wsop1"] == 2 * n and st.counts["wxi"] == 2 * n and st.counts["wred"] == st.counts["sopmw"] == n
    assert st.counts["sop1"] == 6            # the six stores' conversions
    one_lane = dsl.evaluate(unit_progs.sqr4_prog(which, lanes=1, raw=_raw(1)), ins)
    assert [lazy[k] for k in range(12)] == [one_lane[k] for k in range(12)]
    # and the reduced form of the same lane-pair tower (Tower.fq4_sqr / Tower.ksqr as they are)
    monkeypatch.setattr(tower2, "FE2_LAZY", False)
    st0 = dsl.Stats()
    plain = dsl.evaluate(unit_progs.sqr4_prog(which, lanes=2, raw=_raw(2)), ins, st0)
    assert "wsop" not in st0.counts and plain == lazy


# ---- the emitted code of the new ops on a lane pair ----
@pytest.mark.parametrize("which", ["fq4", "ksqr"])
def test_sim_lazy_squarings_lane_pairs(monkeypatch, which):
    """wsop, wxi, the half-by-half add, wred and sopmw as emitted for a lane
    pair: sim.run_lane (pair=True) checks every operation's registers against
    the DSL trace, then the stored record"""
    import sim
    monkeypatch.setattr(tower2, "FE2_LAZY", True)
    prog = unit_progs.sqr4_prog(which, lanes=2)
    dsl.check_scopes(prog)
    cfg = kcfg.FinalExpCfg2()
    cfg.name = prog.name
    code, _ = kcfg.build(prog, cfg, debug=True)
    assert any(t[0] == "v_add_u32_dpp" and t[1] == t[2] for t in code)     # emit_wxi's exchange
    g = random.Random(8)
    ins = [g.randrange(dsl.Q) for _ in range(12)]
    trace = []
    want = dsl.evaluate(prog, {k: ins[k] for k in range(12)}, trace=trace)
    assert {"wsop", "wxi", "wred", "sopmw"} <= {op.kind for _, _, op in trace}
    lane = 3
    IN, OUT, AUX, WS = 0x100000, 0x200000, 0x300000, 0x400000
    sm = sim.run_lane(code, [IN, OUT, AUX, lane + 1, WS], {IN: [0] * (72 * lane) + sim_check.words(ins)},
                      lane=2 * lane, trace=trace, pair=True)
    got = [sum(sm.mem.get(OUT + 576 * lane + 48 * k + 4 * j, 0) << (32 * j) for j in range(12)) for k in range(12)]
    assert got == [want[k] for k in range(12)]


# ---- what the knob selects ----
# the operations of one lane of the lane-pair final exponentiation before this
# change (pa_gen_work.json final_exp_lane_pairs.ops as it was): 2 646 696 limb MACs
FORMER_OPS = {"add": 4456, "bcast": 737, "binv": 6, "const": 82, "dppadd": 3293, "getvar": 1854, "load_raw": 6,
              "neg": 1308, "norm": 2311, "pairz": 737, "red": 1952, "sel": 3347, "selz": 30, "setvar": 1646,
              "shl": 15, "shladd": 1352, "sop": 2836, "sop1": 2055, "sop2": 781, "store_raw": 6, "sub": 3836,
              "swap": 2787}


def _built_counts(prog):
    """as build_gen.write_work_json counts: the program as kcfg.build leaves it (adds fused)"""
    cfg = kcfg.FinalExpCfg2()
    cfg.name = "pa_gen_final_exp2"
    _, em = kcfg.build(prog, cfg)
    g = random.Random(1)
    st = dsl.Stats()
    dsl.evaluate(prog, {k: g.randrange(dsl.Q) for k in range(12)}, st)
    return st.counts, 2 * em.dyn_instr


def test_knob_off_is_the_former_program(monkeypatch):
    counts, instr = _built_counts(_fe2(monkeypatch, False))
    assert counts == FORMER_OPS
    assert 2 * build_gen.macs(counts) == 2646696
    assert round(instr) == 4377390


def test_lazy_work(fe2_lazy):
    counts, instr = _built_counts(fe2_lazy)
    assert counts["sop1"] == 72 and counts["wsop1"] == 1322 and counts["wred"] == counts["sopmw"] == 661
    assert counts["red"] <= FORMER_OPS["red"] and counts["norm"] < FORMER_OPS["norm"]
    assert 2 * build_gen.macs(counts) <= 2460000
    assert round(instr) <= 4377390
