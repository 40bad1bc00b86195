"""CPU tests of the final exponentiation's exponent chain (tools/pgen/kernels.py):

  * exp_by_x_karabina takes the top of |x| = 2^16 + 2^48 + 2^57 * 105 as
    105 = 7 * 15 (7 squarings and 4 Fq12 products, where the set bits one by
    one cost 6 and 5);
  * hard_part_seq evaluates the hard part as one sequential chain,
    r^((x - 1)^2 (x + p) (x^2 + p^2 - 1) + 3), five exp_by_x by the full x.

The value is the same power of the same element, so every output word must
stay: the integer identities, dsl.evaluate of the one-lane and the lane-pair
program against the former chain (final_exp_prog's x715 / seq false, what
PGEN_X715=0 PGEN_HP_SEQ=0 build) and the C oracle, the built programs' work
against the parent's committed pa_gen_work.json, and the emitted lane-pair
code in the instruction simulator.
"""
import json
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
from helpers import GOLDEN, Q, RMONT, limbs, random_scalars, rng, set_infinity  # noqa: E402

X = -0xd201000000010000      # the BLS12-381 parameter (mod.rs:116-121: exp_by_x conjugates)
ONE = [RMONT % Q] + [0] * 11  # the identity as the records hold it (Montgomery form, R = 2^384)


# ---- integers ----
def test_x_is_two_low_bits_and_seven_times_fifteen():
    assert -X == kernels.X_ABS == (1 << 16) + (1 << 48) + (1 << 57) * 7 * 15
    # 7 = 2^3 - 1 and 15 = 2^4 - 1: t^8 conj(t), then its 16th power times its conjugate
    assert 7 * 15 == ((1 << 3) - 1) * ((1 << 4) - 1) == 0b1101001


def test_reference_chain_exponent_is_the_factored_polynomial():
    """mod.rs:125-156 step by step on exponents (r -> r^e; E = exp_by_x is
    multiplication by x, conjugation by -1 in the cyclotomic subgroup, the
    Frobenius map by p^k), against (x - 1)^2 (x + p) (x^2 + p^2 - 1) + 3 --
    equal as integers, not only modulo the group order"""
    x, p = X, Q
    assert x % 2 == 0
    r = 1
    y0 = 2 * r                   # y0 = r^2
    y1 = y0 * x                  # a: exp_by_x(y0, x)
    y2 = y1 * (x // 2)           # b: exp_by_x(y1, x >> 1)
    y3 = -r                      # conj(r)
    y1 = y1 + y3
    y1 = -y1
    y1 = y1 + y2
    y2 = y1 * x                  # c
    y3 = y2 * x                  # d
    y1 = -y1
    y3 = y3 + y1
    y1 = -y1
    y1 = y1 * p ** 3
    y2 = y2 * p ** 2
    y1 = y1 + y2
    y2 = y3 * x                  # e
    y2 = y2 + y0
    y2 = y2 + r
    y1 = y1 + y2
    y2 = y3 * p
    y1 = y1 + y2
    a = (x - 1) ** 2
    assert y1 == a * (p ** 3 + x * p ** 2 + (x * x - 1) * p + x * (x * x - 1)) + 3
    assert y1 == (x - 1) ** 2 * (x + p) * (x * x + p * p - 1) + 3
    # hard_part_seq's steps
    t0 = x - 1
    t1 = t0 * x - t0
    t2 = t1 * x + t1 * p
    t3 = t2 * x * x + (t2 * p * p - t2)
    assert t3 + 3 == y1


# ---- dsl.evaluate ----
def _prog(lanes, x715, seq):
    """the program as build_gen.PROGRAMS "fe" / "fe2" make it, on the given chain"""
    if lanes == 2:
        prog = tower2.two_pass(lambda: kernels.final_exp_prog(lanes=2, x715=x715, seq=seq))()
    else:
        prog = kernels.final_exp_prog(lazy="sq", x715=x715, seq=seq)
    dsl.check_scopes(prog)
    return prog


def test_the_build_takes_the_new_chain(monkeypatch):
    """without switches the built kernels are on the new chain; each switch turns its part back"""
    for k in ("PGEN_X715", "PGEN_HP_SEQ"):
        monkeypatch.delenv(k, raising=False)
    assert kernels.built_chain() == {"x715": True, "seq": True}
    monkeypatch.setenv("PGEN_X715", "0")
    assert kernels.built_chain() == {"x715": False, "seq": True}
    monkeypatch.setenv("PGEN_HP_SEQ", "0")
    assert kernels.built_chain() == {"x715": False, "seq": False}


@pytest.fixture(scope="module")
def progs():
    """(lanes, form) -> program; "new": the chain the build takes, "old": the former chain"""
    out = {}
    for lanes in (1, 2):
        out[lanes, "new"] = _prog(lanes, True, True)
        out[lanes, "old"] = _prog(lanes, False, False)
    return out


def _ints(rec):
    return [sum(int(w) << (64 * i) for i, w in enumerate(rec[6 * k:6 * k + 6])) for k in range(12)]


@pytest.fixture(scope="module")
def cases(oracle):
    """name -> (the 12 canonical input integers, the oracle's 12 output integers)"""
    g = random.Random(31)
    ins = {"random": [g.randrange(Q) for _ in range(12)],
           "one": ONE,
           # c1 = 0: an element of Fq6, conj(f) / f = 1, so every exp_by_x squares and
           # decompresses the identity (b0 = a2 = 0: the shared inversion's 0 -> 0 path)
           "fq6": [g.randrange(Q) for _ in range(6)] + [0] * 6}
    gn = rng(41)
    p = oracle.g1_mul_generator(random_scalars(gn, 2))
    q = oracle.g2_mul_generator(random_scalars(gn, 2))
    set_infinity(p, [1])
    ml = oracle.miller_loop_batch(p, oracle.g2_prepare(q))
    ins["miller"] = _ints(ml[0])
    ins["miller_infinity"] = _ints(ml[1])
    assert ins["miller_infinity"] == ONE
    out = {}
    for name, v in ins.items():
        rec = np.array([sum((limbs(x) for x in v), [])], dtype=np.uint64)
        exp, ok = oracle.final_exponentiation(rec)
        assert ok[0]
        out[name] = (v, _ints(exp[0]))
    return out


@pytest.mark.parametrize("which", ["random", "one", "fq6", "miller", "miller_infinity"])
@pytest.mark.parametrize("lanes", [1, 2])
def test_dsl_new_chain_equals_old_chain_and_oracle(progs, cases, lanes, which):
    ins, want = cases[which]
    new = dsl.evaluate(progs[lanes, "new"], {k: ins[k] for k in range(12)})
    old = dsl.evaluate(progs[lanes, "old"], {k: ins[k] for k in range(12)})
    assert [new[k] for k in range(12)] == [old[k] for k in range(12)] == want
    if which in ("one", "fq6", "miller_infinity"):
        assert want == ONE


def test_each_switch_alone_gives_the_same_value(cases):
    """7 * 15 with the reference chain, and the sequential chain with the bits
    one by one (the attribution builds)"""
    ins, want = cases["random"]
    for x715, seq in ((True, False), (False, True)):
        out = dsl.evaluate(_prog(2, x715, seq), {k: ins[k] for k in range(12)})
        assert [out[k] for k in range(12)] == want


# ---- static: the work of the built programs against the parent's record ----
def _parent_work():
    """tests/golden/fe_chain_parent_work.json: pairing_amd/lib/pa_gen_work.json
    exactly as the commit before the chain change holds it"""
    with open(os.path.join(GOLDEN, "fe_chain_parent_work.json")) as f:
        return json.load(f)


def _built(which, cfgc, kname, prog):
    cfg = cfgc()
    cfg.name = kname
    _, em = kcfg.build(prog, cfg)
    g = random.Random(1)
    st = dsl.Stats()
    dsl.evaluate(prog, {k: g.randrange(Q) for k in range(12)}, st)
    return {"instructions": round(prog.lanes * em.dyn_instr), "limb_macs": prog.lanes * build_gen.macs(st.counts),
            "slots": max(len(em.mslot), 1), "ops": st.counts}


@pytest.fixture(scope="module")
def built(progs):
    out = {}
    for lanes, cfgc, kname in ((1, kcfg.FinalExpCfg, "pa_gen_final_exp"), (2, kcfg.FinalExpCfg2, "pa_gen_final_exp2")):
        for form in ("new", "old"):
            out[lanes, form] = _built(form, cfgc, kname, progs[lanes, form])
    return out


@pytest.mark.parametrize("lanes,name", [(2, "final_exp_lane_pairs"), (1, "final_exp")])
def test_built_program_does_less_work_than_the_parents_record(built, lanes, name):
    parent = _parent_work()[name]
    new, old = built[lanes, "new"], built[lanes, "old"]
    # the committed record, which the build writes from build_gen.PROGRAMS, is the new program's
    with open(os.path.join(ROOT, "pairing_amd", "lib", "pa_gen_work.json")) as f:
        cur = json.load(f)[name]
    assert (cur["instructions"], cur["limb_macs"], cur["ops"]) == (new["instructions"], new["limb_macs"], new["ops"])
    assert new["instructions"] < parent["instructions"] and new["limb_macs"] < parent["limb_macs"]
    assert new["slots"] <= old["slots"]
    # both switches back: the parent's program, operation for operation
    assert old["instructions"] == parent["instructions"] and old["limb_macs"] == parent["limb_macs"]
    assert old["ops"] == parent["ops"]


def test_lane_pair_workspace_shrinks(built):
    """only r and the current call's input are parked across an exp_by_x, and
    the parked t / t7 reuse the snapshots' homes"""
    assert built[2, "new"]["slots"] < built[2, "old"]["slots"]
    assert built[1, "new"]["slots"] < built[1, "old"]["slots"]


# ---- the emitted lane-pair code ----
@pytest.mark.slow
@pytest.mark.parametrize("which", ["one", "random"])
def test_sim_emitted_fe2_equals_dsl(progs, cases, which):
    """pa_gen_final_exp2 as emitted, both lanes of a pair in lockstep
    (sim.run_lane checks every operation's registers against the DSL trace),
    on the identity -- every decompression on its 0 / 0 path -- and on a
    random input"""
    import sim
    prog = progs[2, "new"]
    cfg = kcfg.FinalExpCfg2()
    cfg.name = prog.name
    code, _ = kcfg.build(prog, cfg, debug=True)
    ins = cases[which][0]
    trace = []
    want = dsl.evaluate(prog, {k: ins[k] for k in range(12)}, trace=trace)
    assert [want[k] for k in range(12)] == cases[which][1]
    lane = 3
    IN, OUT, AUX, WS = 0x100000, 0x200000, 0x300000, 0x400000
    sm = sim.run_lane(code, [IN, OUT, AUX, lane + 1, WS], {IN: [0] * (72 * lane) + sim_check.words(ins)},
                      lane=2 * lane, trace=trace, pair=True)
    got = [sum(sm.mem.get(OUT + 576 * lane + 48 * k + 4 * j, 0) << (32 * j) for j in range(12)) for k in range(12)]
    assert got == [want[k] for k in range(12)]
