"""The binary-GCD inversions stop once a = 0 (the generated kernels' loop,
emit.Emitter.emit_binv, per wave; pairing_amd/csrc/bgcd.h per lane): the
result must not move by a bit.  CPU only: the DSL model, the instruction
simulator (one lane, a whole wave of 64, a lane pair) and a host build of
bgcd.h."""
import ctypes
import os
import random
import shutil
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (os.path.join(ROOT, "tools", "pgen"), os.path.join(ROOT, "tools")):
    if p not in sys.path:
        sys.path.insert(0, p)

import dsl  # noqa: E402
import emit  # noqa: E402
import kcfg  # noqa: E402
import sim  # noqa: E402
import sim_check  # noqa: E402
import unit_progs  # noqa: E402

Q = dsl.Q
IN, OUT, AUX, WS = 0x100000, 0x200000, 0x300000, 0x400000


# ---- the model ----
def test_early_stopped_model_equals_the_28_round_definition():
    """binv_core_early == binv_core over test_binv_model_is_the_inverse's edge
    values (as the canonical y the loop sees) plus 2 000 random values; the
    stopping round lies in [0, 28]"""
    g = random.Random(4)
    edges = [0, Q, 1, Q - 1, Q + 1, 2 * Q - 1, dsl.R % Q, 1 << 380]
    vals = [v - Q if v >= Q else v for v in edges] + [g.randrange(Q) for _ in range(2000)]
    rounds = []
    for y in vals:
        w, r = dsl.binv_core_early(y)
        assert w == dsl.binv_core(y), hex(y)
        assert 0 <= r <= dsl.BINV_OUTER
        assert (r == 0) == (y == 0)
        rounds.append(r)
    # random values: the distribution the instruction estimate rests on
    # (dsl.BINV_TYPICAL); edge values such as powers of two may need more
    assert max(rounds[len(edges):]) <= dsl.BINV_TYPICAL < dsl.BINV_OUTER


def test_packed_factor_tracking_equals_the_28_step_factors():
    """two halves of 14 steps with 16-bit rows, composed, give the 28-step
    factors (dsl._binv_round asserts it on every round too): random 58-bit
    approximations, and the extremes a = 0 (g1 = 2^28) and equal values"""
    g = random.Random(8)
    pairs = [(0, Q & ((1 << 58) - 1)), (1, 1), ((1 << 58) - 1, (1 << 58) - 1), ((1 << 58) - 1, 1)]
    pairs += [(g.randrange(1 << 58), g.randrange(1 << 58) | 1) for _ in range(3000)]
    for xa, xb in pairs:
        assert dsl.binv_factors_packed(xa, xb) == dsl._binv_steps(xa, xb, 28)[2:], (hex(xa), hex(xb))
    assert dsl.binv_factors_packed(0, 5) == (1, 0, 0, 1 << 28)


def test_sim_packed_16_bit_opcodes():
    """the simulator's v_pk_sub_i16 / v_pk_add_u16 wrap each half on its own,
    v_bfe_i32 sign-extends, v_mul/mad_i32_i24 are signed"""
    K = emit.K
    code = [("v_mov_b32", 1, K(0x80000001)), ("v_mov_b32", 2, K(0x00010002)),
            ("v_pk_sub_i16", 3, 1, 2),          # (0x8000 - 1, 1 - 2) = 0x7fff, 0xffff
            ("v_pk_add_u16", 4, 1, 1),          # (0x8000 * 2, 2) = 0x0000, 0x0002
            ("v_bfe_i32", 5, 3, K(0), K(16)),   # -1
            ("v_ashrrev_i32", 6, K(16), 1),     # -32768
            ("v_mul_i32_i24", 7, 5, 6),         # 32768
            ("v_mad_i32_i24", 8, 6, 6, 5),      # 2^30 - 1
            ("s_endpgm",)]
    sm = sim.Sim(code)
    sm.run()
    assert [sm.v[k] for k in (3, 4, 5, 6, 7, 8)] == [0x7fffffff, 0x00000002, 0xffffffff, 0xffff8000, 32768, (1 << 30) - 1]


# ---- the simulator ----
def _binv_loops(code):
    """the (top, done) labels of the code's inversion loops, in program order"""
    loops = []
    for k, t in enumerate(code):
        if t[:2] == ("s_cmp_eq_u64", emit.S(32)) and code[k + 1][0] == "long_cbranch_scc1":
            back = next(u for u in code[k + 2:] if u[0] == "long_cbranch_scc1")
            loops.append((back[1], code[k + 1][1]))
    return loops


@pytest.fixture(scope="module")
def unit():
    """the test kernel tunit: its program, its code, its two inversion loops"""
    prog = unit_progs.unit_prog()
    cfg = kcfg.FinalExpCfg()
    cfg.name = prog.name
    code, _ = kcfg.build(prog, cfg, debug=True)
    loops = _binv_loops(code)
    assert len(loops) == 2
    return prog, code, loops


def _model(prog, ins):
    """(the 12 outputs, the rounds each inversion needs) by the DSL"""
    ys = []
    core = dsl.binv_core

    def spy(y):
        ys.append(y)
        return core(y)
    dsl.binv_core = spy
    try:
        out = dsl.evaluate(prog, {k: ins[k] for k in range(12)})
    finally:
        dsl.binv_core = core
    return [out[k] for k in range(12)], [dsl.binv_core_early(y)[1] for y in ys]


def _sim(code, rows, lanes):
    """rows[i]: lane lanes[i]'s record; returns (outputs per lane, Sim)"""
    n = max(lanes) + 1
    words = []
    for ln in range(n):
        words += sim_check.words(rows[lanes.index(ln)]) if ln in lanes else [0] * 72
    sm = sim.run_lane(code, [IN, OUT, AUX, n, WS], {IN: words}, lanes=lanes)
    got = [[sum(sm.mem.get(OUT + 576 * ln + 48 * k + 4 * j, 0) << (32 * j) for j in range(12)) for k in range(12)]
           for ln in lanes]
    return got, sm


def _trips(sm, loops):
    """rounds each inversion's loop ran: back edges taken + 1"""
    return [sm.taken.get(top, 0) + 1 for top, _ in loops]


def sample_rows(prog):
    """random records whose second inversion (of x2 + x3, x3 = 0) needs the
    fewest / the most rounds of a sample of 300, by the model:
    {"lo" | "hi": (rounds, record)}"""
    g = random.Random(2024)
    best = {}
    for _ in range(300):
        ins = [g.randrange(Q) for _ in range(12)]
        ins[3] = 0
        _, (_, r2) = _model(prog, ins)
        if "lo" not in best or r2 < best["lo"][0]:
            best["lo"] = (r2, ins)
        if "hi" not in best or r2 > best["hi"][0]:
            best["hi"] = (r2, ins)
    assert 0 < best["lo"][0] < best["hi"][0] < dsl.BINV_OUTER
    return best


@pytest.fixture(scope="module")
def sample(unit):
    return sample_rows(unit[0])


def _zero_row(g):
    """both inversions see 0: x0 = 0, x2 + x3 = 0"""
    r = [g.randrange(Q) for _ in range(12)]
    r[0] = r[2] = r[3] = 0
    return r


@pytest.mark.parametrize("which", ["zero", "q", "lo", "hi"])
def test_sim_one_lane_stops_at_the_models_round(unit, sample, which):
    """one lane: the loop runs max(1, the model's round) times, fewer than 28,
    and the outputs equal the DSL"""
    prog, code, loops = unit
    g = random.Random(5)
    if which == "zero":
        ins = _zero_row(g)
    elif which == "q":
        ins = [g.randrange(1, Q) for _ in range(12)]
        ins[2] = Q - ins[3]          # the sum is q: canonical 0
    else:
        ins = sample[which][1]
    want, rounds = _model(prog, ins)
    got, sm = _sim(code, [ins], [3])
    assert got[0] == want
    trips = _trips(sm, loops)
    assert trips == [max(1, r) for r in rounds]
    assert all(t < dsl.BINV_OUTER for t in trips)
    if which in ("zero", "q"):
        assert rounds[1] == 0 and trips[1] == 1
    else:
        assert rounds[1] == sample[which][0]


@pytest.mark.parametrize("slow", [0, 31, 32, 63, None])
def test_sim_whole_wave_waits_for_its_slowest_lane(unit, sample, slow):
    """64 lanes in one wave: one highest-round value among 63 zeros, at lane
    0, 31, 32 and 63 -- the wave must not leave before that lane is done --
    and a wave of 64 zeros, which leaves after the first round"""
    prog, code, loops = unit
    g = random.Random(6)
    rows = [_zero_row(g) for _ in range(64)]
    if slow is not None:
        rows[slow] = [0] + sample["hi"][1][1:]     # the first inversion sees 0, the second runs long
    models = [_model(prog, r) for r in rows]
    got, sm = _sim(code, rows, list(range(64)))
    for ln in range(64):
        assert got[ln] == models[ln][0], "lane %d" % ln
    want_trips = [max(1, max(m[1][i] for m in models)) for i in range(2)]
    assert _trips(sm, loops) == want_trips
    if slow is None:
        assert want_trips == [1, 1]
    else:
        assert want_trips[1] == sample["hi"][0]


@pytest.mark.parametrize("which", ["b0_zero", "random"])
def test_sim_lane_pairs_decompression(which):
    """the lane-pair decompression (both lanes in lockstep, the inversion on
    both) equals the DSL and rebuilds the element"""
    import test_pgen as tp
    prog = unit_progs.dec_prog(lanes=2)
    cfg = kcfg.FinalExpCfg2()
    cfg.name = prog.name
    code, _ = kcfg.build(prog, cfg, debug=True)
    ins = tp._abi_words(tp._b0_zero_element() if which == "b0_zero" else tp._cyclotomic(9))
    trace = []
    want = dsl.evaluate(prog, {k: ins[k] for k in range(12)}, trace=trace)
    _, rounds = _model(prog, ins)
    lane = 3
    sm = sim.run_lane(code, [IN, OUT, AUX, lane + 1, WS], {IN: [0] * (72 * lane) + sim_check.words(ins)},
                      lane=2 * lane, trace=trace, pair=True)
    got = [sum(sm.mem.get(OUT + 576 * lane + 48 * k + 4 * j, 0) << (32 * j) for j in range(12)) for k in range(12)]
    assert got == [want[k] for k in range(12)] == ins
    loops = _binv_loops(code)
    assert len(loops) == 1          # one inversion, run by both lanes
    assert _trips(sm, loops) == [max(1, max(rounds))] and max(rounds) < dsl.BINV_OUTER


# ---- bgcd.h, host build ----
@pytest.fixture(scope="module")
def bg(tmp_path_factory):
    if shutil.which("g++") is None:
        pytest.skip("no g++")
    d = tmp_path_factory.mktemp("bgcd_early")
    src = d / "bg.cpp"
    src.write_text('#include "bgcd.h"\n'
                   'extern "C" int bg_inverse(uint32_t* out, const uint32_t* y) '
                   '{ return pa::bgcd::inverse(out, y) ? 1 : 0; }\n')
    so = d / "libbg.so"
    subprocess.run(["g++", "-O2", "-shared", "-fPIC", "-I", os.path.join(ROOT, "pairing_amd", "csrc"),
                    str(src), "-o", str(so)], check=True)
    lib = ctypes.CDLL(str(so))

    def inv(y):
        a = (ctypes.c_uint32 * 12)(*[(y >> (32 * i)) & 0xffffffff for i in range(12)])
        o = (ctypes.c_uint32 * 12)()
        ok = lib.bg_inverse(o, a)
        return bool(ok), sum(o[i] << (32 * i) for i in range(12))
    return inv


def test_bgcd_early_exit_values(bg):
    """0, 1, 2, q - 1, 2^k for k in {29, 30, 31, 380} and 500 random values
    against pow(y, -1, q); the flag is false only for 0"""
    assert bg(0) == (False, 0)
    g = random.Random(77)
    for y in [1, 2, Q - 1] + [1 << k for k in (29, 30, 31, 380)] + [g.randrange(1, Q) for _ in range(500)]:
        ok, r = bg(y)
        assert ok and r == pow(y, -1, Q), hex(y)
