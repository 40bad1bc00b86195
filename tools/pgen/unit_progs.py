"""Small generated TEST kernels (not product code): they exercise single
pieces of the emitted code on the GPU against the DSL model
(tests/test_gen_units.py) -- the in-kernel binary GCD, the zero-test select
and Karabina decompression, whose rare branch random pairings never reach;
and the Miller loop's pieces (ml_step_prog; tests/test_ml_steps.py on the
CPU, tests/test_ml_steps_gpu.py on the GPU).
All use the final-exponentiation record layout (12 Fq in, 12 Fq out)."""
from dsl import Prog
from tower import TowerLazySq


def dec_prog(lanes=1):
    """load an Fq12, keep its compressed coordinates (a1, a2, b0, b2),
    decompress them (kdec_numden + batch_inv2 over one value + kdec_finish)
    and store the Fq12.  lanes = 2: the lane-pair tower (tower2.Tower2, the
    round-5 lane-pair final exponentiation's decompression)"""
    import kernels
    from tower2 import Tower2
    p = Prog("tdec" if lanes == 1 else "tdec2", lanes, use_norm=True)
    p.binv_ok = True
    T = TowerLazySq(p) if lanes == 1 else Tower2(p)
    V = kernels._Vars(p, lanes)
    (_, a1, a2), (b0, _, b2) = V.load12()
    g = (a1, a2, b0, b2)
    num, den, w = T.kdec_numden(g)
    (iden,) = T.batch_inv2([den], "t")
    V.store12(T.kdec_finish(g, num, iden, w))
    return p


def sqr4_prog(which, lanes=2, raw=None):
    """the squarings of the final exponentiation's loops on their own
    (tests/test_pgen_lazy2.py): "fq4": Tower.fq4_sqr of the pairs (a0, b1),
    (b0, a2), (a1, b2) of an Fq12; "ksqr": Tower.ksqr of its compressed
    coordinates (a1, a2, b0, b2), the two other Fq2 passed through.
    raw: a function (prog, k) -> the Fq2 number k of the input as a value of
    the caller's own bounds instead of a load (the loop-carried state)"""
    import kernels
    from tower import Tower
    from tower2 import Tower2
    p = Prog("tsqr4%s%d" % (which, lanes), lanes, use_norm=True)
    T = Tower(p) if lanes == 1 else Tower2(p)
    V = kernels._Vars(p, lanes)
    if raw is None:
        (a0, a1, a2), (b0, b1, b2) = V.load12()
    else:
        a0, a1, a2, b0, b1, b2 = (raw(p, k) for k in range(6))
    if which == "fq4":
        (a0, b1), (b0, a2), (a1, b2) = T.fq4_sqr(a0, b1), T.fq4_sqr(b0, a2), T.fq4_sqr(a1, b2)
    else:
        a1, a2, b0, b2 = T.ksqr((a1, a2, b0, b2))
    V.store12(((a0, a1, a2), (b0, b1, b2)))
    return p


ML_STEPS = ("dbl", "add", "ell", "sqr12", "mul12", "iter")
ITER_TRIPS = 3
ITER_MASK = 0b010     # the addition step: skipped in the first trip, taken in the second, skipped in the third


def ml_step_prog(which, lanes=2, pairing_only=False, raw=None):
    """the pieces of the Miller loop on their own (tests/test_ml_steps.py,
    tests/test_ml_steps_gpu.py), each on one record of six Fq2 in (Fq2 number
    k = slots 2k, 2k + 1) and six Fq2 out:

      "dbl"    R = (Fq2 0, 1, 2)                 -> c0, c1, c2, R'x, R'y, R'z
               kernels.doubling_step (pairing_only: doubling_step_h)
      "add"    R = (Fq2 0, 1, 2), Q = (Fq2 3, 4) -> c0, c1, c2, R'x, R'y, R'z
               kernels.addition_step (pairing_only: addition_step_h)
      "ell"    f = the six Fq2, (px, py) = the two halves of Fq2 0 (over lane
               pairs the packed px | py slot, read by the two broadcasts of
               kernels.line), c2 = Fq2 5, c1 = Fq2 4, c0 = red2(Fq2 3 + Fq2 2)
               -> kernels.ell(f, c, px, py)
      "sqr12"  f -> sqr12(f)
      "mul12"  f -> mul12(f, g), g = f with its six Fq2 rotated by one place
               (g's Fq2 k = f's Fq2 k + 1)
      "iter"   the loop of kernels.miller_loop_prog on its own variables and
               homes, the state taken from the record: packed P = Fq2 0,
               Q = (Fq2 1, 2), R = (Fq2 3, 4, 5), f = the six Fq2; ITER_TRIPS
               trips of line("dbl"), line("add") where ITER_MASK has the
               trip's bit, sqr12; then line("dbl") and conj12 -> f

    lanes = 1: the same program on tower.Tower, the twin the lane pair is
    compared with.  Every program loads the whole record, slot 11 last
    (kcfg.FinalExpCfg.after_load sets the valid mask there; the all-zero
    record is that config's None and gives zeros).
    raw: a function (prog, k) -> the Fq2 number k of the input as a value of
    the caller's own bounds instead of a load (the loop-carried state)"""
    import kernels
    from tower import Tower
    from tower2 import Tower2
    assert which in ML_STEPS
    p = Prog("tml%d_%s%s" % (lanes, which, "h" if pairing_only else ""), lanes, use_norm=kernels._norm(lanes))
    T = Tower(p) if lanes == 1 else Tower2(p)
    V = kernels._Vars(p, lanes)
    steps = kernels.g2_steps(pairing_only)
    if which == "iter":
        kernels.ml_declare(p, V, kernels.ml_homes(lanes))
    if raw is None:
        f = V.load12()
    else:
        xs = [raw(p, k) for k in range(6)]
        f = ((xs[0], xs[1], xs[2]), (xs[3], xs[4], xs[5]))
    xs = [x for c6 in f for x in c6]
    if which == "dbl":
        c, r = steps[0](T, (xs[0], xs[1], xs[2]))
        out = (tuple(c), tuple(r))
    elif which == "add":
        c, r = steps[1](T, (xs[0], xs[1], xs[2]), xs[3], xs[4])
        out = (tuple(c), tuple(r))
    elif which == "ell":
        c = (T.red2(T.add2(xs[3], xs[2])), xs[4], xs[5])
        px, py = xs[0] if lanes == 1 else (p.bcast(xs[0], 0), p.bcast(xs[0], 1))
        out = kernels.ell(T, f, c, px, py)
    elif which == "sqr12":
        out = T.sqr12(f)
    elif which == "mul12":
        g = xs[1:] + xs[:1]
        out = T.mul12(f, ((g[0], g[1], g[2]), (g[3], g[4], g[5])))
    else:
        if lanes == 1:
            p.set("px", xs[0][0])
            p.set("py", xs[0][1])
        else:
            p.set("px", xs[0])       # lane 0: px, lane 1: py
        for n, v in zip(("qx", "qy", "rx", "ry", "rz"), xs[1:]):
            V.set2(n, v)
        V.set12("f", f)
        with p.loop(ITER_TRIPS) as L:
            kernels.line(p, T, V, steps, "dbl")
            with p.if_bit(ITER_MASK, L):
                kernels.line(p, T, V, steps, "add")
            V.set12("f", T.sqr12(V.get12("f")))
        kernels.line(p, T, V, steps, "dbl")
        out = T.conj12(V.get12("f"))
    V.store12(out)
    return p


def unit_prog():
    """binv of a product and of a sum, selz with two tests and with one"""
    p = Prog("tunit", use_norm=True)
    xs = [p.load(k) for k in range(12)]
    y = p.mul(xs[0], xs[1])
    i1 = p.binv(y)
    i2 = p.binv(p.red(p.add(xs[2], xs[3])))
    z = p.selz([p.red_full(xs[4]), p.red_full(xs[5])], i1, i2)
    z2 = p.selz([p.red_full(xs[6])], xs[7], xs[8])
    for k, v in enumerate([i1, i2, z, z2, p.mul(i1, y)] + xs[5:12]):
        p.store(k, p.red(v))
    return p
