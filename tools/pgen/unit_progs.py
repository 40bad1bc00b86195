"""Small generated TEST kernels (not product code): they exercise single
pieces of the emitted code on the GPU against the DSL model
(tests/test_gen_units.py) -- the in-kernel binary GCD, the zero-test select
and Karabina decompression, whose rare branch random pairings never reach.
Both use the final-exponentiation record layout (12 Fq in, 12 Fq out)."""
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
