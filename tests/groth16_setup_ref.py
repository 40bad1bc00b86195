"""CPU reference of Groth16 parameter generation (pa_groth16_generate*,
include/pairing_amd.h) on Python integers mod r, with nothing from the code
under test: bellman's generate_parameters for a given trapdoor.

L_j(tau) is the integer inverse transform of the powers of tau, L_j = n^-1
sum_i tau^i w^(-ij), which needs no inversion and holds for every tau, tau in
the domain and tau = 0 included (groth16_ref.real_setup uses the closed form and
asserts those away).  The expected points are generator multiples of the
oracle, as groth16_ref.Key.points makes them.

A system is `mats` = (A, B, C) as in groth16_ref: lists of rows of (column,
coefficient) pairs."""
import numpy as np

from helpers import R_ORDER, rng, small_scalars
from groth16_ref import rand_fr
from test_fr_ntt import mont_rows, omega


def trapdoor_of(seed):
    """(tau, alpha, beta, gamma, delta) exactly as groth16_ref.real_setup(seed, ...) draws them"""
    return tuple(x or 1 for x in rand_fr(rng(seed), 5))


def lagrange_at(tau, log_n):
    """[L_j(tau)] for j < n by the defining sum n^-1 sum_i tau^i w^(-ij) (n^2 products: for the tests' small n)"""
    n = 1 << log_n
    winv = pow(omega(log_n), -1, R_ORDER) if log_n else 1
    ninv = pow(n, -1, R_ORDER)
    pw = [pow(tau, i, R_ORDER) for i in range(n)]
    wp = [pow(winv, e, R_ORDER) for e in range(n)]
    return [ninv * sum(pw[i] * wp[i * j % n] for i in range(n)) % R_ORDER for j in range(n)]


def lagrange_by_transform(tau, log_n):
    """the same by an integer radix-2 inverse transform of the powers (n log n products: the log_n = 11 test)"""
    n = 1 << log_n
    a = [pow(tau, i, R_ORDER) for i in range(n)]
    if log_n == 0:
        return a
    winv = pow(omega(log_n), -1, R_ORDER)

    def rec(v, w):
        if len(v) == 1:
            return v
        ev, od = rec(v[0::2], w * w % R_ORDER), rec(v[1::2], w * w % R_ORDER)
        out, t, half = [0] * len(v), 1, len(v) // 2
        for k in range(half):
            x = t * od[k] % R_ORDER
            out[k], out[k + half] = (ev[k] + x) % R_ORDER, (ev[k] - x) % R_ORDER
            t = t * w % R_ORDER
        return out

    ninv = pow(n, -1, R_ORDER)
    return [x * ninv % R_ORDER for x in rec(a, winv)]


def column_sums(mats, lag, n_vars):
    """(u, v, w): per matrix the n_vars integers sum_j M[j][i] L_j"""
    out = []
    for rows in mats:
        acc = [0] * n_vars
        for j, row in enumerate(rows):
            for c, v in row:
                acc[c] = (acc[c] + v * lag[j]) % R_ORDER
        out.append(acc)
    return out


class Setup:
    """the discrete logarithms of every point of the keys.  g1_scalars / g2_scalars are the two output arrays
    of the header in their order; the named lists are the slices."""

    def __init__(self, mats, n_vars, n_public, log_n, trapdoor, lag=None):
        tau, alpha, beta, gamma, delta = trapdoor
        assert gamma and delta and all(0 <= x < R_ORDER for x in trapdoor)
        n = 1 << log_n
        assert all(len(rows) <= n for rows in mats) and 0 <= n_public <= n_vars
        self.n_vars, self.n_public, self.log_n, self.trapdoor = n_vars, n_public, log_n, trapdoor
        self.lag = lagrange_at(tau, log_n) if lag is None else lag
        self.u, self.v, self.w = column_sums(mats, self.lag, n_vars)
        ginv, dinv = pow(gamma, -1, R_ORDER), pow(delta, -1, R_ORDER)
        mix = [(beta * a + alpha * b + c) % R_ORDER for a, b, c in zip(self.u, self.v, self.w)]
        self.ic = [x * ginv % R_ORDER for x in mix[:n_public]]
        self.l = [x * dinv % R_ORDER for x in mix[n_public:]]
        z = (pow(tau, n, R_ORDER) - 1) % R_ORDER
        self.h = [pow(tau, i, R_ORDER) * z * dinv % R_ORDER for i in range(n - 1)]
        self.alpha, self.beta, self.gamma, self.delta = alpha, beta, gamma, delta
        self.g1_scalars = self.u + self.v + self.ic + self.l + self.h + [alpha, beta, delta]
        self.g2_scalars = self.v + [beta, gamma, delta]
        assert len(self.g1_scalars) == 3 * n_vars + n + 2 and len(self.g2_scalars) == n_vars + 3

    def trapdoor_rows(self):
        """(5, 4) Montgomery rows tau, alpha, beta, gamma, delta"""
        return mont_rows(list(self.trapdoor))

    def scalar_rows(self):
        """what pa_groth16_generate_scalars writes"""
        return mont_rows(self.g1_scalars)

    def segments(self):
        """name -> (first row, rows) of g1_out, and of g2_out under the names ending in g2 / g2_query"""
        nv, n = self.n_vars, 1 << self.log_n
        c0 = 3 * nv + n - 1
        return {"a_query": (0, nv), "b_g1_query": (nv, nv), "ic": (2 * nv, self.n_public),
                "l_query": (2 * nv + self.n_public, nv - self.n_public), "h_query": (3 * nv, n - 1),
                "alpha_g1": (c0, 1), "beta_g1": (c0 + 1, 1), "delta_g1": (c0 + 2, 1),
                "b_g2_query": (0, nv), "beta_g2": (nv, 1), "gamma_g2": (nv + 1, 1), "delta_g2": (nv + 2, 1)}

    def g1_points(self, oracle, rows=None, mult=1, nthreads=8):
        """the affine records of (mult s_i) G for the rows `rows` of g1_out (all of them by default)"""
        s = self.g1_scalars if rows is None else [self.g1_scalars[i] for i in rows]
        if not s:
            return np.zeros((0, 13), np.uint64)
        return oracle.g1_mul_generator(small_scalars([x * mult % R_ORDER for x in s]), nthreads)

    def g2_points(self, oracle, rows=None, mult=1, nthreads=8):
        s = self.g2_scalars if rows is None else [self.g2_scalars[i] for i in rows]
        if not s:
            return np.zeros((0, 25), np.uint64)
        return oracle.g2_mul_generator(small_scalars([x * mult % R_ORDER for x in s]), nthreads)


def infinity_g1(n):
    """n records of the point at infinity as into_affine writes it: (0, 1) in Montgomery form, flag set"""
    from helpers import set_infinity
    out = np.zeros((n, 13), np.uint64)
    if n:
        set_infinity(out, range(n))
    return out


__all__ = [name for name in dir() if not name.startswith("_")]
