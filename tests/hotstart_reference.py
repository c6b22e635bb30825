"""What the warm-start tests share (ultranest_amd/hotstart.py): the host problem of the fixture, the seeded sample sets, an
independent numpy restatement of the contbox deformation (with five switchable defects, which the fixture must reject), the
derived bound of the summed log-volume, a high-precision restatement of the independent Student-t form, and the evidence
of the contbox problem of a separable Gaussian, ``ln integral_0^1 Z_box(t) dt``, by erf products and quadrature.

The fixture tests/golden/g19_hotstart.npz is recorded from the reference by tests/golden/make_hotstart.py.

The weight bound.  The weight is ``((log w_0 + log w_1) + ...) + log w_(d-1)`` with ``w_i = uhi_i - ulo_i`` in binary64 (the
restatement gives those bits).  Each log is within 1 ulp of the exact logarithm of its binary64 argument (the stated error of
the device's and of glibc's ``log``): ``|l_i - log w_i| <= 2^-52 |log w_i|``.  The d - 1 sequential additions each round
their exact sum by at most ``2^-53 |S_k|`` with ``|S_k| <= sum_i |l_i|``.  So

    |weight - sum_i log w_i|  <=  (2^-52 + (d - 1) * 2^-53) * (1 + 2^-52) * sum_i |log w_i|  =:  weight_bound

with the exact sum taken by mpmath over the binary64 ``w_i``.  A ``w_i`` of 0 gives -inf on both sides (bound 0, compared by
equality); a negative one NaN.
"""
import math
import os

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
FIXTURE = os.path.join(HERE, "golden", "g19_hotstart.npz")
DIMS = (1, 2, 5)
NSAMPLES = (11, 400)
NROWS = 33
STEPS = np.power(10.0, [-1.0, -3.0, -5.0, -7.0])
EPS = 2.0 ** -53
DEFECTS = ("segment_off_by_one", "swapped_lo_hi", "weight_sign", "missing_last_knot", "interp_from_right_knot")


# ---- the host problem of the fixture: an affine transform and a Gaussian around fixed centres ----

def centers(d):
    return (np.sin(np.arange(d) / 2.) * 0.5 + 1.) / 2. * 20.0 - 10.0


def host_transform(x):
    return np.asarray(x) * 20.0 - 10.0


def host_loglike(p):
    p = np.asarray(p)
    return -0.5 * (((p - centers(p.shape[-1])) / 0.7) ** 2).sum(axis=-1)


# ---- seeded samples ----

def samples(d, n):
    """(upoints (n, d), uweights (n,)) strictly inside the cube, weights summing to 1"""
    rs = np.random.RandomState(1000 * d + n)
    ctr = 0.3 + 0.4 * rs.uniform(size=d)
    up = np.clip(ctr + 0.03 * rs.normal(size=(n, d)), 1e-6, 1 - 1e-6)
    w = rs.uniform(0.2, 1.0, size=n)
    return up, w / w.sum()


def moments(up, w):
    """weighted centre, standard deviation and inverse covariance of the samples"""
    ctr = (up * w[:, None]).sum(axis=0)
    dx = up - ctr
    cov = (dx[:, :, None] * dx[:, None, :] * w[:, None, None]).sum(axis=0)
    return ctr, np.sqrt(np.diag(cov)), np.linalg.inv(cov)


def contbox_test_rows(d, xp, seed):
    """33 cube rows (d + 1 wide): t on every knot (at most 25), u within 2^-53 of both ends, the rest seeded"""
    rs = np.random.RandomState(seed)
    u = rs.uniform(size=(NROWS, d + 1))
    m = len(xp)
    u[:m, d] = xp
    u[m:, d] = rs.uniform(size=NROWS - m)
    u[0, :d] = EPS
    u[1, :d] = 1.0 - EPS
    u[m, :d] = EPS
    u[m + 1, :d] = 1.0 - EPS
    u[m + 2, d] = EPS
    u[m + 3, d] = 1.0 - EPS
    return u


def cube_test_rows(d, seed):
    """33 cube rows (d wide) for the Student-t forms: both ends within 2^-53, the rest seeded"""
    u = np.random.RandomState(seed).uniform(size=(NROWS, d))
    u[0] = EPS
    u[1] = 1.0 - EPS
    u[2, ::2] = EPS
    u[3, ::2] = 1.0 - EPS
    u[4] = 0.5
    return u


# ---- the contbox deformation restated (numpy's interp formula, not np.interp) ----

def contbox_restated(u, ulos, uhis, xp, defect=None):
    """(umod (n, d), weight (n,), segment (n,), decided (n,)): every row's segment j is the largest index <= M - 2 with
    xp[j] <= t; `decided` says that a row found its segment (none falls into a gap or past the last knot)."""
    u = np.asarray(u, dtype=float)
    xp = np.asarray(xp, dtype=float)
    M = len(xp)
    if defect == "missing_last_knot":
        xp, ulos, uhis, M = xp[:-1], ulos[:-1], uhis[:-1], M - 1
    d = ulos.shape[1]
    t = u[:, d]
    j = np.clip(np.searchsorted(xp, t, side="right") - 1, 0, M - 2)
    decided = (xp[j] <= t) & ((t < xp[j + 1]) | ((j == M - 2) & (t <= xp[M - 1])))
    if defect == "segment_off_by_one":
        j = np.clip(j + 1, 0, M - 2)
    right, left = t >= xp[M - 1], t <= xp[0]
    dx = xp[j + 1] - xp[j]
    umod = np.empty((len(u), d))
    weight = np.zeros(len(u))
    for i in range(d):
        lo, hi = (uhis, ulos) if defect == "swapped_lo_hi" else (ulos, uhis)
        ends = []
        for fp in (lo[:, i], hi[:, i]):
            slope = (fp[j + 1] - fp[j]) / dx
            if defect == "interp_from_right_knot":
                v = slope * (t - xp[j + 1]) + fp[j + 1]
            else:
                v = slope * (t - xp[j]) + fp[j]
            v = np.where(right, fp[M - 1], np.where(left, fp[0], v))
            ends.append(v)
        wd = ends[1] - ends[0]
        umod[:, i] = ends[0] + wd * u[:, i]
        with np.errstate(all="ignore"):
            lw = np.log(wd)
        weight = weight - lw if defect == "weight_sign" else weight + lw
    return umod, weight, j, decided


def weight_exact_and_bound(u, ulos, uhis, xp):
    """(exact sum of log w_i by mpmath over the binary64 widths, the derived bound) per row"""
    import mpmath
    mpmath.mp.dps = 50
    xp = np.asarray(xp, dtype=float)
    u = np.asarray(u, dtype=float)
    d = ulos.shape[1]
    M = len(xp)
    t = u[:, d]
    j = np.clip(np.searchsorted(xp, t, side="right") - 1, 0, M - 2)
    exact, bound = np.empty(len(u)), np.empty(len(u))
    for r in range(len(u)):
        logs = []
        for i in range(d):
            ends = []
            for fp in (ulos[:, i], uhis[:, i]):
                slope = (fp[j[r] + 1] - fp[j[r]]) / (xp[j[r] + 1] - xp[j[r]])
                v = slope * (t[r] - xp[j[r]]) + fp[j[r]]
                if t[r] >= xp[M - 1]:
                    v = fp[M - 1]
                elif t[r] <= xp[0]:
                    v = fp[0]
                ends.append(v)
            wd = ends[1] - ends[0]
            logs.append(mpmath.log(mpmath.mpf(float(wd))) if wd > 0 else (mpmath.mpf("-inf") if wd == 0 else mpmath.nan))
        s = sum(logs)
        a = sum(abs(v) for v in logs)
        exact[r] = float(s)
        bound[r] = float((2.0 ** -52 + (d - 1) * 2.0 ** -53) * (1 + 2.0 ** -52) * a) if mpmath.isfinite(a) else 0.0
    return exact, bound


def weight_excess(weight, exact, bound):
    """|weight - exact| / bound per row (0 where both are the same non-finite value or equal; inf where they disagree at bound 0)"""
    out = np.zeros(len(weight))
    for r in range(len(weight)):
        if weight[r] == exact[r] or (np.isnan(weight[r]) and np.isnan(exact[r])):
            continue
        # the exact value rounded to binary64 adds half an ulp of its own
        b = bound[r] + 2.0 ** -53 * abs(exact[r])
        out[r] = abs(weight[r] - exact[r]) / b if b > 0 and np.isfinite(weight[r]) else np.inf
    return out


def table(M, d, seed):
    """a contbox table of M knots (2 <= M <= 25): (ulos, uhis, xp), nested boxes growing to the cube, ascending knots"""
    rs = np.random.RandomState(100 * M + d + seed)
    xp = np.concatenate([[0.0], np.sort(rs.uniform(0.05, 0.95, size=M - 2)), [1.0]])
    lo = np.sort(rs.uniform(0.0, 0.45, size=(M, d)), axis=0)[::-1].copy()
    hi = np.sort(rs.uniform(0.55, 1.0, size=(M, d)), axis=0).copy()
    lo[-1], hi[-1] = 0.0, 1.0
    return lo, hi, xp


# ---- form (b) in high precision ----

def independent_exact(u, ctr, err, df, loglike_of_x):
    """L of form (b) per row with the quantile, the log-density and the sum taken by mpmath (40 digits):
    x_i = ctr_i + err_i tppf(u_i w_i + lo_i), L = loglike_of_x(x) - sum_i logpdf_i(x_i); w_i, lo_i the binary64 table values.
    Returns (x (n, d), sum of the log-densities (n,), L (n,))."""
    import mpmath
    from ultranest_amd import hotstart
    mpmath.mp.dps = 40
    ctr, err, w, lo, c, consts = hotstart.independent_tables(np.asarray(ctr, float), np.asarray(err, float), float(df))
    nu = mpmath.mpf(float(df))
    lognorm = mpmath.loggamma((nu + 1) / 2) - mpmath.loggamma(nu / 2) - mpmath.log(nu * mpmath.pi) / 2

    import scipy.stats
    rv = scipy.stats.t(float(df))
    norm = mpmath.gamma((nu + 1) / 2) / (mpmath.sqrt(nu * mpmath.pi) * mpmath.gamma(nu / 2))

    def tppf(q):
        if nu == 1:
            return -mpmath.cospi(q) / mpmath.sinpi(q)
        # Newton's iteration on the exact CDF from the binary64 quantile (relative error about 1e-15): three steps square
        # that to far below 40 digits
        t = mpmath.mpf(float(rv.ppf(float(q))))
        for _ in range(3):
            cdf = mpmath.mpf(1) / 2 + t * norm * mpmath.hyp2f1(mpmath.mpf(1) / 2, (nu + 1) / 2, mpmath.mpf(3) / 2, -t * t / nu)
            t = t - (cdf - q) / (norm * (1 + t * t / nu) ** (-(nu + 1) / 2))
        return t

    n, d = np.shape(u)
    x, s = np.empty((n, d)), np.empty(n)
    for r in range(n):
        tot = mpmath.mpf(0)
        for i in range(d):
            q = mpmath.mpf(float(u[r, i])) * mpmath.mpf(float(w[i])) + mpmath.mpf(float(lo[i]))
            t = tppf(q)
            x[r, i] = float(mpmath.mpf(float(ctr[i])) + mpmath.mpf(float(err[i])) * t)
            tot += lognorm - mpmath.log(mpmath.mpf(float(err[i]))) - (nu + 1) / 2 * mpmath.log1p(t * t / nu)
        s[r] = float(tot)
    return x, s, np.asarray(loglike_of_x(x)) - s


# ---- the contbox evidence of a separable Gaussian ----

def gauss_box_evidence(lo, hi, mu, sigma):
    """the integral of prod_i N(x_i; mu_i, sigma) over the box [lo, hi] (erf product)"""
    r2 = math.sqrt(2.0) * sigma
    z = 1.0
    for a, b, m in zip(lo, hi, mu):
        z *= 0.5 * (math.erf((b - m) / r2) - math.erf((a - m) / r2))
    return z


def contbox_log_evidence(ulos, uhis, xp, mu, sigma, order=16):
    """ln integral_0^1 Z_box(t) dt for the normalised separable Gaussian N(mu, sigma) with the identity transform: the box
    edges are linear in t on every segment of the knots, so Gauss-Legendre quadrature of `order` nodes per segment converges
    fast (the integrand is smooth inside a segment)."""
    nodes, wts = np.polynomial.legendre.leggauss(order)
    total = 0.0
    for j in range(len(xp) - 1):
        a, b = xp[j], xp[j + 1]
        for x, w in zip(nodes, wts):
            f = 0.5 * (x + 1.0)
            lo = ulos[j] + (ulos[j + 1] - ulos[j]) * f
            hi = uhis[j] + (uhis[j + 1] - uhis[j]) * f
            total += 0.5 * (b - a) * w * gauss_box_evidence(lo, hi, mu, sigma)
    return math.log(total)
