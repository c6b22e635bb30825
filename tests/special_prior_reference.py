"""High-precision reference of the iterative prior families (ultranest_amd.priors: Gamma, ChiSquared, InverseGamma, Beta,
StudentT, Dirichlet): the exact quantile from the binary64 u and the binary64 parameters in mpmath at 60 digits, the bound an
error is judged against, and the golden fixture that stores the references (a 60-digit root per point is too slow to recompute
in every test; tests/golden/make_special_priors.py writes it from this module).

Every quantile is found from the smaller tail q = min(u, 1 - u) (1 - u is exact for u >= 0.5) by Newton's iteration on
ln(tail) in the logarithm of the unknown, so that a root far below 2^-1074 is an ordinary number here.

Bounds (RTOL = 1e-12 is prior_reference's):

  Gamma, ChiSquared, InverseGamma   RTOL * |p| * (1 + |ln(p / unit)|) + 2^-1074, unit = scale (2 for ChiSquared): class E
                                    plus the spacing of subnormal results, which small shapes reach
  Beta                              m = min(p, 1 - p): RTOL * m * (1 + |ln m|) + (2^-53 if p > 0.5) + 2^-1074: relative in
                                    both tails; 2^-53 is the rounding of a result in [0.5, 1), which cannot hold 1 - p finer
  StudentT                          RTOL * (|loc| + scale * (1 + |t|)): class A
  Dirichlet                         g row: the Gamma bound with unit 1; p row: bit for bit against `dirichlet_restatement`
                                    from the device's own g row, and |sum p - 1| <= n 2^-52

Fixture format, per setting NAME: ``NAME/u`` (the grid; (rows, n) for a Dirichlet block), ``NAME/m`` (3, ...) and ``NAME/e``:
the reference is (m[0] + m[1] + m[2]) * 2^e, a three-term expansion of the mantissa (about 48 digits: a (hi, lo) pair of
doubles holds 32, which a tail probability with a logarithmic slope of 1000 turns into 1e-29, short of the round trip's 1e-30;
the separate exponent keeps roots below 2^-1022 exact too).  For Beta the stored number is min(p, 1 - p) and ``NAME/side`` says
whether p is 1 minus it.
"""
import os

import mpmath as mp
import numpy as np

from prior_reference import RTOL, grid as _closed_form_grid
from ultranest_amd import priors as P

DPS = 60
FIXTURE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "g17_special_priors.npz")
TINY = 2.0 ** -1074


def grid(seed=17):
    """the fixed points of prior_reference.grid (the extremes of (0, 1) and the three doubles around 0.25, 0.5 and 0.75) and
    64 seeded draws, sorted"""
    full = _closed_form_grid(1)
    fixed = np.setdiff1d(full, np.random.RandomState(1).uniform(size=512))
    u = np.unique(np.concatenate([fixed, np.random.RandomState(seed).uniform(size=64)]))
    assert len(fixed) == 18 and u[0] > 0 and u[-1] < 1
    return u


def block_grid(n, seed=17):
    """rows of a Dirichlet block: every fixed point of prior_reference.grid's extremes in all columns, then 8 seeded rows"""
    edge = [2.0 ** -1022, 1e-300, 1e-100, 1e-17, 2.0 ** -53, 1e-8, 0.01, 0.25, 0.5, 0.75, 1 - 1e-8, 1 - 2.0 ** -53]
    rows = [np.full(n, e) for e in edge]
    rows += list(np.random.RandomState(seed + n).uniform(size=(8, n)))
    return np.array(rows)


def dirichlet_alpha(n):
    return np.array([2.5]) if n == 1 else np.geomspace(0.1, 1000.0, n)


SETTINGS = {
    "Gamma_0": lambda: P.Gamma(0.1, 1.0), "Gamma_1": lambda: P.Gamma(2.5, 3.0), "Gamma_2": lambda: P.Gamma(1000.0, 0.01),
    "ChiSquared_0": lambda: P.ChiSquared(0.2), "ChiSquared_1": lambda: P.ChiSquared(5.0), "ChiSquared_2": lambda: P.ChiSquared(2000.0),
    "InverseGamma_0": lambda: P.InverseGamma(0.1, 1.0), "InverseGamma_1": lambda: P.InverseGamma(3.0, 2.0),
    "InverseGamma_2": lambda: P.InverseGamma(1000.0, 5.0),
    "Beta_0": lambda: P.Beta(0.1, 0.1), "Beta_1": lambda: P.Beta(0.5, 0.5), "Beta_2": lambda: P.Beta(1.0, 3.0),
    "Beta_3": lambda: P.Beta(2.5, 40.0), "Beta_4": lambda: P.Beta(30.0, 1000.0), "Beta_5": lambda: P.Beta(0.1, 1000.0),
    "StudentT_0": lambda: P.StudentT(1.0, 0.0, 1.0), "StudentT_1": lambda: P.StudentT(1.0, -3.0, 0.5),
    "StudentT_2": lambda: P.StudentT(2.5, 0.0, 1.0), "StudentT_3": lambda: P.StudentT(2.5, -3.0, 0.5),
    "StudentT_4": lambda: P.StudentT(30.0, 0.0, 1.0), "StudentT_5": lambda: P.StudentT(30.0, -3.0, 0.5),
    "StudentT_6": lambda: P.StudentT(1000.0, 0.0, 1.0), "StudentT_7": lambda: P.StudentT(1000.0, -3.0, 0.5),
    "Dirichlet_1": lambda: P.Dirichlet(dirichlet_alpha(1)), "Dirichlet_2": lambda: P.Dirichlet(dirichlet_alpha(2)),
    "Dirichlet_5": lambda: P.Dirichlet(dirichlet_alpha(5)), "Dirichlet_64": lambda: P.Dirichlet(dirichlet_alpha(64)),
}
FAMILY_NAMES = ("Gamma", "ChiSquared", "InverseGamma", "Beta", "StudentT", "Dirichlet")


def settings(family):
    return [k for k in sorted(SETTINGS, key=lambda s: (s.split("_")[0], int(s.split("_")[1]))) if k.split("_")[0] == family]


# ---- tails and roots in mpmath --------------------------------------------------------------------------------------------

def gamma_tail(a, x, upper):
    """P(a, x) or Q(a, x) of mpf arguments"""
    return mp.gammainc(a, x, mp.inf, regularized=True) if upper else mp.gammainc(a, 0, x, regularized=True)


def _newton(f_and_slope, t, tmax=None):
    tol = mp.mpf(10) ** (-DPS + 6)
    for _ in range(200):
        f, slope = f_and_slope(t)
        dt = f / slope
        lim = 8 + abs(t) / 2
        dt = max(min(dt, lim), -lim)
        tn = t - dt
        if tmax is not None and tn > tmax:
            tn = tmax
        dt, t = t - tn, tn
        if abs(dt) <= tol * (1 + abs(t)):
            return t
    raise RuntimeError("no convergence")


def gamma_lnx(a, q, upper):
    """t = ln x with P(a, x) = q or Q(a, x) = q (mpf in, mpf out)"""
    a, q = mp.mpf(a), mp.mpf(q)
    lnq, lga = mp.log(q), mp.loggamma(a)
    if not upper:
        t = (lnq + mp.loggamma(a + 1)) / a
    else:
        # from the right of the root: Q <= e^-x / Gamma(a) (a < 1, x >= 1); x = a + 2 sqrt(a) L + 2 L, L = -ln q, bounds a >= 1
        L = -lnq
        t = mp.log(max(1, L - lga)) if a < 1 else mp.log(a + 2 * mp.sqrt(a * L) + 2 * L)

    def fs(t):
        x = mp.exp(t)
        T = gamma_tail(a, x, upper)
        xpdf = mp.exp(a * t - x - lga)
        return mp.log(T) - lnq, (-xpdf if upper else xpdf) / T

    return _newton(fs, t)


def beta_cdf(a, b, x):
    return mp.betainc(a, b, 0, x, regularized=True)


def beta_lnxy(a, b, q):
    """(ln x, ln(1 - x)) with I_x(a, b) = q <= 0.5"""
    a, b, q = mp.mpf(a), mp.mpf(b), mp.mpf(q)
    lnq, lnB = mp.log(q), mp.log(mp.beta(a, b))
    half = mp.mpf(0.5)
    by_y = beta_cdf(a, b, half) < q
    if not by_y:
        def fs(t):
            x = mp.exp(t)
            I = beta_cdf(a, b, x)
            return mp.log(I) - lnq, mp.exp(a * t + (b - 1) * mp.log1p(-x) - lnB) / I
        t = min((lnq + mp.log(a) + lnB) / a, mp.log(half))
    else:
        def fs(t):
            s = mp.exp(t)
            I = beta_cdf(a, b, 1 - s)
            return mp.log(I) - lnq, -mp.exp((a - 1) * mp.log1p(-s) + b * t - lnB) / I
        t = mp.log(half)
    t = _newton(fs, t, tmax=mp.log(half))
    other = mp.log1p(-mp.exp(t))
    return (other, t) if by_y else (t, other)


def _smaller_tail(u):
    u = mp.mpf(float(u))
    return (1 - u, True) if u > mp.mpf(0.5) else (u, False)


def gamma_x(a, u, inverse=False):
    """the Gamma(a, 1) quantile of u, or with `inverse` the x of InverseGamma (Q(a, x) = u), as ln x"""
    q, upper = _smaller_tail(u)
    return gamma_lnx(a, q, upper != inverse)


def student_t(nu, u):
    q, flip = _smaller_tail(u)
    if 2 * q >= 1:
        return mp.mpf(0)
    if 2 * q <= mp.mpf(0.5):
        lx, ly = beta_lnxy(mp.mpf(nu) / 2, 0.5, 2 * q)
    else:
        ly, lx = beta_lnxy(0.5, mp.mpf(nu) / 2, 1 - 2 * q)
    t = mp.exp((mp.log(mp.mpf(nu)) + ly - lx) / 2)
    return t if flip else -t


def beta_m(a, b, u):
    """(min(p, 1 - p), whether p > 0.5) of Beta(a, b)"""
    q, flip = _smaller_tail(u)
    lx, ly = beta_lnxy(b, a, q)[::-1] if flip else beta_lnxy(a, b, q)
    return (mp.exp(lx), False) if lx <= ly else (mp.exp(ly), True)


def _one(prior, u):
    t = type(prior).__name__
    if t in ("Gamma", "ChiSquared"):
        return mp.mpf(prior.scale) * mp.exp(gamma_x(prior.shape, u))
    if t == "InverseGamma":
        return mp.mpf(prior.scale) * mp.exp(-gamma_x(prior.shape, u, inverse=True))
    if t == "StudentT":
        return mp.mpf(prior.loc) + mp.mpf(prior.scale) * student_t(prior.nu, u)
    raise ValueError("no reference for %s" % t)


def reference(prior, u):
    """exact quantiles of a one-column prior as a list of mpf (for Beta a list of (m, side)); for a Dirichlet block `u` is
    (rows, n) and the result the g rows, a list of lists"""
    with mp.workdps(DPS):
        if isinstance(prior, P.Dirichlet):
            return [[mp.exp(gamma_x(a, x)) for a, x in zip(prior.alpha, row)] for row in np.atleast_2d(u)]
        if isinstance(prior, P.Beta):
            return [beta_m(prior.a, prior.b, x) for x in np.ravel(u)]
        return [_one(prior, x) for x in np.ravel(u)]


# ---- the smaller tail's probability at a value: the round trip -------------------------------------------------------------

def tail_probability(prior, u, ref):
    """(the smaller tail's probability at the reference, the tail's probability from u), both mpf"""
    q, flip = _smaller_tail(u)
    t = type(prior).__name__
    if t in ("Gamma", "ChiSquared"):
        return gamma_tail(mp.mpf(prior.shape), ref / mp.mpf(prior.scale), flip), q
    if t == "InverseGamma":
        return gamma_tail(mp.mpf(prior.shape), mp.mpf(prior.scale) / ref, not flip), q
    if t == "Beta":
        m, side = ref
        a, b = mp.mpf(prior.a), mp.mpf(prior.b)
        if not flip:        # I_p(a, b) = u
            return (beta_cdf(a, b, 1 - m) if side else beta_cdf(a, b, m)), q
        return (beta_cdf(b, a, m) if side else beta_cdf(b, a, 1 - m)), q        # I_(1-p)(b, a) = 1 - u
    if t == "StudentT":
        z = (ref - mp.mpf(prior.loc)) / mp.mpf(prior.scale)
        nu = mp.mpf(prior.nu)
        if z == 0:
            return mp.mpf(0.5), q
        return beta_cdf(nu / 2, mp.mpf(0.5), nu / (nu + z * z)) / 2, q
    raise ValueError(t)


# ---- bounds ---------------------------------------------------------------------------------------------------------------

def bound(prior, ref):
    """the error bound at one reference value (mpf)"""
    t = type(prior).__name__
    tiny = mp.mpf(TINY)
    if t in ("Gamma", "ChiSquared", "InverseGamma", "Dirichlet"):
        unit = mp.mpf(1.0 if t == "Dirichlet" else prior.scale)
        return RTOL * abs(ref) * (1 + abs(mp.log(ref / unit))) + tiny
    if t == "Beta":
        m, side = ref
        return RTOL * m * (1 + abs(mp.log(m))) + (mp.mpf(2) ** -53 if side else 0) + tiny
    if t == "StudentT":
        loc, sc = mp.mpf(prior.loc), mp.mpf(prior.scale)
        return RTOL * (abs(loc) + sc * (1 + abs((ref - loc) / sc)))
    raise ValueError(t)


def value(prior, ref):
    """the reference as the number the device returns (mpf): p itself"""
    if isinstance(prior, P.Beta):
        return 1 - ref[0] if ref[1] else ref[0]
    return ref


def excess(prior, u, got, ref=None):
    """error / bound per value, a float array of got's shape (a non-finite `got` gives inf).  `ref` is what `reference` or
    `load` gives for this prior; for a Dirichlet block `got` is the g rows"""
    got = np.asarray(got, dtype=float)
    ref = reference(prior, u) if ref is None else ref
    flat = [r for row in ref for r in row] if isinstance(prior, P.Dirichlet) else list(ref)
    out = np.empty(got.size)
    with mp.workdps(DPS):
        for i, g in enumerate(got.ravel()):
            if not np.isfinite(g):
                out[i] = np.inf
                continue
            out[i] = float(abs(mp.mpf(float(g)) - value(prior, flat[i])) / bound(prior, flat[i]))
    return out.reshape(got.shape)


def accepts(prior, u, got, ref=None):
    return bool(excess(prior, u, got, ref).max() <= 1.0)


def dirichlet_restatement(g):
    """the block's sum and division in numpy, bit for bit, from the g rows (rows, n): ascending order, plain + and /; rows
    whose sum is 0 become 1 / n"""
    g = np.array(g, dtype=float)
    n = g.shape[1]
    s = g[:, 0].copy()
    for k in range(1, n):
        s = s + g[:, k]
    with np.errstate(all="ignore"):
        p = g / s[:, None]
    p[s == 0.0] = 1.0 / n
    return p


# ---- the host build of the device header (tests/special_prior_host.cpp) ---------------------------------------------------

HOST_SOURCE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "special_prior_host.cpp")
_LETTER = {"mlf_prior_gamma": "G", "mlf_prior_invgamma": "I", "mlf_prior_beta": "B", "mlf_prior_studentt": "T"}


def build_host(directory, name="host", flags=(), defines=()):
    """compiles the stand-alone program around the header's text (-O2 -ffp-contract=off) and returns its path"""
    import shutil
    import subprocess
    cxx = shutil.which("g++") or shutil.which("c++") or shutil.which("clang++")
    assert cxx, "no host C++ compiler"
    exe = os.path.join(str(directory), name)
    cmd = [cxx, "-std=c++17", "-O2", "-ffp-contract=off", '-DMLF_SPECIAL_HEADER="%s"' % P.SPECIAL_HEADER]
    cmd += ["-D%s" % d for d in defines] + list(flags) + [HOST_SOURCE, "-o", exe]
    subprocess.run(cmd, check=True, capture_output=True, text=True)
    return exe


def host_lines(prior, u):
    """the program's input for a one-column prior (or the Gamma columns of a Dirichlet block, u of shape (rows, n))"""
    if isinstance(prior, P.Dirichlet):
        cols = prior.gammas()
        return [line for row in np.atleast_2d(u) for g, x in zip(cols, row) for line in host_lines(g, [x])]
    return ["%s %s %s" % (_LETTER[prior.fn], float(x).hex(), " ".join(float(c).hex() for c in prior.consts)) for x in np.ravel(u)]


def run_host(exe, lines):
    """(results, steps per call, {family letter: largest step count}) of one run"""
    import subprocess
    out = subprocess.run([exe], input="\n".join(lines) + "\n", capture_output=True, text=True, check=True).stdout.split("\n")
    vals = [ln.split() for ln in out if ln and not ln.startswith("max")]
    most = {ln.split()[1]: int(ln.split()[2]) for ln in out if ln.startswith("max")}
    assert len(vals) == len(lines)
    return np.array([float.fromhex(v[0]) for v in vals]), np.array([int(v[1]) for v in vals]), most


# ---- the fixture ----------------------------------------------------------------------------------------------------------

def _split(x):
    """an mpf as (three doubles m0 + m1 + m2 of its mantissa, exponent e): x = (m0 + m1 + m2) 2^e"""
    if x == 0:
        return (0.0, 0.0, 0.0), 0
    man, e = mp.frexp(x)
    out = []
    for _ in range(3):
        d = float(man)
        out.append(d)
        man = man - mp.mpf(d)
    return tuple(out), int(e)


def _join(m, e):
    return mp.ldexp(mp.mpf(float(m[0])) + mp.mpf(float(m[1])) + mp.mpf(float(m[2])), int(e))


def pack(name, prior, u, ref):
    """the arrays of one setting for np.savez"""
    with mp.workdps(DPS):
        if isinstance(prior, P.Beta):
            side = np.array([s for _, s in ref], dtype=bool)
            vals = [m for m, _ in ref]
        elif isinstance(prior, P.Dirichlet):
            vals = [r for row in ref for r in row]
        else:
            vals = list(ref)
        parts = [_split(v) for v in vals]
    m = np.array([p[0] for p in parts]).T.reshape((3,) + np.shape(u))
    e = np.array([p[1] for p in parts], dtype=np.int64).reshape(np.shape(u))
    out = {name + "/u": np.asarray(u, dtype=float), name + "/m": m, name + "/e": e}
    if isinstance(prior, P.Beta):
        out[name + "/side"] = side
    return out


_loaded = {}


def load(name):
    """(prior, u, ref) of one setting from the fixture; ref as `reference` gives it"""
    if name not in _loaded:
        with np.load(FIXTURE) as z:
            u, m, e = z[name + "/u"], z[name + "/m"], z[name + "/e"]
            side = z[name + "/side"] if name + "/side" in z.files else None
        prior = SETTINGS[name]()
        with mp.workdps(DPS):
            flat = [_join(m.reshape(3, -1)[:, i], e.ravel()[i]) for i in range(e.size)]
        if side is not None:
            ref = [(v, bool(s)) for v, s in zip(flat, side)]
        elif isinstance(prior, P.Dirichlet):
            n = u.shape[1]
            ref = [flat[r * n:(r + 1) * n] for r in range(u.shape[0])]
        else:
            ref = flat
        _loaded[name] = (prior, u, ref)
    return _loaded[name]
