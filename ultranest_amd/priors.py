"""Prior library for device models: quantile transforms, closed-form, iterative, parameter-dependent and tabulated.

A prior transform maps the unit cube to the parameters, column by column, through each prior's quantile function (inverse
CDF).  In the reference users write it with ``scipy.stats.*.ppf`` inside ``transform``; a host callback keeps a model off every
device route.  Here a list of priors becomes an ordinary ``transform_source`` of ``ultranest_amd.devicemodel``, so every route
that serves a user model serves it unchanged::

    pt = PriorTransform([Uniform(-1, 1, name="x"), LogUniform(1e-3, 10, name="scale"), Normal(0, 2, name="offset"),
                         Sine(name="inclination")])
    model = pt.model(loglike_source)                  # a DeviceModel: model.transform / model.loglike on every device route
    StaticNestedSampler(pt.ndim, model.loglike, transform=model.transform, ...)
    p = pt.transform(u)                                # or the transform alone, for a likelihood that stays a host function

The device functions live in ``csrc/mlf_priors_dev.hpp`` (one ``__device__ __noinline__`` function per family); ``source`` is
that header's text followed by one generated call or statement per column, every constant a hexadecimal floating literal.  The
formulas are the interface.  ``u`` lies in the open interval (0, 1); ``1 - u`` is exact for ``u >= 0.5``::

    Fixed(v)                            v
    Uniform(lo, hi)                     lo + u * w,  w = hi - lo computed on the host in binary64
    LogUniform(lo, hi), 0 < lo < hi     exp(a + u * w),  a = log(lo), w = log(hi) - log(lo) from the host
    Normal(mu, sigma)                   z = u <= 0.5 ? normcdfinv(u) : -normcdfinv(1 - u);  mu + sigma * z
    TruncatedNormal(mu, sigma, lo, hi)  a, b = (lo - mu) / sigma, (hi - mu) / sigma;  Fa, Fb, Qa, Qb = Phi(a), Phi(b), Phi(-a),
                                        Phi(-b) from the host (0.5 * math.erfc(-+x / sqrt 2));  q = Fa + u * (Fb - Fa);
                                        q <= 0.5: z = normcdfinv(q), else z = -normcdfinv(Qb + (1 - u) * (Qa - Qb));
                                        z clamped to [a, b];  mu + sigma * z
    LogNormal(mu, sigma)                exp(mu + sigma * z), z as for Normal
    HalfNormal(sigma)                   u <= 0.5: sigma * (sqrt2 * erfinv(u)), else sigma * -normcdfinv(0.5 * (1 - u))
    Exponential(scale)                  scale * -log1p(-u)
    Rayleigh(sigma)                     sigma * sqrt(-2 * log1p(-u))
    Weibull(scale, k)                   scale * exp(log(-log1p(-u)) / k)
    Pareto(xm, alpha)                   xm * exp(-log1p(-u) / alpha)
    Cauchy(loc, scale)                  loc + scale * (-cospi(u) / sinpi(u))
    HalfCauchy(scale)                   scale * (sinpi(0.5 * u) / cospi(0.5 * u))
    Laplace(loc, b)                     u <= 0.5: loc + b * log(2 u), else loc - b * log(2 * (1 - u))
    Logistic(loc, s)                    loc + s * (log(u) - log1p(-u))
    Gumbel(loc, s)                      loc - s * log(-log(u))
    Triangular(lo, mode, hi)            u <= c: lo + sqrt(u * c1), else hi - sqrt((1 - u) * c2);  c = (mode - lo) / (hi - lo),
                                        c1 = (hi - lo) * (mode - lo), c2 = (hi - lo) * (hi - mode) from the host
    Sine()    density ~ sin on [0, pi]           2 * atan2(sqrt(u), sqrt(1 - u))           (= 2 asin(sqrt u))
    Cosine()  density ~ cos on [-pi/2, pi/2]     atan2(2 u - 1, 2 * sqrt(u * (1 - u)))     (= asin(2 u - 1))

(Sine and Cosine go through atan2 because asin has an infinite slope at +-1, exactly where ``sqrt(u)`` for u -> 1 and
``2 u - 1`` for u -> 0 have rounded away their distance from +-1; the atan2 arguments keep their relative accuracy in both
tails.)

Two block priors span several consecutive columns:

``MultivariateNormal(mean, cov)``, block size n <= 64: ``L = np.linalg.cholesky(cov)`` on the host; the generated code writes
``z_k`` (the Normal(0, 1) form) into ``p[k]`` for every column of the block, then for i = n-1 down to 0
``p[i] = mean_i + (((L_i0 * p[0]) + L_i1 * p[1]) + ... + L_ii * p[i])``: straight-line code in ascending j with plain ``*``
and ``+`` (no FMA is formed), so numpy restates it bit for bit from the z row; no table lives in the program's data section.

``OrderedUniform(lo, hi, n)``, an ascending vector (the order statistics of n uniform draws):
``t_(n-1) = exp(log(u_(n-1)) / n)``, ``t_k = t_(k+1) * exp(log(u_k) / (k + 1))`` for k = n-2 down to 0, ``p_k = lo + t_k * w``.

Gamma, beta, Student-t and Dirichlet priors need inverse incomplete gamma / beta functions, which have no closed form.  Their
device functions are iterative and live in a second header, ``csrc/mlf_priors_special_dev.hpp``, whose text follows the first
one's in ``source`` only when the list holds one of these families (a closed-form list gives exactly the text it always gave).
Every function works from the smaller tail q = min(u, 1 - u) and runs Newton's iteration on ln(tail) in the logarithm of the
unknown, with a compile-time cap on every loop (48 steps, 3000 terms); P, Q are the regularized incomplete gamma functions,
I_x(a, b) the regularized incomplete beta function::

    Gamma(shape, scale=1)               scale * x;  P(shape, x) = u for u <= 0.5, Q(shape, x) = 1 - u otherwise
    ChiSquared(k)                       Gamma(k / 2, 2): the same device function
    InverseGamma(shape, scale=1)        scale / x;  Q(shape, x) = u for u <= 0.5, P(shape, x) = 1 - u otherwise
    Beta(a, b)  on (0, 1)               x with I_x(a, b) = u, solved for the smaller of x and y = 1 - x, returned as x or 1 - y
    StudentT(nu, loc=0, scale=1)        loc + scale * t;  t = -sqrt(nu y / x) from x = nu / (nu + t^2) with I_x(nu/2, 1/2) = 2 q,
                                        carried as ln x and ln y; the sign is flipped for u > 0.5 (StudentT(nu, 0, 1) is odd bit
                                        for bit), t = 0 at u = 0.5
    Dirichlet(alpha), block n <= 64     g_k = the Gamma(alpha_k, 1) quantile of u_k into p[k];  s = ((g_0 + g_1) + ...) + g_(n-1)
                                        in ascending order with plain +;  p[k] = g_k / s, or 1 / n for every k if s == 0

Accepted ranges (the ranges over which each quantile is held to 1e-12 * S against 60-digit references from u = 2^-1022 to
1 - 2^-53; outside them the constructor raises ``ValueError``): shape, a, b and every alpha_k in [0.1, 1000], k in [0.2, 2000],
nu in [1, 1000]; scale > 0, loc finite.  ``lgamma(shape + 1)``, ``ln B(a, b)``, ``1 / shape`` and the logarithms of the
parameters are computed here in binary64 and passed as hexadecimal literals.  The columns of a Dirichlet block sum to 1, so no
ellipsoid in parameter space has a volume: a driver's t-region cannot be built over it and the drivers run without one, as the
reference does.  An iterative quantile costs several times a ``normcdfinv`` (DESIGN.md 7f has the measurement).

Every prior validates its parameters at construction (``ValueError`` before anything is compiled) and takes an optional
``name``.  ``Uniform(..., circular=True)`` marks a periodic parameter (``PriorTransform.wrapped_dims``).

Parameters that are other parameters: ``Ref``
---------------------------------------------
``Ref(target, scale=1.0, offset=0.0)`` in place of a number makes a prior's parameter the value of another column of the same
row, ``scale * p[j] + offset`` (plain ``*`` and ``+``, hexadecimal ``scale`` and ``offset``; just ``p[j]`` for scale 1 and
offset 0).  `target` is a name of ``paramnames`` (``name_k`` for a column of a block) or a column index::

    PriorTransform([Normal(0.0, 10.0, name="mu"), LogUniform(0.01, 10.0, name="tau"),
                    Normal(Ref("mu"), Ref("tau"), name="theta0"), TruncatedNormal(Ref("mu"), Ref("tau"), -50.0, 50.0, name="theta1"),
                    Uniform(Ref("theta1"), 60.0, name="upper"), Normal(0.0, Ref("tau", scale=2.0, offset=0.1))])

A ``Ref`` is taken by: ``Uniform`` lo, hi (not with ``circular=True``: the period would vary); ``LogUniform`` lo, hi; ``Normal``,
``LogNormal`` mu, sigma; ``TruncatedNormal`` mu, sigma, lo, hi; the scale of ``HalfNormal``, ``Exponential``, ``Rayleigh``,
``HalfCauchy``; ``Weibull`` scale, k; ``Pareto`` xm, alpha; loc and scale of ``Cauchy``, ``Laplace``, ``Logistic``, ``Gumbel``;
``Triangular`` lo, mode, hi; the **scale** of ``Gamma`` and ``InverseGamma``; **loc and scale** of ``StudentT``.  The shapes of
the iterative families (shape, k, a, b, nu, alpha: their lgamma and ln B constants come from the host, and their error bounds
hold over a stated range), every parameter of the three block priors, ``Tabulated`` and ``Fixed`` stay constants (a ``Ref``
there is a ``ValueError``); blocks and tables may be targets.

Order.  Column j still consumes u[j]; the statements are written in dependency order, a stable topological sort with ties in
list order (``PriorTransform.order``; ``PriorTransform.parents[j]`` are the columns that column j reads).  A cycle, a
self-reference, an unknown target and a referenced name that occurs twice are ``ValueError``s.

Support check.  Every column has a support, a closed interval of the extended reals (``PriorTransform.supports``): ``Fixed``
[v, v]; ``Uniform``, ``LogUniform``, ``TruncatedNormal``, ``Triangular``, ``OrderedUniform``: their bounds; ``Sine`` [0, pi];
``Cosine`` [-pi/2, pi/2]; ``Beta``, ``Dirichlet`` [0, 1]; ``Pareto`` [xm, inf); the positive families [0, inf); ``Tabulated``
[x_0, x_(n-1)]; everything else the real line; a ``Ref`` maps its target's support affinely, and a prior with ``Ref`` bounds
takes the hull.  A ``Ref`` in a scale-like or strictly positive parameter needs a mapped support with infimum >= 0, and for an
ordered pair (lo / hi, lo / mode / hi) sup(support(lo)) <= inf(support(hi)) must hold; otherwise ``ValueError`` names the
parameter and the target's support (``Normal(0, Ref("mu"))`` with mu ~ Normal is refused, and so is ``Uniform(Ref("x"), 20)``
over an unbounded x).

Run-time contract.  What the support check cannot exclude is a value that rounded to 0 or overflowed to inf, or the NaN of a
parent.  A scale-like parameter must be >= 0 and finite (0 gives the point mass at loc); a strictly positive parameter
(``Weibull`` k, ``Pareto`` xm and alpha, ``LogUniform`` bounds, ``TruncatedNormal`` sigma) must be > 0 and finite; a location must
be finite; bounds must be ordered (equal ``Uniform`` or ``LogUniform`` bounds give the point mass; ``Triangular`` needs lo < hi,
``TruncatedNormal`` some probability between its bounds in binary64).  If any of these fails the column is NaN, and so is every
column that depends on it.  The likelihood is still called; a NaN L fails ``L > Lmin``, so such a row is never kept, harvested
or accepted by any route.

Device code (``csrc/mlf_priors_rt_dev.hpp``, appended to ``source`` after the other header(s) only when the list holds a ``Ref``
or a ``Tabulated``: every other list gives exactly the text it always gave).  Pass-through families call the existing
``mlf_prior_*`` function with each run-time argument wrapped in a guard that returns the value or NaN (``mlf_prior_rt_loc``,
``_scale``, ``_pos``): with ``Fixed`` parents such a column is bit for bit the constant-parameter column.  Four families take
constants that the host computes for constants; with a ``Ref`` the device evaluates the same expressions::

    Uniform          lo + u * (hi - lo)                                      (numpy restates it bit for bit)
    LogUniform       a = log(lo);  exp(a + u * (log(hi) - a))
    TruncatedNormal  a, b, Fa, Fb, Qa, Qb from 0.5 * erfc(-+x / sqrt2) on the device, then the constant form's two-tail formula
                     and clamp; NaN if neither Fb > Fa nor Qa > Qb
    Triangular       w = hi - lo, c = (mode - lo) / w, c1 = w * (mode - lo), c2 = w * (hi - mode), then the constant form

``is_affine`` is False for a list that holds a ``Ref``.

Quantile functions given as numbers: ``Tabulated``
--------------------------------------------------
::

    Tabulated(x, cdf)                          knots of the CDF: F(x_k) = cdf_k, linear in between
    Tabulated.from_samples(samples)            sorted samples, cdf_k = k / (m - 1) in binary64 (np.quantile's "linear" rule)
    Tabulated.from_histogram(edges, density)   piecewise-constant density; the CDF normalised, its ends pinned to 0.0 and 1.0

2 <= n <= 4096 knots, at most 16 384 over all tables of one transform; everything finite; x non-decreasing with
x[0] < x[-1] (a repeated x is a point mass); cdf non-decreasing from exactly 0.0 to exactly 1.0 (a repeated cdf is a gap in the
support); every slope finite; more than 4096 samples are refused with the advice to pass quantile knots.  Weighted samples: pass
``x, cdf``.  The host computes the slopes in binary64, s_k = (x_(k+1) - x_k) / (c_(k+1) - c_k), 0 on a flat CDF segment, and the
table goes into ``source`` as one ``static __device__ const double`` array per prior, ``[c | x | s]`` in hexadecimal literals.
The formula is the interface: k = the largest index <= n - 2 with c_k <= u (a branch-free bisection of ceil(log2(n - 1)) probes),
dl = u - c_k, dr = c_(k+1) - u, ``p = dl <= dr ? x_k + dl * s_k : x_(k+1) - dr * s_k``: only +, -, * and comparisons, so numpy
restates it bit for bit; it is monotone in u, stays within [x_0, x_(n-1)] and lies within
2^-52 |p| + 3 * 2^-53 |x_(k+1) - x_k| of the exact piecewise-linear inverse of the binary64 table (tests/prior_rt_reference.py
derives the bound).  Every load stays inside the table for every u.
"""
import math
import os

import numpy as np

from . import devicemodel
from .devicemodel import DeviceModel

HEADER = os.path.join(devicemodel.INCLUDE_DIR, "mlf_priors_dev.hpp")
SPECIAL_HEADER = os.path.join(devicemodel.INCLUDE_DIR, "mlf_priors_special_dev.hpp")
MAX_BLOCK = 64          # largest MultivariateNormal or Dirichlet block (straight-line code)
SHAPE_MIN, SHAPE_MAX = 0.1, 1000.0      # Gamma / InverseGamma shape, Beta a and b, Dirichlet alpha_k; ChiSquared k is twice it
NU_MIN, NU_MAX = 1.0, 1000.0            # StudentT degrees of freedom
RT_HEADER = os.path.join(devicemodel.INCLUDE_DIR, "mlf_priors_rt_dev.hpp")
MAX_KNOTS = 4096            # knots of one Tabulated
MAX_TABLE_KNOTS = 16384     # knots of all tables of one transform

CONSTANT_LOGLIKE = r"""
__device__ double mlf_user_loglike(const double *p, int d, const double *aux, long long naux) {
  return 0.0;
}
"""


def _hex(x):
    """a binary64 value as a C++17 hexadecimal floating literal (exact, and a function of the value's bits alone)"""
    return float(x).hex()


def _finite(owner, **values):
    out = []
    for key, v in values.items():
        try:
            v = float(v)
        except (TypeError, ValueError):
            raise ValueError("%s: %s must be a number, got %r" % (owner, key, v))
        if not math.isfinite(v):
            raise ValueError("%s: %s must be finite, got %r" % (owner, key, v))
        out.append(v)
    return out


def _positive(owner, **values):
    out = _finite(owner, **values)
    for (key, _), v in zip(values.items(), out):
        if v <= 0:
            raise ValueError("%s: %s must be positive, got %r" % (owner, key, v))
    return out


def _ordered(owner, lo, hi):
    if hi <= lo:
        raise ValueError("%s: hi must be larger than lo, got lo = %r, hi = %r" % (owner, lo, hi))


class Ref(object):
    """A prior parameter that is another column of the row: ``scale * p[j] + offset`` (module docstring).  `target` is a
    column name of ``PriorTransform.paramnames`` or a column index; it is resolved when the list becomes a PriorTransform."""

    def __init__(self, target, scale=1.0, offset=0.0):
        if isinstance(target, bool) or not isinstance(target, (str, int, np.integer)):
            raise ValueError("Ref: target must be a column name or a column index, got %r" % (target,))
        self.target = target if isinstance(target, str) else int(target)
        self.scale, self.offset = _finite("Ref", scale=scale, offset=offset)
        if self.scale == 0:
            raise ValueError("Ref: scale must not be 0 (a constant parameter is written as a number)")

    def __repr__(self):
        return "Ref(%r, scale=%r, offset=%r)" % (self.target, self.scale, self.offset)

    def expr(self, j):
        """the C++ expression of the value from column j: plain * and +, hexadecimal constants"""
        if self.scale == 1.0 and self.offset == 0.0:
            return "p[%d]" % j
        return "(%s * p[%d] + %s)" % (_hex(self.scale), j, _hex(self.offset))

    def value(self, pj):
        """the same expression in numpy (bit for bit: one product, one sum)"""
        if self.scale == 1.0 and self.offset == 0.0:
            return pj
        return self.scale * pj + self.offset

    def map(self, lo, hi):
        """the image of the closed interval [lo, hi] of the extended reals"""
        a, b = self.scale * lo + self.offset, self.scale * hi + self.offset
        return (a, b) if self.scale > 0 else (b, a)


_REAL_LINE = (-math.inf, math.inf)
_POSITIVE = (0.0, math.inf)
_GUARD = {"loc": "mlf_prior_rt_loc", "scale": "mlf_prior_rt_scale", "pos": "mlf_prior_rt_pos"}


class Prior(object):
    """One column (``size == 1``) or one block of consecutive columns of a prior transform.

    ``refs`` maps the attribute of a parameter given as a ``Ref`` to ``(ref, kind, label)``, kind one of "loc" (finite),
    "scale" (>= 0 and finite) and "pos" (> 0 and finite); ``ordered`` names the attributes that must ascend; ``support`` is the
    closed interval of the extended reals that holds every value of the column."""
    size = 1
    affine = False
    circular = False
    ordered = ()
    base_support = _REAL_LINE

    def __init__(self, name=None):
        self.name = name
        self.refs = {}

    def names(self, first):
        base = self.name or "p%d" % first
        return [base] if self.size == 1 else ["%s_%d" % (base, k) for k in range(self.size)]

    def call(self, u, cols=None):
        """the C++ expression of a one-column prior from the expression `u`; `cols` maps the attribute of every ``Ref``
        parameter to the column it reads"""
        raise NotImplementedError

    def statements(self, first, cols=None):
        """the C++ statements that write p[first .. first + size)"""
        return ["p[%d] = %s;" % (first, self.call("u[%d]" % first, cols))]

    def _call(self, fn, u, *consts):
        return "%s(%s)" % (fn, ", ".join((u,) + tuple(_hex(c) for c in consts)))

    def _par(self, kind, attr, v, label=None):
        """a parameter that may be a Ref: a constant is validated as it always was"""
        label = label or attr
        if isinstance(v, Ref):
            self.refs[attr] = (v, kind, label)
            return v
        check = _finite if kind == "loc" else _positive
        return check(type(self).__name__, **{label: v})[0]

    def _const(self, attr, v, label=None):
        """a parameter that stays a constant"""
        if isinstance(v, Ref):
            raise ValueError("%s: %s must be a constant, not a Ref" % (type(self).__name__, label or attr))
        return v

    def _arg(self, attr, cols, guard=True):
        """the C++ expression of one parameter of a call with run-time arguments"""
        if attr not in self.refs:
            return _hex(getattr(self, attr))
        ref, kind, _ = self.refs[attr]
        e = ref.expr(cols[attr])
        return "%s(%s)" % (_GUARD[kind], e) if guard else e

    def _rt_call(self, fn, u, cols, attrs, guard=True):
        return "%s(%s)" % (fn, ", ".join([u] + [self._arg(a, cols, guard) for a in attrs]))

    def interval(self, attr, cols, supports):
        """the interval that holds a parameter: [v, v] of a constant, the mapped support of a Ref's target"""
        if attr in self.refs:
            return self.refs[attr][0].map(*supports[cols[attr]])
        v = getattr(self, attr)
        return (v, v)

    def check_refs(self, cols, supports, names):
        """the support check of the module docstring: ValueError naming the parameter and the target's support"""
        owner = type(self).__name__

        def describe(attr):
            ref, _, label = self.refs[attr]
            j = cols[attr]
            return "%s = %r reads column %d (%s) with support [%r, %r]" % ((label, ref, j, names[j]) + tuple(supports[j]))

        for attr, (ref, kind, label) in self.refs.items():
            lo, hi = self.interval(attr, cols, supports)
            if kind in ("scale", "pos") and not lo >= 0:
                raise ValueError("%s: %s, so the parameter is not bounded below by 0" % (owner, describe(attr)))
        for i, a in enumerate(self.ordered):
            for b in self.ordered[i + 1:]:
                if a in self.refs or b in self.refs:
                    sup, inf = self.interval(a, cols, supports)[1], self.interval(b, cols, supports)[0]
                    if not sup <= inf:
                        raise ValueError("%s: %s <= %s cannot be guaranteed (sup %r, inf %r): %s" % (
                            owner, self.refs.get(a, (0, 0, a))[2], self.refs.get(b, (0, 0, b))[2], sup, inf,
                            "; ".join(describe(x) for x in (a, b) if x in self.refs)))

    def support(self, cols=None, supports=None):
        """(lo, hi): the interval that holds every value of the column (of each column of a block prior)"""
        return self.base_support


class Fixed(Prior):
    affine = True

    def __init__(self, v, name=None):
        Prior.__init__(self, name)
        self.v, = _finite("Fixed", v=self._const("v", v))

    def call(self, u, cols=None):
        return _hex(self.v)

    def support(self, cols=None, supports=None):
        return (self.v, self.v)


class _Bounded(Prior):
    """a family on [lo, hi]: the support is the hull of the two parameters' intervals"""
    ordered = ("lo", "hi")

    def support(self, cols=None, supports=None):
        return (self.interval("lo", cols, supports)[0], self.interval("hi", cols, supports)[1])


class Uniform(_Bounded):
    affine = True

    def __init__(self, lo, hi, circular=False, name=None):
        Prior.__init__(self, name)
        self.lo, self.hi = self._par("loc", "lo", lo), self._par("loc", "hi", hi)
        self.circular = bool(circular)
        if self.refs:
            self.affine = False
            if self.circular:
                raise ValueError("Uniform: a circular parameter needs constant bounds (the period would vary with a Ref)")
            return
        _ordered("Uniform", self.lo, self.hi)
        self.w, = _finite("Uniform", width=self.hi - self.lo)

    def call(self, u, cols=None):
        if self.refs:
            return self._rt_call("mlf_prior_rt_uniform", u, cols, ("lo", "hi"), guard=False)
        return self._call("mlf_prior_uniform", u, self.lo, self.w)


class LogUniform(_Bounded):
    def __init__(self, lo, hi, name=None):
        Prior.__init__(self, name)
        self.lo, self.hi = self._par("pos", "lo", lo), self._par("pos", "hi", hi)
        if self.refs:
            return
        _ordered("LogUniform", self.lo, self.hi)
        self.a = math.log(self.lo)
        self.w = math.log(self.hi) - math.log(self.lo)

    def call(self, u, cols=None):
        if self.refs:
            return self._rt_call("mlf_prior_rt_loguniform", u, cols, ("lo", "hi"), guard=False)
        return self._call("mlf_prior_loguniform", u, self.a, self.w)


class Normal(Prior):
    def __init__(self, mu, sigma, name=None):
        Prior.__init__(self, name)
        self.mu = self._par("loc", "mu", mu)
        self.sigma = self._par("scale", "sigma", sigma)

    def call(self, u, cols=None):
        if self.refs:
            return self._rt_call("mlf_prior_normal", u, cols, ("mu", "sigma"))
        return self._call("mlf_prior_normal", u, self.mu, self.sigma)


class TruncatedNormal(_Bounded):
    def __init__(self, mu, sigma, lo, hi, name=None):
        Prior.__init__(self, name)
        self.mu, self.lo, self.hi = self._par("loc", "mu", mu), self._par("loc", "lo", lo), self._par("loc", "hi", hi)
        self.sigma = self._par("pos", "sigma", sigma)
        if self.refs:
            if "lo" not in self.refs and "hi" not in self.refs:
                _ordered("TruncatedNormal", self.lo, self.hi)
            return
        _ordered("TruncatedNormal", self.lo, self.hi)
        self.a, self.b = (self.lo - self.mu) / self.sigma, (self.hi - self.mu) / self.sigma
        r2 = math.sqrt(2.0)
        self.Fa, self.Fb = 0.5 * math.erfc(-self.a / r2), 0.5 * math.erfc(-self.b / r2)
        self.Qa, self.Qb = 0.5 * math.erfc(self.a / r2), 0.5 * math.erfc(self.b / r2)
        if not (self.Fb > self.Fa or self.Qa > self.Qb):
            raise ValueError("TruncatedNormal: no probability between lo = %r and hi = %r in binary64" % (self.lo, self.hi))

    def call(self, u, cols=None):
        if self.refs:
            return self._rt_call("mlf_prior_rt_truncnormal", u, cols, ("mu", "sigma", "lo", "hi"), guard=False)
        return self._call("mlf_prior_truncnormal", u, self.mu, self.sigma, self.a, self.b, self.Fa, self.Fb, self.Qa, self.Qb)


class LogNormal(Prior):
    base_support = _POSITIVE

    def __init__(self, mu, sigma, name=None):
        Prior.__init__(self, name)
        self.mu = self._par("loc", "mu", mu)
        self.sigma = self._par("scale", "sigma", sigma)

    def call(self, u, cols=None):
        if self.refs:
            return self._rt_call("mlf_prior_lognormal", u, cols, ("mu", "sigma"))
        return self._call("mlf_prior_lognormal", u, self.mu, self.sigma)


class _OneScale(Prior):
    fn, key = None, "scale"
    base_support = _POSITIVE

    def __init__(self, scale, name=None):
        Prior.__init__(self, name)
        self.scale = self._par("scale", "scale", scale, self.key)

    def call(self, u, cols=None):
        if self.refs:
            return self._rt_call(self.fn, u, cols, ("scale",))
        return self._call(self.fn, u, self.scale)


class HalfNormal(_OneScale):
    fn, key = "mlf_prior_halfnormal", "sigma"


class Exponential(_OneScale):
    fn = "mlf_prior_exponential"


class Rayleigh(_OneScale):
    fn, key = "mlf_prior_rayleigh", "sigma"


class HalfCauchy(_OneScale):
    fn = "mlf_prior_halfcauchy"


class _ScaleShape(Prior):
    fn, keys, scale_kind = None, ("scale", "shape"), "scale"
    base_support = _POSITIVE

    def __init__(self, scale, shape, name=None):
        Prior.__init__(self, name)
        self.scale = self._par(self.scale_kind, "scale", scale, self.keys[0])
        self.shape = self._par("pos", "shape", shape, self.keys[1])

    def call(self, u, cols=None):
        if self.refs:
            return self._rt_call(self.fn, u, cols, ("scale", "shape"))
        return self._call(self.fn, u, self.scale, self.shape)


class Weibull(_ScaleShape):
    fn, keys = "mlf_prior_weibull", ("scale", "k")


class Pareto(_ScaleShape):
    fn, keys, scale_kind = "mlf_prior_pareto", ("xm", "alpha"), "pos"

    def support(self, cols=None, supports=None):
        return (self.interval("scale", cols, supports)[0], math.inf)


class _LocScale(Prior):
    fn, key = None, "scale"

    def __init__(self, loc, scale, name=None):
        Prior.__init__(self, name)
        self.loc = self._par("loc", "loc", loc)
        self.scale = self._par("scale", "scale", scale, self.key)

    def call(self, u, cols=None):
        if self.refs:
            return self._rt_call(self.fn, u, cols, ("loc", "scale"))
        return self._call(self.fn, u, self.loc, self.scale)


class Cauchy(_LocScale):
    fn = "mlf_prior_cauchy"


class Laplace(_LocScale):
    fn, key = "mlf_prior_laplace", "b"


class Logistic(_LocScale):
    fn, key = "mlf_prior_logistic", "s"


class Gumbel(_LocScale):
    fn, key = "mlf_prior_gumbel", "s"


class Triangular(_Bounded):
    ordered = ("lo", "mode", "hi")

    def __init__(self, lo, mode, hi, name=None):
        Prior.__init__(self, name)
        self.lo, self.mode, self.hi = self._par("loc", "lo", lo), self._par("loc", "mode", mode), self._par("loc", "hi", hi)
        if self.refs:
            consts = [getattr(self, a) for a in self.ordered if a not in self.refs]
            if consts != sorted(consts):
                raise ValueError("Triangular: lo <= mode <= hi must hold, got %r" % (consts,))
            return
        _ordered("Triangular", self.lo, self.hi)
        if not self.lo <= self.mode <= self.hi:
            raise ValueError("Triangular: mode must lie in [lo, hi], got %r" % (self.mode,))
        w = self.hi - self.lo
        self.c = (self.mode - self.lo) / w
        self.c1, self.c2 = _finite("Triangular", c1=w * (self.mode - self.lo), c2=w * (self.hi - self.mode))

    def call(self, u, cols=None):
        if self.refs:
            return self._rt_call("mlf_prior_rt_triangular", u, cols, ("lo", "mode", "hi"), guard=False)
        return self._call("mlf_prior_triangular", u, self.lo, self.hi, self.c, self.c1, self.c2)


class Sine(Prior):
    base_support = (0.0, math.pi)

    def call(self, u, cols=None):
        return "mlf_prior_sine(%s)" % u


class Cosine(Prior):
    base_support = (-0.5 * math.pi, 0.5 * math.pi)

    def call(self, u, cols=None):
        return "mlf_prior_cosine(%s)" % u


class MultivariateNormal(Prior):
    def __init__(self, mean, cov, name=None):
        Prior.__init__(self, name)
        try:
            mean, cov = np.array(mean, dtype=float), np.array(cov, dtype=float)
        except (TypeError, ValueError):
            raise ValueError("MultivariateNormal: mean and cov must be arrays of numbers")
        if mean.ndim != 1 or not 1 <= len(mean) <= MAX_BLOCK:
            raise ValueError("MultivariateNormal: mean must be a vector of 1 to %d entries, got shape %s" % (MAX_BLOCK, mean.shape))
        if cov.shape != (len(mean), len(mean)):
            raise ValueError("MultivariateNormal: cov must be %d x %d, got shape %s" % (len(mean), len(mean), cov.shape))
        if not (np.isfinite(mean).all() and np.isfinite(cov).all()):
            raise ValueError("MultivariateNormal: mean and cov must be finite")
        if not np.array_equal(cov, cov.T):
            raise ValueError("MultivariateNormal: cov must be symmetric")
        try:
            L = np.linalg.cholesky(cov)
        except np.linalg.LinAlgError:
            raise ValueError("MultivariateNormal: cov is not positive definite")
        if not (np.isfinite(L).all() and (np.diag(L) > 0).all()):
            raise ValueError("MultivariateNormal: cov is not positive definite")
        self.mean, self.cov, self.L = mean, cov, np.tril(L)
        self.size = len(mean)

    def statements(self, first, cols=None):
        n = self.size
        out = ["p[%d] = mlf_prior_z(u[%d]);" % (first + k, first + k) for k in range(n)]
        for i in range(n - 1, -1, -1):      # row i reads z_0 .. z_i only: descending rows may overwrite in place
            s = "%s * p[%d]" % (_hex(self.L[i, 0]), first)
            for j in range(1, i + 1):
                s = "(%s) + %s * p[%d]" % (s, _hex(self.L[i, j]), first + j)
            out.append("p[%d] = %s + (%s);" % (first + i, _hex(self.mean[i]), s))
        return out


class OrderedUniform(Prior):
    def support(self, cols=None, supports=None):
        return (self.lo, self.hi)

    def __init__(self, lo, hi, n, name=None):
        Prior.__init__(self, name)
        self.lo, self.hi = _finite("OrderedUniform", lo=lo, hi=hi)
        _ordered("OrderedUniform", self.lo, self.hi)
        self.w, = _finite("OrderedUniform", width=self.hi - self.lo)
        if isinstance(n, bool) or not isinstance(n, (int, np.integer)) or n < 1:
            raise ValueError("OrderedUniform: n must be a positive integer, got %r" % (n,))
        self.size = int(n)

    def statements(self, first, cols=None):
        n = self.size
        out = ["{", "  double t = mlf_prior_ordered_factor(u[%d], %s);" % (first + n - 1, _hex(n)),
               "  p[%d] = %s + t * %s;" % (first + n - 1, _hex(self.lo), _hex(self.w))]
        for k in range(n - 2, -1, -1):
            out.append("  t = t * mlf_prior_ordered_factor(u[%d], %s);" % (first + k, _hex(k + 1)))
            out.append("  p[%d] = %s + t * %s;" % (first + k, _hex(self.lo), _hex(self.w)))
        out.append("}")
        return out


def _in_range(owner, lo, hi, **values):
    out = _finite(owner, **values)
    for (key, _), v in zip(values.items(), out):
        if not lo <= v <= hi:
            raise ValueError("%s: %s must lie in [%g, %g] (the range over which the device quantile holds its error bound), "
                             "got %r" % (owner, key, lo, hi, v))
    return out


def _lbeta(a, b):
    return math.lgamma(a) + math.lgamma(b) - math.lgamma(a + b)


class _Special(Prior):
    """a family whose quantile is iterative (``csrc/mlf_priors_special_dev.hpp``): ``fn`` and ``consts``, the device function
    and the constants it takes after u"""
    special = True
    fn, consts = None, ()
    rt_attrs = ()       # the attributes behind the leading entries of `consts` that may be a Ref

    def call(self, u, cols=None):
        if self.refs:
            head = [self._arg(a, cols) for a in self.rt_attrs]
            return "%s(%s)" % (self.fn, ", ".join([u] + head + [_hex(c) for c in self.consts[len(head):]]))
        return self._call(self.fn, u, *self.consts)


def _gamma_consts(scale, a):
    return (scale, a, 1.0 / a, math.log(a), math.lgamma(a + 1.0))


class Gamma(_Special):
    fn, rt_attrs, base_support = "mlf_prior_gamma", ("scale",), _POSITIVE

    def __init__(self, shape, scale=1.0, name=None):
        Prior.__init__(self, name)
        self.shape, = _in_range("Gamma", SHAPE_MIN, SHAPE_MAX, shape=shape)
        self.scale = self._par("scale", "scale", scale)
        self.consts = _gamma_consts(self.scale, self.shape)


class ChiSquared(_Special):
    fn, base_support = "mlf_prior_gamma", _POSITIVE

    def __init__(self, k, name=None):
        Prior.__init__(self, name)
        self.k, = _in_range("ChiSquared", 2.0 * SHAPE_MIN, 2.0 * SHAPE_MAX, k=k)
        self.shape, self.scale = 0.5 * self.k, 2.0
        self.consts = _gamma_consts(self.scale, self.shape)


class InverseGamma(_Special):
    fn, rt_attrs, base_support = "mlf_prior_invgamma", ("scale",), _POSITIVE

    def __init__(self, shape, scale=1.0, name=None):
        Prior.__init__(self, name)
        self.shape, = _in_range("InverseGamma", SHAPE_MIN, SHAPE_MAX, shape=shape)
        self.scale = self._par("scale", "scale", scale)
        self.consts = _gamma_consts(self.scale, self.shape)


class Beta(_Special):
    fn, base_support = "mlf_prior_beta", (0.0, 1.0)

    def __init__(self, a, b, name=None):
        Prior.__init__(self, name)
        self.a, self.b = _in_range("Beta", SHAPE_MIN, SHAPE_MAX, a=a, b=b)
        self.consts = (self.a, self.b, _lbeta(self.a, self.b), math.log(self.a), math.log(self.b))


class StudentT(_Special):
    fn, rt_attrs = "mlf_prior_studentt", ("loc", "scale")

    def __init__(self, nu, loc=0.0, scale=1.0, name=None):
        Prior.__init__(self, name)
        self.nu, = _in_range("StudentT", NU_MIN, NU_MAX, nu=nu)
        self.loc = self._par("loc", "loc", loc)
        self.scale = self._par("scale", "scale", scale)
        ha = 0.5 * self.nu
        self.consts = (self.loc, self.scale, ha, _lbeta(ha, 0.5), math.log(ha), math.log(self.nu))


class Dirichlet(_Special):
    base_support = (0.0, 1.0)

    def __init__(self, alpha, name=None):
        Prior.__init__(self, name)
        try:
            alpha = np.array(alpha, dtype=float)
        except (TypeError, ValueError):
            raise ValueError("Dirichlet: alpha must be a vector of numbers")
        if alpha.ndim != 1 or not 1 <= len(alpha) <= MAX_BLOCK:
            raise ValueError("Dirichlet: alpha must be a vector of 1 to %d entries, got shape %s" % (MAX_BLOCK, alpha.shape))
        for k, v in enumerate(alpha):
            _in_range("Dirichlet", SHAPE_MIN, SHAPE_MAX, **{"alpha[%d]" % k: v})
        self.alpha = alpha
        self.size = len(alpha)

    def gammas(self):
        """the block's Gamma(alpha_k, 1) columns: the g row of the module docstring"""
        return [Gamma(a, 1.0) for a in self.alpha]

    def statements(self, first, cols=None):
        n = self.size
        out = ["p[%d] = %s;" % (first + k, g.call("u[%d]" % (first + k))) for k, g in enumerate(self.gammas())]
        out += ["{", "  double s = p[%d];" % first]
        out += ["  s = s + p[%d];" % (first + k) for k in range(1, n)]
        out.append("  if (s == %s) {" % _hex(0.0))
        out += ["    p[%d] = %s;" % (first + k, _hex(1.0 / n)) for k in range(n)]
        out.append("  } else {")
        out += ["    p[%d] = p[%d] / s;" % (first + k, first + k) for k in range(n)]
        out += ["  }", "}"]
        return out


class Tabulated(Prior):
    """A quantile function given as the knots of its CDF: F(x_k) = cdf_k, linear in between (module docstring).  ``table`` is
    the array the generated source holds, ``[c | x | s]`` with the slopes s computed here in binary64; ``steps`` the trip count
    of the device's bisection."""
    tabulated = True

    def __init__(self, x, cdf, name=None):
        Prior.__init__(self, name)
        try:
            x, c = np.array(x, dtype=float), np.array(cdf, dtype=float)
        except (TypeError, ValueError):
            raise ValueError("Tabulated: x and cdf must be arrays of numbers")
        if x.ndim != 1 or c.shape != x.shape:
            raise ValueError("Tabulated: x and cdf must be vectors of one length, got shapes %s and %s" % (x.shape, c.shape))
        n = len(x)
        if not 2 <= n <= MAX_KNOTS:
            raise ValueError("Tabulated: a table has 2 to %d knots, got %d" % (MAX_KNOTS, n))
        if not (np.isfinite(x).all() and np.isfinite(c).all()):
            raise ValueError("Tabulated: x and cdf must be finite")
        if (np.diff(x) < 0).any() or not x[0] < x[-1]:
            raise ValueError("Tabulated: x must be non-decreasing with x[0] < x[-1]")
        if (np.diff(c) < 0).any() or c[0] != 0.0 or c[-1] != 1.0:
            raise ValueError("Tabulated: cdf must be non-decreasing from exactly 0.0 to exactly 1.0")
        dx, dc = x[1:] - x[:-1], c[1:] - c[:-1]
        with np.errstate(all="ignore"):
            s = np.where(dc > 0, dx / np.where(dc > 0, dc, 1.0), 0.0)
        if not np.isfinite(s).all():
            raise ValueError("Tabulated: every slope (x[k+1] - x[k]) / (cdf[k+1] - cdf[k]) must be finite")
        self.x, self.cdf, self.slopes, self.n = x, c, s, n
        self.steps = (n - 2).bit_length()           # ceil(log2(n - 1))
        self.table = np.concatenate([c, x, s])

    @classmethod
    def from_samples(cls, samples, name=None):
        """equally weighted samples: the sorted samples at cdf_k = k / (m - 1) (the "linear" rule of ``np.quantile``)"""
        try:
            x = np.sort(np.array(samples, dtype=float).ravel())
        except (TypeError, ValueError):
            raise ValueError("Tabulated.from_samples: samples must be numbers")
        m = len(x)
        if m > MAX_KNOTS:
            raise ValueError("Tabulated.from_samples: %d samples, above the %d knots of a table: pass quantile knots instead, "
                             "such as Tabulated(np.quantile(samples, q), q) for a grid q from 0 to 1" % (m, MAX_KNOTS))
        if m < 2:
            raise ValueError("Tabulated.from_samples: at least 2 samples are needed")
        return cls(x, np.arange(m) / float(m - 1), name=name)

    @classmethod
    def from_histogram(cls, edges, density, name=None):
        """a piecewise-constant density over the bins between `edges`; the CDF is normalised, its ends pinned to 0.0 and 1.0"""
        try:
            e, h = np.array(edges, dtype=float), np.array(density, dtype=float)
        except (TypeError, ValueError):
            raise ValueError("Tabulated.from_histogram: edges and density must be arrays of numbers")
        if e.ndim != 1 or h.ndim != 1 or len(e) != len(h) + 1 or len(h) < 1:
            raise ValueError("Tabulated.from_histogram: n bins need n + 1 edges, got shapes %s and %s" % (e.shape, h.shape))
        if not (np.isfinite(e).all() and np.isfinite(h).all()) or (h < 0).any() or (np.diff(e) <= 0).any():
            raise ValueError("Tabulated.from_histogram: edges must be finite and ascending, density finite and >= 0")
        cum = np.concatenate([[0.0], np.cumsum(h * np.diff(e))])
        if not (np.isfinite(cum[-1]) and cum[-1] > 0):
            raise ValueError("Tabulated.from_histogram: the density must have a positive, finite integral")
        c = cum / cum[-1]
        c[0], c[-1] = 0.0, 1.0
        return cls(e, c, name=name)

    def support(self, cols=None, supports=None):
        return (float(self.x[0]), float(self.x[-1]))

    def array_name(self, first):
        return "mlf_prior_tab%d" % first

    def declaration(self, first):
        """the table as one array of the generated source"""
        vals = [_hex(v) for v in self.table]
        rows = [", ".join(vals[i:i + 6]) for i in range(0, len(vals), 6)]
        return "static __device__ const double %s[%d] = {\n  %s\n};\n" % (self.array_name(first), len(vals), ",\n  ".join(rows))

    def call(self, u, cols=None):
        raise NotImplementedError("a Tabulated column is written by statements(): it needs its column for the array's name")

    def statements(self, first, cols=None):
        return ["p[%d] = mlf_prior_table(u[%d], %s, %d, %d);" % (first, first, self.array_name(first), self.n, self.steps)]


def header_text():
    """the text of ``csrc/mlf_priors_dev.hpp``"""
    with open(HEADER) as fh:
        return fh.read()


def special_header_text():
    """the text of ``csrc/mlf_priors_special_dev.hpp``"""
    with open(SPECIAL_HEADER) as fh:
        return fh.read()


def rt_header_text():
    """the text of ``csrc/mlf_priors_rt_dev.hpp``"""
    with open(RT_HEADER) as fh:
        return fh.read()


class PriorTransform(object):
    """The prior transform of a list of priors (module docstring): ``ndim``, ``paramnames``, ``wrapped_dims`` (the circular
    columns, for the transform layer's ``wrapped_dims=``), ``is_affine`` (every prior ``Fixed`` or ``Uniform``: what the
    reference's ``is_affine_transform`` would find, and with it whether a driver needs a t-region), ``source`` (a
    self-contained HIP text defining ``mlf_user_transform``, a deterministic function of the priors' parameter bits),
    ``order`` (the priors in the order their statements are written: a stable topological sort of the ``Ref``s, ties in list
    order), ``parents`` (per column, the ascending tuple of columns it reads), ``supports`` (per column, the closed interval that holds
    it), ``model(loglike_source, ...)`` and the vectorized callback ``transform``."""

    def __init__(self, priors):
        self.priors = list(priors)
        if not self.priors:
            raise ValueError("PriorTransform needs at least one prior")
        for p in self.priors:
            if not isinstance(p, Prior):
                raise ValueError("PriorTransform takes Prior objects, got %r" % (p,))
        self.ndim = sum(p.size for p in self.priors)
        if self.ndim > devicemodel.MAX_DIM:
            raise ValueError("the priors span %d columns, above MLF_MAX_DIM = %d" % (self.ndim, devicemodel.MAX_DIM))
        self.paramnames, self.wrapped_dims, firsts = [], [], []
        first = 0
        for p in self.priors:
            self.paramnames += p.names(first)
            if p.circular:
                self.wrapped_dims.append(first)
            firsts.append(first)
            first += p.size
        tables = [p for p in self.priors if getattr(p, "tabulated", False)]
        if sum(p.n for p in tables) > MAX_TABLE_KNOTS:
            raise ValueError("the tables of one transform hold at most %d knots, got %d" % (MAX_TABLE_KNOTS, sum(p.n for p in tables)))
        cols = self._resolve(firsts)
        order = self._sort(firsts, cols)
        self.order = [self.priors[i] for i in order]
        self.parents = [()] * self.ndim
        supports = [None] * self.ndim
        body = []
        for i in order:             # dependency order: every parent's support is known and its statement already written
            p, first = self.priors[i], firsts[i]
            if p.refs:
                self.parents[first] = tuple(sorted(set(cols[i].values())))
                p.check_refs(cols[i], supports, self.paramnames)
            supports[first:first + p.size] = [p.support(cols[i], supports)] * p.size
            body += p.statements(first, cols[i])
        self.supports = supports
        self.is_affine = all(p.affine for p in self.priors)
        special = special_header_text() if any(getattr(p, "special", False) for p in self.priors) else ""
        rt = ""
        if tables or any(p.refs for p in self.priors):
            rt = rt_header_text() + "".join("\n" + p.declaration(firsts[i]) for i, p in enumerate(self.priors) if p in tables)
        self.source = (header_text() + special + rt + "\n__device__ void mlf_user_transform(const double *u, double *p, int d, const double *aux, "
                       "long long naux) {\n" + "".join("  %s\n" % s for s in body) + "}\n")
        self._model = None

    def _resolve(self, firsts):
        """per prior, the column behind every Ref parameter: {attribute: column}"""
        out = []
        for p, first in zip(self.priors, firsts):
            mine = {}
            for attr, (ref, _, label) in p.refs.items():
                where = "%s (column %d): %s = %r" % (type(p).__name__, first, label, ref)
                if isinstance(ref.target, str):
                    hits = [j for j, nm in enumerate(self.paramnames) if nm == ref.target]
                    if not hits:
                        raise ValueError("%s names no column; the columns are %s" % (where, ", ".join(self.paramnames)))
                    if len(hits) > 1:
                        raise ValueError("%s is ambiguous: columns %s carry that name" % (where, hits))
                    j = hits[0]
                else:
                    j = ref.target
                    if not 0 <= j < self.ndim:
                        raise ValueError("%s: there are columns 0 to %d" % (where, self.ndim - 1))
                if j == first:
                    raise ValueError("%s refers to its own column" % where)
                mine[attr] = j
            out.append(mine)
        return out

    def _sort(self, firsts, cols):
        """a stable topological sort of the priors (a block is one unit): of the priors whose parents are all written, the
        one that comes first in the list is next"""
        owner = {}
        for i, p in enumerate(self.priors):
            for k in range(p.size):
                owner[firsts[i] + k] = i
        needs = [set(owner[j] for j in mine.values()) for mine in cols]
        if not any(needs):
            return list(range(len(self.priors)))
        done, order = set(), []
        while len(order) < len(self.priors):
            ready = [i for i in range(len(self.priors)) if i not in done and needs[i] <= done]
            if not ready:
                left = [self.paramnames[firsts[i]] for i in range(len(self.priors)) if i not in done]
                raise ValueError("the Refs of the columns %s form a cycle" % ", ".join(left))
            done.add(ready[0])
            order.append(ready[0])
        return order

    def model(self, loglike_source, aux=None, **kw):
        """``DeviceModel(ndim, loglike_source, transform_source=self.source, aux=aux, **kw)``: name, nterms, nsums, nderived,
        derived_source and gate_derived pass through"""
        return DeviceModel(self.ndim, loglike_source, transform_source=self.source, aux=aux, **kw)

    def transform(self, u):
        """vectorized callback (n, ndim) -> (n, ndim), evaluated on the GPU (a lazily built model with a constant likelihood;
        no CPU fallback), for a likelihood that stays a host function"""
        if self._model is None:
            self._model = self.model(CONSTANT_LOGLIKE, name="PriorTransform%d" % self.ndim)
        return self._model.transform(u)


__all__ = ["Prior", "Fixed", "Uniform", "LogUniform", "Normal", "TruncatedNormal", "LogNormal", "HalfNormal", "Exponential",
           "Rayleigh", "Weibull", "Pareto", "Cauchy", "HalfCauchy", "Laplace", "Logistic", "Gumbel", "Triangular", "Sine",
           "Cosine", "MultivariateNormal", "OrderedUniform", "Gamma", "ChiSquared", "InverseGamma", "Beta", "StudentT",
           "Dirichlet", "Ref", "Tabulated", "PriorTransform"]
