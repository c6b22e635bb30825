"""Warm start: auxiliary problems that deform the unit cube so the sampler begins near the posterior.

The names and signatures are those of the reference's ``ultranest/hotstart.py`` (ideas of Petrosyan & Handley 2022,
arXiv:2212.01760): given samples of an earlier or cheaper run, the cube is deformed towards them and the deformation is
undone by a log-weight added to the likelihood.  For host callbacks every function returns what the reference returns for
the same arguments (numpy / scipy), with two deliberate differences: where the reference asserts, or takes the ``min()`` of an
empty selection, a ``ValueError`` with a message is raised; and ``reuse_samples`` does not print.

Device forms, chosen automatically
----------------------------------
When ``devicemodel.device_route(transform, loglike)`` recognises the pair as one ``DeviceModel``, forms (a) and (b) below
return the callbacks of a NEW ORDINARY ``DeviceModel`` (also reachable as ``.model`` on the returned loglike), so every
device route serves the auxiliary problem unchanged: there is no new program kind, no new C-ABI entry and nothing new in the
built library.  The new model's source is the inner model's source with its entry points renamed (``#define`` / ``#undef``
around the unedited text), then the text of ``csrc/mlf_hotstart_dev.hpp``, then a short generated wrapper that defines the
real ``mlf_user_*`` entry points.  All tables go in a tail appended to the model's ``aux`` array (layout: the header); the
inner functions see their own ``aux`` with their own ``naux``.  Source and code object depend on the inner source, ``d``
and the form, not on the samples: two sample sets at one ``d`` share one code object.  The wrapper keeps the deformed
coordinates in a private array of ``d`` doubles sized by a generated ``#define MLF_HOTSTART_D`` (where the inner model has no
transform, form (a) writes them straight into the ``p`` row and needs none; form (b) keeps them in its ``p`` row and holds the
inner transform's output in such an array).

(a) ``get_auxiliary_contbox_parameterization`` -- the form the reference driver's warm start uses.  ``ndim = d + 1``: the last
    cube coordinate t selects, by numpy's ``interp`` formula over at most 25 knots, a box ``[ulo_i(t), uhi_i(t)]`` per axis;
    ``umod_i = ulo_i + (uhi_i - ulo_i) * u_i``; ``p[0..d) = transform(umod)``, ``p[d] = sum_i log(uhi_i - ulo_i)`` in axis
    order; ``L = loglike(p[0..d)) + p[d]``.  Summed inner models are supported: ``nterms`` and ``nterms, nsums`` models both
    become an ``nsums`` model whose ``finish`` adds ``p[d]`` once (a single-sum model becomes ``nsums = 1``, whose order
    contract is the single-sum one), so the auxiliary L is the inner L plus the weight, bit for bit.  ``nderived`` of the
    inner model is carried over; its derived function sees ``p[0..d)``.

    THE CONTBOX PROBLEM IS NOT EVIDENCE-PRESERVING.  ``Z_aux = integral_0^1 Z_box(t) dt`` with ``Z_box(t)`` the evidence
    inside the box at t, and its x-marginal is ``L(x) * (1 - t_min(x))`` with ``t_min(x)`` the smallest t whose box contains
    x.  This reproduces the reference, not a corrected method.

(b) ``get_extended_auxiliary_independent_problem`` -- an independent Student-t per axis, truncated to the cube.
    ``ndim = d``, ``nderived = d + 1``.  The model's transform is the deformation itself, its ``p`` row the deformed cube
    coordinates:  ``x_i = ctr_i + err_i * tppf(u_i * w_i + lo_i)``;  the likelihood reads that row,
    ``L = loglike(transform(x)) - sum_i logpdf_i(x_i)`` (the log-density taken from x, as the reference's ``logpdf(x)``);
    the derived function gives ``[p | logweight]`` for the rows that are handed out.  So ``model.transform(u)`` is
    ``[x | p | logweight]`` -- the reference's transform returns ``[p | logweight]`` (the same values in the last ``d + 1``
    columns) and its likelihood reads that row; here the likelihood reads x.  This way the quantile runs once per row in a
    function that holds no array, and the likelihood holds one private array of ``d`` doubles (the inner transform's output)
    or none; a likelihood that deformed the cube itself would need two.  ``df = 1`` uses the closed Cauchy forms, otherwise
    ``mlf_prior_studentt`` (1 <= df <= 1000).  The form is exact up to a constant: ``model.logz_offset = sum_i ln w_i`` and
    ``ln Z = ln Z_aux + logz_offset``.  Default-form inner models only (a summed one raises ``ValueError`` naming form (a)).
    An inner model's own derived columns are NOT carried (the derived columns of this form are ``[p | logweight]``): the call
    warns (``UserWarning``) when it drops them.

Three consequences of building the deformation into an ordinary model, for both forms:

* ``device_route(identity_transform, aux_loglike)`` is ``(model, False)`` like for every DeviceModel, and the likelihood then
  reads the raw cube row as its ``p`` row: in (a) ``u[d]`` as the weight, in (b) ``u`` as x.  An auxiliary likelihood is only
  meaningful with its own transform.
* A driver's t-region (``build_tregion=True``) is an ellipsoid over the model's output columns.  For (a) these are the
  physical parameters and the weight; for (b) they are ``[x | p | logweight]``: the deformed cube row first, not only the
  physical parameters (and where the inner transform is affine, or missing, p is a linear function of x, no such ellipsoid
  has a volume and the driver runs without a t-region, as it does for every degenerate parameter set).
* (b) has derived columns and no ``gate_derived``, so by the rule of ``devicemodel`` a refill WITH a t-region returns None and
  that batch takes the host sequence through the same callbacks (correct, and slow); without a t-region every route is the
  device's.  (a) carries the inner model's ``gate_derived`` and is gated on the device like any model.

(c) ``get_auxiliary_problem`` and ``get_extended_auxiliary_problem`` (rotated Student-t) keep the host form only; a
    ``DeviceModel`` pair raises ``ValueError`` naming (a) and (b): they need a d x d product per row in one thread, and rows
    that stay ``ndim`` wide.

A covariance model (``DeviceModel(..., ncov=n)``) has no device form under (a) or (b): its likelihood is not a function the
wrappers can call from one thread.  Both raise ``ValueError`` naming the host form (host callbacks around the model's own).

(d) ``from_results(model, results)`` builds (a) from a results dict (``weighted_samples``: ``upoints`` and ``weights``).
"""
import math
import os
import warnings

import numpy as np

from . import devicemodel, priors
from .devicemodel import DeviceModel
from .utils import resample_equal, vectorize

HEADER = os.path.join(devicemodel.INCLUDE_DIR, "mlf_hotstart_dev.hpp")
# the tail probabilities of the four quantile boxes of form (a), as numpy's power gives them (the literals 1e-3, 1e-5 differ
# from it in the last bit, and the boxes are compared bit for bit)
CONTBOX_STEPS = np.power(10.0, [-1.0, -3.0, -5.0, -7.0])
MAX_KNOTS = 25
_ENTRIES = ("mlf_user_loglike", "mlf_user_loglike_term", "mlf_user_loglike_terms", "mlf_user_loglike_finish",
            "mlf_user_transform", "mlf_user_derived")
_MARK = "MLF_HOTSTART_DEV_HPP"


def header_text():
    """the text of ``csrc/mlf_hotstart_dev.hpp``"""
    with open(HEADER) as fh:
        return fh.read()


def _inner(name):
    return name.replace("mlf_user_", "mlf_hotstart_inner_")


def _renamed(text):
    """`text` between the #defines that rename its entry points and their #undefs; the text itself is not edited"""
    return ("".join("#define %s %s\n" % (n, _inner(n)) for n in _ENTRIES) + text + "\n"
            + "".join("#undef %s\n" % n for n in _ENTRIES))


# What a host auxiliary problem answers outside the cube, and where it stops trusting a weight.  These are values a caller of the
# reference sees (a likelihood of -1e300, a weight of -1e101), so they are part of the interface and kept.
OUTSIDE_LOGLIKE = -1e300
OUTSIDE_WEIGHT = -1e101
WEIGHT_LIMIT = 1e100


class _StudentT(object):
    """The standard Student-t distribution with `df` degrees of freedom (scipy.stats): quantile, CDF, log-density, and
    ``lognorm``, the log-density at 0.  An axis with centre c and scale e has the quantile ``c + e * quantile(q)``, the CDF
    ``cdf((x - c) / e)`` and the log-density ``logpdf((x - c) / e) - log(e)``."""

    def __init__(self, df):
        import scipy.stats
        self.df = float(df)
        self._rv = scipy.stats.t(df)
        self.lognorm = float(self._rv.logpdf(0.0))

    def quantile(self, q):
        return self._rv.ppf(q)

    def cdf(self, t):
        return self._rv.cdf(t)

    def logpdf(self, t):
        return self._rv.logpdf(t)


def _student_args(ctr, second, df, second_name):
    ctr = np.asarray(ctr, dtype=float)
    if ctr.ndim != 1 or len(ctr) < 1:
        raise ValueError("ctr must be a vector (the posterior centre in u-space), got shape %s" % (ctr.shape,))
    second = np.asarray(second, dtype=float)
    want = (len(ctr), len(ctr)) if second_name == "invcov" else (len(ctr),)
    if second.shape != want:
        raise ValueError("%s must have shape %s, got %s" % (second_name, want, second.shape))
    if not df >= 1:
        raise ValueError("df (degrees of freedom) must be at least 1, got %r" % (df,))
    return ctr, second


def _refuse_rotated(name, loglike, transform):
    if devicemodel.device_route(transform, loglike) is not None:
        raise ValueError("%s has no device form (a d x d product per row): for a DeviceModel use (a) "
                         "get_auxiliary_contbox_parameterization or (b) get_extended_auxiliary_independent_problem" % name)


def _principal_axes(invcov, enlargement_factor):
    """The matrix whose column k is the k-th eigenvector of `invcov` scaled to `enlargement_factor` standard deviations along it
    (the eigenvalues of an inverse covariance are inverse variances)."""
    inverse_variances, directions = np.linalg.eigh(invcov)
    return directions * (enlargement_factor / np.sqrt(inverse_variances))


def _inside_cube(x):
    return bool(np.all(x > 0) and np.all(x < 1))


def _weighted_loglike(loglike, weight_ref):
    """The likelihood of the two `extended` problems: the row's last entry is the correction weight (offset by weight_ref)."""
    def aux_loglikelihood(row):
        weight = row[-1]
        if abs(weight) < WEIGHT_LIMIT:          # (False for NaN as well)
            return loglike(row[:-1]) + weight - weight_ref
        return OUTSIDE_LOGLIKE
    return aux_loglikelihood


def get_auxiliary_problem(loglike, transform, ctr, invcov, enlargement_factor, df=1):
    """Rotated d-dimensional Student-t auxiliary problem (host callbacks only).  A cube point u becomes independent standard
    Student-t coordinates t, which are laid along the principal axes of the sample covariance, x = ctr + t A^T; the likelihood is
    L(transform(x)) minus the log-density of t, and OUTSIDE_LOGLIKE where x leaves the cube.  Returns
    ``(aux_loglike, aux_aftertransform)``; ``aux_aftertransform(u)`` gives the parameters of the point."""
    _refuse_rotated("get_auxiliary_problem", loglike, transform)
    ctr, invcov = _student_args(ctr, invcov, df, "invcov")
    dist = _StudentT(df)
    axes_t = _principal_axes(invcov, enlargement_factor)

    def point(u):
        t = dist.quantile(u)
        return t, ctr + np.dot(t, axes_t)

    def aux_loglikelihood(u):
        t, x = point(u)
        if not _inside_cube(x):
            return OUTSIDE_LOGLIKE
        return loglike(transform(x)) - dist.logpdf(t).sum()

    def aux_aftertransform(u):
        return transform(point(u)[1])

    return aux_loglikelihood, aux_aftertransform


def get_extended_auxiliary_problem(loglike, transform, ctr, invcov, enlargement_factor, df=1):
    """Rotated Student-t auxiliary problem whose transform appends the correction weight (host callbacks only): x = ctr + A t,
    the row is ``[transform(x) | weight]`` with weight = -sum logpdf(t) + d logpdf(0); outside the cube the row is that of the
    cube's centre with OUTSIDE_WEIGHT.  Returns ``(aux_loglike, aux_transform)``."""
    _refuse_rotated("get_extended_auxiliary_problem", loglike, transform)
    ctr, invcov = _student_args(ctr, invcov, df, "invcov")
    dist = _StudentT(df)
    axes = _principal_axes(invcov, enlargement_factor)
    weight_ref = dist.lognorm * len(ctr)

    def aux_transform(u):
        t = dist.quantile(u)
        x = ctr + np.dot(axes, t)
        if _inside_cube(x):
            return np.append(transform(x), weight_ref - dist.logpdf(t).sum())
        return np.append(transform(np.full(len(ctr), 0.5)), OUTSIDE_WEIGHT)

    return _weighted_loglike(loglike, weight_ref), aux_transform


def _indep_wrapper(d, inner_transform, cauchy):
    """(likelihood, transform, derived) wrapper texts of form (b); the p row is x"""
    D = "MLF_HOTSTART_D"
    nin = "  const long long nin = mlf_hotstart_indep_nin(naux, %s);" % D
    # Student-t form: the likelihood's body is a function of its own, not inlined.  The kernel then holds the quantile's call
    # but no array, and the array sits in a function without a call of this module's making, whose frame keeps the 8-byte
    # alignment: 8 (d + 1) bytes and not 8 (d + 2) at even d
    like = ["#define %s %d" % (D, d)]
    if not cauchy:
        like += ["__device__ __noinline__ double mlf_hotstart_indep_like(const double *x, const double *aux, long long naux);",
                 "__device__ double mlf_user_loglike(const double *x, int d, const double *aux, long long naux) {",
                 "  return mlf_hotstart_indep_like(x, aux, naux);", "}"]
    like += ["__device__ __noinline__ double mlf_hotstart_indep_like(const double *x, const double *aux, long long naux) {" if not cauchy else
             "__device__ double mlf_user_loglike(const double *x, int d, const double *aux, long long naux) {", nin,
            "  const double s = mlf_hotstart_indep_logpdf(x, %s, aux, naux);" % D]
    if inner_transform:
        like += ["  alignas(8) double y[%s];" % D,
                 "  mlf_hotstart_inner_transform(x, y, %s, aux, nin);" % D,
                 "  return mlf_hotstart_inner_loglike(y, %s, aux, nin) - s;" % D]
    else:
        like += ["  return mlf_hotstart_inner_loglike(x, %s, aux, nin) - s;" % D]
    like += ["}", ""]
    tr = ["__device__ void mlf_user_transform(const double *u, double *p, int d, const double *aux, long long naux) {",
          "  mlf_hotstart_indep_x(u, p, %s, aux, naux);" % D, "}", ""]
    derived = ["__device__ void mlf_user_derived(const double *x, int d, double *q, int nq, const double *aux, long long naux) {", nin,
               "  const double s = mlf_hotstart_indep_logpdf(x, %s, aux, naux);" % D]
    if inner_transform:
        derived += ["  mlf_hotstart_inner_transform(x, q, %s, aux, nin);" % D]
    else:
        derived += ["  for (int i = 0; i < %s; ++i) q[i] = x[i];" % D]
    derived += ["  q[%s] = -s + aux[naux - 2];" % D, "}", ""]
    return "\n".join(like), "\n".join(tr), "\n".join(derived)


def _inner_source(model):
    if _MARK in model.source:
        raise ValueError("%s is itself a warm-start model: build the auxiliary problem from the original model" % model.name)
    return model.source


def independent_tables(ctr, err, df):
    """The per-axis tables of form (b), as the device tail holds them: ``(ctr, err, w, lo, c, consts)`` with
    ``w = cdf(1) - cdf(0)``, ``lo = cdf(0)``, ``c_i = lognorm(df) - log(err_i)`` and ``consts = [df/2, ln B(df/2, 1/2),
    ln(df/2), ln df, df, (df + 1)/2, sum c_i]``."""
    dist = _StudentT(df)
    lo = dist.cdf((0.0 - ctr) / err)
    w = dist.cdf((1.0 - ctr) / err) - lo
    ha = 0.5 * df
    c = dist.lognorm - np.log(err)
    consts = np.array([ha, math.lgamma(ha) + math.lgamma(0.5) - math.lgamma(ha + 0.5), math.log(ha), math.log(df), df,
                       0.5 * (df + 1.0), c.sum()])
    return ctr, err, w, lo, c, consts


def independent_tail(ctr, err, w, lo, c, consts):
    """The tail of form (b) as the device reads it (``csrc/mlf_hotstart_dev.hpp``): one record of 11 values per axis
    ``[w, lo, ha, lnB, lnha, lnnu, ctr, err, c, df, (df + 1) / 2]``, then ``weight_ref`` and ``d``."""
    d = len(ctr)
    rec = np.empty((d, 11))
    rec[:, 0], rec[:, 1], rec[:, 2:6], rec[:, 6], rec[:, 7], rec[:, 8], rec[:, 9:11] = w, lo, consts[:4], ctr, err, c, consts[4:6]
    return np.concatenate([rec.ravel(), [consts[6], float(d)]])


def _refuse_cov(name, model):
    if getattr(model, "ncov", None) is not None:
        raise ValueError("%s has no device form over a covariance model (ncov: %s): pass host callbacks for the host form, "
                         "e.g. ``lambda x: model.loglike(x)`` and ``lambda u: model.transform(u)``" % (name, model.name))


def _independent_device(model, with_transform, ctr, err, df):
    _refuse_cov("get_extended_auxiliary_independent_problem", model)
    d = model.ndim
    if len(ctr) != d:
        raise ValueError("ctr has %d entries, the model %s has %d parameters" % (len(ctr), model.name, d))
    if model.summed:
        raise ValueError("get_extended_auxiliary_independent_problem takes a default-form DeviceModel; for a summed model "
                         "(nterms) use form (a), get_auxiliary_contbox_parameterization")
    if not (np.isfinite(ctr).all() and np.isfinite(err).all() and (err > 0).all()):
        raise ValueError("ctr must be finite and err finite and positive")
    df = float(df)
    if not df <= priors.NU_MAX:
        raise ValueError("df must lie in [1, %g] on the device (the range of mlf_prior_studentt), got %r" % (priors.NU_MAX, df))
    if d + d + 1 > devicemodel.MAX_DIM:
        raise ValueError("the auxiliary model has %d columns, above MLF_MAX_DIM = %d" % (2 * d + 1, devicemodel.MAX_DIM))
    inner = _inner_source(model)
    if model.nderived is not None:
        warnings.warn("%s has %d derived parameters, which the independent Student-t form does not carry: its derived columns are "
                      "[p | logweight]" % (model.name, model.nderived), UserWarning, stacklevel=3)
    tables = independent_tables(ctr, err, df)
    w = tables[2]
    if not (w > 0).all():
        raise ValueError("an axis' Student-t has no probability inside the unit cube in binary64")
    cauchy = df == 1.0
    inner_transform = bool(with_transform and model.has_transform)
    loglike_w, tr_w, derived_w = _indep_wrapper(d, inner_transform, cauchy)
    # (the Student-t quantile stays the header's __noinline__ function: inlined into the wrapper's loop its 64-bit constants
    # fill the scalar registers and the program spills 8 to 44 of them -- measured)
    lib = "" if cauchy else priors.header_text() + priors.special_header_text()
    source = (_renamed(inner) + lib + "#define MLF_HOTSTART_INDEP 1\n#define MLF_HOTSTART_CAUCHY %d\n" % int(cauchy)
              + header_text() + "\n" + loglike_w)
    aux = np.concatenate([model.aux, independent_tail(*tables)])
    new = DeviceModel(d, source, tr_w, aux=aux, name="%s_hotstart_indep" % model.name, nderived=d + 1, derived_source=derived_w)
    new.logz_offset = float(np.log(w).sum())
    new.inner = model
    new.loglike.model = new
    return new


def get_extended_auxiliary_independent_problem(loglike, transform, ctr, err, df=1):
    """Independent Student-t per axis, truncated to the unit cube (module docstring, form (b)).  Returns
    ``(aux_loglike, aux_transform)``.  Host callbacks: the reference's pair (the transform maps d cube coordinates to
    ``[p | logweight]``, the likelihood reads that row).  A ``DeviceModel`` pair: the callbacks of a new DeviceModel
    (``aux_loglike.model``), whose transform returns ``[x | p | logweight]`` and whose ``logz_offset`` completes the evidence;
    derived columns of the inner model are dropped with a ``UserWarning``, and a refill with a t-region takes the host sequence
    (module docstring)."""
    ctr, err = _student_args(ctr, err, df, "err")
    route = devicemodel.device_route(transform, loglike)
    if route is not None:
        new = _independent_device(route[0], route[1], ctr, err, df)
        return new.loglike, new.transform
    dist = _StudentT(df)
    ctr_, err_, inside, below, peak, _ = independent_tables(ctr, err, float(df))      # mass inside the cube, mass below it
    weight_ref = peak.sum()                                                           # the log-density at the centre

    def aux_transform(u):
        x = ctr + err * dist.quantile(u * inside + below)
        logdensity = (dist.logpdf((x - ctr) / err) - np.log(err)).sum()
        return np.append(transform(x), weight_ref - logdensity)

    return _weighted_loglike(loglike, weight_ref), aux_transform


def compute_quantile_intervals(steps, upoints, uweights):
    """Lower and upper axis quantiles: ``(ulos, uhis)`` of shape ``(len(steps) + 1, d)``.  Per axis the samples are sorted and
    their weights accumulated; row j spans the samples whose cumulative weight c satisfies ``steps[j] <= c <= 1 - steps[j]``;
    the last row is the whole cube.  The cumulative weights ascend, so the two ends of a row are two binary searches."""
    samples, weights = np.asarray(upoints, dtype=float), np.asarray(uweights, dtype=float)
    if samples.ndim != 2:
        raise ValueError("upoints must be a 2d array (N, d), got shape %s" % (samples.shape,))
    if weights.shape != (samples.shape[0],):
        raise ValueError("uweights must have one entry per sample, got shape %s for %d samples" % (weights.shape, samples.shape[0]))
    if not (weights >= 0).all():
        raise ValueError("uweights must not be negative")
    tails = [float(q) for q in steps]
    lower = np.zeros((len(tails) + 1, samples.shape[1]))
    upper = np.ones((len(tails) + 1, samples.shape[1]))
    for axis in range(samples.shape[1]):
        rank = np.argsort(samples[:, axis])
        ascending, cumulative = samples[rank, axis], np.cumsum(weights[rank])
        for row, q in enumerate(tails):
            first = int(np.searchsorted(cumulative, q, side="left"))
            last = int(np.searchsorted(cumulative, 1 - q, side="right")) - 1
            if first > last:
                raise ValueError("no sample of axis %d has a cumulative weight between %g and 1 - %g: too few samples, or "
                                 "weights that do not sum to 1" % (axis, q, q))
            lower[row, axis], upper[row, axis] = ascending[first], ascending[last]
    return lower, upper


def compute_quantile_intervals_refined(steps, upoints, uweights, logsteps_max=20):
    """``(ulos, uhis, uinterpspace)``: the quantile boxes of `compute_quantile_intervals`, and between the widest of them, B, and
    the cube a ladder of boxes ``(1 - f) B + f cube`` at f = 10^-K, ..., 10^-1, 1, where K (at most `logsteps_max`) is the
    number of decades that separate B's narrowest side from the cube's.  The knots in t: the quantile boxes evenly spaced
    from 0, the ladder evenly spaced from the last of them to 1."""
    nquantiles = len(steps)
    if nquantiles < 2:
        raise ValueError("steps must hold at least two quantiles for the refined boxes")
    lower, upper = compute_quantile_intervals(steps, upoints, uweights)
    widest_lo, widest_hi = lower[nquantiles - 1], upper[nquantiles - 1]
    narrowest = float((widest_hi - widest_lo).min())
    decades = logsteps_max if not narrowest > 0 else min(logsteps_max, int(math.ceil(-math.log10(max(narrowest, 1e-300)))))
    decades = max(decades, 0)
    f = np.power(10.0, np.arange(-decades, 1, dtype=float))[:, None]
    ladder_lo = widest_lo[None, :] * (1 - f)
    ladder_hi = widest_hi[None, :] * (1 - f) + f
    lower = np.vstack([lower[:nquantiles], ladder_lo])
    upper = np.vstack([upper[:nquantiles], ladder_hi])
    if not ((lower[-1] == 0).all() and (upper[-1] == 1).all()):
        raise ValueError("the last box is not the unit cube: the samples must lie inside it")
    quantile_knots = np.linspace(0, 1, nquantiles + 1)[:nquantiles]
    ladder_knots = np.linspace(quantile_knots[-1], 1, decades + 2)[1:]
    return lower, upper, np.concatenate([quantile_knots, ladder_knots])


def contbox_tail(ulos, uhis, uinterpspace):
    """The tail of form (a) as the device reads it (``csrc/mlf_hotstart_dev.hpp``): ``[xp | lo | slo | hi | shi | M]`` with
    the slopes ``(fp[j+1] - fp[j]) / (xp[j+1] - xp[j])`` of numpy's ``interp`` computed here in binary64."""
    xp = np.asarray(uinterpspace, dtype=float)
    lo, hi = np.asarray(ulos, dtype=float), np.asarray(uhis, dtype=float)
    M = len(xp)
    if not 2 <= M <= 32 or lo.shape != hi.shape or lo.shape[0] != M:
        raise ValueError("a contbox table has 2 to 32 knots and one row of box edges per knot")
    if not (np.diff(xp) > 0).all():
        raise ValueError("the knots must ascend strictly")
    dx = np.diff(xp)[:, None]
    return np.concatenate([xp, lo.ravel(), ((lo[1:] - lo[:-1]) / dx).ravel(), hi.ravel(), ((hi[1:] - hi[:-1]) / dx).ravel(), [float(M)]])


def _contbox_wrapper(d, model, inner_transform):
    D = "MLF_HOTSTART_D"
    head = ["#define %s %d" % (D, d)]
    nin = "  const long long nin = mlf_hotstart_contbox_nin(aux, naux, %s);" % D
    if model.nsums is not None:
        like = ["__device__ void mlf_user_loglike_terms(const double *p, int d, const double *aux, long long naux, long long k, double *t) {",
                nin, "  mlf_hotstart_inner_loglike_terms(p, %s, aux, nin, k, t);" % D, "}",
                "__device__ double mlf_user_loglike_finish(const double *s, int nsums, const double *p, int d, const double *aux, long long naux) {",
                nin, "  return mlf_hotstart_inner_loglike_finish(s, nsums, p, %s, aux, nin) + p[%s];" % (D, D), "}"]
    elif model.summed:
        like = ["__device__ void mlf_user_loglike_terms(const double *p, int d, const double *aux, long long naux, long long k, double *t) {",
                nin, "  t[0] = mlf_hotstart_inner_loglike_term(p, %s, aux, nin, k);" % D, "}",
                "__device__ double mlf_user_loglike_finish(const double *s, int nsums, const double *p, int d, const double *aux, long long naux) {",
                "  return s[0] + p[%s];" % D, "}"]
    else:
        like = ["__device__ double mlf_user_loglike(const double *p, int d, const double *aux, long long naux) {",
                nin, "  return mlf_hotstart_inner_loglike(p, %s, aux, nin) + p[%s];" % (D, D), "}"]
    tr = ["__device__ void mlf_user_transform(const double *u, double *p, int d, const double *aux, long long naux) {",
          "  const int M = (int)aux[naux - 1];",
          "  const long long nin = naux - mlf_hotstart_contbox_tail(M, %s);" % D]
    if inner_transform:
        tr += ["  alignas(8) double umod[%s];" % D,
               "  const double weight = mlf_hotstart_contbox(u, umod, %s, aux + nin, M);" % D,
               "  mlf_hotstart_inner_transform(umod, p, %s, aux, nin);" % D]
    else:
        tr += ["  const double weight = mlf_hotstart_contbox(u, p, %s, aux + nin, M);" % D]
    tr += ["  p[%s] = weight;" % D, "}", ""]
    derived = ["__device__ void mlf_user_derived(const double *p, int d, double *q, int nq, const double *aux, long long naux) {",
               nin, "  mlf_hotstart_inner_derived(p, %s, q, nq, aux, nin);" % D, "}", ""]
    return "\n".join(head + like + [""]), "\n".join(tr), "\n".join(derived)


def _check_samples(upoints, uweights):
    upoints = np.asarray(upoints, dtype=float)
    if upoints.ndim != 2:
        raise ValueError("expected a 2d array (N, d) for upoints, got shape %s" % (upoints.shape,))
    outside = ((upoints <= 0) | (upoints >= 1) | np.isnan(upoints)).any(axis=1)
    if outside.any():
        raise ValueError("upoints must lie strictly between 0 and 1; %d of %d rows do not" % (outside.sum(), len(outside)))
    if upoints.shape[0] <= 10:
        raise ValueError("more than 10 samples are needed, got %d" % upoints.shape[0])
    uweights = np.asarray(uweights, dtype=float)
    if uweights.shape != (upoints.shape[0],):
        raise ValueError("uweights must have one entry per sample, got shape %s for %d samples" % (uweights.shape, upoints.shape[0]))
    return upoints, uweights


def _contbox_device(model, with_transform, ulos, uhis, uinterpspace):
    _refuse_cov("get_auxiliary_contbox_parameterization", model)
    d = model.ndim
    if ulos.shape[1] != d:
        raise ValueError("upoints has %d columns, the model %s has %d parameters" % (ulos.shape[1], model.name, d))
    if d + 1 + (model.nderived or 0) > devicemodel.MAX_DIM:
        raise ValueError("the auxiliary model has %d columns, above MLF_MAX_DIM = %d" % (d + 1 + (model.nderived or 0), devicemodel.MAX_DIM))
    inner = _inner_source(model)
    inner_transform = bool(with_transform and model.has_transform)
    like_w, tr_w, derived_w = _contbox_wrapper(d, model, inner_transform)
    source = _renamed(inner) + header_text() + "\n" + like_w
    aux = np.concatenate([model.aux, contbox_tail(ulos, uhis, uinterpspace)])
    kw = {}
    if model.nderived is not None:
        kw = dict(nderived=model.nderived, derived_source=_renamed(model.derived_source) + derived_w, gate_derived=model.gate_derived)
    if model.summed:
        kw.update(nterms=model.nterms, nsums=model.nsums if model.nsums is not None else 1)
    new = DeviceModel(d + 1, source, tr_w, aux=aux, name="%s_hotstart_contbox" % model.name, **kw)
    new.inner = model
    new.loglike.model = new
    return new


def contbox_rows(u, ulos, uhis, uinterpspace):
    """``(umod, logweight)`` of cube rows ``u`` (n, d + 1) in numpy: the reference's vectorized transform before the inner
    transform (``np.interp`` per axis, the weight summed in axis order)."""
    u = np.asarray(u, dtype=float)
    ndim = ulos.shape[1]
    if u.ndim != 2 or u.shape[1] != ndim + 1:
        raise ValueError("expected cube rows of shape (n, %d), got %s" % (ndim + 1, u.shape))
    umod = np.empty((u.shape[0], ndim))
    logvol = np.zeros((u.shape[0], 1))
    for i in range(ndim):
        ulo = np.interp(u[:, -1], uinterpspace, ulos[:, i])
        uhi = np.interp(u[:, -1], uinterpspace, uhis[:, i])
        umod[:, i] = ulo + (uhi - ulo) * u[:, i]
        logvol[:, 0] += np.log(uhi - ulo)
    return umod, logvol


def get_auxiliary_contbox_parameterization(param_names, loglike, transform, upoints, uweights, vectorized=False):
    """The continuous-box auxiliary problem (module docstring, form (a)).  Returns ``(aux_param_names, aux_loglike,
    aux_transform, vectorized)``: one more parameter, ``aux_logweight``, whose cube coordinate selects the box.  A
    ``DeviceModel`` pair gives the callbacks of a new DeviceModel (``aux_loglike.model``; vectorized is then True).  NOT
    evidence-preserving: ``Z_aux = integral_0^1 Z_box(t) dt``."""
    upoints, uweights = _check_samples(upoints, uweights)
    ndim = upoints.shape[1]
    route = devicemodel.device_route(transform, loglike)
    if route is not None and route[0].ndim != ndim:
        raise ValueError("upoints has %d columns, the model %s has %d parameters" % (ndim, route[0].name, route[0].ndim))
    ulos, uhis, uinterpspace = compute_quantile_intervals_refined(CONTBOX_STEPS, upoints, uweights)
    aux_param_names = list(param_names) + ['aux_logweight']
    if route is not None:
        new = _contbox_device(route[0], route[1], ulos, uhis, uinterpspace)
        return aux_param_names, new.loglike, new.transform, True

    def aux_transform(u):
        if np.shape(u) != (ndim + 1,):
            raise ValueError("expected %d cube coordinates, got shape %s" % (ndim + 1, np.shape(u)))
        umod, logvol = contbox_rows(np.asarray(u, dtype=float)[None, :], ulos, uhis, uinterpspace)
        return np.append(transform(umod[0]), logvol[0, 0])

    def aux_transform_vectorized(u):
        umod, logvol = contbox_rows(u, ulos, uhis, uinterpspace)
        return np.hstack((transform(umod), logvol))

    def aux_loglikelihood(x):
        return loglike(x[:-1]) + x[-1]

    def aux_loglikelihood_vectorized(x):
        return loglike(x[:, :-1]) + x[:, -1]

    if vectorized:
        return aux_param_names, aux_loglikelihood_vectorized, aux_transform_vectorized, vectorized
    return aux_param_names, aux_loglikelihood, aux_transform, vectorized


def from_results(model, results, param_names=None):
    """Form (a) for a DeviceModel from a results dict of an earlier run: ``results['weighted_samples']`` holds ``upoints``
    and ``weights`` (what the reference's ``warmstart_from_similar_file`` does after reading its file: samples of zero weight
    are dropped and the weights normalised).  Returns what `get_auxiliary_contbox_parameterization` returns."""
    try:
        ws = results["weighted_samples"]
        upoints, weights = np.asarray(ws["upoints"], dtype=float), np.asarray(ws["weights"], dtype=float)
    except (KeyError, TypeError):
        raise ValueError("results must hold weighted_samples with upoints and weights")
    if upoints.ndim != 2 or weights.shape != (upoints.shape[0],):
        raise ValueError("weighted_samples: upoints must be (N, d) and weights (N,), got %s and %s" % (upoints.shape, weights.shape))
    mask = weights > 0
    if not mask.any():
        raise ValueError("weighted_samples holds no sample of positive weight")
    weights = weights[mask] / weights[mask].sum()
    if param_names is None:
        param_names = results.get("paramnames") or ["p%d" % k for k in range(model.ndim)]
        param_names = list(param_names)[:model.ndim]
    return get_auxiliary_contbox_parameterization(param_names, model.loglike, model.transform, upoints[mask], weights, vectorized=True)


ONE_SIGMA_PERCENTILES = (15.8655, 84.1345)
INFORMATION_BINS = 40          # edges of the histogram behind information_gain_bits (39 bins over the cube)


def _importance_summary(points, weights):
    """the ``posterior`` entry of `reuse_samples` and the equally weighted samples it is taken from"""
    equal = resample_equal(points, weights)
    edges = np.linspace(0, 1, INFORMATION_BINS)
    bits = []
    for column in points.T:
        density = np.histogram(column, weights=weights, density=True, bins=edges)[0]
        bits.append(float(-np.log2((density + 0.001) * INFORMATION_BINS).sum() / INFORMATION_BINS))
    lo, hi = ONE_SIGMA_PERCENTILES
    summary = dict(mean=equal.mean(axis=0).tolist(), stdev=equal.std(axis=0).tolist(),
                   median=np.percentile(equal, 50, axis=0).tolist(), errlo=np.percentile(equal, lo, axis=0).tolist(),
                   errup=np.percentile(equal, hi, axis=0).tolist(), information_gain_bits=bits)
    return summary, equal


def reuse_samples(param_names, loglike, points, logl, logw=None, logz=0.0, logzerr=0.0, upoints=None, batchsize=128,
                  vectorized=False, log_weight_threshold=-10, **kwargs):
    """Reweight the points of an existing run onto a new likelihood (importance sampling) and return a results dict with the
    keys of the reference's ``reuse_samples``.  The points are visited in batches from the most to the least important under the
    old run (``logl + logw``); the visit ends after a batch whose every new weight lies more than ``-log_weight_threshold``
    below the best one over N (the points not visited keep weight 0).  ``logz`` is the log of the summed new weights, ``ess``
    Kish's effective sample size ``1 / sum w^2``, ``logzerr`` the old error combined in quadrature with ``ln(1 + s)``, s the
    standard error of the normalised weights about 1/N.  Nothing is printed."""
    evaluate = loglike if vectorized else vectorize(loglike)
    points = np.asarray(points)
    if points.ndim != 2:
        raise ValueError("points must be a 2d array (npoints, ndim), got shape %s" % (points.shape,))
    npoints = points.shape[0]
    old_logw = np.full(npoints, -math.log(npoints)) if logw is None else np.asarray(logw, dtype=float)
    old_logl = np.asarray(logl, dtype=float)
    if old_logl.shape != (npoints,) or old_logw.shape != (npoints,):
        raise ValueError("logl and logw must have one entry per point, got shapes %s and %s for %d points"
                         % (old_logl.shape, old_logw.shape, npoints))
    new_logl = np.full(npoints, -np.inf)
    new_logw = np.full(npoints, -np.inf)
    by_importance = np.argsort(-(old_logl + old_logw), kind="stable")
    ncall = 0
    for start in range(0, npoints, int(batchsize)):
        chosen = by_importance[start:start + int(batchsize)]
        new_logl[chosen] = evaluate(points[chosen])
        new_logw[chosen] = old_logw[chosen] + new_logl[chosen]
        ncall += len(chosen)
        negligible = np.nanmax(new_logw) - math.log(npoints) + log_weight_threshold
        if (new_logw[chosen] < negligible).all():
            break
    top = new_logw.max()
    weights = np.exp(new_logw - top)
    total = weights.sum()
    weights = weights / total
    spread = math.sqrt(((weights - 1.0 / npoints) ** 2).sum() / (npoints - 1))
    posterior, equal = _importance_summary(points, weights)
    best = int(np.argmax(new_logl))
    return dict(
        ncall=ncall, niter=npoints, logz=float(np.log(total) + top), logzerr=float(np.hypot(np.log1p(spread), logzerr)),
        ess=float(1.0 / (weights ** 2).sum()), posterior=posterior,
        weighted_samples=dict(upoints=upoints, points=points, weights=weights, logw=old_logw, logl=new_logl),
        samples=equal,
        maximum_likelihood=dict(logl=new_logl[best], point=points[best].tolist(),
                                point_untransformed=None if upoints is None else np.asarray(upoints)[best].tolist()),
        param_names=param_names,
    )


__all__ = ["get_auxiliary_problem", "get_extended_auxiliary_problem", "get_extended_auxiliary_independent_problem",
           "compute_quantile_intervals", "compute_quantile_intervals_refined", "get_auxiliary_contbox_parameterization",
           "reuse_samples", "from_results", "contbox_tail", "contbox_rows", "independent_tables", "header_text"]
