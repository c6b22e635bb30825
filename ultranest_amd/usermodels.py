"""Example user models (ultranest_amd.devicemodel): the reference's example likelihoods restated as HIP device functions.

  rosenbrock  examples/testrosenbrock.py:10-16, written with the term order of the built-in kernel (csrc/mlf_loglike_dev.hpp
              loglike_row) and the transform order of k_elementwise_affine (m = x * 20; p = m + -10): where the built-in
              route evaluates row by row (odd d, d > 128) the two agree bit for bit
  funnel      examples/testfunnel.py: theta0 = log10 sigma with its own prior (x * 6 - 3), the rest x * 20 - 10; the data vector
              is the model's aux array
  gauss       docs/gauss.py:25-27 with the centres in aux (identity transform there; an affine one optionally)
  gauss_derived  gauss with three derived parameters (``DeviceModel(..., nderived=3)``) whose arithmetic numpy reproduces bit for
              bit: q0 = p[0] + p[1], q1 = p[0] * p[1], q2 = the sum of p[k] in ascending k from 0.0
              (``np.cumsum(p, axis=1)[:, -1]``); no log or exp
  gauss_normal_prior  gauss under independent Normal priors from the prior library (``ultranest_amd.priors``), with its
              analytic evidence
  hierarchical_gauss  mu ~ Normal(0, 1), theta_i ~ Normal(Ref("mu"), 0.5): a prior whose location is another parameter
              (``priors.Ref``), Gaussian data around the theta_i, with its analytic evidence

Likelihoods summed over data terms (``DeviceModel(..., nterms=K)``: one wave per row, the lanes split the terms), each with a
default-form twin that computes the same terms in a serial loop k = 0..K-1 inside ``mlf_user_loglike``:

  linear_sum     weighted least squares of a linear model: aux = design matrix X[k, j] (K x d), data y_k, weights
                 w_k = 1 / sigma_k (the inverse is stored: nothing is divided on the device).  m = sum_j p_j X_kj from 0.0 in
                 ascending j, r = (y_k - m) * w_k, term = -0.5 * r * r: only +, - and *, so numpy restates every term bit for bit
  staircase_sum  term = -floor(fabs(p[k % d] - c_k) * 8.0): every term is a small integer, so every summation order gives the
                 same bits and the summed model equals its twin bit for bit -- whole sampler runs can be compared between
                 the two forms without a threshold decision hanging on a last bit

Likelihoods of several sums and a final function (``DeviceModel(..., nterms=K, nsums=M)``), each with a default-form twin whose
``mlf_user_loglike`` adds the same terms serially, k = 0..K-1, into M sums and calls the same finish text:

  amplitude_sum   M = 3: the linear model of linear_sum with its overall amplitude profiled out analytically.  aux as in
                  linear_data; f_k = X_k . p (from 0.0 in ascending j), a = w_k * y_k, b = w_k * f_k, terms a * a, a * b, b * b
                  (w^2 y^2, w^2 y f, w^2 f^2: only + and *, so numpy restates every term bit for bit);
                  L = -0.5 * (s0 - s1 * s1 / s2) - 0.5 * log(s2)
  staircase3_sum  M = 3: a = fabs(p[k % d] - c_k) on three scales, terms -floor(a * 8), floor(a * 4), -floor(a * 2): small
                  integers, so every partial sum is exact in any order; L = s0 - s1 * s1 / (1.0 - s2) with s2 <= 0 (+ - * /
                  only, the denominator is at least 1), so the two forms agree bit for bit

Gaussian likelihoods with a dense covariance (``DeviceModel(..., ncov=n)``: one workgroup per row factorises the matrix in LDS):

  gp_sqexp        a Gaussian process over ndata points: aux = inputs x_i, then data y_i; parameters ln amplitude, ln length scale,
                  ln jitter, mean; K_ij = a^2 exp(-(x_i - x_j)^2 / (2 l^2)) + delta_ij s^2, r_i = y_i - mean; ``affine=True`` puts
                  a uniform prior box on the four (GP_PRIOR_LO, GP_PRIOR_WIDTH)
  gp_sqexp_twin   the same arithmetic in the same order (the contract of csrc/mlf_user_cov.hpp) as a default-form
                  ``mlf_user_loglike`` over a private array, ndata <= 12: the two agree bit for bit on every route
"""
import numpy as np

from .devicemodel import DeviceModel

ROSENBROCK_LOGLIKE = r"""
__device__ double mlf_user_loglike(const double *x, int d, const double *aux, long long naux) {
  double s = 0.0;
  for (int k = 0; k + 1 < d; ++k) {
    const double av = x[k], bv = x[k + 1];
    const double t = bv - av * av;
    const double w = 1.0 - av;
    s += 100.0 * (t * t) + w * w;
  }
  return -2.0 * s;
}
"""

ROSENBROCK_TRANSFORM = r"""
__device__ void mlf_user_transform(const double *u, double *p, int d, const double *aux, long long naux) {
  for (int k = 0; k < d; ++k) {
    const double m = u[k] * 20.0;
    p[k] = m + -10.0;
  }
}
"""

FUNNEL_LOGLIKE = r"""
__device__ double mlf_user_loglike(const double *p, int d, const double *aux, long long naux) {
  const double sigma = pow(10.0, p[0]);
  double s = 0.0;
  for (int k = 1; k < d && k - 1 < naux; ++k) {
    const double z = (p[k] - aux[k - 1]) / sigma;
    s += z * z;
  }
  return -0.5 * s - 0.5 * log(2.0 * 3.141592653589793 * sigma * sigma) * (double)naux;
}
"""

FUNNEL_TRANSFORM = r"""
__device__ void mlf_user_transform(const double *u, double *p, int d, const double *aux, long long naux) {
  p[0] = u[0] * 6.0 - 3.0;
  for (int k = 1; k < d; ++k) p[k] = u[k] * 20.0 - 10.0;
}
"""

GAUSS_LOGLIKE = r"""
#define MLF_GAUSS_SIGMA %r
__device__ double mlf_user_loglike(const double *p, int d, const double *aux, long long naux) {
  const double sigma = MLF_GAUSS_SIGMA;
  double s = 0.0;
  for (int k = 0; k < d && k < naux; ++k) {
    const double z = (p[k] - aux[k]) / sigma;
    s += z * z;
  }
  return -0.5 * s - 0.5 * log(2.0 * 3.141592653589793 * sigma * sigma) * (double)d;
}
"""

# the affine transform of the Rosenbrock (u * 20 - 10), as a prior for the Gaussian of the benchmark
AFFINE_TRANSFORM = ROSENBROCK_TRANSFORM


def rosenbrock(ndim):
    return DeviceModel(ndim, ROSENBROCK_LOGLIKE, ROSENBROCK_TRANSFORM, name="rosenbrock%d" % ndim)


def funnel_data(ndim, sigma=0.5, seed=2):
    """examples/testfunnel.py: data = normal(sin(arange(n) / 2), sigma) of the ndim - 1 non-sigma parameters"""
    rs = np.random.RandomState(seed)
    return rs.normal(np.sin(np.arange(ndim - 1) / 2.), sigma)


def funnel(ndim, data=None):
    data = funnel_data(ndim) if data is None else np.asarray(data, dtype=float)
    return DeviceModel(ndim, FUNNEL_LOGLIKE, FUNNEL_TRANSFORM, aux=data, name="funnel%d" % ndim)


def gauss_centers(ndim, sigma=0.1):
    width = max(0, 1 - 5 * sigma)
    return (np.sin(np.arange(ndim) / 2.) * width + 1.) / 2.


def gauss(ndim, sigma=0.1, affine=False):
    return DeviceModel(ndim, GAUSS_LOGLIKE % float(sigma), AFFINE_TRANSFORM if affine else None,
                       aux=gauss_centers(ndim, sigma), name="gauss%d" % ndim)


def gauss_normal_prior(ndim, sigma=0.1, prior_sigma=1.0, prior_mean=0.5):
    """The normalised Gaussian of `gauss` (centres c_k = gauss_centers, width sigma) under independent priors
    ``Normal(m_k, t)`` from ``ultranest_amd.priors`` (m_k = prior_mean, a number or one per column; t = prior_sigma).  Returns
    ``(model, lnZ)`` with the analytic evidence ln Z = sum_k ln N(c_k; m_k, sqrt(sigma^2 + t^2)): the convolution of two
    Gaussians.  With the defaults every centre lies within 0.25 t of its prior's mean: the posterior sits in the prior's bulk."""
    from . import priors
    centers = gauss_centers(ndim, sigma)
    means = np.broadcast_to(np.asarray(prior_mean, dtype=float), (ndim,))
    pt = priors.PriorTransform([priors.Normal(m, prior_sigma, name="x%d" % k) for k, m in enumerate(means)])
    model = pt.model(GAUSS_LOGLIKE % float(sigma), aux=centers, name="gauss_normal_prior%d" % ndim)
    var = float(sigma) ** 2 + float(prior_sigma) ** 2
    lnz = float(np.sum(-0.5 * (centers - means) ** 2 / var - 0.5 * np.log(2 * np.pi * var)))
    return model, lnz


HIER_GAUSS_LOGLIKE = r"""
#define MLF_HIER_SIGMA %r
__device__ double mlf_user_loglike(const double *p, int d, const double *aux, long long naux) {
  const double sigma = MLF_HIER_SIGMA;
  double s = 0.0;
  for (int k = 1; k < d && k - 1 < naux; ++k) {
    const double z = (p[k] - aux[k - 1]) / sigma;
    s += z * z;
  }
  return -0.5 * s - 0.5 * log(2.0 * 3.141592653589793 * sigma * sigma) * (double)(d - 1);
}
"""


def hierarchical_gauss_data(ngroups):
    """the fixed group means y_i of `hierarchical_gauss`: within one prior sigma of 0, spread over 0.8"""
    return 0.3 + 0.8 * np.sin(1.0 + 2.0 * np.arange(ngroups)) / 2.


def hierarchical_gauss(ngroups, tau=0.5, sigma=0.3):
    """A hierarchical model whose prior needs ``priors.Ref``: mu ~ Normal(0, 1), theta_i ~ Normal(Ref("mu"), tau) for
    i < ngroups, likelihood prod_i N(y_i | theta_i, sigma) with the fixed y of `hierarchical_gauss_data` in aux (columns: mu,
    theta_0, ...).  Returns ``(model, lnZ)``; marginally y ~ N(0, (tau^2 + sigma^2) I + 1 1^T), so with v = tau^2 + sigma^2 and
    n = ngroups, ln Z = -0.5 * (y.y / v - (sum y)^2 / (v (v + n))) - 0.5 * (n ln(2 pi) + (n - 1) ln v + ln(v + n))
    (Sherman-Morrison and the matrix determinant lemma).  With the defaults v = 0.34."""
    from . import priors
    if ngroups < 1:
        raise ValueError("hierarchical_gauss needs at least one group")
    y = hierarchical_gauss_data(ngroups)
    pt = priors.PriorTransform([priors.Normal(0.0, 1.0, name="mu")]
                               + [priors.Normal(priors.Ref("mu"), tau, name="theta%d" % i) for i in range(ngroups)])
    model = pt.model(HIER_GAUSS_LOGLIKE % float(sigma), aux=y, name="hierarchical_gauss%d" % ngroups)
    v, n = float(tau) ** 2 + float(sigma) ** 2, ngroups
    lnz = float(-0.5 * (y.dot(y) / v - y.sum() ** 2 / (v * (v + n))) - 0.5 * (n * np.log(2 * np.pi) + (n - 1) * np.log(v) + np.log(v + n)))
    return model, lnz


GAUSS_DERIVED = r"""
__device__ void mlf_user_derived(const double *p, int d, double *q, int nq, const double *aux, long long naux) {
  q[0] = p[0] + p[1];
  q[1] = p[0] * p[1];
  double s = 0.0;
  for (int k = 0; k < d; ++k) s = s + p[k];
  q[2] = s;
}
"""


def gauss_derived(ndim, sigma=0.1, affine=False):
    """`gauss` with the derived columns p0 + p1, p0 * p1 and sum_k p_k (ndim >= 2); `gauss_derived_columns` restates them"""
    if ndim < 2:
        raise ValueError("gauss_derived reads p[0] and p[1]: ndim must be at least 2")
    return DeviceModel(ndim, GAUSS_LOGLIKE % float(sigma), AFFINE_TRANSFORM if affine else None,
                       aux=gauss_centers(ndim, sigma), name="gauss_derived%d" % ndim, nderived=3, derived_source=GAUSS_DERIVED)


def gauss_derived_columns(p):
    """the three derived columns of `gauss_derived` in numpy, bit for bit (cumsum adds sequentially; np.sum is pairwise)"""
    p = np.asarray(p, dtype=float)
    return np.column_stack([p[:, 0] + p[:, 1], p[:, 0] * p[:, 1], np.cumsum(p, axis=1)[:, -1]])


LINEAR_TERM = r"""
#define MLF_LINEAR_K %dLL
__device__ inline double mlf_linear_term(const double *p, int d, const double *aux, long long k) {
  const double *x = aux + k * d;
  double m = 0.0;
  for (int j = 0; j < d; ++j) m = m + p[j] * x[j];
  const double r = (aux[MLF_LINEAR_K * d + k] - m) * aux[MLF_LINEAR_K * d + MLF_LINEAR_K + k];
  return -0.5 * r * r;
}
"""

STAIRCASE_TERM = r"""
#define MLF_STAIRCASE_K %dLL
__device__ inline double mlf_staircase_term(const double *p, int d, const double *aux, long long k) {
  return -floor(fabs(p[(int)(k %% d)] - aux[k]) * 8.0);
}
"""

# the two forms around a term function NAME(p, d, aux, k) with K terms
SUMMED_LOGLIKE = r"""
__device__ double mlf_user_loglike_term(const double *p, int d, const double *aux, long long naux, long long k) {
  return %(name)s(p, d, aux, k);
}
"""

TWIN_LOGLIKE = r"""
__device__ double mlf_user_loglike(const double *p, int d, const double *aux, long long naux) {
  double s = 0.0;
  for (long long k = 0; k < %(K)s; ++k) s = s + %(name)s(p, d, aux, k);
  return s;
}
"""


def _two_forms(term_source, name, K, ndim, ndata, aux, affine, summed, label):
    if summed:
        source = term_source % ndata + SUMMED_LOGLIKE % dict(name=name)
    else:
        source = term_source % ndata + TWIN_LOGLIKE % dict(name=name, K=K)
    return DeviceModel(ndim, source, AFFINE_TRANSFORM if affine else None, aux=aux,
                       name="%s%s%dx%d" % (label, "_sum" if summed else "_twin", ndim, ndata),
                       nterms=int(ndata) if summed else None)


def linear_data(ndim, ndata, seed=1):
    """(X (ndata, ndim), y (ndata), w (ndata) = 1 / sigma) of linear_sum and its twin"""
    rs = np.random.RandomState(seed)
    X = rs.normal(size=(ndata, ndim))
    sigma = rs.uniform(0.5, 2.0, size=ndata)
    y = X.dot(rs.normal(size=ndim)) + sigma * rs.normal(size=ndata)
    return X, y, 1.0 / sigma


def linear_aux(ndim, ndata, seed=1):
    X, y, w = linear_data(ndim, ndata, seed)
    return np.concatenate([X.ravel(), y, w])


def linear_sum(ndim, ndata, seed=1, affine=False):
    """summed form: K = ndata terms, one wave per row"""
    return _two_forms(LINEAR_TERM, "mlf_linear_term", "MLF_LINEAR_K", ndim, ndata, linear_aux(ndim, ndata, seed), affine, True,
                      "linear")


def linear_twin(ndim, ndata, seed=1, affine=False):
    """default form of linear_sum: the same terms, k = 0..K-1 serially in one thread per row"""
    return _two_forms(LINEAR_TERM, "mlf_linear_term", "MLF_LINEAR_K", ndim, ndata, linear_aux(ndim, ndata, seed), affine, False,
                      "linear")


def staircase_data(ndim, ndata, seed=1, affine=False):
    """the centres c_k, drawn where the parameters live (the cube, or the affine transform's [-10, 10))"""
    c = np.random.RandomState(seed).uniform(size=ndata)
    return c * 20.0 - 10.0 if affine else c


def staircase_sum(ndim, ndata, seed=1, affine=False):
    return _two_forms(STAIRCASE_TERM, "mlf_staircase_term", "MLF_STAIRCASE_K", ndim, ndata,
                      staircase_data(ndim, ndata, seed, affine), affine, True, "staircase")


def staircase_twin(ndim, ndata, seed=1, affine=False):
    return _two_forms(STAIRCASE_TERM, "mlf_staircase_term", "MLF_STAIRCASE_K", ndim, ndata,
                      staircase_data(ndim, ndata, seed, affine), affine, False, "staircase")


AMPLITUDE_TERMS = r"""
#define MLF_AMPLITUDE_K %dLL
__device__ inline void mlf_amplitude_terms(const double *p, int d, const double *aux, long long k, double *t) {
  const double *x = aux + k * d;
  double f = 0.0;
  for (int j = 0; j < d; ++j) f = f + p[j] * x[j];
  const double w = aux[MLF_AMPLITUDE_K * d + MLF_AMPLITUDE_K + k];
  const double a = w * aux[MLF_AMPLITUDE_K * d + k], b = w * f;
  t[0] = a * a;
  t[1] = a * b;
  t[2] = b * b;
}
__device__ inline double mlf_amplitude_finish(const double *s) {
  return -0.5 * (s[0] - s[1] * s[1] / s[2]) - 0.5 * log(s[2]);
}
"""

STAIRCASE3_TERMS = r"""
#define MLF_STAIRCASE3_K %dLL
__device__ inline void mlf_staircase3_terms(const double *p, int d, const double *aux, long long k, double *t) {
  const double a = fabs(p[(int)(k %% d)] - aux[k]);
  t[0] = -floor(a * 8.0);
  t[1] = floor(a * 4.0);
  t[2] = -floor(a * 2.0);
}
__device__ inline double mlf_staircase3_finish(const double *s) {
  return s[0] - s[1] * s[1] / (1.0 - s[2]);
}
"""

# the two forms around NAME_terms(p, d, aux, k, t) and NAME_finish(s) with K terms and M sums
MULTISUM_LOGLIKE = r"""
__device__ void mlf_user_loglike_terms(const double *p, int d, const double *aux, long long naux, long long k, double *t) {
  %(name)s_terms(p, d, aux, k, t);
}
__device__ double mlf_user_loglike_finish(const double *s, int nsums, const double *p, int d, const double *aux, long long naux) {
  return %(name)s_finish(s);
}
"""

MULTISUM_TWIN_LOGLIKE = r"""
__device__ double mlf_user_loglike(const double *p, int d, const double *aux, long long naux) {
  double s[%(M)d];
  for (int j = 0; j < %(M)d; ++j) s[j] = 0.0;
  for (long long k = 0; k < %(K)s; ++k) {
    double t[%(M)d];
    %(name)s_terms(p, d, aux, k, t);
    for (int j = 0; j < %(M)d; ++j) s[j] = s[j] + t[j];
  }
  return %(name)s_finish(s);
}
"""


def _two_multisum_forms(terms_source, name, K, M, ndim, ndata, aux, affine, summed, label):
    if summed:
        source = terms_source % ndata + MULTISUM_LOGLIKE % dict(name=name)
    else:
        source = terms_source % ndata + MULTISUM_TWIN_LOGLIKE % dict(name=name, K=K, M=M)
    return DeviceModel(ndim, source, AFFINE_TRANSFORM if affine else None, aux=aux,
                       name="%s%s%dx%d" % (label, "_sum" if summed else "_twin", ndim, ndata),
                       nterms=int(ndata) if summed else None, nsums=M if summed else None)


def amplitude_sum(ndim, ndata, seed=1, affine=False):
    """three sums and a finish: K = ndata terms, one wave per row"""
    return _two_multisum_forms(AMPLITUDE_TERMS, "mlf_amplitude", "MLF_AMPLITUDE_K", 3, ndim, ndata,
                               linear_aux(ndim, ndata, seed), affine, True, "amplitude")


def amplitude_twin(ndim, ndata, seed=1, affine=False):
    """default form of amplitude_sum: the same terms, k = 0..K-1 serially in one thread per row, the same finish"""
    return _two_multisum_forms(AMPLITUDE_TERMS, "mlf_amplitude", "MLF_AMPLITUDE_K", 3, ndim, ndata,
                               linear_aux(ndim, ndata, seed), affine, False, "amplitude")


def staircase3_sum(ndim, ndata, seed=1, affine=False):
    return _two_multisum_forms(STAIRCASE3_TERMS, "mlf_staircase3", "MLF_STAIRCASE3_K", 3, ndim, ndata,
                               staircase_data(ndim, ndata, seed, affine), affine, True, "staircase3")


def staircase3_twin(ndim, ndata, seed=1, affine=False):
    return _two_multisum_forms(STAIRCASE3_TERMS, "mlf_staircase3", "MLF_STAIRCASE3_K", 3, ndim, ndata,
                               staircase_data(ndim, ndata, seed, affine), affine, False, "staircase3")


# ---- Gaussian likelihoods with a dense covariance (``DeviceModel(..., ncov=n)``: one workgroup per row) ----------------------------
# gp_sqexp: a Gaussian process with a squared-exponential kernel plus jitter over ndata points.  aux = inputs x_i, then data y_i;
# parameters ln amplitude, ln length scale, ln jitter, mean; K_ij = a^2 exp(-(x_i - x_j)^2 / (2 l^2)) + delta_ij s^2, r_i = y_i - mean.
# Each entry recomputes a, l, s from p (pure functions of their arguments, as the contract asks).

GP_SQEXP = r"""
#define MLF_GP_N %d
__device__ inline double mlf_gp_cov(const double *p, const double *aux, int i, int j) {
  const double a = exp(p[0]), l = exp(p[1]);
  const double dx = aux[i] - aux[j];
  double v = (a * a) * exp(-(dx * dx) / (2.0 * (l * l)));
  if (i == j) {
    const double s = exp(p[2]);
    v = v + s * s;
  }
  return v;
}
__device__ inline double mlf_gp_resid(const double *p, const double *aux, int i) { return aux[MLF_GP_N + i] - p[3]; }
"""

GP_COV_LOGLIKE = r"""
__device__ double mlf_user_cov(const double *p, int d, const double *aux, long long naux, int i, int j) { return mlf_gp_cov(p, aux, i, j); }
__device__ double mlf_user_resid(const double *p, int d, const double *aux, long long naux, int i) { return mlf_gp_resid(p, aux, i); }
"""

# the arithmetic contract of csrc/mlf_user_cov.hpp in one thread, over a private array
GP_TWIN_LOGLIKE = r"""
__device__ double mlf_user_loglike(const double *p, int d, const double *aux, long long naux) {
  const int N = MLF_GP_N;
  double A[(MLF_GP_N + 1) * (MLF_GP_N + 2) / 2], diag[MLF_GP_N];
  for (int i = 0; i <= N; ++i)
    for (int j = 0; j <= i; ++j)
      A[i * (i + 1) / 2 + j] = i < N ? mlf_gp_cov(p, aux, i, j) : j < N ? mlf_gp_resid(p, aux, j) : 0.0;
  for (int k = 0; k < N; ++k) {
    const double piv = A[k * (k + 1) / 2 + k];
    if (!(piv > 0.0)) return piv != piv ? piv : -__builtin_inf();
    const double lkk = sqrt(piv);
    diag[k] = lkk;
    for (int i = k + 1; i <= N; ++i) A[i * (i + 1) / 2 + k] = A[i * (i + 1) / 2 + k] / lkk;
    for (int i = k + 1; i <= N; ++i)
      for (int j = k + 1; j <= i && j < N; ++j) {
        const double m = A[i * (i + 1) / 2 + k] * A[j * (j + 1) / 2 + k];
        A[i * (i + 1) / 2 + j] = A[i * (i + 1) / 2 + j] - m;
      }
  }
  double quad = 0.0, h = 0.0;
  for (int k = 0; k < N; ++k) quad = quad + A[N * (N + 1) / 2 + k] * A[N * (N + 1) / 2 + k];
  for (int k = 0; k < N; ++k) h = h + log(diag[k]);
  return ((-0.5 * quad) - h) - (double)N * 0.91893853320467274178;
}
"""

# the prior box of gp_sqexp(affine=True): ln a in [-1, 1], ln l in [-1, 2], ln s in [-2, 0], mean in [-1, 1]
GP_PRIOR_LO = (-1.0, -1.0, -2.0, -1.0)
GP_PRIOR_WIDTH = (2.0, 3.0, 2.0, 2.0)
GP_TRANSFORM = r"""
__device__ void mlf_user_transform(const double *u, double *p, int d, const double *aux, long long naux) {
  p[0] = u[0] * 2.0 + -1.0;
  p[1] = u[1] * 3.0 + -1.0;
  p[2] = u[2] * 2.0 + -2.0;
  p[3] = u[3] * 2.0 + -1.0;
}
"""


def gp_data(ndata, seed=1):
    """(x (ndata) ascending in [0, 10), y (ndata)) of gp_sqexp and its twin: a sine with noise of 0.3"""
    rs = np.random.RandomState(seed)
    x = np.sort(rs.uniform(0.0, 10.0, size=ndata))
    return x, np.sin(x) + 0.3 * rs.normal(size=ndata)


def gp_sqexp(ndata, seed=1, affine=False):
    """covariance form: one workgroup per row factorises the ndata x ndata kernel matrix in LDS"""
    return DeviceModel(4, GP_SQEXP % ndata + GP_COV_LOGLIKE, GP_TRANSFORM if affine else None, aux=np.concatenate(gp_data(ndata, seed)),
                       name="gp_sqexp%d" % ndata, ncov=int(ndata))


def gp_sqexp_twin(ndata, seed=1, affine=False):
    """default form of gp_sqexp: the same arithmetic in the same order in one thread per row, over a private array (ndata <= 12)"""
    if not 1 <= ndata <= 12:
        raise ValueError("gp_sqexp_twin holds the factor in a thread's private memory: ndata must be 1 to 12, got %r" % (ndata,))
    return DeviceModel(4, GP_SQEXP % ndata + GP_TWIN_LOGLIKE, GP_TRANSFORM if affine else None, aux=np.concatenate(gp_data(ndata, seed)),
                       name="gp_sqexp_twin%d" % ndata)
