"""Example user models (ultranest_amd.devicemodel): the reference's example likelihoods restated as HIP device functions.

  rosenbrock  examples/testrosenbrock.py:10-16, written with the term order of the built-in kernel (csrc/mlf_loglike_dev.hpp
              loglike_row) and the transform order of k_elementwise_affine (m = x * 20; p = m + -10): where the built-in
              route evaluates row by row (odd d, d > 128) the two agree bit for bit
  funnel      examples/testfunnel.py: theta0 = log10 sigma with its own prior (x * 6 - 3), the rest x * 20 - 10; the data vector
              is the model's aux array
  gauss       docs/gauss.py:25-27 with the centres in aux (identity transform there; an affine one optionally)
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
