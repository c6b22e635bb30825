// mlf_priors_dev.hpp -- closed-form quantile functions (inverse CDFs) for the prior transform of a user model
// (ultranest_amd/priors.py).  The text of this header is the front part of a generated ``transform_source``: it is compiled
// at run time with the model (hiprtc, -O3 -std=c++17 -ffp-contract=off: no FMA is formed), it is NOT part of
// libmlfriends_hip.so and adds no C-ABI entry.  Plain HIP C++17: no inline assembly, no intrinsics, no data tables.
//
// Every function is __device__ __noinline__ (the precedent is truncnorm_draw of mlf_rwalk.hip): a generated transform of 1024
// columns is then 1024 calls, not 1024 inlined copies of normcdfinv.
//
// u lies in the open interval (0, 1): the region's cube test guarantees it on every route.  With t = 1 - u the subtraction is
// exact for u >= 0.5 (Sterbenz), so every upper tail is evaluated from t.  Constants named below as "from the host" are computed
// in binary64 by priors.py and arrive as hexadecimal floating literals.
//
//   family (parameters)              p(u)
//   Fixed(v)                         v                                                    (generated inline: no function)
//   Uniform(lo, hi)                  lo + u * w,  w = hi - lo from the host
//   LogUniform(lo, hi)               exp(a + u * w),  a = log(lo), w = log(hi) - log(lo) from the host
//   Normal(mu, sigma)                z = u <= 0.5 ? normcdfinv(u) : -normcdfinv(1 - u);  mu + sigma * z
//   TruncatedNormal(mu, sigma, lo, hi)
//                                    a = (lo - mu) / sigma, b = (hi - mu) / sigma, Fa = Phi(a), Fb = Phi(b), Qa = Phi(-a),
//                                    Qb = Phi(-b) from the host (0.5 * erfc(-+x / sqrt 2));  q = Fa + u * (Fb - Fa);
//                                    q <= 0.5: z = normcdfinv(q), else z = -normcdfinv(Qb + (1 - u) * (Qa - Qb));
//                                    z clamped to [a, b];  mu + sigma * z          (the smaller-tail form of truncnorm_draw)
//   LogNormal(mu, sigma)             exp(mu + sigma * z),  z as for Normal
//   HalfNormal(sigma)                u <= 0.5: sigma * (sqrt2 * erfinv(u)), else sigma * -normcdfinv(0.5 * (1 - u))
//   Exponential(scale)               scale * -log1p(-u)
//   Rayleigh(sigma)                  sigma * sqrt(-2 * log1p(-u))
//   Weibull(scale, k)                scale * exp(log(-log1p(-u)) / k)
//   Pareto(xm, alpha)                xm * exp(-log1p(-u) / alpha)
//   Cauchy(loc, scale)               loc + scale * (-cospi(u) / sinpi(u))
//   HalfCauchy(scale)                scale * (sinpi(0.5 * u) / cospi(0.5 * u))
//   Laplace(loc, b)                  u <= 0.5: loc + b * log(2 u), else loc - b * log(2 * (1 - u))
//   Logistic(loc, s)                 loc + s * (log(u) - log1p(-u))
//   Gumbel(loc, s)                   loc - s * log(-log(u))
//   Triangular(lo, mode, hi)         u <= c: lo + sqrt(u * c1), else hi - sqrt((1 - u) * c2);  c = (mode - lo) / (hi - lo),
//                                    c1 = (hi - lo) * (mode - lo), c2 = (hi - lo) * (hi - mode) from the host
//   Sine()  (density ~ sin on [0, pi])          2 * atan2(sqrt(u), sqrt(1 - u))
//   Cosine()  (density ~ cos on [-pi/2, pi/2])  atan2(2 u - 1, 2 * sqrt(u * (1 - u)))
//
// Sine and Cosine are 2 asin(sqrt u) and asin(2 u - 1) written through atan2: asin has an infinite slope at +-1, where sqrt(u)
// (u -> 1) and 2 u - 1 (u -> 0) have lost the bits that say how far from +-1 they are; both atan2 arguments keep their relative
// accuracy in both tails, so the quantile keeps its accuracy there without a seam between branches.
//
// Block priors (generated as straight-line statements by priors.py from the two functions marked "block"):
//   MultivariateNormal(mean, cov)    z_k into p[k] for the block's columns, then for i = n-1 down to 0
//                                    p[i] = mean_i + (((L_i0 * p[0]) + L_i1 * p[1]) + ... + L_ii * p[i]),  L = cholesky(cov)
//   OrderedUniform(lo, hi, n)        t_(n-1) = exp(log(u_(n-1)) / n);  t_k = t_(k+1) * exp(log(u_k) / (k + 1)), k = n-2 .. 0;
//                                    p_k = lo + t_k * w
#ifndef MLF_PRIORS_DEV_HPP
#define MLF_PRIORS_DEV_HPP

// standard normal quantile on the side of the smaller tail; inlined into the three functions that use it, so that none of
// the __noinline__ functions makes a call of its own (a leaf function needs no stack frame)
__device__ __forceinline__ double mlf_prior_z_leaf(double u) {
  return u <= 0.5 ? normcdfinv(u) : -normcdfinv(1.0 - u);
}

// (block: MultivariateNormal writes it into its columns first)
__device__ __noinline__ double mlf_prior_z(double u) {
  return mlf_prior_z_leaf(u);
}

__device__ __noinline__ double mlf_prior_uniform(double u, double lo, double w) {
  return lo + u * w;
}

__device__ __noinline__ double mlf_prior_loguniform(double u, double a, double w) {
  return exp(a + u * w);
}

__device__ __noinline__ double mlf_prior_normal(double u, double mu, double sigma) {
  return mu + sigma * mlf_prior_z_leaf(u);
}

__device__ __noinline__ double mlf_prior_truncnormal(double u, double mu, double sigma, double a, double b, double Fa, double Fb,
                                                     double Qa, double Qb) {
  const double q = Fa + u * (Fb - Fa);
  double z;
  if (q <= 0.5) {
    z = normcdfinv(q);
  } else {
    z = -normcdfinv(Qb + (1.0 - u) * (Qa - Qb));
  }
  z = fmin(fmax(z, a), b);
  return mu + sigma * z;
}

__device__ __noinline__ double mlf_prior_lognormal(double u, double mu, double sigma) {
  return exp(mu + sigma * mlf_prior_z_leaf(u));
}

__device__ __noinline__ double mlf_prior_halfnormal(double u, double sigma) {
  if (u <= 0.5) return sigma * (0x1.6a09e667f3bcdp+0 * erfinv(u));
  return sigma * -normcdfinv(0.5 * (1.0 - u));
}

__device__ __noinline__ double mlf_prior_exponential(double u, double scale) {
  return scale * -log1p(-u);
}

__device__ __noinline__ double mlf_prior_rayleigh(double u, double sigma) {
  return sigma * sqrt(-2.0 * log1p(-u));
}

__device__ __noinline__ double mlf_prior_weibull(double u, double scale, double k) {
  return scale * exp(log(-log1p(-u)) / k);
}

__device__ __noinline__ double mlf_prior_pareto(double u, double xm, double alpha) {
  return xm * exp(-log1p(-u) / alpha);
}

__device__ __noinline__ double mlf_prior_cauchy(double u, double loc, double scale) {
  return loc + scale * (-cospi(u) / sinpi(u));
}

__device__ __noinline__ double mlf_prior_halfcauchy(double u, double scale) {
  return scale * (sinpi(0.5 * u) / cospi(0.5 * u));
}

__device__ __noinline__ double mlf_prior_laplace(double u, double loc, double b) {
  if (u <= 0.5) return loc + b * log(2.0 * u);
  return loc - b * log(2.0 * (1.0 - u));
}

__device__ __noinline__ double mlf_prior_logistic(double u, double loc, double s) {
  return loc + s * (log(u) - log1p(-u));
}

__device__ __noinline__ double mlf_prior_gumbel(double u, double loc, double s) {
  return loc - s * log(-log(u));
}

__device__ __noinline__ double mlf_prior_triangular(double u, double lo, double hi, double c, double c1, double c2) {
  if (u <= c) return lo + sqrt(u * c1);
  return hi - sqrt((1.0 - u) * c2);
}

__device__ __noinline__ double mlf_prior_sine(double u) {
  return 2.0 * atan2(sqrt(u), sqrt(1.0 - u));
}

__device__ __noinline__ double mlf_prior_cosine(double u) {
  return atan2(2.0 * u - 1.0, 2.0 * sqrt(u * (1.0 - u)));
}

// one factor of the ordered uniform vector (block): exp(log(u) / m)
__device__ __noinline__ double mlf_prior_ordered_factor(double u, double m) {
  return exp(log(u) / m);
}

#endif  // MLF_PRIORS_DEV_HPP
