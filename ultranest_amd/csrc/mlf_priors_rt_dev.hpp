// mlf_priors_rt_dev.hpp -- priors whose parameters are other columns of the row (priors.Ref) and quantile functions given as
// a table (priors.Tabulated).  Its text follows mlf_priors_dev.hpp (and mlf_priors_special_dev.hpp, where present) in a
// generated ``transform_source`` only when the list holds a Ref or a Tabulated; it uses normcdfinv and nothing else of the
// earlier headers.  Same rules: compiled with the model (hiprtc, -O3 -std=c++17 -ffp-contract=off: no FMA is formed), plain
// HIP C++17, no inline assembly, no intrinsics; every __noinline__ function is a leaf (it calls no other __noinline__
// function), so the wrapper kernel keeps no stack.
//
// Run-time parameters.  A parameter read from p[j] has passed the support check of priors.py, which cannot exclude a value
// that rounded to 0, overflowed to inf or is the NaN of a failed parent.  The contract: a location must be finite, a
// scale-like parameter >= 0 and finite (0 is the point mass at loc), a strictly positive parameter > 0 and finite, bounds
// ordered; otherwise the column is NaN, and with it every column that reads it.  A NaN likelihood fails L > Lmin on every
// route, so such a row is never kept.
//
// Pass-through families (Normal, LogNormal, the one-scale, scale-shape and loc-scale families, the Gamma / InverseGamma scale,
// the StudentT loc and scale) call the existing mlf_prior_* function; the generated text wraps each run-time argument in one
// of the three guards below, which return the value or NaN.  With Fixed parents such a column is bit for bit the column of
// the constant-parameter prior.
//
// Four families take constants that the host computes for a constant-parameter prior; here the same expressions are
// evaluated on the device:
//   mlf_prior_rt_uniform(u, lo, hi)               lo + u * (hi - lo)
//   mlf_prior_rt_loguniform(u, lo, hi)            a = log(lo);  exp(a + u * (log(hi) - a))
//   mlf_prior_rt_truncnormal(u, mu, sigma, lo, hi)
//                                                 a = (lo - mu) / sigma, b = (hi - mu) / sigma, Fa = 0.5 * erfc(-a / sqrt2),
//                                                 Fb = 0.5 * erfc(-b / sqrt2), Qa = 0.5 * erfc(a / sqrt2), Qb = 0.5 * erfc(b / sqrt2);
//                                                 q = Fa + u * (Fb - Fa);  q <= 0.5: z = normcdfinv(q), else
//                                                 z = -normcdfinv(Qb + (1 - u) * (Qa - Qb));  z clamped to [a, b];  mu + sigma * z;
//                                                 NaN if neither Fb > Fa nor Qa > Qb (no probability between the bounds)
//   mlf_prior_rt_triangular(u, lo, mode, hi)      w = hi - lo, c = (mode - lo) / w, c1 = w * (mode - lo), c2 = w * (hi - mode);
//                                                 u <= c: lo + sqrt(u * c1), else hi - sqrt((1 - u) * c2)
//
// Tables.  mlf_prior_table(u, t, n, steps): t = [c_0 .. c_(n-1) | x_0 .. x_(n-1) | s_0 .. s_(n-2)], the knots of the CDF
// F(x_k) = c_k (c_0 = 0, c_(n-1) = 1, both non-decreasing) and the slopes s_k = (x_(k+1) - x_k) / (c_(k+1) - c_k) from the
// host (0 on a flat CDF segment); steps = ceil(log2(n - 1)).  k = the largest index <= n - 2 with c_k <= u, found by a
// branch-free bisection with exactly `steps` probes; dl = u - c_k, dr = c_(k+1) - u;
//   p = dl <= dr ? x_k + dl * s_k : x_(k+1) - dr * s_k
// (from the nearer knot: both ends of a segment are met exactly and the two forms meet in its middle).  Every load has an
// index in [0, 3 n - 2] for every u, NaN included.
#ifndef MLF_PRIORS_RT_DEV_HPP
#define MLF_PRIORS_RT_DEV_HPP

#define MLF_PRIOR_RT_MAX 0x1.fffffffffffffp+1023
#define MLF_PRIOR_RT_NAN (MLF_PRIOR_RT_MAX * 2.0 - MLF_PRIOR_RT_MAX * 2.0)

// a location: finite
__device__ __forceinline__ double mlf_prior_rt_loc(double v) {
  return fabs(v) <= MLF_PRIOR_RT_MAX ? v : MLF_PRIOR_RT_NAN;
}

// a scale-like parameter: >= 0 and finite
__device__ __forceinline__ double mlf_prior_rt_scale(double v) {
  return (v >= 0.0 && v <= MLF_PRIOR_RT_MAX) ? v : MLF_PRIOR_RT_NAN;
}

// a strictly positive parameter: > 0 and finite
__device__ __forceinline__ double mlf_prior_rt_pos(double v) {
  return (v > 0.0 && v <= MLF_PRIOR_RT_MAX) ? v : MLF_PRIOR_RT_NAN;
}

__device__ __noinline__ double mlf_prior_rt_uniform(double u, double lo, double hi) {
  const double w = hi - lo;
  if (!(fabs(lo) <= MLF_PRIOR_RT_MAX && fabs(hi) <= MLF_PRIOR_RT_MAX && lo <= hi && w <= MLF_PRIOR_RT_MAX)) return MLF_PRIOR_RT_NAN;
  return lo + u * w;
}

__device__ __noinline__ double mlf_prior_rt_loguniform(double u, double lo, double hi) {
  if (!(lo > 0.0 && lo <= hi && hi <= MLF_PRIOR_RT_MAX)) return MLF_PRIOR_RT_NAN;
  const double a = log(lo);
  return exp(a + u * (log(hi) - a));
}

__device__ __noinline__ double mlf_prior_rt_truncnormal(double u, double mu, double sigma, double lo, double hi) {
  if (!(fabs(mu) <= MLF_PRIOR_RT_MAX && sigma > 0.0 && sigma <= MLF_PRIOR_RT_MAX && fabs(lo) <= MLF_PRIOR_RT_MAX &&
        fabs(hi) <= MLF_PRIOR_RT_MAX && lo <= hi))
    return MLF_PRIOR_RT_NAN;
  const double r2 = 0x1.6a09e667f3bcdp+0;
  const double a = (lo - mu) / sigma, b = (hi - mu) / sigma;
  // Fa = 0.5 * erfc(-a / r2), Fb = 0.5 * erfc(-b / r2), Qa = 0.5 * erfc(a / r2), Qb = 0.5 * erfc(b / r2) from one erfc in the
  // code: four inlined copies need more scalar registers than a leaf function may use without saving some to the stack
  double Fa = 0.0, Fb = 0.0, Qa = 0.0, Qb = 0.0;
#pragma unroll 1
  for (int i = 0; i < 4; ++i) {
    const double x = (i & 1) ? b : a;
    const double e = 0.5 * erfc(((i & 2) ? x : -x) / r2);
    if (i == 0) Fa = e;
    if (i == 1) Fb = e;
    if (i == 2) Qa = e;
    if (i == 3) Qb = e;
  }
  if (!(Fb > Fa || Qa > Qb)) return MLF_PRIOR_RT_NAN;
  const double q = Fa + u * (Fb - Fa);
  const bool lower = q <= 0.5;
  // one normcdfinv in the code for both tails (the same values as the constant form's two calls)
  const double zt = normcdfinv(lower ? q : Qb + (1.0 - u) * (Qa - Qb));
  double z = lower ? zt : -zt;
  z = fmin(fmax(z, a), b);
  return mu + sigma * z;
}

__device__ __noinline__ double mlf_prior_rt_triangular(double u, double lo, double mode, double hi) {
  const double w = hi - lo;
  const double c1 = w * (mode - lo), c2 = w * (hi - mode);
  if (!(fabs(lo) <= MLF_PRIOR_RT_MAX && fabs(hi) <= MLF_PRIOR_RT_MAX && lo <= mode && mode <= hi && lo < hi && c1 <= MLF_PRIOR_RT_MAX &&
        c2 <= MLF_PRIOR_RT_MAX))
    return MLF_PRIOR_RT_NAN;
  const double c = (mode - lo) / w;
  if (u <= c) return lo + sqrt(u * c1);
  return hi - sqrt((1.0 - u) * c2);
}

// the window [k, k + len) always holds the answer and lies inside [0, n - 2]: a probe at k + (len >> 1) <= n - 2 reads c
// only, and len shrinks to ceil(len / 2) whichever way the comparison goes, so `steps` probes leave len == 1
__device__ __noinline__ double mlf_prior_table(double u, const double *t, int n, int steps) {
  int k = 0, len = n - 1;
  for (int s = 0; s < steps; ++s) {
    const int half = len >> 1;
    k = t[k + half] <= u ? k + half : k;
    len = len - half;
  }
  const double *x = t + n, *sl = x + n;
  const double dl = u - t[k], dr = t[k + 1] - u;
  return dl <= dr ? x[k] + dl * sl[k] : x[k + 1] - dr * sl[k];
}

#endif  // MLF_PRIORS_RT_DEV_HPP
