// mlf_hotstart_dev.hpp -- warm start for user models on the device (ultranest_amd/hotstart.py): the deformation of the unit
// cube of an auxiliary problem, as device functions around a user's own mlf_user_* functions.  Like the prior headers, the
// text of this header is pasted into a generated model source: hotstart.py puts the inner model's source in front of it (its
// entry points renamed by #define / #undef around the text), and a short generated wrapper that defines the real mlf_user_*
// entry points behind it.  It is compiled at run time with the model (hiprtc, -O3 -std=c++17 -ffp-contract=off: no FMA is
// formed), is NOT part of libmlfriends_hip.so and adds no C-ABI entry.  Plain HIP C++17: no inline assembly, no intrinsics.
//
// Every table lives in a TAIL appended to the inner model's aux array: aux = [inner aux (nin values) | tail], and the inner
// functions are called with (aux, nin), so they see the array they always saw.  The program text depends on the inner source,
// the inner dimension D (#define MLF_HOTSTART_D, which also sizes the private arrays) and the form, never on the samples.
//
// Form (a), "contbox" (reference hotstart.py get_auxiliary_contbox_parameterization).  D + 1 cube coordinates: u[0..D) and
// t = u[D].  M knots (2 <= M <= 32; the host builds at most 25).  Tail, T = 1 + M + 2 * M * D + 2 * (M - 1) * D values:
//
//   xp[M]            the knots of t (uinterpspace): xp[0] = 0 < ... < xp[M-1] = 1
//   lo[M][D]         lower box edges (ulos, row j = knot j)
//   slo[M-1][D]      (lo[j+1][i] - lo[j][i]) / (xp[j+1] - xp[j]), computed on the host in binary64 (numpy's slope, same bits)
//   hi[M][D]         upper box edges (uhis)
//   shi[M-1][D]      their slopes
//   (double)M        the last value of aux: the tail's length follows from it and D, nin = naux - T
//
// j = the largest index <= M - 2 with xp[j] <= t (a branch-free bisection of exactly 5 probes: the window [j, j + len) shrinks
// to ceil(len / 2) whichever way a comparison goes, and 31 -> 16 -> 8 -> 4 -> 2 -> 1; every probe reads xp at an index in
// [0, M - 2] for every t, NaN included).  Per axis i, numpy's interp formula:
//
//   ulo = slo[j][i] * (t - xp[j]) + lo[j][i],  uhi = shi[j][i] * (t - xp[j]) + hi[j][i]
//   (t >= xp[M-1]: ulo = lo[M-1][i], uhi = hi[M-1][i];  t <= xp[0]: lo[0][i], hi[0][i] -- numpy's ends)
//   wd = uhi - ulo;  umod[i] = ulo + wd * u[i];  weight = weight + log(wd)      (from 0.0, in axis order, one addition each)
//
// p[0..D) = inner transform(umod) (umod itself without one), p[D] = weight, L = inner L(p[0..D)) + p[D].
//
// Form (b), independent Student-t per axis, truncated to the cube (get_extended_auxiliary_independent_problem).  D cube
// coordinates.  Tail, T = 11 * D + 2 values: one record of 11 values per axis, then two more:
//
//   axis i:  w_i, lo_i, ha, lnB, lnha, lnnu, ctr_i, err_i, c_i, df, (df + 1) / 2
//            w_i = cdf_i(1) - cdf_i(0), lo_i = cdf_i(0); ha, lnB, lnha, lnnu the constants of mlf_prior_studentt (df / 2,
//            ln B(df/2, 1/2), ln(df/2), ln df); ctr_i, err_i centre and scale; c_i = lognorm(df) - log(err_i), the log-density
//            of axis i at its centre.  The constants of df are repeated in every record ON PURPOSE: all an axis needs is
//            then behind ONE address that changes with i, so nothing but that address is kept in scalar registers across
//            the call of the quantile function (six pointers and six constants kept there made the gated program spill).
//   weight_ref = sum_i c_i     (the reference's last column is -sum logpdf + weight_ref)
//   (double)D                  the last value of aux (nin = naux - T)
//
// The model HAS a transform, and its p row is x, the deformed cube coordinates:
//   transform   q = u[i] * w[i] + lo[i];  t = the standard quantile of q (df = 1: -cospi(q) / sinpi(q), else
//               mlf_prior_studentt(q, 0, 1, ..));  x[i] = ctr[i] + err[i] * t
//   likelihood  z = (x[i] - ctr[i]) / err[i];  s = s + (c[i] - ((df + 1) / 2) * log1p(z * z / df))   (from 0.0, in axis order: the
//               reference's logpdf(x), taken from x);  L = inner L(inner transform(x)) - s
//   derived     [inner transform(x) | -s + weight_ref]
// So the quantile, the expensive part, runs once per row, in a function that holds no array; the likelihood holds at most ONE
// private array of D doubles (the inner transform's output; none without an inner transform) and makes no call of its own.
//
// (MLF_HOTSTART_CAUCHY 1 selects the closed form, written inline; otherwise the texts of mlf_priors_dev.hpp and
// mlf_priors_special_dev.hpp stand in front.)
#ifndef MLF_HOTSTART_DEV_HPP
#define MLF_HOTSTART_DEV_HPP

// ---- form (a) ----

__device__ __forceinline__ long long mlf_hotstart_contbox_tail(int M, int D) {
  return 1LL + (long long)M + 2LL * (long long)M * D + 2LL * (long long)(M - 1) * D;
}

// the number of values of the inner model's aux array in front of the tail
__device__ __forceinline__ long long mlf_hotstart_contbox_nin(const double *aux, long long naux, int D) {
  return naux - mlf_hotstart_contbox_tail((int)aux[naux - 1], D);
}

// the segment of t: the largest index <= M - 2 with xp[j] <= t (0 for a NaN); five probes, every one inside [0, M - 2]
__device__ __forceinline__ int mlf_hotstart_segment(double t, const double *xp, int M) {
  int j = 0, len = M - 1;
#pragma unroll
  for (int s = 0; s < 5; ++s) {
    const int half = len >> 1;
    j = xp[j + half] <= t ? j + half : j;
    len = len - half;
  }
  return j;
}

// umod[0..D) from u[0..D + 1); returns the summed log-volume.  `tail` points at xp[0], M is the tail's last value.
__device__ __forceinline__ double mlf_hotstart_contbox(const double *u, double *umod, int D, const double *tail, int M) {
  const double t = u[D];
  const double *xp = tail;
  const double *lo = xp + M, *slo = lo + (long long)M * D, *hi = slo + (long long)(M - 1) * D, *shi = hi + (long long)M * D;
  const int j = mlf_hotstart_segment(t, xp, M);
  const double dt = t - xp[j];
  const bool right = t >= xp[M - 1], left = t <= xp[0];
  const int je = right ? M - 1 : 0;
  const double *lj = lo + (long long)j * D, *hj = hi + (long long)j * D, *le = lo + (long long)je * D, *he = hi + (long long)je * D;
  const double *sl = slo + (long long)j * D, *sh = shi + (long long)j * D;
  double weight = 0.0;
  for (int i = 0; i < D; ++i) {
    double ulo = sl[i] * dt + lj[i];
    double uhi = sh[i] * dt + hj[i];
    if (right || left) {
      ulo = le[i];
      uhi = he[i];
    }
    const double wd = uhi - ulo;
    umod[i] = ulo + wd * u[i];
    weight = weight + log(wd);
  }
  return weight;
}

// ---- form (b) ----

__device__ __forceinline__ long long mlf_hotstart_indep_nin(long long naux, int D) {
  return naux - (11LL * D + 2LL);
}

#ifdef MLF_HOTSTART_INDEP
// x[0..D) from u[0..D).  The record's address is formed from (aux, naux) inside the loop: the kernel keeps those two alive
// anyway, a pointer to the tail would be one more scalar register pair across the call.  The loop holds the call of the quantile function and no other
// library function, and is not unrolled: the 64-bit constants of an inlined log or exp would have to survive the call in
// scalar registers (D is a constant of the program: at D = 1, 2 an unrolled loop would merge with its surroundings).
__device__ __forceinline__ void mlf_hotstart_indep_x(const double *u, double *x, int D, const double *aux, long long naux) {
#pragma unroll 1
  for (int i = 0; i < D; ++i) {
    const double *r = aux + (mlf_hotstart_indep_nin(naux, D) + 11LL * i);
    const double q = u[i] * r[0] + r[1];
#if MLF_HOTSTART_CAUCHY
    x[i] = r[6] + r[7] * (-cospi(q) / sinpi(q));
#else
    x[i] = mlf_prior_studentt(q, r[6], r[7], r[2], r[3], r[4], r[5]);   // loc + scale * t inside: nothing of the record is needed after the call
#endif
  }
}

// s = the sum of the axes' log-densities at x[0..D)
__device__ __forceinline__ double mlf_hotstart_indep_logpdf(const double *x, int D, const double *aux, long long naux) {
  double s = 0.0;
#pragma unroll 1
  for (int i = 0; i < D; ++i) {
    const double *r = aux + (mlf_hotstart_indep_nin(naux, D) + 11LL * i);
    const double z = (x[i] - r[6]) / r[7];
    s = s + (r[8] - r[10] * log1p(z * z / r[9]));
  }
  return s;
}
#endif

#endif  // MLF_HOTSTART_DEV_HPP
