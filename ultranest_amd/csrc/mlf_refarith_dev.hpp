// mlf_refarith_dev.hpp -- the few lines of arithmetic that must match the reference bit for bit, each stated once for every
// route of MLFriends.inside and the step samplers:
//   * the ellipsoid quadratic form in numpy's c_einsum order: mlf_tregion_q (mlf_tregion_dev.hpp), and mlf_ell_q_row, its
//     call for a row and a centre in memory;
//   * the band decision in front of it (mlf_ell_band);
//   * the wrap of circular axes (mlf_wrap_unit, mlf_wrap_unit_fast).
// Device code; it includes nothing but mlf_tregion_dev.hpp and uses fmod of the including unit, so it also builds for the host
// once the HIP attributes are defined away (tests/refarith_host.cpp).  The units that include it are compiled with
// -ffp-contract=off.
#pragma once
#include "mlf_tregion_dev.hpp"

// q = (row - ctr)^T A (row - ctr) of one row of d doubles, A row-major with stride lda: the reference tier of every bounded
// ellipsoid test (mlfriends.pyx:882-912).  One term at a time: it is the cold branch of kernels at their register limit.
__device__ __forceinline__ double mlf_ell_q_row(const double *row, const double *ctr, int d, const double *A, int lda) {
  const auto delta = [&](int k) { return row[k] - ctr[k]; };
  return mlf_tregion_q<mlf_tregion_plain>(d, delta, delta, [&](int j, int k) { return A[(long long)j * lda + k]; });
}

// The bounded form qt = |L^T delta|^2 against enlarge, with the band eps = eps_scale |delta|^2 (nrm2 = |delta|^2) that covers
// its distance from the reference's q: +1 sure inside, -1 sure outside, 0 undecided -- the reference tier decides.  Every NaN
// and every region without a Cholesky factor (chol_ok == 0) is undecided.
__device__ __forceinline__ int mlf_ell_band(double qt, double nrm2, double eps_scale, double enlarge, int chol_ok) {
  const double eps = eps_scale * nrm2;
  if (chol_ok && qt + eps < enlarge) return 1;
  if (chol_ok && qt - eps > enlarge) return -1;
  return 0;
}

// A coordinate of a circular axis moved by the axis' shift (reference mlfriends.pyx:529-536).  The caller tests the shift:
// NaN marks an axis that is not wrapped.  (The proposal samplers apply the inverse, cut = 1 - shift: mlf_sample.hip.)
__device__ __forceinline__ double mlf_wrap_unit(double w, double shift) { return fmod(w + shift, 1.0); }

// The same value for the matrix-core stages, where a call of fmod in the loop costs registers: sums in [0, 2) -- all that
// coordinates of the unit cube and shifts in [0, 1) give -- need one subtraction (exact, as fmod is); the rest take the call
__device__ __attribute__((noinline)) inline double mlf_wrap_unit_call(double w, double shift) { return mlf_wrap_unit(w, shift); }
__device__ __forceinline__ double mlf_wrap_unit_fast(double w, double shift) {
  const double xs = w + shift;
  return (xs >= 0.0 && xs < 2.0) ? (xs >= 1.0 ? xs - 1.0 : xs) : mlf_wrap_unit_call(w, shift);
}
