// mlf_tregion_dev.hpp -- the driver's parameter-space wrapping ellipsoid (WrappingEllipsoid.inside, reference
// mlfriends.pyx:1551-1649, applied between prior transform and likelihood at integrator.py:1789-1804) as device functions
// of the refill kernels: k_transform_gate (mlf_sample.hip, built-in transforms) and the gated form of mlf_user_rows
// (mlf_user_rows.hpp, compiled by hiprtc: this header includes nothing).
//
// q = sum_j sum_k ((p_j - c_j) * A_jk) * (p_k - c_k) in the order of k_prep (mlf_prep.hip), i.e. of numpy's three-operand
// c_einsum: ONE accumulator, j outer / k inner, term = (delta_j * A_jk) * delta_k, no FMA (the units that include this
// header are compiled with -ffp-contract=off).  inside = q <= enlarge; a non-finite q is outside.
//
// Fixed dimensions (WrappingEllipsoid.variable_dims): the host hands over the dense d x d matrix with the ellipsoid's
// invcov on the variable dimensions and zeros elsewhere, centre 0 on the fixed ones.  Their terms are +-0, which leave a
// finite accumulator as it is, so q is the q of the variable dimensions alone.  fixed_val[k] is the value p_k must equal
// on a fixed dimension, NaN on a variable one.
#pragma once

// q of one row.  delta_j(j), any j < d: p_j - c_j.  delta_k(k): the same values for the inner index -- k < KN where KN > 0
// (a compile-time bound >= d: the row sits in registers, zero beyond d, and mat(j, k) is zero padded), else k < d.
// KN = mlf_tregion_plain: k < d one term at a time -- the cold branch of a kernel that has no registers to spare for the
// operands fetched ahead.
constexpr int mlf_tregion_plain = -1;
template <int KN, class DeltaJ, class DeltaK, class Mat>
__device__ __forceinline__ double mlf_tregion_q(int d, DeltaJ delta_j, DeltaK delta_k, Mat mat) {
  double acc = 0.0;
  for (int j = 0; j < d; ++j) {
    const double dj = delta_j(j);
    if constexpr (KN > 0) {
#pragma unroll
      for (int k = 0; k < KN; ++k) acc += (dj * mat(j, k)) * delta_k(k);
    } else {
      // operands of 8 terms fetched ahead of their use (adjacent wave-uniform loads merge into wide scalar loads and their
      // latency is paid once per group); the terms enter the accumulator one by one, k ascending, as above
      int k = 0;
      if constexpr (KN == 0) {
        for (; k + 8 <= d; k += 8) {
          double a[8], dk[8];
#pragma unroll
          for (int t = 0; t < 8; ++t) {
            a[t] = mat(j, k + t);
            dk[t] = delta_k(k + t);
          }
#pragma unroll
          for (int t = 0; t < 8; ++t) acc += (dj * a[t]) * dk[t];
        }
      }
      for (; k < d; ++k) acc += (dj * mat(j, k)) * delta_k(k);
    }
  }
  return acc;
}

// p_k against fixed_val[k] (NaN: a variable dimension, no condition)
__device__ __forceinline__ bool mlf_tregion_fixed_ok(double pk, double fixed) { return fixed != fixed || pk == fixed; }

// The whole test of one parameter row p (d doubles, unit stride; global memory or LDS) against the dense matrix A (d x d,
// row-major), centre and fixed values in global memory.  Called with kernel-argument pointers and indexed by the loop
// counters only, A, ctr and fixed_val are read through wave-uniform addresses.
__device__ inline bool mlf_tregion_inside(const double *p, int d, const double *__restrict__ A, const double *__restrict__ ctr,
                                          const double *__restrict__ fixed_val, double enlarge) {
  bool ok = true;
  for (int k = 0; k < d; ++k) ok = ok && mlf_tregion_fixed_ok(p[k], fixed_val[k]);
  const auto delta = [&](int k) { return p[k] - ctr[k]; };
  const double q = mlf_tregion_q<0>(d, delta, delta, [&](int j, int k) { return A[j * d + k]; });
  return ok && q <= enlarge;
}

#ifdef MLF_TREGION_SPLIT_ROW
// The same test of a row that lies in two pieces: [p | q], p of d and q of nq doubles (unit stride each), against a matrix, centre
// and fixed values over all w = d + nq columns (the t-region over a model's parameters and derived parameters, mlf_user_rows.hpp
// with MLF_USER_GATE_DERIVED).  The arithmetic is mlf_tregion_q's, reached through an accessor: nothing is copied together first.
// (Only for includers that ask for it: the text the others compile is what it was.)
__device__ inline bool mlf_tregion_inside_split(const double *p, int d, const double *q, int nq, const double *__restrict__ A,
                                                const double *__restrict__ ctr, const double *__restrict__ fixed_val,
                                                double enlarge) {
  const int w = d + nq;
  bool ok = true;
  for (int k = 0; k < d; ++k) ok = ok && mlf_tregion_fixed_ok(p[k], fixed_val[k]);
  for (int k = 0; k < nq; ++k) ok = ok && mlf_tregion_fixed_ok(q[k], fixed_val[d + k]);
  const auto delta = [&](int k) { return (k < d ? p[k] : q[k - d]) - ctr[k]; };   // k is a loop counter: a wave-uniform choice
  const double form = mlf_tregion_q<0>(w, delta, delta, [&](int j, int k) { return A[j * w + k]; });
  return ok && form <= enlarge;
}
#endif
