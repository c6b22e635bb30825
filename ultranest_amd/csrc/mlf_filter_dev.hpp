// mlf_filter_dev.hpp -- device helpers shared by the query quantisation kernels
// (k_quant_queries in mlf_filter.hip, the fused stages k_prep3 / k_prep4).  The threshold functions are binary32 / binary64
// arithmetic on scalars: they also build for the host once the HIP attributes are defined away (tests/prep4_decide_host.cpp);
// the binary16 helpers are for the device compiler only.
#pragma once
#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#endif
#include <math.h>
#include <stddef.h>

namespace mlf {

#if defined(__HIPCC__)
typedef _Float16 half_t;

__device__ __forceinline__ size_t frag_index(int row, int k, int ks) {
  // element (row, k) of a [rows][16*ks] matrix in fragment-major order
  const int tile = row >> 5, rr = row & 31;
  const int kstep = k >> 4, kk = k & 15;
  const int lane = rr + ((kk >> 3) << 5);
  return ((((size_t)tile * ks + kstep) * 64 + lane) << 3) + (kk & 7);
}

// three binary16 pieces of a non-negative value < 60000 (covers ~33 bits)
__device__ __forceinline__ void split3(double v, half_t *p) {
  const half_t p1 = (half_t)(float)v;
  const double r1 = v - (double)(float)p1;
  const half_t p2 = (half_t)(float)r1;
  const double r2 = r1 - (double)(float)p2;
  p[0] = p1;
  p[1] = p2;
  p[2] = (half_t)(float)r2;
}
#endif

// Certain-hit / certain-miss thresholds of one query (derivation: header of mlf_filter.hip and
// DESIGN.md 4b).  nbn2 = |sigma (b - c)|^2 of the unrounded query.  Returns false if the query
// must take the exact scan instead (sentinel rows would not be certain misses any more).
__device__ __forceinline__ bool filter_thresholds(double sigma, double namax, double nbn2, double r2,
                                                  int K, float *lo_f, float *hi_f) {
  const double nbn = sqrt(nbn2);
  const double delta = 0x1p-11 * (1.0 + 0x1p-9) * (namax + nbn) + 2.0 * sqrt((double)K) * 0x1p-24 +
                       0x1p-40 * (namax + nbn);
  const double w = namax + nbn + 0x1p-8;
  const double eacc = 0x1p-15 * w * w + 0x1p-22;
  const double sr = sigma * sqrt(r2);
  const double lo = sr * (1.0 - 0x1p-30) - delta;
  const double hi = sr * (1.0 + 0x1p-30) + delta;
  // lo <= 0: no pair may count as a certain hit; -inf and not -1, because a computed Dt can be as low as -eacc
  // ... and never negative and finite: the kernels take minima on the bit patterns, which order negative values the wrong way
  // round; with T_lo >= 0 every negative Dt is a certain hit whichever of them the minimum keeps
  const double t_lo = (lo > 0.0 && lo * lo - eacc >= 0.0) ? lo * lo - eacc : -INFINITY;
  const double t_hi = hi * hi + eacc;
  float l = (float)t_lo;
  if ((double)l > t_lo) l = nextafterf(l, -INFINITY);
  float h = (float)t_hi;
  if ((double)h < t_hi) h = nextafterf(h, INFINITY);
  *lo_f = l;
  *hi_f = h;
  return t_hi < 30000.0;
}

// The same thresholds for k_prep4 (mlf_prep4.hip), where the query operand is the binary16 rounding of an APPROXIMATE
// whitened point bq (binary32 FMA chain) instead of the exact one: |bq - sigma b'| <= zeta.  Everything is evaluated in
// binary32; every intermediate that must be an upper (lower) bound is multiplied by up = 1 + 2^-18 (dn = 1 - 2^-18),
// which covers the < 16 roundings of 2^-24 each in front of it (all sums are sums of non-negative terms).
//   nb    computed |bh|^2 (relative error <= nu = 2^-18, added to Eacc)
//   zeta  >= |bq - sigma b'|
//   sr_lo <= sigma sqrt(r2) (1 - 2^-30),  sr_hi >= sigma sqrt(r2) (1 + 2^-30)
// |bh - sigma b'| <= |bh - bq| + zeta with |bh - bq| <= 2^-11 |bq| + sqrt(K) 2^-25 (binary16 rounding incl. subnormals) and
// |bq| <= |sigma b'| + zeta, so Delta = 2^-11 (1 + 2^-9)(namax + nbn) + 2 sqrt(K) 2^-24 + 2^-40 (namax + nbn) + (1 + 2^-10) zeta
// with nbn >= |sigma b'| obtained from |bh|: |sigma b'| <= |bq| + zeta, |bq| <= (|bh| + sqrt(K) 2^-25) / (1 - 2^-11).
__device__ __forceinline__ bool filter_thresholds4(float namax, float nb, float zeta, float sqrt_k, float sr_lo,
                                                   float sr_hi, float *lo_f, float *hi_f) {
  const float up = 1.0f + 0x1p-18f, dn = 1.0f - 0x1p-18f;
  const float nbh = __builtin_sqrtf(nb) * up;
  const float nbn = ((nbh + sqrt_k * 0x1p-25f) * (1.0f + 0x1p-10f) + zeta) * up;
  const float w0 = namax + nbn;
  const float delta = (0x1p-11f * (1.0f + 0x1p-9f) * w0 + 2.0f * sqrt_k * 0x1p-24f + 0x1p-40f * w0 +
                       (1.0f + 0x1p-10f) * zeta) * up;
  const float w = w0 + 0x1p-8f;
  const float eacc = (0x1p-15f * w * w + 0x1p-22f + 0x1p-18f * nb) * up;
  const float lo = (sr_lo * dn - delta) * dn;
  const float hi = (sr_hi * up + delta) * up;
  const float t_lo = (lo * lo) * dn - eacc * up;
  *lo_f = (lo > 0.0f && t_lo >= 0.0f) ? t_lo : -INFINITY;   // never negative and finite (see filter_thresholds)
  const float t_hi = ((hi * hi) * up + eacc) * up;
  *hi_f = t_hi;
  return t_hi < 30000.0f;   // false for NaN
}

// filter_thresholds4 with the binary16 rounding of both operands MEASURED instead of charged at its worst case
// (k_prep_sweep, k_prep4; DESIGN.md 4b "measured residues").  With v = sigma (a' - b'), w = ah - bh:
//   |ah - sigma a'| <= ea_max + 2^-40 |sigma a'|   ea_max = max over the live points of |ah - xa|_2, xa = the binary64
//                                                  sigma (a - c) that was rounded (k_quant_refs sums the squares of the exact
//                                                  differences in binary64, x (1 + 2^-40), root, rounded up); 2^-40: the
//                                                  rounding of the centring, as before
//   |bh - sigma b'| <= eb + zeta                   eb = |bh - bq|_2 of THIS proposal: the packing loop sums the squares of
//                                                  v - fl16(v), v = -2 bq (exact in binary32: fl16(v) is v's neighbour on a
//                                                  coarser grid), eb = 0.5 sqrt(sum) x up -- < 32 roundings of 2^-24 in a sum
//                                                  of non-negative terms and one of the root
// Both residues are what the conversions actually left -- binary16 subnormals, underflow to zero and the double rounding
// through binary32 on the live side included -- so the terms 2^-11 (1 + 2^-9) w0 and 2 sqrt(K) 2^-24 of filter_thresholds4 go:
//   Delta = ea_max + eb + 2^-40 w0 + (1 + 2^-10) zeta.
// nbn (>= |sigma b'|, from |bh|) keeps its worst-case form: it only enters w0.
// Accumulation: Dt is a sum of K = 16 KS exact products in binary32.  In the pessimistic model of DESIGN 4b (one rounding per
// product, every partial sum bounded by S = sum |products|) the error is at most K 2^-24 S (1 + K 2^-24), and
// S <= (|ah| + |bh|)^2 (1 + 2^-11) (the norm pieces may alternate in sign) with |ah| <= namax + ea_max: the coefficient is
// c(K) (1 + 2^-9), c(K) = the power of two >= K 2^-24 and not below 2^-18 (K <= 64: 2^-18; K <= 128: 2^-17; filter_thresholds4
// charges 2^-15, the bound at K = 512).  The other terms of Eacc (norm pieces: 2^-22; nb computed in binary32: 2^-18 nb) stay.
template <int KS>
__device__ __forceinline__ bool filter_thresholds4r(float ea_max, float eb, float namax, float nb, float zeta, float sqrt_k,
                                                    float sr_lo, float sr_hi, float *lo_f, float *hi_f) {
  constexpr int K = 16 * KS;
  constexpr float ck = (K <= 64 ? 0x1p-18f : (K <= 128 ? 0x1p-17f : (K <= 256 ? 0x1p-16f : 0x1p-15f))) * (1.0f + 0x1p-9f);
  static_assert(K <= 512, "c(K) is stated up to 512 columns");
  const float up = 1.0f + 0x1p-18f, dn = 1.0f - 0x1p-18f;
  const float nbh = __builtin_sqrtf(nb) * up;
  const float nbn = ((nbh + sqrt_k * 0x1p-25f) * (1.0f + 0x1p-10f) + zeta) * up;
  const float w0 = namax + nbn;
  const float delta = (ea_max + eb + 0x1p-40f * w0 + (1.0f + 0x1p-10f) * zeta) * up;
  const float w = w0 + ea_max + 0x1p-8f;
  const float eacc = (ck * w * w + 0x1p-22f + 0x1p-18f * nb) * up;
  const float lo = (sr_lo * dn - delta) * dn;
  const float hi = (sr_hi * up + delta) * up;
  const float t_lo = (lo * lo) * dn - eacc * up;
  *lo_f = (lo > 0.0f && t_lo >= 0.0f) ? t_lo : -INFINITY;   // never negative and finite (see filter_thresholds)
  const float t_hi = ((hi * hi) * up + eacc) * up;
  *hi_f = t_hi;
  return t_hi < 30000.0f;   // false for NaN
}

}  // namespace mlf
