// mlf_prep4_dev.hpp -- the decisions of the bounded per-proposal stage (error model and layout: header of mlf_prep4.hip), each
// stated once for the three kernels that run the stage: k_prep4 (mlf_prep4.hip), k_prep_sweep (mlf_fused.hip), k_inside_mid
// (mlf_mid.hip):
//   * the shape of an instance (Prep4Shape<DP>; prep4_ns ... prep4_frag_bytes for a run-time dp on the host);
//   * the row order of T^T (prep4_column) and which accumulator pairs hold padding only (prep4_pair_is_padding);
//   * the uniform binary32 quantities of a launch (prep4_uniform);
//   * the binary32 ellipsoid decision with its outward factors (prep4_ell_decide; restated in k_prep4 and k_prep_sweep);
//   * the route byte and the thresholds (prep4_route; restated in k_prep4), the threshold form a named compile-time choice
//     (Prep4Thresholds);
//   * the three binary16 pieces of |bh|^2 in the ones columns (prep4_norm_pieces).
// What the kernels keep is hand scheduled: the matrix chains, the operand and packing loops, the fetches, the ballots, the stores.
// Everything above the device-only section is binary32 / binary64 arithmetic on scalars and builds for the host once the HIP
// attributes are defined away (tests/prep4_decide_host.cpp: bit for bit the numpy restatements of tests/test_prep4_bounds.py
// and tests/test_filter_residue_bounds.py).  The units that include it are compiled with -ffp-contract=off; FMAs only where
// written.
#pragma once
#include <math.h>
#include <stddef.h>

#include "mlf_filter_dev.hpp"
#if defined(__HIPCC__)
#include "mlf_sweep_dev.hpp"   // the vector typedefs
#endif

namespace mlf {

// Host-side constants of one region for the stage (error model: header of mlf_prep4.hip), all in binary32 and rounded
// in the safe direction; the scales are powers of two.
struct Prep4Consts {
  float g_chain;     // g: relative error of one split-binary16 chain (accumulation + operand splitting + dropped product)
  float y0n;         // >= | L^T (c_lay - c_ell) |
  float lf;          // >= | L |_F                (A = L L^T, the ellipsoid matrix)
  float el;          // >= | E_L |_F / s_L        (representation error of the two binary16 pieces of s_L L)
  float l_abs;       // >= | L |_F sqrt(K) 2^-25 / s_x     (binary16 subnormals of the proposal operand)
  float s0n;         // >= | c_lay - c_ell |
  float eps_scale;   // >= 2^-34 | A |_F          (reference rounding + factorisation, as in k_prep3)
  float enl_lo, enl_hi;   // enlarge rounded down / up
  float zt;          // >= g | T |_F + | E_T |_F / s_T     (zeta per unit sigma |delta|)
  float zt_abs;      // >= | T |_F sqrt(K) 2^-25 / s_x     (zeta's absolute term per unit sigma)
  float s_x;         // scale of the centred proposal
  float inv_sx;      // 1 / s_x
  float inv_sl_sx;   // 1 / (s_L s_x): accumulator of the ellipsoid chain -> y
  float inv_st_sx;   // 1 / (s_T s_x): accumulator of the whitening chain -> T^T delta
};

// ---------------------------------------------------------------- shape of an instance (padded dimensionality dp, even)
__host__ __device__ constexpr int prep4_ns(int dp) { return (dp + 15) / 16; }       // k-steps of 16 coordinates (K = 16 NS)
__host__ __device__ constexpr int prep4_ks(int dp) { return (dp + 6 + 15) / 16; }   // filter k-steps of 16 binary16 columns
__host__ __device__ constexpr int prep4_nt(int dp) { return (prep4_ks(dp) + 1) / 2; }   // 32-row output tiles of the whitening
__host__ __device__ constexpr int prep4_ne(int dp) { return (dp + 31) / 32; }       // 32-row output tiles of L^T delta
// every d served by the instance exceeds KMIN - 1
__host__ __device__ constexpr int prep4_kmin(int dp) { return dp <= 32 ? dp - 1 : (dp == 50 ? 49 : dp - 3); }
// stored k-steps of the L^T fragments (tile 1: k >= 32)
__host__ __device__ constexpr int prep4_nlt(int dp) { return prep4_ns(dp) + (prep4_ne(dp) > 1 ? prep4_ns(dp) - 2 : 0); }
// 1 KiB pieces (64 lanes x 16 bytes) that cover a group of 32 rows
__host__ __device__ constexpr int prep4_npc(int dp) { return (dp + 3) / 4; }
// the fragment tables in LDS: T hi, T lo [NT][NS], L^T hi, L^T lo [NLT] (1 KiB each), the start values y0 [32 NE] and the column
// constants [32 NT] (binary32), the scaled centre [16 NS] (binary64)
__host__ __device__ constexpr size_t prep4_frag_bytes(int dp) {
  return (size_t)(2 * prep4_nt(dp) * prep4_ns(dp) + 2 * prep4_nlt(dp)) * 1024 + (size_t)(32 * prep4_ne(dp) + 32 * prep4_nt(dp)) * 4 +
         (size_t)(16 * prep4_ns(dp)) * 8;
}

template <int DP>
struct Prep4Shape {
  static constexpr int NS = prep4_ns(DP), KS = prep4_ks(DP), NT = prep4_nt(DP), NE = prep4_ne(DP), KMIN = prep4_kmin(DP),
                       NLT = prep4_nlt(DP), NPC = prep4_npc(DP);
  static constexpr size_t FRAG = prep4_frag_bytes(DP);
  static constexpr size_t r16(size_t x) { return (x + 15) / 16 * 16; }
};

// filter column of row i of tile t of the whitening product (the host orders the rows of T^T by it: prep4_t_fragments)
__host__ __device__ constexpr int prep4_column(int t, int i) {
  return 32 * t + 16 * (i >> 4) + 8 * ((i >> 2) & 1) + 4 * ((i >> 3) & 1) + (i & 3);
}
// accumulator registers 2 m, 2 m + 1 of tile t hold, in BOTH halves of the wave, rows of T^T that belong to padded columns
// (>= dp): their values are exact zeros (zero matrix rows, zero centre term)
__host__ __device__ constexpr bool prep4_pair_is_padding(int t, int m, int dp) {
  for (int r = 2 * m; r < 2 * m + 2; ++r)
    for (int h = 0; h < 2; ++h)
      if (prep4_column(t, (r & 3) + 8 * (r >> 2) + 4 * h) < dp) return false;
  return true;
}

// ---------------------------------------------------------------- uniform quantities of a launch (binary32, rounded outward)
constexpr float kPrep4Up = 1.0f + 0x1p-18f, kPrep4Dn = 1.0f - 0x1p-18f;

struct Prep4Uniform {
  bool sig_ok;        // sigma is a usable scale
  float sig_f;
  float sqrt_k;       // sqrt(16 KS)
  float namax;        // >= max |sigma (a - c)| over the live points
  float ea_max;       // >= measured binary16 residue of the live points (k_quant_refs)
  float zeta_scale;   // zeta per unit |delta|
  float zeta0;        // zeta's constant term
  float kappa;        // accumulator -> -2 sigma t (powers of two: exact)
  float sr_lo, sr_hi;            // <= sigma sqrt(r2) (1 - 2^-30), >= sigma sqrt(r2) (1 + 2^-30)
  float inv_sx2, inv_slsx2;      // powers of two: exact scalings of |x32|^2 and of the ellipsoid chain's sum of squares
};

// stats: [0] sigma (handed over as `sigma`), [1] namax, [4] ea_max; csl: the 32 NT column constants 2 sigma c_s as the kernel
// put them into LDS.  quant == false (k_prep4 without the filter side): the filter quantities stay zero.  The result goes
// out through a reference: returned by value the copy of the structure cost k_prep_sweep registers.
__device__ __forceinline__ void prep4_uniform(const Prep4Consts &c, const double *stats, double r2, const float *csl,
                                              double sigma, int dp, bool quant, Prep4Uniform &u) {
  constexpr float up = kPrep4Up, dn = kPrep4Dn;
  u.sig_ok = sigma >= 0x1p-60 && sigma <= 0x1p60;
  u.sig_f = u.sig_ok ? (float)sigma : 1.0f;
  u.namax = u.ea_max = u.zeta_scale = u.zeta0 = u.sr_lo = u.sr_hi = u.kappa = 0.0f;
  u.sqrt_k = __builtin_sqrtf((float)(16 * prep4_ks(dp)));
  if (quant) {
    u.namax = (float)stats[1] * up;
    u.ea_max = (float)stats[4] * up + 0x1p-100f;
    float cs2 = 0.0f;
    for (int e = 0; e < 32 * prep4_nt(dp); ++e) cs2 = __builtin_fmaf(csl[e], csl[e], cs2);
    const float csn = 0.5f * __builtin_sqrtf(cs2) * up;
    u.zeta_scale = u.sig_f * c.zt * up;
    u.zeta0 = (c.g_chain * csn + u.sig_f * c.zt_abs) * up + 0x1p-100f;
    u.kappa = -2.0f * u.sig_f * c.inv_st_sx;
    const double sr = sigma * sqrt(r2);
    u.sr_lo = (float)(sr * (1.0 - 0x1p-30)) * dn;
    u.sr_hi = (float)(sr * (1.0 + 0x1p-30)) * up;
  }
  u.inv_sx2 = c.inv_sx * c.inv_sx;
  u.inv_slsx2 = c.inv_sl_sx * c.inv_sl_sx;
}

// ---------------------------------------------------------------- the ellipsoid decision
// qs = |y^|^2, dn2 = |x32|^2 (both already scaled back).  Inside for certain if (sqrt qs + eta)^2 + eps < enlarge, outside for
// certain if (sqrt qs - eta)^2 - eps > enlarge; everything else (NaN / inf included) is the band: decided in binary64.
// dnorm (>= |delta|) goes on to prep4_route.
// Called by k_inside_mid.  k_prep4 and k_prep_sweep keep THIS TEXT in their bodies (k_prep_sweep with its pre-gate folded into
// the two verdicts): through the call, in every spelling tried, some of their instances took more vector registers
// (profiles/prep4_dev_checks.md).  A change here is a change there.
__device__ __forceinline__ void prep4_ell_decide(const Prep4Consts &c, float qs, float dn2, float &dnorm, bool &sure_in,
                                                 bool &sure_out) {
  const float g_chain = c.g_chain, y0n = c.y0n, lf = c.lf, el = c.el, l_abs = c.l_abs, s0n = c.s0n, eps_scale = c.eps_scale,
              enl_lo = c.enl_lo, enl_hi = c.enl_hi;
  constexpr float up = kPrep4Up, dn = kPrep4Dn;
  const bool finite = qs < 3.0e38f && dn2 < 3.0e38f;   // false for NaN
  const float sq = __builtin_sqrtf(qs);
  dnorm = __builtin_sqrtf(dn2) * up + 0x1p-100f;
  const float eta = (g_chain * (y0n + lf * dnorm) + el * dnorm + l_abs) * up;
  const float de = dnorm + s0n;
  const float eps = eps_scale * (de * de) * up;
  const float hi = sq * up + eta;
  const float qhi = ((hi * hi) * up + eps) * up;
  const float lo = (sq * dn - eta) * dn;
  const float qlo = ((lo * lo) * dn - eps * up) * dn;
  sure_in = finite && qhi < enl_lo;
  sure_out = finite && lo > 0.0f && qlo > enl_hi;
}

// ---------------------------------------------------------------- route and thresholds
// The threshold form of an instance: both operands' binary16 rounding charged at its worst case (filter_thresholds4) or
// measured (filter_thresholds4r<KS>: ea_max of the live points, eb of this proposal), mlf_filter_dev.hpp and DESIGN 4b.
enum class Prep4Thresholds { kWorstCase, kMeasured };

// Route of one proposal: 0 outside the ellipsoid for certain, 1 the pre-filter takes it (thresholds in lo_f / hi_f), 2 the exact
// scan (sigma unusable, NaN / inf, |bh|^2 or T_hi does not fit binary16); 0 and 2 leave -1 in both thresholds.
//   nb   computed |bh|^2;  dnorm  from prep4_ell_decide
//   eb2  kMeasured: a callable that returns the sum over the proposal's columns of (v - fl16(v))^2, v = -2 bq (the packing
//        loop's residue sum over both halves of the wave; squares of residues below 2^-74 underflow: 2^-60).  It is called on
//        route 1 only -- handed over as a value, the half-wave exchange ran for every proposal and k_prep_sweep's listing changed
//        shape.  kWorstCase: not used (any value).
// Called by k_prep_sweep and k_inside_mid; k_prep4 keeps this text in its body (registers, profiles/prep4_dev_checks.md).
template <Prep4Thresholds TF, int KS, class EB2>
__device__ __forceinline__ int prep4_route(const Prep4Uniform &u, bool ins_any, float nb, float dnorm, EB2 &&eb2, float &lo_f,
                                           float &hi_f) {
  constexpr float up = kPrep4Up;
  int rt = ins_any ? 1 : 0;
  if (rt == 1 && (!u.sig_ok || !(nb <= 29000.0f))) rt = 2;   // NaN / inf / does not fit binary16: exact scan
  lo_f = hi_f = -1.0f;
  if (rt == 1) {
    const float zeta = (u.zeta_scale * dnorm + u.zeta0) * up;
    bool ok;
    if constexpr (TF == Prep4Thresholds::kMeasured) {
      const float eb = 0.5f * __builtin_sqrtf(eb2()) * up + 0x1p-60f;
      ok = filter_thresholds4r<KS>(u.ea_max, eb, u.namax, nb, zeta, u.sqrt_k, u.sr_lo, u.sr_hi, &lo_f, &hi_f);
    } else {
      ok = filter_thresholds4(u.namax, nb, zeta, u.sqrt_k, u.sr_lo, u.sr_hi, &lo_f, &hi_f);
    }
    if (!ok) {
      rt = 2;
      lo_f = hi_f = -1.0f;
    }
  }
  return rt;
}

#if defined(__HIPCC__)
// ---------------------------------------------------------------- device only: binary16
// Three pieces of |bh|^2 (x the ones columns of the live point) behind three ones (x its |ah|^2 pieces): filter columns
// DP ... DP + 5 of the proposal's operand; pk: the lane's packed pairs, 4 per filter k-step; h: the lane's half of the wave.
template <int C, int NPK>
__device__ __forceinline__ void prep4_put_pair(half2v v, int h, unsigned (&pk)[NPK]) {   // filter columns C, C + 1 (C even)
  // a select on the value: as a conditional store the compiler merges the three into one store at a selected INDEX and the
  // packed operand goes to scratch (k_inside_mid<6>: 12 bytes)
  unsigned &slot = pk[4 * (C >> 4) + ((C & 7) >> 1)];
  slot = h == ((C >> 3) & 1) ? __builtin_bit_cast(unsigned, v) : slot;
}
template <int DP, int NPK>
__device__ __forceinline__ void prep4_norm_pieces(float nb, int h, unsigned (&pk)[NPK]) {
  const _Float16 p1 = (_Float16)nb;
  const float r1 = nb - (float)p1;
  const _Float16 p2 = (_Float16)r1;
  const float r2 = r1 - (float)p2;
  const _Float16 p3 = (_Float16)r2;
  const _Float16 one = (_Float16)1.0f;
  prep4_put_pair<DP>((half2v){one, one}, h, pk);
  prep4_put_pair<DP + 2>((half2v){one, p1}, h, pk);
  prep4_put_pair<DP + 4>((half2v){p2, p3}, h, pk);
}
#endif

}  // namespace mlf
