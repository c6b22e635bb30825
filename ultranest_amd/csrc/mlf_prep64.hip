// mlf_prep64.hip -- per-proposal stage of MLFriends.inside for 65 ... 128 dimensions on the FP64 matrix cores (round 5):
//   H3 ellipsoid test (reference mlfriends.pyx:882-912) in the bounded |L^T delta|^2 form of k_prep3 (the reference's einsum
//   order only inside that form's own band), T1 whitening (:737-743 incl. wraps :529-536).
//
// Rounds 1-4 sent these dimensionalities through the vector kernel k_prep<DP> (lane = proposal, 2 DP registers per lane, the
// matrix broadcast from 90 KB of LDS, 3 d^2 non-fused operations for the quadratic form + 2 d^2 for the whitening: 4-6 ms per
// 10^6 x 100, one wave per SIMD), because the matrix-core stages stop at d = 64: k_prep3 keeps both fragment tables in LDS
// (200 KB at d = 128) and a proposal's k-steps in registers, k_prep4's binary16 tables and staging need 280 KB.  This kernel
// is the k-streamed form: a wave takes 16 proposals, their rows sit in the wave's LDS buffer, and for every k-step of four
// coordinates the A fragment comes straight from the row-major matrix in L2 (one 8-byte load per lane and matrix instruction,
// both matrices together 200 KB: L2-resident) -- v_mfma_f64_16x16x4_f64: A = M[4 ks + (l >> 4)][16 ct + (l & 15)], B = the
// proposals' coordinates 4 ks + (l >> 4), C = 16 outputs x 16 proposals.  The instruction accumulates k-ascending with one
// rounding per fused multiply-add (measured bit-identical to the scalar chain, scripts/probes/mfma64_probe.hip; k_prep3 and
// k_uncertain whiten this way), so the whitened coordinates are k_prep's bit for bit -- live points (whitened by k_prep) and
// proposals still meet at distance exactly 0 -- and the quadratic form keeps k_prep3's bound: |qt - q_ref| <= 2^-34 |A|_F
// |delta|^2, proposals inside that band take the einsum-order evaluation.
#include "mlf_prep64.hpp"

#include <math.h>

#include <atomic>

#include "mlf_dpp_dev.hpp"
#include "mlf_refarith_dev.hpp"

namespace mlf {

typedef double double4m __attribute__((ext_vector_type(4)));

namespace {

constexpr int kP64Waves = 4;

// the decision of proposal p behind qt = |L^T delta|^2 and nrm2 = |delta|^2 (the same in its four lanes): the band, and inside it
// the reference's arithmetic on the row as handed over, by the proposal's first lane (kq == 0; q: its lane).  (The row's
// address is formed inside the cold branch: handed over as a pointer it cost the k_prep_mfma64 instances two registers, profiles/refarith_checks.md.)
__device__ __forceinline__ bool ell_decide64(const Prep64Args &a, long long p, double qt, double nrm2, bool live, int q, int kq) {
  const int band = mlf_ell_band(qt, nrm2, a.ell_eps_scale, a.enlarge, a.chol_ok);
  bool inside = band > 0;
  const bool need_exact = live && band == 0;   // also every NaN
  if (__any(need_exact)) {
    double acc = 0.0;
    if (need_exact && kq == 0) acc = mlf_ell_q_row(a.pts + p * (long long)a.d, a.ell_ctr, a.d, a.ell_A, a.lda);
    acc = __shfl(acc, q, 64);
    if (need_exact) inside = acc <= a.enlarge;
  }
  return inside && live;
}

// NK = k-steps of 4 coordinates (4 NK >= dp), NC = output tiles of 16
template <int NK>
__global__ __launch_bounds__(64 * kP64Waves, 2) void k_prep_mfma64(Prep64Args a) {
  constexpr int NC = (NK + 3) / 4;
  extern __shared__ __attribute__((aligned(16))) double lds64[];
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  const int q = lane & 15, kq = lane >> 4;
  const int d = a.d, dp = a.dp;
  const int ds = d | 1;                          // odd row stride: the 16 proposals of a k-step read 16 different banks
  double *xrow = lds64 + (size_t)wv * 16 * ds;   // [16][ds] this wave's proposals as handed over, later their whitened rows
  const long long ntiles = (a.np + 15) / 16;
  const long long total = a.np * (long long)d;
  for (long long tile = (long long)blockIdx.x * kP64Waves + wv; tile < ntiles; tile += (long long)gridDim.x * kP64Waves) {
    const long long p = tile * 16 + q;
    const bool live = p < a.np;
    // ---- the tile's 16 rows: 16 d contiguous doubles, all requests first
    {
      const long long base = tile * 16 * (long long)d;
      constexpr int kPer = (16 * 128 + 63) / 64;   // 32
      double v[kPer];
#pragma unroll
      for (int i = 0; i < kPer; ++i) {
        const int e = lane + 64 * i;
        const long long g = base + e;
        v[i] = (e < 16 * d && g < total) ? a.pts[g] : 0.0;
      }
      __builtin_amdgcn_wave_barrier();   // the rows of the tile before have been written out
#pragma unroll
      for (int i = 0; i < kPer; ++i) {
        const int e = lane + 64 * i;
        if (e < 16 * d) {
          const int rr = e / d;
          xrow[rr * ds + (e - rr * d)] = v[i];
        }
      }
      __builtin_amdgcn_wave_barrier();
    }
    const double *row = xrow + q * ds;
    // ---- H3 bound: y = L^T delta on the matrix cores, qt = |y|^2 (k_prep3's form)
    double qt = 0.0, nrm2 = 0.0;
    {
      double4m y[NC];
#pragma unroll
      for (int ct = 0; ct < NC; ++ct) y[ct] = (double4m){0.0, 0.0, 0.0, 0.0};
      // (two k-steps per pass: unrolled in full, the compiler kept every fragment address and half of the fragments live --
      // 256 + 224 registers, 710 scalar spills, one wave per SIMD)
#pragma unroll 2
      for (int ks = 0; ks < NK; ++ks) {
        const int k = 4 * ks + kq;
        const double dl = k < d ? row[k] - a.ell_ctr[k] : 0.0;
        nrm2 = __builtin_fma(dl, dl, nrm2);
        double afr[NC];
#pragma unroll
        for (int ct = 0; ct < NC; ++ct) {
          const int c = 16 * ct + q;
          // y_c = sum_k delta_k L[k][c] (row-major L, stride dp: the 16 lanes of a k read 128 contiguous bytes); L[k][c] = 0
          // for c > k: the tiles above the diagonal are skipped
          afr[ct] = (16 * ct <= 4 * ks + 3 && k < d && c < d) ? a.ell_L[(size_t)k * dp + c] : 0.0;
        }
#pragma unroll
        for (int ct = 0; ct < NC; ++ct)
          if (16 * ct <= 4 * ks + 3) y[ct] = __builtin_amdgcn_mfma_f64_16x16x4f64(afr[ct], dl, y[ct], 0, 0, 0);
      }
#pragma unroll
      for (int ct = 0; ct < NC; ++ct)
#pragma unroll
        for (int r = 0; r < 4; ++r) qt = __builtin_fma(y[ct][r], y[ct][r], qt);
      qt = quad_sum(qt);
      nrm2 = quad_sum(nrm2);
    }
    const bool inside = ell_decide64(a, p, qt, nrm2, live, q, kq);
    if (live && kq == 0) a.gate[p] = inside ? 1 : 0;
    if (!a.do_tr || !__any(inside)) continue;
    // ---- T1: t = delta_w T on the matrix cores, k ascending, one fma per term
    double4m t[NC];
#pragma unroll
    for (int ct = 0; ct < NC; ++ct) t[ct] = (double4m){0.0, 0.0, 0.0, 0.0};
#pragma unroll 2
    for (int ks = 0; ks < NK; ++ks) {
      const int k = 4 * ks + kq;
      double dw = 0.0;
      if (k < d) {
        double w = row[k];
        if (a.wrap_shift) {
          const double sh = a.wrap_shift[k];
          if (sh == sh) w = mlf_wrap_unit_fast(w, sh);   // NaN marks an unwrapped dimension
        }
        dw = w - a.lay_ctr[k];
      }
      double afr[NC];
#pragma unroll
      for (int ct = 0; ct < NC; ++ct) {
        const int c = 16 * ct + q;
        afr[ct] = (k < dp && c < d) ? a.T8[(size_t)k * a.ldt8 + c] : 0.0;
      }
#pragma unroll
      for (int ct = 0; ct < NC; ++ct) t[ct] = __builtin_amdgcn_mfma_f64_16x16x4f64(afr[ct], dw, t[ct], 0, 0, 0);
    }
    __builtin_amdgcn_wave_barrier();   // every lane has read the raw rows
#pragma unroll
    for (int ct = 0; ct < NC; ++ct)
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int c = 16 * ct + kq + 4 * r;   // output row of the accumulator register (mlf_prep3.hip)
        if (c < d) xrow[q * ds + c] = t[ct][r];
      }
    __builtin_amdgcn_wave_barrier();
    // ---- the whitened rows leave as they came: contiguous
    {
      const unsigned long long in_bits = __ballot(inside && kq == 0);   // bit q: proposal q of the tile is inside
      double *out = a.t_out + tile * 16 * a.ldt;
      for (int e = lane; e < 16 * d; e += 64) {
        const int rr = e / d, c = e - rr * d;
        if ((in_bits >> rr) & 1ull) out[(long long)rr * a.ldt + c] = xrow[rr * ds + c];
      }
    }
  }
}

// ---------------------------------------------------------------------------------------------------------------------
// The same stage for 129 ... 1024 dimensions, the dimensionality at run time (the per-proposal stage of the batches that take
// the pre-filter of mlf_wide_filter.hip; k_prep_wide -- one thread per proposal, a 64-lane workgroup per CU -- was 91-100 % of
// such a call).  A wave takes 16 proposals.  Nothing is staged: a lane's operand of a k-step is one coordinate of its
// proposal, read from the row as handed over (L1 / L2 hits from the second pass on), and the accumulators hold kW64CT output
// tiles (128 columns) at a time -- the k-loop runs once per chunk of columns.  The whitened coordinates leave straight from
// the accumulator registers.  Arithmetic as above: whitening = the k-ascending FMA chain bit for bit, the quadratic form
// bounded, proposals inside the band evaluated in the einsum order by their first lane.
// The band: eps = 2^-28 |A|_F |delta|^2 (the caller's scale).  Up to 1024 dimensions three errors of up to d^2 2^-53 = 2^-33
// each (same units) meet: the reference's own sequential sum of d^2 terms, the backward error of the host Cholesky factor,
// and the chains of y = L^T delta and |y|^2; 2^-28 leaves a factor of ten above their sum (k_prep3's 2^-34 is stated for
// d <= 128, where they are 2^-39).
constexpr int kW64CT = 8;
__global__ __launch_bounds__(64 * kP64Waves) void k_prep_mfma64_wide(Prep64Args a) {
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  const int q = lane & 15, kq = lane >> 4;
  const int d = a.d, dp = a.dp;
  const int nk = dp / 4, nct = dp / 16;   // dp is a multiple of 16
  const long long ntiles = (a.np + 15) / 16;
  for (long long tile = (long long)blockIdx.x * kP64Waves + wv; tile < ntiles; tile += (long long)gridDim.x * kP64Waves) {
    const long long p = tile * 16 + q;
    const bool live = p < a.np;
    const double *row = a.pts + (live ? p : 0) * (long long)d;
    // ---- H3 bound: y = L^T delta, qt = |y|^2
    double qt = 0.0, nrm2 = 0.0;
    for (int c0 = 0; c0 < nct; c0 += kW64CT) {
      double4m y[kW64CT];
#pragma unroll
      for (int ct = 0; ct < kW64CT; ++ct) y[ct] = (double4m){0.0, 0.0, 0.0, 0.0};
      // L[k][c] = 0 for c > k: k-steps in front of the chunk's first column contribute nothing (the first chunk starts at 0)
#pragma unroll 2
      for (int ks = 4 * c0; ks < nk; ++ks) {
        const int k = 4 * ks + kq;
        const double dl = (live && k < d) ? row[k] - a.ell_ctr[k] : 0.0;
        if (c0 == 0) nrm2 = __builtin_fma(dl, dl, nrm2);
        double afr[kW64CT];
#pragma unroll
        for (int ct = 0; ct < kW64CT; ++ct) {
          const int c = 16 * (c0 + ct) + q;
          afr[ct] = (c0 + ct < nct && 16 * (c0 + ct) <= 4 * ks + 3 && k < d && c < d) ? a.ell_L[(size_t)k * dp + c] : 0.0;
        }
#pragma unroll
        for (int ct = 0; ct < kW64CT; ++ct)
          if (c0 + ct < nct && 16 * (c0 + ct) <= 4 * ks + 3) y[ct] = __builtin_amdgcn_mfma_f64_16x16x4f64(afr[ct], dl, y[ct], 0, 0, 0);
      }
#pragma unroll
      for (int ct = 0; ct < kW64CT; ++ct)
#pragma unroll
        for (int r = 0; r < 4; ++r) qt = __builtin_fma(y[ct][r], y[ct][r], qt);
    }
    qt = quad_sum(qt);
    nrm2 = quad_sum(nrm2);
    const bool inside = ell_decide64(a, live ? p : 0, qt, nrm2, live, q, kq);   // the row index as `row` was formed from it
    if (live && kq == 0) a.gate[p] = inside ? 1 : 0;
    if (!a.do_tr || !__any(inside)) continue;
    // ---- T1: t = delta_w T, k ascending, one fma per term
    for (int c0 = 0; c0 < nct; c0 += kW64CT) {
      double4m t[kW64CT];
#pragma unroll
      for (int ct = 0; ct < kW64CT; ++ct) t[ct] = (double4m){0.0, 0.0, 0.0, 0.0};
#pragma unroll 2
      for (int ks = 0; ks < nk; ++ks) {
        const int k = 4 * ks + kq;
        double dw = 0.0;
        if (live && k < d) {
          double w = row[k];
          if (a.wrap_shift) {
            const double sh = a.wrap_shift[k];
            if (sh == sh) w = mlf_wrap_unit_fast(w, sh);   // NaN marks an unwrapped dimension
          }
          dw = w - a.lay_ctr[k];
        }
        double afr[kW64CT];
#pragma unroll
        for (int ct = 0; ct < kW64CT; ++ct) {
          const int c = 16 * (c0 + ct) + q;
          afr[ct] = (c0 + ct < nct && c < d) ? a.T8[(size_t)k * a.ldt8 + c] : 0.0;   // k < dp: rows past d are zero
        }
#pragma unroll
        for (int ct = 0; ct < kW64CT; ++ct)
          if (c0 + ct < nct) t[ct] = __builtin_amdgcn_mfma_f64_16x16x4f64(afr[ct], dw, t[ct], 0, 0, 0);
      }
      if (inside)
#pragma unroll
        for (int ct = 0; ct < kW64CT; ++ct)
#pragma unroll
          for (int r = 0; r < 4; ++r) {
            const int c = 16 * (c0 + ct) + kq + 4 * r;   // output row of the accumulator register (mlf_prep3.hip)
            if (c0 + ct < nct && c < d) a.t_out[p * a.ldt + c] = t[ct][r];
          }
    }
  }
}

}  // namespace

bool prep64_wide_usable(int d) { return d > 128 && d <= 1024; }

hipError_t launch_prep64_wide(const Prep64Args &a, hipStream_t s) {
  if (a.np <= 0) return hipSuccess;
  if (!prep64_wide_usable(a.d) || (a.dp & 15) || a.dp < a.d || a.ldt8 < a.dp) return hipErrorInvalidValue;
  const long long ntiles = (a.np + 15) / 16;
  long long wgs = (ntiles + kP64Waves - 1) / kP64Waves;
  if (wgs > 256 * 8) wgs = 256 * 8;
  hipLaunchKernelGGL(k_prep_mfma64_wide, dim3((unsigned)wgs), dim3(64 * kP64Waves), 0, s, a);
  return hipGetLastError();
}

bool prep64_usable(int d) { return d > 64 && d <= 128; }

hipError_t launch_prep64(const Prep64Args &a, hipStream_t s) {
  if (a.np <= 0) return hipSuccess;
  const int nk = (a.dp + 3) / 4;
  const size_t lds = (size_t)kP64Waves * 16 * (a.d | 1) * sizeof(double);
  const long long ntiles = (a.np + 15) / 16;
  long long wgs = (ntiles + kP64Waves - 1) / kP64Waves;
  if (wgs > 256 * 8) wgs = 256 * 8;   // grid-stride beyond 8 workgroups per CU
  const dim3 grid((unsigned)wgs), block(64 * kP64Waves);
  if (lds > 48 * 1024) {   // above the default grant (66 KB at d = 128): the attribute belongs to (function, device)
    static DeviceGrant grant;
    if (hipError_t e = grant.ensure([] {
          hipError_t g = hipFuncSetAttribute(reinterpret_cast<const void *>(&k_prep_mfma64<20>), hipFuncAttributeMaxDynamicSharedMemorySize, 80 * 1024);
          if (g == hipSuccess) g = hipFuncSetAttribute(reinterpret_cast<const void *>(&k_prep_mfma64<24>), hipFuncAttributeMaxDynamicSharedMemorySize, 80 * 1024);
          if (g == hipSuccess) g = hipFuncSetAttribute(reinterpret_cast<const void *>(&k_prep_mfma64<28>), hipFuncAttributeMaxDynamicSharedMemorySize, 80 * 1024);
          if (g == hipSuccess) g = hipFuncSetAttribute(reinterpret_cast<const void *>(&k_prep_mfma64<32>), hipFuncAttributeMaxDynamicSharedMemorySize, 80 * 1024);
          return g;
        }))
      return e;
  }
  // instances by k-steps: dp is a multiple of 16 above 64 (80, 96, 112, 128)
  switch (nk) {
    case 20: hipLaunchKernelGGL(k_prep_mfma64<20>, grid, block, lds, s, a); break;
    case 24: hipLaunchKernelGGL(k_prep_mfma64<24>, grid, block, lds, s, a); break;
    case 28: hipLaunchKernelGGL(k_prep_mfma64<28>, grid, block, lds, s, a); break;
    case 32: hipLaunchKernelGGL(k_prep_mfma64<32>, grid, block, lds, s, a); break;
    default: return hipErrorInvalidValue;
  }
  return hipGetLastError();
}

}  // namespace mlf
