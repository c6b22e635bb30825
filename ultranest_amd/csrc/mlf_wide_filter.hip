// mlf_wide_filter.hip -- the f16 matrix-core pre-filter of mlf_filter.hip for 129 ... 1024 dimensions, mask mode only.
//
// The idea is the one of mlf_filter.hip: live points and queries are centred, scaled by a power of two and
// rounded to binary16; one v_mfma_f32_32x32x16_f16 chain per 32 x 32 block of pairs gives Dt = |ah|^2 + |bh|^2 - 2 ah.bh with a
// PROVEN error band; a query whose minimum Dt over all live points is <= T_lo has a neighbour, one whose minimum is > T_hi has
// none, and only a query whose minimum ends between the two goes through the reference's binary64 loop (k_scan_wide_list over
// the list of those queries).  The masks are bit-identical to the exact scan's.
//
// What differs from the kernels for up to 128 dimensions: the dimensionality is a run-time argument (K = 16 ceil((dp + 6) / 16)
// = 160 ... 1040 columns, 10 ... 65 k-steps), so nothing is held per column in registers:
//   k_wide_ref_colsum / _extent / _finish   centre, amax, sigma, namax of the live points: the passes of k_ref_colsum /
//                                           k_ref_extent / k_ref_finish with a loop over the columns (same summation order)
//   k_wide_quant_refs                       live points -> [tile32][ks][64 lanes][8 halves], one wave per row
//   k_wide_quant_queries                    whitened rows (k_prep_wide's binary64 chain) -> the same layout, thresholds, routes
//   k_wide_sweep<G>                         G query groups of a workgroup staged ONCE in LDS, the live tiles streamed as 1 KiB
//                                           wave-wide fragment loads, one accumulator block per (tile, group), minimum only
// The sweep never splits K: every (tile, group) block is one sequential chain of ks matrix instructions into one accumulator,
// so the accumulation model of the bound is the one of the narrow kernels with more terms (wide_thresholds below).
#include "mlf_wide_filter.hpp"
#include "mlf_filter_dev.hpp"
#include "mlf_sweep_dev.hpp"

#include <math.h>

namespace mlf {

namespace {

typedef __attribute__((ext_vector_type(8))) _Float16 half8;

struct half8pack {
  half_t h[8];
};

// ---------------------------------------------------------------- live-point statistics -----
// stats: [0]=sigma [1]=namax [2]=amax [3]=finite flag; the centre follows at [8 ..].  The summation order is k_ref_colsum's:
// row i goes to workgroup (i / 4) % 64, wave i % 4; a wave adds its rows in ascending order, the four waves meet as
// (0 + 1) + (2 + 3), the 64 workgroup sums are added in ascending order by every consumer.
// grid = (64, ceil(dp / 128)): blockIdx.y selects 128 columns
__global__ __launch_bounds__(256) void k_wide_ref_colsum(const double *__restrict__ refR, int n, int dp, double *__restrict__ scratch) {
  __shared__ double part[4][128];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int cb = blockIdx.y * 128;
  const int c0 = cb + lane < dp ? cb + lane : 0, c1 = cb + lane + 64 < dp ? cb + lane + 64 : 0;
  double s0 = 0.0, s1 = 0.0;
  for (int i = blockIdx.x * 4 + wave; i < n; i += 4 * kWideStatBlocks) {
    s0 += refR[(size_t)i * dp + c0];
    s1 += refR[(size_t)i * dp + c1];
  }
  part[wave][lane] = s0;
  part[wave][lane + 64] = s1;
  __syncthreads();
  if (threadIdx.x < 128 && cb + threadIdx.x < dp)
    scratch[(size_t)blockIdx.x * kWideStatCols + cb + threadIdx.x] =
        (part[0][threadIdx.x] + part[1][threadIdx.x]) + (part[2][threadIdx.x] + part[3][threadIdx.x]);
}

// centre from the partial sums, then this workgroup's rows (one wave per row, lane l the columns l, l + 64, ...): largest
// |a_ik - c_k| and largest |a_i - c|^2 as bit patterns (NaN / inf -> all ones)
__global__ __launch_bounds__(256) void k_wide_ref_extent(const double *__restrict__ refR, int n, int dp, const double *__restrict__ scratch,
                                                         unsigned long long *__restrict__ maxima, double *__restrict__ stats) {
  __shared__ double cc[kWideStatCols];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  for (int c = threadIdx.x; c < dp; c += 256) {
    double tot = 0.0;
    for (int b = 0; b < kWideStatBlocks; ++b) tot += scratch[(size_t)b * kWideStatCols + c];
    cc[c] = tot / (double)n;
    if (blockIdx.x == 0) stats[8 + c] = cc[c];
  }
  __syncthreads();
  double amax = 0.0, n2max = 0.0;
  bool finite = true;
  for (int i = blockIdx.x * 4 + wave; i < n; i += 4 * kWideStatBlocks) {
    double sq = 0.0;
    for (int c = lane; c < dp; c += 64) {
      const double v = refR[(size_t)i * dp + c] - cc[c];
      if (!(fabs(v) <= 1.7e308)) finite = false;
      amax = fmax(amax, fabs(v));
      sq += v * v;
    }
    for (int off = 32; off > 0; off >>= 1) sq += __shfl_xor(sq, off, 64);
    n2max = fmax(n2max, sq);
  }
  for (int off = 32; off > 0; off >>= 1) amax = fmax(amax, __shfl_xor(amax, off, 64));
  const bool all_finite = __all(finite) && amax <= 1.7e308 && n2max <= 1.7e308;
  if (lane == 0) {
    atomicMax(&maxima[0], all_finite ? (unsigned long long)__double_as_longlong(amax) : ~0ull);
    atomicMax(&maxima[1], all_finite ? (unsigned long long)__double_as_longlong(n2max) : ~0ull);
  }
}

__global__ void k_wide_ref_finish(unsigned long long *maxima, double *stats) {
  const unsigned long long a = maxima[0], q = maxima[1];
  maxima[0] = maxima[1] = 0ull;   // ready for the next set of live points
  const bool finite = a != ~0ull && q != ~0ull;
  const double amax_all = finite ? __longlong_as_double((long long)a) : INFINITY;
  double sigma = 1.0;
  if (amax_all > 0.0 && amax_all < 1e300) {
    int e;
    frexp(amax_all, &e);  // amax = m * 2^e, m in [0.5, 1)  ->  sigma*amax in [0.5, 1)
    sigma = ldexp(1.0, -e);
  }
  // sigma is a power of two: |sigma (a_i - c)| = sigma |a_i - c| exactly; 1e-12 covers the rounding of the row sums
  // (1024 terms: 1.2e-13 relative)
  const double nmax = finite ? sigma * sqrt(__longlong_as_double((long long)q)) : INFINITY;
  stats[0] = sigma;
  stats[1] = nmax * (1.0 + 1e-12);
  stats[2] = amax_all;
  stats[3] = (amax_all < 1e300) ? 1.0 : 0.0;
}

// ---------------------------------------------------------------- live points -> f16 fragments
// one wave per live-point row (rows >= n are sentinels that can never be hit), lane l the 16-byte pieces (8 columns) l, l + 64
// and l + 128 (K / 8 <= 130 pieces).  The layout is k_quant_refs': coordinates, three pieces of |ah|^2 (x 1 in the queries),
// three columns of ones (x the pieces of |bh|^2), zeros.
// |ah|^2: every product hv * hv is exact in binary64 (11-bit significands: 22 bits), and so is the sum of up to 1024 of them
// whenever the products span less than 53 - 10 = 43 binary places (|hv| <= 1, so: no coordinate below 2^-21 next to one near
// 1).  Where they span more (binary16 subnormals next to full-size coordinates) each of the < 1024 + 6 additions rounds by at
// most 2^-53 of the sum: 2^-42 |ah|^2 in all, inside the 2^-32 w^2 that wide_thresholds grants the norm columns.
__global__ __launch_bounds__(256) void k_wide_quant_refs(const double *__restrict__ refR, int n, int npad32, int d, int ks,
                                                         const double *__restrict__ stats, half_t *__restrict__ refF) {
  const int lane = threadIdx.x & 63;
  const int i = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (i >= npad32) return;   // whole waves leave together
  const int K = ks * 16;
  const double sigma = stats[0];
  const bool have = i < n;
  const double *row = refR + (size_t)(have ? i : 0) * d;
  half8pack pk[3];
  double na = 0.0;
#pragma unroll
  for (int u = 0; u < 3; ++u) {
    const int k0 = 8 * (lane + 64 * u);
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      const int k = k0 + j;
      half_t h = (half_t)0.0f;
      if (have && k < d) {
        h = (half_t)(float)(sigma * (row[k] - stats[8 + k]));
        const double hv = (double)(float)h;
        na += hv * hv;
      }
      pk[u].h[j] = h;
    }
  }
  for (int o = 32; o > 0; o >>= 1) na += __shfl_xor(na, o, 64);
  half_t p[3];
  if (have) {
    split3(na, p);
  } else {
    p[0] = (half_t)60000.0f;  // sentinel row: Dt >= 60000 > every admissible T_hi
    p[1] = p[2] = (half_t)0.0f;
  }
#pragma unroll
  for (int u = 0; u < 3; ++u) {
    const int k0 = 8 * (lane + 64 * u);
    if (k0 >= K) continue;
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      const int k = k0 + j;
      if (k >= d && k < d + 3)
        pk[u].h[j] = p[k - d];               // x 1 in the queries
      else if (k >= d + 3 && k < d + 6)
        pk[u].h[j] = (half_t)1.0f;           // x |bh|^2 pieces
    }
    *reinterpret_cast<half8pack *>(refF + frag_index(i, k0, ks)) = pk[u];   // 16-byte aligned: k0 is a multiple of 8
  }
}

// ---------------------------------------------------------------- thresholds ------------------
// filter_thresholds (mlf_filter_dev.hpp) for K = 160 ... 1040 columns; derivation in DESIGN.md 4b.  What changes with K:
//   input rounding   2 sqrt(K) 2^-24 (binary16 subnormals, per column) is a function of K already;
//   accumulation     one chain of K products per pair, never split: at most K binary32 roundings (one per product in the
//                    pessimistic model), each <= 2^-24 of sum |products| <= w^2.  Coefficient = the power of two >= K 2^-24,
//                    not below the 2^-15 of the narrow kernels: 2^-15 up to K = 512, 2^-14 up to 1024, 2^-13 at K = 1040;
//   norm columns     each squared norm rides as three binary16 pieces: what the third piece drops is <= 2^-33 of the norm
//                    (|ah|^2 < 1040, but |bh|^2 up to the guard's 3e4: 2^-33 (|ah|^2 + |bh|^2) <= 2^-33 w^2 -- the term
//                    2^-32 w^2, which also covers the binary64 sums of the norms, 2^-42 relative) or half a binary16
//                    subnormal step per norm (2^-25 each): the absolute term 2^-20;
//   the reference    sequential binary64 sum of d <= 1024 terms: |s - D| <= 2^-42 D, inside the factors 1 -+ 2^-30 of sqrt(r2).
__device__ __forceinline__ bool wide_thresholds(double sigma, double namax, double nbn2, double r2, int K, float *lo_f, float *hi_f) {
  const double nbn = sqrt(nbn2);
  const double delta = 0x1p-11 * (1.0 + 0x1p-9) * (namax + nbn) + 2.0 * sqrt((double)K) * 0x1p-24 + 0x1p-40 * (namax + nbn);
  const double w = namax + nbn + 0x1p-8;
  double coef = 0x1p-15;
  while (coef < (double)K * 0x1p-24) coef *= 2.0;
  const double eacc = (coef + 0x1p-32) * w * w + 0x1p-20;
  const double sr = sigma * sqrt(r2);
  const double lo = sr * (1.0 - 0x1p-30) - delta;
  const double hi = sr * (1.0 + 0x1p-30) + delta;
  // never negative and finite: the sweep takes minima on the bit patterns (see filter_thresholds)
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

// ---------------------------------------------------------------- queries -> f16 fragments ---
// one wave per query, lane l the 16-byte pieces l, l + 64, l + 128.  route: 0 = outside the ellipsoid (answered here), 1 =
// filtered, 2 = exact scan only (a coordinate that does not fit binary16, NaN / inf, T_hi >= 3e4; listed in qlist), 3 = farther
// from the centre than any live point plus the radius (answered here).  |bh|^2 is exact as in
// k_wide_quant_refs; |sigma (b - c)|^2 enters the thresholds with 2^-40 relative slack, far above what the order of a
// binary64 sum of 1024 terms can move.
__global__ __launch_bounds__(256) void k_wide_quant_queries(WideQuantArgs a) {
  const int lane = threadIdx.x & 63;
  const long long p = (long long)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (blockIdx.x == 0 && threadIdx.x == 0) *a.band_count = 0;
  if (p >= a.nqpad) return;   // whole waves leave together
  const int K = a.ks * 16, d = a.d;
  const double sigma = a.stats[0], namax = a.stats[1];
  int rt = 0;
  if (p < a.nq && (a.gate == nullptr || a.gate[p])) rt = 1;
  const double *row = a.q + (p < a.nq ? p : 0) * a.ldq;
  half8pack pk[3];
  double nb = 0.0, nbn2 = 0.0;
  bool fits = true;
#pragma unroll
  for (int u = 0; u < 3; ++u) {
    const int k0 = 8 * (lane + 64 * u);
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      const int k = k0 + j;
      half_t h = (half_t)0.0f;
      if (rt == 1 && k < d) {
        const double x = sigma * ((k < a.d_src ? row[k] : 0.0) - a.stats[8 + k]);
        if (!(fabs(x) <= 16000.0)) fits = false;  // -2x must stay well inside binary16; NaN lands here too
        nbn2 += x * x;
        const half_t xh = (half_t)(float)x;
        const double hv = (double)(float)xh;
        nb += hv * hv;
        h = (half_t)(-2.0f * (float)xh);   // exact
      }
      pk[u].h[j] = h;
    }
  }
  for (int o = 32; o > 0; o >>= 1) {
    nbn2 += __shfl_xor(nbn2, o, 64);
    nb += __shfl_xor(nb, o, 64);
  }
  fits = __all(fits);
  // Certain miss by the norms alone, whatever the size of the coordinates: |a - b| >= |b - c| - |a - c| for every live point a.
  // sigma |b - c| >= sqrt(nbn2) (1 - 2^-41) (rounded centring 2^-53 per coordinate, 1025 additions, the root), sigma |a - c| <=
  // namax (k_wide_ref_finish), and the reference's sequential sum s >= D (1 - 2^-42): s > r2 follows from
  // sqrt(nbn2) (1 - 2^-30) - namax > sigma sqrt(r2) (1 + 2^-30).  NaN / inf compare false and stay on their way to the exact scan.
  // These are the proposals the binary16 guard below would hand to the exact scan at high dimensionality (|sigma (b - c)|^2 >
  // 3e4 with sigma = 4 and |t|^2 near 2 d at d = 1024) -- every one of them a whole sweep of the live points there.
  if (rt == 1 && nbn2 <= 1e300 && sqrt(nbn2) * (1.0 - 0x1p-30) - namax > sigma * sqrt(a.r2) * (1.0 + 0x1p-30)) rt = 3;
  // (what is left for the magnitude half of `fits` is NaN / inf: a finite row with a coordinate above 16000 has nbn2 > 2.5e8
  // and was a certain miss by the norms just above -- namax + sigma sqrt(r2) stays below 100 for an eligible batch)
  if (rt == 1 && (!fits || !(nbn2 <= 30000.0))) rt = 2;
  half_t pc[3] = {(half_t)0.0f, (half_t)0.0f, (half_t)0.0f};
  float lo_f = -1.0f, hi_f = -1.0f;
  if (rt == 1) {
    split3(nb, pc);
    if (!wide_thresholds(sigma, namax, nbn2, a.r2, K, &lo_f, &hi_f)) {
      rt = 2;
      lo_f = hi_f = -1.0f;
    }
  }
  half_t *qF = reinterpret_cast<half_t *>(a.qF) + (size_t)(p >> 5) * ((size_t)a.ks * 512);
  const int pr = (int)(p & 31);
#pragma unroll
  for (int u = 0; u < 3; ++u) {
    const int k0 = 8 * (lane + 64 * u);
    if (k0 >= K) continue;
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      const int k = k0 + j;
      if (rt != 1)
        pk[u].h[j] = (half_t)0.0f;
      else if (k >= d && k < d + 3)
        pk[u].h[j] = (half_t)1.0f;
      else if (k >= d + 3 && k < d + 6)
        pk[u].h[j] = pc[k - d - 3];
    }
    *reinterpret_cast<half8pack *>(qF + frag_index(pr, k0, a.ks)) = pk[u];
  }
  if (lane == 0) {
    a.tlo[p] = lo_f;
    a.thi[p] = hi_f;
    if (p < a.nq) {
      a.route[p] = (uint8_t)rt;
      if (rt == 0 || rt == 3) a.out_mask[p] = 0;
      if (rt == 2) a.qlist[atomicAdd(a.qcount, 1u)] = (int)p;   // rare: guard cases only
    }
  }
}

// ---------------------------------------------------------------- the sweep ------------------
// Workgroup = 8 waves and G query groups of 32.  The groups' operand ([G][ks][64 lanes][8 halves], the layout it has in HBM)
// is copied into LDS once; wave w then takes the live tiles w, w + 8, ... (rotated per workgroup: all workgroups on one tile
// at one moment would queue on one L2 channel).  Per tile: the k-loop in chunks of kWideKC k-steps -- the chunk's four 1 KiB
// fragment loads of the live tile are in flight while the chunk before it feeds G matrix instructions per k-step from LDS
// (ds_read_b128, lane-consecutive: conflict free) into G accumulator blocks -- then 8 integer min3 per group on the bit
// patterns (mlf_sweep_dev.hpp: tree_min).  The waves' minima meet in LDS (atomicMin on the patterns: a negative Dt has a negative
// pattern and wins, which is all the tests below need -- T_lo is never negative and finite).
constexpr int kWideSweepThreads = 512;
constexpr int kWideKC = 4;

template <int G>
__global__ __launch_bounds__(kWideSweepThreads) void k_wide_sweep(WideSweepArgs a) {
  extern __shared__ __attribute__((aligned(16))) uint4 qs[];   // [G][ks][64]
  __shared__ int qmin[G * 32];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const long long g0 = (long long)blockIdx.x * G;
  const int ks = a.ks, per = ks * 64;   // 16-byte pieces of one group / one tile
  {
    const uint4 *src = reinterpret_cast<const uint4 *>(a.qF);
    for (int e = tid; e < G * per; e += kWideSweepThreads) {
      const int g = e / per;
      qs[e] = g0 + g < a.ngroups ? src[(size_t)(g0 + g) * per + (e - g * per)] : make_uint4(0u, 0u, 0u, 0u);
    }
  }
  if (tid < G * 32) qmin[tid] = 0x7f800000;   // +inf
  __syncthreads();

  const half8 *refF = reinterpret_cast<const half8 *>(a.refF);
  const half8 *qh = reinterpret_cast<const half8 *>(qs);
  int vmin[G];
#pragma unroll
  for (int g = 0; g < G; ++g) vmin[g] = 0x7f800000;
  const int nt = a.ntiles32;
  const int tstart = (int)(((long long)blockIdx.x * 37) % nt);
  auto tile_of = [&](int it) {
    const int t = tstart + it;
    return t >= nt ? t - nt : t;
  };
  auto load_chunk = [&](half8 (&dst)[kWideKC], int t, int s0) {   // k-steps past the last repeat it (never used)
    const half8 *at = refF + (size_t)t * per + lane;
#pragma unroll
    for (int j = 0; j < kWideKC; ++j) dst[j] = at[(s0 + j < ks ? s0 + j : ks - 1) * 64];
  };
  half8 cur[kWideKC], nxt[kWideKC];
  if (wave < nt) load_chunk(cur, tile_of(wave), 0);
  for (int it = wave; it < nt; it += kWideSweepThreads / 64) {
    const int t = tile_of(it);
    float16v acc[G];
#pragma unroll
    for (int g = 0; g < G; ++g) acc[g] = (float16v){0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
    for (int s0 = 0; s0 < ks; s0 += kWideKC) {
      // the next chunk of this tile, or the first of the wave's next tile (the last iteration of all requests its own again)
      const bool more = s0 + kWideKC < ks;
      const int itn = it + kWideSweepThreads / 64;
      load_chunk(nxt, more ? t : (itn < nt ? tile_of(itn) : t), more ? s0 + kWideKC : 0);
#pragma unroll
      for (int j = 0; j < kWideKC; ++j) {
        if (s0 + j < ks) {   // wave-uniform
#pragma unroll
          for (int g = 0; g < G; ++g) acc[g] = __builtin_amdgcn_mfma_f32_32x32x16_f16(cur[j], qh[(g * ks + s0 + j) * 64 + lane], acc[g], 0, 0, 0);
        }
      }
#pragma unroll
      for (int j = 0; j < kWideKC; ++j) cur[j] = nxt[j];
    }
    // all 16 values of a lane belong to ONE query (column = lane & 31) and 16 live points
#pragma unroll
    for (int g = 0; g < G; ++g) {
      vmin[g] = tree_min(acc[g], vmin[g]);
    }
  }
#pragma unroll
  for (int g = 0; g < G; ++g)
    if (vmin[g] != 0x7f800000) atomicMin(&qmin[g * 32 + (lane & 31)], vmin[g]);
  __syncthreads();
  if (tid < 64) {   // one wave answers: G * 32 <= 128 queries, two rounds at most
    unsigned nband = 0;
    for (int e = tid; e < G * 32; e += 64) {
      const long long grp = g0 + (e >> 5);
      const long long q = grp * 32 + (e & 31);
      bool band = false;
      if (grp < a.ngroups && q < a.nq && a.route[q] == 1) {
        const float m = __int_as_float(qmin[e]);
        if (m <= a.tlo[q])
          a.out_mask[q] = 1;          // certain hit
        else if (m > a.thi[q])
          a.out_mask[q] = 0;          // certain miss of every live point
        else {
          a.route[q] = 2;             // the minimum ended in the band (or is NaN): the exact scan decides
          band = true;
        }
      }
      const unsigned long long bm = __ballot(band);
      if (bm != 0ull) {   // wave-uniform: one slot request for the wave's band queries
        unsigned base = 0;
        if (tid == 0) base = atomicAdd(a.qcount, (unsigned)__popcll(bm));
        base = (unsigned)__builtin_amdgcn_readfirstlane((int)base);
        if (band) a.qlist[base + (unsigned)__popcll(bm & ((1ull << tid) - 1ull))] = (int)q;
      }
      nband += (unsigned)__popcll(bm);
    }
    if (tid == 0 && nband) atomicAdd(a.band_count, nband);
  }
}

// dynamic LDS above the default grant (48 KB) has to be granted per kernel instance and device
template <int G>
hipError_t launch_wide_sweep_t(const WideSweepArgs &a, hipStream_t s) {
  const size_t lds = (size_t)G * a.ks * 1024;
  static DeviceGrant grant;
  if (lds > 48 * 1024) {
    const void *fn = reinterpret_cast<const void *>(&k_wide_sweep<G>);
    if (hipError_t e = grant.ensure([fn] { return hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, 152 * 1024); })) return e;
  }
  const unsigned grid = (unsigned)((a.ngroups + G - 1) / G);
  hipLaunchKernelGGL(k_wide_sweep<G>, dim3(grid), dim3(kWideSweepThreads), lds, s, a);
  return hipGetLastError();
}

}  // namespace

void launch_wide_ref_stats(const double *refR, int n, int dp, double *stats, double *scratch, hipStream_t s) {
  unsigned long long *maxima = reinterpret_cast<unsigned long long *>(scratch + (size_t)kWideStatBlocks * kWideStatCols);
  hipLaunchKernelGGL(k_wide_ref_colsum, dim3(kWideStatBlocks, (unsigned)((dp + 127) / 128)), dim3(256), 0, s, refR, n, dp, scratch);
  hipLaunchKernelGGL(k_wide_ref_extent, dim3(kWideStatBlocks), dim3(256), 0, s, refR, n, dp, scratch, maxima, stats);
  hipLaunchKernelGGL(k_wide_ref_finish, dim3(1), dim3(1), 0, s, maxima, stats);
}

void launch_wide_quant_refs(const double *refR, int n, int npad32, int dp, int ks, const double *stats, void *refF, hipStream_t s) {
  hipLaunchKernelGGL(k_wide_quant_refs, dim3((unsigned)((npad32 + 3) / 4)), dim3(256), 0, s, refR, n, npad32, dp, ks, stats,
                     reinterpret_cast<half_t *>(refF));
}

hipError_t launch_wide_quant_queries(const WideQuantArgs &a, hipStream_t s) {
  if (a.nqpad <= 0) return hipSuccess;
  if (a.ks < kWideFilterMinKs || a.ks > kWideFilterMaxKs || a.d > kWideStatCols) return hipErrorInvalidValue;
  hipLaunchKernelGGL(k_wide_quant_queries, dim3((unsigned)((a.nqpad + 3) / 4)), dim3(256), 0, s, a);
  return hipGetLastError();
}

// One 32-query group is ks KiB of LDS (66.5 KB at K = 1040).  Four groups per workgroup where they fit 152 KB less the static
// arrays (ks <= 37: d <= 576) and the batch still fills the chip with them; else two (133 KB at ks = 65).
int wide_sweep_groups(int ks, long long ngroups) { return (ks <= 37 && ngroups >= 2048) ? 4 : 2; }

hipError_t launch_wide_sweep(const WideSweepArgs &a, hipStream_t s) {
  if (a.ngroups <= 0) return hipSuccess;
  if (a.ks < kWideFilterMinKs || a.ks > kWideFilterMaxKs || a.ntiles32 < 1) return hipErrorInvalidValue;
  return wide_sweep_groups(a.ks, a.ngroups) == 4 ? launch_wide_sweep_t<4>(a, s) : launch_wide_sweep_t<2>(a, s);
}

}  // namespace mlf
