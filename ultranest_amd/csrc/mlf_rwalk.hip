// mlf_rwalk.hip -- PopulationRandomWalkSampler's refill on the device (reference ultranest/popstepsampler.py:299-353).
//
// P walkers start from random live points and make nsteps moves each; walkers never interact.  One move: a direction v
// (dw_direction, the generators of the slice sampler), the part [tleft, tright] of the line u + t v inside the unit cube, a
// standard normal t truncated to it, the proposal u + v t, prior transform, likelihood, accept iff inside and L > Lmin.
//
// Two forms with the same results, bit for bit (tests/test_randomwalk_device.py):
//   chain   any d <= kWideDirMaxDim (above 128: k_rwalk_propose_wide), any layer, user models.  Per step three launches: k_rwalk_propose, the evaluation (the user model's
//           kernel with the cube flag as member mask; launch_loglike has no mask and evaluates every row -- the value of a
//           proposal outside the cube is never read: k_rwalk_accept tests the flag first), k_rwalk_accept.  State in HBM.
//   fused   built-in models, even d <= 64, affine layer or none: one launch, a wave owns a walker, (u, p, L, flags) stay in
//           registers across the steps.  The stages are the SAME device functions: dw_direction, line_cube_wave,
//           truncnorm_draw, rwalk_move / rwalk_transform, loglike_pairs (documented bit-identical to launch_loglike).
// Both end with the same two kernels (move diagnostics, counts).
//
// Philox counters (seed, offset of the call; nothing depends on P, the launch shape or the form):
//   stream 2  direction of walker i at step s: dw_direction's block group (i * nsteps + s), (npairs + 2) blocks each
//   stream 7  walker i owns blocks offset + i * (nsteps + 1) + [0, nsteps]: block 0 word 0 = the start row (below(word,
//             nlive)), block 1 + s words 0, 1 = the truncation uniform of step s
// One refill advances the offset by P * nsteps * (npairs + 2) (stream 7 needs fewer).
#include "mlf_rwalk.hpp"

#include <math.h>

#include "mlf_loglike_dev.hpp"
#include "mlf_misc.hpp"
#include "mlf_philox_dev.hpp"
#include "mlf_walk_dev.hpp"

namespace mlf {

namespace {

constexpr unsigned kRwalkStream = 7u;

__device__ __forceinline__ long long rwalk_start_row(const RwalkArgs &a, int i) {
  unsigned r4[4];
  philox_block(a.seed, kRwalkStream, a.offset + (unsigned long long)i * (unsigned long long)(a.w.nsteps + 1), r4);
  return (long long)below(r4[0], (unsigned)a.nlive);
}

__device__ __forceinline__ double rwalk_uniform(const RwalkArgs &a, int i, int step) {
  unsigned r4[4];
  philox_block(a.seed, kRwalkStream,
               a.offset + (unsigned long long)i * (unsigned long long)(a.w.nsteps + 1) + 1ull + (unsigned long long)step, r4);
  return u01(r4[0], r4[1]);
}

// Standard normal truncated to [a, b] by inverse CDF from one uniform q, evaluated on the side of the smaller tail (the
// distribution of scipy.stats.truncnorm.rvs(a, b)): p = Phi(a) + q (Phi(b) - Phi(a)); p <= 0.5: Phi^-1(p), else
// -Phi^-1(Q(b) + (1 - q)(Q(a) - Q(b))) with Q(x) = Phi(-x); clamped to [a, b]
__device__ __noinline__ double truncnorm_draw(double a, double b, double q) {
  const double Fa = normcdf(a), Fb = normcdf(b);
  const double p = Fa + q * (Fb - Fa);
  double t;
  if (p <= 0.5) {
    t = normcdfinv(p);
  } else {
    const double Qa = normcdf(-a), Qb = normcdf(-b);
    t = -normcdfinv(Qb + (1.0 - q) * (Qa - Qb));
  }
  return fmin(fmax(t, a), b);
}

}  // namespace

// ------------------------------------------------------------------ chain form -----------------------------------------
__global__ __launch_bounds__(64) void k_rwalk_start(RwalkArgs a) {
  const RwalkState &w = a.w;
  const int lane = threadIdx.x, d = w.d;
  for (int i = blockIdx.x; i < w.P; i += gridDim.x) {
    const long long row = rwalk_start_row(a, i);
    for (int k = lane; k < d; k += 64) {
      w.u[(size_t)i * d + k] = a.live[(size_t)row * d + k];
      w.p[(size_t)i * d + k] = qnan();
    }
    if (lane == 0) {
      w.L[i] = a.Ls[row];
      w.start[i] = row;
      w.ever[i] = 0;
      w.last[i] = 0;
      w.rej[i] = 0;
      w.tl[i] = qnan();
      w.tr[i] = qnan();
    }
  }
}

__global__ __launch_bounds__(64) void k_rwalk_propose(RwalkArgs a, int step) {
  const RwalkState &w = a.w;
  const int lane = threadIdx.x, d = w.d;
  const WalkState ws = direction_state(d);
  for (int i = blockIdx.x; i < w.P; i += gridDim.x) {
    double uo[2] = {0.0, 0.0}, vr[2];
#pragma unroll
    for (int h = 0; h < 2; ++h)
      if (lane + 64 * h < d) uo[h] = w.u[(size_t)i * d + lane + 64 * h];
    dw_direction(ws, i * w.nsteps + step, lane, a.dirkind, a.dirscale, a.dd, a.seed, a.offset, vr);
    double lo, hi;
    line_cube_wave(uo, vr, d, lane, lo, hi);
    const double t = truncnorm_draw(lo, hi, rwalk_uniform(a, i, step));
    bool ok = true;
#pragma unroll
    for (int h = 0; h < 2; ++h) {
      const int c = lane + 64 * h;
      if (c < d) {
        const double x = rwalk_move(uo[h], vr[h], t);
        w.unew[(size_t)i * d + c] = x;
        ok = ok && inside_open_unit(x);
        if (a.tkind >= 0) w.pnew[(size_t)i * d + c] = rwalk_transform(a.tkind, x, a.ta, a.tb);
      }
    }
    const bool all_ok = __all(ok);
    if (lane == 0) {
      w.inside[i] = all_ok ? 1 : 0;
      w.tl[i] = lo;
      w.tr[i] = hi;
    }
  }
}

// The wide form: kNarrowDirMaxDim < d <= kWideDirMaxDim (enforced by mlf_rwalk_create; every row and LDS access below is
// bounded by it).  The lanes stride over the row, c = lane, lane + 64, ...  The direction goes through dw_direction_wide into
// the walker's row of unew: kind 4 writes v[r] from other lanes than the ones that read it, hence the fence; after it lane l
// reads v[c] and writes the proposal x over it at the SAME c, so no second fence is needed.  The other stages are the
// device functions of the narrow form.  Launched with wide_rwalk_grid: the workgroups walk the population.
__global__ __launch_bounds__(64) void k_rwalk_propose_wide(RwalkArgs a, int step) {
  __shared__ double gs[kWideDirMaxDim];
  const RwalkState &w = a.w;
  const int lane = threadIdx.x, d = w.d;
  for (int i = blockIdx.x; i < w.P; i += gridDim.x) {
    const double *uo = w.u + (size_t)i * d;
    double *v = w.unew + (size_t)i * d;
    dw_direction_wide(d, i * w.nsteps + step, lane, a.dirkind, a.dirscale, a.dd, a.seed, a.offset, v, gs);
    wave_lds_sync();   // (the direction row written above is read back by other lanes of this wave)
    double lo, hi;
    line_cube_wave_wide(uo, v, d, lane, lo, hi);
    const double t = truncnorm_draw(lo, hi, rwalk_uniform(a, i, step));
    bool ok = true;
    for (int c = lane; c < d; c += 64) {
      const double x = rwalk_move(uo[c], v[c], t);
      v[c] = x;
      ok = ok && inside_open_unit(x);
      if (a.tkind >= 0) w.pnew[(size_t)i * d + c] = rwalk_transform(a.tkind, x, a.ta, a.tb);
    }
    const bool all_ok = __all(ok);
    if (lane == 0) {
      w.inside[i] = all_ok ? 1 : 0;
      w.tl[i] = lo;
      w.tr[i] = hi;
    }
  }
}

__global__ __launch_bounds__(64) void k_rwalk_accept(RwalkArgs a) {
  const RwalkState &w = a.w;
  const int lane = threadIdx.x, d = w.d;
  for (int i = blockIdx.x; i < w.P; i += gridDim.x) {
    const double Lnew = w.Lnew[i];
    const bool acc = w.inside[i] != 0 && Lnew > a.Lmin;   // (a NaN likelihood is rejected)
    if (acc)
      for (int k = lane; k < d; k += 64) {
        w.u[(size_t)i * d + k] = w.unew[(size_t)i * d + k];
        w.p[(size_t)i * d + k] = w.pnew[(size_t)i * d + k];
      }
    if (lane == 0) {
      if (acc) {
        w.L[i] = Lnew;
        w.ever[i] = 1;
      } else {
        w.rej[i] += 1;
      }
      w.last[i] = acc ? 1 : 0;
    }
  }
}

// ------------------------------------------------------------------ fused form -----------------------------------------
// even d <= 64: lane k < d holds coordinate k.  The axes matrix of the region-oriented directions (kinds 3, 4, 6) is staged in
// LDS once per workgroup (dynamic: none for the other kinds): kind 4 reads it d times per step with a row stride between lanes.
__global__ __launch_bounds__(64) void k_rwalk_fused(RwalkArgs a, int stage_axes) {
  extern __shared__ double s_axes[];
  const RwalkState &w = a.w;
  const int lane = threadIdx.x, d = w.d;
  const WalkState ws = direction_state(d);
  WalkDirData dd = a.dd;
  if (stage_axes) {
    for (int e = lane; e < d * d; e += 64) s_axes[e] = a.dd.axes[e];
    dd.axes = s_axes;
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
  }
  const bool have = lane < d;
  int hw = 2;
  while (2 * hw < d) hw *= 2;
  for (int i = blockIdx.x; i < w.P; i += gridDim.x) {
    const long long row = rwalk_start_row(a, i);
    double u = have ? a.live[(size_t)row * d + lane] : 0.0;
    double p = qnan();
    double L = a.Ls[row];
    bool ever = false, last = false;
    int rej = 0;
    double lo = qnan(), hi = qnan();
    for (int step = 0; step < w.nsteps; ++step) {
      double uo[2] = {u, 0.0}, vr[2];
      dw_direction(ws, i * w.nsteps + step, lane, a.dirkind, a.dirscale, dd, a.seed, a.offset, vr);
      line_cube_wave(uo, vr, d, lane, lo, hi);
      const double t = truncnorm_draw(lo, hi, rwalk_uniform(a, i, step));
      const double x = rwalk_move(u, vr[0], t);
      const bool inside = __all(!have || inside_open_unit(x));
      const double pcoord = rwalk_transform(a.tkind, x, a.ta, a.tb);
      bool acc = false;
      double Lnew = 0.0;
      if (inside) {   // wave-uniform; loglike_wave's pair layout: lane l < hw holds parameters 2 l, 2 l + 1
        const double x0 = __shfl(pcoord, (2 * lane) & 63, 64), x1 = __shfl(pcoord, (2 * lane + 1) & 63, 64);
        Lnew = loglike_pairs(a.lkind, x0, x1, d, hw, a.aux, a.sigma, lane);
        acc = Lnew > a.Lmin;
      }
      if (acc) {
        u = x;
        p = pcoord;
        L = Lnew;
        ever = true;
      } else {
        ++rej;
      }
      last = acc;
    }
    if (have) {
      w.u[(size_t)i * d + lane] = u;
      w.p[(size_t)i * d + lane] = p;
    }
    if (lane == 0) {
      w.L[i] = L;
      w.start[i] = row;
      w.ever[i] = ever ? 1 : 0;
      w.last[i] = last ? 1 : 0;
      w.rej[i] = rej;
      w.tl[i] = lo;
      w.tr[i] = hi;
    }
  }
}

// ------------------------------------------------------------------ diagnostics and counts (both forms) ----------------
// the reference diagnoses the walkers that accepted their LAST move (popstepsampler.py:334): start row -> final point
__global__ __launch_bounds__(64) void k_rwalk_dist(RwalkArgs a) {
  const RwalkState &w = a.w;
  const int lane = threadIdx.x, d = w.d;
  for (int i = blockIdx.x; i < w.P; i += gridDim.x) {
    double d2 = qnan();
    if (w.last[i] && a.ly.kind >= 0)   // wave-uniform
      d2 = move_distance_rows(a.ly, d, lane, a.live + (size_t)w.start[i] * d, w.u + (size_t)i * d);
    if (lane == 0) w.dist2[i] = d2;
  }
}

constexpr int kRwalkChunk = 1024;
__device__ __forceinline__ void rwalk_block_sum(double (*part)[kRwalkOut], const double (&v)[kRwalkOut], double *dst) {
  for (int c = 0; c < kRwalkOut; ++c) part[threadIdx.x][c] = v[c];
  __syncthreads();
  for (int off = 128; off > 0; off >>= 1) {
    if ((int)threadIdx.x < off)
      for (int c = 0; c < kRwalkOut; ++c) part[threadIdx.x][c] += part[threadIdx.x + off][c];
    __syncthreads();
  }
  if (threadIdx.x < kRwalkOut) dst[threadIdx.x] = part[0][threadIdx.x];
}

__global__ __launch_bounds__(256) void k_rwalk_stats(RwalkArgs a) {
  __shared__ double part[256][kRwalkOut];
  const RwalkState &w = a.w;
  const double r2 = a.ly.r2, ref = sqrt(a.ly.r2);
  double v[kRwalkOut] = {0, 0, 0, 0, 0};
  const int i0 = blockIdx.x * kRwalkChunk;
  for (int j = threadIdx.x; j < kRwalkChunk; j += 256) {
    const int i = i0 + j;
    if (i >= w.P) continue;
    v[0] += (double)w.rej[i];
    v[4] += w.ever[i] ? 0 : 1;
    if (!w.last[i]) continue;
    v[1] += 1;
    const double d2 = w.dist2[i];
    if (!isnan(d2)) {
      v[2] += (d2 > r2) ? 1 : 0;
      v[3] += log(sqrt(d2) / ref + 1e-10);
    }
  }
  rwalk_block_sum(part, v, a.parts + (size_t)blockIdx.x * kRwalkOut);
}

__global__ __launch_bounds__(256) void k_rwalk_stats_sum(RwalkArgs a, int nchunks) {
  __shared__ double part[256][kRwalkOut];
  double v[kRwalkOut] = {0, 0, 0, 0, 0};
  for (int b = threadIdx.x; b < nchunks; b += 256)
    for (int c = 0; c < kRwalkOut; ++c) v[c] += a.parts[(size_t)b * kRwalkOut + c];
  rwalk_block_sum(part, v, a.out);
}

// ------------------------------------------------------------------ launchers -------------------------------------------
// one one-wave workgroup per walker (mlf_walk.hip: walker_grid)
static inline dim3 rwalk_grid(int P) { return dim3((unsigned)(P < (1 << 22) ? P : (1 << 22))); }

// the wide propose kernel: the grid of the wide slice walkers (mlf_walk.hip: wide_walker_grid), each workgroup 8 KiB of LDS
static inline dim3 wide_rwalk_grid(int P) { return dim3((unsigned)(P < (1 << 13) ? P : (1 << 13))); }

unsigned long long rwalk_philox_per_refill(int P, int nsteps, int d) {
  return (unsigned long long)P * (unsigned long long)nsteps * (unsigned long long)((d + 1) / 2 + 2);
}

bool rwalk_fused_covers(int d, int layer_kind) { return !(d & 1) && d <= 64 && layer_kind <= 0; }

void launch_rwalk_start(const RwalkArgs &a, hipStream_t s) {
  hipLaunchKernelGGL(k_rwalk_start, rwalk_grid(a.w.P), dim3(64), 0, s, a);
}

void launch_rwalk_propose(const RwalkArgs &a, int step, hipStream_t s) {
  if (a.w.d > kNarrowDirMaxDim)
    hipLaunchKernelGGL(k_rwalk_propose_wide, wide_rwalk_grid(a.w.P), dim3(64), 0, s, a, step);
  else
    hipLaunchKernelGGL(k_rwalk_propose, rwalk_grid(a.w.P), dim3(64), 0, s, a, step);
}

void launch_rwalk_accept(const RwalkArgs &a, hipStream_t s) {
  hipLaunchKernelGGL(k_rwalk_accept, rwalk_grid(a.w.P), dim3(64), 0, s, a);
}

void launch_rwalk_fused(const RwalkArgs &a, hipStream_t s) {
  const bool stage = a.dirkind == DIR_REGION_ORIENTED || a.dirkind == DIR_REGION_RANDOM || a.dirkind == DIR_MIXTURE;
  // with the matrix staged, 2048 workgroups walk the population: it is copied 2048 times, not once per walker
  const dim3 grid = stage && a.w.P > 2048 ? dim3(2048) : rwalk_grid(a.w.P);
  const size_t lds = stage ? (size_t)a.w.d * a.w.d * sizeof(double) : 0;
  hipLaunchKernelGGL(k_rwalk_fused, grid, dim3(64), lds, s, a, stage ? 1 : 0);
}

void launch_rwalk_finish(const RwalkArgs &a, hipStream_t s) {
  const int nchunks = (a.w.P + kRwalkChunk - 1) / kRwalkChunk;
  hipLaunchKernelGGL(k_rwalk_dist, rwalk_grid(a.w.P), dim3(64), 0, s, a);
  hipLaunchKernelGGL(k_rwalk_stats, dim3(nchunks), dim3(256), 0, s, a);
  hipLaunchKernelGGL(k_rwalk_stats_sum, dim3(1), dim3(256), 0, s, a, nchunks);
}

}  // namespace mlf
