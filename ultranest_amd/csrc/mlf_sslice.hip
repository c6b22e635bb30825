// mlf_sslice.hip -- PopulationSimpleSliceSampler's refill on the device (reference ultranest/popstepsampler.py:907-1002,
// stepfuncs.pyx:537-630).
//
// P points start from random live points and make nsteps slice steps each.  A step draws a direction v per point and the slice
// [tl, tr] = the line's part inside the unit cube (or that clipped to [-1, 1]); then, iteration by iteration, every one of
// the P workers draws t uniformly in the slice of the point it serves, the proposal u + t v is transformed and evaluated,
// and the update walks the workers IN WORKER ORDER: a t outside the point's current slice is skipped (a discard if its L
// passes), a t inside shrinks the slice towards 0, and the first one inside with L > Lmin becomes the point's successor.
// Workers of finished points are dealt round-robin to the unfinished ones.  The step ends when every point has a
// successor or after max_it iterations.
//
// How many iterations a step takes is known on the device only, so ONE launch sequence serves every iteration -- a slot:
//   k_sslice_propose   wave per worker (lane = coordinate pair, the random walk's layout; above 128 dimensions
//                      k_sslice_propose_wide, the lanes striding over the row).  it == 0: worker j serves point j
//                      and first draws the step's direction and slice.  it > 0: worker j serves zlist[j % nz]
//   evaluation         launch_loglike, or the user model's kernel with w.member as its mask
//   k_sslice_update    wave per unfinished point.  The workers of the point at list position q are q, q + nz, q + 2 nz, ...
//                      in worker order: no search.  64 of them are loaded at a time; the wave repeats {ballot the lanes whose
//                      t lies inside the current slice, apply the first, count the passing lanes skipped before it}:
//                      O(shrink events) rounds, not O(workers) dependent loads.  With shrink > 1 the bounds are no prefix
//                      minimum (a skipped t may satisfy t / shrink < hi), which is why the order of application is kept
//   k_sslice_deal      one workgroup: ordered compaction of status == 0 into zlist, then it += 1; at the end of a step the
//                      widths row is written, the step advanced and it reset; after the last step `finished` is set
// The control block w.ctl says what a slot does; only k_sslice_deal writes it.  A slot that finds `finished` set exits at
// that load (the propose kernel then zeroes the user model's mask, so that its kernel reads nothing; launch_loglike has no
// mask and evaluates the stale rows once more, into values nobody reads).  No kernel waits for another workgroup.
//
// Philox counters (seed, offset of the call; nothing depends on the launch shape or on how the slots are batched):
//   stream 2  direction of point k at step s: dw_direction's block group (k * nsteps + s), (npairs + 2) blocks each
//   stream 8  block offset + i, word 0: the start row of point i (below(word, nlive));
//             block offset + P + (s * max_it + it) * P + j, words 0, 1: the uniform of worker j in iteration it of step s
// One refill advances the offset by max(P * nsteps * (npairs + 2), P * (1 + nsteps * max_it)).
#include "mlf_sslice.hpp"

#include <math.h>

#include "mlf_philox_dev.hpp"
#include "mlf_walk_dev.hpp"

namespace mlf {

namespace {

constexpr unsigned kSsliceStream = 8u;

__device__ __forceinline__ long long sslice_start_row(const SsliceArgs &a, int i) {
  unsigned r4[4];
  philox_block(a.seed, kSsliceStream, a.offset + (unsigned long long)i, r4);
  return (long long)below(r4[0], (unsigned)a.nlive);
}

__device__ __forceinline__ double sslice_uniform(const SsliceArgs &a, int j, int step, int it) {
  const unsigned long long P = (unsigned long long)a.w.P;
  unsigned r4[4];
  philox_block(a.seed, kSsliceStream,
               a.offset + P + ((unsigned long long)step * (unsigned long long)a.w.max_it + (unsigned long long)it) * P +
                   (unsigned long long)j,
               r4);
  return u01(r4[0], r4[1]);
}

// One worker's turn in the update loop of stepfuncs.pyx:560-600, with its exact comparisons: false = the worker's t lies
// outside [lo, hi] and is skipped (the caller counts it as discarded if its L passes); true = the slice shrinks towards 0,
// and `take` says whether the proposal becomes the point's successor
__device__ __forceinline__ bool sslice_in_range(double t, double lo, double hi) { return !(t > hi || t < lo); }
__device__ __forceinline__ void sslice_apply(double t, bool passes, double shrink, double &lo, double &hi, bool &done, bool &take) {
  if (0 < t && t < hi) hi = t / shrink;
  if (0 > t && t > lo) lo = t / shrink;
  take = passes && !done;
  done = done || take;
}

}  // namespace

__global__ __launch_bounds__(64) void k_sslice_start(SsliceArgs a) {
  const SsliceState &w = a.w;
  const int lane = threadIdx.x, d = w.d;
  for (int i = blockIdx.x; i < w.P; i += gridDim.x) {
    const long long row = sslice_start_row(a, i);
    for (int k = lane; k < d; k += 64) {
      w.u[(size_t)i * d + k] = a.live[(size_t)row * d + k];
      w.p[(size_t)i * d + k] = qnan();
    }
    if (lane == 0) {
      w.L[i] = a.Ls[row];
      w.start[i] = row;
      w.tl[i] = qnan();
      w.tr[i] = qnan();
      w.taken[i] = -1;
      w.taken_it[i] = -1;
    }
  }
}

__global__ __launch_bounds__(64) void k_sslice_propose(SsliceArgs a) {
  const SsliceState &w = a.w;
  const SsliceCtl c = *w.ctl;
  const int lane = threadIdx.x, d = w.d;
  if (c.finished) {
    if (a.tkind < 0)
      for (long long j = (long long)blockIdx.x * 64 + lane; j < w.P; j += (long long)gridDim.x * 64) w.member[j] = 0;
    return;
  }
  const WalkState ws = direction_state(d);
  for (int j = blockIdx.x; j < w.P; j += gridDim.x) {
    double uo[2] = {0.0, 0.0}, vr[2] = {0.0, 0.0};
    double lo, hi;
    int k = j;
    if (c.it > 0) k = w.zlist[j % c.nz];
#pragma unroll
    for (int h = 0; h < 2; ++h)
      if (lane + 64 * h < d) uo[h] = w.u[(size_t)k * d + lane + 64 * h];
    if (c.it == 0) {   // (wave-uniform) the step's direction and slice of point j; no other wave reads them in this launch
      dw_direction(ws, k * w.nsteps + c.step, lane, a.dirkind, a.dirscale[c.step], a.dd, a.seed, a.offset, vr);
      line_cube_wave(uo, vr, d, lane, lo, hi);
      if (a.limit == 1) {
        lo = fmax(lo, -1.0);
        hi = fmin(hi, 1.0);
      }
#pragma unroll
      for (int h = 0; h < 2; ++h)
        if (lane + 64 * h < d) w.v[(size_t)k * d + lane + 64 * h] = vr[h];
      if (lane == 0) {
        w.tl[k] = lo;
        w.tr[k] = hi;
        w.status[k] = 0;
        w.taken[k] = -1;
        w.taken_it[k] = -1;
      }
    } else {
#pragma unroll
      for (int h = 0; h < 2; ++h)
        if (lane + 64 * h < d) vr[h] = w.v[(size_t)k * d + lane + 64 * h];
      lo = w.tl[k];
      hi = w.tr[k];
    }
    const double width = hi - lo;
    const double t = lo + width * sslice_uniform(a, j, c.step, c.it);
#pragma unroll
    for (int h = 0; h < 2; ++h) {
      const int cc = lane + 64 * h;
      if (cc < d) {
        const double x = rwalk_move(uo[h], vr[h], t);
        w.unew[(size_t)j * d + cc] = x;
        if (a.tkind >= 0) w.pnew[(size_t)j * d + cc] = rwalk_transform(a.tkind, x, a.ta, a.tb);
      }
    }
    if (lane == 0) {
      w.t[j] = t;
      if (a.tkind < 0) w.member[j] = 1;
    }
  }
}

// The wide form: kNarrowDirMaxDim < d <= kWideDirMaxDim (enforced by mlf_sslice_create; every row and LDS access below is
// bounded by it).  The lanes stride over the rows, c = lane, lane + 64, ...; at it == 0 the direction goes through
// dw_direction_wide straight into the point's row of w.v (kind 4 writes v[r] from other lanes than the ones that read it,
// hence the fence).  Everything else -- the control block, the member mask, the clip, the draw -- is the narrow form's.
// Launched with wide_sslice_grid: the workgroups walk the workers.
__global__ __launch_bounds__(64) void k_sslice_propose_wide(SsliceArgs a) {
  __shared__ double gs[kWideDirMaxDim];
  const SsliceState &w = a.w;
  const SsliceCtl c = *w.ctl;
  const int lane = threadIdx.x, d = w.d;
  if (c.finished) {
    if (a.tkind < 0)
      for (long long j = (long long)blockIdx.x * 64 + lane; j < w.P; j += (long long)gridDim.x * 64) w.member[j] = 0;
    return;
  }
  for (int j = blockIdx.x; j < w.P; j += gridDim.x) {
    double lo, hi;
    int k = j;
    if (c.it > 0) k = w.zlist[j % c.nz];
    const double *uo = w.u + (size_t)k * d;
    double *v = w.v + (size_t)k * d;
    if (c.it == 0) {   // (wave-uniform) the step's direction and slice of point j; no other wave reads them in this launch
      dw_direction_wide(d, k * w.nsteps + c.step, lane, a.dirkind, a.dirscale[c.step], a.dd, a.seed, a.offset, v, gs);
      wave_lds_sync();   // (the direction row written above is read back by other lanes of this wave)
      line_cube_wave_wide(uo, v, d, lane, lo, hi);
      if (a.limit == 1) {
        lo = fmax(lo, -1.0);
        hi = fmin(hi, 1.0);
      }
      if (lane == 0) {
        w.tl[k] = lo;
        w.tr[k] = hi;
        w.status[k] = 0;
        w.taken[k] = -1;
        w.taken_it[k] = -1;
      }
    } else {
      lo = w.tl[k];
      hi = w.tr[k];
    }
    const double width = hi - lo;
    const double t = lo + width * sslice_uniform(a, j, c.step, c.it);
    for (int cc = lane; cc < d; cc += 64) {
      const double x = rwalk_move(uo[cc], v[cc], t);
      w.unew[(size_t)j * d + cc] = x;
      if (a.tkind >= 0) w.pnew[(size_t)j * d + cc] = rwalk_transform(a.tkind, x, a.ta, a.tb);
    }
    if (lane == 0) {
      w.t[j] = t;
      if (a.tkind < 0) w.member[j] = 1;
    }
  }
}

__global__ __launch_bounds__(64) void k_sslice_update(SsliceArgs a) {
  const SsliceState &w = a.w;
  const SsliceCtl c = *w.ctl;
  if (c.finished) return;
  const int lane = threadIdx.x, d = w.d, P = w.P;
  // it == 0: every point is served by the worker of its own index alone (stride P leaves lane 0 of the first tile)
  const int npoints = c.it == 0 ? P : c.nz;
  const long long stride = npoints;
  for (int q = blockIdx.x; q < npoints; q += gridDim.x) {
    const int k = c.it == 0 ? q : w.zlist[q];
    double lo = w.tl[k], hi = w.tr[k];
    bool done = false;      // (every point in the list has status 0)
    long long taken = -1;
    unsigned long long ndisc = 0;
    for (long long first = q; first < P; first += 64 * stride) {   // 64 workers of the point at a time, in worker order
      const long long j = first + lane * stride;
      const bool valid = j < P;
      double tj = 0.0;
      bool passes = false;
      if (valid) {
        tj = w.t[j];
        passes = w.Lnew[j] > a.Lmin;
      }
      const unsigned long long pass_mask = __ballot(passes);
      unsigned long long todo = __ballot(valid);
      while (todo) {   // (wave-uniform)
        const unsigned long long in = __ballot(valid && sslice_in_range(tj, lo, hi)) & todo;
        if (!in) {     // all that are left lie outside the slice
          ndisc += __popcll(todo & pass_mask);
          break;
        }
        const int f = __builtin_ctzll(in);
        const unsigned long long upto = (2ull << f) - 1ull;          // lanes 0 .. f
        ndisc += __popcll(todo & pass_mask & (upto >> 1));            // skipped before f under the bounds f met
        bool take;
        sslice_apply(__shfl(tj, f, 64), ((pass_mask >> f) & 1ull) != 0, a.shrink, lo, hi, done, take);
        if (take) taken = first + f * stride;
        todo &= ~upto;
      }
    }
    if (taken >= 0) {
      for (int e = lane; e < d; e += 64) {
        w.u[(size_t)k * d + e] = w.unew[(size_t)taken * d + e];
        w.p[(size_t)k * d + e] = w.pnew[(size_t)taken * d + e];
      }
    }
    if (lane == 0) {
      w.tl[k] = lo;
      w.tr[k] = hi;
      if (taken >= 0) {
        w.L[k] = w.Lnew[taken];
        w.status[k] = 1;
        w.taken[k] = (int)taken;
        w.taken_it[k] = c.it;
      }
      if (ndisc) atomicAdd(&w.ctl->discarded, ndisc);   // (an integer sum: the order of the additions does not show)
    }
  }
}

// One workgroup.  At P = 1e5 the compaction is 98 tiles of two barriers each over 100 KB of flags: tens of microseconds per
// slot on one compute unit, next to P-wide launches before it (unmeasured).
__global__ __launch_bounds__(1024) void k_sslice_deal(SsliceArgs a) {
  __shared__ int s_wave[16];
  __shared__ int s_base;
  const SsliceState &w = a.w;
  const SsliceCtl c = *w.ctl;
  if (c.finished) return;
  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6, P = w.P;
  if (tid == 0) s_base = 0;
  __syncthreads();
  for (int k0 = 0; k0 < P; k0 += 1024) {
    const int k = k0 + tid;
    const bool open = k < P && w.status[k] == 0;
    const unsigned long long mask = __ballot(open);
    if (lane == 0) s_wave[wv] = __popcll(mask);
    __syncthreads();
    int before = s_base;
    for (int x = 0; x < wv; ++x) before += s_wave[x];
    if (open) w.zlist[before + __popcll(mask & ((1ull << lane) - 1ull))] = k;
    __syncthreads();
    if (tid == 0) {
      int total = 0;
      for (int x = 0; x < 16; ++x) total += s_wave[x];
      s_base += total;
    }
    __syncthreads();
  }
  const int nz = s_base;
  const int it = c.it + 1;
  const bool step_over = nz == 0 || it >= w.max_it;
  if (step_over)
    for (int k = tid; k < P; k += 1024) w.widths[(size_t)c.step * P + k] = w.tr[k] - w.tl[k];
  if (tid == 0) {
    SsliceCtl n = c;
    n.nz = nz;
    n.total_it = c.total_it + 1;
    n.discarded = w.ctl->discarded;
    n.it = it;
    if (step_over) {
      w.iters[c.step] = it;
      n.step = c.step + 1;
      n.it = 0;
      n.finished = n.step >= w.nsteps ? 1 : 0;
    }
    *w.ctl = n;
  }
}

// ------------------------------------------------------------------ diagnostics and counts -----------------------------
// all points: start row -> final point through the layer (reference :975)
__global__ __launch_bounds__(64) void k_sslice_dist(SsliceArgs a) {
  const SsliceState &w = a.w;
  const int lane = threadIdx.x, d = w.d;
  for (int i = blockIdx.x; i < w.P; i += gridDim.x) {
    double d2 = qnan();
    if (a.ly.kind >= 0) d2 = move_distance_rows(a.ly, d, lane, a.live + (size_t)w.start[i] * d, w.u + (size_t)i * d);
    bool bad = false;
    for (int e = lane; e < d; e += 64) bad = bad || !isfinite(w.p[(size_t)i * d + e]);
    const bool any_bad = __any(bad);
    if (lane == 0) {
      w.dist2[i] = d2;
      w.nanrow[i] = any_bad ? 1 : 0;
    }
  }
}

// one workgroup, a fixed order of additions for a given P
__global__ __launch_bounds__(1024) void k_sslice_stats(SsliceArgs a) {
  __shared__ double part[1024][kSsliceOut];
  const SsliceState &w = a.w;
  const double r2 = a.ly.r2, ref = sqrt(a.ly.r2);
  double v[kSsliceOut] = {0, 0, 0};
  for (int i = threadIdx.x; i < w.P; i += 1024) {
    v[2] += w.nanrow[i] ? 1 : 0;
    const double d2 = w.dist2[i];
    if (!isnan(d2)) {
      v[0] += (d2 > r2) ? 1 : 0;
      v[1] += log(sqrt(d2) / ref + 1e-10);
    }
  }
  for (int c = 0; c < kSsliceOut; ++c) part[threadIdx.x][c] = v[c];
  __syncthreads();
  for (int off = 512; off > 0; off >>= 1) {
    if ((int)threadIdx.x < off)
      for (int c = 0; c < kSsliceOut; ++c) part[threadIdx.x][c] += part[threadIdx.x + off][c];
    __syncthreads();
  }
  if (threadIdx.x < kSsliceOut) a.out[threadIdx.x] = part[0][threadIdx.x];
}

// ------------------------------------------------------------------ launchers -------------------------------------------
// one one-wave workgroup per worker / point (mlf_walk.hip: walker_grid)
static inline dim3 sslice_grid(int P) { return dim3((unsigned)(P < (1 << 22) ? P : (1 << 22))); }

// the wide propose kernel: the grid of the wide slice walkers (mlf_walk.hip: wide_walker_grid), each workgroup 8 KiB of LDS
static inline dim3 wide_sslice_grid(int P) { return dim3((unsigned)(P < (1 << 13) ? P : (1 << 13))); }

unsigned long long sslice_philox_per_refill(int P, int nsteps, int d, int max_it) {
  const unsigned long long dirs = (unsigned long long)P * (unsigned long long)nsteps * (unsigned long long)((d + 1) / 2 + 2);
  const unsigned long long mine = (unsigned long long)P * (1ull + (unsigned long long)nsteps * (unsigned long long)max_it);
  return dirs > mine ? dirs : mine;
}

void launch_sslice_start(const SsliceArgs &a, hipStream_t s) {
  hipLaunchKernelGGL(k_sslice_start, sslice_grid(a.w.P), dim3(64), 0, s, a);
}

void launch_sslice_propose(const SsliceArgs &a, hipStream_t s) {
  if (a.w.d > kNarrowDirMaxDim)
    hipLaunchKernelGGL(k_sslice_propose_wide, wide_sslice_grid(a.w.P), dim3(64), 0, s, a);
  else
    hipLaunchKernelGGL(k_sslice_propose, sslice_grid(a.w.P), dim3(64), 0, s, a);
}

void launch_sslice_update(const SsliceArgs &a, hipStream_t s) {
  hipLaunchKernelGGL(k_sslice_update, sslice_grid(a.w.P), dim3(64), 0, s, a);
}

void launch_sslice_deal(const SsliceArgs &a, hipStream_t s) {
  hipLaunchKernelGGL(k_sslice_deal, dim3(1), dim3(1024), 0, s, a);
}

void launch_sslice_finish(const SsliceArgs &a, hipStream_t s) {
  hipLaunchKernelGGL(k_sslice_dist, sslice_grid(a.w.P), dim3(64), 0, s, a);
  hipLaunchKernelGGL(k_sslice_stats, dim3(1), dim3(1024), 0, s, a);
}

}  // namespace mlf
