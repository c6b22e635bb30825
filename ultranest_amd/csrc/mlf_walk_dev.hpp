// mlf_walk_dev.hpp -- device functions shared by the population step samplers' kernels (mlf_walk.hip: the resident slice
// walkers; mlf_rwalk.hip: the whole-population random walk; mlf_sslice.hip: the whole-population simple slice sampler).
// Every form of a sampler that promises the bits of another calls the SAME function here, stage by stage: the direction
// draw, the cube-line intersection, the move diagnostics.
#pragma once
#include <hip/hip_runtime.h>
#include <math.h>

#include "mlf_philox_dev.hpp"
#include "mlf_refarith_dev.hpp"
#include "mlf_walk.hpp"

namespace mlf {

__device__ __forceinline__ double qnan() { return __longlong_as_double(0x7ff8000000000000ll); }

__device__ __forceinline__ bool inside_open_unit(double x) { return 0.0 < x && x < 1.0; }

// whitened coordinates of one point (T1: fmod wrap, centre, k-ascending FMA chain like BLAS)
__device__ __forceinline__ void whiten_point(const WalkLayer &ly, const double *x, int d, int c, double &out) {
  if (ly.kind == 1) {
    double v = x[c];
    if (ly.wrap && !isnan(ly.wrap[c])) v = mlf_wrap_unit(v, ly.wrap[c]);
    out = (v - ly.ctr[c]) / ly.mat[c];
    return;
  }
  double acc = 0.0;
  for (int k = 0; k < d; ++k) {
    double v = x[k];
    if (ly.wrap && !isnan(ly.wrap[k])) v = mlf_wrap_unit(v, ly.wrap[k]);
    acc = __builtin_fma(v - ly.ctr[k], ly.mat[(size_t)k * d + c], acc);
  }
  out = acc;
}

// ---- unitcube_line_intersection (popstepsampler.py:26-61), nanmax / nanmin semantics ------------------------------------
// the two parameters at which the line o + t v crosses the faces of one coordinate
__device__ __forceinline__ void line_cube_coord(double o, double v, double &t1, double &t2) {
  const double m = 1.0 / v;
  const double nn = m * (o - 0.5);
  const double kk = fabs(m) * 0.5;
  t1 = -nn - kk;
  t2 = -nn + kk;
}
// NaN-skipping max / min (a coordinate the direction does not move along contributes NaN).  Both are exact, so any order of
// combining the coordinates -- one thread walking them, or a wave's shuffle tree -- gives the same two doubles.
__device__ __forceinline__ void nan_skip_max(double &lo, double t1) {
  if (!isnan(t1) && (isnan(lo) || t1 > lo)) lo = t1;
}
__device__ __forceinline__ void nan_skip_min(double &hi, double t2) {
  if (!isnan(t2) && (isnan(hi) || t2 < hi)) hi = t2;
}
// one line by one thread: o, v = rows of d coordinates
__device__ __forceinline__ void line_cube_row(const double *o, const double *v, int d, double &lo, double &hi) {
  lo = hi = qnan();
  for (int k = 0; k < d; ++k) {
    double t1, t2;
    line_cube_coord(o[k], v[k], t1, t2);
    nan_skip_max(lo, t1);
    nan_skip_min(hi, t2);
  }
}
// one line by one wave: the lane holds coordinates lane + 64 h of the origin and the direction (h < 2; beyond d: ignored);
// every lane gets (lo, hi)
__device__ __forceinline__ void line_cube_wave(const double (&o)[2], const double (&v)[2], int d, int lane, double &lo,
                                               double &hi) {
  lo = hi = qnan();
#pragma unroll
  for (int h = 0; h < 2; ++h)
    if (lane + 64 * h < d) {
      double t1, t2;
      line_cube_coord(o[h], v[h], t1, t2);
      nan_skip_max(lo, t1);
      nan_skip_min(hi, t2);
    }
  for (int off = 32; off > 0; off >>= 1) {
    nan_skip_max(lo, __shfl_xor(lo, off, 64));
    nan_skip_min(hi, __shfl_xor(hi, off, 64));
  }
}

// ---- wave-per-walker helpers: lane = coordinate (d <= 128: two coordinates per lane) ------------------------------------
__device__ __forceinline__ double wave_sum(double v) {
  for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off, 64);
  return v;
}

// Direction of a new slice for walker i (stepfuncs.pyx:348-535), drawn on the device: every lane gets ITS coordinates
// vr[h] = v[lane + 64 h] (0 beyond d).  Philox stream 2, (npairs + 2) blocks per walker: block 0 = integer picks + mixture
// coin, blocks 1.. = Box-Muller pairs (coordinate k takes the cosine / sine branch of pair k / 2).
__device__ inline void dw_direction(const WalkState &w, int i, int lane, int kind, double dirscale, const WalkDirData &dd,
                                    unsigned long long seed, unsigned long long offset, double (&vr)[2]) {
  const int d = w.d;
  const int npairs = (d + 1) / 2;
  const unsigned long long base = offset + (unsigned long long)i * (unsigned long long)(npairs + 2);
  unsigned pick[4];
  philox_block(seed, 2u, base, pick);
  int k = kind;
  if (k == DIR_MIXTURE) k = (u01(pick[2], pick[3]) < 0.5) ? DIR_DIFFERENTIAL : DIR_REGION_ORIENTED;
  vr[0] = vr[1] = 0.0;
  if (k == DIR_CUBE_ORIENTED || k == DIR_CUBE_ORIENTED_SCALED) {
    const int j = (int)below(pick[0], (unsigned)d);
#pragma unroll
    for (int h = 0; h < 2; ++h) {
      const int c = lane + 64 * h;
      if (c < d) vr[h] = c == j ? ((k == DIR_CUBE_ORIENTED) ? dirscale : dirscale * dd.std[j]) : 0.0;
    }
  } else if (k == DIR_REGION_ORIENTED) {
    const int j = (int)below(pick[0], (unsigned)d);
#pragma unroll
    for (int h = 0; h < 2; ++h) {
      const int c = lane + 64 * h;
      if (c < d) vr[h] = dd.axes[(size_t)j * d + c] * dirscale;
    }
  } else if (k == DIR_DIFFERENTIAL) {
    const unsigned a = below(pick[0], (unsigned)dd.nlive);
    unsigned b = below(pick[1], (unsigned)(dd.nlive - 1));
    if (b >= a) ++b;
#pragma unroll
    for (int h = 0; h < 2; ++h) {
      const int c = lane + 64 * h;
      if (c < d) vr[h] = (dd.live[(size_t)a * d + c] - dd.live[(size_t)b * d + c]) * dirscale;
    }
  } else {   // DIR_RANDOM, DIR_REGION_RANDOM: isotropic unit vector of length dirscale
    double g[2] = {0.0, 0.0};
    double part = 0.0;
#pragma unroll
    for (int h = 0; h < 2; ++h) {
      const int c = lane + 64 * h;
      if (c < d) {
        unsigned r4[4];
        philox_block(seed, 2u, base + 1 + (c >> 1), r4);
        const double rad = sqrt(-2.0 * log(u01(r4[0], r4[1])));
        const double ang = 2.0 * M_PI * u01(r4[2], r4[3]);
        g[h] = (c & 1) ? rad * sin(ang) : rad * cos(ang);
        part += g[h] * g[h];
      }
    }
    const double f = dirscale / sqrt(wave_sum(part));
    g[0] *= f;
    g[1] *= f;
    if (k == DIR_RANDOM) {
#pragma unroll
      for (int h = 0; h < 2; ++h)
        if (lane + 64 * h < d) vr[h] = g[h];
    } else {   // v[r] = sum_c axes[r][c] * v1[c]   (einsum 'ij,kj->ki', stepfuncs.pyx:476)
      double acc[2] = {0.0, 0.0};
      for (int c = 0; c < d; ++c) {
        const double v1c = __shfl(c < 64 ? g[0] : g[1], c & 63, 64);
#pragma unroll
        for (int h = 0; h < 2; ++h) {
          const int r = lane + 64 * h;
          if (r < d) acc[h] += dd.axes[(size_t)r * d + c] * v1c;
        }
      }
#pragma unroll
      for (int h = 0; h < 2; ++h)
        if (lane + 64 * h < d) vr[h] = acc[h];
    }
  }
}

// ---- the wide form of dw_direction: kNarrowDirMaxDim < d <= kWideDirMaxDim (the resident slice walkers, mlf_walk.hip) ------
// Same Philox layout, same kinds, one wave per walker; the row goes straight to v (the walker's row of currentv: d doubles in
// global memory) instead of two registers per lane, lane l writing coordinates l, l + 64, ...  Kinds 0, 1, 3, 5 (and both
// branches of 6) are dw_direction's selections, one multiplication, or one subtraction and one multiplication per coordinate:
// the same doubles.  Kinds 2 and 4 stage the d normals in LDS (gs: kWideDirMaxDim doubles of the calling one-wave workgroup;
// lane l draws the Box-Muller PAIRS p = l, l + 64, ... -- one Philox block, one logarithm and one square root per pair -- and
// writes g[2 p], g[2 p + 1]).  SUMMATION ORDERS (no FMA; every wide caller goes through this one function, so the per-step
// route, the graph replay and the memory form of the rounds agree bit for bit):
//   squared norm   lane l adds g[2 p]^2, then g[2 p + 1]^2 (where 2 p + 1 < d), for p = l, l + 64, ... ascending, into one
//                  partial starting at 0; the 64 partials are combined by wave_sum's xor tree (offsets 32, 16, 8, 4, 2, 1).
//                  f = dirscale / sqrt(sum), g[c] <- g[c] * f.
//   kind 4         v[r] = sum_c axes[r][c] * g[c]: lane l adds the products of c = l, l + 64, ... ascending into one partial
//                  starting at 0 (a coalesced read of row r; eight rows in flight); the 64 partials of a row are combined by
//                  the xor tree with offsets 32, 16, 8, 4, 2, 1, at every level own + partner's.  (For offsets 32, 16, 8 the
//                  tree of eight rows is folded -- a lane keeps the half of the rows its bit selects and sends the other --
//                  which changes who holds a sum, not the sum.)
__device__ __forceinline__ void wave_lds_sync() {   // LDS written by some lanes of the wave, read by others
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
  __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

__device__ inline void dw_direction_wide(int d, int i, int lane, int kind, double dirscale, const WalkDirData &dd,
                                         unsigned long long seed, unsigned long long offset, double *v, double *gs) {
  const int npairs = (d + 1) / 2;
  const unsigned long long base = offset + (unsigned long long)i * (unsigned long long)(npairs + 2);
  unsigned pick[4];
  philox_block(seed, 2u, base, pick);
  int k = kind;
  if (k == DIR_MIXTURE) k = (u01(pick[2], pick[3]) < 0.5) ? DIR_DIFFERENTIAL : DIR_REGION_ORIENTED;
  if (k == DIR_CUBE_ORIENTED || k == DIR_CUBE_ORIENTED_SCALED) {
    const int j = (int)below(pick[0], (unsigned)d);
    const double x = (k == DIR_CUBE_ORIENTED) ? dirscale : dirscale * dd.std[j];
    for (int c = lane; c < d; c += 64) v[c] = c == j ? x : 0.0;
  } else if (k == DIR_REGION_ORIENTED) {
    const int j = (int)below(pick[0], (unsigned)d);
    const double *row = dd.axes + (size_t)j * d;
    for (int c = lane; c < d; c += 64) v[c] = row[c] * dirscale;
  } else if (k == DIR_DIFFERENTIAL) {
    const unsigned a = below(pick[0], (unsigned)dd.nlive);
    unsigned b = below(pick[1], (unsigned)(dd.nlive - 1));
    if (b >= a) ++b;
    const double *ra = dd.live + (size_t)a * d, *rb = dd.live + (size_t)b * d;
    for (int c = lane; c < d; c += 64) v[c] = (ra[c] - rb[c]) * dirscale;
  } else {   // DIR_RANDOM, DIR_REGION_RANDOM: isotropic unit vector of length dirscale
    wave_lds_sync();   // (the walker this wave served before has read gs)
    double part = 0.0;
    for (int p = lane; p < npairs; p += 64) {   // (what is written lies below d <= kWideDirMaxDim: inside gs)
      unsigned r4[4];
      philox_block(seed, 2u, base + 1 + p, r4);
      const double rad = sqrt(-2.0 * log(u01(r4[0], r4[1])));
      const double ang = 2.0 * M_PI * u01(r4[2], r4[3]);
      const double g0 = rad * cos(ang), g1 = rad * sin(ang);
      gs[2 * p] = g0;
      part += g0 * g0;
      if (2 * p + 1 < d) {
        gs[2 * p + 1] = g1;
        part += g1 * g1;
      }
    }
    const double f = dirscale / sqrt(wave_sum(part));
    wave_lds_sync();
    if (k == DIR_RANDOM) {
      for (int c = lane; c < d; c += 64) v[c] = gs[c] * f;
    } else {   // v[r] = sum_c axes[r][c] * v1[c]   (einsum 'ij,kj->ki', stepfuncs.pyx:476)
      for (int c = lane; c < d; c += 64) gs[c] = gs[c] * f;   // (the lane that scales an element is the one that reads it below)
      for (int r0 = 0; r0 < d; r0 += 8) {
        double acc[8];
        const double *rows[8];
#pragma unroll
        for (int j = 0; j < 8; ++j) {
          acc[j] = 0.0;
          rows[j] = dd.axes + (size_t)(r0 + j < d ? r0 + j : d - 1) * d;   // past the last row: read it again, never written
        }
        for (int c = lane; c < d; c += 64) {
          const double gc = gs[c];
#pragma unroll
          for (int j = 0; j < 8; ++j) acc[j] += rows[j][c] * gc;
        }
        // offsets 32, 16, 8: the lane keeps rows [0, n) of what it holds where its bit is clear, [n, 2 n) where it is set
#pragma unroll
        for (int level = 0; level < 3; ++level) {
          const int n = 4 >> level, off = 32 >> level;
          const bool upper = (lane & off) != 0;
#pragma unroll
          for (int j = 0; j < n; ++j) {
            const double keep = upper ? acc[j + n] : acc[j];
            const double send = upper ? acc[j] : acc[j + n];
            acc[j] = keep + __shfl_xor(send, off, 64);
          }
        }
        double s = acc[0];
        for (int off = 4; off > 0; off >>= 1) s += __shfl_xor(s, off, 64);
        const int r = r0 + ((lane >> 5) & 1) * 4 + ((lane >> 4) & 1) * 2 + ((lane >> 3) & 1);
        if ((lane & 7) == 0 && r < d) v[r] = s;
      }
    }
  }
}

// one line by one wave, rows in memory of any d (the wide forms of the whole-population samplers): lane l combines the
// coordinates c = l, l + 64, ... of o and v, then line_cube_wave's xor tree; every lane gets (lo, hi).  Max and min are exact,
// so these are the two doubles of line_cube_row.  The rows must be visible to the lanes that read them (wave_lds_sync).
__device__ __forceinline__ void line_cube_wave_wide(const double *o, const double *v, int d, int lane, double &lo, double &hi) {
  lo = hi = qnan();
  for (int c = lane; c < d; c += 64) {
    double t1, t2;
    line_cube_coord(o[c], v[c], t1, t2);
    nan_skip_max(lo, t1);
    nan_skip_min(hi, t2);
  }
  for (int off = 32; off > 0; off >>= 1) {
    nan_skip_max(lo, __shfl_xor(lo, off, 64));
    nan_skip_min(hi, __shfl_xor(hi, off, 64));
  }
}

// ---- a proposal on the line and its built-in prior transform (the whole-population samplers: mlf_rwalk.hip, mlf_sslice.hip)
__device__ __forceinline__ double rwalk_move(double u, double v, double t) {
  const double step = v * t;
  return u + step;
}

__device__ __forceinline__ double rwalk_transform(int tkind, double x, double ta, double tb) {
  double p = x;
  if (tkind == 1) {
    const double m = x * ta;
    p = m + tb;
  } else if (tkind == 2) {
    const double m = x * ta;
    p = m * tb;
  }
  return p;
}

// dw_direction reads only the dimensionality of the state it is given
__device__ __forceinline__ WalkState direction_state(int d) {
  WalkState ws{};
  ws.d = d;
  return ws;
}

// diagnose_move_distances for one walker that moved (wave-wide, lane = whitened coordinate; T rows are read
// coalesced, squared differences summed by a fixed shuffle tree): uo = the point the step started from, un = the
// accepted point
// d <= 64, affine layer: lane k holds coordinate k of the two points (vo: where the step started, vn: the accepted point; 0
// beyond d); returns the squared whitened distance on lane 0.  Both points share every matrix element; the chains read the
// centred coordinates by lane broadcast (same values and order as whiten_point: results are identical)
__device__ __forceinline__ double move_distance_regs(const WalkLayer &ly, int d, int lane, double vo, double vn) {
  if (lane < d) {
    if (ly.wrap && !isnan(ly.wrap[lane])) {
      vo = mlf_wrap_unit(vo, ly.wrap[lane]);
      vn = mlf_wrap_unit(vn, ly.wrap[lane]);
    }
    vo -= ly.ctr[lane];
    vn -= ly.ctr[lane];
  } else {
    vo = vn = 0.0;
  }
  double ta = 0.0, tb = 0.0;
  const int c = lane < d ? lane : 0;
  for (int k = 0; k < d; ++k) {
    const double m = ly.mat[(size_t)k * d + c];
    ta = __builtin_fma(__shfl(vo, k, 64), m, ta);
    tb = __builtin_fma(__shfl(vn, k, 64), m, tb);
  }
  double acc = 0.0;
  if (lane < d) {
    const double diff = ta - tb;
    acc = diff * diff;
  }
  for (int off = 32; off > 0; off >>= 1) acc += __shfl_down(acc, off, 64);
  return acc;
}

// squared whitened distance between two rows in memory, by one wave, on lane 0 (the form dw_move_distance has always taken:
// move_distance_regs where it applies, else the rows' coordinates whitened one by one)
__device__ __forceinline__ double move_distance_rows(const WalkLayer &ly, int d, int lane, const double *uo, const double *un) {
  double acc = 0.0;
  if (ly.kind == 0 && d <= 64) {
    double vo = 0.0, vn = 0.0;
    if (lane < d) {
      vo = uo[lane];
      vn = un[lane];
    }
    acc = move_distance_regs(ly, d, lane, vo, vn);
  } else {
    for (int c = lane; c < d; c += 64) {
      double ta, tb;
      whiten_point(ly, uo, d, c, ta);
      whiten_point(ly, un, d, c, tb);
      const double diff = ta - tb;
      acc += diff * diff;
    }
    for (int off = 32; off > 0; off >>= 1) acc += __shfl_down(acc, off, 64);
  }
  return acc;
}

}  // namespace mlf
