// mlf_wide_filter.hpp -- f16 matrix-core pre-filter of the mask-mode neighbour test above 128 dimensions (see mlf_wide_filter.hip)
#pragma once
#include "mlf_common.hpp"

namespace mlf {

constexpr int kWideFilterMinKs = 10;    // dp = 144: K = 160 columns (up to 9 k-steps: the templated kernels of mlf_filter.hip)
constexpr int kWideFilterMaxKs = 65;    // dp = 1024: K = 1040 columns
constexpr int kWideStatCols = 1024;     // columns of the statistics scratch (= MLF_MAX_DIM)
constexpr int kWideStatBlocks = 64;

struct WideQuantArgs {
  const double *q;       // whitened rows, element (j, k) at q[j*ldq + k]
  long long ldq, nq, nqpad;
  int d_src;             // coordinates present in q
  int d;                 // filter dimensionality (the padded dp; the norm / ones columns sit at d .. d+5)
  int ks;
  const double *stats;   // [0] sigma, [1] namax, [8 + k] centre
  double r2;
  const uint8_t *gate;   // optional: 0 = outside the ellipsoid (route 0, mask 0)
  void *qF;              // [nqpad / 32][ks][64][8] binary16
  float *tlo, *thi;      // [nqpad]
  uint8_t *route;        // [nq] 0 gated out / 1 filtered / 2 exact scan / 3 certain miss by the norm test
  uint8_t *out_mask;     // route 0 and 3 rows are answered here
  unsigned *band_count;  // statistics word, zeroed here, counted up by the sweep
  int *qlist;            // [nq] the route-2 proposals, in any order: what the exact tail scans
  unsigned *qcount;      // their number; zero on entry (cleared in front of the batch)
};

struct WideSweepArgs {
  const void *refF;      // [ntiles32][ks][64][8] binary16
  int ntiles32, ks;
  const void *qF;
  const float *tlo, *thi;
  long long ngroups, nq;
  uint8_t *route;        // a query whose minimum ends in the band: 1 -> 2
  uint8_t *out_mask;     // every other filtered query is answered here
  unsigned *band_count;
  int *qlist;            // the list the quantising kernel started
  unsigned *qcount;
};

inline size_t wide_stat_scratch_bytes() { return ((size_t)kWideStatBlocks * kWideStatCols + 2) * sizeof(double); }
// stats: 8 + kWideStatCols doubles; scratch: wide_stat_scratch_bytes(), zero-initialised once (the last two words are running
// maxima, reset by the launch)
void launch_wide_ref_stats(const double *refR, int n, int dp, double *stats, double *scratch, hipStream_t s);
void launch_wide_quant_refs(const double *refR, int n, int npad32, int dp, int ks, const double *stats, void *refF, hipStream_t s);
hipError_t launch_wide_quant_queries(const WideQuantArgs &a, hipStream_t s);
// query groups of 32 a sweep workgroup stages in LDS
int wide_sweep_groups(int ks, long long ngroups);
hipError_t launch_wide_sweep(const WideSweepArgs &a, hipStream_t s);
// mlf_wide.hip: k_scan_wide in mask mode over the *qcount queries listed in qlist (a.nq = the batch size)
hipError_t launch_scan_wide_list(int dp, const ScanArgs &a, const int *qlist, const unsigned *qcount, hipStream_t s);

}  // namespace mlf
