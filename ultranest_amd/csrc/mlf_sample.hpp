// mlf_sample.hpp -- device-side proposal generation + compaction (mlf_sample.hip)
#pragma once
#include "mlf_common.hpp"

namespace mlf {

void launch_philox_words(unsigned long long seed, unsigned stream, long long n, unsigned *out, hipStream_t s);
hipError_t launch_generate_cube(double *pts, long long nelem, unsigned long long seed, unsigned long long offset,
                                hipStream_t s);
hipError_t launch_generate_ball(double *z, long long n, int d, double enlarge, unsigned long long seed,
                                unsigned long long offset, hipStream_t s);
// sample_from_wrapping_ellipsoid in one launch: w = centre + (ball draw) . A, in_cube[p] = all coordinates strictly inside (0, 1).
// A_padded: the axes matrix (element (j, k) = axes_T[j][k]) as [d][4 generate_ellipsoid_chunk(d)] doubles, zero padded.  d <= 128.
int generate_ellipsoid_chunk(int d);
hipError_t launch_generate_ellipsoid(double *w, long long n, int d, double enlarge, const double *A_padded, const double *center,
                                     uint8_t *in_cube, unsigned long long seed, unsigned long long offset, hipStream_t s);
// AffineLayer.untransform of whole batches: w = t . M + ctr (M padded like A_padded above), circular axes rotated back where
// wrap_shift (NaN = not circular) is given, in_cube[p] = all coordinates strictly inside (0, 1).  d <= 128.
hipError_t launch_rows_affine(const double *t, long long n, int d, const double *M_padded, const double *ctr, const double *wrap_shift,
                              double *w, uint8_t *in_cube, hipStream_t s);
void launch_center_and_cube(double *w, long long n, int d, const double *center, uint8_t *in_cube, hipStream_t s);
hipError_t launch_generate_tbox(double *t, long long n, int d, const double *lo, const double *hi, double pad,
                                unsigned long long seed, unsigned long long offset, hipStream_t s);
// method 3: rows whose 64-row staging fits the device's per-workgroup LDS go through k_generate_around_points, wider ones through
// k_generate_around_points_wide -- the same draws, bit for bit.  force_around_points_wide (tests): every row through the latter.
hipError_t launch_generate_around_points(double *t, double *thin_u, long long n, int d, const double *refR, int nlive, int dp,
                                         double r2, unsigned long long seed, unsigned long long offset, hipStream_t s);
void force_around_points_wide(bool on);
void launch_thin_by_multiplicity(const long long *count, const double *thin_u, long long n, uint8_t *mask, hipStream_t s);
void launch_untransform_rows(const double *t, long long n, int d, const double *invT, const double *ctr,
                             const double *wrap_shift, double *w, uint8_t *in_cube, hipStream_t s);
void launch_elementwise_affine(const double *x, long long n, int tkind, double a, double b, double *out, hipStream_t s);
// The elementwise prior transform of launch_elementwise_affine and the parameter-space wrapping ellipsoid (mlf_tregion_dev.hpp) in
// one pass over n rows of d doubles: p = transform(u) is written for the rows with member[i] != 0 (member == nullptr: all; nothing
// for tkind 0, where the rows are the parameters and p may be null) and member2[i] = member[i] && inside(p_i) for every row.
// A: dense d x d, ctr, fixed_val: d doubles (NaN = variable dimension), all on the device.
struct TransformGateArgs {
  const double *u;
  long long n;
  int d;
  const uint8_t *member;
  int tkind;
  double ta, tb;
  double *p;
  const double *A, *ctr, *fixed_val;
  double enlarge;
  uint8_t *member2;
};
hipError_t launch_transform_gate(const TransformGateArgs &a, hipStream_t s);
// mask[e] = v[e] > threshold (&& also[e] where `also` is given)
void launch_mask_greater(const double *v, long long n, double threshold, uint8_t *mask, hipStream_t s, const uint8_t *also = nullptr);
void launch_mask_and(uint8_t *mask, const uint8_t *other, long long n, hipStream_t s);
void launch_apply_pregate(const uint8_t *pregate, long long n, uint8_t *gate, uint8_t *route, float *tlo,
                          float *thi, hipStream_t s);
void launch_scan_counts(unsigned *blk, int nblk, hipStream_t s);
// Stream compaction of the rows one mask selects, for any number of arrays of the same n rows (n > 0).  The constructor enqueues
// the offsets of the mask into blk (ceil(n / 256) + 1 counters); scatter() copies the selected rows of one array, in order, the
// first `capacity` of them; count() reads the total back with one synchronisation and returns min(total, capacity).  Either
// order works: scatter, then count; or count, then scatter into buffers sized by it.
struct Compaction {
  Compaction(const uint8_t *mask, long long n, unsigned *blk, hipStream_t s);
  void scatter(const double *src, int d, double *dst, size_t capacity) const;   // rows of d doubles; d = 1: scalars
  hipError_t count(size_t capacity, size_t *taken) const;
  const uint8_t *mask;
  long long n;
  unsigned *blk;
  hipStream_t s;
};

}  // namespace mlf
