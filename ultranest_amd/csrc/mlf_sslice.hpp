// mlf_sslice.hpp -- PopulationSimpleSliceSampler's refill on the device (mlf_sslice.hip; reference
// ultranest/popstepsampler.py:907-1002, stepfuncs.pyx:537-630): P points, each nsteps slice steps without stepping out.
// A step shrinks every point's slice until the point has a successor; P workers (likelihood slots) evaluate per iteration,
// the workers of finished points are dealt to the unfinished ones.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

#include "mlf_walk.hpp"

namespace mlf {

// what a slot (propose, evaluation, update, deal) does: read by every kernel of the slot, written by k_sslice_deal alone
struct SsliceCtl {
  int step, it;                    // the step and the iteration within it the next slot serves
  int nz;                          // unfinished points (it > 0: the length of zlist)
  int finished;                    // all nsteps are done: every later slot exits at this load
  long long total_it;              // iterations so far
  unsigned long long discarded;    // proposals above the threshold that lay outside their point's slice
};

struct SsliceState {
  int P, nsteps, d, max_it;
  double *u, *p;           // [P][d]  current point and its transform (p: NaN until the point's first successor)
  double *L;               // [P]
  long long *start;        // [P]     live row the point started from
  double *v;               // [P][d]  the step's direction of every point
  double *tl, *tr;         // [P]     slice bounds of every point
  uint8_t *status;         // [P]     1: the point has its successor in this step
  int *zlist;              // [P]     unfinished points in ascending order; worker j serves zlist[j % nz] (it == 0: point j)
  int *taken, *taken_it;   // [P]     worker and iteration whose proposal became the point's successor in the last step (-1: none)
  // one iteration's proposals, per worker
  double *t;               // [P]
  double *unew, *pnew;     // [P][d]
  double *Lnew;            // [P]
  uint8_t *member;         // [P]     user models: the evaluation's member mask (all ones; zeros once finished)
  double *widths;          // [nsteps][P]  tr - tl at the end of every step
  int *iters;              // [nsteps]     iterations of every step
  double *dist2;           // [P]     whitened distance^2 start row -> final point (NaN without a layer)
  uint8_t *nanrow;         // [P]     the p row holds a non-finite value
  SsliceCtl *ctl;
};

struct SsliceArgs {
  SsliceState w;
  const double *live, *Ls;   // device copy of the live points and their likelihoods
  int nlive;
  int dirkind;
  const double *dirscale;    // [nsteps]  length of the step's directions (scale * jitter, computed in binary64 on the host)
  WalkDirData dd;
  int limit;                 // slice limits: 0 the line's part inside the unit cube, 1 that clipped to [-1, 1]
  double shrink;
  int tkind;                 // built-in transform 0 identity, 1 x*a + b, 2 (x*a)*b; -1: a user model evaluates the proposals
  double ta, tb;
  WalkLayer ly;
  double Lmin;
  unsigned long long seed, offset;
  double *out;               // [0] moves farther than the radius, [1] sum log(dist / radius + 1e-10), [2] points with a non-finite p row
};
constexpr int kSsliceOut = 3;

// Philox counters one refill consumes past `offset`: max(stream 2: P * nsteps * (npairs + 2), stream 8: P * (1 + nsteps * max_it))
unsigned long long sslice_philox_per_refill(int P, int nsteps, int d, int max_it);

void launch_sslice_start(const SsliceArgs &a, hipStream_t s);
// One slot is launch_sslice_propose, the evaluation of w.unew / w.pnew into w.Lnew (w.member: the user model's mask) by the
// caller, launch_sslice_update, launch_sslice_deal.  Which step and iteration the slot serves is read from w.ctl.
void launch_sslice_propose(const SsliceArgs &a, hipStream_t s);
void launch_sslice_update(const SsliceArgs &a, hipStream_t s);
void launch_sslice_deal(const SsliceArgs &a, hipStream_t s);
// move diagnostics and counts into a.out
void launch_sslice_finish(const SsliceArgs &a, hipStream_t s);

}  // namespace mlf
