// mlf_rwalk.hpp -- PopulationRandomWalkSampler's refill on the device (mlf_rwalk.hip; reference
// ultranest/popstepsampler.py:192-358): P independent walkers, each nsteps times direction -> cube-line intersection ->
// truncated-normal step -> transform -> likelihood -> accept.  No chain is kept: a walker is its current (u, p, L).
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

#include "mlf_walk.hpp"

namespace mlf {

struct RwalkState {
  int P, nsteps, d;
  double *u, *p;           // [P][d]  current point and its transform (p: NaN until the walker's first accepted move)
  double *L;               // [P]
  long long *start;        // [P]     live row the walker started from
  uint8_t *ever, *last;    // [P]     accepted some move / accepted the last move
  int *rej;                // [P]     rejected moves
  double *tl, *tr;         // [P]     cube limits of the last step's line
  double *dist2;           // [P]     whitened distance^2 start row -> final point of the walkers with `last`, else NaN
  // chain form: one step's proposals
  double *unew, *pnew;     // [P][d]
  double *Lnew;            // [P]
  uint8_t *inside;         // [P]     the proposal lies strictly inside the unit cube
};

struct RwalkArgs {
  RwalkState w;
  const double *live, *Ls;   // device copy of the live points and their likelihoods
  int nlive;
  int dirkind;
  double dirscale;
  WalkDirData dd;
  int tkind;                 // built-in transform 0 identity, 1 x*a + b, 2 (x*a)*b; -1: a user model evaluates the proposals
  double ta, tb;
  int lkind;
  const double *aux;
  double sigma;
  WalkLayer ly;
  double Lmin;
  unsigned long long seed, offset;
  double *parts;             // [chunks of 1024 walkers][5]
  double *out;               // [0] rejected moves, [1] walkers with `last`, [2] far-enough moves, [3] sum log(dist / radius + 1e-10),
                             // [4] walkers that never moved
};
constexpr int kRwalkOut = 5;

// Philox counters one refill consumes past `offset` (stream 2: P * nsteps direction draws of (npairs + 2) blocks; stream 7:
// P * (nsteps + 1) blocks, fewer)
unsigned long long rwalk_philox_per_refill(int P, int nsteps, int d);
// the fused form (launch_rwalk_fused) covers this shape
bool rwalk_fused_covers(int d, int layer_kind);

void launch_rwalk_start(const RwalkArgs &a, hipStream_t s);
// chain form: step `step` of every walker up to the cube flag (and the built-in transform); then the evaluation into
// w.pnew / w.Lnew by the caller (Lnew of a row whose flag is 0 may hold anything); then the accept, which tests the flag first
void launch_rwalk_propose(const RwalkArgs &a, int step, hipStream_t s);
void launch_rwalk_accept(const RwalkArgs &a, hipStream_t s);
// fused form: start and all nsteps in one launch (built-in models)
void launch_rwalk_fused(const RwalkArgs &a, hipStream_t s);
// both forms: move diagnostics and counts into a.out
void launch_rwalk_finish(const RwalkArgs &a, hipStream_t s);

}  // namespace mlf
