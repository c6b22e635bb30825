// mlf_user_rows.hpp -- the one kernel the library launches around a user model (ultranest_amd/devicemodel.py,
// mlf_user.hip).  hiprtc compiles this header with the user's source in front of it; that source defines
//
//   __device__ double mlf_user_loglike(const double *p, int d, const double *aux, long long naux);          // required
//   __device__ void mlf_user_transform(const double *u, double *p, int d, const double *aux, long long naux);  // optional
//
// (the transform is compiled in when MLF_USER_HAS_TRANSFORM is 1; otherwise p = u).  The library itself includes the
// header with MLF_USER_ROWS_HOST defined to share the choice of form and its LDS size (mlf_user_rows_lds_bytes).
//
// mlf_user_rows(u, n, d, member, aux, naux, p, L): rows are d doubles, row-major, one thread per row.
//   member (nullable)  only rows with member[i] != 0 are evaluated; the others get L[i] = -inf and their p row is not written
//   p      (nullable)  NULL: the rows ARE the parameters (no transform; the likelihood reads u)
//                      else: p = transform(u) (a copy of u without a transform), the likelihood reads p
//   L      (nullable)  NULL: transform only
// u and p must not overlap.
//
// Two forms, chosen from d alone:
//   staged  one wave per workgroup copies its 64 rows (one contiguous block of the batch) into LDS with coalesced loads, at
//           a row pitch of d + 1 doubles (lane = row reads are then conflict-free), runs transform and likelihood from LDS
//           and writes p back through LDS with coalesced stores (the k_loglike scheme of mlf_misc.hip, with a second buffer
//           for p).  LDS per wave: nbuf * 64 * (d + 1) * 8 bytes, nbuf = 2 with a transform writing p, else 1.
//   direct  one thread per row straight from global memory (k_loglike_wide), where the staging would exceed
//           kUserRowsLdsBudget = 64 KiB per wave: d >= 64 with a transform, d >= 128 without.  64 KiB still lets two
//           such waves share a CU's 160 KiB of LDS; above it one wave per CU would be left, with nothing to hide its
//           load latency behind.
//
// Gated form (MLF_USER_TREGION=1, its own code object): the driver's parameter-space wrapping ellipsoid between transform
// and likelihood (mlf_tregion_dev.hpp; mlf_region_set_tregion).  After transform_row has written the p row the lane
// tests it, calls the likelihood only if it passes and writes member2[i] = member[i] && inside(p_i); the kernel is named
// mlf_user_rows_tregion and takes (tr_A, tr_ctr, tr_fixed, tr_enlarge, member2) behind its other parameters.  Matrix, centre and fixed values are read
// through wave-uniform addresses: no extra LDS, the same choice of form.
//
// Summed form (MLF_USER_SUM=1, its own code objects: mlf_user_rows_sum and, with MLF_USER_TREGION=1,
// mlf_user_rows_sum_tregion; they are the only kernel of their program).  The user's source defines, instead of mlf_user_loglike,
//
//   __device__ double mlf_user_loglike_term(const double *p, int d, const double *aux, long long naux, long long k);
//
// and L(p) = sum over k in [0, nterms) of term(k).  The kernels take the eight parameters above, then `long long nterms`, then
// the gate's five in the gated entry (9 and 14).  ONE WAVE OWNS ONE ROW (one wave per workgroup, blockIdx.x = row: every
// barrier is wave-local and the wave of a row outside the mask leaves at once, having written L = -inf (and member2 = 0) from
// lane 0 and read nothing but its member byte).  The wave copies the u row into LDS with coalesced loads; lane 0 alone runs
// mlf_user_transform from that row into a second LDS row (O(d) work on one lane: accepted, the terms are where the time goes)
// and, in the gated entry, mlf_tregion_inside on the p row (the function and arithmetic of the gated default kernel), whose
// result is made wave-uniform; all lanes read the p row back from LDS.  The p row of every member row leaves LDS with coalesced
// stores, whether or not it passes the gate.  Inside the term function p points into LDS and k differs from lane to lane, so
// aux[... k ...] is read by neighbouring lanes at neighbouring addresses.
//
// The order of the sum is part of the interface (compiled with -ffp-contract=off like everything here):
//   per lane      lane l (0..63) starts from s_l = 0.0 and adds term(k) for k = l, l + 64, l + 128, ... < nterms, ascending,
//                 one plain addition each;
//   across lanes  six exchange steps with lane distances 32, 16, 8, 4, 2, 1 in that order, each setting every lane to
//                 s_l + s_(l xor m) (__shfl_xor on the double);
//   result        IEEE addition commutes, so after the six steps all lanes hold the same bits: L is that value.
// L therefore does not depend on the row's place in the batch, the batch size, the mask or the route; a NaN term gives NaN,
// -inf terms give -inf.  LDS per wave: (p buffer ? 2 : 1) * d * 8 bytes (mlf_user_rows_sum_lds_bytes; at most 16 KiB at
// MLF_MAX_DIM = 1024, so there is no direct form and no threshold in d).
//
// Several sums and a final function (MLF_USER_SUM=1 with MLF_USER_NSUMS=M, 1 <= M <= 8, a compile-time constant; its own code
// objects: mlf_user_rows_sums and, with MLF_USER_TREGION=1, mlf_user_rows_sums_tregion, with the parameter lists of the summed
// entries, 9 and 14).  The user's source defines, instead of mlf_user_loglike_term,
//
//   __device__ void mlf_user_loglike_terms(const double *p, int d, const double *aux, long long naux, long long k, double *t);
//   __device__ double mlf_user_loglike_finish(const double *s, int nsums, const double *p, int d, const double *aux, long long naux);
//
// terms writes all M entries t[0..M) for data index k (t is not pre-set: an entry left unwritten is undefined); finish receives
// the M sums s_j = sum over k of t_j(k), the row's p and the data, and returns L.  M = 1 is a function of one sum; per-row
// constants go into term 0 or into finish.  Everything but the sum itself is the summed kernel above, unchanged (and without
// MLF_USER_NSUMS the summed entries are the programs they were).  The order contract, extended:
//   each sum      accumulator j follows, independently of the others, exactly the order of the single-sum form: lane l starts
//                 from s_j = 0.0 and adds t_j(k) for k = l, l + 64, ... < nterms, ascending, one plain addition each; then the
//                 six exchange steps 32, 16, 8, 4, 2, 1, each setting every lane's s_j to s_j + s_j(l xor m);
//   no term       a lane without a term (nterms < 64) never calls terms; its accumulators stay 0.0;
//   finish        after the exchange all lanes hold the same M values; every lane calls finish with them (it must be a pure
//                 function of its arguments) and lane 0's result is L;
//   not called    a row outside the membership mask, or one that fails the t-region gate, calls neither function: L = -inf.
// A NaN term of accumulator j reaches finish as NaN in s[j] only.  The accumulators and t live in registers (M is a constant and
// every loop over j is unrolled).
//
// Derived parameters (MLF_USER_DERIVED=1, its own code object with mlf_user_derive_rows as its only kernel; compiled from the
// model's source followed by the derived source, so the model's helper functions are visible; nothing of this header refers to
// mlf_user_loglike* or mlf_user_transform in this mode).  The derived source defines
//
//   __device__ void mlf_user_derived(const double *p, int d, double *q, int nq, const double *aux, long long naux);
//
// which writes all of q[0..nq) from the row's p (the d transformed parameters); a pure function of its arguments.
//
// mlf_user_derive_rows(p, n, d, nq, aux, naux, out): p holds n rows of d doubles, out n rows of d + nq doubles,
// out_i = [p_i | q_i]; p and out must not overlap.  No membership mask: the kernel runs on compacted rows, after a route has
// finished with them (no route's own rows change their width).  Rows beyond n are neither read nor written.  Two forms, chosen
// from d and nq (mlf_user_rows_derive_lds_bytes):
//   staged  one wave per workgroup copies its 64 rows of p into LDS (stage_in, pitch d + 1), each lane runs mlf_user_derived from
//           its LDS row into a second LDS area of pitch nq + 1 (lane = row accesses conflict-free in both), and the [p | q] rows
//           leave with coalesced stores of (d + nq)-wide rows.  LDS per wave: 64 * (d + 1 + nq + 1) * 8 bytes.
//   direct  one thread per row from and to global memory, where the staging would exceed MLF_USER_ROWS_LDS_BUDGET
//           (d + nq >= 127).
//
// Gate over derived parameters (MLF_USER_TREGION=1 with MLF_USER_GATE_DERIVED=1, its own code objects, compiled like the derive
// program from the model's source followed by the derived source: mlf_user_rows_tregion_derived, and with MLF_USER_SUM=1
// mlf_user_rows_sum_tregion_derived / mlf_user_rows_sums_tregion_derived, each the only kernel of its program).  The driver's
// t-region spans all w = d + nq columns of a model with derived parameters, so the gate needs q BEFORE the likelihood.  The entries
// take the parameter list of their gated sibling, then `int nq, double *q_scratch`; tr_A is w x w, tr_ctr and tr_fixed hold w
// values.  Per member row: transform_row writes the d-wide p row, mlf_user_derived(p, d, q, nq, aux, naux) writes q, the gate runs
// over [p | q] (mlf_tregion_inside_split: the arithmetic of mlf_tregion_inside through an accessor, the two pieces are not copied
// together), the likelihood is called on the d-wide p row only if the gate passes, member2[i] as in the gated kernels.  THE COST:
// mlf_user_derived runs on every member row of the batch, not only on the rows that are kept.  p leaves at pitch d; q serves
// the gate alone and is not written out (the derive program extends the kept rows afterwards, as without a t-region).
//   default form, staged  the u, p and q rows of the wave's 64 rows in LDS at pitches d | 1, d | 1 and nq | 1 doubles: an ODD
//           pitch P puts lane l's 8-byte word on banks 2 P l mod 64, distinct over each 32-lane half, for every d (the d + 1 of
//           the forms above is odd only for even d).  LDS per wave: 64 * ((p buffer ? 2 : 1) * (d | 1) + (nq | 1)) * 8 bytes
//           (mlf_user_rows_gate_derived_lds_bytes), within MLF_USER_ROWS_LDS_BUDGET; q_scratch is not touched.
//   default form, direct  one thread per row from global memory where that exceeds the budget; q in q_scratch (n rows of nq
//           doubles, the caller's).
//   summed forms  lane 0 runs transform, derived function and gate; q sits in LDS behind the p row (nq more doubles:
//           mlf_user_rows_sum_gate_derived_lds_bytes); the verdict is made wave-uniform as in the gated entries; q_scratch is
//           not touched.  The order contract of the sums is untouched.
#pragma once

#define MLF_USER_ROWS_LDS_BUDGET 65536

// bytes of dynamic LDS the launch needs (0: the direct form).  has_p_buffer: a transform writes p (second buffer).
__host__ __device__ inline unsigned mlf_user_rows_lds_bytes(int d, bool has_p_buffer) {
  const unsigned long long bytes = (unsigned long long)(has_p_buffer ? 2 : 1) * 64ull * (unsigned long long)(d + 1) * 8ull;
  return bytes <= MLF_USER_ROWS_LDS_BUDGET ? (unsigned)bytes : 0u;
}

// bytes of dynamic LDS a launch of the summed form needs: the u row, and the p row where a transform writes one
__host__ __device__ inline unsigned mlf_user_rows_sum_lds_bytes(int d, bool has_p_buffer) {
  return (unsigned)((has_p_buffer ? 2u : 1u) * (unsigned)d * 8u);
}

// bytes of dynamic LDS a launch of mlf_user_derive_rows needs (0: the direct form): 64 p rows of pitch d + 1 and 64 q rows of
// pitch nq + 1
__host__ __device__ inline unsigned mlf_user_rows_derive_lds_bytes(int d, int nq) {
  const unsigned long long bytes = 64ull * (unsigned long long)(d + 1 + nq + 1) * 8ull;
  return bytes <= MLF_USER_ROWS_LDS_BUDGET ? (unsigned)bytes : 0u;
}

// bytes of dynamic LDS a launch of mlf_user_rows_tregion_derived needs (0: the direct form): 64 u rows and, where a transform
// writes p, 64 p rows of pitch d | 1, and 64 q rows of pitch nq | 1
__host__ __device__ inline unsigned mlf_user_rows_gate_derived_lds_bytes(int d, int nq, bool has_p_buffer) {
  const unsigned long long bytes =
      64ull * ((has_p_buffer ? 2ull : 1ull) * (unsigned long long)(d | 1) + (unsigned long long)(nq | 1)) * 8ull;
  return bytes <= MLF_USER_ROWS_LDS_BUDGET ? (unsigned)bytes : 0u;
}

// bytes of dynamic LDS a launch of the summed gate-derived entries needs: the rows of the summed form and the q row behind them
__host__ __device__ inline unsigned mlf_user_rows_sum_gate_derived_lds_bytes(int d, int nq, bool has_p_buffer) {
  return mlf_user_rows_sum_lds_bytes(d, has_p_buffer) + (unsigned)nq * 8u;
}

#ifndef MLF_USER_ROWS_HOST

#ifndef MLF_USER_HAS_TRANSFORM
#define MLF_USER_HAS_TRANSFORM 0
#endif
#ifndef MLF_USER_TREGION
#define MLF_USER_TREGION 0
#endif
#ifndef MLF_USER_SUM
#define MLF_USER_SUM 0
#endif
#ifndef MLF_USER_DERIVED
#define MLF_USER_DERIVED 0
#endif
#ifndef MLF_USER_GATE_DERIVED
#define MLF_USER_GATE_DERIVED 0
#endif
#if MLF_USER_GATE_DERIVED && (!MLF_USER_TREGION || MLF_USER_DERIVED)
#error "MLF_USER_GATE_DERIVED is a mode of the gated programs (MLF_USER_TREGION=1), not of the derive program"
#endif
#if MLF_USER_GATE_DERIVED
#define MLF_TREGION_SPLIT_ROW
#endif
// The two optional tails of an entry's parameter list, the gate's five and behind them the q pair of a gate over derived
// parameters, and the entry's name.  Entries that differ in their parameter lists differ in their names: a code object loaded
// as another variant has no such entry (mlf_usermodel_create_variant) instead of a launch with the wrong arguments
#if MLF_USER_TREGION
#include "mlf_tregion_dev.hpp"
#define MLF_USER_GATE_PARAMS                                                                                                  \
  , const double *__restrict__ tr_A, const double *__restrict__ tr_ctr, const double *__restrict__ tr_fixed, double tr_enlarge, \
      unsigned char *member2
#define MLF_USER_GATE_ARGS , tr_A, tr_ctr, tr_fixed, tr_enlarge, member2
#else
#define MLF_USER_GATE_PARAMS
#define MLF_USER_GATE_ARGS
#endif
#if MLF_USER_GATE_DERIVED
#define MLF_USER_Q_PARAMS , int nq, double *q_scratch
#define MLF_USER_ENTRY(base) base##_tregion_derived
#else
#define MLF_USER_Q_PARAMS
#if MLF_USER_TREGION
#define MLF_USER_ENTRY(base) base##_tregion
#else
#define MLF_USER_ENTRY(base) base
#endif
#endif

namespace mlf_user_detail {

// loads in flight per lane while staging (32 VGPRs)
constexpr int kLoads = 16;

__device__ inline double neg_inf() { return -__builtin_inf(); }

// rows of one wave: global block [0, total) -> LDS rows of pitch ds >= d.  Element e = row * d + col; (row, col) of the lane's
// next element is stepped by 64 elements at a time (no integer division per element).
__device__ inline void stage_in(const double *src, int total, int d, int ds, double *lds, int lane) {
  const int qstep = 64 / d, rstep = 64 % d;
  int row = lane / d, col = lane % d;
  for (int e0 = 0; e0 < total; e0 += 64 * kLoads) {
    double v[kLoads];
#pragma unroll
    for (int i = 0; i < kLoads; ++i) {
      const int e = e0 + 64 * i + lane;
      v[i] = e < total ? src[e] : 0.0;
    }
#pragma unroll
    for (int i = 0; i < kLoads; ++i) {
      const int e = e0 + 64 * i + lane;
      if (e < total) lds[row * ds + col] = v[i];
      row += qstep;
      col += rstep;
      if (col >= d) {
        col -= d;
        row += 1;
      }
    }
  }
}

// LDS rows of pitch ds >= d -> global block [0, total); only the rows whose bit is set in `rows` are written
__device__ inline void stage_out(double *dst, int total, int d, int ds, const double *lds, unsigned long long rows, int lane) {
  const int qstep = 64 / d, rstep = 64 % d;
  int row = lane / d, col = lane % d;
  for (int e = lane; e < total; e += 64) {
    if ((rows >> row) & 1ull) dst[e] = lds[row * ds + col];
    row += qstep;
    col += rstep;
    if (col >= d) {
      col -= d;
      row += 1;
    }
  }
}

__device__ inline void transform_row(const double *x, double *y, int d, const double *aux, long long naux) {
#if MLF_USER_HAS_TRANSFORM
  mlf_user_transform(x, y, d, aux, naux);
#else
  (void)aux;
  (void)naux;
  for (int k = 0; k < d; ++k) y[k] = x[k];
#endif
}

// the gate of a row whose p is ready (x): true without a gate; over derived parameters q = mlf_user_derived(p) first, then the
// t-region test over [p | q] (q, nq: read in that mode alone)
__device__ inline bool gate_row(const double *x, int d, double *q, int nq, const double *aux, long long naux MLF_USER_GATE_PARAMS) {
#if MLF_USER_GATE_DERIVED
  mlf_user_derived(x, d, q, nq, aux, naux);
  return mlf_tregion_inside_split(x, d, q, nq, tr_A, tr_ctr, tr_fixed, tr_enlarge);
#elif MLF_USER_TREGION
  return mlf_tregion_inside(x, d, tr_A, tr_ctr, tr_fixed, tr_enlarge);
#else
  return true;
#endif
}

}  // namespace mlf_user_detail

#if MLF_USER_DERIVED

extern "C" __global__ __launch_bounds__(64) void mlf_user_derive_rows(const double *__restrict__ p, long long n, int d, int nq,
                                                                 const double *aux, long long naux, double *__restrict__ out) {
  using namespace mlf_user_detail;
  const int lane = threadIdx.x;
  const long long j0 = (long long)blockIdx.x * 64;
  if (j0 >= n) return;
  const long long left = n - j0;
  const int nrows = left >= 64 ? 64 : (int)left;
  const int w = d + nq;   // an output row: [p | q]
  if (mlf_user_rows_derive_lds_bytes(d, nq) != 0) {
    extern __shared__ __attribute__((aligned(16))) double mlf_user_lds[];
    const int ds = d + 1, qs = nq + 1;
    double *a = mlf_user_lds;        // 64 rows of p
    double *b = a + 64 * ds;         // 64 rows of q
    stage_in(p + j0 * d, nrows * d, d, ds, a, lane);
    __syncthreads();
    if (lane < nrows) mlf_user_derived(a + lane * ds, d, b + lane * qs, nq, aux, naux);
    __syncthreads();
    // element e = row * w + col of the wave's output block, stepped by 64 elements at a time as in stage_out
    double *dst = out + j0 * w;
    const int total = nrows * w;
    const int qstep = 64 / w, rstep = 64 % w;
    int row = lane / w, col = lane % w;
    for (int e = lane; e < total; e += 64) {
      dst[e] = col < d ? a[row * ds + col] : b[row * qs + (col - d)];
      row += qstep;
      col += rstep;
      if (col >= w) {
        col -= w;
        row += 1;
      }
    }
  } else if (lane < nrows) {
    const double *x = p + (j0 + lane) * d;
    double *y = out + (j0 + lane) * w;
    for (int k = 0; k < d; ++k) y[k] = x[k];
    mlf_user_derived(x, d, y + d, nq, aux, naux);
  }
}

#elif !MLF_USER_SUM

namespace mlf_user_detail {

// the step of a thread-per-row entry whose p row is ready (x): (derived q ->) gate -> the likelihood if the row passes and L is
// asked for, else -inf
__device__ inline double evaluate_row(const double *x, int d, double *q, int nq, const double *aux, long long naux, bool want_L,
                                      bool &pass MLF_USER_GATE_PARAMS) {
  pass = gate_row(x, d, q, nq, aux, naux MLF_USER_GATE_ARGS);
  return want_L && pass ? mlf_user_loglike(x, d, aux, naux) : neg_inf();
}

}  // namespace mlf_user_detail

// the thread-per-row entries: mlf_user_rows, mlf_user_rows_tregion and mlf_user_rows_tregion_derived
extern "C" __global__ __launch_bounds__(64) void MLF_USER_ENTRY(mlf_user_rows)(
    const double *u, long long n, int d, const unsigned char *member, const double *aux, long long naux, double *p,
    double *L MLF_USER_GATE_PARAMS MLF_USER_Q_PARAMS) {
  using namespace mlf_user_detail;
  const int lane = threadIdx.x;
  const long long j0 = (long long)blockIdx.x * 64;
  if (j0 >= n) return;
  const long long left = n - j0;
  const int nrows = left >= 64 ? 64 : (int)left;
  const long long i = j0 + lane;
  const bool mine = lane < nrows && (member == nullptr || member[i] != 0);
  const unsigned long long live = __ballot(mine);
  if (live == 0) {   // no member row in this block: nothing is read
    if (L != nullptr && lane < nrows) L[i] = neg_inf();
#if MLF_USER_TREGION
    if (lane < nrows) member2[i] = 0;
#endif
    return;
  }
  const bool p_buffer = p != nullptr && MLF_USER_HAS_TRANSFORM;
  // what the gate over derived parameters adds to the gated form: odd pitches (lane = row accesses without bank conflicts for
  // every d) and a q row per lane, in LDS behind the p rows or, on the direct form, in q_scratch (without it q is a pointer that
  // gate_row never reads)
#if MLF_USER_GATE_DERIVED
  const int ds = d | 1, qs = nq | 1;
  const unsigned staged = mlf_user_rows_gate_derived_lds_bytes(d, nq, p_buffer);
#else
  const int ds = d + 1, qs = 0, nq = 0;
  double *const q_scratch = nullptr;
  const unsigned staged = mlf_user_rows_lds_bytes(d, p_buffer);
#endif
  double like = neg_inf();
  bool pass = false;
  if (staged != 0) {
    extern __shared__ __attribute__((aligned(16))) double mlf_user_lds[];
    double *a = mlf_user_lds;                       // 64 rows of u
    double *b = p_buffer ? a + 64 * ds : a;         // 64 rows of p (the u rows themselves without a transform)
    double *c = b + 64 * ds;                        // 64 rows of q
    stage_in(u + j0 * d, nrows * d, d, ds, a, lane);
    __syncthreads();
    if (mine) {
      const double *x = a + lane * ds;
      if (p_buffer) {
        double *y = b + lane * ds;
        transform_row(x, y, d, aux, naux);
        x = y;
      }
      like = evaluate_row(x, d, c + lane * qs, nq, aux, naux, L != nullptr, pass MLF_USER_GATE_ARGS);
    }
    __syncthreads();
    if (p != nullptr) stage_out(p + j0 * d, nrows * d, d, ds, b, live, lane);
  } else if (mine) {
    const double *x = u + i * d;
    if (p != nullptr) {
      double *y = p + i * d;
      transform_row(x, y, d, aux, naux);
      x = y;
    }
    like = evaluate_row(x, d, q_scratch + i * nq, nq, aux, naux, L != nullptr, pass MLF_USER_GATE_ARGS);
  }
#if MLF_USER_TREGION
  if (lane < nrows) member2[i] = pass ? 1 : 0;   // pass implies mine
#endif
  if (L != nullptr && lane < nrows) L[i] = like;
}

#else  // MLF_USER_SUM: the wave-per-row entries

#ifdef MLF_USER_NSUMS
static_assert(MLF_USER_NSUMS >= 1 && MLF_USER_NSUMS <= 8, "MLF_USER_NSUMS: 1 to 8 sums");
#define MLF_USER_SUM_ENTRY MLF_USER_ENTRY(mlf_user_rows_sums)
#else
#define MLF_USER_SUM_ENTRY MLF_USER_ENTRY(mlf_user_rows_sum)
#endif

extern "C" __global__ __launch_bounds__(64) void MLF_USER_SUM_ENTRY(
    const double *u, long long n, int d, const unsigned char *member, const double *aux, long long naux, double *p, double *L,
    long long nterms MLF_USER_GATE_PARAMS MLF_USER_Q_PARAMS) {
  using namespace mlf_user_detail;
#if MLF_USER_GATE_DERIVED
  (void)q_scratch;   // (the direct default form's: here q lives in LDS, behind the p row)
#else
  const int nq = 0;
#endif
  const int lane = threadIdx.x;
  const long long i = blockIdx.x;   // one wave, one row
  if (i >= n) return;
  if (member != nullptr && member[i] == 0) {   // the same byte in every lane: the whole wave leaves
    if (lane == 0) {
      if (L != nullptr) L[i] = neg_inf();
#if MLF_USER_TREGION
      member2[i] = 0;
#endif
    }
    return;
  }
  extern __shared__ __attribute__((aligned(16))) double mlf_user_lds[];
  const bool p_buffer = p != nullptr && MLF_USER_HAS_TRANSFORM;
  double *a = mlf_user_lds;            // the u row
  double *b = p_buffer ? a + d : a;    // the p row (the u row itself without a transform)
  const double *src = u + i * d;
  for (int e = lane; e < d; e += 64) a[e] = src[e];
  __syncthreads();
#if MLF_USER_HAS_TRANSFORM
  if (p_buffer) {
    if (lane == 0) mlf_user_transform(a, b, d, aux, naux);
    __syncthreads();   // the other lanes read lane 0's p row from LDS
  }
#endif
#if MLF_USER_TREGION
  int inside = 0;
  if (lane == 0) inside = gate_row(b, d, b + d, nq, aux, naux MLF_USER_GATE_ARGS) ? 1 : 0;   // (q behind the p row)
  const bool pass = __builtin_amdgcn_readfirstlane(inside) != 0;   // all 64 lanes are active: lane 0 is the first
#else
  (void)nq;
  const bool pass = true;
#endif
  if (p != nullptr) {
    double *dst = p + i * d;
    for (int e = lane; e < d; e += 64) dst[e] = b[e];
  }
  double s = neg_inf();
  if (L != nullptr && pass) {
#ifdef MLF_USER_NSUMS
    double acc[MLF_USER_NSUMS];   // registers: every loop over j is unrolled
#pragma unroll
    for (int j = 0; j < MLF_USER_NSUMS; ++j) acc[j] = 0.0;
    for (long long k = lane; k < nterms; k += 64) {
      double t[MLF_USER_NSUMS];   // not pre-set: the terms function writes all of it
      mlf_user_loglike_terms(b, d, aux, naux, k, t);
#pragma unroll
      for (int j = 0; j < MLF_USER_NSUMS; ++j) acc[j] = acc[j] + t[j];
    }
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) {
#pragma unroll
      for (int j = 0; j < MLF_USER_NSUMS; ++j) acc[j] = acc[j] + __shfl_xor(acc[j], m);
    }
    s = mlf_user_loglike_finish(acc, MLF_USER_NSUMS, b, d, aux, naux);   // every lane, the same arguments; lane 0's is L
#else
    s = 0.0;
    for (long long k = lane; k < nterms; k += 64) s = s + mlf_user_loglike_term(b, d, aux, naux, k);
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) s = s + __shfl_xor(s, m);
#endif
  }
  if (lane == 0) {
    if (L != nullptr) L[i] = s;
#if MLF_USER_TREGION
    member2[i] = pass ? 1 : 0;
#endif
  }
}

#endif  // MLF_USER_SUM

#endif  // MLF_USER_ROWS_HOST
