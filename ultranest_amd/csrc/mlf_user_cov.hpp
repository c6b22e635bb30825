// mlf_user_cov.hpp -- the kernel the library launches around a user model whose likelihood is a Gaussian with a dense,
// parameter-dependent covariance (ultranest_amd/devicemodel.py "Gaussian likelihoods with a dense covariance", mlf_user.hip).
// hiprtc compiles this header, INSTEAD of mlf_user_rows.hpp, with the user's source in front of it and -DMLF_USER_NCOV=n; that
// source defines, instead of mlf_user_loglike,
//
//   __device__ double mlf_user_cov(const double *p, int d, const double *aux, long long naux, int i, int j);   // 0 <= j <= i < n
//   __device__ double mlf_user_resid(const double *p, int d, const double *aux, long long naux, int i);        // 0 <= i < n
//   __device__ void mlf_user_transform(const double *u, double *p, int d, const double *aux, long long naux);  // optional
//
// (pure functions of their arguments; only the lower triangle of the covariance is asked for) and
//
//   L(p) = -1/2 r^T K^-1 r - 1/2 ln det K - (n/2) ln 2 pi,   K_ij = cov(i, j), r_i = resid(i).
//
// The library itself includes the header with MLF_USER_COV_HOST defined, for mlf_user_rows_cov_lds_bytes alone.
//
// Entries: mlf_user_rows_cov and, with -DMLF_USER_TREGION=1, mlf_user_rows_cov_tregion; each the only kernel of its program.  They
// take the eight parameters of mlf_user_rows (u, n, d, member, aux, naux, p, L: mlf_user_rows.hpp), then `double *tri`, then the
// gate's five in the gated entry (9 and 14).  tri (nullable): the row's augmented factor, (n + 1)(n + 2) / 2 doubles per row, for
// mlf_covmodel_factor; every route passes NULL.
//
// ONE WORKGROUP OF 256 THREADS (four waves) OWNS ONE ROW, blockIdx.x = row.
//   1. all threads read the row's member byte and leave together if it is 0; lane 0 has then written L = -inf (member2 = 0);
//   2. wave 0 copies the u row into LDS with coalesced loads;
//   3. lane 0 runs mlf_user_transform from it into a second LDS row (without a transform the u row is the p row);
//   4. in the gated entry lane 0 runs mlf_tregion_inside on the p row; the verdict goes through LDS and a barrier.  The p row of
//      every member row leaves with coalesced stores, whether or not it passes (as in the summed form);
//   5. all 256 threads fill the augmented triangle from the user functions, p pointing into LDS;
//   6. the right-looking column loop below, two barriers per column;
//   7. a copy of the current column (its diagonal included) is kept in a contiguous LDS vector `col`: an update reads one broadcast
//      word col[i], one unit-stride word col[j] and its own element, not two strided places of the packed triangle;
//   8. every thread reads the pivot word itself from LDS after the barrier that completes it -- the same word in every thread, so
//      every thread takes the same path through every barrier -- and lane 0 records a failure in an LDS word for the tail.
//
// THE ARITHMETIC CONTRACT (part of the interface; compiled with -ffp-contract=off like every user program).  It does not depend on
// how the threads share the work.
//   augmented triangle  A is the packed lower triangle of an (n + 1) x (n + 1) matrix, element (i, j), j <= i, at i (i + 1) / 2 + j:
//                       A_ij = cov(i, j) for j <= i < n, A_nj = resid(j), A_nn is unused (0.0 in tri).
//   factor              for k = 0 .. n-1 in order: the pivot is A_kk after its updates; L_kk = sqrt(A_kk); L_ik = A_ik / L_kk for
//                       k < i <= n; every remaining A_ij (k < j <= i, j < n) becomes A_ij - L_ik * L_jk, one multiplication and one
//                       subtraction, each rounded: no fused multiply-add is formed.  Every element receives its subtractions in
//                       ascending k, so its value is independent of the schedule.  Row n of the factor is z = Lfac^-1 r.
//   sums                quad = sum_k z_k * z_k and h = sum_k log(L_kk), both sequential from 0.0 in ascending k (the logarithms are
//                       taken in parallel, the additions are one lane's).
//   likelihood          L = ((-0.5 * quad) - h) - (double)n * 0.91893853320467274178.
//   failure             the first pivot in ascending k that is not > 0 decides: a NaN pivot gives L = NaN, any other L = -inf;
//                       nothing after it is computed; tri of that row is NaN throughout.
//   skipped rows        a row outside the membership mask, or one that fails the t-region gate, calls neither function: L = -inf
//                       (its p row is treated as in the summed form: not written outside the mask, written when it fails the gate).
//   independence        L does not depend on the row's position, the batch size, the mask or the route.
//
// LDS.  Static, sized from MLF_USER_NCOV (mlf_user_rows_cov_lds_bytes): the triangle, (n + 1)(n + 2) / 2 doubles; col, n + 1 doubles;
// one word of flags.  Dynamic, as in the summed form: the u row and, where a transform writes one, the p row
// (mlf_user_rows_sum_lds_bytes).  A workgroup may declare all 163,840 bytes of a CU on this device; static + dynamic above that is
// refused by the Python constructor (devicemodel.max_ncov: n = 199 at small d with this layout).  Larger matrices need the factor
// in HBM with LDS panels: a later step.
#pragma once

#define MLF_USER_COV_THREADS 256
#define MLF_USER_COV_LDS_CAP 163840

// doubles of the packed augmented triangle of an n x n covariance
__host__ __device__ constexpr inline unsigned mlf_user_rows_cov_tri_doubles(int n) {
  return (unsigned)(n + 1) * (unsigned)(n + 2) / 2u;
}

// bytes of STATIC LDS of the covariance kernels at MLF_USER_NCOV = n: the triangle, the column vector and the flag word
__host__ __device__ constexpr inline unsigned mlf_user_rows_cov_lds_bytes(int n) {
  return ((mlf_user_rows_cov_tri_doubles(n) + (unsigned)(n + 1) + 1u + 1u) & ~1u) * 8u;   // (a multiple of 16: the dynamic rows follow)
}

#ifndef MLF_USER_COV_HOST

#ifndef MLF_USER_NCOV
#error "the covariance programs are compiled with -DMLF_USER_NCOV=n"
#endif
#ifndef MLF_USER_HAS_TRANSFORM
#define MLF_USER_HAS_TRANSFORM 0
#endif
#ifndef MLF_USER_TREGION
#define MLF_USER_TREGION 0
#endif
static_assert(MLF_USER_NCOV >= 1 && mlf_user_rows_cov_lds_bytes(MLF_USER_NCOV) <= MLF_USER_COV_LDS_CAP,
              "MLF_USER_NCOV: the augmented triangle must fit the LDS of one CU");
#if MLF_USER_TREGION
#include "mlf_tregion_dev.hpp"
#define MLF_USER_COV_ENTRY mlf_user_rows_cov_tregion
#else
#define MLF_USER_COV_ENTRY mlf_user_rows_cov
#endif

namespace mlf_user_cov_detail {

constexpr int kN = MLF_USER_NCOV;
constexpr int kThreads = MLF_USER_COV_THREADS;
constexpr int kTri = (kN + 1) * (kN + 2) / 2;

__device__ inline double neg_inf() { return -__builtin_inf(); }
__device__ inline int at(int i, int j) { return i * (i + 1) / 2 + j; }

// row of packed element e: the largest i with i (i + 1) / 2 <= e (a float estimate, corrected in integers)
__device__ inline int row_of(int e) {
  int i = (int)((__builtin_sqrtf(8.0f * (float)e + 1.0f) - 1.0f) * 0.5f);
  while (i * (i + 1) / 2 > e) --i;
  while ((i + 1) * (i + 2) / 2 <= e) ++i;
  return i;
}

}  // namespace mlf_user_cov_detail

extern "C" __global__ __launch_bounds__(MLF_USER_COV_THREADS) void MLF_USER_COV_ENTRY(
    const double *u, long long n, int d, const unsigned char *member, const double *aux, long long naux, double *p, double *L,
    double *tri
#if MLF_USER_TREGION
    ,
    const double *__restrict__ tr_A, const double *__restrict__ tr_ctr, const double *__restrict__ tr_fixed, double tr_enlarge,
    unsigned char *member2
#endif
) {
  using namespace mlf_user_cov_detail;
  const int tid = threadIdx.x;
  const long long row = blockIdx.x;   // one workgroup, one row
  if (row >= n) return;
  if (member != nullptr && member[row] == 0) {   // the same byte in every thread: the whole workgroup leaves
    if (tid == 0) {
      if (L != nullptr) L[row] = neg_inf();
#if MLF_USER_TREGION
      member2[row] = 0;
#endif
    }
    return;
  }
  __shared__ __attribute__((aligned(16))) double cov_lds[mlf_user_rows_cov_lds_bytes(kN) / 8];
  extern __shared__ __attribute__((aligned(16))) double mlf_user_lds[];
  double *A = cov_lds;                      // the packed augmented triangle
  double *col = A + kTri;                   // column k of the factor, rows k .. n, at its row index; entries < k: earlier diagonals
  int *flags = (int *)(col + kN + 1);       // [0] the gate's verdict, [1] 0 | 1 pivot not > 0 | 2 pivot NaN
  const bool p_buffer = p != nullptr && MLF_USER_HAS_TRANSFORM;
  double *a = mlf_user_lds;                 // the u row
  double *b = p_buffer ? a + d : a;         // the p row (the u row itself without a transform)
  if (tid < 64) {
    const double *src = u + row * d;
    for (int e = tid; e < d; e += 64) a[e] = src[e];
  }
  if (tid == 0) flags[0] = 1, flags[1] = 0;
  __syncthreads();
#if MLF_USER_HAS_TRANSFORM
  if (p_buffer) {
    if (tid == 0) mlf_user_transform(a, b, d, aux, naux);
    __syncthreads();   // the other threads read lane 0's p row from LDS
  }
#endif
#if MLF_USER_TREGION
  if (tid == 0) flags[0] = mlf_tregion_inside(b, d, tr_A, tr_ctr, tr_fixed, tr_enlarge) ? 1 : 0;
  __syncthreads();
#endif
  const bool pass = flags[0] != 0;   // the same word in every thread
  if (p != nullptr && tid < 64) {
    double *dst = p + row * d;
    for (int e = tid; e < d; e += 64) dst[e] = b[e];
  }
#if MLF_USER_TREGION
  if (tid == 0) member2[row] = pass ? 1 : 0;
#endif
  if (L == nullptr) return;   // transform only
  if (!pass) {
    if (tid == 0) L[row] = neg_inf();
    return;
  }

  // 5. the augmented triangle: element e = (i, j); row n holds the residuals, A_nn is unused
  for (int e = tid; e < kTri; e += kThreads) {
    const int i = row_of(e), j = e - i * (i + 1) / 2;
    A[e] = i < kN ? mlf_user_cov(b, d, aux, naux, i, j) : j < kN ? mlf_user_resid(b, d, aux, naux, j) : 0.0;
  }
  __syncthreads();

  // 6. right-looking columns.  At the top of column k every A_ik, i >= k, has received its k subtractions.
  const int wave = tid >> 6, lane = tid & 63;
  for (int k = 0; k < kN; ++k) {
    const double piv = A[at(k, k)];   // the same word in every thread; nobody writes it before the barrier below
    if (!(piv > 0.0)) {
      if (tid == 0) flags[1] = piv != piv ? 2 : 1;
      break;
    }
    const double lkk = sqrt(piv);
    for (int i = k + 1 + tid; i <= kN; i += kThreads) {
      const double v = A[at(i, k)] / lkk;
      A[at(i, k)] = v;
      col[i] = v;
    }
    if (tid == 0) col[k] = lkk;
    __syncthreads();
    if (tid == 0) A[at(k, k)] = lkk;   // (no thread reads the diagonal of column k again)
    // the trailing update: a wave takes rows i = k + 1 + wave, + 4, ... <= n, four of them at a time (their loads ahead of their
    // stores); its lanes the columns j = k + 1 + lane, + 64, ... <= min(i, n - 1)
    for (int i0 = k + 1 + wave; i0 <= kN; i0 += 16) {
      for (int j = k + 1 + lane; j < kN && j <= i0 + 12; j += 64) {
        const double cj = col[j];
        double x[4], ci[4];
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const int i = i0 + 4 * r;
          const bool on = i <= kN && j <= i;
          ci[r] = on ? col[i] : 0.0;
          x[r] = on ? A[at(i, j)] : 0.0;
        }
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const int i = i0 + 4 * r;
          if (i <= kN && j <= i) {
            const double m = ci[r] * cj;
            A[at(i, j)] = x[r] - m;
          }
        }
      }
    }
    __syncthreads();
  }
  __syncthreads();   // flags[1]; after a failure also the tail of the last column's barrier pair
  const int failed = flags[1];

  if (tri != nullptr) {
    double *dst = tri + row * kTri;
    const double nan = __builtin_nan("");
    for (int e = tid; e < kTri; e += kThreads) dst[e] = failed ? nan : A[e];
  }
  if (failed) {
    if (tid == 0) L[row] = failed == 2 ? __builtin_nan("") : neg_inf();
    return;
  }
  // the logarithms in parallel (col[k], k < n, holds L_kk), the two sums on lane 0
  for (int k = tid; k < kN; k += kThreads) col[k] = log(col[k]);
  __syncthreads();
  if (tid == 0) {
    double quad = 0.0, h = 0.0;
    for (int k = 0; k < kN; ++k) {
      const double z = A[at(kN, k)];
      quad = quad + z * z;
    }
    for (int k = 0; k < kN; ++k) h = h + col[k];
    L[row] = ((-0.5 * quad) - h) - (double)kN * 0.91893853320467274178;
  }
}

#endif  // MLF_USER_COV_HOST
