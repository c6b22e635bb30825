// Host build of ultranest_amd/csrc/mlf_refarith_dev.hpp (tests/test_refarith_host_build.py): the header's text is compiled as
// plain C++ with the HIP attributes defined away.  Numbers are hexadecimal floating literals, one per line where a block is
// read; every block lives in a heap block of exactly its size, so a load outside it is a finding of AddressSanitizer.
//   Q d n        quadratic form: the next lines hold the centre (d), the matrix (d x d, row-major) and n rows (d each).
//                Output per row: mlf_tregion_q<0>, mlf_tregion_q<KN> (KN = the instantiated bound at or above d; row and
//                matrix zero padded to it) and mlf_ell_q_row (the matrix with row stride d + 3).
//   B c n        band: the next lines hold eps_scale, enlarge and n pairs (qt, nrm2); chol_ok = c.  Output per pair: the band.
//   W n          wrap: the next lines hold n pairs (w, shift).  Output per pair: mlf_wrap_unit and mlf_wrap_unit_fast.
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <vector>

#define __device__
#define __forceinline__ inline

using std::fmod;

#include MLF_REFARITH_HEADER

static bool read_value(double &v) {
  char line[256];
  if (!std::fgets(line, sizeof line, stdin)) return false;
  v = std::strtod(line, nullptr);
  return true;
}

static bool read_block(double *p, long long n) {
  for (long long k = 0; k < n; ++k)
    if (!read_value(p[k])) return false;
  return true;
}

template <int KN>
static double q_bounded(int d, const double *row, const double *ctr, const double *A) {
  double *dl = new double[KN](), *mat = new double[(size_t)d * KN]();
  for (int k = 0; k < d; ++k) dl[k] = row[k] - ctr[k];
  for (int j = 0; j < d; ++j)
    for (int k = 0; k < d; ++k) mat[j * KN + k] = A[j * d + k];
  const double q = mlf_tregion_q<KN>(
      d, [&](int j) { return row[j] - ctr[j]; }, [&](int k) { return dl[k]; }, [&](int j, int k) { return mat[j * KN + k]; });
  delete[] dl;
  delete[] mat;
  return q;
}

static double q_bounded_for(int d, const double *row, const double *ctr, const double *A) {
  if (d <= 2) return q_bounded<2>(d, row, ctr, A);
  if (d <= 8) return q_bounded<8>(d, row, ctr, A);
  if (d <= 10) return q_bounded<10>(d, row, ctr, A);
  if (d <= 18) return q_bounded<18>(d, row, ctr, A);
  if (d <= 50) return q_bounded<50>(d, row, ctr, A);
  return q_bounded<64>(d, row, ctr, A);
}

int main() {
  char line[256];
  while (std::fgets(line, sizeof line, stdin)) {
    if (line[0] == 'Q') {
      int d = 0;
      long long n = 0;
      if (std::sscanf(line + 1, "%d %lld", &d, &n) != 2 || d < 1 || d > 64 || n < 0) return 2;
      const int lda = d + 3;
      double *ctr = new double[d], *A = new double[(size_t)d * d], *Al = new double[(size_t)(d - 1) * lda + d], *row = new double[d];
      if (!read_block(ctr, d) || !read_block(A, (long long)d * d)) return 2;
      for (int j = 0; j < d; ++j)
        for (int k = 0; k < d; ++k) Al[j * lda + k] = A[j * d + k];
      for (long long i = 0; i < n; ++i) {
        if (!read_block(row, d)) return 2;
        const auto delta = [&](int k) { return row[k] - ctr[k]; };
        const double q0 = mlf_tregion_q<0>(d, delta, delta, [&](int j, int k) { return A[j * d + k]; });
        std::printf("%a %a %a\n", q0, q_bounded_for(d, row, ctr, A), mlf_ell_q_row(row, ctr, d, Al, lda));
      }
      delete[] ctr;
      delete[] A;
      delete[] Al;
      delete[] row;
    } else if (line[0] == 'B') {
      int chol_ok = 0;
      long long n = 0;
      double eps_scale, enlarge, v[2];
      if (std::sscanf(line + 1, "%d %lld", &chol_ok, &n) != 2 || !read_value(eps_scale) || !read_value(enlarge)) return 2;
      for (long long i = 0; i < n; ++i) {
        if (!read_block(v, 2)) return 2;
        std::printf("%d\n", mlf_ell_band(v[0], v[1], eps_scale, enlarge, chol_ok));
      }
    } else if (line[0] == 'W') {
      long long n = 0;
      double v[2];
      if (std::sscanf(line + 1, "%lld", &n) != 1) return 2;
      for (long long i = 0; i < n; ++i) {
        if (!read_block(v, 2)) return 2;
        std::printf("%a %a\n", mlf_wrap_unit(v[0], v[1]), mlf_wrap_unit_fast(v[0], v[1]));
      }
    } else if (line[0] != '\n') {
      std::fprintf(stderr, "bad line: %s", line);
      return 2;
    }
  }
  return 0;
}
