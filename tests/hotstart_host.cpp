// Host build of ultranest_amd/csrc/mlf_hotstart_dev.hpp (tests/test_hotstart_host_build.py): the header's text is compiled as
// plain C++ with the HIP attributes defined away, and form (a) is evaluated on the rows read from standard input.  Numbers are
// hexadecimal floating literals, one per line where a block is read:
//   T n D        starts a tail of n values for inner dimension D: the next n lines hold one number each; the tail lives in a
//                heap block of exactly n values, so a load outside it is a finding of AddressSanitizer.  Its last value is M.
//   r            one cube row: the next D + 1 lines hold u[0..D]
// Output per row, one line: the segment j, whether the row is decided (xp[j] <= t, and t < xp[j+1] or j == M - 2 and
// t <= xp[M-1]), umod[0..D) and the weight (%a).
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <vector>

#define __device__
#define __forceinline__ inline

using std::log;

#include MLF_HS_HEADER

static bool read_value(double &v) {
  char line[256];
  if (!std::fgets(line, sizeof line, stdin)) return false;
  v = std::strtod(line, nullptr);
  return true;
}

int main() {
  char line[256];
  double *tail = nullptr;
  long long n = 0;
  int D = 0;
  while (std::fgets(line, sizeof line, stdin)) {
    if (line[0] == 'T') {
      if (std::sscanf(line + 1, "%lld %d", &n, &D) != 2 || n < 2 || D < 1 || D > 1024) {
        std::fprintf(stderr, "bad tail line: %s", line);
        return 2;
      }
      delete[] tail;
      tail = new double[n];
      for (long long k = 0; k < n; ++k)
        if (!read_value(tail[k])) return 2;
      const int M = (int)tail[n - 1];
      if (mlf_hotstart_contbox_tail(M, D) != n || mlf_hotstart_contbox_nin(tail, n, D) != 0) {
        std::fprintf(stderr, "the tail's length does not follow from M and D\n");
        return 2;
      }
    } else if (line[0] == 'r' && tail) {
      std::vector<double> u(D + 1), umod(D);
      for (int k = 0; k <= D; ++k)
        if (!read_value(u[k])) return 2;
      const int M = (int)tail[n - 1];
      const double weight = mlf_hotstart_contbox(u.data(), umod.data(), D, tail, M);
      const double t = u[D];
      const int j = mlf_hotstart_segment(t, tail, M);
      const bool decided = tail[j] <= t && (t < tail[j + 1] || (j == M - 2 && t <= tail[M - 1]));
      std::printf("%d %d", j, decided ? 1 : 0);
      for (int k = 0; k < D; ++k) std::printf(" %a", umod[k]);
      std::printf(" %a\n", weight);
    } else if (line[0] != '\n') {
      std::fprintf(stderr, "bad line: %s", line);
      return 2;
    }
  }
  delete[] tail;
  return 0;
}
