// Host build of ultranest_amd/csrc/mlf_priors_rt_dev.hpp (tests/test_prior_rt_host_build.py): the header's text is compiled
// as plain C++ with the three HIP attributes defined away, and its functions are evaluated at the points read from standard
// input.  One input line per call, the numbers as hexadecimal floating literals (nan and inf as strtod reads them):
//   U u lo hi            mlf_prior_rt_uniform          L u lo hi            mlf_prior_rt_loguniform
//   N u mu sigma lo hi   mlf_prior_rt_truncnormal      R u lo mode hi       mlf_prior_rt_triangular
//   l v / s v / p v      the guards mlf_prior_rt_loc / _scale / _pos
//   T n steps            starts a table: the next 3 n - 1 lines hold one number each, [c | x | s]; the table lives in a heap
//                        block of exactly that size, so an out-of-table load is a finding of AddressSanitizer
//   t u                  mlf_prior_table(u, table, n, steps) of the last table
// One output line per call: the result (%a).  normcdfinv, which the device takes from its library, is supplied here: Newton's
// iteration on ln Phi with std::erfc, accurate to a few ulp of x.
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>

#define __device__
#define __noinline__
#define __forceinline__ inline

using std::erfc;
using std::exp;
using std::fabs;
using std::fmax;
using std::fmin;
using std::log;
using std::sqrt;

// x with Phi(x) = p for 0 < p <= 0.5 (and its mirror image above): ln Phi is concave, Newton from the asymptotic start
static double normcdfinv(double p) {
  if (!(p > 0.0 && p < 1.0)) return p == 0.0 ? -HUGE_VAL : (p == 1.0 ? HUGE_VAL : NAN);
  if (p > 0.5) return -normcdfinv(1.0 - p);
  const double r2 = 0x1.6a09e667f3bcdp+0, lnp = log(p);
  double x = -sqrt(-2.0 * lnp);
  if (p > 0.1) x = -1.2 * (0.5 - p) / 0.4 * 1.07;
  for (int it = 0; it < 100; ++it) {
    const double Phi = 0.5 * erfc(-x / r2);
    const double phi = exp(-0.5 * x * x) * 0x1.9884533d43651p-2;      // 1 / sqrt(2 pi)
    const double step = (log(Phi) - lnp) * Phi / phi;
    x -= step;
    if (fabs(step) <= 1e-16 * (1.0 + fabs(x))) break;
  }
  return x;
}

#include MLF_RT_HEADER

int main() {
  char line[1024];
  double *table = nullptr;
  int n = 0, steps = 0;
  while (std::fgets(line, sizeof line, stdin)) {
    char *s = line;
    while (*s == ' ') ++s;
    const char fam = *s++;
    if (fam == '\n' || fam == 0) continue;
    double v[8];
    int m = 0;
    while (m < 8) {
      char *end;
      const double x = std::strtod(s, &end);
      if (end == s) break;
      v[m++] = x;
      s = end;
    }
    double r;
    if (fam == 'U' && m == 3) {
      r = mlf_prior_rt_uniform(v[0], v[1], v[2]);
    } else if (fam == 'L' && m == 3) {
      r = mlf_prior_rt_loguniform(v[0], v[1], v[2]);
    } else if (fam == 'N' && m == 5) {
      r = mlf_prior_rt_truncnormal(v[0], v[1], v[2], v[3], v[4]);
    } else if (fam == 'R' && m == 4) {
      r = mlf_prior_rt_triangular(v[0], v[1], v[2], v[3]);
    } else if (fam == 'l' && m == 1) {
      r = mlf_prior_rt_loc(v[0]);
    } else if (fam == 's' && m == 1) {
      r = mlf_prior_rt_scale(v[0]);
    } else if (fam == 'p' && m == 1) {
      r = mlf_prior_rt_pos(v[0]);
    } else if (fam == 'T' && m == 2) {
      n = (int)v[0];
      steps = (int)v[1];
      if (n < 2 || n > (1 << 20)) {
        std::fprintf(stderr, "bad table size: %s", line);
        return 2;
      }
      delete[] table;
      table = new double[3 * n - 1];
      for (int k = 0; k < 3 * n - 1; ++k) {
        if (!std::fgets(line, sizeof line, stdin)) {
          std::fprintf(stderr, "table ends early\n");
          return 2;
        }
        table[k] = std::strtod(line, nullptr);
      }
      continue;
    } else if (fam == 't' && m == 1 && table) {
      r = mlf_prior_table(v[0], table, n, steps);
    } else {
      std::fprintf(stderr, "bad line: %s", line);
      return 2;
    }
    std::printf("%a\n", r);
  }
  delete[] table;
  return 0;
}
