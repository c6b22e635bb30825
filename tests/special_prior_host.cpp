// Host build of ultranest_amd/csrc/mlf_priors_special_dev.hpp (tests/test_special_prior_host_build.py): the header's text is
// compiled as plain C++ with the three HIP attributes defined away, and every family is evaluated at the points read from
// standard input.  One input line per call: the family's letter, u, then the constants the generated code passes, all as
// hexadecimal floating literals.  One output line per call: the result (%a) and the number of Newton steps the call took.
// A last line "max <family letter> <steps>" per family reports the largest count.
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>

#define __device__
#define __noinline__
#define __forceinline__ inline

static int g_steps = 0;
#define MLF_PRIOR_SPECIAL_NOTE(steps) g_steps = (steps)

using std::copysign;
using std::exp;
using std::fabs;
using std::fmax;
using std::fmin;
using std::frexp;
using std::ldexp;
using std::rint;
using std::log;
using std::log1p;
using std::sqrt;

#include MLF_SPECIAL_HEADER

int main() {
  char line[1024];
  int most[256];
  std::memset(most, 0, sizeof most);
  while (std::fgets(line, sizeof line, stdin)) {
    char *s = line;
    while (*s == ' ') ++s;
    const unsigned char fam = (unsigned char)*s++;
    if (fam == '\n' || fam == 0) continue;
    double v[8];
    int n = 0;
    while (n < 8) {
      char *end;
      const double x = std::strtod(s, &end);
      if (end == s) break;
      v[n++] = x;
      s = end;
    }
    double r;
    g_steps = 0;
    if (fam == 'G' && n == 6) {
      r = mlf_prior_gamma(v[0], v[1], v[2], v[3], v[4], v[5]);
    } else if (fam == 'I' && n == 6) {
      r = mlf_prior_invgamma(v[0], v[1], v[2], v[3], v[4], v[5]);
    } else if (fam == 'B' && n == 6) {
      r = mlf_prior_beta(v[0], v[1], v[2], v[3], v[4], v[5]);
    } else if (fam == 'T' && n == 7) {
      r = mlf_prior_studentt(v[0], v[1], v[2], v[3], v[4], v[5], v[6]);
    } else {
      std::fprintf(stderr, "bad line: %s", line);
      return 2;
    }
    if (g_steps > most[fam]) most[fam] = g_steps;
    std::printf("%a %d\n", r, g_steps);
  }
  const char fams[] = "GIBT";
  for (int k = 0; k < 4; ++k) std::printf("max %c %d\n", fams[k], most[(unsigned char)fams[k]]);
  return 0;
}
