// Host build of ultranest_amd/csrc/mlf_prep4_dev.hpp (tests/test_prep4_decide_host_build.py): the header's binary32 decisions
// compiled as plain C++ with the HIP attributes defined away (the device-only section stays off: no __HIPCC__).  Numbers are
// hexadecimal floating literals, the values of one record on one line; every block that a function reads through a pointer
// lives in a heap block of exactly its size, so a load outside it is a finding of AddressSanitizer.
//   U dp quant    uniform quantities: the next line holds the 15 constants, stats[0..4], r2 and sigma, the one after it the
//                 32 NT column constants.  Output: the 12 fields of Prep4Uniform.
//   E n           ellipsoid decision: the next line holds the 15 constants, then n lines (qs, dn2).
//                 Output per line: sure_in sure_out dnorm.
//   R form ks n   route and thresholds (form 0 = worst case, 1 = measured residues): n lines (sig_ok, namax, ea_max,
//                 zeta_scale, zeta0, sqrt_k, sr_lo, sr_hi, ins_any, nb, dnorm, eb2).  Output per line: route lo hi and the
//                 number of times the residue sum has been asked for so far.
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <iostream>
#include <string>
#include <vector>

#define __device__
#define __host__
#define __forceinline__ inline

#include MLF_PREP4_HEADER

using namespace mlf;

static bool read_line(std::vector<double> &v, size_t want) {
  std::string line;
  if (!std::getline(std::cin, line)) return false;
  v.clear();
  const char *p = line.c_str();
  while (true) {
    char *end = nullptr;
    const double x = std::strtod(p, &end);
    if (end == p) break;
    v.push_back(x);
    p = end;
  }
  return v.size() == want;
}

static Prep4Consts consts_of(const std::vector<double> &v) {
  Prep4Consts c;
  float *f[15] = {&c.g_chain, &c.y0n,    &c.lf,     &c.el,  &c.l_abs,  &c.s0n,       &c.eps_scale, &c.enl_lo,
                  &c.enl_hi,  &c.zt,     &c.zt_abs, &c.s_x, &c.inv_sx, &c.inv_sl_sx, &c.inv_st_sx};
  for (int i = 0; i < 15; ++i) *f[i] = (float)v[i];
  return c;
}

// the residue sum goes in as the kernels hand it over: a callable for the measured form (and it must be called on route 1
// only: `calls` counts), a plain value that nothing reads for the worst-case form
static long long calls = 0;
template <Prep4Thresholds TF, int KS>
static int route_one(const Prep4Uniform &u, bool ins_any, float nb, float dnorm, float eb2, float &lo, float &hi) {
  if constexpr (TF == Prep4Thresholds::kMeasured)
    return prep4_route<TF, KS>(u, ins_any, nb, dnorm, [&]() { ++calls; return eb2; }, lo, hi);
  else
    return prep4_route<TF, KS>(u, ins_any, nb, dnorm, 0.0f, lo, hi);
}
template <Prep4Thresholds TF>
static int route_ks(int ks, const Prep4Uniform &u, bool ins_any, float nb, float dnorm, float eb2, float &lo, float &hi) {
  switch (ks) {
    case 1: return route_one<TF, 1>(u, ins_any, nb, dnorm, eb2, lo, hi);
    case 4: return route_one<TF, 4>(u, ins_any, nb, dnorm, eb2, lo, hi);
    case 5: return route_one<TF, 5>(u, ins_any, nb, dnorm, eb2, lo, hi);
  }
  std::exit(2);
}

int main() {
  std::string head;
  std::vector<double> v;
  while (std::getline(std::cin, head)) {
    if (head.empty()) continue;
    if (head[0] == 'U') {
      int dp = 0, quant = 0;
      if (std::sscanf(head.c_str() + 1, "%d %d", &dp, &quant) != 2 || dp < 2 || dp > 64 || (dp & 1)) return 2;
      if (!read_line(v, 22)) return 2;
      const Prep4Consts c = consts_of(v);
      double *stats = new double[5];
      for (int i = 0; i < 5; ++i) stats[i] = v[15 + i];
      const double r2 = v[20], sigma = v[21];
      const int ncs = 32 * prep4_nt(dp);
      if (!read_line(v, (size_t)ncs)) return 2;
      float *csl = new float[ncs];
      for (int i = 0; i < ncs; ++i) csl[i] = (float)v[i];
      Prep4Uniform u;
      prep4_uniform(c, stats, r2, csl, sigma, dp, quant != 0, u);
      std::printf("%d %a %a %a %a %a %a %a %a %a %a %a\n", (int)u.sig_ok, u.sig_f, u.sqrt_k, u.namax, u.ea_max, u.zeta_scale, u.zeta0,
                  u.kappa, u.sr_lo, u.sr_hi, u.inv_sx2, u.inv_slsx2);
      delete[] stats;
      delete[] csl;
    } else if (head[0] == 'E') {
      long long n = 0;
      if (std::sscanf(head.c_str() + 1, "%lld", &n) != 1 || !read_line(v, 15)) return 2;
      const Prep4Consts c = consts_of(v);
      for (long long i = 0; i < n; ++i) {
        if (!read_line(v, 2)) return 2;
        bool sure_in = false, sure_out = false;
        float dnorm = 0.0f;
        prep4_ell_decide(c, (float)v[0], (float)v[1], dnorm, sure_in, sure_out);
        std::printf("%d %d %a\n", (int)sure_in, (int)sure_out, dnorm);
      }
    } else if (head[0] == 'R') {
      int form = 0, ks = 0;
      long long n = 0;
      if (std::sscanf(head.c_str() + 1, "%d %d %lld", &form, &ks, &n) != 3) return 2;
      for (long long i = 0; i < n; ++i) {
        if (!read_line(v, 12)) return 2;
        Prep4Uniform u{};
        u.sig_ok = v[0] != 0.0;
        u.namax = (float)v[1];
        u.ea_max = (float)v[2];
        u.zeta_scale = (float)v[3];
        u.zeta0 = (float)v[4];
        u.sqrt_k = (float)v[5];
        u.sr_lo = (float)v[6];
        u.sr_hi = (float)v[7];
        float lo = 0.0f, hi = 0.0f;
        const int rt = form ? route_ks<Prep4Thresholds::kMeasured>(ks, u, v[8] != 0.0, (float)v[9], (float)v[10], (float)v[11], lo, hi)
                            : route_ks<Prep4Thresholds::kWorstCase>(ks, u, v[8] != 0.0, (float)v[9], (float)v[10], (float)v[11], lo, hi);
        std::printf("%d %a %a %lld\n", rt, lo, hi, calls);
      }
    } else {
      std::fprintf(stderr, "bad line: %s\n", head.c_str());
      return 2;
    }
  }
  return 0;
}
