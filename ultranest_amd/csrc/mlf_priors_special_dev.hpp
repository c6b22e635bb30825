// mlf_priors_special_dev.hpp -- iterative quantile functions (inverse incomplete gamma and beta functions) for the prior
// transform of a user model (ultranest_amd/priors.py): Gamma, ChiSquared, InverseGamma, Beta, StudentT and the Gamma(alpha, 1)
// column of a Dirichlet block.  Its text follows that of mlf_priors_dev.hpp in a generated ``transform_source`` only when the
// list of priors holds one of these families; the contract is that header's: compiled at run time with the model (hiprtc,
// -O3 -std=c++17 -ffp-contract=off), plain HIP C++17, no inline assembly, no intrinsics, no data tables, no local arrays.
//
// Every family is one __device__ __noinline__ leaf function; the shared pieces (starting values, the incomplete gamma series
// and continued fraction, the incomplete beta continued fraction, the two Newton iterations) are __device__ __forceinline__.
//
// u lies in the open interval (0, 1); every function works from the smaller tail q = min(u, 1 - u) (1 - u is exact for
// u >= 0.5) and iterates on the LOGARITHM of that tail's probability in the LOGARITHM of the unknown:
//
//   gamma   ln P(a, x) = ln q  (lower) or  ln Q(a, x) = ln q  (upper)  in  t = ln x
//   beta    ln I_x(a, b) = ln q  in  t = ln x  while the root is at most 0.5, else in  t = ln(1 - x)
//
// ln(tail) is concave in t for both (the gamma and the beta distribution have an increasing generalized failure rate), so
// Newton's iteration approaches the root monotonically from one side after at most one step across it, and a tail that is
// nearly a power of x is nearly linear: x = exp(t) may underflow to 0 by itself (Gamma(0.1) at u = 2^-1022 is 2^-10220) while
// t stays an ordinary number.  Constants "from the host" are computed in binary64 by priors.py (math.lgamma, math.log).
//
//   family (parameters)              p(u)
//   Gamma(shape, scale)              scale * x;  P(shape, x) = u for u <= 0.5, Q(shape, x) = 1 - u otherwise
//   ChiSquared(k)                    Gamma(k / 2, 2): the same function
//   InverseGamma(shape, scale)       scale / x;  Q(shape, x) = u for u <= 0.5, P(shape, x) = 1 - u otherwise
//   Beta(a, b)                       u <= 0.5: I_x(a, b) = u;  else I_y(b, a) = 1 - u, y = 1 - x;  the smaller of x and y is
//                                    the iteration's unknown s, the result s or 1 - s
//   StudentT(nu, loc, scale)         q = min(u, 1 - u), x = nu / (nu + t^2):  2 q <= 5/8: I_x(nu/2, 1/2) = 2 q, else
//                                    I_y(1/2, nu/2) = 1 - 2 q;  t = -exp((ln nu + ln y - ln x) / 2), sign flipped for u > 0.5,
//                                    t = 0 at u = 0.5;  loc + scale * t
//   Dirichlet(alpha), block          g_k = mlf_prior_gamma(u_k, 1, alpha_k, ...) into p[k];  s = ((g_0 + g_1) + ...) + g_(n-1);
//                                    p[k] = g_k / s, or 1 / n for every k if s == 0   (generated as straight-line statements)
//
// Shape of the loops.  The wrapper kernel must keep its scalar registers across these calls, and the 64-bit constants of
// every exp and log that stands inside a loop stay in scalar registers for the whole loop.  So each Newton loop holds exactly
// ONE exp and ONE log: a step whose tail is the complement of the sum it has (Q from the series of P, I_x from the continued
// fraction of I_y) takes a second trip through the loop for its second exponential, and ln(1 - s) is an atanh series with
// no constants.  One trip is therefore "exp, then either the sum and the log, or the sum and the next exp's argument".
//
// No loop's exit depends on convergence alone: a Newton iteration makes at most MLF_PRIOR_SPECIAL_MAX_STEPS steps (twice as
// many trips) and a series or continued fraction sums at most MLF_PRIOR_SPECIAL_MAX_TERMS terms; at the cap a function
// returns its current iterate.  (A host build may define the two caps and MLF_PRIOR_SPECIAL_NOTE(steps) before this text to
// lower a cap or to record the number of steps a call took; the generated source defines none of them.)
#ifndef MLF_PRIORS_SPECIAL_DEV_HPP
#define MLF_PRIORS_SPECIAL_DEV_HPP

#ifndef MLF_PRIOR_SPECIAL_MAX_STEPS
#define MLF_PRIOR_SPECIAL_MAX_STEPS 48
#endif
#ifndef MLF_PRIOR_SPECIAL_MAX_TERMS
#define MLF_PRIOR_SPECIAL_MAX_TERMS 3000
#endif
#ifndef MLF_PRIOR_SPECIAL_NOTE
#define MLF_PRIOR_SPECIAL_NOTE(steps)
#endif
// End of a Newton iteration.  It converges quadratically, |error after a step| <= K * step^2 with K <= 30 over the accepted
// parameter ranges (K = |f'' / 2 f'| of ln(tail) in t).  After a step of at most 2^-17 the iterate is within 2e-9 of the root;
// it is rounded to a multiple of 2^-24 and ONE more step is taken from there (error <= 30 * (2^-25 + 2e-9)^2 < 3e-14, a
// fortieth of the bound).  Neighbouring u reach the same rounded point, and the last step, t - (F(t) - ln q) / F'(t) with
// F(t) and F'(t) the same numbers for both, is a monotone function of ln q in floating point: the quantile does not step
// backwards between adjacent u through the noise of the iteration (except where two iterates straddle a multiple of 2^-24,
// one pair of neighbours in 10^8).  The rounded point itself is about 1e-8 from the root, far outside the bound: an
// iteration that the cap ends there shows in every accuracy test.

// starting value only: the standard normal upper quantile z >= 0 of a tail probability q <= 0.5 from ln q (Abramowitz and
// Stegun 26.2.23, |error| < 4.5e-4)
__device__ __forceinline__ double mlf_psp_z(double lnq) {
  const double t = sqrt(-2.0 * lnq);
  const double z = t - (2.515517 + t * (0.802853 + t * 0.010328)) / (1.0 + t * (1.432788 + t * (0.189269 + t * 0.001308)));
  return fmax(z, 0.0);
}

// ln(1 - s) for 0 <= s <= 0.5, relatively accurate down to s = 0:  -2 atanh(w) = -2 (w + w^3 / 3 + w^5 / 5 + ...),
// w = s / (2 - s) <= 1/3 (at most 17 terms)
__device__ __forceinline__ double mlf_psp_ln1m(double s) {
  const double w = s / (2.0 - s);
  const double w2 = w * w;
  double term = w, sum = w;
  for (int k = 1; k < MLF_PRIOR_SPECIAL_MAX_TERMS; ++k) {
    term *= w2;
    const double add = term / (2.0 * k + 1.0);
    sum += add;
    if (ldexp(add, 53) <= sum) break;
  }
  return -2.0 * sum;
}

// ln v for v > 0 inside a Newton loop, where the library's log would keep ten 64-bit constants in scalar registers:
// v = m 2^k with m in [1/2, 1),  ln v = k ln 2 + 2 atanh(w),  w = (m - 1) / (m + 1) in (-1/3, 0] (at most 17 terms); ln 2 in
// the two words that mlf_psp_exp uses
__device__ __forceinline__ double mlf_psp_log(double v) {
  int k;
  const double m = frexp(v, &k);
  const double w = (m - 1.0) / (m + 1.0);
  const double w2 = w * w;
  double term = w, sum = w;
  for (int j = 1; j < MLF_PRIOR_SPECIAL_MAX_TERMS; ++j) {
    term *= w2;
    const double add = term / (2.0 * j + 1.0);
    sum += add;
    if (ldexp(fabs(add), 53) <= fabs(sum)) break;
  }
  return k * 0x1.62e42feep-1 + (k * 0x1.a39ef35793c76p-33 + 2.0 * sum);
}

// exp(arg) inside a Newton loop, for the same reason (the library's exp keeps seventeen): arg = k ln 2 + r, |r| <= ln 2 / 2,
// with the two-word ln 2 of fdlibm (k times its upper word is exact), e^r - 1 = r + r^2 / 2 + ... (at most 15 terms), and
// one ldexp, which underflows to 0 and overflows to infinity by itself.  The only 64-bit constants of the three functions
// above and below are these two words: every tolerance is an ldexp by a small integer, which needs no register
__device__ __forceinline__ double mlf_psp_exp(double arg) {
  int ex;
  const double am = frexp(arg == arg ? arg : 0.0, &ex);
  arg = ldexp(am, ex < 11 ? ex : 11);            // |arg| < 2048, unchanged below that: the int conversion below is defined
  const double kf = rint(arg / 0x1.62e42feep-1);
  const double nk = -kf;                         // the same two constants as in mlf_psp_log, signs included
  const double r = (arg + nk * 0x1.62e42feep-1) + nk * 0x1.a39ef35793c76p-33;
  double term = r, sum = r;
  for (int j = 2; j < MLF_PRIOR_SPECIAL_MAX_TERMS; ++j) {
    term *= r / j;
    sum += term;
    if (ldexp(fabs(term), 53) <= 1.0) break;
  }
  return ldexp(1.0 + sum, (int)kf);
}

// S(a, x) = 1 + x / (a + 1) + x^2 / ((a + 1) (a + 2)) + ... :  P(a, x) = x^a e^-x / Gamma(a + 1) * S   (for x < a + 1)
__device__ __forceinline__ double mlf_psp_gamma_series(double a, double x) {
  double sum = 1.0, term = 1.0, ap = a;
  for (int n = 0; n < MLF_PRIOR_SPECIAL_MAX_TERMS; ++n) {
    ap += 1.0;
    term *= x / ap;
    sum += term;
    if (ldexp(term, 53) <= sum) break;
  }
  return sum;
}

// h(a, x):  Q(a, x) = x^a e^-x / Gamma(a) * h   (for x >= a + 1; Lentz's evaluation of Legendre's continued fraction)
__device__ __forceinline__ double mlf_psp_gamma_cf(double a, double x) {
  double b = x + 1.0 - a;
  double c = 0.0;                                // Lentz's c_0 is infinite: c_1 = b_1
  double d = 1.0 / b;
  double h = d;
  for (int i = 1; i <= MLF_PRIOR_SPECIAL_MAX_TERMS; ++i) {
    const double an = -i * (i - a);
    b += 2.0;
    d = 1.0 / (an * d + b);                      // no denominator vanishes for x >= a + 1
    c = i == 1 ? b : b + an / c;
    const double del = d * c;
    h *= del;
    if (ldexp(fabs(del - 1.0), 53) <= 1.0) break;
  }
  return h;
}

// t = ln x with P(a, x) = q (upper == false) or Q(a, x) = q (upper == true), q <= 0.5 given as ln q.
// inva = 1 / a, lna = ln a, lg1 = lgamma(a + 1) from the host.
__device__ __forceinline__ double mlf_psp_gamma_lnx(double lnq, bool upper, double a, double inva, double lna, double lg1) {
  // starting value.  Lower tail: P(a, x) <= x^a / Gamma(a + 1) gives a lower bound of the root, exact in the limit x -> 0;
  // Wilson-Hilferty where it is larger.  Upper tail: Wilson-Hilferty for a >= 1; for a < 1, Q(a, x) <= e^-x / Gamma(a) for
  // x >= 1 gives an upper bound of the root
  const double z = mlf_psp_z(lnq);
  const double c = 1.0 - inva / 9.0 + (upper ? z : -z) * sqrt(inva) / 3.0;
  const bool wh = c > 0.0 && !(upper && a < 1.0);
  const double l = log(wh ? c : fmax(1.0, -lnq - (lg1 - lna)));
  const double small = (lnq + lg1) * inva;
  double t;
  if (!upper) {
    t = wh ? fmax(small, lna + 3.0 * l) : small;
  } else {
    t = wh ? lna + 3.0 * l : l;
  }
  // one trip: e = exp(arg); first trip of a step: x = e, the sum v for x, base = ln of the factor in front of v.  If the sum's
  // own tail is the wanted one (natural), f = base + ln v - ln q; otherwise a second trip takes E = exp(base): the other
  // tail is W = E v and f = ln(1 - W) - ln q
  // (the state between trips is kept in numbers, not in flags: a flag that lives across the loop is a scalar register pair)
  double arg = t, v = 0.0, base = 0.0, mul = 1.0;
  bool second = false;
  int left = MLF_PRIOR_SPECIAL_MAX_STEPS;         // steps left; -1 once the iterate has been rounded for the last step
  int it = 0;                                     // steps taken, for MLF_PRIOR_SPECIAL_NOTE alone
  for (int n = 0; n < 2 * MLF_PRIOR_SPECIAL_MAX_STEPS + 2 && left != 0; ++n) {
    const double e = mlf_psp_exp(arg);
    double larg, mag;                            // the log's argument and |d ln(tail) / dt|
    if (!second) {
      const double lnD = a * t - e - lg1;        // ln of x^a e^-x / Gamma(a + 1);  x * pdf = a * D
      const bool series = e < a + 1.0;
      if (series) {
        v = mlf_psp_gamma_series(a, e);
        base = lnD;
        mul = a;
      } else {
        v = mlf_psp_gamma_cf(a, e);
        base = lna + lnD;
        mul = 1.0;
      }
      if (series == upper) {                     // not the sum's own tail
        second = true;
        arg = base;
        base = 0.0;
        continue;
      }
      larg = v;
      mag = mul / v;
    } else {
      second = false;
      larg = 1.0 - e * v;
      mag = mul * e / larg;
    }
    if (!(larg > 0.0)) break;                    // no tail left to take the logarithm of: keep the iterate
    const double f = base + mlf_psp_log(larg) - lnq;
    double dt = upper ? -f / mag : f / mag;
    if (!(dt == dt)) break;                      // a NaN step changes nothing
    const double lim = 4.0 + fabs(t);
    dt = fmin(fmax(dt, -lim), lim);
    t -= dt;
    ++it;
    const bool fin = left < 0;                   // this was the one step from the rounded point
    left = fin ? 0 : left - 1;
    if (!fin && fabs(ldexp(dt, 17)) <= 1.0) {    // the last step starts from a multiple of 2^-24 (see above)
      t = ldexp(ldexp(rint(ldexp(t, 24)), -12), -12);
      if (left > 0) left = -1;
    }
    arg = t;
  }
  MLF_PRIOR_SPECIAL_NOTE(it);
  return t;
}

// the continued fraction of the incomplete beta function:  I_x(a, b) = x^a y^b / (a B(a, b)) * h   (for x <= (a+1)/(a+b+2), where Lentz's
// evaluation meets no vanishing denominator short of an exact cancellation, which ends the iteration with a NaN step)
__device__ __forceinline__ double mlf_psp_beta_cf(double a, double b, double x) {
  const double qab = a + b, qap = a + 1.0, qam = a - 1.0;
  double c = 1.0;
  double d = 1.0 / (1.0 - qab * x / qap);          // x <= (a + 1) / (a + b + 2) < qap / qab
  double h = d;
  for (int m = 1; m <= MLF_PRIOR_SPECIAL_MAX_TERMS; ++m) {
    const double m2 = 2.0 * m;
    double aa = m * (b - m) * x / ((qam + m2) * (a + m2));
    d = 1.0 / (1.0 + aa * d);
    c = 1.0 + aa / c;
    h *= d * c;
    aa = -(a + m) * (qab + m) * x / ((a + m2) * (qap + m2));
    d = 1.0 / (1.0 + aa * d);
    c = 1.0 + aa / c;
    const double del = d * c;
    h *= del;
    if (ldexp(fabs(del - 1.0), 53) <= 1.0) break;
  }
  return h;
}

// The smaller one, s, of x and 1 - x with I_x(a, b) = q, q <= 0.5 given with ln q: t = ln s is returned, s = exp(t) and
// by_y (s is 1 - x) through the references.  lnB = lgamma(a) + lgamma(b) - lgamma(a + b), lna = ln a, lnb = ln b from the host.
__device__ __forceinline__ double mlf_psp_beta_lns(double q, double lnq, double a, double b, double lnB, double lna, double lnb,
                                                   double &s_out, bool &by_y_out) {
  const double ln_half = -0x1.62e42fefa39efp-1;
  // starting values of both forms, t = ln x (tx) and t = ln y (ty)
  double tx, ty;
  if (a >= 1.0 && b >= 1.0) {
    // Abramowitz and Stegun 26.5.22: x = a / (a + b e^2w), y = b e^2w / (a + b e^2w)
    const double z = -mlf_psp_z(lnq);
    const double al = (z * z - 3.0) / 6.0;
    const double ra = 1.0 / (2.0 * a - 1.0), rb = 1.0 / (2.0 * b - 1.0);
    const double hm = 2.0 / (ra + rb);
    const double w = z * sqrt(al + hm) / hm - (rb - ra) * (al + 5.0 / 6.0 - 2.0 / (3.0 * hm));
    const double r = fmin(fmax(lnb - lna + 2.0 * w, -700.0), 700.0);        // ln(y / x)
    tx = -(fmax(r, 0.0) + log(1.0 + exp(-fabs(r))));
    ty = tx + r;
    // for b >= 1, I_x <= x^a / (a B) bounds the root from below, and is the far tail's limit, where the normal form is poor
    tx = fmax(tx, (lnq + lna + lnB) / a);
  } else {
    tx = (lnq + lna + lnB) / a;                   // I_x ~ x^a / (a B)
    ty = (mlf_psp_ln1m(q) + lnb + lnB) / b;       // 1 - I_x = I_y(b, a) ~ y^b / (b B)
  }
  const double split = (a + 1.0) / (a + b + 2.0);
  // the first pass through the loop evaluates I_0.5(a, b): below q, the root is above 0.5 and the unknown is y (by_y).
  // Then as for the gamma function: e = exp(arg); first trip of a step: s = e, the continued fraction v on the side of the
  // mean s lies on, base = ln of the factor in front of it.  direct: f = base + ln v - ln q; otherwise a second trip takes
  // E = exp(base): the upper tail is W = E v and f = ln(1 - W) - ln q.  g = x^a y^b / (B I)
  double t = ln_half, arg = ln_half, v = 0.0, base = 0.0, o = 0.5;
  bool by_y = false, second = false;
  int left = MLF_PRIOR_SPECIAL_MAX_STEPS + 1;     // steps left, the first pass counted as one
  int it = 0;
  for (int n = 0; n < 2 * MLF_PRIOR_SPECIAL_MAX_STEPS + 4 && left != 0; ++n) {
    const double e = mlf_psp_exp(arg);
    double larg, g;
    if (!second) {
      o = 1.0 - e;
      const double lo = mlf_psp_ln1m(fmin(e, 0.5));
      const double x = by_y ? o : e, y = by_y ? e : o;
      const double lnpref = a * (by_y ? lo : t) + b * (by_y ? t : lo) - lnB;
      const bool direct = x <= split;
      v = mlf_psp_beta_cf(direct ? a : b, direct ? b : a, direct ? x : y);
      if (!direct) {
        second = true;
        base = 0.0;
        arg = lnpref - lnb;
        continue;
      }
      base = lnpref - lna;
      larg = v;
      g = a / v;
    } else {
      second = false;
      larg = 1.0 - e * v;
      g = b * e / larg;
    }
    if (!(larg > 0.0)) break;
    const double f = base + mlf_psp_log(larg) - lnq;
    if (left > MLF_PRIOR_SPECIAL_MAX_STEPS) {
      left = MLF_PRIOR_SPECIAL_MAX_STEPS;
      by_y = f < 0.0;
      t = fmin(by_y ? ty : tx, ln_half);
      if (!(t == t)) t = ln_half;
      arg = t;
      continue;
    }
    double dt = (by_y ? -f : f) * o / g;
    if (!(dt == dt)) break;
    const double lim = 4.0 + fabs(t);
    dt = fmin(fmax(dt, -lim), lim);
    const double tn = fmin(t - dt, ln_half);
    dt = t - tn;
    t = tn;
    ++it;
    const bool fin = left < 0;
    left = fin ? 0 : left - 1;
    if (!fin && fabs(ldexp(dt, 17)) <= 1.0) {
      t = fmin(ldexp(ldexp(rint(ldexp(t, 24)), -12), -12), ln_half);
      if (left > 0) left = -1;
    }
    arg = t;
  }
  MLF_PRIOR_SPECIAL_NOTE(it);
  s_out = fmin(exp(t), 0.5);
  by_y_out = by_y;
  return t;
}

// Gamma(shape, scale), ChiSquared(k) = Gamma(k / 2, 2) and the columns of a Dirichlet block (scale 1)
__device__ __noinline__ double mlf_prior_gamma(double u, double scale, double a, double inva, double lna, double lg1) {
  const bool upper = u > 0.5;
  const double q = upper ? 1.0 - u : u;
  return scale * exp(mlf_psp_gamma_lnx(log(q), upper, a, inva, lna, lg1));
}

// InverseGamma(shape, scale): the gamma quantile entered from the other tail
__device__ __noinline__ double mlf_prior_invgamma(double u, double scale, double a, double inva, double lna, double lg1) {
  const bool upper = u <= 0.5;
  const double q = upper ? u : 1.0 - u;
  return scale * exp(-mlf_psp_gamma_lnx(log(q), upper, a, inva, lna, lg1));
}

// Beta(a, b) on (0, 1); lnB, lna, lnb from the host
__device__ __noinline__ double mlf_prior_beta(double u, double a, double b, double lnB, double lna, double lnb) {
  const bool flip = u > 0.5;                      // I_y(b, a) = 1 - u: the same problem with a and b exchanged
  const double q = flip ? 1.0 - u : u;
  double s;
  bool by_y;
  mlf_psp_beta_lns(q, log(q), flip ? b : a, flip ? a : b, lnB, flip ? lnb : lna, flip ? lna : lnb, s, by_y);
  return by_y == flip ? s : 1.0 - s;
}

// StudentT(nu, loc, scale); ha = nu / 2, lnB = ln B(nu / 2, 1 / 2), lnha = ln(nu / 2), lnnu = ln nu from the host
__device__ __noinline__ double mlf_prior_studentt(double u, double loc, double scale, double ha, double lnB, double lnha,
                                                  double lnnu) {
  const double ln_half = -0x1.62e42fefa39efp-1;
  const bool flip = u > 0.5;
  const double q = flip ? 1.0 - u : u;
  const double q2 = 2.0 * q;
  if (q2 >= 1.0) return loc + scale * 0.0;
  // else the tail of y: I_y(1/2, nu/2) = 1 - 2 q, exact above 2 q = 1/2.  The seam between the two equations lies at
  // 2 q = 5/8 and not at 1/2, because u = 1/4 and u = 3/4 are values that users pass and both equations hold there
  const bool far = q2 <= 0.625;
  const double r = far ? q2 : 1.0 - q2;
  double s;
  bool by_y;
  const double t = mlf_psp_beta_lns(r, log(r), far ? ha : 0.5, far ? 0.5 : ha, lnB, far ? lnha : ln_half, far ? ln_half : lnha, s,
                                    by_y);
  const double lo = mlf_psp_ln1m(s);
  const bool s_is_y = by_y == far;
  const double lx = s_is_y ? lo : t, ly = s_is_y ? t : lo;
  const double tq = exp(0.5 * (lnnu + ly - lx));
  return loc + scale * (flip ? tq : -tq);
}

#endif  // MLF_PRIORS_SPECIAL_DEV_HPP
