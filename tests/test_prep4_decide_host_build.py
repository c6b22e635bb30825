"""The decisions of the bounded per-proposal stage (ultranest_amd/csrc/mlf_prep4_dev.hpp: prep4_uniform, prep4_ell_decide,
prep4_route with both threshold forms of mlf_filter_dev.hpp) built for the host: a stand-alone C++ program
(tests/prep4_decide_host.cpp, its own main) defines the HIP attributes away and evaluates the header's functions on the values
read from standard input.  -O2 -ffp-contract=off, as the device build forms no FMA.  Every output must equal, bit for bit, the
numpy float32 restatements whose soundness tests/test_prep4_bounds.py and tests/test_filter_residue_bounds.py prove
(ellipsoid_decision_tail, thresholds4, thresholds4r), so the three kernels that call the header -- k_prep4, k_prep_sweep,
k_inside_mid -- decide by the arithmetic those tests are about.  The same program is built and run once more under
AddressSanitizer and UndefinedBehaviorSanitizer (host code in a program of its own: nothing is preloaded)."""
import os
import shutil
import subprocess
from fractions import Fraction

import numpy as np
import pytest

from test_filter_residue_bounds import thresholds4r
from test_prep4_bounds import DN, UP, EllSetup, dn32, ellipsoid_decision_tail, f32, thresholds4, up32

HERE = os.path.dirname(os.path.abspath(__file__))
HOST_SOURCE = os.path.join(HERE, "prep4_decide_host.cpp")
HEADER = os.path.join(os.path.dirname(HERE), "ultranest_amd", "csrc", "mlf_prep4_dev.hpp")
NAN = float("nan")
INF = float("inf")
CONST_KEYS = ("g", "y0n", "lf", "el", "l_abs", "s0n", "eps_scale", "enl_lo", "enl_hi", "zt", "zt_abs", "s_x", "inv_sx", "inv_sl_sx",
              "inv_st_sx")                                  # the order of Prep4Consts
ELL_DIMS = (2, 50, 64)
FORMS = (("worst", 0, 16), ("worst", 0, 64), ("measured", 1, 16), ("measured", 1, 64), ("measured", 1, 80))


def build_host(directory, name, flags=()):
    cxx = shutil.which("g++") or shutil.which("c++") or shutil.which("clang++")
    assert cxx, "no host C++ compiler"
    exe = os.path.join(str(directory), name)
    cmd = [cxx, "-std=c++17", "-O2", "-ffp-contract=off", '-DMLF_PREP4_HEADER="%s"' % HEADER] + list(flags) + [HOST_SOURCE, "-o", exe]
    subprocess.run(cmd, check=True, capture_output=True, text=True)
    return exe


def hexline(values):
    return " ".join(float(v).hex() for v in values)


def bits32(a):
    return np.asarray(a, dtype=np.float32).view(np.uint32)


def same_bits32(a, b):
    a, b = np.asarray(a, dtype=np.float32), np.asarray(b, dtype=np.float32)
    return a.shape == b.shape and bool(np.all((bits32(a) == bits32(b)) | (np.isnan(a) & np.isnan(b))))


def f32_of_fraction(q):
    """round-to-nearest-even binary32 value of a rational number"""
    if q == 0:
        return f32(0)
    sign, q = (-1, -q) if q < 0 else (1, q)
    e = q.numerator.bit_length() - q.denominator.bit_length()
    if Fraction(2) ** e > q:
        e -= 1                                             # 2^e <= q < 2^(e + 1)
    e = max(e, -126)
    m = q / Fraction(2) ** (e - 23)
    n, r = divmod(m.numerator, m.denominator)
    r = Fraction(r, m.denominator)
    if r > Fraction(1, 2) or (r == Fraction(1, 2) and n & 1):
        n += 1
    return f32(sign * float(np.ldexp(float(n), e - 23)))


def fma32(a, b, c):
    """fmaf: one rounding of the exact a b + c"""
    return f32_of_fraction(Fraction(float(a)) * Fraction(float(b)) + Fraction(float(c)))


# ------------------------------------------------------------------------------------------------ restatements written here
def uniform(c, stats, r2, csl, sigma, dp, quant):
    """float32 restatement of prep4_uniform from stats, r2, csl and the constants"""
    ks = (dp + 6 + 15) // 16
    sig_ok = bool(sigma >= 2.0**-60 and sigma <= 2.0**60)
    sig_f = f32(sigma) if sig_ok else f32(1)
    z = f32(0)
    u = dict(sig_ok=sig_ok, sig_f=sig_f, sqrt_k=np.sqrt(f32(16 * ks)), namax=z, ea_max=z, zeta_scale=z, zeta0=z, kappa=z, sr_lo=z,
             sr_hi=z)
    if quant:
        u["namax"] = f32(stats[1]) * UP
        u["ea_max"] = f32(stats[4]) * UP + f32(2.0**-100)
        cs2 = f32(0)
        for v in csl:
            cs2 = fma32(v, v, cs2)
        csn = f32(0.5) * np.sqrt(cs2) * UP
        u["zeta_scale"] = sig_f * c["zt"] * UP
        u["zeta0"] = (c["g"] * csn + sig_f * c["zt_abs"]) * UP + f32(2.0**-100)
        u["kappa"] = f32(-2) * sig_f * c["inv_st_sx"]
        with np.errstate(invalid="ignore"):
            sr = np.float64(sigma) * np.sqrt(np.float64(r2))
        u["sr_lo"] = f32(sr * (1.0 - 2.0**-30)) * DN
        u["sr_hi"] = f32(sr * (1.0 + 2.0**-30)) * UP
    u["inv_sx2"] = c["inv_sx"] * c["inv_sx"]
    u["inv_slsx2"] = c["inv_sl_sx"] * c["inv_sl_sx"]
    return u


UNIFORM_FIELDS = ("sig_f", "sqrt_k", "namax", "ea_max", "zeta_scale", "zeta0", "kappa", "sr_lo", "sr_hi", "inv_sx2", "inv_slsx2")


def route(form, K, t):
    """prep4_route: the route byte, then zeta and eb, then the threshold form's restatement; returns (route, lo, hi, cause)"""
    sig_ok, namax, ea_max, zeta_scale, zeta0, sqrt_k, sr_lo, sr_hi, ins_any, nb, dnorm, eb2 = (f32(v) for v in t)
    if not ins_any:
        return 0, -1.0, -1.0, "outside"
    if not sig_ok:
        return 2, -1.0, -1.0, "sigma"
    if not nb <= f32(29000):
        return 2, -1.0, -1.0, "nb"
    with np.errstate(invalid="ignore", over="ignore"):
        zeta = (zeta_scale * dnorm + zeta0) * UP
        if form == "measured":
            eb = f32(0.5) * np.sqrt(eb2) * UP + f32(2.0**-60)
            lo, hi, ok = thresholds4r(ea_max, eb, namax, nb, zeta, sqrt_k, sr_lo, sr_hi, K)
        else:
            lo, hi, ok = thresholds4(namax, nb, zeta, sqrt_k, sr_lo, sr_hi)
    if not ok:
        return 2, -1.0, -1.0, "t_hi"
    return 1, lo, hi, "filter"


# ------------------------------------------------------------------------------------------------ inputs
def ell_consts(d):
    """the constants of tests/test_prep4_bounds.py's EllSetup for one region, with the fields the decisions do not read made up"""
    rs = np.random.RandomState(40 + d)
    Q, _ = np.linalg.qr(rs.normal(size=(d, d)))
    A = np.linalg.inv((Q * (np.geomspace(1.0, 9.0, d) * 1e-3)) @ Q.T)
    A = 0.5 * (A + A.T)
    L = np.linalg.cholesky(A)
    c_ell = 0.5 + 0.01 * rs.normal(size=d)
    c_lay = c_ell + 1e-3 * rs.normal(size=d)
    es = EllSetup(L, A, c_ell, c_lay, 0.12)
    enlarge = 1.3 * d
    c = dict(es.consts)
    c.update(enl_lo=dn32(enlarge), enl_hi=up32(enlarge), zt=up32(float(es.g) * 31.0 + 2.0**-20), zt_abs=up32(31.0 * 8 * 2.0**-25 / es.sx),
             s_x=f32(es.sx), inv_sx=f32(1.0 / es.sx), inv_sl_sx=f32(1.0 / (es.sl * es.sx)), inv_st_sx=f32(2.0**-11 / es.sx))
    return c, enlarge


def crossing(verdict, dn2):
    """per dn2 the smallest positive binary32 qs (as a bit pattern) at which the monotone verdict(qs, dn2) is true"""
    lo = np.zeros(len(dn2), dtype=np.uint32)
    hi = np.full(len(dn2), f32(1e30).view(np.uint32), dtype=np.uint32)
    assert not verdict(lo.view(np.float32), dn2).any() and verdict(hi.view(np.float32), dn2).all()
    while (hi - lo > 1).any():
        mid = lo + (hi - lo) // 2
        up = verdict(mid.view(np.float32), dn2)
        hi = np.where(up, mid, hi)
        lo = np.where(up, lo, mid)
    return hi


def ell_case(d):
    """(qs, dn2): 2 x 4000 pairs within 2^-24 ... 2^-10 relative of the two comparison edges on both sides, the six binary32
    values around each edge (the comparison itself flips between two of them), lo <= 0, zeros, NaN / inf in either argument,
    values above 3e38, and pairs far from the boundary"""
    c, enlarge = ell_consts(d)
    rs = np.random.RandomState(d)
    n = 4000
    dn2 = (rs.uniform(0.02, 0.3, size=n) ** 2).astype(np.float32)
    not_in = lambda qs, x: ~ellipsoid_decision_tail(qs, x, c, enlarge)[0]
    is_out = lambda qs, x: ellipsoid_decision_tail(qs, x, c, enlarge)[1]
    e_in, e_out = crossing(not_in, dn2), crossing(is_out, dn2)
    pairs = []
    for edge in (e_in, e_out):
        q = edge.view(np.float32).astype(np.float64)
        rel = rs.choice([-1.0, 1.0], size=n) * 2.0 ** rs.uniform(-24, -10, size=n)
        pairs.append(np.stack([(q * (1.0 + rel)).astype(np.float32), dn2], axis=1))
        for k in (-3, -2, -1, 0, 1, 2):
            pairs.append(np.stack([(edge[:300].astype(np.int64) + k).astype(np.uint32).view(np.float32), dn2[:300]], axis=1))
    small = (rs.uniform(0.0, 1e-9, size=200)).astype(np.float32)          # sqrt(qs) below eta: lo <= 0
    far = np.stack([(enlarge * rs.uniform(0.0, 4.0, size=400)).astype(np.float32), dn2[:400]], axis=1)
    special = [(0.0, 0.0), (0.0, 0.01), (enlarge, 0.0), (NAN, 0.01), (enlarge, NAN), (NAN, NAN), (INF, 0.01), (enlarge, INF), (INF, INF),
               (3.1e38, 0.01), (enlarge, 3.2e38), (3.0e38, 0.01), (-1.0, 0.01), (enlarge, -1.0), (-0.0, -0.0), (2.0**-140, 2.0**-140), (3.3e38, 3.3e38), (NAN, INF)]
    pairs += [np.stack([small, dn2[:200]], axis=1), far, np.array(special, dtype=np.float32)]
    return c, enlarge, np.concatenate(pairs).astype(np.float32), (e_in, e_out, dn2)


def route_case(seed, K):
    """5000 tuples per (form, K): sigma-scaled operands as the kernels see them, sr so that T_hi lies on either side of 30000
    and so that the lower edge is negative, nb on either side of 29000, an unusable sigma, proposals outside the ellipsoid,
    NaN in every argument"""
    rs = np.random.RandomState(seed)
    n = 5000
    t = np.zeros((n, 12))
    t[:, 0] = 1.0
    t[:, 1] = rs.uniform(0.3, 2.0, size=n)                       # namax
    t[:, 2] = 2.0 ** rs.uniform(-14, -9, size=n)                 # ea_max
    t[:, 3] = 2.0 ** rs.uniform(-20, -12, size=n)                # zeta_scale
    t[:, 4] = 2.0 ** rs.uniform(-24, -14, size=n)                # zeta0
    t[:, 5] = np.sqrt(f32(K))
    sr = rs.uniform(0.01, 1.5, size=n)
    t[:, 8] = 1.0
    t[:, 9] = rs.uniform(0.0, 2.0, size=n) ** 2                  # nb
    t[:, 10] = rs.uniform(0.0, 0.5, size=n)                      # dnorm
    t[:, 11] = (2.0 ** rs.uniform(-13, -9, size=n)) ** 2 * 4.0   # eb2
    sr[200:500] = rs.uniform(172.0, 174.5, size=300)             # T_hi around 30000 ...
    sr[500:520] = [np.sqrt(30000.0) * (1 + k * 2.0**-22) for k in range(-10, 10)]
    t[500:520, 2:5] = 0.0
    sr[520:700] = 2.0 ** rs.uniform(-16, -8, size=180)           # ... and lo <= 0, or lo^2 below Eacc: -inf
    nb_edge = np.nextafter(f32(29000), f32(0))
    t[700:709, 9] = [29000.0, nb_edge, np.nextafter(f32(29000), f32(INF)), 28999.0, 29001.0, 6e4, INF, NAN, 3e38]
    sr[700:709] = 1.0
    t[709:800, 9] = rs.uniform(28000.0, 30000.0, size=91)
    t[800:830, 0] = 0.0                                          # sigma unusable
    t[830:900, 8] = 0.0                                          # outside the ellipsoid for certain
    for k, col in enumerate((1, 2, 3, 4, 10, 11)):
        t[900 + k, col] = NAN
        t[910 + k, col] = INF
    t[:, 6] = [dn32(v * (1 - 2.0**-30)) * DN for v in sr]
    t[:, 7] = [up32(v * (1 + 2.0**-30)) * UP for v in sr]
    t[920, 6:8] = NAN
    t[921, 7] = INF
    return t.astype(np.float32)


def uniform_cases():
    out = []
    for i, (dp, quant, sigma, r2) in enumerate([(2, 1, 2.0**-3, 0.37), (8, 1, 1.0, 2.5e-3), (50, 1, 2.0**-1, 41.0), (50, 0, 1.0, 0.0),
                                                (64, 1, 2.0**5, 1e-8), (50, 1, 2.0**-61, 1.0), (50, 1, NAN, 1.0), (22, 1, 2.0**61, 1.0),
                                                (50, 1, 0.25, NAN)]):
        rs = np.random.RandomState(70 + i)
        c = ell_consts(50)[0]
        nt = ((dp + 6 + 15) // 16 + 1) // 2
        stats = np.array([sigma, rs.uniform(0.5, 2.0), 0.0, 0.0, 2.0 ** rs.uniform(-14, -9)])
        csl = (2.0 * sigma * 0.01 * rs.normal(size=32 * nt)).astype(np.float32) if np.isfinite(sigma) else np.zeros(32 * nt, np.float32)
        csl[rs.randint(32 * nt, size=4)] = 0.0
        out.append((dp, quant, c, stats, r2, csl, sigma))
    return out


def program_input():
    lines = []
    uni = uniform_cases()
    for dp, quant, c, stats, r2, csl, sigma in uni:
        lines += ["U %d %d" % (dp, quant), hexline([c[k] for k in CONST_KEYS] + list(stats) + [r2, sigma]), hexline(csl)]
    ell = [ell_case(d) for d in ELL_DIMS]
    for c, _, pairs, _ in ell:
        lines += ["E %d" % len(pairs), hexline(c[k] for k in CONST_KEYS)] + [hexline(p) for p in pairs]
    routes = [route_case(900 + i, K) for i, (_, _, K) in enumerate(FORMS)]
    for (_, form, K), t in zip(FORMS, routes):
        lines += ["R %d %d %d" % (form, K // 16, len(t))] + [hexline(row) for row in t]
    return lines, uni, ell, routes


def run_host(exe, lines):
    out = subprocess.run([exe], input="\n".join(lines) + "\n", capture_output=True, text=True, check=True).stdout
    return [line.split() for line in out.splitlines()]


@pytest.fixture(scope="module")
def plain(tmp_path_factory):
    lines, uni, ell, routes = program_input()
    exe = build_host(tmp_path_factory.mktemp("prep4_decide_host"), "plain")
    out = run_host(exe, lines)
    nu, ne = len(uni), [len(e[2]) for e in ell]
    assert len(out) == nu + sum(ne) + sum(len(t) for t in routes)
    pos = nu
    ell_out = []
    for n in ne:
        ell_out.append(out[pos:pos + n])
        pos += n
    route_out = []
    for t in routes:
        route_out.append(out[pos:pos + len(t)])
        pos += len(t)
    return dict(lines=lines, out=out, uni=uni, uni_out=out[:nu], ell=ell, ell_out=ell_out, routes=routes, route_out=route_out)


# ------------------------------------------------------------------------------------------------ checks
def test_uniform_quantities_equal_the_numpy_restatement_bit_for_bit(plain):
    seen_ok = set()
    for (dp, quant, c, stats, r2, csl, sigma), got in zip(plain["uni"], plain["uni_out"]):
        want = uniform(c, stats, r2, csl, sigma, dp, bool(quant))
        assert int(got[0]) == int(want["sig_ok"])
        assert same_bits32([float.fromhex(v) for v in got[1:]], [want[k] for k in UNIFORM_FIELDS]), (dp, quant, sigma, got, want)
        seen_ok.add((bool(quant), want["sig_ok"]))
        if not quant:
            assert not any(float(want[k]) for k in ("namax", "ea_max", "zeta_scale", "zeta0", "kappa", "sr_lo", "sr_hi"))
    assert seen_ok == {(True, True), (True, False), (False, True)}


@pytest.mark.parametrize("d", ELL_DIMS)
def test_ellipsoid_decision_equals_the_numpy_restatement_bit_for_bit(plain, d):
    i = ELL_DIMS.index(d)
    c, enlarge, pairs, (e_in, e_out, dn2) = plain["ell"][i]
    assert len(pairs) >= 10000
    got = plain["ell_out"][i]
    sure_in, sure_out, dnorm, _ = ellipsoid_decision_tail(pairs[:, 0], pairs[:, 1], c, enlarge)
    assert np.array_equal(np.array([int(g[0]) for g in got]), sure_in.astype(int))
    assert np.array_equal(np.array([int(g[1]) for g in got]), sure_out.astype(int))
    assert same_bits32([float.fromhex(g[2]) for g in got], dnorm)
    # every branch is taken, and the inputs sit where they are meant to
    band = ~sure_in & ~sure_out
    assert not (sure_in & sure_out).any()
    assert sure_in.sum() > 2000 and sure_out.sum() > 2000 and band.sum() > 2000
    with np.errstate(invalid="ignore"):
        odd = ~(pairs[:, 0] < f32(3e38)) | ~(pairs[:, 1] < f32(3e38))
    assert odd.sum() >= 10 and band[odd].all()                                  # NaN, inf, above 3e38: the band
    for edge, verdict in ((e_in, sure_in), (e_out, sure_out)):                  # the comparison flips between two neighbours
        at = ellipsoid_decision_tail(edge.view(np.float32), dn2, c, enlarge)
        below = ellipsoid_decision_tail((edge - 1).view(np.float32), dn2, c, enlarge)
        k = 0 if verdict is sure_in else 1
        assert (at[k] != below[k]).all()
        near = pairs[5800 * k:5800 * k + 4000, 0].astype(np.float64) / edge.view(np.float32) - 1.0
        assert (np.abs(near) <= 2.0**-10 * (1 + 1e-6)).all() and (near > 0).sum() > 1000 and (near < 0).sum() > 1000
    tiny = pairs[:, 0] <= f32(1e-9)
    assert tiny.sum() >= 200 and not sure_out[tiny].any()                       # lo <= 0: never outside for certain


@pytest.mark.parametrize("name,form,K", FORMS)
def test_route_and_thresholds_equal_the_numpy_restatements_bit_for_bit(plain, name, form, K):
    i = FORMS.index((name, form, K))
    t, got = plain["routes"][i], plain["route_out"][i]
    causes = {}
    neg_inf = 0
    asked = int(plain["route_out"][i - 1][-1][3]) if i else 0      # the program's running count before this block
    for row, g in zip(t, got):
        rt, lo, hi, cause = route(name, K, row)
        assert int(g[0]) == rt, (row, g, cause)
        asked += int(name == "measured" and cause in ("filter", "t_hi"))      # only where the thresholds are formed
        assert int(g[3]) == asked, (row, g, cause)
        assert same_bits32([float.fromhex(g[1]), float.fromhex(g[2])], [lo, hi]), (row, g, lo, hi)
        causes[cause] = causes.get(cause, 0) + 1
        neg_inf += int(rt == 1 and lo == -INF)
        if rt != 1:
            assert lo == -1.0 and hi == -1.0
        else:
            assert hi < 30000.0 and (lo == -INF or lo >= 0.0)
    # every branch: outside, the pre-filter, the exact scan by each of its causes, a lower threshold of -inf
    assert causes["outside"] >= 70 and causes["sigma"] >= 30 and causes["nb"] >= 20 and causes["t_hi"] >= 50
    assert causes["filter"] > 3000 and neg_inf >= 50 and causes["filter"] - neg_inf > 2500
    edge = t[700:703]
    assert [route(name, K, row)[3] for row in edge] == ["filter", "filter", "nb"]       # 29000 and its neighbours


def test_at_least_ten_thousand_route_tuples_per_threshold_form(plain):
    for name in ("worst", "measured"):
        assert sum(len(t) for f, t in zip(FORMS, plain["routes"]) if f[0] == name) >= 10000


def test_the_same_program_under_address_and_undefined_behaviour_sanitizers(plain, tmp_path):
    exe = build_host(tmp_path, "sanitized", flags=("-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-g"))
    assert run_host(exe, plain["lines"]) == plain["out"]          # a finding ends the program with a non-zero status
