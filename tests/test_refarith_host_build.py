"""The reference arithmetic shared by every route (ultranest_amd/csrc/mlf_refarith_dev.hpp with mlf_tregion_dev.hpp) built for
the host: a stand-alone C++ program (tests/refarith_host.cpp, its own main) defines the HIP attributes away and evaluates the
quadratic form, the band decision and the wrap on the values read from standard input.  -O2 -ffp-contract=off, as the device
build forms no FMA.  The quadratic form must equal numpy's three-operand einsum bit for bit, the band must follow its two
comparisons exactly, and the fast wrap must equal fmod bit for bit.  The same program is built and run once more under
AddressSanitizer and UndefinedBehaviorSanitizer (host code in a program of its own: nothing is preloaded); every operand lives
in a heap block of exactly its size, so a load outside it ends that run."""
import os
import shutil
import subprocess

import numpy as np
import pytest

import ellipsoid_reference as ER

HERE = os.path.dirname(os.path.abspath(__file__))
HOST_SOURCE = os.path.join(HERE, "refarith_host.cpp")
HEADER = os.path.join(os.path.dirname(HERE), "ultranest_amd", "csrc", "mlf_refarith_dev.hpp")
DIMS = (1, 2, 7, 8, 9, 17, 50, 64)      # on both sides of the groups of 8 of the prefetch form
KINDS = ("W", "I")                      # well spread; ill conditioned (kappa_2 about 1e6)
ROWS = 64
ENLARGE = 1.7
NAN = float("nan")
INF = float("inf")


def build_host(directory, name, flags=()):
    cxx = shutil.which("g++") or shutil.which("c++") or shutil.which("clang++")
    assert cxx, "no host C++ compiler"
    exe = os.path.join(str(directory), name)
    cmd = [cxx, "-std=c++17", "-O2", "-ffp-contract=off", '-DMLF_REFARITH_HEADER="%s"' % HEADER] + list(flags) + [HOST_SOURCE, "-o", exe]
    subprocess.run(cmd, check=True, capture_output=True, text=True)
    return exe


def hexes(values):
    return [float(v).hex() for v in np.asarray(values, dtype=float).ravel()]


def same_bits(a, b):
    a, b = np.asarray(a, dtype=float), np.asarray(b, dtype=float)
    return a.shape == b.shape and bool(np.all((a.view(np.uint64) == b.view(np.uint64)) | (np.isnan(a) & np.isnan(b))))


# ------------------------------------------------------------------------------------------------ inputs
def quadform_case(kind, d):
    """centre and inverse covariance of a family of tests/ellipsoid_reference.py; 64 rows: every second one scaled onto
    q = ENLARGE within a few ulp (as test_prep64_proposals_on_the_ellipsoid_boundary_and_wrapped_axes does), the last with a NaN
    coordinate"""
    rs = np.random.RandomState(1000 * d + ord(kind))
    u = ER.family(kind, 7 * d + ord(kind), max(4 * d, 64), d)
    ctr = u.mean(axis=0)
    cov = np.atleast_2d(np.cov(u, rowvar=0))
    inv = np.linalg.inv(cov)
    w, v = np.linalg.eigh(cov)
    dl = (rs.normal(size=(ROWS, d)) * np.sqrt(w)) @ v.T
    q = np.einsum('ij,jk,ik->i', dl, inv, dl)
    scale = np.sqrt(ENLARGE / q)
    scale[1::2] *= 1.0 + rs.uniform(-3e-16, 3e-16, size=len(scale[1::2]))
    rows = ctr + dl * np.where(np.arange(ROWS) % 4 < 2, scale, 1.0)[:, None]
    rows[-1, d // 2] = NAN
    return ctr, inv, rows


def band_case(seed):
    """10^4 pairs (qt, nrm2) around ENLARGE: distances from 2^-52 to 2^-20 relative on both sides, pairs exactly on either
    comparison's edge, NaN in either argument"""
    rs = np.random.RandomState(seed)
    n = 10000
    eps_scale = 2.0 ** -34 * 37.5
    nrm2 = rs.uniform(0.0, 4.0, size=n)
    qt = ENLARGE * (1.0 + rs.choice([-1.0, 1.0], size=n) * 2.0 ** rs.uniform(-52, -20, size=n))
    eps = eps_scale * nrm2
    qt[:500] = ENLARGE - eps[:500]
    qt[500:1000] = ENLARGE + eps[500:1000]
    qt[1000:1100] = ENLARGE
    qt[1100:1150] = NAN
    nrm2[1150:1200] = NAN
    nrm2[1200:1210] = INF
    return eps_scale, qt, nrm2


def wrap_case(seed):
    """(w, shift) with w + shift on 0, 1, 2 and both binary64 neighbours of each, negative sums, sums above 2, signed zeros,
    infinities, NaN, and 10^4 seeded pairs of [0, 1) + [0, 1)"""
    rs = np.random.RandomState(seed)
    pairs = []
    for s in (0.0, 1.0, 2.0):
        for t in (np.nextafter(s, -INF), s, np.nextafter(s, INF)):
            pairs += [(t, 0.0), (0.0, t), (t - 0.5, 0.5), (0.25, t - 0.25)]
    pairs += [(0.0, 0.0), (-0.0, -0.0), (-0.0, 0.0), (0.5, -0.5), (-1.0, 0.0), (-0.25, 0.0), (-3.75, 0.5), (-1e300, 0.5),
              (2.5, 0.75), (7.0, 0.0), (1e17, 0.5), (1e300, 0.25), (INF, 0.5), (-INF, 0.5), (0.5, INF), (NAN, 0.5),
              (5e-324, 0.0), (-5e-324, 0.0), (1.0 - 2.0 ** -53, 2.0 ** -54)]
    w = rs.uniform(size=10000)
    sh = rs.uniform(size=10000)
    return np.concatenate([np.array(pairs), np.stack([w, sh], axis=1)])


def program_input():
    lines, quad = [], []
    for kind in KINDS:
        for d in DIMS:
            ctr, inv, rows = quadform_case(kind, d)
            quad.append((kind, d, ctr, inv, rows))
            lines += ["Q %d %d" % (d, len(rows))] + hexes(ctr) + hexes(inv) + hexes(rows)
    eps_scale, qt, nrm2 = band_case(5)
    for chol_ok in (1, 0):
        lines += ["B %d %d" % (chol_ok, len(qt)), float(eps_scale).hex(), float(ENLARGE).hex()] + hexes(np.stack([qt, nrm2], axis=1))
    wraps = wrap_case(6)
    lines += ["W %d" % len(wraps)] + hexes(wraps)
    return lines, quad, (eps_scale, qt, nrm2), wraps


def run_host(exe, lines):
    out = subprocess.run([exe], input="\n".join(lines) + "\n", capture_output=True, text=True, check=True).stdout
    return [line.split() for line in out.splitlines()]


@pytest.fixture(scope="module")
def plain(tmp_path_factory):
    lines, quad, band, wraps = program_input()
    exe = build_host(tmp_path_factory.mktemp("refarith_host"), "plain")
    out = run_host(exe, lines)
    nq = len(quad) * ROWS
    nb = len(band[1])
    assert len(out) == nq + 2 * nb + len(wraps)
    q_out = np.array([[float.fromhex(v) for v in t] for t in out[:nq]]).reshape(len(quad), ROWS, 3)
    b_out = np.array([int(t[0]) for t in out[nq:nq + 2 * nb]]).reshape(2, nb)
    w_out = np.array([[float.fromhex(v) for v in t] for t in out[nq + 2 * nb:]])
    return dict(lines=lines, out=out, quad=quad, band=band, wraps=wraps, q_out=q_out, b_out=b_out, w_out=w_out)


# ------------------------------------------------------------------------------------------------ checks
@pytest.mark.parametrize("d", DIMS)
@pytest.mark.parametrize("kind", KINDS)
def test_quadratic_form_equals_numpy_einsum_bit_for_bit(plain, kind, d):
    (i, (_, _, ctr, inv, rows)), = [(i, c) for i, c in enumerate(plain["quad"]) if c[0] == kind and c[1] == d]
    dl = rows - ctr
    want = np.einsum('ij,jk,ik->i', dl, inv, dl)
    # the inputs do what they are there for: rows on the boundary (up to the rounding of the rows themselves), a NaN row
    assert np.isnan(want[-1]) and np.isfinite(want[:-1]).all()
    on = np.arange(ROWS - 1) % 4 < 2
    assert (np.abs(want[:-1][on] - ENLARGE) <= 1e-6 * ENLARGE).all()
    assert (np.abs(want[:-1][~on] - ENLARGE) > 1e-6 * ENLARGE).any()
    got = plain["q_out"][i]
    assert same_bits(got[:, 0], want), "mlf_tregion_q<0>"
    assert same_bits(got[:, 1], want), "mlf_tregion_q<KN>"
    assert same_bits(got[:, 2], want), "mlf_ell_q_row"
    assert np.isnan(got[-1]).all()


def test_band_follows_its_two_comparisons(plain):
    eps_scale, qt, nrm2 = plain["band"]
    with np.errstate(invalid="ignore"):
        eps = eps_scale * nrm2
        sure_in = qt + eps < ENLARGE
        sure_out = qt - eps > ENLARGE
    assert sure_in.sum() > 1000 and sure_out.sum() > 1000 and (~sure_in & ~sure_out).sum() > 1000
    got = plain["b_out"][0]
    assert np.array_equal(got == 1, sure_in)
    assert np.array_equal(got == -1, sure_out)
    assert np.isin(got, (-1, 0, 1)).all()
    assert (got[np.isnan(qt) | np.isnan(nrm2)] == 0).all() and (np.isnan(qt) | np.isnan(nrm2)).sum() == 100
    assert (plain["b_out"][1] == 0).all()      # chol_ok == 0: everything is undecided


def test_fast_wrap_equals_the_plain_wrap_bit_for_bit(plain):
    wraps, got = plain["wraps"], plain["w_out"]
    with np.errstate(invalid="ignore"):
        s = wraps[:, 0] + wraps[:, 1]
        want = np.fmod(s, 1.0)
    for lo, hi in ((-INF, 0.0), (0.0, 1.0), (1.0, 2.0), (2.0, INF)):      # every branch of the fast form is taken
        assert ((s >= lo) & (s < hi)).sum() >= 5
    assert same_bits(got[:, 0], want)
    assert same_bits(got[:, 1], got[:, 0])


def test_the_same_program_under_address_and_undefined_behaviour_sanitizers(plain, tmp_path):
    exe = build_host(tmp_path, "sanitized", flags=("-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-g"))
    assert run_host(exe, plain["lines"]) == plain["out"]          # a finding ends the program with a non-zero status
