"""The device header of the warm start (ultranest_amd/csrc/mlf_hotstart_dev.hpp) built for the host: a stand-alone C++ program
(tests/hotstart_host.cpp, its own main) defines the HIP attributes away, includes <cmath> and the header's text and evaluates
form (a) over tables of M = 2 ... 25 knots.  -O2 -ffp-contract=off, as the device build forms no FMA.  Every row must be
decided (none falls in a gap or past the last knot), the umod columns must equal the numpy restatement bit for bit, and the
weight must lie within the derived bound of tests/hotstart_reference.py of the exact sum (mpmath).  The same program is built
and run once more under AddressSanitizer and UndefinedBehaviorSanitizer (host code in a program of its own: nothing is
preloaded); the tail lives in a heap block of exactly its size, so a load outside it ends that run."""
import os
import shutil
import subprocess

import numpy as np
import pytest

import hotstart_reference as HR
from ultranest_amd import hotstart as hs

HERE = os.path.dirname(os.path.abspath(__file__))
HOST_SOURCE = os.path.join(HERE, "hotstart_host.cpp")
KNOTS = tuple(range(2, 26))
DIMS = (1, 3)


def build_host(directory, name, flags=()):
    cxx = shutil.which("g++") or shutil.which("c++") or shutil.which("clang++")
    assert cxx, "no host C++ compiler"
    exe = os.path.join(str(directory), name)
    cmd = [cxx, "-std=c++17", "-O2", "-ffp-contract=off", '-DMLF_HS_HEADER="%s"' % hs.HEADER] + list(flags) + [HOST_SOURCE, "-o", exe]
    subprocess.run(cmd, check=True, capture_output=True, text=True)
    return exe


def rows_of(xp, d, seed):
    """cube rows: t on every knot and on both binary64 neighbours of every knot (inside [0, 1]), t at 2^-53 and 1 - 2^-53, u at
    both extremes, the rest seeded"""
    rs = np.random.RandomState(seed)
    ts = list(xp) + [np.nextafter(x, 2.0) for x in xp[:-1]] + [np.nextafter(x, -1.0) for x in xp[1:]] + [HR.EPS, 1.0 - HR.EPS]
    ts += list(rs.uniform(size=8))
    u = rs.uniform(size=(len(ts), d + 1))
    u[:, d] = ts
    u[0, :d] = HR.EPS
    u[1, :d] = 1.0 - HR.EPS
    return u


def cases():
    out = []
    for M in KNOTS:
        for d in DIMS:
            ulos, uhis, xp = HR.table(M, d, seed=1)
            out.append((M, d, ulos, uhis, xp, rows_of(xp, d, seed=M + d)))
    return out


def program_input(all_cases):
    lines = []
    for M, d, ulos, uhis, xp, u in all_cases:
        tail = hs.contbox_tail(ulos, uhis, xp)
        lines.append("T %d %d" % (len(tail), d))
        lines += [float(v).hex() for v in tail]
        for row in u:
            lines.append("r")
            lines += [float(v).hex() for v in row]
    return lines


def run_host(exe, lines):
    out = subprocess.run([exe], input="\n".join(lines) + "\n", capture_output=True, text=True, check=True).stdout
    return [line.split() for line in out.splitlines()]


@pytest.fixture(scope="module")
def plain(tmp_path_factory):
    all_cases = cases()
    lines = program_input(all_cases)
    exe = build_host(tmp_path_factory.mktemp("hs_host"), "plain")
    return all_cases, lines, run_host(exe, lines)


def _split(all_cases, out):
    first = 0
    for M, d, ulos, uhis, xp, u in all_cases:
        block = out[first:first + len(u)]
        first += len(u)
        j = np.array([int(t[0]) for t in block])
        decided = np.array([t[1] == "1" for t in block])
        vals = np.array([[float.fromhex(v) for v in t[2:]] for t in block])
        yield M, d, ulos, uhis, xp, u, j, decided, vals[:, :d], vals[:, d]
    assert first == len(out)


def test_every_row_is_decided(plain):
    all_cases, lines, out = plain
    seen = set()
    for M, d, ulos, uhis, xp, u, j, decided, umod, weight in _split(all_cases, out):
        want = HR.contbox_restated(u, ulos, uhis, xp)
        assert decided.all() and want[3].all() and np.array_equal(j, want[2]), (M, d)
        assert j.min() == 0 and j.max() == M - 2
        seen.add(M)
    assert seen == set(KNOTS)


@pytest.mark.parametrize("M", KNOTS)
def test_umod_columns_equal_the_restatement_bit_for_bit(plain, M):
    all_cases, lines, out = plain
    n = 0
    for m, d, ulos, uhis, xp, u, j, decided, umod, weight in _split(all_cases, out):
        if m == M:
            assert np.array_equal(umod, HR.contbox_restated(u, ulos, uhis, xp)[0]), (M, d)
            assert np.array_equal(umod, hs.contbox_rows(u, ulos, uhis, xp)[0]), (M, d)          # np.interp itself
            n += 1
    assert n == len(DIMS)


@pytest.mark.parametrize("M", KNOTS)
def test_weight_is_within_the_derived_bound(plain, M):
    all_cases, lines, out = plain
    worst = 0.0
    for m, d, ulos, uhis, xp, u, j, decided, umod, weight in _split(all_cases, out):
        if m == M:
            exact, bound = HR.weight_exact_and_bound(u, ulos, uhis, xp)
            assert np.isfinite(exact).all()
            worst = max(worst, HR.weight_excess(weight, exact, bound).max())
    print("MEASURED host weight M=%d: largest error %.3g of the bound" % (M, worst))
    assert worst <= 1.0


def test_the_same_program_under_address_and_undefined_behaviour_sanitizers(plain, tmp_path):
    all_cases, lines, out = plain
    exe = build_host(tmp_path, "sanitized", flags=("-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-g"))
    assert run_host(exe, lines) == out          # a finding ends the program with a non-zero status
    # a NaN t and values of t outside [0, 1], which no route produces, still load inside the tail
    ulos, uhis, xp = HR.table(25, 2, seed=1)
    tail = hs.contbox_tail(ulos, uhis, xp)
    extra = ["T %d 2" % len(tail)] + [float(v).hex() for v in tail]
    for t in ("nan", "-0x1p+0", "0x1p+1", "inf", "-inf"):
        extra += ["r", "0x1p-1", "0x1p-1", t]
    got = run_host(exe, extra)
    assert len(got) == 5 and got[0][1] == "0"


def test_a_search_with_the_knots_shifted_is_caught(tmp_path, plain):
    """the check has teeth: a tail whose knots are those of another table no longer matches the restatement"""
    all_cases, lines, out = plain
    M, d, ulos, uhis, xp, u = all_cases[-1]
    xp2 = xp.copy()
    xp2[1:-1] = 0.5 * (xp[1:-1] + xp[2:])
    tail = hs.contbox_tail(ulos, uhis, xp2)
    extra = ["T %d %d" % (len(tail), d)] + [float(v).hex() for v in tail]
    for row in u:
        extra += ["r"] + [float(v).hex() for v in row]
    got = run_host(build_host(tmp_path, "plain2"), extra)
    umod = np.array([[float.fromhex(v) for v in t[2:2 + d]] for t in got])
    assert not np.array_equal(umod, HR.contbox_restated(u, ulos, uhis, xp)[0])
