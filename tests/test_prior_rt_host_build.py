"""The device header of the run-time priors (ultranest_amd/csrc/mlf_priors_rt_dev.hpp) built for the host: a stand-alone C++
program (tests/prior_rt_host.cpp, its own main) defines the three HIP attributes away, supplies normcdfinv, includes <cmath>
and the header's text, and evaluates its functions over the text fixture tests/golden/g18_prior_rt_host.txt.  -O2
-ffp-contract=off, as the device build forms no FMA.  The run-time families must come out inside the bound of the constant
prior built from the same parameter bits, parameters that a PriorTransform refuses must give NaN, and the table function must
equal its numpy restatement bit for bit at every knot, both neighbours of every knot and both extremes of (0, 1).  The same
program is built and run once more under AddressSanitizer and UndefinedBehaviorSanitizer (host code in a program of its own:
nothing is preloaded); the table lives in a heap block of exactly its size, so a load outside it ends that run.

Fixture lines: ``U|L|N|R u params...`` a run-time family at valid parameters, ``!U ...`` at refused ones, ``l|s|p v`` a guard,
``X n seed kind`` a table of prior_rt_reference.make_table, expanded here into the table and its u values."""
import os
import shutil
import subprocess

import numpy as np
import pytest

import prior_rt_reference as RT
from ultranest_amd import priors as P

HERE = os.path.dirname(os.path.abspath(__file__))
FIXTURE = os.path.join(HERE, "golden", "g18_prior_rt_host.txt")
HOST_SOURCE = os.path.join(HERE, "prior_rt_host.cpp")
FAMILY = {"U": "Uniform", "L": "LogUniform", "N": "TruncatedNormal", "R": "Triangular"}


def build_host(directory, name, flags=()):
    cxx = shutil.which("g++") or shutil.which("c++") or shutil.which("clang++")
    assert cxx, "no host C++ compiler"
    exe = os.path.join(str(directory), name)
    cmd = [cxx, "-std=c++17", "-O2", "-ffp-contract=off", '-DMLF_RT_HEADER="%s"' % P.RT_HEADER] + list(flags) + [HOST_SOURCE, "-o", exe]
    subprocess.run(cmd, check=True, capture_output=True, text=True)
    return exe


def program_input():
    """(input lines, records): a record is (kind, payload, first output line, number of output lines)"""
    lines, records, nout = [], [], 0
    with open(FIXTURE) as fh:
        for raw in fh:
            raw = raw.strip()
            if not raw or raw.startswith("#"):
                continue
            tok = raw.split()
            if tok[0] == "X":
                tab = RT.make_table(int(tok[1]), int(tok[2]), tok[3])
                u = RT.table_u(tab)
                lines.append("T %d %d" % (tab.n, tab.steps))
                lines += [float(v).hex() for v in tab.table]
                lines += ["t %s" % float(v).hex() for v in u]
                records.append(("table", (tab, u, raw), nout, len(u)))
                nout += len(u)
            else:
                lines.append(raw.lstrip("!"))
                records.append(("bad" if raw[0] == "!" else "guard" if tok[0] in "lsp" else "family",
                                (tok[0].lstrip("!"), [float.fromhex(t) for t in tok[1:]]), nout, 1))
                nout += 1
    return lines, records, nout


def run_host(exe, lines, nout):
    out = subprocess.run([exe], input="\n".join(lines) + "\n", capture_output=True, text=True, check=True).stdout.split()
    assert len(out) == nout
    return np.array([float.fromhex(v) for v in out])


def _calls(records, kind):
    """(letter, values, output line) of the one-line records of a kind"""
    return [(payload[0], payload[1], first) for k, payload, first, _ in records if k == kind]


@pytest.fixture(scope="module")
def plain(tmp_path_factory):
    exe = build_host(tmp_path_factory.mktemp("rt_host"), "plain")
    lines, records, nout = program_input()
    return lines, records, run_host(exe, lines, nout)


def test_run_time_families_are_inside_their_bounds(plain):
    lines, records, got = plain
    worst = {}
    for letter, v, first in _calls(records, "family"):
        name = FAMILY[letter]
        e = RT.ref_excess(name, [v[1:]], [v[0]], got[first:first + 1])[0]
        worst[name] = max(worst.get(name, 0.0), e)
        assert e <= 1.0, (name, v, got[first], e)
    assert set(worst) == set(RT.RUN_TIME_FORMS)
    for name in RT.RUN_TIME_FORMS:
        print("MEASURED host rt %s: largest error %.3g of the bound" % (name, worst[name]))


def test_uniform_is_the_numpy_expression_bit_for_bit(plain):
    lines, records, got = plain
    n = 0
    for letter, v, first in _calls(records, "family"):
        if letter == "U":
            assert got[first] == v[1] + v[0] * (v[2] - v[1])
            n += 1
    assert n > 50


def test_refused_parameters_give_nan(plain):
    lines, records, got = plain
    seen = set()
    for letter, v, first in _calls(records, "bad"):
        assert np.isnan(got[first]), (letter, v, got[first])
        seen.add(letter)
    assert seen == set("ULNR")


def test_guards_return_the_value_or_nan(plain):
    lines, records, got = plain
    big = np.finfo(float).max
    rule = {"l": lambda v: abs(v) <= big, "s": lambda v: 0 <= v <= big, "p": lambda v: 0 < v <= big}
    n = 0
    for letter, v, first in _calls(records, "guard"):
        r = got[first]
        if rule[letter](v[0]):
            assert r == v[0] and np.signbit(r) == np.signbit(v[0]), (letter, v)
        else:
            assert np.isnan(r), (letter, v, r)
        n += 1
    assert n == 30


def test_tables_equal_the_numpy_restatement_bit_for_bit(plain):
    lines, records, got = plain
    sizes, worst = [], 0.0
    for kind, payload, first, count in records:
        if kind != "table":
            continue
        tab, u, raw = payload
        mine = got[first:first + count]
        assert np.array_equal(mine, RT.table_restatement(tab, u)), raw
        assert (np.diff(mine) >= 0).all() and mine[0] >= tab.x[0] and mine[-1] <= tab.x[-1], raw
        worst = max(worst, RT.table_excess(tab, u, mine).max())
        sizes.append(tab.n)
    assert set(RT.TABLE_SIZES) <= set(sizes)
    print("MEASURED host table: largest error %.3g of the bound" % worst)
    assert worst <= 1.0


def test_the_same_program_under_address_and_undefined_behaviour_sanitizers(plain, tmp_path):
    lines, records, got = plain
    exe = build_host(tmp_path, "sanitized", flags=("-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-g"))
    got2 = run_host(exe, lines, len(got))          # a finding ends the program with a non-zero status
    assert np.array_equal(got2, got, equal_nan=True)
    # a NaN u, which no route produces, still loads inside the table
    tab = RT.make_table(5, 1)
    extra = ["T %d %d" % (tab.n, tab.steps)] + [float(v).hex() for v in tab.table] + ["t nan", "t 0x0p+0", "t 0x1p+0", "t -0x1p+0", "t 0x1p+1"]
    assert np.isnan(run_host(exe, extra, 5)[0])


def test_a_search_that_runs_one_probe_short_is_caught(tmp_path):
    """the check has teeth: with `steps` one too small the restatement no longer matches"""
    exe = build_host(tmp_path, "plain2")
    tab = RT.make_table(1025, 1)
    u = RT.table_u(tab)
    lines = ["T %d %d" % (tab.n, tab.steps - 1)] + [float(v).hex() for v in tab.table] + ["t %s" % float(v).hex() for v in u]
    assert not np.array_equal(run_host(exe, lines, len(u)), RT.table_restatement(tab, u))
