"""The device header of the iterative prior families (ultranest_amd/csrc/mlf_priors_special_dev.hpp) built for the host: a
stand-alone C++ program (tests/special_prior_host.cpp, its own main) defines the three HIP attributes away, includes <cmath>
and the header's text, and evaluates every family over the golden fixture.  -O2 -ffp-contract=off, as the device build forms
no FMA.  Every family must come out inside its bound and below the iteration cap; the same program is built and run once more
under AddressSanitizer and UndefinedBehaviorSanitizer (host code in a program of its own: nothing is preloaded).

This is the check that runs without a GPU.  The device differs from it only by the library's log and exp outside the Newton
loops (inside them the header uses its own): the largest error / bound per family printed here stands beside the device's in
DESIGN.md 7f."""
import re

import numpy as np
import pytest

import special_prior_reference as SR
from ultranest_amd import priors as P

LETTER = {"Gamma": "G", "ChiSquared": "G", "InverseGamma": "I", "Beta": "B", "StudentT": "T", "Dirichlet": "G"}


def cap():
    m = re.search(r"#define MLF_PRIOR_SPECIAL_MAX_STEPS (\d+)", P.special_header_text())
    return int(m.group(1))


def fixture_lines():
    """(lines, [(setting name, first line, number of lines)]) of the whole fixture"""
    lines, spans = [], []
    for family in SR.FAMILY_NAMES:
        for name in SR.settings(family):
            prior, u, _ = SR.load(name)
            mine = SR.host_lines(prior, u)
            spans.append((name, len(lines), len(mine)))
            lines += mine
    return lines, spans


@pytest.fixture(scope="module")
def plain(tmp_path_factory):
    exe = SR.build_host(tmp_path_factory.mktemp("host"), "plain")
    lines, spans = fixture_lines()
    return (lines, spans) + SR.run_host(exe, lines)


def test_every_family_is_inside_its_bound_and_below_the_cap(plain):
    lines, spans, got, steps, most = plain
    worst, count = {}, {}
    for name, first, n in spans:
        prior, u, ref = SR.load(name)
        family = name.split("_")[0]
        e = SR.excess(prior, u, got[first:first + n].reshape(np.shape(u)), ref)
        worst[family] = max(worst.get(family, 0.0), float(e.max()))
        count[family] = max(count.get(family, 0), int(steps[first:first + n].max()))
        assert e.max() <= 1.0, (name, np.ravel(u)[np.argmax(e)], e.max())
    for family in SR.FAMILY_NAMES:
        print("MEASURED host %s: largest error %.3g of the bound, at most %d of %d steps" % (family, worst[family], count[family], cap()))
        assert 0 < count[family] < cap()
    assert max(most.values()) == max(count.values()) and set(most) == set("GIBT")


def test_the_same_program_under_address_and_undefined_behaviour_sanitizers(plain, tmp_path):
    lines, spans, got, steps, most = plain
    exe = SR.build_host(tmp_path, "sanitized", flags=("-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-g"))
    got2, steps2, most2 = SR.run_host(exe, lines)          # a finding ends the program with a non-zero status
    assert np.array_equal(got2, got, equal_nan=True) and np.array_equal(steps2, steps) and most2 == most


def test_the_cap_ends_an_iteration_and_returns_the_iterate(tmp_path):
    """with a cap of 2 steps no call takes more, every result is finite, and the accuracy check exposes it"""
    exe = SR.build_host(tmp_path, "cap2", defines=("MLF_PRIOR_SPECIAL_MAX_STEPS=2",))
    prior, u, ref = SR.load("Gamma_0")
    got, steps, most = SR.run_host(exe, SR.host_lines(prior, u))
    assert steps.max() == 2 and np.isfinite(got).all()
    assert not SR.accepts(prior, u, got, ref)
