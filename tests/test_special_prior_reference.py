"""The reference of the iterative prior families (tests/special_prior_reference.py) and its golden fixture, without a GPU:
every stored root is checked by a round trip at 60 digits, the bounds accept the binary64 stand-ins that are known to hold them
and reject a set of seeded defects, each of which an implementation of these quantile functions can have."""
import mpmath as mp
import numpy as np
import pytest

import special_prior_reference as SR
from ultranest_amd import priors as P


def _sc():
    """scipy.special, imported at first use: importing scipy loads a BLAS pool of its own, which the tests of the BLAS scope
    (collected in the same process) must not find changed by the collection of this module"""
    from scipy import special
    return special


ALL = [name for family in SR.FAMILY_NAMES for name in SR.settings(family)]
FIXED = np.setdiff1d(SR.grid(), np.random.RandomState(17).uniform(size=64))          # the 18 fixed points


def test_the_fixture_holds_every_setting_on_the_stated_grid():
    assert len(ALL) == 27 and len(FIXED) == 18
    for name in ALL:
        prior, u, ref = SR.load(name)
        if isinstance(prior, P.Dirichlet):
            assert u.shape == (20, prior.size) and np.array_equal(u, SR.block_grid(prior.size))
        else:
            assert np.array_equal(u, SR.grid()) and len(u) == 82 and len(ref) == 82
        assert u.min() == 2.0 ** -1022 and u.max() == 1 - 2.0 ** -53


@pytest.mark.parametrize("name", ALL)
def test_round_trip_at_60_digits(name):
    """CDF(reference) from the smaller tail is that tail's probability to 1e-30 relative; a root below 2^-1074 is stored as
    what it is, and its rounding to binary64 is 0"""
    prior, u, ref = SR.load(name)
    worst, zeros = mp.mpf(0), 0
    with mp.workdps(SR.DPS):
        if isinstance(prior, P.Dirichlet):
            cases = [(g, x, r) for row_u, row_r in zip(u, ref) for g, x, r in zip(prior.gammas(), row_u, row_r)]
        else:
            cases = [(prior, x, r) for x, r in zip(u, ref)]
        for pr, x, r in cases:
            tail, q = SR.tail_probability(pr, x, r)
            worst = max(worst, abs(tail - q) / q)
            v = SR.value(pr, r)
            if 0 < v < mp.mpf(2) ** -1075:
                zeros += 1
                assert float(v) == 0.0
    assert worst < mp.mpf(10) ** -30, worst
    if name in ("Gamma_0", "ChiSquared_0", "Beta_0", "Beta_5", "Dirichlet_64"):
        assert zeros > 0          # the small shapes reach below the smallest subnormal


def _short_reference(prior):
    return SR.reference(prior, FIXED)


def _gamma_standin(a, scale, u):
    lower = u <= 0.5
    return scale * np.where(lower, _sc().gammaincinv(a, np.where(lower, u, 0.5)), _sc().gammainccinv(a, np.where(lower, 0.5, 1.0 - u)))


@pytest.mark.parametrize("shape", [0.1, 0.5, 1.0, 2.5, 30.0, 1000.0])
def test_scipy_gamma_stand_in_is_accepted(shape):
    prior = P.Gamma(shape, 1.0)
    e = SR.excess(prior, FIXED, _gamma_standin(shape, 1.0, FIXED), _short_reference(prior))
    print("gammaincinv / gammainccinv, shape %g: %.3g of the bound" % (shape, e.max()))
    assert e.max() <= 1.0


@pytest.mark.parametrize("ab", [(0.5, 0.5), (1.0, 3.0), (2.5, 40.0), (30.0, 1000.0), (1000.0, 1000.0)])
def test_scipy_beta_stand_in_is_accepted(ab):
    """(the scipy at hand returns NaN for (2.5, 40) at u = 2^-1022 and 1e-300, where the root is 1e-124 and 1e-121: a
    non-finite result is rejected, and the stand-in is held to the bound at the sixteen points where it gives a number)"""
    prior = P.Beta(*ab)
    got = _sc().betaincinv(ab[0], ab[1], FIXED)
    e = SR.excess(prior, FIXED, got, _short_reference(prior))
    finite = np.isfinite(got)
    print("betaincinv %r: %.3g of the bound at %d of %d points" % (ab, e[finite].max(), finite.sum(), len(FIXED)))
    assert e[finite].max() <= 1.0 and finite.sum() >= 16 and finite[2:].all()
    assert np.isinf(e[~finite]).all()


def _t_by_the_beta_route(nu, u, carry_log=False):
    """t = -sqrt(nu y / x), x = I^-1_(2q)(nu / 2, 1 / 2), y from the complementary call when x > 0.5"""
    out = []
    for v in u:
        q = min(v, 1.0 - v)
        if q == 0.5:
            out.append(0.0)
            continue
        x = _sc().betaincinv(0.5 * nu, 0.5, 2.0 * q)
        y = _sc().betaincinv(0.5, 0.5 * nu, 1.0 - 2.0 * q) if x > 0.5 else 1.0 - x
        if x > 0.5:
            x = 1.0 - y
        with np.errstate(all="ignore"):
            t = np.sqrt(nu * y / x)
        out.append(t if v > 0.5 else -t)
    return np.array(out)


@pytest.mark.parametrize("nu", [2.5, 30.0])
def test_textbook_student_t_route_is_accepted(nu):
    prior = P.StudentT(nu)
    e = SR.excess(prior, FIXED, _t_by_the_beta_route(nu, FIXED), _short_reference(prior))
    print("t = -sqrt(nu y / x), nu %g: %.3g of the bound" % (nu, e.max()))
    assert e.max() <= 1.0


# ---- seeded defects ------------------------------------------------------------------------------------------------

def test_stdtrit_is_rejected_at_nu_1():
    prior = P.StudentT(1.0)
    u = np.array([0.25])
    e = SR.excess(prior, u, _sc().stdtrit(1.0, u), SR.reference(prior, u))
    print("stdtrit(1, 0.25): %.3g of the bound" % e.max())
    assert e.max() > 1.0


def test_betaincinv_is_rejected_in_the_far_tail_of_a_small_shape():
    prior = P.Beta(0.1, 0.1)
    u = np.array([1e-100])
    got = _sc().betaincinv(0.1, 0.1, u)
    ref = SR.reference(prior, u)
    assert ref[0][0] < mp.mpf(2) ** -1074 and got[0] > 0        # the exact quantile is below the smallest subnormal
    assert not SR.accepts(prior, u, got, ref)
    assert SR.accepts(prior, u, np.zeros(1), ref)               # 0, what exp(ln x) underflows to, is the correct rounding


def test_the_beta_route_without_ln_x_is_rejected_at_nu_1():
    prior = P.StudentT(1.0)
    u = np.array([1e-300])
    got = _t_by_the_beta_route(1.0, u)                          # x = O(q^2) has underflowed
    assert not SR.accepts(prior, u, got, SR.reference(prior, u))


@pytest.fixture(scope="module")
def counted(tmp_path_factory):
    """per one-column setting: (prior, u, ref, results of the header's host build, steps per call)"""
    exe = SR.build_host(tmp_path_factory.mktemp("ref_host"), "counted")
    out = {}
    for name in ALL:
        prior, u, ref = SR.load(name)
        if not isinstance(prior, P.Dirichlet):
            got, steps, _ = SR.run_host(exe, SR.host_lines(prior, u))
            out[name] = (prior, u, ref, got, steps)
    return out


def test_the_starting_approximation_alone_is_rejected(counted, tmp_path):
    exe = SR.build_host(tmp_path, "start", defines=("MLF_PRIOR_SPECIAL_MAX_STEPS=0",))
    for name in ("Gamma_1", "InverseGamma_1", "Beta_3", "StudentT_4"):
        prior, u, ref, got, steps = counted[name]
        assert SR.accepts(prior, u, got, ref)
        start, s0, _ = SR.run_host(exe, SR.host_lines(prior, u))
        assert s0.max() == 0 and not SR.accepts(prior, u, start, ref), name


@pytest.mark.parametrize("family", ["Gamma", "InverseGamma", "Beta", "StudentT"])
def test_one_step_fewer_is_rejected_where_the_most_are_needed(family, counted, tmp_path):
    """the grid point of the family at which the device function takes the most steps, evaluated with the cap set to one step
    fewer: the iterate it returns is outside the bound, so a cap that is hit cannot hide"""
    most, where = 0, None
    for name in SR.settings(family):
        prior, u, ref, got, steps = counted[name]
        i = int(np.argmax(steps))
        if steps[i] > most:
            most, where = int(steps[i]), (name, i)
    name, i = where
    prior, u, ref, got, steps = counted[name]
    exe = SR.build_host(tmp_path, "fewer", defines=("MLF_PRIOR_SPECIAL_MAX_STEPS=%d" % (most - 1),))
    short, s1, _ = SR.run_host(exe, SR.host_lines(prior, u[i:i + 1]))
    print("%s: %d steps at u = %r; with %d the error is %.3g of the bound" % (name, most, u[i], most - 1,
                                                                             SR.excess(prior, u[i:i + 1], short, ref[i:i + 1])[0]))
    assert s1[0] == most - 1
    assert SR.accepts(prior, u[i:i + 1], got[i:i + 1], ref[i:i + 1])
    assert not SR.accepts(prior, u[i:i + 1], short, ref[i:i + 1])


def test_a_dirichlet_block_summed_in_descending_order_mismatches():
    rs = np.random.RandomState(3)
    g = rs.gamma(SR.dirichlet_alpha(5), size=(64, 5))
    want = SR.dirichlet_restatement(g)
    s = g[:, 4].copy()
    for k in range(3, -1, -1):
        s = s + g[:, k]
    assert not np.array_equal(g / s[:, None], want)
    assert np.allclose(g / s[:, None], want, rtol=1e-15, atol=0)
    # and the rules of the restatement: rows sum to 1 within n 2^-52, a row of zeros becomes 1 / n
    assert np.abs(want.sum(axis=1) - 1.0).max() <= 5 * 2.0 ** -52
    assert np.array_equal(SR.dirichlet_restatement(np.zeros((1, 4))), np.full((1, 4), 0.25))
