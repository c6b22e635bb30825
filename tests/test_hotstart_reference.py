"""Warm start, host side (ultranest_amd/hotstart.py) against the reference: the fixture tests/golden/g19_hotstart.npz holds what
the reference's hotstart.py returns for the seeded sample sets of tests/hotstart_reference.py (d = 1, 2, 5 with 11 and 400
samples; 33 cube rows per problem, with u within 2^-53 of both ends and t on every knot).  The quantile tables must come out
bit for bit, the four auxiliary problems within 1e-13 relative; the numpy restatement the device tests use must equal the
fixture too, and each of five seeded defects in it must be rejected by the same comparison."""
import numpy as np
import pytest

import hotstart_reference as HR
from ultranest_amd import hotstart as hs

RTOL = 1e-13
CASES = [(d, n) for d in HR.DIMS for n in HR.NSAMPLES]


@pytest.fixture(scope="module")
def golden():
    with np.load(HR.FIXTURE) as z:
        return {k: z[k] for k in z.files}


def _close(got, want):
    got, want = np.asarray(got, dtype=float), np.asarray(want, dtype=float)
    if got.shape != want.shape:
        return False
    same = (got == want) | (np.isnan(got) & np.isnan(want))
    with np.errstate(all="ignore"):
        near = np.abs(got - want) <= RTOL * np.abs(want)
    return bool((same | near).all())


def _df(n):
    return 1 if n == 11 else 4.5


@pytest.mark.parametrize("d,n", CASES)
def test_quantile_tables_bit_for_bit(golden, d, n):
    key = "d%d_n%d_" % (d, n)
    up, w = HR.samples(d, n)
    assert np.array_equal(up, golden[key + "upoints"]) and np.array_equal(w, golden[key + "uweights"])
    ulos, uhis, xp = hs.compute_quantile_intervals_refined(HR.STEPS, up, w)
    assert np.array_equal(ulos, golden[key + "ulos"]) and np.array_equal(uhis, golden[key + "uhis"])
    assert np.array_equal(xp, golden[key + "uinterpspace"])
    lo0, hi0 = hs.compute_quantile_intervals(HR.STEPS, up, w)
    assert np.array_equal(lo0[:-1], ulos[:len(HR.STEPS)]) and (lo0[-1] == 0).all() and (hi0[-1] == 1).all()
    assert 5 <= len(xp) <= hs.MAX_KNOTS


@pytest.mark.parametrize("d,n", CASES)
def test_contbox_problem_equals_the_reference(golden, d, n):
    key = "d%d_n%d_" % (d, n)
    up, w = HR.samples(d, n)
    u = golden[key + "box_u"]
    xp = golden[key + "uinterpspace"]
    assert set(xp) <= set(u[:, d]) and (u[:, :d] == HR.EPS).any() and (u[:, :d] == 1.0 - HR.EPS).any()
    names, L, T, vec = hs.get_auxiliary_contbox_parameterization(["x%d" % k for k in range(d)], HR.host_loglike, HR.host_transform,
                                                                 up, w, vectorized=True)
    assert names == ["x%d" % k for k in range(d)] + ["aux_logweight"] and vec is True
    p = T(u)
    assert _close(p, golden[key + "box_p"]) and _close(L(p), golden[key + "box_L"])
    names, L1, T1, vec = hs.get_auxiliary_contbox_parameterization(["x%d" % k for k in range(d)], HR.host_loglike, HR.host_transform, up, w)
    assert vec is False
    p1 = np.array([T1(row) for row in u])
    assert _close(p1, golden[key + "box_p"]) and _close([L1(row) for row in p1], golden[key + "box_L"])


@pytest.mark.parametrize("d,n", CASES)
def test_student_t_problems_equal_the_reference(golden, d, n):
    key = "d%d_n%d_" % (d, n)
    up, w = HR.samples(d, n)
    ctr, err, invcov = HR.moments(up, w)
    df = _df(n)
    u = golden[key + "ind_u"]
    assert (u == HR.EPS).any() and (u == 1.0 - HR.EPS).any()
    with np.errstate(all="ignore"):
        L, T = hs.get_extended_auxiliary_independent_problem(HR.host_loglike, HR.host_transform, ctr, err, df=df)
        p = np.array([T(row) for row in u])
        assert _close(p, golden[key + "ind_p"]) and _close([L(row) for row in p], golden[key + "ind_L"])
        L, T = hs.get_auxiliary_problem(HR.host_loglike, HR.host_transform, ctr, invcov, np.sqrt(d), df=df)
        assert _close([T(row) for row in u], golden[key + "rot_p"]) and _close([L(row) for row in u], golden[key + "rot_L"])
        L, T = hs.get_extended_auxiliary_problem(HR.host_loglike, HR.host_transform, ctr, invcov, np.sqrt(d), df=df)
        p = np.array([T(row) for row in u])
        assert _close(p, golden[key + "ext_p"]) and _close([L(row) for row in p], golden[key + "ext_L"])


def _restated_rows(golden, d, n, defect=None):
    key = "d%d_n%d_" % (d, n)
    u = golden[key + "box_u"]
    umod, weight, j, decided = HR.contbox_restated(u, golden[key + "ulos"], golden[key + "uhis"], golden[key + "uinterpspace"], defect)
    p = np.hstack([HR.host_transform(umod), weight[:, None]])
    return p, HR.host_loglike(p[:, :d]) + p[:, d], decided


def _accepted(golden, key, d, p, L):
    """the comparison of the restatement with the fixture: the umod columns bit for bit, weight and likelihood within RTOL"""
    return (np.array_equal(p[:, :d], golden[key + "box_p"][:, :d]) and _close(p, golden[key + "box_p"])
            and _close(L, golden[key + "box_L"]))


@pytest.mark.parametrize("d,n", CASES)
def test_the_restatement_equals_the_reference(golden, d, n):
    key = "d%d_n%d_" % (d, n)
    p, L, decided = _restated_rows(golden, d, n)
    assert decided.all()
    assert _accepted(golden, key, d, p, L)
    umod, logvol = hs.contbox_rows(golden[key + "box_u"], golden[key + "ulos"], golden[key + "uhis"], golden[key + "uinterpspace"])
    assert np.array_equal(HR.host_transform(umod), p[:, :d]) and np.array_equal(logvol[:, 0], p[:, d])


@pytest.mark.parametrize("defect", HR.DEFECTS)
def test_each_seeded_defect_is_rejected(golden, defect):
    rejected = set()
    for d, n in CASES:
        key = "d%d_n%d_" % (d, n)
        with np.errstate(all="ignore"):
            p, L, decided = _restated_rows(golden, d, n, defect)
        if not _accepted(golden, key, d, p, L):
            rejected.add((d, n))
    if defect == "interp_from_right_knot":
        # the same line in exact arithmetic: it differs from the left-knot form in last bits only.  These five cases of the
        # recorded fixture show such a bit on at least one of their 33 rows; d = 2 with 11 samples happens to show none
        assert rejected >= {(1, 11), (1, 400), (2, 400), (5, 11), (5, 400)}, rejected
    else:
        assert rejected == set(CASES), (defect, rejected)


def test_the_tail_holds_numpys_slopes(golden):
    key = "d5_n400_"
    ulos, uhis, xp = golden[key + "ulos"], golden[key + "uhis"], golden[key + "uinterpspace"]
    tail = hs.contbox_tail(ulos, uhis, xp)
    M, d = ulos.shape
    assert len(tail) == 1 + M + 2 * M * d + 2 * (M - 1) * d and tail[-1] == M
    assert np.array_equal(tail[:M], xp) and np.array_equal(tail[M:M + M * d], ulos.ravel())
    slo = tail[M + M * d:M + M * d + (M - 1) * d].reshape(M - 1, d)
    assert np.array_equal(slo, (ulos[1:] - ulos[:-1]) / (xp[1:] - xp[:-1])[:, None])


def test_value_errors_carry_messages():
    up, w = HR.samples(2, 400)
    f, t = HR.host_loglike, HR.host_transform
    with pytest.raises(ValueError, match="2d array"):
        hs.get_auxiliary_contbox_parameterization(["a"], f, t, up[:, 0], w)
    with pytest.raises(ValueError, match="strictly between 0 and 1"):
        hs.get_auxiliary_contbox_parameterization(["a", "b"], f, t, up * 3, w)
    with pytest.raises(ValueError, match="more than 10 samples"):
        hs.get_auxiliary_contbox_parameterization(["a", "b"], f, t, up[:10], w[:10])
    with pytest.raises(ValueError, match="cumulative weight"):            # the reference: min() of an empty selection
        hs.compute_quantile_intervals([0.1], up, w * 0.01)
    with pytest.raises(ValueError, match="invcov must have shape"):
        hs.get_auxiliary_problem(f, t, np.full(2, 0.5), np.eye(3), 1.0)
    with pytest.raises(ValueError, match="df"):
        hs.get_extended_auxiliary_problem(f, t, np.full(2, 0.5), np.eye(2), 1.0, df=0.5)
    with pytest.raises(ValueError, match="err must have shape"):
        hs.get_extended_auxiliary_independent_problem(f, t, np.full(2, 0.5), np.full(3, 0.1))


def test_reuse_samples_is_silent_and_reweights(capsys):
    rs = np.random.RandomState(3)
    pts = rs.uniform(size=(300, 2))
    logl = -0.5 * (((pts - 0.5) / 0.2) ** 2).sum(axis=1)

    def shifted(x):
        return -0.5 * (((x - 0.5) / 0.2) ** 2).sum(axis=1) + 1.5

    res = hs.reuse_samples(["a", "b"], shifted, pts, logl, upoints=pts, vectorized=True)
    assert capsys.readouterr().out == ""
    assert res["niter"] == 300 and res["ncall"] == 300 and res["param_names"] == ["a", "b"]      # no batch is negligible here
    # equally weighted points, reweighted by exp(L_new): ln Z = ln mean exp(L_new); Kish's effective sample size
    w = np.exp(shifted(pts))
    assert abs(res["logz"] - np.log(np.mean(w))) < 1e-12
    assert abs(res["ess"] - w.sum() ** 2 / (w ** 2).sum()) < 1e-9 * res["ess"]
    spread = np.sqrt(((w / w.sum() - 1.0 / 300) ** 2).sum() / 299)
    assert abs(res["logzerr"] - np.log1p(spread)) < 1e-14
    assert np.array_equal(res["weighted_samples"]["logl"], shifted(pts)) and res["maximum_likelihood"]["logl"] == shifted(pts).max()
    assert res["maximum_likelihood"]["point"] == pts[np.argmax(shifted(pts))].tolist() and len(res["posterior"]["information_gain_bits"]) == 2
    # the scalar form of the likelihood gives the same numbers
    one = hs.reuse_samples(["a", "b"], lambda x: float(shifted(x[None, :])[0]), pts, logl, upoints=pts, logzerr=0.3)
    assert one["logz"] == res["logz"] and abs(one["logzerr"] - np.hypot(res["logzerr"], 0.3)) < 1e-15
    # a likelihood ten times narrower: the visit ends after the second batch of 32 (pinned for this seeded case), the 236 points
    # not visited keep weight 0, and what they would have added is below the threshold
    def narrow(x):
        return -0.5 * (((x - 0.5) / 0.02) ** 2).sum(axis=1)

    early = hs.reuse_samples(["a", "b"], narrow, pts, logl, upoints=pts, vectorized=True, batchsize=32)
    assert early["ncall"] == 64 and np.isinf(early["weighted_samples"]["logl"]).sum() == 236
    assert (early["weighted_samples"]["weights"][np.isinf(early["weighted_samples"]["logl"])] == 0).all()
    assert abs(early["logz"] - np.log(np.mean(np.exp(narrow(pts))))) < 1e-9
    with pytest.raises(ValueError, match="one entry per point"):
        hs.reuse_samples(["a", "b"], lambda x: x[:, 0], pts, logl[:-1], vectorized=True)
