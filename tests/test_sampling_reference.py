"""The CPU leg of the proposal sampling tests (sampling_reference.py): the matcher on synthetic data, the binary64 restatement
of oracle/philox.py within 1e-13 * scale of the high-precision reference, the two references within 1e-17 * scale of each
other, and the verdicts against the plain host tests on decided draws.  The margin of the device bound (1e-12 * scale,
test_sampling_draws.py) stays on record here and is never measured on the kernels under test."""
import numpy as np
import pytest

from oracle import philox

import sampling_reference as S

D_ALL = (1, 2, 4, 5, 8, 9, 16, 17, 32, 33, 52, 53, 64, 65, 127, 128, 129, 130, 318)      # 318: test_sampling_draws.D_POINTS_WIDE
N = 389          # six workgroups of 64 rows and a ragged one of 5


def host_geometry(d, seed, wrapped=False, friends=True, nlive=None):
    """a region's numbers from host numpy alone: live points as test_philox._region draws them, AffineLayer.optimize,
    MLFriends.ellipsoid_parts; enlargement and radius are free inputs of the draws"""
    import ultranest_amd.mlfriends as m
    rng = np.random.RandomState(seed)
    u = 0.5 + 0.08 * rng.normal(size=(nlive or (150 if d < 100 else max(300, 2 * d)), d)) * np.linspace(0.5, 1.5, d)
    if wrapped:
        u[:, 0] = (0.98 + 0.05 * rng.normal(size=len(u))) % 1.0
    u = u[np.logical_and(u > 0, u < 1).all(axis=1)]
    layer = S.affine_layer(u, [0] if wrapped else [])
    ctr, cov, precision, axes = m.MLFriends.ellipsoid_parts(u)
    t = layer.transform(u)
    return S.Geometry(u, layer.ctr, layer.T, layer.invT, layer.wrap_shift_vector(d), ctr, precision, axes[2], 1.7, 0.35,
                      t.min(axis=0), t.max(axis=0), friends), layer


# ------------------------------------------------------------------------------------------------ the matcher
def _synthetic(seed=1, n=600, d=3):
    rs = np.random.RandomState(seed)
    ref = rs.normal(size=(n, d)).astype(S.LD) + rs.normal(size=(n, d)).astype(S.LD) * 1e-17
    scale = np.abs(ref).astype(np.float64) + 1.0
    verdict = rs.choice([S.OUT, S.IN], size=n, p=[0.4, 0.6]).astype(np.int8)
    verdict[[17, 200, 431]] = S.UNDECIDED
    return ref, scale, verdict


def _accepted(ref, verdict, keep_undecided=(17, 431)):
    take = (verdict == S.IN)
    take[list(keep_undecided)] = True
    return np.flatnonzero(take), ref[take].astype(np.float64)


def test_matcher_accepts_the_reference_itself():
    ref, scale, verdict = _synthetic()
    idx, got = _accepted(ref, verdict)
    assert S.match_in_draw_order(got, ref, verdict, scale) == (3, len(got))
    # every undecided row dropped, or every one kept: both are the device's right
    assert S.match_in_draw_order(_accepted(ref, verdict, ())[1], ref, verdict, scale)[1] == len(got) - 2
    assert S.match_in_draw_order(_accepted(ref, verdict, (17, 200, 431))[1], ref, verdict, scale)[1] == len(got) + 1
    # perturbed by 1e-14 * scale
    rs = np.random.RandomState(2)
    moved = got + 1e-14 * scale[idx] * rs.choice([-1.0, 1.0], size=got.shape)
    assert S.match_in_draw_order(moved, ref, verdict, scale) == (3, len(got))
    assert S.match_in_draw_order(got[:0], ref, np.where(verdict == S.IN, S.OUT, verdict), scale) == (3, 0)


@pytest.mark.parametrize("where", [0, 150, -1])
def test_matcher_rejects_a_dropped_decided_row(where):
    ref, scale, verdict = _synthetic()
    idx, got = _accepted(ref, verdict)
    assert verdict[idx[where]] == S.IN
    with pytest.raises(S.DrawMismatch):
        S.match_in_draw_order(np.delete(got, where, axis=0), ref, verdict, scale)
    # ... also next to an undecided draw that the device dropped as well
    pos = int(np.searchsorted(idx, 200))
    assert verdict[idx[pos]] == S.IN
    with pytest.raises(S.DrawMismatch):
        S.match_in_draw_order(np.delete(_accepted(ref, verdict, ())[1], pos - 1, axis=0), ref, verdict, scale)


@pytest.mark.parametrize("where", [0, 150, -1])
def test_matcher_rejects_a_duplicated_row(where):
    ref, scale, verdict = _synthetic()
    idx, got = _accepted(ref, verdict)
    where %= len(got)
    with pytest.raises(S.DrawMismatch):
        S.match_in_draw_order(np.insert(got, where, got[where], axis=0), ref, verdict, scale)


def test_matcher_rejects_swapped_columns_and_a_value_off_by_1e11():
    ref, scale, verdict = _synthetic()
    idx, got = _accepted(ref, verdict)
    with pytest.raises(S.DrawMismatch):
        S.match_in_draw_order(got[:, [0, 2, 1]], ref, verdict, scale)
    one_row = got.copy()
    one_row[77] = one_row[77, [1, 0, 2]]
    with pytest.raises(S.DrawMismatch, match="column 0"):
        S.match_in_draw_order(one_row, ref, verdict, scale)
    for sign in (-1.0, 1.0):
        off = got.copy()
        off[301, 2] += sign * 1e-11 * scale[idx[301], 2]
        with pytest.raises(S.DrawMismatch, match="draw %d .*column 2" % idx[301]):
            S.match_in_draw_order(off, ref, verdict, scale)
    with pytest.raises(S.DrawMismatch):
        S.match_in_draw_order(np.where(np.arange(len(got))[:, None] == 5, np.nan, got), ref, verdict, scale)


def test_matcher_rejects_rows_left_over_and_an_undecided_row_with_a_wrong_value():
    ref, scale, verdict = _synthetic()
    idx, got = _accepted(ref, verdict)
    with pytest.raises(S.DrawMismatch):
        S.match_in_draw_order(np.vstack([got, got[-1:] + 0.5]), ref, verdict, scale)
    wrong = got.copy()
    wrong[int(np.searchsorted(idx, 17))] += 1e-6      # an undecided draw may be absent, not different
    with pytest.raises(S.DrawMismatch):
        S.match_in_draw_order(wrong, ref, verdict, scale)


# ------------------------------------------------------------------------------------------------ oracle/philox.py, binary64
SEED, OFFSET = 2**63 + 12345, 2**32 - 700      # high key word; the batch crosses a multiple of 2^32


@pytest.mark.parametrize("d", D_ALL)
def test_binary64_ellipsoid_draw_within_1e13(d):
    g, _ = host_geometry(d, 100 + d)
    w, scale, nxt = S.ellipsoid_draws(g, SEED, OFFSET, N)
    z, nxt64 = philox.ball_points(SEED, OFFSET, N, d, g.enlarge)
    assert nxt == nxt64 == OFFSET + N * ((d + 1) // 2 + 1)
    assert S.excess(g.center + np.dot(z, g.axes_T), w, scale, rtol=1e-13) <= 1.0
    assert (scale * (1 + 1e-15) >= np.abs(S.REFERENCE.f64(w))).all()


@pytest.mark.parametrize("d,wrapped", [(d, False) for d in D_ALL] + [(5, True), (17, True)])
def test_binary64_tspace_draws_within_1e13(d, wrapped):
    g, layer = host_geometry(d, 200 + d, wrapped=wrapped)
    B = S.REFERENCE
    t, ts, nxt = S.tbox_draws(g, SEED, OFFSET, N)
    t64, nxt64 = philox.tbox_points(SEED, OFFSET, N, d, g.bbox_lo, g.bbox_hi, g.r2 ** 0.5)
    assert nxt == nxt64
    assert S.excess(t64, t, ts, rtol=1e-13) <= 1.0
    with B.ctx():
        w, ws = S.untransform(B, g, t, ts)
    assert S.excess(layer.untransform(t64), w, ws, rtol=1e-13) <= 1.0
    t, ts, thin, which, nxt = S.around_draws(g, SEED, OFFSET, N)
    t64, thin64, which64, nxt64 = philox.around_points(SEED, OFFSET, N, d, layer.transform(g.u), g.r2)
    assert nxt == nxt64 and np.array_equal(thin, thin64) and np.array_equal(which, which64)
    assert len(np.unique(which)) > min(N, len(g.u)) // 3
    assert S.excess(t64, t, ts, rtol=1e-13) <= 1.0
    with B.ctx():
        w, ws = S.untransform(B, g, t, ts)
    assert S.excess(layer.untransform(t64), w, ws, rtol=1e-13) <= 1.0


# ------------------------------------------------------------------------------------------------ the two references
def _disagreement(mp_values, ld_values, scale):
    """max |mpmath - long double| / scale, the subtraction done at 50 digits"""
    diff = S.LR.mp_minus(list(np.asarray(mp_values).ravel()), np.asarray(ld_values).ravel())
    return float((diff / np.maximum(np.asarray(scale).ravel(), 1e-300)).max())


@pytest.mark.parametrize("d,wrapped", [(1, False), (2, False), (5, True), (17, False), (53, False), (129, False), (318, False)])
def test_long_double_and_mpmath_agree(d, wrapped):
    if not (S.HAVE_LONGDOUBLE and S.HAVE_MPMATH):
        return      # one reference only: nothing to compare
    g, _ = host_geometry(d, 300 + d, wrapped=wrapped, nlive=max(40, 3 * d))
    rows = np.array([0, 1, 63, 64, N - 1] if d < 200 else [64, N - 1])      # (mpmath at d = 318: 6 s with these two)
    L, M = S.LongDouble, S.MpMath
    for draw in (S.ellipsoid_draws, S.tbox_draws, S.around_draws):
        a = draw(g, SEED, OFFSET, N, rows=rows, B=L)
        b = draw(g, SEED, OFFSET, N, rows=rows, B=M)
        assert np.allclose(a[1], b[1], rtol=1e-12, atol=0) and a[2:] == b[2:] if draw is not S.around_draws else a[4] == b[4]
        assert _disagreement(b[0], a[0], a[1]) <= 1e-17
        if draw is not S.ellipsoid_draws:
            wa, sa = S.untransform(L, g, a[0], a[1])
            with M.ctx():
                wb, sb = S.untransform(M, g, b[0], b[1])
            assert _disagreement(wb, wa, sa) <= 1e-17


# ------------------------------------------------------------------------------------------------ verdicts
@pytest.mark.parametrize("method,d,wrapped", [(1, 2, False), (1, 8, False), (2, 2, False), (2, 5, True), (3, 5, True), (3, 9, False)])
def test_verdicts_are_the_host_tests_on_decided_draws(method, d, wrapped):
    """plain binary64 numpy on the binary64 restatement: cube, einsum ellipsoid, pair distances; it may differ from the
    reference on undecided draws only, and the share of undecided draws is what the band predicts (none, in a few thousand)"""
    g, layer = host_geometry(d, 400 + d, wrapped=wrapped)
    n = 4133
    ref = S.Reference(g, method, n, 7, 11)
    live = layer.transform(g.u)

    def near(t):
        return (((t[:, None, :] - live[None, :, :]) ** 2).sum(axis=2) <= g.r2).sum(axis=1)

    if method == 1:
        z, _ = philox.ball_points(7, 11, n, d, g.enlarge)
        w = g.center + np.dot(z, g.axes_T)
        keep = near(layer.transform(w)) > 0
    elif method == 2:
        t, _ = philox.tbox_points(7, 11, n, d, g.bbox_lo, g.bbox_hi, g.r2 ** 0.5)
        w = layer.untransform(t)
        keep = near(t) > 0
    else:
        t, thin, which, _ = philox.around_points(7, 11, n, d, live, g.r2)
        w = layer.untransform(t)
        mult = near(t)
        keep = (mult > 0) & (thin * mult < 1)
    dl = w - g.center
    keep &= np.logical_and(w > 0, w < 1).all(axis=1) & (np.einsum("ij,jk,ik->i", dl, g.invcov, dl) <= g.enlarge)
    decided = ref.verdict != S.UNDECIDED
    assert np.array_equal(keep[decided], ref.verdict[decided] == S.IN)
    assert ref.undecided <= 2 and 50 < ref.decided_in <= n
    assert ref.match(w[keep]) == (ref.undecided, int(keep.sum()))
