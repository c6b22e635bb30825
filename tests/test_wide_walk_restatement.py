"""The numpy restatement of the device-side direction draw (tests/randomwalk_reference.py::directions) above 128 dimensions,
where tests/test_wide_walk_gpu.py leans on it: what each of the seven kinds must produce, checked on the restatement alone
(no GPU)."""
import numpy as np
import pytest

import randomwalk_reference as R


def problem(d, nlive=64, seed=5):
    """(axes, live, std): a seeded, well-conditioned d x d matrix (identity plus a perturbation of spectral norm about 0.6)
    scaled to the size of a region's axes, and live points around the middle of the cube"""
    rs = np.random.RandomState(seed + d)
    axes = 0.05 * (np.eye(d) + 0.3 * rs.normal(size=(d, d)) / np.sqrt(d))
    live = np.clip(0.5 + 0.1 * rs.normal(size=(nlive, d)), 0.01, 0.99)
    return axes, live, live.std(axis=0)


@pytest.mark.parametrize("d,P", [(130, 70), (1024, 3)])
def test_what_the_seven_kinds_produce(d, P):
    axes, live, std = problem(d)
    seed, offset, dirscale = 17, 1000, 0.7
    v = {k: R.directions(seed, offset, k, dirscale, P, 1, 0, d, axes=axes, live=live, std=std) for k in range(7)}
    for k in range(7):
        assert v[k].shape == (P, d) and np.isfinite(v[k]).all(), k
    # isotropic kinds: length dirscale, kind 4 in the layer's metric (v = axes g with |g| = dirscale)
    assert np.abs(np.linalg.norm(v[2], axis=1) - dirscale).max() <= 1e-12 * dirscale
    g = np.linalg.solve(axes, v[4].T).T
    assert np.abs(np.linalg.norm(g, axis=1) - dirscale).max() <= 1e-12 * dirscale
    # the two draw the same normals: kind 4 is the axes applied to kind 2
    assert np.abs(g - v[2]).max() <= 1e-11 * dirscale        # (the solve: d * 2^-53 * cond(axes) is 5e-13 at d = 1024)
    # one axis per walker
    for k in (0, 1):
        assert ((v[k] != 0).sum(axis=1) == 1).all(), k
    axis = np.argmax(v[0] != 0, axis=1)
    assert np.array_equal(axis, np.argmax(v[1] != 0, axis=1))
    assert (v[0][np.arange(P), axis] == dirscale).all()
    assert np.array_equal(v[1][np.arange(P), axis], dirscale * std[axis])
    assert np.array_equal(v[3], axes[axis] * dirscale)
    # differences of two distinct live points
    diffs = (live[:, None, :] - live[None, :, :]) * dirscale           # [a][b]
    for i in range(P):
        a, b = np.nonzero((diffs == v[5][i]).all(axis=2))
        assert len(a) == 1 and a[0] != b[0], i
    # the mixture takes one of the two, walker by walker
    from5 = (v[6] == v[5]).all(axis=1)
    from3 = (v[6] == v[3]).all(axis=1)
    assert np.logical_xor(from5, from3).all()
    if P >= 70:
        assert from5.any() and from3.any()
    assert R.next_offset(offset, P, 1, d) == offset + P * ((d + 1) // 2 + 2)
