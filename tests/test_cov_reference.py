"""The references of the covariance form (cov_reference.py), CPU only: the numpy restatement of the arithmetic contract lies within
the DERIVED bound of an mpmath Cholesky at 60 digits (error over bound is printed), it follows the contract's failure rule, and
each seeded defect is seen -- the gross ones by the bound, the rounding-order ones by the bit-for-bit comparison the GPU tests
make with the device's factor."""
import numpy as np
import pytest

import cov_reference as R
from ultranest_amd import usermodels


def _spd(n, seed, kappa=None):
    rs = np.random.RandomState(seed)
    Q, _ = np.linalg.qr(rs.normal(size=(n, n)))
    lam = np.exp(rs.uniform(0, np.log(kappa if kappa else 10.0), size=n))
    K = (Q * lam).dot(Q.T)
    return np.tril(0.5 * (K + K.T)), rs.normal(size=n)


@pytest.mark.parametrize("kappa", [1e1, 1e6, 1e10])
@pytest.mark.parametrize("n", [1, 2, 3, 24, 65])
def test_restatement_within_the_derived_bound(n, kappa):
    K, r = _spd(n, 7 * n, kappa)
    tri, L = R.restate(K, r)
    want = R.mp_loglike(K, r)            # the same binary64 entries: no entry term in the bound
    b = R.bound(K, r)
    err = abs(float(want - R.mp_mpf(L)))
    print("n = %d, kappa_2 = %.3g: error %.3g, bound %.3g, error / bound = %.3g" % (n, np.linalg.cond(K + np.tril(K, -1).T), err, b, err / b))
    assert np.isfinite(b) and err <= b
    # the factor is a factor: |Lfac Lfac^T - K| <= gamma_(n+1) |Lfac||Lfac|^T entrywise (the theorem the bound starts from), and the
    # forward substitution's residual likewise (gamma_n |Lfac||z|)
    Lfac, z = R.unpack(tri, n)
    full = K + np.tril(K, -1).T
    assert (np.abs(Lfac.dot(Lfac.T) - full) <= 2 * R.gamma(n + 1) * np.abs(Lfac).dot(np.abs(Lfac).T)).all()
    assert (np.abs(Lfac.dot(z) - r) <= 2 * R.gamma(n + 1) * np.abs(Lfac).dot(np.abs(z))).all()
    assert R.finish(tri, n) == L


@pytest.mark.parametrize("kappa", [1e1, 1e6, 1e10])
def test_gp_model_within_the_bound_with_its_entry_errors(kappa):
    """what the GPU test asks of the device, asked of numpy: the exact model as the reference, the entries' own rounding in the bound"""
    n = 24
    x, y = usermodels.gp_data(n)
    lam = np.linalg.eigvalsh(R.gp_matrices([[0.0, 0.0, -50.0, 0.0]], x, y)[0][0]).max()
    p = np.array([0.0, 0.0, 0.5 * np.log(lam / kappa), 0.1])
    K, r = R.gp_matrices(p, x, y)
    L = R.restate(K[0], r[0])[1]
    err, b = abs(float(R.gp_mp_loglike(p, x, y) - R.mp_mpf(L))), R.bound(K[0], r[0], entry_eps=R.GP_ENTRY_EPS)
    print("kappa_2 = %.3g: error / bound = %.3g" % (np.linalg.cond(K[0]), err / b))
    assert err <= b


def test_failure_rule():
    K, r = _spd(9, 3)
    for k in (0, 4, 8):
        bad = K.copy()
        bad[k, k] = -1e6
        tri, L = R.restate(bad, r)
        assert np.isneginf(L) and np.isnan(tri).all()
        bad[k, k] = np.nan
        tri, L = R.restate(bad, r)
        assert np.isnan(L) and np.isnan(tri).all()
    zero = K.copy()
    zero[0, 0] = 0.0                      # "not > 0" includes 0
    assert np.isneginf(R.restate(zero, r)[1])
    both = K.copy()
    both[2, 2], both[6, 6] = -1e6, np.nan      # the first failing pivot in ascending k decides
    assert np.isneginf(R.restate(both, r)[1])
    both[2, 2], both[6, 6] = np.nan, -1e6
    assert np.isnan(R.restate(both, r)[1])


@pytest.mark.parametrize("defect", R.DEFECTS)
def test_seeded_defects_are_seen(defect):
    """every defect changes the bits of the factor or of L on each of three matrices (what the bit-for-bit GPU comparison sees);
    the three that change the mathematics also leave the bound"""
    gross = defect in ("skip_aug", "bad_index", "no_sqrt")
    for seed in (1, 2, 3):
        n = 33
        K, r = _spd(n, seed, 1e3)
        tri, L = R.restate(K, r)
        tri_d, L_d = R.restate(K, r, defect=defect)
        assert not (np.array_equal(tri, tri_d) and L == L_d), defect
        if defect in ("descending", "unrounded"):
            assert not np.array_equal(tri, tri_d)      # the rounding order shows in the factor itself
        err = abs(float(R.mp_loglike(K, r) - R.mp_mpf(L_d)))
        assert (err > R.bound(K, r)) == gross, (defect, err, R.bound(K, r))


def test_packing():
    full = np.arange(16.0).reshape(4, 4)
    tri = R.pack(full)
    assert list(tri) == [0, 4, 5, 8, 9, 10, 12, 13, 14, 15] and len(tri) == R.tri_size(3)
    for i in range(4):
        for j in range(i + 1):
            assert tri[i * (i + 1) // 2 + j] == full[i, j]
    Lfac, z = R.unpack(tri, 3)
    assert np.array_equal(Lfac, np.tril(full)[:3, :3]) and list(z) == [12, 13, 14]


def test_quadrature_converges():
    x, y = usermodels.gp_data(20)
    lo, width = usermodels.GP_PRIOR_LO, usermodels.GP_PRIOR_WIDTH
    a, b = R.gp_lnz_quadrature(x, y, lo, width, 20), R.gp_lnz_quadrature(x, y, lo, width, 28)
    assert abs(a - b) < 1e-3
