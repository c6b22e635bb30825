"""StaticNestedSampler and a batched step sampler: such a sampler hands out points it prepared under an EARLIER threshold, so
the driver discards a point that no longer lies above the current one and asks again (reference integrator.py:1941-1950)."""
import numpy as np


class _StaleEveryOtherCall(object):
    """A step sampler whose every other point lies below the threshold; the others are fresh prior draws above it."""
    nsteps = 1

    def __init__(self, loglike):
        self.loglike, self.calls, self.rs = loglike, [], np.random.RandomState(9)

    def region_changed(self, Ls, region):
        pass

    def __next__(self, region, Lmin, us, Ls, transform, loglike, **kwargs):
        stale = len(self.calls) % 2 == 0
        if stale:
            u = np.full(us.shape[1], 0.001)
        else:
            while True:
                cand = self.rs.uniform(size=(4096, us.shape[1]))
                ok = np.flatnonzero(self.loglike(cand) > Lmin)
                if len(ok):
                    u = cand[ok[0]]
                    break
        L = float(self.loglike(u[None, :])[0])
        self.calls.append((Lmin, L, stale))
        return u, u.copy(), L, 1


def test_points_below_the_threshold_are_discarded(backend):
    from ultranest_amd.harness import StaticNestedSampler
    sigma, centers = 0.1, np.array([0.5, 0.5])
    if backend == "hip":
        from ultranest_amd.likelihoods import GaussLikelihood
        loglike = GaussLikelihood(centers, sigma, 2)
    else:
        def loglike(theta):
            return -0.5 * (((theta - centers) / sigma) ** 2).sum(axis=1) - 0.5 * np.log(2 * np.pi * sigma ** 2) * 2
    step = _StaleEveryOtherCall(loglike)
    s = StaticNestedSampler(2, loglike, num_live_points=50, seed=3, stepsampler=step)
    res = s.run(dlogz=0.5)
    calls = step.calls
    assert res["niter"] > 50 and len(calls) >= 2 * (res["niter"] - 1)
    thresholds = [c[0] for c in calls]
    assert all(b >= a for a, b in zip(thresholds, thresholds[1:]))        # the threshold never falls
    for (Lmin, L, stale), (Lmin_next, _, _) in zip(calls, calls[1:]):
        if stale:
            assert L <= Lmin and Lmin_next == Lmin      # asked again under the same threshold
        else:
            assert L > Lmin
    assert abs(res["logz"]) < 5 * res["logzerr"] + 0.3, res
