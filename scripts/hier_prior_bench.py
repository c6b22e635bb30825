#!/usr/bin/env python3
"""What priors with run-time parameters (priors.Ref) and tabulated quantiles (priors.Tabulated) cost inside the device refill,
measured on one GPU in one process; writes profiles/hier_prior_bench.json.

    python scripts/hier_prior_bench.py [--reps 20] [--warmup 5] [--out profiles/hier_prior_bench.json]

The method of scripts/prior_transform_bench.py: shape C5 (N = 4000 live points, d = 50), region.refill of 2^20 draws from the
wrapping ellipsoid, the SAME likelihood text and data (the Gaussian of usermodels.gauss, sigma 0.1) on regions of identical
state and the same Philox position, so that the models differ in the transform alone.  Two legs: Lmin = -1e300 keeps every
member row, Lmin = 1e300 keeps none (what is left is the device work).  The models:
  (a) normal     50 Normal(0, 2) priors (the baseline of the constant-parameter library, re-measured here)
  (b) hier       mu ~ Normal(0, 2), tau ~ LogUniform(0.5, 2), 48 Normal(Ref(mu), Ref(tau)): the same device function with two
                 guarded register arguments in place of two literals
  (c) table327   50 Tabulated of 327 knots each (the quantiles of Normal(0, 2) on an even grid of the CDF): 16 350 knots, the most
                 that fifty tables of one transform may hold (the cap is 16 384 knots)
      table1024  16 Tabulated of 1024 knots (16 384 knots) and 34 Normal(0, 2)
  (d) table4096  4 Tabulated of 4096 knots (16 384 knots) and 46 Normal(0, 2)
`warmup` rounds, then `reps` rounds in which the models take turns; wall clock around each call (every one synchronises),
medians.  Recorded per leg: every model's time over a's, the member rows per call; the device name and the kernel-source hash.  No
threshold: the ratios are reported, not asserted.
"""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def normal_table(n, sigma=2.0):
    """n knots of the Normal(0, sigma) quantile function on an even grid of the CDF, the ends at +-6 sigma"""
    from ultranest_amd import priors as P
    nd = statistics.NormalDist(0.0, sigma)
    c = np.linspace(0.0, 1.0, n)
    x = np.array([-6.0 * sigma] + [nd.inv_cdf(float(v)) for v in c[1:-1]] + [6.0 * sigma])
    return P.Tabulated(x, c)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--draws", type=int, default=2 ** 20)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "hier_prior_bench.json"))
    args = ap.parse_args()
    from ultranest_amd import _lib, usermodels
    from ultranest_amd import priors as P
    from ultranest_amd.regions import DeviceRNG
    import ultranest_amd.mlfriends as M
    from csrc_build import source_hash
    N, d, n = 4000, 50, args.draws
    if _lib.device_count() < 1:
        raise SystemExit("hier_prior_bench needs a GPU: nothing is measured without one")
    res = dict(device=_lib.device_name(), source_hash=source_hash(), nlive=N, d=d, draws=n,
               method="sample_from_wrapping_ellipsoid", reps=args.reps, warmup=args.warmup)
    rs = np.random.RandomState(1)
    live = np.clip(0.5 + 0.1 * rs.normal(size=(N, d)), 1e-6, 1 - 1e-6)

    def make_region():
        layer = M.AffineLayer()
        layer.optimize(live, live)
        region = M.MLFriends(live.copy(), layer)
        region.maxradiussq, region.enlarge = region.compute_enlargement(nbootstraps=30, rng=np.random.RandomState(2))
        region.create_ellipsoid()
        return region

    loglike, centers = usermodels.GAUSS_LOGLIKE % 0.1, usermodels.gauss_centers(d, 0.1)
    hier = [P.Normal(0.0, 2.0, name="mu"), P.LogUniform(0.5, 2.0, name="tau")] + \
        [P.Normal(P.Ref("mu"), P.Ref("tau")) for _ in range(d - 2)]
    normal = lambda: P.Normal(0.0, 2.0)
    lists = dict(
        a_normal=[normal() for _ in range(d)],
        b_hier=hier,
        c_table327=[normal_table(327) for _ in range(d)],
        c_table1024=[normal_table(1024) for _ in range(16)] + [normal() for _ in range(d - 16)],
        d_table4096=[normal_table(4096) for _ in range(4)] + [normal() for _ in range(d - 4)])
    models, res["compile_s"] = {}, {}
    for k, pri in lists.items():
        t0 = time.perf_counter()
        models[k] = P.PriorTransform(pri).model(loglike, aux=centers, name=k)
        res["compile_s"][k] = time.perf_counter() - t0
    regions = {k: make_region() for k in models}
    legs = dict(keep_all=-1e300, keep_none=1e300)
    for leg, Lmin in legs.items():
        ms = {k: [] for k in models}
        out = {}
        for r in range(args.warmup + args.reps):
            for k, m in models.items():
                reg = regions[k]
                reg.device_rng = DeviceRNG(7)
                reg.current_sampling_method = reg.sample_from_wrapping_ellipsoid
                t0 = time.perf_counter()
                got = reg.refill(n, Lmin, m.transform, m.loglike)
                t1 = time.perf_counter()
                assert got is not None, k
                if r >= args.warmup:
                    ms[k].append((t1 - t0) * 1e3)
                out[k] = got
        res[leg] = {k: dict(ms_median=float(np.median(v)), ms_min=float(np.min(v)), ms_max=float(np.max(v)),
                            kept=int(len(out[k][0])), evaluated=int(out[k][3])) for k, v in ms.items()}
        res[leg]["same_rows"] = bool(all(np.array_equal(out["a_normal"][0], out[k][0]) for k in models))
        for k in models:
            if k != "a_normal":
                res[leg][k + "_over_a"] = res[leg][k]["ms_median"] / res[leg]["a_normal"]["ms_median"]
    for m in models.values():
        m.close()
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as fh:
        json.dump(res, fh, indent=1, sort_keys=True)
    print(json.dumps(res, sort_keys=True))


if __name__ == "__main__":
    sys.path.insert(0, os.path.join(ROOT, "ultranest_amd", "csrc"))
    import importlib
    sys.modules["csrc_build"] = importlib.import_module("build")
    main()
