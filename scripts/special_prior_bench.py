#!/usr/bin/env python3
"""What the iterative prior families of the prior library (ultranest_amd.priors: Gamma, Beta, StudentT) cost inside the device
refill, measured on one GPU in one process; writes profiles/special_prior_bench.json.

    python scripts/special_prior_bench.py [--reps 20] [--warmup 5] [--out profiles/special_prior_bench.json]

The method is that of scripts/prior_transform_bench.py.  Shape C5 (N = 4000 live points, d = 50), region.refill of 2^20 draws
from the wrapping ellipsoid: draw, region test, transform + likelihood of the member rows in one fused launch, compaction.
Every model has the SAME likelihood text and data (the Gaussian of usermodels.gauss, sigma 0.1), a region of identical state and
the same Philox position, so that the models differ in the transform alone.  Two legs: Lmin = 1e300 keeps no row (what is left
is the device work), Lmin = -1e300 keeps every member row (mostly the copy of those rows to the host).  The models:
  affine    usermodels.gauss(50, affine=True): the hand-written transform u * 20 - 10
  normal    50 Normal(0, 2): one normcdfinv per column -- the BASELINE of every ratio; this code is the closed-form library's
  gamma     50 Gamma(2.5, 1)
  beta      50 Beta(2, 3)
  studentt  50 StudentT(5)
  mixed     ten each of Gamma(2.5), Beta(2, 3), StudentT(5), InverseGamma(3, 2) and Normal(0, 2)
`warmup` rounds, then `reps` rounds in which the models take turns; wall clock around each call (every one synchronises),
medians.  An iterative quantile whose lanes end at different step counts costs several times a normcdfinv: the ratio is
reported for users to decide by, not asserted against a threshold.
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--draws", type=int, default=2 ** 20)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "special_prior_bench.json"))
    args = ap.parse_args()
    from ultranest_amd import _lib, usermodels
    from ultranest_amd import priors as P
    from ultranest_amd.regions import DeviceRNG
    import ultranest_amd.mlfriends as M
    from csrc_build import source_hash
    N, d, n = 4000, 50, args.draws
    if _lib.device_count() < 1:
        raise SystemExit("special_prior_bench needs a GPU: nothing is measured without one")
    res = dict(device=_lib.device_name(), source_hash=source_hash(), nlive=N, d=d, draws=n,
               method="sample_from_wrapping_ellipsoid", reps=args.reps, warmup=args.warmup, baseline="normal")
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
    cycle = [lambda: P.Gamma(2.5, 1.0), lambda: P.Beta(2.0, 3.0), lambda: P.StudentT(5.0), lambda: P.InverseGamma(3.0, 2.0),
             lambda: P.Normal(0.0, 2.0)]

    def of(make, name):
        return P.PriorTransform([make(k) for k in range(d)]).model(loglike, aux=centers, name=name)

    models = dict(
        affine=usermodels.gauss(d, affine=True),
        normal=of(lambda k: P.Normal(0.0, 2.0), "normal50"),
        gamma=of(lambda k: P.Gamma(2.5, 1.0), "gamma50"),
        beta=of(lambda k: P.Beta(2.0, 3.0), "beta50"),
        studentt=of(lambda k: P.StudentT(5.0), "studentt50"),
        mixed=of(lambda k: cycle[k % len(cycle)](), "special_mixed50"))
    regions = {k: make_region() for k in models}
    legs = dict(keep_none=1e300, keep_all=-1e300)
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
        res[leg]["same_rows"] = bool(all(np.array_equal(out["normal"][0], out[k][0]) for k in models))
        for k in models:
            res[leg][k + "_over_normal"] = res[leg][k]["ms_median"] / res[leg]["normal"]["ms_median"]
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
