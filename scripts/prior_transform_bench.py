#!/usr/bin/env python3
"""What a prior transform from the prior library (ultranest_amd.priors) costs inside the device refill, measured on one GPU in
one process; writes profiles/prior_transform_bench.json.

    python scripts/prior_transform_bench.py [--reps 20] [--warmup 5] [--out profiles/prior_transform_bench.json]

Shape C5 (N = 4000 live points, d = 50), region.refill of 2^20 draws from the wrapping ellipsoid (method 1): draw, region test,
transform + likelihood of the member rows in one fused launch, compaction.  Three models with the SAME likelihood text and data
(the Gaussian of usermodels.gauss, sigma 0.1) on regions of identical state and the same Philox position, so that they differ in
the transform alone.  Two legs: Lmin = -1e300 keeps every member row (the three calls return the same rows of u, and the call is
mostly the copy of those rows to the host), Lmin = 1e300 keeps none (what is left is the device work: draw, test, transform,
likelihood).  The models:
  (a) affine   usermodels.gauss(50, affine=True): the hand-written transform u * 20 - 10 (the baseline)
  (b) normal   50 Normal(0, 2) priors: 50 calls of mlf_prior_normal per row (one normcdfinv each)
  (c) mixed    five each of Uniform, LogUniform, Normal, TruncatedNormal, Exponential, Cauchy, Laplace, Sine, HalfNormal and
               Weibull priors
`warmup` rounds, then `reps` rounds in which the three take turns (a drift of the clocks meets all alike); wall clock around each
call (every one synchronises), medians.  Recorded per leg: b / a and c / a, the member rows per call; the device name and the
kernel-source hash.  No threshold: the ratio is reported, not asserted.
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
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "prior_transform_bench.json"))
    args = ap.parse_args()
    from ultranest_amd import _lib, usermodels
    from ultranest_amd import priors as P
    from ultranest_amd.regions import DeviceRNG
    import ultranest_amd.mlfriends as M
    from csrc_build import source_hash
    N, d, n = 4000, 50, args.draws
    if _lib.device_count() < 1:
        raise SystemExit("prior_transform_bench needs a GPU: nothing is measured without one")
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
    cycle = [lambda: P.Uniform(-10.0, 10.0), lambda: P.LogUniform(1e-3, 10.0), lambda: P.Normal(0.0, 2.0),
             lambda: P.TruncatedNormal(0.0, 1.0, -1.0, 2.0), lambda: P.Exponential(2.0), lambda: P.Cauchy(0.0, 1.0),
             lambda: P.Laplace(0.0, 1.0), lambda: P.Sine(), lambda: P.HalfNormal(1.0), lambda: P.Weibull(1.0, 1.5)]
    models = dict(
        a_affine=usermodels.gauss(d, affine=True),
        b_normal=P.PriorTransform([P.Normal(0.0, 2.0) for _ in range(d)]).model(loglike, aux=centers, name="normal50"),
        c_mixed=P.PriorTransform([cycle[k % len(cycle)]() for k in range(d)]).model(loglike, aux=centers, name="mixed50"))
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
        res[leg]["same_rows"] = bool(np.array_equal(out["a_affine"][0], out["b_normal"][0])
                                     and np.array_equal(out["a_affine"][0], out["c_mixed"][0]))
        res[leg]["normal_over_affine"] = res[leg]["b_normal"]["ms_median"] / res[leg]["a_affine"]["ms_median"]
        res[leg]["mixed_over_affine"] = res[leg]["c_mixed"]["ms_median"] / res[leg]["a_affine"]["ms_median"]
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
