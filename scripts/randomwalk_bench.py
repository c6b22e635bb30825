#!/usr/bin/env python3
"""One refill of PopulationRandomWalkSampler three ways, measured on one GPU in one process; writes
profiles/randomwalk_bench.json.

    python scripts/randomwalk_bench.py [--reps 7] [--shapes c5,small] [--out profiles/randomwalk_bench.json]

Rosenbrock under the prior u * 20 - 10 (built-in device pair), isotropic directions (generate_random_direction):
  c5     the sampler shape of C5: d = 50, N = 4000 live points, popsize 10^5, nsteps 50
  small  d = 10, N = 400, popsize 1024, nsteps 40
For each shape, on the same region, live points, threshold and scale:
  (a) host   the host loop (no device_rng): numpy directions, device cube intersection, scipy truncnorm.rvs, transform and
             likelihood through the callbacks -- the code path of the parent commit, which this route leaves intact
  (b) chain  the device refill forced through the chain form (three launches per step)
  (c) fused  the device refill as the shape chooses (one launch for all steps)
Two warm-up rounds, then `reps` rounds in which (a), (b), (c) take turns (a drift of the clocks meets all three alike); wall
clock around each refill (every one of them ends in a synchronisation), medians.  Recorded per route: median and minimum
milliseconds per refill and per step, the acceptance rate of the last step; (b) and (c) start every round from the same Philox
position and must return the same points; device name and kernel-source hash.
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SHAPES = dict(c5=dict(d=50, nlive=4000, popsize=100000, nsteps=50), small=dict(d=10, nlive=400, popsize=1024, nsteps=40))


def bench_shape(shape, reps):
    import ultranest_amd.mlfriends as M
    import ultranest_amd.popstepsampler as pop
    from ultranest_amd import likelihoods
    from ultranest_amd.regions import DeviceRNG
    d, N, P, nsteps = shape["d"], shape["nlive"], shape["popsize"], shape["nsteps"]
    rs = np.random.RandomState(1)
    live = np.clip(0.55 + 0.01 * rs.normal(size=(N, d)), 1e-6, 1 - 1e-6)      # around the Rosenbrock's maximum p = 1
    layer = M.AffineLayer()
    layer.optimize(live, live)
    region = M.MLFriends(live.copy(), layer)
    region.maxradiussq, region.enlarge = region.compute_enlargement(nbootstraps=30, rng=np.random.RandomState(2))
    region.create_ellipsoid()
    transform, loglike = likelihoods.rosenbrock_transform, likelihoods.rosenbrock_loglike
    Ls = loglike(transform(live))
    Lmin = float(np.quantile(Ls, 0.02))
    scale = 0.01      # a step of about the live points' spread per coordinate: acceptance well away from 0 and 1

    def sampler(device, chain=False):
        s = pop.PopulationRandomWalkSampler(popsize=P, nsteps=nsteps, generate_direction=pop.generate_random_direction,
                                            scale=scale, scale_adapt_factor=1.0, device_rng=DeviceRNG(7) if device else None)
        s.force_chain_form = chain
        return s

    samplers = dict(a_host=sampler(False), b_chain=sampler(True, True), c_fused=sampler(True))
    ms = {k: [] for k in samplers}
    last = {}
    for r in range(2 + reps):
        for k, s in samplers.items():
            if s.device_rng is not None:
                s.device_rng.offset = 0
            np.random.seed(3)
            s.prepared_samples = []
            t0 = time.perf_counter()
            nc = s._refill(region, Lmin, live, Ls, transform, loglike)
            t1 = time.perf_counter()
            assert nc == P * nsteps
            if r >= 2:
                ms[k].append((t1 - t0) * 1e3)
            last[k] = s
    entry = dict(shape)
    for k, v in ms.items():
        entry[k] = dict(ms_median=float(np.median(v)), ms_min=float(np.min(v)), ms_per_step=float(np.median(v)) / nsteps,
                        last_step_accept_rate=float(last[k].logstat[-1][0]))
    fused, chain = last["c_fused"].last_refill, last["b_chain"].last_refill
    assert chain["chain_form"] and not fused["chain_form"]
    entry["fused_points_equal_chain_points"] = bool(np.array_equal(fused["u"], chain["u"]) and np.array_equal(fused["L"], chain["L"]))
    entry["fused_over_host"] = entry["c_fused"]["ms_median"] / entry["a_host"]["ms_median"]
    entry["chain_over_host"] = entry["b_chain"]["ms_median"] / entry["a_host"]["ms_median"]
    return entry


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--shapes", default="c5,small")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "randomwalk_bench.json"))
    args = ap.parse_args()
    from ultranest_amd import _lib
    from csrc_build import source_hash
    res = dict(device=_lib.device_name(), source_hash=source_hash(), reps=args.reps, model="rosenbrock, u * 20 - 10",
               direction="generate_random_direction")
    for name in args.shapes.split(","):
        res[name] = bench_shape(SHAPES[name], args.reps)
    res["anchor"] = "PopulationSliceSampler's whole step on the device: 0.236 ms per step at 10^5 walkers x 50"
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as fh:
        json.dump(res, fh, indent=1, sort_keys=True)
    print(json.dumps(res, sort_keys=True))


if __name__ == "__main__":
    sys.path.insert(0, os.path.join(ROOT, "ultranest_amd", "csrc"))
    import importlib
    sys.modules["csrc_build"] = importlib.import_module("build")
    main()
