#!/usr/bin/env python3
"""One refill of PopulationSimpleSliceSampler on its two routes, measured on one GPU in one process; writes
profiles/simpleslice_bench.json.

    python scripts/simpleslice_bench.py [--reps 5] [--host-reps 2] [--shapes small,c5] [--out profiles/simpleslice_bench.json]

Rosenbrock under the prior u * 20 - 10 (built-in device pair), isotropic directions (generate_random_direction), slices
clipped to [-1, 1] of a direction of length 0.05 (slice_limit_to_scale), threshold below every live point:
  c5     the sampler shape of C5: d = 50, N = 4000 live points, popsize 10^5, nsteps 50
  small  d = 10, N = 400, popsize 1024, nsteps 40
For each shape, on the same region, live points, threshold and scale:
  (a) host    the host loop (no device_rng): numpy directions, device cube intersection, transform and likelihood through the
              callbacks, update_vectorised_slice_sampler per iteration -- the parent commit's only path, the baseline
  (b) device  the device refill (csrc/mlf_sslice.hip), batch policy of the library
One warm-up round, then the host route `host-reps` times and the device route `reps` times; wall clock around each refill
(every one ends in a synchronisation), medians.  Recorded per route: median and minimum milliseconds per refill, per step
and per iteration, iterations per step, likelihood evaluations; device name and kernel-source hash.  The two routes draw
from different random streams, so their iteration counts differ slightly: compare the milliseconds per iteration too.
The file is rewritten after every shape.
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


def bench_shape(shape, reps, host_reps):
    import types
    import ultranest_amd.mlfriends as M
    import ultranest_amd.popstepsampler as pop
    from ultranest_amd import likelihoods
    from ultranest_amd.regions import DeviceRNG
    d, N, P, nsteps = shape["d"], shape["nlive"], shape["popsize"], shape["nsteps"]
    rs = np.random.RandomState(1)
    live = np.clip(0.55 + 0.01 * rs.normal(size=(N, d)), 1e-6, 1 - 1e-6)      # around the Rosenbrock's maximum p = 1
    layer = M.AffineLayer()
    layer.optimize(live, live)
    region = types.SimpleNamespace(u=live, transformLayer=layer, maxradiussq=float(d))
    transform, loglike = likelihoods.rosenbrock_transform, likelihoods.rosenbrock_loglike
    Ls = loglike(transform(live))
    Lmin = float(Ls.min()) - 1.0      # every start row lies above the threshold, as in a nested-sampling run

    def sampler(device):
        return pop.PopulationSimpleSliceSampler(popsize=P, nsteps=nsteps, generate_direction=pop.generate_random_direction,
                                                scale=0.05, slice_limit=pop.slice_limit_to_scale,
                                                device_rng=DeviceRNG(7) if device else None)

    entry = dict(shape)
    for key, s, n in (("a_host", sampler(False), host_reps), ("b_device", sampler(True), reps)):
        ms, ncs = [], []
        for r in range(1 + n):
            if s.device_rng is not None:
                s.device_rng.offset = 0
            np.random.seed(3)
            s.prepared_samples = []
            t0 = time.perf_counter()
            nc = s._refill(region, Lmin, live, Ls, transform, loglike)
            t1 = time.perf_counter()
            if r >= 1:
                ms.append((t1 - t0) * 1e3)
                ncs.append(nc)
        med = float(np.median(ms))
        niter = float(np.median(ncs)) / P
        entry[key] = dict(ms_median=med, ms_min=float(np.min(ms)), ms_per_step=med / nsteps, ms_per_iteration=med / niter,
                          iterations_per_step=niter / nsteps, likelihood_evaluations=int(np.median(ncs)), refills_timed=n)
        assert (s._sslice is not None) == (key == "b_device")
    entry["device_over_host"] = entry["b_device"]["ms_median"] / entry["a_host"]["ms_median"]
    entry["device_over_host_per_iteration"] = entry["b_device"]["ms_per_iteration"] / entry["a_host"]["ms_per_iteration"]
    return entry


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--host-reps", type=int, default=2)
    ap.add_argument("--shapes", default="small,c5")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "simpleslice_bench.json"))
    args = ap.parse_args()
    from ultranest_amd import _lib
    from csrc_build import source_hash
    res = dict(device=_lib.device_name(), source_hash=source_hash(), reps=args.reps, host_reps=args.host_reps,
               model="rosenbrock, u * 20 - 10", direction="generate_random_direction", slice_limit="slice_limit_to_scale, scale 0.05")
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    for name in args.shapes.split(","):
        res[name] = bench_shape(SHAPES[name], args.reps, args.host_reps)
        with open(args.out, "w") as fh:
            json.dump(res, fh, indent=1, sort_keys=True)
        print(json.dumps({name: res[name]}, sort_keys=True), flush=True)


if __name__ == "__main__":
    sys.path.insert(0, os.path.join(ROOT, "ultranest_amd", "csrc"))
    import importlib
    sys.modules["csrc_build"] = importlib.import_module("build")
    main()
