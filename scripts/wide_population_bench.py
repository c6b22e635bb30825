#!/usr/bin/env python3
"""PopulationRandomWalkSampler and PopulationSimpleSliceSampler above 128 dimensions: the host loop against the device refill,
measured on one GPU in one process; writes profiles/wide_population_bench.json.

    python scripts/wide_population_bench.py [--reps 7] [--dims 128,256,512,1024] [--append] [--out profiles/wide_population_bench.json]
    python scripts/wide_population_bench.py --consecutive 24 --dims 512 [--out ...]
    python scripts/wide_population_bench.py --profile-shape                      (under rocprofv3 --kernel-trace --stats)
    python scripts/wide_population_bench.py --fold-kernel-stats <kernel_stats.csv> [--out ...]     (no GPU needed)

popsize 1024, nsteps 16, DeviceRNG, at d = 128 (the narrow propose kernels, the anchor of every ratio) and 256, 512, 1024 (the
wide ones).  The region is an affine layer optimised on the host over 400 live points (d + 176 from d = 400 on: an affine
layer needs more points than dimensions) around the Gaussian's centre; threshold just below the lowest live point, as in a
nested-sampling run; no scale adaptation, so every refill of a run does the same work.
  samplers    randomwalk (scale 0.05), simpleslice (unit-cube slices, max_it 100)
  models      builtin  identity transform + GaussLikelihood (above 128 dimensions: one thread per row)
              user     usermodels.gauss (the user-model wrapper kernel)
  directions  region-random (a d x d matrix-vector product per direction), mixture, cube-oriented
  routes      (a) the sampler without device_max_dim: above 128 dimensions the host loop -- numpy / scipy draws, one host
                  round trip per step or iteration; what the parent commit runs there.  At d = 128 it is the device refill too
              (b) the sampler with device_max_dim = 1024: the device refill
Two warm-up rounds, then `reps` rounds in which all runs take turns (a drift of the clocks meets all alike); wall clock around
one refill (every one ends in a synchronisation or with the results on the host); median and minimum over the rounds.
Recorded per run: milliseconds per refill, likelihood evaluations per refill, refills that ended in one of the samplers'
assertions (raised after the work is done); per shape a / b; every number's ratio to d = 128 of the same run; device
name and kernel-source hash.  A d = 1024 host refill with region-random directions takes about ten seconds (its einsum), so the
dims may be measured in several processes, each with d = 128 as its own anchor: --append adds this process's run to the runs
already in the file.

--consecutive N times N device refills in a row, with nothing between them, of the random walk (built-in model, region-random
and mixture directions) at each of the dims and adds every single time to the JSON: in the rounds above a device refill follows
other runs' host loops, during which the device idles for up to seconds.

--profile-shape runs ten device refills of both samplers at d = 1024 (built-in model, region-random directions) and nothing
else: the program to put behind `rocprofv3 --kernel-trace --stats --`.  --fold-kernel-stats reads that run's kernel_stats.csv
and adds the shares of the propose and the diagnostics kernels to the JSON.
"""
import argparse
import csv
import json
import os
import sys
import time
import types

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

POPSIZE, NSTEPS = 1024, 16
DIRECTIONS = ("generate_region_random_direction", "generate_mixture_random_direction", "generate_cube_oriented_direction")
KERNELS = dict(randomwalk=("k_rwalk_propose", "k_rwalk_dist"), simpleslice=("k_sslice_propose", "k_sslice_dist"))


def nlive_of(d):
    return 400 if d < 400 else d + 176


def problem(d):
    import ultranest_amd.mlfriends as M
    from ultranest_amd import usermodels
    rs = np.random.RandomState(1000 + d)
    centers = usermodels.gauss_centers(d)
    u = np.clip(centers + 0.05 * rs.normal(size=(nlive_of(d), d)), 1e-3, 1 - 1e-3)
    layer = M.AffineLayer()
    layer.optimize(u, u)
    return types.SimpleNamespace(u=u, transformLayer=layer, maxradiussq=float(d)), centers


def make_sampler(which, direction, device_max_dim):
    import ultranest_amd.popstepsampler as pop
    from ultranest_amd.regions import DeviceRNG
    kw = {} if device_max_dim is None else dict(device_max_dim=device_max_dim)
    if which == "randomwalk":
        return pop.PopulationRandomWalkSampler(popsize=POPSIZE, nsteps=NSTEPS, generate_direction=getattr(pop, direction),
                                               scale=0.05, scale_adapt_factor=1.0, device_rng=DeviceRNG(7), **kw)
    return pop.PopulationSimpleSliceSampler(popsize=POPSIZE, nsteps=NSTEPS, generate_direction=getattr(pop, direction),
                                            scale_adapt_factor=1.0, device_rng=DeviceRNG(7), **kw)


def refill(run):
    """one refill on the clock: (milliseconds, likelihood evaluations, whether it ended in one of the samplers' assertions --
    a walker that never moved, a host-loop proposal on the cube's face -- which they raise after the work is done)"""
    s = run["sampler"]
    s.prepared_samples = []
    never = False
    t0 = time.perf_counter()
    try:
        nc = s.__next__(*run["args"])[3]
    except AssertionError:
        nc, never = 0, True
    t1 = time.perf_counter()
    return (t1 - t0) * 1e3, nc, never


def summary(ms):
    return dict(ms_median=float(np.median(ms)), ms_min=float(np.min(ms)), ms_max=float(np.max(ms)))


def models_of(d, centers):
    from ultranest_amd import likelihoods, usermodels
    G = usermodels.gauss(d)
    return dict(builtin=(likelihoods.identity_transform, likelihoods.GaussLikelihood(centers, 0.1, d)),
                user=(G.transform, G.loglike))


def bench(dims, reps):
    runs = []
    for d in dims:
        region, centers = problem(d)
        models = models_of(d, centers)
        Ls = models["builtin"][1](region.u)
        Lmin = float(Ls.min() - 0.1)
        for which in ("randomwalk", "simpleslice"):
            for model, (transform, loglike) in models.items():
                for direction in DIRECTIONS:
                    for route, max_dim in (("a", None), ("b", 1024)):
                        s = make_sampler(which, direction, max_dim)
                        on_device = s._device_route(transform, loglike, d) is not None
                        runs.append(dict(d=d, sampler_name=which, model=model, direction=direction, route=route,
                                         on_device=on_device, sampler=s, ms=[], nc=[], never=0,
                                         args=(region, Lmin, region.u, Ls, transform, loglike)))
    np.random.seed(1)      # (the host loops draw from np.random)
    for r in range(2 + reps):
        for run in runs:
            ms, nc, never = refill(run)
            if r >= 2:
                run["ms"].append(ms)
                run["nc"].append(nc)
                run["never"] += never
        print("round %d of %d done" % (r + 1, 2 + reps), file=sys.stderr, flush=True)
    rows = [dict(d=run["d"], sampler=run["sampler_name"], model=run["model"], direction=run["direction"], route=run["route"],
                 on_device=run["on_device"], likelihood_evals_per_refill=float(np.mean(run["nc"])),
                 refills_ending_in_an_assertion=run["never"], **summary(run["ms"])) for run in runs]

    def key(row):
        return row["sampler"], row["model"], row["direction"]
    for row in rows:
        anchor = [x for x in rows if x["d"] == 128 and key(x) == key(row) and x["route"] == row["route"]]
        row["over_d128"] = row["ms_median"] / anchor[0]["ms_median"] if anchor else None
    ratios = []
    for b in (x for x in rows if x["route"] == "b"):
        a = [x for x in rows if x["route"] == "a" and x["d"] == b["d"] and key(x) == key(b)][0]
        ratios.append(dict(d=b["d"], sampler=b["sampler"], model=b["model"], direction=b["direction"],
                           a_on_device=a["on_device"], a_ms=a["ms_median"], b_ms=b["ms_median"],
                           a_over_b=a["ms_median"] / b["ms_median"]))
    return rows, ratios


def consecutive(dims, n):
    rows = []
    for d in dims:
        region, centers = problem(d)
        transform, loglike = models_of(d, centers)["builtin"]
        Ls = loglike(region.u)
        for direction in DIRECTIONS[:2]:
            run = dict(sampler=make_sampler("randomwalk", direction, 1024),
                       args=(region, float(Ls.min() - 0.1), region.u, Ls, transform, loglike))
            ms = [refill(run)[0] for _ in range(2 + n)][2:]
            rows.append(dict(d=d, sampler="randomwalk", model="builtin", direction=direction, ms=ms, **summary(ms)))
    return rows


def profile_shape():
    d = 1024
    region, centers = problem(d)
    transform, loglike = models_of(d, centers)["builtin"]
    Ls = loglike(region.u)
    for which in ("randomwalk", "simpleslice"):
        run = dict(sampler=make_sampler(which, DIRECTIONS[0], 1024), args=(region, float(Ls.min() - 0.1), region.u, Ls, transform, loglike))
        assert run["sampler"]._device_route(transform, loglike, d) is not None
        for _ in range(10):
            refill(run)


def fold_kernel_stats(path):
    """kernel_stats.csv of rocprofv3 --kernel-trace --stats: per sampler the propose and the diagnostics kernel's share of the
    time of all kernels in the run"""
    with open(path) as fh:
        rows = list(csv.DictReader(fh))
    total = sum(float(r["TotalDurationNs"]) for r in rows)
    out = dict(shape="d = 1024, popsize 1024, nsteps 16, built-in Gaussian, region-random directions, ten refills per sampler",
               all_kernels_ms=total / 1e6, kernels=[])
    for which, names in KERNELS.items():
        for name in names:
            hit = [r for r in rows if name in r["Name"]]
            ns = sum(float(r["TotalDurationNs"]) for r in hit)
            out["kernels"].append(dict(sampler=which, kernel=[r["Name"].split("(")[0] for r in hit], calls=sum(int(r["Calls"]) for r in hit),
                                       total_ms=ns / 1e6, share_of_all_kernels=ns / total))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--dims", default="128,256,512,1024")
    ap.add_argument("--append", action="store_true")
    ap.add_argument("--consecutive", type=int, default=0)
    ap.add_argument("--profile-shape", action="store_true")
    ap.add_argument("--fold-kernel-stats", default=None)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "wide_population_bench.json"))
    args = ap.parse_args()
    if args.profile_shape:
        profile_shape()
        return
    if args.fold_kernel_stats:
        with open(args.out) as fh:
            res = json.load(fh)
        res["kernel_shares_d1024"] = fold_kernel_stats(args.fold_kernel_stats)
    elif args.consecutive:
        with open(args.out) as fh:
            res = json.load(fh)
        res["consecutive_device_refills"] = consecutive([int(x) for x in args.dims.split(",")], args.consecutive)
    else:
        dims = [int(x) for x in args.dims.split(",")]
        from ultranest_amd import _lib
        from csrc_build import source_hash
        run = dict(device=_lib.device_name(), source_hash=source_hash(), reps=args.reps, popsize=POPSIZE, nsteps=NSTEPS,
                   nlive={str(d): nlive_of(d) for d in dims}, dims=dims)
        run["refill"], run["host_over_device"] = bench(dims, args.reps)
        res = dict(runs=[])
        if args.append and os.path.exists(args.out):
            with open(args.out) as fh:
                res = json.load(fh)
        res["runs"].append(run)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as fh:
        json.dump(res, fh, indent=1, sort_keys=True)
    print(json.dumps(res, sort_keys=True))


if __name__ == "__main__":
    sys.path.insert(0, os.path.join(ROOT, "ultranest_amd", "csrc"))
    import importlib
    sys.modules["csrc_build"] = importlib.import_module("build")
    main()
