#!/usr/bin/env python3
"""The summed form of a user model against its default-form twin, measured on one GPU in one process; writes
profiles/summed_model_bench.json.

    python scripts/summed_model_bench.py [--reps 20] [--out profiles/summed_model_bench.json]

usermodels.linear_sum at d = 10 under the prior u * 20 - 10 (summed form: one wave per row, the 64 lanes split the K terms)
and usermodels.linear_twin (default form: one thread per row walks the K terms; the only form there was before, so it is the
baseline).

Kernel timing: DeviceModel.eval_dev on resident rows, with p and L written (the summed form's one-lane transform is inside the
figure), rows x K as listed in ROWS x TERMS.  Device events around `inner` launches on one stream, `inner` chosen in the
warm-up so that a timed window is a few milliseconds; the launches of a window walk through a ring of input buffers that
together exceed the 256 MiB Infinity Cache where the shape allows it (at most 32 buffers), so the rows of the larger shapes
come from memory; the model's own data (aux, K * 12 doubles) is resident data of the model and stays where the hardware keeps
it.  Three warm-up windows, then `reps` windows in which the two forms take turns; median and minimum of the per-launch time.
"speedup" is twin / summed.  "crossover" names, per K, the row counts between which the ratio passes 1 (or says that it
does not within the measured range).  Both forms' L are compared on the first buffer (relative to the sum of the terms'
magnitudes, which is what the forms' different orders are bounded by).

End to end: one refill of PopulationSimpleSliceSampler(device_rng=...) at popsize 1024, nsteps 10, K = 16384, wall clock around
the refilling __next__ (it synchronises), one warm-up refill and `e2e_reps` timed ones per form, taking turns.
"""
import argparse
import json
import os
import sys
import time
import types

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

D = 10
ROWS = (256, 1024, 4096, 16384, 65536, 2 ** 17)
TERMS = (1024, 16384)
CACHE_BYTES = 256 << 20
MAX_BUFFERS = 32
WINDOW_MS = 4.0


def kernel_timing(torch, models, rows, reps):
    """per-launch milliseconds of each model's eval_dev at `rows` rows: dict name -> list of `reps` window means"""
    dev = torch.device("cuda")
    nbuf = int(min(MAX_BUFFERS, max(2, -(-int(1.25 * CACHE_BYTES) // (rows * D * 8)))))
    gen = torch.Generator(device=dev)
    gen.manual_seed(rows)
    # around the data's own parameters (|p| of order 1): u = (p + 10) / 20
    ring = [0.5 + 0.05 * torch.randn((rows, D), dtype=torch.float64, device=dev, generator=gen) for _ in range(nbuf)]
    tp = torch.empty((rows, D), dtype=torch.float64, device=dev)
    tL = {k: torch.empty(rows, dtype=torch.float64, device=dev) for k in models}
    stream = torch.cuda.current_stream().cuda_stream
    pos = dict.fromkeys(models, 0)

    def window(name, inner):
        m = models[name]
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(inner):
            m.eval_dev(ring[pos[name] % nbuf].data_ptr(), rows, tp.data_ptr(), tL[name].data_ptr(), None, stream)
            pos[name] += 1
        b.record()
        b.synchronize()
        return a.elapsed_time(b) / inner

    inner = {}
    for name in models:      # warm-up: the code object is loaded, and one launch is timed to size the window
        window(name, 1)
        one = max(window(name, 2), 1e-3)
        inner[name] = int(min(200, max(1, round(WINDOW_MS / one))))
        for _ in range(3):
            window(name, inner[name])
    ms = {k: [] for k in models}
    for _ in range(reps):
        for name in models:
            ms[name].append(window(name, inner[name]))
    # the two forms on the same rows
    for name, m in models.items():
        m.eval_dev(ring[0].data_ptr(), rows, tp.data_ptr(), tL[name].data_ptr(), None, stream)
    torch.cuda.synchronize()
    return ms, inner, nbuf, {k: v.cpu().numpy() for k, v in tL.items()}, (ring[0] * 20.0 + -10.0).cpu().numpy()


def crossover(rows, speedups):
    """between which measured row counts twin / summed passes 1"""
    above = [s > 1.0 for s in speedups]
    if all(above):
        return "the summed form is faster at every measured row count (up to %d rows)" % rows[-1]
    if not any(above):
        return "the default form is faster at every measured row count (from %d rows)" % rows[0]
    for i in range(len(rows) - 1):
        if above[i] and not above[i + 1]:
            return "between %d rows (summed form %.2fx faster) and %d rows (%.2fx)" % (rows[i], speedups[i], rows[i + 1],
                                                                                      speedups[i + 1])
    return "not monotonic: " + ", ".join("%d: %.2fx" % rs for rs in zip(rows, speedups))


def end_to_end(usermodels, K, reps):
    import ultranest_amd.mlfriends as M
    import ultranest_amd.popstepsampler as pop
    from ultranest_amd.regions import DeviceRNG
    P, nsteps, nlive = 1024, 10, 400
    models = dict(summed=usermodels.linear_sum(D, K, seed=1, affine=True), twin=usermodels.linear_twin(D, K, seed=1, affine=True))
    X, y, w = usermodels.linear_data(D, K, seed=1)
    best = np.linalg.lstsq(X * w[:, None], y * w, rcond=None)[0]
    rs = np.random.RandomState(2)
    us = np.clip((best + 10.0) / 20.0 + 0.002 * rs.normal(size=(nlive, D)), 1e-6, 1 - 1e-6)
    Ls = models["twin"].loglike(models["twin"].transform(us))
    Lmin = float(Ls.min() - 0.5)
    layer = M.AffineLayer()
    layer.optimize(us, us)
    region = types.SimpleNamespace(u=us, transformLayer=layer, maxradiussq=float(D))
    samplers = {k: pop.PopulationSimpleSliceSampler(P, nsteps, pop.generate_mixture_random_direction, scale=1.0,
                                                    device_rng=DeviceRNG(7)) for k in models}
    ms = {k: [] for k in models}
    iters = {}
    for r in range(1 + reps):
        for name, m in models.items():
            s = samplers[name]
            s.prepared_samples = []
            t0 = time.perf_counter()
            s.__next__(region, Lmin, us, Ls, m.transform, m.loglike)
            t1 = time.perf_counter()
            if r >= 1:
                ms[name].append((t1 - t0) * 1e3)
            iters[name] = int(s.last_refill["niter"])
    out = {k: dict(ms_median=float(np.median(v)), ms_min=float(np.min(v)), slice_iterations_last_refill=iters[k])
           for k, v in ms.items()}
    out.update(popsize=P, nsteps=nsteps, nterms=K, d=D, nlive=nlive, reps=reps,
               speedup=out["twin"]["ms_median"] / out["summed"]["ms_median"],
               note="likelihood evaluations per refill = popsize * slice iterations; the two forms' runs differ in the last "
                    "bits of L, so their iteration counts need not be equal")
    for m in models.values():
        m.close()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--e2e-reps", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "summed_model_bench.json"))
    args = ap.parse_args()
    import torch
    from ultranest_amd import _lib, usermodels
    from csrc_build import source_hash
    if _lib.device_count() == 0:
        raise SystemExit("no GPU visible: nothing is measured")
    res = dict(device=_lib.device_name(), source_hash=source_hash(), d=D, reps=args.reps, model="usermodels.linear_sum / linear_twin, affine prior",
               timing="device events around `inner` eval_dev launches (p and L written), inputs rotated through `buffers` buffers",
               kernel=[])
    for K in TERMS:
        models = dict(summed=usermodels.linear_sum(D, K, seed=1, affine=True), twin=usermodels.linear_twin(D, K, seed=1, affine=True))
        X, y, w = usermodels.linear_data(D, K, seed=1)
        speedups = []
        for rows in ROWS:
            ms, inner, nbuf, L, p = kernel_timing(torch, models, rows, args.reps)
            c = min(rows, 256)                # the two forms' L on the first rows, against the sum of the terms' magnitudes
            r = (y - p[:c].dot(X.T)) * w
            scale = np.abs(-0.5 * r * r).sum(axis=1)
            entry = dict(rows=rows, nterms=K, buffers=nbuf, input_bytes_in_rotation=nbuf * rows * D * 8, rows_compared=c,
                         max_abs_difference_over_term_magnitudes=float((np.abs(L["summed"][:c] - L["twin"][:c]) / scale).max()))
            for name in models:
                entry[name] = dict(ms_median=float(np.median(ms[name])), ms_min=float(np.min(ms[name])), inner=inner[name])
            entry["speedup"] = entry["twin"]["ms_median"] / entry["summed"]["ms_median"]
            speedups.append(entry["speedup"])
            res["kernel"].append(entry)
            print(json.dumps(entry, sort_keys=True), flush=True)
        res["crossover_nterms_%d" % K] = crossover(ROWS, speedups)
        for m in models.values():
            m.close()
    res["end_to_end_simple_slice_refill"] = end_to_end(usermodels, 16384, args.e2e_reps)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as fh:
        json.dump(res, fh, indent=1, sort_keys=True)
    print(json.dumps(res, sort_keys=True))


if __name__ == "__main__":
    sys.path.insert(0, os.path.join(ROOT, "ultranest_amd", "csrc"))
    import importlib
    sys.modules["csrc_build"] = importlib.import_module("build")
    main()
