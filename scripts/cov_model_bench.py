#!/usr/bin/env python3
"""The covariance form of a user model (DeviceModel(..., ncov=n): one workgroup per row factorises the row's n x n covariance in
LDS) against what a user had before it: the same model as a host callback.  One GPU, one process; writes
profiles/cov_model_bench.json.

    python scripts/cov_model_bench.py [--reps 10] [--out profiles/cov_model_bench.json]

Model: usermodels.gp_sqexp(n, affine=True), 4 parameters.  Shapes: 1024 and 16384 rows; n = 32, 64, 128 and max_ncov.

  device   DeviceModel.eval_dev on resident rows, p and L written; device events around `inner` launches on one stream (the method
           and the input ring of scripts/summed_model_bench.py)
  host     the callback a user writes in numpy: the kernel matrices of all rows at once, batched np.linalg.cholesky, a batched
           triangular solve by np.linalg.solve, the sums; wall time of the call; the BLAS thread count is what the environment
           sets (recorded)

A PopulationSimpleSliceSampler refill (popsize 1024, 10 steps) at n = 64 through the device route and through the host callback.

Per shape the device time per row is set against two bounds from the figures of the MI355X guide, both for all 256 CUs busy with
n^3/6 + n^2/2 updates per row, each update reading col[i], col[j] and its own element from LDS and writing it back:
  lds    24 bytes read at 150 TB/s (ds_read_b64, chip) and 8 bytes written at 38 TB/s (ds_write_b64, the lower end given)
  fp64   one multiplication and one subtraction, unfused, at the FP64 vector rate counted without FMA: a quarter of the 157.3
         TFLOP/s the guide gives for FP32 vector FMA (FP64 vector is half the FP32 rate on this part)
and `binds` names the larger; `over_bound` is measured / that bound.
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
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import summed_model_bench as SB  # noqa: E402   (the window constants)

ROWS = (1024, 16384)
LDS_READ, LDS_WRITE, FP64_UNFUSED = 150e12, 38e12, 157.3e12 / 4


def host_loglike(x, y):
    """the vectorised numpy callback of the same model (parameters in, L out)"""
    n = len(x)
    dx2 = (x[:, None] - x[None, :]) ** 2
    eye = np.eye(n)

    def loglike(p):
        if len(p) > 1024:      # (1024 rows at a time: the matrices of 16384 rows at n = 199 would take 5 GB)
            return np.concatenate([loglike(p[k:k + 1024]) for k in range(0, len(p), 1024)])
        a2, l2, s2 = np.exp(2 * p[:, 0]), np.exp(2 * p[:, 1]), np.exp(2 * p[:, 2])
        K = a2[:, None, None] * np.exp(-dx2[None] / (2.0 * l2)[:, None, None]) + s2[:, None, None] * eye[None]
        Lc = np.linalg.cholesky(K)
        z = np.linalg.solve(Lc, (y[None, :] - p[:, 3:4])[:, :, None])[:, :, 0]
        return -0.5 * (z * z).sum(axis=1) - np.log(np.diagonal(Lc, axis1=1, axis2=2)).sum(axis=1) - 0.5 * n * np.log(2 * np.pi)
    return loglike


def device_timing(torch, model, rows, reps):
    dev = torch.device("cuda")
    gen = torch.Generator(device=dev)
    gen.manual_seed(rows)
    ring = [torch.rand((rows, 4), dtype=torch.float64, device=dev, generator=gen) for _ in range(4)]
    tp = torch.empty((rows, 4), dtype=torch.float64, device=dev)
    tL = torch.empty(rows, dtype=torch.float64, device=dev)
    stream = torch.cuda.current_stream().cuda_stream
    pos = [0]

    def window(inner):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(inner):
            model.eval_dev(ring[pos[0] % 4].data_ptr(), rows, tp.data_ptr(), tL.data_ptr(), None, stream)
            pos[0] += 1
        b.record()
        b.synchronize()
        return a.elapsed_time(b) / inner

    window(1)
    inner = int(min(200, max(1, round(SB.WINDOW_MS / max(window(2), 1e-3)))))
    for _ in range(3):
        window(inner)
    ms = [window(inner) for _ in range(reps)]
    model.eval_dev(ring[0].data_ptr(), rows, tp.data_ptr(), tL.data_ptr(), None, stream)
    torch.cuda.synchronize()
    return ms, inner, tp.cpu().numpy(), tL.cpu().numpy()


def refill(usermodels, n, reps):
    import ultranest_amd.mlfriends as M
    import ultranest_amd.popstepsampler as pop
    from ultranest_amd.regions import DeviceRNG
    P, nsteps, nlive = 1024, 10, 400
    model = usermodels.gp_sqexp(n, affine=True)
    x, y = usermodels.gp_data(n)
    host = host_loglike(x, y)
    lo, width = np.array(usermodels.GP_PRIOR_LO), np.array(usermodels.GP_PRIOR_WIDTH)
    pairs = dict(device=(model.transform, model.loglike), host=(lambda u: u * width + lo, host))
    us = np.clip(0.5 + 0.05 * np.random.RandomState(2).normal(size=(nlive, 4)), 0.01, 0.99)
    Ls = model.loglike(model.transform(us))
    Lmin = float(Ls.min() - 0.5)
    layer = M.AffineLayer()
    layer.optimize(us, us)
    region = types.SimpleNamespace(u=us, transformLayer=layer, maxradiussq=4.0)
    out = {}
    for name, (tr, ll) in pairs.items():
        s = pop.PopulationSimpleSliceSampler(P, nsteps, pop.generate_mixture_random_direction, scale=1.0, device_rng=DeviceRNG(7))
        ms = []
        for r in range(1 + reps):
            s.prepared_samples = []
            t0 = time.perf_counter()
            s.__next__(region, Lmin, us, Ls, tr, ll)
            if r >= 1:
                ms.append((time.perf_counter() - t0) * 1e3)
        out[name] = dict(ms_median=float(np.median(ms)), ms_min=float(np.min(ms)), likelihood_calls_last_refill=int(s.ncalls))
    out.update(popsize=P, nsteps=nsteps, ncov=n, nlive=nlive, reps=reps, host_over_device=out["host"]["ms_median"] / out["device"]["ms_median"])
    model.close()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--host-reps", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "cov_model_bench.json"))
    args = ap.parse_args()
    import torch
    from ultranest_amd import _lib, devicemodel, usermodels
    from csrc_build import source_hash
    if _lib.device_count() == 0:
        raise SystemExit("no GPU visible: nothing is measured")
    nmax = devicemodel.max_ncov(4, True)
    res = dict(device=_lib.device_name(), source_hash=source_hash(), reps=args.reps, host_reps=args.host_reps,
               model="usermodels.gp_sqexp(n, affine=True)", host_threads=os.environ.get("OMP_NUM_THREADS"), max_ncov=nmax,
               bounds=dict(lds_read_bytes_per_s=LDS_READ, lds_write_bytes_per_s=LDS_WRITE, fp64_unfused_flop_per_s=FP64_UNFUSED),
               kernel=[])
    for n in (32, 64, 128, nmax):
        model = usermodels.gp_sqexp(n, affine=True)
        host = host_loglike(*usermodels.gp_data(n))
        updates = n ** 3 / 6.0 + n ** 2 / 2.0
        t_lds, t_fp = updates * (24 / LDS_READ + 8 / LDS_WRITE), updates * 2 / FP64_UNFUSED
        for rows in ROWS:
            ms, inner, p, L = device_timing(torch, model, rows, args.reps)
            hms = []
            for r in range(1 + args.host_reps):
                t0 = time.perf_counter()
                Lh = host(p)
                if r >= 1:
                    hms.append((time.perf_counter() - t0) * 1e3)
            per_row = float(np.median(ms)) * 1e-3 / rows
            entry = dict(rows=rows, ncov=n, inner=inner, device_ms_median=float(np.median(ms)), device_ms_min=float(np.min(ms)),
                         host_ms_median=float(np.median(hms)), host_ms_min=float(np.min(hms)),
                         host_over_device=float(np.median(hms) / np.median(ms)),
                         max_relative_difference=float((np.abs(L - Lh) / np.abs(Lh)).max()),
                         device_seconds_per_row=per_row, lds_bound_seconds_per_row=t_lds, fp64_bound_seconds_per_row=t_fp,
                         binds="lds" if t_lds > t_fp else "fp64", over_bound=per_row / max(t_lds, t_fp),
                         barriers_per_row=2 * n + 6)
            res["kernel"].append(entry)
            print(json.dumps(entry, sort_keys=True), flush=True)
        model.close()
    res["refill"] = refill(usermodels, 64, max(2, args.host_reps))
    print(json.dumps(res["refill"], sort_keys=True), flush=True)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as fh:
        json.dump(res, fh, indent=1, sort_keys=True)


if __name__ == "__main__":
    sys.path.insert(0, os.path.join(ROOT, "ultranest_amd", "csrc"))
    import importlib
    sys.modules["csrc_build"] = importlib.import_module("build")
    main()
