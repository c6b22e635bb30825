"""TEST INFRASTRUCTURE -- numpy restatement of one device refill of PopulationSimpleSliceSampler (csrc/mlf_sslice.hip;
reference ultranest/popstepsampler.py:907-1002, stepfuncs.pyx:537-630): the Philox counter layout, the direction generators
and the cube-line intersection of tests/randomwalk_reference.py, the slice limits, and the reference's update loop over the
workers, literally, with numpy callbacks for the model.

Counter layout (seed, offset of the call):
  stream 2  direction of point k at step s: block group (k * nsteps + s) of (npairs + 2) blocks
  stream 8  block offset + i, word 0 = start row of point i; block offset + P + (s * max_it + it) * P + j, words 0, 1 =
            the uniform of worker j in iteration it of step s
  next offset = offset + max(P * nsteps * (npairs + 2), P * (1 + nsteps * max_it))
"""
import numpy as np

from oracle import philox
from randomwalk_reference import below, directions, line_intersection

STREAM = 8


def next_offset(offset, P, nsteps, d, max_it):
    return offset + max(P * nsteps * ((d + 1) // 2 + 2), P * (1 + nsteps * max_it))


def update(t, tleft, tright, proposed_L, proposed_u, proposed_p, worker_running, status, threshold, shrink, allu, allL, allp,
           popsize, margins=None):
    """stepfuncs.pyx:537-630, literally; arrays updated in place and returned like the reference, then the number of
    discarded proposals and `taken` (per point the worker whose proposal it took, -1: none).  margins (a list): every
    comparison of a t with a bound appends |t - bound| / max(1, |t|)."""
    taken = np.full(popsize, -1, dtype=np.int64)
    discarded = 0
    for j in range(popsize):
        k = worker_running[j]
        tj = t[j]
        if margins is not None:
            margins.append(abs(tj - tright[k]) / max(1.0, abs(tj)))
            margins.append(abs(tj - tleft[k]) / max(1.0, abs(tj)))
        if tj > tright[k] or tj < tleft[k]:
            if proposed_L[j] > threshold:
                discarded += 1
            continue
        if 0 < tj and tj < tright[k]:
            tright[k] = tj / shrink
        if 0 > tj and tj > tleft[k]:
            tleft[k] = tj / shrink
        if proposed_L[j] > threshold and status[k] == 0:
            status[k] = 1
            allu[k, :] = proposed_u[j, :]
            allL[k] = proposed_L[j]
            allp[k, :] = proposed_p[j, :]
            taken[k] = j
    zlist = np.flatnonzero(status == 0)
    if len(zlist):
        worker_running[:] = zlist[np.arange(popsize) % len(zlist)]
    return tleft, tright, worker_running, status, allu, allL, allp, discarded, taken


def refill(seed, offset, us, Ls, Lmin, kind, dirscale, limit, shrink, P, nsteps, max_it, transform, loglike, axes=None, std=None,
           whiten=None, maxradiussq=None):
    """One refill.  dirscale: one direction length per step; limit 0 = unit cube, 1 = clipped to [-1, 1].  Returns the
    per-point results (u, p, L, start, tleft, tright, taken, taken_it of the last step), per step `iters` and `widths`, the
    counts as the device reports them (discarded, niter, nfar, sumlog, nnan), the next offset, the smallest margins
    (min_L_margin: |L - Lmin| / max(1, |Lmin|) over all proposals; min_t_margin: over all comparisons of a t with a bound)
    and `steps`: per step v and the list `its` of per-iteration dicts (t, Lnew, unew, worker_running and nz BEFORE the
    update; tleft, tright, status, discarded, taken after it)."""
    us, Ls = np.asarray(us, dtype=float), np.asarray(Ls, dtype=float)
    nlive, d = us.shape
    rows = np.arange(P, dtype=np.uint64)
    start = below(philox.blocks(seed, STREAM, np.uint64(offset) + rows)[:, 0], nlive)
    u, L = us[start].copy(), Ls[start].copy()
    p = np.full((P, d), np.nan)
    tleft = tright = np.full(P, np.nan)
    taken_last = np.full(P, -1, dtype=np.int64)
    taken_it = np.full(P, -1, dtype=np.int64)
    discarded = niter = 0
    iters, widths, steps = [], [], []
    t_margins = []
    min_L_margin = np.inf
    for s in range(nsteps):
        v = directions(seed, offset, kind, dirscale[s], P, nsteps, s, d, axes=axes, live=us, std=std)
        tleft, tright = line_intersection(u, v)
        if limit == 1:
            tleft, tright = np.fmax(tleft, -1.0), np.fmin(tright, 1.0)
        worker_running = np.arange(P, dtype=np.int64)
        status = np.zeros(P, dtype=np.int64)
        taken_last[:] = -1
        taken_it[:] = -1
        its = []
        for it in range(max_it):
            ctr = np.uint64(offset) + np.uint64(P) + np.uint64((s * max_it + it) * P) + rows
            w = philox.blocks(seed, STREAM, ctr)
            wl, wr = tleft[worker_running], tright[worker_running]
            t = wl + (wr - wl) * philox.u01(w[:, 0], w[:, 1])
            unew = u[worker_running] + t.reshape((-1, 1)) * v[worker_running]
            pnew = np.asarray(transform(unew), dtype=float)
            with np.errstate(all="ignore"):
                Lnew = np.asarray(loglike(pnew), dtype=float)
            min_L_margin = min(min_L_margin, np.abs(Lnew - Lmin).min() / max(1.0, abs(Lmin)))
            before = dict(t=t, Lnew=Lnew, unew=unew, worker_running=worker_running.copy(), nz=int((status == 0).sum()))
            tleft, tright, worker_running, status, u, L, p, nd, taken = update(
                t, tleft, tright, Lnew, unew, pnew, worker_running, status, Lmin, shrink, u, L, p, P, margins=t_margins)
            got = taken >= 0
            taken_last[got] = taken[got]
            taken_it[got] = it
            discarded += nd
            niter += 1
            before.update(tleft=tleft.copy(), tright=tright.copy(), status=status.copy(), discarded=nd, taken=taken)
            its.append(before)
            if not np.any(status == 0):
                break
        iters.append(len(its))
        widths.append(tright - tleft)
        steps.append(dict(v=v, its=its))
    nfar, sumlog = 0.0, 0.0
    if maxradiussq is not None:
        d2 = ((whiten(us[start]) - whiten(u))**2).sum(axis=1)
        nfar = float((d2 > maxradiussq).sum())
        sumlog = float(np.log(np.sqrt(d2) / np.sqrt(maxradiussq) + 1e-10).sum())
    return dict(u=u, p=p, L=L, start=start, tleft=tleft, tright=tright, taken=taken_last, taken_it=taken_it,
                iters=np.array(iters), widths=np.array(widths), discarded=discarded, niter=niter, nfar=nfar, sumlog=sumlog,
                nnan=int((~np.isfinite(p).all(axis=1)).sum()), next_offset=next_offset(offset, P, nsteps, d, max_it),
                min_L_margin=min_L_margin, min_t_margin=min(t_margins), steps=steps)
