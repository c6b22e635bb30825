"""TEST INFRASTRUCTURE -- numpy restatement of one device refill of PopulationRandomWalkSampler (csrc/mlf_rwalk.hip;
reference ultranest/popstepsampler.py:299-353): the Philox counter layout, the direction generators, the cube-line
intersection, the truncated-normal inverse CDF and the accept rule, with numpy callbacks for the model.

Counter layout (seed, offset of the call):
  stream 2  direction of walker i at step s: block group (i * nsteps + s) of (npairs + 2) blocks (block 0: integer picks
            and the mixture coin; blocks 1 ...: Box-Muller pairs)
  stream 7  walker i owns blocks offset + i * (nsteps + 1) + [0, nsteps]: block 0 word 0 = start row, block 1 + s words
            0, 1 = the truncation uniform of step s
  next offset = offset + P * nsteps * (npairs + 2)
"""
import numpy as np

from oracle import philox

STREAM = 7


def _u64(x):
    return np.asarray(x, dtype=np.uint64)


def below(word, n):
    return ((word.astype(np.uint64) * np.uint64(n)) >> np.uint64(32)).astype(np.int64)


def truncnorm_icdf(a, b, q):
    """Standard normal truncated to [a, b] at quantile q, evaluated on the side of the smaller tail:
    p = Phi(a) + q (Phi(b) - Phi(a)); p <= 0.5: Phi^-1(p); else -Phi^-1(Q(b) + (1 - q)(Q(a) - Q(b))), Q(x) = Phi(-x);
    clamped to [a, b]."""
    from scipy.special import ndtr, ndtri      # (not at import: collecting the suite must not load scipy's BLAS pool)
    a, b, q = np.broadcast_arrays(np.asarray(a, dtype=float), np.asarray(b, dtype=float), np.asarray(q, dtype=float))
    Fa, Fb = ndtr(a), ndtr(b)
    p = Fa + q * (Fb - Fa)
    Qa, Qb = ndtr(-a), ndtr(-b)
    with np.errstate(all="ignore"):
        t = np.where(p <= 0.5, ndtri(p), -ndtri(Qb + (1.0 - q) * (Qa - Qb)))
    return np.minimum(np.maximum(t, a), b)


def line_intersection(u, v):
    """(tleft, tright) of u + t v with the unit cube; coordinates the direction does not move along are ignored."""
    with np.errstate(all="ignore"):
        m = 1.0 / v
        nn = m * (u - 0.5)
        kk = np.abs(m) * 0.5
        t1, t2 = -nn - kk, -nn + kk
        import warnings
        with warnings.catch_warnings():
            warnings.simplefilter("ignore", RuntimeWarning)
            return np.nanmax(t1, axis=1), np.nanmin(t2, axis=1)


def directions(seed, offset, kind, dirscale, P, nsteps, step, d, axes=None, live=None, std=None):
    """Rows v[i] of walker i at `step`: the device generator dw_direction (kinds 0-6 = the reference's seven functions)."""
    npairs = (d + 1) // 2
    per = np.uint64(npairs + 2)
    base = np.uint64(offset) + (np.arange(P, dtype=np.uint64) * np.uint64(nsteps) + np.uint64(step)) * per
    pick = philox.blocks(seed, 2, base)
    k = np.full(P, kind)
    if kind == 6:
        k = np.where(philox.u01(pick[:, 2], pick[:, 3]) < 0.5, 5, 3)
    v = np.zeros((P, d))
    rows = np.arange(P)
    axis = below(pick[:, 0], d)
    if kind in (0, 1):
        v[rows, axis] = dirscale if kind == 0 else dirscale * np.asarray(std)[axis]
    if (k == 3).any():
        sel = k == 3
        v[sel] = np.asarray(axes)[axis[sel]] * dirscale
    if (k == 5).any():
        sel = k == 5
        nlive = len(live)
        a = below(pick[:, 0], nlive)
        b = below(pick[:, 1], nlive - 1)
        b = b + (b >= a)
        v[sel] = ((live[a] - live[b]) * dirscale)[sel]
    if kind in (2, 4):
        g = np.empty((P, 2 * npairs))
        for j in range(npairs):
            w = philox.blocks(seed, 2, base + np.uint64(1 + j))
            rad = np.sqrt(-2.0 * np.log(philox.u01(w[:, 0], w[:, 1])))
            ang = 2.0 * np.pi * philox.u01(w[:, 2], w[:, 3])
            g[:, 2 * j] = rad * np.cos(ang)
            g[:, 2 * j + 1] = rad * np.sin(ang)
        g = g[:, :d]
        g = g * (dirscale / np.sqrt((g * g).sum(axis=1)))[:, None]
        v = g if kind == 2 else np.einsum('ij,kj->ki', np.asarray(axes), g)
    return v


def next_offset(offset, P, nsteps, d):
    return offset + P * nsteps * ((d + 1) // 2 + 2)


def refill(seed, offset, us, Ls, Lmin, kind, dirscale, P, nsteps, transform, loglike, axes=None, std=None, whiten=None,
           maxradiussq=None):
    """One refill.  Returns the per-walker results (u, p, L, start, ever, last), the counts as the device reports them
    (nrejects, nlast, nfar, sumlog, nnever), the next offset, and `steps`: per step (v, tleft, tright, t, unew, Lnew,
    inside, accepted)."""
    us, Ls = np.asarray(us, dtype=float), np.asarray(Ls, dtype=float)
    nlive, d = us.shape
    mine = np.uint64(offset) + np.arange(P, dtype=np.uint64) * np.uint64(nsteps + 1)
    start = below(philox.blocks(seed, STREAM, mine)[:, 0], nlive)
    u, L = us[start].copy(), Ls[start].copy()
    p = np.full((P, d), np.nan)
    ever = np.zeros(P, dtype=bool)
    acc = np.zeros(P, dtype=bool)
    nrejects = 0
    steps = []
    for s in range(nsteps):
        v = directions(seed, offset, kind, dirscale, P, nsteps, s, d, axes=axes, live=us, std=std)
        tl, tr = line_intersection(u, v)
        w = philox.blocks(seed, STREAM, mine + np.uint64(1 + s))
        t = truncnorm_icdf(tl, tr, philox.u01(w[:, 0], w[:, 1]))
        unew = u + v * t[:, None]
        inside = np.logical_and(unew > 0, unew < 1).all(axis=1)
        pnew = np.asarray(transform(unew), dtype=float)
        with np.errstate(all="ignore"):
            Lnew = np.asarray(loglike(pnew), dtype=float)
        acc = np.logical_and(inside, Lnew > Lmin)
        nrejects += int((~acc).sum())
        u[acc], p[acc], L[acc] = unew[acc], pnew[acc], Lnew[acc]
        ever |= acc
        steps.append(dict(v=v, tleft=tl, tright=tr, t=t, unew=unew, Lnew=Lnew, inside=inside, accepted=acc.copy()))
    nfar, sumlog = 0.0, 0.0
    if maxradiussq is not None and acc.any():
        d2 = ((whiten(us[start[acc]]) - whiten(u[acc]))**2).sum(axis=1)
        nfar = float((d2 > maxradiussq).sum())
        sumlog = float(np.log(np.sqrt(d2) / np.sqrt(maxradiussq) + 1e-10).sum())
    return dict(u=u, p=p, L=L, start=start, ever=ever, last=acc, nrejects=nrejects, nlast=int(acc.sum()), nfar=nfar,
                sumlog=sumlog, nnever=int((~ever).sum()), next_offset=next_offset(offset, P, nsteps, d), steps=steps)
