"""High-precision restatement of the device proposal generator's four draws (csrc/mlf_sample.hip, csrc/mlf_region_sample.hip),
an error scale per element, a three-way verdict per draw and the matcher that compares the device's accepted rows with it in
draw order (shared by test_sampling_draws.py, test_philox.py and test_sampling_reference.py).  A plain module, not a conftest.

The draws start from the same Philox words as the device: `oracle.philox.blocks` and `u01` are exact (integers, and one
exactly representable binary64 value per pair of words) and stay the source.  Everything after the uniforms is restated here:

    method 1   z_j = sqrt(-2 log u) (cos, sin)(2 pi u') per pair;  w = center + z sqrt(enlarge) u''^(1/d) / |z| . axes_T
    method 2   t = low + (high - low) U,  low = bbox_lo - sqrt(r2), high = bbox_hi + sqrt(r2);  w = untransform(t)
    method 3   t = live[which] + z u''^(1/d) / |z| sqrt(r2), thinning uniform, live index;   w = untransform(t)
    untransform (AffineLayer)   w = t . invT + ctr, circular axes rotated back: fmod(v + 1 - shift, 1)

once, over an arithmetic that is either np.longdouble (64-bit mantissa where the platform has one; vectorised, all rows) or
mpmath at 50 digits (object arrays; a subsample of rows as a cross-check, or every row where no extended long double exists).
The availability rule is that of loglike_reference.py: where only one of the two exists, that one is the reference; neither
is a reason to skip.

Scale: the same formula with every term taken positive (|z_j s A_jk| summed, + |ctr_k|, ...), a direction component z_j / |z|
counted as min(rad_j / |z|, 1) (cos and sin as 1: a component near a zero of the cosine inherits the absolute rounding of its
pair).  Tolerance 1e-12 * scale, the class of loglike_reference.RTOL; the binary64 restatement of oracle/philox.py stays within
1e-13 * scale (test_sampling_reference.py, on the CPU).

Verdict: every test the device applies to a draw has a margin and a scale of its own, the first-order size of what a value
error of 1e-12 * scale can move the tested quantity by (plus the arithmetic of the quantity itself):

    cube        min(v_k, 1 - v_k) against scale_k
    ellipsoid   enlarge - q,  q = dl' P dl, against  2 sum_i s_i |P dl|_i + sum_ij |dl_i| |P_ij| |dl_j|,  s_i = scale_i + |c_i|
    neighbours  r2 - |t - l|^2 per live point l, against  2 |t - l| (|s_t| + |s_l|) + |t - l|^2   (Cauchy-Schwarz over the columns)
    thinning    1 - thin * multiplicity against 1 + thin * multiplicity, for every multiplicity the neighbour margins leave open

A draw is UNDECIDED if some test that could still change its fate has |margin| < 1e-9 * scale -- one thousand times the value
tolerance, so a kernel whose values pass cannot disagree on a decided draw -- and IN or OUT otherwise.
"""
import contextlib

import numpy as np

from oracle import philox

import loglike_reference as LR

LD = LR.LD
HAVE_LONGDOUBLE = LR.HAVE_LONGDOUBLE
HAVE_MPMATH = LR.HAVE_MPMATH
mpmath = LR.mpmath

RTOL = LR.RTOL          # value tolerance, relative to scale
BAND = 1e-9             # verdict band, relative to the test's scale: 1000 RTOL
OUT, IN, UNDECIDED = 0, 1, 2
_TINY = 1e-300


class DrawMismatch(AssertionError):
    pass


# ------------------------------------------------------------------------------------------------ the two arithmetics
class LongDouble(object):
    name = "longdouble"
    ctx = staticmethod(contextlib.nullcontext)
    log, sqrt, cos, sin, trunc = np.log, np.sqrt, np.cos, np.sin, np.trunc

    @staticmethod
    def conv(x):
        return np.asarray(x, dtype=np.float64).astype(LD)

    @staticmethod
    def num(x):
        return LD(float(x))

    @staticmethod
    def pi():
        return 4 * np.arctan(LD(1))

    @staticmethod
    def root(u, d):
        return np.power(u, LD(1) / LD(d))

    @staticmethod
    def f64(x):
        return np.asarray(x).astype(np.float64)


class MpMath(object):
    """object arrays of mpf; every call happens inside ctx() (50 digits)"""
    name = "mpmath"

    @staticmethod
    def ctx():
        return mpmath.workdps(50)

    @staticmethod
    def _each(fn):
        return np.frompyfunc(fn, 1, 1)

    @classmethod
    def conv(cls, x):
        x = np.asarray(x, dtype=np.float64)
        return cls._each(lambda v: mpmath.mpf(float(v)))(x) if x.size else x.astype(object)

    @staticmethod
    def num(x):
        return mpmath.mpf(float(x))

    @staticmethod
    def pi():
        return +mpmath.pi

    @classmethod
    def log(cls, x):
        return cls._each(mpmath.log)(x)

    @classmethod
    def sqrt(cls, x):
        return mpmath.sqrt(x) if isinstance(x, mpmath.mpf) else cls._each(mpmath.sqrt)(x)

    @classmethod
    def cos(cls, x):
        return cls._each(mpmath.cos)(x)

    @classmethod
    def sin(cls, x):
        return cls._each(mpmath.sin)(x)

    @classmethod
    def trunc(cls, x):
        return cls._each(lambda v: mpmath.mpf(int(v)))(x)

    @classmethod
    def root(cls, u, d):
        return cls._each(lambda v: mpmath.power(v, mpmath.mpf(1) / d))(u)

    @classmethod
    def f64(cls, x):
        return np.frompyfunc(float, 1, 1)(np.asarray(x, dtype=object)).astype(np.float64)


REFERENCE = LongDouble if HAVE_LONGDOUBLE else MpMath


# ------------------------------------------------------------------------------------------------ geometry
class Geometry(object):
    """What the device holds of a region: live points u, layer (ctr, T, invT, shift = 1 - cut per circular axis, NaN elsewhere,
    or None), ellipsoid (center, invcov, axes_T, enlarge), r2 = maxradiussq, the t-space bounding box of the live points,
    friends = whether the neighbour test belongs to the region (MLFriends) or not (RobustEllipsoidRegion)."""

    def __init__(self, u, ctr, T, invT, shift, center, invcov, axes_T, enlarge, r2, bbox_lo, bbox_hi, friends):
        f = lambda a: None if a is None else np.array(a, dtype=np.float64)
        self.u, self.ctr, self.T, self.invT, self.shift = f(u), f(ctr), f(T), f(invT), f(shift)
        self.center, self.invcov, self.axes_T = f(center), f(invcov), f(axes_T)
        self.enlarge, self.r2 = float(enlarge), float(r2)
        self.bbox_lo, self.bbox_hi = f(bbox_lo), f(bbox_hi)
        self.friends = bool(friends)
        self.d = self.u.shape[1]

    @classmethod
    def of_region(cls, region):
        layer = region.transformLayer
        d = region.u.shape[1]
        return cls(np.asarray(region.u), layer.ctr, layer.T, layer.invT, layer.wrap_shift_vector(d), region.ellipsoid_center,
                   region.ellipsoid_invcov, region.ellipsoid_axes_T, region.enlarge, region.maxradiussq, region.bbox_lo,
                   region.bbox_hi, region._uses_scan())


def affine_layer(u, wrapped_dims=()):
    """AffineLayer.optimize(u, u).  At d = 1 np.cov returns a scalar, which eigh does not take (the reference's driver uses a
    ScalingLayer there): the 1 x 1 layer is written out, formula by formula."""
    import ultranest_amd.mlfriends as m
    layer = m.AffineLayer(wrapped_dims=list(wrapped_dims))
    if u.shape[1] > 1:
        layer.optimize(u, u)
        return layer
    layer.optimize_wrap(u)
    layer.ctr = np.mean(layer.wrap(u), axis=0)
    layer.cov = np.atleast_2d(np.cov(u, rowvar=0)) * 3
    layer.logvolscale = np.linalg.slogdet(np.linalg.inv(layer.cov))[1] * -0.5
    layer.T = layer.cov ** -0.5
    layer.invT = np.linalg.inv(layer.T)
    layer.axes = layer.invT
    layer.set_clusterids(npoints=len(u))
    return layer


def fmod1(B, x):
    """C's fmod(x, 1): the sign of x, exact"""
    return x - B.trunc(x)


def live_tspace(B, g, rows=None):
    """(live_t, scale): the whitened live points (AffineLayer.transform: circular axes rotated by shift, - ctr, . T); all
    of them, or the given rows"""
    u = g.u if rows is None else g.u[rows]
    w, s = B.conv(u), np.abs(u)
    if g.shift is not None:
        wrapped = ~np.isnan(g.shift)
        sh = np.where(wrapped, g.shift, 0.0)
        w = np.where(wrapped, fmod1(B, w + B.conv(sh)), w)
        s = s + np.where(wrapped, 1.0 + np.abs(sh), 0.0)
    return np.dot(w - B.conv(g.ctr), B.conv(g.T)), np.dot(s + np.abs(g.ctr), np.abs(g.T))


def transform(B, g, w, w_scale):
    """(t, scale) of cube-space rows (no circular axes: the cases of methods 0 and 1 have none)"""
    assert g.shift is None
    return np.dot(w - B.conv(g.ctr), B.conv(g.T)), np.dot(w_scale + np.abs(g.ctr), np.abs(g.T))


def untransform(B, g, t, t_scale):
    """(w, scale): AffineLayer.untransform, w = t . invT + ctr, circular axes rotated back as fmod(v + 1 - shift, 1)"""
    w = np.dot(t, B.conv(g.invT)) + B.conv(g.ctr)
    s = np.dot(t_scale, np.abs(g.invT)) + np.abs(g.ctr)
    if g.shift is not None:
        wrapped = ~np.isnan(g.shift)
        sh = np.where(wrapped, g.shift, 0.0)
        w = np.where(wrapped, fmod1(B, w + (1 - B.conv(sh))), w)
        s = s + np.where(wrapped, 1.0 + np.abs(sh), 0.0)
    return w, s


# ------------------------------------------------------------------------------------------------ the draws
def _rows(n, rows):
    return np.arange(n, dtype=np.uint64) if rows is None else np.asarray(rows, dtype=np.uint64)


def _pair_uniforms(seed, stream, counters):
    w = philox.blocks(seed, stream, counters)
    return philox.u01(w[:, 0], w[:, 1]), philox.u01(w[:, 2], w[:, 3])


def _directions(B, seed, stream, base, d):
    """Box-Muller rows on the blocks base + 0 ... base + npairs - 1: (z (n, d), |z| (n,), bound (n, d) on |z_j| / |z|)"""
    npairs = (d + 1) // 2
    n = len(base)
    z = np.empty((n, 2 * npairs), dtype=object if B is MpMath else LD)
    rad = np.empty((n, 2 * npairs), dtype=object if B is MpMath else LD)
    two_pi = 2 * B.pi()
    for j in range(npairs):
        u0, u1 = _pair_uniforms(seed, stream, base + np.uint64(j))
        r = B.sqrt(-2 * B.log(B.conv(u0)))
        ang = two_pi * B.conv(u1)
        z[:, 2 * j], z[:, 2 * j + 1] = r * B.cos(ang), r * B.sin(ang)
        rad[:, 2 * j] = rad[:, 2 * j + 1] = r
    z, rad = z[:, :d], rad[:, :d]
    norm = B.sqrt((z * z).sum(axis=1))
    return z, norm, np.minimum(B.f64(rad / norm[:, None]), 1.0)


def ellipsoid_draws(g, seed, offset, n, rows=None, B=None):
    """method 1 -> (w (rows, d), scale (rows, d), next offset); Philox stream 1, npairs + 1 blocks per proposal"""
    B = B or REFERENCE
    d = g.d
    per = (d + 1) // 2 + 1
    base = np.uint64(offset) + _rows(n, rows) * np.uint64(per)
    with B.ctx():
        z, norm, direction = _directions(B, seed, 1, base, d)
        u, _ = _pair_uniforms(seed, 1, base + np.uint64(per - 1))
        radius = B.sqrt(B.num(g.enlarge)) * B.root(B.conv(u), d)
        ball = z * (radius / norm)[:, None]
        w = B.conv(g.center) + np.dot(ball, B.conv(g.axes_T))
        scale = np.dot(direction * B.f64(radius)[:, None], np.abs(g.axes_T)) + np.abs(g.center)
    return w, scale, int(offset) + n * per


def _cube_uniforms(seed, stream, offset, n, d, rows):
    """element e = row d + k of a flat batch: block offset + e // 2, its first or second pair of words"""
    e = _rows(n, rows)[:, None] * np.uint64(d) + np.arange(d, dtype=np.uint64)[None, :]
    first, second = _pair_uniforms(seed, stream, np.uint64(offset) + (e.ravel() >> np.uint64(1)))
    return np.where((e.ravel() & np.uint64(1)) == 0, first, second).reshape(e.shape), int(offset) + (n * d + 1) // 2


def tbox_draws(g, seed, offset, n, rows=None, B=None):
    """method 2 -> (t (rows, d), scale (rows, d), next offset); Philox stream 5, two elements per block"""
    B = B or REFERENCE
    U, nxt = _cube_uniforms(seed, 5, offset, n, g.d, rows)
    with B.ctx():
        pad = B.sqrt(B.num(g.r2))
        low, high = B.conv(g.bbox_lo) - pad, B.conv(g.bbox_hi) + pad
        t = low + (high - low) * B.conv(U)
        fpad = float(pad)
        scale = (np.abs(g.bbox_lo) + fpad) + (np.abs(g.bbox_hi) + np.abs(g.bbox_lo) + 2 * fpad) * U
    return t, scale, nxt


def around_draws(g, seed, offset, n, rows=None, B=None, live=None):
    """method 3 -> (t (rows, d), scale (rows, d), thinning uniform (rows,), live index (rows,), next offset); Philox stream 6,
    npairs + 2 blocks per proposal: live index and radial uniform, thinning uniform, the Box-Muller pairs"""
    B = B or REFERENCE
    d = g.d
    per = (d + 1) // 2 + 2
    base = np.uint64(offset) + _rows(n, rows) * np.uint64(per)
    w0 = philox.blocks(seed, 6, base)
    which = ((w0[:, 0].astype(np.uint64) * np.uint64(len(g.u))) >> np.uint64(32)).astype(np.int64)
    radial = philox.u01(w0[:, 2], w0[:, 3])
    thin, _ = _pair_uniforms(seed, 6, base + np.uint64(1))
    with B.ctx():
        if live is not None:
            centre, centre_scale = live[0][which], live[1][which]
        else:      # the chosen live points alone
            chosen, back = np.unique(which, return_inverse=True)
            centre, centre_scale = (a[back] for a in live_tspace(B, g, chosen))
        z, norm, direction = _directions(B, seed, 6, base + np.uint64(2), d)
        f = B.root(B.conv(radial), d) / norm * B.sqrt(B.num(g.r2))
        t = centre + z * f[:, None]
        scale = centre_scale + direction * B.f64(f * norm)[:, None]
    return t, scale, thin, which, int(offset) + n * per


# ------------------------------------------------------------------------------------------------ verdicts
def three_way(margin, scale):
    """IN where margin > BAND scale, OUT where margin < -BAND scale, UNDECIDED between (and for a NaN)"""
    margin, scale = np.asarray(margin, dtype=np.float64), np.asarray(scale, dtype=np.float64)
    out = np.full(margin.shape, UNDECIDED, dtype=np.int8)
    out[margin > BAND * scale] = IN
    out[margin < -BAND * scale] = OUT
    return out


def combine(*verdicts):
    """OUT if some test says OUT; else UNDECIDED if some test is undecided; else IN"""
    v = np.stack(verdicts)
    out = np.where((v == UNDECIDED).any(axis=0), UNDECIDED, IN).astype(np.int8)
    out[(v == OUT).any(axis=0)] = OUT
    return out


def cube_verdict(B, w, w_scale):
    with B.ctx():
        margin = B.f64(np.minimum(w, 1 - w))
    return combine(*three_way(margin, np.maximum(w_scale, _TINY)).T)


def ellipsoid_verdict(B, g, w, w_scale):
    with B.ctx():
        dl = w - B.conv(g.center)
        Pd = np.dot(dl, B.conv(g.invcov))
        q = (Pd * dl).sum(axis=1)
        margin = B.f64(B.num(g.enlarge) - q)
        adl = np.abs(B.f64(dl))
        scale = 2 * ((w_scale + np.abs(g.center)) * np.abs(B.f64(Pd))).sum(axis=1) + (np.dot(adl, np.abs(g.invcov)) * adl).sum(axis=1)
    return three_way(margin, scale)


def neighbour_counts(B, g, t, t_scale, live=None, chunk=4096):
    """(sure, maybe): live points certainly within r2 of each row of t, and those within r2 or in the band.  Pairs further
    than 1e-6 * scale from r2 are settled in binary64 (expanded squares through BLAS: 1e-13 * scale); the others are taken
    again in the reference arithmetic, coordinate by coordinate."""
    with B.ctx():
        live_t, live_scale = live if live is not None else live_tspace(B, g)
        l64, t64 = B.f64(live_t), B.f64(t)
        ls, ts = np.sqrt((live_scale ** 2).sum(axis=1)), np.sqrt((t_scale ** 2).sum(axis=1))
        l2 = (l64 * l64).sum(axis=1)
        sure = np.zeros(len(t64), dtype=np.int64)
        maybe = np.zeros(len(t64), dtype=np.int64)
        r2 = B.num(g.r2)
        for lo in range(0, len(t64), chunk):
            tc = t64[lo:lo + chunk]
            d2 = np.maximum((tc * tc).sum(axis=1)[:, None] + l2[None, :] - 2 * np.dot(tc, l64.T), 0.0)
            scale = 2 * np.sqrt(d2) * (ts[lo:lo + chunk, None] + ls[None, :]) + d2
            near = ~(np.abs(d2 - g.r2) > 1e-6 * scale)
            sure[lo:lo + chunk] = ((d2 < g.r2) & ~near).sum(axis=1)
            ii, jj = np.nonzero(near)
            if len(ii):
                diff = t[lo + ii] - live_t[jj]
                exact = (diff * diff).sum(axis=1)
                e64 = B.f64(exact)
                v = three_way(B.f64(r2 - exact), 2 * np.sqrt(e64) * (ts[lo + ii] + ls[jj]) + e64)
                np.add.at(sure, lo + ii[v == IN], 1)
                np.add.at(maybe, lo + ii[v == UNDECIDED], 1)
        maybe += sure
    return sure, maybe


def neighbour_verdict(sure, maybe):
    """some live point within r2 (methods 0, 1 and 2)"""
    return np.where(sure > 0, IN, np.where(maybe > 0, UNDECIDED, OUT)).astype(np.int8)


def thinning_verdict(B, thin, sure, maybe):
    """method 3: multiplicity > 0 and thin * multiplicity < 1, for every multiplicity in [sure, maybe]"""
    with B.ctx():
        th = B.conv(thin)
        side = []
        for m in (np.maximum(sure, 1), np.maximum(maybe, 1)):
            tm = th * B.conv(m.astype(np.float64))
            side.append(three_way(B.f64(1 - tm), B.f64(1 + tm)))
    out = np.where(side[0] == side[1], side[0], UNDECIDED).astype(np.int8)
    out[(sure == 0) & (maybe > 0)] = UNDECIDED
    out[maybe == 0] = OUT
    return out


class Reference(object):
    """The reference of one batch of `method` (1, 2 or 3): rows (n, d) in cube space as the device returns them, scale
    (n, d) binary64, verdict (n,), next_offset.  The caps are conditions on the inputs, asserted before any device output
    is looked at."""

    def __init__(self, g, method, n, seed, offset, B=None):
        B = B or REFERENCE
        self.n, self.method = n, method
        live = None
        if method == 3 or (g.friends and method in (1, 2)):
            with B.ctx():
                live = live_tspace(B, g)
        verdict = np.full(n, IN, dtype=np.int8)

        def apply(test, *rows):
            """one more test, taken of the draws that no earlier test has put OUT"""
            open_ = np.flatnonzero(verdict != OUT)
            verdict[open_] = combine(verdict[open_], test(*(a[open_] for a in rows)))

        if method == 1:
            w, ws, self.next_offset = ellipsoid_draws(g, seed, offset, n, B=B)
            apply(lambda w, ws: cube_verdict(B, w, ws), w, ws)
            apply(lambda w, ws: ellipsoid_verdict(B, g, w, ws), w, ws)
            if g.friends:
                def neighbours(w, ws):
                    with B.ctx():
                        t, ts = transform(B, g, w, ws)
                    return neighbour_verdict(*neighbour_counts(B, g, t, ts, live))
                apply(neighbours, w, ws)
        else:
            if method == 2:
                t, ts, self.next_offset = tbox_draws(g, seed, offset, n, B=B)
                apply(lambda t, ts: neighbour_verdict(*neighbour_counts(B, g, t, ts, live)), t, ts)
            else:
                t, ts, thin, self.which, self.next_offset = around_draws(g, seed, offset, n, B=B, live=live)
                apply(lambda t, ts, thin: thinning_verdict(B, thin, *neighbour_counts(B, g, t, ts, live)), t, ts, thin)
            # cube-space rows of the draws still open alone (the others are never compared): NaN elsewhere
            open_ = np.flatnonzero(verdict != OUT)
            w, ws = np.full(t.shape, np.nan, dtype=t.dtype), np.full(t.shape, np.nan)
            with B.ctx():
                w[open_], ws[open_] = untransform(B, g, t[open_], ts[open_])
            apply(lambda w, ws: cube_verdict(B, w, ws), w, ws)
            apply(lambda w, ws: ellipsoid_verdict(B, g, w, ws), w, ws)
        self.rows, self.scale, self.verdict = w, ws, verdict
        self.undecided = int((verdict == UNDECIDED).sum())
        self.decided_in = int((verdict == IN).sum())

    def assert_caps(self):
        assert self.undecided <= max(2, self.n // 10000), "%d undecided draws of %d" % (self.undecided, self.n)
        assert self.decided_in >= 200, "only %d decided-in draws of %d" % (self.decided_in, self.n)

    def match(self, got):
        return match_in_draw_order(got, self.rows, self.verdict, self.scale)


# ------------------------------------------------------------------------------------------------ the matcher
def match_in_draw_order(got, ref_rows, verdict, scale, rtol=RTOL):
    """The device returns its accepted rows in draw order, without indices.  Every row of `got` must equal the next reference
    row whose verdict is IN or UNDECIDED within rtol * scale; an undecided reference row may be skipped, a decided-in one may
    not, and no device row may be left over.  Returns (undecided draws of the batch, rows compared); raises DrawMismatch with
    the draw index, the column and both values."""
    got = np.asarray(got, dtype=np.float64)
    verdict = np.asarray(verdict)
    ref = np.asarray(ref_rows)
    if ref.dtype == object:       # mpmath rows: their binary64 rounding (1.1e-16 relative) is the reference here
        ref = MpMath.f64(ref)
    tol = rtol * np.asarray(scale, dtype=np.float64)
    undecided = int((verdict == UNDECIDED).sum())
    cand = np.flatnonzero(verdict != OUT)
    gl = got.astype(ref.dtype)

    def agrees(i, j):
        return (np.abs(gl[i] - ref[j]).astype(np.float64) <= tol[j])

    if len(got) == len(cand) and bool(agrees(slice(None), cand).all()):
        return undecided, len(got)
    c = 0
    for i in range(len(got)):
        while True:
            if c >= len(cand):
                raise DrawMismatch("device row %d = %r matches no remaining draw of the reference (%d draws could be accepted)"
                                   % (i, got[i], len(cand)))
            j = cand[c]
            c += 1
            ok = agrees(i, j)
            if ok.all():
                break
            if verdict[j] == UNDECIDED:
                continue
            k = int(np.flatnonzero(~ok)[0])
            raise DrawMismatch("draw %d (decided in), column %d: device row %d has %r, the reference %r (tolerance %.3g)"
                               % (j, k, i, got[i, k], float(ref[j, k]), tol[j, k]))
    dropped = [j for j in cand[c:] if verdict[j] == IN]
    if dropped:
        raise DrawMismatch("draw %d (decided in) is missing: the device returned %d rows, %d decided-in draws remain"
                           % (dropped[0], len(got), len(dropped)))
    return undecided, len(got)


def excess(got, ref_rows, scale, rtol=RTOL):
    """max |got - ref| / (rtol scale) over all elements of aligned arrays (<= 1 passes), in the reference's arithmetic"""
    ref = np.asarray(ref_rows)
    if ref.dtype == object:
        with MpMath.ctx():
            err = MpMath.f64(np.abs(MpMath.conv(got) - ref))
    else:
        err = np.abs(np.asarray(got, dtype=np.float64).astype(ref.dtype) - ref).astype(np.float64)
    ratio = err / (rtol * np.maximum(np.asarray(scale, dtype=np.float64), _TINY))
    ratio[np.isnan(ratio)] = np.inf
    return float(ratio.max()) if ratio.size else 0.0
