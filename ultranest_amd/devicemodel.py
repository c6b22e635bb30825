"""User-written likelihoods and prior transforms that run on the GPU.

The GPU counterpart of the reference's compiled-language likelihoods (reference languages/c/mylib.c: the
``(params, d, n, like)`` convention that ``ultranest_amd.likelihoods`` follows): the user writes two HIP
device functions, the package compiles them at run time for gfx950 (hiprtc) around one wrapper kernel
(``csrc/mlf_user_rows.hpp``) and hands back a pair of vectorized callbacks::

    model = DeviceModel(ndim, loglike_source, transform_source=None, aux=None, name=None, nterms=None, nsums=None,
                        nderived=None, derived_source=None, gate_derived=False, ncov=None)
    model.loglike(theta)    # (n, ndim) -> (n,)      vectorized callback, evaluated on the GPU
    model.transform(u)      # (n, ndim) -> (n, ndim)  vectorized callback (identity without a transform source)

(with ``nderived=Q`` the transform returns ``(n, ndim + Q)`` and the likelihood accepts either width: "Derived parameters" below)

The sources define::

    __device__ double mlf_user_loglike(const double *p, int d, const double *aux, long long naux);           // required
    __device__ void mlf_user_transform(const double *u, double *p, int d, const double *aux, long long naux);  // optional

(``ultranest_amd.priors`` writes the transform source from a list of priors -- ``PriorTransform([...]).model(loglike_source)``.)

``aux`` is the model's data array (float64, uploaded once).  The code runs on a shared GPU: it reads ``aux`` only
within ``naux``, writes nothing but the ``p`` row it is handed, and contains no inline assembly.  It is compiled with
``-O3 -std=c++17 -ffp-contract=off`` (the library's arithmetic contract: no FMA is formed, so a restated built-in
function can agree with the built-in kernels bit for bit).

The callbacks work everywhere a host callback works (``vectorized=True`` contract), and the device routes recognise
them by their ``device_spec`` marker (a ``UserModelSpec``, never one of the ``(kind, a, b)`` tuples):

* ``MLFriends.refill`` (and ``RobustEllipsoidRegion`` / ``SimpleRegion``): draw, region test, transform + likelihood in
  ONE fused launch (``mlf_region_refill_user``), threshold, compaction -- the rows outside the membership mask are not
  evaluated.  With the driver's parameter-space wrapping ellipsoid (``refill(..., tregion=...)``, reference
  integrator.py:1789-1804) the same launch tests ``tregion.inside(p)`` between transform and likelihood: the model's
  *gated* variant (``handle(with_transform, gated=True)``: the wrapper compiled with ``-DMLF_USER_TREGION=1``, its own
  code object, compiled on first gated use) calls the likelihood only for the rows that pass, and the batch never
  leaves the device;
* ``PopulationSliceSampler``: host-RNG mode through ``mlf_walkers_finish_user``, Philox mode through
  ``mlf_walkers_step_user``; only the acceptable proposals are evaluated.

The device route is taken when ``loglike`` is a model's ``loglike`` and ``transform`` is the same model's
``transform`` or ``likelihoods.identity_transform``; every other combination keeps the host-callback route.

Not covered (a user model then runs on the per-step route, which returns the same records):

* graph replay of the sampler step (``PopulationSliceSampler.use_graph``): ``step_user`` runs without capture;
* the single-launch multi-round kernel (``max_rounds > 1``): ``k_walk_rounds`` inlines the built-in likelihoods, and
  compiling it per model is a later step.

Derived parameters (``nderived=Q``)
-----------------------------------
Output columns computed from the parameters -- a flux from an amplitude and a width, a mass ratio, a radius: the reference
driver's ``derived_param_names``, ``num_params = x_dim + Q``.  With ``nderived=Q`` (a Python int, ``Q >= 1`` and
``ndim + Q <= MLF_MAX_DIM``; ``nderived`` and ``derived_source`` are given together) the derived source defines::

    __device__ void mlf_user_derived(const double *p, int d, double *q, int nq, const double *aux, long long naux);

It writes all of ``q[0..nq)`` from the row's ``p`` -- the ``d`` transformed parameters, or the cube coordinates of a model
without a transform -- and is a pure function of its arguments, compiled under the contract of everything else (``-O3
-std=c++17 -ffp-contract=off``, no inline assembly, reads of ``aux`` within ``naux``).  Then:

* ``model.nparams == ndim + Q`` (``ndim`` without ``nderived``) and ``model.nderived`` is ``Q`` (or None);
* ``model.transform(u)`` returns ``(n, ndim + Q)``: columns ``[0, ndim)`` are what the model without ``nderived`` returns, bit
  for bit, columns ``[ndim, ndim + Q)`` are ``q``;
* ``model.loglike(theta)`` accepts ``(n, ndim + Q)`` or ``(n, ndim)`` and reads the first ``ndim`` columns only.  THE LIKELIHOOD
  DOES NOT SEE THE DERIVED COLUMNS (a stated restriction): a likelihood that needs such a quantity computes it itself;
* ``model.derive(p)`` turns host rows ``(n, ndim)`` into ``(n, ndim + Q)``; ``model.derive_dev(d_p, n, d_out, stream=0)`` does
  the same on device pointers, as ``eval_dev`` does (the two arrays must not overlap).

Inside every device route a p row stays ``ndim`` wide: transform, t-region gate, likelihood, compaction and walker state are
those of the model without ``nderived``, and its main programs are compiled from exactly that model's source string (the same
cache keys and code objects: one compile serves both).  The derived columns come from ONE more program, compiled from
``source + "\n" + derived_source`` with ``-DMLF_USER_DERIVED=1`` under its own cache key (the model's helper functions are
visible to it), whose only kernel ``mlf_user_derive_rows`` (``csrc/mlf_user_rows.hpp``) runs on the rows a route hands out,
after the route has finished with them -- in the reference's routes the derived columns are consumed only when a point is
handed to the driver, so the rows are the same: the kept rows of a region refill (on the device, inside
``mlf_region_refill_user_derived``), the prepared samples of ``PopulationRandomWalkSampler`` / ``PopulationSimpleSliceSampler``
once per refill, the harvested point of ``PopulationSliceSampler``.  It combines with ``nterms`` / ``nsums`` without more programs.
With ``identity_transform`` paired to the model's likelihood the host route yields no derived columns, so the device route
yields none either (``device_route`` returns ``(model, False)`` and ``p`` is ``ndim`` wide).

A t-region together with derived parameters (``gate_derived=True``).  The reference builds the driver's parameter-space
wrapping ellipsoid over all ``num_params`` columns whenever the prior transform is not affine, so its gate needs ``q`` BEFORE the
likelihood.  By default ``refill(..., tregion=)`` returns None for a model with ``nderived`` and the batch takes the host sequence
through the callbacks above, which is correct and slow.  With ``gate_derived=True`` (it needs ``nderived``) the model has one
more program, compiled on first gated use from ``source + "\n" + derived_source`` with ``-DMLF_USER_TREGION=1
-DMLF_USER_GATE_DERIVED=1`` under its own cache key (``handle(with_transform, gated=True, derived=True)``): per member row
transform, ``mlf_user_derived``, the gate over ``[p | q]``, and the likelihood on the ``ndim``-wide row if the gate passes, in
one launch (``mlf_region_refill_user_derived_gated``); the rows stay ``ndim`` wide and the derive program extends the kept rows as
without a t-region.  The flag is an opt-in because it is a statement about COST: ``mlf_user_derived`` then runs on every member
row of a gated batch, not only on the kept rows.  It applies where ``tregion_on_device(tregion, ndim + Q)`` holds and the model is
paired with its own transform; without the flag every object, cache key, program and route is what it was.

Not covered: likelihoods that read derived columns.

Likelihoods summed over data terms (``nterms=K``)
-------------------------------------------------
The default form gives every row one thread: a likelihood that loops over ``aux`` (chi-square over spectral bins, a
Gaussian over observations) walks its data serially in that thread, all 64 lanes of a wave reading the same ``aux[k]``.
The routes above evaluate populations of 10^2 to 10^4 rows, which is a few dozen waves on a device with 1024 SIMDs.  With
``nterms=K`` (a Python int, K >= 1) the likelihood source defines, INSTEAD of ``mlf_user_loglike``::

    __device__ double mlf_user_loglike_term(const double *p, int d, const double *aux, long long naux, long long k);

and ``L(p) = sum over k in [0, K) of term(k)``.  One wave then owns one row, its 64 lanes split the terms and read ``aux``
side by side (index ``aux`` by ``k``).  Transform source, ``aux``, the callbacks, ``eval_dev`` and ``device_route`` are
unchanged, and every route recognises a summed model exactly as it does a default one; its four programs (with or without
transform, gated or not) are compiled with ``-DMLF_USER_SUM=1`` under their own cache keys ("Forms" below).  The prior transform
of a summed model runs on one lane of the row's wave.

The order of the sum is part of the interface (``csrc/mlf_user_rows.hpp``; ``-ffp-contract=off`` as above):

* per lane: lane ``l`` (0..63) starts from ``s_l = 0.0`` and adds ``term(k)`` for ``k = l, l+64, l+128, ... < K`` in
  ascending order, one plain addition each;
* across lanes: six exchange steps with lane distances 32, 16, 8, 4, 2, 1, in that order, each setting every lane to
  ``s_l + s_(l xor m)``;
* result: IEEE addition commutes, so all lanes hold the same bits after the six steps, and ``L`` is that value.

In numpy (sequential additions; ``np.sum`` is pairwise and is NOT this order)::

    s = np.zeros(64)
    for k in range(K): s[k % 64] += t[k]
    for m in (32, 16, 8, 4, 2, 1): s = s + s[np.arange(64) ^ m]
    L = s[0]

So ``L`` does not depend on the row's position in the batch, the batch size, the membership mask or the route; a NaN term
gives NaN; ``-inf`` terms give ``-inf``.  Per-row constants can live in term 0; a likelihood that is a FUNCTION of one or more
sums uses the next form.

Several sums and a final function (``nterms=K, nsums=M``)
---------------------------------------------------------
A profiled or marginalised amplitude (``L`` a function of ``sum y^2/sigma^2``, ``sum y f/sigma^2``, ``sum f^2/sigma^2``), a
marginalised noise level (``-(K/2) log sum r^2``), a Poisson fit with a free normalisation: a handful of sums over the data,
then a few scalar operations.  With ``nsums=M`` (a Python int, 1 <= M <= 8; it requires ``nterms``) the likelihood source
defines, INSTEAD of ``mlf_user_loglike_term``::

    __device__ void   mlf_user_loglike_terms(const double *p, int d, const double *aux, long long naux, long long k, double *t);
    __device__ double mlf_user_loglike_finish(const double *s, int nsums, const double *p, int d, const double *aux, long long naux);

``terms`` writes all M entries ``t[0..M)`` for data index ``k`` (the kernel does not pre-set ``t``: an entry the function
leaves unwritten is undefined); ``finish`` receives the M sums, the row's ``p`` and the data and returns ``L``.  ``nsums=1`` is
a function of one sum.  Per-row constants go into term 0 or into ``finish``.  M is a constant of the program (the accumulators
live in registers); the programs are compiled with ``-DMLF_USER_SUM=1 -DMLF_USER_NSUMS=M`` under their own cache keys ("Forms"
below); everything else -- transform, ``aux``, callbacks, ``eval_dev``, ``device_route``, every route -- is that of a summed model.

The order contract extends the one above and is part of the interface:

* each accumulator ``j`` follows, independently, exactly the order of the single-sum form: lane ``l`` starts from
  ``s_j = 0.0`` and adds ``t_j(k)`` for ``k = l, l+64, ... < K`` in ascending order, one plain addition each; then the six
  exchange steps with lane distances 32, 16, 8, 4, 2, 1, each setting every lane's ``s_j`` to ``s_j + s_j(l xor m)``;
* a lane with no term (``K < 64``) never calls ``terms``; its accumulators stay 0.0;
* after the exchange all lanes hold the same M values; ``finish`` is called by every lane with those values (it must be a
  pure function of its arguments), and lane 0's result is ``L``;
* a row outside the membership mask, or one that fails the t-region gate, calls neither function and gets ``L = -inf``.

In numpy::

    s = np.zeros((M, 64))
    for k in range(K): s[:, k % 64] += t[:, k]
    for m in (32, 16, 8, 4, 2, 1): s = s + s[:, np.arange(64) ^ m]
    L = finish(s[:, 0])

A NaN term of accumulator ``j`` reaches ``finish`` as NaN in ``s[j]`` only.  ``usermodels.amplitude_sum`` (M = 3, a profiled
amplitude) and ``usermodels.staircase3_sum`` are examples, each with a default-form twin.  Measured at d = 10
(``scripts/multisum_model_bench.py``, ``profiles/multisum_model_bench.json``): ``amplitude_sum`` takes 0.98 to 1.03 times the
time of the single-sum ``linear_sum`` on the same data at every shape (two more accumulators and the finish do not show), and
is 29 (1024 terms) and 49 (16384 terms) times faster than its twin at 1024 rows, 4.2 and 2.5 times at 16384 rows; no crossover
up to 16384 rows per call, the largest count measured -- "which form" above applies unchanged.

Which form.  Measured with ``usermodels.linear_sum`` against its twin at d = 10 (``scripts/summed_model_bench.py``,
``profiles/summed_model_bench.json``): at 1024 rows the summed form is 29.5 times faster with 1024 terms and 35.5 times with
16384 terms, at 16384 rows still 3.9 and 1.9 times; the crossover lies between 16384 and 65536 rows per call, and at 2^17
rows the default form is about 4 times faster (every row's wave then reads all of ``aux`` through the caches, which the
default form reads once per 64 rows).  So: the summed form for what the population routes send -- ``PopulationSliceSampler``,
the whole-refill samplers, region refills of a few thousand draws, up to about 10^4 rows per call -- and for many terms; the
default form for batches of 10^5 rows and more, or for a likelihood of a handful of terms.

Gaussian likelihoods with a dense covariance (``ncov=n``)
---------------------------------------------------------
A Gaussian process over a light curve or a radial-velocity series, correlated noise, a red-noise kernel plus jitter: a Gaussian
whose covariance depends on the parameters,

    L(p) = -1/2 r(p)^T K(p)^-1 r(p) - 1/2 ln det K(p) - (n/2) ln 2 pi.

A row needs an n x n Cholesky factorisation, which one thread cannot hold and the summed forms cannot express (the terms are
coupled).  With ``ncov=n`` (a Python int >= 1, at most ``max_ncov(ndim, has_transform)``) the likelihood source defines, INSTEAD
of ``mlf_user_loglike``::

    __device__ double mlf_user_cov(const double *p, int d, const double *aux, long long naux, int i, int j);   // 0 <= j <= i < n
    __device__ double mlf_user_resid(const double *p, int d, const double *aux, long long naux, int i);        // 0 <= i < n

Both are pure functions of their arguments under the contract of every user function; only the lower triangle is asked for.  One
workgroup of 256 threads then owns one row and factorises its matrix in LDS (``csrc/mlf_user_cov.hpp``).  Transform source,
``aux``, the callbacks, ``eval_dev``, ``device_route``, ``nderived`` / ``derived_source`` and ``priors.PriorTransform(...).model(src,
ncov=n)`` are unchanged and every route recognises the model as it does any other; its four programs (with or without transform,
gated or not) are compiled with ``-DMLF_USER_NCOV=n`` around that header under their own cache keys (tag ``" cov=n"``).  ``ncov``
combines with neither ``nterms`` / ``nsums`` nor ``gate_derived`` (``ValueError``; with derived columns and a t-region the batch takes
the host sequence, as for any model without the flag), and the ``hotstart`` device forms refuse such an inner model.

``model.cov_factor(theta, with_transform=False)`` returns ``(Lfac (m, n, n), z (m, n), L (m,))`` of host rows -- the Cholesky
factor, ``z = Lfac^-1 r`` and the likelihood -- which is what GP prediction needs.

The arithmetic contract (part of the interface; it does not depend on how the threads share the work):

* augmented triangle: ``A`` is the packed lower triangle of an ``(n+1) x (n+1)`` matrix, ``A_ij = cov(i, j)`` for ``j <= i < n``,
  ``A_nj = resid(j)``, ``A_nn`` unused;
* factor: for ``k = 0 .. n-1`` in order the pivot is ``A_kk`` after its updates, ``L_kk = sqrt(A_kk)``, ``L_ik = A_ik / L_kk`` for
  ``k < i <= n``, and every remaining ``A_ij`` (``k < j <= i``, ``j < n``) becomes ``A_ij - L_ik * L_jk``: one multiplication and one
  subtraction, each rounded, no fused multiply-add.  Every element receives its subtractions in ascending ``k``, so its value is
  independent of the schedule.  Row ``n`` of the factor is ``z``;
* sums: ``quad = sum_k z_k * z_k`` and ``h = sum_k log(L_kk)``, both sequential from 0.0 in ascending ``k`` (the logarithms may be
  taken in parallel; the additions are one lane's);
* likelihood: ``L = ((-0.5 * quad) - h) - (double)n * 0.91893853320467274178``;
* failure: the first pivot in ascending ``k`` that is not ``> 0`` decides -- a NaN pivot gives ``L = NaN``, any other ``L = -inf``;
  nothing after it is computed and ``cov_factor`` returns that row's factor as NaN;
* skipped rows: a row outside the membership mask, or one that fails the t-region gate, calls neither function and gets
  ``L = -inf``; its ``p`` row is treated as in the summed form;
* independence: ``L`` does not depend on the row's position, the batch size, the mask or the route.

``tests/cov_reference.py`` restates the contract in numpy; the device's factor equals it bit for bit (square root, division,
product and difference are IEEE operations on both sides).

The cap.  The packed triangle, a copy of the current column and a flag word are static LDS (``cov_lds_bytes(n)``, the library's
``mlf_covmodel_lds_bytes``); the row's u and p are dynamic LDS as in the summed form; together at most the 163,840 bytes a
workgroup may declare on this device.  ``max_ncov(ndim, has_transform)`` is 199 at small ``ndim`` with this layout.  Larger
matrices need the factor in HBM with LDS panels: a later step.  Structured covariances (banded, Toeplitz, low rank plus diagonal)
want kernels of their own.

Which form.  A likelihood of independent terms is a summed model; this form is for coupled data.  Measured with
``usermodels.gp_sqexp`` against the same model as a vectorised numpy host callback (batched ``np.linalg.cholesky``, 16 threads;
``scripts/cov_model_bench.py``, ``profiles/cov_model_bench.json``): at 1024 rows 145 (n = 32), 321 (64), 329 (128: 0.83 against
272 ms) and 158 (199) times faster, at 16384 rows 228, 491, 347 and 166 times; a ``PopulationSimpleSliceSampler`` device refill
(popsize 1024, 10 steps, n = 64) takes 5.3 ms against 1594 ms through the host callback.

Forms
-----
Which program a handle runs is one ``Form(has_transform, gated, summed, nsums, derived, ncov)``: it checks the combination, gives the
library's variant number (``Form.variant``; the table in ``include/mlfriends_hip.h`` names each variant's kernel and the entries
that compile and load it; a covariance form is no numbered variant and has its own two entries) and the option tags of the cache key.  ``_cache_key(source, form)`` is the only key, ``compile_form``
the only caller of the library's compile entries, ``_Handle`` the only handle class, and a model keeps its handles by ``Form``.

Compiling needs no GPU; code objects are cached per process, keyed by a hash of the source, the options and the
wrapper header.  Evaluating without a GPU raises ``HipLibraryError`` like every other compute call (no CPU fallback).
"""
import collections
import ctypes
import hashlib
import os

import numpy as np

from . import _lib
from ._lib import check, f64, ptr

INCLUDE_DIR = os.path.join(os.path.dirname(os.path.abspath(__file__)), "csrc")
HEADER = os.path.join(INCLUDE_DIR, "mlf_user_rows.hpp")
COV_HEADER = os.path.join(INCLUDE_DIR, "mlf_user_cov.hpp")          # what a covariance program includes instead of HEADER
GATE_HEADER = os.path.join(INCLUDE_DIR, "mlf_tregion_dev.hpp")      # included by the gated variant only
VARIANT_DEFAULT, VARIANT_TREGION, VARIANT_SUM, VARIANT_SUM_TREGION = 0, 1, 2, 3     # MLF_USERMODEL_* of include/mlfriends_hip.h
VARIANT_SUMS, VARIANT_SUMS_TREGION = 4, 5
VARIANT_DERIVED = 6
VARIANT_TREGION_DERIVED, VARIANT_SUM_TREGION_DERIVED, VARIANT_SUMS_TREGION_DERIVED = 7, 8, 9
# the covariance form is no numbered variant of the library (its entries take `gated` as a flag): Form.variant of such a form
VARIANT_COV, VARIANT_COV_TREGION = 16, 17
COV_LDS_CAP = 163840                                                                # bytes of LDS a workgroup may declare (gfx950)
MAX_SUMS = 8                                                                        # MLF_USERMODEL_MAX_SUMS
MAX_DIM = 1024                                                                      # MLF_MAX_DIM
# what mlf_usermodel_compile passes to hiprtc besides -I, -DMLF_USER_HAS_TRANSFORM, -DMLF_USER_TREGION, -DMLF_USER_SUM and (with
# nsums) -DMLF_USER_NSUMS (part of the cache key)
COMPILE_OPTIONS = ("--offload-arch=gfx950", "-O3", "-std=c++17", "-ffp-contract=off")
MLF_E_COMPILE = 5

_code_cache = {}
compile_calls = 0      # hiprtc compiles made by this process (the cache avoids repeats)


class DeviceModelCompileError(RuntimeError):
    """hiprtc rejected the model's source (or hiprtc is not available); ``log`` holds its diagnostics."""

    def __init__(self, log):
        self.log = log
        RuntimeError.__init__(self, "the device model did not compile:\n" + log)


def _check_count(name, value, what, most=None):
    """A count as an int (None stays None); ValueError naming the argument otherwise.  No library call."""
    if value is None:
        return None
    if isinstance(value, bool) or not isinstance(value, (int, np.integer)):
        raise ValueError("%s must be an integer (the number of %s), got %r" % (name, what, value))
    if most is not None and not 1 <= value <= most:
        raise ValueError("%s must be 1 to %d, got %d" % (name, most, value))
    if value < 1:
        raise ValueError("%s must be at least 1, got %d" % (name, value))
    return int(value)


def _check_nderived(ndim, nderived, derived_source):
    """nderived as an int (None stays None); ValueError naming the argument otherwise.  No library call."""
    if nderived is None:
        if derived_source is not None:
            raise ValueError("derived_source needs nderived (the number of derived parameters it writes)")
        return None
    nderived = _check_count("nderived", nderived, "derived parameters")
    if ndim + nderived > MAX_DIM:
        raise ValueError("ndim + nderived must be at most %d (MLF_MAX_DIM), got %d + %d" % (MAX_DIM, ndim, nderived))
    if derived_source is None:
        raise ValueError("nderived needs derived_source (the source that defines mlf_user_derived)")
    return nderived


def cov_lds_bytes(ncov):
    """Static LDS of a covariance program in bytes: ``mlf_user_rows_cov_lds_bytes`` of ``csrc/mlf_user_cov.hpp`` restated (the
    packed augmented triangle, the column vector and the flag word, rounded up to 16), so that the constructor can refuse an
    ``ncov`` before any library call; the library exports the original as ``mlf_covmodel_lds_bytes``."""
    doubles = (ncov + 1) * (ncov + 2) // 2 + (ncov + 1) + 1
    return (doubles + 1) // 2 * 16


def max_ncov(ndim, has_transform):
    """The largest ``ncov`` a model of `ndim` parameters can have: static LDS plus the launch's dynamic rows (u, and p where a
    transform writes one) within the 163,840 bytes a workgroup may declare.  199 at small ndim with the layout of
    ``csrc/mlf_user_cov.hpp``; 0 where even ``ncov = 1`` does not fit."""
    rows = (2 if has_transform else 1) * int(ndim) * 8
    n = 0
    while cov_lds_bytes(n + 1) + rows <= COV_LDS_CAP:
        n += 1
    return n


class Form(collections.namedtuple("Form", "has_transform gated summed nsums derived ncov")):
    """Which program of a model: with its transform or the identity; gated by a t-region; the summed form, with nsums=M several
    sums; derived="derive" the derive program (none of the others apply), derived="gate" the gate over derived parameters (a gated
    program); ncov=n the covariance form (neither summed nor a gate over derived parameters).  The one place that maps these to a
    MLF_USERMODEL_* number and to the option tags of a cache key.  ValueError for a combination that is no program."""
    __slots__ = ()

    def __new__(cls, has_transform, gated=False, summed=False, nsums=None, derived=None, ncov=None):
        nsums = _check_count("nsums", nsums, "sums of the summed form", MAX_SUMS)
        if nsums is not None and not summed:
            raise ValueError("nsums needs the summed form: give nterms (the number of data terms) as well")
        if derived == "gate" and not gated:
            raise ValueError("derived=True names the gate over the derived parameters: it needs gated=True")
        if derived not in (None, "gate") and (derived != "derive" or has_transform or gated or summed):
            raise ValueError("derived is None, 'gate' or 'derive' (the derive program: no transform, gate or sum), got %r" % (derived,))
        ncov = _check_count("ncov", ncov, "rows of the covariance matrix")
        if ncov is not None and (summed or derived is not None):
            raise ValueError("ncov (the covariance form) combines with neither nterms / nsums (the summed forms) nor a derived "
                             "kind of program (gate_derived; the derive program is the model's own)")
        return super(Form, cls).__new__(cls, bool(has_transform), bool(gated), bool(summed), nsums, derived, ncov)

    @property
    def variant(self):
        if self.ncov is not None:
            return VARIANT_COV_TREGION if self.gated else VARIANT_COV
        if self.derived == "derive":
            return VARIANT_DERIVED
        kind = 2 if self.nsums is not None else 1 if self.summed else 0      # default, one sum, several sums
        if self.derived == "gate":
            return (VARIANT_TREGION_DERIVED, VARIANT_SUM_TREGION_DERIVED, VARIANT_SUMS_TREGION_DERIVED)[kind]
        return (VARIANT_DEFAULT, VARIANT_SUM, VARIANT_SUMS)[kind] + (VARIANT_TREGION if self.gated else 0)

    @property
    def tags(self):
        """what the options part of a cache key says behind ``repr((COMPILE_OPTIONS, has_transform))``"""
        return ((" tregion" if self.gated else "") + (" gate_derived" if self.derived == "gate" else "") +
                (" sum" if self.summed else "") + ("" if self.nsums is None else " sums=%d" % self.nsums) +
                (" derived" if self.derived == "derive" else "") + ("" if self.ncov is None else " cov=%d" % self.ncov))

    @property
    def headers(self):
        """the headers the form's program includes, in the order a cache key hashes them"""
        return (HEADER if self.ncov is None else COV_HEADER,) + ((GATE_HEADER,) if self.gated else ())


DERIVE = Form(False, derived="derive")


def _cache_key(source, form, *flags, **more):
    """sha256 over the source, the options and the headers the program includes (``Form.headers``).  `form`: a
    Form, or the arguments of one (``has_transform, gated, summed, nsums``)"""
    if not isinstance(form, Form):
        form = Form(form, *flags, **more)
    h = hashlib.sha256()
    header = b""
    for path in form.headers:
        with open(path, "rb") as fh:
            header += fh.read()
    options = repr((COMPILE_OPTIONS, form.has_transform)) + form.tags
    for part in (source.encode(), b"\0", options.encode(), b"\0", header):
        h.update(part)
    return h.hexdigest()


def compile_form(source, form):
    """The gfx950 code object (bytes) of `source` + the wrapper kernel as `form`, from the cache or from the library's compile
    entry for ``form.variant`` (once more with the reported size where the buffer was too small); cached per process."""
    global compile_calls
    key = _cache_key(source, form)
    code = _code_cache.get(key)
    if code is not None:
        return code
    L = _lib.lib()
    v = form.variant
    size = ctypes.c_size_t(0)
    log = ctypes.create_string_buffer(1 << 16)
    cap = 1 << 20
    for _ in range(2):
        buf = ctypes.create_string_buffer(cap)
        head = (source.encode(), INCLUDE_DIR.encode(), int(form.has_transform), v)
        tail = (buf, cap, ctypes.byref(size), log, len(log))
        compile_calls += 1
        if form.ncov is not None:
            rc = L.mlf_covmodel_compile(*(head[:3] + (int(form.gated), form.ncov) + tail))
        elif form.derived == "gate":
            rc = L.mlf_usermodel_compile_gate_derived(*(head + (form.nsums or 0,) + tail))
        elif form.nsums is not None:
            rc = L.mlf_usermodel_compile_sums(*(head + (form.nsums,) + tail))
        else:
            rc = L.mlf_usermodel_compile_variant(*(head + tail))
        if rc == MLF_E_COMPILE:
            raise DeviceModelCompileError(log.value.decode(errors="replace"))
        if rc != 0 and size.value > cap:      # code object larger than the buffer: once more with its size
            cap = size.value
            continue
        check(rc)
        break
    code = buf.raw[:size.value]
    _code_cache[key] = code
    return code


def compile_model(source, has_transform, gated=False, summed=False, nsums=None):
    """The gfx950 code object (bytes) of `source` + the wrapper kernel; cached per process.  gated: the variant with the
    t-region test between transform and likelihood (module docstring), another program under its own key.  summed: the
    one-wave-per-row form around ``mlf_user_loglike_term`` (module docstring), two more programs under their own keys.
    nsums=M (with summed): M sums and a final function (``mlf_user_loglike_terms`` / ``_finish``), two more programs per M."""
    return compile_form(source, Form(has_transform, gated, summed, nsums))


def compile_derived(source):
    """The gfx950 code object of the derive program of `source` (a model's source followed by its derived source): the
    wrapper compiled with ``-DMLF_USER_DERIVED=1``, ``mlf_user_derive_rows`` its only kernel; cached per process."""
    return compile_form(source, DERIVE)


def compile_gate_derived(source, has_transform, summed=False, nsums=None):
    """The gfx950 code object of the gate-derived program of `source` (a model's source followed by its derived source): the
    gated wrapper compiled with ``-DMLF_USER_GATE_DERIVED=1`` as well, whose only kernel computes the derived columns of every
    member row and gates over ``[p | q]`` (module docstring); cached per process under its own key."""
    return compile_form(source, Form(has_transform, True, summed, nsums, "gate"))


class UserModelSpec(object):
    """``device_spec`` marker of a DeviceModel's callbacks: names the model and which callback carries it."""
    __slots__ = ("model", "role")

    def __init__(self, model, role):
        self.model, self.role = model, role

    def __repr__(self):
        return "UserModelSpec(%s, %s)" % (self.model.name, self.role)


class _Callback(object):
    def __init__(self, model, role):
        self.device_spec = UserModelSpec(model, role)
        self.__name__ = "%s.%s" % (model.name, role)

    def __call__(self, x):
        m = self.device_spec.model
        return m._loglike(x) if self.device_spec.role == "loglike" else m._transform(x)


class _Handle(object):
    """One loaded program (``mlf_usermodel``) on the library's device, created through the entry that owns its form's variant.
    nterms: the summed form; derived, nderived: one of the two derived kinds (``Form``)."""

    def __init__(self, code, ndim, has_transform, aux, gated=False, nterms=None, nsums=None, derived=None, nderived=None,
                 ncov=None):
        form = Form(has_transform, gated, nterms is not None, nsums, derived, ncov)
        L, h = _lib.lib(), ctypes.c_void_p()
        head = (code, len(code), int(ndim))
        tail = (ptr(aux), len(aux), ctypes.byref(h))
        if form.ncov is not None:
            rc = L.mlf_covmodel_create(*(head + (int(form.has_transform), int(form.gated), form.ncov) + tail))
        elif form == DERIVE:
            rc = L.mlf_usermodel_create_derived(*(head + (int(nderived),) + tail))
        else:
            head += (int(form.has_transform), form.variant)
            if form.derived == "gate":
                rc = L.mlf_usermodel_create_gate_derived(*(head + (int(nterms or 0), int(nderived)) + tail))
            elif form.summed:
                rc = L.mlf_usermodel_create_sum(*(head + (int(nterms),) + tail))
            else:
                rc = L.mlf_usermodel_create_variant(*(head + tail))
        check(rc)
        self._h = h
        self.has_transform = form.has_transform

    @property
    def handle(self):
        return self._h

    def close(self):
        h, self._h = getattr(self, "_h", None), None
        if h:
            check(_lib.lib().mlf_usermodel_destroy(h))

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class DeviceModel(object):
    """A likelihood (and optional prior transform) written as HIP device functions (module docstring).  nterms=K: the
    summed form, whose likelihood source defines ``mlf_user_loglike_term`` and whose L is the sum of its K terms in the
    documented order.  nterms=K, nsums=M (1 <= M <= 8): the source defines ``mlf_user_loglike_terms`` (M terms per data
    index) and ``mlf_user_loglike_finish`` (L from the M sums) instead; each sum follows that order.  nderived=Q with
    derived_source (``mlf_user_derived``): Q derived columns behind the parameters, ``nparams == ndim + Q``; every route keeps
    its ndim-wide rows and the derive program extends the rows that are handed out.  gate_derived=True (with nderived): a region
    refill with a t-region over all ``ndim + Q`` columns runs on the device, at the cost of ``mlf_user_derived`` on every member
    row of such a batch (module docstring); without it such a refill returns None and the batch takes the host sequence.
    ncov=n: a Gaussian likelihood with a dense n x n covariance; the source defines ``mlf_user_cov`` and ``mlf_user_resid`` instead
    and one workgroup per row factorises the matrix in LDS under the documented arithmetic contract (``cov_factor``)."""

    _count = 0

    def __init__(self, ndim, loglike_source, transform_source=None, aux=None, name=None, nterms=None, nsums=None,
                 nderived=None, derived_source=None, gate_derived=False, ncov=None):
        self.ndim = int(ndim)
        if self.ndim <= 0:
            raise ValueError("ndim must be positive")
        self.nderived = _check_nderived(self.ndim, nderived, derived_source)
        if gate_derived and self.nderived is None:
            raise ValueError("gate_derived needs nderived and derived_source: it gates the t-region over the derived parameters")
        self.gate_derived = bool(gate_derived)
        self.nparams = self.ndim + (self.nderived or 0)
        self.nterms = _check_count("nterms", nterms, "terms of the summed form")
        self.nsums = Form(False, summed=self.summed, nsums=nsums).nsums
        self.has_transform = transform_source is not None
        self.ncov = _check_count("ncov", ncov, "rows of the covariance matrix")
        if self.ncov is not None:
            if self.summed:
                raise ValueError("ncov (the covariance form) does not combine with nterms / nsums (the summed forms)")
            if self.gate_derived:
                raise ValueError("gate_derived has no covariance form (ncov): without the flag a refill with a t-region over "
                                 "derived columns takes the host sequence")
            most = max_ncov(self.ndim, self.has_transform)
            if self.ncov > most:
                raise ValueError("ncov = %d: the factor must fit the LDS of one CU, at most ncov = %d for ndim = %d %s a transform "
                                 "(max_ncov)" % (self.ncov, most, self.ndim, "with" if self.has_transform else "without"))
        self.source = loglike_source if transform_source is None else loglike_source + "\n" + transform_source
        self.aux = np.empty(0) if aux is None else f64(np.ravel(aux)).copy()
        DeviceModel._count += 1
        self.name = name or "DeviceModel%d" % DeviceModel._count
        self._forms = {}
        self.code = self._compile(self.has_transform, False)
        # the derive program: the model's source (helpers included) followed by the derived source; the main programs above
        # are compiled from self.source alone, as those of the model without nderived
        self.derived_source = derived_source
        self.derive_code = None if self.nderived is None else compile_derived(self.source + "\n" + derived_source)
        self._handles = {}
        self.loglike = _Callback(self, "loglike")
        self.transform = _Callback(self, "transform")

    @property
    def summed(self):
        return self.nterms is not None

    def _form(self, tr, gated, derived=None):
        """(remembered: every route asks for its handle once per device call)"""
        key = (tr, gated, derived)
        if key not in self._forms:
            self._forms[key] = DERIVE if derived == "derive" else Form(tr, gated, self.summed, self.nsums, derived, self.ncov)
        return self._forms[key]

    def _compile(self, tr, gated, derived=None):
        """the code object of one of the model's programs: the derived kinds over the source followed by the derived source"""
        if derived is None:
            return compile_form(self.source, self._form(tr, gated))
        if self.nderived is None:
            raise ValueError("%s has no derived parameters (nderived)" % self.name)
        return compile_form(self.source + "\n" + self.derived_source, self._form(tr, gated, derived))

    def compile_gate_derived(self, with_transform=True):
        """The code object of the model's gate-derived program (needs no GPU; cached per process)."""
        return self._compile(bool(with_transform and self.has_transform), True, "gate")

    def handle(self, with_transform=True, gated=False, derived=False):
        """The loaded model (created on first use: needs the GPU).  with_transform=False: the variant whose prior
        transform is the identity (a route that pairs this model's likelihood with ``identity_transform``).  gated=True:
        the variant with the t-region test (compiled and loaded on first gated use; it runs in a gated refill only).  A summed
        model (``nterms``) loads its own programs under its own keys, and so does one of several sums (``nsums``).
        gated=True, derived=True: the gate over ``[p | q]`` (a model with ``nderived``; compiled and loaded on first such use; it
        runs in ``mlf_region_refill_user_derived_gated`` only)."""
        return self._load(bool(with_transform and self.has_transform), bool(gated), "gate" if derived else None)

    def derive_handle(self):
        """The loaded derive program (created on first use: needs the GPU); cached with the model's other handles."""
        return self._load(False, False, "derive")

    def _load(self, tr, gated, derived):
        """the handle of one program, keyed by its Form; compiled unless it is one of the constructor's two programs"""
        form = self._form(tr, gated, derived)
        h = self._handles.get(form)
        if h is None:
            code = {self._form(self.has_transform, False): self.code, DERIVE: self.derive_code}.get(form)
            # (a count that is not the form's stays out of the call)
            counts = dict(nterms=self.nterms if form.summed else None, nsums=form.nsums, derived=form.derived,
                          nderived=self.nderived if form.derived else None, ncov=form.ncov)
            h = self._handles[form] = _Handle(code or self._compile(tr, gated, derived), self.ndim, tr, self.aux, gated=gated,
                                              **{k: v for k, v in counts.items() if v is not None})
        return h.handle

    def close(self):
        """Unload the model now (after the library's stream has finished with it)."""
        for h in self._handles.values():
            h.close()
        self._handles = {}

    def _rows(self, x):
        a = f64(x)
        if a.ndim != 2 or a.shape[1] != self.ndim:
            raise ValueError("%s expects an (n, %d) array, got shape %s" % (self.name, self.ndim, np.shape(x)))
        return a

    def _loglike(self, theta):
        if self.nderived is not None and np.ndim(theta) == 2 and np.shape(theta)[1] == self.nparams:
            theta = np.asarray(theta)[:, :self.ndim]      # the likelihood does not see the derived columns
        p = self._rows(theta)
        out = np.empty(p.shape[0])
        if p.shape[0]:
            check(_lib.lib().mlf_usermodel_eval(self.handle(), ptr(p), p.shape[0], None, ptr(out)))
        return out

    def _transform(self, u):
        x = self._rows(u)
        out = np.empty_like(x)
        if x.shape[0]:
            check(_lib.lib().mlf_usermodel_eval(self.handle(), ptr(x), x.shape[0], ptr(out), None))
        return out if self.nderived is None else self.derive(out)

    def cov_factor(self, theta, with_transform=False):
        """The factorisation behind the likelihood of a covariance model (``ncov=n``), for GP prediction: host rows ``(m, ndim)``
        -- parameters, or cube rows with ``with_transform=True`` -- give ``(Lfac (m, n, n), z (m, n), L (m,))``: the lower
        triangular Cholesky factor of K (zeros above the diagonal), ``z = Lfac^-1 r`` and the likelihood, exactly the values the
        kernel computed (module docstring, "The arithmetic contract").  A row whose factorisation failed has NaN throughout
        ``Lfac`` and ``z``."""
        if self.ncov is None:
            raise ValueError("%s is no covariance model (ncov)" % self.name)
        x = self._rows(theta)
        n, m = self.ncov, x.shape[0]
        tri = np.empty((m, (n + 1) * (n + 2) // 2))
        out = np.empty(m)
        if m:
            check(_lib.lib().mlf_covmodel_factor(self.handle(bool(with_transform)), ptr(x), m, ptr(tri), ptr(out)))
        rows, cols = np.tril_indices(n + 1)      # row-major over the lower triangle: the packed order
        full = np.zeros((m, n + 1, n + 1))
        full[:, rows, cols] = tri
        return np.ascontiguousarray(full[:, :n, :n]), np.ascontiguousarray(full[:, n, :n]), out

    def derive(self, p):
        """Host rows ``(n, ndim)`` of parameters -> ``(n, ndim + nderived)``: ``[p | q]`` with q from ``mlf_user_derived``."""
        if self.nderived is None:
            raise ValueError("%s has no derived parameters (nderived)" % self.name)
        x = self._rows(p)
        out = np.empty((x.shape[0], self.nparams))
        if x.shape[0]:
            check(_lib.lib().mlf_usermodel_derive(self.derive_handle(), ptr(x), x.shape[0], ptr(out)))
        return out

    def derive_dev(self, d_p, n, d_out, stream=0):
        """`derive` on device pointers: d_p (n, ndim) -> d_out (n, ndim + nderived), which must not overlap.  Enqueued on
        `stream`."""
        check(_lib.lib().mlf_usermodel_derive_dev(self.derive_handle(), ctypes.c_void_p(d_p), int(n), ctypes.c_void_p(d_out),
                                                  ctypes.c_void_p(stream)))

    def eval_dev(self, d_u, n, d_p=None, d_L=None, d_member=None, stream=0):
        """Device pointers (e.g. ``tensor.data_ptr()``): p = transform(u) when d_p is given, L = loglike(p or u) when d_L
        is given; rows with d_member[i] == 0 are not evaluated (L = -inf).  Enqueued on `stream`."""
        check(_lib.lib().mlf_usermodel_eval_dev(self.handle(), ctypes.c_void_p(d_u), int(n), ctypes.c_void_p(d_member),
                                                ctypes.c_void_p(d_p), ctypes.c_void_p(d_L), ctypes.c_void_p(stream)))


def is_user_spec(spec):
    return isinstance(spec, UserModelSpec)


def device_route(transform, loglike):
    """``(model, with_transform)`` when this callback pair runs on a user model's device route, else None: `loglike` is a
    model's loglike and `transform` is that model's transform or ``likelihoods.identity_transform``."""
    from .likelihoods import identity_transform
    lspec = getattr(loglike, "device_spec", None)
    if not isinstance(lspec, UserModelSpec) or lspec.role != "loglike":
        return None
    model = lspec.model
    if transform is identity_transform:      # (the host route then yields no derived columns: neither does the device route)
        return model, False
    tspec = getattr(transform, "device_spec", None)
    if isinstance(tspec, UserModelSpec) and tspec.role == "transform" and tspec.model is model:
        return model, True
    return None


def extend_derived(user, p):
    """The p rows ``(n, ndim)`` (or one row ``(ndim,)``) a device route hands out for ``user = (model, with_transform)``,
    with the model's derived columns where the host route would yield them: a model with ``nderived`` paired with its own
    transform.  Every other `p` comes back as it is."""
    if user is None or not user[1] or user[0].nderived is None:
        return p
    p = np.asarray(p)
    return user[0].derive(p[None, :])[0] if p.ndim == 1 else user[0].derive(p)


__all__ = ["DeviceModel", "DeviceModelCompileError", "UserModelSpec", "compile_model", "compile_derived", "compile_gate_derived",
           "device_route", "extend_derived"]
