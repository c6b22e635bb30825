"""User-written likelihoods and prior transforms that run on the GPU.

The GPU counterpart of the reference's compiled-language likelihoods (reference languages/c/mylib.c: the
``(params, d, n, like)`` convention that ``ultranest_amd.likelihoods`` follows): the user writes two HIP
device functions, the package compiles them at run time for gfx950 (hiprtc) around one wrapper kernel
(``csrc/mlf_user_rows.hpp``) and hands back a pair of vectorized callbacks::

    model = DeviceModel(ndim, loglike_source, transform_source=None, aux=None)
    model.loglike(theta)    # (n, ndim) -> (n,)       vectorized callback, evaluated on the GPU
    model.transform(u)      # (n, ndim) -> (n, ndim)  vectorized callback (identity without a transform source)

The sources define::

    __device__ double mlf_user_loglike(const double *p, int d, const double *aux, long long naux);           // required
    __device__ void mlf_user_transform(const double *u, double *p, int d, const double *aux, long long naux);  // optional

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

Derived parameters (``num_params != x_dim``) keep the host route: a model has ``nparams == ndim``.

Compiling needs no GPU; code objects are cached per process, keyed by a hash of the source, the options and the
wrapper header.  Evaluating without a GPU raises ``HipLibraryError`` like every other compute call (no CPU fallback).
"""
import ctypes
import hashlib
import os

import numpy as np

from . import _lib
from ._lib import check, f64, ptr

INCLUDE_DIR = os.path.join(os.path.dirname(os.path.abspath(__file__)), "csrc")
HEADER = os.path.join(INCLUDE_DIR, "mlf_user_rows.hpp")
GATE_HEADER = os.path.join(INCLUDE_DIR, "mlf_tregion_dev.hpp")      # included by the gated variant only
VARIANT_DEFAULT, VARIANT_TREGION = 0, 1                             # MLF_USERMODEL_* of include/mlfriends_hip.h
# what mlf_usermodel_compile passes to hiprtc besides -I, -DMLF_USER_HAS_TRANSFORM and -DMLF_USER_TREGION (part of the cache key)
COMPILE_OPTIONS = ("--offload-arch=gfx950", "-O3", "-std=c++17", "-ffp-contract=off")
MLF_E_COMPILE = 5

_code_cache = {}
compile_calls = 0      # hiprtc compiles made by this process (the cache avoids repeats)


class DeviceModelCompileError(RuntimeError):
    """hiprtc rejected the model's source (or hiprtc is not available); ``log`` holds its diagnostics."""

    def __init__(self, log):
        self.log = log
        RuntimeError.__init__(self, "the device model did not compile:\n" + log)


def _cache_key(source, has_transform, gated=False):
    h = hashlib.sha256()
    with open(HEADER, "rb") as fh:
        header = fh.read()
    options = repr((COMPILE_OPTIONS, bool(has_transform)))
    if gated:
        options += " tregion"
        with open(GATE_HEADER, "rb") as fh:
            header += fh.read()
    for part in (source.encode(), b"\0", options.encode(), b"\0", header):
        h.update(part)
    return h.hexdigest()


def compile_model(source, has_transform, gated=False):
    """The gfx950 code object (bytes) of `source` + the wrapper kernel; cached per process.  gated: the variant with the
    t-region test between transform and likelihood (module docstring), another program under its own key."""
    global compile_calls
    key = _cache_key(source, has_transform, gated)
    code = _code_cache.get(key)
    if code is not None:
        return code
    L = _lib.lib()
    size = ctypes.c_size_t(0)
    log = ctypes.create_string_buffer(1 << 16)
    cap = 1 << 20
    for _ in range(2):
        buf = ctypes.create_string_buffer(cap)
        compile_calls += 1
        if gated:
            rc = L.mlf_usermodel_compile_variant(source.encode(), INCLUDE_DIR.encode(), int(bool(has_transform)),
                                                 VARIANT_TREGION, buf, cap, ctypes.byref(size), log, len(log))
        else:
            rc = L.mlf_usermodel_compile(source.encode(), INCLUDE_DIR.encode(), int(bool(has_transform)), buf, cap,
                                         ctypes.byref(size), log, len(log))
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
    """One loaded model (``mlf_usermodel``) on the library's device."""

    def __init__(self, code, ndim, has_transform, aux, gated=False):
        h = ctypes.c_void_p()
        if gated:
            check(_lib.lib().mlf_usermodel_create_variant(code, len(code), int(ndim), int(bool(has_transform)),
                                                          VARIANT_TREGION, ptr(aux), len(aux), ctypes.byref(h)))
        else:
            check(_lib.lib().mlf_usermodel_create(code, len(code), int(ndim), int(bool(has_transform)), ptr(aux), len(aux),
                                                  ctypes.byref(h)))
        self._h = h
        self.has_transform = bool(has_transform)

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
    """A likelihood (and optional prior transform) written as HIP device functions (module docstring)."""

    _count = 0

    def __init__(self, ndim, loglike_source, transform_source=None, aux=None, name=None):
        self.ndim = int(ndim)
        if self.ndim <= 0:
            raise ValueError("ndim must be positive")
        self.has_transform = transform_source is not None
        self.source = loglike_source if transform_source is None else loglike_source + "\n" + transform_source
        self.aux = np.empty(0) if aux is None else f64(np.ravel(aux)).copy()
        DeviceModel._count += 1
        self.name = name or "DeviceModel%d" % DeviceModel._count
        self.code = compile_model(self.source, self.has_transform)
        self._handles = {}
        self.loglike = _Callback(self, "loglike")
        self.transform = _Callback(self, "transform")

    def handle(self, with_transform=True, gated=False):
        """The loaded model (created on first use: needs the GPU).  with_transform=False: the variant whose prior
        transform is the identity (a route that pairs this model's likelihood with ``identity_transform``).  gated=True:
        the variant with the t-region test (compiled and loaded on first gated use; it runs in a gated refill only)."""
        tr = bool(with_transform and self.has_transform)
        key = (tr, True) if gated else tr
        h = self._handles.get(key)
        if h is None:
            if gated:
                code = compile_model(self.source, tr, gated=True)
            else:
                code = self.code if tr == self.has_transform else compile_model(self.source, tr)
            h = self._handles[key] = _Handle(code, self.ndim, tr, self.aux, gated=gated)
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
        return out

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
    if transform is identity_transform:
        return model, False
    tspec = getattr(transform, "device_spec", None)
    if isinstance(tspec, UserModelSpec) and tspec.role == "transform" and tspec.model is model:
        return model, True
    return None


__all__ = ["DeviceModel", "DeviceModelCompileError", "UserModelSpec", "compile_model", "device_route"]
