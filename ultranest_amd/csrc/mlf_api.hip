// mlf_api.hip -- the library itself behind the C ABI of libmlfriends_hip.so (include/mlfriends_hip.h): error text, tuning
// options, the context (one device, one stream), host<->device staging and the device-memory entry points.  The single
// definition of every piece of state the host units share (mlf_host.hpp).  No numerics live here.
#include <hip/hip_runtime.h>

#include <atomic>
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

#include "../../include/mlfriends_hip.h"
#include "mlf_host.hpp"

namespace {

using namespace mlf;

thread_local std::string g_err;

const char *const kOptNames[OPT_COUNT] = {"filter", "filter_first_range_pct", "filter_split_waves", "filter_narrow_tail",
                                          "small_path", "fused_prep", "filter_phase_min_queries", "filter_phases",
                                          "time_filter_launches", "prep_bounded", "filter_min_queries", "sweep_min", "mid_max_queries", "fused_first_range",
                                          "boot_symmetric", "filter_order", "filter_second_range_pct", "filter_third_range_min_work", "fused_waves", "fused_variant"};

int opt_id(const char *name) {
  for (int i = 0; i < OPT_COUNT; ++i)
    if (!strcmp(name, kOptNames[i])) return i;
  return -1;
}

long long opt_clamp(int id, long long value) {
  switch (id) {
    case OPT_FIRST_RANGE_PCT: return value < 10 ? 10 : (value > 90 ? 90 : value);
    case OPT_SPLIT_WAVES: return value < 256 ? 256 : (value > 16384 ? 16384 : value);
    case OPT_PHASES: return value < 0 ? 0 : (value > 64 ? 64 : value);
    case OPT_SECOND_RANGE_PCT: return value < 0 ? 0 : (value > 90 ? 90 : value);
    case OPT_FUSED_WAVES: return value == 4 ? 4 : 8;
    case OPT_FUSED_VARIANT: return value & 3;
    case OPT_BOOT_SYM: return value < 0 ? 0 : (value > 2 ? 2 : value);
    case OPT_THIRD_MIN_WORK: return value < 0 ? 0 : value;
    case OPT_PHASE_MIN_QUERIES:
    case OPT_MID_MAX:
    case OPT_MIN_QUERIES: return value;
    default: return value != 0;
  }
}

}  // namespace

namespace mlf {

std::atomic<unsigned> g_grant_epoch{0u};
std::atomic<unsigned long long> g_grant_calls{0ull};
long long g_opt[OPT_COUNT] = {1, 30, 2048, 1, 1, 1, 32768, 1, 0, 1, kFilterMinQueriesDefault, 1, 2048, 1, 1, 1, 50, 100000000ll, 4, 3};

Ctx g_ctx;

HostArena *g_arena = nullptr;

int fail_hip(hipError_t e, const char *what, const char *file, int line) {
  char buf[512];
  snprintf(buf, sizeof buf, "HIP error %d (%s) at %s:%d: %s", (int)e, hipGetErrorString(e), file, line, what);
  g_err = buf;
  return -(int)e;
}

int fail_arg(int code, const char *msg) {
  g_err = msg;
  return code;
}

int ensure_ctx() {
  if (g_ctx.ready) return 0;
  int count = 0;
  hipError_t e = hipGetDeviceCount(&count);
  if (e != hipSuccess || count <= 0) {
    g_err = "libmlfriends_hip: no HIP device visible (this library has no CPU fallback)";
    return MLF_E_NODEVICE;
  }
  CK(hipSetDevice(g_ctx.device));
  CK(hipStreamCreate(&g_ctx.stream));
  g_ctx.ready = true;
  return 0;
}

hipStream_t ctx_stream() { return g_ctx.stream; }

// d x d row-major -> d rows of dp doubles, zero padded; optional transpose
std::vector<double> pad_matrix(const double *m, int d, int dp, bool transpose) {
  std::vector<double> o((size_t)d * dp, 0.0);
  for (int r = 0; r < d; ++r)
    for (int c = 0; c < d; ++c) o[(size_t)r * dp + c] = transpose ? m[(size_t)c * d + r] : m[(size_t)r * d + c];
  return o;
}

std::vector<double> pad_vector(const double *v, int d, int dp, double fill) {
  std::vector<double> o((size_t)dp, fill);
  for (int k = 0; k < d; ++k) o[k] = v[k];
  return o;
}

bool arena_active() { return g_arena != nullptr; }

// Everything staged so far leaves in ONE launch (the device reads the pinned arena itself).  To be called in front of every
// kernel that reads a constant uploaded under the arena, and before the arena is dropped.
int arena_flush(hipStream_t s) {
  if (!g_arena || g_arena->npending == 0) return 0;
  launch_scatter_copy(g_arena->pending, g_arena->npending, s);
  g_arena->npending = 0;
  CK(hipGetLastError());
  return 0;
}

bool is_device_pointer(const void *p) {
  hipPointerAttribute_t attr;
  if (hipPointerGetAttributes(&attr, p) != hipSuccess) {
    (void)hipGetLastError();   // plain host memory the runtime has never seen
    return false;
  }
  return attr.type == hipMemoryTypeDevice;
}

// `src` may be a host or a device pointer (unified addressing picks the direction): the array arguments of the
// stateless entry points can stay on the device between calls (device-resident rebuild, ultranest_amd.device_rebuild)
int upload(DevBuf &b, const void *src, size_t bytes, hipStream_t s) {
  CK(b.reserve(bytes ? bytes : 1));
  if (!bytes) return 0;
  // the arena branch reads `src` with a host memcpy: never for a device pointer (mlf_region_set accepts the live points
  // from either side; VRAM is host-readable only on large-BAR boxes)
  if (g_arena && bytes <= kArenaMaxPiece && !is_device_pointer(src)) {
    if (void *stage = g_arena->take(bytes)) {
      memcpy(stage, src, bytes);
      if (g_arena->npending == kScatterMax)
        if (int rc = arena_flush(s)) return rc;
      HostArena &a = *g_arena;
      a.pending.dst[a.npending] = b.p;
      a.pending.src[a.npending] = a.p_dev + (static_cast<unsigned char *>(stage) - a.p);
      a.pending.bytes[a.npending] = (unsigned)bytes;
      ++a.npending;
      return 0;
    }
  }
  if (int rc = arena_flush(s)) return rc;   // keep the order of the stream
  CK(hipMemcpyAsync(b.p, src, bytes, hipMemcpyDefault, s));
  if (g_arena) CK(hipStreamSynchronize(s));   // did not fit: the caller relies on the source being consumed
  return 0;
}

// like upload(), but `src` may be a host OR a device pointer (unified addressing picks the direction): the bootstrap
// selection masks arrive from a device-side broadcast in the multi-GPU rebuild
int upload_any(DevBuf &b, const void *src, size_t bytes, hipStream_t s) {
  CK(b.reserve(bytes ? bytes : 1));
  if (bytes) CK(hipMemcpyAsync(b.p, src, bytes, hipMemcpyDefault, s));
  return 0;
}

int check_dims(size_t d) {
  if (d == 0) return fail_arg(MLF_E_BADARG, "dimensionality must be positive");
  if (d > MLF_MAX_DIM) return fail_arg(MLF_E_DIM, "dimensionality above MLF_MAX_DIM (1024) is not supported");
  return 0;
}

// Live points (row-major, host) -> device layouts in the context scratch.
int stage_live_points(const double *pts, size_t n, size_t d, int dp, int npad, bool want_rows) {
  Ctx &c = g_ctx;
  int rc = upload(c.src, pts, n * d * sizeof(double), c.stream);
  if (rc) return rc;
  CK(c.refT.reserve((size_t)npad * dp * sizeof(double)));
  CK(c.refR.reserve((size_t)(npad + 1) * dp * sizeof(double)));   // k_boot requests the first block of the row after its last
  (void)want_rows;
  launch_build_layouts(c.src.as<double>(), (int)n, (int)d, dp, npad, c.refT.as<double>(),
                       c.refR.as<double>(), c.stream);
  CK(hipGetLastError());
  return 0;
}

int prep_consts(DevBuf &ctr_b, DevBuf &mat_b, const double *ctr, const double *mat, int d, int dp,
                bool transpose, hipStream_t s) {
  std::vector<double> pc = pad_vector(ctr, d, dp);
  std::vector<double> pm = pad_matrix(mat, d, dp, transpose);
  if (int rc = upload(ctr_b, pc.data(), pc.size() * sizeof(double), s)) return rc;
  if (int rc = upload(mat_b, pm.data(), pm.size() * sizeof(double), s)) return rc;
  if (!arena_active()) CK(hipStreamSynchronize(s));  // host vectors go out of scope
  return 0;
}

int pick_dp(int d) {
#define X(D) \
  if (d <= D) return D;
  MLF_FOR_EACH_DP(X)
#undef X
  if (d <= MLF_MAX_DIM) return (d + 15) / 16 * 16;   // above 128: the run-time kernels of mlf_wide.hip, coordinates padded to 16
  return -1;
}

}  // namespace mlf

extern "C" {

int mlf_abi_version(void) { return MLF_ABI_VERSION; }

const char *mlf_last_error(void) { return g_err.c_str(); }

int mlf_device_count(int *count) {
  if (!count) return fail_arg(MLF_E_BADARG, "null pointer");
  int c = 0;
  hipError_t e = hipGetDeviceCount(&c);
  *count = (e == hipSuccess) ? c : 0;
  return 0;
}

int mlf_set_device(int device) {
  if (g_ctx.ready && device != g_ctx.device)
    return fail_arg(MLF_E_STATE, "mlf_set_device must be called before the first compute call");
  g_ctx.device = device;
  return 0;
}

int mlf_device_name(char *buf, size_t buflen) {
  if (!buf || !buflen) return fail_arg(MLF_E_BADARG, "null pointer");
  if (int rc = ensure_ctx()) return rc;
  hipDeviceProp_t prop;
  CK(hipGetDeviceProperties(&prop, g_ctx.device));
  snprintf(buf, buflen, "%s (%s, %d CUs)", prop.name, prop.gcnArchName, prop.multiProcessorCount);
  return 0;
}

int mlf_set_option(const char *name, long long value) {
  if (!name) return fail_arg(MLF_E_BADARG, "null pointer");
  const int id = opt_id(name);
  if (id < 0) return fail_arg(MLF_E_BADARG, "unknown option");
  g_opt[id] = opt_clamp(id, value);
  return 0;
}

int mlf_get_option(const char *name, long long *value) {
  if (!name || !value) return fail_arg(MLF_E_BADARG, "null pointer");
  const int id = opt_id(name);
  if (id < 0) return fail_arg(MLF_E_BADARG, "unknown option");
  *value = g_opt[id];
  return 0;
}

int mlf_region_get_option(mlf_region *r, const char *name, long long *value) {
  if (!r || !name || !value) return fail_arg(MLF_E_BADARG, "null pointer");
  const int id = opt_id(name);
  if (id < 0) return fail_arg(MLF_E_BADARG, "unknown option");
  *value = opt(r->filter, id);
  return 0;
}

int mlf_region_set_option(mlf_region *r, const char *name, long long value, int inherit) {
  if (!r) return fail_arg(MLF_E_BADARG, "null pointer");
  if (!name) {   // every option of the handle back to the process defaults (a recycled handle starts clean)
    if (!inherit) return fail_arg(MLF_E_BADARG, "null pointer");
    if (r->filter.ov.set[OPT_ORDER] && r->filter.refs_ready) r->filter.refs_dirty = true;
    r->filter.ov = OptOverrides{};
    return 0;
  }
  const int id = opt_id(name);
  if (id < 0) return fail_arg(MLF_E_BADARG, "unknown option");
  r->filter.ov.set[id] = !inherit;
  r->filter.ov.v[id] = inherit ? 0 : opt_clamp(id, value);
  if (id == OPT_ORDER && r->filter.refs_ready) r->filter.refs_dirty = true;   // the next batch builds (or drops) the ordered operand
  return 0;
}

int mlf_option_name(int index, char *buf, size_t buflen) {
  if (!buf || !buflen || index < 0 || index >= OPT_COUNT) return fail_arg(MLF_E_BADARG, "no such option");
  snprintf(buf, buflen, "%s", kOptNames[index]);
  return 0;
}

int mlf_synchronize(void) {
  if (int rc = ensure_ctx()) return rc;
  CK(hipDeviceSynchronize());
  return 0;
}

// ---- device memory for callers that keep arrays resident between calls (ultranest_amd.device_rebuild) -------------------
int mlf_dev_alloc(size_t bytes, void **out) {
  if (!out) return fail_arg(MLF_E_BADARG, "null pointer");
  if (int rc = ensure_ctx()) return rc;
  CK(hipMalloc(out, bytes ? bytes : 1));
  return 0;
}

int mlf_dev_free(void *p) {
  if (!p) return 0;
  if (int rc = ensure_ctx()) return rc;
  CK(hipFree(p));
  return 0;
}

// dst / src: host or device (unified addressing picks the direction); ordered on the library's stream; `sync` != 0 waits
// for it (needed before a host destination is read or a host source is re-used)
int mlf_dev_copy(void *dst, const void *src, size_t bytes, int sync) {
  if (bytes && (!dst || !src)) return fail_arg(MLF_E_BADARG, "null pointer");
  if (int rc = ensure_ctx()) return rc;
  Ctx &c = g_ctx;
  if (bytes) CK(hipMemcpyAsync(dst, src, bytes, hipMemcpyDefault, c.stream));
  if (sync) CK(hipStreamSynchronize(c.stream));
  return 0;
}

// lo[c], hi[c] = extents of column c of the (n, d) row-major array `pts` (host or device); lo / hi on the host
int mlf_col_extent(const double *pts, size_t n, size_t d, double *lo, double *hi) {
  if (int rc = check_dims(d)) return rc;
  if (d > 128) return fail_arg(MLF_E_DIM, "mlf_col_extent covers up to 128 columns (the device-resident rebuild it serves: d <= 64)");
  if (!pts || !lo || !hi || n == 0) return fail_arg(MLF_E_BADARG, "null pointer or no rows");
  if (int rc = ensure_ctx()) return rc;
  Ctx &c = g_ctx;
  const double *dp = pts;
  if (!is_device_pointer(pts)) {
    if (int rc = upload(c.src, pts, n * d * sizeof(double), c.stream)) return rc;
    dp = c.src.as<double>();
  }
  CK(c.small2.reserve((size_t)(kExtentScratchBlocks + 1) * 2 * d * sizeof(double)));
  double *part = c.small2.as<double>();
  double *out = part + (size_t)kExtentScratchBlocks * 2 * d;
  launch_col_extent(dp, (int)n, (int)d, part, out, c.stream);
  CK(hipGetLastError());
  std::vector<double> h(2 * d);
  CK(hipMemcpyAsync(h.data(), out, 2 * d * sizeof(double), hipMemcpyDeviceToHost, c.stream));
  CK(hipStreamSynchronize(c.stream));
  memcpy(lo, h.data(), d * sizeof(double));
  memcpy(hi, h.data() + d, d * sizeof(double));
  return 0;
}

}  // extern "C"
