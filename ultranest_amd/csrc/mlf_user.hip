// mlf_user.hip -- user models (include/mlfriends_hip.h, section "user models"): a likelihood and prior transform written
// as HIP device functions, compiled at run time by hiprtc around mlf_user_rows.hpp, loaded as a module on the library's
// device and launched on the library's stream (ordered with the kernels around it: the refill and walker routes of
// mlf_region_sample.hip / mlf_walk_api.hip call usermodel_rows between their own launches).
//
// hiprtc is loaded with dlopen, not linked: where it is missing the library loads and every other entry point works;
// mlf_usermodel_compile then fails with MLF_E_COMPILE and says why.
#include <hip/hip_runtime.h>
#include <hip/hiprtc.h>   // types and prototypes only: the functions are looked up in the dlopen'ed library

#include <dlfcn.h>

#include <cstdlib>
#include <cstring>
#include <mutex>
#include <string>
#include <vector>

#include "../../include/mlfriends_hip.h"
#include "mlf_ctx.hpp"
#define MLF_USER_ROWS_HOST
#include "mlf_user_rows.hpp"

using namespace mlf;

struct mlf_usermodel {
  hipModule_t module = nullptr;
  hipFunction_t fn = nullptr;
  int d = 0;
  bool has_transform = false;
  bool gated = false;   // the MLF_USERMODEL_TREGION / _SUM_TREGION / _SUMS_TREGION variants: the kernel takes the gate's five
                        // parameters as well
  bool summed = false;  // the MLF_USERMODEL_SUM / _SUM_TREGION / _SUMS / _SUMS_TREGION variants: one wave per row, nterms behind
                        // the first eight parameters (the number of sums is baked into a _SUMS program)
  long long nterms = 0;
  int nderived = 0;     // the MLF_USERMODEL_DERIVED variant: fn is mlf_user_derive_rows, p (n, d) -> [p | q] (n, d + nderived); such a
                        // handle runs in the derive entries only
  int gate_nq = 0;      // the _TREGION_DERIVED variants (gated is set too): the kernel computes this many derived columns per member
                        // row, gates over d + gate_nq columns and takes (nq, q_scratch) behind the gate's five parameters; such a
                        // handle runs in mlf_region_refill_user_derived_gated only
  long long naux = 0;
  DevBuf aux;
  DevBuf hu, hp, hL;   // staging of mlf_usermodel_eval (host arrays)
};

namespace {

struct Rtc {
  bool tried = false;
  void *handle = nullptr;
  std::string why;
  decltype(&hiprtcCreateProgram) create = nullptr;
  decltype(&hiprtcCompileProgram) compile = nullptr;
  decltype(&hiprtcDestroyProgram) destroy = nullptr;
  decltype(&hiprtcGetCodeSize) code_size = nullptr;
  decltype(&hiprtcGetCode) code = nullptr;
  decltype(&hiprtcGetProgramLogSize) log_size = nullptr;
  decltype(&hiprtcGetProgramLog) log = nullptr;
  decltype(&hiprtcGetErrorString) error_string = nullptr;
};
Rtc g_rtc;
std::mutex g_rtc_mutex;   // one hiprtc compile at a time

template <class F>
bool rtc_sym(void *h, const char *name, F &f) {
  f = reinterpret_cast<F>(dlsym(h, name));
  return f != nullptr;
}

// under g_rtc_mutex
bool rtc_load() {
  Rtc &r = g_rtc;
  if (r.tried) return r.handle != nullptr;
  r.tried = true;
  std::vector<std::string> names = {"libhiprtc.so", "libhiprtc.so.7"};
  const char *rocm = getenv("ROCM_PATH");
  names.push_back(std::string(rocm && *rocm ? rocm : "/opt/rocm") + "/lib/libhiprtc.so");
  std::string errors;
  for (const std::string &n : names) {
    r.handle = dlopen(n.c_str(), RTLD_NOW | RTLD_LOCAL);
    if (r.handle) break;
    const char *e = dlerror();
    errors += "\n  " + n + ": " + (e ? e : "not found");
  }
  if (!r.handle) {
    r.why = "libhiprtc.so (the HIP run-time compiler, part of ROCm) could not be loaded:" + errors;
    return false;
  }
  if (!rtc_sym(r.handle, "hiprtcCreateProgram", r.create) || !rtc_sym(r.handle, "hiprtcCompileProgram", r.compile) ||
      !rtc_sym(r.handle, "hiprtcDestroyProgram", r.destroy) || !rtc_sym(r.handle, "hiprtcGetCodeSize", r.code_size) ||
      !rtc_sym(r.handle, "hiprtcGetCode", r.code) || !rtc_sym(r.handle, "hiprtcGetProgramLogSize", r.log_size) ||
      !rtc_sym(r.handle, "hiprtcGetProgramLog", r.log) || !rtc_sym(r.handle, "hiprtcGetErrorString", r.error_string)) {
    r.why = "libhiprtc.so lacks an expected hiprtc entry point";
    dlclose(r.handle);
    r.handle = nullptr;
    return false;
  }
  return true;
}

void put_log(char *log, size_t cap, const std::string &text) {
  if (!log || cap == 0) return;
  const size_t k = text.size() < cap - 1 ? text.size() : cap - 1;
  memcpy(log, text.data(), k);
  log[k] = '\0';
}

}  // namespace

namespace mlf {

int usermodel_dim(const mlf_usermodel *m) { return m->d; }
bool usermodel_has_transform(const mlf_usermodel *m) { return m->has_transform; }
bool usermodel_gated(const mlf_usermodel *m) { return m->gated; }
int usermodel_nderived(const mlf_usermodel *m) { return m->nderived; }
int usermodel_gate_nderived(const mlf_usermodel *m) { return m->gate_nq; }

int usermodel_rows(const mlf_usermodel *m, const double *u, long long n, const uint8_t *member, double *p, double *L,
                   hipStream_t s, const TregionGate *gate) {
  if (m->nderived) return fail_arg(MLF_E_STATE, "a derive handle (mlf_usermodel_create_derived) evaluates nothing: it runs in the derive entries only");
  // the two variants differ in their parameter lists: never launch one with the other's
  if (m->gated != (gate != nullptr))
    return fail_arg(MLF_E_STATE, m->gated ? "user model loaded as the t-region variant: it runs only in a refill with a t-region set"
                                          : "user model not loaded as the t-region variant (mlf_usermodel_create_variant)");
  // a gate over derived columns is w = d + gate_nq wide and brings the q rows' scratch; every other gate is d wide
  if (m->gate_nq ? (gate->width != m->d + m->gate_nq || gate->q_scratch == nullptr) : (gate != nullptr && gate->width != 0))
    return fail_arg(MLF_E_STATE, m->gate_nq ? "user model loaded as a _TREGION_DERIVED variant: it runs only in "
                                              "mlf_region_refill_user_derived_gated, with a t-region over d + nderived columns"
                                            : "a t-region over d + nderived columns needs a user model loaded as a _TREGION_DERIVED "
                                              "variant (mlf_usermodel_create_gate_derived)");
  if (n <= 0) return 0;
  // default form: one thread per row, 64 rows per workgroup; summed form: one wave (= one workgroup) per row
  const long long blocks = m->summed ? n : (n + 63) / 64;
  if (blocks > 0x7fffffffLL) return fail_arg(MLF_E_BADARG, "user model: too many rows for one launch");
  const bool p_buffer = p != nullptr && m->has_transform;
  const unsigned lds = m->gate_nq ? (m->summed ? mlf_user_rows_sum_gate_derived_lds_bytes(m->d, m->gate_nq, p_buffer)
                                               : mlf_user_rows_gate_derived_lds_bytes(m->d, m->gate_nq, p_buffer))
                       : m->summed ? mlf_user_rows_sum_lds_bytes(m->d, p_buffer)
                                   : mlf_user_rows_lds_bytes(m->d, p_buffer);
  // the kernel's parameters, in order and with its exact types (mlf_user_rows.hpp)
  const double *a_u = u;
  long long a_n = n;
  int a_d = m->d;
  const unsigned char *a_member = member;
  const double *a_aux = m->aux.as<double>();
  long long a_naux = m->naux;
  double *a_p = p, *a_L = L;
  long long a_nterms = m->nterms;
  const double *g_A = nullptr, *g_ctr = nullptr, *g_fixed = nullptr;
  double g_enlarge = 0.0;
  unsigned char *g_member2 = nullptr;
  if (gate) {
    g_A = gate->A, g_ctr = gate->ctr, g_fixed = gate->fixed_val;
    g_enlarge = gate->enlarge;
    g_member2 = gate->member2;
  }
  int g_nq = m->gate_nq;
  double *g_scratch = gate ? gate->q_scratch : nullptr;
  // the first eight, nterms in the ninth place of a summed model, the gate's five behind them when gated, (nq, q_scratch) behind
  // those in a _TREGION_DERIVED variant
  void *args[16] = {&a_u, &a_n, &a_d, &a_member, &a_aux, &a_naux, &a_p, &a_L};
  int na = 8;
  if (m->summed) args[na++] = &a_nterms;
  if (gate) {
    void *g[] = {&g_A, &g_ctr, &g_fixed, &g_enlarge, &g_member2};
    for (void *x : g) args[na++] = x;
  }
  if (m->gate_nq) {
    args[na++] = &g_nq;
    args[na++] = &g_scratch;
  }
  CK(hipModuleLaunchKernel(m->fn, (unsigned)blocks, 1, 1, 64, 1, 1, lds, s, args, nullptr));
  return 0;
}

int usermodel_derive_rows(const mlf_usermodel *m, const double *p, long long n, double *out, hipStream_t s) {
  if (!m->nderived) return fail_arg(MLF_E_STATE, "not a derive handle (mlf_usermodel_create_derived)");
  if (n <= 0) return 0;
  const long long blocks = (n + 63) / 64;   // one thread per row, 64 rows per workgroup
  if (blocks > 0x7fffffffLL) return fail_arg(MLF_E_BADARG, "user model: too many rows for one launch");
  const unsigned lds = mlf_user_rows_derive_lds_bytes(m->d, m->nderived);
  // the kernel's parameters, in order and with its exact types (mlf_user_rows.hpp)
  const double *a_p = p;
  long long a_n = n;
  int a_d = m->d, a_nq = m->nderived;
  const double *a_aux = m->aux.as<double>();
  long long a_naux = m->naux;
  double *a_out = out;
  void *args[7] = {&a_p, &a_n, &a_d, &a_nq, &a_aux, &a_naux, &a_out};
  CK(hipModuleLaunchKernel(m->fn, (unsigned)blocks, 1, 1, 64, 1, 1, lds, s, args, nullptr));
  return 0;
}

}  // namespace mlf

namespace {

// the gate over derived columns: the gated variants with MLF_USER_GATE_DERIVED=1
bool variant_gate_derived(int v) {
  return v == MLF_USERMODEL_TREGION_DERIVED || v == MLF_USERMODEL_SUM_TREGION_DERIVED || v == MLF_USERMODEL_SUMS_TREGION_DERIVED;
}
bool variant_gated(int v) {
  return v == MLF_USERMODEL_TREGION || v == MLF_USERMODEL_SUM_TREGION || v == MLF_USERMODEL_SUMS_TREGION || variant_gate_derived(v);
}
bool variant_multi(int v) { return v == MLF_USERMODEL_SUMS || v == MLF_USERMODEL_SUMS_TREGION || v == MLF_USERMODEL_SUMS_TREGION_DERIVED; }
bool variant_summed(int v) {
  return v == MLF_USERMODEL_SUM || v == MLF_USERMODEL_SUM_TREGION || v == MLF_USERMODEL_SUM_TREGION_DERIVED || variant_multi(v);
}

// the checks every create entry makes before it touches the device
int check_create_args(const void *code, size_t nbytes, size_t d) {
  if (d == 0) return fail_arg(MLF_E_BADARG, "dimensionality must be positive");
  if (d > MLF_MAX_DIM) return fail_arg(MLF_E_DIM, "user model: dimensionality above MLF_MAX_DIM");
  if (nbytes < 64 || memcmp(code, "\x7f" "ELF", 4) != 0) return fail_arg(MLF_E_BADARG, "not a code object (ELF)");
  return 0;
}

// loads the code object as `variant` (arguments checked by the caller); nterms: 0 unless the variant is a summed one; nderived:
// 0 unless the variant is MLF_USERMODEL_DERIVED (a derive handle) or a _TREGION_DERIVED one (the columns its gate spans)
int load_model(const void *code, size_t d, int has_transform, int variant, size_t nterms, const double *aux, size_t naux,
               mlf_usermodel **out, size_t nderived = 0) {
  if (int rc = ensure_ctx()) return rc;
  hipStream_t s = ctx_stream();
  mlf_usermodel *m = new mlf_usermodel();
  m->d = (int)d;
  m->has_transform = has_transform != 0;
  m->gated = variant_gated(variant);
  m->summed = variant_summed(variant);
  m->nterms = (long long)nterms;
  m->nderived = variant == MLF_USERMODEL_DERIVED ? (int)nderived : 0;
  m->gate_nq = variant_gate_derived(variant) ? (int)nderived : 0;
  m->naux = (long long)naux;
  const char *entry = variant == MLF_USERMODEL_DERIVED ? "mlf_user_derive_rows"
                      : variant == MLF_USERMODEL_TREGION_DERIVED      ? "mlf_user_rows_tregion_derived"
                      : variant == MLF_USERMODEL_SUM_TREGION_DERIVED  ? "mlf_user_rows_sum_tregion_derived"
                      : variant == MLF_USERMODEL_SUMS_TREGION_DERIVED ? "mlf_user_rows_sums_tregion_derived"
                      : variant_multi(variant) ? (m->gated ? "mlf_user_rows_sums_tregion" : "mlf_user_rows_sums")
                      : m->summed            ? (m->gated ? "mlf_user_rows_sum_tregion" : "mlf_user_rows_sum")
                                             : (m->gated ? "mlf_user_rows_tregion" : "mlf_user_rows");
  hipError_t e = hipModuleLoadData(&m->module, code);
  if (e == hipSuccess && hipModuleGetFunction(&m->fn, m->module, entry) != hipSuccess) {
    // the variants' entries differ in name: this code object was compiled as the other one (or is no user model at all)
    (void)hipGetLastError();
    (void)hipModuleUnload(m->module);
    delete m;
    return fail_arg(MLF_E_BADARG, "the code object has no entry of this variant (compiled as another variant?)");
  }
  if (e == hipSuccess) e = m->aux.reserve(naux ? naux * sizeof(double) : sizeof(double));
  if (e == hipSuccess && naux) e = hipMemcpyAsync(m->aux.p, aux, naux * sizeof(double), hipMemcpyHostToDevice, s);
  if (e == hipSuccess) e = hipStreamSynchronize(s);
  if (e != hipSuccess) {
    if (m->module) (void)hipModuleUnload(m->module);
    m->aux.release();
    delete m;
    return fail_hip(e, "mlf_usermodel_create", "mlf_user.hip", __LINE__);
  }
  *out = m;
  return 0;
}

// hiprtc on `source` + the wrapper header as `variant` (checked by the caller); nsums: 0 unless the variant is a _SUMS one
int compile_program(const char *source, const char *include_dir, int has_transform, int variant, int nsums, void *code_out,
                    size_t code_cap, size_t *code_size, char *log, size_t log_cap) {
  const bool v_gated = variant_gated(variant);
  const bool v_summed = variant_summed(variant);
  const bool v_derived = variant == MLF_USERMODEL_DERIVED;
  const bool v_gate_derived = variant_gate_derived(variant);
  *code_size = 0;
  put_log(log, log_cap, "");
  std::lock_guard<std::mutex> lock(g_rtc_mutex);
  if (!rtc_load()) {
    put_log(log, log_cap, g_rtc.why);
    return fail_arg(MLF_E_COMPILE, g_rtc.why.c_str());
  }
  const Rtc &r = g_rtc;
  const std::string src = std::string(source) + "\n#include \"mlf_user_rows.hpp\"\n";
  const std::string inc = std::string("-I") + include_dir;
  const std::string sums = "-DMLF_USER_NSUMS=" + std::to_string(nsums);
  // (a _SUMS variant adds its one option behind the others, and so does the derive program, which never calls the transform:
  // the other variants' programs are compiled as they were)
  const char *opts[10] = {"--offload-arch=gfx950", "-O3", "-std=c++17", "-ffp-contract=off", inc.c_str(),
                          has_transform && !v_derived ? "-DMLF_USER_HAS_TRANSFORM=1" : "-DMLF_USER_HAS_TRANSFORM=0",
                          v_gated ? "-DMLF_USER_TREGION=1" : "-DMLF_USER_TREGION=0",
                          v_summed ? "-DMLF_USER_SUM=1" : "-DMLF_USER_SUM=0", v_derived ? "-DMLF_USER_DERIVED=1" : sums.c_str()};
  int nopts = variant_multi(variant) || v_derived ? 9 : 8;
  if (v_gate_derived) opts[nopts++] = "-DMLF_USER_GATE_DERIVED=1";   // (behind whatever its gated sibling is compiled with)
  hiprtcProgram prog = nullptr;
  hiprtcResult res = r.create(&prog, src.c_str(), "mlf_user_model.hip", 0, nullptr, nullptr);
  if (res != HIPRTC_SUCCESS) {
    const std::string msg = std::string("hiprtcCreateProgram: ") + r.error_string(res);
    put_log(log, log_cap, msg);
    return fail_arg(MLF_E_COMPILE, msg.c_str());
  }
  res = r.compile(prog, nopts, opts);
  if (res != HIPRTC_SUCCESS) {
    std::string text = std::string("hiprtcCompileProgram: ") + r.error_string(res);
    size_t nlog = 0;
    if (r.log_size(prog, &nlog) == HIPRTC_SUCCESS && nlog > 1) {
      std::vector<char> buf(nlog + 1, '\0');
      if (r.log(prog, buf.data()) == HIPRTC_SUCCESS) text += "\n" + std::string(buf.data());
    }
    r.destroy(&prog);
    put_log(log, log_cap, text);
    return fail_arg(MLF_E_COMPILE, "the user model did not compile (hiprtc log in the caller's buffer)");
  }
  size_t size = 0;
  res = r.code_size(prog, &size);
  if (res != HIPRTC_SUCCESS || size == 0) {
    r.destroy(&prog);
    return fail_arg(MLF_E_COMPILE, "hiprtc returned no code object");
  }
  *code_size = size;
  int rc = 0;
  if (code_out) {
    if (code_cap < size) {
      rc = fail_arg(MLF_E_BADARG, "code buffer smaller than the code object (size in *code_size)");
    } else if (r.code(prog, static_cast<char *>(code_out)) != HIPRTC_SUCCESS) {
      rc = fail_arg(MLF_E_COMPILE, "hiprtcGetCode failed");
    }
  }
  r.destroy(&prog);
  return rc;
}

}  // namespace

extern "C" {

int mlf_usermodel_compile(const char *source, const char *include_dir, int has_transform, void *code_out, size_t code_cap,
                          size_t *code_size, char *log, size_t log_cap) {
  return mlf_usermodel_compile_variant(source, include_dir, has_transform, MLF_USERMODEL_DEFAULT, code_out, code_cap, code_size,
                                       log, log_cap);
}

int mlf_usermodel_compile_variant(const char *source, const char *include_dir, int has_transform, int variant, void *code_out,
                                  size_t code_cap, size_t *code_size, char *log, size_t log_cap) {
  if (!source || !include_dir || !code_size) return fail_arg(MLF_E_BADARG, "null pointer");
  if (variant_gate_derived(variant))
    return fail_arg(MLF_E_BADARG, "a _TREGION_DERIVED variant is compiled with mlf_usermodel_compile_gate_derived");
  if (variant_multi(variant))
    return fail_arg(MLF_E_BADARG, "a user-model variant with several sums needs their number: mlf_usermodel_compile_sums");
  if (variant != MLF_USERMODEL_DEFAULT && variant != MLF_USERMODEL_TREGION && variant != MLF_USERMODEL_SUM &&
      variant != MLF_USERMODEL_SUM_TREGION && variant != MLF_USERMODEL_DERIVED)
    return fail_arg(MLF_E_BADARG, "unknown user-model variant");
  return compile_program(source, include_dir, has_transform, variant, 0, code_out, code_cap, code_size, log, log_cap);
}

int mlf_usermodel_compile_sums(const char *source, const char *include_dir, int has_transform, int variant, int nsums,
                               void *code_out, size_t code_cap, size_t *code_size, char *log, size_t log_cap) {
  if (!source || !include_dir || !code_size) return fail_arg(MLF_E_BADARG, "null pointer");
  if (!variant_multi(variant) || variant_gate_derived(variant))
    return fail_arg(MLF_E_BADARG, "mlf_usermodel_compile_sums: the variant must be MLF_USERMODEL_SUMS or MLF_USERMODEL_SUMS_TREGION");
  if (nsums < 1 || nsums > MLF_USERMODEL_MAX_SUMS)
    return fail_arg(MLF_E_BADARG, "mlf_usermodel_compile_sums: nsums must be 1 to 8");
  return compile_program(source, include_dir, has_transform, variant, nsums, code_out, code_cap, code_size, log, log_cap);
}

int mlf_usermodel_compile_gate_derived(const char *source, const char *include_dir, int has_transform, int variant, int nsums,
                                       void *code_out, size_t code_cap, size_t *code_size, char *log, size_t log_cap) {
  if (!source || !include_dir || !code_size) return fail_arg(MLF_E_BADARG, "null pointer");
  if (!variant_gate_derived(variant))
    return fail_arg(MLF_E_BADARG, "mlf_usermodel_compile_gate_derived: the variant must be MLF_USERMODEL_TREGION_DERIVED, "
                                  "_SUM_TREGION_DERIVED or _SUMS_TREGION_DERIVED");
  if (variant_multi(variant) ? (nsums < 1 || nsums > MLF_USERMODEL_MAX_SUMS) : nsums != 0)
    return fail_arg(MLF_E_BADARG, "mlf_usermodel_compile_gate_derived: nsums must be 1 to 8 for _SUMS_TREGION_DERIVED, else 0");
  return compile_program(source, include_dir, has_transform, variant, nsums, code_out, code_cap, code_size, log, log_cap);
}

int mlf_usermodel_create(const void *code, size_t nbytes, size_t d, int has_transform, const double *aux, size_t naux,
                         mlf_usermodel **out) {
  return mlf_usermodel_create_variant(code, nbytes, d, has_transform, MLF_USERMODEL_DEFAULT, aux, naux, out);
}

int mlf_usermodel_create_variant(const void *code, size_t nbytes, size_t d, int has_transform, int variant, const double *aux,
                                 size_t naux, mlf_usermodel **out) {
  if (!out || !code || (naux && !aux)) return fail_arg(MLF_E_BADARG, "null pointer");
  *out = nullptr;
  if (variant_gate_derived(variant))
    return fail_arg(MLF_E_BADARG, "a _TREGION_DERIVED variant is loaded with mlf_usermodel_create_gate_derived");
  if (variant_summed(variant))
    return fail_arg(MLF_E_BADARG, "a summed user-model variant needs its number of terms: mlf_usermodel_create_sum");
  if (variant != MLF_USERMODEL_DEFAULT && variant != MLF_USERMODEL_TREGION)
    return fail_arg(MLF_E_BADARG, "unknown user-model variant");
  if (int rc = check_create_args(code, nbytes, d)) return rc;
  return load_model(code, d, has_transform, variant, 0, aux, naux, out);
}

int mlf_usermodel_create_sum(const void *code, size_t nbytes, size_t d, int has_transform, int variant, size_t nterms,
                             const double *aux, size_t naux, mlf_usermodel **out) {
  if (!out || !code || (naux && !aux)) return fail_arg(MLF_E_BADARG, "null pointer");
  *out = nullptr;
  if (!variant_summed(variant) || variant_gate_derived(variant))
    return fail_arg(MLF_E_BADARG, "mlf_usermodel_create_sum: the variant must be MLF_USERMODEL_SUM, _SUM_TREGION, _SUMS or _SUMS_TREGION");
  if (nterms == 0 || nterms > 0x7fffffffffffffffull) return fail_arg(MLF_E_BADARG, "a summed user model has at least one term");
  if (int rc = check_create_args(code, nbytes, d)) return rc;
  return load_model(code, d, has_transform, variant, nterms, aux, naux, out);
}

int mlf_usermodel_create_derived(const void *code, size_t nbytes, size_t d, size_t nderived, const double *aux, size_t naux,
                                 mlf_usermodel **out) {
  if (!out || !code || (naux && !aux)) return fail_arg(MLF_E_BADARG, "null pointer");
  *out = nullptr;
  if (nderived == 0) return fail_arg(MLF_E_BADARG, "a derive program has at least one derived parameter");
  if (int rc = check_create_args(code, nbytes, d)) return rc;
  if (nderived > MLF_MAX_DIM - d) return fail_arg(MLF_E_DIM, "user model: parameters and derived parameters above MLF_MAX_DIM");
  return load_model(code, d, 0, MLF_USERMODEL_DERIVED, 0, aux, naux, out, nderived);
}

int mlf_usermodel_create_gate_derived(const void *code, size_t nbytes, size_t d, int has_transform, int variant, size_t nterms,
                                      size_t nderived, const double *aux, size_t naux, mlf_usermodel **out) {
  if (!out || !code || (naux && !aux)) return fail_arg(MLF_E_BADARG, "null pointer");
  *out = nullptr;
  if (!variant_gate_derived(variant))
    return fail_arg(MLF_E_BADARG, "mlf_usermodel_create_gate_derived: the variant must be MLF_USERMODEL_TREGION_DERIVED, "
                                  "_SUM_TREGION_DERIVED or _SUMS_TREGION_DERIVED");
  if (nderived == 0) return fail_arg(MLF_E_BADARG, "a gate over derived parameters has at least one derived parameter");
  if (variant_summed(variant) ? (nterms == 0 || nterms > 0x7fffffffffffffffull) : nterms != 0)
    return fail_arg(MLF_E_BADARG, "nterms: at least one term for a summed variant, 0 for MLF_USERMODEL_TREGION_DERIVED");
  if (int rc = check_create_args(code, nbytes, d)) return rc;
  if (nderived > MLF_MAX_DIM - d) return fail_arg(MLF_E_DIM, "user model: parameters and derived parameters above MLF_MAX_DIM");
  return load_model(code, d, has_transform, variant, nterms, aux, naux, out, nderived);
}

int mlf_usermodel_gate_derived_lds_bytes(size_t d, size_t nderived, int has_p_buffer) {
  if (d == 0 || nderived == 0 || d > MLF_MAX_DIM || nderived > MLF_MAX_DIM) return 0;
  return (int)mlf_user_rows_gate_derived_lds_bytes((int)d, (int)nderived, has_p_buffer != 0);   // (at most MLF_USER_ROWS_LDS_BUDGET)
}

int mlf_usermodel_derive_lds_bytes(size_t d, size_t nderived) {
  if (d == 0 || nderived == 0 || d > MLF_MAX_DIM || nderived > MLF_MAX_DIM) return 0;
  return (int)mlf_user_rows_derive_lds_bytes((int)d, (int)nderived);   // (at most MLF_USER_ROWS_LDS_BUDGET)
}

int mlf_usermodel_destroy(mlf_usermodel *m) {
  if (!m) return 0;
  // the model's last launches may still be queued (the library's stream, or a caller's stream of eval_dev)
  hipError_t e = hipDeviceSynchronize();
  if (m->module) {
    const hipError_t e2 = hipModuleUnload(m->module);
    if (e == hipSuccess) e = e2;
  }
  m->aux.release();
  m->hu.release();
  m->hp.release();
  m->hL.release();
  delete m;
  if (e != hipSuccess) return fail_hip(e, "mlf_usermodel_destroy", "mlf_user.hip", __LINE__);
  return 0;
}

int mlf_usermodel_eval(mlf_usermodel *m, const double *u, size_t n, double *p_out, double *L_out) {
  if (!m || !u || (!p_out && !L_out)) return fail_arg(MLF_E_BADARG, "null pointer");
  if (m->nderived) return fail_arg(MLF_E_STATE, "a derive handle (mlf_usermodel_create_derived) evaluates nothing");
  if (n == 0) return 0;
  if (n > 0x7fffffffffffull / (size_t)m->d) return fail_arg(MLF_E_BADARG, "batch too large");
  hipStream_t s = ctx_stream();
  const size_t rows = n * (size_t)m->d * sizeof(double);
  CK(m->hu.reserve(rows));
  if (p_out) CK(m->hp.reserve(rows));
  if (L_out) CK(m->hL.reserve(n * sizeof(double)));
  CK(hipMemcpyAsync(m->hu.p, u, rows, hipMemcpyHostToDevice, s));
  if (int rc = usermodel_rows(m, m->hu.as<double>(), (long long)n, nullptr, p_out ? m->hp.as<double>() : nullptr,
                              L_out ? m->hL.as<double>() : nullptr, s))
    return rc;
  CK(hipGetLastError());
  if (p_out) CK(hipMemcpyAsync(p_out, m->hp.p, rows, hipMemcpyDeviceToHost, s));
  if (L_out) CK(hipMemcpyAsync(L_out, m->hL.p, n * sizeof(double), hipMemcpyDeviceToHost, s));
  CK(hipStreamSynchronize(s));
  return 0;
}

int mlf_usermodel_derive(mlf_usermodel *m, const double *p, size_t n, double *out) {
  if (!m) return fail_arg(MLF_E_BADARG, "null model");
  if (!m->nderived) return fail_arg(MLF_E_STATE, "not a derive handle (mlf_usermodel_create_derived)");
  if (n == 0) return 0;
  if (!p || !out) return fail_arg(MLF_E_BADARG, "null pointer");
  const size_t w = (size_t)m->d + (size_t)m->nderived;
  if (n > 0x7fffffffffffull / w) return fail_arg(MLF_E_BADARG, "batch too large");
  hipStream_t s = ctx_stream();
  const size_t in_bytes = n * (size_t)m->d * sizeof(double), out_bytes = n * w * sizeof(double);
  CK(m->hu.reserve(in_bytes));
  CK(m->hp.reserve(out_bytes));
  CK(hipMemcpyAsync(m->hu.p, p, in_bytes, hipMemcpyHostToDevice, s));
  if (int rc = usermodel_derive_rows(m, m->hu.as<double>(), (long long)n, m->hp.as<double>(), s)) return rc;
  CK(hipGetLastError());
  CK(hipMemcpyAsync(out, m->hp.p, out_bytes, hipMemcpyDeviceToHost, s));
  CK(hipStreamSynchronize(s));
  return 0;
}

int mlf_usermodel_derive_dev(mlf_usermodel *m, const double *d_p, size_t n, double *d_out, void *stream) {
  if (!m) return fail_arg(MLF_E_BADARG, "null model");
  if (!m->nderived) return fail_arg(MLF_E_STATE, "not a derive handle (mlf_usermodel_create_derived)");
  if (n == 0) return 0;
  if (!d_p || !d_out) return fail_arg(MLF_E_BADARG, "null pointer");
  if (int rc = usermodel_derive_rows(m, d_p, (long long)n, d_out, (hipStream_t)stream)) return rc;
  CK(hipGetLastError());
  return 0;
}

int mlf_usermodel_eval_dev(mlf_usermodel *m, const double *d_u, size_t n, const uint8_t *d_member, double *d_p, double *d_L,
                           void *stream) {
  if (!m) return fail_arg(MLF_E_BADARG, "null model");
  if (n == 0) return 0;
  if (!d_u || (!d_p && !d_L)) return fail_arg(MLF_E_BADARG, "null pointer");
  if (int rc = usermodel_rows(m, d_u, (long long)n, d_member, d_p, d_L, (hipStream_t)stream)) return rc;
  CK(hipGetLastError());
  return 0;
}

}  // extern "C"
