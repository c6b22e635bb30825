// mlf_user.hip -- user models (include/mlfriends_hip.h, section "user models"): a likelihood and prior transform written
// as HIP device functions, compiled at run time by hiprtc around mlf_user_rows.hpp (a covariance model: mlf_user_cov.hpp), loaded as a module on the library's
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
#define MLF_USER_COV_HOST
#include "mlf_user_cov.hpp"

using namespace mlf;

namespace {

// THE FORM TABLE: what each program form is, one row per number: the MLF_USERMODEL_* variants, and behind them the covariance pair,
// whose numbers only mlf_covmodel_compile / _create use (Form.variant of devicemodel.py).  Nothing else in the library tells the
// forms apart.
enum Shape {
  THREAD_PER_ROW,   // workgroups of one wave, one row per thread
  WAVE_PER_ROW,     // one wave (= one workgroup) per row: the summed forms, `long long nterms` behind the first eight parameters
  GROUP_PER_ROW,    // one workgroup of MLF_USER_COV_THREADS per row: the covariance form (mlf_user_cov.hpp), `double *tri` there
};
struct Variant {
  int number;
  const char *kernel;   // the only kernel of the variant's program (mlf_user_rows.hpp, mlf_user_cov.hpp)
  Shape shape;
  bool gated;           // the kernel takes the t-region gate's five parameters behind the others
  bool multi;           // several sums: their number is a constant of the program (-DMLF_USER_NSUMS)
  bool derive;          // p (n, d) -> [p | q] (n, d + nderived); such a handle runs in the derive entries only
  bool gate_derived;    // (gated is set too) the kernel computes nderived columns per member row, gates over d + nderived columns and
                        // takes (nq, q_scratch) behind the gate's five; such a handle runs in mlf_region_refill_user_derived_gated only
  const char *compile_entry, *create_entry;   // the exported entries that accept the variant
  unsigned (*lds_bytes)(int d, int nq, bool p_buffer);   // dynamic LDS of a launch (0: the kernel's direct form)

  constexpr bool summed() const { return shape == WAVE_PER_ROW; }
  constexpr bool cov() const { return shape == GROUP_PER_ROW; }
  constexpr unsigned threads() const { return cov() ? MLF_USER_COV_THREADS : 64; }   // per workgroup
  constexpr unsigned rows_per_group() const { return shape == THREAD_PER_ROW ? threads() : 1; }
};

unsigned lds_rows(int d, int, bool p_buffer) { return mlf_user_rows_lds_bytes(d, p_buffer); }
unsigned lds_sum(int d, int, bool p_buffer) { return mlf_user_rows_sum_lds_bytes(d, p_buffer); }
unsigned lds_derive(int d, int nq, bool) { return mlf_user_rows_derive_lds_bytes(d, nq); }
unsigned lds_gate_derived(int d, int nq, bool p_buffer) { return mlf_user_rows_gate_derived_lds_bytes(d, nq, p_buffer); }
unsigned lds_sum_gate_derived(int d, int nq, bool p_buffer) { return mlf_user_rows_sum_gate_derived_lds_bytes(d, nq, p_buffer); }

// the exported entries' names: an entry owns the variants whose row names it
constexpr char COMPILE_VARIANT[] = "mlf_usermodel_compile_variant", COMPILE_SUMS[] = "mlf_usermodel_compile_sums",
               COMPILE_GATE_DERIVED[] = "mlf_usermodel_compile_gate_derived", COMPILE_COV[] = "mlf_covmodel_compile",
               CREATE_VARIANT[] = "mlf_usermodel_create_variant", CREATE_SUM[] = "mlf_usermodel_create_sum",
               CREATE_DERIVED[] = "mlf_usermodel_create_derived", CREATE_GATE_DERIVED[] = "mlf_usermodel_create_gate_derived",
               CREATE_COV[] = "mlf_covmodel_create";
constexpr int COVMODEL = 16, COVMODEL_TREGION = 17;
constexpr Variant kVariants[] = {
    //                                                                                       gated  multi  derive gate_derived
    {MLF_USERMODEL_DEFAULT, "mlf_user_rows", THREAD_PER_ROW,                                 false, false, false, false, COMPILE_VARIANT, CREATE_VARIANT, lds_rows},
    {MLF_USERMODEL_TREGION, "mlf_user_rows_tregion", THREAD_PER_ROW,                         true,  false, false, false, COMPILE_VARIANT, CREATE_VARIANT, lds_rows},
    {MLF_USERMODEL_SUM, "mlf_user_rows_sum", WAVE_PER_ROW,                                   false, false, false, false, COMPILE_VARIANT, CREATE_SUM, lds_sum},
    {MLF_USERMODEL_SUM_TREGION, "mlf_user_rows_sum_tregion", WAVE_PER_ROW,                   true,  false, false, false, COMPILE_VARIANT, CREATE_SUM, lds_sum},
    {MLF_USERMODEL_SUMS, "mlf_user_rows_sums", WAVE_PER_ROW,                                 false, true,  false, false, COMPILE_SUMS, CREATE_SUM, lds_sum},
    {MLF_USERMODEL_SUMS_TREGION, "mlf_user_rows_sums_tregion", WAVE_PER_ROW,                 true,  true,  false, false, COMPILE_SUMS, CREATE_SUM, lds_sum},
    {MLF_USERMODEL_DERIVED, "mlf_user_derive_rows", THREAD_PER_ROW,                          false, false, true,  false, COMPILE_VARIANT, CREATE_DERIVED, lds_derive},
    {MLF_USERMODEL_TREGION_DERIVED, "mlf_user_rows_tregion_derived", THREAD_PER_ROW,         true,  false, false, true,  COMPILE_GATE_DERIVED, CREATE_GATE_DERIVED, lds_gate_derived},
    {MLF_USERMODEL_SUM_TREGION_DERIVED, "mlf_user_rows_sum_tregion_derived", WAVE_PER_ROW,   true,  false, false, true,  COMPILE_GATE_DERIVED, CREATE_GATE_DERIVED, lds_sum_gate_derived},
    {MLF_USERMODEL_SUMS_TREGION_DERIVED, "mlf_user_rows_sums_tregion_derived", WAVE_PER_ROW, true,  true,  false, true,  COMPILE_GATE_DERIVED, CREATE_GATE_DERIVED, lds_sum_gate_derived},
    {COVMODEL, "mlf_user_rows_cov", GROUP_PER_ROW,                                           false, false, false, false, COMPILE_COV, CREATE_COV, lds_sum},
    {COVMODEL_TREGION, "mlf_user_rows_cov_tregion", GROUP_PER_ROW,                           true,  false, false, false, COMPILE_COV, CREATE_COV, lds_sum},
};
constexpr int kLastPublicVariant = MLF_USERMODEL_SUMS_TREGION_DERIVED;   // the numbers above it are known to their own entries only

// what the entries bring besides the variant: each is 0 where its rule (check_counts) says so
struct Counts {
  int nsums = 0;         // of a variant with several sums (a compile entry's)
  int ncov = 0;          // of a covariance model: the order of its matrix (a constant of its program)
  size_t nterms = 0;     // of a summed variant (a create entry's)
  size_t nderived = 0;   // of the derive variant and the gate_derived ones (a create entry's)
};

}  // namespace

struct mlf_usermodel {
  hipModule_t module = nullptr;
  hipFunction_t fn = nullptr;
  const Variant *v = nullptr;
  int d = 0;
  bool has_transform = false;
  long long nterms = 0;   // of a summed variant
  int nderived = 0;       // of the derive variant and the gate_derived ones
  int ncov = 0;           // of a covariance model: the order of its matrix (a constant of its program)
  DevBuf htri;            // staging of mlf_covmodel_factor
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

// the model's kernel over n > 0 rows: the grid from the row's shape, its dynamic LDS (nderived is 0 in every row whose LDS does
// not depend on it), the launch
int launch_rows(const mlf_usermodel *m, long long n, bool p_buffer, void **args, hipStream_t s) {
  const Variant &v = *m->v;
  const long long blocks = (n + v.rows_per_group() - 1) / v.rows_per_group();
  if (blocks > 0x7fffffffLL) return fail_arg(MLF_E_BADARG, "user model: too many rows for one launch");
  const unsigned lds = v.lds_bytes(m->d, m->nderived, p_buffer);
  CK(hipModuleLaunchKernel(m->fn, (unsigned)blocks, 1, 1, v.threads(), 1, 1, lds, s, args, nullptr));
  return 0;
}

}  // namespace

namespace mlf {

int usermodel_dim(const mlf_usermodel *m) { return m->d; }
bool usermodel_has_transform(const mlf_usermodel *m) { return m->has_transform; }
bool usermodel_gated(const mlf_usermodel *m) { return m->v->gated; }
int usermodel_nderived(const mlf_usermodel *m) { return m->v->derive ? m->nderived : 0; }
int usermodel_gate_nderived(const mlf_usermodel *m) { return m->v->gate_derived ? m->nderived : 0; }

int usermodel_rows(const mlf_usermodel *m, const double *u, long long n, const uint8_t *member, double *p, double *L,
                   hipStream_t s, const TregionGate *gate, double *tri) {
  const Variant &v = *m->v;
  const int gate_nq = usermodel_gate_nderived(m);
  if (v.derive) return fail_arg(MLF_E_STATE, "a derive handle (mlf_usermodel_create_derived) evaluates nothing: it runs in the derive entries only");
  // the two variants differ in their parameter lists: never launch one with the other's
  if (v.gated != (gate != nullptr))
    return fail_arg(MLF_E_STATE, v.gated ? "user model loaded as the t-region variant: it runs only in a refill with a t-region set"
                                         : "user model not loaded as the t-region variant (mlf_usermodel_create_variant)");
  // a gate over derived columns is w = d + gate_nq wide and brings the q rows' scratch; every other gate is d wide
  if (gate_nq ? (gate->width != m->d + gate_nq || gate->q_scratch == nullptr) : (gate != nullptr && gate->width != 0))
    return fail_arg(MLF_E_STATE, gate_nq ? "user model loaded as a _TREGION_DERIVED variant: it runs only in "
                                           "mlf_region_refill_user_derived_gated, with a t-region over d + nderived columns"
                                         : "a t-region over d + nderived columns needs a user model loaded as a _TREGION_DERIVED "
                                           "variant (mlf_usermodel_create_gate_derived)");
  if (n <= 0) return 0;
  if (tri != nullptr && !v.cov()) return fail_arg(MLF_E_STATE, "not a covariance model (mlf_covmodel_create): it has no factor");
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
  int g_nq = gate_nq;
  double *g_scratch = gate ? gate->q_scratch : nullptr;
  // the first eight, nterms in the ninth place of a summed model (tri of a covariance model), the gate's five behind them when
  // gated, (nq, q_scratch) behind those in a _TREGION_DERIVED variant
  void *args[16] = {&a_u, &a_n, &a_d, &a_member, &a_aux, &a_naux, &a_p, &a_L};
  int na = 8;
  if (v.summed()) args[na++] = &a_nterms;
  double *a_tri = tri;
  if (v.cov()) args[na++] = &a_tri;
  if (gate) {
    void *g[] = {&g_A, &g_ctr, &g_fixed, &g_enlarge, &g_member2};
    for (void *x : g) args[na++] = x;
  }
  if (gate_nq) {
    args[na++] = &g_nq;
    args[na++] = &g_scratch;
  }
  return launch_rows(m, n, p != nullptr && m->has_transform, args, s);
}

int usermodel_derive_rows(const mlf_usermodel *m, const double *p, long long n, double *out, hipStream_t s) {
  if (!m->v->derive) return fail_arg(MLF_E_STATE, "not a derive handle (mlf_usermodel_create_derived)");
  if (n <= 0) return 0;
  // the kernel's parameters, in order and with its exact types (mlf_user_rows.hpp)
  const double *a_p = p;
  long long a_n = n;
  int a_d = m->d, a_nq = m->nderived;
  const double *a_aux = m->aux.as<double>();
  long long a_naux = m->naux;
  double *a_out = out;
  void *args[7] = {&a_p, &a_n, &a_d, &a_nq, &a_aux, &a_naux, &a_out};
  return launch_rows(m, n, false, args, s);
}

}  // namespace mlf

namespace {

// the row of `variant` where the exported entry `mine` (one of the names above) owns it; else NULL, and the message names the
// entry that does
const Variant *owned(int variant, const char *mine, const char *Variant::*owner) {
  const Variant *v = nullptr;
  for (const Variant &row : kVariants)
    if (row.number == variant) v = &row;
  if (v && v->*owner == mine) return v;
  if (!v || variant > kLastPublicVariant) {
    fail_arg(MLF_E_BADARG, "unknown user-model variant");
    return nullptr;
  }
  fail_arg(MLF_E_BADARG, (std::string(mine) + ": user-model variant " + std::to_string(variant) + " (entry " + v->kernel +
                          ") goes through " + v->*owner).c_str());
  return nullptr;
}

// the counts against the row, each rule once.  Both kinds of entry bring ncov; a compile entry the number of sums besides, a
// create entry the numbers of terms and of derived columns (the entries without one: 0).
int check_counts(const Variant &v, const Counts &c, bool compile) {
  if (v.cov() ? (c.ncov < 1 || c.ncov > 1024 || mlf_user_rows_cov_lds_bytes(c.ncov) > MLF_USER_COV_LDS_CAP) : c.ncov != 0)
    return fail_arg(MLF_E_BADARG, "ncov: the augmented triangle of an ncov x ncov covariance must fit the LDS of one CU "
                                  "(mlf_covmodel_lds_bytes(ncov) <= 163840)");
  if (compile) {
    if (v.multi ? (c.nsums < 1 || c.nsums > MLF_USERMODEL_MAX_SUMS) : c.nsums != 0)
      return fail_arg(MLF_E_BADARG, "nsums must be 1 to 8 for a variant with several sums (_SUMS), else 0");
    return 0;
  }
  const size_t nterms = c.nterms, nderived = c.nderived;
  if (v.summed() ? (nterms == 0 || nterms > 0x7fffffffffffffffull) : nterms != 0)
    return fail_arg(MLF_E_BADARG, "nterms: a summed user model has at least one term, every other variant 0");
  if ((v.derive || v.gate_derived) ? nderived == 0 : nderived != 0)
    return fail_arg(MLF_E_BADARG, "nderived: a derive program and a gate over derived parameters have at least one derived "
                                  "parameter, every other variant 0");
  return 0;
}

// the checks every create entry makes before it touches the device
int check_create_args(const void *code, size_t nbytes, size_t d, const Counts &c) {
  if (d == 0) return fail_arg(MLF_E_BADARG, "dimensionality must be positive");
  if (d > MLF_MAX_DIM) return fail_arg(MLF_E_DIM, "user model: dimensionality above MLF_MAX_DIM");
  if (nbytes < 64 || memcmp(code, "\x7f" "ELF", 4) != 0) return fail_arg(MLF_E_BADARG, "not a code object (ELF)");
  if (c.nderived > MLF_MAX_DIM - d) return fail_arg(MLF_E_DIM, "user model: parameters and derived parameters above MLF_MAX_DIM");
  if (c.ncov && (size_t)mlf_user_rows_cov_lds_bytes(c.ncov) + 2 * d * sizeof(double) > MLF_USER_COV_LDS_CAP)
    return fail_arg(MLF_E_BADARG, "ncov and d: the triangle and the row's u and p exceed the LDS of one CU");
  return 0;
}

// loads the code object as the variant `v` (arguments checked by the caller)
int load_model(const void *code, size_t d, int has_transform, const Variant &v, const Counts &c, const double *aux, size_t naux,
               mlf_usermodel **out) {
  if (int rc = ensure_ctx()) return rc;
  hipStream_t s = ctx_stream();
  mlf_usermodel *m = new mlf_usermodel();
  m->v = &v;
  m->d = (int)d;
  m->has_transform = has_transform != 0;
  m->nterms = (long long)c.nterms;
  m->nderived = (int)c.nderived;
  m->ncov = c.ncov;
  m->naux = (long long)naux;
  hipError_t e = hipModuleLoadData(&m->module, code);
  if (e == hipSuccess && hipModuleGetFunction(&m->fn, m->module, v.kernel) != hipSuccess) {
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

// hiprtc on `source` + the wrapper header as the variant `v` (counts checked by the caller); a covariance form compiles
// mlf_user_cov.hpp instead
int compile_program(const char *source, const char *include_dir, int has_transform, const Variant &v, const Counts &c,
                    void *code_out, size_t code_cap, size_t *code_size, char *log, size_t log_cap) {
  *code_size = 0;
  put_log(log, log_cap, "");
  std::lock_guard<std::mutex> lock(g_rtc_mutex);
  if (!rtc_load()) {
    put_log(log, log_cap, g_rtc.why);
    return fail_arg(MLF_E_COMPILE, g_rtc.why.c_str());
  }
  const Rtc &r = g_rtc;
  const std::string src = std::string(source) + (v.cov() ? "\n#include \"mlf_user_cov.hpp\"\n" : "\n#include \"mlf_user_rows.hpp\"\n");
  const std::string inc = std::string("-I") + include_dir;
  const std::string sums = "-DMLF_USER_NSUMS=" + std::to_string(c.nsums);
  const std::string cov = "-DMLF_USER_NCOV=" + std::to_string(c.ncov);
  // every program gets the first eight; a variant's own options follow (the derive program never calls the transform)
  const char *opts[12] = {"--offload-arch=gfx950", "-O3", "-std=c++17", "-ffp-contract=off", inc.c_str(),
                          has_transform && !v.derive ? "-DMLF_USER_HAS_TRANSFORM=1" : "-DMLF_USER_HAS_TRANSFORM=0",
                          v.gated ? "-DMLF_USER_TREGION=1" : "-DMLF_USER_TREGION=0",
                          v.summed() ? "-DMLF_USER_SUM=1" : "-DMLF_USER_SUM=0"};
  int nopts = 8;
  if (v.multi) opts[nopts++] = sums.c_str();
  if (v.derive) opts[nopts++] = "-DMLF_USER_DERIVED=1";
  if (v.gate_derived) opts[nopts++] = "-DMLF_USER_GATE_DERIVED=1";
  if (v.cov()) opts[nopts++] = cov.c_str();
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

// every exported compile entry: the pointers, "is this variant mine", the counts, one compile
int compile_entry(const char *mine, const char *source, const char *include_dir, int has_transform, int variant, const Counts &c,
                  void *code_out, size_t code_cap, size_t *code_size, char *log, size_t log_cap) {
  if (!source || !include_dir || !code_size) return fail_arg(MLF_E_BADARG, "null pointer");
  const Variant *v = owned(variant, mine, &Variant::compile_entry);
  if (!v) return MLF_E_BADARG;
  if (int rc = check_counts(*v, c, true)) return rc;
  return compile_program(source, include_dir, has_transform, *v, c, code_out, code_cap, code_size, log, log_cap);
}

// every exported create entry: the pointers, "is this variant mine", the counts, d and the code object, one load
int create_entry(const char *mine, const void *code, size_t nbytes, size_t d, int has_transform, int variant, const Counts &c,
                 const double *aux, size_t naux, mlf_usermodel **out) {
  if (!out || !code || (naux && !aux)) return fail_arg(MLF_E_BADARG, "null pointer");
  *out = nullptr;
  const Variant *v = owned(variant, mine, &Variant::create_entry);
  if (!v) return MLF_E_BADARG;
  if (int rc = check_counts(*v, c, false)) return rc;
  if (int rc = check_create_args(code, nbytes, d, c)) return rc;
  return load_model(code, d, has_transform, *v, c, aux, naux, out);
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
  return compile_entry(COMPILE_VARIANT, source, include_dir, has_transform, variant, Counts{}, code_out, code_cap, code_size, log, log_cap);
}

int mlf_usermodel_compile_sums(const char *source, const char *include_dir, int has_transform, int variant, int nsums,
                               void *code_out, size_t code_cap, size_t *code_size, char *log, size_t log_cap) {
  return compile_entry(COMPILE_SUMS, source, include_dir, has_transform, variant, Counts{nsums}, code_out, code_cap, code_size, log, log_cap);
}

int mlf_usermodel_compile_gate_derived(const char *source, const char *include_dir, int has_transform, int variant, int nsums,
                                       void *code_out, size_t code_cap, size_t *code_size, char *log, size_t log_cap) {
  return compile_entry(COMPILE_GATE_DERIVED, source, include_dir, has_transform, variant, Counts{nsums}, code_out, code_cap, code_size, log,
                       log_cap);
}

int mlf_usermodel_create(const void *code, size_t nbytes, size_t d, int has_transform, const double *aux, size_t naux,
                         mlf_usermodel **out) {
  return mlf_usermodel_create_variant(code, nbytes, d, has_transform, MLF_USERMODEL_DEFAULT, aux, naux, out);
}

int mlf_usermodel_create_variant(const void *code, size_t nbytes, size_t d, int has_transform, int variant, const double *aux,
                                 size_t naux, mlf_usermodel **out) {
  return create_entry(CREATE_VARIANT, code, nbytes, d, has_transform, variant, Counts{}, aux, naux, out);
}

int mlf_usermodel_create_sum(const void *code, size_t nbytes, size_t d, int has_transform, int variant, size_t nterms,
                             const double *aux, size_t naux, mlf_usermodel **out) {
  return create_entry(CREATE_SUM, code, nbytes, d, has_transform, variant, Counts{0, 0, nterms}, aux, naux, out);
}

int mlf_usermodel_create_derived(const void *code, size_t nbytes, size_t d, size_t nderived, const double *aux, size_t naux,
                                 mlf_usermodel **out) {
  return create_entry(CREATE_DERIVED, code, nbytes, d, 0, MLF_USERMODEL_DERIVED, Counts{0, 0, 0, nderived}, aux, naux, out);
}

int mlf_usermodel_create_gate_derived(const void *code, size_t nbytes, size_t d, int has_transform, int variant, size_t nterms,
                                      size_t nderived, const double *aux, size_t naux, mlf_usermodel **out) {
  return create_entry(CREATE_GATE_DERIVED, code, nbytes, d, has_transform, variant, Counts{0, 0, nterms, nderived}, aux, naux, out);
}

int mlf_usermodel_gate_derived_lds_bytes(size_t d, size_t nderived, int has_p_buffer) {
  if (d == 0 || nderived == 0 || d > MLF_MAX_DIM || nderived > MLF_MAX_DIM) return 0;
  return (int)mlf_user_rows_gate_derived_lds_bytes((int)d, (int)nderived, has_p_buffer != 0);   // (at most MLF_USER_ROWS_LDS_BUDGET)
}

int mlf_usermodel_derive_lds_bytes(size_t d, size_t nderived) {
  if (d == 0 || nderived == 0 || d > MLF_MAX_DIM || nderived > MLF_MAX_DIM) return 0;
  return (int)mlf_user_rows_derive_lds_bytes((int)d, (int)nderived);   // (at most MLF_USER_ROWS_LDS_BUDGET)
}

int mlf_covmodel_lds_bytes(int ncov) {
  // (0: no such program.  The bound keeps the arithmetic below in range; the Python constructor holds static + dynamic to the CU's)
  if (ncov < 1 || ncov > 1024) return 0;
  return (int)mlf_user_rows_cov_lds_bytes(ncov);
}

int mlf_covmodel_compile(const char *source, const char *include_dir, int has_transform, int gated, int ncov, void *code_out,
                         size_t code_cap, size_t *code_size, char *log, size_t log_cap) {
  return compile_entry(COMPILE_COV, source, include_dir, has_transform, gated ? COVMODEL_TREGION : COVMODEL, Counts{0, ncov},
                       code_out, code_cap, code_size, log, log_cap);
}

int mlf_covmodel_create(const void *code, size_t nbytes, size_t d, int has_transform, int gated, int ncov, const double *aux,
                        size_t naux, mlf_usermodel **out) {
  if (int rc = create_entry(CREATE_COV, code, nbytes, d, has_transform, gated ? COVMODEL_TREGION : COVMODEL, Counts{0, ncov}, aux,
                            naux, out))
    return rc;
  // ncov sizes the factor rows of mlf_covmodel_factor: it must be the program's own constant, which the kernel's static LDS names
  // (mlf_user_rows_cov_lds_bytes grows strictly with n)
  int shared = 0;
  const hipError_t e = hipFuncGetAttribute(&shared, HIP_FUNC_ATTRIBUTE_SHARED_SIZE_BYTES, (*out)->fn);
  if (e != hipSuccess || shared != (int)mlf_user_rows_cov_lds_bytes(ncov)) {
    (void)hipGetLastError();
    (void)mlf_usermodel_destroy(*out);
    *out = nullptr;
    if (e != hipSuccess) return fail_hip(e, "mlf_covmodel_create", "mlf_user.hip", __LINE__);
    return fail_arg(MLF_E_BADARG, "ncov is not the ncov the code object was compiled with");
  }
  return 0;
}

int mlf_covmodel_factor(mlf_usermodel *m, const double *u, size_t n, double *tri_out, double *L_out) {
  if (!m || !u || !tri_out || !L_out) return fail_arg(MLF_E_BADARG, "null pointer");
  if (!m->v->cov()) return fail_arg(MLF_E_STATE, "not a covariance model (mlf_covmodel_create): it has no factor");
  if (m->v->gated) return fail_arg(MLF_E_STATE, "the gated program of a covariance model runs in a refill with a t-region only");
  if (n == 0) return 0;
  const size_t tri_doubles = mlf_user_rows_cov_tri_doubles(m->ncov);
  if (n > 0x7fffffffull || n > 0x7fffffffffffull / (tri_doubles + (size_t)m->d)) return fail_arg(MLF_E_BADARG, "batch too large");
  hipStream_t s = ctx_stream();
  const size_t rows = n * (size_t)m->d * sizeof(double), tri_bytes = n * tri_doubles * sizeof(double);
  CK(m->hu.reserve(rows));
  if (m->has_transform) CK(m->hp.reserve(rows));
  CK(m->hL.reserve(n * sizeof(double)));
  CK(m->htri.reserve(tri_bytes));
  CK(hipMemcpyAsync(m->hu.p, u, rows, hipMemcpyHostToDevice, s));
  // (with a transform the rows are cube rows and p its output; without one they are the parameters)
  if (int rc = usermodel_rows(m, m->hu.as<double>(), (long long)n, nullptr, m->has_transform ? m->hp.as<double>() : nullptr,
                              m->hL.as<double>(), s, nullptr, m->htri.as<double>()))
    return rc;
  CK(hipGetLastError());
  CK(hipMemcpyAsync(tri_out, m->htri.p, tri_bytes, hipMemcpyDeviceToHost, s));
  CK(hipMemcpyAsync(L_out, m->hL.p, n * sizeof(double), hipMemcpyDeviceToHost, s));
  CK(hipStreamSynchronize(s));
  return 0;
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
  m->htri.release();
  delete m;
  if (e != hipSuccess) return fail_hip(e, "mlf_usermodel_destroy", "mlf_user.hip", __LINE__);
  return 0;
}

int mlf_usermodel_eval(mlf_usermodel *m, const double *u, size_t n, double *p_out, double *L_out) {
  if (!m || !u || (!p_out && !L_out)) return fail_arg(MLF_E_BADARG, "null pointer");
  if (m->v->derive) return fail_arg(MLF_E_STATE, "a derive handle (mlf_usermodel_create_derived) evaluates nothing");
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
  if (!m->v->derive) return fail_arg(MLF_E_STATE, "not a derive handle (mlf_usermodel_create_derived)");
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
  if (!m->v->derive) return fail_arg(MLF_E_STATE, "not a derive handle (mlf_usermodel_create_derived)");
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
