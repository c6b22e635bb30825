// mlf_ctx.hpp -- what every C-ABI translation unit shares: the grow-only device buffer, the library
// context (one device, one stream) and error reporting.  mlf_host.hpp adds what the membership / region units share.
#pragma once
#include <hip/hip_runtime.h>

#include <cstddef>
#include <cstdint>

struct mlf_usermodel;   // include/mlfriends_hip.h

namespace mlf {

// grow-only device buffer
struct DevBuf {
  void *p = nullptr;
  size_t cap = 0;
  hipError_t reserve(size_t bytes) {
    if (bytes <= cap) return hipSuccess;
    if (p) {
      hipError_t e = hipFree(p);
      p = nullptr;
      cap = 0;
      if (e != hipSuccess) return e;
    }
    // grow by half and in 64 KiB steps: scratch buffers shared by calls of slightly different sizes would otherwise be
    // freed and re-allocated (hipFree synchronises the device) every time a new maximum comes along
    const size_t want = (bytes + bytes / 2 + 65535) / 65536 * 65536;
    hipError_t e = hipMalloc(&p, want);
    if (e != hipSuccess) return e;
    cap = want;
    return hipSuccess;
  }
  template <class T>
  T *as() const { return static_cast<T *>(p); }
  void release() {
    if (p) (void)hipFree(p);
    p = nullptr;
    cap = 0;
  }
};

// defined in mlf_api.hip; the fail_* set the text that mlf_last_error returns
int ensure_ctx();                    // 0 or MLF_E_NODEVICE (message set)
hipStream_t ctx_stream();
int fail_hip(hipError_t e, const char *what, const char *file, int line);   // "HIP error N (text) at FILE:LINE: call"; returns -(int)e
int fail_arg(int code, const char *msg);                                    // returns code

// defined in mlf_user.hip: a user model's dimensionality / transform flag, and one launch of its mlf_user_rows kernel on `s`
// (argument meaning as in mlf_user_rows.hpp)
int usermodel_dim(const mlf_usermodel *m);
bool usermodel_has_transform(const mlf_usermodel *m);
// the parameter-space wrapping ellipsoid of a gated launch (mlf_tregion_dev.hpp): dense d x d matrix, centre, fixed values (NaN =
// variable dimension), all on the device; member2[i] = member[i] && inside(p_i) is written for every row
struct TregionGate {
  const double *A, *ctr, *fixed_val;
  double enlarge;
  uint8_t *member2;
  // a gate over parameters AND derived parameters (the _TREGION_DERIVED variants): the width w = d + nderived of matrix, centre
  // and fixed values (0: the model's d), and n rows of nderived doubles for the direct form's q rows
  int width = 0;
  double *q_scratch = nullptr;
};
bool usermodel_gated(const mlf_usermodel *m);   // loaded as the MLF_USERMODEL_TREGION variant: launches with a gate only
int usermodel_rows(const mlf_usermodel *m, const double *u, long long n, const uint8_t *member, double *p, double *L,
                   hipStream_t s, const TregionGate *gate = nullptr, double *tri = nullptr);
// (tri: a covariance model's rows of augmented factors, mlf_user_cov.hpp; NULL on every route, set by mlf_covmodel_factor alone)
// a derive handle (MLF_USERMODEL_DERIVED): its number of derived columns (0 for every other handle) and one launch of its
// mlf_user_derive_rows kernel on `s`: p (n, d) -> out (n, d + nderived), which must not overlap
int usermodel_nderived(const mlf_usermodel *m);
// a handle of a _TREGION_DERIVED variant: the number of derived columns its gate spans (0 for every other handle); it launches only
// with a gate of width d + that number and a q_scratch
int usermodel_gate_nderived(const mlf_usermodel *m);
int usermodel_derive_rows(const mlf_usermodel *m, const double *p, long long n, double *out, hipStream_t s);

}  // namespace mlf

// a failed HIP call ends the calling function with fail_hip's code
#define CK(x)                                                                    \
  do {                                                                           \
    hipError_t e_ = (x);                                                         \
    if (e_ != hipSuccess) return mlf::fail_hip(e_, #x, __FILE_NAME__, __LINE__); \
  } while (0)
