// mlf_sweep_dev.hpp -- what the sweeps of the MFMA pre-filter share: the vector types of the 32x32x16 binary16 matrix
// instruction's operands and results, and the running minimum of a lane over an accumulator block (k_sweep, k_sweep_min,
// k_prep_sweep, k_inside_mid; min3i also k_filter and k_wide_sweep).  Device code.
#pragma once
#include <hip/hip_runtime.h>

namespace mlf {

typedef float float16v __attribute__((ext_vector_type(16)));
typedef _Float16 half2v __attribute__((ext_vector_type(2)));
typedef _Float16 half8v __attribute__((ext_vector_type(8)));
typedef float float2v __attribute__((ext_vector_type(2)));

// Minimum of three MFMA results through their bit patterns (v_min3_i32): fminf() makes hipcc canonicalise every operand first
// (one extra v_max per value), and an inline-asm v_min3_f32 would read the MFMA result without the wait states the compiler
// only inserts for its own instructions.  Signed-integer order equals float order for values >= 0; a (tiny, rounding-induced)
// negative value has a negative pattern and so still wins the minimum, which is all the threshold tests need.
__device__ __forceinline__ int min3i(int a, int b, int c) {
  const int m = a < b ? a : b;
  return m < c ? m : c;
}

constexpr int kPosInf = 0x7f800000;   // +inf as a bit pattern: the start of a running minimum

// running minimum of a lane: its 16 values of this tile and what it had
__device__ __forceinline__ int tree_min(const float16v &c, int run) {
  const int m0 = min3i(__float_as_int(c[0]), __float_as_int(c[1]), __float_as_int(c[2]));
  const int m1 = min3i(__float_as_int(c[3]), __float_as_int(c[4]), __float_as_int(c[5]));
  const int m2 = min3i(__float_as_int(c[6]), __float_as_int(c[7]), __float_as_int(c[8]));
  const int m3 = min3i(__float_as_int(c[9]), __float_as_int(c[10]), __float_as_int(c[11]));
  const int m4 = min3i(__float_as_int(c[12]), __float_as_int(c[13]), __float_as_int(c[14]));
  return min3i(min3i(m0, m1, m2), min3i(m3, m4, __float_as_int(c[15])), run);
}

}  // namespace mlf
