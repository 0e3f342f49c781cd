// K5 — the f16 hi + lo split of the top-k scores (scheme in topk.hip's opening comment): the
// scale exponent and the split of one scaled value.  V's preparation kernels (topk_prep.h)
// split the table with them, the sweep kernels (topk_sweep.h) the query rows.
#pragma once
#include "als_common.h"

namespace als {

typedef float floatx4 __attribute__((ext_vector_type(4)));

namespace {

typedef _Float16 tk_half8 __attribute__((ext_vector_type(8)));

// Power-of-two scale exponent: the largest |t| of the operand lands in [2^14, 2^15).
__device__ __forceinline__ int tk_split_exponent(float m) {
  if (!(m > 0.f) || !(m < 3.0e38f)) return 0;
  int e = 14 - ilogbf(m);
  return e < -60 ? -60 : (e > 60 ? 60 : e);
}

__device__ __forceinline__ void tk_split(float t, _Float16& hi, _Float16& lo) {
  hi = (_Float16)t;  // round to nearest
  lo = (_Float16)(t - (float)hi);
}

}  // namespace

}  // namespace als
