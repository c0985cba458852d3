// What the plane kernels of the output side (pack.hip, regrid.hip) share: the de-normalising value and the level reversal, both
// folded into the pass that reads the field.
#pragma once
#include "common.h"

// v = x * mul + add in two roundings, rollout.norm_back's arithmetic.  hipcc contracts a product and a sum into one v_fma_f32 by
// default (even __fadd_rn(__fmul_rn(..))): contraction is switched off for these two operations.
template <bool AFFINE>
__device__ __forceinline__ float pk_value(float x, float m, float a) {
#pragma clang fp contract(off)
  if (!AFFINE) return x;
  const float p = x * m;
  return p + a;
}

// output plane -> source plane: with `levels` = L the level index inside each variable is reversed
__device__ __forceinline__ int pk_src_plane(int p, int levels) {
  if (levels <= 1) return p;
  const int v = p / levels, l = p - v * levels;
  return v * levels + (levels - 1 - l);
}
