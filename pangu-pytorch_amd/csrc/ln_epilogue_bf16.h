// The LayerNorm + residual epilogue pieces of the fused bf16 GEMMs (both kernels of gemm_ln_bf16.hip), one definition each, for the
// swapped-operand MFMA layout: a workgroup of WM x WNW waves with wave tiles of 64 x 96 spans the whole row (N = 96 WNW,
// wave = wm * WNW + wn), and lane (lg, lc) of acc[i][j] holds y[m = wm*64 + 16i + lc][n = wn*96 + 16j + 4lg + r], r = 0..3, bias
// included.  The statistics are taken on the fp32 accumulators, i.e. BEFORE the bf16 rounding the unfused path applies to y.
// What differs between the callers stays with them: the barriers around the statistics table (a __syncthreads in the
// register-staged kernel, two raw barriers in the persistent one, which must not wait for its operand requests in flight) and where
// gamma / beta come from (global memory / the LDS-resident parameter vectors).
#pragma once
#include "gemm_bf16_loop.h"

namespace pangu_bf16 {

// Per-row (sum, sum of squares) of this wave's 96 columns, in fp32 straight from the accumulators (in-lane + 2 shuffles), into the
// workgroup's table stats[WM][WNW][64 rows][sum, sumsq]; the caller's barrier follows.
template <int WNW>
__device__ __forceinline__ void ln_stats_partials(const f32x4 (&acc)[4][6], float* stats, int wm, int wn, int lc, int lg) {
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    float s = 0.f, q = 0.f;
#pragma unroll
    for (int j = 0; j < 6; ++j)
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        s += acc[i][j][r];
        q = fmaf(acc[i][j][r], acc[i][j][r], q);
      }
    s += __shfl_xor(s, 16, 64);
    q += __shfl_xor(q, 16, 64);
    s += __shfl_xor(s, 32, 64);
    q += __shfl_xor(q, 32, 64);
    if (lg == 0) {
      float* st = stats + (((wm * WNW + wn) * 64) + i * 16 + lc) * 2;
      st[0] = s;
      st[1] = q;
    }
  }
}

// mean and 1 / std of row 16i + lc of wave row wm: the WNW partials of the row, combined in wave order
template <int WNW>
__device__ __forceinline__ void ln_row_stats(const float* stats, int wm, int i, int lc, float& mean, float& rstd) {
  constexpr float INV_C = 1.0f / (96 * WNW);
  float s = 0.f, q = 0.f;
#pragma unroll
  for (int w = 0; w < WNW; ++w) {
    const float* st = stats + (((wm * WNW + w) * 64) + i * 16 + lc) * 2;
    s += st[0];
    q += st[1];
  }
  mean = s * INV_C;
  rstd = rsqrtf(fmaxf(q * INV_C - mean * mean, 0.f) + LN_EPS);
}

// One accumulator quad: shortcut (four bf16, as they lie in the patch slot) + LayerNorm(y) * gamma + beta, packed for the slot
__device__ __forceinline__ u32x2 ln_residual_pack(f32x4 y, float mean, float rstd, f32x4 gamma, f32x4 beta, u32x2 shortcut) {
  f32x4 v = (y - mean) * rstd * gamma + beta;
  v += unpack_bf16x4(shortcut);
  return pack_bf16x4(v);
}

}  // namespace pangu_bf16
