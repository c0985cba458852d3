// The LayerNorm + residual epilogue of the fused fp32 GEMMs (gemm_ln_f32_dma.hip, gemm_ln_f32_split.hip): one definition, so the
// product in the main loop is the only numerical difference between the fp32-MFMA path and the exact-split path.
#pragma once
#include "common.h"

namespace pangu_ln {

// sum over the 8 lanes that share lane >> 3 (DPP quad_perm x2 + row_half_mirror), result in every lane
__device__ inline float oct_sum(float v) {
  v += __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, v), 0xB1, 0xF, 0xF, true));
  v += __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, v), 0x4E, 0xF, 0xF, true));
  v += __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, v), 0x141, 0xF, 0xF, true));
  return v;
}

// C[m0 .., 0 .. N) = shortcut + branch_scale * (LayerNorm(acc + bias) * gamma + beta) for a tile that spans the row: WMW x WNW
// waves of 64 x 96 (N = 96 WNW, wave = wm * WNW + wn), acc the wave's 2 x 3 accumulator tiles of the 32x32 MFMA (C/D layout:
// col = lane&31, row = (reg&3) + 8*(reg>>2) + 4*(lane>>5)).  smem is the main loop's ring, free behind the loop's last barrier.
// One 32-row group at a time: the wave's three 32x32 tiles go through its LDS patch and come back as row-major float4s
// (+ bias), per-row (sum, sum of squares) are reduced over the 8 lanes sharing a row with DPP adds, the WNW partial rows meet
// in a small LDS table behind one barrier, then normalise / gamma / beta / branch scale / shortcut and 16-B stores of whole 128-B
// row segments.
//
// Register budget of the fp32-MFMA caller (PIN_COL = true): 96 accumulator registers + the 128-VGPR cap of four workgroups per CU
// leave 32 for everything else, so the transposed rows of a 32-row group (48 registers) can only live in the registers its own
// accumulators free one 32 x 32 tile at a time, while the OTHER row group's 48 accumulators stay live: a few values go through
// scratch (round 3: 20-22 registers; round 4, with the column-block loop outermost and bias / gamma / beta re-loaded per (row
// group, column block) instead of hoisted, which the register barrier on `col` enforces: 8-15), all of it outside the MFMA loop.
// Measured alternative (round 4): two transposition passes (statistics, then normalise from the accumulators again) keep the
// accumulators live through both passes and spill 48-61.  The exact-split caller runs at 256 VGPRs, holds all of this in registers
// and passes PIN_COL = false: with the barrier its N = 192, K = 192 launch measures 1.4 % slower (the barrier changes no value,
// only where the compiler may move the column loads).
template <int WMW, int WNW, bool HAS_BIAS, bool PIN_COL>
__device__ __forceinline__ void ln_residual_epilogue(unsigned char* smem, const f32x16 (&acc)[2][3], const float* __restrict__ bias,
                                                     const float* __restrict__ shortcut, int lds_sc,
                                                     const float* __restrict__ gamma, const float* __restrict__ beta,
                                                     float* __restrict__ C, int ldc, int M, int m0, float branch_scale) {
  constexpr int NW = WMW * WNW;
  constexpr int BN = 96 * WNW;
  constexpr int EP_LD = 36;
  constexpr float INV_C = 1.0f / BN;
  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int wm = wave / WNW, wn = wave % WNW;
  const int lr = lane & 31, lh = lane >> 5;
  float* ep = reinterpret_cast<float*>(smem) + wave * (32 * EP_LD);
  float* stats = reinterpret_cast<float*>(smem) + NW * (32 * EP_LD);     // [WMW][WNW][64 rows][sum, sumsq]
  const int er = lane >> 3, ec = (lane & 7) * 4;
  const __amdgpu_buffer_rsrc_t c_rsrc = __builtin_amdgcn_make_buffer_rsrc(
      C, 0, (int)(((size_t)(M - 1) * ldc + BN) * sizeof(float)), 0x00020000);
  const __amdgpu_buffer_rsrc_t s_rsrc = __builtin_amdgcn_make_buffer_rsrc(
      const_cast<float*>(shortcut), 0, (int)(((size_t)(M - 1) * lds_sc + BN) * sizeof(float)), 0x00020000);
#pragma unroll
  for (int i = 0; i < 2; ++i) {
    f32x4 y[3][4];
    float s[4] = {0.f, 0.f, 0.f, 0.f}, q[4] = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int j = 0; j < 3; ++j) {
      int col = wn * 96 + j * 32 + ec;
      if (PIN_COL) asm volatile("" : "+v"(col));
      f32x4 bv = {0.f, 0.f, 0.f, 0.f};
      if (HAS_BIAS) bv = *reinterpret_cast<const f32x4*>(bias + col);
#pragma unroll
      for (int r = 0; r < 16; ++r) ep[((r & 3) + 8 * (r >> 2) + 4 * lh) * EP_LD + lr] = acc[i][j][r];
#pragma unroll
      for (int it = 0; it < 4; ++it) {
        f32x4 v = *reinterpret_cast<const f32x4*>(&ep[(er + 8 * it) * EP_LD + ec]);
        v += bv;
        y[j][it] = v;
        s[it] += (v[0] + v[1]) + (v[2] + v[3]);
        q[it] += (v[0] * v[0] + v[1] * v[1]) + (v[2] * v[2] + v[3] * v[3]);
      }
    }
#pragma unroll
    for (int it = 0; it < 4; ++it) {
      const float ss = oct_sum(s[it]), qq = oct_sum(q[it]);
      if ((lane & 7) == 0) {
        float* st = stats + (((wm * WNW + wn) * 64) + i * 32 + er + 8 * it) * 2;
        st[0] = ss;
        st[1] = qq;
      }
    }
    __syncthreads();
    float mean[4], rstd[4];
#pragma unroll
    for (int it = 0; it < 4; ++it) {
      const int rloc = i * 32 + er + 8 * it;
      float ts = 0.f, tq = 0.f;
#pragma unroll
      for (int w = 0; w < WNW; ++w) {
        const float* st = stats + ((wm * WNW + w) * 64 + rloc) * 2;
        ts += st[0];
        tq += st[1];
      }
      mean[it] = ts * INV_C;
      rstd[it] = rsqrtf(fmaxf(tq * INV_C - mean[it] * mean[it], 0.f) + LN_EPS);
    }
#pragma unroll
    for (int j = 0; j < 3; ++j) {
      int col = wn * 96 + j * 32 + ec;
      if (PIN_COL) asm volatile("" : "+v"(col));
      const f32x4 gm = *reinterpret_cast<const f32x4*>(gamma + col);
      const f32x4 bt = *reinterpret_cast<const f32x4*>(beta + col);
#pragma unroll
      for (int it = 0; it < 4; ++it) {
        // rows >= M fall outside the descriptors' range: the shortcut reads zeros and the store is dropped
        const unsigned row = (unsigned)(m0 + wm * 64 + i * 32 + er + 8 * it);
        const f32x4 sc = __builtin_bit_cast(
            f32x4, __builtin_amdgcn_raw_buffer_load_b128(s_rsrc, (int)((row * (unsigned)lds_sc + (unsigned)col) * 4u), 0, 0));
        const f32x4 v = sc + branch_scale * ((y[j][it] - mean[it]) * rstd[it] * gm + bt);
        __builtin_amdgcn_raw_buffer_store_b128(__builtin_bit_cast(u32x4, v), c_rsrc,
                                               (int)((row * (unsigned)ldc + (unsigned)col) * 4u), 0, 0);
      }
    }
  }
}

// The same epilogue for the row-owning tiling of the exact-split GEMM (split_f32.h, ROWS): WMW x WNW waves of 32 x 192 (N = 192
// WNW), acc the wave's 1 x 6 accumulator tiles.  A wave holds two of the row's 96-column groups, and the sums are formed as
// ln_residual_epilogue forms them, where one wave holds one group: per lane over the three column tiles of a group, oct_sum per
// group, then the groups in ascending column order from 0.f -- so the two tilings give the same bits.  The 2 WNW group sums meet
// in the LDS table behind one barrier.
template <int WMW, int WNW, bool HAS_BIAS>
__device__ __forceinline__ void ln_residual_epilogue_rows(unsigned char* smem, const f32x16 (&acc)[1][6],
                                                          const float* __restrict__ bias, const float* __restrict__ shortcut,
                                                          int lds_sc, const float* __restrict__ gamma,
                                                          const float* __restrict__ beta, float* __restrict__ C, int ldc, int M,
                                                          int m0, float branch_scale) {
  constexpr int NW = WMW * WNW;
  constexpr int BN = 192 * WNW;
  constexpr int NG = 2 * WNW;                      // 96-column groups of a row
  constexpr int EP_LD = 36;
  constexpr float INV_C = 1.0f / BN;
  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int wm = wave / WNW, wn = wave % WNW;
  const int lr = lane & 31, lh = lane >> 5;
  float* ep = reinterpret_cast<float*>(smem) + wave * (32 * EP_LD);
  float* stats = reinterpret_cast<float*>(smem) + NW * (32 * EP_LD);     // [WMW][NG][32 rows][sum, sumsq]
  const int er = lane >> 3, ec = (lane & 7) * 4;
  const __amdgpu_buffer_rsrc_t c_rsrc = __builtin_amdgcn_make_buffer_rsrc(
      C, 0, (int)(((size_t)(M - 1) * ldc + BN) * sizeof(float)), 0x00020000);
  const __amdgpu_buffer_rsrc_t s_rsrc = __builtin_amdgcn_make_buffer_rsrc(
      const_cast<float*>(shortcut), 0, (int)(((size_t)(M - 1) * lds_sc + BN) * sizeof(float)), 0x00020000);
  f32x4 y[6][4];
#pragma unroll
  for (int g = 0; g < 2; ++g) {
    float s[4] = {0.f, 0.f, 0.f, 0.f}, q[4] = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int jj = 0; jj < 3; ++jj) {
      const int j = 3 * g + jj;
      const int col = wn * 192 + j * 32 + ec;
      f32x4 bv = {0.f, 0.f, 0.f, 0.f};
      if (HAS_BIAS) bv = *reinterpret_cast<const f32x4*>(bias + col);
#pragma unroll
      for (int r = 0; r < 16; ++r) ep[((r & 3) + 8 * (r >> 2) + 4 * lh) * EP_LD + lr] = acc[0][j][r];
#pragma unroll
      for (int it = 0; it < 4; ++it) {
        f32x4 v = *reinterpret_cast<const f32x4*>(&ep[(er + 8 * it) * EP_LD + ec]);
        v += bv;
        y[j][it] = v;
        s[it] += (v[0] + v[1]) + (v[2] + v[3]);
        q[it] += (v[0] * v[0] + v[1] * v[1]) + (v[2] * v[2] + v[3] * v[3]);
      }
    }
#pragma unroll
    for (int it = 0; it < 4; ++it) {
      const float ss = oct_sum(s[it]), qq = oct_sum(q[it]);
      if ((lane & 7) == 0) {
        float* st = stats + ((wm * NG + 2 * wn + g) * 32 + er + 8 * it) * 2;
        st[0] = ss;
        st[1] = qq;
      }
    }
  }
  // A wave's own two group sums go through the table too, as (sum, sum of squares) pairs: which of the multiplies above the compiler
  // fuses into the adds (-ffp-contract) follows from how it pairs these stores, and a form that kept them in registers gave other
  // bits than ln_residual_epilogue.  tests/test_gpu_split_fingerprint.py holds the two against each other
  __syncthreads();
  float mean[4], rstd[4];
#pragma unroll
  for (int it = 0; it < 4; ++it) {
    float ts = 0.f, tq = 0.f;
#pragma unroll
    for (int g = 0; g < NG; ++g) {
      const float* st = stats + ((wm * NG + g) * 32 + er + 8 * it) * 2;
      ts += st[0];
      tq += st[1];
    }
    mean[it] = ts * INV_C;
    rstd[it] = rsqrtf(fmaxf(tq * INV_C - mean[it] * mean[it], 0.f) + LN_EPS);
  }
#pragma unroll
  for (int j = 0; j < 6; ++j) {
    const int col = wn * 192 + j * 32 + ec;
    const f32x4 gm = *reinterpret_cast<const f32x4*>(gamma + col);
    const f32x4 bt = *reinterpret_cast<const f32x4*>(beta + col);
#pragma unroll
    for (int it = 0; it < 4; ++it) {
      // rows >= M fall outside the descriptors' range: the shortcut reads zeros and the store is dropped
      const unsigned row = (unsigned)(m0 + wm * 32 + er + 8 * it);
      const f32x4 sc = __builtin_bit_cast(
          f32x4, __builtin_amdgcn_raw_buffer_load_b128(s_rsrc, (int)((row * (unsigned)lds_sc + (unsigned)col) * 4u), 0, 0));
      const f32x4 v = sc + branch_scale * ((y[j][it] - mean[it]) * rstd[it] * gm + bt);
      __builtin_amdgcn_raw_buffer_store_b128(__builtin_bit_cast(u32x4, v), c_rsrc,
                                             (int)((row * (unsigned)ldc + (unsigned)col) * 4u), 0, 0);
    }
  }
}

}  // namespace pangu_ln
