// The fp32-MFMA LDS-DMA main loop of gemm_f32_dma.hip and gemm_ln_f32_dma.hip (one definition: the two differ in their epilogues
// only), and the swizzled 64-byte-row fp32 LDS image it shares with the exact-split kernels (split_f32.h).
#pragma once
#include "common.h"

namespace pangu_dma {

constexpr int BM = 128;      // rows of the output tile: 2 wave rows of 64
constexpr int BK = 16;       // floats per K-step = one 64-byte LDS row

// 2 x WNW waves of 64 x 32 TN: a 128 x 32 TN WNW tile, a ring of two stages of (BM + BN) 64-byte rows
template <int WNW, int TN>
struct DmaTile {
  static constexpr int NW = 2 * WNW;           // waves
  static constexpr int BN = 32 * TN * WNW;
  static constexpr int ROWS = BM + BN;
  static constexpr int STAGE = ROWS * 64;      // bytes per ring slot
  static constexpr int LPS = ROWS / 16 / NW;   // LDS-DMA instructions per wave and stage (16 rows of 64 B each)
  static constexpr int SMEM = 2 * STAGE;
  static_assert(ROWS % (16 * NW) == 0, "every wave issues the same number of pieces");
};

// acc[i][j] += A[m0 + wm 64 + i 32 .. +31, :] @ W[n0 + wn 32 TN + j 32 .. +31, :]^T over all of K (K % 16 == 0), exact-f32
// v_mfma_f32_32x32x2_f32 on permuted-k b128 fragments.  The operands travel L2 -> LDS by LDS-DMA into smem (DmaTile::SMEM
// bytes), one k-step ahead.  wave = wm * WNW + wn is the caller's uniform wave index, handed in and not derived again: with a
// second readfirstlane of its own the loop costs gemm_tn_f32_dma_kernel<2, ADD, bias> a register, which it spills.  Ends behind a
// barrier: every wave is done with the ring, the caller's epilogue may reuse it.
template <int WNW, int TN>
__device__ __forceinline__ void dma_main_loop(unsigned char* smem, const float* __restrict__ A, int lda,
                                              const float* __restrict__ W, int M, int N, int K, int m0, int n0, int wave,
                                              f32x16 (&acc)[2][TN]) {
  using T = DmaTile<WNW, TN>;
  constexpr int NW = T::NW, STAGE = T::STAGE, LPS = T::LPS;
  const int tid = threadIdx.x, lane = tid & 63;
  const int wm = wave / WNW, wn = wave % WNW;
  const int lr = lane & 31, lh = lane >> 5;

  const __amdgpu_buffer_rsrc_t a_rsrc = __builtin_amdgcn_make_buffer_rsrc(
      const_cast<float*>(A), 0, (int)(((size_t)(M - 1) * lda + K) * sizeof(float)), 0x00020000);
  const __amdgpu_buffer_rsrc_t w_rsrc = __builtin_amdgcn_make_buffer_rsrc(
      const_cast<float*>(W), 0, (int)((size_t)N * K * sizeof(float)), 0x00020000);
  // DMA instruction q = i*NW + wave (i < LPS) fills rows 16q .. 16q+15 (1 KB): this lane fills (row 16q + lane>>2, physical
  // chunk lane&3) and therefore fetches logical chunk (lane&3) ^ F(row).  Rows >= M / >= N are out of range: zeros.
  unsigned voff[LPS];
#pragma unroll
  for (int i = 0; i < LPS; ++i) {
    const int row = 16 * (i * NW + wave) + (lane >> 2);
    const int f = (0x78 >> (((row >> 2) & 3) * 2)) & 3;
    const int c = (lane & 3) ^ f;
    voff[i] = row < BM ? ((unsigned)(m0 + row) * (unsigned)lda + c * 4) * 4u
                       : ((unsigned)(n0 + row - BM) * (unsigned)K + c * 4) * 4u;
  }
  auto issue = [&](int kt) {
    unsigned char* base = smem + (kt & 1) * STAGE;
#pragma unroll
    for (int i = 0; i < LPS; ++i) {
      const int q = i * NW + wave;
      auto dst = (__attribute__((address_space(3))) void*)(base + q * 1024);
      if (16 * q < BM) __builtin_amdgcn_raw_ptr_buffer_load_lds(a_rsrc, dst, 16, (int)voff[i], kt * BK * 4, 0, 0);
      else __builtin_amdgcn_raw_ptr_buffer_load_lds(w_rsrc, dst, 16, (int)voff[i], kt * BK * 4, 0, 0);
    }
  };

#pragma unroll
  for (int i = 0; i < 2; ++i)
#pragma unroll
    for (int j = 0; j < TN; ++j)
#pragma unroll
      for (int r = 0; r < 16; ++r) acc[i][j][r] = 0.f;

  // fragment byte offsets: lane (lr, lh) owns k = 8lh .. 8lh+7 of row (.. + lr): logical chunks 2lh (half 0), 2lh+1 (half 1)
  int off_a[2][2], off_w[TN][2];
#pragma unroll
  for (int h = 0; h < 2; ++h) {
#pragma unroll
    for (int i = 0; i < 2; ++i) off_a[i][h] = kswz64(wm * 64 + i * 32 + lr, 2 * lh + h);
#pragma unroll
    for (int j = 0; j < TN; ++j) off_w[j][h] = BM * 64 + kswz64(wn * 32 * TN + j * 32 + lr, 2 * lh + h);
  }

  const int KT = K / BK;
  issue(0);
  for (int kt = 0; kt < KT; ++kt) {
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");       // this wave's part of step kt has landed
    __builtin_amdgcn_s_barrier();                          // ... and everybody's; slot (kt+1)&1 is free
    asm volatile("" ::: "memory");
    if (kt + 1 < KT) issue(kt + 1);
    const unsigned char* St = smem + (kt & 1) * STAGE;
#pragma unroll
    for (int h = 0; h < 2; ++h) {                           // the two k-halves share the fragment registers
      f32x4 fa[2], fw[TN];
#pragma unroll
      for (int i = 0; i < 2; ++i) fa[i] = *reinterpret_cast<const f32x4*>(St + off_a[i][h]);
#pragma unroll
      for (int j = 0; j < TN; ++j) fw[j] = *reinterpret_cast<const f32x4*>(St + off_w[j][h]);
#pragma unroll
      for (int s = 0; s < 4; ++s)
#pragma unroll
        for (int i = 0; i < 2; ++i)
#pragma unroll
          for (int j = 0; j < TN; ++j)
            acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x2f32(fa[i][s], fw[j][s], acc[i][j], 0, 0, 0);
    }
  }
  __syncthreads();
}

}  // namespace pangu_dma
