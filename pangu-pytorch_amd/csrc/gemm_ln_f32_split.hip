// fp32 projection GEMM + post-norm residual in one launch on the bf16 matrix pipe (inference path):
//   out[M,N] = shortcut + branch_scale * (LayerNorm(A[M,K] @ W[N,K]^T + bias) * gamma + beta)           (layers.py:250-251)
// for N = 192 and N = 384, W given as its exact-split image (pangu_split_weight_bf16x3).  The main loop is split_main_loop of
// split_f32.h, the one gemm_f32_split.hip runs; the epilogue is ln_residual_epilogue of ln_epilogue_f32.h, the one
// gemm_ln_f32_dma.hip runs, so the product is the only numerical difference between the two fused kernels.
//
//   N = 192: 128 x 192 tile, 2 x 2 waves of 64 x 96, ring of three 26-KB stages = 78 KB, two workgroups per CU.
//   N = 384: the tile spans the row (the LayerNorm statistics stay in the workgroup), its W part is the image's two 192-row
//            n-tile blocks of the k-step, 36 KB: 64 x 384 tile, 1 x 4 waves of 64 x 96 or (K >= 1536) 2 x 2 row-owning waves of
//            32 x 192 (every A row split by one wave, not by four), ring of two 40-KB stages (LDS-DMA one k-step ahead)
//            = 80 KB, two workgroups per CU, so one workgroup's main loop covers the other's epilogue.  The measured alternative,
//            128 x 384 with 2 x 4 waves and three 44-KB stages (<2, 4, 3>: 132 KB, one workgroup per CU), is 7 % slower at
//            K = 384 and at K = 1536 (profiles/f32_split_ln_per_shape.md) and is not instantiated.
// Either way 2 waves per SIMD: 256 VGPRs, so the 96 accumulators and the transposed row registers of the epilogue (48 of a 64 x 96
// wave's row group, 96 of a row-owning wave) are live together without scratch (the fp32-MFMA kernel's 128-VGPR cap is gone).
#include "ln_epilogue_f32.h"
#include "split_f32.h"

namespace {

using namespace pangu_split;

// WMW x WNW waves (ROWS: of 32 x 192, else of 64 x 96); NST ring stages (3: LDS-DMA two k-steps ahead; 2: one ahead)
template <int WMW, int WNW, int NST, bool ROWS, bool HAS_BIAS>
__global__ __launch_bounds__(64 * WMW * WNW, WMW * WNW == 8 ? 1 : 2) void gemm_ln_residual_f32_split_kernel(
    const float* __restrict__ A, int lda, const unsigned char* __restrict__ image, const float* __restrict__ bias,
    const float* __restrict__ shortcut, int lds_sc, const float* __restrict__ gamma, const float* __restrict__ beta,
    float* __restrict__ C, int ldc, int M, int K, float branch_scale) {
  using Tile = SplitTile<WMW, WNW, NST, ROWS>;     // Tile::BN = N: the tile spans the row, first n-tile block 0
  __shared__ __attribute__((aligned(16))) unsigned char smem[Tile::SMEM];
  const int m0 = blockIdx.x * Tile::BM;
  f32x16 acc[Tile::RB][Tile::CB];
  split_main_loop<WMW, WNW, NST, ROWS>(smem, A, lda, image, M, Tile::BN, K, m0, 0, acc);
  if constexpr (ROWS)
    pangu_ln::ln_residual_epilogue_rows<WMW, WNW, HAS_BIAS>(smem, acc, bias, shortcut, lds_sc, gamma, beta, C, ldc, M, m0,
                                                            branch_scale);
  else
    pangu_ln::ln_residual_epilogue<WMW, WNW, HAS_BIAS, false>(smem, acc, bias, shortcut, lds_sc, gamma, beta, C, ldc, M, m0,
                                                             branch_scale);
}

template <int WMW, int WNW, int NST, bool ROWS>
int launch_ln_split(hipStream_t s, const float* A, int lda, const unsigned char* image, const float* bias, const float* shortcut,
                    int lds, const float* gamma, const float* beta, float* out, int ldo, int M, int K, float branch_scale) {
  constexpr int BM = SplitTile<WMW, WNW, NST, ROWS>::BM;
  dim3 g((M + BM - 1) / BM), blk(64 * WMW * WNW);
  if (bias)
    hipLaunchKernelGGL((gemm_ln_residual_f32_split_kernel<WMW, WNW, NST, ROWS, true>), g, blk, 0, s, A, lda, image, bias, shortcut,
                       lds, gamma, beta, out, ldo, M, K, branch_scale);
  else
    hipLaunchKernelGGL((gemm_ln_residual_f32_split_kernel<WMW, WNW, NST, ROWS, false>), g, blk, 0, s, A, lda, image, bias, shortcut,
                       lds, gamma, beta, out, ldo, M, K, branch_scale);
  return pangu_launch_status();
}

}  // namespace

extern "C" int pangu_linear_ln_residual_fwd_split(pangu_stream_t stream, const float* A, int lda, const void* image,
                                                  const float* bias, const float* shortcut, int lds, const float* gamma,
                                                  const float* beta, float* out, int ldo, int M, int N, int K,
                                                  float branch_scale) {
  if (!A || !image || !shortcut || !gamma || !beta || !out) return PANGU_E_NULL;
  if (M <= 0 || K <= 0 || (K % BK) != 0 || lda < K || (lda & 3) || ldo < N || (ldo & 3) || lds < N || (lds & 3))
    return PANGU_E_SHAPE;
  if (N != 192 && N != 384) return PANGU_E_SHAPE;          // the tile must span the whole row
  if (!pangu_fits_u32(M, lda, 4) || !pangu_fits_u32(M, ldo, 4) || !pangu_fits_u32(M, lds, 4) ||
      (long long)N * K * 6 >= 0xFFFFFFFFll)
    return PANGU_E_RANGE;
  hipStream_t s = (hipStream_t)stream;
  const unsigned char* img = reinterpret_cast<const unsigned char*>(image);
  // Which wave tiling: the one that measured faster per shape, new median below the other's minimum (profiles/f32_split_rows_speed.md).
  // N = 192 keeps the 64 x 96 waves: the row-owning form (4 x 1 waves, three stages) measured 1.7 % slower at K = 192 and level at
  // K = 768 (one wave walks all 192 columns of its rows in the epilogue) and is not built.  N = 384 takes the row-owning 2 x 2 waves
  // for MLP-down (K = 1536: 1.1 % faster than 1 x 4 waves of 64 x 96, where four waves split every A row); at K = 384 the two are
  // level, so the short K stay where they were.  Nothing between the two K was measured: the model has no such shape
  if (N == 192) return launch_ln_split<2, 2, 3, false>(s, A, lda, img, bias, shortcut, lds, gamma, beta, out, ldo, M, K, branch_scale);
  if (K < 1536) return launch_ln_split<1, 4, 2, false>(s, A, lda, img, bias, shortcut, lds, gamma, beta, out, ldo, M, K, branch_scale);
  return launch_ln_split<2, 2, 2, true>(s, A, lda, img, bias, shortcut, lds, gamma, beta, out, ldo, M, K, branch_scale);
}
