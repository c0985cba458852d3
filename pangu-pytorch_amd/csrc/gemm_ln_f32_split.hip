// fp32 projection GEMM + post-norm residual in one launch on the bf16 matrix pipe (inference path):
//   out[M,N] = shortcut + branch_scale * (LayerNorm(A[M,K] @ W[N,K]^T + bias) * gamma + beta)           (layers.py:250-251)
// for N = 192 and N = 384, W given as its exact-split image (pangu_split_weight_bf16x3).  The main loop is split_main_loop of
// split_f32.h, the one gemm_f32_split.hip runs; the epilogue is ln_residual_epilogue of ln_epilogue_f32.h, the one
// gemm_ln_f32_dma.hip runs, so the product is the only numerical difference between the two fused kernels.
//
//   N = 192: 128 x 192 tile, 2 x 2 waves, ring of three 26-KB stages = 78 KB, two workgroups per CU.
//   N = 384: the tile spans the row (the LayerNorm statistics stay in the workgroup), its W part is the image's two 192-row
//            n-tile blocks of the k-step, 36 KB: 64 x 384 tile, 1 x 4 waves, ring of two 40-KB stages (LDS-DMA one k-step ahead)
//            = 80 KB, two workgroups per CU, so one workgroup's main loop covers the other's epilogue.  The measured alternative,
//            128 x 384 with 2 x 4 waves and three 44-KB stages (<2, 4, 3>: 132 KB, one workgroup per CU), is 7 % slower at
//            K = 384 and at K = 1536 (profiles/f32_split_ln_per_shape.md) and is not instantiated.
// Either way 2 waves per SIMD: 256 VGPRs, so the 96 accumulators and the 48 transposed row registers of the epilogue are live
// together without scratch (the fp32-MFMA kernel's 128-VGPR cap is gone).
#include "ln_epilogue_f32.h"
#include "split_f32.h"

namespace {

using namespace pangu_split;

// WMW x WNW waves of 64 x 96; NST ring stages (3: LDS-DMA two k-steps ahead; 2: one ahead)
template <int WMW, int WNW, int NST, bool HAS_BIAS>
__global__ __launch_bounds__(64 * WMW * WNW, WMW * WNW == 8 ? 1 : 2) void gemm_ln_residual_f32_split_kernel(
    const float* __restrict__ A, int lda, const unsigned char* __restrict__ image, const float* __restrict__ bias,
    const float* __restrict__ shortcut, int lds_sc, const float* __restrict__ gamma, const float* __restrict__ beta,
    float* __restrict__ C, int ldc, int M, int K, float branch_scale) {
  using Tile = SplitTile<WMW, WNW, NST>;           // Tile::BN = N: the tile spans the row, first n-tile block 0
  __shared__ __attribute__((aligned(16))) unsigned char smem[Tile::SMEM];
  const int m0 = blockIdx.x * Tile::BM;
  f32x16 acc[2][3];
  split_main_loop<WMW, WNW, NST>(smem, A, lda, image, M, Tile::BN, K, m0, 0, acc);
  pangu_ln::ln_residual_epilogue<WMW, WNW, HAS_BIAS, false>(smem, acc, bias, shortcut, lds_sc, gamma, beta, C, ldc, M, m0,
                                                           branch_scale);
}

template <int WMW, int WNW, int NST>
int launch_ln_split(hipStream_t s, const float* A, int lda, const unsigned char* image, const float* bias, const float* shortcut,
                    int lds, const float* gamma, const float* beta, float* out, int ldo, int M, int K, float branch_scale) {
  constexpr int BM = 64 * WMW;
  dim3 g((M + BM - 1) / BM), blk(64 * WMW * WNW);
  if (bias)
    hipLaunchKernelGGL((gemm_ln_residual_f32_split_kernel<WMW, WNW, NST, true>), g, blk, 0, s, A, lda, image, bias, shortcut, lds,
                       gamma, beta, out, ldo, M, K, branch_scale);
  else
    hipLaunchKernelGGL((gemm_ln_residual_f32_split_kernel<WMW, WNW, NST, false>), g, blk, 0, s, A, lda, image, bias, shortcut, lds,
                       gamma, beta, out, ldo, M, K, branch_scale);
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
  if (N == 192) return launch_ln_split<2, 2, 3>(s, A, lda, img, bias, shortcut, lds, gamma, beta, out, ldo, M, K, branch_scale);
  return launch_ln_split<1, 4, 2>(s, A, lda, img, bias, shortcut, lds, gamma, beta, out, ldo, M, K, branch_scale);
}
