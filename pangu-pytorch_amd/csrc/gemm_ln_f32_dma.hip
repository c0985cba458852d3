// fp32 projection GEMM + post-norm residual in one launch, LDS-DMA variant (inference path):
//   out[M,N] = shortcut + branch_scale * (LayerNorm(A[M,K] @ W[N,K]^T + bias) * gamma + beta)           (layers.py:250-251)
// for N = 192 (WNW = 2: 4 waves, 128 x 192 tile, 40-KB ring, four workgroups per CU) and N = 384 (WNW = 4: 8 waves,
// 128 x 384 tile, 64-KB ring, two workgroups per CU): either way 16 waves per CU at <= 128 VGPRs, the occupancy of the plain
// LDS-DMA GEMM (gemm_f32_dma.hip), whose main loop this is (dma_main_loop of gemm_f32_dma_loop.h) -- and the tile spans the
// whole row, so the LayerNorm statistics never leave the workgroup.  The epilogue is ln_residual_epilogue of ln_epilogue_f32.h,
// shared with gemm_ln_f32_split.hip.
#include "gemm_f32_dma_loop.h"
#include "ln_epilogue_f32.h"

namespace {

using namespace pangu_dma;

template <int WNW, bool HAS_BIAS>
__global__ __launch_bounds__(128 * WNW, 4) void gemm_ln_residual_f32_dma_kernel(
    const float* __restrict__ A, int lda, const float* __restrict__ W, const float* __restrict__ bias,
    const float* __restrict__ shortcut, int lds_sc, const float* __restrict__ gamma, const float* __restrict__ beta,
    float* __restrict__ C, int ldc, int M, int K, float branch_scale) {
  using Tile = DmaTile<WNW, 3>;                    // Tile::BN = N: the tile spans the row, n0 = 0
  __shared__ __attribute__((aligned(16))) unsigned char smem[Tile::SMEM];
  const int m0 = blockIdx.x * BM;
  f32x16 acc[2][3];
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  dma_main_loop<WNW, 3>(smem, A, lda, W, M, Tile::BN, K, m0, 0, wave, acc);
  pangu_ln::ln_residual_epilogue<2, WNW, HAS_BIAS, true>(smem, acc, bias, shortcut, lds_sc, gamma, beta, C, ldc, M, m0,
                                                       branch_scale);
}

template <int WNW>
int launch_ln_dma(hipStream_t s, const float* A, int lda, const float* W, const float* bias, const float* shortcut, int lds,
                  const float* gamma, const float* beta, float* out, int ldo, int M, int K, float branch_scale) {
  dim3 g((M + BM - 1) / BM), blk(128 * WNW);
  if (bias)
    hipLaunchKernelGGL((gemm_ln_residual_f32_dma_kernel<WNW, true>), g, blk, 0, s, A, lda, W, bias, shortcut, lds, gamma, beta,
                       out, ldo, M, K, branch_scale);
  else
    hipLaunchKernelGGL((gemm_ln_residual_f32_dma_kernel<WNW, false>), g, blk, 0, s, A, lda, W, bias, shortcut, lds, gamma, beta,
                       out, ldo, M, K, branch_scale);
  return pangu_launch_status();
}

}  // namespace

extern "C" int pangu_linear_ln_residual_fwd(pangu_stream_t stream, const float* A, int lda, const float* W, const float* bias,
                                            const float* shortcut, int lds, const float* gamma, const float* beta, float* out,
                                            int ldo, int M, int N, int K, float branch_scale) {
  if (!A || !W || !shortcut || !gamma || !beta || !out) return PANGU_E_NULL;
  if (M <= 0 || K <= 0 || (K % BK) != 0 || lda < K || (lda & 3) || ldo < N || (ldo & 3) || lds < N || (lds & 3))
    return PANGU_E_SHAPE;
  if (N != 192 && N != 384) return PANGU_E_SHAPE;          // the tile must span the whole row
  if (!pangu_fits_u32(M, lda, 4) || !pangu_fits_u32(M, ldo, 4) || !pangu_fits_u32(M, lds, 4)) return PANGU_E_RANGE;
  hipStream_t s = (hipStream_t)stream;
  if (N == 192) return launch_ln_dma<2>(s, A, lda, W, bias, shortcut, lds, gamma, beta, out, ldo, M, K, branch_scale);
  return launch_ln_dma<4>(s, A, lda, W, bias, shortcut, lds, gamma, beta, out, ldo, M, K, branch_scale);
}
