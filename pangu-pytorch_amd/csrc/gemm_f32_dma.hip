// fp32 projection GEMM, LDS-DMA variant for the 128 x 192 tile (TN = 3): C[M,N] = act(A[M,K] @ W[N,K]^T + bias).
//
// Same MFMA scheme as gemm_f32.hip (exact-f32 v_mfma_f32_32x32x2_f32, permuted-k b128 fragments, 2 x 2 waves of 64 x 96),
// but built for OCCUPANCY, the strongest lever measured on this chip: the register-staged kernel needs 168 VGPRs and
// 51 KB of LDS (three workgroups per CU); here the operands travel L2 -> LDS by LDS-DMA (buffer_load_dwordx4 ... lds: no
// staging registers, no ds_write pass) into an UNPADDED 64-byte-row image whose 16-B chunks are XOR-swizzled on the
// SOURCE side (conflict-free ds_read_b128 lane groups), the fragments of the two k-halves share registers, and a ring of
// two 20-KB stages leaves 40 KB per workgroup: FOUR workgroups per CU at <= 128 VGPRs.
// The main loop is dma_main_loop of gemm_f32_dma_loop.h, shared with gemm_ln_f32_dma.hip; this file holds the plain store epilogue.
#include "gemm_f32_dma_loop.h"

namespace {

using namespace pangu_dma;

// TN = 3: 128 x 192 tile, 40 KB ring, 126 VGPRs -> four workgroups per CU; TN = 2: 128 x 128 tile, 32 KB ring -> five
template <int TN, int ACT, bool HAS_BIAS>
__global__ __launch_bounds__(256, TN == 3 ? 4 : 5) void gemm_tn_f32_dma_kernel(const float* __restrict__ A, int lda,
                                                                 const float* __restrict__ W, const float* __restrict__ bias,
                                                                 float* __restrict__ C, int ldc, int M, int N, int K,
                                                                 int m_tiles, int n_tiles, float* __restrict__ aux) {
  using Tile = DmaTile<2, TN>;
  constexpr int BN = Tile::BN;
  __shared__ __attribute__((aligned(16))) unsigned char smem[Tile::SMEM];

  // XCD-aware tile assignment (blocks b, b+8, b+16.. share an XCD; they walk the n-tiles of one m-tile).
  const int b = blockIdx.x;
  const int xcd = b & 7, local = b >> 3;
  const int m_tile = (local / n_tiles) * 8 + xcd;
  const int n_tile = local % n_tiles;
  if (m_tile >= m_tiles) return;
  const int m0 = m_tile * BM, n0 = n_tile * BN;

  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int wm = wave >> 1, wn = wave & 1;
  const int lr = lane & 31, lh = lane >> 5;

  f32x16 acc[2][TN];
  dma_main_loop<2, TN>(smem, A, lda, W, M, N, K, m0, n0, wave, acc);

  // epilogue (as gemm_f32.hip): each 32x32 tile is transposed through a wave-private LDS patch -> 16-B row segments
  constexpr int EP_LD = 36;
  float* ep = reinterpret_cast<float*>(smem) + wave * (32 * EP_LD);
  const int er = lane >> 3, ec = (lane & 7) * 4;
  const __amdgpu_buffer_rsrc_t c_rsrc = __builtin_amdgcn_make_buffer_rsrc(
      C, 0, (int)(((size_t)(M - 1) * ldc + N) * sizeof(float)), 0x00020000);
  const __amdgpu_buffer_rsrc_t x_rsrc = __builtin_amdgcn_make_buffer_rsrc(
      aux, 0, aux ? (int)((size_t)M * N * sizeof(float)) : 0, 0x00020000);
#pragma unroll
  for (int j = 0; j < TN; ++j) {
    const int col = n0 + wn * 32 * TN + j * 32 + ec;
    const bool col_ok = col < N;
    f32x4 bv = {0.f, 0.f, 0.f, 0.f};
    if (HAS_BIAS) bv = *reinterpret_cast<const f32x4*>(bias + (col_ok ? col : 0));
#pragma unroll
    for (int i = 0; i < 2; ++i) {
#pragma unroll
      for (int r = 0; r < 16; ++r) ep[((r & 3) + 8 * (r >> 2) + 4 * lh) * EP_LD + lr] = acc[i][j][r];
      const int row0 = m0 + wm * 64 + i * 32 + er;
#pragma unroll
      for (int it = 0; it < 4; ++it) {
        f32x4 v = *reinterpret_cast<const f32x4*>(&ep[(er + 8 * it) * EP_LD + ec]);
        v += bv;
        const unsigned xoff = col_ok ? ((unsigned)(row0 + 8 * it) * (unsigned)N + (unsigned)col) * 4u : 0xFFFFFFFFu;
        if (ACT == PANGU_ACT_GELU) {
          __builtin_amdgcn_raw_buffer_store_b128(__builtin_bit_cast(u32x4, v), x_rsrc, (int)xoff, 0, 0);
#pragma unroll
          for (int c = 0; c < 4; ++c) v[c] = gelu_erf(v[c]);
        }
        if (ACT == PANGU_ACT_GELU_BWD) {
          const f32x4 x = __builtin_bit_cast(f32x4, __builtin_amdgcn_raw_buffer_load_b128(x_rsrc, (int)xoff, 0, 0));
#pragma unroll
          for (int c = 0; c < 4; ++c) v[c] *= gelu_erf_grad(x[c]);
        }
        if (ACT == PANGU_ACT_ADD) v += __builtin_bit_cast(f32x4, __builtin_amdgcn_raw_buffer_load_b128(x_rsrc, (int)xoff, 0, 0));
        const unsigned off = col_ok ? ((unsigned)(row0 + 8 * it) * (unsigned)ldc + (unsigned)col) * 4u : 0xFFFFFFFFu;
        // non-temporal: the 0.2-1.6 GB output is written once and read by the NEXT kernel; streaming it past L2 keeps the A / W
        // panels resident (+2-4 % per launch, +0.7 % on the forward)
        __builtin_amdgcn_raw_buffer_store_b128(__builtin_bit_cast(u32x4, v), c_rsrc, (int)off, 0, 2);
      }
    }
  }
}

}  // namespace

template <int TN>
int launch_dma(hipStream_t s, const float* A, int lda, const float* W, const float* bias, float* C, int ldc, int M, int N, int K,
               int act, float* aux) {
  constexpr int BN = 64 * TN;
  const int m_tiles = (M + BM - 1) / BM, n_tiles = (N + BN - 1) / BN;
  const int grid = ((m_tiles + 7) / 8) * 8 * n_tiles;
  dim3 g(grid), blk(256);
#define PANGU_DMA_LAUNCH(ACT, HB) \
  hipLaunchKernelGGL((gemm_tn_f32_dma_kernel<TN, ACT, HB>), g, blk, 0, s, A, lda, W, bias, C, ldc, M, N, K, m_tiles, n_tiles, aux)
  if (act == PANGU_ACT_GELU) {
    if (bias) PANGU_DMA_LAUNCH(PANGU_ACT_GELU, true); else PANGU_DMA_LAUNCH(PANGU_ACT_GELU, false);
  } else if (act == PANGU_ACT_GELU_BWD) {
    if (bias) PANGU_DMA_LAUNCH(PANGU_ACT_GELU_BWD, true); else PANGU_DMA_LAUNCH(PANGU_ACT_GELU_BWD, false);
  } else if (act == PANGU_ACT_ADD) {
    if (bias) PANGU_DMA_LAUNCH(PANGU_ACT_ADD, true); else PANGU_DMA_LAUNCH(PANGU_ACT_ADD, false);
  } else {
    if (bias) PANGU_DMA_LAUNCH(PANGU_ACT_NONE, true); else PANGU_DMA_LAUNCH(PANGU_ACT_NONE, false);
  }
#undef PANGU_DMA_LAUNCH
  return pangu_launch_status();
}

// gemm_f32.hip dispatches here: tn = 3 for its 192-wide-tile shapes, 2 for the 128-wide ones
int pangu_linear_f32_dma(hipStream_t s, const float* A, int lda, const float* W, const float* bias, float* C, int ldc, int M,
                         int N, int K, int act, float* aux, int tn) {
  if (tn == 3) return launch_dma<3>(s, A, lda, W, bias, C, ldc, M, N, K, act, aux);
  return launch_dma<2>(s, A, lda, W, bias, C, ldc, M, N, K, act, aux);
}
