// fp32 projection GEMM on the bf16 matrix pipe: C[M,N] = act(A[M,K] @ W[N,K]^T + bias), fp32 in, fp32 out.
//
// An fp32 number is EXACTLY the sum of three bf16 numbers, hi = bf16(a), mid = bf16(a - hi), lo = bf16(a - hi - mid) (24
// significand bits = 3 x 8, both subtractions exact, bf16 has fp32's exponent range), so a product a*b is the sum of nine exact
// bf16 x bf16 products.  The six of order >= 2^-16 -- (lo,hi) (hi,lo) (mid,mid) (mid,hi) (hi,mid) (hi,hi), small terms first into
// one fp32 accumulator -- drop only terms of relative size <= 2^-23 per product: the size of the one rounding the fp32 MFMA
// chain commits per product.  Six v_mfma_f32_32x32x16_bf16 (32 cycles each) replace eight v_mfma_f32_32x32x2_f32 (64 each).
//
//   * W is split ONCE per weight (pangu_split_weight_bf16x3) into an image that is already the LDS stage image of the GEMM:
//     [n-tile of 192][k-step of 16][plane hi/mid/lo][k-half][row 0..191][8 bf16], 18 KB per (n-tile, k-step), streamed by 18
//     linear 1-KB LDS-DMA pieces; a fragment read (32 consecutive rows of one plane and k-half, 16 B each) is conflict-free.
//   * A stays fp32 in memory, travels L2 -> LDS by LDS-DMA into the swizzled 64-byte-row image of gemm_f32_dma_loop.h; a lane
//     reads its 8 consecutive k as two b128 and splits them in registers (plain casts: v_cvt_pk_bf16_f32, two exact subtracts).
//   * 128 x 192 tile, 4 x 1 waves of 32 x 192: a wave owns its 32 rows, so every A element is split once (two waves shared the
//     rows of the 2 x 2 waves of 64 x 96 this replaces, and each split them: 88 VALU instructions per wave and k-step, now 40).
//     A ring of two 26-KB stages (LDS-DMA one k-step ahead, one barrier per step): 52 KB and 163 VGPRs -> THREE workgroups per
//     CU, which is where the time comes from on the K = 192 / 384 launches (prologue and epilogue of one workgroup under the
//     loops of two others): 5-7 % at K = 192, 0.6-3 % at K = 384, bit for bit the same product (profiles/f32_split_rows_speed.md).
//     The main loop is split_main_loop<4, 1, 2, true, true> of split_f32.h, shared with gemm_ln_f32_split.hip; this file holds
//     the weight split and the plain store epilogue.
//
// Values whose bf16 rounding overflows (|a| >= 2^128 - 2^119) or whose lo part falls below the bf16 denormal range lose the
// exactness of the split; neither occurs in weights or activations of this model.
#include "split_f32.h"

namespace {

using namespace pangu_split;      // bf16x8, BK, PLANE, B_BYTES, split8, SplitTile, split_main_loop

using Tile = SplitTile<4, 1, 2, true>;           // 4 x 1 row-owning waves, ring of two stages
constexpr int BM = Tile::BM;                     // 128
constexpr int BN = Tile::BN;                     // 192 = W_ROWS: one n-tile block of the image per tile

// One thread per (row n, 8 consecutive k): W[N][K] fp32 -> the three planes of the image (layout above; N % 4 == 0, K % 16 == 0).
// The image has rows = ceil(N / 192) * 192 rows.  PAD (rows > N): rows >= N are zero rows, never read from W, +0 in all three planes.
template <bool PAD>
__global__ __launch_bounds__(256) void split_weight_kernel(const float* __restrict__ W, unsigned char* __restrict__ image, int N,
                                                           int K, int rows) {
  const int kc = K >> 3;
  const long long t = (long long)blockIdx.x * 256 + threadIdx.x;
  if (t >= (long long)(PAD ? rows : N) * kc) return;
  const int n = (int)(t / kc), c = (int)(t - (long long)n * kc);
  const float* src = W + (size_t)n * K + c * 8;
  f32x4 c0 = {0.f, 0.f, 0.f, 0.f}, c1 = {0.f, 0.f, 0.f, 0.f};
  if (!PAD || n < N) {
    c0 = *reinterpret_cast<const f32x4*>(src);
    c1 = *reinterpret_cast<const f32x4*>(src + 4);
  }
  bf16x8 p[3];
  split8(c0, c1, p[0], p[1], p[2]);
  const int nt = n / BN, nl = n - nt * BN, kt = c >> 1, lh = c & 1;
  unsigned char* dst = image + ((size_t)nt * (K / BK) + kt) * B_BYTES + (lh * BN + nl) * 16;
#pragma unroll
  for (int q = 0; q < 3; ++q) *reinterpret_cast<bf16x8*>(dst + q * PLANE) = p[q];
}

// PADN: the image has 192 n_tiles rows, of which the first N (N % 4 == 0) are W's and the rest zero rows; the epilogue skips the
// bias load and the store of every 16-byte column segment that starts at a column >= N (segments are whole: N % 4 == 0), so
// neither bias[N..] is read nor C's columns >= N are written (ldc may exceed N).  The product is the unpadded kernel's.
template <int ACT, bool HAS_BIAS, bool PADN = false>
__global__ __launch_bounds__(256, 3) void gemm_f32_split_kernel(const float* __restrict__ A, int lda,
                                                                const unsigned char* __restrict__ image,
                                                                const float* __restrict__ bias, float* __restrict__ C, int ldc,
                                                                int M, int N, int K, int m_tiles, int n_tiles) {
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
  const int lr = lane & 31, lh = lane >> 5;

  f32x16 acc[1][6];                                // the wave's rows 32 wave .. +31 x the tile's 192 columns
  split_main_loop<4, 1, 2, true, true>(smem, A, lda, image, M, PADN ? n_tiles * BN : N, K, m0, n_tile, acc);

  // epilogue (as gemm_f32_dma.hip): each 32x32 tile is transposed through a wave-private LDS patch -> 16-B row segments
  constexpr int EP_LD = 36;
  float* ep = reinterpret_cast<float*>(smem) + wave * (32 * EP_LD);
  const int er = lane >> 3, ec = (lane & 7) * 4;
  const __amdgpu_buffer_rsrc_t c_rsrc = __builtin_amdgcn_make_buffer_rsrc(
      C, 0, (int)(((size_t)(M - 1) * ldc + N) * sizeof(float)), 0x00020000);
  const int row0 = m0 + wave * 32 + er;
#pragma unroll
  for (int j = 0; j < 6; ++j) {
    const int col = n0 + j * 32 + ec;
    const bool live = !PADN || col < N;            // PADN: this lane's column segment of the tile exists
    f32x4 bv = {0.f, 0.f, 0.f, 0.f};
    if (HAS_BIAS && live) bv = *reinterpret_cast<const f32x4*>(bias + col);
#pragma unroll
    for (int r = 0; r < 16; ++r) ep[((r & 3) + 8 * (r >> 2) + 4 * lh) * EP_LD + lr] = acc[0][j][r];
#pragma unroll
    for (int it = 0; it < 4; ++it) {
      f32x4 v = *reinterpret_cast<const f32x4*>(&ep[(er + 8 * it) * EP_LD + ec]);
      v += bv;
      if (ACT == PANGU_ACT_GELU) {
#pragma unroll
        for (int c = 0; c < 4; ++c) v[c] = gelu_erf(v[c]);
      }
      // rows >= M fall outside the descriptor's range and are dropped; non-temporal as in gemm_f32_dma.hip
      const unsigned off = ((unsigned)(row0 + 8 * it) * (unsigned)ldc + (unsigned)col) * 4u;
      if (live) __builtin_amdgcn_raw_buffer_store_b128(__builtin_bit_cast(u32x4, v), c_rsrc, (int)off, 0, 2);
    }
  }
}

}  // namespace

// Rows of the image of an N-row weight: W's N rows and zero rows behind them up to whole 192-row n-tile blocks.
static long long image_rows(int N) { return ((long long)N + BN - 1) / BN * BN; }

extern "C" int pangu_split_weight_bf16x3(pangu_stream_t stream, const float* W, int N, int K, void* image) {
  if (!W || !image) return PANGU_E_NULL;
  if (N <= 0 || K <= 0 || (N % 4) != 0 || (K % BK) != 0) return PANGU_E_SHAPE;
  const long long rows = image_rows(N);
  if (rows * K * 6 >= 0xFFFFFFFFll) return PANGU_E_RANGE;
  const dim3 g((unsigned)((rows * (K / 8) + 255) / 256)), blk(256);
  hipLaunchKernelGGL(rows == N ? split_weight_kernel<false> : split_weight_kernel<true>, g, blk, 0, (hipStream_t)stream, W,
                     reinterpret_cast<unsigned char*>(image), N, K, (int)rows);
  return pangu_launch_status();
}

extern "C" int pangu_linear_fwd_split(pangu_stream_t stream, const float* A, int lda, const void* image, const float* bias,
                                      float* C, int ldc, int M, int N, int K, int act) {
  if (!A || !image || !C) return PANGU_E_NULL;
  if (M <= 0 || N <= 0 || K <= 0 || lda < K || ldc < N || (lda & 3) || (ldc & 3)) return PANGU_E_SHAPE;
  if (act != PANGU_ACT_NONE && act != PANGU_ACT_GELU) return PANGU_E_ARG;
  if ((N % 4) != 0 || (K % BK) != 0) return PANGU_E_SHAPE;       // not served: the caller takes pangu_linear_fwd
  const long long rows = image_rows(N);
  if (!pangu_fits_u32(M, lda, 4) || !pangu_fits_u32(M, ldc, 4) || rows * K * 6 >= 0xFFFFFFFFll) return PANGU_E_RANGE;
  const int m_tiles = (M + BM - 1) / BM, n_tiles = (int)(rows / BN);
  const dim3 g(((m_tiles + 7) / 8) * 8 * n_tiles), blk(256);
  hipStream_t s = (hipStream_t)stream;
  const unsigned char* img = reinterpret_cast<const unsigned char*>(image);
  const bool whole = rows == N;      // whole 192-column tiles: the instantiation without the column guard (same bits either way)
#define PANGU_SPLIT_LAUNCH(ACT, HB)                                                                                          \
  hipLaunchKernelGGL((whole ? gemm_f32_split_kernel<ACT, HB, false> : gemm_f32_split_kernel<ACT, HB, true>), g, blk, 0, s, A, \
                     lda, img, bias, C, ldc, M, N, K, m_tiles, n_tiles)
  if (act == PANGU_ACT_GELU) {
    if (bias) PANGU_SPLIT_LAUNCH(PANGU_ACT_GELU, true); else PANGU_SPLIT_LAUNCH(PANGU_ACT_GELU, false);
  } else {
    if (bias) PANGU_SPLIT_LAUNCH(PANGU_ACT_NONE, true); else PANGU_SPLIT_LAUNCH(PANGU_ACT_NONE, false);
  }
#undef PANGU_SPLIT_LAUNCH
  return pangu_launch_status();
}
