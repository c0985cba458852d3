// fp32 projection GEMM + post-norm residual in one launch on the bf16 matrix pipe (inference path):
//   out[M,N] = shortcut + branch_scale * (LayerNorm(A[M,K] @ W[N,K]^T + bias) * gamma + beta)           (layers.py:250-251)
// for N = 192 and N = 384, W given as its exact-split image (pangu_split_weight_bf16x3).  The main loop is that of
// gemm_f32_split.hip (fp32 A through LDS-DMA into the swizzled 64-byte-row image and split in registers, W planes as linear 1-KB
// LDS-DMA pieces, waves of 64 x 96, the six products small terms first into one accumulator); the epilogue is that of
// gemm_ln_f32_dma.hip, operation for operation, so the product is the only numerical difference between the two.
//
//   N = 192: 128 x 192 tile, 2 x 2 waves, ring of three 26-KB stages = 78 KB, two workgroups per CU.
//   N = 384: the tile spans the row (the LayerNorm statistics stay in the workgroup), its W part is the image's two 192-row
//            n-tile blocks of the k-step, 36 KB: 64 x 384 tile, 1 x 4 waves, ring of two 40-KB stages (LDS-DMA one k-step ahead)
//            = 80 KB, two workgroups per CU, so one workgroup's main loop covers the other's epilogue.  The measured alternative,
//            128 x 384 with 2 x 4 waves and three 44-KB stages (<2, 4, 3>: 132 KB, one workgroup per CU), is 7 % slower at
//            K = 384 and at K = 1536 (profiles/f32_split_ln_per_shape.md) and is not instantiated.
// Either way 2 waves per SIMD: 256 VGPRs, so the 96 accumulators and the 48 transposed row registers of the epilogue are live
// together without scratch (the fp32-MFMA kernel's 128-VGPR cap is gone).
#include "split_f32.h"

namespace {

using namespace pangu_split;

constexpr float LN_EPS = 1e-5f;

// sum over the 8 lanes that share lane >> 3 (DPP quad_perm x2 + row_half_mirror), result in every lane
__device__ inline float oct_sum(float v) {
  v += __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, v), 0xB1, 0xF, 0xF, true));
  v += __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, v), 0x4E, 0xF, 0xF, true));
  v += __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, v), 0x141, 0xF, 0xF, true));
  return v;
}

// WMW x WNW waves of 64 x 96; NST ring stages (3: LDS-DMA two k-steps ahead; 2: one ahead)
template <int WMW, int WNW, int NST, bool HAS_BIAS>
__global__ __launch_bounds__(64 * WMW * WNW, WMW * WNW == 8 ? 1 : 2) void gemm_ln_residual_f32_split_kernel(
    const float* __restrict__ A, int lda, const unsigned char* __restrict__ image, const float* __restrict__ bias,
    const float* __restrict__ shortcut, int lds_sc, const float* __restrict__ gamma, const float* __restrict__ beta,
    float* __restrict__ C, int ldc, int M, int K, float branch_scale) {
  constexpr int NW = WMW * WNW;                    // waves
  constexpr int BM = 64 * WMW;
  constexpr int BN = 96 * WNW;                     // = N
  constexpr int NT = BN / W_ROWS;                  // n-tile blocks of the image per k-step
  constexpr int A_BYTES = BM * 64;                 // fp32 A image: BM rows of 64 B
  constexpr int A_PIECES = A_BYTES / 1024;
  constexpr int STAGE = A_BYTES + NT * B_BYTES;
  constexpr int PIECES = STAGE / 1024;             // piece q goes to wave q % NW
  constexpr int A_IT = A_PIECES / NW;              // issue rounds that are all A
  constexpr int IT = (PIECES + NW - 1) / NW;       // issue rounds; waves < REM issue IT pieces, the others IT - 1 (REM = 0: all IT)
  constexpr int REM = PIECES % NW;
  static_assert(NST == 2 || NST == 3, "ring depth");
  static_assert(A_PIECES % NW == 0 && BN % W_ROWS == 0, "piece rounds");
  __shared__ __attribute__((aligned(16))) unsigned char smem[NST * STAGE];

  const int m0 = blockIdx.x * BM;
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int wm = wave / WNW, wn = wave % WNW;
  const int lr = lane & 31, lh = lane >> 5;
  const int KT = K / BK;

  const __amdgpu_buffer_rsrc_t a_rsrc = __builtin_amdgcn_make_buffer_rsrc(
      const_cast<float*>(A), 0, (int)(((size_t)(M - 1) * lda + K) * sizeof(float)), 0x00020000);
  const __amdgpu_buffer_rsrc_t w_rsrc = __builtin_amdgcn_make_buffer_rsrc(
      const_cast<unsigned char*>(image), 0, (int)((size_t)BN * K * 6), 0x00020000);
  // piece q = i*NW + wave (q < PIECES).  q < A_PIECES: rows 16q .. 16q+15 of A, this lane fills (row 16q + lane>>2, physical chunk
  // lane&3), i.e. fetches logical chunk (lane&3) ^ F(row); rows >= M are out of range: zeros.  Otherwise piece p = q - A_PIECES of
  // the W part: bytes 1024 (p % 18) .. +1023 of the (n-tile p / 18, k-step) block of the image, copied linearly.
  unsigned voff_a[A_IT], voff_w[IT - A_IT];
#pragma unroll
  for (int i = 0; i < A_IT; ++i) {
    const int row = 16 * (i * NW + wave) + (lane >> 2);
    const int f = (0x78 >> (((row >> 2) & 3) * 2)) & 3;
    voff_a[i] = ((unsigned)(m0 + row) * (unsigned)lda + ((lane & 3) ^ f) * 4) * 4u;
  }
#pragma unroll
  for (int i = A_IT; i < IT; ++i) {
    const int p = i * NW + wave - A_PIECES;
    voff_w[i - A_IT] = (unsigned)(p / W_PIECES) * (unsigned)KT * (unsigned)B_BYTES + (unsigned)(p % W_PIECES) * 1024u + lane * 16;
  }
  auto issue = [&](int kt, int slot) {
    unsigned char* base = smem + slot * STAGE;
#pragma unroll
    for (int i = 0; i < IT; ++i) {
      const int q = i * NW + wave;
      auto dst = (__attribute__((address_space(3))) void*)(base + q * 1024);
      if (i < A_IT) {
        __builtin_amdgcn_raw_ptr_buffer_load_lds(a_rsrc, dst, 16, (int)voff_a[i], kt * BK * 4, 0, 0);
      } else if (i * NW + NW - 1 < PIECES || q < PIECES) {
        __builtin_amdgcn_raw_ptr_buffer_load_lds(w_rsrc, dst, 16, (int)voff_w[i - A_IT], kt * B_BYTES, 0, 0);
      }
    }
  };

  f32x16 acc[2][3];
#pragma unroll
  for (int i = 0; i < 2; ++i)
#pragma unroll
    for (int j = 0; j < 3; ++j)
#pragma unroll
      for (int r = 0; r < 16; ++r) acc[i][j][r] = 0.f;

  // fragment byte offsets: lane (lr, lh) owns k = 8lh .. 8lh+7 of its row: logical chunks 2lh, 2lh+1 of the fp32 A row, and
  // chunk (k-half lh, row) of each W plane of the wave's n-tile block
  int off_a[2][2];
#pragma unroll
  for (int i = 0; i < 2; ++i)
#pragma unroll
    for (int h = 0; h < 2; ++h) off_a[i][h] = kswz64(wm * 64 + i * 32 + lr, 2 * lh + h);
  const int off_w = A_BYTES + (wn >> 1) * B_BYTES + (lh * W_ROWS + (wn & 1) * 96 + lr) * 16;

  issue(0, 0);
  if (NST == 3 && KT > 1) issue(1, 1);
  int slot = 0;
  for (int kt = 0; kt < KT; ++kt) {
    // this wave's pieces of step kt have landed (three stages: those of step kt+1 may still fly, IT or IT - 1 per wave)
    if (NST == 3 && kt + 1 < KT) {
      if (REM == 0 || wave < REM) asm volatile("s_waitcnt vmcnt(%0)" ::"n"(IT) : "memory");
      else asm volatile("s_waitcnt vmcnt(%0)" ::"n"(IT - 1) : "memory");
    } else {
      asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    }
    __builtin_amdgcn_s_barrier();                          // ... and everybody's; the slot read in step kt-1 is free
    asm volatile("" ::: "memory");
    if (NST == 3) {
      if (kt + 2 < KT) issue(kt + 2, slot == 0 ? 2 : slot - 1);
    } else {
      if (kt + 1 < KT) issue(kt + 1, slot ^ 1);
    }
    const unsigned char* St = smem + slot * STAGE;
    slot = slot == NST - 1 ? 0 : slot + 1;

    bf16x8 bw[3][3];                                       // [column block][plane]
#pragma unroll
    for (int j = 0; j < 3; ++j)
#pragma unroll
      for (int p = 0; p < 3; ++p) bw[j][p] = *reinterpret_cast<const bf16x8*>(St + off_w + p * PLANE + j * 512);
    f32x4 ca[2][2];
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
      for (int h = 0; h < 2; ++h) ca[i][h] = *reinterpret_cast<const f32x4*>(St + off_a[i][h]);
    bf16x8 ah[2], am[2], al[2];
    split8(ca[0][0], ca[0][1], ah[0], am[0], al[0]);
    auto products = [&](int i) {                            // small terms first, one accumulator per output block
#pragma unroll
      for (int j = 0; j < 3; ++j) {
        acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(al[i], bw[j][0], acc[i][j], 0, 0, 0);
        acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(ah[i], bw[j][2], acc[i][j], 0, 0, 0);
        acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(am[i], bw[j][1], acc[i][j], 0, 0, 0);
        acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(am[i], bw[j][0], acc[i][j], 0, 0, 0);
        acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(ah[i], bw[j][1], acc[i][j], 0, 0, 0);
        acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(ah[i], bw[j][0], acc[i][j], 0, 0, 0);
      }
    };
    // the split of the second row block (44 VALU instructions) goes into the issue gaps of the first block's 18 MFMAs
    __builtin_amdgcn_sched_barrier(0);
    products(0);
    split8(ca[1][0], ca[1][1], ah[1], am[1], al[1]);
#pragma unroll
    for (int g = 0; g < 18; ++g) {
      __builtin_amdgcn_sched_group_barrier(0x008, 1, 0);
      __builtin_amdgcn_sched_group_barrier(0x002, 3, 0);
    }
    __builtin_amdgcn_sched_barrier(0);
    products(1);
  }
  __syncthreads();                                         // every wave is done with the ring before the epilogue reuses it

  // ---- epilogue (gemm_ln_f32_dma.hip).  C/D layout of the 32x32 MFMA: col = lane&31, row = (reg&3) + 8*(reg>>2) + 4*(lane>>5).
  constexpr int EP_LD = 36;
  float* ep = reinterpret_cast<float*>(smem) + wave * (32 * EP_LD);
  float* stats = reinterpret_cast<float*>(smem) + NW * (32 * EP_LD);     // [WMW][WNW][64 rows][sum, sumsq]
  const int er = lane >> 3, ec = (lane & 7) * 4;
  const __amdgpu_buffer_rsrc_t c_rsrc = __builtin_amdgcn_make_buffer_rsrc(
      C, 0, (int)(((size_t)(M - 1) * ldc + BN) * sizeof(float)), 0x00020000);
  const __amdgpu_buffer_rsrc_t s_rsrc = __builtin_amdgcn_make_buffer_rsrc(
      const_cast<float*>(shortcut), 0, (int)(((size_t)(M - 1) * lds_sc + BN) * sizeof(float)), 0x00020000);
  constexpr float INV_C = 1.0f / BN;
#pragma unroll
  for (int i = 0; i < 2; ++i) {
    f32x4 y[3][4];
    float s[4] = {0.f, 0.f, 0.f, 0.f}, q[4] = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int j = 0; j < 3; ++j) {
      const int col = wn * 96 + j * 32 + ec;
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
      const int col = wn * 96 + j * 32 + ec;
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
