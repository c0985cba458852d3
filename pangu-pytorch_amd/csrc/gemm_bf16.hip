// bf16 projection GEMM for gfx950: C[M,N] = act(A[M,K] @ W[N,K]^T + bias), bf16 operands, fp32 accumulate.
//
// At this path's shapes (M = 65k..521k tokens, N,K <= 1536) a bf16 projection moves ~1 GB for ~0.15 TFLOP: it sits on
// the HBM/MFMA ridge, so the kernel is built to stream: 128 x (64*TN) tile per 256-thread workgroup (4 waves 2x2,
// wave tile 64 x 32*TN), BK = 64, two workgroups per CU (2 x 80 KB LDS) so one workgroup's barrier / epilogue hides
// under the other's MFMAs.
//   MFMA: v_mfma_f32_16x16x32_bf16 with SWAPPED operands (W fragment as A, activation fragment as B), so an
//   accumulator lane holds 4 consecutive output COLUMNS of one row: bias/GELU act on float4s and the bf16 result
//   packs to 8 bytes; the tile is then transposed through LDS and leaves as whole 16-B row segments.
//   LDS image: [row][64 bf16] (128-B rows), 16-B chunk index XOR-swizzled with (row>>1)&7: conflict-free for the
//   ds_read_b128 lane groups (each group holds 16 distinct rows with chunks c / c^1) and for the staging writes.
//   Staging: global_load_dwordx4 -> registers -> ds_write_b128 one K-step ahead (double-buffered LDS).
// The register-staged main loop, the K-step, the DMA issue and the leaf helpers are in gemm_bf16_loop.h, shared with gemm_ln_bf16.hip.
#include "gemm_bf16_loop.h"

namespace {

using namespace pangu_bf16;

constexpr int BBM = 128;

template <int TN, int ACT, bool HAS_BIAS, bool OUT_F32>
__device__ __forceinline__ void bf16_epilogue(f32x4 (&acc)[4][2 * TN], unsigned char* smem, const float* __restrict__ bias,
                                              void* __restrict__ Cv, int ldc, int M, int N, u16* __restrict__ aux, int m0,
                                              int n0, int wave, int lane, u16* __restrict__ aux2 = nullptr) {
  const int wm = wave >> 1, wn = wave & 1;
  const int lc = lane & 15, lg = lane >> 4;
  // ---- epilogue.  lane (lg, lc) of tile (i, j) holds C[m = wm*64 + 16i + lc][n = wn*32TN + 16j + 4lg + r], r = 0..3
  const int wave_n0 = n0 + wn * 32 * TN;
  const int wave_m0 = m0 + wm * 64;
  if (OUT_F32) {
    float* C = reinterpret_cast<float*>(Cv);
    const __amdgpu_buffer_rsrc_t c_rsrc = __builtin_amdgcn_make_buffer_rsrc(
        C, 0, (int)(((size_t)(M - 1) * ldc + N) * sizeof(float)), 0x00020000);
#pragma unroll
    for (int j = 0; j < 2 * TN; ++j) {
      const int col = wave_n0 + j * 16 + lg * 4;
      const bool ok = col < N;
      f32x4 bv = {0.f, 0.f, 0.f, 0.f};
      if (HAS_BIAS) bv = *reinterpret_cast<const f32x4*>(bias + (ok ? col : 0));
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        f32x4 v = acc[i][j] + bv;
        if (ACT == PANGU_ACT_GELU) {
#pragma unroll
          for (int c = 0; c < 4; ++c) v[c] = gelu_erf(v[c]);
        }
        const unsigned off = ok ? ((unsigned)(wave_m0 + i * 16 + lc) * (unsigned)ldc + (unsigned)col) * 4u : 0xFFFFFFFFu;
        __builtin_amdgcn_raw_buffer_store_b128(__builtin_bit_cast(u32x4, v), c_rsrc, (int)off, 0, 0);
      }
    }
    return;
  }
  // bf16 output: per-wave [64][32*TN] bf16 patch in LDS (row stride EP_LD bytes), written as 8-B packed quads,
  // read back as 16-B row segments -> buffer stores (rows >= M and columns >= N dropped by the range check)
  constexpr int ROWB = 32 * TN * 2;                        // bytes of payload per patch row
  constexpr int EP_LD = ROWB + 16;
  unsigned char* ep = smem + wave * (64 * EP_LD);
  u16* C = reinterpret_cast<u16*>(Cv);
  const __amdgpu_buffer_rsrc_t c_rsrc = __builtin_amdgcn_make_buffer_rsrc(
      C, 0, (int)(((size_t)(M - 1) * ldc + N) * sizeof(u16)), 0x00020000);
  const __amdgpu_buffer_rsrc_t x_rsrc = __builtin_amdgcn_make_buffer_rsrc(
      aux, 0, aux ? (int)((size_t)M * N * sizeof(u16)) : 0, 0x00020000);
  constexpr int CPR = ROWB / 16;                           // 16-B chunks per patch row
  const __amdgpu_buffer_rsrc_t h_rsrc = __builtin_amdgcn_make_buffer_rsrc(
      aux2, 0, ACT == PANGU_ACT_GELU_BWD_H ? (int)((size_t)M * N * sizeof(u16)) : 0, 0x00020000);
  if (ACT == PANGU_ACT_GELU_BWD || ACT == PANGU_ACT_GELU_BWD_H || ACT == PANGU_ACT_ADD) {
    // stage the saved pre-activation (or addend) patch first (coalesced 16-B loads), so gelu' can be applied in the MFMA layout
    // (in place, not patch_stage_rows / patch_store_rows of gemm_bf16_loop.h: behind a helper the compiler waits for this patch's loads in
    // two batches of four instead of one of eight and linear_gelu_bwd measured +2.8 / +5.5 %: profiles/gemm_bf16_shared_speed.md)
#pragma unroll
    for (int it = 0; it < CPR; ++it) {
      const int f = lane + 64 * it, row = f / CPR, ch = f - row * CPR;
      const int col = wave_n0 + ch * 8;
      const unsigned off = col < N ? ((unsigned)(wave_m0 + row) * (unsigned)N + (unsigned)col) * 2u : 0xFFFFFFFFu;
      *reinterpret_cast<u32x4*>(ep + row * EP_LD + ch * 16) = __builtin_amdgcn_raw_buffer_load_b128(x_rsrc, (int)off, 0, 0);
    }
  }
  // 16-row groups: finish (bias/activation/pack -> LDS) one group, then read it back as whole 16-B row segments and
  // store it, so the stores of group i overlap the activation VALU work of group i+1.
  f32x4 bv[2 * TN];
#pragma unroll
  for (int j = 0; j < 2 * TN; ++j) {
    const int col = wave_n0 + j * 16 + lg * 4;
    bv[j] = f32x4{0.f, 0.f, 0.f, 0.f};
    if (HAS_BIAS) bv[j] = *reinterpret_cast<const f32x4*>(bias + (col < N ? col : 0));
  }
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    [[maybe_unused]] u32x2 hp[2 * TN];                                      // GELU_BWD_H: h of this row group, until the patch rows are free
#pragma unroll
    for (int j = 0; j < 2 * TN; ++j) {
      const int col = wave_n0 + j * 16 + lg * 4;
      f32x4 v = acc[i][j] + bv[j];
      unsigned char* slot = ep + (i * 16 + lc) * EP_LD + (j * 16 + lg * 4) * 2;
      if (ACT == PANGU_ACT_GELU_BWD) {
        const f32x4 x = unpack_bf16x4(*reinterpret_cast<const u32x2*>(slot));
#pragma unroll
        for (int c = 0; c < 4; ++c) v[c] *= gelu_erf_grad_lp(x[c]);
      }
      if (ACT == PANGU_ACT_GELU_BWD_H) {
        // gelu'(x) = Phi(x) + x phi(x) and h = gelu(x) = x Phi(x) share Phi
        const f32x4 x = unpack_bf16x4(*reinterpret_cast<const u32x2*>(slot));
        f32x4 hh;
#pragma unroll
        for (int c = 0; c < 4; ++c) {
          const float phi_c = 0.5f * (1.0f + erf_poly(x[c] * 0.70710678118654752440f));
          hh[c] = x[c] * phi_c;
          v[c] *= phi_c + x[c] * 0.3989422804014327f * __expf(-0.5f * x[c] * x[c]);
        }
        hp[j] = pack_bf16x4(hh);
      }
      if (ACT == PANGU_ACT_ADD) v += unpack_bf16x4(*reinterpret_cast<const u32x2*>(slot));
      if (ACT == PANGU_ACT_GELU) {
        if (aux) {                                          // pre-activation out (rounded to bf16, as it will be re-read)
          const unsigned xo = col < N ? ((unsigned)(wave_m0 + i * 16 + lc) * (unsigned)N + (unsigned)col) * 2u : 0xFFFFFFFFu;
          __builtin_amdgcn_raw_buffer_store_b64(pack_bf16x4(v), x_rsrc, (int)xo, 0, 0);
        }
        v = gelu_erf_lp4(v);
      }
      *reinterpret_cast<u32x2*>(slot) = pack_bf16x4(v);
    }
    // read back rows 16i .. 16i+15 of the patch: 16 * CPR chunks of 16 B
#pragma unroll
    for (int it = 0; it < (16 * CPR + 63) / 64; ++it) {
      const int f = lane + 64 * it;
      const int row = i * 16 + f / CPR, ch = f % CPR;
      const int col = wave_n0 + ch * 8;
      if (f < 16 * CPR) {
        const u32x4 v = *reinterpret_cast<const u32x4*>(ep + row * EP_LD + ch * 16);
        const unsigned off = col < N ? ((unsigned)(wave_m0 + row) * (unsigned)ldc + (unsigned)col) * 2u : 0xFFFFFFFFu;
        __builtin_amdgcn_raw_buffer_store_b128(v, c_rsrc, (int)off, 0, 2);
      }
    }
    // h through the same patch rows: whole 16-B row segments instead of 8-B pieces straight from the MFMA layout (measured
    // 0.57 vs 0.67 ms at C = 192, 0.36 vs 0.41 at C = 384)
    if (ACT == PANGU_ACT_GELU_BWD_H) {
#pragma unroll
      for (int j = 0; j < 2 * TN; ++j)
        *reinterpret_cast<u32x2*>(ep + (i * 16 + lc) * EP_LD + (j * 16 + lg * 4) * 2) = hp[j];
      // (in place like the store of C above: behind patch_store_rows this path came out 27 instructions longer)
#pragma unroll
      for (int it = 0; it < (16 * CPR + 63) / 64; ++it) {
        const int f = lane + 64 * it;
        const int row = i * 16 + f / CPR, ch = f % CPR;
        const int col = wave_n0 + ch * 8;
        if (f < 16 * CPR) {
          const u32x4 v = *reinterpret_cast<const u32x4*>(ep + row * EP_LD + ch * 16);
          const unsigned off = col < N ? ((unsigned)(wave_m0 + row) * (unsigned)N + (unsigned)col) * 2u : 0xFFFFFFFFu;
          __builtin_amdgcn_raw_buffer_store_b128(v, h_rsrc, (int)off, 0, 0);
        }
      }
    }
  }
}

template <int TN, int ACT, bool HAS_BIAS, bool OUT_F32>
__global__ __launch_bounds__(256, 2) void gemm_tn_bf16_kernel(const u16* __restrict__ A, int lda,
                                                              const u16* __restrict__ W, const float* __restrict__ bias,
                                                              void* __restrict__ Cv, int ldc, int M, int N, int K,
                                                              int m_tiles, int n_tiles, u16* __restrict__ aux, u16* __restrict__ aux2) {
  constexpr int BN = 64 * TN;
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];

  const int b = blockIdx.x;
  const int xcd = b & 7, local = b >> 3;
  const int m_tile = (local / n_tiles) * 8 + xcd;
  const int n_tile = local % n_tiles;
  if (m_tile >= m_tiles) return;
  const int m0 = m_tile * BBM, n0 = n_tile * BN;

  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int lc = lane & 15, lg = lane >> 4;

  f32x4 acc[4][2 * TN];                                    // [m tile 16][n tile 16], lane: 4 consecutive n of row m=lc
  bf16_staged_main_loop<2, 2 * TN>(smem, A, lda, W, M, N, K, m0, n0, tid, wave, lc, lg, acc);
  bf16_epilogue<TN, ACT, HAS_BIAS, OUT_F32>(acc, smem, bias, Cv, ldc, M, N, aux, m0, n0, wave, lane, aux2);
}

// ---- direct-to-LDS variant -------------------------------------------------------------------------------------------
// Same tile and fragment scheme, but the operands travel HBM/L2 -> LDS with buffer_load_dwordx4 ... lds (no staging VGPRs,
// no ds_write pass; addressing and source-side swizzle: gemm_bf16_loop.h), BK = 32 and a ring of TWO slots (40 KB ring, 53 KB
// with the epilogue patches: THREE workgroups per CU at <= 168 VGPRs -- there are no staging registers), loads one K-step
// ahead of the MFMAs behind s_waitcnt vmcnt(0) and ONE raw s_barrier per step.  Rows >= M / >= N fall outside the
// descriptor's range and arrive as zeros.
// (A ring of FOUR slots -- 4 x 20 KB, two workgroups per CU, loads three K-steps ahead behind counted vmcnt(LPS), vmcnt(2 LPS) --
// measured equal to register staging everywhere: removed, and the ring-depth template parameter with it.)
constexpr int GBK = 32;

template <int TN, int ACT, bool HAS_BIAS, bool OUT_F32>
__global__ __launch_bounds__(256, 3) void gemm_tn_bf16_glds_kernel(const u16* __restrict__ A, int lda,
                                                                   const u16* __restrict__ W, const float* __restrict__ bias,
                                                                   void* __restrict__ Cv, int ldc, int M, int N, int K,
                                                                   int m_tiles, int n_tiles, u16* __restrict__ aux, u16* __restrict__ aux2) {
  constexpr int BN = 64 * TN;
  constexpr int ROWS = BBM + BN;
  constexpr int STAGE = ROWS * 64;                        // bytes per ring slot
  constexpr int LPS = ROWS / 64;                          // LDS-DMA instructions per wave and stage (16 rows each)
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];

  const int b = blockIdx.x;
  const int xcd = b & 7, local = b >> 3;
  const int m_tile = (local / n_tiles) * 8 + xcd;
  const int n_tile = local % n_tiles;
  if (m_tile >= m_tiles) return;
  const int m0 = m_tile * BBM, n0 = n_tile * BN;
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int wm = wave >> 1, wn = wave & 1;
  const int lc = lane & 15, lg = lane >> 4;

  const __amdgpu_buffer_rsrc_t a_rsrc = __builtin_amdgcn_make_buffer_rsrc(
      const_cast<u16*>(A), 0, (int)(((size_t)(M - 1) * lda + K) * sizeof(u16)), 0x00020000);
  const __amdgpu_buffer_rsrc_t w_rsrc = __builtin_amdgcn_make_buffer_rsrc(
      const_cast<u16*>(W), 0, (int)((size_t)N * K * sizeof(u16)), 0x00020000);
  // instruction q = i*4 + wave (i < LPS) fills rows 16q .. 16q+15; this lane fills (row 16q + lane>>2, chunk lane&3)
  unsigned voff[LPS];
#pragma unroll
  for (int i = 0; i < LPS; ++i) {      // = bf16_dma_offset<4, BBM, GBK>, in place: the helper moves the epilogue's waits (see bf16_epilogue)
    const int row = 16 * (i * 4 + wave) + (lane >> 2);
    const int f = (0x78 >> (((row >> 2) & 3) * 2)) & 3;
    const int c = (lane & 3) ^ f;                           // logical chunk this physical slot must receive
    voff[i] = row < BBM ? ((unsigned)(m0 + row) * (unsigned)lda + c * 8) * 2u
                        : ((unsigned)(n0 + row - BBM) * (unsigned)K + c * 8) * 2u;
  }
  auto issue = [&](int kt) { bf16_dma_issue<LPS, 4, BBM, GBK>(smem + (kt & 1) * STAGE, a_rsrc, w_rsrc, voff, 0u, kt, wave); };

  f32x4 acc[4][2 * TN];
#pragma unroll
  for (int i = 0; i < 4; ++i)
#pragma unroll
    for (int j = 0; j < 2 * TN; ++j) acc[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};

  const int KT = K / GBK;                                  // >= 1: K > 0 (entry points) and K % GBK == 0 (launch_bf16)
  issue(0);
  for (int kt = 0; kt < KT; ++kt) {
    wait_vmcnt<0>();                                       // this wave's part of step kt has landed
    __builtin_amdgcn_s_barrier();                          // ... and every wave's; slot (kt+1)&1 is free
    asm volatile("" ::: "memory");
    if (kt + 1 < KT) issue(kt + 1);
    const unsigned char* As = smem + (kt & 1) * STAGE;
    bf16_mfma_kstep<4, 2 * TN, GBK>(As, As + BBM * 64, wm * 64, wn * 32 * TN, lc, lg, acc);
  }
  __syncthreads();                                         // every wave is done with the ring before the epilogue reuses it
  bf16_epilogue<TN, ACT, HAS_BIAS, OUT_F32>(acc, smem, bias, Cv, ldc, M, N, aux, m0, n0, wave, lane, aux2);
}

template <int TN, bool OUT_F32>
int launch_bf16(hipStream_t s, const u16* A, int lda, const u16* W, const float* bias, void* C, int ldc, int M, int N,
                int K, int act, u16* aux, u16* aux2 = nullptr) {
  constexpr int BN = 64 * TN;
  const int m_tiles = (M + BBM - 1) / BBM, n_tiles = (N + BN - 1) / BN;
  const int grid = ((m_tiles + 7) / 8) * 8 * n_tiles;
  // Staging pipelines, A/B-measured on MI355X at this model's shapes (tools/bench_kernels.py gemm_bf16): the LDS-DMA ring of 2
  // runs THREE workgroups per CU (no staging registers, 53 KB of LDS) and wins 7-13 % on the K = 384 / 768 shapes; for
  // K >= 1024 the register-staged BK = 64 kernel (two workgroups per CU, half the barriers) is 4 % ahead; the ring of 4
  // equals the register-staged kernel everywhere.
  const bool glds = K < 1024 && (K % GBK == 0);      // (a ring of 4 measured equal to register staging: removed)
  const size_t epi = OUT_F32 ? 0 : (size_t)4 * 64 * (32 * TN * 2 + 16);
  const size_t ring = (size_t)2 * (BBM + BN) * 64;
  const size_t shm = glds ? (ring > epi ? ring : epi) : 2 * (size_t)(BBM + BN) * 128;
  dim3 g(grid), blk(256);
#define PANGU_BGEMM(ACT, HB)                                                                                          \
  do {                                                                                                                \
    if (glds) {                                                                                                       \
      auto kern = gemm_tn_bf16_glds_kernel<TN, ACT, HB, OUT_F32>;                                                     \
      PANGU_ENSURE_DYN_LDS(kern, shm);                                                                                \
      hipLaunchKernelGGL(kern, g, blk, shm, s, A, lda, W, bias, C, ldc, M, N, K, m_tiles, n_tiles, aux, aux2);        \
      break;                                                                                                          \
    }                                                                                                                 \
    auto kern = gemm_tn_bf16_kernel<TN, ACT, HB, OUT_F32>;                                                            \
    PANGU_ENSURE_DYN_LDS(kern, shm);                                                                                  \
    hipLaunchKernelGGL(kern, g, blk, shm, s, A, lda, W, bias, C, ldc, M, N, K, m_tiles, n_tiles, aux, aux2);          \
  } while (0)
  if (act == PANGU_ACT_GELU) {
    if (bias) PANGU_BGEMM(PANGU_ACT_GELU, true); else PANGU_BGEMM(PANGU_ACT_GELU, false);
  } else if (act == PANGU_ACT_GELU_BWD_H) {
    if constexpr (OUT_F32) return PANGU_E_ARG; else PANGU_BGEMM(PANGU_ACT_GELU_BWD_H, false);
  } else if (act == PANGU_ACT_GELU_BWD) {
    if (OUT_F32) return PANGU_E_ARG;
    PANGU_BGEMM(PANGU_ACT_GELU_BWD, false);
  } else if (act == PANGU_ACT_ADD) {
    if (OUT_F32) return PANGU_E_ARG;
    if (bias) PANGU_BGEMM(PANGU_ACT_ADD, true); else PANGU_BGEMM(PANGU_ACT_ADD, false);
  } else {
    if (bias) PANGU_BGEMM(PANGU_ACT_NONE, true); else PANGU_BGEMM(PANGU_ACT_NONE, false);
  }
#undef PANGU_BGEMM
  return pangu_launch_status();
}

}  // namespace

int pangu_linear_ws_bf16(hipStream_t s, const void* A, int lda, const void* W, const float* bias, void* C, int ldc, int M,
                         int N, int K, int act, void* aux, int out_f32);      // gemm_ws_bf16.hip

extern "C" int pangu_linear_gelu_bwd_bf16(pangu_stream_t stream, const void* A, int lda, const void* W, void* dpre, int ldc,
                                          int M, int N, int K, const void* pre, void* h) {
  if (!A || !W || !dpre || !pre) return PANGU_E_NULL;
  if (M <= 0 || N <= 0 || K <= 0 || (K & 7) || (N & 7) || lda < K || ldc < N || (lda & 7) || (ldc & 7)) return PANGU_E_SHAPE;
  if (!pangu_fits_u32(M, lda, 2) || !pangu_fits_u32(M, ldc, 2) || !pangu_fits_u32(M, N, 2)) return PANGU_E_RANGE;
  hipStream_t s = (hipStream_t)stream;
  const int act = h ? PANGU_ACT_GELU_BWD_H : PANGU_ACT_GELU_BWD;
  // K <= 192: the weights-stationary kernel re-reads dm once per 192-column slice (4x at N = 768) next to the pre-activation
  // read and the dpre / h writes; measured (tools/bench_kernels.py mlp_train, MI355X) the tiled LDS-DMA kernel is 7-13 % ahead
  // on this epilogue (0.677 vs 0.729 ms with h, 0.479 vs 0.553 without), so it is the one used here
  const u16* a = (const u16*)A;
  const u16* w = (const u16*)W;
  u16* x = (u16*)const_cast<void*>(pre);
  // with h the epilogue moves three (tokens x N) tensors per tile: 128 x 128 tiles (116 VGPRs, 37 KB of patches: four workgroups
  // per CU cover its load -> gelu' -> store chain) beat 128 x 192 (three per CU): 0.53 vs 0.57 ms at C = 192, 0.34 vs 0.36 at
  // C = 384 (tools/bench_kernels.py mlp_train); without h the two are level.
  const bool tn2 = h != nullptr;
  if (tn2 && N % 128 == 0) return launch_bf16<2, false>(s, a, lda, w, nullptr, dpre, ldc, M, N, K, act, x, (u16*)h);
  if ((N % 192 == 0) || (N > 128 && N < 192)) return launch_bf16<3, false>(s, a, lda, w, nullptr, dpre, ldc, M, N, K, act, x, (u16*)h);
  if (N % 128 == 0) return launch_bf16<2, false>(s, a, lda, w, nullptr, dpre, ldc, M, N, K, act, x, (u16*)h);
  return launch_bf16<1, false>(s, a, lda, w, nullptr, dpre, ldc, M, N, K, act, x, (u16*)h);
}

extern "C" int pangu_linear_fwd_bf16(pangu_stream_t stream, const void* A, int lda, const void* W, const float* bias,
                                     void* C, int ldc, int M, int N, int K, int act, void* aux, int out_dtype) {
  if (!A || !W || !C) return PANGU_E_NULL;
  if (M <= 0 || N <= 0 || K <= 0 || (K & 7) || (N & 7) || lda < K || ldc < N || (lda & 7) || (ldc & 3)) return PANGU_E_SHAPE;
  if (!pangu_fits_u32(M, lda, 2) || !pangu_fits_u32(M, ldc, 4)) return PANGU_E_RANGE;
  if (act != PANGU_ACT_NONE && act != PANGU_ACT_GELU && act != PANGU_ACT_GELU_BWD && act != PANGU_ACT_ADD) return PANGU_E_ARG;
  if (act == PANGU_ACT_GELU_BWD && (!aux || bias)) return PANGU_E_ARG;
  if (act == PANGU_ACT_ADD && !aux) return PANGU_E_ARG;
  if (out_dtype != PANGU_BF16 && out_dtype != PANGU_F32) return PANGU_E_DTYPE;
  if (out_dtype == PANGU_BF16 && (ldc & 7)) return PANGU_E_SHAPE;
  hipStream_t s = (hipStream_t)stream;
  // K <= 192: weights-stationary barrier-free kernel (gemm_ws_bf16.hip; not for the GELU-backward epilogue: the tiled LDS-DMA
  // kernel is 7-13 % ahead there, see pangu_linear_gelu_bwd_bf16)
  if (M >= 4096 && act != PANGU_ACT_ADD && act != PANGU_ACT_GELU_BWD) {
    const int rc = pangu_linear_ws_bf16(s, A, lda, W, bias, C, ldc, M, N, K, act, aux, out_dtype == PANGU_F32);
    if (rc != PANGU_E_SHAPE) return rc;
  }
  const u16* a = (const u16*)A;
  const u16* w = (const u16*)W;
  u16* x = (u16*)aux;
  const bool wide = (N % 192 == 0) || (N > 128 && N < 192);
  if (out_dtype == PANGU_F32) {
    if (wide) return launch_bf16<3, true>(s, a, lda, w, bias, C, ldc, M, N, K, act, x);
    if (N % 128 == 0) return launch_bf16<2, true>(s, a, lda, w, bias, C, ldc, M, N, K, act, x);
    return launch_bf16<1, true>(s, a, lda, w, bias, C, ldc, M, N, K, act, x);
  }
  if (wide) return launch_bf16<3, false>(s, a, lda, w, bias, C, ldc, M, N, K, act, x);
  if (N % 128 == 0) return launch_bf16<2, false>(s, a, lda, w, bias, C, ldc, M, N, K, act, x);
  return launch_bf16<1, false>(s, a, lda, w, bias, C, ldc, M, N, K, act, x);
}
