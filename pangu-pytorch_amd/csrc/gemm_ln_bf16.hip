// bf16 projection GEMM with the post-norm residual fused into its epilogue (inference path), gfx950:
//   out[M,N] = shortcut[M,N] + LayerNorm(A[M,K] @ W[N,K]^T + bias) * gamma + beta        (reference layers.py:250-251)
// for N = 192 or 384 (the model's two widths): the workgroup tile is 128 rows x the WHOLE row (wave grid 2 x WNW, wave
// tile 64 x 96, WNW = N / 96), so the row statistics never leave the workgroup.  Same operand staging, LDS swizzle and
// swapped-operand MFMA layout as gemm_bf16.hip (a lane owns 4 consecutive output columns of one row).
// Epilogue: the shortcut patch is staged in LDS with coalesced 16-B loads; each wave reduces (sum, sum of squares) of its
// 96 columns in fp32 straight from the accumulators (in-lane + 2 shuffles), the WNW partials of a row meet in a 4-KB LDS
// table behind ONE barrier, then normalise / gamma / beta / residual run in the MFMA layout and the rows leave as 16-B
// segments.  Saves the branch's HBM round trip (write y, read y, read shortcut, write out -> read shortcut, write out):
// the standalone LN-residual kernel is HBM-bound at ~5 TB/s and was 12 % of the bf16 forward.
// The statistics are taken on the fp32 accumulators, i.e. BEFORE the bf16 rounding the unfused path applies to y.
// The main loop / ring addressing (gemm_bf16_loop.h) and the LayerNorm pieces (ln_epilogue_bf16.h) are shared by the two kernels here.
#include "ln_epilogue_bf16.h"

namespace {

using namespace pangu_bf16;

constexpr int LBM = 128;

template <int WNW>
__global__ __launch_bounds__(128 * WNW, 2) void gemm_ln_residual_bf16_kernel(
    const u16* __restrict__ A, int lda, const u16* __restrict__ W, const float* __restrict__ bias,
    const u16* __restrict__ shortcut, const float* __restrict__ gamma, const float* __restrict__ beta, u16* __restrict__ out,
    int ldo, int M, int K) {
  constexpr int BN = 96 * WNW;                             // = N
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];

  const int m0 = blockIdx.x * LBM;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int wm = wave / WNW, wn = wave % WNW;
  const int lc = lane & 15, lg = lane >> 4;

  f32x4 acc[4][6];                                         // [m tile 16][n tile 16], lane: 4 consecutive n of row m = lc
  bf16_staged_main_loop<WNW, 6>(smem, A, lda, W, M, BN, K, m0, 0, tid, wave, lc, lg, acc);      // N = BN: no W row is clamped

  // ---- epilogue.  lane (lg, lc) of tile (i, j) holds y[m = wm*64 + 16i + lc][n = wn*96 + 16j + 4lg + r], r = 0..3
  constexpr int EP_LD = 96 * 2 + 16;                       // bytes per patch row
  constexpr int CPR = 12;                                  // 16-B chunks per patch row
  unsigned char* ep = smem + wave * (64 * EP_LD);
  float* stats = reinterpret_cast<float*>(smem + 2 * WNW * 64 * EP_LD);      // [2 wm][WNW][64 rows][sum, sumsq]
  const int wave_n0 = wn * 96, wave_m0 = m0 + wm * 64;
  const __amdgpu_buffer_rsrc_t o_rsrc = __builtin_amdgcn_make_buffer_rsrc(
      out, 0, (int)(((size_t)(M - 1) * ldo + BN) * sizeof(u16)), 0x00020000);
  const __amdgpu_buffer_rsrc_t s_rsrc = __builtin_amdgcn_make_buffer_rsrc(
      const_cast<u16*>(shortcut), 0, (int)((size_t)M * BN * sizeof(u16)), 0x00020000);
  // shortcut patch [64][96] -> LDS (rows >= M arrive as zeros)
  patch_stage_rows<CPR>(ep, s_rsrc, wave_m0, BN, wave_n0, lane);
  // y = acc + bias (kept in acc), per-row partial statistics of this wave's 96 columns
#pragma unroll
  for (int j = 0; j < 6; ++j) {
    const f32x4 bv = bias ? *reinterpret_cast<const f32x4*>(bias + wave_n0 + j * 16 + lg * 4) : f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int i = 0; i < 4; ++i) acc[i][j] += bv;
  }
  ln_stats_partials<WNW>(acc, stats, wm, wn, lc, lg);
  __syncthreads();
  f32x4 gv[6], bt[6];
#pragma unroll
  for (int j = 0; j < 6; ++j) {
    gv[j] = *reinterpret_cast<const f32x4*>(gamma + wave_n0 + j * 16 + lg * 4);
    bt[j] = *reinterpret_cast<const f32x4*>(beta + wave_n0 + j * 16 + lg * 4);
  }
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    float mean, rstd;
    ln_row_stats<WNW>(stats, wm, i, lc, mean, rstd);
#pragma unroll
    for (int j = 0; j < 6; ++j) {
      u32x2* slot = reinterpret_cast<u32x2*>(ep + (i * 16 + lc) * EP_LD + (j * 16 + lg * 4) * 2);
      *slot = ln_residual_pack(acc[i][j], mean, rstd, gv[j], bt[j], *slot);
    }
    // read back rows 16i .. 16i+15 of the patch: 16 * 12 chunks of 16 B -> whole row segments
    patch_store_rows<CPR, 2>(ep + i * 16 * EP_LD, o_rsrc, wave_m0 + i * 16, ldo, wave_n0, lane);
  }
}

// ---- persistent LDS-DMA variant (round 6) ----------------------------------------------------------------------------
// The kernel above owns one 128-row tile per workgroup and stages its operands through registers one K-step ahead: with K = C the
// whole K-loop is 3-6 steps of ~770 MFMA cycles each, i.e. far shorter than one memory latency, and -- N = 384: 128 KB of LDS, ONE
// workgroup per CU -- nothing overlaps a tile's prologue, its per-step load latencies and its epilogue: 22 us per tile, 1.84x the
// HBM floor (profiles/r05_fwd_bf16_issue_table.md: 0.47 of the wave-cycles parked, MFMA busy 0.17).  Here the same tile, wave grid
// and fragment reads run in a PERSISTENT workgroup whose operand ring never drains:
//   * A and W travel L2/HBM -> LDS by LDS-DMA (buffer_load .. lds: no staging registers) in K-steps of 32 through a ring of RING
//     slots; the requests of the NEXT tile's first RING-1 steps are issued under the current tile's last K-steps, so its epilogue
//     (LayerNorm, residual, stores) runs with the next tile's operands already in flight;
//   * the tile's 128 x N shortcut patch (the other HBM stream) is requested into registers at the tile's first K-step -- 12 16-B
//     loads per thread in the layout the output rows leave in -- and is consumed by the epilogue one 16-row group at a time
//     through a 3.3-KB per-wave LDS patch (26 KB instead of the 106 KB the tile-at-once epilogue needs);
//   * every wait is a COUNTED s_waitcnt vmcnt(n): the in-order queue holds, per thread, LPS DMA requests per step, 12 shortcut
//     loads and 12 output stores per tile at known positions.
// LDS: RING x (128 + N) x 64 B ring + 2 WNW x 3328 B patches + 4 KB statistics (N = 384, RING = 3: 127 KB, one 8-wave workgroup
// per CU; N = 192, RING = 3: 75 KB, two 4-wave workgroups per CU).
// DBK = channels per K-step: 32 (64-byte ring rows, swizzle kswz64) or 64 (128-byte rows, swizzle swz: half the barriers, the second
// half-step's fragment reads can overlap the first's MFMAs; ring of 2 only -- 2 x 64 KB at N = 384).
// WM = wave rows of 64 tokens: the tile is 64 WM x N (2: 128 rows, the N = 384 form; 4: 256 rows x 192 columns -- one 8-wave workgroup
// per CU at N = 192 as well, the W panel re-streamed half as often).
template <int WNW, int RING, int DBK = 32, int WM = 2>
__global__ __launch_bounds__(64 * WM * WNW, 2) void gemm_ln_residual_bf16_dma_kernel(
    const u16* __restrict__ A, int lda, const u16* __restrict__ W, const float* __restrict__ bias,
    const u16* __restrict__ shortcut, const float* __restrict__ gamma, const float* __restrict__ beta, u16* __restrict__ out,
    int ldo, int M, int K, int m_tiles) {
  static_assert((DBK == 32 && RING == 3) || (DBK == 64 && RING == 2), "ring of three K-steps of 32, or two of 64");
  constexpr int ROWB = DBK * 2;                            // bytes per ring row
  constexpr int RPI = 1024 / ROWB;                         // ring rows per LDS-DMA instruction (1 KB)
  constexpr int NW = WM * WNW;                             // waves
  constexpr int TBM = 64 * WM;                             // token rows per tile
  constexpr int BN = 96 * WNW;                             // = N
  constexpr int ROWS = TBM + BN;
  constexpr int STAGE = ROWS * ROWB;                       // bytes per ring slot
  constexpr int LPS = ROWS / (RPI * NW);                   // LDS-DMA instructions per wave and K-step (RPI rows each)
  static_assert(ROWS % (RPI * NW) == 0, "whole DMA instructions per wave");
  constexpr int EP_LD = 96 * 2 + 16;                       // bytes per patch row
  constexpr int CPR = 12;                                  // 16-B chunks per patch row
  constexpr int NS = 12;                                   // shortcut loads = output stores per thread and tile
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  unsigned char* ep = smem + RING * STAGE + (threadIdx.x >> 6) * (16 * EP_LD);
  // the statistics table [WM][WNW][64 rows][sum, sumsq] (4 KB) ALIASES the patches: it is dead (every wave has taken
  // its rows' mean / rstd into registers, second barrier) before the first patch is written -- what lets a ring of four fit
  float* stats = reinterpret_cast<float*>(smem + RING * STAGE);
  static_assert(WM * WNW * 64 * 2 * 4 <= NW * 16 * (96 * 2 + 16), "statistics fit in the patch area");
  float* prm = reinterpret_cast<float*>(smem + RING * STAGE + NW * 16 * EP_LD);      // [bias | gamma | beta][N]: resident

  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int wm = wave / WNW, wn = wave % WNW;
  const int lc = lane & 15, lg = lane >> 4;
  const int wave_n0 = wn * 96;

  const __amdgpu_buffer_rsrc_t a_rsrc = __builtin_amdgcn_make_buffer_rsrc(
      const_cast<u16*>(A), 0, (int)(((size_t)(M - 1) * lda + K) * sizeof(u16)), 0x00020000);
  const __amdgpu_buffer_rsrc_t w_rsrc = __builtin_amdgcn_make_buffer_rsrc(
      const_cast<u16*>(W), 0, (int)((size_t)BN * K * sizeof(u16)), 0x00020000);
  const __amdgpu_buffer_rsrc_t o_rsrc = __builtin_amdgcn_make_buffer_rsrc(
      out, 0, (int)(((size_t)(M - 1) * ldo + BN) * sizeof(u16)), 0x00020000);
  const __amdgpu_buffer_rsrc_t s_rsrc = __builtin_amdgcn_make_buffer_rsrc(
      const_cast<u16*>(shortcut), 0, (int)((size_t)M * BN * sizeof(u16)), 0x00020000);

  // ring addressing (gemm_bf16_loop.h): rows < TBM are A, TILE-relative -- the tile's byte offset is added to the vector offset at
  // issue time -- rows >= TBM are W
  unsigned voff[LPS];
#pragma unroll
  for (int i = 0; i < LPS; ++i) voff[i] = bf16_dma_offset<NW, TBM, DBK>(i, wave, lane, 0, 0, lda, K);
  const int KT = K / DBK;
  // global step g = it * KT + kt of this workgroup's it-th tile
  auto issue = [&](int g, int tile, int kt) {
    const unsigned a_base = (unsigned)tile * (unsigned)(TBM * 2) * (unsigned)lda;      // < 2^32: checked by the launcher
    bf16_dma_issue<LPS, NW, TBM, DBK>(smem + (g % RING) * STAGE, a_rsrc, w_rsrc, voff, a_base, kt, wave);
  };

  for (int c = tid; c < BN; c += 64 * NW) {
    prm[c] = bias ? bias[c] : 0.f;
    prm[BN + c] = gamma[c];
    prm[2 * BN + c] = beta[c];
  }
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");            // the counted waits below see DMA / shortcut / store traffic only
  __syncthreads();

  int tile = blockIdx.x;
  if (tile >= m_tiles) return;
#pragma unroll
  for (int p0 = 0; p0 < RING - 1; ++p0) issue(p0, tile, p0);          // KT >= RING - 1: checked by the launcher
  bool first = true;
  int g = 0;
  for (; tile < m_tiles; tile += gridDim.x) {
    const int next = tile + gridDim.x;
    const bool has_next = next < m_tiles;
    const int m0 = tile * TBM, wave_m0 = m0 + wm * 64;
    f32x4 acc[4][6];
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
      for (int j = 0; j < 6; ++j) acc[i][j] = *reinterpret_cast<const f32x4*>(prm + wave_n0 + j * 16 + lg * 4);
    u32x4 sc[NS];
    for (int kt = 0; kt < KT; ++kt, ++g) {
      // In-order queue of this thread (oldest first) within a tile: DMA(0 .. RING-2) were issued under the PREVIOUS tile's last
      // K-steps, then that tile's NS output stores, then at step k: DMA(k + RING - 1), and at step 0 also the NS shortcut loads.
      // Step k needs DMA(k); NEWER than it (allowed to stay in flight) are
      //   the DMA groups k+1 .. k+RING-2 that exist, the stores iff k <= RING-2 (not in this workgroup's first tile), and the
      //   shortcut loads iff 1 <= k <= RING-1.
      {
        int groups = RING - 2;
        if (!has_next && KT - 1 - kt < groups) groups = KT - 1 - kt;
        const int extra = ((kt <= RING - 2 && !first) ? 1 : 0) + ((kt >= 1 && kt <= RING - 1) ? 1 : 0);
        const int code = groups * 3 + extra;                 // (groups 0..2) x (extra 0..2)
        if (code == 0) wait_vmcnt<0>();
        else if (code == 1) wait_vmcnt<NS>();
        else if (code == 2) wait_vmcnt<2 * NS>();
        else if (code == 3) wait_vmcnt<LPS>();
        else if (code == 4) wait_vmcnt<LPS + NS>();
        else if (code == 5) wait_vmcnt<LPS + 2 * NS>();
        else if (code == 6) wait_vmcnt<2 * LPS>();
        else if (code == 7) wait_vmcnt<2 * LPS + NS>();
        else wait_vmcnt<2 * LPS + 2 * NS>();
      }
      asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");       // this wave's fragment reads of step g-1 have returned
      __builtin_amdgcn_sched_barrier(0);
      __builtin_amdgcn_s_barrier();                            // step g landed for every wave; slot (g-1) % RING is free
      asm volatile("" ::: "memory");
      if (kt + RING - 1 < KT) issue(g + RING - 1, tile, kt + RING - 1);
      else if (has_next) issue(g + RING - 1, next, kt + RING - 1 - KT);
      if (kt == 0) {
        // shortcut patch [64 rows][96 columns] of this wave, 16-B chunks in the order the output rows leave in (rows >= M: zeros)
#pragma unroll
        for (int it = 0; it < NS; ++it) sc[it] = patch_load_chunk<CPR>(s_rsrc, wave_m0, BN, wave_n0, lane, it);
      }
      const unsigned char* As = smem + (g % RING) * STAGE;
      bf16_mfma_kstep<4, 6, DBK>(As, As + TBM * ROWB, wm * 64, wn * 96, lc, lg, acc);
    }
    first = false;

    // ---- epilogue.  lane (lg, lc) of tile (i, j) holds y[m = wm*64 + 16i + lc][n = wn*96 + 16j + 4lg + r] (bias included)
    // (the compiler guards each group's first use of the shortcut registers with vmcnt(9..11): in the in-order queue that is a
    // wait for the OLDEST of the next tile's operand requests from the third group on -- requests issued two K-steps and half an
    // epilogue earlier; forcing the registers "landed" inside the K-loop costs a full vmcnt(0) there instead, which is worse)
    ln_stats_partials<WNW>(acc, stats, wm, wn, lc, lg);
    // (a raw barrier: __syncthreads() would also wait for the next tile's operand requests -- vmcnt(0); the statistics went
    // through LDS only, and the next tile's statistics are >= KT barriers away)
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
    __builtin_amdgcn_s_barrier();
    asm volatile("" ::: "memory");
    float mean_[4], rstd_[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) ln_row_stats<WNW>(stats, wm, i, lc, mean_[i], rstd_[i]);
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
    __builtin_amdgcn_s_barrier();                              // the table is dead: the patches may overwrite it
    asm volatile("" ::: "memory");
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const float mean = mean_[i], rstd = rstd_[i];
      // the group's shortcut rows -> patch (the previous group's read-back must have returned: same wave, LDS in order)
#pragma unroll
      for (int it = 0; it < 3; ++it) {
        const int f = lane + 64 * it, row = f / CPR, ch = f - row * CPR;
        *reinterpret_cast<u32x4*>(ep + row * EP_LD + ch * 16) = sc[3 * i + it];
      }
#pragma unroll
      for (int j = 0; j < 6; ++j) {
        u32x2* slot = reinterpret_cast<u32x2*>(ep + lc * EP_LD + (j * 16 + lg * 4) * 2);
        const u32x2 xp = *slot;
        const f32x4 gj = *reinterpret_cast<const f32x4*>(prm + BN + wave_n0 + j * 16 + lg * 4);
        const f32x4 bj = *reinterpret_cast<const f32x4*>(prm + 2 * BN + wave_n0 + j * 16 + lg * 4);
        *slot = ln_residual_pack(acc[i][j], mean, rstd, gj, bj, xp);
      }
      // (the chunk helper in a loop of this kernel's own: with the loop inside a helper -- patch_store_rows -- the compiler allocates
      // 6 more registers, and <2, 2, 64, 4> spills three of them inside the K-loop: profiles/gemm_bf16_shared_resources.md)
#pragma unroll
      for (int it = 0; it < 3; ++it) patch_store_chunk<CPR, 2>(ep, o_rsrc, wave_m0 + i * 16, ldo, wave_n0, lane, it);
    }
  }
}

template <int WNW, int RING, int DBK = 32, int WM = 2>
int launch_ln_dma(hipStream_t s, const u16* A, int lda, const u16* W, const float* bias, const u16* shortcut, const float* gamma,
                  const float* beta, u16* out, int ldo, int M, int K) {
  constexpr int BN = 96 * WNW, TBM = 64 * WM, NW = WM * WNW;
  const int m_tiles = (M + TBM - 1) / TBM;
  const size_t shm = (size_t)RING * (TBM + BN) * (DBK * 2) + (size_t)NW * 16 * (96 * 2 + 16) + (size_t)3 * BN * sizeof(float);
  auto kern = gemm_ln_residual_bf16_dma_kernel<WNW, RING, DBK, WM>;
  PANGU_ENSURE_DYN_LDS(kern, shm);
  const int per_cu = (int)(160 * 1024 / shm) < 1 ? 1 : (int)(160 * 1024 / shm);
  int grid = 256 * (per_cu > 2 ? 2 : per_cu);
  if (grid > m_tiles) grid = m_tiles;
  hipLaunchKernelGGL(kern, dim3(grid), dim3(64 * NW), shm, s, A, lda, W, bias, shortcut, gamma, beta, out, ldo, M, K, m_tiles);
  return pangu_launch_status();
}

template <int WNW>
int launch_ln(hipStream_t s, const u16* A, int lda, const u16* W, const float* bias, const u16* shortcut, const float* gamma,
              const float* beta, u16* out, int ldo, int M, int K) {
  constexpr int BN = 96 * WNW;
  const size_t stages = 2 * (size_t)(LBM + BN) * 128;
  const size_t epi = (size_t)2 * WNW * 64 * (96 * 2 + 16) + (size_t)2 * WNW * 64 * 2 * sizeof(float);
  const size_t shm = stages > epi ? stages : epi;
  auto kern = gemm_ln_residual_bf16_kernel<WNW>;
  PANGU_ENSURE_DYN_LDS(kern, shm);
  hipLaunchKernelGGL(kern, dim3((M + LBM - 1) / LBM), dim3(128 * WNW), shm, s, A, lda, W, bias, shortcut, gamma, beta, out, ldo,
                     M, K);
  return pangu_launch_status();
}

}  // namespace

extern "C" int pangu_linear_ln_residual_fwd_bf16(pangu_stream_t stream, const void* A, int lda, const void* W,
                                                 const float* bias, const void* shortcut, const float* gamma,
                                                 const float* beta, void* out, int ldo, int M, int N, int K) {
  if (!A || !W || !shortcut || !gamma || !beta || !out) return PANGU_E_NULL;
  if (M <= 0 || K <= 0 || (K & 7) || lda < K || (lda & 7) || ldo < N || (ldo & 7)) return PANGU_E_SHAPE;
  if (!pangu_fits_u32(M, lda, 2) || !pangu_fits_u32(M, ldo, 2)) return PANGU_E_RANGE;
  if (N != 192 && N != 384) return PANGU_E_SHAPE;          // the tile must span the whole row
  hipStream_t s = (hipStream_t)stream;
  // the persistent LDS-DMA kernel: K a multiple of 32 and at least three K-steps, dense A rows addressable through the scalar offset
  // N = 384: always.  N = 192: the 256-row-tile form where the K-loop is long enough to pay (K >= 384: -7 % at K = 768; at
  // K = 192 -- the forward's launch -- it measured level with the register-staged kernel, which then stays).
  const bool dma = K % 32 == 0 && K >= 96 && pangu_fits_u32(M, lda, 2) && (N == 384 || K >= 384);
  if (N == 192) {
    if (dma && K % 64 == 0 && K >= 192)      // 256 x 192 tiles, one 8-wave workgroup per CU, K-steps of 64, ring of two
      return launch_ln_dma<2, 2, 64, 4>(s, (const u16*)A, lda, (const u16*)W, bias, (const u16*)shortcut, gamma, beta, (u16*)out, ldo, M, K);
    if (dma) return launch_ln_dma<2, 3>(s, (const u16*)A, lda, (const u16*)W, bias, (const u16*)shortcut, gamma, beta, (u16*)out, ldo, M, K);
    return launch_ln<2>(s, (const u16*)A, lda, (const u16*)W, bias, (const u16*)shortcut, gamma, beta, (u16*)out, ldo, M, K);
  }
  if (dma) {
    // TWO ring slots of 64-channel K-steps (128 KB): half the barriers, and the second half-step's fragment reads overlap the first's
    // MFMAs -- -6..-9 % against three or four slots of 32-channel K-steps (96 / 128 KB; level with each other),
    // profiles/r06_gemm_ln_bf16_ab.md.  Three slots of 32 channels where K is not a multiple of 64.
    if (K % 64 == 0 && K >= 192)
      return launch_ln_dma<4, 2, 64>(s, (const u16*)A, lda, (const u16*)W, bias, (const u16*)shortcut, gamma, beta, (u16*)out, ldo, M, K);
    return launch_ln_dma<4, 3>(s, (const u16*)A, lda, (const u16*)W, bias, (const u16*)shortcut, gamma, beta, (u16*)out, ldo, M, K);
  }
  return launch_ln<4>(s, (const u16*)A, lda, (const u16*)W, bias, (const u16*)shortcut, gamma, beta, (u16*)out, ldo, M, K);
}
