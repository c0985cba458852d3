// The hand-scheduled pieces that the bf16 GEMM kernels share (gemm_bf16.hip, gemm_ln_bf16.hip, gemm_ws_bf16.hip), one definition
// each: the swizzled 128-byte-row LDS image, the fragment reads + MFMAs of one K-step, the register-staged BK = 64 main loop, the
// LDS-DMA addressing of the ring kernels, and the 16-B row-segment traffic of the epilogue patches.  (The 64-byte-row image
// `kswz64`, `wait_vmcnt<N>` and the bf16 typedefs are in common.h: the attention and fused-MLP kernels use them too.)
// Every piece is __forceinline__ and takes the caller's wave / lane / lc / lg: the persistent LayerNorm kernel counts its
// vector-memory queue by hand, and a second derivation of `wave` cost the fp32 loop a spill (profiles/gemm_f32_shared_loops_resources.md).
// The ring-offset helper and the chunk forms of the patch helpers are ONE piece per call, their loops stay with the caller: with
// the loop inside the helper the ring kernels were allocated 6-11 more VGPRs (profiles/gemm_bf16_shared_resources.md).
// The patch helpers serve the LayerNorm kernels; the plain kernels' own patch traffic
// and the ring offsets of gemm_tn_bf16_glds_kernel stay in place, where the helpers measured slower (profiles/gemm_bf16_shared_speed.md).
#pragma once
#include "common.h"

namespace pangu_bf16 {

// LDS image [row][64 bf16] (128-B rows), 16-B chunk index XOR-swizzled with (row>>1)&7: conflict-free for the ds_read_b128 lane
// groups (each group holds 16 distinct rows with chunks c / c^1) and for the staging writes.  Byte offset.
__device__ inline int swz(int row, int chunk) { return row * 128 + ((chunk ^ ((row >> 1) & 7)) << 4); }

// four bf16 (two packed pairs, low half first) -> four floats
__device__ __forceinline__ f32x4 unpack_bf16x4(u32x2 p) {
  return f32x4{__builtin_bit_cast(float, p[0] << 16), __builtin_bit_cast(float, p[0] & 0xFFFF0000u),
               __builtin_bit_cast(float, p[1] << 16), __builtin_bit_cast(float, p[1] & 0xFFFF0000u)};
}
__device__ __forceinline__ u32x2 pack_bf16x4(f32x4 v) { return u32x2{pack_bf16x2(v[0], v[1]), pack_bf16x2(v[2], v[3])}; }

// One K-step of DBK channels: acc[i][j] += A rows a_row0 + 16i .. +15 x W rows w_row0 + 16j .. +15, from the LDS images As / Ws
// (DBK = 32: 64-byte rows, kswz64; DBK = 64: 128-byte rows, swz, two half-steps that share the fragment registers).
// v_mfma_f32_16x16x32_bf16 with SWAPPED operands (W fragment as A, activation fragment as B): lane (lg, lc) of acc[i][j] holds
// 4 consecutive output COLUMNS 16j + 4lg .. +3 of row 16i + lc.
template <int NI, int NJ, int DBK>
__device__ __forceinline__ void bf16_mfma_kstep(const unsigned char* As, const unsigned char* Ws, int a_row0, int w_row0, int lc,
                                                int lg, f32x4 (&acc)[NI][NJ]) {
#pragma unroll
  for (int kk = 0; kk < DBK / 32; ++kk) {
    bf16x8 fa[NI], fw[NJ];
#pragma unroll
    for (int i = 0; i < NI; ++i) {
      const int row = a_row0 + i * 16 + lc;
      fa[i] = *reinterpret_cast<const bf16x8*>(As + (DBK == 32 ? kswz64(row, lg) : swz(row, kk * 4 + lg)));
    }
#pragma unroll
    for (int j = 0; j < NJ; ++j) {
      const int row = w_row0 + j * 16 + lc;
      fw[j] = *reinterpret_cast<const bf16x8*>(Ws + (DBK == 32 ? kswz64(row, lg) : swz(row, kk * 4 + lg)));
    }
#pragma unroll
    for (int i = 0; i < NI; ++i)
#pragma unroll
      for (int j = 0; j < NJ; ++j)
        acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(fw[j], fa[i], acc[i][j], 0, 0, 0);   // D[n][m]
  }
}

// The register-staged main loop: acc = A[m0 .. m0+127, :] @ W[n0 .. n0+BN-1, :]^T over all of K (K % 8 == 0) for a workgroup of
// 2 x WNW waves with wave tiles of 64 x 16 NJ (BN = 16 NJ WNW, wave = wm * WNW + wn).  BK = 64; staging is global_load_dwordx4 ->
// registers -> ds_write_b128 one K-step ahead into a double-buffered LDS image of (128 + BN) swizzled 128-byte rows per stage.
// A rows past M and W rows past N are clamped to the last valid row (their products are never stored); a caller whose tile spans
// the whole of W passes N = BN, and the clamp folds away.  Ends behind a barrier: the caller's epilogue may reuse smem.
template <int WNW, int NJ>
__device__ __forceinline__ void bf16_staged_main_loop(unsigned char* smem, const u16* __restrict__ A, int lda,
                                                      const u16* __restrict__ W, int M, int N, int K, int m0, int n0, int tid,
                                                      int wave, int lc, int lg, f32x4 (&acc)[4][NJ]) {
  constexpr int BM = 128, BK = 64;
  constexpr int NT = 128 * WNW;                            // threads
  constexpr int BN = 16 * NJ * WNW;
  constexpr int STAGE = (BM + BN) * 128;                   // bytes per LDS stage
  const int wm = wave / WNW, wn = wave % WNW;

  // staging: (BM + BN) rows x 8 chunks of 16 B; chunk id f = tid + NT*i -> row f>>3, chunk f&7
  constexpr int NCH = (BM + BN) * 8 / NT;                  // 16-B chunks staged per thread and K-step
  const u16* src[NCH];
  int dst[NCH];
  const int kchunk = tid & 7;
#pragma unroll
  for (int i = 0; i < NCH; ++i) {
    const int row = (tid >> 3) + (NT / 8) * i;              // 0 .. BM+BN-1
    if (row < BM) {
      int r = m0 + row;
      r = r < M ? r : M - 1;
      src[i] = A + (size_t)r * lda + kchunk * 8;
    } else {
      int r = n0 + row - BM;
      r = r < N ? r : N - 1;
      src[i] = W + (size_t)r * K + kchunk * 8;
    }
    dst[i] = (row < BM ? swz(row, kchunk) : BM * 128 + swz(row - BM, kchunk));
  }
  const int KT = (K + BK - 1) / BK;
  u32x4 stg[NCH];
  auto fetch = [&](int kt) {
    const bool in = kt * BK + kchunk * 8 < K;              // K % 8 == 0: a chunk is entirely inside or outside
#pragma unroll
    for (int i = 0; i < NCH; ++i)
      stg[i] = in ? *reinterpret_cast<const u32x4*>(src[i] + (size_t)kt * BK) : u32x4{0u, 0u, 0u, 0u};
  };
  auto stash = [&](int buf) {
#pragma unroll
    for (int i = 0; i < NCH; ++i) *reinterpret_cast<u32x4*>(smem + buf * STAGE + dst[i]) = stg[i];
  };

#pragma unroll
  for (int i = 0; i < 4; ++i)
#pragma unroll
    for (int j = 0; j < NJ; ++j) acc[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};

  fetch(0);
  stash(0);
  __syncthreads();
  for (int kt = 0; kt < KT; ++kt) {
    const bool more = kt + 1 < KT;
    if (more) fetch(kt + 1);
    const unsigned char* As = smem + (kt & 1) * STAGE;
    bf16_mfma_kstep<4, NJ, BK>(As, As + BM * 128, wm * 64, wn * 16 * NJ, lc, lg, acc);
    if (more) stash((kt + 1) & 1);
    __syncthreads();
  }
}

// ---- LDS-DMA operand ring (buffer_load_dwordx4 ... lds: no staging VGPRs, no ds_write pass) -----------------------------------------
// A ring slot holds TBM rows of A, then the rows of W, DBK channels (DBK * 2 bytes) per row.  An LDS-DMA wave-instruction writes 1 KB
// linearly (RPI = 1024 / row bytes rows), so the bank swizzle is applied on the SOURCE side: the lane that fills physical chunk p
// of row r fetches logical chunk p ^ F(r) (F of kswz64 for 64-byte rows, of swz for 128-byte rows).  DMA instruction
// q = i * NW + wave (i < LPS) fills ring rows RPI q .. RPI q + RPI - 1; this lane fills (row RPI q + lane / CH, physical chunk
// lane % CH).  The offset of piece i = the lane's byte offset into A (rows < TBM, from row a_row0) or W (from row w_row0).  Rows >= M / >= N fall
// outside the descriptor's range and arrive as zeros.
template <int NW, int TBM, int DBK>
__device__ __forceinline__ unsigned bf16_dma_offset(int i, int wave, int lane, int a_row0, int w_row0, int lda, int K) {
  constexpr int RPI = 1024 / (DBK * 2), CH = DBK / 8;
  const int row = RPI * (i * NW + wave) + lane / CH;
  const int f = DBK == 32 ? ((0x78 >> (((row >> 2) & 3) * 2)) & 3) : ((row >> 1) & 7);
  const int c = (lane % CH) ^ f;                             // logical chunk this physical slot must receive
  return row < TBM ? ((unsigned)(a_row0 + row) * (unsigned)lda + c * 8) * 2u : ((unsigned)(w_row0 + row - TBM) * (unsigned)K + c * 8) * 2u;
}

// This wave's LPS pieces of K-step kt into ring slot `slot`, in the order i = 0 .. LPS-1 (the callers' counted waits rely on it).
// a_base = byte offset of the tile's first A row where voff is tile-relative: it is added to the VECTOR offset -- the descriptor's
// range check sees vector + immediate offsets only, and rows >= M must arrive as zeros.
template <int LPS, int NW, int TBM, int DBK>
__device__ __forceinline__ void bf16_dma_issue(unsigned char* slot, __amdgpu_buffer_rsrc_t a_rsrc, __amdgpu_buffer_rsrc_t w_rsrc,
                                               const unsigned (&voff)[LPS], unsigned a_base, int kt, int wave) {
  constexpr int RPI = 1024 / (DBK * 2);
#pragma unroll
  for (int i = 0; i < LPS; ++i) {
    const int q = i * NW + wave;
    auto dst = (__attribute__((address_space(3))) void*)(slot + q * 1024);
    if (RPI * q < TBM) __builtin_amdgcn_raw_ptr_buffer_load_lds(a_rsrc, dst, 16, (int)(voff[i] + a_base), kt * DBK * 2, 0, 0);
    else __builtin_amdgcn_raw_ptr_buffer_load_lds(w_rsrc, dst, 16, (int)voff[i], kt * DBK * 2, 0, 0);
  }
}

// ---- epilogue patches --------------------------------------------------------------------------------------------------------------
// A wave's output leaves through a bf16 patch in LDS of CPR 16-B chunks per row (row pitch 16 CPR + 16 bytes), written as 8-B
// packed quads in the MFMA layout and read back as whole 16-B row segments.  Chunk f = lane + 64 it of a row group is
// (row f / CPR, chunk f % CPR); it belongs to global row grow0 + row, columns col0 + 8 ch .. +7 of a matrix of leading dimension ld.
// Rows >= M are dropped (stores) or arrive as zeros (loads) by the descriptor's range check.  There is NO column check: these
// serve the LayerNorm kernels, whose tile IS the row (N == BN).  The plain kernels, whose tile may reach past column N, route such
// chunks to offset 0xFFFFFFFF in their own loops.
__device__ __forceinline__ unsigned patch_chunk_offset(unsigned grow, unsigned ld, int col) { return (grow * ld + (unsigned)col) * 2u; }

// 16-B chunk `it` (of CPR per lane) of a 64-row patch from global memory, coalesced
template <int CPR>
__device__ __forceinline__ u32x4 patch_load_chunk(__amdgpu_buffer_rsrc_t rsrc, int grow0, int ld, int col0, int lane, int it) {
  const int f = lane + 64 * it, row = f / CPR, ch = f - row * CPR;
  return __builtin_amdgcn_raw_buffer_load_b128(rsrc, (int)patch_chunk_offset((unsigned)(grow0 + row), (unsigned)ld, col0 + ch * 8), 0, 0);
}

// stage a [64][8 CPR] bf16 patch from global memory into LDS with coalesced 16-B loads
template <int CPR>
__device__ __forceinline__ void patch_stage_rows(unsigned char* patch, __amdgpu_buffer_rsrc_t rsrc, int grow0, int ld, int col0, int lane) {
#pragma unroll
  for (int it = 0; it < CPR; ++it) {
    const int f = lane + 64 * it, row = f / CPR, ch = f - row * CPR;
    *reinterpret_cast<u32x4*>(patch + row * (16 * CPR + 16) + ch * 16) = patch_load_chunk<CPR>(rsrc, grow0, ld, col0, lane, it);
  }
}

// 16-B chunk `it` of a 16-row patch group (`patch` = its first row) read back and buffer-stored; CACHE = the store's cache policy
template <int CPR, int CACHE>
__device__ __forceinline__ void patch_store_chunk(const unsigned char* patch, __amdgpu_buffer_rsrc_t rsrc, int grow0, int ld, int col0,
                                                  int lane, int it) {
  const int f = lane + 64 * it, row = f / CPR, ch = f - row * CPR;
  if ((16 * CPR) % 64 == 0 || f < 16 * CPR) {
    const u32x4 v = *reinterpret_cast<const u32x4*>(patch + row * (16 * CPR + 16) + ch * 16);
    __builtin_amdgcn_raw_buffer_store_b128(v, rsrc, (int)patch_chunk_offset((unsigned)(grow0 + row), (unsigned)ld, col0 + ch * 8), 0, CACHE);
  }
}

// read a 16-row patch group back as 16-B row segments and buffer-store it
template <int CPR, int CACHE>
__device__ __forceinline__ void patch_store_rows(const unsigned char* patch, __amdgpu_buffer_rsrc_t rsrc, int grow0, int ld, int col0, int lane) {
#pragma unroll
  for (int it = 0; it < (16 * CPR + 63) / 64; ++it) patch_store_chunk<CPR, CACHE>(patch, rsrc, grow0, ld, col0, lane, it);
}

}  // namespace pangu_bf16
