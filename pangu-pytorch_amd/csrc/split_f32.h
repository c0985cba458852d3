// What the exact-split fp32 GEMMs (gemm_f32_split.hip, gemm_ln_f32_split.hip) share: the bf16 hi/mid/lo split of fp32 values, the
// layout constants of the weight image (pangu_split_weight_bf16x3) and of the LDS stage it is streamed into, and the main loop
// (one definition: the two kernels differ in their epilogues only).  The fp32 A image and its swizzle are those of the fp32-MFMA
// LDS-DMA loop (gemm_f32_dma_loop.h).
#pragma once
#include "gemm_f32_dma_loop.h"

namespace pangu_split {

using pangu_dma::BK;                             // k-step of 16: one 64-byte fp32 A row, two 8-wide bf16 k-halves

typedef short bf16x8 __attribute__((ext_vector_type(8)));

constexpr int W_ROWS = 192;                      // rows of one n-tile block of the image
constexpr int PLANE = 2 * W_ROWS * 16;           // one bf16 plane of an (n-tile, k-step) block: [k-half][row][8 bf16]
constexpr int B_BYTES = 3 * PLANE;               // 18432: hi, mid, lo
constexpr int W_PIECES = B_BYTES / 1024;         // 18 linear 1-KB LDS-DMA pieces per block

// two fp32 -> their bf16 triples, packed (low half = a): hi + mid + lo == the fp32 value, exactly
__device__ inline void split2(float a, float b, unsigned& hi, unsigned& mid, unsigned& lo) {
  const bf16x2_t h = __builtin_convertvector(f32x2_t{a, b}, bf16x2_t);
  const f32x2_t r1 = f32x2_t{a, b} - __builtin_convertvector(h, f32x2_t);
  const bf16x2_t m = __builtin_convertvector(r1, bf16x2_t);
  const f32x2_t r2 = r1 - __builtin_convertvector(m, f32x2_t);
  hi = __builtin_bit_cast(unsigned, h);
  mid = __builtin_bit_cast(unsigned, m);
  lo = __builtin_bit_cast(unsigned, __builtin_convertvector(r2, bf16x2_t));
}

__device__ inline void split8(const f32x4 c0, const f32x4 c1, bf16x8& hi, bf16x8& mid, bf16x8& lo) {
  unsigned h0, h1, h2, h3, m0, m1, m2, m3, l0, l1, l2, l3;
  split2(c0[0], c0[1], h0, m0, l0);
  split2(c0[2], c0[3], h1, m1, l1);
  split2(c1[0], c1[1], h2, m2, l2);
  split2(c1[2], c1[3], h3, m3, l3);
  hi = __builtin_bit_cast(bf16x8, u32x4{h0, h1, h2, h3});
  mid = __builtin_bit_cast(bf16x8, u32x4{m0, m1, m2, m3});
  lo = __builtin_bit_cast(bf16x8, u32x4{l0, l1, l2, l3});
}

// WMW x WNW waves, each of RB row blocks x CB column tiles of 32 x 32; NST ring stages (3: LDS-DMA two k-steps ahead; 2: one
// ahead), one barrier per step.  ROWS = true is the row-owning tiling: a wave holds ONE 32-row block and all 192 columns of an
// n-tile block (32 x 192), so every A element is split by exactly one wave; ROWS = false is the 64 x 96 wave (two row blocks, half
// an n-tile block), where the WNW waves that share rows each split them again.  A stage is the fp32 A image (BM rows of 64 B)
// followed by the NT n-tile blocks of the weight image the tile's columns span: the same image, the same LDS-DMA pieces and, per
// output element, the same six MFMAs per k-step in the same order under either tiling, so the two compute the same bits.
template <int WMW, int WNW, int NST, bool ROWS>
struct SplitTile {
  static constexpr int RB = ROWS ? 1 : 2;              // 32-row blocks per wave
  static constexpr int CB = ROWS ? 6 : 3;              // 32-column tiles per wave
  static constexpr int NW = WMW * WNW;                 // waves
  static constexpr int BM = 32 * RB * WMW;
  static constexpr int BN = 32 * CB * WNW;
  static constexpr int NT = BN / W_ROWS;               // n-tile blocks of the image per k-step
  static constexpr int A_BYTES = BM * 64;
  static constexpr int STAGE = A_BYTES + NT * B_BYTES;
  static constexpr int SMEM = NST * STAGE;
  static_assert(NST == 2 || NST == 3, "ring depth");
  static_assert(BN % W_ROWS == 0, "whole n-tile blocks");
};

// acc[i][j] += A[m0 + (wm RB + i) 32 .. +31, :] @ W[first_n_tile 192 + (wn CB + j) 32 .. +31, :]^T over all of K (K % 16 == 0), W
// given as its split image of N rows; wave = wm * WNW + wn.  smem: SplitTile::SMEM bytes.  Ends behind a barrier: every wave is
// done with the ring, the caller's epilogue may reuse it.  LEAN (ROWS only): the W fragments of three column tiles in flight
// instead of all six, 163 VGPRs instead of 198: the form that fits three workgroups per CU (<= 168).
template <int WMW, int WNW, int NST, bool ROWS, bool LEAN = false>
__device__ __forceinline__ void split_main_loop(unsigned char* smem, const float* __restrict__ A, int lda,
                                                const unsigned char* __restrict__ image, int M, int N, int K, int m0,
                                                int first_n_tile,
                                                f32x16 (&acc)[SplitTile<WMW, WNW, NST, ROWS>::RB][SplitTile<WMW, WNW, NST, ROWS>::CB]) {
  using T = SplitTile<WMW, WNW, NST, ROWS>;
  constexpr int NW = T::NW, A_BYTES = T::A_BYTES, STAGE = T::STAGE, RB = T::RB, CB = T::CB;
  constexpr int A_PIECES = A_BYTES / 1024;
  constexpr int PIECES = STAGE / 1024;             // piece q goes to wave q % NW
  constexpr int A_IT = A_PIECES / NW;              // issue rounds that are all A
  constexpr int IT = (PIECES + NW - 1) / NW;       // issue rounds; waves < REM issue IT pieces, the others IT - 1 (REM = 0: all IT)
  constexpr int REM = PIECES % NW;                 // <2, 2, 3>: 26 pieces, IT = 7, REM = 2: waves 0, 1 issue 7, waves 2, 3 issue 6
  static_assert(A_PIECES % NW == 0, "piece rounds");

  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int wm = wave / WNW, wn = wave % WNW;
  const int lr = lane & 31, lh = lane >> 5;
  const int KT = K / BK;

  const __amdgpu_buffer_rsrc_t a_rsrc = __builtin_amdgcn_make_buffer_rsrc(
      const_cast<float*>(A), 0, (int)(((size_t)(M - 1) * lda + K) * sizeof(float)), 0x00020000);
  const __amdgpu_buffer_rsrc_t w_rsrc = __builtin_amdgcn_make_buffer_rsrc(
      const_cast<unsigned char*>(image), 0, (int)((size_t)N * K * 6), 0x00020000);
  // piece q = i*NW + wave (q < PIECES).  q < A_PIECES: rows 16q .. 16q+15 of A, this lane fills (row 16q + lane>>2, physical chunk
  // lane&3), i.e. fetches logical chunk (lane&3) ^ F(row); rows >= M are out of range: zeros.  Otherwise piece p = q - A_PIECES of
  // the W part: bytes 1024 (p % 18) .. +1023 of the (n-tile first_n_tile + p / 18, k-step) block of the image, copied linearly.
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
    voff_w[i - A_IT] = (unsigned)(first_n_tile + p / W_PIECES) * (unsigned)KT * (unsigned)B_BYTES +
                       (unsigned)(p % W_PIECES) * 1024u + lane * 16;
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

#pragma unroll
  for (int i = 0; i < RB; ++i)
#pragma unroll
    for (int j = 0; j < CB; ++j)
#pragma unroll
      for (int r = 0; r < 16; ++r) acc[i][j][r] = 0.f;

  // fragment byte offsets: lane (lr, lh) owns k = 8lh .. 8lh+7 of its row: logical chunks 2lh, 2lh+1 of the fp32 A row, and
  // chunk (k-half lh, row) of each W plane of the wave's n-tile block
  int off_a[RB][2];
#pragma unroll
  for (int i = 0; i < RB; ++i)
#pragma unroll
    for (int h = 0; h < 2; ++h) off_a[i][h] = kswz64((wm * RB + i) * 32 + lr, 2 * lh + h);
  const int wcol = wn * CB * 32;                           // the wave's first column in the tile
  const int off_w = A_BYTES + (wcol / W_ROWS) * B_BYTES + (lh * W_ROWS + wcol % W_ROWS + lr) * 16;

  issue(0, 0);
  if (NST == 3 && KT > 1) issue(1, 1);
  int slot = 0;
  for (int kt = 0; kt < KT; ++kt) {
    // this wave's pieces of step kt have landed.  Three stages: those of step kt+1 may still fly, and vmcnt counts this wave's
    // own loads only, so the count to wait down to is the wave's pieces per step: IT, or IT - 1 on the waves past REM
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

    bf16x8 bw[CB][3];                                      // [column tile][plane]
    f32x4 ca[RB][2];
    auto read_w = [&](int j0, int j1) {
#pragma unroll
      for (int j = j0; j < j1; ++j)
#pragma unroll
        for (int p = 0; p < 3; ++p) bw[j][p] = *reinterpret_cast<const bf16x8*>(St + off_w + p * PLANE + j * 512);
    };
    read_w(0, LEAN ? 3 : CB);
#pragma unroll
    for (int i = 0; i < RB; ++i)
#pragma unroll
      for (int h = 0; h < 2; ++h) ca[i][h] = *reinterpret_cast<const f32x4*>(St + off_a[i][h]);
    bf16x8 ah[RB], am[RB], al[RB];
    auto tile = [&](int i, int j) {                         // small terms first, one accumulator per output block
      acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(al[i], bw[j][0], acc[i][j], 0, 0, 0);
      acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(ah[i], bw[j][2], acc[i][j], 0, 0, 0);
      acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(am[i], bw[j][1], acc[i][j], 0, 0, 0);
      acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(am[i], bw[j][0], acc[i][j], 0, 0, 0);
      acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(ah[i], bw[j][1], acc[i][j], 0, 0, 0);
      acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(ah[i], bw[j][0], acc[i][j], 0, 0, 0);
    };
    auto products = [&](int i) {
#pragma unroll
      for (int j = 0; j < CB; ++j) tile(i, j);
    };
    if constexpr (ROWS) {
      // One split per wave and k-step.  Every accumulator's first product takes the lo part, the end of the split's dependency
      // chain, so no MFMA of this wave can start under the split (the SIMD's other waves run theirs meanwhile); what can be
      // arranged is that the LDS reads are out before it.  Left free, the compiler reads A, splits, and only then reads W, a pair
      // of column tiles at a time into the same registers, so the MFMAs wait for LDS three more times per step (measured: up to 2.4 %
      // slower, profiles/f32_split_rows_speed.md).
      if constexpr (LEAN) {
        // A and three tiles of W before the split; behind each of the first three tiles' MFMAs the reads of the tile three
        // further on, into the registers that tile frees: two tiles' MFMAs (384 matrix cycles) between a read and its use
        static_assert(CB == 6, "three tiles ahead");
        __builtin_amdgcn_sched_barrier(0);
        split8(ca[0][0], ca[0][1], ah[0], am[0], al[0]);
        __builtin_amdgcn_sched_barrier(0);
#pragma unroll
        for (int j = 0; j < 3; ++j) {
          tile(0, j);
          read_w(j + 3, j + 4);
          __builtin_amdgcn_sched_barrier(0);
        }
#pragma unroll
        for (int j = 3; j < CB; ++j) tile(0, j);
      } else {
        // all 20 reads before the split: at two workgroups per CU the wave has the registers for all of W (96 accumulators + 72
        // + the split's)
        split8(ca[0][0], ca[0][1], ah[0], am[0], al[0]);
        __builtin_amdgcn_sched_group_barrier(0x100, 2 + 3 * CB, 0);
        __builtin_amdgcn_sched_group_barrier(0x002, 40, 0);
        products(0);
      }
    } else {
      static_assert(!LEAN, "LEAN is a schedule of the row-owning tiling");
      split8(ca[0][0], ca[0][1], ah[0], am[0], al[0]);
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
  }
  __syncthreads();
}

}  // namespace pangu_split
