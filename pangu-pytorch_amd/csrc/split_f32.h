// What the exact-split fp32 GEMMs (gemm_f32_split.hip, gemm_ln_f32_split.hip) share: the bf16 hi/mid/lo split of fp32 values, the
// layout constants of the weight image (pangu_split_weight_bf16x3) and of the LDS stage both kernels stream it into, and the
// swizzle of the fp32 A image.
#pragma once
#include "common.h"

namespace pangu_split {

typedef short bf16x8 __attribute__((ext_vector_type(8)));

constexpr int BK = 16;                           // k-step: one 64-byte fp32 A row, two 8-wide bf16 k-halves
constexpr int W_ROWS = 192;                      // rows of one n-tile block of the image
constexpr int PLANE = 2 * W_ROWS * 16;           // one bf16 plane of an (n-tile, k-step) block: [k-half][row][8 bf16]
constexpr int B_BYTES = 3 * PLANE;               // 18432: hi, mid, lo
constexpr int W_PIECES = B_BYTES / 1024;         // 18 linear 1-KB LDS-DMA pieces per block
constexpr int NSTAGE = 3;                        // ring depth: LDS-DMA two k-steps ahead, one barrier per step

// byte offset of logical 16-B chunk `chunk` of row `row` (64-byte rows, chunk XOR F[(row>>2)&3], F = {0,2,3,1}): gemm_f32_dma.hip
__device__ inline int kswz64(int row, int chunk) {
  const int f = (0x78 >> (((row >> 2) & 3) * 2)) & 3;
  return row * 64 + ((chunk ^ f) << 4);
}

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

}  // namespace pangu_split
