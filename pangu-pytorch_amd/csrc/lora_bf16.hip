// LoRA adapter-gradient kernel (bf16 operands) for gfx950: the bf16 training path's counterpart of lora_f32.hip.
//
//   dA = s * V^T x,   V = dy bf16(B)   (r, K)
//   dB = s * dy^T U,  U = x bf16(A)^T  (N, r)
// x (M, K) and dy (M, N) are bf16 and row-strided; A (r, K) and B (N, r) are the fp32 master parameters, rounded to nearest-even
// bf16 by the kernel ONCE per workgroup into the MFMA fragments every wave keeps in registers for its own columns.  All products
// are bf16 MFMA (v_mfma_f32_16x16x16_bf16) with fp32 accumulation; U and V are rounded to bf16 once, to become the second
// product's operand.  Nothing else is rounded; s is applied in fp32 by the reduce launch.
//
// ONE pass: every workgroup owns a contiguous slab of tokens and walks it 16 tokens at a time.  A step's image is 16 rows of
// [x row | dy row | pad] in LDS -- 60.5 KB at the widest projection (K + N = 1920), so TWO stages fit the CU's LDS: the next
// step's rows are requested (range-checked buffer loads into registers) before this step's products and written to the other
// stage after them.  The 16-wide column blocks of [K | N] are dealt round-robin to the 8 waves: wave w owns blocks w + 8 j.
//   product 1: the wave's partial of U (x blocks) / V (dy blocks) over its own columns, operand = a ROW read of the image;
//              the 8 partials are summed in LDS in wave order and stored as bf16 [rank][token]
//   product 2: contraction over the 16 tokens; the x / dy operand is a TRANSPOSING read (ds_read_b64_tr_b16) of the same image;
//              the dA / dB tiles of the wave's blocks live in registers for the whole slab.
// Image rows are an odd multiple of 32 B long: the 8 token rows a 32-lane half takes in one transposing read lie in 8 different
// 32-B bank groups (conflict-free); the row reads of product 1 are 2-way.
// The per-workgroup partials go to the caller's workspace and one reduce launch sums them in workgroup order: no float atomics,
// bit-identical results from run to run.  Ranks 4 / 8 run on the 16-wide tiles with the columns >= r zero.
#include <algorithm>

#include "common.h"

namespace {

typedef short s16x4 __attribute__((ext_vector_type(4)));
typedef unsigned short u16;

constexpr int LB_ROWS = 16;            // tokens per step (the contraction length of one 16x16x16 MFMA)
constexpr int LB_THREADS = 512;        // 8 waves
constexpr int LB_WAVES = LB_THREADS / 64;
constexpr int LB_MAX_KN = 1920;        // K + N of the widest projection of the model (384 -> 1536, 1536 -> 384)
constexpr int LB_NARROW_KN = 1024;     // the MAXB = 8 instantiation covers K + N up to here

// bytes of one image row: [K + N bf16 | pad], an odd multiple of 32 B
constexpr int lb_row_bytes(int K, int N) { return (K + N) * 2 + ((((K + N) >> 4) & 1) ? 0 : 32); }
constexpr size_t lb_lds_bytes(int K, int N, int RT) {
  return 2 * (size_t)LB_ROWS * lb_row_bytes(K, N) + (size_t)LB_WAVES * 2 * RT * 256 * sizeof(float) + (size_t)2 * RT * 256 * sizeof(u16);
}

__device__ inline s16x4 bf16x4_of(float a, float b, float c, float d) {
  typedef unsigned u32x2 __attribute__((ext_vector_type(2)));
  return __builtin_bit_cast(s16x4, u32x2{pack_bf16x2(a, b), pack_bf16x2(c, d)});
}

// The adapter-dropout policy (pangu_lora_wgrad_dropout_bf16): the kernel's one trailing argument, absent in the plain pass
struct LoraDropOut {
  LoraDrop d;
  float* V;      // (M, r) fp32: s * dy bf16(B), what the input-gradient correction reads (lora_dropout_bf16.hip)
  float s;
};
inline __device__ const LoraDropOut* drop_arg() { return nullptr; }
inline __device__ const LoraDropOut* drop_arg(const LoraDropOut& o) { return &o; }

// RT = 16-column tiles of the rank (1: r <= 16, 2: r = 32); MAXB = column blocks per wave (8: K + N <= 1024, 15: <= 1920).
// DropArgs: empty (the plain pass: the instantiation is what it was before the policy existed) or one LoraDropOut: the dropped
// entries of the staged x slab are then zeroed in LDS, once per step, before the two products that read it (U = drop(x) A^T and
// dA = V^T drop(x); the factor 1 / (1 - p) is left to the reduce launch, in fp32 with s: both gradients are linear in drop(x) and
// the masking adds no rounding), and V of every token is written out from the reduced fp32 partials.
template <int RT, int MAXB, typename... DropArgs>
__global__ __launch_bounds__(LB_THREADS) void lora_wgrad_bf16_kernel(const u16* __restrict__ dy, int lddy, const u16* __restrict__ x,
                                                                     int ldx, const float* __restrict__ A,
                                                                     const float* __restrict__ B, float* __restrict__ ws, int M,
                                                                     int N, int K, int r, int rows_per_wg,
                                                                     DropArgs... drop_args) {
  constexpr bool DROP = sizeof...(DropArgs) != 0;
  const LoraDropOut* const drop = drop_arg(drop_args...);
  constexpr int NF = MAXB / 2 + 2;      // staged 16-B chunks per thread: ceil(2 K / 512) + ceil(2 N / 512) <= (K + N) / 256 + 2
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  const int LD = lb_row_bytes(K, N);
  const int STAGE = LB_ROWS * LD;
  float* red = reinterpret_cast<float*>(smem + 2 * STAGE);             // [wave][U | V][RT][16 tokens][16 rank columns]
  u16* uvt = reinterpret_cast<u16*>(red + LB_WAVES * 2 * RT * 256);   // [U | V][RT][16 rank columns][16 tokens], bf16

  const int m_begin = blockIdx.x * rows_per_wg;
  const int m_end = min(M, m_begin + rows_per_wg);
  const int rows = max(m_end - m_begin, 0);
  const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int l16 = lane & 15, lq = lane >> 4;
  const int kb = K >> 4, nblk = (K + N) >> 4;

  // range-checked descriptors over this slab only: rows past its end (the ragged last step) read as zero
  const int x_bytes = rows > 0 ? (int)(((size_t)(rows - 1) * ldx + K) * sizeof(u16)) : 0;
  const int d_bytes = rows > 0 ? (int)(((size_t)(rows - 1) * lddy + N) * sizeof(u16)) : 0;
  const __amdgpu_buffer_rsrc_t x_rsrc =
      __builtin_amdgcn_make_buffer_rsrc(const_cast<u16*>(x + (size_t)m_begin * ldx), 0, x_bytes, 0x00020000);
  const __amdgpu_buffer_rsrc_t d_rsrc =
      __builtin_amdgcn_make_buffer_rsrc(const_cast<u16*>(dy + (size_t)m_begin * lddy), 0, d_bytes, 0x00020000);

  // staging of one step: 16-B chunk f = tid + 512 i of the x rows (i < nfx: 16 rows of K / 8 chunks), then of the dy rows.
  // goff: byte offset in the step's rows; loff: byte offset in the image, -1 for a chunk that does not exist
  const int xc = K >> 3, dc = N >> 3;
  const int nfx = (LB_ROWS * xc + LB_THREADS - 1) / LB_THREADS, nfd = (LB_ROWS * dc + LB_THREADS - 1) / LB_THREADS;
  unsigned goff[NF];
  int loff[NF];
#pragma unroll
  for (int i = 0; i < NF; ++i) {
    goff[i] = 0u;
    loff[i] = -1;
    if (i < nfx) {
      const int f = tid + LB_THREADS * i, row = f / xc, c = f - row * xc;
      if (row < LB_ROWS) {
        goff[i] = ((unsigned)row * (unsigned)ldx + 8u * c) * 2u;
        loff[i] = row * LD + 16 * c;
      }
    } else if (i < nfx + nfd) {
      const int f = tid + LB_THREADS * (i - nfx), row = f / dc, c = f - row * dc;
      if (row < LB_ROWS) {
        goff[i] = ((unsigned)row * (unsigned)lddy + 8u * c) * 2u;
        loff[i] = row * LD + 2 * K + 16 * c;
      }
    }
  }
  u32x4 rg[NF];
  auto fetch = [&](int m0) {          // m0: first token of the step, relative to the slab
    const unsigned xo = (unsigned)m0 * (unsigned)ldx * 2u, dof = (unsigned)m0 * (unsigned)lddy * 2u;
#pragma unroll
    for (int i = 0; i < NF; ++i) {
      if (i < nfx) rg[i] = __builtin_amdgcn_raw_buffer_load_b128(x_rsrc, (int)(loff[i] >= 0 ? xo + goff[i] : 0xFFFFFFFFu), 0, 0);
      else if (i < nfx + nfd) rg[i] = __builtin_amdgcn_raw_buffer_load_b128(d_rsrc, (int)(loff[i] >= 0 ? dof + goff[i] : 0xFFFFFFFFu), 0, 0);
    }
  };
  auto stash = [&](int buf) {
    unsigned char* img = smem + buf * STAGE;
#pragma unroll
    for (int i = 0; i < NF; ++i)
      if (i < nfx + nfd && loff[i] >= 0) *reinterpret_cast<u32x4*>(img + loff[i]) = rg[i];
  };

  // the wave's column blocks b = wave + 8 j of [K | N]; for each, the bf16 fragment of A (x blocks) / B (dy blocks) as the B
  // operand of product 1: element j of lane (q, c) = bf16(A[rank c][16 b + 4 q + j]) / bf16(B[16 (b - kb) + 4 q + j][rank c])
  // (A and B are addressed through descriptors with 32-bit offsets: 64-bit addresses of all blocks at once would spill)
  const __amdgpu_buffer_rsrc_t a_rsrc = __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(A), 0, r * K * (int)sizeof(float), 0x00020000);
  const __amdgpu_buffer_rsrc_t b_rsrc = __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(B), 0, N * r * (int)sizeof(float), 0x00020000);
  s16x4 wf[MAXB * RT];
  f32x4 acc[MAXB * RT];
#pragma unroll
  for (int jb = 0; jb < MAXB; ++jb) {
    const int b = wave + LB_WAVES * jb;
#pragma unroll
    for (int t = 0; t < RT; ++t) {
      const int c = t * 16 + l16;
      f32x4 v = f32x4{0.f, 0.f, 0.f, 0.f};
      if (b < kb) {
        if (c < r) v = __builtin_bit_cast(f32x4, __builtin_amdgcn_raw_buffer_load_b128(a_rsrc, (c * K + b * 16 + 4 * lq) * 4, 0, 0));
      } else if (b < nblk) {
        const int n = (b - kb) * 16 + 4 * lq;
        if (c < r) {
#pragma unroll
          for (int j = 0; j < 4; ++j) v[j] = __builtin_bit_cast(float, __builtin_amdgcn_raw_buffer_load_b32(b_rsrc, ((n + j) * r + c) * 4, 0, 0));
        }
      }
      wf[jb * RT + t] = bf16x4_of(v[0], v[1], v[2], v[3]);
      acc[jb * RT + t] = f32x4{0.f, 0.f, 0.f, 0.f};
    }
  }

  const int steps = (rows + LB_ROWS - 1) / LB_ROWS;
  if (steps > 0) {
    fetch(0);
    stash(0);
  }
  __syncthreads();
  for (int st = 0; st < steps; ++st) {
    const bool more = st + 1 < steps;
    if (more) fetch((st + 1) * LB_ROWS);
    const unsigned char* img = smem + (st & 1) * STAGE;
    if constexpr (DROP) {
      // x -> keep * x, once, in the staged slab: 32 threads per token row, 16-B pieces of 8 columns
      const int row = tid >> 5;
      const uint32_t hrow = lora_drop_row(drop->d, (uint32_t)(m_begin + st * LB_ROWS + row));
      for (int c = tid & 31; c < (K >> 3); c += 32) {
        u32x4* q = reinterpret_cast<u32x4*>(smem + (st & 1) * STAGE + row * LD + 16 * c);
        u32x4 v = *q;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          const unsigned lo = lora_drop_keep(drop->d, hrow, (uint32_t)(8 * c + 2 * j)) ? 0x0000FFFFu : 0u;
          const unsigned hi = lora_drop_keep(drop->d, hrow, (uint32_t)(8 * c + 2 * j + 1)) ? 0xFFFF0000u : 0u;
          v[j] &= lo | hi;
        }
        *q = v;
      }
      __syncthreads();
    }

    // product 1: U = x A^T, V = dy B of these 16 tokens, this wave's columns (A operand: token l16, columns 16 b + 4 q ..)
    f32x4 pu[RT], pv[RT];
#pragma unroll
    for (int t = 0; t < RT; ++t) pu[t] = pv[t] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int jb = 0; jb < MAXB; ++jb) {
      const int b = wave + LB_WAVES * jb;
      if (b < nblk) {
        const s16x4 xa = *reinterpret_cast<const s16x4*>(img + l16 * LD + b * 32 + 8 * lq);
        if (b < kb) {
#pragma unroll
          for (int t = 0; t < RT; ++t) pu[t] = __builtin_amdgcn_mfma_f32_16x16x16bf16_1k(xa, wf[jb * RT + t], pu[t], 0, 0, 0);
        } else {
#pragma unroll
          for (int t = 0; t < RT; ++t) pv[t] = __builtin_amdgcn_mfma_f32_16x16x16bf16_1k(xa, wf[jb * RT + t], pv[t], 0, 0, 0);
        }
      }
    }
    // partials -> LDS (C/D map: column (rank) = lane & 15, row (token) = 4 (lane >> 4) + v), then the sum over the waves in
    // wave order, rounded to bf16 and stored [rank][token]: the layout product 2 reads 4 tokens of one rank from
#pragma unroll
    for (int t = 0; t < RT; ++t)
#pragma unroll
      for (int v = 0; v < 4; ++v) {
        red[((wave * 2 + 0) * RT + t) * 256 + (4 * lq + v) * 16 + l16] = pu[t][v];
        red[((wave * 2 + 1) * RT + t) * 256 + (4 * lq + v) * 16 + l16] = pv[t][v];
      }
    __syncthreads();
    for (int e = tid; e < 2 * RT * 256; e += LB_THREADS) {
      float s = red[e];
#pragma unroll
      for (int w = 1; w < LB_WAVES; ++w) s += red[w * 2 * RT * 256 + e];
      const int tile = e >> 8, tok = (e >> 4) & 15, c = e & 15;
      uvt[tile * 256 + c * 16 + tok] = (u16)(pack_bf16x2(s, 0.f) & 0xFFFFu);
      if constexpr (DROP) {
        if (tile >= RT) {                                      // V[token][rank] of this step's tokens, scaled, before its rounding
          const int m = m_begin + st * LB_ROWS + tok, cr = (tile - RT) * 16 + c;
          if (m < m_end && cr < r) drop->V[(size_t)m * r + cr] = drop->s * s;
        }
      }
    }
    __syncthreads();

    // product 2: dA (rt, kt) += V^T x and dB (nt, rt) += dy^T U over these 16 tokens (lane quarter q, element j: token 4 q + j)
    s16x4 uf[RT], vf[RT];
#pragma unroll
    for (int t = 0; t < RT; ++t) {
      uf[t] = *reinterpret_cast<const s16x4*>(&uvt[(0 * RT + t) * 256 + l16 * 16 + 4 * lq]);
      vf[t] = *reinterpret_cast<const s16x4*>(&uvt[(1 * RT + t) * 256 + l16 * 16 + 4 * lq]);
    }
#pragma unroll
    for (int jb = 0; jb < MAXB; ++jb) {
      const int b = wave + LB_WAVES * jb;
      if (b < nblk) {          // wave-uniform: the transposing read runs with every lane active
        // lane (q, c) supplies the address of row 4 q + (c >> 2), columns 16 b + 4 (c & 3) ..; it receives [token 4 q + j][16 b + c]
        const unsigned char* p = img + (4 * lq + (l16 >> 2)) * LD + b * 32 + 8 * (l16 & 3);
        const s16x4 tr = __builtin_amdgcn_ds_read_tr16_b64_v4i16((__attribute__((address_space(3))) s16x4*)(p));
        if (b < kb) {
#pragma unroll
          for (int t = 0; t < RT; ++t)
            acc[jb * RT + t] = __builtin_amdgcn_mfma_f32_16x16x16bf16_1k(vf[t], tr, acc[jb * RT + t], 0, 0, 0);
        } else {
#pragma unroll
          for (int t = 0; t < RT; ++t)
            acc[jb * RT + t] = __builtin_amdgcn_mfma_f32_16x16x16bf16_1k(tr, uf[t], acc[jb * RT + t], 0, 0, 0);
        }
      }
    }
    if (more) stash((st + 1) & 1);
    __syncthreads();
  }

  // this workgroup's partial: ws[wg] = [dA (r, K) | dB (N, r)], the padded rank columns dropped
  const int per = r * (K + N);
  // plain stores with 32-bit element offsets (per < 2^16).  Not raw_buffer_store_b32 on a bit_cast accumulator element: hipcc
  // (ROCm 7.2) then stored element 0 of every tile four times
  float* __restrict__ out = ws + (size_t)blockIdx.x * (size_t)per;
#pragma unroll
  for (int jb = 0; jb < MAXB; ++jb) {
    const int b = wave + LB_WAVES * jb;
#pragma unroll
    for (int rt = 0; rt < RT; ++rt) {
      if (b < kb) {              // dA tile: row (rank) = rt*16 + 4 q + v, column k = 16 b + lane & 15
#pragma unroll
        for (int v = 0; v < 4; ++v) {
          const int c = rt * 16 + 4 * lq + v;
          if (c < r) out[c * K + b * 16 + l16] = acc[jb * RT + rt][v];
        }
      } else if (b < nblk) {     // dB tile: row n = 16 (b - K/16) + 4 q + v, column (rank) = rt*16 + lane & 15
        const int c = rt * 16 + l16;
        if (c < r) {
#pragma unroll
          for (int v = 0; v < 4; ++v)
            out[r * K + ((b - kb) * 16 + 4 * lq + v) * r + c] = acc[jb * RT + rt][v];
        }
      }
    }
  }
}

// dA / dB = s * (sum of the workgroup partials, in workgroup order)
__global__ __launch_bounds__(256) void lora_reduce_bf16_kernel(const float* __restrict__ ws, int parts, int per,
                                                               float* __restrict__ dA, float* __restrict__ dB, int rK, float s) {
  const int e = blockIdx.x * 256 + threadIdx.x;
  if (e >= per) return;
  float acc = 0.f;
#pragma unroll 8
  for (int g = 0; g < parts; ++g) acc += ws[(size_t)g * per + e];
  if (e < rK) dA[e] = s * acc;
  else dB[e - rK] = s * acc;
}

// drop_args: none (the plain pass) or the dropout policy's argument
template <int RT, int MAXB, typename... DropArgs>
void launch_lora_wgrad_bf16(hipStream_t s, int parts, size_t lds, const u16* dY, int lddy, const u16* X, int ldx, const float* A,
                            const float* B, float* ws, int M, int N, int K, int r, int rows, DropArgs... drop_args) {
  auto kern = lora_wgrad_bf16_kernel<RT, MAXB, DropArgs...>;
  PANGU_ENSURE_DYN_LDS(kern, lds);
  hipLaunchKernelGGL(kern, dim3((unsigned)parts), dim3(LB_THREADS), lds, s, dY, lddy, X, ldx, A, B, ws, M, N, K, r, rows,
                     drop_args...);
}

// the launches behind both entries; drop: nullptr (the plain pass) or the dropout policy's argument
int lora_wgrad_bf16_launch(pangu_stream_t stream, const void* dY, int lddy, const void* X, int ldx, const float* A, const float* B,
                           float* dA, float* dB, int M, int N, int K, int r, float scaling, float* workspace,
                           long long workspace_bytes, const LoraDropOut* drop) {
  if (!dY || !X || !A || !B || !dA || !dB || !workspace) return PANGU_E_NULL;
  if (M <= 0 || !(r == 4 || r == 8 || r == 16 || r == 32) || K <= 0 || N <= 0 || (K & 15) || (N & 15) || K + N > LB_MAX_KN)
    return PANGU_E_SHAPE;
  if (ldx < K || lddy < N || (ldx & 7) || (lddy & 7)) return PANGU_E_SHAPE;
  if ((reinterpret_cast<size_t>(X) | reinterpret_cast<size_t>(dY) | reinterpret_cast<size_t>(A) | reinterpret_cast<size_t>(B) |
       reinterpret_cast<size_t>(workspace)) & 15)
    return PANGU_E_ARG;                                         // b128 loads
  const long long per = (long long)r * (K + N);                 // floats of one partial
  if (workspace_bytes < per * (long long)sizeof(float)) return PANGU_E_ARG;
  const int RT = r > 16 ? 2 : 1;
  const bool narrow = K + N <= LB_NARROW_KN;
  const size_t lds = lb_lds_bytes(K, N, RT);
  // one workgroup per CU (two where the LDS footprint allows it), fewer when the workspace cannot hold their partials
  long long parts = lds <= 80 * 1024 ? 512 : 256;
  parts = std::min(parts, workspace_bytes / (per * (long long)sizeof(float)));
  const int rows = (int)(((M + parts - 1) / parts + LB_ROWS - 1) / LB_ROWS * LB_ROWS);
  parts = (M + rows - 1) / rows;
  // 32-bit byte offsets of the slab descriptors
  if ((long long)(rows + LB_ROWS) * std::max(ldx, lddy) * (long long)sizeof(u16) >= 0x7FFFFFFFll) return PANGU_E_RANGE;
  hipStream_t s = (hipStream_t)stream;
  const u16* d = (const u16*)dY;
  const u16* x = (const u16*)X;
  if (drop) {
    if (RT == 2 && narrow) launch_lora_wgrad_bf16<2, 8>(s, (int)parts, lds, d, lddy, x, ldx, A, B, workspace, M, N, K, r, rows, *drop);
    else if (RT == 2) launch_lora_wgrad_bf16<2, 15>(s, (int)parts, lds, d, lddy, x, ldx, A, B, workspace, M, N, K, r, rows, *drop);
    else if (narrow) launch_lora_wgrad_bf16<1, 8>(s, (int)parts, lds, d, lddy, x, ldx, A, B, workspace, M, N, K, r, rows, *drop);
    else launch_lora_wgrad_bf16<1, 15>(s, (int)parts, lds, d, lddy, x, ldx, A, B, workspace, M, N, K, r, rows, *drop);
  } else if (RT == 2 && narrow) launch_lora_wgrad_bf16<2, 8>(s, (int)parts, lds, d, lddy, x, ldx, A, B, workspace, M, N, K, r, rows);
  else if (RT == 2) launch_lora_wgrad_bf16<2, 15>(s, (int)parts, lds, d, lddy, x, ldx, A, B, workspace, M, N, K, r, rows);
  else if (narrow) launch_lora_wgrad_bf16<1, 8>(s, (int)parts, lds, d, lddy, x, ldx, A, B, workspace, M, N, K, r, rows);
  else launch_lora_wgrad_bf16<1, 15>(s, (int)parts, lds, d, lddy, x, ldx, A, B, workspace, M, N, K, r, rows);
  const int rc = pangu_launch_status();
  if (rc != PANGU_OK) return rc;
  hipLaunchKernelGGL(lora_reduce_bf16_kernel, dim3((unsigned)((per + 255) / 256)), dim3(256), 0, s, workspace, (int)parts, (int)per,
                     dA, dB, r * K, drop ? scaling * drop->d.inv : scaling);
  return pangu_launch_status();
}

}  // namespace

extern "C" int pangu_lora_wgrad_bf16(pangu_stream_t stream, const void* dY, int lddy, const void* X, int ldx, const float* A,
                                     const float* B, float* dA, float* dB, int M, int N, int K, int r, float scaling,
                                     float* workspace, long long workspace_bytes) {
  return lora_wgrad_bf16_launch(stream, dY, lddy, X, ldx, A, B, dA, dB, M, N, K, r, scaling, workspace, workspace_bytes, nullptr);
}

extern "C" int pangu_lora_wgrad_dropout_bf16(pangu_stream_t stream, const void* dY, int lddy, const void* X, int ldx, const float* A,
                                             const float* B, float* dA, float* dB, float* V, int M, int N, int K, int r,
                                             float scaling, double p, unsigned seed, float* workspace, long long workspace_bytes) {
  if (!V) return PANGU_E_NULL;
  if ((K & 63) || (N & 63)) return PANGU_E_SHAPE;              // the dropout entries' common contract
  if (reinterpret_cast<size_t>(V) & 15) return PANGU_E_ARG;
  LoraDropOut drop;
  if (!lora_drop_make(p, seed, &drop.d)) return PANGU_E_ARG;
  drop.V = V;
  drop.s = scaling;
  return lora_wgrad_bf16_launch(stream, dY, lddy, X, ldx, A, B, dA, dB, M, N, K, r, scaling, workspace, workspace_bytes, &drop);
}
