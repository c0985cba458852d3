// LoRA adapter kernels (fp32) for gfx950.
//
// A LoRA-adapted projection y = x W_eff^T + b with W_eff = W + s * B A (A (r, K), B (N, r), s = alpha / r) trains only A and B:
//   dA = s * V^T x,   V = dy B   (r, K)
//   dB = s * dy^T U,  U = x A^T  (N, r)
// pangu_lora_wgrad_f32 computes both in ONE pass over x (M, K) and dy (M, N).  Every workgroup owns a contiguous slab of
// tokens and walks it 16 tokens at a time: the 16 x K slab of x and the 16 x N slab of dy are staged in LDS by LDS-DMA, U and V of those 16 tokens are made from them with v_mfma_f32_16x16x4_f32 (the K / N
// contraction split over the 8 waves, summed in LDS in a fixed order), and the same LDS slabs then feed the dA / dB tiles,
// which live in registers for the whole slab.  x and dy are read from HBM exactly once; A and B (<= 240 KB) come from L2.
// The per-workgroup partials go to a caller-owned workspace and one reduce launch sums them in workgroup order: no float
// atomics, bit-identical results from run to run.
// Ranks 4 / 8 run on the 16-wide tiles with the columns >= r zero (their MFMA work is padding; the pass is HBM-bound there).
//
// pangu_lora_merge_f32: W_eff = W + s * (B A), fp32, the rank sum in the fixed order j = 0 .. r-1.
#include <algorithm>

#include "common.h"

namespace {

constexpr int LR_ROWS = 16;           // tokens per step (the M dimension of one 16x16x4 MFMA)
constexpr int LR_THREADS = 512;       // 8 waves
constexpr int LR_WAVES = LR_THREADS / 64;
constexpr int LR_MAX_KN = 1920;       // K + N of the widest projection of the model (384 -> 1536, 1536 -> 384)
constexpr int LR_NF = (LR_ROWS * LR_MAX_KN / 4 + LR_THREADS - 1) / LR_THREADS;      // staged float4 per thread (15)

constexpr size_t lora_lds_bytes(int K, int N, int RT) {
  return ((size_t)LR_ROWS * (K + N) + (size_t)LR_WAVES * 2 * RT * 256) * sizeof(float);
}

// The adapter-dropout policy (pangu_lora_wgrad_dropout_f32): the kernel's one trailing argument, absent in the plain pass
struct LoraDropOut {
  LoraDrop d;
  float* V;      // (M, r): s * dy B, what the input-gradient correction reads (lora_dropout_f32.hip)
  float s;
};
inline __device__ const LoraDropOut* drop_arg() { return nullptr; }
inline __device__ const LoraDropOut* drop_arg(const LoraDropOut& o) { return &o; }

// RT = 16-column tiles of the rank (1: r <= 16, 2: r = 32).  DropArgs: empty (the plain pass, the instantiation is what it was
// before the policy existed) or one LoraDropOut: the staged x slab is then turned into drop(x) = keep * x / (1 - p) in LDS
// before the two products that read it (U = drop(x) A^T and dA = V^T drop(x)), and V of every token is written out as well.
template <int RT, typename... DropArgs>
__global__ __launch_bounds__(LR_THREADS, 1) void lora_wgrad_f32_kernel(const float* __restrict__ dy, int lddy,
                                                                       const float* __restrict__ x, int ldx,
                                                                       const float* __restrict__ A, const float* __restrict__ B,
                                                                       float* __restrict__ ws, int M, int N, int K, int r,
                                                                       int rows_per_wg, DropArgs... drop_args) {
  constexpr bool DROP = sizeof...(DropArgs) != 0;
  const LoraDropOut* const drop = drop_arg(drop_args...);
  constexpr int MAXB = (LR_MAX_KN / 16 + LR_WAVES - 1) / LR_WAVES;     // column blocks per wave
  extern __shared__ __attribute__((aligned(16))) float lds[];
  float* xs = lds;                                             // [16][K] (swizzled, below)
  float* ds = xs + LR_ROWS * K;                                // [16][N]
  float* red = ds + LR_ROWS * N;                                // [wave][U | V][RT][16 tokens][16 rank columns]

  const int m_begin = blockIdx.x * rows_per_wg;
  const int m_end = min(M, m_begin + rows_per_wg);
  const int rows = max(m_end - m_begin, 0);
  const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int l16 = lane & 15, lq = lane >> 4;

  // range-checked descriptors over this slab only: rows past its end (the ragged last step) read as zero
  const int x_bytes = rows > 0 ? (int)(((size_t)(rows - 1) * ldx + K) * sizeof(float)) : 0;
  const int d_bytes = rows > 0 ? (int)(((size_t)(rows - 1) * lddy + N) * sizeof(float)) : 0;
  const __amdgpu_buffer_rsrc_t x_rsrc =
      __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(x + (size_t)m_begin * ldx), 0, x_bytes, 0x00020000);
  const __amdgpu_buffer_rsrc_t d_rsrc =
      __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(dy + (size_t)m_begin * lddy), 0, d_bytes, 0x00020000);

  // staging of one 16-token step by LDS-DMA (`buffer_load_dwordx4 ... lds`: no staging registers).  The step's image is
  // [x: 16 rows of K | dy: 16 rows of N], 16-B piece p at byte 16 p (what the DMA writes: lane-linear), and within a row
  // the float4 slot s holds column group s ^ (row & 15): the U / V fragments (16 rows, one column group) hit 16 distinct
  // 16-B bank groups.  16 K / 4 and 16 (K + N) / 4 are multiples of 64: each wave-instruction is all x or all dy.
  const int x4 = K >> 2, d4 = N >> 2;
  const int nx = LR_ROWS * x4, ntot = nx + LR_ROWS * d4;
  unsigned goff[LR_NF];
#pragma unroll
  for (int i = 0; i < LR_NF; ++i) {
    const int f = tid + LR_THREADS * i;
    goff[i] = 0u;
    if (f < nx) {
      const int row = f / x4, c4 = (f - row * x4) ^ (row & 15);
      goff[i] = ((unsigned)row * (unsigned)ldx + 4u * c4) * 4u;
    } else if (f < ntot) {
      const int g = f - nx, row = g / d4, c4 = (g - row * d4) ^ (row & 15);
      goff[i] = ((unsigned)row * (unsigned)lddy + 4u * c4) * 4u;
    }
  }
  auto issue = [&](int m0) {          // m0: first token of the step, relative to the slab
    const unsigned xo = (unsigned)m0 * (unsigned)ldx * 4u, dof = (unsigned)m0 * (unsigned)lddy * 4u;
#pragma unroll
    for (int i = 0; i < LR_NF; ++i) {
      const int f0 = LR_THREADS * i + 64 * wave;               // first piece of this wave-instruction
      auto dst = (__attribute__((address_space(3))) void*)(reinterpret_cast<unsigned char*>(lds) + 16 * f0);
      if (f0 < nx) __builtin_amdgcn_raw_ptr_buffer_load_lds(x_rsrc, dst, 16, (int)(xo + goff[i]), 0, 0, 0);
      else if (f0 < ntot) __builtin_amdgcn_raw_ptr_buffer_load_lds(d_rsrc, dst, 16, (int)(dof + goff[i]), 0, 0, 0);
    }
  };
  auto xs_at = [&](int row, int col) { return xs[row * K + 4 * ((col >> 2) ^ (row & 15)) + (col & 3)]; };
  auto ds_at = [&](int row, int col) { return ds[row * N + 4 * ((col >> 2) ^ (row & 15)) + (col & 3)]; };

  // the 16-wide column blocks of [K | N] are dealt round-robin to the waves: wave w owns blocks b = w + 8 j.  For each it
  // computes the U / V partial over those columns, and it owns the RT output tiles of those columns: dA (rt, b) for b < K/16,
  // dB (b - K/16, rt) after
  f32x4 acc[MAXB * RT];
#pragma unroll
  for (int i = 0; i < MAXB * RT; ++i) acc[i] = f32x4{0.f, 0.f, 0.f, 0.f};

  const int kb = K >> 4, nblk = (K + N) >> 4;
  const int steps = (rows + LR_ROWS - 1) / LR_ROWS;
  for (int st = 0; st < steps; ++st) {
    issue(st * LR_ROWS);
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");       // this wave's pieces have landed
    __syncthreads();                                       // ... and everybody's
    if constexpr (DROP) {
      // x -> drop(x) = keep * x / (1 - p), once, in the staged slab: the U and the dA product below both read it from there.
      // 32 threads per token row; slot c of a row holds the column group c ^ (row & 15)
      const int row = tid >> 5;
      const uint32_t hrow = lora_drop_row(drop->d, (uint32_t)(m_begin + st * LR_ROWS + row));
      for (int c = tid & 31; c < x4; c += 32) {
        f32x4* q = reinterpret_cast<f32x4*>(&xs[row * K + 4 * c]);
        f32x4 v = *q;
        const uint32_t k = 4u * (uint32_t)(c ^ (row & 15));
#pragma unroll
        for (int j = 0; j < 4; ++j) v[j] = lora_drop_keep(drop->d, hrow, k + j) ? v[j] * drop->d.inv : 0.f;
        *q = v;
      }
      __syncthreads();
    }

    // U = x A^T, V = dy B of these 16 tokens.  Within a block, lane quarter q and MFMA step j take column 16 b + 4 q + j on
    // BOTH operands (a permutation of the contraction order: each lane reads 4 consecutive values with one b128 load)
    f32x4 pu[RT], pv[RT];
#pragma unroll
    for (int t = 0; t < RT; ++t) pu[t] = pv[t] = f32x4{0.f, 0.f, 0.f, 0.f};
    for (int b = wave; b < nblk; b += LR_WAVES) {
      if (b < kb) {
        const int k = b * 16 + 4 * lq;
        const f32x4 xa = *reinterpret_cast<const f32x4*>(&xs[l16 * K + 4 * ((k >> 2) ^ l16)]);
#pragma unroll
        for (int t = 0; t < RT; ++t) {
          const int c = t * 16 + l16;
          const f32x4 af = c < r ? *reinterpret_cast<const f32x4*>(&A[(size_t)c * K + k]) : f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
          for (int j = 0; j < 4; ++j) pu[t] = __builtin_amdgcn_mfma_f32_16x16x4f32(xa[j], af[j], pu[t], 0, 0, 0);
        }
      } else {
        const int n = (b - kb) * 16 + 4 * lq;
        const f32x4 da = *reinterpret_cast<const f32x4*>(&ds[l16 * N + 4 * ((n >> 2) ^ l16)]);
#pragma unroll
        for (int t = 0; t < RT; ++t) {
          const int c = t * 16 + l16;
          float bf[4];
#pragma unroll
          for (int j = 0; j < 4; ++j) bf[j] = c < r ? B[(size_t)(n + j) * r + c] : 0.f;
#pragma unroll
          for (int j = 0; j < 4; ++j) pv[t] = __builtin_amdgcn_mfma_f32_16x16x4f32(da[j], bf[j], pv[t], 0, 0, 0);
        }
      }
    }
    // partials -> LDS (C/D map: column = lane & 15, row = 4 (lane >> 4) + v), then the sum over the waves in wave order
#pragma unroll
    for (int t = 0; t < RT; ++t)
#pragma unroll
      for (int v = 0; v < 4; ++v) {
        red[((wave * 2 + 0) * RT + t) * 256 + (4 * lq + v) * 16 + l16] = pu[t][v];
        red[((wave * 2 + 1) * RT + t) * 256 + (4 * lq + v) * 16 + l16] = pv[t][v];
      }
    __syncthreads();
    for (int e = tid; e < 2 * RT * 256; e += LR_THREADS) {
      float s = red[e];
#pragma unroll
      for (int w = 1; w < LR_WAVES; ++w) s += red[w * 2 * RT * 256 + e];
      red[e] = s;                                              // U = red[0 .. RT*256), V = red[RT*256 .. 2*RT*256)
      if constexpr (DROP) {
        if (e >= RT * 256) {                                   // V[token][rank] of this step's tokens, scaled
          const int v = e - RT * 256, rt = v >> 8, row = (v >> 4) & 15, c = rt * 16 + (v & 15);
          const int m = m_begin + st * LR_ROWS + row;
          if (m < m_end && c < r) drop->V[(size_t)m * r + c] = drop->s * s;
        }
      }
    }
    __syncthreads();

    // dA (rt, kt) += V^T x  and  dB (nt, rt) += dy^T U over these 16 tokens (contraction over the tokens: step j, quarter q
    // take token 4 j + q)
#pragma unroll
    for (int jb = 0; jb < MAXB; ++jb) {
      const int b = wave + LR_WAVES * jb;
      if (b < kb) {
#pragma unroll
        for (int rt = 0; rt < RT; ++rt)
#pragma unroll
          for (int j = 0; j < 4; ++j) {
            const int row = 4 * j + lq;
            acc[jb * RT + rt] = __builtin_amdgcn_mfma_f32_16x16x4f32(red[(RT + rt) * 256 + row * 16 + l16],
                                                                      xs_at(row, b * 16 + l16), acc[jb * RT + rt], 0, 0, 0);
          }
      } else if (b < nblk) {
#pragma unroll
        for (int rt = 0; rt < RT; ++rt)
#pragma unroll
          for (int j = 0; j < 4; ++j) {
            const int row = 4 * j + lq;
            acc[jb * RT + rt] = __builtin_amdgcn_mfma_f32_16x16x4f32(ds_at(row, (b - kb) * 16 + l16),
                                                                      red[rt * 256 + row * 16 + l16], acc[jb * RT + rt], 0, 0, 0);
          }
      }
      __builtin_amdgcn_sched_barrier(0);      // one block's operands live at a time (hoisting them all would spill)
    }
    __syncthreads();
  }

  // this workgroup's partial: ws[wg] = [dA (r, K) | dB (N, r)], the padded rank columns dropped
  float* out = ws + (size_t)blockIdx.x * (size_t)r * (K + N);
#pragma unroll
  for (int jb = 0; jb < MAXB; ++jb) {
    const int b = wave + LR_WAVES * jb;
#pragma unroll
    for (int rt = 0; rt < RT; ++rt) {
      if (b < kb) {              // dA tile: row (rank) = rt*16 + 4 q + v, column k = 16 b + lane & 15
#pragma unroll
        for (int v = 0; v < 4; ++v) {
          const int c = rt * 16 + 4 * lq + v;
          if (c < r) out[(size_t)c * K + b * 16 + l16] = acc[jb * RT + rt][v];
        }
      } else if (b < nblk) {     // dB tile: row n = 16 (b - K/16) + 4 q + v, column (rank) = rt*16 + lane & 15
        const int c = rt * 16 + l16;
        if (c < r) {
#pragma unroll
          for (int v = 0; v < 4; ++v) out[(size_t)r * K + (size_t)((b - kb) * 16 + 4 * lq + v) * r + c] = acc[jb * RT + rt][v];
        }
      }
    }
  }
}

// dA / dB = s * (sum of the workgroup partials, in workgroup order)
__global__ __launch_bounds__(256) void lora_reduce_f32_kernel(const float* __restrict__ ws, int parts, int per,
                                                              float* __restrict__ dA, float* __restrict__ dB, int rK, float s) {
  const int e = blockIdx.x * 256 + threadIdx.x;
  if (e >= per) return;
  float acc = 0.f;
#pragma unroll 8
  for (int g = 0; g < parts; ++g) acc += ws[(size_t)g * per + e];
  if (e < rK) dA[e] = s * acc;
  else dB[e - rK] = s * acc;
}

__global__ __launch_bounds__(256) void lora_merge_f32_kernel(const float* __restrict__ W, const float* __restrict__ A,
                                                             const float* __restrict__ B, float* __restrict__ We, int N, int K,
                                                             int r, float s) {
  const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
  if (i >= (long long)N * K) return;
  const int n = (int)(i / K), k = (int)(i - (long long)n * K);
  float acc = 0.f;
  for (int j = 0; j < r; ++j) acc = fmaf(B[(size_t)n * r + j], A[(size_t)j * K + k], acc);
  We[i] = W[i] + s * acc;
}

bool lora_rank_ok(int r) { return r == 4 || r == 8 || r == 16 || r == 32; }

// the launch behind both entries; drop: nullptr (the plain pass) or the dropout policy's argument
int lora_wgrad_launch(pangu_stream_t stream, const float* dY, int lddy, const float* X, int ldx, const float* A, const float* B,
                      float* dA, float* dB, int M, int N, int K, int r, float scaling, float* workspace, long long workspace_bytes,
                      const LoraDropOut* drop) {
  if (!dY || !X || !A || !B || !dA || !dB || !workspace) return PANGU_E_NULL;
  if (M <= 0 || !lora_rank_ok(r) || K <= 0 || N <= 0 || (K & 63) || (N & 63) || K + N > LR_MAX_KN) return PANGU_E_SHAPE;
  if (ldx < K || lddy < N || (ldx & 3) || (lddy & 3)) return PANGU_E_SHAPE;
  if ((reinterpret_cast<size_t>(X) | reinterpret_cast<size_t>(dY) | reinterpret_cast<size_t>(A) |
       reinterpret_cast<size_t>(workspace)) & 15)
    return PANGU_E_ARG;                                         // b128 loads
  const long long per = (long long)r * (K + N);                 // floats of one partial
  if (workspace_bytes < per * (long long)sizeof(float)) return PANGU_E_ARG;
  const int RT = r > 16 ? 2 : 1;
  const size_t lds = lora_lds_bytes(K, N, RT);
  // one workgroup per CU (two where the LDS footprint allows it), fewer when the workspace cannot hold their partials
  long long parts = lds <= 80 * 1024 ? 512 : 256;
  parts = std::min(parts, workspace_bytes / (per * (long long)sizeof(float)));
  const int rows = (int)(((M + parts - 1) / parts + LR_ROWS - 1) / LR_ROWS * LR_ROWS);
  parts = (M + rows - 1) / rows;
  // 32-bit byte offsets of the slab descriptors
  if ((long long)(rows + LR_ROWS) * std::max(ldx, lddy) * (long long)sizeof(float) >= 0x7FFFFFFFll) return PANGU_E_RANGE;
  hipStream_t s = (hipStream_t)stream;
  if (drop && RT == 2) {
    PANGU_ENSURE_DYN_LDS((lora_wgrad_f32_kernel<2, LoraDropOut>), lds);
    hipLaunchKernelGGL((lora_wgrad_f32_kernel<2, LoraDropOut>), dim3((unsigned)parts), dim3(LR_THREADS), lds, s, dY, lddy, X, ldx, A,
                       B, workspace, M, N, K, r, rows, *drop);
  } else if (drop) {
    PANGU_ENSURE_DYN_LDS((lora_wgrad_f32_kernel<1, LoraDropOut>), lds);
    hipLaunchKernelGGL((lora_wgrad_f32_kernel<1, LoraDropOut>), dim3((unsigned)parts), dim3(LR_THREADS), lds, s, dY, lddy, X, ldx, A,
                       B, workspace, M, N, K, r, rows, *drop);
  } else if (RT == 2) {
    PANGU_ENSURE_DYN_LDS(lora_wgrad_f32_kernel<2>, lds);
    hipLaunchKernelGGL(lora_wgrad_f32_kernel<2>, dim3((unsigned)parts), dim3(LR_THREADS), lds, s, dY, lddy, X, ldx, A, B,
                       workspace, M, N, K, r, rows);
  } else {
    PANGU_ENSURE_DYN_LDS(lora_wgrad_f32_kernel<1>, lds);
    hipLaunchKernelGGL(lora_wgrad_f32_kernel<1>, dim3((unsigned)parts), dim3(LR_THREADS), lds, s, dY, lddy, X, ldx, A, B,
                       workspace, M, N, K, r, rows);
  }
  const int rc = pangu_launch_status();
  if (rc != PANGU_OK) return rc;
  hipLaunchKernelGGL(lora_reduce_f32_kernel, dim3((unsigned)((per + 255) / 256)), dim3(256), 0, s, workspace, (int)parts, (int)per,
                     dA, dB, r * K, scaling);
  return pangu_launch_status();
}

}  // namespace

extern "C" int pangu_lora_wgrad_f32(pangu_stream_t stream, const float* dY, int lddy, const float* X, int ldx, const float* A,
                                    const float* B, float* dA, float* dB, int M, int N, int K, int r, float scaling,
                                    float* workspace, long long workspace_bytes) {
  return lora_wgrad_launch(stream, dY, lddy, X, ldx, A, B, dA, dB, M, N, K, r, scaling, workspace, workspace_bytes, nullptr);
}

extern "C" int pangu_lora_wgrad_dropout_f32(pangu_stream_t stream, const float* dY, int lddy, const float* X, int ldx, const float* A,
                                            const float* B, float* dA, float* dB, float* V, int M, int N, int K, int r, float scaling,
                                            double p, unsigned seed, float* workspace, long long workspace_bytes) {
  if (!V) return PANGU_E_NULL;
  LoraDropOut drop;
  if (!lora_drop_make(p, seed, &drop.d)) return PANGU_E_ARG;
  drop.V = V;
  drop.s = scaling;
  return lora_wgrad_launch(stream, dY, lddy, X, ldx, A, B, dA, dB, M, N, K, r, scaling, workspace, workspace_bytes, &drop);
}

extern "C" int pangu_lora_merge_f32(pangu_stream_t stream, const float* W, const float* A, const float* B, float* W_eff, int N,
                                    int K, int r, float scaling) {
  if (!W || !A || !B || !W_eff) return PANGU_E_NULL;
  if (N <= 0 || K <= 0 || !lora_rank_ok(r)) return PANGU_E_SHAPE;
  const long long n = (long long)N * K;
  if ((n + 255) / 256 > 0x7FFFFFFFll) return PANGU_E_RANGE;
  hipLaunchKernelGGL(lora_merge_f32_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, (hipStream_t)stream, W, A, B, W_eff,
                     N, K, r, scaling);
  return pangu_launch_status();
}
