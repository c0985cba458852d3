// LoRA adapter dropout (fp32) for gfx950: the two streaming corrections around the unchanged projection launches.
//
// peft computes an adapted projection as y = x W^T + b + s * drop(x) A^T B^T with drop(x) = keep * x / (1 - p) in training mode.
// The projection kernels run on W_eff = W + s B A, i.e. they already hold the term without dropout; with c = keep / (1 - p) - 1
// (p / (1 - p) where an entry is kept, -1 where it is dropped; the mask: common.h, LoraDrop) drop(x) = x + c * x and what is
// missing is additive:
//   forward         y  += s * ((c * x) A^T) B^T                     pangu_lora_dropout_fwd_f32, after the projection's launch
//   input gradient  dx += c * (V A),  V = s * dy B  (M, r)          pangu_lora_dropout_dx_f32, after the projection's dx GEMM
// (V comes out of the adapter-gradient pass, pangu_lora_wgrad_dropout_f32 in lora_f32.hip).
//
// Both kernels give a wave 32 tokens (two 16-token tiles that share every A / B fragment) and use v_mfma_f32_16x16x4_f32 with the
// TOKEN on the lane (the D column): a lane then owns four consecutive columns of one token's row in every product, so x, y, h and
// dx move as 16-B vector loads and stores, and the (token x r) intermediate u = (c * x) A^T leaves the first product in exactly
// the layout the second one reads (no LDS, no barrier, no scratch).  A and B (<= 240 KB) come from L2.  Each output element is
// written by one lane in a fixed order of operations: bit-identical from run to run.
#include "common.h"

namespace {

constexpr int LD_THREADS = 256;
constexpr int LD_WAVES = LD_THREADS / 64;
constexpr int LD_SUB = 2;                         // 16-token tiles per wave
constexpr int LD_WG_TOK = LD_WAVES * LD_SUB * 16;  // tokens per workgroup (128)
constexpr int LD_MAX_KN = 1920;                   // as lora_f32.hip: K + N of the widest projection

// MFMA lane roles (D = Aop Bop, 16x16x4): lane (l16 = lane & 15, lq = lane >> 4) supplies Aop[row l16][k lq] and Bop[k lq][col l16]
// and receives D[row 4 lq + v][col l16] in register v.  Every contraction below is walked in a permuted order that both operands
// share: lane quarter lq and step j take index 4 lq + j of a 16-wide group (one b128 load per lane where the index is contiguous).

// RT: 16-column tiles of the rank (1: r <= 16 with the columns >= r zero, 2: r = 32)
template <int RT, bool GELU>
__global__ __launch_bounds__(LD_THREADS) void lora_dropout_fwd_kernel(const float* __restrict__ x, long long ldx, float* __restrict__ y,
                                                                       long long ldy, const float* __restrict__ A,
                                                                       const float* __restrict__ B, float* __restrict__ h,
                                                                       long long ldh, int M, int N, int K, int r, float s, LoraDrop d) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int l16 = lane & 15, lq = lane >> 4;
  const long long m0 = ((long long)blockIdx.x * LD_WAVES + wave) * (LD_SUB * 16);
  if (m0 >= M) return;                            // (wave-uniform; the kernel has no barrier)
  long long row[LD_SUB];
  bool ok[LD_SUB];
  uint32_t hrow[LD_SUB];
#pragma unroll
  for (int u = 0; u < LD_SUB; ++u) {
    row[u] = m0 + 16 * u + l16;
    ok[u] = row[u] < M;
    hrow[u] = lora_drop_row(d, (uint32_t)row[u]);
  }

  // u^T (rank x token) = A (c * x)^T: Aop = A[rank 16 t + l16][k], Bop = (c * x)[token l16][k]; D[rank 16 t + 4 lq + v][token l16]
  f32x4 pu[LD_SUB][RT];
#pragma unroll
  for (int u = 0; u < LD_SUB; ++u)
#pragma unroll
    for (int t = 0; t < RT; ++t) pu[u][t] = f32x4{0.f, 0.f, 0.f, 0.f};
  for (int kb = 0; kb < (K >> 4); ++kb) {
    const int k = kb * 16 + 4 * lq;
    f32x4 af[RT];
#pragma unroll
    for (int t = 0; t < RT; ++t) {
      const int c = t * 16 + l16;
      af[t] = c < r ? *reinterpret_cast<const f32x4*>(&A[(size_t)c * K + k]) : f32x4{0.f, 0.f, 0.f, 0.f};
    }
#pragma unroll
    for (int u = 0; u < LD_SUB; ++u) {
      f32x4 xv = f32x4{0.f, 0.f, 0.f, 0.f};
      if (ok[u]) xv = *reinterpret_cast<const f32x4*>(&x[row[u] * ldx + k]);
      f32x4 cx;
#pragma unroll
      for (int j = 0; j < 4; ++j) cx[j] = lora_drop_keep(d, hrow[u], (uint32_t)(k + j)) ? d.c_keep * xv[j] : -xv[j];
#pragma unroll
      for (int t = 0; t < RT; ++t)
#pragma unroll
        for (int j = 0; j < 4; ++j) pu[u][t] = __builtin_amdgcn_mfma_f32_16x16x4f32(af[t][j], cx[j], pu[u][t], 0, 0, 0);
    }
  }
#pragma unroll
  for (int u = 0; u < LD_SUB; ++u)
#pragma unroll
    for (int t = 0; t < RT; ++t) pu[u][t] *= s;

  // y^T (n x token) += B (s u)^T: Aop = B[n 16 nb + l16][rank 16 t + 4 lq + j], Bop = pu[t][j] (that rank, token l16), the accumulator
  // starts as y[token l16][16 nb + 4 lq + v]
  for (int nb = 0; nb < (N >> 4); ++nb) {
    f32x4 bf[RT];
#pragma unroll
    for (int t = 0; t < RT; ++t) {
      const int c = t * 16 + 4 * lq;
      bf[t] = c < r ? *reinterpret_cast<const f32x4*>(&B[(size_t)(nb * 16 + l16) * r + c]) : f32x4{0.f, 0.f, 0.f, 0.f};
    }
    const int n = nb * 16 + 4 * lq;
#pragma unroll
    for (int u = 0; u < LD_SUB; ++u) {
      f32x4 acc = f32x4{0.f, 0.f, 0.f, 0.f};
      if (ok[u]) acc = *reinterpret_cast<const f32x4*>(&y[row[u] * ldy + n]);
#pragma unroll
      for (int t = 0; t < RT; ++t)
#pragma unroll
        for (int j = 0; j < 4; ++j) acc = __builtin_amdgcn_mfma_f32_16x16x4f32(bf[t][j], pu[u][t][j], acc, 0, 0, 0);
      if (ok[u]) {
        *reinterpret_cast<f32x4*>(&y[row[u] * ldy + n]) = acc;
        if (GELU) {
          f32x4 g;
#pragma unroll
          for (int v = 0; v < 4; ++v) g[v] = gelu_erf(acc[v]);
          *reinterpret_cast<f32x4*>(&h[row[u] * ldh + n]) = g;
        }
      }
    }
  }
}

// dx^T (k x token) += c * A^T V^T: Aop = A[rank 16 t + 4 lq + j][k 16 kb + l16], Bop = V[token l16][that rank];
// D[k 16 kb + 4 lq + v][token l16].  GELU_BWD: the projection's input is gelu(pre) and dx is already the gradient of pre (the dx
// GEMM's epilogue multiplied by gelu'(pre)): the correction takes the same factor.
template <int RT, bool GELU_BWD>
__global__ __launch_bounds__(LD_THREADS) void lora_dropout_dx_kernel(float* __restrict__ dx, long long lddx, const float* __restrict__ V,
                                                                      const float* __restrict__ A, const float* __restrict__ pre,
                                                                      long long ldpre, int M, int K, int r, LoraDrop d) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int l16 = lane & 15, lq = lane >> 4;
  const long long m0 = ((long long)blockIdx.x * LD_WAVES + wave) * (LD_SUB * 16);
  if (m0 >= M) return;
  long long row[LD_SUB];
  bool ok[LD_SUB];
  uint32_t hrow[LD_SUB];
  f32x4 vf[LD_SUB][RT];
#pragma unroll
  for (int u = 0; u < LD_SUB; ++u) {
    row[u] = m0 + 16 * u + l16;
    ok[u] = row[u] < M;
    hrow[u] = lora_drop_row(d, (uint32_t)row[u]);
#pragma unroll
    for (int t = 0; t < RT; ++t) {
      const int c = t * 16 + 4 * lq;
      vf[u][t] = (ok[u] && c < r) ? *reinterpret_cast<const f32x4*>(&V[row[u] * r + c]) : f32x4{0.f, 0.f, 0.f, 0.f};
    }
  }
  for (int kb = 0; kb < (K >> 4); ++kb) {
    float af[RT][4];
#pragma unroll
    for (int t = 0; t < RT; ++t)
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const int c = t * 16 + 4 * lq + j;
        af[t][j] = c < r ? A[(size_t)c * K + kb * 16 + l16] : 0.f;
      }
    const int k = kb * 16 + 4 * lq;
#pragma unroll
    for (int u = 0; u < LD_SUB; ++u) {
      f32x4 acc = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
      for (int t = 0; t < RT; ++t)
#pragma unroll
        for (int j = 0; j < 4; ++j) acc = __builtin_amdgcn_mfma_f32_16x16x4f32(af[t][j], vf[u][t][j], acc, 0, 0, 0);
      if (ok[u]) {
        f32x4 g = *reinterpret_cast<const f32x4*>(&dx[row[u] * lddx + k]);
        f32x4 pv = f32x4{0.f, 0.f, 0.f, 0.f};
        if (GELU_BWD) pv = *reinterpret_cast<const f32x4*>(&pre[row[u] * ldpre + k]);
#pragma unroll
        for (int v = 0; v < 4; ++v) {
          float c = lora_drop_keep(d, hrow[u], (uint32_t)(k + v)) ? d.c_keep : -1.0f;
          if (GELU_BWD) c *= gelu_erf_grad(pv[v]);
          g[v] = fmaf(c, acc[v], g[v]);
        }
        *reinterpret_cast<f32x4*>(&dx[row[u] * lddx + k]) = g;
      }
    }
  }
}

bool rank_ok(int r) { return r == 4 || r == 8 || r == 16 || r == 32; }
bool aligned16(const void* p) { return (reinterpret_cast<size_t>(p) & 15) == 0; }

}  // namespace

extern "C" int pangu_lora_dropout_fwd_f32(pangu_stream_t stream, const float* X, int ldx, float* Y, int ldy, const float* A,
                                          const float* B, int M, int N, int K, int r, float scaling, double p, unsigned seed, int act,
                                          float* H, int ldh) {
  if (!X || !Y || !A || !B) return PANGU_E_NULL;
  if (act != PANGU_ACT_NONE && act != PANGU_ACT_GELU) return PANGU_E_ARG;
  if (act == PANGU_ACT_GELU && !H) return PANGU_E_NULL;
  if (M <= 0 || !rank_ok(r) || K <= 0 || N <= 0 || (K & 63) || (N & 63) || K + N > LD_MAX_KN) return PANGU_E_SHAPE;
  if (ldx < K || ldy < N || (ldx & 3) || (ldy & 3)) return PANGU_E_SHAPE;
  if (act == PANGU_ACT_GELU && (ldh < N || (ldh & 3))) return PANGU_E_SHAPE;
  if (!aligned16(X) || !aligned16(Y) || !aligned16(A) || !aligned16(B) || (act == PANGU_ACT_GELU && !aligned16(H))) return PANGU_E_ARG;
  LoraDrop d;
  if (!lora_drop_make(p, seed, &d)) return PANGU_E_ARG;
  const long long blocks = ((long long)M + LD_WG_TOK - 1) / LD_WG_TOK;
  const dim3 grid((unsigned)blocks), block(LD_THREADS);
  hipStream_t st = (hipStream_t)stream;
#define PANGU_LD_FWD(RT, G) \
  hipLaunchKernelGGL((lora_dropout_fwd_kernel<RT, G>), grid, block, 0, st, X, (long long)ldx, Y, (long long)ldy, A, B, H, (long long)ldh, M, N, K, r, scaling, d)
  if (r > 16) {
    if (act == PANGU_ACT_GELU) PANGU_LD_FWD(2, true); else PANGU_LD_FWD(2, false);
  } else {
    if (act == PANGU_ACT_GELU) PANGU_LD_FWD(1, true); else PANGU_LD_FWD(1, false);
  }
#undef PANGU_LD_FWD
  return pangu_launch_status();
}

extern "C" int pangu_lora_dropout_dx_f32(pangu_stream_t stream, float* dX, int lddx, const float* V, const float* A, int M, int K, int r,
                                         double p, unsigned seed, const float* pre, int ldpre) {
  if (!dX || !V || !A) return PANGU_E_NULL;
  if (M <= 0 || !rank_ok(r) || K <= 0 || (K & 63) || K > LD_MAX_KN) return PANGU_E_SHAPE;
  if (lddx < K || (lddx & 3) || (pre && (ldpre < K || (ldpre & 3)))) return PANGU_E_SHAPE;
  if (!aligned16(dX) || !aligned16(V) || !aligned16(A) || !aligned16(pre)) return PANGU_E_ARG;
  LoraDrop d;
  if (!lora_drop_make(p, seed, &d)) return PANGU_E_ARG;
  const long long blocks = ((long long)M + LD_WG_TOK - 1) / LD_WG_TOK;
  const dim3 grid((unsigned)blocks), block(LD_THREADS);
  hipStream_t st = (hipStream_t)stream;
#define PANGU_LD_DX(RT, G) \
  hipLaunchKernelGGL((lora_dropout_dx_kernel<RT, G>), grid, block, 0, st, dX, (long long)lddx, V, A, pre, (long long)ldpre, M, K, r, d)
  if (r > 16) {
    if (pre) PANGU_LD_DX(2, true); else PANGU_LD_DX(2, false);
  } else {
    if (pre) PANGU_LD_DX(1, true); else PANGU_LD_DX(1, false);
  }
#undef PANGU_LD_DX
  return pangu_launch_status();
}
