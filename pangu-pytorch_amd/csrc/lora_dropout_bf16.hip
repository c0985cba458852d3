// LoRA adapter dropout (bf16 activations) for gfx950: the bf16 training path's counterpart of lora_dropout_f32.hip.
//
// The projection kernels run on W_eff = W + s B A; with c = keep / (1 - p) - 1 (p / (1 - p) where an entry is kept, -1 where it is
// dropped; the mask: common.h, LoraDrop -- the one the fp32 kernels use, recomputed here and never stored) what is missing is
//   forward         y  = bf16(float(y) + s * ((c * x) bf16(A)^T) bf16(B)^T)            pangu_lora_dropout_fwd_bf16
//   input gradient  dx = bf16(float(dx) + c * (V bf16(A)) [* gelu'(float(pre))])       pangu_lora_dropout_dx_bf16
// (V = s dy B comes out of the adapter-gradient pass, pangu_lora_wgrad_dropout_bf16 in lora_bf16.hip).  x, y, h, dx and pre are
// bf16 and row-strided, A and B the fp32 master adapters (rounded to nearest-even bf16 in the fragments), V is fp32.  Products
// are v_mfma_f32_16x16x16_bf16 with fp32 accumulation; c * x, u = s (c * x) A^T and V are rounded to bf16 once each.
//
// A wave takes 64 tokens (four 16-token tiles that share every A / B fragment) with the TOKEN on the lane (the D column).  The
// 16 rows of an MFMA's other operand are dealt out so that a lane's four results of two MFMAs are 8 CONSECUTIVE columns of its
// token's row: y, h, dx and pre move as 16-B loads and stores, and u leaves the first product in the layout the second one reads
// (no LDS, no barrier, no scratch).  Every load is unconditional: row indices are clamped to M - 1 and rank indices to r - 1 (so
// nothing is read past the last row, past a row's K / N columns or past A / B), padding is a select on the loaded value, the
// loads of a 64-column step are issued together, and only the stores are predicated.  Each output element is written by one lane
// in a fixed order of operations: bit-identical from run to run.
#include "common.h"

namespace {

typedef short s16x4 __attribute__((ext_vector_type(4)));
typedef unsigned short u16;

constexpr int LD_THREADS = 256;
constexpr int LD_WAVES = LD_THREADS / 64;
constexpr int LD_SUB = 4;                          // 16-token tiles per wave
constexpr int LD_WG_TOK = LD_WAVES * LD_SUB * 16;   // tokens per workgroup (256)
constexpr int LD_MAX_KN = 1920;                    // as lora_bf16.hip: K + N of the widest projection

// MFMA lane roles (D = Aop Bop, 16x16x16): lane (l16 = lane & 15, lq = lane >> 4) supplies Aop[row l16][k 4 lq + j] and
// Bop[k 4 lq + j][col l16], j < 4, and receives D[row 4 lq + v][col l16] in register v.
// Column dealing: a step covers 32 columns with two MFMAs e = 0, 1.  As a CONTRACTION index (product 1) lane quarter lq, element j
// of MFMA e takes column 8 lq + 4 e + j on both operands (any order both operands share is a valid contraction order).  As an
// OUTPUT row (product 2, dx) Aop row l16 of MFMA e stands for column 8 (l16 >> 2) + 4 e + (l16 & 3), so D row 4 lq + v is column
// 8 lq + 4 e + v: either way a lane owns columns 8 lq .. 8 lq + 7 of the step, one 16-B piece of its token's row.

__device__ inline s16x4 bf16x4_of(f32x4 v) {
  typedef unsigned u32x2 __attribute__((ext_vector_type(2)));
  return __builtin_bit_cast(s16x4, u32x2{pack_bf16x2(v[0], v[1]), pack_bf16x2(v[2], v[3])});
}
__device__ inline float bf16_lo(unsigned w) { return __builtin_bit_cast(float, w << 16); }
__device__ inline float bf16_hi(unsigned w) { return __builtin_bit_cast(float, w & 0xFFFF0000u); }
// the fp32 values of elements 4 e .. 4 e + 3 of a 16-B piece of 8 bf16
__device__ inline f32x4 bf16x4_to_f32(const u32x4& q, int e) {
  return f32x4{bf16_lo(q[2 * e]), bf16_hi(q[2 * e]), bf16_lo(q[2 * e + 1]), bf16_hi(q[2 * e + 1])};
}
__device__ inline float bf16_round(float v) { return bf16_lo(pack_bf16x2(v, 0.f) & 0xFFFFu); }

// RT: 16-column tiles of the rank (1: r <= 16 with the columns >= r zero, 2: r = 32)
template <int RT, bool GELU>
__global__ __launch_bounds__(LD_THREADS) void lora_dropout_fwd_bf16_kernel(const u16* __restrict__ x, long long ldx, u16* __restrict__ y,
                                                                            long long ldy, const float* __restrict__ A,
                                                                            const float* __restrict__ B, u16* __restrict__ h,
                                                                            long long ldh, int M, int N, int K, int r, float s,
                                                                            LoraDrop d) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int l16 = lane & 15, lq = lane >> 4;
  const long long m0 = ((long long)blockIdx.x * LD_WAVES + wave) * (LD_SUB * 16);
  if (m0 >= M) return;                            // (wave-uniform; the kernel has no barrier)
  bool ok[LD_SUB];
  uint32_t hrow[LD_SUB];
  const u16* xr[LD_SUB];                          // the lane's token rows, clamped to the last one
  u16* yr[LD_SUB];
#pragma unroll
  for (int u = 0; u < LD_SUB; ++u) {
    const long long row = m0 + 16 * u + l16;
    const long long rc = row < M ? row : (long long)M - 1;
    ok[u] = row < M;
    hrow[u] = lora_drop_row(d, (uint32_t)row);
    xr[u] = x + rc * ldx;
    yr[u] = y + rc * ldy;
  }
  const s16x4 zero4 = s16x4{0, 0, 0, 0};

  // u^T (rank x token) = A (c * x)^T: Aop = bf16(A)[rank 16 t + l16][k], Bop = (c * x)[token l16][k]; D[rank 16 t + 4 lq + v][token l16]
  f32x4 pu[LD_SUB][RT];
#pragma unroll
  for (int u = 0; u < LD_SUB; ++u)
#pragma unroll
    for (int t = 0; t < RT; ++t) pu[u][t] = f32x4{0.f, 0.f, 0.f, 0.f};
  const float* ar[RT];
  bool aok[RT];
#pragma unroll
  for (int t = 0; t < RT; ++t) {
    const int c = t * 16 + l16;
    aok[t] = c < r;
    ar[t] = A + (size_t)(c < r ? c : r - 1) * K + 8 * lq;
  }
  for (int k0 = 0; k0 < K; k0 += 64) {
    u32x4 xq[2][LD_SUB];
    f32x4 aq[2][RT][2];
#pragma unroll
    for (int hf = 0; hf < 2; ++hf) {
#pragma unroll
      for (int u = 0; u < LD_SUB; ++u) xq[hf][u] = *reinterpret_cast<const u32x4*>(xr[u] + k0 + 32 * hf + 8 * lq);
#pragma unroll
      for (int t = 0; t < RT; ++t)
#pragma unroll
        for (int e = 0; e < 2; ++e) aq[hf][t][e] = *reinterpret_cast<const f32x4*>(ar[t] + k0 + 32 * hf + 4 * e);
    }
#pragma unroll
    for (int hf = 0; hf < 2; ++hf) {
      s16x4 af[RT][2];
#pragma unroll
      for (int t = 0; t < RT; ++t)
#pragma unroll
        for (int e = 0; e < 2; ++e) af[t][e] = aok[t] ? bf16x4_of(aq[hf][t][e]) : zero4;
      const uint32_t k = (uint32_t)(k0 + 32 * hf + 8 * lq);
#pragma unroll
      for (int u = 0; u < LD_SUB; ++u) {
#pragma unroll
        for (int e = 0; e < 2; ++e) {
          const f32x4 xv = bf16x4_to_f32(xq[hf][u], e);
          f32x4 cx;
#pragma unroll
          for (int j = 0; j < 4; ++j) cx[j] = lora_drop_keep(d, hrow[u], k + 4 * e + j) ? d.c_keep * xv[j] : -xv[j];
          const s16x4 cb = bf16x4_of(cx);
#pragma unroll
          for (int t = 0; t < RT; ++t) pu[u][t] = __builtin_amdgcn_mfma_f32_16x16x16bf16_1k(af[t][e], cb, pu[u][t], 0, 0, 0);
        }
      }
    }
  }
  // s u, rounded to bf16 once: element j of lane (lq, l16) = u[rank 16 t + 4 lq + j][token l16], the Bop of the second product
  s16x4 ub[LD_SUB][RT];
#pragma unroll
  for (int u = 0; u < LD_SUB; ++u)
#pragma unroll
    for (int t = 0; t < RT; ++t) ub[u][t] = bf16x4_of(pu[u][t] * s);

  // y^T (n x token) += B (s u)^T: Aop = bf16(B)[n of row l16][rank 16 t + 4 lq + j], the accumulator starts as float(y)
  const float* br[RT];
  bool bok[RT];
#pragma unroll
  for (int t = 0; t < RT; ++t) {
    const int c = t * 16 + 4 * lq;
    bok[t] = c < r;
    br[t] = B + (size_t)(8 * (l16 >> 2) + (l16 & 3)) * r + (c < r ? c : r - 4);
  }
  for (int n0 = 0; n0 < N; n0 += 64) {
    u32x4 yq[2][LD_SUB];
    f32x4 bq[2][RT][2];
#pragma unroll
    for (int hf = 0; hf < 2; ++hf) {
#pragma unroll
      for (int u = 0; u < LD_SUB; ++u) yq[hf][u] = *reinterpret_cast<const u32x4*>(yr[u] + n0 + 32 * hf + 8 * lq);
#pragma unroll
      for (int t = 0; t < RT; ++t)
#pragma unroll
        for (int e = 0; e < 2; ++e) bq[hf][t][e] = *reinterpret_cast<const f32x4*>(br[t] + (size_t)(n0 + 32 * hf + 4 * e) * r);
    }
#pragma unroll
    for (int hf = 0; hf < 2; ++hf) {
      s16x4 bf[RT][2];
#pragma unroll
      for (int t = 0; t < RT; ++t)
#pragma unroll
        for (int e = 0; e < 2; ++e) bf[t][e] = bok[t] ? bf16x4_of(bq[hf][t][e]) : zero4;
      const int n = n0 + 32 * hf + 8 * lq;
#pragma unroll
      for (int u = 0; u < LD_SUB; ++u) {
        f32x4 acc[2];
#pragma unroll
        for (int e = 0; e < 2; ++e) {
          acc[e] = bf16x4_to_f32(yq[hf][u], e);
#pragma unroll
          for (int t = 0; t < RT; ++t) acc[e] = __builtin_amdgcn_mfma_f32_16x16x16bf16_1k(bf[t][e], ub[u][t], acc[e], 0, 0, 0);
        }
        const u32x4 yo = u32x4{pack_bf16x2(acc[0][0], acc[0][1]), pack_bf16x2(acc[0][2], acc[0][3]),
                               pack_bf16x2(acc[1][0], acc[1][1]), pack_bf16x2(acc[1][2], acc[1][3])};
        if (ok[u]) *reinterpret_cast<u32x4*>(yr[u] + n) = yo;
        if (GELU) {                               // h = gelu of the ROUNDED y: what the backward re-creates from the stored pre
          u32x4 ho;
#pragma unroll
          for (int i = 0; i < 4; ++i) ho[i] = pack_bf16x2(gelu_erf(bf16_lo(yo[i])), gelu_erf(bf16_hi(yo[i])));
          if (ok[u]) *reinterpret_cast<u32x4*>(h + (m0 + 16 * u + l16) * ldh + n) = ho;
        }
      }
    }
  }
}

// dx^T (k x token) += c * A^T V^T: Aop = bf16(A)[rank 16 t + 4 lq + j][k of row l16], Bop = bf16(V)[token l16][that rank];
// D row 4 lq + v = column 8 lq + 4 e + v of the step.  GELU_BWD: the projection's input is gelu(pre) and dx is already the gradient
// of pre (the dx GEMM's epilogue multiplied by gelu'(pre)): the correction takes the same factor.
template <int RT, bool GELU_BWD>
__global__ __launch_bounds__(LD_THREADS) void lora_dropout_dx_bf16_kernel(u16* __restrict__ dx, long long lddx, const float* __restrict__ V,
                                                                           const float* __restrict__ A, const u16* __restrict__ pre,
                                                                           long long ldpre, int M, int K, int r, LoraDrop d) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int l16 = lane & 15, lq = lane >> 4;
  const long long m0 = ((long long)blockIdx.x * LD_WAVES + wave) * (LD_SUB * 16);
  if (m0 >= M) return;
  bool ok[LD_SUB];
  uint32_t hrow[LD_SUB];
  u16* dr[LD_SUB];
  const u16* pr[LD_SUB];
  s16x4 vf[LD_SUB][RT];
  const s16x4 zero4 = s16x4{0, 0, 0, 0};
  bool cok[RT];
  int cc[RT];
#pragma unroll
  for (int t = 0; t < RT; ++t) {
    const int c = t * 16 + 4 * lq;
    cok[t] = c < r;
    cc[t] = c < r ? c : r - 4;
  }
#pragma unroll
  for (int u = 0; u < LD_SUB; ++u) {
    const long long row = m0 + 16 * u + l16;
    const long long rc = row < M ? row : (long long)M - 1;
    ok[u] = row < M;
    hrow[u] = lora_drop_row(d, (uint32_t)row);
    dr[u] = dx + rc * lddx;
    pr[u] = GELU_BWD ? pre + rc * ldpre : nullptr;
#pragma unroll
    for (int t = 0; t < RT; ++t) {
      const f32x4 v = *reinterpret_cast<const f32x4*>(V + rc * r + cc[t]);
      vf[u][t] = cok[t] ? bf16x4_of(v) : zero4;
    }
  }
  // the lane's A column of MFMA e = 0 in a step's first half; rank rows cc[t] + j
  const float* ac = A + 8 * (l16 >> 2) + (l16 & 3);
  for (int k0 = 0; k0 < K; k0 += 64) {
    u32x4 gq[2][LD_SUB], pq[2][LD_SUB];
    f32x4 aq[2][RT][2];
#pragma unroll
    for (int hf = 0; hf < 2; ++hf) {
#pragma unroll
      for (int u = 0; u < LD_SUB; ++u) {
        gq[hf][u] = *reinterpret_cast<const u32x4*>(dr[u] + k0 + 32 * hf + 8 * lq);
        if (GELU_BWD) pq[hf][u] = *reinterpret_cast<const u32x4*>(pr[u] + k0 + 32 * hf + 8 * lq);
      }
#pragma unroll
      for (int t = 0; t < RT; ++t)
#pragma unroll
        for (int e = 0; e < 2; ++e)
#pragma unroll
          for (int j = 0; j < 4; ++j) aq[hf][t][e][j] = ac[(size_t)(cc[t] + j) * K + k0 + 32 * hf + 4 * e];
    }
#pragma unroll
    for (int hf = 0; hf < 2; ++hf) {
      s16x4 af[RT][2];
#pragma unroll
      for (int t = 0; t < RT; ++t)
#pragma unroll
        for (int e = 0; e < 2; ++e) af[t][e] = cok[t] ? bf16x4_of(aq[hf][t][e]) : zero4;
      const int k = k0 + 32 * hf + 8 * lq;
#pragma unroll
      for (int u = 0; u < LD_SUB; ++u) {
        f32x4 g[2];
#pragma unroll
        for (int e = 0; e < 2; ++e) {
          f32x4 acc = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
          for (int t = 0; t < RT; ++t) acc = __builtin_amdgcn_mfma_f32_16x16x16bf16_1k(af[t][e], vf[u][t], acc, 0, 0, 0);
          g[e] = bf16x4_to_f32(gq[hf][u], e);
          f32x4 pv = f32x4{0.f, 0.f, 0.f, 0.f};
          if (GELU_BWD) pv = bf16x4_to_f32(pq[hf][u], e);
#pragma unroll
          for (int v = 0; v < 4; ++v) {
            float c = lora_drop_keep(d, hrow[u], (uint32_t)(k + 4 * e + v)) ? d.c_keep : -1.0f;
            if (GELU_BWD) c *= gelu_erf_grad(pv[v]);
            g[e][v] = fmaf(c, acc[v], g[e][v]);
          }
        }
        const u32x4 go = u32x4{pack_bf16x2(g[0][0], g[0][1]), pack_bf16x2(g[0][2], g[0][3]), pack_bf16x2(g[1][0], g[1][1]),
                               pack_bf16x2(g[1][2], g[1][3])};
        if (ok[u]) *reinterpret_cast<u32x4*>(dr[u] + k) = go;
      }
    }
  }
}

bool rank_ok(int r) { return r == 4 || r == 8 || r == 16 || r == 32; }
bool aligned16(const void* p) { return (reinterpret_cast<size_t>(p) & 15) == 0; }

}  // namespace

extern "C" int pangu_lora_dropout_fwd_bf16(pangu_stream_t stream, const void* X, int ldx, void* Y, int ldy, const float* A,
                                           const float* B, int M, int N, int K, int r, float scaling, double p, unsigned seed, int act,
                                           void* H, int ldh) {
  if (!X || !Y || !A || !B) return PANGU_E_NULL;
  if (act != PANGU_ACT_NONE && act != PANGU_ACT_GELU) return PANGU_E_ARG;
  if (act == PANGU_ACT_GELU && !H) return PANGU_E_NULL;
  if (M <= 0 || !rank_ok(r) || K <= 0 || N <= 0 || (K & 63) || (N & 63) || K + N > LD_MAX_KN) return PANGU_E_SHAPE;
  if (ldx < K || ldy < N || (ldx & 7) || (ldy & 7)) return PANGU_E_SHAPE;
  if (act == PANGU_ACT_GELU && (ldh < N || (ldh & 7))) return PANGU_E_SHAPE;
  if (!aligned16(X) || !aligned16(Y) || !aligned16(A) || !aligned16(B) || (act == PANGU_ACT_GELU && !aligned16(H))) return PANGU_E_ARG;
  LoraDrop d;
  if (!lora_drop_make(p, seed, &d)) return PANGU_E_ARG;
  const long long blocks = ((long long)M + LD_WG_TOK - 1) / LD_WG_TOK;
  const dim3 grid((unsigned)blocks), block(LD_THREADS);
  hipStream_t st = (hipStream_t)stream;
  const u16* x = (const u16*)X;
  u16* y = (u16*)Y;
  u16* h = (u16*)H;
#define PANGU_LD_FWD(RT, G) \
  hipLaunchKernelGGL((lora_dropout_fwd_bf16_kernel<RT, G>), grid, block, 0, st, x, (long long)ldx, y, (long long)ldy, A, B, h, (long long)ldh, M, N, K, r, scaling, d)
  if (r > 16) {
    if (act == PANGU_ACT_GELU) PANGU_LD_FWD(2, true); else PANGU_LD_FWD(2, false);
  } else {
    if (act == PANGU_ACT_GELU) PANGU_LD_FWD(1, true); else PANGU_LD_FWD(1, false);
  }
#undef PANGU_LD_FWD
  return pangu_launch_status();
}

extern "C" int pangu_lora_dropout_dx_bf16(pangu_stream_t stream, void* dX, int lddx, const float* V, const float* A, int M, int K, int r,
                                          double p, unsigned seed, const void* pre, int ldpre) {
  if (!dX || !V || !A) return PANGU_E_NULL;
  if (M <= 0 || !rank_ok(r) || K <= 0 || (K & 63) || K > LD_MAX_KN) return PANGU_E_SHAPE;
  if (lddx < K || (lddx & 7) || (pre && (ldpre < K || (ldpre & 7)))) return PANGU_E_SHAPE;
  if (!aligned16(dX) || !aligned16(V) || !aligned16(A) || !aligned16(pre)) return PANGU_E_ARG;
  LoraDrop d;
  if (!lora_drop_make(p, seed, &d)) return PANGU_E_ARG;
  const long long blocks = ((long long)M + LD_WG_TOK - 1) / LD_WG_TOK;
  const dim3 grid((unsigned)blocks), block(LD_THREADS);
  hipStream_t st = (hipStream_t)stream;
  u16* dx = (u16*)dX;
  const u16* pp = (const u16*)pre;
#define PANGU_LD_DX(RT, G) \
  hipLaunchKernelGGL((lora_dropout_dx_bf16_kernel<RT, G>), grid, block, 0, st, dx, (long long)lddx, V, A, pp, (long long)ldpre, M, K, r, d)
  if (r > 16) {
    if (pre) PANGU_LD_DX(2, true); else PANGU_LD_DX(2, false);
  } else {
    if (pre) PANGU_LD_DX(1, true); else PANGU_LD_DX(1, false);
  }
#undef PANGU_LD_DX
  return pangu_launch_status();
}
