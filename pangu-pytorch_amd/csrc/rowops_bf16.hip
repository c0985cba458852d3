// bf16-I/O variants of the HBM-bound row kernels (fp32 statistics and arithmetic, bf16 loads/stores as 8-byte
// quads per lane): post-norm residual, down/up-sample gather + LayerNorm, patch-embed gather.
#include "common.h"

namespace {

typedef unsigned short u16;
typedef unsigned int u32x2 __attribute__((ext_vector_type(2)));

constexpr int ROWS_PER_BLOCK = 4;

__device__ inline f32x4 ld4(const u16* p) {
  const u32x2 u = *reinterpret_cast<const u32x2*>(p);
  return f32x4{__builtin_bit_cast(float, u[0] << 16), __builtin_bit_cast(float, u[0] & 0xFFFF0000u),
               __builtin_bit_cast(float, u[1] << 16), __builtin_bit_cast(float, u[1] & 0xFFFF0000u)};
}
__device__ inline void st4(u16* p, f32x4 v) {
  *reinterpret_cast<u32x2*>(p) = u32x2{pack_bf16x2(v[0], v[1]), pack_bf16x2(v[2], v[3])};
}

template <int NV>
__device__ inline void row_layernorm(f32x4 (&v)[NV], int nvec, int lane, int C, const float* gamma,
                                     const float* beta) {
  float s = 0.f;
#pragma unroll
  for (int i = 0; i < NV; ++i)
    if (lane + 64 * i < nvec) s += (v[i][0] + v[i][1]) + (v[i][2] + v[i][3]);
  const float mean = wave_sum(s) / C;
  float q = 0.f;
#pragma unroll
  for (int i = 0; i < NV; ++i)
    if (lane + 64 * i < nvec) {
#pragma unroll
      for (int c = 0; c < 4; ++c) { const float d = v[i][c] - mean; q += d * d; }
    }
  const float rstd = rsqrtf(wave_sum(q) / C + LN_EPS);
#pragma unroll
  for (int i = 0; i < NV; ++i)
    if (lane + 64 * i < nvec) {
      const f32x4 gm = *reinterpret_cast<const f32x4*>(gamma + 4 * (lane + 64 * i));
      const f32x4 bt = *reinterpret_cast<const f32x4*>(beta + 4 * (lane + 64 * i));
      v[i] = (v[i] - mean) * rstd * gm + bt;
    }
}

template <int NV>
__global__ __launch_bounds__(256) void ln_residual_bf16_kernel(const u16* __restrict__ y, const u16* __restrict__ shortcut,
                                                               int lds, const float* __restrict__ gamma,
                                                               const float* __restrict__ beta, u16* __restrict__ out,
                                                               int ldo, int N, int C, float branch_scale) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int nvec = C >> 2;
  for (int row = blockIdx.x * ROWS_PER_BLOCK + wave; row < N; row += gridDim.x * ROWS_PER_BLOCK) {
    f32x4 v[NV];
#pragma unroll
    for (int i = 0; i < NV; ++i)
      if (lane + 64 * i < nvec) v[i] = ld4(y + (size_t)row * C + 4 * (lane + 64 * i));
    row_layernorm<NV>(v, nvec, lane, C, gamma, beta);
#pragma unroll
    for (int i = 0; i < NV; ++i)
      if (lane + 64 * i < nvec) {
        const f32x4 sc = ld4(shortcut + (size_t)row * lds + 4 * (lane + 64 * i));
        st4(out + (size_t)row * ldo + 4 * (lane + 64 * i), sc + branch_scale * v[i]);
      }
  }
}

// Fast path of the post-norm residual for C % 8 == 0, C <= 512 (the model's 192 / 384): 16-B loads (8 channels per
// lane), LPR lanes per row (32 -> two rows per wave at C <= 256), gamma/beta held in registers, the branch AND the
// shortcut requested together before any arithmetic, two row groups in flight per wave.
template <int LPR>
__global__ __launch_bounds__(256) void ln_residual_bf16_v8_kernel(const u16* __restrict__ y, const u16* __restrict__ shortcut,
                                                                  int lds, const float* __restrict__ gamma,
                                                                  const float* __restrict__ beta, u16* __restrict__ out,
                                                                  int ldo, int N, int C, float branch_scale) {
  constexpr int RPW = 64 / LPR, UNR = 2;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int sub = lane / LPR, l = lane % LPR;
  const bool act = l * 8 < C;
  float gm[8], bt[8];
#pragma unroll
  for (int c = 0; c < 8; ++c) {
    gm[c] = act ? gamma[l * 8 + c] : 0.f;
    bt[c] = act ? beta[l * 8 + c] : 0.f;
  }
  const float inv_c = 1.0f / C;
  const int rows_per_block = 4 * RPW * UNR;
  for (int base = blockIdx.x * rows_per_block + wave * RPW * UNR; base < N; base += gridDim.x * rows_per_block) {
    u32x4 yv[UNR], sv[UNR];
    bool ok[UNR];
#pragma unroll
    for (int u = 0; u < UNR; ++u) {
      const int row = base + u * RPW + sub;
      ok[u] = act && row < N;
      yv[u] = u32x4{0u, 0u, 0u, 0u};
      sv[u] = u32x4{0u, 0u, 0u, 0u};
      if (ok[u]) {
        yv[u] = *reinterpret_cast<const u32x4*>(y + (size_t)row * C + l * 8);
        sv[u] = *reinterpret_cast<const u32x4*>(shortcut + (size_t)row * lds + l * 8);
      }
    }
#pragma unroll
    for (int u = 0; u < UNR; ++u) {
      float v[8];
#pragma unroll
      for (int c = 0; c < 4; ++c) {
        v[2 * c] = __builtin_bit_cast(float, yv[u][c] << 16);
        v[2 * c + 1] = __builtin_bit_cast(float, yv[u][c] & 0xFFFF0000u);
      }
      float s = ((v[0] + v[1]) + (v[2] + v[3])) + ((v[4] + v[5]) + (v[6] + v[7]));
      s = group_sum<LPR>(s);
      const float mean = s * inv_c;
      float q = 0.f;
#pragma unroll
      for (int c = 0; c < 8; ++c) { const float d = v[c] - mean; q += d * d; }
      if (!act) q = 0.f;                       // idle lanes hold zeros, not (0 - mean)^2
      q = group_sum<LPR>(q);
      const float rstd = rsqrtf(q * inv_c + LN_EPS);
      if (ok[u]) {
        u32x4 o4;
#pragma unroll
        for (int c = 0; c < 4; ++c) {
          const float s0 = __builtin_bit_cast(float, sv[u][c] << 16);
          const float s1 = __builtin_bit_cast(float, sv[u][c] & 0xFFFF0000u);
          const float r0 = s0 + branch_scale * ((v[2 * c] - mean) * rstd * gm[2 * c] + bt[2 * c]);
          const float r1 = s1 + branch_scale * ((v[2 * c + 1] - mean) * rstd * gm[2 * c + 1] + bt[2 * c + 1]);
          o4[c] = pack_bf16x2(r0, r1);
        }
        const int row = base + u * RPW + sub;
        *reinterpret_cast<u32x4*>(out + (size_t)row * ldo + l * 8) = o4;
      }
    }
  }
}

template <int NV>
__global__ __launch_bounds__(256) void downsample_ln_bf16_kernel(const u16* __restrict__ x, int ldx,
                                                                 const float* __restrict__ gamma,
                                                                 const float* __restrict__ beta, u16* __restrict__ out,
                                                                 int Z, int H, int W, int C) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int H2 = (H + 1) / 2, W2 = W / 2, C4 = 4 * C, nvec = C4 >> 2, cvec = C >> 2;
  const int N2 = Z * H2 * W2;
  for (int row = blockIdx.x * ROWS_PER_BLOCK + wave; row < N2; row += gridDim.x * ROWS_PER_BLOCK) {
    const int w2 = row % W2, h2 = (row / W2) % H2, z = row / (W2 * H2);
    f32x4 v[NV];
#pragma unroll
    for (int i = 0; i < NV; ++i) {
      const int f = lane + 64 * i;
      if (f < nvec) {
        const int quad = f / cvec, c4 = f - quad * cvec;
        const int h = 2 * h2 + (quad >> 1), w = 2 * w2 + (quad & 1);
        v[i] = h < H ? ld4(x + ((size_t)(z * H + h) * W + w) * ldx + 4 * c4) : f32x4{0.f, 0.f, 0.f, 0.f};
      }
    }
    row_layernorm<NV>(v, nvec, lane, C4, gamma, beta);
#pragma unroll
    for (int i = 0; i < NV; ++i)
      if (lane + 64 * i < nvec) st4(out + (size_t)row * C4 + 4 * (lane + 64 * i), v[i]);
  }
}

template <int NV>
__global__ __launch_bounds__(256) void upsample_ln_bf16_kernel(const u16* __restrict__ y, const float* __restrict__ gamma,
                                                               const float* __restrict__ beta, u16* __restrict__ out,
                                                               int Z, int H2, int W2, int H, int Co) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int Wf = 2 * W2, nvec = Co >> 2;
  const int N = Z * H * Wf;
  for (int row = blockIdx.x * ROWS_PER_BLOCK + wave; row < N; row += gridDim.x * ROWS_PER_BLOCK) {
    const int w = row % Wf, h = (row / Wf) % H, z = row / (Wf * H);
    const u16* src = y + ((size_t)(z * H2 + (h >> 1)) * W2 + (w >> 1)) * (4 * Co) + ((h & 1) * 2 + (w & 1)) * Co;
    f32x4 v[NV];
#pragma unroll
    for (int i = 0; i < NV; ++i)
      if (lane + 64 * i < nvec) v[i] = ld4(src + 4 * (lane + 64 * i));
    row_layernorm<NV>(v, nvec, lane, Co, gamma, beta);
#pragma unroll
    for (int i = 0; i < NV; ++i)
      if (lane + 64 * i < nvec) st4(out + (size_t)row * Co + 4 * (lane + 64 * i), v[i]);
  }
}

// ---- fast paths of the two resampling LayerNorms (round 3): the generic kernels above spend a whole wave on one row with 4
// channels (8 B) per lane and one row in flight -- at 521 280 rows of 192 channels (up-sampling) that is issue-bound, not
// HBM-bound: 152 / 189 us for 0.4 GB.  Same layout ideas as ln_residual_bf16_v8_kernel: 16-B accesses, gamma / beta in
// registers, several rows in flight per wave, persistent grid.
__device__ inline void unpack8(const u32x4 v, float* f) {
#pragma unroll
  for (int c = 0; c < 4; ++c) {
    f[2 * c] = __builtin_bit_cast(float, v[c] << 16);
    f[2 * c + 1] = __builtin_bit_cast(float, v[c] & 0xFFFF0000u);
  }
}

// Down-sampling (reference layers.py:441-454): one wave per output row of 4C channels, 16 channels (two 16-B loads from ONE of
// the four source tokens) per lane, C / 16 lanes per source token (C % 16 == 0, C <= 256), UNR rows in flight.
template <int UNR>
__global__ __launch_bounds__(256) void downsample_ln_bf16_v16_kernel(const u16* __restrict__ x, int ldx,
                                                                     const float* __restrict__ gamma,
                                                                     const float* __restrict__ beta, u16* __restrict__ out,
                                                                     int Z, int H, int W, int C) {
  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int lpq = C >> 4;
  const bool act = lane < 4 * lpq;
  const int quad = act ? lane / lpq : 0, c0 = (lane - quad * lpq) * 16;
  const int H2 = (H + 1) / 2, W2 = W / 2, C4 = 4 * C, N2 = Z * H2 * W2;
  float gm[16], bt[16];
#pragma unroll
  for (int c = 0; c < 16; ++c) {
    gm[c] = act ? gamma[lane * 16 + c] : 0.f;
    bt[c] = act ? beta[lane * 16 + c] : 0.f;
  }
  const float inv_c = 1.0f / C4;
  for (int base = (blockIdx.x * 4 + wave) * UNR; base < N2; base += gridDim.x * 4 * UNR) {
    u32x4 a[UNR], b[UNR];
#pragma unroll
    for (int u = 0; u < UNR; ++u) {
      const int row = base + u;
      a[u] = u32x4{0u, 0u, 0u, 0u};
      b[u] = a[u];
      if (row < N2) {
        const int w2 = row % W2, h2 = (row / W2) % H2, z = row / (W2 * H2);
        const int h = 2 * h2 + (quad >> 1), w = 2 * w2 + (quad & 1);
        if (act && h < H) {                              // the padded latitude row (reference layers.py:441) is zeros
          const u16* p = x + ((size_t)(z * H + h) * W + w) * ldx + c0;
          a[u] = *reinterpret_cast<const u32x4*>(p);
          b[u] = *reinterpret_cast<const u32x4*>(p + 8);
        }
      }
    }
#pragma unroll
    for (int u = 0; u < UNR; ++u) {
      float v[16];
      unpack8(a[u], v);
      unpack8(b[u], v + 8);
      float s = 0.f;
#pragma unroll
      for (int c = 0; c < 16; c += 4) s += (v[c] + v[c + 1]) + (v[c + 2] + v[c + 3]);
      const float mean = wave_sum(s) * inv_c;
      float q = 0.f;
#pragma unroll
      for (int c = 0; c < 16; ++c) { const float d = v[c] - mean; q += d * d; }
      if (!act) q = 0.f;
      const float rstd = rsqrtf(wave_sum(q) * inv_c + LN_EPS);
      const int row = base + u;
      if (act && row < N2) {
        u32x4 o0, o1;
#pragma unroll
        for (int c = 0; c < 4; ++c) {
          o0[c] = pack_bf16x2((v[2 * c] - mean) * rstd * gm[2 * c] + bt[2 * c], (v[2 * c + 1] - mean) * rstd * gm[2 * c + 1] + bt[2 * c + 1]);
          o1[c] = pack_bf16x2((v[8 + 2 * c] - mean) * rstd * gm[8 + 2 * c] + bt[8 + 2 * c],
                              (v[9 + 2 * c] - mean) * rstd * gm[9 + 2 * c] + bt[9 + 2 * c]);
        }
        u16* p = out + (size_t)row * C4 + lane * 16;
        *reinterpret_cast<u32x4*>(p) = o0;
        *reinterpret_cast<u32x4*>(p + 8) = o1;
      }
    }
  }
}

// Up-sampling (reference layers.py:480-495): LPR = 32 lanes per output row of Co <= 256 channels (8 per lane), two rows per wave,
// UNR row pairs in flight; the source of row (z, h, w) is the (h & 1, w & 1) quarter of coarse token (z, h / 2, w / 2).
template <int UNR>
__global__ __launch_bounds__(256) void upsample_ln_bf16_v8_kernel(const u16* __restrict__ y, const float* __restrict__ gamma,
                                                                  const float* __restrict__ beta, u16* __restrict__ out,
                                                                  int Z, int H2, int W2, int H, int Co) {
  constexpr int LPR = 32, RPW = 2;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int sub = lane / LPR, l = lane % LPR;
  const bool act = l * 8 < Co;
  const int Wf = 2 * W2, N = Z * H * Wf;
  float gm[8], bt[8];
#pragma unroll
  for (int c = 0; c < 8; ++c) {
    gm[c] = act ? gamma[l * 8 + c] : 0.f;
    bt[c] = act ? beta[l * 8 + c] : 0.f;
  }
  const float inv_c = 1.0f / Co;
  for (int base = (blockIdx.x * 4 + wave) * RPW * UNR; base < N; base += gridDim.x * 4 * RPW * UNR) {
    u32x4 a[UNR];
#pragma unroll
    for (int u = 0; u < UNR; ++u) {
      const int row = base + u * RPW + sub;
      a[u] = u32x4{0u, 0u, 0u, 0u};
      if (act && row < N) {
        const int w = row % Wf, h = (row / Wf) % H, z = row / (Wf * H);
        a[u] = *reinterpret_cast<const u32x4*>(y + ((size_t)(z * H2 + (h >> 1)) * W2 + (w >> 1)) * (4 * Co) +
                                               ((h & 1) * 2 + (w & 1)) * Co + l * 8);
      }
    }
#pragma unroll
    for (int u = 0; u < UNR; ++u) {
      float v[8];
      unpack8(a[u], v);
      const float s = group_sum<LPR>(((v[0] + v[1]) + (v[2] + v[3])) + ((v[4] + v[5]) + (v[6] + v[7])));
      const float mean = s * inv_c;
      float q = 0.f;
#pragma unroll
      for (int c = 0; c < 8; ++c) { const float d = v[c] - mean; q += d * d; }
      if (!act) q = 0.f;
      const float rstd = rsqrtf(group_sum<LPR>(q) * inv_c + LN_EPS);
      const int row = base + u * RPW + sub;
      if (act && row < N) {
        u32x4 o;
#pragma unroll
        for (int c = 0; c < 4; ++c)
          o[c] = pack_bf16x2((v[2 * c] - mean) * rstd * gm[2 * c] + bt[2 * c], (v[2 * c + 1] - mean) * rstd * gm[2 * c + 1] + bt[2 * c + 1]);
        *reinterpret_cast<u32x4*>(out + (size_t)row * Co + l * 8) = o;
      }
    }
  }
}

// patch embed gather, bf16 out; the surface matrix is zero-padded from 112 to 128 columns (K multiple of 64 for the
// bf16 GEMM; the weight shadow is padded the same way).
constexpr int EMB_TOK = 64;

__global__ __launch_bounds__(256) void patch_embed_gather_bf16_kernel(
    const float* __restrict__ input, const float* __restrict__ input_surface, const float* __restrict__ s_mean,
    const float* __restrict__ s_std, const float* __restrict__ u_mean, const float* __restrict__ u_std,
    const float* __restrict__ maps, const float* __restrict__ const_h, u16* __restrict__ a_surface,
    u16* __restrict__ a_upper, int LAT, int LON, int H4, int W4, int chunks, int levels_reversed) {
  constexpr int TLD = 200;               // tile row stride in bf16: rows 16-B aligned
  __shared__ __attribute__((aligned(16))) u16 tile[EMB_TOK * TLD];
  const int chunk = blockIdx.x % chunks, h4 = (blockIdx.x / chunks) % H4, zp = blockIdx.x / (chunks * H4);
  const int w0 = chunk * EMB_TOK;
  const int ntok = min(EMB_TOK, W4 - w0);
  const int tid = threadIdx.x;
  const int ncol = zp == 0 ? 112 : 192;
  const int nrun = ncol / 4;
  const size_t plane = (size_t)LAT * LON;
  for (int run = tid >> 6; run < nrun; run += 4) {
    int c, pz, ph;
    if (zp == 0) { c = run >> 2; pz = 0; ph = run & 3; } else { c = run >> 3; pz = (run >> 2) & 1; ph = run & 3; }
    const int lat = 4 * h4 + ph;
    const float* src = nullptr;
    float mean = 0.f, sd = 1.f;
    bool valid = lat < LAT;
    if (zp == 0) {
      if (c < 4) { src = input_surface + c * plane + (size_t)lat * LON; mean = s_mean[c]; sd = s_std[c]; }
      else { src = maps + (size_t)(c - 4) * (4 * H4) * LON + (size_t)lat * LON; valid = true; }
    } else {
      const int lev = 2 * (zp - 1) + pz;
      valid = valid && lev < 13;
      if (valid) {
        if (c < 5) {
          src = input + ((size_t)c * 13 + (levels_reversed ? 12 - lev : lev)) * plane + (size_t)lat * LON;   // see rowops.hip
          mean = u_mean[(12 - lev) * 5 + c]; sd = u_std[(12 - lev) * 5 + c];
        } else {
          src = const_h + (size_t)lev * plane + (size_t)lat * LON;
        }
      }
    }
    const bool norm = (zp == 0) ? (c < 4) : (c < 5);
    for (int tk = (tid & 63); tk < ntok; tk += 64) {      // LON % 4 == 0: a token's 4 longitudes are one aligned float4
      f32x4 v = {0.f, 0.f, 0.f, 0.f};
      if (valid) {
        v = *reinterpret_cast<const f32x4*>(src + 4 * (w0 + tk));
        if (norm) {
#pragma unroll
          for (int e = 0; e < 4; ++e) v[e] = (v[e] - mean) / sd;
        }
      }
      *reinterpret_cast<u32x2*>(&tile[tk * TLD + run * 4]) = u32x2{pack_bf16x2(v[0], v[1]), pack_bf16x2(v[2], v[3])};
    }
  }
  __syncthreads();
  const int ocol = zp == 0 ? 128 : 192;
  u16* dst = zp == 0 ? a_surface + ((size_t)h4 * W4 + w0) * 128 : a_upper + (((size_t)(zp - 1) * H4 + h4) * W4 + w0) * 192;
  const int c8n = ocol / 8;
  for (int i = tid; i < ntok * c8n; i += 256) {
    const int tk = i / c8n, c8 = i - tk * c8n;
    reinterpret_cast<u32x4*>(dst)[i] =
        c8 * 8 < ncol ? *reinterpret_cast<const u32x4*>(&tile[tk * TLD + c8 * 8]) : u32x4{0u, 0u, 0u, 0u};
  }
}

int row_grid(int rows) {
  constexpr int cap = 8192;
  int blocks = (rows + ROWS_PER_BLOCK - 1) / ROWS_PER_BLOCK;
  return blocks < cap ? blocks : cap;
}

}  // namespace

#define PANGU_NVB(C_, KERNEL, ...)                                                   \
  do {                                                                               \
    if ((C_) <= 256) hipLaunchKernelGGL(KERNEL<1>, g, b, 0, s, __VA_ARGS__);         \
    else if ((C_) <= 512) hipLaunchKernelGGL(KERNEL<2>, g, b, 0, s, __VA_ARGS__);    \
    else hipLaunchKernelGGL(KERNEL<4>, g, b, 0, s, __VA_ARGS__);                     \
  } while (0)

extern "C" int pangu_ln_residual_fwd_bf16(pangu_stream_t stream, const void* y, const void* shortcut, int lds,
                                          const float* gamma, const float* beta, void* out, int ldo, int N, int C,
                                          float branch_scale) {
  if (!y || !shortcut || !gamma || !beta || !out) return PANGU_E_NULL;
  if (N <= 0 || C <= 0 || (C & 3) || C > 1024 || lds < C || ldo < C || (lds & 3) || (ldo & 3)) return PANGU_E_SHAPE;
  hipStream_t s = (hipStream_t)stream;
  dim3 g(row_grid(N)), b(256);
  if ((C & 7) == 0 && C <= 512 && (lds & 7) == 0 && (ldo & 7) == 0) {
    constexpr int cap = 2048;   // 8 workgroups per CU, grid-stride: workgroup launch rate limits smaller blocks
    if (C <= 256) {
      const int blocks = (N + 15) / 16;
      hipLaunchKernelGGL(ln_residual_bf16_v8_kernel<32>, dim3(blocks < cap ? blocks : cap), b, 0, s, (const u16*)y,
                         (const u16*)shortcut, lds, gamma, beta, (u16*)out, ldo, N, C, branch_scale);
    } else {
      const int blocks = (N + 7) / 8;
      hipLaunchKernelGGL(ln_residual_bf16_v8_kernel<64>, dim3(blocks < cap ? blocks : cap), b, 0, s, (const u16*)y,
                         (const u16*)shortcut, lds, gamma, beta, (u16*)out, ldo, N, C, branch_scale);
    }
    return pangu_launch_status();
  }
  PANGU_NVB(C, ln_residual_bf16_kernel, (const u16*)y, (const u16*)shortcut, lds, gamma, beta, (u16*)out, ldo, N, C, branch_scale);
  return pangu_launch_status();
}

extern "C" int pangu_downsample_ln_fwd_bf16(pangu_stream_t stream, const void* x, int ldx, const float* gamma,
                                            const float* beta, void* out, int Z, int H, int W, int C) {
  if (!x || !gamma || !beta || !out) return PANGU_E_NULL;
  if (Z <= 0 || H <= 0 || W <= 0 || (W & 1) || (C & 3) || 4 * C > 1024 || ldx < C || (ldx & 3)) return PANGU_E_SHAPE;
  hipStream_t s = (hipStream_t)stream;
  dim3 g(row_grid(Z * ((H + 1) / 2) * (W / 2))), b(256);
  constexpr bool fast = true;      // 16-B fast path where the shape allows (the generic one-row-per-wave kernel below otherwise)
  if (fast && (C & 15) == 0 && C <= 256 && (ldx & 7) == 0) {
    const int rows = Z * ((H + 1) / 2) * (W / 2), blocks = (rows + 7) / 8;
    hipLaunchKernelGGL(downsample_ln_bf16_v16_kernel<2>, dim3(blocks < 2048 ? blocks : 2048), b, 0, s, (const u16*)x, ldx, gamma,
                       beta, (u16*)out, Z, H, W, C);
    return pangu_launch_status();
  }
  PANGU_NVB(4 * C, downsample_ln_bf16_kernel, (const u16*)x, ldx, gamma, beta, (u16*)out, Z, H, W, C);
  return pangu_launch_status();
}

extern "C" int pangu_upsample_ln_fwd_bf16(pangu_stream_t stream, const void* y, const float* gamma, const float* beta,
                                          void* out, int Z, int H2, int W2, int H, int Co) {
  if (!y || !gamma || !beta || !out) return PANGU_E_NULL;
  if (Z <= 0 || H2 <= 0 || W2 <= 0 || H <= 0 || H > 2 * H2 || (Co & 3) || Co > 1024) return PANGU_E_SHAPE;
  hipStream_t s = (hipStream_t)stream;
  dim3 g(row_grid(Z * H * 2 * W2)), b(256);
  constexpr bool fast = true;      // 16-B fast path where the shape allows (the generic one-row-per-wave kernel below otherwise)
  if (fast && (Co & 7) == 0 && Co <= 256) {
    const int rows = Z * H * 2 * W2, blocks = (rows + 15) / 16;
    hipLaunchKernelGGL(upsample_ln_bf16_v8_kernel<2>, dim3(blocks < 2048 ? blocks : 2048), b, 0, s, (const u16*)y, gamma, beta,
                       (u16*)out, Z, H2, W2, H, Co);
    return pangu_launch_status();
  }
  PANGU_NVB(Co, upsample_ln_bf16_kernel, (const u16*)y, gamma, beta, (u16*)out, Z, H2, W2, H, Co);
  return pangu_launch_status();
}

extern "C" int pangu_patch_embed_gather_bf16(pangu_stream_t stream, const float* input, const float* input_surface,
                                             const float* surface_mean, const float* surface_std,
                                             const float* upper_mean, const float* upper_std, const float* maps,
                                             const float* const_h, void* a_surface, void* a_upper, int LAT, int LON,
                                             int levels_reversed) {
  if (!input || !input_surface || !surface_mean || !surface_std || !upper_mean || !upper_std || !maps || !const_h ||
      !a_surface || !a_upper)
    return PANGU_E_NULL;
  if (LAT <= 0 || LON <= 0 || (LON & 3)) return PANGU_E_SHAPE;
  const int H4 = (LAT + 3) / 4, W4 = LON / 4, chunks = (W4 + EMB_TOK - 1) / EMB_TOK;
  hipLaunchKernelGGL(patch_embed_gather_bf16_kernel, dim3(8 * H4 * chunks), dim3(256), 0, (hipStream_t)stream, input,
                     input_surface, surface_mean, surface_std, upper_mean, upper_std, maps, const_h, (u16*)a_surface,
                     (u16*)a_upper, LAT, LON, H4, W4, chunks, levels_reversed != 0);
  return pangu_launch_status();
}
