// Earth-specific 3D window attention, fp32 in / fp32 out, contractions as exact-split bf16 MFMA products, gfx950.  Inference only:
// no lse is written (training keeps attn_f32.hip, whose backward recomputes from its lse).
//
// Same contract and decomposition as attn_f32.hip: one workgroup per (longitude window l, window type t, head), 144 tokens x 32
// dims; roll / pad / partition / reverse / crop are address arithmetic (win_src_token), the shift mask is closed form, pad tokens
// read qkv_bias, the expanded and the compact bias table put the same values into the same registers (bit-identical modes), and
// the scores are computed TRANSPOSED so that the probability registers are the B operand of the second product.
//
// Every fp32 operand is the exact sum of three bf16 values (split_f32.h: hi + mid + lo); each product is six
// v_mfma_f32_16x16x32_bf16 into ONE fp32 accumulator, small terms first: (lo,hi) (hi,lo) (mid,mid) (mid,hi) (hi,mid) (hi,hi).  The
// three dropped terms are below 2^-24 of the product.
//   S^T = bias^T + K (scale Q)^T: q * scale in fp32 as in attn_f32.hip, then split in registers; K is split ONCE per workgroup when
//     it is staged, into three [144 keys][32 d] bf16 planes (kswz of attn_bf16_tile.h).  k = head dim = 32: six MFMAs per key tile,
//     the bias row is the accumulators' initial value.
//   O^T = V^T P^T: the UNNORMALISED probabilities are split in registers (1 / sum is applied to the fp32 result); the key order of
//     the score tiles is the interleaved one of attn_bf16_tile.h (key_of), so a lane's eight values of a tile pair are eight
//     consecutive keys = one B fragment.  V is split once when staged; keys 0 .. 127 are stored TRANSPOSED as three [32 d][128 keys]
//     bf16 planes (vt128_off: conflict-free ds_read_b128 fragments); a staging thread holds the same four dims of two neighbouring
//     keys, so every plane write is a whole dword.  The 16-key tail is one k-step of the 16-wide MFMA whose V fragments (12
//     registers) every wave loads and splits for itself: they are the same for its three query tiles.
// Limits: a probability below the bf16 normal range (about exp(-87) of the row maximum; the -100 of the shift mask produces such
// values) loses its mid / lo parts or all of itself to underflow.  Against a row sum >= 1 (the maximum contributes exp(0)) that is
// below 1e-37 relative: far under fp32 rounding.  |q k| products far outside fp32 range are not guarded, as in attn_f32.hip.
//
// LDS and occupancy (profiles/attn_f32_split_speed.md).  The kernel is bound by the sum of its matrix and vector issue cycles per
// tile (114 MFMAs + about 550 VALU instructions, half of them the splits) and, around that, by how well the staging of one
// workgroup (global loads, split, LDS writes) hides under the tiles of the others: with no tile work a launch takes 0.32 ms at
// C = 192, with no global loads 0.48 ms, with both 0.62 ms at two workgroups per CU.  Six full planes are 55 296 B, 683 B too many
// for three workgroups in a CU's 160 KB; with the V tail in registers the image is 3 x 9216 B (K) + 3 x 8192 B (V^T) = 52 224 B,
// THREE workgroups of three waves per CU (<= 168 VGPRs), and the same launch takes 0.58 ms (fp32-MFMA kernel: 0.63 - 0.79 ms).
// Measured and not kept: nine waves per workgroup with one tile each at two workgroups per CU (18 waves per CU, 95 VGPRs): level
// with three waves at the same LDS image (0.60 - 0.66 ms), slower with the expanded bias table at C = 384.
#include "common.h"

#include "attn_bf16_tile.h"
#include "split_f32.h"

namespace {

constexpr int KPLANE = PANGU_WTOK * 64;                // one bf16 plane of K: [144 keys][64 B]
constexpr int VPLANE = 32 * 256;                       // one bf16 plane of V^T: [32 d][128 keys]

// byte offset of (d, key < 128) in a V^T plane: 256-byte rows = 16 chunks of 8 keys, chunk XOR (d & 15).  A fragment read takes, per
// 16 lanes of one k-step, the rows d = 0 .. 15 (or 16 .. 31) at one chunk: 16 distinct 16-byte slots of the 256-byte bank window
// (also under the real ds_read_b128 lane groups, which pair 8 rows of lane group lg with the other 8 rows of lg ^ 1).
__device__ inline int vt128_off(int d, int key) { return d * 256 + ((((key >> 3) ^ d) & 15) << 4) + (key & 7) * 2; }
constexpr int NW = 3, NT = 64 * NW, TPW = 9 / NW;      // waves, threads, 16-query tiles per wave
constexpr int UPT = 576 / NT;                          // staging units per thread
static_assert(3 * (3 * KPLANE + 3 * VPLANE) <= 160 * 1024, "three workgroups per CU");

typedef f32x4 f32x4_al4 __attribute__((aligned(4)));
constexpr int COMPACT_BIAS = 3312;

// One query row of the bias tile in the lane's key order: s[j][r] <- bias[qn][key_of(j, 4lg + r)], four consecutive keys per tile.
// COMPACT: the closed-form position index of attn_f32.hip (load_bias_row): the four keys share (zk, hk) and their entries are four
// consecutive floats in falling order.
template <bool COMPACT>
__device__ __forceinline__ void load_bias_row_il(f32x4 (&s)[9], const float* __restrict__ bias_tile, int qn, int lg) {
  if (COMPACT) {
    const int zq = qn / 72, hq = (qn / 12) % 6, wq = qn % 12;
#pragma unroll
    for (int j = 0; j < 9; ++j) {
      const int k0 = key_of(j, 4 * lg);
      const int zk = k0 / 72, hk = (k0 / 12) % 6, wk = k0 % 12;
      const int idx = (zq + 2 * zk) * 828 + (hq + 6 * hk) * 23 + (wq - wk + 11);      // key k0; key k0 + r: idx - r
      const f32x4 v = *reinterpret_cast<const f32x4_al4*>(bias_tile + idx - 3);
      s[j] = f32x4{v[3], v[2], v[1], v[0]};
    }
  } else {
    const float* brow = bias_tile + (size_t)qn * PANGU_WTOK;
#pragma unroll
    for (int j = 0; j < 9; ++j) s[j] = *reinterpret_cast<const f32x4*>(brow + key_of(j, 4 * lg));
  }
}

typedef short bf16x4s __attribute__((ext_vector_type(4)));

// acc += a b with a = ah + am + al, b = bh + bm + bl: the six products of split_f32.h, small terms first
#define PANGU_SPLIT6(MFMA, acc, ah, am, al, bh, bm, bl) \
  do {                                                  \
    acc = MFMA(al, bh, acc, 0, 0, 0);                   \
    acc = MFMA(ah, bl, acc, 0, 0, 0);                   \
    acc = MFMA(am, bm, acc, 0, 0, 0);                   \
    acc = MFMA(am, bh, acc, 0, 0, 0);                   \
    acc = MFMA(ah, bm, acc, 0, 0, 0);                   \
    acc = MFMA(ah, bh, acc, 0, 0, 0);                   \
  } while (0)

// One 16-query tile of one wave: scores (s enters holding the bias row), mask, softmax, PV, store.  q0 / q1: this lane's
// q * scale, d = 8lg .. 8lg+3 / 8lg+4 .. 8lg+7.  Fragment addresses: the closed forms of attn_tile (attn_bf16_tile.h).
template <bool SHIFTED>
__device__ __forceinline__ void split_tile(const unsigned char* Kp, const unsigned char* Vp, const f32x4 q0, const f32x4 q1,
                                           f32x4 (&s)[9], int qn, int qtok, int lq, int lg, bool zcut, bool hcut,
                                           unsigned long long kz_bits, unsigned long long kh_bits,
                                           const bf16x4s (&vtail)[2][3], float* __restrict__ out, int C, int hd) {
  // V^T fragment of k-step u: vt128_off(d, 32u + 8lg) = 256 d + (16 (lg ^ lq) ^ 64u), d = lq or 16 + lq
  int ke = kswz(key_of(0, lq), lg), kt = kswz(128 + lq, lg);
  int vrow = lq * 256, vx = ((lg ^ lq) & 15) << 4;
  asm volatile("" : "+v"(ke), "+v"(kt), "+v"(vrow), "+v"(vx));
  const int ko = ke ^ 32;

  // ---- S^T += K (scale Q)^T: key tiles three at a time, product-major, so consecutive MFMAs hit different accumulators
  bf16x8 qh, qm, ql;
  pangu_split::split8(q0, q1, qh, qm, ql);
#pragma unroll
  for (int j0 = 0; j0 < 9; j0 += 3) {
    bf16x8 kf[3][3];                                   // [tile][plane hi, mid, lo]
#pragma unroll
    for (int jj = 0; jj < 3; ++jj) {
      const int j = j0 + jj;
      const int ka = j == 8 ? kt : ((j & 1) ? ko : ke) + 2048 * (j >> 1) + 256 * (j & 1);
#pragma unroll
      for (int p = 0; p < 3; ++p) kf[jj][p] = *reinterpret_cast<const bf16x8*>(Kp + p * KPLANE + ka);
    }
#define PANGU_S3(KP, QF)                                                                                              \
  _Pragma("unroll") for (int jj = 0; jj < 3; ++jj) s[j0 + jj] =                                                       \
      __builtin_amdgcn_mfma_f32_16x16x32_bf16(kf[jj][KP], QF, s[j0 + jj], 0, 0, 0)
    PANGU_S3(2, qh);
    PANGU_S3(0, ql);
    PANGU_S3(1, qm);
    PANGU_S3(1, qh);
    PANGU_S3(0, qm);
    PANGU_S3(0, qh);
#undef PANGU_S3
  }

  // ---- shift mask (closed form, only in the cut window types), softmax numerators
  float mx = -INFINITY;
  if (SHIFTED) {
    if (zcut || hcut) {
      const bool zq = qn >= 72, hq = ((qn / 12) % 6) < 3;
      const unsigned long long zsel = zq ? ~kz_bits : kz_bits;      // keys whose z-half differs from the query's
      const unsigned long long hsel = hq ? ~kh_bits : kh_bits;
      const unsigned long long cut = (zcut ? zsel : 0ull) | (hcut ? hsel : 0ull);
#pragma unroll
      for (int j = 0; j < 9; ++j)
#pragma unroll
        for (int r = 0; r < 4; ++r)
          if ((cut >> (4 * j + r)) & 1ull) s[j][r] += -100.0f;
    }
  }
#pragma unroll
  for (int j = 0; j < 9; ++j)
#pragma unroll
    for (int r = 0; r < 4; ++r) mx = fmaxf(mx, s[j][r]);
  mx = fmaxf(mx, __shfl_xor(mx, 16, 64));
  mx = fmaxf(mx, __shfl_xor(mx, 32, 64));
  float sum = 0.f;
  const float nmx = -mx * 1.4426950408889634f;      // exp(s - mx) = exp2(s*log2e - mx*log2e): one fma + v_exp_f32
#pragma unroll
  for (int j = 0; j < 9; ++j)
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const float e = __builtin_amdgcn_exp2f(fmaf(s[j][r], 1.4426950408889634f, nmx));
      s[j][r] = e;
      sum += e;
    }
  sum += __shfl_xor(sum, 16, 64);
  sum += __shfl_xor(sum, 32, 64);

  // ---- O^T = V^T P^T.  k-step u < 4: fragment element e <-> key 32u + 8lg + e; tail: element e < 4 <-> key 128 + 4lg + e
  f32x4 o0 = {0.f, 0.f, 0.f, 0.f}, o1 = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
  for (int u = 0; u < 4; ++u) {
    bf16x8 ph, pm, pl, v0[3], v1[3];
    const int a0 = vrow + (vx ^ (64 * u)), a1 = a0 + 16 * 256;
#pragma unroll
    for (int p = 0; p < 3; ++p) {
      v0[p] = *reinterpret_cast<const bf16x8*>(Vp + p * VPLANE + a0);
      v1[p] = *reinterpret_cast<const bf16x8*>(Vp + p * VPLANE + a1);
    }
    pangu_split::split8(s[2 * u], s[2 * u + 1], ph, pm, pl);
    // the two d-tiles alternate: two independent accumulator chains
#define PANGU_O2(VP, PF)                                                    \
  o0 = __builtin_amdgcn_mfma_f32_16x16x32_bf16(v0[VP], PF, o0, 0, 0, 0);    \
  o1 = __builtin_amdgcn_mfma_f32_16x16x32_bf16(v1[VP], PF, o1, 0, 0, 0)
    PANGU_O2(2, ph);
    PANGU_O2(0, pl);
    PANGU_O2(1, pm);
    PANGU_O2(1, ph);
    PANGU_O2(0, pm);
    PANGU_O2(0, ph);
#undef PANGU_O2
  }
  {
    unsigned h0, h1, m0, m1, l0, l1;
    pangu_split::split2(s[8][0], s[8][1], h0, m0, l0);
    pangu_split::split2(s[8][2], s[8][3], h1, m1, l1);
    const bf16x4s ph = __builtin_bit_cast(bf16x4s, u32x2{h0, h1}), pm = __builtin_bit_cast(bf16x4s, u32x2{m0, m1}),
                  pl = __builtin_bit_cast(bf16x4s, u32x2{l0, l1});
    PANGU_SPLIT6(__builtin_amdgcn_mfma_f32_16x16x16bf16_1k, o0, vtail[0][0], vtail[0][1], vtail[0][2], ph, pm, pl);
    PANGU_SPLIT6(__builtin_amdgcn_mfma_f32_16x16x16bf16_1k, o1, vtail[1][0], vtail[1][1], vtail[1][2], ph, pm, pl);
  }

  // lane holds O^T[d = 16dt + 4lg + r][query]
  if (qtok >= 0) {
    const float inv = 1.0f / sum;
    float* dst = out + (size_t)qtok * C + hd * 32 + lg * 4;
    *reinterpret_cast<f32x4*>(dst) = o0 * inv;
    *reinterpret_cast<f32x4*>(dst + 16) = o1 * inv;
  }
}

template <bool SHIFTED, bool COMPACT>
__global__ __launch_bounds__(NT, 3) void window_attn_f32_split_kernel(const float* __restrict__ qkv,
                                                                         const float* __restrict__ qkv_bias,
                                                                         const float* __restrict__ esb, float* __restrict__ out,
                                                                         WinGeom g, int C, int heads, int n_pairs) {
  __shared__ __attribute__((aligned(16))) unsigned char Kp[3 * KPLANE];
  __shared__ __attribute__((aligned(16))) unsigned char Vp[3 * VPLANE];

  // block -> (pair=(t,head), l): blocks b, b+8, .. share an XCD and walk l for one pair (attn_f32.hip)
  const int b = blockIdx.x;
  const int xcd = b & 7, local = b >> 3;
  const int pair = (local / g.nLon) * 8 + xcd;
  const int l = local % g.nLon;
  if (pair >= n_pairs) return;
  const int t = pair / heads, hd = pair - t * heads;

  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int lq = lane & 15, lg = lane >> 4;
  const int C3 = 3 * C;
  const float scale = 0.17677669529663687f;   // 32^-0.5, reference layers.py:289
  const float* bias_tile = esb + (size_t)(t * heads + hd) * (COMPACT ? COMPACT_BIAS : PANGU_WTOK * PANGU_WTOK);

  // ---- every up-front global load, back to back.  K unit f: key f >> 2, dims 8 (f & 3) .. +7.  V unit f: keys 2 (f >> 3) and
  // 2 (f >> 3) + 1 (< 128), dims 4 (f & 7) .. +3.
  f32x4 k0[UPT], k1[UPT], va[UPT], vb[UPT];
#pragma unroll
  for (int i = 0; i < UPT; ++i) {
    const int f = tid + NT * i;
    {
      const int tok = win_src_token(g, l, t, f >> 2, SHIFTED);
      const float* src = (tok >= 0 ? qkv + (size_t)tok * C3 : qkv_bias) + C + hd * 32 + (f & 3) * 8;
      k0[i] = *reinterpret_cast<const f32x4*>(src);
      k1[i] = *reinterpret_cast<const f32x4*>(src + 4);
    }
    {
      const int n = 2 * (f >> 3), c = (f & 7) * 4;
      if (n < 128) {
        const int ta = win_src_token(g, l, t, n, SHIFTED), tb = win_src_token(g, l, t, n + 1, SHIFTED);
        va[i] = *reinterpret_cast<const f32x4*>((ta >= 0 ? qkv + (size_t)ta * C3 : qkv_bias) + 2 * C + hd * 32 + c);
        vb[i] = *reinterpret_cast<const f32x4*>((tb >= 0 ? qkv + (size_t)tb * C3 : qkv_bias) + 2 * C + hd * 32 + c);
      }
    }
  }
  int qtok[TPW];
  f32x4 q0[TPW], q1[TPW];
#pragma unroll
  for (int i = 0; i < TPW; ++i) {
    const int qn = (wave + NW * i) * 16 + lq;
    qtok[i] = win_src_token(g, l, t, qn, SHIFTED);
    const float* src = (qtok[i] >= 0 ? qkv + (size_t)qtok[i] * C3 : qkv_bias) + hd * 32 + lg * 8;
    q0[i] = *reinterpret_cast<const f32x4*>(src);
    q1[i] = *reinterpret_cast<const f32x4*>(src + 4);
  }
  // the 16-key tail of V stays out of LDS: every wave holds its own tail fragments (keys 128 + 4lg + r, d = lq and 16 + lq)
  float vta[2][4];
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    const int tok = win_src_token(g, l, t, 128 + 4 * lg + r, SHIFTED);
    const float* src = (tok >= 0 ? qkv + (size_t)tok * C3 : qkv_bias) + 2 * C + hd * 32 + lq;
    vta[0][r] = src[0];
    vta[1][r] = src[16];
  }

  bool zcut = false, hcut = false;
  // per-lane key-class bits (bit 4j+r <-> key key_of(j, 4lg+r)): kz = key in the upper z-plane, kh = key in rows hi<3
  unsigned long long kz_bits = 0ull, kh_bits = 0ull;
  if (SHIFTED) {
    const int zwin = t / g.nHw, hwin = t - zwin * g.nHw;
    zcut = zwin == g.nZw - 1;
    hcut = hwin == g.nHw - 1;
#pragma unroll
    for (int j = 0; j < 9; ++j)
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int kn = key_of(j, lg * 4 + r);
        if (kn >= 72) kz_bits |= 1ull << (4 * j + r);
        if (((kn / 12) % 6) < 3) kh_bits |= 1ull << (4 * j + r);
      }
  }

  // ---- split and stage: K planes [key][32 d] (16-B writes), V^T planes [d][key] (the two keys of a unit fill one dword)
#pragma unroll
  for (int i = 0; i < UPT; ++i) {
    const int f = tid + NT * i;
    bf16x8 h, m, lo;
    pangu_split::split8(k0[i], k1[i], h, m, lo);
    const int ka = kswz(f >> 2, f & 3);
    *reinterpret_cast<bf16x8*>(Kp + ka) = h;
    *reinterpret_cast<bf16x8*>(Kp + KPLANE + ka) = m;
    *reinterpret_cast<bf16x8*>(Kp + 2 * KPLANE + ka) = lo;
    const int n = 2 * (f >> 3), c = (f & 7) * 4;
    if (n < 128) {
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        unsigned vh, vm, vl;
        pangu_split::split2(va[i][e], vb[i][e], vh, vm, vl);
        const int a = vt128_off(c + e, n);
        *reinterpret_cast<unsigned*>(Vp + a) = vh;
        *reinterpret_cast<unsigned*>(Vp + VPLANE + a) = vm;
        *reinterpret_cast<unsigned*>(Vp + 2 * VPLANE + a) = vl;
      }
    }
  }
  bf16x4s vtail[2][3];
#pragma unroll
  for (int dt = 0; dt < 2; ++dt) {
    unsigned h0, h1, m0, m1, l0, l1;
    pangu_split::split2(vta[dt][0], vta[dt][1], h0, m0, l0);
    pangu_split::split2(vta[dt][2], vta[dt][3], h1, m1, l1);
    vtail[dt][0] = __builtin_bit_cast(bf16x4s, u32x2{h0, h1});
    vtail[dt][1] = __builtin_bit_cast(bf16x4s, u32x2{m0, m1});
    vtail[dt][2] = __builtin_bit_cast(bf16x4s, u32x2{l0, l1});
  }
#pragma unroll
  for (int i = 0; i < TPW; ++i) { q0[i] *= scale; q1[i] *= scale; }
  // the first tile's bias row is requested once the staged values' registers are free (held from the start, 36 more registers
  // live across the staging: spills at three workgroups per CU)
  f32x4 sA[9], sB[9];
  load_bias_row_il<COMPACT>(sA, bias_tile, wave * 16 + lq, lg);
  __syncthreads();

#pragma unroll
  for (int i = 0; i < TPW; ++i) {
    // the bias row of tile i+1 is requested before tile i computes
    f32x4 (&sc)[9] = (i & 1) ? sB : sA;
    f32x4 (&sn)[9] = (i & 1) ? sA : sB;
    if (i + 1 < TPW) load_bias_row_il<COMPACT>(sn, bias_tile, (wave + NW * (i + 1)) * 16 + lq, lg);
    split_tile<SHIFTED>(Kp, Vp, q0[i], q1[i], sc, (wave + NW * i) * 16 + lq, qtok[i], lq, lg, zcut, hcut, kz_bits, kh_bits,
                        vtail, out, C, hd);
  }
}

int check_split_geom(int Z, int H, int W) {
  if (Z <= 0 || H <= 0 || W <= 0) return PANGU_E_SHAPE;
  if (Z % PANGU_WZ || (H + PANGU_PAD_H) % PANGU_WH || W % PANGU_WW) return PANGU_E_SHAPE;
  return PANGU_OK;
}

}  // namespace

static int launch_attn_split(pangu_stream_t stream, const float* qkv, const float* qkv_bias, const float* esb, float* out,
                             int Z, int H, int W, int C, int heads, int shifted, bool compact) {
  if (!qkv || !qkv_bias || !esb || !out) return PANGU_E_NULL;
  if (int e = check_split_geom(Z, H, W)) return e;
  if (heads <= 0 || C != heads * PANGU_HEAD_DIM) return PANGU_E_SHAPE;
  const WinGeom g = make_geom(Z, H, W);
  const int n_pairs = g.types * heads;
  const int grid = ((n_pairs + 7) / 8) * 8 * g.nLon;
  hipStream_t s = (hipStream_t)stream;
#define PANGU_LAUNCH_ATTN(SH, CP)                                                                                       \
  hipLaunchKernelGGL((window_attn_f32_split_kernel<SH, CP>), dim3(grid), dim3(NT), 0, s, qkv, qkv_bias, esb, out, g, C, heads, \
                     n_pairs)
  if (shifted) {
    if (compact) PANGU_LAUNCH_ATTN(true, true); else PANGU_LAUNCH_ATTN(true, false);
  } else {
    if (compact) PANGU_LAUNCH_ATTN(false, true); else PANGU_LAUNCH_ATTN(false, false);
  }
#undef PANGU_LAUNCH_ATTN
  return pangu_launch_status();
}

extern "C" int pangu_window_attn_fwd_split(pangu_stream_t stream, const float* qkv, const float* qkv_bias, const float* esb,
                                           float* out, int Z, int H, int W, int C, int heads, int shifted) {
  return launch_attn_split(stream, qkv, qkv_bias, esb, out, Z, H, W, C, heads, shifted, false);
}

extern "C" int pangu_window_attn_fwd_split_compact(pangu_stream_t stream, const float* qkv, const float* qkv_bias,
                                                   const float* esb_compact, float* out, int Z, int H, int W, int C, int heads,
                                                   int shifted) {
  return launch_attn_split(stream, qkv, qkv_bias, esb_compact, out, Z, H, W, C, heads, shifted, true);
}
