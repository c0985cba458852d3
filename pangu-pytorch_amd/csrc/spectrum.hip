// Zonal power spectra of forecast fields (fp32) for gfx950: power per zonal wavenumber along each latitude circle, averaged over
// up to four latitude bands, as a folded real DFT on the f32-input MFMA.
//
// pangu_zonal_spectrum_f32 reads fields [N][planes][H][W] (item stride in elements, a multiple of 4), optionally minus
// [planes][H][W], band_weight [B][H] (1 <= B <= 4) and the two basis tables, and writes out [N][B][planes][K + 1] for the
// wavenumbers 0..K, 1 <= K <= W/2; W % 4 == 0, W >= 8.  Per row (n, plane, h), all in fp32:
//   d[j]  = fields[j] - minus[j] (one rounding) with minus, fields[j] without;
//   pivot = d[0],  a[j] = d[j] - pivot.  Subtracting a constant changes only wavenumber 0, and it takes the large offset of
//           fields such as geopotential or temperature out of every accumulation (an offset of 5e4 on an anomaly of 1e3 costs two
//           digits at every wavenumber otherwise) without a pass over the row, which the row mean would need;
//   X_k   = sum_j a[j] exp(-2 pi i jk / W);
//   P_0   = (pivot + Re X_0 * (1 / W))^2;
//   P_k   = (Re X_k^2 + Im X_k^2) * (c_k / W^2) for 1 <= k <= K,  c_k = 2 except c_{W/2} = 1 (1 / W, 2 / W^2 and 1 / W^2 are
//           rounded to fp32 once, on the host).  With K = W/2, sum_k P_k is the row's mean square (Parseval).
// Per band:  out[n][b][plane][k] = sum_h band_weight[b][h] * P_k(n, plane, h).  A row whose weight in band b is exactly 0 adds
// nothing to band b whatever it holds.
// Non-finite values are NOT detected: a NaN in a row makes every wavenumber of that (item, plane) NaN in the bands that give the
// row a non-zero weight (an infinity: NaN or infinite); the other bands, planes and items are not touched by it.
//
// Transform: with M = W/2, e[j] = a[j] + a[W - j] and o[j] = a[j] - a[W - j] for 0 < j < M, e[0] = a[0], e[M] = a[M], o[0] =
// o[M] = 0,
//   Re X_k = sum_{j <= M} e[j] cos(2 pi jk / W),   Im X_k = -sum_{0 < j < M} o[j] sin(2 pi jk / W),
// which halves the reduction length of the plain DFT.  basis_cos / basis_sin [M + 1][K + 1] hold cos / sin(2 pi ((j k) mod W) / W),
// computed in float64 and rounded once (score.spectrum_basis).  The sign of Im X_k does not enter the power.
//
// Implementation: a workgroup (256 threads, 4 waves) owns a tile of SP_ROWS = 128 rows of one (item, plane) by SP_COLS = 128
// wavenumbers; each wave owns 64 x 64 of it as 2 x 2 tiles of v_mfma_f32_32x32x2_f32, one accumulator for Re and one for Im
// (128 accumulator registers).  The reduction index j is walked in chunks of SP_JC = 16: the chunk's rows are read forwards
// (x[j]) and backwards (x[W - j]) with 16-byte loads (four lanes cover the 64 contiguous bytes of a row, a wave 16 rows per
// load), folded and written transposed ([j][row]) to LDS together with the chunk of the two basis tables ([j][k]); e and o never
// go to memory.  The loads of chunk c + 1 are spread over the 8 product steps of chunk c (load_part), branch-free.  Both operand
// fragments are reads of 32 consecutive floats per half-wave: conflict-free without a swizzle.  Sub-tiles that lie wholly
// beyond H or K are skipped (wave-uniform), rows at or beyond H are staged as zeros and get weight 0.  Workgroup ids are mapped to
// tiles so that an XCD works on neighbouring tiles (the wavenumber tiles of a row tile share its rows in that XCD's L2).
// Epilogue: square, scale, multiply by the B band weights of the row and add over the tile's rows in a fixed order (the 32 rows a
// lane holds, the two half-waves, the two waves); the tile's partial sums go to the workspace [N][planes][row tiles][B][K + 1]
// and a second launch adds the row tiles in tile order in double.  No atomics: every output is bit-identical from run to run,
// and the chain of column k is the same for every K, every N and every stride.
#include "common.h"

#include <type_traits>

namespace {

constexpr int SP_THREADS = 256;
constexpr int SP_ROWS = 128;       // rows of a workgroup tile
constexpr int SP_COLS = 128;       // wavenumbers of a workgroup tile
constexpr int SP_JC = 16;          // folded samples staged per step
constexpr int SP_LDA = SP_ROWS + 2;  // row stride of the [j][row] images: the staging writes of a half-wave (8 rows x 4 sample
                                     // quads, element i of each) fall on banks 8 q + 2 i + r, all different
constexpr int SP_MAX_B = 4;
constexpr int SP_XCDS = 8;         // consecutive workgroups go to different XCDs (private L2s): see the swizzle below

struct SpectrumScale {             // by value in the kernel arguments
  float inv_w, c2, c1;             // 1 / W, 2 / W^2, 1 / W^2
};

// The raw samples of one row a thread stages per chunk, as loaded: x[jq .. jq + 3], x[W - jq - 4 .. W - jq - 1] and x[W - jq] of
// fields (f0, b0, bs) and of minus (g0, h0, hs).
struct RowQuad {
  f32x4 f0, b0, g0, h0;
  float bs, hs;
};

// One row quad of fields or of minus: one aligned 16-byte load forwards, one backwards ([W - jq - 4, W - jq - 1]) and the single
// x[W - jq] (x[0] at jq == 0, where the fold does not use it).  No branch: loads behind divergent branches wait for each other.
// Every address lies inside the row for jq <= M (jq + 3 <= M + 3 < W and W - jq - 4 >= M - 4 >= 0, as W >= 8); a quad wholly
// beyond M reads quad 0 instead, and a row at or beyond H row 0 of the plane (xr points there).  What is read beyond M or H is
// discarded by the caller, which stages zeros for it.
__device__ __forceinline__ void load_row_quad(f32x4& fwd, f32x4& bwd, float& single, const float* __restrict__ xr, int jq, int M,
                                              int W) {
  jq = jq <= M ? jq : 0;
  fwd = *reinterpret_cast<const f32x4*>(xr + jq);
  bwd = *reinterpret_cast<const f32x4*>(xr + (W - jq - 4));
  single = xr[jq == 0 ? 0 : W - jq];
}

// d[jq + i] and d[W - jq - i], i = 0..3, of a loaded quad (the subtraction waits for the loads: done when the quad is staged)
template <bool MINUS>
__device__ __forceinline__ void quad_values(const RowQuad& c, float (&f)[4], float (&b)[4]) {
  // Element 0 of the backward loads is not needed.  Keep its register until here all the same: handed out earlier, while the
  // load is in flight, its next writer waits for the load (and every load before it) in the middle of the product steps.
  asm volatile("" ::"v"(c.b0[0]));
  if (MINUS) asm volatile("" ::"v"(c.h0[0]));
  f[0] = c.f0[0]; f[1] = c.f0[1]; f[2] = c.f0[2]; f[3] = c.f0[3];
  b[0] = c.bs; b[1] = c.b0[3]; b[2] = c.b0[2]; b[3] = c.b0[1];
  if (MINUS) {
    f[0] -= c.g0[0]; f[1] -= c.g0[1]; f[2] -= c.g0[2]; f[3] -= c.g0[3];
    b[0] -= c.hs; b[1] -= c.h0[3]; b[2] -= c.h0[2]; b[3] -= c.h0[1];
  }
}

template <bool MINUS>
__global__ __launch_bounds__(SP_THREADS, 2) void zonal_spectrum_kernel(const float* __restrict__ fields, long long stride,
                                                                       const float* __restrict__ minus,
                                                                       const float* __restrict__ band_w, int B,
                                                                       const float* __restrict__ basis_cos,
                                                                       const float* __restrict__ basis_sin, int K,
                                                                       float* __restrict__ ws, int planes, int H, int W, int row_tiles,
                                                                       int col_tiles, long long total, long long per_xcd,
                                                                       const SpectrumScale sc) {
  __shared__ float e_s[SP_JC][SP_LDA], o_s[SP_JC][SP_LDA];        // [j][row]: the A operand images
  __shared__ float cos_s[SP_JC][SP_COLS], sin_s[SP_JC][SP_COLS];  // [j][k]: the B operand images
  __shared__ float wt_s[SP_MAX_B][SP_ROWS], pivot_s[SP_ROWS];

  // XCD-aware order: workgroup ids go round-robin over the 8 XCDs, so give each XCD a contiguous run of tiles.  The tiles of a run
  // share their rows (col tile is the fastest index) and read them from HBM once.
  const long long tile = (long long)(blockIdx.x % SP_XCDS) * per_xcd + blockIdx.x / SP_XCDS;
  if (tile >= total) return;
  const int ct = (int)(tile % col_tiles);
  long long rest = tile / col_tiles;
  const int rt = (int)(rest % row_tiles);
  rest /= row_tiles;
  const int plane = (int)(rest % planes), n = (int)(rest / planes);
  const int row0 = rt * SP_ROWS, k0 = ct * SP_COLS, M = W >> 1, ldb = K + 1;

  const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
  // staging roles, rows: one quad of the chunk's 16 samples of rows ar and ar + 64 -- four lanes cover the 64 contiguous bytes
  // of a row's chunk, a wave 16 rows per load
  const int aq = t & 3, ar = t >> 2;
  const float* xr[2];
  const float* mr[2];
  bool row_ok[2];
  float pivot[2];
#pragma unroll
  for (int p = 0; p < 2; ++p) {
    const int grow = row0 + ar + 64 * p;
    row_ok[p] = grow < H;
    const long long roff = (long long)plane * H * W + (long long)(row_ok[p] ? grow : 0) * W;
    xr[p] = fields + (long long)n * stride + roff;
    mr[p] = MINUS ? minus + roff : nullptr;
    pivot[p] = 0.0f;
    if (row_ok[p]) pivot[p] = MINUS ? xr[p][0] - mr[p][0] : xr[p][0];
  }
  // staging roles, basis and row constants: a wavenumber (or a row) and one half of the chunk's 16 samples
  const int srow = t & (SP_ROWS - 1), shalf = t >> 7;
  if (shalf == 0) {
    const int grow = row0 + srow;
    float pv = 0.0f;
    if (grow < H) {
      const long long o = (long long)plane * H * W + (long long)grow * W;
      pv = MINUS ? fields[(long long)n * stride + o] - minus[o] : fields[(long long)n * stride + o];
    }
    pivot_s[srow] = pv;
#pragma unroll
    for (int b = 0; b < SP_MAX_B; ++b) wt_s[b][srow] = (b < B && grow < H) ? band_w[b * H + grow] : 0.0f;
  }
  const int sk = k0 + srow;      // this thread's wavenumber when it stages the basis
  const bool k_ok = sk <= K;

  // compute roles: wave (wr, wc) owns rows [64 wr, 64 wr + 64) x wavenumbers [64 wc, 64 wc + 64) of the tile
  const int wr = wave >> 1, wc = wave & 1, l31 = lane & 31, lh = lane >> 5;
  bool sub_ok[2][2];
#pragma unroll
  for (int rs = 0; rs < 2; ++rs)
#pragma unroll
    for (int cs = 0; cs < 2; ++cs)
      sub_ok[rs][cs] = (row0 + wr * 64 + rs * 32 < H) && (k0 + wc * 64 + cs * 32 <= K);

  f32x16 re[2][2], im[2][2];
#pragma unroll
  for (int rs = 0; rs < 2; ++rs)
#pragma unroll
    for (int cs = 0; cs < 2; ++cs)
#pragma unroll
      for (int r = 0; r < 16; ++r) re[rs][cs][r] = im[rs][cs][r] = 0.0f;

  RowQuad rc[2];
  float bc[8], bs[8];
  // The loads of a chunk in 8 parts, one per product step of the chunk before: a wave that issued them all at once would wait
  // for the memory pipeline to take them before its first MFMA, and the two workgroups of a CU run in step with each other.
  // Part s: basis row s of this thread's half (entries beyond M or K: a clamped entry is read and a zero is staged), parts 0
  // and 1 the two rows of fields, parts 2 and 3 those of minus.
  const int skc = min(sk, K);
  auto load_part = [&](int s, int j0) {
    const int at = min(j0 + shalf * 8 + s, M) * ldb + skc;
    bc[s] = basis_cos[at];
    bs[s] = basis_sin[at];
    if (s < 2) load_row_quad(rc[s].f0, rc[s].b0, rc[s].bs, xr[s], j0 + aq * 4, M, W);
    if (MINUS && s >= 2 && s < 4) load_row_quad(rc[s - 2].g0, rc[s - 2].h0, rc[s - 2].hs, mr[s - 2], j0 + aq * 4, M, W);
  };

  // one step: two samples (one per half-wave) into the wave's 2 x 2 tiles; `full`: no sub-tile of this wave is skipped
  auto products = [&](auto full, int s) {
    const int ja = 2 * s + lh;
    float ae[2], ao[2], cb[2], sb[2];
#pragma unroll
    for (int q = 0; q < 2; ++q) {
      ae[q] = e_s[ja][wr * 64 + q * 32 + l31];
      ao[q] = o_s[ja][wr * 64 + q * 32 + l31];
      cb[q] = cos_s[ja][wc * 64 + q * 32 + l31];
      sb[q] = sin_s[ja][wc * 64 + q * 32 + l31];
    }
#pragma unroll
    for (int rs = 0; rs < 2; ++rs)
#pragma unroll
      for (int cs = 0; cs < 2; ++cs)
        if (decltype(full)::value || sub_ok[rs][cs]) {
          re[rs][cs] = __builtin_amdgcn_mfma_f32_32x32x2f32(ae[rs], cb[cs], re[rs][cs], 0, 0, 0);
          im[rs][cs] = __builtin_amdgcn_mfma_f32_32x32x2f32(ao[rs], sb[cs], im[rs][cs], 0, 0, 0);
        }
  };
  const bool all_ok = sub_ok[1][1];      // the last sub-tile in both directions: the others lie before it

  const int chunks = (M + SP_JC) / SP_JC;      // ceil((M + 1) / SP_JC)
#pragma unroll
  for (int s = 0; s < SP_JC / 2; ++s) load_part(s, 0);
  for (int c = 0; c < chunks; ++c) {
    const int j0 = c * SP_JC;
    __syncthreads();      // the products of the chunk before have read the images
#pragma unroll
    for (int p = 0; p < 2; ++p) {
      float df[4], db[4];
      quad_values<MINUS>(rc[p], df, db);
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        const int jj = aq * 4 + i, j = j0 + jj;
        const float af = df[i] - pivot[p], ab = db[i] - pivot[p];
        float e = af + ab, o = af - ab;
        e = (j == 0 || j == M) ? af : e;
        o = (j == 0 || j == M) ? 0.0f : o;
        const bool none = j > M || !row_ok[p];
        e_s[jj][ar + 64 * p] = none ? 0.0f : e;
        o_s[jj][ar + 64 * p] = none ? 0.0f : o;
      }
    }
#pragma unroll
    for (int i = 0; i < 8; ++i) {
      const bool ok = k_ok && j0 + shalf * 8 + i <= M;
      cos_s[shalf * 8 + i][srow] = ok ? bc[i] : 0.0f;
      sin_s[shalf * 8 + i][srow] = ok ? bs[i] : 0.0f;
    }
    __syncthreads();
    // (the loads beyond the last chunk go to the clamped addresses and nothing of them is used)
    const int steps = min(SP_JC / 2, (M - j0) / 2 + 1);      // samples beyond M are zeros: skip their steps
    if (all_ok && steps == SP_JC / 2) {
#pragma unroll
      for (int s = 0; s < SP_JC / 2; ++s) {
        products(std::true_type{}, s);
        load_part(s, j0 + SP_JC);
        __builtin_amdgcn_sched_barrier(0);      // keep the loads between the steps: hoisted, they are one burst again
      }
    } else {
#pragma unroll
      for (int s = 0; s < SP_JC / 2; ++s) load_part(s, j0 + SP_JC);
      for (int s = 0; s < steps; ++s) products(std::false_type{}, s);
    }
  }

  // epilogue: lane (l31, lh) holds column l31 of each 32 x 32 tile, rows (r & 3) + 8 (r >> 2) + 4 lh in register r
  float sum[SP_MAX_B][2];
#pragma unroll
  for (int b = 0; b < SP_MAX_B; ++b) sum[b][0] = sum[b][1] = 0.0f;
#pragma unroll
  for (int cs = 0; cs < 2; ++cs) {
    const int k = k0 + wc * 64 + cs * 32 + l31;
    const float ck = k == M ? sc.c1 : sc.c2;
#pragma unroll
    for (int rs = 0; rs < 2; ++rs) {
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const int row = wr * 64 + rs * 32 + (r & 3) + 8 * (r >> 2) + 4 * lh;
        const float xr_ = re[rs][cs][r], xi_ = im[rs][cs][r];
        float p = (xr_ * xr_ + xi_ * xi_) * ck;
        if (k == 0) {
          const float m0 = pivot_s[row] + xr_ * sc.inv_w;
          p = m0 * m0;
        }
#pragma unroll
        for (int b = 0; b < SP_MAX_B; ++b) {
          const float w = wt_s[b][row];
          sum[b][cs] += w != 0.0f ? w * p : 0.0f;      // weight 0: the row does not enter the band, NaN or not
        }
      }
    }
  }
  __syncthreads();      // every wave is done with the operand images: reuse e_s for the two row halves
  float(*red)[SP_MAX_B][SP_COLS] = reinterpret_cast<float(*)[SP_MAX_B][SP_COLS]>(&e_s[0][0]);      // [2][4][128] = 4 KB of 8
#pragma unroll
  for (int b = 0; b < SP_MAX_B; ++b)
#pragma unroll
    for (int cs = 0; cs < 2; ++cs) {
      const float v = sum[b][cs] + __shfl_xor(sum[b][cs], 32, 64);
      if (lh == 0) red[wr][b][wc * 64 + cs * 32 + l31] = v;
    }
  __syncthreads();
  if (t < SP_COLS && k_ok) {
    float* dst = ws + (((long long)n * planes + plane) * row_tiles + rt) * B * ldb + sk;
    for (int b = 0; b < B; ++b) dst[(long long)b * ldb] = red[0][b][t] + red[1][b][t];
  }
}

// out[n][b][plane][k]: the row tiles' partial sums added in tile order in double
__global__ __launch_bounds__(SP_THREADS) void zonal_spectrum_final_kernel(const float* __restrict__ ws, float* __restrict__ out,
                                                                          int B, int planes, int row_tiles, int ldb,
                                                                          long long total) {
  const long long i = (long long)blockIdx.x * SP_THREADS + threadIdx.x;
  if (i >= total) return;
  const int k = (int)(i % ldb);
  long long rest = i / ldb;
  const int plane = (int)(rest % planes);
  rest /= planes;
  const int b = (int)(rest % B);
  const long long n = rest / B;
  const float* p = ws + (((n * planes + plane) * row_tiles) * B + b) * ldb + k;
  double s = 0.0;
  for (int rt = 0; rt < row_tiles; ++rt) s += (double)p[(long long)rt * B * ldb];
  out[i] = (float)s;
}

}  // namespace

extern "C" long long pangu_zonal_spectrum_ws_bytes(int N, int planes, int H, int B, int K) {
  if (N < 1 || planes <= 0 || H <= 0 || B < 1 || B > SP_MAX_B || K < 1 || K >= (1 << 14)) return PANGU_E_SHAPE;
  const long long row_tiles = (H + SP_ROWS - 1) / SP_ROWS;
  const long long per_item = (long long)planes * row_tiles * B * (K + 1);      // < 2^31 * 2^24 * 4 * 2^14: no overflow
  if (per_item > (1ll << 40) / N) return PANGU_E_SHAPE;
  return per_item * N * 4;
}

extern "C" int pangu_zonal_spectrum_f32(pangu_stream_t stream, const float* fields, long long item_stride, int N,
                                        const float* minus, const float* band_weight, int B, const float* basis_cos,
                                        const float* basis_sin, int K, float* out, void* workspace, long long workspace_bytes,
                                        int planes, int H, int W) {
  if (!fields || !band_weight || !basis_cos || !basis_sin || !out || !workspace) return PANGU_E_NULL;
  if (N < 1 || B < 1 || B > SP_MAX_B || planes <= 0 || H <= 0 || W < 8 || (W & 3) || W >= (1 << 15)) return PANGU_E_SHAPE;
  if (K < 1 || K > W / 2) return PANGU_E_SHAPE;
  const long long HW = (long long)H * W;
  if (HW > 0x7FFFFFFFll) return PANGU_E_SHAPE;
  if (planes > (1ll << 40) / HW) return PANGU_E_SHAPE;
  const long long HWp = HW * planes;
  if (item_stride < HWp || (item_stride & 3) || item_stride > (1ll << 40)) return PANGU_E_SHAPE;
  if (N > 1 && item_stride > ((1ll << 40) - HWp) / (N - 1)) return PANGU_E_SHAPE;      // (N - 1) * stride + planes*H*W > 2^40
  const long long need = pangu_zonal_spectrum_ws_bytes(N, planes, H, B, K);
  if (need < 0) return PANGU_E_SHAPE;
  const int row_tiles = (H + SP_ROWS - 1) / SP_ROWS, col_tiles = (K + SP_COLS) / SP_COLS;      // ceil((K + 1) / SP_COLS)
  const long long total = (long long)N * planes * row_tiles * col_tiles;
  const long long per_xcd = (total + SP_XCDS - 1) / SP_XCDS;
  const long long outs = (long long)N * B * planes * (K + 1);
  if (per_xcd * SP_XCDS > 0x7FFFFFFFll || (outs + SP_THREADS - 1) / SP_THREADS > 0x7FFFFFFFll) return PANGU_E_SHAPE;
  if (workspace_bytes < need) return PANGU_E_ARG;
  const size_t misaligned = reinterpret_cast<size_t>(fields) | reinterpret_cast<size_t>(minus) | reinterpret_cast<size_t>(out) |
                            reinterpret_cast<size_t>(basis_cos) | reinterpret_cast<size_t>(basis_sin);
  if ((misaligned & 15) || (reinterpret_cast<size_t>(workspace) & 3)) return PANGU_E_ARG;

  SpectrumScale sc;
  sc.inv_w = (float)(1.0 / (double)W);
  sc.c2 = (float)(2.0 / ((double)W * (double)W));
  sc.c1 = (float)(1.0 / ((double)W * (double)W));
  hipStream_t s = (hipStream_t)stream;
  float* ws = static_cast<float*>(workspace);
  const dim3 grid((unsigned)(per_xcd * SP_XCDS)), block(SP_THREADS);
  if (minus)
    hipLaunchKernelGGL((zonal_spectrum_kernel<true>), grid, block, 0, s, fields, item_stride, minus, band_weight, B, basis_cos,
                       basis_sin, K, ws, planes, H, W, row_tiles, col_tiles, total, per_xcd, sc);
  else
    hipLaunchKernelGGL((zonal_spectrum_kernel<false>), grid, block, 0, s, fields, item_stride, minus, band_weight, B, basis_cos,
                       basis_sin, K, ws, planes, H, W, row_tiles, col_tiles, total, per_xcd, sc);
  const int rc = pangu_launch_status();
  if (rc != PANGU_OK) return rc;
  hipLaunchKernelGGL(zonal_spectrum_final_kernel, dim3((unsigned)((outs + SP_THREADS - 1) / SP_THREADS)), block, 0, s, ws, out, B,
                     planes, row_tiles, K + 1, outs);
  return pangu_launch_status();
}
