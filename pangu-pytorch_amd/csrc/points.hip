// The observation operator for gfx950: bilinear interpolation of (variable, level) planes to N arbitrary points, and the departure
// statistics of a forecast against observations at those points (SYNOP stations, buoys, radiosonde levels, masts).
//
// The points come as a plan (score.point_plan): per point the grid node north-west of it, row in 0..H-1 and col in 0..W-1, and the
// fp32 weights wy, wx in [0, 1) of the next row and the next column; columns wrap (c1 = (col + 1) mod W), rows do not (r1 =
// min(row + 1, H - 1); the plan gives wy = 0 on the last row).  With v = src * mul[q] + add[q] in two roundings (pk_value; q the
// source plane, level-reversed with `levels`, pk_src_plane), every operation rounded once to fp32, no contraction:
//   line(j) = wx == 0 ? v[j][col] : fl(fl(v[j][col] * fl(1 - wx)) + fl(v[j][c1] * wx))
//   f       = wy == 0 ? line(row) : fl(fl(line(row) * fl(1 - wy)) + fl(line(r1) * wy))
// A tap of weight zero is a select, never a product: a NaN or an infinity at a node reaches exactly the points whose stencil
// holds that node with a non-zero weight, and a point on a node returns the node's value bit for bit.  Non-finite values are not
// masked otherwise.
//
// pangu_sample_points_f32 writes f to out [planes][N].  pangu_point_scores_f32 compares f with obs [planes][N]: with c = clim[p] (0
// without clim), d = f - o, a = f - c, b = o - c (one fp32 rounding each) and the fp32 products |d|, d d, a b, a a, b b, over the
// points of a region whose observation is not NaN (NaN marks a missing report; infinities are values), per (plane, region):
//   sums[0] = n   sums[1] = sum d   sums[2] = sum |d|   sums[3] = sum d^2   sums[4] = sum a   sums[5] = sum b   sums[6] = sum a b
//   sums[7] = sum a^2   sums[8] = sum b^2   sums[9] = n
// the layout of pangu_scorecard_sums_f32 with weight 1, so that sums[k] / sums[0] are the means.  departures (optional) receives d,
// NaN where the observation is missing.  Membership and validity are selects: a non-finite forecast value reaches the sums of
// exactly the regions that hold its point with a report; a region without a valid point gives ten zeros.
//
// Implementation.  One workgroup per (plane, chunk of PT_CHUNK points), lanes over points, PT_PER_LANE points per lane, plane-major
// (all chunks of a plane are neighbours in the grid).  A lane reads its points' plan entries (coalesced), issues the four 4-B tap
// loads of all its points -- always all four, in bounds by construction, so that no load waits behind a branch -- and only then
// uses the first; zero weights are applied as selects afterwards.  out, obs and departures are coalesced.  The alternative, lanes
// over planes for one point, would put every lane of a load in a different plane (64 cache lines 4 H W bytes apart per
// wave-instruction, none shared), stride the stores by N and serve no launch of fewer than 64 planes; with lanes over points the
// two column taps of a point share a cache line, neighbouring stations share lines, and a plane's 4 H W bytes stay in the L2s
// while its chunks run.
//   Scores: a lane adds its points' terms per region by selects (fp32), the wave adds its lanes (wave_sum: a fixed DPP / shuffle
// order), one thread per (region, sum) adds the waves in wave order and writes the chunk's partial to the workspace
// [plane][chunk][R][10] (32-bit words: fp32 sums, the counts as integers).  A second launch adds the chunks in chunk order in double.
// No atomics, every order is fixed: outputs are bit-identical from run to run and a plane's outputs do not depend on the other
// planes of the launch.
//
// Rounding of the sums.  The terms are exact fp32 values of the pinned arithmetic.  A term then passes through at most
// (PT_PER_LANE - 1) + 6 + (PT_WAVES - 1) = 12 rounded fp32 additions (in the lane: the first addition, to zero, is exact; six
// levels in the wave; the waves), each of a partial sum no larger than the chunk's sum of |terms|, and one double addition per
// chunk.  So |sums[k] - exact| <= gamma(12, 2^-24) S + gamma(chunks, 2^-53) S with S = sum |terms| and gamma(n, u) = n u / (1 - n u).
#include "common.h"
#include "plane_value.h"

namespace {

constexpr int PT_THREADS = 256;
constexpr int PT_PER_LANE = 4;                       // points a lane has in flight: 16 tap loads
constexpr int PT_CHUNK = PT_THREADS * PT_PER_LANE;   // the points of one workgroup, and of one workspace partial
constexpr int PT_SUMS = 10;
constexpr int PT_MAX_R = 8;
constexpr int PT_WAVES = PT_THREADS / 64;
constexpr int PT_FINAL_BATCH = 32;                   // chunk partials a thread of the second launch has in flight

struct PointPlan {
  const int* row;
  const int* col;
  const float* wy;
  const float* wx;
};

struct PointTaps {
  int o00, o01, o10, o11;      // offsets inside a plane: (row, col), (row, c1), (r1, col), (r1, c1)
  float wy, wx;
};

// The plan entry of point i.  The plan is trusted; an index outside the grid is still clamped into it, so that a broken plan gives
// wrong numbers and never an access outside the plane.
__device__ __forceinline__ PointTaps pt_taps(const PointPlan& pl, unsigned i, int H, int W) {
  PointTaps t;
  const int row = min(max(pl.row[i], 0), H - 1), col = min(max(pl.col[i], 0), W - 1);
  const int r1 = min(row + 1, H - 1), c1 = col + 1 == W ? 0 : col + 1;
  t.o00 = row * W + col;       // < H * W < 2^31
  t.o01 = row * W + c1;
  t.o10 = r1 * W + col;
  t.o11 = r1 * W + c1;
  t.wy = pl.wy[i];
  t.wx = pl.wx[i];
  return t;
}

// The pinned sampling arithmetic (the head comment) of the four raw taps
template <bool AFFINE>
__device__ __forceinline__ float pt_lerp(float x00, float x01, float x10, float x11, float wy, float wx, float m, float a) {
#pragma clang fp contract(off)
  const float v00 = pk_value<AFFINE>(x00, m, a), v01 = pk_value<AFFINE>(x01, m, a);
  const float v10 = pk_value<AFFINE>(x10, m, a), v11 = pk_value<AFFINE>(x11, m, a);
  const float ux = 1.0f - wx, uy = 1.0f - wy;
  const float p0 = v00 * ux, q0 = v01 * wx, p1 = v10 * ux, q1 = v11 * wx;
  const float l0 = wx == 0.0f ? v00 : p0 + q0;
  const float l1 = wx == 0.0f ? v10 : p1 + q1;
  const float pa = l0 * uy, pb = l1 * wy;
  return wy == 0.0f ? l0 : pa + pb;
}

// x[0..7]: the terms of sums[1..8] of one point, each product rounded on its own
__device__ __forceinline__ void pt_terms(float f, float o, float c, float (&x)[8]) {
#pragma clang fp contract(off)
  const float d = f - o, a = f - c, b = o - c;
  x[0] = d; x[1] = fabsf(d); x[2] = d * d;
  x[3] = a; x[4] = b; x[5] = a * b; x[6] = a * a; x[7] = b * b;
}

template <bool AFFINE>
__global__ __launch_bounds__(PT_THREADS) void sample_points_kernel(const float* __restrict__ src, const float* __restrict__ mul,
                                                                   const float* __restrict__ add, PointPlan pl,
                                                                   float* __restrict__ out, int H, int W, int N, int chunks,
                                                                   int levels) {
  const int p = blockIdx.x / chunks, ch = blockIdx.x - p * chunks;
  const int q = pk_src_plane(p, levels);
  const float* sp = src + (size_t)q * H * W;
  const float m = AFFINE ? mul[q] : 1.0f, a = AFFINE ? add[q] : 0.0f;
  const unsigned first = (unsigned)ch * PT_CHUNK + threadIdx.x, last = (unsigned)N - 1u;
  PointTaps t[PT_PER_LANE];
  float x[PT_PER_LANE][4];
#pragma unroll
  for (int j = 0; j < PT_PER_LANE; ++j) t[j] = pt_taps(pl, min(first + j * PT_THREADS, last), H, W);   // lanes past N: point N - 1
#pragma unroll
  for (int j = 0; j < PT_PER_LANE; ++j) {
    x[j][0] = sp[t[j].o00];
    x[j][1] = sp[t[j].o01];
    x[j][2] = sp[t[j].o10];
    x[j][3] = sp[t[j].o11];
  }
  float* op = out + (size_t)p * N;
#pragma unroll
  for (int j = 0; j < PT_PER_LANE; ++j) {
    const unsigned i = first + j * PT_THREADS;
    const float f = pt_lerp<AFFINE>(x[j][0], x[j][1], x[j][2], x[j][3], t[j].wy, t[j].wx, m, a);
    if (i <= last) op[i] = f;
  }
}

// RMAX: region accumulators kept (1, 4 or 8 >= R); MASK: region_bits given
template <int RMAX, bool AFFINE, bool MASK>
__global__ __launch_bounds__(PT_THREADS) void point_scores_kernel(const float* __restrict__ src, const float* __restrict__ mul,
                                                                  const float* __restrict__ add, PointPlan pl,
                                                                  const float* __restrict__ obs, const float* __restrict__ clim,
                                                                  const unsigned char* __restrict__ bits, int R,
                                                                  float* __restrict__ departures, uint32_t* __restrict__ ws, int H,
                                                                  int W, int N, int chunks, int levels) {
  __shared__ uint32_t pt_part[PT_WAVES][RMAX * 9];      // per wave and region: eight fp32 sums and the count
  const int p = blockIdx.x / chunks, ch = blockIdx.x - p * chunks;
  const int q = pk_src_plane(p, levels);
  const float* sp = src + (size_t)q * H * W;
  const float m = AFFINE ? mul[q] : 1.0f, a = AFFINE ? add[q] : 0.0f;
  const float c = clim ? clim[p] : 0.0f;
  const unsigned first = (unsigned)ch * PT_CHUNK + threadIdx.x, last = (unsigned)N - 1u;
  const float* ob = obs + (size_t)p * N;
  const uint32_t keep = MASK ? (1u << R) - 1u : 1u;      // bits of regions >= R are ignored
  PointTaps t[PT_PER_LANE];
  float x[PT_PER_LANE][4], o[PT_PER_LANE];
  uint32_t member[PT_PER_LANE];
#pragma unroll
  for (int j = 0; j < PT_PER_LANE; ++j) {
    const unsigned i = min(first + j * PT_THREADS, last);
    t[j] = pt_taps(pl, i, H, W);
    o[j] = ob[i];
    member[j] = MASK ? (bits[i] & keep) : 1u;
  }
#pragma unroll
  for (int j = 0; j < PT_PER_LANE; ++j) {
    x[j][0] = sp[t[j].o00];
    x[j][1] = sp[t[j].o01];
    x[j][2] = sp[t[j].o10];
    x[j][3] = sp[t[j].o11];
  }
  float s[RMAX][8];
  uint32_t n[RMAX];
#pragma unroll
  for (int r = 0; r < RMAX; ++r) {
#pragma unroll
    for (int k = 0; k < 8; ++k) s[r][k] = 0.0f;
    n[r] = 0u;
  }
#pragma unroll
  for (int j = 0; j < PT_PER_LANE; ++j) {
    const unsigned i = first + j * PT_THREADS;
    const float f = pt_lerp<AFFINE>(x[j][0], x[j][1], x[j][2], x[j][3], t[j].wy, t[j].wx, m, a);
    float e[8];
    pt_terms(f, o[j], c, e);
    if (departures && i <= last) departures[(size_t)p * N + i] = e[0];
    const bool valid = i <= last && o[j] == o[j];
#pragma unroll
    for (int r = 0; r < RMAX; ++r) {
      const bool in = valid && ((member[j] >> r) & 1u);
#pragma unroll
      for (int k = 0; k < 8; ++k) s[r][k] += in ? e[k] : 0.0f;
      n[r] += in ? 1u : 0u;
    }
  }
  // the lanes of a wave in wave_sum's fixed order, then the waves in wave order
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
  for (int r = 0; r < RMAX; ++r) {
#pragma unroll
    for (int k = 0; k < 8; ++k) {
      const float v = wave_sum(s[r][k]);
      if (lane == 0) pt_part[wave][r * 9 + k] = __float_as_uint(v);
    }
    uint32_t cnt = n[r];
#pragma unroll
    for (int sh = 1; sh < 64; sh <<= 1) cnt += (uint32_t)__shfl_xor((int)cnt, sh, 64);
    if (lane == 0) pt_part[wave][r * 9 + 8] = cnt;
  }
  __syncthreads();
  for (int i = threadIdx.x; i < R * PT_SUMS; i += PT_THREADS) {
    const int r = i / PT_SUMS, k = i - r * PT_SUMS;
    uint32_t out;
    if (k == 0 || k == 9) {
      out = 0u;
      for (int wv = 0; wv < PT_WAVES; ++wv) out += pt_part[wv][r * 9 + 8];
    } else {
      float v = __uint_as_float(pt_part[0][r * 9 + k - 1]);
      for (int wv = 1; wv < PT_WAVES; ++wv) v += __uint_as_float(pt_part[wv][r * 9 + k - 1]);
      out = __float_as_uint(v);
    }
    ws[(size_t)blockIdx.x * R * PT_SUMS + i] = out;
  }
}

// sums [plane][region][10] from the chunk partials, added in chunk order: the fp32 sums in double, the counts as integers.  A
// thread requests PT_FINAL_BATCH chunks' words before it adds the first (a million points are 977 chunks: one load per round
// trip would cost more than the pass over the points)
__global__ __launch_bounds__(256) void point_scores_final_kernel(const uint32_t* __restrict__ ws, double* __restrict__ sums, int planes,
                                                                 int chunks, int per_plane) {
  const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
  if (i >= (long long)planes * per_plane) return;
  const long long plane = i / per_plane, j = i - plane * per_plane;
  const uint32_t* src = ws + plane * chunks * per_plane + j;
  const int k = (int)(j % PT_SUMS);
  const bool count = k == 0 || k == 9;
  unsigned long long n = 0ull;
  double s = 0.0;
  for (int c0 = 0; c0 < chunks; c0 += PT_FINAL_BATCH) {
    uint32_t v[PT_FINAL_BATCH];
#pragma unroll
    for (int u = 0; u < PT_FINAL_BATCH; ++u) v[u] = src[(long long)min(c0 + u, chunks - 1) * per_plane];
#pragma unroll
    for (int u = 0; u < PT_FINAL_BATCH; ++u) {
      if (c0 + u < chunks) {
        n += v[u];
        s += (double)__uint_as_float(v[u]);
      }
    }
  }
  sums[i] = count ? (double)n : s;
}

long long point_chunks(int N) { return ((long long)N + PT_CHUNK - 1) / PT_CHUNK; }

// what both entries ask of the field, the plan and the sizes
int point_check(const float* src, const float* mul, const float* add, const int* row, const int* col, const float* wy,
                const float* wx, int planes, int H, int W, int N, int levels) {
  if (!src || !row || !col || !wy || !wx) return PANGU_E_NULL;
  if ((mul == nullptr) != (add == nullptr)) return PANGU_E_NULL;
  if (planes <= 0 || H < 2 || W <= 0 || N <= 0) return PANGU_E_SHAPE;
  if ((long long)H * W > 0x7fffffffll) return PANGU_E_SHAPE;                       // 32-bit indices within a plane
  if ((long long)planes * N > 0x7fffffffll) return PANGU_E_SHAPE;                  // and a one-dimensional grid of its chunks
  if (levels < 0 || (levels > 0 && planes % levels != 0)) return PANGU_E_SHAPE;
  return PANGU_OK;
}

bool misaligned4(const void* a, const void* b = nullptr, const void* c = nullptr, const void* d = nullptr) {
  return ((reinterpret_cast<size_t>(a) | reinterpret_cast<size_t>(b) | reinterpret_cast<size_t>(c) | reinterpret_cast<size_t>(d)) & 3) != 0;
}

template <int RMAX, bool MASK>
void launch_point_scores(hipStream_t s, int grid, const float* src, const float* mul, const float* add, const PointPlan& pl,
                         const float* obs, const float* clim, const unsigned char* bits, int R, float* departures, uint32_t* ws,
                         int H, int W, int N, int chunks, int levels) {
  if (mul)
    hipLaunchKernelGGL((point_scores_kernel<RMAX, true, MASK>), dim3(grid), dim3(PT_THREADS), 0, s, src, mul, add, pl, obs, clim, bits,
                       R, departures, ws, H, W, N, chunks, levels);
  else
    hipLaunchKernelGGL((point_scores_kernel<RMAX, false, MASK>), dim3(grid), dim3(PT_THREADS), 0, s, src, mul, add, pl, obs, clim, bits,
                       R, departures, ws, H, W, N, chunks, levels);
}

}  // namespace

extern "C" int pangu_sample_points_f32(pangu_stream_t stream, const float* src, const float* mul, const float* add, const int* row,
                                       const int* col, const float* wy, const float* wx, float* out, int planes, int H, int W, int N,
                                       int levels) {
  if (!out) return PANGU_E_NULL;
  const int rc = point_check(src, mul, add, row, col, wy, wx, planes, H, W, N, levels);
  if (rc != PANGU_OK) return rc;
  if (misaligned4(src, mul, add, out) || misaligned4(row, col, wy, wx)) return PANGU_E_ARG;
  const PointPlan pl{row, col, wy, wx};
  const int chunks = (int)point_chunks(N);
  const dim3 grid((unsigned)((long long)planes * chunks)), block(PT_THREADS);
  if (mul)
    hipLaunchKernelGGL(sample_points_kernel<true>, grid, block, 0, (hipStream_t)stream, src, mul, add, pl, out, H, W, N, chunks, levels);
  else
    hipLaunchKernelGGL(sample_points_kernel<false>, grid, block, 0, (hipStream_t)stream, src, mul, add, pl, out, H, W, N, chunks, levels);
  return pangu_launch_status();
}

extern "C" long long pangu_point_scores_ws_bytes(int planes, int N, int R) {
  if (planes <= 0 || N <= 0 || R < 1 || R > PT_MAX_R) return PANGU_E_SHAPE;
  if ((long long)planes * N > 0x7fffffffll) return PANGU_E_SHAPE;
  return (long long)planes * point_chunks(N) * R * PT_SUMS * 4;
}

extern "C" int pangu_point_scores_f32(pangu_stream_t stream, const float* src, const float* mul, const float* add, const int* row,
                                      const int* col, const float* wy, const float* wx, const float* obs, const float* clim,
                                      const unsigned char* region_bits, int R, float* departures, double* sums, void* workspace,
                                      long long workspace_bytes, int planes, int H, int W, int N, int levels) {
  if (!obs || !sums || !workspace) return PANGU_E_NULL;
  if (!region_bits && R != 1) return PANGU_E_NULL;
  const int rc = point_check(src, mul, add, row, col, wy, wx, planes, H, W, N, levels);
  if (rc != PANGU_OK) return rc;
  const long long need = pangu_point_scores_ws_bytes(planes, N, R);
  if (need < 0) return PANGU_E_SHAPE;
  if (workspace_bytes < need) return PANGU_E_ARG;
  if (misaligned4(src, mul, add, obs) || misaligned4(row, col, wy, wx) || misaligned4(clim, departures, workspace)) return PANGU_E_ARG;
  if (reinterpret_cast<size_t>(sums) & 7) return PANGU_E_ARG;
  hipStream_t s = (hipStream_t)stream;
  const PointPlan pl{row, col, wy, wx};
  const int chunks = (int)point_chunks(N), grid = (int)((long long)planes * chunks);
  uint32_t* ws = static_cast<uint32_t*>(workspace);
  if (!region_bits)
    launch_point_scores<1, false>(s, grid, src, mul, add, pl, obs, clim, region_bits, R, departures, ws, H, W, N, chunks, levels);
  else if (R == 1)
    launch_point_scores<1, true>(s, grid, src, mul, add, pl, obs, clim, region_bits, R, departures, ws, H, W, N, chunks, levels);
  else if (R <= 4)
    launch_point_scores<4, true>(s, grid, src, mul, add, pl, obs, clim, region_bits, R, departures, ws, H, W, N, chunks, levels);
  else
    launch_point_scores<8, true>(s, grid, src, mul, add, pl, obs, clim, region_bits, R, departures, ws, H, W, N, chunks, levels);
  const int launched = pangu_launch_status();
  if (launched != PANGU_OK) return launched;
  const int per_plane = R * PT_SUMS;
  const long long outs = (long long)planes * per_plane;
  hipLaunchKernelGGL(point_scores_final_kernel, dim3((unsigned)((outs + 255) / 256)), dim3(256), 0, s, ws, sums, planes, chunks,
                     per_plane);
  return pangu_launch_status();
}
