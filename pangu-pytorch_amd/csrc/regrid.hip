// First-order conservative remapping of (variable, level) planes from the native lat-lon grid to a coarser one of the same family
// (poles included, longitudes from 0): out = R_lat . v . R_lon^T per plane, with the banded weights of score.regrid_plan.  The
// de-normalisation v = x * mul + add and the level reversal are folded into the pass, as in pack.hip, so that a forecast goes from
// the model's output to a WeatherBench-style 1.5 degree field in one read of the fine field.
//
//   one workgroup per (output plane, output row J):
//   stage 1  the lat_count[J] input rows are combined vertically, lanes along longitude, 16 B per lane and row; a lane issues the
//            loads of its rows (up to 8 at a time) before the first is used (the tap count is a template argument, picked by a
//            workgroup-uniform switch), then acc = w_0 v_0, acc = fma(w_t, v_t, acc) for t = 1.. in that order -> one LDS row of
//            W_in floats
//   barrier
//   stage 2  a lane per output column I: out = w_0 r[s], out = fma(w_t, r[(s + t) mod W_in], out) over the lon_count[I] taps, plain
//            stores.
// No atomics, no workspace, one fixed order: bit-identical from run to run; a tap of weight 1 alone returns its input bit for bit.
// Non-finite values are not masked: they reach exactly the output cells whose stencil holds them.
//
// Data movement: each input row is read once per output row whose band holds it -- rows on a shared cell edge twice (7/6 of the
// field at ratio 6; the workgroups of adjacent J run on one XCD, so the second read of an edge row is served by its L2, not by
// HBM) -- and W_out floats are written per workgroup.  A lane requests the start, count and first 8 weights of its output column
// before stage 1, so that their latency passes under the row loads.  A plane whose rows are not all 16-B aligned (W_in % 4 != 0,
// or a plane base off 16 B) takes 4-B loads; the choice depends on the plane alone, so it is uniform over the workgroup.
#include "common.h"
#include "plane_value.h"

namespace {

constexpr int RG_THREADS = 256;
constexpr int RG_MAX_TAPS = 16;
constexpr int RG_CHUNK = 8;                    // rows (stage 1) / weights (stage 2) a lane has in flight
constexpr unsigned RG_XCDS = 8;
constexpr int RG_MAX_W = 16384;                // one LDS row of W_in floats: 64 KB

struct RegridTables {
  const int* lat_start;
  const int* lat_count;
  const float* lat_w;
  const int* lon_start;
  const int* lon_count;
  const float* lon_w;
  int lat_taps, lon_taps;
};

// One piece of stage 1: N <= RG_CHUNK rows starting at `rows` (row stride W floats) with the weights w[0..N); VEC lanes take 4
// columns, the others 1.  A lane issues its N loads before it uses the first.  FIRST: acc = w_0 v_0, then one fma per row;
// otherwise the piece continues the sum this lane left in the LDS row (bands of more than RG_CHUNK rows: the pieces bound the
// registers, and a lane only ever reads back what it wrote itself).
template <int N, bool VEC, bool AFFINE, bool FIRST>
__device__ __forceinline__ void rg_combine_rows(const float* __restrict__ rows, const float* __restrict__ w, int W, float m, float a,
                                                float* __restrict__ lds) {
  float wt[N];
#pragma unroll
  for (int t = 0; t < N; ++t) wt[t] = w[t];
  if (VEC) {
    const int groups = W >> 2;
#pragma unroll 1
    for (int g = threadIdx.x; g < groups; g += RG_THREADS) {
      f32x4 x[N];
#pragma unroll
      for (int t = 0; t < N; ++t) x[t] = *(const f32x4*)(rows + (size_t)t * W + 4 * g);
      f32x4 acc;
      if (!FIRST) acc = *(const f32x4*)(lds + 4 * g);
#pragma unroll
      for (int t = 0; t < N; ++t) {
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          const float v = pk_value<AFFINE>(x[t][j], m, a);
          acc[j] = (FIRST && t == 0) ? wt[0] * v : __builtin_fmaf(wt[t], v, acc[j]);
        }
      }
      *(f32x4*)(lds + 4 * g) = acc;
    }
  } else {
#pragma unroll 1
    for (int c = threadIdx.x; c < W; c += RG_THREADS) {
      float x[N];
#pragma unroll
      for (int t = 0; t < N; ++t) x[t] = rows[(size_t)t * W + c];
      float acc = FIRST ? 0.0f : lds[c];
#pragma unroll
      for (int t = 0; t < N; ++t) {
        const float v = pk_value<AFFINE>(x[t], m, a);
        acc = (FIRST && t == 0) ? wt[0] * v : __builtin_fmaf(wt[t], v, acc);
      }
      lds[c] = acc;
    }
  }
}

// One output column's longitude band: start, count and the first RG_CHUNK weights (the table rows are zero-padded to lon_taps, so
// every weight read is in bounds; the loads do not depend on one another and are in flight together).
struct LonTaps {
  int start, count;
  float w[RG_CHUNK];
};
__device__ __forceinline__ LonTaps rg_lon_taps(const RegridTables& tb, int I) {
  LonTaps r;
  r.start = tb.lon_start[I];
  r.count = tb.lon_count[I];
  const float* lw = tb.lon_w + (size_t)I * tb.lon_taps;
#pragma unroll
  for (int t = 0; t < RG_CHUNK; ++t) r.w[t] = lw[t < tb.lon_taps ? t : tb.lon_taps - 1];
  return r;
}

template <bool VEC, bool AFFINE, bool FIRST>
__device__ __forceinline__ void rg_piece(int n, const float* rows, const float* w, int W, float m, float a, float* lds) {
  switch (n) {                                  // (workgroup-uniform)
#define RG_CASE(N) case N: rg_combine_rows<N, VEC, AFFINE, FIRST>(rows, w, W, m, a, lds); break;
    RG_CASE(1) RG_CASE(2) RG_CASE(3) RG_CASE(4) RG_CASE(5) RG_CASE(6) RG_CASE(7) RG_CASE(8)
#undef RG_CASE
    default: break;
  }
}

// Stage 1 for a band of n rows, 1 <= n <= 16 (a count outside is outside the plan's contract and is clamped into it)
template <bool VEC, bool AFFINE>
__device__ __forceinline__ void rg_stage1(int n, const float* rows, const float* w, int W, float m, float a, float* lds) {
  n = n < 1 ? 1 : (n > RG_MAX_TAPS ? RG_MAX_TAPS : n);
  rg_piece<VEC, AFFINE, true>(n < RG_CHUNK ? n : RG_CHUNK, rows, w, W, m, a, lds);
  if (n > RG_CHUNK) rg_piece<VEC, AFFINE, false>(n - RG_CHUNK, rows + (size_t)RG_CHUNK * W, w + RG_CHUNK, W, m, a, lds);
}

template <bool AFFINE>
__global__ __launch_bounds__(RG_THREADS) void regrid_planes_kernel(const float* __restrict__ src, const float* __restrict__ mul,
                                                                   const float* __restrict__ add, float* __restrict__ dst,
                                                                   int H_in, int W_in, int H_out, int W_out, RegridTables tb,
                                                                   int levels) {
  extern __shared__ __attribute__((aligned(16))) float rg_row[];
  // Consecutive workgroup ids go round the 8 XCDs, each with its own L2; (plane, row) pairs are dealt so that every XCD takes one
  // contiguous run of them: the workgroups of rows J and J + 1 then meet in one L2, which serves the second read of their shared
  // edge row.  A bijection for any grid size; placement changes the speed only.
  const unsigned nwg = gridDim.x, per = nwg / RG_XCDS, extra = nwg % RG_XCDS, x = blockIdx.x % RG_XCDS;
  const int wg = (int)(x * per + (x < extra ? x : extra) + blockIdx.x / RG_XCDS);
  const int p = wg / H_out, J = wg - p * H_out;
  const int q = pk_src_plane(p, levels);
  const float* sp = src + (size_t)q * H_in * W_in;
  const float m = AFFINE ? mul[q] : 1.0f, a = AFFINE ? add[q] : 0.0f;
  // stage 2's operands for this lane's first output column are requested now: their latency passes under stage 1
  LonTaps taps = rg_lon_taps(tb, threadIdx.x < (unsigned)W_out ? (int)threadIdx.x : W_out - 1);
  const int n = tb.lat_count[J];
  const float* rows = sp + (size_t)tb.lat_start[J] * W_in;
  const float* w = tb.lat_w + (size_t)J * tb.lat_taps;
  const bool vec = (((size_t)sp & 15) == 0) && ((W_in & 3) == 0);      // every row of the plane 16-B aligned
  if (vec)
    rg_stage1<true, AFFINE>(n, rows, w, W_in, m, a, rg_row);
  else
    rg_stage1<false, AFFINE>(n, rows, w, W_in, m, a, rg_row);
  __syncthreads();
  float* op = dst + ((size_t)p * H_out + J) * W_out;
  for (int I = threadIdx.x; I < W_out;) {
    int i = taps.start;                         // in (-W_in, W_in): one wrap each way serves every tap
    if (i < 0) i += W_in;
    float acc = taps.w[0] * rg_row[i];
#pragma unroll
    for (int t = 1; t < RG_CHUNK; ++t) {
      if (++i >= W_in) i -= W_in;
      if (t < taps.count) acc = __builtin_fmaf(taps.w[t], rg_row[i], acc);
    }
    if (taps.count > RG_CHUNK) {                // (ratios above 7: the rest of the row, one tap at a time)
      const float* lw = tb.lon_w + (size_t)I * tb.lon_taps;
      for (int t = RG_CHUNK; t < taps.count; ++t) {
        if (++i >= W_in) i -= W_in;
        acc = __builtin_fmaf(lw[t], rg_row[i], acc);
      }
    }
    op[I] = acc;
    I += RG_THREADS;
    if (I < W_out) taps = rg_lon_taps(tb, I);
  }
}

}  // namespace

extern "C" int pangu_regrid_planes_f32(pangu_stream_t stream, const float* src, const float* mul, const float* add, float* dst,
                                       int planes, int H_in, int W_in, int H_out, int W_out, const int* lat_start,
                                       const int* lat_count, const float* lat_w, int lat_taps, const int* lon_start,
                                       const int* lon_count, const float* lon_w, int lon_taps, int levels) {
  if (!src || !dst || !lat_start || !lat_count || !lat_w || !lon_start || !lon_count || !lon_w) return PANGU_E_NULL;
  if ((mul == nullptr) != (add == nullptr)) return PANGU_E_NULL;
  if (planes <= 0 || H_in <= 0 || W_in <= 0 || H_out <= 0 || W_out <= 0) return PANGU_E_SHAPE;
  if (H_out > H_in || W_out > W_in) return PANGU_E_SHAPE;
  if (lat_taps < 1 || lat_taps > RG_MAX_TAPS || lon_taps < 1 || lon_taps > RG_MAX_TAPS) return PANGU_E_SHAPE;
  if (levels < 0 || (levels > 0 && planes % levels != 0)) return PANGU_E_SHAPE;
  if (W_in > RG_MAX_W) return PANGU_E_SHAPE;                                       // the LDS row
  if ((long long)H_in * W_in > 0x7fffffffll) return PANGU_E_SHAPE;                 // 32-bit indices within a plane
  if ((long long)planes * H_out > 0x7fffffffll) return PANGU_E_SHAPE;              // a one-dimensional grid
  if (((size_t)src & 3) || ((size_t)dst & 3)) return PANGU_E_ARG;
  const RegridTables tb{lat_start, lat_count, lat_w, lon_start, lon_count, lon_w, lat_taps, lon_taps};
  const dim3 grid((unsigned)((long long)planes * H_out)), block(RG_THREADS);
  const size_t lds = (((size_t)W_in + 3) & ~(size_t)3) * sizeof(float);
  if (mul)
    hipLaunchKernelGGL(regrid_planes_kernel<true>, grid, block, lds, (hipStream_t)stream, src, mul, add, dst, H_in, W_in, H_out,
                       W_out, tb, levels);
  else
    hipLaunchKernelGGL(regrid_planes_kernel<false>, grid, block, lds, (hipStream_t)stream, src, mul, add, dst, H_in, W_in, H_out,
                       W_out, tb, levels);
  return pangu_launch_status();
}
