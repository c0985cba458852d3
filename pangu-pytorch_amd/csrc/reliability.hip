// Ensemble reliability (fp32) for gfx950: verification rank histogram, reliability tables of threshold events and
// exceedance-probability fields of E member fields, one streaming pass.
//
// pangu_ensemble_reliability_f32 reads members x [E][planes][H][W], optionally a target y [planes][H][W], and T thresholds
// thr[t][plane].  Per grid point (h, w) of plane p, global plane id g = first_plane + p (the plane numbering of the
// perturbation, ensemble.hip: 0..64 upper, 65..68 surface):
//   less = #{i : x_i < y},  ties = #{i : x_i == y},
//   u    = lowbias32(lowbias32(lowbias32(seed) ^ g) ^ (uint32)(h*W + w))           (lowbias32: common.h)
//   rank = less + (uint32)(((uint64)u * (ties + 1)) >> 32)                           (0..E; no ties: rank = less; ties are
//                                                                                     broken uniformly, integers only)
//   k_t  = #{i : x_i > thr[t][p]}  (strict),   o_t = (y > thr[t][p])                 for t < T.
// Tables per plane, E + 1 bins each:   table 0: counts[rank] += 1;   table 1 + 2t: N_t[k_t] += 1;   table 2 + 2t:
// O_t[k_t] += o_t.  freq is the same table with each point weighted by lat_weight[h] and divided by H*W;
// prob[t][p][h][w] = k_t / E.  Without a target, table 0 and every O_t are zero; N_t and prob are as with one.
// Non-finite values are not detected: a comparison with NaN is false (a NaN member counts nowhere, a NaN target gives rank 0
// and o_t = 0), and a threshold of +inf is an event that never happens.
//
// Implementation: one workgroup per (plane, slab of RL_ROWS rows).  A thread owns four neighbouring grid points, holds y and the
// thresholds, and streams the members with RL_UNROLL 16-byte loads in flight: no member stays live, VGPR use does not depend on
// E.  The points go into per-row integer tables in LDS (integer LDS atomics: order-independent).  After the slab one thread per
// bin forms the integer sum over the rows and the fp32 partial sum_h w_h * c_h[bin] in row order and writes both to the
// workspace; a second launch adds the slabs in slab order, counts as integers and the partials in double.  No floating-point
// atomics: counts are exact and freq is bit-identical from run to run.  freq differs from the exactly weighted sum of the
// counts by at most 4 fp32 roundings per slab partial (2.4e-7 of the terms' magnitudes), the double sum and one final rounding.
#include "common.h"

namespace {

constexpr int RL_ROWS = 4;          // rows per workgroup (one slab), as the stats kernel
constexpr int RL_THREADS = 256;
constexpr int RL_UNROLL = 4;        // member loads in flight per thread (16 B each)
constexpr int RL_MAX_T = 4;

// TMAX thresholds are counted (0: rank table only; 4: unused ones are +inf and their tables are not written); TGT: a target
template <int TMAX, bool TGT>
__device__ __forceinline__ void rl_count(const f32x4 x, const f32x4 y, const float (&thr)[RL_MAX_T], uint32_t (&less)[4],
                                         uint32_t (&ties)[4], uint32_t (&k)[RL_MAX_T][4]) {
#pragma unroll
  for (int q = 0; q < 4; ++q) {
    if (TGT) {
      less[q] += x[q] < y[q] ? 1u : 0u;
      ties[q] += x[q] == y[q] ? 1u : 0u;
    }
#pragma unroll
    for (int t = 0; t < TMAX; ++t) k[t][q] += x[q] > thr[t] ? 1u : 0u;
  }
}

template <int TMAX, bool TGT>
__global__ __launch_bounds__(RL_THREADS) void ensemble_reliability_kernel(
    const float* __restrict__ x, long long stride, int E, const float* __restrict__ y, const float* __restrict__ thresholds, int T,
    const float* __restrict__ lat_w, uint32_t seed, int first_plane, float* __restrict__ prob, uint32_t* __restrict__ ws_counts,
    float* __restrict__ ws_part, int planes, int H, int W, int slabs) {
  extern __shared__ __attribute__((aligned(16))) uint32_t rl_tab[];      // [RL_ROWS][1 + 2T][E + 1]
  const int plane = blockIdx.x / slabs, slab = blockIdx.x - plane * slabs;
  const int h0 = slab * RL_ROWS, rows = min(RL_ROWS, H - h0);
  const int bins = E + 1, nt = 1 + 2 * T, per_row = nt * bins;
  for (int i = threadIdx.x; i < RL_ROWS * per_row; i += RL_THREADS) rl_tab[i] = 0u;

  float thr[RL_MAX_T];
#pragma unroll
  for (int t = 0; t < RL_MAX_T; ++t) thr[t] = t < T ? thresholds[(long long)t * planes + plane] : __builtin_inff();
  const uint32_t hp = lowbias32(lowbias32(seed) ^ (uint32_t)(first_plane + plane));
  const long long HW = (long long)H * W;
  const long long sbase = (long long)plane * HW + (long long)h0 * W;      // the slab's rows are contiguous
  const int w4 = W >> 2, items = rows * w4;
  __syncthreads();

  for (int it = threadIdx.x; it < items; it += RL_THREADS) {
    const long long off = sbase + 4ll * it;
    const float* px = x + off;
    f32x4 yv = {0.f, 0.f, 0.f, 0.f};
    if (TGT) yv = *reinterpret_cast<const f32x4*>(y + off);
    uint32_t less[4] = {0u, 0u, 0u, 0u}, ties[4] = {0u, 0u, 0u, 0u}, k[RL_MAX_T][4] = {};
    int e = 0;
    for (; e + RL_UNROLL <= E; e += RL_UNROLL) {
      f32x4 v[RL_UNROLL];
#pragma unroll
      for (int j = 0; j < RL_UNROLL; ++j) v[j] = *reinterpret_cast<const f32x4*>(px + (long long)j * stride);
      px += (long long)RL_UNROLL * stride;
#pragma unroll
      for (int j = 0; j < RL_UNROLL; ++j) rl_count<TMAX, TGT>(v[j], yv, thr, less, ties, k);
    }
    for (; e < E; ++e) {
      const f32x4 v = *reinterpret_cast<const f32x4*>(px);
      px += stride;
      rl_count<TMAX, TGT>(v, yv, thr, less, ties, k);
    }

    const int r = it / w4, c4 = (it - r * w4) << 2;
    uint32_t* row_tab = rl_tab + r * per_row;
    if (TGT) {
      const uint32_t pt = (uint32_t)(h0 + r) * (uint32_t)W + (uint32_t)c4;
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        const uint32_t u = lowbias32(hp ^ (pt + (uint32_t)q));
        atomicAdd(row_tab + less[q] + __umulhi(u, ties[q] + 1u), 1u);
      }
    }
#pragma unroll
    for (int t = 0; t < TMAX; ++t) {
      if (t < T) {
        uint32_t* nt_tab = row_tab + (1 + 2 * t) * bins;
        f32x4 pv;
#pragma unroll
        for (int q = 0; q < 4; ++q) {
          atomicAdd(nt_tab + k[t][q], 1u);
          if (TGT && yv[q] > thr[t]) atomicAdd(nt_tab + bins + k[t][q], 1u);
          pv[q] = (float)k[t][q] / (float)E;          // correctly rounded: within half an ulp of k / E
        }
        if (prob) *reinterpret_cast<f32x4*>(prob + ((long long)t * planes * HW + off)) = pv;
      }
    }
  }
  __syncthreads();

  // one thread per (table, bin): the slab's integer count and its weighted fp32 partial, rows in order
  float wr[RL_ROWS];
#pragma unroll
  for (int r = 0; r < RL_ROWS; ++r) wr[r] = r < rows ? lat_w[h0 + r] : 0.0f;
  const long long obase = (long long)blockIdx.x * per_row;
  for (int i = threadIdx.x; i < per_row; i += RL_THREADS) {
    uint32_t n = 0u;
    float s = 0.0f;
#pragma unroll
    for (int r = 0; r < RL_ROWS; ++r) {
      const uint32_t c = rl_tab[r * per_row + i];      // <= W < 2^24: exact as a float
      n += c;
      s = fmaf(wr[r], (float)c, s);
    }
    ws_counts[obase + i] = n;
    ws_part[obase + i] = s;
  }
}

// counts / freq [plane][table][bin] from the slab partials, added in slab order: integers, and the weighted partials in double
__global__ __launch_bounds__(RL_THREADS) void ensemble_reliability_final_kernel(const uint32_t* __restrict__ ws_counts,
                                                                                const float* __restrict__ ws_part,
                                                                                uint32_t* __restrict__ counts,
                                                                                float* __restrict__ freq, int planes, int slabs,
                                                                                int per_row, double inv_n) {
  const long long i = (long long)blockIdx.x * RL_THREADS + threadIdx.x;
  if (i >= (long long)planes * per_row) return;
  const long long plane = i / per_row, b = i - plane * per_row;
  const long long base = plane * slabs * per_row + b;
  uint32_t n = 0u;
  double s = 0.0;
  for (int sl = 0; sl < slabs; ++sl) {
    n += ws_counts[base + (long long)sl * per_row];
    s += (double)ws_part[base + (long long)sl * per_row];
  }
  counts[i] = n;
  freq[i] = (float)(s * inv_n);
}

template <int TMAX, bool TGT>
void launch_reliability(hipStream_t s, int grid, size_t lds, const float* x, long long stride, int E, const float* y,
                        const float* thr, int T, const float* w, uint32_t seed, int first_plane, float* prob, uint32_t* wc,
                        float* wp, int planes, int H, int W, int slabs) {
  hipLaunchKernelGGL((ensemble_reliability_kernel<TMAX, TGT>), dim3(grid), dim3(RL_THREADS), lds, s, x, stride, E, y, thr, T, w, seed,
                     first_plane, prob, wc, wp, planes, H, W, slabs);
}

}  // namespace

extern "C" int pangu_ensemble_reliability_f32(pangu_stream_t stream, const float* members, long long member_stride, int E,
                                              const float* target, const float* thresholds, int T, const float* lat_weight,
                                              unsigned int seed, int first_plane, unsigned int* counts, float* freq, float* prob,
                                              void* workspace, long long workspace_bytes, int planes, int H, int W) {
  if (!members || !lat_weight || !counts || !freq || !workspace) return PANGU_E_NULL;
  if ((T > 0 && !thresholds) || (T == 0 && prob) || (T == 0 && !target)) return PANGU_E_NULL;
  if (E < 2 || E > 128 || T < 0 || T > RL_MAX_T || first_plane < 0 || planes <= 0 || H <= 0 || W <= 0 || (W & 3))
    return PANGU_E_SHAPE;
  const long long HW = (long long)H * W, HWp = HW * planes;
  if (HW > 0x7FFFFFFFll || W >= (1 << 24)) return PANGU_E_SHAPE;      // 32-bit counts per plane, exact float counts per row
  if (member_stride < HWp || (member_stride & 3) || (long long)(E - 1) * member_stride + HWp > (1ll << 40)) return PANGU_E_SHAPE;
  const int slabs = (H + RL_ROWS - 1) / RL_ROWS;
  if ((long long)planes * slabs > 0x7FFFFFFFll) return PANGU_E_SHAPE;
  const long long per_row = (long long)(1 + 2 * T) * (E + 1);
  const long long cells = (long long)planes * slabs * per_row;          // workspace: cells uint32 counts, then cells floats
  if (workspace_bytes < cells * 8) return PANGU_E_ARG;
  if ((reinterpret_cast<size_t>(members) | reinterpret_cast<size_t>(target) | reinterpret_cast<size_t>(counts) |
       reinterpret_cast<size_t>(freq) | reinterpret_cast<size_t>(prob) | reinterpret_cast<size_t>(workspace)) & 15)
    return PANGU_E_ARG;
  hipStream_t s = (hipStream_t)stream;
  uint32_t* wc = static_cast<uint32_t*>(workspace);
  float* wp = reinterpret_cast<float*>(wc + cells);
  const int grid = planes * slabs;
  const size_t lds = (size_t)RL_ROWS * per_row * sizeof(uint32_t);      // <= 4 * 9 * 129 * 4 = 18576 B
  if (T == 0)
    launch_reliability<0, true>(s, grid, lds, members, member_stride, E, target, thresholds, T, lat_weight, seed, first_plane, prob,
                                wc, wp, planes, H, W, slabs);
  else if (target)
    launch_reliability<RL_MAX_T, true>(s, grid, lds, members, member_stride, E, target, thresholds, T, lat_weight, seed, first_plane,
                                       prob, wc, wp, planes, H, W, slabs);
  else
    launch_reliability<RL_MAX_T, false>(s, grid, lds, members, member_stride, E, target, thresholds, T, lat_weight, seed, first_plane,
                                        prob, wc, wp, planes, H, W, slabs);
  const int rc = pangu_launch_status();
  if (rc != PANGU_OK) return rc;
  const long long outs = (long long)planes * per_row;
  hipLaunchKernelGGL(ensemble_reliability_final_kernel, dim3((unsigned)((outs + RL_THREADS - 1) / RL_THREADS)), dim3(RL_THREADS), 0, s,
                     wc, wp, counts, freq, planes, slabs, (int)per_row, 1.0 / (double)HW);
  return pangu_launch_status();
}
