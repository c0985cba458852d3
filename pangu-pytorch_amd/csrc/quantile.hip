// Ensemble quantile fields and quantile scores (fp32) for gfx950: Q order statistics of E member fields per grid point, and the
// pinball score and coverage that verify them, one streaming pass.
//
// pangu_ensemble_quantiles_f32 reads members x [E][planes][H][W], Q levels q_l in [0, 1] (host doubles) and optionally a target
// y [planes][H][W].  Per level, on the host in double:
//   h = q * (E - 1),   lo = floor(h),   frac = (float)(h - lo)            (0 <= lo <= E - 1; frac == 0 whenever lo == E - 1)
// Per grid point, x_(0) <= ... <= x_(E-1) are the point's RAW member values, sorted (not centred: a selection returns a member's
// bits unchanged).  The quantile is
//   frac == 0:  x_(lo)                                                     a pure selection, no arithmetic: q = 0, q = 1 and the
//                                                                          median of an odd E are member values bit for bit, also
//                                                                          when other members are +-inf;
//   otherwise:  fmin(fmax(fmaf(frac, x_(lo+1) - x_(lo), x_(lo)), x_(lo)), x_(lo+1))
// i.e. numpy's default "linear" method clamped into its bracket, so q1 <= q2 gives field(q1) <= field(q2) at every point.  fmin /
// fmax return the other operand when one is NaN: a bracket with an infinite end whose interpolation is inf - inf gives x_(lo).
// -0 and +0 compare equal: which of them a selection among equal zeros returns is not specified.
// NaN rule: a point where any member is NaN gets NaN in every quantile field, contributes nothing to the scores and counts, and
// is counted in nonfinite[plane] (as pangu_pack_planes_i16 reports non-finite values).  Infinite members are ordinary values.
// With a target, per (level l, plane p), u = y - x_q the fp32 difference to the very value written to fields:
//   pinball[l][p]        = (1 / HW) sum_{h,w} lat_w[h] * rho_q(u),   rho_q(u) = u * (q - (u < 0 ? 1 : 0))      (q as fp32)
//   coverage_count[l][p] = #{(h, w) : y <= x_q}                                                                (uint32, exact)
//   coverage_freq[l][p]  = (1 / HW) sum_{h,w} lat_w[h] * (y <= x_q ? 1 : 0)
// The integral of pinball over q is CRPS / 2.  A NaN target is not detected: it makes the plane's pinball NaN and covers nothing;
// an infinite quantile or target makes pinball +inf or NaN.
//
// Implementation: one workgroup per (plane, slab of QT_ROWS rows), a thread per grid point of the slab (the slab's rows are
// contiguous).  The E values go into P = next power of two >= E registers (pads +inf, they sort to the end), NaN is looked for
// pairwise (v_cmp_u_f32) and the static bitonic network of the stats kernel sorts them (bitonic_sort.h).  lo is wave-uniform but
// not a compile-time constant: x_(lo) is read with a binary select tree over the bits of lo (P - 1 v_cndmask on log2 P scalar
// conditions), which keeps the sorted array in VGPRs; a dynamic index would send it to scratch.  Interpolated levels run the tree
// twice, selections once.  Each thread keeps 3 Q score accumulators with the latitude weight folded in; the workgroup's sums go
// to the workspace in a fixed order (wave_sum, then the four waves), and a second launch adds the slabs in slab order in double:
// no atomics, every output is bit-identical from run to run.
#include "common.h"
#include "bitonic_sort.h"

#include <math.h>

namespace {

constexpr int QT_ROWS = 4;          // rows per workgroup (one slab), as the stats kernel
constexpr int QT_THREADS = 256;
constexpr int QT_MAX_Q = 8;

struct QuantileLevels {             // by value in the kernel arguments: wave-uniform
  int lo[QT_MAX_Q];
  float frac[QT_MAX_Q];             // 0: a pure selection
  float q[QT_MAX_Q];
};

// v[idx] for a wave-uniform idx without dynamic indexing of the register array: a binary tree over the bits of idx, N - 1
// v_cndmask on log2 N scalar conditions.  The two candidates are read into values first: `c ? v[a] : v[b]` on the array elements
// themselves is an lvalue conditional, i.e. a select of ADDRESSES followed by one load, and that dynamic address moves the array
// to scratch or LDS.
template <int N>
__device__ __forceinline__ float select_slot(const float (&v)[N], int idx) {
  if constexpr (N == 1) {
    return v[0];
  } else {
    float t[N / 2];
    const bool odd = (idx & 1) != 0;
#pragma unroll
    for (int i = 0; i < N / 2; ++i) {
      const float even_v = v[2 * i], odd_v = v[2 * i + 1];      // values, not lvalues: see above
      t[i] = odd ? odd_v : even_v;
    }
    return select_slot<N / 2>(t, idx >> 1);
  }
}

// workspace record of one workgroup, 3Q + 1 32-bit words: pinball partial [Q], coverage_freq partial [Q], coverage count [Q]
// (uint32), non-finite points (uint32)
template <int P, bool TGT>
__global__ __launch_bounds__(QT_THREADS) void ensemble_quantiles_kernel(const float* __restrict__ x, long long stride, int E,
                                                                        const QuantileLevels lev, int Q,
                                                                        const float* __restrict__ y,
                                                                        const float* __restrict__ lat_w, float* __restrict__ fields,
                                                                        uint32_t* __restrict__ ws, int planes, int H, int W,
                                                                        int slabs) {
  __shared__ float red[QT_THREADS / 64][3 * QT_MAX_Q + 1];
  const int plane = blockIdx.x / slabs, slab = blockIdx.x - plane * slabs;
  const int h0 = slab * QT_ROWS, rows = min(QT_ROWS, H - h0);
  const long long HW = (long long)H * W;
  const long long sbase = (long long)plane * HW + (long long)h0 * W;      // the slab's rows are contiguous
  const int items = rows * W;

  float pin[QT_MAX_Q], cov[QT_MAX_Q], cnt[QT_MAX_Q];      // cnt: point counts, at most 4 W < 2^24 per workgroup: exact in fp32
#pragma unroll
  for (int l = 0; l < QT_MAX_Q; ++l) pin[l] = cov[l] = cnt[l] = 0.0f;
  float bad_pts = 0.0f;

  for (int it = threadIdx.x; it < items; it += QT_THREADS) {
    const long long off = sbase + it;
    float v[P];
#pragma unroll
    for (int k = 0; k < P; ++k) v[k] = k < E ? x[off + k * stride] : __builtin_inff();
    bool bad = false;
#pragma unroll
    for (int k = 0; k < P; k += 2) bad |= __builtin_isunordered(v[k], v[k + 1]);
    bitonic_sort<P>(v);

    float yv = 0.0f, wt = 0.0f;
    if (TGT) {
      yv = y[off];
      wt = lat_w[h0 + it / W];      // it < rows * W: a row of this slab
    }
    bad_pts += bad ? 1.0f : 0.0f;
#pragma unroll
    for (int l = 0; l < QT_MAX_Q; ++l) {
      if (l < Q) {
        const int lo = lev.lo[l];
        const float fr = lev.frac[l];
        const float a = select_slot<P>(v, lo);
        float f = a;
        if (fr != 0.0f) {
          const float b = select_slot<P>(v, lo + 1);
          f = fminf(fmaxf(fmaf(fr, b - a, a), a), b);
        }
        if (bad) f = __builtin_nanf("");
        if (fields) fields[(long long)l * planes * HW + off] = f;
        if (TGT && !bad) {
          const float u = yv - f;
          pin[l] = fmaf(wt, u * (lev.q[l] - (u < 0.0f ? 1.0f : 0.0f)), pin[l]);
          const bool c = yv <= f;
          cov[l] += c ? wt : 0.0f;
          cnt[l] += c ? 1.0f : 0.0f;
        }
      }
    }
  }

  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  if (TGT) {
#pragma unroll
    for (int l = 0; l < QT_MAX_Q; ++l) {
      if (l < Q) {
        const float tp = wave_sum(pin[l]), tc = wave_sum(cov[l]), tn = wave_sum(cnt[l]);      // tn <= 4 W < 2^24: an exact integer
        if (lane == 0) { red[wave][l] = tp; red[wave][QT_MAX_Q + l] = tc; red[wave][2 * QT_MAX_Q + l] = tn; }
      }
    }
  }
  const float tb = wave_sum(bad_pts);
  if (lane == 0) red[wave][3 * QT_MAX_Q] = tb;
  __syncthreads();
  uint32_t* rec = ws + (long long)blockIdx.x * (3 * Q + 1);
  const int t = threadIdx.x;
  if (t < 3 * QT_MAX_Q + 1) {
    const float s = (red[0][t] + red[1][t]) + (red[2][t] + red[3][t]);
    const int kind = t / QT_MAX_Q, l = t - kind * QT_MAX_Q;      // kind 3: the non-finite count (l == 0)
    if (kind == 3) rec[3 * Q] = (uint32_t)s;
    else if (TGT && l < Q) rec[kind * Q + l] = kind == 2 ? (uint32_t)s : __builtin_bit_cast(uint32_t, s);
  }
}

// per (level, plane): the slab records added in slab order, counts as integers and the partials in double
__global__ __launch_bounds__(QT_THREADS) void ensemble_quantiles_final_kernel(const uint32_t* __restrict__ ws,
                                                                              float* __restrict__ pinball,
                                                                              uint32_t* __restrict__ coverage_count,
                                                                              float* __restrict__ coverage_freq,
                                                                              uint32_t* __restrict__ nonfinite, int planes, int slabs,
                                                                              int Q, int tgt, double inv_n) {
  const int i = blockIdx.x * QT_THREADS + threadIdx.x;
  if (i >= planes * Q) return;
  const int l = i / planes, plane = i - l * planes;
  const int rec = 3 * Q + 1;
  const uint32_t* p = ws + (long long)plane * slabs * rec;
  if (tgt) {
    double sp = 0.0, sc = 0.0;
    uint32_t n = 0u;
    for (int b = 0; b < slabs; ++b) {
      const uint32_t* r = p + (long long)b * rec;
      sp += (double)__builtin_bit_cast(float, r[l]);
      sc += (double)__builtin_bit_cast(float, r[Q + l]);
      n += r[2 * Q + l];
    }
    pinball[i] = (float)(sp * inv_n);
    coverage_freq[i] = (float)(sc * inv_n);
    coverage_count[i] = n;
  }
  if (l == 0) {
    uint32_t n = 0u;
    for (int b = 0; b < slabs; ++b) n += p[(long long)b * rec + 3 * Q];
    nonfinite[plane] = n;
  }
}

template <int P>
void launch_quantiles(hipStream_t s, int grid, const float* x, long long stride, int E, const QuantileLevels& lev, int Q,
                      const float* y, const float* w, float* fields, uint32_t* ws, int planes, int H, int W, int slabs) {
  if (y)
    hipLaunchKernelGGL((ensemble_quantiles_kernel<P, true>), dim3(grid), dim3(QT_THREADS), 0, s, x, stride, E, lev, Q, y, w, fields,
                       ws, planes, H, W, slabs);
  else
    hipLaunchKernelGGL((ensemble_quantiles_kernel<P, false>), dim3(grid), dim3(QT_THREADS), 0, s, x, stride, E, lev, Q, y, w, fields,
                       ws, planes, H, W, slabs);
}

}  // namespace

extern "C" long long pangu_ensemble_quantiles_ws_bytes(int planes, int H, int Q) {
  if (planes <= 0 || H <= 0 || Q < 1 || Q > QT_MAX_Q) return PANGU_E_SHAPE;
  const long long slabs = (H + QT_ROWS - 1) / QT_ROWS;
  if ((long long)planes * slabs > 0x7FFFFFFFll) return PANGU_E_SHAPE;
  return (long long)planes * slabs * (3 * Q + 1) * 4;
}

extern "C" int pangu_ensemble_quantiles_f32(pangu_stream_t stream, const float* members, long long member_stride, int E,
                                            const double* levels, int Q, const float* target, const float* lat_weight,
                                            float* fields, float* pinball, unsigned int* coverage_count, float* coverage_freq,
                                            unsigned int* nonfinite, void* workspace, long long workspace_bytes, int planes, int H,
                                            int W) {
  if (!members || !levels || !nonfinite || !workspace) return PANGU_E_NULL;
  if (!target && !fields) return PANGU_E_NULL;
  if (target && (!lat_weight || !pinball || !coverage_count || !coverage_freq)) return PANGU_E_NULL;
  if (E < 2 || E > 128 || Q < 1 || Q > QT_MAX_Q || planes <= 0 || H <= 0 || W <= 0 || (W & 3)) return PANGU_E_SHAPE;
  const long long HW = (long long)H * W, HWp = HW * planes;
  if (HW > 0x7FFFFFFFll) return PANGU_E_SHAPE;                          // 32-bit counts per plane
  if (W >= (1 << 22)) return PANGU_E_SHAPE;                             // a slab's point counts are exact as floats
  if (member_stride < HWp || (long long)(E - 1) * member_stride + HWp > (1ll << 40) || (long long)Q * HWp > (1ll << 40))
    return PANGU_E_SHAPE;
  const long long need = pangu_ensemble_quantiles_ws_bytes(planes, H, Q);
  if (need < 0) return PANGU_E_SHAPE;
  if ((long long)planes * Q > 0x7FFFFFFFll / 2) return PANGU_E_SHAPE;
  QuantileLevels lev = {};
  for (int l = 0; l < Q; ++l) {
    const double q = levels[l];
    if (!(q >= 0.0 && q <= 1.0)) return PANGU_E_ARG;                  // NaN included
    const double h = q * (double)(E - 1), fl = floor(h);
    lev.lo[l] = (int)fl;
    lev.frac[l] = (float)(h - fl);
    lev.q[l] = (float)q;
    if (lev.lo[l] >= E - 1) { lev.lo[l] = E - 1; lev.frac[l] = 0.0f; }  // q = 1 (the kernel reads slot lo + 1 when frac != 0)
  }
  if (workspace_bytes < need) return PANGU_E_ARG;
  if (reinterpret_cast<size_t>(workspace) & 3) return PANGU_E_ARG;
  hipStream_t s = (hipStream_t)stream;
  uint32_t* ws = static_cast<uint32_t*>(workspace);
  const int slabs = (H + QT_ROWS - 1) / QT_ROWS, grid = planes * slabs;
  const int P = E <= 2 ? 2 : E <= 4 ? 4 : E <= 8 ? 8 : E <= 16 ? 16 : E <= 32 ? 32 : E <= 64 ? 64 : 128;
  switch (P) {
    case 2: launch_quantiles<2>(s, grid, members, member_stride, E, lev, Q, target, lat_weight, fields, ws, planes, H, W, slabs); break;
    case 4: launch_quantiles<4>(s, grid, members, member_stride, E, lev, Q, target, lat_weight, fields, ws, planes, H, W, slabs); break;
    case 8: launch_quantiles<8>(s, grid, members, member_stride, E, lev, Q, target, lat_weight, fields, ws, planes, H, W, slabs); break;
    case 16: launch_quantiles<16>(s, grid, members, member_stride, E, lev, Q, target, lat_weight, fields, ws, planes, H, W, slabs); break;
    case 32: launch_quantiles<32>(s, grid, members, member_stride, E, lev, Q, target, lat_weight, fields, ws, planes, H, W, slabs); break;
    case 64: launch_quantiles<64>(s, grid, members, member_stride, E, lev, Q, target, lat_weight, fields, ws, planes, H, W, slabs); break;
    default: launch_quantiles<128>(s, grid, members, member_stride, E, lev, Q, target, lat_weight, fields, ws, planes, H, W, slabs); break;
  }
  const int rc = pangu_launch_status();
  if (rc != PANGU_OK) return rc;
  const int outs = planes * Q;
  hipLaunchKernelGGL(ensemble_quantiles_final_kernel, dim3((outs + QT_THREADS - 1) / QT_THREADS), dim3(QT_THREADS), 0, s, ws, pinball,
                     coverage_count, coverage_freq, nonfinite, planes, slabs, Q, target ? 1 : 0, 1.0 / (double)HW);
  return pangu_launch_status();
}
