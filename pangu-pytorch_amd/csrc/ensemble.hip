// Ensemble kernels (fp32) for gfx950: perturbed initial states and on-device ensemble scores.
//
// pangu_ensemble_perturb_f32 adds spatially correlated noise, in place, to E member states upper (E,5,13,H,W) and
// surface (E,4,H,W).  The noise of member m = first_member + e on plane p (p = var*13 + level for the upper variables,
// 65 + var for the surface) at grid point (h, w) is
//   noise = sum_{o < octaves} persistence^o * perlin_o(h, w)
// with perlin_o the 2-D gradient noise of octave o:
//   L = period * 2^o lattice cells around the longitude circle, cell width s = W / L grid points (W % L == 0);
//   ix = w / s, fx = (w - ix*s) / s, iy = h / s, fy = (h - iy*s) / s (integers; rows counted from row 0);
//   corner (j, i), j in {iy, iy+1}, i in {ix, ix+1}, has the gradient (cos t, sin t), t = 2 pi * h32 * 2^-32, where
//     h32 = lowbias32(lowbias32(lowbias32(lowbias32(lowbias32(seed) ^ m) ^ plane) ^ o) ^ (j*L + (i mod L)))   (uint32),
//     lowbias32(x): x ^= x>>16; x *= 0x7feb352d; x ^= x>>15; x *= 0x846ca68b; x ^= x>>16
//   (i mod L: the lattice wraps at the dateline, the field has no seam there);
//   d_ji = g_ji . (fx - (i - ix), fy - (j - iy));  u = fade(fx), v = fade(fy), fade(t) = t^3 (t (6t - 15) + 10);
//   perlin_o = lerp(lerp(d_00, d_01, u), lerp(d_10, d_11, u), v)      (d_ji: row j - iy, column i - ix).
// The perturbation is amplitude[var] * std[plane] * noise.  With `control`, member m = 0 is not touched (bit-identical).
// The noise is a function of (seed, m, plane, h, w) alone, so a member gets the same field in any chunk or batch.
//
// Implementation: one workgroup per (member, plane, EP_ROWS rows).  The bilinear blend is regrouped by lattice column:
//   perlin_o = (1-u) (A_ix fx + B_ix) + u (A_ix+1 (fx-1) + B_ix+1),
//   A_i = (1-v) gx(iy,i) + v gx(iy+1,i),  B_i = (1-v) gy(iy,i) fy + v gy(iy+1,i) (fy-1),
// so the workgroup first tabulates (A_i, B_i) of its rows for every octave in LDS (the only hashes and sincos), and each
// grid point then costs two LDS reads and four FMAs per octave and row.  Equal to the definition above up to fp32 rounding.
//
// pangu_ensemble_stats_f32 reduces E member fields (and a target) to latitude-weighted scores per plane in one pass:
// per grid point the E values are held in registers, the mean, unbiased variance and sum |x_i - y| are formed directly,
// and the pairwise CRPS term uses sum_ij |x_i - x_j| = 2 sum_k (2k - E - 1) x_(k) (k = 1..E, x_(k) the sorted values) after a
// static bitonic sorting network over P = next power of two >= E values (pads are +inf and sort to the end).  That costs
// P log2 P (log2 P + 1) / 2 min/max per point (3584 at E = 100) against E (E - 1) for the pair sum (9900 at E = 100): the pair
// sum's VALU time alone would reach the 2x-HBM target at E = 100.  Values are centred on the mean before the sort so the
// weighted sum cancels little.  Each workgroup writes its six partial sums to a workspace and one launch adds them per plane
// in slab order: no atomics, bit-identical from run to run.
#include "common.h"
#include "bitonic_sort.h"

namespace {

// (lowbias32: common.h)
__device__ inline float fade(float t) { return t * t * t * fmaf(t, fmaf(t, 6.0f, -15.0f), 10.0f); }

constexpr int EP_ROWS = 4;          // rows per workgroup: every LDS table read serves all of them
constexpr int EP_THREADS = 256;
constexpr int EP_MAX_OCT = 8;
constexpr int EP_MAX_NODES = 1024;  // sum over octaves of (L + 1) lattice columns: LDS = EP_ROWS * 8 B * nodes <= 32 KB

struct OctaveParams {
  int L, s, off;      // lattice columns, cell width, first table column of the octave
  float inv_s, wt;    // 1 / s, persistence^o
};

// q = n / s and the remainder, exact for 0 <= n < 2^24 (one float estimate, one correction step)
__device__ inline int div_small(int n, int s, float inv_s, int& rem) {
  int q = (int)((float)n * inv_s);
  int r = n - q * s;
  if (r >= s) { ++q; r -= s; }
  if (r < 0) { --q; r += s; }
  rem = r;
  return q;
}

__global__ __launch_bounds__(EP_THREADS) void ensemble_perturb_kernel(float* __restrict__ upper, long long su,
                                                                      float* __restrict__ surface, long long ss, int first_member,
                                                                      int H, int W, const float* __restrict__ amplitude,
                                                                      const float* __restrict__ ustd,
                                                                      const float* __restrict__ sstd, uint32_t seed, int octaves,
                                                                      int period, float persistence, int control, int nodes) {
  extern __shared__ __attribute__((aligned(16))) float ep_lds[];
  float2* tab = reinterpret_cast<float2*>(ep_lds);      // [node][EP_ROWS] (A, B)
  __shared__ OctaveParams prm[EP_MAX_OCT];

  const int m = first_member + (int)blockIdx.z;
  if (control && m == 0) return;
  const int plane = blockIdx.y;
  const int h0 = blockIdx.x * EP_ROWS;
  const int HW = H * W;
  float* base = plane < 65 ? upper + (long long)blockIdx.z * su + (long long)plane * HW
                           : surface + (long long)blockIdx.z * ss + (long long)(plane - 65) * HW;
  const int var = plane < 65 ? plane / 13 : 5 + (plane - 65);
  const float scale = amplitude[var] * (plane < 65 ? ustd[plane] : sstd[plane - 65]);
  const uint32_t hm = lowbias32(lowbias32(lowbias32(seed) ^ (uint32_t)m) ^ (uint32_t)plane);

  if (threadIdx.x == 0) {
    int off = 0;
    float wt = 1.0f;
    for (int o = 0; o < octaves; ++o) {
      const int L = period << o, s = W / L;
      prm[o] = OctaveParams{L, s, off, 1.0f / (float)s, wt};
      off += L + 1;
      wt *= persistence;
    }
  }
  __syncthreads();

  // lattice tables: (A_i, B_i) of every row of this workgroup, octave and column i = 0..L (column L wraps to 0)
  for (int t = threadIdx.x; t < nodes * EP_ROWS; t += EP_THREADS) {
    const int node = t / EP_ROWS, r = t - node * EP_ROWS;
    int o = 0;
    while (o + 1 < octaves && node >= prm[o + 1].off) ++o;
    const OctaveParams p = prm[o];
    const int i = node - p.off, im = i == p.L ? 0 : i;
    int rem;
    const int iy = div_small(h0 + r, p.s, p.inv_s, rem);
    const float fy = (float)rem * p.inv_s, v = fade(fy);
    const uint32_t ho = lowbias32(hm ^ (uint32_t)o);
    const uint32_t c0 = (uint32_t)iy * (uint32_t)p.L + (uint32_t)im;
    float s0, g0x, s1, g1x;
    sincospif((float)lowbias32(ho ^ c0) * 0x1p-31f, &s0, &g0x);
    sincospif((float)lowbias32(ho ^ (c0 + (uint32_t)p.L)) * 0x1p-31f, &s1, &g1x);
    const float A = fmaf(v, g1x - g0x, g0x);
    const float b0 = s0 * fy, b1 = s1 * (fy - 1.0f);
    tab[t] = make_float2(A, fmaf(v, b1 - b0, b0));
  }
  __syncthreads();

  const int rows = min(EP_ROWS, H - h0);
  const int w4 = W >> 2;
  for (int c = threadIdx.x; c < w4; c += EP_THREADS) {
    float acc[EP_ROWS][4];
#pragma unroll
    for (int r = 0; r < EP_ROWS; ++r)
#pragma unroll
      for (int q = 0; q < 4; ++q) acc[r][q] = 0.0f;
    for (int o = 0; o < octaves; ++o) {
      const OctaveParams p = prm[o];
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        int rem;
        const int ix = div_small(4 * c + q, p.s, p.inv_s, rem);
        const float fx = (float)rem * p.inv_s, u = fade(fx);
        const float4* t0 = reinterpret_cast<const float4*>(tab + (p.off + ix) * EP_ROWS);
        const float4 a01 = t0[0], a23 = t0[1], b01 = t0[2], b23 = t0[3];   // column ix rows 0-3, column ix+1 rows 0-3
        const float ea[EP_ROWS] = {fmaf(a01.x, fx, a01.y), fmaf(a01.z, fx, a01.w), fmaf(a23.x, fx, a23.y), fmaf(a23.z, fx, a23.w)};
        const float fx1 = fx - 1.0f;
        const float eb[EP_ROWS] = {fmaf(b01.x, fx1, b01.y), fmaf(b01.z, fx1, b01.w), fmaf(b23.x, fx1, b23.y), fmaf(b23.z, fx1, b23.w)};
#pragma unroll
        for (int r = 0; r < EP_ROWS; ++r) acc[r][q] = fmaf(p.wt, fmaf(u, eb[r] - ea[r], ea[r]), acc[r][q]);
      }
    }
#pragma unroll
    for (int r = 0; r < EP_ROWS; ++r) {
      if (r < rows) {
        f32x4* px = reinterpret_cast<f32x4*>(base + (long long)(h0 + r) * W) + c;
        f32x4 x = *px;
#pragma unroll
        for (int q = 0; q < 4; ++q) x[q] = fmaf(scale, acc[r][q], x[q]);
        *px = x;
      }
    }
  }
}

// ---- scores --------------------------------------------------------------------------------------------------------

constexpr int ES_ROWS = 4;          // rows per workgroup (one slab)
constexpr int ES_THREADS = 256;
constexpr int ES_PART = 8;          // floats per slab partial (6 used)

// (bitonic_sort<P>: bitonic_sort.h)

template <int P>
__global__ __launch_bounds__(ES_THREADS) void ensemble_stats_kernel(const float* __restrict__ x, long long stride, int E,
                                                                    const float* __restrict__ y, const float* __restrict__ clim,
                                                                    const float* __restrict__ lat_w, float* __restrict__ mean_out,
                                                                    float* __restrict__ std_out, float* __restrict__ ws, int H,
                                                                    int W, int slabs) {
  __shared__ float red[ES_THREADS / 64][6];
  const int plane = blockIdx.x / slabs, slab = blockIdx.x - plane * slabs;
  const long long pbase = (long long)plane * H * W;
  const int h0 = slab * ES_ROWS, h1 = min(H, h0 + ES_ROWS);
  const bool tgt = y != nullptr;
  const float c = tgt ? clim[plane] : 0.0f;
  const float invE = 1.0f / (float)E, invE1 = 1.0f / (float)(E - 1), invEE1 = 1.0f / ((float)E * (float)(E - 1));
  float S[6] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
  for (int h = h0; h < h1; ++h) {
    float a[6] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
    for (int w = threadIdx.x; w < W; w += ES_THREADS) {
      const long long off = pbase + (long long)h * W + w;
      float v[P];
#pragma unroll
      for (int k = 0; k < P; ++k) v[k] = k < E ? x[off + k * stride] : 0.0f;
      float sum = 0.0f;
#pragma unroll
      for (int k = 0; k < P; ++k) sum += v[k];                // pads are 0
      const float m = sum * invE;
      const float yv = tgt ? y[off] : 0.0f;
      float q = 0.0f, mae = 0.0f;
#pragma unroll
      for (int k = 0; k < P; ++k) {
        if (k < E) {
          mae += fabsf(v[k] - yv);
          v[k] -= m;
          q = fmaf(v[k], v[k], q);
        } else {
          v[k] = __builtin_inff();
        }
      }
      const float var = q * invE1;
      if (mean_out) mean_out[off] = m;
      if (std_out) std_out[off] = sqrtf(var);
      a[4] += var;
      if (tgt) {
        bitonic_sort<P>(v);
        float pair = 0.0f;
#pragma unroll
        for (int k = 0; k < P; ++k)
          if (k < E) pair = fmaf((float)(2 * k + 1 - E), v[k], pair);
        const float dm = m - yv, mc = m - c, yc = yv - c;
        a[0] = fmaf(dm, dm, a[0]);
        a[1] = fmaf(mc, yc, a[1]);
        a[2] = fmaf(mc, mc, a[2]);
        a[3] = fmaf(yc, yc, a[3]);
        a[5] += mae * invE - pair * invEE1;
      }
    }
    const float wt = lat_w[h];
#pragma unroll
    for (int k = 0; k < 6; ++k) S[k] = fmaf(wt, a[k], S[k]);
  }
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
  for (int k = 0; k < 6; ++k) {
    const float t = wave_sum(S[k]);
    if (lane == 0) red[wave][k] = t;
  }
  __syncthreads();
  if (threadIdx.x < 6) {
    const int k = threadIdx.x;
    ws[(long long)blockIdx.x * ES_PART + k] = (red[0][k] + red[1][k]) + (red[2][k] + red[3][k]);
  }
}

// out[plane] = {rmse_mean, acc_mean, spread, crps} from the slab partials, summed in slab order
__global__ __launch_bounds__(64) void ensemble_stats_final_kernel(const float* __restrict__ ws, float* __restrict__ out,
                                                                 int planes, int slabs, int n, int tgt) {
  const int plane = blockIdx.x * 64 + threadIdx.x;
  if (plane >= planes) return;
  double s[6] = {0, 0, 0, 0, 0, 0};
  for (int b = 0; b < slabs; ++b) {
    const float* p = ws + ((long long)plane * slabs + b) * ES_PART;
#pragma unroll
    for (int k = 0; k < 6; ++k) s[k] += (double)p[k];
  }
  const float nan = __builtin_nanf("");
  const double inv_n = 1.0 / (double)n;
  f32x4 r;
  r[0] = tgt ? (float)sqrt(s[0] * inv_n) : nan;
  r[1] = tgt ? (float)(s[1] / sqrt(s[2] * s[3])) : nan;
  r[2] = (float)sqrt(s[4] * inv_n);
  r[3] = tgt ? (float)(s[5] * inv_n) : nan;
  reinterpret_cast<f32x4*>(out)[plane] = r;
}

template <int P>
void launch_stats(hipStream_t s, int grid, const float* x, long long stride, int E, const float* y, const float* clim,
                  const float* w, float* mean_out, float* std_out, float* ws, int H, int W, int slabs) {
  hipLaunchKernelGGL(ensemble_stats_kernel<P>, dim3(grid), dim3(ES_THREADS), 0, s, x, stride, E, y, clim, w, mean_out, std_out,
                     ws, H, W, slabs);
}

}  // namespace

extern "C" int pangu_ensemble_perturb_f32(pangu_stream_t stream, float* upper, long long upper_member_stride, float* surface,
                                          long long surface_member_stride, int E, int first_member, int H, int W,
                                          const float* amplitude, const float* upper_std, const float* surface_std,
                                          unsigned int seed, int octaves, int period, float persistence, int control) {
  if (!upper || !surface || !amplitude || !upper_std || !surface_std) return PANGU_E_NULL;
  if (E < 1 || E > 65535 || first_member < 0 || H <= 0 || W <= 0 || (W & 3) || octaves < 1 || octaves > EP_MAX_OCT ||
      period <= 0)
    return PANGU_E_SHAPE;
  const long long HW = (long long)H * W;
  if (HW * 65 > 0x7FFFFFFFll || upper_member_stride < 65 * HW || surface_member_stride < 4 * HW ||
      (upper_member_stride & 3) || (surface_member_stride & 3))
    return PANGU_E_SHAPE;
  long long nodes = 0;
  for (int o = 0; o < octaves; ++o) {
    const long long L = (long long)period << o;
    if (L > W || W % L) return PANGU_E_SHAPE;                  // whole cells around the longitude circle
    nodes += L + 1;
  }
  if (nodes > EP_MAX_NODES) return PANGU_E_SHAPE;
  if ((reinterpret_cast<size_t>(upper) | reinterpret_cast<size_t>(surface)) & 15) return PANGU_E_ARG;
  const size_t lds = (size_t)nodes * EP_ROWS * sizeof(float2);
  hipLaunchKernelGGL(ensemble_perturb_kernel, dim3((H + EP_ROWS - 1) / EP_ROWS, 69, E), dim3(EP_THREADS), lds,
                     (hipStream_t)stream, upper, upper_member_stride, surface, surface_member_stride, first_member, H, W,
                     amplitude, upper_std, surface_std, (uint32_t)seed, octaves, period, persistence, control, (int)nodes);
  return pangu_launch_status();
}

extern "C" int pangu_ensemble_stats_f32(pangu_stream_t stream, const float* members, long long member_stride, int E,
                                        const float* target, const float* clim, const float* lat_weight, float* out,
                                        float* mean_out, float* std_out, float* workspace, long long workspace_bytes,
                                        int planes, int H, int W) {
  if (!members || !lat_weight || !out || !workspace || (target && !clim)) return PANGU_E_NULL;
  if (E < 2 || E > 128 || planes <= 0 || H <= 0 || W <= 0 || (W & 3)) return PANGU_E_SHAPE;
  const long long HWp = (long long)planes * H * W;
  if (member_stride < HWp || (long long)(E - 1) * member_stride + HWp > (1ll << 40)) return PANGU_E_SHAPE;
  const int slabs = (H + ES_ROWS - 1) / ES_ROWS;
  if ((long long)planes * slabs > 0x7FFFFFFFll) return PANGU_E_SHAPE;
  if (workspace_bytes < (long long)planes * slabs * ES_PART * (long long)sizeof(float)) return PANGU_E_ARG;
  if (reinterpret_cast<size_t>(out) & 15) return PANGU_E_ARG;
  hipStream_t s = (hipStream_t)stream;
  const int grid = planes * slabs;
  const int P = E <= 2 ? 2 : E <= 4 ? 4 : E <= 8 ? 8 : E <= 16 ? 16 : E <= 32 ? 32 : E <= 64 ? 64 : 128;
  switch (P) {
    case 2: launch_stats<2>(s, grid, members, member_stride, E, target, clim, lat_weight, mean_out, std_out, workspace, H, W, slabs); break;
    case 4: launch_stats<4>(s, grid, members, member_stride, E, target, clim, lat_weight, mean_out, std_out, workspace, H, W, slabs); break;
    case 8: launch_stats<8>(s, grid, members, member_stride, E, target, clim, lat_weight, mean_out, std_out, workspace, H, W, slabs); break;
    case 16: launch_stats<16>(s, grid, members, member_stride, E, target, clim, lat_weight, mean_out, std_out, workspace, H, W, slabs); break;
    case 32: launch_stats<32>(s, grid, members, member_stride, E, target, clim, lat_weight, mean_out, std_out, workspace, H, W, slabs); break;
    case 64: launch_stats<64>(s, grid, members, member_stride, E, target, clim, lat_weight, mean_out, std_out, workspace, H, W, slabs); break;
    default: launch_stats<128>(s, grid, members, member_stride, E, target, clim, lat_weight, mean_out, std_out, workspace, H, W, slabs); break;
  }
  const int rc = pangu_launch_status();
  if (rc != PANGU_OK) return rc;
  hipLaunchKernelGGL(ensemble_stats_final_kernel, dim3((planes + 63) / 64), dim3(64), 0, s, workspace, out, planes, slabs,
                     H * W, target ? 1 : 0);
  return pangu_launch_status();
}
