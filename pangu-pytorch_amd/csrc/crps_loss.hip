// Fair-CRPS training loss over E ensemble members, one pass over the fields per direction.  Per grid point, with x_e the members'
// normalised outputs and t the normalised target (the fair CRPS score.ensemble_scores reports, csrc/ensemble.hip):
//   c = (1/E) sum_e |x_e - t|  -  1/(2E(E-1)) sum_e sum_f |x_e - x_f|
//   loss = mean_{v,l,h,w}(w_u[v] a[h] c) + 0.25 * mean_{v,h,w}(w_s[v] a[h] c_s)          (weighted_l1_loss's shape, csrc/loss.hip)
// a[h]: the latitude weight of row h (lat_weight, H floats; null = 1).  Backward, g the incoming scalar gradient, k = 1/n_u (upper)
// or 0.25/n_s (surface), sign(0) = 0 (what torch's autograd gives for ties between members and with the target):
//   d x_e = g k w[v] a[h] (sign(x_e - t)/E - sum_f sign(x_e - x_f) / (E(E-1)))
//         = g k w[v] a[h] * n_e / (E(E-1)),   n_e = (E-1) sign(x_e - t) - sum_f sign(x_e - x_f)   (an integer: exact in fp32)
// As torch ops the pair term is O(E^2) passes over the 286 MB fields; here every member and the target are read once and the E
// values of an element stay in registers (the kernels are instantiated per E, 2..16; the plain pair sum is E(E-1)/2 subtractions).
// Members arrive as E separate fields (the outputs of E forwards), their addresses in the kernel-argument struct.
// The target side is loss.hip's: normalised on the fly from physical units (loss_target.h), level reversal as an address.
// A block owns CHUNK consecutive elements of ONE (sample, variable, level) plane, so variable weight, statistics and the target's
// plane are block-uniform; the latitude weight is looked up per 16-byte vector (row = index / W: W % 4 == 0 on that path, so a
// vector never straddles rows) or per element (scalar path).  Block partials in fp32, one fixed-order fp64 final launch: no
// atomics, the same bits every run.
#include "common.h"
#include "loss_target.h"

namespace {

constexpr int CRPS_MAX_E = 16;

// 16-byte vectors per thread and batch: about 16 member vectors (plus the targets) in flight per thread whatever E is
__host__ __device__ constexpr int crps_unroll(int E) { return E >= 9 ? 1 : 16 / E; }     // E = 2: 8, 3: 5, 4: 4, 5: 3, 6..8: 2
__host__ __device__ constexpr int crps_chunk(int E) { return crps_unroll(E) * 1024; }    // elements per block

struct CrpsMembers { const float* u[CRPS_MAX_E]; const float* s[CRPS_MAX_E]; };
struct CrpsGrads { float* u[CRPS_MAX_E]; float* s[CRPS_MAX_E]; };

struct CrpsGeom {
  unsigned plane, W;                  // elements of one (sample, variable, level) plane (= a surface plane) = H * W
  int chunks;                         // blocks per plane
  int planes_u, planes_s;             // B * Vu * L, B * Vs
  int Vu, Vs, L;
  int t_rev;                          // the target's level axis is stored reversed
};

struct CrpsTile {
  bool surface;
  int var, stat;                      // variable (weight index), index of the plane's statistics
  unsigned begin, end;                // [begin, end) inside the plane
  long long base, base_t;             // the plane's offset in a member field / in the target
};

template <int E>
__device__ inline CrpsTile crps_locate(const CrpsGeom& g, int b) {
  CrpsTile w;
  const int nb_u = g.planes_u * g.chunks;
  w.surface = b >= nb_u;
  const int bb = w.surface ? b - nb_u : b;
  const int p = bb / g.chunks, c = bb - p * g.chunks;
  if (w.surface) {
    w.var = p % g.Vs;
    w.stat = w.var;
    w.base_t = (long long)p * g.plane;
  } else {
    const int lev = p % g.L;
    w.var = (p / g.L) % g.Vu;
    w.stat = w.var * g.L + lev;
    w.base_t = (long long)(p - lev + (g.t_rev ? g.L - 1 - lev : lev)) * g.plane;
  }
  w.base = (long long)p * g.plane;
  w.begin = (unsigned)c * crps_chunk(E);
  w.end = w.begin + crps_chunk(E) < g.plane ? w.begin + crps_chunk(E) : g.plane;
  return w;
}

template <int VW>
__device__ inline void crps_load(const float* p, float (&v)[VW]) {
  if constexpr (VW == 4) {
    const f32x4 q = *reinterpret_cast<const f32x4*>(p);
    v[0] = q[0]; v[1] = q[1]; v[2] = q[2]; v[3] = q[3];
  } else {
    v[0] = *p;
  }
}

template <int VW>
__device__ inline void crps_store(float* p, const float (&v)[VW]) {
  if constexpr (VW == 4) *reinterpret_cast<f32x4*>(p) = f32x4{v[0], v[1], v[2], v[3]};
  else *p = v[0];
}

__device__ inline float crps_sign(float a, float b) { return (a > b ? 1.f : 0.f) - (a < b ? 1.f : 0.f); }

// VW = 4: the 16-byte path (W % 4 == 0, every base 16-byte aligned), one batch of U vectors per thread; VW = 1: the scalar path,
// four batches of U elements per thread over the same chunk.
template <int E, int VW>
__global__ __launch_bounds__(256) void fair_crps_partial_kernel(const CrpsMembers m, const float* __restrict__ t,
                                                                const float* __restrict__ ts, const float* __restrict__ wu,
                                                                const float* __restrict__ ws, const float* __restrict__ lat,
                                                                float* __restrict__ partial, const CrpsGeom g, const TargetStats st) {
  constexpr int U = crps_unroll(E);
  const CrpsTile w = crps_locate<E>(g, blockIdx.x);
  const float* __restrict__ b = (w.surface ? ts : t) + w.base_t;
  const bool nrm = st.mean_u != nullptr;
  const float mn = nrm ? (w.surface ? st.mean_s[w.stat] : st.mean_u[w.stat]) : 0.f;
  const float sd = nrm ? (w.surface ? st.std_s[w.stat] : st.std_u[w.stat]) : 1.f;
  float acc[VW] = {};
  for (int pass = 0; pass < 4 / VW; ++pass) {
    float x[U][E][VW] = {}, y[U][VW] = {};
#pragma unroll
    for (int k = 0; k < U; ++k) {
      const unsigned i = w.begin + (unsigned)((pass * U + k) * 256 + (int)threadIdx.x) * VW;
      if (i < w.end) {
#pragma unroll
        for (int e = 0; e < E; ++e) crps_load<VW>((w.surface ? m.s[e] : m.u[e]) + w.base + i, x[k][e]);
        crps_load<VW>(b + i, y[k]);
      }
    }
#pragma unroll
    for (int k = 0; k < U; ++k) {
      const unsigned i = w.begin + (unsigned)((pass * U + k) * 256 + (int)threadIdx.x) * VW;
      if (i < w.end) {
        const float a = lat ? lat[i / g.W] : 1.f;
#pragma unroll
        for (int j = 0; j < VW; ++j) {
          const float tv = nrm ? (y[k][j] - mn) / sd : y[k][j];
          float s1 = 0.f, s2 = 0.f;
#pragma unroll
          for (int e = 0; e < E; ++e) s1 += fabsf(x[k][e][j] - tv);
#pragma unroll
          for (int e = 1; e < E; ++e)
#pragma unroll
            for (int f = 0; f < e; ++f) s2 += fabsf(x[k][e][j] - x[k][f][j]);
          // the double sum counts every pair twice: 1/(2E(E-1)) * 2
          acc[j] += a * (s1 * (1.f / E) - s2 * (1.f / (E * (E - 1))));
        }
      }
    }
  }
  float s = acc[0];
  if constexpr (VW == 4) s = (acc[0] + acc[1]) + (acc[2] + acc[3]);
#pragma unroll
  for (int off = 32; off >= 1; off >>= 1) s += __shfl_xor(s, off, 64);
  __shared__ float red[4];
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = s;
  __syncthreads();
  if (threadIdx.x == 0) partial[blockIdx.x] = ((red[0] + red[1]) + (red[2] + red[3])) * (w.surface ? ws[w.var] : wu[w.var]);
}

// loss[0] = total, loss[1] = upper mean, loss[2] = surface mean (the final launch of csrc/loss.hip, over this file's partials)
__global__ __launch_bounds__(256) void fair_crps_final_kernel(const float* __restrict__ partial, float* __restrict__ loss, int nb_u,
                                                              int nb_s, double n_u, double n_s) {
  double su = 0.0, ss = 0.0;
  for (int i = threadIdx.x; i < nb_u; i += 256) su += (double)partial[i];
  for (int i = threadIdx.x; i < nb_s; i += 256) ss += (double)partial[nb_u + i];
  __shared__ double ru[256], rs[256];
  ru[threadIdx.x] = su;
  rs[threadIdx.x] = ss;
  __syncthreads();
  for (int off = 128; off >= 1; off >>= 1) {
    if ((int)threadIdx.x < off) {
      ru[threadIdx.x] += ru[threadIdx.x + off];
      rs[threadIdx.x] += rs[threadIdx.x + off];
    }
    __syncthreads();
  }
  if (threadIdx.x == 0) {
    const float lu = (float)(ru[0] / n_u), ls = (float)(rs[0] / n_s);
    loss[1] = lu;
    loss[2] = ls;
    loss[0] = lu + ls * 0.25f;
  }
}

// d.u[e] / d.s[e] may BE m.u[e] / m.s[e] (the gradients written over the member fields): a thread loads all E values of every
// element of its batch before its first store, by hand -- behind a store the compiler would have to keep every later load of a
// field that may alias it.  Hence no __restrict__ on the member and gradient fields.
template <int E, int VW>
__global__ __launch_bounds__(256) void fair_crps_bwd_kernel(const CrpsMembers m, const float* __restrict__ t,
                                                            const float* __restrict__ ts, const float* __restrict__ wu,
                                                            const float* __restrict__ ws, const float* __restrict__ lat,
                                                            const float* __restrict__ grad, const CrpsGrads d, const CrpsGeom g,
                                                            const TargetStats st, float inv_nu, float inv_ns) {
  constexpr int U = crps_unroll(E);
  const CrpsTile w = crps_locate<E>(g, blockIdx.x);
  const float* __restrict__ b = (w.surface ? ts : t) + w.base_t;
  const bool nrm = st.mean_u != nullptr;
  const float mn = nrm ? (w.surface ? st.mean_s[w.stat] : st.mean_u[w.stat]) : 0.f;
  const float sd = nrm ? (w.surface ? st.std_s[w.stat] : st.std_u[w.stat]) : 1.f;
  // torch's autograd order, as in l1_loss_bwd_kernel: d(mean) = g * (1 / n) (the surface term's incoming gradient is g * 0.25),
  // times the variable weight; then the row's latitude weight
  const float gr = grad[0];
  const float c = (w.surface ? ((gr * 0.25f) * inv_ns) : (gr * inv_nu)) * (w.surface ? ws[w.var] : wu[w.var]);
  for (int pass = 0; pass < 4 / VW; ++pass) {
    float x[U][E][VW] = {}, y[U][VW] = {};
#pragma unroll
    for (int k = 0; k < U; ++k) {
      const unsigned i = w.begin + (unsigned)((pass * U + k) * 256 + (int)threadIdx.x) * VW;
      if (i < w.end) {
#pragma unroll
        for (int e = 0; e < E; ++e) crps_load<VW>((w.surface ? m.s[e] : m.u[e]) + w.base + i, x[k][e]);
        crps_load<VW>(b + i, y[k]);
      }
    }
#pragma unroll
    for (int k = 0; k < U; ++k) {
      const unsigned i = w.begin + (unsigned)((pass * U + k) * 256 + (int)threadIdx.x) * VW;
      if (i < w.end) {
        const float ca = lat ? c * lat[i / g.W] : c;
#pragma unroll
        for (int j = 0; j < VW; ++j) {
          const float tv = nrm ? (y[k][j] - mn) / sd : y[k][j];
          float n[E];                                   // n_e: small integers, exact
#pragma unroll
          for (int e = 0; e < E; ++e) n[e] = (float)(E - 1) * crps_sign(x[k][e][j], tv);
#pragma unroll
          for (int e = 1; e < E; ++e)
#pragma unroll
            for (int f = 0; f < e; ++f) {
              const float sg = crps_sign(x[k][e][j], x[k][f][j]);
              n[e] -= sg;
              n[f] += sg;
            }
#pragma unroll
          for (int e = 0; e < E; ++e) x[k][e][j] = ca * (n[e] * (1.f / (E * (E - 1))));      // n = 0: an exact zero
        }
#pragma unroll
        for (int e = 0; e < E; ++e) crps_store<VW>((w.surface ? d.s[e] : d.u[e]) + w.base + i, x[k][e]);
      }
    }
  }
}

bool make_crps_geom(CrpsGeom& g, int E, int B, int Vu, int levels, int Vs, int H, int W, int t_rev) {
  if (B <= 0 || Vu <= 0 || levels <= 0 || Vs <= 0 || H <= 0 || W <= 0) return false;
  const long long plane = (long long)H * W;
  if (plane > (1ll << 31) - 2 * crps_chunk(2)) return false;            // in-plane indices are 32-bit, a chunk's end included
  long long pu = (long long)B * Vu, ps = (long long)B * Vs;
  if (pu > (1 << 24) || ps > (1 << 24)) return false;
  pu *= levels;
  if (pu > (1 << 24)) return false;
  const long long chunks = (plane + crps_chunk(E) - 1) / crps_chunk(E);
  if ((pu + ps) * chunks >= (1ll << 30)) return false;
  g.plane = (unsigned)plane; g.W = (unsigned)W;
  g.chunks = (int)chunks;
  g.planes_u = (int)pu; g.planes_s = (int)ps;
  g.Vu = Vu; g.Vs = Vs; g.L = levels; g.t_rev = t_rev != 0;
  return true;
}

bool aligned16(const void* p) { return ((uintptr_t)p & 15) == 0; }

// E in 2..16 (checked by the callers): one instantiation per member count
#define CRPS_DISPATCH(E_, CALL)                                                                                              \
  switch (E_) {                                                                                                              \
    case 2: CALL(2); break;   case 3: CALL(3); break;   case 4: CALL(4); break;   case 5: CALL(5); break;                     \
    case 6: CALL(6); break;   case 7: CALL(7); break;   case 8: CALL(8); break;   case 9: CALL(9); break;                     \
    case 10: CALL(10); break; case 11: CALL(11); break; case 12: CALL(12); break; case 13: CALL(13); break;                   \
    case 14: CALL(14); break; case 15: CALL(15); break; case 16: CALL(16); break;                                             \
  }

}  // namespace

extern "C" long long pangu_fair_crps_loss_blocks(int E, int B, int Vu, int levels, int Vs, int H, int W) {
  if (E < 2 || E > CRPS_MAX_E) return PANGU_E_ARG;
  CrpsGeom g;
  if (!make_crps_geom(g, E, B, Vu, levels, Vs, H, W, 0)) return PANGU_E_SHAPE;
  return ((long long)g.planes_u + g.planes_s) * g.chunks;
}

extern "C" int pangu_fair_crps_loss_fwd(pangu_stream_t stream, const float* const* members, const float* const* members_surface, int E,
                                        const float* target, const float* target_surface, const float* w_upper,
                                        const float* w_surface, const float* lat_weight, float* partial, float* loss, int B, int Vu,
                                        int levels, int Vs, int H, int W, int target_levels_reversed, const float* t_mean_upper,
                                        const float* t_std_upper, const float* t_mean_surface, const float* t_std_surface) {
  if (!members || !members_surface || !target || !target_surface || !w_upper || !w_surface || !partial || !loss) return PANGU_E_NULL;
  if (E < 2 || E > CRPS_MAX_E) return PANGU_E_ARG;
  CrpsMembers m = {};
  bool vec = W % 4 == 0 && aligned16(target) && aligned16(target_surface);
  for (int e = 0; e < E; ++e) {
    if (!members[e] || !members_surface[e]) return PANGU_E_NULL;
    m.u[e] = members[e];
    m.s[e] = members_surface[e];
    vec = vec && aligned16(m.u[e]) && aligned16(m.s[e]);
  }
  CrpsGeom g;
  TargetStats st;
  if (!make_crps_geom(g, E, B, Vu, levels, Vs, H, W, target_levels_reversed)) return PANGU_E_SHAPE;
  if (!make_stats(st, t_mean_upper, t_std_upper, t_mean_surface, t_std_surface)) return PANGU_E_NULL;
  const int nb_u = g.planes_u * g.chunks, nb_s = g.planes_s * g.chunks;
  hipStream_t s = (hipStream_t)stream;
#define CRPS_FWD(N)                                                                                                            \
  if (vec) hipLaunchKernelGGL((fair_crps_partial_kernel<N, 4>), dim3(nb_u + nb_s), dim3(256), 0, s, m, target, target_surface, \
                              w_upper, w_surface, lat_weight, partial, g, st);                                                 \
  else hipLaunchKernelGGL((fair_crps_partial_kernel<N, 1>), dim3(nb_u + nb_s), dim3(256), 0, s, m, target, target_surface,     \
                          w_upper, w_surface, lat_weight, partial, g, st)
  CRPS_DISPATCH(E, CRPS_FWD)
#undef CRPS_FWD
  hipLaunchKernelGGL(fair_crps_final_kernel, dim3(1), dim3(256), 0, s, partial, loss, nb_u, nb_s,
                     (double)g.planes_u * (double)g.plane, (double)g.planes_s * (double)g.plane);
  return pangu_launch_status();
}

extern "C" int pangu_fair_crps_loss_bwd(pangu_stream_t stream, const float* const* members, const float* const* members_surface, int E,
                                        const float* target, const float* target_surface, const float* w_upper,
                                        const float* w_surface, const float* lat_weight, const float* grad, float* const* d_members,
                                        float* const* d_members_surface, int B, int Vu, int levels, int Vs, int H, int W,
                                        int target_levels_reversed, const float* t_mean_upper, const float* t_std_upper,
                                        const float* t_mean_surface, const float* t_std_surface) {
  if (!members || !members_surface || !target || !target_surface || !w_upper || !w_surface || !grad || !d_members || !d_members_surface)
    return PANGU_E_NULL;
  if (E < 2 || E > CRPS_MAX_E) return PANGU_E_ARG;
  CrpsMembers m = {};
  CrpsGrads d = {};
  bool vec = W % 4 == 0 && aligned16(target) && aligned16(target_surface);
  for (int e = 0; e < E; ++e) {
    if (!members[e] || !members_surface[e] || !d_members[e] || !d_members_surface[e]) return PANGU_E_NULL;
    m.u[e] = members[e];
    m.s[e] = members_surface[e];
    d.u[e] = d_members[e];
    d.s[e] = d_members_surface[e];
    vec = vec && aligned16(m.u[e]) && aligned16(m.s[e]) && aligned16(d.u[e]) && aligned16(d.s[e]);
  }
  CrpsGeom g;
  TargetStats st;
  if (!make_crps_geom(g, E, B, Vu, levels, Vs, H, W, target_levels_reversed)) return PANGU_E_SHAPE;
  if (!make_stats(st, t_mean_upper, t_std_upper, t_mean_surface, t_std_surface)) return PANGU_E_NULL;
  const int nb = (g.planes_u + g.planes_s) * g.chunks;
  const float inv_nu = 1.0f / (float)((double)g.planes_u * (double)g.plane), inv_ns = 1.0f / (float)((double)g.planes_s * (double)g.plane);
  hipStream_t s = (hipStream_t)stream;
#define CRPS_BWD(N)                                                                                                           \
  if (vec) hipLaunchKernelGGL((fair_crps_bwd_kernel<N, 4>), dim3(nb), dim3(256), 0, s, m, target, target_surface, w_upper,    \
                              w_surface, lat_weight, grad, d, g, st, inv_nu, inv_ns);                                         \
  else hipLaunchKernelGGL((fair_crps_bwd_kernel<N, 1>), dim3(nb), dim3(256), 0, s, m, target, target_surface, w_upper,        \
                          w_surface, lat_weight, grad, d, g, st, inv_nu, inv_ns)
  CRPS_DISPATCH(E, CRPS_BWD)
#undef CRPS_BWD
  return pangu_launch_status();
}
