// Output side of the forecast loop: pack each (variable, level) plane of a field to int16 with a per-plane scale / offset -- the
// storage format of ERA5 NetCDF (`scale_factor` / `add_offset`; the reference's NetCDFDataset reads it) -- so that one lead time
// crosses the link as 143 MB instead of 286 MB and lands in page-locked memory as arrays a NetCDF writer stores as they are.
// De-normalisation (`normBackData`, reference era5_data/utils_data.py:324-330: v = x * std + mean, two roundings) and the reader's
// level reversal (utils_data.py:117) are folded into the addressing, as normData and the flip are on the input side.
//
//   launch 1 (reduce):    one workgroup per (plane, slab of PK_SLAB values): min, max over the FINITE values v and the count of the
//                         non-finite ones -> 16 bytes of workspace per workgroup.  No atomics, nothing needs zeroing.
//   launch 2 (quantise):  the same grid; every workgroup first folds its plane's partials (a few dozen, in one fixed order), derives
//                         offset = (max + min) / 2, scale = (max - min) / 65534 (1 when that is 0) and stores
//                         q = clamp(rint((v - offset) * (1 / scale)), -32767, 32767), non-finite v -> -32768.
//
// Data movement: a lane loads 8 consecutive values (two 16-B loads) and stores them as one 16-B int16 vector.  A plane whose first
// packed value is not 16-B aligned starts with a scalar head of up to 7 values; what is left after the last whole group of 8 is a
// scalar tail; a source that is not 16-B aligned at the first group is read with scalar loads.  The field (286 MB) exceeds the
// 256 MB Infinity Cache, so both launches read it from HBM: floor = 2 x 286.6 MB read + 143.3 MB written.
#include <cmath>
#include <cstring>
#include <thread>
#include <vector>

#include "common.h"
#include "plane_value.h"      // pk_value, pk_src_plane

namespace {

constexpr int PK_THREADS = 256;
constexpr int PK_SLAB = 16384;                 // values per workgroup: 8 groups of 8 per lane, 64 KB of source
constexpr int PK_GROUPS = PK_SLAB / 8;         // 16-B int16 vectors per slab
constexpr int PK_PART = 4;                     // floats per partial: min, max, non-finite count (as bits), pad
constexpr int PK_UNROLL = 4;                   // groups of 8 per lane in flight: 8 x 16 B = 128 B per lane, 32 KB per workgroup
constexpr float PK_QMAX = 32767.0f;
constexpr int PK_FILL = -32768;

typedef short i16x8 __attribute__((ext_vector_type(8)));

__device__ __forceinline__ bool pk_finite(float v) { return (__float_as_uint(v) & 0x7f800000u) != 0x7f800000u; }

// Where the 16-B groups of one plane lie.  `head` values come before the first group, `groups` whole groups of VEC follow, the rest
// is the tail; `vec_src`: the source is 16-B aligned at the first group.
struct PlaneSplit {
  long long head, groups, tail_at;
  bool vec_src;
};
template <int VEC, int OUT_BYTES>
__device__ __forceinline__ PlaneSplit pk_split(const float* sp, const void* op, long long E) {
  PlaneSplit s;
  const long long mis = (long long)((16 - ((size_t)op & 15)) & 15) / OUT_BYTES;      // output elements up to the next 16-B boundary
  s.head = mis < E ? mis : E;
  s.groups = (E - s.head) / VEC;
  s.tail_at = s.head + s.groups * VEC;
  s.vec_src = (((size_t)(sp + s.head)) & 15) == 0;
  return s;
}

struct MinMaxCount {
  float mn, mx;
  unsigned bad;
};
__device__ __forceinline__ void pk_acc(MinMaxCount& r, float v) {
  if (pk_finite(v)) {
    r.mn = fminf(r.mn, v);
    r.mx = fmaxf(r.mx, v);
  } else {
    r.bad += 1u;
  }
}
// workgroup-wide fold, result valid in every thread; `sm` is 3 * (PK_THREADS / 64) words of LDS
__device__ __forceinline__ MinMaxCount pk_block_fold(MinMaxCount r, unsigned* sm) {
#pragma unroll
  for (int o = 32; o >= 1; o >>= 1) {
    r.mn = fminf(r.mn, __shfl_xor(r.mn, o, 64));
    r.mx = fmaxf(r.mx, __shfl_xor(r.mx, o, 64));
    r.bad += __shfl_xor(r.bad, o, 64);
  }
  constexpr int NW = PK_THREADS / 64;
  const int w = threadIdx.x >> 6;
  __syncthreads();                                     // (sm may still be read from an earlier fold)
  if ((threadIdx.x & 63) == 0) {
    sm[w] = __float_as_uint(r.mn);
    sm[NW + w] = __float_as_uint(r.mx);
    sm[2 * NW + w] = r.bad;
  }
  __syncthreads();
  MinMaxCount t{__uint_as_float(sm[0]), __uint_as_float(sm[NW]), sm[2 * NW]};
#pragma unroll
  for (int i = 1; i < NW; ++i) {
    t.mn = fminf(t.mn, __uint_as_float(sm[i]));
    t.mx = fmaxf(t.mx, __uint_as_float(sm[NW + i]));
    t.bad += sm[2 * NW + i];
  }
  return t;
}

// the 8 values of one group: two 16-B loads, or eight scalar ones for a misaligned source
template <bool VEC>
__device__ __forceinline__ void pk_load8(const float* gp, f32x4& a, f32x4& b) {
  if (VEC) {
    a = *(const f32x4*)gp;
    b = *(const f32x4*)(gp + 4);
  } else {
    a = f32x4{gp[0], gp[1], gp[2], gp[3]};
    b = f32x4{gp[4], gp[5], gp[6], gp[7]};
  }
}

// This lane's groups of [g0, g1): PK_UNROLL groups loaded unconditionally before the first is used (no branch between the loads, so
// all of them are in flight together), then the ragged rest one at a time.  fn(group index, first four values, last four values).
template <bool VEC, class F>
__device__ __forceinline__ void pk_for_groups8(const float* body, long long g0, long long g1, F fn) {
  long long g = g0 + threadIdx.x;
  for (; g + (long long)(PK_UNROLL - 1) * PK_THREADS < g1; g += PK_THREADS * PK_UNROLL) {
    f32x4 x[PK_UNROLL][2];
#pragma unroll
    for (int u = 0; u < PK_UNROLL; ++u) pk_load8<VEC>(body + (g + (long long)u * PK_THREADS) * 8, x[u][0], x[u][1]);
#pragma unroll
    for (int u = 0; u < PK_UNROLL; ++u) fn(g + (long long)u * PK_THREADS, x[u][0], x[u][1]);
  }
  for (; g < g1; g += PK_THREADS) {
    f32x4 a, b;
    pk_load8<VEC>(body + g * 8, a, b);
    fn(g, a, b);
  }
}

template <bool AFFINE>
__global__ __launch_bounds__(PK_THREADS) void pack_reduce_kernel(const float* __restrict__ src, const float* __restrict__ mul,
                                                                 const float* __restrict__ add, const short* packed,
                                                                 float* __restrict__ partial, long long E, int slabs, int levels) {
  __shared__ unsigned sm[3 * (PK_THREADS / 64)];
  const int p = blockIdx.x / slabs, slab = blockIdx.x - p * slabs;
  const int q = pk_src_plane(p, levels);
  const float* sp = src + (size_t)q * E;
  const PlaneSplit s = pk_split<8, 2>(sp, packed + (size_t)p * E, E);
  const float m = AFFINE ? mul[q] : 1.0f, a = AFFINE ? add[q] : 0.0f;
  MinMaxCount r{INFINITY, -INFINITY, 0u};
  const long long g0 = (long long)slab * PK_GROUPS;
  const long long g1 = g0 + PK_GROUPS < s.groups ? g0 + PK_GROUPS : s.groups;
  auto fold = [&](long long, const f32x4& x0, const f32x4& x1) {
#pragma unroll
    for (int j = 0; j < 4; ++j) pk_acc(r, pk_value<AFFINE>(x0[j], m, a));
#pragma unroll
    for (int j = 0; j < 4; ++j) pk_acc(r, pk_value<AFFINE>(x1[j], m, a));
  };
  if (s.vec_src)
    pk_for_groups8<true>(sp + s.head, g0, g1, fold);
  else
    pk_for_groups8<false>(sp + s.head, g0, g1, fold);
  if (slab == 0) {        // head and tail of the plane: at most 7 values each
    if ((long long)threadIdx.x < s.head) pk_acc(r, pk_value<AFFINE>(sp[threadIdx.x], m, a));
    const long long t = s.tail_at + threadIdx.x - 64;
    if (threadIdx.x >= 64 && t < E) pk_acc(r, pk_value<AFFINE>(sp[t], m, a));
  }
  r = pk_block_fold(r, sm);
  if (threadIdx.x == 0) {
    float* o = partial + (size_t)blockIdx.x * PK_PART;
    o[0] = r.mn;
    o[1] = r.mx;
    o[2] = __uint_as_float(r.bad);
    o[3] = 0.0f;
  }
}

__device__ __forceinline__ short pk_quant(float v, float offset, float inv) {
  const float t = fminf(fmaxf(rintf((v - offset) * inv), -PK_QMAX), PK_QMAX);
  return (short)(pk_finite(v) ? (int)t : PK_FILL);
}

template <bool AFFINE>
__global__ __launch_bounds__(PK_THREADS) void pack_quant_kernel(const float* __restrict__ src, const float* __restrict__ mul,
                                                                const float* __restrict__ add, short* __restrict__ packed,
                                                                float* __restrict__ scale_offset, int* __restrict__ nonfinite,
                                                                const float* __restrict__ partial, long long E, int slabs,
                                                                int levels) {
  __shared__ unsigned sm[3 * (PK_THREADS / 64)];
  const int p = blockIdx.x / slabs, slab = blockIdx.x - p * slabs;
  const int q = pk_src_plane(p, levels);
  // the plane's partials, thread t taking t, t + 256, ...: the same order in every workgroup of the plane
  MinMaxCount r{INFINITY, -INFINITY, 0u};
  const float* pp = partial + (size_t)p * slabs * PK_PART;
  for (int i = threadIdx.x; i < slabs; i += PK_THREADS) {
    const float* v = pp + (size_t)i * PK_PART;
    r.mn = fminf(r.mn, v[0]);
    r.mx = fmaxf(r.mx, v[1]);
    r.bad += __float_as_uint(v[2]);
  }
  r = pk_block_fold(r, sm);
  float offset = 0.0f, scale = 1.0f;
  if (r.mn <= r.mx) {                                   // at least one finite value
    offset = (r.mx + r.mn) * 0.5f;
    scale = (r.mx - r.mn) / 65534.0f;
    if (!(scale > 0.0f)) scale = 1.0f;                  // constant plane, or a range that underflows: packs to zeros
  }
  const float inv = 1.0f / scale;
  if (slab == 0 && threadIdx.x == 0) {
    scale_offset[2 * (size_t)p] = scale;
    scale_offset[2 * (size_t)p + 1] = offset;
    nonfinite[p] = (int)r.bad;
  }
  const float* sp = src + (size_t)q * E;
  short* op = packed + (size_t)p * E;
  const PlaneSplit s = pk_split<8, 2>(sp, op, E);
  const float m = AFFINE ? mul[q] : 1.0f, a = AFFINE ? add[q] : 0.0f;
  const long long g0 = (long long)slab * PK_GROUPS;
  const long long g1 = g0 + PK_GROUPS < s.groups ? g0 + PK_GROUPS : s.groups;
  short* obody = op + s.head;
  auto quant = [&](long long g, const f32x4& x0, const f32x4& x1) {
    i16x8 o;
#pragma unroll
    for (int j = 0; j < 4; ++j) o[j] = pk_quant(pk_value<AFFINE>(x0[j], m, a), offset, inv);
#pragma unroll
    for (int j = 0; j < 4; ++j) o[4 + j] = pk_quant(pk_value<AFFINE>(x1[j], m, a), offset, inv);
    __builtin_nontemporal_store(o, (i16x8*)(obody + g * 8));
  };
  if (s.vec_src)
    pk_for_groups8<true>(sp + s.head, g0, g1, quant);
  else
    pk_for_groups8<false>(sp + s.head, g0, g1, quant);
  if (slab == 0) {
    if ((long long)threadIdx.x < s.head) op[threadIdx.x] = pk_quant(pk_value<AFFINE>(sp[threadIdx.x], m, a), offset, inv);
    const long long t = s.tail_at + threadIdx.x - 64;
    if (threadIdx.x >= 64 && t < E) op[t] = pk_quant(pk_value<AFFINE>(sp[t], m, a), offset, inv);
  }
}

// fp32 staging copy with the same addressing and the same v = x * mul + add: groups of 4 values, one 16-B load and store each when
// source and destination plane are misaligned by the same amount, scalar otherwise
template <bool AFFINE>
__global__ __launch_bounds__(PK_THREADS) void stage_planes_kernel(const float* __restrict__ src, const float* __restrict__ mul,
                                                                  const float* __restrict__ add, float* __restrict__ dst,
                                                                  long long E, int slabs, int levels) {
  const int p = blockIdx.x / slabs, slab = blockIdx.x - p * slabs;
  const int q = pk_src_plane(p, levels);
  const float* sp = src + (size_t)q * E;
  float* op = dst + (size_t)p * E;
  const float m = AFFINE ? mul[q] : 1.0f, a = AFFINE ? add[q] : 0.0f;
  const PlaneSplit s = pk_split<4, 4>(sp, op, E);
  if (!s.vec_src) {       // (wave-uniform) no common 16-B phase: scalar over the slab
    const long long e0 = (long long)slab * PK_SLAB, e1 = e0 + PK_SLAB < E ? e0 + PK_SLAB : E;
    for (long long e = e0 + threadIdx.x; e < e1; e += PK_THREADS) op[e] = pk_value<AFFINE>(sp[e], m, a);
    return;
  }
  constexpr int G4 = PK_SLAB / 4;
  const long long g0 = (long long)slab * G4;
  const long long g1 = g0 + G4 < s.groups ? g0 + G4 : s.groups;
  const f32x4* body = (const f32x4*)(sp + s.head);
  f32x4* obody = (f32x4*)(op + s.head);
  auto put = [&](long long g, const f32x4& x) {
    f32x4 o;
#pragma unroll
    for (int j = 0; j < 4; ++j) o[j] = pk_value<AFFINE>(x[j], m, a);
    __builtin_nontemporal_store(o, obody + g);
  };
  long long g = g0 + threadIdx.x;
  for (; g + (long long)(PK_UNROLL - 1) * PK_THREADS < g1; g += PK_THREADS * PK_UNROLL) {
    f32x4 x[PK_UNROLL];
#pragma unroll
    for (int u = 0; u < PK_UNROLL; ++u) x[u] = body[g + (long long)u * PK_THREADS];
#pragma unroll
    for (int u = 0; u < PK_UNROLL; ++u) put(g + (long long)u * PK_THREADS, x[u]);
  }
  for (; g < g1; g += PK_THREADS) put(g, body[g]);
  if (slab == 0) {
    if ((long long)threadIdx.x < s.head) op[threadIdx.x] = pk_value<AFFINE>(sp[threadIdx.x], m, a);
    const long long t = s.tail_at + threadIdx.x - 64;
    if (threadIdx.x >= 64 && t < E) op[t] = pk_value<AFFINE>(sp[t], m, a);
  }
}

// slabs per plane, or -1: sizes out of range (a plane's non-finite count is an int; the grid is one dimension)
long long pk_slabs(int planes, long long plane_elems) {
  if (planes <= 0 || plane_elems <= 0 || plane_elems > 0x7fffffffll) return -1;
  const long long slabs = (plane_elems + PK_SLAB - 1) / PK_SLAB;
  if (slabs * planes > 0x7fffffffll) return -1;
  return slabs;
}

}  // namespace

extern "C" long long pangu_pack_i16_ws_bytes(int planes, long long plane_elems) {
  const long long slabs = pk_slabs(planes, plane_elems);
  if (slabs < 0) return PANGU_E_SHAPE;
  return slabs * planes * PK_PART * (long long)sizeof(float);
}

extern "C" int pangu_pack_planes_i16(pangu_stream_t stream, const float* src, const float* mul, const float* add, short* packed,
                                     float* scale_offset, int* nonfinite, void* workspace, long long workspace_bytes, int planes,
                                     long long plane_elems, int levels) {
  if (!src || !packed || !scale_offset || !nonfinite || !workspace) return PANGU_E_NULL;
  if ((mul == nullptr) != (add == nullptr)) return PANGU_E_NULL;
  const long long slabs = pk_slabs(planes, plane_elems);
  if (slabs < 0 || levels < 0 || (levels > 0 && planes % levels != 0)) return PANGU_E_SHAPE;
  if (((size_t)src & 3) || ((size_t)packed & 1) || ((size_t)workspace & 3)) return PANGU_E_ARG;
  if (workspace_bytes < pangu_pack_i16_ws_bytes(planes, plane_elems)) return PANGU_E_ARG;
  const dim3 grid((unsigned)(slabs * planes)), block(PK_THREADS);
  hipStream_t st = (hipStream_t)stream;
  float* partial = (float*)workspace;
  if (mul) {
    hipLaunchKernelGGL(pack_reduce_kernel<true>, grid, block, 0, st, src, mul, add, packed, partial, plane_elems, (int)slabs, levels);
    hipLaunchKernelGGL(pack_quant_kernel<true>, grid, block, 0, st, src, mul, add, packed, scale_offset, nonfinite, partial,
                       plane_elems, (int)slabs, levels);
  } else {
    hipLaunchKernelGGL(pack_reduce_kernel<false>, grid, block, 0, st, src, mul, add, packed, partial, plane_elems, (int)slabs, levels);
    hipLaunchKernelGGL(pack_quant_kernel<false>, grid, block, 0, st, src, mul, add, packed, scale_offset, nonfinite, partial,
                       plane_elems, (int)slabs, levels);
  }
  return pangu_launch_status();
}

extern "C" int pangu_stage_planes_f32(pangu_stream_t stream, const float* src, const float* mul, const float* add, float* dst,
                                      int planes, long long plane_elems, int levels) {
  if (!src || !dst) return PANGU_E_NULL;
  if ((mul == nullptr) != (add == nullptr)) return PANGU_E_NULL;
  const long long slabs = pk_slabs(planes, plane_elems);
  if (slabs < 0 || levels < 0 || (levels > 0 && planes % levels != 0)) return PANGU_E_SHAPE;
  if (((size_t)src & 3) || ((size_t)dst & 3)) return PANGU_E_ARG;
  const dim3 grid((unsigned)(slabs * planes)), block(PK_THREADS);
  if (mul)
    hipLaunchKernelGGL(stage_planes_kernel<true>, grid, block, 0, (hipStream_t)stream, src, mul, add, dst, plane_elems, (int)slabs,
                       levels);
  else
    hipLaunchKernelGGL(stage_planes_kernel<false>, grid, block, 0, (hipStream_t)stream, src, mul, add, dst, plane_elems, (int)slabs,
                       levels);
  return pangu_launch_status();
}

// Pure host code (next to pangu_host_copy): dst = q * scale + offset in fp32, two roundings; the fill value -> NaN.  The planes *
// plane_elems values are split into contiguous spans, one per thread (below 1 M values a thread costs more than it converts).
#pragma clang fp contract(off)
extern "C" int pangu_unpack_i16_host(float* dst, const short* src, const float* scale_offset, int planes, long long plane_elems,
                                     int threads) {
  if (planes <= 0 || plane_elems <= 0) return PANGU_E_SHAPE;
  if (!dst || !src || !scale_offset) return PANGU_E_NULL;
  const long long total = (long long)planes * plane_elems;
  constexpr long long kMinPerThread = 1ll << 20;
  long long n = threads < 1 ? 1 : threads;
  if (n > 64) n = 64;
  if (n > total / kMinPerThread) n = total / kMinPerThread;
  if (n < 1) n = 1;
  const long long span = ((total + n - 1) / n + 1023) & ~1023ll;
  auto piece = [=](long long i) {
    const long long b = i * span, e = b + span < total ? b + span : total;
    long long k = b;
    while (k < e) {
      const long long p = k / plane_elems, pe = (p + 1) * plane_elems < e ? (p + 1) * plane_elems : e;
      const float scale = scale_offset[2 * p], offset = scale_offset[2 * p + 1];
      for (; k < pe; ++k) {
        const float v = (float)src[k] * scale;
        dst[k] = src[k] == (short)PK_FILL ? NAN : v + offset;
      }
    }
  };
  if (n == 1) {
    piece(0);
    return PANGU_OK;
  }
  std::vector<std::thread> pool;
  pool.reserve((size_t)n - 1);
  for (long long i = 1; i < n; ++i) pool.emplace_back(piece, i);
  piece(0);
  for (auto& t : pool) t.join();
  return PANGU_OK;
}
