// Statistics ACROSS the leads of a rollout, kept on the device: one launch folds ONE lead's field into the accumulators of ONE lead
// window -- the running sum (the window mean), the minimum and maximum with the leads at which they occur, and per threshold the
// number of exceeding leads, the current run of consecutive exceeding leads and the longest such run (spell length).  The
// de-normalisation v = x * mul + add and the level reversal are folded into the pass, as in pack.hip and regrid.hip, so the step's
// field is read once, where the forward's last kernel left it.
//
// Definitions, per element, v this lead's value (pk_value: two roundings), `lead` in 0..254, thr[t][p] the threshold of output plane p:
//   first != 0 (the window's first lead): every output is ASSIGNED and never read -- nothing has to be zeroed beforehand:
//       sum = v;  vmin = vmax = v;  when_min = when_max = lead;  e_t = (v > thr[t][p]);  count_t = run_t = longest_t = e_t
//   first == 0:
//       sum = sum + v                                       one fp32 add: over a window the left-to-right fp32 sum in lead order
//                                                           (the assignment at the first lead keeps a -0.0)
//       if (v < vmin || v != v) { vmin = v; when_min = lead; }        and the same with > for vmax / when_max
//       e_t = (v > thr[t][p]);  count_t += e_t;  run_t = e_t ? run_t + 1 : 0;  longest_t = max(longest_t, run_t)
//   A NaN takes both extremes at its first occurrence, and no number takes them back (a later NaN takes them again, with its lead);
//   a tie keeps the earlier lead, -0.0 and +0.0 tie; +-inf behave as numbers; e_t is false for NaN and for thr = +inf.  A window
//   holds at most 255 leads, so no byte counter wraps.
// Every output pointer may be NULL (that statistic is not kept).  No atomics, no workspace, every element is owned by one lane:
// bit-identical from run to run, and a plane's results do not depend on the other planes of the launch.
//
// Data movement: a lane takes LS_VEC = 4 consecutive elements at a time -- one 16-B access per fp32 field and one 4-B word per byte
// field -- and LS_UNROLL = 2 such groups, LS_THREADS * LS_VEC elements apart, whose loads are all issued before the first value is
// used.  A workgroup of 256 lanes owns a slab of 2048 consecutive elements of one plane; grid = planes * ceil(plane_elems / 2048).
// A plane is taken in groups when every array of the launch has the same phase there, i.e. after `head` (0..3) scalar elements all
// fp32 plane bases are 16-B aligned and all byte plane bases 4-B aligned; at most 3 elements are then left as a scalar tail.  A plane
// whose arrays disagree in phase is taken one element per lane (4-B and 1-B accesses).  Both choices depend on the plane alone, so
// they are uniform over the workgroup; no lane reads or writes a byte outside its own elements.
#include "common.h"
#include "plane_value.h"

namespace {

constexpr int LS_THREADS = 256;
constexpr int LS_VEC = 4;                      // elements per lane and group: 16 B of fp32, one word of bytes
constexpr int LS_UNROLL = 2;                   // groups per lane in flight
constexpr int LS_MAX_T = 4;
constexpr int LS_GROUPS = LS_THREADS * LS_UNROLL;          // groups per slab
constexpr long long LS_SLAB = (long long)LS_GROUPS * LS_VEC;

struct LeadStatsArgs {
  const float* src;
  const float* mul;
  const float* add;
  float* sum;
  float* vmin;
  float* vmax;
  unsigned char* when_min;
  unsigned char* when_max;
  const float* thr;
  unsigned char* count;
  unsigned char* run;
  unsigned char* longest;
  long long E;
  int planes, levels, T, lead, slabs;
};

// N consecutive values / bytes at p: one 16-B or 4-B access (N = 4; the caller guarantees the alignment) or one element (N = 1).
// Bytes travel as the low N bytes of a word, element j in bits 8j..8j+7.
template <int N>
__device__ __forceinline__ void ls_load(const float* p, float (&x)[N]) {
  if constexpr (N == 4) {
    const f32x4 t = *(const f32x4*)p;
#pragma unroll
    for (int j = 0; j < N; ++j) x[j] = t[j];
  } else {
    x[0] = *p;
  }
}
template <int N>
__device__ __forceinline__ void ls_store(float* p, const float (&x)[N]) {
  if constexpr (N == 4)
    *(f32x4*)p = f32x4{x[0], x[1], x[2], x[3]};
  else
    *p = x[0];
}
template <int N>
__device__ __forceinline__ unsigned ls_load_bytes(const unsigned char* p) {
  if constexpr (N == 4)
    return *(const unsigned*)p;
  else
    return (unsigned)*p;
}
template <int N>
__device__ __forceinline__ void ls_store_bytes(unsigned char* p, unsigned w) {
  if constexpr (N == 4)
    *(unsigned*)p = w;
  else
    *p = (unsigned char)w;
}

// U chunks of N elements, the u-th at plane offset i + u * stride: every load is issued before the first value is used.  sp: the
// SOURCE plane; `op` offsets an output plane's arrays, `bp` (+ t * tstride) the byte fields of threshold t.
template <int N, int U, bool AFFINE, bool FIRST>
__device__ __forceinline__ void ls_elems(const LeadStatsArgs& a, const float* sp, long long op, long long tstride, float m, float ad,
                                         const float (&thr)[LS_MAX_T], long long i, long long stride) {
  float x[U][N], s[U][N], mn[U][N], mx[U][N];
  unsigned wmn[U], wmx[U], cnt[U][LS_MAX_T], run[U][LS_MAX_T], lng[U][LS_MAX_T];
  const bool keep_run = a.run != nullptr;
#pragma unroll
  for (int u = 0; u < U; ++u) {
    const long long e = i + u * stride;
    ls_load<N>(sp + e, x[u]);
    wmn[u] = wmx[u] = 0u;
#pragma unroll
    for (int j = 0; j < N; ++j) s[u][j] = mn[u][j] = mx[u][j] = 0.0f;
#pragma unroll
    for (int t = 0; t < LS_MAX_T; ++t) cnt[u][t] = run[u][t] = lng[u][t] = 0u;
    if (!FIRST) {
      if (a.sum) ls_load<N>(a.sum + op + e, s[u]);
      if (a.vmin) ls_load<N>(a.vmin + op + e, mn[u]);
      if (a.vmax) ls_load<N>(a.vmax + op + e, mx[u]);
      if (a.when_min) wmn[u] = ls_load_bytes<N>(a.when_min + op + e);
      if (a.when_max) wmx[u] = ls_load_bytes<N>(a.when_max + op + e);
#pragma unroll
      for (int t = 0; t < LS_MAX_T; ++t) {
        if (t < a.T) {
          const long long b = op + t * tstride + e;
          if (a.count) cnt[u][t] = ls_load_bytes<N>(a.count + b);
          if (keep_run) run[u][t] = ls_load_bytes<N>(a.run + b);
          if (a.longest) lng[u][t] = ls_load_bytes<N>(a.longest + b);
        }
      }
    }
  }
  const unsigned lead = (unsigned)a.lead;
#pragma unroll
  for (int u = 0; u < U; ++u) {
    unsigned nmn = 0u, nmx = 0u, ncnt[LS_MAX_T] = {0u, 0u, 0u, 0u}, nrun[LS_MAX_T] = {0u, 0u, 0u, 0u},
             nlng[LS_MAX_T] = {0u, 0u, 0u, 0u};
#pragma unroll
    for (int j = 0; j < N; ++j) {
      const float v = pk_value<AFFINE>(x[u][j], m, ad);
      if (FIRST) {
        s[u][j] = mn[u][j] = mx[u][j] = v;
        nmn |= lead << (8 * j);
        nmx |= lead << (8 * j);
      } else {
        s[u][j] = s[u][j] + v;
        const bool lo = (v < mn[u][j]) || (v != v), hi = (v > mx[u][j]) || (v != v);
        mn[u][j] = lo ? v : mn[u][j];
        mx[u][j] = hi ? v : mx[u][j];
        nmn |= (lo ? lead : ((wmn[u] >> (8 * j)) & 0xffu)) << (8 * j);
        nmx |= (hi ? lead : ((wmx[u] >> (8 * j)) & 0xffu)) << (8 * j);
      }
#pragma unroll
      for (int t = 0; t < LS_MAX_T; ++t) {
        if (t < a.T) {
          const unsigned ev = v > thr[t] ? 1u : 0u;
          unsigned c = ev, r = ev, l = ev;
          if (!FIRST) {
            c = ((cnt[u][t] >> (8 * j)) & 0xffu) + ev;
            r = ev ? ((run[u][t] >> (8 * j)) & 0xffu) + 1u : 0u;
            l = (lng[u][t] >> (8 * j)) & 0xffu;
            l = l > r ? l : r;
          }
          ncnt[t] |= c << (8 * j);
          nrun[t] |= r << (8 * j);
          nlng[t] |= l << (8 * j);
        }
      }
    }
    const long long e = i + u * stride;
    if (a.sum) ls_store<N>(a.sum + op + e, s[u]);
    if (a.vmin) ls_store<N>(a.vmin + op + e, mn[u]);
    if (a.vmax) ls_store<N>(a.vmax + op + e, mx[u]);
    if (a.when_min) ls_store_bytes<N>(a.when_min + op + e, nmn);
    if (a.when_max) ls_store_bytes<N>(a.when_max + op + e, nmx);
#pragma unroll
    for (int t = 0; t < LS_MAX_T; ++t) {
      if (t < a.T) {
        const long long b = op + t * tstride + e;
        if (a.count) ls_store_bytes<N>(a.count + b, ncnt[t]);
        if (keep_run) ls_store_bytes<N>(a.run + b, nrun[t]);
        if (a.longest) ls_store_bytes<N>(a.longest + b, nlng[t]);
      }
    }
  }
}

// elements before the next 16-B (fp32) / 4-B (byte) boundary, 0..3
__device__ __forceinline__ unsigned ls_phase(const float* p) { return (unsigned)(((size_t)p >> 2) & 3); }
__device__ __forceinline__ unsigned ls_phase(const unsigned char* p) { return (unsigned)((size_t)p & 3); }

template <bool AFFINE, bool FIRST>
__global__ __launch_bounds__(LS_THREADS) void lead_stats_kernel(LeadStatsArgs a) {
  const int p = blockIdx.x / a.slabs, slab = blockIdx.x - p * a.slabs;
  const int q = pk_src_plane(p, a.levels);
  const long long E = a.E, op = (long long)p * E, tstride = (long long)a.planes * E;
  const float* sp = a.src + (long long)q * E;
  const float m = AFFINE ? a.mul[q] : 1.0f, ad = AFFINE ? a.add[q] : 0.0f;
  float thr[LS_MAX_T];
#pragma unroll
  for (int t = 0; t < LS_MAX_T; ++t) thr[t] = t < a.T ? a.thr[(long long)t * a.planes + p] : INFINITY;
  // the plane goes in groups of LS_VEC when every array of the launch has the source's phase at this plane
  const unsigned ph = ls_phase(sp);
  bool same = true;
  if (a.sum) same = same && ls_phase(a.sum + op) == ph;
  if (a.vmin) same = same && ls_phase(a.vmin + op) == ph;
  if (a.vmax) same = same && ls_phase(a.vmax + op) == ph;
  if (a.when_min) same = same && ls_phase(a.when_min + op) == ph;
  if (a.when_max) same = same && ls_phase(a.when_max + op) == ph;
#pragma unroll
  for (int t = 0; t < LS_MAX_T; ++t) {
    if (t < a.T) {
      const long long b = op + t * tstride;
      if (a.count) same = same && ls_phase(a.count + b) == ph;
      if (a.run) same = same && ls_phase(a.run + b) == ph;
      if (a.longest) same = same && ls_phase(a.longest + b) == ph;
    }
  }
  if (same) {
    const long long mis = (LS_VEC - ph) & 3;
    const long long head = mis < E ? mis : E;
    const long long groups = (E - head) / LS_VEC, tail_at = head + groups * LS_VEC;
    const long long g0 = (long long)slab * LS_GROUPS, g1 = g0 + LS_GROUPS < groups ? g0 + LS_GROUPS : groups;
    long long g = g0 + threadIdx.x;
    for (; g + (long long)(LS_UNROLL - 1) * LS_THREADS < g1; g += (long long)LS_THREADS * LS_UNROLL)
      ls_elems<LS_VEC, LS_UNROLL, AFFINE, FIRST>(a, sp, op, tstride, m, ad, thr, head + g * LS_VEC, (long long)LS_THREADS * LS_VEC);
    for (; g < g1; g += LS_THREADS) ls_elems<LS_VEC, 1, AFFINE, FIRST>(a, sp, op, tstride, m, ad, thr, head + g * LS_VEC, 0);
    // the head and tail elements of the plane (at most 6): one lane each, in the plane's first workgroup
    const long long ends = head + (E - tail_at);
    if (slab == 0 && (long long)threadIdx.x < ends) {
      const long long i = (long long)threadIdx.x < head ? (long long)threadIdx.x : tail_at + ((long long)threadIdx.x - head);
      ls_elems<1, 1, AFFINE, FIRST>(a, sp, op, tstride, m, ad, thr, i, 0);
    }
  } else {
    const long long i0 = (long long)slab * LS_SLAB, i1 = i0 + LS_SLAB < E ? i0 + LS_SLAB : E;
    for (long long i = i0 + threadIdx.x; i < i1; i += LS_THREADS) ls_elems<1, 1, AFFINE, FIRST>(a, sp, op, tstride, m, ad, thr, i, 0);
  }
}

}  // namespace

extern "C" int pangu_lead_stats_update_f32(pangu_stream_t stream, const float* src, const float* mul, const float* add, float* sum,
                                           float* vmin, float* vmax, unsigned char* when_min, unsigned char* when_max,
                                           const float* thr, int T, unsigned char* count, unsigned char* run, unsigned char* longest,
                                           int planes, long long plane_elems, int levels, int lead, int first) {
  if (!src) return PANGU_E_NULL;
  if ((mul == nullptr) != (add == nullptr)) return PANGU_E_NULL;
  if (T > 0 && !thr) return PANGU_E_NULL;
  if (planes <= 0 || plane_elems <= 0) return PANGU_E_SHAPE;
  if (plane_elems > 0x7fffffffll) return PANGU_E_SHAPE;
  if (levels < 0 || (levels > 0 && planes % levels != 0)) return PANGU_E_SHAPE;
  if (T < 0 || T > LS_MAX_T) return PANGU_E_SHAPE;
  if (lead < 0 || lead > 254) return PANGU_E_SHAPE;
  const long long slabs = (plane_elems + LS_SLAB - 1) / LS_SLAB;
  if ((long long)planes * slabs > 0x7fffffffll) return PANGU_E_SHAPE;              // a one-dimensional grid
  if (!sum && !vmin && !vmax && !when_min && !when_max && !count && !run && !longest) return PANGU_E_ARG;
  if ((when_min && !vmin) || (when_max && !vmax)) return PANGU_E_ARG;
  if (longest && !run) return PANGU_E_ARG;
  if (T > 0 && !count && !longest) return PANGU_E_ARG;
  if (T == 0 && (count || run || longest)) return PANGU_E_ARG;
  if (((size_t)src & 3) || ((size_t)mul & 3) || ((size_t)add & 3) || ((size_t)sum & 3) || ((size_t)vmin & 3) || ((size_t)vmax & 3) ||
      ((size_t)thr & 3))
    return PANGU_E_ARG;
  const LeadStatsArgs a{src, mul, add, sum, vmin, vmax, when_min, when_max, thr, count, run, longest,
                        plane_elems, planes, levels, T, lead, (int)slabs};
  const dim3 grid((unsigned)((long long)planes * slabs)), block(LS_THREADS);
  const hipStream_t s = (hipStream_t)stream;
  if (mul) {
    if (first)
      hipLaunchKernelGGL((lead_stats_kernel<true, true>), grid, block, 0, s, a);
    else
      hipLaunchKernelGGL((lead_stats_kernel<true, false>), grid, block, 0, s, a);
  } else {
    if (first)
      hipLaunchKernelGGL((lead_stats_kernel<false, true>), grid, block, 0, s, a);
    else
      hipLaunchKernelGGL((lead_stats_kernel<false, false>), grid, block, 0, s, a);
  }
  return pangu_launch_status();
}
