// Event verification of one deterministic forecast (fp32) for gfx950: the contingency table of threshold events and the sums of the
// Fractions Skill Score (FSS, Roberts & Lean 2008) over square neighbourhoods, in one streaming pass over forecast and target.
//
// pangu_event_scores_f32 reads pred and target [planes][H][W] (the target plane optionally level-reversed, as scorecard.hip addresses
// it), thresholds thr [T][planes], the row weights lat_weight [H] and domain_bits [H][W] (NULL: every point).
//   Events     f = pred > thr[t][p], o = target > thr[t][p], both strict: +inf never happens, a comparison with NaN is false
//              (non-finite values are not detected, as in reliability.hip).
//   Domain     a point is in the domain iff domain_bits == NULL or bit domain_bit of its byte is set.  The domain selects CENTRE
//              points only: every grid point feeds the neighbourhood counts, in the domain or not.
//   Table      over domain points, counts[t][p] = {hits (f and o), false alarms (f, not o), misses (o, not f), correct negatives},
//              exact integers; wsums[t][p] the same four with every point weighted by lat_weight[h], in double.
//   Box        radius r: the (2r+1) x (2r+1) grid points around (h, w); columns wrap modulo W, rows outside 0..H-1 are absent:
//              rows_h = min(h+r, H-1) - max(h-r, 0) + 1, n_h = rows_h (2r+1).  cf(h,w), co(h,w): the numbers of f and o events in it.
//   FSS sums   fss[t][p][i] = { sum_h s_h A_h, sum_h s_h B_h } with s_h = (double)lat_weight[h] / ((double)n_h n_h),
//              A_h = sum over domain points w of (cf - co)^2, B_h = sum over domain points w of (cf^2 + co^2): exact 64-bit integer
//              row sums.  FSS = 1 - num / den.  At r = 0: num = false alarms + misses, den = 2 hits + false alarms + misses.
//
// Implementation.  One workgroup owns a plane, a slab of EV_ROWS whole rows and TL of the T thresholds: TL = 4, 2 or 1, the largest
// whose LDS leaves room for three workgroups on a CU (else 1); further thresholds ride on grid.y and read the rows again.  One lane
// owns a group of four columns.  The workgroup streams the rows h0 - r_max .. h1 - 1 + r_max once, four rows in flight per lane (two
// with a stencil).  Of every row a lane keeps ONE word: 2 TL nibbles, the f bits of its four columns per threshold, then the o bits
// -- in an LDS ring of 2 r_max + 2 rows that only the lane itself reads.  Per radius and nibble it holds the VERTICAL counts of its
// four columns as the four bytes of one register (<= 65 each), moved down a row by adding the expanded nibble of row h + r and
// subtracting that of row h - r - 1.
//   For a centre row and a radius, the vertical counts are prefix-summed along the row (four columns in the lane, a shuffle scan in
// the wave with f and o of a threshold in the halves of one word, the waves' totals through LDS) into LDS; a box count is then the
// difference of two prefix entries, plus the row total where the window wraps.  A lane squares the counts of its four columns where
// the domain bit is set (< 2^28 per lane and row), the wave adds them (32-bit across 16 lanes, 64-bit beyond: B_h passes 2^32 at
// W = 1440, r = 32), and after the row's last barrier one thread per value adds the waves in wave order and writes (A_h, B_h) per
// threshold and radius > 0 to the workspace.  The row's counts -- n_domain and (n_f, n_o, n_fo) per threshold, ten bits each in one
// word -- are added across the wave, kept per (row, wave) in LDS and written after the slab's last row.  Radius 0 needs no stencil:
// its A_h = n_f + n_o - 2 n_fo and B_h = n_f + n_o follow from the row's counts.  A call whose only radius is 0 has no ring, no halo
// and one barrier.
//   A second launch, one workgroup of 256 threads per (plane, threshold), applies lat_weight and s_h in double: thread i adds rows
// i, i + 256, .. in row order, the lanes of a wave are added by a fixed butterfly and the four waves in wave order.  No atomics,
// every order is fixed: the outputs are bit-identical from run to run and do not depend on which other planes, thresholds or radii
// are in the call.
#include "common.h"
#include "plane_value.h"

namespace {

constexpr int EV_ROWS = 32;                    // rows per workgroup (one slab)
constexpr int EV_MAX_T = 4, EV_MAX_N = 4, EV_MAX_RADIUS = 32, EV_MAX_W = 4096;
constexpr int EV_MAX_WAVES = EV_MAX_W / 4 / 64;
constexpr int EV_LDS_LIMIT = 160 * 1024;       // LDS of one CU of gfx950
constexpr int EV_LDS_TARGET = EV_LDS_LIMIT / 3; // thresholds per workgroup: as many as leave room for three workgroups on a CU

struct EvRadii {
  int n;                                       // N, all radii
  int r[EV_MAX_N];                             // as given (strictly increasing)
};

template <int TL> struct EvWord { typedef uint32_t type; };
template <> struct EvWord<1> { typedef uint8_t type; };
template <> struct EvWord<2> { typedef uint16_t type; };

// values a wave leaves per row: (A, B) per radius > 0 and threshold in 64 bits; n_domain and the packed counts per threshold in 32
__host__ __device__ constexpr int ev_red_values(int TL, int NR) { return 2 * TL * NR; }
__host__ __device__ constexpr int ev_cnt_values(int TL) { return 1 + TL; }
// 64-bit words of a workspace row: n_domain, (n_f, n_o, n_fo) per threshold, (A_h, B_h) per threshold and radius
__host__ __device__ constexpr int ev_row_words(int T, int N) { return 1 + 3 * T + 2 * T * N; }

long long ev_lds_bytes(int TL, int NR, int nthreads, int rmax) {
  long long b = 2ll * EV_MAX_WAVES * ev_red_values(TL, NR) * 8;
  b += (long long)EV_ROWS * (nthreads / 64) * ev_cnt_values(TL) * 4;    // the slab's counts per wave
  if (NR > 0) {
    b += 2ll * TL * EV_MAX_WAVES * 4;                                   // the waves' totals (half of it used: f and o share a word)
    b += 2ll * TL * (4 * nthreads + 4) * 4;                             // the row's prefix sums per nibble
    b += (long long)(2 * rmax + 2) * nthreads * (TL == 4 ? 4 : TL);     // the ring
  }
  return b;
}

// the sum of the four bytes of v, each <= 65: up to 260, so it is formed in 16-bit halves (the top byte of v * 0x01010101 would hold
// it modulo 256)
__device__ __forceinline__ uint32_t ev_byte_sum(uint32_t v) {
  const uint32_t s = (v & 0x00FF00FFu) + ((v >> 8) & 0x00FF00FFu);
  return (s & 0xFFFFu) + (s >> 16);
}

// bit j of a nibble -> bit 0 of byte j
__device__ __forceinline__ uint32_t ev_expand(uint32_t nibble) { return ((nibble & 15u) * 0x00204081u) & 0x01010101u; }

// the integer twin of row16_sum (common.h): the sum over the 16 lanes of a DPP row in every lane, no LDS crossbar round trips
__device__ __forceinline__ uint32_t ev_row16_sum(uint32_t v) {
  v += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0xB1, 0xF, 0xF, true);
  v += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x4E, 0xF, 0xF, true);
  v += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x141, 0xF, 0xF, true);
  v += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x140, 0xF, 0xF, true);
  return v;
}

__device__ __forceinline__ uint32_t ev_wave_sum_u32(uint32_t v) {
  v = ev_row16_sum(v);
  v += (uint32_t)__shfl_xor((int)v, 16, 64);
  v += (uint32_t)__shfl_xor((int)v, 32, 64);
  return v;
}

// v < 2^28 per lane: 32-bit across 16 lanes, 64-bit beyond
__device__ __forceinline__ unsigned long long ev_wave_sum_u64(uint32_t v) {
  v = ev_row16_sum(v);
  unsigned long long s = v;
  s += (unsigned long long)__shfl_xor((long long)s, 16, 64);
  s += (unsigned long long)__shfl_xor((long long)s, 32, 64);
  return s;
}

__device__ __forceinline__ uint32_t ev_wave_scan(uint32_t v, int lane) {      // inclusive
#pragma unroll
  for (int d = 1; d < 64; d <<= 1) {
    const uint32_t o = (uint32_t)__shfl_up((int)v, d, 64);
    if (lane >= d) v += o;
  }
  return v;
}

// TL: thresholds of this workgroup (grid.y * TL is its first); NR: radii > 0; MASK: domain_bits given
template <int TL, int NR, bool MASK>
__global__ __launch_bounds__(EV_MAX_WAVES * 64) void event_rows_kernel(
    const float* __restrict__ pred, const float* __restrict__ target, int target_levels, const float* __restrict__ thr, int T,
    EvRadii radii, const uint32_t* __restrict__ bits, int domain_bit, unsigned long long* __restrict__ ws, int planes, int H, int W,
    int slabs) {
  typedef typename EvWord<TL>::type word_t;
  constexpr int NP = 2 * TL;                               // nibbles of a word: f of the TL thresholds, then o
  constexpr int K = ev_red_values(TL, NR);
  extern __shared__ __attribute__((aligned(16))) unsigned long long ev_lds[];
  const int nthreads = blockDim.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, waves = nthreads >> 6;
  const int PW = 4 * nthreads + 4;
  constexpr int KC = ev_cnt_values(TL);
  unsigned long long* red = ev_lds;                                              // [2][EV_MAX_WAVES][K]
  uint32_t* cnt = reinterpret_cast<uint32_t*>(red + 2 * EV_MAX_WAVES * K);       // [EV_ROWS][waves][KC]
  uint32_t* wt = cnt + EV_ROWS * waves * KC;                                     // [NP][EV_MAX_WAVES]
  uint32_t* pref = wt + NP * EV_MAX_WAVES;                                       // [NP][PW]: entry x = the sum of columns < x
  word_t* ring = reinterpret_cast<word_t*>(pref + NP * PW);                      // [2 rmax + 2][nthreads]

  const int plane = blockIdx.x / slabs, slab = blockIdx.x - plane * slabs;
  const int t0 = blockIdx.y * TL, tn = min(TL, T - t0);
  const int h0 = slab * EV_ROWS, h1 = min(H, h0 + EV_ROWS);
  const int w4 = W >> 2;
  const bool valid = tid < w4;
  const int g = valid ? tid : w4 - 1;                      // lanes past the row read its last group and count nothing
  const size_t HW = (size_t)H * W;
  const float* pp = pred + (size_t)plane * HW;
  const float* tp = target + (size_t)pk_src_plane(plane, target_levels) * HW;
  float th[TL];
#pragma unroll
  for (int t = 0; t < TL; ++t) th[t] = t < tn ? thr[(size_t)(t0 + t) * planes + plane] : __builtin_inff();

  int pr[NR > 0 ? NR : 1], pi[NR > 0 ? NR : 1];            // the radii > 0 and their places among all radii
  {
    const int skip = radii.n - NR;                         // 1 if the first radius is 0
#pragma unroll
    for (int i = 0; i < NR; ++i) {
      pr[i] = radii.r[i + skip];
      pi[i] = i + skip;
    }
  }
  const int rmax = NR > 0 ? pr[NR - 1] : 0, RING = 2 * rmax + 2;
  uint32_t V[NR > 0 ? NR : 1][NP];                         // vertical counts: byte j = column 4 g + j
#pragma unroll
  for (int i = 0; i < (NR > 0 ? NR : 1); ++i)
#pragma unroll
    for (int k = 0; k < NP; ++k) V[i][k] = 0u;

  constexpr int EV_RB = NR > 0 ? 2 : 4;                    // rows a lane has in flight: a stencil needs the registers, not the bandwidth
  const int xend = h1 + rmax;
  f32x4 p[EV_RB], q[EV_RB];                                // the rows xr .. xr + EV_RB - 1 of the lane's columns, in flight
  uint32_t dm[EV_RB];                                      // and the mask words of the centre rows they complete
  auto load_row = [&](int xr, f32x4& pv, f32x4& qv, uint32_t& dv) {
    const int hr = min(max(xr, 0), H - 1);                 // rows outside the grid are read clamped and not used
    const int off = hr * W + 4 * g;                        // < H * W < 2^31
    pv = *reinterpret_cast<const f32x4*>(pp + off);
    qv = *reinterpret_cast<const f32x4*>(tp + off);
    const int hc = min(max(xr - rmax, 0), H - 1);
    dv = MASK ? bits[hc * w4 + g] : 0u;
  };
#pragma unroll
  for (int b = 0; b < EV_RB; ++b) load_row(h0 - rmax + b, p[b], q[b], dm[b]);
#pragma unroll 1
  for (int xr = h0 - rmax; xr < xend; ++xr) {              // (workgroup-uniform throughout)
    const f32x4 pc = p[0], qc = q[0];
    const uint32_t dmc = dm[0];
#pragma unroll
    for (int b = 0; b + 1 < EV_RB; ++b) {
      p[b] = p[b + 1];
      q[b] = q[b + 1];
      dm[b] = dm[b + 1];
    }
    load_row(xr + EV_RB, p[EV_RB - 1], q[EV_RB - 1], dm[EV_RB - 1]);
    uint32_t wnew = 0u;
    if (xr >= 0 && xr < H) {
      if (valid) {
#pragma unroll
        for (int t = 0; t < TL; ++t) {
          uint32_t f = 0u, o = 0u;
#pragma unroll
          for (int j = 0; j < 4; ++j) {
            f |= (pc[j] > th[t] ? 1u : 0u) << j;
            o |= (qc[j] > th[t] ? 1u : 0u) << j;
          }
          wnew |= f << (4 * t) | o << (4 * (TL + t));
        }
      }
      if (NR > 0) ring[(xr % RING) * nthreads + tid] = (word_t)wnew;
    }
    const int c = xr - rmax;                             // the centre row whose boxes are complete now
    if (NR > 0) {
#pragma unroll
      for (int i = 0; i < NR; ++i) {
        const int a = c + pr[i], d = c - pr[i] - 1, first = max(h0 - pr[i], 0);      // rows >= first are counted
        if (a >= first && a < H) {
          const uint32_t wa = ring[(a % RING) * nthreads + tid];
#pragma unroll
          for (int k = 0; k < NP; ++k) V[i][k] += ev_expand(wa >> (4 * k));
        }
        if (d >= first) {
          const uint32_t wd = ring[(d % RING) * nthreads + tid];
#pragma unroll
          for (int k = 0; k < NP; ++k) V[i][k] -= ev_expand(wd >> (4 * k));
        }
      }
    }
    if (c < h0) continue;                                // c < h1 holds: xr < xend

    // ---- centre row c
    const uint32_t wc = NR > 0 ? (uint32_t)ring[(c % RING) * nthreads + tid] : wnew;
    uint32_t dn = valid ? 15u : 0u;                      // domain nibble of the lane's four columns
    if (MASK) {
      uint32_t m = 0u;
#pragma unroll
      for (int j = 0; j < 4; ++j) m |= ((dmc >> (8 * j + domain_bit)) & 1u) << j;
      dn &= m;
    }
    unsigned long long* rw = red + ((c & 1) * EV_MAX_WAVES + wave) * K;
    {
      uint32_t* cw = cnt + ((c - h0) * waves + wave) * KC;                 // read after the slab's last row
      if (MASK) {
        const uint32_t nd = ev_wave_sum_u32(__popc(dn));
        if (lane == 0) cw[0] = nd;
      }
#pragma unroll
      for (int t = 0; t < TL; ++t) {
        const uint32_t f = (wc >> (4 * t)) & dn, o = (wc >> (4 * (TL + t))) & dn;      // dn has four bits
        const uint32_t packed = ev_wave_sum_u32(__popc(f) | __popc(o) << 10 | __popc(f & o) << 20);      // <= 256 each
        if (lane == 0) cw[1 + t] = packed;
      }
    }
    if (NR > 0) {
#pragma unroll 1
      for (int i = 0; i < NR; ++i) {
        int r = 0;
#pragma unroll
        for (int ii = 0; ii < NR; ++ii) r = ii == i ? pr[ii] : r;          // selects, as for V below: no indexed register array
        uint32_t excl[TL];                                                 // f and o of a threshold share a scan: 16 bits each
#pragma unroll
        for (int t = 0; t < TL; ++t) {
          uint32_t vf = 0u, vo = 0u;
#pragma unroll
          for (int ii = 0; ii < NR; ++ii) {                                // a select keeps V in registers
            vf = ii == i ? V[ii][t] : vf;
            vo = ii == i ? V[ii][TL + t] : vo;
          }
          const uint32_t tot4 = ev_byte_sum(vf) | ev_byte_sum(vo) << 16;     // <= 260 each
          const uint32_t incl = ev_wave_scan(tot4, lane);                  // <= 64 * 260 each
          excl[t] = incl - tot4;
          if (lane == 63) wt[t * EV_MAX_WAVES + wave] = incl;
        }
        __syncthreads();
#pragma unroll
        for (int t = 0; t < TL; ++t) {
          uint32_t base[2] = {excl[t] & 0xFFFFu, excl[t] >> 16}, total[2] = {0u, 0u};
          for (int wv = 0; wv < waves; ++wv) {
            const uint32_t s = wt[t * EV_MAX_WAVES + wv];
            base[0] += wv < wave ? s & 0xFFFFu : 0u;
            base[1] += wv < wave ? s >> 16 : 0u;
            total[0] += s & 0xFFFFu;
            total[1] += s >> 16;
          }
#pragma unroll
          for (int fo = 0; fo < 2; ++fo) {
            const int k = fo * TL + t;
            uint32_t v = 0u;
#pragma unroll
            for (int ii = 0; ii < NR; ++ii) v = ii == i ? V[ii][k] : v;
            const uint32_t b0 = v & 255u, b1 = (v >> 8) & 255u, b2 = (v >> 16) & 255u, e = base[fo];
            if (valid) *reinterpret_cast<u32x4*>(pref + k * PW + 4 * tid) = u32x4{e, e + b0, e + b0 + b1, e + b0 + b1 + b2};
            if (tid == 0) pref[k * PW + W] = total[fo];
          }
        }
        __syncthreads();
#pragma unroll 1
        for (int t = 0; t < TL; ++t) {                                     // (no register array is indexed by t here)
          const uint32_t* ef = pref + t * PW;
          const uint32_t* eo = pref + (TL + t) * PW;
          const uint32_t totf = ef[W], toto = eo[W];
          uint32_t sa = 0u, sb = 0u;
#pragma unroll
          for (int j = 0; j < 4; ++j) {
            int lo = 4 * g + j - r, hi = 4 * g + j + r + 1;               // columns lo .. hi - 1; 2 r + 1 <= W: one wrap at most
            const bool wrap = lo < 0 || hi > W;
            lo += lo < 0 ? W : 0;
            hi -= hi > W ? W : 0;
            const uint32_t cf = ef[hi] - ef[lo] + (wrap ? totf : 0u);
            const uint32_t co = eo[hi] - eo[lo] + (wrap ? toto : 0u);
            const uint32_t df = cf - co;                                  // modulo 2^32; its square is exact: |cf - co| <= 4225
            const bool in = (dn >> j) & 1u;
            sa += in ? df * df : 0u;
            sb += in ? cf * cf + co * co : 0u;
          }
          const unsigned long long A = ev_wave_sum_u64(sa), B = ev_wave_sum_u64(sb);
          if (lane == 0) {
            rw[(i * TL + t) * 2] = A;
            rw[(i * TL + t) * 2 + 1] = B;
          }
        }
      }
    }
    if (NR > 0) {
      __syncthreads();
      // one thread per value: the waves in wave order -> the row's integers.  The next row writes the other half of `red`.
      if (tid < K) {
        const int i = tid / (2 * TL), t = (tid >> 1) % TL, ab = tid & 1;
        if (t < tn) {
          const unsigned long long* rb = red + (c & 1) * EV_MAX_WAVES * K;
          unsigned long long s = 0ull;
          for (int wv = 0; wv < waves; ++wv) s += rb[wv * K + tid];
          int place = 0;
#pragma unroll
          for (int ii = 0; ii < NR; ++ii) place = ii == i ? pi[ii] : place;
          ws[((size_t)plane * H + c) * ev_row_words(T, radii.n) + 1 + 3 * T + ((t0 + t) * radii.n + place) * 2 + ab] = s;
        }
      }
    }
  }
  // the slab's counts: one thread per (row, value), the waves in wave order
  __syncthreads();
  for (int e = tid; e < (h1 - h0) * (1 + 3 * TL); e += nthreads) {
    const int row = e / (1 + 3 * TL), j = e - row * (1 + 3 * TL);
    const uint32_t* cb = cnt + row * waves * KC;
    unsigned long long* out = ws + ((size_t)plane * H + h0 + row) * ev_row_words(T, radii.n);
    if (j == 0) {
      if (t0 == 0) {
        unsigned long long s = (unsigned long long)W;                        // no mask: every point
        if (MASK) {
          s = 0ull;
          for (int wv = 0; wv < waves; ++wv) s += cb[wv * KC];
        }
        out[0] = s;
      }
    } else {
      const int t = (j - 1) / 3, which = (j - 1) - 3 * t;
      if (t < tn) {
        unsigned long long s = 0ull;
        for (int wv = 0; wv < waves; ++wv) s += (cb[wv * KC + 1 + t] >> (10 * which)) & 0x3FFu;
        out[1 + 3 * (t0 + t) + which] = s;
      }
    }
  }
}

// one workgroup per (plane, threshold): thread i takes rows i, i + EV_FINAL_THREADS, .. in row order (three at H = 721: their loads
// are in flight together), the lanes of a wave join in a fixed butterfly, thread 0 adds the waves in wave order
constexpr int EV_FINAL_THREADS = 256;
__global__ __launch_bounds__(EV_FINAL_THREADS) void event_final_kernel(const unsigned long long* __restrict__ ws,
                                                                       const float* __restrict__ lat_w,
                                                         EvRadii radii, int T, int planes, int H, int W,
                                                         unsigned long long* __restrict__ counts, double* __restrict__ wsums,
                                                         double* __restrict__ fss) {
#pragma clang fp contract(off)
  __shared__ unsigned long long fin[EV_FINAL_THREADS / 64][8 + 2 * EV_MAX_N];
  const int p = blockIdx.x, t = blockIdx.y, lane = threadIdx.x & 63, wave = threadIdx.x >> 6, N = radii.n;
  const int RW = ev_row_words(T, N);
  unsigned long long cnt[4] = {0ull, 0ull, 0ull, 0ull};
  double wsum[4] = {0.0, 0.0, 0.0, 0.0};
  double fa[EV_MAX_N], fb[EV_MAX_N];
#pragma unroll
  for (int i = 0; i < EV_MAX_N; ++i) fa[i] = fb[i] = 0.0;
#pragma unroll 4
  for (int h = threadIdx.x; h < H; h += EV_FINAL_THREADS) {
    const unsigned long long* row = ws + ((size_t)p * H + h) * RW;
    const unsigned long long nd = row[0], nf = row[1 + 3 * t], no = row[2 + 3 * t], nfo = row[3 + 3 * t];
    const unsigned long long c4[4] = {nfo, nf - nfo, no - nfo, nd - nf - no + nfo};
    const double w = (double)lat_w[h];
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      cnt[k] += c4[k];
      wsum[k] += w * (double)c4[k];
    }
#pragma unroll
    for (int i = 0; i < EV_MAX_N; ++i) {
      if (i < N) {
        const int r = radii.r[i];
        unsigned long long A, B;
        if (r == 0) {
          A = c4[1] + c4[2];
          B = nf + no;
        } else {
          A = row[1 + 3 * T + (t * N + i) * 2];
          B = row[1 + 3 * T + (t * N + i) * 2 + 1];
        }
        const double n = (double)((min(h + r, H - 1) - max(h - r, 0) + 1) * (2 * r + 1));
        const double s = w / (n * n);
        fa[i] += s * (double)A;
        fb[i] += s * (double)B;
      }
    }
  }
#pragma unroll
  for (int d = 1; d < 64; d <<= 1) {
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      cnt[k] += (unsigned long long)__shfl_xor((long long)cnt[k], d, 64);
      wsum[k] += __shfl_xor(wsum[k], d, 64);
    }
#pragma unroll
    for (int i = 0; i < EV_MAX_N; ++i) {
      fa[i] += __shfl_xor(fa[i], d, 64);
      fb[i] += __shfl_xor(fb[i], d, 64);
    }
  }
  if (lane == 0) {
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      fin[wave][k] = cnt[k];
      fin[wave][4 + k] = __builtin_bit_cast(unsigned long long, wsum[k]);
    }
#pragma unroll
    for (int i = 0; i < EV_MAX_N; ++i) {
      fin[wave][8 + 2 * i] = __builtin_bit_cast(unsigned long long, fa[i]);
      fin[wave][9 + 2 * i] = __builtin_bit_cast(unsigned long long, fb[i]);
    }
  }
  __syncthreads();
  if (threadIdx.x < 8 + 2 * N) {                           // one thread per output value
    const int v = threadIdx.x;
    const size_t tp = (size_t)t * planes + p;
    if (v < 4) {
      unsigned long long c = fin[0][v];
      for (int wv = 1; wv < EV_FINAL_THREADS / 64; ++wv) c += fin[wv][v];
      counts[tp * 4 + v] = c;
    } else {
      double x = __builtin_bit_cast(double, fin[0][v]);
      for (int wv = 1; wv < EV_FINAL_THREADS / 64; ++wv) x += __builtin_bit_cast(double, fin[wv][v]);
      if (v < 8) wsums[tp * 4 + (v - 4)] = x;
      else fss[tp * N * 2 + (v - 8)] = x;
    }
  }
}

long long event_slabs(int H) { return ((long long)H + EV_ROWS - 1) / EV_ROWS; }

template <int TL, int NR, bool MASK>
void launch_event_rows(hipStream_t s, dim3 grid, int threads, int lds, const float* pred, const float* target, int target_levels,
                       const float* thr, int T, const EvRadii& radii, const uint32_t* bits, int domain_bit, unsigned long long* ws,
                       int planes, int H, int W, int slabs) {
  auto kern = event_rows_kernel<TL, NR, MASK>;
  PANGU_ENSURE_DYN_LDS(kern, EV_LDS_LIMIT);
  hipLaunchKernelGGL(kern, grid, dim3(threads), lds, s, pred, target, target_levels, thr, T, radii, bits, domain_bit, ws, planes, H,
                     W,
                     slabs);
}

}  // namespace

extern "C" long long pangu_event_scores_ws_bytes(int planes, int H, int T, int N) {
  if (planes <= 0 || H <= 0 || T < 1 || T > EV_MAX_T || N < 1 || N > EV_MAX_N) return PANGU_E_SHAPE;
  if ((long long)planes * event_slabs(H) > 0x7FFFFFFFll) return PANGU_E_SHAPE;      // grid.x
  return (long long)planes * H * ev_row_words(T, N) * 8;
}

extern "C" int pangu_event_scores_f32(pangu_stream_t stream, const float* pred, const float* target, int target_levels,
                                      const float* thresholds, int T, const int* radii, int N, const float* lat_weight,
                                      const unsigned char* domain_bits, int domain_bit, unsigned long long* counts, double* wsums,
                                      double* fss, void* workspace, long long workspace_bytes, int planes, int H, int W) {
  if (!pred || !target || !thresholds || !radii || !lat_weight || !counts || !wsums || !fss || !workspace) return PANGU_E_NULL;
  if (planes <= 0 || H <= 0 || W <= 0 || (W & 3) || W > EV_MAX_W) return PANGU_E_SHAPE;
  if (T < 1 || T > EV_MAX_T || N < 1 || N > EV_MAX_N) return PANGU_E_SHAPE;
  EvRadii rad;
  rad.n = N;
  for (int i = 0; i < EV_MAX_N; ++i) rad.r[i] = 0;
  for (int i = 0; i < N; ++i) {
    const int r = radii[i];
    if (r < 0 || r > EV_MAX_RADIUS || 2 * r + 1 > W || (i > 0 && r <= radii[i - 1])) return PANGU_E_SHAPE;
    rad.r[i] = r;
  }
  if ((long long)H * W > 0x7FFFFFFFll) return PANGU_E_SHAPE;                             // 32-bit indices within a plane
  if (target_levels < 0 || (target_levels > 1 && planes % target_levels != 0)) return PANGU_E_SHAPE;
  const long long need = pangu_event_scores_ws_bytes(planes, H, T, N);
  if (need < 0) return PANGU_E_SHAPE;
  if (domain_bit < 0 || domain_bit > 7) return PANGU_E_ARG;
  if (workspace_bytes < need) return PANGU_E_ARG;
  if ((reinterpret_cast<size_t>(pred) | reinterpret_cast<size_t>(target) | reinterpret_cast<size_t>(workspace)) & 15)
    return PANGU_E_ARG;
  if ((reinterpret_cast<size_t>(thresholds) | reinterpret_cast<size_t>(lat_weight) | reinterpret_cast<size_t>(domain_bits)) & 3)
    return PANGU_E_ARG;
  if ((reinterpret_cast<size_t>(counts) | reinterpret_cast<size_t>(wsums) | reinterpret_cast<size_t>(fss)) & 7) return PANGU_E_ARG;

  hipStream_t s = (hipStream_t)stream;
  const int slabs = (int)event_slabs(H);
  const int threads = 64 * (((W >> 2) + 63) / 64);
  const int NR = N - (rad.r[0] == 0 ? 1 : 0), rmax = NR > 0 ? rad.r[N - 1] : 0;
  int TL = T >= 3 ? 4 : T;
  while (TL > 1 && ev_lds_bytes(TL, NR, threads, rmax) > EV_LDS_TARGET) TL >>= 1;      // (measured: DESIGN.md 3d)
  const int lds = (int)ev_lds_bytes(TL, NR, threads, rmax);      // TL = 1 always fits: 106,656 bytes at W = 4096, r = 32
  const dim3 grid((unsigned)(planes * slabs), (unsigned)((T + TL - 1) / TL));
  unsigned long long* ws = static_cast<unsigned long long*>(workspace);
  const uint32_t* bits = reinterpret_cast<const uint32_t*>(domain_bits);
#define EV_ARGS s, grid, threads, lds, pred, target, target_levels, thresholds, T, rad, bits, domain_bit, ws, planes, H, W, slabs
#define EV_LAUNCH_NR(TLV, NRV)                              \
  do {                                                      \
    if (bits) launch_event_rows<TLV, NRV, true>(EV_ARGS);   \
    else launch_event_rows<TLV, NRV, false>(EV_ARGS);       \
  } while (0)
#define EV_LAUNCH_TL(TLV)                 \
  do {                                    \
    if (NR == 0) EV_LAUNCH_NR(TLV, 0);    \
    else if (NR == 1) EV_LAUNCH_NR(TLV, 1); \
    else if (NR == 2) EV_LAUNCH_NR(TLV, 2); \
    else if (NR == 3) EV_LAUNCH_NR(TLV, 3); \
    else EV_LAUNCH_NR(TLV, 4);            \
  } while (0)
  if (TL == 4) EV_LAUNCH_TL(4);
  else if (TL == 2) EV_LAUNCH_TL(2);
  else EV_LAUNCH_TL(1);
#undef EV_LAUNCH_TL
#undef EV_LAUNCH_NR
#undef EV_ARGS
  const int rc = pangu_launch_status();
  if (rc != PANGU_OK) return rc;
  hipLaunchKernelGGL(event_final_kernel, dim3((unsigned)planes, (unsigned)T), dim3(EV_FINAL_THREADS), 0, s, ws, lat_weight, rad, T,
                     planes, H, W,
                     counts, wsums, fss);
  return pangu_launch_status();
}
