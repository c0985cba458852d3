// Regional scorecard sums of one deterministic forecast (fp32) for gfx950: every latitude-weighted sum that bias, MAE, RMSE, ACC
// (uncentred and centred), forecast activity and wind-vector RMSE need, for up to 8 arbitrary regions, in one streaming pass.
//
// pangu_scorecard_sums_f32 reads pred p and target t [planes][H][W] (the target plane optionally level-reversed, as pack.hip and
// regrid.hip address it), a climatology c (none: c = 0; one scalar per plane; or a field [planes][H][W]), the row weights w [H]
// and region_bits [H][W] (bit r of a point's byte: the point belongs to region r < R; NULL: one region that holds every point).
// With d = p - t, a = p - c, b = t - c (one fp32 rounding each), per (plane, region), over the region's points:
//   sums[0] = sum w      sums[1] = sum w d     sums[2] = sum w |d|    sums[3] = sum w d^2    sums[4] = sum w a
//   sums[5] = sum w b    sums[6] = sum w a b   sums[7] = sum w a^2    sums[8] = sum w b^2    sums[9] = number of points
//
// Implementation.  One workgroup per (plane, slab of SCD_ROWS rows), one lane per column group of four points: a lane walks DOWN
// its four columns through the slab's rows, SCD_RB rows at a time, and issues the 16-byte loads of those rows (pred, target, the
// climatology field) and their 4-byte mask words before it uses the first.  The block has one wave per 64 column groups (six waves
// for W = 1440: 360 of 384 lanes work), at most eight; wider rows are swept in column tiles.
//   Region membership costs nothing per point where the mask does not change down a lane's columns: a lane keeps two CLASS
// accumulators A and B (nine weighted sums and a count each), keyed by the mask byte they collect (A: the byte of its first word, B:
// the first other byte that fills a whole word).  The four points of a word are added without their weight and enter the class
// whose key all four bytes equal with ONE fma per sum and row.  A word that belongs to neither class -- a coastline or a box edge
// that cuts the word, a third class in the slab -- is DEFERRED: the lane sets the row's bit and goes on.  After the rows the
// wave packs its deferred words into a queue in LDS (16 bits each: row and lane), in (row, lane) order, and takes them 64 at a
// time: every lane reads one word again (it is in cache) and adds its four points straight into the accumulators of the regions
// whose bit the point's byte holds; a region that holds none of the 64 lanes' points is skipped (a wave-uniform branch).
// So the point-by-point work costs what the mixed words are, a few per cent, not a pass of the whole wave per row that holds
// one.  The classes join the region accumulators through wave-uniform branches when all lanes hold one key, else by selects.
// Membership is always a select or a branch, never a product with 0: a non-finite value reaches exactly the regions that hold its
// point.
//   The lanes' region accumulators are added across the wave through LDS, 16 values at a time: the wave writes value-major and
// every lane adds 16 lanes' entries of one value in lane order, a quad of lanes then holds the four parts (two more adds); one
// thread per value adds the waves in wave order and writes the slab's partial to the workspace.  Up to that last step a wave works
// in its own part of LDS: its accesses are ordered by waiting for them (sc_wave_sync), the workgroup meets at one barrier.  A second launch adds the slabs
// in slab order in double (the counts as integers).  No atomics, every order is fixed: the sums are bit-identical from run to
// run, and a plane's sums do not depend on the other planes of the launch.
//
// Rounding.  Per column tile a term passes through at most 3 + SCD_ROWS fp32 additions in its class, 2 when the classes join the
// region accumulators and 4 * SCD_ROWS from the deferred words (a lane takes at most SCD_ROWS of them); then 17 in the wave, one
// per column tile, and 7 across eight waves.
#include "common.h"
#include "plane_value.h"

namespace {

constexpr int SCD_ROWS = 32;                   // rows per workgroup (one slab)
constexpr int SCD_RB = 4;                      // rows a lane has in flight
constexpr int SCD_MAX_WAVES = 8;
constexpr int SCD_SUMS = 10;                   // per (plane, region): nine fp32 sums and the count
constexpr int SCD_MAX_R = 8;
constexpr uint32_t SCD_NOKEY = 0x100u;         // the key of an empty class: no mask byte equals it and it holds no region's bit

struct ScClass {                               // s[0] = sum w, s[1..8] as sums[1..8]; n points
  float s[9];
  uint32_t n;
};

__device__ __forceinline__ void sc_zero(ScClass& c) {
#pragma unroll
  for (int k = 0; k < 9; ++k) c.s[k] = 0.0f;
  c.n = 0u;
}

template <int RMAX>
struct ScRegions {
  float s[RMAX][9];
  uint32_t n[RMAX];
};

// x[1..8]: the unweighted terms of one point
template <int CLIM>
__device__ __forceinline__ void sc_terms(float p, float t, float c, float (&x)[9]) {
  const float d = p - t, a = CLIM ? p - c : p, b = CLIM ? t - c : t;
  x[0] = 1.0f;
  x[1] = d; x[2] = fabsf(d); x[3] = d * d;
  x[4] = a; x[5] = b; x[6] = a * b; x[7] = a * a; x[8] = b * b;
}

// class `c` into the regions whose bit `key` holds, by selects (key differs from lane to lane)
template <int RMAX>
__device__ __forceinline__ void sc_retire_select(ScRegions<RMAX>& acc, const ScClass& c, uint32_t key) {
#pragma unroll
  for (int r = 0; r < RMAX; ++r) {
    const bool in = (key >> r) & 1u;
#pragma unroll
    for (int k = 0; k < 9; ++k) acc.s[r][k] += in ? c.s[k] : 0.0f;
    acc.n[r] += in ? c.n : 0u;
  }
}

// the same with a key that is uniform over the wave (an SGPR): branches instead of selects
template <int RMAX>
__device__ __forceinline__ void sc_retire_uniform(ScRegions<RMAX>& acc, const ScClass& c, uint32_t key) {
#pragma unroll
  for (int r = 0; r < RMAX; ++r) {
    if ((key >> r) & 1u) {
#pragma unroll
      for (int k = 0; k < 9; ++k) acc.s[r][k] += c.s[k];
      acc.n[r] += c.n;
    }
  }
}

// orders a wave's own LDS accesses: the earlier ones are complete before the later ones are issued, and the compiler moves none across
__device__ __forceinline__ void sc_wave_sync() {
  __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "workgroup");
  __builtin_amdgcn_wave_barrier();
}

// g[1..8]: the terms of the four points of a word, added without their weight
template <int CLIM>
__device__ __forceinline__ void sc_word_sums(const f32x4 p, const f32x4 t, const f32x4 cl, float (&g)[9]) {
  float x[9];
  sc_terms<CLIM>(p[0], t[0], cl[0], g);
#pragma unroll
  for (int q = 1; q < 4; ++q) {
    sc_terms<CLIM>(p[q], t[q], cl[q], x);
#pragma unroll
    for (int k = 1; k < 9; ++k) g[k] += x[k];
  }
}

// a word's four points into their class: one fma per sum
__device__ __forceinline__ void sc_class_add(ScClass& c, const float (&g)[9], float w) {
  c.s[0] = fmaf(w, 4.0f, c.s[0]);
#pragma unroll
  for (int k = 1; k < 9; ++k) c.s[k] = fmaf(w, g[k], c.s[k]);
  c.n += 4u;
}

// RMAX: region accumulators kept (1, 4 or 8 >= R); CLIM: the climatology kind; MASK: region_bits given
template <int RMAX, int CLIM, bool MASK>
__global__ __launch_bounds__(SCD_MAX_WAVES * 64) void scorecard_sums_kernel(
    const float* __restrict__ pred, const float* __restrict__ target, int target_levels, const float* __restrict__ clim,
    const float* __restrict__ lat_w, const uint32_t* __restrict__ bits, int R, uint32_t* __restrict__ ws, int H, int W, int slabs) {
  constexpr int FVALS = 9 * RMAX, FCH = (FVALS + 15) / 16, XW = (FCH + 1) * 16;
  // per wave: the queue of deferred words (at most SCD_ROWS * 64), then 16 values of every lane, value-major
  __shared__ __attribute__((aligned(16))) uint32_t sc_tr[SCD_MAX_WAVES][16 * 64];
  __shared__ uint32_t sc_xw[SCD_MAX_WAVES][XW];                                        // the waves' sums per value
  static_assert(SCD_ROWS <= 32 && SCD_ROWS * 64 * 2 <= 16 * 64 * 4, "a bit per row; the queue of deferred words (16 bits each) lives in the wave's transpose buffer");

  const int plane = blockIdx.x / slabs, slab = blockIdx.x - plane * slabs;
  const int h0 = slab * SCD_ROWS, hend = min(H, h0 + SCD_ROWS);
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, nthreads = blockDim.x;
  const int w4 = W >> 2;
  const size_t HW = (size_t)H * W;
  const float* pp = pred + (size_t)plane * HW;
  const float* tp = target + (size_t)pk_src_plane(plane, target_levels) * HW;
  const float* cp = CLIM == 2 ? clim + (size_t)plane * HW : nullptr;
  const float cs = CLIM == 1 ? clim[plane] : 0.0f;
  const uint32_t keep = (MASK ? ((1u << R) - 1u) : 1u) * 0x01010101u;                  // bits of regions >= R are ignored
  uint32_t* tr = sc_tr[wave];
  uint16_t* queue = reinterpret_cast<uint16_t*>(tr);

  // Up to the last step a wave touches its own part of LDS only, and a wave's LDS operations execute in order: its lanes' writes
  // and reads are ordered by sc_wave_sync (no s_barrier)
  for (int i = lane; i < XW; i += 64) sc_xw[wave][i] = 0u;      // +0.0f and 0
  sc_wave_sync();

  for (int tile = 0; tile * nthreads < w4; ++tile) {        // (workgroup-uniform) one column tile: a lane's four columns
    const int gw = tile * nthreads + wave * 64;             // this wave's first column group
    const bool valid = gw + lane < w4;
    const int g = valid ? gw + lane : w4 - 1;               // lanes past the row read its last group and add nothing
    ScClass A, B;
    sc_zero(A);
    sc_zero(B);
    uint32_t keyA = MASK ? SCD_NOKEY : 1u, keyB = SCD_NOKEY;      // A takes the byte of the lane's first word
    uint32_t defer = 0u;                                    // bit i: the word of row h0 + i waits for the second pass

    for (int h = h0; h < hend; h += SCD_RB) {
      f32x4 p[SCD_RB], t[SCD_RB], c[SCD_RB];
      uint32_t m[SCD_RB];
#pragma unroll
      for (int r = 0; r < SCD_RB; ++r) {
        const int hr = min(h + r, hend - 1);
        const int off = hr * W + 4 * g;                     // < H * W < 2^31
        p[r] = *reinterpret_cast<const f32x4*>(pp + off);
        t[r] = *reinterpret_cast<const f32x4*>(tp + off);
        if (CLIM == 2) c[r] = *reinterpret_cast<const f32x4*>(cp + off);
        else c[r] = f32x4{cs, cs, cs, cs};
        m[r] = MASK ? (bits[hr * w4 + g] & keep) : 0x01010101u;
      }
      if (MASK && h == h0) keyA = m[0] & 0xFFu;             // (workgroup-uniform)
#pragma unroll
      for (int r = 0; r < SCD_RB; ++r) {
        if (h + r < hend) {                                 // (workgroup-uniform)
          const float w = lat_w[h + r];
          float gs[9];
          sc_word_sums<CLIM>(p[r], t[r], c[r], gs);
          if (!MASK) {
            sc_class_add(A, gs, w);
          } else {
            const uint32_t byte = m[r] & 0xFFu;
            const bool whole = m[r] == byte * 0x01010101u;  // one class holds the four points
            if (whole && byte != keyA && keyB == SCD_NOKEY) keyB = byte;
            if (whole && byte == keyA)
              sc_class_add(A, gs, w);
            else if (whole && byte == keyB)
              sc_class_add(B, gs, w);
            else
              defer |= 1u << (h + r - h0);
          }
        }
      }
    }
    if (!valid) {                                           // what a lane past the row gathered from the last group is dropped
      sc_zero(A);
      sc_zero(B);
      keyA = 0u;
      keyB = SCD_NOKEY;
      defer = 0u;
    }

    ScRegions<RMAX> acc;
#pragma unroll
    for (int r = 0; r < RMAX; ++r) {
#pragma unroll
      for (int k = 0; k < 9; ++k) acc.s[r][k] = 0.0f;
      acc.n[r] = 0u;
    }
    // the two classes into the regions whose bit their key holds
    const uint32_t sA = (uint32_t)__builtin_amdgcn_readfirstlane((int)keyA);
    if (__ballot(valid && keyA != sA) == 0ull)
      sc_retire_uniform<RMAX>(acc, A, sA);                  // (lanes past the row hold zeros)
    else
      sc_retire_select<RMAX>(acc, A, keyA);
    if (MASK && __ballot(keyB != SCD_NOKEY) != 0ull) sc_retire_select<RMAX>(acc, B, keyB);

    // second pass: the deferred words of the wave, packed 64 at a time, point by point straight into the regions
    if (MASK && __ballot(defer != 0u) != 0ull) {            // (wave-uniform)
      int total = 0;
#pragma unroll 1
      for (int b = 0; b < SCD_ROWS; ++b) {                  // the queue, in (row, lane) order
        const bool mine = (defer >> b) & 1u;
        const unsigned long long bal = __ballot(mine);
        if (mine) {
          const uint32_t before = __builtin_amdgcn_mbcnt_hi((uint32_t)(bal >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)bal, 0u));
          queue[total + before] = (uint16_t)((b << 6) | lane);
        }
        total += __popcll(bal);
      }
      sc_wave_sync();
#pragma unroll 1
      for (int i0 = 0; i0 < total; i0 += 64) {
        if (i0 + lane < total) {
          const uint32_t e = queue[i0 + lane];
          const int hr = h0 + (int)(e >> 6), gq = gw + (int)(e & 63u);
          const int off = hr * W + 4 * gq;
          f32x4 pq = *reinterpret_cast<const f32x4*>(pp + off), tq = *reinterpret_cast<const f32x4*>(tp + off);
          f32x4 cq = f32x4{cs, cs, cs, cs};
          if (CLIM == 2) cq = *reinterpret_cast<const f32x4*>(cp + off);
          uint32_t mq = bits[hr * w4 + gq] & keep;
          const float w = lat_w[hr];
#pragma unroll 1
          for (int q = 0; q < 4; ++q) {
            float x[9];
            sc_terms<CLIM>(pq[0], tq[0], cq[0], x);
            x[0] = w;
#pragma unroll
            for (int k = 1; k < 9; ++k) x[k] *= w;
#pragma unroll
            for (int r = 0; r < RMAX; ++r) {
              const bool in = (mq >> r) & 1u;
              if (__ballot(in) == 0ull) continue;             // (wave-uniform) no lane's point lies in this region
#pragma unroll
              for (int k = 0; k < 9; ++k) acc.s[r][k] += in ? x[k] : 0.0f;
              acc.n[r] += in ? 1u : 0u;
            }
            pq = f32x4{pq[1], pq[2], pq[3], pq[0]};
            tq = f32x4{tq[1], tq[2], tq[3], tq[0]};
            cq = f32x4{cq[1], cq[2], cq[3], cq[0]};
            mq >>= 8;
          }
        }
      }
    }

  // the lanes' sums across the wave, 16 values at a time: value-major into LDS, lane l adds lanes 16 (l % 4) .. + 15 of value
  // l / 4 in lane order, its quad holds the four parts
#pragma unroll
  for (int ch = 0; ch <= FCH; ++ch) {
#pragma unroll
    for (int j = 0; j < 16; ++j) {
      const int v = ch * 16 + j;
      uint32_t bitsv = 0u;
      if (ch < FCH) {
        if (v < FVALS) bitsv = __builtin_bit_cast(uint32_t, acc.s[v / 9][v % 9]);
      } else if (j < RMAX) {
        bitsv = acc.n[j];
      }
      tr[j * 64 + lane] = bitsv;
    }
    sc_wave_sync();
    const u32x4* src = reinterpret_cast<const u32x4*>(tr + lane * 16);
    uint32_t e[16];
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const u32x4 x = src[i];
      e[4 * i] = x[0];
      e[4 * i + 1] = x[1];
      e[4 * i + 2] = x[2];
      e[4 * i + 3] = x[3];
    }
    uint32_t out;
    if (ch < FCH) {
      float s = __uint_as_float(e[0]);
#pragma unroll
      for (int i = 1; i < 16; ++i) s += __uint_as_float(e[i]);
      s += __shfl_xor(s, 1, 64);
      s += __shfl_xor(s, 2, 64);
      out = __builtin_bit_cast(uint32_t, s);
    } else {
      uint32_t s = 0u;
#pragma unroll
      for (int i = 0; i < 16; ++i) s += e[i];
      s += (uint32_t)__shfl_xor((int)s, 1, 64);
      s += (uint32_t)__shfl_xor((int)s, 2, 64);
      out = s;
    }
    if ((lane & 3) == 0) {                                  // this tile's sum joins the earlier tiles' (the first joins zero)
      uint32_t& cell = sc_xw[wave][ch * 16 + (lane >> 2)];
      cell = ch < FCH ? __float_as_uint(__uint_as_float(cell) + __uint_as_float(out)) : cell + out;
    }
    sc_wave_sync();
  }
  }
  __syncthreads();

  // one thread per (region, sum): the waves in wave order -> the slab's partial
  const int waves = nthreads >> 6;
  for (int i = threadIdx.x; i < R * SCD_SUMS; i += nthreads) {
    const int r = i / SCD_SUMS, k = i - r * SCD_SUMS;
    const int v = k < 9 ? r * 9 + k : FCH * 16 + r;
    uint32_t out;
    if (k < 9) {
      float s = __builtin_bit_cast(float, sc_xw[0][v]);
      for (int wv = 1; wv < waves; ++wv) s += __builtin_bit_cast(float, sc_xw[wv][v]);
      out = __builtin_bit_cast(uint32_t, s);
    } else {
      out = 0u;
      for (int wv = 0; wv < waves; ++wv) out += sc_xw[wv][v];
    }
    ws[(size_t)blockIdx.x * R * SCD_SUMS + i] = out;
  }
}

// sums [plane][region][10] from the slab partials, added in slab order: the fp32 sums in double, the counts as integers
__global__ __launch_bounds__(256) void scorecard_final_kernel(const uint32_t* __restrict__ ws, double* __restrict__ sums, int planes,
                                                              int slabs, int per_plane) {
  const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
  if (i >= (long long)planes * per_plane) return;
  const long long plane = i / per_plane, j = i - plane * per_plane;
  const uint32_t* src = ws + plane * slabs * per_plane + j;
  if (j % SCD_SUMS == 9) {
    unsigned long long n = 0ull;
    for (int sl = 0; sl < slabs; ++sl) n += src[(long long)sl * per_plane];
    sums[i] = (double)n;
  } else {
    double s = 0.0;
    for (int sl = 0; sl < slabs; ++sl) s += (double)__builtin_bit_cast(float, src[(long long)sl * per_plane]);
    sums[i] = s;
  }
}

template <int RMAX, bool MASK>
void launch_scorecard(hipStream_t s, int grid, int threads, const float* pred, const float* target, int target_levels,
                      const float* clim, int clim_kind, const float* w, const uint32_t* bits, int R, uint32_t* ws, int H, int W,
                      int slabs) {
#define SCD_LAUNCH(CLIM)                                                                                                        \
  hipLaunchKernelGGL((scorecard_sums_kernel<RMAX, CLIM, MASK>), dim3(grid), dim3(threads), 0, s, pred, target, target_levels, \
                     clim, w, bits, R, ws, H, W, slabs)
  if (clim_kind == 0) SCD_LAUNCH(0);
  else if (clim_kind == 1) SCD_LAUNCH(1);
  else SCD_LAUNCH(2);
#undef SCD_LAUNCH
}

long long scorecard_slabs(int H) { return ((long long)H + SCD_ROWS - 1) / SCD_ROWS; }

}  // namespace

extern "C" long long pangu_scorecard_ws_bytes(int planes, int H, int R) {
  if (planes <= 0 || H <= 0 || R < 1 || R > SCD_MAX_R) return PANGU_E_SHAPE;
  if ((long long)planes * scorecard_slabs(H) > 0x7FFFFFFFll) return PANGU_E_SHAPE;      // a one-dimensional grid
  return (long long)planes * scorecard_slabs(H) * R * SCD_SUMS * 4;
}

extern "C" int pangu_scorecard_sums_f32(pangu_stream_t stream, const float* pred, const float* target, int target_levels,
                                        const float* clim, int clim_kind, const float* lat_weight,
                                        const unsigned char* region_bits, int R, double* sums, void* workspace,
                                        long long workspace_bytes, int planes, int H, int W) {
  if (!pred || !target || !lat_weight || !sums || !workspace) return PANGU_E_NULL;
  if (clim_kind != 0 && !clim) return PANGU_E_NULL;
  if (!region_bits && R != 1) return PANGU_E_NULL;
  if (planes <= 0 || H <= 0 || W <= 0 || (W & 3) || R < 1 || R > SCD_MAX_R) return PANGU_E_SHAPE;
  if ((long long)H * W > 0x7FFFFFFFll) return PANGU_E_SHAPE;                             // 32-bit indices within a plane
  if (target_levels < 0 || (target_levels > 1 && planes % target_levels != 0)) return PANGU_E_SHAPE;
  const long long need = pangu_scorecard_ws_bytes(planes, H, R);
  if (need < 0) return PANGU_E_SHAPE;
  if (clim_kind < 0 || clim_kind > 2) return PANGU_E_ARG;
  if (workspace_bytes < need) return PANGU_E_ARG;
  if ((reinterpret_cast<size_t>(pred) | reinterpret_cast<size_t>(target) | reinterpret_cast<size_t>(workspace)) & 15)
    return PANGU_E_ARG;
  if (clim_kind == 2 && (reinterpret_cast<size_t>(clim) & 15)) return PANGU_E_ARG;
  if (clim_kind == 1 && (reinterpret_cast<size_t>(clim) & 3)) return PANGU_E_ARG;
  if ((reinterpret_cast<size_t>(lat_weight) & 3) || (reinterpret_cast<size_t>(sums) & 7) ||
      (reinterpret_cast<size_t>(region_bits) & 3))
    return PANGU_E_ARG;
  hipStream_t s = (hipStream_t)stream;
  const int slabs = (int)scorecard_slabs(H), grid = planes * slabs;
  const int waves = min(SCD_MAX_WAVES, ((W >> 2) + 63) / 64), threads = 64 * waves;
  uint32_t* ws = static_cast<uint32_t*>(workspace);
  const uint32_t* bits = reinterpret_cast<const uint32_t*>(region_bits);
  if (!bits)
    launch_scorecard<1, false>(s, grid, threads, pred, target, target_levels, clim, clim_kind, lat_weight, bits, R, ws, H, W, slabs);
  else if (R == 1)
    launch_scorecard<1, true>(s, grid, threads, pred, target, target_levels, clim, clim_kind, lat_weight, bits, R, ws, H, W, slabs);
  else if (R <= 4)
    launch_scorecard<4, true>(s, grid, threads, pred, target, target_levels, clim, clim_kind, lat_weight, bits, R, ws, H, W, slabs);
  else
    launch_scorecard<8, true>(s, grid, threads, pred, target, target_levels, clim, clim_kind, lat_weight, bits, R, ws, H, W, slabs);
  const int rc = pangu_launch_status();
  if (rc != PANGU_OK) return rc;
  const int per_plane = R * SCD_SUMS;
  const long long outs = (long long)planes * per_plane;
  hipLaunchKernelGGL(scorecard_final_kernel, dim3((unsigned)((outs + 255) / 256)), dim3(256), 0, s, ws, sums, planes, slabs, per_plane);
  return pangu_launch_status();
}
