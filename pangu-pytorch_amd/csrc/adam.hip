// Adam for the whole model in ONE launch (reference finetune_fully.py:121: torch.optim.Adam(lr=5e-6, weight_decay=3e-6); the step of
// models/pangu_sample.py:75).  torch's fused Adam walks the 223 tensors in 14 launches of at most 320 workgroups each (its tensor-list
// metadata caps a launch): 1.8 ms for 7.7 GB = 4.3 TB/s, about one workgroup per CU.  Here a device-resident job table describes
// every (param, grad, exp_avg, exp_avg_sq) quadruple and one launch of ~67 000 workgroups streams them.
//
// The arithmetic follows ATen/native/cuda/fused_adam_utils.cuh (adam_math, ADAM_MODE::ORIGINAL, no amsgrad / maximize / grad
// scaling) operation by operation, INCLUDING its mixed precision -- lr, betas, weight_decay, eps are doubles there, so the decay
// term, both moment updates, the step size and the denominator are evaluated in double and rounded to float where that code assigns
// to its float variables -- so the result is bit-identical to torch.optim.Adam(fused=True) (tests/test_gpu_extras.py).
//
// Job table: (n_jobs + 1) rows of 8 int64: [0] param [1] grad (0 = a zero gradient, never read) [2] exp_avg [3] exp_avg_sq (float*)  [4] bf16 image of the updated
// param or 0  [5] n  [6] 0 = use the launch's bias corrections (every tensor at the same step count: the table then only changes
// when a pointer does), else float bits of bias_correction1 | float bits of sqrt(bias_correction2) << 32  [7] first block; the last
// row is a sentinel whose [7] = total blocks.  4096 elements per block.
//
// Gradient clipping / accumulation scale / non-finite skip ride on the same table (train.HipAdam(max_grad_norm=, skip_nonfinite=),
// step(grad_scale=)): grad_sumsq_kernel reads every gradient once (one double partial per table block, fixed summation order, no
// atomics: bit-identical from run to run), clip_state_kernel folds the partials of all groups into a 32-byte device record
// (ClipState) and adam_multi_kernel<true> multiplies each gradient by the record's multiplier on its way into adam_one -- the
// gradients themselves are never written, and the host never waits for the norm.
#include "common.h"

namespace {

constexpr int ADAM_CHUNK = 4096;
typedef unsigned short u16;
typedef unsigned int u32x2 __attribute__((ext_vector_type(2)));

__device__ inline void adam_one(float& param, float g, float& exp_avg, float& exp_avg_sq, double lr, double beta1, double beta2,
                                double weight_decay, double eps, float bc1, float bc2_sqrt) {
  float grad = g;
  if (weight_decay != 0) grad = (float)((double)grad + (double)param * weight_decay);      // grad += param * weight_decay
  exp_avg = (float)(beta1 * (double)exp_avg + (1 - beta1) * (double)grad);
  exp_avg_sq = (float)(beta2 * (double)exp_avg_sq + (1 - beta2) * (double)grad * (double)grad);
  const float step_size = (float)(lr / (double)bc1);
  const float denom = (float)((double)(sqrtf(exp_avg_sq) / bc2_sqrt) + eps);
  param -= step_size * exp_avg / denom;
}

// The device record of one clipped / scaled / guarded step (pangu_hip.h: pangu_grad_clip_state)
struct ClipState {
  float norm;                // fl32(grad_scale * sqrt(sum of squares)): the pre-clip norm of the scaled gradient
  float multiplier;          // what every gradient is multiplied by on its way into Adam
  int skip;                  // 1: this step leaves parameters and moments alone
  int pad_;
  long long skipped_total;   // steps skipped so far
};
static_assert(sizeof(ClipState) == 24, "ClipState layout is part of the C ABI");

// the job that table block `b` belongs to (rows are sorted by first block)
__device__ inline const long long* adam_job_of(const long long* __restrict__ jobs, int n_jobs, long long b) {
  int lo = 0, hi = n_jobs;
  while (hi - lo > 1) {
    const int mid = (lo + hi) >> 1;
    if (jobs[(size_t)mid * 8 + 7] <= b) lo = mid; else hi = mid;
  }
  return jobs + (size_t)lo * 8;
}

// lane -> wave -> workgroup, always in the same order; the total is valid in thread 0
__device__ inline double block_sum_f64(double v, double* lds) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off, 64);
  if ((threadIdx.x & 63) == 0) lds[threadIdx.x >> 6] = v;
  __syncthreads();
  return ((lds[0] + lds[1]) + lds[2]) + lds[3];
}

// Stage 1: partial[b] = sum of g^2 over table block b, in double (4 B read per element; a cvt and an fma in fp64 per element)
__global__ __launch_bounds__(256) void grad_sumsq_kernel(const long long* __restrict__ jobs, int n_jobs, double* __restrict__ partial) {
  __shared__ double lds[4];
  const long long b = blockIdx.x;
  const long long* J = adam_job_of(jobs, n_jobs, b);
  const float* __restrict__ G = reinterpret_cast<const float*>(J[1]);
  const long long n = J[5];
  const long long base = (b - J[7]) * ADAM_CHUNK;
  const bool vec = (n & 3) == 0;
  double acc = 0.0;
  if (G) {                                     // workgroup-uniform; a null gradient is all zeros and is never read
#pragma unroll
    for (int k = 0; k < ADAM_CHUNK / 1024; ++k) {
      const long long i = base + k * 1024 + threadIdx.x * 4;
      if (vec && i + 4 <= n) {
        const f32x4 g = *reinterpret_cast<const f32x4*>(G + i);
#pragma unroll
        for (int e = 0; e < 4; ++e) acc += (double)g[e] * (double)g[e];
      } else {
        for (long long j = i; j < n && j < i + 4; ++j) acc += (double)G[j] * (double)G[j];
      }
    }
  }
  const double tot = block_sum_f64(acc, lds);
  if (threadIdx.x == 0) partial[b] = tot;
}

// Stage 2 (one workgroup): lane t adds partials t, t + 256, ... in ascending order, the lanes combine as in stage 1
__global__ __launch_bounds__(256) void clip_state_kernel(const double* __restrict__ partial, long long n_partial, ClipState* __restrict__ st,
                                                         int clip, float max_norm, double grad_scale, int skip_nonfinite) {
  __shared__ double lds[4];
  double acc = 0.0;
  for (long long i = threadIdx.x; i < n_partial; i += 256) acc += partial[i];
  const double sumsq = block_sum_f64(acc, lds);
  if (threadIdx.x != 0) return;
  const float norm = (float)(grad_scale * sqrt(sumsq));
  float mult = (float)grad_scale;
  if (clip) {
    // torch.nn.utils.clip_grad_norm_ in fp32 on the fp32 norm: clamp(max_norm / (norm + 1e-6), max=1), a NaN stays a NaN
    float denom = norm + 1e-6f;
    asm volatile("" : "+v"(denom));
    float coef = max_norm / denom;
    coef = coef > 1.0f ? 1.0f : coef;
    asm volatile("" : "+v"(coef));
    mult = mult * coef;
  }
  const bool nonfinite = !__builtin_isfinite(sumsq);       // NaN or Inf (torch's error_if_nonfinite criterion, on the sum)
  const int skip = (skip_nonfinite && nonfinite) ? 1 : 0;
  st->norm = norm;
  st->multiplier = mult;
  st->skip = skip;
  st->skipped_total += skip;
}

// SCALED: the gradient is multiplied by st->multiplier (rounded to float) before adam_one; st->skip leaves P, M, V alone
template <bool SCALED>
__global__ __launch_bounds__(256) void adam_multi_kernel(const long long* __restrict__ jobs, int n_jobs, double lr, double beta1,
                                                         double beta2, double weight_decay, double eps, float bc1_all,
                                                         float bc2s_all, const ClipState* __restrict__ st) {
  const long long b = blockIdx.x;
  const long long* J = adam_job_of(jobs, n_jobs, b);
  float* __restrict__ P = reinterpret_cast<float*>(J[0]);
  const float* __restrict__ G = reinterpret_cast<const float*>(J[1]);
  float* __restrict__ M = reinterpret_cast<float*>(J[2]);
  float* __restrict__ V = reinterpret_cast<float*>(J[3]);
  u16* __restrict__ S = reinterpret_cast<u16*>(J[4]);
  const long long n = J[5];
  // bias corrections: per job when the tensors are at different step counts (row field != 0), else the launch's
  const float bc1 = J[6] ? __builtin_bit_cast(float, (unsigned)(J[6] & 0xFFFFFFFFll)) : bc1_all;
  const float bc2s = J[6] ? __builtin_bit_cast(float, (unsigned)((unsigned long long)J[6] >> 32)) : bc2s_all;
  const long long base = (b - J[7]) * ADAM_CHUNK;
  const bool vec = (n & 3) == 0;
  float mult = 1.f;
  if constexpr (SCALED) {
    mult = st->multiplier;
    if (st->skip) {                            // workgroup-uniform (one record per launch)
      // the caller marks imaged parameters fresh without knowing the outcome: the image is re-made from the unchanged parameter
      if (!S) return;
#pragma unroll
      for (int k = 0; k < ADAM_CHUNK / 1024; ++k) {
        const long long i = base + k * 1024 + threadIdx.x * 4;
        if (vec && i + 4 <= n) {
          const f32x4 p = *reinterpret_cast<const f32x4*>(P + i);
          *reinterpret_cast<u32x2*>(S + i) = u32x2{pack_bf16x2(p[0], p[1]), pack_bf16x2(p[2], p[3])};
        } else {
          for (long long j = i; j < n && j < i + 4; ++j) S[j] = __builtin_bit_cast(u16, (__bf16)P[j]);
        }
      }
      return;
    }
  }
  // g * multiplier is rounded to float before it enters adam_one, as a gradient scaled in place would be (the empty asm keeps
  // hipcc from contracting the product into adam_one's first multiply-add)
  auto scaled = [&](float g) {
    if constexpr (SCALED) {
      g *= mult;
      asm volatile("" : "+v"(g));
    }
    return g;
  };
#pragma unroll
  for (int k = 0; k < ADAM_CHUNK / 1024; ++k) {
    const long long i = base + k * 1024 + threadIdx.x * 4;
    if (vec && i + 4 <= n) {
      f32x4 p = *reinterpret_cast<const f32x4*>(P + i);
      const f32x4 g = G ? __builtin_nontemporal_load(reinterpret_cast<const f32x4*>(G + i)) : f32x4{0.f, 0.f, 0.f, 0.f};
      f32x4 m = *reinterpret_cast<const f32x4*>(M + i);
      f32x4 v = *reinterpret_cast<const f32x4*>(V + i);
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        float pe = p[e], me = m[e], ve = v[e];
        adam_one(pe, scaled(g[e]), me, ve, lr, beta1, beta2, weight_decay, eps, bc1, bc2s);
        p[e] = pe; m[e] = me; v[e] = ve;
      }
      *reinterpret_cast<f32x4*>(P + i) = p;
      *reinterpret_cast<f32x4*>(M + i) = m;
      *reinterpret_cast<f32x4*>(V + i) = v;
      if (S) *reinterpret_cast<u32x2*>(S + i) = u32x2{pack_bf16x2(p[0], p[1]), pack_bf16x2(p[2], p[3])};
    } else {
      for (long long j = i; j < n && j < i + 4; ++j) {
        float pe = P[j], me = M[j], ve = V[j];
        adam_one(pe, scaled(G ? G[j] : 0.f), me, ve, lr, beta1, beta2, weight_decay, eps, bc1, bc2s);
        P[j] = pe; M[j] = me; V[j] = ve;
        if (S) S[j] = __builtin_bit_cast(u16, (__bf16)pe);
      }
    }
  }
}

bool adam_args_ok(double lr, double beta1, double beta2, double weight_decay, double eps) {
  return lr >= 0 && beta1 >= 0 && beta1 < 1 && beta2 >= 0 && beta2 < 1 && eps >= 0 && weight_decay >= 0;
}

}  // namespace

extern "C" int pangu_adam_step_multi(pangu_stream_t stream, const void* jobs, int n_jobs, long long total_blocks, double lr,
                                     double beta1, double beta2, double weight_decay, double eps, float bias_correction1,
                                     float bias_correction2_sqrt) {
  if (!jobs) return PANGU_E_NULL;
  if (n_jobs <= 0 || total_blocks <= 0 || total_blocks > 0x7FFFFFFFll) return PANGU_E_SHAPE;
  if (!adam_args_ok(lr, beta1, beta2, weight_decay, eps)) return PANGU_E_ARG;
  hipLaunchKernelGGL(adam_multi_kernel<false>, dim3((unsigned)total_blocks), dim3(256), 0, (hipStream_t)stream,
                     reinterpret_cast<const long long*>(jobs), n_jobs, lr, beta1, beta2, weight_decay, eps, bias_correction1,
                     bias_correction2_sqrt, (const ClipState*)nullptr);
  return pangu_launch_status();
}

extern "C" int pangu_adam_step_multi_scaled(pangu_stream_t stream, const void* jobs, int n_jobs, long long total_blocks, double lr,
                                            double beta1, double beta2, double weight_decay, double eps, float bias_correction1,
                                            float bias_correction2_sqrt, const void* state) {
  if (!jobs || !state) return PANGU_E_NULL;
  if (n_jobs <= 0 || total_blocks <= 0 || total_blocks > 0x7FFFFFFFll) return PANGU_E_SHAPE;
  if (!adam_args_ok(lr, beta1, beta2, weight_decay, eps)) return PANGU_E_ARG;
  hipLaunchKernelGGL(adam_multi_kernel<true>, dim3((unsigned)total_blocks), dim3(256), 0, (hipStream_t)stream,
                     reinterpret_cast<const long long*>(jobs), n_jobs, lr, beta1, beta2, weight_decay, eps, bias_correction1,
                     bias_correction2_sqrt, reinterpret_cast<const ClipState*>(state));
  return pangu_launch_status();
}

extern "C" int pangu_grad_sumsq_multi(pangu_stream_t stream, const void* jobs, int n_jobs, long long total_blocks, void* partials) {
  if (!jobs || !partials) return PANGU_E_NULL;
  if (n_jobs <= 0 || total_blocks <= 0 || total_blocks > 0x7FFFFFFFll) return PANGU_E_SHAPE;
  hipLaunchKernelGGL(grad_sumsq_kernel, dim3((unsigned)total_blocks), dim3(256), 0, (hipStream_t)stream,
                     reinterpret_cast<const long long*>(jobs), n_jobs, reinterpret_cast<double*>(partials));
  return pangu_launch_status();
}

extern "C" int pangu_grad_clip_state(pangu_stream_t stream, const void* partials, long long n_partials, void* state, int clip,
                                     double max_norm, double grad_scale, int skip_nonfinite) {
  if (!partials || !state) return PANGU_E_NULL;
  if (n_partials <= 0 || n_partials > 0x7FFFFFFFll) return PANGU_E_SHAPE;
  if ((clip && !(max_norm > 0)) || !(grad_scale > 0 && grad_scale <= 1.7976931348623157e308)) return PANGU_E_ARG;
  hipLaunchKernelGGL(clip_state_kernel, dim3(1), dim3(256), 0, (hipStream_t)stream, reinterpret_cast<const double*>(partials),
                     n_partials, reinterpret_cast<ClipState*>(state), clip ? 1 : 0, (float)max_norm, grad_scale,
                     skip_nonfinite ? 1 : 0);
  return pangu_launch_status();
}
