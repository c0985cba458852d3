// The static bitonic sorting network over P register-resident floats (P a power of two), shared by the ensemble stats kernel
// (ensemble.hip) and the quantile kernel (quantile.hip).  P log2 P (log2 P + 1) / 4 compare-exchanges, each one v_min_f32 and one
// v_max_f32; every index is a compile-time constant, so the array stays in VGPRs.  fminf / fmaxf return the other operand when one
// is NaN: a NaN does not survive the network (callers that care detect it before sorting); +-inf sort to the ends.
#pragma once

// one stage (k, j) of the bitonic network, then the next; all indices compile-time
template <int P, int K, int J>
__device__ __forceinline__ void bitonic_stage(float (&v)[P]) {
#pragma unroll
  for (int i = 0; i < P; ++i) {
    constexpr int j = J;
    const int l = i ^ j;
    if (l > i) {
      const float a = v[i], b = v[l];
      if ((i & K) == 0) { v[i] = fminf(a, b); v[l] = fmaxf(a, b); }
      else { v[i] = fmaxf(a, b); v[l] = fminf(a, b); }
    }
  }
  if constexpr (J > 1) bitonic_stage<P, K, J / 2>(v);
  else if constexpr (K < P) bitonic_stage<P, 2 * K, K>(v);
}

template <int P>
__device__ __forceinline__ void bitonic_sort(float (&v)[P]) {
  bitonic_stage<P, 2, 1>(v);
}
