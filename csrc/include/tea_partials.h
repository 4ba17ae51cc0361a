// The finish half of the per-block-partials plan (device only): blocks write partials, a small
// second launch adds them in a fixed order, so a result is bit-identical from run to run.  Every
// sum below has ONE association order, which is part of each caller's behaviour.  The block sums
// inside the streaming kernels stay with their units: through a shared K-value block sum
// corr_row_kernel and kid_gram_kernel no longer compile to the same instructions, and the units
// that add four wave totals pairwise, (w0 + w1) + (w2 + w3), keep that line of their own
// (profiles/partials_dedup_codegen.txt).
#pragma once

#include "tea_common.h"

namespace tea {

// Ordered sum of src[k * stride] over the run k in [begin, end).  An empty run returns Acc's zero
// and reads nothing.  16 unconditional loads in flight (clamped to the run's last element, counted
// as 0 past it), then their adds in order: a load per add waits one round trip each, 17.6 us for
// 1024 blocks of 15 bins against 9.5 (profiles/calibration_r11.json).
template <typename Acc, typename T>
__device__ __forceinline__ Acc run_fold(const T* src, int64_t stride, int begin, int end) {
  Acc acc = Acc(0);
  for (int k = begin; k < end; k += 16) {
    T v[16];
#pragma unroll
    for (int i = 0; i < 16; ++i) v[i] = src[static_cast<int64_t>(min(k + i, end - 1)) * stride];
#pragma unroll
    for (int i = 0; i < 16; ++i) acc += k + i < end ? v[i] : T(0);
  }
  return acc;
}

// One wave's sums of K interleaved rows of n partials, value k of partial i at
// p[i * stride + k * vstride] (indexed in the type of n): lane l adds partials l, l + 64, ... in
// that order, then the butterfly of wave_sum, so every lane holds the K totals.
template <int K, typename Acc, typename T, typename N>
__device__ __forceinline__ void wave_strided_sum(const T* p, N n, N stride, N vstride, Acc (&s)[K]) {
#pragma unroll
  for (int k = 0; k < K; ++k) s[k] = Acc(0);
  for (N i = lane_id(); i < n; i += kWave) {
#pragma unroll
    for (int k = 0; k < K; ++k) s[k] += static_cast<Acc>(p[i * stride + k * vstride]);
  }
#pragma unroll
  for (int k = 0; k < K; ++k) s[k] = wave_sum(s[k]);
}
template <typename T, typename N>
__device__ __forceinline__ T wave_strided_sum(const T* p, N n) {
  T s[1];
  wave_strided_sum(p, n, N(1), N(0), s);
  return s[0];
}

}  // namespace tea
