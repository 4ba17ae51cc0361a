// Padded token-id rows as K29 (edit_distance.hip) and K30 (lcs.hip) read them: the length of a row and the
// removal of `ignore_index` into a workspace (the body of both prep launches).
#pragma once

#include "tea_common.h"

namespace tea {

constexpr int kTokenPrepWaves = 4;  // rows per workgroup of a prep launch

// a row's length, clamped to [0, width]; row_len: of a wave-uniform row, as a scalar
__device__ __forceinline__ int clamped_len(const int64_t* lengths, int64_t pair, int64_t width) {
  const int64_t v = lengths ? lengths[pair] : width;
  return static_cast<int>(v < 0 ? 0 : (v > width ? width : v));
}
__device__ __forceinline__ int row_len(const int64_t* lengths, int64_t pair, int64_t width) {
  return __builtin_amdgcn_readfirstlane(clamped_len(lengths, pair, width));
}

// One wave per row and side, kTokenPrepWaves rows per workgroup: rows 0 .. b - 1 are `input` ([b, li]), rows
// b .. 2 b - 1 `target` ([b, lt]).  The kept tokens of a row (its first `len`, without those equal to
// `ignore_index`) go to the front of the row's place in `ws_tokens` (input rows, then target rows, at
// their own widths) by ballot and popcount prefix, 64 at a time; ws_lengths[row] takes their number.
template <typename T>
__device__ __forceinline__ void compact_token_rows(const void* input, const void* target, const int64_t* input_lengths,
                                                   const int64_t* target_lengths, int64_t b, int64_t li, int64_t lt,
                                                   int64_t ignore_index, void* ws_tokens, int64_t* ws_lengths) {
  const int64_t row = static_cast<int64_t>(blockIdx.x) * kTokenPrepWaves + wave_id();
  if (row >= 2 * b) return;
  const bool tg = row >= b;
  const int64_t pair = tg ? row - b : row, width = tg ? lt : li;
  const int len = row_len(tg ? target_lengths : input_lengths, pair, width);
  const T* src = static_cast<const T*>(tg ? target : input) + pair * width;
  T* dst = static_cast<T*>(ws_tokens) + (tg ? b * li : 0) + pair * width;
  const int lane = lane_id();
  int kept = 0;
  for (int base = 0; base < len; base += kWave) {
    const int idx = base + lane;
    const T v = idx < len ? src[idx] : T(0);
    const bool keep = idx < len && static_cast<int64_t>(v) != ignore_index;
    const unsigned long long mask = __ballot(keep);
    if (keep) dst[kept + __popcll(mask & ((1ull << lane) - 1ull))] = v;
    kept += __popcll(mask);
  }
  if (lane == 0) ws_lengths[row] = kept;
}

}  // namespace tea
