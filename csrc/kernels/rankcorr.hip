// K14: Spearman rank correlation of [rows, n] operand pairs, after K3a has sorted both operands
// (stacked as [2 rows, n]: the rows of the first operand, then those of the second).
//
// Replaces the ATen form (functional/regression/spearman.py): two torch.sort, four searchsorted,
// about ten elementwise passes over int64 ranks and three reductions.  Here, per operand, K3a
// (radix.hip) gives the descending sorted row and its int32 source permutation, and three kernels
// finish the job:
//
//   rank_center   for each sorted position p the tie run [lo, hi) of its key by float equality
//                 (so -0.0 == +0.0; +-inf are ordinary values), and the centred doubled rank
//                 c = n - lo - hi  (= 2 rank - (n + 1), rank the 1-based tie-averaged ascending
//                 rank) as int32 to c[row][order[p]].  A block stages its span of the sorted row in
//                 LDS: a key that differs from both neighbours is a run of one; otherwise the run's
//                 ends come from a binary search of the span in LDS.  Runs that leave the span are
//                 resolved once per block, by a binary search of the sorted row on each side.  The
//                 thread that owns position 0 stores the row's NaN flag (K3a puts every NaN first).
//   rank_moments  reads cx, cy in source order (16-byte loads; the rows of `c` are pitched to 16
//                 bytes) and writes sum cx cy, sum cx^2, sum cy^2 per block as FP64 partials of
//                 fixed spans, every factor converted to double before the multiply.
//   rank_finish   one wave per row adds the partials in a fixed order and stores
//                 sxy / sqrt(sxx syy) as float32; NaN for a NaN flag, n < 2, a zero denominator or
//                 a faulted sort.
//
// No atomics, no waiting between workgroups, no host read.  Every loop is bounded by the span or
// by log2 n: a row that holds NaN (whose compares are not monotone) still ends every search inside
// the row and only produces ranks nobody uses.  For n <= 2^17 all three sums are integers below
// 2^53 and therefore exact in any order.
#include <hip/hip_runtime.h>

#include <cstdint>

#include "tea_kernels.h"

namespace tea {
namespace {

constexpr int kBlock = 256;
constexpr int kCPer = kRankCenterSpan / kBlock;              // sorted positions per thread
constexpr int kMVec = kRankMomentsSpan / (kBlock * 4);       // int4 loads per thread and operand
static_assert(kRankCenterSpan % kBlock == 0 && kRankMomentsSpan % (kBlock * 4) == 0, "span / block");

__global__ __launch_bounds__(kBlock) void rank_center_kernel(RankCorrArgs a, int64_t tiles) {
  __shared__ float sk[kRankCenterSpan];
  __shared__ int64_t edge[2];
  const int64_t tile = blockIdx.x % tiles;
  const int64_t orow = blockIdx.x / tiles;  // operand * rows + row
  const float* s = a.sorted + orow * a.n;
  const int32_t* o = a.order + orow * a.n;
  int32_t* c = a.c + orow * a.pitch;
  const int64_t n = a.n;
  const int64_t lo0 = tile * kRankCenterSpan;
  const int len = static_cast<int>(min(static_cast<int64_t>(kRankCenterSpan), n - lo0));

  float k[kCPer];
  int32_t src[kCPer];
#pragma unroll
  for (int u = 0; u < kCPer; ++u) {  // clamped (always valid) addresses, masked below
    const int i = u * kBlock + threadIdx.x;
    const int ic = i < len ? i : len - 1;
    k[u] = s[lo0 + ic];
    src[u] = o[lo0 + ic];
    if (i < len) sk[i] = k[u];
  }
  const float kf = s[lo0], kl = s[lo0 + len - 1];
  if (threadIdx.x == 0) {
    if (tile == 0) a.nan_flag[orow] = kf != kf ? 1 : 0;
    // where the run of the span's first key starts in the row: the first index whose key is not
    // greater, searched in [0, lo0 - 1] when the neighbour on the left ties
    int64_t L = lo0;
    if (lo0 > 0 && s[lo0 - 1] == kf) {
      L = 0;
      int64_t R = lo0 - 1;
      while (L < R) {
        const int64_t mid = L + ((R - L) >> 1);
        if (s[mid] > kf) L = mid + 1; else R = mid;
      }
    }
    edge[0] = L;
  }
  if (threadIdx.x == 64) {
    // where the run of the span's last key ends: the first index whose key is smaller (n if none)
    int64_t L = lo0 + len;
    if (L < n && s[L] == kl) {
      L = L + 1;
      int64_t R = n;
      while (L < R) {
        const int64_t mid = L + ((R - L) >> 1);
        if (s[mid] < kl) R = mid; else L = mid + 1;
      }
    }
    edge[1] = L;
  }
  __syncthreads();
  const int64_t glo = edge[0], ghi = edge[1];
#pragma unroll
  for (int u = 0; u < kCPer; ++u) {
    const int i = u * kBlock + threadIdx.x;
    if (i >= len) continue;
    const float key = k[u];
    int l = i, h = i + 1;
    if (i > 0 && sk[i - 1] == key) {  // first index of the span whose key is not greater
      int L = 0, R = i - 1;
      while (L < R) {
        const int mid = (L + R) >> 1;
        if (sk[mid] > key) L = mid + 1; else R = mid;
      }
      l = L;
    }
    if (i + 1 < len && sk[i + 1] == key) {  // first index of the span whose key is smaller
      int L = i + 2, R = len;
      while (L < R) {
        const int mid = (L + R) >> 1;
        if (sk[mid] < key) R = mid; else L = mid + 1;
      }
      h = L;
    }
    const int64_t lo = l == 0 ? glo : lo0 + l;
    const int64_t hi = h == len ? ghi : lo0 + h;
    // K3a's permutation holds 0 .. n - 1; a faulted sort (RankCorrArgs::sort_fault) may not
    if (static_cast<uint32_t>(src[u]) < static_cast<uint64_t>(n)) c[src[u]] = static_cast<int32_t>(n - lo - hi);
  }
}

__global__ __launch_bounds__(kBlock) void rank_moments_kernel(RankCorrArgs a, int blocks, int64_t span) {
  const int64_t row = blockIdx.x / blocks;
  const int b = static_cast<int>(blockIdx.x - row * blocks);
  const int32_t* cx = a.c + row * a.pitch;  // 16-byte aligned rows (pitch % 4 == 0)
  const int32_t* cy = a.c + (a.rows + row) * a.pitch;
  const int64_t lo = static_cast<int64_t>(b) * span;  // span % kRankMomentsSpan == 0
  const int64_t hi = min(a.n, lo + span);
  const int64_t vend = hi > lo ? lo + ((hi - lo) & ~int64_t{3}) : lo;
  double sxy = 0.0, sxx = 0.0, syy = 0.0;
  for (int64_t base = lo; base < vend; base += kRankMomentsSpan) {
    int4 x[kMVec], y[kMVec];
#pragma unroll
    for (int u = 0; u < kMVec; ++u) {  // clamped (always valid) addresses, masked below
      const int64_t i = base + (static_cast<int64_t>(u) * kBlock + threadIdx.x) * 4;
      const int64_t ic = i < vend ? i : lo;
      x[u] = *reinterpret_cast<const int4*>(cx + ic);
      y[u] = *reinterpret_cast<const int4*>(cy + ic);
    }
#pragma unroll
    for (int u = 0; u < kMVec; ++u) {
      const int64_t i = base + (static_cast<int64_t>(u) * kBlock + threadIdx.x) * 4;
      if (i >= vend) continue;
      const double x0 = x[u].x, x1 = x[u].y, x2 = x[u].z, x3 = x[u].w;
      const double y0 = y[u].x, y1 = y[u].y, y2 = y[u].z, y3 = y[u].w;
      sxy += (x0 * y0 + x1 * y1) + (x2 * y2 + x3 * y3);
      sxx += (x0 * x0 + x1 * x1) + (x2 * x2 + x3 * x3);
      syy += (y0 * y0 + y1 * y1) + (y2 * y2 + y3 * y3);
    }
  }
  {  // scalar tail: at most 3 elements
    const int64_t i = vend + threadIdx.x;
    if (i < hi) {
      const double x = cx[i], y = cy[i];
      sxy += x * y;
      sxx += x * x;
      syy += y * y;
    }
  }
  // block sums: wave shuffles, then the 4 wave totals in order
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) {
    sxy += __shfl_xor(sxy, off, 64);
    sxx += __shfl_xor(sxx, off, 64);
    syy += __shfl_xor(syy, off, 64);
  }
  __shared__ double w[3][kBlock / 64];
  if ((threadIdx.x & 63) == 0) {
    w[0][threadIdx.x >> 6] = sxy;
    w[1][threadIdx.x >> 6] = sxx;
    w[2][threadIdx.x >> 6] = syy;
  }
  __syncthreads();
  if (threadIdx.x < 3) {
    const double* v = w[threadIdx.x];
    a.part[static_cast<int64_t>(blockIdx.x) * 3 + threadIdx.x] = (v[0] + v[1]) + (v[2] + v[3]);
  }
}

__global__ __launch_bounds__(64) void rank_finish_kernel(RankCorrArgs a, int blocks) {
  const int64_t row = blockIdx.x;
  const double* p = a.part + row * blocks * 3;
  double sxy = 0.0, sxx = 0.0, syy = 0.0;
  for (int b = threadIdx.x; b < blocks; b += 64) {
    sxy += p[b * 3 + 0];
    sxx += p[b * 3 + 1];
    syy += p[b * 3 + 2];
  }
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) {
    sxy += __shfl_xor(sxy, off, 64);
    sxx += __shfl_xor(sxx, off, 64);
    syy += __shfl_xor(syy, off, 64);
  }
  if (threadIdx.x == 0) {
    const bool nan = a.nan_flag[row] != 0 || a.nan_flag[a.rows + row] != 0 ||
                     (a.sort_fault != nullptr && *a.sort_fault != 0u);
    const bool defined = !nan && a.n >= 2 && sxx != 0.0 && syy != 0.0;
    a.out[row] = defined ? static_cast<float>(sxy / sqrt(sxx * syy)) : __uint_as_float(0x7fc00000u);
  }
}

}  // namespace

int64_t rank_corr_pitch(int64_t n) { return (n + 3) & ~int64_t{3}; }

int rank_moments_blocks(int64_t n) {
  const int64_t b = (n + kRankMomentsSpan - 1) / kRankMomentsSpan;
  return static_cast<int>(b < 1 ? 1 : (b > 256 ? 256 : b));
}

int launch_rank_corr(const RankCorrArgs& a, hipStream_t stream) {
  if (a.rows <= 0) return 0;
  if (a.n < 2 || a.n >= (int64_t{1} << 31) || a.pitch < a.n || (a.pitch & 3) != 0 ||
      (reinterpret_cast<uintptr_t>(a.c) & 15) != 0)
    return 1;
  const int64_t tiles = (a.n + kRankCenterSpan - 1) / kRankCenterSpan;
  const int blocks = rank_moments_blocks(a.n);
  const int64_t span =
      ((a.n + blocks - 1) / blocks + kRankMomentsSpan - 1) / kRankMomentsSpan * kRankMomentsSpan;
  if (2 * a.rows * tiles >= (int64_t{1} << 31) || a.rows * blocks >= (int64_t{1} << 31)) return 1;
  hipLaunchKernelGGL(rank_center_kernel, dim3(static_cast<unsigned>(2 * a.rows * tiles)), dim3(kBlock), 0, stream, a,
                     tiles);
  hipLaunchKernelGGL(rank_moments_kernel, dim3(static_cast<unsigned>(a.rows * blocks)), dim3(kBlock), 0, stream, a,
                     blocks, span);
  hipLaunchKernelGGL(rank_finish_kernel, dim3(static_cast<unsigned>(a.rows)), dim3(64), 0, stream, a, blocks);
  return hipGetLastError() == hipSuccess ? 0 : 2;
}

}  // namespace tea
