// K19: Kendall rank correlation (tau-b / tau-c) of [rows, n] operand pairs, as a ratio of exact
// 64-bit integers (docs/parity.md, "Not in the reference").
//
// Replaces the ATen form (functional/regression/kendall.py): two torch.sort, run boundaries and a
// log2 n-level loop of searchsorted plus a re-sort of the whole sample.  Here K3a (radix.hip)
// sorts `target` descending with its source permutation, then `input` (gathered into that order)
// descending and stable with the tie-run start `s` of each item's target as its payload; the
// number of discordant pairs Q is the number of strict inversions (i < j, s_i > s_j) of the
// carried sequence.  Five kernels do the rest:
//
//   kendall_prepare  on the sorted target: the start of every position's tie run (float equality,
//                    so -0.0 == +0.0; +-inf ordinary) -> s[k]; the gathered input
//                    xg[k] = x[perm[k]] (K3a folds -0.0 into +0.0 in its keys, f2key_desc in
//                    radix.hip, so the second sort keeps a -0.0 / +0.0 tie group whole and in
//                    stable order: s stays sorted inside it, and no canonical zero is needed
//                    here); per-block partials of n2 = sum (k - start_k) and my = run starts.
//   kendall_ties     on the sorted input and the carried s: n1 and mx the same way, and n3 from
//                    the joint runs (input and s both equal), which are contiguous because s is
//                    non-decreasing inside an input tie run.
//   kendall_tile     sorts tiles of kKendallTile carried values ascending in LDS by log2(tile)
//                    rounds of merge-by-rank (every element finds its place in the partner run by
//                    a binary search) and counts each round's inversions.
//   kendall_merge    one launch per level: a block owns one kKendallTile-wide output tile of one
//                    (A, B) run pair, cut out by two merge-path diagonals (ties A-first), and adds
//                    for every staged b the number of a > b.
//   kendall_finish   one wave per task adds the partials and stores the value and the six counts.
//
// A block spans a tile, resolves runs in LDS and resolves a run that leaves its span by a binary
// search of the sorted row (as K14's rank_center).  Every partial is a 64-bit integer, so any
// order of addition is exact; each is stored by the one block that owns it, without atomics.  No
// waiting between workgroups, no host read, every loop bounded by the tile or by log2 n: a row
// that holds NaN (whose compares are not monotone) still ends every search inside the row and only
// produces counts nobody uses.
#include <hip/hip_runtime.h>

#include <cstdint>

#include "tea_kernels.h"
#include "tea_partials.h"

namespace tea {
namespace {

constexpr int kBlock = 256;
constexpr int kT = kKendallTile;
constexpr int kPer = kT / kBlock;  // positions per thread
static_assert(kT % kBlock == 0 && (kT & (kT - 1)) == 0, "tile: a power of two, a multiple of the block");

using u64 = unsigned long long;

// block total of v in every thread of wave 0 (callers read it in thread 0)
__device__ __forceinline__ u64 block_sum(u64 v, u64* w) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off, 64);
  if ((threadIdx.x & 63) == 0) w[threadIdx.x >> 6] = v;
  __syncthreads();
  return (w[0] + w[1]) + (w[2] + w[3]);
}

// x desc, then s asc: whether (xa, sa) sorts strictly before (xb, sb)
__device__ __forceinline__ bool joint_before(float xa, int32_t sa, float xb, int32_t sb) {
  return xa > xb || (xa == xb && sa < sb);
}

__global__ __launch_bounds__(kBlock) void kendall_prepare_kernel(KendallPrepareArgs a, int64_t tiles) {
  __shared__ float sk[kT];
  __shared__ int64_t edge;
  __shared__ u64 w[2][kBlock / 64];
  const int64_t tile = blockIdx.x % tiles;
  const int64_t row = blockIdx.x / tiles;
  const int64_t n = a.n;
  const float* s = a.sorted + row * n;
  const int32_t* o = a.order + row * n;
  const float* x = a.x + row * n;
  const int64_t lo0 = tile * kT;
  const int len = static_cast<int>(min(static_cast<int64_t>(kT), n - lo0));

  float k[kPer], xv[kPer];
#pragma unroll
  for (int u = 0; u < kPer; ++u) {  // clamped (always valid) addresses, masked below
    const int i = u * kBlock + threadIdx.x;
    const int ic = i < len ? i : len - 1;
    k[u] = s[lo0 + ic];
    // K3a's permutation holds 0 .. n - 1; a faulted sort (sort_fault) may not
    const uint32_t src = static_cast<uint32_t>(o[lo0 + ic]);
    xv[u] = x[src < static_cast<uint64_t>(n) ? src : 0u];
    if (i < len) sk[i] = k[u];
  }
  const float kf = s[lo0];
  if (threadIdx.x == 0) {
    if (tile == 0)
      a.flags[row * 2] = (kf != kf ? 1 : 0) | (a.sort_fault != nullptr && *a.sort_fault != 0u ? 2 : 0);
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
    edge = L;
  }
  __syncthreads();
  const int64_t glo = edge;
  u64 ties = 0, starts = 0;
#pragma unroll
  for (int u = 0; u < kPer; ++u) {
    const int i = u * kBlock + threadIdx.x;
    if (i >= len) continue;
    const float key = k[u];
    int l = i;
    if (i > 0 && sk[i - 1] == key) {  // first index of the span whose key is not greater
      int L = 0, R = i - 1;
      while (L < R) {
        const int mid = (L + R) >> 1;
        if (sk[mid] > key) L = mid + 1; else R = mid;
      }
      l = L;
    }
    const int64_t lo = l == 0 ? glo : lo0 + l;
    const int64_t pos = lo0 + i;
    a.s[row * n + pos] = static_cast<int32_t>(lo);
    a.xg[row * n + pos] = xv[u];
    ties += static_cast<u64>(pos - lo);
    starts += pos == lo ? 1u : 0u;
  }
  const u64 t0 = block_sum(ties, w[0]);
  const u64 t1 = block_sum(starts, w[1]);
  if (threadIdx.x == 0) {
    int64_t* p = a.part + row * 6 * tiles + tile;
    p[1 * tiles] = static_cast<int64_t>(t0);  // n2
    p[5 * tiles] = static_cast<int64_t>(t1);  // my
  }
}

__global__ __launch_bounds__(kBlock) void kendall_ties_kernel(KendallCountArgs a, int64_t tiles) {
  __shared__ float sk[kT];
  __shared__ int32_t ss[kT];
  __shared__ int64_t edge[2];
  __shared__ u64 w[3][kBlock / 64];
  const int64_t tile = blockIdx.x % tiles;
  const int64_t row = blockIdx.x / tiles;
  const int64_t n = a.n;
  const float* s = a.sorted + row * n;
  const int32_t* c = a.carried + row * n;
  const int64_t lo0 = tile * kT;
  const int len = static_cast<int>(min(static_cast<int64_t>(kT), n - lo0));

  float k[kPer];
  int32_t cv[kPer];
#pragma unroll
  for (int u = 0; u < kPer; ++u) {  // clamped (always valid) addresses, masked below
    const int i = u * kBlock + threadIdx.x;
    const int ic = i < len ? i : len - 1;
    k[u] = s[lo0 + ic];
    cv[u] = c[lo0 + ic];
    if (i < len) {
      sk[i] = k[u];
      ss[i] = cv[u];
    }
  }
  const float kf = s[lo0];
  const int32_t cf = c[lo0];
  if (threadIdx.x == 0) {
    if (tile == 0) a.flags[row * 2 + 1] = kf != kf ? 1 : 0;
    int64_t L = lo0;  // start of the input run of the span's first key
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
    int64_t L = lo0;  // start of the joint run of the span's first position
    if (lo0 > 0 && s[lo0 - 1] == kf && c[lo0 - 1] == cf) {
      L = 0;
      int64_t R = lo0 - 1;
      while (L < R) {
        const int64_t mid = L + ((R - L) >> 1);
        if (joint_before(s[mid], c[mid], kf, cf)) L = mid + 1; else R = mid;
      }
    }
    edge[1] = L;
  }
  __syncthreads();
  const int64_t glo = edge[0], gjo = edge[1];
  u64 ties = 0, starts = 0, joint = 0;
#pragma unroll
  for (int u = 0; u < kPer; ++u) {
    const int i = u * kBlock + threadIdx.x;
    if (i >= len) continue;
    const float key = k[u];
    const int32_t car = cv[u];
    int l = i, j = i;
    if (i > 0 && sk[i - 1] == key) {
      int L = 0, R = i - 1;
      while (L < R) {
        const int mid = (L + R) >> 1;
        if (sk[mid] > key) L = mid + 1; else R = mid;
      }
      l = L;
      if (ss[i - 1] == car) {
        L = 0, R = i - 1;
        while (L < R) {
          const int mid = (L + R) >> 1;
          if (joint_before(sk[mid], ss[mid], key, car)) L = mid + 1; else R = mid;
        }
        j = L;
      }
    }
    const int64_t pos = lo0 + i;
    const int64_t lo = l == 0 ? glo : lo0 + l;
    const int64_t jo = j == 0 ? gjo : lo0 + j;
    ties += static_cast<u64>(pos - lo);
    starts += pos == lo ? 1u : 0u;
    joint += static_cast<u64>(pos - jo);
  }
  const u64 t0 = block_sum(ties, w[0]);
  const u64 t1 = block_sum(starts, w[1]);
  const u64 t2 = block_sum(joint, w[2]);
  if (threadIdx.x == 0) {
    int64_t* p = a.part + row * 6 * tiles + tile;
    p[0 * tiles] = static_cast<int64_t>(t0);  // n1
    p[2 * tiles] = static_cast<int64_t>(t2);  // n3
    p[4 * tiles] = static_cast<int64_t>(t1);  // mx
  }
}

// sorts one tile of the carried values ascending and counts its strict inversions.  Positions past
// the row are INT32_MAX (every carried value is below n < 2^31): they sit at the end and stay there
__global__ __launch_bounds__(kBlock) void kendall_tile_kernel(KendallCountArgs a, int64_t tiles) {
  __shared__ int32_t buf[2][kT];
  __shared__ u64 w[kBlock / 64];
  const int64_t tile = blockIdx.x % tiles;
  const int64_t row = blockIdx.x / tiles;
  const int64_t n = a.n;
  const int32_t* c = a.carried + row * n;
  const int64_t lo0 = tile * kT;
  const int len = static_cast<int>(min(static_cast<int64_t>(kT), n - lo0));
#pragma unroll
  for (int u = 0; u < kPer; ++u) {
    const int i = u * kBlock + threadIdx.x;
    buf[0][i] = i < len ? c[lo0 + i] : INT32_MAX;
  }
  __syncthreads();
  u64 cnt = 0;
  int cur = 0;
  for (int L = 1; L < kT; L <<= 1) {
    const int32_t* in = buf[cur];
    int32_t* out = buf[cur ^ 1];
    // A left-run element goes behind the right run's elements below it, a right-run element behind
    // the left run's elements not above it; the rest of the left run are its inversions.  The
    // partner run has L = 2^k elements, so every search is the same k + 1 steps: the thread's
    // searches advance together, one LDS latency per step and not per step and element
    int32_t v[kPer];
    const int32_t* r[kPer];
    int pos[kPer];
    bool right[kPer];
#pragma unroll
    for (int u = 0; u < kPer; ++u) {
      const int i = u * kBlock + threadIdx.x;
      v[u] = in[i];
      right[u] = (i & L) != 0;
      r[u] = in + (i & ~(2 * L - 1)) + (right[u] ? 0 : L);
      pos[u] = 0;
    }
    for (int h = L >> 1; h > 0; h >>= 1) {
#pragma unroll
      for (int u = 0; u < kPer; ++u) {
        const int32_t x = r[u][pos[u] + h - 1];
        pos[u] += (right[u] ? x <= v[u] : x < v[u]) ? h : 0;
      }
    }
#pragma unroll
    for (int u = 0; u < kPer; ++u) {  // pos <= L - 1 so far
      const int i = u * kBlock + threadIdx.x;
      const int32_t x = r[u][pos[u]];
      pos[u] += (right[u] ? x <= v[u] : x < v[u]) ? 1 : 0;
      out[(right[u] ? i - L : i) + pos[u]] = v[u];
      cnt += right[u] ? static_cast<u64>(L - pos[u]) : 0u;
    }
    __syncthreads();
    cur ^= 1;
  }
  int32_t* dst = a.buf0 + row * n + lo0;
#pragma unroll
  for (int u = 0; u < kPer; ++u) {
    const int i = u * kBlock + threadIdx.x;
    if (i < len) dst[i] = buf[cur][i];
  }
  const u64 total = block_sum(cnt, w);
  if (threadIdx.x == 0) a.part[row * 6 * tiles + 3 * tiles + tile] = static_cast<int64_t>(total);
}

// how many of the first d merged elements of (A, B) come from A, ties A-first.  One thread bisects:
// a search by 128 probes per round (3 rounds of one dependent load each at a 2^19-element run, where
// the bisection takes 20) measured 18.3 us per level against 17.2 at n = 2^20
// (profiles/kendall_r15.json) and was dropped
__device__ __forceinline__ int64_t merge_path(const int32_t* A, int64_t lenA, const int32_t* B, int64_t lenB,
                                              int64_t d) {
  int64_t lo = d > lenB ? d - lenB : 0, hi = d < lenA ? d : lenA;
  while (lo < hi) {
    const int64_t mid = lo + ((hi - lo) >> 1);
    if (A[mid] <= B[d - mid - 1]) lo = mid + 1; else hi = mid;
  }
  return lo;
}

// one level: sorted runs of `run` elements of `in` merge pairwise into `out` (when `write`); the
// inversions between the two runs of each pair are added to the tile's partial
__global__ __launch_bounds__(kBlock) void kendall_merge_kernel(KendallCountArgs a, int64_t tiles, const int32_t* in,
                                                               int32_t* out, int64_t run, int write) {
  __shared__ int32_t st[kT];
  __shared__ int32_t mo[kT];
  __shared__ int64_t diag[2];
  __shared__ u64 w[kBlock / 64];
  const int64_t tile = blockIdx.x % tiles;
  const int64_t row = blockIdx.x / tiles;
  const int64_t n = a.n;
  const int32_t* src = in + row * n;
  int32_t* dst = out + row * n;
  const int64_t o0 = tile * kT;
  const int olen = static_cast<int>(min(static_cast<int64_t>(kT), n - o0));
  const int64_t pbase = o0 / (2 * run) * (2 * run);
  if (pbase + run >= n) {  // an unpaired last run is copied through
    if (write) {
#pragma unroll
      for (int u = 0; u < kPer; ++u) {
        const int i = u * kBlock + threadIdx.x;
        if (i < olen) dst[o0 + i] = src[o0 + i];
      }
    }
    return;
  }
  const int64_t lenA = run, lenB = min(run, n - pbase - run);
  const int32_t* A = src + pbase;
  const int32_t* B = A + run;
  const int64_t d0 = o0 - pbase, d1 = d0 + olen;  // the pair ends at min(pbase + 2 run, n) >= o0 + olen
  if (threadIdx.x == 0) diag[0] = merge_path(A, lenA, B, lenB, d0);
  if (threadIdx.x == 64) diag[1] = merge_path(A, lenA, B, lenB, d1);
  __syncthreads();
  const int64_t a0 = diag[0], a1 = diag[1];
  const int64_t b0 = d0 - a0;
  // sorted runs give 0 <= a1 - a0 <= olen; the clamp keeps every index below in the tile regardless
  const int na = static_cast<int>(min(max(a1 - a0, int64_t{0}), static_cast<int64_t>(olen))), nb = olen - na;
#pragma unroll
  for (int u = 0; u < kPer; ++u) {
    const int i = u * kBlock + threadIdx.x;
    if (i < olen) st[i] = i < na ? A[a0 + i] : B[b0 + (i - na)];
  }
  __syncthreads();
  // with A-first ties every A element before a0 is <= each staged b and every one from a1 on is above it
  const u64 above = static_cast<u64>(lenA - a1);
  u64 cnt = 0;
#pragma unroll
  for (int u = 0; u < kPer; ++u) {
    const int i = u * kBlock + threadIdx.x;
    if (i >= olen) continue;
    const int32_t v = st[i];
    if (i < na) {  // behind the staged B elements below it
      int lo = 0, hi = nb;
      const int32_t* r = st + na;
      while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        if (r[mid] < v) lo = mid + 1; else hi = mid;
      }
      mo[i + lo] = v;
    } else {  // behind the staged A elements not above it; the others are inversions
      int lo = 0, hi = na;
      while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        if (st[mid] <= v) lo = mid + 1; else hi = mid;
      }
      mo[(i - na) + lo] = v;
      cnt += above + static_cast<u64>(na - lo);
    }
  }
  __syncthreads();
  if (write) {
#pragma unroll
    for (int u = 0; u < kPer; ++u) {
      const int i = u * kBlock + threadIdx.x;
      if (i < olen) dst[o0 + i] = mo[i];
    }
  }
  const u64 total = block_sum(cnt, w);
  if (threadIdx.x == 0) a.part[row * 6 * tiles + 3 * tiles + tile] += static_cast<int64_t>(total);
}

__global__ __launch_bounds__(64) void kendall_finish_kernel(KendallCountArgs a, int64_t tiles) {
  const int64_t row = blockIdx.x;
  const int64_t* p = a.part + row * 6 * tiles;
  u64 v[6] = {0, 0, 0, 0, 0, 0};
  for (int64_t b = threadIdx.x; b < tiles; b += 64) {
#pragma unroll
    for (int k = 0; k < 6; ++k) v[k] += static_cast<u64>(p[k * tiles + b]);
  }
#pragma unroll
  for (int k = 0; k < 6; ++k) v[k] = wave_sum(v[k]);
  if (threadIdx.x >= 6) return;
  const bool nan = a.flags[row * 2] != 0 || a.flags[row * 2 + 1] != 0 ||
                   (a.sort_fault != nullptr && *a.sort_fault != 0u);
  // a task without a value has no counts either
  int64_t mine = 0;
#pragma unroll
  for (int k = 0; k < 6; ++k) mine = threadIdx.x == k ? static_cast<int64_t>(v[k]) : mine;
  a.counts[row * 6 + threadIdx.x] = nan ? int64_t{-1} : mine;
  if (threadIdx.x != 0) return;
  const int64_t n = a.n;
  const int64_t n0 = n * (n - 1) / 2;
  const int64_t n1 = static_cast<int64_t>(v[0]), n2 = static_cast<int64_t>(v[1]), n3 = static_cast<int64_t>(v[2]);
  const int64_t q = static_cast<int64_t>(v[3]);
  const int64_t mx = static_cast<int64_t>(v[4]), my = static_cast<int64_t>(v[5]);
  const int64_t S = n0 - n1 - n2 + n3 - 2 * q;
  const bool defined = !nan && n >= 2 && n0 != n1 && n0 != n2;
  double tau;
  if (a.variant == 0) {
    tau = static_cast<double>(S) / (sqrt(static_cast<double>(n0 - n1)) * sqrt(static_cast<double>(n0 - n2)));
  } else {
    const double m = static_cast<double>(mx < my ? mx : my), dn = static_cast<double>(n);
    tau = (2.0 * static_cast<double>(S)) / (dn * dn * ((m - 1.0) / m));
  }
  a.out[row] = defined ? static_cast<float>(tau) : __uint_as_float(0x7fc00000u);
}

bool kendall_shape_ok(int64_t rows, int64_t n) {
  return rows >= 1 && n >= 2 && n < (int64_t{1} << 31) && rows * kendall_tiles(n) < (int64_t{1} << 31);
}

}  // namespace

int64_t kendall_tiles(int64_t n) { return (n + kT - 1) / kT; }

int launch_kendall_prepare(const KendallPrepareArgs& a, hipStream_t stream) {
  if (a.rows <= 0) return 0;
  if (!kendall_shape_ok(a.rows, a.n)) return 1;
  const int64_t tiles = kendall_tiles(a.n);
  hipLaunchKernelGGL(kendall_prepare_kernel, dim3(static_cast<unsigned>(a.rows * tiles)), dim3(kBlock), 0, stream, a,
                     tiles);
  return hipGetLastError() == hipSuccess ? 0 : 2;
}

int launch_kendall_count(const KendallCountArgs& a, hipStream_t stream) {
  if (a.rows <= 0) return 0;
  if (!kendall_shape_ok(a.rows, a.n) || (a.variant != 0 && a.variant != 1)) return 1;
  const int64_t tiles = kendall_tiles(a.n);
  const dim3 grid(static_cast<unsigned>(a.rows * tiles));
  hipLaunchKernelGGL(kendall_ties_kernel, grid, dim3(kBlock), 0, stream, a, tiles);
  hipLaunchKernelGGL(kendall_tile_kernel, grid, dim3(kBlock), 0, stream, a, tiles);
  int levels = 0;
  while ((int64_t{1} << levels) < tiles) ++levels;
  const int32_t* in = a.buf0;
  int32_t* out = a.buf1;
  for (int l = 0; l < levels; ++l) {
    // nobody reads the last level's merged row
    hipLaunchKernelGGL(kendall_merge_kernel, grid, dim3(kBlock), 0, stream, a, tiles, in, out,
                       static_cast<int64_t>(kT) << l, l + 1 < levels ? 1 : 0);
    const int32_t* t = in;
    in = out;
    out = const_cast<int32_t*>(t);
  }
  hipLaunchKernelGGL(kendall_finish_kernel, dim3(static_cast<unsigned>(a.rows)), dim3(64), 0, stream, a, tiles);
  return hipGetLastError() == hipSuccess ? 0 : 2;
}

}  // namespace tea
