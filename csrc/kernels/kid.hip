// K20: Kernel Inception Distance (docs/parity.md, "Not in the reference").
//
// Per subset s of m rows of `real` (X) and m rows of `fake` (Y), with the polynomial kernel
// k(a, b) = (gamma <a, b> + coef)^degree:
//   sxx = sum_{i != j} k(x_i, x_j)   syy = sum_{i != j} k(y_i, y_j)   sxy = sum_{i, j} k(x_i, y_j)
//   mmd2 = (sxx + syy) / (m (m - 1)) - 2 sxy / m^2
// The ATen form gathers two [m, D] copies per subset, writes three [m, m] Gram matrices and runs
// about a dozen passes over them.  Here everything after the dot product happens in the registers
// that hold the Gram tile, so neither the Gram matrices nor the gathered rows ever exist.
//
// kid_gram_kernel, gfx950 mapping (the only arm; the tile itself is tea_gramtile.h's):
//  * one block = one 128 x 128 tile of one Gram block of one subset.  With T = ceil(m / 128) a
//    subset has T (T + 1) / 2 upper-triangle tiles of XX, as many of YY and T^2 tiles of XY, in
//    that order, each row-major.  The grid is padded to a multiple of 8 and block b takes item
//    (b % 8) * (nb / 8) + b / 8 (K8's order), so an XCD owns a contiguous run of items that share a
//    subset and a row panel in its L2.
//  * rows are fetched through the index lists; the rows past m stage zeros.  Every index is
//    clamped on the unsigned compare to n - 1 before it forms an address.  One FP32 chain over all
//    of D: the next stage's loads are issued into registers before this stage's MFMAs and stored
//    to LDS after them.
//  * epilogue in registers: each accumulator element is widened to FP64, v = fma(d, gamma, coef),
//    the power by left-to-right repeated multiplication, then the mask: padding rows and columns
//    are dropped (with coef != 0 they would add coef^degree each), i == j is dropped on the
//    diagonal tiles of XX and YY (which are computed whole), and the off-diagonal tiles of XX and
//    YY carry weight 2.  Lanes are combined by shuffles, waves in wave order through LDS, and the
//    block stores one FP64 partial to partials[s][item], non-atomically.
// kid_finish_kernel: one block, a wave per subset (strided): the lanes stride the subset's
// partials, are combined by the same fixed shuffle tree, and lane 0 stores sxx, syy, sxy and
// mmd2; after a barrier wave 0 forms the mean and the population standard deviation of the
// values the same way in FP64.  No atomics, no host sync, no cross-block waiting: results are
// bit-identical from run to run.
#include <algorithm>

#include "tea_common.h"
#include "tea_gramtile.h"
#include "tea_kernels.h"

namespace tea {

namespace {

using namespace gramtile;

constexpr int kFinishThreads = 1024;
static_assert(kKidTile == kT, "the tile is tea_gramtile.h's");

__device__ __forceinline__ int64_t clamp_index(int32_t i, int64_t n) {
  const uint32_t u = static_cast<uint32_t>(i);  // a negative index compares as a large one
  return u < static_cast<uint32_t>(n) ? static_cast<int64_t>(u) : n - 1;
}

template <bool kVec>
__global__ __launch_bounds__(kThreads) void kid_gram_kernel(KidGramArgs a, int T, int items, int64_t total) {
  const int64_t nb = gridDim.x;
  const int64_t b = blockIdx.x;
  const int64_t work = (b % 8) * (nb / 8) + b / 8;
  if (work >= total) return;  // grid padding (whole block)
  const int64_t s = work / items;
  const int item = static_cast<int>(work % items);
  const int tri = T * (T + 1) / 2;
  int ti, tj;
  const bool sym = item < 2 * tri;
  const bool rows_fake = item >= tri && sym;  // YY
  const bool cols_fake = item >= tri;          // YY and XY
  if (sym) {
    upper_tile_coords(item < tri ? item : item - tri, T, ti, tj);
  } else {
    ti = (item - 2 * tri) / T;
    tj = (item - 2 * tri) % T;
  }
  const int m = static_cast<int>(a.m);
  const int d = static_cast<int>(a.d);

  __shared__ __attribute__((aligned(16))) float sA[kImage];
  __shared__ __attribute__((aligned(16))) float sB[kImage];
  __shared__ double s_wave[kThreads / kWave];

  const int lane = threadIdx.x & 63;
  const int w = threadIdx.x >> 6;
  const int wr = w >> 1, wc = w & 1;

  // ---- staging: the thread's rows of both operands, through the index lists
  Stage st;
  st.rslot = threadIdx.x >> 3;
  st.kq = threadIdx.x & 7;
  st.d = d;
#pragma unroll
  for (int q = 0; q < kPieces; ++q) {
    const int r = st.rslot + 32 * q;
    const int gi = ti * kT + r, gj = tj * kT + r;
    st.pa[q] = nullptr;
    st.pb[q] = nullptr;
    if (gi < m) {
      st.pa[q] = rows_fake ? a.fake + clamp_index(a.idx_f[s * a.m + gi], a.n_f) * a.fake_stride
                           : a.real + clamp_index(a.idx_r[s * a.m + gi], a.n_r) * a.real_stride;
    }
    if (gj < m) {
      st.pb[q] = cols_fake ? a.fake + clamp_index(a.idx_f[s * a.m + gj], a.n_f) * a.fake_stride
                           : a.real + clamp_index(a.idx_r[s * a.m + gj], a.n_r) * a.real_stride;
    }
  }

  f32x16 acc[2][2];
  zero(acc);
  const int offA = operand_offset(lane, wr), offB = operand_offset(lane, wc);

  st.load<kVec>(0);
  for (int k0 = 0; k0 < d; k0 += kBK) {
    st.store(sA, sB);
    __syncthreads();
    if (k0 + kBK < d) st.load<kVec>(k0 + kBK);  // in flight behind this stage's MFMAs
    mfma_stage(sA, sB, offA, offB, acc);
    __syncthreads();
  }

  // ---- epilogue
  const bool diag = sym && ti == tj;
  double sum = 0.0;
#pragma unroll
  for (int bm = 0; bm < 2; ++bm)
#pragma unroll
    for (int bn = 0; bn < 2; ++bn) {
      const int j = tj * kT + wc * 64 + bn * 32 + (lane & 31);
#pragma unroll
      for (int r = 0; r < 16; ++r) {
#pragma clang fp contract(off)  // the power is a chain of rounded FP64 products (the definition)
        const int i = ti * kT + wr * 64 + bm * 32 + cd_row(r, lane);
        const double v = fma(static_cast<double>(acc[bm][bn][r]), a.gamma, a.coef);
        double p = v;
        for (int e = 1; e < a.degree; ++e) p *= v;
        const bool keep = i < m && j < m && !(diag && i == j);
        sum += keep ? p : 0.0;
      }
    }
  sum = wave_sum(sum);
  if (lane == 0) s_wave[w] = sum;
  __syncthreads();
  if (threadIdx.x == 0) {
    double t = 0.0;
#pragma unroll
    for (int k = 0; k < kThreads / kWave; ++k) t += s_wave[k];
    a.partials[s * items + item] = sym && !diag ? 2.0 * t : t;
  }
}

// the lanes of one wave stride [lo, hi) of p; every lane returns the sum
__device__ __forceinline__ double wave_range_sum(const double* p, int lo, int hi) {
  double t = 0.0;
  for (int k = lo + lane_id(); k < hi; k += kWave) t += p[k];
  return wave_sum(t);
}

__global__ __launch_bounds__(kFinishThreads) void kid_finish_kernel(KidFinishArgs a, int T, int items) {
  const int w = threadIdx.x >> 6;
  const int tri = T * (T + 1) / 2;
  const double m = static_cast<double>(a.m);
  for (int64_t s = w; s < a.subsets; s += kFinishThreads / kWave) {
    const double* p = a.partials + s * items;
    const double sxx = wave_range_sum(p, 0, tri);
    const double syy = wave_range_sum(p, tri, 2 * tri);
    const double sxy = wave_range_sum(p, 2 * tri, items);
    if (lane_id() == 0) {
      a.sums[3 * s] = sxx;
      a.sums[3 * s + 1] = syy;
      a.sums[3 * s + 2] = sxy;
      a.values[s] = (sxx + syy) / (m * (m - 1.0)) - 2.0 * sxy / (m * m);
    }
  }
  __threadfence_block();
  __syncthreads();
  if (w != 0) return;
  const double n = static_cast<double>(a.subsets);
  double t = 0.0;
  for (int64_t s = lane_id(); s < a.subsets; s += kWave) t += a.values[s];
  const double mean = wave_sum(t) / n;
  double q = 0.0;
  for (int64_t s = lane_id(); s < a.subsets; s += kWave) {
    const double dv = a.values[s] - mean;
    q += dv * dv;
  }
  q = wave_sum(q);
  if (lane_id() == 0) {
    a.out[0] = static_cast<float>(mean);
    a.out[1] = static_cast<float>(sqrt(q / n));
  }
}

}  // namespace

int64_t kid_items(int64_t m) {
  const int64_t T = tiles_of(m);
  return T * (T + 1) + T * T;
}

int launch_kid_gram(const KidGramArgs& a, hipStream_t stream) {
  if (a.subsets < 1 || a.m < 2 || a.d < 1 || a.n_r < 1 || a.n_f < 1 || a.degree < 1 || a.degree > 16) return -1;
  if (a.m >= (int64_t{1} << 24) || a.d >= (int64_t{1} << 31) - kBK || a.n_r >= (int64_t{1} << 31) ||
      a.n_f >= (int64_t{1} << 31))
    return -1;
  const int64_t items = kid_items(a.m);
  const int64_t total = a.subsets * items;
  const int64_t grid = (total + 7) / 8 * 8;
  if (grid >= (int64_t{1} << 31)) return -1;
  const bool vec = a.d % 4 == 0 && rows_aligned16(a.real, a.real_stride) && rows_aligned16(a.fake, a.fake_stride);
  const int T = static_cast<int>(tiles_of(a.m));
  if (vec)
    hipLaunchKernelGGL(kid_gram_kernel<true>, dim3(static_cast<unsigned>(grid)), dim3(kThreads), 0, stream, a, T,
                       static_cast<int>(items), total);
  else
    hipLaunchKernelGGL(kid_gram_kernel<false>, dim3(static_cast<unsigned>(grid)), dim3(kThreads), 0, stream, a, T,
                       static_cast<int>(items), total);
  return static_cast<int>(hipGetLastError());
}

int launch_kid_finish(const KidFinishArgs& a, hipStream_t stream) {
  if (a.subsets < 1 || a.m < 2 || a.m >= (int64_t{1} << 24) || kid_items(a.m) >= (int64_t{1} << 31)) return -1;
  hipLaunchKernelGGL(kid_finish_kernel, dim3(1), dim3(kFinishThreads), 0, stream, a, static_cast<int>(tiles_of(a.m)),
                     static_cast<int>(kid_items(a.m)));
  return static_cast<int>(hipGetLastError());
}

}  // namespace tea
