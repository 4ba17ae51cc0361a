// K27: Hausdorff and average surface distance of integer label-map pairs (docs/parity.md, "Not in the
// reference"), for unit pixel spacing.  For image n and class c, A = (input == c) and B = (target == c);
// a surface pixel of a mask is a pixel of it with a 4-neighbour outside it (the image border counts as
// outside).  The nearest-surface search is exact and separated by axis:
//
//   clear    zeroes the per-plane surface counts (a kernel, so the op can sit in a captured graph)
//   rows     one wave per (plane, row): the surface bits of the row as ballot words, one per 64-column
//            segment; from them the distance along the row to the nearest surface pixel on either side
//            (carried across the segments), the smaller as u16 g[plane][y][x]
//   search   one wave per (plane, row, segment): the lanes that are surface pixels of the plane's side
//            walk the OTHER side's g up and down their column, best = min(best, g[y +- k][x]^2 + k^2),
//            until k^2 >= best in every lane of the wave (and never past the image); adjacent lanes are
//            adjacent columns, so every step is two coalesced row loads.  No distance plane is formed.
//   finish   one block per (image, class, direction): the u32 maximum, the FP64 sum of the square roots
//            in one association order, or the two order statistics of a percentile by a radix select
//            over the integer squared distances
//   combine  one block: the two directions, the empty-surface rules, the [n, classes] values and the
//            class states
//
// Everything before the final square root is integer arithmetic, the only atomics are integer adds,
// and every floating-point sum has one order: a result is bit-identical from run to run.
#include "tea_common.h"
#include "tea_kernels.h"

namespace tea {
namespace {

constexpr int kRowWaves = 4;       // waves of a rows / search block
constexpr int kFinishT = 1024;     // threads of a finish block
constexpr int kCombineT = 256;     // threads of the combine block: 4 image slices x 64 class lanes
constexpr int kNoIndex = 1 << 20;  // "no surface pixel to the right" (> any column)

struct Maps {
  const void* p[2];  // side 0: input, side 1: target
  DType dt[2];
  int h, w;
  int classes, class_base;
};

__device__ __forceinline__ unsigned long long readlane_u64(unsigned long long v, int l) {
  const unsigned lo = __builtin_amdgcn_readlane(static_cast<unsigned>(v), l);
  const unsigned hi = __builtin_amdgcn_readlane(static_cast<unsigned>(v >> 32), l);
  return (static_cast<unsigned long long>(hi) << 32) | lo;
}

__global__ void surface_clear_kernel(uint32_t* counts, int64_t planes) {
  const int64_t i = static_cast<int64_t>(blockIdx.x) * blockDim.x + threadIdx.x;
  if (i < planes) counts[i] = 0u;
}

// One wave per (plane, row).  Segment s of the row is columns [64 s, 64 s + 64); w <= kSurfMaxSide, so a
// row has at most 32 segments and lane s keeps the ballot word of segment s.
__global__ __launch_bounds__(kRowWaves* kWave) void surface_rows_kernel(Maps m, int64_t waves, uint16_t* g,
                                                                        uint32_t* counts) {
  const int64_t wv = static_cast<int64_t>(blockIdx.x) * kRowWaves + wave_id();
  if (wv >= waves) return;
  const int lane = lane_id();
  const int64_t plane = wv / m.h;
  const int y = static_cast<int>(wv - plane * m.h);
  const int side = static_cast<int>(plane & 1);
  const int64_t image = (plane >> 1) / m.classes;
  const int64_t cls = (plane >> 1) % m.classes + m.class_base;
  const void* lab = m.p[side];
  const DType dt = m.dt[side];
  const int64_t base = image * m.h * m.w;
  const int64_t row = base + static_cast<int64_t>(y) * m.w;
  const int segs = (m.w + kWave - 1) / kWave;

  unsigned long long mine = 0ull;
  for (int s = 0; s < segs; ++s) {
    const int x = s * kWave + lane;
    bool surface = false;
    if (x < m.w && load_as_i64(lab, dt, row + x) == cls) {
      const bool up = y > 0 && load_as_i64(lab, dt, row - m.w + x) == cls;
      const bool down = y + 1 < m.h && load_as_i64(lab, dt, row + m.w + x) == cls;
      const bool left = x > 0 && load_as_i64(lab, dt, row + x - 1) == cls;
      const bool right = x + 1 < m.w && load_as_i64(lab, dt, row + x + 1) == cls;
      surface = !(up && down && left && right);
    }
    const unsigned long long word = __ballot(surface);
    if (lane == s) mine = word;
  }

  // per segment: the last surface column of the segments before it, the first of those after it
  int last = mine != 0ull ? lane * kWave + 63 - __builtin_clzll(mine) : -1;
  int first = mine != 0ull ? lane * kWave + __builtin_ctzll(mine) : kNoIndex;
#pragma unroll
  for (int o = 1; o < kWave; o <<= 1) {
    const int a = __shfl_up(last, o, kWave);
    const int b = __shfl_down(first, o, kWave);
    if (lane >= o) last = max(last, a);
    if (lane + o < kWave) first = min(first, b);
  }
  int before = __shfl_up(last, 1, kWave);
  int after = __shfl_down(first, 1, kWave);
  if (lane == 0) before = -1;
  if (lane == kWave - 1) after = kNoIndex;

  const unsigned total = static_cast<unsigned>(wave_sum(static_cast<int>(__popcll(mine))));
  if (lane == 0 && total != 0u) atomicAdd(&counts[plane], total);

  uint16_t* grow = g + plane * m.h * m.w + static_cast<int64_t>(y) * m.w;
  for (int s = 0; s < segs; ++s) {
    const unsigned long long word = readlane_u64(mine, s);
    const int carry_l = __builtin_amdgcn_readlane(before, s);
    const int carry_r = __builtin_amdgcn_readlane(after, s);
    const int x = s * kWave + lane;
    const unsigned long long at_or_below = word & ((2ull << lane) - 1ull);  // lane 63: every bit
    const unsigned long long at_or_above = word & (~0ull << lane);
    const int li = at_or_below != 0ull ? s * kWave + 63 - __builtin_clzll(at_or_below) : carry_l;
    const int ri = at_or_above != 0ull ? s * kWave + __builtin_ctzll(at_or_above) : carry_r;
    const int dl = li >= 0 ? x - li : static_cast<int>(kSurfNone);
    const int dr = ri < kNoIndex ? ri - x : static_cast<int>(kSurfNone);
    if (x < m.w) grow[x] = static_cast<uint16_t>(min(dl, dr));
  }
}

__device__ __forceinline__ unsigned surf_candidate(const uint16_t* col, int64_t off, unsigned k2) {
  const unsigned u = col[off];
  return u == kSurfNone ? kSurfNoPixel : u * u + k2;
}

// One wave per (plane, row, segment) of the planes that search: every plane, or side 0 only when
// `sides` is 1.  The loop is wave-uniform and ends at the image's edge whatever g holds.
__global__ __launch_bounds__(kRowWaves* kWave) void surface_search_kernel(int h, int w, int sides, int64_t waves,
                                                                          const uint16_t* g, const uint32_t* counts,
                                                                          uint32_t* d2) {
  const int64_t wv = static_cast<int64_t>(blockIdx.x) * kRowWaves + wave_id();
  if (wv >= waves) return;
  const int segs = (w + kWave - 1) / kWave;
  const int s = static_cast<int>(wv % segs);
  const int64_t r = wv / segs;
  const int y = static_cast<int>(r % h);
  const int64_t plane = sides == 2 ? r / h : (r / h) * 2;
  const int64_t other = plane ^ 1;
  const int x = s * kWave + lane_id();
  const bool inside = x < w;
  const int64_t hw = static_cast<int64_t>(h) * w;
  const int64_t at = static_cast<int64_t>(y) * w + x;
  uint32_t* out = d2 + plane * hw;
  if (counts[plane] == 0u || counts[other] == 0u) {  // the value is +inf or NaN by the counts
    if (inside) out[at] = kSurfNoPixel;
    return;
  }
  const bool surface = inside && g[plane * hw + at] == 0;
  const uint16_t* col = g + other * hw;
  unsigned best = inside ? surf_candidate(col, at, 0u) : kSurfNoPixel;
  const int kmax = max(y, h - 1 - y);
  // four steps between two looks at the exit: their eight row loads are in flight together, and a
  // step past a lane's exit only offers it larger candidates
  for (int k0 = 1; k0 <= kmax; k0 += 4) {
    if (__ballot(surface && static_cast<unsigned>(k0) * k0 < best) == 0ull) break;
    unsigned c[8];
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const int k = k0 + i;
      const unsigned k2 = static_cast<unsigned>(k) * k;
      c[2 * i] = inside && y - k >= 0 ? surf_candidate(col, at - static_cast<int64_t>(k) * w, k2) : kSurfNoPixel;
      c[2 * i + 1] = inside && y + k < h ? surf_candidate(col, at + static_cast<int64_t>(k) * w, k2) : kSurfNoPixel;
    }
#pragma unroll
    for (int i = 0; i < 8; ++i) best = min(best, c[i]);
  }
  if (inside) out[at] = surface ? best : kSurfNoPixel;
}

// block-wide exclusive prefix sum of one count per thread (kFinishT threads); `total` in every thread
__device__ __forceinline__ unsigned block_excl_sum(unsigned v, unsigned* s_wave, unsigned& total) {
  const unsigned incl = wave_incl_sum(v);
  const int wv = threadIdx.x >> 6;
  __syncthreads();
  if (lane_id() == kWave - 1) s_wave[wv] = incl;
  __syncthreads();
  unsigned before = 0u;
  total = 0u;
  for (int k = 0; k < kFinishT / kWave; ++k) {
    const unsigned t = s_wave[k];
    before += k < wv ? t : 0u;
    total += t;
  }
  return before + incl - v;
}

// One block per (image, class, direction): partial[plane] = {the direction's Hausdorff value, the sum of
// its distances}.  A plane without a value (either surface empty) is left alone.
__global__ __launch_bounds__(kFinishT) void surface_finish_kernel(int64_t hw, int sides, int mode, double quantile,
                                                                  const uint32_t* d2, const uint32_t* counts,
                                                                  double* partial) {
  __shared__ unsigned s_hist[256];
  __shared__ unsigned s_wave[kFinishT / kWave];
  __shared__ double s_sum[kFinishT / kWave];
  __shared__ unsigned s_pick[3];
  const int64_t b = blockIdx.x;
  const int64_t plane = sides == 2 ? b : b * 2;
  const unsigned m = counts[plane];
  if (m == 0u || counts[plane ^ 1] == 0u) return;
  const uint32_t* v = d2 + plane * hw;
  const int tid = threadIdx.x;

  unsigned mx = 0u;
  double sum = 0.0;
  for (int64_t i = tid; i < hw; i += kFinishT) {
    const unsigned d = v[i];
    if (d == kSurfNoPixel) continue;
    mx = max(mx, d);
    if (mode == 1) sum += sqrt(static_cast<double>(d));
  }
  // lane-strided above; the wave butterfly; the waves in order
  mx = wave_max(mx);
  sum = wave_sum(sum);
  if (lane_id() == 0) {
    s_wave[tid >> 6] = mx;
    s_sum[tid >> 6] = sum;
  }
  __syncthreads();
  mx = 0u;
  sum = 0.0;
  for (int k = 0; k < kFinishT / kWave; ++k) {
    mx = max(mx, s_wave[k]);
    sum += s_sum[k];
  }
  double value = sqrt(static_cast<double>(mx));

  if (mode == 0 && quantile >= 0.0) {
    // numpy's linear interpolation at position quantile * (m - 1) of the sorted distances: the order
    // statistics `lo` and `lo + 1` of the squared distances, by three histogram passes (8 + 8 + 7 bits)
    const double pos = quantile * static_cast<double>(m - 1u);
    unsigned lo = static_cast<unsigned>(pos);
    lo = min(lo, m - 1u);
    const double frac = pos - static_cast<double>(lo);
    unsigned rank = lo, prefix = 0u, equal = 0u;
    int fixed_from = 23;  // the bits of `prefix` at and above this are decided
    for (int pass = 0; pass < 3; ++pass) {
      const int shift = pass == 0 ? 15 : (pass == 1 ? 7 : 0);
      const unsigned bins = pass == 2 ? 128u : 256u;
      __syncthreads();
      if (tid < 256) s_hist[tid] = 0u;
      __syncthreads();
      for (int64_t i = tid; i < hw; i += kFinishT) {
        const unsigned d = v[i];
        if (d != kSurfNoPixel && (d >> fixed_from) == (prefix >> fixed_from))
          atomicAdd(&s_hist[(d >> shift) & (bins - 1u)], 1u);
      }
      __syncthreads();
      const unsigned cnt = tid < 256 ? s_hist[tid] : 0u;
      unsigned total;
      const unsigned before = block_excl_sum(cnt, s_wave, total);
      if (cnt != 0u && before <= rank && rank < before + cnt) {  // exactly one thread
        s_pick[0] = static_cast<unsigned>(tid);
        s_pick[1] = rank - before;
        s_pick[2] = cnt;
      }
      __syncthreads();
      prefix |= s_pick[0] << shift;
      rank = s_pick[1];
      equal = s_pick[2];
      fixed_from = shift;
    }
    const double a = sqrt(static_cast<double>(prefix));
    value = a;
    if (frac > 0.0 && rank + 1u >= equal) {  // the next order statistic is the next larger value
      unsigned next = kSurfNoPixel;
      for (int64_t i = tid; i < hw; i += kFinishT) {
        const unsigned d = v[i];
        if (d > prefix) next = min(next, d);  // kSurfNoPixel is the largest u32
      }
      next = ~wave_max(~next);
      __syncthreads();
      if (lane_id() == 0) s_wave[tid >> 6] = next;
      __syncthreads();
      for (int k = 0; k < kFinishT / kWave; ++k) next = min(next, s_wave[k]);
      // lo + 1 <= m - 1 when frac > 0, so a larger value exists
      if (next != kSurfNoPixel) value = a + (sqrt(static_cast<double>(next)) - a) * frac;
    }
  }
  if (tid == 0) {
    partial[plane * 2] = value;
    partial[plane * 2 + 1] = sum;
  }
}

// One block: lane k of wave j takes class k and the images j, j + 4, ...; the four slices of a class are
// added in order.  The states take the float32 values, so they equal the sums of what `out` holds.
__global__ __launch_bounds__(kCombineT) void surface_combine_kernel(int64_t n, int classes, int mode, int both,
                                                                    const uint32_t* counts, const double* partial,
                                                                    float* out, double* value_sum, double* num_finite,
                                                                    double* num_inf) {
  __shared__ double s_acc[kCombineT / kWave][3][kWave];
  const int k = lane_id();
  const int slice = threadIdx.x >> 6;
  double sum = 0.0, finite = 0.0, inf = 0.0;
  if (k < classes) {
    for (int64_t i = slice; i < n; i += kCombineT / kWave) {
      const int64_t plane = (i * classes + k) * 2;
      const unsigned ma = counts[plane], mb = counts[plane + 1];
      float value;
      if (ma == 0u && mb == 0u) {
        value = __builtin_nanf("");
      } else if (ma == 0u || mb == 0u) {
        value = __builtin_inff();
      } else if (mode == 0) {
        const double ab = partial[plane * 2];
        value = static_cast<float>(both ? fmax(ab, partial[plane * 2 + 2]) : ab);
      } else {
        const double ab = partial[plane * 2 + 1];
        value = static_cast<float>(both ? (ab + partial[plane * 2 + 3]) / (static_cast<double>(ma) + mb)
                                        : ab / static_cast<double>(ma));
      }
      if (out != nullptr) out[i * classes + k] = value;
      if (ma != 0u && mb != 0u) {
        sum += static_cast<double>(value);
        finite += 1.0;
      } else if (ma != 0u || mb != 0u) {
        inf += 1.0;
      }
    }
  }
  s_acc[slice][0][k] = sum;
  s_acc[slice][1][k] = finite;
  s_acc[slice][2][k] = inf;
  __syncthreads();
  if (value_sum != nullptr && slice == 0 && k < classes) {
    double t[3] = {0.0, 0.0, 0.0};
    for (int j = 0; j < kCombineT / kWave; ++j) {
      for (int q = 0; q < 3; ++q) t[q] += s_acc[j][q][k];
    }
    value_sum[k] += t[0];
    num_finite[k] += t[1];
    num_inf[k] += t[2];
  }
}

bool label_dtype(DType dt) {
  return dt == DType::u8 || dt == DType::i8 || dt == DType::i16 || dt == DType::i32 || dt == DType::i64;
}

}  // namespace

bool surface_distance_geometry_ok(int64_t n, int64_t h, int64_t w, int64_t classes) {
  if (n < 1 || h < 1 || w < 1 || h > kSurfMaxSide || w > kSurfMaxSide) return false;
  if (classes < 1 || classes > kSurfMaxClasses) return false;
  // the search launch has the most waves: one per (plane, row, segment), kRowWaves to a block
  const int64_t segs = (w + kWave - 1) / kWave;
  return n <= (int64_t{1} << 31) / (classes * 2 * h * segs);
}

int launch_surface_distance(const SurfaceDistanceArgs& a, hipStream_t stream) {
  if (!surface_distance_geometry_ok(a.n, a.h, a.w, a.classes) || !label_dtype(a.in_dt) || !label_dtype(a.tg_dt))
    return 1;
  if (a.input == nullptr || a.target == nullptr || a.g == nullptr || a.d2 == nullptr || a.counts == nullptr ||
      a.partial == nullptr)
    return 1;
  if (a.out == nullptr && a.value_sum == nullptr) return 1;
  if ((a.value_sum == nullptr) != (a.num_finite == nullptr) || (a.value_sum == nullptr) != (a.num_inf == nullptr))
    return 1;
  if (a.mode == 0 && a.quantile > 1.0) return 1;
  const int64_t planes = surface_distance_planes(a.n, a.classes);
  const int sides = a.both ? 2 : 1;
  const int64_t segs = (a.w + kWave - 1) / kWave;
  Maps m;
  m.p[0] = a.input;
  m.p[1] = a.target;
  m.dt[0] = a.in_dt;
  m.dt[1] = a.tg_dt;
  m.h = a.h;
  m.w = a.w;
  m.classes = a.classes;
  m.class_base = a.class_base;

  hipLaunchKernelGGL(surface_clear_kernel, dim3(static_cast<unsigned>((planes + 255) / 256)), dim3(256), 0, stream,
                     a.counts, planes);
  const int64_t row_waves = planes * a.h;
  hipLaunchKernelGGL(surface_rows_kernel, dim3(static_cast<unsigned>((row_waves + kRowWaves - 1) / kRowWaves)),
                     dim3(kRowWaves * kWave), 0, stream, m, row_waves, a.g, a.counts);
  const int64_t search_waves = a.n * a.classes * sides * a.h * segs;
  hipLaunchKernelGGL(surface_search_kernel, dim3(static_cast<unsigned>((search_waves + kRowWaves - 1) / kRowWaves)),
                     dim3(kRowWaves * kWave), 0, stream, a.h, a.w, sides, search_waves, a.g, a.counts, a.d2);
  hipLaunchKernelGGL(surface_finish_kernel, dim3(static_cast<unsigned>(a.n * a.classes * sides)), dim3(kFinishT), 0,
                     stream, static_cast<int64_t>(a.h) * a.w, sides, a.mode, a.mode == 0 ? a.quantile : -1.0, a.d2,
                     a.counts, a.partial);
  hipLaunchKernelGGL(surface_combine_kernel, dim3(1), dim3(kCombineT), 0, stream, a.n, a.classes, a.mode, a.both,
                     a.counts, a.partial, a.out, a.value_sum, a.num_finite, a.num_inf);
  return hipGetLastError() == hipSuccess ? 0 : 2;
}

}  // namespace tea
