// K17: segmentation mean IoU and Dice, docs/parity.md "Not in the reference".
//
// Replaces the ATen form (functional/classification/mean_iou.py): argmax over the strided class
// axis into an int64 map, a mask for the ignored label and three bincounts.  Here one pass over the
// scores finds every pixel's prediction and counts it:
//  * plane arm (unit pixel stride): a block owns kSegSpan consecutive pixels of one image at a
//    time and a thread a group of 4 (f32, one 16-B load per class at any 4-B alignment) or 8
//    (16-bit, 16-B aligned: groups start where the image's class-0 plane crosses a 16-B boundary,
//    and every class plane shares that alignment because stride_c % 8 == 0) consecutive pixels.
//    The groups cut by the ends of a span read their pixels one element at a time (K7's head and
//    tail).  The thread walks the classes in ascending order, kAhead classes' loads issued before
//    the first compare, and keeps a running maximum per pixel that only a strictly larger value or
//    a first NaN replaces: torch.argmax's lowest index among the maxima, NaN the maximum.  The
//    group's int64 / int32 labels come in 16-B loads too (profiles/segmentation_r13.json).
//  * element arm (any other layout whose pixels flatten to one stride, channels_last among them):
//    the same walk with one pixel per thread and one element per load.
//  * label arm: both operands are contiguous integer maps; no argmax.
// Counting: three u32 [C] histograms per block in LDS (intersection, predicted, target).  A wave
// first folds its pixels by distinct (target, prediction) value, kFoldRounds values at most: a
// ballot of the leader's value, a popcount and one LDS add per histogram, which is all a wave
// inside one segment needs; pixels still left (a wave across many labels) add themselves with
// LDS integer atomics.  The grid is persistent and every block stores its histograms as one
// [3, C] partial, non-atomically; the finish launch adds the partials in block order, as integers,
// into the float64 states, or into a scratch triple whose value it evaluates.  A counted pixel
// with a target (or, in the label arm, a prediction) outside [0, C) is counted nowhere and sets a
// bit of ``err``, the only global atomic.  Integer sums: results are bit-identical run to run.
#include "tea_common.h"
#include "tea_kernels.h"
#include "tea_partials.h"
#include "tea_rowload.h"

namespace tea {

namespace {

constexpr int kB = 256;
constexpr int kAhead = 8;       // classes whose loads are in flight before the first compare
constexpr int kFoldRounds = 2;  // distinct (target, prediction) values a wave folds before its lanes add singly
constexpr int kFinishThreads = 1024;
constexpr int kKeyShift = 10;   // key = target << kKeyShift | prediction
constexpr int kLabels = 3;      // KIND of the label arm (0 / 1 / 2: f32 / bf16 / f16 scores)
static_assert(kSegMaxClasses <= (1 << kKeyShift), "a key holds two class indices");
static_assert(kSegSpan % (8 * kB) == 0, "a span is whole steps of every arm");

// W consecutive pixels of class plane `off` (elements from the image's base): one 16-B load for
// W = 4 (f32, 4-B aligned) and W = 8 (16-bit, 16-B aligned), one element for W = 1
template <int KIND, int W>
__device__ __forceinline__ void load_pixels(const void* img, int64_t off, float (&v)[W]) {
  if constexpr (W == 1) {
    v[0] = load1<KIND>(img, off);
  } else if constexpr (KIND == 0) {
    const float4 x = load_f4u(static_cast<const float*>(img) + off);
    v[0] = x.x, v[1] = x.y, v[2] = x.z, v[3] = x.w;
  } else {
    load_vals<KIND>(img, off, v);
  }
}

// The W consecutive labels from element i of the contiguous target map.  int64 and int32 maps
// (what data loaders hand over) in 16-B loads at the element's own alignment, as load_f4u; the
// narrow dtypes one label per load.
typedef long long ll2u_t __attribute__((ext_vector_type(2), aligned(8)));
typedef int i4u_t __attribute__((ext_vector_type(4), aligned(4)));

template <int W>
__device__ __forceinline__ void load_targets(const void* tg, DType dt, int64_t i, int64_t (&t)[W]) {
  static_assert(W % 4 == 0, "whole 16-B loads");
  if (dt == DType::i64) {
    const ll2u_t* p = reinterpret_cast<const ll2u_t*>(static_cast<const int64_t*>(tg) + i);
#pragma unroll
    for (int u = 0; u < W / 2; ++u) {
      const ll2u_t v = p[u];
      t[2 * u] = v.x, t[2 * u + 1] = v.y;
    }
  } else if (dt == DType::i32) {
    const i4u_t* p = reinterpret_cast<const i4u_t*>(static_cast<const int32_t*>(tg) + i);
#pragma unroll
    for (int u = 0; u < W / 4; ++u) {
      const i4u_t v = p[u];
      t[4 * u] = v.x, t[4 * u + 1] = v.y, t[4 * u + 2] = v.z, t[4 * u + 3] = v.w;
    }
  } else {
#pragma unroll
    for (int j = 0; j < W; ++j) t[j] = load_as_i64(tg, dt, i + j);
  }
}

// torch.argmax over the classes of W pixels whose class-0 values start at element `off`
template <int KIND, int W>
__device__ __forceinline__ void argmax_pixels(const void* img, int64_t off, int64_t stride_c, int C, int (&idx)[W]) {
  float m[W];
  load_pixels<KIND, W>(img, off, m);
#pragma unroll
  for (int j = 0; j < W; ++j) idx[j] = 0;
  int c = 1;
  for (; c + kAhead <= C; c += kAhead) {
    float v[kAhead][W];
#pragma unroll
    for (int u = 0; u < kAhead; ++u) load_pixels<KIND, W>(img, off + (c + u) * stride_c, v[u]);
#pragma unroll
    for (int u = 0; u < kAhead; ++u) {
#pragma unroll
      for (int j = 0; j < W; ++j) {
        const bool take = v[u][j] > m[j] || (v[u][j] != v[u][j] && m[j] == m[j]);
        m[j] = take ? v[u][j] : m[j];
        idx[j] = take ? c + u : idx[j];
      }
    }
  }
  for (; c < C; ++c) {
    float v[W];
    load_pixels<KIND, W>(img, off + c * stride_c, v);
#pragma unroll
    for (int j = 0; j < W; ++j) {
      const bool take = v[j] > m[j] || (v[j] != v[j] && m[j] == m[j]);
      m[j] = take ? v[j] : m[j];
      idx[j] = take ? c : idx[j];
    }
  }
}

// One pixel of every lane (key < 0: none) into the block's histograms: hist[0 .. C) intersection,
// [C .. 2C) predicted, [2C .. 3C) target.  Called by whole waves.
__device__ __forceinline__ void fold(int key, uint32_t* hist, int C, int lane) {
  uint64_t todo = __ballot(key >= 0);
  for (int r = 0; r < kFoldRounds && todo != 0; ++r) {
    const int leader = __builtin_amdgcn_readfirstlane(__ffsll(static_cast<unsigned long long>(todo)) - 1);
    const int k = __builtin_amdgcn_readlane(key, leader);
    const uint64_t members = __ballot(key == k);
    const uint32_t cnt = static_cast<uint32_t>(__popcll(members));
    const int t = k >> kKeyShift, p = k & ((1 << kKeyShift) - 1);
    if (lane < 3 && (lane != 0 || t == p)) atomicAdd(&hist[lane * C + (lane == 1 ? p : t)], cnt);
    if (key == k) key = -1;
    todo &= ~members;
  }
  if (key >= 0) {
    const int t = key >> kKeyShift, p = key & ((1 << kKeyShift) - 1);
    atomicAdd(&hist[C + p], 1u);
    atomicAdd(&hist[2 * C + t], 1u);
    if (t == p) atomicAdd(&hist[t], 1u);
  }
}

// KIND 0 / 1 / 2 with PIX 4 / 8 / 8: plane arm; with PIX 1: element arm; KIND kLabels, PIX 1: label arm
template <int KIND, int PIX>
__global__ __launch_bounds__(kB) void segmentation_count_kernel(SegmentationArgs a) {
  extern __shared__ uint32_t hist[];
  const int C = a.c;
  for (int i = threadIdx.x; i < 3 * C; i += kB) hist[i] = 0u;
  __syncthreads();
  const int lane = lane_id();
  const int64_t spans_per_image = (a.p + kSegSpan - 1) / kSegSpan;
  const int64_t spans = a.n * spans_per_image;
  int flags = 0;
  for (int64_t s = blockIdx.x; s < spans; s += gridDim.x) {
    const int64_t n = s / spans_per_image;
    const int64_t lo = (s - n * spans_per_image) * kSegSpan;
    const int64_t hi = lo + kSegSpan < a.p ? lo + kSegSpan : a.p;
    const char* img = nullptr;
    if constexpr (KIND != kLabels) img = static_cast<const char*>(a.input) + n * a.stride_n * kind_bytes<KIND>;
    // the pixel at which the span's first group starts: lo, or for 16-B loads of 16-bit values the
    // last pixel at or before lo that is 16-B aligned in every class plane (it may lie before lo)
    int64_t g0 = lo;
    if constexpr (PIX == 8) {
      const int64_t h = head_elems<KIND>(img);
      g0 = lo - (((lo - h) % 8) + 8) % 8;
    }
    const int groups = static_cast<int>((hi - g0 + PIX - 1) / PIX);
    // block-uniform trip count: every lane takes part in the wave's fold
    for (int k0 = 0; k0 < groups; k0 += kB) {
      const int k = k0 + threadIdx.x;
      const int64_t q0 = g0 + static_cast<int64_t>(k) * PIX;
      int key[PIX];
#pragma unroll
      for (int j = 0; j < PIX; ++j) key[j] = -1;
      if (k < groups) {
        int pred[PIX];
        bool live[PIX];
        const bool full = q0 >= lo && q0 + PIX <= hi;
#pragma unroll
        for (int j = 0; j < PIX; ++j) live[j] = q0 + j >= lo && q0 + j < hi;
        if constexpr (KIND == kLabels) {
          const int64_t v = load_as_i64(a.input, a.in_dt, n * a.p + q0);
          pred[0] = v >= 0 && v < C ? static_cast<int>(v) : -1;
        } else if (PIX > 1 && full) {
          argmax_pixels<KIND, PIX>(img, q0, a.stride_c, C, pred);
        } else {
#pragma unroll
          for (int j = 0; j < PIX; ++j) {
            int one[1] = {0};
            if (live[j]) argmax_pixels<KIND, 1>(img, (q0 + j) * a.stride_p, a.stride_c, C, one);
            pred[j] = one[0];
          }
        }
        int64_t label[PIX];
        if constexpr (PIX > 1) {
          if (full) load_targets<PIX>(a.target, a.tg_dt, n * a.p + q0, label);
        }
#pragma unroll
        for (int j = 0; j < PIX; ++j) {
          if (!live[j]) continue;
          const int64_t t = PIX > 1 && full ? label[j] : load_as_i64(a.target, a.tg_dt, n * a.p + q0 + j);
          if (a.has_ignore && t == a.ignore_index) continue;
          const int bad = ((t >= 0 && t < C) ? 0 : 1) | (pred[j] >= 0 ? 0 : 2);
          flags |= bad;
          if (bad == 0) key[j] = (static_cast<int>(t) << kKeyShift) | pred[j];
        }
      }
#pragma unroll
      for (int j = 0; j < PIX; ++j) fold(key[j], hist, C, lane);
    }
  }
  if (flags != 0 && a.err) atomicOr(a.err, flags);
  __syncthreads();
  uint32_t* part = a.partial + static_cast<int64_t>(blockIdx.x) * 3 * C;
  for (int i = threadIdx.x; i < 3 * C; i += kB) part[i] = hist[i];
}

// ---------------------------------------------------------------- value and finish
// By one whole wave.  FP64; a class absent from both maps (union 0) is NaN and outside the macro mean
__device__ void segmentation_value(const double* inter, const double* pred, const double* target, int64_t C, int dice,
                                   int average, float* out, int lane) {
  double num = 0.0, den = 0.0;
  for (int64_t c = lane; c < C; c += kWave) {
    const double i = inter[c], both = pred[c] + target[c], u = both - i;
    const double top = dice ? 2.0 * i : i, bottom = dice ? both : u;
    if (average == 2) {
      out[c] = static_cast<float>(top / bottom);
    } else if (average == 1) {
      num += top;
      den += bottom;
    } else if (u > 0.0) {
      num += top / bottom;
      den += 1.0;
    }
  }
  if (average == 2) return;
  num = wave_sum(num);
  den = wave_sum(den);
  if (lane == 0) *out = static_cast<float>(num / den);
}

// One block.  The [3, C] pairs are taken kFinishThreads at a time (once for C <= 341): thread
// (q, p) adds pair p over the q-th run of consecutive blocks, 16 loads in flight (K15's finish),
// then the runs are added.  Integer sums, so the grouping does not show in the result.
__global__ __launch_bounds__(kFinishThreads) void segmentation_finish_kernel(SegmentationArgs a, int blocks) {
  __shared__ unsigned long long run[kFinishThreads];
  const int C = a.c, pairs = 3 * C;
  for (int p0 = 0; p0 < pairs; p0 += kFinishThreads) {
    const int np = pairs - p0 < kFinishThreads ? pairs - p0 : kFinishThreads;
    const int runs = kFinishThreads / np;
    const int per = (blocks + runs - 1) / runs;
    const int q = threadIdx.x / np, p = p0 + threadIdx.x % np;
    if (q < runs)
      run[threadIdx.x] = run_fold<unsigned long long>(a.partial + p, pairs, q * per, min(blocks, (q + 1) * per));
    __syncthreads();
    if (threadIdx.x < np) {
      unsigned long long acc = 0;
      for (int r = 0; r < runs; ++r) acc += run[r * np + threadIdx.x];
      double* dst = a.dst[p / C] + p % C;
      *dst = a.accumulate ? *dst + static_cast<double>(acc) : static_cast<double>(acc);
    }
    __syncthreads();
  }
  if (a.out && threadIdx.x < kWave)
    segmentation_value(a.dst[0], a.dst[1], a.dst[2], C, a.dice, a.average, a.out, threadIdx.x);
}

__global__ __launch_bounds__(kWave) void segmentation_value_kernel(const double* inter, const double* pred,
                                                                   const double* target, int64_t C, int dice,
                                                                   int average, float* out) {
  segmentation_value(inter, pred, target, C, dice, average, out, threadIdx.x);
}

template <int KIND>
void launch_scores(const SegmentationArgs& a, int blocks, size_t lds, hipStream_t s) {
  constexpr int kVec = KIND == 0 ? 4 : 8;
  if (a.arm == 0) hipLaunchKernelGGL((segmentation_count_kernel<KIND, kVec>), dim3(blocks), dim3(kB), lds, s, a);
  else hipLaunchKernelGGL((segmentation_count_kernel<KIND, 1>), dim3(blocks), dim3(kB), lds, s, a);
}

bool integer_dtype(DType d) {
  return d == DType::u8 || d == DType::i8 || d == DType::i16 || d == DType::i32 || d == DType::i64;
}

}  // namespace

int segmentation_blocks(int64_t n, int64_t p) {
  return stream_grid(n * ((p + kSegSpan - 1) / kSegSpan), 1, kSegMaxBlocks);
}

int launch_segmentation(const SegmentationArgs& a, hipStream_t stream) {
  if (a.n <= 0 || a.p <= 0) return 0;
  if (a.c < 1 || a.c > kSegMaxClasses || a.arm < 0 || a.arm > 2 || a.average < 0 || a.average > 2) return -1;
  if (a.input == nullptr || a.target == nullptr || a.partial == nullptr) return -1;
  if (a.dst[0] == nullptr || a.dst[1] == nullptr || a.dst[2] == nullptr) return -1;
  if (!integer_dtype(a.tg_dt)) return -1;
  const int blocks = segmentation_blocks(a.n, a.p);
  const int64_t spans = a.n * ((a.p + kSegSpan - 1) / kSegSpan);
  // a block's u32 counts: the pixels it owns must stay below 2^32
  if ((spans + blocks - 1) / blocks >= (int64_t{1} << 32) / kSegSpan) return -3;
  const size_t lds = static_cast<size_t>(3) * a.c * sizeof(uint32_t);
  if (a.arm == 2) {
    if (!integer_dtype(a.in_dt)) return -1;
    hipLaunchKernelGGL((segmentation_count_kernel<kLabels, 1>), dim3(blocks), dim3(kB), lds, stream, a);
  } else {
    const int els = dtype_bytes(a.in_dt);
    if (reinterpret_cast<uintptr_t>(a.input) % els != 0) return -2;  // planes must be element-aligned
    if (a.arm == 0 && a.p > 1 && a.stride_p != 1) return -2;
    if (a.arm == 0 && els == 2 && a.c > 1 && a.stride_c % 8 != 0) return -2;  // one alignment for every class plane
    if (with_kind(a.in_dt, [&](auto kind) { return launch_scores<kind()>(a, blocks, lds, stream), 0; }) != 0) return -1;
  }
  hipLaunchKernelGGL(segmentation_finish_kernel, dim3(1), dim3(kFinishThreads), 0, stream, a, blocks);
  return static_cast<int>(hipGetLastError());
}

int launch_segmentation_value(const double* intersection, const double* pred_count, const double* target_count,
                              int64_t c, int dice, int average, float* out, hipStream_t stream) {
  if (c < 1 || average < 0 || average > 2) return -1;
  hipLaunchKernelGGL(segmentation_value_kernel, dim3(1), dim3(kWave), 0, stream, intersection, pred_count,
                     target_count, c, dice, average, out);
  return static_cast<int>(hipGetLastError());
}

}  // namespace tea
