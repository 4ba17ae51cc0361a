// K26: multi-scale SSIM (Wang, Simoncelli and Bovik 2003) of [N, C, H, W] image pairs.
//
// Not in the reference tree; the definition is docs/parity.md "Multi-scale structural similarity":
// level 0 is the input pair, level j + 1 the 2 x 2 average of level j (floor: an odd last row or
// column is dropped); per level and plane the means over the "valid" positions of
// cs = (2 sxy + C2) / (sxx + syy + C2) and ssim = cs (2 mx my + C1) / (mx^2 + my^2 + C1) with K12's
// window; a plane's value is prod_{j < M - 1} max(cs_j, 0)^beta_j * max(ssim_{M-1}, 0)^beta_{M-1}, an
// image's value the mean of its planes' values.
//
// 1. msssim_level<Src, KS, Last>: one launch per level whose plane does not fit one halo, on K12's
//    geometry (csrc/kernels/ssim.hip: a workgroup of four waves per (plane, 64 x 64 output tile), the
//    (64 + ks - 1)^2 halo of both images in LDS as interleaved FP32 (x, y) pairs shifted by the tile's
//    first pixel, the separable window with the horizontal moments kept in registers, bands of 16
//    output rows per wave; the band walk below is a copy of K12's).  Level 0 reads the input dtype;
//    every later level reads the pair workspace, one 8-byte load per pixel straight into the LDS
//    layout.  Unless Last, the block then pools the input rows [row0, row0 + 64) (through H in the
//    last tile row) and the same columns out of LDS: tile edges are even, so no 2 x 2 block straddles
//    two tiles and every pixel of the level is pooled by exactly one block; each thread averages
//    2 x 2 blocks of pairs, adds the shift back and stores one coalesced 8-byte (x, y) per pooled
//    pixel into level j + 1 of the workspace.  The epilogue sums cs (ssim when Last) in FP64 into
//    partial[level][plane][tile].
// 2. msssim_tail<Src, KS>: from the first level whose plane fits one halo, one workgroup per plane
//    stages the plane in LDS and walks it, pools inside LDS into a second (ping-pong) image that is
//    shifted by that level's own first pixel, and after one barrier walks that, through level M - 1:
//    no global round trip between those levels.  One partial per (plane, level).
// 3. msssim_finish: one workgroup.  Per plane each level's partials are added in a fixed order in
//    FP64, divided by the level's output count, clamped at 0 and raised to beta_j (FP64 pow); the
//    planes of an image are averaged in channel order; the [N] float32 values or their mean are
//    stored and (class update) the sum of the values and N are added to the two float64 states.
//
// No atomics, no host synchronisation and no waiting between workgroups: the result is deterministic.
#include <hip/hip_runtime.h>

#include <cstdint>

#include "tea_common.h"
#include "tea_kernels.h"

namespace tea {
namespace {

constexpr int kT = 256;                           // 4 waves, one per band of output rows
constexpr int kBand = kSsimTileH / (kT / kWave);  // 16 output rows per thread
constexpr int kFT = 1024;                         // finish: one workgroup
constexpr int kSrcPairs = -1;                     // Src: a DType, or the (x, y) pair workspace
static_assert(kSsimTileW == kWave, "one lane per output column");
static_assert((kSsimTileH & 1) == 0 && (kSsimTileW & 1) == 0, "no 2 x 2 block straddles two tiles");

struct Taps {
  float g[kSsimMaxKs];
};

struct FinishLevels {
  int levels;
  long long per[kMsssimMaxLevels];  // partials per plane
  long long off[kMsssimMaxLevels];  // first partial of the level (all planes of earlier levels)
  double count[kMsssimMaxLevels];   // output positions of a plane
  double beta[kMsssimMaxLevels];
};

// an (x, y) pair: one 8-byte LDS or workspace access per pixel
typedef float v2f __attribute__((ext_vector_type(2)));

// byte offsets into the dynamic LDS region (all multiples of 16)
constexpr int kLdsWave = 0;    // [kMsssimMaxLevels][4] double wave totals
constexpr int kLdsTaps = 256;  // [16] float taps (runtime window size)
constexpr int kLdsXY = 320;    // the halo (level) or the two ping-pong images (tail)

__host__ __device__ constexpr int halo_pairs(int ks) { return (kSsimTileH + ks - 1) * (kSsimTileW + ks - 1); }
// the tail's second image: a pooled plane of at most half the halo's sides, kept a multiple of 16 bytes
__host__ __device__ constexpr int pooled_pairs(int ks) {
  return (((kSsimTileH + ks - 1) / 2) * ((kSsimTileW + ks - 1) / 2) + 1) & ~1;
}

template <int Src>
__device__ __forceinline__ v2f load_pair(const void* x, const void* y, int64_t i) {
  v2f v;
  if constexpr (Src == kSrcPairs) {
    v = static_cast<const v2f*>(x)[i];
  } else {
    v.x = load_as_f32(x, static_cast<DType>(Src), i);
    v.y = load_as_f32(y, static_cast<DType>(Src), i);
  }
  return v;
}

// K12's band walk over an LDS pair image of row pitch `pitch`: `bxy` is the first halo row of the
// wave's band at the lane's column.  The thread walks `rows` (wave-uniform, <= kBand + ks - 1) halo
// rows, forms the five horizontal moments of each and adds them into every output row whose vertical
// window holds that row.  Per output row: (sum g x, sum g y), (sum g x^2, sum g y^2), sum g x y.
template <int KS>
__device__ __forceinline__ void band_walk(const v2f* bxy, int pitch, int ks, int rows, const Taps& taps,
                                          const float* s_tap, v2f (&acc1)[kBand], v2f (&acc2)[kBand],
                                          float (&accxy)[kBand]) {
  auto tap = [&](int j) -> float { return KS ? taps.g[j] : s_tap[j]; };
#pragma unroll
  for (int o = 0; o < kBand; ++o) {
    acc1[o] = 0.f;
    acc2[o] = 0.f;
    accxy[o] = 0.f;
  }
  auto row_step = [&](int r) {
    v2f h1 = 0.f, h2 = 0.f;
    float hxy = 0.f;
    const v2f* p = bxy + r * pitch;
#pragma unroll
    for (int j = 0; j < (KS ? KS : ks); ++j) {
      const v2f v = p[j];
      const v2f gv = tap(j) * v;
      h1 += gv;
      h2 = gv * v + h2;
      hxy = fmaf(gv.x, v.y, hxy);
    }
#pragma unroll
    for (int o = 0; o < kBand; ++o) {
      const int t = r - o;  // wave-uniform
      if (t >= 0 && t < ks) {
        const float g = tap(t);
        acc1[o] = g * h1 + acc1[o];
        acc2[o] = g * h2 + acc2[o];
        accxy[o] = fmaf(g, hxy, accxy[o]);
      }
    }
  };
  if (KS) {
#pragma unroll
    for (int r = 0; r < kBand + KS - 1; ++r)
      if (r < rows) row_step(r);
  } else {
#pragma nounroll
    for (int r = 0; r < rows; ++r) row_step(r);
  }
}

// The thread's FP64 sum of cs (Lum = false) or ssim (Lum = true) over its band's output rows
// [oy0, oy0 + kBand) at column ox; rows and columns past (ho, wo) are masked out.  `shift` is what
// the image in LDS was shifted by.
template <bool Lum>
__device__ __forceinline__ double band_value(const v2f (&acc1)[kBand], const v2f (&acc2)[kBand],
                                             const float (&accxy)[kBand], v2f shift, float c1, float c2, int oy0,
                                             int ox, int ho, int wo) {
  double sum = 0.0;
#pragma unroll
  for (int o = 0; o < kBand; ++o) {
    const float dx = acc1[o].x, dy = acc1[o].y;  // means of the shifted inputs
    const float sxx = fmaf(-dx, dx, acc2[o].x);
    const float syy = fmaf(-dy, dy, acc2[o].y);
    const float sxy = fmaf(-dx, dy, accxy[o]);
    float num = fmaf(2.f, sxy, c2);
    float den = sxx + syy + c2;
    if (Lum) {
      const float mx = dx + shift.x, my = dy + shift.y;
      num *= fmaf(2.f * mx, my, c1);
      den *= fmaf(mx, mx, fmaf(my, my, c1));
    }
    const float v = num / den;
    sum += (oy0 + o < ho && ox < wo) ? static_cast<double>(v) : 0.0;
  }
  return sum;
}

// KS: the window size at compile time, or 0 for a runtime-bound loop (taps from LDS).
// x, y: the level's planes [planes][H][W] (Src a DType), or x alone as (x, y) pairs (kSrcPairs).
// pooled: level j + 1 of the workspace, [planes][H / 2][W / 2] pairs (unless Last).
template <int Src, int KS, bool Last>
__global__ __launch_bounds__(kT) void msssim_level_kernel(const void* __restrict__ x, const void* __restrict__ y,
                                                          int H, int W, int ks_rt, Taps taps, float c1, float c2,
                                                          v2f* __restrict__ pooled, double* __restrict__ partial) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  const int ks = KS ? KS : ks_rt;
  const int hw = kSsimTileW + ks - 1;
  const int hh = kSsimTileH + ks - 1;
  double* s_wave = reinterpret_cast<double*>(smem + kLdsWave);
  float* s_tap = reinterpret_cast<float*>(smem + kLdsTaps);
  v2f* halo_xy = reinterpret_cast<v2f*>(smem + kLdsXY);

  const int tid = threadIdx.x;
  const int64_t plane = blockIdx.x;
  const int row0 = blockIdx.z * kSsimTileH;
  const int col0 = blockIdx.y * kSsimTileW;
  const int64_t base = plane * H * W;
  const int64_t origin = base + static_cast<int64_t>(row0) * W + col0;  // always inside the plane
  const v2f a = load_pair<Src>(x, y, origin);

  if (!KS) {
#pragma unroll
    for (int j = 0; j < kSsimMaxKs; ++j)
      if (tid == j) s_tap[j] = taps.g[j];
  }
  // halo staging as in K12: consecutive lanes take consecutive columns of a halo row, elements past
  // the plane's edge (only ever read by masked outputs) load the origin instead and store 0, and the
  // loads of a chunk are all issued before the first is used
  const int halo = hh * hw;
  constexpr int kChunk = KS ? (halo_pairs(KS ? KS : 3) + kT - 1) / kT : 8;
  for (int i0 = tid; i0 < halo; i0 += kChunk * kT) {
    v2f v[kChunk];
    bool ok[kChunk];
#pragma unroll
    for (int u = 0; u < kChunk; ++u) {
      const int i = i0 + u * kT;
      const int r = i / hw;
      const int c = i - r * hw;
      const int gr = row0 + r, gc = col0 + c;
      ok[u] = i < halo && gr < H && gc < W;
      v[u] = load_pair<Src>(x, y, ok[u] ? base + static_cast<int64_t>(gr) * W + gc : origin);
    }
#pragma unroll
    for (int u = 0; u < kChunk; ++u) {
      const int i = i0 + u * kT;
      v2f s = v[u] - a;
      if (!ok[u]) s = 0.f;
      if (i < halo) halo_xy[i] = s;
    }
  }
  __syncthreads();

  if (!Last) {
    // the block owns the level's rows [row0, row0 + 64) (the last tile row: through H) and the same
    // columns; all of them lie in the halo, since the last tile's H - row0 is at most 64 + ks - 1
    const int own_r = blockIdx.z + 1 == gridDim.z ? H - row0 : kSsimTileH;
    const int own_c = blockIdx.y + 1 == gridDim.y ? W - col0 : kSsimTileW;
    const int pr = own_r >> 1, pc = own_c >> 1;  // an odd trailing row or column is dropped
    const int h2 = H >> 1, w2 = W >> 1;
    v2f* dst = pooled + plane * h2 * w2 + static_cast<int64_t>(row0 >> 1) * w2 + (col0 >> 1);
    for (int i = tid; i < pr * pc; i += kT) {
      const int r = i / pc;
      const int c = i - r * pc;
      const v2f* p = halo_xy + 2 * r * hw + 2 * c;
      const v2f s = 0.25f * ((p[0] + p[1]) + (p[hw] + p[hw + 1]));
      dst[static_cast<int64_t>(r) * w2 + c] = s + a;
    }
  }

  const int c = tid & (kWave - 1);
  const int band = __builtin_amdgcn_readfirstlane(tid >> 6);
  v2f acc1[kBand], acc2[kBand];
  float accxy[kBand];
  band_walk<KS>(halo_xy + band * kBand * hw + c, hw, ks, kBand + ks - 1, taps, s_tap, acc1, acc2, accxy);
  double sum =
      band_value<Last>(acc1, acc2, accxy, a, c1, c2, row0 + band * kBand, col0 + c, H - ks + 1, W - ks + 1);
  sum = wave_sum(sum);
  if (c == 0) s_wave[band] = sum;
  __syncthreads();
  if (tid == 0) {
    const int64_t tiles = static_cast<int64_t>(gridDim.y) * gridDim.z;
    const int64_t tile = static_cast<int64_t>(blockIdx.z) * gridDim.y + blockIdx.y;
    partial[plane * tiles + tile] = (s_wave[0] + s_wave[1]) + (s_wave[2] + s_wave[3]);
  }
}

// One workgroup per plane: levels [tail, M) of the pyramid, `levels` of them, out of LDS.  H x W is
// the first of them (at most (64 + ks - 1)^2), read from x, y as in the level kernel.  Image B (the
// pooled plane) lies before image A (the staged plane), so the walk's reads past a small image, which
// only masked outputs take, stay inside the allocation.  partial: [levels][planes].
template <int Src, int KS>
__global__ __launch_bounds__(kT) void msssim_tail_kernel(const void* __restrict__ x, const void* __restrict__ y,
                                                         int H, int W, int levels, int ks_rt, Taps taps, float c1,
                                                         float c2, double* __restrict__ partial) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  const int ks = KS ? KS : ks_rt;
  double* s_wave = reinterpret_cast<double*>(smem + kLdsWave);
  float* s_tap = reinterpret_cast<float*>(smem + kLdsTaps);
  v2f* img_b = reinterpret_cast<v2f*>(smem + kLdsXY);
  v2f* img_a = img_b + pooled_pairs(ks);

  const int tid = threadIdx.x;
  const int64_t plane = blockIdx.x;
  const int64_t base = plane * H * W;
  v2f a = load_pair<Src>(x, y, base);

  if (!KS) {
#pragma unroll
    for (int j = 0; j < kSsimMaxKs; ++j)
      if (tid == j) s_tap[j] = taps.g[j];
  }
  // the plane is contiguous in memory and in LDS (row pitch W)
  const int pixels = H * W;
  constexpr int kChunk = KS ? (halo_pairs(KS ? KS : 3) + kT - 1) / kT : 8;
  for (int i0 = tid; i0 < pixels; i0 += kChunk * kT) {
    v2f v[kChunk];
#pragma unroll
    for (int u = 0; u < kChunk; ++u) {
      const int i = i0 + u * kT;
      v[u] = load_pair<Src>(x, y, base + (i < pixels ? i : 0));
    }
#pragma unroll
    for (int u = 0; u < kChunk; ++u) {
      const int i = i0 + u * kT;
      if (i < pixels) img_a[i] = v[u] - a;
    }
  }
  __syncthreads();

  const int c = tid & (kWave - 1);
  const int band = __builtin_amdgcn_readfirstlane(tid >> 6);
  v2f* cur = img_a;
  v2f* nxt = img_b;
  int h = H, w = W;
  for (int l = 0; l < levels; ++l) {
    const bool last = l + 1 == levels;
    const int h2 = h >> 1, w2 = w >> 1;
    v2f a2 = a;
    if (!last) {
      // pool into the other image, shifted by the pooled level's own first pixel (every thread
      // forms it from the same four words)
      const v2f p00 = 0.25f * ((cur[0] + cur[1]) + (cur[w] + cur[w + 1]));
      a2 = p00 + a;
      for (int i = tid; i < h2 * w2; i += kT) {
        const int r = i / w2;
        const int cc = i - r * w2;
        const v2f* p = cur + 2 * r * w + 2 * cc;
        nxt[i] = 0.25f * ((p[0] + p[1]) + (p[w] + p[w + 1])) - p00;
      }
    }
    const int ho = h - ks + 1, wo = w - ks + 1;
    const int left = ho - band * kBand;  // output rows of this band and below
    double sum = 0.0;
    if (left > 0) {
      const int rows = (left < kBand ? left : kBand) + ks - 1;
      v2f acc1[kBand], acc2[kBand];
      float accxy[kBand];
      band_walk<KS>(cur + band * kBand * w + c, w, ks, rows, taps, s_tap, acc1, acc2, accxy);
      sum = last ? band_value<true>(acc1, acc2, accxy, a, c1, c2, band * kBand, c, ho, wo)
                 : band_value<false>(acc1, acc2, accxy, a, c1, c2, band * kBand, c, ho, wo);
      sum = wave_sum(sum);
    }
    if (c == 0) s_wave[l * 4 + band] = sum;
    __syncthreads();  // the level's wave totals, the pooled image, and every read of `cur` done
    if (tid == 0) {
      const double* s = s_wave + l * 4;
      partial[static_cast<int64_t>(l) * gridDim.x + plane] = (s[0] + s[1]) + (s[2] + s[3]);
    }
    v2f* t = cur;
    cur = nxt;
    nxt = t;
    h = h2;
    w = w2;
    a = a2;
  }
}

// ``group`` (a power of two <= 64) lanes share one image: for each of its planes and levels they
// stride over the partials and combine by xor shuffles below ``group`` (K12's finish).
__global__ __launch_bounds__(kFT) void msssim_finish_kernel(const double* __restrict__ partial, FinishLevels f,
                                                           int64_t n_img, int channels, int group,
                                                           float* __restrict__ out, int mean,
                                                           double* __restrict__ value_sum,
                                                           double* __restrict__ num_images) {
  __shared__ double s_wave[kFT / kWave];
  const int tid = threadIdx.x;
  const int sub = tid & (group - 1);
  const int64_t slot = tid / group;
  const int64_t slots = kFT / group;
  double total = 0.0;
  for (int64_t img0 = 0; img0 < n_img; img0 += slots) {  // uniform trip counts throughout
    const int64_t img = img0 + slot;
    const bool live = img < n_img;
    double value = 0.0;
    for (int ch = 0; ch < channels; ++ch) {
      const int64_t plane = img * channels + ch;
      double prod = 1.0;
      for (int j = 0; j < f.levels; ++j) {
        const int64_t per = f.per[j];
        double acc = 0.0;
        if (live) {
          const double* p = partial + f.off[j] + plane * per;
          for (int64_t k = sub; k < per; k += group) acc += p[k];
        }
        for (int o = group >> 1; o > 0; o >>= 1) acc += __shfl_xor(acc, o, kWave);
        double m = acc / f.count[j];
        m = m < 0.0 ? 0.0 : m;  // a NaN stays
        prod *= pow(m, f.beta[j]);
      }
      value += prod;
    }
    value /= static_cast<double>(channels);
    if (live && sub == 0) {
      if (out != nullptr && !mean) out[img] = static_cast<float>(value);
      total += value;
    }
  }
  total = wave_sum(total);
  if ((tid & (kWave - 1)) == 0) s_wave[tid >> 6] = total;
  __syncthreads();
  if (tid == 0) {
    double t = 0.0;
    for (int w = 0; w < kFT / kWave; ++w) t += s_wave[w];
    if (out != nullptr && mean) out[0] = static_cast<float>(t / static_cast<double>(n_img));
    if (value_sum != nullptr) {
      *value_sum += t;
      *num_images += static_cast<double>(n_img);
    }
  }
}

struct LevelLaunch {
  const void* x;
  const void* y;
  int h, w, ks;
  Taps taps;
  float c1, c2;
  v2f* pooled;      // level kernel, unless last
  int levels;       // tail kernel
  double* partial;
  dim3 grid;
  size_t lds;
  hipStream_t stream;
};

template <int Src, int KS>
void launch_level(const LevelLaunch& l, bool last) {
  if (last) {
    hipLaunchKernelGGL((msssim_level_kernel<Src, KS, true>), l.grid, dim3(kT), l.lds, l.stream, l.x, l.y, l.h, l.w,
                       l.ks, l.taps, l.c1, l.c2, l.pooled, l.partial);
  } else {
    hipLaunchKernelGGL((msssim_level_kernel<Src, KS, false>), l.grid, dim3(kT), l.lds, l.stream, l.x, l.y, l.h, l.w,
                       l.ks, l.taps, l.c1, l.c2, l.pooled, l.partial);
  }
}

template <int Src, int KS>
void launch_tail(const LevelLaunch& l) {
  hipLaunchKernelGGL((msssim_tail_kernel<Src, KS>), l.grid, dim3(kT), l.lds, l.stream, l.x, l.y, l.h, l.w, l.levels,
                     l.ks, l.taps, l.c1, l.c2, l.partial);
}

// tail: the tail launch; otherwise a level launch, the pyramid's last level when `last`
template <int Src>
void launch_src(const LevelLaunch& l, bool tail, bool last) {
  if (tail) {
    l.ks == 11 ? launch_tail<Src, 11>(l) : launch_tail<Src, 0>(l);
  } else {
    l.ks == 11 ? launch_level<Src, 11>(l, last) : launch_level<Src, 0>(l, last);
  }
}

int launch_one(const LevelLaunch& l, bool pairs, DType dt, bool tail, bool last) {
  if (pairs) {
    launch_src<kSrcPairs>(l, tail, last);
    return 0;
  }
  switch (dt) {
    case DType::f32: launch_src<static_cast<int>(DType::f32)>(l, tail, last); break;
    case DType::f16: launch_src<static_cast<int>(DType::f16)>(l, tail, last); break;
    case DType::bf16: launch_src<static_cast<int>(DType::bf16)>(l, tail, last); break;
    case DType::u8: launch_src<static_cast<int>(DType::u8)>(l, tail, last); break;
    default: return 1;
  }
  return 0;
}

}  // namespace

// msssim_geometry_ok and msssim_plan have a twin each in torcheval_amd/ops/msssim.py (`supported`, `plan`),
// which sizes the workspace and the partials: change both together.  The binding checks the two buffers
// against this plan, so a twin that falls behind fails the call, it never writes out of bounds.
bool msssim_geometry_ok(int64_t planes, int64_t h, int64_t w, int64_t ks, int64_t levels) {
  if (levels < 1 || levels > kMsssimMaxLevels || !ssim_geometry_ok(planes, h, w, ks)) return false;
  return (h >> (levels - 1)) >= ks && (w >> (levels - 1)) >= ks;
}

MsssimPlan msssim_plan(int64_t h, int64_t w, int64_t ks, int64_t levels) {
  MsssimPlan p;
  p.levels = static_cast<int>(levels);
  p.tail = p.levels;
  for (int j = 0; j < p.levels; ++j) {
    p.h[j] = static_cast<int>(h >> j);
    p.w[j] = static_cast<int>(w >> j);
    if (p.tail == p.levels && p.h[j] <= kSsimTileH + ks - 1 && p.w[j] <= kSsimTileW + ks - 1) p.tail = j;
    p.per[j] = j < p.tail ? ssim_tiles(p.h[j], p.w[j], ks) : 1;
    p.part_off[j] = p.partials;
    p.partials += p.per[j];
    if (j >= 1 && j <= p.tail) {  // written by level launch j - 1
      p.ws_off[j] = p.ws_pairs;
      p.ws_pairs += static_cast<int64_t>(p.h[j]) * p.w[j];
    }
  }
  return p;
}

int launch_msssim(const MsssimArgs& a, hipStream_t stream) {
  const int64_t planes = a.n * a.c;
  if (!msssim_geometry_ok(planes, a.h, a.w, a.ks, a.levels) || a.partial == nullptr) return 1;
  const MsssimPlan p = msssim_plan(a.h, a.w, a.ks, a.levels);
  if (p.ws_pairs > 0 && a.workspace == nullptr) return 1;
  v2f* ws = reinterpret_cast<v2f*>(a.workspace);

  LevelLaunch l;
  for (int j = 0; j < kSsimMaxKs; ++j) l.taps.g[j] = j < a.ks ? a.taps[j] : 0.f;
  l.ks = a.ks;
  l.c1 = a.c1;
  l.c2 = a.c2;
  l.stream = stream;
  FinishLevels f;
  f.levels = p.levels;
  const int launches = p.tail < p.levels ? p.tail + 1 : p.levels;
  for (int j = 0; j < launches; ++j) {
    const bool tail = j == p.tail;
    const bool pairs = j > 0;
    l.x = pairs ? static_cast<const void*>(ws + planes * p.ws_off[j]) : a.x;
    l.y = pairs ? nullptr : a.y;
    l.h = p.h[j];
    l.w = p.w[j];
    l.partial = a.partial + planes * p.part_off[j];
    if (tail) {
      l.pooled = nullptr;
      l.levels = p.levels - p.tail;
      l.grid = dim3(static_cast<unsigned>(planes));
      l.lds = kLdsXY + static_cast<size_t>(pooled_pairs(a.ks) + halo_pairs(a.ks)) * sizeof(v2f);
    } else {
      const bool last = j + 1 == p.levels;
      l.pooled = last ? nullptr : ws + planes * p.ws_off[j + 1];
      l.levels = 1;
      const unsigned ty = (l.h - a.ks + 1 + kSsimTileH - 1) / kSsimTileH;
      const unsigned tx = (l.w - a.ks + 1 + kSsimTileW - 1) / kSsimTileW;
      l.grid = dim3(static_cast<unsigned>(planes), tx, ty);
      l.lds = kLdsXY + static_cast<size_t>(halo_pairs(a.ks)) * sizeof(v2f);
    }
    if (launch_one(l, pairs, a.dt, tail, !tail && j + 1 == p.levels) != 0) return 1;
  }
  int64_t most = 1;
  for (int j = 0; j < p.levels; ++j) {
    f.per[j] = p.per[j];
    f.off[j] = planes * p.part_off[j];
    f.count[j] = static_cast<double>(p.h[j] - a.ks + 1) * (p.w[j] - a.ks + 1);
    f.beta[j] = a.betas[j];
    most = p.per[j] > most ? p.per[j] : most;
  }
  for (int j = p.levels; j < kMsssimMaxLevels; ++j) {
    f.per[j] = 0;
    f.off[j] = 0;
    f.count[j] = 1.0;
    f.beta[j] = 0.0;
  }
  int group = 1;
  while (group < kWave && group < most) group <<= 1;
  hipLaunchKernelGGL(msssim_finish_kernel, dim3(1), dim3(kFT), 0, stream, a.partial, f, a.n, static_cast<int>(a.c),
                     group, a.out, a.mean, a.value_sum, a.num_images);
  return hipGetLastError() == hipSuccess ? 0 : 2;
}

}  // namespace tea
