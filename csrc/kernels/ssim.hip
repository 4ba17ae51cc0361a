// K12: structural similarity (SSIM) of [N, C, H, W] image pairs in two launches.
//
// Not in the reference tree; the definition is docs/parity.md "Structural similarity": a
// separable Gaussian window g (x) g applied "valid" to x, y, x^2, y^2 and xy, the Wang et al.
// expression per output pixel, the mean over each image's channels and positions.
//
// 1. ssim_tiles: one workgroup per (plane, 64 x 64 output tile).  The (64 + ks - 1)^2 halo of
//    x and y is staged once into LDS as interleaved FP32 (x, y) pairs (converted from the input
//    dtype on load).  Wave b owns the tile's output rows [16 b, 16 b + 16) and lane c its column
//    c: the thread walks the 16 + ks - 1 halo rows of its band, forms the five horizontal
//    moments of each row from LDS (lanes read consecutive 8-byte words: no bank conflicts) and
//    scatters them into the (at most 16) output rows whose vertical window holds that row, so
//    the horizontal moments never go back to LDS; a band of 16 rows recomputes 26 / 16 of the
//    horizontal work at ks = 11, a band of 8 would recompute 18 / 8.  The x and y halves of a
//    pair go through packed FP32 instructions.  The SSIM values are formed in FP32 with FMA and
//    summed in FP64 (thread, wave shuffles, the 4 wave totals in order) into
//    partial[plane][tile]; lanes and rows past the plane's last output are masked out.
//    Both inputs are shifted by the tile's first pixel before the moments are formed: the
//    (co)variances do not depend on the shift, and F(x^2) - F(x)^2 of a nearly flat image no
//    longer cancels from the size of x^2 down to the size of the variance.
// 2. ssim_finish: one workgroup sums each image's partials in a fixed order in FP64, divides by
//    C H' W', stores the [N] float32 values or their mean, and (class update) adds the sum of
//    the N values to mssim_sum and N to num_images.
//
// No atomics and no waiting between workgroups: the result is deterministic.
#include <hip/hip_runtime.h>

#include <cstdint>

#include "tea_common.h"
#include "tea_kernels.h"

namespace tea {
namespace {

constexpr int kT = 256;                     // 4 waves, one per band of output rows
constexpr int kBand = kSsimTileH / (kT / kWave);  // 16 output rows per thread
constexpr int kFT = 1024;                   // finish: one workgroup
static_assert(kSsimTileW == kWave, "one lane per output column");

struct Taps {
  float g[kSsimMaxKs];
};

// an (x, y) pair: one 8-byte LDS access per pixel, and arithmetic on both halves at once
// (packed FP32 instructions)
typedef float v2f __attribute__((ext_vector_type(2)));

// byte offsets into the dynamic LDS region (all multiples of 16, Guideline 17)
constexpr int kLdsWave = 0;   // [4] double wave totals
constexpr int kLdsTaps = 32;  // [16] float taps (runtime window size)
constexpr int kLdsXY = 96;    // the halo, (x, y) interleaved

__host__ __device__ constexpr int halo_pairs(int ks) { return (kSsimTileH + ks - 1) * (kSsimTileW + ks - 1); }

// KS: the window size at compile time, or 0 for a runtime-bound loop (taps from LDS)
template <DType DT, int KS>
__global__ __launch_bounds__(kT) void ssim_tiles_kernel(const void* __restrict__ x, const void* __restrict__ y, int H,
                                                        int W, int ks_rt, Taps taps, float c1, float c2,
                                                        double* __restrict__ partial) {
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
  const float ax = load_as_f32(x, DT, origin);
  const float ay = load_as_f32(y, DT, origin);

  if (!KS) {
#pragma unroll
    for (int j = 0; j < kSsimMaxKs; ++j)
      if (tid == j) s_tap[j] = taps.g[j];
  }
  // halo staging: consecutive lanes take consecutive columns of a halo row; elements past the
  // plane's edge (only ever read by masked outputs) load the origin instead and store 0
  // The loads of a chunk are all issued before the first is used: staging is bound by memory
  // latency, so the whole halo is in flight at once at ks = 11 (2 x 22 loads per thread).
  const int halo = hh * hw;
  constexpr int kChunk = KS ? (halo_pairs(KS ? KS : 3) + kT - 1) / kT : 8;
  for (int i0 = tid; i0 < halo; i0 += kChunk * kT) {
    float vx[kChunk], vy[kChunk];
    bool ok[kChunk];
#pragma unroll
    for (int u = 0; u < kChunk; ++u) {
      const int i = i0 + u * kT;
      const int r = i / hw;
      const int c = i - r * hw;
      const int gr = row0 + r, gc = col0 + c;
      ok[u] = i < halo && gr < H && gc < W;
      const int64_t idx = ok[u] ? base + static_cast<int64_t>(gr) * W + gc : origin;
      vx[u] = load_as_f32(x, DT, idx);
      vy[u] = load_as_f32(y, DT, idx);
    }
#pragma unroll
    for (int u = 0; u < kChunk; ++u) {
      const int i = i0 + u * kT;
      v2f v;
      v.x = ok[u] ? vx[u] - ax : 0.f;
      v.y = ok[u] ? vy[u] - ay : 0.f;
      if (i < halo) halo_xy[i] = v;
    }
  }
  __syncthreads();

  const int c = tid & (kWave - 1);
  const int band = __builtin_amdgcn_readfirstlane(tid >> 6);
  const v2f* bxy = halo_xy + band * kBand * hw + c;  // lanes read consecutive 8-byte words: no conflicts
  auto tap = [&](int j) -> float { return KS ? taps.g[j] : s_tap[j]; };

  // per output row: (sum g x, sum g y), (sum g x^2, sum g y^2), sum g x y
  v2f acc1[kBand], acc2[kBand];
  float accxy[kBand];
#pragma unroll
  for (int o = 0; o < kBand; ++o) {
    acc1[o] = 0.f;
    acc2[o] = 0.f;
    accxy[o] = 0.f;
  }

  // one halo row of the band: horizontal moments, then into every output row that holds it
  auto row_step = [&](int r) {
    v2f h1 = 0.f, h2 = 0.f;
    float hxy = 0.f;
    const v2f* p = bxy + r * hw;
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
    for (int r = 0; r < kBand + KS - 1; ++r) row_step(r);
  } else {
#pragma nounroll
    for (int r = 0; r < kBand + ks - 1; ++r) row_step(r);
  }

  const int ho = H - ks + 1, wo = W - ks + 1;
  const int ox = col0 + c;
  double sum = 0.0;
#pragma unroll
  for (int o = 0; o < kBand; ++o) {
    const int oy = row0 + band * kBand + o;
    const float dx = acc1[o].x, dy = acc1[o].y;  // means of the shifted inputs
    const float sxx = fmaf(-dx, dx, acc2[o].x);
    const float syy = fmaf(-dy, dy, acc2[o].y);
    const float sxy = fmaf(-dx, dy, accxy[o]);
    const float mx = dx + ax, my = dy + ay;
    const float num = fmaf(2.f * mx, my, c1) * fmaf(2.f, sxy, c2);
    const float den = (fmaf(mx, mx, fmaf(my, my, c1))) * (sxx + syy + c2);
    const float v = num / den;
    sum += (oy < ho && ox < wo) ? static_cast<double>(v) : 0.0;
  }
  sum = wave_sum(sum);
  if (c == 0) s_wave[band] = sum;
  __syncthreads();
  if (tid == 0) {
    const int64_t tiles = static_cast<int64_t>(gridDim.y) * gridDim.z;
    const int64_t tile = static_cast<int64_t>(blockIdx.z) * gridDim.y + blockIdx.y;
    partial[plane * tiles + tile] = (s_wave[0] + s_wave[1]) + (s_wave[2] + s_wave[3]);
  }
}

// ``group`` (a power of two <= 64) lanes share one image: they stride over its ``per`` partials
// and combine by xor shuffles below ``group``, so a wave finishes 64 / group images per round
// (one image per lane for single-tile images, one per wave for large ones).
__global__ __launch_bounds__(kFT) void ssim_finish_kernel(const double* __restrict__ partial, int64_t n_img,
                                                         int64_t per, int group, double count,
                                                         float* __restrict__ out, int mean,
                                                         double* __restrict__ mssim_sum,
                                                         double* __restrict__ num_images) {
  __shared__ double s_wave[kFT / kWave];
  const int tid = threadIdx.x;
  const int sub = tid & (group - 1);
  const int64_t slot = tid / group;
  const int64_t slots = kFT / group;
  double total = 0.0;
  for (int64_t img0 = 0; img0 < n_img; img0 += slots) {  // uniform trip count
    const int64_t img = img0 + slot;
    double acc = 0.0;
    if (img < n_img) {
      const double* p = partial + img * per;
      for (int64_t k = sub; k < per; k += group) acc += p[k];
    }
    for (int o = group >> 1; o > 0; o >>= 1) acc += __shfl_xor(acc, o, kWave);
    if (img < n_img && sub == 0) {
      const double v = acc / count;
      if (out != nullptr && !mean) out[img] = static_cast<float>(v);
      total += v;
    }
  }
  total = wave_sum(total);
  if ((tid & (kWave - 1)) == 0) s_wave[tid >> 6] = total;
  __syncthreads();
  if (tid == 0) {
    double t = 0.0;
    for (int w = 0; w < kFT / kWave; ++w) t += s_wave[w];
    if (out != nullptr && mean) out[0] = static_cast<float>(t / static_cast<double>(n_img));
    if (mssim_sum != nullptr) {
      *mssim_sum += t;
      *num_images += static_cast<double>(n_img);
    }
  }
}

template <DType DT>
void launch_tiles(const SsimArgs& a, dim3 grid, size_t lds, const Taps& taps, hipStream_t stream) {
  if (a.ks == 11) {
    hipLaunchKernelGGL((ssim_tiles_kernel<DT, 11>), grid, dim3(kT), lds, stream, a.x, a.y, a.h, a.w, a.ks, taps, a.c1,
                       a.c2, a.partial);
  } else {
    hipLaunchKernelGGL((ssim_tiles_kernel<DT, 0>), grid, dim3(kT), lds, stream, a.x, a.y, a.h, a.w, a.ks, taps, a.c1,
                       a.c2, a.partial);
  }
}

}  // namespace

int64_t ssim_tiles(int64_t h, int64_t w, int64_t ks) {
  const int64_t ty = (h - ks + 1 + kSsimTileH - 1) / kSsimTileH;
  const int64_t tx = (w - ks + 1 + kSsimTileW - 1) / kSsimTileW;
  return ty * tx;
}

bool ssim_geometry_ok(int64_t planes, int64_t h, int64_t w, int64_t ks) {
  if (ks < 3 || ks > kSsimMaxKs || (ks & 1) == 0 || h < ks || w < ks || planes < 1) return false;
  if (h > INT32_MAX || w > INT32_MAX || planes > kSsimMaxPlanes) return false;
  const int64_t ty = (h - ks + 1 + kSsimTileH - 1) / kSsimTileH;
  const int64_t tx = (w - ks + 1 + kSsimTileW - 1) / kSsimTileW;
  return ty <= 65535 && tx <= 65535;
}

int launch_ssim(const SsimArgs& a, hipStream_t stream) {
  const int64_t planes = a.n * a.c;
  if (!ssim_geometry_ok(planes, a.h, a.w, a.ks) || a.partial == nullptr) return 1;
  const int ho = a.h - a.ks + 1, wo = a.w - a.ks + 1;
  const unsigned ty = (ho + kSsimTileH - 1) / kSsimTileH;
  const unsigned tx = (wo + kSsimTileW - 1) / kSsimTileW;
  const dim3 grid(static_cast<unsigned>(planes), tx, ty);
  const size_t lds = kLdsXY + static_cast<size_t>(halo_pairs(a.ks)) * sizeof(v2f);
  Taps taps;
  for (int j = 0; j < kSsimMaxKs; ++j) taps.g[j] = j < a.ks ? a.taps[j] : 0.f;
  switch (a.dt) {
    case DType::f32: launch_tiles<DType::f32>(a, grid, lds, taps, stream); break;
    case DType::f16: launch_tiles<DType::f16>(a, grid, lds, taps, stream); break;
    case DType::bf16: launch_tiles<DType::bf16>(a, grid, lds, taps, stream); break;
    case DType::u8: launch_tiles<DType::u8>(a, grid, lds, taps, stream); break;
    default: return 1;
  }
  const int64_t per = a.c * static_cast<int64_t>(tx) * ty;
  int group = 1;
  while (group < kWave && group < per) group <<= 1;
  const double count = static_cast<double>(a.c) * ho * wo;
  hipLaunchKernelGGL(ssim_finish_kernel, dim3(1), dim3(kFT), 0, stream, a.partial, a.n, per, group, count, a.out,
                     a.mean, a.mssim_sum, a.num_images);
  return hipGetLastError() == hipSuccess ? 0 : 2;
}

}  // namespace tea
