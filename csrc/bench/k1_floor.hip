// K1 floor harness: the production micro-accuracy launch against a
// pure-read kernel of the SAME geometry over the SAME 8-batch pool (bench.py's shape:
// [8192, 1000] fp32 logits + int64 targets per batch, 262 MB > the 256 MiB MALL), and an
// empty launch of the same grid.  Back-to-back launches timed with events, so every number
// includes the per-launch boundary exactly as bench.py's loop does.
//
//   prod   launch_cls_counts (classification.hip cls_micro_kernel, pending-cell epilogue)
//   read   one wave per row, 4 x 16-B loads per lane + the target load, lane max only, one
//          store per wave only when an impossible value appears (keeps the loads live)
//   empty  the same 2048 x 256 grid, no work
//   (+ the read floor behind the wide argument struct, with one atomic, with prod's row reduction)
//   read / prod, preloaded   the same two launches from this file's second compile, in which the
//          kernels' plain parameters are preloaded into SGPRs (as torcheval_amd/ops/build.py
//          compiles classification.hip); in the first compile the same kernels fetch them
//          with scalar loads at the head of every wave
//   head variants (preloaded compile, profiles/k1_oneshot_ab.json): what the instructions between
//          a wave's entry point and its row loads cost.  The read floor with 64 / 128 / 256 bytes
//          of s_nop in front of the loads; cls_micro_pend_kernel's head in front of the read
//          body; the loop arm and the one-shot arm of the production launch, launched directly;
//          each at 8 and at 4 waves per workgroup.  Five interleaved rounds, min / median / max.
//
// Two objects from this one file (the preload flag holds for a whole translation unit):
//   hipcc --offload-arch=gfx950 -O3 -std=c++17 -Icsrc/include -c csrc/bench/k1_floor.hip -o k1_floor.o
//   hipcc --offload-arch=gfx950 -O3 -std=c++17 -Icsrc/include -DK1_FLOOR_PRELOAD_UNIT \
//         -mllvm -amdgpu-kernarg-preload-count=16 -c csrc/bench/k1_floor.hip -o k1_floor_preload.o
//   hipcc --offload-arch=gfx950 k1_floor.o k1_floor_preload.o -o csrc/bench/k1_floor.bin
//
// Usage: k1_floor.bin [pool=8] [iters=400]; prints one line per variant.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <vector>

#ifdef K1_FLOOR_PRELOAD_UNIT  // the second copy of the production launchers gets its own names
#define launch_cls_counts launch_cls_counts_preload
#define launch_micro_finish launch_micro_finish_preload
#define launch_binary_counts launch_binary_counts_preload
#endif
#include "../kernels/classification.hip"

using namespace tea;

#define CK(x)                                                          \
  do {                                                                 \
    hipError_t e_ = (x);                                               \
    if (e_ != hipSuccess) {                                            \
      printf("HIP error %s at %d\n", hipGetErrorString(e_), __LINE__); \
      exit(1);                                                         \
    }                                                                  \
  } while (0)

namespace {

constexpr int N = 8192, C = 1000, FSTEP = 256;

__global__ __launch_bounds__(256) void read_floor_kernel(const float* __restrict__ x, const int64_t* __restrict__ y,
                                                         float* __restrict__ sink) {
  const int lane = threadIdx.x & 63;
  const int64_t row = static_cast<int64_t>(blockIdx.x) * 4 + (threadIdx.x >> 6);
  if (row >= N) return;
  const float* rp = x + row * C;
  float m = -__builtin_huge_valf();
#pragma unroll
  for (int u = 0; u < 4; ++u) {
    const int col = u * FSTEP + lane * 4;
    const float4 q = *reinterpret_cast<const float4*>(rp + (col < C ? col : 0));
    m = fmaxf(m, fmaxf(fmaxf(q.x, q.y), fmaxf(q.z, q.w)));
  }
  const int64_t t = y[row];
  if (m == 12345.678f && t == 7) sink[row] = m;  // never true for randn-like data
}

}  // namespace

// the preloaded variants, defined by the K1_FLOOR_PRELOAD_UNIT compile of this file
void k1_floor_read_preload(const float* x, const int64_t* y, float* sink, hipStream_t s);
int k1_floor_prod_preload(const ClsCountsArgs& a, hipStream_t s);
int k1_floor_finish_preload(unsigned long long* pend, float* correct, const float* total, float* out, hipStream_t s);

// the head-attribution variants (profiles/k1_oneshot_ab.json), all preloaded, all 8192 waves
int k1_floor_head_variants();
const char* k1_floor_head_name(int which);
void k1_floor_head_launch(int which, const float* x, const int64_t* y, float* sink, unsigned long long* pend,
                          float* total, hipStream_t s);

#ifdef K1_FLOOR_PRELOAD_UNIT

namespace {

// the pure-read body with WPB waves per workgroup and PAD s_nop (4 bytes each) between the entry
// point and the first load: 16 of them push the loads one 64-byte instruction line further away
template <int WPB, int PAD>
__global__ __launch_bounds__(WPB * 64) void read_pad_kernel(const float* __restrict__ x, const int64_t* __restrict__ y,
                                                            float* __restrict__ sink) {
#pragma unroll
  for (int i = 0; i < PAD; ++i) asm volatile("s_nop 0");
  const int lane = threadIdx.x & 63;
  const int64_t row = static_cast<int64_t>(blockIdx.x) * WPB + (threadIdx.x >> 6);
  const float* rp = x + row * C;
  float m = -__builtin_huge_valf();
#pragma unroll
  for (int u = 0; u < 4; ++u) {
    const int col = u * FSTEP + lane * 4;
    const float4 q = *reinterpret_cast<const float4*>(rp + (col < C ? col : 0));
    m = fmaxf(m, fmaxf(fmaxf(q.x, q.y), fmaxf(q.z, q.w)));
  }
  const int64_t t = y[row];
  if (m == 12345.678f && t == 7) sink[row] = m;
}

// cls_micro_pend_kernel's head (run-time n, c and row_stride, the 64-bit row clamp and multiply,
// a column clamp per load) in front of the pure-read body
template <int WPB>
__global__ __launch_bounds__(WPB * 64) void prodhead_read_kernel(const char* __restrict__ input,
                                                                 const int64_t* __restrict__ target,
                                                                 float* __restrict__ sink, int64_t n,
                                                                 int64_t row_stride, int32_t c) {
  const int lane = lane_id();
  const int64_t row0 = static_cast<int64_t>(blockIdx.x) * WPB + wave_id();
  const int64_t r0 = row0 < n ? row0 : n - 1;
  const char* rp = input + r0 * row_stride * 4;
  float f[4][4];
#pragma unroll
  for (int u = 0; u < 4; ++u) load_row_vec<0, 4, false>(rp, u * FSTEP + lane * 4, c, f[u]);
  const int64_t t = target[r0];
  __builtin_amdgcn_sched_barrier(0);  // as in production, no use of a loaded value ahead of the last load
  float m = fmaximum(f[0][0], f[0][1]);
#pragma unroll
  for (int e = 2; e < 16; ++e) m = fmaximum(m, f[e / 4][e % 4]);
  if (m == 12345.678f && t == 7) sink[r0] = m;
}

constexpr int kHeadVariants = 11;
const char* const kHeadNames[kHeadVariants] = {
    "read floor, 8 waves per workgroup",
    "read floor + 64 B of s_nop",
    "read floor + 128 B of s_nop",
    "read floor + 256 B of s_nop",
    "production head + read body, 8 waves per workgroup",
    "loop arm (cls_micro_pend_kernel), 8 waves per workgroup",
    "one-shot arm (cls_micro_oneshot_kernel), 8 waves per workgroup",
    "read floor, 4 waves per workgroup",
    "production head + read body, 4 waves per workgroup",
    "loop arm (cls_micro_pend_kernel), 4 waves per workgroup",
    "one-shot arm (cls_micro_oneshot_kernel), 4 waves per workgroup",
};

}  // namespace

int k1_floor_head_variants() { return kHeadVariants; }
const char* k1_floor_head_name(int which) { return kHeadNames[which]; }
void k1_floor_head_launch(int which, const float* x, const int64_t* y, float* sink, unsigned long long* pend,
                          float* total, hipStream_t s) {
  const char* in = reinterpret_cast<const char*>(x);
  const dim3 g8(N / 8), b8(512), g4(N / 4), b4(256);
  const int64_t n = N, stride = C;
  const uint32_t n32 = N, row_bytes = C * 4;
  const int32_t c = C;
  switch (which) {
    case 0: hipLaunchKernelGGL((read_pad_kernel<8, 0>), g8, b8, 0, s, x, y, sink); break;
    case 1: hipLaunchKernelGGL((read_pad_kernel<8, 16>), g8, b8, 0, s, x, y, sink); break;
    case 2: hipLaunchKernelGGL((read_pad_kernel<8, 32>), g8, b8, 0, s, x, y, sink); break;
    case 3: hipLaunchKernelGGL((read_pad_kernel<8, 64>), g8, b8, 0, s, x, y, sink); break;
    case 4: hipLaunchKernelGGL((prodhead_read_kernel<8>), g8, b8, 0, s, in, y, sink, n, stride, c); break;
    case 5:
      hipLaunchKernelGGL((cls_micro_pend_kernel<0, int64_t, 8, false>), g8, b8, 0, s, in, y, pend, total, n, stride, c,
                         N);
      break;
    case 6:
      hipLaunchKernelGGL((cls_micro_oneshot_kernel<0, int64_t, 8, C / FSTEP>), g8, b8, 0, s, in, y, pend, total, n32,
                         row_bytes, c);
      break;
    case 7: hipLaunchKernelGGL((read_pad_kernel<4, 0>), g4, b4, 0, s, x, y, sink); break;
    case 8: hipLaunchKernelGGL((prodhead_read_kernel<4>), g4, b4, 0, s, in, y, sink, n, stride, c); break;
    case 9:
      hipLaunchKernelGGL((cls_micro_pend_kernel<0, int64_t, 4, false>), g4, b4, 0, s, in, y, pend, total, n, stride, c,
                         N);
      break;
    default:
      hipLaunchKernelGGL((cls_micro_oneshot_kernel<0, int64_t, 4, C / FSTEP>), g4, b4, 0, s, in, y, pend, total, n32,
                         row_bytes, c);
      break;
  }
}

void k1_floor_read_preload(const float* x, const int64_t* y, float* sink, hipStream_t s) {
  hipLaunchKernelGGL(read_floor_kernel, dim3(N / 4), dim3(256), 0, s, x, y, sink);
}
int k1_floor_prod_preload(const ClsCountsArgs& a, hipStream_t s) { return launch_cls_counts(a, s); }
int k1_floor_finish_preload(unsigned long long* pend, float* correct, const float* total, float* out, hipStream_t s) {
  return launch_micro_finish(pend, correct, total, out, s);
}

#else

namespace {

// the same pure-read body behind the ~200-byte ClsCountsArgs kernel-argument block
__global__ __launch_bounds__(256) void read_floor_bigargs_kernel(ClsCountsArgs a) {
  const int lane = threadIdx.x & 63;
  const int64_t row = static_cast<int64_t>(blockIdx.x) * 4 + (threadIdx.x >> 6);
  if (row >= a.n) return;
  const float* rp = static_cast<const float*>(a.input) + row * a.row_stride;
  float m = -__builtin_huge_valf();
#pragma unroll
  for (int u = 0; u < 4; ++u) {
    const int col = u * FSTEP + lane * 4;
    const float4 q = *reinterpret_cast<const float4*>(rp + (col < C ? col : 0));
    m = fmaxf(m, fmaxf(fmaxf(q.x, q.y), fmaxf(q.z, q.w)));
  }
  const int64_t t = static_cast<const int64_t*>(a.target)[row];
  if (m == 12345.678f && t == 7) a.micro_total[row] = m;
}

// floor + block 0's one no-return atomic (prod's micro_total update): is the end-of-kernel
// release of a dirty L2 line part of the gap?
__global__ __launch_bounds__(256) void read_atomic_kernel(const float* __restrict__ x, const int64_t* __restrict__ y,
                                                          float* __restrict__ sink) {
  const int lane = threadIdx.x & 63;
  const int64_t row = static_cast<int64_t>(blockIdx.x) * 4 + (threadIdx.x >> 6);
  const float* rp = x + row * C;
  float m = -__builtin_huge_valf();
#pragma unroll
  for (int u = 0; u < 4; ++u) {
    const int col = u * FSTEP + lane * 4;
    const float4 q = *reinterpret_cast<const float4*>(rp + (col < C ? col : 0));
    m = fmaxf(m, fmaxf(fmaxf(q.x, q.y), fmaxf(q.z, q.w)));
  }
  const int64_t t = y[row];
  if (m == 12345.678f && t == 7) sink[row] = m;
  if (blockIdx.x == 0 && threadIdx.x == 0) atomicAdd(sink + N, 1.f);
}

// floor + the wave-max DPP reduction and the target's readlane compare (prod's row work, no
// ballots, no atomics)
__global__ __launch_bounds__(256) void read_reduce_kernel(const float* __restrict__ x, const int64_t* __restrict__ y,
                                                          float* __restrict__ sink) {
  const int lane = threadIdx.x & 63;
  const int64_t row = static_cast<int64_t>(blockIdx.x) * 4 + (threadIdx.x >> 6);
  const float* rp = x + row * C;
  float v[16];
#pragma unroll
  for (int u = 0; u < 4; ++u) {
    const int col = u * FSTEP + lane * 4;
    const float4 q = *reinterpret_cast<const float4*>(rp + (col < C ? col : 0));
    v[4 * u] = q.x;
    v[4 * u + 1] = q.y;
    v[4 * u + 2] = q.z;
    v[4 * u + 3] = q.w;
  }
  const int64_t t = y[row];
  float m = v[0];
#pragma unroll
  for (int e = 1; e < 16; ++e) m = fmaxf(m, v[e]);
  const float wm = wave_max_dpp(m);
  const int tu = static_cast<int>(t);
  const float sel = v[(tu / FSTEP) * 4 + (tu % 4)];
  const float xt = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(sel), (tu % FSTEP) / 4));
  if (xt == wm && lane == 0) sink[row & 1023] = wm;
}

// floor with non-temporal (streaming) 16-B loads: read-once data without L2 allocation
__global__ __launch_bounds__(256) void read_nt_kernel(const float* __restrict__ x, const int64_t* __restrict__ y,
                                                      float* __restrict__ sink) {
  const int lane = threadIdx.x & 63;
  const int64_t row = static_cast<int64_t>(blockIdx.x) * 4 + (threadIdx.x >> 6);
  const float* rp = x + row * C;
  float m = -__builtin_huge_valf();
#pragma unroll
  for (int u = 0; u < 4; ++u) {
    const int col = u * FSTEP + lane * 4;
    typedef float f4 __attribute__((ext_vector_type(4)));
    const f4 q = __builtin_nontemporal_load(reinterpret_cast<const f4*>(rp + (col < C ? col : 0)));
    m = fmaxf(m, fmaxf(fmaxf(q.x, q.y), fmaxf(q.z, q.w)));
  }
  const int64_t t = y[row];
  if (m == 12345.678f && t == 7) sink[row] = m;
}

__global__ void empty_kernel() {}

// the read floor with TPB-thread workgroups (TPB / 64 rows each): same 8192 waves, fewer and
// larger workgroups - is workgroup dispatch part of the per-launch cost?
template <int TPB>
__global__ __launch_bounds__(TPB) void read_floor_wg_kernel(const float* __restrict__ x, const int64_t* __restrict__ y,
                                                            float* __restrict__ sink) {
  const int lane = threadIdx.x & 63;
  const int64_t row = static_cast<int64_t>(blockIdx.x) * (TPB / 64) + (threadIdx.x >> 6);
  const float* rp = x + row * C;
  float m = -__builtin_huge_valf();
#pragma unroll
  for (int u = 0; u < 4; ++u) {
    const int col = u * FSTEP + lane * 4;
    const float4 q = *reinterpret_cast<const float4*>(rp + (col < C ? col : 0));
    m = fmaxf(m, fmaxf(fmaxf(q.x, q.y), fmaxf(q.z, q.w)));
  }
  const int64_t t = y[row];
  if (m == 12345.678f && t == 7) sink[row] = m;
}

template <typename F>
float time_it(F launch, int iters, hipEvent_t e0, hipEvent_t e1) {
  for (int i = 0; i < 20; ++i) launch(i);
  CK(hipDeviceSynchronize());
  CK(hipEventRecord(e0, 0));
  for (int i = 0; i < iters; ++i) launch(i);
  CK(hipEventRecord(e1, 0));
  CK(hipEventSynchronize(e1));
  float ms = 0.f;
  CK(hipEventElapsedTime(&ms, e0, e1));
  return ms * 1000.f / iters;
}

}  // namespace

int main(int argc, char** argv) {
  const int POOL = argc > 1 ? atoi(argv[1]) : 8;
  const int iters = argc > 2 ? atoi(argv[2]) : 400;
  std::vector<float> hx(static_cast<size_t>(N) * C);
  std::vector<int64_t> hy(N);
  srand(1);
  for (auto& v : hx) v = (rand() / static_cast<float>(RAND_MAX)) * 2.f - 1.f;
  for (int i = 0; i < N; ++i) hy[i] = rand() % C;
  std::vector<float*> xs(POOL);
  std::vector<int64_t*> ys(POOL);
  for (int p = 0; p < POOL; ++p) {
    CK(hipMalloc(&xs[p], hx.size() * 4));
    CK(hipMalloc(&ys[p], N * 8));
    CK(hipMemcpy(xs[p], hx.data(), hx.size() * 4, hipMemcpyHostToDevice));
    CK(hipMemcpy(ys[p], hy.data(), N * 8, hipMemcpyHostToDevice));
  }
  float *correct, *total, *sink;
  unsigned long long* pend;
  CK(hipMalloc(&correct, 4));
  CK(hipMalloc(&total, 4));
  CK(hipMalloc(&sink, (N + 64) * 4));
  CK(hipMalloc(&pend, kPendCells * kPendStride * 8));
  CK(hipMemset(correct, 0, 4));
  CK(hipMemset(total, 0, 4));
  CK(hipMemset(pend, 0, kPendCells * kPendStride * 8));
  hipEvent_t e0, e1;
  CK(hipEventCreate(&e0));
  CK(hipEventCreate(&e1));

  auto prod_args = [&](int i) {
    ClsCountsArgs a;
    a.input = xs[i % POOL];
    a.in_dt = DType::f32;
    a.n = N;
    a.c = C;
    a.row_stride = C;
    a.target = ys[i % POOL];
    a.tg_dt = DType::i64;
    a.k = 1;
    a.num_classes = C;
    a.micro_correct = correct;
    a.micro_total = total;
    a.pend = pend;
    return a;
  };
  auto prod = [&](int i) { launch_cls_counts(prod_args(i), 0); };
  auto prodpl = [&](int i) { k1_floor_prod_preload(prod_args(i), 0); };
  auto readpl = [&](int i) { k1_floor_read_preload(xs[i % POOL], ys[i % POOL], sink, 0); };
  auto read = [&](int i) {
    hipLaunchKernelGGL(read_floor_kernel, dim3(N / 4), dim3(256), 0, 0, xs[i % POOL], ys[i % POOL], sink);
  };
  auto empty = [&](int) { hipLaunchKernelGGL(empty_kernel, dim3(N / 4), dim3(256), 0, 0); };
  auto readatomic = [&](int i) {
    hipLaunchKernelGGL(read_atomic_kernel, dim3(N / 4), dim3(256), 0, 0, xs[i % POOL], ys[i % POOL], sink);
  };
  auto readreduce = [&](int i) {
    hipLaunchKernelGGL(read_reduce_kernel, dim3(N / 4), dim3(256), 0, 0, xs[i % POOL], ys[i % POOL], sink);
  };
  auto readnt = [&](int i) {
    hipLaunchKernelGGL(read_nt_kernel, dim3(N / 4), dim3(256), 0, 0, xs[i % POOL], ys[i % POOL], sink);
  };
  auto readbig = [&](int i) {
    ClsCountsArgs a;
    a.input = xs[i % POOL];
    a.n = N;
    a.c = C;
    a.row_stride = C;
    a.target = ys[i % POOL];
    a.micro_total = sink;
    hipLaunchKernelGGL(read_floor_bigargs_kernel, dim3(N / 4), dim3(256), 0, 0, a);
  };

  auto read512 = [&](int i) {
    hipLaunchKernelGGL(read_floor_wg_kernel<512>, dim3(N / 8), dim3(512), 0, 0, xs[i % POOL], ys[i % POOL], sink);
  };
  auto read1024 = [&](int i) {
    hipLaunchKernelGGL(read_floor_wg_kernel<1024>, dim3(N / 16), dim3(1024), 0, 0, xs[i % POOL], ys[i % POOL], sink);
  };
  auto empty1024 = [&](int) { hipLaunchKernelGGL(empty_kernel, dim3(N / 16), dim3(1024), 0, 0); };
  auto empty1 = [&](int) { hipLaunchKernelGGL(empty_kernel, dim3(1), dim3(64), 0, 0); };

  // interleave the variants over 3 rounds and keep each one's best median-of-round
  constexpr int NV = 13;
  float best[NV];
  for (float& b : best) b = 1e9f;
  for (int r = 0; r < 3; ++r) {
    best[0] = std::min(best[0], time_it(prod, iters, e0, e1));
    best[1] = std::min(best[1], time_it(read, iters, e0, e1));
    best[2] = std::min(best[2], time_it(empty, iters, e0, e1));
    best[3] = std::min(best[3], time_it(readbig, iters, e0, e1));
    best[4] = std::min(best[4], time_it(readatomic, iters, e0, e1));
    best[5] = std::min(best[5], time_it(readreduce, iters, e0, e1));
    best[6] = std::min(best[6], time_it(readnt, iters, e0, e1));
    best[7] = std::min(best[7], time_it(read512, iters, e0, e1));
    best[8] = std::min(best[8], time_it(read1024, iters, e0, e1));
    best[9] = std::min(best[9], time_it(empty1024, iters, e0, e1));
    best[10] = std::min(best[10], time_it(empty1, iters, e0, e1));
    best[11] = std::min(best[11], time_it(readpl, iters, e0, e1));
    best[12] = std::min(best[12], time_it(prodpl, iters, e0, e1));
  }
  // the head-attribution variants: interleaved over 5 rounds, every round kept
  constexpr int HR = 5;
  const int nh = k1_floor_head_variants();
  std::vector<std::vector<float>> head(nh);
  for (int r = 0; r < HR; ++r)
    for (int v = 0; v < nh; ++v)
      head[v].push_back(time_it(
          [&](int i) { k1_floor_head_launch(v, xs[i % POOL], ys[i % POOL], sink, pend, total, 0); }, iters, e0, e1));
  const double bytes = static_cast<double>(N) * C * 4 + N * 8;
  const char* names[NV] = {"prod (launch_cls_counts micro)", "read floor (same geometry)", "empty (2048 x 256)",
                           "read floor behind ClsCountsArgs", "read floor + one atomic", "read floor + DPP max + target compare",
                           "read floor, non-temporal loads", "read floor, 512-thread workgroups",
                           "read floor, 1024-thread workgroups", "empty (512 x 1024)", "empty (1 x 64)",
                           "read floor, preloaded arguments", "prod, preloaded arguments"};
  for (int v = 0; v < NV; ++v)
    printf("{\"variant\": \"%s\", \"pool\": %d, \"us_per_launch\": %.3f, \"TBps\": %.2f}\n", names[v], POOL, best[v],
           (v != 2 && (v < 9 || v > 10)) ? bytes / (best[v] * 1e-6) / 1e12 : 0.0);
  for (int v = 0; v < nh; ++v) {
    std::sort(head[v].begin(), head[v].end());
    printf("{\"head_variant\": \"%s\", \"pool\": %d, \"us_min\": %.3f, \"us_median\": %.3f, \"us_max\": %.3f}\n",
           k1_floor_head_name(v), POOL, head[v].front(), head[v][HR / 2], head[v].back());
  }
  printf("{\"prod_over_floor\": %.4f}\n", best[0] / best[1]);
  printf("{\"prod_preloaded_over_prod\": %.4f, \"read_preloaded_over_read\": %.4f}\n", best[12] / best[0],
         best[11] / best[1]);

  // Host side: the host cost of one production launch with no Python in
  // front of it, and bench.py's timed region (synchronize, t0, 20 updates, the micro_finish
  // fold, synchronize, t1) driven from C++: what the region costs with a zero-overhead caller.
  float* acc_out;
  CK(hipMalloc(&acc_out, 4));
  std::vector<double> enq, region1, region20, region1pl, region20pl;
  for (int rep = 0; rep < 41; ++rep) {
    CK(hipDeviceSynchronize());
    auto t0 = std::chrono::steady_clock::now();
    for (int i = 0; i < 20; ++i) prod(i);
    auto t1 = std::chrono::steady_clock::now();
    enq.push_back(std::chrono::duration<double, std::micro>(t1 - t0).count() / 20);
    CK(hipDeviceSynchronize());
    for (int n : {1, 20}) {
      for (int i = 0; i < 5; ++i) prod(i);  // bench.py's warmup right before the region
      CK(hipDeviceSynchronize());
      auto r0 = std::chrono::steady_clock::now();
      for (int i = 0; i < n; ++i) prod(i);
      launch_micro_finish(pend, correct, total, acc_out, 0);
      CK(hipDeviceSynchronize());
      auto r1 = std::chrono::steady_clock::now();
      (n == 1 ? region1 : region20).push_back(std::chrono::duration<double, std::micro>(r1 - r0).count());
      // the same region with preloaded arguments in both kernels
      for (int i = 0; i < 5; ++i) prodpl(i);
      CK(hipDeviceSynchronize());
      r0 = std::chrono::steady_clock::now();
      for (int i = 0; i < n; ++i) prodpl(i);
      k1_floor_finish_preload(pend, correct, total, acc_out, 0);
      CK(hipDeviceSynchronize());
      r1 = std::chrono::steady_clock::now();
      (n == 1 ? region1pl : region20pl).push_back(std::chrono::duration<double, std::micro>(r1 - r0).count());
    }
  }
  auto med = [](std::vector<double> v) {
    std::sort(v.begin(), v.end());
    return v[v.size() / 2];
  };
  printf("{\"host_us_per_launch\": %.3f, \"region_1_us\": %.2f, \"region_20_us\": %.2f, "
         "\"updates_per_s_at_20\": %.0f}\n",
         med(enq), med(region1), med(region20), 20.0 / med(region20) * 1e6);
  printf("{\"preloaded\": true, \"region_1_us\": %.2f, \"region_20_us\": %.2f, \"updates_per_s_at_20\": %.0f}\n",
         med(region1pl), med(region20pl), 20.0 / med(region20pl) * 1e6);
  return 0;
}

#endif  // K1_FLOOR_PRELOAD_UNIT
