// K16: Pearson and Lin's concordance correlation per task, docs/parity.md "Not in the reference".
//
// Replaces the ATen form (functional/regression/pearson.py): two widening copies, two subtracts, five
// products and five row sums, about twenty launches and a dozen [tasks, n]-sized FP64 passes.  Here
// one pass reads both operands once.  Every sample is widened to FP64 (exact for f32 / f16 / bf16)
// and taken against the pivot, the task's first sample of this call, which every block of the task
// reads again (two L2-served loads); a thread keeps the five FP64 sums S_x, S_y, S_xx, S_yy, S_xy of
// those differences.
//  * Row arm: unit stride along the samples, any task stride.  A block owns kCorrRowSpan samples of
//    one task as groups of 8: a thread has at most two groups, all of whose loads are issued before
//    the first convert.  f32 groups are two 16-B loads at any 4-B alignment (load_f4u); 16-bit
//    groups are one 16-B load behind a scalar head that reaches the 16-B boundary, and a scalar tail
//    (K7's shape).  Two 16-bit operands whose heads differ cannot share one: the second operand
//    then takes element loads.
//  * Column arm: unit stride along the tasks (the transposed view of a row-major [n, tasks]
//    tensor).  A lane owns a task column, a block 64 columns and kCorrColSpan samples, its four
//    waves every fourth sample; loads are coalesced along the tasks, eight samples of both operands
//    in flight; the waves fold through LDS in wave order (K5's column layout).
// Both arms write one FP64 5-tuple per (task, block).  The finish launch, a wave per task, adds them
// in a fixed order (lane l the blocks l, l + 64, ..., then the wave butterfly), forms the batch's
// moments and merges them into the [6, tasks] state in place (class update) or writes the value
// (functional).  No atomics anywhere: results are bit-identical from run to run.  A NaN or inf makes
// its own task's m2 NaN through the arithmetic (inf - inf^2 / n) and touches no other task.
#include "tea_common.h"
#include "tea_kernels.h"
#include "tea_partials.h"
#include "tea_rowload.h"

namespace tea {

namespace {

constexpr int kB = 256;
constexpr int kWpb = kB / kWave;
constexpr int kColUnroll = 8;
// a row-arm block is one round of two groups of 8 samples per thread; longer spans (rounds in a
// loop) measured 0.6 - 2.1 us slower up to 100 x 10000 and 0.3 - 0.6 us faster, inside the spread,
// at 1000 x 8192 (profiles/pearson_r12.json)
static_assert(kCorrRowSpan == 8 * 2 * kB, "the row arm's span is two groups of 8 per thread");
static_assert(kCorrColSpan % (kWpb * kColUnroll) == 0, "a column-arm wave walks whole unrolled steps");

// eight consecutive samples as loaded, before any convert
template <int KIND>
struct Raw8 {
  uint4 w;
};
template <>
struct Raw8<0> {
  float4 lo, hi;
};

// `vec`: the address of sample i is 16-B aligned (16-bit kinds; f32 needs 4 B only)
template <int KIND>
__device__ __forceinline__ Raw8<KIND> load8(const void* base, int64_t i, bool vec) {
  Raw8<KIND> r;
  if constexpr (KIND == 0) {
    const float* p = static_cast<const float*>(base) + i;
    r.lo = load_f4u(p);
    r.hi = load_f4u(p + 4);
  } else {
    const uint16_t* p = static_cast<const uint16_t*>(base) + i;
    if (vec) {
      r.w = *reinterpret_cast<const uint4*>(p);
    } else {
      r.w.x = static_cast<uint32_t>(p[0]) | (static_cast<uint32_t>(p[1]) << 16);
      r.w.y = static_cast<uint32_t>(p[2]) | (static_cast<uint32_t>(p[3]) << 16);
      r.w.z = static_cast<uint32_t>(p[4]) | (static_cast<uint32_t>(p[5]) << 16);
      r.w.w = static_cast<uint32_t>(p[6]) | (static_cast<uint32_t>(p[7]) << 16);
    }
  }
  return r;
}

template <int KIND>
__device__ __forceinline__ void widen8(const Raw8<KIND>& r, double (&v)[8]) {
  if constexpr (KIND == 0) {
    const float f[8] = {r.lo.x, r.lo.y, r.lo.z, r.lo.w, r.hi.x, r.hi.y, r.hi.z, r.hi.w};
#pragma unroll
    for (int e = 0; e < 8; ++e) v[e] = static_cast<double>(f[e]);
  } else {
    unpack8<KIND>(r.w, v);
  }
}

// samples until the next 16-B boundary of a 16-bit operand; f32 has no head
template <int KIND>
__device__ __forceinline__ int head_of(const void* p) {
  if constexpr (KIND == 0) return 0;
  return static_cast<int>(head_elems<KIND>(p));
}

// the five sums of differences to the pivot
struct Sums {
  double v[5] = {0.0, 0.0, 0.0, 0.0, 0.0};
  __device__ __forceinline__ void add(double dx, double dy) {
    v[0] += dx;
    v[1] += dy;
    v[2] = __builtin_fma(dx, dx, v[2]);
    v[3] = __builtin_fma(dy, dy, v[3]);
    v[4] = __builtin_fma(dx, dy, v[4]);
  }
};

template <int KX, int KY>
__device__ __forceinline__ void add8(Sums& s, const Raw8<KX>& rx, const Raw8<KY>& ry, double px, double py) {
  double x[8], y[8];
  widen8<KX>(rx, x);
  widen8<KY>(ry, y);
#pragma unroll
  for (int e = 0; e < 8; ++e) s.add(x[e] - px, y[e] - py);
}

// ---------------------------------------------------------------- row arm
template <int KX, int KY>
__global__ __launch_bounds__(kB) void corr_row_kernel(CorrcoefArgs a, int bpt) {
  __shared__ double s_w[kWpb][5];
  const int64_t task = blockIdx.x / bpt;
  const int b = blockIdx.x % bpt;
  const char* xr = static_cast<const char*>(a.x) + task * a.x_task_stride * kind_bytes<KX>;
  const char* yr = static_cast<const char*>(a.y) + task * a.y_task_stride * kind_bytes<KY>;
  const double px = load1<KX>(xr, 0), py = load1<KY>(yr, 0);
  const int64_t s0 = static_cast<int64_t>(b) * kCorrRowSpan;
  const int64_t left = a.n - s0;
  const int len = static_cast<int>(left < kCorrRowSpan ? left : kCorrRowSpan);
  // one head for both operands: the first 16-bit operand's; a second 16-bit operand with another
  // head takes element loads
  const int hx = head_of<KX>(xr + s0 * kind_bytes<KX>), hy = head_of<KY>(yr + s0 * kind_bytes<KY>);
  int head = KX != 0 ? hx : hy;
  const bool yvec = KX == 0 || KY == 0 || hx == hy;
  head = head < len ? head : len;
  const int groups = (len - head) / 8;  // <= 2 kB
  const int tail0 = head + groups * 8;
  const int t = threadIdx.x;
  Sums s;
  const int64_t e0 = s0 + head;
  const int g1 = t + kB;
  if (g1 < groups) {
    const Raw8<KX> x0 = load8<KX>(xr, e0 + 8 * t, true), x1 = load8<KX>(xr, e0 + 8 * g1, true);
    const Raw8<KY> y0 = load8<KY>(yr, e0 + 8 * t, yvec), y1 = load8<KY>(yr, e0 + 8 * g1, yvec);
    add8<KX, KY>(s, x0, y0, px, py);
    add8<KX, KY>(s, x1, y1, px, py);
  } else if (t < groups) {
    const Raw8<KX> x0 = load8<KX>(xr, e0 + 8 * t, true);
    const Raw8<KY> y0 = load8<KY>(yr, e0 + 8 * t, yvec);
    add8<KX, KY>(s, x0, y0, px, py);
  }
  if (t < head) s.add(load1<KX>(xr, s0 + t) - px, load1<KY>(yr, s0 + t) - py);
  if (t < len - tail0) s.add(load1<KX>(xr, s0 + tail0 + t) - px, load1<KY>(yr, s0 + tail0 + t) - py);

  // this block's five sums; kept here: through a shared K-value block sum the kernel's instructions
  // move (profiles/partials_dedup_codegen.txt)
  const int lane = lane_id(), w = wave_id();
#pragma unroll
  for (int k = 0; k < 5; ++k) {
    const double ws = wave_sum(s.v[k]);
    if (lane == 0) s_w[w][k] = ws;
  }
  __syncthreads();
  if (t < 5) {
    double acc = 0.0;
#pragma unroll
    for (int q = 0; q < kWpb; ++q) acc += s_w[q][t];
    a.partial[static_cast<int64_t>(blockIdx.x) * 5 + t] = acc;
  }
}

// ---------------------------------------------------------------- column arm
template <int KX, int KY>
__global__ __launch_bounds__(kB) void corr_col_kernel(CorrcoefArgs a, int bpt) {
  __shared__ double s_f[kWpb][5][kCorrColTasks];
  const int64_t tile = blockIdx.x / bpt;
  const int b = blockIdx.x % bpt;
  const int lane = lane_id(), w = wave_id();
  const int64_t task = tile * kCorrColTasks + lane;
  const bool live = task < a.tasks;
  const int64_t tc = live ? task : a.tasks - 1;  // dead lanes read the last column and write nothing
  const double px = load1<KX>(a.x, tc), py = load1<KY>(a.y, tc);
  const int64_t s0 = static_cast<int64_t>(b) * kCorrColSpan;
  const int64_t end = a.n - s0 < kCorrColSpan ? a.n : s0 + kCorrColSpan;
  Sums s;
  for (int64_t r = s0 + w; r < end; r += kWpb * kColUnroll) {
    double x[kColUnroll], y[kColUnroll];
    // unconditional loads, clamped to the span's last sample; what lies past it is not added
#pragma unroll
    for (int u = 0; u < kColUnroll; ++u) {
      const int64_t q = r + kWpb * u < end ? r + kWpb * u : end - 1;
      x[u] = load1<KX>(a.x, q * a.x_sample_stride + tc);
      y[u] = load1<KY>(a.y, q * a.y_sample_stride + tc);
    }
#pragma unroll
    for (int u = 0; u < kColUnroll; ++u)
      if (r + kWpb * u < end) s.add(x[u] - px, y[u] - py);
  }
#pragma unroll
  for (int k = 0; k < 5; ++k) s_f[w][k][lane] = s.v[k];
  __syncthreads();
  if (w == 0 && live) {
    double* p = a.partial + (task * bpt + b) * 5;
#pragma unroll
    for (int k = 0; k < 5; ++k) {
      double acc = 0.0;
#pragma unroll
      for (int q = 0; q < kWpb; ++q) acc += s_f[q][k][lane];
      p[k] = acc;
    }
  }
}

// ---------------------------------------------------------------- moments
struct Moments {
  double n, mx, my, m2x, m2y, c;
};

__device__ __forceinline__ Moments moments_load(const double* m, int64_t tasks, int64_t task) {
  return {m[task], m[tasks + task], m[2 * tasks + task], m[3 * tasks + task], m[4 * tasks + task],
          m[5 * tasks + task]};
}

__device__ __forceinline__ void moments_store(double* m, int64_t tasks, int64_t task, const Moments& v) {
  m[task] = v.n;
  m[tasks + task] = v.mx;
  m[2 * tasks + task] = v.my;
  m[3 * tasks + task] = v.m2x;
  m[4 * tasks + task] = v.m2y;
  m[5 * tasks + task] = v.c;
}

// a negative rounding residue becomes 0; a NaN stays
__device__ __forceinline__ double not_below_zero(double v) { return v < 0.0 ? 0.0 : v; }

__device__ __forceinline__ Moments batch_moments(double n, double px, double py, const double (&s)[5]) {
  Moments m;
  m.n = n;
  m.mx = px + s[0] / n;
  m.my = py + s[1] / n;
  m.m2x = not_below_zero(s[2] - s[0] * s[0] / n);
  m.m2y = not_below_zero(s[3] - s[1] * s[1] / n);
  m.c = s[4] - s[0] * s[1] / n;
  return m;
}

// the pairwise update (Chan et al.); an empty side contributes nothing
__device__ __forceinline__ Moments moments_merge(const Moments& a, const Moments& b) {
  if (b.n == 0.0) return a;
  if (a.n == 0.0) return b;
  Moments m;
  m.n = a.n + b.n;
  const double dx = b.mx - a.mx, dy = b.my - a.my;
  const double wb = b.n / m.n, wab = a.n * b.n / m.n;
  m.mx = a.mx + dx * wb;
  m.my = a.my + dy * wb;
  m.m2x = a.m2x + b.m2x + dx * dx * wab;
  m.m2y = a.m2y + b.m2y + dy * dy * wab;
  m.c = a.c + b.c + dx * dy * wab;
  return m;
}

// NaN for n < 2 and for a zero (or NaN) denominator
__device__ __forceinline__ float moments_value(const Moments& m, int concordance) {
  double num, den;
  if (concordance) {
    const double d = m.mx - m.my;
    num = 2.0 * m.c;
    den = m.m2x + m.m2y + m.n * d * d;
  } else {
    num = m.c;
    den = sqrt(m.m2x * m.m2y);
  }
  if (!(m.n >= 2.0) || den == 0.0) return __builtin_nanf("");
  double r = num / den;
  if (!concordance) r = r > 1.0 ? 1.0 : (r < -1.0 ? -1.0 : r);
  return static_cast<float>(r);
}

__device__ __forceinline__ double pivot_of(const void* p, DType dt, int64_t i) {
  return static_cast<double>(load_as_f32(p, dt, i));
}

// a wave per task
__global__ __launch_bounds__(kB) void corr_finish_kernel(CorrcoefArgs a, int bpt) {
  const int64_t task = static_cast<int64_t>(blockIdx.x) * kWpb + wave_id();
  if (task >= a.tasks) return;
  const int lane = lane_id();
  double s[5];
  wave_strided_sum(a.partial + task * bpt * 5, bpt, 5, 1, s);
  if (lane != 0) return;
  const double px = pivot_of(a.x, a.x_dt, task * a.x_task_stride);
  const double py = pivot_of(a.y, a.y_dt, task * a.y_task_stride);
  const Moments m = batch_moments(static_cast<double>(a.n), px, py, s);
  if (a.moments) moments_store(a.moments, a.tasks, task, moments_merge(moments_load(a.moments, a.tasks, task), m));
  if (a.out) a.out[task] = moments_value(m, a.concordance);
}

__global__ __launch_bounds__(kB) void corr_merge_kernel(double* state, const double* other, int64_t tasks) {
  const int64_t task = static_cast<int64_t>(blockIdx.x) * kB + threadIdx.x;
  if (task >= tasks) return;
  moments_store(state, tasks, task, moments_merge(moments_load(state, tasks, task), moments_load(other, tasks, task)));
}

__global__ __launch_bounds__(kB) void corr_value_kernel(const double* state, int64_t tasks, int concordance,
                                                        float* out) {
  const int64_t task = static_cast<int64_t>(blockIdx.x) * kB + threadIdx.x;
  if (task >= tasks) return;
  out[task] = moments_value(moments_load(state, tasks, task), concordance);
}

template <int KX, int KY>
void launch_arm(const CorrcoefArgs& a, int64_t grid, int bpt, hipStream_t s) {
  if (a.column) hipLaunchKernelGGL((corr_col_kernel<KX, KY>), dim3(grid), dim3(kB), 0, s, a, bpt);
  else hipLaunchKernelGGL((corr_row_kernel<KX, KY>), dim3(grid), dim3(kB), 0, s, a, bpt);
}

}  // namespace

int corrcoef_blocks(int64_t n, int column) {
  const int64_t span = column ? kCorrColSpan : kCorrRowSpan;
  return static_cast<int>((n + span - 1) / span);
}

int launch_corrcoef(const CorrcoefArgs& a, hipStream_t stream) {
  if (a.tasks < 1 || a.n < 1 || a.n > 2147483647LL) return -1;
  if (a.x == nullptr || a.y == nullptr || a.partial == nullptr || (a.moments == nullptr && a.out == nullptr)) return -1;
  if (reinterpret_cast<uintptr_t>(a.x) % dtype_bytes(a.x_dt) != 0) return -2;
  if (reinterpret_cast<uintptr_t>(a.y) % dtype_bytes(a.y_dt) != 0) return -2;
  if (a.column ? (a.x_task_stride != 1 || a.y_task_stride != 1) : (a.x_sample_stride != 1 || a.y_sample_stride != 1))
    return -1;
  const int bpt = corrcoef_blocks(a.n, a.column);
  const int64_t tiles = a.column ? (a.tasks + kCorrColTasks - 1) / kCorrColTasks : a.tasks;
  const int64_t grid = tiles * bpt;
  const int64_t finish_grid = (a.tasks + kWpb - 1) / kWpb;
  if (grid > 2147483647LL || finish_grid > 2147483647LL) return -3;
  const int rc = with_kind(a.x_dt, [&](auto kx) {
    return with_kind(a.y_dt, [&](auto ky) { return launch_arm<decltype(kx)::value, ky()>(a, grid, bpt, stream), 0; });
  });
  if (rc != 0) return rc;
  hipLaunchKernelGGL(corr_finish_kernel, dim3(finish_grid), dim3(kB), 0, stream, a, bpt);
  return static_cast<int>(hipGetLastError());
}

int launch_corrcoef_merge(double* state, const double* other, int64_t tasks, hipStream_t stream) {
  if (tasks < 1 || state == nullptr || other == nullptr) return -1;
  const int64_t grid = (tasks + kB - 1) / kB;
  if (grid > 2147483647LL) return -3;
  hipLaunchKernelGGL(corr_merge_kernel, dim3(grid), dim3(kB), 0, stream, state, other, tasks);
  return static_cast<int>(hipGetLastError());
}

int launch_corrcoef_value(const double* state, int64_t tasks, int concordance, float* out, hipStream_t stream) {
  if (tasks < 1 || state == nullptr || out == nullptr) return -1;
  const int64_t grid = (tasks + kB - 1) / kB;
  if (grid > 2147483647LL) return -3;
  hipLaunchKernelGGL(corr_value_kernel, dim3(grid), dim3(kB), 0, stream, state, tasks, concordance, out);
  return static_cast<int>(hipGetLastError());
}

}  // namespace tea
