// K15: multiclass calibration error (ECE / MCE / RMS form), docs/parity.md "Not in the reference".
//
// Replaces the ATen form (functional/classification/calibration_error.py): softmax, max, bucketize,
// eq and three scatter_adds, about ten launches and at least three [N, C]-sized passes.  Here one
// pass over the scores does K1's argmax and K7's online sum of exponentials together:
//  * C > 32: a wave per row.  Rows that do not start 16-B aligned stream a scalar head (one value
//    per lane), a 16-B-load body of 16 values per lane and step, and a scalar tail, as K7 does.
//    Each lane keeps its running maximum (NaN-propagating), the first column holding it and, for
//    logits, the sum of exp(x - max) rescaled once per 16 values; lanes combine by the maximum, the
//    lowest column among its holders (torch.argmax's rule) and one rescale per lane.
//  * C <= 32: a thread per row, two passes over the row for logits.
// One lane per row forms the float32 confidence (the maximum, or 1 / sum), finds its bin in the
// float32 edge table e[b] = float32(b / n_bins) held in LDS (a multiply-and-ceil guess corrected
// against the table, which is the definition) and compares the prediction with the target.
// Sums are deterministic and free of float atomics: every wave adds its rows in its own fixed
// order into wave-private LDS bins (u32 count, u32 correct, f64 confidence), the block adds its
// waves in wave order into one partial triple per bin, and the finish launch adds the partials in
// block order into the class states, or into a scratch triple from which the same launch
// evaluates the value.  A target outside [0, C) or a confidence outside [0, 1] (a NaN in the row,
// a +inf logit, an all -inf row, a "probability" above 1) adds NaN to the confidence sum of bin 0,
// is counted nowhere else and sets a bit of ``err``, the only atomic.
#include "tea_common.h"
#include "tea_kernels.h"
#include "tea_partials.h"
#include "tea_rowload.h"

namespace tea {

namespace {

constexpr int kB = 256;
constexpr int kWpb = kB / kWave;
constexpr int kFinishThreads = 1024;
constexpr int kNoIndex = 0x7fffffff;

// exp_neg (tea_rowload.h): e^x to about an ulp for x <= 0.  The plain fast form loses
// |x| * 2^-24 relative to it, which shows in the confidence at the tolerance the tests hold.

// What a lane (or the thread that owns a row) knows of the columns it has seen, which it meets in
// ascending order: their maximum (NaN once it met one), the first column holding it, and for
// logits the sum of exp(x - finite_or_zero(m)).
struct RowState {
  float m = -__builtin_huge_valf();
  int idx = kNoIndex;
  float s = 0.f;
};

template <bool LOGITS>
__device__ __forceinline__ void absorb1(float v, int col, RowState& st) {
  if (v > st.m) st.idx = col;
  const float mn = fmaximum(st.m, v);
  if constexpr (LOGITS) {
    const float ms = finite_or_zero(mn);
    st.s = st.s * exp_neg(st.m - ms) + exp_neg(v - ms);
  }
  st.m = mn;
}

template <bool LOGITS>
__device__ __forceinline__ void absorb16(const float (&v)[16], int col0, RowState& st) {
  float cm = v[0];
#pragma unroll
  for (int e = 1; e < 16; ++e) cm = fmaximum(cm, v[e]);
  int ci = col0 + 15;
#pragma unroll
  for (int e = 14; e >= 0; --e) ci = v[e] == cm ? col0 + e : ci;
  if (cm > st.m) st.idx = ci;
  const float mn = fmaximum(st.m, cm);
  if constexpr (LOGITS) {
    const float ms = finite_or_zero(mn);
    float cs = 0.f;
#pragma unroll
    for (int e = 0; e < 16; ++e) cs += exp_neg(v[e] - ms);
    st.s = st.s * exp_neg(st.m - ms) + cs;
  }
  st.m = mn;
}

// ---------------------------------------------------------------- bins in LDS
struct Bins {
  float edge[kCalibMaxBins + 1];
  uint32_t count[kWpb][kCalibMaxBins];
  uint32_t correct[kWpb][kCalibMaxBins];
  double conf[kWpb][kCalibMaxBins];
};

__device__ __forceinline__ void bins_init(Bins& s, int nb) {
  for (int b = threadIdx.x; b <= nb; b += kB)
    s.edge[b] = static_cast<float>(static_cast<double>(b) / static_cast<double>(nb));
  for (int i = threadIdx.x; i < kWpb * nb; i += kB) {
    const int w = i / nb, b = i % nb;
    s.count[w][b] = 0u;
    s.correct[w][b] = 0u;
    s.conf[w][b] = 0.0;
  }
  __syncthreads();
}

// the bin b with edge[b] < conf <= edge[b + 1] (0 for conf == 0), for 0 <= conf <= 1.  The guess is
// within one bin of it; the table decides.
__device__ __forceinline__ int find_bin(const float* edge, int nb, float conf) {
  int b = static_cast<int>(ceilf(conf * static_cast<float>(nb))) - 1;
  b = b < 0 ? 0 : (b > nb - 1 ? nb - 1 : b);
  while (b > 0 && conf <= edge[b]) --b;
  while (b < nb - 1 && conf > edge[b + 1]) ++b;
  return b;
}

// bit 0: target outside [0, c); bit 1: confidence outside [0, 1] (or NaN)
__device__ __forceinline__ int row_flags(float conf, int64_t t, int64_t c) {
  return ((t >= 0 && t < c) ? 0 : 1) | ((conf >= 0.f && conf <= 1.f) ? 0 : 2);
}

// waves in wave order -> this block's partial triple per bin
__device__ __forceinline__ void bins_store(const Bins& s, int nb, double* partial) {
  __syncthreads();
  double* p = partial + static_cast<int64_t>(blockIdx.x) * 3 * nb;
  for (int b = threadIdx.x; b < nb; b += kB) {
    double n = 0.0, k = 0.0, f = 0.0;
#pragma unroll
    for (int w = 0; w < kWpb; ++w) {
      n += static_cast<double>(s.count[w][b]);
      k += static_cast<double>(s.correct[w][b]);
      f += s.conf[w][b];
    }
    p[b] = n;
    p[nb + b] = k;
    p[2 * nb + b] = f;
  }
}

// ---------------------------------------------------------------- C > 32: a wave per row
template <int KIND, bool LOGITS>
__global__ __launch_bounds__(kB) void calibration_wave_kernel(CalibrationArgs a) {
  __shared__ Bins s;
  constexpr int64_t kStep = kWave * 16;
  const int nb = a.n_bins;
  bins_init(s, nb);
  const int lane = lane_id(), w = wave_id();
  const int C = static_cast<int>(a.c);
  const int64_t nw = static_cast<int64_t>(gridDim.x) * kWpb;
  for (int64_t row = static_cast<int64_t>(blockIdx.x) * kWpb + w; row < a.n; row += nw) {
    const char* rp = static_cast<const char*>(a.input) + row * a.row_stride * kind_bytes<KIND>;
    const int64_t t = load_as_i64(a.target, a.tg_dt, row);
    RowState st;
    int head = static_cast<int>(head_elems<KIND>(rp));
    if (head > C) head = C;
    const int64_t body = ((C - head) / 16) * 16;
    if (lane < head) absorb1<LOGITS>(load1<KIND>(rp, lane), lane, st);
    const char* bp = rp + head * kind_bytes<KIND>;  // 16-B aligned
    int64_t base = static_cast<int64_t>(lane) * 16;
    // two steps loaded before either is reduced: rows too long for the batch to fill the CUs
    for (; base + kStep < body; base += 2 * kStep) {
      float v0[16], v1[16];
      load_vals<KIND>(bp, base, v0);
      load_vals<KIND>(bp, base + kStep, v1);
      absorb16<LOGITS>(v0, head + static_cast<int>(base), st);
      absorb16<LOGITS>(v1, head + static_cast<int>(base + kStep), st);
    }
    for (; base < body; base += kStep) {
      float v0[16];
      load_vals<KIND>(bp, base, v0);
      absorb16<LOGITS>(v0, head + static_cast<int>(base), st);
    }
    const int64_t tc = head + body + lane;
    if (tc < C) absorb1<LOGITS>(load1<KIND>(rp, tc), static_cast<int>(tc), st);

    float wm = st.m;
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) wm = fmaximum(wm, __shfl_xor(wm, o, kWave));
    int pred = st.m == wm ? st.idx : kNoIndex;
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) pred = min(pred, __shfl_xor(pred, o, kWave));
    float conf = wm;
    if constexpr (LOGITS) conf = 1.f / wave_sum(st.s * exp_neg(st.m - finite_or_zero(wm)));
    if (lane == 0) {
      const int flags = row_flags(conf, t, a.c);
      if (flags != 0) {
        s.conf[w][0] += __builtin_nan("");
        if (a.err) atomicOr(a.err, flags);
      } else {
        const int b = find_bin(s.edge, nb, conf);
        s.count[w][b] += 1u;
        s.correct[w][b] += pred == t ? 1u : 0u;
        s.conf[w][b] += static_cast<double>(conf);
      }
    }
  }
  bins_store(s, nb, a.partial);
}

// ---------------------------------------------------------------- C <= 32: a thread per row
template <int KIND, bool LOGITS>
__global__ __launch_bounds__(kB) void calibration_thread_kernel(CalibrationArgs a) {
  __shared__ Bins s;
  const int nb = a.n_bins;
  bins_init(s, nb);
  const int lane = lane_id(), w = wave_id();
  const int C = static_cast<int>(a.c);
  const int64_t stride = static_cast<int64_t>(gridDim.x) * kB;
  // block-uniform trip count: every lane takes part in the wave's fold below
  for (int64_t r0 = static_cast<int64_t>(blockIdx.x) * kB; r0 < a.n; r0 += stride) {
    const int64_t row = r0 + threadIdx.x;
    const bool live = row < a.n;
    float conf = 0.f;
    int bin = -1, flags = 0;
    bool correct = false;
    if (live) {
      const char* rp = static_cast<const char*>(a.input) + row * a.row_stride * kind_bytes<KIND>;
      const int64_t t = load_as_i64(a.target, a.tg_dt, row);
      RowState st;
      for (int c = 0; c < C; ++c) absorb1<false>(load1<KIND>(rp, c), c, st);
      conf = st.m;
      if constexpr (LOGITS) {  // the second pass reads what the first left in the cache
        const float ms = finite_or_zero(st.m);
        float sum = 0.f;
        for (int c = 0; c < C; ++c) sum += exp_neg(load1<KIND>(rp, c) - ms);
        conf = 1.f / sum;
      }
      flags = row_flags(conf, t, a.c);
      if (flags == 0) {
        bin = find_bin(s.edge, nb, conf);
        correct = st.idx == t;
      }
    }
    // the wave's rows into its bins, one distinct bin per round in the order of the first lane
    // that holds it; a bin's confidences are added by the fixed butterfly of wave_sum
    uint64_t todo = __ballot(bin >= 0);
    while (todo != 0) {
      const int b = __shfl(bin, __ffsll(static_cast<unsigned long long>(todo)) - 1, kWave);
      const bool mine = bin == b;
      const uint64_t members = __ballot(mine);
      const uint64_t hits = __ballot(mine && correct);
      const double cs = wave_sum(mine ? static_cast<double>(conf) : 0.0);
      if (lane == 0) {
        s.count[w][b] += static_cast<uint32_t>(__popcll(members));
        s.correct[w][b] += static_cast<uint32_t>(__popcll(hits));
        s.conf[w][b] += cs;
      }
      todo &= ~members;
    }
    const uint64_t bad = __ballot(flags != 0);
    if (bad != 0) {
      if (lane == 0) s.conf[w][0] += __builtin_nan("");
      if (flags != 0 && a.err) atomicOr(a.err, flags);
    }
  }
  bins_store(s, nb, a.partial);
}

// ---------------------------------------------------------------- value and finish
// FP64 over bins in ascending order, empty bins skipped; NaN without rows or with a bad row
__device__ float calibration_value(const double* count, const double* correct, const double* conf, int nb, int norm) {
  double total = 0.0;
  for (int b = 0; b < nb; ++b) total += count[b];
  if (!(total > 0.0) || conf[0] != conf[0]) return __builtin_nanf("");
  double acc = 0.0;
  for (int b = 0; b < nb; ++b) {
    if (count[b] == 0.0) continue;
    const double d = fabs(correct[b] - conf[b]);
    if (norm == 0) {
      acc += d;
    } else if (norm == 1) {
      const double g = d / count[b];
      acc = (g > acc || g != g) ? g : acc;
    } else {
      acc += d * d / (count[b] * total);
    }
  }
  return static_cast<float>(norm == 0 ? acc / total : norm == 1 ? acc : sqrt(acc));
}

// One block.  Thread (q, p) adds pair p = (state, bin) over the q-th run of consecutive blocks, in
// block order; the runs are then added in run order.  A wave reads consecutive pairs of one block.
__global__ __launch_bounds__(kFinishThreads) void calibration_finish_kernel(CalibrationArgs a, int blocks) {
  __shared__ double run[kFinishThreads];
  __shared__ double sum[3 * kCalibMaxBins];
  const int nb = a.n_bins, pairs = 3 * nb;
  const int runs = kFinishThreads / pairs;  // >= 1: pairs <= 3 * kCalibMaxBins < kFinishThreads
  const int per = (blocks + runs - 1) / runs;
  const int q = threadIdx.x / pairs, p = threadIdx.x % pairs;
  if (q < runs) run[q * pairs + p] = run_fold<double>(a.partial + p, pairs, q * per, min(blocks, (q + 1) * per));
  __syncthreads();
  if (threadIdx.x < pairs) {
    double acc = 0.0;
    for (int r = 0; r < runs; ++r) acc += run[r * pairs + p];
    double* dst = a.dst[p / nb] + p % nb;
    *dst = a.accumulate ? *dst + acc : acc;
    sum[p] = acc;
  }
  __syncthreads();
  if (threadIdx.x == 0 && a.out) *a.out = calibration_value(sum, sum + nb, sum + 2 * nb, nb, a.norm);
}

__global__ __launch_bounds__(kWave) void calibration_value_kernel(const double* count, const double* correct,
                                                                  const double* conf, int nb, int norm, float* out) {
  if (threadIdx.x == 0) *out = calibration_value(count, correct, conf, nb, norm);
}

template <int KIND>
void launch_rows(const CalibrationArgs& a, int blocks, hipStream_t s) {
  const bool wave = a.c > kCalibNarrowMaxC;
  if (wave && a.from_logits) hipLaunchKernelGGL((calibration_wave_kernel<KIND, true>), dim3(blocks), dim3(kB), 0, s, a);
  else if (wave) hipLaunchKernelGGL((calibration_wave_kernel<KIND, false>), dim3(blocks), dim3(kB), 0, s, a);
  else if (a.from_logits) hipLaunchKernelGGL((calibration_thread_kernel<KIND, true>), dim3(blocks), dim3(kB), 0, s, a);
  else hipLaunchKernelGGL((calibration_thread_kernel<KIND, false>), dim3(blocks), dim3(kB), 0, s, a);
}

}  // namespace

int calibration_blocks(int64_t n, int64_t c) {
  return stream_grid(n, c > kCalibNarrowMaxC ? kWpb : kB, kCalibMaxBlocks);
}

int launch_calibration(const CalibrationArgs& a, hipStream_t stream) {
  if (a.n <= 0) return 0;
  if (a.c < 1 || a.c > 2147483647LL || a.n_bins < 1 || a.n_bins > kCalibMaxBins || a.norm < 0 || a.norm > 2) return -1;
  if (a.partial == nullptr || a.dst[0] == nullptr || a.dst[1] == nullptr || a.dst[2] == nullptr) return -1;
  if (a.tg_dt != DType::i64 && a.tg_dt != DType::i32) return -1;
  if (reinterpret_cast<uintptr_t>(a.input) % dtype_bytes(a.in_dt) != 0) return -2;  // rows must be element-aligned
  const int blocks = calibration_blocks(a.n, a.c);
  if (with_kind(a.in_dt, [&](auto kind) { return launch_rows<kind()>(a, blocks, stream), 0; }) != 0) return -1;
  hipLaunchKernelGGL(calibration_finish_kernel, dim3(1), dim3(kFinishThreads), 0, stream, a, blocks);
  return static_cast<int>(hipGetLastError());
}

int launch_calibration_value(const double* bin_count, const double* correct_sum, const double* conf_sum, int n_bins,
                             int norm, float* out, hipStream_t stream) {
  if (n_bins < 1 || norm < 0 || norm > 2) return -1;
  hipLaunchKernelGGL(calibration_value_kernel, dim3(1), dim3(kWave), 0, stream, bin_count, correct_sum, conf_sum,
                     n_bins, norm, out);
  return static_cast<int>(hipGetLastError());
}

}  // namespace tea
