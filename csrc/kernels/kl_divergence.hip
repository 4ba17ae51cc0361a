// K18: KL divergence of logit or probability rows, docs/parity.md "Not in the reference".
//
// Replaces the ATen form (functional/regression/kl_divergence.py): log_softmax twice, exp, sub, mul,
// a masked where and a sum, about eight [N, C]-sized passes and four [N, C] temporaries.  Here one
// wave streams row r of `target` (P) and of `input` (Q) together, once, in K7's walk: a scalar head
// up to the next 16-B boundary (one value per lane), a 16-B-load body of 16 values per lane and
// step, and a scalar tail.  Both rows sit at one offset from a 16-B boundary (checked on the host),
// so one split serves both.  All loads of a step, of both operands, are issued before the first
// value is used: 2 x 4 (f32) or 2 x 2 (16-bit) 16-B loads per lane; 16-bit rows run an unrolled
// body of two steps, eight loads, where they are long enough.
//
// Logits: with d_j = t_j - x_j (0 where t_j = -inf) and the row maxima m_t, m_x,
//   KL = (sum e^{t_j - m_t} d_j) / (sum e^{t_j - m_t}) + (m_x - m_t) + log(sum e^{x_j - m_x} / sum e^{t_j - m_t}),
// which never subtracts two log-sum-exps of the size of the logits.  A lane keeps the three sums
// against its running maxima and rescales them once per step (K7's absorb); the wave combines the
// lanes' sums in FP64 and lane 0 forms the value in FP64.  -inf is a masked entry: t_j = -inf adds
// nothing whatever x_j is, x_j = -inf opposite a finite t_j makes the row +inf (kept as a flag, so
// that no inf is ever rescaled), a NaN or +inf anywhere makes the sums and the row NaN, and a row
// that is all -inf in either operand is NaN.
//
// Probabilities: the sums of t, x and t (log t - log x), no maximum.  t_j = 0 adds nothing, x_j = 0
// opposite t_j > 0 makes the row +inf, and a negative, NaN or +inf entry or a zero sum makes it NaN;
//   KL = (sum t_j (log t_j - log x_j)) / sum t + log(sum x / sum t).
//
// Lane 0 of a wave adds its rows in FP64; a block stores one (sum, count) partial, and the finish
// launch adds the partials in block order into the class states or into the scalar result: two
// launches, no atomic, no host synchronisation, bit-identical between runs.
#include "tea_common.h"
#include "tea_kernels.h"
#include "tea_partials.h"
#include "tea_rowload.h"

namespace tea {

namespace {

constexpr int kB = 256;
constexpr int kWpb = kB / kWave;
constexpr int kFinishThreads = 128;           // 64 runs of consecutive blocks for each of the two values
constexpr int kFinishRuns = kFinishThreads / 2;
constexpr float kInf = __builtin_huge_valf();

// What a lane knows of the columns it has seen.  Logits: the running maxima mt, mx and the sums
// st = sum e^{t - mt}, at = sum e^{t - mt} d, sx = sum e^{x - mx} (each against finite_or_zero of
// its maximum).  Probabilities: st = sum t, sx = sum x, at = sum t (log t - log x); mt, mx unused.
struct Lane {
  float mt = -kInf, mx = -kInf;
  float st = 0.f, at = 0.f, sx = 0.f;
  bool hit = false;  // a column with q = 0 under p > 0: the row is +inf unless it is NaN
  bool bad = false;  // probabilities: a negative, NaN or +inf entry
};

// Fold H pairs (t[h], x[h]) into the lane.  Logits: the new maxima first, then every exponent
// against them, so that one call costs one rescale per sum.
template <bool LOGITS, int H>
__device__ __forceinline__ void absorb(const float* t, const float* x, Lane& s) {
  if constexpr (LOGITS) {
    float ct = t[0], cx = x[0];
#pragma unroll
    for (int e = 1; e < H; ++e) {
      ct = fmaxf(ct, t[e]);
      cx = fmaxf(cx, x[e]);
    }
    const float nt = fmaxf(s.mt, ct), nx = fmaxf(s.mx, cx);
    const float ft = finite_or_zero(nt), fx = finite_or_zero(nx);
    float cs = 0.f, ca = 0.f, cq = 0.f;
#pragma unroll
    for (int e = 0; e < H; ++e) {
      const bool off = t[e] == -kInf;          // p_j = 0: the term is 0 whatever x_j is
      const bool zero = x[e] == -kInf && !off;  // q_j = 0 under p_j > 0
      s.hit |= zero;
      const float d = (off || zero) ? 0.f : t[e] - x[e];
      const float w = exp_neg(t[e] - ft);
      cs += w;
      ca = __builtin_fmaf(w, d, ca);
      cq += exp_neg(x[e] - fx);
    }
    const float rt = exp_neg(s.mt - ft);
    s.st = __builtin_fmaf(s.st, rt, cs);
    s.at = __builtin_fmaf(s.at, rt, ca);
    s.sx = __builtin_fmaf(s.sx, exp_neg(s.mx - fx), cq);
    s.mt = nt;
    s.mx = nx;
  } else {
    float lo = fminimum(t[0], x[0]), hi = fmaximum(t[0], x[0]);
#pragma unroll
    for (int e = 1; e < H; ++e) {
      lo = fminimum(lo, fminimum(t[e], x[e]));
      hi = fmaximum(hi, fmaximum(t[e], x[e]));
    }
    s.bad |= !(lo >= 0.f && hi < kInf);  // a NaN fails both
#pragma unroll
    for (int e = 0; e < H; ++e) {
      const bool on = t[e] > 0.f;
      const bool zero = on && x[e] == 0.f;
      s.hit |= zero;
      s.st += t[e];
      s.sx += x[e];
      const float term = t[e] * (logf(t[e]) - logf(x[e]));
      s.at += (on && !zero) ? term : 0.f;
    }
  }
}

// Stream n values (n % 16 == 0, both pointers 16-B aligned) as steps of 16 values per lane.  16-bit
// kinds load two steps a wave-stride apart before either is reduced where the row is long enough,
// eight 16-B loads in flight as in an f32 step.  The same unrolling for f32 (16 loads, 178 VGPRs
// against 84) measured no faster on wide rows and 2.1 x slower at 8192 x 1000
// (profiles/kl_divergence_r14.json, "f32_unrolled_body_experiment").
template <int KIND, bool LOGITS>
__device__ __forceinline__ void stream_rows(const void* tp, const void* xp, int64_t n, int lane, Lane& s) {
  constexpr int64_t step = kWave * 16;
  int64_t base = static_cast<int64_t>(lane) * 16;
  if constexpr (kind_bytes<KIND> == 2) {
    for (; base + step < n; base += 2 * step) {
      float t[2][16], x[2][16];
      load_vals<KIND>(tp, base, t[0]);
      load_vals<KIND>(xp, base, x[0]);
      load_vals<KIND>(tp, base + step, t[1]);
      load_vals<KIND>(xp, base + step, x[1]);
      absorb<LOGITS, 32>(&t[0][0], &x[0][0], s);
    }
  }
  for (; base < n; base += step) {
    float t[16], x[16];
    load_vals<KIND>(tp, base, t);
    load_vals<KIND>(xp, base, x);
    absorb<LOGITS, 16>(t, x, s);
  }
}

// The row value from the wave's sums, FP64.  All lanes call it; lane 0 uses it.
template <bool LOGITS>
__device__ __forceinline__ double row_value(const Lane& s) {
  const double nan = __builtin_nan("");
  double st, at, sx, v;
  bool dead;
  if constexpr (LOGITS) {
    // the row maxima first (a lane's maximum is never NaN), one rescale per lane, then plain sums:
    // an empty lane adds 0 and a NaN in any lane's sum reaches the row's
    const float wt = wave_max(s.mt), wx = wave_max(s.mx);
    const double rt = static_cast<double>(exp_neg(s.mt - finite_or_zero(wt)));
    st = wave_sum(static_cast<double>(s.st) * rt);
    at = wave_sum(static_cast<double>(s.at) * rt);
    sx = wave_sum(static_cast<double>(s.sx) * static_cast<double>(exp_neg(s.mx - finite_or_zero(wx))));
    dead = wt == -kInf || wx == -kInf;  // all of one operand masked
    // (m_x - m_t) on its own: added to the logarithm's argument it would lose the logarithm
    v = at / st + (static_cast<double>(wx) - static_cast<double>(wt)) + log(sx / st);
  } else {
    st = wave_sum(static_cast<double>(s.st));
    at = wave_sum(static_cast<double>(s.at));
    sx = wave_sum(static_cast<double>(s.sx));
    dead = __ballot(s.bad) != 0 || !(st > 0.0) || !(sx > 0.0);  // a NaN sum fails the comparison
    v = at / st + log(sx / st);
  }
  const bool hit = __ballot(s.hit) != 0;
  if (dead) return nan;
  return (hit && v == v) ? static_cast<double>(kInf) : v;
}

template <int KIND, bool LOGITS>
__global__ __launch_bounds__(kB) void kl_divergence_kernel(KlDivArgs a) {
  const int lane = lane_id();
  const int64_t nw = static_cast<int64_t>(gridDim.x) * kWpb;
  double acc = 0.0, cnt = 0.0;
  for (int64_t row = static_cast<int64_t>(blockIdx.x) * kWpb + wave_id(); row < a.n; row += nw) {
    if (a.mask && a.mask[row] == 0) {  // never read
      if (a.rows_out && lane == 0) a.rows_out[row] = 0.f;
      continue;
    }
    const char* tp = static_cast<const char*>(a.target) + row * a.tg_row_stride * kind_bytes<KIND>;
    const char* xp = static_cast<const char*>(a.input) + row * a.in_row_stride * kind_bytes<KIND>;
    Lane s;
    int64_t head = head_elems<KIND>(tp);  // = head_elems(xp): one phase for both (host check)
    if (head > a.c) head = a.c;
    const int64_t body = ((a.c - head) / 16) * 16;
    if (lane < head) {
      const float t[1] = {load1<KIND>(tp, lane)}, x[1] = {load1<KIND>(xp, lane)};
      absorb<LOGITS, 1>(t, x, s);
    }
    stream_rows<KIND, LOGITS>(tp + head * kind_bytes<KIND>, xp + head * kind_bytes<KIND>, body, lane, s);
    const int64_t tc = head + body + lane;
    if (tc < a.c) {
      const float t[1] = {load1<KIND>(tp, tc)}, x[1] = {load1<KIND>(xp, tc)};
      absorb<LOGITS, 1>(t, x, s);
    }
    const double v = row_value<LOGITS>(s);
    if (lane == 0) {
      if (a.rows_out) a.rows_out[row] = static_cast<float>(v);
      acc += v;
      cnt += 1.0;
    }
  }
  if (a.partial == nullptr) return;
  __shared__ double lds[2][kWpb];
  if (lane == 0) {
    lds[0][threadIdx.x >> 6] = acc;
    lds[1][threadIdx.x >> 6] = cnt;
  }
  __syncthreads();
  if (threadIdx.x < 2) {
    double tot = 0.0;
#pragma unroll
    for (int w = 0; w < kWpb; ++w) tot += lds[threadIdx.x][w];
    a.partial[static_cast<int64_t>(threadIdx.x) * gridDim.x + blockIdx.x] = tot;
  }
}

// One block.  Thread (v, q) adds value v (0 sum, 1 count) over the q-th run of consecutive blocks,
// in block order, 16 loads in flight; thread v then adds the runs in run order.
__global__ __launch_bounds__(kFinishThreads) void kl_divergence_finish_kernel(KlDivArgs a, int blocks) {
  __shared__ double run[2][kFinishRuns];
  __shared__ double tot[2];
  const int v = threadIdx.x / kFinishRuns, q = threadIdx.x % kFinishRuns;
  const int per = (blocks + kFinishRuns - 1) / kFinishRuns;
  run[v][q] = run_fold<double>(a.partial + static_cast<int64_t>(v) * blocks, 1, q * per, min(blocks, (q + 1) * per));
  __syncthreads();
  if (threadIdx.x < 2) {
    double s = 0.0;
    for (int r = 0; r < kFinishRuns; ++r) s += run[threadIdx.x][r];
    tot[threadIdx.x] = s;
    double* dst = threadIdx.x == 0 ? a.dst_sum : a.dst_count;
    if (dst) *dst += s;
  }
  __syncthreads();
  if (threadIdx.x == 0 && a.out) *a.out = static_cast<float>(a.mean ? tot[0] / tot[1] : tot[0]);
}

template <int KIND>
void launch_rows(const KlDivArgs& a, int blocks, hipStream_t s) {
  if (a.from_logits) hipLaunchKernelGGL((kl_divergence_kernel<KIND, true>), dim3(blocks), dim3(kB), 0, s, a);
  else hipLaunchKernelGGL((kl_divergence_kernel<KIND, false>), dim3(blocks), dim3(kB), 0, s, a);
}

}  // namespace

int kl_divergence_blocks(int64_t n) { return stream_grid(n, kWpb, kKlMaxBlocks); }

int launch_kl_divergence(const KlDivArgs& a, hipStream_t stream) {
  if (a.n <= 0) return 0;
  if (a.c < 1 || a.c > 2147483647LL || a.input == nullptr || a.target == nullptr) return -1;
  if (a.rows_out == nullptr && a.partial == nullptr) return -1;
  if (a.partial != nullptr && a.out == nullptr && (a.dst_sum == nullptr || a.dst_count == nullptr)) return -1;
  // element-aligned rows, and row r of both operands at one offset from a 16-B boundary
  const int els = dtype_bytes(a.dt);
  const uintptr_t xi = reinterpret_cast<uintptr_t>(a.input), ti = reinterpret_cast<uintptr_t>(a.target);
  if (xi % els != 0 || ti % els != 0 || (xi - ti) % 16 != 0) return -2;
  if (a.n > 1 && ((a.in_row_stride - a.tg_row_stride) * els) % 16 != 0) return -2;
  const int blocks = kl_divergence_blocks(a.n);
  if (with_kind(a.dt, [&](auto kind) { return launch_rows<kind()>(a, blocks, stream), 0; }) != 0) return -1;
  if (a.partial != nullptr)
    hipLaunchKernelGGL(kl_divergence_finish_kernel, dim3(1), dim3(kFinishThreads), 0, stream, a, blocks);
  return static_cast<int>(hipGetLastError());
}

}  // namespace tea
