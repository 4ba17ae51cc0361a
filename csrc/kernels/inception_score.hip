// K21: Inception Score, docs/parity.md "Not in the reference".
//
// Replaces the ATen form (functional/image/inception_score.py): softmax, log_softmax, two widenings,
// a product, a masked where, a row sum and three index_adds, about eight [N, C]-sized passes.  Here
// the logits are read once.  Row i belongs to split (first + i) mod S.  The grid is S x B blocks of
// four waves; block (s, b) walks the rows of split s, i = i0(s) + S k, with k strided over the 4 B
// waves of the split.  One wave handles one row and holds it in registers, VPL values per lane
// (VPL = 4 / 16 / 32 for C <= 256 / 1024 / 2048, columns past C hold -inf):
//
//   m = max x (NaN-propagating), e_j = exp_neg(x_j - finite_or_zero(m)), per-lane float32 sums of e
//   and of e (x - m) (x - m taken as 0 where e = 0, so 0 * -inf is never formed), both added over
//   the lanes in FP64: Z and A.  The row's negative entropy is h = A / Z - log Z in FP64 (K18's
//   form: no two log-sum-exps of the size of the logits are subtracted), and p_j = double(e_j) *
//   (1 / Z) with one FP64 division per row, added into VPL FP64 accumulators per lane that live
//   across the wave's rows.  For rows of 0 / -inf with a power-of-two number of zeros every p is
//   exact.  A NaN or +inf logit or an all -inf row makes Z, h and every p of the row NaN.
//
// A lane owns the same columns in every row of a launch: value v of lane l is column
// ((v / G) * 64 + l) * G + v % G, G the values of one load.  Where the launch's rows are 16-byte
// aligned (base aligned, row stride times element size a multiple of 16) a group is one 16-byte
// load (8 bytes for 16-bit rows of C <= 256, whose lanes own four values); the one group of a row
// that straddles C, and every group of a launch that is not aligned, is read by guarded element
// loads in the same column mapping (correct, not tuned: no A/B against a shifted vector walk was
// run).  No load touches a byte outside a row's C elements.  All loads of a row are issued into raw
// registers before the first value is converted.
//
// At the end the four waves fold their accumulators through LDS in wave order, ((w0 + w1) + w2) +
// w3, and the block stores one FP64 partial [C + 2] (columns, sum of h, row count) with plain
// stores.  inception_finish_kernel adds the B partials of every (s, j) in block order into the three
// states (+=).  inception_value_kernel takes a wave per split, 64-strided columns added in a fixed
// order, writes split_log[s] and then, from one wave, the mean and population standard deviation
// of exp(split_log) over the splits with rows.  No atomic, no host synchronisation, no waiting
// between workgroups: results are bit-identical from run to run.
//
// Registers (hipcc --save-temps, gfx950; .vgpr_count of the 16-byte arm / the element arm, the same
// within one register for f32, bf16 and f16; no AGPRs, no scratch, no spills), the allocation in
// granules of 8 and the waves per SIMD it allows (512 / allocation, at most 8):
//   VPL  4:  55-56 /  55-56  ->  56  -> 8 waves per SIMD, 2112 B of LDS per block
//   VPL 16:  90-91 /  93     ->  96  -> 5 waves per SIMD, 8256 B
//   VPL 32: 161-162 / 141    -> 168 / 144 -> 3 waves per SIMD, 16448 B
// The accumulators are 2 VPL of these (8, 32, 64 VGPRs); a block is one wave per SIMD.
#include "tea_common.h"
#include "tea_kernels.h"
#include "tea_partials.h"
#include "tea_rowload.h"

namespace tea {

namespace {

constexpr int kB = kInceptionWavesPerBlock * kWave;
constexpr int kWpb = kInceptionWavesPerBlock;
constexpr int kFinishThreads = 256;
constexpr int kValueThreads = 1024;
constexpr int kValueWaves = kValueThreads / kWave;

// values of one load of a lane that owns VPL values
template <int KIND, int VPL>
constexpr int group_of = (16 / kind_bytes<KIND>) < VPL ? (16 / kind_bytes<KIND>) : VPL;

// the bits of -inf in KIND
template <int KIND>
constexpr uint32_t ninf_bits = KIND == 0 ? 0xff800000u : KIND == 1 ? 0xff80u : 0xfc00u;

// Row `row` (c columns) into x, the lane's VPL values.  Phase one issues every load into raw
// words, phase two converts.
template <int KIND, int VPL, bool VEC>
__device__ __forceinline__ void load_row(const char* row, int c, int lane, float (&x)[VPL]) {
  constexpr int G = group_of<KIND, VPL>;
  constexpr int U = VPL / G;
  constexpr int WG = G * kind_bytes<KIND> / 4;  // 32-bit words of one group: 4, or 2 (16-bit, G = 4)
  static_assert(WG == 4 || WG == 2, "a group is a 16-byte or an 8-byte load");
  uint32_t raw[U][WG];
#pragma unroll
  for (int u = 0; u < U; ++u) {
    const int col0 = (u * kWave + lane) * G;
    if (VEC && col0 + G <= c) {
      const char* p = row + static_cast<int64_t>(col0) * kind_bytes<KIND>;
      if constexpr (WG == 4) {
        const uint4 q = *reinterpret_cast<const uint4*>(p);
        raw[u][0] = q.x;
        raw[u][1] = q.y;
        raw[u][2] = q.z;
        raw[u][3] = q.w;
      } else {
        const uint2 q = *reinterpret_cast<const uint2*>(p);
        raw[u][0] = q.x;
        raw[u][1] = q.y;
      }
    } else if constexpr (KIND == 0) {
#pragma unroll
      for (int e = 0; e < G; ++e)
        raw[u][e] = col0 + e < c ? reinterpret_cast<const uint32_t*>(row)[col0 + e] : ninf_bits<0>;
    } else {
#pragma unroll
      for (int e = 0; e < G; e += 2) {
        const uint32_t lo = col0 + e < c ? reinterpret_cast<const uint16_t*>(row)[col0 + e] : ninf_bits<KIND>;
        const uint32_t hi = col0 + e + 1 < c ? reinterpret_cast<const uint16_t*>(row)[col0 + e + 1] : ninf_bits<KIND>;
        raw[u][e / 2] = lo | (hi << 16);
      }
    }
  }
#pragma unroll
  for (int u = 0; u < U; ++u) {
    if constexpr (KIND == 0) {
#pragma unroll
      for (int e = 0; e < G; ++e) x[u * G + e] = __uint_as_float(raw[u][e]);
    } else {
#pragma unroll
      for (int e = 0; e < G; e += 2) unpack2<KIND>(raw[u][e / 2], x[u * G + e], x[u * G + e + 1]);
    }
  }
}

// column of value v of lane `lane`
template <int G>
__device__ __forceinline__ int column_of(int v, int lane) {
  return ((v / G) * kWave + lane) * G + v % G;
}

template <int KIND, int VPL, bool VEC>
__global__ __launch_bounds__(kB) void inception_rows_kernel(InceptionArgs a, int bps) {
  constexpr int G = group_of<KIND, VPL>;
  const int lane = lane_id(), w = wave_id();
  const int s = blockIdx.y, b = blockIdx.x;
  const int64_t i0 = (s - a.first + a.splits) % a.splits;  // the first row of split s
  const int64_t step = static_cast<int64_t>(a.splits) * kWpb * bps;
  double acc[VPL];
#pragma unroll
  for (int v = 0; v < VPL; ++v) acc[v] = 0.0;
  double hs = 0.0, cnt = 0.0;
  for (int64_t i = i0 + static_cast<int64_t>(a.splits) * (b * kWpb + w); i < a.n; i += step) {
    const char* row = static_cast<const char*>(a.logits) + i * a.row_stride * kind_bytes<KIND>;
    float x[VPL];
    load_row<KIND, VPL, VEC>(row, a.c, lane, x);
    float m = x[0];
#pragma unroll
    for (int v = 1; v < VPL; ++v) m = fmaximum(m, x[v]);
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) m = fmaximum(m, __shfl_xor(m, o, kWave));
    const float fm = finite_or_zero(m);
    float se = 0.f, sa = 0.f;
#pragma unroll
    for (int v = 0; v < VPL; ++v) {
      const float d = x[v] - fm;
      const float e = exp_neg(d);
      se += e;
      sa = __builtin_fmaf(e, e == 0.f ? 0.f : d, sa);
      x[v] = e;
    }
    const double z = wave_sum(static_cast<double>(se));
    const double t = wave_sum(static_cast<double>(sa));
    const double rz = 1.0 / z;
#pragma unroll
    for (int v = 0; v < VPL; ++v) acc[v] += static_cast<double>(x[v]) * rz;
    hs += t / z - log(z);
    cnt += 1.0;
  }
  __shared__ double fold[VPL * kWave];
  __shared__ double wave_h[kWpb], wave_n[kWpb];
  if (lane == 0) {
    wave_h[w] = hs;
    wave_n[w] = cnt;
  }
  for (int k = 1; k < kWpb; ++k) {
    if (w == k) {
#pragma unroll
      for (int v = 0; v < VPL; ++v) fold[v * kWave + lane] = acc[v];
    }
    __syncthreads();
    if (w == 0) {
#pragma unroll
      for (int v = 0; v < VPL; ++v) acc[v] += fold[v * kWave + lane];
    }
    __syncthreads();
  }
  if (w != 0) return;
  double* p = a.partial + (static_cast<int64_t>(s) * bps + b) * (a.c + 2);
#pragma unroll
  for (int v = 0; v < VPL; ++v) {
    const int col = column_of<G>(v, lane);
    if (col < a.c) p[col] = acc[v];
  }
  if (lane < 2) {
    const double* src = lane == 0 ? wave_h : wave_n;
    double tot = src[0];
#pragma unroll
    for (int k = 1; k < kWpb; ++k) tot += src[k];
    p[a.c + lane] = tot;
  }
}

// Thread (s, j), j in [0, c + 2): the bps partials of value j of split s, in block order, += into
// its state element.
__global__ __launch_bounds__(kFinishThreads) void inception_finish_kernel(InceptionArgs a, int bps) {
  const int64_t width = a.c + 2;
  const int64_t t = static_cast<int64_t>(blockIdx.x) * kFinishThreads + threadIdx.x;
  if (t >= a.splits * width) return;
  const int64_t s = t / width, j = t % width;
  const double v = run_fold<double>(a.partial + s * bps * width + j, width, 0, bps);
  double* dst = j < a.c ? a.prob_sum + s * a.c + j : (j == a.c ? a.neg_entropy_sum + s : a.num_rows + s);
  *dst += v;
}

// One block of 16 waves.  Wave w forms split_log of the splits w, w + 16, ...: lane l adds the
// terms of columns l, l + 64, ... in that order, then the butterfly.  Wave 0, a lane per split,
// then forms the mean and the population standard deviation of exp(split_log).
__global__ __launch_bounds__(kValueThreads) void inception_value_kernel(const double* prob_sum, const double* neg_entropy_sum,
                                                                        const double* num_rows, int splits, int64_t c,
                                                                        double* split_log, float* out) {
  __shared__ double logs[kInceptionMaxSplits];
  const int lane = lane_id(), w = wave_id();
  const double nan = __builtin_nan("");
  for (int s = w; s < splits; s += kValueWaves) {
    const double n = num_rows[s];
    // The launch is bound by the FP64 division and logarithm of its one block's waves on one CU:
    // 14.7 us at 10 x 1000 against 4.4 us at 10 x 10, and four independent columns per step
    // measured the same 14.7 us (profiles/inception_score_r17.json), so the plain loop stays.
    double t = 0.0;
    for (int64_t j = lane; j < c; j += kWave) {
      const double q = prob_sum[s * c + j] / n;
      t += q == 0.0 ? 0.0 : q * log(q);
    }
    t = wave_sum(t);
    const double l = n > 0.0 ? neg_entropy_sum[s] / n - t : nan;
    if (lane == 0) {
      logs[s] = l;
      split_log[s] = l;
    }
  }
  __syncthreads();
  if (w != 0) return;
  const bool have = lane < splits && num_rows[lane < splits ? lane : 0] > 0.0;
  const double v = have ? exp(logs[lane]) : 0.0;
  const double count = wave_sum(have ? 1.0 : 0.0);
  const double mean = wave_sum(v) / count;  // no split with rows: 0 / 0
  const double dev = have ? v - mean : 0.0;
  const double var = wave_sum(dev * dev) / count;
  if (lane == 0) {
    out[0] = static_cast<float>(mean);
    out[1] = static_cast<float>(sqrt(var));
  }
}

template <int KIND, int VPL>
void launch_rows(const InceptionArgs& a, int bps, bool vec, hipStream_t s) {
  const dim3 grid(bps, a.splits);
  if (vec) hipLaunchKernelGGL((inception_rows_kernel<KIND, VPL, true>), grid, dim3(kB), 0, s, a, bps);
  else hipLaunchKernelGGL((inception_rows_kernel<KIND, VPL, false>), grid, dim3(kB), 0, s, a, bps);
}

template <int KIND>
void launch_rows(const InceptionArgs& a, int bps, bool vec, hipStream_t s) {
  if (a.c <= 4 * kWave) launch_rows<KIND, 4>(a, bps, vec, s);
  else if (a.c <= 16 * kWave) launch_rows<KIND, 16>(a, bps, vec, s);
  else launch_rows<KIND, 32>(a, bps, vec, s);
}

}  // namespace

static_assert(kInceptionNarrowColumns == 4 * kWave && kInceptionMaxColumns == 32 * kWave, "the VPL arms");

int inception_blocks(int64_t n, int splits, int c) {
  const int64_t rows = (n + splits - 1) / splits;  // of the largest split
  const int per_wave = c <= kInceptionNarrowColumns ? kInceptionRowsPerWaveNarrow : kInceptionRowsPerWaveWide;
  return stream_grid(rows, kWpb * per_wave, kInceptionMaxBlocks / splits);
}

int launch_inception_update(const InceptionArgs& a, hipStream_t stream) {
  if (a.n <= 0) return 0;
  if (a.n >= (int64_t{1} << 31) || a.c < 1 || a.c > kInceptionMaxColumns) return -1;
  if (a.splits < 1 || a.splits > kInceptionMaxSplits || a.first < 0 || a.first >= a.splits) return -1;
  if (a.logits == nullptr || a.partial == nullptr || a.row_stride < 0) return -1;
  if (a.prob_sum == nullptr || a.neg_entropy_sum == nullptr || a.num_rows == nullptr) return -1;
  const int els = dtype_bytes(a.dt);
  const uintptr_t base = reinterpret_cast<uintptr_t>(a.logits);
  if (base % els != 0) return -2;
  // 16-byte loads where every row of the launch is 16-byte aligned
  const bool vec = base % 16 == 0 && (a.n == 1 || (a.row_stride * els) % 16 == 0);
  const int bps = inception_blocks(a.n, a.splits, a.c);
  if (with_kind(a.dt, [&](auto kind) { return launch_rows<kind()>(a, bps, vec, stream), 0; }) != 0) return -1;
  const int64_t cells = static_cast<int64_t>(a.splits) * (a.c + 2);
  hipLaunchKernelGGL(inception_finish_kernel, dim3(static_cast<unsigned>((cells + kFinishThreads - 1) / kFinishThreads)),
                     dim3(kFinishThreads), 0, stream, a, bps);
  return static_cast<int>(hipGetLastError());
}

int launch_inception_value(const double* prob_sum, const double* neg_entropy_sum, const double* num_rows,
                           int splits, int64_t c, double* split_log, float* out, hipStream_t stream) {
  if (splits < 1 || splits > kInceptionMaxSplits || c < 1) return -1;
  if (!prob_sum || !neg_entropy_sum || !num_rows || !split_log || !out) return -1;
  hipLaunchKernelGGL(inception_value_kernel, dim3(1), dim3(kValueThreads), 0, stream, prob_sum, neg_entropy_sum,
                     num_rows, splits, c, split_log, out);
  return static_cast<int>(hipGetLastError());
}

}  // namespace tea
