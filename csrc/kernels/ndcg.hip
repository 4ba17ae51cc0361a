// K13: normalized discounted cumulative gain, one value per row (docs/parity.md, "Not in the
// reference").
//
// Replaces the ATen form (functional/ranking/ndcg.py): two sorts of an [N, C] tensor, a gather,
// run boundaries from two cumulative scans and five elementwise passes, with ONE read of the
// scores and the relevance.
//
// The tie-averaged DCG needs, per item i, g_i = #{j : s_j > s_i} and e_i = #{j : s_j == s_i}:
//     DCG = sum_i gain_i * (D[min(g_i + e_i, K)] - D[min(g_i, K)]) / e_i
// with D the prefix table of the discounts (K + 1 doubles, built on the host).  IDCG is the same
// functional with the gain as the score.  Scores compare by order_key of tea_rowload.h
// (-0.0 == +0.0, every NaN one key above +inf); gains, terms and sums are FP64.
//
//  * C <= 64: one wave per row, one item per lane.  g and e come from a C-step loop that
//    broadcasts lane j's key and gain (v_readlane of a wave-uniform index); DCG and IDCG are wave
//    sums (a fixed butterfly).  Rows are grid-strided, 4 waves per 256-thread block as in K10.
//  * 64 < C <= kNdcgMaxColumns: one 256-thread workgroup per row.  (key << 32 | column) as u64
//    in LDS, padded to a power of two with 0 (below every real key), bitonic-sorted descending;
//    each sorted position finds its run [start, end) by two binary searches and adds
//    gain[column] * (D[min(end, K)] - D[min(start, K)]) / (end - start).  Then the gains' bit
//    patterns (non-negative doubles order like their bits) are sorted in the second LDS array
//    and IDCG = sum_{p < K} gain[p] * (D[p + 1] - D[p]).  2 * P * 8 bytes of LDS: 64 KiB at the
//    cap, two workgroups per CU.
//
// A row holding a relevance with !(t >= 0) scores NaN and sets bit 0 of ``err`` (the only
// atomic).  With class states, every block writes one FP64 partial (the sum of its unrounded row
// values, in row order) and ``ndcg_finish`` adds the partials in a fixed order into ``ndcg_sum``
// and n into ``num_rows``: no atomics on the value path, no host synchronisation, deterministic.
#include "tea_common.h"
#include "tea_kernels.h"
#include "tea_rowload.h"

namespace tea {

namespace {

constexpr int kBlock = 256;
constexpr int kWavesPerBlock = kBlock / kWave;
constexpr int kMaxGrid = 2048;

template <int KIND>
__device__ __forceinline__ const void* score_row(const NdcgArgs& a, int64_t row) {
  return static_cast<const char*>(a.x) + row * a.x_stride * kind_bytes<KIND>;
}

// gain of a relevance: t or 2^t - 1 (an integer t takes the exact power of two); +0.0 for
// t == -0.0 and for the relevance of a bad row, so the bits of a gain order like its value
__device__ __forceinline__ double gain_of(double t, int exponential) {
  if (!(t >= 0.0)) return 0.0;
  double g = t;
  if (exponential) g = ((floor(t) == t && t < 1024.0) ? ldexp(1.0, static_cast<int>(t)) : exp2(t)) - 1.0;
  return g > 0.0 ? g : 0.0;
}

__device__ __forceinline__ double row_value(double dcg, double idcg, bool bad) {
  if (bad) return __builtin_nan("");
  return idcg == 0.0 ? 0.0 : dcg / idcg;
}

// ------------------------------------------------------------------ C <= 64: a wave per row
template <int KIND>
__global__ __launch_bounds__(kBlock) void ndcg_narrow_kernel(NdcgArgs a) {
  __shared__ double s_part[kWavesPerBlock];
  const int lane = lane_id();
  const int wave = wave_id();
  const int C = a.c, K = a.k;
  const int tsize = dtype_bytes(a.t_dt);
  const int64_t nwaves = static_cast<int64_t>(gridDim.x) * kWavesPerBlock;
  double acc = 0.0;  // this wave's rows, in row order (lane 0's copy is used)
  for (int64_t row = static_cast<int64_t>(blockIdx.x) * kWavesPerBlock + wave; row < a.n; row += nwaves) {
    const bool live = lane < C;
    uint32_t key = 0u;
    double t = 0.0;
    if (live) {
      key = order_key(load1<KIND>(score_row<KIND>(a, row), lane));
      t = load_as_f64(static_cast<const char*>(a.t) + row * a.t_stride * tsize, a.t_dt, lane);
    }
    const bool bad = __any(live && !(t >= 0.0));
    const double gain = gain_of(t, a.exponential);
    int gs = 0, es = 0, gr = 0, er = 0;
    for (int j = 0; j < C; ++j) {
      const uint32_t kj = static_cast<uint32_t>(__builtin_amdgcn_readlane(static_cast<int>(key), j));
      const double gj = readlane_f64(gain, j);
      gs += kj > key;
      es += kj == key;
      gr += gj > gain;
      er += gj == gain;
    }
    double dcg = 0.0, idcg = 0.0;
    if (live) {  // es, er >= 1: the item itself
      dcg = gain * (a.D[min(gs + es, K)] - a.D[min(gs, K)]) / static_cast<double>(es);
      idcg = gain * (a.D[min(gr + er, K)] - a.D[min(gr, K)]) / static_cast<double>(er);
    }
    dcg = wave_sum(dcg);
    idcg = wave_sum(idcg);
    const double v = row_value(dcg, idcg, bad);
    acc += v;
    if (lane == 0) {
      if (a.out) a.out[row] = static_cast<float>(v);
      if (bad && a.err) atomicOr(a.err, 1);
    }
  }
  if (a.partial) {
    if (lane == 0) s_part[wave] = acc;
    __syncthreads();
    if (threadIdx.x == 0) {
      double s = 0.0;
      for (int w = 0; w < kWavesPerBlock; ++w) s += s_part[w];
      a.partial[blockIdx.x] = s;
    }
  }
}

// ------------------------------------------------------------------ C > 64: a workgroup per row
// descending bitonic sort of s[0 .. P), P a power of two >= 128, by all kBlock threads
__device__ __forceinline__ void bitonic_desc(unsigned long long* s, int P) {
  for (int k = 2; k <= P; k <<= 1) {
    for (int j = k >> 1; j > 0; j >>= 1) {
      for (int i = threadIdx.x; i < (P >> 1); i += kBlock) {
        const int lo = ((i & ~(j - 1)) << 1) | (i & (j - 1));
        const int hi = lo + j;  // < P
        const unsigned long long x = s[lo], y = s[hi];
        const bool desc = (lo & k) == 0;
        if ((x < y) == desc && x != y) {
          s[lo] = y;
          s[hi] = x;
        }
      }
      __syncthreads();
    }
  }
}

template <int KIND>
__global__ __launch_bounds__(kBlock) void ndcg_wide_kernel(NdcgArgs a, int P) {
  extern __shared__ __attribute__((aligned(16))) unsigned long long s_dyn[];
  __shared__ double s_red[2 * kWavesPerBlock];
  unsigned long long* s_key = s_dyn;   // [P] (order key << 32) | column, sorted descending
  unsigned long long* s_gain = s_dyn + P;  // [P] gain bits: by column, then sorted descending
  const int C = a.c, K = a.k;
  const int tsize = dtype_bytes(a.t_dt);
  const int lane = lane_id();
  const int wave = wave_id();
  double acc = 0.0;  // thread 0: this block's rows, in row order
  for (int64_t row = blockIdx.x; row < a.n; row += gridDim.x) {
    const void* xr = score_row<KIND>(a, row);
    const void* tr = static_cast<const char*>(a.t) + row * a.t_stride * tsize;
    int bad = 0;
    for (int i = threadIdx.x; i < P; i += kBlock) {
      unsigned long long kc = 0ull, gb = 0ull;
      if (i < C) {
        const double t = load_as_f64(tr, a.t_dt, i);
        bad |= !(t >= 0.0);
        const double gain = gain_of(t, a.exponential);
        kc = (static_cast<unsigned long long>(order_key(load1<KIND>(xr, i))) << 32) | static_cast<unsigned>(i);
        gb = static_cast<unsigned long long>(__double_as_longlong(gain));
      }
      s_key[i] = kc;
      s_gain[i] = gb;
    }
    bad = __syncthreads_or(bad);
    bitonic_desc(s_key, P);
    double dcg = 0.0;
    for (int p = threadIdx.x; p < C; p += kBlock) {
      const unsigned long long kc = s_key[p];
      const unsigned long long top = kc | 0xffffffffull, bot = kc & ~0xffffffffull;
      // start: first position whose entry is <= top; end: first position whose entry is < bot
      int lo = 0, hi = p;
      while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        if (s_key[mid] <= top) hi = mid; else lo = mid + 1;
      }
      const int start = lo;
      if (start >= K) continue;  // the whole run lies beyond the cutoff
      lo = p + 1;
      hi = C;  // entries at and beyond C are pads (0 < bot)
      while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        if (s_key[mid] < bot) hi = mid; else lo = mid + 1;
      }
      const int end = lo;
      const double gain = __longlong_as_double(static_cast<long long>(s_gain[static_cast<unsigned>(kc)]));
      dcg += gain * (a.D[min(end, K)] - a.D[start]) / static_cast<double>(end - start);
    }
    __syncthreads();  // every read of the gains by column is done
    bitonic_desc(s_gain, P);
    double idcg = 0.0;
    for (int p = threadIdx.x; p < K; p += kBlock)  // K <= C <= P
      idcg += __longlong_as_double(static_cast<long long>(s_gain[p])) * (a.D[p + 1] - a.D[p]);
    dcg = wave_sum(dcg);
    idcg = wave_sum(idcg);
    if (lane == 0) {
      s_red[wave] = dcg;
      s_red[kWavesPerBlock + wave] = idcg;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
      double d = 0.0, id = 0.0;
      for (int w = 0; w < kWavesPerBlock; ++w) {
        d += s_red[w];
        id += s_red[kWavesPerBlock + w];
      }
      const double v = row_value(d, id, bad != 0);
      acc += v;
      if (a.out) a.out[row] = static_cast<float>(v);
      if (bad && a.err) atomicOr(a.err, 1);
    }
    __syncthreads();  // s_red and the LDS arrays are free for the next row
  }
  if (a.partial && threadIdx.x == 0) a.partial[blockIdx.x] = acc;
}

// partial[0 .. blocks) -> ndcg_sum += their sum (fixed order), num_rows += n
__global__ __launch_bounds__(kBlock) void ndcg_finish_kernel(const double* partial, int blocks, double n,
                                                             double* ndcg_sum, double* num_rows) {
  __shared__ double s_part[16];
  double v = 0.0;
  for (int i = threadIdx.x; i < blocks; i += kBlock) v += partial[i];
  v = block_sum(v, s_part);
  if (threadIdx.x == 0) {
    *ndcg_sum += v;
    *num_rows += n;
  }
}

template <int KIND>
int launch_kind(const NdcgArgs& a, int blocks, hipStream_t s) {
  if (a.c <= kWave) {
    hipLaunchKernelGGL((ndcg_narrow_kernel<KIND>), dim3(blocks), dim3(kBlock), 0, s, a);
  } else {
    int P = 128;
    while (P < a.c) P <<= 1;
    const int lds = 2 * P * 8;
    static const bool lds_ok =
        hipFuncSetAttribute(reinterpret_cast<const void*>(&ndcg_wide_kernel<KIND>),
                            hipFuncAttributeMaxDynamicSharedMemorySize, 2 * kNdcgMaxColumns * 8) == hipSuccess;
    if (!lds_ok) return -3;
    hipLaunchKernelGGL((ndcg_wide_kernel<KIND>), dim3(blocks), dim3(kBlock), lds, s, a, P);
  }
  return static_cast<int>(hipGetLastError());
}

}  // namespace

int ndcg_blocks(int64_t n, int64_t c) {
  const int64_t want = c <= kWave ? (n + kWavesPerBlock - 1) / kWavesPerBlock : n;
  return static_cast<int>(want < 1 ? 1 : (want > kMaxGrid ? kMaxGrid : want));
}

int launch_ndcg(const NdcgArgs& a, hipStream_t stream) {
  if (a.n <= 0) return 0;
  if (a.c < 1 || a.c > kNdcgMaxColumns || a.k < 1 || a.k > a.c || a.D == nullptr) return -1;
  if ((a.ndcg_sum != nullptr) != (a.partial != nullptr) || (a.ndcg_sum != nullptr) != (a.num_rows != nullptr))
    return -1;
  if (a.out == nullptr && a.partial == nullptr) return -1;
  switch (a.t_dt) {
    case DType::f32: case DType::f16: case DType::bf16: case DType::i64: case DType::i32:
    case DType::i16: case DType::i8: case DType::u8: break;
    default: return -1;
  }
  const int blocks = ndcg_blocks(a.n, a.c);
  const int rc = with_kind(a.x_dt, [&](auto kind) { return launch_kind<kind()>(a, blocks, stream); });
  if (rc || a.partial == nullptr) return rc;
  hipLaunchKernelGGL(ndcg_finish_kernel, dim3(1), dim3(kBlock), 0, stream, a.partial, blocks,
                     static_cast<double>(a.n), a.ndcg_sum, a.num_rows);
  return static_cast<int>(hipGetLastError());
}

}  // namespace tea
