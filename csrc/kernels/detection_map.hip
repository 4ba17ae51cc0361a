// K24: COCO-style detection mean average precision (definition: docs/parity.md, "Not in the
// reference"; wrapper: torcheval_amd/ops/detection.py).
//
// map_match_kernel, one launch per update.  A workgroup of 256 threads owns an image at a time
// (the grid is persistent over the images):
//  1. it stages the image's detection and ground-truth boxes in LDS as float4 and builds one key per
//     box: detections  label << 42 | ~orderable(score) << 10 | index  (u64), ground truths
//     label << 10 | index  (u32; labels take 22 bits, 2^22 - 1 is "no class": a bad box);
//  2. both key lists are sorted ascending with K13's LDS bitonic sort, so a class is a run of
//     detections by score descending (equal scores in input order) and a run of ground truths in
//     input order; the boxes stay where they were staged and are reached through the index bits;
//  3. the waves share the class runs.  A wave walks the kept detections of its run in order, the
//     only sequential loop (at most max_detections long).  Lanes own the run's ground truths, 64 at
//     a time: each forms its IoU in FP64 (box_iou: one rounded operation per step, never an FMA),
//     and per threshold the wave takes the maximum over "unmatched and iou >= min(t, 1 - 1e-10)"
//     and, by a ballot, the highest lane that holds it: the later ground truth among equal IoUs.
//     The matched masks are a u16 per ground truth in LDS, a bit per threshold.
// It writes (score, label, hits) per detection at the image's offset in sorted order and adds the
// ground truths per class with one int64 atomic per (image, class): integer sums, so the result is
// bit-identical from run to run.  The only other global atomic is the flag.  A run of more than 64
// ground truths forms an IoU again per threshold (registers hold the first 64 only).
// LDS: 2 x 16 KB boxes, 8 KB + 4 KB keys, 2 KB masks, 2 KB run starts: 48 KB, three workgroups per CU.
//
// map_curve_kernel, in compute().  A workgroup owns one (class, threshold) and walks the class's
// hits (already in the global order) in chunks of 256 from the right: the chunk's hit count gives
// the count before it, an inclusive scan the cumulative hits tp_j, prec_j = tp / (fp + tp + 2^-52),
// and a suffix maximum joined with the carry from the right the envelope.  The position of the
// m-th hit serves U(m) - U(m - 1) of the 101 recall points, U(m) = #{q : R[q] <= m / n_gt} by a
// binary search of R in LDS and U(0) = 0, so AP = sum(count x envelope) / 101 in FP64 in a fixed
// order.  map_finish_kernel (one workgroup) takes the means; NaN entries are classes without
// ground truth and enter none.
#include "tea_common.h"
#include "tea_kernels.h"

namespace tea {

namespace {

constexpr int kWaves = kMapBlock / kWave;
constexpr unsigned kNoClass = 0x3fffffu;
constexpr unsigned kIndexMask = kMapMaxBoxes - 1;
static_assert(kMapMaxBoxes == 1024 && kMapMaxClasses == static_cast<int>(kNoClass), "key layout");
static_assert(kMapMaxThresholds <= 16, "the matched masks are u16");

// float -> u32 whose unsigned order is the float order, with -0.0 == +0.0 (NaN never gets here)
__device__ __forceinline__ unsigned orderable(float s) {
  unsigned b = __float_as_uint(s);
  if (s == 0.f) b = 0u;
  return (b & 0x80000000u) ? ~b : (b | 0x80000000u);
}

// The IoU of the definition: every coordinate widened exactly, then one rounded FP64 operation
// per step, so the CPU form, the oracle and this kernel decide every threshold compare alike.  The
// pragma alone does not hold under -ffp-contract=fast (the backend fused the inlined body), so
// ops/build.py builds this unit with -ffp-contract=off.
__device__ __forceinline__ double box_iou(const float4 d, const float4 g) {
#pragma clang fp contract(off)
  const double dx1 = d.x, dy1 = d.y, dx2 = d.z, dy2 = d.w;
  const double gx1 = g.x, gy1 = g.y, gx2 = g.z, gy2 = g.w;
  const double area_d = (dx2 - dx1) * (dy2 - dy1);
  const double area_g = (gx2 - gx1) * (gy2 - gy1);
  const double iw = fmax(0.0, fmin(dx2, gx2) - fmax(dx1, gx1));
  const double ih = fmax(0.0, fmin(dy2, gy2) - fmax(dy1, gy1));
  const double inter = iw * ih;
  const double uni = (area_d + area_g) - inter;
  return uni > 0.0 ? inter / uni : 0.0;
}

__device__ __forceinline__ int box_errors(const float4 b) {
  if (!(__builtin_isfinite(b.x) && __builtin_isfinite(b.y) && __builtin_isfinite(b.z) && __builtin_isfinite(b.w)))
    return kMapBadCoordinate;  // one kind per box: an infinite corner is not also an inverted box
  return b.z < b.x || b.w < b.y ? kMapBadBox : 0;
}

// ascending bitonic sort of s[0 .. P), P a power of two, by all kMapBlock threads (K13's, another key)
template <typename K>
__device__ __forceinline__ void bitonic_asc(K* s, int P) {
  for (int k = 2; k <= P; k <<= 1) {
    for (int j = k >> 1; j > 0; j >>= 1) {
      for (int i = threadIdx.x; i < (P >> 1); i += kMapBlock) {
        const int lo = ((i & ~(j - 1)) << 1) | (i & (j - 1));
        const int hi = lo + j;  // < P
        const K x = s[lo], y = s[hi];
        const bool asc = (lo & k) == 0;
        if ((x > y) == asc && x != y) {
          s[lo] = y;
          s[hi] = x;
        }
      }
      __syncthreads();
    }
  }
}

// the first position in s[lo .. hi) whose key is >= v (hi when none)
template <typename K>
__device__ __forceinline__ int lower_bound(const K* s, int lo, int hi, K v) {
  while (lo < hi) {
    const int mid = (lo + hi) >> 1;
    if (s[mid] < v) lo = mid + 1; else hi = mid;
  }
  return lo;
}

__device__ __forceinline__ int pow2_at_least(int n) {
  int p = 1;
  while (p < n) p <<= 1;
  return p;
}

__global__ __launch_bounds__(kMapBlock) void map_match_kernel(MapMatchArgs a) {
  __shared__ float4 s_dbox[kMapMaxBoxes];
  __shared__ float4 s_gbox[kMapMaxBoxes];
  __shared__ unsigned long long s_dkey[kMapMaxBoxes];
  __shared__ unsigned s_gkey[kMapMaxBoxes];
  __shared__ volatile unsigned short s_mask[kMapMaxBoxes];  // read by lanes other than the writer
  __shared__ unsigned short s_seg[kMapMaxBoxes];
  __shared__ double s_tmin[kMapMaxThresholds];
  __shared__ int s_nseg;
  const int lane = lane_id();
  const int wave = wave_id();
  const int T = a.num_thresholds;
  const int C = a.num_classes;
  if (threadIdx.x < T) s_tmin[threadIdx.x] = fmin(a.thresholds[threadIdx.x], 1.0 - 1e-10);
  int bad = 0;
  for (int img = blockIdx.x; img < a.num_images; img += gridDim.x) {
    // the host checked the offsets: sorted, each image within kMapMaxBoxes, the last the row count
    const int64_t d0 = a.offsets[img], g0 = a.offsets[a.num_images + 1 + img];
    const int nd = static_cast<int>(a.offsets[img + 1] - d0);
    const int ng = static_cast<int>(a.offsets[a.num_images + 2 + img] - g0);
    const int Pd = pow2_at_least(nd), Pg = pow2_at_least(ng);
    // ---- 1. stage the boxes, build the keys
    for (int i = threadIdx.x; i < Pd; i += kMapBlock) {
      unsigned long long key = ~0ull;
      if (i < nd) {
        const float4 b = load_f4u(a.det_boxes + (d0 + i) * 4);
        s_dbox[i] = b;
        const float s = load_as_f32(a.det_scores, a.score_dt, d0 + i);
        const int64_t l = load_as_i64(a.det_labels, a.det_label_dt, d0 + i);
        int e = box_errors(b);
        if (s != s) e |= kMapBadScore;
        if (l < 0 || l >= C) e |= kMapBadLabel;
        bad |= e;
        // a bad detection sorts behind every class, in input order
        key = e ? (static_cast<unsigned long long>(kNoClass) << 42) | static_cast<unsigned>(i)
                : (static_cast<unsigned long long>(l) << 42) |
                      (static_cast<unsigned long long>(~orderable(s)) << 10) | static_cast<unsigned>(i);
      }
      s_dkey[i] = key;
    }
    for (int i = threadIdx.x; i < Pg; i += kMapBlock) {
      unsigned key = ~0u;
      if (i < ng) {
        const float4 b = load_f4u(a.gt_boxes + (g0 + i) * 4);
        s_gbox[i] = b;
        const int64_t l = load_as_i64(a.gt_labels, a.gt_label_dt, g0 + i);
        int e = box_errors(b);
        if (l < 0 || l >= C) e |= kMapBadLabel;
        bad |= e;
        key = ((e ? kNoClass : static_cast<unsigned>(l)) << 10) | static_cast<unsigned>(i);
      }
      s_gkey[i] = key;
      s_mask[i] = 0;
    }
    if (threadIdx.x == 0) s_nseg = 0;
    __syncthreads();
    // ---- 2. order both lists
    bitonic_asc(s_dkey, Pd);
    bitonic_asc(s_gkey, Pg);
    // ---- the starts of the detection runs (in any order: a run's output place is its own), and
    // the ground truths per class
    for (int p = threadIdx.x; p < nd; p += kMapBlock) {
      const unsigned lab = static_cast<unsigned>(s_dkey[p] >> 42);
      if (p == 0 || static_cast<unsigned>(s_dkey[p - 1] >> 42) != lab) s_seg[atomicAdd(&s_nseg, 1)] = p;
    }
    for (int p = threadIdx.x; p < ng; p += kMapBlock) {
      const unsigned lab = s_gkey[p] >> 10;
      if (lab != kNoClass && (p == 0 || (s_gkey[p - 1] >> 10) != lab)) {
        const int end = lower_bound(s_gkey, p + 1, ng, (lab + 1u) << 10);
        atomicAdd(reinterpret_cast<unsigned long long*>(a.gt_count) + lab,
                  static_cast<unsigned long long>(end - p));
      }
    }
    __syncthreads();
    // ---- 3. a wave per run
    const int nseg = s_nseg;  // <= nd
    for (int sidx = wave; sidx < nseg; sidx += kWaves) {
      const int ds = s_seg[sidx];
      const unsigned lab = static_cast<unsigned>(s_dkey[ds] >> 42);
      const bool real = lab != kNoClass;
      const int de = real ? lower_bound(s_dkey, ds + 1, nd, static_cast<unsigned long long>(lab + 1u) << 42) : nd;
      const int n = de - ds;
      const int kept = real ? min(n, a.max_detections) : 0;
      const int64_t out0 = d0 + ds;
      for (int j = lane; j < n; j += kWave) {
        const int idx = static_cast<int>(s_dkey[ds + j] & kIndexMask);
        a.scores[out0 + j] = load_as_f32(a.det_scores, a.score_dt, d0 + idx);
        a.labels[out0 + j] = j < kept ? static_cast<int32_t>(lab) : -1;
        if (j >= kept) {
          a.hits[out0 + j] = 0;
          if (a.matched_gt)
            for (int k = 0; k < T; ++k) a.matched_gt[(out0 + j) * T + k] = -1;
        }
      }
      if (kept == 0) continue;
      const int gs = lower_bound(s_gkey, 0, ng, lab << 10);
      const int ge = lower_bound(s_gkey, gs, ng, (lab + 1u) << 10);
      const int chunks = (ge - gs + kWave - 1) / kWave;
      for (int j = 0; j < kept; ++j) {
        const float4 db = s_dbox[s_dkey[ds + j] & kIndexMask];
        const double iou0 = gs + lane < ge ? box_iou(db, s_gbox[s_gkey[gs + lane] & kIndexMask]) : -1.0;
        int hits = 0;
        for (int k = 0; k < T; ++k) {
          const double tmin = s_tmin[k];
          double best = -1.0;
          int pos = -1;
          for (int ch = 0; ch < chunks; ++ch) {
            const int p = gs + ch * kWave + lane;
            const bool valid = p < ge;
            double v = iou0;
            if (ch > 0) v = valid ? box_iou(db, s_gbox[s_gkey[p] & kIndexMask]) : -1.0;
            const bool cand = valid && !((s_mask[p] >> k) & 1) && v >= tmin;
            const unsigned long long any = __ballot(cand);
            if (any == 0ull) continue;  // wave-uniform
            const double m = wave_max(cand ? v : -1.0);
            if (m >= best) {  // a later chunk wins a tie: the later ground truth
              const unsigned long long win = __ballot(cand && v == m);
              best = m;
              pos = gs + ch * kWave + (63 - __clzll(static_cast<long long>(win)));
            }
          }
          if (pos >= 0) {
            hits |= 1 << k;
            if (lane == 0) s_mask[pos] = static_cast<unsigned short>(s_mask[pos] | (1u << k));
          }
          if (a.matched_gt && lane == 0)
            a.matched_gt[(out0 + j) * T + k] = pos >= 0 ? static_cast<int32_t>(s_gkey[pos] & kIndexMask) : -1;
        }
        if (lane == 0) a.hits[out0 + j] = hits;
      }
    }
    __syncthreads();  // the LDS arrays are free for the next image
  }
  if (a.err) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) bad |= __shfl_xor(bad, o, kWave);
    if (lane == 0 && bad) atomicOr(a.err, bad);
  }
}

// ------------------------------------------------------------------ curves
// the sum of one int per thread in every thread (wave sums in wave order)
__device__ __forceinline__ int block_total(int v, int* s_w) {
  v = wave_sum(v);
  if (lane_id() == 0) s_w[threadIdx.x >> 6] = v;
  __syncthreads();
  int t = 0;
  for (int w = 0; w < kMapCurveChunk / kWave; ++w) t += s_w[w];
  return t;
}

// U(x) = #{q : R[q] <= x} over the 101 recall points
__device__ __forceinline__ int count_le(const double* r, double x) {
  int lo = 0, hi = 101;
  while (lo < hi) {
    const int mid = (lo + hi) >> 1;
    if (r[mid] <= x) lo = mid + 1; else hi = mid;
  }
  return lo;
}

__global__ __launch_bounds__(kMapCurveChunk) void map_curve_kernel(MapCurveArgs a) {
  constexpr int W = kMapCurveChunk / kWave;
  __shared__ double s_R[101];
  __shared__ int s_wsum[W];
  __shared__ double s_wmax[W];
  __shared__ double s_wterm[W];
  const int lane = lane_id();
  const int wave = threadIdx.x >> 6;
  const int T = a.num_thresholds;
  const int64_t C = a.num_classes;
  // numpy.linspace(0, 1, 101): q * (1 / 100), the last exactly 1
  for (int q = threadIdx.x; q < 101; q += kMapCurveChunk) s_R[q] = q == 100 ? 1.0 : q * 0.01;
  __syncthreads();
  const int64_t pairs = C * T;
  for (int64_t pair = blockIdx.x; pair < pairs; pair += gridDim.x) {
    const int64_t c = pair / T;
    const int k = static_cast<int>(pair % T);
    const double ngt = a.gt_count[c];
    const int64_t s = a.class_offsets[c], e = a.class_offsets[c + 1];
    const int64_t n = e - s;
    if (!(ngt > 0.0) || n <= 0) {  // block-uniform
      if (threadIdx.x == 0) {
        const double v = ngt > 0.0 ? 0.0 : __longlong_as_double(0x7ff8000000000000ll);
        a.ap[k * C + c] = v;
        a.rec[k * C + c] = v;
      }
      continue;
    }
    int mine = 0;
    for (int64_t i = s + threadIdx.x; i < e; i += kMapCurveChunk) mine += (a.hits[i] >> k) & 1;
    const int total = block_total(mine, s_wsum);
    __syncthreads();  // s_wsum is read
    int running = total;  // hits at and left of the chunk's last position
    double carry = 0.0;   // the envelope right of the chunk (precisions are >= 0)
    double acc = 0.0;     // the same in every thread
    for (int64_t ch = (n - 1) / kMapCurveChunk; ch >= 0; --ch) {
      const int64_t j = ch * kMapCurveChunk + threadIdx.x;
      const bool valid = j < n;
      const int h = valid ? (a.hits[s + j] >> k) & 1 : 0;
      const int incl = wave_incl_sum(h);
      if (lane == kWave - 1) s_wsum[wave] = incl;
      __syncthreads();
      int before_wave = 0, chunk_hits = 0;
      for (int w = 0; w < W; ++w) {
        if (w < wave) before_wave += s_wsum[w];
        chunk_hits += s_wsum[w];
      }
      const int before = running - chunk_hits;
      const double tp = static_cast<double>(before + before_wave + incl);
      const double fp = static_cast<double>(j + 1) - tp;
      double env = valid ? tp / ((fp + tp) + 0x1p-52) : 0.0;
      // suffix maximum: within the wave, then over the waves to the right, then the carry
#pragma unroll
      for (int o = 1; o < kWave; o <<= 1) {
        const double y = __shfl_down(env, o, kWave);
        if (lane + o < kWave) env = fmax(env, y);
      }
      if (lane == 0) s_wmax[wave] = env;
      __syncthreads();
      double right = carry;
      for (int w = W - 1; w >= 0; --w) {
        if (w > wave) env = fmax(env, s_wmax[w]);
        right = fmax(right, s_wmax[w]);
      }
      env = fmax(env, carry);
      double term = 0.0;
      if (h) {  // the m-th hit serves the recall points in ((m - 1) / n_gt, m / n_gt]
        const double m = tp;
        const int u1 = count_le(s_R, m / ngt);
        const int u0 = m > 1.0 ? count_le(s_R, (m - 1.0) / ngt) : 0;
        term = static_cast<double>(u1 - u0) * env;
      }
      term = wave_sum(term);
      if (lane == 0) s_wterm[wave] = term;
      __syncthreads();
      for (int w = 0; w < W; ++w) acc += s_wterm[w];
      carry = right;
      running = before;
    }
    if (threadIdx.x == 0) {
      a.ap[k * C + c] = acc / 101.0;
      a.rec[k * C + c] = static_cast<double>(total) / ngt;
    }
    __syncthreads();  // s_wterm is read before the next pair writes the arrays
  }
}

// the sum of one double per thread in every thread, in a fixed order
__device__ __forceinline__ double block_total(double v, double* s_w) {
  v = wave_sum(v);
  __syncthreads();
  if (lane_id() == 0) s_w[threadIdx.x >> 6] = v;
  __syncthreads();
  double t = 0.0;
  for (int w = 0; w < kMapCurveChunk / kWave; ++w) t += s_w[w];
  return t;
}

__global__ __launch_bounds__(kMapCurveChunk) void map_finish_kernel(MapCurveArgs a) {
  __shared__ double s_w[kMapCurveChunk / kWave];
  const int T = a.num_thresholds;
  const int64_t C = a.num_classes;
  double sum_ap = 0.0, sum_rec = 0.0, sum_50 = 0.0, sum_75 = 0.0, live = 0.0;
  for (int64_t c = threadIdx.x; c < C; c += kMapCurveChunk) {
    double ap = 0.0, rec = 0.0;
    for (int k = 0; k < T; ++k) {
      ap += a.ap[k * C + c];
      rec += a.rec[k * C + c];
    }
    a.map_per_class[c] = static_cast<float>(ap / T);  // NaN without ground truth
    a.mar_per_class[c] = static_cast<float>(rec / T);
    if (a.gt_count[c] > 0.0) {
      sum_ap += ap;
      sum_rec += rec;
      live += 1.0;
      if (a.index_50 >= 0) sum_50 += a.ap[a.index_50 * C + c];
      if (a.index_75 >= 0) sum_75 += a.ap[a.index_75 * C + c];
    }
  }
  sum_ap = block_total(sum_ap, s_w);
  sum_rec = block_total(sum_rec, s_w);
  sum_50 = block_total(sum_50, s_w);
  sum_75 = block_total(sum_75, s_w);
  live = block_total(live, s_w);
  if (threadIdx.x == 0) {
    const float nan = __uint_as_float(0x7fc00000u);
    const bool any = live > 0.0;
    a.scalars[0] = any ? static_cast<float>(sum_ap / (live * T)) : nan;
    a.scalars[1] = any && a.index_50 >= 0 ? static_cast<float>(sum_50 / live) : nan;
    a.scalars[2] = any && a.index_75 >= 0 ? static_cast<float>(sum_75 / live) : nan;
    a.scalars[3] = any ? static_cast<float>(sum_rec / (live * T)) : nan;
  }
}

bool label_dtype(DType dt) { return dt == DType::i64 || dt == DType::i32; }

}  // namespace

int launch_map_match(const MapMatchArgs& a, hipStream_t stream) {
  if (a.num_images <= 0) return 0;
  if (a.num_thresholds < 1 || a.num_thresholds > kMapMaxThresholds || a.num_classes < 1 ||
      a.num_classes > kMapMaxClasses || a.max_detections < 1)
    return -1;
  if (!label_dtype(a.det_label_dt) || !label_dtype(a.gt_label_dt)) return -1;
  if (a.score_dt != DType::f32 && a.score_dt != DType::f16 && a.score_dt != DType::bf16) return -1;
  if (a.offsets == nullptr || a.thresholds == nullptr || a.gt_count == nullptr) return -1;
  const int blocks = a.num_images < kMapGrid ? a.num_images : kMapGrid;
  hipLaunchKernelGGL(map_match_kernel, dim3(blocks), dim3(kMapBlock), 0, stream, a);
  return static_cast<int>(hipGetLastError());
}

int launch_map_curve(const MapCurveArgs& a, hipStream_t stream) {
  if (a.num_classes < 1 || a.num_thresholds < 1 || a.num_thresholds > kMapMaxThresholds) return -1;
  if (a.index_50 >= a.num_thresholds || a.index_75 >= a.num_thresholds) return -1;
  if (a.class_offsets == nullptr || a.gt_count == nullptr || a.ap == nullptr || a.rec == nullptr) return -1;
  const int64_t pairs = static_cast<int64_t>(a.num_classes) * a.num_thresholds;
  const int blocks = static_cast<int>(pairs < kMapCurveGrid ? pairs : kMapCurveGrid);
  hipLaunchKernelGGL(map_curve_kernel, dim3(blocks), dim3(kMapCurveChunk), 0, stream, a);
  int rc = static_cast<int>(hipGetLastError());
  if (rc || a.scalars == nullptr) return rc;
  hipLaunchKernelGGL(map_finish_kernel, dim3(1), dim3(kMapCurveChunk), 0, stream, a);
  return static_cast<int>(hipGetLastError());
}

}  // namespace tea
