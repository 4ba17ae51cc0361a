// K28: panoptic quality (PQ / SQ / RQ), docs/parity.md "Not in the reference".
//
// Replaces the ATen form (functional/classification/panoptic_quality.py): per image a host-synchronising
// unique(dim=0) over the canonical (segment, segment) rows and a chain of bincounts.  A segment is an
// arbitrary (category, instance) pair, so the table of co-occurring pairs is sparse and has no bound the
// host knows; here it is interned in LDS open-addressing tables, in three launches:
//  * panoptic_pairs_kernel reads both maps once.  A block owns a span of kPanSpan consecutive pixels of
//    one image at a time (persistent grid); a pixel is one 16-B (int64 maps) or 8-B (int32) load and all
//    of a thread's loads of both maps are issued before the first compare.  A wave folds its pixels by
//    raw (pc, pi, tc, ti) tuple, kFoldRounds tuples at most (K17's fold: ballot, leader, readlane, ballot
//    of the equal lanes, popcount), so a wave inside one segment pair costs one insert; leftover lanes
//    insert singly.  Only an inserting lane maps its tuple to canonical keys (binary search of the
//    category table in LDS; a stuff instance zeroed, an unknown category the void key); raw tuples that
//    share a canonical key are merged by the tables.  Two segment tables (u64 key, 64-bit CAS claim) and
//    one pair table (u32 key pslot << 16 | tslot, u32 count) of 2 * kPanSpan slots each, linear probe
//    bounded by the table size: a span cannot fill them.  A claimed slot is appended to a list through
//    one LDS counter, and emission and clearing walk the lists only.  The block then stores the span's
//    pairs as (pkey, tkey, count) into the span's own region of the workspace, a count first.
//    kPanSpan = 1024: the tables, lists and the category table are 63 KiB, so two blocks share a CU's
//    160 KiB and one hides the other's barriers and probe chains; at 2048 the block would be alone on
//    its CU.  One arm, untuned: 2048 was not measured.
//  * panoptic_match_kernel, one workgroup of 1024 threads per image (persistent): its waves walk the
//    image's span regions and intern both keys into image-level tables with the same device function,
//    adding the counts into the pair table and both areas with LDS integer atomics.  kPanMaxSegments
//    = 1024 segments a side in 2048 slots and kPanMaxPairs = 4096 pairs in 8192 slots: 159760 B of LDS
//    with the class counters.  An image above either sets kPanFlagCapacity and contributes nothing.
//    Pass A stores the void overlap of every segment (plain stores, one pair per segment), pass B
//    applies the integer match test 2 * inter > union, marks both segments and adds 1 to tp[class] and
//    llrint(ldexp(inter / union, 52)) to a u64 iou_fix[class], pass C counts the unmatched segments
//    whose void share is at most a half as fp / fn.  The IoU sum is an integer sum, so the racy slot
//    order cannot change a bit of it; tp <= 1024 per image and class keeps it below 2^63.
//  * panoptic_finish_kernel, one workgroup: per class the images' partials in image order into the
//    four float64 states (iou_fix scaled by 2^-52 as a double, per image), or into a scratch quadruple
//    whose PQ / SQ / RQ the first wave evaluates in the same launch.
// The only global atomic is the flag's atomicOr; no workgroup waits for another; every store of a
// result is non-atomic: bit-identical from run to run.
#include <type_traits>

#include "tea_common.h"
#include "tea_kernels.h"

namespace tea {

namespace {

constexpr int kB = 256;                // threads of a pairs block
constexpr int kPerThread = kPanSpan / kB;
constexpr int kFoldRounds = 2;         // distinct raw tuples a wave folds before its lanes insert singly
constexpr int kSpanBits = 11;          // 2 * kPanSpan slots in each span-level table
constexpr int kMatchThreads = 1024;
constexpr int kMatchMaxBlocks = 512;
constexpr int kImgSegBits = 11;        // 2 * kPanMaxSegments slots
constexpr int kImgPairBits = 13;       // 2 * kPanMaxPairs slots
constexpr int kFinishThreads = 1024;
constexpr unsigned long long kEmptyKey = ~0ull;
constexpr unsigned long long kPanVoidKey = 0xFFFFFFFEull << 32;
constexpr uint32_t kMatched = 1u << 31;  // bit of a segment's void word
static_assert((1 << kSpanBits) == 2 * kPanSpan && kPanSpan % kB == 0, "a span fills at most half of its tables");
static_assert((1 << kImgSegBits) == 2 * kPanMaxSegments && (1 << kImgPairBits) == 2 * kPanMaxPairs, "likewise");
static_assert((1 << kImgSegBits) <= (1 << 16), "a pair key holds two slot indices");

typedef long long ll2u_t __attribute__((ext_vector_type(2), aligned(8)));
typedef int i2u_t __attribute__((ext_vector_type(2), aligned(4)));

__device__ __forceinline__ int readlane_int(int v, int l) { return __builtin_amdgcn_readlane(v, l); }
__device__ __forceinline__ long long readlane_int(long long v, int l) {
  const int lo = __builtin_amdgcn_readlane(static_cast<int>(v), l);
  const int hi = __builtin_amdgcn_readlane(static_cast<int>(v >> 32), l);
  return (static_cast<long long>(hi) << 32) | static_cast<unsigned int>(lo);
}

// Finds or claims `key` in an open-addressing table of 1 << bits words (empty: all ones) and returns
// its slot; -1 when every slot holds another key.  A claimed slot is appended to `list` (`cap` entries;
// a claim past it only counts) through `*count`.
template <typename Key>
__device__ __forceinline__ int intern(Key* tab, int bits, Key key, uint16_t* list, uint32_t* count, uint32_t cap) {
  const uint32_t mask = (1u << bits) - 1u;
  uint32_t s;
  if constexpr (sizeof(Key) == 8) s = static_cast<uint32_t>((key * 0x9E3779B97F4A7C15ull) >> (64 - bits));
  else s = (key * 0x9E3779B1u) >> (32 - bits);
  for (uint32_t i = 0; i <= mask; ++i, s = (s + 1u) & mask) {
    const Key old = atomicCAS(&tab[s], static_cast<Key>(~Key(0)), key);
    if (old == static_cast<Key>(~Key(0))) {
      const uint32_t at = atomicAdd(count, 1u);
      if (at < cap) list[at] = static_cast<uint16_t>(s);
      return static_cast<int>(s);
    }
    if (old == key) return static_cast<int>(s);
  }
  return -1;
}

// the canonical key of a raw (category, instance): binary search of the k ascending categories
__device__ __forceinline__ unsigned long long canonical(long long cat, long long inst, const long long* s_cat,
                                                        const uint8_t* s_thing, int k, int unknown_bit, int& flags) {
  int lo = 0, hi = k;
  while (lo < hi) {
    const int mid = (lo + hi) >> 1;
    if (s_cat[mid] < cat) lo = mid + 1;
    else hi = mid;
  }
  if (lo == k || s_cat[lo] != cat) {
    flags |= unknown_bit;
    return kPanVoidKey;
  }
  const unsigned long long cls = static_cast<unsigned long long>(lo) << 32;
  if (!s_thing[lo]) return cls;
  if (inst < 0 || inst > 0xFFFFFFFFll) flags |= kPanFlagInstance;
  return cls | static_cast<uint32_t>(inst);
}

// T: long long (int64 maps) or int (int32 maps)
template <typename T>
__global__ __launch_bounds__(kB) void panoptic_pairs_kernel(PanopticArgs a) {
  using Pixel = typename std::conditional<sizeof(T) == 8, ll2u_t, i2u_t>::type;
  __shared__ unsigned long long s_seg[2][1 << kSpanBits];
  __shared__ long long s_cat[kPanMaxClasses];
  __shared__ uint32_t s_pair[1 << kSpanBits], s_count[1 << kSpanBits];
  __shared__ uint32_t s_n[3];  // claimed predicted segments, target segments, pairs
  __shared__ uint16_t s_seg_list[2][kPanSpan], s_pair_list[kPanSpan];
  __shared__ uint8_t s_thing[kPanMaxClasses];
  const int K = a.k;
  for (int i = threadIdx.x; i < (1 << kSpanBits); i += kB) {
    s_seg[0][i] = kEmptyKey, s_seg[1][i] = kEmptyKey;
    s_pair[i] = ~0u, s_count[i] = 0u;
  }
  for (int i = threadIdx.x; i < K; i += kB) {
    s_cat[i] = a.table[i];
    s_thing[i] = a.table[K + i] != 0 ? 1 : 0;
  }
  if (threadIdx.x < 3) s_n[threadIdx.x] = 0u;
  __syncthreads();
  const int lane = lane_id();
  const int unknown_bit = a.allow_unknown ? 0 : kPanFlagUnknown;
  const int64_t spans_per_image = (a.p + kPanSpan - 1) / kPanSpan;
  const int64_t spans = a.n * spans_per_image;
  const Pixel* in = static_cast<const Pixel*>(a.input);
  const Pixel* tg = static_cast<const Pixel*>(a.target);
  int flags = 0;
  for (int64_t s = blockIdx.x; s < spans; s += gridDim.x) {
    const int64_t n = s / spans_per_image;
    const int64_t lo = (s - n * spans_per_image) * kPanSpan;
    const int64_t hi = lo + kPanSpan < a.p ? lo + kPanSpan : a.p;
    Pixel x[kPerThread], y[kPerThread];
    bool live[kPerThread];
#pragma unroll
    for (int j = 0; j < kPerThread; ++j) {
      const int64_t q = lo + j * kB + threadIdx.x;
      live[j] = q < hi;
      x[j] = Pixel{0, 0}, y[j] = Pixel{0, 0};
      if (live[j]) x[j] = in[n * a.p + q], y[j] = tg[n * a.p + q];
    }
#pragma unroll
    for (int j = 0; j < kPerThread; ++j) {
      const T pc = x[j].x, pi = x[j].y, tc = y[j].x, ti = y[j].y;
      uint32_t cnt = live[j] ? 1u : 0u;  // pixels this lane inserts for
      uint64_t todo = __ballot(live[j]);
      for (int r = 0; r < kFoldRounds && todo != 0; ++r) {
        const int leader = __builtin_amdgcn_readfirstlane(__ffsll(static_cast<unsigned long long>(todo)) - 1);
        const bool same = ((todo >> lane) & 1) != 0 && pc == readlane_int(pc, leader) &&
                          pi == readlane_int(pi, leader) && tc == readlane_int(tc, leader) &&
                          ti == readlane_int(ti, leader);
        const uint64_t members = __ballot(same);
        if (same) cnt = lane == leader ? static_cast<uint32_t>(__popcll(members)) : 0u;
        todo &= ~members;
      }
      if (cnt != 0u) {
        const unsigned long long pk = canonical(pc, pi, s_cat, s_thing, K, unknown_bit, flags);
        const unsigned long long tk = canonical(tc, ti, s_cat, s_thing, K, 0, flags);
        const int ps = intern(s_seg[0], kSpanBits, pk, s_seg_list[0], &s_n[0], kPanSpan);
        const int ts = intern(s_seg[1], kSpanBits, tk, s_seg_list[1], &s_n[1], kPanSpan);
        if (ps >= 0 && ts >= 0) {
          const int at = intern(s_pair, kSpanBits, static_cast<uint32_t>(ps) << 16 | static_cast<uint32_t>(ts),
                                s_pair_list, &s_n[2], kPanSpan);
          if (at >= 0) atomicAdd(&s_count[at], cnt);
        }
      }
    }
    __syncthreads();
    // the span's pairs into its region, then the claimed slots back to empty
    const int segs0 = min(s_n[0], static_cast<uint32_t>(kPanSpan)), segs1 = min(s_n[1], static_cast<uint32_t>(kPanSpan));
    const int pairs = min(s_n[2], static_cast<uint32_t>(kPanSpan));
    unsigned long long* keys = a.ws_keys + s * 2 * kPanSpan;
    uint32_t* counts = a.ws_counts + s * kPanSpan;
    for (int i = threadIdx.x; i < pairs; i += kB) {
      const int at = s_pair_list[i];
      const uint32_t pair = s_pair[at];
      keys[i] = s_seg[0][pair >> 16];
      keys[kPanSpan + i] = s_seg[1][pair & 0xFFFFu];
      counts[i] = s_count[at];
    }
    if (threadIdx.x == 0) a.ws_heads[s] = static_cast<uint32_t>(pairs);
    __syncthreads();
    for (int i = threadIdx.x; i < pairs; i += kB) {
      const int at = s_pair_list[i];
      s_pair[at] = ~0u, s_count[at] = 0u;
    }
    for (int i = threadIdx.x; i < segs0; i += kB) s_seg[0][s_seg_list[0][i]] = kEmptyKey;
    for (int i = threadIdx.x; i < segs1; i += kB) s_seg[1][s_seg_list[1][i]] = kEmptyKey;
    if (threadIdx.x < 3) s_n[threadIdx.x] = 0u;
    __syncthreads();
  }
  if (flags != 0) atomicOr(a.flag, flags);
}

// ---------------------------------------------------------------- match: one workgroup per image
struct ImageTables {
  unsigned long long seg[2][1 << kImgSegBits];  // canonical keys: predicted, target
  unsigned long long iou_fix[kPanMaxClasses];
  uint32_t pair[1 << kImgPairBits], count[1 << kImgPairBits];
  uint32_t area[2][1 << kImgSegBits];
  uint32_t voidm[2][1 << kImgSegBits];  // pixels shared with the other side's void segment; kMatched
  uint32_t tp[kPanMaxClasses], fpfn[kPanMaxClasses];  // fpfn: fp in the low half, fn in the high (<= 1024 each)
  uint16_t seg_list[2][kPanMaxSegments], pair_list[kPanMaxPairs];
  uint32_t n[3];  // claimed predicted segments, target segments, pairs
  uint32_t over;
};
static_assert(sizeof(ImageTables) <= 160 * 1024, "one workgroup's tables fit a CU's LDS");

__global__ __launch_bounds__(kMatchThreads) void panoptic_match_kernel(PanopticArgs a) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  ImageTables& t = *reinterpret_cast<ImageTables*>(smem);
  const int K = a.k;
  const int tid = threadIdx.x, lane = lane_id(), wave = tid >> 6;
  const int64_t spans_per_image = (a.p + kPanSpan - 1) / kPanSpan;
  for (int64_t img = blockIdx.x; img < a.n; img += gridDim.x) {
    __syncthreads();  // the previous image's tables are read no more
    for (int i = tid; i < (1 << kImgSegBits); i += kMatchThreads) {
      t.seg[0][i] = kEmptyKey, t.seg[1][i] = kEmptyKey;
      t.area[0][i] = 0u, t.area[1][i] = 0u, t.voidm[0][i] = 0u, t.voidm[1][i] = 0u;
    }
    for (int i = tid; i < (1 << kImgPairBits); i += kMatchThreads) t.pair[i] = ~0u, t.count[i] = 0u;
    for (int i = tid; i < kPanMaxClasses; i += kMatchThreads) t.iou_fix[i] = 0ull, t.tp[i] = 0u, t.fpfn[i] = 0u;
    if (tid < 3) t.n[tid] = 0u;
    if (tid == 3) t.over = 0u;
    __syncthreads();
    // a wave takes every 16th span region of the image, a lane every 64th pair of the region
    for (int64_t sp = wave; sp < spans_per_image; sp += kMatchThreads / kWave) {
      const int64_t s = img * spans_per_image + sp;
      const int pairs = min(a.ws_heads[s], static_cast<uint32_t>(kPanSpan));
      const unsigned long long* keys = a.ws_keys + s * 2 * kPanSpan;
      const uint32_t* counts = a.ws_counts + s * kPanSpan;
      for (int i = lane; i < pairs; i += kWave) {
        const uint32_t c = counts[i];
        const int ps = intern(t.seg[0], kImgSegBits, keys[i], t.seg_list[0], &t.n[0], kPanMaxSegments);
        const int ts = intern(t.seg[1], kImgSegBits, keys[kPanSpan + i], t.seg_list[1], &t.n[1], kPanMaxSegments);
        int at = -1;
        if (ps >= 0 && ts >= 0) {
          atomicAdd(&t.area[0][ps], c);
          atomicAdd(&t.area[1][ts], c);
          at = intern(t.pair, kImgPairBits, static_cast<uint32_t>(ps) << 16 | static_cast<uint32_t>(ts), t.pair_list,
                      &t.n[2], kPanMaxPairs);
        }
        if (at >= 0) atomicAdd(&t.count[at], c);
        else t.over = 1u;
      }
    }
    __syncthreads();
    unsigned long long* out_iou = a.part_iou + img * K;
    uint32_t* out_counts = a.part_counts + img * 3 * K;
    if (t.over != 0u || t.n[0] > kPanMaxSegments || t.n[1] > kPanMaxSegments || t.n[2] > kPanMaxPairs) {
      if (tid == 0) atomicOr(a.flag, kPanFlagCapacity);
      for (int c = tid; c < K; c += kMatchThreads)
        out_iou[c] = 0ull, out_counts[c] = 0u, out_counts[K + c] = 0u, out_counts[2 * K + c] = 0u;
      continue;
    }
    const int pairs = static_cast<int>(t.n[2]);
    // pass A: a segment's overlap with the other side's void segment
    for (int i = tid; i < pairs; i += kMatchThreads) {
      const int at = t.pair_list[i];
      const uint32_t ps = t.pair[at] >> 16, ts = t.pair[at] & 0xFFFFu;
      if (t.seg[1][ts] == kPanVoidKey) t.voidm[0][ps] = t.count[at];
      if (t.seg[0][ps] == kPanVoidKey) t.voidm[1][ts] = t.count[at];
    }
    __syncthreads();
    // pass B: the matches
    for (int i = tid; i < pairs; i += kMatchThreads) {
      const int at = t.pair_list[i];
      const uint32_t ps = t.pair[at] >> 16, ts = t.pair[at] & 0xFFFFu;
      const unsigned long long pk = t.seg[0][ps], tk = t.seg[1][ts];
      const uint32_t cls = static_cast<uint32_t>(pk >> 32);
      if (pk == kPanVoidKey || tk == kPanVoidKey || cls != static_cast<uint32_t>(tk >> 32) || cls >= K) continue;
      const long long inter = t.count[at];
      const long long uni = static_cast<long long>(t.area[0][ps]) - (t.voidm[0][ps] & ~kMatched) + t.area[1][ts] - inter;
      if (2 * inter > uni) {
        atomicOr(&t.voidm[0][ps], kMatched);
        atomicOr(&t.voidm[1][ts], kMatched);
        atomicAdd(&t.tp[cls], 1u);
        const double iou = static_cast<double>(inter) / static_cast<double>(uni);
        atomicAdd(&t.iou_fix[cls], static_cast<unsigned long long>(llrint(ldexp(iou, 52))));
      }
    }
    __syncthreads();
    // pass C: unmatched segments of which at most a half is void
    for (int side = 0; side < 2; ++side) {
      const int segs = static_cast<int>(t.n[side]);
      for (int i = tid; i < segs; i += kMatchThreads) {
        const int at = t.seg_list[side][i];
        const unsigned long long key = t.seg[side][at];
        const uint32_t cls = static_cast<uint32_t>(key >> 32), v = t.voidm[side][at];
        if (key == kPanVoidKey || cls >= K || (v & kMatched) != 0u) continue;
        if (2ull * v <= t.area[side][at]) atomicAdd(&t.fpfn[cls], side == 0 ? 1u : 1u << 16);
      }
    }
    __syncthreads();
    for (int c = tid; c < K; c += kMatchThreads) {
      out_iou[c] = t.iou_fix[c];
      out_counts[c] = t.tp[c];
      out_counts[K + c] = t.fpfn[c] & 0xFFFFu;
      out_counts[2 * K + c] = t.fpfn[c] >> 16;
    }
  }
}

// ---------------------------------------------------------------- value and finish
// By one whole wave: (PQ, SQ, RQ) in FP64 per class, [k, 3], or their means over the classes whose
// denominator is not zero, [3]
__device__ void panoptic_value(const double* iou_sum, const double* tp, const double* fp, const double* fn, int64_t K,
                               int per_class, float* out, int lane) {
  double sum[3] = {0.0, 0.0, 0.0}, num[3] = {0.0, 0.0, 0.0};
  for (int64_t c = lane; c < K; c += kWave) {
    const double den = tp[c] + 0.5 * fp[c] + 0.5 * fn[c];
    const double v[3] = {iou_sum[c] / den, iou_sum[c] / tp[c], tp[c] / den};
    const double d[3] = {den, tp[c], den};
#pragma unroll
    for (int j = 0; j < 3; ++j) {
      if (per_class) {
        out[c * 3 + j] = static_cast<float>(v[j]);
      } else if (d[j] > 0.0) {
        sum[j] += v[j];
        num[j] += 1.0;
      }
    }
  }
  if (per_class) return;
#pragma unroll
  for (int j = 0; j < 3; ++j) {
    const double s = wave_sum(sum[j]), m = wave_sum(num[j]);
    if (lane == 0) out[j] = static_cast<float>(s / m);
  }
}

__global__ __launch_bounds__(kFinishThreads) void panoptic_finish_kernel(PanopticArgs a) {
  const int K = a.k;
  for (int c = threadIdx.x; c < K; c += kFinishThreads) {
    double acc[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) acc[j] = a.accumulate ? a.dst[j][c] : 0.0;
    for (int64_t i = 0; i < a.n; ++i) {
      acc[0] += static_cast<double>(a.part_iou[i * K + c]) * 0x1p-52;
#pragma unroll
      for (int j = 0; j < 3; ++j) acc[1 + j] += static_cast<double>(a.part_counts[(i * 3 + j) * K + c]);
    }
#pragma unroll
    for (int j = 0; j < 4; ++j) a.dst[j][c] = acc[j];
  }
  __syncthreads();
  if (a.out && threadIdx.x < kWave)
    panoptic_value(a.dst[0], a.dst[1], a.dst[2], a.dst[3], K, a.per_class, a.out, threadIdx.x);
}

__global__ __launch_bounds__(kWave) void panoptic_value_kernel(const double* iou_sum, const double* tp, const double* fp,
                                                               const double* fn, int64_t K, int per_class, float* out) {
  panoptic_value(iou_sum, tp, fp, fn, K, per_class, out, threadIdx.x);
}

}  // namespace

int launch_panoptic(const PanopticArgs& a, hipStream_t stream) {
  if (a.n <= 0 || a.p <= 0) return 0;
  if (a.k < 1 || a.k > kPanMaxClasses || a.p >= (int64_t{1} << 31)) return -1;
  if (a.input == nullptr || a.target == nullptr || a.table == nullptr || a.flag == nullptr) return -1;
  if (a.ws_keys == nullptr || a.ws_counts == nullptr || a.ws_heads == nullptr) return -1;
  if (a.part_iou == nullptr || a.part_counts == nullptr) return -1;
  for (int j = 0; j < 4; ++j)
    if (a.dst[j] == nullptr) return -1;
  static const bool lds_ok =
      hipFuncSetAttribute(reinterpret_cast<const void*>(&panoptic_match_kernel),
                          hipFuncAttributeMaxDynamicSharedMemorySize, sizeof(ImageTables)) == hipSuccess;
  if (!lds_ok) return -3;
  const int blocks = stream_grid(panoptic_spans(a.n, a.p), 1, kPanMaxBlocks);
  if (a.wide) hipLaunchKernelGGL(panoptic_pairs_kernel<long long>, dim3(blocks), dim3(kB), 0, stream, a);
  else hipLaunchKernelGGL(panoptic_pairs_kernel<int>, dim3(blocks), dim3(kB), 0, stream, a);
  hipLaunchKernelGGL(panoptic_match_kernel, dim3(stream_grid(a.n, 1, kMatchMaxBlocks)), dim3(kMatchThreads),
                     sizeof(ImageTables), stream, a);
  hipLaunchKernelGGL(panoptic_finish_kernel, dim3(1), dim3(kFinishThreads), 0, stream, a);
  return static_cast<int>(hipGetLastError());
}

int launch_panoptic_value(const double* iou_sum, const double* tp, const double* fp, const double* fn, int64_t k,
                          int per_class, float* out, hipStream_t stream) {
  if (k < 1 || iou_sum == nullptr || tp == nullptr || fp == nullptr || fn == nullptr || out == nullptr) return -1;
  hipLaunchKernelGGL(panoptic_value_kernel, dim3(1), dim3(kWave), 0, stream, iou_sum, tp, fp, fn, k, per_class, out);
  return static_cast<int>(hipGetLastError());
}

}  // namespace tea
