// K25: pair-counting and information clustering indices of two labelings, docs/parity.md "Not in the
// reference".  Rand, adjusted Rand, Fowlkes-Mallows, mutual information, NMI, AMI, homogeneity and
// completeness are all functions of the rectangular contingency table n[i, j] = #{s : true[s] = i,
// pred[s] = j}, kept as an additive int64 [R, C] state.
//
// Replaces the ATen form (functional/clustering/contingency.py): bincount over true * C + pred,
// nonzero / log chains over the table and, for AMI's expected mutual information, an lgamma table
// with a Python loop over n.
//  * contingency_count_kernel<S, B>: the table is cut into slices of S consecutive cells that live
//    in LDS as u32.  Block (slice, group) walks its group's samples, kCtgUnit label pairs per thread
//    and step in 16-byte loads (a scalar head brings labels_true to a 16-byte boundary and a scalar
//    tail takes the rest, K7's scheme; labels_pred is loaded at its own alignment, which gfx950
//    serves at the aligned rate: profiles/unaligned_probe_r5.txt), checks the labels in 64-bit, forms
//    cell = true * C + pred (below 2^22 once they passed) and counts the cells of its own slice with
//    LDS integer atomics.  A wave first folds the lanes that hold the same cell (K17's ballot /
//    leader / popcount, kFoldRounds cells at most), so a dominant cluster does not serialise 64
//    lanes on one LDS address; a wave with at most kFoldSparse pairs in the slice skips the fold.
//    kAhead units' loads are in flight per thread.  Flush: lanes own consecutive cells of the slice
//    and every non-zero cell goes out as one no-return 64-bit integer atomic add.
//    A table of at most S cells is one slice and every label is read once; a larger table re-reads
//    the labels once per slice.  A label outside its range is counted nowhere and sets bit 0 of
//    `err`, the only other atomic.
//  * contingency_cells_kernel + contingency_margins_kernel (launch_contingency_stats): one read of
//    the table.  A wave owns kRows rows of one 64-column segment at a time, so its loads are 512
//    contiguous bytes; row and column sums leave as integer atomics, sum n (n - 1) / 2 as u64, and
//    sum n log n as one FP64 partial per block, stored non-atomically.  The marginal pass does the
//    same for the finished row and column sums and writes EMI's tables of log x and
//    lgamma(x + 1) + lgamma(N - x + 1).
//  * contingency_emi_kernel: EMI = sum_ij sum_n (n / N) log(N n / (a_i b_j)) p(n), p hypergeometric.
//    A wave-item is 1 / P of one pair's n-range (P = contingency_emi_parts: more parts when the table
//    has few pairs), cut into 64 contiguous lane chunks.  A lane evaluates log p at its chunk's first
//    n from four lgammas on top of the tables, takes one exp, and steps with
//    p(n + 1) / p(n) = (a - n)(b - n) / ((n + 1)(N - a - b + n + 1)); one FP64 log(n) per term is left.
//    p is unimodal, so a chunk that starts below exp(kLogFloor) on the falling side, or rises but
//    still ends below it, is skipped, and a rising chunk that starts below it walks to where p is
//    representable and starts from the lgammas there: every term left out is below 1e-300.
//    Sums are FP64 in a fixed order (lane, wave, one partial per block); no cross-workgroup waiting.
//  * contingency_values_kernel: one wave forms every value in FP64 from the statistics.
#include "tea_common.h"
#include "tea_kernels.h"
#include "tea_partials.h"

namespace tea {

namespace {

static_assert(kCtgMaxCells <= (1 << 22), "a cell index is formed with a 24-bit multiply");
constexpr int kFoldRounds = 2;   // distinct cells a wave folds before its lanes add singly
constexpr int kFoldSparse = 4;   // live lanes of a wave up to which nothing is folded
constexpr int kAhead = 2;        // units of a thread whose loads are issued before the first is counted
constexpr int kStatBlock = 256;  // threads of the statistics and EMI kernels
constexpr int kStatWaves = kStatBlock / kWave;
constexpr int kRows = 16;        // rows of a cell-pass item
constexpr int kEmiTargetItems = 4096;  // wave-items the EMI launch aims for when the table has few pairs
constexpr double kLogFloor = -700.0;   // exp(-700) = 1e-304: still a normal double
constexpr double kTiny = 1e-300;

typedef long long ll2u_t __attribute__((ext_vector_type(2), aligned(8)));
typedef int i4u_t __attribute__((ext_vector_type(4), aligned(4)));

// kCtgUnit consecutive labels from element i, in 16-byte loads at the element's own alignment
__device__ __forceinline__ void load_labels(const void* p, DType dt, int64_t i, int64_t (&v)[kCtgUnit]) {
  if (dt == DType::i64) {
    const ll2u_t* q = reinterpret_cast<const ll2u_t*>(static_cast<const int64_t*>(p) + i);
    const ll2u_t x = q[0], y = q[1];
    v[0] = x.x, v[1] = x.y, v[2] = y.x, v[3] = y.y;
  } else {
    const i4u_t x = *reinterpret_cast<const i4u_t*>(static_cast<const int32_t*>(p) + i);
    v[0] = x.x, v[1] = x.y, v[2] = x.z, v[3] = x.w;
  }
}

__device__ __forceinline__ int64_t load_label(const void* p, DType dt, int64_t i) {
  return dt == DType::i64 ? static_cast<const int64_t*>(p)[i] : static_cast<const int32_t*>(p)[i];
}

// the cell of a pair inside the slice [lo, lo + live), -1 outside it or for a bad label.  The labels
// are compared in 64-bit; a pair that passes has true < R and pred < C with R C <= kCtgMaxCells = 2^22,
// so its cell is exact in a 24-bit multiply and 32-bit adds
__device__ __forceinline__ int slice_key(int64_t t, int64_t p, int64_t R, int64_t C, int lo, int live, int& flags) {
  if (static_cast<uint64_t>(t) >= static_cast<uint64_t>(R) || static_cast<uint64_t>(p) >= static_cast<uint64_t>(C)) {
    flags |= kCtgBadLabel;
    return -1;
  }
  const int local = __mul24(static_cast<int>(t), static_cast<int>(C)) + static_cast<int>(p) - lo;
  return local >= 0 && local < live ? local : -1;
}

// One pair of every lane (key < 0: none) into the slice.  Called by whole waves.  With at most
// kFoldSparse live lanes (a table of many slices: most pairs belong to other blocks) the lanes add
// themselves, since no address can then serialise more than that many of them.
__device__ __forceinline__ void fold(int key, uint32_t* cells, int lane) {
  uint64_t todo = __ballot(key >= 0);
  if (__popcll(todo) > kFoldSparse) {
    for (int r = 0; r < kFoldRounds && todo != 0; ++r) {
      const int leader = __builtin_amdgcn_readfirstlane(__ffsll(static_cast<unsigned long long>(todo)) - 1);
      const int k = __builtin_amdgcn_readlane(key, leader);
      const uint64_t members = __ballot(key == k);
      if (lane == 0) atomicAdd(&cells[k], static_cast<uint32_t>(__popcll(members)));
      if (key == k) key = -1;
      todo &= ~members;
    }
  }
  if (key >= 0) atomicAdd(&cells[key], 1u);
}

template <int S, int B>
__global__ __launch_bounds__(B) void contingency_count_kernel(ContingencyCountArgs a) {
  __shared__ uint32_t cells[S];
  const int slice = blockIdx.x / a.groups, g = blockIdx.x - slice * a.groups;
  const int lo = slice * S;  // below kCtgMaxCells
  const int rest = static_cast<int>(a.r * a.c) - lo;
  const int live = rest < S ? rest : S;
  for (int i = threadIdx.x; i < live; i += B) cells[i] = 0u;
  __syncthreads();
  const int lane = lane_id();
  // samples before labels_true's first 16-byte boundary, whole units behind them, and the rest
  const int els = a.true_dt == DType::i64 ? 8 : 4;
  int64_t head = static_cast<int64_t>((16 - reinterpret_cast<uintptr_t>(a.labels_true) % 16) % 16) / els;
  head = head < a.n ? head : a.n;
  const int64_t units = (a.n - head) / kCtgUnit;
  const int64_t tail = a.n - head - units * kCtgUnit;
  int flags = 0;
  if (g == 0) {  // head and tail, one pair per thread: at most 2 (kCtgUnit - 1) < B of them
    int key = -1;
    const int64_t e = threadIdx.x;
    if (e < head + tail) {
      const int64_t i = e < head ? e : a.n - tail + (e - head);
      key = slice_key(load_label(a.labels_true, a.true_dt, i), load_label(a.labels_pred, a.pred_dt, i), a.r, a.c, lo,
                      live, flags);
    }
    fold(key, cells, lane);
  }
  // block-uniform trip count: every lane takes part in the wave's fold.  A step takes kAhead units
  // of a thread, one grid stride apart, and issues all their loads first.
  const int64_t stride = static_cast<int64_t>(a.groups) * B;
  for (int64_t u0 = static_cast<int64_t>(g) * B; u0 < units; u0 += kAhead * stride) {
    int64_t t[kAhead][kCtgUnit], p[kAhead][kCtgUnit];
#pragma unroll
    for (int h = 0; h < kAhead; ++h) {
      const int64_t u = u0 + h * stride + threadIdx.x;
      if (u < units) {
        load_labels(a.labels_true, a.true_dt, head + u * kCtgUnit, t[h]);
        load_labels(a.labels_pred, a.pred_dt, head + u * kCtgUnit, p[h]);
      }
    }
#pragma unroll
    for (int h = 0; h < kAhead; ++h) {
      const bool live_unit = u0 + h * stride + threadIdx.x < units;
#pragma unroll
      for (int j = 0; j < kCtgUnit; ++j) {
        const int key = live_unit ? slice_key(t[h][j], p[h][j], a.r, a.c, lo, live, flags) : -1;
        fold(key, cells, lane);
      }
    }
  }
  if (flags != 0 && a.err) atomicOr(a.err, flags);
  __syncthreads();
  unsigned long long* out = reinterpret_cast<unsigned long long*>(a.table) + lo;
  for (int i = threadIdx.x; i < live; i += B) {
    const uint32_t v = cells[i];
    if (v != 0u) atomicAdd(out + i, static_cast<unsigned long long>(v));
  }
}

// ---------------------------------------------------------------- statistics
// the block's FP64 total in wave order, to thread 0
__device__ __forceinline__ double block_ordered_sum(double v, double* lds) {
  v = wave_sum(v);
  if (lane_id() == 0) lds[threadIdx.x >> 6] = v;
  __syncthreads();
  double s = 0.0;
  if (threadIdx.x == 0) {
    for (int k = 0; k < kStatWaves; ++k) s += lds[k];
  }
  __syncthreads();
  return s;
}

__device__ __forceinline__ unsigned long long pairs_of(unsigned long long x) { return x * (x - 1) / 2; }

__global__ __launch_bounds__(kStatBlock) void contingency_cells_kernel(ContingencyStatsArgs a) {
  __shared__ double lds[kStatWaves];
  const int lane = lane_id();
  const int64_t segs = (a.c + kWave - 1) / kWave;
  const int64_t items = ((a.r + kRows - 1) / kRows) * segs;
  unsigned long long* marg = reinterpret_cast<unsigned long long*>(a.marginals);
  unsigned long long pairs = 0, total = 0;
  double nlogn = 0.0;
  const int64_t stride = static_cast<int64_t>(gridDim.x) * kStatWaves;
  for (int64_t item = static_cast<int64_t>(blockIdx.x) * kStatWaves + (threadIdx.x >> 6); item < items;
       item += stride) {
    const int64_t r0 = (item / segs) * kRows, col = (item % segs) * kWave + lane;
    const int64_t r1 = r0 + kRows < a.r ? r0 + kRows : a.r;
    unsigned long long colsum = 0;
    for (int64_t r = r0; r < r1; ++r) {
      const unsigned long long v = col < a.c ? static_cast<unsigned long long>(a.table[r * a.c + col]) : 0ull;
      colsum += v;
      if (v != 0) {
        pairs += pairs_of(v);
        nlogn += static_cast<double>(v) * log(static_cast<double>(v));
      }
      const unsigned long long rowsum = wave_sum(v);
      if (lane == 0 && rowsum != 0) {
        atomicAdd(marg + r, rowsum);
        total += rowsum;
      }
    }
    if (colsum != 0) atomicAdd(marg + a.r + col, colsum);
  }
  pairs = wave_sum(pairs);
  if (lane == 0) {
    if (pairs != 0) atomicAdd(a.ints + 0, pairs);
    if (total != 0) atomicAdd(a.ints + 3, total);
  }
  const double s = block_ordered_sum(nlogn, lds);
  if (threadIdx.x == 0) a.cell_partials[blockIdx.x] = s;
}

__global__ __launch_bounds__(kStatBlock) void contingency_margins_kernel(ContingencyStatsArgs a) {
  __shared__ double lds[kStatWaves];
  const int64_t m = a.r + a.c;
  const unsigned long long N = a.ints[3];  // finished by the cell pass
  unsigned long long pairs[2] = {0, 0}, present[2] = {0, 0};
  double xlogx[2] = {0.0, 0.0};
  for (int64_t i = static_cast<int64_t>(blockIdx.x) * kStatBlock + threadIdx.x; i < m;
       i += static_cast<int64_t>(gridDim.x) * kStatBlock) {
    const unsigned long long x = static_cast<unsigned long long>(a.marginals[i]);
    const int side = i < a.r ? 0 : 1;
    const double dx = static_cast<double>(x);
    double lx = 0.0;
    if (x != 0) {
      lx = log(dx);
      pairs[side] += pairs_of(x);
      present[side] += 1;
      xlogx[side] += dx * lx;
    }
    a.margin_logs[i] = lx;
    a.margin_logs[m + i] = lgamma(dx + 1.0) + lgamma(static_cast<double>(N - x) + 1.0);
  }
#pragma unroll
  for (int side = 0; side < 2; ++side) {
    const unsigned long long p = wave_sum(pairs[side]), q = wave_sum(present[side]);
    if (lane_id() == 0) {
      if (p != 0) atomicAdd(a.ints + 1 + side, p);
      if (q != 0) atomicAdd(a.ints + 4 + side, q);
    }
    const double s = block_ordered_sum(xlogx[side], lds);
    if (threadIdx.x == 0) a.margin_partials[static_cast<int64_t>(side) * gridDim.x + blockIdx.x] = s;
  }
}

// ---------------------------------------------------------------- expected mutual information
struct EmiPair {
  double a, b, N, g;  // g: every lgamma of log p that does not depend on n
  __device__ __forceinline__ double logp(double n) const {
    return g - lgamma(n + 1.0) - lgamma(a - n + 1.0) - lgamma(b - n + 1.0) - lgamma(N - a - b + n + 1.0);
  }
  // p(n + 1) / p(n) = num / den
  __device__ __forceinline__ double num(double n) const { return (a - n) * (b - n); }
  __device__ __forceinline__ double den(double n) const { return (n + 1.0) * (N - a - b + n + 1.0); }
};

__global__ __launch_bounds__(kStatBlock) void contingency_emi_kernel(ContingencyEmiArgs a, int parts) {
  __shared__ double lds[kStatWaves];
  const int lane = lane_id();
  const int64_t m = a.r + a.c;
  const unsigned long long N = a.ints[3];
  const double dN = static_cast<double>(N);
  const double logN = N != 0 ? log(dN) : 0.0, lgN1 = lgamma(dN + 1.0);
  const int64_t items = a.r * a.c * parts;
  double sum = 0.0, mag = 0.0;
  const int64_t stride = static_cast<int64_t>(gridDim.x) * kStatWaves;
  for (int64_t item = static_cast<int64_t>(blockIdx.x) * kStatWaves + (threadIdx.x >> 6); item < items;
       item += stride) {
    const int64_t pair = item / parts, part = item - pair * parts;
    const int64_t i = pair / a.c, j = a.r + pair % a.c;
    const long long ai = a.marginals[i], bj = a.marginals[j];
    if (ai == 0 || bj == 0) continue;  // wave-uniform
    const long long over = ai + bj - static_cast<long long>(N);
    const long long nlo = over > 1 ? over : 1, nhi = ai < bj ? ai : bj;
    const long long len = nhi - nlo + 1;
    const long long ps = nlo + part * len / parts, pe = nlo + (part + 1) * len / parts;  // len < 2^32, parts <= 64
    const long long chunk = (pe - ps + kWave - 1) / kWave;
    const long long s = ps + lane * chunk;
    const long long e = s + chunk < pe ? s + chunk : pe;
    if (s >= e) continue;
    EmiPair q;
    q.a = static_cast<double>(ai), q.b = static_cast<double>(bj), q.N = dN;
    q.g = (a.margin_logs[m + i] + a.margin_logs[m + j]) - lgN1;
    const double k = logN - a.margin_logs[i] - a.margin_logs[j];  // log(N / (a b))
    double n = static_cast<double>(s);
    const double last = static_cast<double>(e - 1);
    double lp = q.logp(n);
    if (lp < kLogFloor) {
      if (q.num(n) <= q.den(n)) continue;  // falling: everything behind is smaller still
      if (q.num(last) > q.den(last) && q.logp(last) < kLogFloor) continue;  // rising to the end, and below the floor there
      while (n < last && lp < kLogFloor) {  // an approximate walk to where p is representable
        lp += log(q.num(n) / q.den(n));
        n += 1.0;
      }
      lp = q.logp(n);
    }
    double p = exp(lp);
    for (;;) {
      const double term = n / dN * (log(n) + k) * p;
      sum += term;
      mag += fabs(term);
      if (n >= last) break;
      const double up = q.num(n), down = q.den(n);
      if (p < kTiny && up < down) break;  // falling and negligible
      p *= up / down;
      n += 1.0;
    }
  }
  const double s0 = block_ordered_sum(sum, lds);
  const double s1 = block_ordered_sum(mag, lds);
  if (threadIdx.x == 0) {
    a.partials[blockIdx.x] = s0;
    a.partials[gridDim.x + blockIdx.x] = s1;
  }
}

// ---------------------------------------------------------------- values
// hi 2^64 + lo of an exact 128-bit magnitude: three roundings at most
__device__ __forceinline__ double u128_to_f64(unsigned __int128 x) {
  return static_cast<double>(static_cast<unsigned long long>(x >> 64)) * 18446744073709551616.0 +
         static_cast<double>(static_cast<unsigned long long>(x));
}

__global__ __launch_bounds__(kWave) void contingency_values_kernel(ContingencyValuesArgs a) {
  const int lane = threadIdx.x;
  const double s_cell = wave_strided_sum(a.cell_partials, a.stats_blocks);
  const double s_a = wave_strided_sum(a.margin_partials, a.margin_blocks);
  const double s_b = wave_strided_sum(a.margin_partials + a.margin_blocks, a.margin_blocks);
  const double nan = __longlong_as_double(0x7ff8000000000000ll);
  const double emi = a.emi_partials ? wave_strided_sum(a.emi_partials, a.emi_blocks) : nan;
  if (lane != 0) return;
  double* v = a.values;
  const unsigned long long P = a.ints[0], Pa = a.ints[1], Pb = a.ints[2], N = a.ints[3];
  const unsigned long long rows = a.ints[4], cols = a.ints[5];
  if (N == 0) {
    for (int i = 0; i < kCtgValues; ++i) v[i] = nan;
    return;
  }
  // sklearn's pair confusion matrix, exact: all four are at most N (N - 1) < 2^64
  const unsigned long long T = N * (N - 1), tp = 2 * P, fp = 2 * (Pb - P), fn = 2 * (Pa - P);
  const unsigned long long tn = T - tp - fp - fn;
  v[0] = (tn + tp == T || T == 0) ? 1.0 : static_cast<double>(tn + tp) / static_cast<double>(T);
  if (fn == 0 && fp == 0) {
    v[1] = 1.0;
  } else {
    typedef unsigned __int128 u128;
    const u128 agree = static_cast<u128>(tp) * tn, cross = static_cast<u128>(fn) * fp;
    const double top = agree >= cross ? u128_to_f64(agree - cross) : -u128_to_f64(cross - agree);
    // (tp + fn)(fn + tn) + (tp + fp)(fp + tn) <= T^2 < 2^128
    const u128 bottom = static_cast<u128>(tp + fn) * (fn + tn) + static_cast<u128>(tp + fp) * (fp + tn);
    v[1] = 2.0 * top / u128_to_f64(bottom);
  }
  const double dP = static_cast<double>(P);
  v[2] = P != 0 ? sqrt(dP / static_cast<double>(Pb)) * sqrt(dP / static_cast<double>(Pa)) : 0.0;
  const double dN = static_cast<double>(N), logN = log(dN);
  const double hu = rows <= 1 ? 0.0 : logN - s_a / dN, hv = cols <= 1 ? 0.0 : logN - s_b / dN;
  double mi = 0.0;
  if (rows > 1 && cols > 1) {
    mi = ((s_cell - s_a) - s_b) / dN + logN;
    mi = mi > 0.0 ? mi : 0.0;
  }
  v[3] = hu, v[4] = hv, v[5] = mi, v[6] = emi;
  const double norm[4] = {fmin(hu, hv), sqrt(hu * hv), 0.5 * (hu + hv), fmax(hu, hv)};
  const double eps = 2.220446049250313e-16;
  for (int k = 0; k < 4; ++k) {
    v[7 + k] = norm[k];
    double nmi, ami;
    if (rows == 1 && cols == 1) {
      nmi = ami = 1.0;
    } else {
      nmi = fabs(mi) <= 1e-15 ? 0.0 : mi / norm[k];
      if (rows == 1 || cols == 1) {
        ami = 0.0;
      } else {
        double bottom = norm[k] - emi, top = mi - emi;
        bottom = bottom < 0.0 ? fmin(bottom, -eps) : fmax(bottom, eps);
        top = top < 0.0 ? fmin(top, -eps) : fmax(top, eps);
        ami = emi != emi ? nan : top / bottom;
      }
    }
    v[11 + k] = nmi;
    v[15 + k] = ami;
  }
  v[19] = hu != 0.0 ? mi / hu : 1.0;
  v[20] = hv != 0.0 ? mi / hv : 1.0;
}

bool label_dtype(DType d) { return d == DType::i64 || d == DType::i32; }

int64_t clamp_blocks(int64_t want, int64_t cap) { return want < 1 ? 1 : (want > cap ? cap : want); }

}  // namespace

int contingency_stats_blocks(int64_t r, int64_t c) {
  const int64_t items = ((r + kRows - 1) / kRows) * ((c + kWave - 1) / kWave);
  return static_cast<int>(clamp_blocks((items + kStatWaves - 1) / kStatWaves, kCtgStatsBlocks));
}

int contingency_margin_blocks(int64_t r, int64_t c) {
  return static_cast<int>(clamp_blocks((r + c + kStatBlock - 1) / kStatBlock, kCtgMarginBlocks));
}

int contingency_emi_parts(int64_t r, int64_t c) {
  return static_cast<int>(clamp_blocks((kEmiTargetItems + r * c - 1) / (r * c), kCtgEmiMaxParts));
}

int contingency_emi_blocks(int64_t r, int64_t c) {
  const int64_t items = r * c * contingency_emi_parts(r, c);
  return static_cast<int>(clamp_blocks((items + kStatWaves - 1) / kStatWaves, kCtgEmiBlocks));
}

int launch_contingency_count(const ContingencyCountArgs& a, hipStream_t stream) {
  if (a.n < 0 || a.n >= (int64_t{1} << 31) || a.r < 1 || a.c < 1 || a.r > kCtgMaxCells || a.c > kCtgMaxCells) return -1;
  if (a.r * a.c > kCtgMaxCells || !label_dtype(a.true_dt) || !label_dtype(a.pred_dt)) return -1;
  if (a.slice != kCtgSliceSmall && a.slice != kCtgSliceLarge) return -1;
  const int64_t slices = (a.r * a.c + a.slice - 1) / a.slice;
  if (a.groups < 1 || slices * a.groups > kCtgMaxBlocks) return -1;
  if (a.n == 0) return 0;
  if (a.labels_true == nullptr || a.labels_pred == nullptr || a.table == nullptr) return -1;
  const uintptr_t t = reinterpret_cast<uintptr_t>(a.labels_true), p = reinterpret_cast<uintptr_t>(a.labels_pred);
  if (t % dtype_bytes(a.true_dt) != 0 || p % dtype_bytes(a.pred_dt) != 0) return -2;  // element-aligned
  const dim3 grid(static_cast<unsigned>(slices * a.groups));
  if (a.slice == kCtgSliceSmall) {
    hipLaunchKernelGGL((contingency_count_kernel<kCtgSliceSmall, kCtgBlockSmall>), grid, dim3(kCtgBlockSmall), 0,
                       stream, a);
  } else {
    hipLaunchKernelGGL((contingency_count_kernel<kCtgSliceLarge, kCtgBlockLarge>), grid, dim3(kCtgBlockLarge), 0,
                       stream, a);
  }
  return static_cast<int>(hipGetLastError());
}

int launch_contingency_stats(const ContingencyStatsArgs& a, hipStream_t stream) {
  if (a.r < 1 || a.c < 1 || a.r > kCtgMaxCells || a.c > kCtgMaxCells || a.r * a.c > kCtgMaxCells) return -1;
  if (a.table == nullptr || a.marginals == nullptr || a.ints == nullptr || a.cell_partials == nullptr ||
      a.margin_partials == nullptr || a.margin_logs == nullptr)
    return -1;
  hipLaunchKernelGGL(contingency_cells_kernel, dim3(contingency_stats_blocks(a.r, a.c)), dim3(kStatBlock), 0, stream,
                     a);
  hipLaunchKernelGGL(contingency_margins_kernel, dim3(contingency_margin_blocks(a.r, a.c)), dim3(kStatBlock), 0,
                     stream, a);
  return static_cast<int>(hipGetLastError());
}

int launch_contingency_emi(const ContingencyEmiArgs& a, hipStream_t stream) {
  if (a.r < 1 || a.c < 1 || a.r > kCtgMaxCells || a.c > kCtgMaxCells || a.r * a.c > kCtgMaxCells) return -1;
  if (a.marginals == nullptr || a.ints == nullptr || a.margin_logs == nullptr || a.partials == nullptr) return -1;
  hipLaunchKernelGGL(contingency_emi_kernel, dim3(contingency_emi_blocks(a.r, a.c)), dim3(kStatBlock), 0, stream, a,
                     contingency_emi_parts(a.r, a.c));
  return static_cast<int>(hipGetLastError());
}

int launch_contingency_values(const ContingencyValuesArgs& a, hipStream_t stream) {
  if (a.ints == nullptr || a.cell_partials == nullptr || a.margin_partials == nullptr || a.values == nullptr) return -1;
  if (a.stats_blocks < 1 || a.margin_blocks < 1 || (a.emi_partials != nullptr && a.emi_blocks < 1)) return -1;
  hipLaunchKernelGGL(contingency_values_kernel, dim3(1), dim3(kWave), 0, stream, a);
  return static_cast<int>(hipGetLastError());
}

}  // namespace tea
