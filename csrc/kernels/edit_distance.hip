// K29: unit-cost Levenshtein distance of padded token-id rows, docs/parity.md "Not in the reference".
//
// Replaces the ATen form (functional/text/token_edit_distance.py: one batched row recurrence per stream
// position) and the host route of the string metrics (tea_text::levenshtein, one CPU thread per pair).
//
// Systolic strip walk, the body of both arms.  Rows i = 1..n run over one sequence (the stream), columns
// j = 1..m over the other (stationary), in strips of 64 columns.  In strip s lane l owns column
// j = 64 s + l + 1 and keeps its token in registers.  At step k = 0 .. n + 62 lane l computes the cell of
// row i = k - l + 1 when 1 <= i <= n and j <= m:
//  * `up` is its own value of the previous step (initially j = D[0][j]);
//  * `left` is lane l-1's value of the previous step, one DPP wave_shr:1;
//  * `diag` is the `left` it received one step earlier, so it costs no second shift;
//  * the stream token reaches lane l the same way, one (int32) or two (int64) more DPP moves.
// Lane 0 has no source lane and keeps the DPP's `old` operand, through which it is fed wave-uniform
// values by v_readlane of two 64-entry register chunks: the next stream token (loaded coalesced from
// global memory once per 64 steps, a chunk ahead) and the strip's left edge D[i][64 s].  The edge column
// lives in LDS, one 16-bit entry per row (entry i - 1 holds D[i][.]; distances are at most kEditMaxLen =
// 4096); lane 63 writes D[i][64 s + 64] into entry i - 1, 63 steps after lane 0 consumed its old value, so
// one array is updated in place.  The first strip's edge is D[i][0] = i and is never stored.  A cell is
// `diag` on equal tokens and min3(up, left, diag) + 1 otherwise; a lane outside its row range holds its
// value, which is what its right neighbour and the answer (lane (m - 1) & 63 after the last strip) need.
// Per pair, wave-uniformly, the sequence that gives fewer 64-step macro steps goes into the lanes.
//  * edit_distance_wave_kernel: one wave per pair, kEditPairsPerWg pairs per workgroup, strips in
//    sequence; no barrier.
//  * edit_distance_block_kernel: one workgroup of kEditBlockWaves waves per pair.  Wave w takes strips
//    w, w + W, ...; all waves run in macro steps of 64 systolic steps that end in __syncthreads(), and
//    a strip starts two macro steps after its left neighbour: at the start of its macro step c it reads
//    entries 64 c .. 64 c + 63, and the neighbour wrote entries up to 64 c + 64 in its macro step
//    c + 1, one barrier earlier (a lag of one macro step would have reached entry 64 c only).  A strip
//    reads an entry before it writes it, and strip s + 1 reads it only after strip s wrote it, so the
//    single in-place array stays safe across waves: a round of W strips takes max(M, 2 W) macro steps
//    (M those of one strip), so the wave that wraps round to strip s + W - 1 writes an entry at least
//    2 W - 2 macro steps after strip s read it.  No spin-wait, no flag, no atomic.
//  * edit_distance_prep_kernel (only with ignore_index): a wave per row and side compacts the kept
//    tokens into the workspace by ballot and popcount prefix, 64 at a time, and writes the kept lengths
//    (tea_token_rows.h, shared with K30).
//  * edit_distance_finish_kernel (only with totals): one wave adds the distances and lengths as 64-bit
//    integers and adds the four sums to the float64 totals; everything is an integer below 2^53.
// Every store of a result is non-atomic: bit-identical from run to run.  Pairs per workgroup, waves of
// the block arm and the prefetch depth (one chunk) are untuned.
#include "tea_common.h"
#include "tea_kernels.h"
#include "tea_token_rows.h"

namespace tea {

namespace {

constexpr int kShr1 = 0x138;  // DPP control wave_shr:1
constexpr int kPrepWaves = kTokenPrepWaves;

// lane l takes `v` of lane l - 1; lane 0 takes `lane0`
__device__ __forceinline__ uint32_t shr1(uint32_t lane0, uint32_t v) {
  return static_cast<uint32_t>(
      __builtin_amdgcn_update_dpp(static_cast<int>(lane0), static_cast<int>(v), kShr1, 0xf, 0xf, false));
}
__device__ __forceinline__ uint32_t lane_of(uint32_t v, int l) {
  return static_cast<uint32_t>(__builtin_amdgcn_readlane(static_cast<int>(v), l));
}

// token `idx` of a row as (lo, hi) words; zero at and past `n`
template <bool Wide>
__device__ __forceinline__ void load_tok(const void* row, int idx, int n, uint32_t& lo, uint32_t& hi) {
  lo = 0;
  hi = 0;
  if (idx < n) {
    if constexpr (Wide) {
      const unsigned long long v = static_cast<const unsigned long long*>(row)[idx];
      lo = static_cast<uint32_t>(v);
      hi = static_cast<uint32_t>(v >> 32);
    } else {
      lo = static_cast<const uint32_t*>(row)[idx];
    }
  }
}

__device__ __forceinline__ int strips_of(int m) { return (m + 63) >> 6; }
__device__ __forceinline__ int macros_of(int n) { return (n + 126) >> 6; }  // ceil((n + 63) / 64) steps k <= n + 62

// One pair as the walk sees it: `a` streams through the lanes, `b` is stationary in them.
struct Pair {
  const void* a;
  const void* b;
  int n, m;
};

template <bool Wide>
__device__ __forceinline__ Pair pair_of(const EditDistanceArgs& g, int64_t pair) {
  constexpr int64_t kTok = Wide ? 8 : 4;
  const char* in = static_cast<const char*>(g.has_ignore ? g.ws_tokens : g.input);
  const char* tg = g.has_ignore ? in + g.b * g.li * kTok : static_cast<const char*>(g.target);
  const int64_t* il = g.has_ignore ? g.ws_lengths : g.input_lengths;
  const int64_t* tl = g.has_ignore ? g.ws_lengths + g.b : g.target_lengths;
  const int ni = row_len(il, pair, g.li), nt = row_len(tl, pair, g.lt);
  in += pair * g.li * kTok;
  tg += pair * g.lt * kTok;
  // the distance is symmetric: stream the side that gives fewer macro steps
  if (strips_of(nt) * macros_of(ni) <= strips_of(ni) * macros_of(nt)) return Pair{in, tg, ni, nt};
  return Pair{tg, in, nt, ni};
}

// entries of one pair's edge column in LDS
__host__ __device__ inline int edge_entries(int64_t li, int64_t lt) {
  const int64_t w = li > lt ? li : lt;
  return static_cast<int>(w < 64 ? 64 : (w + 63) / 64 * 64);
}

template <bool Wide>
struct Strip {
  Pair p;
  uint16_t* edge;  // p.n entries at least
  int lane;
  int s;           // the strip
  uint32_t b_lo, b_hi;        // this lane's stationary token
  uint32_t val, diag;         // D[i][j] of the last step; the `left` of the last step
  uint32_t t_lo, t_hi;        // the stream token that passes through this lane
  uint32_t rows;              // p.n in a lane whose column exists, else 0
  int kl;                     // k - lane = i - 1 of the next step
  uint32_t next_lo, next_hi;  // the prefetched stream chunk

  __device__ __forceinline__ void begin(int strip) {
    s = strip;
    const int j = 64 * s + lane + 1;
    load_tok<Wide>(p.b, j - 1, p.m, b_lo, b_hi);
    rows = j <= p.m ? static_cast<uint32_t>(p.n) : 0u;
    val = static_cast<uint32_t>(j);        // D[0][j]
    diag = static_cast<uint32_t>(64 * s);  // lane 0: D[0][64 s]; the others receive theirs before they start
    t_lo = 0;
    t_hi = 0;
    kl = -lane;
    load_tok<Wide>(p.a, lane, p.n, next_lo, next_hi);
  }

  // steps 64 c .. 64 c + 63
  __device__ __forceinline__ void macro(int c) {
    const uint32_t cur_lo = next_lo, cur_hi = next_hi;
    load_tok<Wide>(p.a, 64 * (c + 1) + lane, p.n, next_lo, next_hi);
    const int e = 64 * c + lane;  // lane t: the entry lane 0 consumes at step 64 c + t
    uint32_t ecol = static_cast<uint32_t>(e + 1);
    if (s != 0) ecol = e < p.n ? edge[e] : 0u;
#pragma unroll
    for (int t = 0; t < 64; ++t) {
      const uint32_t left = shr1(lane_of(ecol, t), val);
      t_lo = shr1(lane_of(cur_lo, t), t_lo);
      bool eq = t_lo == b_lo;
      if constexpr (Wide) {
        t_hi = shr1(lane_of(cur_hi, t), t_hi);
        eq = eq && t_hi == b_hi;
      }
      const bool act = static_cast<uint32_t>(kl) < rows;
      const uint32_t best = min(min(val, left), diag) + 1u;
      val = act ? (eq ? diag : best) : val;
      diag = left;
      if (lane == 63 && act) edge[kl] = static_cast<uint16_t>(val);
      ++kl;
    }
  }

  __device__ __forceinline__ int64_t answer() const {
    return static_cast<int64_t>(lane_of(val, (p.m - 1) & 63));
  }
};

template <bool Wide>
__global__ __launch_bounds__(kEditPairsPerWg* kWave) void edit_distance_wave_kernel(EditDistanceArgs g) {
  extern __shared__ uint16_t s_edge[];
  const int w = wave_id();
  const int64_t pair = static_cast<int64_t>(blockIdx.x) * kEditPairsPerWg + w;
  if (pair >= g.b) return;
  Strip<Wide> st;
  st.p = pair_of<Wide>(g, pair);
  st.lane = lane_id();
  st.edge = s_edge + w * edge_entries(g.li, g.lt);
  if (st.p.n == 0 || st.p.m == 0) {
    if (st.lane == 0) g.out[pair] = st.p.n + st.p.m;
    return;
  }
  const int S = strips_of(st.p.m), M = macros_of(st.p.n);
  for (int s = 0; s < S; ++s) {
    st.begin(s);
    for (int c = 0; c < M; ++c) st.macro(c);
  }
  const int64_t d = st.answer();
  if (st.lane == 0) g.out[pair] = d;
}

template <bool Wide>
__global__ __launch_bounds__(kEditBlockWaves* kWave) void edit_distance_block_kernel(EditDistanceArgs g) {
  extern __shared__ uint16_t s_edge[];
  constexpr int W = kEditBlockWaves;
  const int w = wave_id();
  const int64_t pair = blockIdx.x;
  Strip<Wide> st;
  st.p = pair_of<Wide>(g, pair);
  st.lane = lane_id();
  st.edge = s_edge;
  if (st.p.n == 0 || st.p.m == 0) {  // block-uniform
    if (threadIdx.x == 0) g.out[pair] = st.p.n + st.p.m;
    return;
  }
  const int S = strips_of(st.p.m), M = macros_of(st.p.n);
  const int P = M > 2 * W ? M : 2 * W;  // macro steps of a round of W strips
  const int R = (S + W - 1) / W;
  const int G = (R - 1) * P + 2 * (W - 1) + M;
  int s = w, c = -2 * w;  // this wave's strip and its macro step
  for (int gstep = 0; gstep < G; ++gstep) {
    if (c >= 0 && c < M && s < S) {
      if (c == 0) st.begin(s);
      st.macro(c);
      if (c == M - 1 && s == S - 1) {
        const int64_t d = st.answer();
        if (st.lane == 0) g.out[pair] = d;
      }
    }
    if (++c == P) {
      c = 0;
      s += W;
    }
    __syncthreads();
  }
}

template <typename T>
__global__ __launch_bounds__(kPrepWaves* kWave) void edit_distance_prep_kernel(EditDistanceArgs g) {
  compact_token_rows<T>(g.input, g.target, g.input_lengths, g.target_lengths, g.b, g.li, g.lt, g.ignore_index,
                        g.ws_tokens, g.ws_lengths);
}

__global__ __launch_bounds__(kWave) void edit_distance_finish_kernel(EditDistanceArgs g) {
  const int64_t* il = g.has_ignore ? g.ws_lengths : g.input_lengths;
  const int64_t* tl = g.has_ignore ? g.ws_lengths + g.b : g.target_lengths;
  long long sum[4] = {0, 0, 0, 0};
  for (int64_t i = threadIdx.x; i < g.b; i += kWave) {
    const int n = clamped_len(il, i, g.li), m = clamped_len(tl, i, g.lt);
    sum[0] += g.out[i];
    sum[1] += n;
    sum[2] += m;
    sum[3] += n > m ? n : m;
  }
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    const long long s = wave_sum(sum[j]);
    if (threadIdx.x == 0) *g.totals[j] = (g.accumulate ? *g.totals[j] : 0.0) + static_cast<double>(s);
  }
}

}  // namespace

bool edit_distance_geometry_ok(int64_t b, int64_t li, int64_t lt) {
  return b >= 1 && b < (int64_t{1} << 30) && li >= 0 && li <= kEditMaxLen && lt >= 0 && lt <= kEditMaxLen;
}

int launch_edit_distance(const EditDistanceArgs& a, hipStream_t stream) {
  if (!edit_distance_geometry_ok(a.b, a.li, a.lt) || a.out == nullptr) return -1;
  if ((a.li > 0 && a.input == nullptr) || (a.lt > 0 && a.target == nullptr)) return -1;
  if (a.arm != kEditArmWave && a.arm != kEditArmBlock) return -1;
  if (a.has_ignore && (a.ws_lengths == nullptr || (a.li + a.lt > 0 && a.ws_tokens == nullptr))) return -1;
  const bool totals = a.totals[0] != nullptr;
  for (int j = 0; j < 4; ++j)
    if ((a.totals[j] != nullptr) != totals) return -1;
  if (a.has_ignore) {
    const dim3 grid(static_cast<unsigned>((2 * a.b + kPrepWaves - 1) / kPrepWaves)), block(kPrepWaves * kWave);
    if (a.wide) hipLaunchKernelGGL(edit_distance_prep_kernel<long long>, grid, block, 0, stream, a);
    else hipLaunchKernelGGL(edit_distance_prep_kernel<int>, grid, block, 0, stream, a);
  }
  const size_t edge = static_cast<size_t>(edge_entries(a.li, a.lt)) * sizeof(uint16_t);
  if (a.arm == kEditArmWave) {
    const dim3 grid(static_cast<unsigned>((a.b + kEditPairsPerWg - 1) / kEditPairsPerWg)), block(kEditPairsPerWg * kWave);
    if (a.wide) hipLaunchKernelGGL(edit_distance_wave_kernel<true>, grid, block, kEditPairsPerWg * edge, stream, a);
    else hipLaunchKernelGGL(edit_distance_wave_kernel<false>, grid, block, kEditPairsPerWg * edge, stream, a);
  } else {
    const dim3 grid(static_cast<unsigned>(a.b)), block(kEditBlockWaves * kWave);
    if (a.wide) hipLaunchKernelGGL(edit_distance_block_kernel<true>, grid, block, edge, stream, a);
    else hipLaunchKernelGGL(edit_distance_block_kernel<false>, grid, block, edge, stream, a);
  }
  if (totals) hipLaunchKernelGGL(edit_distance_finish_kernel, dim3(1), dim3(kWave), 0, stream, a);
  return static_cast<int>(hipGetLastError());
}

}  // namespace tea
