// K23: silhouette coefficient (docs/parity.md, "Not in the reference").
//
//   d(i, j) = sqrt(max(0, (|x_i|^2 + |x_j|^2) - 2 <x_i, x_j>))      (combined in FP64, NaN kept)
//   a(i) = mean of d(i, j) over the other members of i's cluster (0 for a singleton)
//   b(i) = the smallest mean of d(i, j) over another non-empty cluster
//   s(i) = (b - a) / max(a, b), 0 for a singleton or a = b = 0, NaN where a or b is NaN
// The ATen form writes [chunk, N] distance blocks and segment-sums them.  Here an inner product
// never leaves its block, a distance never leaves a register and a per-cluster sum reaches memory
// only at the two ends of a block's walk.
//
// The wrapper (ops/silhouette.py) sorts the samples by cluster and pads every non-empty cluster to
// whole 128-row panels: ref_index[panel row] is a sample or -1, panel_cluster[panel] the panel's one
// cluster, num_panels[0] = T the panels in use (a device value; sizes use the host bound
// max_panels = ceil(N / 128) + K).
//
// silhouette_norms_kernel<kVec>: K22's norms for one set (a wave per row, one order in both load
// arms); a sum that is not finite is stored as NaN, so that a row with a NaN or an inf feature has
// the distance NaN to every other row, whatever the signs in the inner product.
//
// silhouette_tile_kernel<kVec>, gfx950 mapping (the tile itself is tea_gramtile.h's):
//  * K22's prdc_tile_kernel with the roles swapped.  The query samples are the tile's columns, in
//    their original order and addressed directly: block (q, g) owns column tile q.  The tile's rows
//    (the accumulator registers) are the panel's reference samples, fetched through ref_index; a -1
//    stages zeros (the nullptr row of gramtile::Stage).  The block walks the panels
//    [g T / G, (g + 1) T / G) in order (G = SilhouetteArgs::groups, rule at silhouette_groups).
//  * main loop: K22's, unchanged: 32-wide stages, a float32 MFMA chain per 128 k whose sums are
//    added in k order (largest error 3e-7 of sum |a_k| |b_k|; K20's single chain was not tried here,
//    the bounds of the tests are K22's), the next stage's loads in flight behind the MFMAs and the
//    next panel's first loads (and its rows' norms and indices) issued ahead of the epilogue.
//  * epilogue: the registers pass through the wave's own 8 KB of the free staging image, as in K22,
//    so the steps are a loop over a register number.  A lane holds two columns and, per column, 32
//    of the wave's 64 rows: it widens each element, forms d2 with the row's norm (LDS, written per
//    panel) and its columns' norms (two loads per lane and panel, cache hits), clamps with
//    `d2 < 0 ? 0 : d2` (a NaN stays), takes the FP64 square root, makes it exactly 0 for a padding
//    row and for the row whose sample is the column's (the positional self pair) and adds it to the
//    column's FP64 sum: 64 adds per lane and tile in one fixed order, no cross-lane step per
//    register.  One shfl_xor 32 joins the half-waves; lane l of a wave then stands for column l of
//    the wave's 64.
//  * departure from the issue's sketch: the two waves that share the columns exchange their sums
//    through 4 x 64 x 8 B of LDS after every panel, not only when the walk leaves a cluster.  The
//    tile's end barrier orders the exchange either way (no barrier is added), the cost is one LDS
//    store and two loads per lane and tile, and there is no block-uniform branch around an
//    exchange.  Both waves then keep the same running state and the row-half 0 waves store it.
//  * a panel is one cluster, so a lane keeps one running sum (in LDS, like the rest of the
//    column's state: each lane reads back only what it wrote).  When the walk leaves a cluster that
//    is not the range's first, the sum is divided by the cluster's count and lowered into the
//    lane's minimum, or kept raw if it is the column's own cluster.  The first and the last cluster
//    of the range may go on in a neighbouring range, so their raw sums leave as they are:
//    edges[g][0 .. 4)[column] = first sum, last sum (0 if the range holds one cluster), inside
//    minimum (NaN if none), inside own sum (0 if none).  Plain stores, one writer per address.
//  * the minimum ignores a NaN while a number is there (minimum_of below): a cluster that holds a
//    non-finite row cannot be any sample's nearest, and b is NaN only where every candidate is.
// silhouette_stitch_kernel: a thread per sample walks g = 0 .. G - 1, joins edge sums of one cluster
// across neighbouring ranges, divides, completes a and b, forms s in FP64 and writes a, b, s and the
// float32 sample value; block_sum adds the block's s (0 for a sample with a bad label, whose
// outputs are NaN) into one FP64 partial.
// silhouette_finish_kernel: one wave adds the partials in block order (wave_strided_sum) and the
// counts, and lane 0 writes the mean over the labelled samples, NaN when fewer than two clusters
// have a member.
// No atomics (the wrapper raises the bad-label flag with ATen), no host sync, no cross-block
// waiting: results are bit-identical from run to run.
//
// Resources (the compiler's resource report, -Rpass-analysis=kernel-resource-usage, gfx950):
//   silhouette_tile_kernel<true> (16-byte loads) and <false> (element loads): 256 VGPRs, 0 AGPRs,
//   46080 B of LDS, two blocks per CU, no spills (0 VGPR, 0 SGPR) in either.  With the four
//   doubles of a column's state, its cluster and its norms in registers the report showed 10 and 12
//   spilled VGPRs, which is why they live in LDS or are loaded again per panel.
//   norms 18, stitch 32, finish 22 VGPRs; no spills.
// Group rule (silhouette_groups; K22's model with kSilEpilogueStages added per tile, a model until
// measured, nothing of it fitted to this kernel) and the padding factor T 128 / N with clusters of
// about equal size, at the benchmark shapes (N x D, K):
//   10000 x 64, K = 10:     79 column tiles, 89 panels at most, G = 6  (474 blocks), padding 1.02
//   50000 x 128, K = 100:   391 column tiles, 491 at most,      G = 13 (5083 blocks), padding 1.02
//   10000 x 2048, K = 10:   79 column tiles, 89 at most,        G = 6  (474 blocks), padding 1.02
//   50000 x 16, K = 1000:   391 column tiles, 1391 at most,     G = 13 (5083 blocks), padding 2.56
// The last shape is the padding-waste case, accepted here: every cluster of about 50 samples fills a
// 128-row panel.
// Not tried: a 64-row padding unit or unpadded segments, symmetric tiles (d(i, j) = d(j, i)), a
// float32 square root refined to FP64, K20's single MFMA chain, other values of G on the device.
#include <algorithm>

#include "tea_common.h"
#include "tea_gramtile.h"
#include "tea_kernels.h"
#include "tea_partials.h"

namespace tea {

namespace {

using namespace gramtile;

constexpr int kChunk = 128;  // k per MFMA chain: four stages, then the chain's sum joins the accumulator
constexpr int kWaves = kThreads / kWave;
static_assert(kSilTile == kT, "the tile is tea_gramtile.h's");
static_assert(2 * 32 * kWave <= kImage, "two waves' epilogue halves fit one operand's staging image");

__device__ __forceinline__ double nan64() { return __builtin_nan(""); }

// the smaller of two means; a NaN loses to a number, two NaNs stay NaN
__device__ __forceinline__ double minimum_of(double b, double m) { return (m < b || b != b) ? m : b; }

template <bool kVec>
__global__ __launch_bounds__(kThreads) void silhouette_norms_kernel(SilhouetteArgs a) {
  const int64_t row = static_cast<int64_t>(blockIdx.x) * kWaves + (threadIdx.x >> 6);
  if (row >= a.n) return;  // whole wave
  const float* p = a.x + row * a.stride;
  const int64_t d = a.d;
  double s = 0.0;
  for (int64_t c = 4 * lane_id(); c < d; c += 4 * kWave) {
    float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
    if constexpr (kVec) {
      v = *reinterpret_cast<const float4*>(p + c);  // d % 4 == 0: wholly inside
    } else {
      v.x = p[c];
      if (c + 1 < d) v.y = p[c + 1];
      if (c + 2 < d) v.z = p[c + 2];
      if (c + 3 < d) v.w = p[c + 3];
    }
    s += static_cast<double>(v.x) * static_cast<double>(v.x);
    s += static_cast<double>(v.y) * static_cast<double>(v.y);
    s += static_cast<double>(v.z) * static_cast<double>(v.z);
    s += static_cast<double>(v.w) * static_cast<double>(v.w);
  }
  s = wave_sum(s);
  if (lane_id() == 0) a.norms[row] = s < __builtin_huge_val() ? s : nan64();  // inf and NaN: NaN
}

template <bool kVec>
__global__ __launch_bounds__(kThreads, 2) void silhouette_tile_kernel(SilhouetteArgs a) {
  const int G = a.groups;
  const int q = blockIdx.x / G;
  const int g = blockIdx.x % G;
  const int n = static_cast<int>(a.n);
  const int d = static_cast<int>(a.d);
  const int T = min(max(a.num_panels[0], 0), a.max_panels);
  const int t0 = static_cast<int>(static_cast<int64_t>(g) * T / G);
  const int t1 = static_cast<int>(static_cast<int64_t>(g + 1) * T / G);
  if (t0 >= t1) return;  // whole block: the stitch launch skips an empty range

  __shared__ __attribute__((aligned(16))) float sA[kImage];
  __shared__ __attribute__((aligned(16))) float sB[kImage];
  __shared__ double s_norm[kT];       // the panel's row norms
  __shared__ int s_idx[kT];           // the panel's samples, -1 for padding
  __shared__ double s_sum[kWaves * kWave];  // [wave][column of the wave]: the panel's column sums
  __shared__ double s_state[kWaves * 4 * kWave];  // [wave][value][column of the wave]
  __shared__ int s_own[kWaves * kWave];           // [wave][column of the wave]: the column's cluster

  const int lane = threadIdx.x & 63;
  const int w = threadIdx.x >> 6;
  const int wr = w >> 1, wc = w & 1;
  const int half = lane >> 5, j = lane & 31;

  // ---- staging: the thread's columns (fixed); its rows of a panel at first_stage
  Stage st;
  st.rslot = threadIdx.x >> 3;
  st.kq = threadIdx.x & 7;
  st.d = d;
#pragma unroll
  for (int p = 0; p < kPieces; ++p) {
    const int gj = q * kT + st.rslot + 32 * p;
    st.pb[p] = gj < n ? a.x + static_cast<int64_t>(gj) * a.stride : nullptr;
  }
  const int offA = operand_offset(lane, wr), offB = operand_offset(lane, wc);

  int pre_idx = -1;       // threads 0 .. 127: row threadIdx.x of the panel being loaded
  double pre_norm = 0.0;
  auto sample_of = [&](int slot) {  // a panel row's sample, -1 for padding (and for anything out of range)
    const int i = a.ref_index[slot];
    return i >= 0 && i < n ? i : -1;
  };
  auto first_stage = [&](int t) {  // the panel's rows, and its first stage into registers
#pragma unroll
    for (int p = 0; p < kPieces; ++p) {
      const int i = sample_of(t * kT + st.rslot + 32 * p);
      st.pa[p] = i >= 0 ? a.x + static_cast<int64_t>(i) * a.stride : nullptr;
    }
    if (threadIdx.x < kT) {
      pre_idx = sample_of(t * kT + static_cast<int>(threadIdx.x));
      pre_norm = pre_idx >= 0 ? a.norms[pre_idx] : 0.0;
    }
    st.load<kVec>(0);
  };

  // ---- the lane's columns: two in the epilogue, one (column `lane` of the wave's 64) afterwards.
  // The column's state lives in LDS, each lane reading back only what it wrote: the running sum of
  // the cluster being walked, the first cluster's sum, the inside minimum, the inside own sum and the column's own cluster.
  // In registers these (and the columns' norms) made the main loop spill.
  const int c0 = q * kT + wc * 64 + j, c1 = c0 + 32;
  const int col = q * kT + wc * 64 + lane;
  const int cf = a.panel_cluster[t0];  // the range's first cluster
  int cur = cf;                        // the cluster whose panels are being walked
  double* state = s_state + w * 4 * kWave + lane;
  state[0] = 0.0;
  state[kWave] = 0.0;
  state[2 * kWave] = nan64();
  state[3 * kWave] = 0.0;
  s_own[w * kWave + lane] = col < n ? a.labels[col] : -1;

  auto leave = [&]() {  // the walk leaves cluster `cur` for another one
    const double run = state[0];
    if (cur == cf) {
      state[kWave] = run;
    } else if (cur == s_own[w * kWave + lane]) {
      state[3 * kWave] = run;
    } else {
      const int cnt = cur >= 0 && cur < a.k ? a.counts[cur] : 1;
      state[2 * kWave] = minimum_of(state[2 * kWave], run / static_cast<double>(cnt));
    }
    state[0] = 0.0;
  };

  first_stage(t0);
  for (int t = t0; t < t1; ++t) {
    const int c = a.panel_cluster[t];
    if (threadIdx.x < kT) {  // the previous panel's epilogue ended at the tile's end barrier
      s_norm[threadIdx.x] = pre_norm;
      s_idx[threadIdx.x] = pre_idx;
    }
    f32x16 acc[2][2];  // the float32 sum, in k order, of the finished chunks' chains
    zero(acc);

    for (int kc = 0; kc < d; kc += kChunk) {
      f32x16 part[2][2];  // the MFMA chain of this chunk of k
      zero(part);
      const int kend = min(kc + kChunk, d);
      for (int k0 = kc; k0 < kend; k0 += kBK) {
        st.store(sA, sB);
        __syncthreads();
        if (k0 + kBK < d) st.load<kVec>(k0 + kBK);  // in flight behind this stage's MFMAs
        mfma_stage(sA, sB, offA, offB, part);
        __syncthreads();
      }
#pragma unroll
      for (int bm = 0; bm < 2; ++bm)
#pragma unroll
        for (int bn = 0; bn < 2; ++bn) acc[bm][bn] += part[bm][bn];
    }

    if (t + 1 < t1) first_stage(t + 1);  // the next panel's loads fly behind the epilogue

    // ---- epilogue: the tile leaves the registers through the wave's 8 KB of the staging image
    // (free after the main loop's last barrier); a lane reads back only what it wrote itself
    float* stage = (w < 2 ? sA : sB) + (w & 1) * (32 * kWave) + lane;
    const double nb0 = c0 < n ? a.norms[c0] : 0.0, nb1 = c1 < n ? a.norms[c1] : 0.0;
    double s0 = 0.0, s1 = 0.0;
#pragma unroll
    for (int bm = 0; bm < 2; ++bm) {
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        stage[(2 * r) * kWave] = acc[bm][0][r];
        stage[(2 * r + 1) * kWave] = acc[bm][1][r];
      }
#pragma unroll 1
      for (int r = 0; r < 16; ++r) {
        const int rl = wr * 64 + bm * 32 + cd_row(r, lane);  // row of the panel
        const double na = s_norm[rl];
        const int ri = s_idx[rl];
        double e0 = (na + nb0) - 2.0 * static_cast<double>(stage[(2 * r) * kWave]);
        double e1 = (na + nb1) - 2.0 * static_cast<double>(stage[(2 * r + 1) * kWave]);
        e0 = sqrt(e0 < 0.0 ? 0.0 : e0);  // a NaN stays
        e1 = sqrt(e1 < 0.0 ? 0.0 : e1);
        s0 += ri < 0 || ri == c0 ? 0.0 : e0;
        s1 += ri < 0 || ri == c1 ? 0.0 : e1;
      }
    }
    s0 += __shfl_xor(s0, 32, kWave);
    s1 += __shfl_xor(s1, 32, kWave);
    s_sum[w * kWave + lane] = half ? s1 : s0;
    __syncthreads();  // the tile's end barrier: the staging image and s_norm / s_idx are free, s_sum is whole

    // both row halves' sums of the lane's column, in one order for both waves; the next panel's
    // s_sum stores come after the barriers of its main loop
    const double tot = s_sum[wc * kWave + lane] + s_sum[(2 + wc) * kWave + lane];
    if (c != cur) {
      leave();
      cur = c;
    }
    state[0] += tot;
  }

  const double run = state[0];
  const double first_sum = cur == cf ? run : state[kWave], last_sum = cur == cf ? 0.0 : run;
  if (wr != 0 || col >= n) return;
  double* out = a.edges + static_cast<int64_t>(g) * 4 * a.n + col;
  out[0] = first_sum;
  out[a.n] = last_sum;
  out[2 * a.n] = state[2 * kWave];
  out[3 * a.n] = state[3 * kWave];
}

__global__ __launch_bounds__(kSilStitchRows) void silhouette_stitch_kernel(SilhouetteArgs a) {
  __shared__ double s_red[16];
  const int64_t i = static_cast<int64_t>(blockIdx.x) * kSilStitchRows + threadIdx.x;
  const int G = a.groups;
  const int T = min(max(a.num_panels[0], 0), a.max_panels);
  double add = 0.0;
  if (i < a.n) {
    const int own = a.labels[i];
    double av = nan64(), bv = nan64(), sv = nan64();
    if (own >= 0 && own < a.k) {
      const int n_own = a.counts[own];
      double a_raw = 0.0;
      int pc = -1;        // the cluster whose sum is still open at a range's end
      double ps = 0.0;
      auto close = [&]() {
        if (pc < 0 || pc >= a.k) return;
        if (pc == own) a_raw += ps;
        else bv = minimum_of(bv, ps / static_cast<double>(a.counts[pc]));
      };
      for (int g = 0; g < G; ++g) {
        const int t0 = static_cast<int>(static_cast<int64_t>(g) * T / G);
        const int t1 = static_cast<int>(static_cast<int64_t>(g + 1) * T / G);
        if (t0 >= t1) continue;
        const int cf = a.panel_cluster[t0], cl = a.panel_cluster[t1 - 1];
        const double* e = a.edges + static_cast<int64_t>(g) * 4 * a.n + i;
        const double first = e[0], last = e[a.n], inside_min = e[2 * a.n], inside_own = e[3 * a.n];
        if (cf == pc) {
          ps += first;
        } else {
          close();
          pc = cf;
          ps = first;
        }
        bv = minimum_of(bv, inside_min);
        a_raw += inside_own;
        if (cl != cf) {
          close();
          pc = cl;
          ps = last;
        }
      }
      close();
      av = n_own > 1 ? a_raw / static_cast<double>(n_own - 1) : 0.0;
      const double m = av > bv ? av : bv;
      sv = (av != av || bv != bv) ? nan64() : (n_own == 1 || m == 0.0) ? 0.0 : (bv - av) / m;
      add = sv;
    }
    a.a[i] = av;
    a.b[i] = bv;
    a.s[i] = sv;
    a.samples[i] = static_cast<float>(sv);
  }
  add = block_sum(add, s_red);
  if (threadIdx.x == 0) a.block_sums[blockIdx.x] = add;
}

// one wave: the blocks' sums in block order per lane, then the butterfly; lane 0 divides in FP64
__global__ __launch_bounds__(kWave) void silhouette_finish_kernel(SilhouetteArgs a, int blocks) {
  const double total = wave_strided_sum(a.block_sums, blocks);
  long long members = 0, present = 0;
  for (int c = lane_id(); c < a.k; c += kWave) {
    const int cnt = a.counts[c];
    members += cnt;
    present += cnt > 0;
  }
  members = wave_sum(members);
  present = wave_sum(present);
  if (threadIdx.x != 0) return;
  const double v = present >= 2 ? total / static_cast<double>(members) : nan64();
  a.score64[0] = v;
  a.score[0] = static_cast<float>(v);
}

bool args_ok(const SilhouetteArgs& a) {
  return a.x != nullptr && a.norms != nullptr && a.n >= 1 && a.d >= 1 && a.stride >= 0 &&
         a.n < (int64_t{1} << 31) - kT && a.d < (int64_t{1} << 31) - kBK;
}

bool plan_ok(const SilhouetteArgs& a) {
  return a.n >= 1 && a.n < (int64_t{1} << 31) - kT && a.labels != nullptr && a.panel_cluster != nullptr && a.counts != nullptr &&
         a.num_panels != nullptr && a.edges != nullptr && a.k >= 1 && a.max_panels >= 1 && a.groups >= 1 &&
         a.groups <= a.max_panels && static_cast<int64_t>(a.max_panels) * kT < (int64_t{1} << 31);
}

}  // namespace

int64_t silhouette_groups(int64_t n, int64_t max_panels, int64_t d, int64_t groups) {
  const int64_t cols = std::max<int64_t>(1, tiles_of(n));
  const int64_t panels = std::max<int64_t>(1, max_panels);
  if (groups >= 1) return std::min(groups, panels);
  const int64_t stages = std::max<int64_t>(1, (d + kBK - 1) / kBK) + kSilEpilogueStages;
  int64_t best = 1, best_cost = -1;
  for (int64_t g = 1; g <= std::min<int64_t>(panels, kSilMaxGroups); ++g) {
    const int64_t c = (cols * g + kSilCUs - 1) / kSilCUs, t = (panels + g - 1) / g;
    const int64_t cost = c * (t * stages + kSilBlockStages) * (c == 1 ? 4 : 3);
    if (best_cost < 0 || cost < best_cost) {
      best = g;
      best_cost = cost;
    }
  }
  return best;
}

int64_t silhouette_stitch_blocks(int64_t n) { return (n + kSilStitchRows - 1) / kSilStitchRows; }

int launch_silhouette_norms(const SilhouetteArgs& a, hipStream_t stream) {
  if (!args_ok(a)) return -1;
  const bool vec = a.d % 4 == 0 && rows_aligned16(a.x, a.stride);
  const dim3 grid(static_cast<unsigned>((a.n + kWaves - 1) / kWaves));
  if (vec)
    hipLaunchKernelGGL(silhouette_norms_kernel<true>, grid, dim3(kThreads), 0, stream, a);
  else
    hipLaunchKernelGGL(silhouette_norms_kernel<false>, grid, dim3(kThreads), 0, stream, a);
  return static_cast<int>(hipGetLastError());
}

int launch_silhouette_tile(const SilhouetteArgs& a, hipStream_t stream) {
  if (!args_ok(a) || !plan_ok(a) || a.ref_index == nullptr || tiles_of(a.n) * a.groups >= (int64_t{1} << 31)) return -1;
  const bool vec = a.d % 4 == 0 && rows_aligned16(a.x, a.stride);
  const dim3 grid(static_cast<unsigned>(tiles_of(a.n) * a.groups));
  if (vec)
    hipLaunchKernelGGL(silhouette_tile_kernel<true>, grid, dim3(kThreads), 0, stream, a);
  else
    hipLaunchKernelGGL(silhouette_tile_kernel<false>, grid, dim3(kThreads), 0, stream, a);
  return static_cast<int>(hipGetLastError());
}

int launch_silhouette_finish(const SilhouetteArgs& a, hipStream_t stream) {
  if (!plan_ok(a) || a.a == nullptr || a.b == nullptr || a.s == nullptr || a.samples == nullptr ||
      a.block_sums == nullptr || a.score64 == nullptr || a.score == nullptr)
    return -1;
  const int64_t blocks = silhouette_stitch_blocks(a.n);
  hipLaunchKernelGGL(silhouette_stitch_kernel, dim3(static_cast<unsigned>(blocks)), dim3(kSilStitchRows), 0, stream, a);
  hipLaunchKernelGGL(silhouette_finish_kernel, dim3(1), dim3(kWave), 0, stream, a, static_cast<int>(blocks));
  return static_cast<int>(hipGetLastError());
}

}  // namespace tea
