// K22: improved precision / recall and density / coverage (docs/parity.md, "Not in the reference").
//
// Both pairs are k-nearest-neighbour statistics of the squared distances
//   d2(a, b) = max(0, (|a|^2 + |b|^2) - 2 <a, b>)          (combined in FP64)
// between the real features X [N, D] and the generated features Y [M, D]:
//   r_i^2 = k-th smallest d2(x_i, x_j), j != i (positional)     s_j^2 likewise within Y
//   hits_fake[j] = #{i : d2(y_j, x_i) <= r_i^2}                 nearest_fake[j] = min_i d2(y_j, x_i)
//   hits_real[i] = #{j : d2(x_i, y_j) <= s_j^2}                 nearest_real[i] = min_j d2(x_i, y_j)
// The ATen form writes four [N, M]-sized distance matrices (chunked) and runs topk and several mask
// and reduce passes over them.  Here an inner product never leaves its block and a distance never
// leaves a register.
//
// prdc_norms_kernel: a wave per row of either set, FP64 sum of the squares (each square of a widened
// float32 is exact in FP64); lane l takes the columns 4 l .. 4 l + 3 (+ 256 per step) in both load
// arms, so the arms add in one order.
//
// prdc_tile_kernel<Mode, kVec>, gfx950 mapping (the only arm; the tile itself is tea_gramtile.h's):
//  * block (p, g) owns the 128-row panel p of the query set and walks the column tiles g, g + G, ...
//    of the reference set (G = PrdcTileArgs::groups, rule at prdc_groups).  Rows are addressed
//    directly; the rows past n_q and the columns past n_ref stage zeros.  The next stage's loads are
//    issued before this stage's MFMAs.
//  * unlike K20 the inner product is not one chain: a selection compares single
//    distances, where K20 adds thousands, and one k-ordered float32 fmaf chain over D = 2048
//    non-negative features is off by up to 2.6e-6 of sum |a_k| |b_k| (its partial sum grows with k
//    and every step rounds at its size).  The MFMAs therefore run a chain per 128 k (four stages) in
//    a second register set, whose sum is added to the accumulator in float32, in k order: 64 adds
//    per 256 MFMAs, and a largest error of 3e-7 of sum |a_k| |b_k| at D = 768 and 2048.  The first
//    stage of the block's next tile is loaded into registers ahead of the epilogue.
//  * epilogue: accumulator register (bm, r) of a wave is one row per half-wave, whose 32 lanes hold
//    2 x 32 of its columns.  The registers pass through the wave's own 8 KB of the (now free) staging
//    image, 32 at a time, each lane reading back what it wrote, so the steps below are a loop over r.  Each element is widened to FP64
//    and combined with the row's norm (LDS, loaded once per block) and the column's norm (two
//    registers per lane and tile).  The state of a row is kept per wave, so the two waves that share
//    a row panel never meet: a block writes two lists per row, one per 64-column half of its tiles.
//  * Knn (query = reference): the row's own column and the padding columns become +inf.  The wave's
//    64 rows keep their k smallest values ascending in LDS (+inf in unfilled slots).  Per register
//    the half-wave reads the row's k-th value (one broadcast LDS read); if no lane holds a smaller
//    candidate (one ballot, the common case after the first tiles) it moves on.  Otherwise lanes
//    0 .. k - 1 of the half-wave take the list into a register each and at most k rounds follow: the
//    half-wave minimum of the candidates by five xor shuffles, the lowest lane that holds it drops
//    it, and the list lanes shift it in (one shuffle up).  Values leave in ascending order, so after
//    k rounds nothing smaller than the k-th remains; the loop is bounded by k whatever the data.
//    The k smallest are a multiset (equal values are kept as often as they occur), so the lists do
//    not depend on the tile order or on G.
//  * Cross (query != reference): per register two ballots count the columns with d2 <= rad2[col]
//    (padding columns masked out) and the first lane of the half-wave adds the two popcounts to the
//    row's count in LDS; the row's minimum is lowered only when a ballot finds a lane below it.
//  * at the end the wave stores its rows' state to [row][2 g + (w & 1)], non-atomically.
// prdc_radii_kernel: a thread per row merges the row's 2 G ascending lists into the 8 smallest of
// their union by ordered insertion and stores the k-th.  prdc_hits_kernel: a thread per row of
// either side folds the row's lists into hits and nearest (run_fold's plan at eight loads of each kind
// in flight; run_fold itself at 16 spills scalar registers next to this kernel's 17 arguments), and
// the block adds its tallies (block_sum) into one int64 [4] partial.
// prdc_finish_kernel: one wave adds the blocks' partials (wave_strided_sum) and lane 0 divides in
// FP64.  No atomics, no host sync, no cross-block waiting: results are bit-identical from run to run.
#include <algorithm>

#include "tea_common.h"
#include "tea_gramtile.h"
#include "tea_kernels.h"
#include "tea_partials.h"

namespace tea {

namespace {

using namespace gramtile;

constexpr int kChunk = 128;    // k per MFMA chain: four stages, then the chain's sum joins the accumulator
constexpr int kWaves = kThreads / kWave;
constexpr int kWaveRows = 64;  // rows (and columns) of a wave's quadrant
constexpr int kRadiiThreads = 256;
static_assert(kPrdcTile == kT, "the tile is tea_gramtile.h's");
static_assert(kWaves * kWaveRows == 2 * kT, "four quadrants of 64 x 64");
static_assert(2 * 32 * kWave <= kImage, "two waves' epilogue halves fit one operand's staging image");

enum class Mode { Knn, Cross };

__device__ __forceinline__ double inf64() { return __builtin_huge_val(); }

// the minimum over the 32 lanes of a half-wave, in each of them (a NaN loses to a number)
__device__ __forceinline__ double half_wave_min(double m) {
#pragma unroll
  for (int o = 16; o > 0; o >>= 1) m = fmin(m, __shfl_xor(m, o, kWave));
  return m;
}

template <bool kVec>
__global__ __launch_bounds__(kThreads) void prdc_norms_kernel(PrdcNormsArgs a) {
  const int64_t row = static_cast<int64_t>(blockIdx.x) * kWaves + (threadIdx.x >> 6);
  if (row >= a.n_r + a.n_f) return;  // whole wave
  const bool fake = row >= a.n_r;
  const float* p = fake ? a.fake + (row - a.n_r) * a.fake_stride : a.real + row * a.real_stride;
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
  if (lane_id() == 0) (fake ? a.norms_fake + (row - a.n_r) : a.norms_real + row)[0] = s;
}

template <Mode kMode, bool kVec>
__global__ __launch_bounds__(kThreads, 2) void prdc_tile_kernel(PrdcTileArgs a, int col_tiles) {
  constexpr bool kKnn = kMode == Mode::Knn;
  const int G = a.groups;
  const int p = blockIdx.x / G;
  const int g = blockIdx.x % G;
  const int n_q = static_cast<int>(a.n_q);
  const int n_ref = static_cast<int>(a.n_ref);
  const int d = static_cast<int>(a.d);
  const int k = a.k;

  __shared__ __attribute__((aligned(16))) float sA[kImage];
  __shared__ __attribute__((aligned(16))) float sB[kImage];
  __shared__ double s_norm[kT];                                               // the panel's row norms
  __shared__ double s_top[kKnn ? kWaves * kWaveRows * kPrdcMaxK : 1];         // Knn: [wave][row][slot]
  __shared__ double s_min[kKnn ? 1 : kWaves * kWaveRows];                     // Cross: [wave][row]
  __shared__ uint32_t s_cnt[kKnn ? 1 : kWaves * kWaveRows];

  const int lane = threadIdx.x & 63;
  const int w = threadIdx.x >> 6;
  const int wr = w >> 1, wc = w & 1;
  const int half = lane >> 5, j = lane & 31;

  if (threadIdx.x < kT) {
    const int gi = p * kT + static_cast<int>(threadIdx.x);
    s_norm[threadIdx.x] = gi < n_q ? a.norms_q[gi] : 0.0;
  }
  if constexpr (kKnn) {
#pragma unroll
    for (int s = 0; s < kPrdcMaxK; ++s) s_top[(w * kWaveRows + lane) * kPrdcMaxK + s] = inf64();
  } else {
    s_min[w * kWaveRows + lane] = inf64();
    s_cnt[w * kWaveRows + lane] = 0u;
  }
  // the main loop's barriers order these stores before the first epilogue

  // ---- staging: the thread's rows of the panel; those of a column tile at first_stage
  Stage st;
  st.rslot = threadIdx.x >> 3;
  st.kq = threadIdx.x & 7;
  st.d = d;
#pragma unroll
  for (int q = 0; q < kPieces; ++q) {
    const int gi = p * kT + st.rslot + 32 * q;
    st.pa[q] = gi < n_q ? a.query + static_cast<int64_t>(gi) * a.query_stride : nullptr;
  }
  const int offA = operand_offset(lane, wr), offB = operand_offset(lane, wc);

  auto first_stage = [&](int tj) {  // the tile's column rows, and its first stage into registers
#pragma unroll
    for (int q = 0; q < kPieces; ++q) {
      const int gj = tj * kT + st.rslot + 32 * q;
      st.pb[q] = gj < n_ref ? a.ref + static_cast<int64_t>(gj) * a.ref_stride : nullptr;
    }
    st.load<kVec>(0);
  };
  first_stage(g);
  for (int tj = g; tj < col_tiles; tj += G) {
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

    if (tj + G < col_tiles) first_stage(tj + G);  // the next tile's loads fly behind the epilogue

    // ---- epilogue
    const int c0 = tj * kT + wc * 64 + j, c1 = c0 + 32;
    const bool in0 = c0 < n_ref, in1 = c1 < n_ref;
    const double nb0 = in0 ? a.norms_ref[c0] : 0.0, nb1 = in1 ? a.norms_ref[c1] : 0.0;
    double rd0 = 0.0, rd1 = 0.0;
    if constexpr (!kKnn) {
      rd0 = in0 ? a.radii_ref[c0] : 0.0;
      rd1 = in1 ? a.radii_ref[c1] : 0.0;
    }
    // The tile leaves the registers through the wave's 8 KB of the staging image (free after the main
    // loop's last barrier), half of it at a time, so the steps below are one loop over a register
    // number and not 32 unrolled copies that hold all 64 values widened.  A lane reads back only
    // what it wrote itself.
    float* stage = (w < 2 ? sA : sB) + (w & 1) * (32 * kWave) + lane;
#pragma unroll
    for (int bm = 0; bm < 2; ++bm) {
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        stage[(2 * r) * kWave] = acc[bm][0][r];
        stage[(2 * r + 1) * kWave] = acc[bm][1][r];
      }
#pragma unroll 1
      for (int r = 0; r < 16; ++r) {
        const int rl = bm * 32 + cd_row(r, lane);  // row of the wave's 64
        const double na = s_norm[wr * 64 + rl];
        double e0 = fmax(0.0, (na + nb0) - 2.0 * static_cast<double>(stage[(2 * r) * kWave]));
        double e1 = fmax(0.0, (na + nb1) - 2.0 * static_cast<double>(stage[(2 * r + 1) * kWave]));
        if constexpr (kKnn) {
          const int gi = p * kT + wr * 64 + rl;
          e0 = in0 && c0 != gi ? e0 : inf64();
          e1 = in1 && c1 != gi ? e1 : inf64();
          double* list = &s_top[(w * kWaveRows + rl) * kPrdcMaxK];
          double thr = list[k - 1];
          if (__ballot(e0 < thr || e1 < thr) == 0) continue;
          double v = j < kPrdcMaxK ? list[j] : inf64();  // lanes 0 .. k - 1 of the half-wave: the list
          for (int round = 0; round < k; ++round) {
            const double m = half_wave_min(fmin(e0, e1));
            const bool live = m < thr;
            if (__ballot(live) == 0) break;
            const bool holds = live && (e0 == m || e1 == m);
            const uint32_t holders = static_cast<uint32_t>(__ballot(holds) >> (32 * half));
            if (holds && j == __builtin_ctz(holders)) {
              if (e0 == m) e0 = inf64();
              else e1 = inf64();
            }
            const double up = __shfl_up(v, 1, kWave);
            if (live) v = v <= m ? v : (j == 0 || up <= m ? m : up);
            thr = __shfl(v, 32 * half + k - 1, kWave);
          }
          if (j < k) list[j] = v;
        } else {
          const uint64_t hit0 = __ballot(in0 && e0 <= rd0), hit1 = __ballot(in1 && e1 <= rd1);
          double m = fmin(in0 ? e0 : inf64(), in1 ? e1 : inf64());
          const double cur = s_min[w * kWaveRows + rl];
          const bool lower = __ballot(m < cur) != 0;
          if (lower) m = half_wave_min(m);
          if (j == 0) {
            s_cnt[w * kWaveRows + rl] += __popc(static_cast<uint32_t>(hit0 >> (32 * half))) +
                                         __popc(static_cast<uint32_t>(hit1 >> (32 * half)));
            if (lower && m < cur) s_min[w * kWaveRows + rl] = m;
          }
        }
      }
    }
    __syncthreads();  // the next tile's first stage overwrites the image the waves read back from
  }

  // ---- the wave's 64 rows leave: lane = row of the wave
  __syncthreads();
  const int gi = p * kT + wr * 64 + lane;
  if (gi >= n_q) return;
  const int64_t slot = static_cast<int64_t>(gi) * (2 * G) + 2 * g + wc;
  if constexpr (kKnn) {
    for (int s = 0; s < k; ++s) a.partial[slot * k + s] = s_top[(w * kWaveRows + lane) * kPrdcMaxK + s];
  } else {
    a.counts[slot] = s_cnt[w * kWaveRows + lane];
    a.mins[slot] = s_min[w * kWaveRows + lane];
  }
}

__global__ __launch_bounds__(kRadiiThreads) void prdc_radii_kernel(const double* partial, int64_t n, int lists, int k,
                                                                   double* radii) {
  const int64_t row = static_cast<int64_t>(blockIdx.x) * kRadiiThreads + threadIdx.x;
  if (row >= n) return;
  double best[kPrdcMaxK];
#pragma unroll
  for (int s = 0; s < kPrdcMaxK; ++s) best[s] = inf64();
  const double* p = partial + row * lists * k;
  for (int i = 0; i < lists * k; ++i) {
    double v = p[i];
#pragma unroll
    for (int s = 0; s < kPrdcMaxK; ++s) {  // ordered insertion: v carries the value pushed down
      const double lo = fmin(best[s], v), hi = fmax(best[s], v);
      best[s] = lo;
      v = hi;
    }
  }
  double kth = best[0];
#pragma unroll
  for (int s = 1; s < kPrdcMaxK; ++s) kth = s == k - 1 ? best[s] : kth;
  radii[row] = kth;
}

// Rows [kPrdcHitsRows b, + kPrdcHitsRows) of the generated side (b < blocks_f), then of the real
// side: a thread folds its row's lists (eight loads of each kind in flight, clamped to the last list
// and counted as nothing past it) into hits and nearest, and the block adds its two tallies.
__global__ __launch_bounds__(kPrdcHitsRows) void prdc_hits_kernel(PrdcFinishArgs a, int blocks_f) {
  __shared__ long long s_red[2][kPrdcHitsRows / kWave];
  const bool fake = static_cast<int>(blockIdx.x) < blocks_f;
  const int64_t n = fake ? a.n_f : a.n_r;
  const int lists = fake ? a.lists_f : a.lists_r;
  const int64_t row = static_cast<int64_t>(fake ? blockIdx.x : blockIdx.x - blocks_f) * kPrdcHitsRows + threadIdx.x;
  long long some = 0, sum = 0;  // fake: precise rows, total hits; real: recalled rows, covered rows
  if (row < n) {
    const uint32_t* counts = (fake ? a.counts_fake : a.counts_real) + row * lists;
    const double* mins = (fake ? a.mins_fake : a.mins_real) + row * lists;
    uint32_t c = 0u;
    double m = inf64();
    for (int l0 = 0; l0 < lists; l0 += 8) {
      uint32_t u[8];
      double v[8];
#pragma unroll
      for (int i = 0; i < 8; ++i) {
        u[i] = counts[min(l0 + i, lists - 1)];
        v[i] = mins[min(l0 + i, lists - 1)];
      }
#pragma unroll
      for (int i = 0; i < 8; ++i) {
        c += l0 + i < lists ? u[i] : 0u;
        m = fmin(m, v[i]);
      }
    }
    (fake ? a.hits_fake : a.hits_real)[row] = static_cast<int32_t>(c);
    (fake ? a.nearest_fake : a.nearest_real)[row] = m;
    some = c > 0u;
    sum = fake ? static_cast<long long>(c) : static_cast<long long>(m <= a.radii_real[row]);
  }
  some = block_sum(some, s_red[0]);
  sum = block_sum(sum, s_red[1]);
  if (threadIdx.x != 0) return;
  int64_t* out = a.block_tallies + 4 * static_cast<int64_t>(blockIdx.x);
  out[0] = fake ? some : 0;
  out[1] = fake ? 0 : some;
  out[2] = fake ? sum : 0;
  out[3] = fake ? 0 : sum;
}

// one wave: the blocks' tallies in block order per lane, then the butterfly; lane 0 divides in FP64
__global__ __launch_bounds__(kWave) void prdc_finish_kernel(PrdcFinishArgs a, int blocks) {
  long long t[4];
  wave_strided_sum(reinterpret_cast<const long long*>(a.block_tallies), blocks, 4, 1, t);
  if (threadIdx.x != 0) return;
#pragma unroll
  for (int i = 0; i < 4; ++i) a.tallies[i] = t[i];
  const double n_r = static_cast<double>(a.n_r), n_f = static_cast<double>(a.n_f);
  a.values[0] = static_cast<float>(static_cast<double>(t[0]) / n_f);
  a.values[1] = static_cast<float>(static_cast<double>(t[1]) / n_r);
  a.values[2] = static_cast<float>(static_cast<double>(t[2]) / (static_cast<double>(a.k) * n_f));
  a.values[3] = static_cast<float>(static_cast<double>(t[3]) / n_r);
}

bool tile_args_ok(const PrdcTileArgs& a) {
  if (a.n_q < 1 || a.n_ref < 1 || a.d < 1 || a.groups < 1 || a.groups > tiles_of(a.n_ref)) return false;
  if (a.n_q >= (int64_t{1} << 31) - kT || a.n_ref >= (int64_t{1} << 31) - kT || a.d >= (int64_t{1} << 31) - kBK)
    return false;
  return tiles_of(a.n_q) * a.groups < (int64_t{1} << 31);
}

template <Mode kMode>
int launch_tile(const PrdcTileArgs& a, hipStream_t stream) {
  const bool vec = a.d % 4 == 0 && rows_aligned16(a.query, a.query_stride) && rows_aligned16(a.ref, a.ref_stride);
  const dim3 grid(static_cast<unsigned>(tiles_of(a.n_q) * a.groups));
  const int col_tiles = static_cast<int>(tiles_of(a.n_ref));
  if (vec)
    hipLaunchKernelGGL((prdc_tile_kernel<kMode, true>), grid, dim3(kThreads), 0, stream, a, col_tiles);
  else
    hipLaunchKernelGGL((prdc_tile_kernel<kMode, false>), grid, dim3(kThreads), 0, stream, a, col_tiles);
  return static_cast<int>(hipGetLastError());
}

}  // namespace

int64_t prdc_groups(int64_t n_query, int64_t n_ref, int64_t d, int64_t groups) {
  const int64_t panels = std::max<int64_t>(1, tiles_of(n_query));
  const int64_t tiles = std::max<int64_t>(1, tiles_of(n_ref));
  if (groups >= 1) return std::min(groups, tiles);
  const int64_t stages = std::max<int64_t>(1, (d + kBK - 1) / kBK);
  int64_t best = 1, best_cost = -1;
  for (int64_t g = 1; g <= std::min<int64_t>(tiles, kPrdcMaxGroups); ++g) {
    const int64_t c = (panels * g + kPrdcCUs - 1) / kPrdcCUs, t = (tiles + g - 1) / g;
    const int64_t cost = c * (t * stages + kPrdcBlockStages) * (c == 1 ? 4 : 3);
    if (best_cost < 0 || cost < best_cost) {
      best = g;
      best_cost = cost;
    }
  }
  return best;
}

int64_t prdc_hits_blocks(int64_t n_r, int64_t n_f) {
  return (n_r + kPrdcHitsRows - 1) / kPrdcHitsRows + (n_f + kPrdcHitsRows - 1) / kPrdcHitsRows;
}

int launch_prdc_norms(const PrdcNormsArgs& a, hipStream_t stream) {
  if (a.n_r < 1 || a.n_f < 1 || a.d < 1 || a.d >= (int64_t{1} << 31) || a.n_r + a.n_f >= (int64_t{1} << 32)) return -1;
  const bool vec = a.d % 4 == 0 && rows_aligned16(a.real, a.real_stride) && rows_aligned16(a.fake, a.fake_stride);
  const dim3 grid(static_cast<unsigned>((a.n_r + a.n_f + kWaves - 1) / kWaves));
  if (vec)
    hipLaunchKernelGGL(prdc_norms_kernel<true>, grid, dim3(kThreads), 0, stream, a);
  else
    hipLaunchKernelGGL(prdc_norms_kernel<false>, grid, dim3(kThreads), 0, stream, a);
  return static_cast<int>(hipGetLastError());
}

int launch_prdc_knn(const PrdcTileArgs& a, hipStream_t stream) {
  if (!tile_args_ok(a) || a.k < 1 || a.k > kPrdcMaxK || a.partial == nullptr) return -1;
  return launch_tile<Mode::Knn>(a, stream);
}

int launch_prdc_cross(const PrdcTileArgs& a, hipStream_t stream) {
  if (!tile_args_ok(a) || a.radii_ref == nullptr || a.counts == nullptr || a.mins == nullptr) return -1;
  return launch_tile<Mode::Cross>(a, stream);
}

int launch_prdc_radii(const double* partial, int64_t n, int lists, int k, double* radii, hipStream_t stream) {
  if (n < 1 || n >= (int64_t{1} << 31) || lists < 1 || k < 1 || k > kPrdcMaxK) return -1;
  const dim3 grid(static_cast<unsigned>((n + kRadiiThreads - 1) / kRadiiThreads));
  hipLaunchKernelGGL(prdc_radii_kernel, grid, dim3(kRadiiThreads), 0, stream, partial, n, lists, k, radii);
  return static_cast<int>(hipGetLastError());
}

int launch_prdc_finish(const PrdcFinishArgs& a, hipStream_t stream) {
  if (a.n_r < 1 || a.n_f < 1 || a.lists_r < 1 || a.lists_f < 1 || a.k < 1 || a.block_tallies == nullptr) return -1;
  const int64_t blocks = prdc_hits_blocks(a.n_r, a.n_f);
  if (blocks >= (int64_t{1} << 31)) return -1;
  const int blocks_f = static_cast<int>((a.n_f + kPrdcHitsRows - 1) / kPrdcHitsRows);
  const dim3 grid(static_cast<unsigned>(blocks));
  hipLaunchKernelGGL(prdc_hits_kernel, grid, dim3(kPrdcHitsRows), 0, stream, a, blocks_f);
  hipLaunchKernelGGL(prdc_finish_kernel, dim3(1), dim3(kWave), 0, stream, a, static_cast<int>(blocks));
  return static_cast<int>(hipGetLastError());
}

}  // namespace tea
