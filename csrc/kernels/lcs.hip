// K30: length of the longest common subsequence (LCS) of padded token-id rows and the ROUGE-L sums of a
// batch, docs/parity.md "Not in the reference".
//
// Replaces the ATen form (functional/text/token_rouge_l.py: one batched row recurrence with a cummax per
// stream position) and a host copy with a Python table.
//
// Bit-parallel table row (Allison-Dix, Crochemore et al., Hyyro).  Rows i = 1..n run over one sequence (the
// stream), columns j = 1..m over the other (stationary).  Row i of the table is the m-bit vector V whose bit
// j - 1 is 0 exactly where L[i][j] = L[i][j - 1] + 1, so L[i][m] is the number of zero bits; V starts as all
// ones.  With M the match word of stream token i (bit j - 1 set where it equals stationary token j):
//     U = V & M;   V = (V + U) | (V & ~M)
// where the addition is one m-bit addition, carries running from column 1 upwards.  There is no per-cell
// dependent chain, no LDS, no barrier and no atomic.
//  * lcs_kernel<Wide, C>: one wave per pair, kLcsPairsPerWg pairs per workgroup.  The host picks the
//    stationary side from the padded widths (the narrower one, `input` on a tie) and the instance
//    C = pow2ceil(ceil(width / 64)), one of 1, 2, 4 .. 64.  Lane l of register c holds stationary column
//    64 c + l (C registers, 2 C for int64 ids), loaded coalesced once.  The stream is loaded 64 tokens at a
//    time, one chunk ahead, and a token is read wave-uniformly by v_readlane.  One v_cmp_eq of a register
//    against the token (one v_cmp_eq_u64 of a register pair for int64 ids) is a 64-bit match word in a lane mask; the
//    compares of different registers are independent of each other and of V.
//     - C == 1 (the narrower width at most 64): V, M and the update are one wave-uniform 64-bit value in
//       scalar registers; no cross-lane carry.
//     - C >= 2: lane c owns word c of V.  The match word of register c goes into lane c of the per-lane M by
//       two v_writelane; registers are skipped wave-uniformly in groups of four past the pair's actual
//       ceil(m / 64).  Then every lane does U, S = V + U, and the carry between lanes comes from two lane
//       masks, G (the lane's addition carried out) and P (S is all ones): the carry-in mask is
//       ((G | P) + G) ^ (G | P) ^ G in 64-bit scalar arithmetic, and V = (S + carry_in) | (V & ~M).
//    Columns at and past m never match: M is ANDed with a validity word computed once (ids are arbitrary,
//    so no token value could mark them), which also makes the lanes past C inert.  The answer is the
//    popcount of ~V below column m, summed over the wave.
//  * lcs_prep_kernel (only with ignore_index): K29's compaction (tea_token_rows.h), same workspace layout.
//  * lcs_finish_kernel (only with totals): one wave computes precision l / len(input), recall
//    l / len(target) and F = 2 P R / (P + R) per pair in float64 (0 where the denominator is 0), every lane
//    adds its pairs in index order, the lanes are folded by the xor butterfly, and the three sums and the
//    pair count are added to the totals.
// Every store of a result is a plain vector store: bit-identical from run to run.
// Measured on MI355X (profiles/token_rouge_l_r45.json; one TokenROUGEL.update, int64 / int32 ids, about 10 %
// edits; medians of 5 alternating rounds):
//   4096 pairs of 10..60 tokens (C = 1)  0.038 / 0.038 ms; ATen form 3.3 / 3.3 ms; K29 0.042 / 0.037 ms
//   1024 pairs of 256 (C = 4)            0.047 / 0.045 ms; ATen form 13.6 / 13.2 ms; K29 0.090 / 0.072 ms
//   256 pairs of 512 (C = 8)             0.094 / 0.092 ms; ATen form 27.3 / 27.1 ms; K29 0.115 / 0.100 ms
//   32 pairs of 2048 (C = 32)            0.914 / 0.842 ms; ATen form 108.6 / 108.0 ms; K29 0.744 / 0.631 ms
// K29 is TokenErrorRate.update on the same rows (the same table size, the arm its rule picks).  This kernel's time
// over K29's is 0.91 / 1.03 at the short pairs (both are two short launches), 0.52 / 0.63 at
// 1024 x 256 and 0.82 / 0.91 at 256 x 512; at 32 x 2048 it is 1.23 / 1.33, slower than K29: 32 waves on a device
// of 1024 SIMDs against K29's eight waves per pair, and no multi-wave arm is built here.  A host copy with the
// two-row table on Python lists takes 0.4 to 10 s at these shapes (scaled from about 2^21 timed cells).
// Measured during the work and kept: int64 ids as whole 64-bit registers compared by v_cmp_eq_u64, against two
// 32-bit compares and a scalar AND: 32 x 2048 int64 went from 1.70 to 0.91 ms, 256 x 512 from 0.150 to 0.094 ms
// (the same benchmark on the earlier build; that run is not kept in profiles/).  The native windows of the
// benchmark are 200 calls, 8 ms at the two smaller shapes: short, though the five rounds lie within about 1 %.
// Not timed: keeping V wave-uniform for C = 2, other pairs per workgroup (4), a deeper prefetch (one chunk),
// the unroll factors, the instance C = 64 (widths above 2048), and kernel times apart from the launches.
// 8-82 VGPRs for int32 ids, 10-148 for int64 (C = 1 .. 64), no scratch.
#include <type_traits>

#include "tea_common.h"
#include "tea_kernels.h"
#include "tea_token_rows.h"

namespace tea {

namespace {

using u64 = unsigned long long;

// v_writelane_b32: this compiler has no __builtin_amdgcn_writelane, so the intrinsic is declared under its own
// (version-dependent) name; switch to the builtin once the toolchain has it
extern "C" __device__ int tea_lcs_writelane(int v, int lane, int old) __asm("llvm.amdgcn.writelane.i32");
// `v` (wave-uniform) into lane l of `old`
__device__ __forceinline__ uint32_t into_lane(uint32_t v, int l, uint32_t old) {
  return static_cast<uint32_t>(tea_lcs_writelane(static_cast<int>(v), l, static_cast<int>(old)));
}

// A token in registers: int64 ids stay whole, in an aligned register pair, so that one v_cmp_eq_u64 compares them.
template <bool Wide>
using Tok = std::conditional_t<Wide, u64, uint32_t>;

// token `idx` of a row; zero at and past `n`
template <bool Wide>
__device__ __forceinline__ Tok<Wide> load_id(const void* row, int idx, int n) {
  return idx < n ? static_cast<const Tok<Wide>*>(row)[idx] : Tok<Wide>(0);
}
// lane l's token as a wave-uniform value
__device__ __forceinline__ uint32_t lane_of(uint32_t v, int l) {
  return static_cast<uint32_t>(__builtin_amdgcn_readlane(static_cast<int>(v), l));
}
__device__ __forceinline__ u64 lane_of(u64 v, int l) {
  return (static_cast<u64>(lane_of(static_cast<uint32_t>(v >> 32), l)) << 32) | lane_of(static_cast<uint32_t>(v), l);
}

// word c of the m valid columns
__device__ __forceinline__ u64 valid_word(int m, int c) {
  const int r = m - 64 * c;
  return r >= 64 ? ~0ull : (r <= 0 ? 0ull : (1ull << r) - 1ull);
}

// One pair as the kernel sees it: `s` is stationary in the lanes, `t` streams past it.
struct Rows {
  const void* s;
  const void* t;
  int m, n;
};

template <bool Wide>
__device__ __forceinline__ Rows rows_of(const LcsArgs& g, int64_t pair) {
  constexpr int64_t kTok = Wide ? 8 : 4;
  const char* in = static_cast<const char*>(g.has_ignore ? g.ws_tokens : g.input);
  const char* tg = g.has_ignore ? in + g.b * g.li * kTok : static_cast<const char*>(g.target);
  const int64_t* il = g.has_ignore ? g.ws_lengths : g.input_lengths;
  const int64_t* tl = g.has_ignore ? g.ws_lengths + g.b : g.target_lengths;
  const int ni = row_len(il, pair, g.li), nt = row_len(tl, pair, g.lt);
  in += pair * g.li * kTok;
  tg += pair * g.lt * kTok;
  // the LCS is symmetric: the narrower padded side fits the instance
  if (g.li <= g.lt) return Rows{in, tg, ni, nt};
  return Rows{tg, in, nt, ni};
}

template <bool Wide, int C>
__global__ __launch_bounds__(kLcsPairsPerWg* kWave) void lcs_kernel(LcsArgs g) {
  const int64_t pair = static_cast<int64_t>(blockIdx.x) * kLcsPairsPerWg + wave_id();
  if (pair >= g.b) return;
  const Rows r = rows_of<Wide>(g, pair);
  const int lane = lane_id();
  if (r.m == 0 || r.n == 0) {
    if (lane == 0) g.out[pair] = 0;
    return;
  }
  Tok<Wide> s[C];
#pragma unroll
  for (int c = 0; c < C; ++c) s[c] = load_id<Wide>(r.s, 64 * c + lane, r.m);
  Tok<Wide> next = load_id<Wide>(r.t, lane, r.n);
  if constexpr (C == 1) {
    const u64 valid = valid_word(r.m, 0);
    u64 v = ~0ull;  // wave-uniform
    for (int base = 0; base < r.n; base += kWave) {
      const Tok<Wide> cur = next;
      next = load_id<Wide>(r.t, base + kWave + lane, r.n);
      const auto step = [&](int t) {
        const u64 match = __ballot(s[0] == lane_of(cur, t)) & valid;
        const u64 u = v & match;
        v = (v + u) | (v & ~match);
      };
      const int steps = r.n - base;
      if (steps >= kWave) {
#pragma unroll 8
        for (int t = 0; t < kWave; ++t) step(t);
      } else {
        for (int t = 0; t < steps; ++t) step(t);
      }
    }
    if (lane == 0) g.out[pair] = __popcll(~v & valid);
  } else {
    constexpr int kGroup = C < 4 ? C : 4;
    const int live = (r.m + 63) >> 6;  // registers that hold a column; at most C
    const u64 valid = valid_word(r.m, lane);
    const u64 lanebit = 1ull << lane;
    u64 v = ~0ull;  // lane c: word c of V
    uint32_t m_lo = 0, m_hi = 0;
    for (int base = 0; base < r.n; base += kWave) {
      const Tok<Wide> cur = next;
      next = load_id<Wide>(r.t, base + kWave + lane, r.n);
      const int steps = r.n - base < kWave ? r.n - base : kWave;
      for (int t = 0; t < steps; ++t) {
        const Tok<Wide> tok = lane_of(cur, t);
#pragma unroll
        for (int c0 = 0; c0 < C; c0 += kGroup) {
          if (c0 < live) {
#pragma unroll
            for (int c = c0; c < c0 + kGroup; ++c) {
              const u64 match = __ballot(s[c] == tok);
              m_lo = into_lane(static_cast<uint32_t>(match), c, m_lo);
              m_hi = into_lane(static_cast<uint32_t>(match >> 32), c, m_hi);
            }
          }
        }
        const u64 match = ((static_cast<u64>(m_hi) << 32) | m_lo) & valid;
        const u64 u = v & match;
        const u64 s = v + u;
        const u64 gen = __ballot(s < u), prop = __ballot(s == ~0ull);
        const u64 x = gen | prop;
        const u64 carry_in = (x + gen) ^ x ^ gen;
        v = (s + ((carry_in & lanebit) != 0 ? 1ull : 0ull)) | (v & ~match);
      }
    }
    const int zeros = wave_sum(__popcll(~v & valid));
    if (lane == 0) g.out[pair] = zeros;
  }
}

template <typename T>
__global__ __launch_bounds__(kTokenPrepWaves* kWave) void lcs_prep_kernel(LcsArgs g) {
  compact_token_rows<T>(g.input, g.target, g.input_lengths, g.target_lengths, g.b, g.li, g.lt, g.ignore_index,
                        g.ws_tokens, g.ws_lengths);
}

__global__ __launch_bounds__(kWave) void lcs_finish_kernel(LcsArgs g) {
  const int64_t* il = g.has_ignore ? g.ws_lengths : g.input_lengths;
  const int64_t* tl = g.has_ignore ? g.ws_lengths + g.b : g.target_lengths;
  double sum[3] = {0.0, 0.0, 0.0};
  for (int64_t i = threadIdx.x; i < g.b; i += kWave) {
    const int n = clamped_len(il, i, g.li), m = clamped_len(tl, i, g.lt);
    const double l = static_cast<double>(g.out[i]);
    const double p = n > 0 ? l / n : 0.0, r = m > 0 ? l / m : 0.0;
    sum[0] += p;
    sum[1] += r;
    sum[2] += p + r > 0.0 ? 2.0 * p * r / (p + r) : 0.0;
  }
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    const double s = j < 3 ? wave_sum(sum[j]) : static_cast<double>(g.b);
    if (threadIdx.x == 0) *g.totals[j] = (g.accumulate ? *g.totals[j] : 0.0) + s;
  }
}

template <bool Wide>
void launch_instance(const LcsArgs& a, dim3 grid, dim3 block, hipStream_t stream) {
  switch (a.chunks) {
    case 1: hipLaunchKernelGGL((lcs_kernel<Wide, 1>), grid, block, 0, stream, a); break;
    case 2: hipLaunchKernelGGL((lcs_kernel<Wide, 2>), grid, block, 0, stream, a); break;
    case 4: hipLaunchKernelGGL((lcs_kernel<Wide, 4>), grid, block, 0, stream, a); break;
    case 8: hipLaunchKernelGGL((lcs_kernel<Wide, 8>), grid, block, 0, stream, a); break;
    case 16: hipLaunchKernelGGL((lcs_kernel<Wide, 16>), grid, block, 0, stream, a); break;
    case 32: hipLaunchKernelGGL((lcs_kernel<Wide, 32>), grid, block, 0, stream, a); break;
    default: hipLaunchKernelGGL((lcs_kernel<Wide, 64>), grid, block, 0, stream, a); break;
  }
}

}  // namespace

bool lcs_geometry_ok(int64_t b, int64_t li, int64_t lt) {
  return b >= 1 && b < (int64_t{1} << 30) && li >= 0 && li <= kLcsMaxLen && lt >= 0 && lt <= kLcsMaxLen;
}

int launch_lcs(const LcsArgs& a, hipStream_t stream) {
  if (!lcs_geometry_ok(a.b, a.li, a.lt) || a.out == nullptr) return -1;
  if ((a.li > 0 && a.input == nullptr) || (a.lt > 0 && a.target == nullptr)) return -1;
  if (a.chunks < lcs_chunks(a.li, a.lt) || a.chunks > kLcsMaxChunks || (a.chunks & (a.chunks - 1)) != 0) return -1;
  if (a.has_ignore && (a.ws_lengths == nullptr || (a.li + a.lt > 0 && a.ws_tokens == nullptr))) return -1;
  const bool totals = a.totals[0] != nullptr;
  for (int j = 0; j < 4; ++j)
    if ((a.totals[j] != nullptr) != totals) return -1;
  if (a.has_ignore) {
    const dim3 grid(static_cast<unsigned>((2 * a.b + kTokenPrepWaves - 1) / kTokenPrepWaves)), block(kTokenPrepWaves * kWave);
    if (a.wide) hipLaunchKernelGGL(lcs_prep_kernel<long long>, grid, block, 0, stream, a);
    else hipLaunchKernelGGL(lcs_prep_kernel<int>, grid, block, 0, stream, a);
  }
  const dim3 grid(static_cast<unsigned>((a.b + kLcsPairsPerWg - 1) / kLcsPairsPerWg)), block(kLcsPairsPerWg * kWave);
  if (a.wide) launch_instance<true>(a, grid, block, stream);
  else launch_instance<false>(a, grid, block, stream);
  if (totals) hipLaunchKernelGGL(lcs_finish_kernel, dim3(1), dim3(kWave), 0, stream, a);
  return static_cast<int>(hipGetLastError());
}

}  // namespace tea
