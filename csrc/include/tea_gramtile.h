// The 128 x 128 FP32 MFMA tile of row inner products <a_i, b_j> that K20 (kid.hip) and K22
// (prdc.hip) share (device only): what both kernels do between the row pointers and the accumulator
// registers.  How the row pointers are formed, how the stages are chained and what happens to the
// accumulators stay with the kernels.
//
// gfx950 mapping:
//  * one block of 256 threads = one 128 x 128 tile.  The contraction runs over the contiguous
//    dimension D, stepped by 32 (a stage).  Four waves; wave w owns the 64 x 64 quadrant
//    (w >> 1, w & 1) as 2 x 2 blocks of v_mfma_f32_32x32x2_f32: exact FP32 products, a k-ordered
//    fmaf chain per element, 64 accumulator registers.
//  * staging: piece q of thread t is row (t >> 3) + 32 q, k [4 (t & 7), + 4) of the stage, for
//    both operands.  Eight consecutive lanes read one row's 128 bytes of the stage with one 16-byte
//    load each (kVec: D % 4 == 0 and every row address 16-byte aligned, rows_aligned16 of
//    tea_common.h), or with four element loads (any other base, row stride or D: correct, not
//    tuned).  A stage's loads go to registers (load) and from there to LDS (store), so the caller
//    can issue the next stage's loads before this stage's MFMAs and store them after.  A nullptr
//    row (past the operand's last row) and the K tail past D stage zeros.
//  * LDS image [k][row] with a row pitch of 130 floats: an operand read is 32 consecutive floats
//    per half-wave, and the four k of a staged 16-byte piece land 8 banks apart per lane group
//    (4 * 130 = 8 mod 32), so a wave's 64 stores spread over all 32 banks.
//  * operand lane map of v_mfma_f32_32x32x2_f32: A[i = lane & 31][k = lane >> 5],
//    B[k][j = lane & 31]; C/D map: register r of block (bm, bn) is row
//    32 bm + (r & 3) + 8 (r >> 2) + 4 (lane >> 5), column 32 bn + (lane & 31) of the quadrant.
#pragma once

#include "tea_common.h"

namespace tea {
namespace gramtile {

constexpr int kT = 128;        // rows and columns of the tile
constexpr int kBK = 32;        // k per stage
constexpr int kThreads = 256;  // 4 waves
constexpr int kPitch = kT + 2; // floats between two k rows of the LDS image
constexpr int kImage = kBK * kPitch;              // floats of one operand's LDS image
constexpr int kPieces = kT * kBK / 4 / kThreads;  // 16-byte pieces per thread per operand (4)
static_assert(kPieces * 32 == kT, "a thread's pieces are 32 rows apart");

typedef float f32x16 __attribute__((ext_vector_type(16)));

inline int64_t tiles_of(int64_t rows) { return (rows + kT - 1) / kT; }

// columns [col, col + 4) of row p of width d; zeros for a nullptr row and past d
template <bool kVec>
__device__ __forceinline__ float4 fetch(const float* p, int col, int d) {
  float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
  if (p == nullptr) return v;
  if constexpr (kVec) {
    if (col < d) v = *reinterpret_cast<const float4*>(p + col);  // d % 4 == 0: wholly inside
  } else {
    if (col < d) v.x = p[col];
    if (col + 1 < d) v.y = p[col + 1];
    if (col + 2 < d) v.z = p[col + 2];
    if (col + 3 < d) v.w = p[col + 3];
  }
  return v;
}

// A thread's share of the staging: its place in the stage and the rows of its kPieces pieces of
// either operand (nullptr past the operand's last row), all set by the kernel, and the registers a
// stage passes through.  One object: with pa / pb handed to free functions as arrays the pointers
// are kept as <4 x ptr> values, their address space is lost and every load becomes a flat_load
// (profiles/gramtile_dedup_codegen.txt).
struct Stage {
  int rslot, kq;  // threadIdx.x >> 3, threadIdx.x & 7
  int d;          // the rows' width
  const float* pa[kPieces];
  const float* pb[kPieces];
  float4 va[kPieces], vb[kPieces];

  // the stage at k0 into registers
  template <bool kVec>
  __device__ __forceinline__ void load(int k0) {
#pragma unroll
    for (int q = 0; q < kPieces; ++q) {
      va[q] = fetch<kVec>(pa[q], k0 + 4 * kq, d);
      vb[q] = fetch<kVec>(pb[q], k0 + 4 * kq, d);
    }
  }

  // the loaded stage into the LDS images
  __device__ __forceinline__ void store(float (&sA)[kImage], float (&sB)[kImage]) const {
#pragma unroll
    for (int q = 0; q < kPieces; ++q) {
      const int o = 4 * kq * kPitch + rslot + 32 * q;
      sA[o] = va[q].x;
      sA[o + kPitch] = va[q].y;
      sA[o + 2 * kPitch] = va[q].z;
      sA[o + 3 * kPitch] = va[q].w;
      sB[o] = vb[q].x;
      sB[o + kPitch] = vb[q].y;
      sB[o + 2 * kPitch] = vb[q].z;
      sB[o + 3 * kPitch] = vb[q].w;
    }
  }
};

// where a lane reads its operand of k 0 / 1 in an image: `half` is the quadrant's row half
// (w >> 1, for sA) or column half (w & 1, for sB)
__device__ __forceinline__ int operand_offset(int lane, int half) {
  return (lane >> 5) * kPitch + half * 64 + (lane & 31);
}

// row, within a 32 x 32 block, of accumulator register r of this lane (its column is lane & 31)
__device__ __forceinline__ int cd_row(int r, int lane) { return (r & 3) + 8 * (r >> 2) + 4 * (lane >> 5); }

__device__ __forceinline__ void zero(f32x16 (&acc)[2][2]) {
#pragma unroll
  for (int bm = 0; bm < 2; ++bm)
#pragma unroll
    for (int bn = 0; bn < 2; ++bn)
#pragma unroll
      for (int r = 0; r < 16; ++r) acc[bm][bn][r] = 0.f;
}

// the staged 32 k into the quadrant's accumulators, in k order (between two barriers)
__device__ __forceinline__ void mfma_stage(const float (&sA)[kImage], const float (&sB)[kImage], int offA, int offB,
                                           f32x16 (&acc)[2][2]) {
#pragma unroll
  for (int kk = 0; kk < kBK / 2; ++kk) {
    const float a0 = sA[2 * kk * kPitch + offA], a1 = sA[2 * kk * kPitch + offA + 32];
    const float b0 = sB[2 * kk * kPitch + offB], b1 = sB[2 * kk * kPitch + offB + 32];
    acc[0][0] = __builtin_amdgcn_mfma_f32_32x32x2f32(a0, b0, acc[0][0], 0, 0, 0);
    acc[0][1] = __builtin_amdgcn_mfma_f32_32x32x2f32(a0, b1, acc[0][1], 0, 0, 0);
    acc[1][0] = __builtin_amdgcn_mfma_f32_32x32x2f32(a1, b0, acc[1][0], 0, 0, 0);
    acc[1][1] = __builtin_amdgcn_mfma_f32_32x32x2f32(a1, b1, acc[1][1], 0, 0, 0);
  }
}

}  // namespace gramtile
}  // namespace tea
