// Operand loaders of the streaming kernels whose score dtype is a template parameter (K1, K2, K7,
// K10, K13, K15, K16, K18), and the float helpers those kernels share.  Device code only.
//
// KIND: 0 = f32, 1 = bf16, 2 = f16.  The host side of every unit maps DType::f32 / bf16 / f16 to
// <0> / <1> / <2> through with_kind of tea_types.h (K1 alone keeps its own table).  (Operands whose dtype is only known at run time go through
// load_as_f32 / f64 / i64 of tea_common.h instead.)
#pragma once

#include "tea_common.h"

namespace tea {

// bytes per element of KIND
template <int KIND>
constexpr int kind_bytes = KIND == 0 ? 4 : 2;

// a 16-bit value of KIND 1 / 2 as float (exact)
template <int KIND>
__device__ __forceinline__ float widen16(uint16_t b) {
  return KIND == 1 ? bf16_to_f32(b) : f16_to_f32(b);
}

// element i of a KIND row
template <int KIND>
__device__ __forceinline__ float load1(const void* row, int64_t i) {
  if constexpr (KIND == 0) return static_cast<const float*>(row)[i];
  return widen16<KIND>(static_cast<const uint16_t*>(row)[i]);
}

// the two 16-bit values of a 32-bit word, low half first, as T = float, or double where the caller
// widens (K16).  Both halves are cut out before either is converted: written as two nested calls
// the bf16 kernels keep their instruction count but order their shifts and masks differently.
template <int KIND, typename T>
__device__ __forceinline__ void unpack2(uint32_t w, T& a, T& b) {
  const uint16_t lo = static_cast<uint16_t>(w & 0xffffu), hi = static_cast<uint16_t>(w >> 16);
  a = widen16<KIND>(lo);
  b = widen16<KIND>(hi);
}

// the eight 16-bit values of one 16-B load into v[0 .. 8)
template <int KIND, typename T>
__device__ __forceinline__ void unpack8(const uint4& x, T* v) {
  const uint32_t w[4] = {x.x, x.y, x.z, x.w};
#pragma unroll
  for (int e = 0; e < 4; ++e) unpack2<KIND>(w[e], v[2 * e], v[2 * e + 1]);
}

// N values from element i of a row, &row[i] 16-B aligned, as N * kind_bytes / 16 16-B loads:
// float4 for f32, 8 x 16-bit for bf16 / f16 (Guideline 13)
template <int KIND, int N>
__device__ __forceinline__ void load_vals(const void* row, int64_t i, float (&v)[N]) {
  constexpr int PER = 16 / kind_bytes<KIND>;
  static_assert(N % PER == 0, "whole 16-B loads");
  if constexpr (KIND == 0) {
    const float4* q = reinterpret_cast<const float4*>(static_cast<const float*>(row) + i);
#pragma unroll
    for (int u = 0; u < N / PER; ++u) {
      const float4 x = q[u];
      v[4 * u] = x.x;
      v[4 * u + 1] = x.y;
      v[4 * u + 2] = x.z;
      v[4 * u + 3] = x.w;
    }
  } else {
    const uint4* q = reinterpret_cast<const uint4*>(static_cast<const uint16_t*>(row) + i);
#pragma unroll
    for (int u = 0; u < N / PER; ++u) unpack8<KIND>(q[u], v + 8 * u);
  }
}

// elements of a KIND row before the next 16-B boundary (p element-aligned): 0 .. 16 / kind_bytes - 1
template <int KIND>
__device__ __forceinline__ int64_t head_elems(const void* p) {
  return static_cast<int64_t>(((16u - (reinterpret_cast<uintptr_t>(p) & 15u)) & 15u) / kind_bytes<KIND>);
}

// Descending-order key of a score: a larger score has a larger key.  -0.0 ties +0.0 (one key for
// both zeros); every NaN, of any sign or payload, is the canonical NaN and so one key above
// +inf's; the key is never 0, which is free to mean "no item" (padding, an empty maximum).
__device__ __forceinline__ uint32_t order_key(float v) {
  uint32_t u = __float_as_uint(v);
  if (v != v) u = 0x7fc00000u;  // canonical NaN: above +inf after the flip
  if (v == 0.f) u = 0u;         // -0.0 == +0.0: one key for both zeros
  return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}

// -inf logits are masked entries (probability 0); a NaN or +inf logit makes the row's sum NaN.
// Where a maximum is still -inf, the exponent is taken against 0 instead: exp(-inf - 0) = 0 where
// exp(-inf - -inf) would be NaN, and a NaN value or sum still reaches s.
__device__ __forceinline__ float finite_or_zero(float mx) { return mx == -__builtin_huge_valf() ? 0.f : mx; }

// NaN-propagating maximum (v_maximum3_f32), where fmaxf lets a NaN lose to a number
__device__ __forceinline__ float fmaximum(float a, float b) { return __builtin_elementwise_maximum(a, b); }
__device__ __forceinline__ float fminimum(float a, float b) { return __builtin_elementwise_minimum(a, b); }

// e^x to about an ulp for x <= 0 (NaN stays NaN): v_exp_f32 of x * log2(e) with the product's
// rounding error and the constant's put back to first order.  The argument is first raised to -200
// by a NaN-propagating maximum: e^-200 is 0 in float32 as is everything below it, and from -inf or
// a finite x near -FLT_MAX the product would overflow to -inf and the error term to +inf, 0 * inf.
// The plain fast form loses |x| * 2^-24 relative to this one, which shows at the tolerance the
// tests of K15 and K18 hold.
__device__ __forceinline__ float exp_neg(float x) {
  constexpr float kL2e = 1.44269502162933349609375f, kL2eLo = 1.92596299112661746e-8f, kLn2 = 0.693147182464599609375f;
  x = fmaximum(x, -200.f);
  const float t = x * kL2e;
  const float lost = __builtin_fmaf(x, kL2e, -t) + x * kL2eLo;
  const float e = __builtin_amdgcn_exp2f(t);  // 2^-288.5 and below: 0
  return __builtin_fmaf(e, lost * kLn2, e);
}

}  // namespace tea
