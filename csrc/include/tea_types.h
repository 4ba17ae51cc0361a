// Host/device-neutral types shared by kernels and the host glue (no device code here).
#pragma once

#include <stdint.h>

#include <type_traits>

namespace tea {

enum class DType : int {
  f32 = 0,
  f16 = 1,
  bf16 = 2,
  f64 = 3,
  i64 = 4,
  i32 = 5,
  u8 = 6,
  b8 = 7,
  i8 = 8,
  i16 = 9,
};

// element size in bytes
constexpr int dtype_bytes(DType d) {
  switch (d) {
    case DType::f64: case DType::i64: return 8;
    case DType::f32: case DType::i32: return 4;
    case DType::f16: case DType::bf16: case DType::i16: return 2;
    default: return 1;
  }
}

// The KIND rule of tea_rowload.h, stated once for the host: f(std::integral_constant<int, KIND>{})
// with KIND 0 / 1 / 2 for f32 / bf16 / f16, and f's int returned; -1 for any other dtype.
template <typename F>
int with_kind(DType dt, F&& f) {
  switch (dt) {
    case DType::f32: return f(std::integral_constant<int, 0>{});
    case DType::bf16: return f(std::integral_constant<int, 1>{});
    case DType::f16: return f(std::integral_constant<int, 2>{});
    default: return -1;
  }
}

// fold workspace size in u64 cells (tea_fold.h: 64 shards x 64-B stride, 16 value slots)
constexpr int kFoldCells = 64 * 8;

}  // namespace tea
