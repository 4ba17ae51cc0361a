// Tensor-side helpers shared by the binding units (csrc/bindings/*.cpp): dtype tags, the current
// HIP stream, argument checks that several ops repeat word for word, and the per-stream
// workspaces.  ATen only: nothing of pybind11 or the torch extension umbrella header here.
#pragma once

#include <ATen/ATen.h>
#include <ATen/hip/impl/HIPGuardImplMasqueradingAsCUDA.h>
#include <ATen/hip/impl/HIPStreamMasqueradingAsCUDA.h>

#include <initializer_list>

#include "tea_types.h"

namespace tea_torch {

using at::Tensor;
using c10::optional;
using DeviceGuard = c10::hip::OptionalHIPGuardMasqueradingAsCUDA;

inline tea::DType dt_of(const Tensor& t) {
  switch (t.scalar_type()) {
    case at::kFloat: return tea::DType::f32;
    case at::kHalf: return tea::DType::f16;
    case at::kBFloat16: return tea::DType::bf16;
    case at::kDouble: return tea::DType::f64;
    case at::kLong: return tea::DType::i64;
    case at::kInt: return tea::DType::i32;
    case at::kByte: return tea::DType::u8;
    case at::kBool: return tea::DType::b8;
    case at::kChar: return tea::DType::i8;
    case at::kShort: return tea::DType::i16;
    default: TORCH_CHECK(false, "torcheval_amd._C: unsupported dtype ", t.scalar_type());
  }
  return tea::DType::f32;
}

inline hipStream_t stream_for(const Tensor& t) {
  return c10::hip::getCurrentHIPStreamMasqueradingAsCUDA(t.device().index()).stream();
}

inline void check_gpu(const Tensor& t, const char* name) {
  TORCH_CHECK(t.is_cuda(), "torcheval_amd._C: ", name, " must be a ROCm (cuda) tensor");
}

inline float* f32_out(const optional<Tensor>& t, const Tensor& ref, int64_t numel, const char* name) {
  if (!t.has_value()) return nullptr;
  const Tensor& x = *t;
  TORCH_CHECK(x.scalar_type() == at::kFloat, "torcheval_amd._C: ", name, " must be float32");
  TORCH_CHECK(x.is_contiguous(), "torcheval_amd._C: ", name, " must be contiguous");
  TORCH_CHECK(x.device() == ref.device(), "torcheval_amd._C: ", name, " on wrong device");
  TORCH_CHECK(x.numel() == numel, "torcheval_amd._C: ", name, " must have ", numel,
              " elements, got ", x.numel());
  return x.data_ptr<float>();
}

// float32 [n >= 1, D >= 1] features with unit stride along D (K20, K22)
inline void check_features(const Tensor& t, const char* what, const char* name) {
  check_gpu(t, name);
  TORCH_CHECK(t.scalar_type() == at::kFloat && t.dim() == 2 && t.size(0) >= 1 && t.size(1) >= 1 &&
                  (t.stride(1) == 1 || t.size(1) == 1) && t.stride(0) >= 0,
              what, ": ", name, " must be a float32 [n, D] tensor with unit stride along D");
}

// the data of a contiguous tensor of `dtype` with `numel` elements on `ref`'s device
inline void* dense_buf(const Tensor& t, at::ScalarType dtype, const Tensor& ref, int64_t numel, const char* what,
                       const char* name) {
  TORCH_CHECK(t.scalar_type() == dtype && t.is_contiguous() && t.numel() == numel && t.device() == ref.device(),
              what, ": ", name, " must be a contiguous ", dtype, " tensor of ", numel,
              " elements on the inputs' device");
  return t.data_ptr();
}
inline double* f64_buf(const Tensor& t, const Tensor& ref, int64_t numel, const char* what, const char* name) {
  return static_cast<double*>(dense_buf(t, at::kDouble, ref, numel, what, name));
}

inline void check_launch(int rc, const char* what) {
  TORCH_CHECK(rc == 0, "torcheval_amd._C: ", what, " launch failed (code ", rc, ")");
}

// ATen compares a tensor with a Python threshold in the tensor's dtype: the threshold is cast to
// it (round to nearest even, c10's conversions) before ``x < threshold``.  Every bf16 / f16 score
// is exact in float32, so a float32 compare against the rounded threshold decides identically.
// Other dtypes: float32 (float32 scores; integer and bool scores promote to it).
inline float threshold_as(const Tensor& scores, double threshold) {
  const float t = static_cast<float>(threshold);
  if (scores.scalar_type() == at::kBFloat16) return static_cast<float>(c10::BFloat16(t));
  if (scores.scalar_type() == at::kHalf) return static_cast<float>(c10::Half(t));
  return t;
}

// the optional error-flag tensor of an op `what`: null when absent
inline int* err_ptr(const optional<Tensor>& err, const Tensor& ref, const char* what) {
  if (!err.has_value()) return nullptr;
  TORCH_CHECK(err->scalar_type() == at::kInt && err->numel() >= 1 && err->device() == ref.device(),
              what, ": err must be an int32 tensor on the input device");
  return err->data_ptr<int>();
}

// the (sum, count) class states that K12 / K13 accumulate into
inline void check_f64_scalar_states(std::initializer_list<const optional<Tensor>*> states, const Tensor& ref,
                                    const char* what) {
  for (const auto* s : states) {
    if (!s->has_value()) continue;
    const Tensor& t = **s;
    TORCH_CHECK(t.scalar_type() == at::kDouble && t.numel() == 1 && t.device() == ref.device(),
                what, ": class states must be float64 scalars on the inputs' device");
  }
}

// ---------------------------------------------------------------- per-stream workspaces
// One cache per process (csrc/bindings/workspace.cpp), keyed by (device, stream, kind, slot):
// at least 64 KiB, grown on demand, never freed.  Every (kind, user) pair has its own slot, so
// no two users ever see one buffer unless they mean to.  Allocate (warm up) before any HIP-graph
// capture that uses one.

// Zero-filled when allocated; the kernels that use one leave it zeroed again (self-cleaning), so
// no memset launch per call and all kernels on one stream can share it (stream order serialises).
enum class Zeroed : int {
  kBinnedHist = 1,          // K4
  kBinnedSlab = 2,          // K4
  kRowSumsPartials = 3,     // K5b
  kRadixGroups = 4,         // K3a
  kFidCovZeros = 6,         // K8
  kRetrievalCounts = 7,     // K10b
  kMomentsTickets = 8,      // K5 v2
  kRowSumsTickets = 9,      // K5b
  // the onesweep header, whose word 8 is the look-back timeout flag.  Shared on purpose by four
  // users that must see the same buffer: sort_desc writes it, auc_scan and rank_corr read the
  // flag on the device (AucScanArgs / RankCorrArgs::sort_fault) and sort_desc_timeouts reads /
  // clears it from the host
  kOnesweepHeader = 10,
  kOnesweepStatus = 11,     // K3a
  kOnesweepGroups = 12,     // K3a
  kFoldCells = 16,          // tea_fold.h: K1, K2
};

// Uninitialised: kernels overwrite it before reading.
enum class Scratch : int {
  kFidCovSplit = 0,         // K8
  kRetrievalRecords = 1,    // K10b
  kSymEig = 3,              // K9b
  kMomentsPartials = 8,     // K5 v2
  kTrapzPartials = 13,      // K3t
  kSsimPartials = 14,       // K12
  kNdcgPartials = 15,       // K13
  kRankCorrPartials = 16,   // K14
  kCalibrationPartials = 17,  // K15
  kCorrcoefPartials = 18,   // K16
  kSegmentationPartials = 19,  // K17
  kKlDivPartials = 20,      // K18
  kInceptionPartials = 21,  // K21
};

// `capacity`, when given, receives the buffer's size in bytes (>= bytes)
void* workspace(const Tensor& like, hipStream_t stream, int64_t bytes, bool zeroed, int slot, int64_t* capacity);

inline void* zeroed_workspace(const Tensor& like, hipStream_t stream, int64_t bytes, Zeroed slot,
                              int64_t* capacity = nullptr) {
  return workspace(like, stream, bytes, true, static_cast<int>(slot), capacity);
}

inline void* scratch_workspace(const Tensor& like, hipStream_t stream, int64_t bytes, Scratch slot) {
  return workspace(like, stream, bytes, false, static_cast<int>(slot), nullptr);
}

// the 16 * kFoldCells u64 cells of tea_fold.h
inline unsigned long long* fold_workspace(const Tensor& like, hipStream_t stream) {
  return static_cast<unsigned long long*>(
      zeroed_workspace(like, stream, 16 * tea::kFoldCells * 8, Zeroed::kFoldCells));
}

// ---------------------------------------------------------------- dispatcher registration
// Meta kernel of an op that only writes into its arguments: the same parameter list, empty body.
//   m.impl("x", &MetaNoop<&x>::call)
template <auto F>
struct MetaNoop;
template <typename... A, void (*F)(A...)>
struct MetaNoop<F> {
  static void call(A...) {}
};

}  // namespace tea_torch
