// K29 token edit distance (csrc/kernels/edit_distance.hip): a dispatcher op only, in a namespace of its
// own and without a pybind entry, because the attributes of `_C` and the `torcheval_amd::` ops are
// recorded in tests/golden/native_api.json and that fixture stays byte for byte what it was (as K14-K28's
// ops).  Eager and compiled calls both take the dispatcher (ops/edit_distance.py);
// tests/metrics/text/test_token_edit_distance.py pins the schema.
#include <ATen/ATen.h>
#include <torch/library.h>

#include "tea_kernels.h"
#include "tea_torch.h"

namespace {

using namespace tea_torch;

// `out` ([b] int64) takes the unit-cost Levenshtein distance of every pair of rows of the contiguous
// [b, li] `input` and [b, lt] `target`, both int64 or both int32.  A row is its first lengths[b] tokens
// (int64 [b]; clamped to [0, width]; the whole row without the tensor) without the tokens equal to
// `ignore_index`.  With `ignore_index`, `ws_tokens` (the inputs' dtype, at least b * (li + lt) elements)
// and `ws_lengths` (int64, at least 2 * b) are scratch for the compacted rows.  `arm` is tea::kEditArm*.
// The four 0-d float64 totals (errors, input_total, target_total, max_total), all or none, take the
// batch (`accumulate`: +=).
void edit_distance(const Tensor& input, const Tensor& target, const optional<Tensor>& input_lengths,
                   const optional<Tensor>& target_lengths, optional<int64_t> ignore_index,
                   const optional<Tensor>& ws_tokens, const optional<Tensor>& ws_lengths, int64_t arm,
                   const Tensor& out, const optional<Tensor>& errors, const optional<Tensor>& input_total,
                   const optional<Tensor>& target_total, const optional<Tensor>& max_total, bool accumulate) {
  check_gpu(input, "input");
  const auto st = input.scalar_type();
  TORCH_CHECK(input.dim() == 2 && input.is_contiguous() && (st == at::kLong || st == at::kInt),
              "edit_distance: input must be a contiguous int64 or int32 [b, li] tensor");
  TORCH_CHECK(target.dim() == 2 && target.size(0) == input.size(0) && target.is_contiguous() &&
                  target.device() == input.device() && target.scalar_type() == st,
              "edit_distance: target must be a contiguous [b, lt] tensor with the rows, dtype and device of input");
  const int64_t b = input.size(0), li = input.size(1), lt = target.size(1);
  TORCH_CHECK(tea::edit_distance_geometry_ok(b, li, lt), "edit_distance: at least one pair and widths of at most ",
              tea::kEditMaxLen, ", got ", b, " pairs of widths ", li, " and ", lt);
  TORCH_CHECK(arm == tea::kEditArmWave || arm == tea::kEditArmBlock, "edit_distance: arm must be 0 (wave) or 1 (block)");
  tea::EditDistanceArgs a;
  a.input = input.data_ptr();
  a.target = target.data_ptr();
  a.wide = st == at::kLong ? 1 : 0;
  a.b = b;
  a.li = li;
  a.lt = lt;
  if (input_lengths.has_value())
    a.input_lengths = static_cast<const int64_t*>(dense_buf(*input_lengths, at::kLong, input, b, "edit_distance", "input_lengths"));
  if (target_lengths.has_value())
    a.target_lengths = static_cast<const int64_t*>(dense_buf(*target_lengths, at::kLong, input, b, "edit_distance", "target_lengths"));
  if (ignore_index.has_value()) {
    TORCH_CHECK(ws_tokens.has_value() && ws_lengths.has_value(), "edit_distance: ignore_index needs both workspaces");
    const auto scratch = [&](const Tensor& t, at::ScalarType dt, int64_t numel, const char* name) {
      TORCH_CHECK(t.scalar_type() == dt && t.is_contiguous() && t.device() == input.device() && t.numel() >= numel,
                  "edit_distance: ", name, " must be a contiguous ", dt, " tensor of at least ", numel,
                  " elements on the inputs' device");
      return t.data_ptr();
    };
    a.has_ignore = 1;
    a.ignore_index = *ignore_index;
    a.ws_tokens = scratch(*ws_tokens, st, b * (li + lt), "ws_tokens");
    a.ws_lengths = static_cast<int64_t*>(scratch(*ws_lengths, at::kLong, 2 * b, "ws_lengths"));
  }
  a.arm = static_cast<int>(arm);
  a.out = static_cast<int64_t*>(dense_buf(out, at::kLong, input, b, "edit_distance", "out"));
  const optional<Tensor>* totals[4] = {&errors, &input_total, &target_total, &max_total};
  for (int j = 0; j < 4; ++j) {
    TORCH_CHECK(totals[j]->has_value() == errors.has_value(), "edit_distance: the four totals come together or not at all");
    if (errors.has_value()) a.totals[j] = f64_buf(**totals[j], input, 1, "edit_distance", "a total");
  }
  a.accumulate = accumulate ? 1 : 0;
  DeviceGuard guard(input.device());
  check_launch(tea::launch_edit_distance(a, stream_for(input)), "edit_distance");
}

}  // namespace

TORCH_LIBRARY(torcheval_amd_editdist, m) {
  m.def("edit_distance(Tensor input, Tensor target, Tensor? input_lengths, Tensor? target_lengths, int? ignore_index, "
        "Tensor(a!)? ws_tokens, Tensor(b!)? ws_lengths, int arm, Tensor(c!) out, Tensor(d!)? errors, "
        "Tensor(e!)? input_total, Tensor(f!)? target_total, Tensor(g!)? max_total, bool accumulate) -> ()");
}

TORCH_LIBRARY_IMPL(torcheval_amd_editdist, CUDA, m) { m.impl("edit_distance", &edit_distance); }

TORCH_LIBRARY_IMPL(torcheval_amd_editdist, Meta, m) { m.impl("edit_distance", &MetaNoop<&edit_distance>::call); }
