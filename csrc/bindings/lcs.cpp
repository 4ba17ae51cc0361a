// K30 token LCS length and ROUGE-L sums (csrc/kernels/lcs.hip): a dispatcher op only, in a namespace of its
// own and without a pybind entry, because the attributes of `_C` and the `torcheval_amd::` ops are
// recorded in tests/golden/native_api.json and that fixture stays byte for byte what it was (as K14-K29's
// ops).  Eager and compiled calls both take the dispatcher (ops/lcs.py);
// tests/metrics/text/test_token_rouge_l.py pins the schema.
#include <ATen/ATen.h>
#include <torch/library.h>

#include "tea_kernels.h"
#include "tea_torch.h"

namespace {

using namespace tea_torch;

// `out` ([b] int64) takes the length of the longest common subsequence of every pair of rows of the contiguous
// [b, li] `input` and [b, lt] `target`, both int64 or both int32.  A row is its first lengths[b] tokens
// (int64 [b]; clamped to [0, width]; the whole row without the tensor) without the tokens equal to
// `ignore_index`.  With `ignore_index`, `ws_tokens` (the inputs' dtype, at least b * (li + lt) elements)
// and `ws_lengths` (int64, at least 2 * b) are scratch for the compacted rows.  `chunks` is the kernel
// instance: a power of two from tea::lcs_chunks(li, lt) to tea::kLcsMaxChunks.  The four 0-d float64 totals
// (the sums of precision, recall and F-measure over the pairs, and the pairs), all or none, take the batch
// (`accumulate`: +=).
void lcs(const Tensor& input, const Tensor& target, const optional<Tensor>& input_lengths,
         const optional<Tensor>& target_lengths, optional<int64_t> ignore_index, const optional<Tensor>& ws_tokens,
         const optional<Tensor>& ws_lengths, int64_t chunks, const Tensor& out, const optional<Tensor>& precision_sum,
         const optional<Tensor>& recall_sum, const optional<Tensor>& fmeasure_sum, const optional<Tensor>& pairs,
         bool accumulate) {
  check_gpu(input, "input");
  const auto st = input.scalar_type();
  TORCH_CHECK(input.dim() == 2 && input.is_contiguous() && (st == at::kLong || st == at::kInt),
              "lcs: input must be a contiguous int64 or int32 [b, li] tensor");
  TORCH_CHECK(target.dim() == 2 && target.size(0) == input.size(0) && target.is_contiguous() &&
                  target.device() == input.device() && target.scalar_type() == st,
              "lcs: target must be a contiguous [b, lt] tensor with the rows, dtype and device of input");
  const int64_t b = input.size(0), li = input.size(1), lt = target.size(1);
  TORCH_CHECK(tea::lcs_geometry_ok(b, li, lt), "lcs: at least one pair and widths of at most ",
              tea::kLcsMaxLen, ", got ", b, " pairs of widths ", li, " and ", lt);
  TORCH_CHECK(chunks >= tea::lcs_chunks(li, lt) && chunks <= tea::kLcsMaxChunks && (chunks & (chunks - 1)) == 0,
              "lcs: chunks must be a power of two from ", tea::lcs_chunks(li, lt), " to ", tea::kLcsMaxChunks, ", got ", chunks);
  tea::LcsArgs a;
  a.input = input.data_ptr();
  a.target = target.data_ptr();
  a.wide = st == at::kLong ? 1 : 0;
  a.b = b;
  a.li = li;
  a.lt = lt;
  if (input_lengths.has_value())
    a.input_lengths = static_cast<const int64_t*>(dense_buf(*input_lengths, at::kLong, input, b, "lcs", "input_lengths"));
  if (target_lengths.has_value())
    a.target_lengths = static_cast<const int64_t*>(dense_buf(*target_lengths, at::kLong, input, b, "lcs", "target_lengths"));
  if (ignore_index.has_value()) {
    TORCH_CHECK(ws_tokens.has_value() && ws_lengths.has_value(), "lcs: ignore_index needs both workspaces");
    const auto scratch = [&](const Tensor& t, at::ScalarType dt, int64_t numel, const char* name) {
      TORCH_CHECK(t.scalar_type() == dt && t.is_contiguous() && t.device() == input.device() && t.numel() >= numel,
                  "lcs: ", name, " must be a contiguous ", dt, " tensor of at least ", numel,
                  " elements on the inputs' device");
      return t.data_ptr();
    };
    a.has_ignore = 1;
    a.ignore_index = *ignore_index;
    a.ws_tokens = scratch(*ws_tokens, st, b * (li + lt), "ws_tokens");
    a.ws_lengths = static_cast<int64_t*>(scratch(*ws_lengths, at::kLong, 2 * b, "ws_lengths"));
  }
  a.chunks = static_cast<int>(chunks);
  a.out = static_cast<int64_t*>(dense_buf(out, at::kLong, input, b, "lcs", "out"));
  const optional<Tensor>* totals[4] = {&precision_sum, &recall_sum, &fmeasure_sum, &pairs};
  for (int j = 0; j < 4; ++j) {
    TORCH_CHECK(totals[j]->has_value() == pairs.has_value(), "lcs: the four totals come together or not at all");
    if (pairs.has_value()) a.totals[j] = f64_buf(**totals[j], input, 1, "lcs", "a total");
  }
  a.accumulate = accumulate ? 1 : 0;
  DeviceGuard guard(input.device());
  check_launch(tea::launch_lcs(a, stream_for(input)), "lcs");
}

}  // namespace

TORCH_LIBRARY(torcheval_amd_lcs, m) {
  m.def("lcs(Tensor input, Tensor target, Tensor? input_lengths, Tensor? target_lengths, int? ignore_index, "
        "Tensor(a!)? ws_tokens, Tensor(b!)? ws_lengths, int chunks, Tensor(c!) out, Tensor(d!)? precision_sum, "
        "Tensor(e!)? recall_sum, Tensor(f!)? fmeasure_sum, Tensor(g!)? pairs, bool accumulate) -> ()");
}

TORCH_LIBRARY_IMPL(torcheval_amd_lcs, CUDA, m) { m.impl("lcs", &lcs); }

TORCH_LIBRARY_IMPL(torcheval_amd_lcs, Meta, m) { m.impl("lcs", &MetaNoop<&lcs>::call); }
