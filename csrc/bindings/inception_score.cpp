// K21 Inception Score (csrc/kernels/inception_score.hip): dispatcher ops only, in a namespace of
// their own and without pybind entries, because the attributes of `_C` and the `torcheval_amd::`
// ops are recorded in tests/golden/native_api.json and that fixture stays byte for byte what it was
// (as K14 to K20).  Eager and compiled calls both take the dispatcher (ops/inception_score.py);
// tests/metrics/image/test_inception_score.py pins the schemas, the dispatch keys and the Meta
// kernels.
#include <ATen/ATen.h>
#include <torch/library.h>

#include "tea_kernels.h"
#include "tea_torch.h"

namespace {

using namespace tea_torch;

// the three states: float64, contiguous, [s, c], [s] and [s] on `ref`'s device; returns s
int64_t check_states(const Tensor& prob_sum, const Tensor& neg_entropy_sum, const Tensor& num_rows, const Tensor& ref,
                     const char* what) {
  for (const Tensor* t : {&prob_sum, &neg_entropy_sum, &num_rows})
    TORCH_CHECK(t->scalar_type() == at::kDouble && t->is_contiguous() && t->device() == ref.device(), what,
                ": the states must be contiguous float64 tensors on the input's device");
  TORCH_CHECK(prob_sum.dim() == 2 && neg_entropy_sum.dim() == 1 && num_rows.dim() == 1 &&
                  neg_entropy_sum.size(0) == prob_sum.size(0) && num_rows.size(0) == prob_sum.size(0),
              what, ": the states must have shapes [splits, c], [splits] and [splits]");
  const int64_t s = prob_sum.size(0);
  TORCH_CHECK(s >= 1 && s <= tea::kInceptionMaxSplits, what, ": 1 .. ", tea::kInceptionMaxSplits, " splits, got ", s);
  return s;
}

// The three states += the softmax column sums, the negative entropies and the number of the rows of
// `logits`, row i into split (first_split + i) mod splits.  Two launches, no host synchronisation.
void inception_update(const Tensor& logits, int64_t first_split, const Tensor& prob_sum, const Tensor& neg_entropy_sum,
                      const Tensor& num_rows) {
  check_gpu(logits, "logits");
  const auto st = logits.scalar_type();
  TORCH_CHECK(st == at::kFloat || st == at::kHalf || st == at::kBFloat16,
              "inception_update: logits must be float32, float16 or bfloat16");
  TORCH_CHECK(logits.dim() == 2, "inception_update: logits must be [n, c]");
  const int64_t n = logits.size(0), c = logits.size(1);
  const int64_t s = check_states(prob_sum, neg_entropy_sum, num_rows, logits, "inception_update");
  TORCH_CHECK(c >= 1 && c <= tea::kInceptionMaxColumns, "inception_update: 1 .. ", tea::kInceptionMaxColumns,
              " columns, got ", c);
  TORCH_CHECK(prob_sum.size(1) == c, "inception_update: prob_sum must be [splits, ", c, "]");
  TORCH_CHECK(first_split >= 0 && first_split < s, "inception_update: first_split must lie in [0, splits)");
  TORCH_CHECK(n < (int64_t{1} << 31), "inception_update: at most 2^31 - 1 rows");
  TORCH_CHECK(c == 1 || logits.stride(1) == 1, "inception_update: logits need a unit stride along the last dimension");
  TORCH_CHECK(n <= 1 || logits.stride(0) >= 0, "inception_update: logits need a non-negative row stride");
  if (n == 0) return;
  tea::InceptionArgs a;
  a.logits = logits.data_ptr();
  a.dt = dt_of(logits);
  a.row_stride = n > 1 ? logits.stride(0) : c;
  a.n = n;
  a.c = static_cast<int>(c);
  a.splits = static_cast<int>(s);
  a.first = static_cast<int>(first_split);
  a.prob_sum = prob_sum.data_ptr<double>();
  a.neg_entropy_sum = neg_entropy_sum.data_ptr<double>();
  a.num_rows = num_rows.data_ptr<double>();
  DeviceGuard guard(logits.device());
  const hipStream_t stream = stream_for(logits);
  const int64_t bytes = s * tea::inception_blocks(n, a.splits, a.c) * (c + 2) * 8;
  a.partial = static_cast<double*>(scratch_workspace(logits, stream, bytes, Scratch::kInceptionPartials));
  check_launch(tea::launch_inception_update(a, stream), "inception_update");
}

// split_log[s] <- the log score of split s (NaN without rows); out[0 .. 2) (float32) <- the mean
// and the population standard deviation of exp(split_log) over the splits with rows.  One launch.
void inception_value(const Tensor& prob_sum, const Tensor& neg_entropy_sum, const Tensor& num_rows,
                     const Tensor& split_log, const Tensor& out) {
  check_gpu(prob_sum, "prob_sum");
  const int64_t s = check_states(prob_sum, neg_entropy_sum, num_rows, prob_sum, "inception_value");
  TORCH_CHECK(prob_sum.size(1) >= 1, "inception_value: prob_sum needs at least one column");
  TORCH_CHECK(split_log.scalar_type() == at::kDouble && split_log.is_contiguous() && split_log.numel() == s &&
                  split_log.device() == prob_sum.device(),
              "inception_value: split_log must be a contiguous float64 [splits] tensor on the states' device");
  float* o = f32_out(out, prob_sum, 2, "out");
  DeviceGuard guard(prob_sum.device());
  check_launch(tea::launch_inception_value(prob_sum.data_ptr<double>(), neg_entropy_sum.data_ptr<double>(),
                                           num_rows.data_ptr<double>(), static_cast<int>(s), prob_sum.size(1),
                                           split_log.data_ptr<double>(), o, stream_for(prob_sum)),
               "inception_value");
}

}  // namespace

TORCH_LIBRARY(torcheval_amd_inception, m) {
  m.def("inception_update(Tensor logits, int first_split, Tensor(a!) prob_sum, Tensor(b!) neg_entropy_sum, "
        "Tensor(c!) num_rows) -> ()");
  m.def("inception_value(Tensor prob_sum, Tensor neg_entropy_sum, Tensor num_rows, Tensor(a!) split_log, "
        "Tensor(b!) out) -> ()");
}

TORCH_LIBRARY_IMPL(torcheval_amd_inception, CUDA, m) {
  m.impl("inception_update", &inception_update);
  m.impl("inception_value", &inception_value);
}

TORCH_LIBRARY_IMPL(torcheval_amd_inception, Meta, m) {
  m.impl("inception_update", &MetaNoop<&inception_update>::call);
  m.impl("inception_value", &MetaNoop<&inception_value>::call);
}
