// K16 Pearson / concordance correlation (csrc/kernels/corrcoef.hip): dispatcher ops only, in a
// namespace of their own and without pybind entries, because the attributes of `_C` and the
// `torcheval_amd::` ops are recorded in tests/golden/native_api.json and that fixture stays byte for
// byte what it was (as K14's rank_corr and K15's ops).  Eager and compiled calls both take the
// dispatcher (ops/corrcoef.py); tests/metrics/regression/test_pearson.py pins the schemas, the
// dispatch keys and the Meta kernels.
#include <ATen/ATen.h>
#include <torch/library.h>

#include "tea_kernels.h"
#include "tea_torch.h"

namespace {

using namespace tea_torch;

double* moments_state(const Tensor& t, const Tensor& ref, int64_t tasks, const char* what, const char* name) {
  TORCH_CHECK(t.scalar_type() == at::kDouble && t.is_contiguous() && t.dim() == 2 && t.size(0) == 6 &&
                  t.size(1) == tasks && t.device() == ref.device(),
              what, ": ", name, " must be a contiguous float64 [6, tasks] tensor on the inputs' device");
  return t.data_ptr<double>();
}

bool float_kind(const Tensor& t) {
  const auto st = t.scalar_type();
  return st == at::kFloat || st == at::kHalf || st == at::kBFloat16;
}

// the checks and the argument block both ops share: [tasks, n] operands of equal shapes, either
// both with a unit stride along the samples (row arm) or both transposed views of row-major
// [n, >= tasks] parents (column arm: stride(0) == 1, stride(1) >= tasks); the row arm takes a shape both can
tea::CorrcoefArgs corrcoef_args(const Tensor& input, const Tensor& target, const char* what) {
  check_gpu(input, "input");
  TORCH_CHECK(input.dim() == 2 && target.dim() == 2 && input.sizes() == target.sizes() &&
                  target.device() == input.device(),
              what, ": input and target must be [tasks, n] of equal shapes, on one device");
  TORCH_CHECK(float_kind(input) && float_kind(target), what, ": operands must be float32, float16 or bfloat16");
  const int64_t tasks = input.size(0), n = input.size(1);
  TORCH_CHECK(tasks >= 1 && n >= 1 && n < (int64_t{1} << 31), what, ": tasks >= 1 and 1 <= n < 2^31");
  const bool row = n == 1 || (input.stride(1) == 1 && target.stride(1) == 1);
  const bool col = input.stride(0) == 1 && target.stride(0) == 1 && input.stride(1) >= tasks && target.stride(1) >= tasks;
  TORCH_CHECK(row || col, what, ": operands need a unit stride along the samples, or both the layout of a transposed [n, tasks] tensor");
  tea::CorrcoefArgs a;
  a.x = input.data_ptr();
  a.y = target.data_ptr();
  a.x_dt = dt_of(input);
  a.y_dt = dt_of(target);
  a.tasks = tasks;
  a.n = n;
  a.column = row ? 0 : 1;
  a.x_task_stride = row ? input.stride(0) : 1;
  a.y_task_stride = row ? target.stride(0) : 1;
  a.x_sample_stride = row ? 1 : input.stride(1);
  a.y_sample_stride = row ? 1 : target.stride(1);
  TORCH_CHECK(a.x_task_stride >= 0 && a.y_task_stride >= 0 && a.x_sample_stride >= 0 && a.y_sample_stride >= 0, what,
              ": negative strides");
  return a;
}

void corrcoef_launch(tea::CorrcoefArgs& a, const Tensor& input, const char* what) {
  DeviceGuard guard(input.device());
  const hipStream_t st = stream_for(input);
  const int64_t tuples = a.tasks * tea::corrcoef_blocks(a.n, a.column);
  a.partial = static_cast<double*>(scratch_workspace(input, st, tuples * 5 * 8, Scratch::kCorrcoefPartials));
  check_launch(tea::launch_corrcoef(a, st), what);
}

// class update: moments[6, tasks] <- its pairwise merge with this batch's moments.  Two launches,
// no host synchronisation.
void corrcoef_update(const Tensor& input, const Tensor& target, const Tensor& moments) {
  tea::CorrcoefArgs a = corrcoef_args(input, target, "corrcoef_update");
  a.moments = moments_state(moments, input, a.tasks, "corrcoef_update", "moments");
  corrcoef_launch(a, input, "corrcoef_update");
}

// functional: out[tasks] (float32) <- the value of this batch alone; kind 0 Pearson, 1 concordance
void corrcoef_batch(const Tensor& input, const Tensor& target, int64_t kind, const Tensor& out) {
  tea::CorrcoefArgs a = corrcoef_args(input, target, "corrcoef_batch");
  TORCH_CHECK(kind == 0 || kind == 1, "corrcoef_batch: kind must be 0 (Pearson) or 1 (concordance)");
  a.out = f32_out(out, input, a.tasks, "out");
  a.concordance = static_cast<int>(kind);
  corrcoef_launch(a, input, "corrcoef_batch");
}

// merge_state: moments[6, tasks] <- its pairwise merge with other[6, tasks], one launch
void corrcoef_merge(const Tensor& moments, const Tensor& other) {
  check_gpu(moments, "moments");
  TORCH_CHECK(moments.dim() == 2, "corrcoef_merge: moments must be [6, tasks]");
  const int64_t tasks = moments.size(1);
  TORCH_CHECK(tasks >= 1, "corrcoef_merge: no tasks");
  double* m = moments_state(moments, moments, tasks, "corrcoef_merge", "moments");
  const double* o = moments_state(other, moments, tasks, "corrcoef_merge", "other");
  DeviceGuard guard(moments.device());
  check_launch(tea::launch_corrcoef_merge(m, o, tasks, stream_for(moments)), "corrcoef_merge");
}

// compute(): out[tasks] (float32) <- the value of moments[6, tasks], one launch
void corrcoef_value(const Tensor& moments, int64_t kind, const Tensor& out) {
  check_gpu(moments, "moments");
  TORCH_CHECK(moments.dim() == 2, "corrcoef_value: moments must be [6, tasks]");
  const int64_t tasks = moments.size(1);
  TORCH_CHECK(tasks >= 1, "corrcoef_value: no tasks");
  TORCH_CHECK(kind == 0 || kind == 1, "corrcoef_value: kind must be 0 (Pearson) or 1 (concordance)");
  const double* m = moments_state(moments, moments, tasks, "corrcoef_value", "moments");
  float* o = f32_out(out, moments, tasks, "out");
  DeviceGuard guard(moments.device());
  check_launch(tea::launch_corrcoef_value(m, tasks, static_cast<int>(kind), o, stream_for(moments)), "corrcoef_value");
}

}  // namespace

TORCH_LIBRARY(torcheval_amd_corrcoef, m) {
  m.def("corrcoef_update(Tensor input, Tensor target, Tensor(a!) moments) -> ()");
  m.def("corrcoef_batch(Tensor input, Tensor target, int kind, Tensor(a!) out) -> ()");
  m.def("corrcoef_merge(Tensor(a!) moments, Tensor other) -> ()");
  m.def("corrcoef_value(Tensor moments, int kind, Tensor(a!) out) -> ()");
}

TORCH_LIBRARY_IMPL(torcheval_amd_corrcoef, CUDA, m) {
  m.impl("corrcoef_update", &corrcoef_update);
  m.impl("corrcoef_batch", &corrcoef_batch);
  m.impl("corrcoef_merge", &corrcoef_merge);
  m.impl("corrcoef_value", &corrcoef_value);
}

TORCH_LIBRARY_IMPL(torcheval_amd_corrcoef, Meta, m) {
  m.impl("corrcoef_update", &MetaNoop<&corrcoef_update>::call);
  m.impl("corrcoef_batch", &MetaNoop<&corrcoef_batch>::call);
  m.impl("corrcoef_merge", &MetaNoop<&corrcoef_merge>::call);
  m.impl("corrcoef_value", &MetaNoop<&corrcoef_value>::call);
}
