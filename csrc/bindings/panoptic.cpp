// K28 panoptic quality (csrc/kernels/panoptic.hip): dispatcher ops only, in a namespace of their own and
// without pybind entries, because the attributes of `_C` and the `torcheval_amd::` ops are recorded in
// tests/golden/native_api.json and that fixture stays byte for byte what it was (as K14-K27's ops).
// Eager and compiled calls both take the dispatcher (ops/panoptic.py);
// tests/metrics/classification/test_panoptic_quality.py pins the schemas.
#include <ATen/ATen.h>
#include <torch/library.h>

#include "tea_kernels.h"
#include "tea_torch.h"

namespace {

using namespace tea_torch;

// The four [k] float64 `states` (iou_sum, true_positives, false_positives, false_negatives) take the
// batch (`accumulate`: +=).  `input` and `target` are contiguous [n, p, 2] (category, instance) maps, both
// int64 or both int32; `table` is the [2, k] int64 class table (the category ids ascending, then 1 for a
// thing class and 0 for stuff).  `ws_keys` (int64), `ws_counts` and `ws_heads` (int32) are scratch of at
// least spans * 2 * kPanSpan, spans * kPanSpan and spans elements with spans = n * ceil(p / kPanSpan);
// `part_iou` (int64) and `part_counts` (int32) of at least n * k and n * 3 * k (ops/panoptic.py).
// `flag` takes the kPanFlag* bits.  `out`, when given, takes (PQ, SQ, RQ) of the states after the batch:
// [3], or [k, 3] for `per_class`.
void panoptic_quality(const Tensor& input, const Tensor& target, const Tensor& table, bool allow_unknown,
                      const Tensor& ws_keys, const Tensor& ws_counts, const Tensor& ws_heads, const Tensor& part_iou,
                      const Tensor& part_counts, const Tensor& flag, const Tensor& iou_sum, const Tensor& tp,
                      const Tensor& fp, const Tensor& fn, bool accumulate, bool per_class,
                      const optional<Tensor>& out) {
  check_gpu(input, "input");
  const auto st = input.scalar_type();
  TORCH_CHECK(input.dim() == 3 && input.size(2) == 2 && input.is_contiguous() && (st == at::kLong || st == at::kInt),
              "panoptic_quality: input must be a contiguous int64 or int32 [n, p, 2] map");
  TORCH_CHECK(target.sizes() == input.sizes() && target.is_contiguous() && target.device() == input.device() &&
                  target.scalar_type() == st,
              "panoptic_quality: target must be a contiguous map with the shape, dtype and device of input");
  const int64_t n = input.size(0), p = input.size(1);
  TORCH_CHECK(p < (int64_t{1} << 31), "panoptic_quality: fewer than 2^31 pixels per image");
  TORCH_CHECK(table.dim() == 2 && table.size(0) == 2 && table.size(1) >= 1 && table.size(1) <= tea::kPanMaxClasses,
              "panoptic_quality: table must be [2, k] with 1 .. ", tea::kPanMaxClasses, " classes");
  const int64_t k = table.size(1), spans = tea::panoptic_spans(n, p);
  const auto scratch = [&](const Tensor& t, at::ScalarType dt, int64_t numel, const char* name) {
    TORCH_CHECK(t.scalar_type() == dt && t.is_contiguous() && t.device() == input.device() && t.numel() >= numel,
                "panoptic_quality: ", name, " must be a contiguous ", dt, " tensor of at least ", numel,
                " elements on the inputs' device");
    return t.data_ptr();
  };
  tea::PanopticArgs a;
  a.input = input.data_ptr();
  a.target = target.data_ptr();
  a.wide = st == at::kLong ? 1 : 0;
  a.n = n;
  a.p = p;
  a.table = static_cast<const int64_t*>(dense_buf(table, at::kLong, input, 2 * k, "panoptic_quality", "table"));
  a.k = static_cast<int>(k);
  a.allow_unknown = allow_unknown ? 1 : 0;
  a.ws_keys = static_cast<unsigned long long*>(scratch(ws_keys, at::kLong, spans * 2 * tea::kPanSpan, "ws_keys"));
  a.ws_counts = static_cast<uint32_t*>(scratch(ws_counts, at::kInt, spans * tea::kPanSpan, "ws_counts"));
  a.ws_heads = static_cast<uint32_t*>(scratch(ws_heads, at::kInt, spans, "ws_heads"));
  a.part_iou = static_cast<unsigned long long*>(scratch(part_iou, at::kLong, n * k, "part_iou"));
  a.part_counts = static_cast<uint32_t*>(scratch(part_counts, at::kInt, n * 3 * k, "part_counts"));
  a.flag = static_cast<int*>(dense_buf(flag, at::kInt, input, 1, "panoptic_quality", "flag"));
  a.dst[0] = f64_buf(iou_sum, input, k, "panoptic_quality", "iou_sum");
  a.dst[1] = f64_buf(tp, input, k, "panoptic_quality", "true_positives");
  a.dst[2] = f64_buf(fp, input, k, "panoptic_quality", "false_positives");
  a.dst[3] = f64_buf(fn, input, k, "panoptic_quality", "false_negatives");
  a.accumulate = accumulate ? 1 : 0;
  a.per_class = per_class ? 1 : 0;
  a.out = f32_out(out, input, per_class ? 3 * k : 3, "out");
  if (n == 0 || p == 0) return;
  DeviceGuard guard(input.device());
  check_launch(tea::launch_panoptic(a, stream_for(input)), "panoptic_quality");
}

// compute(): out <- (PQ, SQ, RQ) of the four states, one single-wave launch
void panoptic_value(const Tensor& iou_sum, const Tensor& tp, const Tensor& fp, const Tensor& fn, bool per_class,
                    const Tensor& out) {
  check_gpu(iou_sum, "iou_sum");
  const int64_t k = iou_sum.numel();
  TORCH_CHECK(k >= 1, "panoptic_value: at least one class");
  const double* s = f64_buf(iou_sum, iou_sum, k, "panoptic_value", "iou_sum");
  const double* t = f64_buf(tp, iou_sum, k, "panoptic_value", "true_positives");
  const double* p = f64_buf(fp, iou_sum, k, "panoptic_value", "false_positives");
  const double* f = f64_buf(fn, iou_sum, k, "panoptic_value", "false_negatives");
  float* o = f32_out(out, iou_sum, per_class ? 3 * k : 3, "out");
  DeviceGuard guard(iou_sum.device());
  check_launch(tea::launch_panoptic_value(s, t, p, f, k, per_class ? 1 : 0, o, stream_for(iou_sum)), "panoptic_value");
}

}  // namespace

TORCH_LIBRARY(torcheval_amd_panoptic, m) {
  m.def("panoptic_quality(Tensor input, Tensor target, Tensor table, bool allow_unknown, Tensor(a!) ws_keys, "
        "Tensor(b!) ws_counts, Tensor(c!) ws_heads, Tensor(d!) part_iou, Tensor(e!) part_counts, Tensor(f!) flag, "
        "Tensor(g!) iou_sum, Tensor(h!) true_positives, Tensor(i!) false_positives, Tensor(j!) false_negatives, "
        "bool accumulate, bool per_class, Tensor(k!)? out) -> ()");
  m.def("panoptic_value(Tensor iou_sum, Tensor true_positives, Tensor false_positives, Tensor false_negatives, "
        "bool per_class, Tensor(a!) out) -> ()");
}

TORCH_LIBRARY_IMPL(torcheval_amd_panoptic, CUDA, m) {
  m.impl("panoptic_quality", &panoptic_quality);
  m.impl("panoptic_value", &panoptic_value);
}

TORCH_LIBRARY_IMPL(torcheval_amd_panoptic, Meta, m) {
  m.impl("panoptic_quality", &MetaNoop<&panoptic_quality>::call);
  m.impl("panoptic_value", &MetaNoop<&panoptic_value>::call);
}
