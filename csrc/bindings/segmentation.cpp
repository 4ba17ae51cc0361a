// K17 segmentation mean IoU / Dice (csrc/kernels/segmentation.hip): dispatcher ops only, in a
// namespace of their own and without pybind entries, because the attributes of `_C` and the
// `torcheval_amd::` ops are recorded in tests/golden/native_api.json and that fixture stays byte for
// byte what it was (as K15's ops, csrc/bindings/calibration.cpp).  Eager and compiled calls both
// take the dispatcher (ops/segmentation.py); tests/metrics/classification/test_mean_iou.py pins the
// schemas, the dispatch keys and the Meta kernels.
#include <ATen/ATen.h>
#include <torch/library.h>

#include "tea_kernels.h"
#include "tea_torch.h"

namespace {

using namespace tea_torch;

bool integer_map(const Tensor& t) {
  const auto st = t.scalar_type();
  return st == at::kByte || st == at::kChar || st == at::kShort || st == at::kInt || st == at::kLong;
}

// The checks and the argument block both ops share.  `input` is [n, c, p] scores in any strides
// (arm 0: plane, 1: element) or an [n, p] integer map (arm 2), `target` an [n, p] integer map;
// `in` and `tg` keep contiguous copies of the maps alive.
tea::SegmentationArgs segmentation_args(const Tensor& input, const Tensor& target, int64_t num_classes, int64_t arm,
                                        const optional<int64_t>& ignore_index, const optional<Tensor>& err,
                                        Tensor& in, Tensor& tg, const char* what) {
  check_gpu(input, "input");
  TORCH_CHECK(arm >= 0 && arm <= 2, what, ": arm must be 0 (plane), 1 (element) or 2 (label)");
  TORCH_CHECK(num_classes >= 1 && num_classes <= tea::kSegMaxClasses, what, ": 1 .. ", tea::kSegMaxClasses,
              " classes, got ", num_classes);
  TORCH_CHECK(target.dim() == 2 && target.device() == input.device() && integer_map(target), what,
              ": target must be an [n, p] integer map on the input's device");
  tea::SegmentationArgs a;
  if (arm == 2) {
    TORCH_CHECK(input.dim() == 2 && input.sizes() == target.sizes() && integer_map(input), what,
                ": a label-map input must be an integer [n, p] map of the target's shape");
    in = input.is_contiguous() ? input : input.contiguous();
  } else {
    const auto st = input.scalar_type();
    TORCH_CHECK(st == at::kFloat || st == at::kHalf || st == at::kBFloat16, what,
                ": scores must be float32, float16 or bfloat16");
    TORCH_CHECK(input.dim() == 3 && input.size(1) == num_classes && input.size(0) == target.size(0) &&
                    input.size(2) == target.size(1),
                what, ": scores must be [n, num_classes, p] for an [n, p] target");
    in = input;
    a.stride_n = input.stride(0);
    a.stride_c = input.stride(1);
    a.stride_p = input.stride(2);
    const bool wide = st == at::kFloat;
    TORCH_CHECK(arm != 0 || input.size(2) <= 1 || a.stride_p == 1, what, ": the plane arm needs a unit pixel stride");
    TORCH_CHECK(arm != 0 || wide || num_classes == 1 || a.stride_c % 8 == 0, what,
                ": the plane arm needs a class stride of whole 16-B units for 16-bit scores");
  }
  tg = target.is_contiguous() ? target : target.contiguous();
  a.input = in.data_ptr();
  a.in_dt = dt_of(in);
  a.target = tg.data_ptr();
  a.tg_dt = dt_of(tg);
  a.n = target.size(0);
  a.p = target.size(1);
  a.c = static_cast<int>(num_classes);
  a.arm = static_cast<int>(arm);
  a.has_ignore = ignore_index.has_value() ? 1 : 0;
  a.ignore_index = ignore_index.value_or(0);
  a.err = err_ptr(err, input, what);
  return a;
}

// one float64 triple (the functional's sums), then the [blocks, 3, c] u32 partials
double* segmentation_scratch(const Tensor& input, hipStream_t st, tea::SegmentationArgs& a) {
  const int64_t blocks = tea::segmentation_blocks(a.n, a.p);
  const int64_t bytes = int64_t{3} * a.c * 8 + blocks * 3 * a.c * 4;
  char* base = static_cast<char*>(scratch_workspace(input, st, bytes, Scratch::kSegmentationPartials));
  a.partial = reinterpret_cast<uint32_t*>(base + int64_t{3} * a.c * 8);
  return reinterpret_cast<double*>(base);
}

// class update: the three float64 [num_classes] states += the batch's counts.  Two launches, no
// host synchronisation.
void segmentation_update(const Tensor& input, const Tensor& target, int64_t num_classes, int64_t arm,
                         optional<int64_t> ignore_index, const Tensor& intersection, const Tensor& pred_count,
                         const Tensor& target_count, const optional<Tensor>& err) {
  Tensor in, tg;
  tea::SegmentationArgs a =
      segmentation_args(input, target, num_classes, arm, ignore_index, err, in, tg, "segmentation_update");
  a.dst[0] = f64_buf(intersection, input, num_classes, "segmentation_update", "intersection");
  a.dst[1] = f64_buf(pred_count, input, num_classes, "segmentation_update", "pred_count");
  a.dst[2] = f64_buf(target_count, input, num_classes, "segmentation_update", "target_count");
  a.accumulate = 1;
  if (a.n == 0 || a.p == 0) return;
  DeviceGuard guard(input.device());
  const hipStream_t st = stream_for(input);
  segmentation_scratch(input, st, a);
  check_launch(tea::launch_segmentation(a, st), "segmentation_update");
}

// functional: out (float32, one value or [num_classes]) <- the value of this batch alone;
// average 0 macro, 1 micro, 2 none
void segmentation_batch(const Tensor& input, const Tensor& target, int64_t num_classes, int64_t arm,
                        optional<int64_t> ignore_index, bool dice, int64_t average, const Tensor& out,
                        const optional<Tensor>& err) {
  Tensor in, tg;
  tea::SegmentationArgs a =
      segmentation_args(input, target, num_classes, arm, ignore_index, err, in, tg, "segmentation_batch");
  TORCH_CHECK(a.n >= 1 && a.p >= 1, "segmentation_batch: no pixels");
  TORCH_CHECK(average >= 0 && average <= 2, "segmentation_batch: average must be 0 (macro), 1 (micro) or 2 (none)");
  a.out = f32_out(out, input, average == 2 ? num_classes : 1, "out");
  a.dice = dice ? 1 : 0;
  a.average = static_cast<int>(average);
  DeviceGuard guard(input.device());
  const hipStream_t st = stream_for(input);
  double* sums = segmentation_scratch(input, st, a);
  for (int s = 0; s < 3; ++s) a.dst[s] = sums + s * num_classes;
  check_launch(tea::launch_segmentation(a, st), "segmentation_batch");
}

// compute(): out <- the value of the three states, one single-wave launch
void segmentation_value(const Tensor& intersection, const Tensor& pred_count, const Tensor& target_count, bool dice,
                        int64_t average, const Tensor& out) {
  check_gpu(intersection, "intersection");
  const int64_t c = intersection.numel();
  TORCH_CHECK(c >= 1, "segmentation_value: at least one class");
  TORCH_CHECK(average >= 0 && average <= 2, "segmentation_value: average must be 0 (macro), 1 (micro) or 2 (none)");
  const double* i = f64_buf(intersection, intersection, c, "segmentation_value", "intersection");
  const double* p = f64_buf(pred_count, intersection, c, "segmentation_value", "pred_count");
  const double* t = f64_buf(target_count, intersection, c, "segmentation_value", "target_count");
  float* o = f32_out(out, intersection, average == 2 ? c : 1, "out");
  DeviceGuard guard(intersection.device());
  check_launch(tea::launch_segmentation_value(i, p, t, c, dice ? 1 : 0, static_cast<int>(average), o,
                                              stream_for(intersection)),
               "segmentation_value");
}

}  // namespace

TORCH_LIBRARY(torcheval_amd_segmentation, m) {
  m.def("segmentation_update(Tensor input, Tensor target, int num_classes, int arm, int? ignore_index, "
        "Tensor(a!) intersection, Tensor(b!) pred_count, Tensor(c!) target_count, Tensor(d!)? err) -> ()");
  m.def("segmentation_batch(Tensor input, Tensor target, int num_classes, int arm, int? ignore_index, bool dice, "
        "int average, Tensor(a!) out, Tensor(b!)? err) -> ()");
  m.def("segmentation_value(Tensor intersection, Tensor pred_count, Tensor target_count, bool dice, int average, "
        "Tensor(a!) out) -> ()");
}

TORCH_LIBRARY_IMPL(torcheval_amd_segmentation, CUDA, m) {
  m.impl("segmentation_update", &segmentation_update);
  m.impl("segmentation_batch", &segmentation_batch);
  m.impl("segmentation_value", &segmentation_value);
}

TORCH_LIBRARY_IMPL(torcheval_amd_segmentation, Meta, m) {
  m.impl("segmentation_update", &MetaNoop<&segmentation_update>::call);
  m.impl("segmentation_batch", &MetaNoop<&segmentation_batch>::call);
  m.impl("segmentation_value", &MetaNoop<&segmentation_value>::call);
}
