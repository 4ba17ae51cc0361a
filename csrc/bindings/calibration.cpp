// K15 multiclass calibration error (csrc/kernels/calibration.hip): dispatcher ops only, in a
// namespace of their own and without pybind entries, because the attributes of `_C` and the
// `torcheval_amd::` ops are recorded in tests/golden/native_api.json and that fixture stays byte for
// byte what it was (as K14's rank_corr, csrc/bindings/sortscan.cpp).  Eager and compiled calls both
// take the dispatcher (ops/calibration.py); tests/metrics/classification/test_calibration_error.py
// pins the schemas, the dispatch keys and the Meta kernels.
#include <ATen/ATen.h>
#include <torch/library.h>

#include "tea_kernels.h"
#include "tea_torch.h"

namespace {

using namespace tea_torch;

// the checks and the argument block both ops share; `tg` keeps a contiguous copy of the target alive
tea::CalibrationArgs calibration_args(const Tensor& input, const Tensor& target, int64_t n_bins, bool from_logits,
                                      const optional<Tensor>& err, Tensor& tg, const char* what) {
  check_gpu(input, "input");
  TORCH_CHECK(input.dim() == 2 && target.dim() == 1 && target.size(0) == input.size(0) &&
                  target.device() == input.device(),
              what, ": input must be [n, c] and target [n], on one device");
  const int64_t c = input.size(1);
  TORCH_CHECK(c >= 1 && c < (int64_t{1} << 31), what, ": 1 .. 2^31 - 1 columns, got ", c);
  TORCH_CHECK(c == 1 || input.stride(1) == 1, what, ": input needs a unit column stride");
  const auto st = input.scalar_type();
  TORCH_CHECK(st == at::kFloat || st == at::kHalf || st == at::kBFloat16, what,
              ": scores must be float32, float16 or bfloat16");
  TORCH_CHECK(target.scalar_type() == at::kLong || target.scalar_type() == at::kInt, what,
              ": target must be int64 or int32");
  TORCH_CHECK(n_bins >= 1 && n_bins <= tea::kCalibMaxBins, what, ": 1 .. ", tea::kCalibMaxBins, " bins, got ", n_bins);
  tg = target.is_contiguous() ? target : target.contiguous();
  tea::CalibrationArgs a;
  a.input = input.data_ptr();
  a.in_dt = dt_of(input);
  a.row_stride = input.stride(0);
  a.target = tg.data_ptr();
  a.tg_dt = dt_of(tg);
  a.n = input.size(0);
  a.c = c;
  a.n_bins = static_cast<int>(n_bins);
  a.from_logits = from_logits ? 1 : 0;
  a.err = err_ptr(err, input, what);
  return a;
}

// [blocks, 3, n_bins] partials, then one more triple (the functional's sums)
double* calibration_scratch(const Tensor& input, hipStream_t st, const tea::CalibrationArgs& a) {
  const int64_t triples = tea::calibration_blocks(a.n, a.c) + 1;
  return static_cast<double*>(scratch_workspace(input, st, triples * 3 * a.n_bins * 8, Scratch::kCalibrationPartials));
}

// class update: the three float64 [n_bins] states += the batch's bin counts, correct counts and
// confidence sums.  Two launches, no host synchronisation.
void calibration_update(const Tensor& input, const Tensor& target, int64_t n_bins, bool from_logits,
                        const Tensor& bin_count, const Tensor& correct_sum, const Tensor& conf_sum,
                        const optional<Tensor>& err) {
  Tensor tg;
  tea::CalibrationArgs a = calibration_args(input, target, n_bins, from_logits, err, tg, "calibration_update");
  a.dst[0] = f64_buf(bin_count, input, n_bins, "calibration_update", "bin_count");
  a.dst[1] = f64_buf(correct_sum, input, n_bins, "calibration_update", "correct_sum");
  a.dst[2] = f64_buf(conf_sum, input, n_bins, "calibration_update", "conf_sum");
  a.accumulate = 1;
  if (a.n == 0) return;
  DeviceGuard guard(input.device());
  const hipStream_t st = stream_for(input);
  a.partial = calibration_scratch(input, st, a);
  check_launch(tea::launch_calibration(a, st), "calibration_update");
}

// functional: out (float32 scalar) <- the value of this batch alone; norm 0 l1, 1 max, 2 l2
void calibration_error(const Tensor& input, const Tensor& target, int64_t n_bins, bool from_logits, int64_t norm,
                       const Tensor& out, const optional<Tensor>& err) {
  Tensor tg;
  tea::CalibrationArgs a = calibration_args(input, target, n_bins, from_logits, err, tg, "calibration_error");
  TORCH_CHECK(a.n >= 1, "calibration_error: no rows");
  TORCH_CHECK(norm >= 0 && norm <= 2, "calibration_error: norm must be 0 (l1), 1 (max) or 2 (l2)");
  a.out = f32_out(out, input, 1, "out");
  a.norm = static_cast<int>(norm);
  DeviceGuard guard(input.device());
  const hipStream_t st = stream_for(input);
  a.partial = calibration_scratch(input, st, a);
  double* sums = a.partial + static_cast<int64_t>(tea::calibration_blocks(a.n, a.c)) * 3 * n_bins;
  for (int s = 0; s < 3; ++s) a.dst[s] = sums + s * n_bins;
  check_launch(tea::launch_calibration(a, st), "calibration_error");
}

// compute(): out (float32 scalar) <- the value of the three states, one single-wave launch
void calibration_value(const Tensor& bin_count, const Tensor& correct_sum, const Tensor& conf_sum, int64_t norm,
                       const Tensor& out) {
  check_gpu(bin_count, "bin_count");
  const int64_t n_bins = bin_count.numel();
  TORCH_CHECK(n_bins >= 1 && n_bins < (int64_t{1} << 31), "calibration_value: 1 .. 2^31 - 1 bins");
  TORCH_CHECK(norm >= 0 && norm <= 2, "calibration_value: norm must be 0 (l1), 1 (max) or 2 (l2)");
  const double* n = f64_buf(bin_count, bin_count, n_bins, "calibration_value", "bin_count");
  const double* k = f64_buf(correct_sum, bin_count, n_bins, "calibration_value", "correct_sum");
  const double* f = f64_buf(conf_sum, bin_count, n_bins, "calibration_value", "conf_sum");
  float* o = f32_out(out, bin_count, 1, "out");
  DeviceGuard guard(bin_count.device());
  check_launch(tea::launch_calibration_value(n, k, f, static_cast<int>(n_bins), static_cast<int>(norm), o,
                                             stream_for(bin_count)),
               "calibration_value");
}

}  // namespace

TORCH_LIBRARY(torcheval_amd_calibration, m) {
  m.def("calibration_update(Tensor input, Tensor target, int n_bins, bool from_logits, Tensor(a!) bin_count, "
        "Tensor(b!) correct_sum, Tensor(c!) conf_sum, Tensor(d!)? err) -> ()");
  m.def("calibration_error(Tensor input, Tensor target, int n_bins, bool from_logits, int norm, Tensor(a!) out, "
        "Tensor(b!)? err) -> ()");
  m.def("calibration_value(Tensor bin_count, Tensor correct_sum, Tensor conf_sum, int norm, Tensor(a!) out) -> ()");
}

TORCH_LIBRARY_IMPL(torcheval_amd_calibration, CUDA, m) {
  m.impl("calibration_update", &calibration_update);
  m.impl("calibration_error", &calibration_error);
  m.impl("calibration_value", &calibration_value);
}

TORCH_LIBRARY_IMPL(torcheval_amd_calibration, Meta, m) {
  m.impl("calibration_update", &MetaNoop<&calibration_update>::call);
  m.impl("calibration_error", &MetaNoop<&calibration_error>::call);
  m.impl("calibration_value", &MetaNoop<&calibration_value>::call);
}
