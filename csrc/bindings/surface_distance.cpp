// K27 Hausdorff / average surface distance (csrc/kernels/surface_distance.hip): a dispatcher op only, in
// a namespace of its own and without a pybind entry, because the attributes of `_C` and the
// `torcheval_amd::` ops are recorded in tests/golden/native_api.json and that fixture stays byte for byte
// what it was (as K14-K26's ops).  Eager and compiled calls both take the dispatcher
// (ops/surface_distance.py); tests/metrics/classification/test_surface_distance.py pins the schema.
#include <ATen/ATen.h>
#include <torch/library.h>

#include "tea_kernels.h"
#include "tea_torch.h"

namespace {

using namespace tea_torch;

bool label_map(const Tensor& t) {
  const auto st = t.scalar_type();
  return st == at::kByte || st == at::kChar || st == at::kShort || st == at::kInt || st == at::kLong;
}

// ``out`` takes the [n, classes] values, column k the class k + class_base; the optional class states
// ([classes] float64) take += the finite values, their number and the number of +inf.  ``mode`` 0 is the
// Hausdorff distance (``quantile`` < 0: the maximum, else percentile / 100), 1 the average surface
// distance; ``both`` takes both directions.  ``g`` (int16), ``d2`` and ``counts`` (int32) and ``partials``
// (float64) are scratch of at least planes * h * w, planes * h * w, planes and planes * 2 elements, with
// planes = n * classes * 2 (ops/surface_distance.py).
void surface_distance(const Tensor& input, const Tensor& target, int64_t classes, int64_t class_base, int64_t mode,
                      double quantile, bool both, const Tensor& g, const Tensor& d2, const Tensor& counts,
                      const Tensor& partials, const optional<Tensor>& out, const optional<Tensor>& value_sum,
                      const optional<Tensor>& num_finite, const optional<Tensor>& num_inf) {
  check_gpu(input, "input");
  TORCH_CHECK(input.dim() == 3 && input.is_contiguous() && label_map(input),
              "surface_distance: input must be a contiguous integer [n, h, w] label map");
  TORCH_CHECK(target.sizes() == input.sizes() && target.is_contiguous() && target.device() == input.device() &&
                  label_map(target),
              "surface_distance: target must be a contiguous integer label map with the shape and device of input");
  const int64_t n = input.size(0), h = input.size(1), w = input.size(2);
  TORCH_CHECK(tea::surface_distance_geometry_ok(n, h, w, classes),
              "surface_distance: unsupported geometry (sides of 1..", tea::kSurfMaxSide, ", 1..",
              tea::kSurfMaxClasses, " classes)");
  TORCH_CHECK(class_base == 0 || class_base == 1, "surface_distance: class_base must be 0 or 1");
  TORCH_CHECK(mode == 0 || mode == 1, "surface_distance: mode must be 0 (Hausdorff) or 1 (average)");
  TORCH_CHECK(!(quantile > 1.0), "surface_distance: quantile must be at most 1 (negative: the maximum)");
  TORCH_CHECK(out.has_value() || value_sum.has_value(), "surface_distance: nothing to write");
  TORCH_CHECK(value_sum.has_value() == num_finite.has_value() && value_sum.has_value() == num_inf.has_value(),
              "surface_distance: pass all three class states or none");
  const int64_t planes = tea::surface_distance_planes(n, classes);
  const auto scratch = [&](const Tensor& t, at::ScalarType st, int64_t numel, const char* name) {
    TORCH_CHECK(t.scalar_type() == st && t.is_contiguous() && t.device() == input.device() && t.numel() >= numel,
                "surface_distance: ", name, " must be a contiguous ", st, " tensor of at least ", numel,
                " elements on the inputs' device");
    return t.data_ptr();
  };
  tea::SurfaceDistanceArgs a;
  a.input = input.data_ptr();
  a.target = target.data_ptr();
  a.in_dt = dt_of(input);
  a.tg_dt = dt_of(target);
  a.n = n;
  a.h = static_cast<int>(h);
  a.w = static_cast<int>(w);
  a.classes = static_cast<int>(classes);
  a.class_base = static_cast<int>(class_base);
  a.mode = static_cast<int>(mode);
  a.quantile = quantile;
  a.both = both ? 1 : 0;
  a.g = static_cast<uint16_t*>(scratch(g, at::kShort, planes * h * w, "g"));
  a.d2 = static_cast<uint32_t*>(scratch(d2, at::kInt, planes * h * w, "d2"));
  a.counts = static_cast<uint32_t*>(scratch(counts, at::kInt, planes, "counts"));
  a.partial = static_cast<double*>(scratch(partials, at::kDouble, planes * 2, "partials"));
  a.out = f32_out(out, input, n * classes, "out");
  if (value_sum.has_value()) {
    a.value_sum = f64_buf(*value_sum, input, classes, "surface_distance", "value_sum");
    a.num_finite = f64_buf(*num_finite, input, classes, "surface_distance", "num_finite");
    a.num_inf = f64_buf(*num_inf, input, classes, "surface_distance", "num_inf");
  }
  DeviceGuard guard(input.device());
  check_launch(tea::launch_surface_distance(a, stream_for(input)), "surface_distance");
}

}  // namespace

TORCH_LIBRARY(torcheval_amd_surface, m) {
  m.def("surface_distance(Tensor input, Tensor target, int classes, int class_base, int mode, float quantile, "
        "bool both, Tensor(a!) g, Tensor(b!) d2, Tensor(c!) counts, Tensor(d!) partials, Tensor(e!)? out, "
        "Tensor(f!)? value_sum, Tensor(g!)? num_finite, Tensor(h!)? num_inf) -> ()");
}

TORCH_LIBRARY_IMPL(torcheval_amd_surface, CUDA, m) { m.impl("surface_distance", &surface_distance); }

TORCH_LIBRARY_IMPL(torcheval_amd_surface, Meta, m) {
  m.impl("surface_distance", &MetaNoop<&surface_distance>::call);
}
