// K26 multi-scale SSIM (csrc/kernels/msssim.hip): a dispatcher op only, in a namespace of its own and
// without a pybind entry, because the attributes of `_C` and the `torcheval_amd::` ops are recorded in
// tests/golden/native_api.json and that fixture stays byte for byte what it was (as K14-K25's ops).
// Eager and compiled calls both take the dispatcher (ops/msssim.py); the tile constants are K12's
// (`_C.ssim_tile_rows`, `_C.ssim_tile_cols`); tests/metrics/image/test_msssim.py pins the schema.
#include <ATen/ATen.h>
#include <torch/library.h>

#include "tea_kernels.h"
#include "tea_torch.h"

namespace {

using namespace tea_torch;

// ``out`` takes the [n] per-image values, or their mean when ``mean``; the optional class states take
// += sum of the values and += n.  ``workspace`` (float32) and ``partials`` (float64) are scratch of at
// least the sizes of tea::msssim_plan (ops/msssim.py, plan).
void msssim(const Tensor& input, const Tensor& target, at::ArrayRef<double> taps, at::ArrayRef<double> betas,
            double c1, double c2, const Tensor& workspace, const Tensor& partials, const optional<Tensor>& out,
            bool mean, const optional<Tensor>& value_sum, const optional<Tensor>& num_images) {
  check_gpu(input, "input");
  TORCH_CHECK(input.dim() == 4 && input.is_contiguous() && input.numel() > 0,
              "msssim: input must be a contiguous, non-empty [n, c, h, w] tensor");
  TORCH_CHECK(target.sizes() == input.sizes() && target.is_contiguous() && target.device() == input.device() &&
                  target.scalar_type() == input.scalar_type(),
              "msssim: target must be contiguous with the shape, dtype and device of input");
  const auto st = input.scalar_type();
  TORCH_CHECK(st == at::kFloat || st == at::kHalf || st == at::kBFloat16 || st == at::kByte,
              "msssim: inputs must be float32, float16, bfloat16 or uint8");
  const int64_t ks = static_cast<int64_t>(taps.size());
  const int64_t levels = static_cast<int64_t>(betas.size());
  const int64_t n = input.size(0), c = input.size(1), h = input.size(2), w = input.size(3);
  TORCH_CHECK(tea::msssim_geometry_ok(n * c, h, w, ks, levels), "msssim: unsupported geometry (odd window of 3..",
              tea::kSsimMaxKs, " taps no larger than the last of 1..", tea::kMsssimMaxLevels, " levels, at most ",
              tea::kSsimMaxPlanes, " planes)");
  TORCH_CHECK(out.has_value() || value_sum.has_value(), "msssim: nothing to write");
  TORCH_CHECK(value_sum.has_value() == num_images.has_value(), "msssim: pass both class states or neither");
  const tea::MsssimPlan plan = tea::msssim_plan(h, w, ks, levels);
  TORCH_CHECK(workspace.scalar_type() == at::kFloat && workspace.is_contiguous() &&
                  workspace.device() == input.device() && workspace.numel() >= n * c * plan.ws_pairs * 2,
              "msssim: workspace must be a contiguous float32 tensor of at least ", n * c * plan.ws_pairs * 2,
              " elements on the inputs' device");
  TORCH_CHECK(partials.scalar_type() == at::kDouble && partials.is_contiguous() &&
                  partials.device() == input.device() && partials.numel() >= n * c * plan.partials,
              "msssim: partials must be a contiguous float64 tensor of at least ", n * c * plan.partials,
              " elements on the inputs' device");
  tea::MsssimArgs a;
  a.x = input.data_ptr();
  a.y = target.data_ptr();
  a.dt = dt_of(input);
  a.n = n;
  a.c = c;
  a.h = static_cast<int>(h);
  a.w = static_cast<int>(w);
  a.ks = static_cast<int>(ks);
  for (int64_t j = 0; j < ks; ++j) a.taps[j] = static_cast<float>(taps[j]);
  a.c1 = static_cast<float>(c1);
  a.c2 = static_cast<float>(c2);
  a.levels = static_cast<int>(levels);
  for (int64_t j = 0; j < levels; ++j) a.betas[j] = betas[j];
  a.workspace = plan.ws_pairs > 0 ? workspace.data_ptr<float>() : nullptr;
  a.partial = partials.data_ptr<double>();
  a.mean = mean ? 1 : 0;
  a.out = f32_out(out, input, mean ? 1 : n, "out");
  check_f64_scalar_states({&value_sum, &num_images}, input, "msssim");
  if (value_sum.has_value()) {
    a.value_sum = value_sum->data_ptr<double>();
    a.num_images = num_images->data_ptr<double>();
  }
  DeviceGuard guard(input.device());
  check_launch(tea::launch_msssim(a, stream_for(input)), "msssim");
}

}  // namespace

TORCH_LIBRARY(torcheval_amd_msssim, m) {
  m.def("msssim(Tensor input, Tensor target, float[] taps, float[] betas, float c1, float c2, "
        "Tensor(a!) workspace, Tensor(b!) partials, Tensor(c!)? out, bool mean, Tensor(d!)? value_sum, "
        "Tensor(e!)? num_images) -> ()");
}

TORCH_LIBRARY_IMPL(torcheval_amd_msssim, CUDA, m) { m.impl("msssim", &msssim); }

TORCH_LIBRARY_IMPL(torcheval_amd_msssim, Meta, m) { m.impl("msssim", &MetaNoop<&msssim>::call); }
