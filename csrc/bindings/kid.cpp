// K20 Kernel Inception Distance (csrc/kernels/kid.hip): dispatcher ops only, in a namespace of
// their own and without pybind entries, because the attributes of `_C` and the `torcheval_amd::`
// ops are recorded in tests/golden/native_api.json and that fixture stays byte for byte what it was
// (as K14-K19's ops).  Eager and compiled calls both take the dispatcher (ops/kid.py);
// tests/metrics/image/test_kid.py pins the schemas, the dispatch keys and the Meta kernels.
#include <ATen/ATen.h>
#include <torch/library.h>

#include "tea_kernels.h"
#include "tea_torch.h"

namespace {

using namespace tea_torch;

// partials[S, kid_items(m)] (float64) <- per tile of the three Gram blocks of every subset, the sum
// of (gamma <a, b> + coef)^degree over the pairs it counts.  idx_r / idx_f are [S, m] int32 rows of
// `real` / `fake`; indices in [0, n) are the caller's precondition (the kernel clamps).  One launch
void kid_gram(const Tensor& real, const Tensor& fake, const Tensor& idx_r, const Tensor& idx_f, double gamma,
              double coef, int64_t degree, const Tensor& partials) {
  check_features(real, "kid_gram", "real");
  check_features(fake, "kid_gram", "fake");
  TORCH_CHECK(fake.device() == real.device() && fake.size(1) == real.size(1),
              "kid_gram: real and fake must share their device and feature width");
  TORCH_CHECK(idx_r.scalar_type() == at::kInt && idx_r.is_contiguous() && idx_r.dim() == 2 && idx_r.size(0) >= 1 &&
                  idx_r.size(1) >= 2 && idx_r.device() == real.device(),
              "kid_gram: idx_r must be a contiguous int32 [subsets >= 1, m >= 2] tensor on the inputs' device");
  TORCH_CHECK(idx_f.scalar_type() == at::kInt && idx_f.is_contiguous() && idx_f.sizes() == idx_r.sizes() &&
                  idx_f.device() == real.device(),
              "kid_gram: idx_f must be a contiguous int32 tensor of idx_r's shape on the inputs' device");
  TORCH_CHECK(degree >= 1 && degree <= 16, "kid_gram: degree must be in 1 .. 16, got ", degree);
  const int64_t subsets = idx_r.size(0), m = idx_r.size(1);
  TORCH_CHECK(m < (int64_t{1} << 24) && subsets * tea::kid_items(m) < (int64_t{1} << 31) - 8,
              "kid_gram: too many tiles (subsets x tiles per subset must stay below 2^31)");
  TORCH_CHECK(real.size(0) < (int64_t{1} << 31) && fake.size(0) < (int64_t{1} << 31) &&
                  real.size(1) < (int64_t{1} << 31) - 64,
              "kid_gram: rows and features below 2^31");
  DeviceGuard guard(real.device());
  tea::KidGramArgs a;
  a.real = real.data_ptr<float>();
  a.fake = fake.data_ptr<float>();
  a.real_stride = real.stride(0);
  a.fake_stride = fake.stride(0);
  a.n_r = real.size(0);
  a.n_f = fake.size(0);
  a.d = real.size(1);
  a.idx_r = idx_r.data_ptr<int32_t>();
  a.idx_f = idx_f.data_ptr<int32_t>();
  a.subsets = subsets;
  a.m = m;
  a.gamma = gamma;
  a.coef = coef;
  a.degree = static_cast<int>(degree);
  a.partials = f64_buf(partials, real, subsets * tea::kid_items(m), "kid_gram", "partials");
  check_launch(tea::launch_kid_gram(a, stream_for(real)), "kid_gram");
}

// from kid_gram's partials of subsets of m rows: sums[S, 3] <- sxx, syy, sxy, values[S] <- mmd2
// (both float64), out[2] (float32) <- mean and population standard deviation of values.  One launch
void kid_finish(const Tensor& partials, int64_t m, const Tensor& sums, const Tensor& values, const Tensor& out) {
  check_gpu(partials, "partials");
  TORCH_CHECK(m >= 2 && m < (int64_t{1} << 24) && tea::kid_items(m) < (int64_t{1} << 31),
              "kid_finish: m must be in 2 .. 2^24 - 1");
  TORCH_CHECK(partials.scalar_type() == at::kDouble && partials.is_contiguous() && partials.dim() == 2 &&
                  partials.size(0) >= 1 && partials.size(1) == tea::kid_items(m),
              "kid_finish: partials must be a contiguous float64 [subsets >= 1, tiles per subset] tensor");
  const int64_t subsets = partials.size(0);
  DeviceGuard guard(partials.device());
  tea::KidFinishArgs a;
  a.partials = partials.data_ptr<double>();
  a.subsets = subsets;
  a.m = m;
  a.sums = f64_buf(sums, partials, 3 * subsets, "kid_finish", "sums");
  a.values = f64_buf(values, partials, subsets, "kid_finish", "values");
  a.out = f32_out(out, partials, 2, "out");
  check_launch(tea::launch_kid_finish(a, stream_for(partials)), "kid_finish");
}

}  // namespace

TORCH_LIBRARY(torcheval_amd_kid, m) {
  m.def("kid_gram(Tensor real, Tensor fake, Tensor idx_r, Tensor idx_f, float gamma, float coef, int degree, "
        "Tensor(a!) partials) -> ()");
  m.def("kid_finish(Tensor partials, int m, Tensor(a!) sums, Tensor(b!) values, Tensor(c!) out) -> ()");
}

TORCH_LIBRARY_IMPL(torcheval_amd_kid, CUDA, m) {
  m.impl("kid_gram", &kid_gram);
  m.impl("kid_finish", &kid_finish);
}

TORCH_LIBRARY_IMPL(torcheval_amd_kid, Meta, m) {
  m.impl("kid_gram", &MetaNoop<&kid_gram>::call);
  m.impl("kid_finish", &MetaNoop<&kid_finish>::call);
}
