// K18 KL divergence (csrc/kernels/kl_divergence.hip): dispatcher ops only, in a namespace of their
// own and without pybind entries, because the attributes of `_C` and the `torcheval_amd::` ops are
// recorded in tests/golden/native_api.json and that fixture stays byte for byte what it was (as
// K14 to K17).  Eager and compiled calls both take the dispatcher (ops/kl_divergence.py);
// tests/metrics/regression/test_kl_divergence.py pins the schemas, the dispatch keys and the Meta
// kernels.
#include <ATen/ATen.h>
#include <torch/library.h>

#include "tea_kernels.h"
#include "tea_torch.h"

namespace {

using namespace tea_torch;

// rows and row stride (elements) of a [..., c] tensor whose leading dimensions flatten to one stride
void flatten_rows(const Tensor& t, const char* what, const char* name, int64_t& rows, int64_t& row_stride) {
  const int64_t d = t.dim();
  rows = 1;
  row_stride = t.size(d - 1);  // any: a single row is never strided over
  bool first = true;
  for (int64_t i = d - 2; i >= 0; --i) {
    if (t.size(i) == 1) continue;
    if (first) row_stride = t.stride(i);
    else TORCH_CHECK(t.stride(i) == rows * row_stride, what, ": the leading dimensions of ", name,
                     " must flatten to one row stride");
    first = false;
    rows *= t.size(i);
  }
  TORCH_CHECK(row_stride >= 0, what, ": ", name, " needs a non-negative row stride");
}

// the checks and the argument block both ops share; `mk` keeps a contiguous copy of the mask alive
tea::KlDivArgs kl_args(const Tensor& input, const Tensor& target, const optional<Tensor>& mask, bool from_logits,
                       Tensor& mk, const char* what) {
  check_gpu(input, "input");
  TORCH_CHECK(input.dim() >= 1 && input.sizes() == target.sizes() && target.device() == input.device(), what,
              ": input and target must have one shape [..., c] and one device");
  const auto st = input.scalar_type();
  TORCH_CHECK((st == at::kFloat || st == at::kHalf || st == at::kBFloat16) && target.scalar_type() == st, what,
              ": both operands must be float32, float16 or bfloat16, and of one dtype");
  const int64_t c = input.size(-1);
  TORCH_CHECK(c >= 1 && c < (int64_t{1} << 31), what, ": 1 .. 2^31 - 1 columns, got ", c);
  TORCH_CHECK(c == 1 || (input.stride(-1) == 1 && target.stride(-1) == 1), what,
              ": both operands need a unit stride along the last dimension");
  tea::KlDivArgs a;
  int64_t tn = 0;
  flatten_rows(input, what, "input", a.n, a.in_row_stride);
  flatten_rows(target, what, "target", tn, a.tg_row_stride);
  a.input = input.data_ptr();
  a.target = target.data_ptr();
  a.dt = dt_of(input);
  a.c = c;
  a.from_logits = from_logits ? 1 : 0;
  const int els = tea::dtype_bytes(a.dt);
  const uintptr_t xi = reinterpret_cast<uintptr_t>(a.input), ti = reinterpret_cast<uintptr_t>(a.target);
  TORCH_CHECK(xi % els == 0 && ti % els == 0 && (xi - ti) % 16 == 0 &&
                  (a.n <= 1 || ((a.in_row_stride - a.tg_row_stride) * els) % 16 == 0),
              what, ": corresponding rows of input and target must lie at one offset from a 16-byte boundary");
  if (mask.has_value()) {
    TORCH_CHECK(mask->scalar_type() == at::kBool && mask->device() == input.device() &&
                    mask->sizes() == input.sizes().slice(0, input.dim() - 1),
                what, ": mask must be a bool tensor of the operands' leading shape on their device");
    mk = mask->is_contiguous() ? *mask : mask->contiguous();
    a.mask = static_cast<const uint8_t*>(mk.data_ptr());
  }
  return a;
}

double* partials(const Tensor& input, hipStream_t st, const tea::KlDivArgs& a) {
  return static_cast<double*>(
      scratch_workspace(input, st, int64_t{2} * tea::kl_divergence_blocks(a.n) * 8, Scratch::kKlDivPartials));
}

// class update: kl_sum += the sum of the counted rows' values, num_rows += their number.  Two
// launches, no host synchronisation.
void kl_update(const Tensor& input, const Tensor& target, const optional<Tensor>& mask, bool from_logits,
               const Tensor& kl_sum, const Tensor& num_rows) {
  Tensor mk;
  tea::KlDivArgs a = kl_args(input, target, mask, from_logits, mk, "kl_update");
  const optional<Tensor> s0(kl_sum), s1(num_rows);
  check_f64_scalar_states({&s0, &s1}, input, "kl_update");
  a.dst_sum = kl_sum.data_ptr<double>();
  a.dst_count = num_rows.data_ptr<double>();
  if (a.n == 0) return;
  DeviceGuard guard(input.device());
  const hipStream_t st = stream_for(input);
  a.partial = partials(input, st, a);
  check_launch(tea::launch_kl_divergence(a, st), "kl_update");
}

// functional: reduction 0 -> out[n] (float32) <- the row values, 0 for uncounted rows; 1 / 2 -> out
// (float32 scalar) <- their sum / mean over the counted rows
void kl_batch(const Tensor& input, const Tensor& target, const optional<Tensor>& mask, bool from_logits,
              int64_t reduction, const Tensor& out) {
  Tensor mk;
  tea::KlDivArgs a = kl_args(input, target, mask, from_logits, mk, "kl_batch");
  TORCH_CHECK(reduction >= 0 && reduction <= 2, "kl_batch: reduction must be 0 (none), 1 (sum) or 2 (mean)");
  TORCH_CHECK(a.n >= 1, "kl_batch: no rows");
  DeviceGuard guard(input.device());
  const hipStream_t st = stream_for(input);
  if (reduction == 0) {
    a.rows_out = f32_out(out, input, a.n, "out");
  } else {
    a.out = f32_out(out, input, 1, "out");
    a.mean = reduction == 2 ? 1 : 0;
    a.partial = partials(input, st, a);
  }
  check_launch(tea::launch_kl_divergence(a, st), "kl_batch");
}

}  // namespace

TORCH_LIBRARY(torcheval_amd_kldiv, m) {
  m.def("kl_update(Tensor input, Tensor target, Tensor? mask, bool from_logits, Tensor(a!) kl_sum, "
        "Tensor(b!) num_rows) -> ()");
  m.def("kl_batch(Tensor input, Tensor target, Tensor? mask, bool from_logits, int reduction, Tensor(a!) out) -> ()");
}

TORCH_LIBRARY_IMPL(torcheval_amd_kldiv, CUDA, m) {
  m.impl("kl_update", &kl_update);
  m.impl("kl_batch", &kl_batch);
}

TORCH_LIBRARY_IMPL(torcheval_amd_kldiv, Meta, m) {
  m.impl("kl_update", &MetaNoop<&kl_update>::call);
  m.impl("kl_batch", &MetaNoop<&kl_batch>::call);
}
