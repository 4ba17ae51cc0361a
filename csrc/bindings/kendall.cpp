// K19 Kendall rank correlation (csrc/kernels/kendall.hip): dispatcher ops only, in a namespace of
// their own and without pybind entries, because the attributes of `_C` and the `torcheval_amd::`
// ops are recorded in tests/golden/native_api.json and that fixture stays byte for byte what it was
// (as K14's rank_corr and K16's ops).  Eager and compiled calls both take the dispatcher
// (ops/kendall.py); tests/metrics/regression/test_kendall.py pins the schemas, the dispatch keys
// and the Meta kernels.
#include <ATen/ATen.h>
#include <torch/library.h>

#include "tea_kernels.h"
#include "tea_torch.h"

namespace {

using namespace tea_torch;

// a contiguous [rows, n] tensor of `st` on `ref`'s device
void check_rows(const Tensor& t, const Tensor& ref, at::ScalarType st, const char* what, const char* name) {
  TORCH_CHECK(t.scalar_type() == st && t.is_contiguous() && t.sizes() == ref.sizes() && t.device() == ref.device(),
              what, ": ", name, " must be a contiguous ", st, " [rows, n] tensor on the inputs' device");
}

// the shape both ops share, and the partials and flags that travel from one to the other
void check_state(const Tensor& sorted, const Tensor& part, const Tensor& flags, const char* what) {
  check_gpu(sorted, "sorted");
  TORCH_CHECK(sorted.dim() == 2 && sorted.scalar_type() == at::kFloat && sorted.is_contiguous(), what,
              ": sorted must be contiguous float32 [rows, n]");
  const int64_t rows = sorted.size(0), n = sorted.size(1);
  TORCH_CHECK(n >= 2 && n < (int64_t{1} << 31), what, ": rows of 2 .. 2^31 - 1 samples, got ", n);
  TORCH_CHECK(rows * tea::kendall_tiles(n) < (int64_t{1} << 31), what, ": too many rows");
  TORCH_CHECK(part.scalar_type() == at::kLong && part.is_contiguous() && part.dim() == 3 && part.size(0) == rows &&
                  part.size(1) == 6 && part.size(2) == tea::kendall_tiles(n) && part.device() == sorted.device(),
              what, ": part must be a contiguous int64 [rows, 6, tiles] tensor on the inputs' device");
  TORCH_CHECK(flags.scalar_type() == at::kInt && flags.is_contiguous() && flags.dim() == 2 && flags.size(0) == rows &&
                  flags.size(1) == 2 && flags.device() == sorted.device(),
              what, ": flags must be a contiguous int32 [rows, 2] tensor on the inputs' device");
}

// the timeout word of the onesweep sort that produced `sorted`.  More than 8 rows took the legacy
// passes, which neither set nor clear that word: an older sort's flag is not theirs
const uint32_t* sort_fault_word(const Tensor& sorted, hipStream_t st) {
  if (!tea::radix_onesweep_ok(sorted.size(0), sorted.size(1))) return nullptr;
  return static_cast<const uint32_t*>(zeroed_workspace(sorted, st, 16 * 4, Zeroed::kOnesweepHeader)) + 8;
}

// after K3a sorted `target` descending (sorted, its int32 source permutation `order`): s <- the
// start of each sorted position's tie run, xg <- x[order], and the target's partials and
// NaN flag.  One launch
void kendall_prepare(const Tensor& sorted, const Tensor& order, const Tensor& x, const Tensor& s, const Tensor& xg,
                     const Tensor& part, const Tensor& flags) {
  check_state(sorted, part, flags, "kendall_prepare");
  check_rows(order, sorted, at::kInt, "kendall_prepare", "order");
  check_rows(x, sorted, at::kFloat, "kendall_prepare", "x");
  check_rows(s, sorted, at::kInt, "kendall_prepare", "s");
  check_rows(xg, sorted, at::kFloat, "kendall_prepare", "xg");
  if (sorted.size(0) == 0) return;
  DeviceGuard guard(sorted.device());
  const hipStream_t st = stream_for(sorted);
  tea::KendallPrepareArgs a;
  a.sorted = sorted.data_ptr<float>();
  a.order = order.data_ptr<int32_t>();
  a.x = x.data_ptr<float>();
  a.rows = sorted.size(0);
  a.n = sorted.size(1);
  a.s = s.data_ptr<int32_t>();
  a.xg = xg.data_ptr<float>();
  a.part = part.data_ptr<int64_t>();
  a.flags = flags.data_ptr<int32_t>();
  a.sort_fault = sort_fault_word(sorted, st);
  check_launch(tea::launch_kendall_prepare(a, st), "kendall_prepare");
}

// after K3a sorted kendall_prepare's xg descending with s as its payload (sorted, carried):
// out[rows] (float32) <- tau-b (variant 0) or tau-c (1), counts[rows, 6] (int64) <- n1, n2, n3, Q,
// mx, my.  3 + ceil(log2 tiles) launches, no host synchronisation
void kendall_count(const Tensor& sorted, const Tensor& carried, const Tensor& part, const Tensor& flags,
                   int64_t variant, const Tensor& out, const Tensor& counts) {
  check_state(sorted, part, flags, "kendall_count");
  check_rows(carried, sorted, at::kInt, "kendall_count", "carried");
  TORCH_CHECK(variant == 0 || variant == 1, "kendall_count: variant must be 0 (tau-b) or 1 (tau-c)");
  const int64_t rows = sorted.size(0), n = sorted.size(1);
  TORCH_CHECK(counts.scalar_type() == at::kLong && counts.is_contiguous() && counts.dim() == 2 &&
                  counts.size(0) == rows && counts.size(1) == 6 && counts.device() == sorted.device(),
              "kendall_count: counts must be a contiguous int64 [rows, 6] tensor on the inputs' device");
  float* o = f32_out(out, sorted, rows, "out");
  if (rows == 0) return;
  DeviceGuard guard(sorted.device());
  const hipStream_t st = stream_for(sorted);
  tea::KendallCountArgs a;
  a.sorted = sorted.data_ptr<float>();
  a.carried = carried.data_ptr<int32_t>();
  a.rows = rows;
  a.n = n;
  a.part = part.data_ptr<int64_t>();
  a.flags = flags.data_ptr<int32_t>();
  Tensor ws = at::empty({2, rows, n}, sorted.options().dtype(at::kInt));
  a.buf0 = ws.data_ptr<int32_t>();
  a.buf1 = a.buf0 + rows * n;
  a.sort_fault = sort_fault_word(sorted, st);
  a.variant = static_cast<int>(variant);
  a.out = o;
  a.counts = counts.data_ptr<int64_t>();
  check_launch(tea::launch_kendall_count(a, st), "kendall_count");
}

}  // namespace

TORCH_LIBRARY(torcheval_amd_kendall, m) {
  m.def("kendall_prepare(Tensor sorted, Tensor order, Tensor x, Tensor(a!) s, Tensor(b!) xg, Tensor(c!) part, "
        "Tensor(d!) flags) -> ()");
  m.def("kendall_count(Tensor sorted, Tensor carried, Tensor(a!) part, Tensor(b!) flags, int variant, "
        "Tensor(c!) out, Tensor(d!) counts) -> ()");
}

TORCH_LIBRARY_IMPL(torcheval_amd_kendall, CUDA, m) {
  m.impl("kendall_prepare", &kendall_prepare);
  m.impl("kendall_count", &kendall_count);
}

TORCH_LIBRARY_IMPL(torcheval_amd_kendall, Meta, m) {
  m.impl("kendall_prepare", &MetaNoop<&kendall_prepare>::call);
  m.impl("kendall_count", &MetaNoop<&kendall_count>::call);
}
