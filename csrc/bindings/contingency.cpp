// K25 clustering indices of two labelings (csrc/kernels/contingency.hip): dispatcher ops only, in a
// namespace of their own and without pybind entries, because the attributes of `_C` and the
// `torcheval_amd::` ops are recorded in tests/golden/native_api.json and that fixture stays byte for
// byte what it was (as K14-K24's ops).  Eager and compiled calls both take the dispatcher
// (ops/contingency.py); tests/metrics/clustering/test_contingency.py pins the schemas, the dispatch
// keys and the Meta kernels.
#include <ATen/ATen.h>
#include <torch/library.h>

#include "tea_kernels.h"
#include "tea_torch.h"

namespace {

using namespace tea_torch;

void check_table_shape(int64_t r, int64_t c, const char* what) {
  TORCH_CHECK(r >= 1 && c >= 1 && r <= tea::kCtgMaxCells && c <= tea::kCtgMaxCells && r * c <= tea::kCtgMaxCells, what,
              ": the table must be [R >= 1, C >= 1] with R * C <= ", tea::kCtgMaxCells);
}

long long* i64_buf(const Tensor& t, const Tensor& ref, int64_t numel, const char* what, const char* name) {
  return static_cast<long long*>(dense_buf(t, at::kLong, ref, numel, what, name));
}

const void* labels_of(const Tensor& t, const Tensor& ref, int64_t n, const char* name) {
  TORCH_CHECK((t.scalar_type() == at::kLong || t.scalar_type() == at::kInt) && t.dim() == 1 && t.size(0) == n &&
                  t.is_contiguous() && t.device() == ref.device(),
              "contingency_update: ", name, " must be a contiguous int64 / int32 [N] tensor on the table's device");
  return t.data_ptr();
}

// table[R, C] (int64) += the counts of the label pairs; `slice` is the slice size (kCtgSliceSmall or
// kCtgSliceLarge) and `groups` the sample groups of the grid (ops/contingency.py, plan); err |= 1
// when a label lies outside its range
void contingency_update(const Tensor& labels_true, const Tensor& labels_pred, int64_t slice, int64_t groups,
                        const Tensor& table, const optional<Tensor>& err) {
  check_gpu(table, "table");
  TORCH_CHECK(table.dim() == 2, "contingency_update: table must be [R, C]");
  tea::ContingencyCountArgs a;
  a.r = table.size(0);
  a.c = table.size(1);
  check_table_shape(a.r, a.c, "contingency_update");
  a.table = i64_buf(table, table, a.r * a.c, "contingency_update", "table");
  a.n = labels_true.dim() == 1 ? labels_true.size(0) : -1;
  TORCH_CHECK(a.n >= 0 && a.n < (int64_t{1} << 31), "contingency_update: labels must be [N < 2^31]");
  a.labels_true = labels_of(labels_true, table, a.n, "labels_true");
  a.labels_pred = labels_of(labels_pred, table, a.n, "labels_pred");
  a.true_dt = dt_of(labels_true);
  a.pred_dt = dt_of(labels_pred);
  TORCH_CHECK(slice == tea::kCtgSliceSmall || slice == tea::kCtgSliceLarge, "contingency_update: slice must be ",
              tea::kCtgSliceSmall, " or ", tea::kCtgSliceLarge, ", got ", slice);
  const int64_t slices = (a.r * a.c + slice - 1) / slice;
  TORCH_CHECK(groups >= 1 && slices * groups <= tea::kCtgMaxBlocks, "contingency_update: ", slices, " slices times ",
              groups, " groups must be within 1 .. ", tea::kCtgMaxBlocks, " blocks");
  a.slice = static_cast<int>(slice);
  a.groups = static_cast<int>(groups);
  a.err = err_ptr(err, table, "contingency_update");
  DeviceGuard guard(table.device());
  check_launch(tea::launch_contingency_count(a, stream_for(table)), "contingency_update");
}

// From table[R, C]: marginals [R + C + kCtgInts] (int64, zero on entry: row sums, column sums, then
// the exact pair sums, N and the numbers of non-empty rows and columns), cell_partials
// [contingency_stats_blocks], margin_partials [2, contingency_margin_blocks] and margin_logs
// [2, R + C] (float64).  Two launches.
void contingency_stats(const Tensor& table, const Tensor& marginals, const Tensor& cell_partials,
                       const Tensor& margin_partials, const Tensor& margin_logs) {
  check_gpu(table, "table");
  TORCH_CHECK(table.dim() == 2, "contingency_stats: table must be [R, C]");
  tea::ContingencyStatsArgs a;
  a.r = table.size(0);
  a.c = table.size(1);
  check_table_shape(a.r, a.c, "contingency_stats");
  const int64_t m = a.r + a.c;
  a.table = i64_buf(table, table, a.r * a.c, "contingency_stats", "table");
  a.marginals = i64_buf(marginals, table, m + tea::kCtgInts, "contingency_stats", "marginals");
  a.ints = reinterpret_cast<unsigned long long*>(a.marginals + m);
  a.cell_partials =
      f64_buf(cell_partials, table, tea::contingency_stats_blocks(a.r, a.c), "contingency_stats", "cell_partials");
  a.margin_partials = f64_buf(margin_partials, table, 2 * tea::contingency_margin_blocks(a.r, a.c),
                              "contingency_stats", "margin_partials");
  a.margin_logs = f64_buf(margin_logs, table, 2 * m, "contingency_stats", "margin_logs");
  DeviceGuard guard(table.device());
  check_launch(tea::launch_contingency_stats(a, stream_for(table)), "contingency_stats");
}

// emi_partials [2, contingency_emi_blocks(R, C)] (float64) <- per block the sum of the terms of the
// expected mutual information and the sum of their magnitudes
void contingency_emi(const Tensor& marginals, const Tensor& margin_logs, int64_t num_classes, int64_t num_clusters,
                     const Tensor& emi_partials) {
  check_gpu(marginals, "marginals");
  check_table_shape(num_classes, num_clusters, "contingency_emi");
  tea::ContingencyEmiArgs a;
  a.r = num_classes;
  a.c = num_clusters;
  const int64_t m = a.r + a.c;
  a.marginals = i64_buf(marginals, marginals, m + tea::kCtgInts, "contingency_emi", "marginals");
  a.ints = reinterpret_cast<const unsigned long long*>(a.marginals + m);
  a.margin_logs = f64_buf(margin_logs, marginals, 2 * m, "contingency_emi", "margin_logs");
  a.partials =
      f64_buf(emi_partials, marginals, 2 * tea::contingency_emi_blocks(a.r, a.c), "contingency_emi", "emi_partials");
  DeviceGuard guard(marginals.device());
  check_launch(tea::launch_contingency_emi(a, stream_for(marginals)), "contingency_emi");
}

// values [kCtgValues] (float64) <- every index from the statistics; without emi_partials the
// expected mutual information and AMI are NaN
void contingency_values(const Tensor& marginals, const Tensor& cell_partials, const Tensor& margin_partials,
                        const optional<Tensor>& emi_partials, const Tensor& values) {
  check_gpu(marginals, "marginals");
  TORCH_CHECK(marginals.scalar_type() == at::kLong && marginals.is_contiguous() && marginals.dim() == 1 &&
                  marginals.numel() >= 2 + tea::kCtgInts,
              "contingency_values: marginals must be a contiguous int64 [R + C + ", tea::kCtgInts, "] tensor");
  tea::ContingencyValuesArgs a;
  a.ints = reinterpret_cast<const unsigned long long*>(marginals.data_ptr<int64_t>() + marginals.numel() - tea::kCtgInts);
  TORCH_CHECK(cell_partials.numel() >= 1 && cell_partials.numel() <= tea::kCtgStatsBlocks &&
                  margin_partials.numel() >= 2 && margin_partials.numel() <= 2 * tea::kCtgMarginBlocks &&
                  margin_partials.numel() % 2 == 0,
              "contingency_values: the partials are not those of contingency_stats");
  a.stats_blocks = static_cast<int>(cell_partials.numel());
  a.margin_blocks = static_cast<int>(margin_partials.numel() / 2);
  a.cell_partials = f64_buf(cell_partials, marginals, a.stats_blocks, "contingency_values", "cell_partials");
  a.margin_partials = f64_buf(margin_partials, marginals, 2 * a.margin_blocks, "contingency_values", "margin_partials");
  if (emi_partials.has_value()) {
    TORCH_CHECK(emi_partials->numel() >= 2 && emi_partials->numel() <= 2 * tea::kCtgEmiBlocks &&
                    emi_partials->numel() % 2 == 0,
                "contingency_values: emi_partials are not those of contingency_emi");
    a.emi_blocks = static_cast<int>(emi_partials->numel() / 2);
    a.emi_partials = f64_buf(*emi_partials, marginals, 2 * a.emi_blocks, "contingency_values", "emi_partials");
  }
  a.values = f64_buf(values, marginals, tea::kCtgValues, "contingency_values", "values");
  DeviceGuard guard(marginals.device());
  check_launch(tea::launch_contingency_values(a, stream_for(marginals)), "contingency_values");
}

}  // namespace

TORCH_LIBRARY(torcheval_amd_contingency, m) {
  m.def("contingency_update(Tensor labels_true, Tensor labels_pred, int slice, int groups, Tensor(a!) table, "
        "Tensor(b!)? err) -> ()");
  m.def("contingency_stats(Tensor table, Tensor(a!) marginals, Tensor(b!) cell_partials, Tensor(c!) margin_partials, "
        "Tensor(d!) margin_logs) -> ()");
  m.def("contingency_emi(Tensor marginals, Tensor margin_logs, int num_classes, int num_clusters, "
        "Tensor(a!) emi_partials) -> ()");
  m.def("contingency_values(Tensor marginals, Tensor cell_partials, Tensor margin_partials, Tensor? emi_partials, "
        "Tensor(a!) values) -> ()");
}

TORCH_LIBRARY_IMPL(torcheval_amd_contingency, CUDA, m) {
  m.impl("contingency_update", &contingency_update);
  m.impl("contingency_stats", &contingency_stats);
  m.impl("contingency_emi", &contingency_emi);
  m.impl("contingency_values", &contingency_values);
}

TORCH_LIBRARY_IMPL(torcheval_amd_contingency, Meta, m) {
  m.impl("contingency_update", &MetaNoop<&contingency_update>::call);
  m.impl("contingency_stats", &MetaNoop<&contingency_stats>::call);
  m.impl("contingency_emi", &MetaNoop<&contingency_emi>::call);
  m.impl("contingency_values", &MetaNoop<&contingency_values>::call);
}
