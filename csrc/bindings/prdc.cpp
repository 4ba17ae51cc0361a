// K22 precision / recall and density / coverage (csrc/kernels/prdc.hip): dispatcher ops only, in a
// namespace of their own and without pybind entries, because the attributes of `_C` and the
// `torcheval_amd::` ops are recorded in tests/golden/native_api.json and that fixture stays byte for
// byte what it was (as K14-K21's ops).  Eager and compiled calls both take the dispatcher
// (ops/prdc.py); tests/metrics/image/test_prdc.py pins the schemas, the dispatch keys and the Meta
// kernels.
#include <ATen/ATen.h>
#include <torch/library.h>

#include "tea_kernels.h"
#include "tea_torch.h"

namespace {

using namespace tea_torch;

// check_features of tea_torch.h, and sizes that the tile kernels index in 32 bits
void check_tile_features(const Tensor& t, const char* what, const char* name) {
  check_features(t, what, name);
  TORCH_CHECK(t.size(0) < (int64_t{1} << 31) - tea::kPrdcTile && t.size(1) < (int64_t{1} << 31) - 64, what, ": ",
              name, " must have fewer than 2^31 - 128 rows and 2^31 - 64 columns");
}

tea::PrdcTileArgs tile_args(const Tensor& query, const Tensor& ref, const Tensor& norms_q, const Tensor& norms_ref,
                            int64_t groups, const char* what) {
  check_tile_features(query, what, "query");
  check_tile_features(ref, what, "ref");
  TORCH_CHECK(ref.device() == query.device() && ref.size(1) == query.size(1), what,
              ": both feature sets must share their device and width");
  TORCH_CHECK(groups >= 0, what, ": groups must be >= 0 (0: the rule of prdc_groups), got ", groups);
  tea::PrdcTileArgs a;
  a.query = query.data_ptr<float>();
  a.ref = ref.data_ptr<float>();
  a.query_stride = query.stride(0);
  a.ref_stride = ref.stride(0);
  a.n_q = query.size(0);
  a.n_ref = ref.size(0);
  a.d = query.size(1);
  a.norms_q = f64_buf(norms_q, query, a.n_q, what, "the query norms");
  a.norms_ref = f64_buf(norms_ref, query, a.n_ref, what, "the reference norms");
  a.groups = static_cast<int>(tea::prdc_groups(a.n_q, a.n_ref, a.d, groups));
  return a;
}

// norms_real[n_r], norms_fake[n_f] (float64) <- the FP64 sums of squares of the rows.  One launch
void prdc_norms(const Tensor& real, const Tensor& fake, const Tensor& norms_real, const Tensor& norms_fake) {
  check_tile_features(real, "prdc_norms", "real");
  check_tile_features(fake, "prdc_norms", "fake");
  TORCH_CHECK(fake.device() == real.device() && fake.size(1) == real.size(1),
              "prdc_norms: real and fake must share their device and feature width");
  DeviceGuard guard(real.device());
  tea::PrdcNormsArgs a;
  a.real = real.data_ptr<float>();
  a.fake = fake.data_ptr<float>();
  a.real_stride = real.stride(0);
  a.fake_stride = fake.stride(0);
  a.n_r = real.size(0);
  a.n_f = fake.size(0);
  a.d = real.size(1);
  a.norms_real = f64_buf(norms_real, real, a.n_r, "prdc_norms", "norms_real");
  a.norms_fake = f64_buf(norms_fake, real, a.n_f, "prdc_norms", "norms_fake");
  check_launch(tea::launch_prdc_norms(a, stream_for(real)), "prdc_norms");
}

// partial[n, 2 G, k] (float64) <- per row and list the k smallest d2 to the other rows of `feats`
// that the list's column tiles hold, ascending, +inf in unfilled slots; G = prdc_groups(n, n, D, groups)
void prdc_knn(const Tensor& feats, const Tensor& norms, int64_t k, int64_t groups, const Tensor& partial) {
  tea::PrdcTileArgs a = tile_args(feats, feats, norms, norms, groups, "prdc_knn");
  TORCH_CHECK(k >= 1 && k <= tea::kPrdcMaxK, "prdc_knn: k must be in 1 .. ", tea::kPrdcMaxK, ", got ", k);
  TORCH_CHECK(partial.dim() == 3 && partial.size(0) == a.n_q && partial.size(1) == 2 * a.groups && partial.size(2) == k,
              "prdc_knn: partial must be [n, 2 G, k] with G = ", a.groups);
  DeviceGuard guard(feats.device());
  a.k = static_cast<int>(k);
  a.partial = f64_buf(partial, feats, a.n_q * 2 * a.groups * k, "prdc_knn", "partial");
  check_launch(tea::launch_prdc_knn(a, stream_for(feats)), "prdc_knn");
}

// radii[n] (float64) <- the k-th smallest value of each row's lists in partial[n, lists, k]
void prdc_radii(const Tensor& partial, const Tensor& radii) {
  check_gpu(partial, "partial");
  TORCH_CHECK(partial.scalar_type() == at::kDouble && partial.is_contiguous() && partial.dim() == 3 &&
                  partial.size(0) >= 1 && partial.size(0) < (int64_t{1} << 31) && partial.size(1) >= 1 &&
                  partial.size(1) < (int64_t{1} << 24) && partial.size(2) >= 1 && partial.size(2) <= tea::kPrdcMaxK,
              "prdc_radii: partial must be a contiguous float64 [n, lists, k <= ", tea::kPrdcMaxK, "] tensor");
  DeviceGuard guard(partial.device());
  double* out = f64_buf(radii, partial, partial.size(0), "prdc_radii", "radii");
  check_launch(tea::launch_prdc_radii(partial.data_ptr<double>(), partial.size(0), static_cast<int>(partial.size(1)),
                                      static_cast<int>(partial.size(2)), out, stream_for(partial)),
               "prdc_radii");
}

// counts[n_q, 2 G] (int32) <- per query row and list the number of reference rows with
// d2 <= radii_ref[col], mins[n_q, 2 G] (float64) <- the smallest d2; G = prdc_groups(n_q, n_ref, D, groups)
void prdc_cross(const Tensor& query, const Tensor& ref, const Tensor& norms_q, const Tensor& norms_ref,
                const Tensor& radii_ref, int64_t groups, const Tensor& counts, const Tensor& mins) {
  tea::PrdcTileArgs a = tile_args(query, ref, norms_q, norms_ref, groups, "prdc_cross");
  DeviceGuard guard(query.device());
  a.radii_ref = f64_buf(radii_ref, query, a.n_ref, "prdc_cross", "radii_ref");
  TORCH_CHECK(counts.dim() == 2 && counts.size(0) == a.n_q && counts.size(1) == 2 * a.groups &&
                  mins.sizes() == counts.sizes(),
              "prdc_cross: counts and mins must be [n_q, 2 G] with G = ", a.groups);
  a.counts = static_cast<uint32_t*>(dense_buf(counts, at::kInt, query, a.n_q * 2 * a.groups, "prdc_cross", "counts"));
  a.mins = f64_buf(mins, query, a.n_q * 2 * a.groups, "prdc_cross", "mins");
  check_launch(tea::launch_prdc_cross(a, stream_for(query)), "prdc_cross");
}

// folds the two cross passes over their lists into hits_* (int32) and nearest_* (float64), adds the
// four int64 tallies and divides them in FP64 into the four float32 values.  Two launches;
// block_tallies is int64 [prdc_hits_blocks(n_r, n_f), 4] scratch
void prdc_finish(const Tensor& counts_fake, const Tensor& mins_fake, const Tensor& counts_real,
                 const Tensor& mins_real, const Tensor& radii_real, int64_t k, const Tensor& block_tallies,
                 const Tensor& hits_real, const Tensor& hits_fake, const Tensor& nearest_real,
                 const Tensor& nearest_fake, const Tensor& tallies, const Tensor& values) {
  check_gpu(counts_fake, "counts_fake");
  TORCH_CHECK(counts_fake.dim() == 2 && counts_real.dim() == 2 && counts_fake.size(0) >= 1 &&
                  counts_real.size(0) >= 1 && counts_fake.size(1) >= 1 && counts_real.size(1) >= 1 &&
                  counts_fake.size(1) < (int64_t{1} << 24) && counts_real.size(1) < (int64_t{1} << 24),
              "prdc_finish: counts_fake and counts_real must be [n, lists] tensors");
  TORCH_CHECK(k >= 1 && k < (int64_t{1} << 31), "prdc_finish: k must be >= 1, got ", k);
  DeviceGuard guard(counts_fake.device());
  const Tensor& ref = counts_fake;
  tea::PrdcFinishArgs a;
  a.n_f = counts_fake.size(0);
  a.n_r = counts_real.size(0);
  a.lists_f = static_cast<int>(counts_fake.size(1));
  a.lists_r = static_cast<int>(counts_real.size(1));
  a.k = static_cast<int>(k);
  a.counts_fake =
      static_cast<uint32_t*>(dense_buf(counts_fake, at::kInt, ref, a.n_f * a.lists_f, "prdc_finish", "counts_fake"));
  a.mins_fake = f64_buf(mins_fake, ref, a.n_f * a.lists_f, "prdc_finish", "mins_fake");
  a.counts_real =
      static_cast<uint32_t*>(dense_buf(counts_real, at::kInt, ref, a.n_r * a.lists_r, "prdc_finish", "counts_real"));
  a.mins_real = f64_buf(mins_real, ref, a.n_r * a.lists_r, "prdc_finish", "mins_real");
  a.radii_real = f64_buf(radii_real, ref, a.n_r, "prdc_finish", "radii_real");
  a.block_tallies = static_cast<int64_t*>(dense_buf(block_tallies, at::kLong, ref,
                                                    4 * tea::prdc_hits_blocks(a.n_r, a.n_f), "prdc_finish",
                                                    "block_tallies"));
  a.hits_real = static_cast<int32_t*>(dense_buf(hits_real, at::kInt, ref, a.n_r, "prdc_finish", "hits_real"));
  a.hits_fake = static_cast<int32_t*>(dense_buf(hits_fake, at::kInt, ref, a.n_f, "prdc_finish", "hits_fake"));
  a.nearest_real = f64_buf(nearest_real, ref, a.n_r, "prdc_finish", "nearest_real");
  a.nearest_fake = f64_buf(nearest_fake, ref, a.n_f, "prdc_finish", "nearest_fake");
  a.tallies = static_cast<int64_t*>(dense_buf(tallies, at::kLong, ref, 4, "prdc_finish", "tallies"));
  a.values = f32_out(values, ref, 4, "values");
  check_launch(tea::launch_prdc_finish(a, stream_for(ref)), "prdc_finish");
}

}  // namespace

TORCH_LIBRARY(torcheval_amd_prdc, m) {
  m.def("prdc_norms(Tensor real, Tensor fake, Tensor(a!) norms_real, Tensor(b!) norms_fake) -> ()");
  m.def("prdc_knn(Tensor feats, Tensor norms, int k, int groups, Tensor(a!) partial) -> ()");
  m.def("prdc_radii(Tensor partial, Tensor(a!) radii) -> ()");
  m.def("prdc_cross(Tensor query, Tensor ref, Tensor norms_q, Tensor norms_ref, Tensor radii_ref, int groups, "
        "Tensor(a!) counts, Tensor(b!) mins) -> ()");
  m.def("prdc_finish(Tensor counts_fake, Tensor mins_fake, Tensor counts_real, Tensor mins_real, Tensor radii_real, "
        "int k, Tensor(a!) block_tallies, Tensor(b!) hits_real, Tensor(c!) hits_fake, Tensor(d!) nearest_real, "
        "Tensor(e!) nearest_fake, Tensor(f!) tallies, Tensor(g!) values) -> ()");
}

TORCH_LIBRARY_IMPL(torcheval_amd_prdc, CUDA, m) {
  m.impl("prdc_norms", &prdc_norms);
  m.impl("prdc_knn", &prdc_knn);
  m.impl("prdc_radii", &prdc_radii);
  m.impl("prdc_cross", &prdc_cross);
  m.impl("prdc_finish", &prdc_finish);
}

TORCH_LIBRARY_IMPL(torcheval_amd_prdc, Meta, m) {
  m.impl("prdc_norms", &MetaNoop<&prdc_norms>::call);
  m.impl("prdc_knn", &MetaNoop<&prdc_knn>::call);
  m.impl("prdc_radii", &MetaNoop<&prdc_radii>::call);
  m.impl("prdc_cross", &MetaNoop<&prdc_cross>::call);
  m.impl("prdc_finish", &MetaNoop<&prdc_finish>::call);
}
