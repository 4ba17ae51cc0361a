// K23 silhouette coefficient (csrc/kernels/silhouette.hip): dispatcher ops only, in a namespace of
// their own and without pybind entries, because the attributes of `_C` and the `torcheval_amd::`
// ops are recorded in tests/golden/native_api.json and that fixture stays byte for byte what it was
// (as K14-K22's ops).  Eager and compiled calls both take the dispatcher (ops/silhouette.py);
// tests/metrics/clustering/test_silhouette.py pins the schemas, the dispatch keys and the Meta
// kernels.
#include <ATen/ATen.h>
#include <torch/library.h>

#include "tea_kernels.h"
#include "tea_torch.h"

namespace {

using namespace tea_torch;

int32_t* i32_buf(const Tensor& t, const Tensor& ref, int64_t numel, const char* what, const char* name) {
  return static_cast<int32_t*>(dense_buf(t, at::kInt, ref, numel, what, name));
}

tea::SilhouetteArgs feature_args(const Tensor& input, const Tensor& norms, const char* what) {
  check_features(input, what, "input");
  TORCH_CHECK(input.size(0) < (int64_t{1} << 31) - tea::kSilTile && input.size(1) < (int64_t{1} << 31) - 64, what,
              ": input must have fewer than 2^31 - 128 rows and 2^31 - 64 columns");
  tea::SilhouetteArgs a;
  a.x = input.data_ptr<float>();
  a.stride = input.stride(0);
  a.n = input.size(0);
  a.d = input.size(1);
  a.norms = f64_buf(norms, input, a.n, what, "norms");
  return a;
}

// the plan of ops/silhouette.py: labels [n], panel_cluster [max_panels], counts [k], num_panels [1]
void plan_args(tea::SilhouetteArgs& a, const Tensor& ref, const Tensor& labels, const Tensor& panel_cluster,
               const Tensor& counts, const Tensor& num_panels, const char* what) {
  TORCH_CHECK(panel_cluster.dim() == 1 && panel_cluster.size(0) >= 1 &&
                  panel_cluster.size(0) < (int64_t{1} << 31) / tea::kSilTile && counts.dim() == 1 &&
                  counts.size(0) >= 1 && counts.size(0) < (int64_t{1} << 31),
              what, ": panel_cluster must be [max_panels >= 1] and counts [k >= 1]");
  a.max_panels = static_cast<int>(panel_cluster.size(0));
  a.k = static_cast<int>(counts.size(0));
  a.labels = i32_buf(labels, ref, a.n, what, "labels");
  a.panel_cluster = i32_buf(panel_cluster, ref, a.max_panels, what, "panel_cluster");
  a.counts = i32_buf(counts, ref, a.k, what, "counts");
  a.num_panels = i32_buf(num_panels, ref, 1, what, "num_panels");
}

// norms[n] (float64) <- the FP64 sums of squares of the rows, NaN for a row with a NaN or an inf
void silhouette_norms(const Tensor& input, const Tensor& norms) {
  tea::SilhouetteArgs a = feature_args(input, norms, "silhouette_norms");
  DeviceGuard guard(input.device());
  check_launch(tea::launch_silhouette_norms(a, stream_for(input)), "silhouette_norms");
}

// edges[G, 4, n] (float64) <- per panel range and sample the raw distance sums over the range's
// first and last cluster, the smallest mean over the clusters inside it (own excluded) and the raw
// sum over the own cluster inside it; G = silhouette_groups(n, max_panels, D, groups)
void silhouette_tile(const Tensor& input, const Tensor& norms, const Tensor& labels, const Tensor& ref_index,
                     const Tensor& panel_cluster, const Tensor& counts, const Tensor& num_panels, int64_t groups,
                     const Tensor& edges) {
  tea::SilhouetteArgs a = feature_args(input, norms, "silhouette_tile");
  TORCH_CHECK(groups >= 0, "silhouette_tile: groups must be >= 0 (0: the rule of silhouette_groups), got ", groups);
  plan_args(a, input, labels, panel_cluster, counts, num_panels, "silhouette_tile");
  a.ref_index = i32_buf(ref_index, input, static_cast<int64_t>(a.max_panels) * tea::kSilTile, "silhouette_tile",
                        "ref_index");
  a.groups = static_cast<int>(tea::silhouette_groups(a.n, a.max_panels, a.d, groups));
  TORCH_CHECK(edges.dim() == 3 && edges.size(0) == a.groups && edges.size(1) == 4 && edges.size(2) == a.n,
              "silhouette_tile: edges must be [G, 4, n] with G = ", a.groups);
  a.edges = f64_buf(edges, input, 4 * a.groups * a.n, "silhouette_tile", "edges");
  DeviceGuard guard(input.device());
  check_launch(tea::launch_silhouette_tile(a, stream_for(input)), "silhouette_tile");
}

// a, b, s [n] (float64), samples [n] (float32) <- the ranges of edges[G, 4, n] stitched per sample;
// score64 [1], score [1] <- the mean of s over the labelled samples (NaN with fewer than two
// non-empty clusters).  Two launches; block_sums is float64 [silhouette_stitch_blocks(n)] scratch
void silhouette_finish(const Tensor& edges, const Tensor& labels, const Tensor& panel_cluster, const Tensor& counts,
                       const Tensor& num_panels, const Tensor& block_sums, const Tensor& a_out, const Tensor& b_out,
                       const Tensor& s_out, const Tensor& samples, const Tensor& score64, const Tensor& score) {
  check_gpu(edges, "edges");
  TORCH_CHECK(edges.scalar_type() == at::kDouble && edges.is_contiguous() && edges.dim() == 3 && edges.size(0) >= 1 &&
                  edges.size(1) == 4 && edges.size(2) >= 1 && edges.size(2) < (int64_t{1} << 31) - tea::kSilTile,
              "silhouette_finish: edges must be a contiguous float64 [G, 4, n] tensor");
  tea::SilhouetteArgs a;
  a.n = edges.size(2);
  a.d = 1;
  plan_args(a, edges, labels, panel_cluster, counts, num_panels, "silhouette_finish");
  TORCH_CHECK(edges.size(0) <= a.max_panels, "silhouette_finish: more ranges than panels");
  a.groups = static_cast<int>(edges.size(0));
  a.edges = edges.data_ptr<double>();
  a.block_sums = f64_buf(block_sums, edges, tea::silhouette_stitch_blocks(a.n), "silhouette_finish", "block_sums");
  a.a = f64_buf(a_out, edges, a.n, "silhouette_finish", "a");
  a.b = f64_buf(b_out, edges, a.n, "silhouette_finish", "b");
  a.s = f64_buf(s_out, edges, a.n, "silhouette_finish", "s");
  a.samples = f32_out(samples, edges, a.n, "samples");
  a.score64 = f64_buf(score64, edges, 1, "silhouette_finish", "score64");
  a.score = f32_out(score, edges, 1, "score");
  DeviceGuard guard(edges.device());
  check_launch(tea::launch_silhouette_finish(a, stream_for(edges)), "silhouette_finish");
}

}  // namespace

TORCH_LIBRARY(torcheval_amd_silhouette, m) {
  m.def("silhouette_norms(Tensor input, Tensor(a!) norms) -> ()");
  m.def("silhouette_tile(Tensor input, Tensor norms, Tensor labels, Tensor ref_index, Tensor panel_cluster, "
        "Tensor counts, Tensor num_panels, int groups, Tensor(a!) edges) -> ()");
  m.def("silhouette_finish(Tensor edges, Tensor labels, Tensor panel_cluster, Tensor counts, Tensor num_panels, "
        "Tensor(a!) block_sums, Tensor(b!) a, Tensor(c!) b, Tensor(d!) s, Tensor(e!) samples, Tensor(f!) score64, "
        "Tensor(g!) score) -> ()");
}

TORCH_LIBRARY_IMPL(torcheval_amd_silhouette, CUDA, m) {
  m.impl("silhouette_norms", &silhouette_norms);
  m.impl("silhouette_tile", &silhouette_tile);
  m.impl("silhouette_finish", &silhouette_finish);
}

TORCH_LIBRARY_IMPL(torcheval_amd_silhouette, Meta, m) {
  m.impl("silhouette_norms", &MetaNoop<&silhouette_norms>::call);
  m.impl("silhouette_tile", &MetaNoop<&silhouette_tile>::call);
  m.impl("silhouette_finish", &MetaNoop<&silhouette_finish>::call);
}
