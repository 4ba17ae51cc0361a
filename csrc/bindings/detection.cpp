// K24 detection mean average precision (csrc/kernels/detection_map.hip): dispatcher ops only, in a
// namespace of their own and without pybind entries, because the attributes of `_C` and the
// `torcheval_amd::` ops are recorded in tests/golden/native_api.json and that fixture stays byte for
// byte what it was (as K14-K23's ops).  Eager and compiled calls both take the dispatcher
// (ops/detection.py); tests/metrics/detection/test_mean_ap.py pins the schemas, the dispatch keys
// and the Meta kernels.
#include <ATen/ATen.h>
#include <torch/library.h>

#include "tea_kernels.h"
#include "tea_torch.h"

namespace {

using namespace tea_torch;

const void* rows_of(const Tensor& t, const Tensor& ref, int64_t n, const char* name) {
  TORCH_CHECK(t.dim() == 1 && t.size(0) == n && t.is_contiguous() && t.device() == ref.device(), "map_match: ", name,
              " must be a contiguous [", n, "] tensor on the boxes' device");
  return t.data_ptr();
}

const float* boxes_of(const Tensor& t, const Tensor& ref, const char* name) {
  TORCH_CHECK(t.scalar_type() == at::kFloat && t.dim() == 2 && t.size(1) == 4 && t.is_contiguous() &&
                  t.device() == ref.device() && t.size(0) < (int64_t{1} << 31),
              "map_match: ", name, " must be a contiguous float32 [n < 2^31, 4] tensor on one device");
  return static_cast<const float*>(t.data_ptr());
}

int32_t* i32_rows(const Tensor& t, const Tensor& ref, int64_t n, const char* what, const char* name) {
  return static_cast<int32_t*>(dense_buf(t, at::kInt, ref, n, what, name));
}

// The kernel trusts the image offsets, so they arrive as host integers and are checked here before
// the one small copy that hands them to it: `offsets` is a CPU int64 [2, B + 1] tensor, row 0 the
// first detection and row 1 the first ground truth of every image, ending at the row counts.
void map_match(const Tensor& pred_boxes, const Tensor& pred_scores, const Tensor& pred_labels,
               const Tensor& target_boxes, const Tensor& target_labels, const Tensor& offsets,
               const Tensor& thresholds, int64_t max_detections, const Tensor& scores, const Tensor& labels,
               const Tensor& hits, const Tensor& gt_count, const optional<Tensor>& matched_gt,
               const optional<Tensor>& err) {
  check_gpu(pred_boxes, "pred_boxes");
  tea::MapMatchArgs a;
  a.det_boxes = boxes_of(pred_boxes, pred_boxes, "pred_boxes");
  a.gt_boxes = boxes_of(target_boxes, pred_boxes, "target_boxes");
  const int64_t m = pred_boxes.size(0), g = target_boxes.size(0);
  a.det_scores = rows_of(pred_scores, pred_boxes, m, "pred_scores");
  a.score_dt = dt_of(pred_scores);
  a.det_labels = rows_of(pred_labels, pred_boxes, m, "pred_labels");
  a.det_label_dt = dt_of(pred_labels);
  a.gt_labels = rows_of(target_labels, pred_boxes, g, "target_labels");
  a.gt_label_dt = dt_of(target_labels);
  TORCH_CHECK(offsets.is_cpu() && offsets.scalar_type() == at::kLong && offsets.dim() == 2 && offsets.size(0) == 2 &&
                  offsets.size(1) >= 1 && offsets.size(1) < (int64_t{1} << 31) && offsets.is_contiguous(),
              "map_match: offsets must be a contiguous CPU int64 [2, B + 1] tensor");
  const int64_t b = offsets.size(1) - 1;
  const int64_t* off = offsets.data_ptr<int64_t>();
  for (int r = 0; r < 2; ++r) {
    const int64_t* o = off + r * (b + 1);
    TORCH_CHECK(o[0] == 0 && o[b] == (r == 0 ? m : g), "map_match: offsets must run from 0 to the row count");
    for (int64_t i = 0; i < b; ++i)
      TORCH_CHECK(o[i + 1] >= o[i] && o[i + 1] - o[i] <= tea::kMapMaxBoxes,
                  "map_match: every image must hold 0 to ", tea::kMapMaxBoxes, " boxes, image ", i, " holds ",
                  o[i + 1] - o[i]);
  }
  TORCH_CHECK(thresholds.scalar_type() == at::kDouble && thresholds.dim() == 1 && thresholds.is_contiguous() &&
                  thresholds.size(0) >= 1 && thresholds.size(0) <= tea::kMapMaxThresholds &&
                  thresholds.device() == pred_boxes.device(),
              "map_match: thresholds must be a float64 [1 .. ", tea::kMapMaxThresholds, "] tensor on the boxes' device");
  TORCH_CHECK(max_detections >= 1, "map_match: max_detections must be >= 1, got ", max_detections);
  TORCH_CHECK(gt_count.dim() == 1 && gt_count.size(0) >= 1 && gt_count.size(0) <= tea::kMapMaxClasses,
              "map_match: gt_count must be [1 .. 2^22 - 1]");
  a.thresholds = thresholds.data_ptr<double>();
  a.num_images = static_cast<int>(b);
  a.num_thresholds = static_cast<int>(thresholds.size(0));
  a.num_classes = static_cast<int>(gt_count.size(0));
  a.max_detections = static_cast<int>(std::min<int64_t>(max_detections, tea::kMapMaxBoxes));
  a.scores = f32_out(scores, pred_boxes, m, "scores");
  a.labels = i32_rows(labels, pred_boxes, m, "map_match", "labels");
  a.hits = i32_rows(hits, pred_boxes, m, "map_match", "hits");
  a.gt_count = static_cast<long long*>(dense_buf(gt_count, at::kLong, pred_boxes, a.num_classes, "map_match", "gt_count"));
  if (matched_gt.has_value())
    a.matched_gt = i32_rows(*matched_gt, pred_boxes, m * a.num_thresholds, "map_match", "matched_gt");
  a.err = err_ptr(err, pred_boxes, "map_match");
  if (b == 0) return;
  DeviceGuard guard(pred_boxes.device());
  const Tensor device_offsets = offsets.to(pred_boxes.device(), /*non_blocking=*/true);
  a.offsets = device_offsets.data_ptr<int64_t>();
  check_launch(tea::launch_map_match(a, stream_for(pred_boxes)), "map_match");
}

// ap, rec [T, C] (float64) <- the tables of hits [N] (int32) in the global order (label, score
// descending, stored order) with class_offsets [C + 1] (int64) and gt_count [C] (float64);
// scalars [4] (map, map_50, map_75, mar), map_per_class [C] and mar_per_class [C] (float32) <- the
// means.  Two launches.
void map_curve(const Tensor& hits, const Tensor& class_offsets, const Tensor& gt_count, int64_t index_50,
               int64_t index_75, const Tensor& ap, const Tensor& rec, const Tensor& scalars,
               const Tensor& map_per_class, const Tensor& mar_per_class) {
  check_gpu(gt_count, "gt_count");
  TORCH_CHECK(gt_count.dim() == 1 && gt_count.size(0) >= 1 && gt_count.size(0) < (int64_t{1} << 31) &&
                  ap.dim() == 2 && ap.size(0) >= 1 && ap.size(0) <= tea::kMapMaxThresholds &&
                  ap.size(1) == gt_count.size(0),
              "map_curve: gt_count must be [C] and ap [T <= ", tea::kMapMaxThresholds, ", C]");
  TORCH_CHECK(hits.dim() == 1 && hits.size(0) < (int64_t{1} << 31), "map_curve: hits must be [N < 2^31]");
  tea::MapCurveArgs a;
  a.num_classes = static_cast<int>(gt_count.size(0));
  a.num_thresholds = static_cast<int>(ap.size(0));
  TORCH_CHECK(index_50 >= -1 && index_50 < a.num_thresholds && index_75 >= -1 && index_75 < a.num_thresholds,
              "map_curve: index_50 and index_75 must be rows of the tables, or -1");
  a.index_50 = static_cast<int>(index_50);
  a.index_75 = static_cast<int>(index_75);
  const int64_t cells = static_cast<int64_t>(a.num_classes) * a.num_thresholds;
  a.hits = i32_rows(hits, gt_count, hits.size(0), "map_curve", "hits");
  a.class_offsets =
      static_cast<const int64_t*>(dense_buf(class_offsets, at::kLong, gt_count, a.num_classes + 1, "map_curve", "class_offsets"));
  a.gt_count = f64_buf(gt_count, gt_count, a.num_classes, "map_curve", "gt_count");
  a.ap = f64_buf(ap, gt_count, cells, "map_curve", "ap");
  a.rec = f64_buf(rec, gt_count, cells, "map_curve", "rec");
  a.scalars = f32_out(scalars, gt_count, 4, "scalars");
  a.map_per_class = f32_out(map_per_class, gt_count, a.num_classes, "map_per_class");
  a.mar_per_class = f32_out(mar_per_class, gt_count, a.num_classes, "mar_per_class");
  DeviceGuard guard(gt_count.device());
  check_launch(tea::launch_map_curve(a, stream_for(gt_count)), "map_curve");
}

}  // namespace

TORCH_LIBRARY(torcheval_amd_detection, m) {
  m.def("map_match(Tensor pred_boxes, Tensor pred_scores, Tensor pred_labels, Tensor target_boxes, "
        "Tensor target_labels, Tensor offsets, Tensor thresholds, int max_detections, Tensor(a!) scores, "
        "Tensor(b!) labels, Tensor(c!) hits, Tensor(d!) gt_count, Tensor(e!)? matched_gt, Tensor(f!)? err) -> ()");
  m.def("map_curve(Tensor hits, Tensor class_offsets, Tensor gt_count, int index_50, int index_75, Tensor(a!) ap, "
        "Tensor(b!) rec, Tensor(c!) scalars, Tensor(d!) map_per_class, Tensor(e!) mar_per_class) -> ()");
}

TORCH_LIBRARY_IMPL(torcheval_amd_detection, CUDA, m) {
  m.impl("map_match", &map_match);
  m.impl("map_curve", &map_curve);
}

TORCH_LIBRARY_IMPL(torcheval_amd_detection, Meta, m) {
  m.impl("map_match", &MetaNoop<&map_match>::call);
  m.impl("map_curve", &MetaNoop<&map_curve>::call);
}
