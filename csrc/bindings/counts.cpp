// torcheval_amd._C bindings (layout: module.cpp): K1 classification counts, K1b binary counts, K2 multilabel
// counts, K10 rank-of-target scores, K4 binned histograms, K4b per-sample binned AUROC, the binned finalize.
#include <ATen/ATen.h>
#include <torch/csrc/utils/pybind.h>
#include <torch/library.h>

#include "tea_kernels.h"
#include "tea_torch.h"

namespace {

using namespace tea_torch;

// ---------------------------------------------------------------- K1 classification counts
void cls_counts(const Tensor& input, const Tensor& target, int64_t k, int64_t num_classes,
                const optional<Tensor>& micro_correct, const optional<Tensor>& micro_total,
                const optional<Tensor>& cls_correct, const optional<Tensor>& cls_label,
                const optional<Tensor>& cls_pred, const optional<Tensor>& confusion,
                const optional<Tensor>& err, int64_t max_blocks,
                const optional<Tensor>& micro_incorrect, const optional<Tensor>& micro_total2,
                const optional<Tensor>& cls_fp) {
  check_gpu(input, "input");
  check_gpu(target, "target");
  TORCH_CHECK(target.dim() == 1, "cls_counts: target must be 1-D");
  TORCH_CHECK(input.dim() == 1 || input.dim() == 2, "cls_counts: input must be 1-D or 2-D");
  TORCH_CHECK(input.size(0) == target.size(0), "cls_counts: first dims differ");
  TORCH_CHECK(target.is_contiguous(), "cls_counts: target must be contiguous");
  DeviceGuard guard(input.device());
  tea::ClsCountsArgs a;
  Tensor in = input;
  if (input.dim() == 2) {
    if (in.stride(1) != 1) in = in.contiguous();
    a.c = in.size(1);
    a.row_stride = in.stride(0);
    TORCH_CHECK(a.c < (int64_t(1) << 31), "cls_counts: too many classes");
    TORCH_CHECK(k >= 1 && k <= a.c || a.c == 0, "cls_counts: k out of range");
    if (num_classes <= 0) num_classes = a.c;
    TORCH_CHECK(num_classes == a.c, "cls_counts: num_classes must match input.size(1)");
  } else {
    if (!in.is_contiguous()) in = in.contiguous();
    TORCH_CHECK(k == 1, "cls_counts: k > 1 needs 2-D scores");
  }
  const int64_t C = num_classes;
  a.input = in.data_ptr();
  a.in_dt = dt_of(in);
  a.n = in.size(0);
  a.target = target.data_ptr();
  a.tg_dt = dt_of(target);
  a.k = static_cast<int>(k);
  a.num_classes = C;
  a.micro_correct = f32_out(micro_correct, input, 1, "micro_correct");
  a.micro_total = f32_out(micro_total, input, 1, "micro_total");
  a.cls_correct = f32_out(cls_correct, input, C, "cls_correct");
  a.cls_label = f32_out(cls_label, input, C, "cls_label");
  a.cls_pred = f32_out(cls_pred, input, C, "cls_pred");
  a.confusion = f32_out(confusion, input, C * C, "confusion");
  a.micro_incorrect = f32_out(micro_incorrect, input, 1, "micro_incorrect");
  a.micro_total2 = f32_out(micro_total2, input, 1, "micro_total2");
  a.cls_fp = f32_out(cls_fp, input, C, "cls_fp");
  TORCH_CHECK(!(k > 1 && (a.cls_pred || a.confusion || a.cls_fp)),
              "cls_counts: predictions are undefined for k > 1");
  TORCH_CHECK((a.cls_correct || a.cls_label || a.cls_pred || a.confusion || a.cls_fp) == false ||
                  C > 0,
              "cls_counts: num_classes required for histograms");
  if ((a.err = err_ptr(err, input, "cls_counts")) != nullptr) {
    if (err->numel() >= 3) a.err_max = a.err + 1;  // [flags, max bad target, max bad prediction]
    a.check_target = 1;
  }
  a.max_blocks = static_cast<int>(max_blocks);
  const hipStream_t stream = stream_for(input);
  if (a.micro_correct || a.micro_incorrect) a.fold_ws = fold_workspace(input, stream);
  const int rc = tea::launch_cls_counts(a, stream);
  TORCH_CHECK(rc != -1, "cls_counts: unsupported input dtype ", input.scalar_type());
  check_launch(rc, "cls_counts");
}

// Lean entry of the north-star update (MulticlassAccuracy micro, k=1): every precondition of
// the wide K1 launch is tested here, and anything unusual returns false so the caller takes
// the general Python path (which raises the reference's own errors).  One pybind call with
// four positional tensors instead of the 15-argument cls_counts plus its Python-side checks.
bool micro_accuracy_update(const Tensor& input, const Tensor& target, const Tensor& correct,
                           const Tensor& total, int64_t num_classes, const optional<Tensor>& pend) {
  if (!input.is_cuda() || input.dim() != 2 || target.dim() != 1) return false;
  const int64_t n = input.size(0), c = input.size(1);
  if (target.size(0) != n || c <= 0 || c >= (int64_t(1) << 31) || input.stride(1) != 1) return false;
  // a metric built with num_classes only accepts [N, num_classes] scores: anything else goes
  // to the Python path, which raises the reference's ValueError (accuracy.py:340-346)
  if (num_classes > 0 && c != num_classes) return false;
  const auto st = input.scalar_type();
  if (st != at::kFloat && st != at::kBFloat16 && st != at::kHalf) return false;
  switch (target.scalar_type()) {
    case at::kLong: case at::kInt: case at::kShort: case at::kChar: case at::kByte: case at::kBool:
      break;
    default: return false;
  }
  if (!target.is_contiguous()) return false;
  const auto dev = input.device();
  if (target.device() != dev || correct.device() != dev || total.device() != dev) return false;
  if (correct.scalar_type() != at::kFloat || total.scalar_type() != at::kFloat ||
      correct.numel() != 1 || total.numel() != 1)
    return false;
  DeviceGuard guard(dev);
  tea::ClsCountsArgs a;
  a.input = input.data_ptr();
  a.in_dt = dt_of(input);
  a.n = n;
  a.c = c;
  a.row_stride = input.stride(0);
  a.target = target.data_ptr();
  a.tg_dt = dt_of(target);
  a.k = 1;
  a.num_classes = c;
  a.micro_correct = correct.data_ptr<float>();
  a.micro_total = total.data_ptr<float>();
  const hipStream_t stream = stream_for(input);
  if (pend.has_value()) {
    if (pend->scalar_type() != at::kLong || pend->numel() < tea::kPendCells * tea::kPendStride ||
        pend->device() != dev || !pend->is_contiguous())
      return false;
    a.pend = reinterpret_cast<unsigned long long*>(pend->data_ptr<int64_t>());
  } else {
    a.fold_ws = fold_workspace(input, stream);
  }
  check_launch(tea::launch_cls_counts(a, stream), "micro_accuracy_update");
  return true;
}

// Fold the K1 micro kernel's pending cells into ``correct`` (cells zeroed); with ``out``, also
// write correct / total there: the deferred fold and the accuracy division in one launch.
void micro_accuracy_finish(const Tensor& pend, const Tensor& correct, const Tensor& total,
                           const optional<Tensor>& out) {
  check_gpu(pend, "pend");
  TORCH_CHECK(pend.scalar_type() == at::kLong && pend.is_contiguous() &&
                  pend.numel() >= tea::kPendCells * tea::kPendStride,
              "micro_accuracy_finish: pend must be int64 [>= 512]");
  TORCH_CHECK(correct.scalar_type() == at::kFloat && total.scalar_type() == at::kFloat && correct.numel() == 1 &&
                  total.numel() == 1 && correct.device() == pend.device() && total.device() == pend.device(),
              "micro_accuracy_finish: float32 scalar states on the pending cells' device");
  float* o = nullptr;
  if (out.has_value()) {
    TORCH_CHECK(out->scalar_type() == at::kFloat && out->numel() == 1 && out->device() == pend.device(),
                "micro_accuracy_finish: out must be a float32 scalar");
    o = out->data_ptr<float>();
  }
  DeviceGuard guard(pend.device());
  check_launch(tea::launch_micro_finish(reinterpret_cast<unsigned long long*>(pend.data_ptr<int64_t>()),
                                        correct.data_ptr<float>(), total.data_ptr<float>(), o, stream_for(pend)),
               "micro_accuracy_finish");
}

// ---------------------------------------------------------------- K10 rank-of-target scores
Tensor rank_scores(const Tensor& input, const Tensor& target, int64_t mode, int64_t k,
                   const optional<Tensor>& err) {
  check_gpu(input, "input");
  check_gpu(target, "target");
  TORCH_CHECK(input.dim() == 2 && target.dim() == 1 && input.size(0) == target.size(0),
              "rank_scores: input [n, c] and target [n] expected");
  TORCH_CHECK(mode == 0 || mode == 1, "rank_scores: mode must be 0 (hit) or 1 (reciprocal)");
  TORCH_CHECK(input.size(1) < (int64_t(1) << 31), "rank_scores: too many columns");
  DeviceGuard guard(input.device());
  Tensor in = input.stride(1) == 1 ? input : input.contiguous();
  Tensor tg = target.contiguous();
  tea::RankArgs a;
  a.input = in.data_ptr();
  a.in_dt = dt_of(in);
  a.n = in.size(0);
  a.c = in.size(1);
  a.row_stride = in.stride(0);
  a.target = tg.data_ptr();
  a.tg_dt = dt_of(tg);
  a.mode = static_cast<int>(mode);
  a.k = static_cast<int>(k);
  Tensor out = at::empty({a.n}, input.options().dtype(at::kFloat));
  a.out = out.data_ptr<float>();
  a.err = err_ptr(err, input, "rank_scores");
  const int rc = tea::launch_rank_scores(a, stream_for(input));
  TORCH_CHECK(rc != -1, "rank_scores: unsupported input dtype ", input.scalar_type());
  check_launch(rc, "rank_scores");
  return out;
}

void binary_counts(const Tensor& input, const Tensor& target, const optional<Tensor>& weight,
                   double threshold, const optional<Tensor>& tp, const optional<Tensor>& fp,
                   const optional<Tensor>& tn, const optional<Tensor>& fn,
                   const optional<Tensor>& total, int64_t strict, int64_t max_blocks,
                   const optional<Tensor>& tp2, const optional<Tensor>& fp2,
                   const optional<Tensor>& tn2, const optional<Tensor>& fn2) {
  check_gpu(input, "input");
  check_gpu(target, "target");
  TORCH_CHECK(input.numel() == target.numel(), "binary_counts: size mismatch");
  DeviceGuard guard(input.device());
  Tensor in = input.contiguous();
  Tensor tg = target.contiguous();
  Tensor w;
  tea::BinaryCountsArgs a;
  if (weight.has_value()) {
    w = weight->contiguous();
    TORCH_CHECK(w.numel() == in.numel(), "binary_counts: weight size mismatch");
    a.weight = w.data_ptr();
    a.w_dt = dt_of(w);
  }
  a.input = in.data_ptr();
  a.in_dt = dt_of(in);
  a.target = tg.data_ptr();
  a.tg_dt = dt_of(tg);
  a.n = in.numel();
  a.threshold = threshold_as(in, threshold);
  a.threshold64 = threshold;
  a.strict_binary = static_cast<int>(strict);
  a.out[0] = f32_out(tp, input, 1, "tp");
  a.out[1] = f32_out(fp, input, 1, "fp");
  a.out[2] = f32_out(tn, input, 1, "tn");
  a.out[3] = f32_out(fn, input, 1, "fn");
  a.total = f32_out(total, input, 1, "total");
  a.out2[0] = f32_out(tp2, input, 1, "tp2");
  a.out2[1] = f32_out(fp2, input, 1, "fp2");
  a.out2[2] = f32_out(tn2, input, 1, "tn2");
  a.out2[3] = f32_out(fn2, input, 1, "fn2");
  a.max_blocks = static_cast<int>(max_blocks);
  check_launch(tea::launch_binary_counts(a, stream_for(input)), "binary_counts");
}

// K2: multilabel accuracy counts straight into float32 state scalars.
void multilabel_counts(const Tensor& input, const Tensor& target, double threshold, int64_t k,
                       int64_t criteria, const Tensor& num_correct, const optional<Tensor>& num_total,
                       double total) {
  check_gpu(input, "input");
  check_gpu(target, "target");
  TORCH_CHECK(input.dim() == 2 && target.sizes() == input.sizes(),
              "multilabel_counts: input/target must be [n, c] of equal shape");
  TORCH_CHECK(input.stride(1) == 1 && target.stride(1) == 1,
              "multilabel_counts: rows must be contiguous");
  TORCH_CHECK(num_correct.scalar_type() == at::kFloat && num_correct.numel() == 1 &&
                  num_correct.device() == input.device(),
              "multilabel_counts: num_correct must be a float32 scalar on the input device");
  TORCH_CHECK(criteria >= 0 && criteria <= 4, "multilabel_counts: bad criteria");
  TORCH_CHECK(k == 0 || (k >= 1 && k <= input.size(1) && input.size(1) <= tea::multilabel_max_topk_cols()),
              "multilabel_counts: top-k needs 1 <= k <= c <= ", tea::multilabel_max_topk_cols());
  TORCH_CHECK(criteria != 1 || input.numel() < (int64_t{1} << 31),
              "multilabel_counts: hamming counts must fit 31 bits per launch");
  DeviceGuard guard(input.device());
  hipStream_t stream = stream_for(input);
  tea::MultilabelArgs a;
  a.x = input.data_ptr();
  a.x_dt = dt_of(input);
  a.x_row_stride = input.stride(0);
  a.t = target.data_ptr();
  a.t_dt = dt_of(target);
  a.t_row_stride = target.stride(0);
  a.n = input.size(0);
  a.c = input.size(1);
  a.threshold = threshold_as(input, threshold);
  a.k = static_cast<int>(k);
  a.criteria = static_cast<int>(criteria);
  a.num_correct = num_correct.data_ptr<float>();
  if (num_total.has_value()) {
    TORCH_CHECK(num_total->scalar_type() == at::kFloat && num_total->numel() == 1,
                "multilabel_counts: num_total must be a float32 scalar");
    a.num_total = num_total->data_ptr<float>();
    a.total = total;
  }
  a.fold_ws = fold_workspace(input, stream);
  const int rc = tea::launch_multilabel(a, stream);
  TORCH_CHECK(rc != -1, "multilabel_counts: unsupported dtypes ", input.scalar_type(), "/",
              target.scalar_type());
  check_launch(rc, "multilabel_counts");
}

// ---------------------------------------------------------------- K4 binned histograms
// input: [n, c] view (any strides); target: [n, c] view (mode 0) or [n] labels (mode 1);
// thr: float32 [T] sorted; tp/fp/fn: float32 [T, c] views sharing strides (accumulated).
void binned_counts(const Tensor& input, const Tensor& target, const Tensor& thr, int64_t mode,
                   const optional<Tensor>& tp, const optional<Tensor>& fp,
                   const optional<Tensor>& fn, int64_t uniform) {
  check_gpu(input, "input");
  TORCH_CHECK(input.dim() == 2, "binned_counts: input must be a 2-D view [n, c]");
  TORCH_CHECK(thr.dim() == 1 && thr.scalar_type() == at::kFloat && thr.is_contiguous(),
              "binned_counts: thresholds must be a contiguous float32 vector");
  DeviceGuard guard(input.device());
  tea::BinnedArgs a;
  a.input = input.data_ptr();
  a.in_dt = dt_of(input);
  a.n = input.size(0);
  a.c = input.size(1);
  a.in_row_stride = input.stride(0);
  a.in_col_stride = input.stride(1);
  a.mode = static_cast<int>(mode);
  if (mode == 1) {
    TORCH_CHECK(target.dim() == 1 && target.size(0) == a.n, "binned_counts: labels must be [n]");
    a.tg_row_stride = target.stride(0);
  } else {
    TORCH_CHECK(target.dim() == 2 && target.size(0) == a.n && target.size(1) == a.c,
                "binned_counts: target must match input");
    a.tg_row_stride = target.stride(0);
    a.tg_col_stride = target.stride(1);
  }
  a.target = target.data_ptr();
  a.tg_dt = dt_of(target);
  a.thr = thr.data_ptr<float>();
  a.T = static_cast<int>(thr.numel());
  a.uniform = uniform != 0 && a.T >= 2;
  int64_t ks = -1, cs = -1;
  auto out = [&](const optional<Tensor>& t, const char* name) -> float* {
    if (!t.has_value()) return nullptr;
    TORCH_CHECK(t->scalar_type() == at::kFloat && t->dim() == 2 && t->size(0) == a.T &&
                    t->size(1) == a.c && t->device() == input.device(),
                "binned_counts: ", name, " must be float32 [T, c] on the input device");
    TORCH_CHECK(ks < 0 || (ks == t->stride(0) && cs == t->stride(1)),
                "binned_counts: outputs must share strides");
    ks = t->stride(0);
    cs = t->stride(1);
    return t->data_ptr<float>();
  };
  a.tp = out(tp, "tp");
  a.fp = out(fp, "fp");
  a.fn = out(fn, "fn");
  a.out_k_stride = ks;
  a.out_c_stride = cs;
  a.ws = reinterpret_cast<unsigned*>(
      zeroed_workspace(input, stream_for(input), tea::binned_workspace_words(a.T, a.c) * 4, Zeroed::kBinnedHist));
  if (const int64_t sw = tea::binned_slab_words(a.T, a.c))
    a.slab = reinterpret_cast<unsigned*>(zeroed_workspace(input, stream_for(input), sw * 4, Zeroed::kBinnedSlab));
  const int rc = tea::launch_binned(a, stream_for(input));
  TORCH_CHECK(rc != -1, "binned_counts: too many thresholds (", a.T, ") for the LDS histogram");
  check_launch(rc, "binned_counts");
}

// ---------------------------------------------------------------- K4b per-sample binned AUROC
// input float32 [n, c] (unit column stride), target int64 / int32 [n], thr float32 [T] ascending
// (contiguous), out float32 [n], err int32 [>= 1] (bit 0: a label outside [0, c))
void sample_binned_auroc(const Tensor& input, const Tensor& target, const Tensor& thr, const Tensor& out,
                         const Tensor& err) {
  check_gpu(input, "input");
  TORCH_CHECK(input.dim() == 2 && input.scalar_type() == at::kFloat && input.stride(1) == 1,
              "sample_binned_auroc: input must be float32 [n, c] with unit column stride");
  TORCH_CHECK(target.dim() == 1 && target.size(0) == input.size(0) && target.device() == input.device() &&
                  (target.scalar_type() == at::kLong || target.scalar_type() == at::kInt),
              "sample_binned_auroc: target must be int64 / int32 [n] on the input's device");
  TORCH_CHECK(thr.dim() == 1 && thr.scalar_type() == at::kFloat && thr.is_contiguous() && thr.device() == input.device(),
              "sample_binned_auroc: thresholds must be a contiguous float32 vector on the input's device");
  TORCH_CHECK(out.scalar_type() == at::kFloat && out.is_contiguous() && out.numel() == input.size(0) &&
                  out.device() == input.device(),
              "sample_binned_auroc: out must be float32 [n]");
  TORCH_CHECK(err.scalar_type() == at::kInt && err.numel() >= 1 && err.device() == input.device(),
              "sample_binned_auroc: err must be int32");
  DeviceGuard guard(input.device());
  tea::SampleAurocArgs a;
  a.input = input.data_ptr<float>();
  a.n = input.size(0);
  a.c = input.size(1);
  a.row_stride = input.stride(0);
  a.target = target.data_ptr();
  a.tg_dt = dt_of(target);
  a.tg_stride = target.stride(0);
  a.thr = thr.data_ptr<float>();
  a.T = static_cast<int>(thr.numel());
  a.out = out.data_ptr<float>();
  a.err = err.data_ptr<int>();
  const int rc = tea::launch_sample_binned_auroc(a, stream_for(input));
  TORCH_CHECK(rc != -1, "sample_binned_auroc: unsupported arguments (needs c >= 1, T >= 1)");
  check_launch(rc, "sample_binned_auroc");
}

// binned AUROC / AUPRC from [T, rows] float32 counts in one launch
void binned_finalize(const Tensor& tp, const Tensor& fp, const optional<Tensor>& fn,
                     const optional<Tensor>& out_auroc, const optional<Tensor>& out_auprc,
                     const optional<Tensor>& out_prec, const optional<Tensor>& out_rec) {
  check_gpu(tp, "tp");
  TORCH_CHECK(tp.dim() == 2 && tp.scalar_type() == at::kFloat && fp.sizes() == tp.sizes() &&
                  fp.strides() == tp.strides() && fp.scalar_type() == at::kFloat,
              "binned_finalize: tp/fp must be float32 [T, rows] with equal strides");
  DeviceGuard guard(tp.device());
  tea::BinnedFinalizeArgs a;
  a.tp = tp.data_ptr<float>();
  a.fp = fp.data_ptr<float>();
  a.k_stride = tp.stride(0);
  a.r_stride = tp.stride(1);
  a.T = static_cast<int>(tp.size(0));
  a.rows = tp.size(1);
  if (out_auprc.has_value()) {
    TORCH_CHECK(fn.has_value() && fn->sizes() == tp.sizes() && fn->strides() == tp.strides() &&
                    fn->scalar_type() == at::kFloat, "binned_finalize: AUPRC needs fn like tp");
    TORCH_CHECK(out_auprc->scalar_type() == at::kFloat && out_auprc->is_contiguous() &&
                    out_auprc->numel() == a.rows, "binned_finalize: out_auprc float32 [rows]");
    a.fn = fn->data_ptr<float>();
    a.out_auprc = out_auprc->data_ptr<float>();
  }
  if (out_auroc.has_value()) {
    TORCH_CHECK(out_auroc->scalar_type() == at::kDouble && out_auroc->is_contiguous() &&
                    out_auroc->numel() == a.rows, "binned_finalize: out_auroc float64 [rows]");
    a.out_auroc = out_auroc->data_ptr<double>();
  }
  if (out_prec.has_value() || out_rec.has_value()) {
    TORCH_CHECK(out_prec.has_value() && out_rec.has_value() && fn.has_value() &&
                    fn->sizes() == tp.sizes() && fn->strides() == tp.strides() &&
                    fn->scalar_type() == at::kFloat,
                "binned_finalize: a curve needs fn like tp and both out_prec / out_rec");
    for (const Tensor* o : {&*out_prec, &*out_rec})
      TORCH_CHECK(o->scalar_type() == at::kFloat && o->is_contiguous() &&
                      o->numel() == a.rows * (a.T + 1) && o->device() == tp.device(),
                  "binned_finalize: curve outputs must be contiguous float32 [rows, T + 1]");
    a.fn = fn->data_ptr<float>();
    a.out_prec = out_prec->data_ptr<float>();
    a.out_rec = out_rec->data_ptr<float>();
  }
  check_launch(tea::launch_binned_finalize(a, stream_for(tp)), "binned_finalize");
}

// ---------------------------------------------------------------- dispatcher forms
// (only where the schema's argument list differs from the function's: three are trimmed, and the
// schema of binned_counts requires all three count tensors where the function takes each optionally)
void op_cls_counts(const Tensor& input, const Tensor& target, int64_t k, int64_t num_classes,
                   const optional<Tensor>& micro_correct, const optional<Tensor>& micro_total,
                   const optional<Tensor>& cls_correct, const optional<Tensor>& cls_label,
                   const optional<Tensor>& cls_pred, const optional<Tensor>& confusion,
                   const optional<Tensor>& err) {
  cls_counts(input, target, k, num_classes, micro_correct, micro_total, cls_correct, cls_label, cls_pred,
             confusion, err, 0, c10::nullopt, c10::nullopt, c10::nullopt);
}
void op_micro_accuracy(const Tensor& input, const Tensor& target, const Tensor& correct, const Tensor& total) {
  TORCH_CHECK(micro_accuracy_update(input, target, correct, total, 0, c10::nullopt),
              "micro_accuracy: unsupported input (needs [N, C] f32/bf16/f16 scores with unit column stride, "
              "[N] integer targets and float32 scalar states on one ROCm device)");
}
void op_binary_counts(const Tensor& input, const Tensor& target, const optional<Tensor>& weight, double threshold,
                      const optional<Tensor>& tp, const optional<Tensor>& fp, const optional<Tensor>& tn,
                      const optional<Tensor>& fn, const optional<Tensor>& total, int64_t strict) {
  binary_counts(input, target, weight, threshold, tp, fp, tn, fn, total, strict, 0, c10::nullopt, c10::nullopt,
                c10::nullopt, c10::nullopt);
}
void op_binned_counts(const Tensor& input, const Tensor& target, const Tensor& thr, int64_t mode, const Tensor& tp,
                      const Tensor& fp, const Tensor& fn, int64_t uniform) {
  binned_counts(input, target, thr, mode, tp, fp, fn, uniform);
}

}  // namespace

void tea_bind_counts(py::module_& m) {
  m.def("rank_scores", &rank_scores, "K10 rank-of-target scores (hit rate / reciprocal rank)", py::arg("input"),
        py::arg("target"), py::arg("mode"), py::arg("k"), py::arg("err") = py::none());
  m.def("micro_accuracy_update", &micro_accuracy_update,
        "K1 micro accuracy (k=1) accumulated into float32 scalar states; false = not handled", py::arg("input"),
        py::arg("target"), py::arg("correct"), py::arg("total"), py::arg("num_classes") = 0,
        py::arg("pend") = py::none());
  m.def("micro_accuracy_finish", &micro_accuracy_finish,
        "fold the micro kernel's pending cells into correct (and write correct / total to out)", py::arg("pend"),
        py::arg("correct"), py::arg("total"), py::arg("out") = py::none());
  m.def("cls_counts", &cls_counts, "K1 fused classification counts", py::arg("input"), py::arg("target"), py::arg("k"),
        py::arg("num_classes"), py::arg("micro_correct"), py::arg("micro_total"), py::arg("cls_correct"),
        py::arg("cls_label"), py::arg("cls_pred"), py::arg("confusion"), py::arg("err"), py::arg("max_blocks") = 0,
        py::arg("micro_incorrect") = py::none(), py::arg("micro_total2") = py::none(), py::arg("cls_fp") = py::none());
  m.def("binary_counts", &binary_counts, "K1b thresholded binary counts", py::arg("input"), py::arg("target"),
        py::arg("weight"), py::arg("threshold"), py::arg("tp"), py::arg("fp"), py::arg("tn"), py::arg("fn"),
        py::arg("total"), py::arg("strict") = 0, py::arg("max_blocks") = 0, py::arg("tp2") = py::none(),
        py::arg("fp2") = py::none(), py::arg("tn2") = py::none(), py::arg("fn2") = py::none());
  m.def("multilabel_counts", &multilabel_counts, "K2 multilabel accuracy counts", py::arg("input"), py::arg("target"),
        py::arg("threshold"), py::arg("k"), py::arg("criteria"), py::arg("num_correct"),
        py::arg("num_total") = py::none(), py::arg("total") = 0.0);
  m.def("binned_counts", &binned_counts, "K4 binned TP/FP/FN per (threshold, class)", py::arg("input"),
        py::arg("target"), py::arg("thr"), py::arg("mode"), py::arg("tp"), py::arg("fp"), py::arg("fn"),
        py::arg("uniform") = 0);
  m.def("sample_binned_auroc", &sample_binned_auroc,
        "K4b per-sample multiclass binned AUROC (the reference default), labels checked into err", py::arg("input"),
        py::arg("target"), py::arg("thr"), py::arg("out"), py::arg("err"));
  m.def("binned_finalize", &binned_finalize, "binned AUROC / AUPRC / PR-curve points from counts", py::arg("tp"),
        py::arg("fp"), py::arg("fn") = py::none(), py::arg("out_auroc") = py::none(), py::arg("out_auprc") = py::none(),
        py::arg("out_prec") = py::none(), py::arg("out_rec") = py::none());
}

TORCH_LIBRARY_FRAGMENT(torcheval_amd, m) {
  m.def("micro_accuracy(Tensor input, Tensor target, Tensor(a!) correct, Tensor(b!) total) -> ()");
  m.def("cls_counts(Tensor input, Tensor target, int k, int num_classes, Tensor(a!)? micro_correct, "
        "Tensor(b!)? micro_total, Tensor(c!)? cls_correct, Tensor(d!)? cls_label, Tensor(e!)? cls_pred, "
        "Tensor(f!)? confusion, Tensor(g!)? err) -> ()");
  m.def("binary_counts(Tensor input, Tensor target, Tensor? weight, float threshold, Tensor(a!)? tp, "
        "Tensor(b!)? fp, Tensor(c!)? tn, Tensor(d!)? fn, Tensor(e!)? total, int strict) -> ()");
  m.def("multilabel_counts(Tensor input, Tensor target, float threshold, int k, int criteria, "
        "Tensor(a!) num_correct, Tensor(b!)? num_total, float total) -> ()");
  m.def("rank_scores(Tensor input, Tensor target, int score_mode, int k, Tensor(a!)? err) -> Tensor");
  m.def("binned_counts(Tensor input, Tensor target, Tensor thr, int target_mode, Tensor(a!) tp, Tensor(b!) fp, "
        "Tensor(c!) fn, int uniform) -> ()");
  m.def("binned_finalize(Tensor tp, Tensor fp, Tensor? fn, Tensor(a!)? out_auroc, Tensor(b!)? out_auprc, "
        "Tensor(c!)? out_prec, Tensor(d!)? out_rec) -> ()");
}

TORCH_LIBRARY_IMPL(torcheval_amd, CUDA, m) {
  m.impl("micro_accuracy", &op_micro_accuracy);
  m.impl("cls_counts", &op_cls_counts);
  m.impl("binary_counts", &op_binary_counts);
  m.impl("multilabel_counts", &multilabel_counts);
  m.impl("rank_scores", &rank_scores);
  m.impl("binned_counts", &op_binned_counts);
  m.impl("binned_finalize", &binned_finalize);
}

TORCH_LIBRARY_IMPL(torcheval_amd, Meta, m) {
  m.impl("micro_accuracy", &MetaNoop<&op_micro_accuracy>::call);
  m.impl("cls_counts", &MetaNoop<&op_cls_counts>::call);
  m.impl("binary_counts", &MetaNoop<&op_binary_counts>::call);
  m.impl("multilabel_counts", &MetaNoop<&multilabel_counts>::call);
  m.impl("rank_scores", [](const Tensor& input, const Tensor&, int64_t, int64_t, const optional<Tensor>&) {
    return at::empty({input.size(0)}, input.options().dtype(at::kFloat));
  });
  m.impl("binned_counts", &MetaNoop<&op_binned_counts>::call);
  m.impl("binned_finalize", &MetaNoop<&binned_finalize>::call);
}
