// torcheval_amd._C bindings (layout: module.cpp): K3m sorted-run merge, K10b retrieval top-k, K12 SSIM, K13 NDCG,
// the C3 sync kernels.
#include <ATen/ATen.h>
#include <torch/csrc/utils/pybind.h>
#include <torch/library.h>

#include <cmath>
#include <mutex>
#include <unordered_map>

#include "tea_kernels.h"
#include "tea_torch.h"

namespace {

using namespace tea_torch;

// ---------------------------------------------------------------- K3m sorted-run merge
// keys: R 1-D float32 runs, each sorted descending (NaN first).  payloads: optional R 32-bit
// runs carried with their keys (e.g. the f32 target of each sample, so K3 needs no gather);
// without them the payload is each sample's position in the concatenation of the runs.
// Returns (merged keys, merged int32 payload): log2(R) pairwise merge rounds - the merge-path
// kernel on ROCm tensors, a stable host merge on CPU tensors.  The first round reads the runs
// in place (no concatenation copy) and positions are generated there (no arange).
std::vector<Tensor> merge_sorted_runs(const std::vector<Tensor>& keys, const optional<std::vector<Tensor>>& payloads) {
  TORCH_CHECK(!keys.empty(), "merge_sorted_runs: no runs");
  const bool carry = payloads.has_value();
  TORCH_CHECK(!carry || payloads->size() == keys.size(), "merge_sorted_runs: one payload per run");
  const auto dev = keys[0].device();
  const bool gpu = keys[0].is_cuda();
  int64_t n = 0;
  std::vector<int64_t> len;
  for (size_t r = 0; r < keys.size(); ++r) {
    const Tensor& k = keys[r];
    TORCH_CHECK(k.dim() == 1 && k.scalar_type() == at::kFloat && k.is_contiguous() && k.device() == dev,
                "merge_sorted_runs: keys must be contiguous float32 [n] runs on one device");
    if (carry) {
      const Tensor& v = (*payloads)[r];
      TORCH_CHECK(v.dim() == 1 && v.numel() == k.numel() && v.is_contiguous() && v.element_size() == 4 &&
                      v.device() == dev,
                  "merge_sorted_runs: payloads must be contiguous 32-bit runs matching the keys");
    }
    len.push_back(k.numel());
    n += k.numel();
  }
  TORCH_CHECK(n < (int64_t{1} << 31), "merge_sorted_runs: fewer than 2^31 samples");
  const auto fopt = keys[0].options();
  Tensor k0 = at::empty({n}, fopt), v0 = at::empty({n}, fopt.dtype(at::kInt));
  Tensor k1 = at::empty({n}, fopt), v1 = at::empty({n}, fopt.dtype(at::kInt));
  DeviceGuard guard(gpu ? c10::optional<c10::Device>(dev) : c10::nullopt);
  hipStream_t st = gpu ? stream_for(keys[0]) : nullptr;
  // split scratch for the largest pair (every pair of a round is stream-ordered after the last)
  Tensor splits = gpu ? at::empty({tea::merge_splits_count(n)}, fopt.dtype(at::kLong)) : Tensor();
  auto lt = [](float x, float y) {  // descending, NaN first: x goes before y
    const bool xn = x != x, yn = y != y;
    if (xn || yn) return xn && !yn;
    return x > y;
  };
  // one stable two-run merge; va / vb null: payload = base + index
  auto merge2 = [&](const float* ka, const uint32_t* va, int64_t na, uint32_t base_a, const float* kb,
                    const uint32_t* vb, int64_t nb, uint32_t base_b, float* ko, uint32_t* vo) {
    if (gpu) {
      check_launch(tea::launch_merge_desc(ka, va, na, base_a, kb, vb, nb, base_b, ko, vo, splits.data_ptr<int64_t>(), st),
                   "merge_sorted_runs");
      return;
    }
    int64_t i = 0, j = 0, o = 0;
    while (i < na || j < nb) {
      const bool take_a = j >= nb || (i < na && !lt(kb[j], ka[i]));
      if (take_a) {
        ko[o] = ka[i];
        vo[o] = va ? va[i] : base_a + static_cast<uint32_t>(i);
        ++i;
      } else {
        ko[o] = kb[j];
        vo[o] = vb ? vb[j] : base_b + static_cast<uint32_t>(j);
        ++j;
      }
      ++o;
    }
  };
  auto pay = [&](size_t r) -> const uint32_t* {
    return carry ? static_cast<const uint32_t*>((*payloads)[r].data_ptr()) : nullptr;
  };
  // round 1: from the runs in place into (k0, v0)
  std::vector<int64_t> runs;
  {
    float* ko = k0.data_ptr<float>();
    uint32_t* vo = reinterpret_cast<uint32_t*>(v0.data_ptr<int32_t>());
    int64_t off = 0;
    for (size_t r = 0; r < keys.size(); r += 2) {
      const int64_t na = len[r], nb = r + 1 < keys.size() ? len[r + 1] : 0;
      const float* ka = keys[r].data_ptr<float>();
      const float* kb = nb ? keys[r + 1].data_ptr<float>() : ka;
      merge2(ka, pay(r), na, static_cast<uint32_t>(off), kb, nb ? pay(r + 1) : nullptr, nb,
             static_cast<uint32_t>(off + na), ko + off, vo + off);
      runs.push_back(na + nb);
      off += na + nb;
    }
  }
  while (runs.size() > 1) {
    std::vector<int64_t> next;
    int64_t off = 0;
    const float* ki = k0.data_ptr<float>();
    const uint32_t* vi = reinterpret_cast<const uint32_t*>(v0.data_ptr<int32_t>());
    float* ko = k1.data_ptr<float>();
    uint32_t* vo = reinterpret_cast<uint32_t*>(v1.data_ptr<int32_t>());
    for (size_t r = 0; r < runs.size(); r += 2) {
      const int64_t na = runs[r], nb = r + 1 < runs.size() ? runs[r + 1] : 0;
      // (an odd run out is "merged" with an empty run: one pass-through copy)
      merge2(ki + off, vi + off, na, 0, ki + off + na, vi + off + na, nb, 0, ko + off, vo + off);
      next.push_back(na + nb);
      off += na + nb;
    }
    std::swap(k0, k1);
    std::swap(v0, v1);
    runs.swap(next);
  }
  return {k0, v0};
}

// ---------------------------------------------------------------- K10b retrieval top-k
// Merges a batch into RetrievalPrecision's [Q, k] top-k state rows in place (see
// retrieval.hip).  x, t: float32 [n]; q: int64 [n] query ids or None (all query 0).
void retrieval_topk_update(const Tensor& x, const Tensor& t, const optional<Tensor>& q, const Tensor& topk,
                           const Tensor& target, const Tensor& count) {
  check_gpu(x, "scores");
  const int64_t n = x.numel();
  TORCH_CHECK(x.dim() == 1 && x.scalar_type() == at::kFloat && x.is_contiguous(), "retrieval_topk: x must be f32 [n]");
  TORCH_CHECK(t.dim() == 1 && t.numel() == n && t.scalar_type() == at::kFloat && t.is_contiguous() &&
                  t.device() == x.device(), "retrieval_topk: t must be f32 [n]");
  TORCH_CHECK(topk.dim() == 2 && topk.scalar_type() == at::kFloat && topk.is_contiguous() &&
                  target.sizes() == topk.sizes() && target.scalar_type() == at::kFloat && target.is_contiguous() &&
                  topk.device() == x.device() && target.device() == x.device(),
              "retrieval_topk: state rows must be contiguous f32 [Q, k]");
  const int64_t Q = topk.size(0), k = topk.size(1);
  TORCH_CHECK(count.dim() == 1 && count.numel() == Q && count.scalar_type() == at::kLong && count.is_contiguous() &&
                  count.device() == x.device(), "retrieval_topk: count must be int64 [Q]");
  TORCH_CHECK(k >= 1 && k <= 64 && 2 * Q * 4 <= tea::kRetrievalMaxLds && n < (int64_t{1} << 31),
              "retrieval_topk: needs 1 <= k <= 64, Q <= 8192, n < 2^31");
  DeviceGuard guard(x.device());
  tea::RetrievalArgs a;
  a.x = x.data_ptr<float>();
  a.t = t.data_ptr<float>();
  if (q.has_value()) {
    TORCH_CHECK(q->dim() == 1 && q->numel() == n && q->scalar_type() == at::kLong && q->is_contiguous() &&
                    q->device() == x.device(), "retrieval_topk: q must be int64 [n]");
    a.q = q->data_ptr<int64_t>();
  }
  a.n = n;
  a.Q = Q;
  a.k = static_cast<int>(k);
  a.topk = topk.data_ptr<float>();
  a.target_state = target.data_ptr<float>();
  a.count = count.data_ptr<int64_t>();
  hipStream_t st = stream_for(x);
  a.counts = static_cast<int*>(zeroed_workspace(x, st, Q * 4, Zeroed::kRetrievalCounts));
  auto* ws = static_cast<char*>(scratch_workspace(x, st, (2 * Q + 2) * 4 + 2 * n * 4, Scratch::kRetrievalRecords));
  a.offsets = reinterpret_cast<int*>(ws);
  a.cursor = a.offsets + Q + 1;
  a.rec_key = reinterpret_cast<uint32_t*>(a.cursor + Q + 1);
  a.rec_idx = a.rec_key + n;
  check_launch(tea::launch_retrieval_topk(a, st), "retrieval_topk_update");
}

// K12: structural similarity (csrc/kernels/ssim.hip).  ``out`` takes the [n] per-image values, or
// their mean when ``mean``; the optional class states take += sum of the values and += n.
void ssim(const Tensor& input, const Tensor& target, const std::vector<double>& taps, double c1, double c2,
          const optional<Tensor>& out, bool mean, const optional<Tensor>& mssim_sum,
          const optional<Tensor>& num_images) {
  check_gpu(input, "input");
  TORCH_CHECK(input.dim() == 4 && input.is_contiguous() && input.numel() > 0,
              "ssim: input must be a contiguous, non-empty [n, c, h, w] tensor");
  TORCH_CHECK(target.sizes() == input.sizes() && target.is_contiguous() && target.device() == input.device() &&
                  target.scalar_type() == input.scalar_type(),
              "ssim: target must be contiguous with the shape, dtype and device of input");
  const auto st = input.scalar_type();
  TORCH_CHECK(st == at::kFloat || st == at::kHalf || st == at::kBFloat16 || st == at::kByte,
              "ssim: inputs must be float32, float16, bfloat16 or uint8");
  const int64_t ks = static_cast<int64_t>(taps.size());
  const int64_t n = input.size(0), c = input.size(1), h = input.size(2), w = input.size(3);
  TORCH_CHECK(tea::ssim_geometry_ok(n * c, h, w, ks), "ssim: unsupported geometry (odd window of 3..",
              tea::kSsimMaxKs, " taps no larger than the image, at most ", tea::kSsimMaxPlanes, " planes)");
  TORCH_CHECK(out.has_value() || mssim_sum.has_value(), "ssim: nothing to write");
  TORCH_CHECK(mssim_sum.has_value() == num_images.has_value(), "ssim: pass both class states or neither");
  tea::SsimArgs a;
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
  a.mean = mean ? 1 : 0;
  a.out = f32_out(out, input, mean ? 1 : n, "out");
  check_f64_scalar_states({&mssim_sum, &num_images}, input, "ssim");
  if (mssim_sum.has_value()) {
    a.mssim_sum = mssim_sum->data_ptr<double>();
    a.num_images = num_images->data_ptr<double>();
  }
  DeviceGuard guard(input.device());
  const hipStream_t stream = stream_for(input);
  a.partial = static_cast<double*>(
      scratch_workspace(input, stream, n * c * tea::ssim_tiles(h, w, ks) * 8, Scratch::kSsimPartials));
  check_launch(tea::launch_ssim(a, stream), "ssim");
}

// K13: normalized DCG per row (csrc/kernels/ndcg.hip).  ``out`` takes the [n] float32 row values;
// the optional class states take += sum of the (unrounded) values and += n; ``err`` gets bit 0
// when a relevance is negative or NaN.
//
// The discount prefix table D[0] = 0, D[m] = sum_{r < m} 1 / log2(r + 2) does not depend on the
// cutoff, so one table of kNdcgMaxColumns + 1 doubles per device serves every call: summed
// sequentially in FP64 on the host, copied once.  Warm it up before any HIP-graph capture.
const double* ndcg_discounts(const Tensor& like) {
  static std::mutex mu;
  // process-lifetime (never destroyed), as the workspaces of tea_torch.h
  static auto& cache = *new std::unordered_map<int, Tensor>();
  std::lock_guard<std::mutex> lock(mu);
  const int dev = like.device().index();
  auto it = cache.find(dev);
  if (it == cache.end()) {
    Tensor host = at::empty({tea::kNdcgMaxColumns + 1}, at::TensorOptions().dtype(at::kDouble));
    double* d = host.data_ptr<double>();
    d[0] = 0.0;
    for (int r = 0; r < tea::kNdcgMaxColumns; ++r) d[r + 1] = d[r] + 1.0 / std::log2(static_cast<double>(r) + 2.0);
    it = cache.emplace(dev, host.to(like.device())).first;
  }
  return it->second.data_ptr<double>();
}

void ndcg(const Tensor& input, const Tensor& target, int64_t k, bool exponential_gain,
          const optional<Tensor>& out, const optional<Tensor>& ndcg_sum, const optional<Tensor>& num_rows,
          const optional<Tensor>& err) {
  check_gpu(input, "input");
  check_gpu(target, "target");
  TORCH_CHECK(input.dim() == 2 && target.sizes() == input.sizes() && target.device() == input.device(),
              "ndcg: input and target must be [n, c] tensors of one shape on one device");
  const int64_t n = input.size(0), c = input.size(1);
  TORCH_CHECK(c >= 1 && c <= tea::kNdcgMaxColumns, "ndcg: 1 .. ", tea::kNdcgMaxColumns, " columns, got ", c);
  TORCH_CHECK(k >= 1 && k <= c, "ndcg: the cutoff must lie in 1 .. c, got ", k);
  TORCH_CHECK((c == 1 || (input.stride(1) == 1 && target.stride(1) == 1)) && input.stride(0) >= 0 &&
                  target.stride(0) >= 0,
              "ndcg: input and target need a unit column stride");
  const auto xt = input.scalar_type(), tt = target.scalar_type();
  TORCH_CHECK(xt == at::kFloat || xt == at::kHalf || xt == at::kBFloat16,
              "ndcg: scores must be float32, float16 or bfloat16");
  TORCH_CHECK(tt == at::kFloat || tt == at::kHalf || tt == at::kBFloat16 || tt == at::kLong || tt == at::kInt ||
                  tt == at::kShort || tt == at::kChar || tt == at::kByte,
              "ndcg: unsupported relevance dtype ", tt);
  TORCH_CHECK(out.has_value() || ndcg_sum.has_value(), "ndcg: nothing to write");
  TORCH_CHECK(ndcg_sum.has_value() == num_rows.has_value(), "ndcg: pass both class states or neither");
  if (n == 0) return;
  tea::NdcgArgs a;
  a.x = input.data_ptr();
  a.x_dt = dt_of(input);
  a.x_stride = input.stride(0);
  a.t = target.data_ptr();
  a.t_dt = dt_of(target);
  a.t_stride = target.stride(0);
  a.n = n;
  a.c = static_cast<int>(c);
  a.k = static_cast<int>(k);
  a.exponential = exponential_gain ? 1 : 0;
  a.out = f32_out(out, input, n, "out");
  check_f64_scalar_states({&ndcg_sum, &num_rows}, input, "ndcg");
  a.err = err_ptr(err, input, "ndcg");
  DeviceGuard guard(input.device());
  const hipStream_t stream = stream_for(input);
  a.D = ndcg_discounts(input);
  if (ndcg_sum.has_value()) {
    a.ndcg_sum = ndcg_sum->data_ptr<double>();
    a.num_rows = num_rows->data_ptr<double>();
    a.partial = static_cast<double*>(scratch_workspace(input, stream, tea::ndcg_blocks(n, c) * 8, Scratch::kNdcgPartials));
  }
  check_launch(tea::launch_ndcg(a, stream), "ndcg");
}

// ---------------------------------------------------------------- C3 flags inside the all-reduce
void snapshot_flags(const Tensor& src, const Tensor& dst, const optional<Tensor>& err, int64_t words, int64_t rank,
                    int64_t ws) {
  check_gpu(src, "src");
  TORCH_CHECK(src.scalar_type() == at::kByte && dst.scalar_type() == at::kByte && src.is_contiguous() &&
                  dst.is_contiguous() && dst.device() == src.device() && src.numel() % 16 == 0 &&
                  dst.numel() == src.numel() + ws * words * 8,
              "snapshot_flags: uint8 src [16k] and dst [src + ws * words * 8] on one device");
  const int* e = nullptr;
  if (err.has_value()) {
    TORCH_CHECK(err->scalar_type() == at::kInt && err->numel() >= words && err->device() == src.device(),
                "snapshot_flags: err must be int32 [>= words]");
    e = err->data_ptr<int>();
  }
  DeviceGuard guard(src.device());
  check_launch(tea::launch_snapshot_flags(src.data_ptr(), dst.data_ptr(), src.numel(), e, (int)words, (int)rank, (int)ws,
                                          stream_for(src)),
               "snapshot_flags");
}

void merge_flag_slots(const Tensor& slots, const Tensor& out, int64_t words, int64_t ws) {
  check_gpu(slots, "slots");
  TORCH_CHECK(slots.scalar_type() == at::kFloat && slots.is_contiguous() && slots.numel() == ws * words * 2 &&
                  out.scalar_type() == at::kInt && out.numel() == words && out.device() == slots.device(),
              "merge_flag_slots: float32 [ws * words * 2] slots and int32 [words] out");
  DeviceGuard guard(slots.device());
  check_launch(tea::launch_merge_flag_slots(slots.data_ptr<float>(), out.data_ptr<int>(), (int)words, (int)ws,
                                            stream_for(slots)),
               "merge_flag_slots");
}

// ---------------------------------------------------------------- C3 gathered-state reduction
void seg_reduce_rows(const Tensor& rows, const Tensor& out, int64_t ws, at::IntArrayRef offs,
                     at::IntArrayRef counts, at::IntArrayRef dtypes, at::IntArrayRef ops) {
  check_gpu(rows, "rows");
  TORCH_CHECK(rows.scalar_type() == at::kByte && out.scalar_type() == at::kByte && rows.is_contiguous() &&
                  out.is_contiguous() && out.device() == rows.device(),
              "seg_reduce_rows: contiguous uint8 rows / out on one device expected");
  const int64_t nseg = static_cast<int64_t>(offs.size());
  TORCH_CHECK(nseg >= 1 && nseg <= tea::kSegMax && counts.size() == offs.size() && dtypes.size() == offs.size() &&
                  ops.size() == offs.size(),
              "seg_reduce_rows: 1..", tea::kSegMax, " segments with offs / counts / dtypes / ops each");
  TORCH_CHECK(ws >= 1 && rows.numel() == ws * out.numel(), "seg_reduce_rows: rows must be [ws * row_bytes]");
  static const int esize[] = {4, 2, 2, 8, 8, 4, 1, 1, 1, 2};  // by tea::DType
  tea::SegReduceArgs a;
  a.rows = rows.data_ptr<uint8_t>();
  a.out = out.data_ptr<uint8_t>();
  a.ws = static_cast<int>(ws);
  a.row_bytes = out.numel();
  a.nseg = static_cast<int>(nseg);
  for (int64_t s = 0; s < nseg; ++s) {
    TORCH_CHECK(dtypes[s] >= 0 && dtypes[s] <= 9 && ops[s] >= 0 && ops[s] <= 2 && counts[s] >= 0,
                "seg_reduce_rows: bad segment ", s);
    const int es = esize[dtypes[s]];
    TORCH_CHECK(offs[s] >= 0 && offs[s] % es == 0 && offs[s] + counts[s] * es <= a.row_bytes,
                "seg_reduce_rows: segment ", s, " outside the row or misaligned");
    a.off[s] = offs[s];
    a.first[s + 1] = a.first[s] + counts[s];
    a.dtype[s] = static_cast<int>(dtypes[s]);
    a.op[s] = static_cast<int>(ops[s]);
  }
  DeviceGuard guard(rows.device());
  check_launch(tea::launch_seg_reduce(a, stream_for(rows)), "seg_reduce_rows");
}

// ---------------------------------------------------------------- dispatcher forms
// (the dispatcher passes lists as ArrayRef where these two take std::vector)
std::vector<Tensor> op_merge_sorted_runs(at::TensorList keys, at::TensorList payloads) {
  optional<std::vector<Tensor>> pays;
  if (!payloads.empty()) pays = payloads.vec();  // [] = no payloads (positions come back)
  return merge_sorted_runs(keys.vec(), pays);
}
void op_ssim(const Tensor& input, const Tensor& target, at::ArrayRef<double> taps, double c1, double c2,
             const optional<Tensor>& out, bool mean, const optional<Tensor>& mssim_sum,
             const optional<Tensor>& num_images) {
  ssim(input, target, taps.vec(), c1, c2, out, mean, mssim_sum, num_images);
}

}  // namespace

void tea_bind_misc(py::module_& m) {
  m.def("snapshot_flags", &snapshot_flags, "C3 snapshot of a state region + this rank's flag slot (f32 hi/lo)",
        py::arg("src"), py::arg("dst"), py::arg("err"), py::arg("words"), py::arg("rank"), py::arg("ws"));
  m.def("merge_flag_slots", &merge_flag_slots, "C3 summed flag slots -> int32 words (max over ranks)", py::arg("slots"),
        py::arg("out"), py::arg("words"), py::arg("ws"));
  m.def("seg_reduce_rows", &seg_reduce_rows,
        "C3 reduce a gathered [ws][row] state buffer per (op, dtype) segment in one launch", py::arg("rows"),
        py::arg("out"), py::arg("ws"), py::arg("offs"), py::arg("counts"), py::arg("dtypes"), py::arg("ops"));
  m.def("merge_sorted_runs", &merge_sorted_runs,
        "K3m merge of descending-sorted runs -> (keys, int32 payload: carried or positions)", py::arg("keys"),
        py::arg("payloads") = py::none());
  m.def("retrieval_topk_update", &retrieval_topk_update,
        "K10b segmented streaming top-k merge into RetrievalPrecision state rows", py::arg("x"), py::arg("t"),
        py::arg("q"), py::arg("topk"), py::arg("target"), py::arg("count"));
  m.def("ssim", &ssim, "K12 structural similarity: per-image values or their mean, optional class states",
        py::arg("input"), py::arg("target"), py::arg("taps"), py::arg("c1"), py::arg("c2"), py::arg("out"),
        py::arg("mean"), py::arg("mssim_sum") = py::none(), py::arg("num_images") = py::none());
  m.def("ssim_tile_rows", [] { return tea::kSsimTileH; }, "K12 output tile rows");
  m.def("ssim_tile_cols", [] { return tea::kSsimTileW; }, "K12 output tile columns");
  m.def("ssim_max_kernel_size", [] { return tea::kSsimMaxKs; }, "K12 largest native window");
  m.def("ssim_geometry_ok", &tea::ssim_geometry_ok, "K12 launchable (planes, h, w, kernel_size)");
  m.def("ndcg", &ndcg, "K13 normalized DCG per row: float32 row values, optional class states and error flag",
        py::arg("input"), py::arg("target"), py::arg("k"), py::arg("exponential_gain"), py::arg("out"),
        py::arg("ndcg_sum") = py::none(), py::arg("num_rows") = py::none(), py::arg("err") = py::none());
  m.def("ndcg_max_columns", [] { return tea::kNdcgMaxColumns; }, "K13 largest native row width");
}

TORCH_LIBRARY_FRAGMENT(torcheval_amd, m) {
  // no Meta kernel: it allocates and returns its outputs, and its callers reach it through the
  // pybind entry point in a metric's compute, outside the compiled update loops
  m.def("merge_sorted_runs(Tensor[] keys, Tensor[] payloads) -> Tensor[]");
  m.def("retrieval_topk_update(Tensor x, Tensor t, Tensor? q, Tensor(a!) topk, Tensor(b!) target, "
        "Tensor(c!) count) -> ()");
  m.def("ssim(Tensor input, Tensor target, float[] taps, float c1, float c2, Tensor(a!)? out, bool mean, "
        "Tensor(b!)? mssim_sum, Tensor(c!)? num_images) -> ()");
  m.def("ndcg(Tensor input, Tensor target, int k, bool exponential_gain, Tensor(a!)? out, "
        "Tensor(b!)? ndcg_sum, Tensor(c!)? num_rows, Tensor(d!)? err) -> ()");
  m.def("seg_reduce_rows(Tensor rows, Tensor(a!) out, int ws, int[] offs, int[] counts, int[] dtypes, "
        "int[] ops) -> ()");
}

TORCH_LIBRARY_IMPL(torcheval_amd, CUDA, m) {
  m.impl("merge_sorted_runs", &op_merge_sorted_runs);
  m.impl("retrieval_topk_update", &retrieval_topk_update);
  m.impl("ssim", &op_ssim);
  m.impl("ndcg", &ndcg);
  m.impl("seg_reduce_rows", &seg_reduce_rows);
}

TORCH_LIBRARY_IMPL(torcheval_amd, Meta, m) {
  m.impl("retrieval_topk_update", &MetaNoop<&retrieval_topk_update>::call);
  m.impl("ssim", &MetaNoop<&op_ssim>::call);
  m.impl("ndcg", &MetaNoop<&ndcg>::call);
  m.impl("seg_reduce_rows", &MetaNoop<&seg_reduce_rows>::call);
}
