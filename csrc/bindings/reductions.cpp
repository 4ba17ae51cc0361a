// torcheval_amd._C bindings (layout: module.cpp): K5 column moments, K5b per-row sums, K6 normalized-entropy
// sums, K7 perplexity.
#include <ATen/ATen.h>
#include <torch/csrc/utils/pybind.h>
#include <torch/library.h>

#include <cstdlib>

#include "tea_kernels.h"
#include "tea_torch.h"

namespace {

using namespace tea_torch;

// ---------------------------------------------------------------- K5b per-row weighted sums
// x: [rows, n] view (t, w: the same shape, any strides; w may be absent -> w_scalar).
// outs[k] receives stat codes[k] / 8 with op codes[k] % 4 (see tea::RowStat / tea::RowOp), bit 2
// of the code = row 0 only (a scalar state): f32 / f64 tensors of `rows` elements (any stride:
// a ring-buffer column works), or of one element for row-0-only outputs.  CUDA tensors
// run K5b (one launch, two for rows > 32768 elements); CPU tensors the host twin.
static tea::RowSumsArgs row_sums_args(const Tensor& x_in, const optional<Tensor>& t_in, const optional<Tensor>& w_in,
                                      double w_scalar, const std::vector<Tensor>& outs,
                                      const std::vector<int64_t>& codes, int64_t rows, Tensor* x_out,
                                      bool reads_inputs = true) {
  // any shape: a [rows, n] view is used as is, anything else is viewed as rows x (numel / rows)
  auto as_rows = [&](const Tensor& v) -> Tensor {
    if (v.dim() == 2 && v.size(0) == rows) return v;
    TORCH_CHECK(rows > 0 && v.numel() % rows == 0, "row_sums: numel not divisible by rows");
    return v.reshape({rows, v.numel() / rows});
  };
  const Tensor x = as_rows(x_in);
  const optional<Tensor> t = t_in.has_value() ? optional<Tensor>(as_rows(*t_in)) : c10::nullopt;
  const optional<Tensor> w = w_in.has_value() ? optional<Tensor>(as_rows(*w_in)) : c10::nullopt;
  TORCH_CHECK(outs.size() == codes.size() && outs.size() <= static_cast<size_t>(tea::kRowSumsMaxOut),
              "row_sums: outs / codes mismatch");
  const bool gpu = x.is_cuda();
  tea::RowSumsArgs a;
  a.rows = x.size(0);
  a.n = x.size(1);
  auto bind_in = [&](const Tensor& v, const void*& p, tea::DType& dt, int64_t& rs, int64_t& cs, const char* nm) {
    TORCH_CHECK(v.dim() == 2 && v.size(0) == a.rows && v.size(1) == a.n, "row_sums: ", nm, " must match x");
    TORCH_CHECK(v.is_cuda() == gpu && (!gpu || v.device() == x.device()), "row_sums: ", nm, " on another device");
    p = v.data_ptr();
    dt = dt_of(v);
    rs = v.stride(0);
    cs = v.stride(1);
  };
  bind_in(x, a.x, a.x_dt, a.x_rs, a.x_cs, "x");
  if (t.has_value()) bind_in(*t, a.t, a.t_dt, a.t_rs, a.t_cs, "t");
  if (w.has_value()) bind_in(*w, a.w, a.w_dt, a.w_rs, a.w_cs, "w");
  a.w_scalar = w_scalar;
  a.nout = static_cast<int>(outs.size());
  int need = 0;
  for (size_t k = 0; k < outs.size(); ++k) {
    const Tensor& o = outs[k];
    TORCH_CHECK(o.scalar_type() == at::kFloat || o.scalar_type() == at::kDouble, "row_sums: outputs must be f32/f64");
    const bool first = (codes[k] & 4) != 0;
    TORCH_CHECK((o.numel() == a.rows || (first && o.numel() == 1)) && o.is_cuda() == gpu,
                "row_sums: output ", k, " must hold rows elements");
    TORCH_CHECK(o.dim() <= 1, "row_sums: outputs must be 0-d or 1-d");
    a.out[k].p = o.data_ptr();
    a.out[k].dt = o.scalar_type() == at::kFloat ? tea::DType::f32 : tea::DType::f64;
    a.out[k].stride = o.dim() == 1 ? o.stride(0) : 0;
    a.out[k].stat = static_cast<int>(codes[k] / 8);
    a.out[k].op = static_cast<int>(codes[k] % 4);
    a.out[k].first_row_only = first ? 1 : 0;
    TORCH_CHECK(a.out[k].stat >= 0 && a.out[k].stat <= tea::kRANGE, "row_sums: bad stat");
    if (a.out[k].stat < tea::kCOUNT) need |= 1 << a.out[k].stat;
    if (a.out[k].stat == tea::kRANGE) need |= (1 << tea::kTMIN) | (1 << tea::kTMAX);
  }
  // WT, SSE, WSSE, WTT, TMIN, TMAX (and RANGE through the last two) read the target: without one
  // the kernel would load through a null pointer and the host twin would take t as 0 (the fold of
  // pending slots reads no input at all)
  constexpr int need_t = (1 << tea::kWT) | (1 << tea::kSSE) | (1 << tea::kWSSE) | (1 << tea::kWTT) |
                         (1 << tea::kTMIN) | (1 << tea::kTMAX);
  TORCH_CHECK(!reads_inputs || t.has_value() || (need & need_t) == 0,
              "row_sums: a statistic that reads the target needs t");
  a.need = need;
  *x_out = x;
  return a;
}

void row_sums(const Tensor& x_in, const optional<Tensor>& t_in, const optional<Tensor>& w_in, double w_scalar,
              const std::vector<Tensor>& outs, const std::vector<int64_t>& codes, int64_t rows) {
  Tensor x;
  tea::RowSumsArgs a = row_sums_args(x_in, t_in, w_in, w_scalar, outs, codes, rows, &x);
  const bool gpu = x.is_cuda();
  if (!gpu) {
    tea::row_sums_host(a);
    return;
  }
  DeviceGuard guard(x.device());
  // long rows: partials + ordered combine in two launches by default (TORCHEVAL_AMD_K5B_MODE=1:
  // the fat-block fold with a release fence per block; =2: one launch with write-through
  // partials and a last-block combine - measured 14.5 vs 11.4 us for Sum 8192 x 1000,
  // profiles/odd_width_cliff_r5_k5.json: the hand-off sits on the launch's tail)
  static const int mode = [] {
    const char* e = std::getenv("TORCHEVAL_AMD_K5B_MODE");
    return (e != nullptr && e[0] != '\0') ? std::atoi(e) : 0;
  }();
  a.blocks = mode == 0 ? tea::row_sums_blocks(a.rows, a.n)
                       : mode == 1 ? tea::row_sums_fold_blocks(a.rows, a.n) : tea::row_sums_wt_blocks(a.rows, a.n);
  if (a.blocks > 1) {  // stream-ordered scratch, fully rewritten by every call: cached, no allocation
    a.ws = static_cast<double*>(
        zeroed_workspace(x, stream_for(x), a.rows * a.blocks * tea::kRowRaw * 8, Zeroed::kRowSumsPartials));
    if (mode != 0) {  // self-cleaning arrival tickets
      a.ticket = static_cast<unsigned*>(zeroed_workspace(x, stream_for(x), a.rows * 4, Zeroed::kRowSumsTickets));
      a.wt = mode == 2;
    }
  }
  if (a.n == 0 && a.rows > 0) a.blocks = 1;
  check_launch(tea::launch_row_sums(a, stream_for(x)), "row_sums");
}

// deferred-mode K5b update (rows longer than one block; ADD outputs of sums / W / COUNT): the
// grid blocks add their pre-scaled FP64 partials to their slots of `pend` (float64, zeroed,
// rows * kRowPendStats * kRowPendBlocks); returns the blocks used (0: not applicable, the
// caller runs row_sums).  row_sums_fold applies the slots to the same outputs and zeroes them.
int64_t row_sums_pend(const Tensor& x_in, const optional<Tensor>& t_in, const optional<Tensor>& w_in,
                      double w_scalar, const std::vector<Tensor>& outs, const std::vector<int64_t>& codes,
                      int64_t rows, const Tensor& pend) {
  Tensor x;
  tea::RowSumsArgs a = row_sums_args(x_in, t_in, w_in, w_scalar, outs, codes, rows, &x);
  if (!x.is_cuda() || a.n == 0) return 0;
  for (int k = 0; k < a.nout; ++k) {  // sums / COUNT added, extrema min / max, RANGE set
    const auto& o = a.out[k];
    const bool ok = o.stat == tea::kTMIN ? o.op == tea::kMin : o.stat == tea::kTMAX ? o.op == tea::kMax
                  : o.stat == tea::kRANGE ? o.op == tea::kSet : o.op == tea::kAdd;
    if (!ok) return 0;
  }
  const int blocks = tea::row_sums_blocks(a.rows, a.n);
  if (blocks < 2 || blocks > tea::kRowPendBlocks) return 0;
  TORCH_CHECK(pend.scalar_type() == at::kDouble && pend.is_contiguous() && pend.device() == x.device() &&
                  pend.numel() >= a.rows * tea::kRowPendStats * tea::kRowPendBlocks,
              "row_sums_pend: pend must be float64 [rows * ", tea::kRowPendStats, " * ", tea::kRowPendBlocks, "]");
  DeviceGuard guard(x.device());
  a.blocks = blocks;
  a.pend = pend.data_ptr<double>();
  a.pend_blocks = tea::kRowPendBlocks;
  check_launch(tea::launch_row_sums(a, stream_for(x)), "row_sums_pend");
  return blocks;
}

void row_sums_fold(const Tensor& pend, int64_t used, const std::vector<Tensor>& outs,
                   const std::vector<int64_t>& codes, int64_t rows) {
  TORCH_CHECK(!outs.empty(), "row_sums_fold: no outputs");
  const Tensor carrier = at::empty({rows, 0}, pend.options().dtype(at::kFloat));
  Tensor x;
  tea::RowSumsArgs a = row_sums_args(carrier, c10::nullopt, c10::nullopt, 1.0, outs, codes, rows, &x, false);
  TORCH_CHECK(pend.scalar_type() == at::kDouble && pend.is_cuda() &&
                  pend.numel() >= a.rows * tea::kRowPendStats * tea::kRowPendBlocks,
              "row_sums_fold: bad pend buffer");
  DeviceGuard guard(pend.device());
  a.pend = pend.data_ptr<double>();
  a.pend_blocks = tea::kRowPendBlocks;
  check_launch(tea::launch_row_sums_fold(a, static_cast<int>(used), stream_for(pend)), "row_sums_fold");
}

// ---------------------------------------------------------------- K5 / K6 reductions
// x, t: [n, d] views (t optional); w: optional [n]; outputs float32 (accumulated):
// sse/st/stt/sx as [d] views sharing one stride, sw scalar.
// x, t: [n, d] views; w: [n]; outputs float32 [d] sharing a stride, sw scalar (shared by
// column_moments / column_moments_pend / column_moments_fold)
static tea::MomentsArgs moments_args(const optional<Tensor>& x, const optional<Tensor>& t,
                                     const optional<Tensor>& w, const optional<Tensor>& sse,
                                     const optional<Tensor>& st, const optional<Tensor>& stt,
                                     const optional<Tensor>& sx, const optional<Tensor>& sw, const Tensor& ref) {
  tea::MomentsArgs a;
  a.n = ref.size(0);
  a.d = ref.size(1);
  if (x.has_value()) {
    TORCH_CHECK(x->sizes() == ref.sizes(), "column_moments: x shape");
    a.x = x->data_ptr();
    a.x_dt = dt_of(*x);
    a.x_row_stride = x->stride(0);
    a.x_col_stride = x->stride(1);
  }
  if (t.has_value()) {
    TORCH_CHECK(t->sizes() == ref.sizes(), "column_moments: t shape must match x");
    a.t = t->data_ptr();
    a.t_dt = dt_of(*t);
    a.t_row_stride = t->stride(0);
    a.t_col_stride = t->stride(1);
  }
  if (w.has_value()) {
    TORCH_CHECK(w->dim() == 1 && w->size(0) == a.n, "column_moments: w must be [n]");
    a.w = w->data_ptr();
    a.w_dt = dt_of(*w);
    a.w_stride = w->stride(0);
  }
  int64_t os = -1;
  auto out = [&](const optional<Tensor>& o, const char* name) -> float* {
    if (!o.has_value()) return nullptr;
    TORCH_CHECK(o->scalar_type() == at::kFloat && o->numel() == a.d && o->device() == ref.device(),
                "column_moments: ", name, " must be float32 with d elements");
    const int64_t s = o->dim() == 0 ? 1 : o->stride(-1);
    TORCH_CHECK(os < 0 || os == s, "column_moments: outputs must share a stride");
    os = s;
    return o->data_ptr<float>();
  };
  a.sse = out(sse, "sse");
  a.st = out(st, "st");
  a.stt = out(stt, "stt");
  a.sx = out(sx, "sx");
  a.out_stride = os < 0 ? 1 : os;
  if (sw.has_value()) {
    TORCH_CHECK(sw->scalar_type() == at::kFloat && sw->numel() == 1, "column_moments: sw scalar f32");
    a.sw = sw->data_ptr<float>();
  }
  return a;
}

// deferred-mode pend buffer size for d columns and statistic set `need` (the one place the
// slot layout is computed; Python sizes its buffers from here)
int64_t column_moments_pend_numel(int64_t d, int64_t need) {
  const int ns = tea::moments_ns_of(static_cast<int>(need));
  TORCH_CHECK(ns > 0, "column_moments_pend: the slot layout covers the statistic sets {sse}, {sse, st, stt} and "
              "{sse, st, stt, sx} only (need = ", need, ")");
  return tea::kMomentsPendSlots * (ns * d + 1);
}

static void bind_pend(tea::MomentsArgs& a, const Tensor& pend, const Tensor& ref) {
  TORCH_CHECK(tea::moments_ns(a) > 0, "column_moments: deferred mode needs the statistic set {sse}, {sse, st, stt} "
              "or {sse, st, stt, sx} (need = ", tea::moments_need(a), ")");
  TORCH_CHECK(pend.scalar_type() == at::kDouble && pend.is_contiguous() && pend.device() == ref.device() &&
                  pend.numel() >= tea::kMomentsPendSlots * (tea::moments_ns(a) * a.d + 1),
              "column_moments: pend must be a contiguous float64 buffer of slots * (ns * d + 1)");
  a.pend = pend.data_ptr<double>();
  a.pend_slots = tea::kMomentsPendSlots;
}

// deferred-mode class update: FP64 column partials ADDED to the slots of `pend` (zero-initialised
// by the caller, zeroed again by column_moments_fold); the states are only the statistic
// selection here.  Returns the slots used (0: not applicable, the caller takes another path).
int64_t column_moments_pend(const optional<Tensor>& x, const optional<Tensor>& t, const optional<Tensor>& w,
                            const optional<Tensor>& sse, const optional<Tensor>& st, const optional<Tensor>& stt,
                            const optional<Tensor>& sx, const optional<Tensor>& sw, const Tensor& pend) {
  const Tensor& ref = x.has_value() ? *x : *t;
  check_gpu(ref, "x/t");
  TORCH_CHECK(ref.dim() == 2, "column_moments: inputs must be [n, d] views");
  DeviceGuard guard(ref.device());
  tea::MomentsArgs a = moments_args(x, t, w, sse, st, stt, sx, sw, ref);
  if (a.n == 0 || a.d == 0) return 0;
  bind_pend(a, pend, ref);
  int64_t wsd = 0, tk = 0;
  if (!tea::column_moments_v2_plan(a, &wsd, &tk)) return 0;
  check_launch(tea::launch_column_moments(a, stream_for(ref)), "column_moments_pend");
  return a.v2_r;
}

// fold the first `slots` pending slots into the states (float32 +=) and zero them
void column_moments_fold(const Tensor& pend, int64_t slots, const optional<Tensor>& sse,
                         const optional<Tensor>& st, const optional<Tensor>& stt, const optional<Tensor>& sx,
                         const optional<Tensor>& sw) {
  const Tensor& like = sse.has_value() ? *sse : st.has_value() ? *st : *stt;
  check_gpu(like, "states");
  DeviceGuard guard(like.device());
  const Tensor ref = at::empty({0, like.numel()}, like.options());  // shape carrier: n = 0, d
  tea::MomentsArgs a = moments_args(c10::nullopt, c10::nullopt, c10::nullopt, sse, st, stt, sx, sw, ref);
  bind_pend(a, pend, like);
  check_launch(tea::launch_moments_fold(a, static_cast<int>(slots), stream_for(like)), "column_moments_fold");
}

void column_moments(const optional<Tensor>& x, const optional<Tensor>& t,
                    const optional<Tensor>& w, const optional<Tensor>& sse,
                    const optional<Tensor>& st, const optional<Tensor>& stt,
                    const optional<Tensor>& sx, const optional<Tensor>& sw, int64_t overwrite,
                    int64_t mse_mode, const optional<Tensor>& mse_out, int64_t num_regressors) {
  const Tensor& ref = x.has_value() ? *x : *t;
  check_gpu(ref, "x/t");
  TORCH_CHECK(ref.dim() == 2, "column_moments: inputs must be [n, d] views");
  DeviceGuard guard(ref.device());
  tea::MomentsArgs a = moments_args(x, t, w, sse, st, stt, sx, sw, ref);
  a.overwrite = overwrite != 0;
  a.mse_mode = static_cast<int>(mse_mode);
  Tensor raw_scratch;
  if (a.mse_mode) {
    const bool raw = a.mse_mode == 1 || a.mse_mode == 3;
    TORCH_CHECK(a.mse_mode >= 1 && a.mse_mode <= 5 && a.overwrite && a.sse && mse_out.has_value() &&
                    mse_out->scalar_type() == at::kFloat && mse_out->is_contiguous() &&
                    mse_out->device() == ref.device() && mse_out->numel() == (raw ? a.d : 1),
                "column_moments: fused compute needs overwrite, sse and a float32 output of d (raw) or 1 elements");
    TORCH_CHECK(a.mse_mode < 3 || (a.st && a.stt), "column_moments: fused R2 needs st and stt");
    a.mse_out = mse_out->data_ptr<float>();
    a.num_obs = a.n;
    a.num_regressors = static_cast<int>(num_regressors);
    if (!raw) {
      raw_scratch = at::empty({2 * a.d}, ref.options().dtype(at::kFloat));
      a.mse_part_f = raw_scratch.data_ptr<float>();
    }
  }
  if (a.n == 0 || a.d == 0) return;
  int64_t v2_doubles = 0, v2_tickets = 0;
  if (tea::column_moments_v2_plan(a, &v2_doubles, &v2_tickets)) {  // one launch (K5 v2)
    hipStream_t st = stream_for(ref);
    a.part = static_cast<double*>(scratch_workspace(ref, st, v2_doubles * 8, Scratch::kMomentsPartials));
    a.tickets = static_cast<unsigned*>(zeroed_workspace(ref, st, v2_tickets * 4, Zeroed::kMomentsTickets));
    check_launch(tea::launch_column_moments(a, st), "column_moments");
    return;
  }
  a.ws_blocks = tea::column_moments_blocks(a.n, a.d);
  const int64_t nstats = (a.sse != nullptr) + (a.st != nullptr) + (a.stt != nullptr) + (a.sx != nullptr);
  Tensor ws = at::empty({a.ws_blocks * (nstats * a.d + 1)}, ref.options().dtype(at::kDouble));
  a.ws = ws.data_ptr<double>();
  check_launch(tea::launch_column_moments(a, stream_for(ref)), "column_moments");
}

// x, t: [rows, n] (rows contiguous); w optional [rows, n]; out float64 [rows, 3] accumulated.
void ne_sums(const Tensor& x, const Tensor& t, const optional<Tensor>& w, bool from_logits,
             const Tensor& out, const optional<Tensor>& err, bool deterministic) {
  check_gpu(x, "x");
  TORCH_CHECK(x.dim() == 2 && t.sizes() == x.sizes(), "ne_sums: x/t must be [rows, n]");
  TORCH_CHECK(x.stride(1) == 1 && t.stride(1) == 1, "ne_sums: rows must be contiguous");
  TORCH_CHECK(out.scalar_type() == at::kDouble && out.is_contiguous() && out.numel() == x.size(0) * 3,
              "ne_sums: out must be float64 [rows, 3]");
  DeviceGuard guard(x.device());
  tea::NeArgs a;
  a.x = x.data_ptr();
  a.x_dt = dt_of(x);
  a.x_row_stride = x.stride(0);
  a.t = t.data_ptr();
  a.t_dt = dt_of(t);
  a.t_row_stride = t.stride(0);
  if (w.has_value()) {
    TORCH_CHECK(w->sizes() == x.sizes() && w->stride(1) == 1, "ne_sums: weight must match x");
    a.w = w->data_ptr();
    a.w_dt = dt_of(*w);
    a.w_row_stride = w->stride(0);
  }
  a.rows = x.size(0);
  a.n = x.size(1);
  a.from_logits = from_logits ? 1 : 0;
  a.out = out.data_ptr<double>();
  if (err.has_value()) {
    TORCH_CHECK(err->scalar_type() == at::kInt, "ne_sums: err must be int32");
    a.err = err->data_ptr<int>();
    // [flag, pad, range keys as 2 x u64] (8-byte aligned: caching-allocator blocks are)
    if (err->numel() >= 6) a.range = reinterpret_cast<unsigned long long*>(a.err + 2);
  }
  Tensor ws;
  if (deterministic && a.rows > 0) {
    ws = at::empty({a.rows * 3 * tea::ne_sums_blocks(a.n)}, out.options());
    a.ordered_ws = ws.data_ptr<double>();
  }
  check_launch(tea::launch_ne_sums(a, stream_for(x)), "ne_sums");
}

// ---------------------------------------------------------------- K7 perplexity
// input: [rows, v] logits (unit column stride); target: [rows]; out float64 [2] accumulated.
void perplexity_sums(const Tensor& input, const Tensor& target, optional<int64_t> ignore_index,
                     const Tensor& out, const optional<Tensor>& err, bool deterministic) {
  check_gpu(input, "input");
  TORCH_CHECK(input.dim() == 2 && input.stride(1) == 1, "perplexity: input must be [rows, v]");
  TORCH_CHECK(target.dim() == 1 && target.size(0) == input.size(0), "perplexity: target must be [rows]");
  TORCH_CHECK(out.scalar_type() == at::kDouble && out.numel() == 2 && out.is_contiguous(),
              "perplexity: out must be float64 [2]");
  DeviceGuard guard(input.device());
  tea::PerplexityArgs a;
  a.input = input.data_ptr();
  a.in_dt = dt_of(input);
  a.rows = input.size(0);
  a.v = input.size(1);
  a.row_stride = input.stride(0);
  a.target = target.data_ptr();
  a.tg_dt = dt_of(target);
  a.tg_stride = target.stride(0);
  if (ignore_index.has_value()) {
    a.has_ignore = 1;
    a.ignore_index = *ignore_index;
  }
  a.out = out.data_ptr<double>();
  if (err.has_value()) a.err = err->data_ptr<int>();
  Tensor ws;
  if (deterministic && a.rows > 0) {
    ws = at::empty({2 * tea::perplexity_blocks(a)}, out.options());
    a.ordered_ws = ws.data_ptr<double>();
  }
  const int rc = tea::launch_perplexity(a, stream_for(input));
  TORCH_CHECK(rc != -1, "perplexity: unsupported logits dtype ", input.scalar_type());
  TORCH_CHECK(rc != -2, "perplexity: logits storage is not element-aligned");
  check_launch(rc, "perplexity");
}

// dispatcher form: the dispatcher passes lists as ArrayRef
void op_row_sums(const Tensor& x, const optional<Tensor>& t, const optional<Tensor>& w, double w_scalar,
                 at::TensorList outs, at::IntArrayRef codes, int64_t rows) {
  row_sums(x, t, w, w_scalar, outs.vec(), codes.vec(), rows);
}

}  // namespace

void tea_bind_reductions(py::module_& m) {
  m.def("row_sums", &row_sums, "K5b per-row weighted sums merged into state tensors (GPU kernel / host twin)",
        py::arg("x"), py::arg("t"), py::arg("w"), py::arg("w_scalar"), py::arg("outs"), py::arg("codes"),
        py::arg("rows") = 1);
  m.def("row_sums_pend", &row_sums_pend,
        "K5b deferred-mode update: pre-scaled FP64 block partials added to pending slots; returns blocks used",
        py::arg("x"), py::arg("t"), py::arg("w"), py::arg("w_scalar"), py::arg("outs"), py::arg("codes"),
        py::arg("rows"), py::arg("pend"));
  m.def("row_sums_fold", &row_sums_fold, "K5b pending slots -> outputs (ADD), slots zeroed", py::arg("pend"),
        py::arg("used"), py::arg("outs"), py::arg("codes"), py::arg("rows"));
  m.def("column_moments", &column_moments, "K5 weighted column moments (+ fused MSE compute)", py::arg("x"),
        py::arg("t"), py::arg("w"), py::arg("sse"), py::arg("st"), py::arg("stt"), py::arg("sx"), py::arg("sw"),
        py::arg("overwrite") = 0, py::arg("mse_mode") = 0, py::arg("mse_out") = py::none(),
        py::arg("num_regressors") = 0);
  m.def("column_moments_pend_numel", &column_moments_pend_numel, "deferred-mode pend buffer numel for (d, need)");
  m.def("column_moments_pend", &column_moments_pend,
        "K5 deferred-mode class update: FP64 column partials added to pending slots; returns the slots used",
        py::arg("x"), py::arg("t"), py::arg("w"), py::arg("sse"), py::arg("st"), py::arg("stt"), py::arg("sx"),
        py::arg("sw"), py::arg("pend"));
  m.def("column_moments_fold", &column_moments_fold, "K5 pending slots -> float32 states (+=), slots zeroed",
        py::arg("pend"), py::arg("slots"), py::arg("sse"), py::arg("st"), py::arg("stt"), py::arg("sx"), py::arg("sw"));
  m.def("ne_sums", &ne_sums, "K6 normalized-entropy row sums", py::arg("x"), py::arg("t"), py::arg("w"),
        py::arg("from_logits"), py::arg("out"), py::arg("err"), py::arg("deterministic") = false);
  m.def("perplexity_sums", &perplexity_sums, "K7 fused log-softmax gather", py::arg("input"), py::arg("target"),
        py::arg("ignore_index"), py::arg("out"), py::arg("err"), py::arg("deterministic") = false);
}

TORCH_LIBRARY_FRAGMENT(torcheval_amd, m) {
  m.def("row_sums(Tensor x, Tensor? t, Tensor? w, float w_scalar, Tensor(a!)[] outs, int[] codes, int rows) -> ()");
  m.def("column_moments(Tensor? x, Tensor? t, Tensor? w, Tensor(a!)? sse, Tensor(b!)? st, Tensor(c!)? stt, "
        "Tensor(d!)? sx, Tensor(e!)? sw, int overwrite, int mse_mode, Tensor(f!)? mse_out, int num_regressors) -> ()");
  m.def("ne_sums(Tensor x, Tensor t, Tensor? w, bool from_logits, Tensor(a!) out, Tensor(b!)? err, "
        "bool deterministic) -> ()");
  m.def("perplexity_sums(Tensor input, Tensor target, int? ignore_index, Tensor(a!) out, Tensor(b!)? err, "
        "bool deterministic) -> ()");
}

TORCH_LIBRARY_IMPL(torcheval_amd, CUDA, m) {
  m.impl("row_sums", &op_row_sums);
  m.impl("column_moments", &column_moments);
  m.impl("ne_sums", &ne_sums);
  m.impl("perplexity_sums", &perplexity_sums);
}

TORCH_LIBRARY_IMPL(torcheval_amd, CPU, m) {
  m.impl("row_sums", &op_row_sums);  // the C++ host twin
}

TORCH_LIBRARY_IMPL(torcheval_amd, Meta, m) {
  m.impl("row_sums", &MetaNoop<&op_row_sums>::call);
  m.impl("column_moments", &MetaNoop<&column_moments>::call);
  m.impl("ne_sums", &MetaNoop<&ne_sums>::call);
  m.impl("perplexity_sums", &MetaNoop<&perplexity_sums>::call);
}
