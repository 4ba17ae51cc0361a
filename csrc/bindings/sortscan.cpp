// torcheval_amd._C bindings (layout: module.cpp): K3a radix sort (with the onesweep fault handling), K3 scan,
// K3c curves, K3t trapezoids, the f32 transpose, K14 rank correlation.
#include <ATen/ATen.h>
#include <torch/csrc/utils/pybind.h>
#include <torch/library.h>

#include <array>
#include <atomic>
#include <cstdlib>
#include <cstring>
#include <mutex>
#include <unordered_map>

#include "tea_kernels.h"
#include "tea_torch.h"

namespace {

using namespace tea_torch;

// K3a: segmented descending radix sort of f32 rows -> (sorted scores, int32 permutation)
// Onesweep look-back timeouts (RadixArgs::os_hdr[8], set by a pass whose tile gave up waiting on
// its predecessors - forward progress relies on in-order workgroup dispatch per XCD).  Surfaced,
// never silent: the K3 scan reading that sort's output returns NaN (AucScanArgs::sort_fault), the
// word is copied asynchronously into pinned host memory after every onesweep sort, and the next
// sort on the stream that finds it set warns and sends every later sort of the process through
// the legacy (upsweep + downsweep) passes, which never wait on other workgroups.
struct OnesweepHealth {
  std::mutex mu;
  std::unordered_map<uint64_t, uint32_t*> host_word;  // (device, stream) -> pinned copy of hdr[8]
  std::atomic<bool> disabled{false};
};

OnesweepHealth& onesweep_health() {
  static auto& h = *new OnesweepHealth();  // process lifetime (no teardown after HIP's)
  return h;
}

uint64_t stream_key(const Tensor& x, hipStream_t st) {
  return (static_cast<uint64_t>(x.device().index()) << 56) ^ reinterpret_cast<uint64_t>(st);
}

// true when a previous onesweep sort on this stream reported a timeout (then the device word is
// cleared and onesweep is off for the process)
bool onesweep_faulted(const Tensor& x, hipStream_t st) {
  auto& h = onesweep_health();
  if (h.disabled.load()) return true;
  std::lock_guard<std::mutex> lock(h.mu);
  auto it = h.host_word.find(stream_key(x, st));
  if (it == h.host_word.end() || *reinterpret_cast<volatile uint32_t*>(it->second) == 0u) return false;
  h.disabled.store(true);
  auto* hdr = static_cast<uint32_t*>(zeroed_workspace(x, st, 16 * 4, Zeroed::kOnesweepHeader));
  TORCH_CHECK(hipMemsetAsync(hdr + 8, 0, 4, st) == hipSuccess, "sort_desc: timeout word reset failed");
  static const char* kMsg =
      "torcheval_amd K3a: an onesweep radix sort timed out in its look-back (its K3 result was NaN); "
      "every later sort of this process takes the legacy radix passes";
  // a Python warning when called from Python (pybind11 entry points hold the GIL; TORCH_WARN from a
  // plain pybind11 function only reaches stderr), else c10's handler
  if (Py_IsInitialized() && PyGILState_Check()) {
    if (PyErr_WarnEx(PyExc_UserWarning, kMsg, 1) != 0) throw pybind11::error_already_set();
  } else {
    TORCH_WARN(kMsg);
  }
  return true;
}

// the pinned host word of this (device, stream) that each onesweep sort's histogram launch fills
// with the PREVIOUS sort's timeout word (RadixArgs::os_watch): a timed-out sort is reported one
// sort later (its own K3 scan already returned NaN from the device word), and no sort pays a
// device-to-host copy on its stream (the hipMemcpyAsync of round 5 was a ~5 us blit kernel in
// every binary_auroc's timeline)
uint32_t* onesweep_watch_word(const Tensor& x, hipStream_t st) {
  auto& h = onesweep_health();
  std::lock_guard<std::mutex> lock(h.mu);
  auto it = h.host_word.find(stream_key(x, st));
  if (it == h.host_word.end()) {
    void* p = nullptr;
    if (hipHostMalloc(&p, 64, hipHostMallocCoherent) != hipSuccess) return nullptr;
    std::memset(p, 0, 64);
    it = h.host_word.emplace(stream_key(x, st), static_cast<uint32_t*>(p)).first;
  }
  return it->second;
}

void sort_desc(const Tensor& x, const Tensor& out_sorted, const Tensor& out_order,
               const optional<Tensor>& payload, int64_t payload_kind, bool ascending = false) {
  check_gpu(x, "x");
  TORCH_CHECK(x.dim() == 2 && x.scalar_type() == at::kFloat && x.stride(1) == 1,
              "sort_desc: x must be float32 [rows, n] with contiguous rows");
  TORCH_CHECK(out_sorted.scalar_type() == at::kFloat && out_sorted.is_contiguous() &&
                  out_sorted.sizes() == x.sizes(), "sort_desc: out_sorted must be contiguous f32 [rows, n]");
  TORCH_CHECK(out_order.scalar_type() == at::kInt && out_order.is_contiguous() &&
                  out_order.sizes() == x.sizes(), "sort_desc: out_order must be contiguous int32 [rows, n]");
  TORCH_CHECK(x.size(1) < (int64_t{1} << 31), "sort_desc: rows longer than 2^31");
  DeviceGuard guard(x.device());
  tea::RadixArgs a;
  a.in = x.data_ptr<float>();
  a.in_row_stride = x.stride(0);
  a.rows = x.size(0);
  a.n = x.size(1);
  if (a.rows == 0 || a.n == 0) return;
  a.tiles = tea::radix_sort_tiles(a.rows, a.n);
  const int64_t m = a.rows * a.n;
  Tensor ws = at::empty({4 * m + a.rows * 256 * a.tiles}, x.options().dtype(at::kInt));
  uint32_t* base = reinterpret_cast<uint32_t*>(ws.data_ptr<int32_t>());
  a.keys0 = base;
  a.vals0 = base + m;
  a.keys1 = base + 2 * m;
  a.vals1 = base + 3 * m;
  a.hist = base + 4 * m;
  a.ngroups = tea::radix_sort_groups(a.tiles);
  // self-cleaning: [header: cells left dirty in region 3 | pad | 4 regions of `region` cells]
  int64_t cap = 0;
  uint32_t* gws = static_cast<uint32_t*>(
      zeroed_workspace(x, stream_for(x), (4 + 4 * a.rows * a.ngroups * 256) * 4, Zeroed::kRadixGroups, &cap));
  a.dirty = gws;
  a.groups = gws + 4;
  a.region = (cap / 4 - 4) / 4;  // fixed per buffer, so the next call finds region 3 at the same place
  a.out_sorted = out_sorted.data_ptr<float>();
  a.out_order = out_order.data_ptr<int32_t>();
  a.key_xor = ascending ? ~0u : 0u;  // stable either way; ascending puts NaN last (torch.sort)
  static const bool onesweep = [] {
    const char* e = std::getenv("TORCHEVAL_AMD_K3_ONESWEEP");
    return e == nullptr || e[0] != '0';
  }();
  a.spin_limit = [] {
    const char* e = std::getenv("TORCHEVAL_AMD_K3_SPIN_LIMIT");  // test hook: force timeouts
    const int v = e != nullptr ? std::atoi(e) : 0;
    return v > 0 ? v : (1 << 22);
  }();
  if (onesweep && tea::radix_onesweep_ok(a.rows, a.n) && !onesweep_faulted(x, stream_for(x))) {
    // self-cleaning onesweep state (tea_kernels.h RadixArgs): header + digit totals, the status
    // planes and the group planes in three zeroed workspaces whose plane strides depend only on
    // their capacity; if any of them is (re)allocated, all three restart from zero together
    hipStream_t st = stream_for(x);
    int64_t scap = 0, gcap = 0;
    auto* hdr = static_cast<uint32_t*>(zeroed_workspace(x, st, (16 + a.rows * 8 * 4 * 256) * 4, Zeroed::kOnesweepHeader));
    auto* sws = static_cast<uint32_t*>(
        zeroed_workspace(x, st, 2 * tea::radix_onesweep_status_words(a.rows, a.n) * 4, Zeroed::kOnesweepStatus, &scap));
    auto* gws = static_cast<unsigned long long*>(
        zeroed_workspace(x, st, 2 * tea::radix_onesweep_group_words(a.rows, a.n) * 8, Zeroed::kOnesweepGroups, &gcap));
    {
      static std::mutex mu;
      static auto& seen = *new std::unordered_map<uint64_t, std::array<const void*, 3>>();
      const uint64_t key = (static_cast<uint64_t>(x.device().index()) << 56) ^ reinterpret_cast<uint64_t>(st);
      std::lock_guard<std::mutex> lock(mu);
      const std::array<const void*, 3> now{hdr, sws, gws};
      auto it = seen.find(key);
      if (it != seen.end() && it->second != now) {
        // one buffer is new (zero) while the others may hold another layout's dirty words
        TORCH_CHECK(hipMemsetAsync(hdr, 0, (16 + a.rows * 8 * 4 * 256) * 4, st) == hipSuccess &&
                        hipMemsetAsync(sws, 0, scap, st) == hipSuccess && hipMemsetAsync(gws, 0, gcap, st) == hipSuccess,
                    "sort_desc: workspace reset failed");
      }
      seen[key] = now;
    }
    a.os_hdr = hdr;
    a.os_g = hdr + 16;
    a.os_status = sws;
    a.os_splane = scap / 8;  // two u32 planes
    a.os_gacc = gws;
    a.os_gplane = gcap / 16;  // two u64 planes
    a.os_watch = onesweep_watch_word(x, st);
  }
  Tensor pl;
  if (payload.has_value() && payload_kind != 0) {
    TORCH_CHECK(payload_kind == 1 || payload_kind == 2, "sort_desc: payload_kind must be 0, 1 or 2");
    pl = *payload;
    TORCH_CHECK(pl.device() == x.device(), "sort_desc: payload on another device");
    // [n] (shared by every row) or [rows, n], unit stride along samples
    if (pl.dim() == 1) {
      TORCH_CHECK(pl.size(0) == a.n, "sort_desc: payload must have n samples");
      if (!pl.is_contiguous()) pl = pl.contiguous();
      a.payload_row_stride = 0;
    } else {
      TORCH_CHECK(pl.dim() == 2 && pl.size(0) == a.rows && pl.size(1) == a.n, "sort_desc: payload must be [rows, n]");
      if (pl.stride(1) != 1) pl = pl.contiguous();
      a.payload_row_stride = pl.stride(0);
    }
    const auto st = pl.scalar_type();
    TORCH_CHECK(payload_kind == 1 ? (st == at::kFloat || st == at::kLong || st == at::kInt || st == at::kByte ||
                                     st == at::kBool)
                                  : (st == at::kLong || st == at::kInt),
                "sort_desc: unsupported payload dtype ", st);
    a.payload_kind = static_cast<int>(payload_kind);
    a.payload = pl.data_ptr();
    a.payload_dt = dt_of(pl);
  }
  check_launch(tea::launch_radix_sort_desc(a, stream_for(x)), "sort_desc");
}


// test hook: the onesweep look-back timeout word of `x`'s device / stream (0 = every spin of every
// sort on it completed), optionally cleared; one device-to-host read
int64_t sort_desc_timeouts(const Tensor& x, bool clear) {
  check_gpu(x, "x");
  DeviceGuard guard(x.device());
  hipStream_t st = stream_for(x);
  auto* hdr = static_cast<uint32_t*>(zeroed_workspace(x, st, 16 * 4, Zeroed::kOnesweepHeader));
  uint32_t v = 0;
  TORCH_CHECK(hipMemcpyAsync(&v, hdr + 8, 4, hipMemcpyDeviceToHost, st) == hipSuccess &&
                  hipStreamSynchronize(st) == hipSuccess,
              "sort_desc_timeouts: read failed");
  if (clear && v != 0) TORCH_CHECK(hipMemsetAsync(hdr + 8, 0, 4, st) == hipSuccess, "sort_desc_timeouts: clear failed");
  return v;
}

// [n, c] (unit column stride) -> contiguous [c, n]
void transpose_f32(const Tensor& x, const Tensor& out) {
  check_gpu(x, "x");
  TORCH_CHECK(x.dim() == 2 && x.scalar_type() == at::kFloat && x.stride(1) == 1, "transpose_f32: x [n, c] f32");
  TORCH_CHECK(out.is_contiguous() && out.scalar_type() == at::kFloat && out.size(0) == x.size(1) &&
                  out.size(1) == x.size(0), "transpose_f32: out must be contiguous [c, n]");
  DeviceGuard guard(x.device());
  check_launch(tea::launch_transpose_f32(x.data_ptr<float>(), x.size(0), x.size(1), x.stride(0),
                                         out.data_ptr<float>(), stream_for(x)), "transpose_f32");
}

// ---------------------------------------------------------------- K3 sort-scan
// sorted/order: [rows, n] (descending scores and their permutation); target: [rows, n] binary
// targets or (class_mode) [n] labels; weight: optional [rows, n]; outputs float64 [rows].
// shared argument set-up of the K3 scans (auc_scan, the K3c curve passes); tg / w keep any
// contiguous copies alive for the launch
static tea::AucScanArgs scan_args(const Tensor& sorted, const Tensor& order, const Tensor& target,
                                  const optional<Tensor>& weight, bool class_mode, int64_t payload_kind,
                                  Tensor& tg, Tensor& w, const char* who) {
  check_gpu(sorted, "sorted");
  TORCH_CHECK(sorted.dim() == 2 && order.dim() == 2 && sorted.sizes() == order.sizes(),
              who, ": sorted/order must be [rows, n]");
  TORCH_CHECK(sorted.stride(1) == 1 && order.stride(1) == 1, who, ": rows must be contiguous");
  TORCH_CHECK(sorted.scalar_type() == at::kFloat || sorted.scalar_type() == at::kDouble,
              who, ": scores must be float32/float64");
  TORCH_CHECK(order.scalar_type() == at::kLong || order.scalar_type() == at::kInt,
              who, ": order must be int64 or int32");
  const int64_t rows = sorted.size(0), n = sorted.size(1);
  tea::AucScanArgs a;
  a.sorted = sorted.data_ptr();
  a.key_dt = dt_of(sorted);
  a.key_stride = sorted.stride(0);
  if (order.scalar_type() == at::kLong) a.order = order.data_ptr<int64_t>();
  else a.order32 = order.data_ptr<int32_t>();
  a.order_stride = order.stride(0);
  tg = target;
  // with a payload (kinds 1, 2) the sort carried the targets / labels and no kernel reads
  // `target` (tea_scan.h sample_ab): no layout copy for it (a transposed [n, L] multilabel
  // target used to cost one strided ATen transpose per launch here)
  const bool read_target = payload_kind == 0;
  if (class_mode) {
    TORCH_CHECK(tg.dim() == 1 && tg.size(0) == n, who, ": class-mode target must be [n]");
    if (read_target) tg = tg.contiguous();
  } else {
    TORCH_CHECK(tg.dim() == 2 && tg.size(0) == rows && tg.size(1) == n, who, ": target must be [rows, n]");
    if (read_target && tg.stride(1) != 1) tg = tg.contiguous();
    a.target_stride = tg.stride(0);
  }
  a.target = tg.data_ptr();
  a.tg_dt = dt_of(tg);
  if (weight.has_value()) {
    w = *weight;
    TORCH_CHECK(w.dim() == 2 && w.size(0) == rows && w.size(1) == n, who, ": weight must be [rows, n]");
    if (w.stride(1) != 1) w = w.contiguous();
    a.weight = w.data_ptr();
    a.w_dt = dt_of(w);
    a.weight_stride = w.stride(0);
  }
  a.class_mode = class_mode ? 1 : 0;
  TORCH_CHECK(payload_kind == 0 || (order.scalar_type() == at::kInt && !weight.has_value()),
              who, ": a payload order must be int32 and unweighted");
  a.payload_kind = static_cast<int>(payload_kind);
  a.rows = rows;
  a.n = n;
  return a;
}

void auc_scan(const Tensor& sorted, const Tensor& order, const Tensor& target,
              const optional<Tensor>& weight, bool class_mode, const optional<Tensor>& out_auroc,
              const optional<Tensor>& out_auprc, const optional<Tensor>& init,
              const optional<Tensor>& out_raw, int64_t payload_kind) {
  DeviceGuard guard(sorted.device());
  Tensor tg, w;
  tea::AucScanArgs a = scan_args(sorted, order, target, weight, class_mode, payload_kind, tg, w, "auc_scan");
  const int64_t rows = a.rows, n = a.n;
  auto f64_out = [&](const optional<Tensor>& t, const char* name) -> double* {
    if (!t.has_value()) return nullptr;
    TORCH_CHECK(t->scalar_type() == at::kDouble && t->is_contiguous() && t->numel() == rows &&
                    t->device() == sorted.device(),
                "auc_scan: ", name, " must be a contiguous float64 [rows] tensor");
    return t->data_ptr<double>();
  };
  a.out_auroc = f64_out(out_auroc, "out_auroc");
  a.out_auprc = f64_out(out_auprc, "out_auprc");
  if (init.has_value()) {
    TORCH_CHECK(init->scalar_type() == at::kDouble && init->is_contiguous() && init->numel() == 2 * rows,
                "auc_scan: init must be contiguous float64 [rows, 2]");
    a.init = init->data_ptr<double>();
  }
  if (out_raw.has_value()) {
    TORCH_CHECK(out_raw->scalar_type() == at::kDouble && out_raw->is_contiguous() && out_raw->numel() == 4 * rows,
                "auc_scan: out_raw must be contiguous float64 [rows, 4]");
    a.out_raw = out_raw->data_ptr<double>();
  }
  // the latest onesweep sort's timeout word on this stream (zero when none ever ran or it was clean)
  a.sort_fault =
      static_cast<const uint32_t*>(zeroed_workspace(sorted, stream_for(sorted), 16 * 4, Zeroed::kOnesweepHeader)) + 8;
  Tensor ws = at::empty({tea::auc_scan_workspace_bytes(rows, n)},
                        at::TensorOptions().dtype(at::kByte).device(sorted.device()));
  check_launch(tea::launch_auc_scan(a, ws.data_ptr(), stream_for(sorted)), "auc_scan");
}

// ---------------------------------------------------------------- K3c curves
int64_t curve_workspace_bytes(int64_t rows, int64_t n, bool rafp) {
  return tea::curve_workspace_bytes(rows, n, rafp);
}

// passes 1-2: tile totals / tie-group tails and per-row scans into `workspace`; G_r -> sizes
void curve_count(const Tensor& sorted, const Tensor& order, const Tensor& target, bool class_mode,
                 int64_t payload_kind, const Tensor& workspace, const Tensor& sizes) {
  DeviceGuard guard(sorted.device());
  Tensor tg, w;
  tea::AucScanArgs a = scan_args(sorted, order, target, c10::nullopt, class_mode, payload_kind, tg, w, "curve_count");
  TORCH_CHECK(workspace.is_contiguous() && workspace.scalar_type() == at::kByte &&
                  workspace.numel() >= tea::curve_workspace_bytes(a.rows, a.n, false),
              "curve_count: workspace too small");
  TORCH_CHECK(sizes.scalar_type() == at::kLong && sizes.is_contiguous() && sizes.numel() == a.rows,
              "curve_count: sizes must be contiguous int64 [rows]");
  a.sizes = sizes.data_ptr<int64_t>();
  check_launch(tea::launch_curve_count(a, workspace.data_ptr(), false, stream_for(sorted)), "curve_count");
}

// pass 3: ascending curves into the exact outputs (row_off: int64 [rows] threshold offsets)
void curve_emit(const Tensor& sorted, const Tensor& order, const Tensor& target, bool class_mode,
                int64_t payload_kind, const Tensor& workspace, const Tensor& sizes, const Tensor& row_off,
                const Tensor& out_prec, const Tensor& out_rec, const Tensor& out_thr) {
  DeviceGuard guard(sorted.device());
  Tensor tg, w;
  tea::AucScanArgs a = scan_args(sorted, order, target, c10::nullopt, class_mode, payload_kind, tg, w, "curve_emit");
  TORCH_CHECK(workspace.is_contiguous() && workspace.numel() >= tea::curve_workspace_bytes(a.rows, a.n, false),
              "curve_emit: workspace too small");
  TORCH_CHECK(sizes.scalar_type() == at::kLong && sizes.numel() == a.rows && row_off.scalar_type() == at::kLong &&
                  row_off.numel() == a.rows && row_off.is_contiguous() && row_off.device() == sorted.device(),
              "curve_emit: sizes / row_off must be int64 [rows] on the device");
  TORCH_CHECK(out_prec.scalar_type() == at::kFloat && out_rec.scalar_type() == at::kFloat &&
                  out_prec.is_contiguous() && out_rec.is_contiguous() && out_thr.is_contiguous() &&
                  out_thr.scalar_type() == sorted.scalar_type() && out_prec.numel() == out_thr.numel() + a.rows &&
                  out_rec.numel() == out_prec.numel(),
              "curve_emit: outputs must be contiguous f32 [sum G + rows] x2 and key-dtype [sum G]");
  a.sizes = sizes.data_ptr<int64_t>();
  a.row_off = row_off.data_ptr<int64_t>();
  a.out_prec = out_prec.data_ptr<float>();
  a.out_rec = out_rec.data_ptr<float>();
  a.out_thr = out_thr.data_ptr();
  check_launch(tea::launch_curve_emit(a, workspace.data_ptr(), false, stream_for(sorted)), "curve_emit");
}

// recall at fixed precision per row, no host synchronisation
void rafp(const Tensor& sorted, const Tensor& order, const Tensor& target, bool class_mode,
          int64_t payload_kind, double min_precision, const Tensor& out_max_recall, const Tensor& out_best_thr) {
  DeviceGuard guard(sorted.device());
  Tensor tg, w;
  tea::AucScanArgs a = scan_args(sorted, order, target, c10::nullopt, class_mode, payload_kind, tg, w, "rafp");
  TORCH_CHECK(out_max_recall.scalar_type() == at::kFloat && out_max_recall.is_contiguous() &&
                  out_max_recall.numel() == a.rows && out_best_thr.scalar_type() == sorted.scalar_type() &&
                  out_best_thr.is_contiguous() && out_best_thr.numel() == a.rows,
              "rafp: outputs must be contiguous f32 [rows] and key-dtype [rows]");
  Tensor sizes = at::empty({a.rows}, sorted.options().dtype(at::kLong));
  Tensor ws = at::empty({tea::curve_workspace_bytes(a.rows, a.n, true)}, sorted.options().dtype(at::kByte));
  a.sizes = sizes.data_ptr<int64_t>();
  a.min_precision = static_cast<float>(min_precision);
  a.out_max_recall = out_max_recall.data_ptr<float>();
  a.out_best_thr = out_best_thr.data_ptr();
  check_launch(tea::launch_rafp(a, ws.data_ptr(), stream_for(sorted)), "rafp");
}

// K3t: trapezoid area per row of x-sorted (x, y) pairs (csrc/kernels/trapz.hip); y is the f32
// payload K3a carried through its sort (the int32 order buffer, reinterpreted)
void trapz_sorted(const Tensor& x, const Tensor& y_bits, const Tensor& out) {
  check_gpu(x, "x");
  TORCH_CHECK(x.dim() == 2 && x.scalar_type() == at::kFloat && x.is_contiguous(), "trapz_sorted: x must be contiguous f32 [rows, n]");
  TORCH_CHECK((y_bits.scalar_type() == at::kInt || y_bits.scalar_type() == at::kFloat) && y_bits.is_contiguous() &&
                  y_bits.sizes() == x.sizes() && y_bits.device() == x.device(),
              "trapz_sorted: y must be contiguous f32 / int32 bits shaped like x");
  TORCH_CHECK(out.scalar_type() == at::kFloat && out.is_contiguous() && out.numel() == x.size(0) &&
                  out.device() == x.device(),
              "trapz_sorted: out must be f32 [rows]");
  DeviceGuard guard(x.device());
  const hipStream_t st = stream_for(x);
  auto* part = static_cast<double*>(
      scratch_workspace(x, st, x.size(0) * tea::trapz_blocks(x.size(1)) * 8, Scratch::kTrapzPartials));
  check_launch(tea::launch_trapz_sorted(x.data_ptr<float>(), static_cast<const float*>(y_bits.data_ptr()), x.size(0),
                                        x.size(1), part, out.data_ptr<float>(), st),
               "trapz_sorted");
}

// K14: Spearman's rho per row from one K3a sort of both operands (csrc/kernels/rankcorr.hip):
// sorted f32 and order int32, contiguous [2 rows, n] (the first operand's rows, then the
// second's); out f32 [rows]
void rank_corr(const Tensor& sorted, const Tensor& order, const Tensor& out) {
  check_gpu(sorted, "sorted");
  TORCH_CHECK(sorted.dim() == 2 && sorted.scalar_type() == at::kFloat && sorted.is_contiguous() &&
                  sorted.size(0) % 2 == 0,
              "rank_corr: sorted must be contiguous float32 [2 rows, n]");
  TORCH_CHECK(order.scalar_type() == at::kInt && order.is_contiguous() && order.sizes() == sorted.sizes() &&
                  order.device() == sorted.device(),
              "rank_corr: order must be contiguous int32 [2 rows, n]");
  const int64_t rows = sorted.size(0) / 2, n = sorted.size(1);
  TORCH_CHECK(n >= 2 && n < (int64_t{1} << 31), "rank_corr: rows of 2 .. 2^31 - 1 samples, got ", n);
  f32_out(out, sorted, rows, "out");
  if (rows == 0) return;
  DeviceGuard guard(sorted.device());
  const hipStream_t st = stream_for(sorted);
  tea::RankCorrArgs a;
  a.sorted = sorted.data_ptr<float>();
  a.order = order.data_ptr<int32_t>();
  a.rows = rows;
  a.n = n;
  a.pitch = tea::rank_corr_pitch(n);
  Tensor ws = at::empty({2 * rows * a.pitch + 2 * rows}, sorted.options().dtype(at::kInt));
  a.c = ws.data_ptr<int32_t>();
  a.nan_flag = a.c + 2 * rows * a.pitch;
  a.part = static_cast<double*>(
      scratch_workspace(sorted, st, rows * tea::rank_moments_blocks(n) * 3 * 8, Scratch::kRankCorrPartials));
  // the timeout word of the onesweep sort that produced `sorted`.  More than 8 stacked rows took
  // the legacy passes, which neither set nor clear that word: an older sort's flag is not theirs
  if (tea::radix_onesweep_ok(2 * rows, n))
    a.sort_fault = static_cast<const uint32_t*>(zeroed_workspace(sorted, st, 16 * 4, Zeroed::kOnesweepHeader)) + 8;
  a.out = out.data_ptr<float>();
  check_launch(tea::launch_rank_corr(a, st), "rank_corr");
}

}  // namespace

void tea_bind_sortscan(py::module_& m) {
  m.def("auc_scan", &auc_scan, "K3 tie-aware scan -> AUROC / AUPRC per row", py::arg("sorted"), py::arg("order"),
        py::arg("target"), py::arg("weight"), py::arg("class_mode"), py::arg("out_auroc"), py::arg("out_auprc"),
        py::arg("init") = py::none(), py::arg("out_raw") = py::none(), py::arg("payload_kind") = 0);
  m.def("curve_workspace_bytes", &curve_workspace_bytes, "K3c workspace bytes", py::arg("rows"), py::arg("n"),
        py::arg("rafp"));
  m.def("curve_count", &curve_count, "K3c tile totals + tie-group tails + per-row scans (G_r -> sizes)",
        py::arg("sorted"), py::arg("order"), py::arg("target"), py::arg("class_mode"), py::arg("payload_kind"),
        py::arg("workspace"), py::arg("sizes"));
  m.def("curve_emit", &curve_emit, "K3c ascending precision / recall / threshold curves", py::arg("sorted"),
        py::arg("order"), py::arg("target"), py::arg("class_mode"), py::arg("payload_kind"), py::arg("workspace"),
        py::arg("sizes"), py::arg("row_off"), py::arg("out_prec"), py::arg("out_rec"), py::arg("out_thr"));
  m.def("rafp", &rafp, "K3c recall at fixed precision per row (sync-free)", py::arg("sorted"), py::arg("order"),
        py::arg("target"), py::arg("class_mode"), py::arg("payload_kind"), py::arg("min_precision"),
        py::arg("out_max_recall"), py::arg("out_best_thr"));
  m.def("transpose_f32", &transpose_f32, "LDS-tiled [n, c] -> [c, n] float32 transpose", py::arg("x"), py::arg("out"));
  m.def("sort_desc_timeouts", &sort_desc_timeouts, "test hook: onesweep look-back timeout word (0 = none)",
        py::arg("x"), py::arg("clear") = true);
  m.def("sort_desc", &sort_desc,
        "K3a segmented stable radix sort, descending or ascending (f32 -> sorted, int32 order)", py::arg("x"),
        py::arg("out_sorted"), py::arg("out_order"), py::arg("payload") = py::none(), py::arg("payload_kind") = 0,
        py::arg("ascending") = false);
  m.def("trapz_sorted", &trapz_sorted, "K3t trapezoid area per row of x-sorted (x, y)", py::arg("x"), py::arg("y_bits"),
        py::arg("out"));
}

TORCH_LIBRARY_FRAGMENT(torcheval_amd, m) {
  m.def("sort_desc(Tensor x, Tensor(a!) sorted, Tensor(b!) order, Tensor? payload, int payload_kind, bool ascending=False) -> ()");
  m.def("auc_scan(Tensor sorted, Tensor order, Tensor target, Tensor? weight, bool class_mode, "
        "Tensor(a!)? out_auroc, Tensor(b!)? out_auprc, Tensor? init, Tensor(c!)? out_raw, int payload_kind) -> ()");
  // no Meta kernel: the caller reads `sizes` on the host between the two to size curve_emit's outputs
  m.def("curve_count(Tensor sorted, Tensor order, Tensor target, bool class_mode, int payload_kind, "
        "Tensor(a!) workspace, Tensor(b!) sizes) -> ()");
  // no Meta kernel: its output sizes come from curve_count's host read, so no graph holds it
  m.def("curve_emit(Tensor sorted, Tensor order, Tensor target, bool class_mode, int payload_kind, "
        "Tensor(a!) workspace, Tensor sizes, Tensor row_off, Tensor(b!) out_prec, Tensor(c!) out_rec, "
        "Tensor(d!) out_thr) -> ()");
  m.def("rafp(Tensor sorted, Tensor order, Tensor target, bool class_mode, int payload_kind, float min_precision, "
        "Tensor(a!) out_max_recall, Tensor(b!) out_best_thr) -> ()");
  m.def("trapz_sorted(Tensor x, Tensor y_bits, Tensor(a!) out) -> ()");
  m.def("transpose_f32(Tensor x, Tensor(a!) out) -> ()");
}

TORCH_LIBRARY_IMPL(torcheval_amd, CUDA, m) {
  m.impl("sort_desc", &sort_desc);
  m.impl("auc_scan", &auc_scan);
  m.impl("curve_count", &curve_count);
  m.impl("curve_emit", &curve_emit);
  m.impl("rafp", &rafp);
  m.impl("trapz_sorted", &trapz_sorted);
  m.impl("transpose_f32", &transpose_f32);
}

TORCH_LIBRARY_IMPL(torcheval_amd, Meta, m) {
  m.impl("sort_desc", &MetaNoop<&sort_desc>::call);
  m.impl("auc_scan", &MetaNoop<&auc_scan>::call);
  m.impl("rafp", &MetaNoop<&rafp>::call);
  m.impl("trapz_sorted", &MetaNoop<&trapz_sorted>::call);
  m.impl("transpose_f32", &MetaNoop<&transpose_f32>::call);
}

// K14's op: schema, CUDA kernel, Meta kernel.  It sits in a dispatcher namespace of its own and
// has no pybind entry, because the attributes of `_C` and the `torcheval_amd::` ops are recorded
// in tests/golden/native_api.json and that fixture stays byte for byte what it was.  Eager and
// compiled calls both take the dispatcher (ops/rankcorr.py);
// tests/metrics/regression/test_spearman.py pins the schema, the dispatch keys and the Meta kernel.
TORCH_LIBRARY(torcheval_amd_rankcorr, m) {
  m.def("rank_corr(Tensor sorted, Tensor order, Tensor(a!) out) -> ()");
}

TORCH_LIBRARY_IMPL(torcheval_amd_rankcorr, CUDA, m) {
  m.impl("rank_corr", &rank_corr);
}

TORCH_LIBRARY_IMPL(torcheval_amd_rankcorr, Meta, m) {
  m.impl("rank_corr", &MetaNoop<&rank_corr>::call);
}
