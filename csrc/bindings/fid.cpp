// torcheval_amd._C bindings (layout: module.cpp): K8 covariance update, K9b eigenvalues, K9d / K9p Cholesky
// factorisations, the FID prep / finish glue.
#include <ATen/ATen.h>
#include <torch/csrc/utils/pybind.h>
#include <torch/library.h>

#include "tea_kernels.h"
#include "tea_torch.h"

namespace {

using namespace tea_torch;

// ---------------------------------------------------------------- K8 FID covariance
void fid_cov_update(const Tensor& act_in, const Tensor& cov, const optional<Tensor>& colsum) {
  check_gpu(act_in, "activations");
  TORCH_CHECK(act_in.dim() == 2 && act_in.scalar_type() == at::kFloat && act_in.stride(1) == 1,
              "fid_cov_update: activations must be float32 [n, d] with unit column stride");
  const int64_t d = act_in.size(1);
  // K8 stages 16-byte pieces: rows must start 16-byte aligned and a width that is not a
  // multiple of 4 is zero-padded (one copy; the FID feature widths 64 / 192 / 768 / 2048 never
  // need it)
  Tensor act = act_in;
  if (d % 4 != 0) act = at::constant_pad_nd(act_in, {0, 4 - d % 4}, 0);
  TORCH_CHECK(act.stride(0) % 4 == 0 && reinterpret_cast<uintptr_t>(act.data_ptr()) % 16 == 0,
              "fid_cov_update: activation rows must be 16-byte aligned");
  TORCH_CHECK(cov.scalar_type() == at::kFloat && cov.is_contiguous() && cov.numel() == d * d &&
                  cov.device() == act.device(),
              "fid_cov_update: cov must be a contiguous float32 [d, d] on the same device");
  DeviceGuard guard(act.device());
  tea::FidCovArgs a;
  a.act = act.data_ptr<float>();
  a.n = act.size(0);
  a.d = d;
  a.ld = act.size(1);
  a.row_stride = act.stride(0);
  a.cov = cov.data_ptr<float>();
  a.zeros = static_cast<const float*>(zeroed_workspace(act, stream_for(act), 64, Zeroed::kFidCovZeros));
  if (colsum.has_value()) {
    TORCH_CHECK(colsum->scalar_type() == at::kFloat && colsum->is_contiguous() && colsum->numel() == d,
                "fid_cov_update: colsum must be float32 [d]");
    a.colsum = colsum->data_ptr<float>();
  }
  a.split = tea::fid_cov_split(a.n, d);
  if (a.split > 1)
    a.ws = static_cast<float*>(scratch_workspace(act, stream_for(act), tea::fid_cov_workspace_bytes(d, a.split),
                                                 Scratch::kFidCovSplit));
  check_launch(tea::launch_fid_cov(a, stream_for(act)), "fid_cov_update");
}

// ---------------------------------------------------------------- K9b symmetric eigenvalues
// Eigenvalues (ascending) of a symmetric FP64 [n, n] matrix by the on-chip (register-resident) one-launch
// Householder reduction + multisection (csrc/kernels/symeig.hip).  Returns 0 when launched
// (then status[0] != 0 after the stream reaches it means the grid aborted and lam is
// invalid), non-zero when this device / size is not handled (nothing launched).
int64_t sym_eigvals(const Tensor& m, const Tensor& lam, const Tensor& status) {
  check_gpu(m, "matrix");
  TORCH_CHECK(m.dim() == 2 && m.size(0) == m.size(1) && m.scalar_type() == at::kDouble && m.is_contiguous(),
              "sym_eigvals: matrix must be a contiguous float64 [n, n]");
  const int64_t n = m.size(0);
  TORCH_CHECK(lam.scalar_type() == at::kDouble && lam.is_contiguous() && lam.numel() == n &&
                  lam.device() == m.device(),
              "sym_eigvals: lam must be a contiguous float64 [n] on the matrix's device");
  TORCH_CHECK(status.scalar_type() == at::kInt && status.numel() >= 1 && status.device() == m.device(),
              "sym_eigvals: status must be an int32 tensor on the matrix's device");
  DeviceGuard guard(m.device());
  int grid = 0, rows = 0;
  if (tea::symeig_plan(n, &grid, &rows) != 0) return 1;
  const hipStream_t stream = stream_for(m);
  tea::SymEigArgs a;
  a.a = m.data_ptr<double>();
  a.n = n;
  a.ld = tea::symeig_slot_stride(n);
  // layout: ctl (2 KB), d [ld], e [ld], the 2 hand-off slot planes (sentinel-filled by the
  // launcher on every call, so no state carries over between launches), the Sturm-count grid,
  // the tail kernel's trailing block
  const int64_t bytes = 2048 + 2 * a.ld * (int64_t)sizeof(double) + tea::symeig_slot_bytes(n) + tea::symeig_grid_bytes() +
                        tea::symeig_tail_bytes();
  char* ws = static_cast<char*>(scratch_workspace(m, stream, bytes, Scratch::kSymEig));
  a.ctl = reinterpret_cast<unsigned*>(ws);
  a.d = reinterpret_cast<double*>(ws + 2048);
  a.e = a.d + a.ld;
  a.slots = reinterpret_cast<unsigned long long*>(a.e + a.ld);
  a.grid = reinterpret_cast<int*>(reinterpret_cast<char*>(a.slots) + tea::symeig_slot_bytes(n));
  a.tail = reinterpret_cast<double*>(reinterpret_cast<char*>(a.grid) + tea::symeig_grid_bytes());
  a.lam = lam.data_ptr<double>();
  const int rc = tea::launch_symeig(a, stream);
  if (rc == 1 || rc == 3) return rc;
  check_launch(rc, "sym_eigvals");
  TORCH_CHECK(hipMemcpyAsync(status.data_ptr<int>(), a.ctl + 1, sizeof(int), hipMemcpyDeviceToDevice, stream) ==
                  hipSuccess,
              "sym_eigvals: status copy failed");
  return 0;
}

// K9d: the whole blocked FP64 Cholesky in one persistent launch (csrc/kernels/cholesky.hip).
// l: padded [64 nt, 64 nt] float64 output (upper triangle zeroed), linv: >= nt * 4096 float64
// scratch, ctl: >= 1 int32 scratch, status: >= 2 int32 -> [LAPACK info, abort].
void cholesky_factor(const Tensor& a, const Tensor& l, const Tensor& linv, const Tensor& ctl, const Tensor& status) {
  check_gpu(a, "matrix");
  TORCH_CHECK(a.dim() == 2 && a.size(0) == a.size(1) && a.scalar_type() == at::kDouble && a.stride(1) == 1,
              "cholesky_factor: matrix must be a row-contiguous float64 [n, n]");
  const int64_t n = a.size(0);
  const int64_t N = 64 * static_cast<int64_t>(tea::cholesky_tiles(n));
  TORCH_CHECK(l.scalar_type() == at::kDouble && l.is_contiguous() && l.numel() == N * N && l.device() == a.device(),
              "cholesky_factor: l must be a contiguous float64 [", N, ", ", N, "]");
  TORCH_CHECK(linv.scalar_type() == at::kDouble && linv.is_contiguous() && linv.numel() >= (N / 64) * 4096 &&
                  linv.device() == a.device(),
              "cholesky_factor: linv too small");
  TORCH_CHECK(ctl.scalar_type() == at::kInt && ctl.numel() >= 1 && ctl.device() == a.device(), "cholesky_factor: ctl");
  TORCH_CHECK(status.scalar_type() == at::kInt && status.is_contiguous() && status.numel() >= 2 &&
                  status.device() == a.device(),
              "cholesky_factor: status must be int32 [2]");
  DeviceGuard guard(a.device());
  check_launch(tea::launch_cholesky(a.data_ptr<double>(), a.stride(0), n, l.data_ptr<double>(), linv.data_ptr<double>(),
                                    ctl.data_ptr<int>(), status.data_ptr<int>(), stream_for(a)),
               "cholesky_factor");
}

// K9p: pivoted (rank-revealing) FP64 Cholesky of a symmetric PSD matrix in one cooperative
// launch (csrc/kernels/pivchol.hip).  slots: int64 [pivchol_slot_words(n)] scratch, w: contiguous
// float64 [N, N], N = pivchol_padded(n) (row j = factor column j in the original feature order),
// piv: int32 [n], info: int32 [2] -> [rank, status (1 NaN in the matrix, 2 aborted)], ctl: int32
// [>= 1] scratch.  Returns 0 launched, 3 the grid could not be co-scheduled, 4 n unsupported.
int64_t pivchol_impl(const Tensor& a, const Tensor& slots, const Tensor& w, const Tensor& piv, const Tensor& info,
                     const Tensor& ctl, unsigned long long* trace) {
  check_gpu(a, "matrix");
  TORCH_CHECK(a.dim() == 2 && a.size(0) == a.size(1) && a.scalar_type() == at::kDouble && a.stride(1) == 1,
              "pivchol: matrix must be a row-contiguous float64 [n, n]");
  const int64_t n = a.size(0);
  const int64_t N = tea::pivchol_padded(n);
  TORCH_CHECK(slots.scalar_type() == at::kLong && slots.is_contiguous() && slots.numel() >= tea::pivchol_slot_words(n) &&
                  slots.device() == a.device(),
              "pivchol: slots must be int64 [pivchol_slot_words(n)]");
  TORCH_CHECK(w.scalar_type() == at::kDouble && w.is_contiguous() && w.numel() == N * N && w.device() == a.device(),
              "pivchol: w must be a contiguous float64 [", N, ", ", N, "]");
  TORCH_CHECK(piv.scalar_type() == at::kInt && piv.is_contiguous() && piv.numel() >= n && piv.device() == a.device(),
              "pivchol: piv must be int32 [n]");
  TORCH_CHECK(info.scalar_type() == at::kInt && info.is_contiguous() && info.numel() >= 2 && info.device() == a.device(),
              "pivchol: info must be int32 [2]");
  TORCH_CHECK(ctl.scalar_type() == at::kInt && ctl.is_contiguous() && ctl.numel() >= 1 && ctl.device() == a.device(),
              "pivchol: ctl must be int32 [1]");
  DeviceGuard guard(a.device());
  const int rc = tea::launch_pivchol(a.data_ptr<double>(), a.stride(0), n,
                                     reinterpret_cast<unsigned long long*>(slots.data_ptr<int64_t>()), w.data_ptr<double>(),
                                     piv.data_ptr<int>(), info.data_ptr<int>(),
                                     reinterpret_cast<unsigned*>(ctl.data_ptr<int>()), stream_for(a), trace);
  TORCH_CHECK(rc != 2, "pivchol: launch setup failed");
  return rc;
}
int64_t pivchol(const Tensor& a, const Tensor& slots, const Tensor& w, const Tensor& piv, const Tensor& info,
                const Tensor& ctl) {
  return pivchol_impl(a, slots, w, piv, info, ctl, nullptr);
}
// profiling hook: pivchol with the launcher's phase stamps in trace (int64 >= 80)
int64_t pivchol_traced(const Tensor& a, const Tensor& slots, const Tensor& w, const Tensor& piv, const Tensor& info,
                       const Tensor& ctl, const Tensor& trace) {
  TORCH_CHECK(trace.scalar_type() == at::kLong && trace.is_contiguous() && trace.numel() >= 80 &&
                  trace.device() == a.device(),
              "pivchol_traced: trace must be int64 [80]");
  return pivchol_impl(a, slots, w, piv, info, ctl, reinterpret_cast<unsigned long long*>(trace.data_ptr<int64_t>()));
}

// test / profiling hook: cholesky_factor with per-tile-column phase stamps (s_memrealtime,
// 100 MHz) of the pair-owner tasks in trace (int64 [nt * 8]), then the shader-clock stamps of every
// column of tile column 1's factorisation (wave 0: [nt * 8, + 65), wave 1: [nt * 8 + 65, + 65))
void cholesky_factor_traced(const Tensor& a, const Tensor& l, const Tensor& linv, const Tensor& ctl,
                            const Tensor& status, const Tensor& trace) {
  const int64_t nt = tea::cholesky_tiles(a.size(0));
  TORCH_CHECK(trace.scalar_type() == at::kLong && trace.is_contiguous() && trace.numel() >= nt * 8 + 130 &&
                  trace.device() == a.device(),
              "cholesky_factor_traced: trace must be int64 [nt * 8 + 130]");
  check_gpu(a, "matrix");
  TORCH_CHECK(l.numel() == 64 * nt * 64 * nt && linv.numel() >= nt * 4096 && status.numel() >= 2,
              "cholesky_factor_traced: workspace sizes");
  DeviceGuard guard(a.device());
  check_launch(tea::launch_cholesky(a.data_ptr<double>(), a.stride(0), a.size(0), l.data_ptr<double>(),
                                    linv.data_ptr<double>(), ctl.data_ptr<int>(), status.data_ptr<int>(), stream_for(a),
                                    reinterpret_cast<unsigned long long*>(trace.data_ptr<int64_t>())),
               "cholesky_factor_traced");
}

// FID compute glue (csrc/kernels/fid_prep.hip): FP64 symmetric covariance from the FP32 states.
void cov_finalize(const Tensor& cov_sum, const Tensor& colsum, double n, const Tensor& out) {
  check_gpu(cov_sum, "cov_sum");
  const int64_t d = colsum.numel();
  TORCH_CHECK(cov_sum.scalar_type() == at::kFloat && cov_sum.is_contiguous() && cov_sum.numel() == d * d,
              "cov_finalize: cov_sum must be a contiguous float32 [d, d]");
  TORCH_CHECK(colsum.scalar_type() == at::kFloat && colsum.is_contiguous() && colsum.device() == cov_sum.device(),
              "cov_finalize: colsum must be a contiguous float32 [d]");
  TORCH_CHECK(out.scalar_type() == at::kDouble && out.is_contiguous() && out.numel() == d * d &&
                  out.device() == cov_sum.device(),
              "cov_finalize: out must be a contiguous float64 [d, d]");
  TORCH_CHECK(n > 1.0, "cov_finalize: needs n > 1");
  DeviceGuard guard(cov_sum.device());
  check_launch(tea::launch_cov_finalize(cov_sum.data_ptr<float>(), colsum.data_ptr<float>(), n, d,
                                        out.data_ptr<double>(), stream_for(cov_sum)),
               "cov_finalize");
}

// FID's closing combination: |sum1 / n1 - sum2 / n2|^2 + tr S1 + tr S2 - 2 sum sqrt(max(lam, 0))
// -> out (float32 scalar), one launch
void fid_finish(const Tensor& sum1, double n1, const Tensor& sum2, double n2, const Tensor& s1, const Tensor& s2,
                const Tensor& lam, const Tensor& out) {
  check_gpu(sum1, "sum1");
  const int64_t d = sum1.numel();
  TORCH_CHECK(sum1.scalar_type() == at::kFloat && sum1.is_contiguous() && sum2.scalar_type() == at::kFloat &&
                  sum2.is_contiguous() && sum2.numel() == d,
              "fid_finish: sums must be contiguous float32 [d]");
  for (const Tensor* s : {&s1, &s2})
    TORCH_CHECK(s->scalar_type() == at::kDouble && s->dim() == 2 && s->size(0) == d && s->size(1) == d &&
                    s->stride(1) == 1 && s->device() == sum1.device(),
                "fid_finish: covariances must be row-contiguous float64 [d, d]");
  TORCH_CHECK(lam.scalar_type() == at::kDouble && lam.is_contiguous() && lam.device() == sum1.device(),
              "fid_finish: eigenvalues must be contiguous float64");
  TORCH_CHECK(out.scalar_type() == at::kFloat && out.numel() == 1 && out.device() == sum1.device(),
              "fid_finish: out must be a float32 scalar");
  TORCH_CHECK(n1 > 0 && n2 > 0, "fid_finish: needs samples on both sides");
  DeviceGuard guard(sum1.device());
  check_launch(tea::launch_fid_finish(sum1.data_ptr<float>(), n1, sum2.data_ptr<float>(), n2, d, s1.data_ptr<double>(),
                                      s1.stride(0), s2.data_ptr<double>(), s2.stride(0), lam.data_ptr<double>(),
                                      lam.numel(), out.data_ptr<float>(), stream_for(sum1)),
               "fid_finish");
}

void sym_fill_upper(const Tensor& m) {
  check_gpu(m, "matrix");
  TORCH_CHECK(m.dim() == 2 && m.size(0) == m.size(1) && m.scalar_type() == at::kDouble && m.stride(1) == 1 &&
                  m.stride(0) >= m.size(1),
              "sym_fill_upper: matrix must be a row-contiguous float64 [n, n]");
  DeviceGuard guard(m.device());
  check_launch(tea::launch_sym_fill_upper(m.data_ptr<double>(), m.stride(0), m.size(0), stream_for(m)),
               "sym_fill_upper");
}

}  // namespace

void tea_bind_fid(py::module_& m) {
  m.def("fid_cov_update", &fid_cov_update, "K8 FP32-MFMA symmetric rank-k covariance update", py::arg("act"),
        py::arg("cov"), py::arg("colsum"));
  m.def("cholesky_factor", &cholesky_factor, "K9d one-launch blocked FP64 Cholesky (padded factor, info, abort)",
        py::arg("a"), py::arg("l"), py::arg("linv"), py::arg("ctl"), py::arg("status"));
  m.def("cholesky_tiles", &tea::cholesky_tiles, "K9d 64 x 64 tiles per side");
  m.def("pivchol", &pivchol, "K9p pivoted FP64 Cholesky (rank-revealing, W rows in feature order)", py::arg("a"),
        py::arg("slots"), py::arg("w"), py::arg("piv"), py::arg("info"), py::arg("ctl"));
  m.def("pivchol_padded", &tea::pivchol_padded, "K9p factor row stride");
  m.def("fid_finish", &fid_finish, "FID's closing combination in one launch");
  m.def("pivchol_slot_words", &tea::pivchol_slot_words, "K9p hand-off slot words");
  m.def("pivchol_traced", &pivchol_traced, "K9p with per-panel phase stamps (profiling hook)");
  m.def("cholesky_factor_traced", &cholesky_factor_traced, "K9d with per-column phase stamps (profiling hook)");
  m.def("cov_finalize", &cov_finalize, "FP64 symmetric covariance from FP32 FID states", py::arg("cov_sum"),
        py::arg("colsum"), py::arg("n"), py::arg("out"));
  m.def("sym_fill_upper", &sym_fill_upper, "mirror the lower triangle of a float64 matrix into its upper",
        py::arg("m"));
  m.def("sym_eigvals", &sym_eigvals,
        "K9b eigenvalues of a symmetric float64 matrix (on-chip Householder + multisection)", py::arg("m"),
        py::arg("lam"), py::arg("status"));
}

TORCH_LIBRARY_FRAGMENT(torcheval_amd, m) {
  m.def("fid_cov_update(Tensor act, Tensor(a!) cov, Tensor(b!)? colsum) -> ()");
  // no Meta kernel: the returned code (launched / not handled) depends on the device, and the
  // caller branches on it on the host
  m.def("sym_eigvals(Tensor m, Tensor(a!) lam, Tensor(b!) status) -> int");
  m.def("cholesky_factor(Tensor a, Tensor(a!) l, Tensor(b!) linv, Tensor(c!) ctl, Tensor(d!) status) -> ()");
  m.def("pivchol(Tensor a, Tensor(a!) slots, Tensor(b!) w, Tensor(c!) piv, Tensor(d!) info, Tensor(e!) ctl) -> int");
  m.def("cov_finalize(Tensor cov_sum, Tensor colsum, float n, Tensor(a!) out) -> ()");
  m.def("sym_fill_upper(Tensor(a!) m) -> ()");
  m.def("fid_finish(Tensor sum1, float n1, Tensor sum2, float n2, Tensor s1, Tensor s2, Tensor lam, Tensor(a!) out) -> ()");
}

TORCH_LIBRARY_IMPL(torcheval_amd, CUDA, m) {
  m.impl("fid_cov_update", &fid_cov_update);
  m.impl("sym_eigvals", &sym_eigvals);
  m.impl("cholesky_factor", &cholesky_factor);
  m.impl("pivchol", &pivchol);
  m.impl("cov_finalize", &cov_finalize);
  m.impl("sym_fill_upper", &sym_fill_upper);
  m.impl("fid_finish", &fid_finish);
}

TORCH_LIBRARY_IMPL(torcheval_amd, Meta, m) {
  m.impl("fid_cov_update", &MetaNoop<&fid_cov_update>::call);
  m.impl("cholesky_factor", &MetaNoop<&cholesky_factor>::call);
  m.impl("pivchol", [](const Tensor&, const Tensor&, const Tensor&, const Tensor&, const Tensor&, const Tensor&) {
    return int64_t{0};
  });
  m.impl("cov_finalize", &MetaNoop<&cov_finalize>::call);
  m.impl("sym_fill_upper", &MetaNoop<&sym_fill_upper>::call);
  m.impl("fid_finish", &MetaNoop<&fid_finish>::call);
}
