// Host-visible launcher interface of the torcheval_amd HIP kernels.
// Every launcher enqueues on the given HIP stream and returns hipError_t as int (0 = ok,
// -1 = unsupported argument combination, caller must fall back).
#pragma once

#include <hip/hip_runtime_api.h>
#include <stdint.h>

#include "tea_types.h"

namespace tea {

// ------------------------------------------------------------------ K1 classification
struct ClsCountsArgs {
  const void* input = nullptr;  // [n, c] scores (c > 0) or [n] integer labels (c == 0)
  DType in_dt = DType::f32;
  int64_t n = 0;
  int64_t c = 0;
  int64_t row_stride = 0;  // elements between rows of ``input``
  const void* target = nullptr;  // [n] integer labels
  DType tg_dt = DType::i64;
  int k = 1;                     // top-k (k > 1: rank-of-target)
  int64_t num_classes = 0;       // histogram width
  float* micro_correct = nullptr;
  float* micro_incorrect = nullptr;
  float* micro_total = nullptr;   // += n
  float* micro_total2 = nullptr;  // += n (second destination)
  float* cls_correct = nullptr;  // [num_classes] correct at target class
  float* cls_label = nullptr;    // [num_classes] samples per target class
  float* cls_pred = nullptr;     // [num_classes] samples per predicted class
  float* cls_fp = nullptr;       // [num_classes] wrong predictions per predicted class
  float* confusion = nullptr;    // [num_classes, num_classes] (target, pred)
  int* err = nullptr;            // error bits (1: bad target, 2: bad prediction)
  int* err_max = nullptr;        // optional [2]: largest target / prediction >= num_classes
  int check_target = 0;          // flag bad targets even without histograms
  unsigned long long* fold_ws = nullptr;  // tea_fold.h cells (per-stream, self-cleaning)
  // micro kernel only: per-wave correct counts go to these 64 pending cells (u64, 64-B stride)
  // instead of the fold into micro_correct; launch_micro_finish folds them later
  unsigned long long* pend = nullptr;
  int max_blocks = 0;
};
int launch_cls_counts(const ClsCountsArgs& a, hipStream_t stream);
// pending cells -> correct (+= their sum, cells zeroed); out = correct / total when given
constexpr int kPendCells = 64;
constexpr int kPendStride = 8;
int launch_micro_finish(unsigned long long* pend, float* correct, const float* total, float* out, hipStream_t stream);

struct BinaryCountsArgs {
  const void* input = nullptr;
  DType in_dt = DType::f32;
  const void* target = nullptr;
  DType tg_dt = DType::f32;
  const void* weight = nullptr;
  DType w_dt = DType::f32;
  int64_t n = 0;
  float threshold = 0.5f;     // rounded to the score dtype by the caller (bf16 / f16), widened to f32
  double threshold64 = 0.5;   // float64 scores compare in double
  int strict_binary = 0;  // non-{0,1} targets count nowhere (1) or as the "other" class (0)
  float* out[4] = {nullptr, nullptr, nullptr, nullptr};   // tp, fp, tn, fn
  float* out2[4] = {nullptr, nullptr, nullptr, nullptr};  // optional second destinations
  float* total = nullptr;  // += n (sample count)
  int max_blocks = 0;
};
int launch_binary_counts(const BinaryCountsArgs& a, hipStream_t stream);

// ------------------------------------------------------------------ K10 rank-of-target scores
struct RankArgs {
  const void* input = nullptr;  // [n, c] scores, unit column stride
  DType in_dt = DType::f32;
  int64_t n = 0;
  int64_t c = 0;
  int64_t row_stride = 0;
  const void* target = nullptr;  // [n] integer class index
  DType tg_dt = DType::i64;
  int mode = 0;  // 0: hit rate (rank < k), 1: reciprocal rank (0 beyond k when k > 0)
  int k = 0;
  float* out = nullptr;  // [n] float32 scores
  int* err = nullptr;    // bit 0: target out of range (row scored NaN)
};
int launch_rank_scores(const RankArgs& a, hipStream_t stream);

}  // namespace tea

namespace tea {

// ------------------------------------------------------------------ K3 sort-scan (AUROC/AUPRC)
struct AucScanArgs {
  int payload_kind = 0;  // 0: order = source index (gather); 1: order32 = f32 target bits; 2: order32 = class label
  const void* sorted = nullptr;  // [rows, n] scores sorted descending (f32 or f64)
  DType key_dt = DType::f32;
  int64_t key_stride = 0;
  const int64_t* order = nullptr;  // [rows, n] sort permutation (int64, torch.sort) ...
  const int32_t* order32 = nullptr;  // ... or int32 (K3a radix sort); exactly one is set
  int64_t order_stride = 0;
  const void* target = nullptr;  // binary: [rows, n] (row stride) / class mode: [n] labels
  DType tg_dt = DType::f32;
  int64_t target_stride = 0;
  const void* weight = nullptr;  // optional [rows, n]
  DType w_dt = DType::f32;
  int64_t weight_stride = 0;
  int class_mode = 0;  // positives are samples whose label == row index
  int64_t rows = 0;
  int64_t n = 0;
  double* out_auroc = nullptr;  // [rows]
  double* out_auprc = nullptr;  // [rows]
  // the onesweep sort's look-back timeout word of this stream (RadixArgs::os_hdr + 8) or null:
  // non-zero means the sort that produced `sorted` may have misplaced keys, and every output of
  // this scan is NaN instead of a wrong number
  const uint32_t* sort_fault = nullptr;
  // sample-sharded (distributed) mode: per-row (TP, FP) that precede this shard in the global
  // descending order, and raw sums [rows, 4] = (roc sum, pr sum, local P, local N) instead of
  // the normalised areas (the caller all-reduces them and normalises by the global P, N)
  const double* init = nullptr;  // [rows, 2]
  double* out_raw = nullptr;     // [rows, 4]
  // workspace carve-up (set by the launcher)
  void* ab = nullptr;
  void* tsum = nullptr;
  void* tstart = nullptr;
  void* tarea = nullptr;
  void* totals = nullptr;
  // K3c curve emission (PR curves / recall at fixed precision)
  int32_t* tcnt = nullptr;    // [rows, ntiles] tie-group tails per tile
  int32_t* cstart = nullptr;  // [rows, ntiles] exclusive scan of tcnt
  int64_t* sizes = nullptr;   // out [rows]: tie groups G_r (curve points without the final one)
  const int64_t* row_off = nullptr;  // [rows] threshold offset of row r (precision / recall: + r)
  float* out_prec = nullptr;  // [sum G_r + rows], ascending thresholds, final (1, 0) point per row
  float* out_rec = nullptr;
  void* out_thr = nullptr;    // [sum G_r], key dtype
  float min_precision = 0.f;  // RAFP mode
  float* s_rec = nullptr;     // [rows, n] recall per group (descending group order)
  void* s_thr = nullptr;      // [rows, n] threshold per group (key dtype)
  int32_t* gstar = nullptr;   // [rows] last group with precision >= min_precision (-1: none)
  int32_t* glo = nullptr;     // [rows] first group whose recall equals the maximum
  float* out_max_recall = nullptr;  // [rows]
  void* out_best_thr = nullptr;     // [rows], key dtype
};
int64_t auc_scan_workspace_bytes(int64_t rows, int64_t n);
int launch_auc_scan(AucScanArgs a, void* workspace, hipStream_t stream);
// K3c: workspace for the curve passes; count (tile sums + tie-group tails, per-row scan, G_r
// into a.sizes), emit (the compact ascending curves; a.row_off from the host after reading
// sizes) and the sync-free recall-at-fixed-precision chain (count + emit + search + finalize).
int64_t curve_workspace_bytes(int64_t rows, int64_t n, bool rafp);
// K3m: merge two descending-sorted (score, u32 payload) runs into ko / vo (merge path)
// va / vb may be null: the payload is then base_a + i (base_b + j), the sample's position.
// splits: merge_splits_count(na + nb) int64 of scratch.
constexpr int kMergeTile = 2048;
int64_t merge_splits_count(int64_t n);
int launch_merge_desc(const float* ka, const uint32_t* va, int64_t na, uint32_t base_a, const float* kb,
                      const uint32_t* vb, int64_t nb, uint32_t base_b, float* ko, uint32_t* vo, int64_t* splits,
                      hipStream_t stream);
int launch_curve_count(AucScanArgs& a, void* workspace, bool rafp, hipStream_t stream);
int launch_curve_emit(AucScanArgs a, void* workspace, bool rafp, hipStream_t stream);
int launch_rafp(AucScanArgs a, void* workspace, hipStream_t stream);

}  // namespace tea

namespace tea {

// ------------------------------------------------------------------ K4 binned histograms
struct BinnedArgs {
  const void* input = nullptr;  // element (i, j) at i * in_row_stride + j * in_col_stride
  DType in_dt = DType::f32;
  int64_t n = 0;  // samples
  int64_t c = 0;  // classes / labels / tasks
  int64_t in_row_stride = 0;
  int64_t in_col_stride = 0;
  const void* target = nullptr;
  DType tg_dt = DType::i64;
  int mode = 0;  // 0: target(i, j) == 1 is positive; 1: labels, target(i) == j
  int64_t tg_row_stride = 0;
  int64_t tg_col_stride = 0;
  const float* thr = nullptr;  // [T] sorted ascending
  int T = 0;
  int uniform = 0;             // thr is exactly torch.linspace(0, 1, T) (host-known)
  unsigned* ws = nullptr;      // [16 replicas, T + 1, c, 2] u32, zero on entry, left zeroed
  unsigned* slab = nullptr;    // dense path scratch [G, (T + 1) * c] u32, no zero contract
  float* tp = nullptr;         // outputs (accumulated): index k * out_k_stride + j * out_c_stride
  float* fp = nullptr;
  float* fn = nullptr;
  int64_t out_k_stride = 0;
  int64_t out_c_stride = 0;
};
int64_t binned_workspace_words(int T, int64_t c);
int64_t binned_slab_words(int T, int64_t c);  // 0 when the dense path is not used
struct BinnedFinalizeArgs {
  const float* tp = nullptr;  // [T, rows] counts, element (k, r) at k * k_stride + r * r_stride
  const float* fp = nullptr;
  const float* fn = nullptr;  // needed for AUPRC
  int64_t k_stride = 0, r_stride = 0;
  int T = 0;
  int64_t rows = 0;
  double* out_auroc = nullptr;  // [rows] float64 (reference: trapz(...).double())
  float* out_auprc = nullptr;   // [rows] float32
  float* out_prec = nullptr;    // [rows, T + 1] float32 binned PR curve (precision, then 1)
  float* out_rec = nullptr;     // [rows, T + 1] float32 (recall, then 0)
};
int launch_binned_finalize(const BinnedFinalizeArgs& a, hipStream_t stream);
int launch_binned(const BinnedArgs& a, hipStream_t stream);

}  // namespace tea

namespace tea {

// ------------------------------------------------------------------ K5 column moments
struct MomentsArgs {
  const void* x = nullptr;  // element (i, j) at i * x_row_stride + j * x_col_stride
  DType x_dt = DType::f32;
  int64_t x_row_stride = 0, x_col_stride = 0;
  const void* t = nullptr;
  DType t_dt = DType::f32;
  int64_t t_row_stride = 0, t_col_stride = 0;
  const void* w = nullptr;  // optional per-row weight
  DType w_dt = DType::f32;
  int64_t w_stride = 0;
  int64_t n = 0, d = 0;
  float* sse = nullptr;  // [d] outputs (accumulated), element j at j * out_stride
  float* st = nullptr;
  float* stt = nullptr;
  float* sx = nullptr;
  float* sw = nullptr;   // scalar
  int64_t out_stride = 1;
  double* ws = nullptr;  // [ws_blocks, n_requested_stats * d + 1] FP64 partials (caller-allocated)
  int ws_blocks = 0;
  int overwrite = 0;     // 1: outputs are written (=), not accumulated (fresh functional buffers)
  // fused functional compute (post-processing of the column sums inside the finalize):
  //   1 MSE raw_values -> mse_out[d]       2 MSE uniform_average -> mse_out scalar (needs sse, sw)
  //   3 R2 raw_values  -> mse_out[d]       4 R2 uniform_average, 5 R2 variance_weighted -> scalar
  //   (R2 needs sse = RSS, st, stt; num_obs / num_regressors give tss and the adjusted score)
  int mse_mode = 0;
  float* mse_out = nullptr;
  float* mse_part_f = nullptr;  // [2 d] scratch: per-column values (+ tss) for the scalar modes
  int64_t num_obs = 0;
  int num_regressors = 0;
  // one-launch form (f32 x / t with unit column stride, d >= 4, f32 or no weight): per column
  // tile, R row-chunk blocks hand FP64 partials to the tile's last arriver (write-through
  // stores + ticket); the scalar modes add one more ticket over the tiles.
  double* part = nullptr;       // column_moments_v2_ws_doubles(...) doubles
  unsigned* tickets = nullptr;  // [tiles + 1], zero, left zero
  int v2_cg = 0;                // column groups (of 4) per tile: 4 / 16 / 64; 0 = two-launch form
  int v2_r = 0;                 // row chunks per tile
  int64_t v2_chunk = 0;         // rows per chunk
  // deferred mode (class updates): each block ADDS its FP64 column partials to its own slot of
  // pend ([slots][ns][d] then [slots] weight totals / row counts) and the launch ends there;
  // launch_moments_fold folds the slots into the float32 states when they are read
  double* pend = nullptr;
  int pend_slots = 0;
};
int column_moments_blocks(int64_t n, int64_t d);
// v2 plan: whether it applies, and its geometry / workspace size (doubles and tickets)
bool column_moments_v2_plan(MomentsArgs& a, int64_t* ws_doubles, int64_t* tickets);
constexpr int kMomentsPendSlots = 64;
// the deferred-mode slot layout: statistic k of the set sits in slot row k, which holds for the
// sets {sse} (need 1), {sse, st, stt} (7) and {sse, st, stt, sx} (15) only: 0 for any other set
// (constexpr: callable from the fold kernel too)
constexpr int moments_ns_of(int need) { return need == 1 ? 1 : need == 7 ? 3 : need == 15 ? 4 : 0; }
constexpr int moments_need(const MomentsArgs& a) {
  return (a.sse ? 1 : 0) | (a.st ? 2 : 0) | (a.stt ? 4 : 0) | (a.sx ? 8 : 0);
}
constexpr int moments_ns(const MomentsArgs& a) { return moments_ns_of(moments_need(a)); }
// pending slots r < rows_used of a deferred-mode pend buffer -> outputs (+= in float32; sse /
// st / stt / sx at out_stride, sw scalar), slots zeroed
int launch_moments_fold(const MomentsArgs& a, int rows_used, hipStream_t stream);
int launch_column_moments(const MomentsArgs& a, hipStream_t stream);

// ------------------------------------------------------------------ K5b per-row weighted sums
// One pass over [rows, n] x (and t, w) producing per row, in FP64, any of
//   WX = sum w x   WT = sum w t   W = sum w   SSE = sum (x - t)^2   WSSE = sum w (x - t)^2
//   WTT = sum w t^2   TMIN / TMAX = min / max t
//   COUNT = n      RANGE = (merged TMAX output) - (merged TMIN output)
// (w: an elementwise weight tensor, or the scalar w_scalar), merged straight into state tensors:
// each output applies op (= / += / min / max) in its own dtype, so a single launch (two for
// long rows) is the whole update of Sum / Mean / PSNR / ClickThroughRate / WeightedCalibration,
// including a windowed metric's ring-slot write and its lifetime accumulation.
enum RowStat : int {
  kWX = 0, kWT = 1, kW = 2, kSSE = 3, kWSSE = 4, kWTT = 5,  // sums
  kTMIN = 6, kTMAX = 7,                                      // extrema
  kCOUNT = 8, kRANGE = 9                                     // derived
};
constexpr int kRowSums = 6, kRowRaw = 8;
enum RowOp : int { kSet = 0, kAdd = 1, kMin = 2, kMax = 3 };
constexpr int kRowSumsMaxOut = 10;
struct RowSumsOut {
  void* p = nullptr;  // element r at r * stride
  DType dt = DType::f64;
  int64_t stride = 0;
  int stat = 0;
  int op = 0;
  int first_row_only = 0;  // a scalar state fed by row 0 only (e.g. a shared count)
};
struct RowSumsArgs {
  const void* x = nullptr;  // element (r, i) at r * x_rs + i * x_cs
  DType x_dt = DType::f32;
  int64_t x_rs = 0, x_cs = 1;
  const void* t = nullptr;
  DType t_dt = DType::f32;
  int64_t t_rs = 0, t_cs = 1;
  const void* w = nullptr;
  DType w_dt = DType::f32;
  int64_t w_rs = 0, w_cs = 1;
  double w_scalar = 1.0;
  int64_t rows = 0, n = 0;
  int need = 0;  // bit mask of the raw stats to reduce (WX .. TMAX)
  int nout = 0;
  RowSumsOut out[kRowSumsMaxOut];
  double* ws = nullptr;  // [rows, blocks, kRowRaw] partials when blocks > 1
  unsigned* ticket = nullptr;  // [rows] zeroed arrival counters: one-launch fold (left zeroed)
  int wt = 0;            // with ticket: write-through partials instead of the fat-block fold
  int blocks = 1;        // blocks per row
  // deferred mode (long rows, ADD outputs of sums / W / COUNT only): every grid block ADDS its
  // FP64 partials - already scaled by a scalar weight, W and COUNT included - to its own slot of
  // pend ([rows][kRowPendStats][pend_blocks]) and the launch ends there; launch_row_sums_fold
  // applies the slots to the outputs when the states are read
  double* pend = nullptr;
  int pend_blocks = 0;
};
// ------------------------------------------------------------------ K4b per-sample binned AUROC
// the reference-default multiclass_binned_auroc (binned_auroc.py:189-215): out[i] = the binned
// AUROC of sample i's true-class score against its other classes (csrc/kernels/binned_auroc.hip)
struct SampleAurocArgs {
  const float* input = nullptr;  // [n, c], unit column stride
  int64_t n = 0, c = 0, row_stride = 0;
  const void* target = nullptr;  // [n] int64 / int32
  DType tg_dt = DType::i64;
  int64_t tg_stride = 1;
  const float* thr = nullptr;  // [T] ascending
  int T = 0;
  float* out = nullptr;  // [n]
  int* err = nullptr;    // bit 0: a label outside [0, c)
};
int launch_sample_binned_auroc(const SampleAurocArgs& a, hipStream_t stream);

constexpr int kRowPendStats = kRowSums + 3;  // the six sums, COUNT, then the target min / max
                                             // (a slot's extrema are valid while its COUNT != 0)
constexpr int kRowPendBlocks = 2048;
// pending slots b < blocks_used of every row -> the outputs of a (ADD), slots zeroed
int launch_row_sums_fold(const RowSumsArgs& a, int blocks_used, hipStream_t stream);
int row_sums_blocks(int64_t rows, int64_t n);       // two-launch grid (partials + combine)
int row_sums_fold_blocks(int64_t rows, int64_t n);
int row_sums_wt_blocks(int64_t rows, int64_t n);  // one-launch fold (needs a ticket)
int launch_row_sums(const RowSumsArgs& a, hipStream_t stream);
// the same update on host memory (CPU tensors): the small-batch twin of the kernel
void row_sums_host(const RowSumsArgs& a);

// ------------------------------------------------------------------ K6 normalized entropy
struct NeArgs {
  const void* x = nullptr;
  DType x_dt = DType::f32;
  int64_t x_row_stride = 0;
  const void* t = nullptr;
  DType t_dt = DType::f32;
  int64_t t_row_stride = 0;
  const void* w = nullptr;
  DType w_dt = DType::f32;
  int64_t w_row_stride = 0;
  int64_t rows = 0, n = 0;
  int from_logits = 0;
  double* out = nullptr;  // [rows, 3]: sum w*bce, sum w*t, sum w (accumulated)
  int* err = nullptr;
  // optional: order-preserving u64 keys of max(x) and (complemented) min(x) over the launch,
  // atomicMax-accumulated (zero = unset), so a deferred range error can print the batch range
  unsigned long long* range = nullptr;
  double* ordered_ws = nullptr;  // deterministic mode: [rows * 3, ne_sums_blocks] partials
};
int ne_sums_blocks(int64_t n);
int launch_ne_sums(const NeArgs& a, hipStream_t stream);

// deterministic fold: out[v] += sum_{p < parts} ws[v * parts + p], summed in index order
int launch_ordered_sum(const double* ws, int64_t nvals, int64_t parts, double* out, hipStream_t stream);

}  // namespace tea

namespace tea {

// ------------------------------------------------------------------ K7 perplexity
struct PerplexityArgs {
  const void* input = nullptr;  // [rows, v] logits (row stride)
  DType in_dt = DType::f32;
  int64_t rows = 0, v = 0, row_stride = 0;
  const void* target = nullptr;  // [rows] (stride)
  DType tg_dt = DType::i64;
  int64_t tg_stride = 1;
  int has_ignore = 0;
  int64_t ignore_index = 0;
  double* out = nullptr;  // [2]: sum of -log p(target), token count (accumulated)
  int* err = nullptr;
  double* ordered_ws = nullptr;  // deterministic mode: [2, perplexity_blocks] partials
};
int perplexity_blocks(const PerplexityArgs& a);  // grid of the launch launch_perplexity makes
int launch_perplexity(const PerplexityArgs& a, hipStream_t stream);

}  // namespace tea

namespace tea {

// ------------------------------------------------------------------ K8 FID covariance
struct FidCovArgs {
  const float* act = nullptr;  // [n, ld] activations (row stride, unit column stride)
  int64_t n = 0, d = 0, row_stride = 0;
  int64_t ld = 0;               // loaded width: d rounded up to 4 (columns [d, ld) must be 0)
  const float* zeros = nullptr;  // >= 16 B of zeros (the source of masked LDS-DMA slots)
  float* cov = nullptr;     // [d, d] contiguous, += act^T act
  float* colsum = nullptr;  // [d], += column sums (optional)
  int split = 1;            // K-range items per output tile (> 1: partials + fix-up pass)
  float* ws = nullptr;      // split > 1: fid_cov_workspace_bytes(d, split) of scratch
};
// split-K factor the launcher would pick for [n, d] on this device (env TORCHEVAL_AMD_K8_SPLIT
// overrides) and the scratch it needs
int fid_cov_split(int64_t n, int64_t d);
// K8 product path: 2 = bf16 MFMA on the exact three-way split, staged once per block (default);
// 1 = the same split done per wave (TORCHEVAL_AMD_K8_MODE=1); 0 = FP32 MFMA (TORCHEVAL_AMD_K8_EXACT=1)
int fid_cov_mode();
int64_t fid_cov_workspace_bytes(int64_t d, int split);
int launch_fid_cov(const FidCovArgs& a, hipStream_t stream);

}  // namespace tea

// ------------------------------------------------------------------ K2 multilabel accuracy
namespace tea {
struct MultilabelArgs {
  const void* x = nullptr;  // [n, c] scores (f32 / bf16 / f16), rows at x_row_stride
  DType x_dt = DType::f32;
  int64_t x_row_stride = 0;
  const void* t = nullptr;  // [n, c] targets (f32 / i64 / i32 / u8 / bool)
  DType t_dt = DType::f32;
  int64_t t_row_stride = 0;
  int64_t n = 0, c = 0;
  float threshold = 0.5f;
  int k = 0;         // > 0: top-k labels instead of thresholding
  int criteria = 0;  // 0 exact_match, 1 hamming, 2 overlap, 3 contain, 4 belong
  float* num_correct = nullptr;  // accumulated
  float* num_total = nullptr;    // optional: += total (block 0)
  double total = 0.0;
  unsigned long long* fold_ws = nullptr;
};
int multilabel_max_topk_cols();
int launch_multilabel(const MultilabelArgs& a, hipStream_t stream);
}  // namespace tea

// ------------------------------------------------------------------ K3a radix sort
namespace tea {
struct RadixArgs {
  const float* in = nullptr;  // [rows, n] scores, rows at in_row_stride (unit column stride)
  int64_t in_row_stride = 0;
  int64_t rows = 0, n = 0;
  int64_t tiles = 0;          // radix_sort_tiles(rows, n)
  uint32_t* keys0 = nullptr;  // ping-pong [rows * n]
  uint32_t* vals0 = nullptr;
  uint32_t* keys1 = nullptr;
  uint32_t* vals1 = nullptr;
  uint32_t* hist = nullptr;   // [rows, tiles, 256] per-tile digit counts of the current pass
  uint32_t* groups = nullptr; // 4 pass regions (`region` cells apart) of [rows, ngroups, 256] digit
                              // counts per group of tiles.  Self-cleaning: passes 1-3 clear the
                              // previous pass's region; pass 3's is cleared by the next sort's pass 0
                              // (a last-block-done clear in the final downsweep serialised 512
                              // same-address atomics: +5 us per 1M-key sort)
  int64_t region = 0;
  uint32_t* dirty = nullptr;  // cells of region 3 left to clear (written by the final downsweep)
  int64_t ngroups = 0;        // radix_sort_groups(tiles)
  float* out_sorted = nullptr;  // [rows, n] descending
  int32_t* out_order = nullptr; // [rows, n] source index within the row (or the payload)
  // optional payload carried instead of the source index (pass 0 reads it, coalesced):
  //   1: f32 bits of payload[row * payload_row_stride + i]  (binary targets)
  //   2: int32 of payload[row * payload_row_stride + i]     (class labels; row stride 0 = shared)
  int payload_kind = 0;
  const void* payload = nullptr;
  DType payload_dt = DType::f32;
  int64_t payload_row_stride = 0;
  // onesweep mode (radix_onesweep_ok): one histogram launch for all four digits, then four
  // passes that each rank, look back and scatter in ONE launch (no upsweeps).  Self-cleaning,
  // zero-initialised workspaces:
  uint32_t* os_hdr = nullptr;     // [16]: [4..7] dirty extents of the status / group planes,
                                  // [8] look-back timeout flag (cleared by each sort's histogram
                                  // launch, so it describes the latest onesweep sort of the stream)
  uint32_t* os_watch = nullptr;   // host (pinned) word: the histogram launch copies [8] there before
                                  // clearing it, so the host learns of a timed-out sort one sort
                                  // later without a device-to-host copy on the stream
  int spin_limit = 1 << 22;       // look-back polls before a tile gives up (TORCHEVAL_AMD_K3_SPIN_LIMIT)
  uint32_t* os_g = nullptr;       // [rows, 8 copies, 4, 256] digit totals (hist kernel; cleared by pass 3)
  uint32_t* os_status = nullptr;  // 2 planes of [rows * tiles, 256] ready-flagged tile counts
  int64_t os_splane = 0;          // words per status plane
  unsigned long long* os_gacc = nullptr;  // 2 planes of [rows * ngroups, 256] (arrivals << 32 | sum)
  int64_t os_gplane = 0;          // words per group plane
  // 0: descending (NaN first); ~0u: ascending (NaN last, as torch.sort ascending), both stable -
  // XORed into every key at load and out of it at the final store
  uint32_t key_xor = 0;
};
bool radix_onesweep_ok(int64_t rows, int64_t n);  // the tiling the onesweep passes take
int64_t radix_onesweep_status_words(int64_t rows, int64_t n);
int64_t radix_onesweep_group_words(int64_t rows, int64_t n);
int radix_sort_rounds(int64_t rows, int64_t n);  // keys per thread of the tiling
int64_t radix_sort_tiles(int64_t rows, int64_t n);
int64_t radix_sort_groups(int64_t tiles);
int launch_transpose_f32(const float* in, int64_t n, int64_t c, int64_t ld_in, float* out, hipStream_t stream);
int launch_radix_sort_desc(const RadixArgs& a, hipStream_t stream);
// ------------------------------------------------------------------ K10b retrieval top-k
struct RetrievalArgs {
  const float* x = nullptr;        // [n] scores
  const float* t = nullptr;        // [n] targets
  const int64_t* q = nullptr;      // [n] query ids (null: every sample is query 0)
  int64_t n = 0, Q = 0;
  int k = 0;                        // 1..64
  float* topk = nullptr;            // [Q, k] state (best first, -inf padded)
  float* target_state = nullptr;    // [Q, k]
  int64_t* count = nullptr;         // [Q] valid entries (<= k)
  int* counts = nullptr;            // [Q] zeroed scratch (left zeroed)
  int* offsets = nullptr;           // [Q + 1] scratch
  int* cursor = nullptr;            // [Q] scratch
  uint32_t* rec_key = nullptr;      // [n] scratch
  uint32_t* rec_idx = nullptr;      // [n] scratch
};
constexpr int kRetrievalMaxLds = 64 * 1024;  // 2 x Q int32 of LDS: Q <= 8192
int launch_retrieval_topk(const RetrievalArgs& a, hipStream_t stream);

}  // namespace tea

namespace tea {

// ------------------------------------------------------------------ K9b symmetric eigenvalues
struct SymEigArgs {
  const double* a = nullptr;  // [n, n] symmetric, contiguous
  int64_t n = 0;
  int64_t ld = 0;             // slot stride, symeig_slot_stride(n)
  double* d = nullptr;        // [n] tridiagonal diagonal (workspace)
  double* e = nullptr;        // [n] off-diagonal (workspace)
  double* lam = nullptr;      // [n] eigenvalues, ascending
  unsigned long long* slots = nullptr;  // 2 planes of [n - 2, ld] hand-off slots,
                                        // symeig_slot_bytes(n) (sentinel-filled by the launcher)
  unsigned* ctl = nullptr;    // 128 B: ctl[1] abort word (zeroed by the launcher)
  int* grid = nullptr;        // symeig_grid_bytes(): Sturm counts of the eigenvalue search grid
  double* tail = nullptr;     // symeig_tail_bytes(): the trailing block the one-workgroup tail finishes
};
// 0 when the on-chip one-launch reduction fits this device (grid / rows per block out)
int symeig_plan(int64_t n, int* grid, int* rows_per_block);
int64_t symeig_slot_stride(int64_t n);
int64_t symeig_slot_bytes(int64_t n);
int64_t symeig_grid_bytes();
int64_t symeig_tail_bytes();
// 0 launched, 1 unsupported size, 2 HIP error, 3 cooperative launch refused
int launch_symeig(const SymEigArgs& a, hipStream_t stream);

}  // namespace tea

namespace tea {
// K9d (cholesky.hip): the whole blocked Cholesky in one persistent launch.  L: padded
// [64 nt, 64 nt] factor, Linv: nt x 64 x 64, ctl: 1 int (ticket), status: 2 ints (info, abort)
int cholesky_tiles(int64_t n);
// fid_prep.hip: S = ((C + C^T) / 2 - n mu mu^T) / (n - 1) in FP64 from the FP32 K8 states;
// M[i][j] = M[j][i] above the diagonal (in place)
// trapz.hip: per-row trapezoid area of x-sorted rows (x, y f32 [rows, n]) -> out f32 [rows];
// part: FP64 scratch of rows * trapz_blocks(n)
int trapz_blocks(int64_t n);
int launch_trapz_sorted(const float* x, const float* y, int64_t rows, int64_t n, double* part, float* out,
                        hipStream_t stream);
int launch_cov_finalize(const float* C, const float* colsum, double n, int64_t d, double* S, hipStream_t stream);
int launch_sym_fill_upper(double* M, int64_t ld, int64_t n, hipStream_t stream);
int launch_fid_finish(const float* sum1, double n1, const float* sum2, double n2, int64_t d, const double* s1,
                      int64_t ld1, const double* s2, int64_t ld2, const double* lam, int64_t r, float* out,
                      hipStream_t stream);
int launch_cholesky(const double* A, int64_t lda, int64_t n, double* L, double* Linv, int* ctl, int* status,
                    hipStream_t stream, unsigned long long* trace = nullptr);
// K9p (pivchol.hip): pivoted FP64 Cholesky, one cooperative launch.  slots: pivchol_slot_words(n)
// 64-bit words, w: [N, N] doubles, N = pivchol_padded(n); info {rank, status}; ctl 1 word.
// 0 launched, 3 not co-schedulable, 4 n unsupported
int pivchol_padded(int64_t n);
int64_t pivchol_slot_words(int64_t n);
int launch_pivchol(const double* A, int64_t lda, int64_t n, unsigned long long* slots, double* w, int* piv, int* info,
                   unsigned* ctl, hipStream_t stream, unsigned long long* trace = nullptr);
}  // namespace tea

namespace tea {
// C3: reduce a gathered [ws][row_bytes] metric-state buffer segment by segment across ranks
// (rank 0 first) into ``out`` (same byte layout).  op: 0 sum, 1 max, 2 min; dtype: DType.
constexpr int kSegMax = 32;
struct SegReduceArgs {
  const uint8_t* rows = nullptr;
  uint8_t* out = nullptr;
  int ws = 1;
  int64_t row_bytes = 0;
  int nseg = 0;
  int64_t off[kSegMax] = {};        // byte offset of each segment in a row
  int64_t first[kSegMax + 1] = {};  // prefix sum of segment element counts
  int dtype[kSegMax] = {};
  int op[kSegMax] = {};
};
int launch_seg_reduce(const SegReduceArgs& a, hipStream_t stream);
// copy ``bytes`` (multiple of 16) of src to dst and append this rank's flag words as f32 (hi16,
// lo16) pairs in slot ``rank`` of a zeroed [ws][words][2] block (err null: zeros)
int launch_snapshot_flags(const void* src, void* dst, int64_t bytes, const int* err, int words, int rank, int ws,
                          hipStream_t stream);
// summed [ws][words][2] slots -> int32 [words], max over ranks
int launch_merge_flag_slots(const float* slots, int* out, int words, int ws, hipStream_t stream);
// test support (csrc/kernels/testing.hip): one lane spins until *flag != 0 or max_ms elapse
// low-latency host read (hostread.hip): words <= kHostReadWords int32 from src into a pinned,
// device-mapped host slot [seq, words...], published by a system-scope release store of seq
constexpr int kHostReadWords = 14;
int launch_publish_words(const int32_t* src, int words, int32_t* slot_dev, int32_t seq, hipStream_t stream,
                         const int32_t* src2 = nullptr, int words2 = 0);
int launch_spin_on_flag(const int* flag, int64_t max_ms, hipStream_t stream);
}  // namespace tea

namespace tea {
// K12: structural similarity of contiguous [n, c, h, w] image pairs (csrc/kernels/ssim.hip).
// One workgroup per (plane, kSsimTileH x kSsimTileW output tile) writes an FP64 partial; the
// finish launch turns them into per-image values (or their mean) and the class states.
constexpr int kSsimTileH = 64;
constexpr int kSsimTileW = 64;
constexpr int kSsimMaxKs = 15;
constexpr int64_t kSsimMaxPlanes = (int64_t{1} << 24) - 1;  // grid.x * 256 threads stays below 2^32
struct SsimArgs {
  const void* x = nullptr;
  const void* y = nullptr;
  DType dt = DType::f32;  // f32 / f16 / bf16 / u8, both inputs
  int64_t n = 0, c = 0;
  int h = 0, w = 0;
  int ks = 11;                    // odd, 3..kSsimMaxKs
  float taps[kSsimMaxKs] = {};    // the 1-D window, normalised on the host in FP64
  float c1 = 0.f, c2 = 0.f;
  double* partial = nullptr;      // [n * c * ssim_tiles(h, w, ks)] scratch
  float* out = nullptr;           // [n] values, or [1] mean when ``mean``; may be null
  int mean = 0;
  double* mssim_sum = nullptr;    // class states (both or neither): += sum of the n values, += n
  double* num_images = nullptr;
};
int64_t ssim_tiles(int64_t h, int64_t w, int64_t ks);  // output tiles per plane
bool ssim_geometry_ok(int64_t planes, int64_t h, int64_t w, int64_t ks);
int launch_ssim(const SsimArgs& a, hipStream_t stream);
}  // namespace tea

namespace tea {
// K13: normalized discounted cumulative gain per row of [n, c] scores / graded relevance
// (csrc/kernels/ndcg.hip).  c <= 64 runs a wave per row, larger c a workgroup per row with the
// row sorted in LDS; kNdcgMaxColumns keeps two such workgroups on a CU (2 * 4096 * 8 B each).
constexpr int kNdcgMaxColumns = 4096;
struct NdcgArgs {
  const void* x = nullptr;  // [n, c] scores, unit column stride: f32 / f16 / bf16
  DType x_dt = DType::f32;
  int64_t x_stride = 0;     // elements between rows
  const void* t = nullptr;  // [n, c] relevance, unit column stride: f32 / f16 / bf16 / i64 / i32 / i16 / i8 / u8
  DType t_dt = DType::i64;
  int64_t t_stride = 0;
  int64_t n = 0;
  int c = 0;                // 1 .. kNdcgMaxColumns
  int k = 0;                // cutoff, 1 .. c
  int exponential = 0;      // gain 2^t - 1 instead of t
  const double* D = nullptr;  // [k + 1] prefix sums of 1 / log2(r + 2), D[0] = 0
  float* out = nullptr;       // [n] row values; may be null when the class states are given
  double* partial = nullptr;  // [ndcg_blocks(n, c)] scratch, with the class states
  double* ndcg_sum = nullptr;   // class states (both or neither): += sum of the row values, += n
  double* num_rows = nullptr;
  int* err = nullptr;           // bit 0: a relevance with !(t >= 0) (row scored NaN)
};
int ndcg_blocks(int64_t n, int64_t c);  // grid of the row launch = number of partials
int launch_ndcg(const NdcgArgs& a, hipStream_t stream);
}  // namespace tea

namespace tea {
// K14: Spearman rank correlation per row (csrc/kernels/rankcorr.hip) of two operands that K3a has
// sorted as one [2 rows, n] stack, the first operand's rows and then the second's (descending
// sorted rows and their int32 source permutations, payload_kind 0).
constexpr int kRankCenterSpan = 2048;   // sorted positions a rank_center block resolves in LDS
constexpr int kRankMomentsSpan = 4096;  // elements per round of a rank_moments block; its span is a multiple
struct RankCorrArgs {
  const float* sorted = nullptr;   // [2 rows, n] sorted keys, contiguous
  const int32_t* order = nullptr;  // [2 rows, n] source index of each sorted position
  int64_t rows = 0;
  int64_t n = 0;                // 2 .. 2^31 - 1
  int32_t* c = nullptr;         // [2, rows, pitch] centred doubled ranks in source order, 16-byte aligned
  int64_t pitch = 0;            // rank_corr_pitch(n)
  int32_t* nan_flag = nullptr;  // [2, rows]: the operand's row holds a NaN
  double* part = nullptr;       // [rows, rank_moments_blocks(n), 3] scratch: sxy, sxx, syy
  const uint32_t* sort_fault = nullptr;  // K3a's onesweep timeout word or null (non-zero: every row scores NaN)
  float* out = nullptr;         // [rows]
};
int64_t rank_corr_pitch(int64_t n);
int rank_moments_blocks(int64_t n);
int launch_rank_corr(const RankCorrArgs& a, hipStream_t stream);
}  // namespace tea

namespace tea {
// K15: multiclass calibration error (csrc/kernels/calibration.hip).  One pass over [n, c] scores
// finds each row's argmax and confidence (the row maximum, or 1 / sum exp(x - max) for logits) and
// folds (count, correct, confidence) into n_bins bins whose edges are float32(b / n_bins).
// kCalibMaxBins: a 4-wave block holds 4 wave-private bin sets (u32 count, u32 correct, f64
// confidence: 64 B per bin) plus the edge table, 17 KiB at the cap, so the 8 blocks a CU can hold
// at full occupancy fit its 160 KiB of LDS.
constexpr int kCalibMaxBins = 256;
constexpr int kCalibMaxBlocks = 1024;  // grid cap of the row launch, both arms
constexpr int kCalibNarrowMaxC = 32;   // a thread owns a row up to here, a wave above
struct CalibrationArgs {
  const void* input = nullptr;  // [n, c] f32 / f16 / bf16, unit column stride, element-aligned rows
  DType in_dt = DType::f32;
  int64_t row_stride = 0;       // elements
  const void* target = nullptr; // [n] int64 / int32, contiguous
  DType tg_dt = DType::i64;
  int64_t n = 0;
  int64_t c = 0;                // 1 .. 2^31 - 1
  int n_bins = 0;               // 1 .. kCalibMaxBins
  int from_logits = 0;
  int* err = nullptr;           // bit 0: target outside [0, c); bit 1: confidence outside [0, 1]
  double* partial = nullptr;    // [calibration_blocks(n, c), 3, n_bins] scratch
  // the finish launch: dst[s][b] (+)= the partials of state s (count, correct, confidence) added in
  // block order; `accumulate` 0 overwrites (the functional's scratch triple).  With `out`, the same
  // launch then evaluates the value from dst
  double* dst[3] = {nullptr, nullptr, nullptr};
  int accumulate = 0;
  int norm = 0;                 // 0: l1 (ECE), 1: max (MCE), 2: l2
  float* out = nullptr;
};
int calibration_blocks(int64_t n, int64_t c);  // grid of the row launch = number of partial triples
int launch_calibration(const CalibrationArgs& a, hipStream_t stream);
// the value of three [n_bins] float64 states, by one wave
int launch_calibration_value(const double* bin_count, const double* correct_sum, const double* conf_sum, int n_bins,
                             int norm, float* out, hipStream_t stream);
}  // namespace tea

namespace tea {
// K16: Pearson and concordance correlation per task (csrc/kernels/corrcoef.hip) from six FP64
// moments per task, the rows of a [6, tasks] state: n, mean_x, mean_y, m2_x, m2_y, c_xy
// (docs/parity.md, "Not in the reference").  A batch's moments are formed from five sums of
// differences to the task's first sample and merged into the state by the pairwise update.
constexpr int kCorrRowSpan = 4096;  // samples of one task a row-arm block owns
constexpr int kCorrColSpan = 128;   // samples (of 64 tasks each) a column-arm block owns
constexpr int kCorrColTasks = 64;   // task columns of a column-arm block, one per lane
struct CorrcoefArgs {
  // element (task, i) of an operand is at task * task_stride + i * sample_stride (elements).
  // Row arm: sample strides 1, any task strides.  Column arm: task strides 1.
  const void* x = nullptr;      // f32 / f16 / bf16, element-aligned
  const void* y = nullptr;
  DType x_dt = DType::f32;
  DType y_dt = DType::f32;
  int64_t x_task_stride = 0, x_sample_stride = 1;
  int64_t y_task_stride = 0, y_sample_stride = 1;
  int64_t tasks = 0;
  int64_t n = 0;                // samples per task, >= 1
  int column = 0;               // 0: row arm, 1: column arm
  double* partial = nullptr;    // [tasks, corrcoef_blocks(n, column), 5] scratch: S_x, S_y, S_xx, S_yy, S_xy
  // the finish launch: with `moments`, the batch merges into that [6, tasks] state in place;
  // with `out`, out[task] <- the batch's value (concordance 0: Pearson, 1: Lin's concordance)
  double* moments = nullptr;
  float* out = nullptr;
  int concordance = 0;
};
int corrcoef_blocks(int64_t n, int column);  // partials per task
int launch_corrcoef(const CorrcoefArgs& a, hipStream_t stream);
// state[6, tasks] <- its pairwise merge with other[6, tasks]; one launch
int launch_corrcoef_merge(double* state, const double* other, int64_t tasks, hipStream_t stream);
// out[task] <- the value of state[6, tasks]; one launch
int launch_corrcoef_value(const double* state, int64_t tasks, int concordance, float* out, hipStream_t stream);
}  // namespace tea

namespace tea {
// K17: segmentation mean IoU and Dice (csrc/kernels/segmentation.hip).  One pass over [n, c, p]
// scores (class axis strided) or over a pair of label maps folds every counted pixel into three
// per-class counts: intersection, predicted and target (docs/parity.md, "Not in the reference").
// kSegMaxClasses: a block holds three u32 [c] histograms in LDS, 12 KiB at the cap; a CU holds at
// most 8 blocks of 256 threads (2048 threads), 8 * 12 KiB = 96 KiB of its 160 KiB.
constexpr int kSegSpan = 2048;        // pixels of one image a block owns at a time
constexpr int kSegMaxBlocks = 1024;   // the persistent grid's cap = the most partial triples
constexpr int kSegMaxClasses = 1024;
struct SegmentationArgs {
  // arm 0 (plane) and 1 (element): element (n, c, p) of the f32 / f16 / bf16 scores is at
  // n * stride_n + c * stride_c + p * stride_p (elements).  The plane arm needs stride_p == 1 and,
  // for 16-bit scores, stride_c % 8 == 0.  Arm 2 (label): `input` is a contiguous [n, p] integer map
  const void* input = nullptr;
  DType in_dt = DType::f32;
  int64_t stride_n = 0, stride_c = 0, stride_p = 1;
  const void* target = nullptr;  // [n, p] u8 / i8 / i16 / i32 / i64, contiguous
  DType tg_dt = DType::i64;
  int64_t n = 0;
  int64_t p = 0;                 // pixels per image
  int c = 0;                     // 1 .. kSegMaxClasses
  int arm = 0;
  int has_ignore = 0;
  int64_t ignore_index = 0;
  int* err = nullptr;            // bit 0: counted target outside [0, c); bit 1: such a label-map prediction
  uint32_t* partial = nullptr;   // [segmentation_blocks(n, p), 3, c] scratch: intersection, pred, target
  // the finish launch: dst[s][k] (+)= the partials of state s added in block order; `accumulate` 0
  // overwrites (the functional's scratch triple).  With `out`, the same launch evaluates the value
  double* dst[3] = {nullptr, nullptr, nullptr};
  int accumulate = 0;
  int dice = 0;                  // 0: IoU, 1: Dice
  int average = 0;               // 0: macro, 1: micro, 2: none ([c] values)
  float* out = nullptr;
};
int segmentation_blocks(int64_t n, int64_t p);  // grid of the count launch = number of partial triples
int launch_segmentation(const SegmentationArgs& a, hipStream_t stream);
// the value of three [c] float64 states (c >= 1, any size), by one wave
int launch_segmentation_value(const double* intersection, const double* pred_count, const double* target_count,
                              int64_t c, int dice, int average, float* out, hipStream_t stream);
}  // namespace tea

namespace tea {
// K18: KL divergence KL(P || Q) of corresponding rows of two [n, c] tensors (csrc/kernels/
// kl_divergence.hip; docs/parity.md, "Not in the reference").  P comes from `target`, Q from
// `input`: their softmaxes (from_logits) or the rows divided by their sums.  One wave streams both
// rows of a counted row pair once and lane 0 forms the row value in FP64.
constexpr int kKlMaxBlocks = 1024;  // grid cap of the row launch in 4-wave blocks; rows past it grid-stride
struct KlDivArgs {
  // Both operands have one dtype (f32 / bf16 / f16), unit stride along c and element-aligned rows;
  // row r of `input` and row r of `target` lie at the same offset from a 16-B boundary.
  const void* input = nullptr;
  const void* target = nullptr;
  DType dt = DType::f32;
  int64_t in_row_stride = 0, tg_row_stride = 0;  // elements
  const uint8_t* mask = nullptr;  // optional [n] bool: a row with 0 is never read and not counted
  int64_t n = 0;
  int64_t c = 0;                  // 1 .. 2^31 - 1
  int from_logits = 0;
  float* rows_out = nullptr;      // optional [n]: the row values, 0 for uncounted rows
  // optional [2, kl_divergence_blocks(n)] scratch: per block the FP64 sum of its row values, then
  // its count of rows.  With it the finish launch adds the partials in block order and either
  // accumulates into *dst_sum and *dst_count (class states) or writes *out = sum (mean: / count)
  double* partial = nullptr;
  double* dst_sum = nullptr;
  double* dst_count = nullptr;
  float* out = nullptr;
  int mean = 0;
};
int kl_divergence_blocks(int64_t n);  // grid of the row launch = number of partial pairs
int launch_kl_divergence(const KlDivArgs& a, hipStream_t stream);
}  // namespace tea

namespace tea {
// K19: Kendall rank correlation per row (csrc/kernels/kendall.hip; docs/parity.md, "Not in the
// reference").  K3a sorts `target` (payload_kind 0), kendall_prepare turns the sorted rows into the
// tie-run starts `s` and the gathered `input`, K3a sorts that with `s` as its payload
// (payload_kind 2), and kendall_count counts ties and the strict inversions of the carried `s`.
constexpr int kKendallTile = 2048;  // positions a block resolves, sorts or merges in LDS
struct KendallPrepareArgs {
  const float* sorted = nullptr;   // [rows, n] target, sorted descending, contiguous
  const int32_t* order = nullptr;  // [rows, n] source index of each sorted position
  const float* x = nullptr;        // [rows, n] input in source order, contiguous
  int64_t rows = 0;
  int64_t n = 0;                   // 2 .. 2^31 - 1
  int32_t* s = nullptr;            // [rows, n] start of the target tie run of each sorted position
  float* xg = nullptr;             // [rows, n] x[order]
  int64_t* part = nullptr;         // [rows, 6, kendall_tiles(n)]: writes planes 1 (n2) and 5 (my)
  int32_t* flags = nullptr;        // [rows, 2]: writes [row][0] = target holds NaN | 2 * sort fault
  const uint32_t* sort_fault = nullptr;  // K3a's onesweep timeout word of the target sort, or null
};
struct KendallCountArgs {
  const float* sorted = nullptr;    // [rows, n] gathered input, sorted descending (stable), contiguous
  const int32_t* carried = nullptr; // [rows, n] the `s` that sort carried
  int64_t rows = 0;
  int64_t n = 0;
  int64_t* part = nullptr;          // [rows, 6, kendall_tiles(n)] partials of n1, n2, n3, Q, mx, my
  int32_t* flags = nullptr;         // [rows, 2]: writes [row][1] = input holds NaN
  int32_t* buf0 = nullptr;          // 2 x [rows, n] scratch: the merge levels' ping-pong rows
  int32_t* buf1 = nullptr;
  const uint32_t* sort_fault = nullptr;  // the timeout word of the input sort, or null
  int variant = 0;                  // 0: tau-b, 1: tau-c
  float* out = nullptr;             // [rows]
  int64_t* counts = nullptr;        // [rows, 6]: n1, n2, n3, Q, mx, my; -1 for a task without a value
};
int64_t kendall_tiles(int64_t n);
int launch_kendall_prepare(const KendallPrepareArgs& a, hipStream_t stream);
int launch_kendall_count(const KendallCountArgs& a, hipStream_t stream);
}  // namespace tea

namespace tea {
// K20: Kernel Inception Distance (csrc/kernels/kid.hip; docs/parity.md, "Not in the reference").
// kid_gram_kernel forms, per subset, the three sums of the polynomial kernel over XX, YY and XY
// straight from FP32-MFMA Gram tiles of index-gathered rows (no Gram matrix and no gathered copy
// ever exists); kid_finish_kernel adds the tile partials, forms mmd2 per subset and its mean and
// population standard deviation.
constexpr int kKidTile = 128;  // rows and columns of one Gram tile
struct KidGramArgs {
  const float* real = nullptr;     // [n_r, D], unit stride along D
  const float* fake = nullptr;     // [n_f, D]
  int64_t real_stride = 0;         // row strides in elements
  int64_t fake_stride = 0;
  int64_t n_r = 0;
  int64_t n_f = 0;
  int64_t d = 0;                   // >= 1
  const int32_t* idx_r = nullptr;  // [subsets, m] rows of `real`, contiguous; clamped to [0, n_r)
  const int32_t* idx_f = nullptr;  // [subsets, m] rows of `fake`
  int64_t subsets = 0;             // >= 1
  int64_t m = 0;                   // >= 2
  double gamma = 0.0;
  double coef = 0.0;
  int degree = 1;                  // 1 .. 16
  double* partials = nullptr;      // [subsets, kid_items(m)]
};
struct KidFinishArgs {
  const double* partials = nullptr;  // [subsets, kid_items(m)]
  int64_t subsets = 0;
  int64_t m = 0;
  double* sums = nullptr;            // [subsets, 3]: sxx, syy, sxy
  double* values = nullptr;          // [subsets]: mmd2
  float* out = nullptr;              // [2]: mean and population standard deviation of `values`
};
int64_t kid_items(int64_t m);  // tiles per subset: T (T + 1) / 2 of XX, as many of YY, T^2 of XY
int launch_kid_gram(const KidGramArgs& a, hipStream_t stream);
int launch_kid_finish(const KidFinishArgs& a, hipStream_t stream);
}  // namespace tea

namespace tea {
// K21: Inception Score (csrc/kernels/inception_score.hip; docs/parity.md, "Not in the reference").
// Row i of the [n, c] logits belongs to split (first + i) mod s.  inception_rows_kernel reads every
// row once and writes, per block, the FP64 column sums of the softmax probabilities of its rows,
// the sum of their negative entropies and their number; inception_finish_kernel adds the blocks'
// partials in block order into the three states; inception_value_kernel forms the splits' log
// scores and the mean and population standard deviation of their exponentials.
constexpr int kInceptionMaxColumns = 2048;  // a wave holds one row in registers, 32 values per lane
constexpr int kInceptionMaxSplits = 64;     // one lane per split in the value launch's last step
constexpr int kInceptionMaxBlocks = 1024;   // grid cap of the row launch: splits x blocks per split
constexpr int kInceptionWavesPerBlock = 4;
constexpr int kInceptionNarrowColumns = 256;  // rows this narrow or narrower ...
constexpr int kInceptionRowsPerWaveNarrow = 32;  // ... aim at this many rows per wave,
constexpr int kInceptionRowsPerWaveWide = 8;     // wider ones at this many
struct InceptionArgs {
  const void* logits = nullptr;  // [n, c], unit stride along c, rows element-aligned
  DType dt = DType::f32;         // f32 / bf16 / f16
  int64_t row_stride = 0;        // elements, >= 0
  int64_t n = 0;                 // 1 .. 2^31 - 1
  int c = 0;                     // 1 .. kInceptionMaxColumns
  int splits = 0;                // 1 .. kInceptionMaxSplits
  int first = 0;                 // 0 .. splits - 1: the split of row 0
  double* partial = nullptr;     // [splits * inception_blocks(n, splits, c), c + 2] scratch
  double* prob_sum = nullptr;    // [splits, c] +=
  double* neg_entropy_sum = nullptr;  // [splits] +=
  double* num_rows = nullptr;    // [splits] +=
};
// Blocks per split of the row launch.  A split has about n / splits rows, a block four waves; a wave
// should walk kInceptionRowsPerWave{Narrow, Wide} rows, so that the block's one [c + 2] partial
// (8 bytes per column, written here and read by the finish launch) stays small against the rows it
// stands for, until splits x blocks reaches kInceptionMaxBlocks; past that the waves take more rows.
int inception_blocks(int64_t n, int splits, int c);
int launch_inception_update(const InceptionArgs& a, hipStream_t stream);
// split_log[s] (NaN for a split without rows) and out[0 .. 2) = mean and population standard
// deviation of exp(split_log) over the splits with rows; 1 <= splits <= kInceptionMaxSplits, c >= 1
int launch_inception_value(const double* prob_sum, const double* neg_entropy_sum, const double* num_rows,
                           int splits, int64_t c, double* split_log, float* out, hipStream_t stream);
}  // namespace tea

namespace tea {
// K22: improved precision / recall and density / coverage (csrc/kernels/prdc.hip; docs/parity.md,
// "Not in the reference").  All four are k-nearest-neighbour statistics of the squared distances
// d2(a, b) = max(0, (|a|^2 + |b|^2) - 2 <a, b>) between two feature sets.  prdc_tile_kernel walks
// 128 x 128 FP32-MFMA tiles of <a, b> (K20's main loop) and keeps, per query row, either the k
// smallest d2 (Knn) or the count of d2 <= rad2[col] and the smallest d2 (Cross) over the column
// tiles of its block; no distance is ever written to memory.
constexpr int kPrdcTile = 128;         // rows and columns of one tile
constexpr int kPrdcMaxK = 8;           // neighbours kept per row
constexpr int kPrdcCUs = 256;          // compute units of the MI355X, which the group rule balances over
constexpr int kPrdcMaxGroups = 16;     // the rule's largest G: at most 32 lists per row
constexpr int kPrdcBlockStages = 12;   // a block's fixed cost in the rule, in 32-wide k-steps of one tile
constexpr int kPrdcHitsRows = 256;     // rows per block of prdc_hits_kernel
// Column groups G of a pass of n_query rows of width d over n_ref columns: block (p, g) owns the
// 128-row panel p and walks the column tiles g, g + G, ...  `groups` >= 1 is taken as given (clamped
// to the number of column tiles).  0 is the rule: the G in 1 .. min(column tiles, kPrdcMaxGroups)
// with the smallest modelled time of the busiest CU (the smallest such G on a tie),
//   c (t ceil(d / 32) + kPrdcBlockStages) (c == 1 ? 4 : 3),   c = ceil(panels G / kPrdcCUs),  t = ceil(tiles / G):
// a CU is handed c blocks of t tiles each, a block costs about 12 k-steps before its first tile, and
// a block alone on its CU walks a tile in 2/3 of the time two resident blocks share, not in 1/2.
// The model follows the measured times of profiles/prdc_r18.json to a few percent.  Every block
// writes two lists per row (one per 64-column half of its tiles): 2 G lists in all.
int64_t prdc_groups(int64_t n_query, int64_t n_ref, int64_t d, int64_t groups);
struct PrdcNormsArgs {
  const float* real = nullptr;  // [n_r, D], unit stride along D
  const float* fake = nullptr;  // [n_f, D]
  int64_t real_stride = 0;      // row strides in elements
  int64_t fake_stride = 0;
  int64_t n_r = 0;
  int64_t n_f = 0;
  int64_t d = 0;
  double* norms_real = nullptr;  // [n_r]: FP64 sums of squares
  double* norms_fake = nullptr;  // [n_f]
};
struct PrdcTileArgs {
  const float* query = nullptr;  // [n_q, D], unit stride along D
  const float* ref = nullptr;    // [n_ref, D] (Knn: the query set itself)
  int64_t query_stride = 0;
  int64_t ref_stride = 0;
  int64_t n_q = 0;
  int64_t n_ref = 0;
  int64_t d = 0;
  const double* norms_q = nullptr;    // [n_q]
  const double* norms_ref = nullptr;  // [n_ref]
  int groups = 0;                     // G >= 1 (prdc_groups)
  // Knn
  int k = 0;                   // 1 .. kPrdcMaxK
  double* partial = nullptr;   // [n_q, 2 G, k]: ascending, +inf in the slots never filled
  // Cross
  const double* radii_ref = nullptr;  // [n_ref]: squared radii of the reference rows
  uint32_t* counts = nullptr;         // [n_q, 2 G]
  double* mins = nullptr;             // [n_q, 2 G]: +inf where the list saw no column
};
struct PrdcFinishArgs {
  // cross partials of the pass fake -> real ([n_f, lists_f]) and real -> fake ([n_r, lists_r])
  const uint32_t* counts_fake = nullptr;
  const double* mins_fake = nullptr;
  const uint32_t* counts_real = nullptr;
  const double* mins_real = nullptr;
  const double* radii_real = nullptr;  // [n_r]
  int64_t n_r = 0;
  int64_t n_f = 0;
  int lists_r = 0;
  int lists_f = 0;
  int k = 0;
  int64_t* block_tallies = nullptr; // [prdc_hits_blocks(n_r, n_f), 4] scratch
  int32_t* hits_real = nullptr;     // [n_r]
  int32_t* hits_fake = nullptr;     // [n_f]
  double* nearest_real = nullptr;   // [n_r]
  double* nearest_fake = nullptr;   // [n_f]
  int64_t* tallies = nullptr;       // [4]: precise rows, recalled rows, total hits_fake, covered rows
  float* values = nullptr;          // [4]: precision, recall, density, coverage
};
int launch_prdc_norms(const PrdcNormsArgs& a, hipStream_t stream);
int launch_prdc_knn(const PrdcTileArgs& a, hipStream_t stream);
int launch_prdc_cross(const PrdcTileArgs& a, hipStream_t stream);
// radii[row] <- the k-th smallest of the row's `lists` ascending k-lists
int launch_prdc_radii(const double* partial, int64_t n, int lists, int k, double* radii, hipStream_t stream);
// blocks of prdc_hits_kernel: kPrdcHitsRows rows of the generated side each, then of the real side
int64_t prdc_hits_blocks(int64_t n_r, int64_t n_f);
int launch_prdc_finish(const PrdcFinishArgs& a, hipStream_t stream);  // two launches
}  // namespace tea

namespace tea {
// K23: silhouette coefficient (csrc/kernels/silhouette.hip; docs/parity.md, "Not in the reference").
// With d(i, j) the Euclidean distance, a(i) is the mean of d over the other members of i's cluster,
// b(i) the smallest mean of d over another non-empty cluster and s(i) = (b - a) / max(a, b).
// silhouette_tile_kernel walks 128 x 128 FP32-MFMA tiles of <x_r, x_i> (K22's main loop) whose rows
// are 128-row panels of one cluster each (the samples sorted by cluster, every cluster padded to
// whole panels) and whose columns are the query samples; a lane adds its columns' distances over
// the rows in FP64, so neither a distance nor a per-cluster table is ever written to memory.
constexpr int kSilTile = 128;          // rows of a panel, columns of a column tile
constexpr int kSilCUs = 256;           // compute units of the MI355X, which the group rule balances over
constexpr int kSilMaxGroups = 16;      // the rule's largest G
constexpr int kSilBlockStages = 12;    // a block's fixed cost in the rule, in 32-wide k-steps of one tile
constexpr int kSilEpilogueStages = 6;  // a tile's epilogue (128 FP64 square roots per lane), in k-steps
constexpr int kSilStitchRows = 256;    // samples per block of silhouette_stitch_kernel
// Panel groups G of a call with n samples of width d and at most max_panels panels: block (q, g)
// owns column tile q and walks the panels [g T / G, (g + 1) T / G) of the T <= max_panels panels the
// device counted.  `groups` >= 1 is taken as given (clamped to max_panels).  0 is the rule, K22's
// with the epilogue added to a tile: the G in 1 .. min(max_panels, kSilMaxGroups) with the smallest
//   c (t (ceil(d / 32) + kSilEpilogueStages) + kSilBlockStages) (c == 1 ? 4 : 3),
//   c = ceil(column tiles G / kSilCUs),  t = ceil(max_panels / G)
// (the smallest such G on a tie).  A model: nothing of it has been fitted to this kernel yet.
int64_t silhouette_groups(int64_t n, int64_t max_panels, int64_t d, int64_t groups);
int64_t silhouette_stitch_blocks(int64_t n);
struct SilhouetteArgs {
  const float* x = nullptr;              // [n, D], unit stride along D
  int64_t stride = 0;                    // row stride in elements
  int64_t n = 0;
  int64_t d = 0;
  double* norms = nullptr;               // [n]: FP64 sums of squares, NaN for a row with a NaN or inf
  const int32_t* labels = nullptr;       // [n]: cluster of a sample, -1 for a label outside [0, k)
  const int32_t* ref_index = nullptr;    // [max_panels * 128]: sample of a panel row, -1 for padding
  const int32_t* panel_cluster = nullptr;  // [max_panels]: cluster of a panel, -1 past the last
  const int32_t* counts = nullptr;       // [k]: members per cluster
  const int32_t* num_panels = nullptr;   // [1]: T, on the device
  int max_panels = 0;
  int k = 0;
  int groups = 0;                        // G >= 1 (silhouette_groups)
  double* edges = nullptr;               // [G, 4, n]: first sum, last sum, inside minimum, inside own sum
  double* a = nullptr;                   // [n]
  double* b = nullptr;                   // [n]
  double* s = nullptr;                   // [n]
  float* samples = nullptr;              // [n]
  double* block_sums = nullptr;          // [silhouette_stitch_blocks(n)] scratch
  double* score64 = nullptr;             // [1]
  float* score = nullptr;                // [1]
};
int launch_silhouette_norms(const SilhouetteArgs& a, hipStream_t stream);
int launch_silhouette_tile(const SilhouetteArgs& a, hipStream_t stream);
int launch_silhouette_finish(const SilhouetteArgs& a, hipStream_t stream);  // stitch and finish: two launches
}  // namespace tea

namespace tea {
// K24: COCO-style detection mean average precision (csrc/kernels/detection_map.hip; docs/parity.md,
// "Not in the reference").  map_match_kernel: a workgroup per image (persistent grid) stages the
// image's boxes in LDS, orders detections by (label, score descending, index) and ground truths by
// (label, index) with an LDS bitonic sort, and its waves share the class segments: per kept
// detection a wave forms the FP64 IoUs with the class's ground truths, 64 at a time, and per
// threshold takes the unmatched ground truth of the largest IoU (the later among equals).
// map_curve_kernel: a workgroup per (class, threshold) walks the class's hits from the right.
constexpr int kMapMaxBoxes = 1024;      // detections, and ground truths, of one image (LDS: about 46 KB)
constexpr int kMapBlock = 256;          // threads of a map_match workgroup
constexpr int kMapGrid = 768;           // its largest grid: three workgroups per compute unit
constexpr int kMapMaxThresholds = 16;   // bits of a ground truth's matched mask
constexpr int kMapMaxClasses = 4194303;  // labels take 22 bits of the keys; 2^22 - 1 is "no class"
constexpr int kMapCurveChunk = 256;     // positions of a map_curve step, one per thread
constexpr int kMapCurveGrid = 4096;     // its largest grid
// bits of the flag: a NaN score, a non-finite coordinate, x2 < x1 or y2 < y1, a label outside [0, C)
constexpr int kMapBadScore = 1, kMapBadCoordinate = 2, kMapBadBox = 4, kMapBadLabel = 8;
struct MapMatchArgs {
  const float* det_boxes = nullptr;    // [M, 4]
  const void* det_scores = nullptr;    // [M], f32 / f16 / bf16
  DType score_dt = DType::f32;
  const void* det_labels = nullptr;    // [M], i64 / i32
  DType det_label_dt = DType::i64;
  const float* gt_boxes = nullptr;     // [G, 4]
  const void* gt_labels = nullptr;     // [G], i64 / i32
  DType gt_label_dt = DType::i64;
  const int64_t* offsets = nullptr;    // [2, B + 1] on the device: first detection / ground truth of an image
  const double* thresholds = nullptr;  // [T]
  int num_images = 0;
  int num_thresholds = 0;
  int num_classes = 0;
  int max_detections = 0;
  float* scores = nullptr;             // [M]: every image's detections in the matching order
  int32_t* labels = nullptr;           // [M]: -1 for a dropped detection
  int32_t* hits = nullptr;             // [M]: bit k, matched under threshold k
  long long* gt_count = nullptr;       // [C]: += ground truths per class
  int32_t* matched_gt = nullptr;       // [M, T] or null: index within the image of the matched ground truth, -1
  int* err = nullptr;                  // or null: |= kMapBad* bits
};
int launch_map_match(const MapMatchArgs& a, hipStream_t stream);
struct MapCurveArgs {
  const int32_t* hits = nullptr;       // [N] in the global order (label, score descending, stored order)
  const int64_t* class_offsets = nullptr;  // [C + 1]
  const double* gt_count = nullptr;    // [C]
  int num_classes = 0;
  int num_thresholds = 0;
  int index_50 = -1;                   // rows of the thresholds 0.5 and 0.75, -1 when absent
  int index_75 = -1;
  double* ap = nullptr;                // [T, C], NaN for a class without ground truth
  double* rec = nullptr;               // [T, C]
  float* scalars = nullptr;            // [4]: map, map_50, map_75, mar
  float* map_per_class = nullptr;      // [C]
  float* mar_per_class = nullptr;      // [C]
};
int launch_map_curve(const MapCurveArgs& a, hipStream_t stream);  // two launches
}  // namespace tea

namespace tea {
// K25: pair-counting and information clustering indices of two labelings (csrc/kernels/contingency.hip;
// docs/parity.md, "Not in the reference").  All of them are functions of the rectangular int64
// contingency table n[i, j] = #{s : true[s] = i, pred[s] = j}.  contingency_count_kernel adds one
// batch of label pairs to it: the table is cut into slices of S consecutive cells held in LDS as u32,
// block (slice, group) walks its group's samples and counts the cells of its slice, and flushes the
// non-zero cells with 64-bit integer atomics.  Integer sums only: bit-identical from run to run.
constexpr int kCtgSliceSmall = 4096;    // cells of a small slice: 16 KiB of LDS, eight blocks of 256 threads per CU
constexpr int kCtgSliceLarge = 32768;   // cells of a large slice: 128 KiB of a CU's 160 KiB, one block of 1024 threads
constexpr int kCtgBlockSmall = 256;
constexpr int kCtgBlockLarge = 1024;
constexpr int kCtgUnit = 4;             // label pairs a thread takes per step (16-byte loads)
constexpr int kCtgMaxBlocks = 1024;     // slices * groups of the count launch
constexpr int kCtgMaxCells = 1 << 22;   // R * C of the native path
constexpr int kCtgStatsBlocks = 1024;   // largest grid of the cell pass; its FP64 partials
constexpr int kCtgMarginBlocks = 256;   // largest grid of the marginal pass
constexpr int kCtgEmiBlocks = 2048;     // largest grid of the EMI launch
constexpr int kCtgEmiMaxParts = 64;     // a pair's n-range is cut into at most this many wave-items
constexpr int kCtgInts = 6;             // pairs of cells, of rows, of columns; N; non-empty rows, columns
constexpr int kCtgValues = 21;          // length of the values vector (indices: ops/contingency.py)
constexpr int kCtgBadLabel = 1;         // bit of the flag: a label outside its range
struct ContingencyCountArgs {
  const void* labels_true = nullptr;   // [n], i64 / i32
  const void* labels_pred = nullptr;   // [n], i64 / i32
  DType true_dt = DType::i64;
  DType pred_dt = DType::i64;
  int64_t n = 0;                       // < 2^31
  int64_t r = 0;                       // rows: labels_true in [0, r)
  int64_t c = 0;                       // columns: labels_pred in [0, c)
  int slice = 0;                       // kCtgSliceSmall or kCtgSliceLarge
  int groups = 0;                      // sample groups; ceil(r c / slice) * groups <= kCtgMaxBlocks
  long long* table = nullptr;          // [r, c] += counts
  int* err = nullptr;                  // or null: |= kCtgBadLabel
};
int launch_contingency_count(const ContingencyCountArgs& a, hipStream_t stream);
// Blocks of the three statistics grids for an [r, c] table (lengths of the partial vectors)
int contingency_stats_blocks(int64_t r, int64_t c);
int contingency_margin_blocks(int64_t r, int64_t c);
int contingency_emi_blocks(int64_t r, int64_t c);
int contingency_emi_parts(int64_t r, int64_t c);
struct ContingencyStatsArgs {
  const long long* table = nullptr;    // [r, c], every cell >= 0 and the total < 2^32
  int64_t r = 0;
  int64_t c = 0;
  long long* marginals = nullptr;      // [r + c], zero on entry: row sums, then column sums
  unsigned long long* ints = nullptr;  // [kCtgInts], zero on entry
  double* cell_partials = nullptr;     // [contingency_stats_blocks]: sums of n log n over the cells
  double* margin_partials = nullptr;   // [2, contingency_margin_blocks]: sums of a log a, of b log b
  double* margin_logs = nullptr;       // [2, r + c]: log x, then lgamma(x + 1) + lgamma(N - x + 1) (EMI's tables)
};
int launch_contingency_stats(const ContingencyStatsArgs& a, hipStream_t stream);  // two launches
struct ContingencyEmiArgs {
  const long long* marginals = nullptr;         // of launch_contingency_stats
  const unsigned long long* ints = nullptr;
  const double* margin_logs = nullptr;
  int64_t r = 0;
  int64_t c = 0;
  double* partials = nullptr;                   // [2, contingency_emi_blocks]: sums of the terms, of their magnitudes
};
int launch_contingency_emi(const ContingencyEmiArgs& a, hipStream_t stream);
struct ContingencyValuesArgs {
  const unsigned long long* ints = nullptr;
  const double* cell_partials = nullptr;
  const double* margin_partials = nullptr;
  const double* emi_partials = nullptr;         // or null: EMI and AMI come out NaN
  int stats_blocks = 0;
  int margin_blocks = 0;
  int emi_blocks = 0;
  double* values = nullptr;                     // [kCtgValues]
};
int launch_contingency_values(const ContingencyValuesArgs& a, hipStream_t stream);
}  // namespace tea
