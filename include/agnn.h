/*
 * agnn.h — C-ABI of libagnn_hip.so: the MI355X (gfx950) kernels behind the AnalysisGNN
 * heterogeneous message-passing hot path.
 *
 * The reference (manoskary/analysisgnn) is 100 % Python and has no FFI of its own; its hot path
 * bottoms out in three third-party operator families.  Each entry point below replaces one of
 * them, and the Python host side (analysisgnn_amd/_lib.py, ctypes) is the only caller:
 *
 *   agnn_csr_build        the per-relation `edge_index[:, edge_type == r]` compaction and the
 *                         COO bookkeeping that torch_scatter / PyG redo on every call
 *                         (ref: analysisgnn/models/core/hgnn.py:137-139, :481-483)
 *   agnn_csr_rowend       PyG `trim_to_layer` edge narrowing (ref: models/cadence.py:167-173)
 *   agnn_spmm_f32         `h[edge_index[1]]` gather + `torch_scatter.scatter(..., reduce=sum|mean,
 *                         out=...)` (ref: core/gnn.py:70-74, :511, :539; core/hgnn.py:406-407;
 *                         models/analysis.py:580-586) and PyG `SAGEConv` mean aggregation under
 *                         `HeteroConv` (ref: models/cadence.py:147-159,174)
 *   agnn_gru_fwd/bwd_f32  `torch.nn.GRU` of the hybrid sequence branch (ref: models/cadence.py:249-285)
 *   agnn_lstm_seq_*       `torch.nn.LSTM` over long sequences (ref: models/pitch_spelling.py:50-151; models/chord.py:751-783)
 *   agnn_gated_*          `ResGatedGraphConv` edge gate + scatter (ref: core/gnn.py:246-257)
 *   agnn_absdiff_*        `RelEdgeConv` per-row sums of h_j and |h_i - h_j| (ref: core/gnn.py:99-105)
 *   agnn_norm_act_*       LayerNorm / ReLU / Dropout chains between the projections (ref: models/analysis.py:429-443)
 *   agnn_wgrad_f32        weight/bias gradients of the dense projections (fp32 MFMA, split over N)
 *   agnn_pack_f32         per-relation parameter cat / sum / gradient fan-out of the fused HeteroConv (ref: models/cadence.py:147-159)
 *   agnn_embed_cat_*      note-input assembly `cat([x, pitch_embedding(ps), key_embedding(ks)])` and the tables' gradient
 *                         (ref: models/analysis.py:399-400, :574)
 *   agnn_gproj_*          the task heads' last Linear layers as one grouped projection (ref: models/analysis.py:486-496)
 *   agnn_adamw_f32        gradient clipping + `torch.optim.AdamW` step on the flat buffers (ref: models/analysis.py:1380-1381)
 *   agnn_adamw_sched_f32  the same step under the reference's per-step LR schedulers and SWA, the rate a closed form of the
 *                         device step counter (ref: models/analysis.py:104-275, :1380-1410; train/train_analysisgnn.py:243-245)
 *   agnn_multitask_ce_f32 the 21 per-task CrossEntropyLoss terms (ref: models/analysis.py:881-888)
 *   agnn_multitask_kd_f32 the per-task distillation terms against the frozen memory model (ref: models/analysis.py:1041-1062)
 *   agnn_ewc_f32          the EWC penalty and the Fisher accumulation over the flat buffers (ref: models/analysis.py:1440-1495)
 *   agnn_multitask_eval_f32 the per-task torchmetrics Accuracy / macro F1Score and the gated / joint Roman-numeral accuracies of
 *                         the validation and test steps, as integer counters (ref: models/analysis.py:1143-1164, :1221-1282)
 *   agnn_sample_hops      graphmuse `MuseNeighborLoader` batch assembly (ref: data/datamodules/analysis.py:270-293)
 *   agnn_relt_*           PyG `HGTConv` per-head relation transforms (k_rel / v_rel)
 *   agnn_hgt_attn_*       PyG `HGTConv` message/softmax/aggregate, reached through graphmuse
 *                         `HybridHGT` (ref: models/analysis.py:445-453)
 *   agnn_taskattn_*       `CrossTaskTransformer`: attention over the task tokens of every note (ref: models/analysis.py:408-418)
 *   agnn_link_bce_*       the staff / voice link prediction of the pretraining stage: endpoint gathers, dot product,
 *                         BCEWithLogitsLoss, pair membership and the index_add_ backward (ref: models/analysis.py:397-401, :704-731)
 *   agnn_edge_*           `EdgeDecoder` and the edge-consistency term of the continual trainer: pair features with in-kernel
 *                         dropout, edge labels, the two-class cross entropy (ref: models/analysis.py:805-836, :986-1019)
 *   agnn_colnorm_*        `activation -> BatchNorm1d -> Dropout` over the row axis (ref: models/chord.py:569-570, core/mlp.py:27-35)
 *   agnn_onset_pool_*     `OnsetEdgePoolingVersion2`: scatter-mean over onset neighbours and self, selected rows only
 *                         (ref: models/chord.py:284-287)
 *   agnn_graphnorm_*      PyG `GraphNorm`: per-graph, per-column normalisation with a learnable mean scale (ref:
 *                         models/pitch_spelling.py:158, :222)
 *
 * Conventions (all entry points)
 *   - plain pointers and sizes only; every `const T*`/`T*` marked (device) is device memory owned
 *     by the caller (PyTorch's caching allocator); arrays marked (host) are read during the call.
 *   - this file is READ by the Python binding (analysisgnn_amd/_abi.py), which accepts the forms used here and nothing else.  A
 *     comment that begins with (host) behind a parameter is part of the contract: it makes a scalar or pointer array a typed host
 *     array there (POINTER(int32) ...); every other non-struct pointer is an address (c_void_p).
 *   - all work is enqueued on `stream`; no implicit synchronisation, no default-stream use, no
 *     allocation, no global mutable state: safe to call from several host threads and under
 *     hipGraph capture.
 *   - return 0 on success, a negative errno-style code otherwise (AGNN_E*); the message is
 *     available from agnn_last_error() (thread-local).  Nothing is printed, nothing throws.
 *   - feature matrices are fp32, row-major, rows 16-byte aligned, H % 4 == 0.
 *   - index arrays produced by the library are int32; COO inputs are int64 as PyTorch holds them.
 *   - sums run in a fixed order (CSR order = original edge order inside a row): results are
 *     bitwise reproducible; no float atomics anywhere.
 */
#ifndef AGNN_H_
#define AGNN_H_

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef void* agnn_stream_t; /* hipStream_t */

#define AGNN_OK        0
#define AGNN_EINVAL  (-22) /* bad shape / size / flag combination */
#define AGNN_EALIGN  (-14) /* misaligned pointer or leading dimension */
#define AGNN_ENOMEM  (-12) /* workspace too small */
#define AGNN_ERUNTIME (-5) /* HIP runtime error */

#define AGNN_MAX_SEG 32    /* segments (relations x directions) per call */

const char* agnn_last_error(void);
/* library / ABI version: (major << 16) | minor */
int agnn_version(void);

/* ------------------------------------------------------------------------------------------
 * CSR construction.  A "segment" is one relation in one direction: edges (row_e, col_e),
 * e < n_edges, grouped by row.  If `etype` is non-NULL only edges with etype[e] == etype_code
 * take part (the in-tree layers' `edge_type == code` mask, hgnn.py:138).
 * Output (device):
 *   rowstart [total_rows + 1]  with total_rows = sum_s n_rows[s];  segment s owns the slice
 *            rowstart + rowbase[s] (n_rows[s] + 1 entries, rowbase = exclusive prefix of n_rows);
 *            entries are offsets into col/perm shared by all segments.
 *   col      [E_total]  column (gathered row) id of every kept edge, grouped by row,
 *   perm     [E_total]  original edge position e inside its segment's COO arrays.
 * Inside a row, edges keep their original order (stable) so perm is increasing there.
 * E_total = sum_s n_edges[s] is the capacity; slots past the number of kept edges are undefined.
 * ------------------------------------------------------------------------------------------ */
typedef struct {
  const int64_t* row;    /* (device) [n_edges] */
  const int64_t* col;    /* (device) [n_edges] */
  const int64_t* etype;  /* (device) [n_edges] or NULL */
  int64_t etype_code;
  int64_t n_edges;
  int64_t n_rows;
} agnn_coo_seg_t;

size_t agnn_csr_workspace_bytes(int64_t e_total, int64_t total_rows);

/* `status` (device int32[1], may be NULL; caller-owned, zero-initialised once, never reset by the library): incremented
 * for every edge whose position falls outside its row — impossible when the build's own counters are intact, so a non-zero
 * word means the workspace was disturbed while the build ran (round 1: a memset node of a captured graph that had not
 * cleared the counters).  Nothing is written out of range in that case; the index is incomplete and agnn_check_status
 * reports it. */
int agnn_csr_build(int n_seg, const agnn_coo_seg_t* segs /* (host) */,
                   int32_t* rowstart, int32_t* col, int32_t* perm,
                   void* workspace, size_t workspace_bytes, int32_t* status, agnn_stream_t stream);

/* Synchronises `stream`, reads the status word and returns AGNN_ERUNTIME (with a message) when it is non-zero.  The only
 * entry point that waits for the device: meant for tests, the end of a benchmark, or once per epoch. */
int agnn_check_status(const int32_t* status, agnn_stream_t stream);

/* rowend[i] = first position p in [rowptr[i], rowptr[i+1]) with perm[p] >= e_limit (or
 * rowptr[i+1]): the row's edges restricted to the COO prefix [0, e_limit) — PyG trim_to_layer. */
int agnn_csr_rowend(const int32_t* rowptr, const int32_t* perm, int64_t n_rows, int64_t e_limit,
                    int32_t* rowend, agnn_stream_t stream);

/* The same for up to AGNN_ROWEND_MAX_ITEMS (CSR, limit) pairs in ONE launch: a sampled batch needs the row ends of
 * every relation, in both directions, for every trimmed layer (reference models/cadence.py:165-173 trims per layer;
 * R = 4, L = 3: 16 items). */
#define AGNN_ROWEND_MAX_ITEMS 64
typedef struct {
  const int32_t* rowptr;   /* (device) [n_rows + 1] */
  const int32_t* perm;     /* (device) shared with rowptr's offsets */
  int32_t* rowend;         /* (device) [n_rows] out */
  int32_t n_rows;
  int32_t e_limit;
} agnn_rowend_item_t;
int agnn_csr_rowend_batch(int n_items, const agnn_rowend_item_t* items /* (host) */, agnn_stream_t stream);

/* ------------------------------------------------------------------------------------------
 * Multi-relation segmented gather-reduce ("hetero SpMM").  For every output row i < n_rows and
 * relation r < n_rel:
 *     acc_r(i) = sum_{p in [rowptr_r[i], end_r(i))}  w_r(p) * src_r[ col_r[p], 0:H ]
 *     w_r(p)   = (ew_r ? ew_r[p] : 1) * (colscale_r ? colscale_r[col_r[p]] : 1) * valid(p)
 *     valid(p) = !(SKIP_SELF && col==i) && col < col_limit
 *     cnt_r(i) = number of valid p
 *     val_r(i) = (acc_r(i) + (self ? self[i] : 0)) * (MEAN ? 1 / max(cnt_r(i), 1) : 1)
 * and out[i*ld_out + r*rel_stride + 0:H] (=|+=) val_r(i); with rel_stride == 0 all relations
 * add into the same slot (first one obeys `accumulate`).  `self` reproduces torch_scatter's
 * `out=x.clone()` numerator.  inv_cnt (optional, [n_rel, n_rows]) receives
 * 1/max(cnt,1) for the backward pass.
 * ------------------------------------------------------------------------------------------ */
typedef struct {
  const float* src;        /* (device) [n_src, ld_src] */
  const int32_t* rowptr;   /* (device) [n_rows + 1] */
  const int32_t* rowend;   /* (device) [n_rows] or NULL */
  const int32_t* col;      /* (device) base shared with rowptr's offsets */
  const float* ew;         /* (device) per-position weights or NULL */
  const float* colscale;   /* (device) [n_src] or NULL */
  int64_t ld_src;
} agnn_rel_t;

#define AGNN_SPMM_MEAN      1u
#define AGNN_SPMM_SKIP_SELF 2u
#define AGNN_SPMM_ACCUM     4u
#define AGNN_SPMM_ROOT      8u  /* set by agnn_spmm_root_f32 (internal) */
#define AGNN_SPMM_GENERIC 1024u /* never take the specialised fast path (tests / A/B timing) */

int agnn_spmm_f32(int n_rel, const agnn_rel_t* rels /* (host) */, int64_t n_rows, int32_t H,
                  float* out, int64_t ld_out, int64_t rel_stride,
                  const float* self, int64_t ld_self,
                  float* inv_cnt, int32_t col_limit, uint32_t flags, agnn_stream_t stream);

/* The same aggregation with the ROOT operand of a SAGE layer riding along, so that PyG `SAGEConv`'s
 * `lin_l(mean_j x_j) + lin_r(x_i)` summed over the relations of a destination type (ref: models/cadence.py:147-159,174) is ONE
 * GEMM over [A_1 .. A_R | x_dst] and its backward ONE transposed launch (no slice gradient, no gradient add):
 *   rel_stride != 0 (forward):  out[i, r*rel_stride + 0:H] as agnn_spmm_f32, and out[i, n_rel*rel_stride + 0:H] = root[i]
 *                               (root_rows >= n_rows, ld_out >= n_rel*rel_stride + H);
 *   rel_stride == 0 (backward): out[i] = sum_r (...)  +  (i < root_rows ? root[i] : 0).
 * H must be 256 or 512, no per-edge weights; flags: AGNN_SPMM_MEAN, AGNN_SPMM_SKIP_SELF. */
int agnn_spmm_root_f32(int n_rel, const agnn_rel_t* rels /* (host) */, int64_t n_rows, int32_t H,
                       float* out, int64_t ld_out, int64_t rel_stride,
                       const float* root, int64_t ld_root, int64_t root_rows,
                       float* inv_cnt, int32_t col_limit, uint32_t flags, agnn_stream_t stream);

/* Gradient of agnn_spmm_f32 w.r.t. its `self` operand, optionally added onto an existing gradient:
 *     out[i, 0:H] (=|+=) sum_{r < n_rel} dout[i*ld_dout + r*rel_stride + 0:H] * (inv_cnt ? inv_cnt[r*ld_inv + i] : 1)
 * (rel_stride == 0: every relation read the same slot).  One launch instead of the reduce / multiply / add chain; with
 * `accumulate` it lands on the neighbour gradient the backward SpMM has just written when `self` and the source are the
 * same matrix (onset pooling, ref: models/analysis.py:580-587). */
int agnn_spmm_self_grad_f32(const float* dout, int64_t ld_dout, int64_t rel_stride, int32_t n_rel, const float* inv_cnt,
                            int64_t ld_inv, int64_t n_rows, int32_t H, float* out, int64_t ld_out, int32_t accumulate,
                            agnn_stream_t stream);

/* The join block between the encoder and the wrapper's project_enc (ref: models/analysis.py:580-587 followed by project_enc[0] =
 * LayerNorm(2H)): the onset pooling writes its own concatenation and normalises it, one wave per row, one launch.  For i < n:
 *     pooled_i = i < pool_rows ? (x_i + sum_{valid p in row i} x[col[p]]) / max(cnt_i, 1) : x_i
 *                (valid(p) = col != i && col < col_limit; exactly agnn_spmm_f32's MEAN | SKIP_SELF result with self = x, shared slot)
 *     u_i      = [x_i | pooled_i]                     -> u [n, 2H]   (what the LayerNorm's backward reads)
 *     y_i      = LayerNorm_eps(u_i) * gamma + beta    -> y [n, 2H],  mean [n], rstd [n]  (as agnn_norm_act_fwd_f32, no flags)
 *     inv_cnt[i] = 1 / max(cnt_i, 1)                  (optional; 1 for i >= pool_rows)
 * `rel`: rowptr / col (/ rowend) of the by-destination index with at least pool_rows rows; its src, ld_src, ew, colscale are
 * ignored (ew must be NULL).  H = 256 or 512; 1 <= pool_rows <= n. */
int agnn_pool_cat_norm_f32(const agnn_rel_t* rel /* (host) */, const float* x, int64_t ld_x, int64_t n, int64_t pool_rows, int32_t H,
                           int32_t col_limit, const float* gamma, const float* beta, float eps, float* u, int64_t ld_u,
                           float* y, int64_t ld_y, float* mean, float* rstd, float* inv_cnt, agnn_stream_t stream);
/* Its backward behind the LayerNorm's (du [n, 2H] from agnn_norm_act_bwd_f32), one launch:
 *     dx_i = du[i, 0:H] + inv_cnt[i] * du[i, H:2H] + sum_{valid p in row i of rel_t} inv_cnt[col[p]] * du[col[p], H:2H]
 * `rel_t`: the transposed (by-source) index, at least pool_rows rows; valid(p) = col != i && col < pool_rows; rows at or beyond
 * pool_rows have no neighbour term. */
int agnn_pool_cat_bwd_f32(const agnn_rel_t* rel_t /* (host) */, const float* du, int64_t ld_du, const float* inv_cnt, int64_t n,
                          int64_t pool_rows, int32_t H, float* dx, int64_t ld_dx, agnn_stream_t stream);

/* The join of the cadence models (ref: models/cadence.py:204-205 and :324-330, `LayerNorm(scatter_mean(x[src], dst, out=x.clone()))`),
 * csrc/pooljoin.hip: one wave per row, one launch.  For i < n:
 *     u_i = i < pool_rows ? (x_i + sum_{valid p in row i} x[col[p]]) / max(cnt_i, 1) : x_i          -> u [n, H]
 *           (valid(p) = 0 <= col < min(col_limit, n) && !(SKIP_SELF && col == i); neighbours summed in CSR order)
 *     y_i = LayerNorm_eps(u_i) * gamma + beta                                                         -> y [n, H], mean [n], rstd [n]
 *           (statistics centred twice: exact to fp32 rounding of the deviations also where the row's level dwarfs its spread)
 *     inv_cnt[i] = 1 / max(cnt_i, 1)                                                                  (1 for i >= pool_rows)
 * (u, mean, rstd) are what agnn_norm_act_bwd_f32 (seg = H, no flags) takes as (x, mean, rstd).
 * `rel`: rowptr / col (/ rowend) of the by-destination index with at least pool_rows rows; its src, ld_src and colscale are
 * ignored, ew must be NULL.  H any multiple of 4 in [4, 1024]; 1 <= pool_rows <= n; n == 0: nothing is done.  flags: AGNN_SPMM_SKIP_SELF
 * or 0.  u and y must not be x. */
int agnn_pool_norm_f32(const agnn_rel_t* rel /* (host) */, const float* x, int64_t ld_x, int64_t n, int64_t pool_rows, int32_t H,
                       int32_t col_limit, uint32_t flags, const float* gamma, const float* beta, float eps, float* u, int64_t ld_u,
                       float* y, int64_t ld_y, float* mean, float* rstd, float* inv_cnt, agnn_stream_t stream);
/* The pooling's backward behind the LayerNorm's (du [n, H] from agnn_norm_act_bwd_f32), one launch:
 *     dx_i = (i < pool_rows ? inv_cnt[i] : 1) * du_i + sum_{valid p in row i of rel_t} inv_cnt[col[p]] * du[col[p]]
 * `rel_t`: the transposed (by-source) index with at least min(col_limit, n) rows; valid(p) = 0 <= col < pool_rows &&
 * !(SKIP_SELF && col == i); rows at or beyond min(col_limit, n) were nobody's neighbour and take their own term only.  Same
 * col_limit and flags as the forward call.  dx must not be du. */
int agnn_pool_bwd_f32(const agnn_rel_t* rel_t /* (host) */, const float* du, int64_t ld_du, const float* inv_cnt, int64_t n,
                      int64_t pool_rows, int32_t H, int32_t col_limit, uint32_t flags, float* dx, int64_t ld_dx, agnn_stream_t stream);

/* Class-balanced cross entropy, the loss of the cadence models' validation steps (ref: models/cadence.py:425-434 and :535-544,
 * `weight = 1 / (bincount(y) + 1e-6); F.cross_entropy(logits, y, weight=weight)`), csrc/balce.hip:
 *     count_c = #{r : y_r == c},      w_c = 1 / (count_c + eps_w)
 *     loss    = sum_r w_{y_r} (logsumexp(z_r) - z_r[y_r]) / sum_r w_{y_r}
 *     dlogits[r, c] = w_{y_r} (softmax(z_r)[c] - [c == y_r]) / sum_r w_{y_r}        (optional, may be NULL)
 * logits [n_rows, n_classes] with leading dimension ld (any alignment: rows are read float by float); labels int64 [n_rows]; a
 * row whose label equals ignore_index is left out of the counts, both sums and gets a zero row of dlogits.  eps_w > 0 (the
 * reference's 1e-6).  Outputs: class_count int64 [n_classes] and weight float [n_classes] (either may be NULL), loss (device
 * scalar), dlogits [n_rows, >= n_classes] with leading dimension ld_d.  Three launches: a count pass, a row pass, a fixed-order
 * sum of one partial per 256 rows.  A thread owns a row in the row pass (strided reads, a serial loop over the classes): the kernel is
 * meant for the few classes of a cadence head, not for a wide one.  No float atomics: two runs give the same bits.
 * If no row is valid the loss is 0 and dlogits is 0 — this library's rule for an empty task (agnn_train_loss_f32); torch
 * returns NaN there.  A label outside [0, n_classes) that is not ignore_index contributes nothing, gets a zero row of dlogits
 * and adds 1 to *status (device int32, may be NULL; torch: device assert).  The reference only evaluates this loss; the gradient
 * is one more store in the row pass and makes the function usable as a training loss.
 * `workspace`: agnn_balanced_ce_workspace_bytes(n_rows) bytes, 4-byte aligned, need not be cleared.
 * AGNN_EINVAL: n_classes outside [1, AGNN_BCE_MAX_CLASSES], n_rows < 0, eps_w <= 0, loss or workspace NULL, logits or labels
 * NULL with n_rows > 0, ld or ld_d < n_classes; AGNN_ENOMEM: workspace too small.  n_rows == 0 writes loss = 0. */
#define AGNN_BCE_MAX_CLASSES 256
size_t agnn_balanced_ce_workspace_bytes(int64_t n_rows);
int agnn_balanced_ce_f32(const float* logits, int64_t ld, int64_t n_rows, int32_t n_classes, const int64_t* labels,
                         int64_t ignore_index, float eps_w, int64_t* class_count, float* weight, float* loss, float* dlogits,
                         int64_t ld_d, int32_t* status, void* workspace, size_t workspace_bytes, agnn_stream_t stream);

/* ------------------------------------------------------------------------------------------
 * Persistent bidirectional GRU layer (one launch for all T steps), replacing `torch.nn.GRU` in the
 * hybrid branch (ref: models/cadence.py:249-285, models/analysis.py:527-537).  hidden must be 128
 * (the H = 256 configuration); other sizes return AGNN_EINVAL and the host falls back to the
 * library RNN.  Gate order r, z, n and equations are torch's.
 *   gi    [B, T, 2, 3*hidden]   x W_ih^T + b_ih for both directions (library GEMM, done by the caller)
 *   w_hh  [2, 3*hidden, hidden], b_hh [2, 3*hidden]
 *   y     [B, T, 2*hidden]      forward | reverse halves, as nn.GRU(batch_first) returns
 *   saved [B, T, 2, 4, hidden]  r, z, n, W_hn h + b_hn  (kept for the backward pass)
 * Backward: given dy emits dgi [B, T, 2, 3*hidden] (gradient w.r.t. gi) and dgh [B, T, 2, 3*hidden]
 * (gradient w.r.t. W_hh h + b_hh: the r and z blocks equal dgi's, the n block is d n_pre * r);
 * weight/input gradients are GEMMs over those.
 * ------------------------------------------------------------------------------------------ */
int agnn_gru_fwd_f32(const float* gi, const float* w_hh, const float* b_hh, int64_t B, int64_t T,
                     int32_t hidden, float* y, float* saved, const float* drop_scale, float* y_drop,
                     agnn_stream_t stream);
int agnn_gru_bwd_f32(const float* dy, const float* y, const float* saved, const float* w_hh,
                     int64_t B, int64_t T, int32_t hidden, float* dgi, float* dgh, const float* drop_scale, float* hprev,
                     agnn_stream_t stream);
/* hprev (optional) [B, T, 2, hidden]: the backward walk reads h_{t-1} anyway and leaves it here — the right operand of the
 * W_hh weight-gradient product (the same matrix agnn_gru_hprev_f32 builds in a pass of its own). */
/* Inter-layer dropout of `nn.GRU(dropout=p)` (ref: models/cadence.py:249-251) rides along: drop_scale [B, T, 2*hidden]
 * holds 0 or 1 / (1 - p) per element; forward additionally writes y_drop = y * drop_scale (the next layer's input),
 * backward takes dy = d(y_drop) and applies the same factor.  Both NULL: no dropout. */
/* hp [B, T, 2, hidden]: the previous hidden state of each direction (forward: y[b, t-1, :hidden], reverse:
 * y[b, t+1, hidden:], zero at the sequence ends) — the operand of the W_hh weight-gradient GEMMs, in one launch. */
int agnn_gru_hprev_f32(const float* y, int64_t B, int64_t T, int32_t hidden, float* hp, agnn_stream_t stream);

/* ------------------------------------------------------------------------------------------
 * Persistent bidirectional LSTM layer over long sequences (csrc/lstmseq.hip) = one layer of
 * `torch.nn.LSTM(batch_first=True, bidirectional=True)`, zero initial state, gate order i, f, g, o
 * (ref: models/pitch_spelling.py:50-151 with cell_type="LSTM"; models/chord.py:751-783).
 * hidden (per direction) is 64 or 128.  B >= 1 and T >= 1: empty work is the caller's to skip.
 *   gi    [B, T, 2, 4*hidden]   x W_ih^T + b_ih for both directions (computed by the caller)
 *   w_hh  [2, 4*hidden, hidden], b_hh [2, 4*hidden]
 *   y     [B, T, 2*hidden]      forward | reverse halves, as nn.LSTM(batch_first) returns
 *   saved [B, T, 2, 5, hidden]  i, f, g, o after their non-linearities, and c_t  (kept for the backward pass)
 * Backward: given dy emits ONE dg [B, T, 2, 4*hidden], the gradient of the pre-activations: an LSTM adds its input-side and
 * hidden-side terms before the non-linearity, so dg is the gradient w.r.t. gi and w.r.t. W_hh h + b_hh alike (db_ih == db_hh).
 * hprev (optional) [B, T, 2, hidden]: h_{t-1} of each direction (zero at the chain's first step), copied from y by the walk —
 * the right operand of the W_hh weight-gradient product; y may be NULL without it.
 * Inter-layer dropout of `nn.LSTM(dropout=p)` rides along as in the GRU pair: drop_scale [B, T, 2*hidden] holds 0 or
 * 1 / (1 - p) per element; forward additionally writes y_drop = y * drop_scale (the next layer's input), backward takes
 * dy = d(y_drop) and applies the same factor.  Both NULL: no dropout.
 * ------------------------------------------------------------------------------------------ */
int agnn_lstm_seq_fwd_f32(const float* gi, const float* w_hh, const float* b_hh, int64_t B, int64_t T,
                          int32_t hidden, float* y, float* saved, const float* drop_scale, float* y_drop,
                          agnn_stream_t stream);
int agnn_lstm_seq_bwd_f32(const float* dy, const float* y, const float* saved, const float* w_hh,
                          int64_t B, int64_t T, int32_t hidden, float* dg, const float* drop_scale, float* hprev,
                          agnn_stream_t stream);

/* ------------------------------------------------------------------------------------------
 * HGT edge-softmax attention = message / softmax / aggregate of PyG `HGTConv`, reached through
 * graphmuse `HybridHGT` (ref: models/analysis.py:445-453; semantics SURVEY.md App. A.4).
 * For destination row i, head h (D = H / heads floats per head), over ALL incoming edges e of all
 * n_rel relations:   s_e = <q_i,h, k_r[col_e],h> * pscale_r[h]      (pscale = p_rel / sqrt(D))
 *                    a_e = exp(s_e - max) / (sum exp(s_e - max) + 1e-16),   out_i,h = sum_e a_e v_r[col_e],h
 * k_r / v_r are the relation-transformed keys / values of the source type (computed by the caller).
 * m_out / linv_out [n_rows, heads] keep the row max and 1/(sum + 1e-16) for the backward pass.
 * D must be 4*2^k, <= 256.
 * Backward, pass by destination: dq plus per-edge alpha, gs = ds*pscale, tdot = ds*<q,k> written at the
 * edge's COO position perm[p] into [n_edges, heads] arrays of its relation.
 * Backward, pass by source (one relation, transposed CSR, col = destination row, rows >= col_limit
 * skipped): dv[j] = sum_e alpha_e dm[col_e], dk[j] = sum_e gs_e q[col_e].
 * ------------------------------------------------------------------------------------------ */
typedef struct {
  const float* k;          /* (device) [n_src, ld] */
  const float* v;          /* (device) [n_src, ld] */
  const int32_t* rowptr;   /* (device) [n_rows + 1] */
  const int32_t* rowend;   /* (device) [n_rows] or NULL */
  const int32_t* col;      /* (device) */
  const int32_t* perm;     /* (device) COO position of every CSR position (backward only) */
  const float* pscale;     /* (device) [heads] */
  int64_t ld;
  float* alpha;            /* (device) [n_edges, heads]  backward outputs */
  float* gs;               /* (device) [n_edges, heads] */
  float* tdot;             /* (device) [n_edges, heads], or head-major [heads, ld_tdot] when ld_tdot > 0 */
  int64_t ld_tdot;         /* 0: edge-major tdot; > 0: tdot[h * ld_tdot + e] (a contiguous sum over the edges per head) */
} agnn_hgt_rel_t;

int agnn_hgt_attn_fwd_f32(int n_rel, const agnn_hgt_rel_t* rels /* (host) */, const float* q, int64_t ld_q,
                          int64_t n_rows, int32_t H, int32_t heads, float* out, int64_t ld_out,
                          float* m_out, float* linv_out, agnn_stream_t stream);
/* The attention of several DESTINATION types in one launch (an HGT layer has one per destination type; ref. as above): item i =
 * one agnn_hgt_attn_fwd_f32 call.  Items and their relation tables are read on the host during the call; at most
 * AGNN_HGT_MAX_DST items, AGNN_MAX_SEG relations in all. */
#define AGNN_HGT_MAX_DST 4
typedef struct {
  const agnn_hgt_rel_t* rels;   /* (host) n_rel relations ending in this destination type */
  int32_t n_rel;
  const float* q;
  int64_t ld_q;
  int64_t n_rows;
  float* out;
  int64_t ld_out;
  float* m_out;
  float* linv_out;
} agnn_hgt_dst_item_t;
int agnn_hgt_attn_fwd_multi_f32(int32_t n_items, const agnn_hgt_dst_item_t* items /* (host) */, int32_t H, int32_t heads,
                                agnn_stream_t stream);
int agnn_hgt_attn_bwd_dst_f32(int n_rel, const agnn_hgt_rel_t* rels /* (host) */, const float* q, int64_t ld_q,
                              const float* dm, int64_t ld_dm, const float* out, int64_t ld_out,
                              const float* m_in, const float* linv_in, int64_t n_rows, int32_t H,
                              int32_t heads, float* dq, int64_t ld_dq, agnn_stream_t stream);
/* Backward, pass by source, for up to AGNN_MAX_SEG relations in one launch (item i = one relation) — all relations ending in one
 * destination type share q and dm; item i writes its own dk / dv (a column block of its source type's gradient).  Items are read
 * on the host during the call. */
typedef struct {
  const int32_t* rowptr;
  const int32_t* rowend;      /* NULL: rowptr + 1 */
  const int32_t* col;
  const int32_t* perm;
  const float* alpha;
  const float* gs;
  float* dk;
  float* dv;
  int64_t ld_o;
  int32_t n_src_rows;
  int32_t col_limit;
} agnn_hgt_src_item_t;
int agnn_hgt_attn_bwd_src_batch_f32(int32_t n_items, const agnn_hgt_src_item_t* items /* (host) */, const float* q, int64_t ld_q,
                                    const float* dm, int64_t ld_dm, int32_t H, int32_t heads, agnn_stream_t stream);


/* ------------------------------------------------------------------------------------------
 * Edge-gated aggregation of the in-tree ResGatedGraphConv (ref: models/core/gnn.py:243-258):
 *     S_i = sum_{p in row i} sigmoid(a_i + b_col[p] [+ c_perm[p]]) * h_col[p]
 * a, b, h are [*, ld] fp32 matrices (W3 x, W4 x, W2 x), c an optional per-edge [E, ld_c] term in COO order.
 * fwd / bwd_dst take the CSR grouped by the aggregating row (a indexed by row; b, h by col);
 * bwd_src takes the TRANSPOSED CSR (b, h indexed by row; a and dS by col).  Same a/b/h/c pointers in all calls.
 *   bwd_dst: da_i = sum_e dS_i h_j z(1-z)   and, when dc != NULL, dc[perm[p]] = that summand
 *   bwd_src: db_j = sum_e dS_i h_j z(1-z),  dh_j = sum_e z dS_i
 * da, db, dh have the leading dimension ld of a / b / h, dc that of c (ld_c; dc needs c).  H % 4 == 0, H <= 1024; every
 * pointer 16-byte aligned, every leading dimension a multiple of 4 and >= H (ld_out and ld_ds included), rowptr / col /
 * a / b / h non-NULL: AGNN_EINVAL / AGNN_EALIGN otherwise, before any launch.  n_rows == 0: success, nothing is read.
 * ------------------------------------------------------------------------------------------ */
typedef struct {
  const int32_t* rowptr;  /* (device) [n_rows + 1] */
  const int32_t* col;     /* (device) */
  const int32_t* perm;    /* (device) COO position per CSR position (needed when c != NULL and in backward) */
  const float* a;
  const float* b;
  const float* h;
  const float* c;         /* (device) [n_edges, ld_c] or NULL */
  int64_t ld, ld_c;
  int64_t n_rows;
  int32_t H;
} agnn_gated_t;

int agnn_gated_fwd_f32(const agnn_gated_t* g /* (host) */, float* out, int64_t ld_out, agnn_stream_t stream);
int agnn_gated_bwd_dst_f32(const agnn_gated_t* g /* (host) */, const float* ds, int64_t ld_ds, float* da,
                           float* dc, agnn_stream_t stream);
int agnn_gated_bwd_src_f32(const agnn_gated_t* g /* (host) */, const float* ds, int64_t ld_ds, float* db,
                           float* dh, agnn_stream_t stream);

/* ------------------------------------------------------------------------------------------
 * fp32 projection GEMM on the matrix cores (v_mfma_f32_32x32x2_f32, exact fp32):  C[M, N] = A[M, K] * W[N, K]^T (+ bias[N])
 * — `nn.Linear` / PyG SAGEConv's lin_l, lin_r on a tall activation matrix (ref: models/cadence.py:147-159, core/gnn.py:65,75).
 * agnn_gemm_nt_f32: both operands K-contiguous (the forward product with the weight [out, in] as it lies in memory);
 * agnn_gemm_nn_f32: the second operand K-MAJOR, w[K, N] — C[M, N] = A[M, K] * w[K, N] (+ bias): the input-gradient product
 * dX = dY * W with the same weight [out = K, in = N], no transposed copy.  N % 64 == 0, K % 16 == 0, 16-byte aligned rows
 * (ld % 4 == 0, covering a row of their operand).  linear.HAND_GEMM sends the step's projections with >= 4 096 rows here.
 * ------------------------------------------------------------------------------------------ */
int agnn_gemm_nn_f32(const float* a, int64_t ld_a, const float* w /* [K, N] */, int64_t ld_w, const float* bias, int64_t M, int32_t N,
                     int32_t K, float* c, int64_t ld_c, agnn_stream_t stream);
int agnn_gemm_nt_f32(const float* a, int64_t ld_a, const float* w, int64_t ld_w, const float* bias, int64_t M, int32_t N,
                     int32_t K, float* c, int64_t ld_c, agnn_stream_t stream);
/* agnn_gemm_nt_f32 with its first operand in two column blocks that are never concatenated:  C = [a0 | a1] * w^T (+ bias), a0 [M, K0] and
 * a1 [M, K1] with their own leading dimensions, w [N, K0 + K1].  K0 and K1 multiples of 16 (the tile's k-step); same k order, so the
 * result has the bits of agnn_gemm_nt_f32 on the concatenation. */
int agnn_gemm_nt2_f32(const float* a0, int64_t ld_a0, int32_t K0, const float* a1, int64_t ld_a1, int32_t K1, const float* w,
                      int64_t ld_w, const float* bias, int64_t M, int32_t N, float* c, int64_t ld_c, agnn_stream_t stream);

/* ------------------------------------------------------------------------------------------
 * Aggregation side of the in-tree RelEdgeConv (ref: models/core/gnn.py:99-105: m_ij = W_e [h_j || |h_i - h_j|] + b_e scattered
 * with mean onto row i).  W_e is linear, so sum_j m_ij = W_e [S_i || D_i] + deg_i b_e with the two per-row aggregates
 *     S_i = sum_{p in row i} h_col[p] ,    D_i = sum_{p in row i} |h_i - h_col[p]|
 * computed here in one pass (either output may be NULL); the edge GEMM [E, 2F] x [2F, F] becomes a node GEMM.
 * Backward, one launch per CSR direction, the second with accumulate = 1 onto the first's output:
 *     by_col = 0 (the forward CSR):      out_r (+)= gd_r * sum_p sign(h_r - h_col[p])
 *     by_col = 1 (the transposed CSR):   out_r (+)= sum_p [ sign(h_r - h_col[p]) * gd_col[p] + gs_col[p] ]
 * (gd / gs: gradients of D / S, either may be NULL; sign(0) = 0 as torch.abs' backward.)  H % 4 == 0, H <= 1024.
 * ------------------------------------------------------------------------------------------ */
int agnn_absdiff_fwd_f32(const int32_t* rowptr, const int32_t* col, const float* h, int64_t ld, int64_t n_rows, int32_t H,
                         float* out_s, float* out_d, int64_t ld_out, agnn_stream_t stream);
int agnn_absdiff_bwd_f32(const int32_t* rowptr, const int32_t* col, const float* h, int64_t ld, int64_t n_rows, int32_t H,
                         const float* gd, const float* gs, int64_t ld_g, int32_t by_col, int32_t accumulate, float* out,
                         int64_t ld_out, agnn_stream_t stream);

/* ------------------------------------------------------------------------------------------
 * Fused [ReLU ->] LayerNorm [-> ReLU] [-> dropout] over the rows of x [n, H] (the element-wise chains between the
 * projections, ref: models/analysis.py:429-443, :474-485; models/cadence.py:252-259).  Saves mean / rstd [n];
 * backward recomputes the ReLU masks from x and the dropout mask from the counter-based generator:
 * Philox-4x32-10(seed = rng_state[0], counter = (element, call_id, step = rng_state[1])), rng_state a DEVICE
 * int64[2] so a captured graph draws new masks when the caller bumps the step between replays.  The forward call copies
 * the (seed, step) pair it used into `rng_used` (DEVICE int64[2], may be NULL): hand THAT to the backward call as its
 * rng_state — the live counter may have been bumped by another forward in between (two batches with a joint backward,
 * gradient accumulation, the reference's memory replay: models/analysis.py:1064-1066).
 * `seg`: the statistics are taken over segments of `seg` consecutive floats of a row (seg = H: plain LayerNorm;
 * seg = 64 with H = T*64: the T task heads' LayerNorms of one note in one pass, gamma / beta being the [T*64]
 * concatenation of the per-task affines).  seg must be 4*2^k, divide 256 and divide H.  mean / rstd: [n, H/seg].
 * ------------------------------------------------------------------------------------------ */
#define AGNN_NA_PRE_RELU  1u
#define AGNN_NA_POST_RELU 2u
size_t agnn_norm_act_workspace_bytes(int32_t H);
int agnn_norm_act_fwd_f32(const float* x, int64_t ld_x, const float* gamma, const float* beta, int32_t seg,
                          int64_t n, int32_t H, float eps, float p, uint32_t flags, const int64_t* rng_state, uint32_t call_id, float* y,
                          int64_t ld_y, float* mean, float* rstd, int64_t* rng_used, agnn_stream_t stream);
int agnn_norm_act_bwd_f32(const float* x, int64_t ld_x, const float* gamma, const float* beta, int32_t seg,
                          int64_t n, int32_t H, float eps, float p, uint32_t flags, const int64_t* rng_state, uint32_t call_id,
                          const float* dy, int64_t ld_dy, const float* mean, const float* rstd, float* dx,
                          int64_t ld_dx, float* dgamma, float* dbeta, void* workspace, size_t workspace_bytes,
                          agnn_stream_t stream);

/* agnn_norm_act_bwd_f32 with dgamma == dbeta == NULL leaves the per-block partial sums in `workspace` and launches only the
 * input-gradient kernel; this entry point turns them into dgamma / dbeta later (same n, H, workspace): the two parameter
 * gradients only feed the optimizer and need not sit on the backward pass's dependent chain. */
/* Several pending column sums (agnn_norm_act_colsum_f32) in one launch: they only feed the optimizer and are pending together at
 * the encoder's flush points.  At most 16 items. */
typedef struct {
  const void* workspace;   /* what agnn_norm_act_bwd_f32 (dgamma == dbeta == NULL) left */
  size_t workspace_bytes;
  int64_t n;
  int32_t H;
  float* dgamma;
  float* dbeta;
} agnn_colsum_item_t;
int agnn_norm_act_colsum_batch_f32(int32_t n_items, const agnn_colsum_item_t* items /* (host) */, agnn_stream_t stream);

/* HGT layer epilogue in one launch each way (round 3):  z = dropout_p( relu?( x + sigmoid(*skip) * (o - x) ) )  — PyG HGTConv's
 * learnable skip connection (alpha = sigmoid(skip[node type])) followed by the ReLU + dropout the encoders put between layers
 * (graphmuse HybridHGT via models/analysis.py:445-453).  x == skip == NULL: no skip connection, z = act(o).  flags bit 0 = ReLU.
 * Dropout as agnn_norm_act_* (counter-based masks; `rng_used` receives the (seed, step) this call drew from, backward takes it).
 * Backward recomputes both masks, writes d o (= alpha g), d x (= (1 - alpha) g, optional) and d skip (optional; needs
 * `workspace`: agnn_skip_act_workspace_bytes(), 256-byte aligned, ZERO-FILLED once by the caller — every call leaves it so). */
size_t agnn_skip_act_workspace_bytes(void);
int agnn_skip_act_fwd_f32(const float* x, int64_t ld_x, const float* o, int64_t ld_o, const float* skip, int64_t n, int32_t H, float p,
                          uint32_t flags, const int64_t* rng_state, uint32_t call_id, float* z, int64_t ld_z, int64_t* rng_used,
                          agnn_stream_t stream);
int agnn_skip_act_bwd_f32(const float* x, int64_t ld_x, const float* o, int64_t ld_o, const float* skip, int64_t n, int32_t H, float p,
                          uint32_t flags, const int64_t* rng_state, uint32_t call_id, const float* dz, int64_t ld_dz, float* dx,
                          int64_t ld_dx, float* dout, int64_t ld_do, float* dskip, void* workspace, size_t workspace_bytes,
                          agnn_stream_t stream);
int agnn_norm_act_colsum_f32(const void* workspace, size_t workspace_bytes, int64_t n, int32_t H, float* dgamma, float* dbeta,
                             agnn_stream_t stream);

/* ------------------------------------------------------------------------------------------
 * Weight-gradient GEMM of a projection layer y = x W^T + b over N rows (N large, out/in small):
 *     dw[out, in] = sum_n dy[n, out] * x[n, in]        db[out] = sum_n dy[n, out]   (db may be NULL)
 * fp32-input MFMA, split along N into slabs in `workspace` (agnn_wgrad_workspace_bytes), summed in a fixed
 * order.  Replaces the backward of the `nn.Linear` / PyG `lin_l`, `lin_r` projections on the path
 * (ref: models/analysis.py:429-443,474-485; models/cadence.py:147-159).  out, in and all leading dimensions
 * must be even, pointers 8-byte aligned.
 * ------------------------------------------------------------------------------------------ */
size_t agnn_wgrad_workspace_bytes(int64_t n, int32_t out_f, int32_t in_f);
int agnn_wgrad_f32(const float* dy, int64_t ld_dy, const float* x, int64_t ld_x, int64_t n, int32_t out_f,
                   int32_t in_f, float* dw, int64_t ld_dw, float* db, void* workspace, size_t workspace_bytes,
                   agnn_stream_t stream);
/* Several weight gradients in ONE launch pair (product kernel + slab reduction): the items' workgroups fill the chip together, so
 * every item gets by with a few row slices instead of up to 64 (fewer slabs written and read back, longer K loops) and the
 * step's ~20 reduction launches become one per group.  Same arithmetic per item as agnn_wgrad_f32 with that slice count
 * (deterministic; the slice count — hence the summation order — depends on the group's composition).  At most
 * AGNN_WGRAD_BATCH_MAX_ITEMS items: the host groups 16 products, and a product whose input lies in two column blocks comes as two
 * items (same tiles, same slices, same bits as the one item on the concatenation when the blocks are multiples of the 128-column
 * tile). */
#define AGNN_WGRAD_BATCH_MAX_ITEMS 24
typedef struct {
  const float* dy;   /* (device) [n, out_f], leading dimension ld_dy */
  const float* x;    /* (device) [n, in_f],  leading dimension ld_x  */
  float* dw;         /* (device) out [out_f, in_f], leading dimension ld_dw */
  float* db;         /* (device) out [out_f] or NULL */
  int64_t ld_dy, ld_x, ld_dw, n;
  int32_t out_f, in_f;
} agnn_wgrad_item_t;
size_t agnn_wgrad_batch_workspace_bytes(int32_t n_items, const agnn_wgrad_item_t* items /* (host) */);
int agnn_wgrad_batch_f32(int32_t n_items, const agnn_wgrad_item_t* items /* (host) */, void* workspace, size_t workspace_bytes,
                         agnn_stream_t stream);

/* ------------------------------------------------------------------------------------------
 * Batched small 2-D gather / sum, one launch for many parameter-sized pieces:
 *     dst_i[r, c] = sum_{k < n_src_i} src_{i,k}[r, c]        r < rows_i, c < cols_i
 * Used to present per-relation parameters as one GEMM operand (PyG HeteroConv over SAGEConv: the lin_l weights side by
 * side, lin_r weights and biases summed — ref: models/cadence.py:147-159,174) and to split / fan out the operand's
 * gradient again.  All sources of an item share ld_src.  Destinations of different items must not overlap.
 * n_src_i = 0 zero-fills the piece (ld_src ignored).
 * `vec_ok` is filled in by the library.  Items are read on the host during the call.
 * ------------------------------------------------------------------------------------------ */
#define AGNN_PACK_MAX_SRC   8
#define AGNN_PACK_MAX_ITEMS 24
typedef struct {
  float* dst;                               /* (device) */
  const float* src[AGNN_PACK_MAX_SRC];      /* (device) */
  int64_t ld_dst, ld_src;
  int32_t rows, cols, n_src, vec_ok;
} agnn_pack_item_t;
int agnn_pack_f32(int32_t n_items, const agnn_pack_item_t* items /* (host) */, agnn_stream_t stream);

/* ------------------------------------------------------------------------------------------
 * Gradient epilogue: the products of agnn_wgrad_batch_f32 and the column sums of agnn_norm_act_colsum_batch_f32 with their
 * results stored where they are finally wanted, in ONE reduction launch behind the product kernel.
 *   * A product has up to AGNN_PACK_MAX_SRC weight destinations.  Record k receives columns [c0, c1) of dW: element (o, c) goes
 *     to p[o * ld + (c - c0)].  Several records may name the same range (the summed root weight of a SAGE layer: one copy per
 *     relation); columns that no record names are dropped (the spare column of an operand padded to an even width).  A record
 *     with an even column count needs an even c0, an even ld and an 8-byte aligned p (stored as float2); one with an odd column
 *     count is stored float by float (any ld >= its width).  `db[k]`, k < n_db: every one receives the bias gradient.
 *   * Product kernel, tiles, row slices, slab layout and summation order are those of agnn_wgrad_batch_f32 on the same operand
 *     list; a column sum has the bits of agnn_norm_act_colsum_f32.  No atomics.
 *   * Destinations of one call must not overlap, except records of one product that name the same column range at the same
 *     address with the same ld (they receive the same values): AGNN_EINVAL.  n_items <= AGNN_WGRAD_BATCH_MAX_ITEMS, n_sums <= AGNN_GRAD_MAX_SUMS; both zero: AGNN_OK, nothing is launched.
 * ------------------------------------------------------------------------------------------ */
#define AGNN_GRAD_MAX_SUMS 16   /* column sums per agnn_grad_epilogue_f32 call */
typedef struct {
  float* p;          /* (device) element (0, c0) of the destination */
  int64_t ld;
  int32_t c0, c1;
} agnn_grad_dst_t;
typedef struct {
  const float* dy;   /* operand fields: as agnn_wgrad_item_t */
  const float* x;
  int64_t ld_dy, ld_x, n;
  int32_t out_f, in_f;
  int32_t n_dw, n_db;
  agnn_grad_dst_t dw[AGNN_PACK_MAX_SRC];
  float* db[AGNN_PACK_MAX_SRC];
} agnn_grad_item_t;
size_t agnn_grad_epilogue_workspace_bytes(int32_t n_items, const agnn_grad_item_t* items /* (host) */);
int agnn_grad_epilogue_f32(int32_t n_items, const agnn_grad_item_t* items /* (host) */, int32_t n_sums,
                           const agnn_colsum_item_t* sums /* (host) */, void* workspace, size_t workspace_bytes, agnn_stream_t stream);

/* Many contiguous pieces copied (src != NULL) or zero-filled (src == NULL) in one launch per AGNN_GATHER_MAX_ITEMS pieces:
 * what dp.FlatGradBuffer.pack has left to do once the producers write their gradients in place — the remaining gradients into
 * their slots of the flat buffer, the slots of parameters without a gradient cleared.  Plainer items than agnn_pack_f32's (no
 * sums, no strides), so that a whole model's remainder fits one kernel argument.  n < 2^31 floats per piece; pieces of one call
 * must not overlap.  Items are read on the host during the call. */
#define AGNN_GATHER_MAX_ITEMS 128
typedef struct {
  float* dst;          /* (device) */
  const float* src;    /* (device) or NULL */
  int64_t n;
} agnn_gather_item_t;
int agnn_gather_f32(int32_t n_items, const agnn_gather_item_t* items /* (host) */, agnn_stream_t stream);

/* Measurement aid (scripts/step_stamps.py): one single-lane kernel that stores the constant-rate 100 MHz counter
 * (s_memrealtime) into *slot when the stream reaches it — a time stamp that can be captured into a hipGraph and read back
 * after the replay, without a profiler attached.  Not used by the product path. */
int agnn_debug_stamp(uint64_t* slot /* (device) */, agnn_stream_t stream);

/* ------------------------------------------------------------------------------------------
 * Note-input assembly (ref: models/analysis.py:574 `torch.cat([x_dict["note"], self.pitch_embedding(pitch_spelling),
 * self.key_embedding(key_signature)], dim=-1)`; tables models/analysis.py:399-400) and the gradient of the tables.
 *   forward   out[n, :] = [ x[n, 0:in_x] | tables[0][idx[0][n], :] | ... | tables[n_tab-1][idx[n_tab-1][n], :] | 0 ... ]
 *             x [n_rows, in_x] (ld_x), idx[t] DEVICE int64 [n_rows] (ids outside [0, vocab[t]) are clamped — torch raises
 *             a device assert there), tables[t] DEVICE [vocab[t], dim] contiguous, out [n_rows, ld_out] with
 *             ld_out >= in_x + n_tab*dim; the columns behind the last table are zero-filled.
 *   backward  dtables[vbase_t + v, :] = sum_{n: idx[t][n] == v} dout[n, col0 + t*dim : col0 + (t+1)*dim]  with
 *             vbase_t = vocab[0] + ... + vocab[t-1]; dtables DEVICE [sum vocab, dim] contiguous; dim even.  Rows are
 *             added in row order inside 32 row slices that are summed in a fixed order (no atomics, reproducible).
 * `idx`, `tables`, `vocab` are HOST arrays (of device pointers / sizes) read during the call.
 * ------------------------------------------------------------------------------------------ */
#define AGNN_EMBED_MAX_TABLES 4
int agnn_embed_cat_fwd_f32(const float* x, int64_t ld_x, int32_t in_x, int64_t n_rows, int32_t n_tab,
                           const int64_t* const* idx /* (host) */, const float* const* tables /* (host) */,
                           const int32_t* vocab /* (host) */, int32_t dim, float* out, int64_t ld_out, agnn_stream_t stream);
size_t agnn_embed_workspace_bytes(int32_t n_tab, const int32_t* vocab /* (host) */, int32_t dim);
int agnn_embed_cat_bwd_f32(const float* dout, int64_t ld_dout, int32_t col0, int64_t n_rows, int32_t n_tab,
                           const int64_t* const* idx /* (host) */, const int32_t* vocab /* (host) */, int32_t dim, float* dtables,
                           void* workspace, size_t workspace_bytes, agnn_stream_t stream);

/* ------------------------------------------------------------------------------------------
 * The task-head block in one launch (ref: models/analysis.py:486-496 `clf_dict[task] = Linear(o, o/2) -> ReLU ->
 * LayerNorm(o/2) -> Linear(o/2, C_t)`, :546-548): for every task t
 *     z_t = x W1_t^T + b1_t;   y_t = LayerNorm_t(ReLU(z_t));   logits[:, offs[t]:offs[t+1]] = y_t W2_t^T + b2_t
 *   x [n_rows, in_f] (ld_x), w1 [T*hidden, in_f] / b1, gamma, beta [T*hidden] = the tasks' parameters stacked along rows,
 *   w2 [sum_c, hidden] / b2 [sum_c] (b2 may be NULL), offs_dev DEVICE int32 [T+1], offs_host the same on the HOST (it sizes
 *   the grid and deals the tasks to workgroups).  Written for the backward pass (agnn_norm_act_bwd_f32 with seg = hidden,
 *   agnn_gproj_bwd_f32): z, y [n_rows, T*hidden] (ld_h), mean / rstd [n_rows, T].  This build: in_f = 128, hidden = 64, T <= 64.
 * ------------------------------------------------------------------------------------------ */
int agnn_heads_fwd_f32(const float* x, int64_t ld_x, int64_t n_rows, int32_t in_f, int32_t hidden, int32_t T, const float* w1,
                       const float* b1, const float* gamma, const float* beta, float eps, const float* w2, const float* b2,
                       const int32_t* offs_dev, const int32_t* offs_host /* (host) */, float* z, float* y, int64_t ld_h, float* mean,
                       float* rstd, float* logits, int64_t ld_o, agnn_stream_t stream);

/* ------------------------------------------------------------------------------------------
 * Grouped projection: the last Linear(h2 -> C_t) of all task heads in one launch per direction
 * (ref: models/analysis.py:486-496 `clf_dict[task]`, :546-548).  Group g reads columns [g*K, (g+1)*K) of a and
 * owns output columns [seg_off[g], seg_off[g+1]) (the same side-by-side logits layout agnn_multitask_ce_f32 takes):
 *     out[n, seg_off[g] + c] = b[seg_off[g] + c] + sum_k a[n, g*K + k] * w[seg_off[g] + c, k]
 *   a [n_rows, n_groups*K] (ld_a), w [sum_c, K] = the per-task weights stacked along rows, b [sum_c] or NULL,
 *   seg_off DEVICE int32 [n_groups + 1], n_tiles32 = sum_g ceil(C_g / 32) (host-side count that sizes the grid),
 *   K in {32, 64, 128}.  Backward: da [n_rows, n_groups*K] (NULL to skip), dw [sum_c, K] and db [sum_c] (dw NULL to
 *   skip both; db may be NULL); dw/db are summed over row slices held in `workspace` in a fixed order.
 * ------------------------------------------------------------------------------------------ */
int agnn_gproj_fwd_f32(const float* a, int64_t ld_a, const float* w, const float* b, const int32_t* seg_off,
                       int32_t n_groups, int32_t K, int32_t n_tiles32, int64_t n_rows, float* out, int64_t ld_out,
                       agnn_stream_t stream);
size_t agnn_gproj_workspace_bytes(int64_t n_rows, int32_t sum_c, int32_t K, int32_t n_tiles32);
int agnn_gproj_bwd_f32(const float* dout, int64_t ld_dout, const float* a, int64_t ld_a, const float* w,
                       const int32_t* seg_off, int32_t n_groups, int32_t K, int32_t n_tiles32, int32_t sum_c,
                       int64_t n_rows, float* da, int64_t ld_da, float* dw, float* db, void* workspace,
                       size_t workspace_bytes, agnn_stream_t stream);

/* ------------------------------------------------------------------------------------------
 * Fused multi-task cross entropy (label smoothing, ignore index) over column segments of one logits
 * matrix: replaces the per-task `nn.CrossEntropyLoss(ignore_index=-1, label_smoothing=0.1)` terms
 * (ref: models/analysis.py:881-888, models/chord.py:39-49).  Task t owns columns [seg_off[t], seg_off[t+1]).
 *   labels    int64 [n_tasks, n_rows]
 *   row_loss  [n_tasks, n_rows]  per-row loss terms (0 for ignored rows)                      (scratch output)
 *   dlogits   [n_rows, ld]       d loss_row / d logits, NOT yet divided by the task's row count (ignored rows: 0;
 *                                columns outside the segments untouched)
 *   loss      [n_tasks]          mean loss per task = sum_n row_loss[t][n] / max(count_t, 1)
 *   inv_count [n_tasks]          1 / max(count_t, 1), count_t = rows with label != ignore_index
 * agnn_multitask_ce_scale_f32: out[n, c] = dlogits[n, c] * scale[task(c)] for c < n_cols (columns outside every
 * segment are copied) — the backward pass with scale[t] = inv_count[t] * (incoming gradient of loss[t]).
 * ------------------------------------------------------------------------------------------ */
int agnn_multitask_ce_f32(const float* logits, int64_t ld, const int32_t* seg_off, int32_t n_tasks,
                          const int64_t* labels, int64_t n_rows, float label_smoothing,
                          int64_t ignore_index, float* row_loss, float* dlogits, float* loss, float* inv_count,
                          agnn_stream_t stream);
int agnn_multitask_ce_scale_f32(const float* dlogits, int64_t ld, const int32_t* seg_off, int32_t n_tasks,
                                int64_t n_rows, int32_t n_cols, const float* scale, float* out, int64_t ld_out,
                                agnn_stream_t stream);

/* ------------------------------------------------------------------------------------------
 * Training loss of one step in two launches, its gradient in one:
 *     total = ce_scale * sum_t (w_t * loss[t] + reg_t) + lambda_feat * mean(feat^2)
 *     task_param == NULL: w_t = 1, reg_t = 0;  else p = task_param[t]: w_t = 0.5 / p^2, reg_t = log(1 + p^2)
 * i.e. the per-task label-smoothed cross entropies above, combined as the reference's MultiTaskLoss does (learned
 * uncertainty weights, ref models/chord.py:39-49; selected by the CLI default --mt_strategy wloss, models/analysis.py:
 * 899-908), divided by the number of tasks (ce_scale = 1/T: models/analysis.py:1036), plus the feature-norm term
 * (models/analysis.py:984 `feature_loss = x.pow(2).mean()`, :1072 `... + feature_loss * self.lambda_featl`, :910 default
 * 0.1).  Same per-task outputs as agnn_multitask_ce_f32, plus `total` (device scalar), `wscale[t]` = ce_scale * w_t *
 * inv_count[t] (the per-task gradient scale: hand it to agnn_train_loss_bwd_f32 as its `inv_count`) and `dparam[t]` =
 * d total / d p_t = ce_scale * (2 p / (1 + p^2) - loss[t] / p^3) (0 without task_param); wscale / dparam may be NULL.
 * A task without any valid row contributes loss 0 (torch: NaN).  feat [n_rows, feat_cols] (ld_feat) may be NULL (no
 * feature term).  `workspace` (agnn_train_loss_workspace_bytes(), 256-byte aligned) must be ZERO-FILLED before its first
 * use; every call leaves its ticket zero again (it orders the fixed-order final sum).  Backward, given g =
 * d(objective)/d(total) as a DEVICE scalar:
 *     out[n, c]   = dlogits[n, c] * g * inv_count[task(c)]          (columns outside the segments: 0)
 *     dfeat[n, c] = g * 2 * lambda_feat / (n_rows * feat_cols) * feat[n, c]        (dfeat NULL to skip)
 * ------------------------------------------------------------------------------------------ */
size_t agnn_train_loss_workspace_bytes(void);
int agnn_train_loss_f32(const float* logits, int64_t ld, const int32_t* seg_off, int32_t n_tasks, const int64_t* labels,
                        int64_t n_rows, float label_smoothing, int64_t ignore_index, const float* feat, int64_t ld_feat,
                        int32_t feat_cols, float lambda_feat, const float* task_param, float ce_scale, float* row_loss,
                        float* dlogits, float* loss, float* inv_count, float* total, float* wscale, float* dparam,
                        void* workspace, size_t workspace_bytes, agnn_stream_t stream);
/* The same objective with the gradients FINISHED in the forward launches (for an incoming gradient of 1, which is what
 * `total.backward()` passes): wscale[t] is computed first (a count of the task's valid labels: one small launch), the
 * cross-entropy kernel then writes dlogits[n, c] = wscale[task(c)] * (p - target) directly, and the launch that reduces the
 * losses also writes dfeat[n, c] = 2 * lambda_feat / (n_rows * feat_cols) * feat[n, c] (dfeat may be NULL).  The backward pass
 * then has no launch of its own (agnn_train_loss_bwd_f32's scale pass re-read and re-wrote the [N, C] matrix: 23 us at C2 on
 * the step's serial stretch); a caller with another incoming gradient g multiplies the three gradients by g.  Same
 * reference lines, outputs, workspace contract and error behaviour as agnn_train_loss_f32; wscale is required here. */
int agnn_train_loss_final_f32(const float* logits, int64_t ld, const int32_t* seg_off, int32_t n_tasks, const int64_t* labels,
                              int64_t n_rows, float label_smoothing, int64_t ignore_index, const float* feat, int64_t ld_feat,
                              int32_t feat_cols, float lambda_feat, const float* task_param, float ce_scale, float* row_loss,
                              float* dlogits, float* loss, float* inv_count, float* total, float* wscale, float* dparam,
                              float* dfeat, int64_t ld_dfeat, void* workspace, size_t workspace_bytes, agnn_stream_t stream);
int agnn_train_loss_bwd_f32(const float* dlogits, int64_t ld, const int32_t* seg_off, int32_t n_tasks, int64_t n_rows,
                            int32_t n_cols, const float* inv_count, const float* g, float* out, int64_t ld_out,
                            const float* feat, int64_t ld_feat, int32_t feat_cols, float lambda_feat, float* dfeat,
                            int64_t ld_dfeat, agnn_stream_t stream);

/* ------------------------------------------------------------------------------------------
 * Device-side batch assembly: neighbour sampling of note windows out of score graphs resident in device memory
 * (replaces graphmuse's `MuseNeighborLoader` + collation + host-to-device copy, ref data/datamodules/analysis.py:270-293:
 * subgraph_size target notes per window, num_neighbors per hop, batch_size windows; PyG NeighborLoader layout consumed at
 * models/analysis.py:948-961).  One launch fills buffers of STATIC shape (hop blocks padded to capacity), so the sampled
 * batch — and with it the whole training step — is a fixed launch sequence a hipGraph can replay:
 *   nodes  [ n_sub*n_targets | n_sub*cap[0] | n_sub*cap[1] | ... ]   node_gid = global note id, -1 in unused slots; a
 *          subgraph's new nodes of a hop take its slots in ascending global id;
 *   edges[r]  int64 [2, e_cap] (row 0 = source, row 1 = target, batch-local ids; (-1, -1) in unused slots, which
 *          agnn_csr_build drops): hop h owns n_sub * F_h * fan[h] slots, F_1 = n_targets, F_h = cap[h-2]; slot
 *          ((s*F_h + i)*fan[h] + k) = k-th sampled in-neighbour of frontier node i of subgraph s.
 * rowptr / col: CSR by DESTINATION of every relation over all notes of all scores (int32).  All in-neighbours are taken
 * when there are at most fan[h]; otherwise fan[h] of them without replacement (selection sampling on Philox-4x32-10 keyed
 * by rng = (seed, step) and (destination, relation, hop)).  Hop h+1 expands only the nodes hop h added (PyG semantics).
 * `drops` (optional device int32[1], caller-owned, only ever incremented) counts sources dropped because a hop proposed
 * more than cap[h] new nodes — a STATISTIC, expected on crowded scores: the cap[h] smallest global ids are kept, whatever
 * their number, and a dropped source stays dropped in later hops.  `status` (optional, the agnn_csr_build word) is bumped
 * only by an ERROR: a subgraph proposed more distinct out-of-window sources than the kernel's table holds (4096); the
 * sources that found no place are left out of the batch and agnn_check_status reports it.
 * agnn_gather_rows_f32 / agnn_gather_i64 fetch the batch's feature rows / integer attributes by node_gid (0 / `fill` for
 * padding slots).
 * ------------------------------------------------------------------------------------------ */
#define AGNN_SAMPLER_MAX_REL 8
#define AGNN_SAMPLER_MAX_HOPS 4
#define AGNN_SAMPLER_MAX_FAN 16
#define AGNN_SAMPLER_MAX_CAP 256
typedef struct {
  int32_t n_rel;
  const int32_t* rowptr[AGNN_SAMPLER_MAX_REL];   /* (device) [n_notes_total + 1] */
  const int32_t* col[AGNN_SAMPLER_MAX_REL];      /* (device) source note of every in-edge */
  const int32_t* win_start;                      /* (device) [n_sub] global id of each window's first target note */
  int32_t n_sub, n_targets, n_hops;
  int32_t fan[AGNN_SAMPLER_MAX_HOPS];
  int32_t cap[AGNN_SAMPLER_MAX_HOPS];
  const int64_t* rng;                            /* (device) int64[2]: seed, step */
  int32_t* node_gid;                             /* (device) out [agnn_sampler_num_nodes] */
  int64_t* edges[AGNN_SAMPLER_MAX_REL];          /* (device) out, per relation int64 [2, e_cap] */
  int64_t e_cap;                                 /* = agnn_sampler_edge_capacity */
  int32_t* status;                               /* (device) int32[1] or NULL: errors (agnn_check_status) */
  int32_t* drops;                                /* (device) int32[1] or NULL: sources cut by cap[h] (statistic) */
  int32_t* kept;                                 /* (device) int32[n_hops * n_sub] or NULL: nodes kept per (hop, subgraph) */
} agnn_sampler_t;
int64_t agnn_sampler_num_nodes(const agnn_sampler_t* cfg /* (host) */);
int64_t agnn_sampler_edge_capacity(const agnn_sampler_t* cfg /* (host) */);
int agnn_sample_hops(const agnn_sampler_t* cfg /* (host) */, agnn_stream_t stream);
/* Metrical nodes of a sampled batch (the reference's graphs carry beat and measure nodes unless `remove_beats/measures` is set,
 * ref data/datamodules/analysis.py:213-225; every note belongs to one beat and one measure, hgraph edge type
 * (note, connects, beat|measure)).  `group_of` (device int32 [n_notes_total]): the global id of the note's group, non-decreasing
 * inside a score (notes are sorted by onset), so the groups of a window's target notes are ONE contiguous range
 * [group_of[w], group_of[w + n_targets - 1]] — no set, no sort.  After agnn_sample_hops (same layout arguments):
 *   group_gid [n_sub * cap_g]   subgraph s owns slots [s*cap_g, (s+1)*cap_g): its range in ascending id, -1 in unused slots
 *                               (`drops`, optional, counts groups beyond the capacity);
 *   edges int64 [2, n_nodes]    slot i = batch note i: (i, batch-local group slot) when the note's group lies in its subgraph's
 *                               range, else (-1, -1).  Slot order = node order, so the per-hop edge counts that drive
 *                               trim_to_layer are [n_sub*(n_targets + cap[0]), n_sub*cap[1], ...]: an edge is trimmed with
 *                               its source note's hop block; the group nodes themselves are all hop-0 (never trimmed). */
int agnn_sample_members(const int32_t* node_gid, int64_t n_nodes, const int64_t* batch /* NULL, or (pool layout) subgraph id per slot */,
                        const int32_t* group_of, const int32_t* win_start, int32_t n_sub, int32_t n_targets, int32_t n_hops,
                        const int32_t* cap /* (host) [n_hops] */, int32_t cap_g, int32_t* group_gid, int64_t* edges, int32_t* drops,
                        agnn_stream_t stream);
/* The padded hop blocks [n_sub x cap[h]] squeezed into batch-wide POOLS of pool[h] <= n_sub * cap[h] slots (a subgraph rarely
 * fills its capacity: at C2 170 of 2 048 slots are used): subgraph s's kept nodes of hop h move to
 * pool_base[h] + sum_{s' < s} kept[h][s'] + rank — still hop-ordered, still static shapes (trim counts = the pool sizes), a
 * subgraph's nodes still contiguous.  Run after agnn_sample_hops with the same configuration (`kept` set): writes the node ids
 * in pool layout (agnn_sample_compact_nodes slots) and the subgraph id of every slot, and rewrites the endpoints of every edge
 * slot IN PLACE; nodes past a pool's end are dropped with their edges and counted in `drops`. */
int64_t agnn_sample_compact_nodes(const agnn_sampler_t* cfg /* (host) */, const int32_t* pool /* (host) [n_hops] */);
int agnn_sample_compact(const agnn_sampler_t* cfg /* (host) */, const int32_t* pool /* (host) [n_hops] */, int32_t* node_gid_out,
                        int64_t* batch_out, agnn_stream_t stream);
int agnn_gather_rows_f32(const float* src, int64_t ld_src, const int32_t* gid, int64_t n, int32_t H, float* out,
                         int64_t ld_out, agnn_stream_t stream);
int agnn_gather_i64(const int64_t* src, int64_t ld_src, const int32_t* gid, int64_t n, int32_t n_vec, int64_t fill,
                    int64_t* out, int64_t ld_out, agnn_stream_t stream);

/* ------------------------------------------------------------------------------------------
 * Per-head relation transforms of HGTConv (PyG `k_rel` / `v_rel`: one D x D matrix per (edge type, head); reached through
 * graphmuse's HybridHGT, ref models/analysis.py:445-453 `heads=4`).  For the n_rel relations leaving one node type:
 *     forward   y[n, (r*heads + h)*D + j] = sum_i x[n, h*D + i] * w[((r*heads + h)*D + i)*D + j]
 *     backward  dx[n, h*D + i]            = sum_r sum_j dy[n, (r*heads + h)*D + j] * wt[((r*heads + h)*D + j)*D + i]
 *     dw        dw[((r*heads + h)*D + i)*D + j] = sum_n x[n, h*D + i] * dy[n, (r*heads + h)*D + j]
 * i.e. n_rel*heads independent [n, D] x [D, D] products on the fp32-input MFMA instead of one dense GEMM against a
 * block-diagonal weight (heads x the useful FLOPs).  D is one of 4, 8, 16, 32, 64, 128, 256 (the head widths of agnn_hgt_attn_*;
 * anything else: AGNN_EINVAL): plain FMAs at D = 4, 8, one 16x16x4 / 32x32x2 fp32 MFMA tile per block at D = 16 / 32, the
 * 32x32x2 fp32 MFMA over 64 x 64 pieces of the block at D = 64, 128, 256.  fwd / bwd: x and w 16-byte aligned, ld_x % 4 == 0;
 * dw: x and dy 8-byte aligned, even leading dimensions (AGNN_EALIGN otherwise).  n_rows = 0: fwd / bwd write nothing, dw
 * zero-fills its outputs.  Up to AGNN_RELT_MAX_ITEMS operands of the same shape (K and V) per launch.  Item fields per entry point:
 *     fwd: x = x [n, heads*D] (ld_x), w = blocks [n_rel*heads][D][D], y = y [n, n_rel*heads*D] (ld_y)
 *     bwd: x = dy (ld_x), w = the TRANSPOSED blocks, y = dx [n, heads*D] (ld_y)
 *     dw:  x = x (ld_x), w = dy (ld_y), y = dw blocks [n_rel*heads][D][D] (contiguous); row slices are summed in a
 *          fixed order through `workspace` (agnn_relt_dw_workspace_bytes).
 * ------------------------------------------------------------------------------------------ */
#define AGNN_RELT_MAX_ITEMS 4
typedef struct {
  const float* x;
  const float* w;
  float* y;
  int64_t ld_x, ld_y;
} agnn_relt_item_t;
int agnn_relt_fwd_f32(int n_items, const agnn_relt_item_t* items /* (host) */, int32_t n_rel, int32_t heads, int32_t D,
                      int64_t n_rows, agnn_stream_t stream);
int agnn_relt_bwd_f32(int n_items, const agnn_relt_item_t* items /* (host) */, int32_t n_rel, int32_t heads, int32_t D,
                      int64_t n_rows, agnn_stream_t stream);
size_t agnn_relt_dw_workspace_bytes(int n_items, int32_t n_rel, int32_t heads, int32_t D, int64_t n_rows);
int agnn_relt_dw_f32(int n_items, const agnn_relt_item_t* items /* (host) */, int32_t n_rel, int32_t heads, int32_t D,
                     int64_t n_rows, void* workspace, size_t workspace_bytes, agnn_stream_t stream);

/* ------------------------------------------------------------------------------------------
 * Global-norm gradient clipping + AdamW over flat fp32 buffers (ref optimizer: models/analysis.py:1380-1381
 * `torch.optim.AdamW`; clipping as Lightning's gradient_clip_val does before the step):
 *     g' = g * min(max_norm / (||g||_2 + 1e-6), 1)            (max_norm <= 0: no clipping)
 *     p  = p (1 - lr wd) - lr * (m' / (1 - b1^t)) / (sqrt(v') / sqrt(1 - b2^t) + eps),  m' = b1 m + (1-b1) g', v' = b2 v + (1-b2) g'^2
 * `step` is a DEVICE float holding t-1; the call increments it (so a captured hipGraph advances it on replay).
 * norm_out (device float, may be NULL) receives ||g||_2 before clipping.  write_clipped_grad != 0 stores g' back.
 * Two launches, sums in a fixed order.  Buffers 16-byte aligned.
 * ------------------------------------------------------------------------------------------ */
size_t agnn_adamw_workspace_bytes(void);
int agnn_adamw_f32(float* p, float* g, float* m, float* v, int64_t n, float lr, float beta1, float beta2, float eps,
                   float weight_decay, float max_norm, float* step, float* norm_out, int32_t write_clipped_grad,
                   void* workspace, size_t workspace_bytes, agnn_stream_t stream);

/* ------------------------------------------------------------------------------------------
 * The same step with the learning rate as a CLOSED FORM OF THE DEVICE STEP COUNTER, and stochastic weight averaging.
 * agnn_adamw_f32 takes lr as a host float: inside a captured hipGraph it is a constant of the kernel node, while the
 * reference changes the rate after every optimizer step (`LinearWarmupCosineAnnealingLR` with "interval": "step",
 * models/analysis.py:104-188, :1380-1410; `LinearWarmupExponentialDecayLR`, :191-275) and `--use_swa` adds
 * `StochasticWeightAveraging(swa_lrs=5e-5, swa_epoch_start=50)` (train/train_analysisgnn.py:243-245).  Here the schedule's
 * hyper-parameters are a host struct passed by value into the launch, and the launch that advances the counter evaluates it.
 *
 * Step index: k = optimizer steps already taken = *step before this call's increment; step k uses lr(k).
 * Below the SWA start (k < swa_start, or swa_start < 0), with c = k + count_offset, b = base_lr, s = warmup_start_lr:
 *     c < warmup_steps (both warm-up kinds)   lr = s + (b - s) * c / warmup_steps
 *     AGNN_LR_WARMUP_COSINE, otherwise        lr = eta_min + (b - eta_min) / 2 * (1 + cos(pi * (k - cos_a) / (cos_b - cos_a)))
 *     AGNN_LR_WARMUP_EXP, otherwise           lr = max(eta_min, b * gamma^((c - warmup_steps) / decay_steps))
 *     AGNN_LR_CONSTANT                        lr = b
 * The reference's cosine class stepped once per optimizer step is count_offset = 1, cos_a = warmup_steps / 3, cos_b =
 * max_epochs (its `steps_per_epoch` is current_step / last_epoch at its third step() call: 3.0; it raises AttributeError
 * for warmup_steps < 3, which the host constructor dp.LRSchedule.reference_cosine refuses); its exponential class is
 * count_offset = 1.
 * From the SWA start on (k >= swa_start), with e = (k - swa_start) / swa_period (integer division):
 *     alpha = (1 - cos(pi * min(1, e / swa_anneal))) / 2          (swa_anneal == 0: alpha = 1)
 *     lr    = (1 - alpha) * lr(swa_start) of the schedule above + alpha * swa_lr
 * the closed form of `torch.optim.swa_utils.SWALR(anneal_strategy="cos")` created at step swa_start and stepped once per
 * swa_period optimizer steps.  When (k - swa_start) % swa_period == 0 the parameters AS THEY ARE BEFORE this step's update
 * enter the average: the first snapshot is avg = p, later ones avg += (p - avg) / (n + 1), the default rule of
 * `torch.optim.swa_utils.AveragedModel`; n lives on the device.  The contract is these two torch classes driven as
 * described; parity with Lightning's StochasticWeightAveraging callback (which also swaps the averaged weights in at the
 * end of fit and refreshes BatchNorm statistics, `update_bn`) is NOT pinned, and `update_bn` is not provided.  Resuming
 * from an optimizer checkpoint written by the reference (Lightning / torch.optim layout) is not pinned either: the host
 * side saves and loads these flat buffers (dp.FlatAdamW.state_dict).
 *
 * lr is evaluated once per step, in double (cospi on the phase), rounded to float once, handed to the update launch through
 * the workspace and written to state[0].  `state` (device float[2]): [0] the rate the last step used, [1] the number of
 * snapshots averaged so far (the caller zeroes it once).  swa_avg (device, n floats, 16-byte aligned) is NULL iff
 * swa_start < 0; steps that take no snapshot do not touch it.  The schedule is a launch constant: changing its
 * hyper-parameters needs a new capture; advancing, resuming (write *step, state, swa_avg, m, v in place) and averaging do
 * not.  A constant schedule gives agnn_adamw_f32's results bit for bit (one update body).  Two launches; a snapshot step
 * moves 9 streams of 4n bytes instead of 7.  The counter is a float: exact up to 2^24 steps, like agnn_adamw_f32's.
 * agnn_lr_schedule_at evaluates the same function on the host (no GPU needed); NaN (and a message) for an invalid schedule
 * or k < 0.
 * ------------------------------------------------------------------------------------------ */
#define AGNN_LR_CONSTANT      0
#define AGNN_LR_WARMUP_COSINE 1
#define AGNN_LR_WARMUP_EXP    2
typedef struct {
  int32_t kind;          /* AGNN_LR_* */
  int32_t warmup_steps;  /* W >= 0 */
  int32_t count_offset;  /* c0: warm-up / decay run on c = k + c0 */
  int32_t swa_period;    /* P > 0 optimizer steps per SWA "epoch" */
  int64_t swa_start;     /* K; < 0: no SWA */
  int32_t swa_anneal;    /* Na >= 0 epochs of cosine annealing towards swa_lr */
  double base_lr, warmup_start_lr, eta_min, cos_a, cos_b, gamma, decay_steps, swa_lr;
} agnn_lr_schedule_t;

double agnn_lr_schedule_at(const agnn_lr_schedule_t* sched /* (host) */, int64_t k);
size_t agnn_adamw_sched_workspace_bytes(void);
int agnn_adamw_sched_f32(float* p, float* g, float* m, float* v, int64_t n, const agnn_lr_schedule_t* sched /* (host) */,
                         float beta1, float beta2, float eps, float weight_decay, float max_norm, float* step, float* swa_avg,
                         float* state, float* norm_out, int32_t write_clipped_grad, void* workspace, size_t workspace_bytes,
                         agnn_stream_t stream);

/* ------------------------------------------------------------------------------------------
 * Knowledge distillation of the previous tasks against a frozen copy of the model, the first continual-learning term of
 * the reference's step (ref: models/analysis.py:1052-1062: per task `F.kl_div(F.log_softmax(student / temp, 1),
 * F.softmax(teacher / temp, 1), reduction='batchmean') * temp**2`, temp = 2, `.mean()` over the tasks, times lambda_dctn).
 * student [n_rows, ld_s] and teacher [n_rows, ld_t] hold the tasks' logits in the same column layout (independent row
 * strides; no alignment asked).  Task t owns the columns [seg_off[t], seg_end ? seg_end[t] : seg_off[t+1]): seg_off int32
 * [n_tasks + 1] (device) as for agnn_multitask_ce_f32; seg_end int32 [n_tasks] (device, may be NULL) lets ascending segments
 * leave columns between them uncovered.  With tau = temperature, q = softmax(student_t / tau), p = softmax(teacher_t / tau):
 *     kd[t]          = tau^2 / n_rows * sum_n sum_c p (log p - log q)        both logs as x / tau - logsumexp: a teacher
 *                                                                            probability that underflows to 0 contributes 0
 *     total          = weight / n_tasks * sum_t kd[t]                        (device scalar; weight = the caller's lambda_dctn)
 *     dstudent[n, c] = weight * tau / (n_rows * n_tasks) * (q - p)           d total / d student, FINISHED (incoming gradient 1)
 * Columns c < n_cols that no segment covers are WRITTEN as 0 in dstudent [n_rows, ld_d]; the teacher gets no gradient.
 * Three launches: the row pass (both matrices read once, the gradient written once; rows up to 1024 columns through an LDS
 * image, wider ones from global memory with the same results), a fixed-order sum of the per-row terms per task, and the
 * sum over the tasks in index order: bitwise reproducible.  `workspace` (agnn_kd_workspace_bytes(n_rows, n_tasks) bytes,
 * 4-byte aligned) holds the per-row terms; it carries nothing from call to call.  n_rows == 0: kd and total are set to 0.
 * The offsets are device data and are not checked here: the caller guarantees 0 <= start < end <= n_cols, ascending.
 * ------------------------------------------------------------------------------------------ */
size_t agnn_kd_workspace_bytes(int64_t n_rows, int32_t n_tasks);
int agnn_multitask_kd_f32(const float* student, int64_t ld_s, const float* teacher, int64_t ld_t, const int32_t* seg_off,
                          const int32_t* seg_end, int32_t n_tasks, int64_t n_rows, int32_t n_cols, float temperature,
                          float weight, float* dstudent, int64_t ld_d, float* kd, float* total, void* workspace,
                          size_t workspace_bytes, agnn_stream_t stream);

/* ------------------------------------------------------------------------------------------
 * Elastic weight consolidation over flat fp32 buffers of one layout (parameters, their snapshot, the Fisher estimate, the
 * gradient), the second continual-learning term (ref: models/analysis.py:1479-1495 `ewc_penalty += (self.fisher[n] *
 * (p - self._means[n]).pow(2)).sum()`, weighted by lambda_ewc at :1068):
 *     penalty = sum_i fisher_i (p_i - mean_i)^2                  UNWEIGHTED, device scalar
 *     g_i    += 2 lambda fisher_i (p_i - mean_i)                 if g != NULL: added to the gradient already there
 * One pass (1024 per-block partial sums over slices that depend on n alone) and a fixed-order sum of the partials: bitwise
 * reproducible.  `workspace`: agnn_ewc_workspace_bytes() bytes, nothing carried from call to call.  n == 0: penalty = 0.
 * agnn_fisher_accum_f32: fisher_i += scale * g_i^2 — the reference's `self.fisher[n] += p.grad.data.clone().pow(2) /
 * len_dataloader` (:1440-1455) with scale = 1 / len_dataloader.  Buffers 16-byte aligned.
 * ------------------------------------------------------------------------------------------ */
size_t agnn_ewc_workspace_bytes(void);
int agnn_ewc_f32(const float* p, const float* mean, const float* fisher, int64_t n, float lambda, float* g, float* penalty,
                 void* workspace, size_t workspace_bytes, agnn_stream_t stream);
int agnn_fisher_accum_f32(const float* g, int64_t n, float scale, float* fisher, agnn_stream_t stream);

/* ------------------------------------------------------------------------------------------
 * Validation / test metrics of the task heads (ref: models/analysis.py:1143-1164, :1221-1282: per task torchmetrics
 * `Accuracy(task="multiclass")` and `F1Score(average="macro")`, the same accuracies on the notes predicted as chord tones, and
 * the joint Roman-numeral accuracies): the per-task argmax and the integer counters all of them are ratios of, in ONE launch.
 * logits [n_rows, n_cols] fp32 with leading dimension ld (column-slice views are fine: 4-byte alignment is all that is asked);
 * task t owns the columns [seg_off[t], seg_end ? seg_end[t] : seg_off[t+1]), C = end - start classes: seg_off int32
 * [n_tasks + 1] and seg_end int32 [n_tasks] (may be NULL) on the device, as for agnn_multitask_kd_f32, not checked here (the
 * kernel clamps them to [0, n_cols], so nothing is read or counted out of range whatever they hold).  1 <= n_tasks <=
 * AGNN_MAX_SEG.  labels int64 [n_tasks, n_rows], task-major, or NULL (then counts must be NULL: predictions only);
 * row_mask uint8 [n_rows] or NULL = every row.
 *   pred [n_tasks, n_rows] int32, task-major, optional: the argmax of segment t of row r, for EVERY row whatever mask and
 *     labels say.  torch.argmax's rule: the lowest index among equal maxima; a NaN is the maximum, the first NaN wins; -inf
 *     is an ordinary value; -0 equals +0.
 *   counts, int64 [agnn_eval_counts_len(n_tasks, n_cols) = 4 n_tasks + 4 + 3 n_cols], 8-byte aligned, optional:
 *       valid[T] | correct[T] | valid_g[T] | correct_g[T] | joint_valid, joint_correct, joint_valid_g, joint_correct_g |
 *       tp[n_cols] | n_pred[n_cols] | n_label[n_cols]            (class bins indexed by logits COLUMN)
 *     For a row with row_mask NULL or row_mask[r] != 0, task t with label y != ignore_index and prediction p, a = start of t:
 *       valid[t] += 1, n_pred[a + p] += 1;   0 <= y < C: n_label[a + y] += 1;   additionally p == y: correct[t] += 1, tp[a + y] += 1.
 *     A label outside [0, C) that is not the ignore value counts as valid and wrong and touches no class bin.
 *     gate_task >= 0: valid_g / correct_g count the same events on the rows with pred[gate_task, r] != 0 (the reference's
 *       `mask = logits["tpc_in_label"].argmax(-1).bool()`); gate_task = -1 leaves them alone.
 *     group_mask (bit t = task t) != 0: joint_valid counts the rows that take part and carry a non-ignored label in every
 *       task of the group, joint_correct those of them with every task of the group correct; joint_*_g the same on gated rows.
 *     Counters are ADDED TO, never overwritten: the caller zeroes the buffer and an epoch accumulates on the device.  Bins
 *     of columns outside every segment stay as they are.
 * One launch: 16 lanes per row stage the row's covered columns in LDS and reduce every segment (max, then the lowest index
 * among the equal maxima); the counters go through a per-workgroup int32 histogram in LDS, whose non-zero bins are added to
 * `counts` with 64-bit integer atomics — integer sums do not depend on order: bitwise reproducible.  The staged rows and the
 * histogram share 64 KiB of LDS: n_cols <= AGNN_EVAL_MAX_COLS, AGNN_EINVAL beyond.  AGNN_EINVAL also for NULL logits /
 * seg_off, pred and counts both NULL, counts without labels, n_tasks outside [1, AGNN_MAX_SEG], n_rows < 0, n_cols < 1 or
 * > ld, gate_task outside [-1, n_tasks), group_mask bits at or above n_tasks; AGNN_EALIGN for counts off 8 bytes.
 * n_rows == 0: success, no pointer is looked at.
 * ------------------------------------------------------------------------------------------ */
#define AGNN_EVAL_MAX_COLS 800
size_t agnn_eval_counts_len(int32_t n_tasks, int32_t n_cols);
int agnn_multitask_eval_f32(const float* logits, int64_t ld, const int32_t* seg_off, const int32_t* seg_end, int32_t n_tasks,
                            int32_t n_cols, const int64_t* labels, int64_t n_rows, int64_t ignore_index,
                            const uint8_t* row_mask, int32_t gate_task, uint32_t group_mask, int32_t* pred, int64_t* counts,
                            agnn_stream_t stream);

/* ------------------------------------------------------------------------------------------
 * JumpingKnowledge (ref: models/core/gnn.py:345-365) — a bidirectional LSTM over the T layer outputs of every row, an attention
 * score per layer, a softmax over the layers and the weighted sum of the layer outputs.  fp32, no atomics: every cross-tile sum
 * goes through a partials buffer summed in a fixed order (two runs give the same bits).  analysisgnn_amd/jk.py orders the calls.
 *
 * agnn_lstm_step_f32: ONE time step of one or two directions (n_items <= 2, same M, K0, h, both first steps or both later ones):
 *     g = x[M, K0] W_ih[4h, K0]^T + hprev[M, h] W_hh[4h, h]^T + b_ih + b_hh      (gate order i, f, g, o: PyTorch's row blocks)
 *     cout = sigmoid(f) cprev + sigmoid(i) tanh(g) ,   hout = sigmoid(o) tanh(cout)
 *   on the tile of agnn_gemm_nt2_f32 with the cell in its epilogue.  The weights and biases are contiguous and read where they
 *   lie.  hprev == NULL: the first step (h = c = 0; no recurrent product, cprev not read).  act != NULL: the post-nonlinearity
 *   gates act[M, 4h] (ld 4h) are written for the backward.  att_w != NULL (this direction's h entries of att.weight):
 *   part[m, j] = sum_{u in [32 j, 32 j + 32)} att_w[u] hout[m, u], part [M, h / 32] contiguous.
 *   K0 % 16 == 0, h % 32 == 0; x, hprev and the weights 16-byte aligned with ld % 4 == 0.
 * agnn_jk_combine_fwd_f32: score[m, t] = sum_d sum_j part[d][t][m][j] (part [n_dir, T, M, n_tiles], summed in that order),
 *   alpha[m, :] = softmax_t(score) (written, [M, T]), out[m, :] = sum_t alpha[m, t] x_t[m, :].  The T <= AGNN_JK_MAX_T inputs are
 *   read through a host list of pointers with their leading dimensions.  att.bias shifts every score of a row alike and cancels
 *   in the softmax: it is not an argument.
 * agnn_jk_combine_bwd_f32: dalpha_t = dout . x_t, dscore[m, t] = alpha_t (dalpha_t - sum_s alpha_s dalpha_s) ([M, T]), and the
 *   direct term dx_t = alpha_t dout into dxs[t].
 * agnn_lstm_cell_bwd_f32: the pointwise backward of one step (1 - 2 items).  dh = dh (NULL at the last step) + dscore[m] att_w
 *   (rank one, never materialised), dc = dc_next (NULL at the last step) + dh o (1 - tanh^2 c); dgates[M, 4h] (pre-activation,
 *   ld 4h) and dc_prev = dc f (NULL: not wanted); cprev == NULL at the first step (c_{-1} = 0).  wpart[b, u] = sum over the rows
 *   of row block b (agnn_lstm_cell_bwd_row_blocks(M) blocks) of dscore[m] h[m, u] with h = o tanh(c) recomputed: the partials of
 *   att.weight's gradient, summed by agnn_colsum_parts_f32 (out[c] = sum_r parts[r, c], fixed order).  h % 4 == 0, 16-byte
 *   aligned operands.
 * ------------------------------------------------------------------------------------------ */
#define AGNN_JK_MAX_T 8
typedef struct {
  const float* x;       int64_t ld_x;
  const float* hprev;   int64_t ld_hprev;
  const float* cprev;   int64_t ld_cprev;
  const float* w_ih;    /* [4h, K0] */
  const float* w_hh;    /* [4h, h] */
  const float* b_ih;    /* [4h] */
  const float* b_hh;    /* [4h] */
  float* hout;          int64_t ld_hout;
  float* cout;          int64_t ld_cout;
  float* act;           /* [M, 4h] or NULL */
  const float* att_w;   /* [h] or NULL */
  float* part;          /* [M, h / 32] */
  int64_t M;
  int32_t K0, h;
} agnn_lstm_step_t;
int agnn_lstm_step_f32(int32_t n_items, const agnn_lstm_step_t* items /* (host) */, agnn_stream_t stream);
int agnn_jk_combine_fwd_f32(int32_t T, const float* const* xs /* (host) */, const int64_t* ld_xs /* (host) */, int64_t M, int32_t H,
                            const float* part, int32_t n_dir, int32_t n_tiles, float* alpha, float* out, int64_t ld_out,
                            agnn_stream_t stream);
int agnn_jk_combine_bwd_f32(int32_t T, const float* const* xs /* (host) */, const int64_t* ld_xs /* (host) */, int64_t M, int32_t H,
                            const float* alpha, const float* dout, int64_t ld_dout, float* dscore, float* const* dxs /* (host) */,
                            const int64_t* ld_dxs /* (host) */, agnn_stream_t stream);
typedef struct {
  const float* act;      /* [M, 4h] */
  const float* c;        int64_t ld_c;
  const float* cprev;    int64_t ld_cprev;
  const float* dh;       int64_t ld_dh;
  const float* dc_next;  int64_t ld_dc_next;
  const float* dscore;   int64_t ld_dscore;     /* dscore[m * ld_dscore] */
  const float* att_w;    /* [h] */
  float* dgates;         /* [M, 4h] */
  float* dc_prev;        int64_t ld_dc_prev;
  float* wpart;          /* [row blocks, h] */
  int64_t M;
  int32_t h;
} agnn_lstm_cell_bwd_t;
int64_t agnn_lstm_cell_bwd_row_blocks(int64_t M);
int agnn_lstm_cell_bwd_f32(int32_t n_items, const agnn_lstm_cell_bwd_t* items /* (host) */, agnn_stream_t stream);
int agnn_colsum_parts_f32(const float* parts, int64_t n_rows, int32_t n_cols, float* out, agnn_stream_t stream);

/* ------------------------------------------------------------------------------------------
 * Dense multi-head self-attention over the N rows of a batch (ref: nn.MultiheadAttention as GPSLayer / HGPSLayer call it,
 * models/core/gnn.py:471, core/hgnn.py:273: one unbatched sequence, no mask), exact fp32, flash style: nothing of size N x N
 * is written.  q, k, v: [N, heads D] column blocks with ONE row stride ld_qkv (the three blocks of the in-projection's
 * [N, 3E] output where they lie).  D in {8, 16, 32, 64}, heads >= 1, N >= 1; anything else is AGNN_EINVAL before any HIP call.
 * All rows 16-byte aligned (AGNN_EALIGN).  q_rows: query rows per workgroup, 0 (chosen from N and heads), 64 or 128.
 *
 * agnn_attn_fwd_f32:  P = softmax(scale q k^T) per head, o = (P o keep) v with the heads side by side ([N, heads D], ld_o),
 *   lse[heads, N] = log sum exp of the scaled scores.  Dropout p acts on the normalised probabilities as torch's does: keep is
 *   0 or 1 / (1 - p), drawn by the project's counter-based generator from (rng_state[0] = seed, rng_state[1] = step, call_id);
 *   one draw serves keys 4g .. 4g + 3 of a query row, its counter is the 64-bit element index (head N + query) N + 4g.
 *   With p > 0 the (seed, step) read is copied to rng_used (device int64[2]) for the backward.  p == 0: neither is touched.
 * agnn_attn_bwd_f32:  dq, dk, dv ([N, heads D] column blocks with one row stride ld_dqkv: the in-projection's dY) from dO, o,
 *   lse and the forward's inputs; P is recomputed; rng_used is the forward's.  dq is formed in a pass of its own over the query
 *   rows (S is computed twice): no atomics, no workgroup waits for another, and two runs give the same bits.
 *   workspace: agnn_attn_bwd_workspace_bytes(N, heads) bytes, 16-byte aligned (the row sums of dO o o).
 * agnn_attn_dropout_keep_f32:  the keep factors of (rng, call_id) as a dense [heads, N, N] matrix (all ones at p == 0), by the
 *   device function the two kernels use: for inspection and tests, N <= 8192.
 * ------------------------------------------------------------------------------------------ */
int agnn_attn_fwd_f32(const float* q, const float* k, const float* v, int64_t ld_qkv, int64_t N, int32_t heads, int32_t D, float scale,
                      float p, const int64_t* rng_state, uint32_t call_id, int32_t q_rows, float* o, int64_t ld_o, float* lse,
                      int64_t* rng_used, agnn_stream_t stream);
size_t agnn_attn_bwd_workspace_bytes(int64_t N, int32_t heads);
int agnn_attn_bwd_f32(const float* q, const float* k, const float* v, int64_t ld_qkv, int64_t N, int32_t heads, int32_t D, float scale,
                      float p, const int64_t* rng_used, uint32_t call_id, int32_t q_rows, const float* dO, int64_t ld_do,
                      const float* o, int64_t ld_o, const float* lse, float* dq, float* dk, float* dv, int64_t ld_dqkv,
                      void* workspace, size_t workspace_bytes, agnn_stream_t stream);
int agnn_attn_dropout_keep_f32(int64_t N, int32_t heads, float p, const int64_t* rng, uint32_t call_id, float* keep,
                               agnn_stream_t stream);

/* ------------------------------------------------------------------------------------------
 * Cross-task attention of the logit-fusion block (ref: CrossTaskTransformer, models/analysis.py:408-418): n_seq independent
 * sequences of T tokens, exact fp32, one lane per (sequence, head, row); nothing of size n_seq x heads x T x T is written.
 * qkv: the packed in-projection [n_seq T, 3E] with row stride ld_qkv, row n T + t = token t of sequence n, columns q | k | v,
 * head h in columns h D .. h D + D - 1 of each block (E = heads D).  o: [n_seq T, E], the heads side by side.  dqkv: [n_seq T, 3E],
 * written completely.  D in {8, 16, 32}, 1 <= T <= AGNN_MAX_SEG, heads >= 1 with heads D <= 128 and heads T <= 256, n_seq >= 0,
 * p in [0, 1): anything else is AGNN_EINVAL before any HIP call, as are NULL pointers, leading dimensions below 3E (E for o / dO)
 * and p > 0 without its state; a pointer off 16 bytes or a leading dimension that is no multiple of 4 floats is AGNN_EALIGN.
 * n_seq == 0 returns AGNN_OK and looks at no pointer.
 *
 * agnn_taskattn_fwd_f32:  P = softmax(scale q k^T) over the T keys per (sequence, head), o = (P o keep) v.  lse (optional, NULL:
 *   not written): [n_seq T, heads], log2 of the sum of exp2 of the scores in log2 units (scale log2(e) q k^T): what the backward
 *   reads.  Dropout p acts on the normalised probabilities as torch's does: keep is 0 or 1 / (1 - p), drawn by the project's
 *   counter-based generator from (rng_state[0] = seed, rng_state[1] = step, call_id); one draw serves keys 4g .. 4g + 3 of a
 *   query row, its counter is the element index ((n heads + h) 32 + i) 32 + 4g.  With p > 0 the (seed, step) read is copied to
 *   rng_used (device int64[2]); at p == 0 nothing is drawn and neither is touched (both may be NULL).
 * agnn_taskattn_bwd_f32:  dqkv from dO, the forward's qkv, o and lse; P is recomputed (twice: once query-major for dq, once
 *   key-major for dk and dv), the masks are redrawn from rng_used.  No atomics; two runs give the same bits.
 * agnn_taskattn_dropout_keep_f32:  the keep factors of (rng, call_id) as a dense [n_seq, heads, T, T] tensor (all ones at
 *   p == 0), by the device function the two kernels use: for inspection and tests.
 * ------------------------------------------------------------------------------------------ */
int agnn_taskattn_fwd_f32(const float* qkv, int64_t ld_qkv, int64_t n_seq, int32_t T, int32_t heads, int32_t D, float scale, float p,
                          const int64_t* rng_state, uint32_t call_id, float* o, int64_t ld_o, float* lse, int64_t* rng_used,
                          agnn_stream_t stream);
int agnn_taskattn_bwd_f32(const float* qkv, int64_t ld_qkv, int64_t n_seq, int32_t T, int32_t heads, int32_t D, float scale, float p,
                          const int64_t* rng_used, uint32_t call_id, const float* dO, int64_t ld_do, const float* o, int64_t ld_o,
                          const float* lse, float* dqkv, int64_t ld_dqkv, agnn_stream_t stream);
int agnn_taskattn_dropout_keep_f32(int64_t n_seq, int32_t T, int32_t heads, float p, const int64_t* rng, uint32_t call_id,
                                   float* keep /* [n_seq, heads, T, T] */, agnn_stream_t stream);

/* ------------------------------------------------------------------------------------------
 * SMOTE oversampling of the minority classes and the nearest-original search of its feature penalty (ref:
 * models/cadence.py:13-118 `SMOTE`, models/analysis.py:1412-1438 `update_feature_loss`; csrc/smote.hip).
 * D % 4 == 0 and 4 <= D <= 512, rows 16-byte aligned, leading dimensions multiples of 4 floats: AGNN_EINVAL / AGNN_EALIGN
 * before any HIP call otherwise, as for NULL pointers.  No float atomics: two runs give the same bits.
 *
 * agnn_rowsel_f32:  for every query row the ksel (1 .. AGNN_ROWSEL_MAX_K) smallest scores among the candidate rows of its own
 *   segment, ascending, ties to the lower index.  Query p of segment s (q_off[s] <= p < q_off[s + 1], HOST arrays of
 *   n_seg + 1 <= AGNN_MAX_SEG + 1 ascending offsets, read during the call) is row q_rows[p] of q (p itself with q_rows NULL);
 *   candidates likewise from c, c_rows, c_off.  q_n / c_n: rows of q / c; a row index outside them makes the row NaN, and a NaN
 *   score is never selected.  Scores: AGNN_ROWSEL_COSINE  q.c / (max(|q|, 1e-12) max(|c|, 1e-12))  (the similarity of
 *   F.normalize'd rows; the SMALLEST similarities are selected), AGNN_ROWSEL_SQDIST  sum (q - c)^2  summed from the differences.
 *   idx [Q, ksel] holds candidate POSITIONS (p in c_off's numbering, so inside the query's segment) or -1, score [Q, ksel] the
 *   scores or +inf, where the segment has fewer than ksel candidates.  Nothing of size queries x candidates is written.
 * agnn_smote_synth_fwd_f32:  x_over [N + S, D] = x, then the synthetic rows; y_over [N + S] likewise (optional).  The plan
 *   (HOST, read during the call) lists the oversampled classes in output order: class i owns the class-sorted positions
 *   t_off[i] .. t_off[i + 1] - 1, makes `copies[i]` >= 1 rows per original and writes them at s_off[i] + j copies[i] + n with label
 *   label[i].  rows [T] maps a class-sorted position to its row of x, nbr [T, ld_nbr] is agnn_rowsel_f32's idx with
 *   ksel >= k: rank 0 is dropped and rank 1 + choice used.  Synthetic row s = x_i + gap[s] o (x_nb - x_i), choice[s] in
 *   [0, k - 2], gap [S, D]: both given, or both NULL and drawn from (rng, call_id) — the state is copied to rng_used for the
 *   backward.  nb_row [S] (optional) receives the neighbour's row of x.  2 <= k < AGNN_ROWSEL_MAX_K.
 * agnn_smote_synth_bwd_f32:  g = d x_over [N + S, D]; dx [N, D] must hold g's head on entry and receives
 *   dx[rows[p]] += sum_n (1 - gap) o g[N + s] over the position's consecutive synthetic rows; w [S, D] = gap o g[N + s], the
 *   addend of the neighbour's row (summed by agnn_spmm_f32 over a CSR by nb_row).  gap as in the forward, or NULL with rng_used.
 * agnn_smote_draws_f32:  the draws of (rng, call_id) for S rows by the device functions the two kernels use.
 * ------------------------------------------------------------------------------------------ */
#define AGNN_ROWSEL_MAX_K  8
#define AGNN_ROWSEL_COSINE 0
#define AGNN_ROWSEL_SQDIST 1
typedef struct {
  int32_t n_seg;
  int32_t t_off[AGNN_MAX_SEG + 1];
  int32_t s_off[AGNN_MAX_SEG + 1];
  int32_t copies[AGNN_MAX_SEG];
  int64_t label[AGNN_MAX_SEG];
} agnn_smote_plan_t;
int agnn_rowsel_f32(const float* q, int64_t ld_q, const int32_t* q_rows, int64_t q_n, const float* c, int64_t ld_c,
                    const int32_t* c_rows, int64_t c_n, int32_t n_seg, const int32_t* q_off /* (host) */,
                    const int32_t* c_off /* (host) */, int32_t D, int32_t ksel, int32_t mode, int32_t* idx, float* score,
                    agnn_stream_t stream);
int agnn_smote_synth_fwd_f32(const float* x, int64_t ld_x, const int64_t* y, int64_t N, int32_t D, const agnn_smote_plan_t* plan,
                             const int32_t* rows, const int32_t* nbr, int32_t ld_nbr, int32_t k, const int32_t* choice,
                             const float* gap, const int64_t* rng, uint32_t call_id, float* x_over, int64_t ld_over,
                             int64_t* y_over, int32_t* nb_row, int64_t* rng_used, agnn_stream_t stream);
int agnn_smote_synth_bwd_f32(const float* g, int64_t ld_g, int64_t N, int32_t D, const agnn_smote_plan_t* plan, const int32_t* rows,
                             const float* gap, const int64_t* rng_used, uint32_t call_id, float* dx, int64_t ld_dx, float* w,
                             int64_t ld_w, agnn_stream_t stream);
int agnn_smote_draws_f32(int64_t S, int32_t D, int32_t k, const int64_t* rng, uint32_t call_id, int32_t* choice, float* gap,
                         agnn_stream_t stream);

/* ------------------------------------------------------------------------------------------
 * Link prediction of the pretraining stage (ref: models/analysis.py:360-406 `PreEncoder`, :697-744 `PreEncoderPL._common_step`;
 * csrc/linkpred.hip): candidate edges scored by the dot product of their endpoint rows, BCEWithLogitsLoss against membership in
 * a true relation.  One call serves a table (HOST, read during the call) of at most AGNN_MAX_SEG tasks with their own features,
 * candidates and true relations; H is shared.  H % 4 == 0, rows 16-byte aligned, leading dimensions multiples of 4 floats:
 * AGNN_EINVAL / AGNN_EALIGN before any HIP call otherwise, as for NULL pointers, negative sizes and limit > n.  No float
 * atomics; two runs give the same bits.
 *
 * agnn_link_bce_fwd_f32:  for candidate e = (src[e], dst[e]) (int64, rows 0 and 1 of a PyG edge_index) of a task
 *     alive_e = 0 <= src, dst < limit         (limit <= n: the batch's target rows; the reference's mask compactions :712-717)
 *     logit_e = <z[src], z[dst]>              label_e = 1 iff dst occurs in row src of the true relation's by-source CSR
 *     loss_e  = max(x, 0) - x y + log1p(exp(-|x|))                 g_e = sigmoid(x) - y
 *   (t_rowptr: n + 1 offsets into t_col, as agnn_csr_build lays them out; duplicate true edges are harmless).  A candidate that
 *   is not alive reads no row and gets logit 0, label 0, g 0.  Per task: loss[0] = sum of loss_e / alive count, inv_cnt[0] =
 *   1 / alive count, counts[5] = alive, tp, fp, fn, tn with "predicted positive" = logit > 0.  A task without an alive candidate
 *   gets loss 0 and inv_cnt 0 (torch's BCEWithLogitsLoss over nothing: NaN).  The loss is summed per tile of 64 candidates into
 *   the workspace (agnn_link_bce_workspace_bytes) and the tiles by one workgroup per task, both in a fixed order.  Tasks with
 *   E == 0 look at no candidate pointer.
 * agnn_link_bce_bwd_f32:  dz[i] = scale[task] (sum_{e: src_e = i} g_e z[dst_e] + sum_{e: dst_e = i} g_e z[src_e]) for every row
 *   i < n, from the candidate list's CSR by source (s_*: col = destination) and by destination (d_*: col = source), perm = the
 *   candidate's position (agnn_csr_build).  scale: (device) one float per task, the incoming gradient times inv_cnt.  Every row
 *   of dz is written exactly once (rows without a candidate: zeros); a self loop lies in both CSRs and contributes 2 g_e z[i].
 *   Entries whose col or perm is out of range are skipped.
 * ------------------------------------------------------------------------------------------ */
typedef struct {
  const float* z;          /* (device) [n, H], row stride ld_z */
  int64_t ld_z;
  int64_t n;
  const int64_t* src;      /* (device) [E] */
  const int64_t* dst;      /* (device) [E] */
  int64_t E;
  int64_t limit;
  const int32_t* t_rowptr; /* (device) [n + 1] */
  const int32_t* t_col;    /* (device) */
  float* logit;            /* (device) [E] */
  uint8_t* label;          /* (device) [E] */
  float* g;                /* (device) [E] */
  float* loss;             /* (device) [1] */
  float* inv_cnt;          /* (device) [1] */
  int32_t* counts;         /* (device) [5] */
} agnn_link_task_t;
typedef struct {
  const float* z;          /* (device) [n, H], row stride ld_z */
  int64_t ld_z;
  int64_t n;
  const float* g;          /* (device) [E] */
  int64_t E;
  const int32_t* s_rowptr; /* (device) [n + 1] */
  const int32_t* s_col;
  const int32_t* s_perm;
  const int32_t* d_rowptr; /* (device) [n + 1] */
  const int32_t* d_col;
  const int32_t* d_perm;
  float* dz;               /* (device) [n, H], row stride ld_dz */
  int64_t ld_dz;
} agnn_link_bwd_t;
size_t agnn_link_bce_workspace_bytes(int32_t n_tasks, const agnn_link_task_t* tasks);
int agnn_link_bce_fwd_f32(int32_t n_tasks, const agnn_link_task_t* tasks, int32_t H, void* workspace, size_t workspace_bytes,
                          agnn_stream_t stream);
int agnn_link_bce_bwd_f32(int32_t n_tasks, const agnn_link_bwd_t* tasks, int32_t H, const float* scale, agnn_stream_t stream);

/* ------------------------------------------------------------------------------------------
 * Edge-consistency term of the continual trainer (ref: models/analysis.py:805-836 `EdgeDecoder`, :986-1019; csrc/edgedec.hip):
 * for every note-note relation r the selected edges e = (s, d) are classified "all label rows agree at s and d" from the product
 * of the two ends' embeddings.  `embed[r]` is row-wise up to its dropout, so A_r = LN(ReLU(x W_r^T + b_r)) is computed once per
 * node (a column block of a stacked [n, R H] matrix, its own leading dimension) and the dropout is applied per (edge, end, column)
 * inside the pair kernel.  One call serves a table (HOST, read during the call) of at most AGNN_MAX_SEG relations; H is shared.
 * H % 4 == 0, 4 <= H <= 512, rows 16-byte aligned, leading dimensions multiples of 4 floats: AGNN_EINVAL / AGNN_EALIGN before
 * any HIP call otherwise, as for NULL pointers, negative sizes and limit > n.  No float atomics; two runs give the same bits.
 * An edge is ALIVE when 0 <= src, dst < limit (limit <= n; an unselected edge carries ids outside that range: edge_loss.edge_plan).
 * `pos0` is the global position of the relation's first edge: the masks are indexed by pos0 + e.
 *
 * agnn_edge_select_keys:  key[e] = (word << 31) | e for an alive edge, word = the first word of the random stream at index
 *   pos0 + e (E < 2^31: the keys of a relation are distinct), INT64_MAX otherwise: the k smallest keys are a uniform k-subset.
 * agnn_edge_pair_fwd_f32:  f[e, :] = m1 * a[src, :] * m2 * a[dst, :], m1 / m2 keep factors 0 or 1 / (1 - p) of end 0 / 1:
 *   columns 4 q .. 4 q + 3 take the four words of the stream at index ((pos0 + e) 2 + end) (H / 4) + q.  p == 0: no bits are
 *   drawn, rng_state may be NULL.  label[e] = 1 iff labels[k, src] == labels[k, dst] for all K rows of `labels` (int64 [K, >=
 *   limit], row stride ld_labels; equal -1s are equal; labels == NULL or K == 0: label 0).  An edge that is not alive reads no
 *   row: f row zero, label 0.  With p > 0 the (seed, step) read is copied to rng_used (device int64[2]) for the backward.
 * agnn_edge_pair_bwd_f32:  da[i, :] = sum_{e: src_e = i} df[e] * m1 m2 * a[dst_e] + sum_{e: dst_e = i} df[e] * m1 m2 * a[src_e]
 *   for every row i < n, from the edge list's CSR by source (s_*: col = destination) and by destination (d_*: col = source),
 *   perm = the edge's position (agnn_csr_build).  Every row of da is written exactly once (rows without an alive edge: zeros); a
 *   self loop lies in both CSRs and contributes twice.  Entries whose col or perm is out of range, and rows >= limit, add nothing.
 * agnn_edge_ce_fwd_f32:  per alive edge the two logits y[e] . w4[c] + b4[c] (w4 [2, H] dense, 16-byte aligned), the
 *   label-smoothed two-class cross entropy  -sum_c q_c log softmax_c, q = (1 - smoothing) onehot(label) + smoothing / 2, and its
 *   finished coefficient dlogit[e, c] = softmax_c - q_c; edges that are not alive read no row and get logits 0, dlogit 0.  Per
 *   relation: loss[0] = sum / alive count, inv_cnt[0] = 1 / alive count, counts[5] = alive, tp, fp, fn, tn with "predicted
 *   positive" = logit 1 > logit 0; a relation without an alive edge gets loss 0 and inv_cnt 0 (torch: NaN).  total[0] = (sum of
 *   the relations' losses) / n_rel.  The loss is summed per tile of 64 edges into the workspace (agnn_edge_ce_workspace_bytes)
 *   and the tiles by a second kernel, both in a fixed order.
 * agnn_edge_ce_bwd_f32:  dy[e, :] = scale[r] (dlogit[e, 0] w4[0, :] + dlogit[e, 1] w4[1, :]) for every edge (zeros where not
 *   alive), dw4[c, :] = sum_e scale[r] dlogit[e, c] y[e, :], db4[c] = sum_e scale[r] dlogit[e, c] as fixed-order partials in the
 *   workspace (agnn_edge_ce_bwd_workspace_bytes) plus one reduction.  scale: (device) one float per relation.
 * ------------------------------------------------------------------------------------------ */
typedef struct {
  const int64_t* src;      /* (device) [E] */
  const int64_t* dst;      /* (device) [E] */
  int64_t E;
  int64_t limit;
  int64_t pos0;
  int64_t* key;            /* (device) [E] */
} agnn_edge_keys_t;
typedef struct {
  const float* a;          /* (device) [n, H], row stride ld_a */
  int64_t ld_a;
  int64_t n;
  const int64_t* src;      /* (device) [E] */
  const int64_t* dst;      /* (device) [E] */
  int64_t E;
  int64_t limit;
  int64_t pos0;
  float* f;                /* (device) [E, H], row stride ld_f */
  int64_t ld_f;
  uint8_t* label;          /* (device) [E] */
} agnn_edge_pair_t;
typedef struct {
  const float* a;          /* (device) [n, H], row stride ld_a */
  int64_t ld_a;
  int64_t n;
  const float* df;         /* (device) [E, H], row stride ld_df */
  int64_t ld_df;
  int64_t E;
  int64_t limit;
  int64_t pos0;
  const int32_t* s_rowptr; /* (device) [n + 1] */
  const int32_t* s_col;
  const int32_t* s_perm;
  const int32_t* d_rowptr; /* (device) [n + 1] */
  const int32_t* d_col;
  const int32_t* d_perm;
  float* da;               /* (device) [n, H], row stride ld_da */
  int64_t ld_da;
} agnn_edge_pair_bwd_t;
typedef struct {
  const float* y;          /* (device) [E, H], row stride ld_y */
  int64_t ld_y;
  const int64_t* src;      /* (device) [E] */
  const int64_t* dst;      /* (device) [E] */
  const uint8_t* label;    /* (device) [E] */
  int64_t E;
  int64_t limit;
  float* logit;            /* (device) [E, 2] */
  float* dlogit;           /* (device) [E, 2] */
  float* loss;             /* (device) [1] */
  float* inv_cnt;          /* (device) [1] */
  int32_t* counts;         /* (device) [5] */
} agnn_edge_ce_t;
typedef struct {
  const float* y;          /* (device) [E, H], row stride ld_y */
  int64_t ld_y;
  const float* dlogit;     /* (device) [E, 2] */
  int64_t E;
  float* dy;               /* (device) [E, H], row stride ld_dy */
  int64_t ld_dy;
} agnn_edge_ce_bwd_t;
int agnn_edge_select_keys(int32_t n_rel, const agnn_edge_keys_t* rels, const int64_t* rng_state, uint32_t call_id,
                          agnn_stream_t stream);
int agnn_edge_pair_fwd_f32(int32_t n_rel, const agnn_edge_pair_t* rels, int32_t H, const int64_t* labels, int32_t K,
                           int64_t ld_labels, float p, const int64_t* rng_state, uint32_t call_id, int64_t* rng_used,
                           agnn_stream_t stream);
int agnn_edge_pair_bwd_f32(int32_t n_rel, const agnn_edge_pair_bwd_t* rels, int32_t H, float p, const int64_t* rng_state,
                           uint32_t call_id, agnn_stream_t stream);
size_t agnn_edge_ce_workspace_bytes(int32_t n_rel, const agnn_edge_ce_t* rels);
int agnn_edge_ce_fwd_f32(int32_t n_rel, const agnn_edge_ce_t* rels, int32_t H, const float* w4, const float* b4, float smoothing,
                         float* total, void* workspace, size_t workspace_bytes, agnn_stream_t stream);
size_t agnn_edge_ce_bwd_workspace_bytes(int32_t n_rel, const agnn_edge_ce_bwd_t* rels, int32_t H);
int agnn_edge_ce_bwd_f32(int32_t n_rel, const agnn_edge_ce_bwd_t* rels, int32_t H, const float* w4, const float* scale,
                         float* dw4, float* db4, void* workspace, size_t workspace_bytes, agnn_stream_t stream);

/* ------------------------------------------------------------------------------------------
 * Score graph construction (ref: utils/hgraph.py:214-300 `hetero_graph_from_note_array`; csrc/scoregraph.hip): the note arrays of
 * one or many scores, concatenated on the device — onset_div / duration_div int64 [n_notes], score_start int32 [n_scores + 1] —
 * become the four note relations as int64 COO with GLOBAL note ids.  Inside a score onsets are non-decreasing, and
 * 0 <= onset, 0 <= duration, onset + duration < 2^31.  With end = onset + duration and lb / ub the lower / upper bound inside the
 * score's slice, source i reaches
 *   relation 0 onset        [lb(onset_i), ub(onset_i)), i itself only with AGNN_SG_SELF_LOOPS
 *   relation 1 consecutive  [lb(end_i), ub(end_i))
 *   relation 2 during       [ub(onset_i), max(ub(onset_i), lb(end_i)))
 *   relation 3 rest         when no note of the score starts at end_i and a later onset exists: the onset group of the first one
 * Edges are source-major with destinations ascending; rest takes its sources in stable order of end: (end, source, destination).
 * edges[r] is int64 [2, cap[r]] (row 0 sources, row 1 destinations), or [3, cap[r]] when bit r of rev_mask is set: row 2 repeats
 * row 0, so that rows 1 .. 2 are the reverse relation without a copy.  Slots past the real count hold -1 (what agnn_csr_build
 * drops).  totals (device int64[4]) receives the real counts, note_score (device int64[n_notes], may be NULL) every note's score.
 * faults (device int32[AGNN_SG_FAULT_WORDS], caller-owned, zeroed by the caller, only ever incremented) COUNTS bad input, one word
 * per kind: an onset that decreases inside a score, a value outside the range above, a score_start that does not tile
 * [0, n_notes), per relation an edge count over its capacity, more groups than capacity (agnn_score_groups).  A score with a
 * fault gets no edge, a bad score_start leaves every score without edges, an overflowing relation is cut at its capacity; nothing
 * is written out of range in any of these cases and the agnn_check_status word is not involved.
 * agnn_score_graph_count does everything up to the totals and leaves the runs in the workspace; agnn_score_graph_fill writes the
 * edges from that workspace (same g apart from edges / cap / rev_mask); agnn_score_graph_build is both.  Stream-ordered, no host
 * read.  n_scores < 1, n_notes < 1, NULL pointers, negative capacities: AGNN_EINVAL; a workspace below
 * agnn_score_graph_workspace_bytes: AGNN_ENOMEM.
 *
 * agnn_score_groups: metrical nodes.  key (int64 [n_notes], taken as floor(key / div), non-decreasing inside a score) -> a compact
 * group id per note, global over the scores: a note opens a group when it starts a score or its key differs from its
 * predecessor's.  note_edge int64 [2 (3 with rev), n_notes] = (note, group); per group < cap its score, its first note and, with
 * parent_edge (int64 [2 (3 with rev), cap]), the pair (group, parent_of[first note]) — beat -> measure with parent_of = row 1 of
 * the measures' note_edge; padding groups hold -1.  per_score (int64 [n_scores]) and total (int64 [1]) receive the group counts.
 * A decreasing key is counted in faults[AGNN_SG_FAULT_ORDER] (it still only opens a group).
 * ------------------------------------------------------------------------------------------ */
#define AGNN_SG_SELF_LOOPS     1u
#define AGNN_SG_FAULT_ORDER    0
#define AGNN_SG_FAULT_RANGE    1
#define AGNN_SG_FAULT_SCORES   2
#define AGNN_SG_FAULT_OVERFLOW 3   /* + relation: words 3 .. 6 */
#define AGNN_SG_FAULT_GROUPS   7
#define AGNN_SG_FAULT_WORDS    8
typedef struct {
  const int64_t* onset_div;      /* (device) [n_notes] */
  const int64_t* duration_div;   /* (device) [n_notes] */
  const int32_t* score_start;    /* (device) [n_scores + 1] */
  int64_t n_notes;
  int32_t n_scores;
  uint32_t flags;                /* AGNN_SG_SELF_LOOPS */
  uint32_t rev_mask;
  int64_t* edges[4];             /* (device) out int64 [2 or 3, cap[r]] */
  int64_t cap[4];
  int64_t* totals;               /* (device) out int64[4] */
  int64_t* note_score;           /* (device) out int64[n_notes] or NULL */
  int32_t* faults;               /* (device) int32[AGNN_SG_FAULT_WORDS] */
} agnn_score_graph_t;
typedef struct {
  const int64_t* key;            /* (device) [n_notes] */
  int64_t div;
  const int32_t* score_start;    /* (device) [n_scores + 1] */
  int64_t n_notes;
  int32_t n_scores;
  int32_t rev;
  const int64_t* parent_of;      /* (device) [n_notes] or NULL */
  int64_t* note_edge;            /* (device) out int64 [2 or 3, n_notes] */
  int64_t cap;
  int64_t* group_score;          /* (device) out int64[cap] or NULL */
  int64_t* group_first;          /* (device) out int64[cap] or NULL */
  int64_t* parent_edge;          /* (device) out int64 [2 or 3, cap] or NULL */
  int64_t* per_score;            /* (device) out int64[n_scores] or NULL */
  int64_t* total;                /* (device) out int64[1] or NULL */
  int32_t* faults;               /* (device) int32[AGNN_SG_FAULT_WORDS] */
} agnn_score_groups_t;
size_t agnn_score_graph_workspace_bytes(int64_t n_notes, int32_t n_scores);
int agnn_score_graph_count(const agnn_score_graph_t* g /* (host) */, void* workspace, size_t workspace_bytes, agnn_stream_t stream);
int agnn_score_graph_fill(const agnn_score_graph_t* g /* (host) */, void* workspace, size_t workspace_bytes, agnn_stream_t stream);
int agnn_score_graph_build(const agnn_score_graph_t* g /* (host) */, void* workspace, size_t workspace_bytes, agnn_stream_t stream);
size_t agnn_score_groups_workspace_bytes(int64_t n_notes);
int agnn_score_groups(const agnn_score_groups_t* g /* (host) */, void* workspace, size_t workspace_bytes, agnn_stream_t stream);

/* ------------------------------------------------------------------------------------------
 * Note descriptors (ref: descriptors/general.py:110-139 `select_features`, descriptors/utils/note_features.py:176-226
 * `get_voice_separation_features`, descriptors/utils/cadence_features.py:6-119 `get_cad_features`; csrc/notefeat.hip): the note
 * array of one or many scores, concatenated on the device, becomes x (fp32 [n_notes, 25 | 56], row stride ld_x), the rows that
 * `in_channels` counts.  Inside a score the notes are in (onset, pitch) order, as for agnn_score_graph_*, and onset_beat does not
 * decrease where onset_div does not; nothing is reordered.
 *   AGNN_NF_VOICE    25 columns: 1 - tanh(duration_beat / ts_beats); remainder(onset_beat, ts_beats) / ts_beats (the remainder
 *                    has the divisor's sign); remainder(onset_beat, 1) == 0; one-hot of pitch % 12; one-hot of pitch / 12 (10)
 *   AGNN_NF_CADENCE  those 25, then the 31 columns of get_cad_features(include_pitch_spelling=False), in its order (DESIGN.md,
 *                    "Note descriptors").  Needs voice and is_downbeat; a non-zero is_downbeat is written as 1.
 * is_note_onset may be NULL (all ones), as the reference appends the field when it is absent.
 * faults (device int32[AGNN_NF_FAULT_WORDS], caller-owned, zeroed by the caller, only ever incremented) COUNTS bad input, one
 * word per kind and one count per offending note: pitch outside [0, 120) (the reference raises), ts_beats <= 0, voice outside
 * [0, 2^15) (where voice is given), an onset_div below its predecessor's inside a score; and ONE count when score_start does not
 * tile [0, n_notes).  An offending note's row is zeros and the note is left out of every chord, window and voice list, so the
 * other rows are those of the array without it (where what is left is in onset order; otherwise they are unspecified).  A bad
 * score_start zeroes every row.  No read leaves the score's slice and no write leaves x's rows in any of these cases; the
 * agnn_check_status word is not involved.
 * Stream-ordered, no host read, no allocation, integer atomics only (bitwise reproducible), capturable.  n_notes < 1,
 * n_scores < 1, NULL pointers, ld_x below the set's width, an unknown feature_set: AGNN_EINVAL before any HIP call; a workspace
 * below agnn_note_features_workspace_bytes: AGNN_ENOMEM.
 * ------------------------------------------------------------------------------------------ */
#define AGNN_NF_VOICE          0
#define AGNN_NF_CADENCE        1
#define AGNN_NF_VOICE_WIDTH    25
#define AGNN_NF_CADENCE_WIDTH  56
#define AGNN_NF_FAULT_PITCH    0
#define AGNN_NF_FAULT_TS       1
#define AGNN_NF_FAULT_VOICE    2
#define AGNN_NF_FAULT_ORDER    3
#define AGNN_NF_FAULT_SCORES   4
#define AGNN_NF_FAULT_WORDS    5
typedef struct {
  const int64_t* onset_div;      /* (device) [n_notes] */
  const int64_t* duration_div;   /* (device) [n_notes] */
  const int64_t* pitch;          /* (device) [n_notes] */
  const int64_t* voice;          /* (device) [n_notes]; may be NULL for AGNN_NF_VOICE */
  const int64_t* ts_beats;       /* (device) [n_notes] */
  const int64_t* is_downbeat;    /* (device) [n_notes]; may be NULL for AGNN_NF_VOICE */
  const float* onset_beat;       /* (device) [n_notes] */
  const float* duration_beat;    /* (device) [n_notes] */
  const uint8_t* is_note_onset;  /* (device) [n_notes] or NULL: all ones */
  const int32_t* score_start;    /* (device) [n_scores + 1] */
  int64_t n_notes;
  int32_t n_scores;
  int32_t feature_set;           /* AGNN_NF_VOICE | AGNN_NF_CADENCE */
  float* x;                      /* (device) out fp32 [n_notes, 25 | 56], row stride ld_x */
  int64_t ld_x;
  int32_t* faults;               /* (device) int32[AGNN_NF_FAULT_WORDS] */
} agnn_note_features_t;
size_t agnn_note_features_workspace_bytes(int64_t n_notes, int32_t n_scores, int32_t feature_set);
int agnn_note_features_f32(const agnn_note_features_t* f /* (host) */, void* workspace, size_t workspace_bytes, agnn_stream_t stream);

/* ------------------------------------------------------------------------------------------
 * Column-statistics block (csrc/colnorm.hip):  y = dropout_p( BatchNorm1d( act(x) ) )  over the ROWS of x [n, C] fp32 (row stride
 * ld_x), act = ReLU (AGNN_CN_RELU) or identity: `layernorm1/2` of the reference's MetricalChordEncoder (models/chord.py:569-570,
 * BatchNorm1d despite the name) and the body of core/mlp.py's MLP (:27-35).  The statistics are per column, so one call serves
 * the stacked [n, T * hidden] matrix of T task heads.
 *   AGNN_CN_TRAIN  batch statistics: workgroups own slabs of AGNN_CN_SLAB rows x 64 columns (16 float4 lanes along the columns,
 *                  16 lanes down the rows); a slab leaves (mean, M2) of act(x) - K per column, K = act(x[0, column]) (the shift:
 *                  the variance is never formed as E[a^2] - mean^2), and a final pass joins the slabs' (count, mean, M2) triples
 *                  pairwise in a fixed order (Chan et al.).  It writes stats and updates running_mean / running_var (unbiased
 *                  variance, `momentum`) and *num_batches_tracked += 1 in place, on the device; the three may be NULL together.
 *                  n == 1: AGNN_EINVAL (torch refuses it too).
 *   otherwise      running statistics (required), one pass, no reduction.
 * stats [3, C] (caller-owned, written by every forward call, read by backward): the mean as a sum of two floats (hi, lo: y is
 * computed as ((a - hi) - lo) * rstd, which keeps a column with |mean| >> std exact) and rstd = 1 / sqrt(biased var + eps).
 * Dropout as agnn_norm_act_* (the library's one random stream, one counter per float4 = row * C / 4 + column / 4; `rng_used`
 * receives the (seed, step) drawn from); p == 0 draws nothing.
 * Backward: dx = relu'(x) * gamma * rstd * (g - sum(g) / n - xhat * sum(g * xhat) / n) with g = dy * mask (without
 * AGNN_CN_TRAIN: gamma * rstd * g), dgamma = sum g * xhat, dbeta = sum g: slabs leave partial column sums, a second launch adds
 * them in slab order (the scheme of agnn_norm_act_colsum_f32), a third writes dx.  No float atomics: two runs give the same bits.
 * C % 4 == 0, C >= 4, 16-byte aligned pointers and leading dimensions % 4 == 0 (AGNN_EALIGN), workspace >=
 * agnn_colnorm_workspace_bytes(n, C) (AGNN_ENOMEM).  n == 0: AGNN_OK, no pointer is looked at.  Stream-ordered, no host read.
 * ------------------------------------------------------------------------------------------ */
#define AGNN_CN_RELU   1
#define AGNN_CN_TRAIN  2
#define AGNN_CN_SLAB   128
#define AGNN_CN_FINAL_LANES 16
size_t agnn_colnorm_workspace_bytes(int64_t n, int32_t C);
int agnn_colnorm_fwd_f32(const float* x, int64_t ld_x, int64_t n, int32_t C, const float* gamma, const float* beta,
                         float* running_mean, float* running_var, int64_t* num_batches_tracked, float eps, float momentum,
                         float p, uint32_t flags, const int64_t* rng_state, uint32_t call_id, float* y, int64_t ld_y,
                         float* stats, int64_t* rng_used, void* workspace, size_t workspace_bytes, agnn_stream_t stream);
int agnn_colnorm_bwd_f32(const float* x, int64_t ld_x, int64_t n, int32_t C, const float* gamma, const float* stats, float p,
                         uint32_t flags, const int64_t* rng_state, uint32_t call_id, const float* dy, int64_t ld_dy,
                         float* dx, int64_t ld_dx, float* dgamma, float* dbeta, void* workspace, size_t workspace_bytes,
                         agnn_stream_t stream);

/* ------------------------------------------------------------------------------------------
 * Onset pooling with row selection (csrc/onsetpool.hip; reference OnsetEdgePoolingVersion2, models/chord.py:284-287):
 *   out[k, 0:H] = ( a[idx[k]] + sum_{e : dst[e] == idx[k]} a[src[e]] ) / (1 + indeg(idx[k])),   k < n_sel
 * i.e. scatter(mean) of the edge list with one appended self loop per node, of which only the rows idx are computed.  The edge
 * list comes as the CSR by destination over all n rows (agnn_csr_build: d_rowptr [n + 1], d_col = sources); a self loop in the
 * list counts once more.  idx (int64) may be unsorted and may repeat.
 * Backward through the transposed structures: da[j] = w(j) G(j) + sum_{e : src[e] == j} w(dst[e]) G(dst[e]), w(r) = 1 /
 * (1 + indeg(r)), G(r) = sum_{k : idx[k] == r} g[k] — s_rowptr / s_col: the CSR by source; sel_rowptr / sel_k: the CSR of idx by
 * node (row = idx[k], col = k).  Every sum runs in CSR order: no atomics, the same bits every run; every row of da is written.
 * A group of 4 .. 64 lanes owns a row.  An idx entry or an edge end outside [0, n) contributes nothing and adds 1 to *status
 * (device int32, may be NULL).  H % 4 == 0, H >= 4, n and n_sel < 2^31: AGNN_EINVAL; alignment as above: AGNN_EALIGN.
 * n_sel == 0 (forward) / n == 0 (backward): AGNN_OK, no pointer is looked at.
 * ------------------------------------------------------------------------------------------ */
int agnn_onset_pool_fwd_f32(const float* a, int64_t ld_a, int64_t n, int32_t H, const int32_t* d_rowptr, const int32_t* d_col,
                            const int64_t* idx, int64_t n_sel, float* out, int64_t ld_out, int32_t* status, agnn_stream_t stream);
int agnn_onset_pool_bwd_f32(const float* g, int64_t ld_g, int64_t n_sel, int32_t H, int64_t n, const int32_t* d_rowptr,
                            const int32_t* s_rowptr, const int32_t* s_col, const int32_t* sel_rowptr, const int32_t* sel_k,
                            float* da, int64_t ld_da, agnn_stream_t stream);

/* ------------------------------------------------------------------------------------------
 * GraphNorm (csrc/graphnorm.hip): PyG `GraphNorm(C, eps)` over the rows of x [n, C] fp32 (row stride ld_x), per graph g and per
 * column, as the reference's PitchSpellingGNN uses it (models/pitch_spelling.py:158, :222).  With I_g the rows of graph g:
 *   m = mean_{I_g} x,  o = x - mean_scale * m,  v = mean_{I_g} o^2 (not the centred variance when mean_scale != 1),
 *   y = weight * o / sqrt(v + eps) + bias.          Training and evaluation are the same function; no running statistics.
 * The rows of graph g are rows[seg_ptr[g] .. seg_ptr[g + 1]) (int32; what agnn_csr_build returns for row = batch, col =
 * arange(n), n_rows = G), so a sorted and an unsorted `batch` take the one path.  A graph may be empty (its stats are written as
 * zeros, no row is touched) or have one row (with mean_scale = 1: y = bias).  seg_ptr is read through a clamp to [0, n] and a
 * row index outside [0, n) is skipped, so an inconsistent index cannot make a kernel leave its operands.
 *   agnn_graphnorm_slabs  writes the slab table of a batch from seg_ptr, once per batch: a slab is at most AGNN_GN_SLAB
 *                  consecutive positions of ONE graph; the host knows only the bound ceil(n / AGNN_GN_SLAB) + G on their
 *                  number, every grid is that bound and surplus workgroups exit.  table (caller-owned, int32,
 *                  agnn_graphnorm_table_bytes(n, G)): the first slab of every graph [G + 1, padded to 4], then (graph, first
 *                  position, count, 0) per slab.
 *   forward        (a) per slab and column (count, mean, M2) of x - K, K = x[first row of the slab] (E[x^2] - mean^2 is never
 *                  formed); (b) per graph the slabs' triples joined pairwise in slab order (AGNN_GN_JOIN_LANES lanes take slabs
 *                  l, l + 16, ..., then lane order; Chan et al.), v = M2 / n + ((1 - mean_scale) m)^2, stats; (c) y.
 *   backward       with ohat = o * rstd: do = weight * rstd * (g - ohat * mean_g(g * ohat)), dx = do - mean_scale * mean_g(do),
 *                  dweight = sum g * ohat, dbias = sum g, dmean_scale = -sum_g n_g m_g mean_g(do).  (a) per slab the sums of
 *                  g * ohat, g and o; (b) per graph their join in the same order; (c) dx, and the three parameter gradients as
 *                  the sum of the graphs' terms in a fixed order (lanes take graphs l, l + 16, ..., then lane order).
 * stats [G, 3, C] (caller-owned, written by forward, read by backward): the shift mean_scale * m as a sum of two floats (hi, lo)
 * and rstd; y = ((x - hi) - lo) * rstd * weight + bias, which keeps a column with |mean| >> std exact.  m is NOT stored and NOT
 * divided out of hi + lo (mean_scale may be 0): backward recomputes it as (hi + lo) + mean_g(o) from its third slab sum.
 * The joins carry the row counts as floats: exact up to 2^24 rows in ONE graph, beyond that the join weights are rounded (relative
 * 6e-8; n_g itself stays an integer in every division).
 * No float atomics: two runs give the same bits.  C % 4 == 0, C >= 4, n < 2^31 (AGNN_EINVAL); x, y, dy, dx, the [C] vectors,
 * stats, table and workspace 16-byte aligned, seg_ptr and rows 4-byte aligned, leading dimensions % 4 == 0 (AGNN_EALIGN);
 * workspace >= agnn_graphnorm_workspace_bytes(n, G, C), table >= agnn_graphnorm_table_bytes(n, G) (AGNN_ENOMEM).  n == 0:
 * AGNN_OK, no pointer is looked at; n > 0 with G == 0: AGNN_EINVAL.  Stream-ordered, no host read.
 * ------------------------------------------------------------------------------------------ */
#define AGNN_GN_SLAB   128
#define AGNN_GN_JOIN_LANES 16
size_t agnn_graphnorm_table_bytes(int64_t n, int64_t G);
size_t agnn_graphnorm_workspace_bytes(int64_t n, int64_t G, int32_t C);
int agnn_graphnorm_slabs(const int32_t* seg_ptr, int64_t n, int64_t G, int32_t* table, size_t table_bytes, agnn_stream_t stream);
int agnn_graphnorm_fwd_f32(const float* x, int64_t ld_x, int64_t n, int64_t G, int32_t C, const int32_t* seg_ptr,
                           const int32_t* rows, const int32_t* table, size_t table_bytes, const float* weight, const float* bias,
                           const float* mean_scale, float eps, float* y, int64_t ld_y, float* stats, void* workspace,
                           size_t workspace_bytes, agnn_stream_t stream);
int agnn_graphnorm_bwd_f32(const float* x, int64_t ld_x, int64_t n, int64_t G, int32_t C, const int32_t* seg_ptr,
                           const int32_t* rows, const int32_t* table, size_t table_bytes, const float* weight,
                           const float* mean_scale, const float* stats, const float* dy, int64_t ld_dy, float* dx, int64_t ld_dx,
                           float* dweight, float* dbias, float* dmean_scale, void* workspace, size_t workspace_bytes,
                           agnn_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* AGNN_H_ */
