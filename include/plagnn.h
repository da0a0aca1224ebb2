/*
 * plagnn.h — C-ABI of the MI355X-native message-passing engine for PLA-GNN.
 *
 * This is the drop-in boundary for the reference's hot path. The reference
 * (quinlanW/PLA-GNN) reaches its message passing only through DGL 0.8.2's
 * Python API; every entry point below replaces one native operation that
 * DGL/torch runs underneath the reference's call sites:
 *
 *   pg_csr_from_coo      <- dgl.graph((start, end), num_nodes=N) + dgl.add_self_loop
 *                           and DGL's lazy COO->CSC (in-CSR) build
 *                           (code/utils.py:44-45, first update_all at code/model.py:20)
 *   pg_csr_transpose     <- DGL's reverse-graph CSR used by GSpMM.backward
 *   pg_spmm_max_fwd      <- update_all(copy_u('h','m'), max('m','neigh')) inside
 *                           SAGEConv(..., 'pool')  (code/model.py:13-15, 20, 22, 24)
 *                           = DGL SpMMCmpCsr<copy_lhs, Max> (argmax recorded)
 *   pg_spmm_max_bwd      <- DGL GSpMM.backward, copy_lhs/max branch:
 *                           dX = zeros; dX.scatter_add_(0, argX, dZ)   (reached from
 *                           train_loss.backward(), code/train.py:204), fused with the
 *                           relu' mask of fc_pool's activation
 *   pg_spmm_max_bwd_scatter  same, in DGL's scatter form (float atomics)
 *   pg_spmm_sum          <- update_all(copy_u / u_mul_e, sum|mean) (SAGEConv 'mean',
 *                           GraphConv, edge_weight=...) and their backward on the
 *                           transposed CSR. Not run by the reference: reference-unpinned.
 *   pg_sddmm_dot         <- GSpMM.backward's dY for u_mul_e; apply_edges(u_dot_v)
 *   pg_edge_softmax_*    <- dgl.ops.edge_softmax (norm_by='dst') forward and backward, H heads
 *   pg_spmm_sum_heads    <- update_all(u_mul_e, sum) with (N, H, Fh) features and (E, H, 1)
 *                           weights (GATConv's aggregation) and its feature gradient
 *   pg_sddmm_dot_heads   <- its weight gradient; apply_edges(u_dot_v) on (N, H, Fh) operands.
 *                           Attention is not used by the reference: reference-unpinned.
 *   pg_gspmm, pg_gsddmm  <- dgl.ops.gspmm / gsddmm: update_all and apply_edges with vector edge
 *                           features ((E, F) beside (N, F)), every builtin binary message, copy_e,
 *                           min; their backward. Not used by the reference: reference-unpinned.
 *   pg_gatv2_score, _bwd <- GATv2Conv's attention score attn . leaky_relu(xl[u] + xr[v]) and its
 *                           three gradients, fused: no (E, H, Fh) tensor. Reference-unpinned.
 *   pg_sample_count,     <- dgl.sampling.sample_neighbors (uniform, without replacement, in-edges) and
 *   pg_sample_fill,         dgl.to_block (include_dst_in_src): the per-batch work of a sampled mini-batch
 *   pg_block_compact        loop (dgl.dataloading.NeighborSampler). Not used by the reference, which trains
 *                           the full graph: reference-unpinned.
 *   pg_sample_*_excl,    <- the same loop seeded by edges (dgl.dataloading.as_edge_prediction_sampler,
 *   pg_edge_bits_update,    exclude_eids, dgl.dataloading.negative_sampler, g.has_edges_between /
 *   pg_edge_lookup,         g.edge_ids)
 *   pg_negative_sample
 *   pg_csr_transpose_dev,   <- the same loop: each sampled block's reverse CSR and both work schedules,
 *   pg_schedule_count_dev,     built where the block was sampled (the device twins of pg_csr_transpose /
 *   pg_schedule_build_dev      pg_schedule_*). Reference-unpinned.
 *   pg_argpos_to_src     <- DGL's argX (source node id of the max) from our compact
 *                           per-row edge positions
 *   pg_sigmoid_multi_loss<- th.sigmoid (code/model.py:29) + multi_loss
 *                           (code/train.py:89-108) forward and backward
 *   pg_mlp_head          <- liner2 + sigmoid + multi_loss (train and val) + their backward
 *                           down to liner1's activation (code/model.py:28-29), fused
 *   pg_adam_*            <- torch.optim.Adam(model.parameters(), lr) .step()
 *                           (code/train.py:180, 205), torch 1.10 formula
 *   pg_bias_act[_bwd]    <- nn.Linear bias add + F.relu / F.leaky_relu(0.01)
 *                           (code/model.py:21-27), fused
 *   pg_col_sum           <- bias gradients (sum of dY over nodes)
 *   pg_gemm_f32          <- nn.Linear GEMMs (fc_pool / fc_self / fc_neigh / liner1-2),
 *                           f32 in / f32 out with f32 accuracy: aligned operands run as
 *                           three-piece bf16 splits on v_mfma_f32_32x32x16_bf16
 *                           (gemm_x3.hip), the rest on v_mfma_f32_32x32x2_f32 (gemm.hip)
 *   pg_gemm_f32_cat      <- fc_self(h) + fc_neigh(h_neigh) (code/model.py:13-15) as one
 *                           product over two K pieces, and its input gradient
 *   pg_gemm_*_group      <- a step's weight-gradient GEMMs (code/train.py:204), one launch
 *   pg_pad2d_group       <- the drop-in SAGEConv's zero-padded weight images (503 -> 512)
 *   pg_gemm_bf16,        <- the same layers and aggregation in the bf16-storage mode
 *   pg_spmm_max_*_bf16      (BASELINE configs[4]: bf16 storage, f32 accumulate); not run
 *   pg_cast_*               by the reference (fp32 only): reference-unpinned
 *   pg_ecc               <- edge_clustering_coefficients (code/data_preprocess.py:175-214),
 *                           the ECC feature / edge-weight front end
 *   pg_loc_correction,   <- protein_loc_correction / performances_record
 *   pg_loc_performance      (code/train.py:19-86), the per-epoch eval
 *   pg_csr_spmm_f64      <- the centred products of pca() (code/data_preprocess.py:475-487,
 *                           scikit-learn 1.1.1 randomized PCA), the PCA front end
 *   pg_perturb_*         <- construct_gcn_matrix's np.corrcoef (code/data_preprocess.py:
 *                           165-170) + modify_network_topology (217-257), fused: the
 *                           N x N correlation / difference matrices are never stored
 *
 * Conventions
 *   - All buffers are caller-owned. Device entry points take device pointers and
 *     enqueue asynchronously on `stream` (a hipStream_t; NULL = default stream);
 *     they never allocate, copy to host or synchronise, so they can be captured
 *     into a HIP graph. Scratch comes from the caller through (ws, ws_bytes),
 *     sized by the matching *_workspace() query.
 *   - Host entry points (pg_csr_*, pg_schedule_*) take host pointers; their twins suffixed _dev
 *     are device entry points.
 *   - Dense matrices are row-major with an explicit leading dimension (elements).
 *   - Return 0 on success, a negative PG_ERR_* code for an argument error, or a
 *     positive hipError_t for a launch error. pg_last_error_string() gives a
 *     thread-local message for the last failure. No C++ exception crosses the ABI.
 *   - Entry points suffixed _cpu are the same operations on host pointers (OpenMP)
 *     for tensors the caller keeps on the CPU device (DGL's CPU backend role,
 *     main_normal.py -d cpu). They are never used as a fallback for a GPU call.
 */
#ifndef PLAGNN_H
#define PLAGNN_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef void* pg_stream_t; /* hipStream_t */

#define PG_OK 0
#define PG_ERR_INVALID (-1)     /* bad argument / shape */
#define PG_ERR_UNSUPPORTED (-2) /* valid but not implemented for these arguments */
#define PG_ERR_WORKSPACE (-3)   /* ws_bytes smaller than the *_workspace() query */
#define PG_ERR_HOST (-4)        /* host-side failure (allocation, ...) */

/* element type of the per-(row, feature) argmax record */
#define PG_ARG_U16 16 /* position of the winning edge inside its row, 0xFFFF = none */
#define PG_ARG_I32 32 /* same, int32, -1 = none (rows with degree >= 65535) */
/* flag OR-ed into arg_kind of pg_spmm_max_fwd[_bf16] / pg_spmm_max_bwd[_bf16] (ABI 6): the
 * forward records "none" where the maximum is 0 (not DGL's argX there: for relu inputs
 * whose gradient the relu' mask removes anyway); the backward then skips those entries
 * as fwd_out would, without reading fwd_out, and takes mask_src (required, X >= 0) as
 * implied. The other record consumers take the plain kind. */
#define PG_ARG_DEAD_NONE 0x100

/* activation codes for pg_bias_act / pg_gemm_f32 epilogues */
/* storage types of pg_gemm_bf16's output */
#define PG_DTYPE_F32 0
#define PG_DTYPE_BF16 1

#define PG_ACT_NONE 0
#define PG_ACT_RELU 1
#define PG_ACT_LEAKY 2 /* F.leaky_relu, negative_slope given separately */

/*
 * A compressed sparse row view of one graph direction plus its launch schedule.
 * For the in-CSR (DGL's CSC): rows = destination nodes, col = source node ids,
 * entries of a row in ascending edge id (the order DGL reduces them in).
 * For its transpose (out-CSR): rows = source nodes, col = destination ids in
 * ascending order, eslot = the in-CSR slot j of the same edge, epos = j - ptr_in[col]
 * (the edge's position inside its in-CSR row, which is what argmax records hold).
 * Work schedule (built by pg_schedule_build): items {row, k0, k1, slot} cover every
 * row; a row longer than `chunk` entries is split into several items that write
 * partial results to `slot`; merges {row, first_slot, n_slots, 0} combine them.
 */
typedef struct pg_csr {
  int64_t n_rows;
  int64_t n_cols;
  int64_t nnz;
  const int32_t* ptr;    /* [n_rows + 1] */
  const int32_t* col;    /* [nnz] */
  const int32_t* eslot;  /* [nnz] or NULL (NULL: slot == k) */
  const int32_t* epos;   /* [nnz] transposed CSR: position inside the in-CSR row; in-CSR
                          * (optional, ABI 10): the transposed index of each slot, used by
                          * pg_spmm_max_bwd[_bf16] to store list descriptors where the pull
                          * reads them in order (NULL: at the slots) */
  const float* ew;       /* edge weights indexed by in-CSR slot, or NULL */
  const int32_t* items;  /* [4 * n_items] */
  int64_t n_items;
  const int32_t* merges; /* [4 * n_merges] */
  int64_t n_merges;
  int64_t n_slots;
  int32_t max_deg;
  int32_t chunk;
} pg_csr_t;

/* ---------------- host: graph construction (code/utils.py:44-45) ---------------- */

/* COO (src[e], dst[e]) -> in-CSR: ptr[n_dst+1], col[nnz] = src, eid[nnz] = edge id.
 * Stable counting sort by dst, so each row lists its edges in ascending edge id. */
int pg_csr_from_coo(const int64_t* src, const int64_t* dst, int64_t nnz, int64_t n_src,
                    int64_t n_dst, int32_t* ptr, int32_t* col, int32_t* eid);

/* Transpose: tptr[n_cols+1], tcol[nnz] = row ids ascending, tslot[nnz] = slot in the
 * input CSR, tpos[nnz] = tslot - ptr[tcol] (may be NULL). */
int pg_csr_transpose(const int32_t* ptr, const int32_t* col, int64_t n_rows, int64_t n_cols,
                     int64_t nnz, int32_t* tptr, int32_t* tcol, int32_t* tslot, int32_t* tpos);

/* Work schedule sizes for rows of `ptr` split at `chunk` entries. */
int pg_schedule_count(const int32_t* ptr, int64_t n_rows, int32_t chunk, int64_t* n_items,
                      int64_t* n_merges, int64_t* n_slots, int32_t* max_deg);
/* Fill items[4*n_items] and merges[4*n_merges] (both longest first). */
int pg_schedule_build(const int32_t* ptr, int64_t n_rows, int32_t chunk, int32_t* items,
                      int32_t* merges);

/* ---------------- device: message passing ---------------- */

/* Leading dimensions and alignment of the max family (pg_spmm_max_fwd, pg_spmm_max_bwd,
 * pg_spmm_max_bwd_rows, their _bf16 forms, pg_spmm_max_bwd_scatter, pg_argpos_to_src). E is the
 * feature element (4 bytes, 2 for the _bf16 forms), R the record (2 bytes for PG_ARG_U16, 4 for
 * PG_ARG_I32). Every 2-D operand is row-major with its own leading dimension >= F (else
 * PG_ERR_INVALID, nothing launched) and a base pointer aligned to its element. For every entry
 * point: nothing outside the F columns of a row is written (pad columns of out, argpos, dx and
 * argx, and everything before and after the rows, keep their bytes), no value outside the F
 * columns of an input's rows influences a result, and every element inside the F columns of an
 * output is written by every call (no zero fill by the caller, rows without entries included).
 * The result does not depend on the path taken: the paths below differ in access width only.
 *   pg_spmm_max_fwd[_bf16]: the vector path (16-byte accesses of X, out and the workspace
 *     values, 4 R-byte accesses of the records) needs F, ldx, ldo and lda multiples of 4, X,
 *     out and ws 16-byte aligned and argpos aligned to 4 R (8 bytes for u16 records, 16 for
 *     i32). Anything else takes the scalar path (element accesses, 1024 columns per feature
 *     tile, split rows combined by a second launch). On the vector path split rows are
 *     combined inside the launch when ws is also 256-byte aligned, else by a second launch.
 *     ws: 4-byte aligned at least.
 *   pg_spmm_max_bwd[_rows][_bf16], grouped form (PG_ARG_U16 records, F <= 1024, N F < 2^31),
 *     two independent decisions. Pack: vector when F, lda, ldd (and ldf with fwd_out) are
 *     multiples of 4, argpos is 8-byte aligned and dout (and fwd_out) aligned to 4 E; else
 *     element accesses of all three. Pull: a split source row is combined inside the pull's
 *     launch when F and ldx are multiples of 4 and dx is aligned to 4 E, and, where the mask is
 *     read (mask_src given and no PG_ARG_DEAD_NONE), ldm is a multiple of 4 and mask_src
 *     aligned to 4 E; else by a second launch (element accesses of dx and mask_src unless its
 *     own rows are 4-aligned). With PG_ARG_DEAD_NONE mask_src is not read at all. _rows: the
 *     same; row_active and eslot_active are flat arrays.
 *   pg_spmm_max_bwd, record gather (PG_ARG_I32 records or F > 1024; f32 only): the vector path
 *     needs F, lda, ldd, ldx (and ldm with a mask) multiples of 4, dout, dx, mask_src and ws
 *     16-byte aligned and argpos aligned to 4 R; else the scalar path, 1024 columns per launch.
 *   ws of pg_spmm_max_bwd[_rows][_bf16] must be 16-byte aligned (PG_ERR_INVALID otherwise,
 *     nothing launched): its regions (partial rows | records | descriptors | tickets) start
 *     multiples of 256 bytes past ws and are accessed 16 bytes at a time.
 *   pg_spmm_max_bwd_scatter, pg_argpos_to_src: element accesses only, no alignment beyond the
 *     element's; lda, ldd, ldx are free (>= F). */

/* out[v,f] = max_{k in row v} (ew? ew[k]:1) * X[col[k], f]  (strict >, first wins, start -inf);
 * argpos[v,f] = k - ptr[v] of the winner. Rows with no entries: out = 0, argpos = none.
 * A +-inf result is stored as 0 (DGL's replace_inf_with_zero after a max reduce).
 * Requires X, out 4-byte aligned; the vector path is taken when ldx, ldo, F are
 * multiples of 4 and the base pointers are 16-byte aligned. Rows the schedule splits are
 * combined in piece order (the earliest maximal entry wins); with a 256-byte aligned ws
 * (at least the query's bytes) inside the same launch, else by a second launch. */
size_t pg_spmm_max_fwd_workspace(const pg_csr_t* g, int64_t F, int arg_kind);
int pg_spmm_max_fwd(const pg_csr_t* g, const float* X, int64_t ldx, int64_t F, float* out,
                    int64_t ldo, void* argpos, int64_t lda, int arg_kind, void* ws,
                    size_t ws_bytes, pg_stream_t stream);

/* Deterministic backward (gather over the transposed CSR gt of g; gt->epos required):
 *   dx[u,f] = sum_{(v,j) in gt row u, ascending v} [argpos[v,f] == j - g.ptr[v]] * ew[j] * dout[v,f]
 * then, if mask_src != NULL, dx[u,f] *= (mask_src[u,f] > 0)  (relu' of fc_pool).
 * fwd_out (optional, needs mask_src = the forward's input X): the forward's output. An
 * entry (v, f) with fwd_out[v,f] == 0 is skipped: its winner u has X[u,f] * w == 0, so it
 * is either masked (X[u,f] = 0) or weighted 0 — the result is unchanged. (A +-inf
 * maximum, stored as 0, is skipped too.) The mask is still applied.
 * PG_ARG_DEAD_NONE records (the same skip made by the forward; needs mask_src = X, a relu
 * output, X >= 0): every entry left has X[u,f] * w != 0, hence X[u,f] > 0, so the mask is
 * implied and mask_src is not read (an element no entry reaches is +0 either way). With
 * X < 0 somewhere the result is undefined.
 * Every dx element is written (no zero-fill needed). A source row the schedule of gt
 * splits is summed piece by piece (each piece in ascending v from +0) and the pieces in
 * order from +0, inside the pull's launch for 16-byte rows (F, ldx multiples of 4). */
size_t pg_spmm_max_bwd_workspace(const pg_csr_t* gt, int64_t F);
int pg_spmm_max_bwd(const pg_csr_t* g, const pg_csr_t* gt, const void* argpos, int64_t lda,
                    int arg_kind, const float* dout, int64_t ldd, int64_t F,
                    const float* mask_src, int64_t ldm, const float* fwd_out, int64_t ldf,
                    float* dx, int64_t ldx, void* ws, size_t ws_bytes, pg_stream_t stream);
/* The same with a set of active destination rows: row_active int8 [N], nonzero =
 * the row's dout may be nonzero; an inactive row counts as dout = 0 and its dout and argpos
 * rows are never read. eslot_active int32 [nnz] is gt->eslot with -1 at every entry whose
 * destination row (gt->col) is inactive; the caller builds it once per graph and row set.
 * dx is bitwise what pg_spmm_max_bwd gives on a dout whose inactive rows are zero: a list
 * entry of value +-0 changes no bit of a sum that starts at +0. Both arrays NULL: exactly
 * pg_spmm_max_bwd; one NULL: PG_ERR_INVALID. Grouped path only (PG_ARG_U16 records,
 * F <= 1024, N F < 2^31), else PG_ERR_UNSUPPORTED: the caller uses the plain call. Same
 * workspace. */
int pg_spmm_max_bwd_rows(const pg_csr_t* g, const pg_csr_t* gt, const void* argpos, int64_t lda,
                         int arg_kind, const float* dout, int64_t ldd, int64_t F,
                         const float* mask_src, int64_t ldm, const float* fwd_out, int64_t ldf,
                         float* dx, int64_t ldx, const int8_t* row_active, const int32_t* eslot_active,
                         void* ws, size_t ws_bytes, pg_stream_t stream);

/* DGL-form backward: dx = 0; dx[src(argpos[v,f]), f] += ew * dout[v,f] with f32
 * atomics (summation order not reproducible). The callee zero-fills dx. */
int pg_spmm_max_bwd_scatter(const pg_csr_t* g, const void* argpos, int64_t lda, int arg_kind,
                            const float* dout, int64_t ldd, int64_t F, float* dx, int64_t ldx,
                            int64_t n_src, pg_stream_t stream);

/* out[r,f] = sum_{k in row r} coef_k * X[col[k], f] with
 *   coef_k = (ew ? ew[eslot ? eslot[k] : k] : 1)
 *   norm_mode 0: plain sum; 1: divide the row sum by the row's entry count (mean);
 *   2: each term divided by the entry count of col[k] in norm_ptr (mean backward).
 * Rows with no entries get +0. Every element out[r, f], r < n_rows, f < F, is written exactly
 * once (nothing outside the F columns of a row is read or written, ldx, ldo >= F), without
 * atomics, as one fixed float32 expression (the library is built without FMA contraction):
 *   a schedule item {row, k0, k1, slot} starts at +0 and adds, for k = k0 .. k1 - 1 in
 *     order, x = X[col[k], f] (with ew: x * coef_k; then in mode 2 that divided by
 *     (float)(entry count of col[k])), each step one rounding;
 *   an unsplit row (slot < 0) is its item, in mode 1 divided by (float)(the row's entry
 *     count) when that is not 0;
 *   a split row adds its items' partial sums (workspace slots s0 .. s0 + ns - 1 of its
 *     merge) in slot order from +0, then in mode 1 divides by (float)(the row's entry count).
 * So the result is bitwise reproducible, does not depend on the path taken, and on rows the
 * schedule does not split it equals pg_spmm_sum_cpu bit for bit (which sums every row as one
 * item). The vector path (float4 accesses, 256 columns per launch) is taken when F, ldx and
 * ldo are multiples of 4 and X, out and ws are 16-byte aligned; the scalar path (1024 columns
 * per launch) otherwise. F == 0 and n_rows == 0 succeed without touching a buffer. The call
 * allocates nothing and does not synchronise (graph-capturable). PG_ERR_INVALID: ldx or ldo
 * below F, norm_mode outside 0 .. 2, mode 2 without norm_ptr, X or out NULL with work to do
 * (pg_spmm_sum_cpu the same); PG_ERR_WORKSPACE: ws_bytes below pg_spmm_sum_workspace(g, F)
 * (0 for a schedule without split rows). Nothing is launched after an error. */
size_t pg_spmm_sum_workspace(const pg_csr_t* g, int64_t F);
int pg_spmm_sum(const pg_csr_t* g, const float* X, int64_t ldx, int64_t F, int norm_mode,
                const int32_t* norm_ptr, float* out, int64_t ldo, void* ws, size_t ws_bytes,
                pg_stream_t stream);

/* Per-edge dot products over the in-CSR g (SDDMM), in slot order:
 *   de[k] = sum_f D[v,f] * X[col[k],f]                 for every slot k of row v
 *   norm_mode 1: the finished sum is divided by (float)(entry count of row v)  (mean)
 *   argpos != NULL (max form): only the f with argpos[v,f] == k - ptr[v] are summed
 *     (arg_kind PG_ARG_U16 | PG_ARG_I32, PG_ARG_DEAD_NONE accepted: "none" matches no edge)
 * g->ew is not read. Every de[k], k < nnz, is written exactly once (no workspace, no
 * atomics: each slot lies in exactly one schedule item), in a fixed summation order, so
 * the result is bitwise reproducible. The vector path is taken when F, ldd, ldx (and lda
 * in the max form) are multiples of 4 and D, X (and argpos) are 16-byte aligned. The call
 * allocates nothing and does not synchronise (graph-capturable). */
int pg_sddmm_dot(const pg_csr_t* g, const float* D, int64_t ldd, const float* X, int64_t ldx,
                 int64_t F, int norm_mode, const void* argpos, int64_t lda, int arg_kind,
                 float* de, pg_stream_t stream);

/* Multi-head attention over the in-CSR g (dgl.ops.edge_softmax and GATConv's aggregation):
 * edge features are [nnz][ld] row-major in in-CSR SLOT order with H heads, ld >= H; v is the
 * row (destination) that owns slot k. 1 <= H <= 64, Fh >= 1, H * Fh as wide as pg_spmm_sum
 * takes; outputs must not alias inputs. nnz == 0 and n_rows == 0 succeed (pg_spmm_sum_heads
 * still zero-fills the rows of a graph without edges). Every output element is written
 * exactly once, without atomics, in a reduction order that depends on the graph and the
 * shapes only: two runs give bitwise-equal results. Nothing is allocated or synchronised.
 *
 * a[k,h] = exp(s[k,h] - m[v,h]) / sum_{k' in row v} exp(s[k',h] - m[v,h]),
 * m[v,h] = max_{k' in row v} s[k',h]. A -inf score gives a = 0 when its row has a finite
 * score for that head; a row whose scores for a head are all -inf or contain NaN is
 * unspecified. One wave per row, one workgroup per row the schedule splits. */
int pg_edge_softmax_fwd(const pg_csr_t* g, const float* s, int64_t lds, int32_t H, float* a,
                        int64_t lda, pg_stream_t stream);
/* ds[k,h] = a[k,h] * (da[k,h] - sum_{k' in row v} a[k',h] * da[k',h]) */
int pg_edge_softmax_bwd(const pg_csr_t* g, const float* a, int64_t lda, const float* da,
                        int64_t ldda, int32_t H, float* ds, int64_t ldds, pg_stream_t stream);
/* out[r, h*Fh + j] = sum_{k in row r} A[(eslot ? eslot[k] : k), h] * X[col[k], h*Fh + j];
 * rows without entries: 0. g->ew is not read. On the transposed CSR (eslot set) this is the
 * feature gradient. The vector path needs Fh % 4 == 0 besides pg_spmm_sum's conditions.
 * Workspace: pg_spmm_sum_workspace(g, H*Fh). */
int pg_spmm_sum_heads(const pg_csr_t* g, const float* A, int64_t lda, int32_t H, const float* X,
                      int64_t ldx, int64_t Fh, float* out, int64_t ldo, void* ws, size_t ws_bytes,
                      pg_stream_t stream);
/* de[k,h] = sum_{j < Fh} Dm[v, h*Fh + j] * X[col[k], h*Fh + j]: the gradient of
 * pg_spmm_sum_heads w.r.t. A (Dm = dout), and apply_edges(u_dot_v) on (N, H, Fh) operands.
 * The wave-wide path needs Fh in {4, 8, ... 256} and pg_sddmm_dot's vector conditions. */
int pg_sddmm_dot_heads(const pg_csr_t* g, const float* Dm, int64_t ldd, const float* X,
                       int64_t ldx, int32_t H, int64_t Fh, float* de, int64_t lde,
                       pg_stream_t stream);

/* GATv2 attention scores (Brody, Alon, Yahav 2022; dgl.nn.pytorch.GATv2Conv), fused: no
 * [nnz][H*Fh] tensor exists, forward or backward. Conventions of the multi-head family above
 * (slot order, 1 <= H <= 64, Fh >= 1); attn is [H*Fh], lrelu(x) = x > 0 ? x : slope * x and
 * lrelu'(x) = x > 0 ? 1 : slope (0 counts as negative).
 *
 *   s[k,h] = sum_{d < Fh} attn[h*Fh + d] * lrelu(XL[col[k], h*Fh + d] + XR[v, h*Fh + d])
 *
 * One wave per schedule item; every s[k,h] is written exactly once (a head that straddles
 * 256-column feature tiles is accumulated inside the wave), no workspace. The vector path
 * needs Fh % 4 == 0, ldl and ldr multiples of 4 and XL, XR, attn 16-byte aligned; anything
 * else takes a scalar path (one (entry, head) per lane, d ascending). */
int pg_gatv2_score(const pg_csr_t* g, const float* XL, int64_t ldl, const float* XR, int64_t ldr,
                   const float* attn, int32_t H, int64_t Fh, float slope, float* s, int64_t lds,
                   pg_stream_t stream);
/* One backward pass over the CSR g, which is the in-CSR or its transpose: the pre-activation
 * t_k = Xown[r] + Xgat[col[k]] is recomputed for every entry k of row r, and with
 * e(k) = eslot ? eslot[k] : k
 *   dXown[r, f] = attn[f] * sum_{k in row r} ds[e(k), h(f)] * lrelu'(t_k[f])   (if dXown)
 *   dattn[f]    = sum_k ds[e(k), h(f)] * lrelu(t_k[f])                          (if dattn)
 * On the in-CSR (Xown = XR, Xgat = XL) dXown is dXR; on the transposed CSR with the operands
 * swapped it is dXL; dattn comes out of either pass. Both outputs NULL: nothing is done.
 * Split rows: partial sums in workspace slots, combined in slot order. dattn: one partial row
 * per workgroup, reduced in workgroup order by two small launches. No atomics; bitwise
 * reproducible. Workspace: pg_gatv2_bwd_workspace(g, H, Fh, dattn != NULL) bytes. */
size_t pg_gatv2_bwd_workspace(const pg_csr_t* g, int32_t H, int64_t Fh, int with_dattn);
int pg_gatv2_bwd(const pg_csr_t* g, const float* ds, int64_t ldds, const float* Xown, int64_t ldown,
                 const float* Xgat, int64_t ldgat, const float* attn, int32_t H, int64_t Fh,
                 float slope, float* dXown, int64_t lddx, float* dattn, void* ws, size_t ws_bytes,
                 pg_stream_t stream);

/* g-SpMM / g-SDDMM (DGL's gspmm / gsddmm): messages with vector edge features, f32.
 * Binary operator of a message z = op(l, r), the reducer, and where an operand row of entry
 * k of the CSR that is passed comes from: */
#define PG_OP_ADD 0
#define PG_OP_SUB 1
#define PG_OP_MUL 2
#define PG_OP_DIV 3      /* a true division (DGL multiplies by a reciprocal) */
#define PG_OP_COPY_LHS 4 /* R is not read and may be NULL */
#define PG_OP_COPY_RHS 5 /* L is not read and may be NULL */
#define PG_RED_SUM 0
#define PG_RED_MAX 1
#define PG_RED_MIN 2
#define PG_TGT_U 0 /* row col[k] */
#define PG_TGT_V 1 /* the row that owns entry k (pg_gsddmm only) */
#define PG_TGT_E 2 /* the edge row: eidx[k] if eidx != NULL, else g->eslot[k] if set, else k */

/* out[v,f] = reduce_{k in row v} op(L[t_l(k), f], R[t_r(k), f]), lt, rt in {PG_TGT_U, PG_TGT_E}.
 * On the transposed CSR the same call gives the source-side gradients. g->ew is not read.
 * Sum: every schedule item sums in ascending k from +0, the pieces of a split row are added
 *   in slot order from +0; norm_mode 1 divides a finished sum by the row's entry count
 *   (rows without entries are not divided). argpos is not written.
 * Max / min: pg_spmm_max_fwd's rules: strict compare, the first entry wins, pieces combined
 *   in piece order (the earliest extremal entry wins); rows without entries give 0 and the
 *   record "none"; a +-inf result is stored as 0; argpos (may be NULL) holds in-row positions,
 *   u16 or i32 by arg_kind. norm_mode must be 0.
 * No atomics, every out element is written, bitwise repeatable. The vector path (16-byte
 * loads) needs F and every leading dimension a multiple of 4 and 16-byte aligned base
 * pointers (8-byte for u16 records); anything else takes the scalar path. nnz == 0,
 * n_rows == 0 and F == 0 succeed. Nothing is allocated or synchronised. */
size_t pg_gspmm_workspace(const pg_csr_t* g, int64_t F, int reduce, int arg_kind);
int pg_gspmm(const pg_csr_t* g, int op, int reduce, const float* L, int64_t ldl, int lt,
             const float* R, int64_t ldr, int rt, const int32_t* eidx, int64_t F, int norm_mode,
             float* out, int64_t ldo, void* argpos, int64_t lda, int arg_kind, void* ws,
             size_t ws_bytes, pg_stream_t stream);
/* out[e(k), f] = op(L[t_l(k), f], R[t_r(k), f]) for every entry k, targets in {U, V, E};
 * e(k) is PG_TGT_E's row index, so with eidx a permutation every output row is written
 * exactly once (out must not alias an operand). argpos != NULL: the masked form of the
 * max / min backward: the value where argpos[v,f] == k - ptr[v], +0 elsewhere ("none"
 * matches no edge). Every slot lies in exactly one schedule item: no workspace, no merge. */
int pg_gsddmm(const pg_csr_t* g, int op, const float* L, int64_t ldl, int lt, const float* R,
              int64_t ldr, int rt, const int32_t* eidx, int64_t F, float* out, int64_t ldo,
              const void* argpos, int64_t lda, int arg_kind, pg_stream_t stream);

/* argx[v,f] = col[ptr[v] + argpos[v,f]] (DGL's argX, int64), -1 where none. */
int pg_argpos_to_src(const pg_csr_t* g, const void* argpos, int64_t lda, int arg_kind,
                     int64_t F, int64_t* argx, int64_t ldx, pg_stream_t stream);

/* ---------------- device: neighbour sampling and block compaction ---------------- */

/* Mini-batch sampling (dgl.sampling.sample_neighbors, dgl.to_block). g is the parent's in-CSR
 * (rows = destinations, entries in ascending edge id; its schedule is not read). seeds[n_seeds]
 * are int32 parent ids; they may repeat. A seed outside [0, g->n_rows) counts as a row without
 * entries. fanout < 0 keeps whole rows, fanout == 0 gives empty rows.
 *
 * pg_sample_count: out_ptr[n_seeds + 1] = the exclusive scan of min(deg(seed_i), fanout) (int32;
 *   the total must stay below 2^31). Workspace: pg_sample_count_workspace(n_seeds) bytes.
 * pg_sample_fill: row i of the sampled CSR, at out_ptr[i]. A row with deg <= fanout (or
 *   fanout < 0) is copied. Any other row keeps the `fanout` entries with the smallest
 *   (key, edge id) pairs, key = a 32-bit stateless function of (seed64, edge id) only
 *   (two rounds of the splitmix64 finaliser, csrc/sample_key.hpp). The kept entries are
 *   written in ascending edge id. out_col = parent source ids, out_eid = parent edge ids;
 *   eid[nnz] maps in-CSR slots to edge ids (NULL: the identity). The result depends on the
 *   arguments only, never on launch shape, the row's place in seeds, or timing: it equals
 *   pg_sample_fill_cpu bit for bit. One wave per row; the selection is a bitwise threshold
 *   search over (key, position) with a fixed number of passes (32 + position bits). Rows up
 *   to PG_SAMPLE_LDS_KEYS entries keep their keys in LDS. A longer row recomputes its keys in
 *   every pass over it, so it is first narrowed: the keys below a threshold set for an
 *   expected 2 fanout + 64 of them are counted (the threshold doubled or halved, at most 40
 *   times, until between fanout and PG_SAMPLE_LDS_KEYS / 2 keys pass: a function of the row's
 *   keys only), those (key, position) pairs are gathered into LDS and searched there. Only
 *   when 2 fanout + 64 > PG_SAMPLE_LDS_KEYS / 2, or that adjustment does not settle, does
 *   every pass of the search walk the whole row. No global workspace.
 * Nothing is allocated or synchronised; the caller reads out_ptr[n_seeds] back between the
 * two calls (so the pair is not captured into a graph). n_seeds == 0 and nnz == 0 succeed. */
#define PG_SAMPLE_LDS_KEYS 2048
size_t pg_sample_count_workspace(int64_t n_seeds);
int pg_sample_count(const pg_csr_t* g, const int32_t* seeds, int64_t n_seeds, int32_t fanout,
                    int32_t* out_ptr, void* ws, size_t ws_bytes, pg_stream_t stream);
int pg_sample_fill(const pg_csr_t* g, const int32_t* eid, const int32_t* seeds, int64_t n_seeds,
                   int32_t fanout, uint64_t seed64, const int32_t* out_ptr, int32_t* out_col,
                   int32_t* out_eid, pg_stream_t stream);
/* Relabel the sources of a sampled CSR into a compact block (dgl.to_block with
 * include_dst_in_src=True): src_ids[n_dst + nnz] starts with dst_ids[n_dst] in the given order,
 * every other parent id of col[nnz] follows in the order of its first appearance in col;
 * col_local[k] = the position of col[k] in src_ids; *n_src_dev (int32, device) = the number of
 * src_ids written, -1 if dst_ids holds a duplicate, -2 if an id lies outside [0, n_parent)
 * (src_ids and col_local are then unspecified). A dense first-position map over n_parent
 * (int32 in the workspace, filled with atomicMin, which is order-independent on integers) and
 * one prefix sum: bitwise repeatable. Workspace: pg_block_compact_workspace(n_dst, nnz,
 * n_parent) bytes. Nothing is allocated or synchronised. */
size_t pg_block_compact_workspace(int64_t n_dst, int64_t nnz, int64_t n_parent);
int pg_block_compact(const int32_t* dst_ids, int64_t n_dst, const int32_t* col, int64_t nnz,
                     int64_t n_parent, int32_t* src_ids, int32_t* col_local, int32_t* n_src_dev,
                     void* ws, size_t ws_bytes, pg_stream_t stream);

/* ---------------- device: link-prediction mini-batches ---------------- */

/* The per-batch work of an edge-seeded loop (dgl.dataloading.as_edge_prediction_sampler): sampling
 * that leaves the seed edges out, edge lookup and negative pairs. Integer only; every entry point
 * equals its _cpu twin bit for bit and follows the device contract above (enqueue on `stream`,
 * scratch through (ws, ws_bytes), nothing allocated, copied to the host or synchronised, an
 * argument error launches nothing, empty inputs succeed and read no buffer). Every id read from
 * a caller's array is range-checked before it indexes anything. g is an in-CSR as for
 * pg_sample_*; its schedule is not read.
 *
 * pg_edge_bits_update: a bit set over edge ids, bit (e & 31) of bits[e >> 5] for edge id e,
 *   ceil(n_edge_ids / 32) words that the caller owns and zeroes once. set = 1 sets the bits of
 *   eids[n] (atomic OR), set = 0 clears them (atomic AND): both order-independent, duplicates
 *   are fine. An id outside [0, n_edge_ids) is skipped and stores -2 to *status_dev (int32,
 *   device; written on that error only, so the caller zeroes it; NULL: not reported). A batch
 *   sets its ids before sampling and clears the same ids afterwards: O(batch), not O(E).
 * pg_sample_count_excl / pg_sample_fill_excl: pg_sample_count / pg_sample_fill on the graph
 *   with the entries whose edge id has its bit set in excl_bits deleted and the edge ids kept:
 *   row i holds min(deg - excluded in the row, fanout) entries, the ones with the fanout
 *   smallest (sample key, edge id) among the entries that remain, in ascending edge id; a row
 *   with at most fanout entries left (or fanout < 0) keeps them all in order. eid[nnz] maps
 *   slots to edge ids (NULL: the identity); the count reads it too, the bit set being indexed
 *   by edge id. excl_bits covers the edge ids [0, g->nnz) (an id outside counts as not
 *   excluded) and must not change between the two calls; NULL gives pg_sample_*'s result bit
 *   for bit. The count is one wave per seed row (it walks the row and tests the bits), then
 *   the tile scan of pg_sample_count. The fill keeps pg_sample_fill's structure: one wave per
 *   row, the bitwise threshold search over (key, position) composites counted with ballots. A
 *   row of up to PG_SAMPLE_LDS_KEYS entries keeps its keys in LDS and its exclusion flags in
 *   PG_SAMPLE_LDS_KEYS / 32 LDS words beside them, read from the bit set once; an excluded
 *   entry's composite lies above every searched bit, so no pass counts it and the final
 *   compare skips it. A longer row narrows to the surviving (key, position) pairs below a key
 *   threshold estimated from the row's remaining count, as pg_sample_fill does from deg.
 *   Workspace of the count: pg_sample_count_excl_workspace(n_seeds) bytes.
 * pg_edge_lookup: out_eid[i] = the smallest edge id among the entries of row v[i] whose column
 *   is u[i] (the edge u[i] -> v[i]; rows ascend in edge id, so the first matching position),
 *   -1 when there is none or u[i] / v[i] lies outside the graph. One wave per pair scans the
 *   row, the first match found with a ballot.
 * pg_negative_sample: slot (i, j), j < k, writes index i * k + j. Attempts t = 0 .. tries - 1:
 *   u = pos_src[i] (NULL: a draw over [0, g->n_cols)), v = a draw over [0, g->n_rows); the first
 *   attempt that passes `flags` wins: PG_NEG_REJECT_EDGE rejects when u -> v is an edge (the
 *   lookup above), PG_NEG_REJECT_SELF when u == v. A slot without a passing attempt, or with
 *   pos_src[i] outside [0, g->n_cols), writes -1 to both outputs and counts in *n_fail_dev (int32,
 *   device; zeroed by the call, then an integer atomic add). A draw is a 32-bit stateless
 *   function of (seed64, pos_id[i] (NULL: i), j, t, which end) only (csrc/sample_key.hpp,
 *   domain-separated from the neighbour sampler's key), mapped to a range of n by
 *   ((uint64_t)key * n) >> 32: the result depends on the arguments only, never on the slot's
 *   place in the batch, the launch shape or timing. 1 <= tries <= 64, k >= 1,
 *   n_pos * k < 2^31. */
#define PG_NEG_REJECT_EDGE 1
#define PG_NEG_REJECT_SELF 2
int pg_edge_bits_update(uint32_t* bits, int64_t n_edge_ids, const int32_t* eids, int64_t n, int set,
                        int32_t* status_dev, pg_stream_t stream);
size_t pg_sample_count_excl_workspace(int64_t n_seeds);
int pg_sample_count_excl(const pg_csr_t* g, const int32_t* eid, const int32_t* seeds, int64_t n_seeds,
                         int32_t fanout, const uint32_t* excl_bits, int32_t* out_ptr, void* ws,
                         size_t ws_bytes, pg_stream_t stream);
int pg_sample_fill_excl(const pg_csr_t* g, const int32_t* eid, const int32_t* seeds, int64_t n_seeds,
                        int32_t fanout, uint64_t seed64, const uint32_t* excl_bits,
                        const int32_t* out_ptr, int32_t* out_col, int32_t* out_eid, pg_stream_t stream);
int pg_edge_lookup(const pg_csr_t* g, const int32_t* eid, const int32_t* u, const int32_t* v, int64_t n,
                   int32_t* out_eid, pg_stream_t stream);
int pg_negative_sample(const pg_csr_t* g, const int32_t* pos_src, const int32_t* pos_id, int64_t n_pos,
                       int32_t k, int32_t tries, int flags, uint64_t seed64, int32_t* neg_src,
                       int32_t* neg_dst, int32_t* n_fail_dev, pg_stream_t stream);

/* A sampled block's transpose and schedules on the device: the twins of the host entry points
 * pg_csr_transpose / pg_schedule_count / pg_schedule_build on device pointers, equal to them bit
 * for bit (the host functions are the specification), so that dgl.dataloading.NeighborSampler
 * moves no index array across the bus. They follow the device contract above: enqueue on
 * `stream`, scratch through (ws, ws_bytes), nothing allocated, copied to the host or
 * synchronised (each can be captured), an argument error launches nothing. All three succeed
 * and read no input buffer when there are no rows, no columns or no entries. No atomics: every
 * result is a function of the arguments. Core: a stable LSD radix sort of (key, value) u32
 * pairs, 8-bit digits, 1024 entries per workgroup; a pass = per-tile digit counts, a scan of the
 * (digit-major, tile-minor) table, a stable scatter whose ranks inside a tile come from wave
 * ballots and a cross-wave prefix in LDS.
 *
 * pg_csr_transpose_dev: tslot = the slots sorted stably by column over
 *   ceil(bits(n_cols - 1) / 8) passes (row ids ascending in each transposed row, duplicates in
 *   slot order), tptr[c] = the first sorted position whose column is >= c, tcol[t] = the row of
 *   tslot[t] (binary search in ptr), tpos[t] = tslot[t] - ptr[tcol[t]] (tslot, tpos may be
 *   NULL). *status_dev (int32, device) = 0, -2 when a col[k] lies outside [0, n_cols) (it is
 *   then taken as column 0: nothing is indexed with it), -3 when ptr does not span nnz; the
 *   outputs are then unspecified but every access stays inside the buffers.
 * pg_schedule_count_dev: counts_dev[6] (int64, device) = n_items, n_merges, n_slots, max_deg,
 *   min_deg (0 without rows), status (-1: ptr not monotone, -2: a total reaches 2^31).
 * pg_schedule_build_dev: items[4 n_items], merges[4 n_merges] in pg_schedule_build's order.
 *   n_items, n_merges and max_deg are the count's, read back by the caller; every write is
 *   guarded by them. Raw item indices and slots come from exclusive scans over the rows; items
 *   are sorted stably by chunk - len over bits(chunk) key bits, merges by
 *   ceil(max_deg / chunk) - n, both with the raw index as value. */
size_t pg_csr_transpose_dev_workspace(int64_t n_rows, int64_t n_cols, int64_t nnz);
int pg_csr_transpose_dev(const int32_t* ptr, const int32_t* col, int64_t n_rows, int64_t n_cols,
                         int64_t nnz, int32_t* tptr, int32_t* tcol, int32_t* tslot, int32_t* tpos,
                         int32_t* status_dev, void* ws, size_t ws_bytes, pg_stream_t stream);
size_t pg_schedule_count_dev_workspace(int64_t n_rows);
int pg_schedule_count_dev(const int32_t* ptr, int64_t n_rows, int32_t chunk, int64_t* counts_dev,
                          void* ws, size_t ws_bytes, pg_stream_t stream);
size_t pg_schedule_build_dev_workspace(int64_t n_rows, int64_t n_items, int64_t n_merges);
int pg_schedule_build_dev(const int32_t* ptr, int64_t n_rows, int32_t chunk, int64_t n_items,
                          int64_t n_merges, int32_t max_deg, int32_t* items, int32_t* merges,
                          void* ws, size_t ws_bytes, pg_stream_t stream);

/* ---------------- device: dense helpers of the training step ---------------- */

/* y = act(y + bias) in place (bias may be NULL). */
int pg_bias_act(float* y, int64_t ldy, int64_t rows, int64_t cols, const float* bias, int act,
                float slope, pg_stream_t stream);
/* dy = dy * act'(y) in place, from the activation OUTPUT y (relu: y>0; leaky: y>0?1:slope). */
int pg_act_bwd(float* dy, int64_t lddy, const float* y, int64_t ldy, int64_t rows, int64_t cols,
               int act, float slope, pg_stream_t stream);
/* out[c] (+)= sum_r x[r,c]; deterministic (fixed two-level order). */
size_t pg_col_sum_workspace(int64_t rows, int64_t cols);
int pg_col_sum(const float* x, int64_t ldx, int64_t rows, int64_t cols, float* out,
               int accumulate, void* ws, size_t ws_bytes, pg_stream_t stream);

/* Sigmoid + class-weighted BCE of code/train.py:89-108 on the rows in index[]:
 *   prob = sigmoid(z) for all n_rows rows (written if prob != NULL)
 *   loss[0] = sum_c -(1/n) sum_{r in index} (t log(clamp(p,1e-9,10)) w_c
 *                                   + (1-t) log(clamp(1-p,1e-9,10))) / (w_c+1) * 2
 *   dz (if not NULL) = d loss / d z for rows in index, 0 elsewhere (all n_rows rows written).
 * class_w[2c] = (float)w_c and class_w[2c+1] = (float)(w_c + 1), both rounded from the
 * float64 weights of weight_cal (code/train.py:111-126). C <= 64. loss may be NULL.
 * n_index = 0 (index may then be NULL): prob and dz (all zeros) are still written for all
 * n_rows rows; loss[0] is NOT written (there is no mean over no rows) and keeps its value. */
/* The model head after liner1, fused (code/model.py:28-29, code/train.py:89-108, 199-207):
 *   z = A4 W2^T + b2;  prob = sigmoid(z);  multi_loss over the rows with row_set 1 (train,
 *   loss2[0], n = n_train) and row_set 2 (val, loss2[1], n = n_val);  dz = d loss2[0] / dz
 *   (0 outside the train rows);  dA4 = (dz W2) * leaky'(A4) with negative slope `slope`.
 * A4 [n][K] and dA4 [n][K] are f32 or bf16 (a_dtype); W2 [C][K], b2 [C] f32; K <= 128,
 * C <= 16. Optional outputs (NULL = skip): prob, dz, dz_bf16 (a bf16 copy of dz, leading
 * dimension lddz), dA4. Scratch: pg_mlp_head_workspace(n, C) bytes.
 * n_train / n_val are the numbers of rows with row_set 1 / 2. An empty set's loss slot is
 * NOT written and keeps its value (n_train = 0: loss2[0]; n_val = 0: loss2[1]); with
 * n_train = 0, dz, dz_bf16 and dA4 are written as zeros for every row. prob does not depend
 * on the sets. The same holds for pg_mlp_l1_head[_ex]. */
size_t pg_mlp_head_workspace(int64_t n, int32_t C);
int pg_mlp_head(const void* A4, int64_t lda, int64_t n, int32_t K, int a_dtype, const float* W2,
                int64_t ldw, const float* b2, int32_t C, const float* labels, int64_t ldl,
                const float* class_w, const int8_t* row_set, int64_t n_train, int64_t n_val,
                float* prob, int64_t ldp, float* dz, int64_t lddz, void* dz_bf16, void* dA4,
                int64_t ldg, float slope, float* loss2, void* ws, size_t ws_bytes,
                pg_stream_t stream);
/* liner1 + the head above + liner1's input gradient in one pass (ABI 12; f32; replaces the
 * fwd.liner1 GEMM, pg_mlp_head and the dgrad.liner1 GEMM of a training step, code/model.py:
 * 26-29 and their backward):
 *   A4 = leaky(H3 W1^T + b1);  then pg_mlp_head's outputs on A4 (prob, dz, dA4, loss2);
 *   dH3 = (dA4 W1) * leaky'(H3)  (liner1's input gradient through the last SAGE layer's
 *   leaky_relu, with negative slope `slope` for both activations).
 * H3 [n][F3], W1 [K1][F3], b1 [K1], A4 [n][K1], dA4 [n][K1], dH3 [n][F3] f32; F3 % 4 == 0,
 * K1 <= 128, C <= 16; H3, W1, W2 16-B aligned with leading dimensions multiples of 4. The two
 * products are computed exactly as pg_gemm_f32's three-piece kernel computes them (same
 * split, same k order and MFMA sequence), so A4 and dH3 equal its results bitwise. prob and
 * dz are optional (NULL). Scratch (256-B aligned): pg_mlp_l1_head_workspace(n, C, F3, K1)
 * bytes; F3 <= 4096. adam_state (optional, NULL = none): the launch also does
 * pg_adam_prepare(adam_state, lr, beta1, beta2)'s work (one per step, before pg_adam_apply),
 * so a training step needs one launch fewer. */
size_t pg_mlp_l1_head_workspace(int64_t n, int32_t C, int32_t F3, int32_t K1);
int pg_mlp_l1_head(const float* H3, int64_t ldh, int64_t n, int32_t F3, const float* W1, int64_t ldw1,
                   const float* b1, int32_t K1, float* A4, int64_t lda4, const float* W2, int64_t ldw,
                   const float* b2, int32_t C, const float* labels, int64_t ldl, const float* class_w,
                   const int8_t* row_set, int64_t n_train, int64_t n_val, float* prob, int64_t ldp,
                   float* dz, int64_t lddz, float* dA4, int64_t ldg, float* dH3, int64_t lddh, float slope,
                   float* loss2, void* ws, size_t ws_bytes, float* adam_state, double lr, double beta1,
                   double beta2, pg_stream_t stream);
/* (ABI 13) W1's three bf16 pieces kept by the caller instead of split in each call:
 * pg_mlp_l1_split writes them (two fragment-native layouts, pg_mlp_l1_pieces_bytes(F3, K1)
 * bytes, 256-B aligned) from W1; pg_mlp_l1_head_ex is pg_mlp_l1_head reading them (W1
 * itself is then not read); pg_adam_apply_l1 is pg_adam_apply over the n flat parameters
 * that also rewrites, for W1 = param + w1_offset ([K1][ldw1] inside the n), the pieces of
 * every element it updates: after it the pieces equal pg_mlp_l1_split of the new W1 bitwise,
 * so a training step needs no split launch. The pieces go stale if W1 is written any other
 * way: split again. Results are bitwise those of pg_mlp_l1_head / pg_adam_apply. */
size_t pg_mlp_l1_pieces_bytes(int32_t F3, int32_t K1);
int pg_mlp_l1_split(const float* W1, int64_t ldw1, int32_t F3, int32_t K1, void* pieces, pg_stream_t stream);
int pg_mlp_l1_head_ex(const float* H3, int64_t ldh, int64_t n, int32_t F3, const float* W1, int64_t ldw1,
                      const float* b1, int32_t K1, float* A4, int64_t lda4, const float* W2, int64_t ldw,
                      const float* b2, int32_t C, const float* labels, int64_t ldl, const float* class_w,
                      const int8_t* row_set, int64_t n_train, int64_t n_val, float* prob, int64_t ldp,
                      float* dz, int64_t lddz, float* dA4, int64_t ldg, float* dH3, int64_t lddh, float slope,
                      float* loss2, void* ws, size_t ws_bytes, float* adam_state, double lr, double beta1,
                      double beta2, const void* w1_pieces, pg_stream_t stream);
int pg_adam_apply_l1(float* param, const float* grad, float* exp_avg, float* exp_avg_sq, int64_t n,
                     const float* state, double beta1, double beta2, double eps, double weight_decay,
                     int64_t w1_offset, int64_t ldw1, int32_t F3, int32_t K1, void* w1_pieces,
                     pg_stream_t stream);
size_t pg_sigmoid_multi_loss_workspace(int64_t n_index, int32_t C);
int pg_sigmoid_multi_loss(const float* z, int64_t ldz, int64_t n_rows, int32_t C,
                          const float* labels, int64_t ldl, const float* class_w,
                          const int32_t* index, int64_t n_index, float* prob, int64_t ldp,
                          float* loss, float* dz, int64_t lddz, void* ws, size_t ws_bytes,
                          pg_stream_t stream);

/* Adam, torch 1.10 formula (code/train.py:180,205 with the pinned torch 1.10.0):
 *   m = m*b1 + (1-b1)*g;  v = v*b2 + (1-b2)*g*g;
 *   p = p + (-lr/bc1) * (m / (sqrt(v)/sqrt(bc2) + eps)),  bc_i = 1 - b_i^step
 * Hyper-parameters are doubles, as the Python floats torch receives; scalar factors are
 * formed in double and rounded to float once, like torch's scalar arguments.
 * state[0] = step count (float, exact to 2^24), advanced on the device by
 * pg_adam_prepare so a captured graph replays correctly; state[1..3] scratch. */
int pg_adam_prepare(float* state, double lr, double beta1, double beta2, pg_stream_t stream);
int pg_adam_apply(float* param, const float* grad, float* exp_avg, float* exp_avg_sq, int64_t n,
                  const float* state, double beta1, double beta2, double eps,
                  double weight_decay, pg_stream_t stream);

/* Epilogue of pg_gemm_f32 (NULL = plain C = alpha * op(A) op(B) + beta * C). */
typedef struct pg_gemm_epilogue {
  const float* bias; /* [N] row vector added after alpha*AB + beta*C, or NULL */
  int act;           /* PG_ACT_*: applied to the result, unless dact is given */
  float slope;       /* negative slope of PG_ACT_LEAKY */
  const float* dact; /* if not NULL: multiply the result by act'(dact[m][n]) instead, dact being
                        the activation OUTPUT (relu: dact > 0 ? 1 : 0; leaky: dact > 0 ? 1 : slope)
                        = the fused backward of relu / leaky_relu */
  int64_t lddact;
  float* rowsum;     /* if not NULL: rowsum[m] = sum_k op(A)[m][k] (overwritten). For a weight
                        gradient dY^T X (transa) these are the bias gradients sum_nodes dY. */
} pg_gemm_epilogue_t;

/* C[M,N] = alpha * op(A) * op(B) + beta * C, then the epilogue.
 * op(A) = A (M x K, lda) or A^T when transa (A stored K x M); op(B) = B (K x N) or B^T when
 * transb (B stored N x K). fp32 in, fp32 out, f32 accumulate on the matrix cores:
 *   - 16-B aligned operands whose contiguous extents and leading dimensions are multiples
 *     of 4: every element split into three bf16 pieces a = a_h + a_m + a_l, six piece
 *     products (h.h, h.m, m.h, h.l, l.h, m.m) on v_mfma_f32_32x32x16_bf16. Error per
 *     output <= ~1e-6 of sum_k |a b| (f32 level). Finite operands with |x| < 3.39e38
 *     only: an Inf or NaN operand gives NaN in its outputs (where f32 arithmetic could
 *     give +-Inf), and finite values that round to Inf in bf16 also give NaN.
 *   - otherwise: v_mfma_f32_32x32x2_f32 (f32 products, IEEE non-finite behaviour).
 * When split_k > 1, beta must be 0 or 1 and the epilogue may only carry rowsum (partials
 * are combined in the workspace, in slice order: deterministic). */
/* Recommended split_k for pg_gemm_f32 (long-K products such as weight gradients):
 * about five 64 x 64 workgroups per CU, each slice >= 96 entries of K, at most 256. */
int pg_gemm_f32_split_k(int64_t M, int64_t N, int64_t K);
size_t pg_gemm_f32_workspace(int64_t M, int64_t N, int64_t K, int split_k);
/* Deferred split-K: pg_gemm_f32_partials runs the split product (C = op(A) op(B), rowsum
 * allowed, nothing else) and leaves the partial slabs in ws (layout of pg_gemm_f32:
 * split_used slabs of M x N, then split_used row-sum slices of M); *split_used = the slice
 * count actually run. pg_gemm_splitk_reduce_batch then combines up to 16 such products in
 * one launch, C = alpha * sum_z slab_z (+ beta * C, beta 0 or 1), each exactly as
 * pg_gemm_f32's own combine (bitwise the same result). The ws regions must stay untouched
 * between the two calls. */
typedef struct pg_splitk_job {
  const float* ws;  /* the partials' workspace */
  int split_k;      /* *split_used of the partials call */
  int64_t M, N;
  float alpha, beta;
  float* C;
  int64_t ldc;
  float* rowsum;    /* or NULL (must match the partials call's ep->rowsum != NULL) */
} pg_splitk_job_t;
int pg_gemm_f32_partials(int transa, int transb, int64_t M, int64_t N, int64_t K, const float* A,
                         int64_t lda, const float* B, int64_t ldb, const pg_gemm_epilogue_t* ep,
                         int split_k, void* ws, size_t ws_bytes, int* split_used, pg_stream_t stream);
int pg_gemm_splitk_reduce_batch(const pg_splitk_job_t* jobs, int n_jobs, pg_stream_t stream);
/* Grouped split-K products (a training step's weight gradients, code/model.py:13-17
 * backward: they feed only the optimizer, so all of them can run at the end of the
 * backward): part p computes C_p = op(A_p) op(B_p) (+ C_p when beta_p = 1; beta 0 or 1)
 * and, if rowsum_p, rowsum_p = the row sums of op(A_p), as pg_gemm_f32 with no other
 * epilogue. The parts' tiles times one K-slice count for the whole group run as ONE
 * three-piece launch sized for the chip (so the partial slabs scale with the group's
 * workgroups, not with each product's), then one combine launch; deterministic. Parts
 * that are not all of one (transa, transb), or whose operands the three-piece kernel does
 * not take (16-B alignment, extents multiple of 4), run one after another as pg_gemm_f32.
 * Up to 16 parts. The workspace size depends on the shapes and flags only. */
typedef struct pg_gemm_part {
  int32_t transa, transb;
  int64_t M, N, K;
  const void* A; /* f32 (pg_gemm_f32_group) or bf16 bits (pg_gemm_bf16_group); C is f32 */
  int64_t lda;
  const void* B;
  int64_t ldb;
  float beta;
  float* C;
  int64_t ldc;
  float* rowsum; /* or NULL */
} pg_gemm_part_t;
size_t pg_gemm_f32_group_workspace(const pg_gemm_part_t* parts, int n_parts);
int pg_gemm_f32_group(const pg_gemm_part_t* parts, int n_parts, void* ws, size_t ws_bytes,
                      pg_stream_t stream);
int pg_gemm_f32(int transa, int transb, int64_t M, int64_t N, int64_t K, float alpha,
                const float* A, int64_t lda, const float* B, int64_t ldb, float beta, float* C,
                int64_t ldc, const pg_gemm_epilogue_t* ep, int split_k, void* ws,
                size_t ws_bytes, pg_stream_t stream);
/* pg_gemm_f32 with both operands given as two pieces concatenated along K (ABI 10):
 * C = alpha [A1 | A2] op([B1 ; B2]) + beta C (+ bias, leaky_relu), A1 M x K1, A2 M x K2 (not
 * transposed), op(B1) K1 x N, op(B2) K2 x N: the dgl shim's SAGEConv products
 * [H | M] [Wself | Wneigh]^T and [dY | dP] [Wself ; Wpool] without copying the pieces
 * together (code/model.py:13-15, 20-25). Three-piece kernel only: K1 a multiple of 4, each
 * piece's operands 16-B aligned with leading dimensions and contiguous extents multiples of
 * 4, else PG_ERR_UNSUPPORTED (the caller concatenates instead); ep: bias and act none |
 * leaky only. */
int pg_gemm_f32_cat(int transb, int64_t M, int64_t N, int64_t K1, int64_t K2, float alpha, const float* A1,
                    int64_t lda1, const float* A2, int64_t lda2, const float* B1, int64_t ldb1, const float* B2,
                    int64_t ldb2, float beta, float* C, int64_t ldc, const pg_gemm_epilogue_t* ep,
                    pg_stream_t stream);
/* Row-list product: for a sorted list rows[n_rows] (int32, device) of distinct row
 * ids below M, C[rows[i], :] = A[rows[i], :] op(B) (A [M][K] not transposed, op(B) K x N,
 * alpha 1, beta 0, no epilogue, no split-K). Rows of C that are not listed are neither read
 * nor written. Three-piece kernel only, tile chosen as for an n_rows x N product; every
 * element is summed in the same k order as in pg_gemm_f32's product, so the listed rows
 * equal its rows bitwise. Operands that kernel does not take (see pg_gemm_f32_cat):
 * PG_ERR_UNSUPPORTED, the caller runs the full product. n_rows == 0 launches nothing. */
int pg_gemm_f32_rows(int transb, int64_t M, int64_t N, int64_t K, const float* A, int64_t lda,
                     const float* B, int64_t ldb, float* C, int64_t ldc, const int32_t* rows,
                     int64_t n_rows, pg_stream_t stream);

/* ---------------- device: bf16 storage mode (f32 accumulate) ---------------- */

/* pg_gemm_f32's contract with bf16 operands (uint16 bits, row-major): op(A), op(B) bf16,
 * products on v_mfma_f32_32x32x16_bf16 with f32 accumulate; C is f32 (c_dtype =
 * PG_DTYPE_F32) or bf16 (PG_DTYPE_BF16, rounded to nearest even). The epilogue's bias and
 * rowsum are f32; C read for beta != 0 is in C's storage type; ep->dact points to bf16
 * values (activation outputs are stored bf16 in this mode).
 * Requirements: 16-B aligned A, B, C; lda, ldb multiples of 8; the contiguous extent of
 * each operand (K for A / B^T, M for A^T, N for B) a multiple of 8; N and ldc multiples of
 * 4; split_k > 1 only with an f32 C. Else PG_ERR_UNSUPPORTED. */
int pg_gemm_bf16_split_k(int64_t M, int64_t N, int64_t K);
size_t pg_gemm_bf16_workspace(int64_t M, int64_t N, int64_t K, int split_k);
/* pg_gemm_f32_group's contract with bf16 operands and f32 C (bf16 weight gradients): parts
 * of one (transa, transb) whose 256 x 256 tiles waste at most 4x their area run as one
 * split-K launch of the two-phase kernel (one K-slice count for the group, chosen so the
 * items fill whole rounds of one workgroup per CU) and one combine; the others (and all of
 * them when the operands break pg_gemm_bf16's layout rules) one after another as
 * pg_gemm_bf16. Up to 16 parts. */
size_t pg_gemm_bf16_group_workspace(const pg_gemm_part_t* parts, int n_parts);
int pg_gemm_bf16_group(const pg_gemm_part_t* parts, int n_parts, void* ws, size_t ws_bytes,
                       pg_stream_t stream);
int pg_gemm_bf16(int transa, int transb, int64_t M, int64_t N, int64_t K, float alpha,
                 const void* A, int64_t lda, const void* B, int64_t ldb, float beta, void* C,
                 int64_t ldc, int c_dtype, const pg_gemm_epilogue_t* ep, int split_k, void* ws,
                 size_t ws_bytes, pg_stream_t stream);
/* pg_spmm_max_fwd / pg_spmm_max_bwd on bf16 features (X, out, dout, mask_src, dx): the
 * max is a selection, so out holds the winning bf16 value exactly (u_mul_e products are
 * rounded to nearest even); the backward accumulates in f32 and rounds dx once. Same
 * workspace queries. The backward needs PG_ARG_U16 records and F <= 1024. */
int pg_spmm_max_fwd_bf16(const pg_csr_t* g, const void* X, int64_t ldx, int64_t F, void* out,
                         int64_t ldo, void* argpos, int64_t lda, int arg_kind, void* ws,
                         size_t ws_bytes, pg_stream_t stream);
int pg_spmm_max_bwd_bf16(const pg_csr_t* g, const pg_csr_t* gt, const void* argpos, int64_t lda,
                         int arg_kind, const void* dout, int64_t ldd, int64_t F,
                         const void* mask_src, int64_t ldm, const void* fwd_out, int64_t ldf,
                         void* dx, int64_t ldx, void* ws, size_t ws_bytes, pg_stream_t stream);
int pg_spmm_max_bwd_rows_bf16(const pg_csr_t* g, const pg_csr_t* gt, const void* argpos, int64_t lda,
                              int arg_kind, const void* dout, int64_t ldd, int64_t F,
                              const void* mask_src, int64_t ldm, const void* fwd_out, int64_t ldf,
                              void* dx, int64_t ldx, const int8_t* row_active, const int32_t* eslot_active,
                              void* ws, size_t ws_bytes, pg_stream_t stream);
/* dst[i] = bf16(src[map ? map[i] : i]) (map[i] < 0: 0), round to nearest even: the bf16
 * weight copies of the f32 master parameters, in any layout the GEMMs want. */
int pg_cast_f32_bf16(const float* src, const int32_t* map, int64_t n, void* dst, pg_stream_t stream);
int pg_cast_bf16_f32(const void* src, int64_t n, float* dst, pg_stream_t stream);

/* Zero-padded 2-D copies in one launch (ABI 11): for each part, dst[r][c] = src[r][c] for
 * r < rows, c < cols, else 0, over drows x dcols (row-major, leading dimensions lds / ldd).
 * The drop-in SAGEConv's padded weight images (503 -> 512: [Wpool], bpool, [Wself | Wneigh])
 * built from the layer's parameters each forward (code/model.py:13-15). */
#define PG_PAD2D_MAX 8
typedef struct pg_pad2d {
  const float* src;
  int64_t lds, rows, cols;
  float* dst;
  int64_t ldd, drows, dcols;
} pg_pad2d_t;
int pg_pad2d_group(const pg_pad2d_t* parts, int n, pg_stream_t stream);

/* The PCA front end (code/data_preprocess.py:475-487 `pca`, scikit-learn 1.1.1
 * PCA(n_components, random_state=42) on the ECC / GCN*PPI matrices, 528-546): its randomized
 * SVD's products with the centred matrix, float64, as a CSR x dense SpMM with a rank-1 term:
 *   Y[r, :] = sum_{j in row r} val[j] X[col[j], :] - (u ? u[r] : 1) * v[:]   (v NULL: no term)
 * k <= 512 columns. Sum in CSR order (deterministic). */
int pg_csr_spmm_f64(int64_t n_rows, const int32_t* ptr, const int32_t* col, const double* val,
                    const double* X, int64_t ldx, int64_t k, const double* u, const double* v,
                    double* Y, int64_t ldy, pg_stream_t stream);

/* ---------------- host (_cpu): the same operations on host pointers ---------------- */
int pg_spmm_max_fwd_cpu(const pg_csr_t* g, const float* X, int64_t ldx, int64_t F, float* out,
                        int64_t ldo, void* argpos, int64_t lda, int arg_kind);
int pg_spmm_max_bwd_cpu(const pg_csr_t* g, const pg_csr_t* gt, const void* argpos, int64_t lda,
                        int arg_kind, const float* dout, int64_t ldd, int64_t F,
                        const float* mask_src, int64_t ldm, float* dx, int64_t ldx);
int pg_spmm_sum_cpu(const pg_csr_t* g, const float* X, int64_t ldx, int64_t F, int norm_mode,
                    const int32_t* norm_ptr, float* out, int64_t ldo);
int pg_argpos_to_src_cpu(const pg_csr_t* g, const void* argpos, int64_t lda, int arg_kind,
                         int64_t F, int64_t* argx, int64_t ldx);
/* f32 accumulation in ascending f, OpenMP over rows; needs no work schedule. */
int pg_sddmm_dot_cpu(const pg_csr_t* g, const float* D, int64_t ldd, const float* X, int64_t ldx,
                     int64_t F, int norm_mode, const void* argpos, int64_t lda, int arg_kind,
                     float* de);
/* The multi-head entry points on host pointers: row reductions (softmax, sum) in ascending
 * k, dot products in ascending j, OpenMP over rows; no work schedule, no workspace. */
int pg_edge_softmax_fwd_cpu(const pg_csr_t* g, const float* s, int64_t lds, int32_t H, float* a,
                            int64_t lda);
int pg_edge_softmax_bwd_cpu(const pg_csr_t* g, const float* a, int64_t lda, const float* da,
                            int64_t ldda, int32_t H, float* ds, int64_t ldds);
int pg_spmm_sum_heads_cpu(const pg_csr_t* g, const float* A, int64_t lda, int32_t H,
                          const float* X, int64_t ldx, int64_t Fh, float* out, int64_t ldo);
int pg_sddmm_dot_heads_cpu(const pg_csr_t* g, const float* Dm, int64_t ldd, const float* X,
                           int64_t ldx, int32_t H, int64_t Fh, float* de, int64_t lde);
/* pg_gspmm / pg_gsddmm on host pointers: every row reduced in ascending k (a split row is
 * not cut), OpenMP over rows; no work schedule, no workspace. */
int pg_gspmm_cpu(const pg_csr_t* g, int op, int reduce, const float* L, int64_t ldl, int lt,
                 const float* R, int64_t ldr, int rt, const int32_t* eidx, int64_t F,
                 int norm_mode, float* out, int64_t ldo, void* argpos, int64_t lda, int arg_kind);
int pg_gsddmm_cpu(const pg_csr_t* g, int op, const float* L, int64_t ldl, int lt, const float* R,
                  int64_t ldr, int rt, const int32_t* eidx, int64_t F, float* out, int64_t ldo,
                  const void* argpos, int64_t lda, int arg_kind);
/* pg_gatv2_score / pg_gatv2_bwd on host pointers: every row reduced in ascending k, dot
 * products in ascending d, dattn in ascending k per column; OpenMP over rows (dattn: over
 * columns); no work schedule, no workspace. */
int pg_gatv2_score_cpu(const pg_csr_t* g, const float* XL, int64_t ldl, const float* XR, int64_t ldr,
                       const float* attn, int32_t H, int64_t Fh, float slope, float* s, int64_t lds);
int pg_gatv2_bwd_cpu(const pg_csr_t* g, const float* ds, int64_t ldds, const float* Xown,
                     int64_t ldown, const float* Xgat, int64_t ldgat, const float* attn, int32_t H,
                     int64_t Fh, float slope, float* dXown, int64_t lddx, float* dattn);

/* The sampling primitives on host pointers: the statement of their results (the device
 * entry points equal them bit for bit). No workspace; *n_src is a host int32. */
int pg_sample_count_cpu(const pg_csr_t* g, const int32_t* seeds, int64_t n_seeds, int32_t fanout,
                        int32_t* out_ptr);
int pg_sample_fill_cpu(const pg_csr_t* g, const int32_t* eid, const int32_t* seeds, int64_t n_seeds,
                       int32_t fanout, uint64_t seed64, const int32_t* out_ptr, int32_t* out_col,
                       int32_t* out_eid);
int pg_block_compact_cpu(const int32_t* dst_ids, int64_t n_dst, const int32_t* col, int64_t nnz,
                         int64_t n_parent, int32_t* src_ids, int32_t* col_local, int32_t* n_src);

/* The link-prediction primitives on host pointers: the statement of their results (the plain
 * exact selection; the device entry points equal them bit for bit). No workspace; *status and
 * *n_fail are host int32 (status written on an out-of-range id only, n_fail always). */
int pg_edge_bits_update_cpu(uint32_t* bits, int64_t n_edge_ids, const int32_t* eids, int64_t n, int set,
                            int32_t* status);
int pg_sample_count_excl_cpu(const pg_csr_t* g, const int32_t* eid, const int32_t* seeds, int64_t n_seeds,
                             int32_t fanout, const uint32_t* excl_bits, int32_t* out_ptr);
int pg_sample_fill_excl_cpu(const pg_csr_t* g, const int32_t* eid, const int32_t* seeds, int64_t n_seeds,
                            int32_t fanout, uint64_t seed64, const uint32_t* excl_bits,
                            const int32_t* out_ptr, int32_t* out_col, int32_t* out_eid);
int pg_edge_lookup_cpu(const pg_csr_t* g, const int32_t* eid, const int32_t* u, const int32_t* v, int64_t n,
                       int32_t* out_eid);
int pg_negative_sample_cpu(const pg_csr_t* g, const int32_t* pos_src, const int32_t* pos_id, int64_t n_pos,
                           int32_t k, int32_t tries, int flags, uint64_t seed64, int32_t* neg_src,
                           int32_t* neg_dst, int32_t* n_fail);

/* ---------------- device: §8f — edge clustering coefficient ---------------- */

/* code/data_preprocess.py:175-214 edge_clustering_coefficients on a symmetric adjacency
 * in CSR form (sorted, unique column ids per row):
 *   ecc[k] for entry k = (i, j), i != j:
 *     epsilon if min(deg_i, deg_j) - 1 == 0, else |N(i) ∩ N(j)| / (min(deg_i, deg_j) - 1)
 *   deg = row sums of the stored values (NULL: row lengths); diagonal entries get 0.
 * mirror[k] = index of the entry (j, i); order = any permutation of the rows, or NULL for
 * 0..n-1 (speed only: longest first balances the workgroups; the result does not depend on it).
 * n <= 1 310 720: the neighbour bitmap of a row lives in LDS, one bit per node in at most
 * 160 KB (above 64 KB fewer workgroups share a CU). Larger n: PG_ERR_UNSUPPORTED up to 2^22,
 * PG_ERR_INVALID beyond. n == 0 or nnz == 0 writes nothing. Bit-exact (integer counts, one
 * f64 division). */
int pg_ecc(const int32_t* ptr, const int32_t* col, const int32_t* mirror, const double* deg,
           const int32_t* order, int64_t n, int64_t nnz, double epsilon, double* ecc,
           pg_stream_t stream);

/* ---------------- device: §8f — per-epoch evaluation ---------------- */

/* code/train.py:19-39 protein_loc_correction on proba[n][C] (float32, C <= 64):
 *   new = (p - colmin) / (colmax - colmin); new /= rowsum(new);
 *   pred[r][c] = new > rowmax - (rowmax - rowmin) * (float)alpha ? 1.0 : 0.0  (float64)
 * code/train.py:42-86 performances_record: out3 = {aim, coverage, accuracy}, the row terms
 * summed in row order in float32 and divided by n, as the reference's running scalars.
 * Scratch: pg_loc_eval_workspace(n, C) bytes. */
size_t pg_loc_eval_workspace(int64_t n, int32_t C);
int pg_loc_correction(const float* proba, int64_t ldp, int64_t n, int32_t C, double alpha,
                      double* pred, int64_t ldpred, void* ws, size_t ws_bytes, pg_stream_t stream);
int pg_loc_performance(const float* loc_true, int64_t ldt, const double* loc_pred, int64_t ldp,
                       int64_t n, int32_t C, double* out3, void* ws, size_t ws_bytes,
                       pg_stream_t stream);

/* ---------------- device: §8f — topology perturbation ---------------- */

/* code/data_preprocess.py:165-170 (np.corrcoef of the expression rows, diagonal and NaN
 * set to 0) for the normal and the intervention state, and :217-257
 * modify_network_topology on their difference, without materialising any N x N matrix.
 * xc_*: [n][S] float64 CENTRED expression rows (x - x.mean(axis=1), computed by the
 * caller as numpy does), 2 <= S <= 8; inv_fact = 1 / (S - 1).
 *   pcc(i, j) = clip(((fma-chain dot(xc_i, xc_j)) * inv_fact) / sd_i / sd_j, -1, 1),
 *               0 on the diagonal and where NaN;  sd_i = sqrt(dot(xc_i, xc_i) * inv_fact)
 *   diff(i, j) = pcc_inter(i, j) - pcc_normal(i, j)
 * pg_perturb_prepare: sd_* [n].
 * pg_perturb_sum: *total = sum over all n*n entries of diff (squared = 0) or of
 *   (diff - mean)^2 (squared = 1); compensated f64, deterministic. Scratch:
 *   pg_perturb_workspace(n) bytes. The caller forms mean = total / n^2,
 *   std = sqrt(total_sq / n^2), lo_thr = mean - thr * std, hi_thr = mean + thr * std.
 * pg_perturb_count / pg_perturb_fill: the perturbed adjacency, given the original as CSR
 *   (sorted unique columns per row; val = stored int64 values, NULL = all ones):
 *   v' = 0 if v == 1 and diff < lo_thr;  1 if v == 0 and diff > hi_thr;  v otherwise.
 *   count: non-zeros per row; fill: column ids and values of the non-zeros, row-major,
 *   ascending columns, row i starting at offsets[i]. n <= 1 310 720 (LDS row bitmap). */
size_t pg_perturb_workspace(int64_t n);
int pg_perturb_prepare(const double* xc_normal, const double* xc_inter, int64_t n, int32_t S,
                       double inv_fact, double* sd_normal, double* sd_inter, pg_stream_t stream);
int pg_perturb_sum(const double* xc_normal, const double* xc_inter, const double* sd_normal,
                   const double* sd_inter, int64_t n, int32_t S, double inv_fact, int squared,
                   double mean, double* total, void* ws, size_t ws_bytes, pg_stream_t stream);
int pg_perturb_count(const double* xc_normal, const double* xc_inter, const double* sd_normal,
                     const double* sd_inter, int64_t n, int32_t S, double inv_fact,
                     const int32_t* ptr, const int32_t* col, const int64_t* val, double lo_thr,
                     double hi_thr, int32_t* counts, pg_stream_t stream);
int pg_perturb_fill(const double* xc_normal, const double* xc_inter, const double* sd_normal,
                    const double* sd_inter, int64_t n, int32_t S, double inv_fact,
                    const int32_t* ptr, const int32_t* col, const int64_t* val, double lo_thr,
                    double hi_thr, const int64_t* offsets, int32_t* out_col, int64_t* out_val,
                    pg_stream_t stream);

/* ---------------- misc ---------------- */
const char* pg_last_error_string(void);
int pg_version(void); /* 2: pg_csr_t.einv; 3: pg_spmm_max_bwd fwd_out; 5: no in-kernel split-K
                         (epilogue without splitk_cnt), no grouped SpMM pair; 6: with fwd_out,
                         pg_spmm_max_bwd[_bf16] takes mask_src >= 0 and does not read it;
                         PG_ARG_DEAD_NONE; 7: pg_spmm_max_bwd reads no einv, smaller
                         workspace; 8: pg_csr_t without einv; max backward lists as 8-B
                         records with the edge weight folded in; with fwd_out alone the
                         relu' mask is applied, only PG_ARG_DEAD_NONE implies it;
                         9: pg_gemm_f32_group; 10: the in-CSR's epos = transposed
                         indices (transposed max-backward descriptors), pg_gemm_f32_cat;
                         11: pg_pad2d_group; 12: pg_mlp_l1_head;
                         13: pg_mlp_l1_split, pg_mlp_l1_head_ex, pg_adam_apply_l1;
                         13 also: pg_sddmm_dot; pg_edge_softmax_fwd / _bwd,
                         pg_spmm_sum_heads, pg_sddmm_dot_heads and their _cpu twins;
                         13 also (additions only, so the number the suite pins stays):
                         pg_gemm_f32_rows, pg_spmm_max_bwd_rows[_bf16] (the top layer's
                         backward on the train rows only);
                         13 also: pg_gspmm, pg_gspmm_workspace, pg_gsddmm and their _cpu
                         twins (vector edge features);
                         13 also: pg_gatv2_score, pg_gatv2_bwd, pg_gatv2_bwd_workspace and
                         the _cpu twins of the first two (fused GATv2 attention scores);
                         13 also: pg_sample_count, pg_sample_fill,
                         pg_block_compact, their workspace queries and _cpu twins
                         (neighbour sampling and block compaction);
                         13 also: pg_csr_transpose_dev, pg_schedule_count_dev,
                         pg_schedule_build_dev and their workspace queries (a sampled
                         block's transpose and schedules on the device);
                         13 also: pg_edge_bits_update, pg_sample_count_excl,
                         pg_sample_count_excl_workspace, pg_sample_fill_excl, pg_edge_lookup,
                         pg_negative_sample and the _cpu twins of the five (link-prediction
                         mini-batches) */

#ifdef __cplusplus
}
#endif
#endif /* PLAGNN_H */
