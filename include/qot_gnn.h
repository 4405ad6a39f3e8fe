/*
 * qot_gnn.h -- C ABI of libqot_gnn.so, the MI355X (gfx950) message-passing engine that
 * replaces the torch_geometric operator layer under the reference's two models.
 *
 * Reference interface each entry point replaces (paths relative to the reference repo;
 * [PyG-ext] = third-party torch_geometric code reached from that line):
 *
 *   qot_csr_build            edge_index handling inside every conv call:
 *                            topological_training/models.py:53,57 and
 *                            lightpath_training/models.py:30 ([PyG-ext] propagate's
 *                            index_select/scatter bookkeeping; GATConv's
 *                            remove_self_loops + add_self_loops)
 *   qot_embed_{fwd,bwd}      topological_training/models.py:12,51-52  (nn.Embedding lookup)
 *   qot_tconv_*              topological_training/models.py:15-17,53 ([PyG-ext] TransformerConv)
 *   qot_nnconv_*             topological_training/models.py:20-30,57 ([PyG-ext] NNConv aggr="mean")
 *   qot_act_{fwd,bwd}        topological_training/models.py:54-55,58-59 (leaky_relu + Dropout)
 *   qot_pool_{fwd,bwd}       topological_training/models.py:61 ([PyG-ext] global_mean_pool)
 *   qot_gat_*                lightpath_training/models.py:13,30 ([PyG-ext] GATConv heads=4)
 *   qot_bn_*                 lightpath_training/models.py:14,31-32 ([PyG-ext] BatchNorm + relu)
 *   qot_rows_gather/scatter  lightpath_training/models.py:39-40 (x[lut_mask] and its adjoint)
 *
 * Conventions
 *   - Stateless and stream-ordered: every call only enqueues work on `stream`
 *     (a hipStream_t passed as void*); the library never allocates, frees or synchronises.
 *     All outputs and workspaces are caller-allocated DEVICE memory.
 *   - Return value: 0 = ok; >0 = hipError_t of the failed launch/runtime call;
 *     <0 = QOT_ERR_* argument error.  qot_error_string() describes either.
 *   - Feature matrices are row-major fp32.  `ld` arguments are row strides in floats, so a
 *     packed [N, 4H] projection output can be passed as four column slices.
 *   - Indices inside the library are int32 (N, E < 2^31); the int64 edge_index of the
 *     reference contract is consumed only by qot_csr_build.
 *   - Supported widths: H (and heads*C) power of two in [16, 256] (heads*C up to 1024),
 *     edge_dim D in {1..8} for TransformerConv and for the NNConv building blocks qot_nnconv_agg /
 *     qot_nnconv_bwd_edge; the FUSED NNConv tile kernels (qot_nnconv_fused, qot_nnconv_adjoint_dw,
 *     qot_nnconv_gradh_fused, qot_nnconv_dw) are built for D <= 4 (K = 2D <= 8 operand blocks per LDS tile)
 *     and return QOT_ERR_UNSUPPORTED above it -- the host side (functional.NNConvFn) then runs
 *     {qot_nnconv_agg, GEMM, qot_nnconv_bwd_edge}.  Anything else returns QOT_ERR_UNSUPPORTED (callers must
 *     fail loudly; there is no CPU fallback).
 */
#ifndef QOT_GNN_H
#define QOT_GNN_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef void* qot_stream_t; /* hipStream_t */

#define QOT_ABI_VERSION 13
#define QOT_OK 0
#define QOT_ERR_UNSUPPORTED (-1) /* width / edge_dim not instantiated */
#define QOT_ERR_BADARG (-2)      /* null pointer, negative size, workspace too small */

int qot_abi_version(void);
const char* qot_error_string(int code);

/* ---- graph preparation ------------------------------------------------------------
 * Builds, from edge_index[2,E] (int64, row 0 = source j, row 1 = target i):
 *   CSR by destination : rowptr[N+1], col[cap] (source of each in-edge), eid[cap]
 *                        (original edge id, or -1 for an inserted self loop), row[cap]
 *                        (destination of each CSR slot)
 *   CSC by source      : rowptr_t[N+1], col_t[cap] (destination of each out-edge),
 *                        pos_t[cap] (CSR slot of that edge), eid_t[cap] (its original edge id)
 * cap = E (+ N when gat_self_loops).  Edge order inside a destination follows the
 * original edge order (stable), so results are run-to-run bitwise reproducible.
 * gat_self_loops != 0: edges with j == i are dropped and one (n,n) edge per node is
 * appended (GATConv semantics); the live edge count is rowptr[N] (device side).
 * invdeg[N] = 1 / max(in_degree, 1).
 */
size_t qot_csr_workspace_bytes(int64_t E, int64_t N, int gat_self_loops);
int qot_csr_build(const int64_t* edge_index, int64_t E, int64_t N, int gat_self_loops,
                  int32_t* rowptr, int32_t* col, int32_t* eid, int32_t* row,
                  int32_t* rowptr_t, int32_t* col_t, int32_t* pos_t, int32_t* eid_t, float* invdeg,
                  void* workspace, size_t workspace_bytes, qot_stream_t stream);
/* Same index for a BLOCK-DIAGONAL batch whose graphs keep their nodes and edges contiguous (what a
 * collate produces; PyG's Batch keeps the same slices): node_ptr[B+1], edge_ptr[B+1] (int64, device)
 * give graph b's node / edge ranges, max_nodes / max_edges bound the largest graph (host-known).
 * One launch, one workgroup per graph, everything in LDS: no global atomics, no workspace.  Output
 * identical to qot_csr_build(gat_self_loops = 0).  Returns QOT_ERR_UNSUPPORTED when the largest graph
 * does not fit LDS ((4 max_nodes + 6 max_edges) * 4 bytes > 144 KB, or max_nodes > 65535): use
 * qot_csr_build then.
 * status (optional, device int32, caller-zeroed): bit 0 = an edge leaves its graph's node range,
 * bit 1 = a graph exceeds max_nodes / max_edges.
 * Optional by-products of the same pass (NULL to skip): with node_ids[N] (int64) the TransformerConv
 * table-mode maps ids32[N] = node_ids, colf[E] = node_ids[col], colf_t[E] = node_ids[col_t]
 * (qot_table_maps); ptr32[B+1] = node_ptr narrowed to int32 (read-out boundaries). */
int qot_csr_build_by_graph(const int64_t* edge_index, int64_t E, int64_t N, const int64_t* node_ptr,
                           const int64_t* edge_ptr, int64_t B, int64_t max_nodes, int64_t max_edges,
                           int32_t* rowptr, int32_t* col, int32_t* eid, int32_t* row, int32_t* rowptr_t,
                           int32_t* col_t, int32_t* pos_t, int32_t* eid_t, float* invdeg, int32_t* status,
                           const int64_t* node_ids, int32_t* ids32, int32_t* colf, int32_t* colf_t, int32_t* ptr32,
                           qot_stream_t stream);
/* GATConv's self-looped index (qot_csr_build with gat_self_loops = 1: PyG GATConv rebuilds it in every call,
 * lightpath_training/models.py:30) of a block-diagonal batch of SMALL graphs -- LightpathGNN's chain graphs of 2..20
 * nodes -- in one launch, one wave per graph.  Requires max_nodes <= 64, max_edges <= 256
 * (qot_csr_gat_by_graph_supported; QOT_ERR_UNSUPPORTED otherwise) and an input WITHOUT self loops: then graph b owns the
 * slots [edge_ptr[b] + node_ptr[b], ... + m + n) whatever the other graphs hold.  Output bit for bit qot_csr_build's.
 * status (optional, device int32): bits 0 / 1 as qot_csr_build_by_graph, bit 2 = a self loop was met (the index is
 * then wrong: rebuild with qot_csr_build).  ptr32 (optional): node_ptr narrowed to int32. */
int qot_csr_gat_by_graph_supported(int64_t max_nodes, int64_t max_edges);
int qot_csr_build_gat_by_graph(const int64_t* edge_index, int64_t E, int64_t N, const int64_t* node_ptr,
                               const int64_t* edge_ptr, int64_t B, int64_t max_nodes, int64_t max_edges, int32_t* rowptr,
                               int32_t* col, int32_t* eid, int32_t* row, int32_t* rowptr_t, int32_t* col_t, int32_t* pos_t,
                               int32_t* eid_t, float* invdeg, int32_t* status, int32_t* ptr32, qot_stream_t stream);
/* out[i] = map[idx[i]] (int32): table row of every CSR / CSC slot's source / destination
 * (node_ids[col], node_ids[col_t]) for TransformerConv's table mode.  idx values must be < len(map). */
int qot_i32_gather(const int32_t* map, const int32_t* idx, int32_t* out, int64_t n, qot_stream_t stream);
/* int64 -> int32 narrowing of node_ids / batch vectors */
int qot_i64_to_i32(const int64_t* in, int32_t* out, int64_t n, qot_stream_t stream);
/* ptr[B+1] from a sorted batch vector */
int qot_batch_ptr(const int32_t* batch, int64_t N, int64_t B, int32_t* ptr, qot_stream_t stream);

/* ---- embedding -------------------------------------------------------------------- */
int qot_embed_fwd(const float* table, const int32_t* ids, float* out, int64_t N, int V, int H,
                  qot_stream_t stream);
/* grad_table must be zero-filled by the caller; accumulates with per-workgroup LDS
 * pre-reduction then float atomics. */
int qot_embed_bwd(const float* grad_out, const int32_t* ids, float* grad_table, int64_t N, int V,
                  int H, qot_stream_t stream);

/* ---- TransformerConv (heads=1) ----------------------------------------------------
 * fwd: out_i = sum_e softmax_e(<q_i, k_j + We ea_e>/sqrt(H)) (v_j + We ea_e) + skip_i
 * stats[N,2] = (max logit, denominator incl. 1e-16) saved for backward.
 * edge_attr is in ORIGINAL edge order ([E,D]); the kernels index it through eid.
 * act != 0 fuses dropout(leaky_relu(out, act_slope), act_p) into the epilogue with the mask of
 * qot_act_fwd/qot_act_bwd (same seed / step counter / element indexing), so the backward is
 * qot_act_bwd(grad, out) followed by the conv backward.
 * Table mode (rowmap != NULL): q/k/v/skip are rows of a PROJECTED EMBEDDING TABLE [V, 4H]
 * ((emb W^T + b)[node_ids] == (emb[node_ids]) W^T + b, topological_training/models.py:51-53);
 * rowmap[i] = table row of node i and `col` must then hold the table row of each in-edge's source
 * (node_ids[col]).  NULL: one row per node, as produced by a node-level GEMM.
 */
/* qot_tconv_fwd in table mode with the logits' dense part <q_i, k_j> looked up in scores[V, ld_scores] = T_q T_k^T
 * (unscaled; qot_gemm_nt on the projected table) instead of gathered and multiplied per edge: rowmap (required) = table row
 * of every node, col = table row of every in-edge's source.  Same results up to the order of the H-term dot. */
int qot_tconv_fwd_scores(const float* q, const float* v, const float* skip, int ld, const float* scores, int ld_scores,
                         const float* edge_attr, const float* w_edge, const int32_t* rowptr, const int32_t* col,
                         const int32_t* eid, const int32_t* rowmap, float* out, float* stats, int64_t N, int H, int D,
                         int act, float act_slope, float act_p, uint64_t act_seed, const int64_t* act_step,
                         qot_stream_t stream);
/* Row form of TransformerConv's backward in table mode for large tables (csrc/tconv_rows.hip; autograd of
 * TransformerConv.propagate under loss.backward(), topological_training/train.py:115, with x = emb[node_ids],
 * models.py:51-53, and node_ids == arange(n) in each of the B graphs, dataset.py:78): no per-node grad_q / grad_k --
 * grad M[r_i, r_j] += ds_e on the score matrix of qot_tconv_fwd_scores, from which the caller forms
 * grad T_q = (grad M T_k + grad P W_e^T) / sqrt(H) and grad T_k = grad M^T T_q / sqrt(H).
 * qot_tconv_bwd_dst_rows: a workgroup owns table row r for one of `parts` slices of the graphs; leaves parts * n partial
 * rows (row part * n + r) of qot_tconv_rows_ld(n, H, D) floats, [grad T_skip (H) | grad M (qot_tconv_rows_npad(n): n
 * rounded up to 32, the tail zero) | grad P (D)], parts * n rows of H * D lin_edge partials (sum of g_i[c] p2_i[d]; the
 * T_q part of that gradient is rs * T_q^T grad P), grad_skip [N, H] (gradient wrt the conv output behind the fused
 * activation), escr [slots, 2] = (a_e, ds_e) for the source pass, and delta.  qot_tconv_bwd_src_rows: parts * n partial
 * rows of grad T_v (H).  The grad M rows are summed as 64-bit fixed point whose power-of-two scale every workgroup takes
 * from its own largest |ds_e| and addend count (relative precision at any gradient scale, bit-reproducible, homogeneous
 * in grad_out); a workgroup that meets a NaN / Inf ds_e leaves its whole grad M row NaN.
 * The caller sums the `parts` row blocks in order.  H in {64, 128, 256}; qot_tconv_rows_supported(n, H, D). */
int qot_tconv_rows_supported(int n, int H, int D);
int qot_tconv_rows_npad(int n);
int qot_tconv_rows_ld(int n, int H, int D);
int qot_tconv_bwd_dst_rows(const float* grad_out, const float* q, const float* v, int ld, const float* edge_attr,
                           const float* w_edge, const float* stats, const int32_t* rowptr, const int32_t* colf,
                           const int32_t* eid, const float* scores, int ld_scores, float* grad_skip, float* escr, float* delta,
                           const float* y_act, float act_slope, float act_p, uint64_t act_seed, const int64_t* act_step, int n,
                           int64_t B, int parts, float* part_rows, float* wedge_partials, int H, int D, qot_stream_t stream);
/* forward of the row form: out / stats bit-equal to qot_tconv_fwd_scores; a workgroup owns table row r for one of `parts`
 * slices of the B graphs (row r of the score matrix staged once, q_r W_e and the skip row in registers) */
int qot_tconv_fwd_rows(const float* q, const float* v, const float* skip, int ld, const float* scores, int ld_scores,
                       const float* edge_attr, const float* w_edge, const int32_t* rowptr, const int32_t* colf, const int32_t* eid,
                       float* out, float* stats, int n, int64_t B, int parts, int H, int D, int act, float act_slope, float act_p,
                       uint64_t act_seed, const int64_t* act_step, qot_stream_t stream);
int qot_tconv_bwd_src_rows(const float* grad_skip, const float* escr, const int32_t* rowptr_t, const int32_t* col_t,
                           const int32_t* pos_t, int n, int64_t B, int parts, float* part_rows, int H, qot_stream_t stream);
int qot_tconv_fwd(const float* q, const float* k, const float* v, const float* skip, int ld,
                  const float* edge_attr, const float* w_edge, const int32_t* rowptr,
                  const int32_t* col, const int32_t* eid, const int32_t* rowmap, float* out,
                  float* stats, int64_t N, int H, int D, int act, float act_slope, float act_p,
                  uint64_t act_seed, const int64_t* act_step, qot_stream_t stream);
/* Forward in the TILE form of table mode (rowmap != NULL, node_ids == arange(tile_n) in each of the tile_B graphs, N = tile_n *
 * tile_B; col = table row of every in-edge's source): a workgroup takes node r of qot_tconv_rows_per_block(H) consecutive
 * graphs, forms row r of T_q T_k^T / sqrt(H) once in LDS, and an in-edge costs one lookup there instead of a key-row
 * gather + dot + lane reduction.  Same results as qot_tconv_fwd up to the order of that dot.  tile_n <= 12288. */
int qot_tconv_fwd_tile(const float* q, const float* k, const float* v, const float* skip, int ld,
                       const float* edge_attr, const float* w_edge, const int32_t* rowptr, const int32_t* col,
                       const int32_t* eid, const int32_t* rowmap, float* out, float* stats, int64_t N, int H, int D,
                       int tile_n, int64_t tile_B, int act, float act_slope, float act_p, uint64_t act_seed,
                       const int64_t* act_step, qot_stream_t stream);
/* bwd, destination pass: grad_q[N,H] (ld_g), grad_skip[N,H] (= grad wrt the conv output, same ld_g;
 * may be NULL), per-edge scratch escr[cap,2] = (alpha, dalpha), delta[N], pds[N,D] = sum_e ds_e ea_e,
 * pal[N,D] = sum_e alpha_e ea_e.
 * y_act != NULL: grad_out is the gradient wrt y = dropout(leaky_relu(conv)) (the epilogue qot_tconv_fwd
 * fused, models.py:54-55) and y_act is that output; the kernel goes back through the activation
 * itself, so grad_skip then holds the gradient wrt the conv output -- pass IT (ld_go = ld_g) to
 * qot_tconv_bwd_src.  grad_w_edge != NULL: grad of lin_edge.weight [H,D] is produced as well
 * (fixed-order block partials; workspace qot_tconv_bwd_dst_workspace_floats(N,H,D) floats),
 * in the same launch.
 * Tile mode (grad_part != NULL; table mode with node_ids == arange(tile_n) for each of the tile_B graphs,
 * N = tile_n * tile_B): a workgroup takes node r of RPB = qot_tconv_rows_per_block(H) consecutive graphs and pre-reduces the
 * table gradient over them: grad_part[ceil(tile_B/RPB), tile_n, 4H] receives the partial sums of
 * grad_q (columns 0..H) and grad_skip (3H..4H) here and of grad_k / grad_v (H..3H) in qot_tconv_bwd_src;
 * the caller sums its first axis.  grad_q may then be NULL; grad_skip[N,H] is still written per node
 * (the source pass gathers it).
 * destinations per workgroup of the TransformerConv kernels at width H (1024/H today; callers size grad_part and the
 * workspace from this query, not from the formula); 0 for an unsupported width.
 * grad_w_edge == NULL with workspace != NULL: the per-workgroup partials [qot_tconv_bwd_dst_blocks(...), H*D] are
 * left in the workspace for the caller to sum (QOT_ROLE_SUM_ROWS of the step's backward epilogue). */
int qot_tconv_rows_per_block(int H);
int64_t qot_tconv_bwd_dst_blocks(int64_t N, int H, int tile_n, int64_t tile_B);
size_t qot_tconv_bwd_dst_workspace_floats(int64_t N, int H, int D);
int qot_tconv_bwd_dst(const float* grad_out, const float* q, const float* k, const float* v, int ld,
                      const float* edge_attr, const float* w_edge, const float* stats,
                      const int32_t* rowptr, const int32_t* col, const int32_t* eid,
                      const int32_t* rowmap, float* grad_q, float* grad_skip, int ld_g, float* escr,
                      float* delta, float* pds, float* pal, const float* y_act, float act_slope, float act_p,
                      uint64_t act_seed, const int64_t* act_step, float* grad_w_edge, float* workspace,
                      int tile_n, int64_t tile_B, float* grad_part, int64_t N, int H, int D, qot_stream_t stream);
/* bwd, source pass: grad_k, grad_v [N,H] (ld_g).  qmap_t (table mode, else NULL): table row of
 * each out-edge's destination (node_ids[col_t]) for the q gather; grad_out (row stride ld_go) and
 * delta stay per node. */
int qot_tconv_bwd_src(const float* grad_out, int ld_go, const float* q, int ld, const float* escr,
                      const float* delta, const int32_t* rowptr_t, const int32_t* col_t,
                      const int32_t* pos_t, const int32_t* qmap_t, float* grad_k, float* grad_v,
                      int ld_g, int tile_n, int64_t tile_B, float* grad_part, int64_t N, int H,
                      qot_stream_t stream);

/* ---- TransformerConv, table mode, GRAPH form (csrc/tconv_graph.hip) -----------------
 * The reference's only mode (topological_training/models.py:51-53 with dataset.py:78): x = node_embeddings(node_ids),
 * node_ids == arange(n) in each of the B graphs, so q / k / v / skip rows are rows of the projected table t4 [V, 4H]
 * (ld floats per row) and the dense part of a logit is an entry of the score matrix
 *     M [n, qot_tconv_graph_ldm(n)] = T_q T_k^T / sqrt(H),      P [n, D] = T_q w_edge / sqrt(H)
 * (qot_table_scores forms both from the PARAMETERS: table [V,H], lin_query, lin_key, lin_edge).  A workgroup takes
 * whole graphs (graph b owns nodes [b n, (b+1) n) and the index slots [rowptr[b n], rowptr[(b+1) n)) of the
 * block-diagonal batch) with M and T_v in LDS.  colf = node_ids[col] (= the source's index inside its graph).
 * qot_tconv_graph_supported(n, max_e, H, D): n <= 128 and the LDS images fit (max_e = most edges of one graph);
 * the entry points return QOT_ERR_UNSUPPORTED otherwise and callers use qot_tconv_fwd / qot_tconv_bwd_*.
 * fwd: out [N,H] as qot_tconv_fwd (same fused activation, same dropout mask); row = the index's destination of every
 * CSR slot.  Left behind for the backward (it needs no logits): alpha [E] = the attention weights, ea_csr [E,D] = the
 * edge features, both in CSR slot order, and aa [N,D] = sum_e alpha_e ea_e per destination.
 * bwd: grad_out [N,H] (through the fused activation when y_act != NULL, as qot_tconv_bwd_dst) ->
 * partials [qot_tconv_bwd_graph_blocks(B)][qot_tconv_graph_row_floats(n,H,D)], one row per workgroup:
 *     [ grad T_v n*H | grad T_skip n*H | grad M n*ldm | grad P n*D | grad w_edge (value path) H*D ]   (parts padded to 4 floats)
 * The caller sums the rows in order (QOT_ROLE_SUM_ROWS: bitwise reproducible).
 * qot_table_project_bwd_scores is qot_table_project_bwd fed by that summed row S: it forms
 *     grad T_q = (grad M T_k + grad P w_edge^T) / sqrt(H),   grad T_k = grad M^T T_q / sqrt(H)
 * where it needs them (rows >= n of the table receive zero) -- the [V, 4H] table gradient is never materialised -- and
 * completes grad w_edge [H,D] = S's value-path share + T_q^T grad P / sqrt(H). */
int qot_tconv_graph_supported(int n, int max_e, int H, int D);
int qot_tconv_graph_ldm(int n);
size_t qot_tconv_graph_row_floats(int n, int H, int D);
int qot_tconv_bwd_graph_blocks(int64_t B);
int qot_table_scores(const float* table, const float* wq, const float* bq, const float* wk, const float* bk,
                     const float* w_edge, float* M, float* P, int n, int H, int D, qot_stream_t stream);
int qot_tconv_fwd_graph(const float* t4, int ld, const float* M, const float* P, const float* w_edge,
                        const float* edge_attr, const int32_t* rowptr, const int32_t* colf, const int32_t* eid,
                        const int32_t* row, float* out, float* alpha, float* ea_csr, float* aa, int n, int64_t B, int max_e,
                        int H, int D, int act, float act_slope, float act_p, uint64_t act_seed, const int64_t* act_step,
                        qot_stream_t stream);
int qot_tconv_bwd_graph(const float* grad_out, const float* y_act, float act_slope, float act_p, uint64_t act_seed,
                        const int64_t* act_step, const float* t4, int ld, const float* w_edge, const float* ea_csr,
                        const float* alpha, const float* aa, const int32_t* rowptr, const int32_t* colf,
                        const int32_t* row, const int32_t* rowptr_t, const int32_t* col_t, const int32_t* pos_t,
                        float* partials, int n, int64_t B, int max_e, int H, int D, qot_stream_t stream);
int qot_table_project_bwd_scores(const float* S, const float* t4, const float* w_edge, const float* table,
                                 const float* wq, const float* wk, const float* wv, const float* ws, float* grad_table,
                                 float* grad_w, float* grad_b, float* grad_w_edge, int V, int n, int H, int D,
                                 qot_stream_t stream);

/* ---- NNConv (aggr = mean), factorised ----------------------------------------------
 * h_e = relu(W1 ea_e + b1) in R^K, K = 2D.  Builds the GEMM operand
 *   A[i] = [ invdeg_i * sum_e h_e[0] x_j | ... | invdeg_i * sum_e h_e[K-1] x_j |
 *            invdeg_i * sum_e x_j | x_i ]                       ([N, (K+2) H])
 * so that NNConv(x) = A @ Wcat + bias with Wcat = [W2 blocks; b2 block; W_root^T].
 * transpose != 0 runs the same aggregation over the CSC (out-edges) with the scale taken
 * at the gathered end (invdeg[col]) -- the adjoint used for grad_x.
 */
int qot_nnconv_agg(const float* x, int ld_x, const float* edge_attr, const float* w1,
                   const float* b1, const int32_t* rowptr, const int32_t* col,
                   const int32_t* eid_or_pos, const int32_t* eid_of_pos, const float* invdeg,
                   int transpose, float* A, int64_t N, int H, int D, qot_stream_t stream);
/* Fused form of qot_nnconv_agg + GEMM (+bias) for H == 64: the [32 x (K+2)H] operand tile is
 * built in LDS and multiplied on the matrix cores (v_mfma_f32_32x32x2_f32), A never touches
 * HBM.  w_perm = Wcat ([(K+2)H, H]) permuted into MFMA fragment order (layout documented in
 * csrc/nnconv_mfma.hip).  edge_ids[p] = original edge id of slot p of the index walked (eid for
 * the CSR, eid_t for the CSC).  transpose != 0: adjoint over the CSC with w_perm built from
 * Wcat^T blocks (grad_x).  bias may be NULL.  H == 64: the tuned tile kernel (csrc/nnconv_mfma.hip), w_perm =
 * Wcat in its fragment order.  H in {16, 32, 128, 256} (D <= 4): the per-pass tile kernel of csrc/nnconv_gen.hip,
 * w_perm in ITS layout (one pass per 64 input channels; documented there, built by
 * functional.nnconv_gen_perm_index); transpose = 2 / 3 selects that kernel for H == 64 too (measurements). */
int qot_nnconv_fused(const float* x, int ld_x, const float* edge_attr, const float* w1,
                     const float* b1, const int32_t* rowptr, const int32_t* col,
                     const int32_t* edge_ids, const float* invdeg, int transpose,
                     const float* w_perm, const float* bias, float* out, int64_t N, int H, int D,
                     int act, float act_slope, float act_p, uint64_t act_seed, const int64_t* act_step,
                     qot_stream_t stream);
/* H == 64, transpose = 0 only: as qot_nnconv_fused with the products on the bf16 matrix pipe, each fp32 product as six
 * bf16 cross products of three-way splits (csrc/split_bf16.hpp).  w_split: Wcat split into three bf16 planes
 * split_stride elements apart (functional.nnconv_split_index, the QOT_ROLE_GATHER3 split part), 16-byte aligned.
 * The operand tile is split once per tile on its way to LDS (bf16 planes, two K phases) unless
 * QOT_NNCONV_FWD_SPLIT_AFTER_READ=1 is set in the environment, read on every call: the earlier loop, which splits every
 * fragment after its read (another per-wave summation order: results differ in the last bits). */
int qot_nnconv_fused_split(const float* x, int ld_x, const float* edge_attr, const float* w1,
                           const float* b1, const int32_t* rowptr, const int32_t* col,
                           const int32_t* edge_ids, const float* invdeg, const void* w_split,
                           int64_t split_stride, const float* bias, float* out, int64_t N, int H, int D,
                           int act, float act_slope, float act_p, uint64_t act_seed, const int64_t* act_step,
                           qot_stream_t stream);
/* C[KT,64] = A[N,KT]^T @ G[N,64] (fp32 MFMA, operands streamed from HBM in fragment order,
 * deterministic slab reduction).  Weight-gradient GEMM of NNConv (gWcat = A^T g) -- the shape
 * library GEMMs run at 13-28 TFLOP/s.  KT multiple of 128, <= 1280.  workspace:
 * qot_gemm_tn_workspace_floats(KT) floats. */
size_t qot_gemm_tn_workspace_floats(int KT);
int qot_gemm_tn(const float* A, int lda, const float* G, int ldg, int64_t N, int KT, float* C,
                float* workspace, qot_stream_t stream);
/* NNConv backward, data and weight gradients from one gather (H == 64, D <= 4): grad_x = U @ WcatT
 * (as qot_nnconv_fused transpose=1) and gwcat_t = per-block transposes of d/dWcat
 * (gwcat_t[k*64+o][a] = dWcat[k*64+a][o]) computed as X^T U from the same LDS tile.  Replaces
 * {qot_nnconv_fused(transpose=1), qot_nnconv_agg, qot_gemm_tn}.  x = the forward input rows.
 * param_layout = 1 writes the weight gradient in the parameters' own layouts instead:
 * [d nn.2.weight [H*H, K] | d nn.2.bias [H*H] | d lin.weight [H, H]] (same total size).
 * param_layout = 2 (profiling only) launches the main kernel alone: per-workgroup slabs stay in the
 * workspace and gwcat_t is not written -- lets bench.py time exactly the kernel rocprofv3 lists.
 * The X^T U product is issued as split-bf16 MFMAs (csrc/split_bf16.hpp) unless QOT_NNCONV_F32_MFMA=1 is set in the
 * environment, read on every call; the grad_x product is an fp32 MFMA either way.
 * workspace: qot_nnconv_adjoint_dw_workspace_floats(D) floats. */
size_t qot_nnconv_adjoint_dw_workspace_floats(int D);
int qot_nnconv_adjoint_dw(const float* grad_out, int ld_g, const float* x, int ld_x,
                          const float* edge_attr, const float* w1, const float* b1,
                          const int32_t* rowptr_t, const int32_t* col_t, const int32_t* eid_t,
                          const float* invdeg, const float* w_perm, float* grad_x, float* gwcat_t, int param_layout,
                          float* workspace, int64_t N, int H, int D, qot_stream_t stream);
/* Fused form of {GA = g @ Wk^T ; qot_nnconv_bwd_edge}, D <= 4: the GA tile is produced by MFMA into LDS and
 * consumed there.  b_perm: Wk^T in fragment order (H == 64: csrc/nnconv_mfma.hip; H in {16, 32, 128, 256}:
 * 32 input channels per pass, layout in csrc/nnconv_gen.hip, built by functional.nnconv_gen_gradh_perm_index).
 * workspace: qot_nnconv_gradh_workspace_floats(D) floats.  gw1/gb1 are overwritten. */
size_t qot_nnconv_gradh_workspace_floats(int D);
int qot_nnconv_gradh_fused(const float* grad_out, int ld_g, const float* x, int ld_x,
                           const float* edge_attr, const float* w1, const float* b1,
                           const int32_t* rowptr, const int32_t* col, const int32_t* eid,
                           const float* invdeg, const float* b_perm, float* gw1, float* gb1,
                           float* workspace, int64_t N, int H, int D, qot_stream_t stream);
/* H == 64: as qot_nnconv_gradh_fused with the GA products on the bf16 matrix pipe (csrc/split_bf16.hpp).  b_split: Wk^T
 * split into three bf16 planes split_stride elements apart (functional.nnconv_split_index), 16-byte aligned. */
int qot_nnconv_gradh_split(const float* grad_out, int ld_g, const float* x, int ld_x,
                           const float* edge_attr, const float* w1, const float* b1,
                           const int32_t* rowptr, const int32_t* col, const int32_t* eid,
                           const float* invdeg, const void* b_split, int64_t split_stride, float* gw1, float* gb1,
                           float* workspace, int64_t N, int H, int D, qot_stream_t stream);
/* Weight gradient of NNConv for every supported width (H in {16, 32, 64, 128, 256}, D <= 4) without
 * materialising the [N, (K+2)H] operand: grad_params = [d nn.2.weight [H*H, K] | d nn.2.bias [H*H] |
 * d lin.weight [H, H]] (the parameters' own layouts, (2D+2)*H*H floats) = A^T grad_out, with the operand
 * tile A of 32 destinations gathered into LDS 16 input channels at a time (csrc/nnconv_gen.hip).  x = the
 * forward input rows; rowptr/col/eid = CSR by destination.  Replaces {qot_nnconv_agg, A^T g GEMM} of
 * NNConv's autograd (topological_training/models.py:57 under loss.backward(), train.py:115).
 * workspace: qot_nnconv_dw_workspace_floats(N, H, D) floats.  Fixed summation order. */
size_t qot_nnconv_dw_workspace_floats(int64_t N, int H, int D);
int qot_nnconv_dw(const float* x, int ld_x, const float* grad_out, int ld_g, const float* edge_attr,
                  const float* w1, const float* b1, const int32_t* rowptr, const int32_t* col,
                  const int32_t* eid, const float* invdeg, float* grad_params, float* workspace, int64_t N,
                  int H, int D, qot_stream_t stream);
/* H == 64: both second-stage sums of the NNConv backward in ONE launch.  Call qot_nnconv_adjoint_dw with
 * param_layout = 2 (slabs stay in its workspace) and qot_nnconv_gradh_fused with gw1 = gb1 = NULL (block partials stay in
 * its workspace), then this: grad_params as qot_nnconv_adjoint_dw(param_layout = 1), gw1[K,D], gb1[K].  Fixed order. */
int qot_nnconv_bwd_finalize(const float* adj_workspace, const float* gradh_workspace, float* grad_params,
                            float* gw1, float* gb1, int64_t N, int H, int D, qot_stream_t stream);
/* grad of the edge MLP's first layer: GA[N, K*H] = g @ Wcat[:K*H]^T (caller GEMM);
 * gw1[K,D], gb1[K] zero-filled by caller, accumulated with atomics. */
int qot_nnconv_bwd_edge(const float* GA, int ld_ga, const float* x, int ld_x,
                        const float* edge_attr, const float* w1, const float* b1,
                        const int32_t* rowptr, const int32_t* col, const int32_t* eid,
                        const float* invdeg, float* gw1, float* gb1, int64_t N, int H, int D,
                        qot_stream_t stream);

/* ---- gradients wrt the edge features (csrc/edge_grad.hip) --------------------------
 * edge_attr.grad of the two convolutions; the training step never asks for it.  Both kernels run in addition to the
 * parameter backward of whichever form the forward took, recompute what they need, and write grad_edge_attr [E,D] in the
 * caller's edge order (slot p -> row eid[p]) with plain stores: one owner per edge, bitwise reproducible, every row
 * written (no zero fill needed).  H in {16, 32, 64, 128, 256}, D in {1..8}.
 * TransformerConv: grad_out [N,H], y_act / act_* as qot_tconv_bwd_dst (the fused activation is undone when y_act != NULL);
 * qkvs = the packed [q|k|v|skip] rows (ld floats per row): node rows, or table rows through rowmap (node -> table row,
 * NULL in node mode) with col = the table row of each slot's source (colf in table mode, the CSR col in node mode).
 *     grad ea_e = ds_e u_i + alpha_e w_i,   u_i = W_e^T q_i / sqrt(H),   w_i = W_e^T g_i,   ds_e = alpha_e (da_e - delta_i)
 * NNConv (mean): GA [N, 2D*H] = g @ Wk^T (ld_ga, as qot_nnconv_bwd_edge), x = the forward input rows, CSR by destination.
 *     grad ea_e = W1^T ((W1 ea_e + b1 > 0) * invdeg_i GA_i x_j)                                                        */
int qot_tconv_edge_attr_grad(const float* grad_out, const float* y_act, float act_slope, float act_p, uint64_t act_seed,
                             const int64_t* act_step, const float* qkvs, int ld, const int32_t* rowmap, const int32_t* col,
                             const int32_t* rowptr, const int32_t* eid, const float* edge_attr, const float* w_edge,
                             float* grad_edge_attr, int64_t N, int H, int D, qot_stream_t stream);
int qot_nnconv_edge_attr_grad(const float* GA, int ld_ga, const float* x, int ld_x, const float* edge_attr,
                              const float* w1, const float* b1, const int32_t* rowptr, const int32_t* col,
                              const int32_t* eid, const float* invdeg, float* grad_edge_attr, int64_t N, int H, int D,
                              qot_stream_t stream);

/* ---- attention weights (csrc/attention.hip) ------------------------------------------
 * PyG's return_attention_weights=True readout, recomputed from the rows the forward built; one owner per output row and
 * plain stores: bitwise reproducible, every row written (no zero fill needed).
 * qot_tconv_attention (heads = 1, H in {16, 32, 64, 128, 256}, D in {1..8}): qkvs / ld / rowmap / col as
 * qot_tconv_edge_attr_grad (node rows, or table rows through rowmap); alpha [E] in the caller's edge order (slot p -> eid[p])
 *     alpha_e = exp(s_e - max_i) / (sum_i + 1e-16),   s_e = <q_i, k_j + W_e ea_e> / sqrt(H)
 * qot_gat_attention (heads = 4): a_src / a_dst [N, 4] logits, CSR with gat_self_loops; alpha [num_kept + N, 4], the order
 * of remove_self_loops + add_self_loops: slot p with eid[p] >= 0 -> row edge_pos[eid[p]] (its index among the input's
 * non-self-loop edges, num_kept of them; edge_pos may be NULL when num_kept = 0), the self loop of node i -> num_kept + i
 *     alpha_p = softmax over i's slots of leaky_relu(a_src[col[p]] + a_dst[i], neg_slope).  a_src, a_dst, alpha 16-byte
 * aligned. */
int qot_tconv_attention(const float* qkvs, int ld, const int32_t* rowmap, const int32_t* col, const int32_t* rowptr,
                        const int32_t* eid, const float* edge_attr, const float* w_edge, float* alpha, int64_t N, int H,
                        int D, qot_stream_t stream);
int qot_gat_attention(const float* a_src, const float* a_dst, const int32_t* rowptr, const int32_t* col,
                      const int32_t* eid, const int32_t* edge_pos, int64_t num_kept, float* alpha, int64_t N, int heads,
                      float neg_slope, qot_stream_t stream);

/* ---- activation: y = dropout(leaky_relu(x, slope), p) ------------------------------
 * Counter-based RNG: keep = hash(seed, *step_counter, element) >= p.  step_counter is a
 * DEVICE int64 the caller bumps once per train step (graph-replay safe).  p == 0 or
 * step_counter == NULL disables dropout.  bwd regenerates the mask from the same inputs.
 */
int qot_act_fwd(const float* x, float* y, int64_t n, float slope, float p, uint64_t seed,
                const int64_t* step_counter, qot_stream_t stream);
int qot_act_bwd(const float* grad_y, const float* y_or_x, float* grad_x, int64_t n, float slope,
                float p, uint64_t seed, const int64_t* step_counter, qot_stream_t stream);

/* ---- global mean pool -------------------------------------------------------------- */
int qot_pool_fwd(const float* x, const int32_t* ptr, float* out, int64_t B, int H,
                 qot_stream_t stream);
int qot_pool_bwd(const float* grad_out, const int32_t* ptr, const int32_t* batch, float* grad_x,
                 int64_t N, int64_t B, int H, qot_stream_t stream);

/* ---- GATConv (concat heads) ---------------------------------------------------------
 * z[N, heads*C], a_src/a_dst[N, heads]; graph = CSR built with gat_self_loops.
 * out[N, heads*C] (+bias fused); stats[N, heads, 2].  stats and escr are read and written as (float, float) pairs:
 * 8-byte aligned, as are all row matrices 16-byte (QOT_ERR_BADARG otherwise).
 * qot_gat_logits: a_src[n,h] = <z[n,h,:], att_src[h,:]>, a_dst likewise (App. B.3), one pass over z.
 * qot_gat_fwd, bn_partials != NULL: also writes per-workgroup column (mean, sum of squared deviations) of out - bias,
 *   [qot_gat_blocks(N, heads, C)][2][heads*C] floats (buffer of qot_gat_bn_partials_floats), which
 *   qot_bn_stats_from_partials(shift = bias, ...) turns into the batch statistics of the BatchNorm that follows
 *   (lightpath_training/models.py:30-31) without another pass over out. */
int qot_gat_blocks(int64_t N, int heads, int C);
size_t qot_gat_bn_partials_floats(int64_t N, int heads, int C);
int qot_gat_logits(const float* z, const float* att_src, const float* att_dst, float* a_src, float* a_dst,
                   int64_t N, int heads, int C, qot_stream_t stream);
int qot_gat_fwd(const float* z, const float* a_src, const float* a_dst, const float* bias,
                const int32_t* rowptr, const int32_t* col, float* out, float* stats, int64_t N,
                int heads, int C, float neg_slope, float* bn_partials, qot_stream_t stream);
/* Thin forms (r04): the layer's projection z = x W^T (x [N, K], K <= 8 input features -- LightpathGNN's first layer, K = 5;
 * W [heads*C, K] = GATConv.lin.weight) is formed inside the attention kernels, so that z is never written or read.  Same
 * outputs and partials layout as qot_gat_fwd / qot_gat_bwd_dst; a_src / a_dst are the caller's (x (W_h^T att_h): two
 * qot_skinny_linear_fwd of width 4).  qot_gat_thin_supported: 1 when K is in 1..8 and W^T fits next to the walk's LDS image;
 * the entry points return QOT_ERR_UNSUPPORTED otherwise. */
int qot_gat_thin_supported(int heads, int C, int K);
int qot_gat_fwd_thin(const float* x, int K, const float* w, const float* a_src, const float* a_dst, const float* bias,
                     const int32_t* rowptr, const int32_t* col, float* out, float* stats, int64_t N, int heads, int C,
                     float neg_slope, float* bn_partials, qot_stream_t stream);
int qot_gat_bwd_dst_thin(const float* grad_out, const float* x, int K, const float* w, const float* a_src,
                         const float* a_dst, const float* stats, const int32_t* rowptr, const int32_t* col,
                         float* grad_a_dst, float* escr, float* delta, int64_t N, int heads, int C, float neg_slope,
                         float* grad_bias, float* workspace, qot_stream_t stream);
/* destination pass: grad_a_dst[N,heads], escr[cap, heads, 2] = (alpha, dalpha), delta[N,heads].
 * grad_bias != NULL: also GATConv's bias gradient [heads*C] = column sums of grad_out (every row passes through this
 * kernel once anyway); workspace: qot_gat_bn_partials_floats(N, heads, C) floats. */
int qot_gat_bwd_dst(const float* grad_out, const float* z, const float* a_src, const float* a_dst,
                    const float* stats, const int32_t* rowptr, const int32_t* col, float* grad_a_dst,
                    float* escr, float* delta, int64_t N, int heads, int C, float neg_slope,
                    float* grad_bias, float* workspace, qot_stream_t stream);
/* source pass: grad_z[N, heads*C], grad_a_src[N, heads].  att_src != NULL (logits formed by qot_gat_logits):
 * grad_z also receives grad_a_src[j,h] att_src[h,:] + grad_a_dst[j,h] att_dst[h,:]. */
int qot_gat_bwd_src(const float* grad_out, const float* a_src, const float* a_dst, const float* escr,
                    const float* delta, const int32_t* rowptr_t, const int32_t* col_t,
                    const int32_t* pos_t, float* grad_z, float* grad_a_src, int64_t N, int heads,
                    int C, float neg_slope, const float* att_src, const float* att_dst,
                    const float* grad_a_dst, qot_stream_t stream);
/* grad_att_src[h*C + c] = sum_n grad_a_src[n,h] z[n,h,c] (grad_att_dst with grad_a_dst); fixed summation order.
 * workspace: qot_gat_bn_partials_floats(N, heads, C) floats. */
int qot_gat_att_grad(const float* z, const float* grad_a_src, const float* grad_a_dst, float* grad_att_src,
                     float* grad_att_dst, float* workspace, int64_t N, int heads, int C, qot_stream_t stream);

/* ---- BatchNorm1d (+ fused ReLU) over the node matrix [N, C] -------------------------
 * qot_bn_stats: mean[C], rstd[C] (biased var, eps), and when running_* != NULL the
 * momentum update with the unbiased variance.  partials: workspace of
 * qot_bn_partials_floats(N, C) floats. */
size_t qot_bn_partials_floats(int64_t N, int C);
int qot_bn_stats(const float* x, int64_t N, int C, float eps, float momentum, float* mean,
                 float* rstd, float* running_mean, float* running_var, float* partials,
                 qot_stream_t stream);
/* y = relu?((x - mean) * rstd * w + b) */
/* batch statistics from per-workgroup column (mean, M2 = sum of squared deviations) pairs [nblk][2][C] of x - shift
 * written by the producer of x (qot_gat_fwd: workgroup b holds rows [b * chunk_rows, min((b + 1) * chunk_rows, N)),
 * chunk_rows = qot_gat_chunk_rows(N, heads, C)), merged with Chan's formula in fp64: same results as qot_bn_stats
 * without reading x again, and no E[d^2] - E[d]^2 cancellation for channels whose mean is far from the shift. */
int64_t qot_gat_chunk_rows(int64_t N, int heads, int C);
int qot_bn_stats_from_partials(const float* shift, const float* partials, int nblk, int64_t chunk_rows, int64_t N, int C,
                               float eps, float momentum, float* mean, float* rstd, float* running_mean,
                               float* running_var, qot_stream_t stream);
int qot_bn_apply(const float* x, const float* mean, const float* rstd, const float* w,
                 const float* b, float* y, int64_t N, int C, int relu, qot_stream_t stream);
/* train-mode backward: needs column sums first (qot_bn_bwd_reduce -> gw[C], gb[C]), then
 * qot_bn_bwd_apply.  eval mode (batch_stats == 0) skips the mean-subtraction terms.
 * relu != 0 with y == NULL: the ReLU mask is recomputed from x, mean, rstd, w (weight), b (bias) with the forward's
 * expression instead of being read from the saved output -- one [N, C] read fewer in each kernel. */
int qot_bn_bwd_reduce(const float* grad_y, const float* y, const float* x, const float* mean,
                      const float* rstd, float* gw, float* gb, int64_t N, int C, int relu,
                      float* partials, const float* w, const float* b, qot_stream_t stream);
int qot_bn_bwd_apply(const float* grad_y, const float* y, const float* x, const float* mean,
                     const float* rstd, const float* w, const float* gw, const float* gb,
                     float* grad_x, int64_t N, int C, int relu, int batch_stats, const float* b,
                     qot_stream_t stream);
/* BatchNorm(+ReLU) of which only some rows are consumed: y_rows = act(BatchNorm(x))[idx] -- LightpathGNN normalises the
 * whole node matrix and then keeps the LUT nodes' rows (lightpath_training/models.py:31-32, 35-40).  Statistics over all
 * N rows as before (qot_bn_stats / qot_bn_stats_from_partials); idx: n unique row numbers.
 * qot_bn_apply_rows: the n output rows only.  qot_bn_bwd_reduce_rows: the column sums over the n rows that carry a
 * gradient (partials: qot_bn_partials_floats(n, C) floats).  qot_bn_bwd_apply_rows: grad_x [N, C] (batch-statistics
 * form), bit for bit what qot_bn_bwd_apply gives for the zero-filled [N, C] gradient with grad_rows scattered into it. */
int qot_bn_apply_rows(const float* x, const int32_t* idx, int64_t n, const float* mean, const float* rstd, const float* w,
                      const float* b, float* y_rows, int C, int relu, qot_stream_t stream);
int qot_bn_bwd_reduce_rows(const float* grad_rows, const int32_t* idx, int64_t n, const float* x, const float* mean,
                           const float* rstd, float* gw, float* gb, int C, int relu, float* partials, const float* w,
                           const float* b, qot_stream_t stream);
int qot_bn_bwd_apply_rows(const float* grad_rows, const int32_t* idx, int64_t n, const float* x, const float* mean,
                          const float* rstd, const float* w, const float* gw, const float* gb, float* grad_x, int64_t N,
                          int C, int relu, const float* b, qot_stream_t stream);

/* ---- train-step envelope helpers (topological_training/train.py:109-116) ----------------
 * qot_sgd_momentum: torch.optim.SGD(lr, momentum) update over one flat buffer; first_step != 0
 * initialises the momentum buffer with the gradient (torch semantics).
 * qot_small_gemm: C[M,N] = op(A) op(B) (+bias) with element strides (head MLP, table projection:
 * topological_training/models.py:33-38,63; a few MFLOP each).  split_k > 1: C holds split_k partial
 * planes [M, ldc] (K chunks of ceil(K/split_k) rounded to 32), summed by the caller in a fixed order.
 * qot_colsum: out[C] = column sums of x[N, C] (bias gradients), deterministic two-stage.
 * qot_act_bwd_colsum: grad_x = qot_act_bwd(grad_y, y) AND colsum(grad_x) in the same pass (bias
 * gradient of a conv whose epilogue carried leaky_relu+dropout, models.py:54-58).
 * Both take qot_colsum_workspace_floats(C) floats of workspace. */
int qot_sgd_momentum(float* param, const float* grad, float* momentum_buf, int64_t n, float lr,
                     float momentum, int first_step, qot_stream_t stream);
/* The same update with the gradient pack folded in: parameter i's gradient is read from grads[i]
 * (device pointer, NULL = zero gradient; `grads` and `offsets` are HOST arrays of `count` pointers and
 * count+1 element offsets into the flat buffers, offsets[0] = 0, offsets[count] = n, count <= 48), the
 * packed value is also stored to grad_flat (may be NULL).  lr_dev != NULL: learning rate read from device
 * memory (as qot_sgd_momentum_dev), else `lr`.  Replaces FlatModel.gather_grads' concatenation launch. */
int qot_sgd_momentum_multi(float* param, const float* const* grads, const int64_t* offsets, int count,
                           float* grad_flat, float* momentum_buf, int64_t n, float lr, const float* lr_dev,
                           float momentum, int first_step, qot_stream_t stream);
/* same update with the learning rate read from device memory at run time, so that a step captured in a
 * HIP graph follows the scheduler (StepLR, topological_training/train.py:67,181) without re-capture */
int qot_sgd_momentum_dev(float* param, const float* grad, float* momentum_buf, int64_t n, const float* lr_dev,
                         float momentum, int first_step, qot_stream_t stream);
int qot_small_gemm(const float* A, int64_t stride_am, int64_t stride_ak, const float* B, int64_t stride_bk,
                   int64_t stride_bn, const float* bias, float* C, int ldc, int M, int N, int K,
                   int split_k, qot_stream_t stream);
size_t qot_colsum_workspace_floats(int C);
/* out[C] = sum over the B rows of x[B, C] for wide rows (sum over graphs of a per-node gradient,
 * TransformerConv table mode); workspace: qot_rowsum_wide_workspace_floats(C) floats. */
size_t qot_rowsum_wide_workspace_floats(int64_t C);
int qot_rowsum_wide(const float* x, int64_t B, int64_t C, float* out, float* workspace, qot_stream_t stream);
int qot_colsum(const float* x, int ld, int64_t N, int C, float* out, float* workspace, qot_stream_t stream);
int qot_act_bwd_colsum(const float* grad_y, const float* y, float* grad_x, int64_t N, int C, float slope, float p,
                       uint64_t seed, const int64_t* step_counter, float* colsum_out, float* workspace,
                       qot_stream_t stream);

/* ---- fused read-out head: global_mean_pool -> Linear(H,H) -> LeakyReLU -> Dropout -> Linear(H,O)
 * (topological_training/models.py:33-38,61-63).  fwd saves pooled[B,H] and hidden[B,H] (post dropout).
 * bwd: grad_x[N,H] (pool backward included) and grads = [gW0 | gb0 | gW3 | gb3] contiguous
 * (deterministic partial sums; workspace qot_head_bwd_workspace_floats(H, O) floats).  O <= 8.
 * x_in != NULL (the head's input, i.e. the last conv's output y = dropout(leaky_relu(conv)) with the
 * in_* activation parameters of that conv's epilogue, models.py:58-59): grad_x is then the gradient
 * wrt the CONV output (the activation backward is applied while the pool gradient is written) and
 * grads gets H more floats: its column sums = that conv's bias gradient.
 * grads == NULL: the per-workgroup partials [qot_head_bwd_blocks(B), H*H + H + O*H + O (+ H with x_in)] are left in
 * the workspace for the caller to sum (QOT_ROLE_SUM_ROWS of the step's backward epilogue). */
int qot_head_fwd(const float* x, const int32_t* ptr, const float* w0, const float* b0, const float* w3,
                 const float* b3, float* pooled, float* hidden, float* out, int64_t B, int H, int O,
                 float slope, float p, uint64_t seed, const int64_t* step_counter, qot_stream_t stream);
/* As qot_head_fwd, with the criterion of the train step folded in (topological_training/train.py:69,113-115:
 * SmoothL1Loss(reduction="mean", beta) on out vs target[B,O]): also writes grad_out[B,O] = d loss / d out and
 * loss_rows[B] = each graph's share of the mean loss; the loss value is the sum of loss_rows (the caller sums it
 * where it sums its other partials: QOT_ROLE_SUM_ROWS).  Replaces the separate qot_smooth_l1 launch of a step. */
int qot_head_fwd_loss(const float* x, const int32_t* ptr, const float* w0, const float* b0, const float* w3,
                      const float* b3, float* pooled, float* hidden, float* out, int64_t B, int H, int O,
                      float slope, float p, uint64_t seed, const int64_t* step_counter, const float* target,
                      float beta, float* grad_out, float* loss_rows, qot_stream_t stream);
/* The read-out of a TRAIN step in one kernel: forward + SmoothL1(mean, beta) + backward per graph (a graph's rows are read
 * once and stay in LDS for the pool backward; pooled / hidden never leave the workgroup).  grad_x[N,H] is the gradient wrt
 * the CONV output when fold != 0 (x = dropout(leaky_relu(conv)) with the in_* parameters, as qot_head_bwd(x_in)).
 * workspace: per-workgroup parameter-gradient partials [qot_head_train_blocks(B, H)][H*H + H + O*H + O (+ H when fold)] for
 * the caller to sum (QOT_ROLE_SUM_ROWS); the loss value is the sum of loss_rows[B].  Replaces {qot_head_fwd_loss, qot_head_bwd}
 * of a step (topological_training/train.py:111-115).  H <= 64 (r04): 256 / H graphs per pass of a workgroup, a graph's rows
 * kept in registers from the pool to the pool backward (csrc/head.hip: head_train_batched_kernel). */
int qot_head_train_blocks(int64_t B, int H);
int qot_head_train(const float* x, const int32_t* ptr, const float* w0, const float* b0, const float* w3, const float* b3,
                   const float* target, float beta, float* out, float* grad_out, float* loss_rows, float* grad_x,
                   float* workspace, int64_t B, int H, int O, float slope, float p, uint64_t seed,
                   const int64_t* step_counter, int fold, float in_slope, float in_p, uint64_t in_seed,
                   const int64_t* in_step, qot_stream_t stream);
size_t qot_head_bwd_workspace_floats(int H, int O);
int qot_head_bwd_blocks(int64_t B);
int qot_head_bwd(const float* grad_out, const float* pooled, const float* hidden, const int32_t* ptr,
                 const float* w0, const float* w3, float* grad_x, float* grads, float* workspace, int64_t B,
                 int H, int O, float slope, float p, uint64_t seed, const int64_t* step_counter,
                 const float* x_in, float in_slope, float in_p, uint64_t in_seed, const int64_t* in_step,
                 qot_stream_t stream);

/* ---- SmoothL1Loss(reduction="mean", beta) value and gradient in one launch
 * (criterion at topological_training/train.py:69, used at :113-115).  grad = d loss / d pred.
 * workspace: qot_smooth_l1_workspace_floats() floats whose first word is 0 before the first call
 * (the kernel leaves it 0). */
size_t qot_smooth_l1_workspace_floats(void);
int qot_smooth_l1(const float* pred, const float* target, int64_t n, float beta, float* loss, float* grad,
                  float* workspace, qot_stream_t stream);

/* ---- embedding-table projection for TransformerConv table mode: out[V,4H] = [q|k|v|skip] rows of
 * table[V,H] under lin_query/lin_key/lin_value/lin_skip (topological_training/models.py:51-53 with
 * x = node_embeddings(node_ids)); reads the four Linear parameters in place.
 * step_counter != NULL: the launch also performs qot_step_advance(step_counter, step_snapshot) -- in table
 * mode it is the forward's first kernel, and the dropout counter's own launch was ~5 us of a 0.6 ms step.
 * bwd: grad_table[V,H], grad_w[4H,H] and grad_b[4H] in q|k|v|skip order. */
int qot_table_project_fwd(const float* table, const float* wq, const float* bq, const float* wk, const float* bk,
                          const float* wv, const float* bv, const float* ws, const float* bs, float* out, int V,
                          int H, int64_t* step_counter, int64_t* step_snapshot, qot_stream_t stream);
int qot_table_project_bwd(const float* grad_out, const float* table, const float* wq, const float* wk,
                          const float* wv, const float* ws, float* grad_table, float* grad_w, float* grad_b, int V,
                          int H, qot_stream_t stream);

/* ---- TransformerConv table mode index maps in one launch (x = node_embeddings(node_ids),
 * topological_training/models.py:51): ids32[N] = node_ids, colf[E] = node_ids[col],
 * colf_t[E] = node_ids[col_t]. */
int qot_table_maps(const int64_t* node_ids, const int32_t* col, const int32_t* col_t, int32_t* ids32,
                   int32_t* colf, int32_t* colf_t, int64_t N, int64_t E, qot_stream_t stream);
/* ---- dropout draw counter: *counter += 1 and *snapshot = *counter, on the stream (replay-safe). */
int qot_step_advance(int64_t* counter, int64_t* snapshot, qot_stream_t stream);

/* ---- streamed replay: stage graphs [lo, lo + B) of an HBM-resident shard into the static buffers of a batch slot, `lo`
 * taken from DEVICE memory, so that one captured launch stages a different slice on every replay (csrc/stage.hip;
 * loader.StageSlot).  No counterpart in the reference: its DataLoader collates on the host (train.py:93-95,107).
 * ctl[4 + sched_cap] (int64, device): [0] position, [1] number of valid schedule entries, [2] snapshot (written by the
 * call: the `lo` it staged, or -1), [3] reserved (qot_shard_stage_padded: the slice's edge total), [4 ...] the schedule of `lo` values.  Each call takes
 * schedule[position] and advances the position on the device.
 * Shard: node_ptr / edge_ptr [G + 1] and graph_of_node [N_total] (int64, device), edge_index [2, E_total] (int64, numbered
 * within the shard), and optionally (NULL: absent) edge_attr [E_total, D], node_ids [N_total] (int64), x [N_total, F],
 * y [G, Y]; D, F, Y count 4-byte words per row.  Slot: buffers for exactly B graphs, N nodes, E edges; what is written is
 * what PackedGraphs.device_batch(lo, lo + B) hands out (edge_index, ptr, edge_ptr re-based, batch = graph id per node).
 * Validated on the device before anything is written: the position lies inside the schedule, 0 <= lo <= G - B and the
 * slice inside the arrays (else QOT_STAGE_BAD_RANGE); the slice holds exactly N nodes and E edges and no graph more than
 * max_nodes / max_edges (else QOT_STAGE_BAD_SHAPE).  On either, NOTHING is staged.  V > 0: a node id outside [0, V) is
 * staged as 0 and reported as QOT_STAGE_BAD_NODE_ID.  The bits are ORed into status (device int32, caller-zeroed). */
#define QOT_STAGE_BAD_SHAPE 1
#define QOT_STAGE_BAD_RANGE 2
#define QOT_STAGE_BAD_NODE_ID 4
int qot_shard_stage(int64_t* ctl, int64_t sched_cap, int32_t* status, const int64_t* node_ptr, const int64_t* edge_ptr,
                    const int64_t* graph_of_node, int64_t G, int64_t N_total, int64_t E_total, const int64_t* edge_index,
                    const void* edge_attr, int D, const int64_t* node_ids, const void* x, int F, const void* y, int Y,
                    int64_t B, int64_t N, int64_t E, int64_t max_nodes, int64_t max_edges, int64_t V,
                    int64_t* dst_edge_index, void* dst_edge_attr, int64_t* dst_node_ids, void* dst_x, void* dst_y,
                    int64_t* dst_ptr, int64_t* dst_edge_ptr, int64_t* dst_batch, qot_stream_t stream);
/* qot_shard_stage for batches of UNEQUAL edge totals through one slot (loader.PaddedStageSlot): every graph of the shard
 * has n nodes and at most max_edges edges; the slot holds B + P graphs, (B + P) * n nodes and E_cap edges, dst_y B rows.
 * A slice of B graphs with E_real edges is accepted when it holds B * n nodes and 0 <= E_cap - E_real <= P * max_edges
 * (else QOT_STAGE_BAD_SHAPE, nothing staged); ctl[2] receives `lo`, ctl[3] E_real.  The first B graphs / B * n nodes /
 * E_real edges of the slot are what qot_shard_stage writes.  Behind them P pad graphs take the spare edges: pad graph p
 * gets m_p = min(max_edges, spare left) edges, edge k of it runs (k mod n) -> ((k + 1) mod n) inside its own node range
 * (a ring: in-degree <= ceil(max_edges / n)), with zero edge_attr rows; its nodes carry node_ids 0 .. n-1 and zero x rows;
 * batch / ptr / edge_ptr continue to B + P graphs.  n >= 2 when P > 0 (a ring over one node would be a self loop). */
int qot_shard_stage_padded(int64_t* ctl, int64_t sched_cap, int32_t* status, const int64_t* node_ptr,
                           const int64_t* edge_ptr, const int64_t* graph_of_node, int64_t G, int64_t N_total,
                           int64_t E_total, const int64_t* edge_index, const void* edge_attr, int D,
                           const int64_t* node_ids, const void* x, int F, const void* y, int Y, int64_t B, int64_t n,
                           int64_t E_cap, int64_t P, int64_t max_edges, int64_t V, int64_t* dst_edge_index,
                           void* dst_edge_attr, int64_t* dst_node_ids, void* dst_x, void* dst_y, int64_t* dst_ptr,
                           int64_t* dst_edge_ptr, int64_t* dst_batch, qot_stream_t stream);
/* qot_shard_stage_padded for batches given as a LIST of single graphs (shuffled batches; loader.GatherStageSlot).  The
 * slot is the padded slot.  ctl[4 + sched_cap * B]: [0] position, [1] number of valid BATCHES in the schedule, [2] snapshot
 * (the number of the batch the call staged, or -1), [3] its edge total E_real, then B graph ids per batch; a call takes ids
 * [position * B, (position + 1) * B) and advances the position.  offs[B] (int64, device): scratch owned by the slot, the
 * exclusive prefix sum of the batch's edge counts.  Validated on the device before anything is written: the position lies
 * inside the schedule and every id in [0, G) with its slices inside the arrays (else QOT_STAGE_BAD_RANGE); every graph
 * holds n nodes and at most max_edges edges and 0 <= E_cap - E_real <= P * max_edges (else QOT_STAGE_BAD_SHAPE).  On
 * either, nothing is staged.  Graph i of the batch lands where collating the listed graphs puts it: nodes i n .., edge
 * columns offs[i] .., edge_index re-based to batch numbering, batch = i, ptr[i] = i n, edge_ptr[i] = offs[i]; an id may
 * repeat.  Node ids and the pad graphs as in qot_shard_stage_padded. */
int qot_shard_stage_gather(int64_t* ctl, int64_t sched_cap, int32_t* status, int64_t* offs, const int64_t* node_ptr,
                           const int64_t* edge_ptr, int64_t G, int64_t N_total, int64_t E_total, const int64_t* edge_index,
                           const void* edge_attr, int D, const int64_t* node_ids, const void* x, int F, const void* y, int Y,
                           int64_t B, int64_t n, int64_t E_cap, int64_t P, int64_t max_edges, int64_t V,
                           int64_t* dst_edge_index, void* dst_edge_attr, int64_t* dst_node_ids, void* dst_x, void* dst_y,
                           int64_t* dst_ptr, int64_t* dst_edge_ptr, int64_t* dst_batch, qot_stream_t stream);

/* ---- out[i] = concat(s0[0:n0], s1[0:n1], s2)[idx[i]]: one gather builds the fragment-ordered NNConv
 * operands from nn.2.weight / nn.2.bias / lin.weight (topological_training/models.py:20-25). */
int qot_gather3(const float* s0, int64_t n0, const float* s1, int64_t n1, const float* s2, const int32_t* idx,
                float* out, int64_t n, qot_stream_t stream);

/* ---- dense fp32 projections on the matrix cores (csrc/gemm.hip): GATConv's shared projection z = x W^T and its
 * autograd (lightpath_training/models.py:13,30; train.py:128), the LUT head's first layer (models.py:17-22).
 * qot_gemm_nt: C[M, N] = A'[M, K] . B[N, K]^T (+ bias[N]); scale != NULL: A' = relu(A * scale[k] + shift[k]) applied
 * while the operand is loaded (BatchNorm + ReLU of the previous layer, models.py:31-32, never materialised).
 * K multiple of 32; N, lda, ldb, ldc multiples of 4; operands 16-byte aligned.
 * qot_gemm_tn_planes: Cpart[splits, M, N], plane z = A[Kz, M]^T . B'[Kz, N] over its chunk of K (the weight gradient
 * g^T y, K = number of nodes; B' = relu(B * scale[n] + shift[n]) when scale != NULL); the caller sums the planes in
 * order (QOT_ROLE_SUM_ROWS: bitwise reproducible).  M, N multiples of 4; splits = qot_gemm_tn_splits(M, N, K). */
int qot_gemm_nt(const float* A, int64_t lda, const float* B, int64_t ldb, float* C, int64_t ldc, int64_t M, int N, int K,
                const float* scale, const float* shift, const float* bias, qot_stream_t stream);
/* qot_gemm_nt_logits: qot_gemm_nt for GATConv with 128 channels per head (N = heads * 128: one 128-column output tile per
 * head), which also leaves the attention logits a_src[m, h] = <C[m, h, :], att_src[h, :]>, a_dst likewise ([M, heads];
 * PyG GATConv's alpha_src / alpha_dst, lightpath_training/models.py:13) -- formed in the epilogue instead of by another
 * pass over the [M, 4C] matrix (qot_gat_logits).  att_src / att_dst: [N] floats, 16-byte aligned. */
int qot_gemm_nt_logits(const float* A, int64_t lda, const float* B, int64_t ldb, float* C, int64_t ldc, int64_t M, int N, int K,
                       const float* scale, const float* shift, const float* bias, const float* att_src,
                       const float* att_dst, float* a_src, float* a_dst, qot_stream_t stream);
/* qot_gemm_nt for few output tiles and a long inner dimension: Cpart[kslices][M, N], plane s = the product over the s-th
 * slice of K (K / kslices a multiple of 32); the caller sums the planes in order (QOT_ROLE_SUM_ROWS). */
int qot_gemm_nt_planes(const float* A, int64_t lda, const float* B, int64_t ldb, float* Cpart, int64_t M, int N, int K,
                       int kslices, qot_stream_t stream);
int qot_gemm_tn_splits(int M, int N, int64_t K);
/* 1 when qot_gemm_nt / qot_gemm_nt_logits run a product of this size on the 256 x 256 x 32 tiles of csrc/gemm256.hip (one
 * persistent workgroup per CU; at least one tile per CU and N >= 256), 0 for the 128 x 128 tiles of csrc/gemm.hip.  Same
 * results either way up to the order of the K sum inside a tile; for tests and tools. */
int qot_gemm256_takes(int64_t M, int N);
int qot_gemm_tn_planes(const float* A, int64_t lda, const float* B, int64_t ldb, float* Cpart, int M, int N, int64_t K,
                       int splits, const float* scale, const float* shift, qot_stream_t stream);

/* ---- first-layer projection with a handful of input features (lightpath_training/models.py:13: GATConv(in_channels = 5,
 * ...).lin): out[N, C] = x[N, F] . w[C, F]^T, F <= 8, C multiple of 4 (<= 1024) -- pure bandwidth; and its weight gradient
 * g^T x as per-workgroup partials [qot_skinny_linear_dw_blocks(N)][C * F] the caller sums in order (QOT_ROLE_SUM_ROWS). */
int qot_skinny_linear_fwd(const float* x, const float* w, float* out, int64_t N, int F, int C, qot_stream_t stream);
/* ... with the attention logits of qot_gemm_nt_logits (C = heads * 128, C in {128, 256, 512, 1024}) */
int qot_skinny_linear_fwd_logits(const float* x, const float* w, float* out, int64_t N, int F, int C, const float* att_src,
                                 const float* att_dst, float* a_src, float* a_dst, qot_stream_t stream);
int qot_skinny_linear_dw_blocks(int64_t N);
int qot_skinny_linear_dw(const float* g, const float* x, float* partials, int64_t N, int F, int C, qot_stream_t stream);

/* ---- multi-role launch: several INDEPENDENT small jobs of one train step in ONE kernel launch -------------------
 * The reference's step (topological_training/train.py:109-116) reaches ~60 small torch / PyG kernels around the two
 * convolutions; on this engine the convolutions are a handful of launches and what is left are 4-9 us jobs whose
 * cost is the launch itself.  Jobs that do not depend on each other share a launch: role r gets a contiguous
 * range of 256-thread workgroups and runs the body of the standalone entry point of its kind (those entry points
 * are one-role calls of this function).  The table is copied into the kernel arguments: nothing is read from the
 * caller's array after the call returns, nothing is allocated, no synchronisation.
 * Jobs of one call MUST be independent: none may read what another one writes.
 *
 * kind                        p[] (device pointers)                                       i[] (host integers)
 * QOT_ROLE_CSR_BY_GRAPH       0 edge_index, 1 node_ptr, 2 edge_ptr, 3 rowptr, 4 col, 5 eid, 6 row, 7 rowptr_t,
 *                             8 col_t, 9 pos_t, 10 eid_t, 11 invdeg, 12 status, 13 node_ids, 14 ids32, 15 colf,
 *                             16 colf_t, 17 ptr32                                          0 E, 1 N, 2 B (> 0),
 *                             (as qot_csr_build_by_graph)                                  3 max_nodes, 4 max_edges
 * QOT_ROLE_TABLE_PROJECT_FWD  0 table, 1 wq, 2 bq, 3 wk, 4 bk, 5 wv, 6 bv, 7 ws, 8 bs, 9 out,
 *                             10 step_counter, 11 step_snapshot (as qot_table_project_fwd)  0 V (> 0), 1 H
 * QOT_ROLE_GATHER3            0 s0, 1 s1, 2 s2, 3 idx, 4 out (as qot_gather3)               0 n0, 1 n1, 2 n,
 *                             optional: 5 idx2 [m], 6 out2 (uint16 [3, m]): the gather       3 m (0: none)
 *                             through idx2 split into bf16 planes hi / mid / lo (the split
 *                             NNConv operands)
 * QOT_ROLE_SUM_ROWS           0 partials [nblk, n], 1 out [groups, n]:                     0 nblk, 1 n, 2 rows per
 *                             out[g, t] = sum of partials[b, t] over the rows b of group g,   group (0 = all rows:
 *                             fixed order (bitwise reproducible)                            one output row);
 *                                                                                           3, 4 derived
 * QOT_ROLE_NNCONV_FINALIZE64  0 adj_workspace, 1 gradh_workspace, 2 grad_params, 3 gw1,    0 N, 1 D; 2..7 derived
 *                             4 gb1 (as qot_nnconv_bwd_finalize, H = 64)
 * QOT_ROLE_TABLE_PROJECT_BWD  0 grad_out, 1 table, 2 wq, 3 wk, 4 wv, 5 ws, 6 grad_table,   0 V, 1 H
 *                             7 grad_w, 8 grad_b (as qot_table_project_bwd)
 * QOT_ROLE_TABLE_SCORES       0 table, 1 wq, 2 bq, 3 wk, 4 bk, 5 w_edge, 6 M, 7 P          0 n, 1 H, 2 D
 *                             (as qot_table_scores)
 * QOT_ROLE_TABLE_PROJECT_BWD_SCORES  0 S, 1 t4, 2 w_edge, 3 table, 4 wq, 5 wk, 6 wv, 7 ws,  0 V, 1 n, 2 H, 3 D
 *                             8 grad_table, 9 grad_w, 10 grad_b, 11 grad_w_edge (as qot_table_project_bwd_scores)
 * QOT_ROLE_NNCONV_SLAB_SUM64   the slab half of QOT_ROLE_NNCONV_FINALIZE64 alone: 0 adj_workspace, 2 grad_params (same
 *                             slots; 1, 3, 4 unused); it depends on qot_nnconv_adjoint_dw only       0 N, 1 D; 2..7 derived
 * QOT_ROLE_NNCONV_GRADH_SUM64  the grad-h half alone: 1 gradh_workspace, 3 gw1, 4 gb1 (0, 2 unused)   0 N, 1 D; 2..7 derived
 * "derived" fields are filled by the library in its own copy; callers leave them 0. */
#define QOT_MAX_ROLES 12
enum {
    QOT_ROLE_CSR_BY_GRAPH = 1,
    QOT_ROLE_TABLE_PROJECT_FWD = 2,
    QOT_ROLE_GATHER3 = 3,
    QOT_ROLE_SUM_ROWS = 4,
    QOT_ROLE_NNCONV_FINALIZE64 = 5,
    QOT_ROLE_TABLE_PROJECT_BWD = 6,
    QOT_ROLE_TABLE_SCORES = 7,
    QOT_ROLE_TABLE_PROJECT_BWD_SCORES = 8,
    QOT_ROLE_NNCONV_SLAB_SUM64 = 9,
    QOT_ROLE_NNCONV_GRADH_SUM64 = 10
};
typedef struct qot_role {
    int32_t kind;
    int32_t reserved;
    const void* p[18];
    int64_t i[8];
} qot_role_t;
int qot_run_roles(const qot_role_t* roles, int n_roles, qot_stream_t stream);

/* Sums hosted by the next grad-h launch.  The persistent tile walk of the H = 64 grad-h kernel ends in a ragged round (at
 * 12.5 tiles per CU three quarters of its workgroup slots idle for the last tile time); workgroups appended to that launch
 * start in the freed slots.  This call hands the NEXT qot_nnconv_gradh_split / qot_nnconv_gradh_fused call of the calling
 * thread up to QOT_MAX_ROLES jobs to run there.
 *   - Kinds: QOT_ROLE_SUM_ROWS and QOT_ROLE_NNCONV_SLAB_SUM64 (streaming sums, at most 4 KB of scratch); any other known
 *     kind: QOT_ERR_UNSUPPORTED.  Each role is validated as qot_run_roles validates it; on any error NOTHING is stored
 *     (what an earlier call left stays).  n_roles = 0 withdraws what an earlier call left.
 *   - A hosted job may read only what launches enqueued BEFORE the grad-h call wrote; it must not read what the grad-h call
 *     writes (a QOT_ROLE_SUM_ROWS whose partials lie in the grad-h call's workspace makes that call return QOT_ERR_BADARG
 *     before it launches anything), and hosted jobs are independent of each other.  No workgroup waits for another: the
 *     results are the same bits whenever and wherever the jobs run.
 *   - Contract: when the work of the next grad-h call is done, the hosted jobs are done.  At H = 64 (every form: fp32 or
 *     split, 1 <= D <= 4) they are tail workgroups of the grad-h kernel itself; at any other width the grad-h call launches
 *     them through qot_run_roles on its own stream right behind its kernel.  A grad-h call that returns an error before
 *     its launch drops them.  The state is taken (cleared) by that one call: a later grad-h call hosts nothing.
 *   - Host state only (thread-local, no device access): safe under stream capture.  Nothing is read from `roles` after
 *     the call returns. */
int qot_nnconv_gradh_host_roles(const qot_role_t* roles, int n_roles);

/* ---- row gather / scatter (LUT read-out and its adjoint) ---------------------------- */
int qot_rows_gather(const float* x, const int32_t* idx, float* out, int64_t n_idx, int C,
                    qot_stream_t stream);
/* grad_x must be zero-filled; idx values are unique (a boolean-mask selection) */
int qot_rows_scatter(const float* grad_out, const int32_t* idx, float* grad_x, int64_t n_idx, int C,
                     qot_stream_t stream);

/* ---- single-launch inference: the whole eval-mode TopologicalGNN forward -----------------------------------------
 * topological_training/models.py:49-64 with dropout off (test.py:58-64), for a block-diagonal batch of B graphs in ONE
 * launch: one workgroup per graph builds the graph's destination-sorted index in LDS, runs TransformerConv -> leaky_relu
 * -> NNConv aggr="mean" -> leaky_relu -> mean pool -> Linear -> leaky_relu -> Linear and writes out[b, 0..O).  Every sum
 * runs in a fixed order inside the graph's own workgroup: the result is bitwise reproducible and a graph's row does not
 * depend on which other graphs share the launch.  Plain fp32 FMA throughout.
 *
 * The batch as a collate leaves it (all int64, device): node_ids[N] (table rows, NOT offset), edge_index[2, E]
 * (row 0 = source, row 1 = target, offset by the graph's first node), edge_attr[E, D], node_ptr[B+1], edge_ptr[B+1].
 * n_max / max_e bound the largest graph (host-known; they size the LDS image).  Nodes of in-degree 0, graphs without
 * edges or with a single node, self loops and repeated edges are legal and come out as PyG's operators give them.
 *
 * Parameter-only tables (refresh them when the parameters change, not per batch), V = rows of the embedding table:
 *   t4  [V, ld4]  projected table [q|k|v|skip] (qot_table_project_fwd; ld4 >= 4H, a multiple of 4)
 *   M   [V, ldm]  score matrix and P [V, D] (qot_table_scores with n = V; ldm = qot_tconv_graph_ldm of V)
 *   wcat [(2D+2)*H, H] row-major: block k < 2D holds nn.2.weight[a*H + o, k] at [k*H + a, o], block 2D holds nn.2.bias
 *        [a*H + o], block 2D+1 holds lin.weight[o, a] (the NNConv root); read from global memory (L2-resident)
 * and the parameters read in place: w_edge [H, D] (conv1.lin_edge), w1 [2D, D] / b1 [2D] (conv2.nn.0), bias2 [H]
 * (conv2.bias), w0 [H, H] / b0 [H] (mlp.0), w3 [O, H] / b3 [O] (mlp.3).  slope_conv: leaky_relu slope behind both
 * convolutions (models.py:54,58: 0.01); slope_head: the read-out's LeakyReLU.
 *
 * Envelope (QOT_ERR_UNSUPPORTED outside it): H in {16, 32, 64}, 1 <= D <= 4, 1 <= O <= 8, n_max <= 128 and max_e within
 * the LDS budget -- qot_topological_infer_supported answers 1 / 0 from the kernel's own LDS layout, and
 * qot_topological_infer_max_edges gives the largest max_e it accepts for (n_max, H, D), -1 when none.
 * status (optional, device int32, caller-zeroed): bit 0 = an edge leaves its graph's node range, bit 1 = a graph
 * exceeds n_max / max_e or its slices leave the arrays, bit 2 = a node id outside [0, V); the rows of such graphs are
 * written as NaN. */
int qot_topological_infer_supported(int n_max, int max_e, int H, int D, int O);
int qot_topological_infer_max_edges(int n_max, int H, int D);
int qot_topological_infer(const int64_t* node_ids, const int64_t* edge_index, const float* edge_attr,
                          const int64_t* node_ptr, const int64_t* edge_ptr, int64_t N, int64_t E, int64_t B, int n_max,
                          int max_e, const float* t4, int ld4, const float* M, int ldm, const float* P, int V,
                          const float* w_edge, const float* w1, const float* b1, const float* wcat, const float* bias2,
                          const float* w0, const float* b0, const float* w3, const float* b3, float slope_conv,
                          float slope_head, float* out, int H, int D, int O, int32_t* status, qot_stream_t stream);

/* ---- Monte-Carlo dropout in one launch: T stochastic forwards of the same model and batch -------------------------
 * samples[t, b, 0..O) (fp32, [T, B, O]) is the output of a TRAIN-MODE forward of the engine on this batch at dropout step
 * first_step + t with base seed base_seed: leaky_relu + Dropout(p_conv) behind both convolutions, Dropout(p_head) inside
 * the read-out, masks by the rule at the top of this header -- keep = 16 bits of hash(site seed, step, flat / 4) >= thr16,
 * site seed = base_seed + 0x9E3779B97F4A7C15 * site (mod 2^64) with site 1 behind conv1, 2 behind conv2, 97 in the
 * read-out; flat = (node_ptr[b] + j) * H + c over the batch's [N, H] at the conv sites, b * H + c over [B, H] in the
 * read-out; kept values times 1 / (1 - p) in fp32.  A graph's draw therefore depends on its row offset in the batch (as in
 * training); a given (batch, seed, first_step, t) is bitwise reproducible and independent of T and chunk.  With p_conv ==
 * p_head == 0 every sample equals qot_topological_infer's row bit for bit (same sums in the same order, no multiply taken).
 *
 * Grid (B, ceil(T / chunk)): a workgroup builds its graph's index and the first convolution ONCE (nothing before conv1's
 * activation depends on the draw) and then runs NNConv, pool and read-out for chunk samples.  Everything else -- batch
 * layout, tables, status bits (all T rows of a flagged graph are NaN) -- as qot_topological_infer.  Envelope: that of
 * qot_topological_infer with a lower edge cap (the LDS image holds a masked copy of conv1's output: n_max * H more words);
 * qot_topological_infer_mc_supported / _max_edges answer from the kernel's own layout.  1 <= T <= 4096, 1 <= chunk <= T,
 * else QOT_ERR_UNSUPPORTED; first_step < 0 or a probability outside [0, 1): QOT_ERR_BADARG. */
int qot_topological_infer_mc_supported(int n_max, int max_e, int H, int D, int O);
int qot_topological_infer_mc_max_edges(int n_max, int H, int D);
int qot_topological_infer_mc(const int64_t* node_ids, const int64_t* edge_index, const float* edge_attr,
                             const int64_t* node_ptr, const int64_t* edge_ptr, int64_t N, int64_t E, int64_t B, int n_max,
                             int max_e, const float* t4, int ld4, const float* M, int ldm, const float* P, int V,
                             const float* w_edge, const float* w1, const float* b1, const float* wcat, const float* bias2,
                             const float* w0, const float* b0, const float* w3, const float* b3, float slope_conv,
                             float slope_head, float* samples, int H, int D, int O, int32_t* status, int T,
                             int64_t first_step, uint64_t base_seed, float p_conv, float p_head, int chunk,
                             qot_stream_t stream);

/* ---- per-link sensitivity in one launch (TopologicalPredictor.sensitivity) --------------------------
 * The eval-mode forward of qot_topological_infer -- the same sums in the same order: `out` is that entry's row bit for bit
 * -- followed, inside the graph's workgroup, by one back pass per requested output to the edge features:
 *   jac[q, e, d] = d out[graph(e), outputs[q]] / d edge_attr[e, d],   jac [Q, E, D] row-major, outputs [Q] device int32,
 * distinct values in 0 ... O - 1 (the caller checks the contents; 1 <= Q <= O is checked here).  Graphs are block-diagonal,
 * so this is the whole Jacobian.  The derivative of leaky_relu / relu at 0 is the forward's own branch (v > 0 ? 1 : slope;
 * relu: 0), torch's rule.  alpha (optional, [E]): TransformerConv's softmax weights in the order of edge_index.
 * No parameter or embedding gradient is formed and there is no float atomic anywhere: every element of jac, alpha and
 * every intermediate sum has one owning thread and a fixed order, so the result is bitwise reproducible and a graph's
 * slices do not depend on the other graphs of the batch.  Every jac / alpha element of a graph with edges is written once
 * (no zero fill needed).  Batch layout, tables and status bits as qot_topological_infer; a flagged graph gets NaN in its
 * out row, its jac slices and its alpha slice.
 * Envelope: that of qot_topological_infer with a lower edge cap (the LDS image also holds the adjoint of conv1's output,
 * one row tile of conv2's adjoint and 2 D words per edge); qot_topological_infer_grad_supported / _max_edges answer from
 * the kernel's own layout.  QOT_ERR_UNSUPPORTED: outside the envelope, Q outside 1 ... O, slope_conv <= 0 (conv1's branch
 * is read off the sign of its output); QOT_ERR_BADARG: a null required pointer. */
int qot_topological_infer_grad_supported(int n_max, int max_e, int H, int D, int O);
int qot_topological_infer_grad_max_edges(int n_max, int H, int D);
int qot_topological_infer_grad(const int64_t* node_ids, const int64_t* edge_index, const float* edge_attr,
                               const int64_t* node_ptr, const int64_t* edge_ptr, int64_t N, int64_t E, int64_t B, int n_max,
                               int max_e, const float* t4, int ld4, const float* M, int ldm, const float* P, int V,
                               const float* w_edge, const float* w1, const float* b1, const float* wcat, const float* bias2,
                               const float* w0, const float* b0, const float* w3, const float* b3, float slope_conv,
                               float slope_head, float* out, int H, int D, int O, int32_t* status, const int32_t* outputs,
                               int Q, float* jac, float* alpha, qot_stream_t stream);

/* ---- "what if" in one launch: the eval-mode forward of K edits of the batch's graphs ----------------
 * Candidate k names base graph graph[k] (null: graph 0 -- legal only with B == 1), removes the edges at positions
 * drop[drop_ptr[k] .. drop_ptr[k+1]) of edge_index (at most 32 per candidate; any order, a repeat counts once; drop and
 * drop_ptr null: no removals) and appends the edges add_edge_index[:, add_ptr[k] .. add_ptr[k+1]) ([2, A] int64, batch node
 * numbering as edge_index) with features add_edge_attr [A, D].  The edited graph holds the base graph's nodes, its
 * surviving edges in their order and the added edges behind them; out[k, 0..O) ([K, O]) is, bit for bit, the row
 * qot_topological_infer writes for that graph in any batch: the same code runs the same sums in the same order, and a
 * candidate's row does not depend on the other candidates.  Grid (K), one workgroup per candidate; the batch is only read.
 * max_add bounds the additions of one candidate (host-known).  Batch layout and tables as qot_topological_infer.
 * Envelope: that of qot_topological_infer with max_e + max_add in the place of max_e (the LDS image is the eval kernel's,
 * sized for a base graph and its additions; removals are not credited); qot_topological_infer_whatif_supported /
 * _max_edges answer for that sum and equal the eval kernel's.  QOT_ERR_BADARG: negative sizes, max_add > A, R > 0 without
 * drop / drop_ptr, graph null with B != 1, K > 0 with B == 0, a null required pointer; K == 0: QOT_OK, no launch.
 * status: bit 0 = an edge, added ones included, leaves its graph's node range; bit 1 = graph[k] outside 0 .. B-1, a drop
 * position outside that graph's edge slice, more than 32 removals or max_add additions, slices outside the arrays; bit 2
 * as qot_topological_infer.  Only the flagged candidate's row is NaN. */
int qot_topological_infer_whatif_supported(int n_max, int max_e, int H, int D, int O);
int qot_topological_infer_whatif_max_edges(int n_max, int H, int D);
int qot_topological_infer_whatif(const int64_t* node_ids, const int64_t* edge_index, const float* edge_attr,
                                 const int64_t* node_ptr, const int64_t* edge_ptr, int64_t N, int64_t E, int64_t B, int n_max,
                                 int max_e, const float* t4, int ld4, const float* M, int ldm, const float* P, int V,
                                 const float* w_edge, const float* w1, const float* b1, const float* wcat, const float* bias2,
                                 const float* w0, const float* b0, const float* w3, const float* b3, float slope_conv,
                                 float slope_head, float* out, int H, int D, int O, int32_t* status,
                                 const int64_t* add_edge_index, const float* add_edge_attr, const int64_t* add_ptr, int64_t A,
                                 const int64_t* drop, const int64_t* drop_ptr, int64_t R, const int64_t* graph, int64_t K,
                                 int max_add, qot_stream_t stream);

/* ---- single-launch inference: the eval-mode LightpathGNN forward of the LUT rows ------------------------------------
 * lightpath_training/models.py:7-45 with dropout off, reference architecture (ONE GATConv(heads = 4) -> BatchNorm on the
 * running statistics -> ReLU -> LUT rows -> Linear -> LeakyReLU -> Linear), for a block-diagonal batch in ONE launch, one
 * wavefront per output row.  A row depends on the one-hop in-neighbourhood of its LUT node only: the wave scans its graph's
 * edge slice for the messages into that node (dst == i and src != i, plus exactly one self loop: PyG's remove_self_loops
 * + add_self_loops; repeated edges are separate messages), forms the logits as leaky_relu(s_h . x_j + d_h . x_i) with
 * s_h = W_h^T att_src_h, d_h = W_h^T att_dst_h, takes the softmax per head (max subtraction, + 1e-16), and applies W_h to
 * u_h = sum_e alpha_e x_j.  No graph index is built and no other node's row is computed.  Every sum runs in one fixed order
 * given by the edge's offset inside its graph's slice (the messages one after the other by rising offset, the self loop
 * last): a row is bitwise reproducible and does not depend on the other graphs of the launch or on the mode.  fp32 FMA.
 *
 * The batch (device): x [N, F] raw features, edge_index [2, E] int64 (row 0 = source, row 1 = target, offset by the graph's
 * first node), node_ptr [B+1] / edge_ptr [B+1] int64 (the edges of a graph are one slice).
 *   rows mode   (lut_idx != NULL): lut_idx [L] int64 node numbers, batch [N] int64 (graph of every node); out [L, O].
 *   graphs mode (lut_idx == NULL): one row per graph; the wave tests x[n, lut_col] == 1.0f (exact) over the graph's nodes,
 *               writes count[g] (int32 [B]: LUT nodes found) and out[g, :] for the lowest-numbered one, NaN when there is
 *               none; out [B, O].  `batch` and L are not read.
 * The model's own parameters, read in place: w [4C, F] (conv1.lin.weight), att_src / att_dst [4, C], conv_bias [4C],
 * slope_att (conv1.negative_slope); bn_weight / bn_bias / bn_mean / bn_var [4C] and bn_eps (norm1.module, running
 * statistics); w0 [C, 4C] / b0 [C] (mlp.0), w3 [O, C] / b3 [O] (mlp.3), slope_head (mlp.1).
 *
 * Envelope (QOT_ERR_UNSUPPORTED outside it): 1 <= F <= 16, 1 <= C <= 256, 1 <= O <= 8, heads == 4, 0 <= lut_col < F.  No
 * cap on in-degree, graph size or batch size.
 * status (optional, device int32, caller-zeroed): bit 0 = an edge of the row's graph slice has an end outside the graph's
 * node range, bit 1 = a LUT index, graph number or slice outside the arrays; such rows are written as NaN and nothing is
 * read through the offending index. */
int qot_lightpath_infer(const float* x, const int64_t* edge_index, const int64_t* batch, const int64_t* node_ptr,
                        const int64_t* edge_ptr, const int64_t* lut_idx, int64_t L, int64_t N, int64_t E, int64_t B,
                        const float* w, const float* att_src, const float* att_dst, const float* conv_bias, float slope_att,
                        const float* bn_weight, const float* bn_bias, const float* bn_mean, const float* bn_var,
                        float bn_eps, const float* w0, const float* b0, const float* w3, const float* b3, float slope_head,
                        float* out, int32_t* count, int F, int C, int O, int heads, int lut_col, int32_t* status,
                        qot_stream_t stream);

/* ---- per-neighbour sensitivity of the LUT rows in one launch (LightpathPredictor.sensitivity) --------
 * The forward of qot_lightpath_infer -- the same sums in the same order: `out` (and `count`) are that entry's, bit for bit
 * -- followed, inside the row's wavefront, by the Jacobian of Q requested outputs wrt the node features of the row's
 * one-hop in-neighbourhood.  outputs [Q] device int32, distinct values in 0 ... O - 1 (the caller checks the contents; a
 * value outside that range gives NaN, nothing is read through it).  R = L (rows mode) or B (graphs mode) rows.
 *   jac_edge [Q, E, F]  for an edge e that is a message into computed row r (dst(e) is the row's node, src(e) != dst(e)):
 *                       d out[r, outputs[q]] / d x[src(e), :] THROUGH THAT MESSAGE (repeated edges are separate messages).
 *                       Every other edge is NOT WRITTEN: the caller zero-fills the array.
 *   jac_self [Q, R, F]  the derivative wrt the row's own features: the appended self loop's message and logit, and the
 *                       d_h . x_i term of every message's logit.
 *   alpha_self [R, 4], alpha_edge [E, 4] (optional, both may be NULL): conv1's softmax weights of the self loop and of the
 *                       message edges; alpha_edge is caller-zeroed like jac_edge.
 * With J[q] = zeros(N, F): J[q].index_add_(0, src, jac_edge[q]); J[q][row nodes] += jac_self[q] is x.grad of
 * out[:, outputs[q]].sum() -- the LUT selection taken as constant.  leaky_relu' / relu' at 0 as torch (v > 0 ? 1 : slope;
 * relu: 0).  No float atomics: an edge has one destination, so every element has at most one owning wave, and every sum
 * has one order (the destination-side sums run over the messages by rising offset in the graph's slice): bitwise
 * reproducible, independent of the other graphs of the launch and of the mode.
 * A row that is not computed (flagged as in qot_lightpath_infer, or a graph without a LUT node in graphs mode) has NaN in
 * its out, jac_self and alpha_self rows; a flagged row whose graph's edge slice lies inside the edge array also writes NaN
 * over that slice of jac_edge / alpha_edge.
 * Envelope and return codes of qot_lightpath_infer, plus QOT_ERR_UNSUPPORTED for Q outside 1 ... O, and -- when there are
 * rows -- QOT_ERR_BADARG for a NULL outputs, jac_self or (E > 0) jac_edge. */
int qot_lightpath_infer_grad(const float* x, const int64_t* edge_index, const int64_t* batch, const int64_t* node_ptr,
                             const int64_t* edge_ptr, const int64_t* lut_idx, int64_t L, int64_t N, int64_t E, int64_t B,
                             const float* w, const float* att_src, const float* att_dst, const float* conv_bias,
                             float slope_att, const float* bn_weight, const float* bn_bias, const float* bn_mean,
                             const float* bn_var, float bn_eps, const float* w0, const float* b0, const float* w3,
                             const float* b3, float slope_head, float* out, int32_t* count, int F, int C, int O, int heads,
                             int lut_col, int32_t* status, const int32_t* outputs, int Q, float* jac_self, float* jac_edge,
                             float* alpha_self, float* alpha_edge, qot_stream_t stream);

/* ---- "what if" for the LUT rows: K candidate lightpaths in one launch (LightpathPredictor.what_if) ---
 * Rows mode only: lut_idx [K] names the candidates' nodes (repeats are the normal case), L == K, count must be NULL.
 * Candidate k
 *   - replaces its node's feature row by x_lut[k, 0..F) (x_lut [K, F]; NULL: every candidate keeps its node's row);
 *   - removes the edges at positions drop[drop_ptr[k] .. drop_ptr[k+1]) of edge_index (at most 32 per candidate; any
 *     order, a repeat counts once; they must lie in the edge slice of the node's graph; a removed edge is not looked at
 *     further, an edge that is no message into the node changes nothing; drop_ptr NULL: no removals);
 *   - appends the messages add_src[add_ptr[k] .. add_ptr[k+1]) -> its node behind the surviving edges, in the order given
 *     (int64 node numbers of the batch inside the node's graph; a source equal to the node is an input self loop and no
 *     message; a source that sends already sends once more; no cap on their number; add_ptr NULL: no additions).
 * out[k, 0..O) ([K, O]) is, bit for bit, the row qot_lightpath_infer writes for that node in the explicitly built graph
 * (the base graph's nodes with that one row replaced, its surviving edges in their order, the added edges behind them):
 * the same code runs the same sums in the same order -- the messages one after the other by rising position, the
 * additions behind the slice, the self loop last.  A candidate's row does not depend on the other candidates, and a
 * candidate without an edit has qot_lightpath_infer's row.  One wavefront per candidate, each rescans its graph's edge
 * slice; the batch is only read.  Everything else as qot_lightpath_infer.
 * Return codes, before any launch, in that entry's order: QOT_ERR_BADARG for a negative size or L != K, then the
 * envelope (QOT_ERR_UNSUPPORTED), then -- when K > 0 -- QOT_ERR_BADARG for a NULL required pointer, a NULL lut_idx, a
 * non-NULL count, A > 0 without add_src / add_ptr or R > 0 without drop / drop_ptr.  K == 0: QOT_OK, no launch.
 * status: bit 0 = an edge of the slice that is not removed, or an added source, leaves the graph's node range; bit 1 =
 * lut_idx[k] outside 0 .. N-1, a drop position outside the graph's edge slice, more than 32 removals, list slices or graph
 * slices outside the arrays; bit 2 = the candidate's effective feature row does not hold exactly 1.0f in column lut_col.
 * Only the flagged candidate's row is NaN; nothing is read through an offending index. */
int qot_lightpath_infer_whatif(const float* x, const int64_t* edge_index, const int64_t* batch, const int64_t* node_ptr,
                               const int64_t* edge_ptr, const int64_t* lut_idx, int64_t L, int64_t N, int64_t E, int64_t B,
                               const float* w, const float* att_src, const float* att_dst, const float* conv_bias,
                               float slope_att, const float* bn_weight, const float* bn_bias, const float* bn_mean,
                               const float* bn_var, float bn_eps, const float* w0, const float* b0, const float* w3,
                               const float* b3, float slope_head, float* out, int32_t* count, int F, int C, int O, int heads,
                               int lut_col, int32_t* status, const float* x_lut, const int64_t* add_src,
                               const int64_t* add_ptr, int64_t A, const int64_t* drop, const int64_t* drop_ptr, int64_t R,
                               int64_t K, qot_stream_t stream);

/* ---- graph construction from network-status samples (csrc/status_graph.hip) ----------------
 * data [S, P, L, Q] fp64 (sample, lp_feat, link, freq), target [S, M] fp64, freq [Q] fp64, all on the device.  samples
 * [G] int64 picks the samples of the call, in order, repeats allowed (NULL: samples 0 .. G-1).  One workgroup per
 * sample.  A channel (l, q) is occupied when any of its P values != 0 (a NaN counts); scan order is l * Q + q; the
 * lightpaths are the distinct trunc(conn_id) values, attributes from the first occupied channel of each.
 *
 *   QOT_SG_LIGHTPATH    nodes = lightpaths in first-seen order; a -- b when a link that carries at least two lightpaths
 *                       has an occupied channel of each with 0 < |freq[q1] - freq[q2]| < freq_threshold (fp64); a == b
 *                       gives one self loop.
 *   QOT_SG_TOPOLOGICAL  75 nodes; one link per unordered {src_id - 1, dst_id - 1} pair, carrying the features of the
 *                       lightpath with the largest conn of the pair.
 * Directed links of a graph are sorted by (source, target); both directions of a link, a self loop once.
 *
 * qot_status_graph_count writes info [2 + 2 G] int32 (caller-zeroed): info[0] the status word (QOT_SG_BAD_*, OR-ed over
 * the samples), info[1] != 0 when some graph has a self loop, info[2 + 2 g] / info[3 + 2 g] nodes / directed links of
 * graph g; and the scratch (qot_status_graph_scratch_bytes, 16-byte aligned) that qot_status_graph_fill reads.  The host
 * reads info once, forms the exclusive prefix sums node_ptr / edge_ptr [G + 1] int64 (device copies are passed to fill)
 * and allocates the outputs.  Nothing read from data is used as an index unchecked; fill writes nothing for a graph
 * whose offsets do not match info.
 *
 * qot_status_graph_fill: cols [ncol, 4] fp64, one row per output column: (lp_feat row, min, max - min, has_range); row
 * -1 (lightpath only) is the is_lut column, 1.0f iff osnr == snr == ber == -1 on the first channel.  tcols [3, 4]
 * likewise over the columns of target (-1: absent, reads 0.0).  A column is ((v - min) / (max - min)) in fp64 rounded
 * once to fp32, or v rounded to fp32 without a range.  Outputs: edge_index [2, e_total] int64 (shard numbering), feat =
 * x [n_total, ncol] (lightpath) or edge_attr [e_total, ncol] (topological), node_ids [n_total] int64 (topological
 * only), y [G, 3].
 *
 * Envelope: any L, P, S with L * Q < 2^31; Q <= QOT_SG_MAX_FREQS (QOT_ERR_UNSUPPORTED above); at most
 * QOT_SG_MAX_LIGHTPATHS lightpaths per sample (QOT_SG_TOO_MANY in the status word above). */
#define QOT_SG_LIGHTPATH 0
#define QOT_SG_TOPOLOGICAL 1
#define QOT_SG_MAX_FREQS 1024
#define QOT_SG_MAX_LIGHTPATHS 256
#define QOT_SG_NODES 75
#define QOT_SG_BAD_CONN 1      /* conn_id not finite or beyond +-2^53 */
#define QOT_SG_TOO_MANY 2      /* more than QOT_SG_MAX_LIGHTPATHS lightpaths in a sample */
#define QOT_SG_BAD_ENDPOINT 4  /* topological: src_id / dst_id outside 1 .. 75 or not integral */
#define QOT_SG_BAD_SAMPLE 8    /* sample number outside [0, S) */
size_t qot_status_graph_scratch_bytes(int64_t G, int64_t L, int64_t Q, int representation);
int qot_status_graph_count(const double* data, const double* freq, const int64_t* samples, int64_t G, int64_t S, int P,
                           int64_t L, int64_t Q, int conn_row, int src_row, int dst_row, double freq_threshold,
                           int representation, void* scratch, size_t scratch_bytes, int32_t* info, qot_stream_t stream);
int qot_status_graph_fill(const double* data, const double* target, const int64_t* samples, int64_t G, int64_t S, int P,
                          int64_t L, int64_t Q, int M, int osnr_row, int snr_row, int ber_row, const double* cols, int ncol,
                          const double* tcols, int representation, const void* scratch, const int32_t* info,
                          const int64_t* node_ptr, const int64_t* edge_ptr, int64_t n_total, int64_t e_total,
                          int64_t* edge_index, float* feat, int64_t* node_ids, float* y, qot_stream_t stream);

/* ---- the LUT row of every network-status sample in one launch (LightpathPredictor.from_status) -------
 * From data [S, P, L, Q] fp64 to out [G, O] fp32 and count [G] int64 without a graph in between: for sample samples[g]
 * (NULL: sample g), count[g] is the number of lightpaths with osnr == snr == ber == -1 on their first channel and out[g]
 * the row of the first-seen one (NaN when there is none).  Both are, bit for bit, what qot_lightpath_infer's graphs mode
 * gives for the QOT_SG_LIGHTPATH graph that qot_status_graph_count / _fill build of that sample with the same cols and
 * freq_threshold: the lightpaths are the same first-seen table, the feature rows the same fp64 scaling rounded once, the
 * interferers of the row's lightpath a -- every b != a that shares a link with a on slots with 0 < |freq[q1] - freq[q2]|
 * < freq_threshold (fp64), once however many links and slots the pair shares -- are summed one after the other by rising
 * lightpath number, the self loop last, by the same row routine.  One 256-thread workgroup per sample; no workspace.
 *
 * The argument list is qot_lightpath_infer's up to `status`, then the sample's.  There is no batch: x, edge_index, batch,
 * node_ptr, edge_ptr and lut_idx must be NULL and n_lut, N, E 0 (QOT_ERR_BADARG otherwise); G takes B's place; count is
 * int64 here.  cols [ncol, 4] fp64 as qot_status_graph_fill's, ncol == F, and the is_lut column (row -1) at lut_col.
 * Return codes before any launch: QOT_ERR_BADARG for a negative size, P, L or Q < 1; the envelope of qot_lightpath_infer
 * and Q <= QOT_SG_MAX_FREQS, L * Q < 2^31, G < 2^31 (QOT_ERR_UNSUPPORTED); QOT_ERR_BADARG for ncol != F, a row outside
 * 0 .. P-1, a freq_threshold that is not a finite positive number and -- when G > 0 -- a NULL required pointer or S == 0.
 * G == 0: QOT_OK, no launch.
 * status (optional, device int32, caller-zeroed), on the device since nothing is read back; the bits lie above
 * qot_lightpath_infer's and _whatif's (1, 2, 4).  The flagged sample's row is NaN and its count 0, the other rows are
 * untouched; no index is formed from an offending value. */
#define QOT_LP_STATUS_BAD_CONN 8     /* a conn_id not finite or beyond +-2^53 */
#define QOT_LP_STATUS_TOO_MANY 16    /* more than QOT_SG_MAX_LIGHTPATHS lightpaths in a sample */
#define QOT_LP_STATUS_BAD_SAMPLE 32  /* a sample number outside [0, S) */
int qot_lightpath_infer_status(const float* x, const int64_t* edge_index, const int64_t* batch, const int64_t* node_ptr,
                               const int64_t* edge_ptr, const int64_t* lut_idx, int64_t n_lut, int64_t N, int64_t E, int64_t G,
                               const float* w, const float* att_src, const float* att_dst, const float* conv_bias,
                               float slope_att, const float* bn_weight, const float* bn_bias, const float* bn_mean,
                               const float* bn_var, float bn_eps, const float* w0, const float* b0, const float* w3,
                               const float* b3, float slope_head, float* out, int64_t* count, int F, int C, int O, int heads,
                               int lut_col, int32_t* status, const double* data, const double* freq, const int64_t* samples,
                               int64_t S, int P, int64_t L, int64_t Q, int conn_row, int osnr_row, int snr_row, int ber_row,
                               const double* cols, int ncol, double freq_threshold, qot_stream_t stream);

/* ---- K candidate lightpaths placed into network-status samples, one launch (LightpathPredictor.place)
 * Candidate k is the raw lp_feat vector values[k, P] (fp64, status units) written into the channels cells[:, cell_ptr[k] :
 * cell_ptr[k + 1]] of sample samples[k]; cells [2, M] int64 holds link indices, then frequency indices; cell_ptr [K + 1]
 * int64; samples [K] int64 (required; repeats are the normal case).  Let edited_k be that sample with values[k] in each of
 * the candidate's cells.  out[k] is, bit for bit, the row that graphs mode of the eval entry gives the candidate's node in
 * the QOT_SG_LIGHTPATH graph of edited_k (same cols, same freq_threshold), and count[k] the lightpaths of edited_k with
 * osnr == snr == ber == -1 on their first channel: the sample's own flagged ones plus one.  When the candidate is the
 * first-seen flagged lightpath of edited_k this is what the status entry above gives for edited_k.  edited_k is never
 * built and data is never written: the candidate fills free channels, so the other lightpaths keep their first-seen
 * numbers; its interferers -- every lightpath of the sample on a slot with 0 < |freq[q1] - freq[q2]| < freq_threshold
 * (fp64) of the link of one of its cells, once each; a pair of its own cells names nobody -- are summed by rising
 * first-seen number, the self loop last.  One 256-thread workgroup per candidate: O(L Q) for the scan plus O(cells Q); no
 * cap on the cells of a candidate, duplicates allowed; no workspace.
 *
 * The argument list is the status entry's up to freq_threshold (K takes G's place; the batch arguments of the common
 * prefix must be empty), then values, cells, cell_ptr, M.  Return codes before any launch: the status entry's, and
 * QOT_ERR_BADARG for M < 0 or -- when K > 0 -- a NULL samples, values or cell_ptr, or NULL cells with M > 0.  K == 0:
 * QOT_OK, no launch.
 * status, on the device since nothing is read back: the refused candidate's row is NaN and its count 0, the other rows
 * are untouched; nothing read from data or values is used as an index.  The bits lie beside QOT_LP_STATUS_*, which are
 * reused: BAD_CONN also for a candidate conn_id that is not finite or beyond +-2^53, TOO_MANY for a sample that holds
 * QOT_SG_MAX_LIGHTPATHS lightpaths already (edited_k would hold one more), BAD_SAMPLE as there. */
#define QOT_LP_PLACE_BAD_CELL 64     /* a link / frequency index outside [0, L) / [0, Q), or a cell_ptr slice that is empty, descending or beyond M */
#define QOT_LP_PLACE_OCCUPIED 128    /* a cell whose channel is occupied in the sample */
#define QOT_LP_PLACE_CONN_TAKEN 256  /* the candidate's conn_id equals a lightpath of the sample */
#define QOT_LP_PLACE_NOT_LUT 512     /* values[k] without osnr == snr == ber == -1 */
int qot_lightpath_infer_place(const float* x, const int64_t* edge_index, const int64_t* batch, const int64_t* node_ptr,
                              const int64_t* edge_ptr, const int64_t* lut_idx, int64_t n_lut, int64_t N, int64_t E, int64_t K,
                              const float* w, const float* att_src, const float* att_dst, const float* conv_bias,
                              float slope_att, const float* bn_weight, const float* bn_bias, const float* bn_mean,
                              const float* bn_var, float bn_eps, const float* w0, const float* b0, const float* w3,
                              const float* b3, float slope_head, float* out, int64_t* count, int F, int C, int O, int heads,
                              int lut_col, int32_t* status, const double* data, const double* freq, const int64_t* samples,
                              int64_t S, int P, int64_t L, int64_t Q, int conn_row, int osnr_row, int snr_row, int ber_row,
                              const double* cols, int ncol, double freq_threshold, const double* values, const int64_t* cells,
                              const int64_t* cell_ptr, int64_t M, qot_stream_t stream);

/* ---- the TopologicalGNN row of every network-status sample in one launch (TopologicalPredictor.from_status, DESIGN.md
 * 4.21) -- From data [S, P, L, Q] fp64 to out [G, O] fp32 and links [G] int64 without a graph in between: for sample
 * samples[g] (NULL: sample g), out[g] is, bit for bit, the row qot_topological_infer writes for the QOT_SG_TOPOLOGICAL
 * graph that qot_status_graph_count / _fill build of that sample with the same cols, and links[g] that graph's directed
 * link count.  The lightpaths are the same first-seen table; among the lightpaths of one unordered node pair the largest
 * conn wins; a winner with u != v gives the links (u, v) and (v, u), one with u == v the self loop; the links are numbered
 * ascending by (source, target); a link's features are the winner's, the same fp64 scaling rounded once (a row outside
 * 0 .. P-1 reads 0); the forward is the eval kernel's code behind another edge source.  One 256-thread workgroup per
 * sample; no workspace.
 *
 * The argument list is qot_topological_infer's up to `status`, then the sample's.  There is no batch: node_ids is the
 * caller's arange(QOT_SG_NODES) with N == n_max == QOT_SG_NODES, max_e must be 512 (2 x QOT_SG_MAX_LIGHTPATHS, the
 * kernel's own edge cap), edge_index, edge_attr, node_ptr and edge_ptr must be NULL and E 0 (QOT_ERR_BADARG otherwise); G
 * takes B's place.  cols [ncol, 4] fp64 as qot_status_graph_fill's, ncol == D.
 * Return codes before any launch: QOT_ERR_BADARG for a negative size, P, L or Q < 1; the envelope of
 * qot_topological_infer at (75, 512) with this kernel's static LDS added to the image, Q <= QOT_SG_MAX_FREQS, L * Q <
 * 2^31, G < 2^31 (QOT_ERR_UNSUPPORTED); QOT_ERR_BADARG for ncol != D, a row outside 0 .. P-1 and -- when G > 0 -- a NULL
 * required pointer, a bad ld4 / ldm or S == 0.  G == 0: QOT_OK, no launch.
 * status (optional, device int32, caller-zeroed), on the device since nothing is read back; the bits lie above
 * qot_topological_infer's (1, 2, 4).  The flagged sample's row is NaN and its links 0, the other rows are untouched; no
 * index is formed from an offending value. */
#define QOT_TOPO_STATUS_BAD_CONN 8       /* a conn_id not finite or beyond +-2^53 */
#define QOT_TOPO_STATUS_TOO_MANY 16      /* more than QOT_SG_MAX_LIGHTPATHS lightpaths in a sample */
#define QOT_TOPO_STATUS_BAD_SAMPLE 32    /* a sample number outside [0, S) */
#define QOT_TOPO_STATUS_BAD_ENDPOINT 64  /* a src_id / dst_id that is not an integer in 1 .. QOT_SG_NODES */
int qot_topological_infer_status(const int64_t* node_ids, const int64_t* edge_index, const float* edge_attr,
                                 const int64_t* node_ptr, const int64_t* edge_ptr, int64_t N, int64_t E, int64_t G, int n_max,
                                 int max_e, const float* t4, int ld4, const float* M, int ldm, const float* P, int V,
                                 const float* w_edge, const float* w1, const float* b1, const float* wcat, const float* bias2,
                                 const float* w0, const float* b0, const float* w3, const float* b3, float slope_conv,
                                 float slope_head, float* out, int H, int D, int O, int32_t* status, int64_t* links,
                                 const double* data, const int64_t* samples, int64_t S, int rows, int64_t L, int64_t Q,
                                 int conn_row, int src_row, int dst_row, const double* cols, int ncol, qot_stream_t stream);

/* ---- K candidate lightpaths placed into network-status samples, the TopologicalGNN row of each in one launch
 * (TopologicalPredictor.place) -- Candidate k is the raw lp_feat vector values[k, rows] (fp64, status
 * units) written into the channels cells[:, cell_ptr[k] : cell_ptr[k + 1]] of sample samples[k]; cells [2, n_cells] int64
 * holds link indices, then frequency indices; cell_ptr [K + 1] int64; samples [K] int64 (required; repeats are the normal
 * case).  Let edited_k be that sample with values[k] in each of the candidate's cells.  out[k] and links[k] are, bit for
 * bit, what the status entry above gives for edited_k with the same cols.  edited_k is never built and data is never
 * written: the candidate fills free channels, so the sample's lightpaths keep their first channels, and the candidate
 * joins the pair contest as one more lightpath whose end nodes and features come from values[k] -- when its trunc(conn_id)
 * is the largest on its unordered node pair (or the pair is new: 2 more links, 1 for a self loop) the pair's links carry
 * its features, otherwise the row is the unedited sample's.  The cells decide only whether the placement is legal.  One
 * 256-thread workgroup per candidate: O(L Q) for the scan plus O(cells); no cap on the cells of a candidate, duplicates
 * allowed; no workspace.
 *
 * The argument list is the status entry's up to ncol (K takes G's place), then values, cells, cell_ptr, n_cells.  Return
 * codes before any launch: the status entry's, and QOT_ERR_BADARG for n_cells < 0 or -- when K > 0 -- a NULL samples,
 * values or cell_ptr, or NULL cells with n_cells > 0.  K == 0: QOT_OK, no launch.
 * status, on the device since nothing is read back: the refused candidate's row is NaN and its links 0, the other rows
 * are untouched; nothing read from data or values is used as an index before it is checked.  The bits lie beside
 * QOT_TOPO_STATUS_*, which are reused: BAD_CONN also for a candidate conn_id that is not finite or beyond +-2^53,
 * BAD_ENDPOINT also for a candidate src_id / dst_id that is no integer in 1 .. QOT_SG_NODES, TOO_MANY for a sample that
 * holds QOT_SG_MAX_LIGHTPATHS lightpaths already (edited_k would hold one more), BAD_SAMPLE as there. */
#define QOT_TOPO_PLACE_BAD_CELL 128    /* a link / frequency index outside [0, L) / [0, Q), or a cell_ptr slice that is empty, descending or beyond n_cells */
#define QOT_TOPO_PLACE_OCCUPIED 256    /* a cell whose channel is occupied in the sample */
#define QOT_TOPO_PLACE_CONN_TAKEN 512  /* the candidate's conn_id equals a lightpath of the sample */
int qot_topological_infer_place(const int64_t* node_ids, const int64_t* edge_index, const float* edge_attr,
                                const int64_t* node_ptr, const int64_t* edge_ptr, int64_t N, int64_t E, int64_t K, int n_max,
                                int max_e, const float* t4, int ld4, const float* M, int ldm, const float* P, int V,
                                const float* w_edge, const float* w1, const float* b1, const float* wcat, const float* bias2,
                                const float* w0, const float* b0, const float* w3, const float* b3, float slope_conv,
                                float slope_head, float* out, int H, int D, int O, int32_t* status, int64_t* links,
                                const double* data, const int64_t* samples, int64_t S, int rows, int64_t L, int64_t Q,
                                int conn_row, int src_row, int dst_row, const double* cols, int ncol, const double* values,
                                const int64_t* cells, const int64_t* cell_ptr, int64_t n_cells, qot_stream_t stream);

/* ---- the two place entries with established lightpaths RELEASED in the same launch: a reroute, or an admission together
 * with a tear-down (LightpathPredictor.place / TopologicalPredictor.place with release=) -- Candidate k
 * names, beside the place entry's arguments, the conns release[release_ptr[k] : release_ptr[k + 1]] (release [R] int64,
 * release_ptr [K + 1] int64; an empty slice and a conn named twice are allowed, at most QOT_PLACE_MAX_RELEASE per
 * candidate).  Let edited_k be sample samples[k] with all rows zeroed in every occupied channel whose trunc(conn_id) is one
 * of them (occupancy and conn as everywhere: any value != 0; a conn_id of 0 in an occupied channel is conn 0), then
 * values[k] written into the candidate's cells.  out[k] and count[k] / links[k] are, bit for bit, what the place entry's
 * definition says of this edited_k: the lightpath entry gives the row of the candidate's node and the flagged survivors
 * plus one, the topological entry what its status entry gives for edited_k.  edited_k is never built and data is never
 * written.  Releasing zeroes whole channels and the candidate fills channels that are free afterwards, so a survivor keeps
 * its first channel and the survivors their relative first-seen order: the messages of the lightpath row are the
 * surviving interferers' by rising first-seen number of the unedited sample, the self loop last; in the pair contest a
 * released lightpath takes no part, so its pair goes to the largest surviving conn, to the candidate, or disappears.
 *
 * Each argument list is its place entry's up to M / n_cells, then release, release_ptr, R.  Return codes before any
 * launch: the place entry's, and QOT_ERR_BADARG for R < 0 or -- when K > 0 -- a NULL release_ptr, or NULL release with
 * R > 0.  K == 0: QOT_OK, no launch.
 * status: the place entry's bits with these differences -- OCCUPIED only for a cell whose owner survives; CONN_TAKEN and
 * (topological) BAD_ENDPOINT are tested against the survivors and the candidate, so the candidate may carry a released
 * conn_id; TOO_MANY for survivors + 1 > QOT_SG_MAX_LIGHTPATHS, and still for more than QOT_SG_MAX_LIGHTPATHS lightpaths in
 * the unedited sample, which the table cannot hold -- and the two below.  The release_ptr slice is checked against [0, R]
 * and the cap before release is read; nothing read from data, values or release is used as an index: conns are only
 * compared. */
#define QOT_PLACE_MAX_RELEASE 32            /* released lightpaths per candidate */
#define QOT_LP_PLACE_NO_SUCH_CONN 1024      /* a released conn that is no lightpath of the sample */
#define QOT_LP_PLACE_BAD_RELEASE 2048       /* a release_ptr slice that is descending, beyond R or longer than QOT_PLACE_MAX_RELEASE */
#define QOT_TOPO_PLACE_NO_SUCH_CONN 1024    /* a released conn that is no lightpath of the sample */
#define QOT_TOPO_PLACE_BAD_RELEASE 2048     /* a release_ptr slice that is descending, beyond R or longer than QOT_PLACE_MAX_RELEASE */
int qot_lightpath_infer_place_release(const float* x, const int64_t* edge_index, const int64_t* batch, const int64_t* node_ptr,
                                      const int64_t* edge_ptr, const int64_t* lut_idx, int64_t n_lut, int64_t N, int64_t E,
                                      int64_t K, const float* w, const float* att_src, const float* att_dst,
                                      const float* conv_bias, float slope_att, const float* bn_weight, const float* bn_bias,
                                      const float* bn_mean, const float* bn_var, float bn_eps, const float* w0, const float* b0,
                                      const float* w3, const float* b3, float slope_head, float* out, int64_t* count, int F,
                                      int C, int O, int heads, int lut_col, int32_t* status, const double* data,
                                      const double* freq, const int64_t* samples, int64_t S, int P, int64_t L, int64_t Q,
                                      int conn_row, int osnr_row, int snr_row, int ber_row, const double* cols, int ncol,
                                      double freq_threshold, const double* values, const int64_t* cells,
                                      const int64_t* cell_ptr, int64_t M, const int64_t* release, const int64_t* release_ptr,
                                      int64_t R, qot_stream_t stream);
int qot_topological_infer_place_release(const int64_t* node_ids, const int64_t* edge_index, const float* edge_attr,
                                        const int64_t* node_ptr, const int64_t* edge_ptr, int64_t N, int64_t E, int64_t K,
                                        int n_max, int max_e, const float* t4, int ld4, const float* M, int ldm, const float* P,
                                        int V, const float* w_edge, const float* w1, const float* b1, const float* wcat,
                                        const float* bias2, const float* w0, const float* b0, const float* w3, const float* b3,
                                        float slope_conv, float slope_head, float* out, int H, int D, int O, int32_t* status,
                                        int64_t* links, const double* data, const int64_t* samples, int64_t S, int rows,
                                        int64_t L, int64_t Q, int conn_row, int src_row, int dst_row, const double* cols,
                                        int ncol, const double* values, const int64_t* cells, const int64_t* cell_ptr,
                                        int64_t n_cells, const int64_t* release, const int64_t* release_ptr, int64_t R,
                                        qot_stream_t stream);

/* ---- the place entry together with a RETEST of the established lightpaths the candidate disturbs, one launch
 * (LightpathPredictor.place_impact) -- out[k] and count[k] are the place entry's, bit for bit.  The
 * candidate's interferers are, by symmetry of the interference rule, the only lightpaths of its sample whose own
 * neighbourhood it changes.  n_affected[k] (int64) is their number; the first A = max_affected of them by rising
 * first-seen number get a slot i: affected[k, i] (int64 [K, A]) is the lightpath's trunc(conn_id), before[k, i] / after[k,
 * i] (fp32 [K, A, O]) the row of that lightpath scored as the lightpath under test of sample samples[k] without / with the
 * candidate established next to it.  "Scored as the lightpath under test": the row that graphs mode of the eval entry
 * gives the lightpath's node in the QOT_SG_LIGHTPATH graph of the sample in which its channels carry osnr = snr = ber = -1
 * and -- after -- values[k] with osnr = snr = ber = 0 lies in the candidate's cells: the lightpath's own feature row with 1
 * in the is_lut column, the messages of its own interferers (found by the status entry's walk over its channels of the
 * unedited sample) by rising first-seen number with their is_lut as the sample has it, and -- after -- the candidate's
 * row, is_lut 0, at the candidate's first-seen position: behind the lightpaths whose first channel l * Q + q lies below
 * the smallest of its cells.  cols must not scale osnr, snr or ber (the caller's check: cols lives on the device).  Slots
 * i >= min(n_affected[k], A) hold -1 / NaN; n_affected[k] > A is no error.  A refused candidate (the place entry's status
 * bits, no new one) has a NaN out row, count 0, n_affected 0, affected -1, before and after NaN.  data is never written.
 * One 256-thread workgroup per candidate: the place entry's cost plus one slot walk per channel of a slotted lightpath and
 * two rows per slot.
 *
 * The argument list is the place entry's up to M, then affected, n_affected, before, after, max_affected.  Return codes
 * before any launch: the place entry's, QOT_ERR_BADARG for max_affected outside 1 .. QOT_PLACE_MAX_AFFECTED or -- when K >
 * 0 -- a NULL affected, n_affected, before or after.  K == 0: QOT_OK, no launch. */
#define QOT_PLACE_MAX_AFFECTED 32           /* retested lightpaths per candidate (their byte maps: 32 x 256 B of LDS) */
int qot_lightpath_infer_place_impact(const float* x, const int64_t* edge_index, const int64_t* batch, const int64_t* node_ptr,
                                     const int64_t* edge_ptr, const int64_t* lut_idx, int64_t n_lut, int64_t N, int64_t E,
                                     int64_t K, const float* w, const float* att_src, const float* att_dst,
                                     const float* conv_bias, float slope_att, const float* bn_weight, const float* bn_bias,
                                     const float* bn_mean, const float* bn_var, float bn_eps, const float* w0, const float* b0,
                                     const float* w3, const float* b3, float slope_head, float* out, int64_t* count, int F,
                                     int C, int O, int heads, int lut_col, int32_t* status, const double* data,
                                     const double* freq, const int64_t* samples, int64_t S, int P, int64_t L, int64_t Q,
                                     int conn_row, int osnr_row, int snr_row, int ber_row, const double* cols, int ncol,
                                     double freq_threshold, const double* values, const int64_t* cells,
                                     const int64_t* cell_ptr, int64_t M, int64_t* affected, int64_t* n_affected, float* before,
                                     float* after, int max_affected, qot_stream_t stream);

/* ---- every ESTABLISHED lightpath of a network-status sample, or a named subset, retested as the lightpath under test in
 * one launch (LightpathPredictor.retest) -- Sample samples[g] (NULL: sample g) has n[g] (int64) lightpaths
 * and count[g] flagged ones (the status entry's count).  M = max_lightpaths slots per sample: conn[g, i] (int64 [G, M]) is
 * the trunc(conn_id) of the lightpath in slot i, out[g, i] (fp32 [G, M, O]) that lightpath "scored as the lightpath under
 * test" as the place_impact entry defines it for `before`: its own feature row with 1 in the is_lut column, the messages of
 * its own interferers by rising first-seen number with their is_lut as the sample has it.  conns == NULL: slot i holds
 * lightpath number i of the first-seen order (the node order of the QOT_SG_LIGHTPATH graph) while i < n[g]; n[g] > M is no
 * error.  conns (int64 [G, M]): slot i holds the lightpath whose conn is conns[g, i]; -1 is an empty slot; a conn named
 * twice gives equal rows; a conn the sample does not hold leaves the slot empty and sets QOT_LP_RETEST_NO_SUCH_CONN.  An
 * empty slot holds conn -1 and a NaN row.  cols must not scale osnr, snr or ber (the caller's check).  data is never
 * written.  G * ceil(M / chunk) 256-thread workgroups; a workgroup discovers its sample, marks the neighbourhoods of its
 * chunk slots in one rescan and computes their rows one after the other in one wave, so no result depends on chunk.
 *
 * The argument list is the status entry's up to freq_threshold, then conns, conn, n, max_lightpaths, chunk.  Return codes
 * before any launch: the status entry's, QOT_ERR_BADARG for max_lightpaths outside 1 .. QOT_SG_MAX_LIGHTPATHS or chunk
 * outside 1 .. QOT_LP_RETEST_MAX_CHUNK, QOT_ERR_UNSUPPORTED for G * ceil(M / chunk) >= 2^31, QOT_ERR_BADARG -- when G > 0 --
 * for a NULL conn or n.  G == 0: QOT_OK, no launch.
 * status: QOT_LP_STATUS_BAD_CONN / TOO_MANY / BAD_SAMPLE as the status entry -- all M rows of that sample NaN, its conn
 * -1, n = count = 0, the other samples untouched -- and the bit below.  Nothing read from data or conns is used as an
 * index: conns are only compared. */
#define QOT_LP_RETEST_MAX_CHUNK 32          /* slots one workgroup runs one after the other (their byte maps: 32 x 256 B of LDS) */
#define QOT_LP_RETEST_NO_SUCH_CONN 4096     /* a named conn that is no lightpath of the sample */
int qot_lightpath_infer_retest(const float* x, const int64_t* edge_index, const int64_t* batch, const int64_t* node_ptr,
                               const int64_t* edge_ptr, const int64_t* lut_idx, int64_t n_lut, int64_t N, int64_t E, int64_t G,
                               const float* w, const float* att_src, const float* att_dst, const float* conv_bias,
                               float slope_att, const float* bn_weight, const float* bn_bias, const float* bn_mean,
                               const float* bn_var, float bn_eps, const float* w0, const float* b0, const float* w3,
                               const float* b3, float slope_head, float* out, int64_t* count, int F, int C, int O, int heads,
                               int lut_col, int32_t* status, const double* data, const double* freq, const int64_t* samples,
                               int64_t S, int P, int64_t L, int64_t Q, int conn_row, int osnr_row, int snr_row, int ber_row,
                               const double* cols, int ncol, double freq_threshold, const int64_t* conns, int64_t* conn,
                               int64_t* n, int max_lightpaths, int chunk, qot_stream_t stream);

/* ---- the place_impact entry with established lightpaths RELEASED in the same launch: who a reroute, or an admission
 * together with a tear-down, helps and whom it hurts (LightpathPredictor.reroute_impact) -- out[k] and
 * count[k] are the place_release entry's, bit for bit.  The affected lightpaths of candidate k are the SURVIVORS of its
 * sample (the lightpaths it does not release) that (a) interfere with the candidate or (b) interfere, in the unedited
 * sample, with a released lightpath; a released lightpath is never affected.  n_affected[k] (int64) is their number; the
 * first A = max_affected of them by rising first-seen number of the unedited sample get a slot i: affected[k, i] (int64 [K,
 * A]) is the lightpath's trunc(conn_id); before[k, i] (fp32 [K, A, O]) the lightpath "scored as the lightpath under test"
 * of the unedited sample, as the place_impact entry defines it -- the released lightpaths still send their messages;
 * after[k, i] the same in edited_k of the place_release entry with the candidate established (values[k] with osnr = snr =
 * ber = 0, is_lut 0): the messages of the lightpath's surviving interferers by rising first-seen number and, where the
 * candidate interferes with it, the candidate's row at the candidate's first-seen position among the survivors, behind
 * the lightpaths whose first channel l * Q + q lies below the smallest of its cells.  gains[k, i] (uint8 [K, A]) is 1
 * where the candidate is a source of after; lost[k, i] (int64 [K, A]) the released lightpaths that were sources of before,
 * a conn named twice counted once.  cols must not scale osnr, snr or ber (the caller's check).  Slots i >=
 * min(n_affected[k], A) hold affected -1, NaN rows, gains 0, lost -1; n_affected[k] > A is no error.  A refused candidate
 * (the place_release entry's status bits, no new one) has a NaN out row, count 0, n_affected 0 and every slot empty.  data
 * is never written.  One 256-thread workgroup per candidate: the place_impact entry's cost plus one more rescan of the
 * conn_id row for the released lightpaths' neighbourhoods.
 *
 * The argument list is the place_release entry's up to R, then affected, n_affected, before, after, gains, lost,
 * max_affected.  release == release_ptr == NULL with R == 0: no candidate releases anything.  Return codes before any
 * launch: the place entry's, QOT_ERR_BADARG for R < 0, for max_affected outside 1 .. QOT_PLACE_MAX_AFFECTED or -- when K > 0
 * -- a NULL release or release_ptr with R > 0, or a NULL affected, n_affected, before, after, gains or lost.  K == 0:
 * QOT_OK, no launch.  Nothing read from data, values or release is used as an index: conns are only compared. */
int qot_lightpath_infer_reroute_impact(const float* x, const int64_t* edge_index, const int64_t* batch,
                                       const int64_t* node_ptr, const int64_t* edge_ptr, const int64_t* lut_idx, int64_t n_lut,
                                       int64_t N, int64_t E, int64_t K, const float* w, const float* att_src,
                                       const float* att_dst, const float* conv_bias, float slope_att, const float* bn_weight,
                                       const float* bn_bias, const float* bn_mean, const float* bn_var, float bn_eps,
                                       const float* w0, const float* b0, const float* w3, const float* b3, float slope_head,
                                       float* out, int64_t* count, int F, int C, int O, int heads, int lut_col, int32_t* status,
                                       const double* data, const double* freq, const int64_t* samples, int64_t S, int P,
                                       int64_t L, int64_t Q, int conn_row, int osnr_row, int snr_row, int ber_row,
                                       const double* cols, int ncol, double freq_threshold, const double* values,
                                       const int64_t* cells, const int64_t* cell_ptr, int64_t M, const int64_t* release,
                                       const int64_t* release_ptr, int64_t R, int64_t* affected, int64_t* n_affected,
                                       float* before, float* after, uint8_t* gains, int64_t* lost, int max_affected,
                                       qot_stream_t stream);

/* ---- the place entry for every start slot of R routes in one launch: given a route, which frequency slot?
 * (LightpathPredictor.place_slots) -- Route r is the links links[link_ptr[r] : link_ptr[r + 1]] (links [M]
 * int64 link indices, link_ptr [R + 1] int64; a slice must be non-empty, a duplicate link is allowed, no cap on its length)
 * in sample samples[r] (required) with the raw lp_feat vector values[r] (fp64 [R, P]).  The candidate that starts at slot q
 * occupies the slots q .. q + width - 1 on every link of the route.  free[r, q] (uint8 [R, Q]) is 1 when every one of those
 * channels is free (all P values 0) and q + width <= Q; out[r, q] (fp32 [R, Q, O]) is then, bit for bit, the place entry's
 * row for that candidate -- cells route x {q .. q + width - 1} in any order, values[r] with, when slot_row >= 0, freq[q] in
 * the lp_feat row slot_row (slot_row -1: values[r] unchanged at every slot) -- and a NaN row otherwise.  An occupied slot
 * is an answer: it sets no status bit.  count[r] (int64 [R]) is the place entry's count, the flagged lightpaths of the
 * sample plus one, the same at every slot.  data is never written.  R * ceil(Q / chunk) 256-thread workgroups; a workgroup
 * discovers its sample once, marks the neighbourhoods of its chunk start slots with four waves and computes their rows one
 * after the other in one wave, so no result depends on chunk; O(L Q + chunk * route * width * Q) per workgroup; no
 * workspace.
 *
 * The argument list is the place entry's up to values (R takes K's place; the envelope is asked for R * Q rows), then links,
 * link_ptr, M, slot_row, width, chunk, free.  Return codes before any launch: the status entry's, QOT_ERR_UNSUPPORTED for
 * R * Q >= 2^31 or R * ceil(Q / chunk) >= 2^31, QOT_ERR_BADARG for M < 0, slot_row outside -1 .. P - 1, width outside 1 ..
 * QOT_LP_PLACE_SLOTS_MAX_WIDTH, chunk outside 1 .. QOT_LP_PLACE_SLOTS_MAX_CHUNK or -- when R > 0 -- a NULL samples, values,
 * link_ptr or free, or NULL links with M > 0.  R == 0: QOT_OK, no launch.
 * status, per route since nothing is read back -- all Q rows of the route NaN, its free 0, its count 0, the other routes
 * untouched -- with the place entry's bits: QOT_LP_STATUS_BAD_SAMPLE; QOT_LP_PLACE_BAD_CELL for a link_ptr slice that is
 * empty, descending or beyond M or a link index outside [0, L); QOT_LP_STATUS_BAD_CONN; QOT_LP_PLACE_NOT_LUT;
 * QOT_LP_PLACE_CONN_TAKEN; QOT_LP_STATUS_TOO_MANY.  QOT_LP_PLACE_OCCUPIED is never set.  Nothing read from data or values
 * is used as an index; a link index is range-checked before it is. */
#define QOT_LP_PLACE_SLOTS_MAX_CHUNK 32     /* start slots one workgroup runs one after the other (their byte maps: 32 x 256 B of LDS) */
#define QOT_LP_PLACE_SLOTS_MAX_WIDTH 8      /* slots a candidate occupies on every link of its route */
int qot_lightpath_infer_place_slots(const float* x, const int64_t* edge_index, const int64_t* batch, const int64_t* node_ptr,
                                    const int64_t* edge_ptr, const int64_t* lut_idx, int64_t n_lut, int64_t N, int64_t E,
                                    int64_t R, const float* w, const float* att_src, const float* att_dst,
                                    const float* conv_bias, float slope_att, const float* bn_weight, const float* bn_bias,
                                    const float* bn_mean, const float* bn_var, float bn_eps, const float* w0, const float* b0,
                                    const float* w3, const float* b3, float slope_head, float* out, int64_t* count, int F,
                                    int C, int O, int heads, int lut_col, int32_t* status, const double* data,
                                    const double* freq, const int64_t* samples, int64_t S, int P, int64_t L, int64_t Q,
                                    int conn_row, int osnr_row, int snr_row, int ber_row, const double* cols, int ncol,
                                    double freq_threshold, const double* values, const int64_t* links,
                                    const int64_t* link_ptr, int64_t M, int slot_row, int width, int chunk, uint8_t* free,
                                    qot_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* QOT_GNN_H */
