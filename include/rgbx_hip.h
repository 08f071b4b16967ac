/*
 * rgbx_hip.h — C ABI of librgbx_hip.so, the MI355X (gfx950) native library behind the
 * message-passing hot path of rgb-experiment.
 *
 * What each entry point replaces in the reference (paths relative to the reference repo root;
 * "[PyG]" = the arithmetic lives in the un-vendored torch_geometric dependency the reference
 * imports at that line):
 *
 *   rgbx_csr_*            self-loop rewrite + grouping of edges by aggregation index that
 *                         MessagePassing.propagate performs implicitly on every call
 *                         (models/gcn.py:27,29; models/graphsage.py:53-58; models/gat.py:28,30;
 *                         models/appnp_stack.py:29), restated in-repo by models/dagnn.py:20-24.
 *   rgbx_gcn_norm_f32     gcn_norm, models/dagnn.py:12-31 (degree over the target index,
 *                         deg^-1/2 with inf -> 0, w = dis[src] * dis[tgt]).
 *   rgbx_loop_weights_f32 / rgbx_edge_slot_weights_f32 / rgbx_weighted_deg_inv_sqrt_f32 / rgbx_gcn_norm_weighted_f32 /
 *   rgbx_edge_dot_f32 / rgbx_gcn_norm_bwd_f32
 *                         the same gcn_norm with its edge_weight argument given (models/dagnn.py:12-31), and its
 *                         gradient in the weights.
 *   rgbx_inv_degree_f32   the 1/max(count,1) of aggr='mean' (models/graphsage.py:39,58) [PyG].
 *   rgbx_spmm_csr_f32     MessagePassing.propagate with aggr='add' / 'mean' and message
 *                         norm * x_j (models/dagnn.py:34-36,46,57-59; models/graphsage.py:58).
 *   rgbx_spmm_csr_bf16 / rgbx_rows_f32_to_bf16
 *                         the same propagate with the gathered matrix stored as bfloat16 (fp32 sums), and the
 *                         rounding in front of it (tensor.to(torch.bfloat16)).
 *   rgbx_spmm_csr_extremum_f32 / rgbx_extremum_bwd_f32
 *                         the same propagate with aggr='max' / 'min' (the keyword models/graphsage.py:38-40 leaves to
 *                         the caller) and its backward.
 *   rgbx_appnp_f32        APPNP.forward's K-step recurrence (models/appnp_stack.py:29),
 *                         restated in-repo by models/pta.py:79-84.
 *   rgbx_dagnn_gate_*     Prop.forward's sigmoid-gated mix of the K+1 hops (models/dagnn.py:49-55) and its backward.
 *   rgbx_gat_*            GATConv.forward/message + segment softmax (models/gat.py:28,30) [PyG].
 *   rgbx_supergat_*       SuperGATConv ('MX' attention, attention loss, negative sampling; models/supergat.py) [PyG].
 *   rgbx_gatv2_*          GATv2Conv (dynamic attention) [PyG]; not in the reference's zoo, shaped like models/gat.py.
 *   rgbx_transformer_*    TransformerConv (scaled dot-product attention) [PyG]; not in the reference's zoo.
 *   rgbx_resgated_*       ResGatedGraphConv (per-channel sigmoid gate) [PyG]; not in the reference's zoo.
 *   rgbx_gine_*           GINEConv (GIN with a feature row per edge: relu(x_j + e_ji) summed) [PyG]; the zoo's
 *                         models/gin.py is its sibling without edge features.
 *   rgbx_cgconv_*         CGConv (gated softplus message over [x_i, x_j, e_ij]) [PyG]; not in the reference's zoo.
 *   rgbx_pna_*            PNAConv (statistics of a per-edge message, scaled by functions of the in-degree) [PyG]; not in
 *                         the reference's zoo.
 *   rgbx_rgcn_*           RGCNConv (a relation per edge: mean per (target, relation), basis decomposition) [PyG]; not
 *                         in the reference's zoo.
 *   rgbx_softmax_aggr_*   SoftmaxAggregation / GENConv(aggr="softmax") (per-channel softmax at a trained temperature)
 *                         [PyG]; not in the reference's zoo.
 *   rgbx_gemm_tn_f32      dW = dY^T X of the nn.Linear / conv.lin layers under loss.backward()
 *                         (itexperiments.py:439; layers at models/gcn.py:18-21, appnp_stack.py:19-20).
 *   rgbx_bn_* / rgbx_affine_cols_f32
 *                         nn.BatchNorm1d over all N nodes between conv layers (models/gcn.py:23,28;
 *                         graphsage.py:24,29; gat.py:23,29; appnp_stack.py:21,27), forward and backward.
 *   rgbx_masked_nll_*     nn.NLLLoss on out[mask] and the arg-max accuracy (itexperiments.py:400,
 *                         429,434,624-626,643).
 *   rgbx_coalesce_* / rgbx_split_edge_keys_i64
 *                         the one-shot edge-list edits in front of the path: torch_sparse.coalesce
 *                         (rd2pd.py:92-93) and torch_geometric.utils.to_undirected (itexperiments.py:235-238) [PyG].
 *   rgbx_gather_rows_f32 / rgbx_scatter_add_rows_f32
 *                         halo pack / unpack for the 1-D node partition (new capability; the
 *                         reference is single-device, itexperiments.py:246).
 *   rgbx_sample_*         fan-out neighbour sampling (GraphSAGE's mini-batches; new capability: the reference trains on
 *                         the whole graph in every step, itexperiments.py:417-440).
 *
 * Conventions
 *   - Plain C types only. Every pointer except `rgbx_last_error_string`'s result is a DEVICE
 *     pointer owned by the caller; the library never allocates or frees device memory.
 *   - Every call is asynchronous on `stream` (a hipStream_t passed as void*; NULL = the null
 *     stream); nothing inside synchronises the device.
 *   - Return value: 0 = OK; < 0 = argument/shape/alignment error (RGBX_E_*); > 0 = hipError_t.
 *     `rgbx_last_error_string()` describes the calling thread's last failure.
 *   - Feature matrices are fp32 row-major with an explicit leading dimension in ELEMENTS (the one exception: the
 *     bfloat16 table of rgbx_spmm_csr_bf16, passed as uint16_t).
 *   - Indices inside the library are int32 (requires N < 2^31 and E' < 2^31); `edge_index`
 *     arrives as the reference's int64 [2, E].
 */
#ifndef RGBX_HIP_H
#define RGBX_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define RGBX_VERSION 501 /* major*10000 + minor*100 + patch */

#define RGBX_OK 0
#define RGBX_E_ARG (-1)    /* null pointer / negative size / bad enum */
#define RGBX_E_RANGE (-2)  /* N or E' does not fit int32 */
#define RGBX_E_ALIGN (-3)  /* pointer or leading dimension not aligned for the vector path */
#define RGBX_E_WS (-4)     /* workspace too small */
#define RGBX_E_SHAPE (-5)  /* unsupported shape (e.g. heads*channels combination) */

typedef void* rgbx_stream_t;

/* Self-loop rewrite applied while grouping edges (what the conv layers do before propagate). */
enum {
  RGBX_LOOPS_KEEP = 0,          /* edges as given (SAGEConv [PyG], models/graphsage2.py:20-23) */
  RGBX_LOOPS_ADD_REMAINING = 1, /* add_remaining_self_loops, fill 1 (models/dagnn.py:20-24) */
  RGBX_LOOPS_REMOVE_ADD = 2     /* remove_self_loops + add_self_loops (models/graphsage.py:53-56) */
};
/* For unweighted graphs modes 1 and 2 give the same edge list: the non-loop edges in their
 * original order followed by one self-loop per node, nodes ascending. */

int rgbx_version(void);
const char* rgbx_last_error_string(void);

/* ---- graph preparation: int64 edge list -> CSR grouped by `agg_row` ------------------------ */

/* Bytes of scratch `rgbx_csr_build` needs for E input edges over N nodes. */
int rgbx_csr_workspace_bytes(int64_t E, int64_t N, size_t* bytes);

/* Group edges by aggregation index with a STABLE sort.
 *   agg_row[e]   = index the edge aggregates INTO  (edge_index[1] forward, edge_index[0] for the
 *                  transposed graph used by backward)
 *   other_row[e] = index the edge gathers FROM
 * Outputs (capacity E + N entries each for col / perm; rowptr has N + 1):
 *   rowptr[i]..rowptr[i+1]  edges aggregating into node i; rowptr[N] = E'
 *   col[p]                  gather index of CSR slot p
 *   perm[p]                 id of the edge in slot p: e in [0,E) = column of edge_index,
 *                           E + i = the added self-loop of node i
 * Within a row, slots keep the order of the rewritten edge list (original edges first, in
 * input order; the added self-loop last). */
int rgbx_csr_build(const int64_t* agg_row, const int64_t* other_row, int64_t E, int64_t N,
                   int loops_mode, int32_t* rowptr, int32_t* col, int32_t* perm, void* workspace,
                   size_t workspace_bytes, rgbx_stream_t stream);

/* dis[i] = (rowptr[i+1]-rowptr[i])^-1/2, 0 where the count is 0 (models/dagnn.py:27-30). */
int rgbx_deg_inv_sqrt_f32(const int32_t* rowptr, int64_t N, float* dis, rgbx_stream_t stream);

/* w[p] = dis[col[p]] * dis[i] for every slot p of row i (models/dagnn.py:31). `dis` must come
 * from the FORWARD (target-grouped) CSR also when (rowptr, col) is the transposed one. */
int rgbx_gcn_norm_f32(const int32_t* rowptr, const int32_t* col, int64_t N, const float* dis,
                      float* w, rgbx_stream_t stream);

/* inv[i] = 1 / max(rowptr[i+1]-rowptr[i], 1) — the divisor of aggr='mean'. */
int rgbx_inv_degree_f32(const int32_t* rowptr, int64_t N, float* inv, rgbx_stream_t stream);

/* ---- weighted graphs: gcn_norm(edge_index, edge_weight, ...) of models/dagnn.py:12-31 with the weight present ------- */

/* Weight of the self-loop every node gets from the rewrite (models/dagnn.py:20-24 -> add_remaining_self_loops, fill 1):
 *   RGBX_LOOPS_ADD_REMAINING: loop_w[i] = ew[e] of node i's input self-loop e, `fill` if it has none; of several input
 *     self-loops the one with the HIGHEST edge id supplies the weight (an integer atomic max over edge ids, then a read: the
 *     same answer in every run). loop_src[i] = that edge id, -1 where the loop was filled in.
 *   RGBX_LOOPS_REMOVE_ADD: loop_w[i] = fill, loop_src[i] = -1 for every node.
 * src / dst = edge_index[0] / edge_index[1] (int64 [E]); loop_w f32 [N], loop_src int32 [N].
 * RGBX_LOOPS_KEEP adds no loops: RGBX_E_ARG. */
int rgbx_loop_weights_f32(const int64_t* src, const int64_t* dst, const float* ew, int64_t E, int64_t N, int loops_mode,
                          float fill, float* loop_w, int32_t* loop_src, rgbx_stream_t stream);

/* ew_slot[p] = perm[p] < E ? ew[perm[p]] : loop_w[perm[p] - E] for the nnz slots of a CSR from rgbx_csr_build (forward
 * or transposed; loop_w may be NULL when nnz <= E, i.e. RGBX_LOOPS_KEEP). */
int rgbx_edge_slot_weights_f32(const int32_t* perm, int64_t nnz, const float* ew, int64_t E, const float* loop_w,
                               float* ew_slot, rgbx_stream_t stream);

/* deg[i] = sum of ew_slot over row i of the FORWARD CSR (rows of any length; fixed summation order: bitwise reproducible),
 * dis[i] = deg[i]^-1/2 with inf -> 0 (models/dagnn.py:25-30). Not clamped: deg = 0 gives 0, a negative sum gives NaN. */
int rgbx_weighted_deg_inv_sqrt_f32(const int32_t* rowptr, const float* ew_slot, int64_t N, float* dis,
                                   rgbx_stream_t stream);

/* w[p] = dis[col[p]] * ew_slot[p] * dis[i] for every slot p of row i (models/dagnn.py:31); either CSR with its own
 * ew_slot, `dis` from the forward one. Unit weights give rgbx_gcn_norm_f32's bits. */
int rgbx_gcn_norm_weighted_f32(const int32_t* rowptr, const int32_t* col, const float* ew_slot, int64_t N,
                               const float* dis, float* w, rgbx_stream_t stream);

/* Backward of the weighted normalisation (models/dagnn.py:12-31 differentiated in edge_weight). g = dL/dw per FORWARD
 * slot, ew_slot the forward slot weights, dis from rgbx_weighted_deg_inv_sqrt_f32. With w_p = dis[j] ew_p dis[i]:
 *   dL/dew_p = g_p dis[j] dis[i] + ddeg[i],  ddeg[k] = -1/2 deg[k]^-3/2 ddis[k],
 *   ddis[k]  = sum_{p: tgt = k} g_p ew_p dis[src] + sum_{p: src = k} g_p ew_p dis[tgt]
 * (first sum over forward row k, second over transposed row k through t2f[q] = forward slot of transposed slot q; both
 * row-wise in a fixed order, no float atomics). dew [E] receives dL/dew of every input edge: a slot's gradient goes to
 * edge perm[p]; that of an added loop E + i goes to loop_src[i] (the input self-loop that supplied its weight), nowhere
 * when loop_src[i] < 0 or loop_src == NULL; input self-loops that the rewrite dropped get 0. ddeg: f32 [N] scratch. */
int rgbx_gcn_norm_bwd_f32(const int32_t* rowptr, const int32_t* col, const int32_t* perm, const int32_t* rowptr_t,
                          const int32_t* col_t, const int32_t* t2f, const int32_t* loop_src, const float* g,
                          const float* ew_slot, const float* dis, int64_t N, int64_t E, float* ddeg, float* dew,
                          rgbx_stream_t stream);

/* ---- aggregation ------------------------------------------------------------------------- */

/* Optional plan for rows with very many slots (hub nodes). Rows with more than `threshold` slots are
 * skipped by the row-per-wave kernel; each is cut into consecutive chunks (chunk c covers slots
 * [chunk_begin[c], chunk_end[c]) of the CSR), one wave sums one chunk into partial[c, :], and the
 * partials of long row r (chunks long_chunk_ptr[r] .. long_chunk_ptr[r+1]) are added in chunk order
 * before the epilogue — bitwise reproducible, no atomics. All arrays are device memory owned by the
 * caller; `partial` is an [n_chunks, d] fp32 scratch. NULL (or threshold 0) = no splitting. */
typedef struct rgbx_row_split {
  int32_t threshold;
  int32_t n_chunks;
  int32_t n_long;
  const int32_t* chunk_begin;    /* [n_chunks] */
  const int32_t* chunk_end;      /* [n_chunks] */
  const int32_t* chunk_row;      /* [n_chunks] row id of every chunk (used by the GAT kernels) */
  const int32_t* long_row;       /* [n_long] row ids, ascending */
  const int32_t* long_chunk_ptr; /* [n_long + 1] */
  float* partial;                /* [n_chunks, d] fp32 scratch; GAT: [n_chunks, H*C + 2*H] */
} rgbx_row_split_t;

/* out[i,:] = a * rs[i] * sum_{p in row i} w[p] * x[col[p],:]  +  b * y[i,:]  +  bias[:]
 *   w  == NULL -> every weight is 1;  rs == NULL -> every row scale is 1;
 *   y  == NULL -> no additive term (b ignored);  bias == NULL -> no per-column term (the conv
 *   layer's `out += bias`, fused into the store).  `out` may alias `y` but not `x`.
 * N rows, d columns; x has n_src rows (col[] < n_src is the caller's contract). */
int rgbx_spmm_csr_f32(const int32_t* rowptr, const int32_t* col, const float* w, const float* rs,
                      const float* x, int64_t ldx, const float* y, int64_t ldy, const float* bias,
                      float* out, int64_t ldo, int64_t N, int64_t d, float a, float b,
                      const rgbx_row_split_t* split, rgbx_stream_t stream);

/* ---- the same gather with the gathered table stored as bfloat16 ------------------------------------------------------
 * bfloat16 values are passed as uint16_t: the upper 16 bits of the fp32 pattern (widening is `bits << 16`, exact). */

/* 1 if rgbx_spmm_csr_bf16 takes width d: d % 8 == 0 and 8 <= d <= 256 (a lane holds 8 columns = one 16-byte load and a
 * lane group a whole row); other widths: zero-pad the rows. */
int rgbx_spmm_csr_bf16_supported(int64_t d);

/* rgbx_spmm_csr_f32 with x stored as bfloat16 (replaces the same propagate, models/dagnn.py:57-59 / graphsage.py:58, at
 * half the bytes of the gathered table): the same expression, x widened exactly, every sum and the whole epilogue in
 * fp32; w, rs, y, bias are fp32 and optional as there. Outputs: `out` (fp32) and / or `out_bf16` (the same fp32 result
 * rounded to nearest-even; NaN -> the quiet NaN 0xffff, overflow -> inf) — at least one (RGBX_E_ARG). `out` may alias
 * `y`; out_bf16 must not alias x. Leading dimensions may exceed d (column slices).
 * Constraints, checked on the host before any launch: rgbx_spmm_csr_bf16_supported(d) (RGBX_E_SHAPE); x and out_bf16
 * 16-byte aligned with ldx % 8 == 0, ldob % 8 == 0; y / out / bias 16-byte aligned with ldy % 4 == 0, ldo % 4 == 0
 * (RGBX_E_ALIGN); null rowptr / col / x, a leading dimension < d, an incomplete plan (RGBX_E_ARG).
 * `split`: as rgbx_spmm_csr_f32 — rows above the threshold are cut into the plan's chunks, the partials are fp32 in
 * split->partial ([n_chunks, d], 16-byte aligned) and added in chunk order. No float atomics, no scratch memory: two
 * launches give the same bits. The backward pass is this entry on the transposed CSR. */
int rgbx_spmm_csr_bf16(const int32_t* rowptr, const int32_t* col, const float* w, const float* rs, const uint16_t* x,
                       int64_t ldx, const float* y, int64_t ldy, const float* bias, float* out, int64_t ldo,
                       uint16_t* out_bf16, int64_t ldob, int64_t N, int64_t d, float a, float b,
                       const rgbx_row_split_t* split, rgbx_stream_t stream);

/* dst[r, 0:d] = src[r, 0:d] rounded to bfloat16, nearest-even, for r in [0, n): the conversion in front of
 * rgbx_spmm_csr_bf16 (replaces tensor.to(torch.bfloat16), whose CPU result it matches bit for bit: NaN -> 0xffff, the
 * largest finite fp32 -> inf, subnormals rounded like any value). Strided source and destination (lds, ldd >= d), so a
 * column slice needs no contiguous copy; any d (rows on the 16-byte grid with d % 8 == 0, lds % 4 == 0, ldd % 8 == 0 take
 * the vector path). n == 0 or d == 0: nothing to do, returns 0. */
int rgbx_rows_f32_to_bf16(const float* src, int64_t lds, uint16_t* dst, int64_t ldd, int64_t n, int64_t d,
                          rgbx_stream_t stream);

/* g[p] = sum_c a[i,c] * b[col[p],c] for every slot p of row i: dL/dw of the aggregation out = sum_p w[p] x[col[p],:]
 * (message norm * x_j, models/dagnn.py:57-59, norm from models/dagnn.py:12-31) with a = dL/dout and b = x. One wave per
 * row, the gather's lane layout; every g[p] is written once with plain stores. d % 4 == 0, 4 <= d <= 256
 * (rgbx_edge_dot_supported; other widths: zero-pad, or cut into column blocks and add); a, b 16-byte aligned with leading
 * dimensions % 4 == 0. `split`: rows above split->threshold are cut into the plan's chunks, one wave each (needs
 * chunk_begin / chunk_end / chunk_row; `partial` is not used). */
int rgbx_edge_dot_supported(int64_t d);
int rgbx_edge_dot_f32(const int32_t* rowptr, const int32_t* col, const float* a, int64_t lda, const float* b, int64_t ldb,
                      float* g, int64_t N, int64_t d, const rgbx_row_split_t* split, rgbx_stream_t stream);

/* Max / min neighbourhood aggregation: MessagePassing.propagate with aggr='max' | 'min', the choice my_SAGEConv leaves to
 * its caller (models/graphsage.py:38-40: kwargs.setdefault('aggr', 'mean'); message x_j at :58) and SAGEConv(aggr=...)
 * takes as well (models/graphsage2.py:20-23) [PyG].
 *   out[i,c] = max (min) over the slots p of row i of x[col[p], c];   arg[i,c] = the slot p that supplied it
 * A row without slots gets out = 0 and arg = -1 (PyG: nodes without in-edges aggregate 0). Ties: the LOWEST slot wins
 * (strict > / < while walking the slots in order — torch_scatter's CPU scatter_max in edge order, the CSR build being a
 * stable sort). INPUTS ARE FINITE: there is no NaN policy (a NaN never wins a strict comparison; an infinity of the losing
 * sign in every slot leaves arg = -1). An extremum involves no rounding: values and arg are exact and the same in every run.
 * arg: int32 [N, d] (leading dimension d), or NULL = the inference form, which stores nothing extra. d % 4 == 0,
 * 4 <= d <= 256 (rgbx_spmm_csr_extremum_supported; other widths: pad, or cut into column blocks); x, out, arg 16-byte
 * aligned, leading dimensions % 4 == 0. `split`: rows above split->threshold are cut into the plan's chunks, one wave each,
 * and the chunk results are merged in chunk order under the same strict comparison — the split changes neither values nor
 * arg. split->partial must then hold 2 * n_chunks * d 4-byte words (chunk values, then chunk slots), 16-byte aligned. */
enum { RGBX_EXTREMUM_MAX = 0, RGBX_EXTREMUM_MIN = 1 };
int rgbx_spmm_csr_extremum_supported(int64_t d);
int rgbx_spmm_csr_extremum_f32(const int32_t* rowptr, const int32_t* col, const float* x, int64_t ldx, float* out,
                               int64_t ldo, int32_t* arg, int64_t N, int64_t d, int mode, const rgbx_row_split_t* split,
                               rgbx_stream_t stream);

/* Source-side backward of rgbx_spmm_csr_extremum_f32 over the TRANSPOSED CSR (rows = sources, col_t = targets) with
 * t2f[q] = the forward slot of transposed slot q:
 *   gx[j,c] = sum over the slots q of transposed row j, i = col_t[q], of gout[i,c] * [arg[i,c] == t2f[q]]
 * Matching the slot, not the source id, keeps duplicate edges j -> i from counting twice. Row-wise sums in a fixed order,
 * no float atomics: bitwise reproducible. N = rows of the transposed CSR (gx [N, ldgx]); gout / arg are indexed by col_t.
 * Widths and alignment as the forward; `split` (of the transposed CSR): partial [n_chunks, d], added in chunk order. */
int rgbx_extremum_bwd_f32(const int32_t* rowptr_t, const int32_t* col_t, const int32_t* t2f, const float* gout, int64_t ldg,
                          const int32_t* arg, float* gx, int64_t ldgx, int64_t N, int64_t d, const rgbx_row_split_t* split,
                          rgbx_stream_t stream);

/* ---- one-pass multi-aggregation: sum / mean / var / std / max / min of a neighbourhood from ONE gather ----------------
 * MessagePassing.propagate with aggr='std' | 'var' or a LIST of aggregators (PyG's MultiAggregation, mode='cat': the PNA
 * recipe) behind SAGEConv(aggr=...) (models/graphsage2.py:20-23 passes the keyword on) [PyG]. Every neighbour row is read
 * once; each statistic goes straight to its own matrix (pointer + leading dimension), so the column blocks of ONE
 * [N, k*d] tensor can be passed and the concatenation costs nothing. For target row i with n slots p, v_p = x[col[p], c]:
 *   sum  = sum_p v_p                      mean = sum / max(n, 1)
 *   var  = mean(v^2) - mean(v)^2          (biased, NOT clamped; PyG VarAggregation)
 *   std  = sqrt(var) where var > 1e-5, else 0   (PyG StdAggregation: sqrt(max(var, 1e-5)), 0 where that is <= sqrt(1e-5))
 *   max / min, argmax / argmin            exactly rgbx_spmm_csr_extremum_f32's values and arg (lowest slot wins on ties)
 * A row without slots gets 0 in every statistic and arg = -1. INPUTS ARE FINITE. A NULL pointer means "not wanted": that
 * statistic is neither computed nor stored; argmax / argmin NULL with max / min set is the inference form. An arg without
 * its extremum, or no statistic at all: RGBX_E_ARG.
 * The second moment is accumulated as deviations from a per-(row, column) shift (the first slot's value) and merged across
 * lane groups and hub-row chunks by exact re-basing in a fixed order (Chan's update on shifted sums): offset features keep
 * their variance, and a neighbourhood whose values are all equal gives var == 0 and std == 0 EXACTLY. No float atomics:
 * bitwise reproducible.
 * d % 4 == 0, 4 <= d <= 256 (rgbx_spmm_csr_multi_supported; other widths: pad, or cut into column blocks); x and every
 * output 16-byte aligned with leading dimensions % 4 == 0 and >= d; no output may alias x. `split`: rows above
 * split->threshold are cut into the plan's chunks, one wave each, merged in chunk order (the split changes no extremum or
 * arg); split->partial must hold rgbx_spmm_csr_multi_partial_words(n_chunks, d, which) 4-byte words, 16-byte aligned,
 * `which` = the OR of the RGBX_MULTI_* bits of the wanted statistics. */
enum {
  RGBX_MULTI_SUM = 1, RGBX_MULTI_MEAN = 2, RGBX_MULTI_VAR = 4, RGBX_MULTI_STD = 8, RGBX_MULTI_MAX = 16, RGBX_MULTI_MIN = 32,
  RGBX_MULTI_ALL = 63
};
typedef struct rgbx_multi_out {
  float* sum;      int64_t ld_sum;
  float* mean;     int64_t ld_mean;
  float* var;      int64_t ld_var;
  float* std;      int64_t ld_std;
  float* max;      int64_t ld_max;
  int32_t* argmax; int64_t ld_argmax;
  float* min;      int64_t ld_min;
  int32_t* argmin; int64_t ld_argmin;
} rgbx_multi_out_t;
int rgbx_spmm_csr_multi_supported(int64_t d);
int rgbx_spmm_csr_multi_partial_words(int64_t n_chunks, int64_t d, int which, int64_t* words);
int rgbx_spmm_csr_multi_f32(const int32_t* rowptr, const int32_t* col, const float* x, int64_t ldx,
                            const rgbx_multi_out_t* out, int64_t N, int64_t d, const rgbx_row_split_t* split,
                            rgbx_stream_t stream);

/* Source-side backward of rgbx_spmm_csr_multi_f32 in ONE pass over the TRANSPOSED CSR (rows = sources, col_t = targets),
 * t2f[q] = the forward slot of transposed slot q (needed only with an extremum term). For source row j, slots q, i = col_t[q]:
 *   gx[j,c] = sum_q a[i,c] + x[j,c] * sum_q b[i,c] + sum_q gmax[i,c] [argmax[i,c] == t2f[q]] + sum_q gmin[i,c] [argmin[i,c] == t2f[q]]
 * a and b are per-TARGET rows the caller prepares (nothing in them is indexed by an edge):
 *   b = g_std / (n std) (0 where std == 0) + 2 g_var / n,      a = g_sum + g_mean / n - b * mean.
 * Any of the four terms may be NULL and is then neither read nor added (no term at all: RGBX_E_ARG); x is read only with b
 * (row j, once). Row-wise sums in slot order with a fixed butterfly over the lane groups, hub rows through chunk partials
 * added in chunk order, no float atomics: bitwise reproducible. Four rows in flight per lane group, two when a slot loads
 * more than three 16-byte fragments. Widths and alignment as the forward; gx must alias no input; `split` (of the
 * transposed CSR, with chunk_row): partial [n_chunks, d]. */
typedef struct rgbx_multi_grad {
  const float* a;        int64_t ld_a;
  const float* b;        int64_t ld_b;
  const float* x;        int64_t ld_x;
  const float* gmax;     int64_t ld_gmax;
  const int32_t* argmax; int64_t ld_argmax;
  const float* gmin;     int64_t ld_gmin;
  const int32_t* argmin; int64_t ld_argmin;
} rgbx_multi_grad_t;
int rgbx_multi_bwd_f32(const int32_t* rowptr_t, const int32_t* col_t, const int32_t* t2f, const rgbx_multi_grad_t* terms,
                       float* gx, int64_t ldgx, int64_t N, int64_t d, const rgbx_row_split_t* split, rgbx_stream_t stream);

/* ---- PNAConv: degree-scaled multi-aggregation of a per-edge message -----------------------------------------------------
 * PNAConv.message with pre_layers = 1, split by linearity into a target part a, a source part b and an edge part c, and
 * DegreeScalerAggregation behind it, in PyG's own column order (tower, then scaler, then aggregator) [PyG]; Corso et al.,
 * "Principal Neighbourhood Aggregation for Graph Nets". Not in the reference's zoo. For an edge j -> i in forward CSR
 * slot p (RGBX_LOOPS_KEEP: the edges as given, n = the slots of row i), b [N, d], c [nnz, d] ONE ROW PER SLOT in forward
 * slot order (NULL: u_p = b[j,:]), a [N, d] (NULL: no shift), d = T * F:
 *   u_p    = b[j,:] + c[p,:]                                              (one fp32 add)
 *   stat_k = sum | mean | var | std | max | min of u_p over the slots of i  (rgbx_spmm_csr_multi_f32's definitions, word
 *            for word: biased var from shifted sums, std = sqrt(var) where var > 1e-5 else 0, the lowest slot wins a tie,
 *            a row without slots gives 0 and arg = -1; with c == NULL that entry point's bits)
 *   shift  : mean, max, min += a[i,:];  sum += n * a[i,:];  var, std unchanged;  a row without slots stays 0
 *   scale_s: RGBX_PNA_IDENTITY 1 | _AMPLIFICATION log(D+1)/avg_log | _ATTENUATION avg_log/log(D+1) | _LINEAR D/avg_lin |
 *            _INVERSE_LINEAR avg_lin/D,   D = max(n, 1)
 *   out[i, t*S*A*F + (s*A + k)*F + f] = scale_s(i) * stat_k[i, t*F + f]
 * `avg_deg` = two floats [avg_lin, avg_log] in DEVICE memory, read by the kernel (a captured launch needs no read-back;
 * averages of 0 give inf / NaN in the scaled blocks of rows WITH slots, as in PyG; rows without slots are exact zeros).
 * `which`: the OR of the RGBX_MULTI_* bits of the A aggregators; `aggr_order`: their A bits in output order k (HOST
 * memory, read before the call returns; NULL = ascending bits); `scalers`: the S scale kinds in output order
 * (HOST memory, 1 <= S <= 8). F = the tower width: F % 4 == 0 and F divides d, so a lane's four columns stay in one tower.
 * rgbx_pna_out_t: out [N, T*S*A*F]; the others are what a backward needs and the scaled blocks do not hold, each [N, d]
 * of u BEFORE the shift, NULL = not wanted: mean (with any of sum, mean, var, std), var / std (with var or std),
 * argmax / argmin (with that extremum; otherwise RGBX_E_ARG).
 * d % 4 == 0, 4 <= d <= 256 (rgbx_pna_supported; wider: cut at tower boundaries); a, b, c and every output 16-byte
 * aligned with leading dimensions % 4 == 0 and >= their width; out aliases no input. `split`: rows above
 * split->threshold are cut into the plan's chunks, one wave each, their records merged in chunk order by the same exact
 * re-basing (the split changes no extremum or arg); split->partial holds `partial_words` 4-byte words, at least
 * rgbx_pna_partial_words(n_chunks, d, which [| RGBX_MULTI_MEAN when the raw mean is kept]) (else RGBX_E_WS), 16-byte
 * aligned. No float atomics: bitwise reproducible. */
enum {
  RGBX_PNA_IDENTITY = 0, RGBX_PNA_AMPLIFICATION = 1, RGBX_PNA_ATTENUATION = 2, RGBX_PNA_LINEAR = 3,
  RGBX_PNA_INVERSE_LINEAR = 4
};
typedef struct rgbx_pna_out {
  float* out;      int64_t ld_out;
  float* mean;     int64_t ld_mean;
  float* var;      int64_t ld_var;
  float* std;      int64_t ld_std;
  int32_t* argmax; int64_t ld_argmax;
  int32_t* argmin; int64_t ld_argmin;
} rgbx_pna_out_t;
int rgbx_pna_supported(int64_t d, int64_t F);
int rgbx_pna_partial_words(int64_t n_chunks, int64_t d, int which, int64_t* words);
int rgbx_pna_fwd_f32(const int32_t* rowptr, const int32_t* col, const float* a, int64_t lda, const float* b, int64_t ldb,
                     const float* c, int64_t ldc, const float* avg_deg, int which, const int32_t* aggr_order,
                     const int32_t* scalers, int n_scalers, const rgbx_pna_out_t* out, int64_t N, int64_t d, int64_t F,
                     const rgbx_row_split_t* split, int64_t partial_words, rgbx_stream_t stream);

/* Backward of rgbx_pna_fwd_f32 in b and c. A, B, gmax, gmin are per-TARGET rows [N, d] the caller prepares (nothing in
 * them is indexed by an edge), with G_k = sum_s scale_s * g_out[(s, k)]:
 *   B = G_std / (n std) (0 where std == 0) + 2 G_var / n,     A = G_sum + G_mean / n - B * mean_u,    gmax / gmin = G_max / G_min
 *   bracket(i, p) = A[i,:] + B[i,:] * u_p + gmax[i,:] [argmax[i,:] == p] + gmin[i,:] [argmin[i,:] == p]
 * with u_p recomputed from the forward's own add. Any term may be NULL and is then neither read nor added (none at all,
 * or an extremum cotangent without its arg: RGBX_E_ARG). The gradient in a needs no kernel (the second-moment terms sum
 * to zero over a row): g_a[i] = n G_sum + (G_mean + G_max + G_min) [n > 0].
 *   rgbx_pna_bwd_src_f32, over the TRANSPOSED CSR (rows = sources j, col_t = targets, t2f [nnz] = the forward slot of
 *     every transposed slot; needed with an extremum term, or with B and c):
 *       g_b[j,:] = sum over the slots q of transposed row j of bracket(col_t[q], t2f[q])
 *     b[j] is read once per row, c[t2f[q]] gathered (c may be NULL; both are read only with B). Row-wise sums in slot order
 *     with a fixed butterfly over the lane groups, hub rows through split->partial [n_chunks, d] added in chunk order.
 *   rgbx_pna_bwd_edge_f32, over the forward CSR: g_c[p,:] = bracket(i, p), one row per slot in forward slot order, every
 *     slot row written; b and c are required with B. `split` only balances the hub rows (chunk_begin / chunk_end /
 *     chunk_row; split->partial is not touched).
 * Widths and alignment as the forward (any d % 4 == 0 up to 256: the towers play no part). No float atomics. */
typedef struct rgbx_pna_grad {
  const float* A;        int64_t ld_A;
  const float* B;        int64_t ld_B;
  const float* gmax;     int64_t ld_gmax;
  const int32_t* argmax; int64_t ld_argmax;
  const float* gmin;     int64_t ld_gmin;
  const int32_t* argmin; int64_t ld_argmin;
} rgbx_pna_grad_t;
int rgbx_pna_bwd_src_f32(const int32_t* rowptr_t, const int32_t* col_t, const int32_t* t2f, const float* b, int64_t ldb,
                         const float* c, int64_t ldc, const rgbx_pna_grad_t* terms, float* g_b, int64_t ldgb, int64_t N,
                         int64_t d, const rgbx_row_split_t* split, rgbx_stream_t stream);
int rgbx_pna_bwd_edge_f32(const int32_t* rowptr, const int32_t* col, const float* b, int64_t ldb, const float* c,
                          int64_t ldc, const rgbx_pna_grad_t* terms, float* g_c, int64_t ldgc, int64_t N, int64_t d,
                          const rgbx_row_split_t* split, rgbx_stream_t stream);

/* rgbx_spmm_csr_f32 with an epilogue over the finished output rows, for layers that transform BEFORE they aggregate
 * (in > out — every default configuration of the reference, initial_params.py:25-29: F -> 64 -> C with C = 7, 6, 3, 40 ...),
 * whose last kernel is this gather and not the fused aggregate+transform one. A lane group holds a target's complete
 * output row, so what the reference runs next as separate passes over [N, d] comes out of the registers:
 *   out_colsums ([2, d] doubles): column sums of out and out^2 — the statistics of the training-mode BatchNorm1d
 *     behind the layer (models/gcn.py:27 then :28); per 32-row tile an fp32 record (sum, squared deviations from the
 *     tile's own mean), the tiles' sum x and sum x^2 = M2 + S^2 / n added in fp64 in a fixed order (a column whose
 *     spread is far below its mean keeps its variance);
 *     stats_ws: rgbx_spmm_linear_stats_workspace_bytes(N, d) bytes, 8-byte aligned. `out` is written as usual.
 *   ce: log_softmax + NLLLoss on out[mask] + arg-max (models/gcn.py:31, itexperiments.py:400,429,434,624-626) exactly as
 *     rgbx_ce_epilogue_t describes: statistics only (out not written, may be NULL; rows no mask selects are not even
 *     gathered) or, with grad_scale, `out` = the loss gradient w.r.t. the logits. n_classes = C <= d: columns [C, d) are
 *     PADDING (rows padded to a multiple of 4 floats: C = 7 -> d = 8) — no part in max / sum-exp / arg-max, gradient 0;
 *     0 = all d columns. Labels outside [0, C) deselect a row. ce->scratch as for rgbx_spmm_linear_f32.
 * Exactly one of out_colsums / ce. d % 4 == 0, d <= 256 (rgbx_spmm_csr_epilogue_supported); x, y, out, bias 16-byte
 * aligned, leading dimensions % 4 == 0. The logits are bit-identical to rgbx_spmm_csr_f32's (same summation order).
 * `split`: as rgbx_spmm_linear_f32 — split->partial must hold (n_chunks + n_long) * d floats. */
typedef struct rgbx_spmm_epilogue {
  const struct rgbx_ce_epilogue* ce; /* or NULL */
  int64_t n_classes;
  double* out_colsums;               /* or NULL */
  void* stats_ws;
  size_t stats_ws_bytes;
} rgbx_spmm_epilogue_t;

int rgbx_spmm_csr_epilogue_supported(int64_t d);
int rgbx_spmm_csr_epilogue_f32(const int32_t* rowptr, const int32_t* col, const float* w, const float* rs,
                               const float* x, int64_t ldx, const float* y, int64_t ldy, const float* bias,
                               float* out, int64_t ldo, int64_t N, int64_t d, float a, float b,
                               const rgbx_row_split_t* split, const rgbx_spmm_epilogue_t* epi,
                               rgbx_stream_t stream);

/* The same weighted row gather for SHORT rows over a SMALL table, one lane group per target row (a wave takes 64 / G rows):
 *   out[i,:] = sum_{p in row i} w[p] * x[col[p],:] + bias      (w optional: NULL = 1; slot order, deterministic)
 * What it replaces: the first Linear of every reference model applied to bag-of-words features — x W^T with x the
 * row-normalised counts of itexperiments.py:296 (models/gcn.py:27, graphsage.py:49-50, appnp_stack.py:25, dagnn.py:73) —
 * computed over the features' non-zeros: CSR rows = nodes, col = feature ids, w = feature values, the gathered table
 * W^T [F, d] (L2-resident). rgbx_spmm_csr_f32 gives the same sums (up to summation order) with one wave per row; with the
 * table in cache that form is bound by wave issue. d % 4 == 0, d <= 256; x, out, bias 16-byte aligned, ldx, ldo % 4 == 0.
 * No row-split plan: a long row is walked by its one lane group. */
int rgbx_spmm_csr_short_rows_supported(int64_t d);
int rgbx_spmm_csr_short_rows_f32(const int32_t* rowptr, const int32_t* col, const float* w, const float* x, int64_t ldx,
                                 const float* bias, float* out, int64_t ldo, int64_t N, int64_t d, rgbx_stream_t stream);

/* Fused aggregate-then-transform for layers whose propagate commutes with their Linear
 * (GCNConv, the mean branch of SAGEConv / my_SAGEConv):
 *   z[i,:]   = rs[i] * sum_{p in row i} w[p] * x[col[p],:]          (w, rs optional as above)
 *   out[i,:] = z[i,:] * wt + x_root[i,:] * wt_root + bias,   wt = W^T as a [K, Nout] row-major matrix
 * The [32 x K] tile of z lives in LDS and is multiplied on v_mfma_f32_32x32x2_f32 (exact fp32). If z_out is
 * not NULL the aggregate is also stored (ldz), for the weight gradient dy^T z of a training pass.
 * Root term (optional; x_root and wt_root both NULL or both set): SAGEConv's lin_r(x_i)
 * (models/graphsage.py:50,60; graphsage2.py:29 [PyG]) — x_root [N, K] (ldr) are the targets' own rows
 * (usually x itself), wt_root = Wr^T [K, Nout].
 * Supported shapes: K % 4 == 0, K <= 256, Nout % 32 == 0, and Nout <= 256 with a root term
 * (rgbx_spmm_linear_supported); otherwise RGBX_E_SHAPE and the caller runs rgbx_spmm_csr_f32 + GEMMs.
 * `split` (optional): hub rows are aggregated first by the split-row kernels (chunk sums added in chunk order)
 * and the fused kernel copies their finished aggregates; `split->partial` must then hold
 * (n_chunks + n_long) * K floats.
 * `pre_scale`, `pre_shift` ([K]) and `pre_rowsum` ([N]) — all NULL or all set: the layer's input is the affinely
 * mapped matrix x' = x * pre_scale + pre_shift (per column), which is never materialised: a training-mode
 * BatchNorm1d in front of the conv layer (models/gcn.py:28 then :29). By linearity
 *   z[i,:] = pre_scale * (rs[i] * sum_p w[p] x[col[p],:]) + pre_shift * pre_rowsum[i],
 * pre_rowsum[i] = rs[i] * sum_{p in row i} w[p] (the caller's per-graph constant); the root rows get the map as
 * they are loaded; z_out receives the mapped aggregate (what dW = dy^T z needs).
 * `out_colsums` ([2, Nout] doubles, optional): out_colsums[0,c] = sum_i out[i,c], [1,c] = sum_i out[i,c]^2 — the
 * statistics of a training-mode BatchNorm1d that follows the layer (models/gcn.py:27 then :28), taken from the
 * MFMA accumulators of the 32-row tiles (per tile an fp32 record of the sum and of the squared deviations from the
 * tile's mean; sum x and sum x^2 = M2 + S^2 / n over the tiles in fp64 in a fixed order) instead of a pass
 * over `out`; needs `stats_ws` of rgbx_spmm_linear_stats_workspace_bytes(N, Nout) bytes (8-byte aligned). */
/* Optional cross-entropy epilogue of rgbx_spmm_linear_f32, for the model's LAST layer (models/gcn.py:29-31: the
 * logits go straight into log_softmax + NLLLoss on out[mask], itexperiments.py:400,429, or into the arg-max /
 * loss metrics of :624-626): the loss quantities come out of the 32 x Nout output tiles while they are in LDS.
 *   stats[0] = sum over selected rows of logsumexp(out_i) - out[i, y_i], stats[1] = selected rows,
 *   stats[2] = selected rows whose first arg-max equals y_i    (selection as rgbx_masked_ce_fwd_f32)
 * grad_scale == NULL: statistics only, `out` is NOT written (may be NULL) — an eval forward whose logits nobody
 * reads. grad_scale != NULL (device scalar): `out` receives grad_scale * (softmax(out_i) - onehot(y_i)) for selected
 * rows, 0 otherwise: the gradient of grad_scale * stats[0] w.r.t. the logits (rgbx_masked_ce_bwd_f32), instead of
 * the logits. scratch: (ceil(N / 32) + 64) * 3 doubles. Needs Nout <= 128; excludes out_colsums. */
typedef struct rgbx_ce_epilogue {
  const int64_t* y;        /* [N] labels */
  const uint8_t* mask;     /* [N] or NULL = all rows */
  const float* grad_scale; /* device scalar or NULL */
  double* stats;           /* [3]; [6] with mask_groups == 2 */
  double* scratch;         /* [(ceil(N / 32) + 64) * 3]; * 6 with mask_groups == 2; with `rows` AND grad_scale:
                            * rgbx_ce_rows_grad_scratch_doubles(N) = (ceil(N / 32) + 64) * 3 + ceil(N / 2) + ceil(N / 8) */
  /* 0 / 1: `mask` is a boolean. 2 (since 4.0.2; statistics only, mask required): bit 0 / bit 1 of mask[i] select row i
   * for statistics set 0 / set 1 — stats[0:3] and stats[3:6] — so that ONE eval forward serves the val and the test
   * metrics of an epoch (itexperiments.py:464-473 runs two identical forwards for them). */
  int32_t mask_groups;
  /* Selected rows only (single-GPU callers; all zero = every row as before). A row is SELECTED when its mask bit(s) are
   * set (any of the two with mask_groups == 2) AND its label lies in [0, C): the epilogue's own predicate, which the
   * row list and rgbx_fused_layer_t.col_sel of the backward must restate exactly.
   *   rows / n_rows: an aggregating launch of rgbx_spmm_linear_f32 / rgbx_fused_layer_f32 (not DENSE, no w_pos): the
   *     ascending int32 device list of exactly the selected rows (with mask_groups == 2 those of the union of both masks),
   *     0 <= n_rows <= N. Tile t aggregates rows[32 t .. 32 t + 31]: ceil(n_rows / 32) tiles and workgroups instead of
   *     ceil(N / 32); unlisted rows are not gathered at all. Hub rows of `split` keep working for listed rows.
   *     - statistics only (grad_scale == NULL, no z_out): one record per list tile; statistics as without the list (the
   *       nll sum up to the order of its fp64 additions).
   *     - with the loss gradient (grad_scale set, z_out optional, mask_groups != 2): `out`, z_out and the
   *       statistics are those of skip_unselected BIT FOR BIT. Unlisted rows of `out` and z_out are written as 0: the wave
   *       that takes list slot i zero-fills rows rows[i-1] + 1 .. rows[i] - 1 (from row 0 for i = 0; the last slot also
   *       the rows behind it), which needs `out` 16-byte aligned with ldo % 4 == 0. The kernel writes per listed row its
   *       fp32 nll term and arg-max hit into the tail of `scratch` (N floats, then N bytes, behind the records; never
   *       read for a row the predicate does not select, so it needs no initialisation), and a small kernel forms the
   *       ceil(N / 32) tile records of the unlisted form from them in that form's order of additions; `scratch` must
   *       hold rgbx_ce_rows_grad_scratch_doubles(N) doubles. n_rows == 0 runs as skip_unselected.
   *   skip_unselected != 0: the tiles map to rows as without a list, but a row that is not selected issues no gather;
   *     its z_out row is written as 0 (pre_* not applied), its `out` row (loss gradient) is 0 as always. The gradient,
   *     the statistics and dW = dy^T z are unchanged (the gradient row is 0 there). Not with w_pos (ignored). */
  const int32_t* rows;
  int64_t n_rows;
  int32_t skip_unselected;
  /* no_fill != 0 (default 0 = fill as described above): the loss gradient over a row list leaves the unlisted rows of `out`
   * and z_out UNWRITTEN instead of writing them as 0 — whatever the buffers held stays there and may be NaN. Listed rows
   * and the statistics keep every bit. For callers all of whose readers of the two matrices walk the same list or honour
   * the same selection (rgbx_gemm_tn_rows_f32; rgbx_fused_layer_t.col_sel on a transposed CSR without hub rows): the
   * zeros are then bytes nobody reads. Ignored by every other form (no list, statistics only, n_rows == 0: those write
   * what they always wrote). */
  int32_t no_fill;
} rgbx_ce_epilogue_t;

int rgbx_spmm_linear_supported(int64_t K, int64_t Nout, int has_root);
/* Doubles of rgbx_ce_epilogue_t.scratch a loss-gradient launch over a row list needs for N rows. */
int rgbx_ce_rows_grad_scratch_doubles(int64_t N, int64_t* count);
int rgbx_spmm_linear_stats_workspace_bytes(int64_t N, int64_t Nout, size_t* bytes);
int rgbx_spmm_linear_f32(const int32_t* rowptr, const int32_t* col, const float* w, const float* rs,
                         const float* x, int64_t ldx, const float* wt, const float* x_root, int64_t ldr,
                         const float* wt_root, const float* bias, float* out, int64_t ldo, float* z_out,
                         int64_t ldz, const float* pre_scale, const float* pre_shift, const float* pre_rowsum,
                         double* out_colsums, void* stats_ws, size_t stats_ws_bytes,
                         const rgbx_ce_epilogue_t* ce, int64_t N, int64_t K, int64_t Nout,
                         const rgbx_row_split_t* split, rgbx_stream_t stream);

/* The same layer with everything a NODE-PARTITIONED run needs of it (new capability: the reference is single-device,
 * itexperiments.py:246; the layer arithmetic is unchanged: models/gcn.py:27-29, graphsage.py:49-62), all arguments in
 * one struct. On top of rgbx_spmm_linear_f32:
 *  - DENSE mode (rowptr == NULL): the 32-row tile is not aggregated here but LOADED — row i of the tile is row i of
 *    `x` (after the optional pre-affine map, where pre_rowsum[i] multiplies pre_shift as above). This is the RETURN
 *    stage of the row-group x column-slice exchange: another rank aggregated column slices of this rank's rows and
 *    sent them back; transform, root term, statistics and the loss epilogue then run here without an unpack pass.
 *    It is also the plain product x * wt (e.g. dy * W of the backward pass) with any of the stores below.
 *  - BLOCKED layouts: a matrix whose columns are cut into blocks of `cols` columns, each block stored as its own
 *    contiguous [N, cols] matrix, `stride` elements from one block to the next: element (i, c) lives at
 *    base + (c / cols) * stride + i * cols + c % cols. cols == 0 means plain row-major with the leading dimension
 *    given beside it. Column slices of the rows are what the exchange sends and receives, so a producer writes its
 *    output blocked straight into the send buffer (out_blk; `out` row-major may be written as well, or be NULL) and a
 *    consumer reads the received slices in place (x in DENSE mode, x_root always). cols % 4 == 0.
 * Everything else (w, rs, root term, z_out, pre_*, out_colsums, ce, split) as rgbx_spmm_linear_f32. */
typedef struct rgbx_fused_layer {
  const int32_t* rowptr;   /* NULL = DENSE mode (col, w, rs, split ignored) */
  const int32_t* col;
  const float* w;
  const float* rs;
  const float* x;
  int64_t ldx;
  int64_t x_blk_cols, x_blk_stride;   /* DENSE mode only */
  const float* wt;         /* [K, Nout] */
  const float* x_root;     /* or NULL */
  int64_t ldr;
  int64_t xr_blk_cols, xr_blk_stride;
  const float* wt_root;
  const float* bias;
  float* out;              /* row-major [N, Nout] (ldo), or NULL */
  int64_t ldo;
  float* out_blk;          /* blocked copy of the output, or NULL */
  int64_t ob_cols, ob_stride;
  float* z_out;            /* [N, K] (ldz) or NULL */
  int64_t ldz;
  const float* pre_scale;
  const float* pre_shift;
  const float* pre_rowsum;
  double* out_colsums;
  void* stats_ws;
  size_t stats_ws_bytes;
  const rgbx_ce_epilogue_t* ce;
  int64_t N, K, Nout;
  const rgbx_row_split_t* split;
  /* Second aggregate (both NULL, or both set): z_pos_out[i,:] (ld = ldz) = sum_p w_pos[p] x[col[p],:] over the same
   * slots, from the rows the launch gathers anyway; never transformed. Single-head GAT's training forward: w = the
   * attention coefficients, w_pos = those of edges with a positive score (rgbx_gat_edge_softmax_f32), the pair
   * (z_out, z_pos_out) = (out, out_pos) of rgbx_gat_bwd_prep_f32. Needs w and z_out, K in {64, 128, 256}, Nout <= 128,
   * no rs / pre_* / out_blk; with `split`, split->partial must hold n_chunks * K + 2 * n_long * K floats. */
  const float* w_pos;
  float* z_pos_out;
  /* Column selection (optional, NULL = every slot gathered): a slot whose column c has col_sel[c] == 0 issues no gather
   * and adds 0, exactly as a slot whose gathered row is 0 would (per-slot weights >= 0, e.g. gcn_norm / mean). For the
   * transposed launch of a last layer whose output gradient is 0 outside the rows its loss selects (rgbx_ce_epilogue_t:
   * mask bit AND a label in [0, C)): those rows are not read, and every slot keeps its place in the summation, so the
   * result is bit-identical to the full gather. An aggregating launch without ce / w_pos / blocked layouts; col_sel must
   * have an entry for every column of the CSR. Honoured for K in {64, 128, 256} and Nout <= 128 without blocked layouts;
   * elsewhere, and for the hub rows of `split`, every slot is gathered (the same result). */
  const uint8_t* col_sel;
  /* The same selection carried in the column stream (optional, only together with col_sel and under its conditions; NULL =
   * col_sel is looked up per slot as before): [nnz] entries made by rgbx_col_tag_i32 from `col` and col_sel,
   * col_tag[p] = col[p] if col_sel[col[p]] else ~col[p]. Where col_sel is honoured the launch reads a slot's entry from
   * col_tag instead of `col`: a negative entry is a hole (no gather, no load of w[p], adds 0 in its place), col_sel itself
   * is not touched. `col` stays as it is and must still be passed: the hub rows of `split` and every launch that does not
   * honour col_sel read it, and ignore col_tag. Same result as col_sel alone, bit for bit. */
  const int32_t* col_tag;
} rgbx_fused_layer_t;

int rgbx_fused_layer_f32(const rgbx_fused_layer_t* layer, rgbx_stream_t stream);

/* col_tag[p] = sel[col[p]] ? col[p] : ~col[p] for p < nnz: rgbx_fused_layer_t.col_tag of a CSR's `col` [nnz] under the
 * selection `sel` (uint8 [n_cols]). A deselected slot is negative and keeps its column recoverable (~col_tag[p]); a
 * column outside [0, n_cols) is tagged as deselected. Made once per (CSR, selection); nnz == 0 does nothing. */
int rgbx_col_tag_i32(const int32_t* col, const uint8_t* sel, int64_t nnz, int64_t n_cols, int32_t* col_tag,
                     rgbx_stream_t stream);

/* dst[i, c] (row-major, ldd) = src (blocked as above: blk_cols, blk_stride)[i, c] (+ bias[c], bias optional) for
 * i < n, c < d: the unpack of received column slices where a consumer wants plain rows (BatchNorm's backward kernels; the
 * logits of an eval forward whose last transform ran before the exchange, + the layer's bias). */
int rgbx_blocked_to_rows_f32(const float* src, int64_t blk_cols, int64_t blk_stride, float* dst, int64_t ldd,
                             int64_t n, int64_t d, const float* bias, rgbx_stream_t stream);

/* z_0 = h;  z_{k+1} = (1-alpha) * A_hat z_k + alpha * h, k = 0..K-1; result in `out`.
 * `tmp` is an [N, d] scratch (ld = ldo); h, out, tmp must not alias. K >= 0. */
int rgbx_appnp_f32(const int32_t* rowptr, const int32_t* col, const float* w, const float* h,
                   int64_t ldh, float* out, float* tmp, int64_t ldo, int64_t N, int64_t d, int K,
                   float alpha, const rgbx_row_split_t* split, rgbx_stream_t stream);

/* ---- DAGNN: adaptive mix of the K+1 hops (reference models/dagnn.py:49-55) ---------------- */

/* Hop 0 is the layer input h0 [N, d] (ld0); hops 1..K are K matrices [N, d] (ldh) `hop_stride` floats apart,
 * written there by K calls of rgbx_spmm_csr_f32.  s [d] / b [1] = weight / bias of Prop.proj = Linear(C, 1),
 * both on the device.   retain[i,k] = sigmoid(<hop_k[i,:], s> + b);   out[i,:] = sum_k retain[i,k] * hop_k[i,:]
 * (the stack / proj / sigmoid / matmul of dagnn.py:51-54 in one pass over the hops).  d % 4 == 0, d <= 256,
 * 16-byte aligned rows. */
int rgbx_dagnn_gate_fwd_f32(const float* h0, int64_t ld0, const float* hops, int64_t hop_stride, int64_t ldh,
                            const float* s, const float* b, float* out, int64_t ldo, int64_t N, int64_t d, int K,
                            rgbx_stream_t stream);

/* Backward of the mix for gout = dL/dout [N, d]: per hop the DIRECT part of that hop's gradient,
 *   direct_k[i,:] = retain[i,k] * gout[i,:] + c[i,k] * s,   c[i,k] = <gout_i, hop_k[i]> retain (1 - retain),
 * written to d0 (hop 0) and dk + (k-1) * d_stride (hops 1..K) — the `y` operands of the Horner chain
 * G_k = A_hat^T G_{k+1} + direct_k run with rgbx_spmm_csr_f32 on the transposed CSR — and the gradients of the
 * projection, g_s[d] = sum_ik c[i,k] hop_k[i,:], g_b[1] = sum_ik c[i,k] (g_b may be NULL).  `ws`: scratch of
 * rgbx_dagnn_gate_bwd_workspace_bytes(d) bytes (per-block partial sums, added in block order). */
int rgbx_dagnn_gate_bwd_workspace_bytes(int64_t d, size_t* bytes);
int rgbx_dagnn_gate_bwd_f32(const float* h0, int64_t ld0, const float* hops, int64_t hop_stride, int64_t ldh,
                            const float* s, const float* b, const float* gout, int64_t ldg, float* d0,
                            int64_t ldd0, float* dk, int64_t d_stride, int64_t ldd, float* g_s, float* g_b,
                            void* ws, size_t ws_bytes, int64_t N, int64_t d, int K, rgbx_stream_t stream);

/* ---- GGNN: one GatedGraphConv step (PyG GatedGraphConv, reference models/ggnn.py) ----------- */

/* One propagation step on the state x [N, C] with the GRUCell's gates in the column order (r, z, n):
 *   pre = (A x) Weffᵀ + x Wrootᵀ + bias   [N, 4C], columns [ r, z pre-activations (2C) | gi_n (C) | gh_n (C) ]
 *   r = σ(pre_r), z = σ(pre_z), n = tanh(gi_n + r ⊙ gh_n),   out = (1 - z) ⊙ n + z ⊙ x
 * A = the plain edge sum over the target-grouped CSR (rowptr, col), no weights. wt = Weffᵀ and wt_root = Wrootᵀ are
 * [C, 4C] row-major, bias [4C], all on the device (Weff = [W_ih[r,z]; W_ih[n]; 0] weight[i]ᵀ,
 * Wroot = [W_hh[r,z]; 0; W_hh[n]], bias = [b_ih[r,z] + b_hh[r,z]; b_ih[n]; b_hh[n]]).
 * ONE kernel: the gather, both MFMA products and the GRU epilogue; only `out` is written, plus (training) the
 * aggregate A x into z_out [N, C] and pre into pre_out [N, 4C] when they are not NULL.
 * C % 8 == 0, 8 <= C <= 64 (rgbx_gru_step_supported); x, out, z_out, pre_out 16-byte aligned, leading dimensions % 4 == 0;
 * out must not alias x. `split`: as rgbx_spmm_linear_f32 — split->partial must hold (n_chunks + n_long) * C floats. */
int rgbx_gru_step_supported(int64_t C);
int rgbx_gru_step_f32(const int32_t* rowptr, const int32_t* col, const float* x, int64_t ldx, const float* wt,
                      const float* wt_root, const float* bias, float* out, int64_t ldo, float* z_out, int64_t ldz,
                      float* pre_out, int64_t ldp, int64_t N, int64_t C, const rgbx_row_split_t* split,
                      rgbx_stream_t stream);

/* The GRU cell alone over a finished pre [N, 4C] (ldp) as rgbx_gru_step_f32 lays it out: out [N, C] = the new state
 * for the old state x. C % 4 == 0; every matrix 16-byte aligned with leading dimension % 4 == 0. */
int rgbx_gru_gate_fwd_f32(const float* pre, int64_t ldp, const float* x, int64_t ldx, float* out, int64_t ldo,
                          int64_t N, int64_t C, rgbx_stream_t stream);

/* Backward of the cell for gout = dL/dout [N, C]:
 *   dpre [N, 4C] = [ dr ⊙ r(1-r) | dz ⊙ z(1-z) | dgi_n | dgi_n ⊙ r ],  dgi_n = gout (1 - z)(1 - n²), dr = dgi_n ⊙ gh_n,
 *   dz = gout ⊙ (x - n);   dx [N, C] = gout ⊙ z (the direct part of the state's gradient; the parts through A and
 *   Wroot are the caller's products). Same shape rules as rgbx_gru_gate_fwd_f32. */
int rgbx_gru_gate_bwd_f32(const float* pre, int64_t ldp, const float* x, int64_t ldx, const float* gout, int64_t ldg,
                          float* dpre, int64_t lddp, float* dx, int64_t lddx, int64_t N, int64_t C,
                          rgbx_stream_t stream);

/* ---- GAT: fused score + edge-softmax + aggregate ------------------------------------------ */

/* a_src[n,h] = <hfeat[n,h,:], att_src[h,:]>, a_dst likewise; hfeat is [n, H*C] (ld = ldh). */
int rgbx_gat_scores_f32(const float* hfeat, int64_t ldh, const float* att_src,
                        const float* att_dst, float* a_src, float* a_dst, int64_t n, int H, int C,
                        rgbx_stream_t stream);

/* Floats of device scratch rgbx_gat_scores_bwd_f32 needs (per-workgroup partial sums). */
int rgbx_gat_scores_bwd_scratch_floats(int64_t n, int H, int C, int64_t* count);

/* Backward of rgbx_gat_scores_f32, fused with the accumulation into the feature gradient:
 *   g_hfeat[r,h,:] += g_a_src[r,h] * att_src[h,:] + g_a_dst[r,h] * att_dst[h,:]   (in place; skipped when
 *                                                  g_hfeat is NULL: rgbx_gat_bwd_src_f32 can fold it into its store)
 *   g_att_src[h,:]  = sum_r g_a_src[r,h] * hfeat[r,h,:],   g_att_dst likewise
 * over rows r in [0, n); g_a_dst has n_dst <= n rows (rows beyond are zero: halo rows of a partitioned
 * run have no target role). Partial sums per workgroup are added in workgroup order (reproducible). */
int rgbx_gat_scores_bwd_f32(const float* hfeat, int64_t ldh, const float* g_a_src, const float* g_a_dst,
                            int64_t n_dst, const float* att_src, const float* att_dst, float* g_hfeat,
                            int64_t ldgh, float* g_att_src, float* g_att_dst, float* scratch,
                            int64_t scratch_floats, int64_t n, int H, int C, rgbx_stream_t stream);

/* Forward over the target-grouped CSR. For every target i and head h:
 *   e_p   = leaky_relu(a_src[col[p],h] + a_dst[i,h], slope)
 *   alpha = exp(e_p - max_p e_p) / (sum_p exp(e_p - max) + 1e-16)
 *   out[i,h,:] = sum_p alpha_p * hfeat[col[p],h,:]
 * Saves m[i,h] = max and rden[i,h] = 1/(sum + 1e-16) for backward (both [N,H]).
 * Rows without edges produce 0 (m = 0, rden = 0).
 * Source scores: either `a_src` ([n_src, H], gathered per edge) or, when `att_src` ([H, C]) is not
 * NULL, recomputed inside the kernel from each gathered row as <hfeat[col[p],h,:], att_src[h,:]>
 * (saves one cache-line request per edge; `a_src` is then ignored and may be NULL).
 * Target scores: `a_dst` ([N, H]) is an INPUT when `att_dst` is NULL. With `att_dst` ([H, C]) the kernel forms
 * a_dst[i,h] = <hfeat[i,h,:], att_dst[h,:]> itself from the target's own row (targets are rows [0, N) of hfeat) and,
 * if `a_dst` is not NULL, stores it there for the backward: rgbx_gat_scores_f32 is then not needed at all.
 * `bias` ([H*C], optional): added to every stored row (GATConv's `out + bias` with concat=True, or heads=1);
 * pass the same pointer to rgbx_gat_bwd_prep_f32, which needs the bare aggregate.
 * `out_scale` ([H*C], optional, inference only): stored row = aggregate * out_scale + bias — an eval-mode
 * BatchNorm after the layer (models/gat.py:29) folded into the store (bias then = bias * scale + shift).
 * `out_pos` ([N, H*C], dense) and `a_pos` ([N, H]) — both NULL (inference) or both set (a forward whose backward
 * will be asked for): the part of the aggregate, and of the attention mass, carried by edges whose pre-activation
 * score a_src[j] + a_dst[i] is positive,
 *   out_pos[i,h,:] = sum_{p: s_p > 0} alpha_p * hfeat[col[p],h,:],   a_pos[i,h] = sum_{p: s_p > 0} alpha_p.
 * LeakyReLU's derivative is 1 on those edges and `slope` on the others, which turns the target-side score
 * gradient into a per-node expression (rgbx_gat_bwd_prep_f32): no per-edge tensor is written in the backward.
 * `split` (optional): hub targets are cut into chunks whose online-softmax states are merged in chunk
 * order; `split->partial` must hold n_chunks * (H*C + 2*H) floats, or n_chunks * (2*H*C + 3*H) with out_pos. */
int rgbx_gat_aggregate_fwd_f32(const int32_t* rowptr, const int32_t* col, const float* hfeat,
                               int64_t ldh, const float* a_src, const float* att_src,
                               float* a_dst, const float* att_dst, const float* out_scale, const float* bias,
                               float* out, int64_t ldo, float* m, float* rden, float* out_pos, float* a_pos,
                               int64_t N, int H, int C, float slope, const rgbx_row_split_t* split,
                               rgbx_stream_t stream);

/* Single head: the attention coefficients of every in-edge as a per-edge vector in CSR slot order,
 *   alpha[p] = exp(e_p - max) / (sum + 1e-16),  e_p = leaky_relu(a_src[col[p]] + a_dst[i], slope)   (p in row i),
 * plus m[i] / rden[i] as rgbx_gat_aggregate_fwd_f32 saves them. With ONE head the transform of a GATConv can run
 * behind the aggregation, out_i = (sum_j alpha_ij x_j) W^T + b with scores a = x (W^T att) (GATConv.forward with
 * heads = 1 [PyG], the last layer of reference models/gat.py:21,30), which is rgbx_fused_layer_f32 with w = alpha:
 * no h = x W^T product and no logits pass (the loss epilogue applies). `alpha_pos` ([E']) and `a_pos` ([N]): both NULL
 * (inference) or both set — alpha_pos[p] = alpha[p] where the pre-activation score is positive, else 0, a_pos[i] their
 * sum: rgbx_fused_layer_f32's w_pos / z_pos_out then yield the out_pos of rgbx_gat_bwd_prep_f32.
 * `split` (optional): rows with more than split->threshold slots (split->long_row, n_long) get a workgroup each
 * instead of 8 lanes; no scratch needed (split->partial is not used). */
int rgbx_gat_edge_softmax_f32(const int32_t* rowptr, const int32_t* col, const float* a_src, const float* a_dst,
                              float slope, float* alpha, float* alpha_pos, float* m, float* rden, float* a_pos,
                              int64_t N, const rgbx_row_split_t* split, rgbx_stream_t stream);

/* Backward, target side (same CSR as forward). Per target i, head h:
 *   dsum[i,h]    = <gout[i,h,:], out[i,h,:]>
 *   g_a_dst[i,h] = sum_p alpha_p * (<gout[i,h,:], hfeat[col[p],h,:]> - dsum[i,h]) * lrelu'(s_p)
 * `nodeq` ([N,H,4] floats, 16-byte aligned) is an output consumed by the source-side pass: the record
 * (a_dst, m - log(rden), dsum, 0) of every (target, head) — alpha = exp(e - m) * rden = exp(e - (m - log rden)) —
 * so that pass needs one 16-byte gather per edge and head instead of four 4-byte ones. */
int rgbx_gat_bwd_dst_f32(const int32_t* rowptr, const int32_t* col, const float* hfeat,
                         int64_t ldh, const float* a_src, const float* a_dst, const float* m,
                         const float* rden, const float* out, int64_t ldo, const float* gout,
                         int64_t ldg, float* nodeq, float* g_a_dst, int64_t N, int H, int C,
                         float slope, rgbx_stream_t stream);

/* The per-target record alone (no neighbour loop, one streaming pass over out / gout):
 *   nodeq[i,h] = (a_dst[i,h], m[i,h] - log(rden[i,h]), dsum = <gout[i,h,:], out[i,h,:] - bias[h,:]>, 0)
 * (`bias` = the pointer given to the forward, or NULL). With the forward's `out_pos` / `a_pos` (all three of
 * out_pos, a_pos, g_a_dst set, or all NULL) also the target-side score gradient, with no pass over the edges:
 *   g_a_dst[i,h] = sum_p alpha_p (<gout_i, h_j> - dsum) lrelu'(s_p) = (1 - slope) (<gout_i, out_pos_i> - dsum a_pos_i). */
int rgbx_gat_bwd_prep_f32(const float* a_dst, const float* m, const float* rden, const float* out,
                          int64_t ldo, const float* bias, const float* gout, int64_t ldg, float* nodeq,
                          const float* out_pos, const float* a_pos, float slope, float* g_a_dst,
                          int64_t N, int H, int C, rgbx_stream_t stream);

/* Backward, source side, over the TRANSPOSED CSR (rows = sources j, col = targets i):
 *   g_hfeat[j,h,:] = sum_{p: j->i} alpha_p * gout[i,h,:]
 *   ds_p[h]        = alpha_p * (<gout[i,h,:], hfeat[j,h,:]> - dsum[i,h]) * lrelu'(s_p)
 *   g_a_src[j,h]   = sum_{p: j->i} ds_p[h]
 * alpha is recomputed from a_src[j] and nodeq[i]. If `ds` is not NULL, ds_p is also stored at
 * ds[p, :] ([E', H] in transposed-slot order): g_a_dst[i,h] = sum of ds over the in-edges of i is then a
 * width-H segment sum (rgbx_spmm_csr_f32 over the forward rowptr with col = the forward-slot ->
 * transposed-slot map), which replaces the second full gather pass of rgbx_gat_bwd_dst_f32.
 * `a_src` NULL: the source's own score is formed from its row with att_src = att2[0], as the forward did.
 * `att2` ([2, H, C] = [att_src; att_dst], optional) with `g_a_dst` ([N, H]: the target-side score gradient of every
 * SOURCE row, zero for rows that are no target): the backward of the two score products is folded into the store,
 *   g_hfeat[j,h,:] += g_a_src[j,h] * att_src[h,:] + g_a_dst[j,h] * att_dst[h,:]
 * — rgbx_gat_scores_bwd_f32 then runs with g_hfeat = NULL (attention-vector gradients only). */
int rgbx_gat_bwd_src_f32(const int32_t* rowptr_t, const int32_t* col_t, const float* hfeat,
                         int64_t ldh, const float* a_src, const float* nodeq, const float* gout,
                         int64_t ldg, float* g_hfeat, int64_t ldgh, float* g_a_src, float* ds,
                         const float* att2, const float* g_a_dst, int64_t N, int H, int C, float slope,
                         const rgbx_row_split_t* split, rgbx_stream_t stream);

/* ---- SuperGAT: "MX" attention (per-edge dot product inside the edge-softmax) + link-prediction loss ---------- */

/* For an edge j -> i (p = its slot in the target-grouped CSR) and head h, with hfeat [N, H*C]:
 *   d_p   = <hfeat[i,h,:], hfeat[j,h,:]>
 *   s_p   = (<hfeat[j,h,:], att_l[h,:]> + <hfeat[i,h,:], att_r[h,:]>) * sigmoid(d_p)
 *   alpha = softmax over the in-edges of i of leaky_relu(s_p, slope), as rgbx_gat_aggregate_fwd_f32 forms it
 *   out[i,h,:] = sum_p alpha_p * kappa_p * hfeat[j,h,:] (+ bias)
 * (SuperGATConv with attention_type='MX' [PyG], reference models/supergat.py). kappa = 1 in inference mode.
 *
 * Randomness. `seed` points to two 32-bit words ON THE DEVICE; NULL selects inference mode. Every random decision is
 * a hash of (seed, forward CSR slot, head) or (seed, negative slot, re-draw), so that the backward passes recompute
 * them and no per-edge tensor is stored:
 *   attention dropout  kappa_p[h] = keep / (1 - p_drop), keep with probability 1 - p_drop per (slot, head);
 *   positive sample    slot p takes part in the loss with probability pos_ratio (edge_sample_ratio).
 * rgbx_supergat_draws_u8 writes both decisions out ([E'] and [E', H], 0 / 1) for inspection. */

/* 1 if the attention kernels take H heads of C channels (as GATConv.kernel_channels: any C <= 64, even C <= 128,
 * C % 4 == 0 up to 256), else 0. Wider heads are padded per head by the caller. */
int rgbx_supergat_supported(int H, int C);

/* Number of 8-byte (sum, count) records the training forward over N rows with this split writes. */
int rgbx_supergat_loss_records(int64_t N, const rgbx_row_split_t* split, int64_t* count);

/* Forward over the target-grouped CSR: one gather pass; the target's row stays in registers. Saves m / rden ([N, H],
 * of the UNDROPPED softmax). `bias` ([H*C], optional) is added in the store. Training mode (seed != NULL) also forms the
 * positive half of the link-prediction loss in the same pass: for every kept slot the term softplus(-mean_h d_p);
 * (sum, count) per workgroup go to `loss_records` (n_loss_records >= rgbx_supergat_loss_records, 16-byte aligned) and
 * are added in record order, in double, into pos_stats[0] = sum and pos_stats[1] = count (reproducible).
 * `split`: hub rows as in rgbx_gat_aggregate_fwd_f32; split->partial holds n_chunks * (H*C + 2*H) floats. */
int rgbx_supergat_aggregate_fwd_f32(const int32_t* rowptr, const int32_t* col, const float* hfeat, int64_t ldh,
                                    const float* att_l, const float* att_r, const float* bias, float* out, int64_t ldo,
                                    float* m, float* rden, int64_t N, int H, int C, float slope, const uint32_t* seed,
                                    float p_drop, float pos_ratio, float* loss_records, int64_t n_loss_records,
                                    double* pos_stats, const rgbx_row_split_t* split, rgbx_stream_t stream);

/* Backward. Per edge and head, with t = <h_j, att_l> + <h_i, att_r>, sg = sigmoid(d):
 *   g_e = alpha (kappa <gout_i, h_j> - <gout_i, out_i - bias>),  g_s = g_e lrelu'(s),  g_t = g_s sg,
 *   g_d = g_s t sg (1 - sg)  +  [slot kept as a positive] (sigmoid(mean_h d) - 1) / H * gl[0]
 * `gl` (device scalar, training mode) = d loss / d att_loss divided by the number of loss terms.
 * Target side, over the forward CSR: g_hfeat[i,h,:] = sum_p g_d h_j + (sum_p g_t) att_r[h,:] (STORED), g_ar[i,h] = sum_p g_t,
 * and the record nodeq[i,h] = (<h_i, att_r>, m - log(rden), <gout_i, out_i - bias>, 0) ([N, H, 4], 16-byte aligned).
 * split->partial holds n_chunks * (H*C + H) floats. */
int rgbx_supergat_bwd_dst_f32(const int32_t* rowptr, const int32_t* col, const float* hfeat, int64_t ldh,
                              const float* att_l, const float* att_r, const float* m, const float* rden,
                              const float* out, int64_t ldo, const float* bias, const float* gout, int64_t ldg,
                              float* nodeq, float* g_hfeat, int64_t ldgh, float* g_ar, int64_t N, int H, int C,
                              float slope, const uint32_t* seed, float p_drop, float pos_ratio, const float* gl,
                              const rgbx_row_split_t* split, rgbx_stream_t stream);

/* Source side, over the TRANSPOSED CSR (rows = sources j, col_t = targets i), run AFTER the target side:
 *   g_hfeat[j,h,:] += sum_p (alpha_p kappa_p gout[i,h,:] + g_d h_i) + (sum_p g_t) att_l[h,:],   g_al[j,h] = sum_p g_t.
 * `t2f` ([E'], training mode): the forward CSR slot of every transposed slot (the key of its random decisions).
 * The attention-vector gradients are rgbx_gat_scores_bwd_f32(hfeat, g_al, g_ar, ..., g_hfeat = NULL). */
int rgbx_supergat_bwd_src_f32(const int32_t* rowptr_t, const int32_t* col_t, const int32_t* t2f, const float* hfeat,
                              int64_t ldh, const float* att_l, const float* nodeq, const float* gout, int64_t ldg,
                              float* g_hfeat, int64_t ldgh, float* g_al, int64_t N, int H, int C, float slope,
                              const uint32_t* seed, float p_drop, float pos_ratio, const float* gl,
                              const rgbx_row_split_t* split, rgbx_stream_t stream);

/* n_neg ordered pairs (u, v), u != v, neither in `keys`: the ascending distinct keys a * N + b of the UNDIRECTED edge
 * set (rgbx_coalesce_keys_i64 with mirror = 1). Slot k tries up to `redraws` i.i.d. uniform pairs; neg[k] = u,
 * neg[n_neg + k] = v, valid[k] = 1, or valid[k] = 0 (pair (0, 0)) when every draw was rejected. Duplicates may occur. */
int rgbx_supergat_sample_negatives(const uint64_t* keys, int64_t n_keys, int64_t N, const uint32_t* seed, int64_t n_neg,
                                   int redraws, int64_t* neg, uint8_t* valid, rgbx_stream_t stream);

/* Negative half of the loss: for every valid pair (valid NULL = all) the term softplus(<h_u, h_v> / H) over the whole
 * row; neg_stats[0] = sum, neg_stats[1] = count (double), via at most 8192 (sum, count) records added in record order. */
int rgbx_supergat_neg_loss_fwd_f32(const float* hfeat, int64_t ldh, const int64_t* neg, const uint8_t* valid,
                                   int64_t n_neg, int H, int C, float* loss_records, int64_t n_loss_records,
                                   double* neg_stats, rgbx_stream_t stream);

/* Its backward: g_hfeat[u,:] += g_z h_v and g_hfeat[v,:] += g_z h_u, g_z = sigmoid(z) gl[0] / H. Pairs share rows, so
 * the rows are updated with float atomics: THIS ONE SUM IS ORDER-DEPENDENT (last-bit differences between runs). */
int rgbx_supergat_neg_loss_bwd_f32(const float* hfeat, int64_t ldh, const int64_t* neg, const uint8_t* valid,
                                   int64_t n_neg, int H, int C, const float* gl, float* g_hfeat, int64_t ldgh,
                                   rgbx_stream_t stream);

/* pos[p] = 1 where slot p is a kept positive, drop[p * H + h] = 1 where (p, h) survives the attention dropout. */
int rgbx_supergat_draws_u8(const uint32_t* seed, int64_t nnz, int H, float p_drop, float pos_ratio, uint8_t* pos,
                           uint8_t* drop, rgbx_stream_t stream);

/* ---- GATv2: dynamic attention (the non-linearity in front of the attention vector) ---------------------------- */

/* For an edge j -> i (p = its slot in the target-grouped CSR) and head h, with xl, xr [N, H*C] and att [H*C]:
 *   s_p[c] = xl[j,h,c] + xr[i,h,c]
 *   e_p    = sum_c att[h,c] * leaky_relu(s_p[c], slope)
 *   alpha  = softmax over the in-edges of i of e_p, as rgbx_gat_aggregate_fwd_f32 forms it
 *   out[i,h,:] = sum_p alpha_p * kappa_p * xl[j,h,:] (+ bias)
 * (GATv2Conv.forward / edge_update / message [PyG]; Brody et al. 2022. The reference's zoo has no GATv2: the layer
 * sits where models/gat.py puts GATConv.) The score is no sum of per-node scalars, so every gathered xl row is scored
 * against the target's xr row in registers; the same row is the message.
 *
 * Attention dropout. `seed` points to two 32-bit words ON THE DEVICE; NULL = no dropout (kappa = 1). Otherwise
 * kappa_p[h] = keep / (1 - p_drop) with keep a hash of (seed, forward CSR slot, head), true with probability
 * 1 - p_drop; the backward passes recompute it and every score, so nothing per edge is stored.
 * rgbx_gatv2_draws_u8 writes the keep bits out for inspection. No entry point uses float atomics: two runs are
 * bit-identical. */

/* 1 if the kernels take H heads of C channels (as GATConv.kernel_channels: any C <= 64, even C <= 128, C % 4 == 0 up
 * to 256), else 0. Other widths are padded per head by the caller. */
int rgbx_gatv2_supported(int H, int C);

/* Forward over the target-grouped CSR: one gather pass with an online softmax. m / rden ([N, H], of the UNDROPPED
 * softmax) are saved for the backward; both NULL = inference form (and then seed must be NULL). `bias` ([H*C],
 * optional) is added in the store. `split`: hub rows as in rgbx_gat_aggregate_fwd_f32; split->partial holds
 * n_chunks * (H*C + 2*H) floats. Float pointers that are not 4-byte aligned: RGBX_E_ALIGN. */
int rgbx_gatv2_fwd_f32(const int32_t* rowptr, const int32_t* col, const float* xl, int64_t ldl, const float* xr,
                       int64_t ldr, const float* att, const float* bias, float* out, int64_t ldo, float* m, float* rden,
                       int64_t N, int H, int C, float slope, const uint32_t* seed, float p_drop,
                       const rgbx_row_split_t* split, rgbx_stream_t stream);

/* Floats of the `att_partial` workspace of rgbx_gatv2_bwd_dst_f32: one [H*C] record per workgroup. */
int rgbx_gatv2_att_partial_floats(int64_t N, int H, int C, const rgbx_row_split_t* split, int64_t* count);

/* Backward. Per edge and head, with D_i = <gout_i, out_i - bias>:
 *   de = alpha (kappa <gout_i, xl_j> - D_i),   ds[c] = de att[h,c] lrelu'(s[c])
 * Target side, over the forward CSR: g_xr[i,h,:] = sum_p ds, g_att[h,c] = sum over all edges of de lrelu(s[c]) (per
 * workgroup records in att_partial, added in record order), and the record nodeq[i,h] = (m - log(rden), D_i)
 * ([N, H, 2], 8-byte aligned) of the source side. split->partial holds n_chunks * H*C floats. */
int rgbx_gatv2_bwd_dst_f32(const int32_t* rowptr, const int32_t* col, const float* xl, int64_t ldl, const float* xr,
                           int64_t ldr, const float* att, const float* m, const float* rden, const float* out,
                           int64_t ldo, const float* bias, const float* gout, int64_t ldg, float* nodeq, float* g_xr,
                           int64_t ldgr, float* g_att, float* att_partial, int64_t n_att_partial, int64_t N, int H,
                           int C, float slope, const uint32_t* seed, float p_drop, const rgbx_row_split_t* split,
                           rgbx_stream_t stream);

/* Source side, over the TRANSPOSED CSR (rows = sources j, col_t = targets i), run AFTER the target side:
 *   g_xl[j,h,:] = sum_p (alpha_p kappa_p gout[i,h,:] + ds_p).
 * `t2f` ([E'], needed when seed != NULL): the forward CSR slot of every transposed slot (the key of its keep bit).
 * split->partial holds n_chunks * H*C floats. */
int rgbx_gatv2_bwd_src_f32(const int32_t* rowptr_t, const int32_t* col_t, const int32_t* t2f, const float* xl,
                           int64_t ldl, const float* xr, int64_t ldr, const float* att, const float* nodeq,
                           const float* gout, int64_t ldg, float* g_xl, int64_t ldgl, int64_t N, int H, int C,
                           float slope, const uint32_t* seed, float p_drop, const rgbx_row_split_t* split,
                           rgbx_stream_t stream);

/* keep[p * H + h] = 1 where (forward CSR slot p, head h) survives the attention dropout. */
int rgbx_gatv2_draws_u8(const uint32_t* seed, int64_t nnz, int H, float p_drop, uint8_t* keep, rgbx_stream_t stream);

/* ---- TransformerConv: scaled dot-product attention over the in-edges --------------------------------------------- */

/* For an edge j -> i (p = its slot in the target-grouped CSR) and head h, with q, k, v [N, H*C] (each with its own
 * pointer and leading dimension; column blocks of one wider matrix are taken as they are):
 *   e_p    = <q[i,h,:], k[j,h,:]> * scale     (scale = 1 / sqrt(C) of the TRUE head width: the caller passes it, so
 *                                              zero-padding a head changes nothing)
 *   alpha  = softmax over the in-edges of i of e_p (online, max-shifted)
 *   out[i,h,:] = sum_p alpha_p * kappa_p * v[j,h,:]
 * (TransformerConv.forward / message [PyG]; Shi et al., "Masked Label Prediction". The reference's zoo has no
 * TransformerConv.) The scored row k_j is not the message v_j: two rows are gathered per slot. The edges are taken as
 * they are (RGBX_LOOPS_KEEP): a row WITHOUT slots stores exact zeros in `out`, the state m = rden = 0, the record
 * (0, 0) and a zero g_q row; a source without out-edges gets zero g_k and g_v rows. Every output row is written.
 *
 * Attention dropout as for rgbx_gatv2_*: `seed` = two 32-bit words ON THE DEVICE, NULL = no dropout; the keep bit of
 * (forward CSR slot, head) is the same hash, so rgbx_gatv2_draws_u8 writes these decisions out as well. No entry point
 * uses float atomics: two runs are bit-identical. */

/* 1 if the kernels take H heads of C channels (the set of rgbx_gatv2_supported), else 0. */
int rgbx_transformer_supported(int H, int C);

/* Forward over the target-grouped CSR: one gather pass with an online softmax. m / rden ([N, H], of the UNDROPPED
 * softmax) are saved for the backward; both NULL = inference form (and then seed must be NULL). `split`: hub rows as
 * in rgbx_gatv2_fwd_f32; split->partial holds n_chunks * (H*C + 2*H) floats, merged in chunk order. */
int rgbx_transformer_fwd_f32(const int32_t* rowptr, const int32_t* col, const float* q, int64_t ldq, const float* k,
                             int64_t ldk, const float* v, int64_t ldv, float* out, int64_t ldo, float* m, float* rden,
                             int64_t N, int H, int C, float scale, const uint32_t* seed, float p_drop,
                             const rgbx_row_split_t* split, rgbx_stream_t stream);

/* Backward. Per edge and head, with D_i = <gout_i, out_i>:  de = alpha (kappa <gout_i, v_j> - D_i).
 * Target side, over the forward CSR: g_q[i,h,:] = scale * sum_p de k_j and the record nodeq[i,h] = (m - log(rden), D_i)
 * ([N, H, 2], 8-byte aligned) of the source side. split->partial holds n_chunks * H*C floats. */
int rgbx_transformer_bwd_dst_f32(const int32_t* rowptr, const int32_t* col, const float* q, int64_t ldq, const float* k,
                                 int64_t ldk, const float* v, int64_t ldv, const float* m, const float* rden,
                                 const float* out, int64_t ldo, const float* gout, int64_t ldg, float* nodeq, float* g_q,
                                 int64_t ldgq, int64_t N, int H, int C, float scale, const uint32_t* seed, float p_drop,
                                 const rgbx_row_split_t* split, rgbx_stream_t stream);

/* Source side, over the TRANSPOSED CSR (rows = sources j, col_t = targets i), run AFTER the target side:
 *   g_k[j,h,:] = scale * sum_p de q_i,   g_v[j,h,:] = sum_p alpha_p kappa_p gout[i,h,:].
 * `t2f` ([E'], needed when seed != NULL): the forward CSR slot of every transposed slot (the key of its keep bit).
 * split->partial holds n_chunks * 2*H*C floats (g_k | g_v per chunk). */
int rgbx_transformer_bwd_src_f32(const int32_t* rowptr_t, const int32_t* col_t, const int32_t* t2f, const float* q,
                                 int64_t ldq, const float* k, int64_t ldk, const float* v, int64_t ldv,
                                 const float* nodeq, const float* gout, int64_t ldg, float* g_k, int64_t ldgk,
                                 float* g_v, int64_t ldgv, int64_t N, int H, int C, float scale, const uint32_t* seed,
                                 float p_drop, const rgbx_row_split_t* split, rgbx_stream_t stream);

/* ---- ResGatedGraphConv: per-channel sigmoid gate over the in-edges ------------------------------------------------- */

/* For an edge j -> i (p = its slot in the target-grouped CSR), with k, q, v [N, C] (each with its own pointer and
 * leading dimension; column blocks of one wider matrix are taken as they are):
 *   s_p      = sigmoid(k[i,:] + q[j,:])           (a vector per edge: one gate per channel)
 *   out[i,:] = sum_p s_p (.) v[j,:]
 * (ResGatedGraphConv.forward / message [PyG]; Bresson & Laurent, "Residual Gated Graph ConvNets". The reference's zoo
 * has no ResGatedGraphConv.) No softmax and no normaliser: nothing is saved for the backward, and the two backward
 * passes are independent of each other (each recomputes the gate from k and q). The sigmoid is evaluated through
 * exp(-|z|): no intermediate overflows, a saturated gate is exactly 0 or 1. The edges are taken as they are
 * (RGBX_LOOPS_KEEP): a row WITHOUT slots stores exact zeros in `out` and g_k; a source without out-edges gets zero g_q
 * and g_v rows. Every output row is written. No entry point uses float atomics: two runs are bit-identical. */

/* 1 if the kernels take C channels (the widths of rgbx_transformer_supported(1, C)), else 0. */
int rgbx_resgated_supported(int C);

/* Forward over the target-grouped CSR. `split`: hub rows as in rgbx_gatv2_fwd_f32; split->partial holds n_chunks * C
 * floats, added in chunk order. */
int rgbx_resgated_fwd_f32(const int32_t* rowptr, const int32_t* col, const float* k, int64_t ldk, const float* q,
                          int64_t ldq, const float* v, int64_t ldv, float* out, int64_t ldo, int64_t N, int C,
                          const rgbx_row_split_t* split, rgbx_stream_t stream);

/* Backward, target side, over the forward CSR:  g_k[i,:] = gout[i,:] (.) sum_p v[j,:] (.) s_p (1 - s_p).
 * split->partial holds n_chunks * C floats. */
int rgbx_resgated_bwd_dst_f32(const int32_t* rowptr, const int32_t* col, const float* k, int64_t ldk, const float* q,
                              int64_t ldq, const float* v, int64_t ldv, const float* gout, int64_t ldg, float* g_k,
                              int64_t ldgk, int64_t N, int C, const rgbx_row_split_t* split, rgbx_stream_t stream);

/* Backward, source side, over the TRANSPOSED CSR (rows = sources j, col_t = targets i), in any order with the target
 * side:   g_q[j,:] = v[j,:] (.) sum_p gout[i,:] (.) s_p (1 - s_p),   g_v[j,:] = sum_p s_p (.) gout[i,:].
 * split->partial holds n_chunks * 2*C floats (g_q | g_v per chunk). */
int rgbx_resgated_bwd_src_f32(const int32_t* rowptr_t, const int32_t* col_t, const float* k, int64_t ldk, const float* q,
                              int64_t ldq, const float* v, int64_t ldv, const float* gout, int64_t ldg, float* g_q,
                              int64_t ldgq, float* g_v, int64_t ldgv, int64_t N, int C, const rgbx_row_split_t* split,
                              rgbx_stream_t stream);

/* ---- GINEConv: relu(x_j + e_ji) summed over the in-edges, with a feature row per edge ------------------------------ */

/* For an edge j -> i (p = its slot in the target-grouped CSR), with x [N, C] and e [nnz, C] — ONE ROW PER SLOT, in
 * forward CSR slot order — each with its own pointer and leading dimension (column blocks of a wider matrix are taken
 * as they are):
 *   out[i,:] = (1 + eps) * x[i,:] + sum_p relu(x[j,:] + e[p,:])
 * (GINEConv.forward / message [PyG]; Hu et al., "Strategies for Pre-training Graph Neural Networks". The reference's
 * zoo has GIN, models/gin.py, and no GINEConv.) `eps` is ONE float in DEVICE memory, read by the kernels, never by the
 * host: a captured launch follows a parameter that an optimizer moves; NULL = no root term. Nothing is saved for the
 * backward: its two passes recompute the mask [x[j,:] + e[p,:] > 0] from the forward's own float32 add (relu'(0) = 0)
 * and are independent of each other. The edges are taken as they are (RGBX_LOOPS_KEEP): a row WITHOUT slots stores the
 * root term alone, a source without out-edges (1 + eps) gout[j,:]. Every output row is written, every slot row of g_e
 * too. No entry point uses float atomics: two runs are bit-identical. */

/* 1 if the kernels take C channels (the widths of rgbx_resgated_supported), else 0. */
int rgbx_gine_supported(int C);

/* Forward over the target-grouped CSR: x rows gathered, the e rows of a target read as a stream. `split`: hub rows as
 * in rgbx_gatv2_fwd_f32; split->partial holds n_chunks * C floats, added in chunk order (the root term rides on the
 * row's first chunk). */
int rgbx_gine_fwd_f32(const int32_t* rowptr, const int32_t* col, const float* x, int64_t ldx, const float* e,
                      int64_t lde, const float* eps, float* out, int64_t ldo, int64_t N, int C,
                      const rgbx_row_split_t* split, rgbx_stream_t stream);

/* Backward, edge side, over the forward CSR:  g_e[p,:] = gout[i,:] (.) [x[j,:] + e[p,:] > 0], one row per slot in
 * forward slot order. No sum is formed: every value is a copy of gout or an exact zero. `split` only balances the hub
 * rows (split->partial is not touched). */
int rgbx_gine_bwd_edge_f32(const int32_t* rowptr, const int32_t* col, const float* x, int64_t ldx, const float* e,
                           int64_t lde, const float* gout, int64_t ldg, float* g_e, int64_t ldge, int64_t N, int C,
                           const rgbx_row_split_t* split, rgbx_stream_t stream);

/* Backward, source side, over the TRANSPOSED CSR (rows = sources j, col_t = targets i, t2f [nnz] = the forward slot of
 * every transposed slot), in any order with the edge side:
 *   g_x[j,:] = (1 + eps) * gout[j,:] + sum_q gout[col_t[q],:] (.) [x[j,:] + e[t2f[q],:] > 0].
 * split->partial holds n_chunks * C floats. */
int rgbx_gine_bwd_src_f32(const int32_t* rowptr_t, const int32_t* col_t, const int32_t* t2f, const float* x,
                          int64_t ldx, const float* e, int64_t lde, const float* gout, int64_t ldg, const float* eps,
                          float* g_x, int64_t ldgx, int64_t N, int C, const rgbx_row_split_t* split,
                          rgbx_stream_t stream);

/* ---- CGConv: sigmoid(lin_f(z)) * softplus(lin_s(z)) over the in-edges, z = [x_i, x_j, e_ij] ----------------------- */

/* CGConv.message [PyG] forms `z = torch.cat([x_i, x_j, edge_attr], dim=-1)` per edge and returns
 * `self.lin_f(z).sigmoid() * F.softplus(self.lin_s(z))` (Xie & Grossman, "Crystal Graph Convolutional Neural Networks
 * for an Accurate and Interpretable Prediction of Material Properties"). The reference's zoo has no such layer. A
 * Linear over a concatenation is a sum of three Linears, so the dense products come first. For an edge j -> i (p = its
 * slot in the target-grouped CSR), with a, b [N, 2C] and c [nnz, 2C] — ONE ROW PER SLOT, in forward CSR slot order; every
 * row is (f half | s half); each operand its own pointer and leading dimension >= 2C (column blocks of a wider matrix
 * are taken as they are); c == NULL: no edge term —
 *   zf = a[i,:C] + b[j,:C] + c[p,:C]         zs = a[i,C:] + b[j,C:] + c[p,C:]
 *   msg_p    = sigmoid(zf) (.) softplus(zs)                          (a vector per edge: one gate per channel)
 *   out[i,:] = root[i,:] + scale_i * sum_p msg_p                     scale_i = 1, or with mean != 0  1.0f / (float)deg_i
 * with deg_i read from rowptr inside the kernels, never by the host (0 for a row without slots). Both branches go
 * through e = exp(-|z|): sigmoid = (z >= 0 ? 1 : e) / (1 + e), softplus = max(z, 0) + log1p(e), so no intermediate
 * overflows for any z and a saturated gate is exactly 0 or 1; exp, log and the reciprocal are the hardware instructions
 * (about 1 ulp each) and log1p(e) is log(1 + e): an absolute error of at most 2^-24 per slot in softplus. Nothing is saved for the backward: its two passes
 * recompute both branches from a, b, c and are independent of each other. The edges are taken as they are
 * (RGBX_LOOPS_KEEP): a row WITHOUT slots stores the root term alone (exact zeros without one) and a zero g_a row; a
 * source without out-edges gets a zero g_b row. Every output row is written, every slot row of g_c too. No entry point
 * uses float atomics, scratch or LDS; every sum runs in a fixed order: two runs are bit-identical. */

/* 1 if the kernels take C channels (the widths of rgbx_resgated_supported), else 0. */
int rgbx_cgconv_supported(int C);

/* Forward over the target-grouped CSR, out [N, C]: the target's a row stays in registers, b rows are gathered, the c
 * rows of a target read as a stream. `root` [N, C] is optional (NULL: none). `split`: hub rows as in rgbx_gatv2_fwd_f32;
 * split->partial holds n_chunks * C floats, added in chunk order (the root term rides on the row's first chunk). */
int rgbx_cgconv_fwd_f32(const int32_t* rowptr, const int32_t* col, const float* a, int64_t lda, const float* b,
                        int64_t ldb, const float* c, int64_t ldc, const float* root, int64_t ldr, float* out,
                        int64_t ldo, int64_t N, int C, int mean, const rgbx_row_split_t* split, rgbx_stream_t stream);

/* Backward, target side, over the forward CSR. With s = sigmoid(zf), t = softplus(zs), u = sigmoid(zs):
 *   gf_p = scale_i * gout[i,:] (.) s (1 - s) t       gs_p = scale_i * gout[i,:] (.) s u
 *   g_a[i,:] = (sum_p gf_p | sum_p gs_p)  [N, 2C]     g_c[p,:] = (gf_p | gs_p)  [nnz, 2C], one row per slot
 * Each output is optional (NULL: not wanted; both NULL: RGBX_E_ARG); g_c does not need c. split->partial holds
 * n_chunks * 2C floats (a chunk's record is the two sums); every slot's g_c row is written exactly once. */
int rgbx_cgconv_bwd_dst_f32(const int32_t* rowptr, const int32_t* col, const float* a, int64_t lda, const float* b,
                            int64_t ldb, const float* c, int64_t ldc, const float* gout, int64_t ldg, float* g_a,
                            int64_t ldga, float* g_c, int64_t ldgc, int64_t N, int C, int mean,
                            const rgbx_row_split_t* split, rgbx_stream_t stream);

/* Backward, source side, over the TRANSPOSED CSR (rows = sources j, col_t = targets i), in any order with the target
 * side:   g_b[j,:] = (sum_q gf_q | sum_q gs_q)  [N, 2C].
 * `t2f` [nnz] = the forward slot of every transposed slot (needed with c), `rowptr_f` [N + 1] = the forward rowptr
 * (needed with mean != 0: the targets' degrees). split->partial holds n_chunks * 2C floats. */
int rgbx_cgconv_bwd_src_f32(const int32_t* rowptr_t, const int32_t* col_t, const int32_t* t2f, const int32_t* rowptr_f,
                            const float* a, int64_t lda, const float* b, int64_t ldb, const float* c, int64_t ldc,
                            const float* gout, int64_t ldg, float* g_b, int64_t ldgb, int64_t N, int C, int mean,
                            const rgbx_row_split_t* split, rgbx_stream_t stream);

/* ---- RGCNConv: a relation per edge; mean per (target, relation), basis decomposition ------------------------------- */

/* Every edge j -> i carries a category, its relation etype in [0, R) (int32, one per CSR slot; the range is the
 * caller's contract, checked once when the typed view of a graph is built). RGCNConv.forward [PyG] loops over the
 * relations, masks the edge list and propagates once per relation (`for i in range(self.num_relations): tmp =
 * masked_edge_index(edge_index, edge_type == i); h = self.propagate(tmp, x=x_l); out += h @ weight[i]`), with
 * `weight = (self.comp @ weight.view(num_bases, -1))` in front of the loop under a basis decomposition
 * (Schlichtkrull et al., "Modeling Relational Data with Graph Convolutional Networks"). The reference's zoo has no
 * relational layer. Here the dense products come first (h = x @ [V_0 | ... | V_{B-1}], viewed as [N, B, C]) and ONE
 * pass over the edges mixes the B basis rows of every source with a per-slot, per-basis coefficient
 *   a[p, b] = w[p] * comp[etype[p], b]
 * which is neither a softmax nor saved anywhere: `comp` [R, B] (row-major, contiguous) is DEVICE memory read by the
 * kernels, so a captured launch follows a table that an optimizer moves. The edges are taken as they are
 * (RGBX_LOOPS_KEEP). No entry point uses float atomics, scratch or LDS; every sum runs in a fixed order (slots of a
 * lane group in slot order, lane groups, heads of a group, head chunks ascending, hub-row chunks in chunk order): two
 * runs are bit-identical. Nothing per edge passes between forward and backward. */

/* Slot weights of aggr="mean" per (target, relation):  w[p] = 1.0f / (float)#{p' in the row of p : etype[p'] ==
 * etype[p]}  (the `aggr='mean'` of the masked propagate above). The count is integer arithmetic and exact; no [N, R]
 * table is formed, R > 0 is only validated. `split`: hub rows are cut into the plan's chunks, each of which is counted
 * against its whole row (split->partial is not touched). The same call on the transposed CSR gives no meaningful
 * weights: take w_t[q] = w[t2f[q]]. */
int rgbx_rgcn_slot_norm_f32(const int32_t* rowptr, const int32_t* etype, float* w, int64_t N, int R,
                            const rgbx_row_split_t* split, rgbx_stream_t stream);

/* 1 if the mix kernels take B bases of C channels (1 <= B <= 64; C as rgbx_gine_supported), else 0. */
int rgbx_rgcn_mix_supported(int B, int C);

/* Forward over the target-grouped CSR, h [N_src, B*C], out [N, C]:
 *   out[i,:] = y0[i,:] + sum_p sum_b a[p,b] * h[col[p], b, :]
 * y0 [N, C] is optional (NULL: zeros) and carries the dense root + bias term, so that out is written once; out must
 * alias neither h nor y0. A row without slots stores y0 (or zeros). `w` [nnz] is required (ones: aggr="add").
 * split->partial holds n_chunks * C floats; y0 rides on a row's first chunk. */
int rgbx_rgcn_mix_fwd_f32(const int32_t* rowptr, const int32_t* col, const int32_t* etype, const float* w,
                          const float* comp, const float* h, int64_t ldh, const float* y0, int64_t ldy, float* out,
                          int64_t ldo, int64_t N, int R, int B, int C, const rgbx_row_split_t* split,
                          rgbx_stream_t stream);

/* Backward, source side, over the TRANSPOSED CSR (rows = sources j, col_t = targets i; etype_t / w_t per transposed
 * slot):  g_h[j,b,:] = sum_q a[q,b] * gout[col_t[q],:],  g_h [N, B*C]. A source without out-edges stores zeros.
 * split->partial holds n_chunks * B * C floats. */
int rgbx_rgcn_mix_bwd_src_f32(const int32_t* rowptr_t, const int32_t* col_t, const int32_t* etype_t, const float* w_t,
                              const float* comp, const float* gout, int64_t ldg, float* g_h, int64_t ldgh, int64_t N,
                              int R, int B, int C, const rgbx_row_split_t* split, rgbx_stream_t stream);

/* Backward, coefficient side, over the forward CSR:  d[p,b] = w[p] * <h[col[p],b,:], gout[i,:]>,  d [nnz, B]
 * contiguous, one store per (slot, head) and no sum over slots; g_comp[r,:] is the sum of d[p,:] over the slots of
 * relation r, which the caller takes with rgbx_spmm_csr_f32 over the slots grouped by relation (a fixed-order sum).
 * `split` only balances the hub rows (split->partial is not touched). */
int rgbx_rgcn_mix_bwd_coef_f32(const int32_t* rowptr, const int32_t* col, const float* w, const float* h, int64_t ldh,
                               const float* gout, int64_t ldg, float* d, int64_t N, int R, int B, int C,
                               const rgbx_row_split_t* split, rgbx_stream_t stream);

/* ---- FiLMConv / GNN-FiLM: the target modulates every message per channel, before the nonlinearity ------------------- */

/* FiLMConv.forward [PyG] loops over the relations, masks the edge list and propagates once per relation with
 * `message = act(gamma_i * x_j + beta_i)` on [E_r, C] tensors (Brockschmidt, "GNN-FiLM: Graph Neural Networks with
 * Feature-wise Linear Modulation"). The reference's zoo has no such layer. Here the dense products come first, with R
 * relations and C channels:
 *   h  = x @ [W_0 | ... | W_{R-1}]           viewed [N*R, C]:   row j*R + r = the message row of source j under r
 *   fb = [film_0(x) | ... | film_{R-1}(x)]   viewed [N*R, 2C]:  row i*R + r = beta_r[i] | gamma_r[i]   (beta FIRST)
 * (each its own pointer and leading dimension: column blocks of wider matrices are taken as they are; `gofs` >= C is
 * the offset of gamma inside a film row, C for the layout above, and the leading dimension of fb is >= gofs + C, so
 * that the column block [a, b) of a wider fb is the view that starts at beta's column a with gofs = the full C) and
 * ONE pass over the edges forms, for the edge j -> i of relation r in slot p,
 *   z_p = fmaf(gamma_r[i], h[j*R + r], beta_r[i]),   m_p = act(z_p),   act: 0 = identity, 1 = relu.
 * The edges are taken as they are (RGBX_LOOPS_KEEP). No entry point uses float atomics, scratch or LDS; nothing per
 * edge is saved: both backward passes recompute z with the same fmaf, so the relu mask is the forward's (relu'(0) = 0).
 * Every sum runs in a fixed order (slots of a lane group in slot order, lane groups, hub-row chunks in chunk order) and
 * every output row is written: two runs are bit-identical. N * R >= 2^31 is refused with RGBX_E_RANGE. */

/* 1 if the kernels take C channels (the widths of rgbx_transformer_supported(1, C)), else 0. */
int rgbx_film_supported(int C);

/* Forward over the target-grouped CSR, out [N, C]:
 *   out[i,:] = y0[i,:] + sum_p w[p] * act(z_p)
 * `etype` / `w` [nnz]: the relation and the weight of every slot (w: the mean weights of rgbx_rgcn_slot_norm_f32, or
 * ones for aggr="add"); the film row (i, etype[p]) is read from device memory per slot. etype == NULL is the
 * single-relation call (R must be 1, w is ignored): the weight is 1.0f / (float)len from rowptr with mean != 0, else 1,
 * and the target's film row stays in registers. y0 [N, C] is optional (NULL: zeros) and carries the dense skip term,
 * added after the slot loop so that out is written once; out must alias none of h, fb, y0. A row without slots stores
 * y0 (or exact zeros). split->partial holds n_chunks * C floats; y0 rides on a row's first chunk and the partials are
 * added in chunk order. */
int rgbx_film_fwd_f32(const int32_t* rowptr, const int32_t* col, const int32_t* etype, const float* w, const float* h,
                      int64_t ldh, const float* fb, int64_t ldfb, int64_t gofs, const float* y0, int64_t ldy, float* out,
                      int64_t ldo, int64_t N, int R, int C, int mean, int act, const rgbx_row_split_t* split,
                      rgbx_stream_t stream);

/* Backward, source side, over the relation-expanded TRANSPOSED CSR of N*R rows (row j*R + r = the out-edges of j with
 * relation r, col_t = targets i; with R = 1 the plain transposed CSR):
 *   g_h[j*R + r,:] = sum_q w_q * gamma_r[i_q] (.) act'(z_q) (.) gout[i_q,:],   g_h [N*R, C].
 * The slot weight w_q is w_t[q] (in this CSR's slot order), or with w_t == NULL 1.0f / (float)indeg(i_q) read from the
 * forward rowptr `deg_rowptr` [N + 1], or 1 with both NULL. A row without slots stores zeros. split->partial holds
 * n_chunks * C floats. */
int rgbx_film_bwd_src_f32(const int32_t* rowptr_x, const int32_t* col_t, const float* w_t, const int32_t* deg_rowptr,
                          const float* h, int64_t ldh, const float* fb, int64_t ldfb, int64_t gofs, const float* gout,
                          int64_t ldg, float* g_h, int64_t ldgh, int64_t N, int R, int C, int act,
                          const rgbx_row_split_t* split, rgbx_stream_t stream);

/* Backward, film side, over the relation-expanded FORWARD CSR of N*R rows (row i*R + r = the in-edges of i with
 * relation r, col_e = sources j; with R = 1 the plain forward CSR), g_fb [N*R, gofs + C] in fb's layout (the same gofs;
 * columns between the two blocks are not touched):
 *   g_fb[i*R + r, :C] = w (.) gout[i,:] (.) sum_p act'(z_p)          (g_beta)
 *   g_fb[i*R + r, gofs:gofs+C] = w (.) gout[i,:] (.) sum_p act'(z_p) (.) h[col_e[p]*R + r,:]   (g_gamma)
 * with ONE weight per row, w = 1.0f / (float)len with mean != 0 (the bits of the per-slot mean weights), else 1. A row
 * without slots stores zeros. split->partial holds n_chunks * 2C floats: a chunk's record is (g_beta | g_gamma). */
int rgbx_film_bwd_film_f32(const int32_t* rowptr_e, const int32_t* col_e, const float* h, int64_t ldh, const float* fb,
                           int64_t ldfb, int64_t gofs, const float* gout, int64_t ldg, float* g_fb, int64_t ldgfb,
                           int64_t N, int R, int C, int mean, int act, const rgbx_row_split_t* split,
                           rgbx_stream_t stream);

/* ---- GMMConv / MoNet: a trained Gaussian mixture over the pseudo-coordinates of every edge --------------------------- */

/* Every edge j -> i carries D pseudo-coordinates, e [nnz, D] with one row PER SLOT of the target-grouped CSR (its own
 * pointer and leading dimension). GMMConv.message [PyG] (separate_gaussians=False) forms, per edge,
 * `gaussian = -0.5 * (edge_attr.view(E, 1, D) - self.mu.view(1, K, D)).pow(2)`,
 * `gaussian = gaussian / (EPS + self.sigma.view(1, K, D).pow(2))`, `gaussian = torch.exp(gaussian.sum(dim=-1))` and
 * returns `(x_j.view(E, K, M) * gaussian.view(E, K, 1)).sum(dim=-2)`: an [E, K, D] and an [E, K, M] tensor (Monti et al.,
 * "Geometric deep learning on graphs and manifolds using mixture model CNNs"). The reference's zoo has no such layer.
 * Here the dense product comes first (h = x @ g viewed as [N, K, M], k-major columns) and ONE pass over the edges
 * evaluates, in registers,
 *   gauss[p, k] = exp(-0.5 * sum_d (e[p,d] - mu[k,d])^2 * inv[k,d]),   inv[k,d] = 1 / (1e-15 + sigma[k,d]^2)
 * from `mu` and `sigma` [K, D] (row-major, contiguous) in DEVICE memory, so a captured launch follows the parameters an
 * optimizer moves; no [nnz, K] coefficient table passes from forward to backward. The edges are taken as they are
 * (RGBX_LOOPS_KEEP). No entry point uses float atomics, scratch or LDS; every sum runs in a fixed order (slots of a lane
 * group in slot order, lane groups, heads of a group, head chunks ascending, hub-row chunks in chunk order; the parameter
 * gradients over slot ranges of a fixed length, the ranges in ascending order): two runs are bit-identical. */

/* 1 if the kernels take K Gaussian kernels of M channels over D coordinates (1 <= K <= 64; M as rgbx_gine_supported;
 * 1 <= D <= 8), else 0. Anything else is refused with RGBX_E_SHAPE before any launch. */
int rgbx_gmm_supported(int K, int M, int D);

/* Forward over the target-grouped CSR, h [N_src, K*M], out [N, M]:
 *   out[i,:] = y0[i,:] + rs[i] * sum_p sum_k gauss[p,k] * h[col[p], k, :]
 * `rs` [N] is optional: 1 / max(indeg, 1) gives aggr="mean", NULL the sum. y0 [N, M] is optional (NULL: zeros) and
 * carries the dense root + bias term, so that out is written once; out must alias none of h, y0, e. A row without slots
 * stores y0 (or zeros). split->partial holds n_chunks * M floats; y0 rides on a row's first chunk. */
int rgbx_gmm_fwd_f32(const int32_t* rowptr, const int32_t* col, const float* e, int64_t lde, const float* mu,
                     const float* sigma, const float* rs, const float* h, int64_t ldh, const float* y0, int64_t ldy,
                     float* out, int64_t ldo, int64_t N, int K, int M, int D, const rgbx_row_split_t* split,
                     rgbx_stream_t stream);

/* Backward, source side, over the TRANSPOSED CSR (rows = sources j, col_t = targets i, t2f [nnz] = the forward slot of
 * every transposed slot, through which the e row is gathered; w_t [nnz] = rs[col_t[q]] for the mean, NULL for the sum):
 *   g_h[j,k,:] = sum_q w_t[q] * gauss[t2f[q], k] * gout[col_t[q], :],  g_h [N, K*M].
 * A source without out-edges stores zeros. split->partial holds n_chunks * K * M floats. */
int rgbx_gmm_bwd_src_f32(const int32_t* rowptr_t, const int32_t* col_t, const int32_t* t2f, const float* w_t,
                         const float* e, int64_t lde, const float* mu, const float* sigma, const float* gout,
                         int64_t ldg, float* g_h, int64_t ldgh, int64_t N, int K, int M, int D,
                         const rgbx_row_split_t* split, rgbx_stream_t stream);

/* Bytes of workspace rgbx_gmm_bwd_edge_f32 needs: the table s [nnz, K] and one record of 2 K D floats per slot range of
 * the parameter reduction. */
int rgbx_gmm_bwd_edge_workspace_bytes(int64_t nnz, int K, int D, size_t* bytes);

/* Backward, edge side, over the forward CSR. With s[p,k] = rs[i] * gauss[p,k] * <h[col[p],k,:], gout[i,:]> (stored per
 * (slot, head) in the workspace) and t[p,k,d] = (e[p,d] - mu[k,d]) * inv[k,d]:
 *   g_e[p,d]     = -sum_k s[p,k] * t[p,k,d]                     one row per slot, [nnz, D] with leading dimension ldge
 *   g_mu[k,d]    =  sum_p s[p,k] * t[p,k,d]                     [K, D] contiguous
 *   g_sigma[k,d] =  sum_p s[p,k] * t[p,k,d]^2 * sigma[k,d]      [K, D] contiguous
 * g_e NULL skips the first, g_mu and g_sigma NULL (both or neither) the other two; all three NULL launches nothing. The
 * sums over p run per slot range (a fixed number of consecutive slots, a function of nnz alone), per lane in slot
 * order, and the ranges are added in ascending order. `split` only balances the hub rows (split->partial is not
 * touched). `workspace`: rgbx_gmm_bwd_edge_workspace_bytes(nnz, K, D) bytes, 4-byte aligned. nnz = 0 stores zeros in
 * g_mu and g_sigma. */
int rgbx_gmm_bwd_edge_f32(const int32_t* rowptr, const int32_t* col, const float* e, int64_t lde, const float* mu,
                          const float* sigma, const float* rs, const float* h, int64_t ldh, const float* gout,
                          int64_t ldg, float* g_e, int64_t ldge, float* g_mu, float* g_sigma, void* workspace,
                          size_t workspace_bytes, int64_t N, int64_t nnz, int K, int M, int D,
                          const rgbx_row_split_t* split, rgbx_stream_t stream);

/* The MoNet paper's pseudo-coordinates of a graph without edge attributes, u [nnz, 2] contiguous in forward slot order:
 *   u[p] = (1 / sqrt(1 + indeg(col[p])), 1 / sqrt(1 + indeg(i)))  for slot p of row i, indeg(v) = rowptr[v+1] - rowptr[v]
 * (the paper's `deg^-1/2` coordinates, for which PyG's examples apply `T.Cartesian` / a degree transform on the host).
 * The + 1 keeps a source without in-edges finite. Needs a square CSR (every col[p] < N). `split`: hub rows are cut
 * into the plan's chunks (split->partial is not touched). */
int rgbx_gmm_degree_pseudo_f32(const int32_t* rowptr, const int32_t* col, float* u, int64_t N,
                               const rgbx_row_split_t* split, rgbx_stream_t stream);

/* ---- Softmax aggregation (GENConv / DeeperGCN): per-channel softmax over the in-edges at a trained temperature ----- */

/* For an edge j -> i (p = its slot in the target-grouped CSR), with messages m [N, C] (its own pointer and leading
 * dimension) and a temperature t in DEVICE memory (t_stride = 0: one float for every channel; t_stride = 1: t [C]):
 *   z_p[c]     = t[c] m[j,c]
 *   alpha_p[c] = exp(z_p[c] - lse[i,c]),   lse[i,c] = log sum_p exp(z_p[c])
 *   out[i,c]   = sum_p alpha_p[c] m[j,c]
 * (SoftmaxAggregation / GENConv(aggr="softmax") [PyG]; Li et al., "DeeperGCN: All You Need to Train Deeper GCNs". The
 * reference's zoo has no GENConv.) t = 0 gives the mean, t -> inf the maximum, t < 0 a soft minimum: the running
 * maximum is taken of z, so no intermediate overflows whatever t m is. The temperature is read by the kernels, never by
 * the host: a captured launch follows a parameter that an optimizer moves. The edges are taken as they are
 * (RGBX_LOOPS_KEEP): a row WITHOUT slots stores exact zeros in `out` and 0 in `lse`; a source without out-edges gets a
 * zero g_m row. Every output row is written. Nothing per edge is stored: the backward recomputes alpha from `lse`. No
 * entry point uses float atomics: two runs are bit-identical. */

/* 1 if the kernels take C channels (the widths of rgbx_resgated_supported), else 0. */
int rgbx_softmax_aggr_supported(int C);

/* Forward over the target-grouped CSR. `lse` ([N, C], leading dimension ldl) may be NULL (the inference form: the same
 * bits in `out`). `split`: hub rows as in rgbx_gatv2_fwd_f32; split->partial holds n_chunks * 3*C floats (acc | max |
 * den per chunk), merged in chunk order. */
int rgbx_softmax_aggr_fwd_f32(const int32_t* rowptr, const int32_t* col, const float* m, int64_t ldm, const float* t,
                              int t_stride, float* out, int64_t ldo, float* lse, int64_t ldl, int64_t N, int C,
                              const rgbx_row_split_t* split, rgbx_stream_t stream);

/* Floats of caller scratch rgbx_softmax_aggr_bwd_f32 needs for its g_t records, for this N and split plan. */
int rgbx_softmax_aggr_gt_partial_floats(int64_t N, int C, const rgbx_row_split_t* split, int64_t* count);

/* Backward over the TRANSPOSED CSR (rows = sources j, col_t = targets i), with d = m[j,:] - out[i,:]:
 *   g_m[j,c] = sum_p alpha_p gout[i,c] (1 + t[c] d[c]),    g_t[c] = sum over all edges of alpha gout[i,c] d[c]^2.
 * g_m is always formed. g_t ([C], per channel whatever t_stride is; a scalar temperature's gradient is its sum) may be
 * NULL: no record is then kept and no reduction runs. Otherwise `gt_partial` holds n_gt_partial >=
 * rgbx_softmax_aggr_gt_partial_floats floats: one [C] record per workgroup, added in record order.
 * split->partial holds n_chunks * C floats. */
int rgbx_softmax_aggr_bwd_f32(const int32_t* rowptr_t, const int32_t* col_t, const float* m, int64_t ldm, const float* t,
                              int t_stride, const float* out, int64_t ldo, const float* lse, int64_t ldl,
                              const float* gout, int64_t ldg, float* g_m, int64_t ldgm, float* g_t, float* gt_partial,
                              int64_t n_gt_partial, int64_t N, int C, const rgbx_row_split_t* split,
                              rgbx_stream_t stream);

/* ---- dense layers on the MFMA units -------------------------------------------------------- */

/* Scratch bytes for rgbx_gemm_tn_f32 (split-K partial tiles + partial column sums). */
int rgbx_gemm_tn_workspace_bytes(int64_t K, int64_t M, int64_t N, size_t* bytes);

/* C[M,N] = alpha * A^T B, A [K,M] (lda), B [K,N] (ldb), fp32 row-major, K = node count (huge),
 * M,N = feature widths. Split-K over the whole chip on v_mfma_f32_32x32x2_f32 (exact fp32), partials
 * reduced in slab order (bitwise reproducible). This is dW = dY^T X of every Linear on the path.
 * Alignment: when A and B are 16-byte aligned with lda % 4 == 0 and ldb % 4 == 0, rows are read in whole 16-byte groups —
 * for M % 4 != 0 / N % 4 != 0 the last group of a row ends in the row's padding (columns [M, lda) / [N, ldb)), which
 * must therefore be readable memory for EVERY row, the last included (any finite or non-finite contents: those products
 * are never stored). F = 1433 feature rows kept at a stride of 1436 floats take this path; rows that are not 16-byte
 * aligned take a 4-byte path several times slower.
 * `a_colsum` ([M], optional): also receives the column sums of A (unscaled) — the bias gradient
 * db = sum_rows dY, taken from the A tiles the kernel stages anyway. */
int rgbx_gemm_tn_f32(const float* A, int64_t lda, const float* B, int64_t ldb, float* C, int64_t ldc,
                     float* a_colsum, int64_t K, int64_t M, int64_t N, float alpha, void* workspace,
                     size_t workspace_bytes, rgbx_stream_t stream);

/* rgbx_gemm_tn_f32 with A = BatchNorm's input gradient, formed as the A tiles are staged instead of being written by
 * rgbx_bn_bwd_apply_f32 and read back: C = alpha * A'^T B and a_colsum = column sums of A' with
 *   A'[r,c] = (G[r,c] - ca[c] - (X[r,c] - mean[c]) * rstd[c] * cb[c]) * ck[c]
 * (G [K,M] = the gradient of BatchNorm's output, X [K,M] its input, the five [M] vectors as for rgbx_bn_bwd_apply_f32).
 * Same slabs, MFMA order and reduce launches as rgbx_gemm_tn_f32 and the same arithmetic per element as the apply
 * kernel: the results are those of the two-launch sequence, bit for bit. Workspace: rgbx_gemm_tn_workspace_bytes.
 * 16-byte path only: G, X and B 16-byte aligned with ldg, ldx, ldb multiples of 4, else RGBX_E_ALIGN (the caller then
 * runs rgbx_bn_bwd_apply_f32 + rgbx_gemm_tn_f32). */
int rgbx_gemm_tn_bn_bwd_f32(const float* G, int64_t ldg, const float* X, int64_t ldx, const float* mean,
                            const float* rstd, const float* ca, const float* cb, const float* ck, const float* B,
                            int64_t ldb, float* C, int64_t ldc, float* a_colsum, int64_t K, int64_t M, int64_t N,
                            float alpha, void* workspace, size_t workspace_bytes, rgbx_stream_t stream);

/* rgbx_gemm_tn_f32 over the rows of an ascending int32 list `rows` ([n_rows], each in [0, K)), for an A whose other
 * rows are all zero (the loss gradient outside the rows the loss selects): only the listed rows of A and B are read.
 * The K-slabs are those of rgbx_gemm_tn_f32 on K rows and each multiplies the list entries inside its own row range,
 * in list order, so the non-zero products are added in the order of the full product. Workspace:
 * rgbx_gemm_tn_workspace_bytes(K, M, N). 16-byte path only (A, B aligned, lda, ldb multiples of 4), else
 * RGBX_E_ALIGN; K must fit int32. */
int rgbx_gemm_tn_rows_f32(const float* A, int64_t lda, const float* B, int64_t ldb, const int32_t* rows,
                          int64_t n_rows, float* C, int64_t ldc, float* a_colsum, int64_t K, int64_t M, int64_t N,
                          float alpha, void* workspace, size_t workspace_bytes, rgbx_stream_t stream);

/* ---- BatchNorm1d over the node axis --------------------------------------------------------- */

/* Doubles of scratch the two column-reduction entry points need. */
int rgbx_bn_scratch_doubles(int64_t N, int64_t d, int64_t* count);

/* sums[0,c] = sum_r x[r,c], sums[1,c] = sum_r x[r,c]^2 (fp64 accumulation; [2,d] doubles, device).
 * The caller forms mean / biased variance (and, in a node-partitioned run, all-reduces `sums` first). */
int rgbx_bn_stats_f32(const float* x, int64_t ldx, int64_t N, int64_t d, double* sums, double* scratch,
                      int64_t scratch_doubles, rgbx_stream_t stream);

/* Between the raw sums and the apply pass, one launch. `packed` = [sum x (d), sum x^2 (d), row count (1)] in fp64,
 * after any cross-rank reduction. Produces mean, rstd = 1/sqrt(biased var + eps), the training forward's affine map
 * scale = weight * rstd, shift = bias - mean * scale, and (running_* not NULL) the nn.BatchNorm1d update
 * running = (1 - momentum) * running + momentum * (mean | unbiased var). */
int rgbx_bn_finalize_f32(const double* packed, const float* weight, const float* bias, float eps, float momentum,
                         float* running_mean, float* running_var, float* mean, float* rstd, float* scale,
                         float* shift, int64_t d, rgbx_stream_t stream);

/* Eval forwards: the BatchNorm1d BEHIND a linear layer in eval mode (running statistics; models/gcn.py:27-28 under
 * model.eval(), itexperiments.py:619-622) is a per-column affine map of that layer's output, i.e. the same layer with
 * rescaled weights. One launch makes the operands the fused kernels read:
 *   scale[n] = gamma[n] / sqrt(running_var[n] + eps),  shift[n] = beta[n] - running_mean[n] * scale[n]
 *   wt[k, n]  = W[n, k]  * scale[n]      (W [Nout, K] row-major -> W'^T [K, Nout], the [K, Nout] operand layout)
 *   wrt[k, n] = Wr[n, k] * scale[n]      (optional second weight: the root term of SAGEConv / my_SAGEConv)
 *   b_out[n]  = (bias[n] + bias2[n]) * scale[n] + shift[n]      (bias, bias2, b_out optional)
 * gamma == beta == running_mean == running_var == NULL: no BatchNorm (scale 1, shift 0), i.e. the plain transpose
 * of the model's last layer. Replaces ~8 [out]-sized vector launches and two transposes per layer and eval forward. */
int rgbx_fold_bn_linear_f32(const float* W, int64_t ldw, const float* Wr, int64_t ldwr, const float* bias,
                            const float* bias2, const float* gamma, const float* beta, const float* running_mean,
                            const float* running_var, float eps, float* wt, float* wrt, float* b_out, int64_t Nout,
                            int64_t K, rgbx_stream_t stream);

/* Backward counterpart: ca = glob[0]/n, cb = glob[1]/n, ck = weight * rstd for rgbx_bn_bwd_apply_f32 (`glob` = the
 * [2, d] sums of rgbx_bn_bwd_reduce_f32 after any cross-rank reduction, `count` = device pointer to n), and the
 * parameter gradients of this rank, g_bias = local[0], g_weight = local[1]. */
int rgbx_bn_bwd_finalize_f32(const double* glob, const double* local, const double* count, const float* weight,
                             const float* rstd, float* ca, float* cb, float* ck, float* g_weight, float* g_bias,
                             int64_t d, rgbx_stream_t stream);

/* y[r,c] = x[r,c] * scale[c] + shift[c] — BatchNorm's normalise+affine with
 * scale = gamma * rstd, shift = beta - mean * scale (training or running statistics alike). */
int rgbx_affine_cols_f32(const float* x, int64_t ldx, const float* scale, const float* shift, float* y,
                         int64_t ldy, int64_t N, int64_t d, rgbx_stream_t stream);

/* sums[0,c] = sum_r gy[r,c], sums[1,c] = sum_r gy[r,c] * xhat[r,c], xhat = (x - mean) * rstd. */
int rgbx_bn_bwd_reduce_f32(const float* gy, int64_t ldg, const float* x, int64_t ldx, const float* mean,
                           const float* rstd, int64_t N, int64_t d, double* sums, double* scratch,
                           int64_t scratch_doubles, rgbx_stream_t stream);

/* gx[r,c] = (gy[r,c] - ca[c] - xhat[r,c] * cb[c]) * ck[c]
 * (ca = sum gy / n, cb = sum gy*xhat / n, ck = gamma * rstd). */
int rgbx_bn_bwd_apply_f32(const float* gy, int64_t ldg, const float* x, int64_t ldx, const float* mean,
                          const float* rstd, const float* ca, const float* cb, const float* ck, float* gx,
                          int64_t ldgx, int64_t N, int64_t d, rgbx_stream_t stream);

/* ---- loss / metrics on masked rows ---------------------------------------------------------- */

/* Doubles of device scratch rgbx_masked_nll_fwd_f32 needs (3 per workgroup). */
int rgbx_masked_nll_scratch_doubles(int64_t N, int want_accuracy, int64_t* count);

/* stats[0] = sum over selected rows of -logp[i, y[i]]; stats[1] = number of selected rows;
 * stats[2] = number of selected rows whose first arg-max equals y[i] (only if want_accuracy).
 * A row is selected when mask == NULL or mask[i] != 0, and 0 <= y[i] < C. `stats` = 3 doubles (device).
 * Per-workgroup sums go to `scratch` and are added in workgroup order (reproducible; no atomics).
 * logp is [N, C] (ld). */
int rgbx_masked_nll_fwd_f32(const float* logp, int64_t ld, const int64_t* y, const uint8_t* mask,
                            int64_t N, int64_t C, double* stats, double* scratch,
                            int64_t scratch_doubles, int want_accuracy, rgbx_stream_t stream);

/* grad[i,c] = -scale[0] if row i is selected and c == y[i], else 0, for every (i, c): the gradient
 * of scale * stats[0] w.r.t. logp. `scale` is a device scalar (no host sync). */
int rgbx_masked_nll_bwd_f32(const int64_t* y, const uint8_t* mask, int64_t N, int64_t C,
                            const float* scale, float* grad, int64_t ldg, rgbx_stream_t stream);

/* The same loss taken from the LOGITS (cross-entropy = NLLLoss(log_softmax(z)), models/gcn.py:31 +
 * itexperiments.py:400,429): stats as rgbx_masked_nll_fwd_f32 with -logp[i, y_i] = logsumexp(z_i) - z[i, y_i]
 * and the arg-max taken on z (same as on log_softmax(z)); log-softmax is never written out.
 * Scratch: rgbx_masked_nll_scratch_doubles(N, 1). */
int rgbx_masked_ce_fwd_f32(const float* logits, int64_t ld, const int64_t* y, const uint8_t* mask, int64_t N,
                           int64_t C, double* stats, double* scratch, int64_t scratch_doubles,
                           rgbx_stream_t stream);

/* The same statistics from BLOCKED logits (+ bias[c], optional): element (i, c) at logits + (c / blk_cols) * blk_stride
 * + i * blk_cols + c % blk_cols, the layout a node-partitioned run's exchange delivers (rgbx_fused_layer_t) — the eval
 * forward's loss straight from the received column slices (new capability: the reference is single-device,
 * itexperiments.py:246; the arithmetic is itexperiments.py:624-626 on models/gcn.py:29-31). Only the selected rows are
 * read. C % 4 == 0, C <= 256, blk_cols % 4 == 0 dividing C. */
int rgbx_masked_ce_fwd_blocked_f32(const float* logits, int64_t blk_cols, int64_t blk_stride, const float* bias,
                                   const int64_t* y, const uint8_t* mask, int64_t N, int64_t C, double* stats,
                                   double* scratch, int64_t scratch_doubles, rgbx_stream_t stream);

/* grad[i,c] = scale[0] * (softmax(z_i)[c] - [c == y[i]]) for selected rows, 0 otherwise: the gradient of
 * scale * stats[0] w.r.t. the logits, one pass. `scale` is a device scalar. */
int rgbx_masked_ce_bwd_f32(const float* logits, int64_t ld, const int64_t* y, const uint8_t* mask, int64_t N,
                           int64_t C, const float* scale, float* grad, int64_t ldg, rgbx_stream_t stream);

/* ---- edge-list ingest (before the path: rd2pd.py:92-93, itexperiments.py:235-238) ------------ */

/* Sorted set of the pairs (row[e], col[e]) — with `mirror` != 0 also of their reverses (col[e], row[e]): coalesce and
 * to_undirected. Two steps because the caller owns the output and its size is only known on the device:
 *   1. rgbx_coalesce_keys_i64 writes the distinct keys row * N + col in ascending order to keys_out (capacity
 *      M = mirror ? 2E : E) and counts[0] = their number, counts[1] = number of endpoints outside [0, N) (those are
 *      clamped; a caller that sees counts[1] != 0 must discard the result). counts: 2 x uint64 on the device.
 *   2. after reading counts[0] back and allocating int64 [2, count], rgbx_split_edge_keys_i64 writes the rows
 *      (cap = the caller's capacity; min(cap, counts[0]) pairs are written).
 * Workspace: rgbx_coalesce_workspace_bytes(E, N, mirror). Self-loops are kept (once), as both PyG helpers do. */
int rgbx_coalesce_workspace_bytes(int64_t E, int64_t N, int mirror, size_t* bytes);
int rgbx_coalesce_keys_i64(const int64_t* row, const int64_t* col, int64_t E, int64_t N, int mirror,
                           uint64_t* keys_out, uint64_t* counts, void* workspace, size_t workspace_bytes,
                           rgbx_stream_t stream);
int rgbx_split_edge_keys_i64(const uint64_t* keys, const uint64_t* counts, int64_t cap, int64_t N, int64_t* out_row,
                             int64_t* out_col, rgbx_stream_t stream);

/* HOST function (the one entry point that takes a host pointer and runs on the CPU, synchronously): perm[0..n) =
 * list(range(n)) after Python's `random.seed(seed); random.shuffle(...)`, bit for bit (MT19937 seeded by init_by_array over
 * the 32-bit words of |seed|; randbelow by rejection over getrandbits(bit_length)) — the shuffle behind the reference's split
 * masks (utils/mask.py:66-102; itexperiments.py:210-215). n < 2^32. */
int rgbx_py_random_shuffle_i64(int64_t seed, int64_t n, int64_t* perm);

/* ---- halo pack / unpack (multi-GPU node partition) ----------------------------------------- */

/* dst[r,:] = src[idx[r],:] for r in [0,n) — pack boundary rows into a send buffer. */
int rgbx_gather_rows_f32(const float* src, int64_t lds, const int32_t* idx, int64_t n, int64_t d,
                         float* dst, int64_t ldd, rgbx_stream_t stream);

/* dst[idx[r],:] += src[r,:] for r in [0,n); idx entries must be unique (no atomics). */
int rgbx_scatter_add_rows_f32(const float* src, int64_t lds, const int32_t* idx, int64_t n,
                              int64_t d, float* dst, int64_t ldd, rgbx_stream_t stream);

/* Measurement aid, not on the path: dst[0:n] = src[0:n] by `workgroups` workgroups only, i.e. at a rate the caller
 * calibrates — the stand-in for an exchange's memory traffic when ONE GPU emulates a rank of a partitioned job
 * (bench.py --emulate-rank P --emulate-contend GBS). nontemporal != 0: loads and stores that do not allocate in the caches
 * (the optimistic bracket of what a real exchange's DMA traffic does to them). n % 4 == 0, 16-byte aligned pointers. */
int rgbx_paced_copy_f32(const float* src, float* dst, int64_t n, int workgroups, int nontemporal, rgbx_stream_t stream);

/* ---- FAGCN: FAConv (signed tanh attention on the GCN-normalised graph) ----------------------- */

/* For an edge j -> i of the target-grouped CSR (graph mode add-remaining-self-loops, w = gcn_norm weights):
 *   a = tanh(al_j + ar_i),  c = kappa a w,  out[i,:] = sum_j c x[j,:] + eps x0[i,:]
 * with al = x att_l, ar = x att_r interleaved in alr [N, 2] (8-byte aligned) and kappa = keep / (1 - p_drop) in
 * training mode (FAConv [PyG], reference models/fagcn.py). `seed` points to two 32-bit words ON THE DEVICE; NULL
 * selects inference mode. A slot's keep is a hash of (seed, forward CSR slot): the backward passes recompute it and no
 * per-edge tensor is stored. Rows are read in fragments of vec = 4 / 2 / 1 floats for C % 4 == 0 / C % 2 == 0 / odd C:
 * every row pointer must be vec * 4-byte aligned and every leading dimension a multiple of vec (RGBX_E_ALIGN).
 * `split` (hub rows, as rgbx_spmm_csr_f32): split->partial holds n_chunks * (C + 1) floats, 16-byte aligned. */

/* 1 if the fused kernels take width C (any C <= 64, even C <= 128, C % 4 == 0 up to 256), else 0: the caller then
 * composes the layer from rgbx_faconv_edge_coef_f32, rgbx_spmm_csr_f32 and rgbx_faconv_edge_dot_f32. */
int rgbx_faconv_supported(int64_t C);

/* alr[r] = (<x[r,:], att_l>, <x[r,:], att_r>); any C. */
int rgbx_faconv_scores_f32(const float* x, int64_t ldx, const float* att_l, const float* att_r, float* alr, int64_t N,
                           int64_t C, rgbx_stream_t stream);

/* Forward: one gather pass. x0 == NULL skips the eps term. `out` must not alias x. */
int rgbx_faconv_fwd_f32(const int32_t* rowptr, const int32_t* col, const float* w, const float* x, int64_t ldx,
                        const float* alr, const float* x0, int64_t ldx0, float eps, float* out, int64_t ldo, int64_t N,
                        int64_t C, const uint32_t* seed, float p_drop, const rgbx_row_split_t* split,
                        rgbx_stream_t stream);

/* Backward, with q = kappa w (1 - a^2) and s = q <gout[i,:], x[j,:]>. Target side, over the forward CSR:
 * g_alr[i * 2 + 1] = sum_j s (the gradient of ar). */
int rgbx_faconv_bwd_dst_f32(const int32_t* rowptr, const int32_t* col, const float* w, const float* x, int64_t ldx,
                            const float* alr, const float* gout, int64_t ldg, float* g_alr, int64_t N, int64_t C,
                            const uint32_t* seed, float p_drop, const rgbx_row_split_t* split, rgbx_stream_t stream);

/* Source side, over the TRANSPOSED CSR (rows = sources j, col_t = targets i, w_t its gcn_norm weights), run AFTER the
 * target side: g_alr[j * 2] = sum_i s and
 *   g_x[j,:] = sum_i c gout[i,:] + g_alr[j * 2] att_l + g_alr[j * 2 + 1] att_r      (stored; not the eps term).
 * `t2f` ([E'], training mode): the forward CSR slot of every transposed slot. g_att_l / g_att_r are the rows of
 * g_alr^T x (rgbx_gemm_tn_f32). */
int rgbx_faconv_bwd_src_f32(const int32_t* rowptr_t, const int32_t* col_t, const float* w_t, const int32_t* t2f,
                            const float* x, int64_t ldx, const float* alr, const float* gout, int64_t ldg,
                            const float* att_l, const float* att_r, float* g_alr, float* g_x, int64_t ldgx, int64_t N,
                            int64_t C, const uint32_t* seed, float p_drop, const rgbx_row_split_t* split,
                            rgbx_stream_t stream);

/* Composed path: coef[p] = c and (q != NULL) q[p] = kappa w (1 - a^2) of every slot of a CSR. transposed == 0: rows
 * are targets (a = tanh(al[col] + ar[row])); != 0: rows are sources (a = tanh(al[row] + ar[col])). `slot` ([E'] or
 * NULL = identity): the forward slot that keys the dropout decision of slot p. */
int rgbx_faconv_edge_coef_f32(const int32_t* rowptr, const int32_t* col, const float* w, const int32_t* slot,
                              const float* alr, int transposed, int64_t N, const uint32_t* seed, float p_drop,
                              float* coef, float* q, rgbx_stream_t stream);

/* out[i * out_stride] = sum_{p in row i} q[p] <a[i,:], b[col[p],:]>; any C (one wave per row, no hub split). */
int rgbx_faconv_edge_dot_f32(const int32_t* rowptr, const int32_t* col, const float* q, const float* a, int64_t lda,
                             const float* b, int64_t ldb, float* out, int64_t out_stride, int64_t N, int64_t C,
                             rgbx_stream_t stream);

/* keep[p] = 1 where forward slot p survives the dropout of this seed. */
int rgbx_faconv_draws_u8(const uint32_t* seed, int64_t nnz, float p_drop, uint8_t* keep, rgbx_stream_t stream);

/* ---- neighbour sampling: fan-out mini-batches ------------------------------------------------ */

/* One hop over the target-grouped CSR (graph mode keep: no slot is added, duplicate edges are separate slots). Row g =
 * rows[r] (distinct global ids; an id outside [0, N) counts as a row without slots) has deg = rowptr[g + 1] - rowptr[g]
 * slots and keeps min(fanout, deg) of them (fanout = -1: all): the ones with the smallest 64-bit keys
 *   draw32(seed[0], seed[1], 0x082EFA98 + hop, g, t) << 32 | t,    t = slot - rowptr[g]   (draw32: csrc/rgbx_rng.h),
 * written in ascending slot order — a uniform draw without replacement that depends on (seed, hop, g, t) only. `seed`
 * points to two 32-bit words ON THE DEVICE. fanout == 0 or < -1: RGBX_E_ARG. */

/* Bytes of workspace that rgbx_sample_count over n_rows rows and rgbx_sample_frontier over n_cand candidates take (the
 * larger of the two). Asks rocPRIM for its temporary sizes: may return a hipError where no device is present. */
int rgbx_sample_workspace_bytes(int64_t n_rows, int64_t n_cand, int64_t N, size_t* bytes);

/* out_rowptr[0 .. n_rows] = exclusive scan of min(fanout, deg): out_rowptr[n_rows] is the hop's number of sampled
 * edges. class_rows (NULL, or 2 words): the number of rows with more than 64 slots up to 1024, and with more than 1024
 * — the row-length classes whose kernels rgbx_sample_pick may leave out when they are empty. */
int rgbx_sample_count(const int32_t* rowptr, int64_t N, const int32_t* rows, int64_t n_rows, int fanout,
                      int32_t* out_rowptr, int32_t* class_rows, void* workspace, size_t workspace_bytes,
                      rgbx_stream_t stream);

/* The row-length classes of rgbx_sample_pick: one kernel each. */
#define RGBX_SAMPLE_SHORT_ROWS 1 /* deg <= 64: 16 lanes per row */
#define RGBX_SAMPLE_WAVE_ROWS 2  /* 64 < deg <= 1024: a wave per row */
#define RGBX_SAMPLE_HUB_ROWS 4   /* deg > 1024: a workgroup per row */
#define RGBX_SAMPLE_ALL_ROWS 7

/* out_col[p] = the source and out_slot[p] = the CSR slot of every kept slot, p in [out_rowptr[r], out_rowptr[r + 1]) for
 * row r (out_rowptr from rgbx_sample_count with the same rows and fanout). `classes`: the kernels to launch
 * (RGBX_SAMPLE_*); a class that is left out must have no rows. */
int rgbx_sample_pick(const int32_t* rowptr, const int32_t* col, int64_t N, const int32_t* rows, int64_t n_rows,
                     int fanout, const uint32_t* seed, int hop, const int32_t* out_rowptr, int32_t* out_col,
                     int32_t* out_slot, int classes, rgbx_stream_t stream);

/* local_of [N] maps a global id to its id in the batch, -1 = not in the batch. The distinct candidates cand[0 .. n_cand)
 * with local_of < 0 get, in ascending global id, the local ids first_local, first_local + 1, ...; they are written to
 * new_ids (room for n_cand) and *count = how many (device word). Radix sort of the candidates + a scan: O(n_cand). */
int rgbx_sample_frontier(const int32_t* cand, int64_t n_cand, int32_t* local_of, int64_t N, int64_t first_local,
                         int32_t* new_ids, int32_t* count, void* workspace, size_t workspace_bytes,
                         rgbx_stream_t stream);

/* local_of[ids[i]] = first_local + i, or -1 for every i when first_local < 0 (the reset after a batch: it touches the
 * batch's entries only). ids distinct. */
int rgbx_sample_set_local(const int32_t* ids, int64_t n, int64_t first_local, int32_t* local_of, int64_t N,
                          rgbx_stream_t stream);

/* A hop's edges in batch ids, int64 as edge_index is: src[p] = local_of[col[p]], dst[p] = first_row + r for p in row r
 * (the rows of a hop hold consecutive local ids), e_id[p] = perm[slot[p]] (NULL perm: the slot itself; NULL e_id: skipped). */
int rgbx_sample_relabel(const int32_t* out_rowptr, int64_t n_rows, const int32_t* col, const int32_t* slot,
                        int64_t n_edges, const int32_t* local_of, int64_t N, const int32_t* perm, int64_t first_row,
                        int64_t* src, int64_t* dst, int64_t* e_id, rgbx_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* RGBX_HIP_H */
