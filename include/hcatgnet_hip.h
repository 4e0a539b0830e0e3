/*
 * hcatgnet_hip.h -- C ABI of libhcatgnet_hip.so (MI355X / gfx950 only).
 *
 * Drop-in boundary for ONE path of EdAguilarB/hcatgnet: the GCN message-passing
 * forward+backward that `GCN.forward` (reference model/gcn.py:54-76) runs through
 * torch_geometric.  The reference has no FFI layer of its own (pure Python on PyG); this ABI is
 * what a Python `nn.Module` binds with ctypes in place of
 *   - torch_geometric.nn.GCNConv            (call sites model/gcn.py:18-20, 27-29, 58, 62, 127, 131)
 *   - torch_geometric.nn.global_max_pool /
 *     global_mean_pool + torch.cat           (call sites model/gcn.py:65-66, 134-135)
 *   - the readout nn.Linear/LeakyReLU stack  (model/gcn.py:36-45, 70-71)
 *   - torch autograd through all of the above (utils/utils_model.py:65 `loss.backward()`)
 *
 * Conventions
 *   - every pointer is a DEVICE pointer unless the name ends in `_host`;
 *   - fp32 tensors are row-major contiguous; `edge_index` is int64 [2,E] contiguous
 *     (row 0 = source, row 1 = target: flow source->target, as in the reference data/rhcaa.py:160);
 *     `batch` is int64 [N], non-decreasing graph id; derived indices are int32;
 *   - the caller (PyTorch) owns every buffer; the library never allocates or frees device
 *     memory, keeps no global state, and only ENQUEUES work on the `stream` it is given
 *     (no internal synchronisation) -- safe under hipGraph capture and one-process-per-GPU DP;
 *   - every function returns an int: 0 = HCG_OK, negative = error (see below);
 *     nothing throws or exits across the ABI;
 *   - data-dependent violations that only the device can see (index out of range, unsorted
 *     `batch`, an edge that crosses graphs in blocked mode) are reported through the 4-word
 *     `status` array written by hcg_plan_build: the host wrapper reads it when it chooses to sync.
 */
#ifndef HCATGNET_HIP_H
#define HCATGNET_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define HCG_ABI_VERSION 1

#define HCG_OK 0
#define HCG_ERR_INVALID_ARG (-1)
#define HCG_ERR_WORKSPACE (-2)   /* caller-provided workspace too small */
#define HCG_ERR_UNSUPPORTED (-3) /* shape not supported by this entry point */
#define HCG_ERR_HIP_BASE (-1000) /* -1000 - hipError_t */

/* hcg_plan_build flags */
#define HCG_PLAN_GENERAL 0 /* device radix sort; any edge order, any graph size           */
#define HCG_PLAN_BLOCKED 1 /* edges grouped by graph (PyG collate order); per-graph waves */
#define HCG_PLAN_KEEP_STATUS 4 /* OR: do not zero `status` first (flags accumulate in a caller-owned,
                                  once-zeroed buffer until the caller reads and clears it) */
#define HCG_PLAN_PTRS_ONLY 2 /* OR with BLOCKED: only graph_ptr / edge_ptr / status (one launch);
                                all CSR outputs may be NULL -- enough for the hcg_fused_* kernels */

/* bits of status[0] written by hcg_plan_build */
#define HCG_STATUS_INDEX_RANGE 1   /* an edge_index entry outside [0,N)                  */
#define HCG_STATUS_BATCH_UNSORTED 2 /* batch not non-decreasing                           */
#define HCG_STATUS_BATCH_RANGE 4   /* a batch id outside [0,B)                           */
#define HCG_STATUS_EDGE_UNGROUPED 8 /* blocked mode: edges not grouped by graph / cross   */
#define HCG_STATUS_SHAPE_LIMIT 16  /* fused mode: a graph exceeds the tile the host chose */
#define HCG_STATUS_WEIGHTED_SELF_LOOP 32 /* explicit (i,i) edge together with edge_weight: PyG would take its
                                            weight as the node's loop weight; not implemented (loop weight = fill) */

/* activation codes of hcg_linear_* */
#define HCG_ACT_NONE 0
#define HCG_ACT_LEAKY 1

typedef void* hcg_stream_t; /* hipStream_t */
typedef struct hcg_reduce_job hcg_reduce_job; /* defined with the slab reduction below */

int hcg_version(void);
const char* hcg_error_string(int code);

/* ---- batch plan: gcn_norm + CSR/CSC + graph_ptr, ONCE per batch (reference recomputes
 *      gcn_norm every layer, every step: PyG GCNConv(cached=False)) ---------- */
/* workspace sizes of the any-shape entry points, ONE query: kind HCG_WS_PLAN (a, b, c = N, E, B; mode = the plan flags),
 * HCG_WS_LINEAR (M, D_in, D_out), HCG_WS_GCN_LAYER_BWD (N, F, D), HCG_WS_READOUT2 (B) */
#define HCG_WS_PLAN 0
#define HCG_WS_LINEAR 1
#define HCG_WS_GCN_LAYER_BWD 2
#define HCG_WS_READOUT2 3
#define HCG_WS_HEAD_DEEP 4   /* (B, D, C, mode = R): hcg_head_deep_fwd_bwd's workspace; 0 = shape not supported */
size_t hcg_general_workspace_bytes(int kind, int64_t a, int64_t b, int64_t c, int mode);

/* Outputs (all caller-allocated):
 *   graph_ptr [B+1]  node range of each graph                    (a9's `batch`)
 *   edge_ptr  [B+1]  edge range of each graph in CSR order (blocked mode; may be NULL in general)
 *   rowptr [N+1], col [E], eid [E]      incoming edges of each node, stable in input order:
 *                                       col = source id, eid = position in edge_index;
 *                                       col = -1 marks an explicit self-loop edge (i, i): as in PyG's
 *                                       add_remaining_self_loops it is not an edge of its own (every node
 *                                       gets exactly one self loop of weight `fill`) and is not counted in dinv
 *   rowptr_t [N+1], col_t [E], eid_t [E] outgoing edges (the transpose, for the backward)
 *   dinv [N]         (fill + sum of incoming weights)^-1/2, 0 where the degree is 0
 *   ew_csr, ew_csc [E]  edge weights permuted to CSR / CSC order (only when edge_weight != NULL)
 *   dinv_unw [N]     (1 + in-degree)^-1/2, only when edge_weight != NULL: the reference hands the
 *                    weights to conv1 only (model/gcn.py:58 vs :62), later layers run unweighted
 *   status [4]       status[0] = OR of HCG_STATUS_* bits (0 = clean)
 */
int hcg_plan_build(const int64_t* edge_index, const int64_t* batch, const float* edge_weight,
                   int64_t N, int64_t E, int64_t B, float fill, int mode,
                   int32_t* graph_ptr, int32_t* edge_ptr,
                   int32_t* rowptr, int32_t* col, int32_t* eid,
                   int32_t* rowptr_t, int32_t* col_t, int32_t* eid_t,
                   float* dinv, float* ew_csr, float* ew_csc, float* dinv_unw, int32_t* status,
                   void* workspace, size_t workspace_bytes, hcg_stream_t stream);

/* ---- dense linear (a4, a10):  y = act(x W^T + b),  W is [D_out, D_in] like nn.Linear ------ */
int hcg_linear_fwd(const float* x, const float* W, const float* b /*nullable*/, float* y,
                   int64_t M, int64_t D_in, int64_t D_out, int act, float slope, hcg_stream_t stream);
/* dz = dy * act'(y) is formed internally (y = saved OUTPUT); then dW = dz^T x, db = colsum dz,
 * dx = dz W (dx nullable).  dz_ws: caller buffer [M, D_out] (may alias nothing). */
int hcg_linear_bwd(const float* dy, const float* y, const float* x, const float* W,
                   float* dx /*nullable*/, float* dW, float* db /*nullable*/, float* dz_ws,
                   int64_t M, int64_t D_in, int64_t D_out, int act, float slope,
                   void* workspace, size_t workspace_bytes, hcg_stream_t stream);

/* ---- one GCNConv + bias + LeakyReLU (a4-a8), general shapes ------------------------------
 *   h = x W^T ; out_i = leaky( dinv_i * sum_{k in row i} w_k dinv_col[k] h_col[k]
 *                               + fill * dinv_i^2 h_i + b )
 *   h_ws: caller buffer [N, D] (the pre-aggregation features; not needed afterwards). */
int hcg_gcn_layer_fwd(const float* x, const float* W, const float* b,
                      const int32_t* rowptr, const int32_t* col, const float* ew_csr /*nullable*/,
                      const float* dinv, float fill, float slope, int apply_act,
                      float* h_ws, float* out, int64_t N, int64_t E, int64_t F, int64_t D,
                      hcg_stream_t stream);
/* backward of the above.  `out` = saved output (gives the LeakyReLU mask), `x` = saved input.
 *   dh_ws: caller buffer [N, D].  dx nullable (first layer: x has no grad). */
int hcg_gcn_layer_bwd(const float* dout, const float* out, const float* x, const float* W,
                      const int32_t* rowptr_t, const int32_t* col_t, const float* ew_csc /*nullable*/,
                      const float* dinv, float fill, float slope, int apply_act,
                      float* dh_ws, float* dx /*nullable*/, float* dW, float* db,
                      int64_t N, int64_t E, int64_t F, int64_t D,
                      void* workspace, size_t workspace_bytes, hcg_stream_t stream);

/* ---- explain mode (f4): ONE entry point, six jobs (`mode`).  HOST struct; zero it first, unused parts stay NULL.
 * PyG's Explainer multiplies every message by an edge mask inside each MessagePassing layer, AFTER gcn_norm, self loops keep 1
 * (reference scripts_experiments/explain_gnn.py:39-50: edge_mask_type='object'); the node mask multiplies x.
 *
 * HCG_EXPLAIN_GRAPHS: a whole batch of graphs in ONE launch, one workgroup per graph (csrc/explain.hip), weights frozen:
 *     x~ = x s(node_mask);  every conv layer  A = LeakyReLU(Ahat_m (A_prev W^T) + b)  with the message of edge e multiplied by
 *     m_e = s(edge_mask_e);  [max, mean] pooling;  readout of depth R  ->  out [B, C]
 *   s = sigmoid with HCG_EXPLAIN_SIGMOID in `flags`, else the identity.  Upstream gradient per graph g:
 *     target != NULL: l_g = mean_c (out_gc - target_gc)^2 (stored in loss [B]) and dout = 2 (out - target) / C;
 *     dout   != NULL: that row as given;
 *     HCG_EXPLAIN_TARGET_CLASS in `flags`: the target slot holds `target_class` [B], an int64 class index y_g per graph
 *       (the two names share one pointer of the struct, so its size and every offset are what they were; C >= 2 or
 *       HCG_ERR_UNSUPPORTED; the pointer must not be NULL): the cross-entropy of one row,
 *       l_g = -log_softmax(out_g)[y_g] (stored in loss [B]) and dout_gc = softmax(out_g)_c - [c == y_g], in float32 with the
 *       row's maximum subtracted.  y_g is compared, never used as an address: outside 0 .. C - 1 the graph's loss is NaN and
 *       its gradient that of "no class matched" (softmax(out_g));
 *     none of them: forward only (no gradient output is touched).  At most one of the three (HCG_ERR_INVALID_ARG).
 *     The flag belongs to HCG_EXPLAIN_GRAPHS and HCG_EXPLAIN_FIT: in every other mode it must be clear (HCG_ERR_INVALID_ARG).
 *   Gradients of J = sum_g l_g (or sum(dout * out)) with respect to the masks ONLY -- no dW, no db:
 *     d_edge_mask [E] in the caller's edge order (an explicit (i, i) edge collapses into the unit self loop: exactly 0),
 *     d_node_mask [N, F] (with node_mask), dx [N, F] = dJ/dx (nullable).
 *   Graphs are independent: no float atomics, no exchange between workgroups; every result is bitwise reproducible and
 *   bitwise independent of which other graphs share the batch.
 *   Shapes: D = 64, F <= 64, graphs of <= 224 nodes and <= 1024 directed edges (`max_nodes` / `max_edges` = largest graph of
 *   the batch, host metadata; a graph that exceeds them is refused: HCG_STATUS_SHAPE_LIMIT, its outputs zero), n_conv 1..4,
 *   R 1..4 (readout layer i maps 2D >> i to half of it + LeakyReLU, the last one to C), C <= 8.  Anything else:
 *   HCG_ERR_UNSUPPORTED.  Needs graph_ptr / edge_ptr / status of a BLOCKED plan and the raw int64 edge_index grouped by graph.
 *   `workspace`: the layers' H = A_prev W^T and A, which the backward reads again (workspace_bytes_needed, written by every
 *   call; only a call with target / dout / target_class uses it).
 *   HCG_EXPLAIN_QUERY in `flags`: validate the shapes (D, F, C, n_conv, R, max_nodes, max_edges, N, E, B), write
 *   workspace_bytes_needed, launch nothing, touch no GPU: HCG_OK or HCG_ERR_UNSUPPORTED.
 * HCG_EXPLAIN_LAYER_EDGE_GRAD: one layer of the any-shape path -- the gradient with respect to the per-edge multipliers ew_csr
 *   handed to hcg_gcn_layer_fwd:  dew_csr[k] = dinv_i dinv_{col k} <dY_i, h_{col k}>  with dY = layer_dout * act'(layer_out) and
 *   h = x W^T (recompute with hcg_linear_fwd); 0 for explicit self-loop entries.  Reads layer_dout, layer_out, layer_h [N, D],
 *   rowptr, col, dinv, slope, apply_act, N, E, D; writes dew_csr [E].  HCG_EXPLAIN_TARGET_CLASS must be clear (HCG_ERR_INVALID_ARG).
 * HCG_EXPLAIN_ENSEMBLE: `n_models` frozen models of ONE architecture predict the same batch of graphs in ONE launch, forward
 *   only (csrc/ensemble.hip; reference scripts_experiments/predict_test.py:19-103).  One workgroup per (graph, group of
 *   `models_per_group` models): gcn_norm and the row list are built once per workgroup and reused by its models.
 *   conv_W[l] / conv_b[l] / head_W[i] / head_b[i] point at the models' tensors stacked along a leading M axis
 *   ([M, D, F or D], [M, D], [M, out_i, in_i], [M, out_i]; contiguous).  out is [M, B, C]; emb ([M, B, 2D], max first) is
 *   written when not NULL.  edge_mask, node_mask, target / target_class and dout must be NULL (HCG_ERR_INVALID_ARG); loss, the gradient
 *   outputs and the workspace are not used (workspace_bytes_needed = 0).  Shapes and refusals as HCG_EXPLAIN_GRAPHS, plus
 *   1 <= n_models and 1 <= models_per_group <= n_models; a refused graph's rows of out / emb are zero for every model.  The
 *   result for (model, graph) is bitwise independent of n_models, of models_per_group and of the rest of the batch.
 *   HCG_EXPLAIN_QUERY as above.
 * HCG_EXPLAIN_SHAPLEY: Shapley value sampling (Captum's ShapleyValueSampling, baselines 0, one feature per step) of ONE frozen
 *   model for a batch of graphs, forward only (csrc/shapley.hip; reference scripts_experiments/explain_gnn.py).  Graph g with n
 *   nodes and e directed edges has K = n F + e features: local index j < n F is node-feature entry (j / F, j % F), j >= n F is
 *   local edge j - n F (the caller's edge order).  Off = the entry of x replaced by 0 / the edge's mask 0 (mask semantics of
 *   HCG_EXPLAIN_GRAPHS without sigmoid: after gcn_norm, every conv layer, dinv from the unmasked in-degree, self loops keep 1).
 *   `perm` [n_perm][N F + E] int32: row p holds, for every graph g at offset graph_ptr[g] F + edge_ptr[g], a permutation of
 *   0 .. K_g - 1 (contents are trusted; an index outside [0, K_g) is skipped).  One workgroup per (graph, permutation) keeps the
 *   graph in LDS and walks its permutation on chip: v_0 = out[class_index] with everything off, v_k with perm_1 .. perm_k on,
 *   phi_p[perm_k] = v_k - v_(k-1).  A node entry whose x is exactly 0 and an explicit (i, i) edge cannot change the output:
 *   their difference is exactly 0 and no evaluation is spent on them.  A call runs the permutations perm_first ..
 *   perm_first + perm_count - 1 into `workspace` ([perm_count][N F + E] f32 rows, workspace_bytes_needed) and then adds the
 *   rows, p ascending, onto shap_acc [N F + E] (node entries [N, F] first, then the E edges; a call with perm_first = 0 starts
 *   from 0, the call that ends at n_perm divides by n_perm): the mean over n_perm permutations in the fixed order 0, 1, ..,
 *   bitwise independent of how the permutations are split into calls.  out [B, C] = the output with everything on and
 *   out_base [B, C] = with everything off, both written by permutation 0's workgroups.  edge_mask, node_mask, target /
 *   target_class and dout must be NULL (HCG_ERR_INVALID_ARG).  Shapes: as HCG_EXPLAIN_GRAPHS but graphs of <= 184 nodes (three [n][64] tiles are kept
 *   in LDS) and perm_count <= 65535; refusals as there (HCG_STATUS_SHAPE_LIMIT: the graph's rows of every output zero).
 *   HCG_EXPLAIN_QUERY as above (reads perm_count too).
 *   HCG_EXPLAIN_GROUPED in `flags` (this mode only; in every other mode HCG_ERR_INVALID_ARG): the players are GROUPS of
 *   features (Captum's ShapleyValueSampling with feature_mask, baselines 0).  Graph g's K features, indexed as above, are
 *   partitioned into G_g groups with local ids 0 .. G_g - 1 and a background that is never a player: it is on in every
 *   evaluation, the base included.  G = shap_n_groups is the batch's number of groups, shap_group_ptr [B + 1] int32 their
 *   prefix sum (graph g's groups are shap_group_ptr[g] .. shap_group_ptr[g + 1] - 1 of every array of length G).  Only the
 *   LIVE members are listed (a node entry with x != 0, an edge that is not an explicit (i, i)): group shap_group_ptr[g] + y
 *   has the members shap_members[shap_member_ptr[..] .. shap_member_ptr[.. + 1]), local feature indices, ascending;
 *   shap_member_ptr is [G + 1] int32; graph g's live background is shap_bg_members[shap_bg_ptr[g] .. shap_bg_ptr[g + 1]),
 *   ascending, shap_bg_ptr [B + 1] int32 (both lists may lie in one array).  `perm` is [n_perm][G] int32: row p holds, for
 *   every graph at offset shap_group_ptr[g], a permutation of 0 .. G_g - 1.  v_0 = out[class_index] with the background on,
 *   v_k with the groups perm_1 .. perm_k on as well, phi_p[perm_k] = v_k - v_(k-1): a step switches every member of the group
 *   on (every element of the first layer's product has one owner, which adds the members' terms in ascending member order)
 *   and is evaluated ONCE.  A group without a live member -- an empty range -- gets exactly 0 and costs no evaluation.  The
 *   workspace rows and shap_acc have length G (workspace_bytes_needed = perm_count * max(G, 1) * 4 rounded up to 256, by a
 *   query too); out_base [B, C] = the output with the background only, out = with everything on.  Contents are trusted; a
 *   member outside [0, K_g) and a group id outside [0, G_g) are skipped, never used as an address.  0 <= shap_n_groups <=
 *   N F + E and, for a launch, the five arrays non-NULL (HCG_ERR_INVALID_ARG).  A refused graph: its G_g entries zero.  LDS,
 *   shapes and the order of the sum over the permutations as without the flag.  The shap_ fields are the fourth member of
 *   the union of the fit_, path_ and mom_ fields.
 *   A model axis (with and without HCG_EXPLAIN_GROUPED): `n_models` = M frozen models of one architecture (0, what a caller
 *   of the one-model form leaves there, means 1; 1 <= M <= 65535, else HCG_ERR_INVALID_ARG, by a query too).  The weight
 *   pointers name model 0 of tensors stacked along a leading model axis ([M, 64, F], [M, 64, 64], [M, 64], [M, out_i, in_i],
 *   [M, out_i]); the launch is dim3(B, perm_count, M) and workgroup (g, p, m) walks permutation p of graph g with model m:
 *   the model index shifts the weight pointers once, nothing else of the walk changes.  Every output takes a leading model
 *   axis: out / out_base [M][B][C], the workspace [M][perm_count][row] (workspace_bytes_needed = M times the one-model
 *   figure), shap_acc [M][row], each model's rows summed p ascending as above.  The permutations are shared by the models.
 *   Entry [m] is bitwise what a one-model call with model m's weights writes, whatever M and the other models are; a
 *   refused graph's entries are zero in every model's slice.  HCG_EXPLAIN_MOMENTS takes the mean and the standard deviation
 *   over the model axis of shap_acc.
 * HCG_EXPLAIN_COALITIONS: the coalition values of ONE frozen model for a batch of graphs (csrc/shapley.hip,
 *   k_coalition_values): the model's output for EVERY subset of each graph's groups, the table every exact quantity of a few
 *   players is a fixed linear form of (Shapley values, Shapley interaction indices, any single what-if).  Players, background,
 *   features and their indexing are those of HCG_EXPLAIN_SHAPLEY with HCG_EXPLAIN_GROUPED, and the shap_ fields are read as
 *   there, with one rule more: the caller lists the LIVE groups only (a group without a live member changes no output), so
 *   shap_group_ptr [B + 1] is the prefix sum of the graphs' live counts L_g and shap_n_groups their total.  Graph g has 2^L_g
 *   rows in coal_values [coal_rows, C] float32, from row coal_live_ptr[g] (int64 [B + 1]): row coal_live_ptr[g] + m holds
 *   all C outputs with the background and the live groups {k : bit k of m} on.  coal_jobs is an int32 array of triples
 *   (graph, first mask, masks); a call runs the jobs coal_job_first .. coal_job_first + coal_job_count - 1, one workgroup
 *   each, which builds its graph once and then, for every mask of its run, REBUILDS the state from zero -- nothing on, the
 *   live background applied, then the set groups in ascending order, each as the grouped walk applies a group -- and
 *   evaluates it once with the walk's evaluation.  So a row is bitwise independent of the run it sits in, of how the jobs
 *   are split into calls and of the rest of the batch, and row 2^(y + 1) - 1 is bitwise the grouped walk's v_(y + 1) in the
 *   identity order.  Every row has one writer; no workspace (workspace_bytes_needed = 0), no reduction, no atomics; `out`,
 *   out_base and shap_acc are not used.  Contents are trusted, but a graph outside [0, B), a member outside [0, K_g), a
 *   mask outside [0, 2^L_g) and a row outside [0, coal_rows) are skipped, never used as an address.  edge_mask, node_mask,
 *   target / target_class, dout and perm must be NULL and HCG_EXPLAIN_TARGET_CLASS / HCG_EXPLAIN_GROUPED clear
 *   (HCG_ERR_INVALID_ARG); coal_max_live = the largest L_g must be <= 16 and coal_rows < 2^31 (HCG_ERR_UNSUPPORTED); for a
 *   launch the five shap_ arrays, coal_values, coal_jobs and coal_live_ptr non-NULL.  Shapes, LDS and refusals as
 *   HCG_EXPLAIN_SHAPLEY (184 nodes; a refused graph: its rows zero, HCG_STATUS_SHAPE_LIMIT).  HCG_EXPLAIN_QUERY as above;
 *   also writes lds_bytes.  The coal_ fields follow the shap_ fields in the union's fourth member.  ONE model: n_models > 1
 *   is HCG_ERR_UNSUPPORTED (by a query too), never a silent run of model 0.
 * HCG_EXPLAIN_SUBSETS: the values of a caller's LIST of subsets of each graph's groups, for ONE frozen model and a batch of
 *   graphs (csrc/shapley.hip, k_subset_values): the primitive under deletion / insertion curves and any sampled estimator
 *   over groups, for ANY number of groups per graph (atoms as players: 57 - 184).  Players, background, features and their
 *   indexing are those of HCG_EXPLAIN_SHAPLEY with HCG_EXPLAIN_GROUPED and the shap_ fields are read as there: ALL groups of
 *   every graph are listed (a dead group has an empty member range), so a bit position is the caller's group id.  The
 *   subsets are bit words: sub_bits [coal_rows][W] uint32, sub_word_ptr [B + 1] int32 the prefix sum of ceil(G_g / 32),
 *   W = sub_word_ptr[B]; group y of graph g is on in row s iff bit (y & 31) of sub_bits[s W + sub_word_ptr[g] + (y >> 5)] is
 *   set (bits at or above G_g in a graph's last word are ignored).  sub_member_group, int32, parallel to shap_members, gives
 *   the local group id of every listed member.  The mode reuses the coal_ slots whose meaning carries over: coal_values is
 *   the table [S][B][C] float32 (row s of graph g at (s B + g) C), coal_rows = S, coal_jobs the int32 triples (graph, first
 *   row, rows), coal_job_first / coal_job_count the jobs of this call, one workgroup each; coal_live_ptr and coal_max_live
 *   are not read.  A workgroup builds its graph once and, for every row of its run, stages the graph's words of the row in
 *   LDS, REBUILDS the state from zero -- nothing on, the live background applied, then ONE filtered pass over the graph's
 *   whole member range that applies the members whose group's bit is set, in list order (no global load per group) -- and
 *   evaluates it once with the walk's evaluation.  The list is ordered by group, then by local index, and skipping does not
 *   reorder: for the same subset every element of the state takes the updates HCG_EXPLAIN_COALITIONS applies, in the same
 *   order, so the rows are bitwise that mode's, and a row depends on its bits and its graph alone -- not on the run, the
 *   call split, the other rows or the rest of the batch.  Every row has one writer; no workspace (workspace_bytes_needed =
 *   0), no reduction, no atomics; a row no job names is not written.  Contents are trusted, but a graph outside [0, B), a
 *   row outside [0, S), a member outside [0, K_g) and a group id outside [0, G_g) are skipped, never used as an address.
 *   edge_mask, node_mask, target / target_class, dout and perm must be NULL and HCG_EXPLAIN_TARGET_CLASS /
 *   HCG_EXPLAIN_GROUPED clear (HCG_ERR_INVALID_ARG); sub_max_groups = the largest G_g must be <= 16384 (the bits the staging
 *   holds; a graph inside the shape limits has at most 12800 features) and coal_rows < 2^31 (HCG_ERR_UNSUPPORTED); for a
 *   launch the five shap_ arrays, coal_values, coal_jobs, sub_bits, sub_word_ptr and sub_member_group non-NULL.  Shapes, LDS
 *   and refusals as HCG_EXPLAIN_SHAPLEY (184 nodes; a refused graph: the rows of its jobs zero, HCG_STATUS_SHAPE_LIMIT).
 *   HCG_EXPLAIN_QUERY as above; also writes lds_bytes.  The sub_ fields follow the coal_ fields in the union's fourth member.
 *   A model axis: `n_models` = M as in HCG_EXPLAIN_SHAPLEY (0 means 1; 1 <= M <= 65535, else HCG_ERR_INVALID_ARG; weights
 *   stacked [M, ...], the pointers naming model 0).  The launch is dim3(jobs, M): workgroup (j, m) runs job j with model m.
 *   coal_values is [M][S][B][C]; slice m is bitwise the one-model call's table for model m's weights; a refused graph's rows
 *   are zero in every slice.  Jobs, bit words and the member lists are shared by the models.
 * HCG_EXPLAIN_GREEDY: ONE ROUND of the model-driven greedy insertion or deletion order of each graph's groups, for ONE frozen
 *   model and a batch of graphs (csrc/shapley.hip, k_greedy_round): the order every attribution's deletion / insertion curve
 *   is read against, and the top-k sufficient / necessary set.  Players, background, features, their indexing and the shap_
 *   fields are those of HCG_EXPLAIN_SUBSETS (ALL groups listed; a dead group has an empty member range and is never a
 *   candidate), sub_member_group as there.  The on-set of graph g starts empty (insertion) or full (HCG_GREEDY_DELETION in
 *   greedy_flags).  In round k the candidates are the live groups not yet picked; candidate y's value is the output [C] with
 *   the background and (the on-set with y flipped) on; its key is sgn value[class_index], sgn = -1 with HCG_GREEDY_NEGATE
 *   and +1 without; the pick is the candidate with the greatest key, equal keys go to the lower group id and a NaN key
 *   counts as -inf -- a total order on (key, id), so the pick does not depend on the shape of the reduction -- and its bit
 *   is flipped for good.  A call is launch k = greedy_round of a sequence the caller enqueues on one stream, k = 0, 1, ...,
 *   with no host read in between: coal_jobs holds int32 triples (graph, first id, ids), the call runs the jobs
 *   coal_job_first .. coal_job_first + coal_job_count - 1, one workgroup each; launch k's jobs of a graph tile its ids
 *   0 .. G_g - 1, the job whose first id is 0 is the graph's OWNER (exactly one per graph and launch), and a graph whose
 *   rounds have all run gets one job (g, 0, 0) in the next launch and none afterwards.  A workgroup of launch k stages the
 *   graph's on-set after the picks 0 .. k - 2 as bit words in LDS from greedy_order[shap_group_ptr[g] ..] (integer
 *   operations only), and for k >= 1 computes pick k - 1 ITSELF from round k - 1's candidate values -- greedy_cand
 *   [2][G][C] float32, half (k - 1) & 1, written by launch k - 1; this launch writes the other half, so no workgroup reads
 *   what a sibling writes in the same launch, and no workgroup waits for another.  Only the owner writes
 *   greedy_order[shap_group_ptr[g] + k - 1] = the pick (int32 [G], the caller presets it to -1) and the pick's C values to
 *   row shap_group_ptr[g] + k - 1 of coal_values [G][C] (the caller presets 0); the owner of launch 0 evaluates the all-on
 *   and the background-only rows into `out` / out_base [B, C].  Then the workgroup evaluates its job's candidates: for each,
 *   the bit is flipped in LDS, the state REBUILT from zero and evaluated exactly as HCG_EXPLAIN_SUBSETS does for a row with
 *   those bits, the C outputs written to greedy_cand, and the bit flipped back -- so a candidate's value is bitwise that
 *   mode's row, a pick is a function of those values alone, and the result is bitwise independent of the tiling, of the
 *   rest of the batch and of the call.  No workspace (workspace_bytes_needed = 0), no reduction across workgroups, no
 *   atomics on floats.  Contents are trusted, but a graph outside [0, B), an id outside [0, G_g), an entry of greedy_order
 *   outside [0, G_g) and a member outside [0, K_g) are skipped, never used as an address.  edge_mask, node_mask, target /
 *   target_class, dout and perm must be NULL and HCG_EXPLAIN_TARGET_CLASS / HCG_EXPLAIN_GROUPED clear, greedy_round >= 0,
 *   greedy_flags within its two bits, 0 <= class_index < C (HCG_ERR_INVALID_ARG, checked before the shapes and by a query
 *   too); sub_max_groups = the largest G_g must be
 *   <= 16384 (HCG_ERR_UNSUPPORTED); for a launch the five shap_ arrays, sub_member_group, coal_values, coal_jobs,
 *   greedy_order, greedy_cand, `out` and out_base non-NULL.  coal_rows, coal_max_live and sub_word_ptr are not read.
 *   Shapes, LDS and refusals as HCG_EXPLAIN_SHAPLEY (184 nodes, 1024 directed edges, 160 KB; a refused graph: what its
 *   workgroups own is zero -- their candidate rows, the owner's row of coal_values, `out` / out_base -- its greedy_order
 *   entries are left alone, HCG_STATUS_SHAPE_LIMIT).  HCG_EXPLAIN_QUERY as above; also writes lds_bytes.  greedy_round and
 *   greedy_flags follow the sub_ fields in the union's fourth member, which they fill; greedy_order and greedy_cand take
 *   the slots of coal_live_ptr and sub_bits, which this mode does not read.  ONE model: n_models > 1 is HCG_ERR_UNSUPPORTED
 *   (by a query too) -- an ensemble's pick needs a reduction over the models inside a round, which this kernel does not have.
 * HCG_EXPLAIN_FIT: GNNExplainer's whole mask optimisation (published torch_geometric 2.3 / 2.4 GNNExplainer, model explanation,
 *   node_mask_type 'attributes', edge_mask_type 'object'; regression, or multiclass classification on raw outputs) for a
 *   batch of graphs in ONE launch: the kernel of
 *   HCG_EXPLAIN_GRAPHS with an epoch loop around forward and backward, one workgroup per graph, run as a batch-of-one fit
 *   per graph.  The parameters are the LOGITS fit_edge_logit [E] / fit_node_logit [N, F]; every epoch evaluates
 *   HCG_EXPLAIN_GRAPHS with HCG_EXPLAIN_SIGMOID on them against `target` (regression: the mean squared error) or, with
 *   HCG_EXPLAIN_TARGET_CLASS, `target_class` (classification: the cross-entropy, as above) -- the slot is required; loss of
 *   epoch t in fit_loss_hist[t, g] --,
 *   adds -- from the epoch after the hard flags exist -- the gradients of
 *     coeffs[0] sum(m) + coeffs[1] mean(ent(m)) over the graph's hard edges and
 *     coeffs[2] mean(m) + coeffs[3] mean(ent(m)) over its hard node entries,  m = sigmoid(logit),
 *     ent(m) = -m log(m + 1e-15) - (1 - m) log(1 - m + 1e-15)  (a term over an empty set is 0),
 *   and takes one Adam step (fit_lr, fit_beta1, fit_beta2, fit_eps; the update of hcg_adam_step, bias corrections from the
 *   integer step) on both masks.  The epoch at step 0 then sets hard = (gradient != 0) and counts the hard entries per graph
 *   (fit_hard_count); an entry that is not hard never moves.  step_first = steps the state has taken, epoch_count = epochs of
 *   this launch: a fit split into several launches is bitwise the single launch.  out [B, C] = the last epoch's outputs;
 *   fit_edge_mask_out / fit_node_mask_out = sigmoid(logit) of the hard entries, 0 elsewhere.  edge_mask, node_mask, dout and dx
 *   must be NULL.  Shapes, workspace and refusals as HCG_EXPLAIN_GRAPHS (a refused graph: its rows of out, fit_loss_hist and
 *   the two mask outputs zero, its state untouched).  No float atomics, no exchange between workgroups.
 *   HCG_EXPLAIN_QUERY as above; this mode also writes lds_bytes.
 * HCG_EXPLAIN_INTEGRATED: integrated gradients (Captum's IntegratedGradients as torch_geometric's CaptumExplainer calls it:
 *   inputs a node mask of ones [N, F] and an edge mask of ones [E], baselines 0) of output column path_class_index for a batch
 *   of graphs in ONE launch: the kernel of HCG_EXPLAIN_GRAPHS without sigmoid with a loop over the quadrature points around
 *   forward and backward, one workgroup per graph, the graph built once.  For k = path_step_first .. path_step_first +
 *   path_step_count - 1, ascending: every node-mask and edge-mask entry of the graph is path_alpha[k]; the upstream gradient
 *   is 1 at column path_class_index and 0 elsewhere (the index is compared, never used as an address); and the two mask
 *   gradients g are accumulated, acc = fmaf(path_weight[k], g, acc), into path_node_attr [N, F] / path_edge_attr [E] (an
 *   explicit (i, i) edge and an entry whose x is 0: exactly 0).  Every accumulator entry is read and written by ONE thread
 *   of the graph's workgroup, the same in every step; the launch with path_step_first = 0 starts from 0 whatever the arrays
 *   hold, a later one continues from them: a path split into several launches is bitwise the single launch.  The launch
 *   with path_step_first = 0 also runs two forward-only passes, masks of 1 and of 0, into path_out_full / path_out_base
 *   [B, C].  path_alpha / path_weight: float32 device arrays [path_steps].  HCG_EXPLAIN_SIGMOID and HCG_EXPLAIN_TARGET_CLASS
 *   must be clear; target, dout, edge_mask, node_mask and dx must be NULL; path_steps >= 1, 0 <= path_step_first,
 *   path_step_first + path_step_count <= path_steps, 0 <= path_class_index < C (each: HCG_ERR_INVALID_ARG).  `out` is not
 *   used.  The path_ fields share the storage of the fit_ fields (a union: the two modes never meet in one call), so the
 *   struct's size and every earlier offset are what they were.  Shapes, workspace, LDS and refusals as HCG_EXPLAIN_GRAPHS
 *   (a refused graph: its rows of path_out_full / path_out_base and its entries of both attribution arrays zero, the other
 *   graphs untouched).  HCG_EXPLAIN_QUERY as above (checks the flags and the NULL pointers too); also writes lds_bytes.
 *   A model axis: `n_models` = M frozen models of one architecture (0, what a caller of the one-model form leaves there,
 *   means 1; 1 .. 65535, otherwise HCG_ERR_INVALID_ARG) run the same path in ONE launch, one workgroup per (graph, model).
 *   conv_W[l] / conv_b[l] / head_W[i] / head_b[i] then point at tensors stacked along a leading model axis, the layout of
 *   HCG_EXPLAIN_ENSEMBLE; path_node_attr is [M, N, F], path_edge_attr [M, E], path_out_full / path_out_base [M, B, C], and
 *   the workspace M times the one-model workspace (workspace_bytes_needed, the query too, accounts for M; model m uses
 *   slice m).  Entry [m] of every output is bitwise what the one-model call with model m's weights writes, whatever M and
 *   the other models are; a refused graph's rows are zero in every model's outputs.  To run a sub-range of an ensemble the
 *   caller passes pointers already offset to its first model.  `models_per_group` is not read.
 * HCG_EXPLAIN_MOMENTS: mean and standard deviation over a model axis, for the outputs of HCG_EXPLAIN_INTEGRATED with
 *   n_models > 1.  Up to two arrays per call (s = 0, 1; mom_len[s] = 0 leaves one out): mom_values[s] is [mom_count, mom_len[s]]
 *   float32, row j = model mom_first + j of an ensemble of mom_total models.  One thread per entry walks the rows in
 *   ascending order with Welford's recurrence in float32, no operation contracted:  d = v - mean;  mean += d / k;
 *   m2 += d * (v - mean),  k = the 1-based count over the WHOLE ensemble (mom_first + j + 1).  The state is the caller's
 *   mom_mean[s] / mom_m2[s] [mom_len[s]]: the call with mom_first = 0 starts from 0 whatever they hold, a later call
 *   continues from them, and the call with mom_first + mom_count = mom_total also writes mom_std[s] = sqrtf(m2 / mom_total)
 *   (the population form).  Every entry has one owner and a fixed order: the moments are bitwise independent of how the
 *   models are split into calls; an entry that is 0 in every model has mean and std exactly 0.  No atomics; consecutive
 *   threads read consecutive floats.  mom_total >= 1, 0 <= mom_first, mom_first + mom_count <= mom_total, 0 <= mom_len[s] <
 *   2^31 (each: HCG_ERR_INVALID_ARG); HCG_EXPLAIN_TARGET_CLASS must be clear.  No other field is read; no workspace
 *   (workspace_bytes_needed = 0).  The mom_ fields are a third member of the union of the fit_ and path_ fields. */
#define HCG_EXPLAIN_GRAPHS 0
#define HCG_EXPLAIN_LAYER_EDGE_GRAD 1
#define HCG_EXPLAIN_ENSEMBLE 2
#define HCG_EXPLAIN_SHAPLEY 3
#define HCG_EXPLAIN_FIT 4
#define HCG_EXPLAIN_INTEGRATED 5
#define HCG_EXPLAIN_MOMENTS 6
#define HCG_EXPLAIN_COALITIONS 7
#define HCG_EXPLAIN_SUBSETS 8
#define HCG_EXPLAIN_GREEDY 9
#define HCG_GREEDY_DELETION 1  /* greedy_flags: the on-set starts full and a pick removes a group */
#define HCG_GREEDY_NEGATE 2    /* greedy_flags: the key is -value[class_index] */
#define HCG_EXPLAIN_QUERY 1    /* flags */
#define HCG_EXPLAIN_SIGMOID 2  /* flags */
#define HCG_EXPLAIN_TARGET_CLASS 4  /* flags: the target slot holds int64 class indices [B] (target_class), not float [B, C] */
#define HCG_EXPLAIN_GROUPED 8  /* flags: HCG_EXPLAIN_SHAPLEY walks groups of features (the shap_ fields) */
#define HCG_EXPLAIN_MAX_CONVS 4
typedef struct hcg_explain_args {
  int32_t mode;                          /* HCG_EXPLAIN_GRAPHS / _LAYER_EDGE_GRAD / _ENSEMBLE / _SHAPLEY / _FIT / _INTEGRATED / _MOMENTS / _COALITIONS / _SUBSETS / _GREEDY */
  int32_t flags;                         /* HCG_EXPLAIN_QUERY | HCG_EXPLAIN_SIGMOID | HCG_EXPLAIN_TARGET_CLASS | HCG_EXPLAIN_GROUPED */
  const float* x;                        /* [N, F] */
  const int64_t* edge_index;             /* [2, E], grouped by graph */
  const int32_t* graph_ptr;              /* [B + 1] */
  const int32_t* edge_ptr;               /* [B + 1] */
  const float* edge_mask;                /* [E], the caller's edge order */
  const float* node_mask;                /* [N, F], nullable */
  union {                                /* ONE pointer, read by the flag HCG_EXPLAIN_TARGET_CLASS: */
    const float* target;                 /*   clear: [B, C], nullable */
    const int64_t* target_class;         /*   set: [B] class indices (HCG_EXPLAIN_GRAPHS / _FIT) */
  };
  const float* dout;                     /* [B, C], nullable (at most one of target / dout / target_class) */
  const float* conv_W[HCG_EXPLAIN_MAX_CONVS];   /* conv layer l: lin.weight [D, F or D]; entries >= n_conv unused */
  const float* conv_b[HCG_EXPLAIN_MAX_CONVS];   /* conv layer l: bias [D] */
  const float* head_W[4];                /* readout layer i: weight [out_i, in_i]; entries >= R unused (HCG_HEAD_MAX_LAYERS) */
  const float* head_b[4];                /* readout layer i: bias [out_i] */
  float* out;                            /* [B, C] */
  float* loss;                           /* [B]; required with target and with target_class */
  float* d_edge_mask;                    /* [E] */
  float* d_node_mask;                    /* [N, F]; required with node_mask, NULL without */
  float* dx;                             /* [N, F], nullable */
  int32_t* status;                       /* the plan's status words */
  void* workspace;
  size_t workspace_bytes;
  size_t workspace_bytes_needed;         /* OUT */
  int64_t N, E, B, F, D, C;
  int64_t max_nodes, max_edges;
  int32_t n_conv, R;
  float slope;                           /* LeakyReLU negative slope (conv layers and readout) */
  int32_t apply_act;                     /* HCG_EXPLAIN_LAYER_EDGE_GRAD */
  const float* layer_dout;               /* HCG_EXPLAIN_LAYER_EDGE_GRAD from here on */
  const float* layer_out;
  const float* layer_h;
  const int32_t* rowptr;
  const int32_t* col;
  const float* dinv;
  float* dew_csr;
  float* emb;                            /* HCG_EXPLAIN_ENSEMBLE from here on: [M, B, 2D], nullable */
  int32_t n_models;                      /* M (also read by HCG_EXPLAIN_INTEGRATED, _SHAPLEY and _SUBSETS: 0 means 1; _COALITIONS and _GREEDY refuse M > 1) */
  int32_t models_per_group;              /* models one workgroup runs on its graph, 1 .. M */
  const int32_t* perm;                   /* HCG_EXPLAIN_SHAPLEY from here on: [n_perm][N F + E] */
  float* out_base;                       /* [B, C] */
  float* shap_acc;                       /* [N F + E]: running sum, the mean after the last call */
  int32_t n_perm;                        /* P */
  int32_t perm_first;                    /* first permutation of this call */
  int32_t perm_count;                    /* permutations of this call */
  int32_t class_index;                   /* the explained output column, 0 .. C - 1 */
  int32_t lds_bytes;                     /* OUT: dynamic LDS of one workgroup for max_nodes / max_edges (also by a query) */
  int32_t reserved;
  union {                                /* ONE block of storage, read by `mode` (the struct's size and every offset stay): */
  struct {                               /*   HCG_EXPLAIN_FIT */
  float* fit_edge_logit;                 /* IN/OUT state of the edge mask, [E] each */
  float* fit_edge_exp_avg;
  float* fit_edge_exp_avg_sq;
  uint8_t* fit_edge_hard;                /* 1: the entry's first gradient was not 0 (written by the step-0 epoch) */
  float* fit_node_logit;                 /* IN/OUT state of the node-feature mask, [N, F] each */
  float* fit_node_exp_avg;
  float* fit_node_exp_avg_sq;
  uint8_t* fit_node_hard;
  int32_t* fit_hard_count;               /* IN/OUT [B, 2]: hard edges, hard node entries of every graph (read when step_first > 0) */
  float* fit_loss_hist;                  /* OUT [epoch_count, B]: the prediction loss of every epoch */
  float* fit_edge_mask_out;              /* OUT [E]: sigmoid(logit) of the hard entries, 0 elsewhere */
  float* fit_node_mask_out;              /* OUT [N, F] */
  int32_t step_first;                    /* Adam steps the state has taken */
  int32_t epoch_count;                   /* epochs of this launch, >= 1 */
  float fit_lr, fit_beta1, fit_beta2, fit_eps;
  float fit_coeffs[4];                   /* edge_size (on a sum), edge_ent, node_feat_size (on a mean), node_feat_ent */
  };
  struct {                               /*   HCG_EXPLAIN_INTEGRATED */
  const float* path_alpha;               /* [path_steps] quadrature points in (0, 1), device memory */
  const float* path_weight;              /* [path_steps] their weights */
  float* path_node_attr;                 /* IN/OUT [N, F]: sum_k w_k d out[g, c] / d node mask at alpha_k (read when path_step_first > 0) */
  float* path_edge_attr;                 /* IN/OUT [E], the caller's edge order */
  float* path_out_full;                  /* OUT [B, C]: the outputs at masks of 1 (written by the launch with path_step_first = 0) */
  float* path_out_base;                  /* OUT [B, C]: at masks of 0 */
  int32_t path_steps;                    /* n_steps of the whole path, >= 1 */
  int32_t path_step_first;               /* first quadrature point of this launch */
  int32_t path_step_count;               /* points of this launch; path_step_first + path_step_count <= path_steps */
  int32_t path_class_index;              /* the attributed output column c, 0 .. C - 1 */
  };
  struct {                               /*   HCG_EXPLAIN_MOMENTS */
  const float* mom_values[2];            /* [mom_count, mom_len[s]]: row j = model mom_first + j */
  float* mom_mean[2];                    /* IN/OUT [mom_len[s]]: running mean (read when mom_first > 0) */
  float* mom_m2[2];                      /* IN/OUT [mom_len[s]]: running sum of squared deviations */
  float* mom_std[2];                     /* OUT [mom_len[s]]: sqrtf(m2 / mom_total), by the call that ends at mom_total */
  int64_t mom_len[2];                    /* entries per model of array s; 0: the array is not used */
  int32_t mom_total;                     /* models of the whole ensemble, >= 1 */
  int32_t mom_first;                     /* first model of this call */
  int32_t mom_count;                     /* models of this call; mom_first + mom_count <= mom_total */
  int32_t mom_reserved;
  };
  struct {                               /*   HCG_EXPLAIN_SHAPLEY with HCG_EXPLAIN_GROUPED, HCG_EXPLAIN_COALITIONS, HCG_EXPLAIN_SUBSETS and HCG_EXPLAIN_GREEDY */
  const int32_t* shap_group_ptr;         /* [B + 1] prefix sum of the graphs' group counts */
  const int32_t* shap_member_ptr;        /* [G + 1] group -> its range of shap_members */
  const int32_t* shap_members;           /* live members only: local feature indices, ascending within a group */
  const int32_t* shap_bg_ptr;            /* [B + 1] graph -> its range of shap_bg_members */
  const int32_t* shap_bg_members;        /* the live background, ascending within a graph */
  int64_t shap_n_groups;                 /* G */
  float* coal_values;                    /* HCG_EXPLAIN_COALITIONS from here on: OUT [coal_rows, C] */
  const int32_t* coal_jobs;              /* [.][3]: graph, first mask, masks */
  union {                                /* one slot: */
  const int64_t* coal_live_ptr;          /* [B + 1] graph g's rows: coal_live_ptr[g] + mask */
  int32_t* greedy_order;                 /* HCG_EXPLAIN_GREEDY: IN/OUT [G] the picks, graph g's from shap_group_ptr[g]; preset to -1 */
  };
  int64_t coal_rows;                     /* T_live = sum_g 2^L_g */
  int32_t coal_job_first;                /* first job of this call */
  int32_t coal_job_count;                /* jobs of this call (the grid) */
  int32_t coal_max_live;                 /* the largest L_g, <= 16 */
  int32_t coal_reserved;
  union {                                /* one slot: */
  const uint32_t* sub_bits;              /* HCG_EXPLAIN_SUBSETS from here on (it reads coal_values / _jobs / _rows / _job_first / _job_count too): [coal_rows][W] */
  float* greedy_cand;                    /* HCG_EXPLAIN_GREEDY: IN/OUT [2][G][C] the candidates' values of the last two rounds */
  };
  const int32_t* sub_word_ptr;           /* [B + 1] prefix sum of ceil(G_g / 32); W = sub_word_ptr[B] */
  const int32_t* sub_member_group;       /* parallel to shap_members: the member's local group id */
  int32_t sub_max_groups;                /* the largest G_g, <= 16384 */
  int32_t sub_reserved;
  int32_t greedy_round;                  /* HCG_EXPLAIN_GREEDY (it reads the shap_ fields, coal_values / _jobs / _job_first / _job_count, sub_member_group / _max_groups too): k */
  int32_t greedy_flags;                  /* HCG_GREEDY_DELETION | HCG_GREEDY_NEGATE */
  };
  };
} hcg_explain_args;
int hcg_explain(hcg_explain_args* args_host, hcg_stream_t stream);

/* ---- graph pooling (a9): emb[g] = [ max_i a_i , mean_i a_i ]  (max FIRST, model/gcn.py:65-66) */
int hcg_pool_fwd(const float* a, const int32_t* graph_ptr, float* emb /*[B,2D]*/,
                 int64_t N, int64_t B, int64_t D, hcg_stream_t stream);
/* da_i = demb_max[g] * [a_i == max_g] / #ties  +  demb_mean[g] / n_g   (torch amax semantics) */
int hcg_pool_bwd(const float* demb, const float* a, const float* emb, const int32_t* graph_ptr,
                 float* da, int64_t N, int64_t B, int64_t D, hcg_stream_t stream);

/* ---- fused per-layer kernels for batches of small graphs (<= 32 nodes per tile, D = 64, F <= 64) ----
 * One launch per layer: tile of whole graphs -> LDS, gcn_norm rebuilt on chip from the tile's raw COO
 * edges (LDS integer atomics into a [32][32] count matrix: no CSR), x W^T AND the neighbourhood sum
 * on the f32 matrix cores, bias + LeakyReLU, optional [max, mean] pooling epilogue (a3-a9).
 * Needs only graph_ptr / edge_ptr of a BLOCKED plan (edges grouped by graph) and the original int64
 * edge_index [2, E]; unweighted edges (self-loop weight 1).
 *   hcg_fused_graphs_per_tile: graphs packed into one 32-row tile, 0 = shape not supported
 *   emb != NULL  : also write emb[B, 2D] = [max, mean] of `out` per graph (last conv layer)
 *   status       : the plan's status words; HCG_STATUS_SHAPE_LIMIT is raised if a tile exceeds 32 rows,
 *                  HCG_STATUS_EDGE_UNGROUPED if an edge leaves its tile (such edges are ignored)
 */
int hcg_fused_graphs_per_tile(int64_t F, int64_t D, int64_t max_nodes_per_graph);
size_t hcg_fused_workspace_bytes(int64_t B, int64_t F, int64_t D, int graphs_per_tile);
/* EVERY forward form of the small-graph tiles is one entry point with one argument block (HOST struct; zero it first):
 *   W2 != NULL       two stacked conv layers F -> D -> D in ONE launch (the reference's default n_convolutions = 2): the
 *                    first layer's output tile never leaves the chip before it is consumed; out1 (and out2) are written
 *                    once each (the backward needs them)
 *   emb != NULL      also emb[B, 2D] = [max, mean] of the last layer per graph
 *   poolbits != NULL training form of the POOLED (last) layer: its node activations never reach HBM (out2 / out1 of a single
 *                    layer = NULL).  All the pooled backward needs of them is, per element, the sign (LeakyReLU') and
 *                    whether it is its graph's column maximum (torch amax backward: ties share the gradient evenly) -- they
 *                    leave as two bits per element (hcg_fused_aux_bytes: 512 B per 32-row tile, in the matrix-core
 *                    accumulator layout) and hcg_fused_layer_bwd over the SAME plan and graphs_per_tile reads them in
 *                    place of `out` and `emb`
 *   head_W0 != NULL  (stacked training form only) the regression head in the TAIL of the same launch: every workgroup runs
 *                    readout forward, squared error and (unless head_flags = HCG_HEAD_FORWARD_ONLY) the unscaled readout
 *                    backward over its own graphs -- see hcg_head_fwd_bwd for the contract of y / z / out / demb /
 *                    step_counter; head_workspace (hcg_fused_aux_bytes) gets one gradient slab + SSE partial per
 *                    workgroup, described by hcg_fused_head_reduce_job.  A training step is then this launch, the conv
 *                    backward -- two hcg_fused_layer_bwd launches, or ONE pair launch (below) -- and hcg_step_tail: four
 *                    launches, three with the pair.
 * Replaces reference model/gcn.py:58-66 (+ :70-71 with the head).
 *
 * mode = HCG_FUSED_BWD_PAIR: the same block describes the BACKWARD of two consecutive conv layers, F -> D (lower: input x,
 * weight W1, output out1) and D -> D (upper: input out1, weight W2, output out2), as ONE launch: each workgroup runs
 * hcg_fused_layer_bwd's work for the upper layer over its tiles, then -- behind a workgroup barrier, the same waves over the
 * same tiles in the same order -- for the lower layer.  Every result (pair_dx, both slab workspaces) is bitwise that of the two
 * hcg_fused_layer_bwd launches.  The upper layer takes the forms of hcg_fused_layer_bwd: poolbits != NULL (demb given;
 * pair_dout, emb, out2 = NULL), pooled plain (pair_dout = NULL; demb, emb, out2 given) or not pooled (pair_dout given;
 * out2 required with bit 0 of pair_act_upper).  Workspaces and reduce jobs are the single launches': one
 * hcg_fused_workspace_bytes / hcg_fused_reduce_job per layer.  b1, b2, and the head fields are ignored.
 *   HCG_ERR_UNSUPPORTED  the pair does not apply -- D != 64, F > 64, pair_graphs_per_tile_upper != graphs_per_tile, bit 1
 *                        of pair_act_upper clear (dx must go down premasked), pair_act_lower != 0, pair_dx = NULL, out1 or
 *                        pair_dx not 16-byte aligned, or a library built without the pair: issue the two launches instead
 *   pair_flags = HCG_FUSED_PAIR_QUERY  validate only: the same codes, no workspace needed, the GPU is not touched */
#define HCG_FUSED_FORWARD 0
#define HCG_FUSED_BWD_PAIR 1
#define HCG_FUSED_PAIR_QUERY 1
typedef struct hcg_fused_fwd_args {
  const float* x;
  const float* W1;
  const float* b1;
  const float* W2;            /* nullable */
  const float* b2;
  const int64_t* edge_index;
  int64_t E;
  const int32_t* graph_ptr;
  const int32_t* edge_ptr;
  int64_t N, B, F, D;
  int32_t graphs_per_tile;
  int32_t apply_act;
  float slope;
  int32_t head_flags;
  float* out1;                /* layer-1 node embeddings */
  float* out2;                /* layer-2 node embeddings (stacked, no poolbits) */
  float* emb;                 /* nullable */
  uint32_t* poolbits;         /* nullable */
  int32_t* status;
  const float* y;             /* head: targets [B, C] */
  const float* head_W0;       /* NULL = no head */
  const float* head_b0;
  const float* head_W1;
  const float* head_b1;
  int64_t C;
  float* z;
  float* out;
  float* demb;
  void* head_workspace;
  size_t head_workspace_bytes;
  int32_t* step_counter;      /* nullable */
  int32_t mode;               /* HCG_FUSED_FORWARD (0) or HCG_FUSED_BWD_PAIR; the fields below: the pair only */
  int32_t pair_flags;         /* 0 or HCG_FUSED_PAIR_QUERY */
  float* pair_dx;             /* [N, D] gradient between the two layers (written, then read by the same launch) */
  const float* pair_dout;     /* [N, D] upstream gradient of an upper layer that is not pooled; NULL = pooled */
  void* pair_ws_upper;        /* slab workspace of the upper layer (hcg_fused_workspace_bytes with F = D) */
  size_t pair_ws_upper_bytes;
  void* pair_ws_lower;        /* slab workspace of the lower layer */
  size_t pair_ws_lower_bytes;
  int32_t pair_act_upper;     /* apply_act bits of hcg_fused_layer_bwd for the upper layer (bit 1 required) */
  int32_t pair_act_lower;     /* ... for the lower layer: 0 */
  int32_t pair_graphs_per_tile_upper;   /* the upper layer's graphs per tile: must equal graphs_per_tile */
  int32_t pair_reserved;
} hcg_fused_fwd_args;
int hcg_fused_forward(const hcg_fused_fwd_args* args_host, hcg_stream_t stream);
#define HCG_FUSED_POOLBITS 0 /* bytes of `poolbits` */
#define HCG_FUSED_HEAD_WS 1  /* bytes of `head_workspace` */
size_t hcg_fused_aux_bytes(int kind, int64_t B, int graphs_per_tile);
int hcg_fused_head_reduce_job(const void* workspace, size_t workspace_bytes, int64_t B, int graphs_per_tile, int64_t C,
                              float* dW0 /*NULL: partials only*/, float* db0, float* dW1, float* db1, hcg_reduce_job* job_host);
/* backward, stage 1 (ONE launch).  dout == NULL selects the pooled form: the upstream gradient is
 * demb[B, 2D] and is expanded on chip with `emb` (ties of the max split evenly) -- or, poolbits != NULL, with the
 * training form's bits (dout, emb, out = NULL then).  dx nullable (first layer).  Leaves one partial slab
 * [D*KPAD + D] per workgroup in `workspace` (hcg_fused_workspace_bytes); stage 2 = hcg_fused_reduce_job + hcg_step_tail
 * sums them in a fixed order into dW [D, F], db [D]: bitwise reproducible.
 * apply_act here is a bit set: bit 0 = multiply the upstream gradient by LeakyReLU'(out) (as in the forward);
 * bit 1 = hand dx down ALREADY multiplied by LeakyReLU'(x) -- x being the previous layer's activated output, whose
 * rows this kernel holds anyway -- so that layer's backward is called with bit 0 clear and `out` = NULL and never
 * reads its own output.  `out` is only required with bit 0 set or in the pooled form without poolbits. */
int hcg_fused_layer_bwd(const float* dout /*nullable*/, const float* demb, const float* emb,
                        const float* out, const uint32_t* poolbits /*nullable*/, const float* x, const float* W,
                        const int64_t* edge_index, int64_t E,
                        const int32_t* graph_ptr, const int32_t* edge_ptr,
                        int64_t N, int64_t B, int64_t F, int64_t D,
                        int graphs_per_tile, float slope, int apply_act,
                        float* dx /*nullable*/, int32_t* status,
                        void* workspace, size_t workspace_bytes, hcg_stream_t stream);

/* ---- fused per-layer kernels for batches of MID-SIZE graphs: one graph per workgroup, <= 224 nodes and <= 1024
 * directed edges per graph, D = 64 or 128 (two 64-column halves, one launch each), F <= 128 (contracted in chunks of 64)
 * -- the size range of the reference's own reaction graphs (56-184 atoms, F = 25 / 32) and of BASELINE's large-ligand
 * configuration (200 nodes, 128-d).  Same contract as hcg_fused_layer_*: raw int64 edge_index grouped by graph + graph_ptr / edge_ptr of
 * a BLOCKED plan, gcn_norm and the CSR rebuilt on chip per graph, unweighted edges, optional pooled epilogue /
 * pooled-gradient prologue, per-workgroup gradient slabs (hcg_mid_reduce_job + hcg_step_tail).
 * `max_nodes` / `max_edges` = largest graph of the batch (host metadata; sizes the dynamic LDS); a graph that exceeds
 * them is skipped and flagged HCG_STATUS_SHAPE_LIMIT.  apply_act of hcg_mid_layer_bwd is the same bit set as in
 * hcg_fused_layer_bwd (bit 1 = premasked dx; `out` nullable when bit 0 is clear and dout is given). */
int hcg_mid_supported(int64_t F, int64_t D, int64_t max_nodes_per_graph, int64_t max_edges_per_graph);
size_t hcg_mid_workspace_bytes(int64_t B, int64_t F, int64_t D, int64_t max_nodes, int64_t max_edges);
int hcg_mid_layer_fwd(const float* x, const float* W, const float* b,
                      const int64_t* edge_index, int64_t E, const int32_t* graph_ptr, const int32_t* edge_ptr,
                      int64_t N, int64_t B, int64_t F, int64_t D, int64_t max_nodes, int64_t max_edges,
                      float slope, int apply_act, float* out, float* emb /*nullable*/,
                      uint8_t* poolbits /*nullable: see hcg_tall_layer_fwd*/,
                      float* xagg /*nullable*/, uint8_t* signbits /*nullable: both, see hcg_tall_layer_fwd*/, int32_t* status,
                      hcg_stream_t stream);
int hcg_mid_layer_bwd(const float* dout /*nullable*/, const float* demb, const float* emb,
                      const float* out, const float* x, const float* W,
                      const int64_t* edge_index, int64_t E, const int32_t* graph_ptr, const int32_t* edge_ptr,
                      int64_t N, int64_t B, int64_t F, int64_t D, int64_t max_nodes, int64_t max_edges,
                      float slope, int apply_act, float* dx /*nullable*/, int32_t* status,
                      void* workspace, size_t workspace_bytes, hcg_stream_t stream);

/* ---- wide layers over large graphs (D = 128; BASELINE configs[4]: 200-atom graphs x 128-d): the layer as a dense
 * row-streaming transform over all nodes (weight image resident in LDS, A fragments straight from global memory, no
 * barrier in the steady state) + a per-graph segmented sum that keeps only the CSR in LDS and gathers rows through L2
 * (csrc/tall.hip).  Same contract and graph limits as hcg_mid_layer_* (raw grouped edge_index + graph_ptr / edge_ptr of a
 * BLOCKED plan, gcn_norm rebuilt on chip per graph, pooled epilogue / pooled-gradient prologue, apply_act bits of
 * hcg_fused_layer_bwd); F a multiple of 4, <= 128.  The forward needs the workspace too (H = x W^T makes a round trip).
 * hcg_tall_layer_bwd leaves dW / db slabs in the workspace: hcg_tall_reduce_jobs fills TWO jobs (dW, db) for
 * hcg_step_tail.  Replaces the same PyG GCNConv call sites (model/gcn.py:58-63) and their autograd. */
int hcg_tall_supported(int64_t F, int64_t D, int64_t max_nodes_per_graph, int64_t max_edges_per_graph);
size_t hcg_tall_workspace_bytes(int64_t N, int64_t B, int64_t F, int64_t D);
int hcg_tall_layer_fwd(const float* x, const float* W, const float* b,
                       const int64_t* edge_index, int64_t E, const int32_t* graph_ptr, const int32_t* edge_ptr,
                       int64_t N, int64_t B, int64_t F, int64_t D, int64_t max_nodes, int64_t max_edges,
                       float slope, int apply_act, float* out, float* emb /*nullable*/,
                       uint8_t* poolbits /*nullable*/, float* xagg /*nullable*/, uint8_t* signbits /*nullable*/,
                       int32_t* status, void* workspace, size_t workspace_bytes, hcg_stream_t stream);
/* `poolbits` [N, D / 4] bytes (training form of the POOLED layer, needs emb; F <= 64 for D = 64): the layer's output is
 * NOT written (`out` may be NULL) -- one byte per (row, 4 columns) leaves instead: bits 0-3 = the value is positive
 * (LeakyReLU'), bits 4-7 = it is its graph's column maximum (where global_max_pool's gradient goes, ties included).  Given
 * to hcg_tall_layer_bwd (pooled form: dout = NULL) they stand in for `out` AND `emb` (both may be NULL): a sixteenth of the
 * bytes on both sides of the step. */
/* `xagg` [N, 32 | 64 (F <= 32 | F <= 64)] + `signbits` [N, 8] bytes (training form of a FIRST, not pooled, 64-wide layer; given
 * together): besides `out` the forward leaves xagg = Ahat x (zero-padded columns) and, per row, four 16-bit pieces (piece j bit
 * q = column 4 q + j of `out` is positive).  Given to hcg_tall_layer_bwd with dout and dx = NULL they select the first-layer
 * form: dW = (dout (.) leaky'(out))^T xagg and db = the column sums of that product's left operand in ONE dense launch (the
 * same sums as (Ahat^T G)^T x in another order) -- no transpose sum, no dH round trip; `out`, `x` are not read.
 * hcg_tall_reduce_jobs(first_layer_form = 1) describes its slabs. */
int hcg_tall_layer_bwd(const float* dout /*nullable*/, const float* demb, const float* emb,
                       const float* out, const uint8_t* poolbits /*nullable*/,
                       const float* xagg /*nullable*/, const uint8_t* signbits /*nullable*/,
                       const int32_t* n_dev /*nullable; first-layer form: the batch's node count on the device (graph_ptr + B) when
                                              N is a CAPACITY (a captured epoch's batch slot): rows past it stay out of the sums*/,
                       const float* x, const float* W,
                       const int64_t* edge_index, int64_t E, const int32_t* graph_ptr, const int32_t* edge_ptr,
                       int64_t N, int64_t B, int64_t F, int64_t D, int64_t max_nodes, int64_t max_edges,
                       float slope, int apply_act, float* dx /*nullable*/, int32_t* status,
                       void* workspace, size_t workspace_bytes, hcg_stream_t stream);

/* ---- fused readout head (a10 + its backward) for the reference's default shape (the autograd path's form):
 *      z = LeakyReLU(emb W0^T + b0) [B,2D]->[B,D];  out = z W1^T + b1 [B,D]->[B,C];  D = 64, C <= 8 (= hcg_head_supported
 *      with D = 64).  forward: one launch (z is kept for the backward).  backward: hcg_readout2_bwd_partial (below: demb
 *      + per-workgroup slabs, workspace HCG_WS_READOUT2, described in job_host) + hcg_step_tail. */
int hcg_readout2_fwd(const float* emb, const float* W0, const float* b0, const float* W1, const float* b1,
                     int64_t B, int64_t D, int64_t C, float slope, float* z, float* out, hcg_stream_t stream);

/* ---- regression head: readout forward, squared error, readout backward in ONE launch (a10 + a12 + their backward; f2)
 * The reference's step runs  out = readout(emb); loss = torch.sqrt(MSELoss()(out, y.unsqueeze(1)));
 * loss.backward()  (model/gcn.py:70-71, utils/utils_model.py:64-65).  The whole backward is LINEAR in the one number
 * that needs every graph of the batch, dloss/dout = scale * (out - y) with scale = 1 / (B C sqrt(MSE)): so this kernel --
 * and every conv backward launch behind it -- runs on the UNSCALED error (the gradients of SSE / 2), every workgroup
 * leaves ONE partial sum of squared errors in its slab, and the step's last launch (hcg_step_tail) adds the partials in
 * a fixed order, derives loss and scale and multiplies each gradient element as it reduces it.  No grid-wide exchange
 * (round 2's head kernel spent a grid barrier, 520 sync words and a time-out path on that scalar), any grid size.
 *   z [B,D], out [B,C] : forward results
 *   demb [B,2D]        : d (SSE / 2) / d emb  -- unscaled
 *   workspace          : gradient slabs + SSE partials (describe them with hcg_head_reduce_job)
 *   step_counter       : nullable; two int32 device words, each incremented by 1 per launch: [0] the number of the
 *                        training step, read later in the same step by hcg_step_tail's update, [1] the exchange stamp
 *   flags              : HCG_HEAD_FORWARD_ONLY = no backward (demb / gradient slabs untouched; the partials are written)
 *                        HCG_HEAD_LOSS_CE = the classification head (below) instead of the squared error
 * y is [B,C] like out.  D = 64 or 128 (8 waves per workgroup, W0 fragments from L2 instead of LDS), C <= 8
 * (hcg_head_supported).
 * Classification (HCG_HEAD_LOSS_CE, with hcg_head_fwd_bwd and hcg_head_deep_fwd_bwd): the loss is
 * nn.CrossEntropyLoss()(out, y.long()) -- mean over the B graphs of logsumexp(out[g]) - out[g][label], default settings, no
 * sqrt.  y is then [B] float32 holding the class index of every graph.  The error the backward runs on is
 * d[c] = softmax(out[g])[c] - [c == label], the workgroup's partial is its sum of per-graph loss terms, and the deferred
 * scale (HCG_LOSS_CE) is 1 / B.  The row maximum is subtracted before the exponentials; label and class are matched by
 * comparing (float)c == y[g], nothing is indexed by the label: a label that equals none of 0 .. C-1 (out of range,
 * negative, not an integer) makes that graph's loss term -- and so the batch loss -- NaN, `out` is written as usual. */
#define HCG_HEAD_FORWARD_ONLY 1
#define HCG_HEAD_LOSS_CE 2
int hcg_head_supported(int64_t D, int64_t C);
size_t hcg_head_workspace_bytes(int64_t B, int64_t D);
int hcg_head_fwd_bwd(const float* emb, const float* y, const float* W0, const float* b0, const float* W1,
                     const float* b1, int64_t B, int64_t D, int64_t C, float slope, int flags,
                     float* z, float* out, float* demb, void* workspace, size_t workspace_bytes,
                     int32_t* step_counter /*nullable*/, hcg_stream_t stream);

/* ---- regression head of readout depth R = 1, 3, 4 in ONE launch: the contract of hcg_head_fwd_bwd (forward, squared
 * error, backward on the unscaled error, one gradient slab + SSE partial per workgroup, step_counter, flags) for the
 * reference's deeper readouts (model/gcn.py:36-45): layer i maps in_i = 2D >> i to in_i / 2 features followed by
 * LeakyReLU(slope) for i < R - 1, the last layer maps in_{R-1} to C with no activation.  Depth 2 is hcg_head_fwd_bwd.
 * D = 64 or 128, 1 <= C <= 8: the shapes for which hcg_general_workspace_bytes(HCG_WS_HEAD_DEEP, B, D, C, R) is not 0.
 * Weights and emb / demb rows must be 16-byte aligned.  Gradient slab per workgroup: [dW_i | db_i] for i = 0 .. R-1, back
 * to back.  job_host (nullable) receives their description for hcg_step_tail: ONE job of R segments, segment i reduced
 * into grad[i] = layer i's dW with its db directly behind it (the parameter order of a flat gradient buffer); with
 * grad[0] == NULL or HCG_HEAD_FORWARD_ONLY the job carries the SSE partials only (hcg_loss_finalize). */
#define HCG_HEAD_MAX_LAYERS 4
typedef struct hcg_head_args {
  const float* emb;                      /* [B, 2D] pooled graph embedding */
  const float* y;                        /* [B, C] targets; HCG_HEAD_LOSS_CE: [B] class indices */
  const float* W[HCG_HEAD_MAX_LAYERS];   /* readout layer i: weight [out_i, in_i]; entries >= R unused */
  const float* b[HCG_HEAD_MAX_LAYERS];   /* readout layer i: bias [out_i] */
  float* out;                            /* [B, C] */
  float* demb;                           /* [B, 2D] d (SSE / 2) / d emb, unscaled; unused with HCG_HEAD_FORWARD_ONLY */
  void* workspace;                       /* HCG_WS_HEAD_DEEP bytes: gradient slabs + SSE partials */
  size_t workspace_bytes;
  int32_t* step_counter;                 /* nullable: as hcg_head_fwd_bwd */
  float* grad[HCG_HEAD_MAX_LAYERS];      /* layer i's gradient destination [dW_i | db_i] (see job_host) */
  int64_t B, D, C;
  int32_t R;                             /* readout depth */
  int32_t flags;                         /* HCG_HEAD_FORWARD_ONLY | HCG_HEAD_LOSS_CE, or 0 */
  float slope;                           /* LeakyReLU negative slope of the hidden layers */
  int32_t reserved;
} hcg_head_args;
int hcg_head_deep_fwd_bwd(const hcg_head_args* args_host, hcg_reduce_job* job_host, hcg_stream_t stream);

/* loss modes of hcg_step_tail / hcg_loss_finalize / hcg_loss_fwd_bwd */
#define HCG_LOSS_MSE 0  /* nn.MSELoss                                  : scale 2 / count            */
#define HCG_LOSS_RMSE 1 /* torch.sqrt(nn.MSELoss) (the reference's step): scale 1 / (count sqrt(MSE)) */
#define HCG_LOSS_SSE 2  /* data parallel with a collective: gradients stay those of SSE / 2, [SSE, count] go to sse_tail;
                           ranks sum gradients, SSE and count (ONE all-reduce) and hcg_update_dev / hcg_adam_step_dev_sse
                           scale by 1 / (count sqrt(SSE / count)): the gradient of sqrt(MSE) over the concatenated batch of
                           all ranks, which is what the reference's step computes on one device */
#define HCG_LOSS_CE 3   /* nn.CrossEntropyLoss() behind a head launched with HCG_HEAD_LOSS_CE (hcg_step_tail and
                           hcg_loss_finalize only): the partials are sums of per-graph loss terms, count = B,
                           scale 1 / count, loss[0] = loss[1] = sum / count.  hcg_loss_fwd_bwd takes it with the class
                           count in the bits above HCG_LOSS_CE_CLASSES_SHIFT (see there) */
#define HCG_LOSS_CE_CLASSES_SHIFT 8

/* ---- MSE loss (a12 / f2): loss[0] = mean((a - b)^2) over n elements, fixed-order reduction;
 *      backward: da = grad_loss[0] * 2 (a - b) / n, db = -da (either may be NULL). */
int hcg_mse_fwd(const float* a, const float* b, int64_t n, float* loss, hcg_stream_t stream);
int hcg_mse_bwd(const float* a, const float* b, const float* grad_loss, int64_t n,
                float* da /*nullable*/, float* db /*nullable*/, hcg_stream_t stream);

/* Loss AND its gradient in one launch, for heads the fused kernel does not cover (other widths): mode 0 = MSE,
 * 1 = sqrt(MSE) (the reference's step, utils/utils_model.py:64), HCG_LOSS_SSE = unscaled da = a - b with [SSE, n] stored
 * in sse_tail.  loss[0] = the loss, loss[1] = MSE; da [n] = d loss / d a.
 * mode = HCG_LOSS_CE | (C << HCG_LOSS_CE_CLASSES_SHIFT) -- a mode of this entry point rather than a symbol of its own --:
 * nn.CrossEntropyLoss()(a, b.long()) with default settings, for heads the one-launch kernels do not cover (more than 8
 * classes, other widths) and for the eager loss module.  a [B, C] logits with n = B * C, b [B] float32 class indices
 * (matched by (float)c == b[g], as with HCG_HEAD_LOSS_CE: a label outside 0 .. C-1 gives a NaN loss), loss[0] = loss[1] =
 * the mean over the graphs of logsumexp(a[g]) - a[g][label] (fixed-order sum), da [B, C] (nullable in this mode) =
 * (softmax(a[g]) - onehot) / B, the gradient already scaled; sse_tail is not used. */
int hcg_loss_fwd_bwd(const float* a, const float* b, int64_t n, int mode, float* loss, float* da /*nullable with HCG_LOSS_CE*/,
                     float* sse_tail /*nullable unless mode = HCG_LOSS_SSE*/, hcg_stream_t stream);

/* ---- batched slab reduction: ONE launch for all pending gradient reductions of a backward pass.
 * hcg_fused_layer_bwd and hcg_readout2_bwd_partial leave per-workgroup slabs in their workspaces;
 * hcg_fused_reduce_job / hcg_readout2_bwd_partial describe them (host-side), hcg_step_tail
 * sums up to HCG_REDUCE_MAX_JOBS of them in a fixed order. */
#define HCG_REDUCE_MAX_JOBS 8
#define HCG_REDUCE_MAX_SEGS 4
typedef struct hcg_reduce_seg {
  int32_t begin, count;      /* element range of the slab */
  int32_t row_in, row_out;   /* rows of row_in elements are written as rows of row_out (<= row_in) elements */
  float* dst;
} hcg_reduce_seg;
typedef struct hcg_reduce_job {
  const float* slabs;        /* [nslabs][slab_floats] */
  const float* sse_part;     /* != NULL: [nslabs] partial sums of squared errors, one per workgroup, contiguous (the head's
                                job: hcg_head_reduce_job / hcg_fused_head_reduce_job fill it in); NULL = none */
  int32_t nslabs, slab_floats, nseg, reserved;
  hcg_reduce_seg seg[HCG_REDUCE_MAX_SEGS];
} hcg_reduce_job;
/* sizeof of the ABI's HOST structs (a binding checks its mirrors against them) */
#define HCG_STRUCT_REDUCE_JOB 0
#define HCG_STRUCT_TAIL_ARGS 1
#define HCG_STRUCT_FUSED_FWD_ARGS 2
#define HCG_STRUCT_COLLATE_ARGS 3
#define HCG_STRUCT_COLLATE_SLOT 4
#define HCG_STRUCT_UPDATE_ARGS 5
#define HCG_STRUCT_HEAD_ARGS 6
#define HCG_STRUCT_EXPLAIN_ARGS 7
#define HCG_STRUCT_FIT_CONTROL_ARGS 8
#define HCG_STRUCT_FIT_STATE 9   /* (a DEVICE struct the host reads back: hcg_fit_state) */
#define HCG_STRUCT_EPOCH_DRAW_ARGS 10
#define HCG_STRUCT_PCG64 11      /* (a DEVICE struct the host reads back: hcg_pcg64) */
size_t hcg_struct_bytes(int which);
int hcg_fused_reduce_job(const void* workspace, size_t workspace_bytes, int64_t N, int64_t B, int64_t F,
                         int64_t D, int graphs_per_tile, float* dW, float* db, hcg_reduce_job* job_host);
/* the readout2 backward leaves its slabs and describes them (dW0 [D, 2D], db0 [D], dW1 [C, D], db1 [C]) in job_host */
int hcg_readout2_bwd_partial(const float* dout, const float* emb, const float* z, const float* W0,
                             const float* W1, int64_t B, int64_t D, int64_t C, float slope, float* demb,
                             void* workspace, size_t workspace_bytes, float* dW0, float* db0, float* dW1, float* db1,
                             hcg_reduce_job* job_host, hcg_stream_t stream);
/* one job per 64-column half (half = 0 .. D/64 - 1): rows [64 half, 64 half + 64) of dW [D, F] / db [D] */
int hcg_mid_reduce_job(const void* workspace, size_t workspace_bytes, int64_t B, int64_t F, int64_t D,
                       int64_t max_nodes, int64_t max_edges, int half, float* dW, float* db, hcg_reduce_job* job_host);
/* job_host[0] = dW [D, F], job_host[1] = db [D] of hcg_tall_layer_bwd */
int hcg_tall_reduce_jobs(const void* workspace, size_t workspace_bytes, int64_t N, int64_t B, int64_t F, int64_t D,
                         int first_layer_form, float* dW, float* db, hcg_reduce_job* job_host /*[2]*/);
/* the head's slabs; job_host->sse_part = the workgroups' SSE partials.  dW0 == NULL (forward-only head): no segments,
 * the job then only carries the partials (hcg_loss_finalize) */
int hcg_head_reduce_job(const void* workspace, size_t workspace_bytes, int64_t B, int64_t D, int64_t C,
                        float* dW0, float* db0, float* dW1, float* db1, hcg_reduce_job* job_host);
/* `more` (same slab geometry and destinations, slabs directly behind `job`'s) becomes part of `job`: one fixed-order sum */
int hcg_reduce_job_append(hcg_reduce_job* job_host, const hcg_reduce_job* more_host);

/* ---- the step tail: ONE launch behind the backward launches of a training step (f2) --------------------------------
 *   (1) every pending slab reduction (jobs_host[0 .. njobs)), each output element summed in a fixed order;
 *   (2) the loss and its deferred scale: when a job carries SSE partials (sse_part), loss[0] = the loss (`loss_mode`),
 *       loss[1] = MSE, and every reduced element is multiplied by the scale (see hcg_head_fwd_bwd); HCG_LOSS_SSE leaves the
 *       gradients unscaled and stores this rank's [SSE, count] in sse_tail;
 *   (3) inbox != NULL: the data-parallel one-shot exchange over xGMI (below) between reduction and update;
 *   (4) param != NULL: the optimiser's update (`update_rule`, HCG_UPDATE_*) of the parameter / its state at the offset of
 *       each gradient element in the flat buffer [grad_flat, grad_flat + n) -- every segment's dst must point into it and
 *       every element of it must be covered by exactly one segment; `step_dev[0]` = 1-based number of THIS update, already
 *       advanced when the kernel runs (the head launch's step_counter does that earlier in the step; this launch only reads
 *       it), lr_dev[0] = lr.  Adam: exp_avg, exp_avg_sq, beta1, beta2, eps; RMSprop: exp_avg_sq = square_avg, beta2 =
 *       alpha, eps; SGD: no state (exp_avg / exp_avg_sq unused).  The exchange (3) rides with HCG_UPDATE_ADAM only;
 *   (5) next_batch != NULL: the pointers-only plan of the NEXT batch (what hcg_plan_build does with HCG_PLAN_BLOCKED |
 *       HCG_PLAN_PTRS_ONLY | HCG_PLAN_KEEP_STATUS): the one launch of the next step that depends on nothing of this one.
 * Replaces the four hcg_reduce_slabs* entry points of round 2 (one symbol per fusion combination).  HOST struct; zero it
 * first, unused parts stay NULL. */
typedef struct hcg_tail_args {
  const hcg_reduce_job* jobs_host;
  int32_t njobs;
  int32_t loss_mode;           /* HCG_LOSS_*; only read when a job has sse_part */
  float loss_count;            /* elements of the squared-error sum on this rank: B * C; HCG_LOSS_CE: B */
  float beta1, beta2, eps;
  float* loss;                 /* [2], nullable without exchange */
  float* sse_tail;             /* [2], nullable */
  float* grad_flat;            /* [n] ([n + 2] with an exchange: gradients | SSE | count) */
  float* param;                /* NULL = no update */
  float* exp_avg;
  float* exp_avg_sq;
  int64_t n;
  const float* lr_dev;
  const int32_t* step_dev;
  const int64_t* next_edge_index;
  const int64_t* next_batch;   /* NULL = no plan */
  int64_t next_N, next_E, next_B;
  int32_t* next_graph_ptr;
  int32_t* next_edge_ptr;
  int32_t* next_status;
  void* inbox;                 /* NULL = no exchange */
  void* const* peers_host;     /* HOST array of `world` device pointers (peers_host[rank] = inbox) */
  int32_t rank, world, xchg_mode;
  int32_t update_rule;         /* HCG_UPDATE_*; 0 (a zeroed struct) = Adam */
  int32_t* xchg_err;
} hcg_tail_args;
int hcg_step_tail(const hcg_tail_args* args_host, hcg_stream_t stream);
/* forward-only steps (the reference's eval_network body, utils/utils_model.py:75-78): the loss alone from a head job's partials */
int hcg_loss_finalize(const hcg_reduce_job* head_job_host, float count, int loss_mode, float* loss,
                      float* sse_tail /*nullable*/, hcg_stream_t stream);

/* update rules of hcg_step_tail / hcg_update_dev, torch's defaults for each (torch.optim.Adam(lr, betas, eps): amsgrad /
 * weight_decay / maximize off; torch.optim.SGD(lr): momentum / dampening / nesterov / weight_decay / maximize off,
 * p -= lr g; torch.optim.RMSprop(lr, alpha, eps): momentum / centered / weight_decay / maximize off,
 * v = alpha v + (1 - alpha) g^2, p -= lr g / (sqrt(v) + eps)) */
#define HCG_UPDATE_ADAM 0
#define HCG_UPDATE_SGD 1
#define HCG_UPDATE_RMSPROP 2

/* ---- Adam update (f2) over one contiguous fp32 segment: torch.optim.Adam's rule (amsgrad / weight_decay /
 *      maximize off).  `step` = 1-based count of this update.  One launch. */
int hcg_adam_step(float* param, const float* grad, float* exp_avg, float* exp_avg_sq, int64_t n,
                  float lr, float beta1, float beta2, float eps, int64_t step, hcg_stream_t stream);

/* Same update with the step count and the learning rate in DEVICE memory, so that the launch can sit inside a
 * captured hipGraph.  `step_dev` = int32 [count, stamp, ticket, pad]: `step_dev[0]` = number of updates done so far (the
 * kernel uses step_dev[0] + 1 and the last workgroup to finish stores the incremented count); `step_dev[1]` = the
 * exchange stamp (hcg_step_tail), which this update neither reads nor writes; `step_dev[2]` is its ticket word, zero
 * between launches.  `lr_dev[0]` = learning rate (the host rewrites it when a scheduler changes it). */
int hcg_adam_step_dev(float* param, const float* grad, float* exp_avg, float* exp_avg_sq, int64_t n,
                      const float* lr_dev, float beta1, float beta2, float eps, int32_t* step_dev, hcg_stream_t stream);

/* Data-parallel SSE form (HCG_LOSS_SSE): `flat` = [n summed SSE/2-gradients | SSE | count].  Scales the n
 * gradients in place by 1 / (count * L), L = sqrt(SSE / count), and stores loss[0] = L, loss[1] = SSE / count, then
 * applies hcg_adam_step_dev's update with the scaled gradient: one launch. */
int hcg_adam_step_dev_sse(float* param, float* flat, float* exp_avg, float* exp_avg_sq, int64_t n,
                          const float* lr_dev, float beta1, float beta2, float eps, int32_t* step_dev, float* loss,
                          hcg_stream_t stream);

/* ---- fit control: what the reference's epoch loop does on the host between two epochs (scripts_experiments/
 * train_GNN.py:73-111: ReduceLROnPlateau, early stopping, the copy of the best weights, the loss log), as ONE launch of ONE
 * workgroup behind an epoch's train / validation / test graphs on the same stream, so that a whole fit is enqueued without
 * the host reading a loss.  Reached through hcg_update_dev (`fit_control` of hcg_update_args: the exported symbols are
 * capped, tests/test_host_cpu.py); enqueue-only, owns no memory.
 * Thread 0, in float64 with every product, quotient and comparison the one Python's floats make on the host:
 *   stopped, or epoch >= max_epochs: nothing at all is written;
 *   loss_k = *sums[k] / denom[k] (k = train, validation, test); log[epoch] = {train, validation, test, lr after the epoch};
 *   epoch % control_every == 0: torch's ReduceLROnPlateau.step(validation) for mode "min", threshold_mode "rel" (better:
 *     a < best * rel_epsilon, rel_epsilon = 1 - threshold formed by the host; cooldown; num_bad_epochs > patience:
 *     new = max(lr * factor, min_lr), taken when lr - new > eps, then *lr_dev = (float)lr), then the loop's bookkeeping:
 *     validation < val_best: val_best, best_epoch = epoch, stall = 0, snapshot; else ++stall; stopped = stall > early_stopping;
 *   ++epoch, ++epochs_counted.
 * A NaN loss is never better (IEEE comparisons, as on the host).  On a snapshot the whole workgroup copies param [n] into
 * best [n] (16-byte accesses where both are 16-byte aligned, a scalar tail); thread 0 stores the state last. */
typedef struct hcg_fit_state {   /* DEVICE struct, caller-initialised */
  double lr;                   /* the learning rate (param_groups[0]["lr"]) */
  double sched_best;           /* ReduceLROnPlateau.best (+inf at the start) */
  double val_best;             /* best validation loss seen on a control epoch (+inf at the start) */
  int32_t epoch;               /* epochs seen = row of the log the next launch writes */
  int32_t num_bad_epochs, cooldown_counter, last_epoch;   /* ReduceLROnPlateau's */
  int32_t best_epoch, stall, stopped, epochs_counted;
} hcg_fit_state;
typedef struct hcg_fit_control_args {   /* HOST struct; zero it first */
  const double* sums[3];       /* device scalars: dot(losses, counts) of the train, validation and test epoch */
  double denom[3];             /* their denominators (graphs of each dataset), > 0 */
  hcg_fit_state* state;
  float* lr_dev;               /* the optimiser's learning-rate word */
  const float* param;          /* [n] the flat parameters (read) */
  float* best;                 /* [n] the best slot (written on a snapshot) */
  int64_t n;
  double* log;                 /* [max_epochs, 4] */
  double factor, rel_epsilon, min_lr, eps;
  int32_t patience, cooldown, control_every, early_stopping, max_epochs, reserved;
} hcg_fit_control_args;

/* Every rule's capturable update (HCG_UPDATE_*) with hcg_adam_step_dev's step-word contract (step_dev = [count, stamp,
 * ticket, pad]: count advanced by one, stamp untouched, ticket zero between launches), plain or in the SSE form.
 *   fit_control != NULL: the launch is the fit controller above and nothing else of this struct is read;
 *   loss == NULL: `grad` = [n] gradients;
 *   loss != NULL: `grad` = [n summed SSE/2-gradients | SSE | count], scaled in place by 1 / (count * L), L = sqrt(SSE /
 *                 count); loss[0] = L, loss[1] = SSE / count;
 *   param == NULL: no update -- only the SSE form's scale and loss (needs loss; the other pointers and step_dev unused).
 * State per rule as in hcg_tail_args (Adam: exp_avg, exp_avg_sq; RMSprop: exp_avg_sq = square_avg, beta2 = alpha;
 * SGD: none).  HOST struct; zero it first. */
typedef struct hcg_update_args {
  float* param;                /* NULL = no update */
  float* grad;
  float* exp_avg;
  float* exp_avg_sq;
  int64_t n;
  const float* lr_dev;
  int32_t* step_dev;
  float* loss;                 /* NULL = plain form */
  float beta1, beta2, eps;
  int32_t update_rule;         /* HCG_UPDATE_* */
  const hcg_fit_control_args* fit_control;   /* HOST pointer; NULL = an update */
} hcg_update_args;
int hcg_update_dev(const hcg_update_args* args_host, hcg_stream_t stream);

/* ---- data parallel: one-shot gradient exchange over xGMI, fused between the slab reduction and the update ------------
 * Every rank owns an inbox (hcg_xchg_inbox_bytes: 2 x world x (n + 2) eight-byte {value, step} granules) in fine-grained
 * device memory (hcg_xchg_alloc: the ONE allocation this library makes -- ordinary device memory does not make a peer's
 * stores visible to a running kernel), exports it (hcg_xchg_ipc_export -> 64-byte handle, exchanged by the host through
 * torch.distributed) and maps its peers' (hcg_xchg_ipc_open).  hcg_step_tail with `inbox` set: every reduced element is
 * first written into all peers' inboxes (one 8-byte system-scope store per peer, over the direct links), the peers'
 * contributions are polled out of the own inbox and added in rank order, and the update runs on the total: xchg_mode
 * HCG_XCHG_MEAN = mean over the ranks of each rank's own loss gradient; HCG_XCHG_SSE = the gradient of sqrt(MSE) over the
 * concatenated batch (SSE and count travel as elements n, n + 1: from the head's partials, or, without a job that carries
 * them, from grad_flat[n], [n + 1]; loss[0..1] = the global sqrt(MSE), MSE).  Polls are bounded (2 s): HCG_XCHG_ERR_TIMEOUT
 * is ORed into xchg_err[0] and the element becomes NaN.  `step_dev[1]` stamps the granules: it must advance by one per
 * exchange on every rank, and an inbox must be re-zeroed before it serves another optimiser. */
#define HCG_XCHG_MAX_WORLD 8
#define HCG_XCHG_HANDLE_BYTES 64
#define HCG_XCHG_MEAN 0
#define HCG_XCHG_SSE 1
#define HCG_XCHG_ERR_TIMEOUT 1
size_t hcg_xchg_inbox_bytes(int64_t n, int world);
/* workgroups of the exchanging hcg_step_tail that are resident at once on this device (occupancy x CUs).  A launch whose
 * jobs need more polling workgroups (sum over the jobs of ceil(slab_floats / 32)) is refused with HCG_ERR_UNSUPPORTED: two
 * ranks' resident pollers could otherwise wait on each other's queued publishers until the bounded polls expire */
int hcg_xchg_resident_blocks(void);
int hcg_xchg_alloc(size_t bytes, void** ptr);
int hcg_xchg_free(void* ptr);
int hcg_xchg_zero(void* ptr, size_t bytes);
int hcg_xchg_ipc_export(void* ptr, void* handle64);
int hcg_xchg_ipc_open(const void* handle64, void** ptr);
int hcg_xchg_ipc_close(void* ptr);

/* ---- on-device collation (f1): gather the graphs of an HBM-resident dataset into PyG-style batches, ONE launch for one
 * batch or for every batch of an epoch.
 * Dataset side: x_all [N_all, F], local edge lists src_all / dst_all (int32 ids inside their graph),
 * node_ptr_all / edge_ptr_all [G+1] (int64), y_all [G], idx_all [G].
 * A slot = one batch: `ids` [B] selects its graphs (device); graph_ptr / edge_ptr [B+1] (int32) are the batch's prefix sums
 * (the host knows the sizes; they double as the fused path's plan).  Writes x_out [N_out, F], edge_index_out [2, E_out]
 * (batch-local ids), batch_out [N_out], y_out / idx_out [B] (nullable).
 * nslots == 1: the batch is `slot` (host values).  nslots > 1: `slots_dev` is a DEVICE array of nslots descriptors (every
 * batch of a shuffled epoch: train.EpochWindow collates an epoch in one launch in front of its steps), max_B the largest
 * slot.B; the caller has validated them.  Replaces reference data/datasets.py:74-78 + PyG collate (call_methods.py:41-46). */
/* ---- an epoch's shuffle and index arrays drawn on the device: ONE launch of ONE workgroup (csrc/shuffle.hip), reached
 * through hcg_collate (`epoch_draw` of hcg_collate_args: the exported symbols are capped, tests/test_host_cpu.py), so that
 * an epoch of a fit needs no host data and a control interval of epochs can be one captured graph (fit.py).
 * The generator is numpy's PCG64 in device memory, its fields those of `np.random.PCG64().state` (the 128-bit integers as a
 * low and a high word); the draw is bit for bit `np.random.Generator(PCG64).permutation(G)`:
 *   a = arange(G); for i = G-1 .. 1: j = random_interval(i), swap a[i], a[j]     (G == 1 draws nothing)
 *   random_interval(max): mask = the smallest 2^k - 1 >= max; repeat v = next_uint32() & mask until v <= max
 *   next_uint32(): the buffered high half if has_uint32 (cleared), else w = next_uint64(), the high half kept, the low returned
 *   next_uint64(): state = state * 0x2360ED051FC65DA44385DF649FCCF645 + inc (mod 2^128); rotr64(hi ^ lo, state >> 122)
 * One lane walks the swap chain with the array in LDS.  The workgroup then fills `layout` exactly as the host's
 * `store.epoch_layout` does: int64 ids [G] | per batch an int32 block graph_ptr | per batch an int32 block edge_ptr, every
 * block (B + 2) / 2 int64 words holding the B + 1 prefix sums of the permuted graphs' node / edge counts (from node_ptr_all /
 * edge_ptr_all of hcg_collate_args, the only other fields read) behind a zero, a padding int32 zero where B is even; batches
 * of `batch_size` graphs, the last one shorter (dropped with `drop_last`): G + 2 * tot words, tot = the blocks' words.
 * `gate` != NULL and the fit stopped, or its epoch outside [0, gate_max_epochs): NOTHING is written, generator and layout
 * stay as they are -- epochs enqueued past a fit's stop draw nothing, the generator ends where the host loop's would.
 * G <= HCG_EPOCH_DRAW_MAX_GRAPHS (what one workgroup keeps in LDS; any number of batches), else HCG_ERR_UNSUPPORTED. */
#define HCG_EPOCH_DRAW_MAX_GRAPHS 8192
typedef struct hcg_pcg64 {     /* DEVICE struct, caller-initialised */
  uint64_t state_lo, state_hi, inc_lo, inc_hi;
  uint32_t has_uint32, uinteger;
} hcg_pcg64;
typedef struct hcg_epoch_draw_args {   /* HOST struct; zero it first */
  hcg_pcg64* rng;                    /* device */
  int64_t* layout;                   /* device [G + 2 * tot] */
  const hcg_fit_state* gate;         /* device, nullable */
  int64_t G;
  int32_t batch_size, drop_last, gate_max_epochs, reserved;
} hcg_epoch_draw_args;

typedef struct hcg_collate_slot {
  const int64_t* ids;
  const int32_t* graph_ptr;
  const int32_t* edge_ptr;
  float* x_out;
  int64_t* edge_index_out;
  int64_t* batch_out;
  float* y_out;               /* nullable */
  int64_t* idx_out;           /* nullable */
  int64_t B, N_out, E_out;
} hcg_collate_slot;
typedef struct hcg_collate_args {
  const float* x_all;
  const int32_t* src_all;
  const int32_t* dst_all;
  const int64_t* node_ptr_all;
  const int64_t* edge_ptr_all;
  const float* y_all;         /* nullable when no slot has y_out */
  const int64_t* idx_all;     /* nullable when no slot has idx_out */
  int64_t F;
  int32_t nslots;
  int32_t reserved;
  hcg_collate_slot slot;                 /* nslots == 1 */
  const hcg_collate_slot* slots_dev;     /* nslots > 1 */
  int64_t max_B;                         /* nslots > 1 */
  const hcg_epoch_draw_args* epoch_draw; /* HOST pointer; NULL = a collate */
} hcg_collate_args;
int hcg_collate(const hcg_collate_args* args_host, hcg_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* HCATGNET_HIP_H */
