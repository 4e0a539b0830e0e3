"""ctypes binding of libhcatgnet_hip.so (the C ABI declared in include/hcatgnet_hip.h).

There is NO CPU fallback: if the library is missing, or a tensor is not on an MI355X, every
entry point raises.  (The CPU oracle under oracle/ is test infrastructure and is never imported
from this package.)
"""
from __future__ import annotations

import ctypes
import os
from ctypes import c_char_p, c_float, c_int, c_int64, c_size_t, c_void_p

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "csrc", "libhcatgnet_hip.so")

HCG_PLAN_GENERAL, HCG_PLAN_BLOCKED, HCG_PLAN_PTRS_ONLY, HCG_PLAN_KEEP_STATUS = 0, 1, 2, 4
HCG_ACT_NONE, HCG_ACT_LEAKY = 0, 1
HCG_LOSS_MSE, HCG_LOSS_RMSE, HCG_LOSS_SSE = 0, 1, 2      # loss modes of hcg_step_tail / hcg_loss_finalize / hcg_loss_fwd_bwd
HCG_LOSS_CE = 3                                          # ... cross-entropy (hcg_step_tail / hcg_loss_finalize; count = B)
HCG_LOSS_CE_CLASSES_SHIFT = 8                            # hcg_loss_fwd_bwd: mode = HCG_LOSS_CE | (C << shift), n = B * C
HCG_HEAD_FORWARD_ONLY, HCG_HEAD_LOSS_CE = 1, 2           # flags of hcg_head_fwd_bwd / hcg_head_deep_fwd_bwd
HCG_WS_PLAN, HCG_WS_LINEAR, HCG_WS_GCN_LAYER_BWD, HCG_WS_READOUT2, HCG_WS_HEAD_DEEP = 0, 1, 2, 3, 4   # hcg_general_workspace_bytes kinds
HCG_FUSED_POOLBITS, HCG_FUSED_HEAD_WS = 0, 1                                          # hcg_fused_aux_bytes kinds
HCG_STRUCT_REDUCE_JOB, HCG_STRUCT_TAIL_ARGS, HCG_STRUCT_FUSED_FWD_ARGS, HCG_STRUCT_COLLATE_ARGS, HCG_STRUCT_COLLATE_SLOT = 0, 1, 2, 3, 4   # hcg_struct_bytes
HCG_STRUCT_UPDATE_ARGS, HCG_STRUCT_HEAD_ARGS, HCG_STRUCT_EXPLAIN_ARGS = 5, 6, 7
HCG_STRUCT_FIT_CONTROL_ARGS, HCG_STRUCT_FIT_STATE = 8, 9
HCG_STRUCT_EPOCH_DRAW_ARGS, HCG_STRUCT_PCG64 = 10, 11
HCG_EPOCH_DRAW_MAX_GRAPHS = 8192                         # graphs one hcg_collate draw launch takes (its workgroup's LDS)
HCG_EXPLAIN_GRAPHS, HCG_EXPLAIN_LAYER_EDGE_GRAD, HCG_EXPLAIN_ENSEMBLE, HCG_EXPLAIN_SHAPLEY, HCG_EXPLAIN_FIT = 0, 1, 2, 3, 4   # modes of hcg_explain
HCG_EXPLAIN_INTEGRATED = 5
HCG_EXPLAIN_MOMENTS = 6          # mean / std over the model axis of HCG_EXPLAIN_INTEGRATED's outputs with n_models > 1
HCG_EXPLAIN_COALITIONS = 7      # every subset of a graph's live groups evaluated (`COALITION_FIELDS` behind the `shap_` fields)
HCG_EXPLAIN_SUBSETS = 8         # a list of subsets of a graph's groups evaluated (`SUBSET_FIELDS` behind the `coal_` fields)
HCG_EXPLAIN_GREEDY = 9          # one round of the greedy insertion / deletion order of a graph's groups (`GREEDY_FIELDS`, `GREEDY_SLOTS`)
HCG_GREEDY_DELETION, HCG_GREEDY_NEGATE = 1, 2     # its `greedy_flags`
HCG_EXPLAIN_QUERY, HCG_EXPLAIN_SIGMOID, HCG_EXPLAIN_MAX_CONVS = 1, 2, 4  # its flags; conv layers of the one-launch kernel
HCG_EXPLAIN_TARGET_CLASS = 4     # flag: the `target` slot holds int64 class indices [B] (the header's `target_class`)
HCG_EXPLAIN_GROUPED = 8          # flag of HCG_EXPLAIN_SHAPLEY: groups of features are the players (`SHAPLEY_GROUP_FIELDS`)
HCG_ERR_UNSUPPORTED = -3
HCG_FUSED_FORWARD, HCG_FUSED_BWD_PAIR, HCG_FUSED_PAIR_QUERY = 0, 1, 1      # modes of hcg_fused_forward's block; the pair's flag
HCG_HEAD_MAX_LAYERS = 4
HCG_UPDATE_ADAM, HCG_UPDATE_SGD, HCG_UPDATE_RMSPROP = 0, 1, 2      # update rules of hcg_step_tail / hcg_update_dev
HCG_REDUCE_MAX_JOBS, HCG_REDUCE_MAX_SEGS = 8, 4
HCG_XCHG_MEAN, HCG_XCHG_SSE, HCG_XCHG_ERR_TIMEOUT, HCG_XCHG_MAX_WORLD = 0, 1, 1, 8
STATUS_BITS = {1: "edge_index entry outside [0, N)", 2: "batch vector not sorted (non-decreasing)",
               4: "batch id outside [0, num_graphs)", 8: "edges not grouped by graph / edge crosses graphs",
               16: "a graph exceeds the fused-kernel tile",
               32: "explicit self-loop edge together with edge_weight (its weight as loop weight is not implemented)"}
STATUS_EDGE_UNGROUPED = 8

P, I64, SZ, F32, INT = c_void_p, c_int64, c_size_t, c_float, c_int
F64 = ctypes.c_double
I32 = ctypes.c_int32


# ---- host structs of the C ABI (include/hcatgnet_hip.h); tests/test_host_cpu.py checks their sizes against the library
class ReduceSeg(ctypes.Structure):
    _fields_ = [("begin", I32), ("count", I32), ("row_in", I32), ("row_out", I32), ("dst", P)]


class ReduceJob(ctypes.Structure):
    _fields_ = [("slabs", P), ("sse_part", P), ("nslabs", I32), ("slab_floats", I32), ("nseg", I32), ("reserved", I32),
                ("seg", ReduceSeg * HCG_REDUCE_MAX_SEGS)]


class TailArgs(ctypes.Structure):
    """hcg_tail_args: the step's last launch (slab reductions, loss + deferred scale, exchange, update, next plan)."""
    _fields_ = [("jobs_host", P), ("njobs", I32), ("loss_mode", I32), ("loss_count", F32), ("beta1", F32), ("beta2", F32),
                ("eps", F32), ("loss", P), ("sse_tail", P), ("grad_flat", P), ("param", P), ("exp_avg", P), ("exp_avg_sq", P),
                ("n", I64), ("lr_dev", P), ("step_dev", P), ("next_edge_index", P), ("next_batch", P), ("next_N", I64),
                ("next_E", I64), ("next_B", I64), ("next_graph_ptr", P), ("next_edge_ptr", P), ("next_status", P), ("inbox", P),
                ("peers_host", P), ("rank", I32), ("world", I32), ("xchg_mode", I32), ("update_rule", I32), ("xchg_err", P)]


class FitState(ctypes.Structure):
    """hcg_fit_state: the fit controller's DEVICE state (scheduler, early stopping, counters); the host initialises it and
    reads it back."""
    _fields_ = [("lr", F64), ("sched_best", F64), ("val_best", F64), ("epoch", I32), ("num_bad_epochs", I32),
                ("cooldown_counter", I32), ("last_epoch", I32), ("best_epoch", I32), ("stall", I32), ("stopped", I32),
                ("epochs_counted", I32)]


class FitControlArgs(ctypes.Structure):
    """hcg_fit_control_args: one launch of the fit controller behind an epoch's train / validation / test graphs."""
    _fields_ = [("sums", P * 3), ("denom", F64 * 3), ("state", P), ("lr_dev", P), ("param", P), ("best", P), ("n", I64),
                ("log", P), ("factor", F64), ("rel_epsilon", F64), ("min_lr", F64), ("eps", F64), ("patience", I32),
                ("cooldown", I32), ("control_every", I32), ("early_stopping", I32), ("max_epochs", I32), ("reserved", I32)]


class UpdateArgs(ctypes.Structure):
    """hcg_update_args: every rule's capturable update, plain or in the data-parallel SSE form; or, with `fit_control`
    (the host address of a `FitControlArgs`), the fit controller's launch."""
    _fields_ = [("param", P), ("grad", P), ("exp_avg", P), ("exp_avg_sq", P), ("n", I64), ("lr_dev", P), ("step_dev", P),
                ("loss", P), ("beta1", F32), ("beta2", F32), ("eps", F32), ("update_rule", I32), ("fit_control", P)]


class FusedFwdArgs(ctypes.Structure):
    """hcg_fused_fwd_args: every forward form of the small-graph tiles."""
    _fields_ = [("x", P), ("W1", P), ("b1", P), ("W2", P), ("b2", P), ("edge_index", P), ("E", I64), ("graph_ptr", P),
                ("edge_ptr", P), ("N", I64), ("B", I64), ("F", I64), ("D", I64), ("graphs_per_tile", I32), ("apply_act", I32),
                ("slope", F32), ("head_flags", I32), ("out1", P), ("out2", P), ("emb", P), ("poolbits", P), ("status", P),
                ("y", P), ("head_W0", P), ("head_b0", P), ("head_W1", P), ("head_b1", P), ("C", I64), ("z", P), ("out", P),
                ("demb", P), ("head_workspace", P), ("head_workspace_bytes", SZ), ("step_counter", P),
                # mode HCG_FUSED_BWD_PAIR: two conv layers' backward in one launch
                ("mode", I32), ("pair_flags", I32), ("pair_dx", P), ("pair_dout", P), ("pair_ws_upper", P),
                ("pair_ws_upper_bytes", SZ), ("pair_ws_lower", P), ("pair_ws_lower_bytes", SZ), ("pair_act_upper", I32),
                ("pair_act_lower", I32), ("pair_graphs_per_tile_upper", I32), ("pair_reserved", I32)]


class HeadArgs(ctypes.Structure):
    """hcg_head_args: the one-launch readout head of depth 1, 3 or 4 (hcg_head_deep_fwd_bwd)."""
    _fields_ = [("emb", P), ("y", P), ("W", P * HCG_HEAD_MAX_LAYERS), ("b", P * HCG_HEAD_MAX_LAYERS), ("out", P), ("demb", P),
                ("workspace", P), ("workspace_bytes", SZ), ("step_counter", P), ("grad", P * HCG_HEAD_MAX_LAYERS), ("B", I64), ("D", I64), ("C", I64), ("R", I32),
                ("flags", I32), ("slope", F32), ("reserved", I32)]


class ExplainArgs(ctypes.Structure):
    """hcg_explain_args: a batch of graphs explained in one launch, one any-shape layer's edge-multiplier gradient, an
    ensemble of models predicting one batch in one launch, Shapley value sampling of a batch of graphs, the whole
    GNNExplainer mask fit of a batch of graphs, or its integrated gradients.  The header's `path_` fields
    (HCG_EXPLAIN_INTEGRATED) share the storage of the `fit_` block through a union; here they are the `_Overlay` attributes
    attached below (`PATH_FIELDS`), so `_fields_`, the size and every offset stay what they were.  The `mom_` fields
    (HCG_EXPLAIN_MOMENTS, `MOMENT_FIELDS`) are the union's third block and the `shap_` fields (HCG_EXPLAIN_SHAPLEY with
    HCG_EXPLAIN_GROUPED, `SHAPLEY_GROUP_FIELDS`) its fourth, attached the same way; the `coal_` fields (HCG_EXPLAIN_COALITIONS,
    `COALITION_FIELDS`) follow the `shap_` fields in that fourth block and the `sub_` fields (HCG_EXPLAIN_SUBSETS,
    `SUBSET_FIELDS`) the `coal_` fields; `greedy_round` / `greedy_flags` (HCG_EXPLAIN_GREEDY, `GREEDY_FIELDS`) follow the `sub_`
    fields and fill the block, and that mode's two pointers take slots it does not read otherwise (`GREEDY_SLOTS`)."""
    _fields_ = [("mode", I32), ("flags", I32), ("x", P), ("edge_index", P), ("graph_ptr", P), ("edge_ptr", P), ("edge_mask", P),
                ("node_mask", P), ("target", P), ("dout", P), ("conv_W", P * HCG_EXPLAIN_MAX_CONVS),
                ("conv_b", P * HCG_EXPLAIN_MAX_CONVS), ("head_W", P * HCG_HEAD_MAX_LAYERS), ("head_b", P * HCG_HEAD_MAX_LAYERS),
                ("out", P), ("loss", P), ("d_edge_mask", P), ("d_node_mask", P), ("dx", P), ("status", P), ("workspace", P),
                ("workspace_bytes", SZ), ("workspace_bytes_needed", SZ), ("N", I64), ("E", I64), ("B", I64), ("F", I64), ("D", I64),
                ("C", I64), ("max_nodes", I64), ("max_edges", I64), ("n_conv", I32), ("R", I32), ("slope", F32), ("apply_act", I32),
                ("layer_dout", P), ("layer_out", P), ("layer_h", P), ("rowptr", P), ("col", P), ("dinv", P), ("dew_csr", P),
                ("emb", P), ("n_models", I32), ("models_per_group", I32), ("perm", P), ("out_base", P), ("shap_acc", P),
                ("n_perm", I32), ("perm_first", I32), ("perm_count", I32), ("class_index", I32),
                ("lds_bytes", I32), ("reserved", I32),
                ("fit_edge_logit", P), ("fit_edge_exp_avg", P), ("fit_edge_exp_avg_sq", P), ("fit_edge_hard", P),
                ("fit_node_logit", P), ("fit_node_exp_avg", P), ("fit_node_exp_avg_sq", P), ("fit_node_hard", P),
                ("fit_hard_count", P), ("fit_loss_hist", P), ("fit_edge_mask_out", P), ("fit_node_mask_out", P),
                ("step_first", I32), ("epoch_count", I32), ("fit_lr", F32), ("fit_beta1", F32), ("fit_beta2", F32),
                ("fit_eps", F32), ("fit_coeffs", F32 * 4)]


class _Overlay:
    """A member of a union in the header that the ctypes mirror does not list in `_fields_`: a value of `ctype` at a fixed
    byte `offset` of the structure, read and written like a field (None / int for a pointer)."""

    def __init__(self, ctype, offset: int):
        self.ctype, self.offset, self.size = ctype, int(offset), ctypes.sizeof(ctype)

    def __get__(self, obj, owner=None):
        return self if obj is None else self.ctype.from_address(ctypes.addressof(obj) + self.offset).value

    def __set__(self, obj, value):
        self.ctype.from_address(ctypes.addressof(obj) + self.offset).value = value


# hcg_explain_args' HCG_EXPLAIN_INTEGRATED members, in the header's order, from the offset of `fit_edge_logit` on
PATH_FIELDS = (("path_alpha", P), ("path_weight", P), ("path_node_attr", P), ("path_edge_attr", P), ("path_out_full", P),
               ("path_out_base", P), ("path_steps", I32), ("path_step_first", I32), ("path_step_count", I32),
               ("path_class_index", I32))


# hcg_explain_args' HCG_EXPLAIN_MOMENTS members (the union's third block), in the header's order from the same offset; the
# header's two-element arrays are one attribute per element here (`mom_values0`, `mom_values1`, ...)
MOMENT_FIELDS = tuple((f"{name}{s}", ctype) for name, ctype in (("mom_values", P), ("mom_mean", P), ("mom_m2", P), ("mom_std", P),
                                                                 ("mom_len", I64)) for s in (0, 1)) + \
    (("mom_total", I32), ("mom_first", I32), ("mom_count", I32), ("mom_reserved", I32))


def _attach_union_fields(fields):
    off = ExplainArgs.fit_edge_logit.offset
    for name, ctype in fields:
        align = ctypes.alignment(ctype)
        off = (off + align - 1) // align * align
        setattr(ExplainArgs, name, _Overlay(ctype, off))
        off += ctypes.sizeof(ctype)
    assert off <= ctypes.sizeof(ExplainArgs)


# hcg_explain_args' members of HCG_EXPLAIN_SHAPLEY with HCG_EXPLAIN_GROUPED (the union's fourth block), from the same offset
SHAPLEY_GROUP_FIELDS = (("shap_group_ptr", P), ("shap_member_ptr", P), ("shap_members", P), ("shap_bg_ptr", P),
                        ("shap_bg_members", P), ("shap_n_groups", I64))

# what HCG_EXPLAIN_COALITIONS reads behind them, in the same block
COALITION_FIELDS = (("coal_values", P), ("coal_jobs", P), ("coal_live_ptr", P), ("coal_rows", I64), ("coal_job_first", I32),
                    ("coal_job_count", I32), ("coal_max_live", I32), ("coal_reserved", I32))

# what HCG_EXPLAIN_SUBSETS adds behind those (it reads coal_values / coal_jobs / coal_rows / coal_job_first / coal_job_count too)
SUBSET_FIELDS = (("sub_bits", P), ("sub_word_ptr", P), ("sub_member_group", P), ("sub_max_groups", I32), ("sub_reserved", I32))

# what HCG_EXPLAIN_GREEDY adds behind those (it reads the shap_ fields, coal_values / coal_jobs / coal_job_first /
# coal_job_count and sub_member_group / sub_max_groups too); the block is full with them
GREEDY_FIELDS = (("greedy_round", I32), ("greedy_flags", I32))

# ... and its two pointers, which the header declares in a union with a field the mode does not read: name -> that field
GREEDY_SLOTS = (("greedy_order", "coal_live_ptr"), ("greedy_cand", "sub_bits"))


_attach_union_fields(PATH_FIELDS)
_attach_union_fields(MOMENT_FIELDS)
_attach_union_fields(SHAPLEY_GROUP_FIELDS +COALITION_FIELDS + SUBSET_FIELDS + GREEDY_FIELDS)
for _name, _slot in GREEDY_SLOTS:
    setattr(ExplainArgs, _name, _Overlay(P, getattr(ExplainArgs, _slot).offset))


class CollateSlot(ctypes.Structure):
    """hcg_collate_slot: one batch of a collate launch."""
    _fields_ = [("ids", P), ("graph_ptr", P), ("edge_ptr", P), ("x_out", P), ("edge_index_out", P), ("batch_out", P),
                ("y_out", P), ("idx_out", P), ("B", I64), ("N_out", I64), ("E_out", I64)]


class Pcg64(ctypes.Structure):
    """hcg_pcg64: numpy's PCG64 state in DEVICE memory (`np.random.PCG64().state`, the 128-bit integers as two words)."""
    _fields_ = [("state_lo", ctypes.c_uint64), ("state_hi", ctypes.c_uint64), ("inc_lo", ctypes.c_uint64),
                ("inc_hi", ctypes.c_uint64), ("has_uint32", ctypes.c_uint32), ("uinteger", ctypes.c_uint32)]


class EpochDrawArgs(ctypes.Structure):
    """hcg_epoch_draw_args: one epoch's permutation and index arrays drawn on the device (csrc/shuffle.hip)."""
    _fields_ = [("rng", P), ("layout", P), ("gate", P), ("G", I64), ("batch_size", I32), ("drop_last", I32),
                ("gate_max_epochs", I32), ("reserved", I32)]


class CollateArgs(ctypes.Structure):
    """hcg_collate_args: the dataset + one slot (host values) or a device array of slots; or, with `epoch_draw` (the host
    address of an `EpochDrawArgs`), the draw launch."""
    _fields_ = [("x_all", P), ("src_all", P), ("dst_all", P), ("node_ptr_all", P), ("edge_ptr_all", P), ("y_all", P),
                ("idx_all", P), ("F", I64), ("nslots", I32), ("reserved", I32), ("slot", CollateSlot), ("slots_dev", P),
                ("max_B", I64), ("epoch_draw", P)]


# name -> (restype, argtypes); must list every symbol of include/hcatgnet_hip.h
SIGNATURES = {
    "hcg_version": (INT, []),
    "hcg_struct_bytes": (SZ, [INT]),
    "hcg_general_workspace_bytes": (SZ, [INT, I64, I64, I64, INT]),
    "hcg_fused_aux_bytes": (SZ, [INT, I64, INT]),
    "hcg_error_string": (c_char_p, [INT]),
    "hcg_plan_build": (INT, [P, P, P, I64, I64, I64, F32, INT, P, P, P, P, P, P, P, P, P, P, P, P, P, P, SZ, P]),
    "hcg_linear_fwd": (INT, [P, P, P, P, I64, I64, I64, INT, F32, P]),
    "hcg_linear_bwd": (INT, [P, P, P, P, P, P, P, P, I64, I64, I64, INT, F32, P, SZ, P]),
    "hcg_gcn_layer_fwd": (INT, [P, P, P, P, P, P, P, F32, F32, INT, P, P, I64, I64, I64, I64, P]),
    "hcg_gcn_layer_bwd": (INT, [P, P, P, P, P, P, P, P, F32, F32, INT, P, P, P, P, I64, I64, I64, I64, P, SZ, P]),
    "hcg_explain": (INT, [P, P]),
    "hcg_pool_fwd": (INT, [P, P, P, I64, I64, I64, P]),
    "hcg_pool_bwd": (INT, [P, P, P, P, P, I64, I64, I64, P]),
    "hcg_fused_graphs_per_tile": (INT, [I64, I64, I64]),
    "hcg_fused_workspace_bytes": (SZ, [I64, I64, I64, INT]),
    "hcg_fused_forward": (INT, [P, P]),
    "hcg_fused_head_reduce_job": (INT, [P, SZ, I64, INT, I64, P, P, P, P, P]),
    "hcg_fused_layer_bwd": (INT, [P, P, P, P, P, P, P, P, I64, P, P, I64, I64, I64, I64, INT, F32, INT, P, P, P, SZ, P]),
    "hcg_mid_supported": (INT, [I64, I64, I64, I64]),
    "hcg_mid_workspace_bytes": (SZ, [I64, I64, I64, I64, I64]),
    "hcg_mid_layer_fwd": (INT, [P, P, P, P, I64, P, P, I64, I64, I64, I64, I64, I64, F32, INT, P, P, P, P, P, P, P]),
    "hcg_mid_layer_bwd": (INT, [P, P, P, P, P, P, P, I64, P, P, I64, I64, I64, I64, I64, I64, F32, INT, P, P, P, SZ, P]),
    "hcg_mid_reduce_job": (INT, [P, SZ, I64, I64, I64, I64, I64, INT, P, P, P]),
    "hcg_tall_supported": (INT, [I64, I64, I64, I64]),
    "hcg_tall_workspace_bytes": (SZ, [I64, I64, I64, I64]),
    "hcg_tall_layer_fwd": (INT, [P, P, P, P, I64, P, P, I64, I64, I64, I64, I64, I64, F32, INT, P, P, P, P, P, P, P, SZ, P]),
    "hcg_tall_layer_bwd": (INT, [P, P, P, P, P, P, P, P, P, P, P, I64, P, P, I64, I64, I64, I64, I64, I64, F32, INT, P, P, P, SZ, P]),
    "hcg_tall_reduce_jobs": (INT, [P, SZ, I64, I64, I64, I64, INT, P, P, P]),
    "hcg_fused_reduce_job": (INT, [P, SZ, I64, I64, I64, I64, INT, P, P, P]),
    "hcg_readout2_bwd_partial": (INT, [P, P, P, P, P, I64, I64, I64, F32, P, P, SZ, P, P, P, P, P, P]),
    "hcg_reduce_job_append": (INT, [P, P]),
    "hcg_step_tail": (INT, [P, P]),
    "hcg_loss_finalize": (INT, [P, F32, INT, P, P, P]),
    "hcg_collate": (INT, [P, P]),
    "hcg_adam_step": (INT, [P, P, P, P, I64, F32, F32, F32, F32, I64, P]),
    "hcg_mse_fwd": (INT, [P, P, I64, P, P]),
    "hcg_mse_bwd": (INT, [P, P, P, I64, P, P, P]),
    "hcg_loss_fwd_bwd": (INT, [P, P, I64, INT, P, P, P, P]),
    "hcg_readout2_fwd": (INT, [P, P, P, P, P, I64, I64, I64, F32, P, P, P]),
    "hcg_head_supported": (INT, [I64, I64]),
    "hcg_head_workspace_bytes": (SZ, [I64, I64]),
    "hcg_head_fwd_bwd": (INT, [P, P, P, P, P, P, I64, I64, I64, F32, INT, P, P, P, P, SZ, P, P]),
    "hcg_head_reduce_job": (INT, [P, SZ, I64, I64, I64, P, P, P, P, P]),
    "hcg_head_deep_fwd_bwd": (INT, [P, P, P]),
    "hcg_adam_step_dev_sse": (INT, [P, P, P, P, I64, P, F32, F32, F32, P, P, P]),
    "hcg_adam_step_dev": (INT, [P, P, P, P, I64, P, F32, F32, F32, P, P]),
    "hcg_update_dev": (INT, [P, P]),
    "hcg_xchg_inbox_bytes": (SZ, [I64, INT]),
    "hcg_xchg_resident_blocks": (INT, []),
    "hcg_xchg_alloc": (INT, [SZ, P]),
    "hcg_xchg_free": (INT, [P]),
    "hcg_xchg_zero": (INT, [P, SZ]),
    "hcg_xchg_ipc_export": (INT, [P, P]),
    "hcg_xchg_ipc_open": (INT, [P, P]),
    "hcg_xchg_ipc_close": (INT, [P]),
}

_lib = None


class HcgError(RuntimeError):
    pass


def load():
    """Load (once) and return the ctypes library; raises if it has not been built."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.isfile(LIB_PATH):
        raise HcgError(
            f"{LIB_PATH} not found: build it with `python -c 'import __graft_entry__ as g; g.build()'` "
            "(or `make -C hcatgnet_amd/csrc`). hcatgnet_amd has no CPU/PyTorch fallback.")
    lib = ctypes.CDLL(LIB_PATH)
    for name, (res, args) in SIGNATURES.items():
        fn = getattr(lib, name)  # AttributeError here = ABI/header drift: fail loudly
        fn.restype = res
        fn.argtypes = args
    if lib.hcg_version() != 1:
        raise HcgError(f"ABI version mismatch: library reports {lib.hcg_version()}, binding expects 1")
    _lib = lib
    return lib


def check(rc: int, what: str):
    if rc != 0:
        msg = load().hcg_error_string(rc)
        raise HcgError(f"{what} failed: {msg.decode() if msg else rc} (code {rc})")


def ptr(t):
    """Device pointer of a tensor (None -> NULL)."""
    return None if t is None else t.data_ptr()


_raw_stream = None
_gpu_ok = None


def stream_ptr():
    """hipStream_t of torch's CURRENT stream on the current device (so that work enqueued here is
    ordered with the surrounding torch ops, also under torch.cuda.graph capture on a side stream).
    `torch._C._cuda_getCurrentRawStream` is the cheap accessor (~1 us vs ~11 us for the Stream object)."""
    global _raw_stream
    import torch
    if _raw_stream is None:
        _raw_stream = getattr(torch._C, "_cuda_getCurrentRawStream", False)
    if _raw_stream:
        return _raw_stream(torch.cuda.current_device())
    return torch.cuda.current_stream().cuda_stream


def require_gpu(*tensors):
    """Every tensor on the GPU -- and on the CURRENT device: the library enqueues on the current device's stream, a
    pointer into another GPU's memory would fault there."""
    global _gpu_ok
    cur = None
    for t in tensors:
        if t is None:
            continue
        if not t.is_cuda:
            raise HcgError("hcatgnet_amd runs on MI355X (ROCm) tensors only; got a CPU tensor. "
                           "There is no CPU fallback: move the model and the batch to the GPU.")
        if cur is None:
            import torch
            cur = torch.cuda.current_device()
        if t.device.index != cur:
            raise HcgError(f"tensor on cuda:{t.device.index} but the current device is cuda:{cur}: "
                           "call torch.cuda.set_device (one process per GPU) before using hcatgnet_amd")
    if _gpu_ok is None:
        import torch
        _gpu_ok = bool(torch.cuda.is_available())
    if not _gpu_ok:
        raise HcgError("no ROCm GPU visible")


def describe_status(word: int) -> str:
    return "; ".join(msg for bit, msg in STATUS_BITS.items() if word & bit) or "ok"


# ---- struct-argument entry points ------------------------------------------------------------------------------------
def fused_forward(**kw):
    """hcg_fused_forward: keyword = field of hcg_fused_fwd_args (tensors or None for pointers, numbers otherwise)."""
    a = FusedFwdArgs()
    for k, v in kw.items():
        setattr(a, k, v.data_ptr() if hasattr(v, "data_ptr") else v)
    check(load().hcg_fused_forward(ctypes.addressof(a), stream_ptr()), "hcg_fused_forward")


def fused_bwd_pair(query: bool = False, **kw) -> bool:
    """Mode HCG_FUSED_BWD_PAIR of hcg_fused_forward (keywords as `fused_forward`).  `query`: validate only (the GPU is not
    touched) -> whether the pair applies; otherwise launch, and raise on any error."""
    a = FusedFwdArgs()
    for k, v in kw.items():
        setattr(a, k, v.data_ptr() if hasattr(v, "data_ptr") else v)
    a.mode, a.pair_flags = HCG_FUSED_BWD_PAIR, (HCG_FUSED_PAIR_QUERY if query else 0)
    rc = load().hcg_fused_forward(ctypes.addressof(a), None if query else stream_ptr())
    if query and rc == HCG_ERR_UNSUPPORTED:
        return False
    check(rc, "hcg_fused_forward (backward pair)")
    return True


def step_tail(jobs_addr: int, njobs: int, *, loss=None, loss_mode: int = HCG_LOSS_RMSE, loss_count: float = 0.0, sse_tail=None,
              update=None, next_plan=None, xchg=None):
    """hcg_step_tail.  `jobs_addr`: host address of `njobs` hcg_reduce_job; `loss` [2] / `sse_tail` [2] device tensors;
    `update`: dict(rule (HCG_UPDATE_*), grad_flat, param, exp_avg, exp_avg_sq (tensors, None where the rule keeps no such
    state), n, lr_dev, step_dev (tensors), beta1, beta2, eps);
    `next_plan`: a pointers-only blocked BatchPlan; `xchg`: dict(inbox (address), peers_host (address of the host pointer
    array), rank, world, mode, err (tensor))."""
    a = TailArgs()
    a.jobs_host, a.njobs, a.loss_mode, a.loss_count = jobs_addr, njobs, loss_mode, float(loss_count)
    a.loss, a.sse_tail = ptr(loss), ptr(sse_tail)
    if update is not None:
        u = update
        a.update_rule = u["rule"]
        a.grad_flat, a.param, a.exp_avg, a.exp_avg_sq = (u["grad_flat"].data_ptr(), u["param"].data_ptr(),
                                                         ptr(u.get("exp_avg")), ptr(u.get("exp_avg_sq")))
        a.n, a.lr_dev, a.step_dev = u["n"], u["lr_dev"].data_ptr(), u["step_dev"].data_ptr()
        a.beta1, a.beta2, a.eps = u["beta1"], u["beta2"], u["eps"]
    if next_plan is not None:
        np_ = next_plan
        a.next_edge_index, a.next_batch = np_.edge_index.data_ptr(), np_.batch.data_ptr()
        a.next_N, a.next_E, a.next_B = np_.N, np_.E, np_.B
        a.next_graph_ptr, a.next_edge_ptr, a.next_status = np_.graph_ptr.data_ptr(), np_.edge_ptr.data_ptr(), np_.status.data_ptr()
    if xchg is not None:
        a.inbox, a.peers_host, a.rank, a.world, a.xchg_mode = xchg["inbox"], xchg["peers_host"], xchg["rank"], xchg["world"], xchg["mode"]
        a.xchg_err = xchg["err"].data_ptr()
    check(load().hcg_step_tail(ctypes.addressof(a), stream_ptr()), "hcg_step_tail")


def update_dev(grad, *, rule: int = HCG_UPDATE_ADAM, param=None, exp_avg=None, exp_avg_sq=None, n: int = 0, lr_dev=None,
               step_dev=None, beta1: float = 0.0, beta2: float = 0.0, eps: float = 0.0, loss=None):
    """hcg_update_dev: the capturable update of rule `rule` (HCG_UPDATE_*) on `n` elements; `loss` set = the SSE form
    (`grad` = [n gradients | SSE | count], scaled in place); `param` None = that scale and the loss alone."""
    a = UpdateArgs()
    a.param, a.grad, a.exp_avg, a.exp_avg_sq = ptr(param), grad.data_ptr(), ptr(exp_avg), ptr(exp_avg_sq)
    a.n, a.lr_dev, a.step_dev, a.loss = n, ptr(lr_dev), ptr(step_dev), ptr(loss)
    a.beta1, a.beta2, a.eps, a.update_rule = beta1, beta2, eps, rule
    check(load().hcg_update_dev(ctypes.addressof(a), stream_ptr()), "hcg_update_dev")


def fit_control(args: FitControlArgs, stream=None):
    """The fit controller (csrc/fit.hip: k_fit_control) on `stream` (default: the current one): hcg_update_dev with its
    `fit_control` set -- the ABI's symbol count is capped, so the controller has no symbol of its own."""
    a = UpdateArgs()
    a.fit_control = ctypes.addressof(args)
    check(load().hcg_update_dev(ctypes.addressof(a), stream_ptr() if stream is None else stream), "hcg_update_dev (fit control)")


def epoch_draw(dataset: CollateArgs, draw: EpochDrawArgs, stream=None):
    """One epoch's shuffle and index arrays (csrc/shuffle.hip: k_epoch_draw) on `stream` (default: the current one):
    hcg_collate with its `epoch_draw` set, `dataset` lending node_ptr_all / edge_ptr_all -- like the fit controller the
    launch has no symbol of its own."""
    a = CollateArgs.from_buffer_copy(dataset)
    a.epoch_draw = ctypes.addressof(draw)
    check(load().hcg_collate(ctypes.byref(a), stream_ptr() if stream is None else stream), "hcg_collate (epoch draw)")


def layer_edge_grad(dout, out, h, rowptr, col, dinv, slope: float, apply_act: int, dew_csr, N: int, E: int, D: int):
    """hcg_explain, mode HCG_EXPLAIN_LAYER_EDGE_GRAD: d / d ew_csr of one any-shape conv layer (explain mode)."""
    a = ExplainArgs()
    a.mode = HCG_EXPLAIN_LAYER_EDGE_GRAD
    a.layer_dout, a.layer_out, a.layer_h = ptr(dout), ptr(out), ptr(h)
    a.rowptr, a.col, a.dinv, a.dew_csr = ptr(rowptr), ptr(col), ptr(dinv), ptr(dew_csr)
    a.slope, a.apply_act, a.N, a.E, a.D = slope, apply_act, N, E, D
    check(load().hcg_explain(ctypes.addressof(a), stream_ptr()), "hcg_explain (layer edge gradient)")


def ce_fwd_bwd(logits, labels, loss, dout=None):
    """hcg_loss_fwd_bwd in its cross-entropy mode: `logits` [B, C], `labels` [B] float32 class indices -> loss[0] = loss[1] =
    nn.CrossEntropyLoss()(logits, labels.long()), `dout` (optional) = its gradient."""
    B, C = logits.shape
    check(load().hcg_loss_fwd_bwd(ptr(logits), ptr(labels), B * C, HCG_LOSS_CE | (C << HCG_LOSS_CE_CLASSES_SHIFT), ptr(loss),
                                  ptr(dout), None, stream_ptr()), "hcg_loss_fwd_bwd (cross-entropy)")


def job_bytes() -> int:
    """sizeof(hcg_reduce_job): the stride of a host array of jobs (tests/test_host_cpu.py checks the mirror against the library)."""
    return ctypes.sizeof(ReduceJob)


def reduce_jobs(jobs_addr: int, njobs: int):
    """The slab reductions alone (no loss scale, no update)."""
    step_tail(jobs_addr, njobs)
