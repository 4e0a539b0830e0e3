"""autograd Functions over the C ABI: GCN layer, graph pooling, dense linear.

These stand in for what the reference reaches through torch_geometric + torch autograd:
`GCNConv.forward` (gcn_norm, Linear, propagate: gather / message / scatter_add, bias) followed by
LeakyReLU (model/gcn.py:58-63), `global_max_pool` / `global_mean_pool` (model/gcn.py:65-66), the
readout Linear(+LeakyReLU) stack (model/gcn.py:70-71) and `loss.backward()` through them
(utils/utils_model.py:65).  All arithmetic runs in libhcatgnet_hip.so; torch only owns memory.
"""
from __future__ import annotations

import ctypes
from types import SimpleNamespace
from typing import NamedTuple, Optional

import torch

from . import _lib
from .plan import BatchPlan

LEAKY_SLOPE = 0.01  # nn.LeakyReLU() default (reference model/gcn.py:21, :63)


def _f32c(t: torch.Tensor) -> torch.Tensor:
    if t.dtype != torch.float32:
        raise _lib.HcgError(f"hcatgnet_amd computes in float32; got {t.dtype}")
    return t.contiguous()


class _GCNLayerFn(torch.autograd.Function):
    """out = leaky_relu( Ahat (x W^T) + b ), Ahat = D^-1/2 (A + fill I) D^-1/2 from the plan.
    `edge_mult` (optional, [E] in the caller's edge order, may require grad): explain-mode multiplier of every
    message, applied AFTER the normalisation like PyG's Explainer edge mask (self loops keep 1)."""

    @staticmethod
    def forward(ctx, x, weight, bias, plan: BatchPlan, use_edge_weight: bool, apply_act: bool, slope: float, edge_mult=None):
        lib = _lib.load()
        _lib.require_gpu(x, weight, bias, edge_mult)
        x, weight, bias = _f32c(x), _f32c(weight), _f32c(bias)
        N, F = x.shape
        D = weight.shape[0]
        if weight.shape[1] != F or N != plan.N:
            raise ValueError(f"shape mismatch: x {tuple(x.shape)}, weight {tuple(weight.shape)}, plan N {plan.N}")
        mult_csr = mult_csc = None
        if edge_mult is not None:
            if use_edge_weight or plan.ew_csr is not None:
                raise _lib.HcgError("an edge mask cannot be combined with explicit edge weights")
            if edge_mult.numel() != plan.E:
                raise ValueError(f"edge mask has {edge_mult.numel()} entries, the batch has {plan.E} edges")
            plan.ensure_eid()
            em = _f32c(edge_mult.detach()).reshape(-1)
            mult_csr = em[plan.eid.long()[:plan.E]].contiguous() if plan.E else em
            mult_csc = em[plan.eid_t.long()[:plan.E]].contiguous() if plan.E else em
        else:
            plan.ensure_csr()
        out = torch.empty(N, D, dtype=torch.float32, device=x.device)
        h_ws = torch.empty(N, D, dtype=torch.float32, device=x.device)
        ew = plan.ew_csr if use_edge_weight else mult_csr
        fill = plan.fill if use_edge_weight else 1.0
        rc = lib.hcg_gcn_layer_fwd(_lib.ptr(x), _lib.ptr(weight), _lib.ptr(bias), _lib.ptr(plan.rowptr),
                                   _lib.ptr(plan.col), _lib.ptr(ew), _lib.ptr(ctx_dinv(plan, use_edge_weight)),
                                   fill, slope, int(apply_act), _lib.ptr(h_ws), _lib.ptr(out), N, plan.E, F, D,
                                   _lib.stream_ptr())
        _lib.check(rc, "hcg_gcn_layer_fwd")
        ctx.save_for_backward(x, weight, out, *([mult_csc, h_ws] if edge_mult is not None else []))
        ctx.plan, ctx.use_ew, ctx.apply_act, ctx.slope, ctx.masked = plan, use_edge_weight, apply_act, slope, edge_mult is not None
        return out

    @staticmethod
    def backward(ctx, dout):
        lib = _lib.load()
        saved = ctx.saved_tensors
        x, weight, out = saved[:3]
        plan = ctx.plan
        dout = _f32c(dout)
        N, F = x.shape
        D = weight.shape[0]
        dev = x.device
        dx = torch.empty_like(x) if ctx.needs_input_grad[0] else None
        dW = torch.empty_like(weight)
        db = torch.empty(D, dtype=torch.float32, device=dev)
        dh_ws = torch.empty(max(N, 1), D, dtype=torch.float32, device=dev)
        wsb = lib.hcg_general_workspace_bytes(_lib.HCG_WS_GCN_LAYER_BWD, N, F, D, 0)
        ws = torch.empty(wsb, dtype=torch.uint8, device=dev)
        ew = plan.ew_csc if ctx.use_ew else (saved[3] if ctx.masked else None)
        fill = plan.fill if ctx.use_ew else 1.0
        dinv = ctx_dinv(plan, ctx.use_ew)
        rc = lib.hcg_gcn_layer_bwd(_lib.ptr(dout), _lib.ptr(out), _lib.ptr(x), _lib.ptr(weight),
                                   _lib.ptr(plan.rowptr_t), _lib.ptr(plan.col_t), _lib.ptr(ew),
                                   _lib.ptr(dinv), fill, ctx.slope, int(ctx.apply_act),
                                   _lib.ptr(dh_ws), _lib.ptr(dx), _lib.ptr(dW), _lib.ptr(db), N, plan.E, F, D,
                                   _lib.ptr(ws), wsb, _lib.stream_ptr())
        _lib.check(rc, "hcg_gcn_layer_bwd")
        dmult = None
        if ctx.masked and ctx.needs_input_grad[7]:
            h = saved[4]                                     # x W^T of the forward
            dew = torch.zeros(max(plan.E, 1), dtype=torch.float32, device=dev)
            _lib.layer_edge_grad(dout, out, h, plan.rowptr, plan.col, dinv, ctx.slope, int(ctx.apply_act), dew, N, plan.E, D)
            dmult = torch.zeros(plan.E, dtype=torch.float32, device=dev)
            if plan.E:
                dmult[plan.eid.long()[:plan.E]] = dew[:plan.E]    # CSR order -> the caller's edge order (a permutation)
        return dx, dW, db, None, None, None, None, dmult


def ctx_dinv(plan: BatchPlan, use_edge_weight: bool):
    """dinv to use for a layer.  The reference passes `edge_weight` to conv1 only
    (model/gcn.py:58 vs :62); the other layers run unweighted with fill 1 (plan.dinv_unw)."""
    if plan.ew_csr is not None and not use_edge_weight:
        return plan.dinv_unw
    return plan.dinv


class _PoolFn(torch.autograd.Function):
    """emb = cat[global_max_pool(a), global_mean_pool(a)]  ([B, 2D], max first)."""

    @staticmethod
    def forward(ctx, a, plan: BatchPlan):
        lib = _lib.load()
        _lib.require_gpu(a)
        a = _f32c(a)
        N, D = a.shape
        emb = torch.zeros(plan.B, 2 * D, dtype=torch.float32, device=a.device)
        rc = lib.hcg_pool_fwd(_lib.ptr(a), _lib.ptr(plan.graph_ptr), _lib.ptr(emb), N, plan.B, D, _lib.stream_ptr())
        _lib.check(rc, "hcg_pool_fwd")
        ctx.save_for_backward(a, emb)
        ctx.plan = plan
        return emb

    @staticmethod
    def backward(ctx, demb):
        lib = _lib.load()
        a, emb = ctx.saved_tensors
        plan = ctx.plan
        demb = _f32c(demb)
        N, D = a.shape
        da = torch.zeros_like(a)
        rc = lib.hcg_pool_bwd(_lib.ptr(demb), _lib.ptr(a), _lib.ptr(emb), _lib.ptr(plan.graph_ptr), _lib.ptr(da), N,
                              plan.B, D, _lib.stream_ptr())
        _lib.check(rc, "hcg_pool_bwd")
        return da, None


class _LinearFn(torch.autograd.Function):
    """y = act(x W^T + b) with act in {identity, LeakyReLU}."""

    @staticmethod
    def forward(ctx, x, weight, bias, apply_act: bool, slope: float):
        lib = _lib.load()
        _lib.require_gpu(x, weight, bias)
        x, weight = _f32c(x), _f32c(weight)
        bias = _f32c(bias) if bias is not None else None
        M, K = x.shape
        O = weight.shape[0]
        if weight.shape[1] != K:
            raise ValueError(f"shape mismatch: x {tuple(x.shape)} weight {tuple(weight.shape)}")
        y = torch.empty(M, O, dtype=torch.float32, device=x.device)
        rc = lib.hcg_linear_fwd(_lib.ptr(x), _lib.ptr(weight), _lib.ptr(bias), _lib.ptr(y), M, K, O,
                                _lib.HCG_ACT_LEAKY if apply_act else _lib.HCG_ACT_NONE, slope, _lib.stream_ptr())
        _lib.check(rc, "hcg_linear_fwd")
        ctx.save_for_backward(x, weight, y)
        ctx.has_bias, ctx.apply_act, ctx.slope = bias is not None, apply_act, slope
        return y

    @staticmethod
    def backward(ctx, dy):
        lib = _lib.load()
        x, weight, y = ctx.saved_tensors
        dy = _f32c(dy)
        M, K = x.shape
        O = weight.shape[0]
        dev = x.device
        dx = torch.empty_like(x) if ctx.needs_input_grad[0] else None
        dW = torch.empty_like(weight)
        db = torch.empty(O, dtype=torch.float32, device=dev) if ctx.has_bias else None
        dz = torch.empty(max(M, 1), O, dtype=torch.float32, device=dev)
        wsb = lib.hcg_general_workspace_bytes(_lib.HCG_WS_LINEAR, M, K, O, 0)
        ws = torch.empty(wsb, dtype=torch.uint8, device=dev)
        rc = lib.hcg_linear_bwd(_lib.ptr(dy), _lib.ptr(y), _lib.ptr(x), _lib.ptr(weight), _lib.ptr(dx), _lib.ptr(dW),
                                _lib.ptr(db), _lib.ptr(dz), M, K, O,
                                _lib.HCG_ACT_LEAKY if ctx.apply_act else _lib.HCG_ACT_NONE, ctx.slope, _lib.ptr(ws), wsb,
                                _lib.stream_ptr())
        _lib.check(rc, "hcg_linear_bwd")
        return dx, dW, db, None, None


# ---- the fused conv kernel families -----------------------------------------------------------------------------------
# One launcher per family: `forward`, `backward`, `workspace_bytes` and `reduce_jobs` (describes the gradient slabs a
# backward left: -> number of hcg_reduce_job written) over a `Geometry`; `conv_route` picks the family of a layer.  Every
# caller -- the autograd Functions below and `train.FusedTrainStep` -- launches through these.
class Geometry(NamedTuple):
    """Graphs [g0, g0 + B) of a blocked plan as the conv kernels see them (device pointers as integers).  Node rows stay
    absolute: x and the activations need no offsets, graph_ptr / edge_ptr / emb / demb start at graph g0."""
    edge_index: int
    E: int
    graph_ptr: int
    edge_ptr: int
    N: int
    B: int
    max_nodes: Optional[int]
    max_edges: Optional[int]
    status: int
    g0: int


def geometry(plan: BatchPlan, g0: int = 0, B: Optional[int] = None) -> Geometry:
    """Graphs [g0, g0 + B) of `plan` (default: all graphs from g0 on)."""
    return Geometry(plan.edge_index.data_ptr(), plan.E, plan.graph_ptr.data_ptr() + 4 * g0, plan.edge_ptr.data_ptr() + 4 * g0,
                    plan.N, plan.B - g0 if B is None else B, plan.max_nodes, plan.max_edges, plan.status.data_ptr(), g0)


def _a(t):
    """Device address: a tensor's, an address as is, None -> NULL."""
    return t if t is None or t.__class__ is int else t.data_ptr()


def _graph_rows(t, geo: Geometry, D: int):
    """emb / demb [B, 2D] of the geometry's first graph on."""
    return None if t is None else t.data_ptr() + 8 * D * geo.g0


def _tiles_forward(geo, gpt, x, W, b, act, *, out=None, emb=None, poolbits=None, slope=LEAKY_SLOPE, head_out=None,
                   **fields):
    """hcg_fused_forward; `fields`: the stacked (W2, b2, out2) and head forms of hcg_fused_fwd_args (`head_out`: its `out`)."""
    _lib.fused_forward(x=x, W1=W, b1=b, edge_index=geo.edge_index, E=geo.E, graph_ptr=geo.graph_ptr, edge_ptr=geo.edge_ptr,
                       N=geo.N, B=geo.B, F=x.shape[1], D=W.shape[0], graphs_per_tile=gpt, apply_act=act, slope=slope, out1=out,
                       emb=_graph_rows(emb, geo, W.shape[0]), poolbits=poolbits, status=geo.status, out=head_out, **fields)


def _tiles_backward(geo, gpt, x, W, flags, *, dout=None, demb=None, emb=None, out=None, poolbits=None, dx=None, ws, wsb,
                    slope=LEAKY_SLOPE, stream=None):
    D = W.shape[0]
    _lib.check(_lib.load().hcg_fused_layer_bwd(
        _a(dout), _graph_rows(demb, geo, D), _graph_rows(emb, geo, D), _a(out), _a(poolbits), x.data_ptr(), W.data_ptr(), geo.edge_index,
        geo.E, geo.graph_ptr, geo.edge_ptr, geo.N, geo.B, x.shape[1], D, gpt, slope, flags, _a(dx), geo.status, _a(ws), wsb,
        _lib.stream_ptr() if stream is None else stream), "hcg_fused_layer_bwd")


def _tiles_backward_pair(geo, gpt, x, W, h, W_up, flags_up, *, gpt_up=None, dout=None, demb=None, emb=None, out=None,
                         poolbits=None, dx, ws_up=None, wsb_up=0, ws=None, wsb=0, slope=LEAKY_SLOPE, query=False) -> bool:
    """Two consecutive conv layers' backward as ONE launch (csrc/fused.hip: k_fused_bwd_pair): the upper layer (input `h`,
    weight `W_up`, `flags_up` with the premask bit; dout / demb / emb / out / poolbits as `_tiles_backward`) hands `dx`
    down to the lower one (input `x`, weight `W`).  `query`: only ask whether the pair applies (host only)."""
    D = W.shape[0]
    return _lib.fused_bwd_pair(
        query, x=x, W1=W, out1=h, W2=W_up, edge_index=geo.edge_index, E=geo.E, graph_ptr=geo.graph_ptr, edge_ptr=geo.edge_ptr,
        N=geo.N, B=geo.B, F=x.shape[1], D=D, graphs_per_tile=gpt, pair_graphs_per_tile_upper=gpt if gpt_up is None else gpt_up,
        slope=slope, out2=_a(out), emb=_graph_rows(emb, geo, D), demb=_graph_rows(demb, geo, D), poolbits=_a(poolbits),
        status=geo.status, pair_dx=_a(dx), pair_dout=_a(dout), pair_ws_upper=_a(ws_up), pair_ws_upper_bytes=wsb_up,
        pair_ws_lower=_a(ws), pair_ws_lower_bytes=wsb, pair_act_upper=flags_up, pair_act_lower=0)


def _tiles_workspace_bytes(geo, gpt, F, D) -> int:
    return _lib.load().hcg_fused_workspace_bytes(geo.B, F, D, gpt)


def _tiles_reduce_jobs(geo, gpt, F, D, ws, wsb, dW, db, job) -> int:
    _lib.check(_lib.load().hcg_fused_reduce_job(_a(ws), wsb, geo.N, geo.B, F, D, gpt, _a(dW), _a(db), job), "hcg_fused_reduce_job")
    return 1


def _mid_forward(geo, gpt, x, W, b, act, *, out=None, emb=None, poolbits=None, xagg=None, signs=None, slope=LEAKY_SLOPE,
                 stream=None):
    _lib.check(_lib.load().hcg_mid_layer_fwd(
        x.data_ptr(), W.data_ptr(), b.data_ptr(), geo.edge_index, geo.E, geo.graph_ptr, geo.edge_ptr, geo.N, geo.B, x.shape[1], W.shape[0],
        geo.max_nodes, geo.max_edges, slope, act, _a(out), _graph_rows(emb, geo, W.shape[0]), _a(poolbits), _a(xagg), _a(signs),
        geo.status, _lib.stream_ptr() if stream is None else stream), "hcg_mid_layer_fwd")


def _mid_backward(geo, gpt, x, W, flags, *, dout=None, demb=None, emb=None, out=None, dx=None, ws, wsb, slope=LEAKY_SLOPE,
                  stream=None):
    D = W.shape[0]
    _lib.check(_lib.load().hcg_mid_layer_bwd(
        _a(dout), _graph_rows(demb, geo, D), _graph_rows(emb, geo, D), _a(out), x.data_ptr(), W.data_ptr(), geo.edge_index, geo.E,
        geo.graph_ptr, geo.edge_ptr, geo.N, geo.B, x.shape[1], D, geo.max_nodes, geo.max_edges, slope, flags, _a(dx), geo.status,
        _a(ws), wsb, _lib.stream_ptr() if stream is None else stream), "hcg_mid_layer_bwd")


def _mid_workspace_bytes(geo, gpt, F, D) -> int:
    return _lib.load().hcg_mid_workspace_bytes(geo.B, F, D, geo.max_nodes, geo.max_edges)


def _mid_reduce_jobs(geo, gpt, F, D, ws, wsb, dW, db, job) -> int:
    lib, halves = _lib.load(), D // 64                 # one slab set (= one job) per 64-column half
    for half in range(halves):
        _lib.check(lib.hcg_mid_reduce_job(_a(ws), wsb, geo.B, F, D, geo.max_nodes, geo.max_edges, half, _a(dW), _a(db),
                                          job + half * _JOB_BYTES), "hcg_mid_reduce_job")
    return halves


def _tall_forward(geo, gpt, x, W, b, act, *, out=None, emb=None, poolbits=None, xagg=None, signs=None, ws=None, wsb=0,
                  slope=LEAKY_SLOPE, stream=None):
    _lib.check(_lib.load().hcg_tall_layer_fwd(
        x.data_ptr(), W.data_ptr(), b.data_ptr(), geo.edge_index, geo.E, geo.graph_ptr, geo.edge_ptr, geo.N, geo.B, x.shape[1], W.shape[0],
        geo.max_nodes, geo.max_edges, slope, act, _a(out), _graph_rows(emb, geo, W.shape[0]), _a(poolbits), _a(xagg), _a(signs),
        geo.status, _a(ws), wsb, _lib.stream_ptr() if stream is None else stream), "hcg_tall_layer_fwd")


def _tall_backward(geo, gpt, x, W, flags, *, dout=None, demb=None, emb=None, out=None, poolbits=None, xagg=None, signs=None,
                   nodes_dev=None, dx=None, ws, wsb, slope=LEAKY_SLOPE, stream=None):
    D = W.shape[0]
    _lib.check(_lib.load().hcg_tall_layer_bwd(
        _a(dout), _graph_rows(demb, geo, D), _graph_rows(emb, geo, D), _a(out), _a(poolbits), _a(xagg), _a(signs), nodes_dev,
        x.data_ptr(), W.data_ptr(), geo.edge_index, geo.E, geo.graph_ptr, geo.edge_ptr, geo.N, geo.B, x.shape[1], D, geo.max_nodes,
        geo.max_edges, slope, flags, _a(dx), geo.status, _a(ws), wsb, _lib.stream_ptr() if stream is None else stream),
        "hcg_tall_layer_bwd")


def _tall_workspace_bytes(geo, gpt, F, D) -> int:
    """H / dH round trip + gradient slabs: forward and backward share it."""
    return _lib.load().hcg_tall_workspace_bytes(geo.N, geo.B, F, D)


def _tall_reduce_jobs(geo, gpt, F, D, ws, wsb, dW, db, job, first: bool = False) -> int:
    """`first`: the slabs of the first-layer form (xagg + signs given to the backward)."""
    _lib.check(_lib.load().hcg_tall_reduce_jobs(_a(ws), wsb, geo.N, geo.B, F, D, int(first), _a(dW), _a(db), job),
               "hcg_tall_reduce_jobs")
    return 2                                           # dW, db


# small-graph tiles (csrc/fused.hip, graphs up to 32 nodes), one graph per workgroup / wave (csrc/mid.hip, wave.hip), the
# wide-layer route (csrc/tall.hip: dense row-streaming parts + per-graph segmented sums).  `row_streaming`: the family's
# kernels walk all N rows of the batch (N must be the exact row count) and its forward and backward share one workspace
TILES = SimpleNamespace(name="tiles", forward=_tiles_forward, backward=_tiles_backward, workspace_bytes=_tiles_workspace_bytes,
                        reduce_jobs=_tiles_reduce_jobs, backward_pair=_tiles_backward_pair, row_streaming=False)
MID = SimpleNamespace(name="mid", forward=_mid_forward, backward=_mid_backward, workspace_bytes=_mid_workspace_bytes,
                      reduce_jobs=_mid_reduce_jobs, row_streaming=False)
TALL = SimpleNamespace(name="tall", forward=_tall_forward, backward=_tall_backward, workspace_bytes=_tall_workspace_bytes,
                       reduce_jobs=_tall_reduce_jobs, row_streaming=True)

_JOB_BYTES = _lib.job_bytes()


class JobList:
    """A host array of HCG_REDUCE_MAX_JOBS hcg_reduce_job: a family's `reduce_jobs` writes at `slot()`, the count it returns
    goes to `n`; hcg_step_tail -- or `flush`, the reductions alone -- consumes them.  `spare`: one more descriptor behind
    the array, for a job on its way into another through hcg_reduce_job_append."""
    __slots__ = ("buf", "addr", "n", "spare")

    def __init__(self):
        self.buf = ctypes.create_string_buffer(_JOB_BYTES * (_lib.HCG_REDUCE_MAX_JOBS + 1))
        self.addr, self.n = ctypes.addressof(self.buf), 0
        self.spare = self.addr + _JOB_BYTES * _lib.HCG_REDUCE_MAX_JOBS

    def slot(self) -> int:
        return self.addr + self.n * _JOB_BYTES

    def add(self, n: int):
        """Count n more jobs; a full array is reduced right away (one launch)."""
        self.n += n
        if self.n == _lib.HCG_REDUCE_MAX_JOBS:
            self.flush()

    def flush(self):
        if self.n:
            _lib.reduce_jobs(self.addr, self.n)
            self.n = 0


# 64-wide layers: the dense-parts backward of csrc/tall.hip pays off once a batch fills the chip several times over; below
# ~70 k nodes the one-launch-per-layer kernels of csrc/mid.hip are faster (tools/sweep_tall_threshold.sh on the reference's
# graph sizes, end of round 3, ms/step mid vs wide-layer route: 34 k nodes 0.0727 / 0.0766, 45 k 0.0752 / 0.0791, 67 k 0.0968 /
# 0.0971, 89 k 0.1176 / 0.1131, 133 k 0.1587 / 0.1464; the reference's own batch of 40 graphs = 3.5 k nodes: 11 % in round 2)
# (with the first layer's dense backward behind BOTH routes the crossover moved again: 67 k 0.0920 / 0.0959, 89 k 0.1100 / 0.1107,
#  133 k 0.1465 / 0.1458, 177 k 0.1799 / 0.1689 -- profiles/r03_v_sweep_tall_threshold.txt)
TALL_MIN_NODES_D64 = 140000


def fused_graphs_per_tile(plan: Optional[BatchPlan], F: int, D: int, max_nodes: Optional[int] = None) -> int:
    """> 0 when the fused small-graph kernels apply to this plan / layer shape.  `max_nodes` replaces the plan's largest
    graph; with `plan=None` it is all there is (a batch's collate metadata: no plan checks)."""
    if plan is not None:
        if plan.mode != "blocked" or plan.ew_csr is not None or plan.max_nodes is None or plan.B == 0:
            return 0
        max_nodes = plan.max_nodes if max_nodes is None else max_nodes
    return int(_lib.load().hcg_fused_graphs_per_tile(F, D, max_nodes))


def _per_graph_plan(plan: BatchPlan) -> bool:
    return not (plan.mode != "blocked" or plan.ew_csr is not None or plan.max_nodes is None or plan.max_edges is None
                or plan.B == 0 or plan.N == 0)


def mid_supported(plan: Optional[BatchPlan], F: int, D: int, max_nodes: Optional[int] = None,
                  max_edges: Optional[int] = None) -> bool:
    """True when the one-graph-per-workgroup kernels apply to this plan / layer shape (`plan=None`, `max_nodes`: as
    `fused_graphs_per_tile`)."""
    if plan is not None:
        if not _per_graph_plan(plan):
            return False
        max_nodes, max_edges = plan.max_nodes if max_nodes is None else max_nodes, plan.max_edges
    return max_edges is not None and bool(_lib.load().hcg_mid_supported(F, D, max_nodes, max_edges))


def tall_supported(plan: BatchPlan, F: int, D: int, any_rows: bool = False) -> bool:
    """True when the kernels of csrc/tall.hip apply to this plan / layer shape (D = 128; D = 64 over graphs > 64 nodes in
    batches of at least TALL_MIN_NODES_D64 rows -- `any_rows`: of any row count)."""
    return _per_graph_plan(plan) and tall_shape_supported(plan.N, F, D, plan.max_nodes, plan.max_edges, any_rows)


def tall_shape_supported(N: int, F: int, D: int, max_nodes: int, max_edges: int, any_rows: bool = False) -> bool:
    """`tall_supported` from a batch's row count and collate metadata alone (no plan checks)."""
    if D == 64 and N < TALL_MIN_NODES_D64 and not any_rows:
        return False
    return bool(_lib.load().hcg_tall_supported(F, D, max_nodes, max_edges))


def conv_route(plan: Optional[BatchPlan], F: int, D: int, family: str = "auto", *, max_nodes=None, max_edges=None, rows=None):
    """Which fused family takes a conv layer F -> D: (TILES, graphs_per_tile), (TALL, 0), (MID, 0), or (None, 0) = none
    (the any-shape kernels).  Tiles first; then, where the one-graph-per-workgroup kernels apply, the wide-layer route
    unless `family == "mid"` (every layer it takes, mid.hip takes too), else mid.hip.  `max_nodes` replaces the plan's
    largest graph; `plan=None` asks from a batch's collate metadata alone (`max_nodes`, `max_edges`: no plan checks), and
    the wide-layer route, which needs the batch's row count, is considered only when `rows` gives it."""
    gpt = fused_graphs_per_tile(plan, F, D, max_nodes)
    if gpt > 0:
        return TILES, gpt
    if not mid_supported(plan, F, D, max_nodes, max_edges):
        return None, 0
    tall = family != "mid" and (tall_supported(plan, F, D) if plan is not None
                                else rows is not None and tall_shape_supported(rows, F, D, max_nodes, max_edges))
    return (TALL if tall else MID), 0


class _ConvLayerFn(torch.autograd.Function):
    """One launch per layer (and per direction) on a fused family (`conv_route`): returns the node embeddings, or -- with
    `pool=True`, the last conv layer -- the pooled graph embedding [max, mean] directly (the node embeddings stay internal,
    saved for the backward)."""

    @staticmethod
    def forward(ctx, x, weight, bias, plan: BatchPlan, fam, gpt: int, apply_act: bool, slope: float, pool: bool):
        _lib.require_gpu(x, weight, bias)
        x, weight, bias = _f32c(x), _f32c(weight), _f32c(bias)
        N, F = x.shape
        D = weight.shape[0]
        if weight.shape[1] != F or N != plan.N:
            raise ValueError(f"shape mismatch: x {tuple(x.shape)}, weight {tuple(weight.shape)}, plan N {plan.N}")
        dev, geo = x.device, geometry(plan)
        out = torch.empty(N, D, dtype=torch.float32, device=dev)
        emb = torch.empty(plan.B, 2 * D, dtype=torch.float32, device=dev) if pool else None
        extra = {}
        if fam is TALL:
            wsb = TALL.workspace_bytes(geo, gpt, F, D) if D != 64 else 0     # (64-wide: the forward needs none)
            extra = dict(ws=torch.empty(wsb, dtype=torch.uint8, device=dev) if wsb else None, wsb=wsb)
        fam.forward(geo, gpt, x, weight, bias, int(apply_act), out=out, emb=emb, slope=slope, **extra)
        ctx.plan, ctx.fam, ctx.gpt, ctx.apply_act, ctx.slope, ctx.pool = plan, fam, gpt, apply_act, slope, pool
        ctx.save_for_backward(x, weight, out, *([emb] if pool else []))
        return emb if pool else out

    @staticmethod
    def backward(ctx, grad):
        x, weight, out, *emb = ctx.saved_tensors
        fam, gpt, geo = ctx.fam, ctx.gpt, geometry(ctx.plan)
        N, F = x.shape
        D = weight.shape[0]
        dev = x.device
        dx = torch.empty_like(x) if ctx.needs_input_grad[0] else None
        dW = torch.empty_like(weight)
        db = torch.empty(D, dtype=torch.float32, device=dev)
        wsb = fam.workspace_bytes(geo, gpt, F, D)
        ws = torch.empty(wsb, dtype=torch.uint8, device=dev)
        up = dict(demb=_f32c(grad), emb=emb[0]) if ctx.pool else dict(dout=_f32c(grad))
        fam.backward(geo, gpt, x, weight, int(ctx.apply_act), out=out, dx=dx, ws=ws, wsb=wsb, slope=ctx.slope, **up)
        jobs = JobList()
        jobs.n = fam.reduce_jobs(geo, gpt, F, D, ws, wsb, dW, db, jobs.slot())
        jobs.flush()
        return dx, dW, db, None, None, None, None, None, None


def conv_layer(x, weight, bias, plan: BatchPlan, fam, gpt: int = 0, apply_act=True, slope=LEAKY_SLOPE, pool=False):
    """A conv layer on the family `conv_route` picked (fam, gpt)."""
    return _ConvLayerFn.apply(x, weight, bias, plan, fam, gpt, apply_act, slope, pool)


class _Readout2Fn(torch.autograd.Function):
    """out = (LeakyReLU(emb W0^T + b0)) W1^T + b1 in one launch (csrc/readout.hip)."""

    @staticmethod
    def forward(ctx, emb, W0, b0, W1, b1, slope: float):
        lib = _lib.load()
        _lib.require_gpu(emb, W0, b0, W1, b1)
        emb, W0, b0, W1, b1 = _f32c(emb), _f32c(W0), _f32c(b0), _f32c(W1), _f32c(b1)
        B, D, C = emb.shape[0], W0.shape[0], W1.shape[0]
        if emb.shape[1] != 2 * D or W0.shape[1] != 2 * D or W1.shape[1] != D:
            raise ValueError("readout shape mismatch")
        z = torch.empty(B, D, dtype=torch.float32, device=emb.device)
        out = torch.empty(B, C, dtype=torch.float32, device=emb.device)
        rc = lib.hcg_readout2_fwd(_lib.ptr(emb), _lib.ptr(W0), _lib.ptr(b0), _lib.ptr(W1), _lib.ptr(b1), B, D, C, slope,
                                  _lib.ptr(z), _lib.ptr(out), _lib.stream_ptr())
        _lib.check(rc, "hcg_readout2_fwd")
        ctx.save_for_backward(emb, z, W0, W1)
        ctx.slope = slope
        return out

    @staticmethod
    def backward(ctx, dout):
        lib = _lib.load()
        emb, z, W0, W1 = ctx.saved_tensors
        dout = _f32c(dout)
        B, D, C = emb.shape[0], W0.shape[0], W1.shape[0]
        dev = emb.device
        demb = torch.empty_like(emb)
        dW0, dW1 = torch.empty_like(W0), torch.empty_like(W1)
        db0 = torch.empty(D, dtype=torch.float32, device=dev)
        db1 = torch.empty(C, dtype=torch.float32, device=dev)
        wsb = lib.hcg_general_workspace_bytes(_lib.HCG_WS_READOUT2, B, 0, 0, 0)
        ws = torch.empty(wsb, dtype=torch.uint8, device=dev)
        job = _lib.ReduceJob()
        rc = lib.hcg_readout2_bwd_partial(_lib.ptr(dout), _lib.ptr(emb), _lib.ptr(z), _lib.ptr(W0), _lib.ptr(W1), B, D, C, ctx.slope,
                                          _lib.ptr(demb), _lib.ptr(ws), wsb, _lib.ptr(dW0), _lib.ptr(db0), _lib.ptr(dW1),
                                          _lib.ptr(db1), ctypes.addressof(job), _lib.stream_ptr())
        _lib.check(rc, "hcg_readout2_bwd_partial")
        _lib.reduce_jobs(ctypes.addressof(job), 1)
        return demb, dW0, db0, dW1, db1, None


class _MSEFn(torch.autograd.Function):
    """mean((input - target)^2) in one launch each way (csrc/loss.hip)."""

    @staticmethod
    def forward(ctx, inp, target):
        lib = _lib.load()
        _lib.require_gpu(inp, target)
        if inp.shape != target.shape:
            raise ValueError(f"MSELoss: input {tuple(inp.shape)} and target {tuple(target.shape)} must have the same shape")
        a, b = _f32c(inp), _f32c(target)
        loss = torch.empty((), dtype=torch.float32, device=a.device)
        _lib.check(lib.hcg_mse_fwd(_lib.ptr(a), _lib.ptr(b), a.numel(), _lib.ptr(loss), _lib.stream_ptr()), "hcg_mse_fwd")
        ctx.save_for_backward(a, b)
        return loss

    @staticmethod
    def backward(ctx, g):
        lib = _lib.load()
        a, b = ctx.saved_tensors
        g = _f32c(g)
        da = torch.empty_like(a) if ctx.needs_input_grad[0] else None
        db = torch.empty_like(b) if ctx.needs_input_grad[1] else None
        if da is None and db is None:
            return None, None
        _lib.check(lib.hcg_mse_bwd(_lib.ptr(a), _lib.ptr(b), _lib.ptr(g), a.numel(), _lib.ptr(da), _lib.ptr(db),
                                   _lib.stream_ptr()), "hcg_mse_bwd")
        return da, db


def mse_loss(inp, target):
    return _MSEFn.apply(inp, target)


class _CrossEntropyFn(torch.autograd.Function):
    """`nn.CrossEntropyLoss()(logits, target.long())` -- mean over the graphs of logsumexp(logits) - logits[target], default
    settings, no sqrt -- in one launch (csrc/loss.hip: k_ce_fwd_bwd leaves the loss AND d loss / d logits); the backward is
    that gradient times the incoming one."""

    @staticmethod
    def forward(ctx, logits, target):
        _lib.require_gpu(logits, target)
        if logits.dim() != 2 or target.shape != logits.shape[:1]:
            raise ValueError(f"CrossEntropyLoss: logits {tuple(logits.shape)} need class-index targets of shape "
                             f"({logits.shape[0]},), got {tuple(target.shape)}")
        a = _f32c(logits)
        y = target.to(torch.float32).contiguous()           # (class indices: exact in float32)
        loss = torch.empty(2, dtype=torch.float32, device=a.device)
        dout = torch.empty_like(a) if ctx.needs_input_grad[0] else None
        _lib.ce_fwd_bwd(a, y, loss, dout)
        ctx.save_for_backward(dout)
        return loss[0]

    @staticmethod
    def backward(ctx, g):
        (dout,) = ctx.saved_tensors
        return (None if dout is None else dout * g), None


def cross_entropy(logits, target):
    """Cross-entropy of float32 GPU logits [B, C] against class indices [B] (int64, or floats holding integers)."""
    return _CrossEntropyFn.apply(logits, target)


def readout2_supported(D: int, C: int) -> bool:
    return D == 64 and bool(_lib.load().hcg_head_supported(D, C))


def readout2(emb, W0, b0, W1, b1, slope=LEAKY_SLOPE):
    return _Readout2Fn.apply(emb, W0, b0, W1, b1, slope)


class _FusedModelFn(torch.autograd.Function):
    """The whole small-graph model -- every fused conv layer (the last one with its pooling
    epilogue) and the fused readout head -- as ONE autograd node.  Same kernels as the per-layer
    Functions; what it removes is host time: one `apply`, one backward callback and one set of
    allocations instead of four (the eager step is host-bound: ~0.1 ms of autograd/ctypes per node)."""

    @staticmethod
    def forward(ctx, plan: BatchPlan, gpts, slope: float, x, *params):
        lib = _lib.load()
        _lib.require_gpu(x, *params)
        x = _f32c(x)
        params = [_f32c(p) for p in params]
        n_conv = len(gpts)
        convs, (R0w, R0b, R1w, R1b) = params[:2 * n_conv], params[2 * n_conv:]
        N, dev, stream = x.shape[0], x.device, _lib.stream_ptr()
        if N != plan.N:
            raise ValueError(f"x has {N} rows, plan was built for {plan.N}")
        D = convs[0].shape[0]
        acts, geo = [], geometry(plan)
        emb = torch.empty(plan.B, 2 * D, dtype=torch.float32, device=dev)
        if n_conv == 2 and gpts[0] == gpts[1]:
            # the reference's default depth: both conv layers in ONE launch (csrc/fused.hip, STACK2)
            acts = [torch.empty(N, D, dtype=torch.float32, device=dev) for _ in range(2)]
            TILES.forward(geo, gpts[0], x, convs[0], convs[1], 1, out=acts[0], emb=emb, slope=slope, W2=convs[2], b2=convs[3],
                          out2=acts[1])
        else:
            for l in range(n_conv):
                h = torch.empty(N, D, dtype=torch.float32, device=dev)
                TILES.forward(geo, gpts[l], acts[-1] if l else x, convs[2 * l], convs[2 * l + 1], 1, out=h,
                              emb=emb if l == n_conv - 1 else None, slope=slope)
                acts.append(h)
        C = R1w.shape[0]
        z = torch.empty(plan.B, D, dtype=torch.float32, device=dev)
        y = torch.empty(plan.B, C, dtype=torch.float32, device=dev)
        rc = lib.hcg_readout2_fwd(_lib.ptr(emb), _lib.ptr(R0w), _lib.ptr(R0b), _lib.ptr(R1w), _lib.ptr(R1b), plan.B, D, C,
                                  slope, _lib.ptr(z), _lib.ptr(y), stream)
        _lib.check(rc, "hcg_readout2_fwd")
        ctx.save_for_backward(x, emb, z, *acts, *params)
        ctx.plan, ctx.gpts, ctx.slope, ctx.n_conv = plan, list(gpts), slope, n_conv
        ctx.set_materialize_grads(False)   # an unused graph_emb must arrive as None, not as a zero tensor + an add
        return y, emb

    @staticmethod
    def backward(ctx, dy, demb_ext):
        lib = _lib.load()
        plan, gpts, slope, n_conv = ctx.plan, ctx.gpts, ctx.slope, ctx.n_conv
        saved = ctx.saved_tensors
        x, emb, z = saved[0], saved[1], saved[2]
        acts, params = saved[3:3 + n_conv], saved[3 + n_conv:]
        convs, (R0w, R0b, R1w, R1b) = params[:2 * n_conv], params[2 * n_conv:]
        dev, stream = x.device, _lib.stream_ptr()
        D, C, B = convs[0].shape[0], R1w.shape[0], plan.B
        f32 = dict(dtype=torch.float32, device=dev)
        # every backward kernel leaves per-workgroup slabs; ONE batched launch reduces them all at the end (a model deeper
        # than seven conv layers: one launch per HCG_REDUCE_MAX_JOBS of them)
        jobs, keep = JobList(), []                  # workspaces must outlive the reductions' enqueue
        # All weight gradients are views of ONE flat buffer laid out in nn.Module parameter order
        # (conv: bias, lin.weight; readout: weight, bias) -- the data-parallel wrapper can then all-reduce it
        # in place, without first concatenating 8 small tensors.
        sizes = []
        for l in range(n_conv):
            sizes += [D, convs[2 * l].numel()]
        sizes += [R0w.numel(), D, R1w.numel(), C]
        flat = torch.empty(sum(sizes), **f32)
        views, off = [], 0
        for n_el in sizes:
            views.append(flat[off:off + n_el])
            off += n_el
        conv_db = [views[2 * l] for l in range(n_conv)]
        conv_dW = [views[2 * l + 1].view_as(convs[2 * l]) for l in range(n_conv)]
        dR0w, dR0b = views[2 * n_conv].view_as(R0w), views[2 * n_conv + 1]
        dR1w, dR1b = views[2 * n_conv + 2].view_as(R1w), views[2 * n_conv + 3]
        # readout head
        dy = _f32c(dy) if dy is not None else torch.zeros(B, C, **f32)
        demb = torch.empty_like(emb)
        wsb = lib.hcg_general_workspace_bytes(_lib.HCG_WS_READOUT2, B, 0, 0, 0)
        ws = torch.empty(wsb, dtype=torch.uint8, device=dev)
        keep.append(ws)
        rc = lib.hcg_readout2_bwd_partial(_lib.ptr(dy), _lib.ptr(emb), _lib.ptr(z), _lib.ptr(R0w), _lib.ptr(R1w), B, D, C,
                                          slope, _lib.ptr(demb), _lib.ptr(ws), wsb, _lib.ptr(dR0w), _lib.ptr(dR0b), _lib.ptr(dR1w),
                                          _lib.ptr(dR1b), jobs.slot(), stream)
        _lib.check(rc, "hcg_readout2_bwd_partial")
        jobs.add(1)
        if demb_ext is not None:          # the caller also used graph_emb downstream
            demb = demb + _f32c(demb_ext)
        # conv stack, last layer first
        geo = geometry(plan)
        grads = [None] * (2 * n_conv)
        dh = None
        for l in reversed(range(n_conv)):
            W = convs[2 * l]
            inp = x if l == 0 else acts[l - 1]
            F = inp.shape[1]
            dx = torch.empty_like(inp) if (l > 0 or ctx.needs_input_grad[3]) else None
            dW, db = conv_dW[l], conv_db[l]
            wsb = TILES.workspace_bytes(geo, gpts[l], F, D)
            ws = torch.empty(wsb, dtype=torch.uint8, device=dev)
            keep.append(ws)
            up = dict(demb=demb, emb=emb) if l == n_conv - 1 else dict(dout=dh)
            TILES.backward(geo, gpts[l], inp, W, 1, out=acts[l], dx=dx, ws=ws, wsb=wsb, slope=slope, stream=stream, **up)
            jobs.add(TILES.reduce_jobs(geo, gpts[l], F, D, ws, wsb, dW, db, jobs.slot()))
            grads[2 * l], grads[2 * l + 1] = dW, db
            dh = dx
        jobs.flush()
        return (None, None, None, dh if ctx.needs_input_grad[3] else None, *grads, dR0w, dR0b, dR1w, dR1b)


def fused_model(plan: BatchPlan, gpts, x, conv_params, readout_params, slope=LEAKY_SLOPE):
    """-> (out [B, C], graph_emb [B, 2D]).  conv_params = [W1, b1, W2, b2, ...], readout_params = [W0, b0, W1, b1]."""
    return _FusedModelFn.apply(plan, tuple(gpts), slope, x, *conv_params, *readout_params)


def gcn_layer(x, weight, bias, plan: BatchPlan, use_edge_weight=False, apply_act=True, slope=LEAKY_SLOPE, edge_mult=None):
    return _GCNLayerFn.apply(x, weight, bias, plan, use_edge_weight, apply_act, slope, edge_mult)


def graph_pool(a, plan: BatchPlan):
    return _PoolFn.apply(a, plan)


def linear(x, weight, bias=None, apply_act=False, slope=LEAKY_SLOPE):
    return _LinearFn.apply(x, weight, bias, apply_act, slope)
