"""Explain-mode hooks of the conv stack.

The reference explains its model with `torch_geometric.explain.Explainer(GNNExplainer(), node_mask_type='attributes',
edge_mask_type='object')` on `GCN_explain` (scripts_experiments/explain_gnn.py:39-50, utils/other_utils.py:58-60).
PyG implements the edge mask by setting three attributes on every `MessagePassing` layer (`explain`, `_edge_mask`,
`_apply_sigmoid`: torch_geometric.explain.algorithm.utils.set_masks / clear_masks) and multiplying each message by
the mask inside `propagate` -- AFTER gcn_norm, in every conv layer, self loops keep mask 1.  The node mask is a plain
elementwise product on `x` done by the caller.

This module provides the same two functions for `hcatgnet_amd.GCNConv`; the forward then runs the any-shape HIP
kernels with the mask as per-edge multiplier and autograd delivers d out / d mask (csrc/layer.hip:
k_edge_weight_grad) and d out / d x.  `ExplainStep` delivers the same outputs and mask gradients for a whole batch of
graphs in ONE launch (csrc/explain.hip: one workgroup per graph, mask gradients only, weights frozen).  The
optimisation loop of GNNExplainer itself (and the plotting around it) is outside this package: any torch optimiser
over (node_mask, edge_mask) works on these gradients.
"""
from __future__ import annotations

import ctypes
from typing import NamedTuple, Optional

import torch

from . import _frozen, _lib
from .gcn import GCNConv


def set_masks(model: torch.nn.Module, mask: torch.Tensor, edge_index: torch.Tensor = None, apply_sigmoid: bool = True):
    """Attach `mask` ([E], the batch's edge order) to every conv layer of `model` (PyG signature; `edge_index` is
    accepted for compatibility and only used to check the length)."""
    if edge_index is not None and mask.numel() != edge_index.shape[1]:
        raise ValueError(f"edge mask has {mask.numel()} entries for {edge_index.shape[1]} edges")
    for module in model.modules():
        if isinstance(module, GCNConv):
            module.explain = True
            module._edge_mask = mask
            module._apply_sigmoid = apply_sigmoid


def clear_masks(model: torch.nn.Module):
    for module in model.modules():
        if isinstance(module, GCNConv):
            module.explain = False
            module._edge_mask = None
            module._apply_sigmoid = True


class ExplainResult(NamedTuple):
    out: torch.Tensor                       # [B, C]
    loss: Optional[torch.Tensor]            # [B] per-graph mean_c (out - target)^2; None without target
    d_edge_mask: Optional[torch.Tensor]     # [E], the batch's edge order; None for a forward-only call
    d_node_mask: Optional[torch.Tensor]     # [N, F]; None without a node mask (or forward only)
    dx: Optional[torch.Tensor]              # [N, F] = dJ/dx; None unless asked for


class ExplainStep:
    """Outputs and mask gradients of a frozen model for a whole batch of graphs, one launch per call.

        step = ExplainStep(model, apply_sigmoid=True)
        r = step(batch, edge_mask, node_mask=None, target=None, dout=None, want_dx=False)

    The values equal autograd through the model run on `x * s(node_mask)` with the edge mask `s(edge_mask)` multiplied
    into every message of every conv layer (s = sigmoid with `apply_sigmoid`, else the identity; self loops keep 1), of
    J = sum_g l_g with l_g = mean_c (out_gc - target_gc)^2 (`target` [B, C]) or of J = sum(dout * out) (`dout` [B, C]);
    with neither, the call is forward only.  At most one of `target` / `dout`.

    The graphs of a batch are independent, so J's gradient restricted to graph g's mask entries is exactly what a
    batch-of-one explainer run on g computes: one call serves one iteration of an explainer for EVERY graph of a dataset.
    The regularisers of an explainer (mask size, mask entropy) are functions of the masks alone; the caller adds their
    gradients with torch ops and keeps the optimiser loop.

    The weights are read, never written; no parameter's `.grad` is touched and no mask stays attached to the model.
    `batch` needs the collate metadata `FusedTrainStep` needs (`max_nodes`, `max_edges`, grouped edges).  Buffers are
    allocated for the largest batch seen and reused: in steady state a call allocates nothing and can be captured with
    `torch.cuda.graph` -- and the returned tensors are views of those buffers, overwritten by the next call (clone what
    must outlive it).  When `reason(batch)` is not None the step runs the existing path itself (`set_masks`, forward,
    `torch.autograd.grad` with respect to the masks and x only, `clear_masks`) and returns the same fields;
    `last_path` says which one ran ("fused" / "autograd")."""

    def __init__(self, model: torch.nn.Module, apply_sigmoid: bool = True):
        self.model, self.apply_sigmoid = model, bool(apply_sigmoid)
        self.last_path: Optional[str] = None
        self._cap = None            # (N, E, B) capacity of the buffers
        self._bufs = None
        self._args = _lib.ExplainArgs()

    # ------------------------------------------------------------------ support check (host only, no sync)
    def _shape_args(self, a, batch) -> Optional[str]:
        m = self.model
        why = _frozen.model_reason(m)
        if why is None and batch is not None:
            why = _frozen.batch_reason(batch, int(m.n_node_features), "model")
        return why or _frozen.query(a, _lib.HCG_EXPLAIN_GRAPHS, _frozen.model_shape(m), batch)

    def reason(self, batch=None) -> Optional[str]:
        """None when this model (and `batch`) takes the one-launch kernel, else why not.  Host metadata only."""
        return self._shape_args(_lib.ExplainArgs(), batch)

    # ------------------------------------------------------------------ buffers
    def _buffers(self, N, E, B, F, C, ws_bytes, dev):
        cap = self._cap
        if cap is None or N > cap[0] or E > cap[1] or B > cap[2] or ws_bytes > cap[3] or self._bufs["out"].device != dev:
            cap = (max(N, cap[0] if cap else 0), max(E, cap[1] if cap else 0), max(B, cap[2] if cap else 0),
                   max(ws_bytes, cap[3] if cap else 0))
            f32 = dict(dtype=torch.float32, device=dev)
            self._bufs = dict(out=torch.zeros(cap[2], C, **f32), loss=torch.zeros(cap[2], **f32),
                              d_edge=torch.zeros(max(cap[1], 1), **f32), d_node=torch.zeros(max(cap[0], 1), F, **f32),
                              dx=torch.zeros(max(cap[0], 1), F, **f32),
                              ws=torch.empty(max(cap[3], 256), dtype=torch.uint8, device=dev))
            self._cap = cap
        return self._bufs

    @staticmethod
    def _mask(t, shape, what):
        if t.dtype != torch.float32 or not t.is_contiguous() or tuple(t.shape) != tuple(shape):
            raise ValueError(f"{what} must be a contiguous float32 tensor of shape {tuple(shape)}; got {t.dtype} {tuple(t.shape)}")
        return t.detach()

    # ------------------------------------------------------------------ the call
    def __call__(self, batch, edge_mask, node_mask=None, target=None, dout=None, want_dx: bool = False) -> ExplainResult:
        if target is not None and dout is not None:
            raise ValueError("at most one of target / dout")
        a = self._args
        why = self._shape_args(a, batch)
        if why is not None:
            return self._autograd(batch, edge_mask, node_mask, target, dout, want_dx)
        m = self.model
        x = _frozen.batch_x(batch, edge_mask, node_mask, target, dout)
        N, F, E, B, C = a.N, a.F, a.E, a.B, a.C
        em = self._mask(edge_mask, (E,), "edge_mask")
        nm = self._mask(node_mask, (N, F), "node_mask") if node_mask is not None else None
        tg = self._mask(target, (B, C), "target") if target is not None else None
        do = self._mask(dout, (B, C), "dout") if dout is not None else None
        plan = m._plan_for(batch, x, batch.edge_index, batch.batch, None)
        bwd = tg is not None or do is not None
        bufs = self._buffers(N, E, B, F, C, int(a.workspace_bytes_needed), x.device)
        p = _lib.ptr
        a.flags = _lib.HCG_EXPLAIN_SIGMOID if self.apply_sigmoid else 0
        _frozen.fill_graph(a, x, plan)
        _frozen.fill_weights(a, *_frozen.model_weights(m, x.device, "ExplainStep"))
        a.edge_mask, a.node_mask, a.target, a.dout = p(em), p(nm), p(tg), p(do)
        a.out, a.loss, a.d_edge_mask = p(bufs["out"]), p(bufs["loss"]), p(bufs["d_edge"])
        a.d_node_mask = p(bufs["d_node"]) if nm is not None else None
        a.dx = p(bufs["dx"]) if want_dx else None
        a.workspace, a.workspace_bytes = p(bufs["ws"]), bufs["ws"].numel()
        a.slope = _frozen.SLOPE
        _lib.check(_lib.load().hcg_explain(ctypes.addressof(a), _lib.stream_ptr()), "hcg_explain")
        self.last_path = "fused"
        return ExplainResult(bufs["out"][:B], bufs["loss"][:B] if tg is not None else None,
                             bufs["d_edge"][:E] if bwd else None,
                             bufs["d_node"][:N] if bwd and nm is not None else None,
                             bufs["dx"][:N] if bwd and want_dx else None)

    # ------------------------------------------------------------------ the existing path (any shape), under autograd
    def _autograd(self, batch, edge_mask, node_mask, target, dout, want_dx) -> ExplainResult:
        m = self.model
        bwd = target is not None or dout is not None
        s = torch.sigmoid if self.apply_sigmoid else (lambda t: t)
        em = edge_mask.detach().requires_grad_(bwd)
        nm = node_mask.detach().requires_grad_(bwd) if node_mask is not None else None
        x = batch.x.detach().requires_grad_(bwd and want_dx)
        xin = x * s(nm) if nm is not None else x
        set_masks(m, em, batch.edge_index, apply_sigmoid=self.apply_sigmoid)
        try:
            with torch.enable_grad() if bwd else torch.no_grad():
                out = m(x=xin, edge_index=batch.edge_index, batch=batch.batch)
                loss = d_e = d_n = dx = None
                if bwd:
                    if target is not None:
                        loss = ((out - target.detach()) ** 2).mean(dim=1)
                        J = loss.sum()
                    else:
                        J = (dout.detach() * out).sum()
                    wrt = [em] + ([nm] if nm is not None else []) + ([x] if want_dx else [])
                    grads = list(torch.autograd.grad(J, wrt))         # (no parameter's .grad is touched)
                    d_e = grads.pop(0)
                    d_n = grads.pop(0) if nm is not None else None
                    dx = grads.pop(0) if want_dx else None
        finally:
            clear_masks(m)
        self.last_path = "autograd"
        return ExplainResult(out.detach(), loss.detach() if loss is not None else None, d_e, d_n, dx)
