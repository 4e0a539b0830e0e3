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
graphs in ONE launch (csrc/explain.hip: one workgroup per graph, mask gradients only, weights frozen); any torch
optimiser over (node_mask, edge_mask) works on these gradients.  `ExplainFit` is GNNExplainer itself: the whole mask
optimisation of every graph of a batch -- forward, backward, regularisers, Adam, hard masks, all epochs -- in ONE launch
of the same kernel with an epoch loop inside.  Both take a regression model (mean squared error against a target row) and a
classification model (cross-entropy against a class index per graph).  The plotting around an explanation is outside this package.
"""
from __future__ import annotations

import ctypes
import math
from dataclasses import dataclass, fields
from typing import NamedTuple, Optional

import torch
import torch.nn.functional as F_

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
    loss: Optional[torch.Tensor]            # [B] per graph: mean_c (out - target)^2 with `target`, -log_softmax(out)[y] with
                                            # `target_class`; None with `dout` and forward only
    d_edge_mask: Optional[torch.Tensor]     # [E], the batch's edge order; None for a forward-only call
    d_node_mask: Optional[torch.Tensor]     # [N, F]; None without a node mask (or forward only)
    dx: Optional[torch.Tensor]              # [N, F] = dJ/dx; None unless asked for


class ExplainStep(_frozen.FrozenModel):
    """Outputs and mask gradients of a frozen model for a whole batch of graphs, one launch per call.

        step = ExplainStep(model, apply_sigmoid=True)
        r = step(batch, edge_mask, node_mask=None, target=None, dout=None, want_dx=False, target_class=None)

    The values equal autograd through the model run on `x * s(node_mask)` with the edge mask `s(edge_mask)` multiplied
    into every message of every conv layer (s = sigmoid with `apply_sigmoid`, else the identity; self loops keep 1), of
    J = sum_g l_g with l_g = mean_c (out_gc - target_gc)^2 (`target` [B, C]), of J = sum(dout * out) (`dout` [B, C]), or of
    J = sum_g l_g with the cross-entropy l_g = -log_softmax(out_g)[y_g] (`target_class`: y [B] int64 class indices, a model
    of two classes or more; `F.cross_entropy` of one row); with none of them, the call is forward only.  At most one of
    `target` / `dout` / `target_class`.  `loss` holds l_g of the form that has one.  The kernel never uses a class index as
    an address and does not check its range (that would cost a sync): an index outside 0 .. C - 1 gives that graph a NaN
    loss and the gradient of softmax(out_g) alone; the autograd path leaves the index to `F.cross_entropy`.

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

    KERNEL, NAME, REFUSES_CPU = _lib.HCG_EXPLAIN_GRAPHS, "ExplainStep", False

    def __init__(self, model: torch.nn.Module, apply_sigmoid: bool = True):
        super().__init__(model)
        self.apply_sigmoid = bool(apply_sigmoid)

    @staticmethod
    def _mask(t, shape, what):
        if t.dtype != torch.float32 or not t.is_contiguous() or tuple(t.shape) != tuple(shape):
            raise ValueError(f"{what} must be a contiguous float32 tensor of shape {tuple(shape)}; got {t.dtype} {tuple(t.shape)}")
        return t.detach()

    # ------------------------------------------------------------------ the call
    def __call__(self, batch, edge_mask, node_mask=None, target=None, dout=None, want_dx: bool = False,
                 target_class=None) -> ExplainResult:
        if sum(t is not None for t in (target, dout, target_class)) > 1:
            raise ValueError("at most one of target / dout / target_class")
        if target_class is not None:
            B = int(batch.num_graphs)
            if (not torch.is_tensor(target_class) or target_class.dtype != torch.int64 or tuple(target_class.shape) != (B,)
                    or not target_class.is_contiguous()):
                raise ValueError(f"target_class must be a contiguous int64 tensor of shape {(B,)} (one class index per graph); got "
                                 f"{getattr(target_class, 'dtype', type(target_class))} {tuple(getattr(target_class, 'shape', ()))}")
            if target_class.device != batch.x.device:
                raise ValueError(f"target_class is on {target_class.device}, the batch on {batch.x.device}")
            if int(getattr(self.model, "_n_classes", 2)) < 2:
                raise ValueError(f"target_class needs a model of two classes or more; this one has {int(self.model._n_classes)}")
        a = self._args
        why = self._shape_args(a, batch)
        if why is not None:
            return self._autograd(batch, edge_mask, node_mask, target, dout, want_dx, target_class)
        x = _frozen.batch_x(batch, edge_mask, node_mask, target, dout, target_class)
        N, F, E, B, C = a.N, a.F, a.E, a.B, a.C
        em = self._mask(edge_mask, (E,), "edge_mask")
        nm = self._mask(node_mask, (N, F), "node_mask") if node_mask is not None else None
        tg = self._mask(target, (B, C), "target") if target is not None else None
        do = self._mask(dout, (B, C), "dout") if dout is not None else None
        tc = target_class.detach() if target_class is not None else None
        bwd = tg is not None or do is not None or tc is not None
        take, dev = self._bufs.take, x.device
        out, loss, d_edge = take("out", (B, C), dev), take("loss", (B,), dev), take("d_edge", (E,), dev)
        d_node = take("d_node", (N, F), dev) if nm is not None else None
        dx = take("dx", (N, F), dev) if want_dx else None
        p = _lib.ptr
        self._fill(a, (_lib.HCG_EXPLAIN_SIGMOID if self.apply_sigmoid else 0) | (_lib.HCG_EXPLAIN_TARGET_CLASS if tc is not None else 0),
                   batch, x, self._weights(dev), self._bufs.workspace(int(a.workspace_bytes_needed), dev))
        a.edge_mask, a.node_mask, a.dout = p(em), p(nm), p(do)
        a.target = p(tc) if tc is not None else p(tg)        # (one slot of the argument block, read by the flag)
        a.out, a.loss, a.d_edge_mask, a.d_node_mask, a.dx = (_frozen.front(t) for t in (out, loss, d_edge, d_node, dx))
        _lib.check(_lib.load().hcg_explain(ctypes.addressof(a), _lib.stream_ptr()), "hcg_explain")
        self.last_path = "fused"
        return ExplainResult(out, loss if tg is not None or tc is not None else None, d_edge if bwd else None,
                             d_node if bwd else None, dx if bwd else None)

    # ------------------------------------------------------------------ the existing path (any shape), under autograd
    def _autograd(self, batch, edge_mask, node_mask, target, dout, want_dx, target_class=None) -> ExplainResult:
        m = self.model
        bwd = target is not None or dout is not None or target_class is not None
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
                    elif target_class is not None:
                        loss = F_.cross_entropy(out, target_class.detach(), reduction="none")
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


# ====================================================================================================== GNNExplainer
EPS = 1e-15
# torch_geometric.explain.GNNExplainer.coeffs: edge_size weighs a SUM, node_feat_size a MEAN
DEFAULT_COEFFS = dict(edge_size=0.005, edge_ent=1.0, node_feat_size=1.0, node_feat_ent=0.1)
BETA1, BETA2, ADAM_EPS = 0.9, 0.999, 1e-8          # torch.optim.Adam's defaults


@dataclass
class ExplainFitState:
    """What a GNNExplainer fit carries from epoch to epoch: the mask LOGITS, Adam's two moments for each, the hard flags
    (set by the epoch at step 0: the entry's first gradient was not 0) with their per-graph counts, and the number of Adam
    steps taken.  `ExplainFit` updates the tensors IN PLACE; `clone()` keeps a copy."""
    edge_logit: torch.Tensor          # [E] f32
    edge_exp_avg: torch.Tensor        # [E] f32
    edge_exp_avg_sq: torch.Tensor     # [E] f32
    edge_hard: torch.Tensor           # [E] bool
    node_logit: torch.Tensor          # [N, F] f32
    node_exp_avg: torch.Tensor        # [N, F] f32
    node_exp_avg_sq: torch.Tensor     # [N, F] f32
    node_hard: torch.Tensor           # [N, F] bool
    hard_count: torch.Tensor          # [B, 2] int32: hard edges, hard node entries of every graph
    step: int = 0

    def tensors(self):
        return [(f.name, getattr(self, f.name)) for f in fields(self) if f.name != "step"]

    def clone(self) -> "ExplainFitState":
        return ExplainFitState(**{k: t.clone() for k, t in self.tensors()}, step=int(self.step))

    def to(self, device) -> "ExplainFitState":
        return ExplainFitState(**{k: t.to(device) for k, t in self.tensors()}, step=int(self.step))


class ExplainFitResult(NamedTuple):
    edge_mask: torch.Tensor           # [E] sigmoid(edge logit), 0 where the entry is not hard
    node_mask: torch.Tensor           # [N, F]
    out: torch.Tensor                 # [B, C] the model's outputs under the masks the LAST epoch started from
    loss_history: torch.Tensor        # [T, B] the prediction loss of every graph in every epoch of this call
    state: ExplainFitState            # the state after the call (the tensors passed in, updated in place)


def _entropy_grad(m):
    """d/dm of -m log(m + EPS) - (1 - m) log(1 - m + EPS), as written"""
    a, b = m + EPS, (1 - m) + EPS
    return (torch.log(b) + (1 - m) / b) - (torch.log(a) + m / a)


class ExplainFit(_frozen.FrozenModel):
    """GNNExplainer for a whole batch of graphs: every graph's mask optimisation, all epochs, in ONE launch.

        fit = ExplainFit(model, epochs=100, lr=0.01, coeffs=None, mode="regression")
        r = fit(batch, target=None, state=None, epochs=None, generator=None, epochs_per_launch=None)
        # ExplainFitResult(edge_mask [E], node_mask [N, F], out [B, C], loss_history [T, B], state)

    The algorithm is the published torch_geometric 2.3 / 2.4 `GNNExplainer` with `explanation_type='model'`,
    `node_mask_type='attributes'`, `edge_mask_type='object'`, in regression mode or (`mode="multiclass_classification"`,
    `return_type='raw'`) for a model of two classes or more, run as a batch-of-one fit per graph (the graphs of a batch
    never interact).  Per graph g: logits e [E_g] and n [N_g, F]; every epoch runs `ExplainStep(apply_sigmoid=True)`'s
    model on them against `target`.  Regression: `target` is float32 [B, C] (default: the model's own unmasked prediction)
    and l_g = mean_c (out_gc - target_gc)^2.  Classification: `target` is int64 [B], a class index per graph (default: the
    argmax of the model's own unmasked output, the first maximal index on a tie -- the 'model' explanation; the true labels
    give the 'phenomenon' one) and l_g = -log_softmax(out_g)[target_g], `F.cross_entropy` of one row.  On CPU tensors the
    class indices are range-checked; on the GPU they are not (that would cost a sync): an index outside 0 .. C - 1 gives
    that graph a NaN loss history, and its masks follow softmax(out_g) alone.
    From the epoch after the hard masks exist the loss also holds
    edge_size * sum(m) + edge_ent * mean(ent(m)) over g's hard edges and node_feat_size * mean(m) + node_feat_ent *
    mean(ent(m)) over its hard node entries (m = sigmoid(logit), ent(m) = -m log(m + 1e-15) - (1 - m) log(1 - m + 1e-15);
    a term over an empty set is 0); one torch-default Adam step (`lr`, betas 0.9 / 0.999, eps 1e-8; the rule of
    `optim.FusedAdam`) on both masks; and after the very first step hard = (gradient != 0), so an entry that is not
    hard never moves.  The result masks are sigmoid(logit) with the entries that are not hard set to 0.

    `init_state` draws n = 0.1 randn(N, F), then e = randn(E) * std_g with std_g = sqrt(2) * sqrt(2 / (2 N_g)) from the
    graph's own node count, from a CPU generator.  A call with `state=None` starts from `init_state(batch, generator)`;
    passing a returned state continues the fit (the state's tensors are updated in place).  `epochs_per_launch` splits
    the epochs into several launches (default: one launch); the result is bitwise independent of the split, of the run
    and of the rest of the batch.  The weights are read, never written; no mask is ever attached to the model.  Buffers
    are allocated for the largest call seen and reused (with `target` and `state` given a call allocates nothing); the
    returned masks, outputs and history are views of them, overwritten by the next call.

    When `reason(batch)` is not None (shape outside the kernel, CPU tensors, `use_fused` off) the same call runs `loop`:
    identical semantics and state, one `ExplainStep` call per epoch for the gradients (plain torch autograd on CPU
    tensors) and torch ops for the regularisers and Adam.  `last_path` says which one ran ("fused" / "loop")."""

    MODES = ("regression", "multiclass_classification")
    KERNEL, NAME = _lib.HCG_EXPLAIN_FIT, "ExplainFit"

    def __init__(self, model: torch.nn.Module, epochs: int = 100, lr: float = 0.01, coeffs: Optional[dict] = None,
                 mode: str = "regression"):
        if int(epochs) < 1:
            raise ValueError(f"epochs must be at least 1; got {epochs}")
        if mode not in self.MODES:
            raise ValueError(f"mode must be one of {self.MODES}; got {mode!r}")
        self.mode = mode
        self._ce = mode == "multiclass_classification"
        if self._ce and int(getattr(model, "_n_classes", 2)) < 2:
            raise ValueError(f"mode {mode!r} needs a model of two classes or more (n_classes >= 2); this one has {int(model._n_classes)}")
        super().__init__(model)
        self.epochs, self.lr = int(epochs), float(lr)
        self.coeffs = dict(DEFAULT_COEFFS)
        for k, v in (coeffs or {}).items():
            if k not in DEFAULT_COEFFS:
                raise ValueError(f"unknown coefficient {k!r}; known: {sorted(DEFAULT_COEFFS)}")
            self.coeffs[k] = float(v)
        self._step = ExplainStep(model, apply_sigmoid=True)

    # ------------------------------------------------------------------ state
    @staticmethod
    def _owners(batch):
        """-> (graph of every node [N], graph of every edge [E]) on the batch's device"""
        return batch.batch, batch.batch[batch.edge_index[1]]

    def init_state(self, batch, generator: Optional[torch.Generator] = None) -> ExplainFitState:
        """A fresh state on the batch's device, drawn from `generator` (a CPU generator; None: torch's default one):
        the node logits first, then the edge logits."""
        (N, F), E, B = batch.x.shape, int(batch.edge_index.shape[1]), int(batch.num_graphs)
        dev = batch.x.device
        node = 0.1 * torch.randn(N, F, generator=generator)
        nodes = torch.bincount(batch.batch, minlength=B).cpu().clamp_min(1).to(torch.float32)
        std = math.sqrt(2.0) * torch.sqrt(2.0 / (2.0 * nodes))              # calculate_gain('relu') * sqrt(2 / (2 N_g))
        edge = torch.randn(E, generator=generator) * std[self._owners(batch)[1].cpu()]
        f32 = dict(dtype=torch.float32, device=dev)
        return ExplainFitState(edge.to(dev), torch.zeros(E, **f32), torch.zeros(E, **f32),
                               torch.zeros(E, dtype=torch.bool, device=dev),
                               node.to(dev), torch.zeros(N, F, **f32), torch.zeros(N, F, **f32),
                               torch.zeros(N, F, dtype=torch.bool, device=dev),
                               torch.zeros(B, 2, dtype=torch.int32, device=dev), 0)

    @staticmethod
    def _check_state(state, batch):
        (N, F), E, B = batch.x.shape, int(batch.edge_index.shape[1]), int(batch.num_graphs)
        if not isinstance(state, ExplainFitState):
            raise ValueError(f"state must be an ExplainFitState; got {type(state).__name__}")
        want = dict(edge_logit=((E,), torch.float32), edge_exp_avg=((E,), torch.float32), edge_exp_avg_sq=((E,), torch.float32),
                    edge_hard=((E,), torch.bool), node_logit=((N, F), torch.float32), node_exp_avg=((N, F), torch.float32),
                    node_exp_avg_sq=((N, F), torch.float32), node_hard=((N, F), torch.bool), hard_count=((B, 2), torch.int32))
        for name, t in state.tensors():
            shape, dtype = want[name]
            if not torch.is_tensor(t) or t.dtype != dtype or tuple(t.shape) != shape or not t.is_contiguous():
                raise ValueError(f"state.{name} must be a contiguous {dtype} tensor of shape {shape} for this batch; got "
                                 f"{getattr(t, 'dtype', type(t))} {tuple(getattr(t, 'shape', ()))}")
            if t.device != batch.x.device:
                raise ValueError(f"state.{name} is on {t.device}, the batch on {batch.x.device}")
        if int(state.step) < 0:
            raise ValueError(f"state.step must not be negative; got {state.step}")

    def _target(self, batch, target):
        B, C = int(batch.num_graphs), int(self.model._n_classes)
        if self._ce and C < 2:
            raise ValueError(f"mode {self.mode!r} needs a model of two classes or more (n_classes >= 2); this one has {C}")
        if target is None:
            with torch.no_grad():
                if batch.x.is_cuda:
                    target = self.model(batch).reshape(B, C).clone()
                else:
                    ones = torch.ones(batch.edge_index.shape[1], dtype=batch.x.dtype)
                    target = _frozen.torch_forward(self.model, batch.x, batch.edge_index, batch.batch, B, ones).reshape(B, C)
                if self._ce:
                    target = target.argmax(dim=1)           # (on the batch's device, no sync; a tie: the first maximal index)
        if self._ce:
            if not torch.is_tensor(target) or target.dtype != torch.int64 or tuple(target.shape) != (B,) or not target.is_contiguous():
                raise ValueError(f"in mode {self.mode!r} target must be a contiguous int64 tensor of shape {(B,)} (one class index "
                                 f"per graph); got {getattr(target, 'dtype', type(target))} {tuple(getattr(target, 'shape', ()))}")
            if not target.is_cuda and B > 0 and (int(target.min()) < 0 or int(target.max()) >= C):
                raise ValueError(f"target holds class indices outside 0 .. {C - 1}")
            return target.detach()
        if target.dtype != torch.float32 or tuple(target.shape) != (B, C) or not target.is_contiguous():
            raise ValueError(f"target must be a contiguous float32 tensor of shape {(B, C)}; got {target.dtype} {tuple(target.shape)}")
        return target.detach()

    # ------------------------------------------------------------------ the call
    def __call__(self, batch, target=None, state: Optional[ExplainFitState] = None, epochs: Optional[int] = None,
                 generator: Optional[torch.Generator] = None, epochs_per_launch: Optional[int] = None) -> ExplainFitResult:
        T = self.epochs if epochs is None else int(epochs)
        if T < 1:
            raise ValueError(f"epochs must be at least 1; got {epochs}")
        per = T if epochs_per_launch is None else int(epochs_per_launch)
        if per < 1:
            raise ValueError(f"epochs_per_launch must be at least 1; got {epochs_per_launch}")
        a = self._args
        why = self._shape_args(a, batch)
        if why is not None:
            return self.loop(batch, target, state, T, generator)
        x = _frozen.batch_x(batch, target)
        N, F, E, B, C = a.N, a.F, a.E, a.B, a.C
        if state is None:
            state = self.init_state(batch, generator)
        self._check_state(state, batch)
        tg = self._target(batch, target)
        take, dev = self._bufs.take, x.device
        out, hist = take("out", (B, C), dev), take("hist", (T, B), dev)
        edge, node = take("edge", (E,), dev), take("node", (N, F), dev)
        p = _lib.ptr
        self._fill(a, _lib.HCG_EXPLAIN_TARGET_CLASS if self._ce else 0,        # (how the library reads the target slot)
                   batch, x, self._weights(dev), self._bufs.workspace(int(a.workspace_bytes_needed), dev))
        a.target, a.out = p(tg), _frozen.front(out)
        s = state
        a.fit_edge_logit, a.fit_edge_exp_avg, a.fit_edge_exp_avg_sq, a.fit_edge_hard = p(s.edge_logit), p(s.edge_exp_avg), p(s.edge_exp_avg_sq), p(s.edge_hard)
        a.fit_node_logit, a.fit_node_exp_avg, a.fit_node_exp_avg_sq, a.fit_node_hard = p(s.node_logit), p(s.node_exp_avg), p(s.node_exp_avg_sq), p(s.node_hard)
        a.fit_hard_count, a.fit_edge_mask_out, a.fit_node_mask_out = p(s.hard_count), _frozen.front(edge), _frozen.front(node)
        a.fit_lr, a.fit_beta1, a.fit_beta2, a.fit_eps = self.lr, BETA1, BETA2, ADAM_EPS
        for i, k in enumerate(("edge_size", "edge_ent", "node_feat_size", "node_feat_ent")):
            a.fit_coeffs[i] = self.coeffs[k]
        lib, stream = _lib.load(), _lib.stream_ptr()
        for first in range(0, T, per):
            a.step_first, a.epoch_count = int(s.step), min(per, T - first)
            a.fit_loss_hist = _frozen.front(hist) + 4 * first * B
            _lib.check(lib.hcg_explain(ctypes.addressof(a), stream), "hcg_explain (fit)")
            s.step = int(s.step) + int(a.epoch_count)
        self.last_path = "fused"
        return ExplainFitResult(edge, node, out, hist, s)

    # ------------------------------------------------------------------ the loop path (any shape, CPU tensors)
    def _grads(self, batch, s, target):
        """-> (out [B, C], loss [B], d loss / d edge logits, d loss / d node logits) of one epoch"""
        if batch.x.is_cuda:
            r = self._step(batch, s.edge_logit, s.node_logit, **{"target_class" if self._ce else "target": target})
            return r.out, r.loss, r.d_edge_mask, r.d_node_mask
        em = s.edge_logit.detach().clone().requires_grad_(True)
        nm = s.node_logit.detach().clone().requires_grad_(True)
        B = int(batch.num_graphs)
        with torch.enable_grad():
            out = _frozen.torch_forward(self.model, batch.x * nm.sigmoid(), batch.edge_index, batch.batch, B, em.sigmoid()).reshape(B, -1)
            loss = F_.cross_entropy(out, target, reduction="none") if self._ce else ((out - target) ** 2).mean(dim=1)
            d_e, d_n = torch.autograd.grad(loss.sum(), [em, nm])           # (no parameter's .grad is touched)
        return out.detach(), loss.detach(), d_e, d_n

    def loop(self, batch, target=None, state: Optional[ExplainFitState] = None, epochs: Optional[int] = None,
             generator: Optional[torch.Generator] = None) -> ExplainFitResult:
        """One `ExplainStep` call per epoch, the regularisers and Adam in torch ops (see the class docstring), whatever
        `reason(batch)` says."""
        T = self.epochs if epochs is None else int(epochs)
        if T < 1:
            raise ValueError(f"epochs must be at least 1; got {epochs}")
        B = int(batch.num_graphs)
        s = self.init_state(batch, generator) if state is None else state
        self._check_state(s, batch)
        tg = self._target(batch, target)
        node_g, edge_g = self._owners(batch)
        c = self.coeffs
        hist = torch.zeros(T, B, dtype=torch.float32, device=batch.x.device)
        out = None
        for t in range(T):
            out, loss, g_e, g_n = self._grads(batch, s, tg)
            hist[t] = loss
            g_e, g_n = g_e.clone(), g_n.clone()
            if s.step > 0:
                cnt = s.hard_count.to(torch.float32)
                inv = torch.where(cnt > 0, 1.0 / cnt.clamp_min(1.0), torch.zeros_like(cnt))
                m = s.edge_logit.sigmoid()
                g_e += s.edge_hard * (c["edge_size"] + c["edge_ent"] * inv[edge_g, 0] * _entropy_grad(m)) * (m * (1 - m))
                m = s.node_logit.sigmoid()
                inv_n = inv[node_g, 1].unsqueeze(1)
                g_n += s.node_hard * (c["node_feat_size"] * inv_n + c["node_feat_ent"] * inv_n * _entropy_grad(m)) * (m * (1 - m))
            k = s.step + 1
            # (the kernel's scalars: float32 betas, the corrections in double from the integer step, rounded to float32)
            one = torch.tensor(1.0, dtype=torch.float32)
            b1, b2 = float(torch.tensor(BETA1, dtype=torch.float32)), float(torch.tensor(BETA2, dtype=torch.float32))
            not_b1, not_b2 = float(one - b1), float(one - b2)           # 1 - beta in float32, as hcg_adam_update has it
            step_size = float(torch.tensor(self.lr, dtype=torch.float32) / torch.tensor(1.0 - b1 ** k, dtype=torch.float32))
            bc2_sqrt = float(torch.tensor(math.sqrt(1.0 - b2 ** k), dtype=torch.float32))
            for p_, g_, m_, v_ in ((s.edge_logit, g_e, s.edge_exp_avg, s.edge_exp_avg_sq),
                                   (s.node_logit, g_n, s.node_exp_avg, s.node_exp_avg_sq)):
                m_.mul_(b1).add_(g_, alpha=not_b1)
                v_.mul_(b2).addcmul_(g_, g_, value=not_b2)
                p_.addcdiv_(m_, v_.sqrt().div_(bc2_sqrt).add_(ADAM_EPS), value=-step_size)
            if s.step == 0:
                s.edge_hard.copy_(g_e != 0)
                s.node_hard.copy_(g_n != 0)
                s.hard_count[:, 0] = torch.bincount(edge_g[s.edge_hard], minlength=B).to(torch.int32)
                s.hard_count[:, 1] = torch.bincount(node_g, weights=s.node_hard.sum(dim=1).to(torch.float64), minlength=B).to(torch.int32)
            s.step += 1
        self.last_path = "loop"
        return ExplainFitResult(s.edge_logit.sigmoid() * s.edge_hard, s.node_logit.sigmoid() * s.node_hard, out, hist, s)
