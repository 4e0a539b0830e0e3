"""Gradient attributions for a batch of graphs: integrated gradients, input x gradient, saliency -- of one model
(`IntegratedGradients`) or of an ensemble of models in one launch with the mean and the standard deviation over the models
(`EnsembleAttribution`).

The reference's explain stage reaches Captum through `torch_geometric.explain.Explainer(CaptumExplainer(name), ...,
node_mask_type='attributes', edge_mask_type='object')` (scripts_experiments/explain_gnn.py); `ShapleySampling` serves the
name it uses, `'ShapleyValueSampling'`.  The same entry point takes `'IntegratedGradients'`: attributions of the same kind
(the same features, baseline 0, one value per node-feature entry and per edge) for `n_steps` forward and backward passes
per graph instead of one forward per feature per permutation.  `IntegratedGradients` runs the whole path of every graph
of a batch in ONE launch (csrc/explain.hip: `ExplainStep`'s kernel with a loop over the quadrature points inside).  No
artefact of the reference pins these values: parity is against an fp64 restatement on the oracle
(tests/integrated_ref.py).
"""
from __future__ import annotations

import ctypes
from typing import NamedTuple, Optional, Sequence

import numpy as np
import torch

from . import _frozen, _lib
from ._frozen import CUS, LAUNCH_SECONDS
from .ensemble import FrozenEnsemble
from .explain import ExplainStep

METHODS = ("gausslegendre", "riemann_middle", "gradient")
ENDPOINT_METHODS = ("riemann_left", "riemann_right", "riemann_trapezoid")
LAUNCH_BUDGET_BYTES = 1 << 30      # workspace + per-model attribution arrays of one `EnsembleAttribution` launch (default chunking)
STEP_SECONDS = 400e-6              # one forward + backward of a workgroup at the shape limits: an estimate (default_steps_per_launch)


class IntegratedGradientsResult(NamedTuple):
    node_attr: torch.Tensor      # [N, F]
    edge_attr: torch.Tensor      # [E], the batch's edge order
    out_full: torch.Tensor       # [B, C] the model's output at masks of 1 (= the plain forward)
    out_base: torch.Tensor       # [B, C] at masks of 0


def quadrature(method: str, n_steps: int):
    """-> (alpha [n_steps], weight [n_steps]) float32 CPU tensors: the points in (0, 1) and their weights, computed in
    float64 and rounded once.  These float32 values are what every path uses.
        gausslegendre    numpy.polynomial.legendre.leggauss(n) mapped to [0, 1], weights halved
        riemann_middle   alpha_k = (k + 1/2) / n, w_k = 1 / n
        gradient         one point: alpha = 1, w = 1 (`n_steps` must be 1)
    Captum's methods with a point at 0 or 1 (riemann_left / _right / _trapezoid) are refused: at alpha = 0 every node row
    of a graph is identical, the max-pool is one large exact tie and the gradient there is a convention, not a value."""
    n = int(n_steps)
    if method in ENDPOINT_METHODS:
        raise ValueError(f"method {method!r} has a quadrature point at alpha = 0 or 1; at alpha = 0 every node row of a graph is "
                         f"identical and the max-pool is one exact tie, so the gradient there is not defined by the model: use "
                         f"'gausslegendre' or 'riemann_middle'")
    if method not in METHODS:
        raise ValueError(f"method must be one of {METHODS}; got {method!r}")
    if n < 1:
        raise ValueError(f"n_steps must be at least 1; got {n_steps}")
    if method == "gausslegendre":
        t, w = np.polynomial.legendre.leggauss(n)
        alpha, weight = (t + 1.0) / 2.0, w / 2.0
    elif method == "riemann_middle":
        alpha, weight = (np.arange(n, dtype=np.float64) + 0.5) / n, np.full(n, 1.0 / n, dtype=np.float64)
    else:
        if n != 1:
            raise ValueError(f"method 'gradient' is one step; got n_steps = {n_steps}")
        alpha, weight = np.ones(1), np.ones(1)
    return torch.from_numpy(np.ascontiguousarray(alpha)).to(torch.float32), torch.from_numpy(np.ascontiguousarray(weight)).to(torch.float32)


class _Path:
    """The path of `IntegratedGradients` and `EnsembleAttribution`: method, step count and `saliency` with their checks, the
    quadrature points on the device, the default split of the steps into launches, and the launch's `path_` members."""

    def _init_path(self, n_steps: int, method: str, saliency: bool):
        if saliency and method != "gradient":
            raise ValueError(f"saliency=True is the absolute value of method='gradient'; got method {method!r}")
        if method == "gradient":
            n_steps = 1
        quadrature(method, n_steps)                         # (refuses the method or the step count)
        self.n_steps, self.method, self.saliency = int(n_steps), method, bool(saliency)
        self.last_class_index: Optional[int] = None
        self._points = {}           # (n_steps, device) -> (alpha, weight) on the device

    @staticmethod
    def default_steps_per_launch(n_steps: int, num_graphs: int) -> int:
        """Steps of one launch: as many as keep its run time near `LAUNCH_SECONDS`, at least 1.  The device runs
        the graphs in ceil(num_graphs / CUS) rounds of one workgroup per compute unit (the occupancy at the shape limits'
        LDS), each step of a round taking `STEP_SECONDS`.  `STEP_SECONDS` is an ESTIMATE: `ExplainFit` -- the same forward
        and backward per epoch -- takes about 90 us per epoch and workgroup on real-size graphs and two conv layers (README:
        144.8 ms for 100 epochs of 4096 graphs), extrapolated to 224 nodes and four layers; nobody has timed a launch at the
        limit shapes."""
        rounds = max(1, -(-int(num_graphs) // CUS))
        return max(1, min(int(n_steps), int(LAUNCH_SECONDS / (rounds * STEP_SECONDS))))

    def _steps(self, n_steps) -> int:
        n = self.n_steps if n_steps is None else int(n_steps)
        if self.method == "gradient" and n != 1:
            raise ValueError(f"method 'gradient' is one step; got n_steps = {n_steps}")
        if n < 1:
            raise ValueError(f"n_steps must be at least 1; got {n_steps}")
        return n

    def _fill_path(self, a, n: int, cls: int, dev):
        key = (n, str(dev))
        if key not in self._points:
            alpha, weight = quadrature(self.method, n)
            self._points[key] = (alpha.to(dev), weight.to(dev))
        alpha, weight = self._points[key]
        a.path_alpha, a.path_weight = _lib.ptr(alpha), _lib.ptr(weight)
        a.path_steps, a.path_class_index = n, cls


class IntegratedGradients(_Path, _frozen.FrozenModel):
    """Integrated gradients of a frozen model for a whole batch of graphs, one launch per call.

        ig = IntegratedGradients(model, n_steps=50, method="gausslegendre")
        r = ig(batch, class_index=0, n_steps=None, steps_per_launch=None)
        # IntegratedGradientsResult(node_attr [N, F], edge_attr [E], out_full [B, C], out_base [B, C])
        ig.convergence_delta(batch, r)      # [B] float64

    Definition: Captum's `IntegratedGradients` as torch_geometric's `CaptumExplainer` calls it.  The inputs are a node
    mask of ones [N, F] and an edge mask of ones [E], the baselines are 0.  The masks mean what they mean in
    `ExplainStep(apply_sigmoid=False)`: `x * node_mask` goes into the first layer; the edge mask multiplies every message
    of every conv layer after gcn_norm; dinv comes from the unmasked in-degree; self loops keep 1, and an explicit (i, i)
    edge is part of the unit self loop.  For graph g, output column c = `class_index` and quadrature points alpha_k in
    (0, 1) with weights w_k (`quadrature(method, n_steps)`), G_k is the gradient of out[g, c] with respect to (node mask,
    edge mask) evaluated with every node-mask and every edge-mask entry of the graph equal to alpha_k; the attribution is
    sum_k w_k G_k, summed in float32 in the order k = 0, 1, ... (the factor input - baseline is 1).  An entry of x that is
    exactly 0 and an explicit (i, i) edge get exactly 0.  `out_full` / `out_base` are the outputs at masks of 1 and of 0.

    `convergence_delta(batch, r)` = sum of graph g's attributions - (out_full - out_base)[g, c], in float64: a diagnostic.
    The path of a LeakyReLU / max-pool model is piecewise polynomial with thousands of kinks, so the quadrature does not
    close this gap at any practical `n_steps`; nothing here asserts that it does.

    `method="gradient"` is the one-step case alpha = 1, w = 1: `CaptumExplainer`'s `InputXGradient` on the masks (the
    gradient at masks of ones); with `saliency=True` its absolute value (`Saliency`).

    The steps are split into launches of `steps_per_launch` (None: `default_steps_per_launch`); the result is bitwise
    independent of that split, of the run and of the rest of the batch.  The weights are read, never written; no
    parameter's `.grad` is touched and no mask stays attached to the model.  `batch` needs the collate metadata
    `ExplainStep` needs.  Buffers are allocated for the largest call seen and reused (in steady state a call allocates
    nothing); the returned tensors are views of them, overwritten by the next call.

    When `reason(batch)` is not None (shape outside the kernel, `embedding_dim != 64`, CPU tensors, `use_fused` off) the same
    call runs `loop`: one `ExplainStep(apply_sigmoid=False)` call per step with `dout` = the one-hot column on GPU tensors,
    plain torch autograd on CPU tensors, accumulated in float32 in step order.  `last_path` says which one ran ("fused" /
    "loop")."""

    KERNEL, NAME = _lib.HCG_EXPLAIN_INTEGRATED, "IntegratedGradients"

    def __init__(self, model: torch.nn.Module, n_steps: int = 50, method: str = "gausslegendre", saliency: bool = False):
        _frozen.FrozenModel.__init__(self, model)
        self._init_path(n_steps, method, saliency)
        self._step = ExplainStep(model, apply_sigmoid=False)

    # ------------------------------------------------------------------ the call
    def __call__(self, batch, class_index: int = 0, n_steps: Optional[int] = None,
                 steps_per_launch: Optional[int] = None) -> IntegratedGradientsResult:
        n = self._steps(n_steps)
        cls = self._class(class_index)
        if steps_per_launch is not None and int(steps_per_launch) < 1:
            raise ValueError(f"steps_per_launch must be at least 1; got {steps_per_launch}")
        a = self._args
        why = self._shape_args(a, batch)
        if why is not None:
            return self.loop(batch, cls, n)
        x = _frozen.batch_x(batch)
        N, F, E, B, C = a.N, a.F, a.E, a.B, a.C
        per = self.default_steps_per_launch(n, B) if steps_per_launch is None else min(int(steps_per_launch), n)
        take, front, dev = self._bufs.take, _frozen.front, x.device
        node, edge = take("node", (N, F), dev), take("edge", (E,), dev)
        full, base = take("full", (B, C), dev), take("base", (B, C), dev)
        self._fill(a, 0, batch, x, self._weights(dev), self._bufs.workspace(int(a.workspace_bytes_needed), dev))
        self._fill_path(a, n, cls, dev)
        a.path_node_attr, a.path_edge_attr, a.path_out_full, a.path_out_base = front(node), front(edge), front(full), front(base)
        lib, stream = _lib.load(), _lib.stream_ptr()
        for first in range(0, n, per):
            a.path_step_first, a.path_step_count = first, min(per, n - first)
            _lib.check(lib.hcg_explain(ctypes.addressof(a), stream), "hcg_explain (integrated)")
        if self.saliency:
            node.abs_()
            edge.abs_()
        self.last_path, self.last_class_index = "fused", cls
        return IntegratedGradientsResult(node, edge, full, base)

    # ------------------------------------------------------------------ the loop path (any shape, CPU tensors)
    def _grads(self, batch, alpha: float, onehot):
        """-> (d out[:, c] / d node mask [N, F], d out[:, c] / d edge mask [E]) with every mask entry = alpha"""
        (N, F), E, B = batch.x.shape, int(batch.edge_index.shape[1]), int(batch.num_graphs)
        dev = batch.x.device
        if batch.x.is_cuda:
            em = torch.full((E,), alpha, dtype=torch.float32, device=dev)
            nm = torch.full((N, F), alpha, dtype=torch.float32, device=dev)
            r = self._step(batch, em, nm, dout=onehot)
            return r.d_node_mask, r.d_edge_mask
        em = torch.full((E,), alpha, dtype=torch.float32).requires_grad_(True)
        nm = torch.full((N, F), alpha, dtype=torch.float32).requires_grad_(True)
        with torch.enable_grad():
            out = _frozen.torch_forward(self.model, batch.x.detach() * nm, batch.edge_index, batch.batch, B, em).reshape(B, -1)
            d_n, d_e = torch.autograd.grad((out * onehot).sum(), [nm, em])     # (no parameter's .grad is touched)
        return d_n, d_e

    def _forward(self, batch, value: float):
        (N, F), E, B = batch.x.shape, int(batch.edge_index.shape[1]), int(batch.num_graphs)
        dev = batch.x.device
        em = torch.full((E,), value, dtype=torch.float32, device=dev)
        nm = torch.full((N, F), value, dtype=torch.float32, device=dev)
        with torch.no_grad():
            if batch.x.is_cuda:
                return self._step(batch, em, nm).out.reshape(B, -1).clone()
            return _frozen.torch_forward(self.model, batch.x * nm, batch.edge_index, batch.batch, B, em).reshape(B, -1)

    def loop(self, batch, class_index: int = 0, n_steps: Optional[int] = None) -> IntegratedGradientsResult:
        """One `ExplainStep` call per quadrature point (see the class docstring), whatever `reason(batch)` says."""
        n = self._steps(n_steps)
        cls = self._class(class_index)
        (N, F), E, B = batch.x.shape, int(batch.edge_index.shape[1]), int(batch.num_graphs)
        dev = batch.x.device
        alpha, weight = quadrature(self.method, n)
        onehot = torch.zeros(B, int(self.model._n_classes), dtype=torch.float32, device=dev)
        onehot[:, cls] = 1.0
        node = torch.zeros(N, F, dtype=torch.float32, device=dev)
        edge = torch.zeros(E, dtype=torch.float32, device=dev)
        for k in range(n):
            d_n, d_e = self._grads(batch, float(alpha[k]), onehot)
            node.add_(d_n, alpha=float(weight[k]))
            edge.add_(d_e, alpha=float(weight[k]))
        if self.saliency:
            node.abs_()
            edge.abs_()
        out_full, out_base = self._forward(batch, 1.0), self._forward(batch, 0.0)
        self.last_path, self.last_class_index = "loop", cls
        return IntegratedGradientsResult(node, edge, out_full, out_base)

    # ------------------------------------------------------------------ the diagnostic
    def convergence_delta(self, batch, result: IntegratedGradientsResult, class_index: Optional[int] = None) -> torch.Tensor:
        """[B] float64: sum of graph g's node and edge attributions - (out_full - out_base)[g, c]; c = `class_index`
        (None: the last call's)."""
        if class_index is None:
            class_index = self.last_class_index
        if class_index is None:
            raise ValueError("class_index is needed before the first call")
        return convergence_delta(batch, result, self._class(class_index))


def convergence_delta(batch, result, class_index: int) -> torch.Tensor:
    """The formula of `IntegratedGradients.convergence_delta` on any (node_attr, edge_attr, out_full, out_base), in float64."""
    B = int(batch.num_graphs)
    node_attr, edge_attr, out_full, out_base = result[:4]
    dev = node_attr.device
    owner_n = batch.batch.to(dev)
    owner_e = owner_n[batch.edge_index[1].to(dev)]
    total = torch.zeros(B, dtype=torch.float64, device=dev)
    total.index_add_(0, owner_n, node_attr.double().sum(dim=1))
    total.index_add_(0, owner_e, edge_attr.double())
    return total - (out_full.double()[:, class_index] - out_base.double()[:, class_index])



class EnsembleAttributionResult(NamedTuple):
    node_mean: torch.Tensor             # [N, F]  mean over the models of their node attributions
    node_std: torch.Tensor              # [N, F]  population standard deviation over the models
    edge_mean: torch.Tensor             # [E], the batch's edge order
    edge_std: torch.Tensor              # [E]
    out_full: torch.Tensor              # [M, B, C] every model's output at masks of 1
    out_base: torch.Tensor              # [M, B, C] at masks of 0
    node_attr: Optional[torch.Tensor]   # [M, N, F] the per-model attributions; None unless asked for
    edge_attr: Optional[torch.Tensor]   # [M, E]


class EnsembleAttribution(_Path, FrozenEnsemble):
    """Integrated gradients of M frozen models of one architecture for a whole batch of graphs: every (graph, model) pair is
    one workgroup of ONE launch, and the mean and the standard deviation over the models are taken on the device.

        ea = EnsembleAttribution(models, n_steps=50, method="gausslegendre", saliency=False)
        r = ea(batch, class_index=0, per_model=False, models_per_launch=None, steps_per_launch=None)
        # EnsembleAttributionResult(node_mean [N, F], node_std [N, F], edge_mean [E], edge_std [E],
        #                           out_full [M, B, C], out_base [M, B, C], node_attr [M, N, F] | None, edge_attr [M, E] | None)
        ea.refresh(); ea.reason(batch); ea.last_path

    `models` are checked and snapshotted as `EnsemblePredict` does it: the same (node features, embedding_dim, classes,
    conv layers, readout layers) for every model (`ValueError` otherwise), weights stacked once into contiguous [M, ...]
    buffers; later changes of a model do not show until `refresh()` re-stacks them in place.  Methods, step-count rules
    and `saliency` are `IntegratedGradients`': `node_attr[m]` / `edge_attr[m]` / `out_full[m]` / `out_base[m]` are bit for bit
    what `IntegratedGradients(models[m], ...)(batch)` returns, whatever the other models are.

    Integrated gradients are linear in the model output, so `node_mean` / `edge_mean` ARE the integrated gradients of the
    ensemble's mean prediction (`EnsemblePredict.mean`); `node_std` / `edge_std` (population form, ddof = 0, as
    `EnsemblePredict.std`) say where the models disagree.  With `saliency=True` the per-model values are absolute values
    and the mean is THEIR mean -- not the saliency of the mean output, which is `abs(node_mean)` of `method="gradient"`.
    The moments are Welford's recurrence in float32 over the models in ascending order (csrc/explain.hip k_model_moments):
    an entry that is 0 in every model (an `x` entry equal to 0, an explicit (i, i) edge) has mean and std exactly 0, and a
    one-model ensemble has the model's attributions as mean and std exactly 0.

    The models run in chunks of `models_per_launch` (None: `default_models_per_launch`), inside a chunk the steps in chunks
    of `steps_per_launch` (None: `IntegratedGradients.default_steps_per_launch` with graphs x models of the chunk as the
    workgroup count); one moments launch follows each chunk of models.  Every returned value is bitwise independent of
    both splits, of the run and of the rest of the batch.  With `per_model=False` only one chunk's [models_per_launch, ...]
    attribution arrays exist (at 90 models x 535 graphs the full arrays are about 0.4 GB).  Buffers grow to the largest
    call and are reused (a warm call allocates nothing); the returned tensors are views of them, overwritten by the next
    call.  No parameter's `.grad` is touched and no mask stays on a model.

    When `reason(batch)` is not None (shape outside the kernel, `embedding_dim != 64`, CPU tensors, `use_fused` off on any
    model) the same call runs `IntegratedGradients(model_k).loop` per model -- on the models' CURRENT weights -- and takes
    the moments with torch ops (`mean(0)`, `std(0, unbiased=False)`); `last_path` says which one ran ("fused" / "loop")."""

    KERNEL, NAME = _lib.HCG_EXPLAIN_INTEGRATED, "EnsembleAttribution"

    def __init__(self, models: Sequence[torch.nn.Module], n_steps: int = 50, method: str = "gausslegendre", saliency: bool = False):
        FrozenEnsemble.__init__(self, models)
        self._init_path(n_steps, method, saliency)
        self._singles = [IntegratedGradients(m, n_steps, method, saliency) for m in self.models]       # the loop path's workers

    def _shape_args(self, a, batch) -> Optional[str]:
        """None when the kernel takes these models and `batch`; `a` then holds the shapes and the ONE-model workspace bytes"""
        return super()._shape_args(a, batch, n_models=1)

    @staticmethod
    def default_models_per_launch(n_models: int, workspace_bytes: int, entries: int, budget: int = LAUNCH_BUDGET_BYTES) -> int:
        """Models of one launch: all of them, unless their workspace slices (`workspace_bytes` each, the library's
        one-model figure) plus their attribution rows (`entries` = N F + E float32 each) exceed `budget` bytes
        (`LAUNCH_BUDGET_BYTES`); then as many as fit, at least 1."""
        per = int(workspace_bytes) + 4 * int(entries)
        return max(1, min(int(n_models), int(budget) // max(per, 1)))

    # ------------------------------------------------------------------ the call
    def __call__(self, batch, class_index: int = 0, per_model: bool = False, models_per_launch: Optional[int] = None,
                 steps_per_launch: Optional[int] = None, n_steps: Optional[int] = None) -> EnsembleAttributionResult:
        n = self._steps(n_steps)
        cls = self._class(class_index)
        for name, v in (("models_per_launch", models_per_launch), ("steps_per_launch", steps_per_launch)):
            if v is not None and int(v) < 1:
                raise ValueError(f"{name} must be at least 1; got {v}")
        a = self._args
        why = self._shape_args(a, batch)
        if why is not None:
            return self.loop(batch, cls, per_model, n)
        x = _frozen.batch_x(batch)
        dev = x.device
        M = len(self.models)
        N, F, E, B, C = a.N, a.F, a.E, a.B, a.C
        ws_one = int(a.workspace_bytes_needed)
        weights = self._weights(dev)
        Ml = self.default_models_per_launch(M, ws_one, N * F + E) if models_per_launch is None else min(int(models_per_launch), M)
        rows = M if per_model else Ml
        take, front = self._bufs.take, _frozen.front
        node, edge = take("node", (rows, N, F), dev), take("edge", (rows, E), dev)
        full, base = take("full", (M, B, C), dev), take("base", (M, B, C), dev)
        mom = {k: take(k, (N, F) if k.startswith("node") else (E,), dev)
               for k in ("node_mean", "node_m2", "node_std", "edge_mean", "edge_m2", "edge_std")}
        self._fill(a, 0, batch, x, None, self._bufs.workspace(Ml * ws_one, dev))
        self._fill_path(a, n, cls, dev)
        q = self._moments_block((mom["node_mean"], mom["node_m2"], mom["node_std"], N * F),
                                (mom["edge_mean"], mom["edge_m2"], mom["edge_std"], E))
        lib, stream = _lib.load(), _lib.stream_ptr()
        for m0, count, row0 in self._model_chunks(a, weights, Ml, per_model, q):
            q.mom_values0 = a.path_node_attr = front(node) + 4 * row0 * N * F
            q.mom_values1 = a.path_edge_attr = front(edge) + 4 * row0 * E
            a.path_out_full, a.path_out_base = front(full) + 4 * m0 * B * C, front(base) + 4 * m0 * B * C
            per = self.default_steps_per_launch(n, B * count) if steps_per_launch is None else min(int(steps_per_launch), n)
            for first in range(0, n, per):
                a.path_step_first, a.path_step_count = first, min(per, n - first)
                _lib.check(lib.hcg_explain(ctypes.addressof(a), stream), "hcg_explain (integrated, ensemble)")
            if self.saliency:
                node[row0:row0 + count].abs_()
                edge[row0:row0 + count].abs_()
        self.last_path, self.last_class_index = "fused", cls
        return EnsembleAttributionResult(
            mom["node_mean"], mom["node_std"], mom["edge_mean"], mom["edge_std"], full, base,
            node if per_model else None, edge if per_model else None)

    # ------------------------------------------------------------------ the loop path (any shape, CPU tensors)
    def loop(self, batch, class_index: int = 0, per_model: bool = False, n_steps: Optional[int] = None) -> EnsembleAttributionResult:
        """`IntegratedGradients(model_k).loop` per model on the models' current weights, the moments with torch ops."""
        rs = [ig.loop(batch, class_index, n_steps) for ig in self._singles]
        node, edge = torch.stack([r.node_attr for r in rs]), torch.stack([r.edge_attr for r in rs])
        self.last_path, self.last_class_index = "loop", int(class_index)
        return EnsembleAttributionResult(node.mean(0), node.std(0, unbiased=False), edge.mean(0), edge.std(0, unbiased=False),
                                         torch.stack([r.out_full for r in rs]), torch.stack([r.out_base for r in rs]),
                                         node if per_model else None, edge if per_model else None)
