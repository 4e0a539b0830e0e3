"""The host path the frozen-model classes share (`ExplainStep`, `ExplainFit`, `EnsemblePredict`, `ShapleySampling`, `CoalitionValues`,
`SubsetValues`, `GreedySelection`, `IntegratedGradients`, `EnsembleAttribution` and the ensemble classes of ensemble_shapley.py: one
graph per workgroup, all through `hcg_explain`).

    Frozen           what every class is: `last_path`, the argument block `_args`, the buffer pool `_bufs`, the support check
                     (`_shape_args`, `reason`, `lds_bytes`), the class-index check and `_fill`, which sets what every launch sets
    FrozenModel      one model: what it must look like, its weights checked for a launch, and `_masked_forward`, the masked
                     forward every loop path of the Shapley family runs (the ensembles' counterpart, `FrozenEnsemble`, lives
                     beside `stack_weights` in ensemble.py and holds the model-chunk loop and the moments block)
    Pool             name -> flat tensor, grow-only; a request returns the buffer's front in the shape asked for
    query            clears the WHOLE argument block, fills the shapes and asks the library; a class then sets every member
                     its launch reads, so nothing of an earlier launch (the `fit_` / `path_` / `mom_` / `shap_` members overlay
                     one union) can reach the next one
    positive         the check of every `*_per_launch` / `*_per_workgroup` / `*_per_job` argument
    launch_jobs      the jobs of a filled block in launches of `jobs_per_launch` (coalitions, subsets, a greedy round)
    torch_forward    the model's masked forward in plain torch ops: what every loop path runs on CPU tensors
    CUS, LAUNCH_SECONDS   what the launch-size estimates of shapley.py and attribution.py share

The order of a fused call: `_shape_args` (clears and queries; not None: the class's loop path), the class's own argument checks,
`_bufs.take` / `_bufs.workspace`, `_fill`, the class's own members, the launches.  Private: the classes are the interface.
What describes a batch's players -- group layout, group lists, permutations, subsets -- is _groups.py.
"""
from __future__ import annotations

import ctypes
import math
from typing import Optional

import torch
import torch.nn.functional as Fn

from . import _lib

MODEL_ATTRS = ("embedding_dim", "n_node_features", "n_convolutions", "readout_layers", "_n_classes", "conv1", "readout")
SLOPE = 0.01                       # nn.LeakyReLU() default (reference model/gcn.py:21, :63)
CUS = 256                          # compute units of an MI355X
LAUNCH_SECONDS = 1.0               # what one launch should stay near (the machines are shared)

# mode -> (the kernel's name in a reason, its node limit, the label of a failed query)
_MODES = {_lib.HCG_EXPLAIN_GRAPHS: ("one-launch explain", 224, "hcg_explain (query)"),
          _lib.HCG_EXPLAIN_ENSEMBLE: ("one-launch ensemble", 224, "hcg_explain (ensemble query)"),
          _lib.HCG_EXPLAIN_SHAPLEY: ("on-chip Shapley", 184, "hcg_explain (shapley query)"),
          _lib.HCG_EXPLAIN_FIT: ("one-launch explainer fit", 224, "hcg_explain (fit query)"),
          _lib.HCG_EXPLAIN_INTEGRATED: ("one-launch integrated gradients", 224, "hcg_explain (integrated query)"),
          _lib.HCG_EXPLAIN_COALITIONS: ("on-chip coalition", 184, "hcg_explain (coalitions query)"),
          _lib.HCG_EXPLAIN_SUBSETS: ("on-chip subset", 184, "hcg_explain (subsets query)"),
          _lib.HCG_EXPLAIN_GREEDY: ("on-chip greedy selection", 184, "hcg_explain (greedy query)")}


def model_shape(model):
    """-> (F, D, C, n_conv, R)"""
    m = model
    return int(m.n_node_features), int(m.embedding_dim), int(m._n_classes), int(m.n_convolutions), int(m.readout_layers)


def model_layers(model):
    """-> (conv layers, the readout's Linear layers), in layer order"""
    return [model.conv1] + list(model.conv_layers), [q[0] if isinstance(q, torch.nn.Sequential) else q for q in model.readout]


def model_reason(model) -> Optional[str]:
    if any(not hasattr(model, k) for k in MODEL_ATTRS):
        return "not a hcatgnet_amd GCN model"
    if not bool(getattr(model, "use_fused", True)):
        return "fused kernels disabled on the model"
    return None


def check_weights(tensors, device, message: str):
    for q in tensors:
        if q.dtype != torch.float32 or not q.is_contiguous() or q.device != device:
            raise _lib.HcgError(message)


def batch_reason(batch, F: int, what: str) -> Optional[str]:
    """Why `batch` cannot take a kernel of this family, from its host metadata; `what`: "model" or "models"."""
    if None in (getattr(batch, "max_nodes", None), getattr(batch, "max_edges", None)) or not getattr(batch, "edges_grouped", False):
        return "batch lacks collate metadata (max_nodes / max_edges / grouped edges)"
    if getattr(batch, "edge_weight", None) is not None:
        return "explicit edge weights " + ("are outside the ensemble kernel" if what == "models" else "cannot be combined with masks")
    if batch.x.shape[1] != F:
        return f"batch has {batch.x.shape[1]} node features, the {what} take{'s' if what == 'model' else ''} {F}"
    return None


def query(a, mode: int, shape, batch, **extra) -> Optional[str]:
    """Clear `a`, fill its shape fields from `shape` (`model_shape`) and `batch` (checked by `batch_reason`, or None) plus
    `extra`, and ask the library: None when the kernel takes them (`a.workspace_bytes_needed` is set), else the limits."""
    ctypes.memset(ctypes.addressof(a), 0, ctypes.sizeof(a))
    a.mode, a.flags = mode, _lib.HCG_EXPLAIN_QUERY
    a.F, a.D, a.C, a.n_conv, a.R = shape
    if batch is not None:
        a.N, a.E, a.B = int(batch.x.shape[0]), int(batch.edge_index.shape[1]), int(batch.num_graphs)
        a.max_nodes, a.max_edges = int(batch.max_nodes), int(batch.max_edges)
    for k, v in extra.items():
        setattr(a, k, v)
    kernel, nodes, label = _MODES[mode]
    rc = _lib.load().hcg_explain(ctypes.addressof(a), None)
    if rc == _lib.HCG_ERR_UNSUPPORTED:
        return (f"model / graph shape outside the {kernel} kernel (embedding_dim 64, <= 64 node features, <= 4 conv "
                f"layers, readout depth <= 4, <= 8 classes, graphs of <= {nodes} nodes and <= 1024 directed edges)")
    _lib.check(rc, label)
    return None


def batch_x(batch, *more):
    """batch.x, once it, the edges and `more` are on a GPU and x can be read in place"""
    _lib.require_gpu(batch.x, batch.edge_index, *more)
    if batch.x.dtype != torch.float32 or not batch.x.is_contiguous():
        raise ValueError("batch.x must be contiguous float32")
    return batch.x


class Pool(dict):
    """name -> flat tensor.  A buffer is as large as the largest request seen for its name (at least 1 element) and is
    replaced only by a larger request or another device; new storage is zero."""

    def __init__(self):
        super().__init__()
        self._last = {}             # name -> (shape, device, view) of the last request: a warm call builds no tensor at all

    def take(self, name: str, shape: tuple, dev, dtype=torch.float32) -> torch.Tensor:
        """The front of buffer `name` as a contiguous tensor of `shape`"""
        last = self._last.get(name)
        if last is not None and last[0] == shape and last[1] == dev:
            return last[2]
        numel = math.prod(shape)
        t = self.get(name)
        if t is None or t.numel() < numel or t.device != dev:
            t = self[name] = torch.zeros(max(numel, 1), dtype=dtype, device=dev)
        view = t[:numel].view(shape)
        self._last[name] = (shape, dev, view)
        return view

    def workspace(self, nbytes: int, dev) -> torch.Tensor:
        """The whole byte buffer "ws", at least `nbytes` and 256 bytes large; its contents are not defined"""
        t = self.get("ws")
        if t is None or t.numel() < nbytes or t.device != dev:
            t = self["ws"] = torch.empty(max(nbytes, 256), dtype=torch.uint8, device=dev)
        return t


def fill_weights(a, weights, first: int = 0):
    """`weights`: (conv weights, conv biases, readout weights, readout biases), lists of tensors in layer order: one model's,
    or an ensemble's stacked [M, ...] ones, then read from model `first` on (the library has no "first model" field)."""
    for slots, tensors in zip((a.conv_W, a.conv_b, a.head_W, a.head_b), weights):
        for i in range(len(slots)):
            slots[i] = tensors[i].data_ptr() + (4 * first * tensors[i].stride(0) if first else 0) if i < len(tensors) else None


def positive(name: str, value) -> Optional[int]:
    """None for None, else `value` as an int of at least 1 (ValueError otherwise): the check of every `*_per_launch`,
    `*_per_workgroup` and `*_per_job` argument; the caller supplies its default (`positive(...) or default`)."""
    if value is None:
        return None
    if int(value) < 1:
        raise ValueError(f"{name} must be at least 1; got {value}")
    return int(value)


def launch_jobs(a, first: int, count: int, per_launch: int, label: str, stream=None):
    """Run the jobs first .. first + count - 1 of the filled block `a` (`coal_jobs`) in launches of at most `per_launch` on
    `stream` (None: the current one); `label` names the launch in an error."""
    lib, addr = _lib.load(), ctypes.addressof(a)
    stream = _lib.stream_ptr() if stream is None else stream
    for at in range(first, first + count, per_launch):
        a.coal_job_first, a.coal_job_count = at, min(per_launch, first + count - at)
        _lib.check(lib.hcg_explain(addr, stream), label)


def front(view) -> Optional[int]:
    """Device address of the pool buffer that `view` (`Pool.take`) is the front of; None for None.  An empty view has no
    address of its own: the library still gets its buffer's, never NULL."""
    return None if view is None else view.data_ptr() or view.untyped_storage().data_ptr()


class Frozen:
    """What the six classes share.  A subclass names its kernel (`KERNEL`), itself (`NAME`, for messages), says "model" or
    "models" in a reason (`WHAT`) and whether a CPU batch is refused before anything else of it is read (`REFUSES_CPU`), and
    provides `_model_reason()`, `_shape()` (`model_shape`'s tuple) and `_planner()` (the model whose plan cache serves the batch)."""
    KERNEL: int = -1
    NAME = ""
    WHAT = "model"
    REFUSES_CPU = True

    def __init__(self):
        self.last_path: Optional[str] = None
        self._args = _lib.ExplainArgs()
        self._bufs = Pool()

    # ------------------------------------------------------------------ support check (host only, no sync)
    def _shape_args(self, a, batch, **extra) -> Optional[str]:
        why = self._model_reason()
        shape = None if why else self._shape()
        if why is None and batch is not None:
            why = "the batch is on the CPU" if self.REFUSES_CPU and not batch.x.is_cuda else batch_reason(batch, shape[0], self.WHAT)
        return why or query(a, self.KERNEL, shape, batch, **extra)

    def reason(self, batch=None) -> Optional[str]:
        """None when the model(s) (and `batch`) take the kernel, else why not.  Host metadata only."""
        return self._shape_args(_lib.ExplainArgs(), batch)

    def lds_bytes(self, batch) -> Optional[int]:
        """Dynamic LDS of one workgroup of the kernel for this batch, as the library's query reports it (the fit, the
        integrated-gradients and the Shapley kernel do); None when the batch does not take the kernel."""
        a = _lib.ExplainArgs()
        return int(a.lds_bytes) if self._shape_args(a, batch) is None else None

    def _class(self, class_index) -> int:
        C = self._shape()[2]
        if not 0 <= int(class_index) < C:
            raise ValueError(f"class_index must lie in 0 .. {C - 1}; got {class_index}")
        return int(class_index)

    # ------------------------------------------------------------------ what every launch sets
    def _fill(self, a, flags: int, batch, x, weights, ws=None):
        """The launch's flags, the graph, the slope, the weights (`fill_weights`; None: the caller fills them, chunk by
        chunk) and the workspace `ws`, if it has one."""
        p = _lib.ptr
        plan = self._planner()._plan_for(batch, x, batch.edge_index, batch.batch, None)
        a.flags, a.slope = flags, SLOPE
        a.x, a.edge_index, a.graph_ptr, a.edge_ptr = p(x), p(plan.edge_index), p(plan.graph_ptr), p(plan.edge_ptr)
        a.status = p(plan.status)
        if weights is not None:
            fill_weights(a, weights)
        if ws is not None:
            a.workspace, a.workspace_bytes = p(ws), ws.numel()


class FrozenModel(Frozen):
    def __init__(self, model: torch.nn.Module):
        super().__init__()
        self.model = model

    def _model_reason(self):
        return model_reason(self.model)

    def _shape(self):
        return model_shape(self.model)

    def _planner(self):
        return self.model

    def _weights(self, device):
        """-> (conv weights, conv biases, readout weights, readout biases), checked for a launch on `device`"""
        convs, lins = model_layers(self.model)
        w = [c.lin.weight for c in convs], [c.bias for c in convs], [li.weight for li in lins], [li.bias for li in lins]
        check_weights([t for ts in w for t in ts], device, f"{self.NAME}: the model's weights must be contiguous float32 on the batch's device")
        return w

    _masked_step = None             # forward-only `ExplainStep(model, apply_sigmoid=False)`, made on first use

    def _masked_forward(self, batch, node_mask, edge_mask):
        """The model's output [B, C] for `batch.x * node_mask` and `edge_mask` (mask semantics of `ExplainStep` without
        sigmoid): what every loop path of the Shapley family runs -- forward-only `ExplainStep` on GPU tensors, `torch_forward`
        on CPU tensors.  The caller holds `no_grad`; the result is overwritten by the next call on GPU tensors."""
        if not batch.x.is_cuda:
            return torch_forward(self.model, batch.x * node_mask, batch.edge_index, batch.batch, int(batch.num_graphs), edge_mask)
        if self._masked_step is None:
            from .explain import ExplainStep        # (explain.py imports this module)
            self._masked_step = ExplainStep(self.model, apply_sigmoid=False)
        return self._masked_step(batch, edge_mask, node_mask).out


def torch_forward(model, x, edge_index, batch_vec, B: int, edge_mask):
    """The model's masked forward in plain torch ops, for CPU tensors (the package's layers are HIP kernels and take GPU
    tensors only).  The loop paths use it when the batch lives on the CPU; nothing on a GPU ever runs it."""
    convs, lins = model_layers(model)
    N = x.shape[0]
    src, dst = edge_index[0], edge_index[1]
    keep = src != dst                                   # an explicit (i, i) edge is part of the unit self loop
    deg = torch.ones(N, dtype=x.dtype).scatter_add_(0, dst[keep], torch.ones(int(keep.sum()), dtype=x.dtype))
    dinv = deg.pow(-0.5)
    coef = (dinv[src] * dinv[dst] * edge_mask)[keep].unsqueeze(1)
    s, d = src[keep], dst[keep]
    h = x
    for c in convs:
        t = Fn.linear(h, c.lin.weight)
        y = (dinv * dinv).unsqueeze(1) * t
        # (index_select, not t[s]: the same values forward; its backward adds the rows serially in index order, where
        # the backward of t[s] adds them with atomics from several threads -- a gradient that differs in its last bits run to run)
        y = y.index_add(0, d, coef * t.index_select(0, s))
        h = Fn.leaky_relu(y + c.bias, SLOPE)
    idx = batch_vec.unsqueeze(1).expand_as(h)
    mx = h.new_zeros(B, h.shape[1]).scatter_reduce(0, idx, h, reduce="amax", include_self=False)
    cnt = torch.bincount(batch_vec, minlength=B).clamp_min(1).to(h.dtype).unsqueeze(1)
    z = torch.cat([mx, h.new_zeros(B, h.shape[1]).index_add(0, batch_vec, h) / cnt], 1)
    for li in lins[:-1]:
        z = Fn.leaky_relu(Fn.linear(z, li.weight, li.bias), SLOPE)
    z = Fn.linear(z, lins[-1].weight, lins[-1].bias)
    return z
