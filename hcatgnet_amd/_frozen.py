"""The host path the frozen-model classes share (`ExplainStep`, `ExplainFit`, `EnsemblePredict`, `ShapleySampling`, `IntegratedGradients`,
`EnsembleAttribution`: one graph per workgroup, all through `hcg_explain`): what a model must look like, the batch checks and their reason strings, the
library's shape query, and the argument block's graph and weight pointers.  Private: the classes are the interface.
"""
from __future__ import annotations

import ctypes
from typing import Optional

import torch

from . import _lib

MODEL_ATTRS = ("embedding_dim", "n_node_features", "n_convolutions", "readout_layers", "_n_classes", "conv1", "readout")
SLOPE = 0.01                       # nn.LeakyReLU() default (reference model/gcn.py:21, :63)

# mode -> (the kernel's name in a reason, its node limit, the label of a failed query)
_MODES = {_lib.HCG_EXPLAIN_GRAPHS: ("one-launch explain", 224, "hcg_explain (query)"),
          _lib.HCG_EXPLAIN_ENSEMBLE: ("one-launch ensemble", 224, "hcg_explain (ensemble query)"),
          _lib.HCG_EXPLAIN_SHAPLEY: ("on-chip Shapley", 184, "hcg_explain (shapley query)"),
          _lib.HCG_EXPLAIN_FIT: ("one-launch explainer fit", 224, "hcg_explain (fit query)"),
          _lib.HCG_EXPLAIN_INTEGRATED: ("one-launch integrated gradients", 224, "hcg_explain (integrated query)")}


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


def model_weights(model, device, who: str):
    """-> (conv weights, conv biases, readout weights, readout biases) of one model, checked for a launch on `device`"""
    convs, lins = model_layers(model)
    w = [c.lin.weight for c in convs], [c.bias for c in convs], [li.weight for li in lins], [li.bias for li in lins]
    check_weights([t for ts in w for t in ts], device, f"{who}: the model's weights must be contiguous float32 on the batch's device")
    return w


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
    """Fill the shape fields of `a` from `shape` (`model_shape`) and `batch` (checked by `batch_reason`, or None) plus
    `extra`, and ask the library: None when the kernel takes them (`a.workspace_bytes_needed` is set), else the limits."""
    a.mode, a.flags = mode, _lib.HCG_EXPLAIN_QUERY
    a.F, a.D, a.C, a.n_conv, a.R = shape
    a.N = a.E = a.B = a.max_nodes = a.max_edges = 0
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


def fill_graph(a, x, plan):
    p = _lib.ptr
    a.x, a.edge_index, a.graph_ptr, a.edge_ptr = p(x), p(plan.edge_index), p(plan.graph_ptr), p(plan.edge_ptr)
    a.status = p(plan.status)


def fill_weights(a, cW, cb, hW, hb):
    """Lists of tensors in layer order (one model's, or the ensemble's stacked [M, ...] ones)."""
    for slots, tensors in ((a.conv_W, cW), (a.conv_b, cb), (a.head_W, hW), (a.head_b, hb)):
        for i in range(len(slots)):
            slots[i] = _lib.ptr(tensors[i]) if i < len(tensors) else None
