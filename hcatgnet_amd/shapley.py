"""Shapley value sampling for a batch of graphs (the second algorithm of the reference's explain stage).

The reference explains `GCN_explain` through `torch_geometric.explain.Explainer` with two algorithms
(scripts_experiments/explain_gnn.py): GNNExplainer, served by `hcatgnet_amd.explain.ExplainStep`, and Captum's
`ShapleyValueSampling` with `node_mask_type='attributes'`, `edge_mask_type='object'`, baselines 0.  The features of a
graph with n nodes, e directed edges and F node features are its n*F node-feature entries and its e edges; for a random
permutation of them the features are switched on one at a time (a node entry takes its value of x instead of 0, an edge's
mask 1 instead of 0, mask semantics as `ExplainStep` without sigmoid) and every feature is credited with the change of the
chosen output column at its step.  The attribution is the mean over the permutations.

`ShapleySampling` runs that walk on chip (csrc/shapley.hip): one workgroup per (graph, permutation) keeps its graph in LDS
and evaluates the model after every step, with no launch in between.  No reference artefact pins Shapley values: parity
is against the fp64 oracle only.
"""
from __future__ import annotations

import ctypes
from typing import NamedTuple, Optional

import torch
import torch.nn.functional as Fn

from . import _frozen, _lib
from ._frozen import SLOPE
from .explain import ExplainStep

WORKSPACE_CAP_BYTES = 256 << 20    # the per-permutation rows of one launch
CUS = 256                          # compute units of an MI355X
LAUNCH_SECONDS = 1.0               # what one launch should stay near (the machines are shared)
EVAL_SECONDS = 60e-6               # one evaluation at the shape limits: an estimate (default_samples_per_launch)
MAX_WORKGROUPS_PER_CU = 4


class ShapleyResult(NamedTuple):
    node_attr: torch.Tensor      # [N, F]
    edge_attr: torch.Tensor      # [E], the batch's edge order
    out_full: torch.Tensor       # [B, C] the model's output with every feature on (= the plain forward)
    out_base: torch.Tensor       # [B, C] with every feature off


def _layout(batch, F: int):
    """-> (nodes per graph, edges per graph, graph_ptr, edge_ptr, segment start), int64 [B] / [B + 1] on the batch's
    device.  Graph g's segment of a permutation row starts at graph_ptr[g] * F + edge_ptr[g]."""
    B = int(batch.num_graphs)
    n = torch.bincount(batch.batch, minlength=B)
    e = torch.bincount(batch.batch[batch.edge_index[1]], minlength=B)
    gptr = torch.zeros(B + 1, dtype=torch.int64, device=n.device)
    eptr = torch.zeros(B + 1, dtype=torch.int64, device=n.device)
    gptr[1:] = n.cumsum(0)
    eptr[1:] = e.cumsum(0)
    return n, e, gptr, eptr, gptr[:-1] * F + eptr[:-1]


def draw_permutations(batch, F: int, n_samples: int, generator: Optional[torch.Generator] = None) -> torch.Tensor:
    """int32 [n_samples, N * F + E] on the batch's device: in every row, graph g's segment (start graph_ptr[g] * F +
    edge_ptr[g], length K_g = n_g * F + e_g) is a uniformly random permutation of 0 .. K_g - 1, drawn from `generator`
    (on the generator's device; None: the default generator of the batch's device) as the argsort of (graph id, key)."""
    n, e, _, _, seg = _layout(batch, F)
    dev = batch.x.device
    K = n * F + e
    total = int(K.sum())
    gid = torch.repeat_interleave(torch.arange(K.numel(), device=dev), K)
    start = seg[gid]
    gdev = generator.device if generator is not None else dev
    out = torch.empty(int(n_samples), total, dtype=torch.int32, device=dev)
    for p in range(int(n_samples)):
        key = torch.rand(total, generator=generator, device=gdev, dtype=torch.float64).to(dev)
        order = torch.argsort(gid.to(torch.float64) + key)
        out[p] = (order - start).to(torch.int32)
    return out


def _torch_forward(model, x, edge_index, batch_vec, B: int, edge_mask):
    """The model's masked forward in plain torch ops, for CPU tensors (the package's layers are HIP kernels and take GPU
    tensors only).  The loop path uses it when the batch lives on the CPU; nothing on a GPU ever runs it."""
    convs, lins = _frozen.model_layers(model)
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


class ShapleySampling:
    """Shapley value sampling of a frozen model for a whole batch of graphs.

        sv = ShapleySampling(model)
        r = sv(batch, n_samples=25, permutations=None, generator=None, class_index=0, samples_per_launch=None)
        # ShapleyResult(node_attr [N, F], edge_attr [E], out_full [B, C], out_base [B, C])

    Captum's `ShapleyValueSampling` with baselines 0 and one feature per step: for permutation pi of graph g's
    K = n*F + e features (index j < n*F: node entry (j // F, j % F); j >= n*F: local edge j - n*F), v_0 is the model's
    output with everything off, v_k the output with pi_1 .. pi_k on, and feature pi_k gets v_k[c] - v_(k-1)[c] for
    c = `class_index`.  The attribution is the mean over the permutations, summed in the order p = 0, 1, ...  A node
    entry whose x is exactly 0 and an explicit (i, i) edge cannot change the output: their attribution is exactly 0 and
    the kernel spends no evaluation on them.

    `permutations`: int32 [P, N*F + E] (`draw_permutations` states the layout; dtype and shape are checked, the contents
    are trusted).  None: `n_samples` rows are drawn from `generator`.  With `permutations` given, `n_samples` is ignored.

    The permutations are split into launches of `samples_per_launch` (None: `default_samples_per_launch`); the result
    is bitwise independent of that split, of the run and of the rest of the batch.  The weights are read, never written;
    no mask stays attached to the model.  `batch` needs the collate metadata `ExplainStep` needs.  Buffers are allocated
    for the largest call seen and reused; the returned tensors are views of them, overwritten by the next call.

    When `reason(batch)` is not None (shape outside the kernel, CPU tensors, `use_fused` off) the same call runs the
    batch-synchronous loop `loop`: step k switches on the k-th feature of every graph's permutation at once and runs one
    masked forward of the whole batch -- forward-only `ExplainStep` on GPU tensors (its one-launch kernel where that
    applies, else `set_masks` + the model under `no_grad`), plain torch ops on CPU tensors.  `last_path` says which one
    ran ("fused" / "loop")."""

    def __init__(self, model: torch.nn.Module):
        self.model = model
        self.last_path: Optional[str] = None
        self._cap = None            # (N * F + E, B, workspace bytes) capacity of the buffers
        self._bufs = None
        self._args = _lib.ExplainArgs()
        self._step = ExplainStep(model, apply_sigmoid=False)

    # ------------------------------------------------------------------ support check (host only, no sync)
    def _shape_args(self, a, batch, perm_count: int = 1) -> Optional[str]:
        m = self.model
        why = _frozen.model_reason(m)
        if why is None and batch is not None:
            why = "the batch is on the CPU" if not batch.x.is_cuda else _frozen.batch_reason(batch, int(m.n_node_features), "model")
        return why or _frozen.query(a, _lib.HCG_EXPLAIN_SHAPLEY, _frozen.model_shape(m), batch, perm_count=int(perm_count),
                                    edge_mask=None, node_mask=None, target=None, dout=None)

    def reason(self, batch=None) -> Optional[str]:
        """None when this model (and `batch`) takes the on-chip kernel, else why not.  Host metadata only."""
        return self._shape_args(_lib.ExplainArgs(), batch)

    def lds_bytes(self, batch) -> Optional[int]:
        """Dynamic LDS of one workgroup of the kernel for this batch, as the library's query reports it; None when the
        batch does not take the kernel."""
        a = _lib.ExplainArgs()
        return int(a.lds_bytes) if self._shape_args(a, batch) is None else None

    @staticmethod
    def default_samples_per_launch(n_perm: int, num_graphs: int, row: int, max_steps: int = 0) -> int:
        """Permutations of one launch: as many as keep its workspace (4 * row bytes each) under `WORKSPACE_CAP_BYTES` and
        its run time near `LAUNCH_SECONDS`, at least 1.  `max_steps` = max_nodes * F + max_edges bounds the evaluations of
        one workgroup (every step evaluated: dense features); at `EVAL_SECONDS` each, a CU gets as many workgroups as fit
        the time, at least one.  `EVAL_SECONDS` is an ESTIMATE: profiles/shapley_bench.json has about 15-20 us per
        evaluation at two conv layers and 122-node graphs (36 ms per launch of 535 workgroups of about 860 evaluations),
        extrapolated to the 184-node, four-layer limit; nobody has timed a launch at the limit shapes."""
        by_ws = WORKSPACE_CAP_BYTES // max(4 * int(row), 1)
        per_cu = max(1, int(LAUNCH_SECONDS / (max(int(max_steps), 1) * EVAL_SECONDS)))
        by_wg = min(per_cu, MAX_WORKGROUPS_PER_CU) * CUS // max(int(num_graphs), 1)
        return max(1, min(int(n_perm), by_ws, by_wg, 65535))

    # ------------------------------------------------------------------ buffers
    def _buffers(self, row, B, C, ws_bytes, dev):
        cap = self._cap
        if cap is None or row > cap[0] or B > cap[1] or ws_bytes > cap[2] or self._bufs["out"].device != dev:
            cap = (max(row, cap[0] if cap else 0), max(B, cap[1] if cap else 0), max(ws_bytes, cap[2] if cap else 0))
            f32 = dict(dtype=torch.float32, device=dev)
            self._bufs = dict(acc=torch.zeros(max(cap[0], 1), **f32), out=torch.zeros(max(cap[1], 1), C, **f32),
                              base=torch.zeros(max(cap[1], 1), C, **f32),
                              ws=torch.empty(max(cap[2], 256), dtype=torch.uint8, device=dev))
            self._cap = cap
        return self._bufs

    def _permutations(self, batch, F, n_samples, permutations, generator):
        row = int(batch.x.shape[0]) * F + int(batch.edge_index.shape[1])
        if permutations is None:
            if int(n_samples) < 1:
                raise ValueError(f"n_samples must be at least 1; got {n_samples}")
            return draw_permutations(batch, F, int(n_samples), generator)
        t = permutations
        if not torch.is_tensor(t) or t.dtype != torch.int32 or t.dim() != 2 or t.shape[0] < 1 or t.shape[1] != row:
            raise ValueError(f"permutations must be an int32 tensor of shape [P >= 1, N * F + E = {row}]; got "
                             f"{getattr(t, 'dtype', type(t))} {tuple(getattr(t, 'shape', ()))}")
        if t.device != batch.x.device:
            raise ValueError(f"permutations are on {t.device}, the batch on {batch.x.device}")
        return t.contiguous()

    # ------------------------------------------------------------------ the call
    def __call__(self, batch, n_samples: int = 25, permutations=None, generator=None, class_index: int = 0,
                 samples_per_launch: Optional[int] = None) -> ShapleyResult:
        a = self._args
        why = self._shape_args(a, batch)
        if why is not None:
            return self.loop(batch, n_samples, permutations, generator, class_index)
        m = self.model
        x = _frozen.batch_x(batch)
        N, F, E, B, C = a.N, a.F, a.E, a.B, a.C
        if not 0 <= int(class_index) < C:
            raise ValueError(f"class_index must lie in 0 .. {C - 1}; got {class_index}")
        perm = self._permutations(batch, F, n_samples, permutations, generator)
        P, row = int(perm.shape[0]), N * F + E
        spl = self.default_samples_per_launch(P, B, row, a.max_nodes * F + a.max_edges) if samples_per_launch is None else int(samples_per_launch)
        if not 1 <= spl <= 65535:
            raise ValueError(f"samples_per_launch must lie in 1 .. 65535; got {samples_per_launch}")
        spl = min(spl, P)
        self._shape_args(a, batch, spl)                     # the workspace of a launch of `spl` permutations
        plan = m._plan_for(batch, x, batch.edge_index, batch.batch, None)
        bufs = self._buffers(row, B, C, int(a.workspace_bytes_needed), x.device)
        p = _lib.ptr
        a.flags = 0
        _frozen.fill_graph(a, x, plan)
        _frozen.fill_weights(a, *_frozen.model_weights(m, x.device, "ShapleySampling"))
        a.out, a.out_base, a.shap_acc, a.perm = p(bufs["out"]), p(bufs["base"]), p(bufs["acc"]), p(perm)
        a.workspace, a.workspace_bytes = p(bufs["ws"]), bufs["ws"].numel()
        a.slope, a.n_perm, a.class_index = SLOPE, P, int(class_index)
        lib, stream = _lib.load(), _lib.stream_ptr()
        for first in range(0, P, spl):
            a.perm_first, a.perm_count = first, min(spl, P - first)
            _lib.check(lib.hcg_explain(ctypes.addressof(a), stream), "hcg_explain (shapley)")
        self.last_path = "fused"
        acc = bufs["acc"]
        return ShapleyResult(acc[:N * F].view(N, F), acc[N * F:row], bufs["out"][:B], bufs["base"][:B])

    # ------------------------------------------------------------------ the existing path (any shape): one forward per step
    def _forward(self, batch, node_mask, edge_mask):
        if not batch.x.is_cuda:
            return _torch_forward(self.model, batch.x * node_mask, batch.edge_index, batch.batch, int(batch.num_graphs), edge_mask)
        return self._step(batch, edge_mask, node_mask).out

    def loop(self, batch, n_samples: int = 25, permutations=None, generator=None, class_index: int = 0) -> ShapleyResult:
        """The batch-synchronous loop (see the class docstring), whatever `reason(batch)` says."""
        x = batch.x
        (N, F), E, B = x.shape, int(batch.edge_index.shape[1]), int(batch.num_graphs)
        perm = self._permutations(batch, F, n_samples, permutations, generator).to(torch.int64)
        P, dev = int(perm.shape[0]), x.device
        n, e, gptr, eptr, seg = _layout(batch, F)
        nF, K = n * F, n * F + e
        kmax = int(K.max()) if B > 0 else 0
        src, dst = batch.edge_index[0], batch.edge_index[1]
        # what cannot change the output: its difference is exactly 0 by definition
        dead = torch.cat([(x == 0).reshape(-1), src == dst])
        garange = torch.arange(B, device=dev)
        acc = torch.zeros(N * F + E, dtype=torch.float32, device=dev)
        out_full = out_base = None
        with torch.no_grad():
            for p in range(P):
                nm = torch.zeros(N, F, dtype=torch.float32, device=dev)
                em = torch.zeros(E, dtype=torch.float32, device=dev)
                phi = torch.zeros(N * F + E, dtype=torch.float32, device=dev)
                out = self._forward(batch, nm, em).reshape(B, -1).clone()
                if p == 0:
                    out_base = out
                vprev = out[:, class_index].clone()
                for k in range(kmax):
                    act = garange[K > k]                                  # graphs whose walk is not finished
                    j = perm[p, seg[act] + k]
                    is_node = j < nF[act]
                    slot = torch.where(is_node, gptr[act] * F + j, N * F + eptr[act] + j - nF[act])
                    nm.view(-1)[slot[is_node]] = 1.0
                    em[slot[~is_node] - N * F] = 1.0
                    out = self._forward(batch, nm, em).reshape(B, -1).clone()
                    v = out[:, class_index]
                    phi[slot] = torch.where(dead[slot], torch.zeros_like(v[act]), v[act] - vprev[act])
                    vprev = v.clone()
                if p == 0:
                    out_full = out
                acc = acc + phi
        acc = acc / float(P)
        self.last_path = "loop"
        return ShapleyResult(acc[:N * F].view(N, F), acc[N * F:], out_full, out_base)
