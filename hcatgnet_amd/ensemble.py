"""Ensemble prediction: M trained models of one architecture predict the same batch of graphs in ONE launch.

The reference reloads the 90 models of its nested cross-validation and predicts the same unseen set with each of them,
one model and one graph at a time (scripts_experiments/predict_test.py:19-103).  The graphs are shared and only the
weights differ, so `EnsemblePredict` stacks the models' weights along a leading model axis once and hands the batch to
csrc/ensemble.hip: one workgroup per (graph, group of models) builds gcn_norm and the row list of its graph once and runs
its models on it, weights frozen, forward only.
"""
from __future__ import annotations

import ctypes
from typing import Dict, List, NamedTuple, Optional, Sequence

import torch

from . import _frozen, _lib

TARGET_WORKGROUPS = 512       # 2 per CU of an MI355X: what the default `models_per_group` keeps when the batch allows it
MAX_DEFAULT_GROUP = 4         # profiles/ensemble_bench.json: the sweep's best or within 3 % of it in every case; 8 loses 14 %


def default_models_per_group(n_models: int, num_graphs: int) -> int:
    """The largest group (it need not divide M) that still leaves `TARGET_WORKGROUPS` workgroups, between 1 and
    min(M, `MAX_DEFAULT_GROUP`).  The cap follows the recorded sweep (tools/bench_ensemble.py): at 90 models on 52 graphs
    groups of 1 / 2 / 4 / 8 / 90 took 626 / 628 / 642 / 733 / 3358 us, on 535 graphs 6.46 / 6.05 / 5.84 / 5.77 / 8.21 ms; at
    9 models on 535 graphs 691 / 656 / 629 / 733 us (1 / 2 / 4 / 8).  The build a larger group saves is small beside its
    models' work, and a large group leaves CUs idle at the launch's tail."""
    return max(1, min(int(n_models), MAX_DEFAULT_GROUP, (int(n_models) * int(num_graphs)) // TARGET_WORKGROUPS))


def stack_weights(state_dicts: Sequence[Dict[str, torch.Tensor]]) -> Dict[str, torch.Tensor]:
    """The models' tensors stacked along a new leading model axis: name -> contiguous float32 [M, ...], row k = model k.
    Works on CPU and GPU tensors alike.  `ValueError` when the state-dicts differ in their names (other depths) or in a
    tensor's shape."""
    sds = list(state_dicts)
    if not sds:
        raise ValueError("stack_weights needs at least one state-dict")
    names = [k for k, v in sds[0].items() if torch.is_tensor(v)]
    out = {}
    for k, sd in enumerate(sds[1:], 1):
        other = [n for n, v in sd.items() if torch.is_tensor(v)]
        if sorted(other) != sorted(names):
            diff = sorted(set(other) ^ set(names))
            raise ValueError(f"model {k} has other tensors than model 0 (other depths?): {diff[:6]}")
    for n in names:
        shape = tuple(sds[0][n].shape)
        for k, sd in enumerate(sds):
            if tuple(sd[n].shape) != shape:
                raise ValueError(f"{n}: model {k} has shape {tuple(sd[n].shape)}, model 0 has {shape}")
        out[n] = torch.stack([sd[n].detach().to(torch.float32) for sd in sds]).contiguous()
    return out


def weight_names(n_conv: int, n_read: int):
    """-> (conv weights, conv biases, readout weights, readout biases): the state-dict names in layer order."""
    cw = ["conv1.lin.weight"] + [f"conv_layers.{i}.lin.weight" for i in range(n_conv - 1)]
    cb = ["conv1.bias"] + [f"conv_layers.{i}.bias" for i in range(n_conv - 1)]
    hw = [f"readout.{i}.0.weight" for i in range(n_read - 1)] + [f"readout.{n_read - 1}.weight"]
    hb = [f"readout.{i}.0.bias" for i in range(n_read - 1)] + [f"readout.{n_read - 1}.bias"]
    return cw, cb, hw, hb


class EnsembleResult(NamedTuple):
    out: torch.Tensor                 # [M, B, C]
    emb: Optional[torch.Tensor]       # [M, B, 2D] ([max, mean] pooling, max first); None unless asked for
    mean: Optional[torch.Tensor]      # [B, C] = out.mean(0)
    std: Optional[torch.Tensor]       # [B, C] = out.std(0, unbiased=False)


class EnsemblePredict:
    """Predictions of M frozen models for a whole batch of graphs, one launch per call.

        ens = EnsemblePredict(models, models_per_group=None)
        r = ens(batch, return_emb=False)     # EnsembleResult(out [M, B, C], emb [M, B, 2D] | None, mean [B, C], std [B, C])

    `models`: hcatgnet_amd GCNs with the same node features, embedding_dim, classes and depths (`ValueError` otherwise).
    Their weights are stacked into contiguous [M, ...] buffers at construction: a SNAPSHOT -- later changes of a model do
    not show until `refresh()` re-stacks them in place (a captured call then replays with the new values).
    `mean` / `std` are taken over the model axis of `out` with torch ops; `std` is the population form (ddof = 0:
    `out.std(0, unbiased=False)`), so a one-model ensemble has std 0, not NaN.  `stats=False` leaves them None.

    `models_per_group`: the models one workgroup runs on its graph (None: `default_models_per_group` of each batch).  It
    changes the launch's shape, never a value: the result for (model, graph) is bitwise independent of M, of the group
    size and of the rest of the batch.

    `batch` needs the collate metadata `FusedTrainStep` needs (`max_nodes`, `max_edges`, grouped edges).  Buffers are
    allocated for the largest batch seen and reused: in steady state a call allocates nothing and can be captured with
    `torch.cuda.graph`, and the returned tensors are views of those buffers, overwritten by the next call (clone what must
    outlive it).  When `reason(batch)` is not None the call runs `model_k(batch, True)` for every k -- on the models'
    CURRENT weights -- and returns the same fields; `last_path` says which one ran ("fused" / "loop")."""

    def __init__(self, models: Sequence[torch.nn.Module], models_per_group: Optional[int] = None):
        self.models: List[torch.nn.Module] = list(models)
        if not self.models:
            raise ValueError("EnsemblePredict needs at least one model")
        for k, m in enumerate(self.models):
            if any(not hasattr(m, a) for a in _frozen.MODEL_ATTRS):
                raise ValueError(f"model {k} is not a hcatgnet_amd GCN model")
        sig = [_frozen.model_shape(m) for m in self.models]
        for k, s in enumerate(sig):
            if s != sig[0]:
                raise ValueError(f"model {k} has (features, embedding_dim, classes, conv layers, readout layers) = {s}, "
                                 f"model 0 has {sig[0]}")
        self.F, self.D, self.C, self.n_conv, self.R = sig[0]
        if models_per_group is not None and not 1 <= int(models_per_group) <= len(self.models):
            raise ValueError(f"models_per_group must lie in 1 .. {len(self.models)}; got {models_per_group}")
        self.models_per_group = None if models_per_group is None else int(models_per_group)
        self.stacked = stack_weights([m.state_dict() for m in self.models])
        self.last_path: Optional[str] = None
        self._cap = None            # (B,) capacity of the buffers
        self._bufs = None
        self._args = _lib.ExplainArgs()

    @property
    def n_models(self) -> int:
        return len(self.models)

    def refresh(self):
        """Re-stack the models' current weights into the same buffers (in place: pointers, and captured calls, stay valid)."""
        with torch.no_grad():
            for k, m in enumerate(self.models):
                for name, t in m.state_dict().items():
                    if name in self.stacked:
                        self.stacked[name][k].copy_(t.detach())
        return self

    # ------------------------------------------------------------------ support check (host only, no sync)
    def _shape_args(self, a, batch) -> Optional[str]:
        if not all(bool(getattr(m, "use_fused", True)) for m in self.models):
            return "fused kernels disabled on a model"
        why = _frozen.batch_reason(batch, self.F, "models") if batch is not None else None
        if why is not None:
            return why
        M = len(self.models)
        mpg = self.models_per_group or (default_models_per_group(M, int(batch.num_graphs)) if batch is not None else 1)
        return _frozen.query(a, _lib.HCG_EXPLAIN_ENSEMBLE, (self.F, self.D, self.C, self.n_conv, self.R), batch,
                             n_models=M, models_per_group=mpg)

    def reason(self, batch=None) -> Optional[str]:
        """None when these models (and `batch`) take the one-launch kernel, else why not.  Host metadata only."""
        return self._shape_args(_lib.ExplainArgs(), batch)

    # ------------------------------------------------------------------ buffers
    def _buffers(self, B, dev):
        """Flat buffers of the largest batch seen; a call's [M, B, ...] results are contiguous views of their fronts."""
        if self._cap is None or B > self._cap or self._bufs["out"].device != dev:
            cap = max(B, self._cap or 0, 1)
            M = len(self.models)
            f32 = dict(dtype=torch.float32, device=dev)
            self._bufs = dict(out=torch.zeros(M * cap * self.C, **f32), emb=torch.zeros(M * cap * 2 * self.D, **f32),
                              mean=torch.zeros(cap * self.C, **f32), std=torch.zeros(cap * self.C, **f32))
            self._cap = cap
        M, C, D2 = len(self.models), self.C, 2 * self.D
        b = self._bufs
        return (b["out"][:M * B * C].view(M, B, C), b["emb"][:M * B * D2].view(M, B, D2), b["mean"][:B * C].view(B, C),
                b["std"][:B * C].view(B, C))

    # ------------------------------------------------------------------ the call
    def __call__(self, batch, return_emb: bool = False, stats: bool = True) -> EnsembleResult:
        a = self._args
        why = self._shape_args(a, batch)
        if why is not None:
            return self._loop(batch, return_emb, stats)
        x = _frozen.batch_x(batch)
        B = a.B
        S = self.stacked
        _frozen.check_weights(S.values(), x.device, "EnsemblePredict: the stacked weights must be on the batch's device "
                              "(construct the ensemble from models on that device)")
        plan = self.models[0]._plan_for(batch, x, batch.edge_index, batch.batch, None)
        out, emb, mean, std = self._buffers(B, x.device)
        p = _lib.ptr
        a.flags = 0
        _frozen.fill_graph(a, x, plan)
        _frozen.fill_weights(a, *([S[n] for n in names] for names in weight_names(self.n_conv, self.R)))
        a.edge_mask = a.node_mask = a.target = a.dout = None
        a.out, a.emb = p(out), (p(emb) if return_emb else None)
        a.slope = _frozen.SLOPE
        _lib.check(_lib.load().hcg_explain(ctypes.addressof(a), _lib.stream_ptr()), "hcg_explain (ensemble)")
        self.last_path = "fused"
        if stats:
            torch.mean(out, dim=0, out=mean)
            torch.std(out, dim=0, unbiased=False, out=std)
        return EnsembleResult(out, emb if return_emb else None, mean if stats else None, std if stats else None)

    # ------------------------------------------------------------------ the existing path (any shape), model by model
    def _loop(self, batch, return_emb, stats) -> EnsembleResult:
        outs, embs = [], []
        with torch.no_grad():
            for m in self.models:
                o, e = m(batch, True)
                outs.append(o.reshape(batch.num_graphs, -1))
                embs.append(e)
        out = torch.stack(outs)
        self.last_path = "loop"
        mean, std = (out.mean(0), out.std(0, unbiased=False)) if stats else (None, None)
        return EnsembleResult(out, torch.stack(embs) if return_emb else None, mean, std)
