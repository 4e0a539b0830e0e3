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


class FrozenEnsemble(_frozen.Frozen):
    """M models of one architecture, their weights stacked once into contiguous [M, ...] buffers (`stacked`: a snapshot):
    what `EnsemblePredict`, `attribution.EnsembleAttribution` and the classes of ensemble_shapley.py share; the last two kinds
    run the models in chunks (`_model_chunks`) with one moments launch per chunk (`_moments_block`)."""
    WHAT = "models"

    def __init__(self, models: Sequence[torch.nn.Module]):
        super().__init__()
        self.models: List[torch.nn.Module] = list(models)
        if not self.models:
            raise ValueError(f"{self.NAME} needs at least one model")
        for k, m in enumerate(self.models):
            if any(not hasattr(m, a) for a in _frozen.MODEL_ATTRS):
                raise ValueError(f"model {k} is not a hcatgnet_amd GCN model")
        sig = [_frozen.model_shape(m) for m in self.models]
        for k, s in enumerate(sig):
            if s != sig[0]:
                raise ValueError(f"model {k} has (features, embedding_dim, classes, conv layers, readout layers) = {s}, "
                                 f"model 0 has {sig[0]}")
        self.F, self.D, self.C, self.n_conv, self.R = sig[0]
        self.stacked = stack_weights([m.state_dict() for m in self.models])

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

    def _model_reason(self):
        return None if all(bool(getattr(m, "use_fused", True)) for m in self.models) else "fused kernels disabled on a model"

    def _shape(self):
        return self.F, self.D, self.C, self.n_conv, self.R

    def _planner(self):
        return self.models[0]

    def _weights(self, device):
        """-> the stacked (conv weights, conv biases, readout weights, readout biases), checked for a launch on `device`"""
        S = self.stacked
        _frozen.check_weights(S.values(), device, f"{self.NAME}: the stacked weights must be on the batch's device "
                              "(construct the ensemble from models on that device)")
        return [[S[n] for n in names] for names in weight_names(self.n_conv, self.R)]

    # ------------------------------------------------------------------ the model axis of the attribution classes
    def _moments_block(self, *arrays):
        """The argument block of the moments launches (`HCG_EXPLAIN_MOMENTS`) over one or two per-model arrays
        [models, length]: `arrays` = (mean, m2, std, length) each, pool views."""
        q, front = _lib.ExplainArgs(), _frozen.front
        q.mode = _lib.HCG_EXPLAIN_MOMENTS
        for k, (mean, m2, std, length) in enumerate(arrays):
            for name, value in (("mom_mean", front(mean)), ("mom_m2", front(m2)), ("mom_std", front(std)), ("mom_len", length)):
                setattr(q, f"{name}{k}", value)
        q.mom_total = len(self.models)
        return q

    def _model_chunks(self, a, weights, per_launch: int, per_model: bool, q):
        """The models in chunks of `per_launch`.  Per chunk: the block `a` gets the chunk's weights (`fill_weights` from its
        first model) and `n_models`; (first model, models, first row) is yielded -- the row of the per-model arrays the
        chunk writes from: its first model, or 0 when only one chunk's rows exist (`per_model` False); the caller sets the
        chunk's addresses, `q.mom_values0` (`q.mom_values1`) among them, and enqueues its launches; then the moments launch
        `q` (`_moments_block`) runs over the chunk."""
        M = len(self.models)
        lib, stream = _lib.load(), _lib.stream_ptr()
        for m0 in range(0, M, per_launch):
            count = min(per_launch, M - m0)
            _frozen.fill_weights(a, weights, m0)
            a.n_models = count
            yield m0, count, (m0 if per_model else 0)
            q.mom_first, q.mom_count = m0, count
            _lib.check(lib.hcg_explain(ctypes.addressof(q), stream), "hcg_explain (moments)")


class EnsembleResult(NamedTuple):
    out: torch.Tensor                 # [M, B, C]
    emb: Optional[torch.Tensor]       # [M, B, 2D] ([max, mean] pooling, max first); None unless asked for
    mean: Optional[torch.Tensor]      # [B, C] = out.mean(0)
    std: Optional[torch.Tensor]       # [B, C] = out.std(0, unbiased=False)


class EnsemblePredict(FrozenEnsemble):
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

    KERNEL, NAME, REFUSES_CPU = _lib.HCG_EXPLAIN_ENSEMBLE, "EnsemblePredict", False

    def __init__(self, models: Sequence[torch.nn.Module], models_per_group: Optional[int] = None):
        super().__init__(models)
        if models_per_group is not None and not 1 <= int(models_per_group) <= len(self.models):
            raise ValueError(f"models_per_group must lie in 1 .. {len(self.models)}; got {models_per_group}")
        self.models_per_group = None if models_per_group is None else int(models_per_group)

    def _shape_args(self, a, batch) -> Optional[str]:
        M = len(self.models)
        mpg = self.models_per_group or (default_models_per_group(M, int(batch.num_graphs)) if batch is not None else 1)
        return super()._shape_args(a, batch, n_models=M, models_per_group=mpg)

    # ------------------------------------------------------------------ the call
    def __call__(self, batch, return_emb: bool = False, stats: bool = True) -> EnsembleResult:
        a = self._args
        why = self._shape_args(a, batch)
        if why is not None:
            return self._loop(batch, return_emb, stats)
        x = _frozen.batch_x(batch)
        M, B, C, D2 = len(self.models), a.B, self.C, 2 * self.D
        take, dev = self._bufs.take, x.device
        out = take("out", (M, B, C), dev)
        emb = take("emb", (M, B, D2), dev) if return_emb else None
        self._fill(a, 0, batch, x, self._weights(dev))
        a.out, a.emb = _frozen.front(out), _frozen.front(emb)
        _lib.check(_lib.load().hcg_explain(ctypes.addressof(a), _lib.stream_ptr()), "hcg_explain (ensemble)")
        self.last_path = "fused"
        mean = std = None
        if stats:
            mean, std = take("mean", (B, C), dev), take("std", (B, C), dev)
            torch.mean(out, dim=0, out=mean)
            torch.std(out, dim=0, unbiased=False, out=std)
        return EnsembleResult(out, emb, mean, std)

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
