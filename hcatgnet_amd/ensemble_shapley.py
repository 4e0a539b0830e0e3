"""The Shapley family for an ENSEMBLE of models: Shapley value sampling, subset values and deletion / insertion curves of M
frozen models of one architecture, the model a grid axis of the single-model kernels (csrc/shapley.hip).

The reference's product is the ensemble -- the 90 models of its nested cross-validation predict together
(`EnsemblePredict`) -- and `EnsembleAttribution` explains that joint prediction with integrated gradients.  Its other
explain algorithm, Shapley value sampling, and everything built on it (`SubsetValues`, `AttributionCurves`) took one model.
Shapley values are linear in the output, so the Shapley values of the ensemble's mean prediction are the mean over the
models of their Shapley values under the same permutations; and the deletion / insertion curve of the mean output needs
every subset evaluated by every model.  `EnsembleShapley`, `EnsembleSubsetValues` and `EnsembleCurves` do both in launches of
(graph, permutation or job, model) workgroups: the layout, the permutations, the job list and the bit words are built once
per call, the moments over the models are taken on the device (`HCG_EXPLAIN_MOMENTS`), and entry [m] of every per-model
array is bit for bit what the single-model class returns for `models[m]`.

Not done: a loop over a group of models inside one workgroup (`EnsemblePredict`'s `models_per_group`, which builds the graph
once per group), ensemble coalition values and an ensemble greedy order (its pick needs a reduction over the models inside
a round).
"""
from __future__ import annotations

import ctypes
from typing import NamedTuple, Optional, Sequence

import torch

from . import _frozen, _groups, _lib
from .attribution import LAUNCH_BUDGET_BYTES, EnsembleAttribution  # noqa: F401  (LAUNCH_BUDGET_BYTES: importable from here as before)
from .ensemble import FrozenEnsemble
from .shapley import CoalitionValues, ShapleySampling
from .subsets import MAX_SUBSET_GROUPS, AttributionCurves, SubsetValues


class EnsembleShapleyResult(NamedTuple):
    """A grouped `EnsembleShapley` call"""
    group_mean: torch.Tensor             # [G] mean over the models of their group attributions
    group_std: torch.Tensor              # [G] population standard deviation over the models
    group_ptr: torch.Tensor              # [B + 1] int64
    node_mean: torch.Tensor              # [N, F] every member carries its group's value, the background 0
    node_std: torch.Tensor               # [N, F]
    edge_mean: torch.Tensor              # [E]
    edge_std: torch.Tensor               # [E]
    out_full: torch.Tensor               # [M, B, C] every model's output with everything on
    out_base: torch.Tensor               # [M, B, C] with the background only
    group_attr: Optional[torch.Tensor]   # [M, G] the per-model attributions; None unless asked for


class EnsembleFeatureShapleyResult(NamedTuple):
    """An ungrouped `EnsembleShapley` call"""
    node_mean: torch.Tensor              # [N, F]
    node_std: torch.Tensor               # [N, F]
    edge_mean: torch.Tensor              # [E], the batch's edge order
    edge_std: torch.Tensor               # [E]
    out_full: torch.Tensor               # [M, B, C] everything on
    out_base: torch.Tensor               # [M, B, C] everything off
    node_attr: Optional[torch.Tensor]    # [M, N, F]; None unless asked for
    edge_attr: Optional[torch.Tensor]    # [M, E]


class EnsembleSubsetResult(NamedTuple):
    mean: torch.Tensor                   # [S, B, C] mean over the models of values[:, s, g]
    std: torch.Tensor                    # [S, B, C] population standard deviation
    group_ptr: torch.Tensor              # [B + 1] int64
    out_full: torch.Tensor               # [M, B, C] every group on
    out_base: torch.Tensor               # [M, B, C] the background only
    values: Optional[torch.Tensor]       # [M, S, B, C]; None unless asked for


class EnsembleCurveResult(NamedTuple):
    insertion: torch.Tensor              # [Pn, C] the ensemble's MEAN output; points as `CurveResult`
    deletion: torch.Tensor               # [Pn, C]
    k: torch.Tensor                      # [Pn] int64
    curve_ptr: torch.Tensor              # [B + 1] int64
    group_ptr: torch.Tensor              # [B + 1] int64
    insertion_auc: torch.Tensor          # [B] of the mean curve
    deletion_auc: torch.Tensor           # [B]
    out_full: torch.Tensor               # [B, C] the mean output with everything on
    out_base: torch.Tensor               # [B, C] with the background only
    insertion_std: torch.Tensor          # [Pn, C] population standard deviation over the models at every point
    deletion_std: torch.Tensor           # [Pn, C]


def _models_per_launch(value, M: int, workspace_bytes: int, entries: int) -> int:
    """`models_per_launch` of a call (checked by the caller), or `EnsembleAttribution.default_models_per_launch`'s rule"""
    if value is not None:
        return min(int(value), M)
    return EnsembleAttribution.default_models_per_launch(M, workspace_bytes, entries)


class EnsembleShapley(FrozenEnsemble):
    """Shapley value sampling of M frozen models of one architecture for a whole batch of graphs: every (graph, permutation,
    model) triple is one workgroup, and the mean and the standard deviation over the models are taken on the device.

        es = EnsembleShapley(models)
        r = es(batch, n_samples=25, permutations=None, generator=None, class_index=0, node_group=None, edge_group=None,
               group_permutations=None, per_model=False, models_per_launch=None, samples_per_launch=None)
        # grouped:   EnsembleShapleyResult(group_mean [G], group_std [G], group_ptr, node_mean, node_std, edge_mean, edge_std,
        #                                  out_full [M, B, C], out_base [M, B, C], group_attr [M, G] | None)
        # ungrouped: EnsembleFeatureShapleyResult(node_mean [N, F], node_std, edge_mean [E], edge_std, out_full, out_base,
        #                                         node_attr [M, N, F] | None, edge_attr [M, E] | None)
        es.refresh(); es.reason(batch); es.last_path

    `models` are checked and snapshotted as `EnsemblePredict` does it (`refresh()` re-stacks changed weights in place).
    Players, their checks and errors and the drawing of the permutations are `ShapleySampling`'s; ONE set of permutations
    serves all models.  Shapley values are linear in the output, so the means ARE the sampled Shapley values of the
    ensemble's mean prediction; the standard deviations (population form) say where the models disagree.  Entry [m] of
    `group_attr` / `node_attr` / `edge_attr` / `out_full` / `out_base` is bit for bit what `ShapleySampling(models[m])`
    returns for the same permutations, and every returned value is bitwise independent of `models_per_launch`, of
    `samples_per_launch`, of the other models and of the rest of the batch.  The moments are Welford's recurrence in
    float32 over the models in ascending order (`HCG_EXPLAIN_MOMENTS`, one launch per chunk of models): a player that gets 0
    in every model has mean and std exactly 0, and a one-model ensemble has the model's values as mean and std exactly 0.

    The models run in chunks of `models_per_launch` (None: `EnsembleAttribution.default_models_per_launch` -- a model's
    workspace slice plus its outputs under `LAUNCH_BUDGET_BYTES`), inside a chunk the permutations in launches of
    `samples_per_launch` (None: `ShapleySampling.default_samples_per_launch` with graphs x models of the chunk as the
    graph count).  With `per_model=False` only one chunk's per-model accumulators exist.  Buffers grow to the largest call
    and are reused; the returned tensors are views of them (the gathered node / edge moments are new), overwritten by the
    next call.

    When `reason(batch)` is not None (shape outside the kernel, CPU tensors, `use_fused` off on any model) the same call runs
    `loop`: `ShapleySampling(model_k).loop` per model on the models' CURRENT weights with the shared permutations, the moments
    with torch ops (`mean(0)`, `std(0, unbiased=False)`).  `last_path` says which one ran ("fused" / "loop")."""

    KERNEL, NAME = _lib.HCG_EXPLAIN_SHAPLEY, "EnsembleShapley"

    def __init__(self, models: Sequence[torch.nn.Module]):
        super().__init__(models)
        self._singles = [ShapleySampling(m) for m in self.models]          # the loop path's workers

    def _shape_args(self, a, batch, **extra) -> Optional[str]:
        """None when the kernel takes these models and `batch`; `a` then holds the shapes and the ONE-model workspace bytes"""
        return super()._shape_args(a, batch, n_models=1, **extra)

    # ------------------------------------------------------------------ the call
    def __call__(self, batch, n_samples: int = 25, permutations=None, generator=None, class_index: int = 0, node_group=None,
                 edge_group=None, group_permutations=None, per_model: bool = False, models_per_launch: Optional[int] = None,
                 samples_per_launch: Optional[int] = None):
        _frozen.positive("models_per_launch", models_per_launch)
        if samples_per_launch is not None and not 1 <= int(samples_per_launch) <= 65535:
            raise ValueError(f"samples_per_launch must lie in 1 .. 65535; got {samples_per_launch}")
        pl, given = _groups._players(batch, permutations, node_group, edge_group, group_permutations)
        a = self._args
        if self._shape_args(a, batch, perm_count=1, **pl.query) is not None:
            return self._loop(pl, pl.permutations(n_samples, given, generator), class_index, per_model)
        x = _frozen.batch_x(batch)
        M, B, C, dev, row = len(self.models), a.B, a.C, x.device, pl.row
        cls = self._class(class_index)
        perm = pl.permutations(n_samples, given, generator)
        P = int(perm.shape[0])
        steps = pl.max_steps(a)

        def samples(graphs: int) -> int:
            if samples_per_launch is not None:
                return min(int(samples_per_launch), P)
            return ShapleySampling.default_samples_per_launch(P, graphs, row, steps, pl.per_cu)
        # the one-model workspace of the largest launch (a chunk of several models takes no more permutations per launch)
        _frozen.query(a, self.KERNEL, self._shape(), batch, perm_count=samples(B), n_models=1, **pl.query)
        ws_one = int(a.workspace_bytes_needed)
        weights = self._weights(dev)
        Ml = _models_per_launch(models_per_launch, M, ws_one, row + 2 * B * C)
        rows = M if per_model else Ml
        take, front = self._bufs.take, _frozen.front
        acc, out, base = take("acc", (rows, row), dev), take("out", (M, B, C), dev), take("base", (M, B, C), dev)
        mean, m2, std = take("mean", (row,), dev), take("m2", (row,), dev), take("std", (row,), dev)
        self._fill(a, pl.flags, batch, x, None, self._bufs.workspace(Ml * ws_one, dev))
        a.perm, a.n_perm, a.class_index = _lib.ptr(perm), P, cls
        pl.fill(a)
        q = self._moments_block((mean, m2, std, row))
        lib, stream = _lib.load(), _lib.stream_ptr()
        for m0, count, row0 in self._model_chunks(a, weights, Ml, per_model, q):
            a.out, a.out_base = front(out) + 4 * m0 * B * C, front(base) + 4 * m0 * B * C
            q.mom_values0 = a.shap_acc = front(acc) + 4 * row0 * row
            spl = samples(B * count)
            for first in range(0, P, spl):
                a.perm_first, a.perm_count = first, min(spl, P - first)
                _lib.check(lib.hcg_explain(ctypes.addressof(a), stream), pl.label + " (ensemble)")
        self.last_path = "fused"
        return self._result(pl, mean, std, out, base, acc if per_model else None)

    @staticmethod
    def _result(pl, mean, std, out_full, out_base, per):
        """`per`: the per-model accumulators [M, row] or None"""
        rm, rs = pl.result(mean, out_full, out_base), pl.result(std, out_full, out_base)
        if hasattr(pl, "groups"):
            return EnsembleShapleyResult(rm.group_attr, rs.group_attr, rm.group_ptr, rm.node_attr, rs.node_attr, rm.edge_attr,
                                         rs.edge_attr, out_full, out_base, per)
        NF = pl.N * pl.F
        return EnsembleFeatureShapleyResult(rm.node_attr, rs.node_attr, rm.edge_attr, rs.edge_attr, out_full, out_base,
                                            None if per is None else per[:, :NF].view(-1, pl.N, pl.F),
                                            None if per is None else per[:, NF:pl.row])

    # ------------------------------------------------------------------ the loop path (any shape, CPU tensors)
    def loop(self, batch, n_samples: int = 25, permutations=None, generator=None, class_index: int = 0, node_group=None,
             edge_group=None, group_permutations=None, per_model: bool = False):
        """`ShapleySampling(model_k).loop` per model on the models' current weights with one set of permutations, the moments
        with torch ops, whatever `reason(batch)` says."""
        pl, given = _groups._players(batch, permutations, node_group, edge_group, group_permutations)
        return self._loop(pl, pl.permutations(n_samples, given, generator), class_index, per_model)

    def _loop(self, pl, perm, class_index, per_model):
        grouped = hasattr(pl, "groups")
        rs = [s._walk(pl, perm, class_index) for s in self._singles]
        per = torch.stack([(r.group_attr if grouped else torch.cat([r.node_attr.reshape(-1), r.edge_attr])) for r in rs])
        self.last_path = "loop"
        return self._result(pl, per.mean(0), per.std(0, unbiased=False), torch.stack([r.out_full for r in rs]),
                            torch.stack([r.out_base for r in rs]), per if per_model else None)


class EnsembleSubsetValues(FrozenEnsemble):
    """The outputs of M frozen models of one architecture for a LIST of subsets of each graph's groups: every (job, model)
    pair is one workgroup, the mean and the standard deviation over the models taken on the device.

        ev = EnsembleSubsetValues(models)
        r = ev(batch, subsets, node_group=None, edge_group=None, rows_per_graph=None, rows_per_workgroup=None,
               per_model=False, models_per_launch=None)
        # EnsembleSubsetResult(mean [S, B, C], std [S, B, C], group_ptr, out_full [M, B, C], out_base [M, B, C],
        #                      values [M, S, B, C] | None)

    Arguments, checks and errors are `SubsetValues`'; the group layout, the job list and the bit words are built ONCE per
    call (`_groups._SubsetCall`, as that class builds them), and shared by the models.  `values[m]`, `out_full[m]` and
    `out_base[m]` are bit for bit what `SubsetValues(models[m])` returns, and everything is bitwise independent of `models_per_launch`,
    `rows_per_workgroup`, `jobs_per_launch`, of the other models and of the rest of the batch.  `mean` / `std` are the
    moments over the models of the whole [S + 2, B, C] table (Welford in float32, population std, one `HCG_EXPLAIN_MOMENTS`
    launch per chunk of models): `mean` is the value of every subset under the ensemble's mean prediction.

    The models run in chunks of `models_per_launch` (None: as many as keep their tables under `LAUNCH_BUDGET_BYTES`); the
    jobs of a chunk in launches of `jobs_per_launch` (attribute; None: `CoalitionValues.default_jobs_per_launch` divided by
    the chunk's models).  With `per_model=False` only one chunk's tables exist.  The returned tensors are views of pool
    buffers, overwritten by the next call.

    When `reason(batch)` is not None (shape outside the kernel, CPU tensors, `use_fused` off on any model) or a graph has more
    than `MAX_SUBSET_GROUPS` groups the same call runs `loop`: `SubsetValues(model_k).loop` per model on the models' CURRENT
    weights, the moments with torch ops.  `last_path` says which one ran."""

    KERNEL, NAME = _lib.HCG_EXPLAIN_SUBSETS, "EnsembleSubsetValues"
    jobs_per_launch: Optional[int] = None

    def __init__(self, models: Sequence[torch.nn.Module]):
        super().__init__(models)
        self._singles = [SubsetValues(m) for m in self.models]             # the loop path's workers

    def _shape_args(self, a, batch, **extra) -> Optional[str]:
        return super()._shape_args(a, batch, n_models=1, **extra)

    def __call__(self, batch, subsets, node_group=None, edge_group=None, rows_per_graph=None,
                 rows_per_workgroup: Optional[int] = None, per_model: bool = False,
                 models_per_launch: Optional[int] = None) -> EnsembleSubsetResult:
        why = self._shape_args(self._args, batch)
        gr, counts = _groups.subset_layout(batch, node_group, edge_group)
        rp = _groups.check_subsets(batch, gr, subsets, rows_per_graph, self.C)
        mean, std, full, base, values = self._tables(batch, gr, counts, subsets, rp, rows_per_workgroup, per_model,
                                                     models_per_launch, why)
        S = int(subsets.shape[0])
        return EnsembleSubsetResult(mean[:S], std[:S], gr.group_ptr, full, base, None if values is None else values[:, :S])

    def loop(self, batch, subsets, node_group=None, edge_group=None, rows_per_graph=None, per_model: bool = False):
        """`SubsetValues(model_k).loop` per model, the moments with torch ops, whatever `reason(batch)` says."""
        gr, counts = _groups.subset_layout(batch, node_group, edge_group)
        rp = _groups.check_subsets(batch, gr, subsets, rows_per_graph, self.C)
        mean, std, full, base, values = self._loop(batch, gr, subsets, rp, per_model)
        S = int(subsets.shape[0])
        return EnsembleSubsetResult(mean[:S], std[:S], gr.group_ptr, full, base, None if values is None else values[:, :S])

    def _loop(self, batch, gr, subsets, rp, per_model):
        tables = torch.stack([s._loop(batch, gr, subsets, rp) for s in self._singles])       # [M, S + 2, B, C]
        S = int(subsets.shape[0])
        self.last_path = "loop"
        return tables.mean(0), tables.std(0, unbiased=False), tables[:, S], tables[:, S + 1], tables if per_model else None

    def _tables(self, batch, gr, counts, subsets, rp, rows_per_workgroup, per_model, models_per_launch, why):
        """-> (mean [S + 2, B, C], std [S + 2, B, C], out_full [M, B, C], out_base [M, B, C], the models' tables
        [M, S + 2, B, C] or None): the rows of `subsets`, then everything on, then the background only"""
        rpw = _frozen.positive("rows_per_workgroup", rows_per_workgroup)
        _frozen.positive("models_per_launch", models_per_launch)
        jpl = _frozen.positive("jobs_per_launch", self.jobs_per_launch)
        if why is not None or gr.max_groups > MAX_SUBSET_GROUPS:
            return self._loop(batch, gr, subsets, rp, per_model)
        a = self._args
        x = _frozen.batch_x(batch, subsets)
        M, B, C, dev = len(self.models), a.B, a.C, x.device
        S = int(subsets.shape[0])
        rpw = rpw or CoalitionValues.default_subsets_per_workgroup(S * B * M)
        call = _groups._SubsetCall(B, gr, counts, subsets, rp, rpw)
        S2, J = call.S2, call.J
        length = S2 * B * C
        Ml = _models_per_launch(models_per_launch, M, 0, length)
        take, front = self._bufs.take, _frozen.front
        tables = take("tables", (M if per_model else Ml, S2, B, C), dev)
        full, base = take("full", (M, B, C), dev), take("base", (M, B, C), dev)
        mean, m2, std = take("mean", (S2, B, C), dev), take("m2", (S2, B, C), dev), take("std", (S2, B, C), dev)
        if rp is not None:
            tables.zero_()
        self.last_path = "fused"
        if J == 0:                                                          # (no graph: nothing to launch)
            return mean, std, full, base, tables if per_model else None
        _frozen.query(a, self.KERNEL, self._shape(), batch, n_models=1, **call.query)
        weights = self._weights(dev)
        self._fill(a, 0, batch, x, None)
        call.fill(a)
        q = self._moments_block((mean, m2, std, length))
        for m0, count, row0 in self._model_chunks(a, weights, Ml, per_model, q):
            q.mom_values0 = a.coal_values = front(tables) + 4 * row0 * length
            _frozen.launch_jobs(a, 0, J, jpl or max(1, CoalitionValues.default_jobs_per_launch(rpw) // count),
                                "hcg_explain (subsets, ensemble)")
            # (out_full / out_base of the chunk: they read its tables, as the moments launch behind them does)
            chunk = tables[row0:row0 + count]
            full[m0:m0 + count].copy_(chunk[:, S])
            base[m0:m0 + count].copy_(chunk[:, S + 1])
        return mean, std, full, base, tables if per_model else None


class EnsembleCurves:
    """Deletion and insertion curves of an order of each graph's groups under the MEAN output of an ensemble: what judges an
    ensemble attribution (`EnsembleShapley.group_mean`, `EnsembleAttribution`'s means summed by `group_scores`).

        ec = EnsembleCurves(models)
        r = ec(batch, order, node_group=None, edge_group=None, class_index=0, fractions=None)
        # EnsembleCurveResult(insertion [Pn, C], deletion [Pn, C], k, curve_ptr, group_ptr, insertion_auc [B], deletion_auc [B],
        #                     out_full [B, C], out_base [B, C], insertion_std [Pn, C], deletion_std [Pn, C])

    Arguments, points and rows are `AttributionCurves`' (its own row construction); the rows go through ONE
    `EnsembleSubsetValues` call (`values` is that instance: its kernel, its loop path, its `reason`).  A point of `insertion` /
    `deletion` is bitwise the `mean` of that call's row, `insertion_std` / `deletion_std` its `std`; the areas are the
    trapezoid rule over the mean curves, as `AttributionCurves` forms them.  `out_full` / `out_base` are the mean outputs.
    The returned tensors are new."""

    def __init__(self, models: Sequence[torch.nn.Module]):
        self.values = EnsembleSubsetValues(models)

    @property
    def last_path(self) -> Optional[str]:
        return self.values.last_path

    def reason(self, batch=None) -> Optional[str]:
        return self.values.reason(batch)

    def refresh(self):
        self.values.refresh()
        return self

    def __call__(self, batch, order, node_group=None, edge_group=None, class_index: int = 0,
                 fractions: Optional[Sequence[float]] = None, rows_per_workgroup: Optional[int] = None,
                 models_per_launch: Optional[int] = None) -> EnsembleCurveResult:
        ev = self.values
        why = ev._shape_args(ev._args, batch)
        cls = ev._class(class_index)
        fr = AttributionCurves._fractions(fractions)
        gr, counts = _groups.subset_layout(batch, node_group, edge_group)
        plan = AttributionCurves._plan(gr, counts, order, fr, batch.x.device)
        rp = _groups.check_subsets(batch, gr, plan.rows, torch.tensor(plan.rows_per_graph, dtype=torch.int64), ev.C)
        mean, std, _, _, _ = ev._tables(batch, gr, counts, plan.rows, rp, rows_per_workgroup, False, models_per_launch, why)
        insertion, deletion = AttributionCurves._gather(mean, plan)
        ins_std, del_std = AttributionCurves._gather(std, plan)
        ins_auc, del_auc = AttributionCurves._areas(insertion, deletion, plan, cls)
        return EnsembleCurveResult(insertion, deletion, plan.k, plan.curve_ptr, gr.group_ptr, ins_auc, del_auc,
                                   mean[plan.S].clone(), mean[plan.S + 1].clone(), ins_std, del_std)
