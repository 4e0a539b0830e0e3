"""Subset values and deletion / insertion curves: which attribution of a graph's players to believe.

The package has five ways to attribute a prediction to the atoms, bonds or fragments of a graph (`ExplainFit`,
`ShapleySampling`, `CoalitionValues`, `IntegratedGradients`, `EnsembleAttribution`).  The usual way to compare two rankings
of the same players is to ask the model itself: remove the players in the claimed order of importance and watch the output
(the deletion curve), or start from the background and add them in that order (the insertion curve).  Both are model
evaluations on chosen SUBSETS of a graph's groups, about 2 G_g of them per graph and ranking.

`SubsetValues` evaluates a caller's list of subsets for a whole batch on chip (csrc/shapley.hip, k_subset_values,
`HCG_EXPLAIN_SUBSETS`): one workgroup per (graph, run of rows) builds its graph once and, for every row, rebuilds the state
from zero -- the live background, then ONE filtered pass over the graph's member list that applies the members whose
group's bit is set -- and evaluates it with the evaluation the Shapley walk and `CoalitionValues` use.  Any number of
groups per graph (atoms as players: 57 - 184), where `CoalitionValues` enumerates all 2^L masks of at most 16.  For the same
subset the rows are bitwise `CoalitionValues`' rows.  `AttributionCurves` builds the rows of both curves for an order of the
groups, evaluates them in one `SubsetValues` call and returns the curves and their areas; `ranking` and `group_scores` turn
any of the five attributions into such an order.  `pack_subsets` is the bit layout the kernel reads.
"""
from __future__ import annotations

import math
from typing import NamedTuple, Optional, Sequence

import torch

from . import _frozen, _groups, _lib
from ._groups import _group_graph, _group_layout, _member_group, _pack  # noqa: F401  (`_member_group`: reached here as before)
from .shapley import CoalitionValues

MAX_SUBSET_GROUPS = 16384          # groups of one graph: the bits the kernel's staging holds (a graph inside the shape limits
#                                    has at most 184 * 64 + 1024 = 12800 features, so no such graph reaches it)


class SubsetResult(NamedTuple):
    values: torch.Tensor         # [S, B, C]: values[s, g] = the output with the background and row s's groups of graph g on
    group_ptr: torch.Tensor      # [B + 1] int64: column group_ptr[g] + y of `subsets` is group y of graph g
    out_full: torch.Tensor       # [B, C] every group on (= the plain forward)
    out_base: torch.Tensor       # [B, C] the background only


class CurveResult(NamedTuple):
    insertion: torch.Tensor      # [Pn, C] point curve_ptr[g] + j: the background and the first k groups of the order on
    deletion: torch.Tensor       # [Pn, C] everything but those k groups on
    k: torch.Tensor              # [Pn] int64
    curve_ptr: torch.Tensor      # [B + 1] int64
    group_ptr: torch.Tensor      # [B + 1] int64
    insertion_auc: torch.Tensor  # [B] trapezoid rule over x = k / G_g on column `class_index`
    deletion_auc: torch.Tensor   # [B]
    out_full: torch.Tensor       # [B, C]
    out_base: torch.Tensor       # [B, C]


class _CurvePlan(NamedTuple):
    """The points of both curves of an order and the rows that hold them (`AttributionCurves._plan`); tensors on the batch's device."""
    rows: torch.Tensor           # [S, G] bool: row 2 i = the first k groups of a graph's pair i, 2 i + 1 = everything else
    rows_per_graph: list         # [B] host: the rows graph g uses
    S: int
    ins_row: torch.Tensor        # [Pn] int64: the row of the [S + 2, B, C] table that is the point's insertion value
    del_row: torch.Tensor        # [Pn]
    graph: torch.Tensor          # [Pn] int64: the point's graph
    k: torch.Tensor              # [Pn] int64
    curve_ptr: torch.Tensor      # [B + 1] int64
    groups: torch.Tensor         # [Pn] int64: G_g of the point's graph
    points: torch.Tensor         # [B] int64: points per graph
    count: torch.Tensor          # [B] int64: G_g


# ====================================================================== the bit layout
def pack_subsets(subsets: torch.Tensor, group_ptr: torch.Tensor):
    """bool [S, G] (column group_ptr[g] + y = group y of graph g, the layout of `group_permutations`) -> (bits [S, W], the
    uint32 words in int32 storage, and word_ptr int32 [B + 1], the prefix sum of ceil(G_g / 32), W = word_ptr[B]): group y of
    graph g is on in row s iff bit y & 31 of bits[s, word_ptr[g] + (y >> 5)] is set.  Bits at or above G_g in a graph's last
    word are 0.  Built with torch ops on the tensor's device; one host read (W)."""
    if not torch.is_tensor(subsets) or subsets.dtype != torch.bool or subsets.dim() != 2:
        raise ValueError(f"subsets must be a bool tensor [S, G]; got {getattr(subsets, 'dtype', type(subsets))} "
                         f"{tuple(getattr(subsets, 'shape', ()))}")
    gp = torch.as_tensor(group_ptr).to(subsets.device, torch.int64)
    if gp.dim() != 1 or gp.numel() < 1:
        raise ValueError("group_ptr must be [B + 1]")
    ends = gp.tolist()
    if ends[0] != 0 or ends[-1] != subsets.shape[1] or any(b < a for a, b in zip(ends[:-1], ends[1:])):
        raise ValueError(f"group_ptr must ascend from 0 to G = {subsets.shape[1]}; got {ends[0]} .. {ends[-1]}")
    return _pack(subsets, gp, sum((b - a + 31) // 32 for a, b in zip(ends[:-1], ends[1:])))


def _segment_sums(values: torch.Tensor, lengths: torch.Tensor) -> torch.Tensor:
    """float64 [len(lengths)]: the sums of consecutive segments of `values`, each added in its own order by one owner"""
    if values.numel() == 0:
        return torch.zeros(lengths.numel(), dtype=torch.float64, device=values.device)
    return torch.segment_reduce(values.to(torch.float64).contiguous(), "sum", lengths=lengths.to(torch.int64), unsafe=True)


# ====================================================================== orders of the groups
def ranking(scores: torch.Tensor, group_ptr: torch.Tensor, by: str = "value", descending: bool = True) -> torch.Tensor:
    """int32 [1, G] in the layout of `group_permutations`: graph g's segment lists its groups 0 .. G_g - 1 by `scores`
    ([G]: `GroupedShapleyResult.group_attr`, `CoalitionResult.group_attr`, `group_scores(...)`), the highest first
    (`descending`), by the value itself or by its magnitude (`by="abs"`).  A stable sort per graph: ties go to the lower
    group id.  Torch ops on the scores' device, no host read."""
    if by not in ("value", "abs"):
        raise ValueError(f"by must be 'value' or 'abs'; got {by!r}")
    if not torch.is_tensor(scores) or scores.dim() != 1:
        raise ValueError(f"scores must be a tensor [G]; got {tuple(getattr(scores, 'shape', ()))}")
    G, dev = int(scores.numel()), scores.device
    gp = torch.as_tensor(group_ptr).to(dev, torch.int64)
    graph = _group_graph(gp[1:] - gp[:-1], G)
    key = scores.abs() if by == "abs" else scores
    first = torch.sort(key, descending=bool(descending), stable=True).indices       # (equal scores: ascending global id)
    second = torch.sort(graph[first], stable=True).indices                           # graph by graph, the order kept
    order = first[second]
    return (order - gp[graph[order]]).to(torch.int32).reshape(1, G)


def group_scores(node_attr, edge_attr, node_group, edge_group, batch):
    """-> (scores [G] float32, group_ptr [B + 1] int64): a per-entry attribution (`IntegratedGradients`' node_attr [N, F] /
    edge_attr [E], `ExplainFit`'s masks, ungrouped `ShapleySampling`; either may be None = zeros) summed into the groups of
    `node_group` / `edge_group` (`ShapleySampling`'s arguments and checks), so that it can be ranked on the same players as
    a grouped attribution.  The background's entries are dropped.  Every group's sum is formed in float64 by one owner in
    ascending feature order (a stable sort by group, then a segment sum) on the batch's device, and rounded to float32."""
    (N, F), E, dev = batch.x.shape, int(batch.edge_index.shape[1]), batch.x.device
    gr = _group_layout(batch, int(F), node_group, edge_group)
    parts = []
    for t, shape, name in ((node_attr, (N, F), "node_attr"), (edge_attr, (E,), "edge_attr")):
        if t is None:
            parts.append(torch.zeros(math.prod(shape), dtype=torch.float64, device=dev))
            continue
        if not torch.is_tensor(t) or tuple(t.shape) != tuple(shape) or t.device != dev:
            raise ValueError(f"{name} must be a tensor of shape {list(shape)} on {dev}; got {tuple(getattr(t, 'shape', ()))} "
                             f"on {getattr(t, 'device', None)}")
        parts.append(t.detach().reshape(-1).to(torch.float64))
    order = torch.sort(gr.slot, stable=True).indices
    sums = _segment_sums(torch.cat(parts)[order], torch.bincount(gr.slot, minlength=gr.G + 1))
    return sums[:gr.G].to(torch.float32), gr.group_ptr


# ====================================================================== a list of subsets evaluated on chip
class SubsetValues(_frozen.FrozenModel):
    """The model's output for a LIST of subsets of each graph's groups, for a whole batch of graphs.

        sv = SubsetValues(model)
        r = sv(batch, subsets, node_group=None, edge_group=None, rows_per_graph=None, rows_per_workgroup=None)
        # SubsetResult(values [S, B, C], group_ptr [B + 1], out_full [B, C], out_base [B, C])

    `node_group` / `edge_group` are `ShapleySampling`'s: local ids 0 .. G_g - 1, -1 for the background, the same checks and
    errors; any number of groups per graph.  `subsets` is a bool tensor [S, G] on the batch's device, column
    group_ptr[g] + y = group y of graph g (the layout of `group_permutations`; dtype, shape and device are checked); S = 0
    is allowed.  `values[s, g]` is the output [C] with the background and row s's groups of graph g on.  `out_full` /
    `out_base` come from two rows (all on, all off) the class appends itself, so a call with S = 0 still returns them.

    `rows_per_graph`: an integer tensor [B] (on any device: it is read on the host) or None.  Graph g evaluates its rows
    0 .. rows_per_graph[g] - 1 only; its other rows are exactly 0 and cost nothing: no job is emitted for them.

    One workgroup evaluates a run of up to `rows_per_workgroup` rows of one graph on chip (csrc/shapley.hip,
    k_subset_values): it builds the graph once and rebuilds the state from zero for every row -- the live background, then
    one filtered pass over the graph's member list -- so `values[s, g]` depends on row s's bits of graph g and on graph g
    alone: it is bitwise independent of the run length, of the launch split, of the other rows and their order, of the run
    and of the rest of the batch, and bitwise the row `CoalitionValues` has for the same subset.  Rows that differ only in a
    group without a live member are equal.  None for `rows_per_workgroup`: `CoalitionValues.default_subsets_per_workgroup`
    applied to S * B.  Jobs are split into launches by `CoalitionValues.default_jobs_per_launch` (`jobs_per_launch`; set
    the attribute to force a split).  The [S + 2, B, C] table must fit `attribution.LAUNCH_BUDGET_BYTES` (ValueError: split
    the rows or the batch).

    Host reads, once per call each: what `_group_layout` reads (three scalars) and `group_ptr` (and `rows_per_graph`, when
    it is given on the device).  The table is a pool buffer: the returned `values`, `out_full` and `out_base` are views of
    it, overwritten by the next call (it is cleared first on a call with `rows_per_graph`).

    When `reason(batch)` is not None (shape outside the kernel, CPU tensors, `use_fused` off) or a graph has more than
    `MAX_SUBSET_GROUPS` groups the same call runs `loop`: one masked forward of the whole batch per row (forward-only
    `ExplainStep` on GPU tensors, plain torch ops on CPU tensors); its tensors are new.  `last_path` says which one ran."""

    KERNEL, NAME = _lib.HCG_EXPLAIN_SUBSETS, "SubsetValues"
    jobs_per_launch: Optional[int] = None          # None: `CoalitionValues.default_jobs_per_launch`

    # ------------------------------------------------------------------ the call
    def __call__(self, batch, subsets, node_group=None, edge_group=None, rows_per_graph=None,
                 rows_per_workgroup: Optional[int] = None) -> SubsetResult:
        why = self._shape_args(self._args, batch)
        gr, counts = _groups.subset_layout(batch, node_group, edge_group)
        rp = _groups.check_subsets(batch, gr, subsets, rows_per_graph, self._shape()[2])
        table = self._table(batch, gr, counts, subsets, rp, rows_per_workgroup, why)
        S = int(subsets.shape[0])
        return SubsetResult(table[:S], gr.group_ptr, table[S], table[S + 1])

    def loop(self, batch, subsets, node_group=None, edge_group=None, rows_per_graph=None) -> SubsetResult:
        """The batch-synchronous loop (see the class docstring), whatever `reason(batch)` says."""
        gr, counts = _groups.subset_layout(batch, node_group, edge_group)
        rp = _groups.check_subsets(batch, gr, subsets, rows_per_graph, self._shape()[2])
        table = self._loop(batch, gr, subsets, rp)
        S = int(subsets.shape[0])
        return SubsetResult(table[:S], gr.group_ptr, table[S], table[S + 1])

    def _table(self, batch, gr, counts, subsets, rp, rows_per_workgroup, why) -> torch.Tensor:
        """[S + 2, B, C]: the rows of `subsets`, then everything on, then the background only.  `why`: `_shape_args`'
        answer for this batch (not None: the loop)."""
        rpw = _frozen.positive("rows_per_workgroup", rows_per_workgroup)
        if why is not None or gr.max_groups > MAX_SUBSET_GROUPS:
            return self._loop(batch, gr, subsets, rp)
        a = self._args
        x = _frozen.batch_x(batch, subsets)
        B, C, dev = a.B, a.C, x.device
        rpw = rpw or CoalitionValues.default_subsets_per_workgroup(int(subsets.shape[0]) * B)
        jpl = _frozen.positive("jobs_per_launch", self.jobs_per_launch) or CoalitionValues.default_jobs_per_launch(rpw)
        call = _groups._SubsetCall(B, gr, counts, subsets, rp, rpw)
        table = self._bufs.take("table", (call.S2, B, C), dev)
        if rp is not None:
            table.zero_()
        self.last_path = "fused"
        if call.J == 0:                                                     # (no graph: nothing to launch)
            return table
        _frozen.query(a, self.KERNEL, self._shape(), batch, **call.query)
        self._fill(a, 0, batch, x, self._weights(dev))
        call.fill(a)
        a.coal_values = _frozen.front(table)
        _frozen.launch_jobs(a, 0, call.J, jpl, "hcg_explain (subsets)")
        return table

    # ------------------------------------------------------------------ the existing path (any shape): one forward per row
    def _loop(self, batch, gr, subsets, rp) -> torch.Tensor:
        (N, F), B, dev = batch.x.shape, int(batch.num_graphs), batch.x.device
        S, G, C = int(subsets.shape[0]), gr.G, int(self.model._n_classes)
        table = torch.zeros(S + 2, B, C, dtype=torch.float32, device=dev)
        self.last_path = "loop"
        if B == 0:
            return table
        on_bg = torch.ones(1, dtype=torch.bool, device=dev)                 # (the background reads the appended entry)
        extra = (torch.ones(G, dtype=torch.bool, device=dev), torch.zeros(G, dtype=torch.bool, device=dev))
        top = S if rp is None else max(rp)
        with torch.no_grad():
            for s in list(range(top)) + [S, S + 1]:
                row = subsets[s] if s < S else extra[s - S]
                on = torch.cat([row, on_bg])[gr.slot].to(torch.float32)
                table[s] = self._masked_forward(batch, on[:N * F].view(N, F), on[N * F:]).reshape(B, -1).to(torch.float32)
        if rp is not None and S > 0:
            off = torch.arange(S, device=dev).unsqueeze(1) >= torch.tensor(rp, dtype=torch.int64, device=dev).unsqueeze(0)
            table[:S][off] = 0.0
        return table


# ====================================================================== deletion and insertion curves
class AttributionCurves:
    """Deletion and insertion curves of an order of each graph's groups, and their areas.

        ac = AttributionCurves(model)
        r = ac(batch, order, node_group=None, edge_group=None, class_index=0, fractions=None)
        # CurveResult(insertion [Pn, C], deletion [Pn, C], k [Pn] int64, curve_ptr [B + 1], group_ptr,
        #             insertion_auc [B], deletion_auc [B], out_full, out_base)

    `node_group` / `edge_group` are `ShapleySampling`'s.  `order` is an int32 tensor [G] or [1, G] on the batch's device in
    the layout of `group_permutations` (`ranking(...)` makes one from any attribution): graph g's segment must be a
    permutation of 0 .. G_g - 1, which is checked on the device with one sort and one host read (ValueError otherwise).
    For graph g and point j, with k = k[curve_ptr[g] + j]: `insertion` is the output with the background and the first k
    groups of the order on, `deletion` the output with everything but those k groups on.  A good ranking makes the
    insertion curve rise early and the deletion curve fall early.  `fractions=None`: the points are k = 0 .. G_g, G_g + 1
    of them (a graph without groups has one).  `fractions`: a non-decreasing sequence of floats in [0, 1] (at least one):
    every graph has len(fractions) points at k = floor(f * G_g + 0.5), duplicates kept.

    The class builds the bool rows and calls `SubsetValues` once (its kernel, its loop path, its `reason`; `values` is that
    instance), with `rows_per_graph`: no subset of a graph is evaluated twice -- insertion at k = 0 and deletion at k = G_g
    are the one background row, insertion at k = G_g and deletion at k = 0 the one full row, a k that fractions repeat is
    one pair of rows -- and the rows are gathered into the two curves, so a point is bitwise the `SubsetValues` row of its
    subset.  `insertion_auc[g]` / `deletion_auc[g]` are the trapezoid rule over x = k / G_g on column `class_index`, formed
    in float64 by torch ops and rounded to float32; a graph with G_g = 0 gets its single value.

    Fidelity at a fraction is read off the curves, there is no call for it: `out_full - deletion` at that point is the
    fidelity+ of the top-k groups (how much the output moves when they are removed), `out_full - insertion` the fidelity-
    (how much is still missing when only they are kept).  The returned tensors are new."""

    def __init__(self, model: torch.nn.Module):
        self.values = SubsetValues(model)

    @property
    def last_path(self) -> Optional[str]:
        return self.values.last_path

    def reason(self, batch=None) -> Optional[str]:
        return self.values.reason(batch)

    def lds_bytes(self, batch) -> Optional[int]:
        return self.values.lds_bytes(batch)

    @staticmethod
    def _fractions(fractions) -> Optional[list]:
        if fractions is None:
            return None
        try:
            fr = [float(f) for f in fractions]
        except (TypeError, ValueError):
            raise ValueError(f"fractions must be a sequence of floats; got {fractions!r}") from None
        if not fr or any(not 0.0 <= f <= 1.0 for f in fr) or any(b < a for a, b in zip(fr[:-1], fr[1:])):
            raise ValueError(f"fractions must be a non-decreasing sequence of at least one float in [0, 1]; got {fractions!r}")
        return fr

    def __call__(self, batch, order, node_group=None, edge_group=None, class_index: int = 0,
                 fractions: Optional[Sequence[float]] = None, rows_per_workgroup: Optional[int] = None) -> CurveResult:
        sv = self.values
        why = sv._shape_args(sv._args, batch)
        cls = sv._class(class_index)
        fr = self._fractions(fractions)
        gr, counts = _groups.subset_layout(batch, node_group, edge_group)
        plan = self._plan(gr, counts, order, fr, batch.x.device)
        table = sv._table(batch, gr, counts, plan.rows, plan.rows_per_graph, rows_per_workgroup, why)
        insertion, deletion = self._gather(table, plan)
        ins_auc, del_auc = self._areas(insertion, deletion, plan, cls)
        # (rows S and S + 1: everything on, the background only)
        return CurveResult(insertion, deletion, plan.k, plan.curve_ptr, gr.group_ptr, ins_auc, del_auc,
                           table[plan.S].clone(), table[plan.S + 1].clone())

    # ------------------------------------------------------------------ the rows and points of an order (`EnsembleCurves` too)
    @staticmethod
    def _plan(gr, counts, order, fr, dev) -> _CurvePlan:
        """`order` checked; the points of both curves and the bool rows [S, G] of the one `SubsetValues` call that holds them"""
        B, G = len(counts), gr.G
        if not torch.is_tensor(order) or order.dtype != torch.int32 or tuple(order.shape) not in ((G,), (1, G)):
            raise ValueError(f"order must be an int32 tensor of shape [G = {G}] or [1, {G}]; got "
                             f"{getattr(order, 'dtype', type(order))} {tuple(getattr(order, 'shape', ()))}")
        if order.device != dev:
            raise ValueError(f"order is on {order.device}, the batch on {dev}")
        # every graph's segment a permutation of its local ids: one sort, one read
        o = order.reshape(-1).to(torch.int64)
        ggraph = _group_graph(gr.count, G)
        inside = (o >= 0) & (o < gr.count[ggraph])
        glob = gr.group_ptr[ggraph] + torch.where(inside, o, torch.zeros_like(o))
        if not bool(inside.all() & (torch.sort(glob).values == torch.arange(G, device=dev)).all()):
            raise ValueError("order must hold, for every graph at group_ptr[g], a permutation of 0 .. G_g - 1")
        pos = torch.empty(G, dtype=torch.int64, device=dev)
        pos[glob] = torch.arange(G, device=dev) - gr.group_ptr[ggraph]      # the group's place in its graph's order

        # ---- the points, on the host (from `counts`): k, and which row of the call holds each
        cnt = torch.tensor(counts, dtype=torch.int64)
        npts = cnt + 1 if fr is None else torch.full((B,), len(fr), dtype=torch.int64)
        cptr = torch.zeros(B + 1, dtype=torch.int64)
        cptr[1:] = npts.cumsum(0)
        Pn = int(cptr[-1])
        pg = torch.repeat_interleave(torch.arange(B), npts, output_size=Pn)
        j = torch.arange(Pn) - cptr[pg]
        Gp = cnt[pg]
        k = j if fr is None else torch.floor(torch.tensor(fr, dtype=torch.float64)[j] * Gp.to(torch.float64) + 0.5).to(torch.int64)
        # an interior k (0 < k < G_g) takes a pair of rows of its graph, a repeated one the pair it has; k = 0 and k = G_g
        # are the two rows `SubsetValues` appends
        interior = (k > 0) & (k < Gp)
        repeat = torch.zeros(Pn, dtype=torch.bool)
        if Pn > 1:
            repeat[1:] = (pg[1:] == pg[:-1]) & (k[1:] == k[:-1])
        new = interior & ~repeat
        c0 = torch.cat([torch.zeros(1, dtype=torch.int64), new.to(torch.int64).cumsum(0)])
        pair = c0[1:] - c0[cptr[:-1]][pg] - 1                               # the point's pair among its graph's pairs
        pairs = c0[cptr[1:]] - c0[cptr[:-1]]                                # [B]
        S = 2 * int(pairs.max()) if B > 0 else 0
        kpair = torch.zeros(max(S // 2, 1), B, dtype=torch.int16)
        kpair[pair[new], pg[new]] = k[new].to(torch.int16)

        # ---- the rows: 2 i = the first k groups of the order, 2 i + 1 = everything else
        r = torch.arange(S, device=dev)
        kk = kpair.to(dev)[r >> 1][:, ggraph]                               # [S, G]
        first = pos.to(torch.int16).unsqueeze(0) < kk
        rows = torch.where(((r & 1) == 1).unsqueeze(1), ~first, first) & (r.unsqueeze(1) < (2 * pairs).to(dev)[ggraph].unsqueeze(0))
        # ---- which row of the [S + 2, B, C] table holds each point (S: everything on, S + 1: the background only)
        full, base = torch.full_like(k, S), torch.full_like(k, S + 1)
        ins_row = torch.where(k == 0, base, torch.where(k == Gp, full, 2 * pair))
        del_row = torch.where(k == 0, full, torch.where(k == Gp, base, 2 * pair + 1))
        return _CurvePlan(rows, (2 * pairs).tolist(), S, ins_row.to(dev), del_row.to(dev), pg.to(dev), k.to(dev), cptr.to(dev),
                          Gp.to(dev), npts.to(dev), cnt.to(dev))

    @staticmethod
    def _gather(table, plan: _CurvePlan):
        """-> (insertion [Pn, ...], deletion [Pn, ...]): the points' rows of a [S + 2, B, ...] table"""
        return table[plan.ins_row, plan.graph], table[plan.del_row, plan.graph]

    @staticmethod
    def _areas(insertion, deletion, plan: _CurvePlan, cls: int):
        """-> (insertion_auc [B], deletion_auc [B]): the trapezoid rule over x = k / G_g on column `cls`, every graph's sum
        by one owner in point order"""
        pg_d, k_d, cptr_d, cnt, npts, dev = plan.graph, plan.k, plan.curve_ptr, plan.count, plan.points, plan.k.device
        B, Pn = int(cnt.numel()), int(k_d.numel())
        Gd = plan.groups.to(torch.float64)
        xq = torch.where(Gd > 0, k_d.to(torch.float64) / Gd.clamp(min=1.0), torch.zeros_like(Gd))
        aucs = []
        for curve in (insertion, deletion):
            v = curve[:, cls].to(torch.float64)
            area = torch.zeros(Pn, dtype=torch.float64, device=dev)         # (a graph's last point opens no trapezoid)
            if Pn > 1:
                same = pg_d[1:] == pg_d[:-1]
                area[:-1] = torch.where(same, (xq[1:] - xq[:-1]) * (v[1:] + v[:-1]) * 0.5, torch.zeros_like(v[1:]))
            auc = _segment_sums(area, npts)
            if B > 0:
                auc = torch.where(cnt == 0, v[cptr_d[:-1]], auc)
            aucs.append(auc.to(torch.float32))
        return aucs[0], aucs[1]
