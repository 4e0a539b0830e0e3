"""Greedy insertion and deletion orders: what the model itself says is the best order of a graph's players.

`AttributionCurves` tells which of two rankings the model believes; it does not tell how far a ranking is from what this
model allows on this molecule.  The usual yardstick is the model-driven greedy order: start from the background and always
add the group that raises the output most (insertion), or start from everything and always remove the group that lowers it
most (deletion).  Its curve is the practical upper envelope every attribution's curve is read against, and its first k
picks are the top-k sufficient (insertion) or necessary (deletion) set of groups -- "which k atoms carry the prediction?".

Round k's subsets depend on round k - 1's argmax, so the selection cannot be served from a fixed list of subsets: with
`SubsetValues` it is one call per round, each paying that call's host work.  `GreedySelection` decides on the device
(csrc/shapley.hip, k_greedy_round, `HCG_EXPLAIN_GREEDY`): the layout is built once, one launch per round is enqueued with
no host read in between, and every workgroup of a graph picks the previous round's winner itself before it evaluates its
share of this round's candidates with the very sequence `k_subset_values` runs for a row.
"""
from __future__ import annotations

from typing import NamedTuple, Optional

import torch

from . import _frozen, _groups, _lib
from .shapley import SUBSETS_PER_WORKGROUP
from .subsets import MAX_SUBSET_GROUPS, SubsetValues

MODES = ("insertion", "deletion")


class GreedyResult(NamedTuple):
    order: torch.Tensor          # [1, G] int32, the layout of `group_permutations`: group_ptr[g] + k = the pick of round k, -1 = none
    values: torch.Tensor         # [G, C]: values[group_ptr[g] + k] = the output after pick k, 0 where nothing was picked
    steps: torch.Tensor          # [B] int64: the filled positions of graph g (picks plus appended dead groups)
    group_ptr: torch.Tensor      # [B + 1] int64
    out_full: torch.Tensor       # [B, C] every group on (= the plain forward)
    out_base: torch.Tensor       # [B, C] the background only


def greedy_jobs(counts, rounds, ids_per_job: int):
    """The job lists of every launch of a fused call, built on the host: -> (jobs int32 [J, 3] of triples (graph, first id,
    ids), ptr: list [launches + 1] -- launch k runs the jobs ptr[k] .. ptr[k + 1] - 1).  `counts[g]` = G_g, `rounds[g]` =
    the rounds graph g runs.  In launch k a graph with rounds[g] > k has the jobs that tile its ids 0 .. G_g - 1 in ranges
    of `ids_per_job` (the one whose first id is 0 is its owner), a graph with rounds[g] == k the one job (g, 0, 0), which
    only picks, and a graph with rounds[g] < k none: max(rounds) + 1 launches (none without graphs)."""
    B, ipj = len(counts), int(ids_per_job)
    if B == 0:
        return torch.zeros(0, 3, dtype=torch.int32), [0]
    cnt, R = torch.tensor(counts, dtype=torch.int64), torch.tensor(rounds, dtype=torch.int64)
    per = (cnt + ipj - 1) // ipj
    g = torch.repeat_interleave(torch.arange(B), per)
    ptr = torch.zeros(B + 1, dtype=torch.int64)
    ptr[1:] = per.cumsum(0)
    at = (torch.arange(g.numel()) - ptr[g]) * ipj
    tiles = torch.stack([g, at, torch.clamp(cnt[g] - at, max=ipj)], 1)
    left = R[g]
    parts, lptr = [], [0]
    for k in range(int(R.max()) + 1):
        last = torch.nonzero(R == k).flatten()
        part = torch.cat([tiles[left > k], torch.stack([last, torch.zeros_like(last), torch.zeros_like(last)], 1)])
        parts.append(part)
        lptr.append(lptr[-1] + int(part.shape[0]))
    return torch.cat(parts).to(torch.int32).contiguous(), lptr


class GreedySelection(_frozen.FrozenModel):
    """The model-driven greedy insertion or deletion order of each graph's groups, for a whole batch of graphs.

        gs = GreedySelection(model)
        r = gs(batch, node_group=None, edge_group=None, class_index=0, mode="insertion", direction=1, steps=None,
               ids_per_job=None)
        # GreedyResult(order int32 [1, G], values [G, C], steps int64 [B], group_ptr int64 [B + 1], out_full [B, C],
        #              out_base [B, C])

    Players, background, `node_group` / `edge_group`, their checks and errors are `ShapleySampling`'s.  Per graph g with
    the groups 0 .. G_g - 1, of which L_g are live (have a live member):
      * `mode="insertion"`: the on-set starts empty (the background only); `mode="deletion"`: it starts full.
      * round k = 0, 1, ...: the candidates are the live groups not yet picked; candidate y's value is the model's output
        [C] with the background and (the on-set with y flipped) on; its key is sgn * value[class_index], sgn = `direction`
        for insertion and -`direction` for deletion, `direction` in {+1, -1}: by default insertion picks the largest rise
        and deletion the largest fall.  The pick is the candidate with the greatest key; equal keys go to the lower group
        id and a NaN key counts as -inf: a total order on (key, id), so the pick does not depend on the shape of the
        reduction.  The picked group's bit is flipped for good.
      * the graph runs min(`steps`, L_g) rounds (`steps=None`: L_g).  Dead groups are never candidates and cost no
        evaluation.
      * when the graph ran all L_g rounds its dead groups are appended behind the picks, ascending, with the last value
        repeated (rows that differ only in a dead group are equal, as `SubsetValues` documents); with L_g = 0 that value
        is `out_base` for insertion and `out_full` for deletion.
    `order[0, group_ptr[g] + k]` is the group picked in round k (-1 where nothing was picked), so a full run is a valid
    `order` of `AttributionCurves`; `values[group_ptr[g] + k]` is all C outputs of the state after pick k (0 where nothing
    was picked); `steps[g]` counts the filled positions.  The first k picks of an insertion run are the greedy top-k
    sufficient set, those of a deletion run the top-k necessary set.

    A fused call builds the layout once and enqueues max_g min(steps, L_g) + 1 launches on the current stream, one per
    round (csrc/shapley.hip, k_greedy_round), with no host read in between; `launches` counts them.  Launch k's workgroups
    each take `ids_per_job` consecutive group ids of one graph (None: `default_ids_per_job`): each stages the graph's on-set
    from the picks recorded so far, computes pick k - 1 itself from round k - 1's candidate values, and evaluates its own
    candidates of round k exactly as `SubsetValues`' kernel evaluates a row with those bits.  So a candidate's value is
    bitwise the `SubsetValues` row of the same subset, a pick is a function of those values alone, and the result is
    bitwise independent of `ids_per_job`, of the rest of the batch, of the call and of the instance, and bitwise `loop`'s.
    A graph the kernel refuses inside a launch (HCG_STATUS_SHAPE_LIMIT) has no pick (-1) and zero values and outputs.

    Host reads, once per call each: what `_group_layout` reads (three scalars) and the per-graph group and live counts,
    which give every launch's job list; the lists are uploaded once.  The returned tensors are new.  The tail (the dead
    groups' places, `steps`) is formed on the device behind the last launch; its small uploads are ordered behind the
    launches, so the call returns when the device is done.

    `loop` has the same arguments and runs whatever `reason` says: one `SubsetValues` table per round -- the rows are the
    on-set with one remaining candidate flipped each, evaluated through that class's own fused or loop path, so CPU tensors
    work -- and the pick by the same rule with torch ops on the batch's device.  `__call__` takes it when `reason(batch)`
    is not None (shape outside the kernel, CPU tensors, `use_fused` off) or a graph has more than `MAX_SUBSET_GROUPS`
    groups.  `last_path` says which one ran."""

    KERNEL, NAME = _lib.HCG_EXPLAIN_GREEDY, "GreedySelection"

    def __init__(self, model: torch.nn.Module):
        super().__init__(model)
        self.values = SubsetValues(model)           # the loop path's evaluator
        self.launches: Optional[int] = None         # launches of the last fused call

    @staticmethod
    def default_ids_per_job(remaining_total: int) -> int:
        """Group ids per workgroup, from the candidates the batch has in a launch (at most its live groups), after
        `CoalitionValues.default_subsets_per_workgroup`: up to `SUBSETS_PER_WORKGROUP` = 16, which spreads the graph's
        build (about the cost of one evaluation) over 16 candidates, but no more than leaves four workgroups for every
        CU, and never fewer than one id -- one graph of 184 atoms runs one id per workgroup, 535 graphs of 100 atoms 16."""
        return max(1, min(SUBSETS_PER_WORKGROUP, int(remaining_total) // (4 * _frozen.CUS)))

    # ------------------------------------------------------------------ what both paths share
    def _check(self, class_index, mode, direction, steps, ids_per_job):
        cls = self._class(class_index)
        if mode not in MODES:
            raise ValueError(f"mode must be 'insertion' or 'deletion'; got {mode!r}")
        if isinstance(direction, bool) or direction not in (1, -1):
            raise ValueError(f"direction must be +1 or -1; got {direction!r}")
        if steps is not None and int(steps) < 1:
            raise ValueError(f"steps must be at least 1 (or None: every live group); got {steps}")
        _frozen.positive("ids_per_job", ids_per_job)
        deletion = mode == "deletion"
        return cls, deletion, float(-int(direction) if deletion else int(direction)), None if steps is None else int(steps)

    @staticmethod
    def _layout(batch, node_group, edge_group, steps):
        """-> (the group layout, the graph of every group [G], per-graph counts, live counts and rounds on the host); one
        host read beside `_group_layout`'s"""
        B = int(batch.num_graphs)
        gr = _groups._group_layout(batch, int(batch.x.shape[1]), node_group, edge_group)
        ggraph = _groups._group_graph(gr.count, gr.G)
        nlive = _groups._flag_counts(ggraph, B, gr.live_group)
        counts, lives = torch.stack([gr.count, nlive]).tolist() if B > 0 else ([], [])
        rounds = [c if steps is None else min(steps, c) for c in lives]
        return gr, ggraph, counts, lives, rounds

    @staticmethod
    def _finish(gr, ggraph, counts, lives, rounds, deletion, order, values, out_full, out_base) -> GreedyResult:
        """Append the dead groups of every graph that ran all its rounds (ascending, the last value repeated) and count the
        filled positions; torch ops on the device, no host read."""
        dev, B, G = values.device, len(counts), gr.G
        full = [r == c for r, c in zip(rounds, lives)]
        steps = torch.tensor([r + (c - lv if f else 0) for r, c, lv, f in zip(rounds, counts, lives, full)], dtype=torch.int64, device=dev)
        if G > 0:
            lv = torch.tensor(lives, dtype=torch.int64, device=dev)
            dead = ~gr.live_group
            rank = _groups._flag_ranks(ggraph, B, dead).rank                # a dead group's index among its graph's dead groups
            sel = dead & torch.tensor(full, dtype=torch.bool, device=dev)[ggraph]
            # (a scatter with a spare slot for the groups that are not appended: a boolean index would read their number)
            at = torch.where(sel, gr.group_ptr[ggraph] + lv[ggraph] + rank, torch.full_like(rank, G))
            start = out_full if deletion else out_base
            lastv = torch.where((lv > 0).unsqueeze(1), values[(gr.group_ptr[:-1] + lv - 1).clamp(min=0, max=G - 1)], start)
            order = torch.cat([order, order.new_zeros(1)])
            values = torch.cat([values, values.new_zeros(1, values.shape[1])])
            order[at] = (torch.arange(G, device=dev) - gr.group_ptr[ggraph]).to(torch.int32)
            values[at] = lastv[ggraph]
            order, values = order[:G], values[:G]
        return GreedyResult(order.reshape(1, G), values, steps, gr.group_ptr, out_full, out_base)

    # ------------------------------------------------------------------ the call
    def __call__(self, batch, node_group=None, edge_group=None, class_index: int = 0, mode: str = "insertion", direction: int = 1,
                 steps: Optional[int] = None, ids_per_job: Optional[int] = None) -> GreedyResult:
        why = self._shape_args(self._args, batch)
        cls, deletion, sgn, steps = self._check(class_index, mode, direction, steps, ids_per_job)
        gr, ggraph, counts, lives, rounds = self._layout(batch, node_group, edge_group, steps)
        if why is not None or gr.max_groups > MAX_SUBSET_GROUPS:
            return self._loop(batch, gr, ggraph, counts, lives, rounds, cls, deletion, sgn)
        a = self._args
        x = _frozen.batch_x(batch)
        B, C, G, dev = a.B, a.C, gr.G, x.device
        ipj = self.default_ids_per_job(sum(lives)) if ids_per_job is None else int(ids_per_job)
        jobs, lptr = greedy_jobs(counts, rounds, ipj)
        order = self._bufs.take("order", (G,), dev, torch.int32)
        values = self._bufs.take("values", (G, C), dev)
        cand = self._bufs.take("cand", (2, G, C), dev)
        out = self._bufs.take("out", (2, B, C), dev)
        order.fill_(-1)
        values.zero_()
        self.last_path, self.launches = "fused", len(lptr) - 1
        if B > 0:
            member_group = _groups._member_group(gr, ggraph)
            jobs_t = jobs.to(dev)
            _frozen.query(a, self.KERNEL, self._shape(), batch, sub_max_groups=gr.max_groups)
            self._fill(a, 0, batch, x, self._weights(dev))
            p = _lib.ptr
            keep = _groups.fill_lists(a, gr, member_group)                  # noqa: F841  (alive until the launches are enqueued)
            a.sub_max_groups = gr.max_groups
            a.coal_values, a.coal_jobs = _frozen.front(values), p(jobs_t)
            a.greedy_order, a.greedy_cand = _frozen.front(order), _frozen.front(cand)
            a.out, a.out_base = p(out[0]), p(out[1])
            a.class_index = cls
            a.greedy_flags = (_lib.HCG_GREEDY_DELETION if deletion else 0) | (_lib.HCG_GREEDY_NEGATE if sgn < 0 else 0)
            stream = _lib.stream_ptr()
            for k in range(self.launches):                                  # one launch per round: the round's whole job range
                a.greedy_round, n = k, lptr[k + 1] - lptr[k]
                _frozen.launch_jobs(a, lptr[k], n, max(n, 1), "hcg_explain (greedy)", stream)
        return self._finish(gr, ggraph, counts, lives, rounds, deletion, order.clone(), values.clone(), out[0].clone(), out[1].clone())

    def loop(self, batch, node_group=None, edge_group=None, class_index: int = 0, mode: str = "insertion", direction: int = 1,
             steps: Optional[int] = None, ids_per_job: Optional[int] = None) -> GreedyResult:
        """One `SubsetValues` table per round (see the class docstring), whatever `reason(batch)` says."""
        cls, deletion, sgn, steps = self._check(class_index, mode, direction, steps, ids_per_job)
        gr, ggraph, counts, lives, rounds = self._layout(batch, node_group, edge_group, steps)
        return self._loop(batch, gr, ggraph, counts, lives, rounds, cls, deletion, sgn)

    def _loop(self, batch, gr, ggraph, counts, lives, rounds, cls, deletion, sgn) -> GreedyResult:
        sv = self.values
        B, G, C, dev = len(counts), gr.G, int(self.model._n_classes), batch.x.device
        order = torch.full((G,), -1, dtype=torch.int32, device=dev)
        values = torch.zeros(G, C, dtype=torch.float32, device=dev)
        onset = torch.full((G,), deletion, dtype=torch.bool, device=dev)
        picked = torch.zeros(G, dtype=torch.bool, device=dev)
        y = torch.arange(G, device=dev) - gr.group_ptr[ggraph]              # the group's local id
        R = torch.tensor(rounds, dtype=torch.int64, device=dev)
        out_full = out_base = None
        for k in range(max(rounds, default=0) + 1):
            # the candidates of round k and their index among their graph's candidates = their row of the table
            cand = gr.live_group & ~picked & (R[ggraph] > k) if G > 0 else picked
            rank = _groups._flag_ranks(ggraph, B, cand).rank
            rp = [lv - k if k < r else 0 for lv, r in zip(lives, rounds)]
            S = max(rp, default=0)
            if S == 0 and out_full is not None:
                break
            rows = onset.unsqueeze(0) ^ (cand.unsqueeze(0) & (rank.unsqueeze(0) == torch.arange(S, device=dev).unsqueeze(1)))
            table = sv._table(batch, gr, counts, rows, rp, None, sv._shape_args(sv._args, batch))
            if out_full is None:
                out_full, out_base = table[S].clone(), table[S + 1].clone()
            if S == 0:
                break
            # the pick: the greatest key, then the lower id; NaN = -inf
            val = table[rank.clamp(max=S - 1), ggraph]                      # [G, C] (read where `cand`)
            key = sgn * val[:, cls]
            key = torch.where(cand & ~torch.isnan(key), key, torch.full_like(key, float("-inf")))
            best = torch.full((B,), float("-inf"), dtype=torch.float32, device=dev).scatter_reduce(0, ggraph, key, reduce="amax")
            pick = torch.full((B,), G, dtype=torch.int64, device=dev).scatter_reduce(
                0, ggraph, torch.where(cand & (key == best[ggraph]), y, torch.full_like(y, G)), reduce="amin")
            won = cand & (y == pick[ggraph])
            at = (gr.group_ptr[:-1] + k)[ggraph[won]]
            order[at] = y[won].to(torch.int32)
            values[at] = val[won]
            onset = onset ^ won
            picked = picked | won
        self.last_path = "loop"
        return self._finish(gr, ggraph, counts, lives, rounds, deletion, order, values, out_full, out_base)
