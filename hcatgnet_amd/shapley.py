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

Groups as players (Captum's `feature_mask`, PyG's mask type None): with `node_group` / `edge_group` the features of a graph
are partitioned into groups -- an atom, a bond, a fragment -- that are switched on together and share one attribution, plus
a background that is always on.  The same kernel walks them (`HCG_EXPLAIN_GROUPED`): a step applies every live member of
its group and is evaluated once.  `atom_groups`, `bond_groups`, `draw_group_permutations` and `all_group_permutations`
build the usual arguments.

Coalition values: `CoalitionValues` evaluates EVERY subset of a graph's groups once (2^G states where all G! orders cost
G G! evaluations; up to 16 groups) with a second kernel of csrc/shapley.hip that shares the walk's build, application and
evaluation (`HCG_EXPLAIN_COALITIONS`).  Exact Shapley values and pairwise Shapley interaction indices are fixed linear forms
of that table: `shapley_from_coalitions`, `interactions_from_coalitions`.
"""
from __future__ import annotations

import ctypes
import itertools
import math
from typing import NamedTuple, Optional

import torch

from . import _frozen, _groups, _lib
from ._frozen import CUS, LAUNCH_SECONDS  # noqa: F401  (their home; importable from here as before)
from ._groups import (GROUPED_WORKGROUPS_PER_CU, MAX_WORKGROUPS_PER_CU, GroupedShapleyResult, ShapleyResult,  # noqa: F401  (as before)
                      _counts, _draw_segments, _group_layout, _layout, _players)

WORKSPACE_CAP_BYTES = 256 << 20    # the per-permutation rows of one launch
EVAL_SECONDS = 60e-6               # one evaluation at the shape limits: an estimate (default_samples_per_launch)


def draw_permutations(batch, F: int, n_samples: int, generator: Optional[torch.Generator] = None) -> torch.Tensor:
    """int32 [n_samples, N * F + E] on the batch's device: in every row, graph g's segment (start graph_ptr[g] * F +
    edge_ptr[g], length K_g = n_g * F + e_g) is a uniformly random permutation of 0 .. K_g - 1, drawn from `generator`
    (on the generator's device; None: the default generator of the batch's device) as the argsort of (graph id, key)."""
    n, e, _, _, seg = _layout(batch, F)
    return _draw_segments(n * F + e, seg, int(batch.batch.numel()) * F + int(batch.edge_index.shape[1]), n_samples, generator,
                          batch.x.device)


def atom_groups(batch) -> torch.Tensor:
    """`node_group` [N] int64 with one player per atom: the node's index inside its graph."""
    B = int(batch.num_graphs)
    gptr = torch.zeros(B + 1, dtype=torch.int64, device=batch.batch.device)
    gptr[1:] = torch.bincount(batch.batch, minlength=B).cumsum(0)
    return torch.arange(batch.batch.numel(), device=batch.batch.device) - gptr[batch.batch]


def bond_groups(batch, first=0) -> torch.Tensor:
    """`edge_group` [E] int64 that pairs (i, j) with (j, i) inside a graph: ids ascend by first occurrence in the batch's
    edge order and start at `first` in every graph (`first` may be a [B] tensor: bonds numbered after atoms).  An unpaired
    directed edge is a group of its own, every duplicate of a directed edge joins its pair's group, an explicit (i, i) gets
    a group that is simply dead."""
    ei, dev = batch.edge_index, batch.edge_index.device
    E, B, N = int(ei.shape[1]), int(batch.num_graphs), int(batch.batch.numel())
    first = torch.as_tensor(first, dtype=torch.int64, device=dev)
    if first.dim() > 1 or (first.dim() == 1 and first.numel() != B):
        raise ValueError(f"first must be an integer or a [B = {B}] tensor; got shape {tuple(first.shape)}")
    if E == 0:
        return torch.zeros(0, dtype=torch.int64, device=dev)
    lo, hi = torch.minimum(ei[0], ei[1]), torch.maximum(ei[0], ei[1])
    graph = batch.batch[ei[1]]
    _, inv = torch.unique(lo * max(N, 1) + hi, return_inverse=True)              # one id per undirected bond
    U = int(inv.max()) + 1
    pos = torch.full((U,), E, dtype=torch.int64, device=dev).scatter_reduce(0, inv, torch.arange(E, device=dev), reduce="amin")
    bond_graph = torch.zeros(U, dtype=torch.int64, device=dev).scatter(0, inv, graph)
    rank = torch.empty(U, dtype=torch.int64, device=dev)
    rank[torch.argsort(bond_graph * E + pos)] = torch.arange(U, device=dev)      # graph by graph, by first occurrence
    start = torch.zeros(B + 1, dtype=torch.int64, device=dev)
    start[1:] = torch.bincount(bond_graph, minlength=B).cumsum(0)
    return rank[inv] - start[graph] + (first[graph] if first.dim() == 1 else first)


def draw_group_permutations(batch, node_group=None, edge_group=None, n_samples: int = 25,
                            generator: Optional[torch.Generator] = None) -> torch.Tensor:
    """int32 [n_samples, G] on the batch's device: in every row, graph g's segment (start group_ptr[g], length G_g) is a
    uniformly random permutation of 0 .. G_g - 1, drawn as `draw_permutations` draws: the argsort of (graph id, key)."""
    gr = _group_layout(batch, int(batch.x.shape[1]), node_group, edge_group)
    return _draw_segments(gr.count, gr.group_ptr, gr.G, n_samples, generator, batch.x.device)


def all_group_permutations(batch, node_group=None, edge_group=None) -> torch.Tensor:
    """int32 [G_g!, G]: every order of the groups, for a batch whose graphs all have the same G_g <= 6 (ValueError
    otherwise).  The mean over these rows is the exact Shapley value of the groups, at G_g * G_g! evaluations per graph;
    `CoalitionValues` gives the same values from the 2^G_g distinct states, for up to 16 groups, with the pairwise
    interaction indices."""
    gr = _group_layout(batch, int(batch.x.shape[1]), node_group, edge_group)
    counts = set(gr.count.tolist())
    if len(counts) > 1 or (counts and max(counts) > 6):
        raise ValueError(f"all_group_permutations needs the same number of groups <= 6 in every graph; got {sorted(counts)}")
    g0 = counts.pop() if counts else 0
    rows = torch.tensor(list(itertools.permutations(range(g0))), dtype=torch.int32).reshape(-1, g0)
    return rows.repeat(1, gr.count.numel()).to(batch.x.device).contiguous()


class ShapleySampling(_frozen.FrozenModel):
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
    ran ("fused" / "loop").

    Groups as players (Captum's `feature_mask`, baselines 0):

        r = sv(batch, n_samples=25, node_group=atom_groups(batch), edge_group=None, group_permutations=None, ...)
        # GroupedShapleyResult(group_attr [G], group_ptr [B + 1], node_attr [N, F], edge_attr [E], out_full, out_base)

    `node_group`: integer tensor [N] (all F entries of a node share the id) or [N, F]; `edge_group`: integer tensor [E].
    Ids are local to the graph: over both arrays a graph uses exactly 0 .. G_g - 1, each at least once (else ValueError),
    and -1 for the background, which is never a player: it is on in every evaluation, the base included.  Giving one
    array puts the other kind wholly in the background.  For permutation pi of graph g's groups, v_0 is the output with
    the background only, v_k with the groups pi_1 .. pi_k on as well, and group pi_k gets v_k[c] - v_(k-1)[c]; the mean
    over the permutations, p ascending, is `group_attr`.  A group without a live member (a node entry with x != 0, an
    edge that is no explicit (i, i)) gets exactly 0 and costs no evaluation.  `node_attr` / `edge_attr` follow Captum:
    every member carries its group's value, the background 0.  `group_permutations`: int32 [P, G], graph g's segment at
    group_ptr[g] (`draw_group_permutations`, `all_group_permutations`); None: `n_samples` rows from `generator`.
    `permutations` belongs to the ungrouped call.  With neither array given the call is the ungrouped one, unchanged.
    The host checks the ids and lists the members with torch ops: one stable sort and one read of three scalars."""

    KERNEL, NAME = _lib.HCG_EXPLAIN_SHAPLEY, "ShapleySampling"

    @staticmethod
    def default_samples_per_launch(n_perm: int, num_graphs: int, row: int, max_steps: int = 0,
                                   max_per_cu: int = MAX_WORKGROUPS_PER_CU) -> int:
        """Permutations of one launch: as many as keep its workspace (4 * row bytes each) under `WORKSPACE_CAP_BYTES` and
        its run time near `LAUNCH_SECONDS`, at least 1.  `max_steps` = max_nodes * F + max_edges (a grouped call: the
        largest G_g) bounds the evaluations of one workgroup (every step evaluated: dense features); at `EVAL_SECONDS` each, a CU gets as many workgroups as fit
        the time, at least one.  `EVAL_SECONDS` is an ESTIMATE: profiles/shapley_bench.json has about 15-20 us per
        evaluation at two conv layers and 122-node graphs (36 ms per launch of 535 workgroups of about 860 evaluations),
        extrapolated to the 184-node, four-layer limit; nobody has timed a launch at the limit shapes.  `max_per_cu` caps
        the workgroups a CU gets in one launch (a grouped call: `GROUPED_WORKGROUPS_PER_CU`)."""
        by_ws = WORKSPACE_CAP_BYTES // max(4 * int(row), 1)
        per_cu = max(1, int(LAUNCH_SECONDS / (max(int(max_steps), 1) * EVAL_SECONDS)))
        by_wg = min(per_cu, int(max_per_cu)) * CUS // max(int(num_graphs), 1)
        return max(1, min(int(n_perm), by_ws, by_wg, 65535))

    # ------------------------------------------------------------------ the call
    def __call__(self, batch, n_samples: int = 25, permutations=None, generator=None, class_index: int = 0,
                 samples_per_launch: Optional[int] = None, node_group=None, edge_group=None, group_permutations=None):
        pl, given = _players(batch, permutations, node_group, edge_group, group_permutations)
        a = self._args
        if self._shape_args(a, batch, perm_count=1, **pl.query) is not None:
            return self._walk(pl, pl.permutations(n_samples, given, generator), class_index)
        x = _frozen.batch_x(batch)
        B, C, dev = a.B, a.C, x.device
        cls = self._class(class_index)
        perm = pl.permutations(n_samples, given, generator)
        P = int(perm.shape[0])
        spl = self.default_samples_per_launch(P, B, pl.row, pl.max_steps(a), pl.per_cu) if samples_per_launch is None \
            else int(samples_per_launch)
        if not 1 <= spl <= 65535:
            raise ValueError(f"samples_per_launch must lie in 1 .. 65535; got {samples_per_launch}")
        spl = min(spl, P)
        # the workspace of a launch of `spl` permutations (model and batch are checked: the library's query alone)
        _frozen.query(a, self.KERNEL, self._shape(), batch, perm_count=spl, **pl.query)
        take, front = self._bufs.take, _frozen.front
        acc, out, base = take("acc", (pl.row,), dev), take("out", (B, C), dev), take("base", (B, C), dev)
        self._fill(a, pl.flags, batch, x, self._weights(dev), self._bufs.workspace(int(a.workspace_bytes_needed), dev))
        a.out, a.out_base, a.shap_acc, a.perm = front(out), front(base), front(acc), _lib.ptr(perm)
        a.n_perm, a.class_index = P, cls
        pl.fill(a)
        lib, stream = _lib.load(), _lib.stream_ptr()
        for first in range(0, P, spl):
            a.perm_first, a.perm_count = first, min(spl, P - first)
            _lib.check(lib.hcg_explain(ctypes.addressof(a), stream), pl.label)
        self.last_path = "fused"
        return pl.result(acc, out, base)

    # ------------------------------------------------------------------ the existing path (any shape): one forward per step
    def loop(self, batch, n_samples: int = 25, permutations=None, generator=None, class_index: int = 0, node_group=None,
             edge_group=None, group_permutations=None):
        """The batch-synchronous loop (see the class docstring), whatever `reason(batch)` says."""
        pl, given = _players(batch, permutations, node_group, edge_group, group_permutations)
        return self._walk(pl, pl.permutations(n_samples, given, generator), class_index)

    def _walk(self, pl: _groups._Players, perm, class_index):
        """Step k switches on the k-th player of every graph's permutation: a feature, or every member of a group (what no
        group holds, the background, is on from the base on)."""
        batch, N, F, B, row = pl.batch, pl.N, pl.F, pl.B, pl.row
        w = pl.walk()
        perm = perm.to(torch.int64)
        P, dev = int(perm.shape[0]), batch.x.device
        garange = torch.arange(B, device=dev)
        background = (w.owner == row).to(torch.float32)
        acc = torch.zeros(row, dtype=torch.float32, device=dev)
        out_full = out_base = None
        with torch.no_grad():
            for p in range(P):
                on = background.clone()
                phi = torch.zeros(row, dtype=torch.float32, device=dev)
                out = self._masked_forward(batch, on[:N * F].view(N, F), on[N * F:]).reshape(B, -1).clone()
                if p == 0:
                    out_base = out
                vprev = out[:, class_index].clone()
                for k in range(w.steps):
                    act = garange[w.count > k]                            # graphs whose walk is not finished
                    slot = w.place(act, perm[p, w.start[act] + k])
                    step = torch.zeros(row + 1, dtype=torch.bool, device=dev)
                    step[slot] = True
                    on = torch.where(step[w.owner], torch.ones_like(on), on)
                    out = self._masked_forward(batch, on[:N * F].view(N, F), on[N * F:]).reshape(B, -1).clone()
                    v = out[:, class_index]
                    phi[slot] = torch.where(w.live[slot], v[act] - vprev[act], torch.zeros_like(v[act]))
                    vprev = v.clone()
                if p == 0:
                    out_full = out
                acc = acc + phi
        acc = acc / float(P)
        self.last_path = "loop"
        return pl.result(acc, out_full, out_base)


# ====================================================================== coalition values: every subset of a graph's groups
MAX_COALITION_GROUPS = 16          # groups of one graph: 2^16 rows
SUBSETS_PER_WORKGROUP = 16         # the longest run of masks one workgroup evaluates (`default_subsets_per_workgroup`)


class CoalitionResult(NamedTuple):
    values: torch.Tensor         # [T, C]: values[table_ptr[g] + s] = the output with the background and the groups {y : bit y of s} on
    table_ptr: torch.Tensor      # [B + 1] int64, T = sum_g 2^G_g
    group_ptr: torch.Tensor      # [B + 1] int64
    group_attr: torch.Tensor     # [G] the exact Shapley value of every group for `class_index`
    interaction: torch.Tensor    # [Q] graph g's G_g x G_g Shapley interaction indices, row-major at pair_ptr[g]
    pair_ptr: torch.Tensor       # [B + 1] int64, Q = sum_g G_g^2
    out_full: torch.Tensor       # [B, C] everything on: row 2^G_g - 1 of the graph
    out_base: torch.Tensor       # [B, C] the background only: row 0


def _popcount(t: torch.Tensor, bits: int) -> torch.Tensor:
    size = torch.zeros_like(t)
    for y in range(bits):
        size += (t >> y) & 1
    return size


def _spread(t: torch.Tensor, at: int) -> torch.Tensor:
    """`t` with a 0 bit inserted at position `at`"""
    return ((t >> at) << (at + 1)) | (t & ((1 << at) - 1))


def _by_count(counts: list):
    """distinct G_g > 0 -> the graphs that have it, ascending"""
    by = {}
    for g, c in enumerate(counts):
        if c > 0:
            by.setdefault(c, []).append(g)
    return sorted(by.items())


def _tables(values, table_ptr, graphs: list, Gv: int, class_index: int) -> torch.Tensor:
    """float64 [len(graphs), 2^Gv]: column `class_index` of the tables of `graphs`, which all have Gv groups"""
    dev = values.device
    first = table_ptr[torch.tensor(graphs, dtype=torch.int64, device=dev)]
    return values[:, class_index][first.unsqueeze(1) + torch.arange(1 << Gv, device=dev)].to(torch.float64)


def _check_table(values, table_ptr, group_ptr, class_index):
    if values.dim() != 2 or not 0 <= int(class_index) < values.shape[1]:
        raise ValueError(f"values must be [T, C] and class_index lie in 0 .. C - 1; got {tuple(values.shape)}, {class_index}")
    if table_ptr.numel() != group_ptr.numel():
        raise ValueError("table_ptr and group_ptr must both be [B + 1]")


def _shapley_of(values, table_ptr, counts: list, class_index: int) -> torch.Tensor:
    dev = values.device
    gptr = [0]
    for c in counts:
        gptr.append(gptr[-1] + c)
    phi = torch.zeros(gptr[-1], dtype=torch.float64, device=dev)
    for Gv, graphs in _by_count(counts):
        V = _tables(values, table_ptr, graphs, Gv, class_index)
        rest = torch.arange(1 << (Gv - 1), device=dev)                     # the subsets of the other groups, packed
        size = _popcount(rest, Gv - 1)
        fact = [math.factorial(k) for k in range(Gv + 1)]
        w = torch.tensor([fact[k] * fact[Gv - k - 1] / fact[Gv] for k in range(Gv)], dtype=torch.float64, device=dev)[size]
        at = torch.tensor([gptr[g] for g in graphs], dtype=torch.int64, device=dev)
        for y in range(Gv):
            S = _spread(rest, y)
            # (the difference first: a group whose rows repeat the rows without it gets exactly 0)
            phi[at + y] = ((V[:, S | (1 << y)] - V[:, S]) * w).sum(1)
    return phi.to(torch.float32)


def _interactions_of(values, table_ptr, counts: list, class_index: int):
    dev = values.device
    pptr = [0]
    for c in counts:
        pptr.append(pptr[-1] + c * c)
    out = torch.zeros(pptr[-1], dtype=torch.float64, device=dev)
    for Gv, graphs in _by_count(counts):
        if Gv < 2:
            continue
        V = _tables(values, table_ptr, graphs, Gv, class_index)
        rest = torch.arange(1 << (Gv - 2), device=dev)
        size = _popcount(rest, Gv - 2)
        fact = [math.factorial(k) for k in range(Gv + 1)]
        w = torch.tensor([fact[k] * fact[Gv - k - 2] / fact[Gv - 1] for k in range(Gv - 1)], dtype=torch.float64, device=dev)[size]
        at = torch.tensor([pptr[g] for g in graphs], dtype=torch.int64, device=dev)
        for i in range(Gv):
            for j in range(i + 1, Gv):
                S = _spread(_spread(rest, i), j)                           # (i < j: the lower bit goes in first)
                bi, bj = 1 << i, 1 << j
                # (the differences of rows that repeat each other first: a dead group's row and column are exactly 0)
                d = (V[:, S | bi | bj] - V[:, S | bj]) - (V[:, S | bi] - V[:, S])
                val = (d * w).sum(1)
                out[at + i * Gv + j] = val
                out[at + j * Gv + i] = val
    return out.to(torch.float32), torch.tensor(pptr, dtype=torch.int64, device=dev)


def shapley_from_coalitions(values, table_ptr, group_ptr, class_index: int = 0) -> torch.Tensor:
    """float32 [G]: the exact Shapley value of every group for output column `class_index`, from a table of coalition
    values (`CoalitionResult.values`, `.table_ptr`, `.group_ptr`):
        phi_y = sum over S not containing y of |S|! (G - |S| - 1)! / G! (v(S + y) - v(S)).
    Formed in float64 on the table's device, vectorised over the graphs that share a G_g (a loop over the groups, none
    over the subsets), rounded to float32.  One host read: `group_ptr`."""
    _check_table(values, table_ptr, group_ptr, class_index)
    return _shapley_of(values, table_ptr, _counts(group_ptr), int(class_index))


def interactions_from_coalitions(values, table_ptr, group_ptr, class_index: int = 0):
    """-> (float32 [Q], pair_ptr [B + 1] int64): graph g's G_g x G_g matrix of Shapley interaction indices (Grabisch and
    Roubens), row-major at pair_ptr[g], symmetric, 0 on the diagonal:
        I_ij = sum over S within the others of |S|! (G - |S| - 2)! / (G - 1)! (v(S+i+j) - v(S+i) - v(S+j) + v(S)).
    Formed as `shapley_from_coalitions` forms its values (a loop over the pairs of groups, none over the subsets)."""
    _check_table(values, table_ptr, group_ptr, class_index)
    return _interactions_of(values, table_ptr, _counts(group_ptr), int(class_index))


class CoalitionValues(_frozen.FrozenModel):
    """The model's output for EVERY subset of each graph's groups, and what follows from that table.

        cv = CoalitionValues(model)
        r = cv(batch, node_group=None, edge_group=None, class_index=0, subsets_per_workgroup=None)
        # CoalitionResult(values [T, C], table_ptr [B + 1], group_ptr [B + 1], group_attr [G], interaction [Q],
        #                 pair_ptr [B + 1], out_full [B, C], out_base [B, C])

    `node_group` / `edge_group` are `ShapleySampling`'s: local ids 0 .. G_g - 1, -1 for the background, the same checks and
    errors.  A graph may have up to `MAX_COALITION_GROUPS` = 16 groups (ValueError before any launch otherwise), and the
    table must fit `attribution.LAUNCH_BUDGET_BYTES` (ValueError: split the batch).  `values[table_ptr[g] + s]` is the
    output [C] with the background and the groups {y : bit y of s} on, T = sum_g 2^G_g; row 0 is `out_base[g]`, row
    2^G_g - 1 `out_full[g]`; a graph without groups has one row.  That is 2^G evaluations where all G! orders cost G G!,
    and exact for up to 16 groups where `all_group_permutations` stops at 6.

    `group_attr` is the exact Shapley value of every group for `class_index` and `interaction` the pairwise Shapley
    interaction index (`shapley_from_coalitions`, `interactions_from_coalitions`: fixed linear forms of the table, formed
    in float64 by torch ops; call them on `values` for another class without a second launch).

    One workgroup evaluates a run of up to `subsets_per_workgroup` consecutive masks of one graph on chip
    (csrc/shapley.hip, k_coalition_values): it builds the graph once and rebuilds the state from zero for every mask, so
    every row is bitwise independent of the run length, of the launch split, of the run and of the rest of the batch, and
    row 2^(y + 1) - 1 is bitwise what `ShapleySampling` evaluates after group y in the identity order.  A group without a
    live member is not sent to the kernel: the kernel runs over the 2^L_g masks of the graph's live groups and the host
    expands to [T, C] with one gather, so rows that differ only in dead groups are the same row, and a dead group's
    Shapley value and interactions are exactly 0.  None for `subsets_per_workgroup`: `default_subsets_per_workgroup`.  Jobs
    are split into launches by the estimate `ShapleySampling.default_samples_per_launch` uses (`jobs_per_launch`; set the
    attribute to force a split).

    Host reads, once per call each: what `_group_layout` reads (three scalars), and the per-graph group counts and live
    counts, which give T, T_live and the job list.  `shapley_from_coalitions` called on its own reads `group_ptr`.

    When `reason(batch)` is not None (shape outside the kernel, CPU tensors, `use_fused` off) the same call runs `loop`:
    mask index s ascends, every graph with s < 2^G_g is switched to subset s and one masked forward of the whole batch
    follows (forward-only `ExplainStep` on GPU tensors, plain torch ops on CPU tensors).  `last_path` says which one ran.
    The returned tensors are new on the loop path; on the fused path `values`, `out_full` and `out_base` are new and the
    kernel's own live table is a pool buffer."""

    KERNEL, NAME = _lib.HCG_EXPLAIN_COALITIONS, "CoalitionValues"
    jobs_per_launch: Optional[int] = None          # None: `default_jobs_per_launch`

    @staticmethod
    def default_subsets_per_workgroup(live_rows: int) -> int:
        """Masks per workgroup: up to `SUBSETS_PER_WORKGROUP` = 16, which spreads the graph's build (about the cost of one
        evaluation) over 16 of them, but no more than leaves four workgroups for every CU -- a single graph of 10 groups
        runs one mask per workgroup, 535 graphs of 6 groups run 16."""
        return max(1, min(SUBSETS_PER_WORKGROUP, int(live_rows) // (4 * CUS)))

    @staticmethod
    def default_jobs_per_launch(subsets_per_workgroup: int) -> int:
        """Workgroups of one launch by `default_samples_per_launch`'s estimate: a CU gets as many as fit `LAUNCH_SECONDS` at
        `EVAL_SECONDS` per mask (the rebuild is counted as part of the evaluation: nobody has timed it apart), at most
        `GROUPED_WORKGROUPS_PER_CU`."""
        per_cu = max(1, int(LAUNCH_SECONDS / (max(int(subsets_per_workgroup), 1) * EVAL_SECONDS)))
        return min(per_cu, GROUPED_WORKGROUPS_PER_CU) * CUS

    # ------------------------------------------------------------------ what both paths share
    def _layout(self, batch, node_group, edge_group):
        """-> (the group layout, per-graph counts, per-graph live counts, live_group's rank inside its graph [G]); the
        limits checked.  One host read beside `_group_layout`'s."""
        F, B = int(batch.x.shape[1]), int(batch.num_graphs)
        gr = _group_layout(batch, F, node_group, edge_group)
        if gr.max_groups > MAX_COALITION_GROUPS:
            raise ValueError(f"a graph has {gr.max_groups} groups; CoalitionValues takes at most {MAX_COALITION_GROUPS} "
                             f"(2^{MAX_COALITION_GROUPS} rows per graph)")
        ggraph = _groups._group_graph(gr.count, gr.G)
        live = _groups._flag_ranks(ggraph, B, gr.live_group)               # (rank: a live group's index among its graph's live groups)
        counts, lives = torch.stack([gr.count, live.per_graph]).tolist() if B > 0 else ([], [])
        C = int(self.model._n_classes)
        T = sum(1 << c for c in counts)
        from . import attribution
        if T * C * 4 > attribution.LAUNCH_BUDGET_BYTES:
            raise ValueError(f"the table of this batch has {T} rows of {C} outputs, {T * C * 4} bytes, above "
                             f"LAUNCH_BUDGET_BYTES = {attribution.LAUNCH_BUDGET_BYTES}: split the batch")
        return gr, counts, lives, (ggraph, live.ptr, live.rank)

    @staticmethod
    def _expand(gr, counts, lives, aux, dev):
        """-> (table_ptr [B + 1], live_ptr [B + 1], index [T] int64): row table_ptr[g] + s of the full table is row
        index[.] = live_ptr[g] + (the live bits of s, packed) of the live table."""
        ggraph, lptr, rank = aux
        B = len(counts)
        rows = torch.tensor([1 << c for c in counts], dtype=torch.int64, device=dev)
        tptr = torch.zeros(B + 1, dtype=torch.int64, device=dev)
        tptr[1:] = rows.cumsum(0)
        vptr = torch.zeros(B + 1, dtype=torch.int64, device=dev)
        vptr[1:] = torch.tensor([1 << c for c in lives], dtype=torch.int64, device=dev).cumsum(0)
        T = sum(1 << c for c in counts)
        g = torch.repeat_interleave(torch.arange(B, device=dev), rows, output_size=T)
        s = torch.arange(T, device=dev) - tptr[g]
        packed = torch.zeros(T, dtype=torch.int64, device=dev)
        if gr.G > 0:
            for y in range(max(counts)):
                has = (gr.count[g] > y) & (((s >> y) & 1) == 1)
                at = torch.where(has, gr.group_ptr[g] + y, torch.zeros_like(s))
                packed += torch.where(has & gr.live_group[at], torch.ones_like(s) << rank[at], torch.zeros_like(s))
        return tptr, vptr, vptr[g] + packed

    def _result(self, values, tptr, gr, counts, cls) -> CoalitionResult:
        attr = _shapley_of(values, tptr, counts, cls)
        inter, pptr = _interactions_of(values, tptr, counts, cls)
        return CoalitionResult(values, tptr, gr.group_ptr, attr, inter, pptr, values[tptr[1:] - 1], values[tptr[:-1]])

    # ------------------------------------------------------------------ the call
    def __call__(self, batch, node_group=None, edge_group=None, class_index: int = 0, subsets_per_workgroup: Optional[int] = None):
        a = self._args
        if self._shape_args(a, batch) is not None:
            return self.loop(batch, node_group, edge_group, class_index)
        x = _frozen.batch_x(batch)
        B, C, dev = a.B, a.C, x.device
        cls = self._class(class_index)
        gr, counts, lives, aux = self._layout(batch, node_group, edge_group)
        tptr, vptr, index = self._expand(gr, counts, lives, aux, dev)
        T_live = sum(1 << c for c in lives)
        spw = _frozen.positive("subsets_per_workgroup", subsets_per_workgroup) or self.default_subsets_per_workgroup(T_live)
        spw = min(spw, 1 << MAX_COALITION_GROUPS)
        # the jobs (graph, first mask, masks), built on the host from the live counts
        jobs = [(g, m, min(spw, (1 << c) - m)) for g, c in enumerate(lives) for m in range(0, 1 << c, spw)]
        J = len(jobs)
        jobs_t = torch.tensor(jobs, dtype=torch.int32).reshape(J, 3).to(dev)
        # the live groups' lists: a dead group's member range is empty, so dropping its pointer keeps the others' ranges
        keep = torch.cat([gr.live_group, torch.ones(1, dtype=torch.bool, device=dev)])
        member_ptr = gr.member_ptr[keep].contiguous()
        live_ptr32 = aux[1].to(torch.int32)
        table = self._bufs.take("table", (T_live, C), dev)
        self.last_path = "fused"
        if J == 0:                                                          # (no graph: nothing to launch)
            return self._result(table[index], tptr, gr, counts, cls)
        _frozen.query(a, self.KERNEL, self._shape(), batch, coal_rows=T_live, coal_max_live=max(lives))
        self._fill(a, 0, batch, x, self._weights(dev))
        _groups.fill_lists(a, gr, live=(live_ptr32, member_ptr))           # (both live in this frame until the launches are enqueued)
        a.coal_values, a.coal_jobs, a.coal_live_ptr = _frozen.front(table), _lib.ptr(jobs_t), _lib.ptr(vptr)
        a.coal_rows, a.coal_max_live = T_live, max(lives)
        jpl = _frozen.positive("jobs_per_launch", self.jobs_per_launch) or self.default_jobs_per_launch(spw)
        _frozen.launch_jobs(a, 0, J, jpl, "hcg_explain (coalitions)")
        return self._result(table[index], tptr, gr, counts, cls)

    # ------------------------------------------------------------------ the existing path (any shape): one forward per mask index
    def loop(self, batch, node_group=None, edge_group=None, class_index: int = 0):
        """The batch-synchronous loop (see the class docstring), whatever `reason(batch)` says."""
        (N, F), B, dev = batch.x.shape, int(batch.num_graphs), batch.x.device
        gr, counts, lives, aux = self._layout(batch, node_group, edge_group)
        C = int(self.model._n_classes)
        if not 0 <= int(class_index) < C:
            raise ValueError(f"class_index must lie in 0 .. {C - 1}; got {class_index}")
        tptr, vptr, index = self._expand(gr, counts, lives, aux, dev)
        ggraph = aux[0]
        # the feature's bit: its group's local id (the background: always on)
        local = torch.cat([torch.arange(gr.G, device=dev) - gr.group_ptr[ggraph], torch.zeros(1, dtype=torch.int64, device=dev)])[gr.slot]
        background = gr.slot == gr.G
        T = sum(1 << c for c in counts)
        raw = torch.zeros(T, C, dtype=torch.float32, device=dev)
        with torch.no_grad():
            for s in range(1 << max(counts)) if B > 0 else ():
                on = (background | (((torch.full_like(local, s) >> local) & 1) == 1)).to(torch.float32)
                out = self._masked_forward(batch, on[:N * F].view(N, F), on[N * F:]).reshape(B, -1)
                act = (torch.ones_like(gr.count) << gr.count) > s
                raw[tptr[:-1][act] + s] = out[act].to(torch.float32)
        # the rows of the live table, read back through the same gather as the fused path's: a row stands for every row
        # that differs from it in dead groups only (its own dead bits cleared)
        canon = torch.zeros(sum(1 << c for c in lives), dtype=torch.int64, device=dev)
        canon.scatter_reduce_(0, index, torch.arange(T, device=dev), reduce="amin", include_self=False)
        self.last_path = "loop"
        return self._result(raw[canon[index]], tptr, gr, counts, int(class_index))
