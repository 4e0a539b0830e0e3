"""The players of a batch: what the Shapley family (`ShapleySampling`, `CoalitionValues`, `SubsetValues`, `AttributionCurves`,
`GreedySelection` and the ensemble classes of ensemble_shapley.py) shares about features, groups of features and subsets of
groups, whatever the model is.

    _layout, _draw_segments      graph_ptr / edge_ptr of a batch and the permutation rows drawn over its segments
    _Groups, _group_layout       `node_group` / `edge_group` checked and turned into the lists the kernels read
    _group_graph, _counts        the graph of every group; the per-graph counts of a prefix sum on the host
    _flag_counts, _flag_ranks    per graph: how many groups carry a flag (live, dead, candidate), the prefix sum, and a flagged
                                 group's rank among its graph's flagged groups
    _member_group, _pack         the local group id of every listed member; bool rows -> the bit words the kernels read
    fill_lists                   THE place that hands the group lists to the library (`shap_` members, `sub_member_group`)
    _Players, _Features, _GroupPlayers, _players     the players of a Shapley walk: features, or groups of them
    subset_layout, check_subsets, _SubsetCall        the part of a subset call that does not depend on the model

Private: the classes are the interface.  The public helpers stay where they are exported (shapley.py, subsets.py).
"""
from __future__ import annotations

from typing import NamedTuple, Optional

import torch

from . import _lib

MAX_WORKGROUPS_PER_CU = 4
GROUPED_WORKGROUPS_PER_CU = 64     # a grouped walk is short (its steps are the groups): more of them queue on a CU per launch


class ShapleyResult(NamedTuple):
    node_attr: torch.Tensor      # [N, F]
    edge_attr: torch.Tensor      # [E], the batch's edge order
    out_full: torch.Tensor       # [B, C] the model's output with every feature on (= the plain forward)
    out_base: torch.Tensor       # [B, C] with every feature off


class GroupedShapleyResult(NamedTuple):
    group_attr: torch.Tensor     # [G] graph g's groups at group_ptr[g] .. group_ptr[g + 1] - 1
    group_ptr: torch.Tensor      # [B + 1] int64
    node_attr: torch.Tensor      # [N, F] every member carries its group's value, the background 0 (a gather of group_attr)
    edge_attr: torch.Tensor      # [E]
    out_full: torch.Tensor       # [B, C] the model's output with everything on (= the plain forward)
    out_base: torch.Tensor       # [B, C] with the background only


# ====================================================================== the batch and its segments
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


def _draw_segments(count, start, total: int, n_samples: int, generator, dev) -> torch.Tensor:
    """int32 [n_samples, total]: in every row, segment g (start[g], length count[g]; the segments tile the row in order) is
    a uniformly random permutation of 0 .. count[g] - 1: the argsort of (segment id, key), one float64 key per entry and
    one `torch.rand` per row, on the generator's device (None: the default generator of `dev`)."""
    gid = torch.repeat_interleave(torch.arange(count.numel(), device=dev), count)
    first = start[gid]
    gdev = generator.device if generator is not None else dev
    out = torch.empty(int(n_samples), total, dtype=torch.int32, device=dev)
    for p in range(int(n_samples)):
        key = torch.rand(total, generator=generator, device=gdev, dtype=torch.float64).to(dev)
        order = torch.argsort(gid.to(torch.float64) + key)
        out[p] = (order - first).to(torch.int32)
    return out


# ====================================================================== groups of features
class _Groups(NamedTuple):
    """The group layout of one call (`_group_layout`); every tensor on the batch's device."""
    G: int                       # groups of the batch
    max_groups: int              # the largest G_g
    count: torch.Tensor          # [B] int64 G_g
    group_ptr: torch.Tensor      # [B + 1] int64
    slot: torch.Tensor           # [N * F + E] int64: the feature's global group (group_ptr[graph] + id), G for the background
    live_group: torch.Tensor     # [G] bool: the group has a live member
    member_ptr: torch.Tensor     # [G + 1] int32 into `members`
    bg_ptr: torch.Tensor         # [B + 1] int32 into `members`
    members: torch.Tensor        # [N * F + E] int32 local feature indices: the groups' live members, group by group,
    #                              then the graphs' live background, then the dead features


def _group_layout(batch, F: int, node_group, edge_group) -> _Groups:
    """Check `node_group` / `edge_group` and build the lists the kernel reads, with torch ops on the batch's device: one
    stable sort of all features by (group | graph of the background | dead) -- features are numbered graph by graph, node
    entries before edges, so equal keys stay in ascending local index -- and ONE read of three scalars (G, the largest G_g,
    whether the ids are valid) beside what `_layout` costs."""
    x, ei = batch.x, batch.edge_index
    N, E, B, dev = int(x.shape[0]), int(ei.shape[1]), int(batch.num_graphs), x.device

    def ids_of(t, name, shapes):
        if t is None:
            return None
        if not torch.is_tensor(t) or t.dtype not in (torch.int8, torch.int16, torch.int32, torch.int64) or tuple(t.shape) not in shapes:
            raise ValueError(f"{name} must be an integer tensor of shape {' or '.join(str(list(q)) for q in shapes)}; got "
                             f"{getattr(t, 'dtype', type(t))} {tuple(getattr(t, 'shape', ()))}")
        if t.device != dev:
            raise ValueError(f"{name} is on {t.device}, the batch on {dev}")
        return t.to(torch.int64)
    ng = ids_of(node_group, "node_group", ((N,), (N, F)))
    eg = ids_of(edge_group, "edge_group", ((E,),))
    if ng is None and eg is None:
        raise ValueError("give node_group, edge_group or both")
    ng = torch.full((N * F,), -1, dtype=torch.int64, device=dev) if ng is None else \
        (ng.unsqueeze(1).expand(N, F) if ng.dim() == 1 else ng).reshape(-1)
    eg = torch.full((E,), -1, dtype=torch.int64, device=dev) if eg is None else eg
    n, e, gptr, eptr, _ = _layout(batch, F)
    src, dst = ei[0], ei[1]
    egraph = batch.batch[dst]
    ids = torch.cat([ng, eg])
    graph = torch.cat([batch.batch.repeat_interleave(F), egraph])
    count = torch.zeros(B, dtype=torch.int64, device=dev).scatter_reduce(0, graph, ids + 1, reduce="amax", include_self=True)
    group_ptr = torch.zeros(B + 1, dtype=torch.int64, device=dev)
    group_ptr[1:] = count.cumsum(0)
    grouped = ids >= 0
    # (every group has a member, so valid ids have G <= N F + E: the used-slot table needs no size from the device, and a
    # slot beyond it -- ids with a gap -- lands on the spare entry and leaves the count short)
    used = torch.zeros(N * F + E + 1, dtype=torch.int64, device=dev)
    at = group_ptr[graph] + ids
    used[torch.where(grouped & (at < N * F + E), at, N * F + E)] = 1
    bad = (used[:-1].sum() != group_ptr[-1]) | (ids < -1).any()
    G, max_groups, bad = torch.stack([group_ptr[-1], count.max() if B > 0 else group_ptr[-1], bad.to(torch.int64)]).tolist()
    if bad:
        raise ValueError("the group ids of a graph, over node_group and edge_group, must be exactly 0 .. G_g - 1, each used "
                         "at least once, and -1 for the background")
    slot = torch.where(grouped, group_ptr[graph] + ids, G)
    local = torch.cat([((torch.arange(N, device=dev) - gptr[batch.batch]) * F).repeat_interleave(F) + torch.arange(F, device=dev).repeat(N),
                       n[egraph] * F + torch.arange(E, device=dev) - eptr[egraph]])
    live = torch.cat([(x != 0).reshape(-1), src != dst])
    key = torch.where(live, torch.where(grouped, slot, G + graph), G + B)
    order = torch.sort(key, stable=True).indices
    ptr = torch.zeros(G + B + 2, dtype=torch.int64, device=dev)
    ptr[1:] = torch.bincount(key, minlength=G + B + 1).cumsum(0)
    live_group = ptr[1:G + 1] > ptr[:G]
    return _Groups(int(G), int(max_groups), count, group_ptr, slot, live_group, ptr[:G + 1].to(torch.int32).contiguous(),
                   ptr[G:G + B + 1].to(torch.int32).contiguous(), local[order].to(torch.int32).contiguous())


def _counts(ptr) -> list:
    """Host list of the per-graph counts of a [B + 1] prefix sum (one read)."""
    p = ptr.tolist()
    return [b - a for a, b in zip(p[:-1], p[1:])]


def _group_graph(count: torch.Tensor, G: int) -> torch.Tensor:
    """[G] int64: the graph of every group"""
    return torch.repeat_interleave(torch.arange(count.numel(), device=count.device), count, output_size=G)


class _Ranks(NamedTuple):
    """`_flag_ranks`: the flagged groups (the live, the dead, a round's candidates) graph by graph"""
    per_graph: torch.Tensor      # [B] int64 flagged groups of every graph
    ptr: torch.Tensor            # [B + 1] int64 its prefix sum
    rank: torch.Tensor           # [G] int64: a flagged group's index among its graph's flagged groups (read where flagged)


def _flag_counts(ggraph: torch.Tensor, B: int, flag: torch.Tensor) -> torch.Tensor:
    """[B] int64: the groups of every graph that carry `flag` ([G] bool or int64 0 / 1); `ggraph`: `_group_graph`"""
    return torch.zeros(B, dtype=torch.int64, device=ggraph.device).index_add_(0, ggraph, flag.to(torch.int64))


def _flag_ranks(ggraph: torch.Tensor, B: int, flag: torch.Tensor) -> _Ranks:
    """`_flag_counts`, its prefix sum and every flagged group's rank inside its graph; torch ops, no host read"""
    f = flag.to(torch.int64)
    per = _flag_counts(ggraph, B, f)
    ptr = torch.zeros(B + 1, dtype=torch.int64, device=ggraph.device)
    ptr[1:] = per.cumsum(0)
    return _Ranks(per, ptr, f.cumsum(0) - f - ptr[ggraph])


def _member_group(gr: _Groups, ggraph: Optional[torch.Tensor] = None) -> torch.Tensor:
    """int32 [len(gr.members)]: the local group id of every listed member of a `_group_layout`, -1 behind the groups' members
    (the background and the dead, which the kernels never read as group members).  `ggraph`: `_group_graph(gr.count, gr.G)`
    when the caller has it.  What a subset or greedy launch hands the library as `sub_member_group`."""
    L, G, dev = int(gr.members.numel()), gr.G, gr.members.device
    if ggraph is None:
        ggraph = _group_graph(gr.count, G)
    glob = torch.bucketize(torch.arange(L, device=dev), gr.member_ptr[1:].to(torch.int64), right=True)
    local = glob - gr.group_ptr[ggraph[glob.clamp(max=G - 1)]] if G > 0 else glob
    return torch.where(glob < G, local, torch.full_like(glob, -1)).to(torch.int32).contiguous()


def _pack(subsets: torch.Tensor, group_ptr: torch.Tensor, W: int):
    """`subsets.pack_subsets` with W = the words of a row known (no host read): -> (bits [S, W] int32, word_ptr [B + 1] int32)"""
    S, G = subsets.shape
    dev = subsets.device
    group_ptr = group_ptr.to(torch.int64)
    count = group_ptr[1:] - group_ptr[:-1]
    wptr = torch.zeros(count.numel() + 1, dtype=torch.int64, device=dev)
    wptr[1:] = ((count + 31) // 32).cumsum(0)
    graph = _group_graph(count, G)
    y = torch.arange(G, device=dev) - group_ptr[graph]
    one = torch.ones_like(y) << (y & 31)
    # (bit 31 as the int32 that has it: the words are uint32 kept in int32 storage)
    weight = torch.where(one >= (1 << 31), one - (1 << 32), one).to(torch.int32)
    bits = torch.zeros(S, W, dtype=torch.int32, device=dev)
    if G > 0 and S > 0:
        # every (row, word) sums distinct bits: an integer sum, whatever its order
        bits.index_add_(1, wptr[graph] + (y >> 5), subsets.to(torch.int32) * weight)
    return bits, wptr.to(torch.int32)


def fill_lists(a, gr: _Groups, member_group: Optional[torch.Tensor] = None, live=None):
    """Hand the group lists of `gr` to the library: the `shap_` members of the block `a` and, with `member_group`
    (`_member_group`), `sub_member_group`.  `live`: `CoalitionValues`' (group_ptr, member_ptr) int32 of the LIVE groups alone
    in place of all groups'.  `shap_n_groups` is the number of listed groups: G, or the live count.  An array of length 0 (a
    batch without features or without groups) is never read, but must not be NULL: it gets the address of `group_ptr`.
    -> the tensors that must outlive the launches (the caller keeps them)."""
    p = _lib.ptr
    group_ptr, member_ptr = (gr.group_ptr.to(torch.int32), gr.member_ptr) if live is None else live
    spare = p(group_ptr)
    a.shap_group_ptr, a.shap_member_ptr, a.shap_bg_ptr = spare, p(member_ptr), p(gr.bg_ptr)
    # one array holds the groups' members and, behind them, the background
    a.shap_members = a.shap_bg_members = p(gr.members) if gr.members.numel() else spare
    if member_group is not None:
        a.sub_member_group = p(member_group) if gr.members.numel() else spare
    a.shap_n_groups = int(member_ptr.numel()) - 1
    return group_ptr, member_ptr, member_group


# ====================================================================== the players of a Shapley walk
class _Walk(NamedTuple):
    """What the loop path needs of the players (`_Players.walk`); every tensor on the batch's device."""
    count: torch.Tensor          # [B] int64 players of every graph
    start: torch.Tensor          # [B] int64 where graph g's segment of a permutation row starts
    steps: int                   # the largest count
    place: object                # (graphs [A], their local players [A]) -> the players' indices in the accumulator
    owner: torch.Tensor          # [N * F + E] int64: the player that switches the feature on, `row` for one that is always on
    live: torch.Tensor           # [row] bool: the player can change the output


class _Players:
    """The players of one call: the features themselves (`_Features`) or groups of them (`_GroupPlayers`).  `row` players in
    the batch: the width of a permutation row and of the accumulator."""
    arg = width = label = ""     # the permutation argument, its width in a message, the launch's label in an error
    flags = 0                    # of the launch
    per_cu = MAX_WORKGROUPS_PER_CU
    query: dict = {}             # what the shape query takes beside the permutation count

    def __init__(self, batch):
        self.batch = batch
        (self.N, self.F), self.E, self.B = batch.x.shape, int(batch.edge_index.shape[1]), int(batch.num_graphs)

    def permutations(self, n_samples, given, generator) -> torch.Tensor:
        """`given`, checked, or `n_samples` rows drawn from `generator`"""
        dev = self.batch.x.device
        if given is None:
            if int(n_samples) < 1:
                raise ValueError(f"n_samples must be at least 1; got {n_samples}")
            return _draw_segments(*self.segments(), self.row, n_samples, generator, dev)
        t = given
        if not torch.is_tensor(t) or t.dtype != torch.int32 or t.dim() != 2 or t.shape[0] < 1 or t.shape[1] != self.row:
            raise ValueError(f"{self.arg} must be an int32 tensor of shape [P >= 1, {self.width} = {self.row}]; got "
                             f"{getattr(t, 'dtype', type(t))} {tuple(getattr(t, 'shape', ()))}")
        if t.device != dev:
            raise ValueError(f"{self.arg} are on {t.device}, the batch on {dev}")
        return t.contiguous()


class _Features(_Players):
    arg, width, label = "permutations", "N * F + E", "hcg_explain (shapley)"

    def __init__(self, batch):
        super().__init__(batch)
        self.row = self.N * self.F + self.E

    def segments(self):
        n, e, _, _, seg = _layout(self.batch, self.F)
        return n * self.F + e, seg

    def max_steps(self, a) -> int:
        return a.max_nodes * self.F + a.max_edges

    def fill(self, a):
        pass

    def walk(self) -> _Walk:
        N, F, x, ei = self.N, self.F, self.batch.x, self.batch.edge_index
        n, e, gptr, eptr, seg = _layout(self.batch, F)
        nF, K = n * F, n * F + e

        def place(act, j):       # a node entry before the batch's edges, as `ShapleyResult` splits the accumulator
            return torch.where(j < nF[act], gptr[act] * F + j, N * F + eptr[act] + j - nF[act])
        # what cannot change the output: its difference is exactly 0 by definition
        live = torch.cat([(x != 0).reshape(-1), ei[0] != ei[1]])
        return _Walk(K, seg, int(K.max()) if self.B > 0 else 0, place, torch.arange(self.row, device=x.device), live)

    def result(self, acc, out_full, out_base) -> ShapleyResult:
        NF = self.N * self.F
        return ShapleyResult(acc[:NF].view(self.N, self.F), acc[NF:self.row], out_full, out_base)


class _GroupPlayers(_Players):
    arg, width, label = "group_permutations", "G", "hcg_explain (grouped shapley)"
    flags, per_cu = _lib.HCG_EXPLAIN_GROUPED, GROUPED_WORKGROUPS_PER_CU

    def __init__(self, batch, node_group, edge_group):
        super().__init__(batch)
        self.groups = gr = _group_layout(batch, self.F, node_group, edge_group)
        self.row = gr.G
        self.query = dict(flags=_lib.HCG_EXPLAIN_QUERY | _lib.HCG_EXPLAIN_GROUPED, shap_n_groups=gr.G)

    def segments(self):
        return self.groups.count, self.groups.group_ptr

    def max_steps(self, a) -> int:
        return self.groups.max_groups

    def fill(self, a):
        self._lists = fill_lists(a, self.groups)                           # (live as long as the call's players)

    def walk(self) -> _Walk:
        gr = self.groups

        def place(act, j):
            return gr.group_ptr[act] + j
        # a group without a live member cannot change the output: its difference is exactly 0 by definition
        return _Walk(gr.count, gr.group_ptr, gr.max_groups, place, gr.slot, gr.live_group)

    def result(self, acc, out_full, out_base) -> GroupedShapleyResult:
        gr, NF = self.groups, self.N * self.F
        flat = torch.cat([acc[:gr.G], acc.new_zeros(1)])[gr.slot]          # (the background reads the appended 0)
        return GroupedShapleyResult(acc[:gr.G], gr.group_ptr, flat[:NF].view(self.N, self.F), flat[NF:], out_full, out_base)


def _players(batch, permutations, node_group, edge_group, group_permutations):
    """-> (the players of a call with these arguments, the permutations it was given or None)"""
    if node_group is not None or edge_group is not None:
        if permutations is not None:
            raise ValueError("a grouped call takes group_permutations, not permutations")
        return _GroupPlayers(batch, node_group, edge_group), group_permutations
    if group_permutations is not None:
        raise ValueError("group_permutations need node_group or edge_group")
    return _Features(batch), permutations


# ====================================================================== a list of subsets: what does not depend on the model
def subset_layout(batch, node_group, edge_group):
    """-> (the group layout, the per-graph group counts on the host)"""
    gr = _group_layout(batch, int(batch.x.shape[1]), node_group, edge_group)
    return gr, _counts(gr.group_ptr)


def check_subsets(batch, gr: _Groups, subsets, rows_per_graph, C: int):
    """-> rows_per_graph as a host list (or None); `subsets` and the size of the [S + 2, B, C] table checked"""
    dev, B = batch.x.device, int(batch.num_graphs)
    if not torch.is_tensor(subsets) or subsets.dtype != torch.bool or subsets.dim() != 2 or subsets.shape[1] != gr.G:
        raise ValueError(f"subsets must be a bool tensor of shape [S, G = {gr.G}]; got "
                         f"{getattr(subsets, 'dtype', type(subsets))} {tuple(getattr(subsets, 'shape', ()))}")
    if subsets.device != dev:
        raise ValueError(f"subsets are on {subsets.device}, the batch on {dev}")
    S = int(subsets.shape[0])
    from . import attribution
    if (S + 2) * B * C * 4 > attribution.LAUNCH_BUDGET_BYTES:
        raise ValueError(f"the table of this call has {S} + 2 rows of {B} graphs and {C} outputs, {(S + 2) * B * C * 4} bytes, "
                         f"above LAUNCH_BUDGET_BYTES = {attribution.LAUNCH_BUDGET_BYTES}: split the rows or the batch")
    if rows_per_graph is None:
        return None
    t = rows_per_graph
    if not torch.is_tensor(t) or t.dtype not in (torch.int8, torch.int16, torch.int32, torch.int64) or tuple(t.shape) != (B,):
        raise ValueError(f"rows_per_graph must be an integer tensor of shape [B = {B}]; got {getattr(t, 'dtype', type(t))} "
                         f"{tuple(getattr(t, 'shape', ()))}")
    rp = t.tolist()
    if any(not 0 <= r <= S for r in rp):
        raise ValueError(f"rows_per_graph must lie in 0 .. S = {S}")
    return rp


def subset_jobs(B: int, S: int, rp, rpw: int) -> torch.Tensor:
    """int32 [J, 3] on the host: the jobs (graph, first row, rows) -- every graph's rows 0 .. S + 1 (`rp` None), or its rows
    0 .. rp[g] - 1 and the two appended ones, in runs of `rpw`"""
    def runs(first, count):
        # (first [B], count [B]) -> the runs of `rpw` that tile first[g] .. first[g] + count[g] - 1
        per = (count + rpw - 1) // rpw
        g = torch.repeat_interleave(torch.arange(B), per)
        ptr = torch.zeros(B + 1, dtype=torch.int64)
        ptr[1:] = per.cumsum(0)
        at = (torch.arange(g.numel()) - ptr[g]) * rpw
        return torch.stack([g, first[g] + at, torch.clamp(count[g] - at, max=rpw)], 1)
    zero = torch.zeros(B, dtype=torch.int64)
    if rp is None:
        jobs = runs(zero, zero + (S + 2))
    else:
        jobs = torch.cat([runs(zero, torch.tensor(rp, dtype=torch.int64).reshape(B)), runs(zero + S, zero + 2)])
    return jobs.to(torch.int32).contiguous()


class _SubsetCall:
    """The part of a fused subset call that does not depend on the model, built once per call and shared by the models of an
    ensemble: the S + 2 rows (the caller's, then everything on, then the background only), the jobs, and -- in `fill` -- the
    bit words, the members' group ids, the group lists and the `sub_` / `coal_` members of the block."""

    def __init__(self, B: int, gr: _Groups, counts: list, subsets: torch.Tensor, rp, rpw: int):
        self.gr, self.counts, self.subsets = gr, counts, subsets
        self.S = int(subsets.shape[0])
        self.S2 = self.S + 2
        self.jobs = subset_jobs(B, self.S, rp, rpw)
        self.J = int(self.jobs.shape[0])
        self.query = dict(coal_rows=self.S2, sub_max_groups=gr.max_groups)      # what the shape query takes

    def fill(self, a):
        """Build the device arrays and set every member of `a` the launches read beside the model's and `coal_values`"""
        gr, dev, p = self.gr, self.subsets.device, _lib.ptr
        rows = torch.cat([self.subsets, torch.ones(1, gr.G, dtype=torch.bool, device=dev), torch.zeros(1, gr.G, dtype=torch.bool, device=dev)])
        W = sum((c + 31) // 32 for c in self.counts)
        bits, word_ptr = _pack(rows, gr.group_ptr, W)
        self._keep = fill_lists(a, gr, _member_group(gr)), bits, word_ptr, self.jobs.to(dev)
        a.sub_bits, a.sub_word_ptr = (p(bits) if W else p(word_ptr)), p(word_ptr)
        a.coal_jobs, a.coal_rows, a.sub_max_groups = p(self._keep[3]), self.S2, gr.max_groups
