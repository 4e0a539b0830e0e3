"""Host test of `_groups.fill_lists`, the one place that hands the group lists of a batch to the library (no GPU: the block
takes the addresses of CPU tensors, nothing dereferences them).  Three batches: groups and features, every feature in the
background, and no graph at all; both forms: all groups (`ShapleySampling`, `SubsetValues`, `GreedySelection`, the ensemble
classes) and `CoalitionValues`' live groups alone."""
import pytest
import torch

import hcatgnet_amd as H
from hcatgnet_amd import _groups, _lib
from tests import coalition_ref as CR

LISTS = ("shap_group_ptr", "shap_member_ptr", "shap_members", "shap_bg_ptr", "shap_bg_members")


def _batches():
    c = CR.mixed_case()
    full = H.Batch(c.x, c.ei, c.batch, c.B, max_nodes=c.max_nodes, max_edges=c.max_edges, edges_grouped=True)
    none = H.Batch(c.x[:0], c.ei[:, :0], c.batch[:0], 0, max_nodes=0, max_edges=0, edges_grouped=True)
    return {"groups and features": (full, c.ng, c.eg), "all background": (full, torch.full_like(c.ng, -1), None),
            "no graph": (none, c.ng[:0], None)}


@pytest.mark.parametrize("name", ["groups and features", "all background", "no graph"])
def test_the_lists_are_never_null_and_count_the_listed_groups(name):
    batch, ng, eg = _batches()[name]
    gr = _groups._group_layout(batch, int(batch.x.shape[1]), ng, eg)
    L, p = int(gr.members.numel()), _lib.ptr
    assert (gr.G > 0, L > 0) == {"groups and features": (True, True), "all background": (False, True), "no graph": (False, False)}[name]

    # ---- all groups, without and with the members' group ids
    for with_ids in (False, True):
        a = _lib.ExplainArgs()
        mg = _groups._member_group(gr) if with_ids else None
        group_ptr, member_ptr, kept = _groups.fill_lists(a, gr, mg)
        assert group_ptr.dtype == torch.int32 and torch.equal(group_ptr.to(torch.int64), gr.group_ptr) and member_ptr is gr.member_ptr
        assert kept is mg
        assert all(getattr(a, k) for k in LISTS), {k: getattr(a, k) for k in LISTS}
        assert (a.shap_group_ptr, a.shap_member_ptr, a.shap_bg_ptr) == (p(group_ptr), p(gr.member_ptr), p(gr.bg_ptr))
        # one array holds the members and the background; an empty one is stood in for by group_ptr, never NULL
        assert a.shap_members == a.shap_bg_members == (p(gr.members) if L else p(group_ptr))
        assert a.sub_member_group == ((p(mg) if L else p(group_ptr)) if with_ids else None)      # (None: NULL, not touched)
        assert a.shap_n_groups == gr.G
        print(f"\n  {name}, ids {with_ids}: G {gr.G}, members {L}, shap_n_groups {a.shap_n_groups}")

    # ---- CoalitionValues' form: the live groups' pointers
    keep = torch.cat([gr.live_group, torch.ones(1, dtype=torch.bool)])
    live_member_ptr = gr.member_ptr[keep].contiguous()
    B = int(batch.num_graphs)
    live_ptr = _groups._flag_ranks(_groups._group_graph(gr.count, gr.G), B, gr.live_group).ptr.to(torch.int32)
    a = _lib.ExplainArgs()
    got = _groups.fill_lists(a, gr, live=(live_ptr, live_member_ptr))
    assert got[0] is live_ptr and got[1] is live_member_ptr and got[2] is None
    assert all(getattr(a, k) for k in LISTS)
    assert (a.shap_group_ptr, a.shap_member_ptr, a.shap_bg_ptr) == (p(live_ptr), p(live_member_ptr), p(gr.bg_ptr))
    assert a.shap_members == a.shap_bg_members == (p(gr.members) if L else p(live_ptr)) and a.sub_member_group is None
    n_live = int(gr.live_group.sum())
    assert a.shap_n_groups == n_live == int(live_ptr[-1])
    if name == "groups and features":
        assert 0 < n_live < gr.G                                            # (the case has a dead group: the two forms differ)
    print(f"  {name}, live form: {n_live} of {gr.G} groups")


def test_the_flag_helper_counts_and_ranks_inside_each_graph():
    count = torch.tensor([0, 3, 1, 4])
    ggraph = _groups._group_graph(count, 8)
    assert ggraph.tolist() == [1, 1, 1, 2, 3, 3, 3, 3]
    flag = torch.tensor([True, False, True, False, True, True, False, True])
    r = _groups._flag_ranks(ggraph, 4, flag)
    assert r.per_graph.tolist() == [0, 2, 0, 3] == _groups._flag_counts(ggraph, 4, flag).tolist() and r.ptr.tolist() == [0, 0, 2, 2, 5]
    assert r.rank[flag].tolist() == [0, 1, 0, 1, 2]
    dead = _groups._flag_ranks(ggraph, 4, ~flag)
    assert dead.per_graph.tolist() == [0, 1, 1, 1] and dead.rank[~flag].tolist() == [0, 0, 0]
    e = _groups._flag_ranks(_groups._group_graph(count[:0], 0), 0, flag[:0])
    assert e.per_graph.tolist() == [] and e.ptr.tolist() == [0] and e.rank.tolist() == []
