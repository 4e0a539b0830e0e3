"""GPU tests of `CoalitionValues`: every subset of a graph's groups evaluated on chip (csrc/shapley.hip, k_coalition_values,
HCG_EXPLAIN_COALITIONS), and the exact Shapley values and interaction indices formed from that table.
tests/coalition_ref.py states the references (the fp64 oracle per subset, the subset formulas) and the bounds.  Every figure
is printed before it is asserted (`pytest -s`)."""
import functools

import pytest
import torch

from tests import coalition_ref as CR
from tests import shapley_ref as SR

pytestmark = pytest.mark.gpu
PARAM_SEED = 23
SHAPE_LIMIT = 16
NODE_LIMIT = 184


@pytest.fixture(scope="module")
def H():
    import hcatgnet_amd
    import __graft_entry__
    import os
    from hcatgnet_amd import _lib
    if not os.path.isfile(_lib.LIB_PATH):
        __graft_entry__.build()
    return hcatgnet_amd


def _synth_case(bk, share, mk, cls, groups):
    from hcatgnet_amd import synth
    sb = synth.make_batch(**bk)
    c = CR.Case()
    c.x = CR.sparse_x(sb.x, share) if share is not None else (torch.rand(sb.x.shape, generator=torch.Generator().manual_seed(CR.X_SEED)) + 0.5).contiguous()
    c.ei, c.batch, c.B, c.F, c.cls = sb.edge_index, sb.batch, sb.num_graphs, bk["feat"], cls
    c.max_nodes, c.max_edges = sb.max_nodes, sb.max_edges
    c.params = SR.rand_params(bk["feat"], 64, seed=PARAM_SEED, **mk)
    c.ng, c.eg = (CR.fragments(c.batch, c.B, groups) if isinstance(groups, int) else groups(c)), None
    return c


@functools.lru_cache(maxsize=None)
def _case(name):
    two = dict(n_conv=2, n_read=2, n_classes=1)
    if name == "mixed":
        c = CR.mixed_case()
        c.params, c.cls = SR.rand_params(25, 64, seed=PARAM_SEED, **two), 0
    elif name == "four-convs":
        c = _synth_case(dict(num_graphs=4, nodes=16, extra_bonds=2, max_degree=4, feat=25, nodes_jitter=3), 0.3,
                        dict(n_conv=4, n_read=4, n_classes=8), 5, 4)
    elif name == "node-limit":
        c = _synth_case(dict(num_graphs=1, nodes=NODE_LIMIT, extra_bonds=12, max_degree=6, feat=25), 0.12, two, 0, 2)
        assert c.max_nodes == NODE_LIMIT
    elif name == "dense30":
        # every entry of x non-zero; group 0 = 22 atoms = 550 live members: s_apply stages them in two rounds
        c = _synth_case(dict(num_graphs=1, nodes=30, extra_bonds=3, max_degree=4, feat=25), None, two, 0,
                        lambda q: (torch.arange(30) >= 22).to(torch.int64))
        assert int((c.x[:22] != 0).sum()) == 550 > 512
    elif name == "ten-groups":
        # four 20-atom graphs, ten groups of two atoms each: 1024 masks per graph
        c = _synth_case(dict(num_graphs=4, nodes=20, extra_bonds=3, max_degree=4, feat=25), 0.3, two, 0, 10)
        assert torch.bincount(c.batch).tolist() == [20] * 4
    print(f"\n  case {name}: B {c.B} N {c.x.shape[0]} E {c.ei.shape[1]} max {c.max_nodes} / {c.max_edges}  non-zero x {int((c.x != 0).sum())}")
    return c


@functools.lru_cache(maxsize=None)
def _refs(name):
    c = _case(name)
    return CR.reference_batch(c.params, c.x, c.ei, c.batch, c.B, c.ng, c.eg, c.cls)


def _gpu_batch(H, c, max_nodes=None):
    return H.Batch(c.x.cuda(), c.ei.cuda(), c.batch.cuda(), c.B, max_nodes=max_nodes or c.max_nodes, max_edges=c.max_edges,
                   edges_grouped=True)


def _kw(c):
    return dict(node_group=c.ng.cuda(), edge_group=None if c.eg is None else c.eg.cuda(), class_index=c.cls)


def _clone(r):
    return [t.clone() for t in r]


def _one_graph(H, c, g):
    nptr, eptr = SR.pointers(c.batch, c.ei, c.B)
    a, b, ea, eb = int(nptr[g]), int(nptr[g + 1]), int(eptr[g]), int(eptr[g + 1])
    one = H.Batch(c.x[a:b].cuda(), (c.ei[:, ea:eb] - a).contiguous().cuda(), torch.zeros(b - a, dtype=torch.long).cuda(), 1,
                  max_nodes=b - a, max_edges=eb - ea, edges_grouped=True)
    return one, dict(node_group=c.ng[a:b].cuda(), edge_group=None if c.eg is None else c.eg[ea:eb].cuda(), class_index=c.cls)


# ------------------------------------------------------------------------------------------------ 1. parity
@pytest.mark.parametrize("name", ["mixed", "four-convs", "node-limit", "dense30"])
def test_parity_with_the_fp64_table_shapley_values_and_interactions(H, name):
    from hcatgnet_amd.shapley import CoalitionValues
    c = _case(name)
    cv = CoalitionValues(SR.model_from_params(H, c.params).cuda())
    gb = _gpu_batch(H, c)
    assert cv.reason(gb) is None and cv.lds_bytes(gb) > 0
    r = cv(gb, **_kw(c))
    assert cv.last_path == "fused" and isinstance(r, H.CoalitionResult)
    torch.cuda.synchronize()
    assert int(gb._hcg_plan.status[0].item()) == 0
    refs, gptr = _refs(name)
    CR.check_against_reference(r, refs, gptr, c.cls, name)


# ------------------------------------------------------------------------------------------------ 2. the walk
@pytest.mark.parametrize("name", ["mixed", "dense30", "four-convs"])
def test_prefix_masks_are_bitwise_the_walk_in_the_identity_order(H, name):
    """The walk applies the background, then group 0, 1, ... and evaluates after each; the table's rows 2^(y + 1) - 1 are
    rebuilt from zero in that order and evaluated by the same function."""
    from hcatgnet_amd.shapley import CoalitionValues, ShapleySampling
    c = _case(name)
    model = SR.model_from_params(H, c.params).cuda()
    gb = _gpu_batch(H, c)
    r = CoalitionValues(model)(gb, **_kw(c))
    gptr = r.group_ptr.cpu()
    cnt = (gptr[1:] - gptr[:-1]).tolist()
    ident = torch.cat([torch.arange(k, dtype=torch.int32) for k in cnt]).reshape(1, -1).cuda()
    w = ShapleySampling(model)(gb, group_permutations=ident, **_kw(c))
    assert torch.equal(w.out_base, r.out_base) and torch.equal(w.out_full, r.out_full)
    v = r.values[:, c.cls]
    first = r.table_ptr[:-1].repeat_interleave(torch.tensor(cnt).cuda())
    y = torch.cat([torch.arange(k) for k in cnt]).cuda()
    one = torch.ones_like(y)
    want = v[first + (one << (y + 1)) - 1] - v[first + (one << y) - 1]
    print(f"\n  {name}: {want.numel()} steps of the identity walk, {int((want != 0).sum())} non-zero")
    assert want.numel() == sum(cnt) > 0 and torch.equal(w.group_attr, want)


# ------------------------------------------------------------------------------------------------ 3. bitwise
def test_bitwise_run_length_launch_split_batch_call_and_instance(H):
    from hcatgnet_amd.shapley import CoalitionValues
    c = _case("ten-groups")
    model = SR.model_from_params(H, c.params).cuda()
    g = 2
    one, kw = _one_graph(H, c, g)
    cv = CoalitionValues(model)
    base = _clone(cv(one, subsets_per_workgroup=1, **kw))
    assert cv.last_path == "fused" and tuple(base[0].shape) == (1024, 1)
    live = [bool(((c.x[c.batch == g][2 * k:2 * k + 2]) != 0).any()) for k in range(10)]
    assert all(live)                                               # ten live groups: 1024 masks reach the kernel
    assert int(base[0].unique().numel()) > 900
    for spw in (7, 1024, None):
        got = cv(one, subsets_per_workgroup=spw, **kw)
        assert torch.equal(got.values, base[0]), spw
    again = cv(one, subsets_per_workgroup=7, **kw)
    for a, b in zip(base, again):
        assert torch.equal(a, b)
    fresh = CoalitionValues(model)(one, subsets_per_workgroup=7, **kw)
    for a, b in zip(base, fresh):
        assert torch.equal(a, b)
    split = CoalitionValues(model)
    split.jobs_per_launch = 5                                      # 147 jobs of 7 masks: 30 launches
    got = split(one, subsets_per_workgroup=7, **kw)
    for a, b in zip(base, got):
        assert torch.equal(a, b)
    # the same graph inside the batch
    full = cv(_gpu_batch(H, c), **_kw(c))
    assert tuple(full.values.shape) == (4096, 1)
    assert torch.equal(full.values[1024 * g:1024 * (g + 1)], base[0])
    assert torch.equal(full.group_attr[10 * g:10 * (g + 1)], base[3]) and torch.equal(full.interaction[100 * g:100 * (g + 1)], base[4])
    assert not torch.equal(full.values[:1024], base[0])


# ------------------------------------------------------------------------------------------------ 4. dead groups, empty cases
def test_dead_groups_a_graph_without_groups_and_an_empty_batch(H):
    from hcatgnet_amd.shapley import CoalitionValues
    c = _case("mixed")
    cv = CoalitionValues(SR.model_from_params(H, c.params).cuda())
    r = cv(_gpu_batch(H, c), **_kw(c))
    assert cv.last_path == "fused"
    refs, gptr = _refs("mixed")
    g, y = c.dead
    assert [(~q["live"]).nonzero().flatten().tolist() for q in refs] == [[], [], [], [y]]
    pairs = CR.check_dead_rows(r, refs, gptr)
    G = int(gptr[g + 1] - gptr[g])
    I = r.interaction[int(r.pair_ptr[g]):int(r.pair_ptr[g + 1])].view(G, G)
    print(f"\n  dead group {y} of graph {g}: {pairs} pairs of rows equal; group_attr {float(r.group_attr[int(gptr[g]) + y])}")
    assert pairs == 16 and float(r.group_attr[int(gptr[g]) + y]) == 0.0
    assert float(I[y].abs().max()) == 0.0 and float(I[:, y].abs().max()) == 0.0 and float(I.abs().max()) > 0.0
    # graph 0 has no group: one row
    assert int(r.table_ptr[1]) == 1 and torch.equal(r.values[0], r.out_full[0]) and torch.equal(r.values[0], r.out_base[0])
    # no graph at all
    e = H.Batch(c.x[:0].cuda(), c.ei[:, :0].cuda(), c.batch[:0].cuda(), 0, max_nodes=0, max_edges=0, edges_grouped=True)
    r0 = cv(e, node_group=c.ng[:0].cuda())
    assert cv.last_path == "fused"
    assert tuple(r0.values.shape) == (0, 1) and r0.table_ptr.tolist() == [0] and r0.group_ptr.tolist() == [0] and r0.pair_ptr.tolist() == [0]
    assert r0.group_attr.numel() == 0 and r0.interaction.numel() == 0 and tuple(r0.out_full.shape) == (0, 1) == tuple(r0.out_base.shape)


# ------------------------------------------------------------------------------------------------ 5. refusal and fallback
def test_a_graph_over_max_nodes_is_refused_and_the_others_keep_their_values(H):
    from hcatgnet_amd.shapley import CoalitionValues
    c = _case("mixed")
    sizes = torch.bincount(c.batch, minlength=c.B)
    big = sizes == sizes.max()
    assert 0 < int(big.sum()) < c.B
    cv = CoalitionValues(SR.model_from_params(H, c.params).cuda())
    honest = _clone(cv(_gpu_batch(H, c), **_kw(c)))
    gb = _gpu_batch(H, c, max_nodes=int(sizes.max()) - 1)
    r = cv(gb, subsets_per_workgroup=3, **_kw(c))
    assert cv.last_path == "fused"
    torch.cuda.synchronize()
    status = gb._hcg_plan.status
    word = int(status[0].item())
    status.zero_()                                                    # (shared per device: leave it clean for the next test)
    assert word & SHAPE_LIMIT
    rows = (r.table_ptr[1:] - r.table_ptr[:-1]).cpu()
    row_big = big.repeat_interleave(rows).cuda()
    assert torch.equal(r.values[~row_big], honest[0][~row_big]) and float(r.values[row_big].abs().max()) == 0.0
    gptr = r.group_ptr.cpu()
    group_big = big.repeat_interleave(gptr[1:] - gptr[:-1]).cuda()
    assert torch.equal(r.group_attr[~group_big], honest[3][~group_big])
    if bool(group_big.any()):
        assert float(r.group_attr[group_big].abs().max()) == 0.0
    assert float(r.out_full[big.cuda()].abs().max()) == 0.0 and float(r.out_base[big.cuda()].abs().max()) == 0.0


def test_a_model_outside_the_limits_takes_the_loop_with_the_same_bounds(H):
    """D = 128: one masked forward of the whole batch per mask index on `ExplainStep`'s any-shape path."""
    from hcatgnet_amd.shapley import CoalitionValues
    c = _synth_case(dict(num_graphs=3, nodes=8, extra_bonds=2, max_degree=4, feat=6, nodes_jitter=2), 0.5, {}, 1, 3)
    c.params = SR.rand_params(6, 128, seed=PARAM_SEED, n_classes=2)
    model = SR.model_from_params(H, c.params).cuda()
    before = [q.detach().clone() for q in model.parameters()]
    cv = CoalitionValues(model)
    gb = _gpu_batch(H, c)
    assert "shape" in cv.reason(gb)
    r = cv(gb, **_kw(c))
    assert cv.last_path == "loop"
    refs, gptr = CR.reference_batch(c.params, c.x, c.ei, c.batch, c.B, c.ng, c.eg, c.cls)
    CR.check_against_reference(r, refs, gptr, c.cls, "D = 128 (loop)")
    for q, b in zip(model.parameters(), before):
        assert torch.equal(q.detach(), b) and q.grad is None
