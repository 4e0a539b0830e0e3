"""Host side of `EnsembleShapley`, `EnsembleSubsetValues` and `EnsembleCurves` (no GPU): the loop path on CPU tensors against
the stacked single-model loops and torch moments, the argument checks, `per_model`, `refresh()`, the library's answers to
`n_models`, and the two helpers this feature lifted out of `SubsetValues` / `GreedySelection` / `AttributionCurves` against
restatements of what they replaced.  tests/ensemble_shapley_ref.py states the models and the yardsticks."""
import os

import pytest
import torch

import hcatgnet_amd as H
from hcatgnet_amd import _lib
from hcatgnet_amd.shapley import ShapleySampling, _group_layout
from hcatgnet_amd.subsets import AttributionCurves, SubsetValues, _group_graph, _member_group, ranking
from tests import coalition_ref as CR
from tests import ensemble_shapley_ref as ER
from tests import subsets_ref as UR

ROW_SEED = 11


@pytest.fixture(scope="module", autouse=True)
def built():
    if not os.path.isfile(_lib.LIB_PATH):
        import __graft_entry__
        __graft_entry__.build()


def _batch(c):
    return H.Batch(c.x, c.ei, c.batch, c.B, max_nodes=c.max_nodes, max_edges=c.max_edges, edges_grouped=True)


@pytest.fixture(scope="module")
def small():
    """three graphs of 5, 7 and 9 nodes, 7 features, atoms as players; three models of two classes"""
    c = UR.sized_case((5, 7, 9), feat=7)
    c.x = CR.sparse_x(c.x, 0.5)
    c.b = _batch(c)
    c.ng = H.atom_groups(c.b)
    c.models = ER.models(H, 7, 3, dict(n_conv=2, n_read=2, n_classes=2))
    c.G = 21
    return c


# ------------------------------------------------------------------------------------------------ the loop path
def test_cpu_tensors_take_the_loop_and_equal_the_stacked_single_model_loops(small):
    c = small
    es = H.EnsembleShapley(c.models)
    assert "CPU" in es.reason(c.b) and es.reason() is None and es.n_models == 3
    perm = H.draw_group_permutations(c.b, node_group=c.ng, n_samples=2, generator=torch.Generator().manual_seed(3))
    r = es(c.b, group_permutations=perm, node_group=c.ng, class_index=1, per_model=True)
    assert es.last_path == "loop" and isinstance(r, H.EnsembleShapleyResult)
    singles = [ShapleySampling(m).loop(c.b, group_permutations=perm, node_group=c.ng, class_index=1) for m in c.models]
    per = torch.stack([s.group_attr for s in singles])
    assert torch.equal(r.group_attr, per) and not torch.equal(per[0], per[1])
    assert torch.equal(r.group_mean, per.mean(0)) and torch.equal(r.group_std, per.std(0, unbiased=False))
    assert torch.equal(r.out_full, torch.stack([s.out_full for s in singles])) and tuple(r.out_base.shape) == (3, c.B, 2)
    assert torch.equal(r.node_mean, torch.stack([s.node_attr for s in singles]).mean(0)) and tuple(r.edge_std.shape) == (c.ei.shape[1],)
    assert torch.equal(r.group_ptr, singles[0].group_ptr)
    # the same through `loop`, and without the per-model array
    r2 = es.loop(c.b, group_permutations=perm, node_group=c.ng, class_index=1)
    assert r2.group_attr is None and torch.equal(r2.group_mean, r.group_mean)
    # ungrouped
    fperm = H.draw_permutations(c.b, 7, 1, torch.Generator().manual_seed(4))
    rf = es(c.b, permutations=fperm, per_model=True)
    assert es.last_path == "loop" and isinstance(rf, H.EnsembleFeatureShapleyResult)
    sf = [ShapleySampling(m).loop(c.b, permutations=fperm) for m in c.models]
    assert torch.equal(rf.node_attr, torch.stack([s.node_attr for s in sf])) and torch.equal(rf.edge_attr, torch.stack([s.edge_attr for s in sf]))
    assert torch.equal(rf.edge_mean, rf.edge_attr.mean(0)) and torch.equal(rf.node_std, rf.node_attr.std(0, unbiased=False))
    assert es(c.b, permutations=fperm).node_attr is None


def test_subset_values_and_curves_on_the_loop_path(small):
    c = small
    rows = UR.random_rows(5, c.G, ROW_SEED)
    ev = H.EnsembleSubsetValues(c.models)
    assert "CPU" in ev.reason(c.b)
    r = ev(c.b, rows, node_group=c.ng, per_model=True)
    assert ev.last_path == "loop" and isinstance(r, H.EnsembleSubsetResult)
    singles = [SubsetValues(m).loop(c.b, rows, node_group=c.ng) for m in c.models]
    vals = torch.stack([s.values for s in singles])
    assert torch.equal(r.values, vals) and tuple(vals.shape) == (3, 5, c.B, 2) and not torch.equal(vals[0], vals[2])
    assert torch.equal(r.mean, vals.mean(0)) and torch.equal(r.std, vals.std(0, unbiased=False))
    assert torch.equal(r.out_full, torch.stack([s.out_full for s in singles])) and torch.equal(r.out_base, torch.stack([s.out_base for s in singles]))
    assert ev(c.b, rows, node_group=c.ng).values is None
    rp = torch.tensor([0, 5, 2])
    part = ev(c.b, rows, node_group=c.ng, rows_per_graph=rp, per_model=True)
    for g, n in enumerate(rp.tolist()):
        assert torch.equal(part.values[:, :n, g], vals[:, :n, g]) and float(part.values[:, n:, g].abs().sum()) == 0.0
    # curves of the mean output: every point is the mean of the models' single-model curves' points
    order = ranking(torch.randn(c.G, generator=torch.Generator().manual_seed(ROW_SEED)), r.group_ptr)
    ec = H.EnsembleCurves(c.models)
    rc = ec(c.b, order, node_group=c.ng, class_index=1)
    assert ec.last_path == "loop" and isinstance(rc, H.EnsembleCurveResult)
    cs = [AttributionCurves(m)(c.b, order, node_group=c.ng, class_index=1) for m in c.models]
    ins, dele = torch.stack([q.insertion for q in cs]), torch.stack([q.deletion for q in cs])
    assert torch.equal(rc.insertion, ins.mean(0)) and torch.equal(rc.deletion_std, dele.std(0, unbiased=False))
    assert torch.equal(rc.k, cs[0].k) and torch.equal(rc.curve_ptr, cs[0].curve_ptr)
    assert torch.equal(rc.out_full, torch.stack([q.out_full for q in cs]).mean(0))
    cp = rc.curve_ptr.tolist()
    for g in range(c.B):
        G = cp[g + 1] - cp[g] - 1
        for curve, auc in ((rc.insertion, rc.insertion_auc), (rc.deletion, rc.deletion_auc)):
            want = UR.trapezoid(list(range(G + 1)), curve[cp[g]:cp[g + 1], 1].double(), G)
            scale = max(1.0, float(curve[cp[g]:cp[g + 1]].abs().max()))
            assert abs(float(auc[g]) - want) <= UR.TOL * scale + 2.0 ** -23 * scale


# ------------------------------------------------------------------------------------------------ arguments
def test_argument_errors(small):
    c = small
    other = ER.models(H, 7, 1, dict(n_conv=3, n_read=2, n_classes=2))
    for cls in (H.EnsembleShapley, H.EnsembleSubsetValues, H.EnsembleCurves):
        with pytest.raises(ValueError, match="model 1 has"):
            cls([c.models[0], other[0]])
        with pytest.raises(ValueError):
            cls([])
    es, ev = H.EnsembleShapley(c.models), H.EnsembleSubsetValues(c.models)
    rows = UR.random_rows(3, c.G, ROW_SEED)
    with pytest.raises(ValueError, match="models_per_launch"):
        es(c.b, node_group=c.ng, models_per_launch=0)
    with pytest.raises(ValueError, match="samples_per_launch"):
        es(c.b, node_group=c.ng, samples_per_launch=0)
    with pytest.raises(ValueError, match="models_per_launch"):
        ev(c.b, rows, node_group=c.ng, models_per_launch=0)
    with pytest.raises(ValueError, match="rows_per_workgroup"):
        ev(c.b, rows, node_group=c.ng, rows_per_workgroup=0)
    with pytest.raises(ValueError, match="subsets are on"):
        ev(c.b, rows.to("meta"), node_group=c.ng)
    with pytest.raises(ValueError, match="subsets must be a bool"):
        ev(c.b, rows[:, :-1], node_group=c.ng)
    with pytest.raises(ValueError, match="group_permutations"):
        es(c.b, node_group=c.ng, permutations=torch.zeros(1, 3, dtype=torch.int32))
    with pytest.raises(ValueError, match="order must"):
        H.EnsembleCurves(c.models)(c.b, torch.zeros(c.G, dtype=torch.int32), node_group=c.ng)


def test_refresh_picks_up_changed_weights(small):
    ms = ER.models(H, 7, 2, dict(n_conv=2, n_read=2, n_classes=2))
    for obj in (H.EnsembleShapley(ms), H.EnsembleSubsetValues(ms), H.EnsembleCurves(ms)):
        stacked = (obj.values if isinstance(obj, H.EnsembleCurves) else obj).stacked
        name = "conv1.lin.weight"
        buf = stacked[name]
        with torch.no_grad():
            ms[1].conv1.lin.weight.mul_(1.5)
        assert not torch.equal(buf[1], ms[1].conv1.lin.weight) and torch.equal(buf[0], ms[0].conv1.lin.weight)
        assert obj.refresh() is obj
        assert stacked[name] is buf and torch.equal(buf[1], ms[1].conv1.lin.weight)


def test_the_library_reads_n_models():
    figures = ER.library_level(_lib)
    print(f"\n  one-model workspace of 3 permutations: {figures}")
    assert figures[0] == 3 * (120 * 25 + 270) * 4 + (-(3 * (120 * 25 + 270) * 4) % 256) and figures[12] == 256


# ------------------------------------------------------------------------------------------------ the lifted helpers
def _member_group_inline(gr):
    """what `SubsetValues._table` and `GreedySelection.__call__` both spelled out"""
    G, dev = gr.G, gr.members.device
    L = int(gr.members.numel())
    ggraph = torch.repeat_interleave(torch.arange(gr.count.numel(), device=dev), gr.count, output_size=G)
    glob = torch.bucketize(torch.arange(L, device=dev), gr.member_ptr[1:].to(torch.int64), right=True)
    local = glob - gr.group_ptr[ggraph[glob.clamp(max=G - 1)]] if G > 0 else glob
    return torch.where(glob < G, local, torch.full_like(glob, -1)).to(torch.int32).contiguous()


def test_member_group_equals_the_construction_it_replaces(small):
    mixed = CR.mixed_case()
    cases = [(_batch(mixed), mixed.ng, mixed.eg), (small.b, small.ng, None),
             (small.b, None, H.bond_groups(small.b))]
    for b, ng, eg in cases:
        gr = _group_layout(b, int(b.x.shape[1]), ng, eg)
        want = _member_group_inline(gr)
        assert torch.equal(_member_group(gr), want) and torch.equal(_member_group(gr, _group_graph(gr.count, gr.G)), want)
        assert want.dtype == torch.int32 and want.numel() == gr.members.numel()
        # a listed member's id is its group's local id; everything behind the groups' members is -1
        end = int(gr.member_ptr[-1])
        assert bool((want[:end] >= 0).all()) and bool((want[end:] == -1).all()) and end > 0
        for y in range(gr.G):
            a, e = int(gr.member_ptr[y]), int(gr.member_ptr[y + 1])
            g = int(torch.searchsorted(gr.group_ptr, torch.tensor(y), right=True)) - 1
            assert bool((want[a:e] == y - int(gr.group_ptr[g])).all())


def test_the_curve_rows_are_attribution_curves_rows(small):
    """`AttributionCurves._plan` against plain loops: pair i of a graph = (the first k groups of its order, everything else)."""
    c = small
    gr = _group_layout(c.b, 7, c.ng, None)
    counts = [5, 7, 9]
    order = ranking(torch.randn(c.G, generator=torch.Generator().manual_seed(ROW_SEED)), gr.group_ptr)
    o = order.flatten().tolist()
    gp = gr.group_ptr.tolist()
    for fr, ks in ((None, [list(range(n + 1)) for n in counts]), ([0.0, 0.3, 0.3, 1.0], [UR.points_ref(n, [0.0, 0.3, 0.3, 1.0]) for n in counts])):
        plan = AttributionCurves._plan(gr, counts, order, fr, c.x.device)
        pairs = [sorted({k for k in kg if 0 < k < n}) for kg, n in zip(ks, counts)]
        S = 2 * max(len(p) for p in pairs)
        assert plan.S == S and plan.rows_per_graph == [2 * len(p) for p in pairs] and tuple(plan.rows.shape) == (S, c.G)
        want = torch.zeros(S, c.G, dtype=torch.bool)
        for g, n in enumerate(counts):
            seg = o[gp[g]:gp[g] + n]
            for i, k in enumerate(pairs[g]):
                for y in seg[:k]:
                    want[2 * i, gp[g] + y] = True
                for y in seg[k:]:
                    want[2 * i + 1, gp[g] + y] = True
        assert torch.equal(plan.rows, want)
        assert plan.k.tolist() == [k for kg in ks for k in kg] and plan.curve_ptr.tolist()[-1] == sum(len(kg) for kg in ks)
        at = 0
        for g, n in enumerate(counts):
            for k in ks[g]:
                ins = S + 1 if k == 0 else S if k == n else 2 * pairs[g].index(k)
                dele = S if k == 0 else S + 1 if k == n else 2 * pairs[g].index(k) + 1
                assert (int(plan.ins_row[at]), int(plan.del_row[at]), int(plan.graph[at])) == (ins, dele, g)
                at += 1
    # and the class built on it still returns what a `SubsetValues` call on those rows returns
    m = small.models[0]
    plan = AttributionCurves._plan(gr, counts, order, None, c.x.device)
    r = AttributionCurves(m)(c.b, order, node_group=c.ng)
    v = SubsetValues(m)(c.b, plan.rows, node_group=c.ng, rows_per_graph=torch.tensor(plan.rows_per_graph))
    table = torch.cat([v.values, v.out_full.unsqueeze(0), v.out_base.unsqueeze(0)])
    assert torch.equal(r.insertion, table[plan.ins_row, plan.graph]) and torch.equal(r.deletion, table[plan.del_row, plan.graph])
