"""GPU tests of `SubsetValues` and `AttributionCurves`: a list of subsets of a graph's groups evaluated on chip
(csrc/shapley.hip, k_subset_values, HCG_EXPLAIN_SUBSETS), and the deletion / insertion curves built on it.
tests/subsets_ref.py states the references (the fp64 oracle per row and graph, Python loops for curves and areas) and the
bounds.  Every figure is printed before it is asserted (`pytest -s`)."""
import functools

import pytest
import torch

from tests import coalition_ref as CR
from tests import shapley_ref as SR
from tests import subsets_ref as UR

pytestmark = pytest.mark.gpu
PARAM_SEED, ROW_SEED = 23, 11
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


def _host_batch(c):
    import hcatgnet_amd
    return hcatgnet_amd.Batch(c.x, c.ei, c.batch, c.B, max_nodes=c.max_nodes, max_edges=c.max_edges, edges_grouped=True)


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


def _sized(sizes, share, bonds):
    import hcatgnet_amd
    c = UR.sized_case(sizes)
    c.x = CR.sparse_x(c.x, share)
    c.cls = 0
    c.params = SR.rand_params(25, 64, seed=PARAM_SEED, n_conv=2, n_read=2, n_classes=1)
    hb = _host_batch(c)
    c.ng = hcatgnet_amd.atom_groups(hb)
    c.eg = hcatgnet_amd.bond_groups(hb, first=torch.bincount(c.batch, minlength=c.B)) if bonds else None
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
    elif name == "dense30":
        # every entry of x non-zero; group 0 = 22 atoms = 550 live members: the filtered pass runs two staging rounds
        c = _synth_case(dict(num_graphs=1, nodes=30, extra_bonds=3, max_degree=4, feat=25), None, two, 0,
                        lambda q: (torch.arange(30) >= 22).to(torch.int64))
        assert int((c.x[:22] != 0).sum()) == 550 > 512
    elif name == "ten-groups":
        c = _synth_case(dict(num_graphs=4, nodes=20, extra_bonds=3, max_degree=4, feat=25), 0.3, two, 0, 10)
    elif name == "atoms-bonds":
        # atoms plus bonds as players on 33, 36 and 40 nodes: 68 - 82 groups, three words per graph
        c = _sized((33, 36, 40), 0.3, True)
    elif name == "node-limit":
        # one graph at the node limit, atoms as players: 184 groups, six words
        c = _sized((NODE_LIMIT,), 0.12, False)
        assert c.max_nodes == NODE_LIMIT
    elif name == "atoms":
        # atoms as players around the word boundary
        c = _sized((31, 32, 33, 40), 0.3, False)
    print(f"\n  case {name}: B {c.B} N {c.x.shape[0]} E {c.ei.shape[1]} max {c.max_nodes} / {c.max_edges}  non-zero x {int((c.x != 0).sum())}")
    return c


@functools.lru_cache(maxsize=None)
def _forwards(name):
    c = _case(name)
    return UR.Forwards(c.params, c.x, c.ei, c.batch, c.B, c.ng, c.eg)


def _gpu_batch(H, c, max_nodes=None):
    return H.Batch(c.x.cuda(), c.ei.cuda(), c.batch.cuda(), c.B, max_nodes=max_nodes or c.max_nodes, max_edges=c.max_edges,
                   edges_grouped=True)


def _kw(c):
    return dict(node_group=c.ng.cuda(), edge_group=None if c.eg is None else c.eg.cuda())


def _clone(r):
    return [t.clone() for t in r]


def _same(a, b):
    return all(torch.equal(p, q) for p, q in zip(a, b))


def _one_graph(H, c, g):
    nptr, eptr = SR.pointers(c.batch, c.ei, c.B)
    a, b, ea, eb = int(nptr[g]), int(nptr[g + 1]), int(eptr[g]), int(eptr[g + 1])
    one = H.Batch(c.x[a:b].cuda(), (c.ei[:, ea:eb] - a).contiguous().cuda(), torch.zeros(b - a, dtype=torch.long).cuda(), 1,
                  max_nodes=b - a, max_edges=eb - ea, edges_grouped=True)
    ng = c.ng[a:b]
    return one, dict(node_group=ng.cuda(), edge_group=None if c.eg is None else c.eg[ea:eb].cuda())


def _mask_rows(counts, gptr, S):
    """bool [S, G]: row s carries the bits of s in every graph's columns"""
    rows = torch.zeros(S, int(gptr[-1]), dtype=torch.bool)
    for g, G in enumerate(counts):
        for y in range(G):
            rows[:, int(gptr[g]) + y] = (torch.arange(S) >> y) & 1 == 1
    return rows


# ------------------------------------------------------------------------------------------------ 1. parity
@pytest.mark.parametrize("name", ["mixed", "four-convs", "atoms-bonds", "node-limit"])
def test_parity_with_the_fp64_values(H, name):
    from hcatgnet_amd.subsets import SubsetValues
    c, fw = _case(name), _forwards(name)
    counts = [fw.count(g) for g in range(c.B)]
    print(f"  groups {counts}")
    if name == "atoms-bonds":
        assert min(counts) > 64 and all((G + 31) // 32 == 3 for G in counts)
    if name == "node-limit":
        assert counts == [NODE_LIMIT]
    rows = UR.random_rows(14, int(fw.gptr[-1]), ROW_SEED)
    sv = SubsetValues(SR.model_from_params(H, c.params).cuda())
    gb = _gpu_batch(H, c)
    assert sv.reason(gb) is None and sv.lds_bytes(gb) > 0
    r = sv(gb, rows.cuda(), **_kw(c))
    assert sv.last_path == "fused" and isinstance(r, H.SubsetResult)
    torch.cuda.synchronize()
    assert int(gb._hcg_plan.status[0].item()) == 0
    assert tuple(r.values.shape) == (14, c.B, 8 if name == "four-convs" else 1)
    UR.check_values(r, UR.values_ref(fw, rows), fw, name)
    assert torch.equal(r.values[0], r.out_base) and torch.equal(r.values[1], r.out_full)


# ------------------------------------------------------------------------------------------------ 2. the coalition table
@pytest.mark.parametrize("name", ["ten-groups", "dense30", "mixed", "four-convs"])
def test_rows_are_bitwise_the_coalition_table(H, name):
    """The filtered pass applies, for a mask, the members the coalition kernel applies group by group, in the same order."""
    from hcatgnet_amd.shapley import CoalitionValues
    from hcatgnet_amd.subsets import SubsetValues
    c = _case(name)
    model = SR.model_from_params(H, c.params).cuda()
    gb = _gpu_batch(H, c)
    t = CoalitionValues(model)(gb, class_index=c.cls, **_kw(c))
    gptr = t.group_ptr.cpu()
    counts = (gptr[1:] - gptr[:-1]).tolist()
    S = 1 << max(counts)
    rows = _mask_rows(counts, gptr, S)
    sv = SubsetValues(model)
    r = sv(gb, rows.cuda(), rows_per_graph=torch.tensor([1 << G for G in counts]), **_kw(c))
    assert sv.last_path == "fused"
    for g, G in enumerate(counts):
        a = int(t.table_ptr[g])
        assert torch.equal(r.values[:1 << G, g], t.values[a:a + (1 << G)]), (name, g)
        assert float(r.values[1 << G:, g].abs().sum()) == 0.0
    assert torch.equal(r.out_full, t.out_full) and torch.equal(r.out_base, t.out_base)
    print(f"\n  {name}: {sum(1 << G for G in counts)} rows bitwise the coalition table's ({int(r.values.unique().numel())} distinct values)")
    if name == "dense30":
        # group 0's 550 members span two staging rounds; the complement subset {1} filters inside both
        assert counts == [2] and not torch.equal(r.values[2, 0], r.values[1, 0]) and not torch.equal(r.values[2, 0], r.values[0, 0])


# ------------------------------------------------------------------------------------------------ 3. the walk beyond 16 groups
def test_prefix_rows_are_bitwise_the_walk_in_the_identity_order(H):
    from hcatgnet_amd.shapley import ShapleySampling
    from hcatgnet_amd.subsets import SubsetValues
    c = _case("atoms")
    sizes = torch.bincount(c.batch).tolist()
    assert sizes == [31, 32, 33, 40]
    model = SR.model_from_params(H, c.params).cuda()
    gb = _gpu_batch(H, c)
    gptr = torch.tensor([0] + sizes).cumsum(0)
    y = torch.cat([torch.arange(n) for n in sizes])
    rows = torch.arange(max(sizes) + 1).unsqueeze(1) > y.unsqueeze(0)       # row s: the groups 0 .. s - 1 on
    r = SubsetValues(model)(gb, rows.cuda(), **_kw(c))
    ident = y.to(torch.int32).reshape(1, -1).cuda()
    w = ShapleySampling(model)(gb, group_permutations=ident, class_index=c.cls, **_kw(c))
    assert torch.equal(w.out_base, r.out_base) and torch.equal(w.out_full, r.out_full)
    want = torch.cat([r.values[1:n + 1, g, c.cls] - r.values[:n, g, c.cls] for g, n in enumerate(sizes)])
    print(f"\n  atoms: {want.numel()} steps of the identity walk, {int((want != 0).sum())} non-zero")
    assert want.numel() == int(gptr[-1]) and int((want != 0).sum()) > 100 and torch.equal(w.group_attr, want)
    for g, n in enumerate(sizes):
        assert torch.equal(r.values[0, g], r.out_base[g]) and torch.equal(r.values[n, g], r.out_full[g])


# ------------------------------------------------------------------------------------------------ 4. independence
def test_bitwise_run_length_launch_split_row_order_batch_call_and_instance(H):
    from hcatgnet_amd.subsets import SubsetValues
    c = _case("mixed")
    model = SR.model_from_params(H, c.params).cuda()
    gb = _gpu_batch(H, c)
    G = 9
    rows = UR.random_rows(14, G, ROW_SEED).cuda()
    sv = SubsetValues(model)
    base = _clone(sv(gb, rows, rows_per_workgroup=1, **_kw(c)))
    assert sv.last_path == "fused" and int(base[0].unique().numel()) > 10
    for rpw in (7, None):
        assert _same(base, sv(gb, rows, rows_per_workgroup=rpw, **_kw(c))), rpw
    assert _same(base, sv(gb, rows, rows_per_workgroup=7, **_kw(c)))            # a second call
    assert _same(base, SubsetValues(model)(gb, rows, rows_per_workgroup=7, **_kw(c)))   # a fresh instance
    split = SubsetValues(model)
    split.jobs_per_launch = 5                                      # 4 graphs x 16 rows in runs of 3: 24 jobs, 5 launches
    assert _same(base, split(gb, rows, rows_per_workgroup=3, **_kw(c)))
    rev = sv(gb, rows.flip(0), **_kw(c))
    assert torch.equal(rev.values.flip(0), base[0]) and torch.equal(rev.out_full, base[2]) and torch.equal(rev.out_base, base[3])
    # one graph alone against the same graph inside the batch
    gptr = base[1].cpu().tolist()
    for g in (2, 3):
        one, kw = _one_graph(H, c, g)
        alone = sv(one, rows[:, gptr[g]:gptr[g + 1]].contiguous(), **kw)
        assert torch.equal(alone.values[:, 0], base[0][:, g]) and torch.equal(alone.out_full[0], base[2][g])
    assert not torch.equal(base[0][:, 2], base[0][:, 3])
    # rows that differ only in the dead group's bit are equal
    g, y = c.dead
    flipped = rows.clone()
    flipped[:, gptr[g] + y] = ~flipped[:, gptr[g] + y]
    assert torch.equal(sv(gb, flipped, **_kw(c)).values, base[0])


# ------------------------------------------------------------------------------------------------ 5. curves
def test_curves_on_the_atoms_case(H):
    from hcatgnet_amd.subsets import AttributionCurves, SubsetValues, ranking
    c, fw = _case("atoms"), _forwards("atoms")
    sizes = torch.bincount(c.batch).tolist()
    gptr = fw.gptr
    model = SR.model_from_params(H, c.params).cuda()
    gb = _gpu_batch(H, c)
    scores = torch.randn(int(gptr[-1]), generator=torch.Generator().manual_seed(ROW_SEED))
    order = ranking(scores.cuda(), gptr.cuda())
    assert order.is_cuda and tuple(order.shape) == (1, int(gptr[-1]))
    ac = AttributionCurves(model)
    r = ac(gb, order, class_index=c.cls, **_kw(c))
    assert ac.last_path == "fused" and isinstance(r, H.CurveResult)
    o = order.flatten().cpu().tolist()
    UR.check_curves(r, UR.curves_ref(fw, o, c.cls), fw, c.cls, "atoms")
    cp = r.curve_ptr.cpu().tolist()
    assert [b - a for a, b in zip(cp[:-1], cp[1:])] == [n + 1 for n in sizes]
    # the ends are the two outputs, bitwise
    for g in range(c.B):
        assert torch.equal(r.insertion[cp[g]], r.out_base[g]) and torch.equal(r.deletion[cp[g + 1] - 1], r.out_base[g])
        assert torch.equal(r.insertion[cp[g + 1] - 1], r.out_full[g]) and torch.equal(r.deletion[cp[g]], r.out_full[g])
    # every point is the `SubsetValues` row of the same subset
    K = max(sizes) + 1
    pos = torch.empty(int(gptr[-1]), dtype=torch.long)
    for g, n in enumerate(sizes):
        pos[int(gptr[g]) + torch.tensor(o[int(gptr[g]):int(gptr[g]) + n])] = torch.arange(n)
    first = pos.unsqueeze(0) < torch.arange(K).unsqueeze(1)                  # row k: the first k groups of the order
    v = SubsetValues(model)(gb, torch.cat([first, ~first]).cuda(), **_kw(c))
    for g, n in enumerate(sizes):
        assert torch.equal(r.insertion[cp[g]:cp[g + 1]], v.values[:n + 1, g]) and torch.equal(r.deletion[cp[g]:cp[g + 1]], v.values[K:K + n + 1, g])
    # fractions pick the stated k and the full curve's bits there
    fr = [0, .25, .5, 1]
    rf = ac(gb, order, class_index=c.cls, fractions=fr, **_kw(c))
    UR.check_curves(rf, UR.curves_ref(fw, o, c.cls, fr), fw, c.cls, "atoms, fractions")
    cf = rf.curve_ptr.cpu().tolist()
    ks = rf.k.cpu().tolist()
    print(f"  fractions {fr}: k {ks}")
    assert ks == [k for n in sizes for k in UR.points_ref(n, fr)] and cf == [0, 4, 8, 12, 16]
    for g in range(c.B):
        for j in range(4):
            k = ks[cf[g] + j]
            assert torch.equal(rf.insertion[cf[g] + j], r.insertion[cp[g] + k]) and torch.equal(rf.deletion[cf[g] + j], r.deletion[cp[g] + k])


def test_group_scores_on_the_device_match_the_cpu(H):
    from hcatgnet_amd.subsets import group_scores
    c = _case("mixed")
    gen = torch.Generator().manual_seed(ROW_SEED)
    na, ea = torch.randn(c.x.shape, generator=gen), torch.randn(c.ei.shape[1], generator=gen)
    want, _ = group_scores(na, ea, c.ng, c.eg, _host_batch(c))
    got, gptr = group_scores(na.cuda(), ea.cuda(), c.ng.cuda(), c.eg.cuda(), _gpu_batch(H, c))
    print(f"\n  group_scores: {got.cpu().tolist()}")
    assert got.is_cuda and torch.equal(got.cpu(), want) and gptr.tolist() == [0, 0, 1, 4, 9]


# ------------------------------------------------------------------------------------------------ 6. edges
def test_no_rows_no_graphs_a_graph_without_groups_and_rows_per_graph(H):
    from hcatgnet_amd.subsets import AttributionCurves, SubsetValues
    c = _case("mixed")
    model = SR.model_from_params(H, c.params).cuda()
    sv = SubsetValues(model)
    gb = _gpu_batch(H, c)
    rows = UR.random_rows(14, 9, ROW_SEED).cuda()
    big = _clone(sv(gb, rows, **_kw(c)))
    # graph 0 has no group: every row is both outputs
    assert torch.equal(big[2][0], big[3][0])
    for s in range(14):
        assert torch.equal(big[0][s, 0], big[2][0])
    # rows_per_graph on the pool buffer the larger call has filled
    rp = [0, 14, 5, 1]
    part = sv(gb, rows, rows_per_graph=torch.tensor(rp), **_kw(c))
    assert sv.last_path == "fused"
    for g, n in enumerate(rp):
        assert torch.equal(part.values[:n, g], big[0][:n, g]) and float(part.values[n:, g].abs().sum()) == 0.0
    assert torch.equal(part.out_full, big[2]) and torch.equal(part.out_base, big[3])
    assert float(big[0][5:, 2].abs().min()) > 0.0
    # S = 0
    r0 = sv(gb, rows[:0], **_kw(c))
    assert sv.last_path == "fused" and tuple(r0.values.shape) == (0, 4, 1)
    assert torch.equal(r0.out_full, big[2]) and torch.equal(r0.out_base, big[3])
    # no graph at all
    e = H.Batch(c.x[:0].cuda(), c.ei[:, :0].cuda(), c.batch[:0].cuda(), 0, max_nodes=0, max_edges=0, edges_grouped=True)
    re = sv(e, torch.zeros(3, 0, dtype=torch.bool).cuda(), node_group=c.ng[:0].cuda())
    assert sv.last_path == "fused" and tuple(re.values.shape) == (3, 0, 1) and re.group_ptr.tolist() == [0]
    assert tuple(re.out_full.shape) == (0, 1) == tuple(re.out_base.shape)
    rc = AttributionCurves(model)(e, torch.zeros(0, dtype=torch.int32).cuda(), node_group=c.ng[:0].cuda())
    assert tuple(rc.insertion.shape) == (0, 1) and rc.curve_ptr.tolist() == [0] and rc.insertion_auc.numel() == 0


def test_a_graph_over_max_nodes_is_refused_and_the_others_keep_their_values(H):
    from hcatgnet_amd.subsets import SubsetValues
    c = _case("mixed")
    sizes = torch.bincount(c.batch, minlength=c.B)
    big = sizes == sizes.max()
    assert 0 < int(big.sum()) < c.B
    sv = SubsetValues(SR.model_from_params(H, c.params).cuda())
    rows = UR.random_rows(14, 9, ROW_SEED).cuda()
    honest = _clone(sv(_gpu_batch(H, c), rows, **_kw(c)))
    gb = _gpu_batch(H, c, max_nodes=int(sizes.max()) - 1)
    r = sv(gb, rows, rows_per_workgroup=3, **_kw(c))
    assert sv.last_path == "fused"
    torch.cuda.synchronize()
    status = gb._hcg_plan.status
    word = int(status[0].item())
    status.zero_()                                                    # (shared per device: leave it clean for the next test)
    assert word & SHAPE_LIMIT
    keep = (~big).cuda()
    assert torch.equal(r.values[:, keep], honest[0][:, keep]) and float(r.values[:, big.cuda()].abs().max()) == 0.0
    assert torch.equal(r.out_full[keep], honest[2][keep]) and torch.equal(r.out_base[keep], honest[3][keep])
    assert float(r.out_full[big.cuda()].abs().max()) == 0.0 and float(r.out_base[big.cuda()].abs().max()) == 0.0
    assert float(honest[0][:, big.cuda()].abs().min()) > 0.0


def test_a_model_outside_the_limits_takes_the_loop_with_the_same_bounds(H):
    """D = 128: one masked forward of the whole batch per row on `ExplainStep`'s any-shape path."""
    from hcatgnet_amd.subsets import AttributionCurves, SubsetValues, ranking
    c = _synth_case(dict(num_graphs=3, nodes=8, extra_bonds=2, max_degree=4, feat=6, nodes_jitter=2), 0.5, {}, 1, 3)
    c.params = SR.rand_params(6, 128, seed=PARAM_SEED, n_classes=2)
    model = SR.model_from_params(H, c.params).cuda()
    before = [q.detach().clone() for q in model.parameters()]
    sv = SubsetValues(model)
    gb = _gpu_batch(H, c)
    assert "shape" in sv.reason(gb)
    fw = UR.Forwards(c.params, c.x, c.ei, c.batch, c.B, c.ng, c.eg)
    rows = UR.random_rows(8, int(fw.gptr[-1]), ROW_SEED)
    r = sv(gb, rows.cuda(), **_kw(c))
    assert sv.last_path == "loop"
    UR.check_values(r, UR.values_ref(fw, rows), fw, "D = 128 (loop)")
    ac = AttributionCurves(model)
    order = ranking(torch.arange(int(fw.gptr[-1]), dtype=torch.float32).cuda(), fw.gptr.cuda())
    rc = ac(gb, order, class_index=c.cls, **_kw(c))
    assert ac.last_path == "loop"
    UR.check_curves(rc, UR.curves_ref(fw, order.flatten().cpu().tolist(), c.cls), fw, c.cls, "D = 128 (loop)")
    for q, b in zip(model.parameters(), before):
        assert torch.equal(q.detach(), b) and q.grad is None
