"""Host side of `SubsetValues` / `AttributionCurves` (no GPU): the bit packing against Python ints, the loop path on CPU
tensors against the fp64 references of tests/subsets_ref.py (which states the references and the bounds), `ranking`,
`group_scores`, the areas and the points of the curves, the argument checks, and the HCG_EXPLAIN_SUBSETS mode and `sub_`
overlay of hcg_explain_args.  Every figure is printed before it is asserted (`pytest -s`)."""
import ctypes
import os

import pytest
import torch

import hcatgnet_amd as H
from hcatgnet_amd import _lib, subsets
from hcatgnet_amd.shapley import CoalitionValues, ShapleySampling
from hcatgnet_amd.subsets import AttributionCurves, SubsetValues, group_scores, pack_subsets, ranking
from tests import coalition_ref as CR
from tests import shapley_ref as SR
from tests import subsets_ref as UR

PARAM_SEED, ROW_SEED = 23, 11


@pytest.fixture(scope="module", autouse=True)
def built():
    if not os.path.isfile(_lib.LIB_PATH):
        import __graft_entry__
        __graft_entry__.build()


def _batch(c):
    return H.Batch(c.x, c.ei, c.batch, c.B, max_nodes=c.max_nodes, max_edges=c.max_edges, edges_grouped=True)


@pytest.fixture(scope="module")
def mixed():
    c = CR.mixed_case()
    c.params = SR.rand_params(25, 64, n_conv=2, n_read=2, n_classes=2, seed=PARAM_SEED)
    c.cls = 1
    c.model = SR.model_from_params(H, c.params)
    c.fw = UR.Forwards(c.params, c.x, c.ei, c.batch, c.B, c.ng, c.eg)
    return c


@pytest.fixture(scope="module")
def bonds():
    """three small graphs, atoms plus bonds as players"""
    c = UR.sized_case((6, 9, 12), feat=7)
    c.x = CR.sparse_x(c.x, 0.5)
    b = _batch(c)
    c.ng = H.atom_groups(b)
    c.eg = H.bond_groups(b, first=torch.bincount(c.batch, minlength=c.B))
    c.params = SR.rand_params(7, 64, n_conv=2, n_read=2, n_classes=1, seed=PARAM_SEED)
    c.cls = 0
    c.model = SR.model_from_params(H, c.params)
    c.fw = UR.Forwards(c.params, c.x, c.ei, c.batch, c.B, c.ng, c.eg)
    return c


# ------------------------------------------------------------------------------------------------ packing
def test_pack_subsets_matches_python_ints():
    counts = [0, 1, 31, 32, 33, 70]
    gptr = torch.tensor([0] + counts).cumsum(0)
    G = int(gptr[-1])
    rows = UR.random_rows(9, G, ROW_SEED)
    bits, wptr = pack_subsets(rows, gptr)
    want, want_ptr = UR.pack_ref(rows, gptr.tolist())
    print(f"\n  groups {counts}: word_ptr {wptr.tolist()} (W = {bits.shape[1]})")
    assert bits.dtype == torch.int32 and wptr.dtype == torch.int32 and wptr.tolist() == want_ptr == [0, 0, 1, 2, 3, 5, 8]
    got = [[int(v) & 0xFFFFFFFF for v in row] for row in bits.tolist()]
    assert got == want
    # the all-on row: 1, 31 and 32 groups fill one word each, 33 spill one bit, 70 leave six in their third word
    assert want[1] == [1, (1 << 31) - 1, (1 << 32) - 1, (1 << 32) - 1, 1, (1 << 32) - 1, (1 << 32) - 1, 63]
    # S = 0 and G = 0
    b0, w0 = pack_subsets(rows[:0], gptr)
    assert tuple(b0.shape) == (0, 8) and w0.tolist() == want_ptr
    b1, w1 = pack_subsets(torch.zeros(2, 0, dtype=torch.bool), torch.tensor([0, 0]))
    assert tuple(b1.shape) == (2, 0) and w1.tolist() == [0, 0]
    for bad in (rows.float(), rows[0]):
        with pytest.raises(ValueError):
            pack_subsets(bad, gptr)
    with pytest.raises(ValueError):
        pack_subsets(rows, gptr[:-1])


# ------------------------------------------------------------------------------------------------ the loop on CPU tensors
@pytest.mark.parametrize("name", ["mixed", "bonds"])
def test_loop_matches_the_fp64_values(name, request):
    c = request.getfixturevalue(name)
    sv = SubsetValues(c.model)
    assert "CPU" in sv.reason(_batch(c)) and sv.reason() is None
    G = int(c.fw.gptr[-1])
    rows = UR.random_rows(8, G, ROW_SEED)
    r = sv(_batch(c), rows, node_group=c.ng, edge_group=c.eg)
    assert sv.last_path == "loop" and isinstance(r, H.SubsetResult)
    counts = (c.fw.gptr[1:] - c.fw.gptr[:-1]).tolist()
    print(f"\n  {name}: B {c.B} N {c.x.shape[0]} E {c.ei.shape[1]} groups {counts}")
    assert counts == ([0, 1, 3, 5] if name == "mixed" else [6 + 8, 9 + 11, 12 + 14])
    UR.check_values(r, UR.values_ref(c.fw, rows), c.fw, f"{name} (loop, CPU tensors)")
    assert torch.equal(r.values[0], r.out_base) and torch.equal(r.values[1], r.out_full)
    # S = 0 still returns the two outputs
    r0 = sv(_batch(c), rows[:0], node_group=c.ng, edge_group=c.eg)
    assert tuple(r0.values.shape) == (0, c.B, r.values.shape[2]) and torch.equal(r0.out_full, r.out_full) and torch.equal(r0.out_base, r.out_base)
    # rows_per_graph: the other rows exactly 0, the rest unchanged
    rp = torch.tensor([(3 * g + 2) % 9 for g in range(c.B)])
    rr = sv(_batch(c), rows, node_group=c.ng, edge_group=c.eg, rows_per_graph=rp)
    for g in range(c.B):
        assert torch.equal(rr.values[:int(rp[g]), g], r.values[:int(rp[g]), g]) and float(rr.values[int(rp[g]):, g].abs().sum()) == 0.0
    assert torch.equal(rr.out_full, r.out_full) and torch.equal(rr.out_base, r.out_base)


def test_loop_rows_are_the_rows_of_the_coalition_loop(mixed):
    c = mixed
    counts = (c.fw.gptr[1:] - c.fw.gptr[:-1]).tolist()
    S = 1 << max(counts)
    rows = torch.zeros(S, int(c.fw.gptr[-1]), dtype=torch.bool)
    for g, G in enumerate(counts):
        for y in range(G):
            rows[:, int(c.fw.gptr[g]) + y] = (torch.arange(S) >> y) & 1 == 1
    r = SubsetValues(c.model).loop(_batch(c), rows, c.ng, c.eg, rows_per_graph=torch.tensor([1 << G for G in counts]))
    t = CoalitionValues(c.model).loop(_batch(c), c.ng, c.eg, c.cls)
    for g, G in enumerate(counts):
        a = int(t.table_ptr[g])
        assert torch.equal(r.values[:1 << G, g], t.values[a:a + (1 << G)]), g
        assert float(r.values[1 << G:, g].abs().sum()) == 0.0
    assert torch.equal(r.out_full, t.out_full) and torch.equal(r.out_base, t.out_base)
    print(f"\n  {sum(1 << G for G in counts)} rows equal the coalition loop's")


@pytest.mark.parametrize("name", ["mixed", "bonds"])
def test_curves_on_cpu_tensors_match_the_fp64_curves(name, request):
    c = request.getfixturevalue(name)
    G = int(c.fw.gptr[-1])
    scores = torch.randn(G, generator=torch.Generator().manual_seed(ROW_SEED))
    order = ranking(scores, c.fw.gptr)
    ac = AttributionCurves(c.model)
    assert "CPU" in ac.reason(_batch(c))
    r = ac(_batch(c), order, node_group=c.ng, edge_group=c.eg, class_index=c.cls)
    assert ac.last_path == "loop" and isinstance(r, H.CurveResult)
    counts = (c.fw.gptr[1:] - c.fw.gptr[:-1]).tolist()
    assert (r.curve_ptr[1:] - r.curve_ptr[:-1]).tolist() == [G_g + 1 for G_g in counts]
    UR.check_curves(r, UR.curves_ref(c.fw, order.flatten().tolist(), c.cls), c.fw, c.cls, f"{name} (loop)")
    fr = [0, 0.1, 0.5, 0.5, 1]
    rf = ac(_batch(c), order.flatten(), node_group=c.ng, edge_group=c.eg, class_index=c.cls, fractions=fr)
    UR.check_curves(rf, UR.curves_ref(c.fw, order.flatten().tolist(), c.cls, fr), c.fw, c.cls, f"{name} (loop, fractions)")
    # the ends of the curves are the two outputs, and a fraction's point is the full curve's point at that k
    cp, cf = r.curve_ptr.tolist(), rf.curve_ptr.tolist()
    for g, G_g in enumerate(counts):
        assert torch.equal(r.insertion[cp[g]], r.out_base[g]) and torch.equal(r.deletion[cp[g + 1] - 1], r.out_base[g])
        assert torch.equal(r.deletion[cp[g]], r.out_full[g]) and torch.equal(r.insertion[cp[g + 1] - 1], r.out_full[g])
        for j in range(len(fr)):
            k = int(rf.k[cf[g] + j])
            assert torch.equal(rf.insertion[cf[g] + j], r.insertion[cp[g] + k]) and torch.equal(rf.deletion[cf[g] + j], r.deletion[cp[g] + k])


# ------------------------------------------------------------------------------------------------ ranking, group_scores, areas, points
def test_ranking_ties_abs_and_graphs_without_groups():
    gptr = torch.tensor([0, 0, 4, 4, 7])
    scores = torch.tensor([0.5, 2.0, 0.5, -3.0, 1.0, 1.0, -1.0])
    got = ranking(scores, gptr)
    assert got.dtype == torch.int32 and tuple(got.shape) == (1, 7)
    assert got.tolist() == [[1, 0, 2, 3, 0, 1, 2]]                          # ties: the lower id first
    assert ranking(scores, gptr, by="abs").tolist() == [[3, 1, 0, 2, 0, 1, 2]]
    assert ranking(scores, gptr, descending=False).tolist() == [[3, 0, 2, 1, 2, 0, 1]]
    assert tuple(ranking(scores[:0], torch.tensor([0, 0])).shape) == (1, 0)
    with pytest.raises(ValueError):
        ranking(scores, gptr, by="rank")


def test_group_scores_against_a_loop(mixed):
    c = mixed
    gen = torch.Generator().manual_seed(ROW_SEED)
    na, ea = torch.randn(c.x.shape, generator=gen), torch.randn(c.ei.shape[1], generator=gen)
    got, gptr = group_scores(na, ea, c.ng, c.eg, _batch(c))
    assert got.dtype == torch.float32 and torch.equal(gptr, c.fw.gptr)
    nptr, eptr = SR.pointers(c.batch, c.ei, c.B)
    want = torch.zeros(int(gptr[-1]), dtype=torch.float64)
    for g in range(c.B):
        for i in range(int(nptr[g]), int(nptr[g + 1])):
            for f in range(c.F):
                if int(c.ng[i, f]) >= 0:
                    want[int(gptr[g]) + int(c.ng[i, f])] += float(na[i, f])
        for e in range(int(eptr[g]), int(eptr[g + 1])):
            if int(c.eg[e]) >= 0:
                want[int(gptr[g]) + int(c.eg[e])] += float(ea[e])
    err = float((got.double() - want).abs().max())
    print(f"\n  group_scores: {got.numel()} groups, worst error {err:.3e} (scale {float(want.abs().max()):.3f})")
    assert err <= 2.0 ** -23 * float(want.abs().max())                      # float64 sums, one float32 rounding
    only_nodes, _ = group_scores(na, None, c.ng, c.eg, _batch(c))
    only_edges, _ = group_scores(None, ea, c.ng, c.eg, _batch(c))
    assert float((only_nodes.double() + only_edges.double() - want).abs().max()) <= 2.0 ** -22 * float(want.abs().max())
    with pytest.raises(ValueError):
        group_scores(na[:-1], ea, c.ng, c.eg, _batch(c))


def test_auc_on_a_hand_made_table(monkeypatch):
    """One graph of four atoms; v(S) = sum of w_y over S + 1: the curves are prefix sums, the areas known in closed form."""
    w = torch.tensor([4.0, 2.0, 1.0, 0.5])
    x = torch.ones(4, 1)
    b = H.Batch(x, torch.zeros(2, 0, dtype=torch.int64), torch.zeros(4, dtype=torch.long), 1, max_nodes=4, max_edges=0, edges_grouped=True)
    ac = AttributionCurves(H.make_network("GCN", H.default_options(), 1))

    def table(batch, gr, counts, rows, rp, rpw, why):
        S = rows.shape[0]
        full = torch.cat([rows, torch.ones(1, 4, dtype=torch.bool), torch.zeros(1, 4, dtype=torch.bool)])
        assert rp == [6] and S == 6
        return (full.float() @ w + 1.0).reshape(S + 2, 1, 1)
    monkeypatch.setattr(ac.values, "_table", table)
    r = ac(b, torch.tensor([0, 1, 2, 3], dtype=torch.int32), node_group=torch.arange(4))
    assert r.k.tolist() == [0, 1, 2, 3, 4] and r.curve_ptr.tolist() == [0, 5]
    assert r.insertion[:, 0].tolist() == [1.0, 5.0, 7.0, 8.0, 8.5] and r.deletion[:, 0].tolist() == [8.5, 4.5, 2.5, 1.5, 1.0]
    ins = 0.25 * ((1 + 5) / 2 + (5 + 7) / 2 + (7 + 8) / 2 + (8 + 8.5) / 2)
    dele = 0.25 * ((8.5 + 4.5) / 2 + (4.5 + 2.5) / 2 + (2.5 + 1.5) / 2 + (1.5 + 1.0) / 2)
    print(f"\n  areas: insertion {float(r.insertion_auc[0])} (want {ins}), deletion {float(r.deletion_auc[0])} (want {dele})")
    assert float(r.insertion_auc[0]) == ins and float(r.deletion_auc[0]) == dele
    assert r.out_full.tolist() == [[8.5]] and r.out_base.tolist() == [[1.0]]
    # the reversed order swaps what the curves see
    rev = ac(b, torch.tensor([[3, 2, 1, 0]], dtype=torch.int32), node_group=torch.arange(4))
    assert rev.insertion[:, 0].tolist() == [1.0, 1.5, 2.5, 4.5, 8.5]


def test_fractions_pick_k_by_rounding_half_up():
    """[0, 0.1, 0.5, 1] at G_g = 1, 5, 6: floor(f G + 0.5)"""
    sizes = [1, 5, 6]
    x = torch.ones(sum(sizes), 2)
    bv = torch.repeat_interleave(torch.arange(3), torch.tensor(sizes))
    b = H.Batch(x, torch.zeros(2, 0, dtype=torch.int64), bv, 3, max_nodes=6, max_edges=0, edges_grouped=True)
    ac = AttributionCurves(H.make_network("GCN", H.default_options(), 2))
    order = torch.cat([torch.arange(n, dtype=torch.int32) for n in sizes])
    r = ac(b, order, node_group=H.atom_groups(b), fractions=[0, 0.1, 0.5, 1])
    print(f"\n  k {r.k.tolist()}")
    assert r.k.tolist() == [0, 0, 1, 1, 0, 1, 3, 5, 0, 1, 3, 6] and r.curve_ptr.tolist() == [0, 4, 8, 12]
    assert r.k.tolist() == [k for n in sizes for k in UR.points_ref(n, [0, 0.1, 0.5, 1])]
    # duplicates are kept, and are the same row
    assert torch.equal(r.insertion[0], r.insertion[1]) and torch.equal(r.deletion[2], r.deletion[3])


# ------------------------------------------------------------------------------------------------ arguments
def test_every_value_error(mixed, monkeypatch):
    c = mixed
    b = _batch(c)
    G = int(c.fw.gptr[-1])
    rows = UR.random_rows(4, G, ROW_SEED)
    sv, ac, ss = SubsetValues(c.model), AttributionCurves(c.model), ShapleySampling(c.model)
    kw = dict(node_group=c.ng, edge_group=c.eg)
    for bad in (rows.to(torch.int32), rows[:, :-1], rows[0], rows.tolist()):
        with pytest.raises(ValueError, match="subsets must be a bool tensor"):
            sv(b, bad, **kw)
    for bad in (torch.tensor([1, 1, 1]), torch.tensor([1.0, 1, 1, 1]), torch.tensor([1, 1, 1, 5]), torch.tensor([1, 1, 1, -1]), [1, 1, 1, 1]):
        with pytest.raises(ValueError, match="rows_per_graph"):
            sv(b, rows, rows_per_graph=bad, **kw)
    # the group arguments: `ShapleySampling`'s checks and messages
    ok = CR.fragments(c.batch, c.B, 3)
    gap = ok.clone(); gap[ok == 1] = 5
    for gkw in (dict(node_group=gap), dict(node_group=ok.float()), dict(node_group=ok[:-1])):
        with pytest.raises(ValueError) as mine:
            sv(b, rows, **gkw)
        with pytest.raises(ValueError) as curves:
            ac(b, torch.zeros(G, dtype=torch.int32), **gkw)
        with pytest.raises(ValueError) as theirs:
            ss(b, n_samples=1, **gkw)
        assert str(mine.value) == str(curves.value) == str(theirs.value)
    with pytest.raises(ValueError, match="give node_group, edge_group or both"):
        sv(b, rows)
    with pytest.raises(ValueError, match="give node_group, edge_group or both"):
        ac(b, torch.zeros(G, dtype=torch.int32))
    # order: a repeated id, an id of another graph's range, a wrong length, a wrong dtype
    good = ranking(torch.zeros(G), c.fw.gptr).flatten()
    assert good.tolist() == [0, 0, 1, 2, 0, 1, 2, 3, 4]
    ac(b, good, **kw)
    rep = good.clone(); rep[2] = 0
    far = good.clone(); far[3] = 4                                          # graph 2 has ids 0 .. 2; 4 is graph 3's
    neg = good.clone(); neg[0] = -1
    for bad in (rep, far, neg):
        with pytest.raises(ValueError, match="permutation"):
            ac(b, bad, **kw)
    for bad in (good[:-1], good.long(), good.reshape(G, 1), good.tolist()):
        with pytest.raises(ValueError, match="order must be an int32 tensor"):
            ac(b, bad, **kw)
    for bad in ([0.5, 0.25], [-0.1, 1], [0, 1.5], [], "ab"):
        with pytest.raises(ValueError, match="fractions"):
            ac(b, good, fractions=bad, **kw)
    for cls in (-1, 2):
        with pytest.raises(ValueError, match="class_index"):
            ac(b, good, class_index=cls, **kw)
    with pytest.raises(ValueError, match="rows_per_workgroup"):
        sv(b, rows, rows_per_workgroup=0, **kw)
    # the table over the budget says to split
    from hcatgnet_amd import attribution
    monkeypatch.setattr(attribution, "LAUNCH_BUDGET_BYTES", (4 + 2) * c.B * 2 * 4 - 1)
    with pytest.raises(ValueError, match="split"):
        sv(b, rows, **kw)
    monkeypatch.setattr(attribution, "LAUNCH_BUDGET_BYTES", (4 + 2) * c.B * 2 * 4)
    sv(b, rows, **kw)


# ------------------------------------------------------------------------------------------------ ABI
def _query(nodes=184, edges=390, rows=0, max_groups=0, flags=None, **ptrs):
    a = _lib.ExplainArgs()
    a.mode = _lib.HCG_EXPLAIN_SUBSETS
    a.flags = _lib.HCG_EXPLAIN_QUERY if flags is None else flags
    a.F, a.D, a.C, a.n_conv, a.R = 25, 64, 1, 2, 2
    a.max_nodes, a.max_edges, a.N, a.E, a.B = nodes, edges, nodes, edges, 1
    a.coal_rows, a.sub_max_groups = rows, max_groups
    for k, v in ptrs.items():
        setattr(a, k, v)
    rc = _lib.load().hcg_explain(ctypes.addressof(a), None)
    return rc, int(a.workspace_bytes_needed), int(a.lds_bytes)


def test_struct_size_mode_and_overlay_offsets():
    assert ctypes.sizeof(_lib.ExplainArgs) == 608 == _lib.load().hcg_struct_bytes(_lib.HCG_STRUCT_EXPLAIN_ARGS)
    header = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "hcatgnet_hip.h")).read()
    assert _lib.HCG_EXPLAIN_SUBSETS == 8 and "#define HCG_EXPLAIN_SUBSETS 8" in header
    base = _lib.ExplainArgs.fit_edge_logit.offset
    # every earlier member where it was
    assert _lib.ExplainArgs.shap_n_groups.offset == base + 40 and _lib.ExplainArgs.coal_values.offset == base + 48
    assert _lib.ExplainArgs.coal_reserved.offset == base + 92
    at = base + 96
    for name, ctype in _lib.SUBSET_FIELDS:
        f = getattr(_lib.ExplainArgs, name)
        assert f.offset == at and f.size == ctypes.sizeof(ctype) and name in header, name
        at += f.size
    print(f"\n  the sub_ fields end at byte {at} of 608")
    assert at <= 608
    assert [n for n, _ in _lib.SUBSET_FIELDS] == ["sub_bits", "sub_word_ptr", "sub_member_group", "sub_max_groups", "sub_reserved"]


def test_query_takes_the_shapley_limits_and_reports_lds():
    from hcatgnet_amd import _frozen
    assert _lib.HCG_EXPLAIN_SUBSETS in _frozen._MODES
    a = _lib.ExplainArgs()
    a.mode, a.flags = _lib.HCG_EXPLAIN_SHAPLEY, _lib.HCG_EXPLAIN_QUERY
    a.F, a.D, a.C, a.n_conv, a.R, a.max_nodes, a.max_edges, a.N, a.E, a.B, a.perm_count = 25, 64, 1, 2, 2, 184, 390, 184, 390, 1, 1
    assert _lib.load().hcg_explain(ctypes.addressof(a), None) == 0
    rc, ws, lds = _query()
    print(f"\n  subsets query at 184 nodes: rc {rc} workspace {ws} lds {lds} (the walk's {int(a.lds_bytes)})")
    assert rc == 0 and ws == 0 and lds == int(a.lds_bytes) > 0
    assert _query(nodes=185)[0] == -3 and _query(edges=1025)[0] == -3
    assert subsets.MAX_SUBSET_GROUPS == 16384
    assert _query(max_groups=16384, rows=(1 << 31) - 1)[0] == 0
    assert _query(max_groups=16385)[0] == -3 and _query(rows=1 << 31)[0] == -3
    for name in ("edge_mask", "node_mask", "target", "dout", "perm"):
        assert _query(**{name: 8})[0] == -1, name
    Q = _lib.HCG_EXPLAIN_QUERY
    assert _query(flags=Q | _lib.HCG_EXPLAIN_GROUPED)[0] == -1 and _query(flags=Q | _lib.HCG_EXPLAIN_TARGET_CLASS)[0] == -1
    sv = SubsetValues(H.make_network("GCN", H.default_options(), 25))
    assert sv.reason() is None


def test_a_launch_with_null_arrays_is_refused_before_the_gpu_is_touched():
    """flags = 0 (a launch): negative counts and every missing array are HCG_ERR_INVALID_ARG, whether or not a GPU is visible."""
    assert _query(flags=0, rows=-1)[0] == -1 and _query(flags=0, max_groups=-1)[0] == -1
    assert _query(flags=0, coal_job_count=-1)[0] == -1 and _query(flags=0, coal_job_first=-1)[0] == -1
    assert _query(flags=0, coal_job_count=0)[0] == 0                          # nothing to run
    assert _query(flags=0, coal_job_count=1, rows=1)[0] == -1                 # every array NULL


def test_exports():
    for name in ("SubsetValues", "SubsetResult", "AttributionCurves", "CurveResult", "pack_subsets", "ranking", "group_scores"):
        assert getattr(H, name) is not None and name in H.__all__
    assert "fidelity" in AttributionCurves.__doc__
