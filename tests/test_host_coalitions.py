"""Host side of `CoalitionValues` (no GPU): the loop path on CPU tensors against the fp64 table, Shapley values and
interaction indices of tests/coalition_ref.py (which states the references and the bounds), the two derivation functions on
a reference table, the argument checks, and the HCG_EXPLAIN_COALITIONS mode and `coal_` overlay of hcg_explain_args.  Every
figure is printed before it is asserted (`pytest -s`)."""
import ctypes
import os

import pytest
import torch

import hcatgnet_amd as H
from hcatgnet_amd import _lib
from hcatgnet_amd.shapley import (MAX_COALITION_GROUPS, CoalitionValues, ShapleySampling, interactions_from_coalitions,
                                  shapley_from_coalitions)
from tests import coalition_ref as CR
from tests import shapley_ref as SR


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
    c.params = SR.rand_params(25, 64, n_conv=2, n_read=2, n_classes=2, seed=23)
    c.cls = 1
    c.refs, c.gptr = CR.reference_batch(c.params, c.x, c.ei, c.batch, c.B, c.ng, c.eg, c.cls)
    cv = CoalitionValues(SR.model_from_params(H, c.params))
    assert "CPU" in cv.reason(_batch(c))
    c.r = cv(_batch(c), node_group=c.ng, edge_group=c.eg, class_index=c.cls)
    assert cv.last_path == "loop" and isinstance(c.r, H.CoalitionResult)
    return c


# ------------------------------------------------------------------------------------------------ the loop on CPU tensors
def test_loop_matches_the_fp64_table_shapley_values_and_interactions(mixed):
    c = mixed
    assert (c.gptr[1:] - c.gptr[:-1]).tolist() == [0, 1, 3, 5]
    print(f"\n  mixed: B {c.B} N {c.x.shape[0]} E {c.ei.shape[1]} groups {(c.gptr[1:] - c.gptr[:-1]).tolist()} rows {c.r.values.shape[0]}")
    CR.check_against_reference(c.r, c.refs, c.gptr, c.cls, "loop, CPU tensors")
    assert c.r.values.shape[0] == 1 + 2 + 8 + 32
    # a graph without groups: one row, both outputs
    assert torch.equal(c.r.values[0], c.r.out_full[0]) and torch.equal(c.r.values[0], c.r.out_base[0])


def test_rows_that_differ_only_in_the_dead_group_are_equal(mixed):
    c = mixed
    g, y = c.dead
    assert [(~q["live"]).nonzero().flatten().tolist() for q in c.refs] == [[], [], [], [y]]
    pairs = CR.check_dead_rows(c.r, c.refs, c.gptr)
    print(f"\n  dead group {y} of graph {g}: {pairs} pairs of rows equal")
    assert pairs == 16
    assert float(c.r.group_attr[int(c.gptr[g]) + y]) == 0.0


def test_derivations_on_the_reference_table(mixed):
    c = mixed
    values = torch.cat([q["table"] for q in c.refs]).to(torch.float32)
    tptr, gptr = c.r.table_ptr, c.r.group_ptr
    for cls in (0, 1):
        phi = shapley_from_coalitions(values, tptr, gptr, cls)
        inter, pptr = interactions_from_coalitions(values, tptr, gptr, cls)
        assert phi.dtype == inter.dtype == torch.float32 and torch.equal(pptr, c.r.pair_ptr)
        worst = [0.0, 0.0]
        for g, ref in enumerate(c.refs):
            G = int(c.gptr[g + 1] - c.gptr[g])
            v = ref["table"][:, cls]
            e_a = float((phi[int(gptr[g]):int(gptr[g + 1])].double() - CR.shapley_graph(v, G)).abs().max()) if G else 0.0
            e_i = float((inter[int(pptr[g]):int(pptr[g + 1])].double().view(G, G) - CR.interactions_graph(v, G)).abs().max()) if G else 0.0
            worst = [max(worst[0], e_a / (2 * SR.TOL * ref["scale"])), max(worst[1], e_i / (4 * SR.TOL * ref["scale"]))]
        print(f"\n  derivations, class {cls}: worst figure / bound  attr {worst[0]:.4f}  inter {worst[1]:.4f}")
        assert worst[0] <= 1.0 and worst[1] <= 1.0
    # the other class without a second evaluation is what the call returned for it
    assert torch.equal(shapley_from_coalitions(c.r.values, tptr, gptr, c.cls), c.r.group_attr)
    assert torch.equal(interactions_from_coalitions(c.r.values, tptr, gptr, c.cls)[0], c.r.interaction)


def test_two_groups_interact_by_the_four_corner_difference():
    v = torch.tensor([[0.25], [1.5], [-0.75], [3.125]], dtype=torch.float32)
    tptr, gptr = torch.tensor([0, 4]), torch.tensor([0, 2])
    inter, pptr = interactions_from_coalitions(v, tptr, gptr, 0)
    d = v.double()[:, 0]
    want = float(d[3] - d[1] - d[2] + d[0])
    print(f"\n  G = 2: I_01 {float(inter[1])} want {want}")
    assert pptr.tolist() == [0, 4] and inter.tolist() == [0.0, want, want, 0.0]
    phi = shapley_from_coalitions(v, tptr, gptr, 0)
    assert phi.tolist() == [0.5 * float(d[1] - d[0]) + 0.5 * float(d[3] - d[2]), 0.5 * float(d[2] - d[0]) + 0.5 * float(d[3] - d[1])]


# ------------------------------------------------------------------------------------------------ arguments
def test_seventeen_groups_on_one_graph_are_refused():
    x = torch.ones(17, 2)
    b = H.Batch(x, torch.zeros(2, 0, dtype=torch.int64), torch.zeros(17, dtype=torch.long), 1, max_nodes=17, max_edges=0, edges_grouped=True)
    cv = CoalitionValues(H.make_network("GCN", H.default_options(), 2))
    assert MAX_COALITION_GROUPS == 16
    with pytest.raises(ValueError, match=r"17.*16"):
        cv(b, node_group=torch.arange(17))
    with pytest.raises(ValueError, match=r"17.*16"):
        cv.loop(b, node_group=torch.arange(17))


def test_a_table_over_the_budget_says_to_split_the_batch(monkeypatch):
    from hcatgnet_amd import attribution
    c = CR.mixed_case()
    monkeypatch.setattr(attribution, "LAUNCH_BUDGET_BYTES", 43 * 4 - 1)
    with pytest.raises(ValueError, match="split the batch"):
        CoalitionValues(H.make_network("GCN", H.default_options(), 25))(_batch(c), node_group=c.ng, edge_group=c.eg)


def test_bad_ids_raise_what_shapley_sampling_raises():
    c = CR.mixed_case()
    b = _batch(c)
    model = H.make_network("GCN", H.default_options(), 25)
    cv, sv = CoalitionValues(model), ShapleySampling(model)
    ok = CR.fragments(c.batch, c.B, 3)
    gap = ok.clone(); gap[ok == 1] = 5
    low = ok.clone(); low[0] = -2
    for kw in (dict(node_group=gap), dict(node_group=low), dict(node_group=ok.float()), dict(node_group=ok[:-1]),
               dict(edge_group=torch.zeros(c.ei.shape[1] - 1, dtype=torch.int64)), dict(node_group=ok, edge_group=c.eg + 9)):
        with pytest.raises(ValueError) as mine:
            cv(b, **kw)
        with pytest.raises(ValueError) as theirs:
            sv(b, n_samples=1, **kw)
        assert str(mine.value) == str(theirs.value)
    with pytest.raises(ValueError):
        cv(b, node_group=ok, class_index=1)
    with pytest.raises(ValueError, match="give node_group, edge_group or both"):
        cv(b)


def test_launch_size_defaults():
    spw, jpl = CoalitionValues.default_subsets_per_workgroup, CoalitionValues.default_jobs_per_launch
    assert spw(535 * 64) == 16 and spw(1024) == 1 and spw(1) == 1 and spw(52 * 4096) == 16
    assert jpl(16) == 64 * 256 and jpl(1 << 16) == 256


# ------------------------------------------------------------------------------------------------ ABI
def _query(nodes=184, edges=390, rows=0, max_live=0, flags=None, **ptrs):
    a = _lib.ExplainArgs()
    a.mode = _lib.HCG_EXPLAIN_COALITIONS
    a.flags = _lib.HCG_EXPLAIN_QUERY if flags is None else flags
    a.F, a.D, a.C, a.n_conv, a.R = 25, 64, 1, 2, 2
    a.max_nodes, a.max_edges, a.N, a.E, a.B = nodes, edges, nodes, edges, 1
    a.coal_rows, a.coal_max_live = rows, max_live
    for k, v in ptrs.items():
        setattr(a, k, v)
    rc = _lib.load().hcg_explain(ctypes.addressof(a), None)
    return rc, int(a.workspace_bytes_needed), int(a.lds_bytes)


def test_struct_size_mode_and_overlay_offsets():
    # 608: sizeof(hcg_explain_args) before this mode existed
    assert ctypes.sizeof(_lib.ExplainArgs) == 608 == _lib.load().hcg_struct_bytes(_lib.HCG_STRUCT_EXPLAIN_ARGS)
    header = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "hcatgnet_hip.h")).read()
    assert _lib.HCG_EXPLAIN_COALITIONS == 7 and "#define HCG_EXPLAIN_COALITIONS 7" in header
    base = _lib.ExplainArgs.fit_edge_logit.offset
    assert _lib.ExplainArgs.shap_n_groups.offset == base + 40
    at = base + 48
    for name, ctype in _lib.COALITION_FIELDS:
        f = getattr(_lib.ExplainArgs, name)
        assert f.offset == at and f.size == ctypes.sizeof(ctype) and name in header, name
        at += f.size
    assert at <= 608


def test_query_takes_the_shapley_limits_and_reports_lds():
    from hcatgnet_amd import _frozen
    assert _lib.HCG_EXPLAIN_COALITIONS in _frozen._MODES
    a = _lib.ExplainArgs()
    a.mode, a.flags = _lib.HCG_EXPLAIN_SHAPLEY, _lib.HCG_EXPLAIN_QUERY
    a.F, a.D, a.C, a.n_conv, a.R, a.max_nodes, a.max_edges, a.N, a.E, a.B, a.perm_count = 25, 64, 1, 2, 2, 184, 390, 184, 390, 1, 1
    assert _lib.load().hcg_explain(ctypes.addressof(a), None) == 0
    rc, ws, lds = _query()
    print(f"\n  coalitions query at 184 nodes: rc {rc} workspace {ws} lds {lds} (the walk's {int(a.lds_bytes)})")
    assert rc == 0 and ws == 0 and lds == int(a.lds_bytes) > 0
    assert _query(nodes=185)[0] == -3 and _query(edges=1025)[0] == -3
    assert _query(max_live=16, rows=(1 << 31) - 1)[0] == 0
    assert _query(max_live=17)[0] == -3 and _query(rows=1 << 31)[0] == -3
    for name in ("edge_mask", "node_mask", "target", "dout", "perm"):
        assert _query(**{name: 8})[0] == -1, name
    Q = _lib.HCG_EXPLAIN_QUERY
    assert _query(flags=Q | _lib.HCG_EXPLAIN_GROUPED)[0] == -1 and _query(flags=Q | _lib.HCG_EXPLAIN_TARGET_CLASS)[0] == -1
    cv = CoalitionValues(H.make_network("GCN", H.default_options(), 25))
    assert cv.reason() is None


def test_exports_and_pointers_to_the_exact_path():
    for name in ("CoalitionValues", "CoalitionResult", "shapley_from_coalitions", "interactions_from_coalitions"):
        assert getattr(H, name) is not None and name in H.__all__
    assert "CoalitionValues" in H.shapley.all_group_permutations.__doc__
