"""Host side of grouped Shapley value sampling (no GPU): the HCG_EXPLAIN_GROUPED flag and the `shap_` overlay of
hcg_explain_args, the grouped query, the helpers that build groups and group permutations, the id validation, and
`ShapleySampling`'s loop on CPU tensors against the fp64 group walk (tests/shapley_groups_ref.py states the reference and
the bounds).  Every figure is printed before it is asserted (`pytest -s`)."""
import ctypes
import math
import os

import pytest
import torch

import hcatgnet_amd as H
from hcatgnet_amd import _lib, synth
from tests import shapley_groups_ref as GR
from tests import shapley_ref as SR


@pytest.fixture(scope="module", autouse=True)
def built():
    if not os.path.isfile(_lib.LIB_PATH):
        import __graft_entry__
        __graft_entry__.build()


def _header():
    return open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "hcatgnet_hip.h")).read()


def _query(mode=None, flags=None, groups=None, nodes=184, edges=390, N=None, B=1, perm_count=1, F=25):
    a = _lib.ExplainArgs()
    a.mode = _lib.HCG_EXPLAIN_SHAPLEY if mode is None else mode
    a.flags = _lib.HCG_EXPLAIN_QUERY | (_lib.HCG_EXPLAIN_GROUPED if groups is not None else 0) if flags is None else flags
    a.F, a.D, a.C, a.n_conv, a.R = F, 64, 1, 2, 2
    a.max_nodes, a.max_edges = nodes, edges
    a.N, a.E, a.B = nodes if N is None else N, edges, B
    a.perm_count = perm_count
    if groups is not None:
        a.shap_n_groups = groups
    rc = _lib.load().hcg_explain(ctypes.addressof(a), None)
    return rc, int(a.workspace_bytes_needed), int(a.lds_bytes)


# ------------------------------------------------------------------------------------------------ ABI
def test_struct_size_flag_and_overlay_offsets():
    assert ctypes.sizeof(_lib.ExplainArgs) == 608 == _lib.load().hcg_struct_bytes(_lib.HCG_STRUCT_EXPLAIN_ARGS)
    assert _lib.HCG_EXPLAIN_GROUPED == 8
    assert "#define HCG_EXPLAIN_GROUPED 8" in _header()
    base = _lib.ExplainArgs.fit_edge_logit.offset
    names = ("shap_group_ptr", "shap_member_ptr", "shap_members", "shap_bg_ptr", "shap_bg_members", "shap_n_groups")
    assert [n for n, _ in _lib.SHAPLEY_GROUP_FIELDS] == list(names)
    for k, name in enumerate(names):
        f = getattr(_lib.ExplainArgs, name)
        assert f.offset == base + 8 * k and f.size == 8, name
        assert f.offset + f.size <= 608
        assert name in _header()
    # every earlier field is where it was
    assert _lib.ExplainArgs.perm.offset + 48 == base and _lib.ExplainArgs.path_alpha.offset == base


def test_grouped_query_reports_rows_of_G_and_the_same_lds():
    rc0, ws0, lds0 = _query()
    assert rc0 == 0 and ws0 >= (184 * 25 + 390) * 4
    for G, count in ((3, 1), (3, 6), (184 + 195, 25), (1, 1), (0, 4)):
        rc, ws, lds = _query(groups=G, perm_count=count)
        want = (count * max(G, 1) * 4 + 255) // 256 * 256
        print(f"\n  grouped query G {G} perm_count {count}: rc {rc} workspace {ws} (want {want}) lds {lds} (ungrouped {lds0})")
        assert rc == 0 and ws == want and lds == lds0
    rc, ws, _ = _query(groups=535 * 3, nodes=120, edges=250, N=535 * 120, B=535, perm_count=6)
    assert rc == 0 and ws == (6 * 535 * 3 * 4 + 255) // 256 * 256
    # more groups than features, or a negative count
    assert _query(groups=184 * 25 + 390 + 1)[0] == -1 and _query(groups=-1)[0] == -1
    # the shape limits are the ungrouped mode's
    assert _query(groups=3, nodes=185)[0] == -3 and _query(groups=3, edges=1025)[0] == -3


def test_the_flag_is_refused_in_every_other_mode():
    Q, Gf = _lib.HCG_EXPLAIN_QUERY, _lib.HCG_EXPLAIN_GROUPED
    for mode in (_lib.HCG_EXPLAIN_GRAPHS, _lib.HCG_EXPLAIN_LAYER_EDGE_GRAD, _lib.HCG_EXPLAIN_ENSEMBLE, _lib.HCG_EXPLAIN_FIT,
                 _lib.HCG_EXPLAIN_INTEGRATED, _lib.HCG_EXPLAIN_MOMENTS):
        for flags in (Q | Gf, Gf):
            assert _query(mode=mode, flags=flags)[0] == -1, (mode, flags)
    assert _query(mode=_lib.HCG_EXPLAIN_SHAPLEY, flags=Q | Gf)[0] == 0


def test_default_launch_split_takes_the_grouped_walk_length():
    """The largest G_g bounds a workgroup's evaluations: far more permutations fit one launch than at the per-entry grain
    (535 real-size graphs: one per launch there, tests/test_host_shapley.py)."""
    from hcatgnet_amd.shapley import GROUPED_WORKGROUPS_PER_CU as cap, ShapleySampling
    spl = ShapleySampling.default_samples_per_launch
    assert spl(25, 535, 132341, 374, cap) == 21           # atoms plus bonds: 44 workgroups per CU fit the time
    assert spl(25, 535, 65368, 184, cap) == 25            # atoms
    assert spl(6, 535, 1605, 3, cap) == 6                 # three fragments, all orders
    assert spl(25, 535, 1300000, 184 * 25 + 390) == 1     # the ungrouped default is what it was
    assert spl(25, 1, 1 << 26, 3, cap) == 1               # the workspace cap


def test_exports():
    for name in ("GroupedShapleyResult", "atom_groups", "bond_groups", "draw_group_permutations", "all_group_permutations"):
        assert getattr(H, name) is not None and name in H.__all__


# ------------------------------------------------------------------------------------------------ helpers
def _toy():
    """Two graphs: 3 nodes with edges 0-1, 1-2 interleaved, and 4 nodes with an unpaired edge, a duplicate and a self loop."""
    ei = torch.tensor([[0, 1, 1, 2, 2, 0,   3, 4, 4, 3, 5, 6, 4],
                       [1, 2, 0, 1, 0, 2,   4, 5, 3, 4, 5, 3, 3]])
    bv = torch.tensor([0, 0, 0, 1, 1, 1, 1])
    x = torch.ones(7, 2)
    return H.Batch(x, ei, bv, 2, max_nodes=4, max_edges=7, edges_grouped=True)


def test_atom_groups():
    from hcatgnet_amd.shapley import atom_groups
    b = _toy()
    ag = atom_groups(b)
    assert ag.dtype == torch.int64 and ag.tolist() == [0, 1, 2, 0, 1, 2, 3]


def test_bond_groups_pairs_unpaired_duplicates_and_self_loops():
    from hcatgnet_amd.shapley import bond_groups
    b = _toy()
    # graph 0: (0,1) (1,2) (1,0) (2,1) (2,0) (0,2) -> bonds 01, 12, 01, 12, 02, 02
    # graph 1: (3,4) (4,5) (4,3) (3,4) dup (5,5) loop (6,3) unpaired (4,3) dup
    want = [0, 1, 0, 1, 2, 2,   0, 1, 0, 0, 2, 3, 0]
    got = bond_groups(b)
    assert got.dtype == torch.int64 and got.tolist() == want
    assert bond_groups(b, first=5).tolist() == [w + 5 for w in want]
    first = torch.tensor([3, 4])
    assert bond_groups(b, first=first).tolist() == [w + 3 for w in want[:6]] + [w + 4 for w in want[6:]]
    with pytest.raises(ValueError):
        bond_groups(b, first=torch.tensor([1, 2, 3]))


def test_group_permutations_are_per_segment_and_seed_stable():
    from hcatgnet_amd.shapley import atom_groups, bond_groups, draw_group_permutations
    b = _toy()
    ag = atom_groups(b)
    bg = bond_groups(b, first=torch.tensor([3, 4]))
    gptr = torch.tensor([0, 6, 14])
    p1 = draw_group_permutations(b, ag, bg, 5, torch.Generator().manual_seed(3))
    assert tuple(p1.shape) == (5, 14)
    GR.check_group_permutations(p1, gptr)
    assert torch.equal(p1, draw_group_permutations(b, ag, bg, 5, torch.Generator().manual_seed(3)))
    assert not torch.equal(p1, draw_group_permutations(b, ag, bg, 5, torch.Generator().manual_seed(4)))
    assert not torch.equal(p1[0], p1[1])
    # nodes only: the edges are background
    p2 = draw_group_permutations(b, ag, None, 2, torch.Generator().manual_seed(3))
    GR.check_group_permutations(p2, torch.tensor([0, 3, 7]))


def test_all_group_permutations():
    from hcatgnet_amd.shapley import all_group_permutations
    b = _toy()
    frag = torch.tensor([0, 1, 2, 0, 1, 2, 2])
    rows = all_group_permutations(b, frag, None)
    assert rows.dtype == torch.int32 and tuple(rows.shape) == (6, 6)
    GR.check_group_permutations(rows, torch.tensor([0, 3, 6]))
    assert len({tuple(r) for r in rows[:, :3].tolist()}) == 6 and torch.equal(rows[:, :3], rows[:, 3:])
    # unequal G_g
    with pytest.raises(ValueError):
        all_group_permutations(b, torch.tensor([0, 1, 2, 0, 1, 2, 3]), None)
    # G_g = 7
    x = torch.ones(14, 2)
    ei = torch.zeros(2, 0, dtype=torch.int64)
    b7 = H.Batch(x, ei, torch.tensor([0] * 7 + [1] * 7), 2, max_nodes=7, max_edges=0, edges_grouped=True)
    with pytest.raises(ValueError):
        all_group_permutations(b7, torch.arange(7).repeat(2), None)
    six = all_group_permutations(b7, torch.tensor([0, 1, 2, 3, 4, 5, 5] * 2), None)
    assert tuple(six.shape) == (math.factorial(6), 12) and len({tuple(r) for r in six[:, :6].tolist()}) == 720


def test_group_ids_are_validated_on_the_host():
    from hcatgnet_amd.shapley import ShapleySampling, atom_groups
    b = _toy()
    sv = ShapleySampling(H.make_network("GCN", H.default_options(), 2))
    ok = atom_groups(b)
    gap = ok.clone(); gap[ok == 1] = 5                       # ids 0, 2, (3,) 5: a gap, and an id >= the number of distinct ids
    low = ok.clone(); low[0] = -2
    bad = [gap, low, ok.float(), ok[:-1], ok.unsqueeze(1).expand(7, 3), ok.bool()]
    for t in bad:
        with pytest.raises(ValueError):
            sv(b, n_samples=1, node_group=t)
        with pytest.raises(ValueError):
            sv.loop(b, n_samples=1, node_group=t)
    egap = torch.zeros(13, dtype=torch.int64); egap[0] = 2    # edges alone: ids 0 and 2
    for kw in (dict(edge_group=egap), dict(edge_group=torch.zeros(12, dtype=torch.int64)),
               dict(node_group=ok, edge_group=torch.full((13,), 9, dtype=torch.int64)),       # a gap over both arrays
               dict(node_group=ok, group_permutations=torch.zeros(1, 7, dtype=torch.int64)),
               dict(node_group=ok, group_permutations=torch.zeros(1, 8, dtype=torch.int32)),
               dict(node_group=ok, permutations=torch.zeros(1, 27, dtype=torch.int32)),
               dict(group_permutations=torch.zeros(1, 7, dtype=torch.int32))):
        with pytest.raises(ValueError):
            sv(b, n_samples=1, **kw)
    # ids spread over both arrays are fine: atoms 0 .. n - 1, every edge of a graph in group n
    r = sv(b, n_samples=1, node_group=ok, edge_group=torch.tensor([3] * 6 + [4] * 7), generator=torch.Generator().manual_seed(0))
    assert r.group_ptr.tolist() == [0, 4, 9] and tuple(r.group_attr.shape) == (9,)


# ------------------------------------------------------------------------------------------------ the loop on CPU tensors
def _small_case(num_graphs=4, seed=5):
    """Graphs of 8-14 nodes, F = 6 with about half the entries exactly 0, one explicit self-loop edge, 2 classes; node 1 of
    graph 0 has an all-zero row (a dead atom)."""
    sb = synth.make_batch(num_graphs=num_graphs, nodes=11, extra_bonds=2, max_degree=4, feat=6, nodes_jitter=3)
    gen = torch.Generator().manual_seed(seed)
    x = sb.x * (torch.rand(sb.x.shape, generator=gen) < 0.5)
    x[1] = 0
    eg = sb.batch[sb.edge_index[1]]
    pos = int((eg <= 2).sum()) - 2                              # inside graph 2's edge block
    node = int(sb.edge_index[0, pos])
    ei = torch.cat([sb.edge_index[:, :pos], torch.tensor([[node], [node]]), sb.edge_index[:, pos:]], 1).contiguous()
    params = SR.rand_params(6, 64, n_conv=2, n_read=2, n_classes=2, seed=23)
    b = H.Batch(x.contiguous(), ei, sb.batch, sb.num_graphs, max_nodes=sb.max_nodes, max_edges=sb.max_edges + 1, edges_grouped=True)
    return b, params


def _fragments(b, k=3):
    """`k` contiguous node ranges per graph"""
    from hcatgnet_amd.shapley import atom_groups
    n = torch.bincount(b.batch, minlength=b.num_graphs)
    return atom_groups(b) * k // n[b.batch]


def _loop_case(tag, b, params, node_group, edge_group, perm, exact=False):
    from hcatgnet_amd.shapley import ShapleySampling
    model = SR.model_from_params(H, params)
    sv = ShapleySampling(model)
    assert "CPU" in sv.reason(b)
    r = sv(b, group_permutations=perm, class_index=1, node_group=node_group, edge_group=edge_group)
    assert sv.last_path == "loop" and isinstance(r, H.GroupedShapleyResult)
    refs, gptr, ng, eg = GR.reference_batch(params, b.x, b.edge_index, b.batch, b.num_graphs, node_group, edge_group, perm, 1, exact=exact)
    print(f"\n  {tag}: B {b.num_graphs} N {b.x.shape[0]} E {b.edge_index.shape[1]} G {int(gptr[-1])} P {perm.shape[0]} "
          f"dead groups {sum(int((~q['live']).sum()) for q in refs)}")
    GR.check_against_reference(r, refs, gptr, ng, eg, 1, tag, b.batch, b.batch[b.edge_index[1]])
    assert tuple(r.out_full.shape) == (b.num_graphs, 2) and tuple(r.out_base.shape) == (b.num_graphs, 2)
    for q in model.parameters():
        assert q.grad is None
    return r, refs, gptr


def test_loop_atoms_with_edges_as_background():
    from hcatgnet_amd.shapley import atom_groups, draw_group_permutations
    b, params = _small_case()
    ag = atom_groups(b)
    perm = draw_group_permutations(b, ag, None, 2, torch.Generator().manual_seed(11))
    r, refs, gptr = _loop_case("atoms, edges in the background", b, params, ag, None, perm)
    assert float(r.group_attr[1]) == 0.0 and not bool(refs[0]["live"][1])      # the atom whose row of x is zero
    assert float(r.edge_attr.abs().max()) == 0.0                                # the background carries 0
    # the base has the edges on: it differs from the ungrouped base (everything off) unless the graph has no live entry
    assert torch.equal(r.node_attr[:, 0], r.node_attr[:, 5])


def test_loop_atoms_plus_bonds():
    from hcatgnet_amd.shapley import atom_groups, bond_groups, draw_group_permutations
    b, params = _small_case()
    n = torch.bincount(b.batch, minlength=b.num_graphs)
    ag, bg = atom_groups(b), bond_groups(b, first=n)
    perm = draw_group_permutations(b, ag, bg, 2, torch.Generator().manual_seed(12))
    r, refs, gptr = _loop_case("atoms plus bonds", b, params, ag, bg, perm)
    loop = int((b.edge_index[0] == b.edge_index[1]).nonzero()[0])
    assert float(r.edge_attr[loop]) == 0.0                                      # the self loop's bond group is dead
    assert sum(int((~q["live"]).sum()) for q in refs) >= 2


def test_loop_entry_grouping_with_a_partial_background():
    from hcatgnet_amd.shapley import draw_group_permutations
    b, params = _small_case(num_graphs=3)
    N, F = b.x.shape
    # features 0-1 of every node are one group per node pair, features 2-3 one group per graph, features 4-5 background
    from hcatgnet_amd.shapley import atom_groups
    ag = atom_groups(b)
    ng = torch.full((N, F), -1, dtype=torch.int64)
    ng[:, 0:2] = (ag // 2 + 1).unsqueeze(1)
    ng[:, 2:4] = 0
    perm = draw_group_permutations(b, ng, None, 2, torch.Generator().manual_seed(13))
    r, refs, gptr = _loop_case("[N, F] groups, some entries in the background", b, params, ng, None, perm)
    assert float(r.node_attr[:, 4:].abs().max()) == 0.0


def test_loop_three_fragments_walked_exactly():
    from hcatgnet_amd.shapley import all_group_permutations
    b, params = _small_case(num_graphs=5)
    frag = _fragments(b)
    perm = all_group_permutations(b, frag, None)
    assert tuple(perm.shape) == (6, 3 * b.num_graphs)
    _loop_case("three fragments, all 3! orders, against the subset formula", b, params, frag, None, perm, exact=True)
