"""GPU tests of grouped Shapley value sampling (`ShapleySampling(..., node_group=, edge_group=, group_permutations=)`): atoms,
bonds and fragments as the players of the on-chip permutation walk (csrc/shapley.hip, HCG_EXPLAIN_GROUPED).
tests/shapley_groups_ref.py states the reference (the fp64 oracle walked group by group on the CPU, the subset formula for
the exact case) and the bounds; the case shapes are those of tests/test_gpu_shapley.py.  Every figure is printed before it is
asserted (`pytest -s`)."""
import functools

import pytest
import torch

from tests import shapley_groups_ref as GR
from tests import shapley_ref as SR
from tests.helpers import golden_files, load_golden

pytestmark = pytest.mark.gpu
PARAM_SEED, X_SEED, PERM_SEED = 23, 5, 11
SHAPE_LIMIT = 16
NODE_LIMIT = 184            # this mode's documented node limit

# name -> (synth.make_batch arguments, non-zero share of x, model depths, class_index, permutations, players)
CASES = {
    "ragged-onehot25": (dict(num_graphs=6, nodes=30, extra_bonds=3, max_degree=4, feat=25, nodes_jitter=10), 0.12, dict(n_conv=2, n_read=2, n_classes=1), 0, 3, "atoms+bonds"),
    "four-convs": (dict(num_graphs=4, nodes=16, extra_bonds=2, max_degree=4, feat=25, nodes_jitter=3), 0.3, dict(n_conv=4, n_read=4, n_classes=8), 5, 2, "atoms"),
    "one-conv": (dict(num_graphs=5, nodes=20, extra_bonds=3, max_degree=4, feat=32, nodes_jitter=4), 0.5, dict(n_conv=1, n_read=1, n_classes=1), 0, 2, "atoms+bonds"),
    "node-limit": (dict(num_graphs=1, nodes=NODE_LIMIT, extra_bonds=12, max_degree=6, feat=25), 0.12, dict(n_conv=2, n_read=2, n_classes=1), 0, 1, "atoms+bonds"),
}


@pytest.fixture(scope="module")
def H():
    import hcatgnet_amd
    import __graft_entry__
    import os
    from hcatgnet_amd import _lib
    if not os.path.isfile(_lib.LIB_PATH):
        __graft_entry__.build()
    return hcatgnet_amd


class _Case:
    pass


@functools.lru_cache(maxsize=None)
def _case(name):
    from hcatgnet_amd import synth
    c = _Case()
    if name == "golden":
        # one real graph (57-117 atoms, F = 25) with its trained weights
        g = load_golden(golden_files()[0])
        a, b = int(g["node_ptr"][0]), int(g["node_ptr"][1])
        ea, eb = int(g["edge_ptr"][0]), int(g["edge_ptr"][1])
        assert 57 <= b - a <= 117 and g["x"].shape[1] == 25
        c.params = g["params"]
        c.x, c.ei, c.batch, c.B = g["x"][a:b].contiguous(), (g["edge_index"][:, ea:eb] - a).contiguous(), torch.zeros(b - a, dtype=torch.long), 1
        c.max_nodes, c.max_edges = b - a, eb - ea
        c.cls, c.P, c.players = 0, 2, "atoms+bonds"
    else:
        bk, share, mk, c.cls, c.P, c.players = CASES[name]
        sb = synth.make_batch(**bk)
        c.params = SR.rand_params(bk["feat"], 64, seed=PARAM_SEED, **mk)
        x = sb.x * (torch.rand(sb.x.shape, generator=torch.Generator().manual_seed(X_SEED)) < share)
        c.x, c.ei, c.batch, c.B = x.contiguous(), sb.edge_index, sb.batch, sb.num_graphs
        c.max_nodes, c.max_edges = sb.max_nodes, sb.max_edges
    c.F = c.x.shape[1]
    print(f"\n  case {name}: B {c.B} N {c.x.shape[0]} E {c.ei.shape[1]} max {c.max_nodes} / {c.max_edges}  "
          f"non-zero x {int((c.x != 0).sum())} of {c.x.numel()}  P {c.P}  players {c.players}")
    return c


def _gpu_batch(H, c):
    return H.Batch(c.x.cuda(), c.ei.cuda(), c.batch.cuda(), c.B, max_nodes=c.max_nodes, max_edges=c.max_edges,
                   edges_grouped=True)


def _players(gb, players):
    """-> (node_group, edge_group) on the batch's device"""
    from hcatgnet_amd.shapley import atom_groups, bond_groups
    ag = atom_groups(gb)
    if players == "atoms":
        return ag, None
    return ag, bond_groups(gb, first=torch.bincount(gb.batch, minlength=gb.num_graphs))


def _cpu(t):
    return None if t is None else t.cpu()


def _perm(gb, ng, eg, P, seed=PERM_SEED):
    from hcatgnet_amd.shapley import draw_group_permutations
    return draw_group_permutations(gb, ng, eg, P, torch.Generator().manual_seed(seed))


def _clone(r):
    return [t.clone() for t in r]


def _check(r, c, ng, eg, perm, tag, exact=False, graphs=None):
    refs, gptr, ngc, egc = GR.reference_batch(c.params, c.x, c.ei, c.batch, c.B, _cpu(ng), _cpu(eg), perm, c.cls, graphs=graphs, exact=exact)
    if perm is not None and not exact:
        GR.check_group_permutations(perm, gptr)
    GR.check_against_reference(r, refs, gptr, ngc, egc, c.cls, tag, c.batch, c.batch[c.ei[1]])
    return refs, gptr


# ------------------------------------------------------------------------------------------------ 1. parity
@pytest.mark.parametrize("name", ["golden"] + list(CASES))
def test_parity_with_the_fp64_group_walk(H, name):
    from hcatgnet_amd.shapley import ShapleySampling
    c = _case(name)
    if name == "node-limit":
        assert c.max_nodes == NODE_LIMIT
    sv = ShapleySampling(SR.model_from_params(H, c.params).cuda())
    gb = _gpu_batch(H, c)
    assert sv.reason(gb) is None
    ng, eg = _players(gb, c.players)
    perm = _perm(gb, ng, eg, c.P)
    r = sv(gb, group_permutations=perm, class_index=c.cls, node_group=ng, edge_group=eg)
    assert sv.last_path == "fused" and isinstance(r, H.GroupedShapleyResult)
    torch.cuda.synchronize()
    assert int(gb._hcg_plan.status[0].item()) == 0
    _check(r, c, ng, eg, perm, f"{name} ({c.players})")
    if eg is None:
        assert float(r.edge_attr.abs().max()) == 0.0


# ------------------------------------------------------------------------------------------------ 2. exact Shapley values
def test_three_fragments_walked_exactly_match_the_subset_formula(H):
    from hcatgnet_amd import synth
    from hcatgnet_amd.shapley import ShapleySampling, all_group_permutations, atom_groups
    sb = synth.make_batch(num_graphs=4, nodes=20, extra_bonds=3, max_degree=4, feat=25, nodes_jitter=3)
    c = _Case()
    c.x = (sb.x * (torch.rand(sb.x.shape, generator=torch.Generator().manual_seed(X_SEED)) < 0.3)).contiguous()
    c.ei, c.batch, c.B, c.F, c.cls = sb.edge_index, sb.batch, sb.num_graphs, 25, 0
    c.max_nodes, c.max_edges = sb.max_nodes, sb.max_edges
    c.params = SR.rand_params(25, 64, seed=PARAM_SEED)
    gb = _gpu_batch(H, c)
    frag = atom_groups(gb) * 3 // torch.bincount(gb.batch, minlength=c.B)[gb.batch]
    perm = all_group_permutations(gb, frag, None)
    assert tuple(perm.shape) == (6, 3 * c.B)
    sv = ShapleySampling(SR.model_from_params(H, c.params).cuda())
    r = sv(gb, group_permutations=perm, node_group=frag)
    assert sv.last_path == "fused"
    print(f"\n  fragments: B {c.B} N {c.x.shape[0]} E {c.ei.shape[1]}, 3 groups per graph, all 6 orders")
    _check(r, c, frag, None, None, "three fragments, exact", exact=True)


# ------------------------------------------------------------------------------------------------ 3. singleton groups
def test_singleton_groups_are_bitwise_the_ungrouped_call(H):
    from hcatgnet_amd.shapley import ShapleySampling, draw_permutations
    c = _case("ragged-onehot25")
    gb = _gpu_batch(H, c)
    model = SR.model_from_params(H, c.params).cuda()
    perm = draw_permutations(gb, c.F, 3, torch.Generator().manual_seed(PERM_SEED))
    want = _clone(ShapleySampling(model)(gb, permutations=perm))
    nptr, eptr = SR.pointers(c.batch, c.ei, c.B)
    n = nptr[1:] - nptr[:-1]
    local_node = torch.arange(c.x.shape[0]) - nptr[c.batch]
    ng = local_node.unsqueeze(1) * c.F + torch.arange(c.F).unsqueeze(0)                       # [N, F]: the entry's local index
    egraph = c.batch[c.ei[1]]
    eg = n[egraph] * c.F + torch.arange(c.ei.shape[1]) - eptr[egraph]                          # edges numbered after the entries
    sv = ShapleySampling(model)
    r = sv(gb, group_permutations=perm, node_group=ng.cuda(), edge_group=eg.cuda())
    assert sv.last_path == "fused"
    assert torch.equal(r.node_attr, want[0]) and torch.equal(r.edge_attr, want[1])
    assert torch.equal(r.out_full, want[2]) and torch.equal(r.out_base, want[3])
    for g in range(c.B):
        a, b, ea, eb = int(nptr[g]), int(nptr[g + 1]), int(eptr[g]), int(eptr[g + 1])
        s = a * c.F + ea
        assert int(r.group_ptr[g]) == s
        assert torch.equal(r.group_attr[s:s + (b - a) * c.F + eb - ea], torch.cat([want[0][a:b].reshape(-1), want[1][ea:eb]])), g


# ------------------------------------------------------------------------------------------------ 4. one group
def test_one_group_of_everything_gets_full_minus_base_bitwise(H):
    from hcatgnet_amd.shapley import ShapleySampling
    c = _case("ragged-onehot25")
    gb = _gpu_batch(H, c)
    sv = ShapleySampling(SR.model_from_params(H, c.params).cuda())
    ng = torch.zeros(c.x.shape[0], dtype=torch.int64).cuda()
    eg = torch.zeros(c.ei.shape[1], dtype=torch.int32).cuda()                                # (any integer dtype)
    perm = torch.zeros(1, c.B, dtype=torch.int32).cuda()
    r = sv(gb, group_permutations=perm, node_group=ng, edge_group=eg)
    assert sv.last_path == "fused" and r.group_ptr.tolist() == list(range(c.B + 1))
    print(f"\n  one group: group_attr {r.group_attr.tolist()}")
    assert torch.equal(r.group_attr, r.out_full[:, 0] - r.out_base[:, 0])
    # nothing is on at the base: it is the ungrouped call's base, and everything on is the plain forward
    plain = _clone(ShapleySampling(sv.model)(gb, n_samples=1, generator=torch.Generator().manual_seed(0)))
    assert torch.equal(r.out_base, plain[3]) and float((r.out_full - plain[2]).abs().max()) <= SR.TOL * max(1.0, float(plain[2].abs().max()))


# ------------------------------------------------------------------------------------------------ 5. dead groups
def test_groups_without_a_live_member_get_exactly_zero(H):
    from hcatgnet_amd.shapley import ShapleySampling
    c0 = _case("ragged-onehot25")
    c = _Case()
    c.__dict__.update(c0.__dict__)
    c.x = c0.x.clone()
    dead_atom = int((c0.batch == 1).nonzero()[2])                  # an atom of graph 1: its row of x becomes zero
    c.x[dead_atom] = 0
    eg_ = c0.batch[c0.ei[1]]
    pos = int((eg_ <= 1).sum()) - 3                                # an explicit self loop inside graph 1's edge block
    node = int(c0.ei[0, pos])
    c.ei = torch.cat([c0.ei[:, :pos], torch.tensor([[node], [node]]), c0.ei[:, pos:]], 1).contiguous()
    c.max_edges = c0.max_edges + 1
    gb = _gpu_batch(H, c)
    sv = ShapleySampling(SR.model_from_params(H, c.params).cuda())
    nptr, _ = SR.pointers(c.batch, c.ei, c.B)
    # atoms, edges in the background
    ng, eg = _players(gb, "atoms")
    perm = _perm(gb, ng, eg, 2)
    r = sv(gb, group_permutations=perm, node_group=ng)
    assert sv.last_path == "fused"
    refs, gptr = _check(r, c, ng, None, perm, "dead atom, edges in the background")
    zero_rows = (c.x == 0).all(1)
    live = torch.cat([q["live"] for q in refs])
    assert torch.equal(live, ~zero_rows) and not bool(live[dead_atom])
    ref_phi = torch.cat([q["phi"] for q in refs])
    print(f"\n  atoms: {int(live.sum())} live groups of {live.numel()}; smallest live |phi_ref| {float(ref_phi[live].abs().min()):.3e}")
    assert bool((ref_phi[live] != 0).all())                        # (X_SEED: no live group's reference value is 0)
    assert float(r.group_attr[dead_atom]) == 0.0 and float(r.node_attr[dead_atom].abs().max()) == 0.0
    assert int((r.group_attr != 0).sum()) == int(live.sum())
    # atoms plus bonds: the self loop's bond group
    ng, eg = _players(gb, "atoms+bonds")
    perm = _perm(gb, ng, eg, 2)
    r = sv(gb, group_permutations=perm, node_group=ng, edge_group=eg)
    refs, gptr = _check(r, c, ng, eg, perm, "dead atom and self-loop bond")
    live = torch.cat([q["live"] for q in refs])
    ref_phi = torch.cat([q["phi"] for q in refs])
    loop_group = int(gptr[1]) + int(eg[pos])
    print(f"  atoms + bonds: {int(live.sum())} live groups of {live.numel()}; smallest live |phi_ref| {float(ref_phi[live].abs().min()):.3e}")
    egc = eg.cpu()
    assert int((c.ei[0] == c.ei[1]).sum()) == 1 and int((egc[c.batch[c.ei[1]] == 1] == egc[pos]).sum()) == 1     # a group of its own
    assert not bool(live[loop_group]) and float(r.group_attr[loop_group]) == 0.0 and float(r.edge_attr[pos]) == 0.0
    assert bool((ref_phi[live] != 0).all())
    assert int((~live).sum()) == int(zero_rows.sum()) + 1
    assert int((r.group_attr != 0).sum()) == int(live.sum())


# ------------------------------------------------------------------------------------------------ 6. bitwise
def test_bitwise_run_split_batch_and_instance(H):
    """No float atomics, fixed orders: a result depends on nothing but the graph, the model, the groups and the permutations."""
    from hcatgnet_amd.shapley import ShapleySampling
    c = _case("ragged-onehot25")
    model = SR.model_from_params(H, c.params).cuda()
    sv = ShapleySampling(model)
    gb = _gpu_batch(H, c)
    ng, eg = _players(gb, "atoms+bonds")
    P = 5
    perm = _perm(gb, ng, eg, P)
    kw = dict(node_group=ng, edge_group=eg)
    full = _clone(sv(gb, group_permutations=perm, **kw))
    assert sv.last_path == "fused"
    again = _clone(sv(gb, group_permutations=perm, **kw))
    for a, b in zip(full, again):
        assert torch.equal(a, b)
    for spl in (1, 2, P):
        got = _clone(sv(gb, group_permutations=perm, samples_per_launch=spl, **kw))
        for a, b in zip(full, got):
            assert torch.equal(a, b), spl
    # a used instance (its accumulator and workspace hold a larger run) against a fresh one
    want = _clone(ShapleySampling(model)(gb, group_permutations=perm[:3].contiguous(), **kw))
    assert not torch.equal(want[0], full[0])
    got = _clone(sv(gb, group_permutations=perm[:3].contiguous(), **kw))
    for a, b in zip(want, got):
        assert torch.equal(a, b)
    # the rest of the batch
    nptr, eptr = SR.pointers(c.batch, c.ei, c.B)
    gptr = full[1].cpu()
    single = ShapleySampling(model)
    for g in range(c.B):
        a, b, ea, eb = int(nptr[g]), int(nptr[g + 1]), int(eptr[g]), int(eptr[g + 1])
        ga, gq = int(gptr[g]), int(gptr[g + 1])
        one = H.Batch(c.x[a:b].cuda(), (c.ei[:, ea:eb] - a).contiguous().cuda(), torch.zeros(b - a, dtype=torch.long).cuda(), 1,
                      max_nodes=b - a, max_edges=eb - ea, edges_grouped=True)
        r = single(one, group_permutations=perm[:, ga:gq].contiguous(), node_group=ng[a:b], edge_group=eg[ea:eb])
        assert single.last_path == "fused"
        assert torch.equal(r.group_attr, full[0][ga:gq]), g
        assert torch.equal(r.node_attr, full[2][a:b]) and torch.equal(r.edge_attr, full[3][ea:eb]), g
        assert torch.equal(r.out_full, full[4][g:g + 1]) and torch.equal(r.out_base, full[5][g:g + 1]), g


# ------------------------------------------------------------------------------------------------ 7. refusal
def test_a_graph_over_max_nodes_is_refused_and_the_others_keep_their_values(H):
    from hcatgnet_amd.shapley import ShapleySampling
    c0 = _case("ragged-onehot25")
    sizes = torch.bincount(c0.batch, minlength=c0.B)
    big = sizes == sizes.max()
    assert 0 < int(big.sum()) < c0.B
    sv = ShapleySampling(SR.model_from_params(H, c0.params).cuda())
    gb = _gpu_batch(H, c0)
    ng, eg = _players(gb, "atoms+bonds")
    perm = _perm(gb, ng, eg, 3)
    honest = _clone(sv(gb, group_permutations=perm, node_group=ng, edge_group=eg))
    c = _Case()
    c.__dict__.update(c0.__dict__)
    c.max_nodes = int(sizes.max()) - 1
    gb = _gpu_batch(H, c)
    r = sv(gb, group_permutations=perm, node_group=ng, edge_group=eg, samples_per_launch=2)
    assert sv.last_path == "fused"
    torch.cuda.synchronize()
    status = gb._hcg_plan.status
    word = int(status[0].item())
    status.zero_()                                                    # (shared per device: leave it clean for the next test)
    assert word & SHAPE_LIMIT
    gptr = r.group_ptr.cpu()
    group_big = big.repeat_interleave(gptr[1:] - gptr[:-1]).cuda()
    assert torch.equal(r.group_attr[~group_big], honest[0][~group_big])
    assert float(r.group_attr[group_big].abs().max()) == 0.0
    node_big = big[c.batch].cuda()
    assert torch.equal(r.node_attr[~node_big], honest[2][~node_big]) and float(r.node_attr[node_big].abs().max()) == 0.0
    assert torch.equal(r.out_full[~big.cuda()], honest[4][~big.cuda()]) and torch.equal(r.out_base[~big.cuda()], honest[5][~big.cuda()])
    assert float(r.out_full[big.cuda()].abs().max()) == 0.0 and float(r.out_base[big.cuda()].abs().max()) == 0.0


# ------------------------------------------------------------------------------------------------ 8. fallback
def test_a_model_outside_the_limits_takes_the_loop_with_the_same_bounds(H):
    """D = 128: the batch-synchronous loop on `ExplainStep`'s any-shape path."""
    from hcatgnet_amd import synth
    from hcatgnet_amd.shapley import ShapleySampling
    from hcatgnet_amd.gcn import GCNConv
    bk = dict(num_graphs=3, nodes=8, extra_bonds=2, max_degree=4, feat=6, nodes_jitter=2)
    sb = synth.make_batch(**bk)
    c = _Case()
    c.x = (sb.x * (torch.rand(sb.x.shape, generator=torch.Generator().manual_seed(X_SEED)) < 0.5)).contiguous()
    c.ei, c.batch, c.B, c.F, c.cls = sb.edge_index, sb.batch, sb.num_graphs, 6, 1
    c.max_nodes, c.max_edges = sb.max_nodes, sb.max_edges
    c.params = SR.rand_params(6, 128, seed=PARAM_SEED, n_classes=2)
    model = SR.model_from_params(H, c.params).cuda()
    before = [q.detach().clone() for q in model.parameters()]
    sv = ShapleySampling(model)
    gb = _gpu_batch(H, c)
    assert "shape" in sv.reason(gb)
    ng, eg = _players(gb, "atoms+bonds")
    perm = _perm(gb, ng, eg, 1)
    print(f"\n  fallback D = 128: N {c.x.shape[0]} E {c.ei.shape[1]} G {perm.shape[1]}")
    r = sv(gb, group_permutations=perm, class_index=1, node_group=ng, edge_group=eg)
    assert sv.last_path == "loop"
    _check(r, c, ng, eg, perm, "D = 128 (loop)")
    for q, b in zip(model.parameters(), before):
        assert torch.equal(q.detach(), b) and q.grad is None
    for mod in model.modules():
        if isinstance(mod, GCNConv):
            assert mod.explain is False and mod._edge_mask is None
