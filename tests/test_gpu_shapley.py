"""GPU tests of `hcatgnet_amd.shapley.ShapleySampling`: the permutation walk of a batch of graphs on chip
(csrc/shapley.hip).  tests/shapley_ref.py states the reference (the fp64 oracle walked step by step on the CPU) and the
bounds; the cases are sized so that walk stays at seconds.  Every figure is printed before it is asserted (`pytest -s`)."""
import functools

import pytest
import torch

from tests import shapley_ref as SR
from tests.helpers import golden_files, load_golden

pytestmark = pytest.mark.gpu
PARAM_SEED, X_SEED, PERM_SEED = 23, 5, 11
SHAPE_LIMIT = 16
NODE_LIMIT = 184            # this mode's documented node limit

# name -> (synth.make_batch arguments, non-zero share of x (1.0 = dense), model depths, class_index, permutations)
CASES = {
    "small-dense64": (dict(num_graphs=8, nodes=12, extra_bonds=2, max_degree=4, feat=64), 1.0, dict(n_conv=2, n_read=2, n_classes=1), 0, 2),
    "ragged-onehot25": (dict(num_graphs=6, nodes=30, extra_bonds=3, max_degree=4, feat=25, nodes_jitter=10), 0.12, dict(n_conv=2, n_read=2, n_classes=1), 0, 3),
    "deep": (dict(num_graphs=5, nodes=20, extra_bonds=3, max_degree=4, feat=32, nodes_jitter=4), 0.5, dict(n_conv=3, n_read=3, n_classes=2), 1, 2),
    "one-conv": (dict(num_graphs=5, nodes=20, extra_bonds=3, max_degree=4, feat=32, nodes_jitter=4), 0.5, dict(n_conv=1, n_read=1, n_classes=1), 0, 2),
    "four-convs": (dict(num_graphs=4, nodes=16, extra_bonds=2, max_degree=4, feat=25, nodes_jitter=3), 0.3, dict(n_conv=4, n_read=4, n_classes=8), 5, 2),
    "node-limit": (dict(num_graphs=1, nodes=NODE_LIMIT, extra_bonds=12, max_degree=6, feat=25), 0.12, dict(n_conv=2, n_read=2, n_classes=1), 0, 1),
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
        c.cls, c.P = 0, 2
    else:
        bk, share, mk, c.cls, c.P = CASES[name]
        sb = synth.make_batch(**bk)
        c.params = SR.rand_params(bk["feat"], 64, seed=PARAM_SEED, **mk)
        x = sb.x
        if share < 1.0:
            x = x * (torch.rand(x.shape, generator=torch.Generator().manual_seed(X_SEED)) < share)
        c.x, c.ei, c.batch, c.B = x.contiguous(), sb.edge_index, sb.batch, sb.num_graphs
        c.max_nodes, c.max_edges = sb.max_nodes, sb.max_edges
    c.F = c.x.shape[1]
    print(f"\n  case {name}: B {c.B} N {c.x.shape[0]} E {c.ei.shape[1]} max {c.max_nodes} / {c.max_edges}  "
          f"non-zero x {int((c.x != 0).sum())} of {c.x.numel()}  P {c.P}")
    return c


def _gpu_batch(H, c):
    return H.Batch(c.x.cuda(), c.ei.cuda(), c.batch.cuda(), c.B, max_nodes=c.max_nodes, max_edges=c.max_edges,
                   edges_grouped=True)


def _perm(H, c, gb, P=None, seed=PERM_SEED):
    from hcatgnet_amd.shapley import draw_permutations
    perm = draw_permutations(gb, c.F, P or c.P, torch.Generator().manual_seed(seed))
    nptr, eptr = SR.pointers(c.batch, c.ei, c.B)
    SR.check_permutations(perm, nptr, eptr, c.F)
    return perm


def _clone(r):
    return [t.clone() for t in r]


# ------------------------------------------------------------------------------------------------ 1. parity
@pytest.mark.parametrize("name", ["golden"] + list(CASES))
def test_parity_with_the_fp64_oracle_walk(H, name):
    from hcatgnet_amd.shapley import ShapleySampling
    c = _case(name)
    if name == "node-limit":
        assert c.max_nodes == NODE_LIMIT
    sv = ShapleySampling(SR.model_from_params(H, c.params).cuda())
    gb = _gpu_batch(H, c)
    assert sv.reason(gb) is None
    perm = _perm(H, c, gb)
    r = sv(gb, permutations=perm, class_index=c.cls)
    assert sv.last_path == "fused"
    torch.cuda.synchronize()
    assert int(gb._hcg_plan.status[0].item()) == 0
    assert tuple(r.node_attr.shape) == tuple(c.x.shape) and tuple(r.edge_attr.shape) == (c.ei.shape[1],)
    refs = SR.reference_batch(c.params, c.x, c.ei, c.batch, c.B, perm, c.cls)
    SR.check_against_reference(r, refs, c.x, c.ei, c.batch, c.B, c.cls, name)
    SR.check_exact_zeros(r, c.x, c.ei)


# ------------------------------------------------------------------------------------------------ 2. explicit self loop
def test_explicit_self_loop_edge_gets_exactly_zero(H):
    from hcatgnet_amd.shapley import ShapleySampling
    c0 = _case("ragged-onehot25")
    eg = c0.batch[c0.ei[1]]
    pos = int((eg <= 1).sum()) - 3                              # inside graph 1's edge block
    node = int(c0.ei[0, pos])
    c = _Case()
    c.__dict__.update(c0.__dict__)
    c.ei = torch.cat([c0.ei[:, :pos], torch.tensor([[node], [node]]), c0.ei[:, pos:]], 1).contiguous()
    c.max_edges = c0.max_edges + 1
    sv = ShapleySampling(SR.model_from_params(H, c.params).cuda())
    gb = _gpu_batch(H, c)
    perm = _perm(H, c, gb)
    r = sv(gb, permutations=perm, class_index=0)
    assert sv.last_path == "fused"
    refs = SR.reference_batch(c.params, c.x, c.ei, c.batch, c.B, perm, 0)
    SR.check_against_reference(r, refs, c.x, c.ei, c.batch, c.B, 0, "self loop")
    nz, nl = SR.check_exact_zeros(r, c.x, c.ei)
    assert nl == 1 and float(r.edge_attr[pos]) == 0.0
    assert int((r.edge_attr != 0).sum()) == c.ei.shape[1] - 1


# ------------------------------------------------------------------------------------------------ 3. bitwise
def test_bitwise_run_batch_split_and_prefix(H):
    """No float atomics, fixed orders: a result depends on nothing but the graph, the model and the permutations."""
    from hcatgnet_amd.shapley import ShapleySampling
    c = _case("ragged-onehot25")
    model = SR.model_from_params(H, c.params).cuda()
    sv = ShapleySampling(model)
    gb = _gpu_batch(H, c)
    P = 5
    perm = _perm(H, c, gb, P=P)
    full = _clone(sv(gb, permutations=perm))
    assert sv.last_path == "fused"
    again = _clone(sv(gb, permutations=perm))
    for a, b in zip(full, again):
        assert torch.equal(a, b)
    # the split into launches
    for spl in (1, 2, P):
        got = _clone(sv(gb, permutations=perm, samples_per_launch=spl))
        for a, b in zip(full, got):
            assert torch.equal(a, b), spl
    # the first P' rows of a larger tensor: an instance that has just run the larger tensor (its accumulator and workspace
    # hold that run) against a fresh instance that only ever saw the P' rows
    for Pp in (1, 3):
        want = _clone(ShapleySampling(model)(gb, permutations=perm[:Pp].contiguous()))
        big = torch.cat([perm[:Pp], _perm(H, c, gb, P=2, seed=99)]).contiguous()
        used = ShapleySampling(model)
        assert not torch.equal(_clone(used(gb, permutations=big))[0], want[0])
        got = _clone(used(gb, permutations=big[:Pp]))
        for a, b in zip(want, got):
            assert torch.equal(a, b), Pp
    # the rest of the batch
    nptr, eptr = SR.pointers(c.batch, c.ei, c.B)
    single = ShapleySampling(model)
    for g in range(c.B):
        a, b, ea, eb = int(nptr[g]), int(nptr[g + 1]), int(eptr[g]), int(eptr[g + 1])
        s, K = a * c.F + ea, (b - a) * c.F + (eb - ea)
        one = H.Batch(c.x[a:b].cuda(), (c.ei[:, ea:eb] - a).contiguous().cuda(), torch.zeros(b - a, dtype=torch.long).cuda(), 1,
                      max_nodes=b - a, max_edges=eb - ea, edges_grouped=True)
        r = single(one, permutations=perm[:, s:s + K].contiguous())
        assert single.last_path == "fused"
        assert torch.equal(r.node_attr, full[0][a:b]) and torch.equal(r.edge_attr, full[1][ea:eb]), g
        assert torch.equal(r.out_full, full[2][g:g + 1]) and torch.equal(r.out_base, full[3][g:g + 1]), g


# ------------------------------------------------------------------------------------------------ 4. drawn inside the call
def test_n_samples_and_generator_draw_the_permutations(H):
    from hcatgnet_amd.shapley import ShapleySampling
    c = _case("deep")
    sv = ShapleySampling(SR.model_from_params(H, c.params).cuda())
    gb = _gpu_batch(H, c)
    a = _clone(sv(gb, n_samples=3, generator=torch.Generator().manual_seed(7), class_index=1))
    b = _clone(sv(gb, n_samples=3, generator=torch.Generator().manual_seed(7), class_index=1))
    want = _clone(sv(gb, permutations=_perm(H, c, gb, P=3, seed=7), class_index=1))
    for x, y, z in zip(a, b, want):
        assert torch.equal(x, y) and torch.equal(x, z)
    with pytest.raises(ValueError):
        sv(gb, class_index=2)


# ------------------------------------------------------------------------------------------------ 5. refusal
def test_a_graph_over_max_nodes_is_refused_and_the_others_keep_their_values(H):
    from hcatgnet_amd.shapley import ShapleySampling
    c0 = _case("ragged-onehot25")
    sizes = torch.bincount(c0.batch, minlength=c0.B)
    big = sizes == sizes.max()
    assert 0 < int(big.sum()) < c0.B
    sv = ShapleySampling(SR.model_from_params(H, c0.params).cuda())
    gb = _gpu_batch(H, c0)
    perm = _perm(H, c0, gb)
    honest = _clone(sv(gb, permutations=perm))
    c = _Case()
    c.__dict__.update(c0.__dict__)
    c.max_nodes = int(sizes.max()) - 1
    gb = _gpu_batch(H, c)
    r = sv(gb, permutations=perm, samples_per_launch=2)
    assert sv.last_path == "fused"
    torch.cuda.synchronize()
    status = gb._hcg_plan.status
    word = int(status[0].item())
    status.zero_()                                                    # (shared per device: leave it clean for the next test)
    assert word & SHAPE_LIMIT
    node_big = big[c.batch].cuda()
    edge_big = big[c.batch[c.ei[1]]].cuda()
    assert torch.equal(r.node_attr[~node_big], honest[0][~node_big]) and torch.equal(r.edge_attr[~edge_big], honest[1][~edge_big])
    assert torch.equal(r.out_full[~big.cuda()], honest[2][~big.cuda()]) and torch.equal(r.out_base[~big.cuda()], honest[3][~big.cuda()])
    assert float(r.node_attr[node_big].abs().max()) == 0.0 and float(r.edge_attr[edge_big].abs().max()) == 0.0
    assert float(r.out_full[big.cuda()].abs().max()) == 0.0 and float(r.out_base[big.cuda()].abs().max()) == 0.0


# ------------------------------------------------------------------------------------------------ 6. fallback
def test_a_model_outside_the_limits_takes_the_loop_with_the_same_bounds(H):
    """D = 128: the batch-synchronous loop on `ExplainStep`'s any-shape path; 185 nodes: the loop on its one-launch kernel."""
    from hcatgnet_amd import synth
    from hcatgnet_amd.shapley import ShapleySampling
    from hcatgnet_amd.gcn import GCNConv
    todo = [("D = 128", dict(num_graphs=3, nodes=8, extra_bonds=2, max_degree=4, feat=6, nodes_jitter=2), 128, 0.5, None),
            ("185 nodes", dict(num_graphs=2, nodes=185, extra_bonds=4, max_degree=4, feat=4), 64, 0.1, {0})]
    for tag, bk, D, share, which in todo:
        sb = synth.make_batch(**bk)
        c = _Case()
        c.x = (sb.x * (torch.rand(sb.x.shape, generator=torch.Generator().manual_seed(X_SEED)) < share)).contiguous()
        c.ei, c.batch, c.B, c.F = sb.edge_index, sb.batch, sb.num_graphs, bk["feat"]
        c.max_nodes, c.max_edges = sb.max_nodes, sb.max_edges
        c.params = SR.rand_params(bk["feat"], D, seed=PARAM_SEED, n_classes=2)
        model = SR.model_from_params(H, c.params).cuda()
        sv = ShapleySampling(model)
        gb = _gpu_batch(H, c)
        assert "shape" in sv.reason(gb)
        perm = _perm(H, c, gb, P=1)
        print(f"\n  fallback {tag}: N {c.x.shape[0]} E {c.ei.shape[1]}")
        r = sv(gb, permutations=perm, class_index=1)
        assert sv.last_path == "loop"
        refs = SR.reference_batch(c.params, c.x, c.ei, c.batch, c.B, perm, 1, graphs=which)
        SR.check_against_reference(r, refs, c.x, c.ei, c.batch, c.B, 1, tag)
        SR.check_exact_zeros(r, c.x, c.ei)
        assert all(q.grad is None for q in model.parameters())
        for mod in model.modules():
            if isinstance(mod, GCNConv):
                assert mod.explain is False and mod._edge_mask is None


# ------------------------------------------------------------------------------------------------ 7. nothing else moves
def test_weights_and_masks_are_left_alone(H):
    from hcatgnet_amd.shapley import ShapleySampling
    from hcatgnet_amd.gcn import GCNConv
    c = _case("deep")
    model = SR.model_from_params(H, c.params).cuda()
    before = [q.detach().clone() for q in model.parameters()]
    sv = ShapleySampling(model)
    sv(_gpu_batch(H, c), n_samples=2, generator=torch.Generator().manual_seed(1), class_index=1)
    assert sv.last_path == "fused"
    for q, b in zip(model.parameters(), before):
        assert torch.equal(q.detach(), b) and q.grad is None
    for mod in model.modules():
        if isinstance(mod, GCNConv):
            assert mod.explain is False and mod._edge_mask is None
