"""GPU tests of `hcatgnet_amd.attribution.IntegratedGradients`: the whole path of every graph of a batch in one launch
(csrc/explain.hip, k_explain_graphs<false, true>).  tests/integrated_ref.py states the fp64 reference, the decidability screen
(node features re-drawn until no graph is flagged at any quadrature point) and the bound (TOL = 1e-5 per graph).  Every figure
is printed before it is asserted (`pytest -s`).

The default step count (50) cannot be screened -- almost every graph sits within the margins at one of 50 points -- so that
run is judged against the existing kernel: sum_k w_k ExplainStep(masks = alpha_k, dout = one-hot), summed in float64 on the
host.  The two share the forward's arithmetic and so make the same branch decisions."""
import os
from types import SimpleNamespace

import pytest
import torch
import torch.nn.functional as Fn

from tests import integrated_ref as R
from tests.helpers import rel_inf
from tests.test_gpu_explain import PARAM_SEED, _per_graph, _rand_params, _rowwise_linear

pytestmark = pytest.mark.gpu
TOL = R.TOL
SHAPE_LIMIT = 16          # HCG_STATUS_SHAPE_LIMIT


@pytest.fixture(scope="module")
def H():
    import hcatgnet_amd
    from hcatgnet_amd import _lib
    if not os.path.isfile(_lib.LIB_PATH):
        import __graft_entry__
        __graft_entry__.build()
    return hcatgnet_amd


def _ig(H, c, **kw):
    kw.setdefault("method", c.method)
    return H.IntegratedGradients(R.model(H, c, "cuda"), n_steps=c.n_steps, **kw)


def _keep(r):
    return [t.clone() for t in r]


def _same(a, b):
    return all(torch.equal(p, q) for p, q in zip(a, b))


def _ptrs(c):
    nptr = torch.zeros(c.B + 1, dtype=torch.long); nptr[1:] = torch.bincount(c.batch, minlength=c.B).cumsum(0)
    eptr = torch.zeros(c.B + 1, dtype=torch.long); eptr[1:] = torch.bincount(c.edge_owner, minlength=c.B).cumsum(0)
    return nptr, eptr


# ------------------------------------------------------------------------------------------------ 1. parity (and 6. the shape limit)
@pytest.mark.parametrize("method", ["gausslegendre", "riemann_middle"])
@pytest.mark.parametrize("name", list(R.CASES) + ["golden"])
def test_parity_with_the_fp64_oracle(H, name, method):
    c = R.case(name, method)
    ig, gb = _ig(H, c), R.batch(H, c, "cuda")
    assert ig.reason(gb) is None
    r = ig(gb, class_index=c.cls)
    assert ig.last_path == "fused"
    R.check(c, r, f"{name} {method}")
    delta = ig.convergence_delta(gb, r)
    print(f"    convergence delta per graph (a diagnostic, not a bound): {[f'{v:+.2e}' for v in delta.tolist()]}")
    assert delta.dtype == torch.float64 and tuple(delta.shape) == (c.B,)
    if name == "limit224":
        lds = ig.lds_bytes(gb)
        print(f"    224-node graphs: LDS {lds} bytes")
        assert c.max_nodes == 224 and 0 < lds <= 160 * 1024


# ------------------------------------------------------------------------------------------------ 2. split
def test_the_launch_split_is_exact(H):
    c = R.case("small30")
    assert c.n_steps == 6
    ig, gb = _ig(H, c), R.batch(H, c, "cuda")
    one = _keep(ig(gb, steps_per_launch=6))
    assert ig.last_path == "fused"
    assert _same(one, _keep(ig(gb)))                                  # (the default: one launch here)
    for per in (1, 2, 4):
        assert _same(one, _keep(ig(gb, steps_per_launch=per))), per
    # the launch with step_first = 0 starts from 0 whatever the accumulators hold
    for k in ("node", "edge", "full", "base"):
        ig._bufs[k].fill_(float("nan"))
    assert _same(one, _keep(ig(gb, steps_per_launch=6)))
    for k in ("node", "edge"):
        ig._bufs[k].fill_(float("nan"))
    assert _same(one, _keep(ig(gb, steps_per_launch=4)))
    R.check(c, ig(gb, steps_per_launch=1), "small30 one step per launch")


# ------------------------------------------------------------------------------------------------ 3. batching
def test_batched_equals_one_by_one_bitwise(H):
    c = R.case("real-size")
    model = R.model(H, c, "cuda")
    ig = H.IntegratedGradients(model, n_steps=c.n_steps)
    gb = R.batch(H, c, "cuda")
    full = _keep(ig(gb))
    assert _same(full, _keep(ig(gb)))
    nptr, eptr = _ptrs(c)
    single = H.IntegratedGradients(model, n_steps=c.n_steps)
    for g in range(c.B):
        a, b, ea, eb = int(nptr[g]), int(nptr[g + 1]), int(eptr[g]), int(eptr[g + 1])
        one = H.Batch(c.x[a:b].cuda(), (c.ei[:, ea:eb] - a).contiguous().cuda(), torch.zeros(b - a, dtype=torch.long).cuda(), 1,
                      max_nodes=b - a, max_edges=eb - ea, edges_grouped=True)
        r = single(one)
        assert single.last_path == "fused"
        assert torch.equal(r.node_attr, full[0][a:b]) and torch.equal(r.edge_attr, full[1][ea:eb]), g
        assert torch.equal(r.out_full, full[2][g:g + 1]) and torch.equal(r.out_base, full[3][g:g + 1]), g


# ------------------------------------------------------------------------------------------------ 4. the default step count
def test_default_step_count_against_explain_step(H):
    from hcatgnet_amd.explain import ExplainStep
    c = R.case("ragged")
    model = R.model(H, c, "cuda")
    ig = H.IntegratedGradients(model)
    assert ig.n_steps == 50 and ig.method == "gausslegendre"
    gb = R.batch(H, c, "cuda")
    r = ig(gb, steps_per_launch=50)
    assert ig.last_path == "fused"
    got = _keep(r)
    alpha, weight = H.quadrature("gausslegendre", 50)
    step = ExplainStep(model, apply_sigmoid=False)
    (N, F), E = c.x.shape, c.ei.shape[1]
    onehot = torch.zeros(c.B, 1).cuda(); onehot[:, 0] = 1.0
    node, edge = torch.zeros(N, F, dtype=torch.float64), torch.zeros(E, dtype=torch.float64)
    for k in range(50):
        a = float(alpha[k])
        s = step(gb, torch.full((E,), a).cuda(), torch.full((N, F), a).cuda(), dout=onehot)
        assert step.last_path == "fused"
        node += float(weight[k]) * s.d_node_mask.double().cpu()
        edge += float(weight[k]) * s.d_edge_mask.double().cpu()
    fig = dict(node=_per_graph(got[0], node, c.batch, c.B), edge=_per_graph(got[1], edge, c.edge_owner, c.B))
    print(f"\n    50 points, one launch against sum_k w_k ExplainStep (per graph): node {fig['node']:.2e}  edge {fig['edge']:.2e}")
    assert all(v <= TOL for v in fig.values()), fig
    # one point: the step's gradients themselves, bitwise (fmaf(1, g, 0) = g)
    one = H.IntegratedGradients(model, n_steps=1, method="riemann_middle")
    q = _keep(one(gb))
    s = step(gb, torch.full((E,), 0.5).cuda(), torch.full((N, F), 0.5).cuda(), dout=onehot)
    same = torch.equal(q[0], s.d_node_mask) and torch.equal(q[1], s.d_edge_mask)
    print(f"    per-step gradients at alpha = 0.5 bitwise ExplainStep's: {same}")
    assert same


# ------------------------------------------------------------------------------------------------ 5. exact zeros
def test_self_loop_edge_and_zero_features_get_exactly_zero(H):
    from hcatgnet_amd import synth
    sb = synth.make_batch(num_graphs=5, nodes=20, extra_bonds=2, max_degree=4, feat=25, nodes_jitter=4)
    eg = sb.batch[sb.edge_index[1]]
    pos = int((eg <= 1).sum()) - 3                              # inside graph 1's edge block
    node = int(sb.edge_index[0, pos])
    ei = torch.cat([sb.edge_index[:, :pos], torch.tensor([[node], [node]]), sb.edge_index[:, pos:]], 1).contiguous()
    x = sb.x.clone()
    zero = torch.rand(x.shape, generator=torch.Generator().manual_seed(3)) < 0.4
    x[zero] = 0.0
    c = R.custom(_rand_params(25, 64, seed=PARAM_SEED), x, ei, sb.batch, sb.num_graphs, 4, screen=False)
    ig = _ig(H, c)
    r = ig(R.batch(H, c, "cuda"))
    assert ig.last_path == "fused"
    assert float(r.edge_attr[pos]) == 0.0 and int((r.edge_attr != 0).sum()) == ei.shape[1] - 1
    assert int(zero.sum()) > 100 and float(r.node_attr[zero.cuda()].abs().max()) == 0.0
    assert int((r.node_attr[~zero.cuda()] != 0).sum()) > 0.9 * int((~zero).sum())
    assert float(c.ref["edge"][pos]) == 0.0 and float(c.ref["node"][zero].abs().max()) == 0.0


def test_a_single_node_without_edges(H):
    gen = torch.Generator().manual_seed(5)
    params = _rand_params(25, 64, seed=PARAM_SEED)
    # alone in its batch (E = 0), and beside a three-node path
    x1 = torch.randn(1, 25, generator=gen)
    c = R.custom(params, x1, torch.zeros(2, 0, dtype=torch.int64), torch.zeros(1, dtype=torch.int64), 1, 3, screen=False)
    ig = _ig(H, c)
    r = ig(R.batch(H, c, "cuda"))
    assert ig.last_path == "fused" and r.edge_attr.numel() == 0 and bool(torch.isfinite(r.node_attr).all())
    fig = R.figures(c, r)
    print(f"\n    one node, no edges: node {fig['node']:.2e}  out_full {fig['out_full']:.2e}  out_base {fig['out_base']:.2e}")
    assert fig["node"] <= TOL and fig["out_full"] <= TOL and fig["out_base"] <= TOL
    x2 = torch.cat([x1, torch.randn(3, 25, generator=gen)])
    ei = torch.tensor([[1, 2, 2, 3], [2, 1, 3, 2]])
    c = R.custom(params, x2, ei, torch.tensor([0, 1, 1, 1]), 2, 3, screen=False)
    r2 = _keep(_ig(H, c)(R.batch(H, c, "cuda")))
    assert torch.equal(r2[0][:1], r.node_attr) and torch.equal(r2[2][:1], r.out_full) and bool(torch.isfinite(r2[0]).all())
    assert int((c.edge_owner == 0).sum()) == 0 and tuple(r2[1].shape) == (4,)


def test_exact_max_pool_ties_give_identical_rows(H, monkeypatch):
    """The graphs of tests/test_gpu_explain.py::test_exact_max_pool_ties_split_evenly: a centre with k = 2..4 leaves that
    share one feature row.  The masks are uniform here, so the twins stay bit-identical through every layer at every point,
    the max-pool gradient is split evenly among them, and their attribution rows are bit-identical.  The fp64 reference runs
    its dense products through `_rowwise_linear` for the reason given there."""
    from oracle import gcn_oracle as O
    gen = torch.Generator().manual_seed(11)
    xs, eis, bs, off, B = [], [], [], 0, 12
    for g in range(B):
        k = 2 + g % 3
        n = 1 + k + 3
        x = torch.randn(n, 25, generator=gen); x[1:1 + k] = x[1]
        bonds = [(0, j) for j in range(1, 1 + k)] + [(0, k + 1), (k + 1, k + 2), (k + 2, k + 3)]
        e = []
        for i, j in bonds:
            e += [[i, j], [j, i]]
        xs.append(x); eis.append(torch.tensor(e).t() + off); bs.append(torch.full((n,), g)); off += n
    x, ei, bv = torch.cat(xs), torch.cat(eis, 1), torch.cat(bs)
    first = torch.zeros(B + 1, dtype=torch.long); first[1:] = torch.bincount(bv, minlength=B).cumsum(0)

    def redraw(x, m):                                       # new rows for the flagged graphs, their leaves twins again
        x[m] = torch.randn(int(m.sum()), 25, generator=gen)
        for g in range(B):
            x[first[g] + 1:first[g] + 1 + 2 + g % 3] = x[first[g] + 1]

    with monkeypatch.context() as mp:
        mp.setattr(O, "F", SimpleNamespace(linear=_rowwise_linear, leaky_relu=Fn.leaky_relu, mse_loss=Fn.mse_loss))
        c = R.custom(_rand_params(25, 64, seed=PARAM_SEED), x, ei, bv, B, 3, redraw=redraw)
    h = c.x
    assert all(torch.equal(h[first[g] + 1], h[first[g] + j]) for g in range(B) for j in range(2, 2 + g % 3 + 1))
    ig = _ig(H, c)
    r = ig(R.batch(H, c, "cuda"))
    assert ig.last_path == "fused"
    R.check(c, r, "exact ties")
    nptr, _ = _ptrs(c)
    for g in range(B):
        for j in range(2, 2 + (2 + g % 3) - 1):
            assert torch.equal(r.node_attr[nptr[g] + 1], r.node_attr[nptr[g] + j]), (g, j)
            assert torch.equal(c.ref["node"][nptr[g] + 1], c.ref["node"][nptr[g] + j]), (g, j)


# ------------------------------------------------------------------------------------------------ 7. refusal
def test_a_graph_over_the_limit_is_refused_and_the_rest_untouched(H):
    """Host metadata lies (max_nodes one too small): the largest graphs are refused with HCG_STATUS_SHAPE_LIMIT, their rows of
    every output are zero; the other graphs' results are bitwise what they were."""
    c = R.case("ragged")
    ig = _ig(H, c)
    honest = _keep(ig(R.batch(H, c, "cuda")))
    sizes = torch.bincount(c.batch, minlength=c.B)
    big = sizes == sizes.max()
    assert 0 < int(big.sum()) < c.B
    gb = R.batch(H, c, "cuda", max_nodes=int(sizes.max()) - 1)
    for k in ("node", "edge", "full", "base"):
        ig._bufs[k].fill_(7.0)
    got = [t.cpu() for t in ig(gb, steps_per_launch=3)]               # (two launches: the second one refuses it again)
    assert ig.last_path == "fused"
    torch.cuda.synchronize()
    status = gb._hcg_plan.status
    word = int(status[0].item())
    status.zero_()                                                    # (shared per device: leave it clean for the next test)
    assert word & SHAPE_LIMIT
    honest = [t.cpu() for t in honest]
    nb, eb = big[c.batch], big[c.edge_owner]
    assert torch.equal(got[0][~nb], honest[0][~nb]) and torch.equal(got[1][~eb], honest[1][~eb])
    assert torch.equal(got[2][~big], honest[2][~big]) and torch.equal(got[3][~big], honest[3][~big])
    assert float(got[0][nb].abs().max()) == 0.0 and float(got[1][eb].abs().max()) == 0.0
    assert float(got[2][big].abs().max()) == 0.0 and float(got[3][big].abs().max()) == 0.0


# ------------------------------------------------------------------------------------------------ 8. the loop path
def test_the_loop_path_meets_the_same_bound(H):
    c = R.case("ragged")
    assert c.n_steps == 4
    gb = R.batch(H, c, "cuda")
    slow = H.IntegratedGradients(R.model(H, c, "cuda", use_fused=False), n_steps=4)
    assert "disabled" in slow.reason(gb)
    r = slow(gb)
    assert slow.last_path == "loop"
    R.check(c, r, "ragged, use_fused off (loop)")
    forced = _ig(H, c).loop(gb)                                       # the loop on the one-launch ExplainStep
    R.check(c, forced, "ragged, loop() on the fused step")
    w = R.case("ragged-d128")
    wide = _ig(H, w)
    wb = R.batch(H, w, "cuda")
    assert "shape" in wide.reason(wb)
    r = wide(wb)
    assert wide.last_path == "loop"
    R.check(w, r, "ragged, embedding_dim 128 (loop)")
    assert all(q.grad is None for q in wide.model.parameters())


# ------------------------------------------------------------------------------------------------ 9. nothing else moves
def test_weights_grads_and_masks_are_left_alone_and_a_warm_call_allocates_nothing(H):
    from hcatgnet_amd.gcn import GCNConv
    c = R.case("deep")
    model = R.model(H, c, "cuda")
    before = [q.detach().clone() for q in model.parameters()]
    ig = H.IntegratedGradients(model, n_steps=c.n_steps)
    gb = R.batch(H, c, "cuda")
    first = _keep(ig(gb, class_index=c.cls))
    ig(gb, class_index=0, steps_per_launch=2)
    torch.cuda.synchronize()
    held = torch.cuda.memory_allocated()
    r = ig(gb, class_index=c.cls)
    r2 = ig(gb, class_index=c.cls, steps_per_launch=1)
    torch.cuda.synchronize()
    after = torch.cuda.memory_allocated()
    print(f"\n    bytes allocated before / after two warm calls: {held} / {after}")
    assert after == held and ig.last_path == "fused"
    assert r.node_attr.data_ptr() == r2.node_attr.data_ptr() and _same(first, r2)
    for q, b in zip(model.parameters(), before):
        assert torch.equal(q.detach(), b) and q.grad is None
    for mod in model.modules():
        if isinstance(mod, GCNConv):
            assert mod.explain is False and mod._edge_mask is None


# ------------------------------------------------------------------------------------------------ 10. the one-step modes
def test_gradient_and_saliency_are_explain_steps_gradients_at_ones(H):
    from hcatgnet_amd.explain import ExplainStep
    c = R.case("deep")
    model = R.model(H, c, "cuda")
    gb = R.batch(H, c, "cuda")
    (N, F), E = c.x.shape, c.ei.shape[1]
    onehot = torch.zeros(c.B, 2).cuda(); onehot[:, c.cls] = 1.0
    step = ExplainStep(model, apply_sigmoid=False)
    s = step(gb, torch.ones(E).cuda(), torch.ones(N, F).cuda(), dout=onehot)
    assert step.last_path == "fused"
    g = H.IntegratedGradients(model, method="gradient")
    r = g(gb, class_index=c.cls)
    assert g.last_path == "fused" and g.n_steps == 1
    assert torch.equal(r.node_attr, s.d_node_mask) and torch.equal(r.edge_attr, s.d_edge_mask) and torch.equal(r.out_full, s.out)
    assert int((r.node_attr < 0).sum()) > 0 and int((r.edge_attr < 0).sum()) > 0
    sal = H.IntegratedGradients(model, method="gradient", saliency=True)
    q = sal(gb, class_index=c.cls)
    assert sal.last_path == "fused"
    assert torch.equal(q.node_attr, s.d_node_mask.abs()) and torch.equal(q.edge_attr, s.d_edge_mask.abs())
    ref = R.reference(c.params, c.x, c.ei, c.batch, c.B, torch.ones(1), torch.ones(1), c.cls, screen=False)
    print(f"\n    gradient at ones against fp64 (whole tensor, unscreened): node {rel_inf(r.node_attr, ref['node']):.2e}  "
          f"edge {rel_inf(r.edge_attr, ref['edge']):.2e}")
