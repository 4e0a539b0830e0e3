"""GPU tests of `hcatgnet_amd.explain.ExplainFit`: GNNExplainer's whole mask optimisation of a batch of graphs in one launch
(csrc/explain.hip, k_explain_graphs<true>).

Reference of every comparison: tests/explain_fit_ref.py, the definition on `oracle.gcn_forward(..., edge_mask=)` under fp64
autograd on the CPU -- never the GPU path, never the code under test.  That module also states the inputs, the decidability
screen and the checks, which tests/test_host_explain_fit.py applies to the loop path on CPU tensors.

No ill-conditioned quantity is compared elementwise.  Adam's first step on an entry with a tiny gradient is close to a sign
function of that gradient, so one epoch is checked in pieces (`check_one_epoch`): the hard flags; the gradient the step used,
recovered from the first moment (per graph rel_inf <= TOL = 1e-5, the bound `ExplainStep`'s gradients carry); its square
from the second moment (2 TOL of the graph's max g^2); the update rule evaluated in fp64 from the run's OWN moments
(relative 2^-20 of |logit| + |step|); loss and outputs (TOL, floor 1.0).  A fit split into launches must be BITWISE the
single launch, which carries the one-epoch checks to any number of epochs; and a whole fit is compared with a bound
computed from the reference alone (`mask_bound`).  Every figure is printed before it is asserted (`pytest -s`).
"""
import pytest
import torch

from tests import explain_fit_ref as R
from tests.test_gpu_explain import _model_from_params

pytestmark = pytest.mark.gpu
SHAPE_LIMIT = 16          # HCG_STATUS_SHAPE_LIMIT


@pytest.fixture(scope="module")
def H():
    import os
    import hcatgnet_amd
    import __graft_entry__
    from hcatgnet_amd import _lib
    if not os.path.isfile(_lib.LIB_PATH):
        __graft_entry__.build()
    return hcatgnet_amd


def _gpu_batch(H, c, **kw):
    meta = dict(max_nodes=c.max_nodes, max_edges=c.max_edges, edges_grouped=True)
    meta.update(kw)
    return H.Batch(c.x.cuda(), c.ei.cuda(), c.batch.cuda(), c.B, **meta)


def _fit(H, c, **kw):
    return H.ExplainFit(_model_from_params(H, c.params), **kw)


def _run(fit, gb, c, s_in, epochs, **kw):
    """`epochs` epochs from the reference-style state `s_in` -> everything the call returned, on the CPU"""
    st = R.to_fit_state(s_in, c.batch, c.ei, c.B, "cuda")
    r = fit(gb, target=c.target.cuda(), state=st, epochs=epochs, **kw)
    assert r.state is st
    return dict(state=R.from_fit_state(st), out=r.out.cpu().clone(), loss=r.loss_history[-1].cpu().clone(),
                loss_history=r.loss_history.cpu().clone(), edge_mask=r.edge_mask.cpu().clone(), node_mask=r.node_mask.cpu().clone())


def _same(a, b):
    """two results of `_run` bitwise"""
    for k in a:
        if k == "state":
            for q in a[k]:
                assert (torch.equal(a[k][q], b[k][q]) if torch.is_tensor(a[k][q]) else a[k][q] == b[k][q]), q
        else:
            assert torch.equal(a[k], b[k]), k


def _two_states(c):
    """the fresh state, and the fp64 reference's state after c.warm epochs rounded to float32"""
    states, _, _ = R.reference(c, c.warm)
    return [R.rounded(states[0]), R.rounded(states[c.warm])]


# ------------------------------------------------------------------------------------------------ 1. one epoch, in pieces
@pytest.mark.parametrize("name", ["onehot25", "deep", "dense64"])
def test_one_epoch_from_a_given_state(H, name):
    """(a) the fresh state: step 0, no regulariser, discovers the hard masks; (b) the reference's state after 3 epochs."""
    c = R.case(name)
    fit, gb = _fit(H, c), _gpu_batch(H, c)
    assert fit.reason(gb) is None
    states, _, _ = R.reference(c, c.warm)
    assert torch.equal(states[-1]["n_hard"], c.x != 0) and torch.equal(states[-1]["e_hard"], c.ei[0] != c.ei[1])
    for s_in in _two_states(c):
        got = _run(fit, gb, c, s_in, 1)
        assert fit.last_path == "fused"
        R.check_one_epoch(c, s_in, got, name)


# ------------------------------------------------------------------------------------------------ 2. split invariance
@pytest.mark.parametrize("name", ["onehot25", "deep"])
def test_split_into_launches_is_bitwise_the_single_launch(H, name):
    """12 epochs in one launch, as 12 launches of 1 and as 5 + 7; run to run; and a graph alone against the same graph
    inside the batch -- all bitwise, in state, history, outputs and masks."""
    c = R.case(name)
    fit, gb = _fit(H, c), _gpu_batch(H, c)
    s0 = R.rounded(R.reference(c, 0)[0][0])
    one = _run(fit, gb, c, s0, 12)
    assert fit.last_path == "fused" and one["state"]["step"] == 12
    _same(one, _run(fit, gb, c, s0, 12))                                    # run to run
    _same(one, _run(fit, gb, c, s0, 12, epochs_per_launch=1))
    _same(one, _run(fit, gb, c, s0, 12, epochs_per_launch=5))               # 5 + 5 + 2
    st = R.to_fit_state(s0, c.batch, c.ei, c.B, "cuda")                     # 5 + 7: two calls, the state carried over
    tg = c.target.cuda()
    r5 = fit(gb, target=tg, state=st, epochs=5)
    h5 = r5.loss_history.cpu().clone()
    r7 = fit(gb, target=tg, state=st, epochs=7)
    assert st.step == 12
    two = dict(state=R.from_fit_state(st), out=r7.out.cpu(), loss=r7.loss_history[-1].cpu(),
               loss_history=torch.cat([h5, r7.loss_history.cpu()]), edge_mask=r7.edge_mask.cpu(), node_mask=r7.node_mask.cpu())
    _same(one, two)
    # every graph alone
    nptr = torch.zeros(c.B + 1, dtype=torch.long); nptr[1:] = torch.bincount(c.batch, minlength=c.B).cumsum(0)
    eptr = torch.zeros(c.B + 1, dtype=torch.long); eptr[1:] = torch.bincount(c.batch[c.ei[1]], minlength=c.B).cumsum(0)
    for g in range(c.B):
        a, b, ea, eb = int(nptr[g]), int(nptr[g + 1]), int(eptr[g]), int(eptr[g + 1])
        k = R.Case()
        k.x, k.ei, k.batch, k.B = c.x[a:b].contiguous(), (c.ei[:, ea:eb] - a).contiguous(), torch.zeros(b - a, dtype=torch.long), 1
        k.max_nodes, k.max_edges, k.target = b - a, eb - ea, c.target[g:g + 1].contiguous()
        sg = {q: (v[ea:eb].clone() if q.startswith("e") else v[a:b].clone()) if torch.is_tensor(v) else v for q, v in s0.items()}
        alone = _run(fit, _gpu_batch(H, k), k, sg, 12)
        assert fit.last_path == "fused"
        assert torch.equal(alone["out"], one["out"][g:g + 1]) and torch.equal(alone["loss_history"], one["loss_history"][:, g:g + 1]), g
        assert torch.equal(alone["edge_mask"], one["edge_mask"][ea:eb]) and torch.equal(alone["node_mask"], one["node_mask"][a:b]), g
        for q in ("e", "e_m", "e_v", "e_hard"):
            assert torch.equal(alone["state"][q], one["state"][q][ea:eb]), (g, q)
        for q in ("n", "n_m", "n_v", "n_hard"):
            assert torch.equal(alone["state"][q], one["state"][q][a:b]), (g, q)
        assert torch.equal(alone["state"]["hard_count"], one["state"]["hard_count"][g:g + 1]), g


# ------------------------------------------------------------------------------------------------ 3. a whole fit
@pytest.mark.parametrize("name", ["onehot25", "deep"])
def test_a_whole_fit_against_the_fp64_reference(H, name):
    """30 epochs.  Every entry of the loss history within TOL (floor 1.0); the final masks within the bound the reference
    gives for itself under gradient perturbations of TOL (capped at 0.25 lr: above it the test fails)."""
    c = R.case(name)
    fit, gb = _fit(H, c), _gpu_batch(H, c)
    s0 = R.rounded(R.reference(c, 0)[0][0])
    got = _run(fit, gb, c, s0, 30)
    assert fit.last_path == "fused"
    R.check_whole_fit(c, 30, got, name)


# ------------------------------------------------------------------------------------------------ 4. edge cases, the limit
def test_edge_cases(H):
    """A one-node graph without edges, a graph whose x is all zero (no hard node entry: nothing of it moves, no NaN), an
    explicit (i, i) edge (flag off, mask 0, logit unchanged) and a normal graph."""
    c = R.case("edge-cases")
    fit, gb = _fit(H, c), _gpu_batch(H, c)
    for s_in in _two_states(c):
        got = _run(fit, gb, c, s_in, 1)
        assert fit.last_path == "fused"
        R.check_one_epoch(c, s_in, got, "edge-cases")
        g = got["state"]
        assert not bool(g["e_hard"][c.self_loop]) and float(got["edge_mask"][c.self_loop]) == 0.0
        assert float(g["e"][c.self_loop]) == float(s_in["e"][c.self_loop])
        zero = c.batch == 1
        assert not bool(g["n_hard"][zero].any()) and torch.equal(g["n"][zero], s_in["n"][zero])
        assert float(got["node_mask"][zero].abs().max()) == 0.0
        assert g["hard_count"][1, 1] == 0 and g["hard_count"][0, 0] == 0
        assert bool(torch.isfinite(got["loss_history"]).all())


def test_a_graph_at_the_shape_limit(H):
    """224 nodes, 1024 directed edges, two epochs: the fresh state, then the reference's state after one."""
    c = R.case("limit")
    assert c.max_nodes == R.NODE_LIMIT and c.max_edges == R.EDGE_LIMIT
    fit, gb = _fit(H, c), _gpu_batch(H, c)
    assert fit.reason(gb) is None and fit.lds_bytes(gb) <= 160 * 1024
    for s_in in _two_states(c):
        got = _run(fit, gb, c, s_in, 1)
        assert fit.last_path == "fused"
        R.check_one_epoch(c, s_in, got, "limit")


def test_a_graph_over_the_limit_is_refused_and_the_rest_untouched(H):
    """Host metadata lies (max_nodes one too small): the largest graphs are refused with HCG_STATUS_SHAPE_LIMIT, their rows of
    every output are zero and their state stays as it came; the other graphs' results are bitwise what they were."""
    c = R.case("onehot25")
    fit = _fit(H, c)
    s0 = R.rounded(R.reference(c, 0)[0][0])
    honest = _run(fit, _gpu_batch(H, c), c, s0, 3)
    sizes = torch.bincount(c.batch, minlength=c.B)
    big = sizes == sizes.max()
    assert 0 < int(big.sum()) < c.B
    gb = _gpu_batch(H, c, max_nodes=int(sizes.max()) - 1)
    got = _run(fit, gb, c, s0, 3)
    assert fit.last_path == "fused"
    torch.cuda.synchronize()
    status = gb._hcg_plan.status
    word = int(status[0].item())
    status.zero_()                                                    # (shared per device: leave it clean for the next test)
    assert word & SHAPE_LIMIT
    nb, eb = big[c.batch], big[c.batch[c.ei[1]]]
    assert torch.equal(got["out"][~big], honest["out"][~big]) and torch.equal(got["loss_history"][:, ~big], honest["loss_history"][:, ~big])
    assert torch.equal(got["edge_mask"][~eb], honest["edge_mask"][~eb]) and torch.equal(got["node_mask"][~nb], honest["node_mask"][~nb])
    for q, m in (("e", eb), ("e_m", eb), ("e_v", eb), ("e_hard", eb), ("n", nb), ("n_m", nb), ("n_v", nb), ("n_hard", nb)):
        assert torch.equal(got["state"][q][~m], honest["state"][q][~m]), q
        assert torch.equal(got["state"][q][m], s0[q][m]), q
    assert float(got["out"][big].abs().max()) == 0.0 and float(got["loss_history"][:, big].abs().max()) == 0.0
    assert float(got["edge_mask"][eb].abs().max()) == 0.0 and float(got["node_mask"][nb].abs().max()) == 0.0


# ------------------------------------------------------------------------------------------------ 5. paths
def test_the_loop_path_meets_the_same_bounds_and_states_cross_over(H):
    """`use_fused=False` takes the loop path (ExplainStep's gradients, torch ops for the rest) with the whole-fit bounds; a
    state returned by one path continues on the other."""
    c = R.case("onehot25")
    s0 = R.rounded(R.reference(c, 0)[0][0])
    gb = _gpu_batch(H, c)
    params = dict(c.params)
    opt = H.default_options(n_convolutions=2, readout_layers=2, embedding_dim=64, n_classes=1, use_fused=False)
    slow = H.make_network("GCN", opt, c.x.shape[1])
    slow.load_state_dict(params)
    loop = H.ExplainFit(slow.cuda())
    assert "disabled" in loop.reason(gb)
    got = _run(loop, gb, c, s0, 30)
    assert loop.last_path == "loop"
    R.check_whole_fit(c, 30, got, "onehot25 loop path")
    # 15 epochs on one path, 15 on the other, both ways
    fused = _fit(H, c)
    for first, second, tag in ((fused, loop, "fused then loop"), (loop, fused, "loop then fused")):
        st = R.to_fit_state(s0, c.batch, c.ei, c.B, "cuda")
        tg = c.target.cuda()
        r1 = first(gb, target=tg, state=st, epochs=15)
        h1 = r1.loss_history.cpu().clone()
        r2 = second(gb, target=tg, state=st, epochs=15)
        assert {first.last_path, second.last_path} == {"fused", "loop"} and st.step == 30
        both = dict(state=R.from_fit_state(st), loss_history=torch.cat([h1, r2.loss_history.cpu()]),
                    edge_mask=r2.edge_mask.cpu(), node_mask=r2.node_mask.cpu())
        R.check_whole_fit(c, 30, both, "onehot25 " + tag)


def test_default_target_fresh_state_and_steady_state(H):
    """Without `target` the model's own prediction is held; without `state` a fresh one is drawn from the generator; with
    both given a call allocates nothing; no mask stays attached to the model and no weight moves."""
    from hcatgnet_amd.gcn import GCNConv
    c = R.case("onehot25")
    model = _model_from_params(H, c.params)
    before = [q.detach().clone() for q in model.parameters()]
    fit, gb = H.ExplainFit(model, epochs=4), _gpu_batch(H, c)
    r = fit(gb, generator=torch.Generator().manual_seed(3))
    assert fit.last_path == "fused" and r.state.step == 4 and tuple(r.loss_history.shape) == (4, c.B)
    first = [t.clone() for t in (r.edge_mask, r.node_mask, r.out, r.loss_history)]
    with torch.no_grad():
        tg = model(gb).reshape(c.B, -1).clone()
    st = fit.init_state(gb, torch.Generator().manual_seed(3))
    r = fit(gb, target=tg, state=st)
    for a, b in zip(first, (r.edge_mask, r.node_mask, r.out, r.loss_history)):
        assert torch.equal(a, b)
    torch.cuda.synchronize()
    n0 = torch.cuda.memory_stats()["allocation.all.allocated"]
    fit(gb, target=tg, state=st)
    fit(gb, target=tg, state=st, epochs_per_launch=2)
    torch.cuda.synchronize()
    assert torch.cuda.memory_stats()["allocation.all.allocated"] == n0
    assert st.step == 12
    for q, b in zip(model.parameters(), before):
        assert torch.equal(q.detach(), b) and q.grad is None
    for mod in model.modules():
        if isinstance(mod, GCNConv):
            assert mod.explain is False and mod._edge_mask is None
