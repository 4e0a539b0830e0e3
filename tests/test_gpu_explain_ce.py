"""GPU tests of the classification mode of `hcatgnet_amd.explain`: `ExplainStep(target_class=)` and
`ExplainFit(mode="multiclass_classification")`, the cross-entropy objective formed on chip (csrc/explain.hip, both
instantiations of k_explain_graphs).

Reference of every comparison: tests/explain_ce_ref.py -- tests/explain_fit_ref.py with the loss as a parameter -- and, for
`ExplainStep`, fp64 autograd of `F.cross_entropy(out, y, reduction="none")` through `oracle.gcn_forward(..., edge_mask=)`;
never the GPU path, never the code under test.  Bounds: the ones the regression mode carries (TOL = 1e-5 per graph on the
gradients, 2 TOL on their squares, 2^-20 on the update rule, TOL on outputs and loss with floor 1.0; a whole fit within the
bound the reference gives itself).  A cross-entropy gradient scales with exp(-margin), so the inputs are screened by the
reference alone (its own float32 restatement must meet TOL / 2 per graph); the three cases are the screened ones of
tests/explain_ce_ref.py.  Every figure is printed before it is asserted (`pytest -s`).
"""
import pytest
import torch
import torch.nn.functional as Fn

from tests import explain_ce_ref as R
from tests import explain_fit_ref as R0
from tests.helpers import rel_inf
from tests.test_gpu_explain import _decidable_masks, _model_from_params, _per_graph

pytestmark = pytest.mark.gpu
TOL = R.TOL
CE = "multiclass_classification"
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
    return H.ExplainFit(_model_from_params(H, c.params), mode=CE, **kw)


def _slow_model(H, c):
    """the same weights on a model that refuses the one-launch kernels"""
    from oracle import gcn_oracle as O
    n_conv, n_read = O.infer_depths(c.params)
    opt = H.default_options(n_convolutions=n_conv, readout_layers=n_read, embedding_dim=64, n_classes=c.C, use_fused=False)
    m = H.make_network("GCN", opt, c.x.shape[1])
    m.load_state_dict(dict(c.params))
    return m.cuda()


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


# ------------------------------------------------------------------------------------------------ 1. ExplainStep(target_class=)
def _step_reference(c, em, nm, sig, dtype=torch.float64):
    """autograd of sum_g cross_entropy(out_g, y_g) through the masked oracle -> dict(out, loss, d_em, d_nm, dx)"""
    from oracle import gcn_oracle as O
    p = {k: v.to(dtype) for k, v in c.params.items()}
    s = torch.sigmoid if sig else (lambda t: t)
    em_ = em.to(dtype).clone().requires_grad_(True)
    nm_ = nm.to(dtype).clone().requires_grad_(True) if nm is not None else None
    x_ = c.x.to(dtype).clone().requires_grad_(True)
    xin = x_ * s(nm_) if nm_ is not None else x_
    out, _ = O.gcn_forward(p, xin, c.ei, c.batch, c.B, edge_mask=s(em_))
    loss = Fn.cross_entropy(out, c.target, reduction="none")
    loss.sum().backward()
    return dict(out=out.detach(), loss=loss.detach(), d_em=em_.grad, d_nm=nm_.grad if nm_ is not None else None, dx=x_.grad)


_masks = {}


def _step_inputs(c, sig, use_nm):
    """decidable masks of a case (tests/test_gpu_explain.py `_decidable_masks`), the fp64 reference on them, and the input
    condition: the reference's own float32 restatement meets TOL / 2 per graph on every gradient"""
    key = (c.name, sig, use_nm)
    if key not in _masks:
        em, nm = _decidable_masks(c.params, c.x, c.ei, c.batch, c.B, sig, use_nm)
        ref = _step_reference(c, em, nm, sig)
        r32 = _step_reference(c, em, nm, sig, torch.float32)
        eg = c.batch[c.ei[1]]
        own = dict(edge=_per_graph(r32["d_em"], ref["d_em"], eg, c.B), dx=_per_graph(r32["dx"], ref["dx"], c.batch, c.B))
        if use_nm:
            own["node"] = _per_graph(r32["d_nm"], ref["d_nm"], c.batch, c.B)
        print(f"    {c.name} sigmoid={sig} node mask={use_nm}: the float32 oracle against fp64, per graph: "
              + "  ".join(f"{k} {v:.2e}" for k, v in own.items()))
        assert all(v <= 0.5 * TOL for v in own.values()), ("ill-conditioned inputs", own)
        _masks[key] = (em, nm, ref)
    return _masks[key]


def _check_step(step, gb, c, sig, use_nm, expect_path, tag):
    em, nm, ref = _step_inputs(c, sig, use_nm)
    r = step(gb, em.cuda(), nm.cuda() if use_nm else None, target_class=c.target.cuda(), want_dx=True)
    assert step.last_path == expect_path
    eg = c.batch[c.ei[1]]
    fig = dict(out=rel_inf(r.out, ref["out"], floor=1.0),
               loss=float(((r.loss.double().cpu() - ref["loss"]).abs() / ref["loss"].abs().clamp_min(1.0)).max()),
               edge=_per_graph(r.d_edge_mask, ref["d_em"], eg, c.B), dx=_per_graph(r.dx, ref["dx"], c.batch, c.B))
    if use_nm:
        fig["node"] = _per_graph(r.d_node_mask, ref["d_nm"], c.batch, c.B)
    else:
        assert r.d_node_mask is None
    print(f"    {tag} sigmoid={sig} node mask={use_nm} (per graph): " + "  ".join(f"{k} {v:.2e}" for k, v in fig.items()))
    assert all(v <= TOL for v in fig.values()), (tag, fig)
    assert tuple(r.out.shape) == (c.B, c.C) and tuple(r.loss.shape) == (c.B,) and bool(torch.isfinite(r.loss).all())


@pytest.mark.parametrize("name", list(R.MAIN))
def test_explain_step_with_class_indices(H, name):
    """Both mask forms, with and without a node mask, on the one-launch kernel; and the any-shape path on the same bounds."""
    from hcatgnet_amd.explain import ExplainStep
    c = R.case(name)
    gb = _gpu_batch(H, c)
    model = _model_from_params(H, c.params)
    for sig in (True, False):
        step = ExplainStep(model, apply_sigmoid=sig)
        assert step.reason(gb) is None
        for use_nm in (True, False):
            _check_step(step, gb, c, sig, use_nm, "fused", name)
    slow = ExplainStep(_slow_model(H, c))
    assert "disabled" in slow.reason(gb)
    _check_step(slow, gb, c, True, True, "autograd", name + " (autograd path)")
    with pytest.raises(ValueError, match="at most one"):
        step(gb, torch.zeros(c.ei.shape[1]).cuda(), target_class=c.target.cuda(), dout=torch.ones(c.B, c.C).cuda())


# ------------------------------------------------------------------------------------------------ 2. one epoch, in pieces
@pytest.mark.parametrize("name", list(R.MAIN))
def test_one_epoch_from_a_given_state(H, name):
    """(a) the fresh state: step 0, no regulariser, discovers the hard masks; (b) the reference's state after 3 epochs."""
    c = R.case(name)
    fit, gb = _fit(H, c), _gpu_batch(H, c)
    assert fit.reason(gb) is None and fit.mode == CE
    states, _, _ = R.reference(c, c.warm)
    assert torch.equal(states[-1]["n_hard"], c.x != 0) and torch.equal(states[-1]["e_hard"], c.ei[0] != c.ei[1])
    for s_in in _two_states(c):
        got = _run(fit, gb, c, s_in, 1)
        assert fit.last_path == "fused"
        R.check_one_epoch(c, s_in, got, name)


def test_default_and_explicit_targets(H):
    """Without `target` the argmax of the model's own unmasked output is held (computed on the device); an explicit target
    one class off it goes through the same code and meets the same checks."""
    c = R.case("c3x16")
    fit, gb = _fit(H, c, epochs=2), _gpu_batch(H, c)
    held = fit._target(gb, None)
    assert held.is_cuda and held.dtype == torch.int64 and torch.equal(held.cpu(), c.target)
    a = fit(gb, generator=torch.Generator().manual_seed(3))
    assert fit.last_path == "fused"
    first = [t.clone() for t in (a.edge_mask, a.node_mask, a.out, a.loss_history)]
    z = fit(gb, target=c.target.cuda(), generator=torch.Generator().manual_seed(3))
    for p, q in zip(first, (z.edge_mask, z.node_mask, z.out, z.loss_history)):
        assert torch.equal(p, q)
    k = R.off_argmax(c)
    for s_in in _two_states(k):
        got = _run(fit, gb, k, s_in, 1)
        assert fit.last_path == "fused"
        R.check_one_epoch(k, s_in, got, "c3x16, target off the argmax")


# ------------------------------------------------------------------------------------------------ 3. split invariance
@pytest.mark.parametrize("name", ["c3x16", "c8x16"])
def test_split_into_launches_is_bitwise_the_single_launch(H, name):
    """12 epochs in one launch, as 12 launches of 1, as 5 + 5 + 2 and as 5 + 7 through the returned state; run to run; and
    a graph alone against the same graph inside the batch -- all bitwise, in state, history, outputs and masks."""
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


# ------------------------------------------------------------------------------------------------ 4. a whole fit
@pytest.mark.parametrize("name", ["c3x16", "c8x16"])
def test_a_whole_fit_against_the_fp64_reference(H, name):
    """30 epochs.  Every entry of the loss history within TOL (floor 1.0); the final masks within the bound the reference
    gives for itself under gradient perturbations of TOL (capped at 0.25 lr: above it the test fails)."""
    c = R.case(name)
    fit, gb = _fit(H, c), _gpu_batch(H, c)
    s0 = R.rounded(R.reference(c, 0)[0][0])
    got = _run(fit, gb, c, s0, 30)
    assert fit.last_path == "fused"
    R.check_whole_fit(c, 30, got, name)


# ------------------------------------------------------------------------------------------------ 5. edge cases, 6. the limit
def test_edge_cases(H):
    """A one-node graph without edges, a graph whose x is all zero (no hard node entry: nothing of it moves, no NaN), an
    explicit (i, i) edge (gradient exactly 0: flag off, mask 0, logit unchanged) and a normal graph, with a C = 3 model."""
    from hcatgnet_amd.explain import ExplainStep
    c = R.case("edge-cases")
    fit, gb = _fit(H, c), _gpu_batch(H, c)
    for s_in in _two_states(c):
        got = _run(fit, gb, c, s_in, 1)
        assert fit.last_path == "fused"
        R.check_one_epoch(c, s_in, got, "edge-cases")
        g = got["state"]
        assert not bool(g["e_hard"][c.self_loop]) and float(got["edge_mask"][c.self_loop]) == 0.0
        assert float(g["e"][c.self_loop]) == float(s_in["e"][c.self_loop]) and float(g["e_m"][c.self_loop]) == 0.0
        zero = c.batch == 1
        assert not bool(g["n_hard"][zero].any()) and torch.equal(g["n"][zero], s_in["n"][zero])
        assert float(got["node_mask"][zero].abs().max()) == 0.0
        assert g["hard_count"][1, 1] == 0 and g["hard_count"][0, 0] == 0
        assert bool(torch.isfinite(got["loss_history"]).all()) and bool(torch.isfinite(got["out"]).all())
    s0 = _two_states(c)[0]
    r = ExplainStep(fit.model)(gb, s0["e"].cuda(), s0["n"].cuda(), target_class=c.target.cuda())
    assert float(r.d_edge_mask[c.self_loop]) == 0.0 and bool(torch.isfinite(r.d_edge_mask).all()) and bool(torch.isfinite(r.loss).all())


def test_a_graph_at_the_shape_limit(H):
    """224 nodes, 1024 directed edges, C = 8, two epochs: the fresh state, then the reference's state after one."""
    c = R.case("limit")
    assert c.max_nodes == R0.NODE_LIMIT and c.max_edges == R0.EDGE_LIMIT and c.C == 8
    fit, gb = _fit(H, c), _gpu_batch(H, c)
    assert fit.reason(gb) is None and fit.lds_bytes(gb) <= 160 * 1024
    for s_in in _two_states(c):
        got = _run(fit, gb, c, s_in, 1)
        assert fit.last_path == "fused"
        R.check_one_epoch(c, s_in, got, "limit")


# ------------------------------------------------------------------------------------------------ 7. refusal
def test_a_graph_over_the_limit_is_refused_and_the_rest_untouched(H):
    """Host metadata lies (max_nodes one too small): the largest graphs are refused with HCG_STATUS_SHAPE_LIMIT, their rows of
    every output are zero and their state stays as it came; the other graphs' results are bitwise what they were."""
    c = R.case("c3x16")
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


# ------------------------------------------------------------------------------------------------ 8. paths
def test_the_loop_path_meets_the_same_bounds_and_states_cross_over(H):
    """`use_fused=False` takes the loop path (ExplainStep(target_class=)'s gradients, torch ops for the rest) with the
    whole-fit bounds; a state returned by one path continues on the other."""
    c = R.case("c3x16")
    s0 = R.rounded(R.reference(c, 0)[0][0])
    gb = _gpu_batch(H, c)
    loop = H.ExplainFit(_slow_model(H, c), mode=CE)
    assert "disabled" in loop.reason(gb)
    got = _run(loop, gb, c, s0, 30)
    assert loop.last_path == "loop"
    R.check_whole_fit(c, 30, got, "c3x16 loop path")
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
        R.check_whole_fit(c, 30, both, "c3x16 " + tag)


# ------------------------------------------------------------------------------------------------ 9. regression, as before
def test_regression_through_the_same_build(H):
    """`ExplainFit()` with default arguments on a C = 1 case still meets tests/explain_fit_ref.py's one-epoch check (belt and
    braces: tests/test_gpu_explain_fit.py is the real check)."""
    c = R0.case("onehot25")
    fit = H.ExplainFit(_model_from_params(H, c.params))
    assert fit.mode == "regression"
    gb = _gpu_batch(H, c)
    s_in = R0.rounded(R0.reference(c, 0)[0][0])
    st = R0.to_fit_state(s_in, c.batch, c.ei, c.B, "cuda")
    r = fit(gb, target=c.target.cuda(), state=st, epochs=1)
    assert fit.last_path == "fused"
    got = dict(state=R0.from_fit_state(st), out=r.out.cpu().clone(), loss=r.loss_history[-1].cpu().clone())
    R0.check_one_epoch(c, s_in, got, "onehot25, regression")
