"""GPU tests of `hcatgnet_amd.explain.ExplainStep`: a batch of graphs explained in one launch (csrc/explain.hip).

Reference of every comparison: `oracle.gcn_forward(..., edge_mask=)` under fp64 autograd on the CPU -- never the any-shape
GPU path, never the code under test.

Decidability.  The LeakyReLU derivative and the max-pool arg-max are discontinuous in the forward values (oracle/screen.py
explains why that matters); `screen.ambiguous_graphs` takes no edge mask, so `_flagged` below is its masked twin (same
margins: 2e-6 on the pre-activation of conv and readout hidden layers, relative 2e-6 on a positive max-pool gap), evaluated on
the fp64 masked oracle.  Masks are drawn from Generator(6); the masks of flagged graphs are re-drawn from the same generator
until no graph is flagged (at most 12 rounds, asserted): no graph is ever left out of a comparison.

Bounds (TOL = 1e-5, the project's): `dout = 1` mode PER GRAPH rel_inf of both mask gradients (the fp32 oracle's own per-graph
error against fp64 on these inputs is <= 1.3e-6); target mode WHOLE-TENSOR rel_inf of both gradients (fp32 oracle noise
<= 5.3e-7; per graph a prediction near its target leaves a cancelled residual, where the fp32 oracle itself shows 6.9e-6),
outputs with floor 1.0, per-graph loss relative with floor 1.0.  Every figure is printed before it is asserted (`pytest -s`).
"""
import functools

import pytest
import torch
import torch.nn.functional as Fn

from tests.helpers import golden_files, load_golden, rel_inf

pytestmark = pytest.mark.gpu
TOL = 1e-5
MASK_SEED, TARGET_SEED, PARAM_SEED = 6, 99, 23

CASES = {
    "small30": (dict(num_graphs=64, nodes=30, extra_bonds=3, max_degree=4, feat=64), dict(n_conv=2, n_read=2, n_classes=1)),
    "ragged": (dict(num_graphs=48, nodes=57, extra_bonds=4, max_degree=4, feat=25, nodes_jitter=9), dict(n_conv=2, n_read=2, n_classes=1)),
    "real-size": (dict(num_graphs=40, nodes=120, extra_bonds=4, max_degree=4, feat=25, nodes_jitter=64), dict(n_conv=2, n_read=2, n_classes=1)),
    "limit224": (dict(num_graphs=6, nodes=224, extra_bonds=12, max_degree=6, feat=64), dict(n_conv=2, n_read=2, n_classes=1)),
    "deep": (dict(num_graphs=24, nodes=80, extra_bonds=4, max_degree=4, feat=32, nodes_jitter=20), dict(n_conv=3, n_read=3, n_classes=2)),
    "one-conv": (dict(num_graphs=24, nodes=80, extra_bonds=4, max_degree=4, feat=32, nodes_jitter=20), dict(n_conv=1, n_read=1, n_classes=1)),
}
GOLDEN = [f"golden{i}" for i in range(len(golden_files()))]


@pytest.fixture(scope="module")
def H():
    import hcatgnet_amd
    import __graft_entry__
    import os
    from hcatgnet_amd import _lib
    if not os.path.isfile(_lib.LIB_PATH):
        __graft_entry__.build()
    return hcatgnet_amd


def _oracle_mod():
    from oracle import gcn_oracle
    return gcn_oracle


def _rand_params(F, D, n_conv=2, n_read=2, n_classes=1, seed=0):
    g = torch.Generator().manual_seed(seed)
    p = {}

    def glorot(o, i):
        a = (6.0 / (i + o)) ** 0.5
        return (torch.rand(o, i, generator=g) * 2 - 1) * a
    p["conv1.lin.weight"] = glorot(D, F); p["conv1.bias"] = torch.randn(D, generator=g) * 0.1
    for i in range(n_conv - 1):
        p[f"conv_layers.{i}.lin.weight"] = glorot(D, D); p[f"conv_layers.{i}.bias"] = torch.randn(D, generator=g) * 0.1
    dim = 2 * D
    for i in range(n_read - 1):
        p[f"readout.{i}.0.weight"] = glorot(dim // 2, dim); p[f"readout.{i}.0.bias"] = torch.randn(dim // 2, generator=g) * 0.1
        dim //= 2
    p[f"readout.{n_read - 1}.weight"] = glorot(n_classes, dim); p[f"readout.{n_read - 1}.bias"] = torch.randn(n_classes, generator=g) * 0.1
    return p


def _model_from_params(H, params):
    O = _oracle_mod()
    n_conv, n_read = O.infer_depths(params)
    D, F = params["conv1.lin.weight"].shape
    opt = H.default_options(n_convolutions=n_conv, readout_layers=n_read, embedding_dim=D,
                            n_classes=params[f"readout.{n_read - 1}.weight"].shape[0])
    m = H.make_network("GCN", opt, F)
    m.load_state_dict(params)
    return m.cuda()


# ------------------------------------------------------------------------------------------------ the fp64 reference
def _reference(params, x, ei, batch, B, em, nm, sig, target=None, dout=None, want_dx=False):
    """fp64 autograd through the masked oracle -> dict(out, loss, d_em, d_nm, dx, acts, emb)."""
    O = _oracle_mod()
    p = {k: v.double() for k, v in params.items()}
    s = torch.sigmoid if sig else (lambda t: t)
    bwd = target is not None or dout is not None
    em64 = em.double().clone().requires_grad_(bwd)
    nm64 = nm.double().clone().requires_grad_(bwd) if nm is not None else None
    x64 = x.double().clone().requires_grad_(bwd and want_dx)
    xin = x64 * s(nm64) if nm64 is not None else x64
    out, emb, acts = O.gcn_forward(p, xin, ei, batch, B, edge_mask=s(em64), return_intermediates=True)
    r = dict(out=out.detach(), acts=[a.detach() for a in acts], emb=emb.detach(), loss=None, d_em=None, d_nm=None, dx=None)
    if bwd:
        if target is not None:
            loss = ((out - target.double()) ** 2).mean(dim=1)
            r["loss"] = loss.detach()
            J = loss.sum()
        else:
            J = (dout.double() * out).sum()
        J.backward()
        r["d_em"], r["d_nm"], r["dx"] = em64.grad, (nm64.grad if nm64 is not None else None), (x64.grad if want_dx else None)
    return r


def _flagged(params, ref, batch, B, abs_kink=2e-6, rel_tie=2e-6):
    """The masked twin of oracle.screen.ambiguous_graphs on the fp64 reference's activations -> bool [B]."""
    O = _oracle_mod()
    p = {k: v.double() for k, v in params.items()}
    bad = torch.zeros(B, dtype=torch.bool)
    for a in ref["acts"]:
        pre = torch.where(a >= 0, a, a / O.LEAKY_SLOPE)
        bad[batch[(pre.abs() < abs_kink).any(dim=1)]] = True
    h = ref["acts"][-1]
    idx = batch.unsqueeze(1).expand_as(h)
    top = h.new_full((B, h.shape[1]), float("-inf")).scatter_reduce(0, idx, h, reduce="amax", include_self=True)
    below = torch.where(h < top[batch], h, torch.full_like(h, float("-inf")))
    second = h.new_full((B, h.shape[1]), float("-inf")).scatter_reduce(0, idx, below, reduce="amax", include_self=True)
    gap = top - second
    bad |= ((gap > 0) & (gap < rel_tie * top.abs().clamp_min(1e-3))).any(dim=1)
    z = ref["emb"]
    rn = O.readout_param_names(O.infer_depths(p)[1])
    for i, (wk, bk) in enumerate(rn):
        z = Fn.linear(z, p[wk], p[bk])
        if i < len(rn) - 1:
            bad |= (z.abs() < abs_kink).any(dim=1)
            z = Fn.leaky_relu(z, O.LEAKY_SLOPE)
    return bad


def _decidable_masks(params, x, ei, batch, B, sig, use_nm=True, max_rounds=12):
    """Masks from Generator(MASK_SEED) -- N(0, 1) under the sigmoid, U(0, 1) used as they are -- em [E] first, then nm [N, F];
    the masks of flagged graphs re-drawn (em on their edges, then nm on their nodes) until none is flagged."""
    gen = torch.Generator().manual_seed(MASK_SEED)
    draw = (lambda *s: torch.randn(*s, generator=gen)) if sig else (lambda *s: torch.rand(*s, generator=gen))
    E, (N, F) = ei.shape[1], x.shape
    em, nm = draw(E), draw(N, F)
    eg = batch[ei[1]]
    touched = torch.zeros(B, dtype=torch.bool)
    for rounds in range(max_rounds + 1):
        ref = _reference(params, x, ei, batch, B, em, nm if use_nm else None, sig)
        bad = _flagged(params, ref, batch, B)
        if not bool(bad.any()):
            print(f"    masks decidable after {rounds} rounds, {int(touched.sum())} of {B} graphs re-drawn")
            assert rounds <= max_rounds
            return em, (nm if use_nm else None)
        touched |= bad
        me, mn = bad[eg], bad[batch]
        em[me] = draw(int(me.sum()))
        nm[mn] = draw(int(mn.sum()), F)
    raise AssertionError(f"graphs still flagged after {max_rounds} rounds")


class _Case:
    pass


@functools.lru_cache(maxsize=None)
def _case(name, sig, use_nm=True):
    """-> params, graphs (CPU), targets, decidable masks of a named case."""
    from hcatgnet_amd import synth
    c = _Case()
    if name.startswith("golden"):
        g = load_golden(golden_files()[int(name[len("golden"):])])
        c.params, c.x, c.ei, c.batch, c.B = g["params"], g["x"], g["edge_index"], g["batch"], g["num_graphs"]
        c.target = g["ref_pred"].reshape(c.B, -1).float() + 1.0
        n = torch.bincount(c.batch, minlength=c.B)
        e = torch.bincount(c.batch[c.ei[1]], minlength=c.B)
        c.max_nodes, c.max_edges = int(n.max()), int(e.max())
    else:
        bk, mk = CASES[name]
        sb = synth.make_batch(**bk)
        c.params = _rand_params(bk["feat"], 64, seed=PARAM_SEED, **mk)
        c.x, c.ei, c.batch, c.B = sb.x, sb.edge_index, sb.batch, sb.num_graphs
        c.target = torch.randn(c.B, mk["n_classes"], generator=torch.Generator().manual_seed(TARGET_SEED))
        c.max_nodes, c.max_edges = sb.max_nodes, sb.max_edges
    print(f"\n  case {name} sigmoid={sig}: B {c.B} N {c.x.shape[0]} E {c.ei.shape[1]} max {c.max_nodes} / {c.max_edges}")
    c.em, c.nm = _decidable_masks(c.params, c.x, c.ei, c.batch, c.B, sig, use_nm)
    return c


def _gpu_batch(H, c):
    return H.Batch(c.x.cuda(), c.ei.cuda(), c.batch.cuda(), c.B, max_nodes=c.max_nodes, max_edges=c.max_edges,
                   edges_grouped=True)


def _per_graph(a, ref, owner, B):
    """max over the graphs of rel_inf restricted to each graph's entries"""
    a, ref = a.detach().double().cpu(), ref.detach().double().cpu()
    worst = 0.0
    for b in range(B):
        m = owner == b
        if bool(m.any()):
            worst = max(worst, rel_inf(a[m], ref[m]))
    return worst


def _check_modes(step, gb, c, sig, expect_path, tag, use_nm=True, want_dx=False):
    """dout = 1 (per-graph bound) and target mode (whole-tensor bound) of one case against the fp64 reference."""
    em_d = c.em.cuda()
    nm_d = c.nm.cuda() if use_nm else None
    eg = c.batch[c.ei[1]]
    ones = torch.ones(c.B, c.target.shape[1])
    # ---- dout = 1
    ref = _reference(c.params, c.x, c.ei, c.batch, c.B, c.em, c.nm if use_nm else None, sig, dout=ones, want_dx=want_dx)
    r = step(gb, em_d, nm_d, dout=ones.cuda(), want_dx=want_dx)
    assert step.last_path == expect_path
    fig = dict(out=rel_inf(r.out, ref["out"], floor=1.0), edge=_per_graph(r.d_edge_mask, ref["d_em"], eg, c.B))
    if use_nm:
        fig["node"] = _per_graph(r.d_node_mask, ref["d_nm"], c.batch, c.B)
    else:
        assert r.d_node_mask is None
    if want_dx:
        fig["dx"] = _per_graph(r.dx, ref["dx"], c.batch, c.B)
    else:
        assert r.dx is None
    print(f"    {tag} dout=1 (per graph): " + "  ".join(f"{k} {v:.2e}" for k, v in fig.items()))
    assert r.loss is None
    assert all(v <= TOL for v in fig.values()), fig
    # ---- target
    ref = _reference(c.params, c.x, c.ei, c.batch, c.B, c.em, c.nm if use_nm else None, sig, target=c.target, want_dx=want_dx)
    r = step(gb, em_d, nm_d, target=c.target.cuda(), want_dx=want_dx)
    assert step.last_path == expect_path
    fig = dict(out=rel_inf(r.out, ref["out"], floor=1.0), edge=rel_inf(r.d_edge_mask, ref["d_em"]))
    if use_nm:
        fig["node"] = rel_inf(r.d_node_mask, ref["d_nm"])
    if want_dx:
        fig["dx"] = rel_inf(r.dx, ref["dx"])
    fig["loss"] = float(((r.loss.double().cpu() - ref["loss"]).abs() / ref["loss"].abs().clamp_min(1.0)).max())
    print(f"    {tag} target (whole tensor): " + "  ".join(f"{k} {v:.2e}" for k, v in fig.items()))
    assert all(v <= TOL for v in fig.values()), fig
    assert tuple(r.out.shape) == tuple(c.target.shape) and tuple(r.loss.shape) == (c.B,)
    assert tuple(r.d_edge_mask.shape) == (c.ei.shape[1],)


# ------------------------------------------------------------------------------------------------ 1. parity
@pytest.mark.parametrize("apply_sigmoid", [True, False])
@pytest.mark.parametrize("name", GOLDEN + list(CASES))
def test_parity_with_the_fp64_masked_oracle(H, name, apply_sigmoid):
    """Every case, both mask forms, on the one-launch kernel."""
    from hcatgnet_amd.explain import ExplainStep
    c = _case(name, apply_sigmoid)
    step = ExplainStep(_model_from_params(H, c.params), apply_sigmoid=apply_sigmoid)
    gb = _gpu_batch(H, c)
    assert step.reason(gb) is None
    _check_modes(step, gb, c, apply_sigmoid, "fused", name)


# ------------------------------------------------------------------------------------------------ 2. no node mask, dx
@pytest.mark.parametrize("name", ["small30", "deep"])
def test_without_a_node_mask_dx_is_the_input_gradient(H, name):
    from hcatgnet_amd.explain import ExplainStep
    c = _case(name, True, False)
    step = ExplainStep(_model_from_params(H, c.params))
    _check_modes(step, _gpu_batch(H, c), c, True, "fused", name + " (no node mask, dx)", use_nm=False, want_dx=True)


def test_dx_together_with_a_node_mask(H):
    from hcatgnet_amd.explain import ExplainStep
    c = _case("ragged", True)
    step = ExplainStep(_model_from_params(H, c.params))
    _check_modes(step, _gpu_batch(H, c), c, True, "fused", "ragged (node mask and dx)", want_dx=True)


# ------------------------------------------------------------------------------------------------ 3. exact ties
def _rowwise_linear(x, w, b=None):
    """`F.linear` with every output row computed by the same instruction sequence wherever the row sits in the matrix:
    elementwise products and one sum per (row, output).  Bit-identical input rows give bit-identical output rows."""
    y = (x.unsqueeze(1) * w.unsqueeze(0)).sum(-1)
    return y if b is None else y + b


def _screen_report(params, ref, batch, B):
    """What `_flagged` saw, criterion by criterion (printed when a hand-built case is flagged)."""
    O = _oracle_mod()
    for li, a in enumerate(ref["acts"]):
        pre = torch.where(a >= 0, a, a / O.LEAKY_SLOPE)
        print(f"    conv {li} kink hits (graph, value):", [(int(batch[r]), float(pre[r, c])) for r, c in (pre.abs() < 2e-6).nonzero().tolist()][:8])
    h = ref["acts"][-1]; idx = batch.unsqueeze(1).expand_as(h)
    top = h.new_full((B, h.shape[1]), float("-inf")).scatter_reduce(0, idx, h, reduce="amax", include_self=True)
    below = torch.where(h < top[batch], h, torch.full_like(h, float("-inf")))
    second = h.new_full((B, h.shape[1]), float("-inf")).scatter_reduce(0, idx, below, reduce="amax", include_self=True)
    gap = top - second
    m = (gap > 0) & (gap < 2e-6 * top.abs().clamp_min(1e-3))
    print("    max-pool near-ties (graph, feature, gap, max):", [(g, f, float(gap[g, f]), float(top[g, f])) for g, f in m.nonzero().tolist()][:8])


def test_exact_max_pool_ties_split_evenly(H, monkeypatch):
    """A centre with k = 2..4 leaves that share one feature row (plus a 3-atom tail): the leaves' activations are bit-identical,
    the max-pool gradient is split evenly among them (torch amax semantics) on both sides.

    The reference is `oracle.gcn_forward` under fp64 autograd like everywhere; for THIS test its dense products run through
    `_rowwise_linear`.  A BLAS gemm may round the same input row differently depending on where the row sits in the matrix
    (edge tiles of its blocking): on such a host two of three sibling leaves tie exactly and the third sits one ulp (1e-17)
    away, the fp64 reference then hands the whole max-pool gradient to fewer leaves than the inputs define, and the screen
    rightly flags the graph (0 < gap < 2e-6).  The hand-built ties are exact by construction, so the reference has to keep
    them exact whatever the host's BLAS does; the forward of the two evaluations is asserted to agree to 1e-12."""
    from hcatgnet_amd.explain import ExplainStep
    from types import SimpleNamespace
    O = _oracle_mod()
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
    c = _Case()
    c.x, c.ei, c.batch, c.B = torch.cat(xs), torch.cat(eis, 1), torch.cat(bs), B
    c.params = _rand_params(25, 64, seed=PARAM_SEED)
    c.em, c.nm = torch.full((c.ei.shape[1],), 0.3), torch.zeros(c.x.shape[0], 25)
    c.target = torch.zeros(B, 1)
    c.max_nodes, c.max_edges = 8, 14
    stock = _reference(c.params, c.x, c.ei, c.batch, B, c.em, c.nm, True, target=c.target)
    with monkeypatch.context() as mp:
        mp.setattr(O, "F", SimpleNamespace(linear=_rowwise_linear, leaky_relu=Fn.leaky_relu, mse_loss=Fn.mse_loss))
        ref = _reference(c.params, c.x, c.ei, c.batch, B, c.em, c.nm, True, target=c.target)
    drift = max(float((a - b).abs().max()) for a, b in zip(ref["acts"] + [ref["out"]], stock["acts"] + [stock["out"]]))
    print(f"\n  row-wise vs BLAS fp64 forward: max abs difference {drift:.1e}; "
          f"BLAS reference flags graphs {_flagged(c.params, stock, c.batch, B).nonzero().flatten().tolist()}")
    assert drift <= 1e-12
    h = ref["acts"][-1]; idx = c.batch.unsqueeze(1).expand_as(h)
    top = h.new_full((B, 64), float("-inf")).scatter_reduce(0, idx, h, reduce="amax", include_self=True)
    per = torch.zeros(B, 64, dtype=torch.long).scatter_add(0, idx, (h == top[c.batch]).long())
    print(f"  exact ties: {int((per > 1).sum())} of {B * 64} (graph, feature) maxima tied")
    assert int((per > 1).sum()) > 100
    nptr = torch.zeros(B + 1, dtype=torch.long); nptr[1:] = torch.bincount(c.batch, minlength=B).cumsum(0)
    for g in range(B):                                   # the sibling leaves stay bit-identical through every layer
        for a in ref["acts"]:
            for j in range(2, 2 + (2 + g % 3) - 1):
                assert torch.equal(a[nptr[g] + 1], a[nptr[g] + j]), (g, j)
    bad = _flagged(c.params, ref, c.batch, B)
    if bool(bad.any()):
        _screen_report(c.params, ref, c.batch, B)
    assert not bool(bad.any()), bad
    step = ExplainStep(_model_from_params(H, c.params))
    r = step(_gpu_batch(H, c), c.em.cuda(), c.nm.cuda(), target=c.target.cuda())
    assert step.last_path == "fused"
    fig = dict(out=rel_inf(r.out, ref["out"], floor=1.0), edge=rel_inf(r.d_edge_mask, ref["d_em"]), node=rel_inf(r.d_node_mask, ref["d_nm"]))
    print("    ties, target (whole tensor): " + "  ".join(f"{k} {v:.2e}" for k, v in fig.items()))
    assert all(v <= TOL for v in fig.values()), fig


# ------------------------------------------------------------------------------------------------ 4. explicit self loop
def test_explicit_self_loop_edge_gets_exactly_zero(H):
    from hcatgnet_amd import synth
    from hcatgnet_amd.explain import ExplainStep
    sb = synth.make_batch(num_graphs=5, nodes=20, extra_bonds=2, max_degree=4, feat=25, nodes_jitter=4)
    eg = sb.batch[sb.edge_index[1]]
    pos = int((eg <= 1).sum()) - 3                              # inside graph 1's edge block
    node = int(sb.edge_index[0, pos])
    ei = torch.cat([sb.edge_index[:, :pos], torch.tensor([[node], [node]]), sb.edge_index[:, pos:]], 1).contiguous()
    c = _Case()
    c.x, c.ei, c.batch, c.B = sb.x, ei, sb.batch, sb.num_graphs
    c.params = _rand_params(25, 64, seed=PARAM_SEED)
    c.target = torch.randn(c.B, 1, generator=torch.Generator().manual_seed(TARGET_SEED))
    c.max_nodes, c.max_edges = sb.max_nodes, sb.max_edges + 1
    c.em, c.nm = _decidable_masks(c.params, c.x, c.ei, c.batch, c.B, True)
    step = ExplainStep(_model_from_params(H, c.params))
    gb = _gpu_batch(H, c)
    _check_modes(step, gb, c, True, "fused", "self loop")
    r = step(gb, c.em.cuda(), c.nm.cuda(), target=c.target.cuda())
    assert float(r.d_edge_mask[pos]) == 0.0
    assert int((r.d_edge_mask != 0).sum()) == c.ei.shape[1] - 1


# ------------------------------------------------------------------------------------------------ 5. bitwise
def test_batched_equals_one_by_one_bitwise(H):
    """A graph's results do not depend on what shares its batch, nor on the run: no float atomics, fixed orders."""
    from hcatgnet_amd.explain import ExplainStep
    c = _case("real-size", True)
    model = _model_from_params(H, c.params)
    step = ExplainStep(model)
    gb = _gpu_batch(H, c)
    em_d, nm_d, t_d = c.em.cuda(), c.nm.cuda(), c.target.cuda()
    full = [t.clone() for t in step(gb, em_d, nm_d, target=t_d, want_dx=True)]
    again = [t.clone() for t in step(gb, em_d, nm_d, target=t_d, want_dx=True)]
    for a, b in zip(full, again):
        assert torch.equal(a, b)
    nptr = torch.zeros(c.B + 1, dtype=torch.long); nptr[1:] = torch.bincount(c.batch, minlength=c.B).cumsum(0)
    eptr = torch.zeros(c.B + 1, dtype=torch.long); eptr[1:] = torch.bincount(c.batch[c.ei[1]], minlength=c.B).cumsum(0)
    single = ExplainStep(model)
    for g in range(c.B):
        a, b, ea, eb = int(nptr[g]), int(nptr[g + 1]), int(eptr[g]), int(eptr[g + 1])
        one = H.Batch(c.x[a:b].cuda(), (c.ei[:, ea:eb] - a).contiguous().cuda(), torch.zeros(b - a, dtype=torch.long).cuda(), 1,
                      max_nodes=b - a, max_edges=eb - ea, edges_grouped=True)
        r = single(one, em_d[ea:eb].contiguous(), nm_d[a:b].contiguous(), target=t_d[g:g + 1].contiguous(), want_dx=True)
        assert single.last_path == "fused"
        assert torch.equal(r.out, full[0][g:g + 1]) and torch.equal(r.loss, full[1][g:g + 1]), g
        assert torch.equal(r.d_edge_mask, full[2][ea:eb]), g
        assert torch.equal(r.d_node_mask, full[3][a:b]) and torch.equal(r.dx, full[4][a:b]), g


# ------------------------------------------------------------------------------------------------ 6. nothing else moves
def test_weights_grads_and_masks_are_left_alone(H):
    from hcatgnet_amd.explain import ExplainStep
    from hcatgnet_amd.gcn import GCNConv
    c = _case("ragged", True)
    model = _model_from_params(H, c.params)
    before = [q.detach().clone() for q in model.parameters()]
    step = ExplainStep(model)
    gb = _gpu_batch(H, c)
    step(gb, c.em.cuda(), c.nm.cuda(), target=c.target.cuda(), want_dx=True)
    step(gb, c.em.cuda(), c.nm.cuda(), dout=torch.ones(c.B, 1).cuda())
    assert step.last_path == "fused"
    for q, b in zip(model.parameters(), before):
        assert torch.equal(q.detach(), b) and q.grad is None
    for mod in model.modules():
        if isinstance(mod, GCNConv):
            assert mod.explain is False and mod._edge_mask is None


# ------------------------------------------------------------------------------------------------ 7. fallback
def test_other_shapes_take_the_autograd_path_with_the_same_bounds(H):
    from hcatgnet_amd import synth
    from hcatgnet_amd.explain import ExplainStep
    from hcatgnet_amd.gcn import GCNConv
    O = _oracle_mod()
    todo = [("D = 128", dict(num_graphs=8, nodes=57, extra_bonds=4, max_degree=4, feat=25, nodes_jitter=9), 128),
            ("225 nodes", dict(num_graphs=2, nodes=225, extra_bonds=4, max_degree=4, feat=25), 64)]
    for tag, bk, D in todo:
        sb = synth.make_batch(**bk)
        c = _Case()
        c.x, c.ei, c.batch, c.B = sb.x, sb.edge_index, sb.batch, sb.num_graphs
        c.params = _rand_params(25, D, seed=PARAM_SEED)
        c.target = torch.randn(c.B, 1, generator=torch.Generator().manual_seed(TARGET_SEED))
        c.max_nodes, c.max_edges = sb.max_nodes, sb.max_edges
        print(f"\n  fallback {tag}")
        c.em, c.nm = _decidable_masks(c.params, c.x, c.ei, c.batch, c.B, True)
        model = _model_from_params(H, c.params)
        step = ExplainStep(model)
        gb = _gpu_batch(H, c)
        assert "shape" in step.reason(gb)
        _check_modes(step, gb, c, True, "autograd", tag, want_dx=True)
        assert all(q.grad is None for q in model.parameters())
        for mod in model.modules():
            if isinstance(mod, GCNConv):
                assert mod.explain is False and mod._edge_mask is None
        with torch.no_grad():
            plain = model(gb)
        o_plain, _ = O.gcn_forward({k: v.double() for k, v in c.params.items()}, c.x.double(), c.ei, c.batch, c.B)
        assert rel_inf(plain, o_plain, floor=1.0) <= TOL


# ------------------------------------------------------------------------------------------------ 8. capture
def test_captured_call_replays_with_new_mask_values(H):
    from hcatgnet_amd.explain import ExplainStep
    c = _case("ragged", True)
    model = _model_from_params(H, c.params)
    step = ExplainStep(model)
    gb = _gpu_batch(H, c)
    em_d, nm_d, t_d = c.em.cuda(), c.nm.cuda(), c.target.cuda()
    step(gb, em_d, nm_d, target=t_d, want_dx=True)                  # plan, buffers, LDS attribute: before the capture
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        held = step(gb, em_d, nm_d, target=t_d, want_dx=True)
    assert step.last_path == "fused"
    eager = ExplainStep(model)
    gen = torch.Generator().manual_seed(77)
    for _ in range(2):
        em_d.copy_(torch.randn(em_d.shape, generator=gen)); nm_d.copy_(torch.randn(nm_d.shape, generator=gen))
        graph.replay()
        torch.cuda.synchronize()
        got = [t.clone() for t in held]
        want = eager(gb, em_d, nm_d, target=t_d, want_dx=True)
        for a, b in zip(got, want):
            assert torch.equal(a, b)


# ------------------------------------------------------------------------------------------------ 9. forward only
def test_forward_only_call(H):
    from hcatgnet_amd.explain import ExplainStep
    c = _case("deep", True)
    step = ExplainStep(_model_from_params(H, c.params))
    r = step(_gpu_batch(H, c), c.em.cuda(), c.nm.cuda())
    assert step.last_path == "fused"
    ref = _reference(c.params, c.x, c.ei, c.batch, c.B, c.em, c.nm, True)
    v = rel_inf(r.out, ref["out"], floor=1.0)
    print(f"\n    forward only: out {v:.2e}")
    assert v <= TOL
    assert r.loss is None and r.d_edge_mask is None and r.d_node_mask is None and r.dx is None
    with pytest.raises(ValueError):
        step(_gpu_batch(H, c), c.em.cuda(), c.nm.cuda(), target=c.target.cuda(), dout=c.target.cuda())
