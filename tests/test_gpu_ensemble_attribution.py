"""GPU tests of `hcatgnet_amd.attribution.EnsembleAttribution`: integrated gradients of M models for a batch of graphs, one
workgroup per (graph, model) of one launch (csrc/explain.hip, k_explain_graphs<false, true> with a model axis), and the mean
and standard deviation over the models (k_model_moments).  tests/ensemble_attr_ref.py states the models, the yardstick of the
per-model values (bitwise `IntegratedGradients(models[m])`) and the bound of the moments.  Every figure is printed before it
is asserted (`pytest -s`)."""
import os

import pytest
import torch

from tests import ensemble_attr_ref as ER
from tests import integrated_ref as R
from tests.test_gpu_explain import PARAM_SEED, _rand_params

pytestmark = pytest.mark.gpu
SHAPE_LIMIT = 16          # HCG_STATUS_SHAPE_LIMIT
FIELDS = ("node_mean", "node_std", "edge_mean", "edge_std", "out_full", "out_base", "node_attr", "edge_attr")


@pytest.fixture(scope="module")
def H():
    import hcatgnet_amd
    from hcatgnet_amd import _lib
    if not os.path.isfile(_lib.LIB_PATH):
        import __graft_entry__
        __graft_entry__.build()
    return hcatgnet_amd


def _keep(r):
    return [None if t is None else t.clone() for t in r]


def _same(a, b):
    return all((p is None and q is None) or torch.equal(p, q) for p, q in zip(a, b))


def _singles(H, models, batch, cls, **kw):
    """[IntegratedGradients(models[m])(batch)] cloned: the yardstick of the per-model values"""
    out = []
    for m in models:
        ig = H.IntegratedGradients(m, **kw)
        out.append([t.clone() for t in ig(batch, class_index=cls)])
        assert ig.last_path == "fused"
    return out


def _assert_per_model(r, singles, tag):
    for m, one in enumerate(singles):
        for k, (got, want) in enumerate(zip((r.node_attr[m], r.edge_attr[m], r.out_full[m], r.out_base[m]), one)):
            assert torch.equal(got, want), (tag, m, ("node_attr", "edge_attr", "out_full", "out_base")[k])


# ------------------------------------------------------------------------------------------------ 1. per-model identity
@pytest.mark.parametrize("name,counts", [("small30", (1, 3, 5)), ("ragged", (1, 3, 5)), ("deep", (1, 3, 5)), ("limit224", (2,))])
def test_every_model_is_bitwise_its_own_integrated_gradients(H, name, counts):
    c = R.case(name)
    gb = R.batch(H, c, "cuda")
    models = ER.models(H, name, max(counts), "cuda")
    modes = (dict(n_steps=c.n_steps), dict(method="gradient"), dict(method="gradient", saliency=True))
    for kw in modes:
        singles = _singles(H, models, gb, c.cls, **kw)
        for M in counts:
            ea = H.EnsembleAttribution(models[:M], **kw)
            assert ea.reason(gb) is None
            r = ea(gb, class_index=c.cls, per_model=True)
            assert ea.last_path == "fused" and ea.n_steps == (1 if "method" in kw else c.n_steps)
            assert tuple(r.node_attr.shape) == (M,) + tuple(c.x.shape) and tuple(r.edge_attr.shape) == (M, c.ei.shape[1])
            assert tuple(r.out_full.shape) == tuple(r.out_base.shape) == (M, c.B, singles[0][2].shape[1])
            _assert_per_model(r, singles[:M], (name, M, kw))
            if kw.get("saliency"):
                assert float(r.node_attr.min()) >= 0.0 and float(r.edge_attr.min()) >= 0.0 and float(r.node_mean.min()) >= 0.0
    # the models differ: the yardstick is not one array compared with itself
    assert len(models) == 1 or not torch.equal(singles[0][0], singles[1][0])


# ------------------------------------------------------------------------------------------------ 2. splits
def test_both_splits_are_exact(H):
    c = R.case("small30")
    assert c.n_steps == 6
    gb = R.batch(H, c, "cuda")
    ea = H.EnsembleAttribution(ER.models(H, "small30", 5, "cuda"), n_steps=6)
    one = _keep(ea(gb, per_model=True, models_per_launch=5, steps_per_launch=6))
    assert ea.last_path == "fused" and len(one) == len(FIELDS)
    assert _same(one, _keep(ea(gb, per_model=True)))                  # (the default: one launch here)
    pairs = [(mpl, spl) for mpl in (1, 2, 5) for spl in (1, 4, 6)]
    for mpl, spl in pairs:
        got = _keep(ea(gb, per_model=True, models_per_launch=mpl, steps_per_launch=spl))
        for k, name in enumerate(FIELDS):
            assert torch.equal(got[k], one[k]), (mpl, spl, name)
    # ... whatever the buffers hold: step 0 and model 0 start from 0
    for mpl, spl in pairs:
        for t in ea._bufs.values():
            if t.dtype == torch.float32:
                t.fill_(float("nan"))
        got = _keep(ea(gb, per_model=True, models_per_launch=mpl, steps_per_launch=spl))
        for k, name in enumerate(FIELDS):
            assert torch.equal(got[k], one[k]), ("after NaN", mpl, spl, name)
    # per_model=False: one chunk's rows are reused by every chunk; the moments and outputs do not change
    lean = H.EnsembleAttribution(ea.models, n_steps=6)
    for mpl in (1, 2, 5):
        got = _keep(lean(gb, models_per_launch=mpl, steps_per_launch=4))
        assert got[6] is None and got[7] is None and _same(got[:6], one[:6]), mpl
    assert lean._bufs["node"].numel() == 5 * c.x.numel()              # (the largest chunk seen, never the whole ensemble twice)
    small = H.EnsembleAttribution(ea.models, n_steps=6)
    small(gb, models_per_launch=2)
    assert small._bufs["node"].numel() == 2 * c.x.numel() and small._bufs["edge"].numel() == 2 * c.ei.shape[1]


# ------------------------------------------------------------------------------------------------ 3. degenerate ensembles
def test_one_model_and_copies_of_one_model(H):
    c = R.case("ragged")
    gb = R.batch(H, c, "cuda")
    model = ER.models(H, "ragged", 1, "cuda")[0]
    single = _singles(H, [model], gb, c.cls, n_steps=c.n_steps)[0]
    for M in (1, 3):
        ea = H.EnsembleAttribution([model] * M, n_steps=c.n_steps)
        for mpl in (None, 1):
            r = ea(gb, class_index=c.cls, per_model=True, models_per_launch=mpl)
            assert ea.last_path == "fused"
            assert torch.equal(r.node_mean, single[0]) and torch.equal(r.edge_mean, single[1]), (M, mpl)
            assert float(r.node_std.abs().max()) == 0.0 and float(r.edge_std.abs().max()) == 0.0, (M, mpl)
            for m in range(M):
                assert torch.equal(r.node_attr[m], single[0]) and torch.equal(r.out_full[m], single[2])
    assert int((single[0] != 0).sum()) > 0


# ------------------------------------------------------------------------------------------------ 4. the moments
@pytest.mark.parametrize("name", ["ragged", "real-size"])
@pytest.mark.parametrize("M", [5, 9])
def test_moments_against_float64(H, name, M):
    c = R.case(name)
    gb = R.batch(H, c, "cuda")
    ea = H.EnsembleAttribution(ER.models(H, name, M, "cuda"), n_steps=c.n_steps)
    r = ea(gb, class_index=c.cls, per_model=True)
    assert ea.last_path == "fused"
    print()
    ER.check_moments(r.node_attr, r.edge_attr, r, f"{name}")
    assert float(r.node_std.max()) > 0.0 and float(r.edge_std.max()) > 0.0
    # the lean call and a split over the models give the same moments, bitwise
    keep = _keep(r)
    q = ea(gb, class_index=c.cls, models_per_launch=2)
    assert q.node_attr is None and _same(_keep(q)[:6], keep[:6])


def test_entries_that_are_zero_in_every_model_have_moments_exactly_zero(H):
    """The construction of tests/test_gpu_integrated.py::test_self_loop_edge_and_zero_features_get_exactly_zero: an explicit
    (i, i) edge and 40 % of the entries of x equal to 0."""
    from hcatgnet_amd import synth
    sb = synth.make_batch(num_graphs=5, nodes=20, extra_bonds=2, max_degree=4, feat=25, nodes_jitter=4)
    eg = sb.batch[sb.edge_index[1]]
    pos = int((eg <= 1).sum()) - 3                              # inside graph 1's edge block
    node = int(sb.edge_index[0, pos])
    ei = torch.cat([sb.edge_index[:, :pos], torch.tensor([[node], [node]]), sb.edge_index[:, pos:]], 1).contiguous()
    x = sb.x.clone()
    zero = torch.rand(x.shape, generator=torch.Generator().manual_seed(3)) < 0.4
    x[zero] = 0.0
    M = 5
    plist = [_rand_params(25, 64, seed=PARAM_SEED + k) for k in range(M)]
    c = R.custom(plist[0], x, ei, sb.batch, sb.num_graphs, 4, screen=False)
    models = []
    for p in plist:
        proxy = R.Case()
        proxy.params = p
        models.append(R.model(H, proxy, "cuda"))
    ea = H.EnsembleAttribution(models, n_steps=4)
    r = ea(R.batch(H, c, "cuda"), per_model=True)
    assert ea.last_path == "fused"
    z = zero.cuda()
    assert int(zero.sum()) > 100
    assert float(r.node_attr[:, z].abs().max()) == 0.0 and float(r.edge_attr[:, pos].abs().max()) == 0.0
    assert float(r.node_mean[z].abs().max()) == 0.0 and float(r.node_std[z].abs().max()) == 0.0
    assert float(r.edge_mean[pos]) == 0.0 and float(r.edge_std[pos]) == 0.0
    assert int((r.edge_std != 0).sum()) == ei.shape[1] - 1 and int((r.node_std[~z] != 0).sum()) > 0.9 * int((~zero).sum())
    print()
    fn, fe = ER.check_moments(r.node_attr, r.edge_attr, r, "zero features and a self-loop edge")
    assert fn["zeros"] >= int(zero.sum()) and fe["zeros"] == 1


# ------------------------------------------------------------------------------------------------ 5. refusal
def test_a_graph_over_the_limit_is_refused_for_every_model_and_the_rest_untouched(H):
    c = R.case("ragged")
    M = 3
    ea = H.EnsembleAttribution(ER.models(H, "ragged", M, "cuda"), n_steps=c.n_steps)
    honest = [t.cpu() for t in _keep(ea(R.batch(H, c, "cuda"), per_model=True))]
    sizes = torch.bincount(c.batch, minlength=c.B)
    big = sizes == sizes.max()
    assert 0 < int(big.sum()) < c.B
    gb = R.batch(H, c, "cuda", max_nodes=int(sizes.max()) - 1)
    for t in ea._bufs.values():
        if t.dtype == torch.float32:
            t.fill_(7.0)
    got = [t.cpu() for t in ea(gb, per_model=True, models_per_launch=2, steps_per_launch=3)]      # (every launch refuses it again)
    assert ea.last_path == "fused"
    torch.cuda.synchronize()
    status = gb._hcg_plan.status
    word = int(status[0].item())
    status.zero_()                                                    # (shared per device: leave it clean for the next test)
    assert word & SHAPE_LIMIT
    nb, eb = big[c.batch], big[c.edge_owner]
    masks = dict(node_mean=nb, node_std=nb, edge_mean=eb, edge_std=eb)
    for k, name in enumerate(FIELDS):
        g, h = got[k], honest[k]
        if name in masks:
            m = masks[name]
            assert float(g[m].abs().max()) == 0.0 and torch.equal(g[~m], h[~m]), name
        elif name in ("out_full", "out_base"):
            assert float(g[:, big].abs().max()) == 0.0 and torch.equal(g[:, ~big], h[:, ~big]), name
        else:
            m = nb if name == "node_attr" else eb
            assert float(g[:, m].abs().max()) == 0.0 and torch.equal(g[:, ~m], h[:, ~m]), name
    assert float(honest[0][nb].abs().max()) > 0.0 and float(honest[4][:, big].abs().max()) > 0.0


# ------------------------------------------------------------------------------------------------ 6. the loop path
def _assert_loop(H, ea, models, gb, c, tag):
    r = ea(gb, class_index=c.cls, per_model=True)
    assert ea.last_path == "loop", tag
    for m, model in enumerate(models):
        one = H.IntegratedGradients(model, n_steps=c.n_steps).loop(gb, c.cls)
        assert torch.equal(r.node_attr[m], one.node_attr) and torch.equal(r.edge_attr[m], one.edge_attr), (tag, m)
        assert torch.equal(r.out_full[m], one.out_full) and torch.equal(r.out_base[m], one.out_base), (tag, m)
    ER.check_moments(r.node_attr, r.edge_attr, r, tag)
    for model in models:
        assert all(q.grad is None for q in model.parameters())


def test_the_loop_path(H):
    c = R.case("ragged")
    gb = R.batch(H, c, "cuda")
    print()
    models = ER.models(H, "ragged", 2, "cuda") + ER.models(H, "ragged", 1, "cuda", use_fused=False)
    ea = H.EnsembleAttribution(models, n_steps=c.n_steps)
    assert "disabled" in ea.reason(gb)
    _assert_loop(H, ea, models, gb, c, "ragged, use_fused off on one model (loop)")
    w = R.case("ragged-d128")
    wide = ER.models(H, "ragged-d128", 3, "cuda")
    ea = H.EnsembleAttribution(wide, n_steps=w.n_steps)
    wb = R.batch(H, w, "cuda")
    assert "shape" in ea.reason(wb)
    _assert_loop(H, ea, wide, wb, w, "ragged, embedding_dim 128 (loop)")
    cpu = ER.models(H, "ragged", 3)
    ea = H.EnsembleAttribution(cpu, n_steps=c.n_steps)
    cb = R.batch(H, c)
    assert ea.reason(cb) == "the batch is on the CPU"
    _assert_loop(H, ea, cpu, cb, c, "ragged, CPU tensors (loop)")


# ------------------------------------------------------------------------------------------------ 7. nothing else moves
def test_weights_grads_masks_and_memory_are_left_alone_and_refresh_takes_new_weights(H):
    from hcatgnet_amd.gcn import GCNConv
    c = R.case("deep")
    M = 3
    models = ER.models(H, "deep", M, "cuda")
    before = [[q.detach().clone() for q in m.parameters()] for m in models]
    ea = H.EnsembleAttribution(models, n_steps=c.n_steps)
    gb = R.batch(H, c, "cuda")
    first = _keep(ea(gb, class_index=c.cls, per_model=True))
    ea(gb, class_index=0, per_model=True, models_per_launch=2, steps_per_launch=2)
    torch.cuda.synchronize()
    held = torch.cuda.memory_allocated()
    r = ea(gb, class_index=c.cls, per_model=True)
    r2 = ea(gb, class_index=c.cls, per_model=True, models_per_launch=1, steps_per_launch=1)
    torch.cuda.synchronize()
    after = torch.cuda.memory_allocated()
    print(f"\n    bytes allocated before / after two warm calls: {held} / {after}")
    assert after == held and ea.last_path == "fused"
    assert r.node_mean.data_ptr() == r2.node_mean.data_ptr() and _same(first, _keep(r2))
    for m, ws in zip(models, before):
        for q, b in zip(m.parameters(), ws):
            assert torch.equal(q.detach(), b) and q.grad is None
        for mod in m.modules():
            if isinstance(mod, GCNConv):
                assert mod.explain is False and mod._edge_mask is None
    # a snapshot: a model's new weights do not show until refresh()
    with torch.no_grad():
        models[1].conv1.lin.weight.mul_(1.5)
        models[1].readout[-1].bias.add_(0.25)
    assert _same(first, _keep(ea(gb, class_index=c.cls, per_model=True)))
    ea.refresh()
    fresh = _keep(H.EnsembleAttribution(models, n_steps=c.n_steps)(gb, class_index=c.cls, per_model=True))
    now = _keep(ea(gb, class_index=c.cls, per_model=True))
    assert _same(now, fresh) and not torch.equal(now[6][1], first[6][1]) and torch.equal(now[6][0], first[6][0])
    assert not torch.equal(now[0], first[0])
