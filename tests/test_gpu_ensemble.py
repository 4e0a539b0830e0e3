"""GPU tests of `hcatgnet_amd.ensemble.EnsemblePredict`: M models predict one batch of graphs in one launch (csrc/ensemble.hip).

Reference of every comparison: `oracle.gcn_forward` in fp64 on the CPU, run once per model -- never the any-shape GPU path,
never the code under test.  Bounds (TOL = 1e-5, the project's): per model rel_inf of the pooled embedding, rel_inf of the
outputs with floor 1.0; on the golden files the model built from the reference's own weights also meets the reference's
stored embeddings (rel_inf <= TOL) and predictions (abs <= 5e-5), as tests/test_gpu_parity.py asks of the single model.  The
path is forward only -- no LeakyReLU-derivative or arg-max discontinuity enters a value -- so no graph and no model is left
out of any comparison.  Every figure is printed before it is asserted (`pytest -s`).
"""
import pytest
import torch

from tests.helpers import golden_files, load_golden, rel_inf
from tests.test_gpu_explain import CASES, _Case, _gpu_batch, _model_from_params, _rand_params

pytestmark = pytest.mark.gpu
TOL = 1e-5
PARAM_SEED = 23
M_SYNTH, M_GOLDEN = 7, 5
GOLDEN = [f"golden{i}" for i in range(len(golden_files()))]
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


def _oracle_mod():
    from oracle import gcn_oracle
    return gcn_oracle


def _synth_case(name, M=M_SYNTH, D=64, bk=None, mk=None):
    """-> the graphs of a named shape (CPU) and M seeded weight sets."""
    from hcatgnet_amd import synth
    bk0, mk0 = CASES[name] if name in CASES else (None, None)
    bk, mk = bk or bk0, mk or mk0
    sb = synth.make_batch(**bk)
    c = _Case()
    c.x, c.ei, c.batch, c.B = sb.x, sb.edge_index, sb.batch, sb.num_graphs
    c.max_nodes, c.max_edges = sb.max_nodes, sb.max_edges
    c.params = [_rand_params(bk["feat"], D, seed=PARAM_SEED + k, **mk) for k in range(M)]
    return c


def _golden_case(i, M=M_GOLDEN):
    """Golden file i: model 0 = the reference's own weights, models 1 .. M-1 seeded weights of the same architecture."""
    O = _oracle_mod()
    g = load_golden(golden_files()[i])
    c = _Case()
    c.x, c.ei, c.batch, c.B = g["x"], g["edge_index"], g["batch"], g["num_graphs"]
    n = torch.bincount(c.batch, minlength=c.B)
    e = torch.bincount(c.batch[c.ei[1]], minlength=c.B)
    c.max_nodes, c.max_edges = int(n.max()), int(e.max())
    n_conv, n_read = O.infer_depths(g["params"])
    D, F = g["params"]["conv1.lin.weight"].shape
    C = g["params"][f"readout.{n_read - 1}.weight"].shape[0]
    c.params = [g["params"]] + [_rand_params(F, D, n_conv=n_conv, n_read=n_read, n_classes=C, seed=PARAM_SEED + k)
                                for k in range(1, M)]
    c.ref_emb, c.ref_pred = g["ref_emb"], g["ref_pred"]
    return c


def _oracle(c, params=None):
    """fp64 CPU oracle, one run per model -> out [M, B, C], emb [M, B, 2D]."""
    O = _oracle_mod()
    outs, embs = [], []
    for p in (params or c.params):
        out, emb = O.gcn_forward({k: v.double() for k, v in p.items()}, c.x.double(), c.ei, c.batch, c.B)
        outs.append(out.reshape(c.B, -1)); embs.append(emb)
    return torch.stack(outs), torch.stack(embs)


def _models(H, c):
    return [_model_from_params(H, p) for p in c.params]


def _check_against_oracle(r, out64, emb64, tag):
    M = out64.shape[0]
    assert tuple(r.out.shape) == tuple(out64.shape) and tuple(r.emb.shape) == tuple(emb64.shape)
    fig_e = [rel_inf(r.emb[k], emb64[k]) for k in range(M)]
    fig_o = [rel_inf(r.out[k], out64[k], floor=1.0) for k in range(M)]
    print(f"    {tag}: per model emb " + " ".join(f"{v:.2e}" for v in fig_e) + " | out " + " ".join(f"{v:.2e}" for v in fig_o))
    assert max(fig_e) <= TOL, fig_e
    assert max(fig_o) <= TOL, fig_o


# ------------------------------------------------------------------------------------------------ 1. parity
@pytest.mark.parametrize("name", list(CASES))
def test_parity_with_the_fp64_oracle_per_model(H, name):
    c = _synth_case(name)
    ens = H.EnsemblePredict(_models(H, c))
    gb = _gpu_batch(H, c)
    assert ens.reason(gb) is None
    r = ens(gb, return_emb=True)
    assert ens.last_path == "fused"
    out64, emb64 = _oracle(c)
    print(f"\n  case {name}: M {M_SYNTH} B {c.B} N {c.x.shape[0]} E {c.ei.shape[1]} max {c.max_nodes} / {c.max_edges}")
    _check_against_oracle(r, out64, emb64, name)
    assert ens(gb).emb is None


@pytest.mark.parametrize("name", GOLDEN)
def test_parity_on_the_golden_files(H, name):
    c = _golden_case(int(name[len("golden"):]))
    ens = H.EnsemblePredict(_models(H, c))
    gb = _gpu_batch(H, c)
    assert ens.reason(gb) is None
    r = ens(gb, return_emb=True)
    assert ens.last_path == "fused"
    out64, emb64 = _oracle(c)
    print(f"\n  {name}: M {M_GOLDEN} B {c.B} max {c.max_nodes} / {c.max_edges}")
    _check_against_oracle(r, out64, emb64, name)
    e_ref = rel_inf(r.emb[0], c.ref_emb)
    p_ref = (r.out[0, :, 0].cpu() - c.ref_pred).abs().max().item()
    print(f"    model 0 against the reference's own numbers: emb {e_ref:.2e}  pred abs {p_ref:.2e}")
    assert e_ref <= TOL
    assert p_ref <= 5e-5


# ------------------------------------------------------------------------------------------------ 2. bitwise
def test_rows_are_bitwise_independent_of_the_ensemble_the_grouping_and_the_batch(H):
    c = _synth_case("real-size")
    models = _models(H, c)
    gb = _gpu_batch(H, c)
    ens = H.EnsemblePredict(models)
    full = [t.clone() for t in ens(gb, return_emb=True)]
    again = [t.clone() for t in ens(gb, return_emb=True)]
    assert ens.last_path == "fused"
    for a, b in zip(full, again):
        assert torch.equal(a, b)
    for mpg in (1, 2, 7):
        r = H.EnsemblePredict(models, models_per_group=mpg)(gb, return_emb=True)
        assert torch.equal(r.out, full[0]) and torch.equal(r.emb, full[1]), mpg
    for k in range(M_SYNTH):
        one = H.EnsemblePredict([models[k]])
        r = one(gb, return_emb=True)
        assert one.last_path == "fused" and tuple(r.out.shape) == (1, c.B, 1)
        assert torch.equal(r.out[0], full[0][k]) and torch.equal(r.emb[0], full[1][k]), k
    # the graphs of the batch in another order: every graph keeps its rows
    perm = torch.randperm(c.B, generator=torch.Generator().manual_seed(5))
    nptr = torch.zeros(c.B + 1, dtype=torch.long); nptr[1:] = torch.bincount(c.batch, minlength=c.B).cumsum(0)
    eptr = torch.zeros(c.B + 1, dtype=torch.long); eptr[1:] = torch.bincount(c.batch[c.ei[1]], minlength=c.B).cumsum(0)
    xs, eis, bs, off = [], [], [], 0
    for new, g in enumerate(perm.tolist()):
        a, b, ea, eb = int(nptr[g]), int(nptr[g + 1]), int(eptr[g]), int(eptr[g + 1])
        xs.append(c.x[a:b]); eis.append(c.ei[:, ea:eb] - a + off); bs.append(torch.full((b - a,), new)); off += b - a
    p = _Case()
    p.x, p.ei, p.batch, p.B = torch.cat(xs), torch.cat(eis, 1).contiguous(), torch.cat(bs), c.B
    p.max_nodes, p.max_edges = c.max_nodes, c.max_edges
    r = ens(_gpu_batch(H, p), return_emb=True)
    assert torch.equal(r.out, full[0][:, perm.cuda()]) and torch.equal(r.emb, full[1][:, perm.cuda()])


# ------------------------------------------------------------------------------------------------ 3. mean / std
def test_mean_and_std_over_the_model_axis(H):
    c = _synth_case("ragged")
    ens = H.EnsemblePredict(_models(H, c))
    r = ens(_gpu_batch(H, c))
    assert tuple(r.mean.shape) == (c.B, 1) and tuple(r.std.shape) == (c.B, 1)
    assert torch.equal(r.mean, r.out.mean(0))
    assert torch.equal(r.std, r.out.std(0, unbiased=False))
    assert float(r.std.min()) > 0.0
    one = H.EnsemblePredict(ens.models[:1])(_gpu_batch(H, c))
    assert torch.equal(one.std, torch.zeros_like(one.std)) and torch.equal(one.mean, one.out[0])


# ------------------------------------------------------------------------------------------------ 4. snapshot
def test_weights_are_a_snapshot_until_refresh(H):
    c = _synth_case("ragged")
    models = _models(H, c)
    ens = H.EnsemblePredict(models)
    gb = _gpu_batch(H, c)
    first = [t.clone() for t in ens(gb, return_emb=True)]
    with torch.no_grad():
        models[3].conv1.lin.weight.mul_(1.25)
        models[3].readout[-1].bias.add_(0.5)
    r = ens(gb, return_emb=True)
    assert torch.equal(r.out, first[0]) and torch.equal(r.emb, first[1])
    ens.refresh()
    r = ens(gb, return_emb=True)
    assert ens.last_path == "fused"
    assert not torch.equal(r.out[3], first[0][3]) and not torch.equal(r.emb[3], first[1][3])
    for k in (0, 1, 2, 4, 5, 6):
        assert torch.equal(r.out[k], first[0][k]) and torch.equal(r.emb[k], first[1][k])
    now = [{k: v.detach().cpu() for k, v in m.state_dict().items()} for m in models]
    out64, emb64 = _oracle(c, now)
    print()
    _check_against_oracle(r, out64, emb64, "after refresh")


# ------------------------------------------------------------------------------------------------ 5. fallback
def test_other_widths_take_the_loop_path_with_the_same_bounds(H):
    bk = dict(num_graphs=8, nodes=57, extra_bonds=4, max_degree=4, feat=25, nodes_jitter=9)
    c = _synth_case("D = 128", M=3, D=128, bk=bk, mk=dict(n_conv=2, n_read=2, n_classes=1))
    ens = H.EnsemblePredict(_models(H, c))
    gb = _gpu_batch(H, c)
    assert "shape" in ens.reason(gb)
    r = ens(gb, return_emb=True)
    assert ens.last_path == "loop"
    out64, emb64 = _oracle(c)
    print()
    _check_against_oracle(r, out64, emb64, "D = 128 (loop)")
    assert torch.equal(r.mean, r.out.mean(0)) and torch.equal(r.std, r.out.std(0, unbiased=False))


# ------------------------------------------------------------------------------------------------ 6. predict_networks
def test_predict_networks_returns_what_predict_network_returns_per_model(H):
    from hcatgnet_amd import synth, train
    bk, mk = CASES["real-size"]
    sb = synth.make_batch(**bk)
    graphs = sb.as_graph_list()
    models = [_model_from_params(H, _rand_params(bk["feat"], 64, seed=PARAM_SEED + k, **mk)) for k in range(3)]
    loader = H.DataLoader(graphs, batch_size=16)                      # 40 graphs: 16 + 16 + 8
    got = train.predict_networks(models, loader, return_emb=True)
    assert len(got) == 3
    worst = 0.0
    for k, m in enumerate(models):
        y_pred, y_true, idx, frame = train.predict_network(m, loader, return_emb=True)
        g_pred, g_true, g_idx, g_frame = got[k]
        assert (g_idx == idx).all() and (g_true == y_true).all()
        assert g_pred.shape == y_pred.shape == (len(graphs),)
        worst = max(worst, float(abs(g_pred - y_pred).max()))
        assert list(g_frame.columns) == list(frame.columns) == list(range(128)) + ["ddG_exp", "ddG_pred", "index"]
        assert (g_frame["index"].to_numpy() == idx).all() and (g_frame["ddG_exp"].to_numpy() == y_true).all()
        assert (g_frame["ddG_pred"].to_numpy() == g_pred).all()
        emb_diff = float(abs(g_frame[list(range(128))].to_numpy() - frame[list(range(128))].to_numpy()).max())
        assert emb_diff <= 1e-4
    print(f"\n    predict_networks against predict_network: y_pred max abs difference {worst:.2e}")
    assert worst <= 1e-5
    plain = train.predict_networks(models, loader)
    assert all(len(t) == 3 for t in plain)
    assert all((plain[k][0] == got[k][0]).all() for k in range(3))


# ------------------------------------------------------------------------------------------------ 7. capture
def test_captured_call_replays_on_new_node_features(H):
    c = _synth_case("ragged")
    models = _models(H, c)
    ens = H.EnsemblePredict(models)
    gb = _gpu_batch(H, c)
    ens(gb, return_emb=True)                                          # plan, buffers, LDS attribute: before the capture
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        held = ens(gb, return_emb=True)
    assert ens.last_path == "fused"
    gb.x.copy_(torch.randn(gb.x.shape, generator=torch.Generator().manual_seed(77)))
    graph.replay()
    torch.cuda.synchronize()
    got = [t.clone() for t in held]
    want = H.EnsemblePredict(models)(gb, return_emb=True)
    for a, b in zip(got, want):
        assert torch.equal(a, b)
    c.x = gb.x.cpu()
    out64, emb64 = _oracle(c)
    print()
    _check_against_oracle(held, out64, emb64, "replayed")


# ------------------------------------------------------------------------------------------------ 8. refused graphs
def test_an_oversize_graph_is_refused_or_looped_never_wrong(H):
    from hcatgnet_amd import synth
    mk = dict(n_conv=2, n_read=2, n_classes=1)
    # (a) honest metadata, one graph above the kernel's limit: the loop path, same bounds
    c = _synth_case("225 nodes", M=3, bk=dict(num_graphs=2, nodes=225, extra_bonds=4, max_degree=4, feat=25), mk=mk)
    ens = H.EnsemblePredict(_models(H, c))
    gb = _gpu_batch(H, c)
    assert "shape" in ens.reason(gb)
    r = ens(gb, return_emb=True)
    assert ens.last_path == "loop"
    out64, emb64 = _oracle(c)
    print()
    _check_against_oracle(r, out64, emb64, "225 nodes (loop)")
    # (b) metadata that understates the largest graph: the kernel refuses that graph (status bit, zero rows) and the other
    # graphs keep their values
    c = _synth_case("understated", M=3, bk=dict(num_graphs=12, nodes=60, extra_bonds=4, max_degree=4, feat=25, nodes_jitter=20), mk=mk)
    sizes = torch.bincount(c.batch, minlength=c.B)
    big = sizes == sizes.max()
    assert 0 < int(big.sum()) < c.B
    ens = H.EnsemblePredict(_models(H, c))
    honest = [t.clone() for t in ens(_gpu_batch(H, c), return_emb=True)]
    c.max_nodes = int(sizes.max()) - 1
    gb = _gpu_batch(H, c)
    r = ens(gb, return_emb=True)
    assert ens.last_path == "fused"
    torch.cuda.synchronize()
    status = gb._hcg_plan.status
    word = int(status[0].item())
    status.zero_()                                                    # (shared per device: leave it clean for the next test)
    assert word & SHAPE_LIMIT
    keep = (~big).cuda()
    assert torch.equal(r.out[:, keep], honest[0][:, keep]) and torch.equal(r.emb[:, keep], honest[1][:, keep])
    assert float(r.out[:, big.cuda()].abs().max()) == 0.0 and float(r.emb[:, big.cuda()].abs().max()) == 0.0
