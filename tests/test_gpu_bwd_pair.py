"""GPU tests of the two-layer backward pair (csrc/fused.hip: k_fused_bwd_pair; mode HCG_FUSED_BWD_PAIR of
hcg_fused_forward): conv layers 1 and 0 of the small-graph tiles as two phases of ONE launch.  Per-tile arithmetic,
per-wave accumulation order, combine order and slabs are those of the two single launches, so the reference is the
two-launch form on the same inputs and every comparison is `torch.equal`."""
import ctypes
import gc

import numpy as np
import pytest
import torch

from tests.test_gpu_parity import H  # noqa: F401  (fixture)

pytestmark = pytest.mark.gpu
D, SLOPE = 64, 0.01


@pytest.fixture(autouse=True)
def _release_graphs():
    yield
    torch.cuda.synchronize()
    gc.collect()
    torch.cuda.synchronize()


def _graphs(ns, feat, seed, edgeless=()):
    """A collated batch of graphs with `ns` nodes each: a chain plus random chords per graph, both directions, edges
    grouped by graph; the graphs in `edgeless` (and single nodes) have no edge.  -> (x, edge_index, batch, y, max_edges)"""
    rng = np.random.default_rng(seed)
    src, dst, me, base = [], [], 0, 0
    for g, n in enumerate(ns):
        e = []
        if n > 1 and g not in edgeless:
            e = [(i, i + 1) for i in range(n - 1)]
            e += [tuple(rng.choice(n, 2, replace=False)) for _ in range(n // 3)]
        for i, j in e:
            src += [base + i, base + j]
            dst += [base + j, base + i]
        me = max(me, 2 * len(e))
        base += n
    x = torch.from_numpy(rng.standard_normal((base, feat), dtype=np.float32))
    ei = torch.tensor([src, dst], dtype=torch.int64).reshape(2, -1)
    bv = torch.from_numpy(np.repeat(np.arange(len(ns)), ns)).long()
    y = torch.from_numpy((10.0 * rng.standard_normal(len(ns))).astype(np.float32))
    return x, ei, bv, y, max(me, 1)


CASES = ["one_wg", "packed20", "packed19", "multi_wg", "dealt"]
# the upper layer's three forms at the C ABI: the training form on every shape, the other two on three of them
ABI_CASES = [(n, "bits") for n in CASES] + [(n, f) for f in ("pooled", "plain") for n in ("one_wg", "packed20", "multi_wg")]


def _cus():
    return torch.cuda.get_device_properties(0).multi_processor_count


def _case(name):
    """-> (node counts, F, graphs without edges).  The shapes are the smallest that reach each path of the kernel."""
    rng = np.random.default_rng(CASES.index(name))
    if name == "one_wg":        # 3 tiles in the only workgroup: five of its eight waves have no tile in either phase
        return [30, 30, 30], 64, ()
    if name in ("packed20", "packed19"):   # 3 graphs per tile, KPAD 32, non-VEC; 19 graphs: the last tile holds ONE graph
        B = 20 if name == "packed20" else 19
        ns = list(rng.integers(1, 11, B))
        ns[0], ns[4], ns[7], ns[B - 1] = 10, 1, 6, 5      # max 10 -> three per tile; a single node; graph 7 gets no edges
        return ns, 25, (7,)
    if name == "multi_wg":      # 300 tiles: 38 workgroups, one round, the last workgroup has 4 tiles
        return list(rng.integers(24, 31, 300)), 64, ()
    if name == "dealt":         # 8 CUs + 52 tiles on the 8 CUs waves of a full grid: a partial last round -> the host picks DEAL
        return list(rng.integers(29, 31, 8 * _cus() + 52)), 32, ()
    raise KeyError(name)


def _batch(H, name, seed=0):
    ns, feat, edgeless = _case(name)
    x, ei, bv, y, me = _graphs(ns, feat, seed, edgeless)
    x, ei, bv, y = x.cuda(), ei.cuda(), bv.cuda(), y.cuda()      # uploaded once: `mk` also runs inside a stream capture
    mk = lambda: H.Batch(x, ei, bv, len(ns), y=y, max_nodes=int(max(ns)), max_edges=me, edges_grouped=True)
    return mk, feat, ns


# ---------------------------------------------------------------------------------------------------------------- C ABI
@pytest.mark.parametrize("name,form", ABI_CASES)
def test_pair_launch_equals_the_two_launches(H, name, form):
    """dx, both slab workspaces and dW / db after hcg_step_tail: the pair launch against hcg_fused_layer_bwd twice."""
    from hcatgnet_amd import _lib
    from hcatgnet_amd import functional as HF
    from hcatgnet_amd.plan import BatchPlan
    lib, p = _lib.load(), _lib.ptr
    mk, feat, ns = _batch(H, name)
    b = mk()
    plan = BatchPlan.build(b.edge_index, b.batch, b.x.shape[0], num_graphs=b.num_graphs, mode="blocked",
                           max_nodes=b.max_nodes, max_edges=b.max_edges)
    N, B = plan.N, plan.B
    gpt = HF.fused_graphs_per_tile(plan, feat, D)
    assert gpt == 32 // max(ns) and gpt == HF.fused_graphs_per_tile(plan, D, D)
    gen = torch.Generator().manual_seed(17)
    rnd = lambda *s: torch.randn(*s, generator=gen).cuda()
    x = b.x.contiguous()
    W1, b1, W2, b2 = rnd(D, feat) * 0.2, rnd(D) * 0.1, rnd(D, D) * 0.2, rnd(D) * 0.1
    new = lambda *s: torch.full(s, -7.0, device="cuda")
    out1, out2, emb = new(N, D), new(N, D), new(B, 2 * D)
    bits = torch.zeros(lib.hcg_fused_aux_bytes(_lib.HCG_FUSED_POOLBITS, B, gpt), dtype=torch.uint8, device="cuda")
    common = dict(edge_index=plan.edge_index, E=plan.E, graph_ptr=plan.graph_ptr, edge_ptr=plan.edge_ptr, N=N, B=B, D=D,
                  graphs_per_tile=gpt, slope=SLOPE, status=plan.status)
    if form == "bits":
        _lib.fused_forward(x=x, W1=W1, b1=b1, W2=W2, b2=b2, F=feat, out1=out1, emb=emb, poolbits=bits, apply_act=1, **common)
    else:
        _lib.fused_forward(x=x, W1=W1, b1=b1, W2=W2, b2=b2, F=feat, out1=out1, out2=out2, emb=emb, apply_act=1, **common)
    demb, dout = rnd(B, 2 * D), rnd(N, D)
    # the upper layer's arguments in the three forms: (dout, demb, emb, out, poolbits)
    up = {"bits": (None, demb, None, None, bits), "pooled": (None, demb, emb, out2, None),
          "plain": (dout, None, None, out2, None)}[form]
    geo = (p(plan.edge_index), plan.E, p(plan.graph_ptr), p(plan.edge_ptr), N, B)
    wsb1, wsb0 = lib.hcg_fused_workspace_bytes(B, D, D, gpt), lib.hcg_fused_workspace_bytes(B, feat, D, gpt)
    st = _lib.stream_ptr()

    def run(pair):
        ws1 = torch.zeros(wsb1, dtype=torch.uint8, device="cuda")
        ws0 = torch.zeros(wsb0, dtype=torch.uint8, device="cuda")
        dx = new(N, D)
        if pair:
            ok = HF.TILES.backward_pair(HF.geometry(plan), gpt, x, W1, out1, W2, 3, dout=up[0], demb=up[1], emb=up[2],
                                        out=up[3], poolbits=up[4], dx=dx, ws_up=ws1, wsb_up=wsb1, ws=ws0, wsb=wsb0, slope=SLOPE)
            assert ok is True
        else:
            _lib.check(lib.hcg_fused_layer_bwd(p(up[0]), p(up[1]), p(up[2]), p(up[3]), p(up[4]), p(out1), p(W2), *geo, D, D,
                                               gpt, SLOPE, 3, p(dx), p(plan.status), p(ws1), wsb1, st), "upper")
            _lib.check(lib.hcg_fused_layer_bwd(p(dx), None, None, None, None, p(x), p(W1), *geo, feat, D, gpt, SLOPE, 0, None,
                                               p(plan.status), p(ws0), wsb0, st), "lower")
        grads = [new(D, D), new(D), new(D, feat), new(D)]
        jobs = (ctypes.c_char * (2 * _lib.job_bytes()))()
        a = ctypes.addressof(jobs)
        _lib.check(lib.hcg_fused_reduce_job(p(ws1), wsb1, N, B, D, D, gpt, p(grads[0]), p(grads[1]), a), "job")
        _lib.check(lib.hcg_fused_reduce_job(p(ws0), wsb0, N, B, feat, D, gpt, p(grads[2]), p(grads[3]), a + _lib.job_bytes()), "job")
        _lib.reduce_jobs(a, 2)          # hcg_step_tail, reductions only
        torch.cuda.synchronize()
        return [dx, ws1[:-256], ws0[:-256]] + grads

    ref, got = run(False), run(True)
    assert int(plan.status[0]) == 0
    assert bool(torch.isfinite(ref[0]).all()) and float(ref[3].abs().max()) > 0 and float(ref[5].abs().max()) > 0
    for what, r, g in zip(("dx", "upper slabs", "lower slabs", "dW1", "db1", "dW0", "db0"), ref, got):
        assert torch.equal(r, g), what


def test_launch_form_checks_its_workspaces(H):
    from hcatgnet_amd import _lib
    from hcatgnet_amd import functional as HF
    from hcatgnet_amd.plan import BatchPlan
    mk, feat, ns = _batch(H, "one_wg")
    b = mk()
    plan = BatchPlan.build(b.edge_index, b.batch, b.x.shape[0], num_graphs=b.num_graphs, mode="blocked",
                           max_nodes=b.max_nodes, max_edges=b.max_edges)
    z = lambda *s: torch.zeros(*s, device="cuda")
    ws = torch.zeros(64, dtype=torch.uint8, device="cuda")
    with pytest.raises(_lib.HcgError, match="workspace"):
        HF.TILES.backward_pair(HF.geometry(plan), 1, b.x, z(D, feat), z(plan.N, D), z(D, D), 2, dout=z(plan.N, D), dx=z(plan.N, D),
                               ws_up=ws, wsb_up=64, ws=ws, wsb=64)


# ------------------------------------------------------------------------------------------------------ FusedTrainStep
def _model(H, F, n_conv=2, seed=0):
    torch.manual_seed(seed)
    m = H.make_network("GCN", H.default_options(n_convolutions=n_conv), F).cuda()
    with torch.no_grad():
        for q in m.parameters():
            if q.dim() == 1:
                q.add_(0.05)
    return m


def _count(monkeypatch, HF):
    """Counts the launches `FusedTrainStep` issues through the tile family: pair launches and single backward launches."""
    n = {"pair": 0, "single": 0}
    pair, single = HF.TILES.backward_pair, HF.TILES.backward

    def cp(*a, **kw):
        n["pair"] += 0 if kw.get("query") else 1
        return pair(*a, **kw)

    def cs(*a, **kw):
        n["single"] += 1
        return single(*a, **kw)

    monkeypatch.setattr(HF.TILES, "backward_pair", cp)
    monkeypatch.setattr(HF.TILES, "backward", cs)
    return n


def _step_outputs(H, mk, F, pair, n_conv=2, poolbits=True):
    from hcatgnet_amd.train import FusedTrainStep
    m = _model(H, F, n_conv)
    step = FusedTrainStep(m)
    step.BWD_PAIR, step.POOLBITS = pair, poolbits
    batch = mk()
    loss = step(batch)
    torch.cuda.synchronize()
    return ([loss.clone(), step.last_out.clone(), step._bufs["cap"]["emb"][:batch.num_graphs].clone(), step._flat.clone()]
            + [q.detach().clone() for q in m.parameters()])


def _same_step(H, monkeypatch, name, launches, **kw):
    from hcatgnet_amd import functional as HF
    mk, feat, _ = _batch(H, name)
    n = _count(monkeypatch, HF)
    ref = _step_outputs(H, mk, feat, False, **kw)
    assert n["pair"] == 0 and n["single"] == launches[0]
    n["single"] = 0
    got = _step_outputs(H, mk, feat, True, **kw)
    assert n["pair"] == 1 and n["single"] == launches[1]
    assert bool(torch.isfinite(ref[3]).all()) and float(ref[3].abs().max()) > 0
    names = ["loss", "out", "emb", "flat gradient"] + [f"weight {i} after Adam" for i in range(len(ref) - 4)]
    for what, r, g in zip(names, ref, got):
        assert torch.equal(r, g), what


@pytest.mark.parametrize("name", CASES)
def test_step_with_the_pair_equals_the_two_launch_step(H, monkeypatch, name):
    """Loss, out, emb, the flat gradient and the weights after one Adam step, BWD_PAIR on against off."""
    _same_step(H, monkeypatch, name, (2, 0))


@pytest.mark.parametrize("name", ["one_wg", "packed20", "multi_wg"])
def test_upper_layer_pooled_plain(H, monkeypatch, name):
    """POOLBITS = False: the pair's upper layer reads the pooled layer's stored activations and emb."""
    _same_step(H, monkeypatch, name, (2, 0), poolbits=False)


@pytest.mark.parametrize("name", ["one_wg", "packed20", "multi_wg"])
def test_three_conv_model_pairs_its_two_lowest_layers(H, monkeypatch, name):
    """Three conv layers: the top (pooled) layer stays a single launch, layers 1 and 0 are the pair, whose upper layer is
    not pooled and takes the top layer's premasked dx as `dout`."""
    _same_step(H, monkeypatch, name, (3, 1), n_conv=3)


def test_switches_that_rule_the_pair_out(H, monkeypatch):
    from hcatgnet_amd import functional as HF
    from hcatgnet_amd.train import FusedTrainStep
    mk, feat, _ = _batch(H, "one_wg")
    n = _count(monkeypatch, HF)
    step = FusedTrainStep(_model(H, feat), optimizer_step=False)
    step.PREMASK = False                      # dx would not go down premasked: two launches
    step(mk())
    assert n == {"pair": 0, "single": 2}
    one = FusedTrainStep(_model(H, feat, n_conv=1), optimizer_step=False)
    one(mk())
    assert n == {"pair": 0, "single": 3}


def test_captured_step_with_the_pair_replays_equal_to_eager_steps(H, monkeypatch):
    """2 warm-up steps + 3 replays of the captured step (hipGraph) == 5 eager steps on a twin, both with the pair."""
    from hcatgnet_amd import functional as HF
    from hcatgnet_amd.train import FusedTrainStep
    mk, feat, _ = _batch(H, "multi_wg")
    n = _count(monkeypatch, HF)
    a, b = _model(H, feat, seed=2), _model(H, feat, seed=2)
    ea, eb = FusedTrainStep(a), FusedTrainStep(b)
    ea.BWD_PAIR = eb.BWD_PAIR = True
    la = [ea(mk()).clone() for _ in range(5)]
    assert n == {"pair": 5, "single": 0}
    eb.capture(mk)
    lb = [eb.replay().clone() for _ in range(3)]
    torch.cuda.synchronize()
    assert n["single"] == 0 and b.optimizer.steps_done() == 5
    print("losses eager", [float(v) for v in la[2:]], "replayed", [float(v) for v in lb])
    for u, v in zip(la[2:], lb):
        assert torch.equal(u, v)
    assert torch.equal(ea.last_out, eb.last_out)
    for q, r in zip(a.parameters(), b.parameters()):
        assert torch.equal(q, r)
