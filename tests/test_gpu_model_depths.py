"""GPU tests of the fused step on models of other readout and conv depths (the reference's --readout_layers and
--n_convolutions, options/base_options.py:185-197; model/gcn.py:18-45): the one-launch readout head of depth 1, 3 and 4
(csrc/head.hip: k_head_deep) against the fp64 oracle, the carried optimiser updates, and the device-side forms built on
the step -- capture, StepWindow, EpochWindow, the eval window, concurrent runs -- bitwise against the plain steps."""
import gc

import pytest
import torch

from tests.helpers import rel_inf
from tests.test_gpu_parity import H, oracle  # noqa: F401  (fixtures)

pytestmark = pytest.mark.gpu
TOL = 1e-5


@pytest.fixture(autouse=True)
def _release_graphs():
    """The trainers, windows and captured graphs a test builds hang in reference cycles (model -> trainer -> model): destroy
    them here, on an idle device, rather than in whichever later test the cyclic collector next runs -- possibly while
    that test has graphs in flight on other streams."""
    yield
    torch.cuda.synchronize()
    gc.collect()
    torch.cuda.synchronize()


def _model(H, F, D=64, R=2, n_conv=2, C=1, optimizer="Adam", lr=0.01, seed=0):
    torch.manual_seed(seed)
    m = H.make_network("GCN", H.default_options(embedding_dim=D, readout_layers=R, n_convolutions=n_conv, n_classes=C,
                                                optimizer=optimizer, lr=lr), F).cuda()
    with torch.no_grad():
        for q in m.parameters():            # non-zero biases: every gradient path matters
            if q.dim() == 1:
                q.add_(0.05)
    return m


def _synth(cfg, ng, C=1, seed=0):
    from hcatgnet_amd import synth
    sb = synth.make_config(cfg, num_graphs=ng, seed=seed)
    if C > 1:
        sb.y = 3.0 * torch.randn(ng, C, generator=torch.Generator().manual_seed(seed + 1))
    return sb


def _screened(sb, m):
    """The batch's ambiguous graphs (an activation at a LeakyReLU kink, a max-pool near-tie) re-drawn: f32 and fp64 then
    take the same branches (oracle/screen.py)."""
    from oracle import screen
    params = {k: v.detach().cpu() for k, v in m.state_dict().items()}
    sb.x, _ = screen.make_decidable(params, sb.x, sb.edge_index, sb.batch, sb.num_graphs)
    return sb


def _check_grads(oracle, m, step, sb, loss, big=False):
    """Loss, out, emb and every gradient of one step vs the oracle's forward and autograd in fp64.  The loss is
    sqrt(MSE) over the B x C outputs (with C = 1 that is `oracle.train_step_grads`, the reference's
    sqrt(MSELoss(out, y.unsqueeze(1))), which broadcasts for C > 1)."""
    p = {k: v.detach().cpu().double().requires_grad_(True) for k, v in m.state_dict().items()}
    B = sb.num_graphs
    out_ref, emb_ref = oracle.gcn_forward(p, sb.x.double(), sb.edge_index, sb.batch, B)
    l_ref = torch.sqrt(torch.nn.functional.mse_loss(out_ref, sb.y.double().reshape(out_ref.shape)))
    l_ref.backward()
    g_ref = {k: v.grad for k, v in p.items()}
    out_ref, emb_ref = out_ref.detach(), emb_ref.detach()
    l_ref = float(l_ref.detach())
    assert abs(float(loss) - l_ref) <= TOL * abs(l_ref)
    assert rel_inf(step.last_out.reshape(out_ref.shape), out_ref, floor=1.0) <= TOL
    assert rel_inf(step._bufs["cap"]["emb"][:B], emb_ref) <= TOL
    for name, prm in m.named_parameters():
        tol = 1e-4 if (big and "conv" in name) else 2 * TOL        # sums of > 1e5 terms
        assert rel_inf(prm.grad, g_ref[name]) <= tol, name


# (cfg, feature width, graphs, D): REAL = the reference's graph sizes (one graph per workgroup, dense first layer), C3 = the
# small-graph tiles, C5 = 128-wide layers (wide-layer route)
SHAPES = [("REAL", 25, 40, 64), ("C3", 64, 17, 64), ("C5", 128, 40, 128), ("REAL", 25, 1, 128)]


@pytest.mark.parametrize("R", [1, 3, 4])
@pytest.mark.parametrize("cfg,F,B,D", SHAPES)
def test_deep_heads_take_the_fused_step_and_match_the_oracle(H, oracle, R, cfg, F, B, D):
    from hcatgnet_amd.train import FusedTrainStep
    C = {1: 1, 3: 3, 4: 8}[R]
    m = _model(H, F, D=D, R=R, C=C, seed=R)
    sb = _screened(_synth(cfg, B, C=C, seed=7), m)
    step = FusedTrainStep(m, optimizer_step=False)
    batch = sb.as_batch("cuda")
    assert step.reason(batch) is None
    loss = step(batch)
    _check_grads(oracle, m, step, sb, loss)


@pytest.mark.parametrize("R,C", [(3, 1), (4, 8), (1, 3)])
def test_deep_head_at_4096_graphs(H, oracle, R, C):
    from hcatgnet_amd.train import FusedTrainStep
    m = _model(H, 64, R=R, C=C, seed=3)
    sb = _screened(_synth("C3", 4096, C=C, seed=2), m)
    step = FusedTrainStep(m, optimizer_step=False)
    loss = step(sb.as_batch("cuda"))
    _check_grads(oracle, m, step, sb, loss, big=True)


@pytest.mark.parametrize("cfg,F,n_conv", [("C3", 64, 4), ("C3", 64, 5), ("C3", 64, 7), ("REAL", 25, 4), ("REAL", 25, 6)])
def test_deep_conv_stacks_take_the_fused_step(H, oracle, cfg, F, n_conv):
    from hcatgnet_amd.train import FusedTrainStep
    m = _model(H, F, n_conv=n_conv, R=3, seed=n_conv)
    sb = _screened(_synth(cfg, 40, seed=5), m)
    step = FusedTrainStep(m, optimizer_step=False)
    batch = sb.as_batch("cuda")
    assert step.reason(batch) is None
    loss = step(batch)
    _check_grads(oracle, m, step, sb, loss)


def test_real_batch_with_seven_conv_layers_keeps_the_autograd_loop(H):
    from hcatgnet_amd import train
    from hcatgnet_amd.train import FusedTrainStep
    m = _model(H, 25, n_conv=7)
    sb = _synth("REAL", 80, seed=1)
    store = H.DeviceGraphStore(sb.as_graph_list(), device="cuda")
    loader = H.DeviceLoader(store, batch_size=40, shuffle=True, seed=0)
    assert "jobs" in FusedTrainStep(m).reason(next(iter(loader)))
    losses = [train.train_network(m, loader, "cuda") for _ in range(2)]
    assert all(v == v and v > 0 for v in losses)
    assert train.epoch_window_of(m, loader) is None


def _torch_twin(rule, m):
    ps = [q.detach().clone().requires_grad_(True) for q in m.parameters()]
    lr = m.optimizer.param_groups[0]["lr"]
    if rule == "Adam":
        return ps, torch.optim.Adam(ps, lr=lr, eps=1e-9)
    if rule == "SGD":
        return ps, torch.optim.SGD(ps, lr=lr)
    return ps, torch.optim.RMSprop(ps, lr=lr)


@pytest.mark.parametrize("rule", ["Adam", "SGD", "rmsprop"])
def test_carried_updates_follow_torch(H, rule):
    """Several carried steps (the update in the step's last launch, its step number advanced by the deep head): each update
    equals torch's optimiser applied to the same gradients, and the step count rises by one per step."""
    from hcatgnet_amd.train import FusedTrainStep
    m = _model(H, 25, R=4, n_conv=3, optimizer=rule, lr=1e-3 if rule == "rmsprop" else 0.01)
    batch = _synth("REAL", 40, seed=4).as_batch("cuda")
    step = FusedTrainStep(m)
    ps, opt = _torch_twin(rule, m)
    for it in range(5):
        step(batch)
        assert step._last_carried
        assert m.optimizer.steps_done() == it + 1
        for rp, q in zip(ps, m.parameters()):
            rp.grad = q.grad.detach().clone()
        opt.step()
        for q, rp in zip(m.parameters(), ps):
            assert rel_inf(q, rp) <= 2e-6, (it, rule)
            rp.data.copy_(q.detach())          # (each update from the same state)


def test_two_launches_of_a_step_are_bitwise_equal(H):
    from hcatgnet_amd.train import FusedTrainStep
    batch = _synth("REAL", 40, seed=10).as_batch("cuda")
    step = FusedTrainStep(_model(H, 25, R=3, n_conv=4, seed=9), optimizer_step=False)
    l1 = float(step(batch)); g1 = step._flat.clone(); o1 = step.last_out.clone()
    l2 = float(step(batch))
    assert l1 == l2 and torch.equal(step._flat, g1) and torch.equal(step.last_out, o1)


def _fresh(H, cfg, ng, seed):
    sb = _synth(cfg, ng, seed=seed)
    x, ei, bv, y = sb.x.cuda(), sb.edge_index.cuda(), sb.batch.cuda(), sb.y.cuda()
    return lambda: H.Batch(x, ei, bv, sb.num_graphs, y=y, max_nodes=sb.max_nodes, max_edges=sb.max_edges, edges_grouped=True)


def test_captured_step_replays_like_eager_steps(H):
    """2 warm-up steps + 4 replays of the captured step == 6 eager steps on a twin (as tests/test_gpu_train_step.py)."""
    from hcatgnet_amd.train import FusedTrainStep
    a, b = _model(H, 25, R=4, seed=2), _model(H, 25, R=4, seed=2)
    fresh = _fresh(H, "REAL", 40, 3)
    ea, eb = FusedTrainStep(a), FusedTrainStep(b)
    la = [float(ea(fresh())) for _ in range(6)]
    eb.capture(fresh)
    lb = [float(eb.replay()) for _ in range(4)]
    assert b.optimizer.steps_done() == 6
    for u, v in zip(la[2:], lb):
        assert abs(u - v) <= 1e-6 * abs(u)
    for q, r in zip(a.parameters(), b.parameters()):
        assert rel_inf(r, q) <= 1e-6


def test_step_window_equals_the_same_steps_one_by_one(H):
    """Three steps on three batches captured as ONE hipGraph: two replays == the same six steps eagerly, bitwise."""
    from hcatgnet_amd.train import FusedTrainStep, StepWindow
    for cfg, F, R, n_conv in (("C3", 64, 3, 5), ("REAL", 25, 1, 3)):
        fresh = [_fresh(H, cfg, 24, 20 + i) for i in range(3)]
        a, b = _model(H, F, R=R, n_conv=n_conv, seed=4), _model(H, F, R=R, n_conv=n_conv, seed=4)
        sa = [FusedTrainStep(a) for _ in range(3)]
        win = StepWindow([FusedTrainStep(b) for _ in range(3)], fresh)     # its warm-up runs the three steps once
        la = [float(sa[i](fresh[i]())) for i in range(3)]
        lb = []
        for _ in range(2):
            la += [float(sa[i](fresh[i]())) for i in range(3)]
            lb += [float(v) for v in win.replay()]
        assert lb == la[3:], (cfg, lb, la[3:])
        assert b.optimizer.steps_done() == a.optimizer.steps_done() == 9
        for q, r in zip(a.parameters(), b.parameters()):
            assert torch.equal(q, r), cfg


@pytest.mark.parametrize("R,n_conv", [(3, 2), (1, 4)])
def test_epoch_window_equals_the_per_batch_loop(H, R, n_conv):
    """535 REAL graphs in batches of 40 (the reference's training loader): the epoch is ONE hipGraph and its values and
    weights are bitwise those of the per-batch loop on the same permutations."""
    from hcatgnet_amd import train
    store = H.DeviceGraphStore(_synth("REAL", 535, seed=1).as_graph_list(), device="cuda")
    a, b = _model(H, 25, R=R, n_conv=n_conv, seed=6), _model(H, 25, R=R, n_conv=n_conv, seed=6)
    la = H.DeviceLoader(store, batch_size=40, shuffle=True, seed=11)
    lb = H.DeviceLoader(store, batch_size=40, shuffle=True, seed=11)
    win = train.epoch_window_of(a, la, build=True)
    assert win is not None
    assert a.optimizer.steps_done() == 0
    va = [train.train_network(a, la, "cuda") for _ in range(3)]
    train.EPOCH_WINDOW = False
    try:
        vb = [train.train_network(b, lb, "cuda") for _ in range(3)]
    finally:
        train.EPOCH_WINDOW = True
    assert va == vb, (va, vb)
    for q, r in zip(a.parameters(), b.parameters()):
        assert torch.equal(q, r)
    assert a.optimizer.steps_done() == 3 * len(la)


def test_train_networks_over_mixed_depths_equals_the_runs_one_by_one(H):
    from hcatgnet_amd import train
    store = H.DeviceGraphStore(_synth("REAL", 130, seed=2).as_graph_list(), device="cuda")
    depths = [(2, 2), (3, 2), (1, 4), (4, 3)]
    ms = [_model(H, 25, R=R, n_conv=n, seed=i) for i, (R, n) in enumerate(depths)]
    ref = [_model(H, 25, R=R, n_conv=n, seed=i) for i, (R, n) in enumerate(depths)]
    loaders = [H.DeviceLoader(store, batch_size=40, shuffle=True, seed=30 + i) for i in range(len(ms))]
    loaders_r = [H.DeviceLoader(store, batch_size=40, shuffle=True, seed=30 + i) for i in range(len(ms))]
    for _ in range(2):
        got = train.train_networks(ms, loaders, "cuda")
        want = [train.train_network(m, ld, "cuda") for m, ld in zip(ref, loaders_r)]
        assert list(got) == want
    for m, r in zip(ms, ref):
        for q, p in zip(m.parameters(), r.parameters()):
            assert torch.equal(q, p)


def test_eval_window_equals_the_batch_loop(H):
    from hcatgnet_amd.train import FusedTrainStep, eval_network, eval_window_of
    store = H.DeviceGraphStore(_synth("REAL", 130, seed=3).as_graph_list(), device="cuda")
    val = H.DeviceLoader(store, batch_size=40)
    m = _model(H, 25, R=4, n_conv=4, seed=8)
    st = FusedTrainStep(m, optimizer_step=False)
    tot = 0.0
    for b in H.DeviceLoader(store, batch_size=40):
        tot += float(st.evaluate(b)) * b.num_graphs
    want = tot / len(store)
    got = eval_network(m, val, "cuda")
    assert eval_window_of(m, val) is not None
    assert abs(got - want) <= 1e-6 * abs(want), (got, want)


@pytest.mark.parametrize("cfg,F", [("C3", 64), ("REAL", 25)])
def test_default_depth_keeps_its_head_launches(H, cfg, F, monkeypatch):
    """A default-depth model never reaches the deep head: its head stays hcg_head_fwd_bwd or the forward's tail."""
    from hcatgnet_amd.train import FusedTrainStep

    def refuse(self, c):
        raise AssertionError("deep head launched for a depth-2 readout")
    monkeypatch.setattr(FusedTrainStep, "_head_deep", refuse)
    m = _model(H, F)
    step = FusedTrainStep(m)
    for _ in range(2):
        assert float(step(_synth(cfg, 40, seed=1).as_batch("cuda"))) > 0
