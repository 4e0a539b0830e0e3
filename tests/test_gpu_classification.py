"""GPU tests of classification models (`--problem_type classification`) on the fused step: the cross-entropy form of the
three one-launch readout heads (16-row tiles, 32-row tiles at width 128, the deep head) and of the any-shape head against
the fp64 oracle, the carried optimiser updates, the device-side forms built on the step, labels outside the classes, and
the eager loss module.

The loss is `nn.CrossEntropyLoss()(out, y.long())` with `out` [B, C] and `y` [B] class indices: the mean over the graphs of
the batch, no sqrt, no unsqueeze.  Labels are drawn uniformly, independent of the model, so the mean loss stays near ln C
or above and nothing cancels in the comparisons.  Shapes are the smallest that cross each kernel's tile edge (17 graphs =
two 16-row tiles, 33 = two 32-row tiles, 1 = a lone short tile)."""
import math

import pytest
import torch

from tests.helpers import rel_inf
from tests.test_gpu_model_depths import TOL, _model, _release_graphs, _screened, _synth, _torch_twin  # noqa: F401
from tests.test_gpu_parity import H, oracle  # noqa: F401  (fixtures)

pytestmark = pytest.mark.gpu


def _cls_model(H, F, C, **kw):
    from hcatgnet_amd.networks import CrossEntropyLoss
    m = _model(H, F, C=C, **kw)
    m.loss = CrossEntropyLoss()             # what `--problem_type classification` attaches (networks._make_loss)
    return m


def _labels(B, C, seed):
    return torch.randint(0, C, (B,), generator=torch.Generator().manual_seed(seed + 1)).float()


def _cls_synth(cfg, ng, C, seed=0):
    sb = _synth(cfg, ng, seed=seed)
    sb.y = _labels(ng, C, seed)
    return sb


def _check(oracle, m, step, sb, loss):
    """Loss, out, emb and every gradient of one step vs the oracle's fp64 forward, torch's cross_entropy and autograd, at
    the bounds of tests/test_gpu_model_depths.py::_check_grads."""
    p = {k: v.detach().cpu().double().requires_grad_(True) for k, v in m.state_dict().items()}
    B = sb.num_graphs
    out_ref, emb_ref = oracle.gcn_forward(p, sb.x.double(), sb.edge_index, sb.batch, B)
    l_ref = torch.nn.functional.cross_entropy(out_ref, sb.y.long())
    l_ref.backward()
    g_ref = {k: v.grad for k, v in p.items()}
    out_ref, emb_ref, l_ref = out_ref.detach(), emb_ref.detach(), float(l_ref.detach())
    assert abs(float(loss) - l_ref) <= TOL * abs(l_ref), (float(loss), l_ref)
    assert rel_inf(step.last_out.reshape(out_ref.shape), out_ref, floor=1.0) <= TOL
    assert rel_inf(step._bufs["cap"]["emb"][:B], emb_ref) <= TOL
    for name, prm in m.named_parameters():
        assert rel_inf(prm.grad, g_ref[name]) <= 2 * TOL, name


# (cfg, feature width, graphs, D, R, C)
CASES = ([("C3", 64, 17, 64, 2, C) for C in (2, 3, 8)] + [("REAL", 25, 1, 64, 2, C) for C in (2, 3, 8)]     # k_head16
         + [("C5", 128, 33, 128, 2, C) for C in (2, 8)]                                                      # k_head<128>
         + [("C3", 64, 17, 64, R, 3) for R in (1, 3, 4)] + [("C5", 128, 17, 128, 3, 3)]                      # the deep head
         + [("REAL", 25, 17, 64, 2, 9)])                                                                     # the any-shape head


@pytest.mark.parametrize("cfg,F,B,D,R,C", CASES)
def test_one_step_matches_the_oracle(H, oracle, monkeypatch, cfg, F, B, D, R, C):
    from hcatgnet_amd.train import FusedTrainStep
    if cfg == "C3":
        # both conv layers on the small-graph tiles: a regression model's head would ride in the forward launch

        def refuse(self, c):
            raise AssertionError("the regression-only head in the forward launch was taken for a cross-entropy model")
        monkeypatch.setattr(FusedTrainStep, "_forward_with_head", refuse)
    m = _cls_model(H, F, C, D=D, R=R, seed=R + C)
    sb = _screened(_cls_synth(cfg, B, C, seed=7), m)
    step = FusedTrainStep(m, optimizer_step=False)
    batch = sb.as_batch("cuda")
    assert step.reason(batch) is None
    loss = step(batch)
    _check(oracle, m, step, sb, loss)
    # int64 class indices are taken too, with the same result
    batch_i = sb.as_batch("cuda")
    batch_i.y = batch_i.y.long()
    g = step._flat.clone()
    assert float(step(batch_i)) == float(loss) and torch.equal(step._flat, g)


@pytest.mark.parametrize("R", [2, 4])
@pytest.mark.parametrize("rule", ["Adam", "SGD", "rmsprop"])
def test_carried_updates_follow_torch(H, rule, R):
    """As tests/test_gpu_model_depths.py::test_carried_updates_follow_torch, behind the cross-entropy heads."""
    from hcatgnet_amd.train import FusedTrainStep
    m = _cls_model(H, 25, 3, R=R, optimizer=rule, lr=1e-3 if rule == "rmsprop" else 0.01)
    batch = _cls_synth("REAL", 40, 3, seed=4).as_batch("cuda")
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


@pytest.mark.parametrize("R,C,D", [(2, 3, 64), (3, 3, 64), (2, 9, 64), (2, 8, 128)])
def test_two_launches_of_a_step_are_bitwise_equal(H, R, C, D):
    from hcatgnet_amd.train import FusedTrainStep
    batch = _cls_synth("REAL", 40, C, seed=10).as_batch("cuda")
    step = FusedTrainStep(_cls_model(H, 25, C, D=D, R=R, seed=9), optimizer_step=False)
    l1 = float(step(batch)); g1 = step._flat.clone(); o1 = step.last_out.clone()
    l2 = float(step(batch))
    assert l1 == l2 and torch.equal(step._flat, g1) and torch.equal(step.last_out, o1)
    assert math.isfinite(l1) and l1 > 0


def _fresh(H, cfg, ng, seed, C):
    sb = _cls_synth(cfg, ng, C, seed=seed)
    x, ei, bv, y = sb.x.cuda(), sb.edge_index.cuda(), sb.batch.cuda(), sb.y.cuda()
    return lambda: H.Batch(x, ei, bv, sb.num_graphs, y=y, max_nodes=sb.max_nodes, max_edges=sb.max_edges, edges_grouped=True)


def test_step_window_equals_the_same_steps_one_by_one(H):
    """Three steps on three batches captured as ONE hipGraph: two replays == the same six steps eagerly, bitwise."""
    from hcatgnet_amd.train import FusedTrainStep, StepWindow
    for cfg, F, R in (("C3", 64, 2), ("REAL", 25, 3)):
        fresh = [_fresh(H, cfg, 24, 20 + i, 3) for i in range(3)]
        a, b = _cls_model(H, F, 3, R=R, seed=4), _cls_model(H, F, 3, R=R, seed=4)
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


def test_epoch_window_equals_the_per_batch_loop(H):
    """130 REAL graphs in batches of 40: the epoch is ONE hipGraph, bitwise the per-batch loop on the same permutations."""
    from hcatgnet_amd import train
    store = H.DeviceGraphStore(_cls_synth("REAL", 130, 3, seed=1).as_graph_list(), device="cuda")
    a, b = _cls_model(H, 25, 3, seed=6), _cls_model(H, 25, 3, seed=6)
    la = H.DeviceLoader(store, batch_size=40, shuffle=True, seed=11)
    lb = H.DeviceLoader(store, batch_size=40, shuffle=True, seed=11)
    win = train.epoch_window_of(a, la, build=True)
    assert win is not None
    assert a.optimizer.steps_done() == 0
    va = [train.train_network(a, la, "cuda") for _ in range(2)]
    train.EPOCH_WINDOW = False
    try:
        vb = [train.train_network(b, lb, "cuda") for _ in range(2)]
    finally:
        train.EPOCH_WINDOW = True
    assert va == vb, (va, vb)
    assert all(math.isfinite(v) and v > 0 for v in va)
    for q, r in zip(a.parameters(), b.parameters()):
        assert torch.equal(q, r)
    assert a.optimizer.steps_done() == 2 * len(la)


def test_eval_window_equals_the_batch_loop(H):
    from hcatgnet_amd.train import FusedTrainStep, eval_network, eval_window_of
    store = H.DeviceGraphStore(_cls_synth("REAL", 130, 3, seed=3).as_graph_list(), device="cuda")
    val = H.DeviceLoader(store, batch_size=40)
    m = _cls_model(H, 25, 3, R=4, seed=8)
    st = FusedTrainStep(m, optimizer_step=False)
    tot = 0.0
    for b in H.DeviceLoader(store, batch_size=40):
        tot += float(st.evaluate(b)) * b.num_graphs
    want = tot / len(store)
    got = eval_network(m, val, "cuda")
    assert eval_window_of(m, val) is not None
    assert abs(got - want) <= 1e-6 * abs(want), (got, want)


@pytest.mark.parametrize("R,C,D", [(2, 3, 64), (4, 3, 64), (2, 9, 64), (2, 3, 128)])
def test_labels_outside_the_classes_give_a_nan_loss_and_nothing_else(H, R, C, D):
    """A label equal to C, one equal to -1 and one equal to 1.5: no class matches, so those graphs' terms -- and the batch
    loss -- are NaN; the label selects by comparison only, so `out` is what the clean batch gives and the call returns."""
    from hcatgnet_amd.train import FusedTrainStep
    sb = _cls_synth("REAL", 17, C, seed=12)
    m = _cls_model(H, 25, C, D=D, R=R, seed=5)
    step = FusedTrainStep(m, optimizer_step=False)
    clean = float(step.evaluate(sb.as_batch("cuda")))
    out = step.last_out.clone()
    assert math.isfinite(clean)
    sb.y = sb.y.clone()
    sb.y[2], sb.y[9], sb.y[16] = float(C), -1.0, 1.5
    loss = float(step.evaluate(sb.as_batch("cuda")))
    torch.cuda.synchronize()
    assert math.isnan(loss)
    assert torch.equal(step.last_out, out)


@pytest.mark.parametrize("B,C", [(17, 3), (1, 9)])
def test_eager_loss_module_matches_fp64_torch(H, B, C):
    from hcatgnet_amd.networks import CrossEntropyLoss
    g = torch.Generator().manual_seed(B + C)
    out = 3.0 * torch.randn(B, C, generator=g)
    y = torch.randint(0, C, (B,), generator=g)
    ref = out.double().requires_grad_(True)
    l_ref = torch.nn.functional.cross_entropy(ref, y)
    (2.0 * l_ref).backward()
    a = out.cuda().requires_grad_(True)
    loss = CrossEntropyLoss()(a, y.cuda())
    assert loss.dim() == 0
    (2.0 * loss).backward()
    assert abs(float(loss.detach()) - float(l_ref.detach())) <= 1e-6 * abs(float(l_ref.detach()))
    assert rel_inf(a.grad, ref.grad) <= 1e-6
