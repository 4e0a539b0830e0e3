"""GPU checks of the reference's other two optimisers (`--optimizer SGD | rmsprop`, model/networks.py:36-44) on the device
path: torch's default rules

    SGD:      p -= lr g
    RMSprop:  v = alpha v + (1 - alpha) g^2 ;  p -= lr g / (sqrt(v) + eps)

in every form an update takes -- the plain capturable launch (hcg_update_dev), its data-parallel SSE form, the update carried
in the step's last launch (hcg_step_tail) -- element by element against an fp64 evaluation with the float32 hyper-parameters
the C ABI receives, then at model level against torch.optim.SGD / RMSprop fed the same gradients, through the captured step,
StepWindow, the one-graph epoch (EpochWindow), the concurrent runs of train_networks and the RCCL forms at world size 1."""
import copy
import ctypes

import pytest
import torch

from tests.test_gpu_parity import H  # noqa: F401  (fixture)

pytestmark = pytest.mark.gpu

ULP = 2.0 ** -23                     # float32 spacing at 1
ALPHA, EPS = 0.99, 1e-8              # torch.optim.RMSprop's defaults (what the reference builds)
F32 = lambda x: float(torch.tensor(x, dtype=torch.float32))     # the float the C ABI receives
RULES = ["SGD", "rmsprop"]

N_LIST = [1, 255, 256, 257, 14145, 16641, (1 << 22) + 3]          # 16641 / 14145: the default model (F = 64) / F = 25
LRS = [0.01, 1e-4]
ZERO, TINY, HUGE = 0, 1, 2            # gradient classes (the rest are normal values)
SSE, CNT = 160.0, 40.0               # the SSE form's [SSE, count] tail: sqrt(MSE) = 2, gradient scale 1 / 80


def _rule(name):
    from hcatgnet_amd import _lib
    return _lib.HCG_UPDATE_SGD if name == "SGD" else _lib.HCG_UPDATE_RMSPROP


def _inputs(n, lr, seed):
    """Parameters, gradients and square averages of n elements: mostly normal values, plus exact zeros (zero average),
    tiny gradients whose square underflows (zero average) and huge ones whose square overflows float32."""
    g = torch.Generator().manual_seed(seed)
    cls = (torch.arange(n) * 7 + 3) % 16
    grad = torch.randn(n, generator=g)
    v = torch.rand(n, generator=g) * 0.01 + 1e-6
    p = torch.randn(n, generator=g) * (40 * lr)         # |p| ~ |update|: the update is not lost in p's rounding
    sign = torch.where(torch.rand(n, generator=g) < 0.5, -1.0, 1.0)
    grad[cls == ZERO] = 0.0
    grad[cls == TINY] = 1e-30 * sign[cls == TINY]
    grad[cls == HUGE] = 1e30 * sign[cls == HUGE]
    v[(cls == ZERO) | (cls == TINY)] = 0.0
    return p, grad, v, cls


def _reference(rule, p, g, v, lr):
    """fp64 evaluation of the rule with the float32 hyper-parameters -> (p, v, per-element bounds for p, v)."""
    lr = F32(lr)
    p, g, v = (x.double() for x in (p, g, v))
    if rule == "SGD":
        upd = lr * g
        p2 = p - upd
        return p2, v, 2 * ULP * upd.abs() + ULP * p2.abs() + 1e-45, torch.zeros_like(v)
    a, eps = F32(ALPHA), F32(EPS)
    v2 = a * v + (1 - a) * g * g
    upd = lr * g / (v2.sqrt() + eps)
    p2 = p - upd
    return p2, v2, 8 * ULP * upd.abs() + ULP * p2.abs() + 1e-45, 3 * ULP * v2.abs() + 1e-38


def _assert_close(name, got, want, tol, ctx):
    got, want, tol = got.detach().double().cpu().reshape(-1), want.reshape(-1), tol.reshape(-1)
    bad = ~((got - want).abs() <= tol)
    if bool(bad.any()):
        i = int(bad.nonzero()[0])
        raise AssertionError(f"{ctx}: {name}: {int(bad.sum())} of {got.numel()} elements off, first [{i}] got {got[i].item()!r} "
                             f"want {want[i].item()!r} (tol {tol[i].item():.3g})")


def _check_update(rule, ctx, p, v, p0, g0, v0, lr, cls):
    """(p, v) after the launch vs the fp64 rule from (p0, g0, v0)."""
    p, v = p.cpu(), v.cpu()
    p2, v2, tp, tv = _reference(rule, p0, g0, v0, lr)
    keep = torch.ones_like(cls, dtype=torch.bool)
    if rule == "rmsprop":
        huge = cls == HUGE
        # g^2 overflows: float32's rule gives v = inf, g / inf = 0, p unchanged (as float32 torch.optim.RMSprop); fp64 has no
        # overflow
        assert torch.equal(p[huge], p0[huge]) and bool(torch.isinf(v[huge]).all()), ctx
        keep = ~huge
        _assert_close("v", v[keep], v2[keep], tv[keep], ctx)
        # tiny gradients: their square underflows, the average stays exactly 0 (as in float32 torch)
        assert bool((v[cls == TINY] == 0).all()) and bool((v[cls == ZERO] == 0).all()), ctx
    else:
        assert torch.equal(v, v0), ctx                        # (SGD keeps no state: the buffer is not touched)
    _assert_close("p", p[keep], p2[keep], tp[keep], ctx)
    assert torch.equal(p[cls == ZERO], p0[cls == ZERO]), ctx


def _one_slab_job(slab, dst, n):
    """One reduction job over ONE slab = the data itself (the tail's sum is then exactly the slab)."""
    from hcatgnet_amd import _lib
    job = ctypes.create_string_buffer(_lib.job_bytes())
    j = _lib.ReduceJob.from_buffer(job)
    j.slabs, j.sse_part, j.nslabs, j.slab_floats, j.nseg = slab.data_ptr(), None, 1, n, 1
    j.seg[0] = _lib.ReduceSeg(0, n, n, n, dst.data_ptr())
    return job


def _launch(rule, kind, n, p, g, v, lr, step_dev, loss):
    """One update of `kind`: "dev" (hcg_update_dev), "sse" (its SSE form: `g` = [n | SSE | count]), "tail" (hcg_step_tail
    reducing the one slab `g` into a fresh flat gradient; step_dev[0] must already hold this update's number)."""
    from hcatgnet_amd import _lib
    lr_dev = torch.tensor([lr], dtype=torch.float32, device="cuda")
    st = dict(exp_avg_sq=v if rule == "rmsprop" else None)
    if kind == "tail":
        flat = torch.full((n,), float("nan"), device="cuda")
        job = _one_slab_job(g, flat, n)
        _lib.step_tail(ctypes.addressof(job), 1, update=dict(rule=_rule(rule), grad_flat=flat, param=p, n=n, lr_dev=lr_dev,
                                                            step_dev=step_dev, beta1=0.0, beta2=ALPHA, eps=EPS, **st))
        torch.cuda.synchronize()
        assert torch.equal(flat.cpu(), g.cpu())
        return
    _lib.update_dev(g, rule=_rule(rule), param=p, n=n, lr_dev=lr_dev, step_dev=step_dev, beta2=ALPHA, eps=EPS,
                    loss=loss if kind == "sse" else None, **st)
    torch.cuda.synchronize()


def _run_one(rule, kind, n, lr, seed, k=999, stamp=5):
    p0, g0, v0, cls = _inputs(n, lr, seed)
    p, v = p0.cuda(), v0.cuda()
    step_dev = torch.tensor([k + (1 if kind == "tail" else 0), stamp, 0, 0], dtype=torch.int32, device="cuda")
    loss = torch.full((2,), -1.0, device="cuda")
    g = torch.cat([g0, torch.tensor([SSE, CNT])]).cuda() if kind == "sse" else g0.cuda()
    ctx = f"{rule} {kind} n={n} lr={lr}"
    _launch(rule, kind, n, p, g, v, lr, step_dev, loss)
    gu = g0
    if kind == "sse":
        want = g0.double() / (CNT * (SSE / CNT) ** 0.5)
        _assert_close("scaled g", g[:n], want, 4 * ULP * want.abs() + 1e-38, ctx)
        lv, mse = float(loss[0]), float(loss[1])
        assert abs(lv - (SSE / CNT) ** 0.5) <= 2 * ULP * (SSE / CNT) ** 0.5 and abs(mse - SSE / CNT) <= ULP * SSE / CNT, ctx
        gu = g[:n].cpu()                                      # the update uses the scaled gradient
    _check_update(rule, ctx, p, v, p0, gu, v0, lr, cls)
    # the plain forms advance the count by one and leave the stamp; the carried form reads the words only; tickets at 0
    assert step_dev.tolist() == [k + 1, stamp, 0, 0], (ctx, step_dev.tolist())
    return p.cpu(), v.cpu()


@pytest.mark.parametrize("n", N_LIST)
@pytest.mark.parametrize("rule", RULES)
def test_update_launches_match_fp64_rule(H, rule, n):
    """hcg_update_dev, its SSE form and the update carried in hcg_step_tail: parameters and (RMSprop) square averages of every
    element vs the fp64 rule for two learning rates, with zero, underflowing and overflowing gradients; the step words
    as the contract says; and the plain and the carried update bitwise equal on the same gradient."""
    for i, lr in enumerate(LRS):
        seed = 31 * i + n % 991
        dev = _run_one(rule, "dev", n, lr, seed)
        _run_one(rule, "sse", n, lr, seed)
        tail = _run_one(rule, "tail", n, lr, seed)
        assert torch.equal(dev[0], tail[0]) and torch.equal(dev[1], tail[1]), (rule, n, lr)


# ----------------------------------------------------------------------------------------------------------------------
# model level: every update vs torch.optim.SGD / RMSprop from the same state, fed the same gradients
# ----------------------------------------------------------------------------------------------------------------------
def _model(rule, feat=64, seed=5):
    """A GCN with the factory's optimiser for `rule` (RMSprop's first steps move every weight by ~10 lr: lr 1e-3)."""
    import hcatgnet_amd as Hm
    torch.manual_seed(seed)
    lr = 1e-3 if rule == "rmsprop" else 0.01
    return Hm.make_network("GCN", Hm.default_options(optimizer=rule, lr=lr), feat).cuda()


def _state(model):
    """(p, square_avg or None, g) of every parameter, on the host."""
    opt, out = model.optimizer, []
    for q in model.parameters():
        st = opt.state.get(q, {})
        v = st["square_avg"].detach().cpu().clone() if "square_avg" in st else torch.zeros(q.shape)
        g = q.grad.detach().cpu().clone() if q.grad is not None else None
        out.append((q.detach().cpu().clone(), v, g))
    return out


def _bounds(rule, lr, p0, v0, g, rp):
    """Per-element bounds of one update vs torch's.  Besides rounding, they allow for torch's (1 - alpha) being rounded
    from the double 1 - 0.99 where the kernels compute 1 - float(0.99): 1.3e-6 relative in v's increment, half that in the
    update."""
    if rule == "SGD":
        upd = lr * g.double().abs()
        return 1e-6 * upd + 4e-7 * rp.abs() + 1e-12, None
    v_inc = (1 - ALPHA) * g.double() ** 2
    v1 = ALPHA * v0.double() + v_inc
    upd = lr * g.double().abs() / (v1.sqrt() + EPS)
    return 3e-6 * upd + 4e-7 * rp.abs() + 1e-12, 3e-6 * v1.abs() + 1e-30


def _torch_update(rule, lr, p0, v0, g, step):
    ref = torch.nn.Parameter(p0.clone())
    ref.grad = g.clone()
    if rule == "SGD":
        opt = torch.optim.SGD([ref], lr=lr, foreach=False)
    else:
        opt = torch.optim.RMSprop([ref], lr=lr, foreach=False)
        opt.state[ref] = dict(step=torch.tensor(float(step - 1)), square_avg=v0.clone())
    opt.step()
    return ref.detach(), (opt.state[ref]["square_avg"] if rule == "rmsprop" else None)


def _check_against_torch(rule, model, before, after, step, ctx):
    lr = model.optimizer.param_groups[0]["lr"]
    for i, ((p0, v0, _), (p1, v1, g)) in enumerate(zip(before, after)):
        rp, rv = _torch_update(rule, lr, p0, v0, g, step)
        tp, tv = _bounds(rule, lr, p0, v0, g, rp.double())
        c = f"{ctx} param {i}"
        _assert_close("p", p1, rp.double(), tp, c)
        if rule == "rmsprop":
            _assert_close("square_avg", v1, rv.double(), tv, c)


def _small_batches(count, ng, seed0):
    from hcatgnet_amd import synth
    return [synth.make_config("C2", num_graphs=ng, seed=seed0 + i).as_batch("cuda") for i in range(count)]


def _words(model):
    return model.optimizer._flat[0]["step_dev"].tolist()


@pytest.mark.parametrize("rule", RULES)
def test_carried_and_plain_updates_match_torch(H, rule):
    """FusedTrainStep with FusedSGD / FusedRMSprop: the update rides in the step's last launch (nothing after it), and every
    update -- carried, a plain `optimizer.step()` after an autograd backward, a combine="sse" step with an identity collective
    (`step_sse`) -- equals torch's from the same state on the same gradients.  The count is every update; the stamp rises
    with the carried steps only."""
    from hcatgnet_amd import train
    from hcatgnet_amd.train import FusedTrainStep
    model = _model(rule)
    batches = _small_batches(3, 24, 40)
    carried = FusedTrainStep(model)
    sse = FusedTrainStep(model, combine="sse", grad_sync=lambda ext: None)
    seq = ["carried"] * 4 + ["plain"] * 2 + ["sse"] * 2 + ["carried"] * 3
    count, stamp = 0, None
    for i, kind in enumerate(seq):
        b = batches[i % len(batches)]
        before = _state(model)
        if kind == "carried":
            carried(b)
            assert carried._last_carried, "the update must ride in the step's last launch"
        elif kind == "sse":
            sse(b)
        else:
            model.optimizer.zero_grad()
            train._rmse_autograd(model, b).backward()
            model.optimizer.step()
        count += 1
        _check_against_torch(rule, model, before, _state(model), count, f"{rule} update {i} ({kind})")
        w = _words(model)
        stamp = w[1] if stamp is None else stamp + (1 if kind == "carried" else 0)
        assert w[:3] == [count, stamp, 0], (i, kind, w)
    assert model.optimizer.steps_done() == len(seq)
    sd = model.optimizer.state_dict()
    if rule == "rmsprop":
        assert sd["state"][0]["step"].item() == len(seq)
    else:
        assert sd["state"] == {}


@pytest.mark.parametrize("rule", RULES)
def test_captured_step_and_window_equal_eager_steps(H, rule):
    """A captured step replayed k times is bitwise k eager steps; a StepWindow is bitwise its steps one by one."""
    from hcatgnet_amd import synth
    from hcatgnet_amd.train import FusedTrainStep, StepWindow
    sbs = [synth.make_config("C2", num_graphs=96, rank=r) for r in range(3)]
    dev = [(sb, sb.x.cuda(), sb.edge_index.cuda(), sb.batch.cuda(), sb.y.cuda()) for sb in sbs]
    fresh = [(lambda t=t: H.Batch(t[1], t[2], t[3], t[0].num_graphs, y=t[4], max_nodes=t[0].max_nodes,
                                  max_edges=t[0].max_edges, edges_grouped=True)) for t in dev]
    a, b, c = _model(rule), _model(rule), _model(rule)
    b.load_state_dict(a.state_dict())
    c.load_state_dict(a.state_dict())
    eager, graphed = FusedTrainStep(a), FusedTrainStep(b)
    graphed.capture(fresh[0])                                  # (two warm-up steps)
    la = [float(eager(fresh[0]())) for _ in range(2 + 4)]
    lb = [float(graphed.replay()) for _ in range(4)]
    assert lb == la[2:], (lb, la)
    assert a.optimizer.steps_done() == b.optimizer.steps_done() == 6
    for pa, pb in zip(a.parameters(), b.parameters()):
        assert torch.equal(pa, pb)
    sa = [FusedTrainStep(a) for _ in range(3)]
    sc = [FusedTrainStep(c) for _ in range(3)]
    for _ in range(6):                                         # c catches up with a
        sc[0](fresh[0]())
    win = StepWindow(sc, fresh)                                # its warm-up runs the three steps once
    la = [float(sa[i](fresh[i]())) for i in range(3)]
    lc = []
    for _ in range(2):
        la += [float(sa[i](fresh[i]())) for i in range(3)]
        lc += [float(v) for v in win.replay()]
    assert lc == la[3:], (lc, la[3:])
    assert a.optimizer.steps_done() == c.optimizer.steps_done() == 15
    for pa, pc in zip(a.parameters(), c.parameters()):
        assert torch.equal(pa, pc)
    if rule == "rmsprop":
        for q, r in zip(a.parameters(), c.parameters()):
            assert torch.equal(a.optimizer.state[q]["square_avg"], c.optimizer.state[r]["square_avg"])


@pytest.mark.parametrize("rule", RULES)
def test_epoch_window_equals_the_per_batch_loop_on_the_same_permutations(H, rule):
    """train_network over a shuffling DeviceLoader builds the one-graph epoch for SGD / RMSprop too; four epochs are bitwise
    the per-batch loop's on the same permutations, the capture's warm-up epoch is undone (square_avg included), and a new
    learning rate in param_groups reaches the replayed update."""
    from hcatgnet_amd import synth, train
    sb = synth.make_config("REAL", num_graphs=135)
    store = H.DeviceGraphStore(sb.as_graph_list(), device="cuda")
    a, b = _model(rule, feat=25), _model(rule, feat=25)
    b.load_state_dict(a.state_dict())
    la, lb = H.DeviceLoader(store, batch_size=40, shuffle=True, seed=11), H.DeviceLoader(store, batch_size=40, shuffle=True, seed=11)
    train.EPOCH_WINDOW = False
    try:                                                       # a state to undo: weights, square averages and a count
        assert train.train_network(a, la, "cuda") == train.train_network(b, lb, "cuda")
    finally:
        train.EPOCH_WINDOW = True
    fl = a.optimizer._flat[0]
    before = [t.clone() for t in [fl["p"]] + a.optimizer.flat_state(fl)]
    assert len(before) == (2 if rule == "rmsprop" else 1)
    win = train.epoch_window_of(a, la, build=True)
    assert win is not None, "the epoch window must apply to SGD / RMSprop"
    fl = a.optimizer._flat[0]
    for x, y in zip([fl["p"]] + a.optimizer.flat_state(fl), before):
        assert torch.equal(x, y)                               # the capture's warm-up epoch was undone
    assert a.optimizer.steps_done() == len(la)
    va = [train.train_network(a, la, "cuda") for _ in range(4)]
    assert train.epoch_window_of(a, la) is win
    train.EPOCH_WINDOW = False
    try:
        vb = [train.train_network(b, lb, "cuda") for _ in range(4)]
    finally:
        train.EPOCH_WINDOW = True
    assert va == vb, (va, vb)
    for q, r in zip(a.parameters(), b.parameters()):
        assert torch.equal(q, r)
    if rule == "rmsprop":
        for q, r in zip(a.parameters(), b.parameters()):
            assert torch.equal(a.optimizer.state[q]["square_avg"], b.optimizer.state[r]["square_avg"])
    assert a.optimizer.steps_done() == b.optimizer.steps_done() == 5 * len(la)
    for g in a.optimizer.param_groups + b.optimizer.param_groups:
        g["lr"] = g["lr"] * 0.3
    va2 = train.train_network(a, la, "cuda")
    train.EPOCH_WINDOW = False
    try:
        vb2 = train.train_network(b, lb, "cuda")
    finally:
        train.EPOCH_WINDOW = True
    assert va2 == vb2
    for q, r in zip(a.parameters(), b.parameters()):
        assert torch.equal(q, r)


def test_concurrent_runs_of_mixed_rules_equal_the_runs_one_by_one(H):
    """train_networks over Adam, SGD and RMSprop runs: every run's epoch is its own one-graph epoch, and each run is bitwise
    what train_network gives it alone."""
    from hcatgnet_amd import synth
    from hcatgnet_amd.train import epoch_window_of, train_network, train_networks
    rules = ["Adam", "SGD", "rmsprop"]
    sizes = [135, 100, 121]

    def make(k):
        sb = synth.make_config("REAL", num_graphs=sizes[k], seed=synth.BASE_SEED + 7 * k)
        store = H.DeviceGraphStore(sb.as_graph_list(), device="cuda")
        torch.manual_seed(100 + k)
        lr = 1e-3 if rules[k] == "rmsprop" else 0.01
        m = H.make_network("GCN", H.default_options(optimizer=rules[k], lr=lr), 25).cuda()
        return m, H.DeviceLoader(store, batch_size=40, shuffle=True, seed=20 + k)
    together, alone = [make(k) for k in range(3)], [make(k) for k in range(3)]
    for (ma, _), (mb, _) in zip(together, alone):
        mb.load_state_dict(ma.state_dict())
    for _ in range(3):
        tv = train_networks([r[0] for r in together], [r[1] for r in together], "cuda")
        for k, (m, trn) in enumerate(alone):
            assert tv[k] == train_network(m, trn, "cuda"), (rules[k], tv[k])
    for k, ((ma, ta), (mb, tb)) in enumerate(zip(together, alone)):
        assert epoch_window_of(ma, ta) is not None, rules[k]     # the one-graph form ran
        for q, r in zip(ma.parameters(), mb.parameters()):
            assert torch.equal(q, r), rules[k]


class _RecordingLoader:
    """A host-side loader over fixed device batches that records the model's state around every step train_network takes."""

    def __init__(self, model, batches):
        self.model, self.batches, self.log = model, batches, []
        self.dataset = [None] * sum(b.num_graphs for b in batches)

    def __iter__(self):
        for b in self.batches:
            torch.cuda.synchronize()
            self.log.append(_state(self.model))
            yield b
        torch.cuda.synchronize()
        self.log.append(_state(self.model))


def test_rmsprop_train_network_with_a_refused_batch(H):
    """train_network over epochs of fused steps and one batch the fused step refuses (autograd + `optimizer.step()`): carried
    and plain RMSprop updates interleave; every update equals torch's on that step's gradients, steps_done counts all of
    them, and the plain updates leave the exchange stamp where the carried steps put it."""
    from hcatgnet_amd import train
    model = _model("rmsprop", seed=9)
    fused = _small_batches(5, 8, 70)
    odd = fused[0]
    refused = H.Batch(odd.x, odd.edge_index, odd.batch, odd.num_graphs, y=odd.y)
    assert train.FusedTrainStep(model, optimizer_step=False).reason(refused) is not None
    batches = [fused[i % len(fused)] for i in range(6)] + [refused]
    count, stamps = 0, []
    for epoch in range(3):
        loader = _RecordingLoader(model, batches)
        assert train.train_network(model, loader, "cuda") > 0
        for i in range(len(batches)):
            count += 1
            _check_against_torch("rmsprop", model, loader.log[i], loader.log[i + 1], count, f"epoch {epoch} batch {i}")
        assert model.optimizer.steps_done() == count
        w = _words(model)
        assert w[2] == 0, w
        stamps.append(w[1])
    assert [b - a for a, b in zip(stamps, stamps[1:])] == [6, 6], stamps        # one per carried step, none per plain one
    assert model.optimizer.state_dict()["state"][0]["step"].item() == 3 * len(batches)


def test_rmsprop_state_dict_moves_to_torch_and_trains_on(H):
    """k fused steps, `state_dict()` loaded into a fresh torch.optim.RMSprop on a copy of the model; both train on with the
    same gradients and stay within the per-step bounds of torch's update, accumulated over the steps since the hand-over."""
    from hcatgnet_amd.train import FusedTrainStep
    a = _model("rmsprop")
    batches = _small_batches(3, 24, 50)
    step = FusedTrainStep(a)
    for i in range(5):
        step(batches[i % 3])
    b = _model("rmsprop", seed=77)
    b.load_state_dict(a.state_dict())
    tb = torch.optim.RMSprop(b.parameters(), lr=a.optimizer.param_groups[0]["lr"])
    tb.load_state_dict(copy.deepcopy(a.optimizer.state_dict()))
    assert all(float(tb.state[q]["step"]) == 5 for q in b.parameters())
    lr = a.optimizer.param_groups[0]["lr"]
    acc = None
    for i in range(4):
        before = _state(a)
        step(batches[i % 3])
        after = _state(a)
        for q, (_, _, g) in zip(b.parameters(), after):
            q.grad = g.cuda()
        tb.step()
        tols = [_bounds("rmsprop", lr, p0, v0, g, p1.double()) for (p0, v0, _), (p1, _, g) in zip(before, after)]
        acc = tols if acc is None else [(x[0] + y[0], x[1] + y[1]) for x, y in zip(acc, tols)]
        for k, (q, (p1, v1, _), (tp, tv)) in enumerate(zip(b.parameters(), after, acc)):
            _assert_close("p", q.detach(), p1.double(), tp, f"step {i} param {k}")
            _assert_close("square_avg", tb.state[q]["square_avg"], v1.double(), tv, f"step {i} param {k}")
    assert a.optimizer.steps_done() == 9 and all(float(tb.state[q]["step"]) == 9 for q in b.parameters())


@pytest.mark.parametrize("combine", ["mean", "sse"])
@pytest.mark.parametrize("rule", RULES)
def test_rccl_forms_world1_match_the_single_process_step(H, rule, combine):
    """RCCL at world size 1, collective forced: the eager data-parallel step (backward -> all-reduce -> the plain update, or
    the "sse" form's one scale + update launch) equals the plain single-process step; the one-shot exchange refuses the
    rule."""
    import os
    import torch.distributed as dist
    from hcatgnet_amd import synth
    from hcatgnet_amd.ddp import DataParallelGCN
    from hcatgnet_amd.train import FusedTrainStep
    from hcatgnet_amd.xgmi import OneShotExchange
    from tests.helpers import rel_inf
    created = False
    if not dist.is_initialized():
        os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
        os.environ.setdefault("MASTER_PORT", "29541")
        dist.init_process_group("nccl", rank=0, world_size=1, device_id=torch.device("cuda", torch.cuda.current_device()))
        created = True
    try:
        sb = synth.make_config("C2", num_graphs=256)
        x, ei, bv, y = sb.x.cuda(), sb.edge_index.cuda(), sb.batch.cuda(), sb.y.cuda()
        fresh = lambda: H.Batch(x, ei, bv, sb.num_graphs, y=y, max_nodes=sb.max_nodes, max_edges=sb.max_edges, edges_grouped=True)
        ma, mb = _model(rule), _model(rule)
        mb.load_state_dict(ma.state_dict())
        plain = FusedTrainStep(ma)
        dp = DataParallelGCN(mb, force_collective=True, combine=combine)
        eager = dp.make_train_step()
        la = [float(plain(fresh())) for _ in range(3)]
        lb = [float(eager(fresh())) for _ in range(3)]
        for u, v in zip(la, lb):
            assert abs(u - v) <= 1e-6 * abs(u), (la, lb)
        for pa, pb in zip(ma.parameters(), mb.parameters()):
            assert rel_inf(pb, pa) <= 1e-6
        assert ma.optimizer.steps_done() == mb.optimizer.steps_done() == 3
        xchg = OneShotExchange.__new__(OneShotExchange)       # (the rule gate comes before any use of the exchange)
        xchg.ok, xchg.n = True, sum(q.numel() for q in mb.parameters())
        with pytest.raises(ValueError, match="RCCL"):
            xchg.attach(eager)
        assert eager.exchange is None
    finally:
        if created:
            dist.destroy_process_group()
