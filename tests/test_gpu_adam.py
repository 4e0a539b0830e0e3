"""GPU parity of every Adam update path (csrc/optim.hip, FusedAdam) against a plain evaluation of torch's rule

    m = b1 m + (1-b1) g ;  v = b2 v + (1-b2) g^2 ;  p -= lr/(1-b1^t) * m / (sqrt(v)/sqrt(1-b2^t) + eps)

element by element.  The launches are checked in fp64 with the float32 hyper-parameters the C ABI receives, to a few
float32 ulp: a step count off by one at t ~ 1000 moves sqrt(1 - b2^t) by ~6e-4, thousands of ulp.  The model-level tests mix
the two ways an update happens on one optimiser -- carried in the step's last launch (hcg_step_tail, the head advances
step_dev[0] and the exchange stamp step_dev[1]) and the plain capturable update (hcg_adam_step_dev[_sse], whose ticket is
step_dev[2]) -- and check every update against torch.optim.Adam fed the same gradients."""
import pytest
import torch

from tests.test_gpu_parity import H  # noqa: F401  (fixture)

pytestmark = pytest.mark.gpu

ULP = 2.0 ** -23                     # float32 spacing at 1
B1, B2 = 0.9, 0.999
F32 = lambda x: float(torch.tensor(x, dtype=torch.float32))     # the float the C ABI receives

N_LIST = [1, 255, 256, 257, 16641, 14145, (1 << 22) + 3]          # 16641 / 14145: the default model (F = 64) / F = 25
K_LIST = [0, 1, 9, 999, 100000]                                   # updates done before this one; 100000: corrections ~1
HPARAMS = [(0.01, 1e-9), (0.01, 1e-8), (1e-4, 1e-9), (1e-4, 1e-8)]
ZERO, TINY, HUGE = 0, 1, 2            # gradient classes (the rest are normal values)


def _grid(n):
    return (n + 255) // 256           # workgroups of the update launch (256 threads each)


def _inputs(n, lr, seed):
    """Parameters, gradients and moments of n elements: mostly normal values, plus exact zeros (with zero moments: v stays 0),
    tiny gradients whose square underflows (zero moments) and huge ones whose square overflows float32."""
    g = torch.Generator().manual_seed(seed)
    cls = (torch.arange(n) * 7 + 3) % 16
    grad = torch.randn(n, generator=g)
    m = torch.randn(n, generator=g) * 0.1
    v = torch.rand(n, generator=g) * 0.01 + 1e-6
    p = torch.randn(n, generator=g) * (4 * lr)          # |p| ~ |update|: the update is not lost in p's rounding
    sign = torch.where(torch.rand(n, generator=g) < 0.5, -1.0, 1.0)
    grad[cls == ZERO] = 0.0
    grad[cls == TINY] = 1e-30 * sign[cls == TINY]
    grad[cls == HUGE] = 1e30 * sign[cls == HUGE]
    m[(cls == ZERO) | (cls == TINY)] = 0.0
    v[(cls == ZERO) | (cls == TINY)] = 0.0
    return p, grad, m, v, cls


def _reference(p, g, m, v, t, lr, eps):
    """fp64 evaluation of the rule with the float32 hyper-parameters -> (p, m, v, per-element bounds for p, m, v)."""
    b1, b2, lr, eps = F32(B1), F32(B2), F32(lr), F32(eps)
    p, g, m, v = (x.double() for x in (p, g, m, v))
    m2 = b1 * m + (1 - b1) * g
    v2 = b2 * v + (1 - b2) * g * g
    bc1, bc2s = 1 - b1 ** t, (1 - b2 ** t) ** 0.5
    denom = v2.sqrt() / bc2s + eps
    step = lr / bc1
    p2 = p - step * m2 / denom
    m_abs = b1 * m.abs() + (1 - b1) * g.abs()           # what m's rounding errors scale with (m itself may cancel)
    upd_abs = step * m_abs / denom
    tol_p = 8 * ULP * upd_abs + ULP * p2.abs() + 1e-30
    tol_m = 2 * ULP * m_abs + 1e-38
    tol_v = 3 * ULP * v2.abs() + 1e-38
    return p2, m2, v2, tol_p, tol_m, tol_v


def _assert_close(name, got, want, tol, ctx):
    got, want, tol = got.detach().double().cpu().reshape(-1), want.reshape(-1), tol.reshape(-1)
    bad = ~((got - want).abs() <= tol)
    if bool(bad.any()):
        i = int(bad.nonzero()[0])
        raise AssertionError(f"{ctx}: {name}: {int(bad.sum())} of {got.numel()} elements off, first [{i}] got {got[i].item()!r} "
                             f"want {want[i].item()!r} (tol {tol[i].item():.3g})")


def _check_update(ctx, out, inp, t, lr, eps, cls):
    """`out` = (p, m, v) after the launch, `inp` = (p, g, m, v) before it (g = the gradient the update used)."""
    p0, g0, m0, v0 = inp
    p2, m2, v2, tp, tm, tv = _reference(p0, g0, m0, v0, t, lr, eps)
    p, m, v = (x.cpu() for x in out)
    huge = cls == HUGE
    # g^2 overflows: float32's rule gives v = inf, m / inf = 0, p unchanged (torch.optim.Adam below); fp64 has no overflow
    ref = torch.nn.Parameter(p0[huge].clone())
    ref.grad = g0[huge].clone()
    opt = torch.optim.Adam([ref], lr=lr, betas=(B1, B2), eps=eps, foreach=False)
    opt.state[ref] = dict(step=torch.tensor(float(t - 1)), exp_avg=m0[huge].clone(), exp_avg_sq=v0[huge].clone())
    opt.step()
    assert torch.equal(p[huge], ref.detach()), ctx
    assert bool(torch.isinf(v[huge]).all()) and bool(torch.isinf(opt.state[ref]["exp_avg_sq"]).all()), ctx
    keep = ~huge
    _assert_close("p", p[keep], p2[keep], tp[keep], ctx)
    _assert_close("m", m, m2, tm, ctx)
    _assert_close("v", v[keep], v2[keep], tv[keep], ctx)
    # tiny gradients: their square underflows, v stays exactly 0 (as in float32 torch)
    assert bool((v[cls == TINY] == 0).all()) and bool((v[cls == ZERO] == 0).all()), ctx
    assert torch.equal(p[cls == ZERO], p0[cls == ZERO]), ctx


def _launch(lib, kind, n, p, g, m, v, lr, eps, k, step_dev=None, loss=None):
    from hcatgnet_amd import _lib
    P, s = _lib.ptr, _lib.stream_ptr()
    b1, b2 = B1, B2
    if kind == "host":
        rc = lib.hcg_adam_step(P(p), P(g), P(m), P(v), n, lr, b1, b2, eps, k + 1, s)     # step = this update's number
    else:
        lr_dev = torch.tensor([lr], dtype=torch.float32, device="cuda")
        if kind == "dev":
            rc = lib.hcg_adam_step_dev(P(p), P(g), P(m), P(v), n, P(lr_dev), b1, b2, eps, P(step_dev), s)
        else:
            rc = lib.hcg_adam_step_dev_sse(P(p), P(g), P(m), P(v), n, P(lr_dev), b1, b2, eps, P(step_dev), P(loss), s)
    _lib.check(rc, f"adam {kind}")
    torch.cuda.synchronize()


SSE, CNT = 160.0, 40.0               # the SSE form's [SSE, count] tail: sqrt(MSE) = 2, gradient scale 1 / 80


def _run_one(lib, kind, n, k, lr, eps, seed, stamp=0, repeats=1):
    """`repeats` consecutive launches from step count k (the same gradient each time); every element of every update
    checked."""
    p0, g0, m0, v0, cls = _inputs(n, lr, seed)
    p, m, v = p0.cuda(), m0.cuda(), v0.cuda()
    step_dev = torch.tensor([k, stamp, 0, 0], dtype=torch.int32, device="cuda")
    loss = torch.full((2,), -1.0, device="cuda")
    for r in range(repeats):
        ctx = f"{kind} n={n} k={k} lr={lr} eps={eps} stamp={stamp} launch {r}"
        t = k + 1 + r
        g = g0
        if kind == "sse":
            flat = torch.cat([g, torch.tensor([SSE, CNT])]).cuda()
        else:
            flat = g.cuda()
        before = (p.cpu(), g, m.cpu(), v.cpu())
        _launch(lib, kind, n, p, flat, m, v, lr, eps, k + r, step_dev, loss)
        if kind == "sse":
            # the gradient of sqrt(MSE): scaled in place by 1 / (count * sqrt(SSE / count)); the loss pair
            want = g.double() / (CNT * (SSE / CNT) ** 0.5)
            _assert_close("scaled g", flat[:n], want, 4 * ULP * want.abs() + 1e-38, ctx)
            assert torch.equal(flat[n:].cpu(), torch.tensor([SSE, CNT])), ctx
            lv, mse = float(loss[0]), float(loss[1])
            assert abs(lv - (SSE / CNT) ** 0.5) <= 2 * ULP * (SSE / CNT) ** 0.5 and abs(mse - SSE / CNT) <= ULP * SSE / CNT, ctx
            before = (before[0], flat[:n].cpu(), before[2], before[3])     # the update uses the scaled gradient
        _check_update(ctx, (p, m, v), before, t, lr, eps, cls)
        if kind != "host":
            words = step_dev.tolist()
            assert words == [t, stamp, 0, 0], f"{ctx}: step_dev {words}, want [count {t}, stamp {stamp}, ticket 0, 0]"


@pytest.mark.parametrize("n", N_LIST)
@pytest.mark.parametrize("kind", ["host", "dev", "sse"])
def test_adam_launch_matches_fp64_rule(H, kind, n):
    """hcg_adam_step (host step count), hcg_adam_step_dev and hcg_adam_step_dev_sse: parameters and both moments of every
    element after one update vs the fp64 rule, for update numbers 1, 2, 10, 1000 and 100001 and two learning rates and two
    eps; with zero, underflowing and overflowing gradients.  The SSE form also scales the gradient in place and stores the
    loss pair; the device forms advance step_dev[0] by one and leave the stamp alone."""
    from hcatgnet_amd import _lib
    lib = _lib.load()
    for ki, k in enumerate(K_LIST):
        for hi, (lr, eps) in enumerate(HPARAMS):
            _run_one(lib, kind, n, k, lr, eps, seed=1000 * ki + 10 * hi + n % 997)


STAMPS = {"0": lambda g: 0, "1": lambda g: 1, "grid-2": lambda g: g - 2, "grid-1": lambda g: g - 1, "grid": lambda g: g,
          "grid+1": lambda g: g + 1, "12345": lambda g: 12345}


@pytest.mark.parametrize("stamp", list(STAMPS))
@pytest.mark.parametrize("n", [16641, (1 << 22) + 3])
@pytest.mark.parametrize("kind", ["dev", "sse"])
def test_plain_update_keeps_the_step_words(H, kind, n, stamp):
    """The device-side update starting from step_dev = [k, s] with any exchange stamp s -- also one at or past the launch's
    workgroup count, which carried steps reach in a few dozen steps: every element is updated with t = k + 1, the count
    becomes k + 1, the stamp stays s (a plain update exchanges nothing) and the ticket word is back at 0, so a second launch
    right behind it uses t = k + 2."""
    from hcatgnet_amd import _lib
    lib = _lib.load()
    s = STAMPS[stamp](_grid(n))
    _run_one(lib, kind, n, 999, 0.01, 1e-9, seed=17 + s, stamp=s, repeats=2)


# ----------------------------------------------------------------------------------------------------------------------
# model level: carried and plain updates on one optimiser, each update vs torch.optim.Adam fed the same gradients
# ----------------------------------------------------------------------------------------------------------------------
def _state(model):
    """(p, m, v, g) of every parameter, on the host."""
    opt, out = model.optimizer, []
    for q in model.parameters():
        st = opt.state.get(q, {})
        m = st["exp_avg"].detach().cpu().clone() if "exp_avg" in st else torch.zeros(q.shape)
        v = st["exp_avg_sq"].detach().cpu().clone() if "exp_avg_sq" in st else torch.zeros(q.shape)
        g = q.grad.detach().cpu().clone() if q.grad is not None else None
        out.append((q.detach().cpu().clone(), m, v, g))
    return out


def _words(model):
    return model.optimizer._flat[0]["step_dev"].tolist()


def _check_against_torch(model, before, after, t, ctx):
    """One update `before` -> `after` (the gradients are those in `after`) vs torch.optim.Adam from the same state with
    t - 1 updates done.  Besides rounding, the bounds allow for torch's scalars being rounded from doubles where the kernels
    compute with float betas: 1 - beta2 = 0.001 against 1 - float(0.999) (1.3e-5 relative in v's increment, ~1e-5 in the
    update), and m's weights 0.1 / 0.9 against 1 - float(0.9) / float(0.9) (2.4e-7 of |b1 m| + |(1-b1) g|, which is all of
    m where the two terms cancel).  A step number off by one moves an update by 0.7 % at t = 70, 12 % at t = 4."""
    grp = model.optimizer.param_groups[0]
    (b1, b2), lr, eps = grp["betas"], grp["lr"], grp["eps"]
    for i, ((p0, m0, v0, _), (p1, m1, v1, g)) in enumerate(zip(before, after)):
        ref = torch.nn.Parameter(p0.clone())
        ref.grad = g.clone()
        opt = torch.optim.Adam([ref], lr=lr, betas=(b1, b2), eps=eps, foreach=False)
        opt.state[ref] = dict(step=torch.tensor(float(t - 1)), exp_avg=m0.clone(), exp_avg_sq=v0.clone())
        opt.step()
        rm, rv = opt.state[ref]["exp_avg"].double(), opt.state[ref]["exp_avg_sq"].double()
        rp = ref.detach().double()
        m_abs = b1 * m0.double().abs() + (1 - b1) * g.double().abs()
        upd_abs = lr / (1 - b1 ** t) * m_abs / (rv.sqrt() / (1 - b2 ** t) ** 0.5 + eps)
        c = f"{ctx} param {i}"
        _assert_close("p", p1, rp, 3e-5 * (rp - p0.double()).abs() + 1e-6 * upd_abs + 4e-7 * rp.abs() + 1e-12, c)
        _assert_close("m", m1, rm, 1e-6 * m_abs + 1e-30, c)
        _assert_close("v", v1, rv, 2e-5 * rv.abs() + 1e-30, c)


def _small_batches(count, ng, seed0):
    from hcatgnet_amd import synth
    return [synth.make_config("C2", num_graphs=ng, seed=seed0 + i).as_batch("cuda") for i in range(count)]


def _plain_update(model, batch):
    """train_network's fallback for a batch the fused step refuses: autograd, then `optimizer.step()`."""
    from hcatgnet_amd import train
    model.optimizer.zero_grad()
    loss = train._rmse_autograd(model, batch)
    loss.backward()
    model.optimizer.step()


@pytest.mark.parametrize("N", [3, 70])
@pytest.mark.parametrize("plain", ["step", "step_sse"])
def test_carried_then_plain_then_carried_updates(H, N, plain):
    """N carried steps (FusedTrainStep: Adam in the step's last launch), then plain updates -- autograd +
    `optimizer.step()` as train_network does for a refused batch, or a combine="sse" trainer with an identity collective
    (FusedAdam.step_sse) -- then 3 more carried steps.  N = 70 is past the 66 workgroups of the 64-wide model's update.
    Every update equals torch.optim.Adam's with the right step number, the count is N + plain + 3 (steps_done and
    state_dict), and the exchange stamp rises by one per carried step and not at all on a plain update."""
    from hcatgnet_amd.train import FusedTrainStep
    torch.manual_seed(5)
    model = H.make_network("GCN", H.default_options(), 64).cuda()
    batches = _small_batches(3, 24, 40)
    carried = FusedTrainStep(model)
    sse = FusedTrainStep(model, combine="sse", grad_sync=lambda ext: None) if plain == "step_sse" else None
    n_plain = 2
    seq = ["carried"] * N + ["plain"] * n_plain + ["carried"] * 3
    count, stamp = 0, None
    for i, kind in enumerate(seq):
        b = batches[i % len(batches)]
        before = _state(model)
        if kind == "carried":
            carried(b)
        elif sse is not None:
            sse(b)
        else:
            _plain_update(model, b)
        count += 1
        after = _state(model)
        _check_against_torch(model, before, after, count, f"update {i} ({kind})")
        w = _words(model)
        stamp = w[1] if stamp is None else stamp + (1 if kind == "carried" else 0)
        assert w[:3] == [count, stamp, 0], (i, kind, w)
    assert model.optimizer.steps_done() == len(seq)
    assert model.optimizer.state_dict()["state"][0]["step"].item() == len(seq)


class _RecordingLoader:
    """A host-side loader over fixed device batches (iterable, with `.dataset`) that records the model's parameters, moments
    and gradients between the batches, i.e. around every step train_network takes."""

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


def test_train_network_with_a_refused_batch(H):
    """train.train_network over a loader whose epochs are 70 fused steps and one batch the fused step refuses (no collate
    metadata: the autograd path and `optimizer.step()`), three epochs: every update equals torch.optim.Adam's on that step's
    gradients with the right step number, and the count is the number of batches seen."""
    from hcatgnet_amd import train
    torch.manual_seed(9)
    model = H.make_network("GCN", H.default_options(), 64).cuda()
    fused = _small_batches(5, 8, 70)
    odd = fused[0]
    refused = H.Batch(odd.x, odd.edge_index, odd.batch, odd.num_graphs, y=odd.y)
    assert train.FusedTrainStep(model, optimizer_step=False).reason(refused) is not None
    batches = [fused[i % len(fused)] for i in range(70)] + [refused]
    count = 0
    for epoch in range(3):
        loader = _RecordingLoader(model, batches)
        val = train.train_network(model, loader, "cuda")
        assert val > 0
        assert len(loader.log) == len(batches) + 1
        for i in range(len(batches)):
            count += 1
            _check_against_torch(model, loader.log[i], loader.log[i + 1], count, f"epoch {epoch} batch {i}")
        assert model.optimizer.steps_done() == count
    assert model.optimizer.state_dict()["state"][0]["step"].item() == 3 * len(batches)


# ----------------------------------------------------------------------------------------------------------------------
# EpochWindow: a capture that fails after the warm-up epoch leaves the model as it was
# ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("error", ["HcgError", "RuntimeError"])
def test_epoch_window_failed_capture_undoes_its_warm_up(H, monkeypatch, error):
    """EpochWindow's capture runs one hidden warm-up epoch first.  When the capture itself then fails, `build` returns None
    and parameters, both moments and the step count are bitwise what they were; the next train_network epoch (which falls
    back to the per-batch loop) equals that of a twin trained with EPOCH_WINDOW off throughout."""
    from hcatgnet_amd import _lib, synth, train
    sb = synth.make_config("C2", num_graphs=100)
    store = H.DeviceGraphStore(sb.as_graph_list(), device="cuda")
    a = H.make_network("GCN", H.default_options(), 64).cuda()
    b = H.make_network("GCN", H.default_options(), 64).cuda()
    b.load_state_dict(a.state_dict())
    la = H.DeviceLoader(store, batch_size=32, shuffle=True, seed=4)
    lb = H.DeviceLoader(store, batch_size=32, shuffle=True, seed=4)
    train.EPOCH_WINDOW = False
    try:
        assert train.train_network(a, la, "cuda") == train.train_network(b, lb, "cuda")     # moments and a count to keep
    finally:
        train.EPOCH_WINDOW = True
    exc = _lib.HcgError if error == "HcgError" else RuntimeError

    def failing_graph(*args, **kwargs):
        raise exc("capture refused")
    monkeypatch.setattr(torch.cuda, "graph", failing_graph)
    before = [x.clone() for x in (a.optimizer._flat[0][k] for k in ("p", "m", "v"))]
    steps = a.optimizer.steps_done()
    assert train.EpochWindow.build(a, la) is None
    fl = a.optimizer._flat[0]
    for name, x, y in zip("pmv", (fl["p"], fl["m"], fl["v"]), before):
        assert torch.equal(x, y), name
    assert a.optimizer.steps_done() == steps == len(la)
    va = train.train_network(a, la, "cuda")             # the window fails again here: the per-batch loop runs
    monkeypatch.undo()
    train.EPOCH_WINDOW = False
    try:
        vb = train.train_network(b, lb, "cuda")
    finally:
        train.EPOCH_WINDOW = True
    assert va == vb
    for q, r in zip(a.parameters(), b.parameters()):
        assert torch.equal(q, r)
    assert a.optimizer.steps_done() == b.optimizer.steps_done() == 2 * len(la)
