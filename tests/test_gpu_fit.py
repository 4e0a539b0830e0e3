"""GPU tests of the device-side fit (hcatgnet_amd/fit.py, csrc/fit.hip): the controller kernel alone against `FitControl`
after every launch, whole fits against the loop of examples/train_like_reference.py written out here with torch's own
scheduler and `deepcopy`, the host-form fallback, several fits at once.  Every comparison is bitwise: the same kernels run
in the same order, and the controller's float64 arithmetic is the host's."""
from copy import deepcopy

import numpy as np
import pytest
import torch

import hcatgnet_amd as H
from hcatgnet_amd import _lib, synth
from hcatgnet_amd.fit import FitControl, fit_network, fit_networks
from hcatgnet_amd.train import epoch_window_of, eval_network, train_network
from tests import fit_ref

pytestmark = pytest.mark.gpu
INF = float("inf")


def _same(a, b):
    return a == b or (a != a and b != b)


# ---------------------------------------------------------------------------------------------------------------
# the kernel alone
# ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [16641, 1, 16643])
def test_controller_kernel_follows_fit_control_launch_by_launch(n):
    """Every crafted and seeded loss sequence written into device scalars, one launch per epoch, parameters = a pattern that
    encodes the epoch: after EVERY launch the device state, the optimiser's lr word (== float32(lr)), the log and the best
    slot are those of `FitControl`; launches after the stop, and after `max_epochs` rows, change nothing.  n = 16 641 (the
    reference model: 4 160 float4 and one scalar), 1 (tail only), 16 643 (a three-element tail)."""
    dev = torch.device("cuda")
    base = torch.arange(n, dtype=torch.float32, device=dev) * 0.25
    stopped_with_rows_left = 0
    for name, (cfg, rows) in sorted(fit_ref.all_sequences().items()):
        denom = (1.0, 1.0, 1.0) if not name.startswith("seeded") else (535.0, 60.0, 61.0)
        E = len(rows)
        init = _lib.FitState()
        init.lr, init.sched_best, init.val_best = cfg["lr"], INF, INF
        state = torch.frombuffer(bytearray(bytes(init)), dtype=torch.uint8).to(dev)
        sums = torch.zeros(3, dtype=torch.float64, device=dev)
        lr_dev = torch.tensor([cfg["lr"]], dtype=torch.float32, device=dev)
        param, log = base - 1.0, torch.full((E, 4), -7.0, dtype=torch.float64, device=dev)
        best = param.clone()
        a = _lib.FitControlArgs()
        for k in range(3):
            a.sums[k], a.denom[k] = sums[k:].data_ptr(), denom[k]
        a.state, a.lr_dev, a.param, a.best, a.n, a.log = state.data_ptr(), lr_dev.data_ptr(), param.data_ptr(), best.data_ptr(), n, log.data_ptr()
        a.factor, a.rel_epsilon, a.min_lr, a.eps = cfg["factor"], 1.0 - cfg["threshold"], cfg["min_lr"], cfg["eps"]
        a.patience, a.cooldown, a.control_every, a.early_stopping, a.max_epochs = (cfg["patience"], cfg["cooldown"], cfg["control_every"],
                                                                                  cfg["early_stopping"], E)
        fc = fit_ref.make_control(FitControl, cfg, E)
        want_log, want_best = np.full((E, 4), -7.0), -1.0
        for e, row in enumerate(rows + [(0.1, 0.0, 0.1)] * 2):          # (two launches past max_epochs: a loss that would be best)
            s = [row[k] * denom[k] for k in range(3)]
            param.copy_(base + float(e))
            sums.copy_(torch.tensor(s, dtype=torch.float64))
            _lib.fit_control(a)
            torch.cuda.synchronize()
            snap = fc.step(*[s[k] / denom[k] for k in range(3)])
            if snap is not None:
                want_log[e] = fc.log[-1]
            if snap:
                want_best = float(e)
            got = _lib.FitState.from_buffer_copy(state.cpu().numpy().tobytes())
            for k, v in fc.state().items():
                assert _same(getattr(got, k), v), (name, e, k, getattr(got, k), v)
            assert lr_dev.cpu().numpy()[0] == np.float32(fc.lr), (name, e)
            assert np.array_equal(log.cpu().numpy(), want_log, equal_nan=True), (name, e)
            assert torch.equal(best, base + want_best), (name, e, want_best)
        stopped_with_rows_left += int(fc.stopped and fc.epochs_counted < E)
    assert stopped_with_rows_left >= 2          # (some sequences did go on launching after the stop)


# ---------------------------------------------------------------------------------------------------------------
# whole fits
# ---------------------------------------------------------------------------------------------------------------
def _setup(n_train, n_val=12, data_seed=0, loader_seed=5, classes=None, host_train=False, val_from_train=False, **opts):
    """-> make(): a fresh (model, train, validation, test loader) on the same graphs, weights and seeds every call."""
    ng = n_train + 2 * n_val
    sb = synth.make_config("REAL", num_graphs=ng, seed=synth.BASE_SEED + data_seed)
    if classes:
        sb.y = torch.randint(0, classes, (ng,), generator=torch.Generator().manual_seed(data_seed + 1)).float()
        opts.update(problem_type="classification", n_classes=classes)
    graphs = sb.as_graph_list()
    stores = [H.DeviceGraphStore(g, device="cuda") for g in (graphs[:n_train], graphs[:n_val] if val_from_train else
                                                               graphs[n_train:n_train + n_val], graphs[n_train + n_val:])]

    def make():
        model = H.make_network("GCN", H.default_options(**opts), 25).cuda()      # (seeded at construction: equal weights)
        trn = (H.DataLoader(graphs[:n_train], batch_size=40, shuffle=False) if host_train
               else H.DeviceLoader(stores[0], batch_size=40, shuffle=True, seed=loader_seed))
        return model, trn, H.DeviceLoader(stores[1], batch_size=40), H.DeviceLoader(stores[2], batch_size=40)
    return make


def _host_loop(model, trn, val, tst, epochs, early_stopping, control_every):
    """The epoch loop of examples/train_like_reference.py with the control interval as a parameter."""
    val_best, best_epoch, stall, best_params, log = INF, 0, 0, deepcopy(model.state_dict()), []
    for epoch in range(epochs):
        if stall > early_stopping:
            break
        train_loss = train_network(model, trn, "cuda")
        val_loss = eval_network(model, val, "cuda")
        test_loss = eval_network(model, tst, "cuda")
        if epoch % control_every == 0:
            model.scheduler.step(val_loss)
            if val_loss < val_best:
                val_best, best_epoch, stall = val_loss, epoch, 0
                best_params = deepcopy(model.state_dict())
            else:
                stall += 1
        log.append((train_loss, val_loss, test_loss, float(model.optimizer.param_groups[0]["lr"])))
    torch.cuda.synchronize()
    return dict(log=np.array(log, dtype=np.float64), epochs_run=len(log), best_epoch=best_epoch, best_val=val_best,
                best_state=best_params, stopped=stall > early_stopping)


def _assert_result(res, ref, what):
    assert np.array_equal(res.log, ref["log"]), (what, res.log, ref["log"])
    assert (res.epochs_run, res.best_epoch, res.best_val, res.stopped_early) == (
        ref["epochs_run"], ref["best_epoch"], ref["best_val"], ref["stopped"]), what
    assert list(res.best_state) == list(ref["best_state"]), what
    for k, v in ref["best_state"].items():
        assert torch.equal(res.best_state[k], v), (what, k)


def _assert_same_opt(a, b, what):
    sa, sb = a.state_dict(), b.state_dict()
    assert sa["param_groups"] == sb["param_groups"], what
    assert sa["state"].keys() == sb["state"].keys(), what
    for k, st in sa["state"].items():
        for name, v in st.items():
            w = sb["state"][k][name]
            assert torch.equal(v, w) if torch.is_tensor(v) else v == w, (what, k, name)


def _assert_same_sched(a, b, what):
    for k in ("best", "num_bad_epochs", "cooldown_counter", "last_epoch", "_last_lr"):
        assert getattr(a, k) == getattr(b, k), (what, k, getattr(a, k), getattr(b, k))


WHOLE = [("regression-Adam", dict(step_size=0, lr=0.05), None),
         ("classification-SGD", dict(step_size=0, lr=0.05, optimizer="SGD"), 3)]


@pytest.mark.parametrize("case", WHOLE, ids=[c[0] for c in WHOLE])
def test_whole_fit_equals_the_host_loop(case):
    """135 REAL graphs in batches of 40 (three full batches and one of 15), 12-graph validation and test stores, patience 0,
    control every 2nd epoch, early_stopping 1, 40 epochs: in the host loop the lr is reduced and the fit stops before the
    40 (both asserted on the host loop alone).  `fit_network(lookahead=0, load_best=False)` leaves bitwise the loop's log,
    counters, best state, live weights, optimiser state, scheduler and loader generator; `lookahead=1` the same except the
    live weights (`epochs_enqueued` within its bound), and with `load_best=True` the model is `best_state`."""
    name, opts, classes = case
    epochs, es, ce = 40, 1, 2
    make = _setup(135, classes=classes, **opts)
    m0, trn0, val0, tst0 = make()
    ref = _host_loop(m0, trn0, val0, tst0, epochs, es, ce)
    rng_after = trn0.rng.bit_generator.state
    lrs = ref["log"][:, 3]
    print(f"\n    {name}: host loop ran {ref['epochs_run']} of {epochs} epochs, best {ref['best_val']:.6f} at {ref['best_epoch']}, "
          f"lr {opts['lr']} -> {lrs[-1]:.6g} ({len(set(lrs.tolist()))} values)")
    assert ref["stopped"] and ref["epochs_run"] < epochs and lrs[-1] < opts["lr"]
    assert epoch_window_of(m0, trn0) is not None                               # (the loop itself ran the one-graph epochs)

    m1, trn1, val1, tst1 = make()
    res = fit_network(m1, trn1, val1, tst1, "cuda", epochs=epochs, early_stopping=es, control_every=ce, lookahead=0, load_best=False)
    assert res.form == "device" and res.epochs_enqueued == res.epochs_run
    _assert_result(res, ref, name)
    for (k, q), r in zip(m1.named_parameters(), m0.parameters()):
        assert torch.equal(q, r), (name, k)
    _assert_same_opt(m1.optimizer, m0.optimizer, name)
    _assert_same_sched(m1.scheduler, m0.scheduler, name)
    assert trn1.rng.bit_generator.state == rng_after
    assert not m1.training
    # ... and the objects go on as after the loop: one more epoch of each
    assert train_network(m1, trn1, "cuda") == train_network(m0, trn0, "cuda")

    m2, trn2, val2, tst2 = make()
    res2 = fit_network(m2, trn2, val2, tst2, "cuda", epochs=epochs, early_stopping=es, control_every=ce, lookahead=1, load_best=True)
    _assert_result(res2, ref, name + " lookahead=1")
    assert res2.form == "device"
    assert res2.epochs_run < res2.epochs_enqueued <= min(epochs, res2.epochs_run + 1 * ce)
    _assert_same_sched(m2.scheduler, m0.scheduler, name)
    assert m2.optimizer.param_groups[0]["lr"] == m0.optimizer.param_groups[0]["lr"]
    assert trn2.rng.bit_generator.state == rng_after                           # (put back behind the last counted epoch)
    for k, v in m2.state_dict().items():
        assert torch.equal(v, res2.best_state[k]), (name, k)


def test_a_host_loader_takes_the_host_form():
    """A fit whose train loader is a host `DataLoader` has no captured epoch: the host form runs in the same call and returns
    the same fields, equal to the loop's."""
    epochs, es, ce = 5, 1, 2
    make = _setup(50, host_train=True, step_size=0, lr=0.05)
    m0, trn0, val0, tst0 = make()
    ref = _host_loop(m0, trn0, val0, tst0, epochs, es, ce)
    m1, trn1, val1, tst1 = make()
    res = fit_network(m1, trn1, val1, tst1, "cuda", epochs=epochs, early_stopping=es, control_every=ce, load_best=False)
    assert res.form == "host" and res.epochs_enqueued == res.epochs_run
    _assert_result(res, ref, "host form")
    for q, r in zip(m1.parameters(), m0.parameters()):
        assert torch.equal(q, r)
    _assert_same_sched(m1.scheduler, m0.scheduler, "host form")
    _assert_same_opt(m1.optimizer, m0.optimizer, "host form")


def test_a_fit_after_a_rebase_rebuilds_its_windows():
    """`optimizer.load_state_dict` moves parameters and moments onto new flat storages, so every captured window of the
    model holds old addresses.  The next fit notices before it enqueues anything, builds the windows again once and stays in
    the device form; its results are those of the host loop after the same reload (which rebuilds through
    `train._LoaderWindows.launch`)."""
    make = _setup(90, step_size=0, lr=0.05)
    kw = dict(early_stopping=5, control_every=2)
    runs = [make(), make()]
    (m0, *ld0), (m1, *ld1) = runs
    _host_loop(m0, *ld0, epochs=3, **kw)
    fit_network(m1, *ld1, "cuda", epochs=3, lookahead=0, load_best=False, **kw)
    window = epoch_window_of(m1, ld1[0])
    assert window is not None
    for m in (m0, m1):
        m.optimizer.load_state_dict(deepcopy(m.optimizer.state_dict()))
    ref = _host_loop(m0, *ld0, epochs=4, **kw)
    res = fit_network(m1, *ld1, "cuda", epochs=4, lookahead=1, load_best=False, **kw)
    assert res.form == "device" and epoch_window_of(m1, ld1[0]) is not window
    _assert_result(res, ref, "after a rebase")
    for q, r in zip(m1.parameters(), m0.parameters()):
        assert torch.equal(q, r)
    _assert_same_opt(m1.optimizer, m0.optimizer, "after a rebase")


def test_fits_at_once_equal_the_fits_alone():
    """`fit_networks`: three runs with different datasets, sizes, seeds and optimisers on their own streams, bitwise the
    three `fit_network` calls alone.  Run 0 is SGD at lr 0: its validation loss never changes, so it stops at epoch 6 of 11
    whatever the data and drops out while the others go on."""
    epochs, es, ce = 11, 2, 2
    makes = [_setup(135, data_seed=0, loader_seed=3, optimizer="SGD", lr=0.0),
             _setup(100, data_seed=7, loader_seed=4, val_from_train=True),
             _setup(90, data_seed=14, loader_seed=5, val_from_train=True, optimizer="rmsprop", lr=1e-3)]
    together, alone = [mk() for mk in makes], [mk() for mk in makes]
    kw = dict(epochs=epochs, early_stopping=es, control_every=ce, lookahead=1, load_best=False)
    got = fit_networks(*[[r[i] for r in together] for i in range(4)], "cuda", **kw)
    for k, (m, trn, val, tst) in enumerate(alone):
        one = fit_network(m, trn, val, tst, "cuda", **kw)
        print(f"\n    run {k}: {one.epochs_run} epochs counted, {one.epochs_enqueued} enqueued, stopped early: {one.stopped_early}")
        assert got[k].form == one.form == "device"
        _assert_result(got[k], dict(one._asdict(), stopped=one.stopped_early), f"run {k}")
        assert got[k].epochs_enqueued == one.epochs_enqueued
        for q, r in zip(together[k][0].parameters(), m.parameters()):
            assert torch.equal(q, r), k
        _assert_same_opt(together[k][0].optimizer, m.optimizer, f"run {k}")
        assert together[k][1].rng.bit_generator.state == trn.rng.bit_generator.state
    assert got[0].stopped_early and got[0].epochs_run == 7 and got[0].epochs_enqueued == 9
    skipped = fit_networks(*[[r[i] for r in together] for i in range(4)], "cuda", active=[False, True, False], epochs=1)
    assert skipped[0] is None and skipped[2] is None and skipped[1].epochs_run == 1
