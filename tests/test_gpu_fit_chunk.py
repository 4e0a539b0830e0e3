"""GPU tests of the chunk form of a fit (hcatgnet_amd/fit.py: `form="chunk"`) and of the shuffle drawn on the device
(csrc/shuffle.hip): the draw kernel against numpy's own generator and `store.epoch_layout`, its gate, and whole fits against
the existing device form (`form="epoch"`), which is the oracle of the feature.  Every comparison is bitwise: the draw is
numpy's algorithm on the same state, and the same kernels then run in the same order on the same index arrays."""
import ctypes
from functools import lru_cache

import numpy as np
import pytest
import torch

import hcatgnet_amd as H
from hcatgnet_amd import _lib, synth
from hcatgnet_amd import fit as F
from hcatgnet_amd import store as S
from hcatgnet_amd.fit import fit_network, fit_networks
from hcatgnet_amd.train import train_network
from tests.test_gpu_fit import WHOLE, _assert_result, _assert_same_opt, _assert_same_sched, _setup

pytestmark = pytest.mark.gpu
BS, DRAWS, SEED = 40, 4, 5


# ---------------------------------------------------------------------------------------------------------------
# the kernel alone
# ---------------------------------------------------------------------------------------------------------------
@lru_cache(maxsize=None)
def _graphs():
    return synth.make_config("REAL", num_graphs=135, seed=synth.BASE_SEED).as_graph_list()


def _loader(G, drop_last):
    store = H.DeviceGraphStore(_graphs()[:G], device="cuda")
    return H.DeviceLoader(store, batch_size=BS, shuffle=True, seed=SEED, drop_last=drop_last)


def _state_dev(stopped=0, epoch=0):
    st = _lib.FitState()
    st.stopped, st.epoch = stopped, epoch
    return torch.frombuffer(bytearray(bytes(st)), dtype=torch.uint8).cuda()


@pytest.mark.parametrize("drop_last", [False, True], ids=["keep_last", "drop_last"])
@pytest.mark.parametrize("G", [1, 2, 3, 40, 41, 135])
def test_draw_kernel_is_numpys_permutation_and_the_hosts_layout(G, drop_last):
    """Four consecutive draws over a store of G REAL graphs at batch size 40: the order is numpy's, the WHOLE index buffer
    (ids, every batch's graph_ptr and edge_ptr block, the zero in front of each and the padding words) is
    `epoch_layout(..., order)`, the generator read back is numpy's state dict.  The buffer starts as -1 everywhere, so every
    word the host writes must have been written.  G = 41, 135: a partial last batch (kept or dropped); 1, 2, 3: the loop's
    ends and a one-bit mask."""
    loader = _loader(G, drop_last)
    st, ref = loader.store, np.random.default_rng(SEED)
    gen = S.DeviceGenerator(loader).to_device()
    layout = torch.full((gen.layout_words(),), -1, dtype=torch.int64, device="cuda")
    for d in range(DRAWS):
        gen.draw(layout)
        order = ref.permutation(G)
        want = S.epoch_layout(st.n_host, st.e_host, BS, drop_last, order)[0]
        assert want.size == layout.numel()
        assert np.array_equal(gen.order(layout), order), (G, d)
        assert np.array_equal(layout.cpu().numpy(), want), (G, d)
        assert gen.state() == ref.bit_generator.state, (G, d)
    gen.to_host()
    assert loader.rng.bit_generator.state == ref.bit_generator.state
    assert loader.rng.permutation(G).tolist() == ref.permutation(G).tolist()


def test_a_gated_draw_of_a_finished_fit_writes_nothing():
    """A gate whose state is stopped, or whose epoch has reached `max_epochs`: index buffer and generator stay byte for byte;
    a live gate draws."""
    loader = _loader(41, False)
    gen = S.DeviceGenerator(loader).to_device()
    layout = torch.full((gen.layout_words(),), -3, dtype=torch.int64, device="cuda")
    gen.draw(layout)                                               # (one real draw: the generator holds a buffered half or not)
    buf0, rng0 = layout.clone(), gen.state_dev.clone()
    for gate, max_epochs in ((_state_dev(stopped=1, epoch=2), 10), (_state_dev(stopped=0, epoch=10), 10),
                             (_state_dev(stopped=1, epoch=10), 10)):
        gen.draw(layout, gate=gate, max_epochs=max_epochs)
        torch.cuda.synchronize()
        assert torch.equal(layout, buf0) and torch.equal(gen.state_dev, rng0)
    gen.draw(layout, gate=_state_dev(stopped=0, epoch=9), max_epochs=10)
    ref = np.random.default_rng(SEED)
    ref.permutation(41)
    assert np.array_equal(gen.order(layout), ref.permutation(41)) and gen.state() == ref.bit_generator.state


def test_a_store_past_the_cap_and_a_foreign_generator_have_no_device_generator():
    loader = _loader(3, False)
    loader.rng = np.random.Generator(np.random.Philox(1))
    with pytest.raises(_lib.HcgError, match="PCG64"):
        S.DeviceGenerator(loader)
    # the launch itself refuses a store past the cap (the host class never gets there)
    loader = _loader(3, False)
    gen = S.DeviceGenerator(loader).to_device()
    gen.args.G = _lib.HCG_EPOCH_DRAW_MAX_GRAPHS + 1
    with pytest.raises(_lib.HcgError, match="not supported"):
        gen.draw(torch.zeros(gen.layout_words(), dtype=torch.int64, device="cuda"))


# ---------------------------------------------------------------------------------------------------------------
# whole fits against the existing device form
# ---------------------------------------------------------------------------------------------------------------
def _fit(make, form, tweak=None, **kw):
    m, trn, val, tst = make()
    if tweak is not None:
        tweak(trn)
    return m, trn, fit_network(m, trn, val, tst, "cuda", form=form, **kw)


def _same_state(a, b):
    """Two bit generators' state dicts (Philox keeps arrays in its)."""
    if isinstance(a, dict):
        return isinstance(b, dict) and a.keys() == b.keys() and all(_same_state(a[k], b[k]) for k in a)
    return np.array_equal(a, b)


def _assert_same_fit(got, ref, what, live=True):
    """Log, counters, best state, scheduler, lr and loader generator; `live`: weights and optimiser state too."""
    (m1, trn1, r1), (m0, trn0, r0) = got, ref
    _assert_result(r1, dict(r0._asdict(), stopped=r0.stopped_early), what)
    _assert_same_sched(m1.scheduler, m0.scheduler, what)
    assert m1.optimizer.param_groups[0]["lr"] == m0.optimizer.param_groups[0]["lr"], what
    assert _same_state(trn1.rng.bit_generator.state, trn0.rng.bit_generator.state), what
    assert not m1.training
    if live:
        for (k, q), r in zip(m1.named_parameters(), m0.parameters()):
            assert torch.equal(q, r), (what, k)
        _assert_same_opt(m1.optimizer, m0.optimizer, what)


def _assert_chunk(res, epochs, ce, lookahead):
    assert res.form == "device-chunk"
    assert res.epochs_run <= res.epochs_enqueued <= min(epochs, res.epochs_run + lookahead * ce)
    assert res.graph_launches == F.chunk_launches(res.epochs_enqueued, ce)     # (a stop comes at a chunk's end: no tail then)


@pytest.mark.parametrize("case", WHOLE, ids=[c[0] for c in WHOLE])
def test_chunk_fit_equals_the_epoch_form(case):
    """The shapes of tests/test_gpu_fit.py (135 / 12 / 12 REAL graphs, batch 40, patience 0), 40 epochs, control every 2nd,
    early_stopping 1 -- the fit stops early and reduces its lr (asserted on the epoch form).  `form="chunk", lookahead=0,
    load_best=False` is bitwise `form="epoch"`: log, counters, best state, live weights, optimiser, scheduler, loader
    generator, and one further `train_network` epoch; `lookahead=1, load_best=True` the same except the live weights, and
    the model handed back is `best_state`."""
    name, opts, classes = case
    epochs, es, ce = 40, 1, 2
    make = _setup(135, classes=classes, **opts)
    kw = dict(epochs=epochs, early_stopping=es, control_every=ce)
    ref = _fit(make, "epoch", lookahead=0, load_best=False, **kw)
    r0 = ref[2]
    assert r0.form == "device" and r0.stopped_early and r0.epochs_run < epochs and r0.log[-1, 3] < opts["lr"]
    assert r0.graph_launches == 3 * r0.epochs_enqueued
    got = _fit(make, "chunk", lookahead=0, load_best=False, **kw)
    print(f"\n    {name}: {got[2].epochs_run} epochs in {got[2].graph_launches} graph launches (epoch form: {r0.graph_launches})")
    _assert_chunk(got[2], epochs, ce, 0)
    assert got[2].epochs_enqueued == got[2].epochs_run == r0.epochs_run
    _assert_same_fit(got, ref, name)
    ahead = _fit(make, "chunk", lookahead=1, load_best=True, **kw)
    _assert_chunk(ahead[2], epochs, ce, 1)
    assert ahead[2].epochs_run < ahead[2].epochs_enqueued
    _assert_same_fit(ahead, ref, name + " lookahead=1", live=False)
    for k, v in ahead[0].state_dict().items():
        assert torch.equal(v, ahead[2].best_state[k]), (name, k)
    # ... and the objects go on as after the epoch form: one more epoch of each (last: it moves the reference's generator)
    assert train_network(got[0], got[1], "cuda") == train_network(ref[0], ref[1], "cuda")


SCHEDULES = [("epochs7-every3", 7, 3, None), ("epochs8-every3-tail", 8, 3, None), ("every1", 5, 1, None),
             ("no-shuffle", 7, 3, lambda trn: setattr(trn, "shuffle", False))]


@pytest.mark.parametrize("case", SCHEDULES, ids=[c[0] for c in SCHEDULES])
def test_chunk_schedules_equal_the_epoch_form(case):
    """Fits that run all their epochs: 7 at every 3rd (epoch 0, two full chunks), 8 at every 3rd (the same and a one-epoch
    tail), control on every epoch (one-epoch graphs only), a train loader that does not shuffle (no draw launch: the identity
    arrays go up once).  The launch count is the schedule's."""
    name, epochs, ce, tweak = case
    make = _setup(135, step_size=0, lr=0.05)
    kw = dict(epochs=epochs, early_stopping=100, control_every=ce, lookahead=1, load_best=False)
    ref, got = _fit(make, "epoch", tweak, **kw), _fit(make, "chunk", tweak, **kw)
    assert ref[2].form == "device" and ref[2].epochs_run == epochs
    _assert_chunk(got[2], epochs, ce, 1)
    assert got[2].graph_launches == {"epochs7-every3": 3, "epochs8-every3-tail": 4, "every1": 5, "no-shuffle": 3}[name]
    _assert_same_fit(got, ref, name)
    assert train_network(got[0], got[1], "cuda") == train_network(ref[0], ref[1], "cuda")


def test_building_the_chunk_graphs_changes_nothing():
    """`build_chunk_windows` captures the one-epoch and the `control_every`-epoch graph (each capture's warm-up runs its
    epochs once) and launches nothing: weights, optimiser moments and step count and the loader's generator are bitwise what
    they were, and the fit that follows is the fit of a twin that never built ahead."""
    make = _setup(135, step_size=0, lr=0.05)
    kw = dict(epochs=6, early_stopping=100, control_every=2)
    m, trn, val, tst = make()
    fit_network(m, trn, val, tst, "cuda", epochs=1, form="epoch")              # (moments and a step count to compare)
    opt = m.optimizer
    before = ([q.detach().clone() for q in m.parameters()], [t.clone() for t in opt.capture_state()],
              {k: {n: (v.clone() if torch.is_tensor(v) else v) for n, v in s.items()} for k, s in opt.state_dict()["state"].items()},
              trn.rng.bit_generator.state, opt.steps_done())
    cs = F.build_chunk_windows(m, trn, val, tst, **kw)
    assert cs is not None and sorted(cs.graphs) == [1, 2]
    torch.cuda.synchronize()
    for q, r in zip(m.parameters(), before[0]):
        assert torch.equal(q, r)
    for t, u in zip(opt.capture_state(), before[1]):
        assert torch.equal(t, u)
    for k, s in opt.state_dict()["state"].items():
        for n, v in s.items():
            assert torch.equal(v, before[2][k][n]) if torch.is_tensor(v) else v == before[2][k][n], (k, n)
    assert trn.rng.bit_generator.state == before[3] and opt.steps_done() == before[4]
    assert cs.gen.state() == trn.rng.bit_generator.state                        # (the device copy went back too)
    assert F.build_chunk_windows(m, trn, val, tst, **kw) is cs                  # (kept on the loader for the next fit)
    twin = make()
    fit_network(*twin, "cuda", epochs=1, form="epoch")
    r1 = fit_network(m, trn, val, tst, "cuda", form="chunk", lookahead=0, load_best=False, **kw)
    r0 = fit_network(*twin, "cuda", form="epoch", lookahead=0, load_best=False, **kw)
    _assert_same_fit((m, trn, r1), (twin[0], twin[1], r0), "built ahead")


def test_a_foreign_generator_takes_the_device_form():
    """A loader whose generator is not numpy's PCG64 has no device draw: `form="chunk"` runs the existing device form in the
    same call, with the results of `form="epoch"`."""
    make = _setup(135, step_size=0, lr=0.05)
    philox = lambda trn: setattr(trn, "rng", np.random.Generator(np.random.Philox(1)))
    kw = dict(epochs=5, early_stopping=100, control_every=2, lookahead=1, load_best=False)
    ref, got = _fit(make, "epoch", philox, **kw), _fit(make, "chunk", philox, **kw)
    assert got[2].form == ref[2].form == "device" and got[2].graph_launches == 15
    _assert_same_fit(got, ref, "philox")


def test_chunk_fits_at_once_equal_the_fits_alone():
    """`fit_networks(form="chunk")`: the three runs of tests/test_gpu_fit.py's concurrent test on their own streams, bitwise
    the three `fit_network(form="chunk")` calls alone; run 0 (SGD at lr 0) stops early and drops out."""
    epochs, es, ce = 11, 2, 2
    makes = [_setup(135, data_seed=0, loader_seed=3, optimizer="SGD", lr=0.0),
             _setup(100, data_seed=7, loader_seed=4, val_from_train=True),
             _setup(90, data_seed=14, loader_seed=5, val_from_train=True, optimizer="rmsprop", lr=1e-3)]
    together, alone = [mk() for mk in makes], [mk() for mk in makes]
    kw = dict(epochs=epochs, early_stopping=es, control_every=ce, lookahead=1, load_best=False, form="chunk")
    got = fit_networks(*[[r[i] for r in together] for i in range(4)], "cuda", **kw)
    for k, (m, trn, val, tst) in enumerate(alone):
        one = fit_network(m, trn, val, tst, "cuda", **kw)
        _assert_chunk(one, epochs, ce, 1)
        assert got[k].form == "device-chunk"
        assert (got[k].epochs_enqueued, got[k].graph_launches) == (one.epochs_enqueued, one.graph_launches)
        _assert_same_fit((together[k][0], together[k][1], got[k]), (m, trn, one), f"run {k}")
    assert got[0].stopped_early and got[0].epochs_run == 7 and got[0].epochs_enqueued == 9
