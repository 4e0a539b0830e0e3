"""A whole fit -- the reference's epoch loop (scripts_experiments/train_GNN.py:73-111, restated in
examples/train_like_reference.py) -- without a host sync per epoch.

  reference loop, per epoch                              here (`fit_network`, device form)
  ---------------------------------------------------    ------------------------------------------------------------
  train_network / eval_network x 2: three blocking       draw the permutation, upload the index arrays through a ring of
      reads of a host float                                  pinned rows, replay the three hipGraphs (`train.EpochWindow`,
                                                             the two forward-only `train.StepWindow`s)
  every 5th epoch: model.scheduler.step(val_loss)        ONE launch of ONE workgroup behind them (csrc/fit.hip): the three
      (ReduceLROnPlateau), stall counting,                   losses from the graphs' float64 sums, the scheduler, the
      deepcopy(model.state_dict()) of the best epoch         early-stopping counters, the copy of the best weights and the
                                                             loss log, all in device memory
  `if stall > early_stopping: break`                     the host reads ONE flag per control interval, `lookahead`
                                                             intervals behind what it has enqueued

`form="chunk"` takes the first row's host work away too: the permutation and the index arrays are made on the device
(csrc/shuffle.hip, `store.DeviceGenerator`), and a control interval of epochs -- draw, three epochs' steps, controller,
`control_every` times over -- is ONE hipGraph (`ChunkWindow`), bitwise the form above.

Both device forms are one skeleton: `_ControlBlock` is the controller's device memory and launch arguments, `chunk_end` says
where a chunk ends, `_DeviceFit` issues chunks, posts the state copy behind each control epoch, reads the stop flag and gathers
the result; `_EpochFit` and `_ChunkFit` only say how a chunk's epochs are enqueued.

`FitControl` is that launch's state machine in plain Python: the host form of a fit (any loader / scheduler the device form
does not take) runs on it, and the tests hold the kernel against it bit for bit.
"""
from __future__ import annotations

import ctypes
import time
from collections import OrderedDict
from copy import deepcopy
from typing import NamedTuple, Optional

import numpy as np
import torch

from . import _lib
from . import train as T
from .optim import FusedFlatOptimizer


class FitResult(NamedTuple):
    log: np.ndarray             # [epochs_run, 4] float64: train, validation, test loss and the lr after the epoch
    epochs_run: int             # epochs the loop counted (the reference's loop would have run exactly these)
    stopped_early: bool         # the early-stopping limit was reached
    best_epoch: int             # control epoch with the lowest validation loss
    best_val: float
    best_state: dict            # state-dict of clones: the weights after `best_epoch` (the initial ones if none was better)
    epochs_enqueued: int        # epochs issued to the GPU: epochs_run <= ... <= epochs_run + lookahead * control_every
    form: str = "device"        # "device", "device-chunk" or "host"
    enqueue_s: float = 0.0      # host seconds until the last epoch was issued (before the final synchronisation)
    graph_launches: int = 0     # hipGraph launches issued: three per epoch in the device form, one per chunk in the chunk form


def _plateau_of(model):
    """The model's scheduler if the fit controller restates it: ReduceLROnPlateau, mode "min", threshold_mode "rel", one
    parameter group (one min_lr)."""
    sched = getattr(model, "scheduler", None)
    if (isinstance(sched, torch.optim.lr_scheduler.ReduceLROnPlateau) and sched.mode == "min"
            and sched.threshold_mode == "rel" and len(sched.optimizer.param_groups) == 1 and len(sched.min_lrs) == 1):
        return sched
    return None


class FitControl:
    """csrc/fit.hip's state machine on Python floats: per epoch `step(train, val, test)`; on a control epoch (`epoch %
    control_every == 0`) torch's `ReduceLROnPlateau.step(val)` (mode "min", threshold_mode "rel") and then the example
    loop's bookkeeping (best validation loss, stall count, `stopped = stall > early_stopping`).  `schedule=False`: the
    caller steps a scheduler of its own and sets `lr`; only the bookkeeping and the log happen here."""

    STATE = ("lr", "sched_best", "val_best", "epoch", "num_bad_epochs", "cooldown_counter", "last_epoch", "best_epoch",
             "stall", "stopped", "epochs_counted")

    def __init__(self, lr, factor=0.1, patience=10, threshold=1e-4, cooldown=0, min_lr=0.0, eps=1e-8, control_every=5,
                 early_stopping=6, max_epochs=250, sched_best=float("inf"), num_bad_epochs=0, cooldown_counter=0,
                 last_epoch=0, schedule=True):
        self.factor, self.patience, self.rel_epsilon = float(factor), int(patience), 1.0 - threshold
        self.cooldown, self.min_lr, self.eps = int(cooldown), float(min_lr), float(eps)
        self.control_every, self.early_stopping, self.max_epochs = int(control_every), int(early_stopping), int(max_epochs)
        self.schedule = bool(schedule)
        self.lr, self.sched_best, self.val_best = float(lr), float(sched_best), float("inf")
        self.epoch, self.num_bad_epochs, self.cooldown_counter, self.last_epoch = 0, int(num_bad_epochs), int(cooldown_counter), int(last_epoch)
        self.best_epoch, self.stall, self.stopped, self.epochs_counted = 0, 0, 0, 0
        self.log = []

    @classmethod
    def for_model(cls, model, control_every, early_stopping, max_epochs):
        """Continue the model's scheduler where it stands (a fresh one: best = inf, counters 0)."""
        lr, sched = float(model.optimizer.param_groups[0]["lr"]), _plateau_of(model)
        if sched is None:
            return cls(lr, control_every=control_every, early_stopping=early_stopping, max_epochs=max_epochs, schedule=False)
        return cls(lr, sched.factor, sched.patience, sched.threshold, sched.cooldown, sched.min_lrs[0], sched.eps, control_every,
                   early_stopping, max_epochs, sched.best, sched.num_bad_epochs, sched.cooldown_counter, sched.last_epoch)

    def control_epoch(self) -> bool:
        return self.epoch % self.control_every == 0

    def live(self) -> bool:
        return not self.stopped and self.epoch < self.max_epochs

    def step(self, train, val, test) -> Optional[bool]:
        """One epoch's losses -> whether the weights after it are the best so far (a snapshot is due); None = ignored (the
        fit has stopped, or `max_epochs` rows are written)."""
        if not self.live():
            return None
        train, val, test, snapshot = float(train), float(val), float(test), False
        if self.control_epoch():
            if self.schedule:
                self.last_epoch += 1
                if val < self.sched_best * self.rel_epsilon:
                    self.sched_best, self.num_bad_epochs = val, 0
                else:
                    self.num_bad_epochs += 1
                if self.cooldown_counter > 0:
                    self.cooldown_counter -= 1
                    self.num_bad_epochs = 0
                if self.num_bad_epochs > self.patience:
                    new = max(self.lr * self.factor, self.min_lr)
                    if self.lr - new > self.eps:
                        self.lr = new
                    self.cooldown_counter, self.num_bad_epochs = self.cooldown, 0
            if val < self.val_best:
                self.val_best, self.best_epoch, self.stall, snapshot = val, self.epoch, 0, True
            else:
                self.stall += 1
            self.stopped = int(self.stall > self.early_stopping)
        self.log.append((train, val, test, self.lr))
        self.epoch += 1
        self.epochs_counted += 1
        return snapshot

    def state(self) -> dict:
        return {k: getattr(self, k) for k in self.STATE}


def _write_back(model, st: dict):
    """The controller's state -> the host objects a caller goes on with: the group's lr, the optimiser's record of what its
    device word holds (so `sync_lr()` pushes nothing stale), the scheduler's attributes."""
    opt, sched = model.optimizer, _plateau_of(model)
    opt.param_groups[0]["lr"] = st["lr"]
    fl = getattr(opt, "_flat", {}).get(0)
    if fl is not None and "lr_dev" in fl:
        if fl["lr_host"] != st["lr"]:
            fl["lr_dev"].fill_(st["lr"])
        fl["lr_host"] = st["lr"]
    if sched is not None:
        sched.best, sched.num_bad_epochs = st["sched_best"], st["num_bad_epochs"]
        sched.cooldown_counter, sched.last_epoch, sched._last_lr = st["cooldown_counter"], st["last_epoch"], [st["lr"]]


def _result(model, fc_state, log, stopped, best_state, enqueued, form, enqueue_s, load_best, graph_launches=0):
    if load_best:
        model.load_state_dict(best_state)
    return FitResult(np.asarray(log, dtype=np.float64).reshape(-1, 4), int(fc_state["epochs_counted"]), bool(stopped),
                     int(fc_state["best_epoch"]), float(fc_state["val_best"]), best_state, int(enqueued), form, enqueue_s,
                     int(graph_launches))


# ---------------------------------------------------------------------------------------------------------------
# host form: the example's loop
# ---------------------------------------------------------------------------------------------------------------
def _host_fit(model, train_loader, val_loader, test_loader, device, epochs, early_stopping, control_every, load_best):
    fc = FitControl.for_model(model, control_every, early_stopping, epochs)
    sched, group = getattr(model, "scheduler", None), model.optimizer.param_groups[0]
    best_state = deepcopy(model.state_dict())
    t0 = time.perf_counter()
    for _ in range(epochs):
        if fc.stopped:
            break
        train_loss = T.train_network(model, train_loader, device)
        val_loss = T.eval_network(model, val_loader, device)
        test_loss = T.eval_network(model, test_loader, device)
        control = fc.control_epoch()
        if control and not fc.schedule and sched is not None:
            sched.step(val_loss)
            fc.lr = float(group["lr"])
        snapshot = fc.step(train_loss, val_loss, test_loss)
        if control and fc.schedule:
            _write_back(model, fc.state())
        if snapshot:
            best_state = deepcopy(model.state_dict())
    st = fc.state()
    return _result(model, st, fc.log, st["stopped"], best_state, st["epochs_counted"], "host", time.perf_counter() - t0, load_best)


# ---------------------------------------------------------------------------------------------------------------
# device forms: the controller's block, the chunk schedule, the run skeleton
# ---------------------------------------------------------------------------------------------------------------
class _HostForm(Exception):
    """The device form does not take this fit (the reason is the message): the host form runs it."""


class _EpochForm(Exception):
    """The chunk form does not take this fit (the reason is the message): the device form runs it, epoch by epoch."""


def _first_state(model) -> _lib.FitState:
    """The controller's state before a fit's first epoch, as the struct the kernel reads: the group's lr, the model's scheduler
    continued where it stands, nothing counted yet -- `FitControl.for_model(model, ...).state()`.  Needs no device."""
    s, init = _plateau_of(model), _lib.FitState()
    init.lr, init.sched_best, init.val_best = float(model.optimizer.param_groups[0]["lr"]), float(s.best), float("inf")
    init.num_bad_epochs, init.cooldown_counter, init.last_epoch = int(s.num_bad_epochs), int(s.cooldown_counter), int(s.last_epoch)
    return init


class _ControlBlock:
    """The controller launch's device memory for one fit at a time -- `FitState` bytes, loss log, best-weights slot -- and its
    arguments, constants and pointers filled once; `args.sums` is left to whoever issues or records the launch."""

    def __init__(self, model, fl, denominators, epochs, early_stopping, control_every):
        s, dev = _plateau_of(model), fl["p"].device
        self.model, self.fl, self.pins = model, fl, {}
        self.state_dev = torch.zeros(ctypes.sizeof(_lib.FitState), dtype=torch.uint8, device=dev)
        self.log_dev = torch.empty((epochs, 4), dtype=torch.float64, device=dev)
        self.best = torch.empty_like(fl["p"])
        self.args = a = _lib.FitControlArgs()
        a.state, a.best, a.n, a.log = self.state_dev.data_ptr(), self.best.data_ptr(), fl["n"], self.log_dev.data_ptr()
        a.lr_dev, a.param = fl["lr_dev"].data_ptr(), fl["p"].data_ptr()
        a.denom[0], a.denom[1], a.denom[2] = (float(d) for d in denominators)
        a.factor, a.rel_epsilon, a.min_lr, a.eps = float(s.factor), 1.0 - s.threshold, float(s.min_lrs[0]), float(s.eps)
        a.patience, a.cooldown, a.control_every = int(s.patience), int(s.cooldown), control_every
        a.early_stopping, a.max_epochs = early_stopping, epochs

    def reset(self):
        """A fit's start on the current stream: the first state, an empty log, the best slot = the weights as they are."""
        self.state_dev.copy_(torch.frombuffer(bytearray(bytes(_first_state(self.model))), dtype=torch.uint8))
        self.log_dev.fill_(float("nan"))
        self.best.copy_(self.fl["p"])          # (the reference keeps the initial state-dict until an epoch is better)

    def read(self) -> dict:
        """The state as `FitControl.state()` gives it (waits for the current stream)."""
        torch.cuda.current_stream().synchronize()
        raw = _lib.FitState.from_buffer_copy(self.state_dev.cpu().numpy().tobytes())
        return {k: getattr(raw, k) for k in FitControl.STATE}

    def log(self, n):
        return self.log_dev[:n].cpu().numpy()

    def best_state_dict(self) -> OrderedDict:
        """The best slot as a state-dict of clones (entries outside the flat storage: as they are in the model)."""
        off, offs = 0, {}
        for q in self.fl["params"]:
            offs[id(q)] = off
            off += q.numel()
        best_state = OrderedDict()
        for k, v in self.model.state_dict(keep_vars=True).items():
            o = offs.get(id(v))
            best_state[k] = (self.best[o:o + v.numel()].view(v.shape).clone() if o is not None else v.detach().clone())
        return best_state

    def pinned(self, lookahead):
        """Pinned rows and events for the state copies of a fit with this look-ahead: one per unread control epoch."""
        got = self.pins.get(lookahead)
        if got is None:
            got = self.pins[lookahead] = (torch.zeros(lookahead + 1, self.state_dev.numel(), dtype=torch.uint8).pin_memory(),
                                          [torch.cuda.Event() for _ in range(lookahead + 1)])
        return got


def chunk_end(issued: int, epochs: int, control_every: int) -> int:
    """The exclusive end of the chunk that starts at `issued`: epoch 0 alone, then up to and including the next control epoch."""
    return min(epochs, issued + control_every if issued else 1)


def chunk_launches(epochs: int, control_every: int) -> int:
    """Graph launches of a chunk-form fit that runs all `epochs`: epoch 0, the full control intervals, the tail's epochs."""
    return 1 + (epochs - 1) // control_every + (epochs - 1) % control_every


class _DeviceFit:
    """One fit in a device form, issued chunk by chunk (`chunk_end`) on the stream that is current at each call; behind a
    chunk that ends in a control epoch the state struct's asynchronous copy, and `check()` after each chunk is the
    look-ahead's one read of the stop flag.  A form says what it needs on top of this (`_eligible`), what it launches
    (`_bind`: once the windows stand; `_issue`: a chunk's epochs) and where the loader's generator ends (`_settle_generator`)."""

    def __init__(self, model, train_loader, val_loader, test_loader, epochs, early_stopping, control_every, lookahead):
        self.model, self.loaders = model, (train_loader, val_loader, test_loader)
        self.epochs, self.early_stopping, self.every, self.lookahead = epochs, early_stopping, control_every, lookahead
        if _plateau_of(model) is None:
            raise _HostForm("the scheduler is not a ReduceLROnPlateau with mode 'min', threshold_mode 'rel' and one group")
        if not isinstance(model.optimizer, FusedFlatOptimizer) or len(model.optimizer.param_groups) != 1:
            raise _HostForm("the optimiser is not one of the fused ones with one parameter group")
        self._eligible()
        self.block = None
        self._resolve()                        # (the windows, built on first use: not a device form without all three)
        self.state_pin, self.state_events = self.block.pinned(lookahead)
        self.issued, self.controls, self.graph_launches, self.done, self.stop_seen = 0, 0, 0, False, False
        self.t0, self.enqueue_s = time.perf_counter(), 0.0

    def _eligible(self):
        pass

    def _resolve(self):
        """The three windows and the optimiser's flat storages as they are NOW -> `_bind`.  A window whose baked-in addresses
        were replaced since its capture (`load_state_dict` of the optimiser, a larger eager batch) is dropped and built
        again, once, as `train._LoaderWindows.launch` does: nothing is written through an old pointer.  The same pass covers
        what a form captures on top of the windows: where `_bind` ran their steps (it says so), they are looked at again."""
        model, opt = self.model, self.model.optimizer
        kinds = (T._EPOCH_WINDOWS, T._EVAL_WINDOWS, T._EVAL_WINDOWS)
        for attempt in range(2):
            wins = [kind.of(model, ld, build=True) for kind, ld in zip(kinds, self.loaders)]
            if any(w is None for w in wins):
                raise _HostForm("a loader has no captured window (a host loader, a layer on the row-streaming kernels, a live "
                                "multi-rank process group)")
            steps = (wins[0].window, wins[1], wins[2])
            live = opt.capture_state()         # (flat storages and device words; a re-base here shows as a stale window)
            look = lambda: [not T._replayable(w.steps, w._fp, False) for w in steps]
            stale = look()
            if not any(stale):
                fl = opt._flat[0]
                if not opt.on_storages(live) or fl["params"][0].data_ptr() != fl["p"].data_ptr():
                    raise _lib.HcgError("fit_network: the optimiser's flat storages are not the model's parameters")
                opt.sync_lr()
                stale = look() if self._bind(wins, fl) else stale
                if not any(stale):
                    return
            if attempt:
                raise _lib.HcgError("fit_network: a window went stale again right after it was rebuilt")
            for ld, kind, bad in zip(self.loaders, kinds, stale):
                if bad:
                    setattr(ld, kind.attr, None)

    def issue_chunk(self):
        """Enqueue the next chunk on the current stream."""
        first, end = self.issued, chunk_end(self.issued, self.epochs, self.every)
        if end > first:
            self.graph_launches += self._issue(first, end)
            self.issued = end
            if (end - 1) % self.every == 0:
                slot = self.controls % (self.lookahead + 1)
                self.state_pin[slot].copy_(self.block.state_dev, non_blocking=True)
                self.state_events[slot].record()
                self.controls += 1
        self.enqueue_s = time.perf_counter() - self.t0

    def check(self) -> bool:
        """After a chunk: wait for the control epoch `lookahead` chunks back, read its stop flag -> nothing more to issue."""
        c = self.controls - 1 - self.lookahead
        if c >= 0 and not self.stop_seen:
            slot = c % (self.lookahead + 1)
            self.state_events[slot].synchronize()
            self.stop_seen = bool(_lib.FitState.from_buffer_copy(self.state_pin[slot].numpy().tobytes()).stopped)
        self.done = self.stop_seen or self.issued >= self.epochs
        return self.done

    def finish(self, load_best) -> FitResult:
        st = self.block.read()
        self._settle_generator(st["epochs_counted"])
        _write_back(self.model, st)
        self.model.eval()                      # (the loop's last call is an eval_network)
        return _result(self.model, st, self.block.log(st["epochs_counted"]), st["stopped"], self.block.best_state_dict(),
                       self.issued, self.form, self.enqueue_s, load_best, self.graph_launches)


class _EpochFit(_DeviceFit):
    """The device form: every epoch enqueued on its own -- the permutation from the loader's generator, the index upload
    through a ring of pinned rows, three graph replays, the controller launch."""

    form = "device"

    def _bind(self, wins, fl):
        """The fit's block and staging on first use; the controller reads the sums of the windows as they are now."""
        if self.block is None:
            self.block = _ControlBlock(self.model, fl, (wins[0].G, len(self.loaders[1].dataset), len(self.loaders[2].dataset)),
                                       self.epochs, self.early_stopping, self.every)
            self.block.reset()
            nrows = (self.lookahead + 1) * self.every + 1       # (one row of index arrays per epoch that can be in flight)
            self.rows = [torch.zeros_like(wins[0].host).pin_memory() for _ in range(nrows)]
            self.row_events, self.rng_states = [torch.cuda.Event() for _ in range(nrows)], []
        elif fl is not self.block.fl:
            raise _lib.HcgError("fit_network: the optimiser re-based its flat storages during the fit")
        self.wins, a = wins, self.block.args
        a.sums[0], a.sums[1], a.sums[2] = (w.value_dev.data_ptr() for w in (wins[0].window, wins[1], wins[2]))
        return False

    def _issue(self, first, end):
        self._resolve()
        (tw, vw, tew), args = self.wins, self.block.args
        rows, events, nrows = self.rows, self.row_events, len(self.rows)
        rng, states = self.loaders[0].rng, self.rng_states
        for e in range(first, end):
            order = tw.draw_order()
            states.append(rng.bit_generator.state)
            r = e % nrows
            events[r].synchronize()                     # (the upload that read this row has long run; none yet: no wait)
            tw.launch_epoch(order, staging=rows[r])
            events[r].record()
            vw.replay()
            tew.replay()
            _lib.fit_control(args)
        return 3 * (end - first)

    def _settle_generator(self, counted):
        """The loader goes on as after the host loop: the epochs issued past the stop drew permutations it never would have."""
        if counted < self.issued:
            self.loaders[0].rng.bit_generator.state = self.rng_states[counted - 1]


# ---------------------------------------------------------------------------------------------------------------
# chunk form: a control interval of epochs as ONE graph, the shuffle drawn on the device
# ---------------------------------------------------------------------------------------------------------------
class ChunkWindow:
    """`L` consecutive epochs of a fit as ONE hipGraph, recorded per epoch in the order the device form issues them:
      the draw and layout launch (csrc/shuffle.hip) into the `EpochWindow`'s index buffer, gated on the fit state;
      the train epoch -- the `EpochWindow`'s own `FusedTrainStep`s, slot batches and collate launch -- and its float64 sum;
      the validation and the test steps of the two forward-only windows with their sums;
      the controller launch (csrc/fit.hip), `sums` pointing at this graph's own three sum tensors of that epoch.
    Nothing comes from the host between two epochs, so a replay is one launch whatever `L`.  The capture's warm-up runs all of
    it once; `ChunkWindows` takes that back (weights, optimiser, controller, generator, index buffer)."""

    def __init__(self, cs, L: int):
        self.cs, self.L = cs, int(L)
        tw, vw, tew = cs.wins
        self.parts = (tw.window, vw, tew)
        self.steps = [st for w in self.parts for st in w.steps]

        def run():
            a, sums = cs.block.args, []
            for _ in range(self.L):
                if cs.shuffle:
                    cs.gen.draw(tw.dbuf, gate=cs.block.state_dev, max_epochs=cs.epochs)
                three = [w.run()[1] for w in self.parts]
                a.sums[0], a.sums[1], a.sums[2] = (s.data_ptr() for s in three)
                _lib.fit_control(a)
                sums.append(three)
            return sums
        cap = T._Capture(cs.model.optimizer, True, run)
        self.graph = cap.graph
        with cap.recording():
            self.sums = run()                   # (kept alive: the graph's controller launches read them)
        self._fp = [st._graph_fingerprint() for st in self.steps]

    def replayable(self) -> bool:
        return T._replayable(self.steps, self._fp, True)

    def replay(self):
        if not self.replayable():
            raise _lib.HcgError("ChunkWindow.replay(): parameter / optimiser / step buffers changed since the capture: build it again")
        self.graph.replay()


class ChunkWindows:
    """What a fit in the chunk form replays, kept on the train loader for the next fit of the same model and settings: the
    one-epoch graph (epoch 0 and a tail) and the `control_every`-epoch graph, and the device memory they have baked in -- the
    controller's `block` (state, log, best slot), the loader's generator (`store.DeviceGenerator`).  `max_epochs`, the
    scheduler's constants and the stop limit are launch arguments of the recorded controller, so they are part of `key`."""

    ATTR = "_hcg_chunk_windows"

    @classmethod
    def of(cls, model, loaders, wins, fl, epochs, early_stopping, control_every, build=True):
        """The train loader's windows for this model, loaders and settings (`wins`: the three loaders' captured windows as
        they are now, `fl`: the optimiser's flat storages), built on first use; a set whose baked-in addresses were replaced
        since is dropped and built again.  None: the capture failed (kept: not tried again for the same key)."""
        sched, trn = _plateau_of(model), loaders[0]
        key = (epochs, early_stopping, control_every, float(sched.factor), float(sched.threshold), int(sched.patience),
               int(sched.cooldown), float(sched.min_lrs[0]), float(sched.eps), bool(trn.shuffle))
        ent = getattr(trn, cls.ATTR, None)
        if ent is not None and ent[0] is model and ent[1] == key and all(a is b for a, b in zip(ent[2], loaders)):
            cs = ent[3]
            if cs is None or (all(a is b for a, b in zip(cs.wins, wins)) and cs.fl is fl
                              and all(g.replayable() for g in cs.graphs.values())):
                return cs
        if not build:
            return None
        try:
            cs = cls(model, loaders, wins, fl, epochs, early_stopping, control_every)
        except (_lib.HcgError, RuntimeError):       # refused, or the capture failed (memory, an unsupported launch)
            cs = None
        try:
            setattr(trn, cls.ATTR, (model, key, tuple(loaders), cs))
        except Exception:
            pass
        return cs

    def __init__(self, model, loaders, wins, fl, epochs, early_stopping, control_every):
        from .store import DeviceGenerator
        self.model, self.loaders, self.wins, self.fl = model, tuple(loaders), tuple(wins), fl
        self.epochs, self.every, self.shuffle = epochs, control_every, bool(loaders[0].shuffle)
        self.gen = DeviceGenerator(loaders[0])
        self.block = b = _ControlBlock(model, fl, (wins[0].G, len(loaders[1].dataset), len(loaders[2].dataset)), epochs,
                                       early_stopping, control_every)
        self.reset()                            # (the warm-ups run on a fit's first state, not on zeros)
        # every capture's warm-up is L hidden epochs: taken back in place, each graph's starting where a fit would
        opt, self.graphs = model.optimizer, {}
        held = [fl["lr_dev"], b.state_dev, b.log_dev, b.best, self.gen.state_dev, wins[0].dbuf]
        with T._taken_back(opt, held, "ChunkWindows") as restore:
            if not opt.on_storages([fl["p"]]):
                raise _lib.HcgError("ChunkWindows: the optimiser re-based its state before the capture")
            for L in sorted({1, control_every}):
                if self.graphs:
                    restore()
                self.graphs[L] = ChunkWindow(self, L)

    def reset(self):
        """A fit's start on the current stream: the controller's block, the loader's generator moved up; a loader that does
        not shuffle gets its (identity) index arrays once."""
        self.block.reset()
        self.gen.to_device()
        if not self.shuffle:
            self.wins[0]._layout(np.arange(self.wins[0].G))


class _ChunkFit(_DeviceFit):
    """The chunk form: a chunk of `control_every` epochs is ONE replay of the `control_every`-epoch graph, any other (epoch 0,
    a tail shorter than an interval) one-epoch graphs."""

    form = "device-chunk"

    def _eligible(self):
        from .store import DeviceGenerator, DeviceLoader
        if not isinstance(self.loaders[0], DeviceLoader):
            raise _HostForm("the train loader is a host loader")
        why = DeviceGenerator.reason(self.loaders[0])
        if why is not None:
            raise _EpochForm(why)

    def _bind(self, wins, fl):
        """The kept graphs for the windows as they are now (building them runs the windows' steps), at a fit's start."""
        self.cs = ChunkWindows.of(self.model, self.loaders, wins, fl, self.epochs, self.early_stopping, self.every)
        if self.cs is None:
            raise _EpochForm("the chunk graphs could not be captured")
        self.block = self.cs.block
        self.cs.reset()
        return True

    def _issue(self, first, end):
        n = end - first
        L, n = (n, 1) if n == self.every else (1, n)
        graph = self.cs.graphs[L]
        for _ in range(n):
            graph.replay()
        return n

    def _settle_generator(self, counted):
        """Epochs issued past the stop drew nothing (the gate): the device generator IS where the host loop's would be."""
        if self.cs.shuffle:
            self.cs.gen.to_host()


FORMS = ("epoch", "chunk")


def build_chunk_windows(model, train_loader, val_loader, test_loader, epochs=250, early_stopping=6, control_every=5):
    """Capture, ahead of the first `fit_network(..., form="chunk")` with these settings, what it replays -> the
    `ChunkWindows` kept on the train loader, or None where the fit would not take the chunk form.  Launches nothing that
    stays: weights, optimiser, scheduler and the loader's generator are bitwise what they were."""
    epochs, early_stopping, control_every, _ = _check_args(epochs, early_stopping, control_every, 0)
    try:
        return _ChunkFit(model, train_loader, val_loader, test_loader, epochs, early_stopping, control_every, 0).cs
    except (_HostForm, _EpochForm):
        return None


def _make_run(form, model, loaders, epochs, early_stopping, control_every, lookahead):
    """The fit's run object in the form asked for, else the next one down: chunk -> device (epoch by epoch) -> None = host."""
    try:
        if form == "chunk":
            try:
                return _ChunkFit(model, *loaders, epochs, early_stopping, control_every, lookahead)
            except _EpochForm:
                pass
        return _EpochFit(model, *loaders, epochs, early_stopping, control_every, lookahead)
    except _HostForm:
        return None


def _check_args(epochs, early_stopping, control_every, lookahead, form="epoch"):
    if form not in FORMS:
        raise ValueError(f"form must be one of {FORMS}, got {form!r}")
    if int(epochs) < 1:
        raise ValueError(f"epochs must be at least 1, got {epochs}")
    if int(control_every) < 1:
        raise ValueError(f"control_every must be at least 1, got {control_every}")
    if int(lookahead) < 0:
        raise ValueError(f"lookahead must not be negative, got {lookahead}")
    if int(early_stopping) < 0:
        raise ValueError(f"early_stopping must not be negative, got {early_stopping}")
    return int(epochs), int(early_stopping), int(control_every), int(lookahead)


def fit_network(model, train_loader, val_loader, test_loader, device, epochs=250, early_stopping=6, control_every=5,
                lookahead=1, load_best=True, form="epoch") -> FitResult:
    """The reference's whole epoch loop for one model (scripts_experiments/train_GNN.py:73-111): per epoch train, validate,
    test; on every `control_every`-th epoch (0, control_every, ...) `model.scheduler.step(val_loss)`, the best validation
    loss with a copy of its weights, and the stall count that ends the fit once it exceeds `early_stopping`.

    Device form (loaders are `DeviceLoader`s whose epochs are captured windows, a fused optimiser, a ReduceLROnPlateau
    with mode "min" / threshold_mode "rel" and one group): every epoch is enqueued without a blocking read -- the
    permutation from the loader's own generator, the index upload, three graph replays, one controller launch
    (csrc/fit.hip) that keeps schedule, stop decision, best weights and log on the device.  The host reads the stop flag of
    the control epoch `lookahead` intervals behind the one it has just enqueued:
      lookahead = 0   waits on every control epoch: exact in every respect, one sync per `control_every` epochs;
      lookahead > 0   up to lookahead * control_every epochs past the stop have been issued.  The controller ignores them
                      (no log row, no snapshot, no lr change) and the loader's generator is put back, but they DO move the
                      live weights, the optimiser's moments and its step count.
    `load_best=True` (what the reference does next, utils/utils_model.py:170) loads `best_state` into the model, so the
    model handed back does not depend on `lookahead`.  Log, best state, scheduler and lr are bitwise the host loop's.
    Any other case runs the host form in the same call: the example's loop over `train_network` / `eval_network`.

    `form="chunk"` (opt-in; `FitResult.form == "device-chunk"`): the shuffle is drawn ON the device (csrc/shuffle.hip: numpy's
    own PCG64 permutation bit for bit, and the epoch's index arrays made of it), so nothing an epoch needs comes from the
    host and a control interval is ONE graph (`ChunkWindow`): chunk 0 a one-epoch graph, every further chunk one replay of
    the `control_every`-epoch graph, a shorter tail one-epoch graphs -- about epochs / control_every launches
    (`FitResult.graph_launches`) instead of four per epoch and an upload.  `lookahead` as above; the epochs issued past the
    stop draw nothing (the launch is gated on the fit state) and train on the last order, so the loader's generator ends
    where the host loop's would with nothing to put back.  Everything a fit leaves is bitwise the device form's.  Needs the
    device form's conditions, a loader generator that is numpy's PCG64 (the default) and a train store of at most
    `_lib.HCG_EPOCH_DRAW_MAX_GRAPHS` graphs; else the device form runs, and failing that the host form."""
    epochs, early_stopping, control_every, lookahead = _check_args(epochs, early_stopping, control_every, lookahead, form)
    run = _make_run(form, model, (train_loader, val_loader, test_loader), epochs, early_stopping, control_every, lookahead)
    if run is None:
        return _host_fit(model, train_loader, val_loader, test_loader, device, epochs, early_stopping, control_every, load_best)
    while not run.done:
        run.issue_chunk()
        run.check()
    return run.finish(load_best)


def fit_networks(models, train_loaders, val_loaders, test_loaders, device, epochs=250, early_stopping=6, control_every=5,
                 lookahead=1, load_best=True, active=None, form="epoch") -> list:
    """`fit_network` of several independent runs at once (see `train.train_networks`) -> [FitResult] (None where
    `active[k]` is false).  Every run in the device form goes on its own stream with its own controller; each round issues
    one chunk of every live run before any stop flag is waited for, and a run that stops drops out.  Each run is bitwise the
    run alone.  Runs in the host form are fitted in turn.  `form`: as `fit_network`'s, decided run by run."""
    models = list(models)
    K = len(models)
    if any(len(x) != K for x in (train_loaders, val_loaders, test_loaders)) or (active is not None and len(active) != K):
        raise ValueError("fit_networks: one train, validation and test loader (and one `active` flag) per model")
    epochs, early_stopping, control_every, lookahead = _check_args(epochs, early_stopping, control_every, lookahead, form)
    out, runs, host = [None] * K, [], []
    cur = torch.cuda.current_stream(device)
    for k, m in enumerate(models):
        if active is not None and not active[k]:
            continue
        st = T._run_stream(m, device)
        st.wait_stream(cur)
        with torch.cuda.stream(st):
            run = _make_run(form, m, (train_loaders[k], val_loaders[k], test_loaders[k]), epochs, early_stopping, control_every,
                            lookahead)
            if run is None:
                host.append(k)
            else:
                runs.append((k, st, run))
    live = list(runs)
    while live:
        for _, st, run in live:
            with torch.cuda.stream(st):
                run.issue_chunk()
        live = [(k, st, run) for k, st, run in live if not run.check()]
    for k, st, run in runs:
        with torch.cuda.stream(st):
            out[k] = run.finish(load_best)
        cur.wait_stream(st)
    for k in host:
        out[k] = _host_fit(models[k], train_loaders[k], val_loaders[k], test_loaders[k], device, epochs, early_stopping,
                           control_every, load_best)
    return out
