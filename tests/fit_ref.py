"""Reference side of the fit-control tests (tests/test_host_fit.py, tests/test_gpu_fit.py): loss sequences, seeded and
crafted, and the loop of examples/train_like_reference.py over them with torch's own ReduceLROnPlateau on a dummy optimiser.
Nothing here imports hcatgnet_amd.fit."""
import math

import numpy as np
import torch

INF, NAN = float("inf"), float("nan")


def _cfg(**kw):
    d = dict(lr=0.01, factor=0.7, patience=7, threshold=1e-4, cooldown=0, min_lr=1e-8, eps=1e-8, control_every=1,
             early_stopping=10 ** 6)
    d.update(kw)
    return d


def _rows(vals):
    """(train, val, test) per epoch from validation losses: the other two only feed the log."""
    return [(2.0 * v + 1.0 if v == v else v, v, 0.5 * v if v == v else 3.0) for v in vals]


REL = 1.0 - 1e-4
EDGE = 1.0 * REL      # exactly best * (1 - threshold) for best = 1.0


def crafted():
    """name -> (scheduler / loop settings, [(train, val, test)])."""
    return {
        # a long plateau: the lr halves every other epoch and ends pinned at min_lr
        "plateau": (_cfg(factor=0.5, patience=1, min_lr=1e-3), _rows([1.0] * 30)),
        # lr - new <= eps: the reduction is due but not taken
        "eps": (_cfg(lr=1.5e-8, factor=0.5, patience=0, min_lr=0.0), _rows([1.0] * 6)),
        # a value exactly at best * (1 - threshold), one ulp below, one ulp above
        "edge_at": (_cfg(patience=3), _rows([1.0, EDGE, EDGE, 2.0])),
        "edge_below": (_cfg(patience=3), _rows([1.0, math.nextafter(EDGE, 0.0), 2.0, 2.0])),
        "edge_above": (_cfg(patience=3), _rows([1.0, math.nextafter(EDGE, 2.0), 2.0, 2.0])),
        "equal": (_cfg(patience=2, early_stopping=4), _rows([0.5] * 12)),
        "nan": (_cfg(patience=1, factor=0.5, early_stopping=5), _rows([1.0, NAN, NAN, 0.9, NAN, NAN, NAN, 0.8, NAN, NAN, NAN, NAN, NAN, NAN, NAN])),
        "nan_first": (_cfg(patience=1, early_stopping=3), _rows([NAN, NAN, 1.0, NAN, NAN, NAN, NAN, NAN])),
        "inf": (_cfg(patience=1, factor=0.5, early_stopping=3), _rows([INF, INF, 1.0, INF, INF, INF, INF, INF, INF])),
        "patience0": (_cfg(patience=0, factor=0.5, min_lr=1e-4), _rows([1.0, 1.0, 0.5, 0.6, 0.7, 0.1, 0.2, 0.3, 0.4])),
        "cooldown": (_cfg(patience=0, factor=0.5, cooldown=2), _rows([1.0] * 12)),
        # the loop's own shape: control every 3rd epoch, the fit ends while epochs are left
        "stop": (_cfg(patience=0, factor=0.5, control_every=3, early_stopping=1), _rows([1.0 + 0.01 * i for i in range(20)])),
        "every5": (_cfg(control_every=5, early_stopping=2, patience=1), _rows([1.0 / (1 + i) if i < 11 else 1.0 for i in range(40)])),
    }


def seeded(n_seq=6, epochs=60):
    out = {}
    for s in range(n_seq):
        rng = np.random.default_rng(1000 + s)
        v = np.abs(1.0 + np.cumsum(rng.normal(0.0, 0.05, epochs)) - 0.01 * np.arange(epochs) * (s % 2))
        v[rng.random(epochs) < 0.03] = NAN
        cfg = _cfg(patience=int(rng.integers(0, 4)), factor=float(rng.choice([0.1, 0.5, 0.7])), cooldown=int(rng.integers(0, 3)),
                   control_every=int(rng.integers(1, 6)), early_stopping=int(rng.integers(1, 6)),
                   min_lr=float(rng.choice([0.0, 1e-8, 1e-3])), lr=float(rng.choice([0.01, 0.05, 1e-3])))
        out[f"seeded{s}"] = (cfg, _rows([float(x) for x in v]))
    return out


def all_sequences():
    d = crafted()
    d.update(seeded())
    return d


def torch_loop(cfg, rows):
    """The example's loop over `rows` with torch's scheduler -> (state after every epoch it ran, the scheduler).  A state:
    lr, sched_best, num_bad_epochs, cooldown_counter, last_epoch, val_best, best_epoch, stall, stopped, snapshot."""
    opt = torch.optim.SGD([torch.nn.Parameter(torch.zeros(1))], lr=cfg["lr"])
    sched = torch.optim.lr_scheduler.ReduceLROnPlateau(opt, mode="min", factor=cfg["factor"], patience=cfg["patience"],
                                                       threshold=cfg["threshold"], cooldown=cfg["cooldown"], min_lr=cfg["min_lr"],
                                                       eps=cfg["eps"])
    val_best, best_epoch, stall, states = INF, 0, 0, []
    for epoch, (_, val, _) in enumerate(rows):
        if stall > cfg["early_stopping"]:
            break
        snapshot = False
        if epoch % cfg["control_every"] == 0:
            sched.step(val)
            if val < val_best:
                val_best, best_epoch, stall, snapshot = val, epoch, 0, True
            else:
                stall += 1
        states.append(dict(lr=float(opt.param_groups[0]["lr"]), sched_best=float(sched.best), num_bad_epochs=sched.num_bad_epochs,
                           cooldown_counter=sched.cooldown_counter, last_epoch=sched.last_epoch, val_best=val_best,
                           best_epoch=best_epoch, stall=stall, stopped=int(stall > cfg["early_stopping"]), snapshot=snapshot))
    return states, sched


def make_control(FitControl, cfg, max_epochs):
    return FitControl(cfg["lr"], cfg["factor"], cfg["patience"], cfg["threshold"], cfg["cooldown"], cfg["min_lr"], cfg["eps"],
                      cfg["control_every"], cfg["early_stopping"], max_epochs)
