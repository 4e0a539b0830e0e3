#!/usr/bin/env python3
"""Dev tool: one whole fit of the reference's regime (scripts_experiments/train_GNN.py:73-111: 535 / 60 / 60 REAL graphs,
batch 40) as the host loop of examples/train_like_reference.py and as `hcatgnet_amd.fit_network` / `fit_networks`, in one
process, the legs alternating after a warm-up fit of each:

  a  the example's host loop (three blocking reads per epoch, torch's scheduler, deepcopy of the best state-dict)
  b  fit_network(lookahead=0)          c  fit_network(lookahead=1)
  d  train_networks + 2 x eval_networks over K runs with the same host control per run          e  fit_networks, K runs

A window is `--fits` consecutive fits of `--epochs` epochs and ends in a device synchronise; early stopping is set out of
reach so every fit runs all its epochs.  Reported per leg: median, p10 and p90 of the windows in ms per epoch (of all K runs
for d and e), and for b, c and e the host time until the enqueue loop returned -- the host / GPU split of an epoch.
usage: python tools/bench_fit.py [--out profiles/fit_bench.json]"""
import argparse
import gc
import json
import os
import sys
import time
from copy import deepcopy

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402
import torch  # noqa: E402

import hcatgnet_amd as H  # noqa: E402
from hcatgnet_amd import synth  # noqa: E402
from hcatgnet_amd.train import eval_network, eval_networks, train_network, train_networks  # noqa: E402

G_TRAIN, G_VAL, BS, NEVER = 535, 60, 40, 10 ** 6


def make_run(k):
    sb = synth.make_config("REAL", num_graphs=G_TRAIN + 2 * G_VAL, seed=synth.BASE_SEED + k)
    graphs = sb.as_graph_list()
    st = [H.DeviceGraphStore(g, device="cuda") for g in (graphs[:G_TRAIN], graphs[G_TRAIN:G_TRAIN + G_VAL], graphs[G_TRAIN + G_VAL:])]
    m = H.make_network("GCN", H.default_options(), 25).cuda()
    return m, H.DeviceLoader(st[0], batch_size=BS, shuffle=True, seed=k), H.DeviceLoader(st[1], batch_size=BS), H.DeviceLoader(st[2], batch_size=BS)


class HostControl:
    """The example's bookkeeping for one run."""

    def __init__(self, model):
        self.model, self.val_best, self.stall, self.best = model, float("inf"), 0, deepcopy(model.state_dict())

    def control(self, val_loss):
        self.model.scheduler.step(val_loss)
        if val_loss < self.val_best:
            self.val_best, self.stall, self.best = val_loss, 0, deepcopy(self.model.state_dict())
        else:
            self.stall += 1


def host_loop(run, epochs, every):
    m, trn, val, tst = run
    hc = HostControl(m)
    for epoch in range(epochs):
        train_network(m, trn, "cuda")
        val_loss = eval_network(m, val, "cuda")
        eval_network(m, tst, "cuda")
        if epoch % every == 0:
            hc.control(val_loss)


def host_loops(runs, epochs, every):
    ms, trn, val, tst = ([r[i] for r in runs] for i in range(4))
    hcs = [HostControl(m) for m in ms]
    for epoch in range(epochs):
        train_networks(ms, trn, "cuda")
        vals = eval_networks(ms, val, "cuda")
        eval_networks(ms, tst, "cuda")
        if epoch % every == 0:
            for hc, v in zip(hcs, vals):
                hc.control(v)


def time_draw(loader, reps=200, windows=5):
    """The draw launch alone (csrc/shuffle.hip) on the loader's store: us per launch, `reps` back to back between two events."""
    from hcatgnet_amd.store import DeviceGenerator
    state = loader.rng.bit_generator.state
    gen = DeviceGenerator(loader).to_device()
    layout = torch.zeros(gen.layout_words(), dtype=torch.int64, device="cuda")
    for _ in range(20):
        gen.draw(layout)
    out = []
    for _ in range(windows):
        t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t0.record()
        for _ in range(reps):
            gen.draw(layout)
        t1.record()
        t1.synchronize()
        out.append(t0.elapsed_time(t1) / reps)
    loader.rng.bit_generator.state = state
    return dict(graphs=len(loader.store), **stats(out, 1e3))


def stats(xs, scale):
    xs = np.asarray(xs) * scale
    return dict(median=round(float(np.median(xs)), 4), p10=round(float(np.percentile(xs, 10)), 4), p90=round(float(np.percentile(xs, 90)), 4))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--epochs", type=int, default=50)
    ap.add_argument("--every", type=int, default=5)
    ap.add_argument("--fits", type=int, default=3, help="fits per timed window")
    ap.add_argument("--windows", type=int, default=5)
    ap.add_argument("--runs", type=int, default=12)
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "fit_bench.json"))
    ap.add_argument("--form", choices=("epoch", "chunk"), default="epoch", help="chunk: two more legs beside a..e, the fits of c "
                    "and e with form='chunk' (f, g), the draw kernel alone, and the record goes to profiles/fit_chunk_bench.json")
    a = ap.parse_args()
    assert torch.cuda.is_available(), "bench_fit.py measures on an MI355X: no GPU visible"
    chunk = a.form == "chunk"
    if chunk and a.out.endswith(os.path.join("profiles", "fit_bench.json")):
        a.out = a.out[:-len("fit_bench.json")] + "fit_chunk_bench.json"
    runs = [make_run(k) for k in range(a.runs)]
    one = runs[0]
    kw = dict(epochs=a.epochs, early_stopping=NEVER, control_every=a.every, load_best=False)
    enq = {"b_fit_lookahead0": [], "c_fit_lookahead1": [], "e_fit_networks": []}
    launches = {}

    def fit(name, lookahead, form="epoch"):
        def leg():
            r = H.fit_network(*one, "cuda", lookahead=lookahead, form=form, **kw)
            assert r.form == ("device" if form == "epoch" else "device-chunk") and r.epochs_run == a.epochs
            enq[name].append(r.enqueue_s)
            launches[name] = r.graph_launches
        return leg

    def fits(name="e_fit_networks", form="epoch"):
        def leg():
            rs = H.fit_networks(*[[r[i] for r in runs] for i in range(4)], "cuda", lookahead=1, form=form, **kw)
            assert all(r.form == ("device" if form == "epoch" else "device-chunk") and r.epochs_run == a.epochs for r in rs)
            enq[name].append(max(r.enqueue_s for r in rs))
            launches[name] = rs[0].graph_launches
        return leg

    legs = {"a_host_loop": lambda: host_loop(one, a.epochs, a.every), "b_fit_lookahead0": fit("b_fit_lookahead0", 0),
            "c_fit_lookahead1": fit("c_fit_lookahead1", 1), "d_train_eval_networks": lambda: host_loops(runs, a.epochs, a.every),
            "e_fit_networks": fits()}
    if chunk:
        enq.update(f_chunk_lookahead1=[], g_chunk_fit_networks=[])
        legs.update(f_chunk_lookahead1=fit("f_chunk_lookahead1", 1, "chunk"),
                    g_chunk_fit_networks=fits("g_chunk_fit_networks", "chunk"))
    for fn in legs.values():                  # warm-up: every window captured, every kernel loaded
        fn()
    torch.cuda.synchronize()
    for v in enq.values():
        v.clear()
    gc.collect()
    gc.freeze()
    t = {k: [] for k in legs}
    for _ in range(a.windows):
        for k, fn in legs.items():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(a.fits):
                fn()
            torch.cuda.synchronize()
            t[k].append((time.perf_counter() - t0) / (a.fits * a.epochs))
    rec = dict(bench="fit", device=torch.cuda.get_device_name(0), graphs=[G_TRAIN, G_VAL, G_VAL], batch_size=BS, epochs=a.epochs,
               control_every=a.every, fits_per_window=a.fits, windows=a.windows, runs_d_e=a.runs, unit="ms per epoch (d, e: of all runs)")
    rec.update({k: stats(v, 1e3) for k, v in t.items()})
    rec["enqueue_ms_per_epoch"] = {k: stats(v, 1e3 / a.epochs) for k, v in enq.items()}
    rec["c_median_above_a_p90"] = rec["c_fit_lookahead1"]["median"] > rec["a_host_loop"]["p90"]
    rec["a_over_c_median"] = round(rec["a_host_loop"]["median"] / rec["c_fit_lookahead1"]["median"], 3)
    rec["d_over_e_median"] = round(rec["d_train_eval_networks"]["median"] / rec["e_fit_networks"]["median"], 3)
    if chunk:
        rec["graph_launches_per_fit"] = launches
        for single, many, key in (("c_fit_lookahead1", "f_chunk_lookahead1", "one_fit"), ("e_fit_networks", "g_chunk_fit_networks", "runs")):
            # faster only where the chunk form's p90 is below the epoch form's p10 of the same run; slower likewise
            rec[f"chunk_faster_{key}"] = rec[many]["p90"] < rec[single]["p10"]
            rec[f"chunk_slower_{key}"] = rec[many]["p10"] > rec[single]["p90"]
            rec[f"epoch_over_chunk_median_{key}"] = round(rec[single]["median"] / rec[many]["median"], 3)
        rec["draw_kernel_us"] = time_draw(one[1])
    rec["note"] = ("every window ends in a device synchronise; enqueue = host time from a fit's set-up to the return of its enqueue "
                   "loop (b waits on every control epoch inside it), e: the longest of the K runs")
    line = json.dumps(rec)
    print(line)
    with open(a.out, "w") as f:
        f.write(line + "\n")


if __name__ == "__main__":
    main()
