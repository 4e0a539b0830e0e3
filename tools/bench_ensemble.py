#!/usr/bin/env python3
"""Time ensemble prediction (M models, one shared batch of real-size graphs, outputs + embeddings) in ONE process, legs
alternating, for M = 90 and M = 9 on 52 and on 535 graphs:

  (a) the per-model loop: `model_k(batch, True)` for every k.  `EnsemblePredict` does not change this path, so one build
      measures both sides.
  (b) `EnsemblePredict`, one call (default `models_per_group`).
  (c) (b) at `models_per_group` 1, 2, 4, 8 and M.

Warm-up first; then `--windows` rounds of the legs, each window device-synchronised at both ends and at least `--seconds`
long; a window's figure is its time per call (one call = all M models on the batch); reported: median, p10, p90 over the
windows.  One JSON line on stdout (and `--out`).

    python tools/bench_ensemble.py --out profiles/ensemble_bench.json
    rocprofv3 --kernel-trace --stats -d DIR -- python tools/bench_ensemble.py --profile-calls 20     # launches per fused call
"""
from __future__ import annotations

import argparse
import json
import os
import sys
import time

import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

import hcatgnet_amd as H  # noqa: E402
from hcatgnet_amd import synth  # noqa: E402
from hcatgnet_amd.ensemble import EnsemblePredict, default_models_per_group  # noqa: E402

REAL = dict(nodes=120, extra_bonds=4, max_degree=4, feat=25, nodes_jitter=64)
SWEEP = (1, 2, 4, 8)


def window(fn, seconds):
    """Calls of fn() for at least `seconds`, device-synchronised at both ends -> microseconds per call."""
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    calls = 0
    while True:
        fn()
        calls += 1
        torch.cuda.synchronize()
        dt = time.perf_counter() - t0
        if dt >= seconds:
            return 1e6 * dt / calls


def stats(v):
    t = torch.tensor(sorted(v), dtype=torch.float64)
    q = lambda p: float(torch.quantile(t, p))
    return dict(median_us=round(q(0.5), 2), p10_us=round(q(0.1), 2), p90_us=round(q(0.9), 2), windows=len(v))


def make_models(M):
    torch.manual_seed(0)
    models = [H.make_network("GCN", H.default_options(), 25).cuda().eval() for _ in range(M)]
    with torch.no_grad():
        for m in models:
            for q in m.parameters():
                if q.dim() == 1:
                    q.add_(0.05)
    return models


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--seconds", type=float, default=0.5)
    ap.add_argument("--windows", type=int, default=5)
    ap.add_argument("--models", type=int, nargs="+", default=[90, 9])
    ap.add_argument("--graphs", type=int, nargs="+", default=[52, 535])
    ap.add_argument("--out", default=None)
    ap.add_argument("--profile-calls", type=int, default=0, help="only this many fused calls at M = 90, 52 graphs (for a kernel trace)")
    a = ap.parse_args()

    batches = {B: synth.make_batch(num_graphs=B, **REAL).as_batch("cuda") for B in a.graphs}
    models = make_models(max(a.models))

    if a.profile_calls:
        ens = EnsemblePredict(models[:max(a.models)])
        b = batches[a.graphs[0]]
        ens(b, return_emb=True, stats=False)
        torch.cuda.synchronize()
        for _ in range(a.profile_calls):
            ens(b, return_emb=True, stats=False)
        torch.cuda.synchronize()
        print(json.dumps(dict(profiled_fused_calls=a.profile_calls + 1, path=ens.last_path)))
        return

    cases = []
    for M in a.models:
        ms = models[:M]
        for B in a.graphs:
            batch = batches[B]
            groups = sorted(set(g for g in SWEEP if g <= M) | {M})
            legs = {"a_loop": (lambda ms=ms, batch=batch: [m(batch, True) for m in ms])}
            enss = {"b_fused": EnsemblePredict(ms)}
            for g in groups:
                enss[f"c_group_{g}"] = EnsemblePredict(ms, models_per_group=g)
            for name, ens in enss.items():
                assert ens.reason(batch) is None, ens.reason(batch)
                legs[name] = (lambda ens=ens, batch=batch: ens(batch, return_emb=True, stats=False))
            with torch.no_grad():
                for fn in legs.values():          # warm-up: plans, buffers, the LDS attribute, the allocator's pools
                    for _ in range(3):
                        fn()
                torch.cuda.synchronize()
                assert all(e.last_path == "fused" for e in enss.values())
                t = {k: [] for k in legs}
                for _ in range(a.windows):
                    for k, fn in legs.items():
                        t[k].append(window(fn, a.seconds))
            rec = dict(models=M, graphs=B, default_models_per_group=default_models_per_group(M, B))
            rec.update({k: stats(v) for k, v in t.items()})
            rec["b_p90_below_a_p10"] = rec["b_fused"]["p90_us"] < rec["a_loop"]["p10_us"]
            rec["a_over_b_median"] = round(rec["a_loop"]["median_us"] / rec["b_fused"]["median_us"], 2)
            best = min((k for k in rec if k.startswith("c_group_")), key=lambda k: rec[k]["median_us"])
            rec["best_group"] = int(best[len("c_group_"):])
            cases.append(rec)
            print(json.dumps(rec), file=sys.stderr)
    out = dict(bench="ensemble", device=torch.cuda.get_device_name(0), window_seconds=a.seconds, graph_shape=REAL, cases=cases,
               note="one call = all M models on the batch, outputs + embeddings; (a) runs the per-model path, which the ensemble "
                    "kernel does not change: one build measures every leg")
    line = json.dumps(out)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
