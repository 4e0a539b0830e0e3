#!/usr/bin/env python3
"""Time integrated gradients of an ENSEMBLE of models (`hcatgnet_amd.EnsembleAttribution`, 50 Gauss-Legendre points) on a
batch of real-size graphs in ONE process, legs alternating, for M = 9 and 90 models on 52 and 535 graphs (87 +- 30 nodes,
F = 25, 20 % of the entries of x non-zero):

  (a) the loop: `IntegratedGradients(model_k)(batch)` for every model, one launch each, the M results stacked and reduced
      with `torch.mean` / `torch.std(unbiased=False)` over the model axis.
  (b) one `EnsembleAttribution` call: one workgroup per (graph, model), the moments on the device.

Warm-up first; then `--windows` rounds of the legs, each window device-synchronised at both ends and at least `--seconds`
long; a window's figure is its time per call (one call = mean and std of the attributions of every graph over all models);
reported: median, p10, p90 over the windows.  One JSON line on stdout (and `--out`).

    python tools/bench_ensemble_attribution.py --out profiles/ensemble_attribution_bench.json

`--once M B` runs four calls of leg (b) and exits: the program of a `rocprofv3 --kernel-trace --stats` run that counts
the dispatches of a call.
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

REAL = dict(nodes=87, nodes_jitter=30, extra_bonds=4, max_degree=4, feat=25)
KEEP = 0.2


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


def make_batch(B):
    sb = synth.make_batch(num_graphs=B, **REAL)
    sb.x = sb.x * (torch.rand(sb.x.shape, generator=torch.Generator().manual_seed(5)) < KEEP)
    return sb.as_batch("cuda")


def make_models(M):
    # (make_network seeds globally from opt.global_seed: one seed per model, or the M models are one model)
    return [H.make_network("GCN", H.default_options(global_seed=20232023 + k), 25).cuda().eval() for k in range(M)]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--seconds", type=float, default=0.5)
    ap.add_argument("--windows", type=int, default=5)
    ap.add_argument("--steps", type=int, default=50)
    ap.add_argument("--models", type=int, nargs="+", default=[9, 90])
    ap.add_argument("--graphs", type=int, nargs="+", default=[52, 535])
    ap.add_argument("--once", type=int, nargs=2, metavar=("M", "B"), default=None, help="four calls of leg (b) at M models, B graphs, nothing else")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()

    if a.once:
        M, B = a.once
        ea = H.EnsembleAttribution(make_models(M), n_steps=a.steps)
        batch = make_batch(B)
        for _ in range(4):                                  # (the first one allocates the buffers and builds the plan)
            ea(batch)
            torch.cuda.synchronize()
        print(json.dumps(dict(once=True, models=M, graphs=B, path=ea.last_path, calls=4)))
        return

    models = make_models(max(a.models))
    batches = {B: make_batch(B) for B in a.graphs}
    cases = []
    for M in a.models:
        singles = [H.IntegratedGradients(m, n_steps=a.steps) for m in models[:M]]
        ea = H.EnsembleAttribution(models[:M], n_steps=a.steps)
        for B in a.graphs:
            batch = batches[B]
            assert ea.reason(batch) is None, ea.reason(batch)
            N, F, E = batch.x.shape[0], batch.x.shape[1], batch.edge_index.shape[1]
            node = torch.zeros(M, N, F, device="cuda")
            edge = torch.zeros(M, E, device="cuda")
            mom = [torch.zeros(N, F, device="cuda"), torch.zeros(N, F, device="cuda"), torch.zeros(E, device="cuda"), torch.zeros(E, device="cuda")]

            def a_loop():
                for k, ig in enumerate(singles):
                    r = ig(batch)
                    node[k].copy_(r.node_attr)
                    edge[k].copy_(r.edge_attr)
                torch.mean(node, dim=0, out=mom[0])
                torch.std(node, dim=0, unbiased=False, out=mom[1])
                torch.mean(edge, dim=0, out=mom[2])
                torch.std(edge, dim=0, unbiased=False, out=mom[3])

            def b_fused():
                return ea(batch)

            legs = {"a_loop": a_loop, "b_fused": b_fused}
            a_loop()
            assert all(ig.last_path == "fused" for ig in singles)
            r = b_fused()
            assert ea.last_path == "fused"
            scale = max(float(mom[0].abs().max()), float(mom[2].abs().max()), 1e-30)
            agree = max(float((r.node_mean - mom[0]).abs().max()), float((r.edge_mean - mom[2]).abs().max()),
                        float((r.node_std - mom[1]).abs().max()), float((r.edge_std - mom[3]).abs().max())) / scale
            ws_one = int(ea._args.workspace_bytes_needed) // max(int(ea._args.n_models), 1)
            mpl = ea.default_models_per_launch(M, ws_one, N * F + E)
            spl = singles[0].default_steps_per_launch(a.steps, B * mpl)
            torch.cuda.synchronize()
            t = {k: [] for k in legs}
            for _ in range(a.windows):
                for k, fn in legs.items():
                    t[k].append(window(fn, a.seconds))
            rec = dict(models=M, graphs=B, nodes=int(N), edges=int(E), n_steps=a.steps, workgroups=M * B,
                       models_per_launch=mpl, steps_per_launch=spl,
                       path_launches_per_fused_call=-(-M // mpl) * -(-a.steps // spl), moment_launches_per_fused_call=-(-M // mpl),
                       moments_max_difference_between_legs_relative_to_the_largest_mean=agree)
            rec.update({k: stats(v) for k, v in t.items()})
            rec["b_p90_below_a_p10"] = rec["b_fused"]["p90_us"] < rec["a_loop"]["p10_us"]
            rec["a_over_b_median"] = round(rec["a_loop"]["median_us"] / rec["b_fused"]["median_us"], 2)
            cases.append(rec)
            print(json.dumps(rec), file=sys.stderr)
            del node, edge, mom
    out = dict(bench="ensemble_attribution", device=torch.cuda.get_device_name(0), window_seconds=a.seconds, graph_shape=REAL,
               x_nonzero_share=KEEP, method="gausslegendre", cases=cases,
               note="one call = mean and std over the models of the attributions of every graph of the batch; (a) is one "
                    "IntegratedGradients launch per model, two copies per model into the stacked arrays and four torch "
                    "reductions, (b) one EnsembleAttribution call (per_model=False)")
    line = json.dumps(out)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
