#!/usr/bin/env python3
"""Time integrated gradients (`hcatgnet_amd.IntegratedGradients`, 50 Gauss-Legendre points) of a batch of real-size graphs
in ONE process, legs alternating, on 52, 535 and 4096 graphs (87 +- 30 nodes, F = 25, 20 % of the entries of x non-zero):

  (a) the loop path: one `ExplainStep` launch per quadrature point, the weighted sum in torch ops (`IntegratedGradients.loop`).
  (b) the one launch: every graph's 50 points inside one launch of k_explain_graphs<false, true>.
  (c) for scale, on the first batch only: `ShapleySampling` at `--shapley-samples` permutations (default 25), the attribution
      of the same kind the reference's explain stage computes.

Warm-up first; then `--windows` rounds of the legs, each window device-synchronised at both ends and at least `--seconds`
long; a window's figure is its time per call (one call = the whole attribution of every graph); reported: median, p10, p90
over the windows.  One JSON line on stdout (and `--out`).

    python tools/bench_integrated_gradients.py --out profiles/integrated_gradients_bench.json
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--seconds", type=float, default=0.5)
    ap.add_argument("--windows", type=int, default=5)
    ap.add_argument("--steps", type=int, default=50)
    ap.add_argument("--graphs", type=int, nargs="+", default=[52, 535, 4096])
    ap.add_argument("--shapley-samples", type=int, default=25, help="permutations of leg (c) on the first batch; 0: no leg (c)")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()

    torch.manual_seed(0)
    model = H.make_network("GCN", H.default_options(), 25).cuda().eval()
    ig = H.IntegratedGradients(model, n_steps=a.steps)
    sv = H.ShapleySampling(model)
    cases = []
    for i, B in enumerate(a.graphs):
        batch = make_batch(B)
        assert ig.reason(batch) is None, ig.reason(batch)
        legs = {"a_loop": lambda: ig.loop(batch), "b_fused": lambda: ig(batch)}
        if i == 0 and a.shapley_samples > 0:
            perm = H.draw_permutations(batch, 25, a.shapley_samples, torch.Generator().manual_seed(1))
            legs["c_shapley"] = lambda: sv(batch, permutations=perm)
            legs["c_shapley"]()
            assert sv.last_path == "fused"
        r_loop = [t.clone() for t in legs["a_loop"]()]
        assert ig.last_path == "loop"
        r_fused = legs["b_fused"]()
        assert ig.last_path == "fused"
        scale = max(float(r_loop[0].abs().max()), float(r_loop[1].abs().max()), 1e-30)
        agree = max(float((r_fused.node_attr - r_loop[0]).abs().max()), float((r_fused.edge_attr - r_loop[1]).abs().max())) / scale
        torch.cuda.synchronize()
        t = {k: [] for k in legs}
        for _ in range(a.windows):
            for k, fn in legs.items():
                t[k].append(window(fn, a.seconds))
        rec = dict(graphs=B, nodes=int(batch.x.shape[0]), edges=int(batch.edge_index.shape[1]), n_steps=a.steps,
                   launches_per_fused_call=-(-a.steps // ig.default_steps_per_launch(a.steps, B)),
                   attributions_max_difference_between_legs_relative_to_the_largest=agree)
        rec.update({k: stats(v) for k, v in t.items()})
        rec["b_p90_below_a_p10"] = rec["b_fused"]["p90_us"] < rec["a_loop"]["p10_us"]
        rec["a_over_b_median"] = round(rec["a_loop"]["median_us"] / rec["b_fused"]["median_us"], 2)
        if "c_shapley" in rec:
            rec["shapley_samples"] = a.shapley_samples
            rec["c_over_b_median"] = round(rec["c_shapley"]["median_us"] / rec["b_fused"]["median_us"], 1)
        cases.append(rec)
        print(json.dumps(rec), file=sys.stderr)
    out = dict(bench="integrated_gradients", device=torch.cuda.get_device_name(0), window_seconds=a.seconds, graph_shape=REAL,
               x_nonzero_share=KEEP, method="gausslegendre", cases=cases,
               note="one call = the attribution of every graph of the batch; (a) is IntegratedGradients.loop (one ExplainStep launch "
                    "per quadrature point, two mask fills and two weighted adds in torch ops, two forward-only calls), (b) the "
                    "one-launch kernel, (c) ShapleySampling of the same model on the first batch")
    line = json.dumps(out)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
