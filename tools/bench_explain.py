#!/usr/bin/env python3
"""Time one explainer iteration (outputs + mask gradients, frozen weights) three ways, in ONE process, legs alternating:

  (a) the any-shape path under autograd: `explain.set_masks` + forward + `backward()` on ONE real-size graph per call, cycling
      over the 40 graphs of the `real-size` batch.  `ExplainStep` does not change this path, so one build measures both sides.
  (b) `ExplainStep` on the same graphs, one per call.
  (c) `ExplainStep` on 535 graphs at once (the reference's training-set size), per call and per graph.

Warm-up first; then `--windows` rounds of a, b, c, each window device-synchronised and at least `--seconds` long; a window's
figure is its time per call; reported: median, p10, p90 over the windows.  One JSON line on stdout (and `--out`).

    python tools/bench_explain.py --out profiles/explain_bench.json
    rocprofv3 --kernel-trace --stats -d DIR -- python tools/bench_explain.py --profile-calls 20     # launches per fused call
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
from hcatgnet_amd.explain import ExplainStep, clear_masks, set_masks  # noqa: E402

REAL = dict(nodes=120, extra_bonds=4, max_degree=4, feat=25, nodes_jitter=64)


def split(sb):
    """A SynthBatch as one-graph GPU batches."""
    out = []
    for g in sb.as_graph_list():
        n, e = g.x.shape[0], g.edge_index.shape[1]
        out.append(H.Batch(g.x.cuda(), g.edge_index.contiguous().cuda(), torch.zeros(n, dtype=torch.long).cuda(), 1,
                           max_nodes=n, max_edges=e, edges_grouped=True))
    return out


def window(fn, seconds):
    """Calls of fn() for at least `seconds`, device-synchronised at both ends -> microseconds per call."""
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    calls = 0
    while True:
        for _ in range(8):
            fn()
        calls += 8
        torch.cuda.synchronize()
        dt = time.perf_counter() - t0
        if dt >= seconds:
            return 1e6 * dt / calls


def stats(v):
    t = torch.tensor(sorted(v), dtype=torch.float64)
    q = lambda p: float(torch.quantile(t, p))
    return dict(median_us=round(q(0.5), 2), p10_us=round(q(0.1), 2), p90_us=round(q(0.9), 2), windows=len(v))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--seconds", type=float, default=1.0)
    ap.add_argument("--windows", type=int, default=7)
    ap.add_argument("--graphs", type=int, default=535)
    ap.add_argument("--out", default=None)
    ap.add_argument("--profile-calls", type=int, default=0, help="only this many fused one-graph calls (for a kernel trace)")
    a = ap.parse_args()

    torch.manual_seed(0)
    model = H.make_network("GCN", H.default_options(), 25).cuda()
    with torch.no_grad():
        for q in model.parameters():
            if q.dim() == 1:
                q.add_(0.05)
    singles = split(synth.make_batch(num_graphs=40, **REAL))
    big = synth.make_batch(num_graphs=a.graphs, **REAL).as_batch("cuda")
    gen = torch.Generator().manual_seed(6)
    masks = [(torch.randn(b.edge_index.shape[1], generator=gen).cuda(), torch.randn(b.x.shape[0], 25, generator=gen).cuda())
             for b in singles]
    ones1 = torch.ones(1, 1).cuda()
    em_big = torch.randn(big.edge_index.shape[1], generator=gen).cuda()
    nm_big = torch.randn(big.x.shape[0], 25, generator=gen).cuda()
    ones_big = torch.ones(big.num_graphs, 1).cuda()
    step1, step_big = ExplainStep(model), ExplainStep(model)
    for b in singles + [big]:
        assert step1.reason(b) is None, step1.reason(b)
    pos = dict(a=0, b=0)

    def leg_a():
        i = pos["a"] = (pos["a"] + 1) % len(singles)
        b, (em, nm) = singles[i], masks[i]
        em_g, nm_g = em.detach().requires_grad_(True), nm.detach().requires_grad_(True)
        set_masks(model, em_g, b.edge_index, apply_sigmoid=True)
        out = model(x=b.x * nm_g.sigmoid(), edge_index=b.edge_index, batch=b.batch)
        out.sum().backward()
        clear_masks(model)
        for q in model.parameters():
            q.grad = None

    def leg_b():
        i = pos["b"] = (pos["b"] + 1) % len(singles)
        step1(singles[i], masks[i][0], masks[i][1], dout=ones1)

    def leg_c():
        step_big(big, em_big, nm_big, dout=ones_big)

    if a.profile_calls:
        leg_b()
        torch.cuda.synchronize()
        for _ in range(a.profile_calls):
            leg_b()
        torch.cuda.synchronize()
        print(json.dumps(dict(profiled_fused_calls=a.profile_calls + 1, path=step1.last_path)))
        return

    for fn in (leg_a, leg_b, leg_c):          # warm-up: plans, buffers, the LDS attribute, the allocator's pools
        for _ in range(60):
            fn()
    torch.cuda.synchronize()
    assert step1.last_path == "fused" and step_big.last_path == "fused"
    t = dict(a=[], b=[], c=[])
    for _ in range(a.windows):
        t["a"].append(window(leg_a, a.seconds))
        t["b"].append(window(leg_b, a.seconds))
        t["c"].append(window(leg_c, a.seconds))
    c = stats(t["c"])
    rec = dict(bench="explain", device=torch.cuda.get_device_name(0), graphs_c=a.graphs, window_seconds=a.seconds,
               a_autograd_one_graph=stats(t["a"]), b_fused_one_graph=stats(t["b"]), c_fused_batch=c,
               c_per_graph_us=dict(median=round(c["median_us"] / a.graphs, 4), p10=round(c["p10_us"] / a.graphs, 4),
                                   p90=round(c["p90_us"] / a.graphs, 4)),
               note="(a) runs the any-shape path, which this kernel does not change: one build measures all three legs")
    rec["b_p90_below_a_p10"] = rec["b_fused_one_graph"]["p90_us"] < rec["a_autograd_one_graph"]["p10_us"]
    rec["c_per_graph_below_b"] = rec["c_per_graph_us"]["median"] < rec["b_fused_one_graph"]["median_us"]
    line = json.dumps(rec)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
