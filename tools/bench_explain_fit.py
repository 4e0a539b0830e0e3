#!/usr/bin/env python3
"""Time a whole GNNExplainer fit (`hcatgnet_amd.explain.ExplainFit`, 100 epochs) of a batch of real-size graphs in ONE
process, legs alternating, on 52, 535 and 4096 graphs (87 +- 30 nodes, F = 25, 20 % of the entries of x non-zero):

  (a) the loop path: per epoch one `ExplainStep` launch, torch ops for the regularisers' gradients and Adam (`ExplainFit.loop`).
  (b) the one-launch fit: every graph's 100 epochs inside one launch of k_explain_graphs<true>.

`--problem-type classification` (with `--n-classes`, default 3) times the same two legs on a classifier in
`mode="multiclass_classification"` (cross-entropy against the predicted class) and, in the same windows, the two legs of the
regression fit of a one-output model of the same depth (`c_loop_regression`, `d_fused_regression`), so that both objectives
are measured side by side in one process.

Both legs start every call from the same fresh state (nine small device copies, counted in both) and hold the model's own
prediction.  Warm-up first; then `--windows` rounds of the legs, each window device-synchronised at both ends and at least
`--seconds` long; a window's figure is its time per call (one call = the whole fit of every graph); reported: median, p10,
p90 over the windows.  One JSON line on stdout (and `--out`).

    python tools/bench_explain_fit.py --out RECORD.json
    rocprofv3 --kernel-trace --stats -d DIR -- python tools/bench_explain_fit.py --profile-calls 20     # launches per fused call
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
from hcatgnet_amd.explain import ExplainFit  # noqa: E402

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
    ap.add_argument("--epochs", type=int, default=100)
    ap.add_argument("--graphs", type=int, nargs="+", default=[52, 535, 4096])
    ap.add_argument("--out", default=None)
    ap.add_argument("--problem-type", choices=["regression", "classification"], default="regression")
    ap.add_argument("--n-classes", type=int, default=None, help="outputs of the model (default: 1 for regression, 3 for classification)")
    ap.add_argument("--profile-calls", type=int, default=0, help="only this many fused calls on the first batch (for a kernel trace)")
    a = ap.parse_args()

    classify = a.problem_type == "classification"
    n_classes = a.n_classes if a.n_classes is not None else (3 if classify else 1)
    if classify and n_classes < 2:
        ap.error("--problem-type classification needs --n-classes of 2 or more")
    torch.manual_seed(0)
    model = H.make_network("GCN", H.default_options(problem_type=a.problem_type, n_classes=n_classes), 25).cuda().eval()
    fit = ExplainFit(model, epochs=a.epochs, mode="multiclass_classification" if classify else "regression")
    fit_reg = ExplainFit(H.make_network("GCN", H.default_options(), 25).cuda().eval(), epochs=a.epochs) if classify else None
    cases = []
    for B in a.graphs:
        batch = make_batch(B)
        assert fit.reason(batch) is None, fit.reason(batch)
        with torch.no_grad():
            target = model(batch).reshape(B, -1).clone()
            if classify:
                target = target.argmax(dim=1)
                target_reg = fit_reg.model(batch).reshape(B, -1).clone()
        fresh = fit.init_state(batch, torch.Generator().manual_seed(1))
        state = fresh.clone()

        def reset():
            for (_, t), (_, t0) in zip(state.tensors(), fresh.tensors()):
                t.copy_(t0)
            state.step = 0

        def fused():
            reset()
            return fit(batch, target=target, state=state)

        def loop():
            reset()
            return fit.loop(batch, target=target, state=state)

        if a.profile_calls:
            fused()
            torch.cuda.synchronize()
            for _ in range(a.profile_calls):
                fused()
            torch.cuda.synchronize()
            print(json.dumps(dict(profiled_fused_calls=a.profile_calls + 1, path=fit.last_path, graphs=B, epochs=a.epochs)))
            return

        legs = {"a_loop": loop, "b_fused": fused}
        if classify:
            def loop_reg():
                reset()
                return fit_reg.loop(batch, target=target_reg, state=state)

            def fused_reg():
                reset()
                return fit_reg(batch, target=target_reg, state=state)

            fused_reg()
            assert fit_reg.last_path == "fused"
            legs.update(c_loop_regression=loop_reg, d_fused_regression=fused_reg)
        r_loop = loop()
        loop_masks = (r_loop.edge_mask.clone(), r_loop.node_mask.clone())
        assert fit.last_path == "loop"
        r_fused = fused()
        assert fit.last_path == "fused"
        agree = max(float((r_fused.edge_mask - loop_masks[0]).abs().max()), float((r_fused.node_mask - loop_masks[1]).abs().max()))
        torch.cuda.synchronize()
        t = {k: [] for k in legs}
        for _ in range(a.windows):
            for k, fn in legs.items():
                t[k].append(window(fn, a.seconds))
        rec = dict(graphs=B, nodes=int(batch.x.shape[0]), edges=int(batch.edge_index.shape[1]), epochs=a.epochs,
                   masks_max_abs_difference_between_legs=agree)
        rec.update({k: stats(v) for k, v in t.items()})
        rec["b_p90_below_a_p10"] = rec["b_fused"]["p90_us"] < rec["a_loop"]["p10_us"]
        rec["a_over_b_median"] = round(rec["a_loop"]["median_us"] / rec["b_fused"]["median_us"], 2)
        if classify:
            rec["b_over_d_median"] = round(rec["b_fused"]["median_us"] / rec["d_fused_regression"]["median_us"], 3)
        cases.append(rec)
        print(json.dumps(rec), file=sys.stderr)
    out = dict(bench="explain_fit", problem_type=a.problem_type, n_classes=n_classes, device=torch.cuda.get_device_name(0), window_seconds=a.seconds, graph_shape=REAL,
               x_nonzero_share=KEEP, cases=cases,
               note="one call = the whole fit of every graph of the batch from a fresh state; (a) is ExplainFit.loop (one ExplainStep "
                    "launch per epoch plus torch ops), (b) the one-launch kernel; both legs copy the fresh state in first"
                    + ("; (c) / (d) are the same two legs of the regression fit of a one-output model, alternated in the same windows" if classify else ""))
    line = json.dumps(out)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
