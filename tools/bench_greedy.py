#!/usr/bin/env python3
"""Time `GreedySelection` (the greedy insertion order of a graph's groups, one launch per round, the winner picked on chip)
against its own loop path on real-size graphs (52 and 535 of them) in ONE process, legs alternating.  Atoms are the players:
57 - 184 groups per graph.

  (a) `GreedySelection.loop`: one `SubsetValues` call per round (that class's fused kernel), the pick with torch ops; every
      round pays that call's host work: the rows, the bit words, the job list.
  (b) `GreedySelection`, the fused call: the layout built once, one launch per round, no host read in between.
Both run a full insertion run (`full`) and the top-10 run (`steps=10`, `top10`).  (b)'s full run is repeated over `ids_per_job`
(`--sweep`) beside the default.

Protocol of tools/bench_subsets.py: warm-up first; then `--windows` rounds of the legs, one call per window,
device-synchronised at both ends; reported: median, p10, p90 over the windows, per call; the launches per call are the host's
count (`launches`), the candidate evaluations per call are DERIVED on the host from the live counts.  For (b) the time until
the call RETURNS is recorded in the same windows.  One JSON line on stdout (and `--out`).

    python tools/bench_greedy.py --out profiles/greedy_bench.json
"""
from __future__ import annotations

import argparse
import json
import os
import sys

import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

from hcatgnet_amd.greedy import GreedySelection  # noqa: E402
from hcatgnet_amd.shapley import atom_groups  # noqa: E402
from tools.bench_shapley import REAL, commit_hash, make_batch, make_model, stats  # noqa: E402
from tools.bench_subsets import timed2  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--windows", type=int, default=5)
    ap.add_argument("--graphs", type=int, nargs="+", default=[52, 535])
    ap.add_argument("--nonzero-share", type=float, default=0.2)
    ap.add_argument("--sweep", type=int, nargs="*", default=[1, 4, 16], help="ids_per_job of leg (b)'s full run, beside the default")
    ap.add_argument("--top", type=int, default=10)
    ap.add_argument("--commit", default=None, help="commit hash for the record (default: git rev-parse HEAD)")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()

    model = make_model()
    cases = []
    for B in a.graphs:
        batch = make_batch(B, a.nonzero_share)
        atoms = atom_groups(batch)
        ga, gb = GreedySelection(model), GreedySelection(model)
        probe = gb(batch, node_group=atoms)
        assert gb.last_path == "fused"
        live = (probe.order[0] >= 0).to(torch.int64)                       # (a full run lists every group; dead ones carry no evaluation)
        L = torch.bincount(batch.batch, minlength=B)                       # atoms per graph = groups per graph
        gr_live = [int(v) for v in gb._layout(batch, atoms, None, None)[3]]
        launches = {}

        def fused(name, **kw):
            def run():
                gb(batch, node_group=atoms, **kw)
                launches[name] = gb.launches
            return run
        legs = {"a_loop_full": lambda: ga.loop(batch, node_group=atoms),
                "b_fused_full": fused("b_fused_full"),
                "a_loop_top": lambda: ga.loop(batch, node_group=atoms, steps=a.top),
                "b_fused_top": fused("b_fused_top", steps=a.top)}
        for ipj in a.sweep:
            legs[f"b_fused_full_ids_{ipj}"] = fused(f"b_fused_full_ids_{ipj}", ids_per_job=ipj)
        for fn in legs.values():                         # warm-up: plan, buffers, the LDS attribute of either kernel
            fn()
            fn()
        assert gb.last_path == "fused" and ga.last_path == "loop" and ga.values.last_path == "fused"
        same = all(torch.equal(p, q) for p, q in zip(ga.loop(batch, node_group=atoms), gb(batch, node_group=atoms)))
        torch.cuda.synchronize()
        t, ret = {k: [] for k in legs}, {k: [] for k in legs}
        for _ in range(a.windows):
            for k, fn in legs.items():
                back, done = timed2(fn)
                t[k].append(1e3 * done)
                ret[k].append(1e3 * back)
        ev_full = sum(c * (c + 1) // 2 for c in gr_live)
        ev_top = sum(sum(c - k for k in range(min(a.top, c))) for c in gr_live)
        rec = dict(graphs=B, nodes=int(batch.x.shape[0]), edges=int(batch.edge_index.shape[1]), max_nodes=int(batch.max_nodes),
                   max_edges=int(batch.max_edges), groups_per_graph=[int(L.min()), int(L.max())],
                   live_groups_per_graph=[min(gr_live), max(gr_live)], filled=int(live.sum()), lds_bytes=gb.lds_bytes(batch),
                   default_ids_per_job=GreedySelection.default_ids_per_job(sum(gr_live)), loop_and_fused_bitwise_equal=bool(same))
        med = {}
        for k, v in t.items():
            s = stats(v)
            s["candidate_evaluations_per_call"] = ev_top if k.endswith("_top") else ev_full
            if k[0] == "b":
                s["launches_per_call"] = launches[k]
                s["returned_median_ms"] = stats(ret[k])["median_ms"]
            else:
                s["subset_calls_per_call"] = (min(a.top, max(gr_live)) if k.endswith("_top") else max(gr_live))
            rec[k + "_ms_per_call"] = s
            med[k] = s["median_ms"]
        rec["a_over_b_full"] = round(med["a_loop_full"] / med["b_fused_full"], 3)
        rec["a_over_b_top"] = round(med["a_loop_top"] / med["b_fused_top"], 3)
        cases.append(rec)
        print(json.dumps(rec), file=sys.stderr)
    out = dict(bench="greedy", device=torch.cuda.get_device_name(0), commit=a.commit or commit_hash(), graph_shape=REAL,
               nonzero_share=a.nonzero_share, kernels=["k_greedy_round", "k_subset_values"], mode="insertion", top=a.top, cases=cases,
               note="one window = one call, the call's host work included (group lists, job lists and their upload for (b); per "
                    "round the rows, bit words, job list and the torch pick for (a)); ms per call; launches_per_call is the host's "
                    "count, candidate_evaluations_per_call is DERIVED on the host from the live counts, not counted by a kernel; "
                    "returned_median_ms = the time until the call returned, same windows; not measured: deletion runs, a kernel "
                    "trace of k_greedy_round alone, the pick's share of a launch, the limit shapes (184 nodes, 1024 edges), more "
                    "than two conv layers, bonds or fragments as players")
    line = json.dumps(out)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
