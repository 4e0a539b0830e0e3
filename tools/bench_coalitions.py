#!/usr/bin/env python3
"""Time `CoalitionValues` (every subset of a graph's groups evaluated on chip) against the existing way to the exact Shapley
value, on real-size graphs (52 and 535 of them) in ONE process, legs alternating:

  (a) `ShapleySampling` with `all_group_permutations` on 6 fragments per graph: 720 orders x 6 steps, plus 720 bases.
  (b) `CoalitionValues` on the same groups: 2^6 = 64 masks per graph.
  (c) `CoalitionValues` with 12 fragments per graph: 4096 masks per graph (no permutation walk reaches this).
  (d) `CoalitionValues.loop` (one masked forward of the whole batch per mask index) on the 52 graphs with 6 groups, for scale.

Protocol of tools/bench_shapley_groups.py: warm-up first; then `--windows` rounds of the legs, one call per window,
device-synchronised at both ends; reported: median, p10, p90 over the windows, per call and per evaluation.  The evaluation
counts are DERIVED on the host (live masks for (b), (c), (d); live steps plus bases for (a)), not counted by a kernel.  (a) / (b) in
time stands beside 5 040 / 64 in evaluations; the per-evaluation figure of (b) over that of (a) is where the cost of
rebuilding the state for every mask shows.  One JSON line on stdout (and `--out`).

    python tools/bench_coalitions.py --out profiles/coalitions_bench.json
    rocprofv3 --kernel-trace --stats -d DIR -- python tools/bench_coalitions.py --profile-calls 5      # kernels per fused call
"""
from __future__ import annotations

import argparse
import json
import os
import sys

import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

from hcatgnet_amd._groups import _group_layout  # noqa: E402
from hcatgnet_amd.shapley import CoalitionValues, ShapleySampling, all_group_permutations, atom_groups  # noqa: E402
from tools.bench_shapley import REAL, commit_hash, make_batch, make_model, stats, timed  # noqa: E402


def live_counts(batch, frag):
    """-> per-graph numbers of live groups (host list)"""
    gr = _group_layout(batch, int(batch.x.shape[1]), frag, None)
    B = int(batch.num_graphs)
    graph = torch.repeat_interleave(torch.arange(B, device=frag.device), gr.count)
    return torch.zeros(B, dtype=torch.int64, device=frag.device).index_add_(0, graph, gr.live_group.to(torch.int64)).tolist()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--windows", type=int, default=5)
    ap.add_argument("--graphs", type=int, nargs="+", default=[52, 535])
    ap.add_argument("--nonzero-share", type=float, default=0.2)
    ap.add_argument("--loop-graphs", type=int, default=52, help="leg (d) runs on the case with this many graphs")
    ap.add_argument("--commit", default=None, help="commit hash for the record (default: git rev-parse HEAD)")
    ap.add_argument("--out", default=None)
    ap.add_argument("--profile-calls", type=int, default=0, help="only run this many calls of leg (b) on the first case, for a kernel trace")
    a = ap.parse_args()

    model = make_model()
    if a.profile_calls:
        batch = make_batch(a.graphs[0], a.nonzero_share)
        frag = atom_groups(batch) * 6 // torch.bincount(batch.batch, minlength=a.graphs[0])[batch.batch]
        cv = CoalitionValues(model)
        for _ in range(a.profile_calls):
            cv(batch, node_group=frag)
        torch.cuda.synchronize()
        print(json.dumps(dict(profile_calls=a.profile_calls, graphs=a.graphs[0], last_path=cv.last_path)))
        return
    cases = []
    for B in a.graphs:
        batch = make_batch(B, a.nonzero_share)
        n = torch.bincount(batch.batch, minlength=B)
        ag = atom_groups(batch)
        frag6, frag12 = ag * 6 // n[batch.batch], ag * 12 // n[batch.batch]
        perm = all_group_permutations(batch, frag6, None)
        P = int(perm.shape[0])
        sv, cb, cc, cd = ShapleySampling(model), CoalitionValues(model), CoalitionValues(model), CoalitionValues(model)
        legs = {"a_all_orders_6": lambda: sv(batch, group_permutations=perm, node_group=frag6),
                "b_coalitions_6": lambda: cb(batch, node_group=frag6),
                "c_coalitions_12": lambda: cc(batch, node_group=frag12)}
        if B == a.loop_graphs:
            legs["d_loop_6"] = lambda: cd.loop(batch, node_group=frag6)
        for fn in legs.values():                         # warm-up: plan, buffers, the LDS attribute of either kernel
            fn()
            fn()
        assert sv.last_path == cb.last_path == cc.last_path == "fused"
        torch.cuda.synchronize()
        t = {k: [] for k in legs}
        for _ in range(a.windows):
            for k, fn in legs.items():
                t[k].append(1e3 * timed(fn))
        l6, l12 = live_counts(batch, frag6), live_counts(batch, frag12)
        evals = {"a_all_orders_6": P * (sum(l6) + B), "b_coalitions_6": sum(1 << c for c in l6),
                 "c_coalitions_12": sum(1 << c for c in l12), "d_loop_6": sum(1 << c for c in l6)}
        rec = dict(graphs=B, nodes=int(batch.x.shape[0]), edges=int(batch.edge_index.shape[1]), max_nodes=int(batch.max_nodes),
                   max_edges=int(batch.max_edges), orders=P, lds_bytes=cb.lds_bytes(batch),
                   live_groups=dict(six=[min(l6), max(l6)], twelve=[min(l12), max(l12)]),
                   subsets_per_workgroup=dict(b_coalitions_6=CoalitionValues.default_subsets_per_workgroup(evals["b_coalitions_6"]),
                                              c_coalitions_12=CoalitionValues.default_subsets_per_workgroup(evals["c_coalitions_12"])))
        med = {}
        for k, v in t.items():
            s = stats(v)
            s["evaluations_per_call"] = evals[k]
            s["wall_us_per_evaluation"] = round(1e3 * s["median_ms"] / evals[k], 4)      # (of the whole grid, not of one workgroup)
            rec[k + "_ms_per_call"] = s
            med[k] = s
        ta, tb = med["a_all_orders_6"], med["b_coalitions_6"]
        rec["a_over_b"] = dict(time=round(ta["median_ms"] / tb["median_ms"], 3),
                               evaluations=round(evals["a_all_orders_6"] / evals["b_coalitions_6"], 3),
                               nominal_evaluations="5040 / 64 = 78.75")
        rec["b_over_a_per_evaluation"] = round(tb["wall_us_per_evaluation"] / ta["wall_us_per_evaluation"], 3)
        cases.append(rec)
        print(json.dumps(rec), file=sys.stderr)
    out = dict(bench="coalitions", device=torch.cuda.get_device_name(0), commit=a.commit or commit_hash(), graph_shape=REAL,
               nonzero_share=a.nonzero_share, kernels=["k_shapley_walk", "k_coalition_values"], cases=cases,
               note="one window = one call, host work of the call (group lists, job list, the gather to [T, C] and the float64 "
                    "derivation of Shapley values and interactions) included; ms per call; evaluations_per_call is DERIVED on "
                    "the host, not counted by a kernel; b_over_a_per_evaluation is the per-evaluation wall time of the rebuilt "
                    "state over that of the walked state in the same windows; not measured: the rebuild alone, the limit "
                    "shapes (184 nodes, 1024 edges), more than two conv layers, 13-16 groups")
    line = json.dumps(out)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
