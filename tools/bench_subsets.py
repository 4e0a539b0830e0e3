#!/usr/bin/env python3
"""Time `SubsetValues` (a list of subsets of a graph's groups evaluated on chip) and `AttributionCurves` on real-size graphs
(52 and 535 of them) in ONE process, legs alternating.  Atoms are the players of (a), (b) and (e): 57 - 184 groups per graph,
and the rows are those of a deletion and an insertion curve of a random order, about 2 G_g per graph (`rows_per_graph`).

  (a) `SubsetValues.loop`: one masked forward of the whole batch per row, the only way there was.
  (b) `SubsetValues`, the fused call, on the same rows.
  (c) `CoalitionValues` on 6 fragments per graph: 64 masks per graph, the state rebuilt with one application per set group.
  (d) `SubsetValues` on the same 64 rows: the state rebuilt with ONE filtered pass over the member list.  (d) beside (c) is
      what the filtered rebuild costs beside the per-group one (and (c) also derives Shapley values and interactions).
  (e) `AttributionCurves` end to end for that order: the rows built, evaluated, gathered, the areas formed.

Protocol of tools/bench_coalitions.py: warm-up first; then `--windows` rounds of the legs, one call per window,
device-synchronised at both ends; reported: median, p10, p90 over the windows, per call and per evaluation (the evaluation
counts are DERIVED on the host).  For (b), (d) and (e) the time until the call RETURNS is recorded in the same windows: its
share of the synchronised time is the host share of the call (group lists, rows, bit words, job list, every host read).
One JSON line on stdout (and `--out`).

    python tools/bench_subsets.py --out profiles/subsets_bench.json
    rocprofv3 --kernel-trace --stats -d DIR -- python tools/bench_subsets.py --profile-calls 5      # dispatches per fused call
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

from hcatgnet_amd.shapley import CoalitionValues, atom_groups, draw_group_permutations  # noqa: E402
from hcatgnet_amd.subsets import AttributionCurves, SubsetValues  # noqa: E402
from tools.bench_shapley import REAL, commit_hash, make_batch, make_model, stats  # noqa: E402


def timed2(fn):
    """-> (seconds until the call returned, seconds until the device was idle)"""
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    t1 = time.perf_counter()
    torch.cuda.synchronize()
    return t1 - t0, time.perf_counter() - t0


def curve_rows(order, n):
    """The rows `AttributionCurves` builds for `order` (atoms as players, n [B] atoms per graph): row 2 i = the first i + 1
    atoms of the order, row 2 i + 1 = everything else -> (bool [S, G], rows_per_graph [B])"""
    dev = order.device
    B, G = n.numel(), int(order.numel())
    gptr = torch.zeros(B + 1, dtype=torch.int64, device=dev)
    gptr[1:] = n.cumsum(0)
    graph = torch.repeat_interleave(torch.arange(B, device=dev), n, output_size=G)
    pos = torch.empty(G, dtype=torch.int64, device=dev)
    pos[gptr[graph] + order.flatten().long()] = torch.arange(G, device=dev) - gptr[graph]
    rp = 2 * (n - 1).clamp(min=0)
    r = torch.arange(int(rp.max()), device=dev)
    first = pos.unsqueeze(0) < ((r >> 1) + 1).unsqueeze(1)
    rows = torch.where(((r & 1) == 1).unsqueeze(1), ~first, first) & (r.unsqueeze(1) < rp[graph].unsqueeze(0))
    return rows, rp.cpu()


def mask_rows(n, k):
    """bool [2^k, B k]: row s carries the bits of s in every graph's k columns"""
    B = n.numel()
    s = torch.arange(1 << k, device=n.device).unsqueeze(1)
    y = torch.arange(k, device=n.device).repeat(B).unsqueeze(0)
    return ((s >> y) & 1) == 1


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--windows", type=int, default=5)
    ap.add_argument("--graphs", type=int, nargs="+", default=[52, 535])
    ap.add_argument("--nonzero-share", type=float, default=0.2)
    ap.add_argument("--loop-graphs", type=int, nargs="*", default=[52, 535], help="leg (a) runs on the cases with these many graphs")
    ap.add_argument("--commit", default=None, help="commit hash for the record (default: git rev-parse HEAD)")
    ap.add_argument("--out", default=None)
    ap.add_argument("--profile-calls", type=int, default=0, help="only run this many calls of leg (b) on the first case, for a kernel trace")
    a = ap.parse_args()

    model = make_model()
    if a.profile_calls:
        batch = make_batch(a.graphs[0], a.nonzero_share)
        atoms = atom_groups(batch)
        order = draw_group_permutations(batch, atoms, None, n_samples=1, generator=torch.Generator().manual_seed(0))
        rows, rp = curve_rows(order, torch.bincount(batch.batch, minlength=a.graphs[0]))
        sv = SubsetValues(model)
        for _ in range(a.profile_calls):
            sv(batch, rows, node_group=atoms, rows_per_graph=rp)
        torch.cuda.synchronize()
        print(json.dumps(dict(profile_calls=a.profile_calls, graphs=a.graphs[0], rows=int(rows.shape[0]), last_path=sv.last_path)))
        return
    cases = []
    for B in a.graphs:
        batch = make_batch(B, a.nonzero_share)
        n = torch.bincount(batch.batch, minlength=B)
        atoms = atom_groups(batch)
        frag6 = atoms * 6 // n[batch.batch]
        order = draw_group_permutations(batch, atoms, None, n_samples=1, generator=torch.Generator().manual_seed(0))
        rows, rp = curve_rows(order, n)
        rows64 = mask_rows(n, 6)
        sa, sb, sd, cc, ac = SubsetValues(model), SubsetValues(model), SubsetValues(model), CoalitionValues(model), AttributionCurves(model)
        legs = {"b_subsets_atoms": lambda: sb(batch, rows, node_group=atoms, rows_per_graph=rp),
                "c_coalitions_6": lambda: cc(batch, node_group=frag6),
                "d_subsets_6": lambda: sd(batch, rows64, node_group=frag6),
                "e_curves_atoms": lambda: ac(batch, order, node_group=atoms)}
        if B in a.loop_graphs:
            legs = {"a_loop_atoms": lambda: sa.loop(batch, rows, node_group=atoms, rows_per_graph=rp), **legs}
        for fn in legs.values():                         # warm-up: plan, buffers, the LDS attribute of either kernel
            fn()
            fn()
        assert sb.last_path == sd.last_path == cc.last_path == ac.last_path == "fused"
        torch.cuda.synchronize()
        t, ret = {k: [] for k in legs}, {k: [] for k in legs}
        for _ in range(a.windows):
            for k, fn in legs.items():
                back, done = timed2(fn)
                t[k].append(1e3 * done)
                ret[k].append(1e3 * back)
        curve_evals = int(rp.sum()) + 2 * B
        evals = {"a_loop_atoms": curve_evals, "b_subsets_atoms": curve_evals, "c_coalitions_6": 64 * B, "d_subsets_6": 66 * B,
                 "e_curves_atoms": curve_evals}
        rec = dict(graphs=B, nodes=int(batch.x.shape[0]), edges=int(batch.edge_index.shape[1]), max_nodes=int(batch.max_nodes),
                   max_edges=int(batch.max_edges), groups_per_graph=[int(n.min()), int(n.max())], rows=int(rows.shape[0]),
                   live_members=int((batch.x != 0).sum()), lds_bytes=sb.lds_bytes(batch),
                   rows_per_workgroup=dict(b_subsets_atoms=CoalitionValues.default_subsets_per_workgroup(int(rows.shape[0]) * B),
                                           d_subsets_6=CoalitionValues.default_subsets_per_workgroup(64 * B)))
        med = {}
        for k, v in t.items():
            s = stats(v)
            s["evaluations_per_call"] = evals[k]
            s["wall_us_per_evaluation"] = round(1e3 * s["median_ms"] / evals[k], 4)      # (of the whole grid, not of one workgroup)
            if k[0] in "bde":
                h = stats(ret[k])
                s["returned_median_ms"] = h["median_ms"]
                s["host_share"] = round(h["median_ms"] / s["median_ms"], 3)
            rec[k + "_ms_per_call"] = s
            med[k] = s
        if "a_loop_atoms" in med:
            rec["a_over_b"] = round(med["a_loop_atoms"]["median_ms"] / med["b_subsets_atoms"]["median_ms"], 3)
        rec["d_over_c_per_evaluation"] = round(med["d_subsets_6"]["wall_us_per_evaluation"] / med["c_coalitions_6"]["wall_us_per_evaluation"], 3)
        rec["e_over_b"] = round(med["e_curves_atoms"]["median_ms"] / med["b_subsets_atoms"]["median_ms"], 3)
        cases.append(rec)
        print(json.dumps(rec), file=sys.stderr)
    out = dict(bench="subsets", device=torch.cuda.get_device_name(0), commit=a.commit or commit_hash(), graph_shape=REAL,
               nonzero_share=a.nonzero_share, kernels=["k_subset_values", "k_coalition_values"], cases=cases,
               note="one window = one call, the call's host work included (group lists, rows, bit words, job list; (c) also the "
                    "gather to [T, C] and the float64 derivations, (e) also the gather and the areas); ms per call; "
                    "evaluations_per_call is DERIVED on the host, not counted by a kernel ((d): 64 rows and the two appended "
                    "ones); host_share = the time until the call returned over the synchronised time, same windows; not "
                    "measured: the filtered pass alone, the limit shapes (184 nodes, 1024 edges), more than two conv layers")
    line = json.dumps(out)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
