#!/usr/bin/env python3
"""Time the Shapley family of an ENSEMBLE of models (`hcatgnet_amd.EnsembleShapley`, `EnsembleSubsetValues`) against the loop
over the single-model classes, in ONE process, legs alternating, for M = 9 and 90 models on 52 and 535 real-size graphs
(87 +- 30 nodes, F = 25, 20 % of the entries of x non-zero), atoms as players:

  (a) the loop: `ShapleySampling(model_k)(batch, group_permutations=...)` for every model, the M group attributions stacked
      and reduced with `torch.mean` / `torch.std(unbiased=False)`.
  (b) one `EnsembleShapley` call on the same 25 permutations (per_model=False): the moments on the device.
  (c) the loop: `SubsetValues(model_k)(batch, rows, rows_per_graph=...)` for every model, stacked, mean / std with torch.
  (d) one `EnsembleSubsetValues` call on the same rows: the rows of both curves of a random order of the atoms.
  (s) / (p), with `--parent-lib PATH`: ONE model's `ShapleySampling` (atoms) and `SubsetValues` call on this build and on the
      library built from the parent commit, loaded into this process: what the model axis costs the single-model classes.

Warm-up first; then `--windows` rounds of the legs, each window device-synchronised at both ends and at least `--seconds`
long; a window's figure is its time per call; reported: median, p10, p90 over the windows.  One JSON line on stdout (and
`--out`).

    python tools/bench_ensemble_shapley.py --out profiles/ensemble_shapley_bench.json
"""
from __future__ import annotations

import argparse
import json
import os
import sys

import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

import hcatgnet_amd as H  # noqa: E402
from hcatgnet_amd._groups import _group_layout  # noqa: E402
from hcatgnet_amd.subsets import AttributionCurves, ranking  # noqa: E402
from tools.bench_ensemble_attribution import REAL, KEEP, make_batch, make_models, stats, window  # noqa: E402
from tools.bench_shapley import commit_hash  # noqa: E402
from tools.bench_shapley_groups import load_other, use_lib  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--seconds", type=float, default=0.5)
    ap.add_argument("--windows", type=int, default=5)
    ap.add_argument("--permutations", type=int, default=25)
    ap.add_argument("--models", type=int, nargs="+", default=[9, 90])
    ap.add_argument("--graphs", type=int, nargs="+", default=[52, 535])
    ap.add_argument("--parent-lib", default=None, help="libhcatgnet_hip.so built from the parent commit: adds the legs (s) / (p)")
    ap.add_argument("--parent-commit", default=None)
    ap.add_argument("--commit", default=None)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()

    models = make_models(max(a.models))
    parent = load_other(a.parent_lib) if a.parent_lib else None
    P = a.permutations
    setups = {}
    for B in a.graphs:
        batch = make_batch(B)
        ag = H.atom_groups(batch)
        perm = H.draw_group_permutations(batch, node_group=ag, n_samples=P, generator=torch.Generator().manual_seed(1))
        gr = _group_layout(batch, 25, ag, None)
        counts = (gr.group_ptr[1:] - gr.group_ptr[:-1]).tolist()
        order = ranking(torch.randn(gr.G, generator=torch.Generator().manual_seed(2)).cuda(), gr.group_ptr)
        plan = AttributionCurves._plan(gr, counts, order, None, batch.x.device)
        setups[B] = (batch, ag, perm, gr.G, plan.rows, torch.tensor(plan.rows_per_graph))

    cases, single = [], []
    if parent is not None:
        for B in a.graphs:
            batch, ag, perm, G, rows, rp = setups[B]
            sw, sp_, vw, vp = (H.ShapleySampling(models[0]), H.ShapleySampling(models[0]), H.SubsetValues(models[0]), H.SubsetValues(models[0]))

            def on_parent(fn):
                def run():
                    with use_lib(parent):
                        fn()
                return run
            legs = {"s_walk": lambda: sw(batch, group_permutations=perm, node_group=ag),
                    "p_walk_parent": on_parent(lambda: sp_(batch, group_permutations=perm, node_group=ag)),
                    "s_rows": lambda: vw(batch, rows, node_group=ag, rows_per_graph=rp),
                    "p_rows_parent": on_parent(lambda: vp(batch, rows, node_group=ag, rows_per_graph=rp))}
            for fn in legs.values():
                fn()
                fn()
            mine = [sw(batch, group_permutations=perm, node_group=ag).group_attr.clone(),
                    vw(batch, rows, node_group=ag, rows_per_graph=rp).values.clone()]
            with use_lib(parent):
                same = torch.equal(mine[0], sp_(batch, group_permutations=perm, node_group=ag).group_attr) and \
                    torch.equal(mine[1], vp(batch, rows, node_group=ag, rows_per_graph=rp).values)
            torch.cuda.synchronize()
            t = {k: [] for k in legs}
            for _ in range(a.windows):
                for k, fn in legs.items():
                    t[k].append(window(fn, a.seconds))
            rec = dict(graphs=B, groups=G, rows=int(rows.shape[0]), permutations=P, bitwise_the_parents_values=same)
            rec.update({k: stats(v) for k, v in t.items()})
            for what in ("walk", "rows"):
                s, p = rec["s_" + what], rec["p_" + what + "_parent"]
                rec[what + "_vs_parent"] = dict(median_ratio=round(s["median_us"] / p["median_us"], 4),
                                                median_inside_the_parents_p10_p90=p["p10_us"] <= s["median_us"] <= p["p90_us"],
                                                spreads_overlap=s["p10_us"] <= p["p90_us"] and p["p10_us"] <= s["p90_us"])
            single.append(rec)
            print(json.dumps(rec), file=sys.stderr)

    for M in a.models:
        walks = [H.ShapleySampling(m) for m in models[:M]]
        subs = [H.SubsetValues(m) for m in models[:M]]
        es, ev = H.EnsembleShapley(models[:M]), H.EnsembleSubsetValues(models[:M])
        for B in a.graphs:
            batch, ag, perm, G, rows, rp = setups[B]
            assert es.reason(batch) is None, es.reason(batch)
            S, C = int(rows.shape[0]), 1
            attr = torch.zeros(M, G, device="cuda")
            vals = torch.zeros(M, S + 2, B, C, device="cuda")
            mom = [torch.zeros(G, device="cuda"), torch.zeros(G, device="cuda"),
                   torch.zeros(S + 2, B, C, device="cuda"), torch.zeros(S + 2, B, C, device="cuda")]

            def a_loop():
                for k, sv in enumerate(walks):
                    attr[k].copy_(sv(batch, group_permutations=perm, node_group=ag).group_attr)
                torch.mean(attr, dim=0, out=mom[0])
                torch.std(attr, dim=0, unbiased=False, out=mom[1])

            def b_fused():
                return es(batch, group_permutations=perm, node_group=ag)

            def c_loop():
                for k, sv in enumerate(subs):
                    r = sv(batch, rows, node_group=ag, rows_per_graph=rp)
                    vals[k, :S].copy_(r.values)
                    vals[k, S].copy_(r.out_full)
                    vals[k, S + 1].copy_(r.out_base)
                torch.mean(vals, dim=0, out=mom[2])
                torch.std(vals, dim=0, unbiased=False, out=mom[3])

            def d_fused():
                return ev(batch, rows, node_group=ag, rows_per_graph=rp)

            legs = {"a_loop": a_loop, "b_fused": b_fused, "c_loop": c_loop, "d_fused": d_fused}
            for fn in legs.values():
                fn()
            assert all(q.last_path == "fused" for q in walks + subs + [es, ev])
            rb, rd = b_fused(), d_fused()
            agree_walk = float((rb.group_mean - mom[0]).abs().max()) / max(float(mom[0].abs().max()), 1e-30)
            agree_rows = float((rd.mean - mom[2][:S]).abs().max()) / max(float(mom[2].abs().max()), 1e-30)
            torch.cuda.synchronize()
            t = {k: [] for k in legs}
            for _ in range(a.windows):
                for k, fn in legs.items():
                    t[k].append(window(fn, a.seconds))
            rec = dict(models=M, graphs=B, nodes=int(batch.x.shape[0]), edges=int(batch.edge_index.shape[1]), groups=G, permutations=P,
                       subset_rows=S, walk_workgroups_per_call=M * B * P,
                       means_max_difference_between_legs_relative_to_the_largest_mean=dict(walk=agree_walk, rows=agree_rows))
            rec.update({k: stats(v) for k, v in t.items()})
            for one, loop, name in (("b_fused", "a_loop", "walk"), ("d_fused", "c_loop", "rows")):
                rec[name] = dict(one_call_p90_below_loop_p10=rec[one]["p90_us"] < rec[loop]["p10_us"],
                                 loop_over_one_call_median=round(rec[loop]["median_us"] / rec[one]["median_us"], 2))
            cases.append(rec)
            print(json.dumps(rec), file=sys.stderr)
            del attr, vals, mom
    out = dict(bench="ensemble_shapley", device=torch.cuda.get_device_name(0), commit=a.commit or commit_hash(),
               parent_commit=a.parent_commit, window_seconds=a.seconds, graph_shape=REAL, x_nonzero_share=KEEP, players="atoms",
               cases=cases, single_model_vs_parent=single,
               note="one call = mean and std over the models, host work of the call included; (a) / (c) are one single-model call "
                    "per model, copies into the stacked arrays and two torch reductions, (b) / (d) one ensemble call "
                    "(per_model=False); not measured: per_model=True, fragments or bonds as players, more than two conv layers, "
                    "the limit shapes, a loop over a group of models inside a workgroup")
    line = json.dumps(out)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
