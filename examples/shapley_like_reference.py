#!/usr/bin/env python3
"""Shapley value sampling for every graph of a dataset at once on `hcatgnet_amd.ShapleySampling`.

The reference attributes one molecule at a time with torch_geometric's `Explainer(CaptumExplainer('ShapleyValueSampling'),
node_mask_type='attributes', edge_mask_type='object')` (scripts_experiments/explain_gnn.py): one batch-of-one forward per
feature per permutation.  Here one call walks `--samples` permutations of ALL graphs of the batch on chip, one workgroup per
(graph, permutation), and returns the mean attribution of every node-feature entry and every edge.

This is an EXAMPLE, not a parity claim: no artefact of the reference pins Shapley values (the permutations are random, and
Captum draws them its own way), and neither captum nor torch_geometric is a dependency of this package.

`--players` chooses who is credited (Captum's `feature_mask`): `entries` (every node-feature entry and every directed edge,
the reference's setting), `atoms` (one player per atom, the bonds always present), `atoms+bonds` (atoms and undirected
bonds) or `fragments` (the synthetic graphs get three contiguous node ranges as fragments; all 3! orders are walked, which
is the exact Shapley value for 4 evaluations per order).  With `--coalitions` the fragments go through `CoalitionValues`
instead: every subset of them evaluated once, exact Shapley values and the pairwise interaction matrix from that table.
With `--curves` (`--players atoms`) the atoms are ranked by the call's own attribution and `AttributionCurves` asks the model
how good that ranking is: the mean area under the insertion curve (high is good) and under the deletion curve (low is good),
beside the same two figures for a random order drawn from `--seed`.
With `--greedy` (`--players atoms`) `GreedySelection` finds the model's own greedy insertion and deletion orders of the atoms
(high insertion AUC / low deletion AUC by construction: the practical envelope) and prints, per mode, the mean AUC of the
greedy order beside the sampled-Shapley ranking's and the random order's, all three through `AttributionCurves`.

    python examples/shapley_like_reference.py --graphs 64 --samples 25
    python examples/shapley_like_reference.py --graphs 64 --players fragments
    python examples/shapley_like_reference.py --graphs 64 --players fragments --coalitions
    python examples/shapley_like_reference.py --graphs 64 --players atoms --curves
    python examples/shapley_like_reference.py --graphs 64 --players atoms --greedy
"""
from __future__ import annotations

import argparse
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import hcatgnet_amd as H  # noqa: E402
from hcatgnet_amd import synth  # noqa: E402


def grouped(a, sv, batch):
    """Atoms, bonds or fragments as the players: one attribution per group."""
    n = torch.bincount(batch.batch, minlength=batch.num_graphs)
    atoms = H.atom_groups(batch)
    if a.players == "fragments":
        frag = atoms * 3 // n[batch.batch]                      # three contiguous node ranges per graph
        orders = H.all_group_permutations(batch, frag, None)    # all 3! orders: the exact Shapley value
        r = sv(batch, group_permutations=orders, node_group=frag, class_index=0)
        what = f"all {orders.shape[0]} orders of 3 fragments"
    else:
        bonds = H.bond_groups(batch, first=n) if a.players == "atoms+bonds" else None
        r = sv(batch, n_samples=a.samples, generator=torch.Generator().manual_seed(a.seed), class_index=0, node_group=atoms,
               edge_group=bonds)
        what = f"{a.samples} permutations of {a.players}"
    print(f"path {sv.last_path}: {batch.num_graphs} graphs, {what}, {r.group_attr.numel()} groups")
    # efficiency: a graph's group attributions add up to its prediction minus the prediction with the background only
    graph = torch.repeat_interleave(torch.arange(batch.num_graphs, device=r.group_attr.device), r.group_ptr[1:] - r.group_ptr[:-1])
    total = torch.zeros(batch.num_graphs, device=r.group_attr.device).index_add(0, graph, r.group_attr)
    gap = total - (r.out_full[:, 0] - r.out_base[:, 0])
    print("largest |sum of attributions - (prediction - background-only prediction)|: %.2e" % float(gap.abs().max()))
    g0 = r.group_attr[:int(r.group_ptr[1])]
    print("graph 0, groups by |attribution|:", torch.argsort(g0.abs(), descending=True)[:5].tolist(),
          [round(v, 5) for v in g0[torch.argsort(g0.abs(), descending=True)[:5]].tolist()])
    if a.curves:
        curves(a, sv.model, batch, atoms, r)
    if a.greedy:
        greedy(a, sv.model, batch, atoms, r)


def greedy(a, model, batch, atoms, r):
    """How far is the sampled-Shapley ranking from what the model allows?  The greedy insertion order (always add the atom
    that raises the output most) and the greedy deletion order (always remove the atom that lowers it most) beside the
    ranking and a random order, all three through `AttributionCurves`."""
    gs, ac = H.GreedySelection(model), H.AttributionCurves(model)
    drawn = H.draw_group_permutations(batch, atoms, None, n_samples=1, generator=torch.Generator().manual_seed(a.seed))
    orders = {"atoms ranked by their attribution": H.ranking(r.group_attr, r.group_ptr), "a random order": drawn}
    for mode in ("insertion", "deletion"):
        g = gs(batch, node_group=atoms, class_index=0, mode=mode)
        print(f"greedy {mode}, path {gs.last_path}: {int(g.steps.sum())} picks on {batch.num_graphs} graphs in {gs.launches} launches; "
              f"graph 0's first five: {g.order[0, :5].tolist()}")
        for name, order in {f"the greedy {mode} order": g.order, **orders}.items():
            c = ac(batch, order, node_group=atoms, class_index=0)
            print("  mean %s AUC, %-34s %.5f" % (mode, name + ":", float((c.insertion_auc if mode == "insertion" else c.deletion_auc).mean())))


def curves(a, model, batch, atoms, r):
    """Deletion and insertion curves of the atoms ranked by the attribution just computed, and of a random order."""
    ac = H.AttributionCurves(model)
    mine = ac(batch, H.ranking(r.group_attr, r.group_ptr), node_group=atoms, class_index=0)
    path = ac.last_path
    ins, dele = float(mine.insertion_auc.mean()), float(mine.deletion_auc.mean())
    drawn = H.draw_group_permutations(batch, atoms, None, n_samples=1, generator=torch.Generator().manual_seed(a.seed))
    rand = ac(batch, drawn, node_group=atoms, class_index=0)
    print(f"curves, path {path}: {mine.k.numel()} points on {batch.num_graphs} graphs, two evaluations per interior point")
    print("mean insertion AUC / deletion AUC, atoms ranked by their attribution: %.5f / %.5f" % (ins, dele))
    print("mean insertion AUC / deletion AUC, a random order:                    %.5f / %.5f"
          % (float(rand.insertion_auc.mean()), float(rand.deletion_auc.mean())))


def coalitions(model, batch):
    """Three fragments per graph through the table of all 2^3 subsets: exact Shapley values and who matters together."""
    n = torch.bincount(batch.batch, minlength=batch.num_graphs)
    frag = H.atom_groups(batch) * 3 // n[batch.batch]
    cv = H.CoalitionValues(model)
    r = cv(batch, node_group=frag, class_index=0)
    print(f"path {cv.last_path}: {batch.num_graphs} graphs, {r.values.shape[0]} subsets of 3 fragments evaluated")
    G = int(r.group_ptr[1])
    print("graph 0, output per subset (bit y = fragment y on):", [round(v, 5) for v in r.values[:int(r.table_ptr[1]), 0].tolist()])
    print("graph 0, exact Shapley values:", [round(v, 5) for v in r.group_attr[:G].tolist()])
    print("graph 0, Shapley interaction indices:")
    for row in r.interaction[:int(r.pair_ptr[1])].view(G, G).tolist():
        print("   ", [round(v, 5) for v in row])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--graphs", type=int, default=64)
    ap.add_argument("--samples", type=int, default=25)
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--nonzero-share", type=float, default=0.2, help="share of the node-feature entries kept non-zero (one-hot-like)")
    ap.add_argument("--players", choices=("entries", "atoms", "atoms+bonds", "fragments"), default="entries")
    ap.add_argument("--coalitions", action="store_true", help="with --players fragments: every subset through CoalitionValues")
    ap.add_argument("--curves", action="store_true", help="with --players atoms: deletion / insertion curves of the atoms' ranking")
    ap.add_argument("--greedy", action="store_true", help="with --players atoms: the greedy insertion / deletion orders beside the ranking's AUCs")
    a = ap.parse_args()
    if a.greedy and a.players != "atoms":
        ap.error("--greedy goes with --players atoms")
    if a.coalitions and a.players != "fragments":
        ap.error("--coalitions goes with --players fragments")
    if a.curves and a.players != "atoms":
        ap.error("--curves goes with --players atoms")
    model = H.make_network("GCN", H.default_options(), 25).cuda()
    sb = synth.make_batch(num_graphs=a.graphs, nodes=87, nodes_jitter=30, extra_bonds=4, max_degree=4, feat=25)
    keep = torch.rand(sb.x.shape, generator=torch.Generator().manual_seed(a.seed)) < a.nonzero_share
    sb.x = (sb.x * keep).contiguous()
    batch = sb.as_batch("cuda")

    if a.coalitions:
        return coalitions(model, batch)
    sv = H.ShapleySampling(model)
    if a.players != "entries":
        return grouped(a, sv, batch)
    r = sv(batch, n_samples=a.samples, generator=torch.Generator().manual_seed(a.seed), class_index=0)
    print(f"path {sv.last_path}: {batch.num_graphs} graphs, {a.samples} permutations each")

    # efficiency: a graph's attributions add up to its prediction minus the all-off prediction
    node_sum = torch.zeros(batch.num_graphs, device=batch.x.device).index_add(0, batch.batch, r.node_attr.sum(1))
    edge_sum = torch.zeros(batch.num_graphs, device=batch.x.device).index_add(0, batch.batch[batch.edge_index[1]], r.edge_attr)
    gap = (node_sum + edge_sum) - (r.out_full[:, 0] - r.out_base[:, 0])
    print("largest |sum of attributions - (prediction - baseline prediction)|: %.2e" % float(gap.abs().max()))
    top = torch.topk(r.edge_attr.abs(), min(10, r.edge_attr.numel())).indices.tolist()
    print("ten most important edges (batch edge positions):", top)
    per_feature = r.node_attr.abs().sum(0)
    print("node-feature columns by total |attribution|:", torch.argsort(per_feature, descending=True)[:5].tolist())


if __name__ == "__main__":
    main()
