#!/usr/bin/env python3
"""Which atoms does an ENSEMBLE's prediction rest on, and where do its models disagree: `hcatgnet_amd.EnsembleAttribution`.

The reference's last stage predicts an unseen set with all 90 models of its nested cross-validation
(scripts_experiments/predict_test.py; here `EnsemblePredict`), and its explain stage attributes one model and one molecule
at a time (scripts_experiments/explain_gnn.py).  This example joins the two: one call runs integrated gradients of EVERY
model on EVERY graph of the dataset -- one workgroup per (graph, model) of one launch -- and returns the mean over the
models, which is the integrated gradient of the ensemble's mean prediction, and the standard deviation over the models.

The models are loaded from `--weights` (state dicts saved with `torch.save(model.state_dict(), path)`) or, without it,
`--models` models are trained for `--train-steps` steps each from their own initialisation on the synthetic batch's labels.

This is an EXAMPLE, not a parity claim: neither captum nor torch_geometric is a dependency of this package, and no artefact
of the reference pins these values.

    python examples/ensemble_attribution_like_reference.py --models 9 --graphs 52 --steps 50

`--method shapley --players atoms|fragments` explains the same joint prediction with the reference's other algorithm, Shapley
value sampling (`EnsembleShapley`: one set of permutations for all models); `--curves` asks the ensemble itself which ranking
to believe: deletion / insertion AUCs of its MEAN output (`EnsembleCurves`) for the Shapley ranking, the integrated-gradients
ranking (`group_scores` of `EnsembleAttribution`'s means) and a random order.

    python examples/ensemble_attribution_like_reference.py --models 9 --graphs 52 --method shapley --players atoms --curves
"""
from __future__ import annotations

import argparse
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import hcatgnet_amd as H  # noqa: E402
from hcatgnet_amd import synth  # noqa: E402
from hcatgnet_amd.train import FusedTrainStep  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--models", type=int, default=9)
    ap.add_argument("--graphs", type=int, default=52)
    ap.add_argument("--steps", type=int, default=50, help="quadrature points of the path")
    ap.add_argument("--method", default="gausslegendre", choices=["gausslegendre", "riemann_middle", "gradient", "shapley"],
                    help="a quadrature of the integrated-gradients path, or 'shapley': Shapley value sampling of the ensemble (`EnsembleShapley`)")
    ap.add_argument("--players", default="atoms", choices=["atoms", "fragments"], help="--method shapley / --curves: the players (fragments: 3 per graph)")
    ap.add_argument("--permutations", type=int, default=25, help="--method shapley: sampled orders of the players")
    ap.add_argument("--curves", action="store_true", help="deletion / insertion AUCs of the ensemble's MEAN output for the Shapley ranking, "
                                                          "the integrated-gradients ranking and a random order (`EnsembleCurves`)")
    ap.add_argument("--weights", nargs="*", default=None, help="saved state dicts, one per model; default: train on the synthetic labels")
    ap.add_argument("--train-steps", type=int, default=30)
    ap.add_argument("--top", type=int, default=3, help="atoms printed per graph")
    ap.add_argument("--show", type=int, default=8, help="graphs printed")
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--nonzero-share", type=float, default=0.2, help="share of the node-feature entries kept non-zero (one-hot-like)")
    a = ap.parse_args()
    torch.manual_seed(a.seed)
    sb = synth.make_batch(num_graphs=a.graphs, nodes=87, nodes_jitter=30, extra_bonds=4, max_degree=4, feat=25)
    keep = torch.rand(sb.x.shape, generator=torch.Generator().manual_seed(a.seed)) < a.nonzero_share
    sb.x = (sb.x * keep).contiguous()
    batch = sb.as_batch("cuda")
    models = []
    if a.weights:
        for path in a.weights:
            m = H.make_network("GCN", H.default_options(), 25).cuda()
            m.load_state_dict(torch.load(path, map_location="cuda"))
            models.append(m.eval())
        print(f"{len(models)} models from {len(a.weights)} files")
    else:
        for k in range(a.models):
            # (make_network seeds globally from opt.global_seed: every model gets its own initialisation)
            m = H.make_network("GCN", H.default_options(global_seed=a.seed + 1 + k), 25).cuda()
            step = FusedTrainStep(m)
            losses = [float(step(batch)) for _ in range(a.train_steps)]
            models.append(m.eval())
            if losses:
                print(f"model {k}: trained {a.train_steps} steps on the synthetic labels: loss {losses[0]:.4f} -> {losses[-1]:.4f}")

    ag = H.atom_groups(batch)
    sizes = torch.bincount(batch.batch, minlength=batch.num_graphs)
    players = ag if a.players == "atoms" else ag * 3 // sizes[batch.batch]
    if a.method == "shapley" or a.curves:
        # Shapley values are linear in the output: the mean over the models IS the sampled Shapley value of the mean prediction
        es = H.EnsembleShapley(models)
        rs = es(batch, n_samples=a.permutations, generator=torch.Generator().manual_seed(a.seed), node_group=players)
        gp = rs.group_ptr.cpu().tolist()
        print(f"path {es.last_path}: Shapley value sampling of {len(models)} models x {batch.num_graphs} graphs, {a.permutations} shared "
              f"permutations of {gp[-1]} {a.players}")
        for g in range(min(a.show, batch.num_graphs)):
            mean_g, std_g = rs.group_mean[gp[g]:gp[g + 1]].cpu(), rs.group_std[gp[g]:gp[g + 1]].cpu()
            idx = torch.topk(mean_g.abs(), min(a.top, mean_g.numel())).indices
            print(f"graph {g}: " + ", ".join(f"{a.players[:-1]} {int(i)} ({float(mean_g[i]):+.3e} +- {float(std_g[i]):.1e})" for i in idx))
    if a.curves:
        ig = H.EnsembleAttribution(models, n_steps=a.steps, method="gausslegendre" if a.method == "shapley" else a.method)
        ri = ig(batch, class_index=0)
        scores, _ = H.group_scores(ri.node_mean, ri.edge_mean, players, None, batch)
        rand = torch.rand(int(rs.group_mean.numel()), generator=torch.Generator().manual_seed(a.seed + 7)).to(scores.device)
        ec = H.EnsembleCurves(models)
        print(f"mean AUC over the graphs of the ensemble's mean output (insertion: higher is better for a positive prediction; path {ig.last_path}):")
        for label, sc in (("ensemble Shapley", rs.group_mean), ("ensemble integrated gradients", scores), ("random order", rand)):
            rc = ec(batch, H.ranking(sc, rs.group_ptr), node_group=players)
            print(f"  {label:32s} insertion {float(rc.insertion_auc.mean()):+.4f}  deletion {float(rc.deletion_auc.mean()):+.4f}  "
                  f"largest std over the models on a curve {float(torch.maximum(rc.insertion_std.max(), rc.deletion_std.max())):.3e}")
        print(f"path {ec.last_path}: every subset of both curves evaluated by every model in one call per ranking")
    if a.method == "shapley":
        return
    ea = H.EnsembleAttribution(models, n_steps=a.steps, method=a.method)
    r = ea(batch, class_index=0)
    print(f"path {ea.last_path}: {len(models)} models x {batch.num_graphs} graphs, {ea.n_steps} point(s) of {a.method} each, one call")
    ens = H.EnsemblePredict(models)(batch)
    print("largest |mean of out_full - EnsemblePredict.mean|: %.2e" % float((r.out_full.mean(0) - ens.mean).abs().max()))

    # an atom's importance: its node-feature attributions plus half of each of its edges' (both directions count once);
    # the spread is carried the same way (an upper bound of the atom's own std: the terms are not independent)
    def per_atom(node, edge):
        v = node.sum(1)
        return v.index_add(0, batch.edge_index[0], 0.5 * edge).index_add(0, batch.edge_index[1], 0.5 * edge).cpu()

    mean, std = per_atom(r.node_mean, r.edge_mean), per_atom(r.node_std, r.edge_std)
    first = torch.zeros(batch.num_graphs + 1, dtype=torch.long)
    first[1:] = torch.bincount(batch.batch.cpu(), minlength=batch.num_graphs).cumsum(0)
    for g in range(min(a.show, batch.num_graphs)):
        lo, hi = int(first[g]), int(first[g + 1])
        k = min(a.top, hi - lo)
        idx = torch.topk(mean[lo:hi].abs(), k).indices
        line = ", ".join(f"atom {int(i)} ({float(mean[lo + int(i)]):+.3e} +- {float(std[lo + int(i)]):.1e})" for i in idx)
        print(f"graph {g} ({hi - lo} atoms, ensemble prediction {float(ens.mean[g, 0]):+.4f} +- {float(ens.std[g, 0]):.4f}): {line}")
    share = float((r.node_std > r.node_mean.abs()).sum()) / max(int((r.node_mean != 0).sum()), 1)
    print(f"node-feature entries whose std over the models exceeds |mean|: {100 * share:.1f} % of the non-zero ones")


if __name__ == "__main__":
    main()
