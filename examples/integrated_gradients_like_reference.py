#!/usr/bin/env python3
"""Integrated gradients for every graph of a dataset at once on `hcatgnet_amd.IntegratedGradients`.

The reference attributes one molecule at a time through torch_geometric's `Explainer(CaptumExplainer(...),
node_mask_type='attributes', edge_mask_type='object')` (scripts_experiments/explain_gnn.py, with
`'ShapleyValueSampling'`).  The same entry point takes `'IntegratedGradients'`: attributions of the same kind for
`--steps` forward and backward passes per graph.  Here one call runs the whole path of ALL graphs of the batch in one
launch, one workgroup per graph, and returns one value per node-feature entry and per edge.

The model is loaded from `--weights` (a state dict saved with `torch.save(model.state_dict(), path)`) or, without it,
trained for `--train-steps` steps on the synthetic batch's own labels, so that there is something to attribute.

This is an EXAMPLE, not a parity claim: neither captum nor torch_geometric is a dependency of this package, and no
artefact of the reference pins these values.

    python examples/integrated_gradients_like_reference.py --graphs 64 --steps 50
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
    ap.add_argument("--graphs", type=int, default=64)
    ap.add_argument("--steps", type=int, default=50, help="quadrature points of the path")
    ap.add_argument("--method", default="gausslegendre", choices=["gausslegendre", "riemann_middle", "gradient"])
    ap.add_argument("--weights", default=None, help="a saved state dict; default: train on the synthetic labels")
    ap.add_argument("--train-steps", type=int, default=50)
    ap.add_argument("--top", type=int, default=3, help="atoms printed per graph")
    ap.add_argument("--show", type=int, default=8, help="graphs printed")
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--nonzero-share", type=float, default=0.2, help="share of the node-feature entries kept non-zero (one-hot-like)")
    a = ap.parse_args()
    torch.manual_seed(a.seed)
    model = H.make_network("GCN", H.default_options(), 25).cuda()
    sb = synth.make_batch(num_graphs=a.graphs, nodes=87, nodes_jitter=30, extra_bonds=4, max_degree=4, feat=25)
    keep = torch.rand(sb.x.shape, generator=torch.Generator().manual_seed(a.seed)) < a.nonzero_share
    sb.x = (sb.x * keep).contiguous()
    batch = sb.as_batch("cuda")
    if a.weights:
        model.load_state_dict(torch.load(a.weights, map_location="cuda"))
        print(f"weights from {a.weights}")
    else:
        step = FusedTrainStep(model)
        losses = [float(step(batch)) for _ in range(a.train_steps)]
        if losses:
            print(f"trained {a.train_steps} steps on the synthetic labels: loss {losses[0]:.4f} -> {losses[-1]:.4f}")
    model.eval()

    ig = H.IntegratedGradients(model, n_steps=a.steps, method=a.method)
    r = ig(batch, class_index=0)
    print(f"path {ig.last_path}: {batch.num_graphs} graphs, {ig.n_steps} point(s) of {a.method} each, one call")

    # completeness is a diagnostic here, not an identity: the path crosses many LeakyReLU / max-pool kinks
    delta = ig.convergence_delta(batch, r)
    change = (r.out_full[:, 0] - r.out_base[:, 0]).double()
    print("largest |sum of attributions - (prediction - baseline prediction)|: %.2e  (largest |prediction - baseline|: %.2e)"
          % (float(delta.abs().max()), float(change.abs().max())))

    # an atom's importance: its node-feature attributions plus half of each of its edges' (both directions count once)
    atom = r.node_attr.sum(1)
    atom = atom.index_add(0, batch.edge_index[0], 0.5 * r.edge_attr).index_add(0, batch.edge_index[1], 0.5 * r.edge_attr)
    first = torch.zeros(batch.num_graphs + 1, dtype=torch.long)
    first[1:] = torch.bincount(batch.batch.cpu(), minlength=batch.num_graphs).cumsum(0)
    atom = atom.cpu()
    for g in range(min(a.show, batch.num_graphs)):
        lo, hi = int(first[g]), int(first[g + 1])
        k = min(a.top, hi - lo)
        idx = torch.topk(atom[lo:hi].abs(), k).indices
        line = ", ".join(f"atom {int(i)} ({float(atom[lo + int(i)]):+.3e})" for i in idx)
        print(f"graph {g} ({hi - lo} atoms, prediction {float(r.out_full[g, 0]):+.4f}): {line}")
    per_feature = r.node_attr.abs().sum(0)
    print("node-feature columns by total |attribution|:", torch.argsort(per_feature, descending=True)[:5].tolist())


if __name__ == "__main__":
    main()
