#!/usr/bin/env python3
"""Shapley value sampling for every graph of a dataset at once on `hcatgnet_amd.ShapleySampling`.

The reference attributes one molecule at a time with torch_geometric's `Explainer(CaptumExplainer('ShapleyValueSampling'),
node_mask_type='attributes', edge_mask_type='object')` (scripts_experiments/explain_gnn.py): one batch-of-one forward per
feature per permutation.  Here one call walks `--samples` permutations of ALL graphs of the batch on chip, one workgroup per
(graph, permutation), and returns the mean attribution of every node-feature entry and every edge.

This is an EXAMPLE, not a parity claim: no artefact of the reference pins Shapley values (the permutations are random, and
Captum draws them its own way), and neither captum nor torch_geometric is a dependency of this package.

    python examples/shapley_like_reference.py --graphs 64 --samples 25
"""
from __future__ import annotations

import argparse
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import hcatgnet_amd as H  # noqa: E402
from hcatgnet_amd import synth  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--graphs", type=int, default=64)
    ap.add_argument("--samples", type=int, default=25)
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--nonzero-share", type=float, default=0.2, help="share of the node-feature entries kept non-zero (one-hot-like)")
    a = ap.parse_args()
    model = H.make_network("GCN", H.default_options(), 25).cuda()
    sb = synth.make_batch(num_graphs=a.graphs, nodes=87, nodes_jitter=30, extra_bonds=4, max_degree=4, feat=25)
    keep = torch.rand(sb.x.shape, generator=torch.Generator().manual_seed(a.seed)) < a.nonzero_share
    sb.x = (sb.x * keep).contiguous()
    batch = sb.as_batch("cuda")

    sv = H.ShapleySampling(model)
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
