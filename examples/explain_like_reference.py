#!/usr/bin/env python3
"""Explain every graph of a dataset at once: a GNNExplainer-style mask optimisation on `hcatgnet_amd.explain.ExplainStep`.

The reference explains one molecule at a time with torch_geometric's `Explainer(GNNExplainer(epochs=...),
node_mask_type='attributes', edge_mask_type='object')` (scripts_experiments/explain_gnn.py:39-50).  Here one call of
`ExplainStep` delivers, for ALL graphs of the batch, the model's outputs and the gradients of each graph's own prediction
loss with respect to its edge mask and node-feature mask; the graphs are independent, so this is the batch-of-one loop of
every graph run side by side.  The regularisers (mask size, mask entropy) are functions of the masks alone and are written
out below with torch ops; `torch.optim.Adam` updates both masks.

This is an EXAMPLE, not a parity claim: no artefact of the reference pins GNNExplainer's loop (initialisation, coefficients,
the loss's exact form are those of the published algorithm as commonly implemented), and torch_geometric is not a
dependency of this package.

    python examples/explain_like_reference.py --graphs 64 --epochs 100
"""
from __future__ import annotations

import argparse
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import hcatgnet_amd as H  # noqa: E402
from hcatgnet_amd import synth  # noqa: E402
from hcatgnet_amd.explain import ExplainStep  # noqa: E402

EPS = 1e-15


def regulariser(mask_logits, size_coeff, ent_coeff, reduction):
    """size_coeff * reduce(m) + ent_coeff * mean(entropy(m)), m = sigmoid(mask): the mask terms of GNNExplainer's loss."""
    m = mask_logits.sigmoid()
    ent = -m * torch.log(m + EPS) - (1 - m) * torch.log(1 - m + EPS)
    return size_coeff * reduction(m) + ent_coeff * ent.mean()


def explain(model, batch, target, epochs=100, lr=0.01, edge_size=0.005, edge_ent=1.0, node_feat_size=1.0,
            node_feat_ent=0.1, seed=0):
    """-> (edge_mask [E], node_mask [N, F]) after `epochs` Adam steps; `target` [B, C] = what each graph's prediction is held to
    (the model's own unmasked prediction: `explanation_type='model'`)."""
    gen = torch.Generator().manual_seed(seed)
    dev = batch.x.device
    edge_mask = torch.randn(batch.edge_index.shape[1], generator=gen).to(dev).requires_grad_(True)
    node_mask = (0.1 * torch.randn(batch.x.shape, generator=gen)).to(dev).requires_grad_(True)
    opt = torch.optim.Adam([edge_mask, node_mask], lr=lr)
    step = ExplainStep(model, apply_sigmoid=True)
    for epoch in range(epochs):
        opt.zero_grad()
        r = step(batch, edge_mask, node_mask, target=target)           # ONE launch: every graph's loss and mask gradients
        reg = (regulariser(edge_mask, edge_size, edge_ent, torch.sum)
               + regulariser(node_mask, node_feat_size, node_feat_ent, torch.mean))
        reg.backward()                                                  # the regularisers' gradients: torch ops on the masks
        edge_mask.grad += r.d_edge_mask
        node_mask.grad += r.d_node_mask
        opt.step()
        if epoch % 20 == 0 or epoch == epochs - 1:
            print(f"epoch {epoch:4d}  mean prediction loss {float(r.loss.mean()):.5f}  regulariser {float(reg):.4f}  "
                  f"path {step.last_path}")
    return edge_mask.detach().sigmoid(), node_mask.detach().sigmoid()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--graphs", type=int, default=64)
    ap.add_argument("--epochs", type=int, default=100)
    ap.add_argument("--lr", type=float, default=0.01)
    ap.add_argument("--edge-size", type=float, default=0.005)
    ap.add_argument("--edge-ent", type=float, default=1.0)
    ap.add_argument("--node-feat-size", type=float, default=1.0)
    ap.add_argument("--node-feat-ent", type=float, default=0.1)
    a = ap.parse_args()
    model = H.make_network("GCN", H.default_options(), 25).cuda()
    batch = synth.make_batch(num_graphs=a.graphs, nodes=87, nodes_jitter=30, extra_bonds=4, max_degree=4, feat=25).as_batch("cuda")
    with torch.no_grad():
        target = model(batch).reshape(batch.num_graphs, -1).clone()
    em, nm = explain(model, batch, target, a.epochs, a.lr, a.edge_size, a.edge_ent, a.node_feat_size, a.node_feat_ent)
    top = torch.topk(em, min(10, em.numel())).indices.tolist()
    print("ten most important edges (batch edge positions):", top)
    print("node-feature mask: mean %.3f, max %.3f" % (float(nm.mean()), float(nm.max())))


if __name__ == "__main__":
    main()
