#!/usr/bin/env python3
"""Explain every graph of a dataset at once: GNNExplainer on `hcatgnet_amd.explain.ExplainFit`.

The reference explains one molecule at a time with torch_geometric's `Explainer(GNNExplainer(epochs=...),
node_mask_type='attributes', edge_mask_type='object')` (scripts_experiments/explain_gnn.py:39-50).  Here ONE call of
`ExplainFit` runs the whole mask optimisation of ALL graphs of the batch -- every epoch's forward, backward, regularisers
and Adam step, one workgroup per graph -- in one launch; the graphs are independent, so this is the batch-of-one fit of
every graph run side by side.

`--hand-loop` runs the loop a caller had to write before `ExplainFit` existed: one `ExplainStep` call per epoch for the
prediction loss's gradients, the regularisers (mask size, mask entropy) written out with torch ops, `torch.optim.Adam` on
both masks.  It regularises every entry over the whole batch (no hard masks, no per-graph means), so its numbers differ
from `ExplainFit`'s, which follows the published algorithm graph by graph.

This is an EXAMPLE, not a parity claim: no artefact of the reference pins GNNExplainer (`ExplainFit`'s docstring states the
definition used), and torch_geometric is not a dependency of this package.

    python examples/explain_like_reference.py --graphs 64 --epochs 100
    python examples/explain_like_reference.py --graphs 64 --epochs 100 --hand-loop
    python examples/explain_like_reference.py --problem-type classification --n-classes 3

`--problem-type classification` builds a classifier (`--n-classes`, two or more) and explains it as torch_geometric does
for `ModelMode.multiclass_classification` on raw outputs: the prediction loss is the cross-entropy against a class index
per graph -- the class the unmasked model predicts -- instead of the mean squared error against its output row.
"""
from __future__ import annotations

import argparse
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import hcatgnet_amd as H  # noqa: E402
from hcatgnet_amd import synth  # noqa: E402
from hcatgnet_amd.explain import ExplainFit, ExplainStep  # noqa: E402

EPS = 1e-15


def regulariser(mask_logits, size_coeff, ent_coeff, reduction):
    """size_coeff * reduce(m) + ent_coeff * mean(entropy(m)), m = sigmoid(mask): the mask terms of GNNExplainer's loss."""
    m = mask_logits.sigmoid()
    ent = -m * torch.log(m + EPS) - (1 - m) * torch.log(1 - m + EPS)
    return size_coeff * reduction(m) + ent_coeff * ent.mean()


def explain(model, batch, target, epochs=100, lr=0.01, seed=0, mode="regression", **coeffs):
    """-> (edge_mask [E], node_mask [N, F]) of GNNExplainer's fit of every graph, ONE launch; `target` = what each graph's
    prediction is held to (`explanation_type='model'`): the model's own unmasked prediction [B, C] in regression mode, the
    class it predicts (int64 [B]) in classification mode."""
    fit = ExplainFit(model, epochs=epochs, lr=lr, coeffs=coeffs, mode=mode)
    r = fit(batch, target=target, generator=torch.Generator().manual_seed(seed))
    for epoch in list(range(0, epochs, 20)) + [epochs - 1]:
        print(f"epoch {epoch:4d}  mean prediction loss {float(r.loss_history[epoch].mean()):.5f}")
    hard = r.state.hard_count.sum(dim=0).tolist()
    print(f"path {fit.last_path}: {r.state.step} Adam steps, {hard[0]} hard edges, {hard[1]} hard node entries")
    return r.edge_mask, r.node_mask


def explain_hand_loop(model, batch, target, epochs=100, lr=0.01, edge_size=0.005, edge_ent=1.0, node_feat_size=1.0,
                      node_feat_ent=0.1, seed=0, mode="regression"):
    """The hand-written loop on `ExplainStep` (see the module docstring) -> (edge_mask [E], node_mask [N, F])."""
    upstream = "target_class" if mode == "multiclass_classification" else "target"
    gen = torch.Generator().manual_seed(seed)
    dev = batch.x.device
    edge_mask = torch.randn(batch.edge_index.shape[1], generator=gen).to(dev).requires_grad_(True)
    node_mask = (0.1 * torch.randn(batch.x.shape, generator=gen)).to(dev).requires_grad_(True)
    opt = torch.optim.Adam([edge_mask, node_mask], lr=lr)
    step = ExplainStep(model, apply_sigmoid=True)
    for epoch in range(epochs):
        opt.zero_grad()
        r = step(batch, edge_mask, node_mask, **{upstream: target})    # ONE launch: every graph's loss and mask gradients
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
    ap.add_argument("--hand-loop", action="store_true", help="the caller-side loop on ExplainStep instead of ExplainFit")
    ap.add_argument("--problem-type", choices=["regression", "classification"], default="regression")
    ap.add_argument("--n-classes", type=int, default=None, help="outputs of the model (default: 1 for regression, 3 for classification)")
    a = ap.parse_args()
    classify = a.problem_type == "classification"
    n_classes = a.n_classes if a.n_classes is not None else (3 if classify else 1)
    if classify and n_classes < 2:
        ap.error("--problem-type classification needs --n-classes of 2 or more")
    model = H.make_network("GCN", H.default_options(problem_type=a.problem_type, n_classes=n_classes), 25).cuda()
    batch = synth.make_batch(num_graphs=a.graphs, nodes=87, nodes_jitter=30, extra_bonds=4, max_degree=4, feat=25).as_batch("cuda")
    with torch.no_grad():
        target = model(batch).reshape(batch.num_graphs, -1).clone()
    if classify:
        target = target.argmax(dim=1)                      # the class the unmasked model predicts (what ExplainFit defaults to)
        print("explained classes:", torch.bincount(target, minlength=n_classes).tolist(), "graphs per class")
    run = explain_hand_loop if a.hand_loop else explain
    em, nm = run(model, batch, target, a.epochs, a.lr, edge_size=a.edge_size, edge_ent=a.edge_ent,
                 node_feat_size=a.node_feat_size, node_feat_ent=a.node_feat_ent,
                 mode="multiclass_classification" if classify else "regression")
    top = torch.topk(em, min(10, em.numel())).indices.tolist()
    print("ten most important edges (batch edge positions):", top)
    print("node-feature mask: mean %.3f, max %.3f" % (float(nm.mean()), float(nm.max())))


if __name__ == "__main__":
    main()
