#!/usr/bin/env python3
"""Predict one set of graphs with an ensemble of trained models, every model in the same launch.

The reference reloads the models of its nested cross-validation one by one and predicts the same unseen set with each, through
a batch-of-one loader (scripts_experiments/predict_test.py:19-103).  Here `train.predict_networks` hands each batch of the
shared loader to `hcatgnet_amd.EnsemblePredict` once: the graphs' normalisation and row lists are built once per graph and
reused by every model.  Written: per-model `embeddings.csv` in the reference's format (`io.write_embeddings_csv`, one
directory per model) and one table of the ensemble's mean / standard deviation per graph.

    python examples/predict_like_reference.py --state-dicts run/*/model_params.pth --processed data/test/processed --out pred
    python examples/predict_like_reference.py --seeds 0 1 2 3 4 5 6 7 8 --graphs 52 --out pred        # synthetic stand-in
"""
from __future__ import annotations

import argparse
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import hcatgnet_amd as H  # noqa: E402
from hcatgnet_amd import io as hio, synth, train  # noqa: E402


def load_models(a):
    models = []
    if a.state_dicts:
        for path in a.state_dicts:
            m = H.make_network("GCN", H.default_options(), a.features)
            m.load_state_dict(torch.load(path, map_location="cpu", weights_only=True))
            models.append(m.cuda().eval())
    else:
        for seed in a.seeds:
            torch.manual_seed(seed)
            models.append(H.make_network("GCN", H.default_options(), a.features).cuda().eval())
    return models


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--state-dicts", nargs="*", default=[], help="K model_params.pth files of one architecture")
    ap.add_argument("--seeds", type=int, nargs="*", default=[0, 1, 2], help="without state-dicts: K freshly initialised models")
    ap.add_argument("--processed", default=None, help="a processed/ directory of reaction_N.pt files")
    ap.add_argument("--graphs", type=int, default=52, help="without --processed: size of the synthetic set")
    ap.add_argument("--features", type=int, default=25)
    ap.add_argument("--batch-size", type=int, default=64)
    ap.add_argument("--out", default="ensemble_prediction")
    a = ap.parse_args()

    models = load_models(a)
    if a.processed:
        graphs = hio.load_processed_dir(a.processed, a.features)
    else:
        graphs = synth.make_batch(num_graphs=a.graphs, nodes=120, nodes_jitter=64, extra_bonds=4, max_degree=4,
                                  feat=a.features).as_graph_list()
    loader = H.DataLoader(graphs, batch_size=a.batch_size)
    os.makedirs(a.out, exist_ok=True)

    # every model's (y_pred, y_true, idx, embeddings frame), one ensemble call per batch
    results = train.predict_networks(models, loader, return_emb=True)
    for k, (model, (_, _, _, frame)) in enumerate(zip(models, results)):
        d = os.path.join(a.out, f"model_{k}")
        os.makedirs(d, exist_ok=True)
        frame["set"] = "test"
        frame.to_csv(os.path.join(d, "embeddings.csv"))          # the file io.write_embeddings_csv(model, {"test": loader}, ...) writes

    # the ensemble's own table: mean and (population) standard deviation over the models, per graph
    import pandas as pd
    ens = H.EnsemblePredict(models)
    rows = []
    with torch.no_grad():
        for batch in loader:
            batch = batch.to("cuda")
            r = ens(batch)
            rows.append(pd.DataFrame(dict(index=batch.idx.cpu().numpy(), ddG_exp=batch.y.reshape(-1).cpu().numpy(),
                                          ddG_mean=r.mean[:, 0].cpu().numpy(), ddG_std=r.std[:, 0].cpu().numpy())))
    table = pd.concat(rows, axis=0, ignore_index=True)
    table.to_csv(os.path.join(a.out, "ensemble.csv"), index=False)
    print(f"{len(models)} models, {len(graphs)} graphs, path {ens.last_path}: wrote {a.out}/model_*/embeddings.csv and ensemble.csv")
    print(table.head(10).to_string(index=False))


if __name__ == "__main__":
    main()
