"""hcatgnet_amd -- MI355X-native drop-in for the GCN message-passing path of EdAguilarB/hcatgnet.

Public surface (mirrors the reference's names for this path):
    make_network("GCN", opt, n_node_features)   reference call_methods.py:7-12
    GCN, GCN_explain, BaseNetwork               reference model/gcn.py, model/networks.py
    Data, Batch, collate, DataLoader            stand-ins for the PyG containers the loops touch
    BatchPlan                                   per-batch CSR / gcn_norm plan (GPU)
    DeviceGraphStore, DeviceLoader              dataset resident in HBM, batches collated on the GPU
    DataParallelGCN                             one-process-per-GPU gradient all-reduce (RCCL)
    optim.FusedAdam / FusedSGD / FusedRMSprop   the reference's --optimizer Adam | SGD | rmsprop (model/networks.py:36-44),
                                                updated on the device, carried in the step's last launch
    train.FusedTrainStep, train.train_network / eval_network / predict_network
                                                the reference's loops (utils/utils_model.py:55-111); the step as 6 launches
    io.load_processed_dir / write_embeddings_csv the reference's on-disk formats (reaction_N.pt in, embeddings.csv out)
    explain.set_masks / clear_masks             explain-mode edge masks (PyG Explainer hooks)
    fit_network, fit_networks, FitResult        the reference's whole epoch loop (train_GNN.py:73-111) enqueued ahead of the GPU:
                                                scheduler, early stopping, best weights and loss log kept on the device
    ExplainFit                                  GNNExplainer's whole mask optimisation of a batch of graphs in one launch
                                                (the reference's first explain algorithm, explain_gnn.py)
    EnsemblePredict, stack_weights              M trained models predict one batch in one launch (the reference's
                                                predict_test.py loop); train.predict_networks is its loader form
    ShapleySampling, draw_permutations          Shapley value sampling of a batch of graphs, the permutation walk on chip
                                                (the reference's second explain algorithm, explain_gnn.py)
    atom_groups, bond_groups, draw_group_permutations, all_group_permutations
                                                the same walk with atoms, bonds or fragments as the players
    CoalitionValues, shapley_from_coalitions, interactions_from_coalitions
                                                the model's output for every subset of a graph's groups (up to 16), evaluated
                                                on chip; exact Shapley values and pairwise interaction indices from that table
    SubsetValues, AttributionCurves, pack_subsets, ranking, group_scores
                                                the model's output for a LIST of subsets of a graph's groups (any number
                                                of groups) evaluated on chip; deletion / insertion curves and their AUCs
                                                for a ranking of the groups, whichever attribution it came from
    GreedySelection, GreedyResult               the model-driven greedy insertion / deletion order of a graph's groups, one
                                                launch per round and the winner picked on chip: the envelope the curves
                                                are read against, and the top-k sufficient / necessary set of groups
    IntegratedGradients, quadrature             integrated gradients (Captum's IntegratedGradients through the same
                                                CaptumExplainer entry point) of a batch of graphs, the whole path of every
                                                graph in one launch; method="gradient" / saliency=True are its one-step
                                                relatives InputXGradient and Saliency
    EnsembleAttribution                         the same attributions of M models in one launch (one workgroup per graph
                                                and model), with their mean and standard deviation over the models
    EnsembleShapley, EnsembleSubsetValues, EnsembleCurves
                                                Shapley value sampling, subset values and deletion / insertion curves of M
                                                models, the model a grid axis of the single-model kernels: the moments over
                                                the models on the device, entry [m] bitwise the single-model class's
Compute lives in csrc/libhcatgnet_hip.so (hand-written HIP for gfx950) behind include/hcatgnet_hip.h.
"""
from .attribution import EnsembleAttribution, EnsembleAttributionResult, IntegratedGradients, IntegratedGradientsResult, quadrature  # noqa: F401
from .batch import Batch, Data, DataLoader, collate  # noqa: F401
from .call_methods import default_options, make_network  # noqa: F401
from .ensemble import EnsemblePredict, EnsembleResult, stack_weights  # noqa: F401
from .ensemble_shapley import (EnsembleCurveResult, EnsembleCurves, EnsembleFeatureShapleyResult, EnsembleShapley,  # noqa: F401
                               EnsembleShapleyResult, EnsembleSubsetResult, EnsembleSubsetValues)
from .explain import ExplainFit, ExplainFitResult, ExplainFitState  # noqa: F401
from .fit import FitControl, FitResult, fit_network, fit_networks  # noqa: F401
from .gcn import GCN, GCN_explain, GCNConv  # noqa: F401
from .greedy import GreedyResult, GreedySelection  # noqa: F401
from .networks import BaseNetwork  # noqa: F401
from .plan import BatchPlan  # noqa: F401
from .shapley import (CoalitionResult, CoalitionValues, GroupedShapleyResult, ShapleyResult, ShapleySampling,  # noqa: F401
                      all_group_permutations, atom_groups, bond_groups, draw_group_permutations, draw_permutations,
                      interactions_from_coalitions, shapley_from_coalitions)
from .store import DeviceGraphStore, DeviceLoader  # noqa: F401
from .subsets import AttributionCurves, CurveResult, SubsetResult, SubsetValues, group_scores, pack_subsets, ranking  # noqa: F401

__all__ = ["make_network", "default_options", "GCN", "GCN_explain", "GCNConv", "BaseNetwork", "Data", "Batch",
           "collate", "DataLoader", "BatchPlan", "DeviceGraphStore", "DeviceLoader", "EnsemblePredict", "EnsembleResult",
           "stack_weights", "ShapleySampling", "ShapleyResult", "draw_permutations", "GroupedShapleyResult", "atom_groups",
           "bond_groups", "draw_group_permutations", "all_group_permutations", "ExplainFit", "ExplainFitResult",
           "ExplainFitState", "fit_network", "fit_networks", "FitResult", "FitControl", "IntegratedGradients", "IntegratedGradientsResult",
           "quadrature", "EnsembleAttribution", "EnsembleAttributionResult", "CoalitionValues", "CoalitionResult",
           "shapley_from_coalitions", "interactions_from_coalitions", "SubsetValues", "SubsetResult", "AttributionCurves",
           "CurveResult", "pack_subsets", "ranking", "group_scores", "GreedySelection", "GreedyResult",
           "EnsembleShapley", "EnsembleShapleyResult", "EnsembleFeatureShapleyResult", "EnsembleSubsetValues", "EnsembleSubsetResult",
           "EnsembleCurves", "EnsembleCurveResult"]
