"""BaseNetwork: same constructor contract and attributes as the reference's `model/networks.py`
(:8-61): stores the `opt` dimensions, seeds globally, and attaches `loss` / `optimizer` /
`scheduler` to the module, because the training loop reads them from the model
(utils/utils_model.py:62-66, scripts_experiments/train_GNN.py:88)."""
from __future__ import annotations

import argparse
import random

import numpy as np
import torch
import torch.nn as nn


class MSELoss(nn.Module):
    """`nn.MSELoss()` (mean reduction) with the reference's call contract `loss(out, y.unsqueeze(1))`
    (utils/utils_model.py:64); on MI355X tensors it is one HIP launch each way (csrc/loss.hip) instead
    of torch's elementwise + reduction chain.  Same-shape float32 inputs only."""

    def forward(self, inp, target):
        from . import functional as HF
        return HF.mse_loss(inp, target)


class CrossEntropyLoss(nn.CrossEntropyLoss):
    """`nn.CrossEntropyLoss` for `--problem_type classification`.  The reference's own training line cannot execute for a
    classification model (`torch.sqrt(model.loss(out, y.unsqueeze(1)))` is rejected by torch), so the definition here is
    the minimal reading of it: `loss = nn.CrossEntropyLoss()(out, y.long())` with `out` [B, C] and `y` [B] holding class
    indices, the mean over the graphs of the batch, no sqrt and no unsqueeze.  With default settings, float32 MI355X logits
    and class-index targets it is one HIP launch each way (csrc/loss.hip: k_ce_fwd_bwd); anything else -- class weights,
    label smoothing, another reduction, `ignore_index`, class-probability targets, CPU tensors -- is torch's own forward."""

    def default_settings(self) -> bool:
        return (self.weight is None and self.reduction == "mean" and self.label_smoothing == 0.0
                and self.ignore_index == -100)

    def forward(self, inp, target):
        if (self.default_settings() and inp.is_cuda and inp.dtype == torch.float32 and inp.dim() == 2
                and target.dim() == 1 and target.dtype == torch.int64 and target.shape[0] == inp.shape[0]):
            from . import functional as HF
            return HF.cross_entropy(inp, target)
        return super().forward(inp, target)


class BaseNetwork(nn.Module):
    def __init__(self, opt: argparse.Namespace, n_node_features: int):
        super().__init__()
        self._name = "BaseNetwork"
        self._opt = opt
        self.n_node_features = n_node_features
        self._n_classes = opt.n_classes
        self.n_convolutions = opt.n_convolutions
        self.embedding_dim = opt.embedding_dim
        self.readout_layers = opt.readout_layers
        self._seed_everything(opt.global_seed)

    def forward(self):
        raise NotImplementedError

    @property
    def name(self):
        return self._name

    def _make_loss(self, problem_type, mae=None):
        if problem_type == "classification":
            self.loss = CrossEntropyLoss()
        elif problem_type == "regression" and mae is None:
            self.loss = MSELoss()
        else:
            raise ValueError(f"Problem type {problem_type} not supported")

    def _make_optimizer(self, optimizer, lr):
        # the reference's torch.optim.Adam(lr, eps=1e-9) / SGD(lr) / RMSprop(lr) (model/networks.py:36-44); same rules,
        # one HIP launch (or none of their own: carried in the step's last launch)
        from .optim import FusedAdam, FusedRMSprop, FusedSGD
        if optimizer == "Adam":
            self.optimizer = FusedAdam(self.parameters(), lr=lr, eps=1e-9)
        elif optimizer == "SGD":
            self.optimizer = FusedSGD(self.parameters(), lr=lr)
        elif optimizer == "rmsprop":
            self.optimizer = FusedRMSprop(self.parameters(), lr=lr)
        else:
            raise NotImplementedError(f"Optimizer type {optimizer} not implemented")

    def _make_scheduler(self, scheduler, step_size, gamma, min_lr):
        sched = torch.optim.lr_scheduler
        if scheduler == "StepLR":
            self.scheduler = sched.StepLR(self.optimizer, step_size=step_size, gamma=gamma)
        elif scheduler == "MultiStepLR":
            self.scheduler = sched.MultiStepLR(self.optimizer, milestones=step_size, gamma=gamma)
        elif scheduler == "ExponentialLR":
            self.scheduler = sched.ExponentialLR(self.optimizer, gamma=gamma)
        elif scheduler == "ReduceLROnPlateau":
            self.scheduler = sched.ReduceLROnPlateau(self.optimizer, mode="min", factor=gamma, patience=step_size,
                                                     min_lr=min_lr)
        else:
            raise NotImplementedError(f"Scheduler type {scheduler} not implemented")

    def _seed_everything(self, seed):
        # what torch_geometric.seed.seed_everything does (reference model/networks.py:58-61)
        random.seed(seed)
        np.random.seed(seed % (2 ** 32))
        torch.manual_seed(seed)
        if torch.cuda.is_available():
            torch.cuda.manual_seed_all(seed)
