"""CPU-side tests (no GPU) of classification models (`--problem_type classification`) on the fused step: which models
`FusedTrainStep.unsupported_reason` accepts, the host-side argument checks of the cross-entropy modes of the C ABI, the
loss module against `nn.CrossEntropyLoss`, and the autograd fallback of `train_network` / `eval_network`.

The loss is `nn.CrossEntropyLoss()(out, y.long())` with `out` [B, C] and `y` [B] class indices: the mean over the graphs of
the batch, no sqrt, no unsqueeze (the reference's own training line cannot execute for a classification model)."""
import ctypes
import math
import os

import pytest
import torch

import hcatgnet_amd as H
from hcatgnet_amd import _lib
from hcatgnet_amd.networks import CrossEntropyLoss
from hcatgnet_amd.train import FusedTrainStep, eval_network, train_network
from tests.test_host_model_depths import _batch

INVALID = -1


@pytest.fixture(scope="module", autouse=True)
def built():
    if not os.path.isfile(_lib.LIB_PATH):
        import __graft_entry__
        __graft_entry__.build()


def _model(D=64, R=2, C=3, F=25, problem_type="classification"):
    return H.make_network("GCN", H.default_options(embedding_dim=D, readout_layers=R, n_classes=C,
                                                   problem_type=problem_type), F)


# the batch shapes of tests/test_host_model_depths.py: small-graph tiles, one graph per workgroup
BATCHES = [(25, 30, 64), (25, 184, 390)]


@pytest.mark.parametrize("D", [64, 128])
@pytest.mark.parametrize("R,C", [(R, C) for R in (1, 2, 3, 4) for C in (2, 3, 8)] + [(2, 9)])
def test_classification_models_take_the_fused_step(D, R, C):
    m = _model(D=D, R=R, C=C)
    assert isinstance(m.loss, torch.nn.CrossEntropyLoss) and isinstance(m.loss, CrossEntropyLoss)
    for shape in BATCHES:
        assert FusedTrainStep.unsupported_reason(m, _batch(*shape)) is None, shape
    if R == 2:
        assert FusedTrainStep.unsupported_reason(m) is None
    assert FusedTrainStep(m).reason(_batch(*BATCHES[0])) is None


def test_settings_outside_the_kernels_are_named():
    b = _batch(*BATCHES[0])
    m = _model()
    m.loss = CrossEntropyLoss(label_smoothing=0.1)
    assert "label_smoothing" in FusedTrainStep.unsupported_reason(m, b)
    m.loss = CrossEntropyLoss(weight=torch.ones(3))
    assert "weight" in FusedTrainStep.unsupported_reason(m, b)
    m.loss = CrossEntropyLoss(reduction="sum")
    assert "reduction" in FusedTrainStep.unsupported_reason(m, b)
    m.loss = torch.nn.CrossEntropyLoss(reduction="sum")             # (torch's own class: the same answers)
    assert "reduction" in FusedTrainStep.unsupported_reason(m, b)
    m.loss = torch.nn.CrossEntropyLoss()
    assert FusedTrainStep.unsupported_reason(m, b) is None
    one = _model(C=1)
    assert "n_classes" in FusedTrainStep.unsupported_reason(one, b)
    assert "n_classes" in FusedTrainStep.unsupported_reason(one)
    # a depth-9-class deep head stays refused for its shape, whatever the loss
    assert "readout" in FusedTrainStep.unsupported_reason(_model(R=3, C=9), b)


def test_sse_combination_is_refused_at_construction():
    m = _model()
    with pytest.raises(ValueError, match="sse"):
        FusedTrainStep(m, combine="sse")
    FusedTrainStep(m, combine="mean")
    FusedTrainStep(_model(C=1, problem_type="regression"), combine="sse")      # (regression keeps it)


def test_cross_entropy_modes_refuse_bad_arguments_on_the_host():
    lib = _lib.load()
    ce = lambda C: _lib.HCG_LOSS_CE | (C << _lib.HCG_LOSS_CE_CLASSES_SHIFT)
    out, y, loss, dout = 256, 512, 768, 1024
    # hcg_loss_fwd_bwd, cross-entropy mode: logits, labels and the loss must be there (dout is optional), C >= 1, n = B * C
    assert lib.hcg_loss_fwd_bwd(None, y, 12, ce(3), loss, dout, None, None) == INVALID
    assert lib.hcg_loss_fwd_bwd(out, None, 12, ce(3), loss, dout, None, None) == INVALID
    assert lib.hcg_loss_fwd_bwd(out, y, 12, ce(3), None, dout, None, None) == INVALID
    assert lib.hcg_loss_fwd_bwd(out, y, 0, ce(3), loss, dout, None, None) == INVALID
    assert lib.hcg_loss_fwd_bwd(out, y, 13, ce(3), loss, dout, None, None) == INVALID        # not B * C
    assert lib.hcg_loss_fwd_bwd(out, y, 12, ce(0), loss, dout, None, None) == INVALID        # no class count
    assert lib.hcg_loss_fwd_bwd(out, y, 12, _lib.HCG_LOSS_CE + 1, loss, dout, None, None) == INVALID      # unknown mode
    assert lib.hcg_loss_fwd_bwd(out, y, 12, _lib.HCG_LOSS_MSE | (3 << 8), loss, dout, None, None) == INVALID
    # hcg_loss_finalize / hcg_step_tail: a job with partials, then an unknown mode, no loss, no count
    job = _lib.ReduceJob()
    job.slabs, job.sse_part, job.nslabs, job.slab_floats = 4096, 8192, 1, 8
    addr = ctypes.addressof(job)
    assert lib.hcg_loss_finalize(addr, 17.0, _lib.HCG_LOSS_CE + 1, loss, None, None) == INVALID
    assert lib.hcg_loss_finalize(addr, 17.0, -1, loss, None, None) == INVALID
    assert lib.hcg_loss_finalize(addr, 17.0, _lib.HCG_LOSS_CE, None, None, None) == INVALID
    assert lib.hcg_loss_finalize(addr, 0.0, _lib.HCG_LOSS_CE, loss, None, None) == INVALID
    assert lib.hcg_loss_finalize(None, 17.0, _lib.HCG_LOSS_CE, loss, None, None) == INVALID
    t = _lib.TailArgs()
    t.jobs_host, t.njobs, t.loss_mode, t.loss_count, t.loss = addr, 1, _lib.HCG_LOSS_CE + 1, 17.0, loss
    assert lib.hcg_step_tail(ctypes.addressof(t), None) == INVALID
    t.loss_mode, t.loss_count = _lib.HCG_LOSS_CE, 0.0
    assert lib.hcg_step_tail(ctypes.addressof(t), None) == INVALID
    # the heads: an unknown flag, cross-entropy over one class, null pointers
    bad = _lib.HCG_HEAD_LOSS_CE << 1
    args = lambda C, flags, emb=256: (emb, 512, 768, 1024, 1280, 1536, 17, 64, C, 0.01, flags, 2048, 2304, 2560, 4096, 1 << 30,
                                      None, None)
    assert lib.hcg_head_fwd_bwd(*args(3, bad)) == INVALID
    assert lib.hcg_head_fwd_bwd(*args(1, _lib.HCG_HEAD_LOSS_CE)) == INVALID
    assert lib.hcg_head_fwd_bwd(*args(3, _lib.HCG_HEAD_LOSS_CE, emb=None)) == INVALID
    assert lib.hcg_head_fwd_bwd(*args(9, _lib.HCG_HEAD_LOSS_CE)) == _lib.HCG_ERR_UNSUPPORTED
    a = _lib.HeadArgs()
    a.B, a.D, a.C, a.R, a.flags = 17, 64, 3, 3, bad
    assert lib.hcg_head_deep_fwd_bwd(ctypes.addressof(a), addr, None) == INVALID
    a.flags = _lib.HCG_HEAD_LOSS_CE
    assert lib.hcg_head_deep_fwd_bwd(ctypes.addressof(a), addr, None) == INVALID               # no pointers
    a.C = 1
    a.emb, a.y, a.out, a.demb, a.workspace, a.workspace_bytes = 256, 512, 768, 1024, 2048, 1 << 30
    for i in range(3):
        a.W[i], a.b[i] = 4096 * (i + 1), 4096 * (i + 1) + 1024
    assert lib.hcg_head_deep_fwd_bwd(ctypes.addressof(a), addr, None) == INVALID               # one class


@pytest.mark.parametrize("B,C", [(17, 3), (1, 9)])
def test_loss_module_equals_torch_on_cpu_tensors(B, C):
    g = torch.Generator().manual_seed(B)
    out = torch.randn(B, C, generator=g)
    y = torch.randint(0, C, (B,), generator=g)
    a, b = out.clone().requires_grad_(True), out.clone().requires_grad_(True)
    la, lb = CrossEntropyLoss()(a, y), torch.nn.CrossEntropyLoss()(b, y)
    la.backward(); lb.backward()
    assert torch.equal(la, lb) and torch.equal(a.grad, b.grad)
    # non-default settings and class-probability targets keep torch's forward as well
    w = torch.rand(C, generator=g) + 0.5
    assert torch.equal(CrossEntropyLoss(weight=w, label_smoothing=0.1)(out, y),
                       torch.nn.CrossEntropyLoss(weight=w, label_smoothing=0.1)(out, y))
    p = torch.softmax(torch.randn(B, C, generator=g), 1)
    assert torch.equal(CrossEntropyLoss()(out, p), torch.nn.CrossEntropyLoss()(out, p))


class _MeanPoolClassifier(torch.nn.Module):
    """A classification model outside the fused step (no readout depth): mean-pooled node features -> Linear."""

    def __init__(self, F, C):
        super().__init__()
        torch.manual_seed(0)
        self.lin = torch.nn.Linear(F, C)
        self.loss = CrossEntropyLoss()
        self.optimizer = torch.optim.SGD(self.parameters(), lr=0.1)

    def forward(self, batch):
        pooled = torch.zeros(batch.num_graphs, batch.x.shape[1]).index_add_(0, batch.batch, batch.x)
        counts = torch.bincount(batch.batch, minlength=batch.num_graphs).clamp_min(1).unsqueeze(1)
        return self.lin(pooled / counts)


def test_train_and_eval_network_fall_back_to_cross_entropy_on_a_cpu_loader():
    from hcatgnet_amd import synth
    C, G = 3, 23
    sb = synth.make_config("REAL", num_graphs=G, seed=3)
    sb.y = torch.randint(0, C, (G,), generator=torch.Generator().manual_seed(4)).float()
    graphs = sb.as_graph_list()
    loader = H.DataLoader(graphs, batch_size=8)
    a, b = _MeanPoolClassifier(25, C), _MeanPoolClassifier(25, C)
    assert FusedTrainStep(a).reason(next(iter(loader))) is not None
    got_train = [train_network(a, loader, "cpu") for _ in range(2)]
    got_eval = eval_network(a, loader, "cpu")
    # the same epochs by hand
    want_train = []
    for _ in range(2):
        tot = 0.0
        for batch in loader:
            b.optimizer.zero_grad()
            loss = torch.nn.functional.cross_entropy(b(batch), batch.y.long())
            loss.backward()
            b.optimizer.step()
            tot += loss.item() * batch.num_graphs
        want_train.append(tot / G)
    with torch.no_grad():
        want_eval = sum(torch.nn.functional.cross_entropy(b(bt), bt.y.long()).item() * bt.num_graphs for bt in loader) / G
    assert all(math.isfinite(v) for v in got_train + [got_eval])
    for u, v in zip(got_train + [got_eval], want_train + [want_eval]):
        assert abs(u - v) <= 1e-6 * abs(v), (got_train, want_train, got_eval, want_eval)
    assert got_train[1] < got_train[0]
    for q, r in zip(a.parameters(), b.parameters()):
        assert torch.equal(q, r)
