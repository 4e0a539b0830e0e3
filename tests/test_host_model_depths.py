"""CPU-side tests (no GPU) of the fused step's depth coverage: the one-launch readout head of depth 1, 3 and 4 (its
argument struct, the shapes it takes) and `FusedTrainStep.unsupported_reason` over readout depth and conv depth, which
is bounded by the step tail's reduction jobs rather than by a fixed layer count."""
import ctypes
import os

import pytest
import torch

import hcatgnet_amd as H
from hcatgnet_amd import _lib
from hcatgnet_amd.train import FusedTrainStep


@pytest.fixture(scope="module", autouse=True)
def built():
    if not os.path.isfile(_lib.LIB_PATH):
        import __graft_entry__
        __graft_entry__.build()


def _model(D=64, R=2, n_conv=2, C=1, F=25):
    return H.make_network("GCN", H.default_options(embedding_dim=D, readout_layers=R, n_convolutions=n_conv, n_classes=C), F)


def _batch(F, max_nodes, max_edges, nodes=4, C=1):
    x = torch.zeros(nodes, F)
    ei = torch.zeros(2, 0, dtype=torch.int64)
    bv = torch.zeros(nodes, dtype=torch.int64)
    return H.Batch(x, ei, bv, 1, y=torch.zeros(1, C), max_nodes=max_nodes, max_edges=max_edges, edges_grouped=True)


def test_head_args_mirror_matches_the_library():
    lib = _lib.load()
    assert ctypes.sizeof(_lib.HeadArgs) == lib.hcg_struct_bytes(_lib.HCG_STRUCT_HEAD_ARGS)


def test_deep_head_shapes():
    lib = _lib.load()
    ws = lambda B, D, C, R: lib.hcg_general_workspace_bytes(_lib.HCG_WS_HEAD_DEEP, B, D, C, R)
    for D in (64, 128):
        for C in range(1, 9):
            for R in (1, 3, 4):
                assert ws(40, D, C, R) > 0, (D, C, R)
    for B, D, C, R in [(40, 64, 1, 5), (40, 64, 9, 3), (40, 32, 1, 3), (40, 64, 1, 2), (40, 64, 0, 1), (0, 64, 1, 3)]:
        assert ws(B, D, C, R) == 0, (B, D, C, R)
    # the slabs grow with the grid (one workgroup per 16 graphs, at most one per CU) and hold every layer's dW | db
    assert ws(4096, 64, 1, 4) > ws(40, 64, 1, 4) > ws(40, 64, 1, 1)
    per_slab = 128 * 64 + 64 + 64 * 32 + 32 + 32 * 16 + 16 + 16 * 3 + 3
    assert ws(16, 64, 3, 4) >= 4 * (per_slab + 1)


def test_launch_refuses_bad_arguments_on_the_host():
    lib = _lib.load()
    a = _lib.HeadArgs()
    job = _lib.ReduceJob()
    assert lib.hcg_head_deep_fwd_bwd(None, None, None) == -1
    a.B, a.D, a.C, a.R = 40, 64, 1, 5
    assert lib.hcg_head_deep_fwd_bwd(ctypes.addressof(a), ctypes.addressof(job), None) == -3       # depth 5: unsupported
    a.R = 3
    assert lib.hcg_head_deep_fwd_bwd(ctypes.addressof(a), ctypes.addressof(job), None) == -1       # no pointers
    a.emb, a.y, a.out, a.demb, a.workspace = 256, 512, 768, 1024, 2048
    for i in range(3):
        a.W[i], a.b[i] = 4096 * (i + 1), 4096 * (i + 1) + 1024
    a.workspace_bytes = 16
    assert lib.hcg_head_deep_fwd_bwd(ctypes.addressof(a), ctypes.addressof(job), None) == -2       # workspace too small
    a.W[1] = 4100                                                                                  # not 16-byte aligned
    assert lib.hcg_head_deep_fwd_bwd(ctypes.addressof(a), ctypes.addressof(job), None) == -1


@pytest.mark.parametrize("R", [1, 3, 4])
@pytest.mark.parametrize("D", [64, 128])
def test_readout_depths_take_the_fused_step(R, D):
    """Accepted per batch; the batch-less query keeps vouching for depth 2 only (tests/test_host_cpu.py pins that)."""
    m = _model(D=D, R=R)
    assert FusedTrainStep.unsupported_reason(m, _batch(25, 30, 64)) is None
    assert FusedTrainStep.unsupported_reason(m, _batch(25, 184, 390)) is None
    assert "per batch" in FusedTrainStep.unsupported_reason(m)


def test_readout_depths_outside_the_heads_stay_refused():
    assert "readout" in FusedTrainStep.unsupported_reason(_model(R=5))
    assert "readout" in FusedTrainStep.unsupported_reason(_model(R=3, C=9))
    assert "readout" in FusedTrainStep.unsupported_reason(_model(R=3, D=96))


@pytest.mark.parametrize("n_conv", [4, 5, 6, 7])
def test_64_wide_stacks_up_to_seven_layers(n_conv):
    assert FusedTrainStep.unsupported_reason(_model(n_conv=n_conv)) is None
    # small-graph tiles: one reduction job per layer + the head's
    assert FusedTrainStep.unsupported_reason(_model(n_conv=n_conv), _batch(25, 30, 64)) is None
    assert FusedTrainStep.unsupported_reason(_model(n_conv=n_conv, R=4), _batch(25, 30, 64)) is None


def test_conv_depth_bounded_by_the_tails_jobs():
    assert "jobs" in FusedTrainStep.unsupported_reason(_model(n_conv=8))
    assert "jobs" in FusedTrainStep.unsupported_reason(_model(D=128, n_conv=4))
    assert FusedTrainStep.unsupported_reason(_model(D=128, n_conv=3)) is None
    assert FusedTrainStep.unsupported_reason(_model(D=128, n_conv=3, R=4), _batch(128, 200, 424)) is None
    assert "jobs" in FusedTrainStep.unsupported_reason(_model(n_conv=8, R=3))      # (hard limits first, with or without a batch)
    # graphs over 64 nodes: the first layer's dense training form costs two jobs -> 6 layers fit, 7 do not
    real = _batch(25, 184, 390)
    assert FusedTrainStep.unsupported_reason(_model(n_conv=6), real) is None
    assert "jobs" in FusedTrainStep.unsupported_reason(_model(n_conv=7), real)
    assert FusedTrainStep.unsupported_reason(_model(n_conv=7), _batch(25, 30, 64)) is None


def test_job_count_follows_the_routes():
    count = FusedTrainStep._conv_jobs
    assert count(_model(n_conv=3)) == 3 and count(_model(D=128, n_conv=3)) == 6
    assert count(_model(n_conv=3), _batch(25, 30, 64)) == 3                    # small-graph tiles
    assert count(_model(n_conv=3), _batch(25, 184, 390)) == 4                  # dense first layer behind one graph per workgroup
    assert count(_model(n_conv=1), _batch(25, 184, 390)) == 1                  # (a lone layer has no dense training form)
    assert count(_model(D=128, n_conv=3), _batch(28, 159, 330)) == 6           # wide-layer route: dW, db
    big = _batch(25, 184, 390, nodes=150000)                                   # 64-wide layers on the wide-layer route
    assert count(_model(n_conv=3), big) == 6
    step = FusedTrainStep.__new__(FusedTrainStep)
    step.XAGG = False                                                          # (the first layer's plain form)
    assert count(_model(n_conv=3), _batch(25, 184, 390), step) == 3

