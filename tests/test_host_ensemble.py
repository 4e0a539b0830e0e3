"""Host side of ensemble prediction (no GPU): the ensemble mode of hcg_explain (argument block, shape query), `stack_weights`
on CPU state-dicts, and `EnsemblePredict`'s construction and support check."""
import ctypes
import os

import pytest
import torch

import hcatgnet_amd as H
from hcatgnet_amd import _lib
from hcatgnet_amd.ensemble import EnsemblePredict, default_models_per_group, stack_weights, weight_names


@pytest.fixture(scope="module", autouse=True)
def built():
    if not os.path.isfile(_lib.LIB_PATH):
        import __graft_entry__
        __graft_entry__.build()


def _args(F=25, D=64, nodes=184, edges=390, n_conv=2, R=2, C=1, B=52, M=9, mpg=1):
    a = _lib.ExplainArgs()
    a.mode, a.flags = _lib.HCG_EXPLAIN_ENSEMBLE, _lib.HCG_EXPLAIN_QUERY
    a.F, a.D, a.C, a.n_conv, a.R = F, D, C, n_conv, R
    a.max_nodes, a.max_edges = nodes, edges
    a.N, a.E, a.B = nodes * B, edges * B, B
    a.n_models, a.models_per_group = M, mpg
    return a


def _query(**kw):
    a = _args(**kw)
    a.workspace_bytes_needed = 12345
    rc = _lib.load().hcg_explain(ctypes.addressof(a), None)
    return rc, int(a.workspace_bytes_needed)


def test_explain_args_mirror_matches_the_library():
    lib = _lib.load()
    assert _lib.HCG_EXPLAIN_ENSEMBLE == 2
    assert ctypes.sizeof(_lib.ExplainArgs) == lib.hcg_struct_bytes(7)
    for name in ("n_models", "models_per_group", "emb"):
        assert hasattr(_lib.ExplainArgs, name)
    assert lib.hcg_version() == 1
    a = _lib.ExplainArgs()
    a.mode = 9
    assert lib.hcg_explain(ctypes.addressof(a), None) == -1


def test_ensemble_query_accepts_and_refuses_without_a_gpu():
    """HCG_EXPLAIN_QUERY in the ensemble mode validates the shapes and launches nothing (this machine may have no GPU at
    all).  Forward only: no workspace."""
    for M in (1, 9, 90):
        for mpg in sorted({1, M, default_models_per_group(M, 52)}):
            assert _query(M=M, mpg=mpg) == (0, 0), (M, mpg)
    assert _query(F=64, nodes=224, edges=1024, n_conv=4, R=4, C=8, M=90, mpg=9) == (0, 0)
    assert _query(B=535, nodes=120, edges=250, M=90, mpg=90) == (0, 0)
    for n_conv in (1, 2, 3, 4):
        for R in (1, 2, 3, 4):
            assert _query(n_conv=n_conv, R=R)[0] == 0
    for kw in (dict(D=128), dict(F=65), dict(nodes=225), dict(edges=1025), dict(C=9), dict(M=0), dict(mpg=0), dict(M=9, mpg=10),
               dict(R=5), dict(n_conv=5), dict(F=0), dict(C=0), dict(n_conv=0), dict(R=0)):
        assert _query(**kw)[0] == -3, kw


def test_masks_or_a_target_are_invalid_in_ensemble_mode():
    lib = _lib.load()
    dummy = ctypes.create_string_buffer(64)
    for field in ("edge_mask", "node_mask", "target", "dout"):
        a = _args()
        setattr(a, field, ctypes.addressof(dummy))
        assert lib.hcg_explain(ctypes.addressof(a), None) == -1, field
    assert lib.hcg_explain(ctypes.addressof(_args()), None) == 0


def _state_dicts(M, F=25, **kw):
    return [H.make_network("GCN", H.default_options(**kw), F).state_dict() for _ in range(M)]


def test_stack_weights_on_cpu_state_dicts():
    sds = _state_dicts(5, n_convolutions=3, readout_layers=3, n_classes=2)
    S = stack_weights(sds)
    assert set(S) == set(sds[0])
    cw, cb, hw, hb = weight_names(3, 3)
    assert set(cw + cb + hw + hb) == set(S)
    assert tuple(S["conv1.lin.weight"].shape) == (5, 64, 25) and tuple(S["conv_layers.1.lin.weight"].shape) == (5, 64, 64)
    assert tuple(S["conv1.bias"].shape) == (5, 64)
    assert tuple(S["readout.0.0.weight"].shape) == (5, 64, 128) and tuple(S["readout.1.0.weight"].shape) == (5, 32, 64)
    assert tuple(S["readout.2.weight"].shape) == (5, 2, 32) and tuple(S["readout.2.bias"].shape) == (5, 2)
    for name, t in S.items():
        assert t.is_contiguous() and t.dtype == torch.float32
        for k in range(5):
            assert torch.equal(t[k], sds[k][name]), (name, k)
    # a snapshot: the stack does not alias the models
    sds[2]["conv1.bias"].add_(1.0)
    assert not torch.equal(S["conv1.bias"][2], sds[2]["conv1.bias"])
    with pytest.raises(ValueError):
        stack_weights(_state_dicts(2) + _state_dicts(1, F=32))                       # another feature count
    with pytest.raises(ValueError):
        stack_weights(_state_dicts(2) + _state_dicts(1, embedding_dim=128))          # another width
    with pytest.raises(ValueError):
        stack_weights(_state_dicts(2) + _state_dicts(1, n_convolutions=3))           # another conv depth
    with pytest.raises(ValueError):
        stack_weights(_state_dicts(2) + _state_dicts(1, readout_layers=3))           # another readout depth
    with pytest.raises(ValueError):
        stack_weights([])


def _models(M, F=25, **kw):
    return [H.make_network("GCN", H.default_options(**kw), F) for _ in range(M)]


def test_constructor_checks_the_models():
    ens = EnsemblePredict(_models(3))
    assert ens.n_models == 3 and tuple(ens.stacked["conv1.lin.weight"].shape) == (3, 64, 25)
    assert H.EnsemblePredict is EnsemblePredict and H.stack_weights is stack_weights
    with pytest.raises(ValueError):
        EnsemblePredict([])
    with pytest.raises(ValueError):
        EnsemblePredict(_models(2) + [torch.nn.Linear(4, 4)])
    for kw in (dict(embedding_dim=128), dict(n_convolutions=3), dict(readout_layers=3), dict(n_classes=2)):
        with pytest.raises(ValueError):
            EnsemblePredict(_models(2) + _models(1, **kw))
    with pytest.raises(ValueError):
        EnsemblePredict(_models(2) + _models(1, F=32))
    for bad in (0, 4):
        with pytest.raises(ValueError):
            EnsemblePredict(_models(3), models_per_group=bad)
    # refresh() re-stacks in place
    before = ens.stacked["conv1.bias"].data_ptr()
    with torch.no_grad():
        ens.models[1].conv1.bias.add_(0.5)
    assert not torch.equal(ens.stacked["conv1.bias"][1], ens.models[1].conv1.bias)
    ens.refresh()
    assert torch.equal(ens.stacked["conv1.bias"][1], ens.models[1].conv1.bias.detach())
    assert ens.stacked["conv1.bias"].data_ptr() == before


def test_default_group_keeps_the_workgroup_target():
    """The largest group that leaves >= 512 workgroups (2 per CU), between 1 and min(M, 4) (the cap of the recorded sweep)."""
    assert default_models_per_group(90, 52) == 4
    assert default_models_per_group(9, 52) == 1           # 468 (model, graph) pairs: every pair its own workgroup
    assert default_models_per_group(90, 535) == 4
    assert default_models_per_group(9, 535) == 4
    assert default_models_per_group(2, 4000) == 2
    assert default_models_per_group(1, 1) == 1
    for M, B in ((90, 52), (9, 52), (90, 535), (7, 300), (3, 171), (64, 17)):
        g = default_models_per_group(M, B)
        assert 1 <= g <= min(M, 4)
        if g > 1:
            assert B * -(-M // g) >= 512           # workgroups = graphs x groups


def test_ensemble_support_check_is_host_only():
    """`EnsemblePredict.reason` decides on the host (no GPU, no sync) whether the models / a batch take the one-launch kernel."""
    x = torch.zeros(4, 25); ei = torch.zeros(2, 0, dtype=torch.int64); bv = torch.zeros(4, dtype=torch.int64)
    mk = lambda **kw: H.Batch(x, ei, bv, 1, **kw)
    ens = EnsemblePredict(_models(3))
    assert ens.reason() is None
    assert ens.reason(mk(max_nodes=30, max_edges=64, edges_grouped=True)) is None
    assert ens.reason(mk(max_nodes=184, max_edges=390, edges_grouped=True)) is None
    assert ens.reason(mk(max_nodes=224, max_edges=1024, edges_grouped=True)) is None
    assert "shape" in ens.reason(mk(max_nodes=225, max_edges=390, edges_grouped=True))
    assert "shape" in ens.reason(mk(max_nodes=184, max_edges=1025, edges_grouped=True))
    assert "metadata" in ens.reason(mk())
    assert "metadata" in ens.reason(mk(max_nodes=30, max_edges=64))
    wrong = H.Batch(torch.zeros(4, 32), ei, bv, 1, max_nodes=30, max_edges=64, edges_grouped=True)
    assert "features" in ens.reason(wrong)
    for kw in (dict(embedding_dim=128), dict(n_convolutions=5), dict(n_classes=9)):
        assert "shape" in EnsemblePredict(_models(2, **kw)).reason(), kw
    assert "shape" in EnsemblePredict(_models(2, F=65)).reason()
    for kw in (dict(n_convolutions=1, readout_layers=1), dict(n_convolutions=3, readout_layers=3, n_classes=2),
               dict(n_convolutions=4, readout_layers=4, n_classes=8)):
        assert EnsemblePredict(_models(2, F=32, **kw), models_per_group=2).reason() is None, kw
    off = _models(2) + _models(1, use_fused=False)
    assert "disabled" in EnsemblePredict(off).reason()
    assert ens.last_path is None
