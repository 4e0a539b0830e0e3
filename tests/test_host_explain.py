"""Host side of the one-launch explain step (no GPU): the hcg_explain argument block, its shape / workspace query, the
folded C symbol, and `ExplainStep.reason`."""
import ctypes
import os
import re

import pytest
import torch

import hcatgnet_amd as H
from hcatgnet_amd import _lib
from hcatgnet_amd.explain import ExplainStep

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module", autouse=True)
def built():
    if not os.path.isfile(_lib.LIB_PATH):
        import __graft_entry__
        __graft_entry__.build()


def _query(F=25, D=64, nodes=184, edges=390, n_conv=2, R=2, C=1, N=None, B=1):
    a = _lib.ExplainArgs()
    a.mode, a.flags = _lib.HCG_EXPLAIN_GRAPHS, _lib.HCG_EXPLAIN_QUERY
    a.F, a.D, a.C, a.n_conv, a.R = F, D, C, n_conv, R
    a.max_nodes, a.max_edges = nodes, edges
    a.N, a.E, a.B = nodes if N is None else N, edges, B
    rc = _lib.load().hcg_explain(ctypes.addressof(a), None)
    return rc, int(a.workspace_bytes_needed)


def test_explain_args_mirror_matches_the_library():
    lib = _lib.load()
    assert ctypes.sizeof(_lib.ExplainArgs) == lib.hcg_struct_bytes(_lib.HCG_STRUCT_EXPLAIN_ARGS)
    assert _lib.HCG_STRUCT_EXPLAIN_ARGS == 7
    assert lib.hcg_explain(None, None) == -1
    a = _lib.ExplainArgs()
    a.mode = 9
    assert lib.hcg_explain(ctypes.addressof(a), None) == -1


def test_query_accepts_and_refuses_without_a_gpu():
    """HCG_EXPLAIN_QUERY validates the shapes and reports the workspace; nothing is launched (this machine may have no
    GPU at all).  The workspace holds H and A of every conv layer for the backward: 2 * n_conv * N * 64 floats."""
    rc, ws = _query()
    assert rc == 0 and ws >= 2 * 2 * 184 * 64 * 4
    rc, ws = _query(F=64, nodes=224, edges=1024, n_conv=4, R=4, C=8)
    assert rc == 0 and ws >= 2 * 4 * 224 * 64 * 4
    rc, ws = _query(nodes=120, edges=250, N=535 * 120, B=535)
    assert rc == 0 and ws >= 2 * 2 * 535 * 120 * 64 * 4
    for n_conv in (1, 2, 3, 4):
        for R in (1, 2, 3, 4):
            assert _query(n_conv=n_conv, R=R)[0] == 0
    for kw in (dict(D=128), dict(F=65), dict(nodes=225), dict(edges=1025), dict(C=9), dict(R=5), dict(n_conv=5), dict(F=0),
               dict(C=0), dict(n_conv=0), dict(R=0)):
        assert _query(**kw)[0] == -3, kw


def test_old_edge_gradient_symbol_is_folded_into_hcg_explain():
    hdr = open(os.path.join(REPO, "include", "hcatgnet_hip.h")).read()
    assert "hcg_gcn_edge_weight_grad" not in hdr
    code = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    declared = set(re.findall(r"\b(hcg_[a-z0-9_]+)\s*\(", code))
    assert "hcg_explain" in declared and len(declared) <= 55
    assert "hcg_gcn_edge_weight_grad" not in _lib.SIGNATURES and "hcg_explain" in _lib.SIGNATURES
    lib = ctypes.CDLL(_lib.LIB_PATH)
    assert not hasattr(lib, "hcg_gcn_edge_weight_grad")
    assert hasattr(lib, "hcg_explain")
    assert _lib.load().hcg_version() == 1
    # the layer mode's query needs no workspace; its launch arguments are validated like the old entry point's
    a = _lib.ExplainArgs()
    a.mode, a.flags = _lib.HCG_EXPLAIN_LAYER_EDGE_GRAD, _lib.HCG_EXPLAIN_QUERY
    assert _lib.load().hcg_explain(ctypes.addressof(a), None) == 0 and a.workspace_bytes_needed == 0
    a.flags, a.N, a.E, a.D = 0, 4, 3, 0
    assert _lib.load().hcg_explain(ctypes.addressof(a), None) == -1           # D <= 0
    a.D, a.N = 64, 0
    assert _lib.load().hcg_explain(ctypes.addressof(a), None) == 0            # no nodes: nothing to do


def test_explain_step_support_check_is_host_only():
    """`ExplainStep.reason` decides on the host (no GPU, no sync) whether a model / batch takes the one-launch kernel."""
    x = torch.zeros(4, 25); ei = torch.zeros(2, 0, dtype=torch.int64); bv = torch.zeros(4, dtype=torch.int64)
    mk = lambda **kw: H.Batch(x, ei, bv, 1, **kw)
    step = ExplainStep(H.make_network("GCN", H.default_options(), 25))
    assert step.reason() is None
    assert step.reason(mk(max_nodes=30, max_edges=64, edges_grouped=True)) is None
    assert step.reason(mk(max_nodes=184, max_edges=390, edges_grouped=True)) is None
    assert step.reason(mk(max_nodes=224, max_edges=1024, edges_grouped=True)) is None
    assert "shape" in step.reason(mk(max_nodes=225, max_edges=390, edges_grouped=True))
    assert "shape" in step.reason(mk(max_nodes=184, max_edges=1025, edges_grouped=True))
    assert "metadata" in step.reason(mk())
    assert "metadata" in step.reason(mk(max_nodes=30, max_edges=64))
    wrong = H.Batch(torch.zeros(4, 32), ei, bv, 1, max_nodes=30, max_edges=64, edges_grouped=True)
    assert "features" in step.reason(wrong)
    for kw in (dict(embedding_dim=128), dict(n_convolutions=5), dict(n_classes=9)):
        assert "shape" in ExplainStep(H.make_network("GCN", H.default_options(**kw), 25)).reason(), kw
    assert "shape" in ExplainStep(H.make_network("GCN", H.default_options(), 65)).reason()
    for kw in (dict(n_convolutions=1, readout_layers=1), dict(n_convolutions=3, readout_layers=3, n_classes=2),
               dict(n_convolutions=4, readout_layers=4, n_classes=8)):
        deep = ExplainStep(H.make_network("GCN", H.default_options(**kw), 32))
        assert deep.reason() is None, kw
    off = H.make_network("GCN", H.default_options(use_fused=False), 25)
    assert "disabled" in ExplainStep(off).reason()
    assert step.last_path is None


_LIMITS = "embedding_dim 64, <= 64 node features, <= 4 conv layers, readout depth <= 4, <= 8 classes, graphs of <= {} nodes and <= 1024 directed edges)"
_ONE = dict(off="fused kernels disabled on the model", weight="explicit edge weights cannot be combined with masks",
            feat="batch has 32 node features, the model takes 25")
_MANY = dict(off="fused kernels disabled on a model", weight="explicit edge weights are outside the ensemble kernel",
             feat="batch has 32 node features, the models take 25")
_FROZEN = {
    "explain": dict(make=lambda m: ExplainStep(m), nodes=224, cpu=False, **_ONE,
                    limit="model / graph shape outside the one-launch explain kernel (" + _LIMITS.format(224)),
    "ensemble": dict(make=lambda m: H.ensemble.EnsemblePredict([m]), nodes=224, cpu=False, **_MANY,
                     limit="model / graph shape outside the one-launch ensemble kernel (" + _LIMITS.format(224)),
    "shapley": dict(make=lambda m: H.shapley.ShapleySampling(m), nodes=184, cpu=True, **_ONE,
                    limit="model / graph shape outside the on-chip Shapley kernel (" + _LIMITS.format(184)),
    "fit": dict(make=lambda m: H.explain.ExplainFit(m), nodes=224, cpu=True, **_ONE,
                limit="model / graph shape outside the one-launch explainer fit kernel (" + _LIMITS.format(224)),
    "integrated": dict(make=lambda m: H.attribution.IntegratedGradients(m), nodes=224, cpu=True, **_ONE,
                       limit="model / graph shape outside the one-launch integrated gradients kernel (" + _LIMITS.format(224)),
    "ensemble_attribution": dict(make=lambda m: H.attribution.EnsembleAttribution([m]), nodes=224, cpu=True, **_MANY,
                                 limit="model / graph shape outside the one-launch integrated gradients kernel (" + _LIMITS.format(224)),
}


def _stand_in(F=25, is_cuda=True, N=4, E=0, **kw):
    """`reason` and `_shape_args` read host metadata only, so a stand-in batch serves."""
    from types import SimpleNamespace as NS
    return NS(x=NS(is_cuda=is_cuda, shape=(N, F)), edge_index=NS(shape=(2, E)), num_graphs=1, **kw)


@pytest.mark.parametrize("name", sorted(_FROZEN))
def test_frozen_classes_keep_their_own_reason_strings(name):
    """The six frozen-model classes share one support check (hcatgnet_amd/_frozen.py); each still answers in its own
    words.  The stand-in's x claims to be on a GPU: four of the six ask that first, and say so when it is not."""
    import hcatgnet_amd.attribution, hcatgnet_amd.ensemble, hcatgnet_amd.shapley  # noqa: F401
    mk = _stand_in
    w = _FROZEN[name]
    meta = dict(max_nodes=30, max_edges=64, edges_grouped=True)
    obj = w["make"](H.make_network("GCN", H.default_options(), 25))
    assert obj.reason() is None and obj.reason(mk(**meta)) is None
    assert obj.reason(mk(max_nodes=w["nodes"], max_edges=1024, edges_grouped=True)) is None
    assert obj.reason(mk()) == "batch lacks collate metadata (max_nodes / max_edges / grouped edges)"
    assert obj.reason(mk(edge_weight=torch.ones(0), **meta)) == w["weight"]
    assert obj.reason(mk(F=32, **meta)) == w["feat"]
    assert obj.reason(mk(max_nodes=w["nodes"] + 1, max_edges=64, edges_grouped=True)) == w["limit"]
    assert w["make"](H.make_network("GCN", H.default_options(use_fused=False), 25)).reason() == w["off"]
    if w["cpu"]:
        assert obj.reason(mk(is_cuda=False, **meta)) == "the batch is on the CPU"
    assert obj.last_path is None


def test_buffer_pool_grows_one_name_at_a_time():
    """The frozen-model classes' buffers (`obj._bufs`): name -> flat tensor, as large as the largest request seen for the
    name, at least 1 element; a request returns the buffer's front in the shape asked for."""
    from hcatgnet_amd._frozen import Pool
    pool, cpu = Pool(), torch.device("cpu")
    a, b = pool.take("a", (2, 3), cpu), pool.take("b", (4,), cpu)
    assert a.shape == (2, 3) and a.is_contiguous() and a.dtype == torch.float32 and not a.any() and not b.any()      # fresh storage is zero
    assert pool["a"].shape == (6,) and pool["b"].shape == (4,) and sorted(pool) == ["a", "b"]
    a.fill_(3.0)
    pa, pb = pool["a"].data_ptr(), pool["b"].data_ptr()
    for shape in ((5,), (2, 3), (1, 2, 3)):                                       # requests that fit: the same storage
        fit = pool.take("a", shape, cpu)
        assert fit.data_ptr() == pa and pool["a"].data_ptr() == pa and fit.shape == shape and bool((fit == 3.0).all())
    grown = pool.take("a", (3, 3), cpu)                                           # a larger one: this name alone regrows, to the request
    assert pool["a"].shape == (9,) and grown.shape == (3, 3) and not grown.any() and grown.data_ptr() == pool["a"].data_ptr()
    assert pool["b"].data_ptr() == pb and pool["b"].numel() == 4
    assert pool.take("a", (2, 3), cpu).data_ptr() == pool["a"].data_ptr() and pool["a"].numel() == 9      # never shrinks
    none = pool.take("c", (0, 25), cpu)
    assert none.shape == (0, 25) and pool["c"].numel() == 1 and pool.take("i", (3,), cpu, torch.int32).dtype == torch.int32
    meta = pool.take("b", (2,), torch.device("meta"))                             # another device: reallocated, to the request
    assert meta.device.type == "meta" and pool["b"].device.type == "meta" and pool["b"].numel() == 2
    back = pool.take("b", (2,), cpu)
    assert back.device.type == "cpu" and pool["b"].device.type == "cpu" and not back.any()
    ws = pool.workspace(10, cpu)
    assert ws.dtype == torch.uint8 and ws.numel() == 256 and pool["ws"] is ws and pool.workspace(200, cpu) is ws
    assert pool.workspace(1000, cpu).numel() == 1000 and pool.workspace(10, cpu).numel() == 1000


def _set_by_query(extra=()):
    return {"mode", "flags", "F", "D", "C", "n_conv", "R", "N", "E", "B", "max_nodes", "max_edges",
            "workspace_bytes_needed", "lds_bytes", *extra}


_SHAPE_ARGS = {
    "explain": (lambda m: ExplainStep(m), {}, _set_by_query()),
    "fit": (lambda m: H.explain.ExplainFit(m), {}, _set_by_query()),
    "ensemble": (lambda m: H.ensemble.EnsemblePredict([m]), {}, _set_by_query(("n_models", "models_per_group"))),
    "shapley": (lambda m: H.shapley.ShapleySampling(m), dict(perm_count=3), _set_by_query(("perm_count",))),
    "shapley_grouped": (lambda m: H.shapley.ShapleySampling(m),
                        dict(perm_count=3, flags=_lib.HCG_EXPLAIN_QUERY | _lib.HCG_EXPLAIN_GROUPED, shap_n_groups=7),
                        _set_by_query(("perm_count", "shap_n_groups"))),
    "integrated": (lambda m: H.attribution.IntegratedGradients(m), {}, _set_by_query()),
    "ensemble_attribution": (lambda m: H.attribution.EnsembleAttribution([m]), {}, _set_by_query(("n_models",))),
}


@pytest.mark.parametrize("name", sorted(_SHAPE_ARGS))
def test_shape_query_leaves_nothing_of_an_earlier_launch(name):
    """A class reuses one argument block, whose `fit_` / `path_` / `mom_` / `shap_` members overlay one union: whatever an
    earlier launch left there must not reach the next one.  Every byte of a block is set to 0xFF; after the class's
    `_shape_args` every byte outside the members the query itself sets (shapes, mode, flags, its counts and the library's
    two answers) is 0, so a launch reads only what the class sets after the query.  Before `_frozen.query` cleared the
    block this failed for every class: each nulled a hand-kept list of pointers and left the rest."""
    import hcatgnet_amd.attribution, hcatgnet_amd.ensemble, hcatgnet_amd.shapley  # noqa: F401
    make, extra, set_here = _SHAPE_ARGS[name]
    obj = make(H.make_network("GCN", H.default_options(), 25))
    a = _lib.ExplainArgs()
    size = ctypes.sizeof(a)
    ctypes.memset(ctypes.addressof(a), 0xFF, size)
    batch = _stand_in(N=30, E=64, max_nodes=30, max_edges=64, edges_grouped=True)
    assert obj._shape_args(a, batch, **extra) is None
    assert (a.N, a.E, a.B, a.F, a.max_nodes, a.max_edges) == (30, 64, 1, 25, 30, 64)
    assert a.workspace_bytes_needed > 0 or name == "ensemble"                  # (the ensemble kernel needs no workspace)
    left = bytearray(ctypes.string_at(ctypes.addressof(a), size))
    span = lambda f: range(getattr(_lib.ExplainArgs, f).offset, getattr(_lib.ExplainArgs, f).offset + getattr(_lib.ExplainArgs, f).size)
    written = set()
    for field in set_here:
        written.update(span(field))
    for i in written:
        left[i] = 0
    stale = [i for i, v in enumerate(left) if v]
    assert not stale, f"{len(stale)} stale bytes, the first at offset {stale[0]}"
    # the same, member by member: the structure's own fields and the three blocks that overlay its `fit_` members
    names = [f[0] for f in _lib.ExplainArgs._fields_] + [f[0] for f in _lib.PATH_FIELDS + _lib.MOMENT_FIELDS + _lib.SHAPLEY_GROUP_FIELDS]
    assert len(names) > 100
    for field in names:
        if field in set_here or written.intersection(span(field)):
            continue
        v = getattr(a, field)
        assert v is None or v == 0 or (not isinstance(v, (int, float)) and not any(v)), field       # (pointer, number, array)
