"""What tests/test_host_ensemble_shapley.py and tests/test_gpu_ensemble_shapley.py share (tests only).

Models.  Model k of an ensemble is `shapley_ref.rand_params(F, 64, seed=PARAM_SEED + k, **depths)`: with the seed of
tests/test_gpu_subsets.py, model 0 is that file's own model of the case.

Yardsticks.  Per model: `torch.equal` with the existing, tested single-model classes (`ShapleySampling`, `SubsetValues`) on
`models[m]` -- no tolerance, and their fp64-oracle parity carries over.  Moments: `ensemble_attr_ref.moment_figures`, the
bound (M + 4) 2^-24 s derived in that module.  Areas: a Python trapezoid in float64 over the class's own points, within the
bound tests/subsets_ref.py states for `AttributionCurves`.

`library_level` is the part of the checks that needs the library alone (queries and refused launches: no device memory)."""
import ctypes

import torch

from tests import shapley_ref as SR

PARAM_SEED = 23          # tests/test_gpu_subsets.py's
TWO = dict(n_conv=2, n_read=2, n_classes=1)
DEEP = dict(n_conv=4, n_read=4, n_classes=8)
HCG_OK, HCG_ERR_INVALID_ARG = 0, -1          # include/hcatgnet_hip.h


def models(H, F, M, depths, device="cpu"):
    return [SR.model_from_params(H, SR.rand_params(F, 64, seed=PARAM_SEED + k, **depths)).to(device) for k in range(M)]


def group_total(ng, batch_vec, B):
    """G of a `node_group` alone ([N] or [N, F]; ids valid): the sum over the graphs of (largest id + 1)"""
    ids = ng if ng.dim() == 1 else ng.amax(1)
    top = torch.full((B,), -1, dtype=torch.int64).scatter_reduce(0, batch_vec, ids.to(torch.int64), reduce="amax")
    return int((top + 1).sum())


def _args(_lib, mode, n_models, flags=None, **more):
    a = _lib.ExplainArgs()
    a.mode = mode
    a.flags = _lib.HCG_EXPLAIN_QUERY if flags is None else flags
    a.F, a.D, a.C, a.n_conv, a.R = 25, 64, 1, 2, 2
    a.max_nodes, a.max_edges, a.N, a.E, a.B = 40, 90, 120, 270, 3
    a.n_models = n_models
    for k, v in more.items():
        setattr(a, k, v)
    return a


def library_level(_lib):
    """n_models outside 1 .. 65535 is HCG_ERR_INVALID_ARG in the two modes with a model axis (0 means 1); the coalition and
    the greedy mode answer HCG_ERR_UNSUPPORTED for two models; the walk's query reports M times the one-model workspace."""
    lib = _lib.load()
    call = lambda a: lib.hcg_explain(ctypes.addressof(a), None)                     # noqa: E731
    S, V, Cm, Gm = _lib.HCG_EXPLAIN_SHAPLEY, _lib.HCG_EXPLAIN_SUBSETS, _lib.HCG_EXPLAIN_COALITIONS, _lib.HCG_EXPLAIN_GREEDY
    G = _lib.HCG_EXPLAIN_QUERY | _lib.HCG_EXPLAIN_GROUPED
    for mode, more in ((S, dict(perm_count=3)), (S, dict(perm_count=3, flags=G, shap_n_groups=12)), (V, dict(coal_rows=5, sub_max_groups=7))):
        for bad in (-1, 65536):
            assert call(_args(_lib, mode, bad, **more)) == HCG_ERR_INVALID_ARG, (mode, bad)
            assert call(_args(_lib, mode, bad, **dict(more, flags=more.get("flags", 0) & ~_lib.HCG_EXPLAIN_QUERY))) == HCG_ERR_INVALID_ARG
        for ok in (0, 1, 7, 65535):
            assert call(_args(_lib, mode, ok, **more)) == HCG_OK, (mode, ok)
    for mode, more in ((Cm, dict(coal_rows=8, coal_max_live=3)), (Gm, dict(sub_max_groups=7))):
        assert call(_args(_lib, mode, 0, **more)) == call(_args(_lib, mode, 1, **more)) == HCG_OK
        assert call(_args(_lib, mode, 2, **more)) == _lib.HCG_ERR_UNSUPPORTED
        assert call(_args(_lib, mode, 2, flags=0, **more)) == _lib.HCG_ERR_UNSUPPORTED      # a launch too: never one model silently
    figures = {}
    for more in (dict(perm_count=3), dict(perm_count=3, flags=G, shap_n_groups=12)):
        one = _args(_lib, S, 1, **more)
        assert call(one) == HCG_OK and int(one.workspace_bytes_needed) > 0
        zero = _args(_lib, S, 0, **more)
        assert call(zero) == HCG_OK and int(zero.workspace_bytes_needed) == int(one.workspace_bytes_needed)
        for M in (2, 7, 90):
            a = _args(_lib, S, M, **more)
            assert call(a) == HCG_OK and int(a.workspace_bytes_needed) == M * int(one.workspace_bytes_needed)
            assert int(a.lds_bytes) == int(one.lds_bytes)
        figures[more.get("shap_n_groups", 0)] = int(one.workspace_bytes_needed)
    a = _args(_lib, V, 5, coal_rows=5, sub_max_groups=7)
    assert call(a) == HCG_OK and int(a.workspace_bytes_needed) == 0
    return figures
