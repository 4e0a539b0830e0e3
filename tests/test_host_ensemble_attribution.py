"""Host side of `hcatgnet_amd.attribution.EnsembleAttribution` (no GPU): constructor refusals, the library's query with a
model axis, the moments mode's validation, the default chunking, the argument block's size, the float32 restatement of the
moments' recurrence against the bound of tests/ensemble_attr_ref.py, and the loop path on CPU tensors.  Every figure is
printed before it is asserted (`pytest -s`)."""
import ctypes
import os

import numpy as np
import pytest
import torch

import hcatgnet_amd as H
from hcatgnet_amd import _lib
from hcatgnet_amd import attribution as A
from hcatgnet_amd.attribution import EnsembleAttribution, EnsembleAttributionResult, IntegratedGradients
from tests import ensemble_attr_ref as ER
from tests import integrated_ref as R

OK, INVALID, UNSUPPORTED = 0, -1, _lib.HCG_ERR_UNSUPPORTED
EXPLAIN_ARGS_BYTES = 608          # sizeof(hcg_explain_args) before the model axis and the moments mode existed


@pytest.fixture(scope="module", autouse=True)
def built():
    if not os.path.isfile(_lib.LIB_PATH):
        import __graft_entry__
        __graft_entry__.build()


# ------------------------------------------------------------------------------------------------ the constructor
def test_constructor_refusals():
    with pytest.raises(ValueError, match="at least one model"):
        EnsembleAttribution([])
    two = H.make_network("GCN", H.default_options(), 25)
    three = H.make_network("GCN", H.default_options(n_convolutions=3), 25)
    with pytest.raises(ValueError, match="conv layers"):
        EnsembleAttribution([two, three])
    with pytest.raises(ValueError, match="conv layers"):
        EnsembleAttribution([two, H.make_network("GCN", H.default_options(readout_layers=3), 25)])
    with pytest.raises(ValueError, match="not a hcatgnet_amd GCN"):
        EnsembleAttribution([two, torch.nn.Linear(3, 3)])
    with pytest.raises(ValueError, match="gradient"):
        EnsembleAttribution([two], saliency=True)
    with pytest.raises(ValueError, match="max-pool"):
        EnsembleAttribution([two], method="riemann_left")
    with pytest.raises(ValueError, match="n_steps"):
        EnsembleAttribution([two], n_steps=0)
    ea = EnsembleAttribution([two, two], n_steps=50, method="gradient", saliency=True)
    assert ea.n_steps == 1 and ea.saliency and ea.n_models == 2 and ea.last_path is None
    assert ea.reason() is None
    c = R.case("deep")
    b = R.batch(H, c)
    ea = EnsembleAttribution(ER.models(H, "deep", 2), n_steps=2)
    for kw in (dict(class_index=2), dict(class_index=-1)):
        with pytest.raises(ValueError, match="class_index"):
            ea(b, **kw)
    for kw in (dict(models_per_launch=0), dict(steps_per_launch=0)):
        with pytest.raises(ValueError, match="per_launch"):
            ea(b, **kw)
    assert ea.last_path is None


# ------------------------------------------------------------------------------------------------ the library
def _args(n_models=None, nodes=184, edges=390, N=None, B=1, n_conv=2, query=True):
    a = _lib.ExplainArgs()
    a.mode, a.flags = _lib.HCG_EXPLAIN_INTEGRATED, (_lib.HCG_EXPLAIN_QUERY if query else 0)
    a.F, a.D, a.C, a.n_conv, a.R = 25, 64, 1, n_conv, 2
    a.max_nodes, a.max_edges = nodes, edges
    a.N, a.E, a.B = nodes if N is None else N, edges, B
    if n_models is not None:
        a.n_models = n_models
    return a


def _call(a):
    return _lib.load().hcg_explain(ctypes.addressof(a), None), int(a.workspace_bytes_needed)


def test_the_query_accounts_for_the_model_axis():
    rc, one = _call(_args())                      # (n_models left 0: what every caller of the one-model form passes)
    assert rc == OK and one >= 2 * 2 * 184 * 64 * 4
    assert _call(_args(n_models=1)) == (OK, one)
    for M in (2, 3, 9, 90, 65535):
        rc, ws = _call(_args(n_models=M))
        print(f"    n_models {M}: workspace {ws} bytes = {M} x {one}")
        assert rc == OK and ws == M * one
    rc, big = _call(_args(n_models=90, nodes=120, edges=250, N=535 * 120, B=535))
    assert rc == OK and big == 90 * _call(_args(nodes=120, edges=250, N=535 * 120, B=535))[1]
    for M in (65536, 1 << 20, -1):
        assert _call(_args(n_models=M))[0] == INVALID, M
    # the shape limits come first, as for one model
    a = _args(n_models=70000, nodes=225)
    assert _call(a)[0] == UNSUPPORTED
    # a launch with models checks its pointers like the one-model launch: nothing is launched on NULL
    a = _args(n_models=3, query=False)
    a.path_steps, a.path_step_first, a.path_step_count, a.path_class_index = 4, 0, 4, 0
    assert _call(a)[0] == INVALID
    a = _args(n_models=70000, query=False, B=0, N=0)
    a.path_steps, a.path_step_count = 4, 4
    assert _call(a)[0] == INVALID


def test_moments_mode_validation():
    assert _lib.HCG_EXPLAIN_MOMENTS == 6

    def mom(query=True, **kw):
        a = _lib.ExplainArgs()
        a.mode, a.flags = _lib.HCG_EXPLAIN_MOMENTS, (_lib.HCG_EXPLAIN_QUERY if query else 0)
        for k, v in dict(dict(mom_total=5, mom_first=0, mom_count=5, mom_len0=100, mom_len1=7), **kw).items():
            setattr(a, k, v)
        return a

    assert _call(mom()) == (OK, 0)
    assert _call(mom(mom_first=2, mom_count=3))[0] == OK and _call(mom(mom_first=5, mom_count=0))[0] == OK
    for bad in (dict(mom_total=0, mom_count=0), dict(mom_first=-1), dict(mom_count=-1), dict(mom_first=3, mom_count=3),
                dict(mom_len0=-1), dict(mom_len1=1 << 31)):
        assert _call(mom(**bad))[0] == INVALID, bad
    a = mom()
    a.flags |= _lib.HCG_EXPLAIN_TARGET_CLASS
    assert _call(a)[0] == INVALID
    # a launch: nothing to do returns OK before any pointer is looked at; otherwise it stops at the NULL pointers
    assert _call(mom(query=False, mom_count=0))[0] == OK and _call(mom(query=False, mom_len0=0, mom_len1=0))[0] == OK
    assert _call(mom(query=False))[0] == INVALID


def test_the_argument_block_keeps_its_size_and_the_moment_fields_fit_the_union():
    X = _lib.ExplainArgs
    assert ctypes.sizeof(X) == EXPLAIN_ARGS_BYTES == _lib.load().hcg_struct_bytes(_lib.HCG_STRUCT_EXPLAIN_ARGS)
    names = [n for n, _ in _lib.MOMENT_FIELDS]
    assert names == ["mom_values0", "mom_values1", "mom_mean0", "mom_mean1", "mom_m20", "mom_m21", "mom_std0", "mom_std1", "mom_len0",
                     "mom_len1", "mom_total", "mom_first", "mom_count", "mom_reserved"]
    first, last = getattr(X, names[0]), getattr(X, names[-1])
    assert first.offset == X.fit_edge_logit.offset == X.path_alpha.offset
    assert last.offset + 4 <= X.fit_coeffs.offset + X.fit_coeffs.size <= ctypes.sizeof(X)      # no larger than the fit_ block
    assert X.n_models.offset == 416 and X.fit_edge_logit.offset == 472                         # (the offsets before this change)
    a = X()
    a.mom_values0, a.mom_len1, a.mom_count = 0x1234, 77, 3
    assert a.fit_edge_logit == 0x1234 and a.path_alpha == 0x1234 and a.mom_len1 == 77 and a.mom_count == 3


def test_the_header_and_the_mirror_agree_on_the_moment_fields():
    import shutil
    import subprocess
    import tempfile
    cc = next((p for p in (shutil.which(n) for n in ("cc", "gcc", "clang", "c++", "g++", "hipcc")) if p), None)
    if cc is None:
        cc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    repo = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    c_names = ["mom_values[0]", "mom_values[1]", "mom_mean[0]", "mom_mean[1]", "mom_m2[0]", "mom_m2[1]", "mom_std[0]", "mom_std[1]",
               "mom_len[0]", "mom_len[1]", "mom_total", "mom_first", "mom_count", "mom_reserved"]
    prints = "".join(f' printf(" %zu", offsetof(hcg_explain_args, {n}));' for n in c_names)
    with tempfile.TemporaryDirectory() as d:
        src, exe = os.path.join(d, "s.c"), os.path.join(d, "s")
        open(src, "w").write('#include <stdio.h>\n#include <stddef.h>\n#include "hcatgnet_hip.h"\nint main(void) { '
                             'printf("%zu %d", sizeof(hcg_explain_args), HCG_EXPLAIN_MOMENTS);' + prints + ' return 0; }\n')
        subprocess.run([cc, "-I", os.path.join(repo, "include"), src, "-o", exe], check=True, capture_output=True)
        got = [int(v) for v in subprocess.run([exe], check=True, capture_output=True, text=True).stdout.split()]
    assert got[0] == EXPLAIN_ARGS_BYTES and got[1] == _lib.HCG_EXPLAIN_MOMENTS
    assert got[2:] == [getattr(_lib.ExplainArgs, n).offset for n, _ in _lib.MOMENT_FIELDS]


# ------------------------------------------------------------------------------------------------ the default chunking
def test_default_chunking_arithmetic():
    f = EnsembleAttribution.default_models_per_launch
    assert A.LAUNCH_BUDGET_BYTES == 1 << 30
    ws, entries = 2 * 2 * 2000 * 64 * 4, 2000 * 25 + 4500              # 52 real-size graphs, two conv layers
    assert f(90, ws, entries) == 90 and f(1, ws, entries) == 1
    per = ws + 4 * entries
    ws_big, entries_big = 2 * 2 * 64200 * 64 * 4, 64200 * 25 + 134000   # 535 graphs of 120 nodes
    got = f(90, ws_big, entries_big)
    per_big = ws_big + 4 * entries_big
    print(f"\n    52 graphs: {per} bytes per model, all 90 in one launch; 535 graphs: {per_big} bytes per model, {got} per launch")
    assert 1 <= got < 90 and got * per_big <= A.LAUNCH_BUDGET_BYTES < (got + 1) * per_big
    assert f(90, ws, entries, budget=10 * per) == 10 and f(90, ws, entries, budget=10 * per - 1) == 9
    assert f(90, ws, entries, budget=1) == 1                          # (one model always runs)
    # the steps of a launch: IntegratedGradients' rule with graphs x models workgroups
    g = IntegratedGradients.default_steps_per_launch
    assert g(50, 52 * 90) == 50 and g(50, 535 * 90) == g(50, 48150) < 50


# ------------------------------------------------------------------------------------------------ the recurrence in float32
@pytest.mark.parametrize("M", [1, 2, 3, 5, 9, 90])
def test_the_float32_recurrence_meets_the_bound(M):
    rng = np.random.default_rng(1234 + M)
    L = 20000
    normal = rng.standard_normal((M, L))
    near = 3.0 + 1e-4 * rng.standard_normal((M, L))
    wide = rng.standard_normal((M, L)) * 10.0 ** rng.uniform(-6, 6, size=(M, L))
    sparse = rng.standard_normal((M, L)) * (rng.random((M, L)) >= 0.3)
    sparse[:, :50] = 0.0
    for tag, v in (("normal", normal), ("nearly equal", near), ("wide-range", wide), ("30 % zero", sparse)):
        v = v.astype(np.float32)
        mean, std = ER.welford32(v)
        assert mean.dtype == std.dtype == np.float32
        fig = ER.moment_figures(torch.from_numpy(v), torch.from_numpy(mean), torch.from_numpy(std))
        print(f"    M {M} {tag}: worst |got - fp64| / ((M + 4) 2^-24 s): mean {fig['mean']:.3f} std {fig['std']:.3f} "
              f"(= {fig['mean'] * (M + 4):.2f} / {fig['std'] * (M + 4):.2f} ulps of s); all-zero entries {fig['zeros']}")
        assert fig["mean"] <= 1.0 and fig["std"] <= 1.0 and fig["zeros_exact"]
        if tag == "30 % zero":
            assert fig["zeros"] >= 50
        if M == 1:
            assert np.array_equal(mean, v[0]) and not std.any()
    same = np.repeat(normal[:1].astype(np.float32), M, axis=0)
    mean, std = ER.welford32(same)
    assert np.array_equal(mean, same[0]) and not std.any()            # (d is exactly 0 from the second model on)


# ------------------------------------------------------------------------------------------------ the loop path on CPU tensors
def test_loop_path_on_cpu_tensors_is_the_per_model_autograd():
    c = R.case("small30")
    M = 3
    models = ER.models(H, "small30", M)
    b = R.batch(H, c)
    before = [[q.detach().clone() for q in m.parameters()] for m in models]
    ea = EnsembleAttribution(models, n_steps=c.n_steps)
    assert ea.reason(b) == "the batch is on the CPU"
    r = ea(b, class_index=c.cls, per_model=True)
    assert ea.last_path == "loop" and isinstance(r, EnsembleAttributionResult)
    assert tuple(r.node_attr.shape) == (M,) + tuple(c.x.shape) and tuple(r.edge_attr.shape) == (M, c.ei.shape[1])
    assert tuple(r.out_full.shape) == tuple(r.out_base.shape) == (M, c.B, 1)
    for m in range(M):
        one = IntegratedGradients(models[m], n_steps=c.n_steps)(b, class_index=c.cls)      # (torch autograd on CPU tensors)
        assert torch.equal(r.node_attr[m], one.node_attr) and torch.equal(r.edge_attr[m], one.edge_attr), m
        assert torch.equal(r.out_full[m], one.out_full) and torch.equal(r.out_base[m], one.out_base), m
    # model 0 is the case's own model: its screened fp64 reference holds
    R.check(c, A.IntegratedGradientsResult(r.node_attr[0], r.edge_attr[0], r.out_full[0], r.out_base[0]), "small30 model 0 (loop, CPU)")
    ER.check_moments(r.node_attr, r.edge_attr, r, "small30 (loop, CPU)")
    q = ea(b, class_index=c.cls)
    assert q.node_attr is None and q.edge_attr is None and torch.equal(q.node_mean, r.node_mean) and torch.equal(q.edge_std, r.edge_std)
    for m, ws in zip(models, before):
        for p, w in zip(m.parameters(), ws):
            assert torch.equal(p.detach(), w) and p.grad is None
