"""Host side of `hcatgnet_amd.attribution.IntegratedGradients` (no GPU): the quadrature, validation, the loop path on CPU
tensors against the fp64 reference with the checks the GPU tests apply to the kernel (tests/integrated_ref.py states
reference, screen and bound), `convergence_delta`, `reason`, and the library's HCG_EXPLAIN_INTEGRATED query and argument
block.  Every figure is printed before it is asserted (`pytest -s`)."""
import ctypes
import os
import shutil
import subprocess
import tempfile

import numpy as np
import pytest
import torch

import hcatgnet_amd as H
from hcatgnet_amd import _lib
from hcatgnet_amd.attribution import IntegratedGradients, IntegratedGradientsResult, convergence_delta, quadrature
from tests import integrated_ref as R

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module", autouse=True)
def built():
    if not os.path.isfile(_lib.LIB_PATH):
        import __graft_entry__
        __graft_entry__.build()


# ------------------------------------------------------------------------------------------------ quadrature
@pytest.mark.parametrize("n", [1, 2, 3, 4, 6, 50])
def test_gausslegendre_points_are_numpys(n):
    alpha, weight = quadrature("gausslegendre", n)
    t, w = np.polynomial.legendre.leggauss(n)
    assert alpha.dtype == weight.dtype == torch.float32 and tuple(alpha.shape) == tuple(weight.shape) == (n,)
    assert torch.equal(alpha, torch.from_numpy(((t + 1) / 2).astype(np.float32)))
    assert torch.equal(weight, torch.from_numpy((w / 2).astype(np.float32)))
    total = float(weight.double().sum())
    print(f"\n    gausslegendre n = {n}: sum of the weights - 1 = {total - 1:.2e}, points in [{float(alpha.min()):.4f}, {float(alpha.max()):.4f}]")
    assert abs(total - 1.0) <= 1e-6 and bool(((alpha > 0) & (alpha < 1)).all())
    assert not alpha.is_cuda and not weight.is_cuda


@pytest.mark.parametrize("n", [1, 4, 7, 50])
def test_riemann_middle_points(n):
    alpha, weight = quadrature("riemann_middle", n)
    assert torch.equal(alpha, torch.from_numpy(((np.arange(n) + 0.5) / n).astype(np.float32)))
    assert torch.equal(weight, torch.full((n,), np.float32(1.0 / n)))
    assert abs(float(weight.double().sum()) - 1.0) <= 1e-6 and bool(((alpha > 0) & (alpha < 1)).all())


def test_the_one_step_method():
    alpha, weight = quadrature("gradient", 1)
    assert alpha.tolist() == [1.0] and weight.tolist() == [1.0]
    m = H.make_network("GCN", H.default_options(), 25)
    assert IntegratedGradients(m, n_steps=50, method="gradient").n_steps == 1          # (forced)
    with pytest.raises(ValueError):
        quadrature("gradient", 2)
    with pytest.raises(ValueError, match="gradient"):
        IntegratedGradients(m, saliency=True)


def test_validation_errors():
    c = R.case("deep")
    m, b = R.model(H, c), R.batch(H, c)
    for method in ("riemann_left", "riemann_right", "riemann_trapezoid"):
        with pytest.raises(ValueError, match="alpha = 0"):
            quadrature(method, 8)
        with pytest.raises(ValueError, match="max-pool"):
            IntegratedGradients(m, method=method)
    with pytest.raises(ValueError, match="method"):
        quadrature("simpson", 8)
    for n in (0, -3):
        with pytest.raises(ValueError, match="n_steps"):
            quadrature("gausslegendre", n)
        with pytest.raises(ValueError, match="n_steps"):
            IntegratedGradients(m, n_steps=n)
        with pytest.raises(ValueError, match="n_steps"):
            IntegratedGradients(m)(b, n_steps=n)
    ig = IntegratedGradients(m, n_steps=2)
    for cls in (-1, 2, 7):                                            # (the model has two classes)
        with pytest.raises(ValueError, match="class_index"):
            ig(b, class_index=cls)
    with pytest.raises(ValueError, match="steps_per_launch"):
        ig(b, steps_per_launch=0)
    assert ig.last_path is None


# ------------------------------------------------------------------------------------------------ the loop path on CPU tensors
@pytest.mark.parametrize("name", ["small30", "deep"])
def test_loop_path_on_cpu_tensors(name):
    c = R.case(name)
    m, b = R.model(H, c), R.batch(H, c)
    before = [q.detach().clone() for q in m.parameters()]
    ig = IntegratedGradients(m, n_steps=c.n_steps)
    assert ig.reason(b) == "the batch is on the CPU"
    r = ig(b, class_index=c.cls)
    assert ig.last_path == "loop" and isinstance(r, IntegratedGradientsResult)
    R.check(c, r, name + " (loop, CPU)")
    for q, w in zip(m.parameters(), before):
        assert torch.equal(q.detach(), w) and q.grad is None


def test_convergence_delta_is_the_stated_formula():
    """sum of graph g's attributions - (out_full - out_base)[g, c], on the fp64 reference's numbers."""
    c = R.case("deep")
    b = R.batch(H, c)
    ref = c.ref
    want = torch.zeros(c.B, dtype=torch.float64)
    for g in range(c.B):
        want[g] = ref["node"][c.batch == g].sum() + ref["edge"][c.edge_owner == g].sum() - (ref["out_full"][g, c.cls] - ref["out_base"][g, c.cls])
    r64 = IntegratedGradientsResult(ref["node"], ref["edge"], ref["out_full"], ref["out_base"])
    got = convergence_delta(b, r64, c.cls)
    err = float((got - want).abs().max())
    print(f"\n    convergence delta per graph (fp64 reference, {c.n_steps} points): {[f'{v:+.3e}' for v in got.tolist()]}; formula error {err:.1e}")
    assert got.dtype == torch.float64 and tuple(got.shape) == (c.B,) and err <= 1e-12
    ig = IntegratedGradients(R.model(H, c), n_steps=c.n_steps)
    r = ig(b, class_index=c.cls)
    mine = ig.convergence_delta(b, r)                                 # (the class index of the last call)
    assert mine.dtype == torch.float64 and float((mine - convergence_delta(b, r, c.cls)).abs().max()) <= 1e-12
    scale = float((ref["out_full"] - ref["out_base"]).abs().max())
    assert float((mine - want).abs().max()) <= 1e-4 * max(scale, 1.0)   # float32 attributions of ~1e3 entries against fp64


def test_reason_strings():
    from types import SimpleNamespace as NS

    def mk(F=25, **kw):
        return NS(x=NS(is_cuda=True, shape=(4, F)), edge_index=NS(shape=(2, 0)), num_graphs=1, **kw)

    ig = IntegratedGradients(H.make_network("GCN", H.default_options(), 25))
    meta = dict(max_nodes=30, max_edges=64, edges_grouped=True)
    assert ig.reason() is None and ig.reason(mk(**meta)) is None
    assert ig.reason(mk(max_nodes=224, max_edges=1024, edges_grouped=True)) is None
    limit = ("model / graph shape outside the one-launch integrated gradients kernel (embedding_dim 64, <= 64 node features, <= 4 conv "
             "layers, readout depth <= 4, <= 8 classes, graphs of <= 224 nodes and <= 1024 directed edges)")
    assert ig.reason(mk(max_nodes=225, max_edges=64, edges_grouped=True)) == limit
    assert ig.reason(mk(max_nodes=30, max_edges=1025, edges_grouped=True)) == limit
    assert ig.reason(mk()) == "batch lacks collate metadata (max_nodes / max_edges / grouped edges)"
    assert ig.reason(mk(F=32, **meta)) == "batch has 32 node features, the model takes 25"
    assert ig.reason(NS(x=NS(is_cuda=False, shape=(4, 25)), edge_index=NS(shape=(2, 0)), num_graphs=1, **meta)) == "the batch is on the CPU"
    for kw in (dict(embedding_dim=128), dict(n_convolutions=5), dict(n_classes=9)):
        assert IntegratedGradients(H.make_network("GCN", H.default_options(**kw), 25)).reason() == limit, kw
    assert IntegratedGradients(H.make_network("GCN", H.default_options(use_fused=False), 25)).reason() == "fused kernels disabled on the model"
    assert ig.lds_bytes(mk(max_nodes=224, max_edges=1024, edges_grouped=True)) <= 160 * 1024
    assert ig.lds_bytes(mk(max_nodes=225, max_edges=64, edges_grouped=True)) is None


def test_default_split_keeps_a_launch_near_a_second():
    from hcatgnet_amd import attribution as A
    from hcatgnet_amd import shapley
    f = IntegratedGradients.default_steps_per_launch
    assert f(50, 52) == 50 and f(50, 535) == 50 and f(50, 4096) == 50 and f(1, 10 ** 6) == 1
    big = 256 * 1000                                                  # 1000 rounds of workgroups
    per = f(50, big)
    assert 1 <= per < 50 and per * 1000 * A.STEP_SECONDS <= shapley.LAUNCH_SECONDS < (per + 1) * 1000 * A.STEP_SECONDS


# ------------------------------------------------------------------------------------------------ the library
def _args(F=25, D=64, nodes=184, edges=390, n_conv=2, R_=2, C=1, N=None, B=1, query=True):
    a = _lib.ExplainArgs()
    a.mode, a.flags = _lib.HCG_EXPLAIN_INTEGRATED, (_lib.HCG_EXPLAIN_QUERY if query else 0)
    a.F, a.D, a.C, a.n_conv, a.R = F, D, C, n_conv, R_
    a.max_nodes, a.max_edges = nodes, edges
    a.N, a.E, a.B = nodes if N is None else N, edges, B
    return a


def _call(a):
    return _lib.load().hcg_explain(ctypes.addressof(a), None), int(a.workspace_bytes_needed), int(a.lds_bytes)


def test_integrated_query_without_a_gpu():
    OK, INVALID, UNSUPPORTED = 0, -1, _lib.HCG_ERR_UNSUPPORTED
    assert _lib.HCG_EXPLAIN_INTEGRATED == 5
    rc, ws, lds = _call(_args())
    assert rc == OK and ws >= 2 * 2 * 184 * 64 * 4 and 0 < lds <= 160 * 1024
    rc, ws, lds = _call(_args(F=64, nodes=224, edges=1024, n_conv=4, R_=4, C=8))
    print(f"\n    HCG_EXPLAIN_INTEGRATED at the limit: workspace {ws} bytes, LDS {lds} bytes")
    assert rc == OK and ws >= 2 * 4 * 224 * 64 * 4 and lds <= 160 * 1024
    # the tiles and lists of HCG_EXPLAIN_GRAPHS, nothing more
    assert lds == 2 * 224 * 68 * 4 + 4 * 1024 * 4 + 2 * 228 * 4 + 3 * 224 * 4 + 8 * 128 * 4 + 2 * 256 * 4
    assert _call(_args(nodes=120, edges=250, N=535 * 120, B=535))[0] == OK
    for kw in (dict(D=128), dict(F=65), dict(nodes=225), dict(edges=1025), dict(C=9), dict(R_=5), dict(n_conv=5), dict(F=0)):
        assert _call(_args(**kw))[0] == UNSUPPORTED, kw
    # flags and pointers that belong to the other modes
    dummy = ctypes.c_int64(0)
    ptr = ctypes.addressof(dummy)                                     # (never read: the checks look at NULL / not NULL)
    for flag in (_lib.HCG_EXPLAIN_SIGMOID, _lib.HCG_EXPLAIN_TARGET_CLASS):
        a = _args()
        a.flags |= flag
        assert _call(a)[0] == INVALID, flag
    for name in ("target", "dout", "edge_mask", "node_mask", "dx"):
        a = _args()
        setattr(a, name, ptr)
        assert _call(a)[0] == INVALID, name
    # a launch: the step range and the class index.  With B = 0 a call that passes them has nothing to do and returns OK
    # before any pointer is looked at; with B = 1 it stops at the NULL pointers.  Nothing is launched either way.
    good = dict(path_steps=4, path_step_first=0, path_step_count=4, path_class_index=2)

    def launch(B, **kw):
        a = _args(query=False, C=3, B=B, N=0 if B == 0 else None)
        for k, v in dict(good, **kw).items():
            setattr(a, k, v)
        return _call(a)[0]

    assert launch(0) == OK and launch(0, path_step_first=1, path_step_count=3) == OK and launch(0, path_steps=1, path_step_count=1) == OK
    for bad in (dict(path_steps=0, path_step_count=0), dict(path_step_first=-1), dict(path_step_first=2, path_step_count=3),
                dict(path_step_count=5), dict(path_step_count=-1), dict(path_class_index=-1), dict(path_class_index=3)):
        assert launch(0, **bad) == INVALID, bad
    assert launch(1) == INVALID


def test_explain_args_mirror_matches_the_header():
    """sizeof(hcg_explain_args) as a C compiler sees the header = the ctypes mirror = what the library was built with; the
    path_ members sit where the mirror's overlay attributes put them, inside the block they share with the fit_ members."""
    cc = next((p for p in (shutil.which(n) for n in ("cc", "gcc", "clang", "c++", "g++", "hipcc")) if p), None)
    if cc is None:
        cc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    names = [n for n, _ in _lib.PATH_FIELDS]
    assert names == ["path_alpha", "path_weight", "path_node_attr", "path_edge_attr", "path_out_full", "path_out_base", "path_steps",
                     "path_step_first", "path_step_count", "path_class_index"]
    prints = "".join(f' printf(" %zu", offsetof(hcg_explain_args, {n}));' for n in names + ["fit_edge_logit"])
    with tempfile.TemporaryDirectory() as d:
        src, exe = os.path.join(d, "s.c"), os.path.join(d, "s")
        open(src, "w").write('#include <stdio.h>\n#include <stddef.h>\n#include "hcatgnet_hip.h"\nint main(void) { '
                             'printf("%zu %d", sizeof(hcg_explain_args), HCG_EXPLAIN_INTEGRATED);' + prints + ' return 0; }\n')
        subprocess.run([cc, "-I", os.path.join(REPO, "include"), src, "-o", exe], check=True, capture_output=True)
        got = [int(v) for v in subprocess.run([exe], check=True, capture_output=True, text=True).stdout.split()]
    size, mode, offsets = got[0], got[1], got[2:]
    print(f"\n    sizeof(hcg_explain_args) = {size}; path_ offsets {offsets[:-1]}")
    A = _lib.ExplainArgs
    assert ctypes.sizeof(A) == size == _lib.load().hcg_struct_bytes(_lib.HCG_STRUCT_EXPLAIN_ARGS)
    assert mode == _lib.HCG_EXPLAIN_INTEGRATED
    assert [getattr(A, n).offset for n in names] == offsets[:-1]
    assert offsets[0] == offsets[-1] == A.fit_edge_logit.offset and offsets[-2] + 4 <= size
    # the overlay reads and writes the bytes of the block
    a = A()
    a.path_alpha, a.path_steps, a.path_class_index = 0x1234, 7, 3
    assert a.fit_edge_logit == 0x1234 and a.path_alpha == 0x1234 and a.path_steps == 7 and a.path_class_index == 3
    a.path_alpha = None
    assert a.fit_edge_logit is None and a.path_alpha is None
