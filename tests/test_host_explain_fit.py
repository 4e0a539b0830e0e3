"""Host side of `hcatgnet_amd.explain.ExplainFit` (no GPU): the loop path on CPU tensors against the fp64 reference with the
checks the GPU tests apply to the kernel (tests/explain_fit_ref.py states reference, inputs and checks), its exact split
invariance, the default target, the initialisation, validation, `reason`, and the library's HCG_EXPLAIN_FIT query and
argument block.  Every figure is printed before it is asserted (`pytest -s`)."""
import ctypes
import math
import os
import shutil
import subprocess
import sys

import pytest
import torch

import hcatgnet_amd as H
from hcatgnet_amd import _lib
from hcatgnet_amd.explain import ExplainFit, ExplainFitState
from tests import explain_fit_ref as R

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module", autouse=True)
def built():
    if not os.path.isfile(_lib.LIB_PATH):
        import __graft_entry__
        __graft_entry__.build()


def _model(c, **opt):
    from oracle import gcn_oracle as O
    n_conv, n_read = O.infer_depths(c.params)
    o = H.default_options(n_convolutions=n_conv, readout_layers=n_read, embedding_dim=64,
                          n_classes=c.params[f"readout.{n_read - 1}.weight"].shape[0], **opt)
    m = H.make_network("GCN", o, c.x.shape[1])
    m.load_state_dict(c.params)
    return m


def _batch(c, **kw):
    meta = dict(max_nodes=c.max_nodes, max_edges=c.max_edges, edges_grouped=True)
    meta.update(kw)
    return H.Batch(c.x, c.ei, c.batch, c.B, **meta)


def _run(fit, b, c, s_in, epochs, **kw):
    st = R.to_fit_state(s_in, c.batch, c.ei, c.B, "cpu")
    r = fit(b, target=c.target, state=st, epochs=epochs, **kw)
    assert r.state is st and fit.last_path == "loop"
    return dict(state=R.from_fit_state(st), out=r.out.clone(), loss=r.loss_history[-1].clone(), loss_history=r.loss_history.clone(),
                edge_mask=r.edge_mask.clone(), node_mask=r.node_mask.clone())


# ------------------------------------------------------------------------------------------------ the loop path on CPU tensors
@pytest.mark.parametrize("name", ["onehot25", "deep", "dense64", "edge-cases", "limit"])
def test_loop_path_one_epoch_from_a_given_state(name):
    """GPU test 1 (and 4) on the loop path: the fresh state and the reference's state after c.warm epochs."""
    c = R.case(name)
    fit, b = ExplainFit(_model(c)), _batch(c)
    assert fit.reason(b) == "the batch is on the CPU"
    states, _, _ = R.reference(c, c.warm)
    assert torch.equal(states[-1]["n_hard"], c.x != 0) and torch.equal(states[-1]["e_hard"], c.ei[0] != c.ei[1])
    for s_in in (R.rounded(states[0]), R.rounded(states[c.warm])):
        got = _run(fit, b, c, s_in, 1)
        R.check_one_epoch(c, s_in, got, name + " (loop, CPU)")
        if name == "edge-cases":
            g = got["state"]
            assert not bool(g["e_hard"][c.self_loop]) and float(got["edge_mask"][c.self_loop]) == 0.0
            assert float(g["e"][c.self_loop]) == float(s_in["e"][c.self_loop])
            assert not bool(g["n_hard"][c.batch == 1].any()) and g["hard_count"][1, 1] == 0 and g["hard_count"][0, 0] == 0


@pytest.mark.parametrize("name", ["onehot25", "deep"])
def test_loop_path_whole_fit(name):
    """GPU test 3 on the loop path: 30 epochs."""
    c = R.case(name)
    fit, b = ExplainFit(_model(c)), _batch(c)
    got = _run(fit, b, c, R.rounded(R.reference(c, 0)[0][0]), 30)
    R.check_whole_fit(c, 30, got, name + " (loop, CPU)")


def test_loop_path_split_is_exact():
    c = R.case("onehot25")
    fit, b = ExplainFit(_model(c)), _batch(c)
    s0 = R.rounded(R.reference(c, 0)[0][0])
    one = _run(fit, b, c, s0, 12)
    st = R.to_fit_state(s0, c.batch, c.ei, c.B, "cpu")
    h = []
    for n in (5, 7):
        r = fit(b, target=c.target, state=st, epochs=n)
        h.append(r.loss_history.clone())
    assert st.step == 12 and torch.equal(torch.cat(h), one["loss_history"])
    two = R.from_fit_state(st)
    for k, v in one["state"].items():
        assert torch.equal(v, two[k]) if torch.is_tensor(v) else v == two[k], k
    assert torch.equal(r.edge_mask, one["edge_mask"]) and torch.equal(r.node_mask, one["node_mask"]) and torch.equal(r.out, one["out"])


def test_default_target_is_the_models_own_prediction():
    c = R.case("deep")
    fit, b = ExplainFit(_model(c), epochs=2), _batch(c)
    want = R.model_prediction(c.params, c.x, c.ei, c.batch, c.B)
    got = fit._target(b, None)
    err = float((got.double() - want).abs().max()) / max(float(want.abs().max()), 1.0)
    print(f"\n    default target vs the fp64 model: {err:.2e}")
    assert tuple(got.shape) == (c.B, 2) and err <= R.TOL
    a = fit(b, generator=torch.Generator().manual_seed(9))
    first = [t.clone() for t in (a.edge_mask, a.node_mask, a.out, a.loss_history)]
    z = fit(b, target=got, generator=torch.Generator().manual_seed(9))
    for p, q in zip(first, (z.edge_mask, z.node_mask, z.out, z.loss_history)):
        assert torch.equal(p, q)
    assert a.state.step == 2 and tuple(a.loss_history.shape) == (2, c.B)


def test_initialisation():
    """n = 0.1 randn(N, F) first, then e = randn(E) * std_g with std_g = sqrt(2) sqrt(2 / (2 N_g)); moments, flags and counts
    zero; step 0."""
    from hcatgnet_amd import synth
    sb = synth.make_batch(num_graphs=40, nodes=60, nodes_jitter=40, extra_bonds=4, max_degree=4, feat=25)
    b = sb.as_batch()
    fit = ExplainFit(H.make_network("GCN", H.default_options(), 25))
    s = fit.init_state(b, torch.Generator().manual_seed(4))
    r = R.init_state(sb.x, sb.edge_index, sb.batch, sb.num_graphs, torch.Generator().manual_seed(4))
    assert torch.equal(s.edge_logit, r["e"]) and torch.equal(s.node_logit, r["n"])
    gen = torch.Generator().manual_seed(4)
    torch.randn(sb.x.shape, generator=gen)
    z = torch.randn(sb.edge_index.shape[1], generator=gen)
    eg = sb.batch[sb.edge_index[1]]
    nodes = torch.bincount(sb.batch, minlength=sb.num_graphs)
    assert int(nodes.min()) < int(nodes.max())
    for g in range(sb.num_graphs):
        std = math.sqrt(2.0) * math.sqrt(2.0 / (2.0 * int(nodes[g])))
        ratio = s.edge_logit[eg == g] / z[eg == g]
        assert float((ratio - std).abs().max()) <= 1e-6 * std, g
    print(f"\n    node logits: std {float(s.node_logit.std()):.4f} (0.1 asked)")
    assert abs(float(s.node_logit.std()) - 0.1) < 2e-3
    assert s.step == 0 and not bool(s.edge_hard.any()) and not bool(s.node_hard.any()) and int(s.hard_count.abs().sum()) == 0
    for t in (s.edge_exp_avg, s.edge_exp_avg_sq, s.node_exp_avg, s.node_exp_avg_sq):
        assert float(t.abs().max()) == 0.0
    assert s.edge_hard.dtype == torch.bool and s.hard_count.dtype == torch.int32 and tuple(s.hard_count.shape) == (40, 2)


def test_validation_errors():
    c = R.case("deep")
    m, b = _model(c), _batch(c)
    with pytest.raises(ValueError):
        ExplainFit(m, epochs=0)
    with pytest.raises(ValueError):
        ExplainFit(m, coeffs=dict(edge_sise=1.0))
    fit = ExplainFit(m, epochs=2)
    with pytest.raises(ValueError):
        fit(b, epochs=0)
    with pytest.raises(ValueError, match="epochs_per_launch"):
        fit(b, epochs_per_launch=0)                                   # (checked before the path is chosen)
    good = fit.init_state(b, torch.Generator().manual_seed(1))
    for name, bad in (("edge_logit", good.edge_logit.double()), ("edge_logit", good.edge_logit[:-1]),
                      ("node_hard", good.node_hard.to(torch.uint8)), ("node_exp_avg", good.node_exp_avg.t()),
                      ("hard_count", good.hard_count.long()), ("hard_count", good.hard_count[:-1])):
        s = good.clone()
        setattr(s, name, bad)
        with pytest.raises(ValueError, match=name):
            fit(b, state=s)
    with pytest.raises(ValueError):
        fit(b, state=dict(edge_logit=good.edge_logit))
    with pytest.raises(ValueError):
        fit(b, target=torch.zeros(c.B, 5))
    other = R.case("onehot25")                                        # a state from another batch shape
    with pytest.raises(ValueError, match="for this batch"):
        ExplainFit(_model(other))(_batch(other), state=good)
    assert isinstance(good, ExplainFitState) and good.step == 0


def test_reason_strings():
    """`reason` decides on the host: the limits are ExplainStep's (224 nodes, 1024 directed edges)."""
    from types import SimpleNamespace as NS

    def mk(F=25, **kw):
        return NS(x=NS(is_cuda=True, shape=(4, F)), edge_index=NS(shape=(2, 0)), num_graphs=1, **kw)

    fit = ExplainFit(H.make_network("GCN", H.default_options(), 25))
    meta = dict(max_nodes=30, max_edges=64, edges_grouped=True)
    assert fit.reason() is None and fit.reason(mk(**meta)) is None
    assert fit.reason(mk(max_nodes=224, max_edges=1024, edges_grouped=True)) is None
    limit = ("model / graph shape outside the one-launch explainer fit kernel (embedding_dim 64, <= 64 node features, <= 4 conv "
             "layers, readout depth <= 4, <= 8 classes, graphs of <= 224 nodes and <= 1024 directed edges)")
    assert fit.reason(mk(max_nodes=225, max_edges=64, edges_grouped=True)) == limit
    assert fit.reason(mk(max_nodes=30, max_edges=1025, edges_grouped=True)) == limit
    assert fit.reason(mk()) == "batch lacks collate metadata (max_nodes / max_edges / grouped edges)"
    assert fit.reason(mk(F=32, **meta)) == "batch has 32 node features, the model takes 25"
    assert fit.reason(NS(x=NS(is_cuda=False, shape=(4, 25)), edge_index=NS(shape=(2, 0)), num_graphs=1, **meta)) == "the batch is on the CPU"
    for kw in (dict(embedding_dim=128), dict(n_convolutions=5), dict(n_classes=9)):
        assert ExplainFit(H.make_network("GCN", H.default_options(**kw), 25)).reason() == limit, kw
    assert ExplainFit(H.make_network("GCN", H.default_options(use_fused=False), 25)).reason() == "fused kernels disabled on the model"
    assert fit.last_path is None


# ------------------------------------------------------------------------------------------------ the library
def _query(F=25, D=64, nodes=184, edges=390, n_conv=2, R_=2, C=1, N=None, B=1):
    a = _lib.ExplainArgs()
    a.mode, a.flags = _lib.HCG_EXPLAIN_FIT, _lib.HCG_EXPLAIN_QUERY
    a.F, a.D, a.C, a.n_conv, a.R = F, D, C, n_conv, R_
    a.max_nodes, a.max_edges = nodes, edges
    a.N, a.E, a.B = nodes if N is None else N, edges, B
    rc = _lib.load().hcg_explain(ctypes.addressof(a), None)
    return rc, int(a.workspace_bytes_needed), int(a.lds_bytes)


def test_fit_query_without_a_gpu():
    assert _lib.HCG_EXPLAIN_FIT == 4
    rc, ws, lds = _query()
    assert rc == 0 and ws >= 2 * 2 * 184 * 64 * 4 and 0 < lds <= 163840
    rc, ws, lds = _query(F=64, nodes=224, edges=1024, n_conv=4, R_=4, C=8)
    print(f"\n    HCG_EXPLAIN_FIT at the limit: workspace {ws} bytes, LDS {lds} bytes")
    assert rc == 0 and ws >= 2 * 4 * 224 * 64 * 4 and lds <= 163840
    # the same tiles and lists as HCG_EXPLAIN_GRAPHS, plus the two hard counts
    assert lds == 2 * 224 * 68 * 4 + 4 * 1024 * 4 + 2 * 228 * 4 + 3 * 224 * 4 + 8 * 128 * 4 + 2 * 256 * 4 + 16
    assert _query(nodes=120, edges=250, N=535 * 120, B=535)[0] == 0
    for n_conv in (1, 2, 3, 4):
        for R_ in (1, 2, 3, 4):
            assert _query(n_conv=n_conv, R_=R_)[0] == 0
    for kw in (dict(D=128), dict(F=65), dict(nodes=225), dict(edges=1025), dict(C=9), dict(R_=5), dict(n_conv=5), dict(F=0)):
        assert _query(**kw)[0] == -3, kw
    # a launch needs at least one epoch and a step count that is not negative; the masks of the other modes stay NULL
    a = _lib.ExplainArgs()
    a.mode, a.F, a.D, a.C, a.n_conv, a.R, a.B = _lib.HCG_EXPLAIN_FIT, 25, 64, 1, 2, 2, 1
    lib = _lib.load()
    assert lib.hcg_explain(ctypes.addressof(a), None) == -1
    a.epoch_count, a.step_first = 1, -1
    assert lib.hcg_explain(ctypes.addressof(a), None) == -1


def test_explain_args_mirror_matches_the_header():
    """sizeof(hcg_explain_args) as a C compiler sees the header = the ctypes mirror = what the library was built with."""
    cc = next((p for p in (shutil.which(n) for n in ("cc", "gcc", "clang", "c++", "g++", "hipcc")) if p), None)
    if cc is None:
        cc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    import tempfile
    with tempfile.TemporaryDirectory() as d:
        src, exe = os.path.join(d, "s.c"), os.path.join(d, "s")
        open(src, "w").write('#include <stdio.h>\n#include "hcatgnet_hip.h"\nint main(void) { printf("%zu", sizeof(hcg_explain_args)); return 0; }\n')
        subprocess.run([cc, "-I", os.path.join(REPO, "include"), src, "-o", exe], check=True, capture_output=True)
        size = int(subprocess.run([exe], check=True, capture_output=True, text=True).stdout)
    print(f"\n    sizeof(hcg_explain_args) = {size}")
    assert ctypes.sizeof(_lib.ExplainArgs) == size == _lib.load().hcg_struct_bytes(_lib.HCG_STRUCT_EXPLAIN_ARGS)
    names = [f[0] for f in _lib.ExplainArgs._fields_]
    assert names[names.index("reserved") + 1] == "fit_edge_logit" and names[-1] == "fit_coeffs"
