"""Host side of the classification mode of `hcatgnet_amd.explain` (no GPU): `ExplainFit(mode="multiclass_classification")`
on CPU tensors -- the loop path -- against the fp64 reference of tests/explain_ce_ref.py with the checks and tolerances the
regression mode carries, the default target, an explicit off-argmax target, the argument errors, and the library's
class-index form (`HCG_EXPLAIN_TARGET_CLASS`): struct layout, query and refusals.  Every figure is printed before it is asserted (`pytest -s`)."""
import ctypes
import os

import pytest
import torch

import hcatgnet_amd as H
from hcatgnet_amd import _lib
from hcatgnet_amd.explain import ExplainFit, ExplainStep
from tests import explain_ce_ref as R

CE = "multiclass_classification"


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
@pytest.mark.parametrize("name", list(R.MAIN))
def test_loop_path_one_epoch_from_a_given_state(name):
    """The fresh state (step 0: no regulariser, discovers the hard masks) and the reference's state after 3 epochs."""
    c = R.case(name)
    fit, b = ExplainFit(_model(c), mode=CE), _batch(c)
    assert fit.mode == CE and fit.reason(b) == "the batch is on the CPU"
    states, _, _ = R.reference(c, c.warm)
    assert torch.equal(states[-1]["n_hard"], c.x != 0) and torch.equal(states[-1]["e_hard"], c.ei[0] != c.ei[1])
    for s_in in (R.rounded(states[0]), R.rounded(states[c.warm])):
        print(f"    {name}: fp32-vs-fp64 conditioning of the reference per graph: "
              + " ".join(f"{v:.1e}" for v in R.conditioning(c, s_in)))
        got = _run(fit, b, c, s_in, 1)
        R.check_one_epoch(c, s_in, got, name + " (loop, CPU)")


def test_loop_path_whole_fit():
    """12 epochs on the C = 3 case within the bound the reference gives itself."""
    c = R.case("c3x16")
    fit, b = ExplainFit(_model(c), mode=CE), _batch(c)
    got = _run(fit, b, c, R.rounded(R.reference(c, 0)[0][0]), 12)
    R.check_whole_fit(c, 12, got, "c3x16 (loop, CPU)")


def test_default_target_is_the_argmax_of_the_models_own_output():
    c = R.case("c8x16")
    fit, b = ExplainFit(_model(c), epochs=2, mode=CE), _batch(c)
    got = fit._target(b, None)
    assert got.dtype == torch.int64 and tuple(got.shape) == (c.B,) and torch.equal(got, c.target)
    a = fit(b, generator=torch.Generator().manual_seed(9))
    first = [t.clone() for t in (a.edge_mask, a.node_mask, a.out, a.loss_history)]
    z = fit(b, target=c.target, generator=torch.Generator().manual_seed(9))
    for p, q in zip(first, (z.edge_mask, z.node_mask, z.out, z.loss_history)):
        assert torch.equal(p, q)
    assert a.state.step == 2 and tuple(a.loss_history.shape) == (2, c.B)
    # a tie goes to the first maximal index, as torch.argmax has it: a model whose last layer is zero ties every class
    m = _model(c)
    with torch.no_grad():
        last = [q for q in m.readout][-1]
        last.weight.zero_(); last.bias.zero_()
    assert torch.equal(ExplainFit(m, mode=CE)._target(b, None), torch.zeros(c.B, dtype=torch.int64))


def test_an_explicit_target_off_the_argmax():
    """The 'phenomenon' form: the caller's labels, here one class off the argmax, through the same code."""
    c = R.off_argmax(R.case("c3x16"))
    assert not bool((c.target == c.prediction.argmax(1)).any())
    fit, b = ExplainFit(_model(c), mode=CE), _batch(c)
    states, _, _ = R.reference(c, c.warm)
    for s_in in (R.rounded(states[0]), R.rounded(states[c.warm])):
        got = _run(fit, b, c, s_in, 1)
        R.check_one_epoch(c, s_in, got, "c3x16, target off the argmax (loop, CPU)")


def test_argument_errors():
    c = R.case("c3")
    m, b = _model(c), _batch(c)
    assert ExplainFit(m).mode == "regression"
    with pytest.raises(ValueError, match="mode"):
        ExplainFit(m, mode="binary_classification")
    fit = ExplainFit(m, epochs=1, mode=CE)
    with pytest.raises(ValueError, match="int64"):
        fit(b, target=c.prediction.float())                           # a float target in classification mode
    with pytest.raises(ValueError, match="int64"):
        fit(b, target=c.target.to(torch.int32))
    with pytest.raises(ValueError, match="int64"):
        fit(b, target=c.target[:-1])
    with pytest.raises(ValueError, match="float32"):
        ExplainFit(m, epochs=1)(b, target=c.target)                   # an int target in regression mode
    for bad in (-1, c.C):                                             # out of range: checked on CPU tensors
        t = c.target.clone()
        t[1] = bad
        with pytest.raises(ValueError, match="outside"):
            fit(b, target=t)
    one = R.Case()
    one.__dict__.update(c.__dict__)
    from tests.test_gpu_explain import _rand_params
    one.params = _rand_params(c.x.shape[1], 64, seed=1, n_conv=2, n_read=2, n_classes=1)
    with pytest.raises(ValueError, match="two classes"):
        ExplainFit(_model(one), mode=CE)
    with pytest.raises(ValueError, match="two classes"):
        ExplainStep(_model(one))(b, torch.zeros(c.ei.shape[1]), target_class=torch.zeros(c.B, dtype=torch.int64))
    # ExplainStep: at most one upstream form; the class indices int64 [B]
    step = ExplainStep(m)
    em = torch.zeros(c.ei.shape[1])
    for kw in (dict(target=c.prediction.float(), target_class=c.target), dict(dout=c.prediction.float(), target_class=c.target),
               dict(target=c.prediction.float(), dout=c.prediction.float())):
        with pytest.raises(ValueError, match="at most one"):
            step(b, em, **kw)
    with pytest.raises(ValueError, match="int64"):
        step(b, em, target_class=c.target.float())
    with pytest.raises(ValueError, match="int64"):
        step(b, em, target_class=c.target[:-1])


# ------------------------------------------------------------------------------------------------ the library
# hcg_explain_args as it was before the class-index form existed (LP64), written down from that struct.  The form adds NO
# field: `target_class` shares the `target` slot (a union in the header) and HCG_EXPLAIN_TARGET_CLASS in `flags` says which
# of the two the slot holds -- tests/test_host_explain_fit.py pins `fit_coeffs` as the struct's last field and the mirror's
# size to the header's, so an appended field is not open to this interface.  Size and every offset stay what they were.
OFFSETS_BEFORE = dict(mode=0, flags=4, x=8, edge_index=16, graph_ptr=24, edge_ptr=32, edge_mask=40, node_mask=48, target=56, dout=64,
                      conv_W=72, conv_b=104, head_W=136, head_b=168, out=200, loss=208, d_edge_mask=216, d_node_mask=224, dx=232,
                      status=240, workspace=248, workspace_bytes=256, workspace_bytes_needed=264, N=272, E=280, B=288, F=296,
                      D=304, C=312, max_nodes=320, max_edges=328, n_conv=336, R=340, slope=344, apply_act=348, layer_dout=352,
                      layer_out=360, layer_h=368, rowptr=376, col=384, dinv=392, dew_csr=400, emb=408, n_models=416,
                      models_per_group=420, perm=424, out_base=432, shap_acc=440, n_perm=448, perm_first=452, perm_count=456,
                      class_index=460, lds_bytes=464, reserved=468, fit_edge_logit=472, fit_edge_exp_avg=480,
                      fit_edge_exp_avg_sq=488, fit_edge_hard=496, fit_node_logit=504, fit_node_exp_avg=512,
                      fit_node_exp_avg_sq=520, fit_node_hard=528, fit_hard_count=536, fit_loss_hist=544, fit_edge_mask_out=552,
                      fit_node_mask_out=560, step_first=568, epoch_count=572, fit_lr=576, fit_beta1=580, fit_beta2=584,
                      fit_eps=588, fit_coeffs=592)
SIZE_BEFORE = 608
FLAG = 4          # HCG_EXPLAIN_TARGET_CLASS


def test_the_class_index_form_moves_no_offset_and_adds_a_flag():
    A = _lib.ExplainArgs
    assert _lib.HCG_EXPLAIN_TARGET_CLASS == FLAG and FLAG not in (_lib.HCG_EXPLAIN_QUERY, _lib.HCG_EXPLAIN_SIGMOID)
    assert [f[0] for f in A._fields_] == list(OFFSETS_BEFORE)
    for k, off in OFFSETS_BEFORE.items():
        assert getattr(A, k).offset == off, k
    assert ctypes.sizeof(A) == SIZE_BEFORE == _lib.load().hcg_struct_bytes(_lib.HCG_STRUCT_EXPLAIN_ARGS)
    # the header: the two names of the slot sit at the same offset, the flag has the mirror's value, the size is unchanged
    import shutil
    import subprocess
    import tempfile
    cc = next((p for p in (shutil.which(n) for n in ("cc", "gcc", "clang", "c++", "g++", "hipcc")) if p), None)
    if cc is None:
        cc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    repo = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    with tempfile.TemporaryDirectory() as d:
        src, exe = os.path.join(d, "s.c"), os.path.join(d, "s")
        open(src, "w").write('#include <stdio.h>\n#include <stddef.h>\n#include "hcatgnet_hip.h"\nint main(void) { '
                             'printf("%zu %zu %zu %d", offsetof(hcg_explain_args, target), offsetof(hcg_explain_args, target_class), '
                             'sizeof(hcg_explain_args), HCG_EXPLAIN_TARGET_CLASS); return 0; }\n')
        subprocess.run([cc, "-I", os.path.join(repo, "include"), src, "-o", exe], check=True, capture_output=True)
        got = subprocess.run([exe], check=True, capture_output=True, text=True).stdout.split()
    assert [int(v) for v in got] == [OFFSETS_BEFORE["target"], OFFSETS_BEFORE["target"], SIZE_BEFORE, FLAG]


def _args(mode, C=3, query=True, ptr=None):
    """a block of the given mode; with `ptr`, every pointer a launch checks for NULL is set to it except the target slot, dout
    and the workspace, so a call that passes the checks of its arguments ends at HCG_ERR_WORKSPACE -- before anything is read
    or launched"""
    a = _lib.ExplainArgs()
    a.mode, a.flags = mode, (_lib.HCG_EXPLAIN_QUERY if query else 0)
    a.F, a.D, a.C, a.n_conv, a.R = 25, 64, C, 2, 2
    a.max_nodes, a.max_edges, a.N, a.E, a.B = 30, 64, 30, 64, 1
    a.n_models = a.models_per_group = a.perm_count = 1
    if ptr is not None:
        for k in ("x", "edge_index", "graph_ptr", "edge_ptr", "out", "status"):
            setattr(a, k, ptr)
        for slots in (a.conv_W, a.conv_b, a.head_W, a.head_b):
            for i in range(len(slots)):
                slots[i] = ptr
        if mode == _lib.HCG_EXPLAIN_FIT:
            a.epoch_count = 1
            for k, _ in _lib.ExplainArgs._fields_:
                if k.startswith("fit_") and k not in ("fit_lr", "fit_beta1", "fit_beta2", "fit_eps", "fit_coeffs"):
                    setattr(a, k, ptr)
        else:
            a.edge_mask = a.d_edge_mask = a.loss = ptr
    return a


def test_library_checks_of_the_class_index_form_without_a_gpu():
    """No launch is reached: every call is a query, is refused on its arguments, or stops at the missing workspace."""
    lib = _lib.load()
    dummy = ctypes.c_int64(0)
    ptr = ctypes.addressof(dummy)                                     # (never read: the checks look at NULL / not NULL)
    call = lambda a: lib.hcg_explain(ctypes.addressof(a), None)
    OK, INVALID, WORKSPACE, UNSUPPORTED = 0, -1, -2, _lib.HCG_ERR_UNSUPPORTED
    for mode in (_lib.HCG_EXPLAIN_GRAPHS, _lib.HCG_EXPLAIN_FIT):
        assert call(_args(mode)) == OK
        for C, want in ((3, OK), (2, OK), (8, OK), (1, UNSUPPORTED)):   # the query reports C >= 2
            a = _args(mode, C=C)
            a.flags |= FLAG
            assert call(a) == want, (mode, C)
        assert call(_args(mode, C=1)) == OK                           # without the flag C = 1 stays what it was
    for mode in (_lib.HCG_EXPLAIN_ENSEMBLE, _lib.HCG_EXPLAIN_SHAPLEY, _lib.HCG_EXPLAIN_LAYER_EDGE_GRAD):
        a = _args(mode)
        assert call(a) == OK
        a.flags |= FLAG
        assert call(a) == INVALID, mode
    # HCG_EXPLAIN_GRAPHS, a launch: at most one upstream form; the flag needs the slot; the loss is required with it
    G = _lib.HCG_EXPLAIN_GRAPHS
    for names, flag, want in ((("target",), 0, WORKSPACE), (("dout",), 0, WORKSPACE), (("target",), FLAG, WORKSPACE),
                              (("target", "dout"), 0, INVALID), (("target", "dout"), FLAG, INVALID), ((), FLAG, INVALID),
                              (("dout",), FLAG, INVALID)):
        a = _args(G, query=False, ptr=ptr)
        a.flags |= flag
        for k in names:
            setattr(a, k, ptr)
        assert call(a) == want, (names, flag)
    a = _args(G, query=False, ptr=ptr)
    a.flags, a.target, a.loss = FLAG, ptr, None
    assert call(a) == INVALID
    a = _args(G, C=1, query=False, ptr=ptr)
    a.flags, a.target = FLAG, ptr
    assert call(a) == UNSUPPORTED
    # HCG_EXPLAIN_FIT, a launch: the slot is required in either reading
    F = _lib.HCG_EXPLAIN_FIT
    for names, flag, want in ((("target",), 0, WORKSPACE), (("target",), FLAG, WORKSPACE), ((), 0, INVALID), ((), FLAG, INVALID)):
        a = _args(F, query=False, ptr=ptr)
        a.flags |= flag
        for k in names:
            setattr(a, k, ptr)
        assert call(a) == want, (names, flag)
