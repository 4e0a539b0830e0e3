"""Host side of Shapley value sampling (no GPU): the HCG_EXPLAIN_SHAPLEY query of hcg_explain, `draw_permutations`, and
`ShapleySampling`'s batch-synchronous loop on CPU tensors against the fp64 oracle (tests/shapley_ref.py states the
reference and the bounds)."""
import ctypes
import os

import pytest
import torch

import hcatgnet_amd as H
from hcatgnet_amd import _lib, synth
from tests import shapley_ref as SR


@pytest.fixture(scope="module", autouse=True)
def built():
    if not os.path.isfile(_lib.LIB_PATH):
        import __graft_entry__
        __graft_entry__.build()


def _query(F=25, D=64, nodes=184, edges=390, n_conv=2, R=2, C=1, N=None, B=1, perm_count=1, **ptrs):
    a = _lib.ExplainArgs()
    a.mode, a.flags = _lib.HCG_EXPLAIN_SHAPLEY, _lib.HCG_EXPLAIN_QUERY
    a.F, a.D, a.C, a.n_conv, a.R = F, D, C, n_conv, R
    a.max_nodes, a.max_edges = nodes, edges
    a.N, a.E, a.B = nodes if N is None else N, edges, B
    a.perm_count = perm_count
    for k, v in ptrs.items():
        setattr(a, k, v)
    rc = _lib.load().hcg_explain(ctypes.addressof(a), None)
    return rc, int(a.workspace_bytes_needed)


def test_args_mirror_and_mode_number():
    assert ctypes.sizeof(_lib.ExplainArgs) == _lib.load().hcg_struct_bytes(_lib.HCG_STRUCT_EXPLAIN_ARGS)
    assert _lib.HCG_EXPLAIN_SHAPLEY == 3
    hdr = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "hcatgnet_hip.h")).read()
    assert "#define HCG_EXPLAIN_SHAPLEY 3" in hdr


def test_query_accepts_the_reference_regime_and_reports_a_workspace():
    """One row of N F + E floats per permutation of the launch; nothing is launched (this machine may have no GPU)."""
    for F in (25, 32):
        for n_conv in (1, 2, 3, 4):
            for R in (1, 2, 3, 4):
                rc, ws = _query(F=F, n_conv=n_conv, R=R)
                assert rc == 0 and ws >= (184 * F + 390) * 4, (F, n_conv, R)
    rc, ws = _query(perm_count=5)
    assert rc == 0 and ws >= 5 * (184 * 25 + 390) * 4
    rc, ws = _query(nodes=120, edges=250, N=535 * 120, B=535, perm_count=2)
    assert rc == 0 and ws >= 2 * (535 * 120 * 25 + 250) * 4
    # up to the explain limits where LDS allows: F = 64, 8 classes, 1024 edges at this mode's 184 nodes
    assert _query(F=64, nodes=184, edges=1024, n_conv=4, R=4, C=8)[0] == 0


def test_query_reports_the_kernels_lds_bytes():
    """The LDS figure of the bench record comes from the library, not from a copy of its formula: three [npad][68] f32
    tiles, 8 bytes per edge and the structure; the documented limit is the largest shape that fits 160 KB."""
    def lds(nodes, edges):
        a = _lib.ExplainArgs()
        a.mode, a.flags = _lib.HCG_EXPLAIN_SHAPLEY, _lib.HCG_EXPLAIN_QUERY
        a.F, a.D, a.C, a.n_conv, a.R, a.max_nodes, a.max_edges = 25, 64, 1, 2, 2, nodes, edges
        assert _lib.load().hcg_explain(ctypes.addressof(a), None) == 0
        return int(a.lds_bytes)
    top = lds(184, 1024)
    assert 160 * 1024 - 816 < top <= 160 * 1024          # one more row of the three tiles would not fit
    assert lds(184, 1024) - lds(184, 1020) == 4 * 8 and lds(184, 390) - lds(180, 390) == 4 * (3 * 68 * 4 + 12)
    assert lds(8, 16) == lds(16, 16)                      # (the tiles are never smaller than 16 rows)
    from hcatgnet_amd.shapley import ShapleySampling
    x = torch.zeros(4, 25); ei = torch.zeros(2, 0, dtype=torch.int64); bv = torch.zeros(4, dtype=torch.int64)
    sv = ShapleySampling(H.make_network("GCN", H.default_options(), 25))
    assert sv.lds_bytes(H.Batch(x, ei, bv, 1, max_nodes=184, max_edges=390, edges_grouped=True)) is None    # CPU tensors: the loop


def test_query_refuses_outside_the_documented_limits():
    for kw in (dict(D=128), dict(F=65), dict(nodes=185), dict(nodes=224), dict(edges=1025), dict(C=9), dict(R=5), dict(n_conv=5),
               dict(F=0), dict(C=0), dict(n_conv=0), dict(R=0), dict(perm_count=65536)):
        assert _query(**kw)[0] == -3, kw


def test_mask_target_and_dout_pointers_must_be_null():
    for name in ("edge_mask", "node_mask", "target", "dout"):
        assert _query(**{name: 4096})[0] == -1, name


# ------------------------------------------------------------------------------------------------ permutations
def _small_case(seed=5):
    """6 graphs of 8-14 nodes, F = 6 with about half the entries exactly 0, one explicit self-loop edge, 2 classes."""
    sb = synth.make_batch(num_graphs=6, nodes=11, extra_bonds=2, max_degree=4, feat=6, nodes_jitter=3)
    gen = torch.Generator().manual_seed(seed)
    x = sb.x * (torch.rand(sb.x.shape, generator=gen) < 0.5)
    eg = sb.batch[sb.edge_index[1]]
    pos = int((eg <= 2).sum()) - 2                              # inside graph 2's edge block
    node = int(sb.edge_index[0, pos])
    ei = torch.cat([sb.edge_index[:, :pos], torch.tensor([[node], [node]]), sb.edge_index[:, pos:]], 1).contiguous()
    params = SR.rand_params(6, 64, n_conv=2, n_read=2, n_classes=2, seed=23)
    return x.contiguous(), ei, sb.batch, sb.num_graphs, sb.max_nodes, sb.max_edges + 1, params


def test_draw_permutations_layout_and_seed():
    from hcatgnet_amd.shapley import draw_permutations
    x, ei, bv, B, mn, me, _ = _small_case()
    b = H.Batch(x, ei, bv, B, max_nodes=mn, max_edges=me, edges_grouped=True)
    nptr, eptr = SR.pointers(bv, ei, B)
    p1 = draw_permutations(b, 6, 4, torch.Generator().manual_seed(3))
    assert tuple(p1.shape) == (4, x.shape[0] * 6 + ei.shape[1])
    SR.check_permutations(p1, nptr, eptr, 6)
    p2 = draw_permutations(b, 6, 4, torch.Generator().manual_seed(3))
    assert torch.equal(p1, p2)
    p3 = draw_permutations(b, 6, 4, torch.Generator().manual_seed(4))
    assert not torch.equal(p1, p3)
    assert not torch.equal(p1[0], p1[1])


def test_exports():
    assert H.ShapleySampling is not None and H.draw_permutations is not None
    assert "ShapleySampling" in H.__all__ and "draw_permutations" in H.__all__


# ------------------------------------------------------------------------------------------------ the loop on CPU tensors
def test_cpu_tensors_take_the_loop_and_match_the_fp64_reference():
    from hcatgnet_amd.shapley import ShapleySampling, draw_permutations
    x, ei, bv, B, mn, me, params = _small_case()
    print(f"\n  small case: B {B} N {x.shape[0]} E {ei.shape[1]} zero entries {int((x == 0).sum())} of {x.numel()}")
    assert 0.3 < float((x == 0).float().mean()) < 0.7
    model = SR.model_from_params(H, params)
    sv = ShapleySampling(model)
    b = H.Batch(x, ei, bv, B, max_nodes=mn, max_edges=me, edges_grouped=True)
    assert "CPU" in sv.reason(b)
    perm = draw_permutations(b, 6, 3, torch.Generator().manual_seed(11))
    r = sv(b, permutations=perm, class_index=1)
    assert sv.last_path == "loop"
    assert tuple(r.node_attr.shape) == tuple(x.shape) and tuple(r.edge_attr.shape) == (ei.shape[1],)
    assert tuple(r.out_full.shape) == (B, 2) and tuple(r.out_base.shape) == (B, 2)
    refs = SR.reference_batch(params, x, ei, bv, B, perm, 1)
    SR.check_against_reference(r, refs, x, ei, bv, B, 1, "loop on CPU tensors")
    nz, nl = SR.check_exact_zeros(r, x, ei)
    assert nz > 0 and nl == 1
    assert int((r.edge_attr != 0).sum()) == ei.shape[1] - 1
    for q in model.parameters():
        assert q.grad is None
    for mod in model.modules():
        if isinstance(mod, H.GCNConv):
            assert mod.explain is False and mod._edge_mask is None

    # a single-graph batch gives the same values for that graph
    nptr, eptr = SR.pointers(bv, ei, B)
    g = 2
    a, e, ea, eb = int(nptr[g]), int(nptr[g + 1]), int(eptr[g]), int(eptr[g + 1])
    s, K = a * 6 + ea, (e - a) * 6 + (eb - ea)
    one = H.Batch(x[a:e].contiguous(), (ei[:, ea:eb] - a).contiguous(), torch.zeros(e - a, dtype=torch.long), 1,
                  max_nodes=e - a, max_edges=eb - ea, edges_grouped=True)
    r1 = ShapleySampling(model)(one, permutations=perm[:, s:s + K].contiguous(), class_index=1)
    SR.check_against_reference(r1, [refs[g]], one.x, one.edge_index, one.batch, 1, 1, "graph 2 alone")
    d = max(float((r1.node_attr - r.node_attr[a:e]).abs().max()), float((r1.edge_attr - r.edge_attr[ea:eb]).abs().max()))
    print(f"    graph 2 alone vs in the batch: max abs difference {d:.2e} (bound {2 * SR.TOL * max(1.0, refs[g]['vmax']):.2e})")
    assert d <= 2 * SR.TOL * max(1.0, refs[g]["vmax"])


def test_permutation_tensor_is_validated_on_the_host():
    from hcatgnet_amd.shapley import ShapleySampling
    x, ei, bv, B, mn, me, params = _small_case()
    sv = ShapleySampling(SR.model_from_params(H, params))
    b = H.Batch(x, ei, bv, B, max_nodes=mn, max_edges=me, edges_grouped=True)
    row = x.shape[0] * 6 + ei.shape[1]
    for bad in (torch.zeros(2, row, dtype=torch.int64), torch.zeros(2, row + 1, dtype=torch.int32), torch.zeros(row, dtype=torch.int32)):
        with pytest.raises(ValueError):
            sv(b, permutations=bad)


def test_support_check_is_host_only():
    from hcatgnet_amd.shapley import ShapleySampling
    sv = ShapleySampling(H.make_network("GCN", H.default_options(), 25))
    assert sv.reason() is None and sv.last_path is None
    assert "shape" in ShapleySampling(H.make_network("GCN", H.default_options(embedding_dim=128), 25)).reason()
    assert "disabled" in ShapleySampling(H.make_network("GCN", H.default_options(use_fused=False), 25)).reason()
    for kw in (dict(n_convolutions=1, readout_layers=1), dict(n_convolutions=4, readout_layers=4, n_classes=8)):
        assert ShapleySampling(H.make_network("GCN", H.default_options(**kw), 32)).reason() is None, kw
    # real sizes (184 * 25 + 390 steps at most per workgroup): three workgroups per CU; the limit shapes: one
    assert ShapleySampling.default_samples_per_launch(25, 52, 100000, 184 * 25 + 390) == 14
    assert ShapleySampling.default_samples_per_launch(25, 52, 100000, 184 * 64 + 1024) == 4
    assert ShapleySampling.default_samples_per_launch(25, 535, 1300000, 184 * 25 + 390) == 1
    assert ShapleySampling.default_samples_per_launch(25, 1, 1 << 26, 100) == 1          # the workspace cap
    assert ShapleySampling.default_samples_per_launch(25, 2, 1000, 100) == 25
