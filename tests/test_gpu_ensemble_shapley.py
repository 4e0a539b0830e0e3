"""GPU tests of `EnsembleShapley`, `EnsembleSubsetValues` and `EnsembleCurves`: the model axis of k_shapley_walk (both
instantiations) and k_subset_values (csrc/shapley.hip).

No new fp64-oracle comparison: entry [m] of every per-model array must be `torch.equal` to what the existing, tested
single-model classes return for `models[m]`, which carries their oracle parity (tests/test_gpu_shapley_groups.py,
tests/test_gpu_subsets.py) over to the ensemble.  The moments are held to the bound of tests/ensemble_attr_ref.py, the
areas to the bound of tests/subsets_ref.py.  Cases (the smallest at which the axis can go wrong):
    A  4 graphs of 16 - 20 nodes, F = 25, 2 conv / 2 readout / 1 class: fragments (4 groups), atoms, ungrouped
    B  4 conv / 4 readout / 8 classes, class_index 5: every layer's model stride differs
    C  one 30-node graph, every x entry non-zero, a group of 550 live members: two staging rounds read model m's first layer
    D  one graph at the 184-node limit, atoms as players, two models
Every figure is printed before it is asserted (`pytest -s`)."""
import functools

import pytest
import torch

from tests import ensemble_attr_ref as EA
from tests import ensemble_shapley_ref as ER
from tests import subsets_ref as UR
from tests import test_gpu_subsets as TS

pytestmark = pytest.mark.gpu
ROW_SEED, PERM_SEED, P = 11, 5, 3
SHAPE_LIMIT = 16


@pytest.fixture(scope="module")
def H():
    import hcatgnet_amd
    import __graft_entry__
    import os
    from hcatgnet_amd import _lib
    if not os.path.isfile(_lib.LIB_PATH):
        __graft_entry__.build()
    return hcatgnet_amd


@functools.lru_cache(maxsize=None)
def _case(name):
    """-> (case, depths, grouped)"""
    import hcatgnet_amd
    if name.startswith("A-"):
        c = TS._synth_case(dict(num_graphs=4, nodes=18, extra_bonds=2, max_degree=4, feat=25, nodes_jitter=2), 0.3, ER.TWO, 0, 4)
        sizes = torch.bincount(c.batch).tolist()
        assert all(16 <= n <= 20 for n in sizes) and len(set(sizes)) > 1, sizes
        if name == "A-atoms":
            c.ng = hcatgnet_amd.atom_groups(TS._host_batch(c))
        return c, ER.TWO, name != "A-flat"
    if name == "B":
        return TS._case("four-convs"), ER.DEEP, True
    if name == "C":
        return TS._case("dense30"), ER.TWO, True
    if name == "D":
        return TS._case("node-limit"), ER.TWO, True
    assert name == "mixed"
    return TS._case("mixed"), ER.TWO, True


@functools.lru_cache(maxsize=None)
def _models(name, M):
    import hcatgnet_amd
    c, depths, _ = _case(name)
    ms = ER.models(hcatgnet_amd, 25, M, depths, "cuda")
    assert all(torch.equal(ms[0].state_dict()[k].cpu(), v) for k, v in c.params.items())      # model 0: the case's own
    return ms


def _kw(name):
    c, _, grouped = _case(name)
    return TS._kw(c) if grouped else {}


def _G(name):
    c, _, _ = _case(name)
    return 9 if name == "mixed" else ER.group_total(c.ng, c.batch, c.B)


@functools.lru_cache(maxsize=None)
def _perm(name):
    import hcatgnet_amd as H
    c, _, grouped = _case(name)
    gb = TS._gpu_batch(H, c)
    gen = torch.Generator().manual_seed(PERM_SEED)
    if grouped:
        return dict(group_permutations=H.draw_group_permutations(gb, n_samples=P, generator=gen, **_kw(name)))
    return dict(permutations=H.draw_permutations(gb, 25, P, gen))


def _rows(name):
    return UR.random_rows(6, _G(name), ROW_SEED).cuda()


@functools.lru_cache(maxsize=None)
def _single_walk(name, m):
    """`ShapleySampling(models[m])` with the shared permutations, cloned: (attr [row], out_full, out_base)"""
    import hcatgnet_amd as H
    c, _, grouped = _case(name)
    r = H.ShapleySampling(_models(name, 5)[m])(TS._gpu_batch(H, c), class_index=c.cls, **_perm(name), **_kw(name))
    attr = r.group_attr if grouped else torch.cat([r.node_attr.reshape(-1), r.edge_attr])
    return attr.clone(), r.out_full.clone(), r.out_base.clone()


@functools.lru_cache(maxsize=None)
def _single_rows(name, m):
    """`SubsetValues(models[m])` on the shared rows, cloned: (values, out_full, out_base)"""
    import hcatgnet_amd as H
    c, _, _ = _case(name)
    r = H.SubsetValues(_models(name, 5)[m])(TS._gpu_batch(H, c), _rows(name), **_kw(name))
    return r.values.clone(), r.out_full.clone(), r.out_base.clone()


def _walk_fields(r):
    per = r.group_attr if hasattr(r, "group_attr") else torch.cat([r.node_attr.reshape(r.node_attr.shape[0], -1), r.edge_attr], 1)
    mom = (r.group_mean, r.group_std) if hasattr(r, "group_mean") else ()
    return [per, r.out_full, r.out_base, r.node_mean, r.node_std, r.edge_mean, r.edge_std, *mom]


def _clone(ts):
    return [t.clone() for t in ts]


def _same(a, b):
    return len(a) == len(b) and all(torch.equal(p, q) for p, q in zip(a, b))


# ------------------------------------------------------------------------------------------------ 1. per-model identity
IDENTITY = [(n, M) for n in ("A-frag", "A-atoms", "A-flat", "B", "C") for M in (1, 3, 5)] + [("D", 2)]


@pytest.mark.parametrize("name,M", IDENTITY)
def test_the_walk_of_model_m_is_bitwise_shapley_sampling(H, name, M):
    c, _, grouped = _case(name)
    gb = TS._gpu_batch(H, c)
    es = H.EnsembleShapley(_models(name, 5)[:M])
    assert es.reason(gb) is None
    r = es(gb, class_index=c.cls, per_model=True, **_perm(name), **_kw(name))
    assert es.last_path == "fused" and isinstance(r, H.EnsembleShapleyResult if grouped else H.EnsembleFeatureShapleyResult)
    torch.cuda.synchronize()
    assert int(gb._hcg_plan.status[0].item()) == 0
    per = _walk_fields(r)[0]
    assert tuple(r.out_full.shape) == tuple(r.out_base.shape) == (M, c.B, 8 if name == "B" else 1) and per.shape[0] == M
    for m in range(M):
        attr, full, base = _single_walk(name, m)
        assert torch.equal(per[m], attr) and torch.equal(r.out_full[m], full) and torch.equal(r.out_base[m], base), (name, M, m)
    a0, a1 = _single_walk(name, 0)[0], _single_walk(name, 1)[0]
    print(f"\n  {name} M {M}: {per.shape[1]} players, {int((a0 != 0).sum())} non-zero in model 0")
    assert not torch.equal(a0, a1) and int((a0 != 0).sum()) >= 2           # the yardstick is not compared with itself


@pytest.mark.parametrize("name,M", [(n, M) for n, M in IDENTITY if n != "A-flat"])
def test_the_rows_of_model_m_are_bitwise_subset_values(H, name, M):
    c, _, _ = _case(name)
    gb = TS._gpu_batch(H, c)
    ev = H.EnsembleSubsetValues(_models(name, 5)[:M])
    assert ev.reason(gb) is None
    r = ev(gb, _rows(name), per_model=True, **_kw(name))
    assert ev.last_path == "fused" and isinstance(r, H.EnsembleSubsetResult)
    torch.cuda.synchronize()
    assert int(gb._hcg_plan.status[0].item()) == 0
    assert tuple(r.values.shape) == (M, 6, c.B, 8 if name == "B" else 1) and tuple(r.mean.shape) == tuple(r.std.shape) == tuple(r.values.shape[1:])
    for m in range(M):
        values, full, base = _single_rows(name, m)
        assert torch.equal(r.values[m], values) and torch.equal(r.out_full[m], full) and torch.equal(r.out_base[m], base), (name, M, m)
        assert torch.equal(r.values[m, 0], base) and torch.equal(r.values[m, 1], full)     # rows 0 / 1: all off / all on
    assert not torch.equal(_single_rows(name, 0)[0], _single_rows(name, 1)[0])
    if name == "C":
        # group 0's 550 members span two staging rounds; row {1} alone filters inside both
        assert _G(name) == 2 and int((c.x[:22] != 0).sum()) == 550


# ------------------------------------------------------------------------------------------------ 2. splits are exact
def test_walk_splits_are_exact(H):
    name = "A-frag"
    c, _, _ = _case(name)
    gb = TS._gpu_batch(H, c)
    ms = _models(name, 5)
    es = H.EnsembleShapley(ms)
    call = lambda e, **kw: _walk_fields(e(gb, class_index=c.cls, per_model=True, **_perm(name), **_kw(name), **kw))      # noqa: E731
    want = _clone(call(es))
    assert int(want[0].unique().numel()) > 20
    for mpl in (1, 2, 5):
        for spl in (1, 2, P):
            assert _same(want, call(es, models_per_launch=mpl, samples_per_launch=spl)), (mpl, spl)
    assert _same(want, call(H.EnsembleShapley(ms), models_per_launch=2, samples_per_launch=2))      # a fresh instance
    # per_model=False: the same moments and outputs from one chunk's accumulators
    lean = es(gb, class_index=c.cls, models_per_launch=2, **_perm(name), **_kw(name))
    assert lean.group_attr is None and _same(want[1:], _walk_fields(lean._replace(group_attr=want[0]))[1:])
    # the first three models do not depend on the other two
    three = call(H.EnsembleShapley(ms[:3]))
    assert torch.equal(three[0], want[0][:3]) and torch.equal(three[1], want[1][:3]) and torch.equal(three[2], want[2][:3])


def test_subset_splits_are_exact(H):
    name = "A-frag"
    c, _, _ = _case(name)
    gb = TS._gpu_batch(H, c)
    ms = _models(name, 5)
    rows = _rows(name)
    fields = lambda r: [r.values, r.mean, r.std, r.out_full, r.out_base]                          # noqa: E731
    ev = H.EnsembleSubsetValues(ms)
    want = _clone(fields(ev(gb, rows, per_model=True, **_kw(name))))
    assert int(want[0].unique().numel()) > 20
    for mpl in (1, 2, 5):
        for jpl in (1, 3):
            for rpw in (1, 4):
                split = H.EnsembleSubsetValues(ms)
                split.jobs_per_launch = jpl
                got = fields(split(gb, rows, per_model=True, models_per_launch=mpl, rows_per_workgroup=rpw, **_kw(name)))
                assert _same(want, got), (mpl, jpl, rpw)
    lean = ev(gb, rows, models_per_launch=2, **_kw(name))
    assert lean.values is None and _same(want[1:], fields(lean)[1:])
    three = fields(H.EnsembleSubsetValues(ms[:3])(gb, rows, per_model=True, **_kw(name)))
    assert torch.equal(three[0], want[0][:3]) and torch.equal(three[3], want[3][:3]) and torch.equal(three[4], want[4][:3])


# ------------------------------------------------------------------------------------------------ 3. moments
@pytest.mark.parametrize("M", [1, 5])
def test_moments_against_float64(H, M):
    name = "mixed"                      # graph 3's group 4 has no live member: 0 in every model
    c, _, _ = _case(name)
    gb = TS._gpu_batch(H, c)
    ms = _models(name, 5)[:M]
    r = H.EnsembleShapley(ms)(gb, class_index=c.cls, per_model=True, **_perm(name), **_kw(name))
    fig = EA.moment_figures(r.group_attr, r.group_mean, r.group_std)
    print(f"\n  walk, M {M}: worst |got - fp64| / ((M + 4) 2^-24 s): mean {fig['mean']:.3f} std {fig['std']:.3f}, all-zero players {fig['zeros']}")
    assert fig["mean"] <= 1.0 and fig["std"] <= 1.0 and fig["zeros_exact"] and fig["zeros"] >= 1
    g, y = c.dead
    dead = int(r.group_ptr[g]) + y
    assert float(r.group_attr[:, dead].abs().sum()) == 0.0 and float(r.group_mean[dead]) == 0.0 and float(r.group_std[dead]) == 0.0
    # Captum's gather: every member carries its group's moments, the background 0
    from hcatgnet_amd.shapley import _group_layout
    slot = _group_layout(gb, 25, c.ng.cuda(), c.eg.cuda()).slot
    for node, edge, group in ((r.node_mean, r.edge_mean, r.group_mean), (r.node_std, r.edge_std, r.group_std)):
        assert torch.equal(torch.cat([node.reshape(-1), edge]), torch.cat([group, group.new_zeros(1)])[slot])
    rv = H.EnsembleSubsetValues(ms)(gb, _rows(name), per_model=True, **_kw(name))
    fv = EA.moment_figures(rv.values, rv.mean, rv.std)
    print(f"  rows, M {M}: mean {fv['mean']:.3f} std {fv['std']:.3f}")
    assert fv["mean"] <= 1.0 and fv["std"] <= 1.0 and fv["zeros_exact"]
    if M == 1:
        assert torch.equal(r.group_mean, r.group_attr[0]) and float(r.group_std.abs().max()) == 0.0
        assert torch.equal(rv.mean, rv.values[0]) and float(rv.std.abs().max()) == 0.0
    else:
        assert float(r.group_std.max()) > 0.0 and float(rv.std.max()) > 0.0


# ------------------------------------------------------------------------------------------------ 4. a refused graph
def test_a_refused_graph_is_zero_in_every_models_slice(H):
    name = "mixed"
    c, _, _ = _case(name)
    ms = _models(name, 5)[:3]
    sizes = torch.bincount(c.batch, minlength=c.B)
    big = (sizes == sizes.max()).cuda()
    assert 0 < int(big.sum()) < c.B
    keep = ~big
    es, ev = H.EnsembleShapley(ms), H.EnsembleSubsetValues(ms)
    rows = _rows(name)
    honest_w = _clone(_walk_fields(es(TS._gpu_batch(H, c), class_index=c.cls, per_model=True, **_perm(name), **_kw(name))))
    hv = ev(TS._gpu_batch(H, c), rows, per_model=True, **_kw(name))
    honest_v = _clone([hv.values, hv.out_full, hv.out_base, hv.mean, hv.std])
    gptr = hv.group_ptr
    gbig = torch.repeat_interleave(big, gptr[1:] - gptr[:-1])               # [G]: the group's graph is refused
    for run in ("walk", "rows"):
        gb = TS._gpu_batch(H, c, max_nodes=int(sizes.max()) - 1)
        if run == "walk":
            r = es(gb, class_index=c.cls, per_model=True, models_per_launch=2, **_perm(name), **_kw(name))
            assert es.last_path == "fused"
        else:
            r = ev(gb, rows, per_model=True, rows_per_workgroup=3, models_per_launch=2, **_kw(name))
            assert ev.last_path == "fused"
        torch.cuda.synchronize()
        status = gb._hcg_plan.status
        word = int(status[0].item())
        status.zero_()                                                    # (shared per device: leave it clean for the next test)
        assert word & SHAPE_LIMIT, run
        if run == "walk":
            assert torch.equal(r.group_attr[:, ~gbig], honest_w[0][:, ~gbig]) and float(r.group_attr[:, gbig].abs().max()) == 0.0
            assert float(r.group_mean[gbig].abs().max()) == 0.0 and float(r.group_std[gbig].abs().max()) == 0.0
            assert torch.equal(r.group_mean[~gbig], honest_w[7][~gbig]) and float(honest_w[0][:, gbig].abs().max()) > 0.0
            full, base, hf, hb = r.out_full, r.out_base, honest_w[1], honest_w[2]
        else:
            assert torch.equal(r.values[:, :, keep], honest_v[0][:, :, keep]) and float(r.values[:, :, big].abs().max()) == 0.0
            assert torch.equal(r.mean[:, keep], honest_v[3][:, keep]) and float(r.mean[:, big].abs().max()) == 0.0
            assert float(r.std[:, big].abs().max()) == 0.0 and float(honest_v[0][:, :, big].abs().min()) > 0.0
            full, base, hf, hb = r.out_full, r.out_base, honest_v[1], honest_v[2]
        for m in range(3):                                                # zeros in EVERY model's slice
            assert float(full[m, big].abs().max()) == 0.0 and float(base[m, big].abs().max()) == 0.0
            assert torch.equal(full[m, keep], hf[m, keep]) and torch.equal(base[m, keep], hb[m, keep])
            assert float(hf[m, big].abs().min()) > 0.0


# ------------------------------------------------------------------------------------------------ 5. curves of the mean output
def test_curve_points_are_the_moments_of_the_matching_rows(H):
    from hcatgnet_amd.subsets import ranking
    name = "A-atoms"
    c, _, _ = _case(name)
    gb = TS._gpu_batch(H, c)
    ms = _models(name, 5)[:3]
    sizes = torch.bincount(c.batch).tolist()
    gptr = torch.tensor([0] + sizes).cumsum(0)
    G = int(gptr[-1])
    order = ranking(torch.randn(G, generator=torch.Generator().manual_seed(ROW_SEED)).cuda(), gptr.cuda())
    ec = H.EnsembleCurves(ms)
    r = ec(gb, order, class_index=c.cls, **_kw(name))
    assert ec.last_path == "fused" and isinstance(r, H.EnsembleCurveResult)
    cp = r.curve_ptr.cpu().tolist()
    assert [b - a for a, b in zip(cp[:-1], cp[1:])] == [n + 1 for n in sizes] and torch.equal(r.group_ptr.cpu(), gptr)
    # the same subsets as plain rows of one `EnsembleSubsetValues` call: row k = the first k groups of the order, K + k = the rest
    o = order.flatten().cpu().tolist()
    K = max(sizes) + 1
    pos = torch.empty(G, dtype=torch.long)
    for g, n in enumerate(sizes):
        pos[int(gptr[g]) + torch.tensor(o[int(gptr[g]):int(gptr[g]) + n])] = torch.arange(n)
    first = pos.unsqueeze(0) < torch.arange(K).unsqueeze(1)
    v = H.EnsembleSubsetValues(ms)(gb, torch.cat([first, ~first]).cuda(), **_kw(name))
    worst = 0.0
    for g, n in enumerate(sizes):
        a, b = cp[g], cp[g + 1]
        assert torch.equal(r.insertion[a:b], v.mean[:n + 1, g]) and torch.equal(r.deletion[a:b], v.mean[K:K + n + 1, g])
        assert torch.equal(r.insertion_std[a:b], v.std[:n + 1, g]) and torch.equal(r.deletion_std[a:b], v.std[K:K + n + 1, g])
        assert torch.equal(r.out_base[g], v.mean[0, g]) and torch.equal(r.out_full[g], v.mean[n, g])
        assert torch.equal(r.insertion[a], r.out_base[g]) and torch.equal(r.deletion[a], r.out_full[g])
        for curve, auc in ((r.insertion, r.insertion_auc), (r.deletion, r.deletion_auc)):
            pts = curve[a:b, c.cls].double().cpu()
            want = UR.trapezoid(list(range(n + 1)), pts, n)
            scale = max(1.0, float(curve[a:b].abs().max()))
            bound = UR.TOL * scale + 2.0 ** -23 * scale
            worst = max(worst, abs(float(auc[g]) - want) / bound)
    print(f"\n  curves of the mean of 3 models, {G} atoms: worst |auc - python trapezoid| / bound {worst:.4f}")
    assert worst <= 1.0 and float(r.insertion_std.max()) > 0.0 and r.insertion_auc.dtype == torch.float32


# ------------------------------------------------------------------------------------------------ 6. library level
def test_the_library_reads_n_models(H):
    from hcatgnet_amd import _lib
    figures = ER.library_level(_lib)
    print(f"\n  one-model workspace of 3 permutations: {figures}")
