"""A frozen-model object reuses one argument block and one buffer pool from call to call (hcatgnet_amd/_frozen.py).  The
members of the block that differ between call forms overlay one union, and the buffers keep the size of the largest call:
a second call of another form, or of a smaller size, must return bit for bit what a fresh object returns."""
import os

import pytest
import torch

from tests import shapley_ref as SR

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def H():
    import hcatgnet_amd
    import __graft_entry__
    from hcatgnet_amd import _lib
    if not os.path.isfile(_lib.LIB_PATH):
        __graft_entry__.build()
    return hcatgnet_amd


def _keep(r):
    return [t.clone() for t in r]


def _same(a, b):
    return len(a) == len(b) and all(torch.equal(p, q) for p, q in zip(a, b))


def test_a_reused_object_returns_what_a_fresh_one_returns(H):
    """Two graphs of 3 and 5 nodes with 4 and 8 directed edges, F = 25, two conv layers, two classes; every launch loop
    is split (3 permutations in launches of 2, 4 steps in launches of 3)."""
    from hcatgnet_amd.shapley import ShapleySampling, atom_groups, draw_group_permutations, draw_permutations
    gen = lambda seed: torch.Generator().manual_seed(seed)
    F = 25
    x = torch.randn(8, F, generator=gen(3)) * (torch.rand(8, F, generator=gen(4)) < 0.4)
    chain = lambda lo, hi: [(i, i + 1) for i in range(lo, hi)] + [(i + 1, i) for i in range(lo, hi)]
    ei = torch.tensor(chain(0, 2) + chain(3, 7), dtype=torch.int64).t().contiguous()
    bv = torch.tensor([0] * 3 + [1] * 5, dtype=torch.int64)
    assert ei.shape == (2, 12) and int((bv[ei[1]] == 0).sum()) == 4
    gb = H.Batch(x.cuda(), ei.cuda(), bv.cuda(), 2, max_nodes=5, max_edges=8, edges_grouped=True)
    model = SR.model_from_params(H, SR.rand_params(F, 64, seed=23, n_conv=2, n_read=2, n_classes=2)).cuda()

    perm = draw_permutations(gb, F, 3, gen(11))
    ag = atom_groups(gb)
    gperm = draw_group_permutations(gb, ag, None, 3, gen(12))
    calls = (dict(permutations=perm), dict(node_group=ag, group_permutations=gperm), dict(permutations=perm))
    sv = ShapleySampling(model)
    assert sv.reason(gb) is None
    got = []
    for kw in calls:
        got.append(_keep(sv(gb, class_index=1, samples_per_launch=2, **kw)))
        assert sv.last_path == "fused"
    assert isinstance(sv(gb, class_index=1, **calls[1]), H.GroupedShapleyResult)
    for k, kw in enumerate(calls):
        assert _same(got[k], _keep(ShapleySampling(model)(gb, class_index=1, samples_per_launch=2, **kw))), k
    assert _same(got[0], got[2]) and float(got[0][0].abs().max()) > 0 and float(got[1][0].abs().max()) > 0

    calls = (dict(n_steps=4, steps_per_launch=3), dict(n_steps=2))
    ig = H.IntegratedGradients(model, n_steps=4)
    assert ig.reason(gb) is None
    got = []
    for kw in calls:
        got.append(_keep(ig(gb, class_index=1, **kw)))
        assert ig.last_path == "fused"
    for k, kw in enumerate(calls):
        assert _same(got[k], _keep(H.IntegratedGradients(model, n_steps=4)(gb, class_index=1, **kw))), k
    assert not _same(got[0][:2], got[1][:2]) and float(got[1][0].abs().max()) > 0
    torch.cuda.synchronize()
    assert int(gb._hcg_plan.status[0].item()) == 0
