"""GPU tests of `GreedySelection`: the greedy insertion / deletion order of a graph's groups, one launch per round and the
winner picked on chip (csrc/shapley.hip, k_greedy_round, HCG_EXPLAIN_GREEDY).  tests/greedy_ref.py states the reference (a
replay of the result's own order against the fp64 oracle) and the bounds; the cases are those of tests/test_gpu_subsets.py.
Every figure is printed before it is asserted (`pytest -s`)."""
import pytest
import torch

from tests import greedy_ref as YR
from tests import shapley_ref as SR
from tests import subsets_ref as UR
from tests import test_gpu_subsets as TS
from tests.test_gpu_subsets import H  # noqa: F401  (the fixture)

pytestmark = pytest.mark.gpu
COMBOS = [("insertion", 1), ("insertion", -1), ("deletion", 1), ("deletion", -1)]


def _setup(H, name):
    from hcatgnet_amd.greedy import GreedySelection
    c = TS._case(name)
    model = SR.model_from_params(H, c.params).cuda()
    return c, model, GreedySelection(model), TS._gpu_batch(H, c)


def _clone(r):
    return type(r)(*[t.clone() for t in r])


def _status_clean(gb):
    torch.cuda.synchronize()
    return int(gb._hcg_plan.status[0].item()) == 0


# ------------------------------------------------------------------------------------------------ 1. the fp64 replay
@pytest.mark.parametrize("mode, direction", COMBOS)
@pytest.mark.parametrize("name", ["atoms", "mixed", "four-convs", "dense30"])
def test_full_runs_pass_the_fp64_replay(H, name, mode, direction):
    c, model, gs, gb = _setup(H, name)
    fw = TS._forwards(name)
    assert gs.reason(gb) is None
    r = gs(gb, class_index=c.cls, mode=mode, direction=direction, **TS._kw(c))
    assert gs.last_path == "fused" and isinstance(r, H.GreedyResult) and _status_clean(gb)
    if name == "atoms":
        assert [fw.count(g) for g in range(c.B)] == [31, 32, 33, 40]
    if name == "four-convs":
        assert c.cls == 5 and r.values.shape[1] == 8
    if name == "dense30":
        assert fw.count(0) == 2
    YR.replay(r, fw, c.cls, mode, direction, tag=name)


def test_three_rounds_at_the_node_limit(H):
    from hcatgnet_amd.subsets import SubsetValues
    c, model, gs, gb = _setup(H, "node-limit")
    fw = TS._forwards("node-limit")
    assert fw.count(0) == TS.NODE_LIMIT == 184
    r = gs(gb, class_index=c.cls, steps=3, **TS._kw(c))
    assert gs.last_path == "fused" and gs.launches == 4 and _status_clean(gb)
    YR.replay(r, fw, c.cls, "insertion", steps=3, tag="node-limit")
    assert bool((r.order[0, 3:] == -1).all()) and float(r.values[3:].abs().sum()) == 0.0 and r.steps.tolist() == [3]
    lds = gs.lds_bytes(gb)
    print(f"    lds_bytes {lds}")
    assert 0 < lds <= 160 * 1024 and lds == SubsetValues(model).lds_bytes(gb)


# ------------------------------------------------------------------------------------------------ 2. bitwise against what exists
@pytest.mark.parametrize("name", ["atoms", "mixed"])
def test_bitwise_the_loop_the_curves_and_the_subset_outputs(H, name):
    from hcatgnet_amd.subsets import AttributionCurves, SubsetValues
    c, model, gs, gb = _setup(H, name)
    kw = TS._kw(c)
    G = int(TS._forwards(name).gptr[-1])
    ends = SubsetValues(model)(gb, torch.zeros(0, G, dtype=torch.bool).cuda(), **kw)
    out_full, out_base = ends.out_full.clone(), ends.out_base.clone()
    for mode, direction in COMBOS:
        r = gs(gb, class_index=c.cls, mode=mode, direction=direction, **kw)
        assert gs.last_path == "fused"
        lp = gs.loop(gb, class_index=c.cls, mode=mode, direction=direction, **kw)
        assert gs.last_path == "loop" and gs.values.last_path == "fused"
        assert torch.equal(r.order, lp.order) and torch.equal(r.values, lp.values) and torch.equal(r.steps, lp.steps)
        assert torch.equal(r.out_full, out_full) and torch.equal(r.out_base, out_base)
        assert torch.equal(lp.out_full, out_full) and torch.equal(lp.out_base, out_base)
        cur = AttributionCurves(model)(gb, r.order, class_index=c.cls, **kw)
        cp, gp = cur.curve_ptr.tolist(), r.group_ptr.tolist()
        for g in range(c.B):
            curve = (cur.insertion if mode == "insertion" else cur.deletion)[cp[g] + 1:cp[g + 1]]
            assert torch.equal(curve, r.values[gp[g]:gp[g + 1]]), (mode, direction, g)
        print(f"    {name} {mode} {direction:+d}: {int(r.values.unique().numel())} distinct values, bitwise the loop's and the curve's")
    assert int(r.values.unique().numel()) > 5


# ------------------------------------------------------------------------------------------------ 3. independence
@pytest.mark.parametrize("mode", ["insertion", "deletion"])
def test_bitwise_ids_per_job_batch_call_instance_and_truncation(H, mode):
    from hcatgnet_amd.greedy import GreedySelection
    c, model, gs, gb = _setup(H, "atoms")
    kw = dict(class_index=c.cls, mode=mode)
    base = _clone(gs(gb, ids_per_job=1, **kw, **TS._kw(c)))
    assert gs.last_path == "fused" and int(base.values.unique().numel()) > 100
    for ipj in (7, None):
        assert YR.same(base, gs(gb, ids_per_job=ipj, **kw, **TS._kw(c))), ipj
    assert YR.same(base, gs(gb, ids_per_job=7, **kw, **TS._kw(c)))                              # a second call
    assert YR.same(base, GreedySelection(model)(gb, ids_per_job=7, **kw, **TS._kw(c)))          # a second instance
    gp = base.group_ptr.tolist()
    for g in range(c.B):
        one, okw = TS._one_graph(H, c, g)
        alone = gs(one, **kw, **okw)
        assert torch.equal(alone.order[0], base.order[0, gp[g]:gp[g + 1]]) and torch.equal(alone.values, base.values[gp[g]:gp[g + 1]])
        assert torch.equal(alone.steps, base.steps[g:g + 1])
        assert torch.equal(alone.out_full[0], base.out_full[g]) and torch.equal(alone.out_base[0], base.out_base[g])
    assert not torch.equal(base.order[0, gp[0]:gp[0] + 31], base.order[0, gp[1]:gp[1] + 31])
    five = gs(gb, steps=5, **kw, **TS._kw(c))
    assert gs.launches == 6 and five.steps.tolist() == [5] * 4
    for g in range(c.B):
        a, b = gp[g], gp[g + 1]
        assert torch.equal(five.order[0, a:a + 5], base.order[0, a:a + 5]) and torch.equal(five.values[a:a + 5], base.values[a:a + 5])
        assert bool((five.order[0, a + 5:b] == -1).all()) and float(five.values[a + 5:b].abs().sum()) == 0.0
    assert torch.equal(five.out_full, base.out_full) and torch.equal(five.out_base, base.out_base)


# ------------------------------------------------------------------------------------------------ 4. exact ties
@pytest.mark.parametrize("name", ["atoms", "mixed"])
def test_exact_ties_go_to_the_lower_group_id(H, name):
    from hcatgnet_amd.greedy import GreedySelection
    c, fw = TS._case(name), TS._forwards(name)
    p = dict(c.params)
    last = [k for k in p if k.startswith("readout") and k.endswith("weight")][-1]
    p[last] = torch.zeros_like(p[last])
    assert p[last].shape[0] == 1
    gs = GreedySelection(SR.model_from_params(H, p).cuda())
    gb = TS._gpu_batch(H, c)
    want = []
    for g in range(c.B):
        ids = list(range(fw.count(g)))
        want += [y for y in ids if bool(fw.live[g][y])] + [y for y in ids if not bool(fw.live[g][y])]
    for mode, direction in COMBOS:
        r = gs(gb, mode=mode, direction=direction, **TS._kw(c))
        assert gs.last_path == "fused" and r.order.flatten().tolist() == want, (mode, direction)
        assert int(r.values.unique().numel()) == 1 and bool((r.values == r.out_full[0]).all())


# ------------------------------------------------------------------------------------------------ 5. launches
def test_one_launch_per_round_and_one_more(H):
    c, model, gs, gb = _setup(H, "mixed")
    fw = TS._forwards("mixed")
    lives = [int(fw.live[g].sum()) for g in range(c.B)]
    assert lives == [0, 1, 3, 4]
    for steps in (None, 2):
        gs(gb, class_index=c.cls, steps=steps, **TS._kw(c))
        want = max(L if steps is None else min(steps, L) for L in lives) + 1
        print(f"    steps {steps}: {gs.launches} launches")
        assert gs.launches == want and gs.last_path == "fused"


# ------------------------------------------------------------------------------------------------ 6. refusal
def test_a_batch_over_the_node_limit_takes_the_loop_with_the_same_bounds(H):
    c, model, gs, _ = _setup(H, "mixed")
    gb = TS._gpu_batch(H, c, max_nodes=TS.NODE_LIMIT + 1)
    assert "shape" in gs.reason(gb) and gs.lds_bytes(gb) is None
    for mode in ("insertion", "deletion"):
        r = gs(gb, class_index=c.cls, mode=mode, **TS._kw(c))
        assert gs.last_path == "loop" and gs.values.last_path == "loop"
        YR.replay(r, TS._forwards("mixed"), c.cls, mode, tag="mixed, max_nodes 185 (loop)")


def test_a_graph_over_max_nodes_is_refused_and_the_others_keep_their_results(H):
    c, model, gs, gb_honest = _setup(H, "mixed")
    fw = TS._forwards("mixed")
    sizes = torch.bincount(c.batch, minlength=c.B)
    big = (sizes == sizes.max()).tolist()
    assert 0 < sum(big) < c.B
    for mode in ("insertion", "deletion"):
        honest = _clone(gs(gb_honest, class_index=c.cls, mode=mode, **TS._kw(c)))
        gb = TS._gpu_batch(H, c, max_nodes=int(sizes.max()) - 1)
        r = gs(gb, class_index=c.cls, mode=mode, ids_per_job=2, **TS._kw(c))
        assert gs.last_path == "fused"
        torch.cuda.synchronize()
        status = gb._hcg_plan.status
        word = int(status[0].item())
        status.zero_()                                                    # (shared per device: leave it clean for the next test)
        assert word & TS.SHAPE_LIMIT
        gp = r.group_ptr.tolist()
        assert torch.equal(r.steps, honest.steps)
        for g in range(c.B):
            a, b, L = gp[g], gp[g + 1], int(fw.live[g].sum())
            if big[g]:
                # no pick, zero values and outputs (the host still lists the dead groups behind a full run)
                assert bool((r.order[0, a:a + L] == -1).all()) and float(r.values[a:b].abs().sum()) == 0.0
                assert float(r.out_full[g].abs().max()) == 0.0 and float(r.out_base[g].abs().max()) == 0.0
                assert float(honest.out_full[g].abs().min()) > 0.0
            else:
                assert torch.equal(r.order[0, a:b], honest.order[0, a:b]) and torch.equal(r.values[a:b], honest.values[a:b])
                assert torch.equal(r.out_full[g], honest.out_full[g]) and torch.equal(r.out_base[g], honest.out_base[g])
