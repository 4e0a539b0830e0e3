"""GPU tests of the wave-priority rotation in the small-graph tile loops (csrc/fused.hip: tile_prio_begin / _next / _end).

The two waves of a SIMD (w and w + 4 of the 8-wave workgroup) take turns at priority 1, one round of tiles each, and every
wave is back at priority 0 when it leaves a tile loop.  No arithmetic changes, so the cases aim at the LOOP SHAPES where a
priority left raised, or a flip at a wave without a partner, would show as a hang at the barrier behind the loop or as a
changed result: a wave with no tile, partners with different round counts, an odd number of rounds, the dealt partial last
round (whose kernels carry no priority instruction: the waves that run once more are the older ones), several graphs per
tile.  Tile counts follow from the grid the library picks (8 waves per workgroup, one workgroup
per CU) and are derived from the device's CU count.

Each case runs the training step on the tiles -- forward with the readout head in its tail, then the conv backward -- once
with the backward pair (one launch, two phases) and once with the two single launches, and asserts: the pair equals the two
launches (`torch.equal`), a second run equals the first bitwise, every output agrees with the fp64 oracle within the bounds
of tests/test_gpu_fullsize.py (1e-5; conv weight gradients 1e-4)."""
import gc

import pytest
import torch

from tests.helpers import rel_inf
from tests.test_gpu_parity import H, oracle, _model_from_params, _rand_params, TOL, TOL_DW  # noqa: F401

pytestmark = pytest.mark.gpu
F = D = 64
WAVES = 8           # waves per workgroup of the tile kernels; the grid is one workgroup per CU at most


@pytest.fixture(autouse=True)
def _release_graphs():
    yield
    torch.cuda.synchronize()
    gc.collect()
    torch.cuda.synchronize()


def _cus():
    return torch.cuda.get_device_properties(0).multi_processor_count


# name -> (tiles as a function of the CU count, graphs per tile)
CASES = {
    "one_tile":      (lambda cus: 1, 1),                         # one wave works; its partner and six others have no tile
    "partner_short": (lambda cus: WAVES * cus + 1, 1),           # one wave has two rounds, its SIMD partner one
    "two_rounds":    (lambda cus: 2 * WAVES * cus, 1),           # the headline shape: every wave two tiles
    "third_round":   (lambda cus: 2 * WAVES * cus + WAVES, 1),   # one workgroup runs a third round: an odd number of rounds
    "three_rounds":  (lambda cus: 3 * WAVES * cus, 1),           # ... and every wave does, in the plain (rotating) form
    "dealt":         (lambda cus: (5 * WAVES * cus) // 2, 1),    # 2.5 rounds: a partial last round that is not the only one
    "packed":        (lambda cus: 21, 3),                        # three 10-atom graphs per tile, the last tile holds ONE graph
}


def _batch_and_params(case):
    from hcatgnet_amd import synth
    from oracle import screen
    tiles, gpt = CASES[case]
    tiles = tiles(_cus())
    # trees: a ring closure can make structural twins (two bonded atoms with the same closed neighbourhood have equal outputs
    # in exact arithmetic), whose max-pool winner is rounding's call and which no re-draw of the features makes decidable
    if gpt == 1:      # 17 atoms: still one graph per 32-row tile, about half the rows of the 30-atom headline batch
        B, kw = tiles, dict(nodes=17, extra_bonds=0)
    else:
        B, kw = gpt * (tiles - 1) + 1, dict(nodes=10, extra_bonds=0)
    seed = 50 + list(CASES).index(case)
    sb = synth.make_config("C2", num_graphs=B, **kw)
    assert 32 // sb.max_nodes == gpt and -(-B // gpt) == tiles
    params = _rand_params(F, D, seed=seed)
    sb.x, redrawn = screen.make_decidable(params, sb.x, sb.edge_index, sb.batch, sb.num_graphs, seed=seed)
    assert redrawn <= max(1, 0.3 * sb.num_graphs)
    return sb, params, tiles


def _count(monkeypatch, HF):
    """Counts the conv backward launches of the tile family: pair launches and single launches."""
    n = {"pair": 0, "single": 0}
    pair, single = HF.TILES.backward_pair, HF.TILES.backward

    def cp(*a, **kw):
        n["pair"] += 0 if kw.get("query") else 1
        return pair(*a, **kw)

    def cs(*a, **kw):
        n["single"] += 1
        return single(*a, **kw)

    monkeypatch.setattr(HF.TILES, "backward_pair", cp)
    monkeypatch.setattr(HF.TILES, "backward", cs)
    return n


@pytest.mark.parametrize("case", list(CASES))
def test_tile_loops_with_rotating_priority(H, oracle, monkeypatch, case):
    from hcatgnet_amd import functional as HF
    from hcatgnet_amd.train import FusedTrainStep
    sb, params, tiles = _batch_and_params(case)
    N, B = sb.x.shape[0], sb.num_graphs
    grid = min(_cus(), -(-tiles // WAVES))
    if case == "dealt":
        assert tiles > WAVES * grid and tiles % (WAVES * grid) != 0        # what makes the host pick the dealt form
    n = _count(monkeypatch, HF)

    def run(pair):
        m = _model_from_params(H, params)
        step = FusedTrainStep(m, optimizer_step=False)
        step.BWD_PAIR = pair
        batch = sb.as_batch("cuda")
        assert step.reason(batch) is None
        res = []
        for _ in range(2):
            loss = step(batch)
            torch.cuda.synchronize()
            cap = step._bufs["cap"]
            res.append(dict(loss=loss.clone(), out=step.last_out.clone(), emb=cap["emb"][:B].clone(),
                            act0=cap["acts"][0][:N].clone(), flat=step._flat.clone()))
        assert batch._hcg_plan.check_status() == 0
        assert step._head_in_forward(step._prepare(batch, False))          # the head ran in the forward's tail
        return res, {k: v.grad.detach().clone() for k, v in m.named_parameters()}

    (p1, p2), gp = run(True)
    assert n == {"pair": 2, "single": 0}
    (s1, s2), gs = run(False)
    assert n == {"pair": 2, "single": 4}
    assert bool(torch.isfinite(p1["flat"]).all()) and float(p1["flat"].abs().max()) > 0
    for k in p1:
        assert torch.equal(p1[k], p2[k]), ("pair, second run", k)
        assert torch.equal(s1[k], s2[k]), ("two launches, second run", k)
        assert torch.equal(p1[k], s1[k]), ("pair against two launches", k)
    for k in gp:
        assert torch.equal(gp[k], gs[k]), ("pair against two launches", k)

    # fp64 oracle, the reference call and the bounds of tests/test_gpu_fullsize.py
    p64 = {k: v.double() for k, v in params.items()}
    with torch.no_grad():
        _, _, o_acts = oracle.gcn_forward(p64, sb.x.double(), sb.edge_index, sb.batch, B, return_intermediates=True)
    o_loss, o_out, o_emb, g64 = oracle.train_step_grads(params, sb.x, sb.edge_index, sb.batch, sb.y, B, dtype=torch.float64)
    loss = float(p1["loss"])
    errs = {"loss": abs(loss - float(o_loss)) / abs(float(o_loss)), "out": rel_inf(p1["out"], o_out, floor=1.0),
            "emb": rel_inf(p1["emb"], o_emb), "act0": rel_inf(p1["act0"], o_acts[0])}
    gerrs = {k: rel_inf(gp[k], g64[k]) for k in gp}
    print(case, "tiles", tiles, "errors", errs, gerrs)
    for k, e in errs.items():
        assert e <= TOL, (k, errs)
    for k, e in gerrs.items():
        assert e <= (TOL_DW if k.endswith("lin.weight") else TOL), (k, gerrs)
