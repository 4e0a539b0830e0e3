"""GPU tests of the backward pair (csrc/fused.hip: k_fused_bwd_pair) as the training step's default: the shapes at which the
boundary between its two phases can go wrong -- waves without a tile, a dealt third round, tiles with more than 64 edges
and with none, the lower layer's scalar stager, several graphs per tile.  The reference is the two-launch step of the same
build (`BWD_PAIR = False`), itself held to the fp64 oracle by the existing suites; every comparison is `torch.equal`.  One
case is also held to the fp64 oracle directly."""
import gc

import numpy as np
import pytest
import torch

from tests.helpers import rel_inf
from tests.test_gpu_parity import H, oracle, TOL, TOL_DW  # noqa: F401  (fixtures, the full-size suite's tolerances)

pytestmark = pytest.mark.gpu
D = 64
CASES = ["idle_waves", "three_rounds", "edge_counts", "narrow", "packed"]
PACKED = [10, 7, 10, 3, 10, 10, 9, 1, 10, 10, 10, 6, 10]


@pytest.fixture(autouse=True)
def _release_graphs():
    yield
    torch.cuda.synchronize()
    gc.collect()
    torch.cuda.synchronize()


def _cus():
    return torch.cuda.get_device_properties(0).multi_processor_count


def _case(name):
    """-> (node counts, F, {graph: number of bonds} overrides)."""
    if name == "idle_waves":      # one workgroup, three tiles: five of its waves own no tile in either phase
        return [30, 30, 30], 64, {}
    if name == "three_rounds":    # two full rounds + 5 tiles dealt over the workgroups (TileSeq<true>): some waves run a third
        return [30] * (8 * _cus() * 2 + 5), 64, {}        # tile in both phases
    if name == "edge_counts":     # 45 bonds = 90 directed edges: the k0 > 0 reload inside TileEdges::build; graph 2 has no edge
        return [30, 30, 30, 28, 30], 64, {1: 45, 2: 0, 3: 40}
    if name == "narrow":          # KPAD0 = 32, VEC0 = false: the lower layer's x rows come through the scalar stager
        return [20] * 11, 25, {}
    if name == "packed":          # three graphs per tile, the last tile holds a single graph
        return PACKED, 64, {}
    if name == "packed_trees":    # the same graphs as chains: a chord can close a triangle, whose structural twins have EQUAL
        return PACKED, 64, {g: n - 1 for g, n in enumerate(PACKED)}   # outputs in exact arithmetic -- no screening decides their max
    raise KeyError(name)


_GRAPHS = {}


def _graphs(name):
    if name not in _GRAPHS:
        _GRAPHS[name] = _make_graphs(name)
    return _GRAPHS[name]


def _make_graphs(name, seed=0):
    """A collated batch: per graph a chain plus random chords (both directions, grouped by graph), or exactly the number
    of bonds the case asks for.  -> (x, edge_index, batch vector, y, max directed edges of a graph), on the CPU."""
    ns, feat, bonds = _case(name)
    rng = np.random.default_rng(seed + 100 * (CASES + ["packed_trees"]).index(name))
    src, dst, me, base = [], [], 0, 0
    for g, n in enumerate(ns):
        want = bonds.get(g, (n - 1) + n // 3 if n > 1 else 0)
        e = [(i, i + 1) for i in range(min(n - 1, want))]
        while len(e) < want:
            i, j = rng.choice(n, 2, replace=False)
            e.append((int(i), int(j)))
        for i, j in e:
            src += [base + i, base + j]
            dst += [base + j, base + i]
        me = max(me, 2 * len(e))
        base += n
    x = torch.from_numpy(rng.standard_normal((base, feat), dtype=np.float32))
    ei = torch.tensor([src, dst], dtype=torch.int64).reshape(2, -1)
    bv = torch.from_numpy(np.repeat(np.arange(len(ns)), ns)).long()
    y = torch.from_numpy((10.0 * rng.standard_normal(len(ns))).astype(np.float32))
    return x, ei, bv, y, max(me, 1)


def _batch(H, name):
    ns, feat, _ = _case(name)
    x, ei, bv, y, me = _graphs(name)
    x, ei, bv, y = x.cuda(), ei.cuda(), bv.cuda(), y.cuda()      # uploaded once: `mk` also runs inside a stream capture
    return (lambda: H.Batch(x, ei, bv, len(ns), y=y, max_nodes=int(max(ns)), max_edges=me, edges_grouped=True)), feat, ns


def _model(H, F, seed=0):
    torch.manual_seed(seed)
    m = H.make_network("GCN", H.default_options(n_convolutions=2), F).cuda()
    with torch.no_grad():
        for q in m.parameters():
            if q.dim() == 1:
                q.add_(0.05)
    return m


NAMES = ["loss", "out", "emb", "dx", "upper slabs", "lower slabs", "flat gradient"]


def _results(H, step, m, ns, feat):
    """What one step left behind: loss, outputs, pooled embedding, dx, both slab sets, the flat gradient, the weights."""
    cap, B, N = step._bufs["cap"], len(ns), int(sum(ns))
    tiles = -(-B // (32 // max(ns)))
    grid = min(-(-tiles // 8), _cus())
    kpad0 = 32 if feat <= 32 else 64
    slabs = [cap["ws"][1][:grid * (D * D + D) * 4], cap["ws"][0][:grid * (D * kpad0 + D) * 4]]
    return ([None, step.last_out.clone(), cap["emb"][:B].clone(), cap["dacts"][0][:N].clone()] + [s.clone() for s in slabs]
            + [step._flat.clone()] + [q.detach().clone() for q in m.parameters()])     # [0]: the loss, set by the caller


def _one_step(H, name, pair):
    from hcatgnet_amd import functional as HF
    from hcatgnet_amd.train import FusedTrainStep
    mk, feat, ns = _batch(H, name)
    m = _model(H, feat)
    step = FusedTrainStep(m)
    step.BWD_PAIR = pair
    batch = mk()
    launched = []
    orig = HF.TILES.backward_pair
    HF.TILES.backward_pair = lambda *a, **kw: (launched.append(1) if not kw.get("query") else None, orig(*a, **kw))[1]
    try:
        loss = step(batch)
        torch.cuda.synchronize()
    finally:
        HF.TILES.backward_pair = orig
    assert batch._hcg_plan.check_status() == 0
    assert len(launched) == (1 if pair else 0)
    res = _results(H, step, m, ns, feat)
    res[0] = loss.clone()
    return res


_REF = {}


def _reference(H, name):
    """The two-launch step's results, computed once per case and left unchanged."""
    if name not in _REF:
        _REF[name] = _one_step(H, name, False)
    return _REF[name]


@pytest.mark.parametrize("name", CASES)
def test_pair_step_equals_the_two_launch_step(H, name):
    ref, got = _reference(H, name), _one_step(H, name, True)
    assert bool(torch.isfinite(ref[6]).all()) and float(ref[6].abs().max()) > 0 and float(ref[3].abs().max()) > 0
    names = NAMES + [f"weight {i} after Adam" for i in range(len(ref) - len(NAMES))]
    assert len(ref) == len(got) == len(names)
    for what, r, g in zip(names, ref, got):
        assert torch.equal(r, g), what


@pytest.mark.parametrize("name", ["idle_waves", "three_rounds"])
def test_forty_replays_of_the_captured_pair_step_are_bitwise_identical(H, name):
    """The behavioural guard of the MFMA result-fence rule for the pair kernel: the weights are frozen (no optimiser
    step), so every replay computes the same step and must leave the same bits."""
    from hcatgnet_amd.train import FusedTrainStep
    mk, feat, ns = _batch(H, name)
    m = _model(H, feat)
    step = FusedTrainStep(m, optimizer_step=False)
    step.BWD_PAIR = True
    step.capture(mk)
    first = None
    for i in range(40):
        loss = step.replay()
        torch.cuda.synchronize()
        res = _results(H, step, m, ns, feat)
        res[0] = loss.clone()
        if first is None:
            first = res
            assert float(first[6].abs().max()) > 0
            continue
        for what, r, g in zip(NAMES, first, res):
            assert torch.equal(r, g), (what, i)
    assert step._prepare(mk(), False).bwd_pair is True


def test_pair_step_against_the_fp64_oracle(H, oracle):
    """The several-graphs-per-tile case, screened (oracle/screen.py) so that the comparison is decidable, with the
    tolerances of tests/test_gpu_fullsize.py."""
    from hcatgnet_amd.train import FusedTrainStep
    from oracle import screen
    ns, feat, _ = _case("packed_trees")
    x, ei, bv, y, me = _graphs("packed_trees")
    m = _model(H, feat, seed=3)
    params = {k: v.detach().cpu().clone() for k, v in m.state_dict().items()}
    B = len(ns)
    x, _ = screen.make_decidable(params, x, ei, bv, B, seed=5)
    step = FusedTrainStep(m, optimizer_step=False)
    step.BWD_PAIR = True
    batch = H.Batch(x.cuda(), ei.cuda(), bv.cuda(), B, y=y.cuda(), max_nodes=int(max(ns)), max_edges=me, edges_grouped=True)
    loss = float(step(batch))
    torch.cuda.synchronize()
    assert batch._hcg_plan.check_status() == 0 and step._prepare(batch, False).bwd_pair is True
    o_loss, o_out, o_emb, g64 = oracle.train_step_grads(params, x, ei, bv, y, B, dtype=torch.float64)
    assert abs(loss - float(o_loss)) <= TOL * abs(float(o_loss))
    assert rel_inf(step.last_out, o_out, floor=1.0) <= TOL
    assert rel_inf(step._bufs["cap"]["emb"][:B], o_emb) <= TOL
    for k, q in m.named_parameters():
        e64 = rel_inf(q.grad, g64[k])
        print(k, "rel err vs fp64", e64)
        assert e64 <= (TOL_DW if k.endswith("lin.weight") else TOL), (k, e64)
