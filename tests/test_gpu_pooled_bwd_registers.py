"""The pooled layer's backward in its bit form (`poolbits` instead of the stored activations) builds dY' in registers, in the
accumulator layout, and hands it to the aggregation MFMAs without an LDS round trip.  Every case drives the single-layer entry
point and compares it
  1. with the pooled backward on the stored activations and `emb` (dY' built independently, in row layout, staged in LDS):
     dx and dW bitwise, db (summed in another fixed order) to 1e-5 relative;
  2. with the fp64 oracle's autograd, at the project's bounds: 1e-5, and 1e-4 for the conv weight gradient.

The inputs are decidable at fp32: features, weights are small integers, biases odd multiples of 1/32, and every node has 0, 3 or 15
incoming edges, so that (1 + deg)^-1/2 is 1, 1/2 or 1/4 -- the forward is EXACT in fp32 and in fp64 alike, a tie of the column
maximum in one is a tie in the other, and there are no near-ties.  Ties are frequent (integer-valued outputs), a zero row of
W ties a column across ALL rows of every graph, and two isolated nodes with the same features tie pairwise.  The incoming
edges come from random sources: the count matrix is not symmetric, so C and C^T cannot be confused."""
import pytest
import torch
import torch.nn.functional as F

from tests.helpers import rel_inf
from tests.test_gpu_parity import H, oracle  # noqa: F401  (fixtures)
from tests.test_gpu_train_step import _fused_reduce

pytestmark = pytest.mark.gpu

D, SLOPE = 64, 0.01


def _sizes(kind):
    g = torch.Generator().manual_seed({"single": 1, "packed": 2, "many": 3}[kind])
    if kind == "single":      # one graph per tile: 30 nodes, exactly 32 (no empty row), 1 node, and sizes in between
        return torch.tensor([30, 32, 1, 30, 17, 32, 29, 1, 31, 24, 30])
    if kind == "packed":      # three graphs per tile (5..10 nodes), one graph without nodes, the last tile short of graphs
        s = torch.randint(5, 11, (50,), generator=g)
        s[0], s[1], s[17] = 10, 5, 0
        return s
    return torch.randint(17, 33, (2100,), generator=g)   # 2 100 tiles on 2 048 waves: some waves run a second tile


def _make_batch(kind, feat):
    sizes = _sizes(kind)
    B, N = sizes.numel(), int(sizes.sum())
    g = torch.Generator().manual_seed(100 + feat + B)
    batch = torch.repeat_interleave(torch.arange(B), sizes)
    start = torch.cumsum(sizes, 0) - sizes
    local = torch.arange(N) - start[batch]
    n_of = sizes[batch]
    x = torch.randint(-2, 3, (N, feat), generator=g).float()             # mixed signs, exact zeros
    # incoming edges per node: 0, 3 or 15 (dinv 1, 1/2, 1/4).  Graph 3 of `single`: 3 everywhere -> 90 directed edges in a tile
    u = torch.rand(N, generator=g)
    k_in = torch.where(u < 0.15, 0, torch.where(u < 0.95, 3, 15))
    if kind == "single":
        k_in[batch == 3] = 3
    k_in[n_of < 2] = 0
    # pairwise ties: in every second graph the first and the last node are isolated and carry the same features
    pair = (batch % 2 == 0) & (n_of >= 4)
    first, last = pair & (local == 0), pair & (local == n_of - 1)
    k_in[first | last] = 0
    x[last] = x[first]
    dst = torch.repeat_interleave(torch.arange(N), k_in)                  # ascending: edges grouped by graph, as collation emits
    hop = 1 + (torch.rand(dst.numel(), generator=g) * (n_of[dst] - 1).float()).long().clamp(max=(n_of[dst] - 2).clamp(min=0))
    src = start[batch[dst]] + (local[dst] + hop) % n_of[dst]              # another node of the same graph, repeats allowed
    assert bool((src != dst).all()) and bool((batch[src] == batch[dst]).all())
    W = torch.randint(-2, 3, (D, feat), generator=g).float()
    W[5] = 0.0
    W[40] = 0.0                                                           # columns 5 and 40: every row of a graph is the maximum
    # odd multiples of 1/32: dinv * Y is a multiple of 1/16, so no output -- and no column maximum -- is exactly 0.  A maximum
    # of exactly 0 is the one value at which the oracle's max pool (scatter_reduce 'amax' over a zero-filled base) counts the
    # base among the ties and splits the gradient n + 1 ways.
    b = (2 * torch.randint(-8, 8, (D,), generator=g) + 1).float() / 32
    demb = torch.randn(B, 2 * D, generator=g)
    return dict(x=x, ei=torch.stack([src, dst]), batch=batch, B=B, N=N, W=W, b=b, demb=demb, sizes=sizes)


def _oracle_grads(oracle, d, act, premask):
    x, W, b = (t.double().requires_grad_() for t in (d["x"], d["W"], d["b"]))
    y = oracle.gcn_conv(x, d["ei"], W, b)
    a = F.leaky_relu(y, SLOPE) if act else y
    emb = torch.cat([oracle.global_max_pool(a, d["batch"], d["B"]), oracle.global_mean_pool(a, d["batch"], d["B"])], 1)
    (emb * d["demb"].double()).sum().backward()
    dx = x.grad * torch.where(d["x"] > 0, 1.0, SLOPE).double() if premask else x.grad
    return emb.detach(), dx, W.grad, b.grad


_REF = {}


def _reference(oracle, kind, feat, act):
    """the batch and the oracle's gradients, once per (batch, F, activation); the oracle is run twice on the CPU: it has to be
    deterministic on this input (ties, scatter order) before anything is judged by it"""
    key = (kind, feat, act)
    if key not in _REF:
        d = _make_batch(kind, feat)
        first, again = _oracle_grads(oracle, d, act, bool(act)), _oracle_grads(oracle, d, act, bool(act))
        assert all(torch.equal(p, q) for p, q in zip(first, again))
        _REF[key] = (d, first)
    return _REF[key]


# (activation off is run on the two small batches; the large one repeats nothing of it but the size)
@pytest.mark.parametrize("kind,feat,act", [(k, f, a) for k in ("single", "packed", "many") for f in (64, 25) for a in (1, 0)
                                           if not (k == "many" and a == 0)])
def test_bit_form_of_the_pooled_backward(H, oracle, kind, feat, act):
    from hcatgnet_amd import _lib
    from hcatgnet_amd import functional as HF
    from hcatgnet_amd.plan import BatchPlan
    lib, p = _lib.load(), _lib.ptr
    d, (emb_ref, dx_ref, dW_ref, db_ref) = _reference(oracle, kind, feat, act)
    N, B = d["N"], d["B"]
    plan = BatchPlan.build(d["ei"].cuda(), d["batch"].cuda(), N, num_graphs=B, mode="blocked")
    gpt = HF.fused_graphs_per_tile(plan, feat, D)
    assert gpt == (3 if kind == "packed" else 1)
    if kind == "single":
        assert int((plan.edge_ptr[4] - plan.edge_ptr[3]).item()) == 90          # a tile with more than 64 directed edges
    x, W, b, demb = (d[k].cuda() for k in ("x", "W", "b", "demb"))
    new = lambda *s: torch.full(s, float("nan"), device="cuda")
    common = dict(edge_index=plan.edge_index, E=plan.E, graph_ptr=plan.graph_ptr, edge_ptr=plan.edge_ptr, N=N, B=B, D=D,
                  graphs_per_tile=gpt, apply_act=act, slope=SLOPE, status=plan.status)
    out, emb = new(N, D), new(B, 2 * D)
    _lib.fused_forward(x=x, W1=W, b1=b, F=feat, out1=out, emb=emb, **common)
    bits, embt = torch.zeros(lib.hcg_fused_aux_bytes(_lib.HCG_FUSED_POOLBITS, B, gpt), dtype=torch.uint8, device="cuda"), new(B, 2 * D)
    _lib.fused_forward(x=x, W1=W, b1=b, F=feat, emb=embt, poolbits=bits, **common)
    assert torch.equal(emb, embt)
    assert rel_inf(emb, emb_ref) <= 1e-6              # (the forward is exact up to the mean's division)
    # the ties the case is about are there: columns 5 / 40 tie all rows, the isolated twins tie pairwise
    sizes = d["sizes"].cuda()
    assert bool((out[:, 5] == out[0, 5]).all()) and bool((out[:, 40] == out[0, 40]).all())
    gp = plan.graph_ptr.long()
    twins = [g for g in range(0, min(B, 50), 2) if int(sizes[g]) >= 4]
    assert twins and all(torch.equal(out[gp[g]], out[gp[g + 1] - 1]) for g in twins)

    flags = 3 if act else 0      # activation on: dx leaves premasked (x = "the layer below's output"); off: the plain stores
    wsb = lib.hcg_fused_workspace_bytes(B, feat, D, gpt)
    geo = (p(plan.edge_index), plan.E, p(plan.graph_ptr), p(plan.edge_ptr), N, B)

    def run(*lead):
        ws = torch.empty(wsb, dtype=torch.uint8, device="cuda")
        dx, dW, db = new(N, feat), new(D, feat), new(D)
        _lib.check(lib.hcg_fused_layer_bwd(*lead, p(x), p(W), *geo, feat, D, gpt, SLOPE, flags, p(dx), p(plan.status), p(ws), wsb,
                                           _lib.stream_ptr()), "hcg_fused_layer_bwd")
        _fused_reduce(lib, _lib, ws, wsb, N, B, feat, D, gpt, dW, db)
        return dx, dW, db

    dx, dW, db = run(None, p(demb), p(emb), p(out), None)          # stored activations: dY' in row layout, through LDS
    dxt, dWt, dbt = run(None, p(demb), None, None, p(bits))        # bits: dY' in registers
    assert int(plan.status[0]) == 0
    errs = dict(db_forms=rel_inf(dbt, db), dx=rel_inf(dxt, dx_ref), dW=rel_inf(dWt, dW_ref), db=rel_inf(dbt, db_ref))
    print(kind, feat, act, "dx/dW bitwise", torch.equal(dx, dxt), torch.equal(dW, dWt), errs)
    assert torch.equal(dx, dxt) and torch.equal(dW, dWt)
    assert errs["db_forms"] <= 1e-5
    assert errs["dx"] <= 1e-5 and errs["db"] <= 1e-5 and errs["dW"] <= 1e-4
    assert rel_inf(dx, dx_ref) <= 1e-5 and rel_inf(dW, dW_ref) <= 1e-4
