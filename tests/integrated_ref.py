"""Reference, inputs and checks of `hcatgnet_amd.attribution.IntegratedGradients` (tests/test_host_integrated.py and
tests/test_gpu_integrated.py).

Reference.  fp64 autograd through `oracle.gcn_forward(..., edge_mask=)` on `x * node_mask`, at each quadrature point alpha_k
taken as the float32 value of `quadrature` converted to double, every node-mask and edge-mask entry equal to alpha_k, the
upstream gradient 1 at column `class_index`; summed with w_k (the float32 value, as double) in float64 on the CPU.  Never the
any-shape GPU path, never the code under test.

Decidability.  The LeakyReLU derivative and the max-pool arg-max are discontinuous in the forward values (oracle/screen.py and
the docstring of tests/test_gpu_explain.py explain why that matters).  The masks are fixed by the algorithm here, so the
screen re-draws node features: `tests.test_gpu_explain._flagged` (2e-6 absolute on conv and readout pre-activations, relative
2e-6 on a positive max-pool gap) is evaluated at EVERY quadrature point, and x ~ N(0, 1) of the nodes of flagged graphs is
re-drawn from Generator(6) until no graph is flagged at any point (at most 12 rounds, asserted): no graph is ever left out.
The golden fixture's one-hot features cannot be re-drawn; there the flagged graphs' x is perturbed by N(0, 1) * 1e-2.
On the golden fixture the screen also flags a graph with an EXACT max-pool tie at some point (`_tied`).  Its molecules have
symmetric atoms: equal one-hot rows in mirrored neighbourhoods.  Under the uniform masks of this algorithm such rows are equal
in exact arithmetic, but each side sums a row's neighbours in its own order, so whether the tie survives rounding (gradient
split evenly) or breaks by one ulp (everything to one atom) is decided by the summation order, on the fp64 side too: with the
margins alone the CPU loop path missed the bound on this case at 3e-3 and the kernel at 7e-2 on one host while the fp32
oracle met it at 4e-7.  Random masks break the symmetry in tests/test_gpu_explain.py; here the perturbation has to.  Exact
ties between bit-identical rows, which every side must keep, have their own hand-built test.

The step counts of the cases are small on purpose: the number of graphs flagged grows with the number of points (a probe of
`ragged` with 12 graphs had 11 of 12 flagged at 16 points and 12 of 12 at 50, where no re-draw settles).

Bound.  TOL = 1e-5, the project's, as per-graph rel_inf of node_attr and of edge_attr; out_full and out_base with floor 1.0.
The fp32 oracle's own per-graph error against fp64 on these cases is at most 5.7e-7.  Every figure is printed before it is
asserted (`pytest -s`)."""
import functools

import torch

from tests.helpers import golden_files, load_golden, rel_inf
from tests.test_gpu_explain import CASES as SHAPES
from tests.test_gpu_explain import PARAM_SEED, _flagged, _per_graph, _rand_params

TOL = 1e-5
DRAW_SEED = 6
MAX_ROUNDS = 12
# name -> (graphs, n_steps, class_index); shapes and model depths: tests.test_gpu_explain.CASES
CASES = {"small30": (8, 6, 0), "ragged": (8, 4, 0), "deep": (6, 4, 1), "limit224": (2, 3, 0), "real-size": (6, 4, 0)}
GOLDEN_STEPS = 4


def _oracle():
    from oracle import gcn_oracle
    return gcn_oracle


def _tied(h, batch, B):
    """graphs with more than one row at a feature's maximum -> bool [B]"""
    idx = batch.unsqueeze(1).expand_as(h)
    top = h.new_full((B, h.shape[1]), float("-inf")).scatter_reduce(0, idx, h, reduce="amax", include_self=True)
    count = torch.zeros(B, h.shape[1], dtype=torch.long).scatter_add(0, idx, (h == top[batch]).long())
    return (count > 1).any(dim=1)


def reference(params, x, ei, batch, B, alpha, weight, cls, screen=True, ties=False):
    """-> dict(node [N, F], edge [E], out_full [B, C], out_base [B, C], per_step [(G node, G edge)]; all float64,
    flagged bool [B]: graphs whose branch decisions are not decidable at some point; with `ties` an exact max-pool tie counts)"""
    O = _oracle()
    p = {k: v.double() for k, v in params.items()}
    (N, F), E = x.shape, ei.shape[1]
    x64 = x.double()
    node, edge = torch.zeros(N, F, dtype=torch.float64), torch.zeros(E, dtype=torch.float64)
    bad = torch.zeros(B, dtype=torch.bool)
    per_step = []
    for a, w in zip(alpha.double().tolist(), weight.double().tolist()):
        em = torch.full((E,), a, dtype=torch.float64, requires_grad=True)
        nm = torch.full((N, F), a, dtype=torch.float64, requires_grad=True)
        out, emb, acts = O.gcn_forward(p, x64 * nm, ei, batch, B, edge_mask=em, return_intermediates=True)
        g_n, g_e = torch.autograd.grad(out[:, cls].sum(), [nm, em])
        node += w * g_n
        edge += w * g_e
        per_step.append((g_n, g_e))
        if screen:
            bad |= _flagged(params, dict(acts=[t.detach() for t in acts], emb=emb.detach()), batch, B)
            if ties:
                bad |= _tied(acts[-1].detach(), batch, B)
    with torch.no_grad():
        full = O.gcn_forward(p, x64, ei, batch, B, edge_mask=torch.ones(E, dtype=torch.float64))[0]
        base = O.gcn_forward(p, x64 * 0.0, ei, batch, B, edge_mask=torch.zeros(E, dtype=torch.float64))[0]
    return dict(node=node, edge=edge, out_full=full.reshape(B, -1), out_base=base.reshape(B, -1), flagged=bad, per_step=per_step)


def decidable(params, x, ei, batch, B, alpha, weight, cls, redraw, ties=False):
    """-> (x, reference) with no graph flagged at any point; `redraw(x, node mask of the flagged graphs)` changes x in place"""
    x = x.clone()
    touched = torch.zeros(B, dtype=torch.bool)
    for rounds in range(MAX_ROUNDS + 1):
        ref = reference(params, x, ei, batch, B, alpha, weight, cls, ties=ties)
        bad = ref["flagged"]
        if not bool(bad.any()):
            print(f"    node features decidable after {rounds} rounds, {int(touched.sum())} of {B} graphs re-drawn")
            assert rounds <= MAX_ROUNDS
            return x, ref
        touched |= bad
        redraw(x, bad[batch])
    raise AssertionError(f"graphs still flagged after {MAX_ROUNDS} rounds")


class Case:
    pass


def _finish(c, method, redraw, ties=False):
    from hcatgnet_amd.attribution import quadrature
    c.method = method
    c.alpha, c.weight = quadrature(method, c.n_steps)
    c.x, c.ref = decidable(c.params, c.x, c.ei, c.batch, c.B, c.alpha, c.weight, c.cls, redraw, ties)
    c.edge_owner = c.batch[c.ei[1]]
    return c


@functools.lru_cache(maxsize=None)
def case(name, method="gausslegendre"):
    """-> params, graphs (CPU), quadrature and the fp64 reference of a named case; x is what the screen left."""
    from hcatgnet_amd import synth
    c = Case()
    c.name = name
    gen = torch.Generator().manual_seed(DRAW_SEED)
    if name == "golden":
        g = load_golden(golden_files()[0])
        c.params, c.x, c.ei, c.batch, c.B = g["params"], g["x"].float(), g["edge_index"], g["batch"], g["num_graphs"]
        n = torch.bincount(c.batch, minlength=c.B)
        e = torch.bincount(c.batch[c.ei[1]], minlength=c.B)
        c.max_nodes, c.max_edges = int(n.max()), int(e.max())
        c.n_steps, c.cls = GOLDEN_STEPS, 0

        def redraw(x, m):
            x[m] += 1e-2 * torch.randn(int(m.sum()), x.shape[1], generator=gen)
    else:
        shape, _, width = name.partition("-d")              # "ragged-d128": the shapes of `ragged`, embedding_dim 128
        graphs, c.n_steps, c.cls = CASES[shape]
        bk, mk = SHAPES[shape]
        sb = synth.make_batch(**dict(bk, num_graphs=graphs))
        c.params = _rand_params(bk["feat"], int(width or 64), seed=PARAM_SEED, **mk)
        c.x, c.ei, c.batch, c.B = sb.x, sb.edge_index, sb.batch, sb.num_graphs
        c.max_nodes, c.max_edges = sb.max_nodes, sb.max_edges

        def redraw(x, m):
            x[m] = torch.randn(int(m.sum()), x.shape[1], generator=gen)
    print(f"\n  case {name} {method}: B {c.B} N {c.x.shape[0]} E {c.ei.shape[1]} max {c.max_nodes} / {c.max_edges} n_steps {c.n_steps}")
    return _finish(c, method, redraw, ties=name == "golden")


def custom(params, x, ei, batch_vec, B, n_steps, cls=0, method="gausslegendre", screen=True, redraw=None):
    """A hand-built case: the reference of x as given (`screen=False`: exact-zero and shape checks, which no branch decision
    touches), or of x after the screen with the case's own `redraw(x, node mask of the flagged graphs)`."""
    from hcatgnet_amd.attribution import quadrature
    c = Case()
    c.params, c.x, c.ei, c.batch, c.B, c.n_steps, c.cls, c.method = params, x, ei, batch_vec, B, n_steps, cls, method
    c.max_nodes = int(torch.bincount(batch_vec, minlength=B).max())
    c.edge_owner = batch_vec[ei[1]]
    c.max_edges = int(torch.bincount(c.edge_owner, minlength=B).max()) if ei.shape[1] else 0
    c.alpha, c.weight = quadrature(method, n_steps)
    if screen:
        c.x, c.ref = decidable(params, x, ei, batch_vec, B, c.alpha, c.weight, cls, redraw)
    else:
        c.ref = reference(params, x, ei, batch_vec, B, c.alpha, c.weight, cls, screen=False)
    return c


def figures(c, r, ref=None):
    """per-graph rel_inf of both attributions, out_full / out_base with floor 1.0"""
    ref = c.ref if ref is None else ref
    return dict(node=_per_graph(r.node_attr, ref["node"], c.batch, c.B), edge=_per_graph(r.edge_attr, ref["edge"], c.edge_owner, c.B),
                out_full=rel_inf(r.out_full.detach().double().cpu(), ref["out_full"], floor=1.0),
                out_base=rel_inf(r.out_base.detach().double().cpu(), ref["out_base"], floor=1.0))


def check(c, r, tag, ref=None):
    fig = figures(c, r, ref)
    print(f"    {tag} (per graph): " + "  ".join(f"{k} {v:.2e}" for k, v in fig.items()))
    assert tuple(r.node_attr.shape) == tuple(c.x.shape) and tuple(r.edge_attr.shape) == (c.ei.shape[1],)
    assert tuple(r.out_full.shape) == tuple(c.ref["out_full"].shape) == tuple(r.out_base.shape)
    assert all(v <= TOL for v in fig.values()), fig
    return fig


def model(H, c, device="cpu", **opt):
    O = _oracle()
    n_conv, n_read = O.infer_depths(c.params)
    D, F = c.params["conv1.lin.weight"].shape
    o = H.default_options(n_convolutions=n_conv, readout_layers=n_read, embedding_dim=D,
                          n_classes=c.params[f"readout.{n_read - 1}.weight"].shape[0], **opt)
    m = H.make_network("GCN", o, F)
    m.load_state_dict(c.params)
    return m.to(device)


def batch(H, c, device="cpu", **kw):
    meta = dict(max_nodes=c.max_nodes, max_edges=c.max_edges, edges_grouped=True)
    meta.update(kw)
    return H.Batch(c.x.to(device), c.ei.to(device), c.batch.to(device), c.B, **meta)
