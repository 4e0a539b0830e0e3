"""The fp64 reference of grouped Shapley value sampling and the checks both grouped test files share (tests only).

Reference: `oracle.gcn_forward(..., edge_mask=)` in fp64 on the CPU, one graph at a time, walked group by group with the
same permutations -- never the GPU path, never the code under test, and built from the caller's `node_group` /
`edge_group` alone (none of the package's lists).  The background (id -1) is on in every evaluation; a group without a live
member (a node entry with x != 0, or an edge that is not an explicit (i, i)) is switched on without an evaluation and gets
exactly 0.  `exact_graph` is the subset formula
    phi_y = sum over S of |S|! (G - |S| - 1)! / G! (v(S + y) - v(S))
over all 2^G subsets, the value the mean over all G! orders must equal.

Bounds (the project's own, tests/shapley_ref.py; TOL = 1e-5):
    per graph   |phi - phi_ref| <= 2 TOL max(1, max |v_ref|)   elementwise over the graph's groups
    out_full, out_base: rel_inf with floor 1.0 <= TOL
    efficiency  |sum(group_attr) - (out_full[c] - out_base[c])| <= 2 TOL scale + 2^-23 S,  S = the reference's mean over
                the permutations of sum_k |v_k - v_(k-1)|, scale as above
Every figure is printed before it is asserted (`pytest -s`)."""
import itertools
import math

import torch

from tests.helpers import rel_inf
from tests.shapley_ref import TOL, oracle_mod, pointers


def normalise(node_group, edge_group, N, F, E):
    """-> (ng [N, F] int64, eg [E] int64) with -1 where an array is not given"""
    if node_group is None:
        ng = torch.full((N, F), -1, dtype=torch.int64)
    else:
        ng = node_group.cpu().to(torch.int64)
        ng = ng.unsqueeze(1).expand(N, F).clone() if ng.dim() == 1 else ng.clone()
    eg = torch.full((E,), -1, dtype=torch.int64) if edge_group is None else edge_group.cpu().to(torch.int64).clone()
    return ng, eg


def group_pointers(ng, eg, batch_vec, ei, B):
    """[B + 1]: prefix sum of G_g = the graph's largest id + 1"""
    nptr, eptr = pointers(batch_vec, ei, B)
    gptr = torch.zeros(B + 1, dtype=torch.long)
    for g in range(B):
        ids = torch.cat([ng[int(nptr[g]):int(nptr[g + 1])].reshape(-1), eg[int(eptr[g]):int(eptr[g + 1])], torch.tensor([-1])])
        gptr[g + 1] = gptr[g] + int(ids.max()) + 1
    return gptr


def check_group_permutations(perm, gptr):
    perm = perm.cpu()
    assert perm.dtype == torch.int32 and perm.shape[1] == int(gptr[-1])
    for g in range(len(gptr) - 1):
        a, b = int(gptr[g]), int(gptr[g + 1])
        want = torch.arange(b - a, dtype=torch.int32)
        for p in range(perm.shape[0]):
            assert torch.equal(perm[p, a:b].sort().values, want), (g, p)


def _graph_fwd(params64, x, ei_local, ng, eg):
    O = oracle_mod()
    x64 = x.double()

    def fwd(on):
        """on: set of group ids switched on (the background always is)"""
        nm = torch.zeros_like(ng, dtype=torch.float64)
        em = torch.zeros(eg.shape[0], dtype=torch.float64)
        nm[ng < 0] = 1.0
        em[eg < 0] = 1.0
        for y in on:
            nm[ng == y] = 1.0
            em[eg == y] = 1.0
        return O.gcn_forward(params64, x64 * nm, ei_local, None, 1, edge_mask=em)[0][0]
    return fwd


def live_groups(x, ei_local, ng, eg, G):
    live = torch.zeros(G, dtype=torch.bool)
    m = (x != 0) & (ng >= 0)
    live[ng[m]] = True
    m = (ei_local[0] != ei_local[1]) & (eg >= 0)
    live[eg[m]] = True
    return live


def reference_graph(params64, x, ei_local, ng, eg, perm_rows, cls):
    """One graph: x [n, F] f32, ei_local [2, e], ng [n, F], eg [e], perm_rows [P, G] -> dict(phi [G] f64 mean attribution,
    vmax, S, full [C], base [C], live [G]) from the fp64 oracle walked group by group."""
    G = perm_rows.shape[1]
    fwd = _graph_fwd(params64, x, ei_local, ng, eg)
    live = live_groups(x, ei_local, ng, eg, G)
    P = perm_rows.shape[0]
    phi = torch.zeros(G, dtype=torch.float64)
    vmax, S = 0.0, 0.0
    full = base = None
    for p in range(P):
        on = set()
        out = fwd(on)
        if p == 0:
            base = out.clone()
        vprev = float(out[cls])
        vmax = max(vmax, abs(vprev))
        one = torch.zeros_like(phi)
        for y in perm_rows[p].tolist():
            on.add(y)
            if not bool(live[y]):
                continue                           # bit-identical input: v_k = v_(k-1) exactly
            out = fwd(on)
            v = float(out[cls])
            one[y] = v - vprev
            S += abs(v - vprev)
            vmax = max(vmax, abs(v))
            vprev = v
        if p == 0:
            full = out.clone()
        phi += one
    return dict(phi=phi / P, vmax=vmax, S=S / P, full=full, base=base, live=live)


def exact_graph(params64, x, ei_local, ng, eg, G, cls):
    """The subset formula over all 2^G subsets in fp64 -> the same dict as `reference_graph` (S: sum_y sum_S w |dv|)."""
    fwd = _graph_fwd(params64, x, ei_local, ng, eg)
    val = {}
    for r in range(G + 1):
        for sub in itertools.combinations(range(G), r):
            val[frozenset(sub)] = fwd(set(sub))
    phi = torch.zeros(G, dtype=torch.float64)
    S = 0.0
    for y in range(G):
        for sub, out in val.items():
            if y in sub:
                continue
            w = math.factorial(len(sub)) * math.factorial(G - len(sub) - 1) / math.factorial(G)
            d = float(val[sub | {y}][cls]) - float(out[cls])
            phi[y] += w * d
            S += w * abs(d)
    vmax = max(abs(float(o[cls])) for o in val.values())
    return dict(phi=phi, vmax=vmax, S=S, full=val[frozenset(range(G))], base=val[frozenset()],
                live=live_groups(x, ei_local, ng, eg, G))


def reference_batch(params, x, ei, batch_vec, B, node_group, edge_group, perm, cls, graphs=None, exact=False):
    """-> (list over the graphs (None for those not in `graphs`) of reference dicts, gptr, ng, eg).  `exact`: the subset
    formula instead of the walk (`perm` is not used)."""
    p64 = {k: v.double() for k, v in params.items()}
    nptr, eptr = pointers(batch_vec, ei, B)
    N, F = x.shape
    ng, eg = normalise(node_group, edge_group, N, F, ei.shape[1])
    gptr = group_pointers(ng, eg, batch_vec, ei, B)
    perm = None if perm is None else perm.cpu().long()
    refs = []
    for g in range(B):
        if graphs is not None and g not in graphs:
            refs.append(None)
            continue
        a, b, ea, eb = int(nptr[g]), int(nptr[g + 1]), int(eptr[g]), int(eptr[g + 1])
        ga, gb = int(gptr[g]), int(gptr[g + 1])
        if exact:
            refs.append(exact_graph(p64, x[a:b], ei[:, ea:eb] - a, ng[a:b], eg[ea:eb], gb - ga, cls))
        else:
            refs.append(reference_graph(p64, x[a:b], ei[:, ea:eb] - a, ng[a:b], eg[ea:eb], perm[:, ga:gb], cls))
    return refs, gptr, ng, eg


def check_against_reference(r, refs, gptr, ng, eg, cls, tag="", node_graph=None, edge_graph=None):
    """The bounds of the module docstring for every graph with a reference, the result's layout, and node_attr / edge_attr
    as a gather of group_attr (when the graphs of the nodes and edges are given); prints the worst figures first."""
    B = len(refs)
    grp = r.group_attr.detach().cpu()
    assert tuple(grp.shape) == (int(gptr[-1]),) and torch.equal(r.group_ptr.cpu().long(), gptr)
    assert tuple(r.node_attr.shape) == tuple(ng.shape) and tuple(r.edge_attr.shape) == tuple(eg.shape)
    full, base = r.out_full.detach().double().cpu(), r.out_base.detach().double().cpu()
    worst = dict(attr=0.0, eff=0.0, full=0.0, base=0.0)
    fails = []
    for g, ref in enumerate(refs):
        if ref is None:
            continue
        got = grp[int(gptr[g]):int(gptr[g + 1])].double()
        scale = max(1.0, ref["vmax"])
        err = float((got - ref["phi"]).abs().max()) if got.numel() else 0.0
        eff = abs(float(got.sum()) - float(full[g, cls] - base[g, cls]))
        eff_bound = 2 * TOL * scale + 2.0 ** -23 * ref["S"]
        f_full = rel_inf(full[g], ref["full"], floor=1.0)
        f_base = rel_inf(base[g], ref["base"], floor=1.0)
        worst["attr"] = max(worst["attr"], err / (2 * TOL * scale))
        worst["eff"] = max(worst["eff"], eff / eff_bound)
        worst["full"] = max(worst["full"], f_full / TOL)
        worst["base"] = max(worst["base"], f_base / TOL)
        if err > 2 * TOL * scale or eff > eff_bound or f_full > TOL or f_base > TOL:
            fails.append((g, err, 2 * TOL * scale, eff, eff_bound, f_full, f_base))
        dead = ~ref["live"]
        assert bool((got[dead] == 0).all()), (g, "a group without a live member must get exactly 0")
    print(f"    {tag}: worst figure / bound over {sum(q is not None for q in refs)} graphs of {B}: "
          + "  ".join(f"{k} {v:.3f}" for k, v in worst.items()))
    assert not fails, fails
    if node_graph is not None:
        check_gather(r, gptr, ng, eg, node_graph, edge_graph)


def check_gather(r, gptr, ng, eg, node_graph, edge_graph):
    """Captum's convention: every member carries its group's value, the background 0.  node_graph [N] / edge_graph [E]:
    the graph of every node and edge."""
    grp = r.group_attr.detach().cpu()
    pad = torch.cat([grp, grp.new_zeros(1)])
    G = grp.numel()
    want_n = pad[torch.where(ng >= 0, gptr[node_graph].unsqueeze(1) + ng, G)]
    want_e = pad[torch.where(eg >= 0, gptr[edge_graph] + eg, G)]
    assert torch.equal(r.node_attr.detach().cpu(), want_n) and torch.equal(r.edge_attr.detach().cpu(), want_e)
