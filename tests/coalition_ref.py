"""The fp64 references of `CoalitionValues` and the checks both coalition test files share (tests only).

All from the oracle alone, one graph at a time on the CPU, built from the caller's `node_group` / `edge_group` (none of the
package's lists, none of its derivation functions):
    table        `oracle.gcn_forward(..., edge_mask=)` per subset, as `shapley_groups_ref._graph_fwd` masks a subset
    Shapley      `shapley_groups_ref.exact_graph` (the subset formula)
    interaction  I_ij = sum over S within the others of |S|! (G - |S| - 2)! / (G - 1)! (v(S+i+j) - v(S+i) - v(S+j) + v(S)),
                 written with itertools

Bounds, per graph, TOL = 1e-5 (tests/shapley_ref.py), scale = max(1, max |v_ref|) over the graph's table:
    values       |v - v_ref| <= TOL scale            elementwise (the bound the Shapley tests put on out_full / out_base)
    group_attr   |phi - phi_ref| <= 2 TOL scale      (the weights sum to 1, each term has two table values)
    interaction  |I - I_ref| <= 4 TOL scale          (the same with four table values)
    efficiency   |sum_y phi_y - (out_full[c] - out_base[c])| <= 2 TOL scale_c + 2^-23 S   (shapley_groups_ref's: scale_c and S
                 of `exact_graph`, over column c)
Every figure is printed before it is asserted (`pytest -s`)."""
import itertools
import math

import torch

from tests import shapley_groups_ref as GR
from tests.shapley_ref import TOL, pointers

X_SEED = 5


def table_graph(params64, x, ei_local, ng, eg, G):
    """float64 [2^G, C]: row s = the oracle's output with the background and the groups {y : bit y of s} on"""
    fwd = GR._graph_fwd(params64, x, ei_local, ng, eg)
    return torch.stack([fwd({y for y in range(G) if (s >> y) & 1}) for s in range(1 << G)])


def interactions_graph(v, G):
    """float64 [G, G] from one column `v` [2^G] of a table"""
    out = torch.zeros(G, G, dtype=torch.float64)
    for i, j in itertools.combinations(range(G), 2):
        others = [y for y in range(G) if y not in (i, j)]
        acc = 0.0
        for r in range(len(others) + 1):
            w = math.factorial(r) * math.factorial(G - r - 2) / math.factorial(G - 1)
            for sub in itertools.combinations(others, r):
                s = sum(1 << y for y in sub)
                acc += w * float(v[s | 1 << i | 1 << j] - v[s | 1 << i] - v[s | 1 << j] + v[s])
        out[i, j] = out[j, i] = acc
    return out


def shapley_graph(v, G):
    """float64 [G]: the subset formula on one column of a table (for tables that are not the oracle's)"""
    phi = torch.zeros(G, dtype=torch.float64)
    for y in range(G):
        others = [k for k in range(G) if k != y]
        for r in range(G):
            w = math.factorial(r) * math.factorial(G - r - 1) / math.factorial(G)
            for sub in itertools.combinations(others, r):
                s = sum(1 << k for k in sub)
                phi[y] += w * float(v[s | 1 << y] - v[s])
    return phi


def reference_batch(params, x, ei, batch_vec, B, node_group, edge_group, cls, graphs=None):
    """-> (list over the graphs of dict(table [2^G, C], phi [G], inter [G, G], scale, eff_bound, live [G]), gptr)"""
    p64 = {k: v.double() for k, v in params.items()}
    nptr, eptr = pointers(batch_vec, ei, B)
    N, F = x.shape
    ng, eg = GR.normalise(node_group, edge_group, N, F, ei.shape[1])
    gptr = GR.group_pointers(ng, eg, batch_vec, ei, B)
    refs = []
    for g in range(B):
        if graphs is not None and g not in graphs:
            refs.append(None)
            continue
        a, b, ea, eb = int(nptr[g]), int(nptr[g + 1]), int(eptr[g]), int(eptr[g + 1])
        G = int(gptr[g + 1] - gptr[g])
        part = (x[a:b], ei[:, ea:eb] - a, ng[a:b], eg[ea:eb])
        table = table_graph(p64, *part, G)
        ex = GR.exact_graph(p64, *part, G, cls)
        refs.append(dict(table=table, phi=ex["phi"], inter=interactions_graph(table[:, cls], G), live=ex["live"],
                         scale=max(1.0, float(table.abs().max())),
                         eff_bound=2 * TOL * max(1.0, ex["vmax"]) + 2.0 ** -23 * ex["S"]))
    return refs, gptr


def check_layout(r, gptr, C):
    B = gptr.numel() - 1
    cnt = gptr[1:] - gptr[:-1]
    tptr = torch.zeros(B + 1, dtype=torch.long); tptr[1:] = (2 ** cnt).cumsum(0)
    pptr = torch.zeros(B + 1, dtype=torch.long); pptr[1:] = (cnt * cnt).cumsum(0)
    assert r.table_ptr.dtype == r.group_ptr.dtype == r.pair_ptr.dtype == torch.int64
    assert torch.equal(r.table_ptr.cpu(), tptr) and torch.equal(r.group_ptr.cpu(), gptr) and torch.equal(r.pair_ptr.cpu(), pptr)
    assert tuple(r.values.shape) == (int(tptr[-1]), C) and r.values.dtype == torch.float32
    assert tuple(r.group_attr.shape) == (int(gptr[-1]),) and tuple(r.interaction.shape) == (int(pptr[-1]),)
    assert tuple(r.out_full.shape) == (B, C) and tuple(r.out_base.shape) == (B, C)
    v = r.values
    if B:
        assert torch.equal(r.out_base, v[r.table_ptr[:-1]]) and torch.equal(r.out_full, v[r.table_ptr[1:] - 1])
    return tptr, pptr


def check_against_reference(r, refs, gptr, cls, tag=""):
    """The bounds of the module docstring for every graph with a reference, and the result's layout"""
    C = next(q for q in refs if q is not None)["table"].shape[1]
    tptr, pptr = check_layout(r, gptr, C)
    values, attr, inter = r.values.detach().double().cpu(), r.group_attr.detach().double().cpu(), r.interaction.detach().double().cpu()
    worst = dict(values=0.0, attr=0.0, inter=0.0, eff=0.0)
    fails = []
    for g, ref in enumerate(refs):
        if ref is None:
            continue
        G = int(gptr[g + 1] - gptr[g])
        scale = ref["scale"]
        v = values[int(tptr[g]):int(tptr[g + 1])]
        phi = attr[int(gptr[g]):int(gptr[g + 1])]
        I = inter[int(pptr[g]):int(pptr[g + 1])].view(G, G)
        e_v = float((v - ref["table"]).abs().max())
        e_a = float((phi - ref["phi"]).abs().max()) if G else 0.0
        e_i = float((I - ref["inter"]).abs().max()) if G else 0.0
        eff = abs(float(phi.sum()) - float(v[-1, cls] - v[0, cls]))
        worst["values"] = max(worst["values"], e_v / (TOL * scale))
        worst["attr"] = max(worst["attr"], e_a / (2 * TOL * scale))
        worst["inter"] = max(worst["inter"], e_i / (4 * TOL * scale))
        worst["eff"] = max(worst["eff"], eff / ref["eff_bound"])
        if e_v > TOL * scale or e_a > 2 * TOL * scale or e_i > 4 * TOL * scale or eff > ref["eff_bound"]:
            fails.append((g, e_v, e_a, e_i, scale, eff, ref["eff_bound"]))
        assert torch.equal(I, I.t()) and float(I.diagonal().abs().sum()) == 0.0, (g, "symmetric, 0 on the diagonal")
        dead = ~ref["live"]
        assert bool((phi[dead] == 0).all()) and bool((I[dead] == 0).all()), (g, "a dead group gets exactly 0")
    print(f"    {tag}: worst figure / bound over {sum(q is not None for q in refs)} graphs of {len(refs)}: "
          + "  ".join(f"{k} {v:.3f}" for k, v in worst.items()))
    assert not fails, fails


def check_dead_rows(r, refs, gptr):
    """rows that differ only in a dead group are the same row -> the number of pairs compared"""
    pairs = 0
    for g, ref in enumerate(refs):
        a = int(r.table_ptr[g])
        for y in (~ref["live"]).nonzero().flatten().tolist():
            for s in range(1 << int(gptr[g + 1] - gptr[g])):
                if not (s >> y) & 1:
                    assert torch.equal(r.values[a + s], r.values[a + (s | 1 << y)]), (g, y, s)
                    pairs += 1
    return pairs


# ------------------------------------------------------------------------------------------------ the cases both files use
class Case:
    pass


def sparse_x(x, share):
    return (x * (torch.rand(x.shape, generator=torch.Generator().manual_seed(X_SEED)) < share)).contiguous()


def local_index(batch_vec, B):
    nptr = torch.zeros(B + 1, dtype=torch.long)
    nptr[1:] = torch.bincount(batch_vec, minlength=B).cumsum(0)
    return torch.arange(batch_vec.numel()) - nptr[batch_vec], (nptr[1:] - nptr[:-1])[batch_vec], nptr


def fragments(batch_vec, B, k):
    """[N] int64: `k` contiguous node ranges per graph"""
    loc, n, _ = local_index(batch_vec, B)
    return loc * k // n


def mixed_case():
    """Four graphs of 17-23 nodes with 0, 1, 3 and 5 groups: [N]-style node groups, one node whose entries are split between a
    group and the background, edge groups, background nodes and edges, and one group (graph 3's group 4) without a live
    member.  -> Case(x, ei, batch, B, F, max_nodes, max_edges, ng [N, F], eg [E], dead (graph, group))"""
    from hcatgnet_amd import synth
    sb = synth.make_batch(num_graphs=4, nodes=20, extra_bonds=3, max_degree=4, feat=25, nodes_jitter=3)
    c = Case()
    c.ei, c.batch, c.B, c.F = sb.edge_index, sb.batch, sb.num_graphs, 25
    c.max_nodes, c.max_edges = sb.max_nodes, sb.max_edges
    x = sparse_x(sb.x, 0.3)
    N, E = x.shape[0], c.ei.shape[1]
    loc, n, nptr = local_index(c.batch, c.B)
    third = loc * 3 // n
    node = torch.full((N,), -1, dtype=torch.int64)
    egraph = c.batch[c.ei[1]]
    eg = torch.full((E,), -1, dtype=torch.int64)
    node[(c.batch == 1) & (loc * 2 < n)] = 0                              # graph 1: one group, the first half of its atoms
    m2 = c.batch == 2                                                     # graph 2: two thirds of the atoms, and a group of edges
    node[m2 & (third < 2)] = third[m2 & (third < 2)]
    eg[(egraph == 2) & (third[c.ei[1]] == 0)] = 2
    m3 = c.batch == 3                                                     # graph 3: three fragments, every edge, one dead atom
    node[m3] = third[m3]
    eg[egraph == 3] = 3
    dead_atom = int(nptr[3]) + 1
    node[dead_atom] = 4
    x[dead_atom] = 0
    ng = node.unsqueeze(1).expand(N, c.F).clone()
    split = int(nptr[2]) + int(n[int(nptr[2])]) // 3 + 1                  # an atom of graph 2's group 1: half its entries stay behind
    assert int(node[split]) == 1
    ng[split, 12:] = -1
    x[split, 3], x[split, 20] = 0.5, -0.25                                # (both halves have a live entry)
    c.x, c.ng, c.eg, c.dead = x.contiguous(), ng, eg, (3, 4)
    return c
