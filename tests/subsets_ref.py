"""The fp64 references of `SubsetValues` / `AttributionCurves` and the checks both subset test files share (tests only).

All from the oracle alone, one graph at a time on the CPU, built from the caller's `node_group` / `edge_group` (none of the
package's lists, none of its bit packing):
    values   `shapley_groups_ref._graph_fwd(params64, x, ei_local, ng, eg)(set of groups)` per row and graph
    curves   the same forward on the prefixes of an order and on their complements, plain Python loops
    AUC      the trapezoid rule over x = k / G_g, a plain Python loop in float
    packing  Python ints

Bounds (the project's own; TOL = 1e-5 from tests/shapley_ref.py), per graph, scale = max(1, max |v_ref|) over the graph's rows:
    values, curve points   |v - v_ref| <= TOL scale   elementwise
    AUC                    |a - a_ref| <= TOL scale + 2^-23 scale   (a convex combination of bounded points, and one float32 rounding)
The forward is continuous across LeakyReLU kinks and max-pool ties, so no input is screened.
Every figure is printed before it is asserted (`pytest -s`)."""
import math

import torch

from tests import shapley_groups_ref as GR
from tests.shapley_ref import TOL, pointers


class Case:
    pass


def join(parts):
    """One batch out of single synth batches (the graphs keep their own seeds' edges and features)"""
    c = Case()
    xs, eis, bs, off, g0 = [], [], [], 0, 0
    for sb in parts:
        xs.append(sb.x)
        eis.append(sb.edge_index + off)
        bs.append(sb.batch + g0)
        off += sb.x.shape[0]
        g0 += sb.num_graphs
    c.x, c.ei, c.batch, c.B = torch.cat(xs).contiguous(), torch.cat(eis, 1).contiguous(), torch.cat(bs), g0
    c.max_nodes, c.max_edges = max(sb.max_nodes for sb in parts), max(sb.max_edges for sb in parts)
    c.F = c.x.shape[1]
    return c


def sized_case(sizes, feat=25, extra_bonds=3, max_degree=4):
    """Graphs of exactly `sizes` nodes, one `synth.make_batch` graph each (its default seed)"""
    from hcatgnet_amd import synth
    return join([synth.make_batch(num_graphs=1, nodes=n, extra_bonds=extra_bonds, max_degree=max_degree, feat=feat) for n in sizes])


def random_rows(S, G, seed):
    """bool [S, G]: all off, all on, then S - 2 seeded random rows"""
    rows = torch.rand(S, G, generator=torch.Generator().manual_seed(seed)) < 0.5
    rows[0], rows[1] = False, True
    return rows


# ------------------------------------------------------------------------------------------------ references
class Forwards:
    """The oracle's forward of every graph of a batch, by set of groups (cached: a curve and a row list share subsets)"""

    def __init__(self, params, x, ei, batch_vec, B, node_group, edge_group):
        p64 = {k: v.double() for k, v in params.items()}
        nptr, eptr = pointers(batch_vec, ei, B)
        N, F = x.shape
        ng, eg = GR.normalise(node_group, edge_group, N, F, ei.shape[1])
        self.gptr = GR.group_pointers(ng, eg, batch_vec, ei, B)
        self.B, self.fwd, self.live, self.cache = B, [], [], {}
        for g in range(B):
            a, b, ea, eb = int(nptr[g]), int(nptr[g + 1]), int(eptr[g]), int(eptr[g + 1])
            part = (x[a:b], ei[:, ea:eb] - a, ng[a:b], eg[ea:eb])
            self.fwd.append(GR._graph_fwd(p64, *part))
            self.live.append(GR.live_groups(*part, self.count(g)))

    def count(self, g):
        return int(self.gptr[g + 1] - self.gptr[g])

    def __call__(self, g, on):
        key = (g, frozenset(on))
        if key not in self.cache:
            self.cache[key] = self.fwd[g](set(on))
        return self.cache[key]


def values_ref(fw, rows):
    """rows bool [S, G] -> list over the graphs of float64 [S, C]"""
    out = []
    for g in range(fw.B):
        a, G = int(fw.gptr[g]), fw.count(g)
        out.append(torch.stack([fw(g, [y for y in range(G) if bool(rows[s, a + y])]) for s in range(rows.shape[0])])
                   if rows.shape[0] else None)
    return out


def points_ref(G, fractions):
    return list(range(G + 1)) if fractions is None else [int(math.floor(f * G + 0.5)) for f in fractions]


def trapezoid(ks, vs, G):
    if G == 0:
        return float(vs[0])
    area = 0.0
    for j in range(len(ks) - 1):
        area += (ks[j + 1] / G - ks[j] / G) * (float(vs[j]) + float(vs[j + 1])) / 2
    return area


def curves_ref(fw, order, cls, fractions=None):
    """order: [G] ints, graph g's segment a permutation of its local ids -> list over the graphs of dict(k, ins [P, C],
    del [P, C], ins_auc, del_auc, scale)"""
    order = [int(v) for v in order]
    out = []
    for g in range(fw.B):
        a, G = int(fw.gptr[g]), fw.count(g)
        seg = order[a:a + G]
        ks = points_ref(G, fractions)
        ins = torch.stack([fw(g, seg[:k]) for k in ks])
        dele = torch.stack([fw(g, seg[k:]) for k in ks])
        out.append(dict(k=ks, ins=ins, dele=dele, ins_auc=trapezoid(ks, ins[:, cls], G), del_auc=trapezoid(ks, dele[:, cls], G),
                        scale=max(1.0, float(ins.abs().max()), float(dele.abs().max()))))
    return out


def pack_ref(rows, gptr):
    """rows: bool [S, G] -> (list over the rows of lists of W Python ints in [0, 2^32), word_ptr list [B + 1])"""
    B = len(gptr) - 1
    wptr = [0]
    for g in range(B):
        wptr.append(wptr[-1] + (int(gptr[g + 1]) - int(gptr[g]) + 31) // 32)
    words = []
    for s in range(rows.shape[0]):
        row = [0] * wptr[-1]
        for g in range(B):
            for y in range(int(gptr[g + 1]) - int(gptr[g])):
                if bool(rows[s, int(gptr[g]) + y]):
                    row[wptr[g] + (y >> 5)] |= 1 << (y & 31)
        words.append(row)
    return words, wptr


# ------------------------------------------------------------------------------------------------ checks
def check_values(r, refs, fw, tag=""):
    """`SubsetResult` against `values_ref` (and out_full / out_base against the all-on / all-off forwards)"""
    B = fw.B
    assert torch.equal(r.group_ptr.cpu().long(), fw.gptr) and r.group_ptr.dtype == torch.int64
    values, full, base = r.values.detach().double().cpu(), r.out_full.detach().double().cpu(), r.out_base.detach().double().cpu()
    assert r.values.dtype == torch.float32 and values.shape[1] == B and tuple(full.shape) == tuple(base.shape) == (B, values.shape[2])
    worst, fails = 0.0, []
    for g in range(B):
        ref_full, ref_base = fw(g, range(fw.count(g))), fw(g, [])
        ref = [ref_full.unsqueeze(0), ref_base.unsqueeze(0)] + ([refs[g]] if refs[g] is not None else [])
        got = [full[g].unsqueeze(0), base[g].unsqueeze(0)] + ([values[:, g]] if refs[g] is not None else [])
        ref, got = torch.cat(ref), torch.cat(got)
        scale = max(1.0, float(ref.abs().max()))
        err = float((got - ref).abs().max())
        worst = max(worst, err / (TOL * scale))
        if err > TOL * scale:
            fails.append((g, err, TOL * scale))
    print(f"    {tag}: values, worst figure / bound over {B} graphs and {values.shape[0]} rows: {worst:.4f}")
    assert not fails, fails


def check_curves(r, refs, fw, cls, tag=""):
    """`CurveResult` against `curves_ref`: the points picked, both curves, both areas"""
    cptr = r.curve_ptr.cpu().tolist()
    assert r.k.dtype == torch.int64 and r.curve_ptr.dtype == torch.int64 and torch.equal(r.group_ptr.cpu().long(), fw.gptr)
    assert r.insertion_auc.dtype == r.deletion_auc.dtype == torch.float32
    ks = r.k.cpu().tolist()
    worst, fails = dict(points=0.0, auc=0.0), []
    for g, ref in enumerate(refs):
        a, b = cptr[g], cptr[g + 1]
        assert ks[a:b] == ref["k"], (g, ks[a:b], ref["k"])
        scale = ref["scale"]
        e_p = max(float((r.insertion[a:b].double().cpu() - ref["ins"]).abs().max()), float((r.deletion[a:b].double().cpu() - ref["dele"]).abs().max()))
        e_a = max(abs(float(r.insertion_auc[g]) - ref["ins_auc"]), abs(float(r.deletion_auc[g]) - ref["del_auc"]))
        bound_a = TOL * scale + 2.0 ** -23 * scale
        worst["points"] = max(worst["points"], e_p / (TOL * scale))
        worst["auc"] = max(worst["auc"], e_a / bound_a)
        if e_p > TOL * scale or e_a > bound_a:
            fails.append((g, e_p, TOL * scale, e_a, bound_a))
    assert cptr[-1] == r.insertion.shape[0] == r.deletion.shape[0] == len(ks)
    print(f"    {tag}: curves, worst figure / bound over {len(refs)} graphs: " + "  ".join(f"{k} {v:.4f}" for k, v in worst.items()))
    assert not fails, fails
