"""The fp64 reference of Shapley value sampling and the checks both Shapley test files share (tests only).

Reference: `oracle.gcn_forward(..., edge_mask=)` in fp64 on the CPU, one graph at a time, walked step by step with the
same permutations -- never the GPU path, never the code under test.  A node entry whose x is exactly 0 leaves the
reference's input bit-identical, so v_k = v_(k-1) holds exactly there and the reference does not evaluate that step again;
every other step (explicit self-loop edges included) is a forward of its own.

Bounds (TOL = 1e-5, the project's output tolerance); an attribution is a difference of two outputs:
    per graph   |phi - phi_ref| <= 2 TOL max(1, max_k |v_k,ref|)   elementwise over the graph's node and edge attributions
    out_full, out_base: rel_inf with floor 1.0 <= TOL
    efficiency  |sum(phi) - (out_full[c] - out_base[c])| <= 2 TOL scale + 2^-23 S,  S = the reference's mean over the
                permutations of sum_k |v_k - v_(k-1)|, scale as above
Every figure is printed before it is asserted (`pytest -s`)."""
import torch

from tests.helpers import rel_inf

TOL = 1e-5


def oracle_mod():
    from oracle import gcn_oracle
    return gcn_oracle


def rand_params(F, D, n_conv=2, n_read=2, n_classes=1, seed=0):
    g = torch.Generator().manual_seed(seed)
    p = {}

    def glorot(o, i):
        a = (6.0 / (i + o)) ** 0.5
        return (torch.rand(o, i, generator=g) * 2 - 1) * a
    p["conv1.lin.weight"] = glorot(D, F); p["conv1.bias"] = torch.randn(D, generator=g) * 0.1
    for i in range(n_conv - 1):
        p[f"conv_layers.{i}.lin.weight"] = glorot(D, D); p[f"conv_layers.{i}.bias"] = torch.randn(D, generator=g) * 0.1
    dim = 2 * D
    for i in range(n_read - 1):
        p[f"readout.{i}.0.weight"] = glorot(dim // 2, dim); p[f"readout.{i}.0.bias"] = torch.randn(dim // 2, generator=g) * 0.1
        dim //= 2
    p[f"readout.{n_read - 1}.weight"] = glorot(n_classes, dim); p[f"readout.{n_read - 1}.bias"] = torch.randn(n_classes, generator=g) * 0.1
    return p


def model_from_params(H, params, **opt_kw):
    O = oracle_mod()
    n_conv, n_read = O.infer_depths(params)
    D, F = params["conv1.lin.weight"].shape
    opt = H.default_options(n_convolutions=n_conv, readout_layers=n_read, embedding_dim=D,
                            n_classes=params[f"readout.{n_read - 1}.weight"].shape[0], **opt_kw)
    m = H.make_network("GCN", opt, F)
    m.load_state_dict(params)
    return m


def pointers(batch_vec, ei, B):
    nptr = torch.zeros(B + 1, dtype=torch.long); nptr[1:] = torch.bincount(batch_vec, minlength=B).cumsum(0)
    eptr = torch.zeros(B + 1, dtype=torch.long); eptr[1:] = torch.bincount(batch_vec[ei[1]], minlength=B).cumsum(0)
    return nptr, eptr


def check_permutations(perm, nptr, eptr, F):
    """every graph segment of every row is a permutation of 0 .. K_g - 1 at offset graph_ptr * F + edge_ptr"""
    perm = perm.cpu()
    assert perm.dtype == torch.int32 and perm.shape[1] == int(nptr[-1]) * F + int(eptr[-1])
    for g in range(len(nptr) - 1):
        K = int(nptr[g + 1] - nptr[g]) * F + int(eptr[g + 1] - eptr[g])
        s = int(nptr[g]) * F + int(eptr[g])
        want = torch.arange(K, dtype=torch.int32)
        for p in range(perm.shape[0]):
            assert torch.equal(perm[p, s:s + K].sort().values, want), (g, p)


def reference_graph(params64, x, ei_local, perm_rows, cls):
    """One graph: x [n, F] f32, ei_local [2, e], perm_rows [P, K] -> dict(phi [K] f64 mean attribution, vmax, S, full [C],
    base [C]) from the fp64 oracle walked step by step."""
    O = oracle_mod()
    n, F = x.shape
    e = ei_local.shape[1]
    x64 = x.double()
    P = perm_rows.shape[0]
    phi = torch.zeros(n * F + e, dtype=torch.float64)
    vmax, S = 0.0, 0.0
    full = base = None

    def fwd(nm, em):
        return O.gcn_forward(params64, x64 * nm, ei_local, None, 1, edge_mask=em)[0][0]
    for p in range(P):
        nm = torch.zeros(n, F, dtype=torch.float64)
        em = torch.zeros(e, dtype=torch.float64)
        out = fwd(nm, em)
        if p == 0:
            base = out.clone()
        vprev = float(out[cls])
        vmax = max(vmax, abs(vprev))
        one = torch.zeros_like(phi)
        for j in perm_rows[p].tolist():
            if j < n * F:
                nm.view(-1)[j] = 1.0
                if float(x64.view(-1)[j]) == 0.0:
                    continue                       # bit-identical input: v_k = v_(k-1) exactly
            else:
                em[j - n * F] = 1.0
            out = fwd(nm, em)
            v = float(out[cls])
            one[j] = v - vprev
            S += abs(v - vprev)
            vmax = max(vmax, abs(v))
            vprev = v
        if p == 0:
            full = out.clone()
        phi += one
    return dict(phi=phi / P, vmax=vmax, S=S / P, full=full, base=base)


def reference_batch(params, x, ei, batch_vec, B, perm, cls, graphs=None):
    """-> list over the graphs (None for those not in `graphs`) of `reference_graph` results."""
    p64 = {k: v.double() for k, v in params.items()}
    nptr, eptr = pointers(batch_vec, ei, B)
    F = x.shape[1]
    perm = perm.cpu().long()
    refs = []
    for g in range(B):
        if graphs is not None and g not in graphs:
            refs.append(None)
            continue
        a, b, ea, eb = int(nptr[g]), int(nptr[g + 1]), int(eptr[g]), int(eptr[g + 1])
        s = a * F + ea
        K = (b - a) * F + (eb - ea)
        refs.append(reference_graph(p64, x[a:b], ei[:, ea:eb] - a, perm[:, s:s + K], cls))
    return refs


def check_against_reference(r, refs, x, ei, batch_vec, B, cls, tag=""):
    """The bounds of the module docstring for every graph with a reference; prints the worst figures first."""
    nptr, eptr = pointers(batch_vec, ei, B)
    F = x.shape[1]
    node = r.node_attr.detach().double().cpu()
    edge = r.edge_attr.detach().double().cpu()
    full, base = r.out_full.detach().double().cpu(), r.out_base.detach().double().cpu()
    worst = dict(attr=0.0, eff=0.0, full=0.0, base=0.0)
    fails = []
    for g, ref in enumerate(refs):
        if ref is None:
            continue
        a, b, ea, eb = int(nptr[g]), int(nptr[g + 1]), int(eptr[g]), int(eptr[g + 1])
        got = torch.cat([node[a:b].reshape(-1), edge[ea:eb]])
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
    print(f"    {tag}: worst figure / bound over {sum(q is not None for q in refs)} graphs: "
          + "  ".join(f"{k} {v:.3f}" for k, v in worst.items()))
    assert not fails, fails


def check_exact_zeros(r, x, ei):
    """zero entries of x and explicit self-loop edges get attribution exactly 0.0"""
    node, edge = r.node_attr.detach().cpu(), r.edge_attr.detach().cpu()
    zero = x == 0
    assert bool((node[zero] == 0).all())
    loops = ei[0] == ei[1]
    assert bool((edge[loops] == 0).all())
    return int(zero.sum()), int(loops.sum())
