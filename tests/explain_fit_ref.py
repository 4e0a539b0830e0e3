"""The reference of the `ExplainFit` tests: GNNExplainer as `hcatgnet_amd.explain.ExplainFit` defines it, stated on
`oracle.gcn_forward(..., edge_mask=)` under autograd (fp64 unless asked otherwise), state in and state out.  Never the GPU
path, never the code under test; no torch_geometric.

Definition (published torch_geometric 2.3 / 2.4 `GNNExplainer`, `explanation_type='model'`, `node_mask_type='attributes'`,
`edge_mask_type='object'`, regression, a batch-of-one fit per graph):
  parameters of graph g   edge logits e [E_g], node-feature logits n [N_g, F]
  epoch                   out = model(x * sigmoid(n), edge mask sigmoid(e));  l_g = mean_c (out_gc - target_gc)^2;
                          once the hard masks exist:  + edge_size * sum(m) + edge_ent * mean(ent(m)) over g's hard edges
                                                      + node_feat_size * mean(m) + node_feat_ent * mean(ent(m)) over its hard
                                                        node entries,  ent(m) = -m log(m + EPS) - (1 - m) log(1 - m + EPS)
                          (a term over an empty set is 0);  gradient;  one Adam step on both masks;  after the step of the
                          FIRST epoch (step count 0): hard = (gradient != 0).
  result                  sigmoid(logit), entries that are not hard set to 0.
Adam is torch's rule with lr 0.01, eps 1e-8 and the betas the package's kernels carry: float32(0.9) and float32(0.999), with
1 - beta evaluated in float32 as well (`csrc/common.h` hcg_adam_update; tests/test_gpu_adam.py states the same about
`FusedAdam`) -- B1, ONE_MINUS_B1, B2, ONE_MINUS_B2 below.  Everything else of the rule is evaluated in the run's dtype.
The graphs of a batch are independent: J = sum_g (l_g + regularisers_g) has, on graph g's entries, the gradient a
batch-of-one run on g computes.
"""
import math

import numpy as np
import torch

from oracle import gcn_oracle as O

EPS = 1e-15
COEFFS = dict(edge_size=0.005, edge_ent=1.0, node_feat_size=1.0, node_feat_ent=0.1)
LR, ADAM_EPS = 0.01, 1e-8
B1, B2 = float(np.float32(0.9)), float(np.float32(0.999))
ONE_MINUS_B1, ONE_MINUS_B2 = float(np.float32(1) - np.float32(0.9)), float(np.float32(1) - np.float32(0.999))


def init_state(x, ei, batch, B, generator):
    """n = 0.1 randn(N, F), then e = randn(E) * std_g, std_g = sqrt(2) * sqrt(2 / (2 N_g)) -> a fresh state (float32 values)"""
    N, F = x.shape
    n = 0.1 * torch.randn(N, F, generator=generator)
    nodes = torch.bincount(batch, minlength=B).clamp_min(1).float()
    std = math.sqrt(2.0) * torch.sqrt(2.0 / (2.0 * nodes))
    e = torch.randn(ei.shape[1], generator=generator) * std[batch[ei[1]]]
    return dict(e=e, n=n, e_m=torch.zeros_like(e), e_v=torch.zeros_like(e), n_m=torch.zeros_like(n), n_v=torch.zeros_like(n),
                e_hard=torch.zeros(e.shape, dtype=torch.bool), n_hard=torch.zeros(n.shape, dtype=torch.bool), step=0)


def cast(state, dtype):
    return {k: (v.to(dtype).clone() if torch.is_tensor(v) and v.is_floating_point() else (v.clone() if torch.is_tensor(v) else v))
            for k, v in state.items()}


def _ent(m):
    return -m * torch.log(m + EPS) - (1 - m) * torch.log(1 - m + EPS)


def _per_graph_mean(v, owner, hard, B):
    """sum over the hard entries of each graph / their number (0 for a graph without any) -> ([B], counts [B])"""
    cnt = torch.zeros(B, dtype=v.dtype).index_add_(0, owner[hard], torch.ones(int(hard.sum()), dtype=v.dtype))
    s = torch.zeros(B, dtype=v.dtype).index_add_(0, owner[hard], v[hard])
    return torch.where(cnt > 0, s / cnt.clamp_min(1), torch.zeros_like(s)), cnt


def adam_update(p, g, m, v, step, lr=LR):
    """torch.optim.Adam's update number step + 1 in p's dtype -> (p, m, v)"""
    k = step + 1
    m = B1 * m + ONE_MINUS_B1 * g
    v = B2 * v + ONE_MINUS_B2 * g * g
    bc1, bc2_sqrt = 1.0 - B1 ** k, math.sqrt(1.0 - B2 ** k)
    return p - (lr / bc1) * (m / (v.sqrt() / bc2_sqrt + ADAM_EPS)), m, v


def epoch(params, x, ei, batch, B, target, state, dtype=torch.float64, lr=LR, coeffs=COEFFS, perturb=None):
    """One epoch from `state` -> (state after, info).  info: out [B, C], loss [B], g_e, g_n (the gradients the Adam step
    used, the regularisers included), acts, emb (the masked forward's intermediates, for the decidability screen).
    `perturb(g_e, g_n, live_e, live_n) -> (g_e, g_n)`: applied to the gradients before the step (the hard flags are still
    taken from the unperturbed gradient)."""
    p = {k: v.to(dtype) for k, v in params.items()}
    s = cast(state, dtype)
    e = s["e"].requires_grad_(True)
    n = s["n"].requires_grad_(True)
    eg = batch[ei[1]]
    out, emb, acts = O.gcn_forward(p, x.to(dtype) * torch.sigmoid(n), ei, batch, B, edge_mask=torch.sigmoid(e),
                                   return_intermediates=True)
    loss = ((out - target.to(dtype)) ** 2).mean(dim=1)
    J = loss.sum()
    if s["step"] > 0:
        m = torch.sigmoid(e)
        ent_mean, _ = _per_graph_mean(_ent(m), eg, s["e_hard"], B)
        size = torch.zeros(B, dtype=dtype).index_add_(0, eg[s["e_hard"]], m[s["e_hard"]])
        J = J + (coeffs["edge_size"] * size + coeffs["edge_ent"] * ent_mean).sum()
        m = torch.sigmoid(n)
        owner = batch.unsqueeze(1).expand_as(m)
        ent_mean, _ = _per_graph_mean(_ent(m), owner, s["n_hard"], B)
        m_mean, _ = _per_graph_mean(m, owner, s["n_hard"], B)
        J = J + (coeffs["node_feat_size"] * m_mean + coeffs["node_feat_ent"] * ent_mean).sum()
    J.backward()
    g_e, g_n = e.grad.detach(), n.grad.detach()
    first = s["step"] == 0
    live_e, live_n = (g_e != 0, g_n != 0) if first else (s["e_hard"], s["n_hard"])
    u_e, u_n = (g_e, g_n) if perturb is None else perturb(g_e, g_n, live_e, live_n)
    new = dict(s)
    new["e"], new["e_m"], new["e_v"] = adam_update(e.detach(), u_e, s["e_m"], s["e_v"], s["step"], lr)
    new["n"], new["n_m"], new["n_v"] = adam_update(n.detach(), u_n, s["n_m"], s["n_v"], s["step"], lr)
    if first:
        new["e_hard"], new["n_hard"] = g_e != 0, g_n != 0
    new["step"] = s["step"] + 1
    info = dict(out=out.detach(), loss=loss.detach(), g_e=g_e, g_n=g_n, acts=[a.detach() for a in acts], emb=emb.detach())
    return new, info


def run(params, x, ei, batch, B, target, state, epochs, dtype=torch.float64, perturb=None, **kw):
    """`epochs` epochs -> (state after, loss history [epochs, B], the infos of every epoch)"""
    hist, infos = [], []
    for _ in range(epochs):
        state, info = epoch(params, x, ei, batch, B, target, state, dtype, perturb=perturb, **kw)
        hist.append(info["loss"])
        infos.append(info)
    return state, torch.stack(hist), infos


def masks(state):
    """the post-processed masks of a state -> (edge [E], node [N, F])"""
    return torch.sigmoid(state["e"]) * state["e_hard"], torch.sigmoid(state["n"]) * state["n_hard"]


def sign_perturbation(batch, ei, B, tol, seed):
    """`perturb` for `epoch`: every live entry's gradient moved by +- tol * max_g |g| (max over the graph's entries of that
    mask; signs from Generator(seed), drawn anew for every epoch)."""
    gen = torch.Generator().manual_seed(seed)
    eg = batch[ei[1]]

    def per_graph_max(g, owner):
        return torch.zeros(B, dtype=g.dtype).scatter_reduce(0, owner.reshape(-1), g.abs().reshape(-1), reduce="amax", include_self=True)

    def perturb(g_e, g_n, live_e, live_n):
        se = (torch.randint(0, 2, g_e.shape, generator=gen) * 2 - 1).to(g_e.dtype)
        sn = (torch.randint(0, 2, g_n.shape, generator=gen) * 2 - 1).to(g_n.dtype)
        owner_n = batch.unsqueeze(1).expand_as(g_n)
        de = tol * per_graph_max(g_e, eg)[eg] * se * live_e
        dn = tol * per_graph_max(g_n, owner_n)[owner_n] * sn * live_n
        return g_e + de, g_n + dn
    return perturb


def model_prediction(params, x, ei, batch, B, dtype=torch.float64):
    """the model's own unmasked prediction [B, C]: the default target"""
    p = {k: v.to(dtype) for k, v in params.items()}
    return O.gcn_forward(p, x.to(dtype), ei, batch, B)[0]


# ====================================================================================================== inputs and checks
# shared by tests/test_gpu_explain_fit.py (the kernel, the loop path on the GPU) and tests/test_host_explain_fit.py (the loop
# path on CPU tensors)
TOL = 1e-5                       # the bound ExplainStep's gradients carry (tests/test_gpu_explain.py)
PARAM_SEED, X_SEED, INIT_SEED = 23, 5, 41
NODE_LIMIT, EDGE_LIMIT = 224, 1024

# name -> (synth.make_batch arguments, share of x kept (1.0 = dense), model depths)
CASES = {
    "onehot25": (dict(num_graphs=6, nodes=30, nodes_jitter=10, extra_bonds=3, max_degree=4, feat=25), 0.2, dict(n_conv=2, n_read=2, n_classes=1)),
    "deep": (dict(num_graphs=4, nodes=20, nodes_jitter=4, extra_bonds=3, max_degree=4, feat=32), 0.5, dict(n_conv=3, n_read=3, n_classes=2)),
    "dense64": (dict(num_graphs=8, nodes=12, extra_bonds=2, max_degree=4, feat=64), 1.0, dict(n_conv=2, n_read=2, n_classes=1)),
    "limit": (dict(num_graphs=1, nodes=NODE_LIMIT, extra_bonds=EDGE_LIMIT // 2 - (NODE_LIMIT - 1), max_degree=6, feat=64), 1.0,
              dict(n_conv=2, n_read=2, n_classes=1)),
}


class Case:
    pass


def _edge_cases():
    """four graphs: one node and no edge; x all zero; an explicit (i, i) edge; a normal one -> (x, ei, batch, self-loop position)"""
    from hcatgnet_amd import synth
    sb = synth.make_batch(num_graphs=3, nodes=10, nodes_jitter=2, extra_bonds=2, max_degree=4, feat=25)
    x = torch.cat([torch.randn(1, 25, generator=torch.Generator().manual_seed(X_SEED)), sb.x])
    batch = torch.cat([torch.zeros(1, dtype=torch.long), sb.batch + 1])
    ei = sb.edge_index + 1
    x[batch == 1] = 0.0
    eg = batch[ei[1]]
    pos = int((eg <= 2).sum()) - 3                           # inside graph 2's edge block
    node = int(ei[0, pos])
    ei = torch.cat([ei[:, :pos], torch.tensor([[node], [node]]), ei[:, pos:]], 1).contiguous()
    return x, ei, batch, pos


_cache = {}


def case(name):
    """-> params, the graphs (CPU), the target (the fp64 model's own prediction, as float32) and a decidable fresh state"""
    if name in _cache:
        return _cache[name]
    from hcatgnet_amd import synth
    from tests.test_gpu_explain import _rand_params
    c = Case()
    c.name = name
    if name == "edge-cases":
        c.x, c.ei, c.batch, c.self_loop = _edge_cases()
        c.B, mk = 4, dict(n_conv=2, n_read=2, n_classes=1)
    else:
        bk, keep, mk = CASES[name]
        sb = synth.make_batch(**bk)
        c.x, c.ei, c.batch, c.B = sb.x, sb.edge_index, sb.batch, sb.num_graphs
        if keep < 1.0:
            c.x = c.x * (torch.rand(c.x.shape, generator=torch.Generator().manual_seed(X_SEED)) < keep)
    c.max_nodes = int(torch.bincount(c.batch, minlength=c.B).max())
    c.max_edges = int(torch.bincount(c.batch[c.ei[1]], minlength=c.B).max())
    c.params = _rand_params(c.x.shape[1], 64, seed=PARAM_SEED, **mk)
    c.target = model_prediction(c.params, c.x, c.ei, c.batch, c.B).float()
    c.gen = torch.Generator().manual_seed(INIT_SEED)
    c.init = init_state(c.x, c.ei, c.batch, c.B, c.gen)
    c.horizon = 2 if name == "limit" else 30 if name in ("onehot25", "deep") else 12
    c.warm = 1 if name == "limit" else 3          # epochs before the second state of `check_one_epoch`
    c.runs = {}
    print(f"\n  case {name}: B {c.B} N {c.x.shape[0]} E {c.ei.shape[1]} max {c.max_nodes} / {c.max_edges}")
    _cache[name] = c
    return c


def reference(c, epochs, max_rounds=12):
    """The fp64 reference of `epochs` epochs from the case's fresh state -> (states [epochs + 1] (0 = fresh), history, infos).
    Computed once per case for `c.horizon` epochs (the longest any test asks for), so every test of a case sees the same
    fresh state.  The masked forwards of the epochs 0 .. c.warm -- the states from which one epoch is compared piece by
    piece (`check_one_epoch`: the fresh state and the state after c.warm epochs) and the ones between them -- are screened
    for decidability as tests/test_gpu_explain.py screens its masks (LeakyReLU and max-pool margins), and the two compared
    states for conditioning (`ill_conditioned`); the logits of a flagged graph are re-drawn from the case's generator and
    the run repeated, until no graph is flagged: no graph is left out.  Later epochs are not screened: over 30 epochs some activation of some graph nearly always passes within 2e-6
    of a kink (about 22 000 activations per epoch on `onehot25`), and a whole fit is judged by `mask_bound` instead, which
    fails the test when the inputs are undecidable."""
    from tests.test_gpu_explain import _flagged
    assert epochs <= c.horizon
    if c.runs:
        states, hist, infos = c.runs["all"]
        return states[:epochs + 1], hist[:epochs], infos[:epochs]
    eg = c.batch[c.ei[1]]
    redrawn_kink, redrawn_ill = torch.zeros(c.B, dtype=torch.bool), torch.zeros(c.B, dtype=torch.bool)
    for rounds in range(max_rounds + 1):
        states, hist, infos, s = [cast(c.init, torch.float64)], [], [], c.init
        bad = torch.zeros(c.B, dtype=torch.bool)
        for _ in range(c.horizon):
            s, info = epoch(c.params, c.x, c.ei, c.batch, c.B, c.target, s)
            if len(infos) <= c.warm:
                bad |= _flagged(c.params, info, c.batch, c.B)
            states.append(s); hist.append(info["loss"]); infos.append(info)
        ill = torch.zeros(c.B, dtype=torch.bool)
        for i in (0, c.warm):
            ill |= ill_conditioned(c, rounded(states[i]))
        redrawn_kink |= bad
        redrawn_ill |= ill
        bad |= ill
        if not bool(bad.any()):
            print(f"    {c.name}: reference epochs 0 .. {c.warm} decidable and well conditioned after {rounds} rounds; of {c.B} graphs "
                  f"{int(redrawn_kink.sum())} re-drawn for a kink / max-pool margin, {int(redrawn_ill.sum())} for conditioning")
            c.runs["all"] = (states, torch.stack(hist), infos)
            return states[:epochs + 1], c.runs["all"][1][:epochs], infos[:epochs]
        fresh = init_state(c.x, c.ei, c.batch, c.B, c.gen)
        c.init = dict(c.init)
        c.init["e"] = torch.where(bad[eg], fresh["e"], c.init["e"])
        c.init["n"] = torch.where(bad[c.batch].unsqueeze(1), fresh["n"], c.init["n"])
    raise AssertionError(f"graphs still flagged after {max_rounds} rounds")


def rounded(state):
    """a reference state as the float32 state a run is handed (float32 values, held in float32)"""
    return cast(state, torch.float32)


def _per_graph_rel(a, ref, owner, B, each=False):
    """max over the graphs (`each`: the list over the graphs) of max |a - ref| / max |ref| over each graph's entries"""
    a, ref = a.double().reshape(-1), ref.double().reshape(-1)
    owner = owner.reshape(-1)
    den = ref.abs()
    per = [0.0] * B
    for b in range(B):
        m = owner == b
        if bool(m.any()):
            per[b] = float((a[m] - ref[m]).abs().max()) / max(float(den[m].max()), 1e-30)
    return per if each else max(per, default=0.0)


def ill_conditioned(c, s_in):
    """Graphs whose gradients float32 cannot deliver to TOL from the float32 state `s_in` -> bool [B].  The prediction loss's
    gradient is proportional to the residual out - target, and the target is the model's own prediction: where a graph's
    residual is a cancelled difference (2e-3 on outputs of 7e-2 in one graph of `dense64`), the rounding of `out` alone is a
    relative error of the WHOLE gradient of that graph (tests/test_gpu_explain.py notes the same of ExplainStep's target
    mode).  Judged by the reference alone: its own epoch restated in float32 must meet HALF the bound against fp64, per
    graph, on both gradients -- the other half is left to the different rounding of the code under test."""
    _, i64 = epoch(c.params, c.x, c.ei, c.batch, c.B, c.target, s_in)
    _, i32 = epoch(c.params, c.x, c.ei, c.batch, c.B, c.target, s_in, dtype=torch.float32)
    eg, ng = c.batch[c.ei[1]], c.batch.unsqueeze(1).expand_as(c.x)
    e = _per_graph_rel(i32["g_e"], i64["g_e"], eg, c.B, each=True)
    n = _per_graph_rel(i32["g_n"], i64["g_n"], ng, c.B, each=True)
    return torch.tensor([max(a, b) > 0.5 * TOL for a, b in zip(e, n)])


def check_one_epoch(c, s_in, got, tag, lr=LR):
    """Test 1 of the issue: one epoch from `s_in` (float32 state) as the code under test ran it (`got`: dict(state, out,
    loss)) against the reference's epoch from the same state, in well-conditioned pieces.  Prints, then asserts."""
    ref, info = epoch(c.params, c.x, c.ei, c.batch, c.B, c.target, s_in)
    g = got["state"]
    eg, ng = c.batch[c.ei[1]], c.batch.unsqueeze(1).expand_as(c.x)
    assert g["step"] == s_in["step"] + 1
    assert torch.equal(g["e_hard"], ref["e_hard"]) and torch.equal(g["n_hard"], ref["n_hard"]), tag
    fig = {}
    for k, gk, owner in (("e", "g_e", eg), ("n", "g_n", ng)):
        m_in, v_in = s_in[k + "_m"].double(), s_in[k + "_v"].double()
        m_out, v_out, p_out = g[k + "_m"].double(), g[k + "_v"].double(), g[k].double()
        gr = info[gk]
        # the gradient the step used, recovered from the first moment; its square from the second
        fig[k + " grad"] = _per_graph_rel((m_out - B1 * m_in) / ONE_MINUS_B1, gr, owner, c.B)
        fig[k + " sq"] = _per_graph_rel((v_out - B2 * v_in) / ONE_MINUS_B2, gr * gr, owner, c.B)
        # the update rule from the run's OWN moments, in fp64
        kk = s_in["step"] + 1
        step = (lr / (1.0 - B1 ** kk)) * (m_out / (v_out.sqrt() / math.sqrt(1.0 - B2 ** kk) + ADAM_EPS))
        want = s_in[k].double() - step
        rule = (p_out - want).abs() / (want.abs() + step.abs()).clamp_min(1e-300)
        fig[k + " rule"] = float(rule.max()) if rule.numel() else 0.0
        idle = ~ref[k + "_hard"]
        assert torch.equal(g[k][idle], s_in[k][idle]), f"{tag}: an entry that is not hard moved"
    fig["out"] = float((got["out"].double() - info["out"]).abs().max()) / max(float(info["out"].abs().max()), 1.0)
    fig["loss"] = float(((got["loss"].double() - info["loss"]).abs() / info["loss"].abs().clamp_min(1.0)).max())
    print(f"    {tag} step {s_in['step']}: " + "  ".join(f"{k} {v:.2e}" for k, v in fig.items()))
    for k in ("e", "n"):
        assert fig[k + " grad"] <= TOL and fig[k + " sq"] <= 2 * TOL and fig[k + " rule"] <= 2.0 ** -20, (tag, fig)
    assert fig["out"] <= TOL and fig["loss"] <= TOL, (tag, fig)
    for t in list(g.values()) + [got["out"], got["loss"]]:
        assert not torch.is_tensor(t) or not t.is_floating_point() or bool(torch.isfinite(t).all()), tag
    return fig


def mask_bound(c, epochs, lr=LR, seeds=(1, 2)):
    """Test 3's bound on |mask - mask_ref|, from the reference alone: twice the largest deviation of the final masks when
    every epoch's gradient is perturbed by +- TOL * max_g |g| (hard entries only, seeded signs).  Above 0.25 * lr the
    inputs are undecidable: the caller fails."""
    states, _, _ = reference(c, epochs)
    em, nm = masks(states[-1])
    dev = 0.0
    for seed in seeds:
        sp, _, _ = run(c.params, c.x, c.ei, c.batch, c.B, c.target, c.init, epochs,
                       perturb=sign_perturbation(c.batch, c.ei, c.B, TOL, seed))
        ep, np_ = masks(sp)
        dev = max(dev, float((ep - em).abs().max()), float((np_ - nm).abs().max()))
        print(f"    {c.name}: perturbed reference (seed {seed}) moved logits by {float((sp['e'] - states[-1]['e']).abs().max()):.2e} / "
              f"{float((sp['n'] - states[-1]['n']).abs().max()):.2e}, masks by {dev:.2e}")
    return 2.0 * dev, 0.25 * lr


def check_whole_fit(c, epochs, got, tag):
    """Test 3: `got` = dict(state, loss_history [T, B], edge_mask, node_mask) of a fit of `epochs` epochs from the case's
    fresh state.  Prints, then asserts."""
    states, hist, _ = reference(c, epochs)
    bound, cap = mask_bound(c, epochs)
    em, nm = masks(states[-1])
    fig = dict(hist=float(((got["loss_history"].double() - hist).abs() / hist.abs().clamp_min(1.0)).max()),
               edge=float((got["edge_mask"].double() - em).abs().max()), node=float((got["node_mask"].double() - nm).abs().max()),
               e_logit=float((got["state"]["e"].double() - states[-1]["e"]).abs().max()),
               n_logit=float((got["state"]["n"].double() - states[-1]["n"]).abs().max()))
    print(f"    {tag} {epochs} epochs: " + "  ".join(f"{k} {v:.2e}" for k, v in fig.items()) + f"  bound {bound:.2e} cap {cap:.2e}")
    assert bound <= cap, f"{tag}: the inputs are undecidable (bound {bound:.2e} above the cap {cap:.2e})"
    assert torch.equal(got["state"]["e_hard"], states[-1]["e_hard"]) and torch.equal(got["state"]["n_hard"], states[-1]["n_hard"])
    assert fig["hist"] <= TOL and fig["edge"] <= bound and fig["node"] <= bound, (tag, fig, bound)
    assert got["state"]["step"] == epochs
    return fig


# ---- between the reference's state (a dict) and ExplainFitState
def to_fit_state(s, batch_vec, ei, B, device):
    from hcatgnet_amd.explain import ExplainFitState
    eg = batch_vec[ei[1]]
    cnt = torch.stack([torch.bincount(eg[s["e_hard"]], minlength=B),
                       torch.zeros(B, dtype=torch.long).index_add_(0, batch_vec, s["n_hard"].sum(dim=1))], 1).to(torch.int32)
    f = lambda t: t.float().clone().contiguous().to(device)          # (a copy: the fit updates its state in place)
    return ExplainFitState(f(s["e"]), f(s["e_m"]), f(s["e_v"]), s["e_hard"].clone().to(device), f(s["n"]), f(s["n_m"]), f(s["n_v"]),
                           s["n_hard"].clone().to(device), cnt.to(device), int(s["step"]))


def from_fit_state(st):
    c = lambda t: t.detach().cpu().clone()
    return dict(e=c(st.edge_logit), e_m=c(st.edge_exp_avg), e_v=c(st.edge_exp_avg_sq), e_hard=c(st.edge_hard), n=c(st.node_logit),
                n_m=c(st.node_exp_avg), n_v=c(st.node_exp_avg_sq), n_hard=c(st.node_hard), step=int(st.step),
                hard_count=c(st.hard_count))
