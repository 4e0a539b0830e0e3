"""The reference of the classification-mode `ExplainFit` / `ExplainStep(target_class=)` tests: tests/explain_fit_ref.py with
the prediction loss as a parameter.  fp64 autograd on `oracle.gcn_forward(..., edge_mask=)`, state in and state out; never
the GPU path, never the code under test; no torch_geometric.

Definition (published torch_geometric 2.3 / 2.4 `GNNExplainer`, `ModelMode.multiclass_classification`, `return_type='raw'`,
a batch-of-one fit per graph): everything of tests/explain_fit_ref.py -- regularisers, hard flags, Adam, post-processing --
with the prediction loss of graph g
    "ce"    l_g = -log_softmax(out_g)[y_g]   (`F.cross_entropy` of one row; y int64 [B], by default the argmax of the model's
                                              own unmasked output, the first maximal index on a tie)
    "mse"   l_g = mean_c (out_gc - target_gc)^2   (what tests/explain_fit_ref.py states; kept so that the restated functions
                                              can be held against the originals)
Everything that does not depend on the loss is imported from tests/explain_fit_ref.py, not copied; so are its tolerances.

Conditioning is a condition on the INPUTS, checked by the reference alone.  A cross-entropy gradient scales with
exp(-margin): a graph whose logit margin is large is beyond float32 for any code.  `ill_conditioned` sees that (the
reference's own epoch in float32 against fp64 must meet half of TOL).  Figures on these cases (fresh state, target = argmax;
fp32-vs-fp64 per-graph error of the gradients): `c3x16` <= 1.4e-6; `c3` <= 5.8e-7; `c8x16` <= 6.6e-7; one class off the
argmax they stay <= 7e-7 (tests/test_host_explain_ce.py prints them for the states it compares).  `dense64` shapes with
C = 2 and the last layer x 32 reach p_y >= 0.996 and 5e-4: that case fails its own screen and is not used.  A state that
`reference` cannot make decidable is a reason to lower a case's scale, never a tolerance.
"""
import math

import torch
import torch.nn.functional as Fn

from oracle import gcn_oracle as O
from tests.explain_fit_ref import (ADAM_EPS, B1, B2, COEFFS, EDGE_LIMIT, INIT_SEED, LR, NODE_LIMIT, ONE_MINUS_B1, ONE_MINUS_B2,
                                   PARAM_SEED, TOL, X_SEED, Case, _edge_cases, _ent, _per_graph_mean, _per_graph_rel, adam_update,
                                   cast, from_fit_state, init_state, masks, rounded, sign_perturbation, to_fit_state)

__all__ = ["from_fit_state", "to_fit_state", "rounded", "masks", "Case", "TOL", "LR"]

LOSSES = {
    "ce": lambda out, target: Fn.cross_entropy(out, target, reduction="none"),
    "mse": lambda out, target: ((out - target.to(out.dtype)) ** 2).mean(dim=1),
}


def epoch(params, x, ei, batch, B, target, state, dtype=torch.float64, lr=LR, coeffs=COEFFS, perturb=None, loss="ce"):
    """tests/explain_fit_ref.py `epoch` with the prediction loss `loss` (a key of LOSSES) -> (state after, info)"""
    p = {k: v.to(dtype) for k, v in params.items()}
    s = cast(state, dtype)
    e = s["e"].requires_grad_(True)
    n = s["n"].requires_grad_(True)
    eg = batch[ei[1]]
    out, emb, acts = O.gcn_forward(p, x.to(dtype) * torch.sigmoid(n), ei, batch, B, edge_mask=torch.sigmoid(e),
                                   return_intermediates=True)
    l = LOSSES[loss](out, target)
    J = l.sum()
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
    info = dict(out=out.detach(), loss=l.detach(), g_e=g_e, g_n=g_n, acts=[a.detach() for a in acts], emb=emb.detach())
    return new, info


def run(params, x, ei, batch, B, target, state, epochs, dtype=torch.float64, perturb=None, **kw):
    """`epochs` epochs -> (state after, loss history [epochs, B], the infos of every epoch)"""
    hist, infos = [], []
    for _ in range(epochs):
        state, info = epoch(params, x, ei, batch, B, target, state, dtype, perturb=perturb, **kw)
        hist.append(info["loss"])
        infos.append(info)
    return state, torch.stack(hist), infos


def model_prediction(params, x, ei, batch, B, dtype=torch.float64):
    """the model's own unmasked output [B, C]"""
    p = {k: v.to(dtype) for k, v in params.items()}
    return O.gcn_forward(p, x.to(dtype), ei, batch, B)[0]


# ====================================================================================================== inputs and checks
# name -> (synth.make_batch arguments, share of x kept (1.0 = dense), model depths, factor on the last readout layer)
CASES = {
    "c3x16": (dict(num_graphs=6, nodes=30, nodes_jitter=10, extra_bonds=3, max_degree=4, feat=25), 0.2, dict(n_conv=2, n_read=2, n_classes=3), 16.0),
    "c3": (dict(num_graphs=6, nodes=30, nodes_jitter=10, extra_bonds=3, max_degree=4, feat=25), 0.2, dict(n_conv=2, n_read=2, n_classes=3), 1.0),
    "c8x16": (dict(num_graphs=4, nodes=20, nodes_jitter=4, extra_bonds=3, max_degree=4, feat=32), 0.5, dict(n_conv=3, n_read=3, n_classes=8), 16.0),
    "limit": (dict(num_graphs=1, nodes=NODE_LIMIT, extra_bonds=EDGE_LIMIT // 2 - (NODE_LIMIT - 1), max_degree=6, feat=64), 1.0,
              dict(n_conv=2, n_read=2, n_classes=8), 1.0),
}
MAIN = ("c3x16", "c3", "c8x16")          # the cases of the one-epoch, split and whole-fit tests

_cache = {}


def case(name):
    """-> params, the graphs (CPU), the model's fp64 output, target = its argmax (int64 [B]) and a fresh state"""
    if name in _cache:
        return _cache[name]
    from hcatgnet_amd import synth
    from tests.test_gpu_explain import _rand_params
    c = Case()
    c.name, c.loss = name, "ce"
    if name == "edge-cases":
        c.x, c.ei, c.batch, c.self_loop = _edge_cases()
        c.B, mk, scale = 4, dict(n_conv=2, n_read=2, n_classes=3), 1.0
    else:
        bk, keep, mk, scale = CASES[name]
        sb = synth.make_batch(**bk)
        c.x, c.ei, c.batch, c.B = sb.x, sb.edge_index, sb.batch, sb.num_graphs
        if keep < 1.0:
            c.x = c.x * (torch.rand(c.x.shape, generator=torch.Generator().manual_seed(X_SEED)) < keep)
    c.max_nodes = int(torch.bincount(c.batch, minlength=c.B).max())
    c.max_edges = int(torch.bincount(c.batch[c.ei[1]], minlength=c.B).max())
    c.params = _rand_params(c.x.shape[1], 64, seed=PARAM_SEED, **mk)
    last = mk["n_read"] - 1
    c.params[f"readout.{last}.weight"] = c.params[f"readout.{last}.weight"] * scale
    c.params[f"readout.{last}.bias"] = c.params[f"readout.{last}.bias"] * scale
    c.C = mk["n_classes"]
    c.prediction = model_prediction(c.params, c.x, c.ei, c.batch, c.B)
    c.target = c.prediction.argmax(dim=1)
    py = torch.softmax(c.prediction, 1).gather(1, c.target.unsqueeze(1))
    c.gen = torch.Generator().manual_seed(INIT_SEED)
    c.init = init_state(c.x, c.ei, c.batch, c.B, c.gen)
    c.horizon = 2 if name == "limit" else 30 if name in MAIN else 12
    c.warm = 1 if name == "limit" else 3          # epochs before the second state of `check_one_epoch`
    c.runs = {}
    print(f"\n  case {name}: B {c.B} N {c.x.shape[0]} E {c.ei.shape[1]} max {c.max_nodes} / {c.max_edges}  C {c.C}  "
          f"p_y of the unmasked model {float(py.min()):.3f} .. {float(py.max()):.3f}")
    _cache[name] = c
    return c


def off_argmax(c):
    """the case with every graph's target one class off the argmax (its own fresh state and reference)"""
    key = c.name + "+1"
    if key not in _cache:
        k = Case()
        k.__dict__.update(c.__dict__)
        k.name, k.target = key, (c.target + 1) % c.C
        k.gen = torch.Generator().manual_seed(INIT_SEED)
        k.init = init_state(k.x, k.ei, k.batch, k.B, k.gen)
        k.horizon, k.runs = k.warm, {}
        _cache[key] = k
    return _cache[key]


FIRST_STEP_MARGIN = 4.0


def first_step_undecidable(c, info):
    """Graphs with a live entry whose FIRST gradient is within FIRST_STEP_MARGIN * TOL of 0, relative to the largest of the
    graph's entries of that mask -> bool [B].  Adam's first step is lr * g / (|g| + eps): the sign of the gradient.  An entry
    whose first gradient is below the error TOL allows (here: -4e-8 beside a graph maximum of 8e-3, so that a perturbation of
    TOL * max = 8e-8 turns it round) moves by +lr or by -lr depending on that error, for ANY code, and `mask_bound` then
    rightly calls the whole fit undecidable (a logit 2e-2 apart after 12 epochs).  Like a kink or a near-tie this is a
    property of the inputs, seen on the fp64 reference alone; the remedy is the same: the graph's logits are re-drawn."""
    eg, ng = c.batch[c.ei[1]], c.batch.unsqueeze(1).expand_as(c.x)
    bad = torch.zeros(c.B, dtype=torch.bool)
    for g, owner in ((info["g_e"], eg), (info["g_n"], ng)):
        a, owner = g.abs().reshape(-1), owner.reshape(-1)
        top = torch.zeros(c.B, dtype=a.dtype).scatter_reduce(0, owner, a, reduce="amax", include_self=True)
        close = (a > 0) & (a < FIRST_STEP_MARGIN * TOL * top[owner])
        bad[owner[close]] = True
    return bad


def reference(c, epochs, max_rounds=24):
    """tests/explain_fit_ref.py `reference` on this module's `epoch`: the fp64 run of `c.horizon` epochs from the case's fresh
    state, computed once; the epochs 0 .. c.warm screened for decidability, the two compared states for conditioning and the
    first epoch for the sign of Adam's first step (`first_step_undecidable`); the logits of a flagged graph re-drawn from
    the case's generator until no graph is flagged.  No graph is left out."""
    from tests.test_gpu_explain import _flagged
    assert epochs <= c.horizon
    if c.runs:
        states, hist, infos = c.runs["all"]
        return states[:epochs + 1], hist[:epochs], infos[:epochs]
    eg = c.batch[c.ei[1]]
    redrawn_kink, redrawn_ill = torch.zeros(c.B, dtype=torch.bool), torch.zeros(c.B, dtype=torch.bool)
    redrawn_sign = torch.zeros(c.B, dtype=torch.bool)
    for rounds in range(max_rounds + 1):
        states, hist, infos, s = [cast(c.init, torch.float64)], [], [], c.init
        bad = torch.zeros(c.B, dtype=torch.bool)
        for _ in range(c.warm + 1):                           # the screened epochs
            s, info = epoch(c.params, c.x, c.ei, c.batch, c.B, c.target, s, loss=c.loss)
            bad |= _flagged(c.params, info, c.batch, c.B)
            states.append(s); hist.append(info["loss"]); infos.append(info)
        ill = torch.zeros(c.B, dtype=torch.bool)
        for i in (0, c.warm):
            ill |= ill_conditioned(c, rounded(states[i]))
        # (only where a whole fit is judged: one epoch is compared in pieces that do not depend on the step's sign, and among
        #  the 15 000 entries of the `limit` graph some first gradient is always that close to 0)
        sign = first_step_undecidable(c, infos[0]) if c.name.split("+")[0] in MAIN else torch.zeros(c.B, dtype=torch.bool)
        redrawn_kink |= bad
        redrawn_ill |= ill
        redrawn_sign |= sign
        bad |= ill | sign
        if not bool(bad.any()):
            for _ in range(c.warm + 1, c.horizon):            # the rest of the horizon, once the start is settled
                s, info = epoch(c.params, c.x, c.ei, c.batch, c.B, c.target, s, loss=c.loss)
                states.append(s); hist.append(info["loss"]); infos.append(info)
            print(f"    {c.name}: reference epochs 0 .. {c.warm} decidable and well conditioned after {rounds} rounds; of {c.B} graphs "
                  f"{int(redrawn_kink.sum())} re-drawn for a kink / max-pool margin, {int(redrawn_ill.sum())} for conditioning, "
                  f"{int(redrawn_sign.sum())} for the sign of a first gradient")
            c.runs["all"] = (states, torch.stack(hist), infos)
            return states[:epochs + 1], c.runs["all"][1][:epochs], infos[:epochs]
        fresh = init_state(c.x, c.ei, c.batch, c.B, c.gen)
        c.init = dict(c.init)
        c.init["e"] = torch.where(bad[eg], fresh["e"], c.init["e"])
        c.init["n"] = torch.where(bad[c.batch].unsqueeze(1), fresh["n"], c.init["n"])
    raise AssertionError(f"graphs still flagged after {max_rounds} rounds")


def conditioning(c, s_in):
    """per graph: the error of the reference's own float32 epoch from `s_in` against fp64, the larger of both gradients"""
    _, i64 = epoch(c.params, c.x, c.ei, c.batch, c.B, c.target, s_in, loss=c.loss)
    _, i32 = epoch(c.params, c.x, c.ei, c.batch, c.B, c.target, s_in, dtype=torch.float32, loss=c.loss)
    eg, ng = c.batch[c.ei[1]], c.batch.unsqueeze(1).expand_as(c.x)
    e = _per_graph_rel(i32["g_e"], i64["g_e"], eg, c.B, each=True)
    n = _per_graph_rel(i32["g_n"], i64["g_n"], ng, c.B, each=True)
    return [max(a, b) for a, b in zip(e, n)]


def ill_conditioned(c, s_in):
    """Graphs whose gradients float32 cannot deliver to TOL from the float32 state `s_in` -> bool [B]: the reference's own
    epoch restated in float32 must meet HALF the bound against fp64, per graph, on both gradients."""
    return torch.tensor([v > 0.5 * TOL for v in conditioning(c, s_in)])


def check_one_epoch(c, s_in, got, tag, lr=LR):
    """One epoch from `s_in` (float32 state) as the code under test ran it (`got`: dict(state, out, loss)) against the
    reference's epoch from the same state, in well-conditioned pieces (tests/explain_fit_ref.py `check_one_epoch`, its
    tolerances).  Prints, then asserts."""
    ref, info = epoch(c.params, c.x, c.ei, c.batch, c.B, c.target, s_in, loss=c.loss)
    g = got["state"]
    eg, ng = c.batch[c.ei[1]], c.batch.unsqueeze(1).expand_as(c.x)
    assert g["step"] == s_in["step"] + 1
    assert torch.equal(g["e_hard"], ref["e_hard"]) and torch.equal(g["n_hard"], ref["n_hard"]), tag
    fig = {}
    for k, gk, owner in (("e", "g_e", eg), ("n", "g_n", ng)):
        m_in, v_in = s_in[k + "_m"].double(), s_in[k + "_v"].double()
        m_out, v_out, p_out = g[k + "_m"].double(), g[k + "_v"].double(), g[k].double()
        gr = info[gk]
        fig[k + " grad"] = _per_graph_rel((m_out - B1 * m_in) / ONE_MINUS_B1, gr, owner, c.B)
        fig[k + " sq"] = _per_graph_rel((v_out - B2 * v_in) / ONE_MINUS_B2, gr * gr, owner, c.B)
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
    """The bound on |mask - mask_ref| of a whole fit, from the reference alone: twice the largest deviation of the final masks
    when every epoch's gradient is perturbed by +- TOL * max_g |g|.  Above 0.25 * lr the inputs are undecidable."""
    states, _, _ = reference(c, epochs)
    em, nm = masks(states[-1])
    dev = 0.0
    for seed in seeds:
        sp, _, _ = run(c.params, c.x, c.ei, c.batch, c.B, c.target, c.init, epochs,
                       perturb=sign_perturbation(c.batch, c.ei, c.B, TOL, seed), loss=c.loss)
        ep, np_ = masks(sp)
        dev = max(dev, float((ep - em).abs().max()), float((np_ - nm).abs().max()))
        print(f"    {c.name}: perturbed reference (seed {seed}) moved logits by {float((sp['e'] - states[-1]['e']).abs().max()):.2e} / "
              f"{float((sp['n'] - states[-1]['n']).abs().max()):.2e}, masks by {dev:.2e}")
    return 2.0 * dev, 0.25 * lr


_bounds = {}


def check_whole_fit(c, epochs, got, tag):
    """`got` = dict(state, loss_history [T, B], edge_mask, node_mask) of a fit of `epochs` epochs from the case's fresh state
    (tests/explain_fit_ref.py `check_whole_fit`).  Prints, then asserts."""
    states, hist, _ = reference(c, epochs)
    if (c.name, epochs) not in _bounds:                   # (from the reference alone: computed once per case and length)
        _bounds[(c.name, epochs)] = mask_bound(c, epochs)
    bound, cap = _bounds[(c.name, epochs)]
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
