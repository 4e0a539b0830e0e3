"""Models, reference and bound of `hcatgnet_amd.attribution.EnsembleAttribution` (tests/test_host_ensemble_attribution.py and
tests/test_gpu_ensemble_attribution.py).

Models.  Graphs and screened node features are the cases of tests/integrated_ref.py; model k of an ensemble is
`_rand_params(..., seed=PARAM_SEED + k)` with the case's depths, so model 0 is the case's own model.

Per-model yardstick.  Entry [m] of the per-model results must be `torch.equal` to what the existing, tested
`IntegratedGradients(models[m])` returns: no tolerance.

Moments.  ref = the per-model float32 arrays .double().mean(0) / .std(0, unbiased=False) on the CPU.  With s = max_m |v_m| per
entry the bound is |mean - ref_mean| <= (M + 4) 2^-24 s, and the same for std.  Reasoning: every one of the M updates of
Welford's recurrence rounds a handful of float32 operations on values of magnitude <= 2 s, so the error grows at most
linearly in M in units of ulp(s); `welford32` below restates the recurrence in float32 numpy, and the host test holds it to
the bound for M in {1, 2, 3, 5, 9, 90} on normal, nearly equal, wide-range and 30 %-zero inputs.  An entry with s = 0 must
have mean and std exactly 0 (the bound is 0 there).  `moment_figures` prints nothing and asserts nothing: callers print the
worst ratio before they assert it."""
import functools

import numpy as np
import torch

from tests import integrated_ref as R
from tests.test_gpu_explain import CASES as SHAPES
from tests.test_gpu_explain import PARAM_SEED, _rand_params

EPS = 2.0 ** -24


@functools.lru_cache(maxsize=None)
def params(name, k):
    """the weights of model k of the ensemble of case `name` (CPU float32 state-dict); k = 0: the case's own"""
    shape, _, width = name.partition("-d")
    bk, mk = SHAPES[shape]
    return _rand_params(bk["feat"], int(width or 64), seed=PARAM_SEED + k, **mk)


def models(H, name, M, device="cpu", **opt):
    """M models of case `name` on `device` (a fresh list every call: tests change their weights)"""
    c = R.case(name)
    out = []
    for k in range(M):
        proxy = R.Case()
        proxy.params = params(name, k)
        out.append(R.model(H, proxy, device, **opt))
    assert all(torch.equal(params(name, 0)[n], c.params[n]) for n in c.params)
    return out


def welford32(v):
    """The recurrence of csrc/explain.hip k_model_moments restated in float32 numpy: v [M, L] -> (mean [L], std [L])"""
    v = np.asarray(v, dtype=np.float32)
    M = v.shape[0]
    mean, m2 = np.zeros(v.shape[1:], dtype=np.float32), np.zeros(v.shape[1:], dtype=np.float32)
    for k in range(M):
        d = v[k] - mean
        mean = mean + d / np.float32(k + 1)
        m2 = m2 + d * (v[k] - mean)
    return mean, np.sqrt(m2 / np.float32(M))


def moment_figures(values, mean, std):
    """values [M, ...] float32 (the per-model arrays), mean / std [...] float32 under test -> dict(mean, std: the worst
    |got - ref| / ((M + 4) 2^-24 s) over the entries with s > 0; zeros_exact: every entry with s = 0 has mean = std = 0)"""
    v = torch.as_tensor(values).detach().cpu().double()
    M = v.shape[0]
    v = v.reshape(M, -1)
    got_mean, got_std = torch.as_tensor(mean).detach().cpu().double().reshape(-1), torch.as_tensor(std).detach().cpu().double().reshape(-1)
    ref_mean, ref_std = v.mean(0), v.std(0, unbiased=False)
    s = v.abs().amax(0)
    live = s > 0
    bound = (M + 4) * EPS * s[live]
    fig = dict(mean=0.0, std=0.0)
    if bool(live.any()):
        fig["mean"] = float(((got_mean - ref_mean)[live].abs() / bound).max())
        fig["std"] = float(((got_std - ref_std)[live].abs() / bound).max())
    fig["zeros_exact"] = bool((got_mean[~live] == 0).all()) and bool((got_std[~live] == 0).all())
    fig["zeros"] = int((~live).sum())
    return fig


def check_moments(values_node, values_edge, r, tag):
    """print the worst ratios of a result's four moment fields, then assert them (<= 1, exact zeros)"""
    fn = moment_figures(values_node, r.node_mean, r.node_std)
    fe = moment_figures(values_edge, r.edge_mean, r.edge_std)
    M = int(torch.as_tensor(values_node).shape[0])
    print(f"    {tag}: M {M}  worst |got - fp64| / ((M + 4) 2^-24 s):  node mean {fn['mean']:.3f} std {fn['std']:.3f}  "
          f"edge mean {fe['mean']:.3f} std {fe['std']:.3f}  all-zero entries {fn['zeros']} + {fe['zeros']}")
    for f in (fn, fe):
        assert f["mean"] <= 1.0 and f["std"] <= 1.0 and f["zeros_exact"], (fn, fe)
    return fn, fe
