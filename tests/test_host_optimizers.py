"""CPU checks of the reference's other two optimisers (`--optimizer SGD | rmsprop`, model/networks.py:36-44) as fused
optimisers: the factory builds them, they stay torch's classes with torch's defaults, refuse the variants the kernels do not
implement, keep torch's state-dict layout both ways, and the one-shot exchange refuses to carry them.  No GPU needed."""
import ctypes
import types

import pytest
import torch

import hcatgnet_amd as H
from hcatgnet_amd import _lib
from hcatgnet_amd.optim import FusedAdam, FusedRMSprop, FusedSGD


def test_factory_builds_the_fused_sgd_and_rmsprop():
    sgd = H.make_network("GCN", H.default_options(optimizer="SGD", lr=0.05), 25).optimizer
    rms = H.make_network("GCN", H.default_options(optimizer="rmsprop", lr=0.05), 25).optimizer
    assert type(sgd) is FusedSGD and isinstance(sgd, torch.optim.SGD)
    assert type(rms) is FusedRMSprop and isinstance(rms, torch.optim.RMSprop)
    g = sgd.param_groups[0]
    assert (g["lr"], g["momentum"], g["dampening"], g["weight_decay"], g["nesterov"], g["maximize"]) == (0.05, 0, 0, 0, False, False)
    g = rms.param_groups[0]
    assert (g["lr"], g["alpha"], g["eps"], g["momentum"], g["centered"], g["weight_decay"]) == (0.05, 0.99, 1e-8, 0, False, 0)
    assert g["capturable"] is False and g["maximize"] is False
    assert (sgd.RULE, rms.RULE, FusedAdam.RULE) == (_lib.HCG_UPDATE_SGD, _lib.HCG_UPDATE_RMSPROP, _lib.HCG_UPDATE_ADAM)


@pytest.mark.parametrize("kw", [dict(momentum=0.9), dict(dampening=0.1), dict(weight_decay=1e-4), dict(nesterov=True),
                                dict(maximize=True), dict(foreach=True), dict(fused=True), dict(differentiable=True)])
def test_sgd_refuses_what_the_kernels_do_not_implement(kw):
    p = torch.nn.Parameter(torch.zeros(3))
    with pytest.raises(ValueError):
        FusedSGD([p], lr=0.1, **kw)


@pytest.mark.parametrize("kw", [dict(momentum=0.9), dict(weight_decay=1e-4), dict(centered=True), dict(maximize=True),
                                dict(foreach=True), dict(capturable=True), dict(differentiable=True)])
def test_rmsprop_refuses_what_the_kernels_do_not_implement(kw):
    p = torch.nn.Parameter(torch.zeros(3))
    with pytest.raises(ValueError):
        FusedRMSprop([p], lr=0.1, **kw)


def _params(seed):
    g = torch.Generator().manual_seed(seed)
    return [torch.nn.Parameter(torch.randn(4, 3, generator=g)), torch.nn.Parameter(torch.randn(3, generator=g))]


def _torch_trained(cls, ps, steps=3):
    opt = cls(ps, lr=0.01)
    g = torch.Generator().manual_seed(7)
    for _ in range(steps):
        for p in ps:
            p.grad = torch.randn(p.shape, generator=g)
        opt.step()
    return opt


def _same_state_dict(a, b):
    assert a["param_groups"] == b["param_groups"]
    assert a["state"].keys() == b["state"].keys()
    for k in a["state"]:
        assert a["state"][k].keys() == b["state"][k].keys(), k
        for name in a["state"][k]:
            assert torch.equal(a["state"][k][name], b["state"][k][name]), (k, name)


@pytest.mark.parametrize("torch_cls,fused_cls", [(torch.optim.SGD, FusedSGD), (torch.optim.RMSprop, FusedRMSprop)])
def test_torch_state_dict_round_trips_through_the_fused_class(torch_cls, fused_cls):
    """A torch optimiser's state dict (RMSprop: step + square_avg; SGD with momentum 0: no per-parameter state) loads into the
    fused class on CPU parameters and comes back out unchanged; and back into torch's class."""
    ref = _torch_trained(torch_cls, _params(1))
    sd = ref.state_dict()
    if torch_cls is torch.optim.SGD:
        assert sd["state"] == {}
    else:
        assert set(sd["state"][0]) == {"step", "square_avg"} and float(sd["state"][0]["step"]) == 3.0
    fused = fused_cls(_params(2), lr=0.5)
    fused.load_state_dict(sd)
    out = fused.state_dict()
    _same_state_dict(out, sd)
    back = torch_cls(_params(3), lr=0.5)
    back.load_state_dict(out)
    _same_state_dict(back.state_dict(), sd)


def test_tail_and_update_structs_match_the_library():
    """The ctypes mirrors of hcg_tail_args (its former reserved word is the update rule) and hcg_update_args have the
    library's sizes; hcg_update_dev refuses a malformed argument block without touching the GPU."""
    lib = _lib.load()
    assert ctypes.sizeof(_lib.TailArgs) == lib.hcg_struct_bytes(_lib.HCG_STRUCT_TAIL_ARGS)
    assert ctypes.sizeof(_lib.UpdateArgs) == lib.hcg_struct_bytes(_lib.HCG_STRUCT_UPDATE_ARGS)
    assert lib.hcg_update_dev(None, None) == -1
    a = _lib.UpdateArgs()
    assert lib.hcg_update_dev(ctypes.addressof(a), None) == -1                    # n = 0
    a.n, a.grad, a.param = 16, 0x1000, 0x2000
    assert lib.hcg_update_dev(ctypes.addressof(a), None) == -1                    # no lr / step words
    a.lr_dev, a.step_dev, a.update_rule = 0x3000, 0x4000, 7
    assert lib.hcg_update_dev(ctypes.addressof(a), None) == -1                    # unknown rule
    a.update_rule = _lib.HCG_UPDATE_RMSPROP
    assert lib.hcg_update_dev(ctypes.addressof(a), None) == -1                    # RMSprop without square_avg
    a.update_rule = _lib.HCG_UPDATE_ADAM
    assert lib.hcg_update_dev(ctypes.addressof(a), None) == -1                    # Adam without moments
    t = _lib.TailArgs()
    job = ctypes.create_string_buffer(_lib.job_bytes())
    t.jobs_host, t.njobs = ctypes.addressof(job), 1
    t.param, t.grad_flat, t.n, t.lr_dev, t.step_dev = 0x2000, 0x1000, 16, 0x3000, 0x4000
    for rule in (7, _lib.HCG_UPDATE_RMSPROP, _lib.HCG_UPDATE_ADAM):               # bad rule / missing state
        t.update_rule = rule
        assert lib.hcg_step_tail(ctypes.addressof(t), None) == -1, rule


@pytest.mark.parametrize("name", ["SGD", "rmsprop"])
def test_one_shot_exchange_refuses_other_rules(name):
    """The one-shot exchange carries Adam's update only: attaching a trainer whose optimiser is another rule raises a
    ValueError pointing to the RCCL form, and leaves the trainer's collective in place."""
    from hcatgnet_amd.xgmi import OneShotExchange
    model = H.make_network("GCN", H.default_options(optimizer=name), 25)
    xchg = OneShotExchange.__new__(OneShotExchange)               # (the gate runs before anything touches a device)
    xchg.ok, xchg.n = True, sum(q.numel() for q in model.parameters() if q.requires_grad)
    sync = lambda flat: None
    step = types.SimpleNamespace(model=model, optimizer_step=True, grad_sync=sync)
    with pytest.raises(ValueError, match="RCCL"):
        xchg.attach(step)
    assert step.grad_sync is sync and not hasattr(step, "exchange")
