"""The reference's three optimisers (`--optimizer Adam | SGD | rmsprop`, model/networks.py:36-44) with the update done by
ONE HIP launch when the gradients sit in one flat buffer (which the fused backward guarantees), one gather + one launch
otherwise, and carried in the step's last launch (hcg_step_tail) by `train.FusedTrainStep`.

- `FusedAdam`: `torch.optim.Adam` semantics (the reference builds `Adam(self.parameters(), lr, eps=1e-9)`,
  model/networks.py:38).  Restrictions (checked): float32, amsgrad / weight_decay / maximize off.
- `FusedSGD`: `torch.optim.SGD(params, lr)` (model/networks.py:40): p -= lr g; momentum / dampening / nesterov /
  weight_decay / maximize refused.
- `FusedRMSprop`: `torch.optim.RMSprop(params, lr)` (model/networks.py:42): v = alpha v + (1 - alpha) g^2,
  p -= lr g / (sqrt(v) + eps); momentum / centered / weight_decay / maximize refused.

Each IS its torch class (param_groups, state_dict in torch's layout, zero_grad, lr schedulers -- e.g. the reference's
`ReduceLROnPlateau` -- all work): `lr` is read from `param_groups` at every step.  Parameters and the rule's state tensors are
re-based onto flat storages the first time `step()` sees them on the GPU; the `nn.Parameter` objects stay the same (only
`.data` is re-pointed), so `state_dict()/load_state_dict()` of the module are unaffected.  The machinery that is not the rule's
own -- flat storages, the device step / lr words, the carried and the plain update -- is `FusedFlatOptimizer`'s.
"""
from __future__ import annotations

import torch

from . import _lib


class FusedFlatOptimizer:
    """Mixin in front of a `torch.optim.Optimizer` subclass.  A rule supplies `RULE` (HCG_UPDATE_*), `STATE` (pairs of
    flat-buffer slot and torch's state name: slot "m" is the kernels' first moment, "v" the second / RMSprop's square_avg),
    `KEEPS_STEP` (torch keeps a `step` in the parameter's state) and `_hparams(group)` -> (beta1, beta2, eps) of the
    launches; a rule with `HOST_FORM` also has `_host_update`, its launch with a host step count outside the capturable
    mode (a rule without one always runs the device form, whose count is then the authority)."""
    RULE = _lib.HCG_UPDATE_ADAM
    STATE = ()
    KEEPS_STEP = True
    HOST_FORM = False

    def _hparams(self, group):
        raise NotImplementedError

    def flat_state(self, fl) -> list:
        """The flat storages of the rule's state tensors in `fl` (a `_flat` entry), in `STATE` order."""
        return [fl[slot] for slot, _ in self.STATE]

    def _device_count(self) -> bool:
        return self.capturable or not self.HOST_FORM

    # ------------------------------------------------------------------ hipGraph-capturable mode
    def enable_capturable(self):
        """Keep the step count and the learning rate in device memory (hcg_adam_step_dev / hcg_update_dev), so that `step()`
        can be captured into a hipGraph and replayed: from here on the device counter is the authority (`steps_done()`),
        `sync_lr()` pushes a learning rate a scheduler changed.  Needs flat gradients (the fused backward's)."""
        self.capturable = True
        for gi, group in enumerate(self.param_groups):
            fl = self._flat.get(gi)
            if fl is not None:
                self._make_dev_state(fl, group)

    def capture_state(self, gi: int = 0) -> list:
        """Ready group `gi` for a capture that takes its own warm-up back: capturable mode, flat storages (re-based now if
        need be), device words.  -> the live tensors its steps modify: flat parameters, the rule's `STATE` storages, the
        step-count word (NOT the exchange stamp, which never goes back).  `on_storages`: still the group's afterwards?"""
        self.enable_capturable()
        group, fl = self.param_groups[gi], self._flat.get(gi)
        ps = [q for q in group["params"] if q.requires_grad]
        if (fl is None or len(fl["params"]) != len(ps) or any(a is not b for a, b in zip(fl["params"], ps))
                or ps[0].data_ptr() != fl["p"].data_ptr()):
            with torch.no_grad():
                fl = self._rebase(gi, group)
        self._make_dev_state(fl, group)
        return [fl["p"]] + self.flat_state(fl) + [fl["step_dev"][:1]]

    def on_storages(self, live: list, gi: int = 0) -> bool:
        """No re-base of group `gi` since `capture_state` returned `live`."""
        return self._flat.get(gi, {}).get("p") is live[0]

    def _make_dev_state(self, fl, group):
        """step_dev = [step count, exchange stamp, ticket, pad].  Word 1 counts the carried steps (hcg_step_tail) this
        optimiser OBJECT has started and is carried over every re-base / `load_state_dict` (`_keep_stamp`): the one-shot
        exchange (xgmi.py) stamps its granules with it, and a stamp must never repeat although the step count may go
        back to a checkpoint's.  Word 2 is the plain update's ticket (hcg_adam_step_dev[_sse], hcg_update_dev), zero between
        launches."""
        if "step_dev" not in fl:
            dev = fl["p"].device
            stamps = getattr(self, "_stamps", {})
            fl["step_dev"] = torch.tensor([fl["step"], stamps.get(fl.get("gi", 0), 0), 0, 0], dtype=torch.int32, device=dev)
            fl["lr_dev"] = torch.tensor([float(group["lr"])], dtype=torch.float32, device=dev)
            fl["lr_host"] = float(group["lr"])

    def sync_lr(self):
        """Push param_groups' learning rates to the device words the captured update reads (host compare only
        when nothing changed)."""
        for gi, group in enumerate(self.param_groups):
            fl = self._flat.get(gi)
            if fl is not None and "lr_dev" in fl and fl["lr_host"] != float(group["lr"]):
                fl["lr_host"] = float(group["lr"])
                fl["lr_dev"].fill_(fl["lr_host"])

    def steps_done(self, gi: int = 0) -> int:
        fl = self._flat.get(gi)
        if fl is None:
            return 0
        if self._device_count() and "step_dev" in fl:
            return int(fl["step_dev"][0].item())     # synchronises
        return fl["step"]

    def load_state_dict(self, state_dict):
        """Restored state / step counts are copied into fresh flat buffers right away (torch's `load_state_dict` may
        alias the tensors of the dict it is given: a source optimizer that keeps stepping must not leak into this one)."""
        for gi in list(self._flat):
            self._keep_stamp(gi)
        super().load_state_dict(state_dict)
        self._flat = {}
        with torch.no_grad():
            for gi, group in enumerate(self.param_groups):
                ps = [p for p in group["params"] if p.requires_grad]
                if ps and all(p.is_cuda for p in ps):
                    fl = self._rebase(gi, group)
                    if self.capturable:
                        self._make_dev_state(fl, group)

    def state_dict(self):
        for gi, group in enumerate(self.param_groups):
            fl = self._flat.get(gi)
            if fl is not None and self._device_count():
                n = self.steps_done(gi)
                fl["step"] = n
                if self.KEEPS_STEP:
                    for p in fl["params"]:
                        self.state[p]["step"] = torch.tensor(float(n))
        return super().state_dict()

    def _keep_stamp(self, gi):
        """Remember the exchange stamp of a flat state that is about to be replaced (synchronises; re-bases are rare)."""
        old = self._flat.get(gi)
        if old is not None and "step_dev" in old:
            if not hasattr(self, "_stamps"):
                self._stamps = {}
            self._stamps[gi] = max(self._stamps.get(gi, 0), int(old["step_dev"][1].item()))

    def _rebase(self, gi, group):
        """Move the group's parameters and the rule's state onto flat buffers (in parameter order)."""
        self._keep_stamp(gi)
        ps = [p for p in group["params"] if p.requires_grad]
        dev = ps[0].device
        n = sum(p.numel() for p in ps)
        flat_p = torch.empty(n, dtype=torch.float32, device=dev)
        flat_s = {slot: torch.zeros(n, dtype=torch.float32, device=dev) for slot, _ in self.STATE}
        off = 0
        with torch.no_grad():
            for p in ps:
                if p.dtype != torch.float32:
                    raise _lib.HcgError(f"{type(self).__name__} handles float32 parameters only")
                k = p.numel()
                flat_p[off:off + k].copy_(p.reshape(-1))
                p.data = flat_p[off:off + k].view(p.shape)
                if self.STATE or self.KEEPS_STEP:      # (a rule without state leaves torch's `state` empty, as torch does)
                    st = self.state[p]
                    for slot, name in self.STATE:
                        if name in st:         # keep state restored by load_state_dict
                            flat_s[slot][off:off + k].copy_(st[name].reshape(-1))
                        st[name] = flat_s[slot][off:off + k].view(p.shape)
                    if self.KEEPS_STEP:
                        st.setdefault("step", torch.tensor(0.0))
                off += k
        step = int(self.state.get(ps[0], {}).get("step", 0)) if ps else 0
        self._flat[gi] = dict(params=ps, p=flat_p, n=n, gi=gi, step=step, **flat_s)
        return self._flat[gi]

    def _flat_of(self, gi, group, ps):
        fl = self._flat.get(gi)
        if fl is None or fl["params"] != ps or fl["p"].device != ps[0].device or ps[0].data_ptr() != fl["p"].data_ptr():
            with torch.no_grad():
                fl = self._rebase(gi, group)
        return fl

    def _push_lr(self, fl, group):
        lr = float(group["lr"])
        if fl["lr_host"] != lr:
            fl["lr_host"] = lr
            fl["lr_dev"].fill_(lr)

    def fused_update_ready(self, flat_grad: torch.Tensor):
        """Device word the head must advance (`step_counter` of hcg_head_fwd_bwd / hcg_fused_forward) if the NEXT update can be
        fused into the step's last launch (`step_with_reduction`), else None -- nothing is launched or changed here."""
        if not self.capturable or len(self.param_groups) != 1:
            return None
        group = self.param_groups[0]
        ps = [p for p in group["params"] if p.requires_grad]
        if not ps or not all(p.is_cuda for p in ps):
            return None
        fl = self._flat_of(0, group, ps)
        grads = [p.grad for p in ps]
        if any(g is None for g in grads) or not self._grads_flat(grads):
            return None
        if grads[0].data_ptr() != flat_grad.data_ptr() or flat_grad.numel() != fl["n"]:
            return None
        self._make_dev_state(fl, group)
        self._ready = (flat_grad.data_ptr(), fl)       # `step_with_reduction` of the same step need not ask again
        return fl["step_dev"]

    def step_with_reduction(self, jobs_addr: int, njobs: int, flat_grad: torch.Tensor, next_plan=None, exchange=None,
                            flat_ext=None, mode: str = "mean", loss_buf=None, loss_mode: int = _lib.HCG_LOSS_RMSE,
                            loss_count: float = 0.0) -> bool:
        """The step's last launch (hcg_step_tail): the backward's slab reductions, the loss with its deferred scale
        (`loss_mode`, `loss_count` = B * C; used when a job carries the head's SSE partials), this optimiser's update, and
        optionally the data-parallel exchange and the NEXT batch's plan.  `jobs_addr` = host address of the hcg_reduce_job
        array whose segments write `flat_grad` (the buffer the parameters' `.grad` are views of, in parameter order).  The
        step word returned by `fused_update_ready` must have been advanced earlier in this step (the head does).  Returns
        False -- nothing launched -- when the preconditions do not hold; the caller then issues reduction and update
        separately.  `next_plan`: a pointers-only blocked `BatchPlan`."""
        ready, self._ready = getattr(self, "_ready", None), None
        if (ready is not None and ready[0] == flat_grad.data_ptr() and self._flat.get(0) is ready[1]
                and self.capturable and len(self.param_groups) == 1):
            # `fused_update_ready(flat_grad)` answered earlier in this very step (the head launch in between advanced the
            # step word): same parameters, same flat buffers -- the walk over them is not repeated
            group, fl = self.param_groups[0], ready[1]
        else:
            if not self.capturable or len(self.param_groups) != 1:
                return False
            group = self.param_groups[0]
            ps = [p for p in group["params"] if p.requires_grad]
            if not ps or not all(p.is_cuda for p in ps):
                return False
            fl = self._flat_of(0, group, ps)
            grads = [p.grad for p in ps]
            if any(g is None for g in grads) or not self._grads_flat(grads):
                return False
            if grads[0].data_ptr() != flat_grad.data_ptr() or flat_grad.numel() != fl["n"]:
                return False
            self._make_dev_state(fl, group)
        b1, b2, eps = self._hparams(group)
        self._push_lr(fl, group)
        if next_plan is not None:
            np_ = next_plan
            if np_.mode != "blocked" or np_.has_csr or not np_.shared_status:
                raise _lib.HcgError("next_plan must be a pointers-only blocked plan built with validate=False")
        if exchange is not None:      # data parallel: the one-shot xGMI exchange sits between the reduction and the update
            if self.RULE != _lib.HCG_UPDATE_ADAM:
                raise _lib.HcgError("the one-shot exchange carries Adam's update only: use the RCCL form")
            if flat_ext is None or flat_ext.data_ptr() != flat_grad.data_ptr() or flat_ext.numel() != fl["n"] + 2 or loss_buf is None:
                raise _lib.HcgError("one-shot exchange: needs the extended flat buffer [gradients | SSE | count] and the loss buffer")
            exchange.launch(jobs_addr, njobs, flat_ext, fl, b1, b2, eps, mode, loss_buf, next_plan, loss_count=loss_count,
                            loss_mode=loss_mode)
            return True
        _lib.step_tail(jobs_addr, njobs, loss=loss_buf, loss_mode=loss_mode, loss_count=loss_count,
                       update=dict(rule=self.RULE, grad_flat=flat_grad, param=fl["p"], exp_avg=fl.get("m"),
                                   exp_avg_sq=fl.get("v"), n=fl["n"], lr_dev=fl["lr_dev"], step_dev=fl["step_dev"], beta1=b1,
                                   beta2=b2, eps=eps),
                       next_plan=next_plan)
        return True

    def _update_dev(self, fl, grad, group, loss=None):
        """The plain capturable update (hcg_update_dev) of this rule on the flat gradient `grad`."""
        b1, b2, eps = self._hparams(group)
        _lib.update_dev(grad, rule=self.RULE, param=fl["p"], exp_avg=fl.get("m"), exp_avg_sq=fl.get("v"), n=fl["n"],
                        lr_dev=fl["lr_dev"], step_dev=fl["step_dev"], beta1=b1, beta2=b2, eps=eps, loss=loss)

    def step_sse(self, flat_ext: torch.Tensor, loss_buf: torch.Tensor):
        """Data-parallel "sse" form (train.FusedTrainStep combine="sse"): `flat_ext` = [summed SSE/2-gradients | SSE |
        count], the parameters' `.grad` being views of its first n floats.  ONE launch scales the gradients in place to
        those of sqrt(MSE) over all ranks' graphs, stores that loss in `loss_buf[0:2]` and applies the update."""
        name = type(self).__name__
        if not self.capturable or len(self.param_groups) != 1:
            raise _lib.HcgError(f"{name}.step_sse needs the capturable mode and one parameter group")
        group = self.param_groups[0]
        ps = [p for p in group["params"] if p.requires_grad]
        _lib.require_gpu(*ps)
        fl = self._flat_of(0, group, ps)
        if flat_ext.numel() != fl["n"] + 2 or flat_ext.dtype != torch.float32 or not flat_ext.is_contiguous():
            raise _lib.HcgError(f"{name}.step_sse: the flat buffer must hold n gradients + [SSE, count]")
        self._make_dev_state(fl, group)
        self._push_lr(fl, group)
        self._update_dev(fl, flat_ext, group, loss=loss_buf)

    @staticmethod
    def _grads_flat(grads) -> bool:
        g0, off = grads[0], 0
        if not (g0.is_contiguous() and g0.dtype == torch.float32):
            return False
        base = g0.data_ptr()
        for g in grads:
            if g.dtype != torch.float32 or not g.is_contiguous() or g.data_ptr() != base + 4 * off:
                return False
            off += g.numel()
        return True

    @torch.no_grad()
    def step(self, closure=None):
        loss = None
        if closure is not None:
            with torch.enable_grad():
                loss = closure()
        lib = _lib.load()
        name = type(self).__name__
        for gi, group in enumerate(self.param_groups):
            ps = [p for p in group["params"] if p.requires_grad]
            if not ps:
                continue
            _lib.require_gpu(*ps)
            fl = self._flat_of(gi, group, ps)
            grads = [p.grad for p in ps]
            if any(g is None for g in grads):
                raise _lib.HcgError(f"{name}.step(): a parameter has no gradient")
            gflat = grads[0]
            if not self._grads_flat(grads):
                # per-tensor gradients (autograd path): ONE gather into a flat buffer, then the same single launch
                if any(g.dtype != torch.float32 for g in grads):
                    raise _lib.HcgError(f"{name} handles float32 gradients only")
                gflat = torch.cat([g.reshape(-1) for g in grads])
            stream = _lib.stream_ptr()
            if self._device_count():
                self._make_dev_state(fl, group)
                self._push_lr(fl, group)
                self._update_dev(fl, gflat, group)
                continue
            fl["step"] += 1
            step = fl["step"]
            self._host_update(lib, fl, gflat.data_ptr(), group, step, stream)
            for p in ps:
                self.state[p]["step"] = torch.tensor(float(step))
        return loss


class FusedAdam(FusedFlatOptimizer, torch.optim.Optimizer):
    RULE = _lib.HCG_UPDATE_ADAM
    STATE = (("m", "exp_avg"), ("v", "exp_avg_sq"))
    HOST_FORM = True

    def __init__(self, params, lr=1e-3, betas=(0.9, 0.999), eps=1e-8):
        if lr < 0 or eps < 0 or not (0 <= betas[0] < 1 and 0 <= betas[1] < 1):
            raise ValueError("invalid Adam hyper-parameters")
        super().__init__(params, dict(lr=lr, betas=betas, eps=eps))
        self._flat = {}      # group index -> dict(params, p, m, v flat tensors, n, step, device words)
        self.capturable = False

    def _hparams(self, group):
        (b1, b2), eps = group["betas"], float(group["eps"])
        return b1, b2, eps

    def _host_update(self, lib, fl, gptr, group, step, stream):
        b1, b2, eps = self._hparams(group)
        _lib.check(lib.hcg_adam_step(fl["p"].data_ptr(), gptr, fl["m"].data_ptr(), fl["v"].data_ptr(), fl["n"],
                                     float(group["lr"]), b1, b2, eps, step, stream), "hcg_adam_step")


def _refuse(name, **flags):
    """ValueError for every hyper-parameter whose value changes the rule the kernels implement."""
    bad = [k for k, v in flags.items() if v]
    if bad:
        raise ValueError(f"{name}: {', '.join(bad)} not supported (the fused update implements torch's default rule only)")


class FusedSGD(FusedFlatOptimizer, torch.optim.SGD):
    """torch.optim.SGD(params, lr) with momentum 0: p -= lr g.  torch keeps no per-parameter state for that rule."""
    RULE = _lib.HCG_UPDATE_SGD
    STATE = ()
    KEEPS_STEP = False

    def __init__(self, params, lr=1e-3, momentum=0, dampening=0, weight_decay=0, nesterov=False, *, maximize=False,
                 foreach=None, differentiable=False, fused=None):
        _refuse("FusedSGD", momentum=momentum != 0, dampening=dampening != 0, weight_decay=weight_decay != 0,
                nesterov=bool(nesterov), maximize=bool(maximize), foreach=bool(foreach), differentiable=bool(differentiable),
                fused=bool(fused))
        super().__init__(params, lr=lr)
        self._flat = {}
        self.capturable = False

    def _hparams(self, group):
        return 0.0, 0.0, 0.0


class FusedRMSprop(FusedFlatOptimizer, torch.optim.RMSprop):
    """torch.optim.RMSprop(params, lr, alpha, eps), not centered, momentum 0: v = alpha v + (1 - alpha) g^2,
    p -= lr g / (sqrt(v) + eps).  State `step` and `square_avg` as torch's.  The group's own `capturable` key stays False
    (torch's flag, so that a state dict stays loadable by torch.optim.RMSprop); the device mode is `enable_capturable()`."""
    RULE = _lib.HCG_UPDATE_RMSPROP
    STATE = (("v", "square_avg"),)

    def __init__(self, params, lr=1e-2, alpha=0.99, eps=1e-8, weight_decay=0, momentum=0, centered=False, capturable=False,
                 foreach=None, maximize=False, differentiable=False):
        _refuse("FusedRMSprop", weight_decay=weight_decay != 0, momentum=momentum != 0, centered=bool(centered),
                capturable=bool(capturable), foreach=bool(foreach), maximize=bool(maximize),
                differentiable=bool(differentiable))
        super().__init__(params, lr=lr, alpha=alpha, eps=eps)
        self._flat = {}
        self.capturable = False

    def _hparams(self, group):
        return 0.0, float(group["alpha"]), float(group["eps"])
