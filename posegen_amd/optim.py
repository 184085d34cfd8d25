"""The optimiser step on the device (include/posegen_optim.h): `HipAdam`, a `torch.optim.Optimizer` whose `step`
is one `pg_adam_step` call per device -- `clip_grad_norm_` over the parameters that have a gradient and `torch.optim.Adam`'s update of
every one of them -- in place of the chain of stock operators the five training loops ended in.

It keeps `torch.optim.Adam`'s layout: the `param_groups` carry the keys of the installed torch's Adam, `state[p]` is {'step': a 0-dim
float32 CPU tensor, 'exp_avg', 'exp_avg_sq'}, so a `state_dict()` loads into `torch.optim.Adam` and the reverse, and the reference's
`optimizer_state_dict` checkpoints load.  There is no CPU path: a parameter on the host is refused.

Not built: AdamW / decoupled decay, amsgrad, maximize, capturable, differentiable, other optimisers, 16-bit parameter copies,
per-group clipping (the norm is over every tensor of the call, as `clip_grad_norm_(parameters)` is).
"""
from __future__ import annotations

from typing import Optional

import torch

from . import _ffi
from .discriminators import _renderer_for

REFUSED = ("amsgrad", "maximize", "capturable", "differentiable", "decoupled_weight_decay")
IGNORED = ("foreach", "fused")
NO_CPU = ":"


def _refuse_options(group, who: str):
    for k in REFUSED:
        if group.get(k):
            raise NotImplementedError(f"{who}: {k}=True is not built (the device step is torch.optim.Adam with amsgrad=False, maximize=False, "
                                      "coupled weight_decay, outside graph capture and autograd)")


def _host_step(step) -> torch.Tensor:
    """`step` as torch.optim.Adam keeps it by default: a 0-dim float32 tensor on the host"""
    if isinstance(step, torch.Tensor):
        return step.detach().to("cpu", torch.float32).reshape(())
    return torch.tensor(float(step), dtype=torch.float32)


class HipAdam(torch.optim.Optimizer):
    """`torch.optim.Adam` (amsgrad=False, maximize=False, coupled L2 weight_decay) with its step on the device.

    `step(max_norm=c)` clips the gradients of this optimiser's parameters to a total 2-norm of c first, as
    `clip_grad_norm_(params, c)` would, and returns the norm before clipping.  `foreach` and `fused` are accepted and ignored.
    `renderer`: the `HipRenderer` whose handle the call goes through (None: the pose scorer's own on the parameters' device)."""

    def __init__(self, params, lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=0, renderer=None, **options):
        # torch's own checks of the hyperparameters, and the installed torch's keys
        defaults = dict(torch.optim.Adam([torch.zeros(1)], lr=lr, betas=betas, eps=eps, weight_decay=weight_decay).defaults)
        for k, v in options.items():
            if k not in defaults:
                raise TypeError(f"HipAdam: unknown option {k!r}")
            defaults[k] = v
        _refuse_options(defaults, "HipAdam")
        self.renderer = renderer
        self._tables = {}                 # device -> the ctypes tables kept between calls
        self.last_norm_coef = None        # the device [2] float64 of the last clipped step: norm before clipping, coefficient
        super().__init__(params, defaults)

    @classmethod
    def adopt(cls, optimizer: torch.optim.Optimizer, renderer=None) -> "HipAdam":
        """A `HipAdam` on `optimizer`'s param_groups and state (a `torch.optim.Adam`; the tensors and the group dicts are shared, not
        copied), the way `HipHMR.adopt` takes a model."""
        if type(optimizer) is not torch.optim.Adam:
            raise NotImplementedError(f"HipAdam.adopt: {type(optimizer).__name__} is not torch.optim.Adam (AdamW and other optimisers are not built)")
        d = optimizer.defaults
        self = cls(optimizer.param_groups, lr=d["lr"], betas=d["betas"], eps=d["eps"], weight_decay=d["weight_decay"], renderer=renderer,
                   **{k: d[k] for k in REFUSED + IGNORED if k in d})
        self.state = optimizer.state
        self._steps_to_host()
        return self

    def _steps_to_host(self):
        for st in self.state.values():
            if "step" in st and not (isinstance(st["step"], torch.Tensor) and st["step"].device.type == "cpu" and st["step"].dtype == torch.float32
                                     and st["step"].dim() == 0):
                st["step"] = _host_step(st["step"])

    def load_state_dict(self, state_dict):
        super().load_state_dict(state_dict)
        for group in self.param_groups:
            _refuse_options(group, "HipAdam.load_state_dict")
        self._steps_to_host()             # (a fused or capturable Adam keeps `step` on the device: moved once, here)
        self._tables = {}

    def _check(self, p, g):
        who = "HipAdam.step"
        for t, what in ((p, "parameter"), (g, "gradient")):
            if t.is_sparse:
                raise NotImplementedError(f"{who}: a sparse {what} is not built")
            if t.dtype != torch.float32:
                raise NotImplementedError(f"{who}: a {t.dtype} {what} is not built (float32 only)")
            if not t.is_contiguous():
                raise NotImplementedError(f"{who}: a non-contiguous {what} is not built")
        if g.device != p.device or g.shape != p.shape:
            raise NotImplementedError(f"{who}: a gradient of shape {tuple(g.shape)} on {g.device} for a parameter of shape {tuple(p.shape)} on {p.device}")

    @torch.no_grad()
    def step(self, closure=None, max_norm: Optional[float] = None, write_grads: bool = False):
        """One Adam step of every parameter that has a gradient (the others are left out of the call and of the norm, and their
        `step` does not move).  `max_norm`: clip the total 2-norm of those gradients first; `write_grads`: also leave the clipped
        gradients in `.grad`.  Returns the norm before clipping as a 0-dim float64 device tensor when `max_norm` is given (one per
        device in a dict when the parameters are on several), else the closure's loss.  Nothing synchronises."""
        loss = None
        if closure is not None:
            with torch.enable_grad():
                loss = closure()
        per_device = {}
        for gi, group in enumerate(self.param_groups):
            _refuse_options(group, "HipAdam.step")
            for p in group["params"]:
                g = p.grad
                if g is None:
                    continue
                if not p.is_cuda:
                    raise NotImplementedError(f"HipAdam.step: a parameter on {p.device}, not on a HIP device{NO_CPU} there is no CPU path")
                self._check(p, g)
                st = self.state[p]
                if len(st) == 0:
                    st["step"] = torch.tensor(0.0, dtype=torch.float32)
                    st["exp_avg"] = torch.zeros_like(p, memory_format=torch.preserve_format)
                    st["exp_avg_sq"] = torch.zeros_like(p, memory_format=torch.preserve_format)
                per_device.setdefault(p.device, []).append((p, g, st, gi))
        norms = {}
        for device, items in per_device.items():
            renderer = _renderer_for(self.renderer, items[0][0], "HipAdam.step")
            norms[device] = self._device_step(renderer, device, items, max_norm, write_grads)
        if max_norm is None:
            return loss
        if len(norms) == 1:
            return next(iter(norms.values()))
        return norms

    def _device_step(self, renderer, device, items, max_norm, write_grads):
        n = len(items)
        if n > _ffi.PG_ADAM_MAX_TENSORS or len(self.param_groups) > _ffi.PG_ADAM_MAX_GROUPS:
            raise NotImplementedError(f"HipAdam.step: {n} tensors in {len(self.param_groups)} groups (at most {_ffi.PG_ADAM_MAX_TENSORS} in "
                                      f"{_ffi.PG_ADAM_MAX_GROUPS} per call)")
        tb = self._tables.get(device)
        if tb is None or len(tb["tab"]) < n or len(tb["groups"]) != len(self.param_groups):
            cap = max(n, 16)
            tb = {"tab": (_ffi.PgAdamTensor * cap)(), "groups": (_ffi.PgAdamGroup * len(self.param_groups))(), "sig": [None] * cap,
                  "grad": [None] * cap, "step": [(None, None)] * cap}
            self._tables[device] = tb
        tab, sig, grads, steps = tb["tab"], tb["sig"], tb["grad"], tb["step"]
        for k, group in enumerate(self.param_groups):           # lr (and whatever else a schedule moves) is read on every call
            q = tb["groups"][k]
            q.lr, (q.beta1, q.beta2), q.eps, q.weight_decay = float(group["lr"]), group["betas"], float(group["eps"]), float(group["weight_decay"])
        for i, (p, g, st, gi) in enumerate(items):
            e = tab[i]
            m, v = st["exp_avg"], st["exp_avg_sq"]
            s = (p.data_ptr(), m.data_ptr(), v.data_ptr(), p.numel(), gi)
            if sig[i] != s:                                      # only what changed is rewritten
                if m.device != device or v.device != device or m.dtype != torch.float32 or v.dtype != torch.float32 \
                        or not m.is_contiguous() or not v.is_contiguous() or m.numel() != p.numel() or v.numel() != p.numel():
                    raise NotImplementedError("HipAdam.step: exp_avg / exp_avg_sq must be contiguous float32 tensors of the parameter's size on its device")
                e.param, e.exp_avg, e.exp_avg_sq, e.count, e.group = s
                sig[i] = s
            gp = g.data_ptr()
            if grads[i] != gp:                                   # (a new tensor after zero_grad(set_to_none=True))
                e.grad = gp
                grads[i] = gp
            step = st["step"]
            if steps[i][0] is not step:                          # the count moves through a numpy view of the host tensor: no torch operator
                steps[i] = (step, step.numpy())
            view = steps[i][1]
            view[...] = view + 1.0
            e.step = int(view)
        clip = max_norm is not None
        with torch.cuda.device(device):
            out = torch.empty(2, dtype=torch.float64, device=device) if clip else None
            _ffi.call(renderer, "pg_adam_step", n, tab, len(self.param_groups), tb["groups"],
                      float(max_norm) if clip else _ffi.PG_ADAM_NO_CLIP, int(bool(write_grads)), out)
        if clip:
            self.last_norm_coef = out
            return out[0]
        return None
