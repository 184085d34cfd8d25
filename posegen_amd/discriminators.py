"""The adversarial game of the PoseGen loop on the device (include/posegen_gan.h, csrc/pg_disc.hip).

`train_gan` runs three things on every batch of 1024 poses (run_gan.py:1956-2135): `get_adv_loss` (the discriminator on real and
generated poses, backward into the generator's output), `train_dis` (the discriminator on real and pooled fake poses, backward into
its 7.09 M parameters) and `Sample_from_Pool` (a Python loop over 1024 host arrays).  As torch ops the discriminator is about 70
launches forward and several times that backward.  Here:

  HipPos3dDiscriminator / HipPos2dDiscriminator / PartDiscriminator
                        nn.Modules whose submodules are real nn.Linears under the reference's names (so a reference checkpoint loads
                        with strict=True, `apply(init_weights)`, Adam and clip_grad_norm_ work unchanged); the Linears are never
                        called: forward is one autograd.Function over pg_disc_forward / pg_disc_backward (five launches forward)
  adversarial_loss      get_adv_loss:  0.5 mse(D(fake), 1)
  discriminator_loss    train_dis:     0.5 (mse(D(real), 1) + mse(D(fake), 0))
                        both with get_discriminator_accuracy's two numbers as device tensors (pg_disc_loss); nothing synchronises
  FakePool              Sample_from_Pool on the device: host draws in the reference's order, one pg_pool_exchange launch

Differentiable once.  There is no torch fallback and no CPU path: inputs on a CPU device raise NotImplementedError.  The generators
are `generators.py`.  Not built: Adam, clipping, 16-bit operands.
"""
from __future__ import annotations

import ctypes as C
from typing import List, Optional, Sequence, Tuple

import numpy as np
import torch
import torch.nn as nn
from torch.autograd.function import once_differentiable

from . import _ffi

LAYER_NAMES = ("layer_1", "layer_2", "layer_3", "layer_last", "layer_pred")

# this module's clause of the refusal of tensors that are not on a HIP device
POOL_MAX_ITEMS = 8192                      # items of one pg_pool_exchange call (include/posegen_gan.h)

NO_CPU =" (torch 'cuda:N'); the discriminators, their loss and the pool run in the library only,"


class PartSpec:
    """What a `PartDiscriminator` is made of.  `paths`: (name, selected rows, width, mid) in the order of the output columns; a name
    "" puts the five Linears on the module itself (Pos2dDiscriminator).  `module_order`: the names in the order the submodules are
    created (the reference's __init__ order, which is the state dict's); None = the order of `paths`."""

    def __init__(self, n_points: int, point_dim: int, paths: Sequence[Tuple[str, Sequence[int], int, int]], slope: float = 0.01,
                 module_order: Optional[Sequence[str]] = None):
        self.n_points, self.point_dim, self.slope = int(n_points), int(point_dim), float(slope)
        self.paths = [(str(name), [int(j) for j in sel], int(width), int(mid)) for name, sel, width, mid in paths]
        self.module_order = [p[0] for p in self.paths] if module_order is None else [str(n) for n in module_order]
        if not 1 <= len(self.paths) <= _ffi.PG_DISC_MAX_PATHS:
            raise ValueError(f"PartSpec: {len(self.paths)} paths; 1 .. {_ffi.PG_DISC_MAX_PATHS} expected")
        if not 1 <= self.n_points <= _ffi.PG_DISC_MAX_POINTS or self.point_dim not in (2, 3):
            raise ValueError(f"PartSpec: n_points = {self.n_points} (1 .. {_ffi.PG_DISC_MAX_POINTS}), point_dim = {self.point_dim} (2 or 3)")
        if sorted(self.module_order) != sorted(p[0] for p in self.paths) or len(set(self.module_order)) != len(self.paths):
            raise ValueError("PartSpec: module_order does not name every path once")
        if not (np.isfinite(self.slope) and self.slope >= 0.0):
            # the backward reads LeakyReLU's mask off the tape's sign, which a negative slope turns round
            raise ValueError(f"PartSpec: slope = {self.slope}; a finite slope >= 0 expected")
        for name, sel, width, mid in self.paths:
            if not 1 <= len(sel) <= self.n_points or min(sel) < 0 or max(sel) >= self.n_points or width < 1 or mid < 1:
                raise ValueError(f"PartSpec: path {name!r}: rows {sel}, width {width}, mid {mid}")

    def layer_shapes(self, p: int) -> List[Tuple[int, int]]:
        """(out, in) of the five Linears of path p"""
        _, sel, width, mid = self.paths[p]
        return [(width, len(sel) * self.point_dim), (width, width), (width, width), (mid, width), (1, mid)]

    def tape_layout(self, B: int) -> List[List[Tuple[int, int]]]:
        """per path the (offset, columns) of its four tape layers in a tape over B rows (include/posegen_gan.h)"""
        out, at = [], 0
        for _, _, width, mid in self.paths:
            layers = []
            for n in (width, width, width, mid):
                layers.append((at, n))
                at += B * n
            out.append(layers)
        return out

    def c_spec(self) -> _ffi.PgDiscSpec:
        s = _ffi.PgDiscSpec(n_paths=len(self.paths), n_points=self.n_points, point_dim=self.point_dim, slope=self.slope)
        for p, (_, sel, width, mid) in enumerate(self.paths):
            s.path[p].n_sel, s.path[p].width, s.path[p].mid = len(sel), width, mid
            for i, j in enumerate(sel):
                s.path[p].sel[i] = j
        return s


def pos3d_spec() -> PartSpec:
    """Pos3dDiscriminator (run_gan.py:1003-1026): seven Disc_Joint_Path(n, 500, 1000) over SMPL joint subsets; output columns in
    forward's order, submodules in __init__'s"""
    parts = [("layer_left_leg", [4, 7, 10]), ("layer_right_leg", [5, 8, 11]), ("layer_left_arm", [9, 13, 16, 18, 20, 22]),
             ("layer_right_arm", [9, 14, 17, 19, 21, 23]), ("layer_torso", [0, 1, 2, 3, 6, 9, 13, 14, 16, 17]), ("layer_head", [9, 12, 15]),
             ("layer_full_body", list(range(24)))]
    order = ["layer_left_leg", "layer_right_leg", "layer_left_arm", "layer_right_arm", "layer_head", "layer_torso", "layer_full_body"]
    return PartSpec(24, 3, [(n, sel, 500, 1000) for n, sel in parts], module_order=order)


def pos2d_spec() -> PartSpec:
    """Pos2dDiscriminator (run_gan.py:1028-1046): one path 48 -> 1000 -> 1000 -> 1000 -> 100 -> 1 whose Linears sit on the module"""
    return PartSpec(24, 2, [("", list(range(24)), 1000, 100)])


def _renderer_for(renderer, t: torch.Tensor, who: str):
    """the `HipRenderer` whose handle the calls go through: the given one, else the `pose_eval` module's own on the tensor's device"""
    if not t.is_cuda:
        raise NotImplementedError(f"{who}: a tensor on {t.device}, not on a HIP device{NO_CPU} there is no CPU path")
    if renderer is None:
        from . import pose_eval
        renderer = pose_eval.default_scorer(t.device).renderer
    dev = _ffi.device_of(renderer, who, NO_CPU)
    if t.device != dev:
        raise NotImplementedError(f"{who}: a tensor on {t.device}, the renderer on {dev}")
    return renderer


def _pointer_table(spec: PartSpec, tensors) -> _ffi.PgDiscParams:
    """pg_disc_params / pg_disc_grads of `tensors` (path-major, per path w1, b1, .. w5, b5; None = a null pointer)"""
    tab = _ffi.PgDiscParams()
    for p in range(len(spec.paths)):
        for l in range(_ffi.PG_DISC_LAYERS):
            w, b = tensors[(p * _ffi.PG_DISC_LAYERS + l) * 2], tensors[(p * _ffi.PG_DISC_LAYERS + l) * 2 + 1]
            tab.w[p][l] = None if w is None else w.data_ptr()
            tab.b[p][l] = None if b is None else b.data_ptr()
    return tab


class _DiscFn(torch.autograd.Function):
    """pred [B,n_paths] of pg_disc_forward; the tape is kept for pg_disc_backward when anything needs a gradient"""

    @staticmethod
    def forward(ctx, renderer, spec, x, *params):
        B = x.shape[0]
        cspec, ctab = spec.c_spec(), _pointer_table(spec, params)
        pred = torch.empty(B, len(spec.paths), dtype=torch.float32, device=x.device)
        tape = None
        if any(ctx.needs_input_grad):
            n = C.c_int64(0)
            renderer._check(renderer.lib.pg_disc_tape_floats(C.byref(cspec), B, C.byref(n)))
            tape = torch.empty(n.value, dtype=torch.float32, device=x.device)
        with torch.cuda.device(x.device):
            _ffi.call(renderer, "pg_disc_forward", C.byref(cspec), C.byref(ctab), x, B, pred, tape)
        ctx.renderer, ctx.spec = renderer, spec
        ctx.save_for_backward(x, tape, *params)
        return pred

    @staticmethod
    @once_differentiable
    def backward(ctx, g_pred):
        renderer, spec = ctx.renderer, ctx.spec
        x, tape, *params = ctx.saved_tensors
        B = x.shape[0]
        d_pred = g_pred.to(torch.float32).contiguous()
        d_x = torch.empty_like(x) if ctx.needs_input_grad[2] else None
        want = ctx.needs_input_grad[3:]
        grads = [torch.empty_like(p) if w else None for p, w in zip(params, want)]
        gtab = _pointer_table(spec, grads) if any(want) else None
        cspec, ctab = spec.c_spec(), _pointer_table(spec, params)
        with torch.cuda.device(x.device):
            _ffi.call(renderer, "pg_disc_backward", C.byref(cspec), C.byref(ctab), x, B, tape, d_pred, d_x,
                      None if gtab is None else C.byref(gtab))
        return (None, None, d_x) + tuple(grads)


class _JointPath(nn.Module):
    """Disc_Joint_Path's parameters under its names; never called"""

    def __init__(self, shapes):
        super().__init__()
        for name, (n_out, n_in) in zip(LAYER_NAMES, shapes):
            setattr(self, name, nn.Linear(n_in, n_out))


class PartDiscriminator(nn.Module):
    """Independent five-layer LeakyReLU MLPs over row subsets of a pose: x [B,n_points,point_dim] (any shape with those elements per
    row) -> [B,n_paths] float32 on the device, one column per path.  The parameters are nn.Linears (`[out,in]` float32, read by the
    library where torch keeps them); forward asks pg_disc_backward for d_x and for parameter gradients only where autograd needs
    them, so with `requires_grad` off on the parameters no weight-gradient product runs.  `renderer`: the `HipRenderer` to run on;
    None = the `pose_eval` module's own on the input's device."""

    def __init__(self, spec: PartSpec, renderer=None):
        super().__init__()
        self.spec, self.renderer = spec, renderer
        by_name = {p[0]: i for i, p in enumerate(spec.paths)}
        for name in spec.module_order:
            shapes = spec.layer_shapes(by_name[name])
            if name == "":
                for lname, (n_out, n_in) in zip(LAYER_NAMES, shapes):
                    setattr(self, lname, nn.Linear(n_in, n_out))
            else:
                setattr(self, name, _JointPath(shapes))

    def path_linears(self, p: int) -> List[nn.Linear]:
        owner = self if self.spec.paths[p][0] == "" else getattr(self, self.spec.paths[p][0])
        return [getattr(owner, n) for n in LAYER_NAMES]

    def _flat_params(self) -> List[torch.Tensor]:
        out = []
        for p in range(len(self.spec.paths)):
            for lin in self.path_linears(p):
                out += [lin.weight, lin.bias]
        return out

    def forward(self, x: torch.Tensor) -> torch.Tensor:
        who = type(self).__name__
        x = torch.as_tensor(x)
        renderer = _renderer_for(self.renderer, x, who)
        row = self.spec.n_points * self.spec.point_dim
        if x.numel() == 0 or x.numel() % row:
            raise ValueError(f"{who}: input {tuple(x.shape)}; rows of {self.spec.n_points} x {self.spec.point_dim} values expected")
        params = self._flat_params()
        for t in params:
            if t.device != x.device or t.dtype != torch.float32 or not t.is_contiguous():
                raise NotImplementedError(f"{who}: a parameter on {t.device} as {t.dtype}; contiguous float32 on {x.device} expected")
        x = x.to(torch.float32).reshape(-1, self.spec.n_points, self.spec.point_dim).contiguous()
        return _DiscFn.apply(renderer, self.spec, x, *params)


class HipPos3dDiscriminator(PartDiscriminator):
    """Pos3dDiscriminator (run_gan.py:1003-1026): poses [B,24,3] -> [B,7]; columns left leg, right leg, left arm, right arm, torso,
    head, full body; state dict keys `layer_left_leg.layer_1.weight` ... in the reference's order"""

    def __init__(self, renderer=None):
        super().__init__(pos3d_spec(), renderer)


class HipPos2dDiscriminator(PartDiscriminator):
    """Pos2dDiscriminator (run_gan.py:1028-1046): poses [B,24,2] (or [B,48]) -> [B,1]; keys `layer_1.weight` ... `layer_pred.bias`"""

    def __init__(self, renderer=None):
        super().__init__(pos2d_spec(), renderer)


# ---- the loss ------------------------------------------------------------------------------------------------------------------------------
class _DiscLossFn(torch.autograd.Function):
    """(weight mse(pred, label), the count of |pred - label| <= 0.5, n) of pg_disc_loss; d_pred comes from the same call"""

    @staticmethod
    def forward(ctx, renderer, pred, label, weight):
        p32 = pred.detach().to(torch.float32).contiguous()
        out = torch.empty(3, dtype=torch.float64, device=p32.device)
        d_pred = torch.empty_like(p32) if ctx.needs_input_grad[1] else None
        with torch.cuda.device(p32.device):
            _ffi.call(renderer, "pg_disc_loss", p32, p32.numel(), float(label), float(weight), out, d_pred)
        ctx.d_pred, ctx.dtype = d_pred, pred.dtype
        loss, count, n = out[0], out[1], out[2]
        ctx.mark_non_differentiable(count, n)
        return loss, count, n

    @staticmethod
    @once_differentiable
    def backward(ctx, g_loss, _g_count, _g_n):
        d = ctx.d_pred
        return None, None if d is None else (d * g_loss.to(torch.float32)).to(ctx.dtype), None, None


def lsgan_loss(pred: torch.Tensor, label: float, weight: float = 1.0, renderer=None):
    """(`weight` mse(pred, label) as a differentiable float64 device scalar, the accuracy of get_discriminator_accuracy against the same
    label as a float64 device scalar) over all values of `pred` (pg_disc_loss)"""
    renderer = _renderer_for(renderer, pred, "lsgan_loss")
    loss, count, n = _DiscLossFn.apply(renderer, pred, label, weight)
    return loss, count / n


def _accuracy(pred: torch.Tensor, label: float, renderer) -> torch.Tensor:
    with torch.no_grad():
        return lsgan_loss(pred, label, 1.0, renderer)[1]


def adversarial_loss(disc: PartDiscriminator, real: Optional[torch.Tensor], fake: torch.Tensor, accuracies: bool = False):
    """get_adv_loss (run_gan.py:1117-1140): the generator's adversarial loss 0.5 mse(D(fake), 1), differentiable in `fake` (and in the
    discriminator's parameters where they require it).  Returns (loss, real_acc, fake_acc): the accuracies as the reference logs them
    -- D(real) against 1, D(fake) against 0 -- as device scalars, or None unless `accuracies`; the real pass runs only then.  Nothing
    synchronises."""
    pred_fake = disc(fake)
    r = _renderer_for(disc.renderer, pred_fake, "adversarial_loss")
    loss, _ = lsgan_loss(pred_fake, 1.0, 0.5, r)
    if not accuracies:
        return loss, None, None
    with torch.no_grad():
        real_acc = _accuracy(disc(real), 1.0, r)
    return loss, real_acc, _accuracy(pred_fake.detach(), 0.0, r)


def discriminator_loss(disc: PartDiscriminator, real: torch.Tensor, fake: torch.Tensor):
    """train_dis's loss (run_gan.py:1152-1166): 0.5 (mse(D(real), 1) + mse(D(fake), 0)) with the two accuracies, (loss, real_acc,
    fake_acc), all device scalars.  Both sets go through the discriminator as one batch (a row's prediction does not depend on the
    batch around it), each half has its own mean."""
    row = disc.spec.n_points * disc.spec.point_dim
    real, fake = torch.as_tensor(real), torch.as_tensor(fake)
    n_real = real.numel() // row
    pred = disc(torch.cat([real.reshape(-1, row).to(torch.float32), fake.reshape(-1, row).to(torch.float32)]))
    r = _renderer_for(disc.renderer, pred, "discriminator_loss")
    loss_real, real_acc = lsgan_loss(pred[:n_real], 1.0, 0.5, r)
    loss_fake, fake_acc = lsgan_loss(pred[n_real:], 0.0, 0.5, r)
    return loss_real + loss_fake, real_acc, fake_acc


# ---- the pool ------------------------------------------------------------------------------------------------------------------------------
def pool_draws(capacity: int, cur: int, n: int, rng=None):
    """The draws `Sample_from_Pool.__call__` consumes for n items on a pool holding `cur` of `capacity` (run_gan.py:584-599), in its
    order: nothing while the pool fills; then per item `ranf()`, and `randint(0, capacity)` only if that was above 0.5.  `rng`: an
    object with ranf / randint (np.random.RandomState); None = the global `np.random`, as the reference.  -> (swap uint8 [n], slot
    int32 [n])"""
    rng = np.random if rng is None else rng
    ranf = rng.ranf if hasattr(rng, "ranf") else rng.random_sample
    swap, slot = np.zeros(n, np.uint8), np.zeros(n, np.int32)
    for i in range(n):
        if cur + i < capacity:
            continue
        if ranf() > 0.5:
            swap[i], slot[i] = 1, rng.randint(0, capacity)
    return swap, slot


class FakePool:
    """Sample_from_Pool (run_gan.py:578-599) with the pool on the device.  `pool(items, rng)` draws on the host in the reference's
    order, uploads the draws (one pinned array, one asynchronous copy) and calls pg_pool_exchange; `pool.exchange(items, swap, slot)`
    takes the draws directly.  items [n, ...] float32 on the device -> what the reference's call returns, same shape; at most 8192
    items a call."""

    def __init__(self, capacity: int = 4096, renderer=None):
        if int(capacity) < 1:
            raise ValueError(f"FakePool: capacity = {capacity}")
        self.capacity, self.renderer = int(capacity), renderer
        self.cur = 0
        self.pool: Optional[torch.Tensor] = None

    def __call__(self, items: torch.Tensor, rng=None) -> torch.Tensor:
        swap, slot = pool_draws(self.capacity, self.cur, int(items.shape[0]), rng)
        return self.exchange(items, swap, slot)

    def exchange(self, items: torch.Tensor, swap, slot) -> torch.Tensor:
        items = torch.as_tensor(items)
        r = _renderer_for(self.renderer, items, "FakePool")
        n = int(items.shape[0])
        if n < 1:
            raise ValueError("FakePool: no items")
        if n > POOL_MAX_ITEMS:
            raise ValueError(f"FakePool: {n} items in one call; at most {POOL_MAX_ITEMS} (pg_pool_exchange)")
        flat = items.detach().to(torch.float32).reshape(n, -1).contiguous()
        row = int(flat.shape[1])
        if self.pool is None:
            self.pool = torch.zeros(self.capacity, row, dtype=torch.float32, device=flat.device)
        if self.pool.shape[1] != row or self.pool.device != flat.device:
            raise ValueError(f"FakePool: items of {row} values on {flat.device}; the pool holds rows of {self.pool.shape[1]} on {self.pool.device}")
        if torch.is_tensor(swap) and torch.is_tensor(slot) and swap.is_cuda and slot.is_cuda:
            d_swap, d_slot = swap.to(torch.uint8).contiguous(), slot.to(torch.int32).contiguous()
        else:
            # slots then flags in one pinned array: torch's host allocator hands the block out again only after the copy has run
            host = torch.empty(5 * n, dtype=torch.uint8, pin_memory=True)
            host[:4 * n].view(torch.int32).copy_(torch.as_tensor(np.asarray(slot, dtype=np.int32).reshape(n)))
            host[4 * n:].copy_(torch.as_tensor(np.asarray(swap, dtype=np.uint8).reshape(n)))
            dev = host.to(flat.device, non_blocking=True)
            d_slot, d_swap = dev[:4 * n].view(torch.int32), dev[4 * n:]
        out = torch.empty_like(flat)
        with torch.cuda.device(flat.device):
            _ffi.call(r, "pg_pool_exchange", self.pool, self.capacity, row, self.cur, flat, n, d_swap, d_slot, out)
        self.cur = min(self.capacity, self.cur + n)
        return out.reshape(items.shape)
