"""What an A-NeRF training step optimises, on the device: the reference Trainer's losses, pose regulariser and
gradient norms (core/trainer.py:193-205, 321-443).

Between the ray caster's maps and `loss.backward()` the reference runs a chain of small torch operators -- composite on the
background, loss, PSNR, a masked BCE, each for two passes; the 6-D bone difference with a tolerance mask and `lerp`; the temporal
term; their autograd mirror images; three `.item()` syncs -- and `get_gradnorm` one `norm` launch and one `.item()` sync per
parameter tensor.  Here each piece is one call into the library (csrc/pg_trainloss.hip) that produces the values and the gradients
together, wrapped as a `torch.autograd.Function` whose backward scales the stored gradients by the upstream gradient:

  photometric_loss    `pg_train_loss`: both passes' loss (MSE / L1 / Huber), BCE regulariser, PSNR, alpha; 2 launches
  pose_regulariser    `pg_pose_reg_loss`: kp_loss with tolerance, temporal term, MPJPC; 2 launches
  grad_norms          `pg_grad_norms`: total, average and per-tensor norms of up to 256 gradients; 2 launches, no sync

float64 inside, no atomics, every sum in a fixed order.  All are differentiable once (a double backward raises).  There is no torch
fallback and no CPU path.
"""
from __future__ import annotations

import ctypes as C
import math
from typing import Dict, Optional

import numpy as np
import torch
from torch.autograd.function import once_differentiable

from . import _ffi

LOSS_KINDS = {"MSE": _ffi.PG_TRAIN_LOSS_MSE, "L1": _ffi.PG_TRAIN_LOSS_L1, "Huber": _ffi.PG_TRAIN_LOSS_HUBER}
REG_KINDS = {None: _ffi.PG_TRAIN_REG_NONE, "BCE": _ffi.PG_TRAIN_REG_BCE}
REG_REFUSAL = ("reg_fn = {0!r} is refused: the reference calls it with reduction='off', which img2l1 / img2mse do not know and answer "
               "with the unreduced [n] tensor, so its total_loss has shape [n] and backward() raises; only reg_fn = 'BCE' trains there")
SUMMARY = ("total_loss", "rgb_loss", "rgb_loss0", "reg_loss", "reg_loss0", "psnr", "psnr0", "alpha", "n_bce", "n_bce0")

# this module's clause of the refusal of a renderer that is not on a HIP device (_ffi.device_of)
NO_CPU = " (torch 'cuda:N'); the training losses run in the library only,"


def check_loss_settings(loss_fn, reg_fn, loss_beta=0.1):
    """The settings `pg_train_loss` takes, refused on the host before any tensor is touched: (loss kind, reg kind)."""
    if reg_fn in ("L1", "MSE"):
        raise ValueError("photometric_loss: " + REG_REFUSAL.format(reg_fn))
    if reg_fn not in REG_KINDS:
        raise NotImplementedError(f"photometric_loss: reg_fn = {reg_fn!r}, not one of None, 'BCE'")
    if loss_fn not in LOSS_KINDS:
        raise NotImplementedError(f"photometric_loss: loss_fn = {loss_fn!r}, not one of {sorted(LOSS_KINDS)}")
    if loss_fn == "Huber" and not float(loss_beta) >= 0.0:
        raise ValueError(f"photometric_loss: loss_beta = {loss_beta} (smooth-L1 needs beta >= 0)")
    return LOSS_KINDS[loss_fn], REG_KINDS[reg_fn]


def _on_device(t, dev, who, name):
    if t is not None and t.device != dev:
        raise NotImplementedError(f"{who}: {name} is on {t.device}, the renderer on {dev}")
    return t


def _f32(t):
    return None if t is None else t.detach().to(dtype=torch.float32).contiguous()


def _scaled(grads, meta, g_total):
    """the stored gradients times the upstream gradient, in each input's dtype (None where the input wanted none)"""
    out = []
    for d, m in zip(grads, meta):
        if d is None:
            out.append(None)
        else:
            out.append((d * g_total.to(device=d.device, dtype=d.dtype)).reshape(m[0]).to(dtype=m[1]))
    return out


class _PhotometricFn(torch.autograd.Function):
    """the summary entries of pg_train_loss; the gradients of `total` are computed in the same call and kept for backward"""

    @staticmethod
    def forward(ctx, renderer, rgb_map, acc_map, rgb0, acc0, target, bgs, fgs, kinds, scalars):
        maps = [_f32(t) for t in (rgb_map, acc_map, rgb0, acc0)]
        n = maps[1].numel()
        dev = maps[0].device
        need = [t is not None and ctx.needs_input_grad[1 + i] for i, t in enumerate(maps)]
        grads = [torch.empty_like(t) if w else None for t, w in zip(maps, need)]
        summary = torch.empty(len(SUMMARY), dtype=torch.float64, device=dev)
        target, bgs, fgs = _f32(target), _f32(bgs), _f32(fgs)
        loss_kind, reg_kind = kinds
        beta, use_background, coarse_weight, reg_coef, base_bg = scalars
        with torch.cuda.device(dev):
            _ffi.call(renderer, "pg_train_loss", n, *maps, target, bgs, float(base_bg), fgs, loss_kind, float(beta), int(bool(use_background)),
                      float(coarse_weight), reg_kind, float(reg_coef), summary, *grads)
        ctx.grads = grads
        ctx.meta = [None if t is None else (tuple(t.shape), t.dtype) for t in (rgb_map, acc_map, rgb0, acc0)]
        outs = tuple(summary[i] for i in range(len(SUMMARY)))
        ctx.mark_non_differentiable(*outs[1:])
        return outs

    @staticmethod
    @once_differentiable
    def backward(ctx, g_total, *_unused):
        return (None,) + tuple(_scaled(ctx.grads, ctx.meta, g_total)) + (None,) * 5


def photometric_loss(preds: Dict[str, torch.Tensor], batch, *, loss_fn: str, loss_beta: float = 0.1, use_background: bool = True,
                     coarse_weight: float = 1.0, reg_fn: Optional[str] = None, reg_coef: float = 0.0, base_bg: float = 1.0, renderer=None):
    """`Trainer._compute_nerf_loss` for `preds['rgb_map']` / `['acc_map']` and, when present, `['rgb0']` / `['acc0']`, summed as
    `compute_loss` sums them (core/trainer.py:321-383): `(loss_dict, stats)` with the reference's keys -- rgb_loss, rgb_loss0, reg_loss,
    reg_loss0 (those that exist), total_loss; psnr, psnr0, alpha -- every value a 0-dim float64 device tensor, nothing synchronised.
    Only `total_loss` carries a gradient, to whichever of the four maps requires one (the reference backpropagates nothing else).
    `batch`: target_s [n,3], fgs [n,1] (with reg_fn), bgs [n,3] (optional: otherwise the scalar `base_bg`).  reg_fn 'L1' / 'MSE' are
    refused (see REG_REFUSAL).  With BCE and no ray of fgs < 1 the regulariser and the total are NaN and its gradient zero."""
    kinds = check_loss_settings(loss_fn, reg_fn, loss_beta)
    dev = _ffi.device_of(renderer, "photometric_loss", NO_CPU)
    who = "photometric_loss"
    rgb, acc = _on_device(preds["rgb_map"], dev, who, "rgb_map"), _on_device(preds["acc_map"], dev, who, "acc_map")
    rgb0, acc0 = (_on_device(preds[k], dev, who, k) for k in ("rgb0", "acc0")) if "rgb0" in preds else (None, None)
    n = acc.numel()
    target = _on_device(batch["target_s"], dev, who, "target_s")
    bgs = _on_device(batch["bgs"], dev, who, "bgs") if use_background and "bgs" in batch else None
    fgs = _on_device(batch["fgs"], dev, who, "fgs")[..., 0] if reg_fn is not None else None
    for name, t, numel in (("rgb_map", rgb, 3 * n), ("rgb0", rgb0, 3 * n), ("acc0", acc0, n), ("target_s", target, 3 * n), ("bgs", bgs, 3 * n),
                           ("fgs", fgs, n)):
        if t is not None and t.numel() != numel:
            raise ValueError(f"photometric_loss: {name} {tuple(t.shape)} for {n} rays")
    if n < 1:
        raise ValueError("photometric_loss: no rays")
    out = _PhotometricFn.apply(renderer, rgb, acc, rgb0, acc0, target, bgs, fgs, kinds, (loss_beta, use_background, coarse_weight, reg_coef, base_bg))
    v = dict(zip(SUMMARY, out))
    loss_dict = {"rgb_loss": v["rgb_loss"]}
    stats = {"psnr": v["psnr"]}
    if reg_fn is not None:
        loss_dict["reg_loss"] = v["reg_loss"]
    if rgb0 is not None:
        loss_dict["rgb_loss0"] = v["rgb_loss0"]
        stats["psnr0"] = v["psnr0"]
        if reg_fn is not None:
            loss_dict["reg_loss0"] = v["reg_loss0"]
    loss_dict["total_loss"] = v["total_loss"]
    stats["alpha"] = v["alpha"]
    return loss_dict, stats


def check_kp_idx(kp_idx_host, n: int, N: int) -> np.ndarray:
    """`kp_idx` as the contiguous host int32 [n] the library takes; an entry outside [0, N) is an IndexError before anything is launched"""
    idx = np.asarray(kp_idx_host.detach().cpu() if torch.is_tensor(kp_idx_host) else kp_idx_host).reshape(-1)
    if idx.size and not np.issubdtype(idx.dtype, np.integer):
        raise TypeError(f"pose_regulariser: kp_idx must be integers, not {idx.dtype}")
    if idx.size != n:
        raise ValueError(f"pose_regulariser: {idx.size} pose indices for {n} rays")
    if idx.size and (idx.min() < 0 or idx.max() >= N):
        bad = int(np.flatnonzero((idx < 0) | (idx >= N))[0])
        raise IndexError(f"pose_regulariser: kp_idx[{bad}] = {int(idx[bad])} is outside [0, {N})")
    return np.ascontiguousarray(idx, dtype=np.int32)


class _PoseRegFn(torch.autograd.Function):
    """(total, kp_loss, temp_loss, MPJPC) of pg_pose_reg_loss; d_rots / d_kps are written by the same call"""

    @staticmethod
    def forward(ctx, renderer, rots, kps, idx, a_rots, a_kps, temporal, scalars):
        r32, k32 = _f32(rots), _f32(kps)
        dev = r32.device
        n = r32.shape[0]
        d_rots = torch.empty_like(r32) if ctx.needs_input_grad[1] else None
        d_kps = torch.empty_like(k32) if ctx.needs_input_grad[2] else None
        summary = torch.empty(4, dtype=torch.float64, device=dev)
        tol, coef, ext_scale, temp_coef = scalars
        keep = [_f32(a_rots), _f32(a_kps)] + [_f32(t) for t in (temporal or (None,) * 5)]
        with torch.cuda.device(dev):
            _ffi.call(renderer, "pg_pose_reg_loss", n, r32, k32, keep[0].shape[0], keep[0], keep[1], idx.ctypes.data_as(C.POINTER(C.c_int32)),
                      float(tol), float(coef), float(ext_scale), *keep[2:], float(temp_coef), summary, d_rots, d_kps)
        ctx.grads = (d_rots, d_kps)
        ctx.meta = [(tuple(rots.shape), rots.dtype), (tuple(kps.shape), kps.dtype)]
        outs = (summary[3], summary[0], summary[1], summary[2])
        ctx.mark_non_differentiable(*outs[1:])
        return outs

    @staticmethod
    @once_differentiable
    def backward(ctx, g_total, *_unused):
        return (None,) + tuple(_scaled(ctx.grads, ctx.meta, g_total)) + (None,) * 5


def pose_regulariser(rots, kps, kp_idx_host, anchors, *, tol: float, coef: float, ext_scale: float, temporal: Optional[dict] = None,
                     renderer=None):
    """`Trainer._compute_kp_loss` for opt_rot6d (core/trainer.py:384-443): `(total, terms)`, total = kp_loss + temp_loss a 0-dim float64
    device tensor differentiable in `rots` [n,24,3,3] and `kps` [n,24,3] (the pose layer's per-ray outputs), `terms` = kp_loss,
    temp_loss (with `temporal`), MPJPC beside it without a gradient.  `anchors`: dict of device tensors rots [N,24,3,3], kps [N,24,3]
    (popt_anchors); `kp_idx_host` [n]: host integers into them (`RayBatch.kp_idx_host`), checked here.  `temporal`: dict of prev_rots,
    prev_kps, next_rots, next_kps (per ray, constants), temp_val [n] and temp_coef."""
    who = "pose_regulariser"
    rots, kps = torch.as_tensor(rots), torch.as_tensor(kps)
    if rots.dim() != 4 or tuple(rots.shape[1:]) != (24, 3, 3) or tuple(kps.shape) != (rots.shape[0], 24, 3) or rots.shape[0] < 1:
        raise ValueError(f"{who}: rots {tuple(rots.shape)} / kps {tuple(kps.shape)}; [n,24,3,3] and [n,24,3] expected")
    a_rots, a_kps = anchors["rots"], anchors["kps"]
    if a_rots.dim() != 4 or tuple(a_rots.shape[1:]) != (24, 3, 3) or tuple(a_kps.shape) != (a_rots.shape[0], 24, 3):
        raise ValueError(f"{who}: anchors rots {tuple(a_rots.shape)} / kps {tuple(a_kps.shape)}; [N,24,3,3] and [N,24,3] expected")
    n = rots.shape[0]
    idx = check_kp_idx(kp_idx_host, n, a_rots.shape[0])
    temp, temp_coef = None, 0.0
    if temporal is not None:
        temp = tuple(temporal[k] for k in ("prev_rots", "prev_kps", "next_rots", "next_kps", "temp_val"))
        temp_coef = float(temporal["temp_coef"])
        for t, shape in zip(temp, ((n, 24, 3, 3), (n, 24, 3), (n, 24, 3, 3), (n, 24, 3), (n,))):
            if tuple(t.shape) != shape:
                raise ValueError(f"{who}: a temporal tensor is {tuple(t.shape)}, {shape} expected")
    if any(math.isnan(float(x)) for x in (tol, coef, temp_coef)) or not float(ext_scale) > 0.0:
        raise ValueError(f"{who}: tol = {tol}, coef = {coef}, temp_coef = {temp_coef}, ext_scale = {ext_scale} (no NaN; ext_scale > 0)")
    dev = _ffi.device_of(renderer, who, NO_CPU)
    for name, t in (("rots", rots), ("kps", kps), ("anchors['rots']", a_rots), ("anchors['kps']", a_kps)) + tuple(("temporal", t) for t in temp or ()):
        _on_device(t, dev, who, name)
    total, kp_loss, temp_loss, mpjpc = _PoseRegFn.apply(renderer, rots, kps, idx, a_rots, a_kps, temp, (tol, coef, ext_scale, temp_coef))
    terms = {"kp_loss": kp_loss, "MPJPC": mpjpc}
    if temporal is not None:
        terms["temp_loss"] = temp_loss
    return total, terms


@torch.no_grad()
def grad_norms(module_or_params, renderer):
    """`get_gradnorm` (core/trainer.py:193-205) in one call: `(total_norm, avg_norm, per_tensor)` as float64 device tensors, nothing
    synchronised.  Parameters whose `.grad` is None are skipped and not counted, as in the reference; with no gradient at all (the
    reference divides by zero) it raises.  One stated difference: the reference rounds each tensor's norm to float32 before squaring."""
    params = module_or_params.parameters() if hasattr(module_or_params, "parameters") else module_or_params
    grads = [p.grad for p in params if p.grad is not None]
    if not grads:
        raise ValueError("grad_norms: no parameter has a gradient (the reference divides by zero here)")
    dev = _ffi.device_of(renderer, "grad_norms", NO_CPU)
    keep = []
    for g in grads:
        _on_device(g, dev, "grad_norms", "a gradient")
        if g.dtype != torch.float32:
            raise NotImplementedError(f"grad_norms: a {g.dtype} gradient (float32 only)")
        keep.append(g if g.is_contiguous() else g.contiguous())
    k = len(keep)
    ptrs = (C.c_void_p * k)(*[g.data_ptr() for g in keep])
    counts = (C.c_int64 * k)(*[g.numel() for g in keep])
    out = torch.empty(2 + k, dtype=torch.float64, device=dev)
    with torch.cuda.device(dev):
        _ffi.call(renderer, "pg_grad_norms", k, ptrs, counts, out)
    return out[0], out[1], out[2:]
