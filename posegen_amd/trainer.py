"""The A-NeRF training step on the HIP path: the reference's `Trainer` (core/trainer.py:207-485).

`HipTrainer` takes the reference Trainer's constructor arguments and has its `train_batch(batch, i, global_step)`: pose arguments from
the batch or from `popt_kwargs['popt_layer']` (a `HipPoseOptLayer`), the forward through `posegen_amd.render.render` with
`render_kwargs_train` (whose 'ray_caster' is a `TrainableRayCaster`), `compute_loss` from `train_losses.photometric_loss` and
`pose_regulariser`, `optimize` (backward, gradient norms, the optimisers' steps), the learning-rate decay and `update_embed_fns`.  The
optimisers stay `torch.optim`.  Logging, checkpoint writing and config parsing stay with the caller.

Differences from the reference, deliberate:
  * the gradient norms are taken before `zero_grad` in both branches of `optimize`; the reference's pose branch reads them after it
    (trainer.py:473-475), so it reports zeros -- and with torch 2's `set_to_none` it fails;
  * `decay_optimizer_lrate` reads `optimizer.state[...]['step']` every iteration; here the count of optimiser steps is kept on the
    host, initialised once from the optimiser's state;
  * stats are packed into one device vector: `train_batch` returns Python floats from ONE device-to-host copy (`fetch=True`), or the
    device vector with its names and no synchronisation (`fetch=False`);
  * `opt_pose_cache`, `reg_fn` L1 / MSE and pose refinement without `opt_rot6d` are refused.
"""
from __future__ import annotations

import numpy as np
import torch

from . import train_losses
from .render import render


def decayed_lrate(lrate: float, lrate_decay: float, decay_rate: float, optim_steps: int, decay_unit: int = 1000) -> float:
    """`decay_optimizer_lrate`'s formula (core/trainer.py:175-185) for a count of optimiser steps"""
    return lrate * (decay_rate ** ((int(optim_steps) // int(decay_unit)) / lrate_decay))


def temporal_indices(kp_idx, n_poses: int):
    """(previous, next) pose of every entry for the temporal term (trainer.py:412-413): `kp_idx - 1`, where -1 means the last pose as
    numpy indexing gives the reference, and `(kp_idx + 1) % n_poses`"""
    idx = np.asarray(kp_idx, dtype=np.int64)
    prev = idx - 1
    return np.where(prev < 0, prev + n_poses, prev), (idx + 1) % n_poses


class HipTrainer:
    """Drop-in for the reference's `Trainer` (same constructor); see the module docstring.  `args` needs what the reference reads:
    loss_fn, loss_beta, reg_fn, reg_coef, use_background, coarse_weight, opt_pose, opt_pose_stop, opt_pose_step, opt_pose_tol,
    opt_pose_coef, opt_rot6d, use_temp_loss, temp_coef, ext_scale, opt_framecode, chunk, lrate, lrate_decay, lrate_decay_rate,
    decay_unit, finetune (and what `update_embed_fns` reads)."""

    def __init__(self, args, data_attrs, optimizer, pose_optimizer, render_kwargs_train, render_kwargs_test, popt_kwargs=None, device=None):
        if getattr(args, "opt_pose_cache", False):
            raise NotImplementedError("HipTrainer: opt_pose_cache is not built on the HIP path (HipPoseOptLayer has no cache)")
        train_losses.check_loss_settings(args.loss_fn, getattr(args, "reg_fn", None), getattr(args, "loss_beta", 0.1))
        self.has_popt = popt_kwargs is not None and popt_kwargs.get("popt_layer") is not None
        if self.has_popt and getattr(args, "opt_pose", False) and not getattr(args, "opt_rot6d", False):
            raise NotImplementedError("HipTrainer: the pose regulariser is built for opt_rot6d (every shipped opt_pose config sets it)")
        self.args = args
        self.optimizer, self.pose_optimizer = optimizer, pose_optimizer
        self.render_kwargs_train, self.render_kwargs_test = render_kwargs_train, render_kwargs_test
        self.popt_kwargs = popt_kwargs
        self.device = device
        self.hwf = data_attrs["hwf"]
        self.data_attrs = data_attrs
        self.optim_steps = self._steps_of(optimizer)         # host-side count of optimiser steps (one read of the state, here)

    @staticmethod
    def _steps_of(optimizer) -> int:
        if optimizer is None:
            return 0
        state = optimizer.state.get(optimizer.param_groups[0]["params"][0], {})
        return int(state.get("step", 0))

    @property
    def ray_caster(self):
        rc = self.render_kwargs_train["ray_caster"]
        return getattr(rc, "module", rc)

    # ---- the batch ---------------------------------------------------------------------------------------------------------------
    @staticmethod
    def _kp_idx_host(batch) -> np.ndarray:
        idx = getattr(batch, "kp_idx_host", None)
        if idx is None:                                      # (a plain dict: one copy back, as the reference's kp_idx.cpu().numpy())
            idx = batch["kp_idx"]
            idx = idx.cpu().numpy() if torch.is_tensor(idx) else np.asarray(idx)
        return np.asarray(idx, dtype=np.int64)

    def get_fwd_args(self, batch):
        return {"rays": batch["rays"], "cams": batch["cam_idxs"] if getattr(self.args, "opt_framecode", False) else None,
                "subject_idxs": batch.get("subject_idxs", None)}

    def get_kp_args(self, batch, detach=False):
        """human pose data from the batch or from the pose layer (trainer.py:287-314): (kp_args for the caster, extras for the loss)"""
        if not self.has_popt:
            return {"kp_batch": batch["kp3d"], "skts": batch["skts"], "bones": batch["bones"], "cyls": batch["cyls"]}, {}
        kps, bones, skts, _, rots = self.popt_kwargs["popt_layer"](self._kp_idx_host(batch))
        kp_args = {"kp_batch": kps, "skts": skts, "bones": bones, "cyls": batch["cyls"]}
        extras = {"rots": rots}
        if detach:
            kp_args = {k: v.detach() for k, v in kp_args.items() if v is not None}
            extras = {k: v.detach() for k, v in extras.items()}
        return kp_args, extras

    # ---- the loss ----------------------------------------------------------------------------------------------------------------
    def compute_loss(self, batch, preds, kp_opts=None, popt_detach=False):
        """(loss_dict, stats) of 0-dim float64 device tensors; only `total_loss` carries a gradient (trainer.py:321-353)"""
        args = self.args
        r = self.ray_caster.renderer
        loss_dict, stats = train_losses.photometric_loss(
            preds, batch, loss_fn=args.loss_fn, loss_beta=getattr(args, "loss_beta", 0.1), use_background=args.use_background,
            coarse_weight=getattr(args, "coarse_weight", 1.0), reg_fn=getattr(args, "reg_fn", None), reg_coef=getattr(args, "reg_coef", 0.0),
            renderer=r)
        if not popt_detach:
            total, terms = self._compute_kp_loss(batch, kp_opts, r)
            total_loss = loss_dict.pop("total_loss") + total
            stats["MPJPC"] = terms.pop("MPJPC")
            loss_dict.update(terms)
            loss_dict["total_loss"] = total_loss
        return loss_dict, stats

    def _compute_kp_loss(self, batch, kp_opts, renderer):
        args = self.args
        idx = self._kp_idx_host(batch)
        temporal = None
        if getattr(args, "use_temp_loss", False):
            layer = self.popt_kwargs["popt_layer"]
            prev, nxt = temporal_indices(idx, layer.N_kps)
            with torch.no_grad():                            # the neighbours are constants of the regulariser (trainer.py:427-428)
                pk, _, _, _, pr = layer(prev)
                nk, _, _, _, nr = layer(nxt)
            temporal = dict(prev_rots=pr, prev_kps=pk, next_rots=nr, next_kps=nk, temp_val=batch["temp_val"], temp_coef=args.temp_coef)
        return train_losses.pose_regulariser(kp_opts["rots"], kp_opts["kp_batch"], idx, self.popt_kwargs["popt_anchors"],
                                             tol=args.opt_pose_tol, coef=args.opt_pose_coef, ext_scale=args.ext_scale, temporal=temporal,
                                             renderer=renderer)

    # ---- the update --------------------------------------------------------------------------------------------------------------
    def optimize(self, loss, i, popt_detach=False):
        """backward, the gradient norms (before any zero_grad), the optimisers' steps (trainer.py:453-485)"""
        loss.backward()
        total_norm, avg_norm, _ = train_losses.grad_norms(self.ray_caster, self.ray_caster.renderer)
        self.optimizer.step()
        self.optimizer.zero_grad()
        self.optim_steps += 1
        if not popt_detach and i % self.args.opt_pose_step == 0:         # poses move after enough gradient accumulation
            self.pose_optimizer.step()
            self.pose_optimizer.zero_grad()
        return {"total_norm": total_norm, "avg_norm": avg_norm}

    def decay_optimizer_lrate(self):
        args = self.args
        new_lrate = decayed_lrate(args.lrate, args.lrate_decay, args.lrate_decay_rate, self.optim_steps, getattr(args, "decay_unit", 1000))
        for group in self.optimizer.param_groups:
            group["lr"] = new_lrate
        return new_lrate

    def train_batch(self, batch, i=0, global_step=0, fetch=True):
        """One training step on `batch` (a `RayBatch` of `RayBatchSource`, taken as it is: its tensors are on the device).
        fetch=True: `(loss_dict, stats)` of Python floats, read with one device-to-host copy.  fetch=False: `(values, names, host)`,
        `values` the float64 device vector of every loss and stat in the order of `names`, `host` = lrate and cutoff, which never
        were on the device; nothing synchronises."""
        args = self.args
        H, W, focal = self.hwf
        stop = getattr(args, "opt_pose_stop", None)
        popt_detach = not (stop is None or i < stop)
        kp_args, extra_args = self.get_kp_args(batch, detach=popt_detach)
        fwd_args = self.get_fwd_args(batch)
        preds = render(H, W, focal, chunk=args.chunk, **kp_args, **fwd_args, **self.render_kwargs_train)
        no_pose = popt_detach or not getattr(args, "opt_pose", False) or not self.has_popt
        loss_dict, stats = self.compute_loss(batch, preds, kp_opts={**kp_args, **extra_args}, popt_detach=no_pose)
        stats.update(self.optimize(loss_dict["total_loss"], i, no_pose))
        host = {"lrate": self.decay_optimizer_lrate()}
        caster = self.ray_caster
        if not getattr(args, "finetune", False):
            caster.update_embed_fns(global_step, args)
        host["cutoff"] = caster.embed_fn.get_tau()
        names = list(loss_dict) + list(stats)
        values = torch.stack([v.detach() for v in loss_dict.values()] + [v.detach() for v in stats.values()])
        if not fetch:
            return values, names, host
        flat = dict(zip(names, values.cpu().tolist()))
        return {k: flat[k] for k in loss_dict}, {**host, **{k: flat[k] for k in stats}}
