"""Training on pose error, on the device: differentiable key points and the pose losses of the GAN loop.

The reference trains two networks on pose error.  `train_gan` adds `1 - mpjpe(pose, pose_gt)` to the generator's loss with
`pose_gt = get_smpl_l2ws_torch(outputs_axis_angle, scale=0.4)[..., :3, -1]` carrying the gradient (run_gan.py:2032-2034, 2085-2105);
`train_spin` trains the regressor through `get_smpl_l2ws_torch(pred_rotmat, axis_to_matrix=False)` and a norm-matched, capped mean
joint distance (:1886-1937).  There the kinematic chain is about ninety [B,4,4] matmuls per step and autograd runs their mirror
image.  Here each piece is one `torch.autograd.Function` whose backward is one call into the library (csrc/pg_kploss.hip):

  keypoints_from_axis_angle   forward `HipRenderer.pose_kinematics`, backward `pg_pose_kinematics_bwd`
  keypoints_from_rotmats      forward `HipRenderer.pose_kinematics_rot`, backward `pg_pose_kinematics_rot_bwd`
  pose_loss                   `pg_pose_loss`: the loss and its gradients in one call; backward scales them by the upstream gradient

All three are differentiable once (a double backward raises).  There is no torch fallback and no CPU path.  Not built: gradients
through the Procrustes alignments of `pose_eval`, through the SMPL body (`smpl.BodyModel`), and cotangents for skts / l2ws (the A-NeRF
training path has `poseopt.HipPoseOptLayer` for those).
"""
from __future__ import annotations

import ctypes as C
import math

import numpy as np
import torch
from torch.autograd.function import once_differentiable

from . import _ffi

LOSS_KINDS = {"mpjpe": _ffi.PG_POSE_LOSS_MPJPE, "norm_matched": _ffi.PG_POSE_LOSS_NORM_MATCHED}

# this module's clause of the refusal of a renderer that is not on a HIP device (_ffi.device_of)
NO_CPU = " (torch 'cuda:N'); key-point gradients and pose losses run in the library only,"


def _tree(rest_pose, scale, parents, root_parent: int):
    """(bone offsets float64 [24,3] in the rest pose's own dtype, parents int32 [24]) as the two forward calls form them"""
    from .skeleton import SMPLSkeleton
    par = np.ascontiguousarray(np.asarray(SMPLSkeleton.joint_trees if parents is None else parents, dtype=np.int32))
    par[0] = root_parent
    rp = np.asarray(rest_pose).reshape(24, 3)
    rp = rp * np.asarray(scale, dtype=rp.dtype)
    offs = rp.copy()
    offs[1:] = rp[1:] - rp[par[1:]]
    return np.ascontiguousarray(offs.astype(np.float64)), par, rp


class _AxisAngleFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, renderer, bones, rest_scaled, offs, par):
        b64 = bones.detach().to(device=renderer.device, dtype=torch.float64).contiguous()
        kps = renderer.pose_kinematics(b64, rest_scaled, parents=par)[0]
        ctx.renderer, ctx.tree, ctx.saved, ctx.meta = renderer, (offs, par), b64, (bones.dtype, bones.device)
        return kps

    @staticmethod
    @once_differentiable
    def backward(ctx, g_kps):
        r, (offs, par), b64 = ctx.renderer, ctx.tree, ctx.saved
        g = g_kps.to(device=r.device, dtype=torch.float32).contiguous()
        d_bones = torch.empty_like(b64)
        with torch.cuda.device(r.device):
            _ffi.call(r, "pg_pose_kinematics_bwd", b64.shape[0], b64, offs.ctypes.data_as(C.POINTER(C.c_double)),
                      par.ctypes.data_as(C.POINTER(C.c_int32)), g, d_bones)
        dtype, device = ctx.meta
        return None, d_bones.to(device=device, dtype=dtype), None, None, None


class _RotmatFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, renderer, rotmats, rest_pose, scale, offs, par):
        m32 = rotmats.detach().to(device=renderer.device, dtype=torch.float32).contiguous()
        kps = renderer.pose_kinematics_rot(m32, rest_pose, scale=scale, parents=par)[0]
        ctx.renderer, ctx.tree, ctx.saved, ctx.meta = renderer, (offs, par), m32, (rotmats.dtype, rotmats.device)
        return kps

    @staticmethod
    @once_differentiable
    def backward(ctx, g_kps):
        r, (offs, par), m32 = ctx.renderer, ctx.tree, ctx.saved
        g = g_kps.to(device=r.device, dtype=torch.float32).contiguous()
        d_rot = torch.empty_like(m32)
        with torch.cuda.device(r.device):
            _ffi.call(r, "pg_pose_kinematics_rot_bwd", m32.shape[0], m32, offs.ctypes.data_as(C.POINTER(C.c_double)),
                      par.ctypes.data_as(C.POINTER(C.c_int32)), g, d_rot)
        dtype, device = ctx.meta
        return None, d_rot.to(device=device, dtype=dtype), None, None, None, None


def keypoints_from_axis_angle(renderer, bones: torch.Tensor, rest_pose, scale: float = 1.0, parents=None) -> torch.Tensor:
    """bones [F,24,3] axis-angle (any dtype and device) -> device key points [F,24,3] float32, differentiable in `bones`:
    `get_smpl_l2ws_torch(bones, rest_pose, scale)[..., :3, -1]` (run_gan.py:2032-2034).  The forward is
    `renderer.pose_kinematics` on `rest_pose * scale` (in the rest pose's own dtype); the backward is pg_pose_kinematics_bwd, finite at a
    zero rotation vector.  The gradient comes back in the dtype and on the device of `bones`."""
    _ffi.device_of(renderer, "keypoints_from_axis_angle", NO_CPU)
    bones = torch.as_tensor(bones)
    if bones.dim() != 3 or tuple(bones.shape[1:]) != (24, 3):
        raise ValueError(f"keypoints_from_axis_angle: bones {tuple(bones.shape)}; [F,24,3] expected")
    offs, par, rest_scaled = _tree(rest_pose, scale, parents, 0)
    return _AxisAngleFn.apply(renderer, bones, rest_scaled, offs, par)


def keypoints_from_rotmats(renderer, rotmats: torch.Tensor, rest_pose=None, scale: float = 0.4) -> torch.Tensor:
    """rotmats [F,24,3,3] -> device key points [F,24,3] float32, differentiable in `rotmats` (the nine entries of a matrix are free
    variables; the matrices are used as given): `get_smpl_l2ws_torch(pred_rotmat, axis_to_matrix=False, scale=0.4)[:, :, :3, -1]`
    (run_gan.py:1897).  `rest_pose`: None = smpl_rest_pose in float32, as there.  Forward `renderer.pose_kinematics_rot`, backward
    pg_pose_kinematics_rot_bwd."""
    from .skeleton import smpl_rest_pose
    _ffi.device_of(renderer, "keypoints_from_rotmats", NO_CPU)
    rotmats = torch.as_tensor(rotmats)
    if rotmats.dim() != 4 or tuple(rotmats.shape[1:]) != (24, 3, 3):
        raise ValueError(f"keypoints_from_rotmats: rotmats {tuple(rotmats.shape)}; [F,24,3,3] expected")
    rest = smpl_rest_pose.astype(np.float32) if rest_pose is None else rest_pose
    offs, par, _ = _tree(rest, scale, None, -1)
    return _RotmatFn.apply(renderer, rotmats, rest, scale, offs, par)


class _PoseLossFn(torch.autograd.Function):
    """(loss, per_pose, n_kept) of pg_pose_loss; the gradients of `loss` are computed in the same call and kept for backward"""

    @staticmethod
    def forward(ctx, renderer, pred, gt, joints, J, root, kind, weight, cap):
        dev = renderer.device
        p32 = pred.detach().to(device=dev, dtype=torch.float32).contiguous()
        g32 = gt.detach().to(device=dev, dtype=torch.float32).contiguous()
        B, J_in = p32.shape[:2]
        need_p, need_g = ctx.needs_input_grad[1], ctx.needs_input_grad[2]
        d_pred = torch.empty_like(p32) if need_p else None
        d_gt = torch.empty_like(g32) if need_g else None
        summary = torch.empty(3, dtype=torch.float64, device=dev)
        per_pose = torch.empty(B, dtype=torch.float64, device=dev)
        jarr = None if joints is None else (C.c_int32 * J)(*joints)
        with torch.cuda.device(dev):
            _ffi.call(renderer, "pg_pose_loss", B, J_in, p32, g32, jarr, J, root, kind, float(weight), float(cap), per_pose, summary,
                      d_pred, d_gt)
        ctx.grads = (d_pred, d_gt)
        ctx.meta = ((pred.dtype, pred.device), (gt.dtype, gt.device))
        loss, n_kept = summary[0], summary[1]
        ctx.mark_non_differentiable(per_pose, n_kept)
        return loss, per_pose, n_kept

    @staticmethod
    @once_differentiable
    def backward(ctx, g_loss, _g_per_pose, _g_kept):
        out = []
        for d, (dtype, device) in zip(ctx.grads, ctx.meta):
            out.append(None if d is None else (d.to(torch.float64) * g_loss.to(device=d.device, dtype=torch.float64)).to(device=device, dtype=dtype))
        return (None, out[0], out[1]) + (None,) * 6


def pose_loss(pred_kps, gt_kps, *, joints=None, root=None, kind: str = "mpjpe", weight: float = 1.0, cap: float = math.inf,
              renderer=None, return_stats: bool = False):
    """The pose loss of the GAN loop as a 0-dim float64 device tensor, differentiable in whichever of `pred_kps`, `gt_kps` [B,J_in,3]
    requires a gradient (pg_pose_loss).  Rows `joints` (None: all) after row `root` (None: nothing) is subtracted; per pose
    `weight` times the mean joint distance -- kind "mpjpe" (run_gan.py:1458-1464) -- or the same after the prediction is rescaled to the
    ground truth's Frobenius norm -- kind "norm_matched" (:1902-1906).  A finite `cap` keeps the poses strictly below it (:1907-1908) and
    the loss is the mean over those: NaN when none is kept, with zero gradients.  `return_stats`: also per_pose float64 [B] and n_kept
    (a float64 device scalar; nothing synchronises).  `renderer`: the `HipRenderer` to run on; None = the `pose_eval` module's own on
    the key points' device (host tensors without a renderer raise NotImplementedError)."""
    from . import pose_eval
    if kind not in LOSS_KINDS:
        raise ValueError(f"pose_loss: kind = {kind!r}, not one of {sorted(LOSS_KINDS)}")
    pred_kps, gt_kps = torch.as_tensor(pred_kps), torch.as_tensor(gt_kps)
    if pred_kps.dim() != 3 or pred_kps.shape[2] != 3 or pred_kps.shape != gt_kps.shape or pred_kps.shape[0] < 1 or pred_kps.shape[1] < 1:
        raise ValueError(f"pose_loss: pred {tuple(pred_kps.shape)} and gt {tuple(gt_kps.shape)} must both be [B,J,3]")
    joints, J, root = pose_eval.PoseScorer._check_selection(int(pred_kps.shape[1]), joints, root)
    if joints is not None and len(set(joints)) != len(joints):
        raise ValueError("pose_loss: a joint is selected twice")
    weight, cap = float(weight), float(cap)
    if math.isnan(weight) or math.isnan(cap) or cap <= 0.0:
        raise ValueError(f"pose_loss: weight = {weight}, cap = {cap} (no NaN; cap > 0)")
    if renderer is None:
        renderer = pose_eval._scorer_for(None, pred_kps, gt_kps).renderer
    dev = _ffi.device_of(renderer, "pose_loss", NO_CPU)
    for t in (pred_kps, gt_kps):
        if t.is_cuda and t.device != dev:
            raise NotImplementedError(f"pose_loss: key points on {t.device}, the renderer on {dev}")
    loss, per_pose, n_kept = _PoseLossFn.apply(renderer, pred_kps, gt_kps, joints, J, root, LOSS_KINDS[kind], weight, cap)
    return (loss, per_pose, n_kept) if return_stats else loss

