"""float64 torch restatement of what posegen_amd.pose_losses computes (include/posegen_hip.h): the key points of a
pose from axis-angle vectors and from rotation matrices, the two pose losses of the GAN loop, and the two lines of the loop built on
them.  Gradients come from torch's autograd through these formulas; nothing here is imported by the package.

  key points   l2w_0 = [R_0 | rest_0], l2w_j = l2w_parent(j) [R_j | rest_j - rest_parent(j)], kp_j = l2w_j[:3, 3]
               (get_smpl_l2ws / get_smpl_l2ws_torch, core/utils/skeleton_utils.py:379-463)
  axis-angle   the rotation vector -> unit quaternion -> matrix map of posegen_amd.skeleton.rotvec_to_matrix, with BOTH quaternion
               parts written as series in theta^2 below theta = 1e-3 (k = 1/2 - t/48 + t^2/3840, q_w = 1 - t/8 + t^2/384: cos(theta/2)
               to below 1e-22 there), so that autograd never differentiates sqrt at zero
  losses       run_gan.py:1898-1908 (train_spin: centre on joint 0, 14 joints, the prediction rescaled to the ground truth's Frobenius
               norm, 0.1 times the per-pose mean joint distance, poses at or above 0.02 dropped, the mean of the rest), :1924-1934 (the
               same without the drop) and mpjpe (:1458-1464) as train_gan uses it (:2085-2091)
"""
import numpy as np
import torch

from posegen_amd.skeleton import SMPLSkeleton, smpl_rest_pose

GAN_JOINTS = [1, 2, 4, 5, 7, 8, 12, 15, 16, 17, 18, 19, 20, 21]            # run_gan.py:1900, :2087
SMALL_ANGLE = 1e-3
KINDS = {"mpjpe": 0, "norm_matched": 1}


def t64(x):
    return x.to(torch.float64) if torch.is_tensor(x) else torch.as_tensor(np.asarray(x, dtype=np.float64))


def bone_offsets(rest_pose, scale=1.0, parents=None):
    """(offsets float64 [24,3] formed in the rest pose's own dtype as the package forms them, parents int64 [24])"""
    par = np.asarray(SMPLSkeleton.joint_trees if parents is None else parents).astype(np.int64)
    rp = np.asarray(smpl_rest_pose if rest_pose is None else rest_pose).reshape(24, 3)
    rp = rp * np.asarray(scale, dtype=rp.dtype)
    offs = rp.copy()
    offs[1:] = rp[1:] - rp[par[1:]]
    return offs.astype(np.float64), par


def rotvec_to_matrix(rv):
    """[...,3] float64 tensor -> [...,3,3]; differentiable everywhere, the zero vector included"""
    t2 = (rv * rv).sum(-1)
    small = torch.sqrt(t2.detach()) < SMALL_ANGLE          # the switch as the kernel takes it: on theta itself
    th = torch.sqrt(torch.where(small, torch.ones_like(t2), t2))
    k = torch.where(small, 0.5 - t2 / 48.0 + t2 * t2 / 3840.0, torch.sin(0.5 * th) / th)
    qw = torch.where(small, 1.0 - t2 / 8.0 + t2 * t2 / 384.0, torch.cos(0.5 * th))
    q = torch.cat([rv * k[..., None], qw[..., None]], -1)
    q = q / torch.sqrt((q * q).sum(-1, keepdim=True))
    x, y, z, w = q.unbind(-1)
    rows = [x * x - y * y - z * z + w * w, 2 * (x * y - z * w), 2 * (x * z + y * w),
            2 * (x * y + z * w), -x * x + y * y - z * z + w * w, 2 * (y * z - x * w),
            2 * (x * z - y * w), 2 * (y * z + x * w), -x * x - y * y + z * z + w * w]
    return torch.stack(rows, -1).reshape(rv.shape[:-1] + (3, 3))


def chain_kps(R, offs, par):
    """R [F,24,3,3] float64 tensor, offs [24,3], par [24] -> key points [F,24,3]"""
    offs = t64(offs)
    Rw, t = [R[:, 0]], [offs[0].expand(R.shape[0], 3)]
    for j in range(1, 24):
        p = int(par[j])
        Rw.append(Rw[p] @ R[:, j])
        t.append((Rw[p] @ offs[j]) + t[p])
    return torch.stack(t, 1)


def kps_from_axis_angle(bones, rest_pose=None, scale=1.0, parents=None):
    offs, par = bone_offsets(rest_pose, scale, parents)
    return chain_kps(rotvec_to_matrix(t64(bones)), offs, par)


def kps_from_rotmats(rotmats, rest_pose=None, scale=0.4, parents=None):
    offs, par = bone_offsets(smpl_rest_pose.astype(np.float32) if rest_pose is None else rest_pose, scale, parents)
    return chain_kps(t64(rotmats), offs, par)


def select(x, joints=None, root=None):
    x = t64(x)
    if root is not None and root >= 0:
        x = x - x[:, root:root + 1]
    return x if joints is None else x[:, list(joints)]


def pose_loss(pred, gt, joints=None, root=None, kind="mpjpe", weight=1.0, cap=float("inf")):
    """-> (loss 0-dim, per_pose [B], n_kept int)"""
    p, g = select(pred, joints, root), select(gt, joints, root)
    if kind == "norm_matched":
        s = torch.norm(g, dim=(-1, -2)) / torch.norm(p, dim=(-1, -2))
        p = s[:, None, None] * p
    elif kind != "mpjpe":
        raise ValueError(kind)
    per_pose = torch.norm(p - g, dim=-1).mean(-1) * weight
    keep = per_pose < cap if np.isfinite(cap) else torch.ones_like(per_pose, dtype=torch.bool)
    return per_pose[keep].mean(), per_pose, int(keep.sum())


def norm_matched_closed_form(p, g, c=1.0):
    """the closed forms of the header for one pose's selected, centred sets p, g [J,3] (numpy float64): (dp, dg) of c sum_j |s p_j - g_j|"""
    npn, ngn = np.sqrt((p * p).sum()), np.sqrt((g * g).sum())
    s = ngn / npn
    e = s * p - g
    d = np.sqrt((e * e).sum(-1, keepdims=True))
    u = np.divide(e, d, out=np.zeros_like(e), where=d != 0)
    a = (u * p).sum()
    return c * (s * u - s * a * p / npn ** 2), c * (-u + (a * g / (npn * ngn) if ngn != 0 else 0.0))


def as_float32_interface(x):
    """x as it crosses the C ABI in float32: the value rounded once, the cotangent that comes back rounded once too"""
    y = x + (x.detach().to(torch.float32).to(torch.float64) - x.detach())
    if y.requires_grad:
        y.register_hook(lambda gr: gr.to(torch.float32).to(torch.float64))
    return y


def generator_feedback(pred_kps, bones, rest_pose=None, scale=0.4):
    """run_gan.py:2032-2034, :2085-2091: 1 - mpjpe of the regressor's key points against the generator's, differentiable in `bones`
    (a float64 leaf).  The key points cross the ABI in float32 on their way into the loss."""
    rest = smpl_rest_pose.astype(np.float32) if rest_pose is None else rest_pose
    gt = as_float32_interface(kps_from_axis_angle(bones, rest, scale))
    return 1.0 - pose_loss(t64(pred_kps), gt, GAN_JOINTS, 0, "mpjpe")[0]


def regressor_loss(pred_rotmat, gt, gt_is_axis_angle=False, cap=0.02, weight=0.1):
    """run_gan.py:1896-1908 (gt: key points) and :1924-1934 (gt: axis-angle, cap = inf), differentiable in `pred_rotmat`"""
    rest = smpl_rest_pose.astype(np.float32)
    pred = as_float32_interface(kps_from_rotmats(pred_rotmat, rest, 0.4))
    if gt_is_axis_angle:
        gt = kps_from_axis_angle(t64(gt).detach(), rest, 0.4).detach().to(torch.float32)
    return pose_loss(pred, t64(gt), GAN_JOINTS, 0, "norm_matched", weight, cap)[0]
