"""The render call of the PoseGen GAN loop, kept on the device (BASELINE config 5).

In the reference every `run_render` call of the training loop (run_gan.py:2041-2091, 2299-2337)
  * re-parses the arguments and re-loads the A-NeRF checkpoint (load_nerf, run_gan.py:135-165),
  * moves the generator's poses to the host, runs the kinematics and the bounding-box cull in numpy,
  * renders rpi = 20 frames through nn.DataParallel(RayCaster),
  * writes them as PNG files, reads them back, crops [100:412]^2, normalises, and resizes to 224 x 224
    with skimage (anti_aliasing=True) for the SPIN / HMR regressor.
The adversarial game that runs on every batch -- the pose discriminators, their losses and the pool of generated poses -- is
`discriminators.py`; `generator_adversarial_loss` and `discriminator_step` below are the loop's two call sites of it.  The pose
generator itself is `generators.py`; `generator_step` is the generator half of a batch.  The regressor's head is `regressors.py`;
`regressor_step` is one batch of `train_spin`.

`render_for_regressor` is that call with the HIP renderer: poses stay on the GPU (pg_pose_kinematics ->
pg_pose_boxes -> pg_render_frame with a uint8 frame), no files, and one 16-byte-per-frame device->host copy
(the integer boxes size the launches); the crop / normalise / anti-aliased resize run as torch ops on the
device.  The caster comes from `load_raycaster` (memoised: no checkpoint reload per call).
"""
from __future__ import annotations

import math
from typing import Optional, Tuple

import numpy as np
import torch
import torch.nn.functional as F

# ImageNet statistics the reference normalises with (run_gan.py:2342-2343)
IMG_NORM_MEAN = (0.485, 0.456, 0.406)
IMG_NORM_STD = (0.229, 0.224, 0.225)


def resize_antialiased(img: torch.Tensor, size: Tuple[int, int]) -> torch.Tensor:
    """skimage.transform.resize(img, size, anti_aliasing=True) for [N,C,h,w] -> [N,C,H,W] on the device:
    Gaussian prefilter with sigma = (scale - 1) / 2 per axis (truncated at 4 sigma, mirrored borders),
    then order-1 interpolation at pixel centres (run_gan.py:2064-2065)."""
    n, c, h, w = img.shape
    out = img
    for axis, (src, dst) in ((2, (h, size[0])), (3, (w, size[1]))):
        sigma = max(0.0, (src / dst - 1.0) / 2.0)
        if sigma <= 0:
            continue
        radius = int(4.0 * sigma + 0.5)
        if radius == 0:
            continue
        x = torch.arange(-radius, radius + 1, device=img.device, dtype=torch.float32)
        k = torch.exp(-0.5 * (x / sigma) ** 2)
        k = k / k.sum()
        shape = [1, 1, 1, 1]
        shape[axis] = 2 * radius + 1
        pad = [0, 0, 0, 0]
        pad[(3 - axis) * 2] = pad[(3 - axis) * 2 + 1] = radius
        out = F.pad(out, pad, mode="reflect")              # scipy.ndimage 'mirror' = torch 'reflect'
        out = F.conv2d(out.reshape(n * c, 1, *out.shape[2:]), k.reshape(shape)).reshape(n, c, h, w)
    return F.interpolate(out, size=size, mode="bilinear", align_corners=False)


@torch.no_grad()
def render_for_regressor(caster, bones: torch.Tensor, rest_pose, c2w, H: int, W: int, focal: float,
                         ext_scale: float = 0.001, crop: Tuple[int, int] = (100, 412), out_res: int = 224,
                         white_bkgd: bool = True, chunk: int = 4096, n_samples: Optional[int] = None,
                         n_importance: Optional[int] = None, return_frames: bool = False, subject_idxs=None):
    """bones [F,24,3] axis-angle on the device -> regressor input [F,3,out_res,out_res] on the device
    (+ the uint8 frames [F,H,W,3] if `return_frames`).  One camera `c2w` [4,4] for all frames, like the
    fixed extrinsic of the loop (run_gan.py:2023-2028).  `subject_idxs`: one subject of the caster's bank per pose
    ([F], or fewer indexed i % n, or a scalar): several A-NeRF characters in one call."""
    from .render import frame_subjects_of
    r = caster.renderer
    dev = r.device
    subj = frame_subjects_of(r, subject_idxs, bones.shape[0])       # (checked before anything is launched)
    kps, skts = r.pose_kinematics(bones, rest_pose)
    cyls, boxes = r.pose_boxes(kps, c2w, H, W, focal, ext_scale)
    boxes_h = boxes.cpu().numpy()                           # 16 B per frame: the only host round trip
    r.set_chunk(int(chunk))
    c2w_np = np.asarray(torch.as_tensor(c2w).detach().cpu(), dtype=np.float32)
    frames = torch.empty(bones.shape[0], H, W, 3, device=dev, dtype=torch.uint8)
    prev = r.selected_subject if subj is not None else None
    try:
        for i in range(bones.shape[0]):
            b = boxes_h[i]
            if subj is not None:
                r.select_subject(subj[i])
            _, _, _, rgb8 = r.render_frame(H, W, focal, c2w_np, ((int(b[0]), int(b[1])), (int(b[2]), int(b[3]))), skts[i:i + 1],
                                           cyls[i:i + 1], n_samples=n_samples, n_importance=n_importance,
                                           base_bg=1.0 if white_bkgd else 0.0, want_uint8=True)
            frames[i] = rgb8
    finally:
        if prev is not None:
            r.select_subject(prev)
    img = frames[:, crop[0]:crop[1], crop[0]:crop[1], :].permute(0, 3, 1, 2).float() / 255.0
    mean = torch.tensor(IMG_NORM_MEAN, device=dev).view(1, 3, 1, 1)
    std = torch.tensor(IMG_NORM_STD, device=dev).view(1, 3, 1, 1)
    img = resize_antialiased((img - mean) / std, (out_res, out_res))
    return (img, frames) if return_frames else img


@torch.no_grad()
def regressor_keypoints(renderer, pred_rotmat: torch.Tensor, rest_pose=None, scale: float = 0.4) -> torch.Tensor:
    """The regressor's rotation matrices [F,24,3,3] as key points [F,24,3] on the device: the
    `pose[ii] = get_smpl_l2ws_torch(pred_rotmat, axis_to_matrix=False, scale=0.4)[:, :, :3, -1]` line of the loop
    (run_gan.py:2081), by pg_pose_kinematics_rot.  `rest_pose`: None = smpl_rest_pose in float32, as there.  What comes out goes
    into `regressor_feedback`."""
    from .skeleton import smpl_rest_pose
    rest = smpl_rest_pose.astype(np.float32) if rest_pose is None else rest_pose
    return renderer.pose_kinematics_rot(pred_rotmat, rest, scale=scale)[0]


@torch.no_grad()
def regressor_feedback(pred_kps: torch.Tensor, gt_kps: torch.Tensor, scorer=None) -> torch.Tensor:
    """The number the loop feeds back from the regressor (run_gan.py:2085-2091): both [F,24,3] pose sets centred on joint 0, the
    14 joints of run_gan.py:2087, `spin_loss = 1 - mpjpe(pose, pose_gt)` -- as a float64 device scalar from `pg_pose_scores`
    (pose_eval.PoseScorer), with no synchronisation and no copy to the host.  `scorer`: a `PoseScorer` (e.g. of the caster's
    renderer); None = the module's own on the key points' device."""
    from . import pose_eval
    sc = pose_eval._scorer_for(scorer, pred_kps, gt_kps)
    out = sc.enqueue(pred_kps, gt_kps, joints=pose_eval.GAN_LOOP_JOINTS, root=0, align="none")
    return 1.0 - out["summary"][1]


def generator_feedback(renderer, pred_kps: torch.Tensor, bones: torch.Tensor, rest_pose=None, scale: float = 0.4) -> torch.Tensor:
    """`regressor_feedback` as the generator trains on it (run_gan.py:2032-2034, 2085-2091): `1 - mpjpe(pose, pose_gt)` on the loop's 14
    joints, both sets centred on joint 0, with `pose_gt = get_smpl_l2ws_torch(bones, scale=0.4)[..., :3, -1]` differentiable in the
    generator's axis-angle output `bones` [F,24,3] and `pose` = `pred_kps` [F,24,3] a constant (the regressor runs under no_grad
    there).  A float64 device scalar; its backward is two launches (pg_pose_loss's gradient, pg_pose_kinematics_bwd).  `rest_pose`:
    None = smpl_rest_pose in float32."""
    from . import pose_eval, pose_losses
    from .skeleton import smpl_rest_pose
    rest = smpl_rest_pose.astype(np.float32) if rest_pose is None else rest_pose
    gt_kps = pose_losses.keypoints_from_axis_angle(renderer, bones, rest, scale=scale)
    return 1.0 - pose_losses.pose_loss(pred_kps.detach(), gt_kps, joints=pose_eval.GAN_LOOP_JOINTS, root=0, kind="mpjpe", renderer=renderer)


def regressor_loss(renderer, pred_rotmat: torch.Tensor, gt: torch.Tensor, gt_is_axis_angle: bool = False, cap: float = 0.02,
                   weight: float = 0.1) -> torch.Tensor:
    """The loss `train_spin` trains the regressor on (run_gan.py:1896-1908): key points of `pred_rotmat` [F,24,3,3] at scale 0.4, both
    sets centred on joint 0, the loop's 14 joints, the prediction rescaled to the ground truth's Frobenius norm, `weight` times the
    per-pose mean joint distance, poses at or above `cap` dropped, the mean of the rest -- differentiable in `pred_rotmat`.  `gt`: key
    points [F,24,3]; with `gt_is_axis_angle` axis-angle vectors [F,24,3] that go through the same kinematics first, which with
    `cap=math.inf` is the MPII branch (:1924-1934)."""
    from . import pose_eval, pose_losses
    from .skeleton import smpl_rest_pose
    pred_kps = pose_losses.keypoints_from_rotmats(renderer, pred_rotmat, None, scale=0.4)
    if gt_is_axis_angle:
        with torch.no_grad():
            gt = renderer.pose_kinematics(gt, smpl_rest_pose.astype(np.float32) * np.float32(0.4))[0]
    return pose_losses.pose_loss(pred_kps, gt.detach(), joints=pose_eval.GAN_LOOP_JOINTS, root=0, kind="norm_matched", weight=weight,
                                 cap=cap, renderer=renderer)


def regressor_body_loss(body, pred_rotmat: torch.Tensor, pred_betas: torch.Tensor, gt_kps: torch.Tensor, regressor: str, joints=None,
                        root: int = 0, kind: str = "mpjpe", cap: float = math.inf, weight: float = 1.0) -> torch.Tensor:
    """The pose loss on the joints the regressor is scored on: `regressor` (a name in `body.regressors`, e.g. the h36m regressor)
    applied to the body's vertices for `pred_rotmat` [F,24,3,3] and `pred_betas` [F,NB] (or one row), against `gt_kps` [F,K,3] -- the
    same regressor's joints of the ground-truth body --, rows `joints` (None: H36M_TO_J14) after row `root` (the pelvis) is subtracted:
    what `evaluate_smpl_predictions` scores as MPJPE (evaluate.test, run_gan.py:1596-1634).  `body.differentiable(...).regressed` into
    `pose_losses.pose_loss`: a float64 device scalar whose gradients reach `pred_rotmat` (nine free entries a matrix) and `pred_betas`
    through pg_pose_loss's gradient and one pg_smpl_backward call."""
    from . import pose_eval, pose_losses
    pred = body.differentiable(pred_betas, pred_rotmat, pose2rot=False, regressor=regressor, joints=False).regressed
    return pose_losses.pose_loss(pred, gt_kps.detach(), joints=pose_eval.H36M_TO_J14 if joints is None else joints, root=root, kind=kind,
                                 weight=weight, cap=cap, renderer=body.renderer)


def _is_hip_adam(optimizer) -> bool:
    """`optimizer` is an `optim.HipAdam`: its step clips and updates in one device call (pg_adam_step), and the norm is over the
    optimiser's own parameters that have a gradient -- the module's, where the optimiser was built on `module.parameters()`"""
    from . import optim
    return isinstance(optimizer, optim.HipAdam)


def regressor_step(hmr, optimizer, images: torch.Tensor, gt: torch.Tensor, renderer, gt_is_axis_angle: bool = False, cap: float = 0.02,
                   max_norm: Optional[float] = None, masks=None):
    """One batch of `train_spin` (run_gan.py:1880-1940): zero_grad, `hmr(images)` (a `regressors.HipHMR`, or a `regressors.HipHMRHead`
    when `images` are the trunk's features already; in training mode its dropout is live), `regressor_loss` of `pred_rotmat` against
    `gt`, backward -- pg_pose_loss's gradient, pg_pose_kinematics_rot_bwd, pg_hmr_head_backward, then torch's own backward of the trunk --,
    clip_grad_norm_(max_norm) when a norm is given, optimizer.step().  `masks`: the call's dropout keep masks in place of the module's
    own draws.  Returns the loss as a device scalar; nothing synchronises."""
    optimizer.zero_grad()
    pred_rotmat, _, _ = hmr(images, masks=masks)
    loss = regressor_loss(renderer, pred_rotmat, gt, gt_is_axis_angle=gt_is_axis_angle, cap=cap)
    loss.backward()
    if max_norm is not None and _is_hip_adam(optimizer):
        optimizer.step(max_norm=max_norm)
        return loss.detach()
    if max_norm is not None:
        torch.nn.utils.clip_grad_norm_(hmr.parameters(), max_norm=max_norm)
    optimizer.step()
    return loss.detach()


def generator_adversarial_loss(disc, real: Optional[torch.Tensor], fake: torch.Tensor, accuracies: bool = False):
    """The generator step's call of `get_adv_loss` (run_gan.py:1117-1140, 2016-2021): 0.5 mse(D(fake), 1) as a float64 device scalar whose
    backward reaches `fake` through pg_disc_backward -- with `requires_grad` off on the discriminator's parameters (`set_grad([model_d3d],
    False)`) no weight-gradient product runs.  `disc`: a `discriminators.PartDiscriminator`.  Returns (loss, real_acc, fake_acc); the
    accuracies (device scalars) and the real pass only with `accuracies`."""
    from . import discriminators
    return discriminators.adversarial_loss(disc, real, fake, accuracies)


def discriminator_step(disc, optimizer, real: torch.Tensor, fake: torch.Tensor, pool, rng=None, max_norm: float = 1.0):
    """`train_dis` (run_gan.py:1143-1177): zero_grad, the generated poses through the pool (`discriminators.FakePool`; `rng`: its draws,
    None = the global np.random as the reference), 0.5 (mse(D(real), 1) + mse(D(fake), 0)), backward, clip_grad_norm_(max_norm),
    optimizer.step().  Returns (real_acc, fake_acc, loss) as device scalars; nothing synchronises (the reference's three copies to the
    host are gone)."""
    from . import discriminators
    optimizer.zero_grad()
    fake = pool(fake.detach(), rng)
    loss, real_acc, fake_acc = discriminators.discriminator_loss(disc, real.detach(), fake)
    loss.backward()
    if max_norm is not None and _is_hip_adam(optimizer):
        optimizer.step(max_norm=max_norm)
        return real_acc, fake_acc, loss.detach()
    torch.nn.utils.clip_grad_norm_(disc.parameters(), max_norm=max_norm)
    optimizer.step()
    return real_acc, fake_acc, loss.detach()


def generator_step(gen, disc, optimizer, real: torch.Tensor, feedback=None, max_norm: float = 1.0):
    """The generator half of `train_gan` (run_gan.py:2001-2107): zero_grad, `gen(real)` (a `generators.HipPoseGenerator`, which draws
    its noise with torch.randn in the reference's order), `generator_adversarial_loss` of `pose_ba` against `disc` (whose parameters the
    caller has frozen, `set_grad([model_d3d], False)`), plus 0.1 times `feedback(pose_ba)` when a feedback term is given (a callable
    that returns a scalar differentiable in `pose_ba`, e.g. `generator_feedback` on the rendered subset; None = the reference's
    `spin_loss = 0`), backward, clip_grad_norm_(max_norm), optimizer.step().  Returns (the detached `pose_ba` for `discriminator_step`,
    the loss as a device scalar); nothing synchronises."""
    optimizer.zero_grad()
    out = gen(real)
    loss, _, _ = generator_adversarial_loss(disc, real, out["pose_ba"])
    if feedback is not None:
        loss = loss + 0.1 * feedback(out["pose_ba"])
    loss.backward()
    if max_norm is not None and _is_hip_adam(optimizer):
        optimizer.step(max_norm=max_norm)
        return out["pose_ba"].detach(), loss.detach()
    torch.nn.utils.clip_grad_norm_(gen.parameters(), max_norm=max_norm)
    optimizer.step()
    return out["pose_ba"].detach(), loss.detach()
