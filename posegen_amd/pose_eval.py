"""Scoring 3-D poses on the device: MPJPE, PA-MPJPE, N-MPJPE, PCK and AUC.

The reference reports pose error on the host: `Criterion3DPose_ProcrustesCorrected` copies every pose to numpy and runs
`procrustes` on it (core/utils/evaluation_helpers.py:387-504), `reconstruction_error` loops `compute_similarity_transform` over the
batch (run_gan.py:1380-1456), `evaluate_pampjpe_from_smpl_params` forms PCK and AUC from the result (:595-601).  Here key points
stay on the device: `pg_pose_scores` (csrc/pg_posescore.hip) aligns one pose per wave in float64 and reduces a batch to
4 + 2 T doubles, and `PoseScorer.score` makes one copy of those back.  There is no torch fallback and no CPU path.

`pa_mpjpe`, `n_mpjpe`, `reconstruction_error` and `refinement_scores` have the reference's call shapes; they run on a scorer of
their own per device (a `HipRenderer` without weights: the entry point needs none) unless one is passed.

`evaluate_smpl_predictions` (evaluate.test, run_gan.py:1584-1634) and `pampjpe_from_smpl_params`
(evaluate_pampjpe_from_smpl_params, evaluation_helpers.py:542-612) put the SMPL body in front of the scorer: `smpl.BodyModel`
(pg_smpl_forward) regresses the joints on the device and they go into `PoseScorer` without leaving it; kinematics from rotation
matrices are `HipRenderer.pose_kinematics_rot`.

Not built, refused or simply not offered: gradients through the aligned scores (the unaligned and norm-matched losses with their
gradients are `pose_losses`), `procrustes(scaling=False)`, scoring across several
devices.
"""
from __future__ import annotations

import ctypes as C
from typing import Optional

import numpy as np
import torch

from . import _ffi

ALIGN_MODES = {"none": _ffi.PG_POSE_ALIGN_NONE, "scale": _ffi.PG_POSE_ALIGN_SCALE, "best": _ffi.PG_POSE_ALIGN_BEST,
               "rotation": _ffi.PG_POSE_ALIGN_ROTATION}
MAX_JOINTS = MAX_THRESHOLDS = 64
# the 14 joints of the 24 SMPL joints the GAN loop scores, after centring both poses on joint 0 (run_gan.py:2085-2088)
GAN_LOOP_JOINTS = (1, 2, 4, 5, 7, 8, 12, 15, 16, 17, 18, 19, 20, 21)


def _align_code(align) -> int:
    if isinstance(align, str):
        if align not in ALIGN_MODES:
            raise ValueError(f"PoseScorer: align = {align!r}, not one of {sorted(ALIGN_MODES)}")
        return ALIGN_MODES[align]
    if align is False:
        raise NotImplementedError("PoseScorer: procrustes(scaling=False) is not built")
    if int(align) not in ALIGN_MODES.values():
        raise ValueError(f"PoseScorer: align = {align!r}, not one of {sorted(ALIGN_MODES)} or their codes 0..3")
    return int(align)


class PoseScorer:
    """`pg_pose_scores` on `renderer`'s handle and device (`caster.renderer`; any `HipRenderer`, with or without weights)."""

    def __init__(self, renderer):
        self.device = torch.device(getattr(renderer, "device", "cpu"))
        if self.device.type != "cuda":
            raise NotImplementedError(f"PoseScorer: the renderer is on {self.device}, not on a HIP device (torch 'cuda:N'); poses are "
                                      "scored by pg_pose_scores only, there is no CPU path")
        self.renderer = renderer

    # ---- argument checks, all before anything touches the device ------------------------------------------------------------
    @staticmethod
    def _check_shapes(pred, gt):
        ps, gs = tuple(np.shape(pred)), tuple(np.shape(gt))
        if len(ps) == 2:
            ps, gs = (1,) + ps, ((1,) + gs if len(gs) == 2 else gs)
        if len(ps) != 3 or ps[2] != 3 or ps != gs:
            raise ValueError(f"PoseScorer: pred {tuple(np.shape(pred))} and gt {tuple(np.shape(gt))} must both be [B,J,3] (or [J,3])")
        if ps[0] < 1 or ps[1] < 1:
            raise ValueError(f"PoseScorer: no poses or no joints in {ps}")
        return ps

    @staticmethod
    def _check_selection(J_in, joints, root):
        if joints is not None:
            joints = [int(j) for j in np.asarray(joints).reshape(-1)]
            if not joints:
                raise ValueError("PoseScorer: an empty joint selection")
            if min(joints) < 0 or max(joints) >= J_in:
                raise IndexError(f"PoseScorer: a joint index is outside [0, {J_in})")
        J = J_in if joints is None else len(joints)
        if J > MAX_JOINTS:
            raise ValueError(f"PoseScorer: {J} joints to score; the kernel takes at most {MAX_JOINTS} (select with joints=)")
        root = -1 if root is None else int(root)
        if root < -1 or root >= J_in:
            raise IndexError(f"PoseScorer: root = {root} is outside [0, {J_in})")
        return joints, J, root

    @staticmethod
    def _check_thresholds(unit, pck_threshold, auc_thresholds):
        unit = float(unit)
        if not np.isfinite(unit) or unit <= 0.0:
            raise ValueError(f"PoseScorer: unit = {unit} (a positive factor: 1000 for metres to millimetres)")
        auc = np.zeros(0) if auc_thresholds is None else np.asarray(auc_thresholds, dtype=np.float64).reshape(-1)
        th = np.concatenate([np.zeros(0) if pck_threshold is None else [float(pck_threshold)], auc])
        if len(th) > MAX_THRESHOLDS:
            raise ValueError(f"PoseScorer: {len(th)} thresholds; the kernel takes at most {MAX_THRESHOLDS} (pck_threshold and auc_thresholds together)")
        if not np.all(np.isfinite(th)):
            raise ValueError("PoseScorer: a threshold is not finite")
        return unit, th, 0 if pck_threshold is None else 1

    def _to_device(self, x) -> torch.Tensor:
        if torch.is_tensor(x):
            if x.is_cuda and x.device != self.device:
                raise NotImplementedError(f"PoseScorer: key points on {x.device}, the renderer on {self.device}; scoring across devices "
                                          "is not built")
            x = x.detach()
        else:
            x = torch.from_numpy(np.ascontiguousarray(x, dtype=np.float32))
        x = x.to(device=self.device, dtype=torch.float32)
        return (x[None] if x.dim() == 2 else x).contiguous()

    def _launch(self, pred, gt, joints, J, root, align, th, per_pose, aligned, joint_err, summary):
        """pg_pose_scores on the current stream of the scorer's device; nothing waits for it"""
        r = self.renderer
        B, J_in = pred.shape[:2]
        jarr = None if joints is None else (C.c_int32 * J)(*joints)
        tarr = (C.c_double * max(len(th), 1))(*th)
        with torch.cuda.device(self.device):
            _ffi.call(r, "pg_pose_scores", B, J_in, pred, gt, jarr, J, root, align, tarr, len(th), per_pose, aligned, joint_err, summary)

    def enqueue(self, pred, gt, *, joints=None, root=None, align="best", thresholds=(), ret_per_pose=False, ret_aligned=False,
                ret_joint_err=False):
        """The call without the copy back: device tensors {"summary" float64 [4 + 2 T], and as asked "per_pose" float64 [B,4] (raw,
        aligned, d, scale), "aligned" float32 [B,J,3], "joint_err" float32 [B,J]}, in the inputs' unit (thresholds too).  Nothing
        synchronises."""
        self._check_shapes(pred, gt)
        code = _align_code(align)
        J_in = int(np.shape(pred)[-2])
        joints, J, root = self._check_selection(J_in, joints, root)
        th = np.asarray(thresholds, dtype=np.float64).reshape(-1)
        if len(th) > MAX_THRESHOLDS:
            raise ValueError(f"PoseScorer: {len(th)} thresholds; the kernel takes at most {MAX_THRESHOLDS}")
        pred, gt = self._to_device(pred), self._to_device(gt)
        B = pred.shape[0]
        new = lambda *shape, dtype: torch.empty(*shape, dtype=dtype, device=self.device)
        out = {"summary": new(4 + 2 * len(th), dtype=torch.float64)}
        if ret_per_pose:
            out["per_pose"] = new(B, 4, dtype=torch.float64)
        if ret_aligned:
            out["aligned"] = new(B, J, 3, dtype=torch.float32)
        if ret_joint_err:
            out["joint_err"] = new(B, J, dtype=torch.float32)
        self._launch(pred, gt, joints, J, root, code, th, out.get("per_pose"), out.get("aligned"), out.get("joint_err"), out["summary"])
        return out

    @torch.no_grad()
    def score(self, pred, gt, *, joints=None, root=None, align="best", unit=1.0, pck_threshold=150., auc_thresholds=np.linspace(0, 150, 31),
              ret_aligned=False, ret_joint_err=False, ret_per_pose=False):
        """`pred` against `gt`, both [B,J_in,3] (device tensors, or host arrays that are copied over).  `joints`: the rows to score
        (None: all, at most 64), `root`: the row both sets are centred on first, `align`: "none", "scale" (N-MPJPE), "best"
        (PA-MPJPE as `procrustes` fits it, reflections allowed) or "rotation" (`compute_similarity_transform`, det R = +1).
        `unit` scales the errors -- 1000 for metres to millimetres, 1 / ext_scale for MPJPC -- and `pck_threshold`,
        `auc_thresholds` (at most 64 together) are given in that unit.

        Returns Python floats from one device-to-host copy: "mpjpe" (unaligned), "aligned" (the MPJPE after `align`), "d" (the
        residual `procrustes` returns, from the aligned points), "pck" and "auc" of the aligned distances, "pck_raw" and "auc_raw"
        of the unaligned ones (the share of joint distances strictly below the threshold; AUC = the mean share over
        `auc_thresholds`; None without thresholds), "n" poses.  On request, device tensors in the INPUTS' unit: "aligned_kps"
        float32 [B,J,3], "joint_err" float32 [B,J], "per_pose" float64 [B,4] (raw, aligned, d, scale)."""
        unit, th, n_pck = self._check_thresholds(unit, pck_threshold, auc_thresholds)
        dev = self.enqueue(pred, gt, joints=joints, root=root, align=align, thresholds=th / unit, ret_per_pose=ret_per_pose,
                           ret_aligned=ret_aligned, ret_joint_err=ret_joint_err)
        s = dev["summary"].cpu().numpy()                        # the one copy
        T = len(th)
        share_raw, share_al = s[4:4 + T], s[4 + T:4 + 2 * T]
        mean = lambda v: float(np.mean(v)) if len(v) else None
        out = {"n": int(s[0]), "mpjpe": float(s[1] * unit), "aligned": float(s[2] * unit), "d": float(s[3]),
               "pck_raw": float(share_raw[0]) if n_pck else None, "pck": float(share_al[0]) if n_pck else None,
               "auc_raw": mean(share_raw[n_pck:]), "auc": mean(share_al[n_pck:])}
        if ret_aligned:
            out["aligned_kps"] = dev["aligned"]
        if ret_joint_err:
            out["joint_err"] = dev["joint_err"]
        if ret_per_pose:
            out["per_pose"] = dev["per_pose"]
        return out


_scorers: dict = {}


def default_scorer(device) -> PoseScorer:
    """The module's own scorer on `device`: a `HipRenderer` without weights, made on first use and kept"""
    device = torch.device(device)
    if device.type != "cuda":
        raise NotImplementedError(f"pose scores: key points on {device}, not on a HIP device (torch 'cuda:N'); there is no CPU path "
                                  "(pass scorer=PoseScorer(caster.renderer) to score host arrays on that renderer's device)")
    if device.index is None:
        device = torch.device("cuda", torch.cuda.current_device())
    if device not in _scorers:
        from .config import surreal_config
        from .raycaster import HipRenderer
        _scorers[device] = PoseScorer(HipRenderer(surreal_config(), device=device))
    return _scorers[device]


def _scorer_for(scorer: Optional[PoseScorer], *arrays) -> PoseScorer:
    if scorer is not None:
        return scorer
    for a in arrays:
        if torch.is_tensor(a):
            return default_scorer(a.device)
    raise NotImplementedError("pose scores: host arrays and no scorer; there is no CPU path (pass scorer=PoseScorer(caster.renderer))")


def _reduce(who, per_joint: torch.Tensor, reduction):
    """Criterion_MPJPE's reduction of the [B,J] distances (evaluation_helpers.py:475-483)"""
    if reduction == "mean":
        return per_joint.mean()
    if reduction == "sum":
        return per_joint.sum()
    if reduction in (None, "none"):
        return per_joint
    raise ValueError(f"{who}: reduction = {reduction!r} (mean, sum or None)")


@torch.no_grad()
def pa_mpjpe(pred, gt, reduction="mean", scorer: Optional[PoseScorer] = None):
    """`Criterion3DPose_ProcrustesCorrected(Criterion_MPJPE(reduction))(pred, gt)` (evaluation_helpers.py:485-504): (metric,
    aligned_kps) as device tensors -- the mean or the sum of the [B,J] distances after `procrustes`, or the distances themselves
    for reduction=None -- without a copy to the host."""
    _reduce("pa_mpjpe", torch.zeros(1, 1), reduction)
    out = _scorer_for(scorer, pred, gt).enqueue(pred, gt, align="best", ret_aligned=True, ret_joint_err=True)
    return _reduce("pa_mpjpe", out["joint_err"], reduction), out["aligned"]


@torch.no_grad()
def n_mpjpe(pred, gt, reduction="mean", scorer: Optional[PoseScorer] = None):
    """`Criterion3DPose_leastQuaresScaled(Criterion_MPJPE(reduction))(pred, gt)` (evaluation_helpers.py:506-522): (metric, s_opt *
    pred) as device tensors, s_opt = <pred, gt> / <pred, pred> per pose."""
    _reduce("n_mpjpe", torch.zeros(1, 1), reduction)
    out = _scorer_for(scorer, pred, gt).enqueue(pred, gt, align="scale", ret_aligned=True, ret_joint_err=True)
    return _reduce("n_mpjpe", out["joint_err"], reduction), out["aligned"]


@torch.no_grad()
def reconstruction_error(S1, S2, reduction="mean", needpck=False, alpha=0.15, scorer: Optional[PoseScorer] = None):
    """`reconstruction_error(S1, S2, alpha, needpck, reduction)` (run_gan.py:1437-1456): the per-pose mean joint distance after
    `compute_similarity_transform` (det R = +1), as a device tensor: its mean, its sum, or [B] for reduction=None.  With `needpck`:
    (re, error_pck, S1_hat), error_pck [B] = every pose's share of UNALIGNED joint distances below `alpha`.  The reference's loop
    overwrites that share pose by pose and appends once after the loop, so it returns the last pose's share only, as a [1] array;
    this returns all B, and `error_pck[-1:]` is the reference's value."""
    _reduce("reconstruction_error", torch.zeros(1, 1), reduction)
    sc = _scorer_for(scorer, S1, S2)
    out = sc.enqueue(S1, S2, align="rotation", ret_per_pose=True, ret_aligned=needpck)
    re = out["per_pose"][:, 1]
    re = re if reduction in (None, "none") else _reduce("reconstruction_error", re, reduction)
    if not needpck:
        return re
    raw = sc.enqueue(S1, S2, align="none", ret_joint_err=True)["joint_err"]
    return re, (raw < alpha).double().mean(dim=1), out["aligned"]


@torch.no_grad()
def refinement_scores(layer, kp_idx, anchor_kps, gt_kps=None, ext_scale=0.001, scorer: Optional[PoseScorer] = None):
    """How far pose refinement has moved a `HipPoseOptLayer`'s poses `kp_idx`, and how good they are: {"MPJPC": the mean per-joint
    change against `anchor_kps[kp_idx]` divided by ext_scale (core/trainer.py:439-441)}, and with `gt_kps` [N,24,3] also
    {"PA-MPJPE", "MPJPE", "d"} against `gt_kps[kp_idx]` in the same unit (evaluation_helpers.py:566-573).  Floats; one copy per
    score."""
    if not (ext_scale > 0):
        raise ValueError(f"refinement_scores: ext_scale = {ext_scale}")
    idx = np.asarray(kp_idx).reshape(-1)
    if scorer is None:
        renderer = getattr(layer, "_renderer", [None])[0]
        if renderer is None:
            raise _ffi.HipLibraryError("refinement_scores: the layer has no renderer (attach(caster.renderer)); there is no CPU path")
        scorer = PoseScorer(renderer)
    kps = layer(idx)[0].detach()
    pick = lambda a: (a if torch.is_tensor(a) else torch.as_tensor(np.asarray(a), dtype=torch.float32))[torch.as_tensor(idx, dtype=torch.long)]
    unit = 1.0 / float(ext_scale)
    out = {"MPJPC": scorer.score(kps, pick(anchor_kps), align="none", unit=unit, pck_threshold=None, auc_thresholds=None)["mpjpe"]}
    if gt_kps is not None:
        s = scorer.score(kps, pick(gt_kps), align="best", unit=unit, pck_threshold=None, auc_thresholds=None)
        out.update({"PA-MPJPE": s["aligned"], "MPJPE": s["mpjpe"], "d": s["d"]})
    return out


# the 14 of the 17 regressed H36M joints evaluate.test scores (run_gan.py:1608, constants.H36M_TO_J14) and the order in which
# evaluate_pampjpe_from_smpl_params compares them (evaluation_helpers.py:538)
H36M_TO_J14 = (6, 5, 4, 1, 2, 3, 16, 15, 14, 11, 12, 13, 8, 10)
SPIN_TO_CANON = (10, 8, 14, 15, 16, 11, 12, 13, 4, 5, 6, 1, 2, 3, 0, 7, 9)


def _pelvis_j14(regressed: torch.Tensor) -> torch.Tensor:
    """run_gan.py:1606-1609: the regressed joint 0 subtracted as pelvis, the 14 joints selected"""
    idx = torch.as_tensor(H36M_TO_J14, device=regressed.device)
    return (regressed[:, idx] - regressed[:, :1]).contiguous()


@torch.no_grad()
def evaluate_smpl_predictions(body_neutral, body_male, body_female, pred_rotmat, pred_betas, gt_pose, gt_betas, gender, h36m="h36m",
                              scorer: Optional[PoseScorer] = None, alpha=0.15):
    """`evaluate.test` behind the regressor (run_gan.py:1596-1634): `pred_rotmat` [B,24,3,3], `pred_betas` [B,NB] through the
    neutral body, `gt_pose` [B,72] axis-angle, `gt_betas` through the male body and, where `gender` == 1, the female one (a
    `torch.where` on the two bodies' outputs); regressor `h36m` of each body on its vertices, joint 0 as pelvis, H36M_TO_J14.
    Returns float64 numpy arrays [B] from one copy: "mpjpe", "pa-mpjpe" (reconstruction_error: det R = +1), "pck" (every pose's
    share of unaligned distances below `alpha`; the reference keeps the last pose's only), "ume" and "pme" (mean vertex distance of
    the unposed and the posed meshes).  Six passes through pg_smpl_forward, as the reference makes six through lbs."""
    from . import smpl
    dev = body_neutral.device
    B = int(np.shape(pred_rotmat)[0])
    g = torch.as_tensor(gender).to(dev).reshape(-1)
    if g.shape[0] != B:
        raise ValueError(f"evaluate_smpl_predictions: {g.shape[0]} genders for {B} poses")
    female = (g == 1).view(B, 1, 1)
    sc = scorer if scorer is not None else PoseScorer(body_neutral.renderer)
    pred = body_neutral.forward(pred_betas, pred_rotmat, pose2rot=False, regressor=h36m, want_vertices=True, joints=False)
    gt_pose = torch.as_tensor(gt_pose).reshape(B, 24, 3)
    gm = body_male.forward(gt_betas, gt_pose, regressor=h36m, want_vertices=True, joints=False)
    gf = body_female.forward(gt_betas, gt_pose, regressor=h36m, want_vertices=True, joints=False)
    gt_vertices = torch.where(female, gf.vertices, gm.vertices)
    gt_kps = _pelvis_j14(torch.where(female, gf.regressed, gm.regressed))
    pred_kps = _pelvis_j14(pred.regressed)
    eye = torch.eye(3, device=dev).expand(B, 24, 3, 3).contiguous()
    un_pred = body_neutral.forward(pred_betas, eye, pose2rot=False, want_vertices=True, joints=False).vertices
    un_gt = torch.where(female, body_female.forward(gt_betas, eye, pose2rot=False, want_vertices=True, joints=False).vertices,
                        body_male.forward(gt_betas, eye, pose2rot=False, want_vertices=True, joints=False).vertices)
    per_pose = sc.enqueue(pred_kps, gt_kps, align="rotation", ret_per_pose=True)["per_pose"]
    raw = sc.enqueue(pred_kps, gt_kps, align="none", ret_joint_err=True)["joint_err"]
    ume = smpl.vertex_errors(body_neutral.renderer, un_gt, un_pred)[0]
    pme = smpl.vertex_errors(body_neutral.renderer, gt_vertices, pred.vertices)[0]
    out = torch.stack([per_pose[:, 0], per_pose[:, 1], (raw < alpha).double().mean(dim=1), ume, pme]).cpu().numpy()     # the one copy
    return dict(zip(("mpjpe", "pa-mpjpe", "pck", "ume", "pme"), out))


@torch.no_grad()
def pampjpe_from_smpl_params(body, gt_kps, betas, bones, regressor="h36m", pck_threshold=150., use_normalize=False,
                             scorer: Optional[PoseScorer] = None):
    """`evaluate_pampjpe_from_smpl_params(gt_kps, betas, bones, ret_kp=True, ret_pck=True)` (evaluation_helpers.py:542-603):
    `bones` [B,24,3] axis-angle become rotation matrices as axisang_to_rot forms them, go through `body` (pose2rot=False) and its
    17-row `regressor`, in the order SPIN_TO_CANON.  `gt_kps` [B,17,3] in millimetres.  Returns floats {"pampjpe": the mean joint
    distance after `procrustes` against gt_kps (in its unit), "mpjpe": both sets centred on joint 14, gt / 1000, times 1000
    (N-MPJPE with `use_normalize`), "pck": the share of aligned joint distances below `pck_threshold`, "auc": the mean share over
    linspace(0, 150, 31)}, and "pred_kps" [B,17,3] on the device."""
    from . import smpl
    B = int(np.shape(bones)[0])
    if tuple(np.shape(gt_kps)) != (B, len(SPIN_TO_CANON), 3):
        raise ValueError(f"pampjpe_from_smpl_params: gt_kps {tuple(np.shape(gt_kps))}; [{B},{len(SPIN_TO_CANON)},3] expected")
    rots = smpl.bones_to_rotmats(torch.as_tensor(bones).reshape(B, 24, 3))
    reg = body.forward(torch.as_tensor(betas), rots, pose2rot=False, regressor=regressor, joints=False).regressed
    if reg.shape[1] != len(SPIN_TO_CANON):
        raise ValueError(f"pampjpe_from_smpl_params: regressor {regressor!r} has {reg.shape[1]} rows, not {len(SPIN_TO_CANON)}")
    pred_kps = reg[:, torch.as_tensor(SPIN_TO_CANON, device=reg.device)].contiguous()
    sc = scorer if scorer is not None else PoseScorer(body.renderer)
    gt = sc._to_device(gt_kps)
    pa = sc.score(pred_kps, gt, align="best", pck_threshold=pck_threshold, auc_thresholds=np.linspace(0, 150, 31))
    gt_m = (gt.double() / 1000.0).float()                     # (a float32 division by a scalar is a product with its reciprocal on the device)
    mp = sc.score(pred_kps, gt_m, root=14, align="scale" if use_normalize else "none", unit=1000., pck_threshold=None,
                  auc_thresholds=None)
    return {"pampjpe": pa["aligned"], "mpjpe": mp["aligned"] if use_normalize else mp["mpjpe"], "pck": pa["pck"], "auc": pa["auc"],
            "pred_kps": pred_kps}
