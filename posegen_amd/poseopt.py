"""The pose layer of pose refinement on the HIP path: the reference's `PoseOptLayer` (core/pose_opt.py:240-445).

In the reference, `popt_layer(kp_idx)` turns the batch's pose parameters into the per-ray `kps, bones, skts, l2ws, rots`
the ray caster and the pose losses read (core/trainer.py:286-313): 6-D rotations -> matrices, the unrolled SMPL chain,
`+ pelvis`, `torch.inverse`, a gather by `inverse_idxs` -- about a hundred small launches and, in backward, an atomic
scatter-add.  `HipPoseOptLayer` is that module for the configuration every shipped opt_pose config uses (SMPL skeleton,
`use_rot6d=True`, `use_cache=False`): the same parameters and buffers under the same names, `forward(idxs)` with the same
five outputs, one kernel forward and one backward (pg_poseopt_forward / pg_poseopt_backward, csrc/pg_poseopt.hip).  The
backward sums a pose's rays in ascending ray order, so `pelvis.grad` / `bones.grad` are bitwise repeatable.  Its outputs go
into `TrainableRayCaster(opt_pose=True)` unchanged.  There is no torch fallback: without the library `forward` raises.
"""
from __future__ import annotations

import ctypes as C
from typing import NamedTuple, Optional

import numpy as np
import torch

from . import _ffi
from .skeleton import SMPLSkeleton

_I32P = C.POINTER(C.c_int32)


def axisang_to_rot6d(axisang) -> np.ndarray:
    """Axis-angle [...,3] -> the 6-D rotation parameters [...,6] of Zhou et al. (the first two columns of the rotation
    matrix, row-major: r00 r01 r10 r11 r20 r21), float32.

    The reference makes this conversion once, in `PoseOptLayer.__init__` (pose_opt.py:284-288), with pytorch3d's
    `axis_angle_to_matrix` in float32.  Here it is Rodrigues' formula R = I + sin(t)/t K + (1 - cos t)/t^2 K^2 in float64
    (series below t = 1e-4), rounded once: the initial parameters are pinned to that formula, not to pytorch3d's rounding
    -- they agree to float32 precision, and every value after initialisation comes from the optimiser."""
    w = np.asarray(axisang, dtype=np.float64)
    t2 = (w * w).sum(-1)
    small = t2 < 1e-8
    t = np.sqrt(np.where(small, 1.0, t2))
    a = np.where(small, 1.0 - t2 / 6.0, np.sin(t) / t)
    b = np.where(small, 0.5 - t2 / 24.0, (1.0 - np.cos(t)) / np.where(small, 1.0, t2))
    K = np.zeros(w.shape[:-1] + (3, 3))
    K[..., 0, 1], K[..., 0, 2] = -w[..., 2], w[..., 1]
    K[..., 1, 0], K[..., 1, 2] = w[..., 2], -w[..., 0]
    K[..., 2, 0], K[..., 2, 1] = -w[..., 1], w[..., 0]
    R = np.eye(3) + a[..., None, None] * K + b[..., None, None] * (K @ K)
    return R[..., :3, :2].reshape(w.shape[:-1] + (6,)).astype(np.float32)


class RaySegments(NamedTuple):
    """The batch's poses and which rays read them."""
    unique: np.ndarray        # [U] int64: the distinct pose indices, ascending (np.unique)
    inverse: np.ndarray       # [n] int32: ray -> position in `unique`
    seg_start: np.ndarray     # [U+1] int32, seg_rays [n] int32: pose u's rays are seg_rays[seg_start[u]:seg_start[u+1]],
    seg_rays: np.ndarray      # ascending


def ray_segments(idxs) -> RaySegments:
    """`np.unique(idxs, return_inverse=True)` (pose_opt.py:380) plus the rays of every pose as a CSR pair, each pose's rays in
    ascending order (a stable sort): the order in which the backward kernel sums their cotangents.  `idxs`: an int, a list,
    a numpy array or a tensor."""
    if torch.is_tensor(idxs):
        idxs = idxs.detach().cpu().numpy()
    a = np.atleast_1d(np.asarray(idxs)).reshape(-1)
    if a.size and not np.issubdtype(a.dtype, np.integer):
        raise TypeError(f"pose indices must be integers, not {a.dtype}")
    unique, inverse = np.unique(a.astype(np.int64), return_inverse=True)
    inverse = inverse.reshape(-1)
    seg_rays = np.argsort(inverse, kind="stable").astype(np.int32)
    seg_start = np.zeros(len(unique) + 1, dtype=np.int32)
    np.cumsum(np.bincount(inverse, minlength=len(unique)), out=seg_start[1:])
    return RaySegments(unique, np.ascontiguousarray(inverse, dtype=np.int32), seg_start, np.ascontiguousarray(seg_rays))


def _index_tensor(a, device) -> torch.Tensor:
    """host integers as a long tensor on `device`; on a HIP device through pinned memory, so that the upload is enqueued on the
    current stream like the kernels that follow it instead of making the host wait for that stream"""
    t = torch.as_tensor(np.asarray(a), dtype=torch.long)
    if torch.device(device).type == "cuda":
        return t.pin_memory().to(device, non_blocking=True)
    return t.to(device)


def _i32(a: Optional[np.ndarray]):
    return None if a is None else a.ctypes.data_as(_I32P)


class _KinematicsFn(torch.autograd.Function):
    """(kps, skts, l2ws, rots) per ray from the unique poses' (pelvis [U,3], bone [U,24,6]); rest [1 or U,24,3] is a constant."""

    @staticmethod
    def forward(ctx, layer, seg: RaySegments, pelvis, bone, rest):
        r = layer._renderer[0]
        dev = r.device
        f32 = lambda t: t.detach().to(device=dev, dtype=torch.float32).contiguous()
        pelvis_c, bone_c, rest_c = f32(pelvis), f32(bone), f32(rest)
        U, n = len(seg.unique), len(seg.inverse)
        kps = torch.empty(n, 24, 3, device=dev)
        skts = torch.empty(n, 24, 4, 4, device=dev)
        l2ws = torch.empty(n, 24, 4, 4, device=dev)
        rots = torch.empty(n, 24, 3, 3, device=dev)
        _ffi.call(r, "pg_poseopt_forward", U, 6, bone_c, pelvis_c, rest_c, 0 if rest_c.shape[0] == 1 else 72, _i32(layer._parents), n,
                  _i32(seg.inverse), rots, l2ws, skts, kps)
        ctx.layer, ctx.seg, ctx.saved = layer, seg, (pelvis_c, bone_c, rest_c)
        ctx.meta = (pelvis.dtype, pelvis.device, bone.dtype, bone.device)
        ctx.set_materialize_grads(False)
        return kps, skts, l2ws, rots

    @staticmethod
    def backward(ctx, g_kps, g_skts, g_l2ws, g_rots):
        layer, seg = ctx.layer, ctx.seg
        r = layer._renderer[0]
        dev = r.device
        pelvis_c, bone_c, rest_c = ctx.saved
        U, n = len(seg.unique), len(seg.inverse)
        cot = [None if g is None else g.to(device=dev, dtype=torch.float32).contiguous() for g in (g_rots, g_l2ws, g_skts, g_kps)]
        d_bone = torch.empty(U, 24, 6, device=dev)
        d_pelvis = torch.empty(U, 3, device=dev)
        _ffi.call(r, "pg_poseopt_backward", U, 6, bone_c, pelvis_c, rest_c, 0 if rest_c.shape[0] == 1 else 72, _i32(layer._parents), n,
                  _i32(seg.seg_start), _i32(seg.seg_rays), *cot, d_bone, d_pelvis)
        pd, pdev, bd, bdev = ctx.meta
        return None, None, d_pelvis.to(device=pdev, dtype=pd), d_bone.to(device=bdev, dtype=bd), None


class HipPoseOptLayer(torch.nn.Module):
    """Drop-in for the reference's `PoseOptLayer` (core/pose_opt.py:240-445) with its constructor plus `renderer` (the
    `HipRenderer` whose handle and device the kernels run on: `caster.renderer`; None builds a host-side module for
    state-dict work whose `forward` raises until `attach(renderer)`).

    Parameters and buffers carry the reference's names -- `pelvis` [N,3], `bones` [N,24,6] (multi-view, `kp_map` given:
    `root_bones` [N,6], `bones` [len(kp_uidxs),23,6], buffers `kp_map`, `kp_uidxs`), buffer `rest_pose` [1 or M,24,3] -- so
    a `poseopt_layer_state_dict` loads into it and what it saves loads into the reference (`from_state_dict`).
    `kps` / `bones` [N,24,3] are the initial key points and axis-angle rotations; the initial 6-D parameters are
    `axisang_to_rot6d(bones)`: Rodrigues in float64, rounded once (the reference calls pytorch3d in float32 there; pinned to
    the float64 formula, see that function).

    `forward(idxs, rest_pose_idxs=None)` returns `(kps, bones, skts, l2ws, rots)` per ray like the reference.

    Refused with NotImplementedError, before anything is computed: `use_rot6d=False` (axis-angle parameters),
    `use_cache=True`, a skeleton other than SMPL, a renderer that is not on a HIP device."""

    def __init__(self, kps, bones, rest_pose, skel_type=SMPLSkeleton, kp_map=None, kp_uidxs=None, use_cache=False,
                 use_rot6d=False, beta=None, rest_pose_idxs=None, renderer=None):
        super().__init__()
        if not use_rot6d:
            raise NotImplementedError("HipPoseOptLayer: use_rot6d=False (axis-angle pose parameters) is not built on the HIP path; "
                                      "every shipped opt_pose config sets opt_rot6d")
        if use_cache:
            raise NotImplementedError("HipPoseOptLayer: use_cache=True (opt_pose_cache) is not built on the HIP path")
        trees = np.asarray(getattr(skel_type, "joint_trees", []))
        if getattr(skel_type, "root_id", None) != 0 or trees.shape != (24,) or not np.array_equal(trees, SMPLSkeleton.joint_trees):
            raise NotImplementedError("HipPoseOptLayer: only the 24-joint SMPL skeleton is supported (as in the reference)")
        device = self._check_renderer(renderer)
        self._renderer = [renderer]                      # (a list: not a sub-module, not part of the state)
        self.skel_type, self.root_id = skel_type, 0
        self.use_cache, self.use_rot6d = False, True
        self.rest_pose_idxs = rest_pose_idxs
        self.beta = torch.as_tensor(beta) if beta is not None else None
        self._parents = np.ascontiguousarray(trees, dtype=np.int32)
        t = lambda a: torch.as_tensor(np.asarray(a.detach().cpu() if torch.is_tensor(a) else a), dtype=torch.float32)
        kps, rest_pose = t(kps), t(rest_pose)
        if rest_pose.dim() == 2:
            rest_pose = rest_pose[None]
        rot6d = torch.from_numpy(axisang_to_rot6d(t(bones).numpy()))            # [N,24,6]
        if kps.shape[1:] != (24, 3) or rot6d.shape[1:] != (24, 6) or rest_pose.shape[1:] != (24, 3):
            raise ValueError("HipPoseOptLayer: kps / bones [N,24,3] and rest_pose [1 or M,24,3] expected")
        if kp_map is not None:
            self.register_buffer("kp_map", torch.as_tensor(np.asarray(kp_map)).long().to(device))
            self.register_buffer("kp_uidxs", torch.as_tensor(np.asarray(kp_uidxs)).long().to(device))
        else:
            self.kp_map = self.kp_uidxs = None
        self.register_buffer("rest_pose", rest_pose.to(device))
        P = lambda x: torch.nn.Parameter(x.clone().contiguous().to(device), requires_grad=True)
        self.pelvis = P(kps[:, 0])
        if kp_map is None:
            self.bones = P(rot6d)
        else:                                            # multi-view: the root rotation per view, the rest per unique pose
            self.root_bones = P(rot6d[:, 0])
            self.bones = P(rot6d[torch.as_tensor(np.asarray(kp_uidxs)).long(), 1:])
        self.N_kps = self.pelvis.shape[0]

    @staticmethod
    def _check_renderer(renderer):
        if renderer is None:
            return torch.device("cpu")
        device = torch.device(renderer.device)
        if device.type != "cuda":
            raise NotImplementedError(f"HipPoseOptLayer: the renderer is on {device}, not on a HIP device (torch 'cuda:N'); "
                                      "the pose layer has no CPU path")
        return device

    def attach(self, renderer):
        """Run on `renderer`'s handle and device from now on (moves the parameters there)."""
        device = self._check_renderer(renderer)
        self._renderer = [renderer]
        self.to(device)
        return self

    @classmethod
    def from_state_dict(cls, state_dict, renderer=None, rest_pose_idxs=None, beta=None):
        """The layer a checkpoint holds (the reference's load_poseopt_from_state_dict, pose_opt.py:216-238): `state_dict` is
        the checkpoint or its `poseopt_layer_state_dict` entry."""
        sd = state_dict.get("poseopt_layer_state_dict", state_dict)
        if sd["bones"].shape[-1] != 6:
            raise NotImplementedError("HipPoseOptLayer: the checkpoint holds axis-angle pose parameters (use_rot6d=False)")
        n, nj = sd["pelvis"].shape[0], sd["bones"].shape[1]
        kp_map = kp_uidxs = None
        if "kp_map" in sd:
            kp_map, kp_uidxs = sd["kp_map"].cpu().numpy(), sd["kp_uidxs"].cpu().numpy()
            nj += 1
        zeros = np.zeros((n, nj, 3), dtype=np.float32)
        layer = cls(zeros, zeros, np.zeros(tuple(sd["rest_pose"].shape), dtype=np.float32), kp_map=kp_map, kp_uidxs=kp_uidxs,
                    use_rot6d=True, beta=beta, rest_pose_idxs=rest_pose_idxs, renderer=renderer)
        layer.load_state_dict(sd)
        return layer

    # ---- the reference's accessors (pose_opt.py:318-369) ---------------------------------------------------------------
    def idx_to_params(self, idx):
        idx = _index_tensor(idx, self.pelvis.device)
        pelvis = self.pelvis[idx]
        if self.kp_map is None:
            return pelvis, self.bones[idx]
        return pelvis, torch.cat([self.root_bones[idx, None, :], self.bones[self.kp_map[idx]]], dim=1)

    def get_pelvis(self, idx=None):
        return self.idx_to_params(np.arange(self.N_kps) if idx is None else idx)[0]

    def get_beta(self):
        return self.beta

    def get_rest_pose(self, kp_idxs=None, rest_pose_idxs=None):
        if len(self.rest_pose) == 1:
            return self.rest_pose
        if rest_pose_idxs is None:
            rest_pose_idxs = np.asarray(self.rest_pose_idxs)[kp_idxs]
        return self.rest_pose[_index_tensor(rest_pose_idxs, self.rest_pose.device)]

    def forward(self, idxs=None, rest_pose_idxs=None):
        """`calculate_kinematic` (pose_opt.py:372-445): (kps [n,24,3], bones [n,24,6], skts [n,24,4,4], l2ws [n,24,4,4],
        rots [n,24,3,3]) for the rays' pose indices `idxs` (None: every pose once)."""
        if self._renderer[0] is None:
            raise _ffi.HipLibraryError("HipPoseOptLayer.forward needs a renderer (attach(caster.renderer)): the pose layer "
                                       "has no torch fallback")
        seg = ray_segments(np.arange(self.N_kps) if idxs is None else idxs)
        if len(seg.inverse) == 0:
            raise ValueError("HipPoseOptLayer.forward: no pose indices")
        if seg.unique[0] < 0 or seg.unique[-1] >= self.N_kps:
            raise IndexError(f"pose index outside [0, {self.N_kps})")
        rest = self.get_rest_pose(seg.unique, rest_pose_idxs)
        if rest.shape[0] not in (1, len(seg.unique)):
            raise ValueError(f"{rest.shape[0]} rest poses for {len(seg.unique)} unique poses")
        pelvis, bone = self.idx_to_params(seg.unique)
        kps, skts, l2ws, rots = _KinematicsFn.apply(self, seg, pelvis, bone, rest)
        inverse = _index_tensor(seg.inverse, bone.device)
        return kps, bone[inverse], skts, l2ws, rots
