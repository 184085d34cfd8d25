"""The SMPL body on the device: vertices, joints, regressed joints and mesh errors.

The reference runs `smplx.lbs.lbs` (smplx/smplx/lbs.py:152-248) as stock torch ops and materialises a [V,4,4] skinning transform per
vertex and pose; `evaluate.test` (run_gan.py:1584-1634) calls it six times per batch and `evaluate_pampjpe_from_smpl_params`
(core/utils/evaluation_helpers.py:542-612) once, mostly for `J_regressor @ vertices`.  Here `pg_smpl_forward` (csrc/pg_smpl.hip)
blends, skins and regresses in one kernel; vertices reach memory only when they are asked for, and what comes out goes straight
into `pose_eval.PoseScorer`.  There is no torch fallback and no CPU path.

Not built, refused or simply not offered: reading the licensed model .pkl (pass the arrays), SMPL-H / SMPL-X / hands / face /
landmarks, a joint count other than 24, more than 16 shape coefficients, `transl`, second derivatives, per-pose model selection
inside one call, several devices.

Gradients through the body: `BodyModel.differentiable` is `forward` behind a once-differentiable autograd function
whose backward is one `pg_smpl_backward` call -- the transpose of the same kernels, the forward computed again, into `betas` and
`pose` (axis-angle through `batch_rodrigues` as written, or the nine free entries of every rotation matrix).
"""
from __future__ import annotations

import ctypes as C
from collections import namedtuple
from typing import Optional

import numpy as np
import torch

from torch.autograd.function import once_differentiable

from . import _ffi

N_JOINTS = 24
POSE_ROWS = 207
MAX_BETAS = 16
MAX_REGRESSOR_ROWS = 64
MODEL_KEYS = ("v_template", "shapedirs", "posedirs", "J_regressor", "parents", "lbs_weights")

BodyOutput = namedtuple("BodyOutput", ("vertices", "joints", "regressed"))


def check_parents(parents) -> np.ndarray:
    """The joint tree as int32 [24] with parents[0] = -1 (smplx stores -1 or a wrapped 2^32 - 1 there; SMPLSkeleton a 0)"""
    p = np.asarray(parents)
    if p.dtype.kind not in "iu":
        raise TypeError(f"BodyModel: parents of dtype {p.dtype}; integers expected")
    if p.shape != (N_JOINTS,):
        raise ValueError(f"BodyModel: parents {p.shape}; [{N_JOINTS}] expected (SMPL-H / SMPL-X are not built)")
    p = p.astype(np.int64)
    p[0] = -1
    for j in range(1, N_JOINTS):
        if not 0 <= p[j] < j:
            raise ValueError(f"BodyModel: joint {j} must come after its parent ({p[j]})")
    return p.astype(np.int32)


def pack_model(v_template, shapedirs, posedirs, J_regressor):
    """The layout of pg_body_model from smplx-layout arrays: (blend float32 [1+NB+207, 3V], rest_joints float64 [1+NB,24,3]).
    `blend` holds the model's float32 values unchanged: row 0 v_template, row 1 + l shapedirs[:,:,l], then posedirs as stored.
    `rest_joints[r]` = J_regressor applied to blend row r in float64: the rest joints are linear in beta."""
    vt = np.asarray(v_template, dtype=np.float32)
    sd = np.asarray(shapedirs, dtype=np.float32)
    pd = np.asarray(posedirs, dtype=np.float32)
    jr = np.asarray(J_regressor, dtype=np.float32)
    if vt.ndim != 2 or vt.shape[1] != 3 or vt.shape[0] < 1:
        raise ValueError(f"BodyModel: v_template {vt.shape}; [V,3] expected")
    V = vt.shape[0]
    if sd.ndim != 3 or sd.shape[:2] != (V, 3):
        raise ValueError(f"BodyModel: shapedirs {sd.shape}; [{V},3,NB] expected")
    NB = sd.shape[2]
    if not 1 <= NB <= MAX_BETAS:
        raise ValueError(f"BodyModel: {NB} shape coefficients; 1..{MAX_BETAS} are built")
    if pd.shape != (POSE_ROWS, 3 * V):
        raise ValueError(f"BodyModel: posedirs {pd.shape}; [{POSE_ROWS},{3 * V}] expected")
    if jr.shape != (N_JOINTS, V):
        raise ValueError(f"BodyModel: J_regressor {jr.shape}; [{N_JOINTS},{V}] expected")
    if (1 + NB + POSE_ROWS) * 3 * V >= 2 ** 31:
        raise ValueError(f"BodyModel: {V} vertices are more than the blend matrix can index")
    blend = np.concatenate([vt.reshape(1, 3 * V), np.moveaxis(sd, 2, 0).reshape(NB, 3 * V), pd], axis=0)
    rest = np.einsum("jv,rvc->rjc", jr.astype(np.float64), blend[:1 + NB].astype(np.float64).reshape(1 + NB, V, 3))
    return np.ascontiguousarray(blend), np.ascontiguousarray(rest)


def bones_to_rotmats(bones: torch.Tensor) -> torch.Tensor:
    """axisang_to_rot (core/utils/skeleton_utils.py:498: pytorch3d's axis-angle -> quaternion -> matrix) in float64, rounded to
    float32 once: [..., 3] -> [..., 3, 3]"""
    b = bones.to(torch.float64)
    ang = b.norm(dim=-1, keepdim=True)
    half = 0.5 * ang
    small = ang.abs() < 1e-6
    k = torch.where(small, 0.5 - ang * ang / 48.0, torch.sin(half) / torch.where(small, torch.ones_like(ang), ang))
    q = torch.cat([torch.cos(half), b * k], dim=-1)
    r, i, j, k_ = q.unbind(-1)
    two_s = 2.0 / (q * q).sum(-1)
    m = torch.stack([1 - two_s * (j * j + k_ * k_), two_s * (i * j - k_ * r), two_s * (i * k_ + j * r),
                     two_s * (i * j + k_ * r), 1 - two_s * (i * i + k_ * k_), two_s * (j * k_ - i * r),
                     two_s * (i * k_ - j * r), two_s * (j * k_ + i * r), 1 - two_s * (i * i + j * j)], dim=-1)
    return m.reshape(*bones.shape[:-1], 3, 3).to(torch.float32)


class BodyModel:
    """One SMPL body on `renderer`'s handle and device (any `HipRenderer`, with or without weights, as for `PoseScorer`).  Arrays
    as smplx stores them: v_template [V,3], shapedirs [V,3,NB], posedirs [207,3V], J_regressor [24,V], parents [24], lbs_weights
    [V,24]; `regressors`: {name: [K_i,V]} with K_i <= 64, e.g. {"h36m": J_regressor_h36m}."""

    def __init__(self, renderer, v_template, shapedirs, posedirs, J_regressor, parents, lbs_weights, regressors=None):
        self.device = torch.device(getattr(renderer, "device", "cpu"))
        if self.device.type != "cuda":
            raise NotImplementedError(f"BodyModel: the renderer is on {self.device}, not on a HIP device (torch 'cuda:N'); the body "
                                      "runs in pg_smpl_forward only, there is no CPU path")
        par = check_parents(parents)
        blend, rest = pack_model(v_template, shapedirs, posedirs, J_regressor)
        self.V, self.NB = blend.shape[1] // 3, blend.shape[0] - 1 - POSE_ROWS
        skin = np.asarray(lbs_weights, dtype=np.float32)
        if skin.shape != (self.V, N_JOINTS):
            raise ValueError(f"BodyModel: lbs_weights {skin.shape}; [{self.V},{N_JOINTS}] expected")
        regs = {}
        for name, r in (regressors or {}).items():
            r = np.asarray(r, dtype=np.float32)
            if r.ndim != 2 or r.shape[1] != self.V or not 1 <= r.shape[0] <= MAX_REGRESSOR_ROWS:
                raise ValueError(f"BodyModel: regressor {name!r} {r.shape}; [K,{self.V}] with K in 1..{MAX_REGRESSOR_ROWS} expected")
            regs[name] = r
        self.renderer = renderer
        self.parents = par
        dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(self.device)
        self._blend, self._skin, self._rest = dev(blend), dev(skin), dev(rest)
        self.regressors = {name: dev(r) for name, r in regs.items()}
        self._model = _ffi.PgBodyModel(V=self.V, NB=self.NB, blend=self._blend.data_ptr(), skin=self._skin.data_ptr(),
                                       rest_joints=self._rest.data_ptr(), parents=(C.c_int32 * N_JOINTS)(*par))

    @classmethod
    def from_arrays(cls, renderer, mapping, regressors=None):
        """`mapping`: a dict, or the path of an .npz, with the keys v_template, shapedirs, posedirs, J_regressor, parents,
        lbs_weights; every further key `regressor_<name>` is a regressor (what synthetic.make_body_model returns)."""
        if isinstance(mapping, (str, bytes)) or hasattr(mapping, "__fspath__"):
            with np.load(mapping) as z:
                mapping = {k: z[k] for k in z.files}
        missing = [k for k in MODEL_KEYS if k not in mapping]
        if missing:
            raise KeyError(f"BodyModel.from_arrays: no {missing} in the arrays")
        regs = {k[len("regressor_"):]: v for k, v in mapping.items() if k.startswith("regressor_")}
        regs.update(regressors or {})
        return cls(renderer, *(mapping[k] for k in MODEL_KEYS), regressors=regs)

    # ---- argument checks, all before anything touches the library -----------------------------------------------------------
    def _check_inputs(self, betas, pose, pose2rot, regressor, want_vertices, joints):
        bs, ps = tuple(betas.shape), tuple(pose.shape)
        if len(bs) != 2 or bs[1] != self.NB:
            raise ValueError(f"BodyModel.forward: betas {bs}; [B,{self.NB}] or [1,{self.NB}] expected")
        if pose2rot:
            if len(ps) == 2 and ps[1] == N_JOINTS * 3:
                ps = (ps[0], N_JOINTS, 3)
            if len(ps) != 3 or ps[1:] != (N_JOINTS, 3):
                raise ValueError(f"BodyModel.forward: pose {tuple(pose.shape)}; [B,24,3] or [B,72] axis-angle expected (pose2rot=True)")
        elif len(ps) != 4 or ps[1:] != (N_JOINTS, 3, 3):
            raise ValueError(f"BodyModel.forward: pose {ps}; [B,24,3,3] rotation matrices expected (pose2rot=False)")
        B = ps[0]
        if B < 1:
            raise ValueError("BodyModel.forward: no poses")
        if bs[0] not in (1, B):
            raise ValueError(f"BodyModel.forward: {bs[0]} rows of betas for {B} poses")
        if regressor is not None and regressor not in self.regressors:
            raise KeyError(f"BodyModel.forward: no regressor {regressor!r} (have {sorted(self.regressors)})")
        if not (want_vertices or joints or regressor is not None):
            raise ValueError("BodyModel.forward: no output asked for")
        return B

    def _to_device(self, x, who) -> torch.Tensor:
        if torch.is_tensor(x):
            if x.is_cuda and x.device != self.device:
                raise NotImplementedError(f"BodyModel: {who} on {x.device}, the body on {self.device}; several devices are not built")
            if x.requires_grad:
                raise NotImplementedError(f"BodyModel: {who} requires grad; forward gives no gradients through the body: call "
                                          "BodyModel.differentiable")
            if not x.dtype.is_floating_point:
                raise TypeError(f"BodyModel: {who} of dtype {x.dtype}; floating point expected")
            x = x.detach()
        else:
            x = np.asarray(x)
            if x.dtype.kind != "f":
                raise TypeError(f"BodyModel: {who} of dtype {x.dtype}; floating point expected")
            x = torch.from_numpy(np.ascontiguousarray(x, dtype=np.float32))
        return x

    @torch.no_grad()
    def forward(self, betas, pose=None, pose2rot=True, regressor: Optional[str] = None, want_vertices=False, joints=True, *,
                global_orient=None, body_pose=None, transl=None):
        """`lbs` and, with `regressor`, `vertices2joints` of that regressor: BodyOutput(vertices [B,V,3] | None, joints [B,24,3]
        (J_transformed) | None, regressed [B,K,3] | None), float32 device tensors; nothing synchronises.  `pose`: [B,24,3] or
        [B,72] axis-angle, or [B,24,3,3] rotation matrices with pose2rot=False; or `global_orient` + `body_pose` as SMPL.forward
        takes them (run_gan.py:1511).  `betas` [B,NB], or one row for all poses."""
        if transl is not None:
            raise NotImplementedError("BodyModel.forward: transl is not built")
        if pose is None:
            if global_orient is None or body_pose is None:
                raise ValueError("BodyModel.forward: pose, or global_orient and body_pose")
            go, bp = self._to_device(global_orient, "global_orient"), self._to_device(body_pose, "body_pose")
            tail = (3, 3) if not pose2rot else (3,)
            pose = torch.cat([go.reshape(go.shape[0], -1, *tail), bp.reshape(bp.shape[0], -1, *tail)], dim=1)
        betas, pose = self._to_device(betas, "betas"), self._to_device(pose, "pose")
        B = self._check_inputs(betas, pose, pose2rot, regressor, want_vertices, joints)
        f32 = lambda t: t.to(device=self.device, dtype=torch.float32).contiguous()
        betas, pose = f32(betas), f32(pose)
        reg = None if regressor is None else self.regressors[regressor]
        K = 0 if reg is None else reg.shape[0]
        new = lambda *shape: torch.empty(*shape, dtype=torch.float32, device=self.device)
        out = BodyOutput(new(B, self.V, 3) if want_vertices else None, new(B, N_JOINTS, 3) if joints else None,
                         new(B, K, 3) if reg is not None else None)
        with torch.cuda.device(self.device):
            _ffi.call(self.renderer, "pg_smpl_forward", C.byref(self._model), B, betas, self.NB if betas.shape[0] == B and B > 1 else 0,
                      pose, 0 if pose2rot else 1, reg, K, out.vertices, out.joints, out.regressed)
        return out

    __call__ = forward

    def differentiable(self, betas, pose=None, pose2rot=True, regressor: Optional[str] = None, want_vertices=False, joints=True, *,
                       global_orient=None, body_pose=None, transl=None):
        """`forward` with gradients: the same BodyOutput, the same bytes, differentiable once in `betas` and `pose` (or
        `global_orient` and `body_pose`).  The backward is one pg_smpl_backward call; an output that no cotangent reaches is passed as
        NULL.  Axis-angle poses get the derivative of `batch_rodrigues` as written (finite at a zero vector), rotation matrices a
        gradient in each of their nine entries.  One betas row for all poses gets the poses' rows added in float64 in pose order,
        rounded once (B - 1 small additions on the device, one after the other).  `betas` and `pose` must be floating-point tensors on the body's device."""
        if transl is not None:
            raise NotImplementedError("BodyModel.differentiable: transl is not built")
        if pose is None:
            if global_orient is None or body_pose is None:
                raise ValueError("BodyModel.differentiable: pose, or global_orient and body_pose")
            go, bp = self._on_device(global_orient, "global_orient"), self._on_device(body_pose, "body_pose")
            tail = (3, 3) if not pose2rot else (3,)
            pose = torch.cat([go.reshape(go.shape[0], -1, *tail), bp.reshape(bp.shape[0], -1, *tail)], dim=1)
        betas, pose = self._on_device(betas, "betas"), self._on_device(pose, "pose")
        self._check_inputs(betas, pose, pose2rot, regressor, want_vertices, joints)
        outs = list(_BodyFn.apply(self, betas, pose, bool(pose2rot), regressor, bool(want_vertices), bool(joints)))
        return BodyOutput(outs.pop(0) if want_vertices else None, outs.pop(0) if joints else None,
                          outs.pop(0) if regressor is not None else None)

    def _on_device(self, x, who) -> torch.Tensor:
        if not torch.is_tensor(x):
            raise NotImplementedError(f"BodyModel.differentiable: {who} is a host array; a tensor on {self.device} is expected")
        if x.device != self.device:
            raise NotImplementedError(f"BodyModel.differentiable: {who} on {x.device}, the body on {self.device}; host tensors and "
                                      "several devices are not built")
        if not x.dtype.is_floating_point:
            raise TypeError(f"BodyModel.differentiable: {who} of dtype {x.dtype}; floating point expected")
        return x

    def _blend_transposed(self) -> torch.Tensor:
        """blend as [3V, 1+NB+207], what pg_smpl_backward reads its d feat operand from; made on first use"""
        if getattr(self, "_blend_t", None) is None:
            self._blend_t = self._blend.t().contiguous()
        return self._blend_t

    @torch.no_grad()
    def vertex_errors(self, a, b):
        """(per_pose float64 [B], mean float64 scalar) of mean_v |a_v - b_v| (`ume` / `pme`, run_gan.py:1630-1631): device tensors"""
        return vertex_errors(self.renderer, a, b)


class _BodyFn(torch.autograd.Function):
    """pg_smpl_forward / pg_smpl_backward: the outputs that were asked for, in BodyOutput's order"""

    @staticmethod
    def forward(ctx, body, betas, pose, pose2rot, regressor, want_vertices, joints):
        f32 = lambda t: t.detach().to(dtype=torch.float32).contiguous()
        b32, p32 = f32(betas), f32(pose)
        out = body.forward(b32, p32, pose2rot=pose2rot, regressor=regressor, want_vertices=want_vertices, joints=joints)
        ctx.body, ctx.saved, ctx.regressor, ctx.pose2rot = body, (b32, p32), regressor, pose2rot
        ctx.which = [k for k, t in zip(BodyOutput._fields, out) if t is not None]
        ctx.meta = ((betas.dtype, tuple(betas.shape)), (pose.dtype, tuple(pose.shape)))
        ctx.set_materialize_grads(False)
        return tuple(t for t in out if t is not None)

    @staticmethod
    @once_differentiable
    def backward(ctx, *grads):
        body, (b32, p32) = ctx.body, ctx.saved
        need_b, need_p = ctx.needs_input_grad[1], ctx.needs_input_grad[2]
        g = {k: None if t is None else t.to(device=body.device, dtype=torch.float32).contiguous() for k, t in zip(ctx.which, grads)}
        if not (need_b or need_p) or all(t is None for t in g.values()):
            return (None,) * 7
        B = p32.shape[0]
        reg = None if ctx.regressor is None else body.regressors[ctx.regressor]
        d_betas = torch.empty(B, body.NB, dtype=torch.float32, device=body.device) if need_b else None
        d_pose = torch.empty_like(p32) if need_p else None
        with torch.cuda.device(body.device):
            _ffi.call(body.renderer, "pg_smpl_backward", C.byref(body._model), B, b32, body.NB if b32.shape[0] == B and B > 1 else 0,
                      p32, 0 if ctx.pose2rot else 1, reg, 0 if reg is None else reg.shape[0], body._blend_transposed(), g.get("vertices"),
                      g.get("joints"), g.get("regressed"), d_betas, d_pose)
        (bt, bs), (pt, ps) = ctx.meta
        if need_b and bs[0] != B:                            # one row for all poses: the rows in pose order, in float64, rounded once
            rows = d_betas.to(torch.float64)
            total = rows[0]
            for i in range(1, B):
                total = total + rows[i]
            d_betas = total[None].to(torch.float32)
        return (None, d_betas.to(bt).reshape(bs) if need_b else None, d_pose.to(pt).reshape(ps) if need_p else None, None, None, None, None)


@torch.no_grad()
def vertex_errors(renderer, a, b):
    """pg_vertex_errors on `renderer`'s handle: a, b [B,V,3] -> (per_pose float64 [B], their mean, a float64 device scalar)"""
    device = _ffi.device_of(renderer, "vertex_errors", ";")
    sa, sb = tuple(np.shape(a)), tuple(np.shape(b))
    if len(sa) != 3 or sa[2] != 3 or sa != sb or sa[0] < 1 or sa[1] < 1:
        raise ValueError(f"vertex_errors: a {sa} and b {sb} must both be [B,V,3]")
    f32 = lambda t: torch.as_tensor(t).detach().to(device=device, dtype=torch.float32).contiguous()
    a, b = f32(a), f32(b)
    per_pose = torch.empty(sa[0], dtype=torch.float64, device=device)
    summary = torch.empty(2, dtype=torch.float64, device=device)
    with torch.cuda.device(device):
        _ffi.call(renderer, "pg_vertex_errors", sa[0], sa[1], a, b, per_pose, summary)
    return per_pose, summary[1]
