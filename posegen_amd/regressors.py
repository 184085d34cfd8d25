"""The regression head of the SPIN / HMR regressor on the device (include/posegen_regressor.h, csrc/pg_hmr.hip).

`HMR.forward` (run_gan.py:1319-1358) is a ResNet-50 trunk and, on its features `xf` [B,2048], three rounds of cat([xf, pose, shape,
cam]) -> fc1 -> Dropout -> fc2 -> Dropout -> decpose / decshape / deccam -> residual add, then `rot6d_to_rotmat`: about 40 torch
operators forward and a hundred autograd nodes backward between two stages that already run as HIP kernels (the input batches of
`regressor_batches.py` in front, `ganloop.regressor_keypoints` / `regressor_loss` behind).  Here:

  HipHMRHead     an nn.Module with real nn.Linear children under the reference's names (`fc1`, `fc2`, `decpose`, `decshape`, `deccam`)
                 and its buffers (`init_pose`, `init_shape`, `init_cam`): the head's part of a reference state dict loads with
                 strict=True; Adam, clip_grad_norm_, .train() and .eval() work unchanged.  The children are never called: forward is
                 one autograd.Function over pg_hmr_head_forward and pg_hmr_head_backward.
  HipHMR         a trunk (any nn.Module images -> [B, n_feat]) and a head; `HipHMR.adopt(model)` takes both from an instance of the
                 reference's HMR and shares its head Parameters.  No ResNet is written here: the trunk stays with torch.
  stock_forward  the same computation as stock torch operators on whatever device and dtype the parameters are: what the tests and
                 tools/bench_hmr_head.py compare with.  Not a fallback: the modules never come here.

Differentiable once.  There is no torch fallback and no CPU path.
"""
from __future__ import annotations

import ctypes as C
from typing import Optional

import numpy as np
import torch
import torch.nn as nn
import torch.nn.functional as F
from torch.autograd.function import once_differentiable

from . import _ffi
from .discriminators import _renderer_for

LINEARS = ("fc1", "fc2", "decpose", "decshape", "deccam")


class HmrSpec:
    """The widths of one head: xf columns, hidden width, joints (six pose columns each), shape and camera columns, rounds, dropout p"""

    def __init__(self, n_feat: int = 2048, n_hidden: int = 1024, n_joints: int = 24, n_shape: int = 10, n_cam: int = 3, n_iter: int = 3,
                 p_drop: float = 0.5):
        self.n_feat, self.n_hidden, self.n_joints, self.n_shape, self.n_cam, self.n_iter = (int(v) for v in (n_feat, n_hidden, n_joints, n_shape,
                                                                                                                 n_cam, n_iter))
        self.p_drop = float(p_drop)
        lim = ((self.n_feat, 1, _ffi.PG_HMR_MAX_FEAT, "n_feat"), (self.n_hidden, 1, _ffi.PG_HMR_MAX_HIDDEN, "n_hidden"),
               (self.n_joints, 1, _ffi.PG_HMR_MAX_JOINTS, "n_joints"), (self.n_shape, 0, _ffi.PG_HMR_MAX_SHAPE, "n_shape"),
               (self.n_cam, 0, _ffi.PG_HMR_MAX_CAM, "n_cam"), (self.n_iter, 1, _ffi.PG_HMR_MAX_ITER, "n_iter"))
        for v, lo, hi, name in lim:
            if not lo <= v <= hi:
                raise ValueError(f"HmrSpec: {name} = {v}; {lo} .. {hi} expected")
        if not (np.isfinite(self.p_drop) and 0.0 <= self.p_drop < 1.0):
            raise ValueError(f"HmrSpec: p_drop = {self.p_drop}; a probability in [0, 1) expected")

    @property
    def n_pose(self) -> int:
        return 6 * self.n_joints

    @property
    def n_state(self) -> int:
        return self.n_pose + self.n_shape + self.n_cam

    def with_iter(self, n_iter: int) -> "HmrSpec":
        return HmrSpec(self.n_feat, self.n_hidden, self.n_joints, self.n_shape, self.n_cam, n_iter, self.p_drop)

    def shapes(self):
        """name -> shape of the ten tensors in the order of pg_hmr_params"""
        F_, H, S = self.n_feat, self.n_hidden, self.n_state
        return {"fc1_w": (H, F_ + S), "fc1_b": (H,), "fc2_w": (H, H), "fc2_b": (H,), "decpose_w": (self.n_pose, H), "decpose_b": (self.n_pose,),
                "decshape_w": (self.n_shape, H), "decshape_b": (self.n_shape,), "deccam_w": (self.n_cam, H), "deccam_b": (self.n_cam,)}

    def tape_layout(self, B: int):
        """the offsets of P, s_i (i = 0 .. n_iter), h1_i and h2_i into the tape, and its size (include/posegen_regressor.h)"""
        H, S, n = self.n_hidden, self.n_state, self.n_iter
        at = {"P": 0, "s": [B * H + i * B * S for i in range(n + 1)]}
        base = B * H + (n + 1) * B * S
        at["h1"] = [base + 2 * i * B * H for i in range(n)]
        at["h2"] = [base + (2 * i + 1) * B * H for i in range(n)]
        return at, base + 2 * n * B * H

    def c_spec(self) -> _ffi.PgHmrSpec:
        return _ffi.PgHmrSpec(n_feat=self.n_feat, n_hidden=self.n_hidden, n_joints=self.n_joints, n_shape=self.n_shape, n_cam=self.n_cam,
                              n_iter=self.n_iter, p_drop=self.p_drop)


def pointer_table(table, tensors):
    """`table` (a PgHmrParams or PgHmrGrads) with the ten `tensors` (in HMR_TENSORS order) as its device pointers; None or an empty
    tensor = a null pointer"""
    for name, t in zip(_ffi.HMR_TENSORS, tensors):
        setattr(table, name, None if t is None or t.numel() == 0 else t.data_ptr())
    return table


def draw_masks(spec: HmrSpec, B: int, device) -> torch.Tensor:
    """The keep masks of one training-mode call, uint8 [n_iter, 2, B, H], drawn on the device in the order round 0 drop1, round 0
    drop2, round 1, ...: an element is kept where a uniform draw is >= p.  Not nn.Dropout's own bits: those are not reproducible on the
    device (see HipHMRHead)."""
    return (torch.rand(spec.n_iter, 2, B, spec.n_hidden, device=device) >= spec.p_drop).to(torch.uint8)


class _HeadFn(torch.autograd.Function):
    """(pred_rotmat, pred_shape, pred_cam) of one call; the tape is kept for the backward"""

    @staticmethod
    def forward(ctx, renderer, spec, masks, xf, init, *params):
        B, dev = int(xf.shape[0]), xf.device
        cspec = spec.c_spec()
        _, n_f = spec.tape_layout(B)
        tape = torch.empty(n_f, dtype=torch.float32, device=dev)
        rotmat = torch.empty(B, spec.n_joints, 3, 3, dtype=torch.float32, device=dev)
        shape = torch.empty(B, spec.n_shape, dtype=torch.float32, device=dev)
        cam = torch.empty(B, spec.n_cam, dtype=torch.float32, device=dev)
        ctab = pointer_table(_ffi.PgHmrParams(), params)
        with torch.cuda.device(dev):
            _ffi.call(renderer, "pg_hmr_head_forward", C.byref(cspec), C.byref(ctab), xf, init, int(init.dim() == 2), masks, B, tape, rotmat,
                      shape if spec.n_shape else None, cam if spec.n_cam else None)
        ctx.renderer, ctx.spec = renderer, spec
        ctx.save_for_backward(tape, masks, xf, *params)
        return rotmat, shape, cam

    @staticmethod
    @once_differentiable
    def backward(ctx, g_rotmat, g_shape, g_cam):
        renderer, spec = ctx.renderer, ctx.spec
        tape, masks, xf, *params = ctx.saved_tensors
        B, dev = int(xf.shape[0]), xf.device
        need = ctx.needs_input_grad
        d_xf = torch.empty_like(xf) if need[3] else None
        d_init = torch.empty(B, spec.n_state, dtype=torch.float32, device=dev) if need[4] else None
        grads = [torch.empty_like(p) if w else None for p, w in zip(params, need[5:])]
        cot = [None if g is None or g.numel() == 0 else g.to(torch.float32).contiguous() for g in (g_rotmat, g_shape, g_cam)]
        if all(c is None for c in cot):
            cot[0] = torch.zeros(B, spec.n_joints, 3, 3, dtype=torch.float32, device=dev)
        cspec = spec.c_spec()
        ctab = pointer_table(_ffi.PgHmrParams(), params)
        gtab = pointer_table(_ffi.PgHmrGrads(), grads)
        with torch.cuda.device(dev):
            _ffi.call(renderer, "pg_hmr_head_backward", C.byref(cspec), C.byref(ctab), xf, masks, B, tape, cot[0], cot[1], cot[2], C.byref(gtab),
                      d_xf, d_init)
        grads = [torch.zeros_like(p) if (g is not None and p.numel() == 0) else g for g, p in zip(grads, params)]
        return (None, None, None, d_xf, d_init) + tuple(grads)


def _head_tensors(head):
    return [t for name in LINEARS for t in (getattr(head, name).weight, getattr(head, name).bias)]


class HipHMRHead(nn.Module):
    """The head of the reference's HMR (run_gan.py:1273-1298, 1343-1358).  State-dict keys `fc1.*`, `fc2.*`, `decpose.*`, `decshape.*`,
    `deccam.*` and the buffers `init_pose` [1,6J], `init_shape` [1,n_shape], `init_cam` [1,n_cam]; the reference's initialisation
    (nn.Linear's default, xavier_uniform_ with gain 0.01 on the three decoders).  `mean_params`: the reference's smpl_mean_params npz
    (a path, or a mapping with `pose`, `shape`, `cam`); None leaves the three buffers zero for a state dict to fill.

    forward(xf [B,n_feat], init_pose=None, init_shape=None, init_cam=None, n_iter=3, masks=None) -> (pred_rotmat [B,J,3,3],
    pred_shape [B,n_shape], pred_cam [B,n_cam]) float32 on the device.  In training mode the two Dropouts are live: `masks` (uint8 or
    bool [n_iter,2,B,H], non-zero = kept) are the call's keep masks; without `masks=` the module draws them on the device with
    torch.rand in the order round 0 drop1, round 0 drop2, round 1, ... (`draw_masks`).  torch's own dropout bits on the device are
    not reproducible -- nn.Dropout there draws from a Philox stream whose offsets depend on the launch geometry -- so a run of the
    reference under the same torch seed keeps other elements; the distribution is the same.  In eval mode without `masks=` there is
    no dropout.  Gradients reach the parameters, `xf` and any init given per row."""

    def __init__(self, n_feat: int = 2048, n_hidden: int = 1024, n_joints: int = 24, n_shape: int = 10, n_cam: int = 3, p_drop: float = 0.5,
                 mean_params=None, renderer=None):
        super().__init__()
        self.spec = HmrSpec(n_feat, n_hidden, n_joints, n_shape, n_cam, 3, p_drop)
        self.renderer = renderer
        S = self.spec.n_state
        self.fc1 = nn.Linear(n_feat + S, n_hidden)
        self.drop1 = nn.Dropout(p_drop)
        self.fc2 = nn.Linear(n_hidden, n_hidden)
        self.drop2 = nn.Dropout(p_drop)
        self.decpose = nn.Linear(n_hidden, self.spec.n_pose)
        self.decshape = nn.Linear(n_hidden, n_shape)
        self.deccam = nn.Linear(n_hidden, n_cam)
        for lin in (self.decpose, self.decshape, self.deccam):
            if lin.weight.numel():
                nn.init.xavier_uniform_(lin.weight, gain=0.01)
        pose, shape, cam = np.zeros(self.spec.n_pose, np.float32), np.zeros(n_shape, np.float32), np.zeros(n_cam, np.float32)
        if mean_params is not None:
            mp = np.load(mean_params) if isinstance(mean_params, (str, bytes)) or hasattr(mean_params, "__fspath__") else mean_params
            pose, shape, cam = (np.asarray(mp[k], dtype=np.float32).reshape(-1) for k in ("pose", "shape", "cam"))
        self.register_buffer("init_pose", torch.from_numpy(pose.copy()).unsqueeze(0))
        self.register_buffer("init_shape", torch.from_numpy(shape.copy()).unsqueeze(0))
        self.register_buffer("init_cam", torch.from_numpy(cam.copy()).unsqueeze(0))

    def forward(self, xf: torch.Tensor, init_pose=None, init_shape=None, init_cam=None, n_iter: int = 3, masks=None):
        who = type(self).__name__
        xf = torch.as_tensor(xf)
        renderer = _renderer_for(self.renderer, xf, who)
        s0 = self.spec
        spec = HmrSpec(s0.n_feat, s0.n_hidden, s0.n_joints, s0.n_shape, s0.n_cam, n_iter, float(self.drop1.p))
        if xf.dim() != 2 or xf.shape[1] != spec.n_feat or not 1 <= xf.shape[0] <= _ffi.PG_HMR_MAX_ROWS:
            raise ValueError(f"{who}: xf {tuple(xf.shape)}; [B, {spec.n_feat}] with 1 <= B <= {_ffi.PG_HMR_MAX_ROWS} expected")
        B = int(xf.shape[0])
        xf = xf.to(torch.float32).contiguous()
        params = _head_tensors(self)
        for t, (name, shape) in zip(params, spec.shapes().items()):
            if t.device != xf.device or t.dtype != torch.float32 or not t.is_contiguous():
                raise NotImplementedError(f"{who}: a parameter on {t.device} as {t.dtype}; contiguous float32 on {xf.device} expected")
            if tuple(t.shape) != shape:
                raise ValueError(f"{who}: {name} {tuple(t.shape)}; {shape} expected")
        given = (init_pose, init_shape, init_cam)
        buffers = (self.init_pose, self.init_shape, self.init_cam)
        if all(g is None for g in given):
            init = torch.cat([b.reshape(-1) for b in buffers]).to(device=xf.device, dtype=torch.float32).contiguous()
        else:
            cols = (spec.n_pose, spec.n_shape, spec.n_cam)
            parts = [(b.expand(B, -1) if g is None else torch.as_tensor(g).reshape(B, c)).to(device=xf.device, dtype=torch.float32)
                     for g, b, c in zip(given, buffers, cols)]
            init = torch.cat(parts, 1).contiguous()
        if masks is None and self.training:
            masks = draw_masks(spec, B, xf.device)
        if masks is not None:
            masks = torch.as_tensor(masks)
            if tuple(masks.shape) != (spec.n_iter, 2, B, spec.n_hidden):
                raise ValueError(f"{who}: masks {tuple(masks.shape)}; {(spec.n_iter, 2, B, spec.n_hidden)} expected")
            masks = masks.to(device=xf.device).ne(0).to(torch.uint8).contiguous()
        return _HeadFn.apply(renderer, spec, masks, xf, init, *params)


class _Trunk(nn.Module):
    """`conv1 ... avgpool` of an HMR instance, called in HMR.forward's order (run_gan.py:1330-1341); the modules are the instance's own"""

    def __init__(self, model):
        super().__init__()
        for name in ("conv1", "bn1", "relu", "maxpool", "layer1", "layer2", "layer3", "layer4", "avgpool"):
            setattr(self, name, getattr(model, name))

    def forward(self, x):
        x = self.maxpool(self.relu(self.bn1(self.conv1(x))))
        x = self.layer4(self.layer3(self.layer2(self.layer1(x))))
        x = self.avgpool(x)
        return x.view(x.size(0), -1)


class HipHMR(nn.Module):
    """A regressor: `trunk` (any nn.Module that maps images to [B, n_feat]; torch's own convolutions) and a `HipHMRHead`.
    forward(x, init_pose=None, init_shape=None, init_cam=None, n_iter=3, masks=None) as the reference's HMR.forward."""

    def __init__(self, trunk: nn.Module, head: HipHMRHead):
        super().__init__()
        self.trunk, self.head = trunk, head

    def forward(self, x, init_pose=None, init_shape=None, init_cam=None, n_iter: int = 3, masks=None):
        xf = self.trunk(x)
        return self.head(xf.reshape(xf.shape[0], -1), init_pose, init_shape, init_cam, n_iter, masks)

    @classmethod
    def adopt(cls, model: nn.Module, renderer=None) -> "HipHMR":
        """`model`: an instance of the reference's HMR (or the module of a SPIN checkpoint): its own `conv1 ... avgpool` become the
        trunk, and the head takes the instance's `fc1`, `fc2`, `decpose`, `decshape`, `deccam` modules themselves and its three init
        buffers: the Parameters are shared by identity, so an optimiser built on `model` and `model.state_dict()` keep working, and
        `model.train()` / `.eval()` on the result set the head's mode."""
        fc1, decpose, decshape, deccam = model.fc1, model.decpose, model.decshape, model.deccam
        if decpose.out_features % 6:
            raise ValueError(f"HipHMR.adopt: decpose has {decpose.out_features} outputs; a multiple of 6 expected")
        S = decpose.out_features + decshape.out_features + deccam.out_features
        p = float(model.drop1.p) if hasattr(model, "drop1") else 0.5
        head = HipHMRHead(fc1.in_features - S, fc1.out_features, decpose.out_features // 6, decshape.out_features, deccam.out_features, p,
                          renderer=renderer)
        for name in LINEARS:
            setattr(head, name, getattr(model, name))
        for name in ("init_pose", "init_shape", "init_cam"):
            head._buffers[name] = getattr(model, name)
        head.train(model.training)
        return cls(_Trunk(model), head)


# ---- the same computation as stock torch operators ---------------------------------------------------------------------------------------
def rot6d_to_rotmat(x: torch.Tensor) -> torch.Tensor:
    """run_gan.py:1188-1202 in torch's own operators: [.., 6] -> [N,3,3]"""
    x = x.reshape(-1, 3, 2)
    a1, a2 = x[:, :, 0], x[:, :, 1]
    b1 = F.normalize(a1)
    b2 = F.normalize(a2 - torch.einsum("bi,bi->b", b1, a2).unsqueeze(-1) * b1)
    b3 = torch.cross(b1, b2, dim=-1)
    return torch.stack((b1, b2, b3), dim=-1)


def stock_forward(head, xf: torch.Tensor, init_pose=None, init_shape=None, init_cam=None, n_iter: int = 3, masks=None):
    """The head of `HMR.forward` as the reference runs it: `head`'s own nn.Linear children (a HipHMRHead or a reference HMR) called as
    stock torch operators, on whatever device and dtype they are.  `masks` [n_iter,2,B,H] (non-zero = kept) stand in for the two
    nn.Dropouts: a kept element is x * (1 / (1 - p)), a dropped one 0; without `masks` the module's mode decides (F.dropout in training
    mode).  Not a fallback -- `HipHMRHead.forward` never comes here."""
    w = head.fc1.weight
    xf = torch.as_tensor(xf).to(device=w.device, dtype=w.dtype)
    B = xf.shape[0]
    p = float(head.drop1.p) if hasattr(head, "drop1") else 0.5
    pose, shape, cam = ((b.expand(B, -1) if g is None else torch.as_tensor(g)).to(device=w.device, dtype=w.dtype)
                        for g, b in zip((init_pose, init_shape, init_cam), (head.init_pose, head.init_shape, head.init_cam)))
    if masks is not None:
        masks = torch.as_tensor(masks).to(w.device).ne(0)

    def drop(x, i, which):
        if masks is None:
            return F.dropout(x, p, head.training)
        return torch.where(masks[i, which], x * (1.0 / (1.0 - p)), torch.zeros((), dtype=x.dtype, device=x.device))
    for i in range(n_iter):
        xc = drop(head.fc1(torch.cat([xf, pose, shape, cam], 1)), i, 0)
        xc = drop(head.fc2(xc), i, 1)
        pose = head.decpose(xc) + pose
        shape = head.decshape(xc) + shape
        cam = head.deccam(xc) + cam
    return rot6d_to_rotmat(pose).view(B, -1, 3, 3), shape, cam
