"""The pose generator of the PoseGen loop on the device (include/posegen_generator.h, csrc/pg_gen.hip).

`PoseGenerator` (run_gan.py:767-980) is a `BAGenerator` and an `RTGenerator`: three noise MLPs, each five layers of
Linear -> BatchNorm1d -> LeakyReLU with the BatchNorm in training mode (`model_G.train()` is set and never unset).  As torch
operators that is about 60 launches forward and three times that backward on [1024, 256] problems.  Here:

  HipBAGenerator / HipRTGenerator / HipPoseGenerator
                        nn.Modules whose children are real nn.Linear / nn.BatchNorm1d under the reference's names in its __init__
                        order (a reference state dict loads with strict=True; `apply(init_weights)`, Adam, clip_grad_norm_, .train()
                        and .eval() work unchanged); the children are never called: forward is one autograd.Function over
                        pg_gen_trunk_forward, pg_gen_ba_head_forward and pg_gen_rt_head (five launches for all trunks, one per head)
                        and backward over pg_gen_ba_head_backward and pg_gen_trunk_backward
  draw_noise            the reference's draws in its order: BA noise, R noise, the three `eps` columns of torch.normal, T noise

Differentiable once, in training mode only (a gradient asked of an eval-mode forward raises RuntimeError).  `R`, `T` and `pose_rt`
carry no graph -- the loop reads them and never differentiates them -- so `w2_T` and every RT parameter keep `grad None`, as does
`w2_R`, which the reference never applies.  There is no torch fallback and no CPU path.
"""
from __future__ import annotations

import ctypes as C
from typing import Dict, List, Optional, Sequence, Tuple

import numpy as np
import torch
import torch.nn as nn
from torch.autograd.function import once_differentiable

from . import _ffi
from .discriminators import _renderer_for

NOISE_KEYS = ("ba", "r", "eps", "t")


class GenSpec:
    """The trunks of one call: (nz, width, n_stages) each, with LeakyReLU's slope and BatchNorm1d's eps and momentum"""

    def __init__(self, trunks: Sequence[Tuple[int, int, int]], slope: float = 0.01, eps: float = 1e-5, momentum: float = 0.1):
        self.trunks = [(int(nz), int(width), int(n)) for nz, width, n in trunks]
        self.slope, self.eps, self.momentum = float(slope), float(eps), float(momentum)
        if not 1 <= len(self.trunks) <= _ffi.PG_GEN_MAX_TRUNKS:
            raise ValueError(f"GenSpec: {len(self.trunks)} trunks; 1 .. {_ffi.PG_GEN_MAX_TRUNKS} expected")
        if not (np.isfinite(self.slope) and self.slope >= 0.0):
            raise ValueError(f"GenSpec: slope = {self.slope}; a finite slope >= 0 expected")
        if not (np.isfinite(self.eps) and self.eps > 0.0) or not 0.0 <= self.momentum <= 1.0:
            raise ValueError(f"GenSpec: eps = {self.eps}, momentum = {self.momentum}")
        for nz, width, n in self.trunks:
            if not (1 <= nz <= _ffi.PG_GEN_MAX_DIM and 1 <= width <= _ffi.PG_GEN_MAX_DIM and 0 <= n <= _ffi.PG_GEN_MAX_STAGES):
                raise ValueError(f"GenSpec: trunk ({nz}, {width}, {n}); nz and width in 1 .. {_ffi.PG_GEN_MAX_DIM}, stages in 0 .. "
                                 f"{_ffi.PG_GEN_MAX_STAGES} expected")

    def layers(self, t: int) -> int:
        return 1 + 2 * self.trunks[t][2]

    def layer_shapes(self, t: int) -> List[Tuple[int, int]]:
        """(out, in) of the Linears of trunk t"""
        nz, width, _ = self.trunks[t]
        return [(width, nz if l == 0 else width) for l in range(self.layers(t))]

    def tape_layout(self, B: int):
        """per trunk and layer the offsets (z, scale, shift) into the float tape and (mean, var) into the double one, and the two
        sizes (include/posegen_generator.h)"""
        out, f, d = [], 0, 0
        for t, (_, width, _) in enumerate(self.trunks):
            layers = []
            for _ in range(self.layers(t)):
                layers.append({"z": f, "scale": f + B * width, "shift": f + B * width + width, "mean": d, "var": d + width})
                f += (B + 2) * width
                d += 2 * width
            out.append(layers)
        return out, f, d

    def c_spec(self) -> _ffi.PgGenSpec:
        s = _ffi.PgGenSpec(n_trunks=len(self.trunks), slope=self.slope, eps=self.eps, momentum=self.momentum)
        for t, (nz, width, n) in enumerate(self.trunks):
            s.trunk[t].nz, s.trunk[t].width, s.trunk[t].n_stages = nz, width, n
        return s


def pointer_table(table, spec: GenSpec, fields: Dict[str, Sequence[Sequence[Optional[torch.Tensor]]]]):
    """`table` (a PgGenParams or PgGenGrads) with fields[name][t][l] as its device pointers; None = a null pointer"""
    for name, per_trunk in fields.items():
        dst = getattr(table, name)
        for t, per_layer in enumerate(per_trunk):
            for l, x in enumerate(per_layer):
                dst[t][l] = None if x is None else x.data_ptr()
    return table


def pointer_array(tensors: Sequence[Optional[torch.Tensor]]):
    """a host array of per-trunk device pointers (noise, d_out)"""
    return _ffi._GEN_PTRS(*[None if x is None else x.data_ptr() for x in tensors])


def draw_noise(B: int, device, nz_ba: Optional[int] = 32, nz_rt: Optional[int] = 72) -> Dict[str, torch.Tensor]:
    """The generator's draws in the reference's order (run_gan.py:869, 945, 955, 963): BAGenerator's noise, RTGenerator's R noise, the
    [B,3] standard normals behind `torch.normal(mean, std)`, its T noise.  None leaves that generator's draws out."""
    out = {}
    if nz_ba is not None:
        out["ba"] = torch.randn(B, nz_ba, device=device)
    if nz_rt is not None:
        out["r"] = torch.randn(B, nz_rt, device=device)
        out["eps"] = torch.randn(B, 3, device=device)
        out["t"] = torch.randn(B, nz_rt, device=device)
    return out


class _Stage(nn.Module):
    """run_gan.py's `Linear`: two width -> width layers; never called"""

    def __init__(self, width: int):
        super().__init__()
        self.w1 = nn.Linear(width, width)
        self.batch_norm1 = nn.BatchNorm1d(width)
        self.w2 = nn.Linear(width, width)
        self.batch_norm2 = nn.BatchNorm1d(width)


def _trunk_layers(stem: nn.Linear, stem_bn: nn.BatchNorm1d, stages) -> List[Tuple[nn.Linear, nn.BatchNorm1d]]:
    out = [(stem, stem_bn)]
    for s in stages:
        out += [(s.w1, s.batch_norm1), (s.w2, s.batch_norm2)]
    return out


class _GenFn(torch.autograd.Function):
    """(pose_ba, R, T, pose_rt) of the trunks in `plan` in one grouped call; the tape is kept for the backward of pose_ba"""

    @staticmethod
    def forward(ctx, renderer, plan, x, *params):
        spec, B, J, dev = plan["spec"], plan["B"], plan["J"], plan["device"]
        cspec = spec.c_spec()
        _, n_f, n_d = spec.tape_layout(B)
        tape = torch.empty(n_f, dtype=torch.float32, device=dev)
        stats = torch.empty(n_d, dtype=torch.float64, device=dev)
        ctab = pointer_table(_ffi.PgGenParams(), spec, plan["tables"])
        noise = pointer_array(plan["noise"])
        pose_ba = R = T = pose_rt = y = None
        with torch.cuda.device(dev):
            _ffi.call(renderer, "pg_gen_trunk_forward", C.byref(cspec), C.byref(ctab), noise, B, int(plan["training"]), tape, stats)
            if plan["ba"] is not None:
                w2, b2 = params[plan["ba_w2"]], params[plan["ba_w2"] + 1]
                y = torch.empty(B, 4 * J, dtype=torch.float32, device=dev)
                pose_ba = torch.empty(B, J, 3, dtype=torch.float32, device=dev)
                _ffi.call(renderer, "pg_gen_ba_head_forward", C.byref(cspec), plan["ba"], tape, B, J, w2, b2, y, pose_ba)
            if plan["rt"] is not None:
                tr, tt = plan["rt"]
                R = torch.empty(B, 3, 3, dtype=torch.float32, device=dev)
                T = torch.empty(B, 3, dtype=torch.float32, device=dev)
                pose_rt = torch.empty(B, J, 3, dtype=torch.float32, device=dev)
                _ffi.call(renderer, "pg_gen_rt_head", C.byref(cspec), tr, tt, tape, B, J, plan["w2_t"], plan["b2_t"], plan["eps"], x, R, T, pose_rt)
        ctx.renderer, ctx.plan = renderer, plan
        ctx.save_for_backward(tape, stats, y, *params)
        outs = tuple(torch.empty(0, device=dev) if o is None else o for o in (pose_ba, R, T, pose_rt))
        ctx.mark_non_differentiable(*outs[1:])
        return outs

    @staticmethod
    @once_differentiable
    def backward(ctx, g_pose, *_unused):
        renderer, plan = ctx.renderer, ctx.plan
        spec, B, J, dev = plan["spec"], plan["B"], plan["J"], plan["device"]
        if not plan["training"]:
            raise RuntimeError("the pose generator's backward exists in training mode only (BatchNorm's batch statistics); "
                               "call .train(), or run the eval-mode forward under torch.no_grad()")
        tape, stats, y, *params = ctx.saved_tensors
        want = ctx.needs_input_grad[3:]
        grads: List[Optional[torch.Tensor]] = [torch.empty_like(p) if w else None for p, w in zip(params, want)]
        t_ba = plan["ba"]
        n_layers = spec.layers(t_ba)
        fields = {k: [[None] * spec.layers(t) for t in range(len(spec.trunks))] for k in ("w", "b", "gamma", "beta")}
        for l in range(n_layers):
            for i, k in enumerate(("w", "b", "gamma", "beta")):
                fields[k][t_ba][l] = grads[4 * l + i]
        d_w2, d_b2 = grads[plan["ba_w2"]], grads[plan["ba_w2"] + 1]
        trunk_wanted = any(want[:4 * n_layers])
        d_h = torch.empty(B, spec.trunks[t_ba][1], dtype=torch.float32, device=dev) if trunk_wanted else None
        cspec = spec.c_spec()
        g = g_pose.to(torch.float32).contiguous()
        with torch.cuda.device(dev):
            _ffi.call(renderer, "pg_gen_ba_head_backward", C.byref(cspec), t_ba, tape, B, J, params[plan["ba_w2"]], y, g, d_w2, d_b2, d_h)
            if trunk_wanted:
                ctab = pointer_table(_ffi.PgGenParams(), spec, plan["tables"])
                gtab = pointer_table(_ffi.PgGenGrads(), spec, fields)
                d_out = pointer_array([d_h if t == t_ba else None for t in range(len(spec.trunks))])
                _ffi.call(renderer, "pg_gen_trunk_backward", C.byref(cspec), C.byref(ctab), pointer_array(plan["noise"]), B, 1, tape, stats, d_out,
                          C.byref(gtab))
        return (None, None, None) + tuple(grads)


class _GeneratorBase(nn.Module):
    """What the three modules share: the trunks' (Linear, BatchNorm1d) lists, the checks, the grouped call"""

    slope = 0.01                                   # nn.LeakyReLU()

    def _run(self, inputs_3d: torch.Tensor, ba, rt, noise) -> Tuple[Optional[torch.Tensor], ...]:
        who = type(self).__name__
        x = torch.as_tensor(inputs_3d)
        renderer = _renderer_for(self.renderer, x, who)
        B = int(x.shape[0])
        J = (ba.n_joints if ba is not None else x.numel() // max(1, 3 * B))
        if B < 1 or x.numel() != B * J * 3:
            raise ValueError(f"{who}: input {tuple(x.shape)}; [B, {J}, 3] expected")
        if not 1 <= J <= _ffi.PG_GEN_MAX_JOINTS or B > _ffi.PG_GEN_MAX_ROWS:
            raise ValueError(f"{who}: {B} poses of {J} joints; at most {_ffi.PG_GEN_MAX_ROWS} of {_ffi.PG_GEN_MAX_JOINTS}")
        if self.training and B < 2:
            raise ValueError(f"{who}: Expected more than 1 value per channel when training, got input size {[B, 0]}")
        x = x.detach().to(torch.float32).reshape(B, J, 3).contiguous()
        trunks: List[List[Tuple[nn.Linear, nn.BatchNorm1d]]] = []
        if ba is not None:
            trunks.append(ba.trunk_layers())
        if rt is not None:
            trunks += [rt.trunk_layers("R"), rt.trunk_layers("T")]
        bns = [bn for layers in trunks for _, bn in layers]
        b0 = bns[0]
        for bn in bns:
            if bn.eps != b0.eps or bn.momentum != b0.momentum or bn.momentum is None or not bn.track_running_stats or not bn.affine:
                raise NotImplementedError(f"{who}: BatchNorm1d layers with one eps, one momentum, affine and running statistics expected")
        spec = GenSpec([(layers[0][0].in_features, layers[0][0].out_features, (len(layers) - 1) // 2) for layers in trunks], self.slope,
                       b0.eps, b0.momentum)
        if noise is None:
            noise = draw_noise(B, x.device, None if ba is None else ba.noise_channle, None if rt is None else rt.noise_channle)
        elif not isinstance(noise, dict):
            noise = dict(zip(NOISE_KEYS if ba is not None else NOISE_KEYS[1:], noise))
        keys = (["ba"] if ba is not None else []) + (["r", "t"] if rt is not None else [])
        draws = {}
        for k, cols in zip(keys + (["eps"] if rt is not None else []), [t[0] for t in spec.trunks] + [3]):
            if k not in noise:
                raise ValueError(f"{who}: noise[{k!r}] is missing")
            draws[k] = torch.as_tensor(noise[k]).detach().to(device=x.device, dtype=torch.float32).reshape(B, cols).contiguous()
        flat: List[torch.Tensor] = []
        if ba is not None:
            for lin, bn in trunks[0]:
                flat += [lin.weight, lin.bias, bn.weight, bn.bias]
            flat += [ba.w2.weight, ba.w2.bias]
        every = flat + [t for layers in trunks for lin, bn in layers for t in (lin.weight, lin.bias, bn.weight, bn.bias, bn.running_mean, bn.running_var)]
        if rt is not None:
            every += [rt.w2_T.weight, rt.w2_T.bias]
        for t in every:
            if t.device != x.device or t.dtype != torch.float32 or not t.is_contiguous():
                raise NotImplementedError(f"{who}: a parameter on {t.device} as {t.dtype}; contiguous float32 on {x.device} expected")
        tables = {"w": [[lin.weight for lin, _ in layers] for layers in trunks], "b": [[lin.bias for lin, _ in layers] for layers in trunks],
                  "gamma": [[bn.weight for _, bn in layers] for layers in trunks], "beta": [[bn.bias for _, bn in layers] for layers in trunks],
                  "running_mean": [[bn.running_mean for _, bn in layers] for layers in trunks],
                  "running_var": [[bn.running_var for _, bn in layers] for layers in trunks]}
        plan = {"spec": spec, "B": B, "J": J, "device": x.device, "training": bool(self.training), "tables": tables,
                "noise": [draws[k] for k in keys], "ba": 0 if ba is not None else None, "ba_w2": len(flat) - 2,
                "rt": None if rt is None else (len(trunks) - 2, len(trunks) - 1)}
        if rt is not None:
            plan["w2_t"], plan["b2_t"], plan["eps"] = rt.w2_T.weight.detach(), rt.w2_T.bias.detach(), draws["eps"]
        if not flat:
            # the RT generator alone: nothing is differentiable, and autograd needs no node
            with torch.no_grad():
                outs = _GenFn.apply(renderer, plan, x)
        else:
            outs = _GenFn.apply(renderer, plan, x, *flat)
        if self.training:
            torch._foreach_add_([bn.num_batches_tracked for bn in bns], 1)
        return tuple(o if o.numel() else None for o in outs)


class HipBAGenerator(_GeneratorBase):
    """BAGenerator (run_gan.py:818-896): noise [B,noise_channle] -> five BatchNorm layers -> w2 -> [B,24,4] -> axis / |axis| theta,
    joint 0 times 6.28.  State-dict keys `w1`, `batch_norm1`, `linear_stages.{i}.w1/batch_norm1/w2/batch_norm2`, `w2`.
    forward(inputs_3d, noise=None) -> pose_ba [B,24,3] float32 on the device; inputs_3d gives B and the device, as in the reference.
    A joint whose axis is exactly zero comes out NaN, as in the reference."""

    def __init__(self, input_size: int = 24 * 3, noise_channle: int = 72, linear_size: int = 256, num_stage: int = 2, p_dropout: float = 0.5,
                 renderer=None):
        super().__init__()
        self.linear_size, self.p_dropout, self.num_stage, self.noise_channle, self.input_size = linear_size, p_dropout, num_stage, noise_channle, input_size
        self.n_joints, self.renderer = 24, renderer                                # (the reference's literal 24*4)
        self.w1 = nn.Linear(noise_channle, linear_size)
        self.batch_norm1 = nn.BatchNorm1d(linear_size)
        self.linear_stages = nn.ModuleList([_Stage(linear_size) for _ in range(num_stage)])
        self.w2 = nn.Linear(linear_size, self.n_joints * 4)

    def trunk_layers(self):
        return _trunk_layers(self.w1, self.batch_norm1, self.linear_stages)

    def forward(self, inputs_3d: torch.Tensor, noise=None) -> torch.Tensor:
        if noise is not None and not isinstance(noise, dict):
            noise = {"ba": noise}
        return self._run(inputs_3d, self, None, noise)[0]


class HipRTGenerator(_GeneratorBase):
    """RTGenerator (run_gan.py:899-980): two noise trunks; the R trunk's output itself gives the axis mean, spread and angle (w2_R exists
    and is never applied), the T trunk goes through w2_T.  forward(inputs_3d [B,J,3], noise=None) -> (R [B,3,3], T [B,3], pose_rt
    [B,J,3]) without a graph."""

    def __init__(self, input_size: int = 24 * 3, noise_channle: int = 72, linear_size: int = 256, num_stage: int = 2, p_dropout: float = 0.5,
                 renderer=None):
        super().__init__()
        self.linear_size, self.p_dropout, self.num_stage, self.noise_channle, self.input_size = linear_size, p_dropout, num_stage, noise_channle, input_size
        self.renderer = renderer
        self.w1_R = nn.Linear(noise_channle, linear_size)
        self.batch_norm_R = nn.BatchNorm1d(linear_size)
        self.linear_stages_R = nn.ModuleList([_Stage(linear_size) for _ in range(num_stage)])
        self.w1_T = nn.Linear(noise_channle, linear_size)
        self.batch_norm_T = nn.BatchNorm1d(linear_size)
        self.linear_stages_T = nn.ModuleList([_Stage(linear_size) for _ in range(num_stage)])
        self.w2_R = nn.Linear(linear_size, 7)
        self.w2_T = nn.Linear(linear_size, 3)

    def trunk_layers(self, which: str):
        if which == "R":
            return _trunk_layers(self.w1_R, self.batch_norm_R, self.linear_stages_R)
        return _trunk_layers(self.w1_T, self.batch_norm_T, self.linear_stages_T)

    def forward(self, inputs_3d: torch.Tensor, noise=None):
        return self._run(inputs_3d, None, self, noise)[1:]


class HipPoseGenerator(_GeneratorBase):
    """PoseGenerator (run_gan.py:793-815): `BAprocess` (noise of 32) and `RTprocess`; forward(inputs_3d [B,24,3], noise=None) -> the
    reference's dict.  All three trunks go through one grouped launch per layer.  `noise`: a dict (or a tuple in this order) of `ba`
    [B,32], `r` [B,72], `eps` [B,3], `t` [B,72] in place of the torch.randn draws."""

    def __init__(self, args=None, input_size: int = 24 * 3, renderer=None):
        super().__init__()
        self.renderer = renderer
        self.BAprocess = HipBAGenerator(input_size=24 * 3, noise_channle=32, renderer=renderer)
        self.RTprocess = HipRTGenerator(input_size=24 * 3, renderer=renderer)

    def forward(self, inputs_3d: torch.Tensor, noise=None):
        pose_ba, R, T, pose_rt = self._run(inputs_3d, self.BAprocess, self.RTprocess, noise)
        return {"pose_ba": pose_ba, "ba_diff": None, "pose_bl": None, "blr": None, "pose_rt": pose_rt, "R": R, "T": T}


# ---- the same modules as stock torch operators ---------------------------------------------------------------------------------------------
def _axis_angle_to_matrix(v: torch.Tensor) -> torch.Tensor:
    """pytorch3d.transforms.axis_angle_to_matrix: rotation vector -> quaternion -> matrix"""
    ang = torch.linalg.norm(v, dim=-1, keepdim=True)
    small = ang.abs() < 1e-6
    k = torch.where(small, 0.5 - ang * ang / 48, torch.sin(0.5 * ang) / torch.where(small, torch.ones_like(ang), ang))
    q = torch.cat([torch.cos(0.5 * ang), v * k], -1)
    r, i, j, kk = torch.unbind(q, -1)
    two_s = 2.0 / (q * q).sum(-1)
    o = torch.stack([1 - two_s * (j * j + kk * kk), two_s * (i * j - kk * r), two_s * (i * kk + j * r),
                     two_s * (i * j + kk * r), 1 - two_s * (i * i + kk * kk), two_s * (j * kk - i * r),
                     two_s * (i * kk - j * r), two_s * (j * kk + i * r), 1 - two_s * (i * i + j * j)], -1)
    return o.reshape(v.shape[:-1] + (3, 3))


def stock_forward(module: HipPoseGenerator, inputs_3d: torch.Tensor, noise=None, masks=None):
    """`PoseGenerator.forward` as the reference runs it: the module's own nn.Linear / nn.BatchNorm1d children called as stock torch
    operators, on whatever device and dtype they are.  Not a fallback -- `HipPoseGenerator.forward` never comes here: this is what
    tools/bench_generator.py measures the device route against and what the tests build their CPU twins from.  `masks`: per BA layer
    a boolean array that replaces LeakyReLU's own `y > 0` (the tests feed the device's masks to both backwards)."""
    ba, rt = module.BAprocess, module.RTprocess
    lin0 = ba.w1.weight
    B = inputs_3d.shape[0]
    if noise is None:
        noise = draw_noise(B, lin0.device, ba.noise_channle, rt.noise_channle)
    elif not isinstance(noise, dict):
        noise = dict(zip(NOISE_KEYS, noise))
    noise = {k: torch.as_tensor(v).to(device=lin0.device, dtype=lin0.dtype) for k, v in noise.items()}
    slope = module.slope

    def trunk(layers, h, ms=None):
        for l, (lin, bn) in enumerate(layers):
            y = bn(lin(h))
            h = torch.nn.functional.leaky_relu(y, slope) if ms is None else y * torch.where(ms[l], torch.ones((), dtype=y.dtype, device=y.device), torch.full((), slope, dtype=y.dtype, device=y.device))
        return h
    y = ba.w2(trunk(ba.trunk_layers(), noise["ba"], masks)).view(B, -1, 4)
    axis = y[:, :, :3] / torch.linalg.norm(y[:, :, :3], dim=-1, keepdim=True)
    pose_ba = axis * y[:, :, 3:4]
    pose_ba = torch.cat([pose_ba[:, :1] * (3.14 * 2), pose_ba[:, 1:]], 1)
    r = trunk(rt.trunk_layers("R"), noise["r"])
    r_axis = r[:, :3] + r[:, 3:6] * r[:, 3:6] * noise["eps"]
    r_axis = r_axis / torch.linalg.norm(r_axis, dim=-1, keepdim=True) * r[:, 6:7]
    R = _axis_angle_to_matrix(r_axis)
    t = rt.w2_T(trunk(rt.trunk_layers("T"), noise["t"]))
    t = torch.cat([t[:, :2], t[:, 2:3] * t[:, 2:3]], 1)
    x = inputs_3d.to(device=lin0.device, dtype=lin0.dtype).reshape(B, -1, 3)
    pose_rt = torch.matmul(R, (x - x[:, :1]).permute(0, 2, 1)).permute(0, 2, 1) + t[:, None, :]
    return {"pose_ba": pose_ba, "ba_diff": None, "pose_bl": None, "blr": None, "pose_rt": pose_rt, "R": R, "T": t, "y": y.reshape(B, -1)}
