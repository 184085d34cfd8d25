"""Deterministic edge inputs for the per-point tests of the fused embed + MLP kernels (tests/test_gpu_eval_points.py), built on
the CPU, a few hundred to ~1500 points each: the smallest shape that still has the edge.  tests/test_eval_ref_host.py checks on
the CPU that every case can tell a deliberate error (tests/eval_ref.py MUTATIONS) from a precision's rounding.

Every array is float32: the kernels and the float64 restatement read the same values."""
from dataclasses import dataclass, field
from functools import lru_cache
from typing import Optional

import numpy as np
import torch

from posegen_amd import synthetic as syn
from posegen_amd.config import h36m_config, surreal_config
from tests import eval_ref as er

LOG2E = 1.4426950408889634
TAU_MODEL = 79.6                        # what synthetic.make_model returns
SEED = {"surreal": 0, "h36m": 5}        # the model seeds of the rays_surreal / rays_h36m fixtures


def config_of(model):
    return surreal_config(n_samples=64, n_importance=16) if model == "surreal" else h36m_config(n_samples=64, n_importance=16)


@lru_cache(maxsize=None)
def model(name):
    """(cfg, coarse weights, fine weights) of the named synthetic model"""
    cfg = config_of(name)
    wc, wf, _, _ = syn.make_model(cfg, SEED[name])
    return cfg, wc, wf


@dataclass
class Case:
    name: str
    model: str                                  # "surreal" (no frame codes) / "h36m" (frame codes)
    skts: np.ndarray                            # [1|n,24,4,4]
    cutoff_v: np.ndarray = field(default_factory=lambda: np.full(24, 0.5, np.float32))
    cutoff_d: np.ndarray = field(default_factory=lambda: np.full(24, 0.5, np.float32))
    tau_v: float = TAU_MODEL
    tau_d: float = TAU_MODEL
    ray_batch: Optional[np.ndarray] = None      # [n,11]
    z: Optional[np.ndarray] = None              # [n,S]
    cams: Optional[np.ndarray] = None           # None / [1] / [n]
    pts: Optional[np.ndarray] = None            # [P,3]: explicit points of query_density (then no rays)
    note: dict = field(default_factory=dict)    # what the builder knows about the case (indices of the special points, ...)

    @property
    def S(self):
        return self.z.shape[1]

    @property
    def n_points(self):
        return self.pts.shape[0] if self.pts is not None else self.z.size

    def far_radius(self):
        """the kernels' far-skip radius per joint: max over the embedders of cutoff + 24 / (tau log2 e); inf for tau <= 0"""
        r = lambda c, t: c + 24.0 / (t * LOG2E) if t > 0 else np.full(24, np.inf)
        return np.maximum(r(self.cutoff_v.astype(np.float64), self.tau_v), r(self.cutoff_d.astype(np.float64), self.tau_d))

    def reference(self, which, quant=None, mut=None):
        """tests/eval_ref.py on the case: dict raw, pre0 (float64 tensors)"""
        cfg, wc, wf = model(self.model)
        w = wf if which else wc
        emb = (self.cutoff_v, self.cutoff_d, self.tau_v, self.tau_d)
        if self.pts is not None:
            return er.eval_points(w, self.pts, self.skts, *emb, quant=quant, mut=mut)
        return er.eval_rays(w, self.ray_batch, self.z, self.skts, *emb, cams=self.cams, quant=quant, mut=mut)


# ---------------------------------------------------------------------------------------------- bounds
# Against float64, the project's bounds of test_stage_eval_coarse: tol x max(1, |raw|max / 10) on raw, an absolute bound on the
# layer-0 pre-activation.  16-bit: what operand rounding alone does to the case (the yardstick D, measured on the CPU with the
# restatement's `quant`) plus the bound that test holds the kernels to against that emulation.
EXACT_TOL = {"fp32": 4e-5, "bf16x3": 3e-4, "fp16c": 9e-4}
EXACT_TAP_TOL = {"fp32": 2e-5, "bf16x3": 4e-5, "fp16c": 4e-5}
EMUL_TOL = {"bf16": 4e-2, "fp16": 8e-3}
RMS_FACTOR = 2.0        # the kernels round a few operands the other way than the direct form: independent errors of equal size
_CACHE = {}


def reference(case, which):
    """the float64 restatement on the case, computed once per session"""
    key = (case.name, which)
    if key not in _CACHE:
        _CACHE[key] = case.reference(which)
    return _CACHE[key]


def yardstick(case, which, quant):
    """D of a 16-bit precision on the case: how far its operand rounding alone (no kernel) moves raw and the layer-0
    pre-activation from float64, as max-abs and RMS; `scale` = |raw|max of the float64 result.  Sigma only for explicit points."""
    key = (case.name, which, quant)
    if key not in _CACHE:
        ref, emu = reference(case, which), case.reference(which, quant=quant)
        sel = (lambda r: r[..., 3:4]) if case.pts is not None else (lambda r: r)
        d, d0 = sel(emu["raw"]) - sel(ref["raw"]), emu["pre0"] - ref["pre0"]
        _CACHE[key] = {"max": float(d.abs().max()), "rms": float(d.pow(2).mean().sqrt()), "max0": float(d0.abs().max()),
                       "scale": float(sel(ref["raw"]).abs().max())}
    return _CACHE[key]


def bound_exact(prec, scale):
    return EXACT_TOL[prec] * max(1.0, scale / 10)


def bound_16bit(prec, y):
    return y["max"] + EMUL_TOL[prec] * max(1.0, y["scale"] / 10)


# ---------------------------------------------------------------------------------------------- building blocks
def poses(n, seed):
    """kps [n,24,3], skts [n,24,4,4] float32"""
    _, kps, skts = syn.make_pose(n, seed)
    return kps, skts


def camera_origin():
    c2ws, _ = syn.make_camera(1, 64, 64)
    return c2ws[0, :3, 3].astype(np.float64)


def jittered(rng, n, S, half):
    """S irregular, strictly ascending offsets in (-half, half) per ray: one per stratum, at least a tenth of a stratum apart"""
    return ((np.arange(S) + rng.uniform(0.05, 0.95, size=(n, S))) / S * 2 - 1) * half


def rays_at(targets, rng, S, half=0.6, scale=(0.8, 1.25)):
    """Rays from the camera through `targets` [n,3], not of unit length, with S irregular ascending depths over
    +- `half` (world units) around the target -> ray_batch [n,11], z [n,S]"""
    targets = np.asarray(targets, dtype=np.float64)
    n = targets.shape[0]
    o = camera_origin()
    dist = np.linalg.norm(targets - o, axis=-1, keepdims=True)
    d = (targets - o) / dist * rng.uniform(*scale, size=(n, 1))
    dn = np.linalg.norm(d, axis=-1, keepdims=True)
    z = dist / dn + jittered(rng, n, S, half) / dn
    return ray_batch_of(np.repeat(o[None], n, 0), d), z.astype(np.float32)


def tangent_rays(jpos, rho, rng, S, half):
    """Unit rays from the camera whose closest approach to `jpos` is rho[i] exactly (float64), with a sample there"""
    o = camera_origin()
    jpos = np.asarray(jpos, dtype=np.float64)
    D = np.linalg.norm(jpos - o)
    u = (jpos - o) / D
    perp = np.cross(u, [0.0, 1.0, 0.0])
    perp /= np.linalg.norm(perp)
    sin = np.asarray(rho, dtype=np.float64) / D
    cos = np.sqrt(1 - sin * sin)
    d = cos[:, None] * u + sin[:, None] * perp
    z = D * cos[:, None] + jittered(rng, len(sin), S, half)
    z[:, S // 2] = D * cos
    z.sort(axis=1)
    return ray_batch_of(np.repeat(o[None], len(sin), 0), d), z.astype(np.float32)


def ray_batch_of(o, d):
    o, d = np.asarray(o, dtype=np.float32), np.asarray(d, dtype=np.float32)
    n = o.shape[0]
    vd = d / np.linalg.norm(d.astype(np.float64), axis=-1, keepdims=True)
    return np.concatenate([o, d, np.zeros((n, 1)), np.ones((n, 1)), vd], -1).astype(np.float32)


def body_targets(kps_per_ray, rng, jitter=0.1, joints=None):
    """one joint per ray (`joints`, or cycling through the skeleton with a stride coprime to 24) plus a jitter"""
    n = kps_per_ray.shape[0]
    j = (np.arange(n) * 7 + 3) % 24 if joints is None else np.asarray(joints)
    return kps_per_ray[np.arange(n), j].astype(np.float64) + rng.uniform(-jitter, jitter, size=(n, 3))


def far_targets(kps, rng, n, away=6.0):
    """targets whose rays pass `away` world units beside the body: no joint within any far-skip radius of this file"""
    o = camera_origin()
    root = kps[0].astype(np.float64)
    axis = np.cross(root - o, [0.0, 1.0, 0.0])
    axis /= np.linalg.norm(axis)
    return root + axis * away + rng.uniform(-0.2, 0.2, size=(n, 3))


def min_joint_distance(c: Case):
    """float64 distance of every point to its nearest joint / of every (point, joint): [n,S,24]"""
    pts = c.pts.reshape(-1, 1, 3) if c.pts is not None else (c.ray_batch[:, None, 0:3].astype(np.float64)
                                                             + c.ray_batch[:, None, 3:6].astype(np.float64) * c.z[..., None].astype(np.float64))
    return torch.linalg.norm(er.bone_local(pts, c.skts), dim=-1).numpy()


# ---------------------------------------------------------------------------------------------- the cases
SEAM_N = (7, 13)
SEAM_S = (32, 33, 64, 65, 112, 113)


@lru_cache(maxsize=None)
def seams(n, S):
    """Every ray its own pose (3 poses in blocks of 2 rays) and its own frame code; n S is no multiple of 128: rays, poses and
    codes change inside waves and passes, the last pass is ragged, and at S = 64 / 65 a 256-point pass overlaps 5 rays.  A point
    that takes a neighbour's pose, code or depth moves by O(0.1)."""
    assert (n * S) % 128 != 0
    rng = np.random.RandomState(1000 + 31 * n + S)
    kps3, skts3 = poses(3, 31)
    pid = (np.arange(n) // 2) % 3
    rb, z = rays_at(body_targets(kps3[pid], rng), rng, S)
    cfg = config_of("h36m")
    cams = ((np.arange(n) * 11 + 5) % cfg.n_framecodes).astype(np.float32)
    return Case(f"seams[{n}x{S}]", "h36m", skts3[pid].copy(), ray_batch=rb, z=z, cams=cams, note={"pose_of_ray": pid})


CUTOFF_TAUS = ((4.0, TAU_MODEL), (TAU_MODEL, 400.0), (400.0, 4.0), (TAU_MODEL, -4.0))


@lru_cache(maxsize=None)
def cutoffs(tau_v, tau_d, S=64):
    """Per-joint cutoffs in [0.3, 0.7], drawn separately for the two embedders; rays through the body whose depths span +- 1.2,
    so that every joint has points inside and outside its far-skip radius; and two rays that pass joint 21 (a wrist: no other
    joint near) at the far-skip radius times (1 -+ 2^-18) with a sample at the closest approach: the limb is at the mask
    threshold from either side.  tau_d = -4 (a learned tau <= 0: the weight GROWS with distance, no radius bounds it)."""
    rng = np.random.RandomState(77)
    cut_v = rng.uniform(0.3, 0.7, 24).astype(np.float32)
    cut_d = rng.uniform(0.3, 0.7, 24).astype(np.float32)
    kps, skts = poses(1, 33)
    joints = (1, 7, 8, 12, 18, 19, 20, 22, 23)          # (legs, trunk, head and both arms: every joint is near one of the rays)
    n_body = len(joints)
    rb, z = rays_at(body_targets(np.repeat(kps, n_body, 0), rng, joints=joints), rng, S, half=1.2)
    c = Case(f"cutoffs[{tau_v:g},{tau_d:g},S={S}]", "surreal", skts, cut_v, cut_d, float(tau_v), float(tau_d))
    radius = c.far_radius()[21]
    if np.isfinite(radius) and radius < 2.0:
        rho = radius * np.array([1 - 2.0 ** -18, 1 + 2.0 ** -18])
        rb2, z2 = tangent_rays(kps[0, 21], rho, rng, S, half=1.2)
        rb, z = np.concatenate([rb, rb2]), np.concatenate([z, z2])
        c.note["threshold_rays"] = (n_body, n_body + 1)
    c.ray_batch, c.z = rb, z
    return c


@lru_cache(maxsize=None)
def on_joint(S=64):
    """Joint 17's transform is the identity with a dyadic translation and ray 2 is dyadic with a sample at z = 1 exactly on the
    joint: (R o + t) + z (R d) is exactly 0 in fp32, as a + z b and as R p + t.  Its neighbours lie at 2^-10 .. 2^-4 times |d|
    from the joint on either side."""
    rng = np.random.RandomState(17)
    kps, skts = poses(1, 35)
    skts = skts.copy()
    jpos = np.array([0.5, 0.25, 1.5])
    skts[0, 17] = np.eye(4, dtype=np.float32)
    skts[0, 17, :3, 3] = -jpos
    d = np.array([0.5, -0.25, 1.0])
    kp_rays = np.repeat(kps, 4, 0)
    rb, z = rays_at(body_targets(kp_rays, rng), rng, S)
    near = np.concatenate([1 - 2.0 ** -np.arange(4, 11), [1.0], 1 + 2.0 ** -np.arange(10, 3, -1)])
    fill = np.sort(np.concatenate([rng.uniform(0.3, 0.875, (S - 15) // 2), rng.uniform(1.125, 1.7, S - 15 - (S - 15) // 2)]))
    zj = np.sort(np.concatenate([near, fill])).astype(np.float32)
    rb = np.concatenate([rb[:2], ray_batch_of((jpos - d)[None], d[None]), rb[2:]])
    z = np.concatenate([z[:2], zj[None], z[2:]])
    k = int(np.where(zj == 1.0)[0][0])
    return Case(f"on_joint[{S}]", "surreal", skts, ray_batch=rb, z=z, note={"ray": 2, "sample": k, "joint": 17})


@lru_cache(maxsize=None)
def all_far(layout, S=64):
    """Rays that miss every limb's radius: raw is the net's empty-space output and the weight ring starts fully masked.
    layout "all": every ray; "first": the first 256 points (the whole first pass) far, the later passes through the body; "last":
    only the last, ragged pass far."""
    rng = np.random.RandomState({"all": 1, "first": 2, "last": 3}[layout])
    kps, skts = poses(1, 37)
    per256 = 256 // S
    far_rays = {"all": [True] * 5, "first": [True] * per256 + [False] * 6, "last": [False] * per256 + [True] * 3}[layout]
    n = len(far_rays)
    tg = np.where(np.array(far_rays)[:, None], far_targets(kps[0], rng, n), body_targets(np.repeat(kps, n, 0), rng))
    rb, z = rays_at(tg, rng, S)
    return Case(f"all_far[{layout},S={S}]", "surreal", skts, ray_batch=rb, z=z, note={"far_rays": np.array(far_rays)})


@lru_cache(maxsize=None)
def codes(one_element, S=64):
    """frame-code indices -1 (the mean row), 0 and n_codes - 1 mixed per ray, or one index for every ray"""
    rng = np.random.RandomState(41)
    kps, skts = poses(1, 39)
    n = 9
    rb, z = rays_at(body_targets(np.repeat(kps, n, 0), rng), rng, S)
    last = config_of("h36m").n_framecodes - 1
    cams = np.array([last], np.float32) if one_element else np.array([-1, 0, last, last, -1, 0, 0, last, -1], np.float32)
    return Case(f"codes[{'one' if one_element else 'mixed'},S={S}]", "h36m", skts, ray_batch=rb, z=z, cams=cams)


@lru_cache(maxsize=None)
def ties(S=64):
    """ascending depths with runs of 2 .. 5 equal values; ray 3 has one depth for all of its samples (first == last)"""
    rng = np.random.RandomState(43)
    kps, skts = poses(1, 45)
    n = 5
    rb, z = rays_at(body_targets(np.repeat(kps, n, 0), rng), rng, S)
    for r in range(n):
        i = 1
        while i < S - 1:
            run = int(rng.randint(2, 6))
            z[r, i:i + run] = z[r, i]
            i += run + int(rng.randint(1, 4))
    z[3, :] = z[3, S // 2]
    assert (np.diff(z, axis=1) >= 0).all() and (np.diff(z, axis=1) == 0).any()
    return Case(f"ties[S={S}]", "surreal", skts, ray_batch=rb, z=z)


@lru_cache(maxsize=None)
def points(count):
    """Explicit points for query_density: point 0 exactly on joint 17 (the dyadic transform of on_joint), then -- counts above
    1 -- joint 21 at its far-skip radius times (1 -+ 2^-18), a point 6 units away, and points around the body."""
    rng = np.random.RandomState(100 + count)
    base = on_joint(64)
    kps, _ = poses(1, 35)
    pts = [np.array([0.5, 0.25, 1.5])]
    c = Case(f"points[{count}]", "surreal", base.skts)
    if count > 1:
        radius = c.far_radius()[21]
        jpos = kps[0, 21].astype(np.float64)
        u = np.array([0.6, 0.0, 0.8])
        pts += [jpos + u * radius * (1 - 2.0 ** -18), jpos + u * radius * (1 + 2.0 ** -18), kps[0, 0] + np.array([6.0, 0.0, 0.0])]
        j = rng.randint(0, 24, count - 4)
        pts += list(kps[0, j].astype(np.float64) + rng.uniform(-0.4, 0.4, (count - 4, 3)))
    c.pts = np.stack(pts).astype(np.float32)
    assert c.pts.shape == (count, 3)
    return c
