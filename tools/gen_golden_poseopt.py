#!/usr/bin/env python3
"""tests/golden/poseopt.npz from the REAL reference's PoseOptLayer (core/pose_opt.py:240-445), use_rot6d, under its own autograd.

Runs only where the reference checkout exists, through tools/gen_golden.py's import shims (its cases are not touched).  The
reference needs pytorch3d's axis_angle_to_matrix in PoseOptLayer.__init__ only; pytorch3d is stubbed, so the stub gets a Rodrigues
stand-in -- and `layer.bones.data` is then OVERWRITTEN with seeded 6-D values that are not orthonormal: both normalisations are
exercised and the stand-in cannot reach a stored number.  Every joint has |a1| >= 0.5 and 30 deg <= angle(a1, a2) <= 150 deg
(asserted): no case sits near a normalisation's eps.

Two variants in one file, arrays only: 5 poses, 8 rays over 3 unique poses (unsorted, repeated), one shared rest pose (keys
without suffix) and per-pose rest poses (suffix _pp).  Stored: the parameters, `idxs`, the five outputs, seeded cotangents for
kps / skts / l2ws / rots, and pelvis.grad / bones.grad of sum(output * cotangent).

Usage:  python tools/gen_golden_poseopt.py [--ref /root/reference] [--out tests/golden]
"""
from __future__ import annotations

import argparse
import os
import sys

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "tools"))
sys.dont_write_bytecode = True

N_KPS = 5
IDXS = np.array([4, 1, 4, 0, 1, 4, 0, 4], dtype=np.int64)
REST_IDXS = np.array([2, 0, 1, 4, 3], dtype=np.int64)


def _rodrigues(axisang):
    import torch
    w = axisang.double()
    t = w.norm(dim=-1).clamp_min(1e-12)[..., None, None]
    K = torch.zeros(w.shape[:-1] + (3, 3), dtype=torch.float64)
    K[..., 0, 1], K[..., 0, 2], K[..., 1, 0] = -w[..., 2], w[..., 1], w[..., 2]
    K[..., 1, 2], K[..., 2, 0], K[..., 2, 1] = -w[..., 0], -w[..., 1], w[..., 0]
    return (torch.eye(3, dtype=torch.float64) + torch.sin(t) / t * K + (1 - torch.cos(t)) / (t * t) * (K @ K)).to(axisang.dtype)


def seeded_rot6d(rng):
    """[N_KPS,24,6] float32 6-D parameters away from the normalisations' singularities"""
    out = np.zeros((N_KPS, 24, 3, 2), dtype=np.float32)
    for p in range(N_KPS):
        for j in range(24):
            while True:
                a1, a2 = rng.normal(0, 1, 3), rng.normal(0, 1, 3)
                ang = np.degrees(np.arccos(np.clip(a1 @ a2 / (np.linalg.norm(a1) * np.linalg.norm(a2)), -1, 1)))
                if np.linalg.norm(a1) >= 0.6 and np.linalg.norm(a2) >= 0.6 and 35.0 <= ang <= 145.0:
                    break
            out[p, j, :, 0], out[p, j, :, 1] = a1, a2
    return out.reshape(N_KPS, 24, 6)


def check_conditioning(b6):
    x = b6.astype(np.float64).reshape(-1, 3, 2)
    a1, a2 = x[..., 0], x[..., 1]
    n1, n2 = np.linalg.norm(a1, axis=-1), np.linalg.norm(a2, axis=-1)
    ang = np.degrees(np.arccos(np.clip((a1 * a2).sum(-1) / (n1 * n2), -1, 1)))
    assert n1.min() >= 0.5, n1.min()
    assert 30.0 <= ang.min() and ang.max() <= 150.0, (ang.min(), ang.max())
    return float(n1.min()), float(ang.min()), float(ang.max())


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--ref", default="/root/reference")
    ap.add_argument("--out", default=os.path.join(REPO, "tests", "golden"))
    a = ap.parse_args()
    import gen_golden
    gen_golden._install_shims(a.ref)
    import torch
    from core.utils import skeleton_utils
    skeleton_utils.p3dr.axis_angle_to_matrix = _rodrigues           # (the stubbed module as the reference bound it)
    from core.pose_opt import PoseOptLayer
    from posegen_amd.skeleton import smpl_rest_pose

    rng = np.random.RandomState(20)
    kps0 = rng.normal(0, 0.5, (N_KPS, 24, 3)).astype(np.float32)
    bones0 = rng.normal(0, 0.3, (N_KPS, 24, 3)).astype(np.float32)
    b6 = seeded_rot6d(rng)
    print("conditioning: min |a1| %.3f, angle(a1, a2) in [%.1f, %.1f] deg" % check_conditioning(b6))
    rest_shared = smpl_rest_pose[None].astype(np.float32)
    rest_pp = (smpl_rest_pose[None] * rng.uniform(0.8, 1.2, (N_KPS, 1, 1)) + rng.normal(0, 0.02, (N_KPS, 24, 3))).astype(np.float32)
    n = len(IDXS)
    cot = {"kps": rng.normal(0, 1, (n, 24, 3)), "skts": rng.normal(0, 1, (n, 24, 4, 4)), "l2ws": rng.normal(0, 1, (n, 24, 4, 4)),
           "rots": rng.normal(0, 1, (n, 24, 3, 3))}
    cot = {k: v.astype(np.float32) for k, v in cot.items()}
    d = {"idxs": IDXS, "rest_pose_idxs_pp": REST_IDXS}
    for sfx, rest, ridx in (("", rest_shared, None), ("_pp", rest_pp, REST_IDXS)):
        layer = PoseOptLayer(torch.tensor(kps0), torch.tensor(bones0), rest, use_rot6d=True, rest_pose_idxs=ridx)
        assert tuple(layer.bones.shape) == (N_KPS, 24, 6)
        layer.bones.data = torch.tensor(b6)
        kp, bone, skts, l2ws, rots = layer(IDXS)
        loss = sum((o * torch.tensor(cot[k])).sum() for k, o in (("kps", kp), ("skts", skts), ("l2ws", l2ws), ("rots", rots)))
        loss.backward()
        d.update({f"pelvis{sfx}": layer.pelvis.detach().numpy(), f"bones_param{sfx}": layer.bones.detach().numpy(),
                  f"rest_pose{sfx}": layer.rest_pose.numpy(), f"kps{sfx}": kp.detach().numpy(), f"bones{sfx}": bone.detach().numpy(),
                  f"skts{sfx}": skts.detach().numpy(), f"l2ws{sfx}": l2ws.detach().numpy(), f"rots{sfx}": rots.detach().numpy(),
                  f"pelvis_grad{sfx}": layer.pelvis.grad.numpy(), f"bones_grad{sfx}": layer.bones.grad.numpy()})
        names = {k: tuple(v.shape) for k, v in layer.state_dict().items()}
        print(f"[poseopt{sfx}] state dict {names}; max |bones.grad| {float(layer.bones.grad.abs().max()):.3e}")
    for k, v in cot.items():
        d[f"d_{k}"] = v
    path = os.path.join(a.out, "poseopt.npz")
    np.savez_compressed(path, **d)
    print(f"wrote {path}: {os.path.getsize(path)} bytes")


if __name__ == "__main__":
    main()
