#!/usr/bin/env python3
"""tests/golden/train_losses.npz from the REAL reference's Trainer (core/trainer.py): `compute_loss` (`_compute_nerf_loss` for both
passes, `_compute_kp_loss` with opt_rot6d and the temporal term) under its own float32 autograd, and `get_gradnorm`.

Runs only where the reference checkout exists; `core.trainer` imports plainly (os, torch, numpy).  The pose layer the temporal term
calls is a table look-up here (`popt_layer(idx)` -> the table's rows, numpy indexing, so -1 is the last pose as in the reference).

Stored per case `<case>/<name>`: the float32 inputs, the settings, the reference's losses and stats as it reports them (float32,
`.item()`), `alpha = acc_map.mean()` (trainer.py:271) and the gradients `total_loss.backward()` leaves on the inputs.  kp cases hold the
pose tables and `kp_idx`; the per-ray rots / kps are the table's rows (as `popt_layer(kp_idx)` returns them) and of `d_rots` only
columns 0 and 1 are stored (column 2 is asserted zero here).

Planted exact values: a zero difference under L1; |d| = beta = 0.125 under Huber (both with use_background off, so d is exact in
float32 and float64); x = tol = 0.015625 in kp_loss; acc of exactly 0 and 1 under BCE; rays with y = 1.0.  Every OTHER element is
asserted to stay 1e-5 away from the Huber knee and 1e-6 tol away from the kp_loss threshold, so a float32 and a float64 evaluation
cannot take different branches.

Usage:  python tools/gen_golden_train_losses.py [--ref /root/reference] [--out tests/golden]
"""
import argparse
import os
import sys
from types import SimpleNamespace

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

PHOTO_CASES = {
    # name: n, loss_fn, use_background, per-ray bgs, reg_fn, coarse pass, coarse_weight
    "mse_scalar": dict(n=37, loss_fn="MSE", use_background=True, bgs=False, reg_fn=None, coarse=False, coarse_weight=1.0),
    "l1_bgs_bce_coarse": dict(n=200, loss_fn="L1", use_background=True, bgs=True, reg_fn="BCE", coarse=True, coarse_weight=0.5),
    "huber_nobg_coarse": dict(n=101, loss_fn="Huber", use_background=False, bgs=False, reg_fn=None, coarse=True, coarse_weight=1.0),
    "huber_bgs_bce": dict(n=64, loss_fn="Huber", use_background=True, bgs=True, reg_fn="BCE", coarse=False, coarse_weight=1.0),
    "mse_nobg_bce_coarse": dict(n=129, loss_fn="MSE", use_background=False, bgs=True, reg_fn="BCE", coarse=True, coarse_weight=0.5),
    "l1_scalar_coarse": dict(n=77, loss_fn="L1", use_background=True, bgs=False, reg_fn=None, coarse=True, coarse_weight=0.5),
    "planted_l1_zero": dict(n=40, loss_fn="L1", use_background=False, bgs=False, reg_fn=None, coarse=False, coarse_weight=1.0, plant="zero"),
    "planted_huber_knee": dict(n=40, loss_fn="Huber", loss_beta=0.125, use_background=False, bgs=False, reg_fn=None, coarse=True,
                               coarse_weight=0.5, plant="knee"),
    "planted_bce": dict(n=48, loss_fn="L1", use_background=True, bgs=True, reg_fn="BCE", coarse=True, coarse_weight=0.5, plant="bce"),
}
KP_CASES = {
    "kp_tol0": dict(n=37, N=5, tol=0.0, temporal=False),
    "kp_tol001_temp": dict(n=37, N=5, tol=0.01, temporal=True),
    "kp_planted": dict(n=37, N=4, tol=0.015625, temporal=False, plant=True),
}
NORM_SHAPES = [(1,), (3,), (128,), (257,), (256, 7)]
REG_COEF, POSE_COEF, TEMP_COEF, EXT_SCALE = 0.1, 2.0, 0.05, 0.001


def _args(**kw):
    base = dict(loss_fn="MSE", loss_beta=0.1, reg_fn=None, use_background=True, coarse_weight=1.0, reg_coef=REG_COEF, opt_rot6d=True,
                opt_pose_tol=0.01, opt_pose_coef=POSE_COEF, use_temp_loss=False, temp_coef=TEMP_COEF, ext_scale=EXT_SCALE)
    base.update(kw)
    return SimpleNamespace(**base)


def _trainer(T, args, popt_kwargs=None):
    return T.Trainer(args, {"hwf": (0, 0, 0.0)}, None, None, {}, {}, popt_kwargs=popt_kwargs, device="cpu")


def photo_case(T, name, c, rng, out):
    n, beta = c["n"], c.get("loss_beta", 0.1)
    f32 = lambda a: np.ascontiguousarray(a, dtype=np.float32)
    q = lambda a: np.round(a * 64.0) / 64.0                       # multiples of 1/64: sums and differences exact in float32
    maps = {"rgb_map": rng.uniform(0, 1, (n, 3)), "acc_map": rng.uniform(0.02, 0.98, n)}
    if c["coarse"]:
        maps.update(rgb0=rng.uniform(0, 1, (n, 3)), acc0=rng.uniform(0.02, 0.98, n))
    target = rng.uniform(0, 1, (n, 3))
    fgs = np.where(rng.uniform(size=n) < 0.4, 1.0, rng.uniform(0, 0.9, n))
    bgs = rng.uniform(0, 1, (n, 3))
    plant = c.get("plant")
    planted = np.zeros((n, 3), dtype=bool)
    if plant in ("zero", "knee"):
        target = q(target)
        for k in ("rgb_map", "rgb0"):
            if k in maps:
                maps[k] = q(maps[k])
        planted[::3, 1] = True
        planted[1::5, 2] = True
        off = 0.0 if plant == "zero" else beta
        for k in ("rgb_map", "rgb0"):
            if k in maps:
                sign = np.where(np.arange(n)[:, None] % 2 == 0, 1.0, -1.0)
                maps[k] = np.where(planted, target + sign * off, maps[k])
                hit = ~planted & (np.abs(np.abs(maps[k] - target) - off) < 1e-5)      # only the planted elements sit on the value
                maps[k] = np.where(hit, maps[k] + 1.0 / 64.0, maps[k])
    if plant == "bce":
        fgs[:12] = [0.0, 0.0, 0.5, 0.5, 0.25, 0.75, 1.0, 1.0, 1.0, 0.0, 0.5, 1.0]
        for k in ("acc_map", "acc0"):
            maps[k][:12] = [0.0, 1.0, 0.0, 1.0, 1.0, 0.0, 0.0, 1.0, 0.5, 0.5, 0.5, 0.25]
    maps = {k: f32(v) for k, v in maps.items()}
    target, fgs, bgs = f32(target), f32(fgs), f32(bgs)
    if c["loss_fn"] == "Huber":                                    # no other element near the knee: float32 and float64 take the same branch
        for tag in ("", "0"):
            if ("rgb0" if tag else "rgb_map") not in maps:
                continue
            pred = maps["rgb0" if tag else "rgb_map"].astype(np.float64)
            if c["use_background"]:
                pred = pred + (1.0 - maps["acc0" if tag else "acc_map"].astype(np.float64))[:, None] * (bgs if c["bgs"] else 1.0)
            gap = np.abs(np.abs(pred - target) - beta)
            assert (gap[~planted] >= 1e-5).all(), f"{name}: an element within 1e-5 of the Huber knee; change the seed"
            if plant == "knee":
                assert (gap[planted] == 0).all()
    args = _args(loss_fn=c["loss_fn"], loss_beta=beta, reg_fn=c["reg_fn"], use_background=c["use_background"], coarse_weight=c["coarse_weight"])
    preds = {k: torch.tensor(v, requires_grad=True) for k, v in maps.items()}
    batch = {"target_s": torch.tensor(target), "fgs": torch.tensor(fgs)[:, None]}
    if c["bgs"]:
        batch["bgs"] = torch.tensor(bgs)
    loss_dict, stats = _trainer(T, args).compute_loss(batch, preds, popt_detach=True)
    assert loss_dict["total_loss"].dim() == 0
    loss_dict["total_loss"].backward()
    p = f"{name}/"
    for k, v in maps.items():
        out[p + k] = v
        g = preds[k].grad
        out[p + "d_" + k] = np.zeros_like(v) if g is None else g.numpy()
    out[p + "target"], out[p + "fgs"] = target, fgs
    if c["bgs"]:
        out[p + "bgs"] = bgs
    for k in ("loss_fn", "reg_fn"):
        out[p + k] = np.array(str(c[k]))
    for k, v in (("loss_beta", beta), ("use_background", int(c["use_background"])), ("coarse_weight", c["coarse_weight"]), ("reg_coef", REG_COEF)):
        out[p + k] = np.array(v)
    for k, v in loss_dict.items():
        out[p + "ref_" + k] = np.array(v.item(), dtype=np.float64)
    for k, v in stats.items():
        out[p + "ref_" + k] = np.array(v, dtype=np.float64)
    out[p + "ref_alpha"] = np.array(preds["acc_map"].mean().item(), dtype=np.float64)


class _TableLayer:
    """popt_layer of the temporal term: the poses' rows by numpy indexing"""

    def __init__(self, kps, rots):
        self.kps, self.rots, self.bones = kps, rots, rots      # (len(popt_layer.bones) is the pose count)

    def __call__(self, idx):
        idx = np.asarray(idx)
        return self.kps[idx], self.rots[idx], None, None, self.rots[idx]


def kp_case(T, name, c, rng, out):
    n, N, tol = c["n"], c["N"], c["tol"]
    f32 = lambda a: np.ascontiguousarray(a, dtype=np.float32)
    rots = rng.normal(0, 0.5, (N, 24, 3, 3))
    kps = rng.normal(0, 0.3, (N, 24, 3))
    a_rots = rots + rng.normal(0, 0.1, rots.shape)
    a_kps = kps + rng.normal(0, 0.02, kps.shape)
    planted = np.zeros((N, 24, 3, 3), dtype=bool)
    if c.get("plant"):
        rots = np.round(rots * 256.0) / 256.0
        planted[:, 1::4, :, 0] = True
        planted[:, 2::7, 1, 1] = True
        a_rots = np.where(planted, rots + 0.125, a_rots)          # x = 0.125^2 = tol exactly: excluded by the strict >
    rots, kps, a_rots, a_kps = f32(rots), f32(kps), f32(a_rots), f32(a_kps)
    kp_idx = rng.randint(0, N, n).astype(np.int64)
    kp_idx[:3] = [0, N - 1, 0]                                    # the wrap of the temporal term: 0 - 1 -> the last pose, N - 1 + 1 -> 0
    temp_val = f32(np.where(rng.uniform(size=n) < 0.3, 0.0, 1.0))
    x = (a_rots.astype(np.float64) - rots.astype(np.float64))[:, 1:, :, :2] ** 2
    t32 = float(np.float32(tol))
    near = np.abs(x - t32) < 1e-6 * t32
    assert not near[~planted[:, 1:, :, :2]].any(), f"{name}: an element within 1e-6 tol of the threshold; change the seed"
    if c.get("plant"):
        assert (x[planted[:, 1:, :, :2]] == t32).all()
    assert ((x > t32).mean() > 0.1) and ((x > t32).mean() < 0.9 or tol == 0.0)
    args = _args(opt_pose_tol=tol, use_temp_loss=c["temporal"])
    r_ray = torch.tensor(rots[kp_idx], requires_grad=True)
    k_ray = torch.tensor(kps[kp_idx], requires_grad=True)
    layer = _TableLayer(torch.tensor(kps), torch.tensor(rots))
    tr = _trainer(T, args, {"popt_layer": layer, "popt_anchors": {"rots": torch.tensor(a_rots), "kps": torch.tensor(a_kps)}})
    batch = {"kp_idx": kp_idx, "temp_val": torch.tensor(temp_val)}
    loss, stat = tr._compute_kp_loss(batch, {"rots": r_ray, "kp_batch": k_ray})
    sum(loss.values()).backward()
    d_rots = r_ray.grad.numpy()
    assert (d_rots[..., 2] == 0).all()
    p = f"{name}/"
    out[p + "rots"], out[p + "kps"], out[p + "anchor_rots"], out[p + "anchor_kps"] = rots, kps, a_rots, a_kps
    out[p + "kp_idx"], out[p + "temp_val"] = kp_idx.astype(np.int32), temp_val
    out[p + "d_rots01"] = np.ascontiguousarray(d_rots[..., :2])
    if k_ray.grad is not None:
        out[p + "d_kps"] = k_ray.grad.numpy()
    for k, v in (("tol", tol), ("coef", POSE_COEF), ("temp_coef", TEMP_COEF), ("ext_scale", EXT_SCALE), ("temporal", int(c["temporal"]))):
        out[p + k] = np.array(v)
    for k, v in loss.items():
        out[p + "ref_" + k] = np.array(v.item(), dtype=np.float64)
    out[p + "ref_MPJPC"] = np.array(stat["MPJPC"].item(), dtype=np.float64)


def norm_case(T, rng, out):
    m = torch.nn.Module()
    for i, shape in enumerate(NORM_SHAPES):
        prm = torch.nn.Parameter(torch.zeros(shape))
        prm.grad = torch.tensor(rng.normal(0, 10.0 ** (i - 2), shape).astype(np.float32))
        m.register_parameter(f"p{i}", prm)
        out[f"norms/g{i}"] = prm.grad.numpy()
    m.register_parameter("no_grad", torch.nn.Parameter(torch.zeros(5)))      # .grad is None: skipped, not counted
    total, avg = T.get_gradnorm(m)
    out["norms/ref_total_norm"], out["norms/ref_avg_norm"] = np.array(total), np.array(avg)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--ref", default="/root/reference")
    ap.add_argument("--out", default=os.path.join(REPO, "tests", "golden"))
    a = ap.parse_args()
    if not os.path.isfile(os.path.join(a.ref, "core", "trainer.py")):
        sys.exit(f"gen_golden_train_losses: {a.ref}/core/trainer.py not found -- the fixture is made from the reference's own Trainer; pass --ref")
    sys.path.insert(0, a.ref)
    import core.trainer as T
    out = {}
    for i, (name, c) in enumerate(PHOTO_CASES.items()):
        photo_case(T, name, c, np.random.RandomState(100 + i), out)
    for i, (name, c) in enumerate(KP_CASES.items()):
        kp_case(T, name, c, np.random.RandomState(200 + i), out)
    norm_case(T, np.random.RandomState(300), out)
    out["photo_cases"], out["kp_cases"] = np.array(list(PHOTO_CASES)), np.array(list(KP_CASES))
    path = os.path.join(a.out, "train_losses.npz")
    np.savez_compressed(path, **out)
    size = os.path.getsize(path)
    assert size < 200 * 1024, size
    print(f"{path}: {len(out)} arrays, {size} bytes")


if __name__ == "__main__":
    main()
