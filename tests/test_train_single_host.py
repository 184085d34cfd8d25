"""Single-net training without a GPU: the new fixtures (tools/gen_golden.py: train_grads_single, train_grads_single_v4,
train_grads_single_pose -- the reference's own single-net step up to loss.backward()), a restatement of that step from the
oracle's public pieces under torch autograd (the second yardstick of tests/test_gpu_train_single.py), pinned here to the
reference's gradients, and the Python seam that needs no device."""
import os

import numpy as np
import pytest
import torch

from oracle import anerf_oracle as orc
from posegen_amd import synthetic as syn
from posegen_amd.config import RenderConfig, surreal_config, surreal_single_config
from tests.helpers import (GOLDEN, default_dtype, golden_draws, load_golden, loss_of, oracle_cfg, single_cfg, single_model,  # noqa: F401
                           weights_digest)
from tools.gen_golden import grad_sample_index

FIXTURES = ["train_grads_single", "train_grads_single_v4", "train_grads_single_pose"]


def single_net_render(rb, skts, cyls, ocfg, w, S, N, draws=None):
    """One training-mode call of the reference's single-net caster (core/raycasters.py:446-469, ray_utils.py:255-289) from the
    oracle's pieces: the coarse pass, the is_only pdf 0.5 (max(w_l, w_k) + max(w_k, w_u)) + 0.01 sampled at u (detached), ONLY
    the N new points through the SAME weights `w`, the two raw tensors merged by the depth sort, the fine composite."""
    draws = draws or {}
    n = rb.shape[0]
    o, d = rb[:, 0:3], rb[:, 3:6]
    if cyls.shape[0] < n:
        cyls = cyls.expand(n, -1)
    near, far = orc.near_far_in_cylinder(o, d, cyls, rb[:, 6:7], rb[:, 7:8])
    z = orc.coarse_z(near, far, S, False, draws.get("t_rand"))
    rn = draws.get("ray_noise")
    pts = o[:, None, :] + d[:, None, :] * z[..., None]
    if rn is not None:
        pts = pts + rn[:, :S]
    raw_c = orc._run_mlp(orc.embed_points(pts, d, skts, ocfg), w, ocfg)
    out_c = orc.composite(raw_c, z, d, ocfg, draws.get("noise0"))
    wt = out_c["weights"]
    pw = 0.5 * (torch.maximum(wt[:, :-2], wt[:, 1:-1]) + torch.maximum(wt[:, 1:-1], wt[:, 2:])) + 0.01
    pw = pw + 1e-5                                                  # sample_pdf, ray_utils.py:159
    pdf = pw / torch.sum(pw, -1, keepdim=True)
    cdf = torch.cat([torch.zeros_like(pdf[:, :1]), torch.cumsum(pdf, -1)], -1).detach()
    mids = .5 * (z[:, 1:] + z[:, :-1])
    u = draws.get("u_rand")
    u = (torch.linspace(0., 1., steps=N).expand(n, N) if u is None else u).contiguous()
    hi = torch.searchsorted(cdf, u, right=True)
    lo = torch.clamp(hi - 1, min=0)
    hi = torch.clamp(hi, max=cdf.shape[-1] - 1)
    c_lo, c_hi = torch.gather(cdf, 1, lo), torch.gather(cdf, 1, hi)
    b_lo, b_hi = torch.gather(mids, 1, lo), torch.gather(mids, 1, hi)
    den = c_hi - c_lo
    den = torch.where(den < 1e-5, torch.ones_like(den), den)
    z_new = (b_lo + (u - c_lo) / den * (b_hi - b_lo)).detach()
    z_all, order = torch.sort(torch.cat([z, z_new], -1), dim=-1, stable=True)
    pts_n = o[:, None, :] + d[:, None, :] * z_new[..., None]
    if rn is not None:
        pts_n = pts_n + rn[:, S:]
    raw_n = orc._run_mlp(orc.embed_points(pts_n, d, skts, ocfg), w, ocfg)
    raw_m = torch.gather(torch.cat([raw_c, raw_n], 1), 1, order[..., None].expand(-1, -1, 4))
    out = orc.composite(raw_m, z_all, d, ocfg, draws.get("noise1"))
    return {"rgb_map": out["rgb_map"], "acc_map": out["acc_map"], "alpha": out["alpha"], "rgb0": out_c["rgb_map"],
            "acc0": out_c["acc_map"], "alpha0": out_c["alpha"], "n_new_rows": raw_n.shape[0] * raw_n.shape[1]}


def single_net_grads(cfg, w, tv, td, rb, skts, cyls, target, S, N, draws=None, dtype=torch.float64, loss_fn=loss_of, pose=False):
    """the restated step under autograd, everything in `dtype`: (loss, maps, {name: gradient as float64 numpy}, dL/dskts or None)"""
    cast = lambda x: torch.as_tensor(x).detach().cpu().to(dtype)
    with default_dtype(dtype):
        tw = {k: torch.tensor(np.asarray(v), dtype=dtype, requires_grad=True) for k, v in w.items()}
        sk = cast(skts).requires_grad_(pose)
        out = single_net_render(cast(rb), sk, cast(cyls), oracle_cfg(cfg, tv, td), tw, S, N,
                                {k: cast(v) for k, v in draws.items()} if draws else None)
        loss = loss_fn(out, cast(target))
        loss.backward()
    maps = {k: out[k].detach().double().numpy() for k in ("rgb_map", "acc_map", "rgb0", "acc0")}
    grads = {k: (p.grad.double().numpy() if p.grad is not None else np.zeros(p.shape)) for k, p in tw.items()}
    return float(loss.detach()), maps, grads, (sk.grad.double().numpy() if pose else None)


@pytest.mark.parametrize("name", FIXTURES)
def test_fixture_keys_and_size(name):
    path = os.path.join(GOLDEN, f"{name}.npz")
    assert os.path.getsize(path) < (1 << 20)
    g = load_golden(name)
    for k in ("single_net", "multires_views", "n_samples", "n_importance", "grad_sensitivity", "loss", "target", "t_rand", "u_rand",
              "noise0", "noise1", "rgb_map", "acc_map", "rgb0", "acc0", "seed_pose", "digest_coarse"):
        assert k in g, k
    assert int(g["single_net"]) == 1 and float(g["grad_sensitivity"]) <= 1e-5
    v0 = name != "train_grads_single_v4"
    assert int(g["multires_views"]) == (0 if v0 else 4)
    assert (int(g["n_samples"]), int(g["n_importance"])) == ((96, 48) if v0 else (64, 16))
    # the shared net's gradients are stored once, under "coarse"; the view weight has the reference's width
    assert sum(1 for k in g if k.startswith("gnorm_")) == 24 and not any(k.startswith("gnorm_fine_") for k in g)
    assert g["noise1"].shape[1] == int(g["n_samples"]) + int(g["n_importance"])
    if name.endswith("_pose"):
        assert g["dskts"].shape == (g["ray_batch"].shape[0], 24, 4, 4) and "kp_idx" in g
    print(f"[{name}] grad_sensitivity {float(g['grad_sensitivity']):.2e}, seed_pose {int(g['seed_pose'])}")


@pytest.mark.parametrize("name", ["train_grads_single", "train_grads_single_v4"])
def test_restated_single_net_step_is_the_reference_step(name):
    """The restatement in float32 against the reference's own autograd: maps 2e-5, loss 1e-5, every gradient tensor within 1e-4
    of its scale (the bounds tests/test_gpu_train.py holds the HIP step to on the same kind of fixture)."""
    g = load_golden(name)
    cfg = single_cfg(g)
    w, tv, td = single_model(cfg, g)
    loss, maps, grads, _ = single_net_grads(cfg, w, float(g["tau_v"]), float(g["tau_d"]), g["ray_batch"], g["skts"], g["cyl"], g["target"],
                                            cfg.n_samples, cfg.n_importance, golden_draws(g), dtype=torch.float32)
    for k, v in maps.items():
        assert float(np.abs(v - g[k]).max()) <= 2e-5, k
    assert abs(loss - float(g["loss"])) <= 1e-5 * max(1.0, abs(float(g["loss"])))
    worst = 0.0
    for k, got in grads.items():
        ref_vals, ref_norm = g[f"gval_coarse_{k}"], float(g[f"gnorm_coarse_{k}"])
        got = got.reshape(-1)
        scale = max(float(np.abs(ref_vals).max()), ref_norm / np.sqrt(got.size), 1e-12)
        err = float(np.abs(got[grad_sample_index(got.size)] - ref_vals).max()) / scale
        nerr = abs(float(np.linalg.norm(got)) - ref_norm) / max(ref_norm, 1e-12)
        worst = max(worst, err, nerr)
        assert err <= 1e-4 and nerr <= 1e-4, (k, err, nerr)
    assert tuple(grads["views_linears.0.weight"].shape) == (128, 256 + (72 if cfg.multires_views == 0 else 648))
    print(f"[{name}] restatement vs the reference: worst relative gradient deviation {worst:.2e}")


def test_restated_pose_gradient_is_the_reference_pose_gradient():
    from tests.test_pose_grad_host import scale_of
    g = load_golden("train_grads_single_pose")
    cfg = single_cfg(g)
    w, tv, td = single_model(cfg, g)
    idx = g["kp_idx"]
    loss, _, _, dsk = single_net_grads(cfg, w, float(g["tau_v"]), float(g["tau_d"]), g["ray_batch"], g["skts"][idx], g["cyl"][idx],
                                       g["target"], cfg.n_samples, cfg.n_importance, golden_draws(g), dtype=torch.float32, pose=True)
    assert abs(loss - float(g["loss"])) <= 1e-5 * max(1.0, abs(float(g["loss"])))
    assert float(np.abs(dsk - g["dskts"]).max()) <= 1e-4 * scale_of(g["dskts"])


def test_the_seam_without_a_device():
    import posegen_amd
    from posegen_amd import train
    assert posegen_amd.make_trainable is train.make_trainable
    assert posegen_amd.SingleNetTrainableRayCaster is train.SingleNetTrainableRayCaster
    assert issubclass(train.SingleNetTrainableRayCaster, train.TrainableRayCaster)
    with pytest.raises(ValueError):
        train.SingleNetTrainableRayCaster._check_model(surreal_config())
    train.SingleNetTrainableRayCaster._check_model(surreal_single_config())
    train.SingleNetTrainableRayCaster._check_model(surreal_config(single_net=True))
    for cfg in (surreal_single_config(), surreal_config(multires_views=0)):
        with pytest.raises(NotImplementedError):
            train.TrainableRayCaster._check_model(cfg)
    train.TrainableRayCaster._check_model(surreal_config())
