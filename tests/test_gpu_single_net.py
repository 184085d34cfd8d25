"""Single-net A-NeRF models on the GPU (single_net, multires_views = 0; configs/surreal/surreal_single.txt): the render
path against the reference's own vectors (tools/gen_golden.py: rays_single, rays_single_v4, rays_views0,
rays_single_train), its intermediates, the evaluation count, the frame / multi-device routes and the refusals.

The bounds are test_gpu_parity's: fp32 / fp16c / bf16x3 within 1e-4 of the reference on rgb / acc (and rgb0 / acc0),
fp16 1e-3, bf16 5e-3, alpha at its 99th percentile.  PG_PREC_FP16M has no guide pass under single_net: it is fp16c."""
import numpy as np
import pytest
import torch

from posegen_amd import (PREC_BF16, PREC_BF16X3, PREC_FP16, PREC_FP16C, PREC_FP16M, PREC_FP32, PREC_NAMES, _ffi,
                         synthetic as syn)
from posegen_amd.config import RenderConfig, surreal_single_config
from tests.helpers import golden_draws, load_golden, weights_digest

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
BOUND = {PREC_FP32: (1e-4, 1e-4, 2e-4), PREC_BF16X3: (1e-4, 1e-4, 5e-4), PREC_FP16C: (1e-4, 1e-4, 5e-4),
         PREC_FP16: (1e-3, 1e-3, 5e-3), PREC_BF16: (5e-3, 5e-3, 3e-2)}
CASES = ["rays_single", "rays_single_v4", "rays_views0"]


def _cfg(g) -> RenderConfig:
    """the fixture's model, from its own keys"""
    return RenderConfig(n_samples=int(g["n_samples"]), n_importance=int(g["n_importance"]),
                        single_net=bool(int(g["single_net"])), multires_views=int(g["multires_views"]))


def _model(cfg, g):
    wc, wf, tv, td = syn.make_model(cfg, int(g["seed_model"]))
    assert weights_digest(wc) == str(g["digest_coarse"]), "synthetic weight recipe drifted"
    return wc, (None if cfg.single_net else wf), tv, td


@pytest.fixture(scope="module")
def casters():
    from posegen_amd.raycaster import HipRayCaster
    cache = {}

    def get(name, prec):
        g = load_golden(name)
        cfg = _cfg(g)
        key = (cfg.single_net, cfg.multires_views, int(g["seed_model"]))
        if key not in cache:
            cache[key] = HipRayCaster.from_weights(cfg, *_model(cfg, g), device=DEV, precision=prec)
        c = cache[key]
        c.renderer.set_precision(prec)
        return c, g, cfg
    yield get
    for c in cache.values():
        c.renderer.close()


def _call(c, g, cfg, **kw):
    rb, skts, cyl = torch.tensor(g["ray_batch"]), torch.tensor(g["skts"]), torch.tensor(g["cyl"])
    n = rb.shape[0]
    return c(rb, N_samples=cfg.n_samples, kp_batch=torch.tensor(g["kps"]).expand(n, -1, -1),
             skts=skts.expand(n, -1, -1, -1), cyls=cyl.expand(n, -1), bones=torch.tensor(g["bones"]).expand(n, -1, -1),
             cams=None, N_importance=cfg.n_importance, lindisp=False, ext_scale=0.001, preproc_kwargs={},
             nerf_type="nerf", use_viewdirs=True, **kw)


def _maxdiff(a, b):
    return float(np.nanmax(np.abs(np.asarray(a, dtype=np.float64) - np.asarray(b, dtype=np.float64))))


def _errors(out, g):
    errs = {k: _maxdiff(out[k].cpu().numpy(), g[k]) for k in ("rgb_map", "acc_map", "rgb0", "acc0", "disp_map")}
    errs["alpha"] = float(np.quantile(np.abs(out["alpha"].cpu().numpy().astype(np.float64) - g["alpha"]), 0.99))
    return errs


@pytest.mark.parametrize("name", CASES)
@pytest.mark.parametrize("prec", [PREC_FP32, PREC_FP16C, PREC_BF16X3, PREC_FP16, PREC_BF16])
def test_single_net_vs_reference_golden(casters, name, prec):
    c, g, cfg = casters(name, prec)
    out = _call(c, g, cfg, perturb=False, raw_noise_std=0., ray_noise_std=0.)
    n, S, N = g["ray_batch"].shape[0], cfg.n_samples, cfg.n_importance
    assert set(out) == {"rgb_map", "disp_map", "acc_map", "alpha", "rgb0", "disp0", "acc0", "alpha0"}
    assert out["alpha"].shape == (n, S + N) and out["alpha0"].shape == (n, S)
    errs = _errors(out, g)
    print(f"[{name} {PREC_NAMES[prec]}] " + " ".join(f"{k}={v:.2e}" for k, v in errs.items()))
    b_rgb, b_disp, b_alpha = BOUND[prec]
    for k in ("rgb_map", "acc_map", "rgb0", "acc0"):
        assert errs[k] <= b_rgb, (k, errs[k])
    assert errs["disp_map"] <= b_disp
    assert errs["alpha"] <= b_alpha


@pytest.mark.parametrize("name", CASES)
def test_mixed_mode(casters, name):
    """fp16m within fp16c's bound; with single_net no pass is a guide pass, so it IS fp16c, bitwise."""
    c, g, cfg = casters(name, PREC_FP16M)
    out = _call(c, g, cfg)
    errs = _errors(out, g)
    print(f"[{name} fp16m] " + " ".join(f"{k}={v:.2e}" for k, v in errs.items()))
    if cfg.single_net:
        for k in ("rgb_map", "acc_map", "rgb0", "acc0"):
            assert errs[k] <= BOUND[PREC_FP16C][0], (k, errs[k])
        c.renderer.set_precision(PREC_FP16C)
        ref = _call(c, g, cfg)
        for k in out:
            assert torch.equal(out[k], ref[k]), k
    else:       # two nets: the documented fp16m bound (test_gpu_parity.test_mixed_mode_bounds_and_pass_selection)
        for k in ("rgb_map", "acc_map"):
            assert errs[k] <= 2e-4, (k, errs[k])


@pytest.mark.parametrize("name", CASES)
def test_intermediates_match_the_reference(casters, name):
    """z_coarse, raw_coarse, weights0, z_fine (the is_only samples merged by depth) and raw_fine (the coarse and the new
    raw merged by sorted_idxs) against the reference's stage-wise values."""
    c, g, cfg = casters(name, PREC_FP32)
    r = c.renderer
    r.set_chunk(4096)
    out = r.render_rays(torch.tensor(g["ray_batch"]), torch.tensor(g["skts"]), torch.tensor(g["cyl"]),
                        n_samples=cfg.n_samples, n_importance=cfg.n_importance, extras=True)
    ex = {k: v.cpu().numpy() for k, v in out["extras"].items()}
    np.testing.assert_allclose(ex["z_coarse"], g["z_coarse"], rtol=2e-6, atol=1e-6)
    assert _maxdiff(ex["raw_coarse"], g["raw_coarse"]) <= 1e-4 * max(1.0, float(np.abs(g["raw_coarse"]).max()))
    assert _maxdiff(ex["weights0"], g["weights0"]) <= 1e-4
    # importance depths: a sample in a weightless bin may move by up to a bin (the cdf is flat there); < 1 % of them
    dz = np.abs(ex["z_fine"] - g["z_fine"])
    assert np.quantile(dz, 0.99) <= 1e-4, float(np.quantile(dz, 0.99))
    dr = np.abs(ex["raw_fine"] - g["raw_fine"]).max(-1)
    assert np.quantile(dr, 0.99) <= 1e-3, float(np.quantile(dr, 0.99))
    # the merge itself: every coarse raw appears in raw_fine at the depth it belongs to
    if cfg.single_net:
        S = cfg.n_samples
        for ray in range(0, ex["z_fine"].shape[0], 7):
            idx = np.searchsorted(ex["z_fine"][ray], ex["z_coarse"][ray])
            assert np.array_equal(ex["raw_fine"][ray][idx], ex["raw_coarse"][ray][:S])


@pytest.mark.parametrize("prec", [PREC_FP32, PREC_FP16C, PREC_BF16X3, PREC_FP16, PREC_BF16])
def test_training_mode_forward_vs_reference_golden(prec):
    """rays_single_train: the rays_train recipe (perturb, raw noise, ray noise; pytest=True draws) on the single-net
    model.  noise1 applies to the merged raw; the new points' position noise is rows S.. of ray_noise in z_samples order."""
    from posegen_amd.raycaster import HipRayCaster
    g = load_golden("rays_single_train")
    cfg = _cfg(g)
    c = HipRayCaster.from_weights(cfg, *_model(cfg, g), device=DEV, precision=prec)
    try:
        c.train()
        out = _call(c, g, cfg, perturb=float(g["perturb"]), raw_noise_std=float(g["raw_noise_std"]),
                    ray_noise_std=float(g["ray_noise_std"]), pytest=True, draws=golden_draws(g))
    finally:
        c.renderer.close()
    errs = _errors(out, g)
    print(f"[rays_single_train {PREC_NAMES[prec]}] " + " ".join(f"{k}={v:.2e}" for k, v in errs.items()))
    b_rgb, b_disp, b_alpha = BOUND[prec]
    for k in ("rgb_map", "acc_map", "rgb0", "acc0"):
        assert errs[k] <= b_rgb, (k, errs[k])
    assert errs["disp_map"] <= b_disp
    assert errs["alpha"] <= b_alpha


@pytest.mark.parametrize("prec", [PREC_FP32, PREC_BF16, PREC_FP16C])
def test_one_render_evaluates_s_plus_n_points_per_ray(casters, prec):
    c, g, cfg = casters("rays_single", prec)
    r = c.renderer
    n, S, N = g["ray_batch"].shape[0], cfg.n_samples, cfg.n_importance
    r.profile_enable(True)
    try:
        r.profile_read()
        r.render_rays(torch.tensor(g["ray_batch"]), torch.tensor(g["skts"]), torch.tensor(g["cyl"]), n_samples=S, n_importance=N)
        launches, ms, pts = r.profile_read()
    finally:
        r.profile_enable(False)
    assert launches == 2
    assert pts == n * (S + N) and pts != n * (2 * S + N)


def _frame_inputs(H):
    _, kps, skts = syn.make_pose(1, 21)
    c2ws, focals = syn.make_camera(1, H, H)
    return kps, skts, c2ws, focals


def test_render_frame_equals_the_ray_level_path():
    """pg_render_frame (rays made, rendered and scattered on the device) of a small single-net frame against
    kp_to_valid_rays on the host + render_rays over the same rays + the scatter."""
    from posegen_amd.rays import kp_to_valid_rays
    from posegen_amd.raycaster import HipRayCaster
    cfg = surreal_single_config()
    c = HipRayCaster.from_weights(cfg, syn.make_weights(cfg, 0), None, 79.6, 79.6, device=DEV, precision=PREC_FP32)
    try:
        H = W = 48
        kps, skts, c2ws, focals = _frame_inputs(H)
        r = c.renderer
        r.set_chunk(cfg.chunk)
        rays, vids, cyls, boxes = kp_to_valid_rays(torch.tensor(c2ws), H, W, focals, kps=torch.tensor(kps),
                                                   ext_scale=cfg.ext_scale)
        ro, rd = rays[0]
        n = ro.shape[0]
        vd = rd / torch.norm(rd, dim=-1, keepdim=True)
        rb = torch.cat([ro, rd, torch.zeros(n, 1), torch.ones(n, 1), vd], -1).float()
        ret = r.render_rays(rb, torch.tensor(skts), cyls[:1], n_samples=cfg.n_samples, n_importance=cfg.n_importance,
                            want_alpha=False)
        ref_rgb = torch.ones(H * W, 3, device=DEV)
        vid = vids[0].to(DEV)
        ref_rgb[vid] = ret["rgb_map"] + (1. - ret["acc_map"][..., None]) * ref_rgb[vid]
        rgb, disp, acc = r.render_frame(H, W, focals[0], torch.tensor(c2ws[0]), boxes[0], torch.tensor(skts), cyls[:1],
                                        base_bg=1.0)
        e = float((rgb.view(-1, 3) - ref_rgb).abs().max())
        print(f"single-net frame vs ray-level route: max |d rgb| {e:.2e}, bitwise {bool(torch.equal(rgb.view(-1, 3), ref_rgb))}")
        assert n > 200 and e <= 2e-6        # (the bound of test_gpu_frames.test_render_frame_equals_ray_level_path)
        assert torch.isfinite(disp).all() and float(acc.max()) > 0.5
    finally:
        c.renderer.close()


def test_two_workers_on_one_device_are_bitwise_one_device():
    from posegen_amd.raycaster import HipRayCaster
    from posegen_amd.render import render_path
    cfg = surreal_single_config()
    w = syn.make_weights(cfg, 0)
    H = W = 64
    _, kps, skts = syn.make_pose(3, 22)
    c2ws, focals = syn.make_camera(3, H, W)
    kw = dict(kp=torch.tensor(kps), skts=torch.tensor(skts), white_bkgd=True, ret_acc=True, ext_scale=cfg.ext_scale)
    outs = []
    for devs in (None, [0, 0]):
        c = HipRayCaster.from_weights(cfg, w, None, 79.6, 79.6, device=DEV, precision="bf16", devices=devs)
        rk = {"ray_caster": c, "N_samples": cfg.n_samples, "N_importance": cfg.n_importance}
        outs.append(render_path(torch.tensor(c2ws), (H, W, focals), 512, rk, **kw))
        c.renderer.close()
    one, two = outs
    for a, b in zip(one[:3], two[:3]):
        assert a.shape == b.shape and np.array_equal(a, b)
    assert float(np.asarray(one[2]).max()) > 0.5


def test_device_side_weight_load_widens_like_the_host_load():
    """pg_load_weights_device takes the reference's [128, 328] view weight and widens it on the device: the render
    equals the host-loaded one bitwise."""
    from posegen_amd.raycaster import NET_TENSOR_ORDER, HipRayCaster
    cfg = surreal_single_config()
    w0, w1 = syn.make_weights(cfg, 0), syn.make_weights(cfg, 4)
    rb = torch.tensor(load_golden("rays_single")["ray_batch"])
    g = load_golden("rays_single")
    res = []
    for prec in ("bf16", "fp16c"):
        a = HipRayCaster.from_weights(cfg, w1, None, 79.6, 79.6, device=DEV, precision=prec)
        b = HipRayCaster.from_weights(cfg, w0, None, 79.6, 79.6, device=DEV, precision=prec)
        try:
            b.renderer.load_network_device(0, [torch.tensor(w1[k]).to(DEV).contiguous() for k in NET_TENSOR_ORDER])
            outs = [x.renderer.render_rays(rb, torch.tensor(g["skts"]), torch.tensor(g["cyl"]), n_samples=96, n_importance=48)
                    for x in (a, b)]
            for k in outs[0]:
                assert torch.equal(outs[0][k], outs[1][k]), (prec, k)
            res.append(outs[0]["rgb_map"])
        finally:
            a.renderer.close()
            b.renderer.close()
    assert _maxdiff(res[0].cpu().numpy(), res[1].cpu().numpy()) > 0      # the two precisions really ran


def test_refusals():
    from posegen_amd.raycaster import HipRayCaster
    from posegen_amd.train import TrainableRayCaster
    cfg = surreal_single_config()
    wc, wf, tv, td = syn.make_model(cfg, 0)
    c = HipRayCaster(cfg, device=DEV, precision="fp32")
    try:
        emb = {"cutoff_dist": torch.full((24,), cfg.cutoff_dist), "tau": torch.tensor(tv)}
        ck = {"network_fn_state_dict": wc, "network_fine_state_dict": wf, "embed_state_dict": emb, "embeddirs_state_dict": emb}
        with pytest.raises(ValueError):
            c.load_state_dict(ck)
        with pytest.raises(ValueError):
            HipRayCaster.from_weights(cfg, wc, wf, tv, td, device=DEV, precision="fp32")
        ck["network_fine_state_dict"] = {k: v.copy() for k, v in wc.items()}
        c.load_state_dict(ck)                              # the reference's own layout: both keys, one net
        sd = c.state_dict()
        assert sd["network_fine_state_dict"] is sd["network_fn_state_dict"] or all(
            torch.equal(sd["network_fine_state_dict"][k], sd["network_fn_state_dict"][k]) for k in sd["network_fn_state_dict"])
        assert tuple(sd["network_fn_state_dict"]["views_linears.0.weight"].shape) == (128, 256 + 72)
        pts = torch.zeros(8, 3)
        skts = torch.tensor(syn.make_pose(1, 1)[2])
        d0 = c.renderer.query_density(pts, skts)
        assert torch.equal(d0, c.renderer.query_density(pts, skts, which=0))
        with pytest.raises(_ffi.PgError):
            c.renderer.query_density(pts, skts, which=1)
        with pytest.raises(NotImplementedError):
            TrainableRayCaster(c)
    finally:
        c.renderer.close()
    c4 = HipRayCaster.from_weights(RenderConfig(multires_views=0), *syn.make_model(RenderConfig(multires_views=0), 0),
                                   device=DEV, precision="fp32")
    try:
        with pytest.raises(NotImplementedError):
            TrainableRayCaster(c4)
    finally:
        c4.renderer.close()
