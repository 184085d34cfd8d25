#!/usr/bin/env python3
"""Capture golden vectors from the REAL reference implementation.

Runs only where the read-only reference checkout exists (the build container);
the GPU box never sees the reference.  The reference is imported in-process
with stub modules for its unused third-party imports and a 'cuda'->'cpu'
device shim (the reference hard-codes .to('cuda')); nothing of the reference is
written into this repository -- only inputs (seeds / small tensors) and the
numeric outputs, as .npz fixtures under tests/golden/.

Usage:  python tools/gen_golden.py [--ref /root/reference] [--out tests/golden]
"""
from __future__ import annotations

import argparse
import os
import sys
import tempfile
import types
from argparse import Namespace

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.dont_write_bytecode = True


class _StubModule(types.ModuleType):
    """Placeholder for third-party modules the reference imports but the render
    path never calls (cv2, pytorch3d, h5py, ...): any attribute is a dummy."""

    def __getattr__(self, item):
        if item.startswith("__"):
            raise AttributeError(item)
        return _StubModule(f"{self.__name__}.{item}")

    def __call__(self, *a, **k):
        raise RuntimeError(f"stubbed module attribute {self.__name__} was called")


def _install_shims(ref_root: str):
    import torch
    import torch.nn as nn

    if not os.path.isdir(os.path.join(ref_root, "core")):
        sys.exit(f"gen_golden: reference checkout not found at {ref_root}; "
                 "fixtures can only be regenerated in the build container")
    for p in (ref_root, os.path.join(ref_root, "smplx"), os.path.join(ref_root, "pytorch-msssim")):
        sys.path.insert(0, p)
    for name in ("cv2", "pytorch3d", "pytorch3d.transforms",
                 "pytorch3d.transforms.rotation_conversions", "h5py", "imageio",
                 "configargparse", "tensorboard", "tensorboard.backend",
                 "tensorboard.backend.event_processing",
                 "tensorboard.backend.event_processing.event_accumulator",
                 "torch.utils.tensorboard", "deepdish", "skimage", "skimage.transform",
                 "skimage.metrics", "lpips"):
        if name not in sys.modules:
            try:
                __import__(name)
            except Exception:
                m = _StubModule(name)
                m.__path__ = []          # behave like a package
                sys.modules[name] = m
    sys.modules["torch.utils.tensorboard"].SummaryWriter = object
    sys.modules["tensorboard.backend.event_processing.event_accumulator"].EventAccumulator = object

    def _cpu_dev(a):
        if isinstance(a, str) and a.startswith("cuda"):
            return "cpu"
        if isinstance(a, torch.device) and a.type == "cuda":
            return torch.device("cpu")
        return a

    t_to = torch.Tensor.to
    m_to = nn.Module.to

    def tensor_to(self, *args, **kw):
        args = tuple(_cpu_dev(a) for a in args)
        kw = {k: _cpu_dev(v) for k, v in kw.items()}
        return t_to(self, *args, **kw)

    def module_to(self, *args, **kw):
        args = tuple(_cpu_dev(a) for a in args)
        kw = {k: _cpu_dev(v) for k, v in kw.items()}
        return m_to(self, *args, **kw)

    torch.Tensor.to = tensor_to
    nn.Module.to = module_to


def _nerf_args(cfg, workdir) -> Namespace:
    """argparse.Namespace with the renderer-relevant flag values."""
    return Namespace(
        n_framecodes=cfg.n_framecodes if cfg.framecode_ch else None,
        use_cutoff=True, normalize_cutoff=False, cutoff_mm=cfg.cutoff_mm,
        ext_scale=cfg.ext_scale, cutoff_inputs=True, opt_cutoff=False, freq_schedule=False,
        init_freq=0., cut_to_dist=False, cutoff_shift=False, multires=cfg.multires, i_embed=0,
        cutoff_bones=False, multires_bones=cfg.multires_bones, use_viewdirs=True,
        cutoff_viewdir=True, multires_views=cfg.multires_views, N_importance=cfg.n_importance,
        netdepth=cfg.net_depth, netwidth=cfg.net_width, opt_framecode=cfg.framecode_ch > 0,
        framecode_size=cfg.framecode_ch if cfg.framecode_ch else 16, density_scale=cfg.density_scale,
        single_net=bool(cfg.single_net), lrate=5e-4, basedir=workdir, expname="golden", ft_path=None,
        no_reload=True, finetune=False, perturb=0., N_samples=cfg.n_samples, raw_noise_std=0.,
        ray_noise_std=0., lindisp=False, nerf_type="nerf", debug=False, density_type=cfg.density_type,
        softplus_shift=cfg.softplus_shift, pts_tr_type="local", kp_dist_type="reldist", view_type="relray",
        bone_type="reldir", fix_layer=0, weight_decay=None, chunk=cfg.chunk)


def _build_reference_caster(cfg, seed, workdir):
    import torch
    from core.raycasters import create_raycaster
    from core.utils.skeleton_utils import SMPLSkeleton, get_per_joint_coords
    from posegen_amd import synthetic as syn
    from posegen_amd.skeleton import smpl_rest_pose, SURREAL_REST_SCALE

    os.makedirs(os.path.join(workdir, "golden"), exist_ok=True)
    rest = smpl_rest_pose * SURREAL_REST_SCALE
    attrs = {"skel_type": SMPLSkeleton, "near": 0., "far": 1.,
             "n_views": max(cfg.n_framecodes, 1),
             "joint_coords": get_per_joint_coords(rest)[None]}
    _, kw_test, *_ = create_raycaster(_nerf_args(cfg, workdir), attrs)
    caster = kw_test["ray_caster"]
    wc, wf, tau_v, tau_d = syn.make_model(cfg, seed)
    if cfg.single_net:              # network_fine is network: loading wf would overwrite the coarse weights
        assert caster.network_fine is None or caster.network_fine is caster.network
        wf = wc
    sd = {"network_fn_state_dict": {k: torch.tensor(v) for k, v in wc.items()},
          "network_fine_state_dict": {k: torch.tensor(v) for k, v in wf.items()}}
    caster.network.load_state_dict(sd["network_fn_state_dict"])
    if caster.network_fine is not None and not cfg.single_net:
        caster.network_fine.load_state_dict(sd["network_fine_state_dict"])
    caster.embed_fn.tau = torch.tensor(tau_v)
    caster.embeddirs_fn.tau = torch.tensor(tau_d)
    caster.eval()
    return caster, kw_test, (wc, wf, tau_v, tau_d)


def _weights_digest(w):
    import hashlib
    h = hashlib.sha256()
    for k in sorted(w):
        h.update(k.encode())
        h.update(np.ascontiguousarray(w[k]).tobytes())
    return h.hexdigest()


def gen_kinematics(out):
    """a-18: bones -> l2ws / kps / skts via the reference's get_smpl_l2ws."""
    from core.utils.skeleton_utils import get_smpl_l2ws
    from posegen_amd import synthetic as syn
    from posegen_amd.skeleton import smpl_rest_pose, SURREAL_REST_SCALE
    rest = smpl_rest_pose * SURREAL_REST_SCALE
    bones = syn.make_bones(4, seed=7)
    bones[3, 5] = 0.0                               # exercise the small-angle branch
    bones[3, 6] = 1e-5
    l2ws = np.array([get_smpl_l2ws(b, rest, 1.0) for b in bones])
    np.savez_compressed(os.path.join(out, "kinematics.npz"), bones=bones, rest_pose=rest,
                        l2ws=l2ws, kps=l2ws[..., :3, -1], skts=np.linalg.inv(l2ws))


def gen_valid_rays(out):
    """a-2: cylinder, box, pixel ids and rays of the bbox cull."""
    import torch
    from core.utils.ray_utils import kp_to_valid_rays
    from posegen_amd import synthetic as syn
    H = W = 96
    _, kps, _ = syn.make_pose(3, seed=11)
    c2ws, focals = syn.make_camera(3, H, W)
    rays, vids, cyls, boxes = kp_to_valid_rays(torch.tensor(c2ws), H, W, focals,
                                               kps=torch.tensor(kps), ext_scale=0.001)
    d = {"H": H, "W": W, "kps": kps, "c2ws": c2ws, "focals": focals,
         "cyls": cyls.numpy(), "boxes": np.array([[b[0], b[1]] for b in boxes])}
    for i, (r, v) in enumerate(zip(rays, vids)):
        d[f"n_valid_{i}"] = len(v)
        d[f"vid_head_{i}"] = v[:8].numpy()
        d[f"vid_tail_{i}"] = v[-8:].numpy()
        d[f"rays_o_head_{i}"] = r[0][:8].numpy()
        d[f"rays_d_head_{i}"] = r[1][:8].numpy()
        d[f"rays_d_tail_{i}"] = r[1][-8:].numpy()
    np.savez_compressed(os.path.join(out, "valid_rays.npz"), **d)


def _stagewise(caster, kw, batch, kp_b, skt_b, cyl_b, bones_b, cams_b, n_samples, n_importance):
    """Run the reference's own stage functions in render_rays order and keep
    every intermediate (raycasters.py:413-474)."""
    import torch
    from core.utils.ray_utils import get_near_far_in_cylinder
    pk = kw["preproc_kwargs"]
    n = batch.shape[0]
    o, d = batch[:, 0:3], batch[:, 3:6]
    bounds = torch.reshape(batch[..., 6:8], [-1, 1, 2])
    near, far = bounds[..., 0], bounds[..., 1]
    near, far = get_near_far_in_cylinder(o, d, cyl_b, near=near, far=far)
    pts, z = caster.sample_pts(o, d, near, far, n, n_samples, 0., False)
    jc = caster.get_subject_joint_coords(None, pts.device)
    enc = caster.encode_inputs(pts, [o[:, None, :], d[:, None, :]], kp_b, skt_b, bones_b,
                               cam_idxs=cams_b, subject_idxs=None, joint_coords=jc,
                               network=caster.network, **pk)
    x = torch.cat([enc["v"], enc["r"], enc["d"]], -1).clone()
    raw = caster.run_network(enc, caster.network)
    rd = caster.network.raw2outputs(raw, z, d, 0., B=pk["density_scale"], act_fn=pk["density_fn"])
    res = {"near": near, "far": far, "z_coarse": z, "x_coarse": x, "raw_coarse": raw,
           "weights_coarse": rd["weights"], "alpha0": rd["alpha"], "rgb0": rd["rgb_map"],
           "disp0": rd["disp_map"], "acc0": rd["acc_map"]}
    if n_importance > 0:
        pts_is, z_all, z_new, order = caster.sample_pts_is(o, d, z, rd["weights"], n_importance,
                                                           det=True, is_only=caster.single_net)
        enc_is = caster.encode_inputs(pts_is, [o[:, None, :], d[:, None, :]], kp_b, skt_b, bones_b,
                                      cam_idxs=cams_b, subject_idxs=None, joint_coords=jc,
                                      network=caster.network_fine, **pk)
        if caster.single_net:       # raycasters.py:462-469: only the new points through the one net, raw merged by depth
            raw_is = caster.run_network(enc_is, caster.network_fine)
            caster._merge_encodings(enc, enc_is, order, n, n_samples + n_importance)
            raw_f = caster._merge_encodings({"raw": raw}, {"raw": raw_is}, order, n,
                                            n_samples + n_importance)["raw"]
        else:
            merged = caster._merge_encodings(enc, enc_is, order, n, n_samples + n_importance)
            raw_f = caster.run_network(merged, caster.network_fine)
        rf = caster.network_fine.raw2outputs(raw_f, z_all, d, 0., B=pk["density_scale"],
                                             act_fn=pk["density_fn"])
        res.update({"z_fine": z_all, "z_new": z_new, "order": order, "raw_fine": raw_f,
                    "alpha": rf["alpha"], "rgb_map": rf["rgb_map"], "disp_map": rf["disp_map"],
                    "acc_map": rf["acc_map"], "weights_fine": rf["weights"]})
    else:
        res.update({"alpha": rd["alpha"], "rgb_map": rd["rgb_map"], "disp_map": rd["disp_map"],
                    "acc_map": rd["acc_map"]})
    return res


def _model_keys(d, cfg):
    """the keys of the single-net / multires_views = 0 fixtures (the older fixtures are two-net, 4 bands)"""
    d["single_net"] = int(cfg.single_net)
    d["multires_views"] = int(cfg.multires_views)


def gen_render_rays(out, name, cfg, *, n_rays, H, all_hit, seed_model=0, seed_pose=1,
                    use_cams=False, keep_x=16, model_keys=False):
    """a-5..a-16: one `RayCaster.__call__` on a strided subset of a culled frame."""
    import torch
    from core.utils.ray_utils import kp_to_valid_rays
    from posegen_amd import synthetic as syn
    with tempfile.TemporaryDirectory() as wd:
        caster, kw, (wc, wf, tau_v, tau_d) = _build_reference_caster(cfg, seed_model, wd)
    W = H
    bones, kps, skts = syn.make_pose(1, seed_pose)
    c2ws, focals = syn.make_camera(1, H, W)
    rays, vids, cyls, boxes = kp_to_valid_rays(torch.tensor(c2ws), H, W, focals,
                                               kps=torch.tensor(kps), ext_scale=cfg.ext_scale)
    ro, rd = rays[0]
    sel = np.unique(np.linspace(0, ro.shape[0] - 1, n_rays).round().astype(np.int64))
    ro, rd = ro[sel].float(), rd[sel].float()
    n = ro.shape[0]
    if all_hit:
        cyls = cyls.clone()
        cyls[:, 2] = 2.5
    vd = rd / torch.norm(rd, dim=-1, keepdim=True)
    ones = torch.ones(n, 1)
    batch = torch.cat([ro, rd, 0. * ones, 1. * ones, vd], -1)
    kp_b = torch.tensor(kps).expand(n, -1, -1)
    skt_b = torch.tensor(skts).expand(n, -1, -1, -1)
    cyl_b = cyls.expand(n, -1)
    bones_b = torch.tensor(bones).expand(n, -1, -1)
    cams_b = None
    cams_np = None
    if use_cams:
        cams_np = (np.arange(n) % cfg.n_framecodes).astype(np.float32)
        cams_np[: n // 4] = 3.0
        cams_b = torch.tensor(cams_np)
    with torch.no_grad():
        st = _stagewise(caster, kw, batch, kp_b, skt_b, cyl_b, bones_b, cams_b,
                        cfg.n_samples, cfg.n_importance)
        call_kw = {k: v for k, v in kw.items() if k != "ray_caster"}
        call_kw.pop("use_viewdirs", None)
        full = caster(batch, kp_batch=kp_b, skts=skt_b, cyls=cyl_b, bones=bones_b, cams=cams_b,
                      subject_idxs=None, **call_kw)
    for k in ("rgb_map", "disp_map", "acc_map", "alpha"):
        assert torch.equal(full[k], st[k]) or torch.allclose(full[k], st[k], atol=0, rtol=0, equal_nan=True), k
    # the 1080(+1)-vector is kept for a few points only (fixture size)
    pick_r = np.unique(np.linspace(0, n - 1, keep_x).round().astype(np.int64))
    pick_s = np.array([0, cfg.n_samples // 3, cfg.n_samples // 2, cfg.n_samples - 1])
    x_pick = st["x_coarse"][pick_r][:, pick_s].numpy()
    d = {"ray_batch": batch.numpy(), "kps": kps, "skts": skts, "bones": bones, "cyl": cyls.numpy(),
         "tau_v": tau_v, "tau_d": tau_d, "seed_model": seed_model, "n_samples": cfg.n_samples,
         "n_importance": cfg.n_importance, "framecode_ch": cfg.framecode_ch,
         "n_framecodes": cfg.n_framecodes, "digest_coarse": _weights_digest(wc),
         "digest_fine": _weights_digest(wf), "x_pick": x_pick, "x_pick_rays": pick_r,
         "x_pick_samples": pick_s}
    if cfg.density_type != "relu":
        d["density_softplus"] = int(cfg.density_type == "softplus")
        d["softplus_shift"] = float(cfg.softplus_shift)
    if cams_np is not None:
        d["cams"] = cams_np
    for k, v in st.items():
        if k == "x_coarse":
            continue
        d[k] = v.numpy()
    d["n_rays"] = n
    if model_keys:
        _model_keys(d, cfg)
        d["weights0"] = d["weights_coarse"]
    np.savez_compressed(os.path.join(out, f"{name}.npz"), **d)
    acc = st["acc_map"].numpy()
    print(f"[{name}] rays={n} acc in [{acc.min():.3f},{acc.max():.3f}] "
          f"mid-fraction={(np.logical_and(acc > 0.05, acc < 0.95)).mean():.2f}")


def gen_render_rays_train(out, name, cfg, *, n_rays, H, seed_model=0, seed_pose=1, perturb=1.,
                          raw_noise_std=1., ray_noise_std=0.005, model_keys=False):
    """Training-mode `RayCaster.__call__` (render_kwargs_train: perturb, raw_noise_std,
    ray_noise_std) in the reference's own deterministic test mode, pytest=True: the stratified
    jitter, the inverse-cdf positions and the density noise are numpy draws after
    np.random.seed(0) (ray_utils.py:171-180, 241-244; nerf.py:179-182).  The position noise has
    no such override (raycasters.py:660-661, 673-674): the two torch.randn_like results are
    recorded as the reference makes them.  The fixture holds the draws (inputs) and the
    outputs of the call."""
    import torch
    from core.utils.ray_utils import kp_to_valid_rays
    from posegen_amd import synthetic as syn
    with tempfile.TemporaryDirectory() as wd:
        caster, kw, (wc, wf, tau_v, tau_d) = _build_reference_caster(cfg, seed_model, wd)
    W = H
    bones, kps, skts = syn.make_pose(1, seed_pose)
    c2ws, focals = syn.make_camera(1, H, W)
    rays, vids, cyls, boxes = kp_to_valid_rays(torch.tensor(c2ws), H, W, focals,
                                               kps=torch.tensor(kps), ext_scale=cfg.ext_scale)
    ro, rd = rays[0]
    sel = np.unique(np.linspace(0, ro.shape[0] - 1, n_rays).round().astype(np.int64))
    ro, rd = ro[sel].float(), rd[sel].float()
    n = ro.shape[0]
    vd = rd / torch.norm(rd, dim=-1, keepdim=True)
    ones = torch.ones(n, 1)
    batch = torch.cat([ro, rd, 0. * ones, 1. * ones, vd], -1)
    kp_b = torch.tensor(kps).expand(n, -1, -1)
    skt_b = torch.tensor(skts).expand(n, -1, -1, -1)
    cyl_b = cyls.expand(n, -1)
    bones_b = torch.tensor(bones).expand(n, -1, -1)
    S, N = cfg.n_samples, cfg.n_importance
    recorded = []
    randn_like = torch.randn_like

    def recording_randn_like(t, *a, **k):
        r = randn_like(t, *a, **k)
        recorded.append(r.clone())
        return r

    call_kw = {k: v for k, v in kw.items() if k != "ray_caster"}
    call_kw.pop("use_viewdirs", None)
    call_kw.update(perturb=perturb, raw_noise_std=raw_noise_std, ray_noise_std=ray_noise_std, pytest=True)
    caster.train()
    torch.manual_seed(1234)
    torch.randn_like = recording_randn_like
    try:
        with torch.no_grad():
            full = caster(batch, kp_batch=kp_b, skts=skt_b, cyls=cyl_b, bones=bones_b, cams=None,
                          subject_idxs=None, **call_kw)
    finally:
        torch.randn_like = randn_like
        caster.eval()
    d = {"ray_batch": batch.numpy(), "kps": kps, "skts": skts, "bones": bones, "cyl": cyls.numpy(),
         "tau_v": tau_v, "tau_d": tau_d, "seed_model": seed_model, "n_samples": S, "n_importance": N,
         "framecode_ch": cfg.framecode_ch, "n_framecodes": cfg.n_framecodes,
         "digest_coarse": _weights_digest(wc), "digest_fine": _weights_digest(wf),
         "perturb": perturb, "raw_noise_std": raw_noise_std, "ray_noise_std": ray_noise_std, "n_rays": n}
    # the pytest=True draws, exactly as the reference forms them (float64 numpy -> torch.Tensor = float32)
    f32 = lambda a: torch.Tensor(a).numpy()
    if perturb > 0:
        np.random.seed(0); d["t_rand"] = f32(np.random.rand(n, S))
        if N > 0:
            np.random.seed(0); d["u_rand"] = f32(np.random.rand(n, N))
    if raw_noise_std > 0:
        np.random.seed(0); d["noise0"] = f32(np.random.rand(n, S) * raw_noise_std)
        if N > 0:
            np.random.seed(0); d["noise1"] = f32(np.random.rand(n, S + N) * raw_noise_std)
    if ray_noise_std > 0:
        assert len(recorded) == (2 if N > 0 else 1) and recorded[0].shape == (n, S, 3), [r.shape for r in recorded]
        d["ray_noise"] = torch.cat([r * ray_noise_std for r in recorded], 1).numpy()
    for k, v in full.items():
        if torch.is_tensor(v):
            d[k] = v.numpy()
    if model_keys:
        _model_keys(d, cfg)
    np.savez_compressed(os.path.join(out, f"{name}.npz"), **d)
    acc = full["acc_map"].numpy()
    print(f"[{name}] rays={n} keys={sorted(k for k in full)} acc in [{acc.min():.3f},{acc.max():.3f}]")


GRAD_SAMPLES = 256


def grad_sample_index(numel):
    """Fixed positions at which a gradient tensor is stored in the train_grads fixtures (plus its L2 norm)."""
    return (np.arange(GRAD_SAMPLES, dtype=np.int64) * 7919) % numel


N_COND = 8


def _grad_nets(caster):
    """(tag, net) of every parameter set of the caster, each once: a single-net caster's `network_fine` IS its `network`
    (core/raycasters.py:99-104), and its gradients are stored under "coarse" alone."""
    nets = [("coarse", caster.network)]
    if caster.network_fine is not None and caster.network_fine is not caster.network:
        nets.append(("fine", caster.network_fine))
    return nets


def _sampled_grads(caster):
    out = {}
    for tag, net in _grad_nets(caster):
        for pname, p_ in net.named_parameters():
            g = p_.grad.detach().numpy().reshape(-1)
            out[(tag, pname)] = g[grad_sample_index(g.size)].copy()
    return out


def _grad_sensitivity(caster, step):
    """Largest change of a sampled gradient value, relative to its tensor's largest sampled entry, over N_COND reruns
    of `step` with every parameter multiplied by (1 + 1e-7 * normal)."""
    import torch
    base = _sampled_grads(caster)
    params = list(caster.parameters())
    keep = [p_.detach().clone() for p_ in params]
    gen = torch.Generator().manual_seed(5)
    worst = 0.0
    for _ in range(N_COND):
        with torch.no_grad():
            for p_, k_ in zip(params, keep):
                p_.copy_(k_ * (1 + 1e-7 * torch.randn(k_.shape, generator=gen)))
        step()
        got = _sampled_grads(caster)
        for key, b in base.items():
            worst = max(worst, float(np.abs(got[key] - b).max()) / max(float(np.abs(b).max()), 1e-12))
    with torch.no_grad():
        for p_, k_ in zip(params, keep):
            p_.copy_(k_)
    return worst


def gen_train_grads(out, name, cfg, *, n_rays, H, seed_model=0, seed_pose=1, perturb=1., raw_noise_std=1.,
                    use_cams=False, max_seed_tries=16, max_sens=1e-5, model_keys=False):
    """One training step of the reference, up to the gradients: `RayCaster.__call__` in training mode with
    pytest=True draws (as rays_train), the loss of Trainer.compute_loss for the shipped surreal config
    (core/trainer.py:321-383: img2mse of rgb + (1 - acc) * bg, use_background=True, base_bg=1, for the fine and the
    coarse maps, coarse_weight 1) against seeded target colours, and `loss.backward()` (trainer.py:463).  Stored: the
    inputs, the draws, the outputs, the loss and every parameter gradient of both nets as (L2 norm, 256 values at
    grad_sample_index) -- the full tensors are 7 MB.

    Conditioning: the gradient of a ReLU net jumps where a pre-activation crosses zero, and a batch has millions of
    them, some within a rounding error of zero.  On such a batch the reference's own gradient moves by up to 4e-3 of
    a tensor's largest entry when its weights move by 1e-7 relative (seen with seed_pose=2 of the h36m case: one
    view-layer unit of one coarse point), so the batch cannot pin another implementation to 1e-4.  The pose seed is
    therefore advanced until the reference's gradients move by <= `max_sens` (1e-5) under N_COND such perturbations; the
    seed used and the measured sensitivity are stored (`seed_pose`, `grad_sensitivity`).  `max_sens=None` takes the
    FIRST batch whatever its conditioning (the un-filtered fixture: its test sets the tolerance from the stored
    sensitivity instead of rejecting the batch)."""
    import torch
    from core.trainer import img2mse
    from core.utils.ray_utils import kp_to_valid_rays
    from posegen_amd import synthetic as syn
    with tempfile.TemporaryDirectory() as wd:
        caster, kw, (wc, wf, tau_v, tau_d) = _build_reference_caster(cfg, seed_model, wd)
    W = H
    for seed_pose in range(seed_pose, seed_pose + max_seed_tries):
        bones, kps, skts = syn.make_pose(1, seed_pose)
        c2ws, focals = syn.make_camera(1, H, W)
        rays, vids, cyls, boxes = kp_to_valid_rays(torch.tensor(c2ws), H, W, focals,
                                                   kps=torch.tensor(kps), ext_scale=cfg.ext_scale)
        ro, rd = rays[0]
        sel = np.unique(np.linspace(0, ro.shape[0] - 1, n_rays).round().astype(np.int64))
        ro, rd = ro[sel].float(), rd[sel].float()
        n = ro.shape[0]
        vd = rd / torch.norm(rd, dim=-1, keepdim=True)
        ones = torch.ones(n, 1)
        batch = torch.cat([ro, rd, 0. * ones, 1. * ones, vd], -1)
        kp_b = torch.tensor(kps).expand(n, -1, -1)
        skt_b = torch.tensor(skts).expand(n, -1, -1, -1)
        cyl_b = cyls.expand(n, -1)
        bones_b = torch.tensor(bones).expand(n, -1, -1)
        S, N = cfg.n_samples, cfg.n_importance
        rng = np.random.RandomState(11)
        target = torch.tensor(rng.uniform(0, 1, size=(n, 3)).astype(np.float32))
        cams = torch.tensor(rng.randint(0, cfg.n_framecodes, size=n).astype(np.float32)) if use_cams else None
        call_kw = {k: v for k, v in kw.items() if k != "ray_caster"}
        call_kw.pop("use_viewdirs", None)
        call_kw.update(perturb=perturb, raw_noise_std=raw_noise_std, ray_noise_std=0., pytest=True)

        def step():
            caster.train()
            for p_ in caster.parameters():
                p_.grad = None
            full = caster(batch, kp_batch=kp_b, skts=skt_b, cyls=cyl_b, bones=bones_b, cams=cams, subject_idxs=None, **call_kw)
            loss = img2mse(full["rgb_map"] + (1. - full["acc_map"])[..., None] * 1.0, target, reduction="mean")
            if "rgb0" in full:
                loss = loss + img2mse(full["rgb0"] + (1. - full["acc0"])[..., None] * 1.0, target, reduction="mean") * 1.0
            loss.backward()
            return full, loss

        full, loss = step()
        sens = _grad_sensitivity(caster, step)
        print(f"[{name}] seed_pose={seed_pose}: gradient sensitivity to 1e-7 weight noise {sens:.2e}")
        if max_sens is None or sens <= max_sens:
            break
    else:
        raise SystemExit(f"[{name}] no well-conditioned batch in {max_seed_tries} pose seeds")
    full, loss = step()             # the gradients of the unperturbed weights back in .grad
    caster.eval()
    d = {"ray_batch": batch.numpy(), "kps": kps, "skts": skts, "bones": bones, "cyl": cyls.numpy(), "target": target.numpy(),
         "tau_v": tau_v, "tau_d": tau_d, "seed_model": seed_model, "n_samples": S, "n_importance": N,
         "framecode_ch": cfg.framecode_ch, "n_framecodes": cfg.n_framecodes,
         "digest_coarse": _weights_digest(wc), "digest_fine": _weights_digest(wf),
         "perturb": perturb, "raw_noise_std": raw_noise_std, "ray_noise_std": 0., "n_rays": n, "loss": float(loss),
         "seed_pose": seed_pose, "grad_sensitivity": sens}
    if cfg.density_type != "relu":
        d["density_softplus"] = int(cfg.density_type == "softplus")
        d["softplus_shift"] = float(cfg.softplus_shift)
    if cams is not None:
        d["cams"] = cams.numpy()
    if model_keys:
        _model_keys(d, cfg)
    f32 = lambda a: torch.Tensor(a).numpy()
    if perturb > 0:
        np.random.seed(0); d["t_rand"] = f32(np.random.rand(n, S))
        if N > 0:
            np.random.seed(0); d["u_rand"] = f32(np.random.rand(n, N))
    if raw_noise_std > 0:
        np.random.seed(0); d["noise0"] = f32(np.random.rand(n, S) * raw_noise_std)
        if N > 0:
            np.random.seed(0); d["noise1"] = f32(np.random.rand(n, S + N) * raw_noise_std)
    for k in ("rgb_map", "acc_map", "rgb0", "acc0"):
        if k in full:
            d[k] = full[k].detach().numpy()
    worst = 0.0
    for tag, net in _grad_nets(caster):
        for pname, p_ in net.named_parameters():
            g = p_.grad
            assert g is not None, (tag, pname)
            g = g.detach().numpy().reshape(-1)
            d[f"gnorm_{tag}_{pname}"] = np.float64(np.linalg.norm(g.astype(np.float64)))
            d[f"gval_{tag}_{pname}"] = g[grad_sample_index(g.size)]
            worst = max(worst, float(np.abs(g).max()))
    np.savez_compressed(os.path.join(out, f"{name}.npz"), **d)
    print(f"[{name}] rays={n} loss={float(loss):.6f} max |grad| {worst:.3e}, {sum(1 for k in d if k.startswith('gnorm_'))} gradient tensors")


def gen_train_grads_pose(out, name, cfg, *, n_rays, H, n_poses, seed_model=0, seed_pose=1, perturb=1., raw_noise_std=1.,
                         use_cams=False, max_seed_tries=16, max_sens=1e-5, model_keys=False):
    """gen_train_grads with pose refinement (opt_pose, core/trainer.py:286-313): the reference's training step with `skts`
    requiring a gradient, one pose per ray as PoseOptLayer hands them over by kp_idx -- `n_poses` frames, each seen by its own
    camera frame's rays, the batch split evenly between them.  Stored besides what gen_train_grads stores: the per-frame
    poses and cylinders (`skts`, `kps`, `bones`, `cyl` [n_poses, ...]), `kp_idx` [n] and dL/dskts of every ray in full
    (`dskts` [n,24,4,4]: n x 384 floats).  The conditioning filter is gen_train_grads', with the pose gradient among the
    values it watches."""
    import torch
    from core.trainer import img2mse
    from core.utils.ray_utils import kp_to_valid_rays
    from posegen_amd import synthetic as syn
    with tempfile.TemporaryDirectory() as wd:
        caster, kw, (wc, wf, tau_v, tau_d) = _build_reference_caster(cfg, seed_model, wd)
    W = H
    per = n_rays // n_poses
    for seed_pose in range(seed_pose, seed_pose + max_seed_tries):
        bones, kps, skts = syn.make_pose(n_poses, seed_pose)
        c2ws, focals = syn.make_camera(n_poses, H, W)
        rays, vids, cyls, boxes = kp_to_valid_rays(torch.tensor(c2ws), H, W, focals,
                                                   kps=torch.tensor(kps), ext_scale=cfg.ext_scale)
        ros, rds, kp_idx = [], [], []
        for f in range(n_poses):
            ro, rd = rays[f]
            sel = np.unique(np.linspace(0, ro.shape[0] - 1, per).round().astype(np.int64))
            ros.append(ro[sel].float()); rds.append(rd[sel].float()); kp_idx += [f] * len(sel)
        ro, rd = torch.cat(ros), torch.cat(rds)
        kp_idx = np.asarray(kp_idx, dtype=np.int64)
        n = ro.shape[0]
        vd = rd / torch.norm(rd, dim=-1, keepdim=True)
        ones = torch.ones(n, 1)
        batch = torch.cat([ro, rd, 0. * ones, 1. * ones, vd], -1)
        kp_b = torch.tensor(kps)[kp_idx]
        skt_b = torch.tensor(skts)[kp_idx].clone().requires_grad_(True)
        cyl_b = cyls[kp_idx]
        bones_b = torch.tensor(bones)[kp_idx]
        S, N = cfg.n_samples, cfg.n_importance
        rng = np.random.RandomState(11)
        target = torch.tensor(rng.uniform(0, 1, size=(n, 3)).astype(np.float32))
        cams = torch.tensor(rng.randint(0, cfg.n_framecodes, size=n).astype(np.float32)) if use_cams else None
        call_kw = {k: v for k, v in kw.items() if k != "ray_caster"}
        call_kw.pop("use_viewdirs", None)
        call_kw.update(perturb=perturb, raw_noise_std=raw_noise_std, ray_noise_std=0., pytest=True)

        def step():
            caster.train()
            for p_ in caster.parameters():
                p_.grad = None
            skt_b.grad = None
            full = caster(batch, kp_batch=kp_b, skts=skt_b, cyls=cyl_b, bones=bones_b, cams=cams, subject_idxs=None, **call_kw)
            loss = img2mse(full["rgb_map"] + (1. - full["acc_map"])[..., None] * 1.0, target, reduction="mean")
            if "rgb0" in full:
                loss = loss + img2mse(full["rgb0"] + (1. - full["acc0"])[..., None] * 1.0, target, reduction="mean") * 1.0
            loss.backward()
            return full, loss

        def pose_sens():
            """_grad_sensitivity over the parameters and the pose gradient (relative to its largest entry)"""
            base = skt_b.grad.detach().clone()
            params = list(caster.parameters())
            keep = [p_.detach().clone() for p_ in params]
            gen = torch.Generator().manual_seed(5)
            worst = 0.0
            for _ in range(N_COND):
                with torch.no_grad():
                    for p_, k_ in zip(params, keep):
                        p_.copy_(k_ * (1 + 1e-7 * torch.randn(k_.shape, generator=gen)))
                step()
                worst = max(worst, float((skt_b.grad - base).abs().max()) / max(float(base.abs().max()), 1e-12))
            with torch.no_grad():
                for p_, k_ in zip(params, keep):
                    p_.copy_(k_)
            step()
            return worst

        full, loss = step()
        sens = max(_grad_sensitivity(caster, step), pose_sens())
        print(f"[{name}] seed_pose={seed_pose}: gradient sensitivity to 1e-7 weight noise {sens:.2e}")
        if max_sens is None or sens <= max_sens:
            break
    else:
        raise SystemExit(f"[{name}] no well-conditioned batch in {max_seed_tries} pose seeds")
    full, loss = step()             # the gradients of the unperturbed weights back in .grad
    caster.eval()
    d = {"ray_batch": batch.numpy(), "kps": kps, "skts": skts, "bones": bones, "cyl": cyls.numpy(), "kp_idx": kp_idx,
         "target": target.numpy(), "tau_v": tau_v, "tau_d": tau_d, "seed_model": seed_model, "n_samples": S, "n_importance": N,
         "framecode_ch": cfg.framecode_ch, "n_framecodes": cfg.n_framecodes,
         "digest_coarse": _weights_digest(wc), "digest_fine": _weights_digest(wf),
         "perturb": perturb, "raw_noise_std": raw_noise_std, "ray_noise_std": 0., "n_rays": n, "loss": float(loss.detach()),
         "seed_pose": seed_pose, "grad_sensitivity": sens, "dskts": skt_b.grad.detach().numpy().copy()}
    if cams is not None:
        d["cams"] = cams.numpy()
    if model_keys:
        _model_keys(d, cfg)
    f32 = lambda a: torch.Tensor(a).numpy()
    if perturb > 0:
        np.random.seed(0); d["t_rand"] = f32(np.random.rand(n, S))
        if N > 0:
            np.random.seed(0); d["u_rand"] = f32(np.random.rand(n, N))
    if raw_noise_std > 0:
        np.random.seed(0); d["noise0"] = f32(np.random.rand(n, S) * raw_noise_std)
        if N > 0:
            np.random.seed(0); d["noise1"] = f32(np.random.rand(n, S + N) * raw_noise_std)
    for k in ("rgb_map", "acc_map", "rgb0", "acc0"):
        if k in full:
            d[k] = full[k].detach().numpy()
    for tag, net in _grad_nets(caster):
        for pname, p_ in net.named_parameters():
            g = p_.grad.detach().numpy().reshape(-1)
            d[f"gnorm_{tag}_{pname}"] = np.float64(np.linalg.norm(g.astype(np.float64)))
            d[f"gval_{tag}_{pname}"] = g[grad_sample_index(g.size)]
    np.savez_compressed(os.path.join(out, f"{name}.npz"), **d)
    print(f"[{name}] rays={n} poses={n_poses} loss={float(loss.detach()):.6f} max |dL/dskts| {float(np.abs(d['dskts']).max()):.3e}")


def gen_eval_edges(out, name="eval_edges", seed_model=0, seed_pose=21, n_samples=33):
    """The embed + MLP stage alone with NON-UNIFORM cutoffs: the reference's own embedders (encode_inputs) and both of its
    networks (run_network) on rays aimed at joints, `cutoff_dist` drawn per joint in [0.3, 0.7] independently for embed_fn and
    embeddirs_fn, tau_v != tau_d.  Arrays only: the inputs and raw of both nets (9 x 33 points)."""
    import torch
    from posegen_amd import synthetic as syn
    from posegen_amd.config import surreal_config
    cfg = surreal_config(n_samples=n_samples, n_importance=16)      # (N_importance > 0: the caster builds the fine net)
    with tempfile.TemporaryDirectory() as wd:
        caster, kw, (wc, wf, _, _) = _build_reference_caster(cfg, seed_model, wd)
    rng = np.random.RandomState(2101)
    cut_v = rng.uniform(0.3, 0.7, 24).astype(np.float32)
    cut_d = rng.uniform(0.3, 0.7, 24).astype(np.float32)
    tau_v, tau_d = 20.0, 79.6
    with torch.no_grad():
        caster.embed_fn.cutoff_dist.copy_(torch.tensor(cut_v))
        caster.embeddirs_fn.cutoff_dist.copy_(torch.tensor(cut_d))
    caster.embed_fn.tau = torch.tensor(tau_v)
    caster.embeddirs_fn.tau = torch.tensor(tau_d)
    bones, kps, skts = syn.make_pose(1, seed_pose)
    c2ws, _ = syn.make_camera(1, 64, 64)
    cam = c2ws[0, :3, 3].astype(np.float64)
    joints = np.array([0, 3, 4, 7, 12, 15, 18, 20, 23])
    aim = kps[0, joints].astype(np.float64) + rng.uniform(-0.08, 0.08, (len(joints), 3))
    dist = np.linalg.norm(aim - cam, axis=-1, keepdims=True)
    d_np = ((aim - cam) / dist * rng.uniform(0.8, 1.25, (len(joints), 1))).astype(np.float32)    # (rays are not unit length)
    n = len(joints)
    o = torch.tensor(np.repeat(cam[None].astype(np.float32), n, 0))
    d = torch.tensor(d_np)
    mid = torch.tensor((dist[:, 0] / np.linalg.norm(d_np.astype(np.float64), axis=-1)).astype(np.float32))[:, None]
    z = mid + torch.linspace(-0.9, 0.9, n_samples)[None, :] * torch.tensor(rng.uniform(0.7, 1.0, (n, 1)).astype(np.float32))
    pts = o[:, None, :] + d[:, None, :] * z[..., None]
    kp_b = torch.tensor(kps).expand(n, -1, -1)
    skt_b = torch.tensor(skts).expand(n, -1, -1, -1)
    bones_b = torch.tensor(bones).expand(n, -1, -1)
    pk = kw["preproc_kwargs"]
    jc = caster.get_subject_joint_coords(None, pts.device)
    raws = {}
    with torch.no_grad():
        for tag, net in (("coarse", caster.network), ("fine", caster.network_fine)):
            enc = caster.encode_inputs(pts, [o[:, None, :], d[:, None, :]], kp_b, skt_b, bones_b, cam_idxs=None,
                                       subject_idxs=None, joint_coords=jc, network=net, **pk)
            raws[tag] = caster.run_network(enc, net).numpy()
    vd = d / torch.norm(d, dim=-1, keepdim=True)
    ones = torch.ones(n, 1)
    batch = torch.cat([o, d, 0. * ones, 1. * ones, vd], -1)
    np.savez_compressed(os.path.join(out, f"{name}.npz"), ray_batch=batch.numpy(), z=z.numpy(), skts=skts, kps=kps,
                        cutoff_v=cut_v, cutoff_d=cut_d, tau_v=tau_v, tau_d=tau_d, seed_model=seed_model,
                        n_samples=n_samples, n_importance=0, digest_coarse=_weights_digest(wc), digest_fine=_weights_digest(wf),
                        raw_coarse=raws["coarse"].reshape(n, n_samples, 4), raw_fine=raws["fine"].reshape(n, n_samples, 4))
    sig = raws["coarse"].reshape(-1, 4)[:, 3]
    print(f"[{name}] {n} rays x {n_samples}: sigma_raw in [{sig.min():.2f}, {sig.max():.2f}], {(sig > 0).mean():.2f} of the points occupied")


def gen_frame(out, name, cfg, H, chunk, seed_model=0, seed_pose=1, n_frames=2):
    """a-1/a-3: whole frames through the reference's render_path (bbox cull,
    chunk loop with a chunk boundary inside the frame, white background)."""
    import torch
    import run_nerf
    from posegen_amd import synthetic as syn
    with tempfile.TemporaryDirectory() as wd:
        caster, kw, (wc, wf, tau_v, tau_d) = _build_reference_caster(cfg, seed_model, wd)
    W = H
    bones, kps, skts = syn.make_pose(n_frames, seed_pose)
    c2ws, focals = syn.make_camera(n_frames, H, W)
    import tqdm as _tqdm
    run_nerf.tqdm = lambda x, *a, **k: x
    rgbs, disps, accs, vids, boxes = run_nerf.render_path(
        torch.tensor(c2ws), (H, W, focals), chunk, kw, kp=torch.tensor(kps),
        skts=torch.tensor(skts), bones=torch.tensor(bones), cams=None, white_bkgd=True,
        ret_acc=True, ext_scale=cfg.ext_scale)
    np.savez_compressed(
        os.path.join(out, f"{name}.npz"), H=H, W=W, chunk=chunk, c2ws=c2ws, focals=focals,
        bones=bones, kps=kps, skts=skts, tau_v=tau_v, tau_d=tau_d, seed_model=seed_model,
        n_samples=cfg.n_samples, n_importance=cfg.n_importance,
        rgbs=rgbs, disps=disps, accs=accs, n_valid=np.array([len(v) for v in vids]),
        boxes=np.array([[b[0], b[1]] for b in boxes]),
        digest_coarse=_weights_digest(wc), digest_fine=_weights_digest(wf))
    print(f"[{name}] frames={n_frames} valid={[len(v) for v in vids]} acc max={accs.max():.3f}")


def gen_frame_metrics(out):
    """Frame scores (posegen_amd/evaluate.py, pg_frame_metrics): tiny uint8 ground-truth images, masks and a background, float32
    "rendered" frames (ground truth plus seeded noise, with a region that is constant white in both), boxes, and for every box
    of at least 11 x 11 the value of the vendored `pytorch_msssim.SSIM(size_average=False)` on the cropped pair formed by the
    lines of run_render.py:912, 935-937, 944-951 -- float32, one value per image (what `box_ssim.mean()` would be, if :952 could
    run) -- with the float32 taps of that package's `gaussian(11, 1.5)`.  Two frame sizes: 36 x 48, and 50 x 37 (odd width)."""
    import torch
    from pytorch_msssim import SSIM, gaussian
    rng = np.random.RandomState(20)
    d = {"taps": gaussian(11, 1.5).numpy()}
    ssim_eval = SSIM(size_average=False)
    sets = {"a": (2, 36, 48, [(0, 0, 48, 36), (3, 5, 14, 16), (10, 4, 22, 17), (0, 0, 11, 36), (37, 25, 48, 36), (0, 20, 30, 36),
                              (20, 0, 48, 14), (5, 2, 48, 36), (4, 3, 46, 35), (1, 1, 47, 12)]),
            "b": (1, 50, 37, [(0, 0, 37, 50), (1, 1, 36, 49), (20, 30, 37, 50), (0, 0, 12, 11), (3, 0, 37, 43)])}
    cases = []
    for tag, (F, H, W, boxes) in sets.items():
        yy, xx = np.mgrid[0:H, 0:W]
        imgs = np.empty((F, H, W, 3), dtype=np.uint8)
        masks = np.empty((F, H, W), dtype=np.uint8)
        rgbs = np.empty((F, H, W, 3), dtype=np.float32)
        for f in range(F):
            smooth = 127 + 90 * np.stack([np.sin(xx / (5. + c + f) + yy / 9.) * np.cos(yy / (4. + f) - c) for c in range(3)], -1)
            imgs[f] = np.clip(smooth + rng.randint(-20, 21, size=(H, W, 3)), 0, 255).astype(np.uint8)
            masks[f] = ((xx - W * (0.45 + 0.1 * f)) ** 2 / (0.3 * W) ** 2 + (yy - H * 0.55) ** 2 / (0.35 * H) ** 2 < 1).astype(np.uint8)
            white = (yy < H // 3) & (xx >= W - W // 3 - 13)              # > 11 x 11: windows that see nothing but white
            imgs[f][white] = 255
            rgbs[f] = np.clip(imgs[f] / 255. + rng.normal(0, 0.06, size=(H, W, 3)), 0, 1).astype(np.float32)
            rgbs[f][white] = 1.0
        bkgd = rng.randint(0, 256, size=(1, H, W, 3)).astype(np.uint8)
        d.update({f"imgs_{tag}": imgs, f"masks_{tag}": masks, f"bkgds_{tag}": bkgd, f"rgbs_{tag}": rgbs,
                  f"boxes_{tag}": np.asarray(boxes, dtype=np.int32)})
        vals = np.full((F, len(boxes), 2), np.nan, dtype=np.float32)
        for f in range(F):
            for b, (x0, y0, x1, y1) in enumerate(boxes):
                for use_bg in (0, 1):
                    gt_img = imgs[f] / 255.
                    gt_mask = masks[f][:, :, None]
                    if use_bg:
                        gt_img = gt_img * gt_mask + (1. - gt_mask) * (bkgd[0] / 255.)
                    gt_cropped = gt_img[y0:y1, x0:x1].astype(np.float32)
                    rgb_cropped = rgbs[f][y0:y1, x0:x1]
                    rgb_tensor = torch.tensor(rgb_cropped[None]).permute(0, 3, 1, 2)
                    gt_tensor = torch.tensor(gt_cropped[None]).permute(0, 3, 1, 2)
                    v = ssim_eval(rgb_tensor, gt_tensor)
                    assert v.shape == (1,) and v.dtype == torch.float32
                    vals[f, b, use_bg] = v.numpy()[0]
                    cases.append(float(v))
        d[f"ssim_{tag}"] = vals              # [frame, box, use_bg]
    np.savez_compressed(os.path.join(out, "frame_metrics.npz"), **d)
    print(f"[frame_metrics] {len(cases)} reference SSIM values in [{min(cases):.4f}, {max(cases):.4f}]")


def gen_frame_metrics_val(out):
    """Validation scores (posegen_amd/evaluate.py, pg_frame_metrics_val): the frames of frame_metrics.npz area-averaged (numpy, this
    repository's tests/metrics_ref.area_average) to H // rf x W // rf for rf = 2, 3 -- 36 x 48 -> 18 x 24, 12 x 16 and
    50 x 37 -> 25 x 18, 16 x 12, where the size ratios are not integers -- and for every frame, with and without backgrounds, what
    the lines of evaluation_helpers.py:307-344 give on the whole frame: F.interpolate(bilinear, align_corners=False) in float32,
    the vendored `SSIM(size_average=False)`, and the literal PSNR lines -- all pixels (:348), foreground (:325-327) and under a
    valid rectangle (:336-338).  Only arrays are stored."""
    import torch
    import torch.nn.functional as F
    from pytorch_msssim import SSIM
    from tests.metrics_ref import area_average
    g = np.load(os.path.join(out, "frame_metrics.npz"))
    ssim_eval = SSIM(size_average=False)
    d, n = {}, 0
    valid = {"a": (9, 4, 41, 33), "b": (0, 7, 30, 50)}
    for tag in "ab":
        imgs, masks, bkgd, rgbs = g[f"imgs_{tag}"], g[f"masks_{tag}"], g[f"bkgds_{tag}"][0], g[f"rgbs_{tag}"]
        nf, H, W = masks.shape
        vx0, vy0, vx1, vy1 = valid[tag]
        valid_mask = np.zeros((H, W, 1), dtype=np.float32)
        valid_mask[vy0:vy1, vx0:vx1] = 1
        d[f"valid_{tag}"] = np.asarray(valid[tag], dtype=np.int32)
        for rf in (2, 3):
            lo = np.stack([area_average(rgbs[f], rf) for f in range(nf)])
            ssim = np.empty((nf, 2), dtype=np.float32)
            psnr = np.empty((nf, 2, 3), dtype=np.float64)
            for f in range(nf):
                for use_bg in (0, 1):
                    gt_img = imgs[f] / 255.
                    gt_mask = masks[f][:, :, None].astype(np.float32)
                    if use_bg:
                        gt_img = gt_img * gt_mask + (1. - gt_mask) * (bkgd / 255.)
                    gt_imgs = gt_img.astype(np.float32)[None]
                    th_rgbs = torch.tensor(lo[f:f + 1]).permute(0, 3, 1, 2)
                    th_rgbs = F.interpolate(th_rgbs, size=gt_imgs.shape[1:3], mode='bilinear', align_corners=False).cpu()
                    up = th_rgbs.permute(0, 2, 3, 1).numpy()
                    th_gt = torch.tensor(gt_imgs).permute(0, 3, 1, 2).cpu()
                    v = ssim_eval(th_rgbs, th_gt)
                    assert v.shape == (1,) and v.dtype == torch.float32 and up.dtype == np.float32
                    ssim[f, use_bg] = v.numpy()[0]
                    sqr_diff = np.square(gt_imgs - up)
                    psnr[f, use_bg, 0] = (-10. * np.log10(np.mean(sqr_diff.reshape(1, -1), axis=-1)))[0]
                    for j, m in ((1, gt_mask[None]), (2, valid_mask[None])):
                        denom = np.maximum(m.reshape(1, -1).sum(-1) * 3., 1.)
                        psnr[f, use_bg, j] = (-10. * np.log10((sqr_diff * m[..., :1]).reshape(1, -1).sum(-1) / denom))[0]
                    n += 1
            d[f"lo_{tag}_rf{rf}"], d[f"ssim_{tag}_rf{rf}"], d[f"psnr_{tag}_rf{rf}"] = lo, ssim, psnr
    np.savez_compressed(os.path.join(out, "frame_metrics_val.npz"), **d)
    print(f"[frame_metrics_val] {n} cases")


def _reference_definitions(path, names, extra=None):
    """The top-level functions and classes `names` of the reference file `path`, compiled from its syntax tree into a namespace
    that holds numpy and torch only (and `extra`, the further globals those definitions name): the file itself is never imported
    (run_gan.py parses argv and loads model files when it is)."""
    import ast
    import torch
    with open(path) as f:
        tree = ast.parse(f.read(), filename=path)
    body = [n for n in tree.body if isinstance(n, (ast.FunctionDef, ast.ClassDef)) and n.name in names]
    missing = set(names) - {n.name for n in body}
    if missing:
        sys.exit(f"gen_golden: {path} does not define {sorted(missing)}")
    ns = {"np": np, "torch": torch}
    ns.update(extra or {})
    exec(compile(ast.Module(body=body, type_ignores=[]), path, "exec"), ns)
    return ns


POSE_SCORE_SETS = {"j14": [1, 2, 4, 5, 7, 8, 12, 15, 16, 17, 18, 19, 20, 21], "j17": list(range(17)), "j24": list(range(24)),
                   "mirror": [1, 2, 4, 5, 7, 8, 12, 15, 16, 17, 18, 19, 20, 21]}
POSE_SCORE_MIN_RATIO = 1e-2


def gen_pose_scores(out, ref_root):
    """Pose scores (posegen_amd/pose_eval.py, pg_pose_scores): seeded body-like poses -- synthetic.make_pose key points in metres
    (a 1.7 m body), a subset of the 24 joints as ground truth, the prediction = ground truth + 3 cm joint noise under a random
    similarity transform (scale 0.7 .. 1.4, any rotation, a shift of up to 1 m) -- 32 poses each of 14, 17 and 24 joints, and 8
    14-joint poses whose prediction is mirrored as well, so that the reference's own det < 0 branch runs.  A pose whose normalised
    cross-covariance has s3 / s1 < 1e-2 (mirrored: or (s2 - s3) / s1 < 1e-2) is drawn again, so every stored pose is compared.
    Stored: the float32 inputs and, on them, what the reference returns: `procrustes` (d, Z, scale) as
    Criterion3DPose_ProcrustesCorrected calls it and that criterion's distances, Criterion_MPJPE, Criterion3DPose_leastQuaresScaled
    (evaluation_helpers.py:387-522), compute_similarity_transform and reconstruction_error(reduction=None) (run_gan.py:1380-1456).
    Only arrays are stored."""
    import torch
    from posegen_amd import synthetic as syn
    from tests import pose_scores_ref as ref
    eh = _reference_definitions(os.path.join(ref_root, "core", "utils", "evaluation_helpers.py"),
                                ["procrustes", "Criterion_MPJPE", "Criterion3DPose_ProcrustesCorrected", "Criterion3DPose_leastQuaresScaled"])
    rg = _reference_definitions(os.path.join(ref_root, "run_gan.py"),
                                ["compute_similarity_transform", "compute_similarity_transform_batch", "reconstruction_error"])
    rng = np.random.RandomState(20240607)
    _, kps, _ = syn.make_pose(256, seed=31, sigma=0.35)
    kps = kps.astype(np.float64)
    height = (kps[..., 1].max(1) - kps[..., 1].min(1)).mean()
    kps *= 1.7 / max(height, 1e-9)                                  # metres
    d, next_pose, redrawn = {}, 0, 0
    for tag, joints in POSE_SCORE_SETS.items():
        n = 8 if tag == "mirror" else 32
        preds, gts = [], []
        while len(preds) < n:
            gt = kps[next_pose % len(kps)][joints] + rng.normal(0, 0.5, 3)
            next_pose += 1
            q, _ = np.linalg.qr(rng.normal(size=(3, 3)))
            q *= np.sign(np.linalg.det(q))                          # a rotation
            if tag == "mirror":
                q = q @ np.diag([-1.0, 1.0, 1.0])
            pred = rng.uniform(0.7, 1.4) * (gt + rng.normal(0, 0.03, gt.shape)) @ q.T + rng.uniform(-1, 1, 3)
            pred, gt = pred.astype(np.float32), gt.astype(np.float32)
            r3, gap = ref.conditioning(pred[None], gt[None])
            if r3[0] < POSE_SCORE_MIN_RATIO or (tag == "mirror" and gap[0] < POSE_SCORE_MIN_RATIO):
                redrawn += 1
                continue
            preds.append(pred)
            gts.append(gt)
        pred, gt = np.stack(preds), np.stack(gts)
        tp, tg = torch.tensor(pred), torch.tensor(gt)
        mpjpe = eh["Criterion_MPJPE"](reduction=None)
        pa_dist, pa_kps = eh["Criterion3DPose_ProcrustesCorrected"](mpjpe)(tp, tg)
        n_dist, n_kps = eh["Criterion3DPose_leastQuaresScaled"](mpjpe)(tp, tg)
        proc = [eh["procrustes"](gt[i].copy(), pred[i].copy()) for i in range(n)]
        assert all(np.array_equal(proc[i][1], pa_kps[i].numpy()) for i in range(n))
        d[f"pred_{tag}"], d[f"gt_{tag}"] = pred, gt
        d[f"mpjpe_dist_{tag}"] = mpjpe(tp, tg).numpy()
        d[f"mpjpe_mean_{tag}"] = eh["Criterion_MPJPE"](reduction="mean")(tp, tg).numpy()
        d[f"pa_dist_{tag}"], d[f"pa_kps_{tag}"] = pa_dist.numpy(), pa_kps.numpy()
        d[f"pa_d_{tag}"] = np.asarray([p[0] for p in proc])
        d[f"pa_scale_{tag}"] = np.asarray([p[2]["scale"] for p in proc])
        d[f"pa_det_{tag}"] = np.asarray([np.linalg.det(p[2]["rotation"].astype(np.float64)) for p in proc])
        d[f"n_dist_{tag}"], d[f"n_kps_{tag}"] = n_dist.numpy(), n_kps.numpy()
        d[f"cst_kps_{tag}"] = np.stack([rg["compute_similarity_transform"](pred[i], gt[i]) for i in range(n)])
        d[f"re_{tag}"] = np.asarray(rg["reconstruction_error"](pred, gt, reduction=None))
        if tag == "mirror":
            assert np.all(d[f"pa_det_{tag}"] < 0), "the mirrored poses did not take the reference's reflection branch"
    path = os.path.join(out, "pose_scores.npz")
    np.savez_compressed(path, **d)
    print(f"[pose_scores] {sum(len(d[f'pred_{t}']) for t in POSE_SCORE_SETS)} poses, {redrawn} drawn again, {os.path.getsize(path)} bytes")


class _RecordingNumpy:
    """numpy with a `random` whose ranf / randint calls are written down (Sample_from_Pool draws from the global np.random)"""

    class _Random:
        def __init__(self):
            self.log = []

        def ranf(self):
            v = np.random.ranf()
            self.log.append(("ranf", v))
            return v

        def randint(self, lo, hi):
            v = np.random.randint(lo, hi)
            self.log.append(("randint", v))
            return v

    def __init__(self):
        self.random = self._Random()

    def __getattr__(self, item):
        return getattr(np, item)


POSE_DISC_WEIGHT_SEED, POSE_DISC_INPUT_SEED, POSE_DISC_POOL_SEED = 20241020, 77, 5


def gen_pose_discriminators(out, ref_root):
    """The adversarial game (posegen_amd/discriminators.py, include/posegen_gan.h): Disc_Joint_Path, Pos3dDiscriminator,
    Pos2dDiscriminator, Sample_from_Pool and get_discriminator_accuracy lifted out of run_gan.py (:578-599, :982-1046, :1101-1115) and run
    in float64 on the CPU.  Weights come from the project's own generator (tests/gan_ref.make_params at a stored seed, loaded through
    the reference's state-dict keys); B = 5 poses.  Stored: the seeds, the inputs, both models' predictions, for the 3-D model under
    get_adv_loss's 0.5 mse(D(x), 1) the gradient of the input and per parameter the gradient's sum, abs-sum and sampled entries, the
    state-dict key lists, an accuracy case, and a pool trace (capacity 6, rows of 4 floats, three calls of 5 items under
    np.random.seed) with the draws the reference consumed.  Only arrays are stored."""
    import copy
    import torch
    import torch.nn as nn
    from posegen_amd import discriminators as disc
    from tests import gan_ref
    rec = _RecordingNumpy()
    rg = _reference_definitions(os.path.join(ref_root, "run_gan.py"),
                                ["Disc_Joint_Path", "Pos3dDiscriminator", "Pos2dDiscriminator", "Sample_from_Pool", "get_discriminator_accuracy"],
                                extra={"nn": nn, "copy": copy})
    d = {"weight_seed": np.int64(POSE_DISC_WEIGHT_SEED), "input_seed": np.int64(POSE_DISC_INPUT_SEED), "pool_seed": np.int64(POSE_DISC_POOL_SEED)}
    for tag, cls, spec in (("3d", "Pos3dDiscriminator", disc.pos3d_spec()), ("2d", "Pos2dDiscriminator", disc.pos2d_spec())):
        model = rg[cls]().double()
        keys = list(model.state_dict().keys())
        params = gan_ref.make_params(spec, POSE_DISC_WEIGHT_SEED)
        sd = {}
        for p, (name, _, _, _) in enumerate(spec.paths):
            for lname, (w, b) in zip(disc.LAYER_NAMES, params[p]):
                prefix = f"{name}.{lname}" if name else lname
                sd[prefix + ".weight"], sd[prefix + ".bias"] = torch.tensor(w).double(), torch.tensor(b).double()
        model.load_state_dict(sd, strict=True)
        x = gan_ref.make_inputs(spec, 5, POSE_DISC_INPUT_SEED)
        xt = torch.tensor(x).double().requires_grad_(True)
        pred = model(xt)
        d[f"keys_{tag}"] = np.asarray(keys)
        d[f"x_{tag}"], d[f"pred_{tag}"] = x, pred.detach().numpy()
        if tag == "3d":
            loss = 0.5 * nn.MSELoss()(pred, torch.ones_like(pred))
            loss.backward()
            d["loss_3d"], d["d_x_3d"] = np.float64(loss.item()), xt.grad.numpy()
            named = dict(model.named_parameters())
            d["grad_sum_3d"] = np.asarray([named[k].grad.sum().item() for k in keys])
            d["grad_abs_sum_3d"] = np.asarray([named[k].grad.abs().sum().item() for k in keys])
            d["grad_samples_3d"] = np.concatenate([named[k].grad.reshape(-1)[gan_ref.grad_sample_index(named[k].numel())].numpy() for k in keys])
            acc_pred = pred.detach().reshape(-1).float()
            acc_pred[:4] = torch.tensor([0.5, 1.5, 0.49999997, 1.5000001])
            d["acc_pred"] = acc_pred.numpy()
            d["acc_real"] = np.float64(rg["get_discriminator_accuracy"](acc_pred, torch.ones_like(acc_pred)))
            d["acc_fake"] = np.float64(rg["get_discriminator_accuracy"](acc_pred, torch.zeros_like(acc_pred)))
    # the pool: three calls of five rows on a pool of six, the global generator seeded, its draws written down
    rg_pool = _reference_definitions(os.path.join(ref_root, "run_gan.py"), ["Sample_from_Pool"], extra={"np": rec, "copy": copy})
    pool = rg_pool["Sample_from_Pool"](max_elements=6)
    items = np.random.RandomState(9).standard_normal((3, 5, 4)).astype(np.float32)
    np.random.seed(POSE_DISC_POOL_SEED)
    returned, swap, slot = [], np.zeros((3, 5), np.uint8), np.zeros((3, 5), np.int32)
    for c in range(3):
        full_from = min(5, max(0, 6 - pool.cur_elements))
        rec.random.log.clear()
        returned.append(np.stack(pool(items[c])))
        i = full_from - 1
        for kind, v in rec.random.log:
            if kind == "ranf":
                i += 1
                swap[c, i] = v > 0.5
            else:
                slot[c, i] = v
        assert i == 4
    d["pool_items"], d["pool_returned"], d["pool_final"] = items, np.stack(returned), np.stack(pool.items)
    d["pool_swap"], d["pool_slot"] = swap, slot
    path = os.path.join(out, "pose_discriminators.npz")
    np.savez_compressed(path, **d)
    print(f"[pose_discriminators] {os.path.getsize(path)} bytes; pool swaps {swap.sum(1)}")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--ref", default="/root/reference")
    ap.add_argument("--out", default=os.path.join(REPO, "tests", "golden"))
    ap.add_argument("--only", default="")
    a = ap.parse_args()
    _install_shims(a.ref)
    import torch
    torch.manual_seed(0)
    torch.set_num_threads(max(1, os.cpu_count() or 1))
    from posegen_amd.config import surreal_config, surreal_single_config, h36m_config
    os.makedirs(a.out, exist_ok=True)
    only = set(filter(None, a.only.split(",")))
    want = lambda k: not only or k in only
    if want("kinematics"):
        gen_kinematics(a.out)
    if want("valid_rays"):
        gen_valid_rays(a.out)
    if want("rays_surreal"):     # culled frame: contains cylinder misses -> nanmean path
        gen_render_rays(a.out, "rays_surreal", surreal_config(), n_rays=256, H=128, all_hit=False)
    if want("rays_allhit"):      # headline variant: radius 2.5, every ray hits
        gen_render_rays(a.out, "rays_allhit", surreal_config(), n_rays=128, H=128, all_hit=True,
                        seed_pose=2)
    if want("rays_coarse32"):    # N_importance = 0, 32 samples
        gen_render_rays(a.out, "rays_coarse32", surreal_config(n_samples=32, n_importance=0),
                        n_rays=96, H=64, all_hit=False, seed_pose=3)
    if want("rays_cfg1"):        # BASELINE config 1: 32 coarse + 16 importance
        gen_render_rays(a.out, "rays_cfg1", surreal_config(n_samples=32, n_importance=16),
                        n_rays=96, H=128, all_hit=False, seed_pose=4)
    if want("rays_train"):       # training-mode call: perturb + raw noise + ray noise, pytest=True draws
        gen_render_rays_train(a.out, "rays_train", surreal_config(), n_rays=64, H=128, seed_pose=6)
    if want("rays_train_coarse"):  # N_importance = 0, density noise and jitter only
        gen_render_rays_train(a.out, "rays_train_coarse", surreal_config(n_samples=32, n_importance=0),
                              n_rays=48, H=64, seed_pose=7, ray_noise_std=0.)
    if want("train_grads"):      # one training step up to loss.backward(): gradients of all 24 tensors per net
        gen_train_grads(a.out, "train_grads", surreal_config(), n_rays=48, H=128, seed_pose=8)
    if want("train_grads_h36m"): # the same with frame codes (per-ray index): + framecodes.codes.weight
        gen_train_grads(a.out, "train_grads_h36m", h36m_config(n_samples=64, n_importance=16), n_rays=24, H=128,
                        seed_model=5, seed_pose=9, use_cams=True)
    if want("rays_softplus"):    # --density_type softplus --softplus_shift 1.0 (raycasters.py:230-238), hierarchical
        gen_render_rays(a.out, "rays_softplus", surreal_config(density_type="softplus", softplus_shift=1.0),
                        n_rays=96, H=128, all_hit=False, seed_pose=10)
    if want("train_grads_softplus"):   # the training step with the softplus density (its derivative in the backward pass)
        gen_train_grads(a.out, "train_grads_softplus", surreal_config(density_type="softplus", softplus_shift=1.0),
                        n_rays=32, H=128, seed_pose=12)
    if want("train_grads_raw"):  # the FIRST h36m batch, whatever its conditioning (a ReLU kink within rounding of zero)
        gen_train_grads(a.out, "train_grads_raw", h36m_config(n_samples=64, n_importance=16), n_rays=24, H=128,
                        seed_model=5, seed_pose=2, use_cams=True, max_sens=None)
    if want("rays_h36m"):        # BASELINE config 4: frame codes, 128 coarse + 16
        gen_render_rays(a.out, "rays_h36m", h36m_config(), n_rays=64, H=128, all_hit=False,
                        seed_model=5, seed_pose=5, use_cams=True)
    if want("frame64"):
        gen_frame(a.out, "frame64", surreal_config(), H=64, chunk=1024)
    # single-net / multires_views = 0 models (configs/surreal/surreal_single.txt); after every older case, so that the
    # torch RNG state those consume does not move
    if want("rays_single"):      # the shipped single-net config: one net, multires_views = 0, 96 + 48, culled frame
        gen_render_rays(a.out, "rays_single", surreal_single_config(), n_rays=80, H=128, all_hit=False,
                        seed_pose=13, model_keys=True)
    if want("rays_single_v4"):   # the single-net algorithm alone: multires_views = 4, 64 + 16
        gen_render_rays(a.out, "rays_single_v4", surreal_config(single_net=True), n_rays=80, H=128, all_hit=False,
                        seed_pose=14, model_keys=True)
    if want("rays_views0"):      # the 0-band view embedding alone: two nets, 64 + 16
        gen_render_rays(a.out, "rays_views0", surreal_config(multires_views=0), n_rays=80, H=128, all_hit=False,
                        seed_pose=15, model_keys=True)
    if want("rays_single_train"):  # the rays_train recipe on the single-net model
        gen_render_rays_train(a.out, "rays_single_train", surreal_single_config(), n_rays=64, H=128, seed_pose=6,
                              model_keys=True)
    # pose refinement (opt_pose): dL/dskts of the reference's training step, after every older case
    if want("train_grads_pose"):     # per-ray poses, half the rays from each of two frames (PoseOptLayer by kp_idx)
        gen_train_grads_pose(a.out, "train_grads_pose", surreal_config(), n_rays=48, H=128, n_poses=2, seed_pose=16)
    if want("train_grads_pose_h36m"):  # frame codes, 64 + 16 samples, one pose for every ray
        gen_train_grads_pose(a.out, "train_grads_pose_h36m", h36m_config(n_samples=64, n_importance=16), n_rays=24, H=128,
                             n_poses=1, seed_model=5, seed_pose=17, use_cams=True)
    # the single-net training step (one parameter set, its gradients stored once under "coarse"), after every older case
    if want("train_grads_single"):       # the shipped single-net config: multires_views = 0, 96 + 48
        gen_train_grads(a.out, "train_grads_single", surreal_config(single_net=True, multires_views=0, n_samples=96, n_importance=48),
                        n_rays=48, H=128, seed_pose=18, model_keys=True)
    if want("train_grads_single_v4"):    # the single-net step alone: 4-band views, 64 + 16
        gen_train_grads(a.out, "train_grads_single_v4", surreal_config(single_net=True), n_rays=48, H=128, seed_pose=19,
                        model_keys=True)
    if want("train_grads_single_pose"):  # pose refinement on the shipped single-net config, two frames
        gen_train_grads_pose(a.out, "train_grads_single_pose",
                             surreal_config(single_net=True, multires_views=0, n_samples=96, n_importance=48),
                             n_rays=48, H=128, n_poses=2, seed_pose=20, model_keys=True)
    # per-joint cutoffs, different for the two embedders, tau_v != tau_d: embed + MLP of both nets (consumes no torch RNG state)
    if want("eval_edges"):
        gen_eval_edges(a.out)
    # frame scores: the vendored pytorch_msssim on cropped pairs (consumes no torch RNG state)
    if want("frame_metrics"):
        gen_frame_metrics(a.out)
    # validation scores: the same frames at H // rf x W // rf, torch's float32 upsampling (reads frame_metrics.npz; no RNG state)
    if want("frame_metrics_val"):
        gen_frame_metrics_val(a.out)
    # pose scores: the reference's Procrustes / MPJPE functions on seeded poses (consumes no torch RNG state)
    if want("pose_scores"):
        gen_pose_scores(a.out, a.ref)
    # the adversarial game: the reference's discriminators, accuracy and pool in float64 (consumes no torch RNG state)
    if want("pose_discriminators"):
        gen_pose_discriminators(a.out, a.ref)


if __name__ == "__main__":
    main()
