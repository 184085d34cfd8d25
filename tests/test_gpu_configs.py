"""GPU tests of the BASELINE configurations AT SIZE (configs 3-5 had only small fixtures):
  config 4  h36m 512x512 x (128+16) samples, per-ray frame codes, full frame
  config 3  the RCCL path: dist.render_path_distributed under a world-size-1 `nccl` group on cuda:0
  config 5  the GAN loop's render call: 20 poses at 512x512, crop [100:412], resize 224
plus a seeded randomised parity sweep."""
import os
import socket
import subprocess
import sys

import numpy as np
import pytest
import torch

from posegen_amd import h36m_config, surreal_config, synthetic as syn
from tests.helpers import oracle_cfg, torch_weights

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _psnr(a, b):
    mse = float(((a - b) ** 2).mean())
    return -10 * np.log10(max(mse, 1e-30)), mse


def test_config4_h36m_full_frame_at_size():
    """h36m config (128 coarse + 16 importance samples = 272 MLP evaluations per ray, 16-d frame codes with a
    per-ray index, view layer K = 920) on all 262 144 rays of a 512x512 frame: the bf16 path is bitwise
    repeatable, agrees with the exact fp32 mode on the whole frame within the bf16 bound (and 60 dB), and a
    strided 256-ray subset of BOTH equals the oracle (fp32 <= 1e-4, the north star's bound); the compensated-fp16 mode
    (pg_evalc2.hip with frame codes) is within 1e-4 of fp32 on the whole frame and of the oracle on the subset."""
    from bench import full_frame_rays
    from oracle import anerf_oracle as orc
    from posegen_amd.raycaster import HipRayCaster
    cfg = h36m_config()
    assert (cfg.n_samples, cfg.n_importance, cfg.framecode_ch) == (128, 16, 16)
    wc, wf, tv, td = syn.make_model(cfg, 0)
    c = HipRayCaster.from_weights(cfg, wc, wf, tv, td, device=DEV, precision="bf16")
    r = c.renderer
    rb, skts, cyl, rb_cpu, skts_cpu, cyl_cpu = full_frame_rays(512, 512, DEV)
    n = rb.shape[0]
    assert n == 512 * 512
    cams = (torch.arange(n, device=DEV) % cfg.n_framecodes).float()
    r.set_chunk(cfg.chunk)
    a = r.render_rays(rb, skts, cyl, cams=cams, want_alpha=False)
    b = r.render_rays(rb, skts, cyl, cams=cams, want_alpha=False)
    for k in ("rgb_map", "disp_map", "acc_map", "rgb0", "acc0"):
        assert torch.equal(a[k], b[k]), k
        assert torch.isfinite(a[k]).all(), k
    assert float(a["acc_map"].max()) > 0.9 and float(a["acc_map"].min()) < 0.05, "the frame has a body and a background"
    r.set_precision("fp32")
    e = r.render_rays(rb, skts, cyl, cams=cams, want_alpha=False)
    d_rgb = float((a["rgb_map"] - e["rgb_map"]).abs().max())
    d_acc = float((a["acc_map"] - e["acc_map"]).abs().max())
    psnr, _ = _psnr(a["rgb_map"].cpu(), e["rgb_map"].cpu())
    print(f"config 4 full frame: bf16 vs fp32 max |d rgb| {d_rgb:.2e}, |d acc| {d_acc:.2e}, PSNR {psnr:.1f} dB")
    assert d_rgb <= 2e-2 and d_acc <= 2e-2 and psnr >= 55.0
    # strided subset against the oracle (rays that hit are independent of their batch)
    sel = torch.arange(97, n, n // 256)[:256]
    ocfg = oracle_cfg(cfg, tv, td)
    ref = orc.render_rays(rb_cpu[sel], skts_cpu, cyl_cpu, ocfg, torch_weights(wc), torch_weights(wf), cfg.n_samples,
                          cfg.n_importance, cams=cams.cpu()[sel])
    # the compensated-fp16 mode on the same frame: the north star's 1e-4 at matrix-core speed, frame codes included
    r.set_precision("fp16c")
    f = r.render_rays(rb, skts, cyl, cams=cams, want_alpha=False)
    f2 = r.render_rays(rb, skts, cyl, cams=cams, want_alpha=False)
    for k in ("rgb_map", "disp_map", "acc_map", "rgb0", "acc0"):
        assert torch.equal(f[k], f2[k]), k
    dc = max(float((f[k] - e[k]).abs().max()) for k in ("rgb_map", "acc_map"))
    print(f"config 4 full frame: fp16c vs fp32 max |d rgb / acc| {dc:.2e}")
    assert dc <= 1e-4
    for name, got, tol in (("fp32", e, 1e-4), ("bf16", a, 1e-2), ("fp16c", f, 1e-4)):
        err = max(float((got[k].cpu()[sel] - ref[k]).abs().max()) for k in ("rgb_map", "acc_map"))
        ps, mse = _psnr(got["rgb_map"].cpu()[sel], ref["rgb_map"])
        print(f"config 4 subset vs oracle, {name}: max |d| {err:.2e}, rgb MSE {mse:.2e}, PSNR {ps:.1f} dB")
        assert err <= tol and mse <= 1e-4
    r.close()


def test_config4_on_chip_frame_codes_at_size():
    """BASELINE config 4's frame (262 144 rays x (128 + 144) samples, a frame-code index per ray, some rays on the mean
    code) through the on-chip variant of the 16x16x32 kernel (pg_set_onchip ALWAYS: no per-ray records, the code's part of
    the view layer from the table pg_api.hip ensure_ycode makes) against the record variant (RECORDS; what AUTO picks at
    128 samples): no record launch, bitwise repeatable, and the maps agree within the modes' own rounding (the two forms
    round the code's 16 products differently: bf16 4e-3, fp16 5e-4) -- every pass of every persistent workgroup, not only
    the first one the 64-ray golden set reaches."""
    from bench import full_frame_rays
    from posegen_amd.raycaster import HipRayCaster
    cfg = h36m_config()
    c = HipRayCaster.from_weights(cfg, *syn.make_model(cfg, 0), device=DEV, precision="bf16")
    r = c.renderer
    rb, skts, cyl, *_ = full_frame_rays(512, 512, DEV)
    n = rb.shape[0]
    cams = (torch.arange(n, device=DEV) % cfg.n_framecodes).float()
    cams[5::7] = -1.0           # (rays without a frame: the mean code, embedding.py:25-26)
    keys = ("rgb_map", "acc_map", "disp_map")
    for prec, tol in (("bf16", 4e-3), ("fp16", 5e-4)):
        r.set_precision(prec)
        maps = {}
        for mode, want_records in (("always", 0), ("records", 2), ("auto", 2)):
            r.set_onchip(mode)
            r.profile_enable(True)
            r.profile_read(); r.profile_read_aux()
            a = r.render_rays(rb, skts, cyl, cams=cams, want_alpha=False)
            torch.cuda.synchronize()
            launches, _, _ = r.profile_read()
            recs, _ = r.profile_read_aux()
            r.profile_enable(False)
            assert (launches, recs) == (2, want_records), (prec, mode, launches, recs)
            b = r.render_rays(rb, skts, cyl, cams=cams, want_alpha=False)
            assert all(torch.equal(a[k], b[k]) for k in keys), (prec, mode)
            maps[mode] = a
        r.set_onchip("auto")
        assert all(torch.equal(maps["auto"][k], maps["records"][k]) for k in keys)
        d = {k: float((maps["always"][k] - maps["records"][k]).abs().max()) for k in keys}
        print(f"config 4 frame, {prec}: on-chip frame codes vs per-ray records {d}")
        assert all(torch.isfinite(maps["always"][k]).all() for k in keys) and max(d.values()) <= tol, (prec, d)
    r.close()


def test_rccl_world1_render_path_distributed_equals_render_path():
    """The one-process-per-GPU path with RCCL actually initialised on the device: a world-size-1 `nccl` group on
    cuda:0, dist.render_path_distributed (plan, pg_render_frame_range pieces, device-fed all_gather_into_tensor,
    pg_compose_frame) == render_path, bitwise."""
    import torch.distributed as dist
    from posegen_amd.dist import render_path_distributed
    from posegen_amd.raycaster import HipRayCaster
    from posegen_amd.render import render_path
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        port = s.getsockname()[1]
    torch.cuda.set_device(0)
    dist.init_process_group("nccl", init_method=f"tcp://127.0.0.1:{port}", rank=0, world_size=1, device_id=torch.device(DEV))
    try:
        probe = torch.arange(8, device=DEV, dtype=torch.float32)
        got = torch.empty(8, device=DEV)
        dist.all_gather_into_tensor(got, probe)         # RCCL has run on this GPU
        assert torch.equal(got, probe)
        cfg = surreal_config()
        c = HipRayCaster.from_weights(cfg, *syn.make_model(cfg, 0), device=DEV, precision="bf16")
        H = W = 160
        F = 3
        _, kps, skts = syn.make_pose(F, 5)
        c2ws, focals = syn.make_camera(F, H, W)
        kw = dict(kp=torch.tensor(kps), skts=torch.tensor(skts), white_bkgd=True, ret_acc=True, ext_scale=cfg.ext_scale)
        rk = {"ray_caster": c, "N_samples": cfg.n_samples, "N_importance": cfg.n_importance}
        want = render_path(torch.tensor(c2ws), (H, W, focals), 1024, rk, **kw)
        got = render_path_distributed(torch.tensor(c2ws), (H, W, focals), 1024, rk, **kw)
        assert sum(len(v) for v in want[3]) > 3 * 1024
        for x, y in zip(want[:3], got[:3]):
            assert x.shape == y.shape and np.array_equal(x, y)
        assert np.array_equal(np.array(want[4]), np.array(got[4]))
        c.renderer.close()
    finally:
        dist.destroy_process_group()


def test_frame_ranges_compose_to_the_whole_frame_bitwise():
    """pg_render_frame_range on group-aligned runs + pg_compose_frame == pg_render_frame (the unit of work of both
    multi-GPU planners): the same plan an 8-rank job would use, executed on one GPU."""
    from posegen_amd.dist import plan_tasks
    from posegen_amd.raycaster import HipRayCaster
    from posegen_amd.rays import kp_to_boxes
    cfg = surreal_config()
    c = HipRayCaster.from_weights(cfg, *syn.make_model(cfg, 0), device=DEV, precision="bf16")
    r = c.renderer
    H = W = 256
    _, kps, skts = syn.make_pose(1, 9)
    c2ws, focals = syn.make_camera(1, H, W)
    cyls, bboxes, grids = kp_to_boxes(torch.tensor(c2ws), H, W, focals, kps=torch.tensor(kps), ext_scale=cfg.ext_scale)
    n = len(grids[0][0])
    r.set_chunk(1024)
    whole = r.render_frame(H, W, focals[0], c2ws[0], bboxes[0], torch.tensor(skts[:1]), cyls[:1], base_bg=1.0)
    tasks = plan_tasks([n], 8, 1024)
    assert len(tasks) == 8 and all(t.r0 % 1024 == 0 for t in tasks)
    pieces = [r.render_frame_range(H, W, focals[0], c2ws[0], bboxes[0], torch.tensor(skts[:1]), cyls[:1], t.r0, t.r1) for t in tasks]
    rgb = torch.cat([p[:3 * (t.r1 - t.r0)].view(-1, 3) for p, t in zip(pieces, tasks)])
    disp = torch.cat([p[3 * (t.r1 - t.r0):4 * (t.r1 - t.r0)] for p, t in zip(pieces, tasks)])
    acc = torch.cat([p[4 * (t.r1 - t.r0):] for p, t in zip(pieces, tasks)])
    parts = r.compose_frame(H, W, bboxes[0], rgb, disp, acc, base_bg=1.0)
    for x, y in zip(whole, parts):
        assert torch.equal(x, y)
    with pytest.raises(Exception):      # a run that does not start on a group boundary is refused, not rendered differently
        r.render_frame_range(H, W, focals[0], c2ws[0], bboxes[0], torch.tensor(skts[:1]), cyls[:1], 100, 1124)
    r.close()


def test_config5_gan_loop_call_at_size():
    """BASELINE config 5 at size: the render call of the GAN loop -- rpi = 20 generator poses (run_gan.py:104,
    2042-2047) at 512x512, uint8 frames, crop [100:412], anti-aliased resize to 224 (run_gan.py:2057-2081) --
    entirely on the device (render_for_regressor) against the reference-shaped host route (numpy kinematics and
    boxes, render_path, uint8 / crop / normalise / resize on the host)."""
    from posegen_amd.ganloop import IMG_NORM_MEAN, IMG_NORM_STD, render_for_regressor, resize_antialiased
    from posegen_amd.raycaster import HipRayCaster
    from posegen_amd.render import render_path
    from posegen_amd.skeleton import SURREAL_REST_SCALE, bones_to_pose, smpl_rest_pose
    cfg = surreal_config()
    c = HipRayCaster.from_weights(cfg, *syn.make_model(cfg, 0), device=DEV, precision="bf16")
    H = W = 512
    F = 20
    rest = smpl_rest_pose * SURREAL_REST_SCALE
    c2ws, focals = syn.make_camera(F, H, W)
    bones = syn.make_bones(F, 7)
    img, frames = render_for_regressor(c, torch.tensor(bones, device=DEV), rest, c2ws[0], H, W, float(focals[0]),
                                       ext_scale=cfg.ext_scale, crop=(100, 412), out_res=224, return_frames=True)
    assert img.shape == (F, 3, 224, 224) and frames.shape == (F, H, W, 3) and torch.isfinite(img).all()
    kps, skts, _ = bones_to_pose(bones, rest)
    rk = {"ray_caster": c, "N_samples": cfg.n_samples, "N_importance": cfg.n_importance}
    rgbs, *_ = render_path(torch.tensor(c2ws), (H, W, focals), 4096, rk, kp=torch.tensor(kps.astype(np.float32)),
                           skts=torch.tensor(skts.astype(np.float32)), white_bkgd=True, ext_scale=cfg.ext_scale)
    host8 = (rgbs * 255).astype(np.uint8)                                       # run_gan.py:2327
    assert np.array_equal(frames.cpu().numpy(), host8)
    assert (host8 < 255).any(axis=(1, 2, 3)).all(), "every frame shows the body"
    x = torch.tensor(host8[:, 100:412, 100:412, :]).permute(0, 3, 1, 2).float() / 255.0
    x = (x - torch.tensor(IMG_NORM_MEAN).view(1, 3, 1, 1)) / torch.tensor(IMG_NORM_STD).view(1, 3, 1, 1)
    want = resize_antialiased(x, (224, 224))
    assert float((img.cpu() - want).abs().max()) <= 1e-4
    c.renderer.close()


def test_seeded_parity_sweep():
    """tools/parity_sweep.py as a test: 14 seeded random cases (model, pose, camera jitter, 32-128 coarse and 0-32
    importance samples, inverse-depth sampling, frame codes or the mean code), 256 rays each, every precision mode
    against the oracle.  Bounds = what the modes support: the exact-class modes hold the north
    star's 1e-4 wherever the reference's own inverse-cdf sampling is well conditioned (no importance samples, or
    >= 64 coarse samples) and 3e-4 in the ill-conditioned corner (32-48 coarse samples with importance sampling,
    where the fp32 kernel and the fp32 oracle already part by 8e-5); every mode stays above 40 dB, i.e. inside
    'MSE <= 1e-4', everywhere."""
    from tools.parity_sweep import sweep
    recs = sweep(cases=14, rays=256, verbose=True)
    for rec in recs:
        well = rec["N"] == 0 or rec["S"] >= 64
        for m, e in rec["err"].items():
            worst = max(e["rgb"], e["acc"])
            bound = {"fp32": 1e-4 if well else 3e-4, "fp16c": 1e-4 if well else 3e-4, "bf16x3": 1e-4 if well else 3e-4,
                     "fp16": 5e-3 if well else 2e-2, "bf16": 1e-2 if well else 3e-2}[m]
            assert worst <= bound, (rec["case"], rec["S"], rec["N"], m, worst)
            assert e["mse"] <= 1e-4, (rec["case"], m, e["mse"])


@pytest.mark.parametrize("prec,bound", [("bf16", 2e-2), ("fp16", 1e-2), ("fp16c", 1e-3)])
def test_record_kernels_on_odd_ray_and_sample_counts(prec, bound):
    """The 16x16x32 kernel (bf16 / fp16: its on-chip form or, above 112 samples per ray, its record form) and the compensated kernel
    (pg_evalc2.hip, record-free), each with one pose per call and with the pose given per ray, against the fp32 kernel (direct view layer, no records) on shapes that stress their pass bookkeeping: ray counts that leave the last
    pass and the last record tile ragged (1 ray ... 4097 rays), sample counts that make passes straddle 2 to 5 rays at
    every offset (64 ... 200 samples), with and without importance samples.  fp32 is pinned to the reference by
    test_gpu_parity.py; the bounds are what the modes' operand precision gives on random-weight nets with importance sampling
    (tools/parity_sweep.py: worst cases 1.5e-2 / 1.2e-2 / 1.6e-4; one ray of the 2049 x (80 + 16) case here sits at 4.0e-4 in
    fp16c, with records and, identically, in the direct form: its importance samples amplify a 1e-5 coarse difference) -- a
    bookkeeping error shows as 0.1 ... 1."""
    from bench import full_frame_rays
    from posegen_amd import PREC_BY_NAME, surreal_config, synthetic as syn
    from posegen_amd.raycaster import HipRayCaster
    cfg = surreal_config()
    c = HipRayCaster.from_weights(cfg, *syn.make_model(cfg, 2), device=DEV, precision="fp32")
    r = c.renderer
    rb, skts, cyl, *_ = full_frame_rays(128, 128, torch.device(DEV))
    rb = rb[torch.randperm(rb.shape[0], generator=torch.Generator().manual_seed(3)).to(DEV)]      # rays of a pass unrelated
    worst = 0.0
    try:
        for n, S, N in ((1, 64, 0), (7, 65, 5), (33, 79, 16), (255, 96, 0), (1000, 127, 16), (4097, 64, 16), (513, 200, 8), (2049, 80, 16)):
            x = rb[:n].contiguous()
            r.set_precision(PREC_BY_NAME["fp32"])
            ref = r.render_rays(x, skts, cyl, n_samples=S, n_importance=N, want_alpha=False)
            r.set_precision(PREC_BY_NAME[prec])
            got = r.render_rays(x, skts, cyl, n_samples=S, n_importance=N, want_alpha=False)
            # one pose per call runs the on-chip forms (no records); the same pose handed over per ray runs the record forms
            per_ray = r.render_rays(x, skts.expand(n, -1, -1, -1).contiguous(), cyl, n_samples=S, n_importance=N, want_alpha=False)
            for form, out in (("on-chip", got), ("records", per_ray)):
                for k in ("rgb_map", "acc_map"):
                    assert torch.isfinite(out[k]).all(), (form, n, S, N, k)
                    err = float((out[k] - ref[k]).abs().max())
                    worst = max(worst, err)
                    assert err <= bound, (prec, form, n, S, N, k, err)
    finally:
        r.close()
    print(f"{prec}: worst |error| vs the fp32 kernel over the odd shapes, both forms {worst:.2e}")


@pytest.mark.parametrize("fc", [False, True])
@pytest.mark.parametrize("prec", ["bf16", "fp16c", "fp32"])
def test_per_ray_poses_equal_the_per_pose_calls(prec, fc):
    """Per-ray skeleton transforms (skts [n,24,4,4], the layout the reference expands them to before the call,
    raycasters.py:361-380): rays of two poses in ONE call, interleaved in blocks of 100, give bitwise what each pose's
    own call gives (fp32) or the same up to the limb masks' sub-2^-24 products (16-bit and compensated modes) -- the kernels
    read the pose of the ray, not of the call.  fc: the same with frame codes and a code index per ray (h36m's network at 64
    samples per ray: the on-chip 16x16x32 kernel with a pose AND a code per ray, pg_evalc2.hip<FC, PP>)."""
    prec = prec if isinstance(prec, str) else str(prec)
    from bench import full_frame_rays
    from posegen_amd import PREC_BY_NAME, surreal_config, synthetic as syn
    from posegen_amd.raycaster import HipRayCaster
    cfg = h36m_config(n_samples=64) if fc else surreal_config()
    c = HipRayCaster.from_weights(cfg, *syn.make_model(cfg, 1), device=DEV, precision=prec)
    r = c.renderer
    rb, skts_a, cyl, *_ = full_frame_rays(128, 128, torch.device(DEV))
    _, _, skts_np = syn.make_pose(2, 5)
    skts_b = torch.tensor(skts_np[1:2], device=DEV)
    n = 3000
    x = rb[4000:4000 + n].contiguous()
    which = (torch.arange(n, device=DEV) // 100) % 2 == 1
    per_ray = torch.where(which[:, None, None, None], skts_b.expand(n, -1, -1, -1), skts_a.expand(n, -1, -1, -1)).contiguous()
    cams = ((torch.arange(n, device=DEV) * 7) % cfg.n_framecodes).float() if fc else None
    if fc:
        cams[3::11] = -1.0          # (some rays on the mean code)
    try:
        r.profile_enable(True)
        r.profile_read_aux()
        both = r.render_rays(x, per_ray, cyl, cams=cams, n_samples=64, n_importance=16, want_alpha=False)
        torch.cuda.synchronize()
        assert r.profile_read_aux()[0] == 0 or prec == "fp32", "a per-ray-pose call at 64 samples per ray needs no per-ray records"
        r.profile_enable(False)
        one_a = r.render_rays(x, skts_a, cyl, cams=cams, n_samples=64, n_importance=16, want_alpha=False)
        one_b = r.render_rays(x, skts_b, cyl, cams=cams, n_samples=64, n_importance=16, want_alpha=False)
    finally:
        r.close()
    # Since round 5 a per-ray-pose call runs the same record-free kernels as a one-pose call (the 16x16x32 kernel's on-chip
    # variant reads the bone rows per ray, pg_evalc2.hip likewise): the same products in the same order.  What still differs
    # between the mixed call and the one-pose calls are the limb masks -- a limb is left out where NO point of a wave / a pass
    # is in range, and in the mixed call the points of a pass see two poses -- i.e. products below 2^-24 of a value that one
    # call forms and the other does not: a few flipped operand roundings in the 16-bit modes.  fp32 has no masks: bitwise.
    tol = {"bf16": 1e-3, "fp16": 2e-4, "fp16c": 2e-5}.get(prec, 0.0)
    for k in ("rgb_map", "acc_map", "disp_map"):
        w = which if both[k].dim() == 1 else which[:, None]
        want = torch.where(w, one_b[k], one_a[k])
        if tol == 0.0:
            assert torch.equal(both[k], want), k
        else:
            solid = (want.abs() < 1e3) if k == "disp_map" else torch.ones_like(want, dtype=torch.bool)
            assert float((both[k] - want)[solid].abs().max()) <= tol, (k, float((both[k] - want)[solid].abs().max()))
    assert float((one_a["rgb_map"] - one_b["rgb_map"]).abs().max()) > 1e-3        # the poses do differ


@pytest.mark.skipif(torch.cuda.device_count() < 2, reason="needs two GPUs (self-arming: runs wherever the box has them)")
def test_two_process_rccl_strong_scaling_equals_the_single_device_frames():
    """BASELINE configs 3 / 5 on real hardware as soon as a box has >= 2 GPUs: `bench.py --gpus 2 --scaling strong`
    as a CHILD process (one process per GPU under torch.distributed.run, backend nccl = RCCL; a process that has
    touched the GPU must not exec) renders 5 culled 128 x 128 frames shared by the two ranks -- frames cut on
    nanmean-group boundaries, one all-gather, compose on every rank -- and reports the sha256 of the assembled frames:
    it must be the single-device render's, byte for byte."""
    import hashlib
    import json
    from bench import strong_workload
    from posegen_amd.raycaster import HipRayCaster
    cmd = [sys.executable, os.path.join(REPO, "bench.py"), "--gpus", "2", "--scaling", "strong", "--frames", "5", "--res", "128",
           "--steps", "2", "--warmup", "1", "--full", "--no-cpu-baseline", "--no-modes", "--no-extras"]
    env = dict(os.environ, HSA_ENABLE_IPC_MODE_LEGACY=os.environ.get("HSA_ENABLE_IPC_MODE_LEGACY", "0"))
    out = subprocess.run(cmd, capture_output=True, text=True, timeout=900, env=env, cwd=REPO)
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-2000:]
    line = json.loads([ln for ln in out.stdout.splitlines() if ln.startswith("{")][-1])
    assert line["n_gpus"] == 2 and line["scaling"] == "strong" and line["value"] > 0
    cfg = surreal_config()
    c = HipRayCaster.from_weights(cfg, *syn.make_model(cfg, 0), device=DEV, precision="bf16")
    c.renderer.set_chunk(cfg.chunk)
    step, _ = strong_workload(c, cfg, 128, 128, 5)
    o = step()
    sha = hashlib.sha256(torch.cat([o[0], o[1], o[2]], -1).float().cpu().numpy().tobytes()).hexdigest()
    assert line["frames_sha256"] == sha, "two ranks reproduce the single-device frames bitwise"
    c.renderer.close()


@pytest.mark.parametrize("prec", ["bf16", "fp16", "fp16c"])
def test_materialised_one_pose_calls_take_the_record_free_kernels(prec):
    """VERDICT r4 #6/#9.  The reference expands ONE pose to one copy per ray (run_nerf.py:63-90, a stride-0 view) and
    `batchify_rays` then does `[i:i+chunk].to('cuda')` (core/trainer.py:70-74), which MATERIALISES it: the caster is
    handed contiguous `skts [n,24,4,4]` / `cyls [n,5]` whose rows are all equal.  Such a call must not fall off the fast
    path: it runs the record-free kernels (no per-ray record launch: `profile_read_aux` counts none, no 8.75 KiB per ray
    through HBM) and gives bitwise what the one-pose call gives."""
    from bench import full_frame_rays
    from posegen_amd import surreal_config, synthetic as syn
    from posegen_amd.raycaster import HipRayCaster
    cfg = surreal_config()
    c = HipRayCaster.from_weights(cfg, *syn.make_model(cfg, 1), device=DEV, precision=prec)
    r = c.renderer
    rb, skts, cyl, rb_cpu, skts_cpu, cyl_cpu = full_frame_rays(128, 128, torch.device(DEV))
    n = 4096                                            # one `chunk` of the reference's batchify_rays
    x = rb_cpu[6000:6000 + n]
    # exactly what trainer.py:70-74 produces: slices of the expanded host tensors, moved (hence copied) to the device
    sk_n = skts_cpu.expand(n, -1, -1, -1)[0:n].to(DEV)
    cy_n = cyl_cpu.expand(n, -1)[0:n].to(DEV)
    assert sk_n.is_contiguous() and sk_n.stride(0) == 384
    kps = torch.zeros(n, 24, 3)
    try:
        r.profile_enable(True)
        r.profile_read(); r.profile_read_aux()
        many = c(x.to(DEV), N_samples=cfg.n_samples, kp_batch=kps, skts=sk_n, cyls=cy_n, bones=kps, N_importance=cfg.n_importance)
        torch.cuda.synchronize()
        launches, _, _ = r.profile_read()
        rec_launches, _ = r.profile_read_aux()
        r.profile_enable(False)
        one = c(x.to(DEV), N_samples=cfg.n_samples, skts=skts, cyls=cyl, N_importance=cfg.n_importance)
    finally:
        r.close()
    assert launches == 2 and rec_launches == 0, (launches, rec_launches)
    for k in ("rgb_map", "acc_map", "disp_map", "rgb0", "acc0", "alpha"):
        assert torch.equal(many[k], one[k]), k
