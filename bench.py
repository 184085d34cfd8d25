#!/usr/bin/env python3
"""Headline benchmark: rendered rays/s of the A-NeRF hot path on MI355X.

    python bench.py --gpus N --steps K --warmup W [--dump-outputs DIR] [--full]

One step = one 512x512 frame per GPU (262 144 rays, 64 coarse + 16 importance samples per
ray -> 144 MLP point evaluations per ray, both nets, synthetic surreal-config weights),
rendered by `pg_render_rays` with the ray batch already resident in HBM.  With N > 1 there is
one process per GPU (`torch.distributed`, backend nccl = RCCL): started by the driver through
`python -m torch.distributed.run`, or -- when `--gpus N` is given without a rendezvous in the
environment -- by this script itself, as a child process launched before anything touches the
GPU.  Every rank renders its own frame (image-parallel, weak scaling) and the frames are
reassembled on every rank by one all-gather of the packed (rgb, disp, acc) maps, fed from
device memory, inside the timed region.  Rank 0 prints ONE JSON line (README / DESIGN.md).

A plain run sets up, warms up, times the K steps and prints the line: the headline, `ms_per_step`, and
  roofline       hipEvent time of the fused embed+MLP kernel in the timed steps vs the MFMA peak
`--dump-outputs DIR` writes what the last timed step computed as DIR/<name>.npy (dump_outputs).
`--full` adds what takes runs or checks of its own (N = 1 only unless noted, each after the timed region):
  strong_scaling the multi-GPU frame path beside the weak headline (any N); frames_sha256 of --scaling strong
  roofline.*     bare-MFMA calibration, limb masks, far_skip_off, folded_pose
  cpu_baseline   the oracle (CPU port of the reference path) on a bounded sample, config 2, and `parity` on it
  cpu_baselines  the same for config 1 (128x128, 32 samples per ray)
  host_to_host   SURVEY 8(d)'s frame metric: poses on host -> frames on host through render_path
  workloads      BASELINE config 4 (h36m: 128+16 samples, frame codes) on one 512x512 frame
  modes          the other precision modes on the headline workload (and north_star_mode)
  train_step     the training step in both training precisions
the --no-* switches leave parts of it out.
`--dry-run` replaces the renderer by a stub and the backend by gloo: the launch / barrier /
max-over-ranks / gather / JSON plumbing on CPU (tests/test_host_logic.py).
"""
from __future__ import annotations

import argparse
import json
import os
import socket
import subprocess
import sys
import time

REPO = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, REPO)

PEAK_TFLOPS = {"bf16": 2500.0, "fp16": 2500.0, "fp32": 157.3, "bf16x3": 2500.0, "fp16x3": 2500.0, "fp16c": 2500.0, "fp16m": 2500.0}
METRIC = "rendered rays/sec (512x512, 64 samples/ray)"


def parse_args(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--prec", default="bf16")
    ap.add_argument("--res", type=int, default=512)
    ap.add_argument("--cpu-rays", type=int, default=8192)
    ap.add_argument("--no-cpu-baseline", action="store_true")
    ap.add_argument("--no-modes", action="store_true", help="skip the per-precision side measurements")
    ap.add_argument("--no-extras", action="store_true", help="skip host_to_host / workloads / cpu_baselines")
    ap.add_argument("--scaling", choices=("weak", "strong"), default="weak",
                    help="weak: one all-hit frame per GPU per step (the headline); strong: --frames culled frames per step "
                         "shared by all GPUs through dist.render_frames_distributed (the GAN loop's call pattern)")
    ap.add_argument("--frames", type=int, default=20, help="frames per step of --scaling strong (run_gan.py:104: rpi = 20)")
    ap.add_argument("--no-strong", action="store_true", help="skip the strong-scaling side measurement of a --full run")
    ap.add_argument("--dry-run", action="store_true", help="stub renderer on CPU, gloo backend (plumbing test)")
    ap.add_argument("--full", action="store_true",
                    help="also the side measurements and checks (strong scaling, calibration, CPU baselines, parity, modes, "
                         "other workloads, training step); a plain run times the steps only")
    ap.add_argument("--dump-outputs", metavar="DIR", default=None,
                    help="write the arrays the last timed step returned as DIR/<name>.npy (float32, at most 64 MB in all)")
    a = ap.parse_args(argv)
    if a.steps < 1 or a.warmup < 0:
        ap.error("--steps must be >= 1 and --warmup >= 0")
    if a.dump_outputs is not None:
        a.dump_outputs = os.path.abspath(a.dump_outputs)
    return a


DUMP_BYTES = 60 << 20       # --dump-outputs: budget of all arrays together (the .npy headers stay well inside 64 MB)


def dump_outputs(d, arrays):
    """--dump-outputs: each array as d/<name>.npy, float32 (float64 stays float64), C order.  An array larger than its
    equal share of DUMP_BYTES is cut to a sample of its rows (rows = the last axis' entries), the same rows in every run
    with the same arguments (seeded permutation, sorted)."""
    import numpy as np
    import torch
    os.makedirs(d, exist_ok=True)
    share = DUMP_BYTES // max(len(arrays), 1)
    for name, x in arrays.items():
        x = x.detach().cpu().numpy() if torch.is_tensor(x) else np.asarray(x)
        x = np.ascontiguousarray(x, dtype=np.float64 if x.dtype == np.float64 else np.float32)
        if x.nbytes > share:
            rows = x.reshape(-1, x.shape[-1] if x.ndim > 1 else 1)
            keep = share // (rows.shape[1] * x.itemsize)
            x = np.ascontiguousarray(rows[np.sort(np.random.default_rng(0).permutation(rows.shape[0])[:keep])])
        np.save(os.path.join(d, f"{name}.npy"), x)


def self_launch(a) -> int:
    """`python bench.py --gpus N` outside a rendezvous: start one process per GPU as a CHILD
    (nothing in this process has touched the GPU) and relay rank 0's JSON line."""
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        port = s.getsockname()[1]
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", f"--nproc-per-node={a.gpus}",
           "--master-addr", "127.0.0.1", "--master-port", str(port), os.path.abspath(__file__)] + sys.argv[1:]
    env = dict(os.environ, HSA_ENABLE_IPC_MODE_LEGACY=os.environ.get("HSA_ENABLE_IPC_MODE_LEGACY", "0"))
    out = subprocess.run(cmd, env=env, stdout=subprocess.PIPE, text=True)
    line = None
    for ln in out.stdout.splitlines():
        if ln.startswith("{") and '"metric"' in ln:
            line = ln
        else:
            print(ln, file=sys.stderr)
    if out.returncode != 0 or line is None:
        print(f"bench.py: the {a.gpus}-process run failed (exit code {out.returncode})", file=sys.stderr)
        return out.returncode or 1
    print(line)
    return 0


def full_frame_rays(H, W, device, cfg=None, sigma=0.2):
    """All H*W rays of the synthetic camera, cylinder radius 2.5 so that every ray hits
    (SURVEY.md 8(d) 'full' variant).  Ray formula of the reference's get_rays.  sigma: spread of the pose's joint
    angles (0.2 = the headline pose of SURVEY.md 8(d))."""
    import torch
    from posegen_amd import synthetic as syn
    from posegen_amd.skeleton import get_kp_bounding_cylinder
    _, kps, skts = syn.make_pose(1, 1, sigma=sigma)
    c2ws, focals = syn.make_camera(1, H, W)
    c2w = torch.tensor(c2ws[0])
    f = float(focals[0])
    col = torch.arange(W, dtype=torch.float32)[None, :].expand(H, W)
    row = torch.arange(H, dtype=torch.float32)[:, None].expand(H, W)
    dirs = torch.stack([(col - W * 0.5) / f, -(row - H * 0.5) / f, -torch.ones(H, W)], -1)
    rd = torch.sum(dirs[..., None, :] * c2w[:3, :3], -1).reshape(-1, 3)
    ro = c2w[:3, -1].expand(rd.shape)
    vd = rd / torch.norm(rd, dim=-1, keepdim=True)
    n = rd.shape[0]
    rb = torch.cat([ro, rd, torch.zeros(n, 1), torch.ones(n, 1), vd], -1).contiguous()
    cyl = torch.tensor(get_kp_bounding_cylinder(kps, ext_scale=0.001), dtype=torch.float32)
    cyl[:, 2] = 2.5
    return rb.to(device), torch.tensor(skts).to(device), cyl.to(device), rb, torch.tensor(skts), cyl


def cpu_baseline(rb_cpu, skts_cpu, cyl_cpu, cfg, model, n_rays, what):
    """The oracle (CPU port of the reference path) timed on the host cores, on a bounded
    sample of the workload `what`."""
    import torch
    from oracle import anerf_oracle as orc
    wc, wf, tv, td = model
    ocfg = orc.OracleConfig(tau_v=tv, tau_d=td)
    tw = lambda w: {k: torch.tensor(v) for k, v in w.items()}
    # a 1-GPU box owns a 16-core share of its host; more threads than that only oversubscribe
    cores = min(os.cpu_count() or 1, 16)
    torch.set_num_threads(cores)
    n = rb_cpu.shape[0]
    n_rays = min(n_rays, n)
    start = min((n // 2 // 512) * 512 + 128, n - n_rays)     # rows through the body
    sel = torch.arange(start, start + n_rays)
    sample = rb_cpu[sel]
    with torch.no_grad():
        orc.render_rays(sample[:64], skts_cpu, cyl_cpu, ocfg, tw(wc), tw(wf), cfg.n_samples, cfg.n_importance)
        t0 = time.time()
        ref = orc.render_rays(sample, skts_cpu, cyl_cpu, ocfg, tw(wc), tw(wf), cfg.n_samples, cfg.n_importance)
        dt = time.time() - t0
    return {"value": n_rays / dt, "unit": "rays/s", "cores": cores, "kind": "port",
            "sample": f"{n_rays} consecutive rays of {what}, one oracle call, "
                      f"torch {torch.__version__} CPU fp32, {cores} threads, {dt:.1f} s"}, sel, ref


def cpu_train_baseline(rb_cpu, skts_cpu, cyl_cpu, cfg, model, n_rays=512):
    """The oracle under torch autograd (the reference's training step restated on the CPU: forward, the Trainer's MSE
    loss on both maps, loss.backward()) timed on the host cores on a bounded batch."""
    import torch
    from oracle import anerf_oracle as orc
    wc, wf, tv, td = model
    ocfg = orc.OracleConfig(tau_v=tv, tau_d=td)
    cores = min(os.cpu_count() or 1, 16)
    torch.set_num_threads(cores)
    sel = torch.linspace(0, rb_cpu.shape[0] - 1, n_rays).long()
    sample = rb_cpu[sel]
    target = torch.rand(n_rays, 3)
    tw = lambda w: {k: torch.tensor(v, requires_grad=True) for k, v in w.items()}
    dt = 0.0
    for rep in range(2):            # the first repetition warms the allocator up
        a, b = tw(wc), tw(wf)
        t0 = time.time()
        out = orc.render_rays(sample, skts_cpu, cyl_cpu, ocfg, a, b, cfg.n_samples, cfg.n_importance)
        loss = torch.mean((out["rgb_map"] + (1. - out["acc_map"])[..., None] - target) ** 2) \
            + torch.mean((out["rgb0"] + (1. - out["acc0"])[..., None] - target) ** 2)
        loss.backward()
        dt = time.time() - t0
    return {"value": n_rays / dt, "unit": "rays/s", "cores": cores, "kind": "port",
            "sample": f"{n_rays} rays of the training batch, oracle forward + loss + backward under torch autograd, "
                      f"torch {torch.__version__} CPU fp32, {cores} threads, {dt:.1f} s"}


def timed_rays(r, dev, rb, skts, cyl, cfg, steps, cams=None):
    """(rays/s, ms/frame, kernel TFLOP/s on algorithmic flops) of `steps` render_rays calls."""
    import torch
    # one untimed call at full size: workspaces and the per-ray record buffer are sized by the first call
    r.render_rays(rb, skts, cyl, cams=cams, n_samples=cfg.n_samples, n_importance=cfg.n_importance, want_alpha=False)
    torch.cuda.synchronize(dev)
    r.profile_enable(True)
    r.profile_read()
    t0 = time.perf_counter()
    for _ in range(steps):
        r.render_rays(rb, skts, cyl, cams=cams, n_samples=cfg.n_samples, n_importance=cfg.n_importance, want_alpha=False)
    torch.cuda.synchronize(dev)
    dt = time.perf_counter() - t0
    launches, ms, pts = r.profile_read()
    r.profile_enable(False)
    tf = pts * cfg.flops_per_point() / (ms * 1e-3) / 1e12 if ms > 0 else 0.0
    return rb.shape[0] * steps / dt, dt / steps * 1e3, tf, ms / max(launches, 1)


def host_to_host(caster, cfg, dev, H, W, frames=4, all_hit=False):
    """pose tensors on host -> rgb/disp/acc frames on host, reference bbox cull.  all_hit: the
    headline workload's cylinder (radius 2.5: every ray hits, the box is the whole frame up to the excluded
    `br` row / column) instead of the poses' own bounding cylinders."""
    import torch
    from posegen_amd import synthetic as syn
    from posegen_amd.render import render_path
    from posegen_amd.skeleton import get_kp_bounding_cylinder
    _, kps, skts = syn.make_pose(frames, 1)
    c2ws, focals = syn.make_camera(frames, H, W)
    cyls = None
    if all_hit:
        cyls = torch.tensor(get_kp_bounding_cylinder(kps, ext_scale=0.001), dtype=torch.float32)
        cyls[:, 2] = 2.5
    kps, skts, c2ws = torch.tensor(kps), torch.tensor(skts), torch.tensor(c2ws)
    kw = {"ray_caster": caster, "N_importance": cfg.n_importance, "N_samples": cfg.n_samples, "lindisp": False}
    run = lambda: render_path(c2ws, (H, W, focals), 4096, kw, kp=kps, skts=skts, cyls=cyls, white_bkgd=True, ret_acc=True,
                              ext_scale=cfg.ext_scale)
    out = run()
    n_valid = sum(len(v) for v in out[3])
    torch.cuda.synchronize(dev)
    t0 = time.perf_counter()
    reps = 3
    for _ in range(reps):
        run()
    torch.cuda.synchronize(dev)
    dt = (time.perf_counter() - t0) / reps
    return {"valid_rays_per_s": n_valid / dt, "pixels_per_s": frames * H * W / dt, "ms_per_frame": dt / frames * 1e3,
            "frames": frames, "valid_rays": n_valid,
            # share of the frame inside the boxes: valid_rays_per_s / box_share_of_frame is the rate a whole frame of
            # such rays would show (what `value` counts: all H*W rays)
            "box_share_of_frame": n_valid / float(frames * H * W),
            "what": f"render_path: {frames} poses + cameras on host -> float32 rgb/disp/acc frames {H}x{W} on host, "
                    + ("all-hit cylinder of the headline workload (radius 2.5; rays counted = rays inside the box = the frame "
                       "without its last row and column), chunk 4096, " if all_hit else
                       "reference bounding-cylinder cull (rays counted = rays inside the box), chunk 4096, ") +
                    "includes box projection on the host, per-frame launches and the device->host copies"}


def dry_run_step(n, rank):
    """Stub of one step for --dry-run: a deterministic [n,5] 'frame' without a renderer."""
    import torch
    v = torch.arange(n, dtype=torch.float32)[:, None] * 1e-3 + rank
    return {"rgb_map": v.expand(n, 3), "disp_map": v[:, 0], "acc_map": v[:, 0]}


class _DryRenderer:
    """--dry-run stand-in for HipRenderer on the strong-scaling path: deterministic maps, no GPU."""
    def __init__(self):
        import torch
        self.device = torch.device("cpu")
    def set_chunk(self, c):
        self.chunk = c
    def render_frame_range(self, H, W, focal, c2w, box, skts, cyl, r0, r1, **kw):
        import torch
        i = torch.arange(r0, r1, dtype=torch.float32)
        return torch.cat([torch.stack([i % 3, i % 5, i % 7], -1).reshape(-1) / 8, 1 + i * 0, (i % 2) * 0.5])
    def compose_frame(self, H, W, box, rgb_map, disp_map, acc_map, bg=None, base_bg=0., **kw):
        import torch
        (tlx, tly), (brx, bry) = box
        rgb = torch.full((H, W, 3), float(base_bg)); disp = torch.zeros(H, W, 1); acc = torch.zeros(H, W, 1)
        bh, bw = bry - tly, brx - tlx
        rgb[tly:bry, tlx:brx] = rgb_map.view(bh, bw, 3); disp[tly:bry, tlx:brx] = disp_map.view(bh, bw, 1)
        acc[tly:bry, tlx:brx] = acc_map.view(bh, bw, 1)
        return rgb, disp, acc


class _DryCaster:
    def __init__(self):
        self.renderer = _DryRenderer()
    module = property(lambda self: self)


def train_step_rate(dev, n_rand=4096, steps=5, warmup=2, precision="fp32"):
    """SURVEY 8(f) rank 4, the training step on the HIP path (posegen_amd.train.TrainableRayCaster): N_rand rays of the
    benchmark frame (run_nerf.py:211 default 32*32*4), 64 + 16 samples, jitter + density noise, the Trainer's MSE loss
    on both maps (trainer.py:321-383), loss.backward(), Adam -- time per step and the fp32 GEMM rate it implies."""
    import torch
    from posegen_amd import surreal_config, synthetic as syn
    from posegen_amd.raycaster import HipRayCaster
    from posegen_amd.train import TrainableRayCaster
    cfg = surreal_config()
    c = HipRayCaster.from_weights(cfg, *syn.make_model(cfg, 0), device=dev, precision="bf16")
    m = TrainableRayCaster(c, train_precision=precision)    # (the training step's arithmetic; the rendering precision plays no part)
    m.train()
    rb, skts, cyl, *_ = full_frame_rays(512, 512, dev)
    sel = torch.linspace(0, rb.shape[0] - 1, n_rand, device=dev).long()
    rb = rb[sel].contiguous()
    target = torch.rand(n_rand, 3, device=dev)
    opt = torch.optim.Adam([p for p in m.parameters() if p.requires_grad], lr=5e-4, betas=(0.9, 0.999))

    def step():
        opt.zero_grad()
        out = m(rb, N_samples=cfg.n_samples, skts=skts, cyls=cyl, N_importance=cfg.n_importance, perturb=1., raw_noise_std=1.)
        loss = torch.mean((out["rgb_map"] + (1. - out["acc_map"])[..., None] - target) ** 2) \
            + torch.mean((out["rgb0"] + (1. - out["acc0"])[..., None] - target) ** 2)
        loss.backward()
        opt.step()
        return loss

    for _ in range(warmup):
        step()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(steps):
        loss = step()
    torch.cuda.synchronize()
    ms = (time.perf_counter() - t0) * 1e3 / steps
    pts = n_rand * (2 * cfg.n_samples + cfg.n_importance)
    flop = 3.0 * pts * cfg.flops_per_point()
    # parameters -> the fused inference kernels' packed weights (what a validation render between optimiser steps needs)
    sync = {}
    for route, on_dev in (("device", True), ("host", False)):
        m.sync_inference_weights(on_device=on_dev)
        torch.cuda.synchronize()
        ts = []
        for _ in range(7):          # (median: the first device-side call builds the source maps, an allocator hiccup would dominate a mean of 0.1 ms calls)
            t1 = time.perf_counter()
            m.sync_inference_weights(on_device=on_dev)
            torch.cuda.synchronize()
            ts.append((time.perf_counter() - t1) * 1e3)
        sync[route] = sorted(ts)[len(ts) // 2]
    m.renderer.close()
    peak = PEAK_TFLOPS["fp32" if precision == "fp32" else "bf16"]
    return {"n_rand": n_rand, "ms_per_step": ms, "rays_per_s": n_rand / (ms * 1e-3), "points_per_step": pts,
            "gemm_flop_per_step": flop, "tflops": flop / (ms * 1e-3) / 1e12, "peak_tflops": peak,
            "frac": flop / (ms * 1e-3) / 1e12 / peak, "dtype": "f32" if precision == "fp32" else "bf16", "loss": float(loss.detach()),
            "sync_inference_weights_ms": sync["device"], "sync_inference_weights_host_route_ms": sync["host"],
            "what": "forward with a tape + MSE loss + loss.backward() + Adam on the whole step's wall clock, "
                    + ("fp32 (v_mfma_f32_32x32x2_f32 GEMMs)" if precision == "fp32" else
                       "16-bit training mode (the tape -- embedding rows, activations, their gradients -- stored in bf16, bf16 operands in the large GEMMs on v_mfma_f32_32x32x16_bf16, fp32 accumulate; weights, raw, d_raw and weight gradients fp32)")
                    + ", surreal 64+16, perturb=1, raw_noise_std=1; FLOPs = 3 x the forward MLP "
                    "FLOPs of the step's points (forward, dX and dW GEMMs); embedding and compositing not counted"}


def strong_workload(caster, cfg, H, W, frames, group=None):
    """BASELINE config 5's call pattern: `frames` poses at H x W with the reference's bounding-cylinder cull, one
    camera, white background; one step = one dist.render_frames_distributed call (every rank renders its share
    of the frames' nanmean groups, ONE all-gather, frames composed on every rank).  Returns (step, valid rays)."""
    import torch
    from posegen_amd import synthetic as syn
    from posegen_amd.dist import render_frames_distributed
    _, kps, skts = syn.make_pose(frames, 1)
    c2ws, focals = syn.make_camera(frames, H, W)
    kps, skts, c2ws = torch.tensor(kps), torch.tensor(skts), torch.tensor(c2ws)
    kw = {"ray_caster": caster, "N_importance": cfg.n_importance, "N_samples": cfg.n_samples, "lindisp": False}
    state = {"host_pre_launch_ms": []}

    def step():
        st = {}
        out = render_frames_distributed(c2ws, (H, W, focals), cfg.chunk, kw, group=group, kp=kps, skts=skts,
                                        white_bkgd=True, ext_scale=cfg.ext_scale, stats=st)
        state["valid"] = sum(out[3].counts()) if hasattr(out[3], "counts") else sum(len(v) for v in out[3])
        state["host_pre_launch_ms"].append(st.get("host_pre_launch_ms", 0.0))
        state["host_ms"] = st.get("host_ms", 0.0)
        return out
    return step, state


def main():
    a = parse_args()
    world = int(os.environ.get("WORLD_SIZE", "1"))
    if a.gpus > 1 and "RANK" not in os.environ:
        sys.exit(self_launch(a))
    if a.gpus != world:
        sys.exit(f"bench.py: --gpus {a.gpus} but the rendezvous has WORLD_SIZE={world}")

    import numpy as np
    import torch
    from posegen_amd import PREC_BY_NAME, h36m_config, surreal_config, synthetic as syn
    if a.prec not in PREC_BY_NAME:
        sys.exit(f"bench.py: unknown precision {a.prec!r} (one of {sorted(PREC_BY_NAME)})")
    rank = int(os.environ.get("RANK", "0"))
    local = int(os.environ.get("LOCAL_RANK", "0"))
    dist = None
    if a.dry_run:
        dev = torch.device("cpu")
        if world > 1:
            import torch.distributed as dist
            dist.init_process_group("gloo")
    else:
        dev = torch.device("cuda", local)
        torch.cuda.set_device(dev)
        if world > 1:
            import torch.distributed as dist
            dist.init_process_group("nccl", device_id=dev)

    cfg = surreal_config()
    H = W = a.res
    if a.dry_run:
        n, r, caster = H * W, None, None
    else:
        from posegen_amd.raycaster import HipRayCaster
        model = syn.make_model(cfg, 0)
        caster = HipRayCaster.from_weights(cfg, *model, device=dev, precision=a.prec)
        rb, skts, cyl, rb_cpu, skts_cpu, cyl_cpu = full_frame_rays(H, W, dev)
        n = rb.shape[0]
        r = caster.renderer
        r.set_chunk(cfg.chunk)
    packed = torch.empty(n, 5, device=dev)
    gathered = torch.empty(world * n, 5, device=dev) if world > 1 else None
    strong = a.scaling == "strong"

    def weak_step():
        out = dry_run_step(n, rank) if a.dry_run else r.render_rays(
            rb, skts, cyl, n_samples=cfg.n_samples, n_importance=cfg.n_importance, want_alpha=False)
        if world > 1:           # reassemble the frames of all ranks: one all-gather, device to device
            packed[:, 0:3] = out["rgb_map"]
            packed[:, 3] = out["disp_map"]
            packed[:, 4] = out["acc_map"]
            dist.all_gather_into_tensor(gathered, packed)
        return out

    strong_step, strong_state = strong_workload(_DryCaster() if a.dry_run else caster, cfg, H, W, a.frames)
    step = strong_step if strong else weak_step

    def sync():
        if world > 1:
            dist.barrier()
        if not a.dry_run:
            torch.cuda.synchronize(dev)

    def max_over_ranks(x):
        if world == 1:
            return x
        t = torch.tensor([x], device=dev, dtype=torch.float64)
        dist.all_reduce(t, op=dist.ReduceOp.MAX)
        return float(t.item())

    for _ in range(a.warmup):
        step()
    sync()
    if r is not None:
        r.profile_enable(True)
        r.profile_read()
    t0 = time.perf_counter()
    for _ in range(a.steps):
        out = step()
    sync()
    dt = time.perf_counter() - t0
    launches, k_ms, k_pts = r.profile_read() if r is not None else (0, 0.0, 0)
    aux_n, aux_ms = r.profile_read_aux() if r is not None else (0, 0.0)
    if r is not None:
        r.profile_enable(False)
    dt = max_over_ranks(dt)
    if world > 1 and a.dry_run and not strong:      # the gathered frames are every rank's frame, in rank order
        for k in range(world):
            assert float(gathered[k * n, 0]) == float(k), "all-gather order"
    if a.dump_outputs and rank == 0:
        # what a caller of the timed path received from its last step
        if strong:
            dumped = {"rgb": out[0], "disp": out[1], "acc": out[2], "bboxes": [np.concatenate(b) for b in out[4]]}
        else:
            dumped = {k: out[k] for k in ("rgb_map", "disp_map", "acc_map", "rgb0", "disp0", "acc0") if k in out}
            if world > 1:
                dumped["gathered"] = gathered
        dump_outputs(a.dump_outputs, dumped)

    # Strong scaling beside the weak headline, on every rank (it has a collective): the product's multi-GPU path
    # (dist.render_frames_distributed: plan of nanmean groups, one all-gather, compose) on the GAN loop's call
    # pattern -- `--frames` culled frames per step for ALL GPUs together -- so that a scaling run also says
    # something about load balance.
    side = None
    if a.full and not strong and not a.no_strong:
        strong_step()
        sync()
        reps = 3
        strong_state["host_pre_launch_ms"].clear()
        t1 = time.perf_counter()
        for _ in range(reps):
            strong_step()
        sync()
        sdt = max_over_ranks(time.perf_counter() - t1) / reps
        # the serial host part on an IDLE device (in the back-to-back loop above the boxes' copy-back also waits for the
        # previous step's frames): device idle before each of three more steps
        strong_state["host_pre_launch_ms"].clear()
        for _ in range(3):
            sync()
            strong_step()
        sync()
        pre = sorted(strong_state["host_pre_launch_ms"])
        host_serial = max_over_ranks(pre[len(pre) // 2] if pre else 0.0)
        from posegen_amd.dist import plan_tasks
        side = {"scaling": "strong", "frames_per_step": a.frames, "valid_rays_per_step": strong_state["valid"],
                "rays_per_s": strong_state["valid"] / sdt, "ms_per_step": sdt * 1e3, "ms_per_frame": sdt * 1e3 / a.frames,
                "n_gpus": world,
                # host work of a step that no GPU overlaps (call entry -> first render launch on an idle device: device
                # boxes with their 16-byte-per-frame copy back, the plan, the pose upload): what every rank repeats,
                # i.e. the serial term of the 8-GPU bound T1 / (T1 / 8 + host) of DESIGN.md 4; median of three steps,
                # max over ranks
                "host_serial_ms_per_step": host_serial, "host_enqueue_ms_per_step": strong_state.get("host_ms", 0.0),
                "what": f"dist.render_frames_distributed: {a.frames} poses at {H}x{W}, reference bounding-cylinder cull, "
                        f"nanmean groups of {cfg.chunk} rays planned over {world} rank(s), one all-gather of the packed maps "
                        "inside the timed region, frames composed on every rank (device resident); rays counted = rays "
                        "inside the boxes, whole job"}

    frames_sha = None
    if a.full and strong and rank == 0 and out is not None and out[0] is not None:
        # checksum of the last step's assembled frames: a multi-GPU run must reproduce the single-device bytes
        # (groups stay whole) -- tests/test_gpu_configs.py compares the two
        import hashlib
        frames_sha = hashlib.sha256(torch.cat([out[0], out[1], out[2]], -1).float().cpu().numpy().tobytes()).hexdigest()

    if rank != 0:
        if world > 1:
            dist.barrier()
            dist.destroy_process_group()
        return

    flops_pt = cfg.flops_per_point()
    rays_s = (strong_state["valid"] if strong else world * n) * a.steps / dt
    peak = PEAK_TFLOPS[a.prec]
    k_tflops = k_pts * flops_pt / (k_ms * 1e-3) / 1e12 if k_ms > 0 else 0.0
    kernel = {"bf16": "eval16r_kernel", "fp16": "eval16r_kernel", "fp16c": "evalc2_kernel"}.get(a.prec, "eval32_kernel")
    result = {
        "metric": METRIC,
        "value": rays_s, "unit": "rays/s", "n_gpus": world, "steps": a.steps, "warmup": a.warmup,
        "ms_per_step": dt / a.steps * 1e3, "higher_is_better": True, "scaling": a.scaling,
        "vs_baseline": None, "dtype": a.prec, "data": "synthetic (dry run: stub renderer, no GPU)" if a.dry_run else "synthetic",
        "config": ({"workload": f"surreal {H}x{W}, {a.frames} culled frames per step for all GPUs together "
                                f"({strong_state['valid']} rays inside the boxes), {cfg.n_samples} coarse + {cfg.n_importance} "
                                f"importance samples/ray = {cfg.evals_per_ray()} MLP evals/ray, dist.render_frames_distributed "
                                "(nanmean groups planned over the ranks, one all-gather, frames composed on every rank)",
                    "frames_per_step": a.frames, "parallelism": f"ray-group-parallel x{world}" if world > 1 else "single GPU",
                    "flop_per_ray": flops_pt * cfg.evals_per_ray()} if strong else
                   {"workload": f"surreal {H}x{W} full frame per GPU ({n} rays, all rays hit: cylinder radius 2.5), "
                                f"{cfg.n_samples} coarse + {cfg.n_importance} importance samples/ray = "
                                f"{cfg.evals_per_ray()} MLP evals/ray (coarse + fine net), seeded synthetic weights/pose",
                    "frames_per_step_per_gpu": 1, "parallelism": f"image-parallel x{world}" if world > 1 else "single GPU",
                    "flop_per_ray": flops_pt * cfg.evals_per_ray()}),
        "roofline": {"bound": "mfma", "kernel": f"{kernel} (fused embed+MLP)",
                     "achieved": k_tflops, "peak": peak, "unit": "TFLOP/s", "frac": k_tflops / peak,
                     "traffic": None, "launches": launches, "avg_launch_ms": k_ms / max(launches, 1),
                     "points_per_launch": k_pts / max(launches, 1), "flop_per_point": flops_pt,
                     "end_to_end_frac": rays_s / world * flops_pt * cfg.evals_per_ray() / 1e12 / peak,
                     # the path's ALGORITHMIC HBM bytes are 44 B in + 20 B out per ray; the kernels'
                     # counter traffic (`traffic`, per eval launch) is mostly the raw / z intermediates between them
                     "algorithmic_bytes_per_ray": 64, "algorithmic_bytes_per_frame": 64 * n},
    }
    if aux_n:
        # the per-ray record kernel in front of every fused launch (pg_rayrec.hip: what depends on the ray only, once
        # per ray; HBM-bound): its time is part of ms_per_step, not of the fused kernel's `achieved`
        result["roofline"]["record_kernel"] = {"kernel": "ray_records_kernel", "launches": aux_n, "avg_launch_ms": aux_ms / aux_n,
                                               "bytes_written_per_launch": (8192 + 768) * n,
                                               "frac_incl_records": k_pts * flops_pt / ((k_ms + aux_ms) * 1e-3) / 1e12 / peak}
    if side is not None:
        result["strong_scaling"] = side
    if frames_sha is not None:
        result["frames_sha256"] = frames_sha
    if a.dry_run:
        print(json.dumps(result))
        if world > 1:
            dist.barrier()
            dist.destroy_process_group()
        return

    # the peak re-derived on this box: CUs x 4 SIMDs x 1024 bf16 MFMA FLOP/clk x max clock
    di = r.device_info()
    if di["clock_khz"] > 0 and a.prec != "fp32":
        result["roofline"]["peak_derived"] = di["n_cu"] * 4 * 1024 * di["clock_khz"] * 1e3 / 1e12
        result["roofline"]["peak_derived_from"] = f"{di['n_cu']} CUs x 4096 FLOP/clk x {di['clock_khz'] / 1e6:.2f} GHz (hipDeviceProp)"
    # `achieved` counts the ALGORITHMIC flops of the reference network.  The kernels ISSUE fewer: feature_linear
    # is folded into the view layer, the view-direction input is factorised over rays (both exact in real arithmetic), and the
    # limbs of the cutoff embedding that are out of range of a wave / a pass are left out (products below 2^-24 of a value:
    # DESIGN.md 2.1) -- which depends on the pose, tau and the cutoff.  So the line carries its conditions:
    #   issued_frac       MFMA FLOPs really issued per launch (SQ_INSTS_MFMA of the committed PMC pass of this workload)
    #                     over the algorithmic FLOPs
    #   limb_masks        what the kernel itself counts on the coarse launch of this frame (pg_stage_eval, stage 97)
    #   far_skip_off      the same steps with pg_set_far_skip(0): every limb computed for every point
    #   folded_pose       the same frame size with the pose's joint angles drawn three times as wide (limbs folded towards
    #                     the trunk: more limbs in range of a point)
    mfma_flop = 4096 if a.prec == "fp32" else 16384 if a.prec in ("bf16", "fp16", "fp16c") else 32768
    for tname in (f"r5_{a.prec}_traffic.json", f"r4_{a.prec}_traffic.json"):
        tpath = os.path.join(REPO, "profiles", tname)
        if H == 512 and os.path.exists(tpath):
            tj = json.load(open(tpath))
            ins = tj.get("counters_per_launch", {}).get("SQ_INSTS_MFMA")
            if ins:
                per = 16384 if ("eval16r" in tj["kernel"] or "evalc2" in tj["kernel"]) else 32768
                result["roofline"]["issued_frac"] = ins * per / (k_pts / max(launches, 1) * flops_pt)
                result["roofline"]["issued_from"] = (f"SQ_INSTS_MFMA {ins:.4g} per launch x {per} FLOP (profiles/{tname}, commit "
                                                     f"{tj.get('commit', 'unrecorded')}) over points per launch x {flops_pt} algorithmic FLOP")
            break
    if a.full and a.prec in ("bf16", "fp16", "fp16c") and world == 1 and not a.no_extras:    # (not in the profiled command: their launches carry the headline kernel's name)
        nf, z = r.stage_sample_coarse(rb, cyl, cfg.n_samples)
        result["roofline"]["limb_masks"] = dict(r.limb_skip_stats(0, rb, z, skts),
                                                what=f"coarse launch of the benchmark frame ({cfg.n_samples} samples per ray), counted by the kernel: "
                                                     "limbs_left_out_frac of the (wave / 16-point column tile, limb) pairs skip embedding and MFMAs, "
                                                     "limbs_left_out_of_whole_passes_frac of the (pass, limb) pairs also skip the weight fetch; "
                                                     f"tau = {float(model[2]):.1f}, cutoff 0.5")
        r.set_far_skip(False)
        _, _, tf_off, kms_off = timed_rays(r, dev, rb, skts, cyl, cfg, max(2, a.steps // 4))
        r.set_far_skip(True)
        result["roofline"]["far_skip_off"] = {"avg_launch_ms": kms_off, "frac": tf_off / peak,
                                              "what": "the same frame with pg_set_far_skip(0): no limb masks"}
        rb2, skts2, cyl2, *_ = full_frame_rays(H, W, dev, sigma=0.6)
        rs2, msf2, tf2, kms2 = timed_rays(r, dev, rb2, skts2, cyl2, cfg, max(2, a.steps // 4))
        nf2, z2 = r.stage_sample_coarse(rb2, cyl2, cfg.n_samples)
        result["roofline"]["folded_pose"] = {"rays_per_s": rs2, "ms_per_frame": msf2, "avg_launch_ms": kms2, "frac": tf2 / peak,
                                             "limb_masks": r.limb_skip_stats(0, rb2, z2, skts2),
                                             "what": "same frame size and camera, joint angles ~ N(0, 0.6^2) instead of N(0, 0.2^2)"}
    q = r.query()
    result["roofline"]["program_flop_per_point"] = q["mfma_per_group"] * (4096 if a.prec == "fp32" else 32768) / 32.0
    result["roofline"]["program_note"] = "the kernel's program with every limb in range, in FLOPs per point: an upper bound of what a launch issues"

    # What this box SUSTAINS on bare 32x32x16 MFMAs (register operands, 2 waves per SIMD on every CU,
    # nothing else in the loop, one >= 20 ms launch): `peak` stays the nominal dense figure, this says how
    # much of the gap is the chip's clock management under MFMA load rather than the kernel's stalls.
    if a.full and a.prec != "fp32" and world == 1:
        # the shape of the kernel that ran: 16x16x32 for the 16-bit modes (pg_eval16r.hip), 32x32x16 for the compensated one
        small = 2 if a.prec in ("bf16", "fp16", "fp16c") else 0
        shape = "16x16x32" if small else "32x32x16"
        f16 = a.prec != "bf16"
        cal = r.calibrate_mfma(f16=f16, lds_fed=small)
        result["roofline"]["sustained_mfma_tflops"] = cal["tflops"]
        result["roofline"]["sustained_mfma_from"] = (f"bare v_mfma_f32_{shape}_{'f16' if f16 else 'bf16'} loop (the kernel's MFMA shape), "
                                                     f"{cal['ms']:.1f} ms launch on this box (pg_calibrate_mfma)")
        if "issued_frac" in result["roofline"]:
            result["roofline"]["issued_frac_of_sustained"] = k_tflops * result["roofline"]["issued_frac"] / cal["tflops"]
        # the same loop with the A operand of every MFMA read from LDS (one ds_read_b128 per MFMA and wave):
        # the ceiling of the kernels' structure -- weight fragments from the LDS ring
        cal2 = r.calibrate_mfma(f16=f16, lds_fed=small | 1)
        result["roofline"]["sustained_mfma_lds_fed_tflops"] = cal2["tflops"]
        if "issued_frac" in result["roofline"]:
            result["roofline"]["issued_frac_of_lds_fed"] = k_tflops * result["roofline"]["issued_frac"] / cal2["tflops"]
        if small:       # what the chip sustains on the other shape (round 2's kernel): the reason for the re-layout
            cal3 = r.calibrate_mfma(f16=f16, lds_fed=0)
            result["roofline"]["sustained_mfma_32x32x16_tflops"] = cal3["tflops"]

    # HBM traffic of the dominant kernel comes from separate rocprofv3 --pmc passes of this
    # same command (FETCH_SIZE x2 gfx950 correction + WRITE_SIZE); bench.py cannot run the
    # profiler on itself, so the committed measurement of the same build is attached.
    alg_bytes = 20 * k_pts / max(launches, 1)       # z in 4 B/point + raw out 16 B/point
    for tname in (f"r5_{a.prec}_traffic.json", f"r4_{a.prec}_traffic.json", f"r3_{a.prec}_traffic.json", f"r2_{a.prec}_traffic.json", "r1_traffic.json"):
        tpath = os.path.join(REPO, "profiles", tname)
        if H == 512 and os.path.exists(tpath) and (a.prec == "bf16" or not tname.startswith("r1_")):
            tj = json.load(open(tpath))
            result["roofline"]["traffic"] = tj["hbm_bytes"]
            result["roofline"]["traffic_unit"] = f"bytes per launch (PMC, profiles/{tname})"
            # NOT measured by this run: the rocprofv3 --pmc passes of the build named here, taken on the builder's box
            result["roofline"]["traffic_from"] = {"file": f"profiles/{tname}", "commit": tj.get("commit", "unrecorded (round of the file name)"),
                                                  "box": tj.get("box", "a one-GPU MI355X box of the builder's pool"),
                                                  "note": "attached from the committed profile of that build, not a measurement of this run"}
            # what ONE eval launch has to move given the kernel split: z in 4 B/point + raw out 16 B/point
            result["roofline"]["intermediate_bytes_per_launch"] = tj.get("algorithmic_bytes", alg_bytes)
            # against SURVEY 8(d)'s figure for the PATH (64 B/ray): a frame is 2 eval + 2 composite + 1 sampling
            # launch; the composite launches re-read what the eval launches wrote
            per_frame = tj.get("hbm_bytes_per_frame", 2 * tj["hbm_bytes"] + 2 * tj.get("composite_hbm_bytes", 0.95 * tj["hbm_bytes"]))
            result["roofline"]["traffic_per_frame"] = per_frame
            result["roofline"]["traffic_ratio"] = per_frame / (64.0 * n)
            break

    sel = ref = None
    if a.full and world == 1 and not a.no_cpu_baseline:
        base, sel, ref = cpu_baseline(rb_cpu, skts_cpu, cyl_cpu, cfg, model, a.cpu_rays, f"the same {H}x{W} frame")
        result["cpu_baseline"] = base
        # parity of the measured configuration on the CPU-baseline sample
        got = r.render_rays(rb[sel.to(dev)], skts, cyl, n_samples=cfg.n_samples, n_importance=cfg.n_importance)
        err = {k: float((got[k].cpu() - ref[k]).abs().max()) for k in ("rgb_map", "acc_map")}
        solid = ref["acc_map"] > 1e-3        # disparity of an empty ray is 1/(0/0): noise in the reference too
        err["disp_map(acc>1e-3)"] = float((got["disp_map"].cpu() - ref["disp_map"])[solid].abs().max()) if solid.any() else 0.0
        mse = float(((got["rgb_map"].cpu() - ref["rgb_map"]) ** 2).mean())
        result["parity"] = {"vs": "oracle (fp32 CPU port pinned to the reference's golden vectors)", "rays": int(len(sel)),
                            "max_abs": err, "rgb_rmse": mse ** 0.5, "rgb_mse": mse,
                            "rgb_psnr_db": -10 * np.log10(max(mse, 1e-30))}

    if a.full and world == 1 and not a.no_modes:
        modes = {}
        for name in ("fp16m", "fp16c", "fp16", "bf16x3", "fp32"):
            if name == a.prec or name not in PREC_BY_NAME:
                continue
            r.set_precision(name)
            steps = 1 if name == "fp32" else 3
            rs, msf, tf, _ = timed_rays(r, dev, rb, skts, cyl, cfg, steps)
            m = {"rays_per_s": rs, "ms_per_frame": msf, "kernel_tflops": tf, "peak_tflops": PEAK_TFLOPS[name],
                 "frac": tf / PEAK_TFLOPS[name]}
            if sel is not None:
                got = r.render_rays(rb[sel.to(dev)], skts, cyl)
                m["max_abs_rgb_vs_oracle"] = float((got["rgb_map"].cpu() - ref["rgb_map"]).abs().max())
                m["max_abs_acc_vs_oracle"] = float((got["acc_map"].cpu() - ref["acc_map"]).abs().max())
                solid_m = ref["acc_map"] > 1e-3
                m["max_abs_disp_vs_oracle"] = float((got["disp_map"].cpu() - ref["disp_map"])[solid_m].abs().max()) if solid_m.any() else 0.0
                mse_m = float(((got["rgb_map"].cpu() - ref["rgb_map"]) ** 2).mean())
                m["rgb_mse_vs_oracle"] = mse_m
                m["rgb_psnr_db_vs_oracle"] = -10 * np.log10(max(mse_m, 1e-30))
            modes[name] = m
        r.set_precision(a.prec)
        result["modes"] = modes
        # north_star asks for "output within 1e-4 of reference" AND ">= 50 % MFMA roofline": the fastest mode whose
        # max-abs error of rgb, acc and disp (solid rays) against the pinned oracle is <= 1e-4 on the parity sample,
        # next to the bf16 headline (BASELINE config 2 names "bf16 MLP"; bf16 itself is ~2e-3 from the reference)
        if sel is not None:
            cands = {a.prec: {"rays_per_s": rays_s, "frac": result["roofline"]["frac"],
                              "max_abs_rgb_vs_oracle": result["parity"]["max_abs"]["rgb_map"],
                              "max_abs_acc_vs_oracle": result["parity"]["max_abs"]["acc_map"],
                              "max_abs_disp_vs_oracle": result["parity"]["max_abs"]["disp_map(acc>1e-3)"]}}
            cands.update(modes)
            ok = {k: v for k, v in cands.items() if max(v["max_abs_rgb_vs_oracle"], v["max_abs_acc_vs_oracle"],
                                                         v["max_abs_disp_vs_oracle"]) <= 1e-4}
            if ok:
                best = max(ok, key=lambda k: ok[k]["rays_per_s"])
                result["north_star_mode"] = {
                    "mode": best, "rays_per_s": ok[best]["rays_per_s"], "frac": ok[best]["frac"], "tolerance": 1e-4,
                    "max_abs": {k: ok[best][f"max_abs_{k}_vs_oracle"] for k in ("rgb", "acc", "disp")},
                    "rays_in_sample": int(len(sel)),
                    "what": "fastest precision mode within 1e-4 (max-abs rgb / acc / disp of solid rays) of the fp32 oracle on "
                            "the parity sample; frac = fused kernel on algorithmic FLOPs over the 2.5 PFLOP/s dense 16-bit peak"}
            else:
                result["north_star_mode"] = None

    if a.full and world == 1 and not a.no_extras:
        result["host_to_host"] = host_to_host(caster, cfg, dev, H, W)
        # SURVEY 8(d)'s metric on the HEADLINE workload: the same all-hit frame, pose tensors on the host -> float
        # frames on the host through render_path (the cylinder of radius 2.5 projects to the whole frame)
        result["host_to_host_all_hit"] = host_to_host(caster, cfg, dev, H, W, frames=4, all_hit=True)
        # BASELINE config 4: h36m (128 coarse + 16 importance samples, 16-d frame codes), one full frame
        c4 = h36m_config()
        m4 = syn.make_model(c4, 0)
        cast4 = HipRayCaster.from_weights(c4, *m4, device=dev, precision=a.prec)
        cams = (torch.arange(n, device=dev) % c4.n_framecodes).float()
        rs, msf, tf, kms = timed_rays(cast4.renderer, dev, rb, skts, cyl, c4, 2, cams=cams)
        result["workloads"] = {"h36m_512": {
            "workload": f"h36m config, {H}x{W} full frame ({n} rays), {c4.n_samples}+{c4.n_importance} samples/ray = "
                        f"{c4.evals_per_ray()} MLP evals/ray, per-ray frame-code index, view layer K = {c4.ch_view_in}",
            "rays_per_s": rs, "ms_per_frame": msf, "kernel_tflops": tf, "frac": tf / peak, "avg_launch_ms": kms,
            "flop_per_ray": c4.flops_per_point() * c4.evals_per_ray()}}
        if a.prec in ("bf16", "fp16"):      # the two forms of the 16x16x32 kernel on this workload (the default picks by sample count: records here)
            r4 = cast4.renderer
            forms = {}
            for mode in ("records", "always"):
                r4.set_onchip(mode)
                r4.profile_read_aux()
                rs_m, msf_m, tf_m, kms_m = timed_rays(r4, dev, rb, skts, cyl, c4, 2, cams=cams)
                nrec, ms_rec = r4.profile_read_aux()
                forms[mode] = {"rays_per_s": rs_m, "ms_per_frame": msf_m, "frac": tf_m / peak, "avg_launch_ms": kms_m,
                               "record_launches_per_frame": nrec / 2.0, "record_ms_per_frame": ms_rec / 2.0,     # (two profiled frames)
                               "frac_with_record_kernels": (tf_m / peak) * (2 * kms_m) / (2 * kms_m + ms_rec / 2.0)}
            r4.set_onchip("auto")
            result["workloads"]["h36m_512"]["forms"] = {
                "per_ray_records": forms["records"], "on_chip": forms["always"], "default": "per_ray_records (pg_set_onchip AUTO: on chip up to 112 samples per ray)",
                "what": "pg_set_onchip RECORDS / ALWAYS on the same frame: records = 8.75 KiB per ray through HBM and a record launch per eval launch "
                        "(14.7 GB per frame, profiles/r5_h36m_records_traffic.json), on chip = frame-code rows from a host-made table, no records "
                        "(3.7 GB per frame, profiles/r5_h36m_onchip_traffic.json)"}
        if a.prec != "fp16c":       # BASELINE config 4 in the north-star mode as well (no per-ray records since round 5: pg_evalc2.hip)
            cast4.renderer.set_precision("fp16c")
            rs, msf, tf, kms = timed_rays(cast4.renderer, dev, rb, skts, cyl, c4, 1, cams=cams)
            result["workloads"]["h36m_512_fp16c"] = {"rays_per_s": rs, "ms_per_frame": msf, "kernel_tflops": tf, "frac": tf / PEAK_TFLOPS["fp16c"],
                                                     "avg_launch_ms": kms, "what": "the same frame in the compensated-fp16 mode"}
        cast4.renderer.close()
        result["train_step"] = train_step_rate(dev, precision="bf16")
        result["train_step"]["fp32"] = train_step_rate(dev, precision="fp32")
        if not a.no_cpu_baseline:
            result["train_step"]["cpu_baseline"] = cpu_train_baseline(rb_cpu, skts_cpu, cyl_cpu, cfg, model)
        if not a.no_cpu_baseline:   # BASELINE config 1: 128x128, 32 coarse (+16) samples per ray
            c1 = surreal_config(n_samples=32)
            _, _, _, rb1, sk1, cy1 = full_frame_rays(128, 128, "cpu")
            b1, _, _ = cpu_baseline(rb1, sk1, cy1, c1, model, min(a.cpu_rays, 8192), "the 128x128 frame of config 1 (32+16 samples/ray)")
            rs1, msf1, _, _ = timed_rays(r, dev, rb1.to(dev), skts, cyl, c1, 3)
            result["cpu_baselines"] = {"config1_128x128x32": dict(b1, gpu_rays_per_s=rs1, gpu_ms_per_frame=msf1)}

    print(json.dumps(result))
    if world > 1:
        dist.barrier()
        dist.destroy_process_group()


if __name__ == "__main__":
    main()
