#!/usr/bin/env python3
"""Time of scoring one validation frame on the device with the upsampling fused into the metrics kernel (pg_frame_metrics_val,
posegen_amd.ValidationScorer) beside today's route to the same sums, and what scoring adds to a validation render.

For a 256 x 256 frame against 512 x 512 images and a 500 x 500 frame against 1000 x 1000 images, a box covering about 60 % of the
full-size frame and the same rectangle as `valid` (random bytes: the kernel's time does not depend on the values), measured in one
process on one device with HIP events around each of --calls calls behind --warmup warm-ups:
  * fused: pg_frame_metrics_val on the low-resolution frame, with `valid` set;
  * today's route: F.interpolate(bilinear, align_corners=False, float32) on the device into a full-size frame, then pg_frame_metrics;
  * pg_frame_metrics alone on a full-size frame (the ratio is reported, it is no condition).
The fused call must take no longer than today's route at either size; the tool says so and exits non-zero if it does.
End to end: 20 frames of 512 x 512 rendered at render_factor = 2 (the synthetic model, bf16) through evaluate_testset, against
the same frames through render_frames_device with a sink that does nothing: wall clock with a synchronisation, the median of --reps
alternating repetitions.  Prints one JSON line; --out writes it to a file.

usage: bench_metrics_val.py [--calls 20] [--warmup 3] [--reps 3] [--out profiles/frame_metrics_val.json]"""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch
import torch.nn.functional as F

from tools.bench_metrics import event_times


def one_size(r, H, W, rf, a):
    from posegen_amd import DeviceImageBank, FrameScorer, ValidationScorer
    dev = torch.device("cuda:0")
    g = torch.Generator(device=dev).manual_seed(H)
    P = H * W
    imgs = torch.randint(0, 256, (2, P, 3), dtype=torch.uint8, device=dev, generator=g)
    masks = torch.randint(0, 2, (2, P, 1), dtype=torch.uint8, device=dev, generator=g)
    bkgds = torch.randint(0, 256, (1, P, 3), dtype=torch.uint8, device=dev, generator=g)
    lo = torch.rand((H // rf, W // rf, 3), device=dev, generator=g)
    cams = np.tile(np.eye(4, dtype=np.float32)[None], (2, 1, 1))
    bank = DeviceImageBank(r, imgs, masks, masks, cams, np.full(2, 500.0, np.float32), (H, W), bkgds=bkgds, bkgd_idxs=np.zeros(2, np.int32))
    side = 0.6 ** 0.5
    bw, bh = int(round(W * side)), int(round(H * side))
    box = ((W - bw) // 2, (H - bh) // 2, (W - bw) // 2 + bw, (H - bh) // 2 + bh)
    val, old = ValidationScorer(bank), FrameScorer(bank)
    fused = event_times(lambda: val.score(0, lo, 1, box, box=box), a.calls, a.warmup)
    fused_sums = val.sums()[0]

    def today():
        full = F.interpolate(lo.permute(2, 0, 1)[None], size=(H, W), mode="bilinear", align_corners=False)[0].permute(1, 2, 0).contiguous()
        old.score(0, full, 1, box)
    route = event_times(today, a.calls, a.warmup)
    route_sums = old.sums()[0]
    full = F.interpolate(lo.permute(2, 0, 1)[None], size=(H, W), mode="bilinear", align_corners=False)[0].permute(1, 2, 0).contiguous()
    alone = event_times(lambda: old.score(0, full, 1, box), a.calls, a.warmup)
    rel = lambda x, y: float(np.max(np.abs(x - y) / np.maximum(1.0, np.abs(y))))
    return {"H": H, "W": W, "lo": [H // rf, W // rf], "box": list(box), "box_share": bw * bh / (H * W), "fused": fused,
            "interpolate_then_pg_frame_metrics": route, "pg_frame_metrics_alone": alone, "fused_over_route": fused["ms_mean"] / route["ms_mean"],
            "fused_over_alone": fused["ms_mean"] / alone["ms_mean"], "fused_vs_route_float32_upsampling_rel": rel(fused_sums[:8], route_sums),
            "valid_equals_box": bool(fused_sums[8] == fused_sums[0])}


def render_with_and_without(a, n_frames=20, H=512, W=512, rf=2):
    from posegen_amd import DeviceImageBank, PREC_BF16, surreal_config, synthetic as syn
    from posegen_amd.evaluate import evaluate_testset
    from posegen_amd.raycaster import HipRayCaster
    from posegen_amd.render import render_frames_device
    dev = torch.device("cuda:0")
    cfg = surreal_config()
    caster = HipRayCaster.from_weights(cfg, *syn.make_model(cfg, 0), device="cuda:0", precision=PREC_BF16)
    _, kps, skts = syn.make_pose(n_frames, 1)
    c2ws, focals = syn.make_camera(n_frames, H, W)
    g = torch.Generator(device=dev).manual_seed(7)
    imgs = torch.randint(0, 256, (n_frames, H * W, 3), dtype=torch.uint8, device=dev, generator=g)
    masks = torch.randint(0, 2, (n_frames, H * W, 1), dtype=torch.uint8, device=dev, generator=g)
    bank = DeviceImageBank(caster.renderer, imgs, masks, masks, c2ws, focals, (H, W))
    kw = {"ray_caster": caster, "N_importance": cfg.n_importance, "N_samples": cfg.n_samples, "lindisp": False}
    args = (torch.tensor(c2ws), (H, W, focals), 4096 * 8, kw)
    rkw = dict(kp=torch.tensor(kps), skts=torch.tensor(skts).to(dev), white_bkgd=True, ext_scale=cfg.ext_scale)

    def timed(fn):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = fn()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3, out

    plain = lambda: render_frames_device(*args, render_factor=rf, frame_sink=lambda k, rgb, disp, acc: None, **rkw)
    scored = lambda: evaluate_testset(*args, bank, np.arange(n_frames), render_factor=rf, **rkw)
    timed(plain), timed(scored)
    t_plain, t_scored = [], []
    for _ in range(a.reps):
        t_plain.append(timed(plain)[0])
        ms, scores = timed(scored)
        t_scored.append(ms)
    caster.renderer.close()
    return {"frames": n_frames, "H": H, "W": W, "render_factor": rf, "render_ms": float(np.median(t_plain)),
            "render_and_score_ms": float(np.median(t_scored)), "all_render_ms": t_plain, "all_render_and_score_ms": t_scored,
            "scores": {k: None if v is None else float(v) for k, v in scores.items()},
            "added_ms_per_frame": float(np.median(t_scored) - np.median(t_plain)) / n_frames}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    from posegen_amd import surreal_config
    from posegen_amd.raycaster import HipRenderer
    if not torch.cuda.is_available():
        sys.exit("bench_metrics_val: no HIP device (there is nothing to measure on a CPU)")
    r = HipRenderer(surreal_config(), device="cuda:0")
    sizes = [one_size(r, 512, 512, 2, a), one_size(r, 1000, 1000, 2, a)]
    r.close()
    out = {"sizes": sizes, "render": render_with_and_without(a), "calls": a.calls, "warmup": a.warmup, "reps": a.reps,
           "device": torch.cuda.get_device_name(0)}
    line = json.dumps(out)
    print(line, flush=True)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")
    slow = [s for s in sizes if s["fused_over_route"] > 1]
    if slow:
        sys.exit("bench_metrics_val: pg_frame_metrics_val is slower than F.interpolate + pg_frame_metrics at " +
                 ", ".join(f"{s['H']} x {s['W']} ({s['fused']['ms_mean']:.3f} ms against {s['interpolate_then_pg_frame_metrics']['ms_mean']:.3f} ms)"
                           for s in slow))


if __name__ == "__main__":
    main()
