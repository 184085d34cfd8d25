#!/usr/bin/env python3
"""Time of scoring one rendered frame on the device (pg_frame_metrics, posegen_amd.FrameScorer) beside the two other ways to the
same scores, and what scoring adds to a render.

For a 512 x 512 and a 1000 x 1000 frame with a box covering about 60 % of it (random image, mask, background and frame bytes: the
kernel's time does not depend on the values), measured in one process on one device:
  * ms per pg_frame_metrics call: HIP events around each of --calls calls behind --warmup warm-ups (mean and least), and around
    the whole loop;
  * the torch route on the same device: the vendored formula as five F.conv2d calls (float32, the 2-D window, groups = 3) plus the
    masked sums, on the same box, timed the same way;
  * the numpy route on the host: the frame downloaded, then tests/metrics_ref.py (float64) -- what a caller does today;
  * HBM bytes per frame from the shapes: what the tiles stage (inputs with their halo), the unique bytes of the box, and the slots;
  * a 20-frame evaluate_frames call (512 x 512, the synthetic model, bf16) against the same frames through render_frames_device
    with a sink that does nothing: wall clock with a synchronisation, the median of --reps alternating repetitions.
The kernel must not be slower than the torch route at either size; the tool says so and exits non-zero if it is.
Prints one JSON line; --out writes it to a file.

usage: bench_metrics.py [--calls 20] [--warmup 3] [--reps 3] [--out profiles/frame_metrics.json]"""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch
import torch.nn.functional as F

TILE, HALO = 32, 10
C1, C2 = 1e-4, 9e-4


def event_times(fn, calls, warmup):
    """ms of each of `calls` calls of fn by an event pair, and of the loop as a whole per call"""
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    pairs = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(calls)]
    l0, l1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    l0.record()
    for e0, e1 in pairs:
        e0.record()
        fn()
        e1.record()
    l1.record()
    torch.cuda.synchronize()
    per = [e0.elapsed_time(e1) for e0, e1 in pairs]
    return {"ms_mean": float(np.mean(per)), "ms_min": float(np.min(per)), "ms_loop_per_call": l0.elapsed_time(l1) / calls}


def torch_scores(rgb, img, mask, bkgd, box, window):
    """the eight sums by torch on the device: float32, the vendored ssim formula"""
    x0, y0, x1, y1 = box
    m = (mask[y0:y1, x0:x1] > 0)
    gt = torch.where(m[..., None], img[y0:y1, x0:x1], bkgd[y0:y1, x0:x1]).float() / 255.
    x = rgb[y0:y1, x0:x1].permute(2, 0, 1)[None]
    y = gt.permute(2, 0, 1)[None]
    mf = m.float()
    sq = (y - x) ** 2
    mu1, mu2 = F.conv2d(x, window, groups=3), F.conv2d(y, window, groups=3)
    mu1_sq, mu2_sq, mu1_mu2 = mu1 * mu1, mu2 * mu2, mu1 * mu2
    s1 = F.conv2d(x * x, window, groups=3) - mu1_sq
    s2 = F.conv2d(y * y, window, groups=3) - mu2_sq
    s12 = F.conv2d(x * y, window, groups=3) - mu1_mu2
    v1, v2 = 2.0 * s12 + C2, s1 + s2 + C2
    smap = ((2 * mu1_mu2 + C1) * v1) / ((mu1_sq + mu2_sq + C1) * v2)
    mc = mf[5:-5, 5:-5]
    return torch.stack([torch.tensor(float(sq.numel()), device=rgb.device), sq.sum(), 3 * mf.sum(), (sq * mf[None, None]).sum(),
                        torch.tensor(float(smap.numel()), device=rgb.device), smap.sum(), 3 * mc.sum(), (smap * mc[None, None]).sum()])


def traffic(w, h):
    """bytes a frame's tiles stage (12 B frame + 3 B image + 3 B background + 1 B mask per pixel), the box's unique bytes, the slots"""
    along = lambda n: [min(n - t * TILE, TILE + HALO) for t in range(max(1, -(-(n - HALO) // TILE)))]
    staged = sum(a * b for a in along(w) for b in along(h))
    tiles = len(along(w)) * len(along(h))
    return {"tiles": tiles, "staged_bytes": staged * 19, "box_bytes": w * h * 19, "halo_factor": staged / (w * h),
            "bytes_written": tiles * 64 + 64}


def one_size(r, H, W, a):
    from posegen_amd import DeviceImageBank, FrameScorer
    from posegen_amd.evaluate import box_scores
    from tests import metrics_ref as ref
    dev = torch.device("cuda:0")
    g = torch.Generator(device=dev).manual_seed(H)
    P = H * W
    imgs = torch.randint(0, 256, (2, P, 3), dtype=torch.uint8, device=dev, generator=g)
    masks = torch.randint(0, 2, (2, P, 1), dtype=torch.uint8, device=dev, generator=g)
    bkgds = torch.randint(0, 256, (1, P, 3), dtype=torch.uint8, device=dev, generator=g)
    rgb = torch.rand((H, W, 3), device=dev, generator=g)
    cams = np.tile(np.eye(4, dtype=np.float32)[None], (2, 1, 1))
    bank = DeviceImageBank(r, imgs, masks, masks, cams, np.full(2, 500.0, np.float32), (H, W), bkgds=bkgds, bkgd_idxs=np.zeros(2, np.int32))
    side = 0.6 ** 0.5
    bw, bh = int(round(W * side)), int(round(H * side))
    box = ((W - bw) // 2, (H - bh) // 2, (W - bw) // 2 + bw, (H - bh) // 2 + bh)
    scorer = FrameScorer(bank)
    kernel = event_times(lambda: scorer.score(0, rgb, 1, box), a.calls, a.warmup)
    got = scorer.sums()[0]

    window = torch.tensor(ref.header_taps(), device=dev)
    window = (window[:, None] @ window[None, :]).expand(3, 1, 11, 11).contiguous()
    img2, mask2, bk2 = imgs[1].view(H, W, 3), masks[1].view(H, W), bkgds[0].view(H, W, 3)
    route = event_times(lambda: torch_scores(rgb, img2, mask2, bk2, box, window), a.calls, a.warmup)
    via_torch = torch_scores(rgb, img2, mask2, bk2, box, window).double().cpu().numpy()

    himg, hmask, hbk = img2.cpu().numpy(), mask2.cpu().numpy(), bk2.cpu().numpy()
    taps = ref.header_taps()
    t0 = time.perf_counter()
    for _ in range(a.reps):
        host = ref.frame_sums(himg, hmask, hbk, rgb.cpu().numpy(), box, taps, True)
    host_ms = (time.perf_counter() - t0) * 1e3 / a.reps
    rel = lambda x, y: float(np.max(np.abs(x - y) / np.maximum(1.0, np.abs(y))))
    s = box_scores(got[None])
    return {"H": H, "W": W, "box": list(box), "box_share": bw * bh / (H * W), "kernel": kernel, "torch_on_device": route,
            "numpy_on_host_ms": host_ms, "kernel_over_torch": kernel["ms_mean"] / route["ms_mean"],
            "kernel_vs_numpy_float64_rel": rel(got, host), "torch_float32_vs_numpy_float64_rel": rel(via_torch, host),
            "psnr": float(s["psnr"][0]), "ssim": float(s["ssim"][0]), "hbm": traffic(bw, bh)}


def render_with_and_without(a, n_frames=20, H=512, W=512):
    from posegen_amd import DeviceImageBank, PREC_BF16, surreal_config, synthetic as syn
    from posegen_amd.evaluate import evaluate_frames
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

    plain = lambda: render_frames_device(*args, frame_sink=lambda k, rgb, disp, acc: None, **rkw)
    scored = lambda: evaluate_frames(*args, bank, np.arange(n_frames), **rkw)
    timed(plain), timed(scored)
    t_plain, t_scored = [], []
    for _ in range(a.reps):
        t_plain.append(timed(plain)[0])
        ms, scores = timed(scored)
        t_scored.append(ms)
    caster.renderer.close()
    return {"frames": n_frames, "H": H, "W": W, "render_ms": float(np.median(t_plain)), "render_and_score_ms": float(np.median(t_scored)),
            "all_render_ms": t_plain, "all_render_and_score_ms": t_scored, "frames_scored": len(scores["psnr"]),
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
        sys.exit("bench_metrics: no HIP device (there is nothing to measure on a CPU)")
    r = HipRenderer(surreal_config(), device="cuda:0")
    sizes = [one_size(r, 512, 512, a), one_size(r, 1000, 1000, a)]
    r.close()
    out = {"sizes": sizes, "render": render_with_and_without(a), "calls": a.calls, "warmup": a.warmup, "reps": a.reps,
           "device": torch.cuda.get_device_name(0)}
    line = json.dumps(out)
    print(line, flush=True)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")
    slow = [s for s in sizes if s["kernel_over_torch"] > 1]
    if slow:
        sys.exit("bench_metrics: pg_frame_metrics is slower than the torch route on the device at " +
                 ", ".join(f"{s['H']} x {s['W']} ({s['kernel']['ms_mean']:.3f} ms against {s['torch_on_device']['ms_mean']:.3f} ms)" for s in slow))


if __name__ == "__main__":
    main()
