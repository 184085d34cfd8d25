#!/usr/bin/env python3
"""ms per 512 x 512 frame of the single-net model (surreal_single_config: one net, multires_views = 0, 96 + 48 samples)
against the two-net path at the same 96 + 48, in bf16 and fp16c.  All rays hit (bench.full_frame_rays).

The single-net path evaluates S + N = 144 points per ray, the two-net path S + (S + N) = 240; the fused kernel's share of
the frame should move by about 144 / 240.  Prints one JSON line per (model, precision) and, with --out, writes them there.

Usage:  python tools/bench_single_net.py [--steps 10] [--warmup 3] [--out profiles/single_net_frame.json]
"""
from __future__ import annotations

import argparse
import json
import os
import statistics
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--size", type=int, default=512)
    ap.add_argument("--precisions", default="bf16,fp16c")
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    import torch
    from bench import full_frame_rays
    from posegen_amd import synthetic as syn
    from posegen_amd.config import surreal_config, surreal_single_config
    from posegen_amd.raycaster import HipRayCaster
    dev = torch.device("cuda:0")
    H = W = a.size
    models = {"single_net": surreal_single_config(),
              "two_net": surreal_config(n_samples=96, n_importance=48, multires_views=0)}
    lines = []
    for prec in a.precisions.split(","):
        for tag, cfg in models.items():
            wc, wf, tv, td = syn.make_model(cfg, 0)
            c = HipRayCaster.from_weights(cfg, wc, None if cfg.single_net else wf, tv, td, device=dev, precision=prec)
            r = c.renderer
            rb, skts, cyl, *_ = full_frame_rays(H, W, dev, cfg)
            r.set_chunk(cfg.chunk)
            kw = dict(n_samples=cfg.n_samples, n_importance=cfg.n_importance, want_alpha=False)
            for _ in range(a.warmup):
                r.render_rays(rb, skts, cyl, **kw)
            torch.cuda.synchronize(dev)
            times = []
            r.profile_enable(True)
            r.profile_read()
            r.profile_read_aux()
            for _ in range(a.steps):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                r.render_rays(rb, skts, cyl, **kw)
                e1.record()
                e1.synchronize()
                times.append(e0.elapsed_time(e1))
            launches, eval_ms, pts = r.profile_read()
            aux_n, aux_ms = r.profile_read_aux()
            r.profile_enable(False)
            line = {"model": tag, "precision": prec, "H": H, "W": W, "n_samples": cfg.n_samples,
                    "n_importance": cfg.n_importance, "evals_per_ray": cfg.evals_per_ray(),
                    "ms_per_frame_median": statistics.median(times), "ms_per_frame_min": min(times),
                    "eval_kernel_ms_per_frame": eval_ms / a.steps, "eval_launches_per_frame": launches / a.steps,
                    "record_kernel_ms_per_frame": aux_ms / a.steps, "points_per_frame": pts // a.steps,
                    "steps": a.steps, "warmup": a.warmup}
            print(json.dumps(line), flush=True)
            lines.append(line)
            r.close()
    by = {(l["model"], l["precision"]): l for l in lines}
    for prec in a.precisions.split(","):
        s, t = by[("single_net", prec)], by[("two_net", prec)]
        print(json.dumps({"precision": prec, "frame_ratio": s["ms_per_frame_median"] / t["ms_per_frame_median"],
                          "eval_ratio": s["eval_kernel_ms_per_frame"] / t["eval_kernel_ms_per_frame"],
                          "evals_ratio": s["evals_per_ray"] / t["evals_per_ray"]}), flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            for l in lines:
                f.write(json.dumps(l) + "\n")


if __name__ == "__main__":
    main()
