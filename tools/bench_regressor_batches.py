#!/usr/bin/env python3
"""Time of one regressor input batch (posegen_amd.regressor_input, pg_regressor_input) beside the two other routes to the same pixels.

Two batches of 128 items -> [128,3,224,224]:
  * `frames`: 512 x 512 rendered frames, crop [120:392] (pose_dataset, run_gan.py:1647);
  * `mixed` : the same with every tenth item a 900-pixel box of a 1000 x 1000 picture (mpii_nerf_dataset mixes MPII crops in).
Each is timed three ways in one process on one device:
  1. the kernel: one launch per batch;
  2. the torch operators this repository had before it: crop, normalise, ganloop.resize_antialiased on the device (the mixed batch
     needs one call per crop size and a scatter, as any route built on dense operators does);
  3. the reference's route on the host, one process: normalise, scipy.ndimage.gaussian_filter + zoom per image (the two calls
     skimage's resize makes; "not measured" where scipy is missing), extrapolated from --host-images images to the batch.
Routes 1 and 2 alternate over --rounds rounds of --reps batches behind a warm-up, HIP events around each round's loop (device time
of the queue; the loop ends in a synchronise); the median round is reported with the spread.  Prints one JSON line; --out writes it.

usage: bench_regressor_batches.py [--reps 50] [--rounds 5] [--warmup 5] [--host-images 4] [--out profiles/regressor_batches.json]"""
import argparse
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch

B, R = 128, 224


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--host-images", type=int, default=4)
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    from posegen_amd import surreal_config
    from posegen_amd import regressor_batches as rb
    from posegen_amd.ganloop import resize_antialiased
    from posegen_amd.raycaster import HipRenderer
    from tests import regressor_ref as ref
    dev = torch.device("cuda:0")
    g = torch.Generator(device=dev).manual_seed(0)
    frames = torch.randint(0, 256, (B, 512, 512, 3), dtype=torch.uint8, device=dev, generator=g)
    big = torch.randint(0, 256, (13, 1000, 1000, 3), dtype=torch.uint8, device=dev, generator=g)
    r = HipRenderer(surreal_config(), device=dev)
    store = rb.PixelStore(r, frames)
    store.append(big)
    mean = torch.tensor(rb.IMG_NORM_MEAN, device=dev).view(1, 3, 1, 1)
    std = torch.tensor(rb.IMG_NORM_STD, device=dev).view(1, 3, 1, 1)

    rows_f, boxes_f = np.arange(B), rb.fixed_crop_boxes(B, 120, 392)
    tenth = np.arange(0, B, 10)
    rows_m, boxes_m = rows_f.copy(), boxes_f.copy()
    rows_m[tenth], boxes_m[tenth] = B + np.arange(len(tenth)), [50, 50, 950, 950]
    small = torch.from_numpy(np.setdiff1d(np.arange(B), tenth)).to(dev)
    tenth_dev = torch.from_numpy(tenth).to(dev)

    def torch_crop(pics, lo, hi):
        img = pics[:, lo:hi, lo:hi, :].permute(0, 3, 1, 2).float() / 255.0
        return resize_antialiased((img - mean) / std, (R, R))

    def torch_frames():
        return torch_crop(frames, 120, 392)

    def torch_mixed():
        out = torch.empty(B, 3, R, R, device=dev)
        out[small] = torch_crop(frames[small], 120, 392)
        out[tenth_dev] = torch_crop(big, 50, 950)
        return out

    routes = {"frames": (lambda: rb.regressor_input(store, rows_f, boxes_f, out_res=R), torch_frames),
              "mixed": (lambda: rb.regressor_input(store, rows_m, boxes_m, out_res=R), torch_mixed)}

    def timed(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(a.reps):
            fn()
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1) / a.reps

    out = {"batch": {"items": B, "out_res": R, "frame": [512, 512], "crop": [120, 392], "mixed_every": 10, "mixed_box": 900},
           "reps": a.reps, "rounds": a.rounds, "warmup": a.warmup, "device": torch.cuda.get_device_name(0)}
    for name, (kernel, chain) in routes.items():
        got, old = kernel(), chain()
        torch.cuda.synchronize()
        diff = float((got - old).abs().max())              # the two routes on the same pixels (the chain's float32 sample positions)
        for _ in range(a.warmup):
            kernel(), chain()
        torch.cuda.synchronize()
        tk, tc = [], []
        for _ in range(a.rounds):
            tk.append(timed(kernel))
            tc.append(timed(chain))
        rows, boxes = (rows_f, boxes_f) if name == "frames" else (rows_m, boxes_m)
        bytes_in = int(((boxes[:, 2] - boxes[:, 0]) * (boxes[:, 3] - boxes[:, 1]) * 3).sum())
        bytes_out = B * 3 * R * R * 4
        k_ms, c_ms = statistics.median(tk), statistics.median(tc)
        out[name] = {"kernel_ms": k_ms, "kernel_ms_rounds": tk, "torch_chain_ms": c_ms, "torch_chain_ms_rounds": tc,
                     "torch_chain_over_kernel": c_ms / k_ms, "max_abs_difference_of_the_two": diff,
                     "bytes_read": bytes_in, "bytes_written": bytes_out, "kernel_GBps": (bytes_in + bytes_out) / k_ms / 1e6}

    # the host route, one process
    try:
        from scipy import ndimage as ndi
    except ImportError:
        ndi = None
    for name in routes:
        rows, boxes = (rows_f, boxes_f) if name == "frames" else (rows_m, boxes_m)
        if ndi is None:
            out[name]["scipy_host_ms"] = out[name]["scipy_host_over_kernel"] = "not measured"
            continue
        per_kind = {}
        for kind, pick in (("frame", 1), ("box", 0)):
            if name == "frames" and kind == "box":
                continue
            i = int(pick)
            x0, y0, x1, y1 = boxes[i]
            pics = (frames if rows[i] < B else big)[rows[i] - (0 if rows[i] < B else B)].cpu().numpy()
            t0 = time.perf_counter()
            for _ in range(a.host_images):
                v = ref.normalise(pics[y0:y1, x0:x1], rb.IMG_NORM_MEAN, rb.IMG_NORM_STD)
                sig = (0.0, ref.radius(y1 - y0, R)[0], ref.radius(x1 - x0, R)[0])
                ndi.zoom(ndi.gaussian_filter(v, sig, mode="mirror"), (1, R / (y1 - y0), R / (x1 - x0)), order=1, mode="mirror", grid_mode=True)
            per_kind[kind] = (time.perf_counter() - t0) * 1e3 / a.host_images
        n_box = len(tenth) if name == "mixed" else 0
        host_ms = per_kind["frame"] * (B - n_box) + per_kind.get("box", 0.0) * n_box
        out[name].update({"scipy_host_ms": host_ms, "scipy_host_ms_per_image": per_kind, "scipy_host_images_timed": a.host_images,
                          "scipy_host_over_kernel": host_ms / out[name]["kernel_ms"]})
    r.close()
    line = json.dumps(out)
    print(line, flush=True)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
