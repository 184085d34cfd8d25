#!/usr/bin/env python3
"""Time of one training batch from the device image bank (posegen_amd.RayBatchSource) beside the training step it feeds.

A synthetic bank of 64 frames of 1000 x 1000 pixels is built on the device (about a third of every sampling mask valid, the
rest of the pixels random bytes); measured are
  * the one-off index build (pg_pixel_index_count + the scan + pg_pixel_index_emit), wall clock with a synchronisation;
  * ms per batch of 256 images x 12 pixels over --batches batches behind a warm-up: HIP events on the caller's stream around
    the whole loop (device time of the queue), and the wall clock of the same loop (the host's share: launches, row uploads);
  * the single-process time per batch of the numpy restatement tests/batches_ref.py on the same inputs (copied to the host), for
    scale -- the reference does this work per image on the host;
  * the bf16 training step of tools/bench_train.py (bench.train_step_rate) in the same process on the same device.
The batch must cost less than the step it feeds: `batch_over_step` below 1.  Prints one JSON line; --out writes it to a file.

usage: bench_batches.py [--batches 200] [--warmup 20] [--steps 7] [--out profiles/batch_source.json]"""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch

from bench import train_step_rate

F, H, W = 64, 1000, 1000
N_IMAGES, K = 256, 12


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batches", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--steps", type=int, default=7)
    ap.add_argument("--ref-batches", type=int, default=3)
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    from posegen_amd import DeviceImageBank, RayBatchSource, surreal_config, synthetic as syn
    from posegen_amd.raycaster import HipRenderer
    from tests import batches_ref as ref
    dev = torch.device("cuda:0")
    P = H * W
    g = torch.Generator(device=dev).manual_seed(0)
    imgs = torch.randint(0, 256, (F, P, 3), dtype=torch.uint8, device=dev, generator=g)
    masks = torch.randint(0, 2, (F, P, 1), dtype=torch.uint8, device=dev, generator=g)
    sampling = (torch.rand((F, P), device=dev, generator=g) < 0.33).to(torch.uint8)
    bkgds = torch.randint(0, 256, (4, P, 3), dtype=torch.uint8, device=dev, generator=g)
    bkgd_idxs = np.arange(F) % 4
    c2ws, focals = syn.make_camera(F, H, W)
    _, kps, skts = syn.make_pose(F, 1)
    poses = {"kp3d": torch.tensor(kps, device=dev), "bones": torch.zeros(F, 24, 3, device=dev), "skts": torch.tensor(skts, device=dev),
             "cyls": torch.zeros(F, 5, device=dev)}
    r = HipRenderer(surreal_config(), device=dev)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    bank = DeviceImageBank(r, imgs, masks, sampling, c2ws, focals, (H, W), bkgds=bkgds, bkgd_idxs=bkgd_idxs)
    torch.cuda.synchronize()
    first_build_ms = (time.perf_counter() - t0) * 1e3
    t0 = time.perf_counter()
    bank._build_index()                                  # again, with the buffers of the handle in place
    torch.cuda.synchronize()
    build_ms = (time.perf_counter() - t0) * 1e3

    src = RayBatchSource(bank, N_IMAGES * K, N_IMAGES, poses=poses, generator=torch.Generator(device=dev).manual_seed(1),
                         N_iter=a.warmup + a.batches)
    torch.manual_seed(0)
    it = iter(src)
    for _ in range(a.warmup):
        batch = next(it)
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    t0 = time.perf_counter()
    e0.record()
    for _ in range(a.batches):
        batch = next(it)
    e1.record()
    host_ms = (time.perf_counter() - t0) * 1e3 / a.batches          # the loop's wall clock before any synchronisation
    torch.cuda.synchronize()
    wall_ms = (time.perf_counter() - t0) * 1e3 / a.batches
    event_ms = e0.elapsed_time(e1) / a.batches
    n = batch["ray_batch"].shape[0]
    batch_bytes = sum(t.numel() * t.element_size() for k, t in batch.items() if k not in ("rays_o", "rays_d"))

    # the restatement on the host, one process: index + sampler + gather per batch, as the reference works per image
    hbank = {"imgs": imgs.cpu().numpy(), "masks": masks.cpu().numpy(), "bkgds": bkgds.cpu().numpy(), "bkgd_idxs": bkgd_idxs,
             "c2ws": c2ws, "focals": focals, "HW": (H, W)}
    hs = sampling.cpu().numpy()
    rng = np.random.default_rng(0)
    t0 = time.perf_counter()
    for _ in range(a.ref_batches):
        items = np.sort(rng.integers(0, F, N_IMAGES))
        pix = np.empty((N_IMAGES, K), np.int64)
        for i, f in enumerate(items):                    # np.where per item, like sample_pixels (dataset.py:285-290)
            valid = np.where(hs[f] > 0)[0]
            pix[i] = valid[ref.floyd_ranks(len(valid), K, rng.random(K))]
        ref.gather(hbank, items, pix)
    ref_ms = (time.perf_counter() - t0) * 1e3 / a.ref_batches
    nbytes = bank.nbytes
    del src, bank, batch, it
    r.close()

    step = train_step_rate(dev, steps=a.steps, precision="bf16")
    out = {"bank": {"frames": F, "H": H, "W": W, "bytes": nbytes, "valid_share": float(hs.mean())},
           "batch": {"images": N_IMAGES, "pixels_per_image": K, "rays": n, "bytes_out": batch_bytes},
           "index_build_ms": build_ms, "index_build_first_ms": first_build_ms,
           "batch_ms_events": event_ms, "batch_ms_wall": wall_ms, "batch_ms_host_enqueue": host_ms, "batches": a.batches, "warmup": a.warmup,
           "restatement_host_ms_per_batch": ref_ms, "restatement_batches": a.ref_batches,
           "train_step_bf16_ms": step["ms_per_step"], "train_step_n_rand": step["n_rand"], "train_steps": a.steps,
           "batch_over_step": max(event_ms, wall_ms) / step["ms_per_step"], "device": torch.cuda.get_device_name(0)}
    line = json.dumps(out)
    print(line, flush=True)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")
    if out["batch_over_step"] >= 1:
        sys.exit("bench_batches: a batch costs as much as the training step it feeds")


if __name__ == "__main__":
    main()
