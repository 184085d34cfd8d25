#!/usr/bin/env python3
"""Time of scoring a batch of 3-D poses on the device (pg_pose_scores, posegen_amd.PoseScorer) beside the two other ways to the
same numbers.

For B = 35 515 poses of 14 joints (the 3DPW test set's size) and B = 1024 poses of 24 joints (seeded random poses: the kernel's
time does not depend on the values), PA-MPJPE with PCK and 31 AUC thresholds, measured in one process on one device:
  * ms per pg_pose_scores call (align = best, per-pose values, aligned key points and joint errors written): HIP events around a
    warmed loop that runs for at least --window seconds;
  * the torch route on the same device: the same formula as batched ops -- means, norms, torch.linalg.svd of the [B,3,3]
    cross-covariances, the aligned points, distances and threshold shares -- in float64, timed the same way;
  * the numpy route on the host: the key points downloaded, then the reference's loop, one `procrustes`-shaped numpy SVD per pose
    in float32 (restated here: means, norms, np.linalg.svd, Z) -- what a caller does today; wall clock.
No ratio is a condition; the tool reports.  Prints one JSON line; --out writes it to a file.

usage: bench_pose_scores.py [--window 0.5] [--warmup 3] [--out profiles/pose_scores.json]"""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch


def event_window(fn, window_s, warmup):
    """ms per call of fn: warmed, then batches of calls between one event pair until `window_s` seconds of device time are covered"""
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    calls, total_ms, batch = 0, 0.0, 4
    while total_ms < window_s * 1e3:
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(batch):
            fn()
        e1.record()
        torch.cuda.synchronize()
        total_ms += e0.elapsed_time(e1)
        calls += batch
        batch = min(batch * 2, 1024)
    return {"ms_per_call": total_ms / calls, "calls": calls, "window_ms": total_ms}


def torch_route(pred, gt, thresholds):
    """PA-MPJPE, d and the threshold shares by batched torch ops in float64 on the device"""
    p, g = pred.double(), gt.double()
    muX, muY = g.mean(1, keepdim=True), p.mean(1, keepdim=True)
    X0, Y0 = g - muX, p - muY
    nX, nY = X0.pow(2).sum((1, 2)).sqrt(), Y0.pow(2).sum((1, 2)).sqrt()
    X0, Y0 = X0 / nX[:, None, None], Y0 / nY[:, None, None]
    U, s, Vt = torch.linalg.svd(X0.transpose(1, 2) @ Y0)
    T = Vt.transpose(1, 2) @ U.transpose(1, 2)
    tr = s.sum(1)
    Z = (nX * tr)[:, None, None] * (Y0 @ T) + muX
    dist = (Z - g).pow(2).sum(-1).sqrt()
    raw = (p - g).pow(2).sum(-1).sqrt()
    shares = torch.stack([(raw[..., None] < thresholds).double().mean((0, 1)), (dist[..., None] < thresholds).double().mean((0, 1))])
    return raw.mean(), dist.mean(), (1 - tr * tr).mean(), shares


def numpy_loop(pred, gt):
    """the reference's per-pose loop on the host in float32 (Criterion3DPose_ProcrustesCorrected's shape): mean aligned distance"""
    out = np.empty(pred.shape[:2], dtype=np.float32)
    for i in range(len(pred)):
        X, Y = gt[i], pred[i]
        muX, muY = X.mean(0), Y.mean(0)
        X0, Y0 = X - muX, Y - muY
        nX, nY = np.sqrt((X0 ** 2.).sum()), np.sqrt((Y0 ** 2.).sum())
        X0, Y0 = X0 / nX, Y0 / nY
        U, s, Vt = np.linalg.svd(np.dot(X0.T, Y0), full_matrices=False)
        Z = nX * s.sum() * np.dot(Y0, np.dot(Vt.T, U.T)) + muX
        out[i] = np.sqrt(((Z - X) ** 2).sum(-1))
    return float(out.mean())


def one_size(scorer, B, J, a):
    dev = scorer.device
    g = torch.Generator(device=dev).manual_seed(B + J)
    gt = torch.randn((B, J, 3), device=dev, generator=g) * torch.tensor([0.25, 0.5, 0.15], device=dev)
    pred = 1.1 * (gt + 0.03 * torch.randn((B, J, 3), device=dev, generator=g)) + 0.2
    th = np.concatenate([[0.15], np.linspace(0, 0.15, 31)])
    th_dev = torch.tensor(th, device=dev)
    call = lambda: scorer.enqueue(pred, gt, align="best", thresholds=th, ret_per_pose=True, ret_aligned=True, ret_joint_err=True)
    kernel = event_window(call, a.window, a.warmup)
    s = call()["summary"].cpu().numpy()
    try:
        route = event_window(lambda: torch_route(pred, gt, th_dev), a.window, a.warmup)
        t = torch_route(pred, gt, th_dev)
    except RuntimeError as e:                                # a torch build without a batched float64 SVD on the device
        route, t = {"ms_per_call": float("nan"), "error": str(e)[:200]}, None
    hp, hg = pred.cpu().numpy(), gt.cpu().numpy()
    t0 = time.perf_counter()
    host_mean = numpy_loop(hp, hg)
    host_ms = (time.perf_counter() - t0) * 1e3
    return {"B": B, "J": J, "thresholds": len(th), "kernel": kernel, "torch_on_device": route, "numpy_loop_on_host_ms": host_ms,
            "kernel_over_torch": kernel["ms_per_call"] / route["ms_per_call"], "numpy_over_kernel": host_ms / kernel["ms_per_call"],
            "pa_mpjpe": float(s[2]), "pa_mpjpe_torch_float64": None if t is None else float(t[1]), "pa_mpjpe_numpy_float32": host_mean,
            "pck_counts_equal_to_torch": None if t is None else bool(np.array_equal(np.rint(s[4:].reshape(2, -1) * B * J), np.rint(t[3].cpu().numpy() * B * J))),
            "bytes_read": B * J * 24, "bytes_written": B * (32 + J * 16)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--window", type=float, default=0.5)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    from posegen_amd import PoseScorer, surreal_config
    from posegen_amd.raycaster import HipRenderer
    if not torch.cuda.is_available():
        sys.exit("bench_pose_scores: no HIP device (there is nothing to measure on a CPU)")
    r = HipRenderer(surreal_config(), device="cuda:0")
    scorer = PoseScorer(r)
    sizes = [one_size(scorer, 35515, 14, a), one_size(scorer, 1024, 24, a)]
    r.close()
    out = {"sizes": sizes, "window_s": a.window, "warmup": a.warmup, "device": torch.cuda.get_device_name(0)}
    line = json.dumps(out)
    print(line, flush=True)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
