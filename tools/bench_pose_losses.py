#!/usr/bin/env python3
"""Time of one training step's pose loss, forward and backward, on the device route (posegen_amd.pose_losses / ganloop: HIP kernels
behind torch.autograd.Functions) beside the same formulas as float64 torch ops with autograd on the same device.

  case 1, the train_spin batch (run_gan.py:1896-1910): B = 128 rotation matrices -> key points -> norm-matched loss, weight 0.1,
          cap 0.02 -> gradient in the matrices;
  case 2, the generator batch (:2032-2034, 2085-2105): B = 1024 axis-angle poses -> key points -> 1 - mpjpe -> gradient in the poses.
Seeded inputs; both routes run forward + backward.  ms per step: HIP events around a warmed loop that runs for at least --window
seconds.  Launches: the library's kernels per step are counted from its code (forward kinematics 1, pg_pose_loss 3 -- it writes the
gradients with the loss -- and the transpose 1).  What torch launches besides is counted where it can be without a profiler: in
the forward pass the ATen operators that are not views, as they are dispatched (each is at least one launch); in the backward pass
the nodes of the autograd graph, leaf accumulators aside (each runs at least one operator; the library's nodes also cast and
allocate around their one call).  No ratio is a condition; the tool reports.  Prints one JSON line; --out writes it to a file.

usage: bench_pose_losses.py [--window 0.5] [--warmup 3] [--out profiles/pose_losses.json]"""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch
from torch.utils._python_dispatch import TorchDispatchMode

JOINTS = [1, 2, 4, 5, 7, 8, 12, 15, 16, 17, 18, 19, 20, 21]
LIBRARY_KERNELS = {"forward": 4, "backward": 1}              # kinematics, pose loss (per pose, sum, gradient); the kinematics' transpose


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


class OpCounter(TorchDispatchMode):
    """ATen operators dispatched while active, views aside"""

    def __init__(self):
        super().__init__()
        self.n = 0

    def __torch_dispatch__(self, func, types, args=(), kwargs=None):
        if not getattr(func, "is_view", False):
            self.n += 1
        return func(*args, **(kwargs or {}))


def count_launch_sites(forward):
    """(non-view ATen operators of one forward pass, autograd nodes behind its result without the leaf accumulators)"""
    with OpCounter() as c:
        out = forward()
    torch.cuda.synchronize()
    seen, todo = set(), [out.grad_fn]
    while todo:
        f = todo.pop()
        if f is None or f in seen:
            continue
        seen.add(f)
        todo += [n for n, _ in f.next_functions]
    return c.n, sum(type(f).__name__ != "AccumulateGrad" for f in seen)


def torch_rotations(rv):
    """rotation vector -> unit quaternion -> matrix, float64 (posegen_amd.skeleton.rotvec_to_matrix as torch ops; series in theta^2
    below 1e-3 so that the gradient is finite at zero)"""
    t2 = (rv * rv).sum(-1)
    small = t2.detach().sqrt() < 1e-3
    th = torch.where(small, torch.ones_like(t2), t2).sqrt()
    k = torch.where(small, 0.5 - t2 / 48 + t2 * t2 / 3840, torch.sin(0.5 * th) / th)
    qw = torch.where(small, 1 - t2 / 8 + t2 * t2 / 384, torch.cos(0.5 * th))
    q = torch.cat([rv * k[..., None], qw[..., None]], -1)
    x, y, z, w = (q / q.norm(dim=-1, keepdim=True)).unbind(-1)
    return torch.stack([x * x - y * y - z * z + w * w, 2 * (x * y - z * w), 2 * (x * z + y * w),
                        2 * (x * y + z * w), -x * x + y * y - z * z + w * w, 2 * (y * z - x * w),
                        2 * (x * z - y * w), 2 * (y * z + x * w), -x * x - y * y + z * z + w * w], -1).reshape(rv.shape[:-1] + (3, 3))


def torch_chain(R, offs, parents):
    """key points of the chain l2w_j = l2w_parent [R_j | offs_j] as one [B,4,4] matmul per joint, like the reference's unrolled chain"""
    B = R.shape[0]
    rel = torch.zeros(B, 24, 4, 4, dtype=torch.float64, device=R.device)
    rel[:, :, :3, :3], rel[:, :, :3, 3], rel[:, :, 3, 3] = R, offs, 1.0
    l2w = [rel[:, 0]]
    for j in range(1, 24):
        l2w.append(l2w[parents[j]] @ rel[:, j])
    return torch.stack(l2w, 1)[:, :, :3, 3]


def torch_select(x):
    return (x - x[:, :1])[:, JOINTS]


def case_regressor(r, a, offs, parents):
    from posegen_amd import ganloop
    B, dev = 128, r.device
    g = torch.Generator(device=dev).manual_seed(1)
    bones = 0.3 * torch.randn((B, 24, 3), device=dev, generator=g, dtype=torch.float64)
    level = torch.tensor([0.05, 0.15, 0.6], device=dev, dtype=torch.float64)[torch.arange(B, device=dev) % 3][:, None, None]
    gt = torch_chain(torch_rotations(bones), offs, parents).float()
    rot = torch_rotations(bones + level * torch.randn((B, 24, 3), device=dev, generator=g, dtype=torch.float64)).float().requires_grad_(True)

    def ours():
        return ganloop.regressor_loss(r, rot, gt)

    def route():
        p, q = torch_select(torch_chain(rot.double(), offs, parents)), torch_select(gt.double())
        p = p / p.norm(dim=(-1, -2), keepdim=True) * q.norm(dim=(-1, -2), keepdim=True)
        per_pose = (p - q).norm(dim=-1).mean(-1) * 0.1
        return per_pose[per_pose < 0.02].mean()

    return dict(name="train_spin batch: rotmats -> norm-matched capped loss -> d_rotmats", B=B), ours, route, rot


def case_generator(r, a, offs, parents):
    from posegen_amd import ganloop
    B, dev = 1024, r.device
    g = torch.Generator(device=dev).manual_seed(2)
    bones = (0.3 * torch.randn((B, 24, 3), device=dev, generator=g)).requires_grad_(True)
    pred = torch_chain(torch_rotations(bones.detach().double() + 0.15 * torch.randn((B, 24, 3), device=dev, generator=g, dtype=torch.float64)),
                       offs, parents).float()

    def ours():
        return ganloop.generator_feedback(r, pred, bones)

    def route():
        gt = torch_chain(torch_rotations(bones.double()), offs, parents)
        return 1.0 - (torch_select(pred.double()) - torch_select(gt)).norm(dim=-1).mean()

    return dict(name="generator batch: axis-angle -> 1 - mpjpe -> d_bones", B=B), ours, route, bones


def run_case(make, r, a, offs, parents):
    info, ours, route, leaf = make(r, a, offs, parents)

    def step(forward):
        leaf.grad = None
        out = forward()
        out.backward()
        return out

    v_ours = float(step(ours).detach().cpu())
    g_ours = leaf.grad.detach().clone()
    v_route = float(step(route).detach().cpu())
    g_route = leaf.grad.detach().clone()
    info.update(value=v_ours, value_torch=v_route, grad_max_abs=float(g_ours.abs().max().cpu()),
                grad_max_abs_difference=float((g_ours - g_route).abs().max().cpu()))
    ops, nodes = count_launch_sites(ours)
    info["launches"] = {"library_kernels": LIBRARY_KERNELS, "forward_torch_ops": ops, "backward_graph_nodes": nodes}
    ops, nodes = count_launch_sites(route)
    info["launches_torch"] = {"forward_torch_ops": ops, "backward_graph_nodes": nodes}
    info["device_route"] = event_window(lambda: step(ours), a.window, a.warmup)
    info["torch_route"] = event_window(lambda: step(route), a.window, a.warmup)
    info["torch_over_device"] = info["torch_route"]["ms_per_call"] / info["device_route"]["ms_per_call"]
    return info


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--window", type=float, default=0.5)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    from posegen_amd import surreal_config
    from posegen_amd.raycaster import HipRenderer
    from posegen_amd.skeleton import SMPLSkeleton, smpl_rest_pose
    if not torch.cuda.is_available():
        sys.exit("bench_pose_losses: no HIP device (there is nothing to measure on a CPU)")
    r = HipRenderer(surreal_config(), device="cuda:0")
    parents = [int(p) for p in SMPLSkeleton.joint_trees]
    rest = smpl_rest_pose.astype(np.float32) * np.float32(0.4)
    offs = rest.copy()
    offs[1:] = rest[1:] - rest[parents[1:]]
    offs = torch.from_numpy(offs.astype(np.float64)).to(r.device)
    cases = [run_case(case_regressor, r, a, offs, parents), run_case(case_generator, r, a, offs, parents)]
    r.close()
    out = {"cases": cases, "window_s": a.window, "warmup": a.warmup, "device": torch.cuda.get_device_name(0)}
    line = json.dumps(out)
    print(line, flush=True)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
