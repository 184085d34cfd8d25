#!/usr/bin/env python3
"""What a scene costs beside the frames it is made of (pg_render_scene, posegen_amd.scene).

One 512 x 512 frame with two people of a two-subject bank (the synthetic models, bf16, 64 + 16 samples) whose boxes overlap and
whose bodies interleave in depth, in one process on one device:
  * scene:   one render_scene call (both people, the merge, the frame);
  * frames:  two render_frame calls of the same poses and boxes, each with its subject selected (what a caller did before, short
             of the host-side paste by acc);
  * kernel:  scene_composite_kernel alone, in its stage form on the scene's own lists, over the pixels the frame form walks (the
             bounding rectangle of the boxes) with the row map of the boxes.
HIP events around each of --calls calls behind --warmup warm-ups; scene and frames alternate --reps times and the medians of the
repetitions' means are reported, with their ratio.  Also the bytes of the lists (sum n_p S_f 20 B) that the scene kernel reads and
the two-net pipeline copies out of its workspace (read + write), and the bandwidth the kernel's time amounts to.
Prints one JSON line; --out writes it to a file.

usage: bench_scene.py [--size 512] [--calls 10] [--warmup 3] [--reps 3] [--out profiles/scene_frame.json]"""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch


def event_times(fn, calls, warmup):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    pairs = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(calls)]
    for e0, e1 in pairs:
        e0.record()
        fn()
        e1.record()
    torch.cuda.synchronize()
    per = [e0.elapsed_time(e1) for e0, e1 in pairs]
    return float(np.mean(per)), float(np.min(per))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", type=int, default=512)
    ap.add_argument("--calls", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    from posegen_amd import surreal_config, synthetic as syn
    from posegen_amd.raycaster import HipRayCaster
    from posegen_amd.rays import kp_to_boxes
    from posegen_amd.scene import ScenePerson, place_people, stage_scene_composite

    H = W = a.size
    S, N = 64, 16
    cfg = surreal_config()
    dev = "cuda:0"
    caster = HipRayCaster.from_subjects(cfg, [syn.make_model(cfg, s) for s in (0, 1)], device=dev, precision="bf16")
    r = caster.renderer
    c2ws, focals = syn.make_camera(1, H, W)
    c2w, focal = c2ws[0], float(focals[0])
    right, back = c2w[:3, 0], c2w[:3, 2]
    _, kps, skts = syn.make_pose(2, 3)
    # one person 0.3 in front of and one 0.3 behind a plane 3 units behind the origin, 0.25 to either side
    kp2, sk2 = place_people(kps, skts, np.stack([-2.7 * back + 0.25 * right, -3.3 * back - 0.25 * right]).astype(np.float32))
    cyls, boxes, _ = kp_to_boxes([torch.tensor(c2w)] * 2, H, W, focal, kps=torch.tensor(kp2), ext_scale=cfg.ext_scale)
    people = [ScenePerson(torch.tensor(sk2[p]).to(dev), cyls[p].to(dev), boxes[p], p) for p in range(2)]
    kw = dict(n_samples=S, n_importance=N)

    def scene():
        return r.render_scene(H, W, focal, c2w, people, **kw)

    def frames():
        out = []
        for q in people:
            r.select_subject(q.subject)
            out.append(r.render_frame(H, W, focal, c2w, q.box, q.skts[None], q.cyl[None], **kw))
        r.select_subject(0)
        return out

    # the scene's own lists and the row map of its boxes for the kernel alone
    rgb, disp, acc, pacc, lists = r.render_scene(H, W, focal, c2w, people, want_person_acc=True, return_lists=True, **kw)
    rows = torch.full((2, H * W), -1, dtype=torch.int32)
    n_rows = []
    for p, q in enumerate(people):
        (x0, y0), (x1, y1) = q.box
        x0, y0, x1, y1 = max(int(x0), 0), max(int(y0), 0), min(int(x1), W), min(int(y1), H)
        rr, cc = torch.meshgrid(torch.arange(y0, y1), torch.arange(x0, x1), indexing="ij")
        rows[p, (rr * W + cc).reshape(-1)] = torch.arange((y1 - y0) * (x1 - x0), dtype=torch.int32)
        n_rows.append((y1 - y0) * (x1 - x0))
    from posegen_amd.rays import get_rays
    _, d = get_rays(H, W, focal, torch.tensor(c2w))
    covered = (rows >= 0).any(0)
    both = (rows >= 0).all(0)
    yy, xx = torch.nonzero(covered.view(H, W), as_tuple=True)
    rect = torch.zeros(H, W, dtype=torch.bool)
    rect[int(yy.min()):int(yy.max()) + 1, int(xx.min()):int(xx.max()) + 1] = True
    rect = rect.view(-1)
    zs, raws = [z for z, _ in lists], [w for _, w in lists]
    rows_d, dirs = rows[:, rect].contiguous().to(dev), d.reshape(-1, 3)[rect].contiguous().to(dev)
    stage = stage_scene_composite(r, zs, raws, rows_d, dirs)
    torch.cuda.synchronize()
    same = bool(torch.equal(stage["acc_map"], acc.view(-1)[rect.to(dev)]))

    reps = {"scene": [], "frames": []}
    for _ in range(a.reps):                 # alternating: both see the same drift of the device
        reps["scene"].append(event_times(scene, a.calls, a.warmup))
        reps["frames"].append(event_times(frames, a.calls, a.warmup))
    kern = event_times(lambda: stage_scene_composite(r, zs, raws, rows_d, dirs), a.calls, a.warmup)
    med = lambda k: float(np.median([m for m, _ in reps[k]]))
    list_bytes = int(sum(n_rows)) * (S + N) * 20
    res = {
        "bench": "scene_frame", "device": torch.cuda.get_device_name(0), "H": H, "W": W, "precision": "bf16", "n_samples": S,
        "n_importance": N, "people": 2, "box_pixels": n_rows, "pixels_covered": int(covered.sum()), "pixels_covered_by_both": int(both.sum()),
        "calls": a.calls, "warmup": a.warmup, "reps": a.reps,
        "scene_ms": med("scene"), "scene_ms_reps": [m for m, _ in reps["scene"]], "scene_ms_min": min(m for _, m in reps["scene"]),
        "two_frames_ms": med("frames"), "two_frames_ms_reps": [m for m, _ in reps["frames"]],
        "two_frames_ms_min": min(m for _, m in reps["frames"]),
        "scene_over_two_frames": med("scene") / med("frames"),
        "scene_kernel_ms": kern[0], "scene_kernel_ms_min": kern[1], "scene_kernel_form": "stage (row map) on the scene's lists, bounding rectangle",
        "rect_pixels": int(rect.sum()),
        "list_bytes": list_bytes, "scene_kernel_gb_per_s": list_bytes / (kern[0] * 1e-3) / 1e9,
        "list_copy_bytes_two_net": 2 * list_bytes,
        "stage_form_equals_frame_form_acc": same,
        "mean_acc": float(acc.mean()), "max_person_acc": [float(pacc[p].max()) for p in range(2)],
    }
    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")
    caster.renderer.close()


if __name__ == "__main__":
    main()
