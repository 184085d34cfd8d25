#!/usr/bin/env python3
"""Time of the SMPL body on the device (pg_smpl_forward, posegen_amd.smpl.BodyModel) beside the same formula as stock torch ops.

For V = 6890, NB = 10 and a 17-row regressor (the synthetic body of posegen_amd.synthetic.make_body_model: the kernel's time does
not depend on the values), at B = 35 515 (the 3DPW test set), 1024 and 32 poses, measured in one process on one device:
  * ms per pg_smpl_forward call for the regressed joints only, and for the same with the vertices written: HIP events around a
    warmed loop that runs for at least --window seconds, the two alternating, --repeats windows each (median and range reported);
  * the torch route on the same device: `lbs` + `vertices2joints` as the reference writes them (einsum blend, matmul posedirs,
    the chain, the [B,V,4,4] skinning transforms, the regressor einsum) in float32, in chunks of --chunk poses so that it fits,
    timed the same way;
  * the algorithmic FLOPs per pose, 2 (1 + NB + 207) 3V + 2 (24 * 12 + 12) V + 2 * 3 K V, and the share of the 157.3 TF fp32
    peak that the kernel's time implies.
The largest difference between the two routes' regressed joints is reported beside the times.  No ratio is a condition; the tool
reports.  Prints one JSON line; --out writes it to a file.

usage: bench_smpl.py [--window 0.5] [--warmup 3] [--repeats 3] [--chunk 256] [--out profiles/smpl_body.json]"""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch

PEAK_FP32_TF = 157.3


def event_window(fn, window_s, warmup):
    """ms per call of fn: warmed, then batches of calls between one event pair until `window_s` seconds of device time are covered"""
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    calls, total_ms, batch = 0, 0.0, 1
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
    return total_ms / calls


def alternating(fns, window_s, warmup, repeats):
    """{name: {"ms_per_call": median, "min", "max", "windows"}} of the callables, one window of each in turn, `repeats` times"""
    ms = {k: [] for k in fns}
    for _ in range(repeats):
        for k, fn in fns.items():
            ms[k].append(event_window(fn, window_s, warmup))
    return {k: {"ms_per_call": float(np.median(v)), "min": min(v), "max": max(v), "windows": len(v)} for k, v in ms.items()}


def rodrigues(r):
    """batch_rodrigues (smplx/smplx/lbs.py:295-329)"""
    angle = torch.norm(r + 1e-8, dim=1, keepdim=True)
    d = r / angle
    rx, ry, rz = torch.split(d, 1, dim=1)
    zeros = torch.zeros_like(rx)
    K = torch.cat([zeros, -rz, ry, rz, zeros, -rx, -ry, rx, zeros], dim=1).view(-1, 3, 3)
    return torch.eye(3, device=r.device)[None] + torch.sin(angle)[:, None] * K + (1 - torch.cos(angle))[:, None] * torch.bmm(K, K)


def torch_lbs(m, betas, pose, regress, want_verts):
    """lbs + vertices2joints (lbs.py:152-268, 345-401) as stock float32 torch ops on one chunk of poses"""
    B = pose.shape[0]
    v_shaped = m["v_template"] + torch.einsum("bl,mkl->bmk", betas, m["shapedirs"])
    J = torch.einsum("bik,ji->bjk", v_shaped, m["J_regressor"])
    R = rodrigues(pose.view(-1, 3)).view(B, 24, 3, 3)
    feat = (R[:, 1:] - torch.eye(3, device=pose.device)).view(B, -1)
    v_posed = torch.matmul(feat, m["posedirs"]).view(B, -1, 3) + v_shaped
    par = m["parents"]
    rel = J.clone()
    rel[:, 1:] -= J[:, par[1:]]
    T = torch.zeros(B, 24, 4, 4, device=pose.device)
    T[:, :, :3, :3], T[:, :, :3, 3], T[:, :, 3, 3] = R, rel, 1.0
    chain = [T[:, 0]]
    for i in range(1, 24):
        chain.append(torch.matmul(chain[par[i]], T[:, i]))
    G = torch.stack(chain, dim=1)
    A = G.clone()
    A[:, :, :3, 3] -= torch.einsum("bjrc,bjc->bjr", G[:, :, :3, :3], J)
    Tv = torch.matmul(m["lbs_weights"][None].expand(B, -1, -1), A.view(B, 24, 16)).view(B, -1, 4, 4)
    homo = torch.cat([v_posed, torch.ones(B, v_posed.shape[1], 1, device=pose.device)], dim=2)
    verts = torch.matmul(Tv, homo[..., None])[:, :, :3, 0]
    reg = torch.einsum("bik,ji->bjk", verts, regress)
    return (verts if want_verts else None), reg


def one_size(body, tm, regress, B, K, a):
    dev = body.device
    g = torch.Generator(device=dev).manual_seed(B)
    betas = (torch.rand((B, body.NB), device=dev, generator=g) * 6 - 3)
    pose = torch.randn((B, 24, 3), device=dev, generator=g) * 0.4

    def torch_route(want_verts):
        outs = [torch_lbs(tm, betas[i:i + a.chunk], pose[i:i + a.chunk], regress, want_verts) for i in range(0, B, a.chunk)]
        return torch.cat([o[1] for o in outs])

    fns = {"kernel_joints_only": lambda: body.forward(betas, pose, regressor="k", joints=False),
           "kernel_with_verts": lambda: body.forward(betas, pose, regressor="k", want_vertices=True, joints=False),
           "torch_joints_only": lambda: torch_route(False)}
    if B * body.V * 12 <= 2 << 30:                               # the torch route's vertices of the whole batch, where they fit
        fns["torch_with_verts"] = lambda: torch_route(True)
    t = alternating(fns, a.window, a.warmup, a.repeats)
    diff = float((body.forward(betas, pose, regressor="k", joints=False).regressed - torch_route(False)).abs().max())
    flop = 2 * (1 + body.NB + 207) * 3 * body.V + 2 * (24 * 12 + 12) * body.V + 2 * 3 * K * body.V
    tf = flop * B / (t["kernel_joints_only"]["ms_per_call"] * 1e-3) / 1e12
    return {"B": B, "V": body.V, "NB": body.NB, "K": K, "times": t, "torch_chunk": a.chunk,
            "torch_over_kernel_joints_only": t["torch_joints_only"]["ms_per_call"] / t["kernel_joints_only"]["ms_per_call"],
            "flop_per_pose": flop, "kernel_tflops": tf, "share_of_fp32_peak": tf / PEAK_FP32_TF,
            "max_abs_difference_regressed_kernel_vs_torch": diff}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--window", type=float, default=0.5)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--chunk", type=int, default=256)
    ap.add_argument("--sizes", type=int, nargs="*", default=[35515, 1024, 32])
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    from posegen_amd import surreal_config
    from posegen_amd.raycaster import HipRenderer
    from posegen_amd.smpl import MODEL_KEYS, BodyModel
    from posegen_amd.synthetic import make_body_model
    if not torch.cuda.is_available():
        sys.exit("bench_smpl: no HIP device (there is nothing to measure on a CPU)")
    V, NB, K = 6890, 10, 17
    model = make_body_model(V, NB=NB, seed=0, regress_rows=(K,))
    r = HipRenderer(surreal_config(), device="cuda:0")
    body = BodyModel(r, *(model[k] for k in MODEL_KEYS), regressors={"k": model[f"regressor_{K}"]})
    tm = {k: torch.from_numpy(model[k]).to(body.device) for k in MODEL_KEYS if k != "parents"}
    tm["parents"] = [int(p) for p in model["parents"]]
    regress = torch.from_numpy(model[f"regressor_{K}"]).to(body.device)
    sizes = [one_size(body, tm, regress, B, K, a) for B in a.sizes]
    r.close()
    out = {"sizes": sizes, "window_s": a.window, "warmup": a.warmup, "repeats": a.repeats, "device": torch.cuda.get_device_name(0)}
    line = json.dumps(out)
    print(line, flush=True)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
