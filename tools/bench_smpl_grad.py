#!/usr/bin/env python3
"""Time of the differentiable SMPL body on the device (pg_smpl_forward + pg_smpl_backward behind BodyModel.differentiable) beside the
same formulas as stock float32 torch ops under autograd on the same device.

For V = 6890, NB = 10 and a 17-row regressor (the synthetic body of posegen_amd.synthetic.make_body_model: the kernels' time does
not depend on the values), at B = 32, 1024 and 35 515 poses (the 3DPW test set, the largest batch the loop ever holds), in one
process on one device, for a cotangent on the regressed joints only and for cotangents on the vertices too:
  * ms per forward + backward through `BodyModel.differentiable` and `torch.autograd.grad` with the cotangents given (no loss ops
    in the timed region), and ms per `BodyModel.forward` alone with the same outputs; backward = the difference; HIP events around a
    warmed loop that runs for at least --window seconds, the routes alternating, --repeats windows each (median and range);
  * the torch route: `lbs` + `vertices2joints` as tools/bench_smpl.py writes them, under autograd, in chunks of --chunk poses,
    gradients to betas and pose, timed the same way.
The largest difference between the two routes' gradients is reported beside the times, relative to the tensor's largest entry.  No
ratio is a condition; the tool reports.  Prints one JSON line; --out writes it to a file.

usage: bench_smpl_grad.py [--window 0.5] [--warmup 3] [--repeats 3] [--chunk 256] [--sizes 32 1024 35515] [--out profiles/smpl_body_grad.json]"""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch

from tools.bench_smpl import alternating, torch_lbs


def one_size(body, tm, regress, B, K, a):
    dev = body.device
    g = torch.Generator(device=dev).manual_seed(B)
    betas = (torch.rand((B, body.NB), device=dev, generator=g) * 6 - 3).requires_grad_(True)
    pose = (torch.randn((B, 24, 3), device=dev, generator=g) * 0.4).requires_grad_(True)
    g_reg = torch.randn((B, K, 3), device=dev, generator=g)
    g_verts = torch.randn((B, body.V, 3), device=dev, generator=g) / 16

    def kernel_route(with_verts):
        out = body.differentiable(betas, pose, regressor="k", want_vertices=with_verts, joints=False)
        outs, cots = ([out.regressed, out.vertices], [g_reg, g_verts]) if with_verts else ([out.regressed], [g_reg])
        return torch.autograd.grad(outs, [betas, pose], cots)

    def torch_route(with_verts):
        gb, gp = [], []
        for i in range(0, B, a.chunk):
            b, p = betas.detach()[i:i + a.chunk].requires_grad_(True), pose.detach()[i:i + a.chunk].requires_grad_(True)
            verts, reg = torch_lbs(tm, b, p, regress, True)
            outs, cots = ([reg, verts], [g_reg[i:i + a.chunk], g_verts[i:i + a.chunk]]) if with_verts else ([reg], [g_reg[i:i + a.chunk]])
            db, dp = torch.autograd.grad(outs, [b, p], cots)
            gb.append(db)
            gp.append(dp)
        return torch.cat(gb), torch.cat(gp)

    nograd = (betas.detach(), pose.detach())
    fns = {"kernel_fwd_bwd_joints_only": lambda: kernel_route(False), "kernel_fwd_bwd_with_verts": lambda: kernel_route(True),
           "kernel_fwd_joints_only": lambda: body.forward(*nograd, regressor="k", joints=False),
           "kernel_fwd_with_verts": lambda: body.forward(*nograd, regressor="k", want_vertices=True, joints=False),
           "torch_fwd_bwd_joints_only": lambda: torch_route(False), "torch_fwd_bwd_with_verts": lambda: torch_route(True)}
    t = alternating(fns, a.window, a.warmup, a.repeats)
    res = {"B": B, "V": body.V, "NB": body.NB, "K": K, "times": t, "torch_chunk": a.chunk}
    for tag in ("joints_only", "with_verts"):
        fb, f = t[f"kernel_fwd_bwd_{tag}"]["ms_per_call"], t[f"kernel_fwd_{tag}"]["ms_per_call"]
        res[f"kernel_backward_ms_{tag}"] = fb - f
        res[f"backward_over_forward_{tag}"] = (fb - f) / f
        res[f"torch_over_kernel_fwd_bwd_{tag}"] = t[f"torch_fwd_bwd_{tag}"]["ms_per_call"] / fb
        k, w = kernel_route(tag == "with_verts"), torch_route(tag == "with_verts")
        res[f"max_rel_difference_{tag}"] = {n: float((x - y).abs().max() / y.abs().max()) for n, x, y in zip(("d_betas", "d_pose"), k, w)}
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--window", type=float, default=0.5)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--chunk", type=int, default=256)
    ap.add_argument("--sizes", type=int, nargs="*", default=[32, 1024, 35515])
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    from posegen_amd import surreal_config
    from posegen_amd.raycaster import HipRenderer
    from posegen_amd.smpl import MODEL_KEYS, BodyModel
    from posegen_amd.synthetic import make_body_model
    if not torch.cuda.is_available():
        sys.exit("bench_smpl_grad: no HIP device (there is nothing to measure on a CPU)")
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
