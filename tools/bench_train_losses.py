#!/usr/bin/env python3
"""What the trainer's losses, pose regulariser and gradient norms cost on the device route (posegen_amd.train_losses / trainer: HIP
kernels behind torch.autograd.Functions) beside (a) the same formulas as torch operators with autograd on the same device, written as
the reference's Trainer writes them (float32, `.item()` for every stat, one `norm` and one `.item()` per parameter tensor): what one
writes on top of TrainableRayCaster without this module; and, for the norms, (b) the fairest torch form: `torch._foreach_norm`, one
stack, one sync.

Shapes: 3072 and 4096 rays, the shipped settings (L1, background, BCE, coarse pass, kp_loss with tolerance and the temporal term), two
nets of 24 tensors, 256 poses in the batch.  Timed: each of the three calls forward + backward, and the whole `train_batch` (surreal
64 + 16 samples, perturb = 1, Adam over nets and poses, HipPoseOptLayer) in bf16 and fp32 with the device losses and with (a).
Method: wall-clock around a call that ends in torch.cuda.synchronize() (the host syncs are part of what is compared); the versions
alternate inside one process, after warm-up; per version the median and the min / max of the repeats.

`--count VERSION` runs `--steps` rounds of the three calls and nothing else: under `rocprofv3 --kernel-trace --memory-copy-trace` two
such runs of different length give the launches per round (and the copy records the trace holds; host syncs are counted from the code); `--traces DIR` folds the counts of such
runs (DIR/<version>_<steps>/...) into the result.  No ratio is a condition; the tool reports.  Prints one JSON line; --out writes it.

usage: bench_train_losses.py [--repeats 15] [--warmup 3] [--out profiles/train_losses.json] [--traces DIR]
       bench_train_losses.py --count hip|torch [--steps K]"""
import argparse
import glob
import json
import os
import sys
import time
from types import SimpleNamespace

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "tools"))
import numpy as np
import torch

SETTINGS = dict(loss_fn="L1", loss_beta=0.1, use_background=True, coarse_weight=1.0, reg_fn="BCE", reg_coef=0.1)
POSE = dict(tol=0.01, coef=2.0, ext_scale=0.001, temp_coef=0.05)
N_POSES = 256
# Host syncs of one round of the three calls, counted from the code below (the runtime serves a scalar's copy back without a record in
# the memory-copy trace, so the trace cannot count them): the device route fetches the photometric stats and the two norms with one
# copy each; (a) reads psnr, psnr0, alpha and MPJPC with .item() and one norm per tensor with .item() (48 tensors).
HOST_SYNCS = {"hip": 2, "torch": 3 + 1 + 48}


def timed(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3


def alternate(versions, repeats, warmup):
    """{name: {median_ms, min_ms, max_ms}}: the versions run in turn, `repeats` rounds after `warmup` rounds"""
    for _ in range(warmup):
        for fn in versions.values():
            fn()
    times = {k: [] for k in versions}
    for _ in range(repeats):
        for k, fn in versions.items():
            times[k].append(timed(fn))
    return {k: {"median_ms": float(np.median(t)), "min_ms": float(min(t)), "max_ms": float(max(t))} for k, t in times.items()}


# ---- (a): the formulas as torch operators, float32, as the reference's Trainer writes them ------------------------------------------------
def torch_photometric(preds, batch, s):
    total, stats = 0.0, {}
    for tag in ("", "0"):
        rgb, acc = preds["rgb" + tag if tag else "rgb_map"], preds["acc" + tag if tag else "acc_map"]
        pred = rgb + (1.0 - acc)[..., None] * batch["bgs"]
        loss = (pred - batch["target_s"]).abs().mean()
        if tag:
            loss = loss * s["coarse_weight"]
        stats["psnr" + tag] = -10.0 * torch.log(((pred.detach() - batch["target_s"]) ** 2).mean()) / np.log(10.0)
        y = batch["fgs"][..., 0]
        bce = -(y * torch.log(acc + 1e-8) + (1.0 - y) * torch.log(1.0 - acc + 1e-8))
        total = total + loss + bce[y < 1.0].mean() * s["reg_coef"]
    return total, stats


def torch_pose_reg(rots, kps, idx_dev, anchors, prev, nxt, temp_val):
    six = lambda r: r[..., :3, :2].flatten(start_dim=-2)
    bones = six(rots)
    x = ((six(anchors["rots"][idx_dev]) - bones) ** 2)[:, 1:]
    kp = torch.lerp(torch.zeros_like(x), x - POSE["tol"], (x > POSE["tol"]).float()).sum(-1).mean() * POSE["coef"]
    ang = (((bones - six(prev[0])) - (six(nxt[0]) - bones)) ** 2).sum(-1)
    joint = (((kps - prev[1]) - (nxt[1] - kps)) ** 2).sum(-1)
    temp = ((ang + joint) * temp_val[..., None]).mean() * POSE["temp_coef"]
    mpjpc = ((anchors["kps"][idx_dev] - kps.detach()) ** 2).sum(-1).pow(0.5).mean() / POSE["ext_scale"]
    return kp + temp, mpjpc


def torch_gradnorm_reference(params):
    total, cnt = 0.0, 0
    for p in params:
        if p.grad is None:
            continue
        total += p.grad.data.norm(2).item() ** 2
        cnt += 1
    return total ** 0.5, (total / cnt) ** 0.5


def torch_gradnorm_foreach(params):
    sq = torch.stack(torch._foreach_norm([p.grad for p in params if p.grad is not None])).double() ** 2
    total = sq.sum()
    return torch.stack([total.sqrt(), (total / sq.numel()).sqrt()]).cpu().tolist()


# ---- the three calls alone ----------------------------------------------------------------------------------------------------------------
def loss_inputs(n, dev, shapes):
    g = torch.Generator(device="cpu").manual_seed(n)
    f = lambda *s: torch.rand(*s, generator=g).to(dev)
    fgs = torch.where(f(n) < 0.4, torch.ones(n, device=dev), 0.9 * f(n))
    preds = {k: f(n, 3) if k.startswith("rgb") else f(n) for k in ("rgb_map", "acc_map", "rgb0", "acc0")}
    batch = {"target_s": f(n, 3), "bgs": f(n, 3), "fgs": fgs[:, None]}
    idx = np.random.RandomState(n).randint(0, N_POSES, n)
    anchors = {"rots": torch.randn(N_POSES, 24, 3, 3, generator=g).mul(0.5).to(dev), "kps": torch.randn(N_POSES, 24, 3, generator=g).mul(0.3).to(dev)}
    idx_dev = torch.as_tensor(idx, device=dev)
    rots = anchors["rots"][idx_dev] + 0.1 * torch.randn(n, 24, 3, 3, generator=g).to(dev)
    kps = anchors["kps"][idx_dev] + 0.02 * torch.randn(n, 24, 3, generator=g).to(dev)
    near = lambda t, s: t + s * torch.randn(t.shape, generator=g).to(dev)
    pose = dict(rots=rots, kps=kps, idx=idx, idx_dev=idx_dev, anchors=anchors, prev=(near(rots, 0.05), near(kps, 0.02)),
                nxt=(near(rots, 0.05), near(kps, 0.02)), temp_val=(f(n) > 0.3).float())
    params = [torch.nn.Parameter(torch.zeros(s, device=dev)) for s in shapes]
    for p in params:
        p.grad = torch.randn(p.shape, generator=g).to(dev)
    return preds, batch, pose, params


def call_versions(r, n, dev, shapes):
    """the three calls, forward + backward, on the device route and as torch operators: {call: {version: fn}}"""
    from posegen_amd import train_losses as tl
    preds, batch, pose, params = loss_inputs(n, dev, shapes)
    leaves = {k: v.clone().requires_grad_(True) for k, v in preds.items()}
    rots, kps = pose["rots"].clone().requires_grad_(True), pose["kps"].clone().requires_grad_(True)
    temporal = dict(prev_rots=pose["prev"][0], prev_kps=pose["prev"][1], next_rots=pose["nxt"][0], next_kps=pose["nxt"][1], temp_val=pose["temp_val"],
                    temp_coef=POSE["temp_coef"])

    def clear():
        for t in list(leaves.values()) + [rots, kps]:
            t.grad = None

    def photo_hip():
        clear()
        ld, st = tl.photometric_loss(leaves, batch, renderer=r, **SETTINGS)
        ld["total_loss"].backward()
        return torch.stack([ld["total_loss"].detach(), st["psnr"], st["psnr0"], st["alpha"]]).cpu()      # the stats: one copy

    def photo_torch():
        clear()
        total, st = torch_photometric(leaves, batch, SETTINGS)
        total.backward()
        return [st["psnr"].item(), st["psnr0"].item(), leaves["acc_map"].mean().item()]                   # the reference's three .item()

    def reg_hip():
        clear()
        total, terms = tl.pose_regulariser(rots, kps, pose["idx"], pose["anchors"], tol=POSE["tol"], coef=POSE["coef"], ext_scale=POSE["ext_scale"],
                                           temporal=temporal, renderer=r)
        total.backward()
        return terms["MPJPC"]

    def reg_torch():
        clear()
        total, mpjpc = torch_pose_reg(rots, kps, pose["idx_dev"], pose["anchors"], pose["prev"], pose["nxt"], pose["temp_val"])
        total.backward()
        return mpjpc.item()

    return {"photometric": {"hip": photo_hip, "torch": photo_torch}, "pose_regulariser": {"hip": reg_hip, "torch": reg_torch},
            "grad_norms": {"hip": lambda: torch.stack(tl.grad_norms(params, r)[:2]).cpu().tolist(), "torch": lambda: torch_gradnorm_reference(params),
                           "torch_foreach": lambda: torch_gradnorm_foreach(params)}}


# ---- the whole step ------------------------------------------------------------------------------------------------------------------------
def step_versions(precision, n, dev):
    from bench import full_frame_rays
    from bench_poseopt import pose_parameters
    from posegen_amd import surreal_config, synthetic as syn
    from posegen_amd.batches import RayBatch
    from posegen_amd.poseopt import HipPoseOptLayer
    from posegen_amd.raycaster import HipRayCaster
    from posegen_amd.train import TrainableRayCaster
    from posegen_amd.trainer import HipTrainer, temporal_indices
    cfg = surreal_config()
    m = TrainableRayCaster(HipRayCaster.from_weights(cfg, *syn.make_model(cfg, 0), device=dev, precision="bf16"), train_precision=precision, opt_pose=True)
    m.train()
    rb, _, cyl, *_ = full_frame_rays(512, 512, dev)
    rb = rb[torch.linspace(0, rb.shape[0] - 1, n, device=dev).long()].contiguous()
    pelvis, bones, rest, kp_idx = pose_parameters()
    kp_idx = np.asarray(kp_idx[:n], dtype=np.int64)
    g = torch.Generator(device="cpu").manual_seed(3)
    f = lambda *s: torch.rand(*s, generator=g).to(dev)
    batch = RayBatch(rays=torch.stack([rb[:, :3], rb[:, 3:6]]).contiguous(), target_s=f(n, 3), bgs=f(n, 3),
                     fgs=torch.where(f(n) < 0.4, torch.ones(n, device=dev), 0.9 * f(n))[:, None], cyls=cyl,
                     kp_idx=torch.as_tensor(kp_idx, device=dev), temp_val=(f(n) > 0.3).float())
    batch.kp_idx_host = kp_idx
    args = SimpleNamespace(loss_fn="L1", loss_beta=0.1, reg_fn="BCE", reg_coef=0.1, use_background=True, coarse_weight=1.0, opt_pose=True, opt_pose_stop=None,
                           opt_pose_step=1, opt_pose_tol=POSE["tol"], opt_pose_coef=POSE["coef"], opt_rot6d=True, opt_pose_cache=False, use_temp_loss=True,
                           temp_coef=POSE["temp_coef"], ext_scale=POSE["ext_scale"], opt_framecode=False, chunk=4096, lrate=5e-4, lrate_decay=500,
                           lrate_decay_rate=0.1, decay_unit=1000, finetune=True)
    kw = dict(ray_caster=m, N_samples=cfg.n_samples, N_importance=cfg.n_importance, perturb=1.0, raw_noise_std=1.0, near=rb[:, 6:7].contiguous(),
              far=rb[:, 7:8].contiguous())
    sd = {"pelvis": torch.tensor(pelvis), "bones": torch.tensor(bones), "rest_pose": torch.tensor(rest)}

    class TorchLossTrainer(HipTrainer):
        """(a): HipTrainer with the losses and norms as torch operators, stats by .item() as the reference reads them"""

        def compute_loss(self, batch, preds, kp_opts=None, popt_detach=False):
            total, stats = torch_photometric(preds, batch, SETTINGS)
            layer = self.popt_kwargs["popt_layer"]
            prev, nxt = temporal_indices(batch.kp_idx_host, layer.N_kps)
            with torch.no_grad():
                pk, _, _, _, pr = layer(prev)
                nk, _, _, _, nr = layer(nxt)
            reg, mpjpc = torch_pose_reg(kp_opts["rots"], kp_opts["kp_batch"], batch["kp_idx"], self.popt_kwargs["popt_anchors"], (pr, pk), (nr, nk),
                                        batch["temp_val"])
            self.host_stats = {k: v.item() for k, v in stats.items()}
            self.host_stats["MPJPC"] = mpjpc.item()
            self.host_stats["alpha"] = preds["acc_map"].mean().item()
            total = total + reg
            return {"total_loss": total}, {}

        def optimize(self, loss, i, popt_detach=False):
            loss.backward()
            self.host_stats["total_norm"], self.host_stats["avg_norm"] = torch_gradnorm_reference(self.ray_caster.parameters())
            self.optimizer.step()
            self.optimizer.zero_grad()
            self.optim_steps += 1
            self.pose_optimizer.step()
            self.pose_optimizer.zero_grad()
            return {}

    versions = {}
    for name, cls in (("hip", HipTrainer), ("torch", TorchLossTrainer)):
        layer = HipPoseOptLayer.from_state_dict(sd, renderer=m.renderer)
        with torch.no_grad():
            a_kps, _, _, _, a_rots = layer(np.arange(layer.N_kps))
        anchors = {"rots": a_rots.clone(), "kps": a_kps.clone()}
        opt = torch.optim.Adam([p for p in m.parameters() if p.requires_grad], lr=5e-4)
        popt = torch.optim.Adam(list(layer.parameters()), lr=5e-4)
        tr = cls(args, {"hwf": (512, 512, 500.0)}, opt, popt, kw, {}, popt_kwargs={"popt_layer": layer, "popt_anchors": anchors})
        versions[name] = lambda tr=tr: tr.train_batch(batch, i=0, global_step=0)
    return versions, m


def count_run(version, steps, dev):
    from posegen_amd import surreal_config
    from posegen_amd.raycaster import HipRenderer
    r = HipRenderer(surreal_config(), device=dev)
    calls = call_versions(r, 4096, dev, net_shapes())
    for _ in range(steps):
        for c in calls.values():
            c[version]()
    torch.cuda.synchronize()
    r.close()


def net_shapes():
    """the 24 tensors of one surreal net, twice"""
    from posegen_amd import surreal_config, synthetic as syn
    wc, wf, _, _ = syn.make_model(surreal_config(), 0)
    return [tuple(np.asarray(v).shape) for w in (wc, wf) for v in w.values()]


def fold_traces(root):
    """launches and device-to-host copies per round of the three calls from rocprofv3 runs of two lengths per version"""
    out = {}
    for version in ("hip", "torch"):
        runs = {}
        for d in glob.glob(os.path.join(root, f"{version}_*")):
            steps = int(d.rsplit("_", 1)[1])
            k = sum(max(0, sum(1 for _ in open(p)) - 1) for p in glob.glob(os.path.join(d, "**", "*kernel_trace.csv"), recursive=True))
            c = sum(sum("DEVICE_TO_HOST" in line.upper() for line in open(p)) for p in glob.glob(os.path.join(d, "**", "*memory_copy_trace.csv"), recursive=True))
            runs[steps] = (k, c)
        if len(runs) >= 2:
            (s0, (k0, c0)), (s1, (k1, c1)) = sorted(runs.items())[0], sorted(runs.items())[-1]
            out[version] = {"kernel_launches_per_round": (k1 - k0) / (s1 - s0), "device_to_host_copy_records_per_round": (c1 - c0) / (s1 - s0),
                            "host_syncs_per_round_from_the_code": HOST_SYNCS[version], "from_runs_of_rounds": [s0, s1]}
    return out or "not measured"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=15)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default="")
    ap.add_argument("--traces", default="")
    ap.add_argument("--count", default="")
    ap.add_argument("--steps", type=int, default=4)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("bench_train_losses: no HIP device (there is nothing to measure on a CPU)")
    dev = torch.device("cuda:0")
    if a.count:
        return count_run(a.count, a.steps, dev)
    from posegen_amd import surreal_config
    from posegen_amd.raycaster import HipRenderer
    res = {"device": torch.cuda.get_device_name(0), "repeats": a.repeats, "warmup": a.warmup, "n_poses": N_POSES, "calls": {}, "train_batch": {}}
    r = HipRenderer(surreal_config(), device=dev)
    shapes = net_shapes()
    res["n_tensors"] = len(shapes)
    for n in (3072, 4096):
        res["calls"][str(n)] = {call: alternate(v, a.repeats, a.warmup) for call, v in call_versions(r, n, dev, shapes).items()}
    r.close()
    for precision in ("bf16", "fp32"):
        for n in (3072, 4096):
            versions, m = step_versions(precision, n, dev)
            t = alternate(versions, a.repeats, a.warmup)
            t["torch_over_hip"] = t["torch"]["median_ms"] / t["hip"]["median_ms"]
            res["train_batch"][f"{precision}_{n}"] = t
            m.renderer.close()
    res["launches"] = fold_traces(a.traces) if a.traces else "not measured"
    line = json.dumps(res)
    print(line, flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
