"""What the pose layer costs in a pose-refinement training step: tools/bench_train.py's step (surreal 64 + 16, 4096 rays, perturb = 1,
raw_noise_std = 1, both maps' MSE, Adam over the nets and the pose parameters) with the poses coming out of a pose layer by kp_idx,
as in the reference (core/trainer.py:286-313): 4096 rays drawn from 256 of 1000 poses.  The layer is
  (a) "torch": the reference layer restated in torch on the device (tests/poseopt_ref.TorchPoseOptLayer: about a hundred small
      launches forward, autograd's transpose of them backward, the gather's backward an atomic scatter-add), or
  (b) "hip":   HipPoseOptLayer (pg_poseopt_forward / pg_poseopt_backward).
Both run in one process, alternating, in both training precisions: per (precision, layer) the median step time of `--steps` (10) runs
after `--warmup` (2), the layer's own forward + backward time (same cotangents, no render), and whether two runs of the layer on the
same input give the same bones.grad bytes.  One JSON line each, appended to profiles/poseopt_step.jsonl (--out).

usage: bench_poseopt.py [bf16] [fp32] [--steps K] [--warmup W] [--out FILE]"""
import json, os, sys, time
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
import numpy as np
import torch

N_RAND, N_POSES, N_BATCH_POSES = 4096, 1000, 256


def pose_parameters(seed=0):
    """1000 poses around the benchmark frame's: (pelvis [N,3], 6-D bones [N,24,6], rest [1,24,3]) and kp_idx [4096] over 256 of them"""
    from posegen_amd import synthetic as syn
    from posegen_amd.poseopt import axisang_to_rot6d
    from posegen_amd.skeleton import SURREAL_REST_SCALE, smpl_rest_pose
    rng = np.random.RandomState(seed)
    bones, kps, _ = syn.make_pose(1, 1)
    aa = bones + rng.normal(0, 0.01, (N_POSES, 24, 3)).astype(np.float32)
    pelvis = (kps[:, 0] + rng.normal(0, 0.005, (N_POSES, 3))).astype(np.float32)
    rest = (smpl_rest_pose * SURREAL_REST_SCALE).astype(np.float32)[None]
    kp_idx = rng.choice(N_POSES, N_BATCH_POSES, replace=False)[rng.randint(0, N_BATCH_POSES, N_RAND)]
    return pelvis, axisang_to_rot6d(aa), rest, kp_idx


def make_layer(kind, renderer, params, dev):
    from posegen_amd.poseopt import HipPoseOptLayer
    from tests.poseopt_ref import TorchPoseOptLayer
    pelvis, bones, rest, _ = params
    if kind == "torch":
        return TorchPoseOptLayer(pelvis, bones, rest, device=dev)
    sd = {"pelvis": torch.tensor(pelvis), "bones": torch.tensor(bones), "rest_pose": torch.tensor(rest)}
    return HipPoseOptLayer.from_state_dict(sd, renderer=renderer)


def median_ms(fn, steps, warmup):
    for _ in range(warmup):
        fn()
    times = []
    for _ in range(steps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        times.append((time.perf_counter() - t0) * 1e3)
    return float(np.median(times)), times


def run(precision, steps, warmup, dev):
    from bench import full_frame_rays
    from posegen_amd import surreal_config, synthetic as syn
    from posegen_amd.raycaster import HipRayCaster
    from posegen_amd.train import TrainableRayCaster
    cfg = surreal_config()
    c = HipRayCaster.from_weights(cfg, *syn.make_model(cfg, 0), device=dev, precision="bf16")
    m = TrainableRayCaster(c, train_precision=precision, opt_pose=True)
    m.train()
    rb, _, cyl, *_ = full_frame_rays(512, 512, dev)
    rb = rb[torch.linspace(0, rb.shape[0] - 1, N_RAND, device=dev).long()].contiguous()
    target = torch.rand(N_RAND, 3, device=dev)
    params = pose_parameters()
    kp_idx = params[3]
    gen = torch.Generator(device="cpu").manual_seed(1)
    cot = [torch.randn(s, generator=gen).to(dev) for s in ((N_RAND, 24, 3), (N_RAND, 24, 4, 4), (N_RAND, 24, 4, 4), (N_RAND, 24, 3, 3))]
    kinds = ("torch", "hip")
    layers = {k: make_layer(k, m.renderer, params, dev) for k in kinds}
    opts = {k: torch.optim.Adam([p for p in m.parameters() if p.requires_grad] + list(layers[k].parameters()), lr=5e-4) for k in kinds}

    def train_step(k):
        opts[k].zero_grad()
        skts = layers[k](kp_idx)[2]
        out = m(rb, N_samples=cfg.n_samples, skts=skts, cyls=cyl, N_importance=cfg.n_importance, perturb=1., raw_noise_std=1.)
        loss = torch.mean((out["rgb_map"] + (1. - out["acc_map"])[..., None] - target) ** 2) \
            + torch.mean((out["rgb0"] + (1. - out["acc0"])[..., None] - target) ** 2)
        loss.backward()
        opts[k].step()
        return loss

    def layer_only(k):
        layers[k].zero_grad(set_to_none=True)
        kps, _, skts, l2ws, rots = layers[k](kp_idx)
        ((kps * cot[0]).sum() + (skts * cot[1]).sum() + (l2ws * cot[2]).sum() + (rots * cot[3]).sum()).backward()
        return layers[k].bones.grad

    # the layer alone first (the parameters still at their initial values), then the whole step; the two layers alternate run by run
    res = {k: {} for k in kinds}
    for k in kinds:
        a = layer_only(k).detach().cpu().numpy().tobytes()
        b = layer_only(k).detach().cpu().numpy().tobytes()
        res[k]["bones_grad_repeatable"] = a == b
    for k in kinds:
        for _ in range(warmup):
            layer_only(k); train_step(k)
    lt, st = {k: [] for k in kinds}, {k: [] for k in kinds}
    for _ in range(steps):
        for k in kinds:
            lt[k].append(median_ms(lambda: layer_only(k), 1, 0)[0])
            st[k].append(median_ms(lambda: train_step(k), 1, 0)[0])
    m.renderer.close()
    for k in kinds:
        res[k].update(precision=precision, layer=k, n_rand=N_RAND, n_poses=N_POSES, n_batch_poses=N_BATCH_POSES, n_samples=cfg.n_samples,
                      n_importance=cfg.n_importance, steps=steps, warmup=warmup, ms_per_step=float(np.median(st[k])),
                      layer_fwd_bwd_ms=float(np.median(lt[k])))
    return [res[k] for k in kinds]


if __name__ == "__main__":
    args = sys.argv[1:]
    opt = {"--steps": 10, "--warmup": 2, "--out": os.path.join(REPO, "profiles", "poseopt_step.jsonl")}
    for key in list(opt):
        if key in args:
            i = args.index(key)
            opt[key] = type(opt[key])(args[i + 1])
            del args[i:i + 2]
    lines = []
    for prec in args or ["bf16", "fp32"]:
        for r in run(prec, opt["--steps"], opt["--warmup"], torch.device("cuda:0")):
            print(json.dumps(r), flush=True)
            lines.append(json.dumps(r))
    os.makedirs(os.path.dirname(opt["--out"]), exist_ok=True)
    with open(opt["--out"], "a") as f:
        f.write("\n".join(lines) + "\n")
