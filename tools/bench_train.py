"""Time of one training step (bench.py train_step_rate) in both training precisions, for profiling runs.

usage: bench_train.py [bf16] [fp32]            the bench line's training step
       bench_train.py --pose [bf16] [fp32] [--only-pose] [--steps K]
                                              the same step with and without pose refinement (opt_pose): one line per
                                              (precision, opt_pose) with ms per step, on one device in one process
       bench_train.py --single [bf16] [fp32] [--steps K]
                                              the single-net step (configs/surreal/surreal_single.txt: one net, 96 + 48, 4096 rays)
                                              beside the two-net step at 96 + 48, same device, same process: one line each"""
import json, os, sys, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
from bench import full_frame_rays, train_step_rate


def pose_step_ms(dev, precision, opt_pose, n_rand=4096, steps=7, warmup=2):
    """train_step_rate's step (surreal 64 + 16, perturb = 1, raw_noise_std = 1, both maps' MSE, Adam) with the frame's pose as a
    parameter: opt_pose=True hands the caster skts expanded to one pose per ray, as PoseOptLayer does by kp_idx
    (core/trainer.py:286-313), with the pose in the optimiser; False: the same loop with the pose detached."""
    from posegen_amd import surreal_config, synthetic as syn
    from posegen_amd.raycaster import HipRayCaster
    from posegen_amd.train import TrainableRayCaster
    cfg = surreal_config()
    c = HipRayCaster.from_weights(cfg, *syn.make_model(cfg, 0), device=dev, precision="bf16")
    m = TrainableRayCaster(c, train_precision=precision, opt_pose=opt_pose)
    m.train()
    rb, skts, cyl, *_ = full_frame_rays(512, 512, dev)
    sel = torch.linspace(0, rb.shape[0] - 1, n_rand, device=dev).long()
    rb = rb[sel].contiguous()
    target = torch.rand(n_rand, 3, device=dev)
    pose = skts.reshape(1, 24, 4, 4).clone().requires_grad_(opt_pose)
    params = [p for p in m.parameters() if p.requires_grad] + ([pose] if opt_pose else [])
    opt = torch.optim.Adam(params, lr=5e-4, betas=(0.9, 0.999))

    def step():
        opt.zero_grad()
        out = m(rb, N_samples=cfg.n_samples, skts=pose.expand(n_rand, -1, -1, -1), cyls=cyl, N_importance=cfg.n_importance,
                perturb=1., raw_noise_std=1.)
        loss = torch.mean((out["rgb_map"] + (1. - out["acc_map"])[..., None] - target) ** 2) \
            + torch.mean((out["rgb0"] + (1. - out["acc0"])[..., None] - target) ** 2)
        loss.backward()
        opt.step()
        return loss

    for _ in range(warmup):
        step()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(steps):
        loss = step()
    torch.cuda.synchronize()
    ms = (time.perf_counter() - t0) * 1e3 / steps
    m.renderer.close()
    return {"precision": precision, "opt_pose": opt_pose, "n_rand": n_rand, "n_samples": cfg.n_samples,
            "n_importance": cfg.n_importance, "ms_per_step": ms, "steps": steps, "warmup": warmup, "loss": float(loss.detach())}


def single_step_ms(dev, precision, single, n_rand=4096, steps=7, warmup=2):
    """One Adam step at 96 + 48 samples, perturb = 1, raw_noise_std = 1, both maps' MSE: the shipped single-net model
    (make_trainable -> SingleNetTrainableRayCaster: 144 rows of MLP work per ray) or two nets at the same sample counts (240)."""
    from posegen_amd import make_trainable, surreal_config, surreal_single_config, synthetic as syn
    from posegen_amd.raycaster import HipRayCaster
    cfg = surreal_single_config() if single else surreal_config(n_samples=96, n_importance=48)
    wc, wf, tv, td = syn.make_model(cfg, 0)
    c = HipRayCaster.from_weights(cfg, wc, None if single else wf, tv, td, device=dev, precision="bf16")
    m = make_trainable(c, train_precision=precision)
    m.train()
    rb, skts, cyl, *_ = full_frame_rays(512, 512, dev)
    sel = torch.linspace(0, rb.shape[0] - 1, n_rand, device=dev).long()
    rb = rb[sel].contiguous()
    target = torch.rand(n_rand, 3, device=dev)
    opt = torch.optim.Adam([p for p in m.parameters() if p.requires_grad], lr=5e-4, betas=(0.9, 0.999))

    def step():
        opt.zero_grad()
        out = m(rb, N_samples=cfg.n_samples, skts=skts, cyls=cyl, N_importance=cfg.n_importance, perturb=1., raw_noise_std=1.)
        loss = torch.mean((out["rgb_map"] + (1. - out["acc_map"])[..., None] - target) ** 2) \
            + torch.mean((out["rgb0"] + (1. - out["acc0"])[..., None] - target) ** 2)
        loss.backward()
        opt.step()
        return loss

    for _ in range(warmup):
        step()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(steps):
        loss = step()
    torch.cuda.synchronize()
    ms = (time.perf_counter() - t0) * 1e3 / steps
    m.renderer.close()
    return {"model": "single_net" if single else "two_nets", "precision": precision, "n_rand": n_rand, "n_samples": cfg.n_samples,
            "n_importance": cfg.n_importance, "mlp_rows_per_ray": cfg.evals_per_ray(), "ms_per_step": ms, "steps": steps, "warmup": warmup,
            "loss": float(loss.detach())}


if __name__ == "__main__":
    args = sys.argv[1:]
    steps = 7
    if "--steps" in args:
        i = args.index("--steps")
        steps = int(args[i + 1])
        del args[i:i + 2]
    if "--single" in args:
        for prec in [a for a in args if not a.startswith("--")] or ["fp32", "bf16"]:
            two = single_step_ms(torch.device("cuda:0"), prec, False, steps=steps)
            one = single_step_ms(torch.device("cuda:0"), prec, True, steps=steps)
            one["ratio_to_two_nets"] = one["ms_per_step"] / two["ms_per_step"]
            print(json.dumps(two), flush=True)
            print(json.dumps(one), flush=True)
    elif "--pose" in args:
        only = "--only-pose" in args
        precs = [a for a in args if not a.startswith("--")] or ["bf16", "fp32"]
        base = {}
        for prec in precs:
            for opt_pose in ((True,) if only else (False, True)):
                r = pose_step_ms(torch.device("cuda:0"), prec, opt_pose, steps=steps)
                if opt_pose and prec in base:
                    r["ratio_to_no_pose"] = r["ms_per_step"] / base[prec]
                else:
                    base[prec] = r["ms_per_step"]
                print(json.dumps(r), flush=True)
    else:
        for prec in args or ["bf16", "fp32"]:
            r = train_step_rate(torch.device("cuda:0"), steps=steps, precision=prec)
            print(prec, json.dumps({k: v for k, v in r.items() if k != "what"}))
