#!/usr/bin/env python3
"""Time of the optimiser step: `HipAdam.step(max_norm=1)` -- one pg_adam_step call -- beside `clip_grad_norm_` +
`torch.optim.Adam.step()` with torch's defaults, and the same with `fused=True`, on the same device.

Four parameter sets built from shape lists (no model files): the two A-NeRF nets of `get_grad_vars`, `HipPos3dDiscriminator`,
`HipPoseGenerator`, and the HMR regressor (ResNet-50 trunk shapes plus the head).  Each route owns a copy of the set with the same
fixed gradients.  Also `ganloop.generator_step` and `ganloop.discriminator_step` at B = 1024 with a `HipAdam` and with a
`torch.optim.Adam`.

The routes alternate within one process: after `--warmup` calls each, `--windows` windows; in a window every route in turn runs
`--calls` calls between two device events and ends in a synchronise; the figure is the median window, with the fastest and the
slowest.  The host time to enqueue a call (the calls of a window, before the synchronise) is reported separately.  For the device
route the bytes moved per element (4 read by the norm, 16 read and 12 written by the update) and the share of the HBM peak they amount
to are reported; a set that fits the last-level cache does not measure HBM.  No ratio is a condition; the tool reports, including
the sets where the device route loses.  Prints one JSON line; --out writes it to a file.

usage: bench_optim.py [--windows 3] [--calls 20] [--warmup 5] [--out profiles/optimizer_step.json]"""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch

from tools.bench_pose_losses import OpCounter

HBM_PEAK_GBS = 8000.0            # MI355X: 8 TB/s
BYTES_PER_ELEMENT = 4 + 16 + 12  # clipped step without write_grads


def resnet50_shapes():
    shapes = [(64, 3, 7, 7), (64,), (64,)]
    inplanes = 64
    for planes, blocks in ((64, 3), (128, 4), (256, 6), (512, 3)):
        for b in range(blocks):
            shapes += [(planes, inplanes, 1, 1), (planes,), (planes,), (planes, planes, 3, 3), (planes,), (planes,),
                       (planes * 4, planes, 1, 1), (planes * 4,), (planes * 4,)]
            if b == 0:
                shapes += [(planes * 4, inplanes, 1, 1), (planes * 4,), (planes * 4,)]
            inplanes = planes * 4
    return shapes


def parameter_sets(renderer):
    from posegen_amd import discriminators, generators, regressors, surreal_config, synthetic
    nerf = []
    for _ in range(2):
        for _, out, inp in synthetic.layer_shapes(surreal_config()):
            nerf += [(out, inp), (out,)]
    module_shapes = lambda m: [tuple(p.shape) for p in m.parameters() if p.requires_grad]
    return {"anerf_two_nets": nerf,
            "pos3d_discriminator": module_shapes(discriminators.HipPos3dDiscriminator(renderer)),
            "pose_generator": module_shapes(generators.HipPoseGenerator(renderer=renderer)),
            "hmr_regressor_resnet50": resnet50_shapes() + module_shapes(regressors.HipHMRHead(renderer=renderer))}


def windows(fns, n_windows, calls, warmup):
    """per fn: {device ms per call (median window, min, max), host enqueue ms per call (median window)}"""
    for fn in fns:
        for _ in range(warmup):
            fn()
    torch.cuda.synchronize()
    dev, host = [[] for _ in fns], [[] for _ in fns]
    for _ in range(n_windows):
        for i, fn in enumerate(fns):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            t0 = time.perf_counter()
            e0.record()
            for _ in range(calls):
                fn()
            e1.record()
            t1 = time.perf_counter()
            torch.cuda.synchronize()
            dev[i].append(e0.elapsed_time(e1) / calls)
            host[i].append((t1 - t0) * 1e3 / calls)
    med = lambda t: float(sorted(t)[len(t) // 2])
    return [{"ms_per_call": med(d), "min_ms": float(min(d)), "max_ms": float(max(d)), "host_enqueue_ms_per_call": med(h), "windows": n_windows,
             "calls_per_window": calls} for d, h in zip(dev, host)]


def ops_of(fn):
    with OpCounter() as c:
        fn()
    torch.cuda.synchronize()
    return c.n


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--windows", type=int, default=3)
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("bench_optim: no HIP device (there is nothing to measure on a CPU)")
    from posegen_amd import discriminators, ganloop, generators, optim, pose_eval
    dev = torch.device("cuda:0")
    renderer = pose_eval.default_scorer(dev).renderer
    g = torch.Generator(device=dev).manual_seed(1)
    sets = []
    for name, shapes in parameter_sets(renderer).items():
        def copy_of():
            gg = torch.Generator(device=dev).manual_seed(2)
            ps = [torch.nn.Parameter(0.05 * torch.randn(s, device=dev, generator=gg)) for s in shapes]
            for p in ps:
                p.grad = 0.01 * torch.randn(p.shape, device=dev, generator=gg)
            return ps
        p_hip, p_adam, p_fused = copy_of(), copy_of(), copy_of()
        hip = optim.HipAdam(p_hip, lr=1e-5, renderer=renderer)
        adam, fused = torch.optim.Adam(p_adam, lr=1e-5), torch.optim.Adam(p_fused, lr=1e-5, fused=True)

        def route(ps, opt):
            def run():
                torch.nn.utils.clip_grad_norm_(ps, max_norm=1.0)
                opt.step()
            return run
        fns = [lambda: hip.step(max_norm=1.0), route(p_adam, adam), route(p_fused, fused)]
        n = sum(p.numel() for p in p_hip)
        info = {"set": name, "tensors": len(shapes), "elements": n,
                "torch_ops_on_the_calling_thread": dict(zip(("hipadam", "clip_adam", "clip_adam_fused"), (ops_of(f) for f in fns)))}
        info["hipadam"], info["clip_adam"], info["clip_adam_fused"] = windows(fns, a.windows, a.calls, a.warmup)
        ms = info["hipadam"]["ms_per_call"]
        info["hipadam"]["bytes_per_element"] = BYTES_PER_ELEMENT
        info["hipadam"]["gb_per_s"] = n * BYTES_PER_ELEMENT / (ms * 1e-3) / 1e9
        info["hipadam"]["share_of_hbm_peak"] = info["hipadam"]["gb_per_s"] / HBM_PEAK_GBS
        info["clip_adam_over_hipadam"] = info["clip_adam"]["ms_per_call"] / ms
        info["clip_adam_fused_over_hipadam"] = info["clip_adam_fused"]["ms_per_call"] / ms
        sets.append(info)
        del p_hip, p_adam, p_fused, hip, adam, fused
        torch.cuda.empty_cache()

    # the two step helpers of the adversarial loop with both optimisers
    B = 1024
    real = torch.randn((B, 24, 3), device=dev, generator=g)
    fake = 0.5 * torch.randn((B, 24, 3), device=dev, generator=g)
    helpers = []

    def twins(make):
        torch.manual_seed(0)
        m1, m2 = make().to(dev).train(), make().to(dev).train()
        m2.load_state_dict(m1.state_dict())
        return m1, m2
    d1, d2 = twins(lambda: discriminators.HipPos3dDiscriminator(renderer))
    o1, o2 = optim.HipAdam(d1.parameters(), lr=1e-4, renderer=renderer), torch.optim.Adam(d2.parameters(), lr=1e-4)
    pool1, pool2 = discriminators.FakePool(4096, renderer), discriminators.FakePool(4096, renderer)
    import numpy as np
    rng1, rng2 = np.random.RandomState(1), np.random.RandomState(1)
    fns = [lambda: ganloop.discriminator_step(d1, o1, real, fake, pool1, rng1), lambda: ganloop.discriminator_step(d2, o2, real, fake, pool2, rng2)]
    info = {"helper": "discriminator_step", "B": B, "torch_ops_on_the_calling_thread": dict(zip(("hipadam", "torch_adam"), (ops_of(f) for f in fns)))}
    info["hipadam"], info["torch_adam"] = windows(fns, a.windows, a.calls, a.warmup)
    info["torch_adam_over_hipadam"] = info["torch_adam"]["ms_per_call"] / info["hipadam"]["ms_per_call"]
    helpers.append(info)

    frozen = discriminators.HipPos3dDiscriminator(renderer).to(dev)
    for p in frozen.parameters():
        p.requires_grad_(False)
    g1, g2 = twins(lambda: generators.HipPoseGenerator(renderer=renderer))
    o1g, o2g = optim.HipAdam(g1.parameters(), lr=1e-4, renderer=renderer), torch.optim.Adam(g2.parameters(), lr=1e-4)
    fns = [lambda: ganloop.generator_step(g1, frozen, o1g, real), lambda: ganloop.generator_step(g2, frozen, o2g, real)]
    info = {"helper": "generator_step", "B": B, "torch_ops_on_the_calling_thread": dict(zip(("hipadam", "torch_adam"), (ops_of(f) for f in fns)))}
    info["hipadam"], info["torch_adam"] = windows(fns, a.windows, a.calls, a.warmup)
    info["torch_adam_over_hipadam"] = info["torch_adam"]["ms_per_call"] / info["hipadam"]["ms_per_call"]
    helpers.append(info)

    out = {"sets": sets, "helpers": helpers, "windows": a.windows, "calls_per_window": a.calls, "warmup": a.warmup,
           "hbm_peak_gb_per_s": HBM_PEAK_GBS, "device": torch.cuda.get_device_name(0)}
    line = json.dumps(out)
    print(line, flush=True)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
