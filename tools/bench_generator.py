#!/usr/bin/env python3
"""Time of the pose generator of one GAN batch (run_gan.py:2001-2107) on the device route (posegen_amd.generators: pg_gen_trunk_forward /
pg_gen_ba_head_forward / pg_gen_rt_head and their backwards behind one torch.autograd.Function) beside the SAME modules -- the same
nn.Linear / nn.BatchNorm1d children -- run as stock float32 torch operators on the same device (generators.stock_forward).

  case 1, the generator forward alone: B = 1024 poses, training mode, under no_grad;
  case 2, the whole generator step: zero_grad, generate, 0.5 mse(D(pose_ba), 1) against a frozen HipPos3dDiscriminator (the device
          discriminator on both routes), backward, clip_grad_norm_, Adam -- `ganloop.generator_step`, and the same lines around
          stock_forward.
The forward alone takes draws made once, outside the timed calls, on both routes; the step draws its own noise on both routes, as
the reference does (four torch.randn calls a step).  The two routes alternate within the run: `--rounds`
windows each after `--warmup` calls, HIP events around batches of calls that end in a synchronise.  Launches: the library's kernels
are counted from the calls that are made (pg_gen_trunk_forward: one per layer; the heads one each; pg_gen_ba_head_backward 1 + one
per wanted product; pg_gen_trunk_backward one per layer + one grouped); what torch launches besides is counted as
tools/bench_pose_losses.py counts it.  No ratio is a condition; the tool reports.  Prints one JSON line; --out writes it to a file.

usage: bench_generator.py [--window 0.4] [--rounds 3] [--warmup 3] [--out profiles/pose_generator.json]"""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch

from tools.bench_discriminators import alternating_windows
from tools.bench_pose_losses import OpCounter

B = 1024


class LibraryKernels:
    """the kernels behind the _ffi.call sites made while active"""

    def __init__(self):
        self.n, self.calls = 0, {}

    def __enter__(self):
        from posegen_amd import _ffi
        self._ffi, self._real = _ffi, _ffi.call

        def spy(r, name, *args):
            k = {"pg_gen_ba_head_forward": 1, "pg_gen_rt_head": 1, "pg_disc_forward": 5, "pg_disc_loss": 1}.get(name, 0)
            if name in ("pg_gen_trunk_forward", "pg_gen_trunk_backward"):
                spec = args[0]._obj
                k = max(1 + 2 * spec.trunk[t].n_stages for t in range(spec.n_trunks)) + (name.endswith("backward") and args[-1] is not None)
            if name == "pg_gen_ba_head_backward":
                k = 1 + (args[-1] is not None) + (args[-2] is not None or args[-3] is not None)
            if name == "pg_disc_backward":
                k = (6 if args[-2] is not None else 4) + (5 if args[-1] is not None else 0)
            self.n += int(k)
            self.calls[name] = self.calls.get(name, 0) + 1
            return self._real(r, name, *args)
        _ffi.call = spy
        return self

    def __exit__(self, *exc):
        self._ffi.call = self._real


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--window", type=float, default=0.4)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("bench_generator: no HIP device (there is nothing to measure on a CPU)")
    from posegen_amd import discriminators as disc, ganloop, generators as gen
    dev = torch.device("cuda:0")
    g = torch.Generator(device=dev).manual_seed(1)
    real = 0.6 * torch.randn((B, 24, 3), device=dev, generator=g)
    noise = {k: torch.randn((B, n), device=dev, generator=g) for k, n in (("ba", 32), ("r", 72), ("eps", 3), ("t", 72))}

    def model():
        torch.manual_seed(0)
        m = gen.HipPoseGenerator().to(dev).train()
        m.apply(lambda mod: torch.nn.init.kaiming_normal_(mod.weight) if isinstance(mod, torch.nn.Linear) else None)
        return m
    g_dev, g_stock = model(), model()
    torch.manual_seed(0)
    d = disc.HipPos3dDiscriminator().to(dev)
    d.apply(lambda mod: torch.nn.init.kaiming_normal_(mod.weight) if isinstance(mod, torch.nn.Linear) else None)
    for t in d.parameters():
        t.requires_grad_(False)
    cases = []

    # case 1: the forward alone
    def fwd_ours():
        with torch.no_grad():
            return g_dev(real, noise=noise)

    def fwd_stock():
        with torch.no_grad():
            return gen.stock_forward(g_stock, real, noise)
    o, s = fwd_ours(), fwd_stock()
    info = dict(name="generator forward (training mode, no_grad)", B=B,
                max_abs_difference={k: float((o[k] - s[k]).abs().max()) for k in ("pose_ba", "R", "T", "pose_rt")})
    with LibraryKernels() as lk:
        with OpCounter() as c:
            fwd_ours()
        torch.cuda.synchronize()
    info["launches"] = {"library_kernels": lk.n, "library_calls": lk.calls, "torch_ops_on_the_calling_thread": c.n}
    with OpCounter() as c:
        fwd_stock()
    torch.cuda.synchronize()
    info["launches_torch"] = {"torch_ops_on_the_calling_thread": c.n}
    info["device_route"], info["torch_route"] = alternating_windows([fwd_ours, fwd_stock], a.window, a.rounds, a.warmup)
    info["torch_over_device"] = info["torch_route"]["ms_per_call"] / info["device_route"]["ms_per_call"]
    cases.append(info)

    # case 2: the generator step
    opt_dev, opt_stock = torch.optim.Adam(g_dev.parameters(), lr=1e-4), torch.optim.Adam(g_stock.parameters(), lr=1e-4)

    def step_ours():
        return ganloop.generator_step(g_dev, d, opt_dev, real)[1]

    def step_stock():
        opt_stock.zero_grad()
        out = gen.stock_forward(g_stock, real)
        loss, _, _ = ganloop.generator_adversarial_loss(d, real, out["pose_ba"])
        loss.backward()
        torch.nn.utils.clip_grad_norm_(g_stock.parameters(), max_norm=1.0)
        opt_stock.step()
        return loss.detach()
    torch.manual_seed(5)
    loss_ours = float(step_ours())
    torch.manual_seed(5)
    info = dict(name="generator_step: generate, adversarial loss on HipPos3dDiscriminator, backward, clip, Adam", B=B,
                loss=loss_ours, loss_torch=float(step_stock()))
    with LibraryKernels() as lk:
        with OpCounter() as c:
            step_ours()
        torch.cuda.synchronize()
    info["launches"] = {"library_kernels": lk.n, "library_calls": lk.calls, "torch_ops_on_the_calling_thread": c.n}
    with LibraryKernels() as lk:
        with OpCounter() as c:
            step_stock()
        torch.cuda.synchronize()
    info["launches_torch"] = {"library_kernels": lk.n, "torch_ops_on_the_calling_thread": c.n}
    info["device_route"], info["torch_route"] = alternating_windows([step_ours, step_stock], a.window, a.rounds, a.warmup)
    info["torch_over_device"] = info["torch_route"]["ms_per_call"] / info["device_route"]["ms_per_call"]
    cases.append(info)

    out = {"cases": cases, "window_s": a.window, "rounds": a.rounds, "warmup": a.warmup, "device": torch.cuda.get_device_name(0)}
    line = json.dumps(out)
    print(line, flush=True)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
