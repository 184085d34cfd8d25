#!/usr/bin/env python3
"""Time of the adversarial game of one GAN batch (run_gan.py:1956-2135) on the device route (posegen_amd.discriminators / ganloop:
pg_disc_forward / pg_disc_backward / pg_disc_loss / pg_pool_exchange behind torch.autograd.Functions) beside the SAME modules -- the
same nn.Linears -- run as stock float32 torch ops on the same device, with the reference's host-side pool and accuracy.

  case 1, the generator step's adversarial part: B = 1024 generated poses, 0.5 mse(D(fake), 1), backward into the poses
          (requires_grad off on the discriminator, as set_grad([model_d3d], False));
  case 2, the same with the real pass and both accuracies (get_adv_loss as the reference runs it);
  case 3, train_dis: zero_grad, 1024 generated poses through the pool, D on 2 x 1024 rows, loss, accuracies, backward, clip, Adam.
Seeded inputs.  The two routes alternate within the run: `--rounds` windows each, HIP events around warmed batches of calls.
Launches: the library's kernels are counted from the calls that are made (pg_disc_forward 5; pg_disc_backward 5 data + 1 input
kernels where d_x is wanted, else 4, and 5 weight kernels where gradients are; loss and pool 1 each); what torch launches besides
is counted as tools/bench_pose_losses.py counts it: the non-view ATen operators of the forward pass as they are dispatched, and the
nodes of the autograd graph behind the loss.  The optimiser and the clipping are the same torch code on both routes and are not
counted.  No ratio is a condition; the tool reports.  Prints one JSON line; --out writes it to a file.

usage: bench_discriminators.py [--window 0.4] [--rounds 3] [--warmup 3] [--out profiles/pose_discriminators.json]"""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch
import torch.nn.functional as F

from tools.bench_pose_losses import OpCounter, count_launch_sites

B = 1024


def stock_forward(disc, x):
    """the module's Linears as the reference calls them: gather, Linear, LeakyReLU, cat"""
    spec, outs = disc.spec, []
    x = x.reshape(-1, spec.n_points, spec.point_dim)
    for p, (_, sel, _, _) in enumerate(spec.paths):
        h = x[:, sel].reshape(x.shape[0], -1)
        lins = disc.path_linears(p)
        for lin in lins[:4]:
            h = F.leaky_relu(lin(h), spec.slope)
        outs.append(lins[4](h))
    return torch.cat(outs, 1)


class HostPool:
    """Sample_from_Pool as the reference runs it: the batch on the host, one Python step per item"""

    def __init__(self, capacity):
        self.capacity, self.items = capacity, []

    def __call__(self, batch, rng):
        out = []
        for item in batch:
            if len(self.items) < self.capacity:
                self.items.append(item)
                out.append(item)
            elif rng.random_sample() > 0.5:
                i = rng.randint(0, self.capacity)
                out.append(self.items[i].copy())
                self.items[i] = item
            else:
                out.append(item)
        return out


def host_accuracy(pred, label):
    """get_discriminator_accuracy: both arrays to the host"""
    p, l = pred.detach().reshape(-1).cpu().numpy(), label.reshape(-1).cpu().numpy()
    return float(np.sum(np.where(np.abs(p - l) > 0.5, 0, 1)) / l.shape[0])


def stock_adv(disc, real, fake, accuracies):
    pred_fake = stock_forward(disc, fake)
    loss = 0.5 * F.mse_loss(pred_fake, torch.ones_like(pred_fake))
    if accuracies:
        pred_real = stock_forward(disc, real)
        host_accuracy(pred_real, torch.ones_like(pred_real))
        host_accuracy(pred_fake, torch.zeros_like(pred_fake))
    return loss


def stock_dis_step(disc, opt, real, fake, pool, rng):
    opt.zero_grad()
    fake = torch.Tensor(np.asarray(pool(np.asarray(fake.detach().cpu()), rng))).to(real.device)
    pr, pf = stock_forward(disc, real.detach()), stock_forward(disc, fake)
    loss = 0.5 * (F.mse_loss(pr, torch.ones_like(pr)) + F.mse_loss(pf, torch.zeros_like(pf)))
    accs = host_accuracy(pr, torch.ones_like(pr)), host_accuracy(pf, torch.zeros_like(pf))
    loss.backward()
    torch.nn.utils.clip_grad_norm_(disc.parameters(), max_norm=1)
    opt.step()
    return accs


class LibraryKernels:
    """the kernels behind the _ffi.call sites made while active"""

    def __init__(self):
        self.n, self.calls = 0, {}

    def __enter__(self):
        from posegen_amd import _ffi
        self._ffi, self._real = _ffi, _ffi.call

        def spy(r, name, *args):
            k = {"pg_disc_forward": 5, "pg_disc_loss": 1, "pg_pool_exchange": 1}.get(name)
            if name == "pg_disc_backward":
                k = (6 if args[-2] is not None else 4) + (5 if args[-1] is not None else 0)
            self.n += k or 0
            self.calls[name] = self.calls.get(name, 0) + 1
            return self._real(r, name, *args)
        _ffi.call = spy
        return self

    def __exit__(self, *exc):
        self._ffi.call = self._real


def alternating_windows(fns, window_s, rounds, warmup):
    """ms per call of each fn: warmed, then `rounds` windows each in turn (route 0, route 1, route 0, ...)"""
    for fn in fns:
        for _ in range(warmup):
            fn()
    torch.cuda.synchronize()
    tot = [[0, 0.0] for _ in fns]
    for _ in range(rounds):
        for i, fn in enumerate(fns):
            ms, batch = 0.0, 2
            while ms < window_s * 1e3 / rounds:
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                for _ in range(batch):
                    fn()
                e1.record()
                torch.cuda.synchronize()
                dt = e0.elapsed_time(e1)
                ms += dt
                tot[i][0] += batch
                tot[i][1] += dt
                batch = min(batch * 2, 256)
    return [{"ms_per_call": t / n, "calls": n, "window_ms": t} for n, t in tot]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--window", type=float, default=0.4)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("bench_discriminators: no HIP device (there is nothing to measure on a CPU)")
    from posegen_amd import discriminators as disc, ganloop
    dev = torch.device("cuda:0")
    torch.manual_seed(0)
    g = torch.Generator(device=dev).manual_seed(1)
    real = 0.6 * torch.randn((B, 24, 3), device=dev, generator=g)
    fake = (0.6 * torch.randn((B, 24, 3), device=dev, generator=g)).requires_grad_(True)

    def model():
        m = disc.HipPos3dDiscriminator().to(dev)
        torch.manual_seed(0)
        m.apply(lambda mod: torch.nn.init.kaiming_normal_(mod.weight) if isinstance(mod, torch.nn.Linear) else None)
        return m
    d_dev, d_stock = model(), model()
    cases = []

    # cases 1 and 2: the generator step (requires_grad off on the discriminator)
    for m in (d_dev, d_stock):
        for t in m.parameters():
            t.requires_grad_(False)
    for name, acc in (("generator step: 0.5 mse(D(fake), 1) -> d_fake", False), ("the same with the real pass and both accuracies", True)):
        ours = lambda: ganloop.generator_adversarial_loss(d_dev, real, fake, accuracies=acc)[0]
        stock = lambda: stock_adv(d_stock, real, fake, acc)

        def step(forward):
            fake.grad = None
            out = forward()
            out.backward()
            return out
        v_ours, g_ours = float(step(ours).detach()), fake.grad.detach().clone()
        v_stock, g_stock = float(step(stock).detach()), fake.grad.detach().clone()
        info = dict(name=name, B=B, value=v_ours, value_torch=v_stock, grad_max_abs=float(g_ours.abs().max()),
                    grad_max_abs_difference=float((g_ours - g_stock).abs().max()))
        ops, nodes = count_launch_sites(ours)
        with LibraryKernels() as lk:
            step(ours)
            torch.cuda.synchronize()
        info["launches"] = {"library_kernels": lk.n, "library_calls": lk.calls, "forward_torch_ops": ops, "backward_graph_nodes": nodes}
        ops, nodes = count_launch_sites(stock)
        info["launches_torch"] = {"forward_torch_ops": ops, "backward_graph_nodes": nodes}
        info["device_route"], info["torch_route"] = alternating_windows([lambda: step(ours), lambda: step(stock)], a.window, a.rounds, a.warmup)
        info["torch_over_device"] = info["torch_route"]["ms_per_call"] / info["device_route"]["ms_per_call"]
        cases.append(info)

    # case 3: train_dis
    for m in (d_dev, d_stock):
        for t in m.parameters():
            t.requires_grad_(True)
    opt_dev, opt_stock = torch.optim.Adam(d_dev.parameters(), lr=1e-4), torch.optim.Adam(d_stock.parameters(), lr=1e-4)
    pool_dev, pool_stock = disc.FakePool(4096), HostPool(4096)
    rng_dev, rng_stock = np.random.RandomState(7), np.random.RandomState(7)
    ours = lambda: ganloop.discriminator_step(d_dev, opt_dev, real, fake, pool_dev, rng_dev)
    stock = lambda: stock_dis_step(d_stock, opt_stock, real, fake, pool_stock, rng_stock)
    for _ in range(5):                                        # both pools full: the steady state of the loop
        ours()
        stock()
    torch.cuda.synchronize()
    info = dict(name="train_dis: pool, D on 2 x 1024 rows, loss, accuracies, backward, clip, Adam", B=2 * B)
    with LibraryKernels() as lk:
        with OpCounter() as c:
            accs = ours()
        torch.cuda.synchronize()
    info["launches"] = {"library_kernels": lk.n, "library_calls": lk.calls, "torch_ops_on_the_calling_thread": c.n}
    with OpCounter() as c:
        accs_stock = stock()
    torch.cuda.synchronize()
    info["launches_torch"] = {"torch_ops_on_the_calling_thread": c.n}
    info["accuracies"], info["accuracies_torch"] = [float(accs[0]), float(accs[1])], list(accs_stock)
    info["device_route"], info["torch_route"] = alternating_windows([ours, stock], a.window, a.rounds, a.warmup)
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
