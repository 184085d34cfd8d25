#!/usr/bin/env python3
"""Time of the HMR regression head (run_gan.py:1343-1356 and rot6d_to_rotmat) on the device route (posegen_amd.regressors:
pg_hmr_head_forward / pg_hmr_head_backward behind one torch.autograd.Function) beside the SAME nn.Linear children run as stock float32
torch operators on the same device with the same dropout masks (regressors.stock_forward).

  case 1, the head forward in eval mode at B = 20 (the loop's render batch), under no_grad;
  case 2, the same at B = 128;
  case 3, the head forward + backward in training mode at B = 128 (masks made once, outside the timed calls, on both routes);
  case 4, `ganloop.regressor_step` at B = 128 with a stand-in trunk (one strided convolution and a global average pool to 2048
          features; the ResNet is torch's on both routes and is not what this measures), and the same lines around stock_forward.
The two routes alternate within one process: after `--warmup` calls each, `--blocks` timed blocks of `--calls` calls a route, block by
block in turn, device events around a block that ends in a synchronise; the figure is the median block.  Launches: the library's kernels are counted from the calls that are
made (pg_hmr_head_forward: the state, the feature product, three products a round, the rotation epilogue; pg_hmr_head_backward: the
rotation backward, three products a round -- two in round 0 without d_init --, one grouped); what torch launches besides is counted
as tools/bench_pose_losses.py counts it.  No ratio is a condition; the tool reports.  Prints one JSON line; --out writes it to a file.

usage: bench_hmr_head.py [--blocks 15] [--calls 10] [--warmup 5] [--out profiles/hmr_head.json]"""
import argparse
import json
import math
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch

from tools.bench_pose_losses import OpCounter


def interleaved_medians(fns, blocks, calls, warmup):
    """ms per call of each fn: warmed, then `blocks` timed blocks of `calls` calls each, the routes taking turns block by block (route
    0, route 1, route 0, ...), device events around a block; the median block of each route, with its fastest and slowest"""
    for fn in fns:
        for _ in range(warmup):
            fn()
    torch.cuda.synchronize()
    times = [[] for _ in fns]
    for _ in range(blocks):
        for i, fn in enumerate(fns):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(calls):
                fn()
            e1.record()
            torch.cuda.synchronize()
            times[i].append(e0.elapsed_time(e1) / calls)
    return [{"ms_per_call": float(sorted(t)[len(t) // 2]), "min_ms": float(min(t)), "max_ms": float(max(t)), "blocks": blocks, "calls_per_block": calls}
            for t in times]


class LibraryKernels:
    """the kernels behind the _ffi.call sites made while active"""

    def __init__(self):
        self.n, self.calls = 0, {}

    def __enter__(self):
        from posegen_amd import _ffi
        self._ffi, self._real = _ffi, _ffi.call

        def spy(r, name, *args):
            k = 1
            if name == "pg_hmr_head_forward":
                k = 2 + 3 * args[0]._obj.n_iter + 1
            if name == "pg_hmr_head_backward":
                k = 1 + 3 * args[0]._obj.n_iter - (args[-1] is None) + (args[-3] is not None or args[-2] is not None)
            self.n += int(k)
            self.calls[name] = self.calls.get(name, 0) + 1
            return self._real(r, name, *args)
        _ffi.call = spy
        return self

    def __exit__(self, *exc):
        self._ffi.call = self._real


class StandInTrunk(torch.nn.Module):
    def __init__(self, n_feat=2048):
        super().__init__()
        self.conv = torch.nn.Conv2d(3, n_feat, 7, stride=8)
        self.pool = torch.nn.AdaptiveAvgPool2d(1)

    def forward(self, x):
        return self.pool(torch.relu(self.conv(x))).flatten(1)


def measure(name, B, ours, stock, a, extra=None):
    info = dict(name=name, B=B)
    info.update(extra or {})
    with LibraryKernels() as lk:
        with OpCounter() as c:
            ours()
        torch.cuda.synchronize()
    info["launches"] = {"library_kernels": lk.n, "library_calls": lk.calls, "torch_ops_on_the_calling_thread": c.n}
    with LibraryKernels() as lk:
        with OpCounter() as c:
            stock()
        torch.cuda.synchronize()
    info["launches_torch"] = {"library_kernels": lk.n, "torch_ops_on_the_calling_thread": c.n}
    info["device_route"], info["torch_route"] = interleaved_medians([ours, stock], a.blocks, a.calls, a.warmup)
    info["torch_over_device"] = info["torch_route"]["ms_per_call"] / info["device_route"]["ms_per_call"]
    return info


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--blocks", type=int, default=15)
    ap.add_argument("--calls", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("bench_hmr_head: no HIP device (there is nothing to measure on a CPU)")
    from posegen_amd import ganloop, pose_eval, regressors as reg
    dev = torch.device("cuda:0")
    renderer = pose_eval.default_scorer(dev).renderer
    g = torch.Generator(device=dev).manual_seed(1)

    def head():
        torch.manual_seed(0)
        h = reg.HipHMRHead(renderer=renderer)
        with torch.no_grad():
            h.init_pose.normal_()
        return h.to(dev)
    h_dev, h_stock = head(), head()
    cases = []
    for B in (20, 128):
        xf = torch.randn((B, 2048), device=dev, generator=g).relu()
        h_dev.eval(), h_stock.eval()

        def fwd_ours(xf=xf):
            with torch.no_grad():
                return h_dev(xf)

        def fwd_stock(xf=xf):
            with torch.no_grad():
                return reg.stock_forward(h_stock, xf)
        o, s = fwd_ours(), fwd_stock()
        cases.append(measure("head forward (eval mode, no_grad)", B, fwd_ours, fwd_stock, a,
                             {"max_abs_difference": [float((x - y).abs().max()) for x, y in zip(o, s)]}))

    B = 128
    xf = torch.randn((B, 2048), device=dev, generator=g).relu().requires_grad_(True)
    masks = reg.draw_masks(h_dev.spec, B, dev)
    cot = [torch.randn(s, device=dev, generator=g) for s in ((B, 24, 3, 3), (B, 10), (B, 3))]
    h_dev.train(), h_stock.train()

    def both(fn, h):
        def run():
            for p in h.parameters():
                p.grad = None
            xf.grad = None
            outs = fn(h)
            torch.autograd.backward(outs, cot)
            return outs
        return run
    fb_ours, fb_stock = both(lambda h: h(xf, masks=masks), h_dev), both(lambda h: reg.stock_forward(h, xf, masks=masks), h_stock)
    fb_ours()
    g_ours = h_dev.fc1.weight.grad.clone()
    fb_stock()
    cases.append(measure("head forward + backward (training mode, given masks)", B, fb_ours, fb_stock, a,
                         {"max_abs_difference_d_fc1_w": float((g_ours - h_stock.fc1.weight.grad).abs().max())}))

    class Stock(torch.nn.Module):
        def __init__(self, trunk, h):
            super().__init__()
            self.trunk, self.head = trunk, h

        def forward(self, x, masks=None):
            return reg.stock_forward(self.head, self.trunk(x), masks=masks)
    torch.manual_seed(2)
    t_dev = StandInTrunk().to(dev)
    t_stock = StandInTrunk().to(dev)
    t_stock.load_state_dict(t_dev.state_dict())
    m_dev, m_stock = reg.HipHMR(t_dev, h_dev), Stock(t_stock, h_stock)
    opt_dev, opt_stock = torch.optim.Adam(m_dev.parameters(), lr=1e-5), torch.optim.Adam(m_stock.parameters(), lr=1e-5)
    images = torch.randn((B, 3, 224, 224), device=dev, generator=g)
    gt = 0.3 * torch.randn((B, 24, 3), device=dev, generator=g)
    kw = dict(gt_is_axis_angle=True, cap=math.inf)

    def step_ours():
        return ganloop.regressor_step(m_dev, opt_dev, images, gt, renderer, masks=masks, **kw)

    def step_stock():
        return ganloop.regressor_step(m_stock, opt_stock, images, gt, renderer, masks=masks, **kw)
    cases.append(measure("regressor_step: stand-in trunk, head, regressor_loss, backward, Adam", B, step_ours, step_stock, a,
                         {"loss": float(step_ours()), "loss_torch": float(step_stock())}))

    out = {"cases": cases, "blocks": a.blocks, "calls_per_block": a.calls, "warmup": a.warmup, "device": torch.cuda.get_device_name(0)}
    line = json.dumps(out)
    print(line, flush=True)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
