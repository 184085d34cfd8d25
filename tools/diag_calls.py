"""A few render_rays calls of different sizes, each timed on its own (the default), or, with --small, many short calls:
CALLS pg_render_rays calls of ROWS rays each (two nets at 64 + 16, the single-net model at 96 + 48; bf16), REPS times.  Per
repetition one JSON line: `host_us_per_call` -- the host time of the enqueueing loop, nothing waited for: what a call costs
the caller's thread -- and `ms_per_call` with the device synchronised at the end.

Usage:  python tools/diag_calls.py [--small [--rows 2048] [--calls 4000] [--reps 4]]
"""
import argparse, sys, os, time, json
sys.path.insert(0, os.getcwd())
import torch
from posegen_amd import h36m_config, surreal_config, synthetic as syn
from posegen_amd.raycaster import HipRayCaster
from bench import full_frame_rays
dev = torch.device("cuda:0")


def small_calls(rows, calls, reps):
    from posegen_amd.config import surreal_single_config
    for name, cfg in (("two_net", surreal_config()), ("single_net", surreal_single_config())):
        wc, wf, tv, td = syn.make_model(cfg, 0)
        c = HipRayCaster.from_weights(cfg, wc, None if cfg.single_net else wf, tv, td, device=dev, precision="bf16")
        rb, skts, cyl, *_ = full_frame_rays(256, 256, dev, cfg)
        rb = rb[:rows].contiguous()
        r = c.renderer
        r.set_chunk(cfg.chunk)
        kw = dict(n_samples=cfg.n_samples, n_importance=cfg.n_importance, want_alpha=False)
        for _ in range(20):
            r.render_rays(rb, skts, cyl, **kw)
        for rep in range(reps):
            torch.cuda.synchronize(); t0 = time.perf_counter()
            for _ in range(calls):
                r.render_rays(rb, skts, cyl, **kw)
            t1 = time.perf_counter(); torch.cuda.synchronize(); t2 = time.perf_counter()
            print(json.dumps({"bench": "tools/diag_calls.py --small", "model": name, "rows": rows, "calls": calls, "rep": rep,
                              "host_us_per_call": (t1 - t0) / calls * 1e6, "ms_per_call": (t2 - t0) / calls * 1e3}), flush=True)
        r.close()


ap = argparse.ArgumentParser()
ap.add_argument("--small", action="store_true")
ap.add_argument("--rows", type=int, default=2048)
ap.add_argument("--calls", type=int, default=4000)
ap.add_argument("--reps", type=int, default=4)
a = ap.parse_args()
if a.small:
    small_calls(a.rows, a.calls, a.reps)
    sys.exit(0)
for name, cfgf in (("h36m", h36m_config), ("surreal", surreal_config)):
    cfg = cfgf()
    c = HipRayCaster.from_weights(cfg, *syn.make_model(cfg, 0), device=dev, precision="bf16")
    rb, skts, cyl, *_ = full_frame_rays(512, 512, dev)
    n = rb.shape[0]
    cams = (torch.arange(n, device=dev) % max(cfg.n_framecodes, 1)).float() if cfg.framecode_ch else None
    r = c.renderer
    r.set_chunk(cfg.chunk)
    for rows in (32768, n, n, n, 200000, n):
        torch.cuda.synchronize(); t0 = time.perf_counter()
        r.render_rays(rb[:rows], skts, cyl, cams=None if cams is None else cams[:rows], want_alpha=False)
        torch.cuda.synchronize(); print(name, rows, "%.1f ms" % ((time.perf_counter() - t0) * 1e3), flush=True)
    r.close()
