"""Child process of tests/test_gpu_pass_walk.py: POSEGEN_PASS_WALK (and POSEGEN_MAX_WG) are read once per process, so every
(case, walk) pair renders in a process of its own and reports a digest of every output array -- raw, rgb_map, disp_map,
acc_map -- of every call of the case, plus what the kernel's own pass counter says, as one JSON line.

    pass_walk_cases.py CASE

CASE = <config>:<precision>:<pose>:<n_rays>:<S>[,<S>...]    config: surreal | h36m (frame codes); pose: one | per_ray
Rays: the synthetic camera's frame through the body (bench.full_frame_rays), so that passes differ in their limbs in range."""
import hashlib
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
import numpy as np
import torch

from bench import full_frame_rays
from posegen_amd import h36m_config, surreal_config, synthetic as syn
from posegen_amd.raycaster import HipRayCaster


def digest(t):
    a = np.ascontiguousarray(t.detach().cpu().numpy())
    return hashlib.sha256(a.tobytes()).hexdigest()


def main():
    conf, prec, pose, n, samples = sys.argv[1].split(":")
    n = int(n)
    dev = torch.device("cuda:0")
    cfg = h36m_config() if conf == "h36m" else surreal_config()
    c = HipRayCaster.from_weights(cfg, *syn.make_model(cfg, 0), device=dev, precision=prec)
    r = c.renderer
    side = 64
    while side * side < n:
        side *= 2
    rb, skts, cyl, *_ = full_frame_rays(side, side, dev)
    first = (side * side - n) // 2          # the middle rows: through the body
    rb = rb[first:first + n].contiguous()
    cams = (torch.arange(n, device=dev) % cfg.n_framecodes).float() if conf == "h36m" else None
    if pose == "per_ray":                   # a pose per ray: the frame's pose, moved a little from ray to ray
        skts = skts.reshape(1, 24, 4, 4).repeat(n, 1, 1, 1)
        skts[:, :, :3, 3] += 1e-3 * torch.sin(torch.arange(n, device=dev, dtype=torch.float32))[:, None, None]
    out = {}
    for S in (int(s) for s in samples.split(",")):
        res = r.render_rays(rb, skts, cyl, cams=cams, n_samples=S, n_importance=0, want_alpha=False, extras=True)
        torch.cuda.synchronize()
        d = {k: digest(res[k]) for k in ("rgb_map", "disp_map", "acc_map")}
        d["raw"] = digest(res["extras"]["raw_coarse"])
        d["finite"] = bool(torch.isfinite(res["rgb_map"]).all())
        d["acc_max"] = float(res["acc_map"].max())
        default_form = "POSEGEN_ONCHIP" not in os.environ     # (the forms that count)
        if default_form and conf == "surreal" and pose == "one" and n <= (1 << 19) and (prec == "fp16c" or S <= 112):
            # the kernel's own count of the passes it ran: the CNT instantiation of the on-chip 16x16x32 kernel (256 points per
            # pass; up to 112 samples per ray), pg_evalc2.hip's counters (128 points per pass)
            st = r.limb_skip_stats(0, rb, res["extras"]["z_coarse"], skts)
            pts = 128 if prec == "fp16c" else 256
            d["passes_counted"] = st["passes"]
            d["passes"] = (n * S + pts - 1) // pts
        out[str(S)] = d
    r.close()
    print("PASS_WALK " + json.dumps(out))


if __name__ == "__main__":
    main()
