"""The calls of tests/test_gpu_y_segment.py: every case rendered in the on-chip form of the 16x16x32 kernel and in its record
form, and what differs between the two.  Imported by the test for the default grid; run as a child process for
POSEGEN_MAX_WG=1 (read once per process): one workgroup then walks every pass of a launch, so that each pass finds in the Y
image the limbs every earlier pass left there.

    y_segment_cases.py          prints one JSON line: Y_SEGMENT {case id: figures}

Rays: the 32 x 32 all-hit frame of the synthetic camera (bench.full_frame_rays) at pose spreads 0.2 and 0.6, whole (1024
rays) and, of the first, 1, 3 and 37 consecutive rays through the body."""
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
import torch

from bench import full_frame_rays
from posegen_amd import h36m_config, surreal_config, synthetic as syn

SIDE = 32
FIRST = 20 * SIDE + 14              # a ray through the body that is in range of some limbs only
RAY_SETS = {"1": (0.2, FIRST, 1), "3": (0.2, FIRST, 3), "37": (0.2, FIRST - 5, 37), "1024": (0.2, 0, SIDE * SIDE), "1024w": (0.6, 0, SIDE * SIDE)}
SAMPLES = ((64, 16), (96, 16))
PRECS = ("bf16", "fp16")
POSES = ("one", "per_ray", "codes")
MAPS = ("rgb_map", "acc_map", "disp_map")
CASE_IDS = [f"{prec}-{pose}-{rays}-{S}+{N}" for prec in PRECS for pose in POSES for rays in RAY_SETS for S, N in SAMPLES]


def rays_of(name, device):
    """(ray_batch, skts [24, 4, 4], cyl) of a ray set"""
    spread, first, n = RAY_SETS[name]
    rb, skts, cyl, *_ = full_frame_rays(SIDE, SIDE, device, sigma=spread)
    return rb[first:first + n].contiguous(), skts.reshape(24, 4, 4), cyl


def second_pose(device):
    return torch.tensor(syn.make_pose(2, 5)[2][1], device=device).reshape(24, 4, 4)


def per_ray_poses(skts, n, device):
    """a pose per ray: the frame's pose and a second one, alternating in blocks of five rays"""
    other = (torch.arange(n, device=device) // 5) % 2 == 1
    return torch.where(other[:, None, None, None], second_pose(device).expand(n, -1, -1, -1), skts.expand(n, -1, -1, -1)).contiguous()


def run_cases(device="cuda:0"):
    from posegen_amd.raycaster import HipRayCaster
    out = {}
    for pose_kinds, cfg in ((("one", "per_ray"), surreal_config()), (("codes",), h36m_config(n_samples=64))):
        r = HipRayCaster.from_weights(cfg, *syn.make_model(cfg, 0), device=device, precision="bf16").renderer
        try:
            for rays in RAY_SETS:
                rb, skts, cyl = rays_of(rays, device)
                n = rb.shape[0]
                for pose in pose_kinds:
                    sk = per_ray_poses(skts, n, device) if pose == "per_ray" else skts
                    cams = None
                    if pose == "codes":
                        cams = ((torch.arange(n, device=device) * 7) % cfg.n_framecodes).float()
                        cams[3::11] = -1.0          # (some rays on the mean code)
                    for prec in PRECS:
                        r.set_precision(prec)
                        for S, N in SAMPLES:
                            res = {}
                            for form in ("always", "records"):
                                r.set_onchip(form)
                                res[form] = r.render_rays(rb, sk, cyl, cams=cams, n_samples=S, n_importance=N, want_alpha=False)
                            torch.cuda.synchronize()
                            a, b = res["always"], res["records"]
                            d = {k: float((a[k] - b[k]).abs().nan_to_num(nan=float("inf")).max()) for k in MAPS}
                            d.update({f"{k}_equal": bool(torch.equal(a[k].view(torch.int32), b[k].view(torch.int32))) for k in MAPS})      # bit for bit
                            d["finite"] = all(bool(torch.isfinite(a[k]).all()) for k in ("rgb_map", "acc_map"))
                            d["acc_max"] = float(a["acc_map"].max())
                            out[f"{prec}-{pose}-{rays}-{S}+{N}"] = d
        finally:
            r.close()
    return out


if __name__ == "__main__":
    print("Y_SEGMENT " + json.dumps(run_cases()))
