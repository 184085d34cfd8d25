"""Mesh extraction at the reference's defaults (res = 255, radius = 1.80) with bench.py's synthetic model and pose.

Per precision: the ms of HipRenderer.grid_density (grid formed on the device, rows as rays) against the existing
HipRenderer.mesh_density (grid formed on the host, uploaded, explicit points) on the same box -- each the median of 5 after 2
warm-ups, alternating --, the ms of marching cubes (count + emit), the vertex and triangle counts, and the bytes either path moves
across PCIe.  Writes profiles/mesh_extract.json.

usage: python tools/bench_mesh.py [--res 255] [--radius 1.8] [--precisions bf16,fp16,fp16c,fp32] [--out profiles/mesh_extract.json]
"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from posegen_amd import surreal_config, synthetic as syn          # noqa: E402
from posegen_amd.raycaster import HipRayCaster                     # noqa: E402


def timed(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3, out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--res", type=int, default=255)
    ap.add_argument("--radius", type=float, default=1.8)
    ap.add_argument("--precisions", default="bf16,fp16,fp16c,fp32")
    ap.add_argument("--out", default=os.path.join("profiles", "mesh_extract.json"))
    a = ap.parse_args()
    cfg = surreal_config()
    caster = HipRayCaster.from_weights(cfg, *syn.make_model(cfg, 0), device="cuda:0", precision="bf16")
    r = caster.renderer
    _, kps, skts = syn.make_pose(1, 1)
    kps, skts = torch.tensor(kps), torch.tensor(skts)
    R = a.res + 1
    di = r.device_info()
    result = {"res": a.res, "radius": a.radius, "points": R ** 3, "device": torch.cuda.get_device_name(0), "n_cu": di["n_cu"],
              "clock_khz": di["clock_khz"], "warmup": 2, "runs": 5, "precisions": {}}
    for prec in a.precisions.split(","):
        r.set_precision(prec)
        new = lambda: r.grid_density(kps, skts, radius=a.radius, res=a.res)
        old = lambda: r.mesh_density(kps, skts, radius=a.radius, res=a.res).contiguous()
        t_new, t_old = [], []
        for i in range(7):                      # alternating; the first two rounds are warm-ups
            ms_n, grid = timed(new)
            ms_o, ref = timed(old)
            if i >= 2:
                t_new.append(ms_n)
                t_old.append(ms_o)
        diff = float((grid - ref).abs().max())
        pos = grid[grid > 0]
        thr = float(pos.median()) if pos.numel() else 0.0
        t_mc = []
        for i in range(7):
            ms, (v, t) = timed(lambda: r.marching_cubes(grid, thr, clamp=0.0))
            if i >= 2:
                t_mc.append(ms)
        ms10, (v10, t10) = timed(lambda: r.marching_cubes(grid, 10.0, clamp=0.0))
        result["precisions"][prec] = {
            "grid_density_ms": float(np.median(t_new)), "mesh_density_ms": float(np.median(t_old)),
            "grid_density_runs_ms": t_new, "mesh_density_runs_ms": t_old,
            "max_abs_diff_between_the_two": diff, "sigma_raw_max": float(grid.max()), "positive_points": int(pos.numel()),
            "threshold_median_of_positive": thr, "marching_cubes_ms": float(np.median(t_mc)), "vertices": int(v.shape[0]),
            "triangles": int(t.shape[0]), "threshold_10": {"vertices": int(v10.shape[0]), "triangles": int(t10.shape[0]), "ms": ms10},
            # host <-> device traffic of one pose: the new path sends root + pose and reads nothing back until the mesh is asked for
            "pcie_bytes_grid_density": 3 * 4 + 24 * 16 * 4 + R * 4,
            "pcie_bytes_mesh_density": R ** 3 * 12 + 24 * 16 * 4,
            "pcie_bytes_mesh_download": int(v.shape[0]) * 12 + int(t.shape[0]) * 12,
            "pcie_bytes_grid_download_the_host_marching_cubes_needed": R ** 3 * 4,
        }
        print(prec, json.dumps(result["precisions"][prec]), flush=True)
    os.makedirs(os.path.dirname(a.out) or ".", exist_ok=True)
    with open(a.out, "w") as fh:
        json.dump(result, fh, indent=1)
        fh.write("\n")
    r.close()


if __name__ == "__main__":
    main()
