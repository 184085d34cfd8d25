"""Where a pass of the 16x16x32 kernel spends its cycles: the s_memtime stamps of a -DPG_STAMPS build of pg_eval16r.hip
(FILE=pg_eval16r.hip tools/build_variant.sh stamps -DPG_STAMPS; POSEGEN_HIP_LIB=build_ab/lib_stamps.so) on the coarse
(S = 64) and the fine (S = 80) launch of bench.py's 512 x 512 frame.  The kernel keeps the stamps of 1024 passes spread evenly
over the launch (pg_stage_eval, dbg_stage 99).

    python tools/diag_stamps.py [--form onchip|records] [--prec bf16] [--res 512]"""
import argparse
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch

from bench import full_frame_rays
from posegen_amd import surreal_config, synthetic as syn
from posegen_amd.raycaster import HipRayCaster

SLOTS = 1024
# stamp order in a pass: 0 | prologue | 1 | layer 0 (x) | 11 | Y limb chunks (on-chip form) | 2 | layers 1-4 | 3 | layer 5 | 4 | ..
ORDER = [0, 1, 11, 2, 3, 4, 5, 6, 7, 8]
NAMES = ["pass prologue", "L0 (x) + pack", "Y limb chunks", "L1-4", "L5 (h+x) + pack", "L6-7", "alpha tile", "view (trunk+Y)", "rgb+store"]
MFMA = [0, 448, 0, 1024, 704, 512, 16, 144, 8]          # per wave, 16x16x32, every limb in range (Y: 4 per limb chunk)


def table(full, label):
    used = full[:, :, 8] != 0
    full = full[used.all(1)]
    st = full[:, :, ORDER].astype(np.float64)
    d = np.diff(st, axis=-1)                                # [pass, wave, segment]
    tot = st[:, :, -1] - st[:, :, 0]
    print(f"== {label}: {full.shape[0]} passes x 8 waves; pass total {tot.mean():.0f} cycles (min {tot.min():.0f}, max {tot.max():.0f})")
    print("   cycles per pass per wave waiting in vmcnt (weight DMA) %.0f, in s_barrier %.0f; by wave: vmcnt %s barrier %s" % (
        full[:, :, 9].mean(), full[:, :, 10].mean(), full[:, :, 9].mean(0).astype(int).tolist(), full[:, :, 10].mean(0).astype(int).tolist()))
    for k, name in enumerate(NAMES):
        m = d[:, :, k].mean()
        lo, hi = d[:, :4, k].mean(), d[:, 4:, k].mean()
        per = f"{m / MFMA[k]:6.1f} cyc/mfma" if MFMA[k] else ""
        print(f"{name:18s} {m:9.0f} cycles {100 * m / tot.mean():5.1f}%   waves 0-3 {lo:8.0f}  waves 4-7 {hi:8.0f}  {per}")
    # the Y segment by passes with and without a limb in range (no limb: the segment is two stamps apart)
    y = d[:, :, 2].max(1)
    has = y > 300
    if has.any():
        print(f"Y limb chunks: {100 * has.mean():.1f}% of the passes have a limb in range; there {d[has][:, :, 2].mean():.0f} cycles per pass "
              f"(slowest wave {y[has].mean():.0f}), elsewhere {d[~has][:, :, 2].mean() if (~has).any() else 0:.0f}")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--form", default="onchip", choices=("onchip", "records"))
    ap.add_argument("--prec", default="bf16")
    ap.add_argument("--res", type=int, default=512)
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    cfg = surreal_config()
    r = HipRayCaster.from_weights(cfg, *syn.make_model(cfg, 0), device=dev, precision=a.prec).renderer
    r.set_onchip("always" if a.form == "onchip" else "records")
    rb, skts, cyl, *_ = full_frame_rays(a.res, a.res, dev)
    ex = r.render_rays(rb, skts, cyl, n_samples=cfg.n_samples, n_importance=cfg.n_importance, want_alpha=False, extras=True)["extras"]
    for which, z, label in ((0, ex["z_coarse"], "coarse"), (1, ex["z_fine"], "fine")):
        for rep in range(2):
            dbg = torch.zeros(SLOTS * 8 * 16, device=dev, dtype=torch.int64)
            r.stage_eval(which, rb, z, skts, dbg_stage=99, dbg=dbg)
        torch.cuda.synchronize()
        table(dbg.cpu().numpy().reshape(SLOTS, 8, 16), f"{a.form} form, {a.prec}, {label} launch (S = {z.shape[1]})")
    r.close()


if __name__ == "__main__":
    main()
