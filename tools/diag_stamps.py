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
WORDS = 24                                              # 64-bit words of one wave's record of a pass
# The A pipe's restart behind a chunk entry: barrier release -> retire of the entry's first A fragment (Stream::restart_stamp),
# summed per wave and pass; record words (cycles, entries) of every next_a entry of the pass, of layers 1-4 and of layers 6-7
RESTARTS = (("every segment", 16, 17), ("L1-4", 18, 19), ("L6-7", 20, 21))
# stamp order in a pass: 0 | prologue | 1 | layer 0 (x) | 11 | Y limb chunks (on-chip form) | 2 | layers 1-4 | 3 | layer 5 | 4 | ..
ORDER = [0, 1, 11, 2, 3, 4, 5, 6, 7, 8]
# (stamp 6 sits behind the eight view tiles since the empty-wave skip: the row in front of it is the alpha tile AND the view tiles'
# trunk part, 9 x 8 units; the row behind it the view layer's second stage, y_apply16, with its pack)
NAMES = ["pass prologue", "L0 (x) + pack", "Y limb chunks", "L1-4", "L5 (h+x) + pack", "L6-7", "alpha + view tiles", "view 2nd stage (Y)", "rgb+store"]
MFMA = [0, 448, 0, 1024, 704, 512, 144, 16, 8]          # per wave, 16x16x32, every limb in range (Y: 4 per limb chunk)
# inside the two x phases (x_segment16): record words 12 / 13 = in front of layer 0's direction units / behind their last MFMA,
# 14 / 15 = the same in the skip layer; a phase starts at stamp 1 / 3 and ends, behind its ReLU + pack, at stamp 11 / 4
X_PHASES = (("layer 0", 1, 12, 13, 11, "bias + limb units"), ("skip layer", 3, 14, 15, 4, "hidden part + limb units"))
DIR_MFMA = 96                                           # three direction units x 16 out tiles x 2 column tiles


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
    restart_rows(full, tot.mean())
    # the Y segment by passes with and without a limb in range (no limb: the segment is two stamps apart)
    y = d[:, :, 2].max(1)
    has = y > 300
    if has.any():
        print(f"Y limb chunks: {100 * has.mean():.1f}% of the passes have a limb in range; there {d[has][:, :, 2].mean():.0f} cycles per pass "
              f"(slowest wave {y[has].mean():.0f}), elsewhere {d[~has][:, :, 2].mean() if (~has).any() else 0:.0f}")
    x_rows(full, has if has.any() else None)


def restart_rows(full, tot):
    if not (full[:, :, 17] != 0).all():
        print("chunk-entry restart: this build has no restart stamps")
        return
    for name, wt, wn in RESTARTS:
        t, n = full[:, :, wt].astype(np.float64), full[:, :, wn].astype(np.float64)
        print(f"chunk-entry restart, {name:13s} {t.mean():7.0f} cycles {100 * t.mean() / tot:5.2f}%   {n.mean():5.1f} entries, {t.sum() / n.sum():6.1f} cycles each   "
              f"waves 0-3 {t[:, :4].mean():7.0f}  waves 4-7 {t[:, 4:].mean():7.0f}   by wave {t.mean(0).astype(int).tolist()}")


def x_rows(full, has):
    """The two x phases by stretch: what is in front of the direction units, the direction units (96 MFMAs per wave), the ReLU +
    pack behind them -- for passes with and without a limb in range (the record form has no Y segment to tell them by: there a
    pass counts as 'with' when layer 0's limb stretch of its slowest wave is past a chunk entry)."""
    if not (full[:, :, 12:16] != 0).all():
        print("x phases: this build has no stamps inside x_segment16")
        return
    f = full.astype(np.float64)
    if has is None:
        has = (f[:, :, 12] - f[:, :, 1]).max(1) > 600
    for label, sel in (("no limb in range", ~has), ("a limb in range", has)):
        if not sel.any():
            continue
        g = f[sel]
        print(f"x phases, passes with {label} ({100 * sel.mean():.1f}% of the passes):")
        for name, s0, sd, sm, s1, front in X_PHASES:
            a, b, c = (g[:, :, sd] - g[:, :, s0]).mean(), (g[:, :, sm] - g[:, :, sd]).mean(), (g[:, :, s1] - g[:, :, sm]).mean()
            print(f"   {name:10s} {front:24s} {a:7.0f}   direction units {b:6.0f} ({b / DIR_MFMA:5.1f} cyc/mfma)   ReLU + pack {c:6.0f}   "
                  f"phase {a + b + c:7.0f}")
        pro = (g[:, :, 1] - g[:, :, 0]).mean()
        print(f"   pass prologue {pro:6.0f}   pass total {(g[:, :, 8] - g[:, :, 0]).mean():7.0f}")


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
            dbg = torch.zeros(SLOTS * 8 * WORDS, device=dev, dtype=torch.int64)
            r.stage_eval(which, rb, z, skts, dbg_stage=99, dbg=dbg)
        torch.cuda.synchronize()
        table(dbg.cpu().numpy().reshape(SLOTS, 8, WORDS), f"{a.form} form, {a.prec}, {label} launch (S = {z.shape[1]})")
    r.close()


if __name__ == "__main__":
    main()
