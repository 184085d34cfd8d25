"""Share of empty waves on the benchmark frame (profiles/empty_wave_share.txt): (wave, pass) pairs of the fused 16x16x32
kernel whose valid points all have sigma <= 0, counted by the kernel itself (pg_stage_eval, dbg_stage 97) on the coarse and
on the fine launch of bench.py's 512 x 512 all-hit frame, and on the render call's own launches (pg_debug_wave_counts).

    python tools/diag_empty_waves.py [--prec bf16] [--res 512]
    python tools/diag_empty_waves.py --oracle     the same share from the fp32 oracle on the CPU, no GPU: groups of 32
                                                  consecutive samples of 32 blocks of 128 consecutive rays spread over the frame"""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch

from bench import full_frame_rays
from posegen_amd import surreal_config, synthetic as syn
from posegen_amd.raycaster import HipRayCaster


def oracle_share(res, blocks=32, per=128):
    from oracle import anerf_oracle as orc
    cfg = surreal_config()
    wc, wf, tv, td = syn.make_model(cfg, 0)
    tw = lambda w: {k: torch.tensor(v) for k, v in w.items()}
    *_, rb, skts, cyl = full_frame_rays(res, res, "cpu")
    n = rb.shape[0]
    tot = {"raw_coarse": [0, 0, 0, 0], "raw_fine": [0, 0, 0, 0]}
    for b in range(blocks):
        s = int(b * (n - per) / (blocks - 1)) // 2 * 2
        with torch.no_grad():
            ex = orc.render_rays(rb[s:s + per], skts, cyl, orc.OracleConfig(tau_v=tv, tau_d=td), tw(wc), tw(wf), cfg.n_samples,
                                 cfg.n_importance, return_extras=True)["extras"]
        for k, t in tot.items():
            sg = ex[k][..., 3].reshape(-1)
            g = sg[:sg.numel() // 32 * 32].reshape(-1, 32) <= 0
            t[0] += int(g.all(1).sum()); t[1] += g.shape[0]; t[2] += int((sg <= 0).sum()); t[3] += sg.numel()
    print("EMPTY_WAVES_ORACLE " + json.dumps({k: {"rays": blocks * per, "groups": t[1], "empty_groups_frac": t[0] / t[1],
                                                  "points_sigma_le_0": t[2] / t[3]} for k, t in tot.items()}))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--prec", default="bf16")
    ap.add_argument("--res", type=int, default=512)
    ap.add_argument("--oracle", action="store_true")
    a = ap.parse_args()
    if a.oracle:
        return oracle_share(a.res)
    dev = torch.device("cuda:0")
    cfg = surreal_config()
    r = HipRayCaster.from_weights(cfg, *syn.make_model(cfg, 0), device=dev, precision=a.prec).renderer
    rb, skts, cyl, *_ = full_frame_rays(a.res, a.res, dev)
    res = r.render_rays(rb, skts, cyl, n_samples=cfg.n_samples, n_importance=cfg.n_importance, want_alpha=False, extras=True)
    out = {"prec": a.prec, "res": a.res,
           "coarse": r.limb_skip_stats(0, rb, res["extras"]["z_coarse"], skts),
           "fine": r.limb_skip_stats(1, rb, res["extras"]["z_fine"], skts)}
    r.count_waves(True)
    r.render_rays(rb, skts, cyl, n_samples=cfg.n_samples, n_importance=cfg.n_importance, want_alpha=False)
    torch.cuda.synchronize()
    out["render_call_both_launches"] = r.read_wave_counts()
    r.count_waves(False)
    for k in ("raw_coarse", "raw_fine"):
        out[f"points_sigma_le_0_{k}"] = float((res["extras"][k][..., 3] <= 0).float().mean())
    r.close()
    print("EMPTY_WAVES " + json.dumps(out))


if __name__ == "__main__":
    main()
