"""Share of empty waves on the benchmark frame (profiles/empty_wave_share.txt): (wave, pass) pairs of the fused 16x16x32
kernel whose valid points all have sigma <= 0, counted by the kernel itself (pg_stage_eval, dbg_stage 97) on the coarse and
on the fine launch of bench.py's 512 x 512 all-hit frame, and on the render call's own launches (pg_debug_wave_counts).

    python tools/diag_empty_waves.py [--prec bf16] [--res 512]
    python tools/diag_empty_waves.py --oracle     the same share from the fp32 oracle on the CPU, no GPU: groups of 32
                                                  consecutive samples of 32 blocks of 128 consecutive rays spread over the frame;
                                                  and the pass-level figures (256 consecutive points = the 8 waves of a pass): the
                                                  share of passes whose eight waves are all empty, the histogram of live waves per
                                                  pass, and the limbs in range (by point: some point of the pass within the range
                                                  beyond which the cutoff weight is below 2^-24) of all-empty and of live passes"""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch

from bench import full_frame_rays
from posegen_amd import surreal_config, synthetic as syn
from posegen_amd.raycaster import HipRayCaster


PERM16 = [1, 2, 16, 17, 0, 12, 4, 5, 18, 19, 3, 13, 7, 8, 20, 21, 6, 14, 10, 11, 22, 23, 9, 15]     # pg_layout.h: slot -> joint
LIMBS = [[PERM16[6 * g + jj] for g in range(4)] for jj in range(6)]                                    # limb jj = its four joints
LOG2E = 1.4426950408889634


def limbs_in_range(rb, z, skts, cfg, tau_v, tau_d):
    """[n, S, 6] bool: point (ray, sample) is in range of limb jj -- within cutoff + 24 / (tau log2 e) of one of its four joints
    in that joint's bone-local frame, for the wider of the two embedders (pg_eval16r.hip: the distance beyond which a joint's
    cutoff weight is below 2^-24).  rb [n, 11], z [n, S], skts [J, 4, 4] or [n, J, 4, 4]; CPU tensors."""
    pts = (rb[:, None, 0:3] + rb[:, None, 3:6] * z[..., None]).double()
    sk = skts.double().reshape(-1, 24, 4, 4)
    q = torch.einsum("njab,nsb->nsja", sk[..., :3, :3], pts) + sk[:, None, :, :3, 3]
    far = float(cfg.cutoff_dist) + 24.0 / (min(float(tau_v), float(tau_d)) * LOG2E)
    near = q.norm(dim=-1) < far                                                 # [n, S, J]
    return torch.stack([near[..., l].any(-1) for l in LIMBS], -1)


def pass_figures(sigma, near, pts=256):
    """Pass-level figures of one launch: sigma [n, S] and limbs_in_range [n, S, 6] in launch order, passes of `pts` consecutive
    points in waves of 32 (points past the end of the launch count as empty and in range of nothing)."""
    sg = sigma.reshape(-1)
    nr = near.reshape(-1, near.shape[-1])
    pad = -sg.numel() % pts
    live = torch.cat([sg > 0, torch.zeros(pad, dtype=torch.bool)]).reshape(-1, pts // 32, 32).any(-1)         # [pass, wave]
    limbs = torch.cat([nr, torch.zeros(pad, nr.shape[1], dtype=torch.bool)]).reshape(-1, pts, nr.shape[1]).any(1)   # [pass, limb]
    nlive = live.sum(1)
    empty = nlive == 0
    nl = limbs.sum(1).double()
    return {"passes": int(live.shape[0]), "all_empty_passes_frac": float(empty.double().mean()),
            "live_waves_hist": torch.bincount(nlive, minlength=pts // 32 + 1).tolist(),
            "limbs_in_range_all_empty": float(nl[empty].mean()) if bool(empty.any()) else 0.0,
            "limbs_in_range_live": float(nl[~empty].mean()) if bool((~empty).any()) else 0.0,
            "limbs_left_out_frac": float(1.0 - nl.mean() / nr.shape[1]),
            "passes_with_limbs_in_and_out": int(((nl > 0) & (nl < nr.shape[1])).sum())}


def oracle_share(res, blocks=32, per=128):
    from oracle import anerf_oracle as orc
    cfg = surreal_config()
    wc, wf, tv, td = syn.make_model(cfg, 0)
    tw = lambda w: {k: torch.tensor(v) for k, v in w.items()}
    *_, rb, skts, cyl = full_frame_rays(res, res, "cpu")
    n = rb.shape[0]
    tot = {"raw_coarse": [0, 0, 0, 0], "raw_fine": [0, 0, 0, 0]}
    sig, rng = {}, {}
    for b in range(blocks):
        s = int(b * (n - per) / (blocks - 1)) // 2 * 2
        with torch.no_grad():
            ex = orc.render_rays(rb[s:s + per], skts, cyl, orc.OracleConfig(tau_v=tv, tau_d=td), tw(wc), tw(wf), cfg.n_samples,
                                 cfg.n_importance, return_extras=True)["extras"]
        for k, zk in (("raw_coarse", "z_coarse"), ("raw_fine", "z_fine")):
            sig.setdefault(k, []).append(ex[k][..., 3])
            rng.setdefault(k, []).append(limbs_in_range(rb[s:s + per], ex[zk], skts, cfg, tv, td))
        for k, t in tot.items():
            sg = ex[k][..., 3].reshape(-1)
            g = sg[:sg.numel() // 32 * 32].reshape(-1, 32) <= 0
            t[0] += int(g.all(1).sum()); t[1] += g.shape[0]; t[2] += int((sg <= 0).sum()); t[3] += sg.numel()
    print("EMPTY_WAVES_ORACLE " + json.dumps({k: {"rays": blocks * per, "groups": t[1], "empty_groups_frac": t[0] / t[1],
                                                  "points_sigma_le_0": t[2] / t[3]} for k, t in tot.items()}))
    # (a block is 128 rays: its 8192 / 10240 points are whole passes of 256)
    print("PASSES_ORACLE " + json.dumps({k: pass_figures(torch.cat(sig[k]), torch.cat(rng[k])) for k in tot}))


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
