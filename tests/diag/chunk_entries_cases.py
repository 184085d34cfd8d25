"""Child process of tests/test_gpu_chunk_entries.py: POSEGEN_MAX_WG is read once per process, so every grid renders in a process
of its own and reports, as one JSON line, a digest of every output array of every call, each call made three times -- and, with
`ref`, the comparisons that need no second grid.

    chunk_entries_cases.py [ref]

walk    render_rays with extras (raw_coarse / raw_fine are handed out, no wave skips its colour branch), bf16 and fp16, the on-chip
        and the record form of the 16x16x32 kernel: 1 ray x 32 samples (below the kernel's 64: it runs the direct kernel, pg_eval16.hip, and exercises nothing of the change),
        1 x 64, 5 x 64 (a last pass of 64 points), 13 x (64 + 16) (rays straddle passes at S = 80), 48 x (128 + 16) with frame
        codes, 40 rays with a pose each.  Three times each: a ring read that runs ahead of a refill shows as a changed byte.
stage   pg_stage_eval on edge inputs: rays with no limb in range of any pass (the ring starts fully masked), tau_d <= 0 (nothing is
        masked), and the rays, pose, per-joint cutoffs and taus of tests/golden/eval_edges.npz -- its 33 depths per ray with their
        midpoints between them, 66 per ray: the kernel takes rays of 64 samples or more.  With `ref`: max / RMS error against the
        float64 restatement (tests/eval_ref.py) with the bounds of tests/eval_cases.py.
masks   (`ref`) limb masks on against set_far_skip(False) on a 64 x 64 frame through the body at 64 + 16 samples; the empty-wave skip
        on against off there, maps only."""
import hashlib
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
import numpy as np
import torch

from bench import full_frame_rays
from posegen_amd import PREC_BY_NAME
from posegen_amd.raycaster import HipRayCaster
from tests import eval_cases as ec

DEV = "cuda:0"
PRECS = ("bf16", "fp16")
FORMS = ("always", "records")
# (config, pose, rays, coarse samples, importance samples)
WALK_CALLS = (("surreal", "one", 1, 32, 0), ("surreal", "one", 1, 64, 0), ("surreal", "one", 5, 64, 0), ("surreal", "one", 13, 64, 16),
              ("h36m", "one", 48, 128, 16), ("surreal", "per_ray", 40, 64, 16))
MAPS = ("rgb_map", "disp_map", "acc_map")


def digest(t):
    return hashlib.sha256(np.ascontiguousarray(t.detach().cpu().numpy()).tobytes()).hexdigest()


def body_rays(n):
    rb, skts, cyl, *_ = full_frame_rays(64, 64, torch.device(DEV))
    # row 32 from the body's middle (column 28) outwards, alternating sides: the first rays go through the trunk, the outer ones
    # pass beside the body out of every limb's range -- waves and passes differ in their limbs in range
    cols = [min(63, max(0, 28 + ((k + 1) // 2) * (1 if k % 2 else -1) * (4 if n <= 16 else 1))) for k in range(n)]
    idx = torch.tensor([32 * 64 + c for c in cols], device=rb.device)
    return rb[idx].contiguous(), skts, cyl


def edges_case():
    """eval_edges.npz at 66 samples per ray: every fixture depth, and the midpoint to the next one (the last: half a step on)"""
    g = np.load(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "golden", "eval_edges.npz"))
    assert int(g["seed_model"]) == ec.SEED["surreal"]
    z = g["z"].astype(np.float32)
    nxt = np.concatenate([z[:, 1:], 2 * z[:, -1:] - z[:, -2:-1]], axis=1)
    z66 = np.stack([z, 0.5 * (z + nxt)], axis=-1).reshape(z.shape[0], -1).astype(np.float32)
    assert z66.shape[1] == 66 and (np.diff(z66, axis=1) >= 0).all() and (z66[:, ::2] == z).all()
    return ec.Case("eval_edges_66", "surreal", g["skts"], g["cutoff_v"], g["cutoff_d"], float(g["tau_v"]), float(g["tau_d"]),
                   ray_batch=g["ray_batch"], z=z66)


def stage_cases():
    return [ec.all_far("all"), ec.cutoffs(ec.TAU_MODEL, -4.0), edges_case()]


def walk(renderers, out):
    for conf, pose, n, S, imp in WALK_CALLS:
        r = renderers[conf]
        rb, skts, cyl = body_rays(n)
        cams = (torch.arange(n, device=DEV) % r.cfg.n_framecodes).float() if conf == "h36m" else None
        if pose == "per_ray":       # the frame's pose, moved a little from ray to ray
            skts = skts.reshape(1, 24, 4, 4).repeat(n, 1, 1, 1)
            skts[:, :, :3, 3] += 1e-3 * torch.sin(torch.arange(n, device=DEV, dtype=torch.float32))[:, None, None]
        for prec in PRECS:
            for form in FORMS:
                reps = []
                try:
                    r.set_precision(PREC_BY_NAME[prec])
                    r.set_onchip(form)
                    for _ in range(3):
                        res = r.render_rays(rb, skts, cyl, cams=cams, n_samples=S, n_importance=imp, want_alpha=False, extras=True)
                        torch.cuda.synchronize()
                        d = {k: digest(res[k]) for k in MAPS}
                        raws = ["raw_coarse"] + (["raw_fine"] if imp else [])
                        for k in raws:
                            d[k] = digest(res["extras"][k])
                        d["finite"] = bool(all(torch.isfinite(res["extras"][k]).all() for k in raws) and torch.isfinite(res["rgb_map"]).all())
                        reps.append(d)
                finally:
                    r.set_onchip("auto")
                out[f"walk:{conf}:{pose}:{n}x{S}+{imp}:{prec}:{form}"] = reps


def stage(renderers, out, ref):
    for case in stage_cases():
        r = renderers[case.model]
        for which in (0, 1):
            for prec in PRECS:
                for form in FORMS:
                    reps = []
                    try:
                        r.set_precision(PREC_BY_NAME[prec])
                        r.set_onchip(form)
                        r.set_embedder(0, case.tau_v, case.cutoff_v)
                        r.set_embedder(1, case.tau_d, case.cutoff_d)
                        for _ in range(3):
                            raw = r.stage_eval(which, torch.tensor(case.ray_batch), torch.tensor(case.z), torch.tensor(case.skts))
                            torch.cuda.synchronize()
                            reps.append({"raw": digest(raw), "finite": bool(torch.isfinite(raw).all())})
                    finally:
                        r.set_onchip("auto")
                        r.set_embedder(0, ec.TAU_MODEL)
                        r.set_embedder(1, ec.TAU_MODEL)
                    if ref:
                        want = ec.reference(case, which)["raw"]
                        y = ec.yardstick(case, which, prec)
                        err = raw.cpu().double() - want
                        reps[-1].update(emax=float(err.abs().max()), bmax=ec.bound_16bit(prec, y), erms=float(err.pow(2).mean().sqrt()),
                                        brms=ec.RMS_FACTOR * y["rms"])
                    out[f"stage:{case.name}:{which}:{prec}:{form}"] = reps


def masks(renderers, out):
    r = renderers["surreal"]
    rb, skts, cyl, *_ = full_frame_rays(64, 64, torch.device(DEV))      # 4096 rays: the bound on the share of rays that differ needs many
    for prec in PRECS:
        for form in FORMS:
            r.set_precision(PREC_BY_NAME[prec])
            r.set_onchip(form)
            try:
                on = r.render_rays(rb, skts, cyl, n_samples=64, n_importance=16, want_alpha=False, extras=True)
                r.set_far_skip(False)
                off = r.render_rays(rb, skts, cyl, n_samples=64, n_importance=16, want_alpha=False, extras=True)
                r.set_far_skip(True)
                # (without extras no raw is handed out: the call may leave the colour branch of empty waves out)
                skip = r.render_rays(rb, skts, cyl, n_samples=64, n_importance=16, want_alpha=False)
                r.set_empty_skip(False)
                noskip = r.render_rays(rb, skts, cyl, n_samples=64, n_importance=16, want_alpha=False)
            finally:
                r.set_far_skip(True)
                r.set_empty_skip(True)
                r.set_onchip("auto")
            d = {}
            for k in ("rgb_map", "acc_map", "rgb0", "acc0"):
                diff = (on[k] - off[k]).abs().reshape(on[k].shape[0], -1)
                d[k] = {"max": float(diff.max()), "mean": float(diff.mean()), "frac": float((diff.amax(-1) > 0).float().mean())}
            d["finite"] = bool(torch.isfinite(off["rgb_map"]).all() and torch.isfinite(on["rgb_map"]).all())
            d["acc_max"] = float(on["acc_map"].max())
            d["empty_skip_same"] = {k: digest(skip[k]) == digest(noskip[k]) for k in MAPS + ("rgb0", "acc0")}
            out[f"masks:{prec}:{form}"] = d


def main():
    ref = len(sys.argv) > 1 and sys.argv[1] == "ref"
    renderers = {}
    for name in ("surreal", "h36m"):
        cfg, wc, wf = ec.model(name)
        renderers[name] = HipRayCaster.from_weights(cfg, wc, wf, ec.TAU_MODEL, ec.TAU_MODEL, device=DEV, precision="bf16").renderer
    out = {}
    walk(renderers, out)
    stage(renderers, out, ref)
    if ref:
        masks(renderers, out)
    for r in renderers.values():
        r.close()
    print("CHUNK_ENTRIES " + json.dumps(out))


if __name__ == "__main__":
    main()
