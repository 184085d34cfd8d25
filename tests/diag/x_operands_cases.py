"""Child process of tests/test_gpu_x_operands.py: POSEGEN_MAX_WG is read once per process, so every grid renders in a process of
its own and reports, as one JSON line, a digest of every output array of every call -- and, with `ref`, how far the calls are
from the float64 restatement (tests/eval_ref.py) and what the limb masks left out.

    x_operands_cases.py [ref]

walk   render_rays with extras (no wave skips its colour branch) on rays through the body: 1 x 64 (one partial pass), 4 x 64
       (exactly one pass), 5 x 64 (second pass ragged), 13 x 80 (five passes, the last one 16 points), in both forms of the
       16x16x32 kernel, and 7 x 113 and 3 x 171 (513 points: the last pass is one point) with records; bf16 and fp16; one pose, a
       pose per ray, the h36m model with frame codes.  The fine launch of each call has 16 samples per ray more.
stage  pg_stage_eval on edge inputs of tests/eval_cases.py, both forms, both precisions: digests, and with `ref` max / RMS error
       against float64 with the bounds of tests/eval_cases.py.
masks  (`ref` only) the 13 x 80 call with the limb masks off against the default, and the kernel's own count of limbs left out
       per wave against the formula restated on the host in float64."""
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
from tests import eval_ref as er

DEV = "cuda:0"
PRECS = ("bf16", "fp16")
WALK_CALLS = ((1, 64, ("always", "records")), (4, 64, ("always", "records")), (5, 64, ("always", "records")),
              (13, 80, ("always", "records")), (7, 113, ("records",)), (3, 171, ("records",)))
PERM16 = [1, 2, 16, 17, 0, 12, 4, 5, 18, 19, 3, 13, 7, 8, 20, 21, 6, 14, 10, 11, 22, 23, 9, 15]     # pg_layout.h: slot -> joint


def stage_cases():
    return [ec.seams(1, 64), ec.seams(5, 64), ec.seams(13, 80), ec.seams(7, 113), ec.seams(3, 171),
            ec.all_far("all"), ec.all_far("first"), ec.all_far("last"), ec.on_joint(64),
            ec.cutoffs(ec.TAU_MODEL, -4.0), ec.cutoffs(400.0, 4.0)]


def digest(t):
    return hashlib.sha256(np.ascontiguousarray(t.detach().cpu().numpy()).tobytes()).hexdigest()


def body_rays(n):
    rb, skts, cyl, *_ = full_frame_rays(64, 64, torch.device(DEV))
    # row 32 from the body's middle (column 28) outwards in steps of four pixels: the first rays go through the trunk, the
    # 12th and 13th pass beside the body out of every limb's range -- waves and passes differ in their limbs in range
    cols = [28 + 4 * ((k + 1) // 2) * (1 if k % 2 else -1) for k in range(n)]
    idx = torch.tensor([32 * 64 + c for c in cols], device=rb.device)
    return rb[idx].contiguous(), skts, cyl


def walk(renderers, out):
    for conf, pose in (("surreal", "one"), ("surreal", "per_ray"), ("h36m", "one")):
        r = renderers[conf]
        for n, S, forms in WALK_CALLS:
            rb, skts, cyl = body_rays(n)
            cams = (torch.arange(n, device=DEV) % r.cfg.n_framecodes).float() if conf == "h36m" else None
            if pose == "per_ray":       # the frame's pose, moved a little from ray to ray
                skts = skts.reshape(1, 24, 4, 4).repeat(n, 1, 1, 1)
                skts[:, :, :3, 3] += 1e-3 * torch.sin(torch.arange(n, device=DEV, dtype=torch.float32))[:, None, None]
            for prec in PRECS:
                for form in forms:
                    r.set_precision(PREC_BY_NAME[prec])
                    r.set_onchip(form)
                    res = r.render_rays(rb, skts, cyl, cams=cams, n_samples=S, n_importance=16, want_alpha=False, extras=True)
                    torch.cuda.synchronize()
                    d = {k: digest(res[k]) for k in ("rgb_map", "disp_map", "acc_map")}
                    d["raw_coarse"] = digest(res["extras"]["raw_coarse"])
                    d["raw_fine"] = digest(res["extras"]["raw_fine"])
                    d["finite"] = bool(all(torch.isfinite(res["extras"][k]).all() for k in ("raw_coarse", "raw_fine"))
                                       and torch.isfinite(res["rgb_map"]).all())
                    out[f"walk:{conf}:{pose}:{n}x{S}:{prec}:{form}"] = d
                    r.set_onchip("auto")


def stage(renderers, out, ref):
    for case in stage_cases():
        r = renderers[case.model]
        cams = None if case.cams is None else torch.tensor(case.cams)
        for which in (0, 1):
            for prec in PRECS:
                for form in ("always", "records"):
                    try:
                        r.set_precision(PREC_BY_NAME[prec])
                        r.set_onchip(form)
                        r.set_embedder(0, case.tau_v, case.cutoff_v)
                        r.set_embedder(1, case.tau_d, case.cutoff_d)
                        raw = r.stage_eval(which, torch.tensor(case.ray_batch), torch.tensor(case.z), torch.tensor(case.skts), cams=cams)
                        torch.cuda.synchronize()
                    finally:
                        r.set_onchip("auto")
                        r.set_embedder(0, ec.TAU_MODEL)
                        r.set_embedder(1, ec.TAU_MODEL)
                    d = {"raw": digest(raw), "finite": bool(torch.isfinite(raw).all())}
                    if ref:
                        want = ec.reference(case, which)["raw"]
                        y = ec.yardstick(case, which, prec)
                        err = raw.cpu().double() - want
                        d.update(emax=float(err.abs().max()), bmax=ec.bound_16bit(prec, y), erms=float(err.pow(2).mean().sqrt()),
                                 brms=ec.RMS_FACTOR * y["rms"])
                    out[f"stage:{case.name}:{which}:{prec}:{form}"] = d


def host_limbs_left_out(rb, z, skts, radius):
    """The kernel's formula restated: limb jj (joint slots jj, 6 + jj, 12 + jj, 18 + jj) is left out by a wave of 32 consecutive
    points of a 256-point pass when |q| >= the joint's far radius for all four joints and all 32 points (points past the end of
    the call repeat its last point).  float64; also returns how close any (point, joint) comes to its radius, relatively."""
    pts = rb[:, None, 0:3].double() + rb[:, None, 3:6].double() * z[..., None].double()
    dist = torch.linalg.norm(er.bone_local(pts.numpy(), skts.numpy()), dim=-1).reshape(-1, 24).numpy()         # [points, joint]
    far = dist >= radius[None, :]
    n_pts = far.shape[0]
    passes = (n_pts + 255) // 256
    idx = np.minimum(np.arange(passes * 256), n_pts - 1).reshape(passes, 8, 32)
    count = 0
    for jj in range(6):
        joints = [PERM16[6 * g + jj] for g in range(4)]
        count += int(far[idx][..., joints].all(axis=(-1, -2)).sum())
    return count, passes, float(np.abs(dist / radius[None, :] - 1).min())


def masks(renderers, out):
    r = renderers["surreal"]
    n, S = 13, 80
    rb, skts, cyl = body_rays(n)
    radius = ec.Case("radius", "surreal", None).far_radius()
    for prec in PRECS:
        r.set_precision(PREC_BY_NAME[prec])
        r.set_onchip("always")
        try:
            on = r.render_rays(rb, skts, cyl, n_samples=S, n_importance=16, want_alpha=False, extras=True)
            r.set_far_skip(False)
            off = r.render_rays(rb, skts, cyl, n_samples=S, n_importance=16, want_alpha=False, extras=True)
        finally:
            r.set_far_skip(True)
        d = {k: float((on[k] - off[k]).abs().max()) for k in ("rgb_map", "acc_map", "rgb0", "acc0")}
        d["finite"] = bool(torch.isfinite(off["rgb_map"]).all())
        for which, zk in ((0, "z_coarse"), (1, "z_fine")):
            z = on["extras"][zk]
            st = r.limb_skip_stats(which, rb, z, skts)
            want, passes, margin = host_limbs_left_out(rb.cpu(), z.cpu(), skts.cpu().reshape(1, 24, 4, 4), radius)
            d[f"count{which}"] = {"passes": st["passes"], "left_out": round(st["limbs_left_out_frac"] * 48 * st["passes"]),
                                  "host_passes": passes, "host_left_out": want, "margin": margin}
        r.set_onchip("auto")
        out[f"masks:{prec}"] = d


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
    print("X_OPERANDS " + json.dumps(out))


if __name__ == "__main__":
    main()
