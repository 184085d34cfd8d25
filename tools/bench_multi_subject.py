"""Multi-subject batches (BASELINE config 4: "multi-subject batch render"): what it costs to alternate subjects between frames.

Two workloads -- config 4's frame (h36m: 512 x 512 full frame, 128 + 16 samples, a frame-code index per ray) and the GAN loop's
render call (ganloop.render_for_regressor: 20 culled 512 x 512 surreal frames) -- each three ways:
  one_subject          one model, every frame;
  bank_round_robin     S = 4 subjects, frame f with subject f % 4, through ONE caster (the subject bank);
  casters_round_robin  the same frames through four separate one-subject casters.
One JSON line per case is appended to profiles/multi_subject.jsonl: ms per frame, image_bytes per subject, image_builds after
warm-up (and after the timed run: steady state builds nothing), device memory in use.  The round-robin numbers are reported, not
asserted: nobody had measured alternating 4 x 2 weight images through L2 between frames.

    python tools/bench_multi_subject.py [--prec bf16] [--frames 20] [--reps 5] [--subjects 4] [--tag this-commit]
    python tools/bench_multi_subject.py --baseline     # only the one-subject cases, no bank call at all: runs on a checkout
                                                       # from before the bank (the same box's baseline for the file)
"""
import argparse, json, os, sys, time
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
import torch
from bench import full_frame_rays
from posegen_amd import h36m_config, surreal_config, synthetic as syn
from posegen_amd.ganloop import render_for_regressor
from posegen_amd.raycaster import HipRayCaster
from posegen_amd.skeleton import SURREAL_REST_SCALE, smpl_rest_pose

ap = argparse.ArgumentParser()
ap.add_argument("--prec", default="bf16")
ap.add_argument("--frames", type=int, default=20)
ap.add_argument("--reps", type=int, default=5)
ap.add_argument("--subjects", type=int, default=4)
ap.add_argument("--tag", default="this-commit")
ap.add_argument("--baseline", action="store_true")
ap.add_argument("--out", default=os.path.join(REPO, "profiles", "multi_subject.jsonl"))
a = ap.parse_args()
dev = torch.device("cuda:0")
S = a.subjects


def mem_in_use():
    free, total = torch.cuda.mem_get_info(dev)
    return int(total - free)


def info(casters):
    """image bytes / builds per subject over the casters of a case (a bank: one caster, S subjects)"""
    rows = []
    for c in casters:
        r = c.renderer
        if hasattr(r, "subject_info"):
            rows += [r.subject_info(s) for s in range(r.n_subjects)]
    return {"image_bytes_per_subject": [i["image_bytes"] for i in rows], "image_builds": [i["image_builds"] for i in rows]}


def timed(fn):
    fn()                                    # warm-up: every subject renders once, every image is packed
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(a.reps):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / a.reps * 1e3 / a.frames


def emit(workload, case, ms, casters, warm):
    line = {"tag": a.tag, "workload": workload, "case": case, "prec": a.prec, "frames": a.frames, "subjects": 1 if case == "one_subject" else S,
            "ms_per_frame": round(ms, 4), "device_bytes_in_use": mem_in_use(), "image_builds_after_warmup": warm["image_builds"], **info(casters)}
    print(json.dumps(line), flush=True)
    with open(a.out, "a") as f:
        f.write(json.dumps(line) + "\n")


def run_case(workload, case, make_casters, frame_fn):
    """frame_fn(casters, f) enqueues frame f; warm-up, builds after warm-up, timed reps"""
    casters = make_casters()
    call = lambda: [frame_fn(casters, f) for f in range(a.frames)]
    call()
    torch.cuda.synchronize()
    warm = info(casters)
    ms = timed(call)
    emit(workload, case, ms, casters, warm)
    for c in casters:
        c.renderer.close()
    del casters
    torch.cuda.empty_cache()


# ---- config 4's frame: h36m, 128 + 16, frame codes ------------------------------------------------------------------------
cfg4 = h36m_config()
rb, skts, cyl, *_ = full_frame_rays(512, 512, dev)
cams = (torch.arange(rb.shape[0], device=dev) % cfg4.n_framecodes).float()
h36m_frame = lambda r: r.render_rays(rb, skts, cyl, cams=cams, want_alpha=False)
one4 = lambda seed: HipRayCaster.from_weights(cfg4, *syn.make_model(cfg4, seed), device=dev, precision=a.prec)
W4 = "h36m 512x512 full frame, 128+16, frame codes (config 4)"
run_case(W4, "one_subject", lambda: [one4(0)], lambda cs, f: h36m_frame(cs[0].renderer))
if not a.baseline:
    def bank_frame(cs, f):
        cs[0].renderer.select_subject(f % S)
        h36m_frame(cs[0].renderer)
    run_case(W4, "bank_round_robin", lambda: [HipRayCaster.from_subjects(cfg4, [syn.make_model(cfg4, s) for s in range(S)], device=dev, precision=a.prec)],
             bank_frame)
    run_case(W4, "casters_round_robin", lambda: [one4(s) for s in range(S)], lambda cs, f: h36m_frame(cs[f % S].renderer))

# ---- the GAN loop's call: 20 culled 512 x 512 surreal frames ---------------------------------------------------------------
cfg5 = surreal_config()
H = W = 512
rest = smpl_rest_pose * SURREAL_REST_SCALE
c2ws, focals = syn.make_camera(1, H, W)
bones = torch.tensor(syn.make_bones(a.frames, 7), device=dev)
one5 = lambda seed: HipRayCaster.from_weights(cfg5, *syn.make_model(cfg5, seed), device=dev, precision=a.prec)
gan = lambda c, b, **kw: render_for_regressor(c, b, rest, c2ws[0], H, W, float(focals[0]), ext_scale=cfg5.ext_scale, **kw)
W5 = f"GAN loop render call: {a.frames} culled 512x512 surreal frames, 64+16"


def run_call(case, make_casters, call_fn):
    casters = make_casters()
    call_fn(casters)
    torch.cuda.synchronize()
    warm = info(casters)
    ms = timed(lambda: call_fn(casters))
    emit(W5, case, ms, casters, warm)
    for c in casters:
        c.renderer.close()
    torch.cuda.empty_cache()


run_call("one_subject", lambda: [one5(0)], lambda cs: gan(cs[0], bones))
if not a.baseline:
    subj = [f % S for f in range(a.frames)]
    run_call("bank_round_robin", lambda: [HipRayCaster.from_subjects(cfg5, [syn.make_model(cfg5, s) for s in range(S)], device=dev, precision=a.prec)],
             lambda cs: gan(cs[0], bones, subject_idxs=subj))
    # four casters: each renders its own frames of the call (f % S == s), the call's frames stitched by the caller
    idx = [torch.tensor([f for f in range(a.frames) if f % S == s], device=dev) for s in range(S)]
    run_call("casters_round_robin", lambda: [one5(s) for s in range(S)], lambda cs: [gan(cs[s], bones[idx[s]]) for s in range(S)])
