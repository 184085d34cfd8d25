"""Stream-ordering harness of tests/test_gpu_streams.py (a plain helper module; its tables import without a GPU).

Every compute entry point of include/posegen_hip.h takes the caller's stream.  On the default stream a kernel, memset or copy
issued on stream 0 instead, or a host staging array overwritten by the next call, is invisible: everything lands on one stream
and the tests synchronise after every call.  `run_decoy` makes such a mistake deterministic instead of a lucky race:

  1. the case runs on the default stream with a synchronise after each call -- the reference, and the warm-up that grows
     every buffer of the handle;
  2. the device inputs are overwritten with a decoy (a second VALID input of the same shapes), memory of the outputs' sizes is
     soaked with a sentinel, and everything is synchronised;
  3. on a non-blocking side stream a delay (a chain of matrix products, >= 50 ms) is enqueued, and BEHIND it the copies that put
     the real inputs in place; then the case is called twice back to back, with different host arrays, nothing synchronised
     between.  Work that the library or a wrapper puts on another stream runs at once, during the delay, and reads the decoy;
     an accumulator zeroed on another stream is zeroed before the first call's kernel has added into it; a staging array that
     the second call overwrites while the first copy has not read it gives the first call the second call's indices;
  4. both results must be the reference's bytes;
  5. the delay must still be pending when the two calls have returned, for every entry point that the header documents as
     asynchronous (ASYNCHRONOUS) -- which also proves that step 3's order was the one described.

The tables below are data: tests/test_stream_cases_host.py checks them against the header without a GPU."""
import os
import re

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(REPO, "include", "posegen_hip.h")

# ---- the case table: case of tests/test_gpu_streams.py -> the stream-taking entry points it calls -------------------------------
CASES = {
    "render_rays_fp32": ("pg_render_rays",),
    "render_rays_train": ("pg_render_rays_train",),
    "query_density": ("pg_query_density",),
    "grid_mesh": ("pg_grid_density", "pg_mesh_count", "pg_mesh_emit"),
    "train_fp32": ("pg_train_forward", "pg_train_backward"),
    "train_pose": ("pg_train_backward_pose",),
    "load_weights_device": ("pg_load_weights_device",),
    "train_loss": ("pg_train_loss",),
    "pose_reg_loss": ("pg_pose_reg_loss",),
    "grad_norms": ("pg_grad_norms",),
    "kinematics_boxes_frame": ("pg_pose_kinematics", "pg_pose_boxes", "pg_render_frame"),
    "frame_ranges_compose": ("pg_render_frame_range", "pg_compose_frame"),
    "stage_frame_rays": ("pg_stage_frame_rays",),
    "render_scene": ("pg_render_scene",),
    "stage_scene_composite": ("pg_stage_scene_composite",),
    "batch_chain": ("pg_pixel_index_count", "pg_pixel_index_emit", "pg_batch_sample_pixels", "pg_batch_gather"),
    "regressor_input": ("pg_regressor_input",),
    "frame_metrics": ("pg_frame_metrics",),
    "frame_metrics_val": ("pg_frame_metrics_val",),
    "pose_scores": ("pg_pose_scores",),
    "pose_loss": ("pg_pose_loss",),
    "vertex_errors": ("pg_vertex_errors",),
    "poseopt": ("pg_poseopt_forward", "pg_poseopt_backward"),
    "kinematics_rot": ("pg_pose_kinematics_rot",),
    "kinematics_bwd": ("pg_pose_kinematics_bwd",),
    "kinematics_rot_bwd": ("pg_pose_kinematics_rot_bwd",),
    "smpl": ("pg_smpl_forward", "pg_smpl_backward"),
    "stage_composite_bwd": ("pg_stage_composite_bwd",),
    "stage_merged_composite_bwd": ("pg_stage_merged_composite_bwd",),
}

# Further cases that run entry points of the table again in another configuration (an entry point is NAMED by one case above;
# these add paths of it): case -> the entry points it re-runs.
VARIANTS = {
    "render_rays_bf16_records": ("pg_render_rays",),
    "render_rays_fp16c": ("pg_render_rays",),
    "render_rays_per_ray_poses": ("pg_render_rays",),
    "render_rays_frame_codes": ("pg_render_rays",),
    "train_bf16": ("pg_train_forward", "pg_train_backward"),
    "train_frame_codes": ("pg_train_forward", "pg_train_backward"),
    "train_single": ("pg_train_forward", "pg_train_backward"),
    "train_single_coarse": ("pg_train_forward", "pg_train_backward"),
}

# pg_stage_* entry points without a case of their own: stage entry -> (case, reason).  The reason names the launcher that the stage
# entry point and the case's entry point both call with the caller's stream; tests/test_stream_cases_host.py checks that the
# launcher is a symbol of posegen_amd/csrc and that pg_api.hip calls it in more than one place.  The two composite-backward stage
# entry points launch their kernels themselves (pg_train.hip) and therefore have cases of their own.
COVERED_BY = {
    "pg_stage_sample_coarse": ("render_rays_fp32", "pg_launch_sample_coarse, which the coarse stage of pg_render_rays calls with the same stream argument"),
    "pg_stage_sample_coarse_draws": ("render_rays_train", "pg_launch_sample_coarse with t_rand, as the coarse stage of pg_render_rays_train calls it"),
    "pg_stage_eval": ("render_rays_fp32", "launch_eval, the one eval call of pg_api.hip that every render pass goes through"),
    "pg_stage_composite": ("render_rays_fp32", "pg_launch_composite, the composite launch of both passes of pg_render_rays"),
    "pg_stage_composite_form": ("render_rays_train", "pg_launch_composite with noise and draws, as pg_render_rays_train calls it"),
}

# entry points that wait for the stream by contract: name -> the header sentence that says so
SYNCHRONISES = {
    "pg_mesh_count": "pg_mesh_count synchronises the stream",
}

# entry points the header documents as asynchronous: name -> the header's words.  A case all of whose entry points are here must
# leave the delay pending when its two back-to-back calls have returned.
_BATCH = "All are asynchronous on `stream`"
_TRAINER = "asynchronous on `stream`, no host synchronisation"
_ASYNC = "Asynchronous on `stream`"
_STAGE = "pg_stage_* entry points are asynchronous with respect to the host"
ASYNCHRONOUS = {
    "pg_render_rays": "pg_render_rays and the pg_stage_* entry points are asynchronous with respect to the host",
    "pg_poseopt_forward": _ASYNC, "pg_poseopt_backward": _ASYNC, "pg_render_frame_range": _ASYNC, "pg_stage_frame_rays": _ASYNC,
    "pg_pixel_index_count": _BATCH, "pg_pixel_index_emit": _BATCH, "pg_batch_sample_pixels": _BATCH, "pg_batch_gather": _BATCH,
    "pg_regressor_input": _ASYNC, "pg_frame_metrics": _ASYNC, "pg_frame_metrics_val": _ASYNC, "pg_render_scene": _ASYNC,
    "pg_pose_scores": _ASYNC, "pg_smpl_forward": _ASYNC, "pg_smpl_backward": _ASYNC, "pg_pose_kinematics_bwd": _ASYNC,
    "pg_pose_kinematics_rot_bwd": "otherwise as pg_pose_kinematics_bwd", "pg_pose_loss": _ASYNC,
    "pg_train_loss": _TRAINER, "pg_pose_reg_loss": _TRAINER, "pg_grad_norms": _TRAINER,
    "pg_stage_scene_composite": _STAGE, "pg_stage_composite_bwd": _STAGE, "pg_stage_merged_composite_bwd": _STAGE,
}

# Chains that mix documented-asynchronous entry points with others: case -> the entry points whose part of the chain ends at a
# probe (`stage_done`), where the delay must still be pending although the case as a whole makes no such promise.
PROBES = {
    "frame_ranges_compose": ("pg_render_frame_range",),
}


def header_text() -> str:
    with open(HEADER) as f:
        return f.read()


def stream_entry_points(text=None):
    """every function of the header with a `void* stream` parameter, in the header's order"""
    text = header_text() if text is None else text
    code = re.sub(r"/\*.*?\*/", " ", text, flags=re.S)
    return [m.group(1) for m in re.finditer(r"\bint\s+(pg_\w+)\s*\(([^;]*?)\)\s*;", code, flags=re.S) if re.search(r"void\s*\*\s*stream\b", m.group(2))]


def must_stay_pending(entry_points) -> bool:
    return all(e in ASYNCHRONOUS and e not in SYNCHRONISES for e in entry_points)


def asserted_pending():
    """every entry point whose asynchrony some case asserts: at the end of a case all of whose entry points are documented as
    asynchronous, or at a probe inside a mixed chain"""
    out = set()
    for table in (CASES, VARIANTS):
        for eps in table.values():
            if must_stay_pending(eps):
                out.update(eps)
    for eps in PROBES.values():
        assert must_stay_pending(eps), eps
        out.update(eps)
    return out


# ---- the GPU side (torch is imported on use) --------------------------------------------------------------------------------------
DELAY_MIN_MS = 50.0
DELAY_CAP_MS = 2000.0
SENTINEL = 12345.0


_probe = None        # while the side-stream calls of a case run: (the delay's event, list of (entry points, pending))


def stage_done(entry_points):
    """Called by a case's `run` between the stages of a chain: notes whether the delay is still pending now that the calls of
    `entry_points` have returned.  Outside the side-stream run of `run_decoy` it does nothing."""
    if _probe is not None:
        _probe[1].append((tuple(entry_points), not _probe[0].query()))


class Mismatch(AssertionError):
    """a result of the side-stream run is not the reference's bytes"""


class Delay:
    """>= 50 ms of public torch work on the side stream: a chain of fp32 torch.mm on two 4096 x 4096 tensors, its length calibrated
    once against the delay alone (timed with events, doubled until it lasts DELAY_MIN_MS; more than DELAY_CAP_MS is a failure)."""

    def __init__(self, side, device):
        import torch
        self.side = side
        g = torch.Generator(device="cpu").manual_seed(11)
        with torch.cuda.stream(side):
            self.a = (torch.randn(4096, 4096, generator=g) / 64).to(device)
            self.b = (torch.randn(4096, 4096, generator=g) / 64).to(device)
            self.c = torch.empty(4096, 4096, device=device)
            self.enqueue(2)                                          # (the BLAS library's own set-up is not part of the timing)
        side.synchronize()
        n = 8
        while True:
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            with torch.cuda.stream(side):
                e0.record(side)
                self.enqueue(n)
                e1.record(side)
            side.synchronize()
            ms = e0.elapsed_time(e1)
            if ms > DELAY_CAP_MS:
                raise AssertionError(f"the delay chain of {n} products lasts {ms:.0f} ms: above the cap of {DELAY_CAP_MS:.0f} ms")
            if ms >= DELAY_MIN_MS:
                break
            n *= 2
        self.n, self.ms = n, ms
        print(f"stream harness: delay = {n} x mm(4096^2) = {ms:.1f} ms")

    def enqueue(self, n=None):
        import torch
        for _ in range(self.n if n is None else n):
            torch.mm(self.a, self.b, out=self.c)


def _bytes_equal(a, b) -> bool:
    import torch
    if a.shape != b.shape or a.dtype != b.dtype:
        return False
    a, b = a.contiguous().reshape(-1), b.contiguous().reshape(-1)
    return bool(torch.equal(a.view(torch.uint8), b.view(torch.uint8)))


def _to_device(dev_inputs, device):
    return {k: v.to(device).contiguous() for k, v in dev_inputs.items()}


def _host_copy(out):
    return {k: v.detach().cpu().clone() for k, v in out.items()}


def run_decoy(name, make, run, side, delay, device, pend=None, between=None):
    """The decoy pattern for one case.  `make(variant)` -> (dev, host) for variant "A", "A2", "B": `dev` a dict of host tensors that
    become the case's device inputs, `host` whatever else `run` takes (host arrays, scalars).  `run(dev, host)` -> dict of device
    tensors: one call of the entry point (or chain) on the CURRENT stream, without synchronising unless the entry point does.
    `pend`: the delay must still be pending after the two calls (None: no assertion, the flag is only reported).
    `between`: called between the reference runs and before each side run (e.g. to clear gradients).
    A chain may call `stage_done(entry_points)` between its stages: the delay must be pending there too where those are documented
    as asynchronous.  Returns {"delay_ms", "pending", "probes"}; raises Mismatch."""
    import torch
    A, A2, B = make("A"), make("A2"), make("B")
    # 1. the reference on the default stream, a full synchronise after each call (also the warm-up that grows every buffer)
    refs = []
    for dev_in, host in (A, A2, B):
        if between:
            between()
        out = run(_to_device(dev_in, device), host)
        torch.cuda.synchronize()
        refs.append(_host_copy(out))
    ref1, ref2, refB = refs
    differs = lambda x, y: any(not _bytes_equal(x[k], y[k]) for k in x)
    assert not A[0] or differs(ref1, refB), f"{name}: the decoy input gives the reference's result: it would hide a read of the decoy"
    assert differs(ref1, ref2), f"{name}: the second input gives the first one's result"
    # 2. decoys in the device inputs, sentinels in memory of the outputs' sizes (the side stream's allocator pool hands these
    #    blocks to the calls' own torch.empty), everything synchronised
    x1, x2 = _to_device(B[0], device), _to_device(B[0], device)
    srcA, srcA2 = _to_device(A[0], device), _to_device(A2[0], device)
    keep = [x1, x2, srcA, srcA2]
    with torch.cuda.stream(side):
        soak = [torch.full(v.shape, SENTINEL if v.dtype.is_floating_point else 90, dtype=v.dtype, device=device)
                for r in (ref1, ref2) for v in r.values() if v.numel()]
    side.synchronize()
    del soak
    torch.cuda.synchronize()
    # 3. the side stream: delay, the real inputs behind it, two calls back to back
    e0, ev_delay = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    with torch.cuda.stream(side):
        e0.record(side)
        delay.enqueue()
        ev_delay.record(side)
        assert not ev_delay.query(), f"{name}: the delay had finished before anything was enqueued behind it"
        for k in x1:
            x1[k].copy_(srcA[k])
            x2[k].copy_(srcA2[k])
        global _probe
        _probe = (ev_delay, [])
        try:
            if between:
                between()
            o1 = run(x1, A[1])
            if between:
                between()
            o2 = run(x2, A2[1])
            pending = not ev_delay.query()
            probes = _probe[1]
        finally:
            _probe = None
        c1 = {k: v.detach().clone() for k, v in o1.items()}
        c2 = {k: v.detach().clone() for k, v in o2.items()}
        keep += [o1, o2, c1, c2]
        side.synchronize()
    torch.cuda.synchronize()
    ms = e0.elapsed_time(ev_delay)
    print(f"stream case {name}: delay {ms:.1f} ms, still pending when both calls had returned: {pending}")
    # 4. both results are the reference's bytes
    for tag, got, ref in (("first", c1, ref1), ("second", c2, ref2)):
        for k in ref:
            if not _bytes_equal(got[k].cpu(), ref[k]):
                d = ""
                if got[k].dtype.is_floating_point and got[k].shape == ref[k].shape and ref[k].numel():
                    d = f" (max |difference| {float((got[k].cpu().double() - ref[k].double()).abs().nan_to_num(nan=float('inf')).max()):.3e})"
                raise Mismatch(f"{name}: output {k!r} of the {tag} of two back-to-back calls on a busy side stream is not the "
                               f"default-stream result{d}")
    # 5. asynchrony
    assert name not in PROBES or any(eps == PROBES[name] for eps, _ in probes), f"{name}: no probe after {PROBES.get(name)}"
    for eps, was_pending in probes:
        print(f"stream case {name}: after {', '.join(eps)}: still pending: {was_pending}")
        assert was_pending or not must_stay_pending(eps), (f"{name}: {', '.join(eps)} documented as asynchronous, but the {ms:.0f} ms delay in "
                                                           "front had finished when the calls returned: a call blocked the host")
    if pend:
        assert pending, (f"{name}: documented as asynchronous, but the {ms:.0f} ms delay in front of it had finished when the two calls "
                         "returned: a call blocked the host")
    del keep
    return {"delay_ms": ms, "pending": pending, "probes": probes}
