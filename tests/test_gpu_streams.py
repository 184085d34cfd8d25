"""Every stream-taking entry point of include/posegen_hip.h on a busy, non-blocking side stream (tests/stream_harness.py): the
same bytes as on the default stream, from two calls enqueued back to back behind work that has not finished, with the real
inputs put in place only behind that work.  Through the Python wrapper where there is one (its temporaries and uploads are then
part of what is tested), through ctypes otherwise.  The case table and what it must cover: stream_harness.CASES, checked against
the header by tests/test_stream_cases_host.py.

A case that owns its output tensors (the ctypes cases) fills them with a sentinel on the current stream in front of the call,
so that zeroing or writing them from another stream cannot go unnoticed.  Where a wrapper allocates its own outputs that is not
possible: the harness soaks blocks of the outputs' sizes in the side stream's allocator pool instead, which is where the
wrappers' torch.empty takes them from (a heuristic: a temporary of the same size may take a block first)."""
import ctypes as C
import types

import numpy as np
import pytest
import torch

from posegen_amd import _ffi, surreal_config, synthetic as syn
from tests import stream_harness as sh
from tests.helpers import cfg_from_golden, load_golden, loss_of, model_for, single_cfg, single_model

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
H, W = 48, 64                     # frames: 64 x 48, boxes off the square and inside the frame
VARIANT = {"A": 0, "A2": 1, "B": 2}
_ptr = lambda t: None if t is None else C.c_void_p(t.data_ptr())


def _sentinel(*shape, dtype=torch.float32):
    """an output tensor the case owns, filled on the CURRENT stream: behind everything that another stream could do to it early"""
    return torch.full(shape, sh.SENTINEL if dtype.is_floating_point else 90, dtype=dtype, device=DEV)


def _rng(name, variant):
    return np.random.RandomState(1000 * (sum(map(ord, name)) % 997) + VARIANT[variant])


def _t(a, dtype=torch.float32):
    return torch.as_tensor(np.ascontiguousarray(a)).to(dtype)


class Env:
    """what the cases share: the side stream, the calibrated delay, renderers by configuration, built on first use"""

    def __init__(self):
        self.dev = torch.device(DEV)
        self.side = torch.cuda.Stream(self.dev)
        self.delay = sh.Delay(self.side, self.dev)
        self._made = {}
        self.report = {}

    def get(self, key, build):
        if key not in self._made:
            self._made[key] = build()
            torch.cuda.synchronize()
        return self._made[key]

    def caster(self, key="main", golden="rays_surreal", precision="fp32"):
        def build():
            from posegen_amd.raycaster import HipRayCaster
            g = load_golden(golden)
            cfg = cfg_from_golden(g)
            wc, wf, tv, td = model_for(cfg, int(g["seed_model"]))
            return HipRayCaster.from_weights(cfg, wc, wf, float(g["tau_v"]), float(g["tau_d"]), device=DEV, precision=precision)
        return self.get(("caster", key), build)

    def trainable(self, key, golden="train_grads", **kw):
        def build():
            from posegen_amd.train import TrainableRayCaster
            m = TrainableRayCaster(self.caster(("train", key), golden), **kw)
            m.train()
            return m
        return self.get(("trainable", key), build)

    def trainable_single(self):
        def build():
            from posegen_amd.raycaster import HipRayCaster
            from posegen_amd.train import make_trainable
            g = load_golden("train_grads_single")
            cfg = single_cfg(g)
            w, tv, td = single_model(cfg, g)
            c = self._made[("caster", "single")] = HipRayCaster.from_weights(cfg, w, None, float(g["tau_v"]), float(g["tau_d"]), device=DEV,
                                                                             precision="fp32")
            m = make_trainable(c, train_precision="fp32")
            m.train()
            return m
        return self.get(("trainable", "single"), build)

    def close(self):
        torch.cuda.synchronize()
        for k, v in self._made.items():
            if k[0] == "caster":
                v.renderer.close()


@pytest.fixture(scope="module")
def env():
    e = Env()
    yield e
    e.close()
    print("stream cases:", {k: (round(v["delay_ms"], 1), v["pending"]) for k, v in e.report.items()})


def check(env, name, make, run, between=None, entry_points=None, warm=0):
    """`warm`: calls on the default stream in front of the case -- as many as the library's upload ring has slots, so that the
    side-stream calls take slots that have been used (the reuse path with its event wait, device buffers that hold valid items)"""
    eps = entry_points or sh.CASES.get(name) or sh.VARIANTS[name]
    for _ in range(warm):
        dev_in, host = make("A")
        run({k: v.to(env.dev) for k, v in dev_in.items()}, host)
    torch.cuda.synchronize()
    env.report[name] = sh.run_decoy(name, make, run, env.side, env.delay, env.dev, pend=sh.must_stay_pending(eps), between=between)


# ---- the premise and the negative controls (torch ops only) ------------------------------------------------------------------------

def test_control_c_streams_are_independent(env):
    """The premise: a trivial op on the default stream, enqueued while the side stream sits in the delay, completes before the delay."""
    x = torch.zeros(16, device=DEV)
    x.add_(1.0)                                     # (the first launch of a kernel loads its code: not part of what is timed)
    torch.cuda.synchronize()
    ev_delay, ev_op = torch.cuda.Event(), torch.cuda.Event()
    with torch.cuda.stream(env.side):
        env.delay.enqueue()
        ev_delay.record(env.side)
    x.add_(1.0)
    ev_op.record(torch.cuda.default_stream(env.dev))
    ev_op.synchronize()
    independent = not ev_delay.query()
    torch.cuda.synchronize()
    assert independent, ("an op on the default stream did not complete while the side stream sat in the delay: the streams are not "
                         "independent on this machine, and no case of this module can see a wrongly ordered operation")


def _vec(name):
    def make(v):
        return {"x": _t(_rng(name, v).uniform(1, 2, 1000))}, None
    return make


def test_control_a_work_on_the_default_stream_is_reported(env):
    """A fake entry point that computes on the default stream reads the decoy: the harness reports a mismatch."""
    def run(dev, host):
        out = torch.empty_like(dev["x"])
        with torch.cuda.stream(torch.cuda.default_stream(env.dev)):
            out.copy_(2 * dev["x"])
        return {"y": out}
    with pytest.raises(sh.Mismatch, match="first"):
        sh.run_decoy("control_a", _vec("control_a"), run, env.side, env.delay, env.dev)
    torch.cuda.synchronize()


def test_control_b_an_accumulator_zeroed_on_the_default_stream_is_reported(env):
    """A fake entry point that zeroes its accumulator on the default stream and adds into it on the current one: the zeroing of the
    second call overtakes the first call's addition, and the second result is reported."""
    acc = torch.zeros(1000, device=DEV)

    def run(dev, host):
        with torch.cuda.stream(torch.cuda.default_stream(env.dev)):
            acc.zero_()
        acc.add_(dev["x"])
        return {"y": acc.clone()}
    with pytest.raises(sh.Mismatch, match="second"):
        sh.run_decoy("control_b", _vec("control_b"), run, env.side, env.delay, env.dev)
    torch.cuda.synchronize()


def test_the_harness_passes_a_correctly_ordered_fake(env):
    """... and does not cry wolf: the same fake entry points on the current stream pass, with the delay still pending."""
    acc = torch.zeros(1000, device=DEV)

    def run(dev, host):
        acc.zero_()
        acc.add_(2 * dev["x"])
        return {"y": acc.clone()}
    rep = sh.run_decoy("control_ok", _vec("control_ok"), run, env.side, env.delay, env.dev, pend=True)
    assert rep["pending"]


# ---- ray rendering -------------------------------------------------------------------------------------------------------------------

def _ray_inputs(g, n, name, per_ray=False, cams=False, draws=None, S=0, N=0):
    rb, sk, cy = _t(g["ray_batch"]), _t(g["skts"]).reshape(-1, 24, 4, 4)[:1], _t(g["cyl"]).reshape(-1, 5)[:1]
    assert rb.shape[0] >= 3 * n
    other = _t(syn.make_pose(3, 9)[2])

    def make(v):
        i = VARIANT[v]
        rng = _rng(name, v)
        pose = sk if v != "B" else other[:1]
        d = {"rb": rb[i * n:(i + 1) * n], "skts": pose, "cyl": cy}
        if per_ray:             # a pose per ray: the call's own pose and two more, in an order that differs between the variants
            pick = rng.randint(0, 3, n)
            d["skts"] = torch.cat([sk, other[1:]])[torch.as_tensor(pick)].contiguous()
        if cams:
            d["cams"] = _t((np.asarray(g["cams"][i * n:(i + 1) * n]) + i) % int(g["n_framecodes"]))
        for k in draws or ():
            shape = {"t_rand": (n, S), "u_rand": (n, N), "noise0": (n, S), "noise1": (n, S + N)}[k]
            d[k] = _t(rng.uniform(0.0, 1.0, shape) * (1.0 if k.endswith("rand") else 0.1))
        return d, None
    return make


def _render(r, S, N, draws=()):
    def run(dev, host):
        return r.render_rays(dev["rb"], dev["skts"], dev["cyl"], cams=dev.get("cams"), n_samples=S, n_importance=N,
                             draws={k: dev[k] for k in draws} or None)
    return run


RAY_CASES = {       # name: (golden, rays per call, precision, on-chip mode, per-ray poses, frame codes, draws)
    "render_rays_fp32": ("rays_surreal", 64, "fp32", "auto", False, False, ()),
    "render_rays_bf16_records": ("rays_surreal", 64, "bf16", "records", False, False, ()),
    "render_rays_fp16c": ("rays_surreal", 64, "fp16c", "auto", False, False, ()),
    "render_rays_per_ray_poses": ("rays_surreal", 64, "bf16", "auto", True, False, ()),
    "render_rays_frame_codes": ("rays_h36m", 20, "bf16", "auto", False, True, ()),
    "render_rays_train": ("rays_surreal", 64, "bf16", "auto", False, False, ("t_rand", "u_rand", "noise0", "noise1")),
}


@pytest.mark.parametrize("name", list(RAY_CASES))
def test_ray_rendering(env, name):
    golden, n, prec, onchip, per_ray, cams, draws = RAY_CASES[name]
    g = load_golden(golden)
    r = env.caster("main" if golden == "rays_surreal" else golden, golden).renderer
    S, N = int(g["n_samples"]), int(g["n_importance"])
    r.set_precision(prec)
    r.set_onchip(onchip)
    try:
        check(env, name, _ray_inputs(g, n, name, per_ray, cams, draws, S, N), _render(r, S, N, draws))
    finally:
        r.set_onchip("auto")


def test_alternating_streams_on_one_handle(env):
    """The padding records of the record form are zeroed once per (n, stream) (rec_pad_stream): one bf16 input rendered on the
    default stream, on the side stream behind the delay, and on the default stream again gives the same bytes three times; and a
    call of 64 rays after one of 200 on the side stream, whose padding lies where the large call wrote records, is the 64-ray
    call of the default stream."""
    g = load_golden("rays_surreal")
    r = env.caster().renderer
    S, N = int(g["n_samples"]), int(g["n_importance"])
    r.set_precision("bf16")
    r.set_onchip("records")
    default = torch.cuda.default_stream(env.dev)
    try:
        rb, sk, cy = (_t(g[k]).to(DEV) for k in ("ray_batch", "skts", "cyl"))
        call = lambda a: r.render_rays(a, sk, cy, n_samples=S, n_importance=N)
        small_ref = call(rb[:64].contiguous())
        torch.cuda.synchronize()
        first = call(rb[:200].contiguous())
        env.side.wait_stream(default)
        with torch.cuda.stream(env.side):
            env.delay.enqueue()
            second = call(rb[:200].contiguous())
        default.wait_stream(env.side)
        third = call(rb[:200].contiguous())
        torch.cuda.synchronize()
        for k in first:
            assert sh._bytes_equal(first[k], second[k]) and sh._bytes_equal(first[k], third[k]), k
        with torch.cuda.stream(env.side):
            env.delay.enqueue()
            big = call(rb[:200].contiguous())
            small = call(rb[:64].contiguous())
        torch.cuda.synchronize()
        for k in first:
            assert sh._bytes_equal(big[k], first[k]), k
            assert sh._bytes_equal(small[k], small_ref[k]), k
    finally:
        r.set_onchip("auto")


def test_query_density(env):
    r = env.caster().renderer
    r.set_precision("fp32")
    kps = syn.make_pose(3, 9)[1]
    sk = _t(syn.make_pose(3, 9)[2])

    def make(v):
        i = VARIANT[v]
        pts = kps[i][_rng("qd", v).randint(0, 24, 200)] + _rng("qd2", v).randn(200, 3) * 0.1
        return {"pts": _t(pts), "skts": sk[i:i + 1]}, None
    check(env, "query_density", make, lambda dev, host: {"sigma": r.query_density(dev["pts"], dev["skts"])})


def test_grid_density_and_marching_cubes(env):
    r = env.caster().renderer
    r.set_precision("fp32")
    _, kps, skts = syn.make_pose(3, 9)

    def make(v):
        i = VARIANT[v]
        return {"skts": _t(skts[i:i + 1])}, {"kps": kps[i:i + 1], "radius": 1.2 + 0.1 * i}

    def run(dev, host):
        sigma = r.grid_density(host["kps"], dev["skts"], radius=host["radius"], res=15)
        verts, tris = r.marching_cubes(sigma, 0.0, clamp=float("-inf"))
        return {"sigma": sigma, "verts": verts, "tris": tris}
    check(env, "grid_mesh", make, run)


# ---- training ------------------------------------------------------------------------------------------------------------------------

def _train_case(env, name, key, pose=False, coarse_only=False, golden="train_grads", **kw):
    single = key == "single"
    g = load_golden("train_grads_single" if single else golden)
    m = env.trainable_single() if single else env.trainable(key, golden, **kw)
    cfg = m.cfg
    n = g["ray_batch"].shape[0] // 3
    S, N = cfg.n_samples, 0 if coarse_only else cfg.n_importance
    draws = ("t_rand", "noise0") if coarse_only else ("t_rand", "u_rand", "noise0", "noise1")
    base = _ray_inputs(g, n, name, cams="cams" in g, draws=draws, S=S, N=N)
    target = _t(g["target"])

    def make(v):
        d, _ = base(v)
        d["target"] = target[VARIANT[v] * n:(VARIANT[v] + 1) * n]
        return d, None

    def clear():
        for p in m.parameters():
            p.grad = None

    def run(dev, host):
        skts = dev["skts"].detach().requires_grad_() if pose else dev["skts"]
        out = m(dev["rb"], N_samples=S, skts=skts, cyls=dev["cyl"], cams=dev.get("cams"), N_importance=N, draws={k: dev[k] for k in draws})
        loss_of(out, dev["target"]).backward()
        res = {k: out[k].detach() for k in ("rgb_map", "acc_map", "rgb0", "acc0") if k in out}
        for tag, net in (("c", m.network),) if single else (("c", m.network), ("f", m.network_fine)):
            for k, p in net.named_parameters():
                res[f"{tag}.{k}"] = p.grad
        if pose:
            res["d_skts"] = skts.grad
        clear()
        return res
    check(env, name, make, run, between=clear)


def test_train_forward_backward_fp32(env):
    _train_case(env, "train_fp32", "fp32", train_precision="fp32")


def test_train_forward_backward_bf16(env):
    _train_case(env, "train_bf16", "bf16", train_precision="bf16")


def test_train_forward_backward_frame_codes(env):
    """a model with frame codes: their gradient is accumulated into a buffer that a memset in front has zeroed"""
    _train_case(env, "train_frame_codes", "codes", golden="train_grads_h36m", train_precision="fp32")


def test_train_forward_backward_single_net(env):
    """the single-net step: merged_composite_bwd_kernel adds into a d_raw that a memset in front of it has zeroed"""
    _train_case(env, "train_single", "single")


def test_train_forward_backward_single_net_coarse_only(env):
    """N_importance = 0: the one composite's backward ADDS into the zeroed d_raw (with importance samples the merged composite
    writes every row first, and the zeroing changes nothing)"""
    _train_case(env, "train_single_coarse", "single", coarse_only=True)


def test_train_forward_backward_pose(env):
    """forward, backward, forward, backward: a second forward makes the first tape stale by contract"""
    _train_case(env, "train_pose", "pose", pose=True, opt_pose=True)


def test_load_weights_device(env):
    """sync_inference_weights (pg_load_weights_device) after the parameters changed on the stream, and a render after it"""
    m = env.trainable("fp32", train_precision="fp32")
    r = m.renderer
    g = load_golden("train_grads")
    S, N = m.cfg.n_samples, m.cfg.n_importance
    rb, sk, cy = _t(g["ray_batch"])[:32], _t(g["skts"]).reshape(-1, 24, 4, 4)[:1], _t(g["cyl"]).reshape(-1, 5)[:1]
    params = [dict(net.named_parameters())["pts_linears.7.bias"] for net in (m.network, m.network_fine)]
    keep = [p.detach().clone() for p in params]
    sk, cy = sk.to(DEV), cy.to(DEV)
    r.set_precision("bf16")

    def make(v):
        return {"rb": rb, "b0": keep[0].cpu() + _t(_rng("lw", v).randn(256) * 0.05), "b1": keep[1].cpu() + _t(_rng("lw1", v).randn(256) * 0.05)}, None

    def run(dev, host):
        with torch.no_grad():
            params[0].copy_(dev["b0"])
            params[1].copy_(dev["b1"])
        m.sync_inference_weights()
        return r.render_rays(dev["rb"], sk, cy, n_samples=S, n_importance=N)
    try:
        check(env, "load_weights_device", make, run)
    finally:
        with torch.no_grad():
            for p, k in zip(params, keep):
                p.copy_(k)
        m.sync_inference_weights()
        r.set_precision("fp32")


def test_train_loss(env):
    from posegen_amd.train_losses import photometric_loss
    r = env.caster().renderer
    n = 101

    def make(v):
        rng = _rng("tl", v)
        u = lambda *s: _t(rng.uniform(0.02, 0.98, s))
        return {"rgb_map": u(n, 3), "acc_map": u(n), "rgb0": u(n, 3), "acc0": u(n), "target_s": u(n, 3), "bgs": u(n, 3),
                "fgs": _t(rng.randint(0, 2, (n, 1)))}, None

    def run(dev, host):
        preds = {k: dev[k].detach().requires_grad_() for k in ("rgb_map", "acc_map", "rgb0", "acc0")}
        losses, stats = photometric_loss(preds, dev, loss_fn="L1", coarse_weight=0.5, reg_fn="BCE", reg_coef=0.1, renderer=r)
        losses["total_loss"].backward()
        out = {f"d_{k}": p.grad for k, p in preds.items()}
        out.update({k: t.detach() for k, t in losses.items()})
        out.update({k: t.detach() for k, t in stats.items()})
        return out
    check(env, "train_loss", make, run)


def _rotations(rng, *shape):
    """proper rotation matrices [*shape,3,3] (QR of Gaussian matrices, determinant +1)"""
    q, _ = np.linalg.qr(rng.randn(*shape, 3, 3))
    q[..., :, 0] *= np.sign(np.linalg.det(q))[..., None]
    return q


def test_pose_reg_loss(env):
    from posegen_amd.train_losses import pose_regulariser
    r = env.caster().renderer
    n, NA = 40, 8

    def make(v):
        rng = _rng("prl", v)
        d = {"rots": _t(_rotations(rng, n, 24)), "kps": _t(rng.randn(n, 24, 3)), "a_rots": _t(_rotations(rng, NA, 24)),
             "a_kps": _t(rng.randn(NA, 24, 3)), "temp_val": _t(rng.randint(0, 2, n))}
        for k in ("prev", "next"):
            d[f"{k}_rots"], d[f"{k}_kps"] = _t(_rotations(rng, n, 24)), _t(rng.randn(n, 24, 3))
        return d, rng.randint(0, NA, n)

    def run(dev, kp_idx):
        rots, kps = dev["rots"].detach().requires_grad_(), dev["kps"].detach().requires_grad_()
        temporal = {k: dev[k] for k in ("prev_rots", "prev_kps", "next_rots", "next_kps", "temp_val")}
        temporal["temp_coef"] = 0.3
        total, terms = pose_regulariser(rots, kps, kp_idx, {"rots": dev["a_rots"], "kps": dev["a_kps"]}, tol=0.01, coef=2.0, ext_scale=0.001,
                                        temporal=temporal, renderer=r)
        total.backward()
        return {"total": total.detach(), "d_rots": rots.grad, "d_kps": kps.grad, **{k: t.detach() for k, t in terms.items()}}
    check(env, "pose_reg_loss", make, run)


def test_grad_norms(env):
    from posegen_amd.train_losses import grad_norms
    r = env.caster().renderer

    def make(v):
        rng = _rng("gn", v)
        return {"g0": _t(rng.randn(37)), "g1": _t(rng.randn(1000)), "g2": _t(rng.randn(5, 77))}, v

    def run(dev, v):
        table = [dev["g0"], dev["g1"], dev["g2"]] if v != "A2" else [dev["g2"], dev["g1"][3:], dev["g0"][1:], dev["g1"][:3]]
        total, avg, per = grad_norms([types.SimpleNamespace(grad=t) for t in table], r)
        return {"total": total, "avg": avg, "per_tensor": per}
    check(env, "grad_norms", make, run)


# ---- frames --------------------------------------------------------------------------------------------------------------------------

C2W, FOCALS = syn.make_camera(1, H, W)
C2W, FOCAL = C2W[0], float(FOCALS[0])
RIGHT, BACK = C2W[:3, 0], C2W[:3, 2]
CFG = surreal_config()
S_FRAME, N_FRAME = 32, 16


def _people(seed, offsets=None):
    """two synthetic poses in front of the camera -> (bones, kps, skts, cyls tensor [2,5], boxes [(tl, br)])"""
    from posegen_amd.rays import kp_to_boxes
    from posegen_amd.scene import place_people
    bones, kps, skts = syn.make_pose(2, seed)
    if offsets is None:
        offsets = np.stack([-7 * BACK - 1.5 * RIGHT, -7 * BACK + 2.0 * RIGHT]).astype(np.float32)
    kp2, sk2 = place_people(kps, skts, offsets)
    cyls, boxes, _ = kp_to_boxes([torch.tensor(C2W)] * 2, H, W, FOCAL, kps=torch.tensor(kp2), ext_scale=CFG.ext_scale)
    boxes = [((int(b[0][0]), int(b[0][1])), (int(b[1][0]), int(b[1][1]))) for b in boxes]
    for (x0, y0), (x1, y1) in boxes:
        assert 0 <= x0 < x1 <= W and 0 <= y0 < y1 <= H, boxes
    return bones, kp2, sk2, cyls, boxes


def _frame_renderer(env):
    r = env.caster().renderer
    r.set_precision("bf16")
    return r


def _bg(v):
    return _t(_rng("bg", v).uniform(0, 1, (H * W, 3)))


def test_kinematics_boxes_frame(env):
    """pg_pose_kinematics -> pg_pose_boxes -> pg_render_frame: the frame renders the pose and the cylinder that the two calls
    before it left on the device; its box is a host argument (that of the same pose, computed on the host)."""
    from posegen_amd.rays import kp_to_boxes
    from posegen_amd.skeleton import smpl_rest_pose
    from posegen_amd.synthetic import SURREAL_REST_SCALE
    r = _frame_renderer(env)
    rest = smpl_rest_pose * SURREAL_REST_SCALE

    def make(v):
        bones, kps, _ = syn.make_pose(2, 20 + VARIANT[v])
        _, boxes, _ = kp_to_boxes([torch.tensor(C2W)] * 2, H, W, FOCAL, kps=torch.tensor(kps), ext_scale=CFG.ext_scale)
        (x0, y0), (x1, y1) = boxes[0]
        box = ((max(int(x0), 0), max(int(y0), 0)), (min(int(x1), W), min(int(y1), H)))
        return {"bones": _t(bones, torch.float64), "bg": _bg(v)}, box

    def run(dev, box):
        kps, skts = r.pose_kinematics(dev["bones"], rest)
        cyls, boxes = r.pose_boxes(kps, C2W, H, W, FOCAL, CFG.ext_scale)
        rgb, disp, acc = r.render_frame(H, W, FOCAL, C2W, box, skts[:1], cyls[:1], n_samples=S_FRAME, n_importance=N_FRAME, bg=dev["bg"])
        return {"kps": kps, "skts": skts, "cyls": cyls, "boxes": boxes, "rgb": rgb, "disp": disp, "acc": acc}
    check(env, "kinematics_boxes_frame", make, run)


def test_frame_ranges_and_compose(env):
    r = _frame_renderer(env)
    keep = r._chunk
    r.set_chunk(64)

    def make(v):
        _, _, sk, cyls, boxes = _people(30 + VARIANT[v])
        p = VARIANT[v] % 2
        return {"skts": _t(sk[p:p + 1]), "cyl": cyls[p:p + 1].float(), "bg": _bg(v)}, (boxes[p], 64 * (1 + VARIANT[v] % 2))

    def run(dev, host):
        box, cut = host
        n = (box[1][0] - box[0][0]) * (box[1][1] - box[0][1])
        assert cut < n
        parts = [r.render_frame_range(H, W, FOCAL, C2W, box, dev["skts"], dev["cyl"], a, b, n_samples=S_FRAME, n_importance=N_FRAME)
                 for a, b in ((0, cut), (cut, n))]
        sh.stage_done(("pg_render_frame_range",))
        rgb_map = torch.cat([p[:3 * m].view(m, 3) for p, m in zip(parts, (cut, n - cut))])
        disp_map = torch.cat([p[3 * m:4 * m] for p, m in zip(parts, (cut, n - cut))])
        acc_map = torch.cat([p[4 * m:] for p, m in zip(parts, (cut, n - cut))])
        rgb, disp, acc, rgb8 = r.compose_frame(H, W, box, rgb_map, disp_map, acc_map, bg=dev["bg"], want_uint8=True)
        return {"rgb_map": rgb_map, "rgb": rgb, "disp": disp, "acc": acc, "rgb8": rgb8}
    try:
        check(env, "frame_ranges_compose", make, run)
    finally:
        r.set_chunk(keep)


def test_stage_frame_rays(env):
    """every argument of pg_stage_frame_rays is a host argument: no decoy, but two calls with different cameras, boxes and ranges"""
    r = _frame_renderer(env)

    def make(v):
        i = VARIANT[v]
        c2w = C2W.copy()
        c2w[:3, 3] += 0.1 * i
        return {}, (c2w, ((10 + i, 5), (31, 29 + i)), 7 * i, 200 + 11 * i, float(i))

    def run(dev, host):
        c2w, box, r0, r1, cam = host
        rays, cams = r.stage_frame_rays(H, W, FOCAL, c2w, box, r0, r1, cam=cam, want_cams=True)
        return {"rays": rays, "cams": cams}
    check(env, "stage_frame_rays", make, run)


def test_render_scene(env):
    from posegen_amd.scene import ScenePerson
    r = _frame_renderer(env)
    near = np.stack([-6 * BACK + 0.25 * RIGHT, -6.6 * BACK - 0.25 * RIGHT]).astype(np.float32)      # the two boxes overlap

    def make(v):
        _, _, sk, cyls, boxes = _people(40 + VARIANT[v], near)
        return {"sk0": _t(sk[0]), "sk1": _t(sk[1]), "cy0": cyls[0].float(), "cy1": cyls[1].float(), "bg": _bg(v)}, boxes

    def run(dev, boxes):
        people = [ScenePerson(dev["sk0"], dev["cy0"], boxes[0]), ScenePerson(dev["sk1"], dev["cy1"], boxes[1])]
        rgb, disp, acc, rgb8, pacc = r.render_scene(H, W, FOCAL, C2W, people, n_samples=S_FRAME, n_importance=N_FRAME, bg=dev["bg"],
                                                    want_uint8=True, want_person_acc=True)
        return {"rgb": rgb, "disp": disp, "acc": acc, "rgb8": rgb8, "person_acc": pacc}
    check(env, "render_scene", make, run)


def test_stage_scene_composite(env):
    from posegen_amd.scene import stage_scene_composite
    r = env.caster().renderer
    P, S, n_pix, rows_p = 2, 8, 100, (60, 70)

    def make(v):
        rng = _rng("ssc", v)
        d = {"dirs": _t(rng.randn(n_pix, 3)), "rows": _t(np.stack([rng.randint(-10, m, n_pix) for m in rows_p]), torch.int32)}
        for p, m in enumerate(rows_p):
            d[f"z{p}"] = _t(np.sort(rng.uniform(2, 6, (m, S)), axis=1))
            d[f"raw{p}"] = _t(rng.randn(m, S, 4))
        return d, None

    def run(dev, host):
        return stage_scene_composite(r, [dev["z0"], dev["z1"]], [dev["raw0"], dev["raw1"]], dev["rows"], dev["dirs"])
    check(env, "stage_scene_composite", make, run)


# ---- batches and scoring -------------------------------------------------------------------------------------------------------------

def test_batch_chain(env):
    """pg_pixel_index_count -> pg_pixel_index_emit -> pg_batch_sample_pixels -> pg_batch_gather through ctypes (the wrapper's bank
    reads the counts back when it is built).  All three variants' sampling masks have the same number of valid pixels per image
    (each is a permutation of one mask), so the host arguments derived from the masks hold for whichever mask a kernel reads."""
    r = env.caster().renderer
    lib, h = r.lib, r.handle
    F, bh, bw, k, n_img = 4, 12, 16, 5, 3
    P = bh * bw
    base = (np.random.RandomState(5).uniform(0, 1, (F, P)) < 0.4).astype(np.uint8)
    base[:, :k] = 1
    counts = base.sum(1).astype(np.int64)
    total = int(counts.sum())
    cam = torch.as_tensor(np.stack([C2W[:3, :4]] * F)).contiguous().to(DEV)
    foc = torch.full((F, 2), FOCAL, device=DEV)

    def make(v):
        rng = _rng("bc", v)
        sm = np.stack([row[rng.permutation(P)] for row in base]) * (1 + VARIANT[v])
        d = {"sampling_masks": _t(sm, torch.uint8), "imgs": _t(rng.randint(0, 256, (F, P, 3)), torch.uint8),
             "masks": _t(rng.randint(0, 2, (F, P)), torch.uint8), "draws": _t(rng.uniform(0, 1, (n_img, k)), torch.float64)}
        rows = np.ascontiguousarray(rng.permutation(F)[:n_img], dtype=np.int32)
        return d, (rows, np.ascontiguousarray(rows[::-1]))

    def run(dev, host):
        img_rows, cam_rows = host
        st = r._stream()
        i32p = lambda a: a.ctypes.data_as(C.POINTER(C.c_int32))
        cnt = _sentinel(F, dtype=torch.int64)
        r._check(lib.pg_pixel_index_count(h, st, _ptr(dev["sampling_masks"]), F, P, _ptr(cnt)))
        start = torch.zeros(F + 1, dtype=torch.int64, device=DEV)
        torch.cumsum(cnt, 0, out=start[1:])
        ids = _sentinel(total, dtype=torch.int32)
        r._check(lib.pg_pixel_index_emit(h, st, _ptr(dev["sampling_masks"]), F, P, _ptr(start), total, _ptr(ids)))
        pix = _sentinel(n_img * k, dtype=torch.int32)
        r._check(lib.pg_batch_sample_pixels(h, st, _ptr(ids), _ptr(start), counts.ctypes.data_as(C.POINTER(C.c_int64)), F, i32p(img_rows),
                                            n_img, k, _ptr(dev["draws"]), _ptr(pix)))
        bank = _ffi.PgImageBank(imgs=dev["imgs"].data_ptr(), masks=dev["masks"].data_ptr(), bkgds=None, bkgd_idxs=None, c2ws=cam.data_ptr(),
                                focals=foc.data_ptr(), centers=None, F=F, P=P, n_bkgd=0, n_cam=F, H=bh, W=bw, mask_img=0)
        n = n_img * k
        out = {"counts": cnt, "ids": ids, "pix": pix, "target_s": _sentinel(n, 3), "fgs": _sentinel(n, 1), "rays_o": _sentinel(n, 3),
               "rays_d": _sentinel(n, 3), "ray_batch": _sentinel(n, 11)}
        r._check(lib.pg_batch_gather(h, st, C.byref(bank), i32p(img_rows), i32p(cam_rows), n_img, k, _ptr(pix), _ptr(out["target_s"]),
                                     _ptr(out["fgs"]), None, _ptr(out["rays_o"]), _ptr(out["rays_d"]), _ptr(out["ray_batch"])))
        return out
    check(env, "batch_chain", make, run, warm=8)


def test_regressor_input(env):
    from posegen_amd.regressor_batches import PixelStore, regressor_input
    r = env.caster().renderer
    n_items = 11

    def make(v):
        rng = _rng("ri", v)
        x0, y0 = rng.randint(0, 10, n_items), rng.randint(0, 10, n_items)
        boxes = np.stack([x0, y0, x0 + rng.randint(3, 26, n_items), y0 + rng.randint(3, 30, n_items)], 1).astype(np.int32)
        return {"pix": _t(rng.randint(0, 256, (4, 40, 36, 3)), torch.uint8)}, (rng.randint(0, 4, n_items), boxes)

    def run(dev, host):
        return {"out": regressor_input(PixelStore(r, dev["pix"]), host[0], host[1], out_res=16)}
    check(env, "regressor_input", make, run, warm=8)


def _metrics_bank(env):
    def build():
        from posegen_amd.batches import DeviceImageBank
        g = load_golden("frame_metrics")
        F, bh, bw = g["imgs_a"].shape[:3]
        c2ws, foc = syn.make_camera(F, bh, bw)
        return DeviceImageBank(env.caster().renderer, g["imgs_a"].reshape(F, -1, 3), g["masks_a"].reshape(F, -1, 1), g["masks_a"].reshape(F, -1),
                               c2ws, foc, (bh, bw), bkgds=g["bkgds_a"].reshape(1, -1, 3), bkgd_idxs=np.zeros(F, dtype=np.int32))
    return env.get("metrics_bank", build)


def test_frame_metrics(env):
    from posegen_amd.evaluate import FrameScorer
    bank = _metrics_bank(env)
    bh, bw = bank.HW

    def make(v):
        i = VARIANT[v]
        return {"rgb": _t(_rng("fm", v).uniform(0, 1, (bh, bw, 3)))}, (i % 2, (3 + i, 2, 40 - i, 30 + i))

    def run(dev, host):
        sc = FrameScorer(bank, capacity=1)
        sc.score(0, dev["rgb"], host[0], host[1])
        return {"sums": sc._sums}
    check(env, "frame_metrics", make, run)


def test_frame_metrics_val(env):
    from posegen_amd.evaluate import ValidationScorer
    bank = _metrics_bank(env)
    bh, bw = bank.HW

    def make(v):
        i = VARIANT[v]
        return {"rgb": _t(_rng("fmv", v).uniform(0, 1, (bh // 2, bw // 2, 3)))}, (i % 2, (5, 4 + i, 30 + i, 33), (1 + i, 0, 45, 36 - i))

    def run(dev, host):
        sc = ValidationScorer(bank, capacity=1)
        sc.score(0, dev["rgb"], host[0], valid_box=host[1], box=host[2])
        return {"sums": sc._sums}
    check(env, "frame_metrics_val", make, run)


def _kps(name, v, B=8):
    rng = _rng(name, v)
    gt = rng.randn(B, 24, 3)
    return {"pred": _t(gt + 0.1 * rng.randn(B, 24, 3)), "gt": _t(gt)}


def test_pose_scores(env):
    from posegen_amd.pose_eval import PoseScorer
    scorer = PoseScorer(env.caster().renderer)

    def make(v):
        i = VARIANT[v]
        return _kps("ps", v), (list(range(i, 24, 1 + i)), i, (0.05 * (1 + i), 0.1, 0.2 + 0.1 * i))

    def run(dev, host):
        return scorer.enqueue(dev["pred"], dev["gt"], joints=host[0], root=host[1], align="rotation", thresholds=host[2], ret_per_pose=True,
                              ret_aligned=True, ret_joint_err=True)
    check(env, "pose_scores", make, run)


def test_pose_loss(env):
    from posegen_amd.pose_losses import pose_loss
    r = env.caster().renderer

    def make(v):
        i = VARIANT[v]
        return _kps("pl", v), (list(range(1 + i, 24, 2)), i)

    def run(dev, host):
        pred = dev["pred"].detach().requires_grad_()
        loss, per_pose, kept = pose_loss(pred, dev["gt"], joints=host[0], root=host[1], kind="norm_matched", weight=2.0, cap=0.9, renderer=r,
                                         return_stats=True)
        loss.backward()
        return {"loss": loss.detach(), "per_pose": per_pose, "kept": kept, "d_pred": pred.grad}
    check(env, "pose_loss", make, run)


# ---- the composite-backward stage entry points: they launch their kernels themselves (pg_train.hip) ------------------------------

def _composite_inputs(name, n=40, S=16, N=8):
    def make(v):
        rng = _rng(name, v)
        rays = rng.randn(n, 11)
        zc, zn = np.sort(rng.uniform(2, 6, (n, S)), axis=1), rng.uniform(2, 6, (n, N))
        cat = np.concatenate([zc, zn], axis=1)
        order = np.argsort(cat, axis=1, kind="stable")
        return {"rays": _t(rays), "z": _t(zc), "z_fine": _t(np.take_along_axis(cat, order, 1)), "order": _t(order, torch.int32),
                "raw": _t(rng.randn(n * (S + N), 4)), "noise0": _t(0.1 * rng.rand(n, S)), "noise1": _t(0.1 * rng.rand(n, S + N)),
                "d_rgb": _t(rng.randn(n, 3)), "d_acc": _t(rng.randn(n)), "d_rgb0": _t(rng.randn(n, 3)), "d_acc0": _t(rng.randn(n))}, None
    return make, n, S, N


def test_stage_composite_bwd(env):
    """pg_stage_composite_bwd through ctypes, d_raw the case's own tensor with a sentinel written on the stream in front of the call"""
    r = env.caster().renderer
    make, n, S, N = _composite_inputs("scb")

    def run(dev, host):
        d_raw = _sentinel(n, S, 4)
        r._check(r.lib.pg_stage_composite_bwd(r.handle, r._stream(), n, S, _ptr(dev["rays"]), _ptr(dev["z"]), _ptr(dev["raw"]), _ptr(dev["noise0"]),
                                              _ptr(dev["d_rgb0"]), _ptr(dev["d_acc0"]), _ptr(d_raw)))
        return {"d_raw": d_raw}
    check(env, "stage_composite_bwd", make, run)


def test_stage_merged_composite_bwd(env):
    """pg_stage_merged_composite_bwd through ctypes: once with all four cotangents, once with the coarse maps' alone -- then the
    new points' rows keep the zeros of the call's own memset and the coarse rows are ADDED to them, so a memset that is not
    ordered behind the sentinel (written on the stream in front of the call) shows in every row."""
    r = env.caster().renderer
    make, n, S, N = _composite_inputs("smcb")

    def run(dev, host):
        out = {}
        for tag, fine in (("all", True), ("coarse_only", False)):
            d_raw = _sentinel(n * (S + N), 4)
            r._check(r.lib.pg_stage_merged_composite_bwd(
                r.handle, r._stream(), n, S, N, _ptr(dev["rays"]), _ptr(dev["z"]), _ptr(dev["z_fine"]), _ptr(dev["raw"]), _ptr(dev["noise0"]),
                _ptr(dev["noise1"]), _ptr(dev["order"]), _ptr(dev["d_rgb"]) if fine else None, _ptr(dev["d_acc"]) if fine else None,
                _ptr(dev["d_rgb0"]), _ptr(dev["d_acc0"]), _ptr(d_raw)))
            out[tag] = d_raw
        return out
    check(env, "stage_merged_composite_bwd", make, run)


# ---- pose and body -------------------------------------------------------------------------------------------------------------------

def _body(env):
    from posegen_amd.smpl import BodyModel
    return env.get("body", lambda: BodyModel.from_arrays(env.caster().renderer, syn.make_body_model(431, NB=10, seed=3, regress_rows=(17,))))


def test_vertex_errors(env):
    from posegen_amd.smpl import vertex_errors
    r = env.caster().renderer

    def make(v):
        rng = _rng("ve", v)
        return {"a": _t(rng.randn(3, 431, 3)), "b": _t(rng.randn(3, 431, 3))}, None

    def run(dev, host):
        per_pose, mean = vertex_errors(r, dev["a"], dev["b"])
        return {"per_pose": per_pose, "mean": mean}
    check(env, "vertex_errors", make, run)


def test_smpl_forward_backward(env):
    body = _body(env)

    def make(v):
        rng = _rng("smpl", v)
        return {"betas": _t(rng.randn(5, 10)), "pose": _t(rng.randn(5, 24, 3) * 0.3), "cv": _t(rng.randn(5, 431, 3)), "cj": _t(rng.randn(5, 24, 3)),
                "cr": _t(rng.randn(5, 17, 3))}, None

    def run(dev, host):
        betas, pose = dev["betas"].detach().requires_grad_(), dev["pose"].detach().requires_grad_()
        out = body.differentiable(betas, pose, regressor="17", want_vertices=True)
        ((out.vertices * dev["cv"]).sum() + (out.joints * dev["cj"]).sum() + (out.regressed * dev["cr"]).sum()).backward()
        return {"verts": out.vertices.detach(), "joints": out.joints.detach(), "regressed": out.regressed.detach(), "d_betas": betas.grad,
                "d_pose": pose.grad}
    check(env, "smpl", make, run)


def test_poseopt_forward_backward(env):
    """HipPoseOptLayer with a rest pose per pose: the layer's parameters are device tensors, so the real values are copied into them
    on the stream; the ray -> pose indices (host) differ between the two calls.  The layer uploads its index tensors itself."""
    from posegen_amd.poseopt import HipPoseOptLayer
    g = load_golden("poseopt")
    r = env.caster().renderer
    sd = {"pelvis": _t(g["pelvis_pp"]), "bones": _t(g["bones_param_pp"]), "rest_pose": _t(g["rest_pose_pp"])}
    layer = HipPoseOptLayer.from_state_dict(sd, renderer=r, rest_pose_idxs=g["rest_pose_idxs_pp"])
    U = g["pelvis_pp"].shape[0]

    def make(v):
        rng = _rng("po", v)
        idxs = np.concatenate([np.arange(U), rng.randint(0, U, 3)])[rng.permutation(U + 3)]      # 8 rays, every pose at least once
        d = {"pelvis": _t(g["pelvis_pp"] + 0.05 * rng.randn(U, 3)), "bones": _t(g["bones_param_pp"] + 0.05 * rng.randn(U, 24, 6))}
        for k in ("d_kps", "d_skts", "d_l2ws", "d_rots"):
            d[k] = _t(rng.randn(*g[k].shape))
        return d, idxs

    def clear():
        layer.pelvis.grad = layer.bones.grad = None

    def run(dev, idxs):
        with torch.no_grad():
            layer.pelvis.copy_(dev["pelvis"])
            layer.bones.copy_(dev["bones"])
        kps, bones, skts, l2ws, rots = layer(idxs)
        ((kps * dev["d_kps"]).sum() + (skts * dev["d_skts"]).sum() + (l2ws * dev["d_l2ws"]).sum() + (rots * dev["d_rots"]).sum()).backward()
        res = {"kps": kps.detach(), "bones": bones.detach(), "skts": skts.detach(), "l2ws": l2ws.detach(), "rots": rots.detach(),
               "d_pelvis": layer.pelvis.grad, "d_bones": layer.bones.grad}
        clear()
        return res
    check(env, "poseopt", make, run, between=clear)


def _rest():
    from posegen_amd.skeleton import smpl_rest_pose
    return smpl_rest_pose.astype(np.float32)


def test_pose_kinematics_rot(env):
    r = env.caster().renderer

    def make(v):
        return {"rotmats": _t(_rotations(_rng("kr", v), 4, 24))}, 0.4 + 0.1 * VARIANT[v]

    def run(dev, scale):
        kps, skts, l2ws = r.pose_kinematics_rot(dev["rotmats"], _rest(), scale=scale, want_l2ws=True)
        return {"kps": kps, "skts": skts, "l2ws": l2ws}
    check(env, "kinematics_rot", make, run)


def test_pose_kinematics_bwd(env):
    from posegen_amd.pose_losses import keypoints_from_axis_angle
    r = env.caster().renderer

    def make(v):
        rng = _rng("kb", v)
        return {"bones": _t(syn.make_bones(4, 50 + VARIANT[v]), torch.float64), "c": _t(rng.randn(4, 24, 3))}, 1.0 + 0.1 * VARIANT[v]

    def run(dev, scale):
        bones = dev["bones"].detach().requires_grad_()
        kps = keypoints_from_axis_angle(r, bones, _rest(), scale=scale)
        (kps * dev["c"]).sum().backward()
        return {"kps": kps.detach(), "d_bones": bones.grad}
    check(env, "kinematics_bwd", make, run)


def test_pose_kinematics_rot_bwd(env):
    from posegen_amd.pose_losses import keypoints_from_rotmats
    r = env.caster().renderer

    def make(v):
        rng = _rng("krb", v)
        return {"rotmats": _t(_rotations(rng, 4, 24)), "c": _t(rng.randn(4, 24, 3))}, 0.4 + 0.1 * VARIANT[v]

    def run(dev, scale):
        m = dev["rotmats"].detach().requires_grad_()
        kps = keypoints_from_rotmats(r, m, scale=scale)
        (kps * dev["c"]).sum().backward()
        return {"kps": kps.detach(), "d_rotmats": m.grad}
    check(env, "kinematics_rot_bwd", make, run)
