"""The modules' state over a handle's life (csrc/pg_modules.h): created by the first call that needs it, freed by pg_destroy, one
per handle.  One module per kind of ownership -- plain buffers (pg_pose_scores, pg_train_loss), an upload ring with events
(pg_regressor_input), a stream, events and pinned staging (pg_render_frames), two buffers and a validity flag (pg_train_forward /
pg_train_backward_pose), state that a later call reads (pg_mesh_count, then pg_mesh_emit) -- each with its smallest inputs of
tests/test_gpu_streams.py.  No kernel is under test: the results of a fresh handle are compared bitwise with those of a handle that
has been destroyed, and with those of the same handle after another one has come and gone."""
import numpy as np
import pytest
import torch

from posegen_amd import _ffi, synthetic as syn
from tests.helpers import cfg_from_golden, load_golden, loss_of, model_for

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
H, W = 48, 64
S_FRAME, N_FRAME = 32, 16


def _t(a, dtype=torch.float32):
    return torch.as_tensor(np.ascontiguousarray(a)).to(dtype).to(DEV)


@pytest.fixture(scope="module")
def inputs():
    """every call's inputs, made once and left unchanged"""
    from posegen_amd.rays import kp_to_boxes
    g = load_golden("train_grads")
    rng = np.random.RandomState(7)
    n = g["ray_batch"].shape[0] // 3
    d = {"golden": g, "n": n}
    gt = rng.randn(8, 24, 3)
    d["pose"] = {"pred": _t(gt + 0.1 * rng.randn(8, 24, 3)), "gt": _t(gt)}
    u = lambda *s: _t(rng.uniform(0.02, 0.98, s))
    d["loss"] = {"rgb_map": u(101, 3), "acc_map": u(101), "rgb0": u(101, 3), "acc0": u(101), "target_s": u(101, 3), "bgs": u(101, 3),
                 "fgs": _t(rng.randint(0, 2, (101, 1)))}
    x0, y0 = rng.randint(0, 10, 11), rng.randint(0, 10, 11)
    d["crops"] = (_t(rng.randint(0, 256, (4, 40, 36, 3)), torch.uint8), rng.randint(0, 4, 11),
                  np.stack([x0, y0, x0 + rng.randint(3, 26, 11), y0 + rng.randint(3, 30, 11)], 1).astype(np.int32))
    c2ws, focals = syn.make_camera(1, H, W)
    _, kps, skts = syn.make_pose(2, 20)
    cfg = cfg_from_golden(g)
    cyls, boxes, _ = kp_to_boxes([torch.tensor(c2ws[0])] * 2, H, W, float(focals[0]), kps=torch.tensor(kps), ext_scale=cfg.ext_scale)
    boxes = [((max(int(b[0][0]), 0), max(int(b[0][1]), 0)), (min(int(b[1][0]), W), min(int(b[1][1]), H))) for b in boxes]
    d["frames"] = (float(focals[0]), [c2ws[0]] * 2, boxes, skts, cyls)
    S, N = cfg.n_samples, cfg.n_importance
    d["train"] = {"rb": _t(g["ray_batch"])[:n], "skts": _t(g["skts"]).reshape(-1, 24, 4, 4)[:1], "cyl": _t(g["cyl"]).reshape(-1, 5)[:1],
                  "target": _t(g["target"])[:n], "t_rand": u(n, S), "u_rand": u(n, N), "noise0": 0.1 * u(n, S), "noise1": 0.1 * u(n, S + N)}
    d["grid"] = _t(rng.randn(9, 7, 6))
    return d


def _handle(g):
    """a fresh handle with the model of the fixture loaded, and its trainable wrapper"""
    from posegen_amd.raycaster import HipRayCaster
    from posegen_amd.train import TrainableRayCaster
    cfg = cfg_from_golden(g)
    wc, wf, tv, td = model_for(cfg, int(g["seed_model"]))
    caster = HipRayCaster.from_weights(cfg, wc, wf, float(g["tau_v"]), float(g["tau_d"]), device=DEV, precision="fp32")
    m = TrainableRayCaster(caster, train_precision="fp32", opt_pose=True)
    m.train()
    return caster.renderer, m


def _pose_scores(r, d):
    from posegen_amd.pose_eval import PoseScorer
    out = PoseScorer(r).enqueue(d["pose"]["pred"], d["pose"]["gt"], joints=list(range(1, 24, 2)), root=1, align="rotation",
                                thresholds=(0.05, 0.1, 0.3), ret_per_pose=True, ret_aligned=True, ret_joint_err=True)
    return {f"scores.{k}": v for k, v in out.items()}


def _train_loss(r, d):
    from posegen_amd.train_losses import photometric_loss
    preds = {k: d["loss"][k].detach().requires_grad_() for k in ("rgb_map", "acc_map", "rgb0", "acc0")}
    losses, stats = photometric_loss(preds, d["loss"], loss_fn="L1", coarse_weight=0.5, reg_fn="BCE", reg_coef=0.1, renderer=r)
    losses["total_loss"].backward()
    out = {f"loss.d_{k}": p.grad for k, p in preds.items()}
    out.update({f"loss.{k}": t.detach() for k, t in {**losses, **stats}.items()})
    return out


def _per_handle(r, d):
    """the two calls with plain buffers"""
    out = {**_pose_scores(r, d), **_train_loss(r, d)}
    torch.cuda.synchronize()
    return out


def _the_set(r, m, d):
    from posegen_amd.regressor_batches import PixelStore, regressor_input
    out = _per_handle(r, d)
    pix, rows, boxes = d["crops"]
    out["regressor"] = regressor_input(PixelStore(r, pix), rows, boxes, out_res=16)
    focal, c2ws, fboxes, skts, cyls = d["frames"]
    r.set_precision("bf16")
    for k, a in zip(("rgbs", "disps", "accs"), r.render_frames(H, W, [focal] * 2, c2ws, fboxes, skts, cyls, n_samples=S_FRAME, n_importance=N_FRAME)):
        out[f"frames.{k}"] = torch.from_numpy(a.copy())
    r.set_precision("fp32")
    t = d["train"]
    skts_t = t["skts"].detach().requires_grad_()
    draws = {k: t[k] for k in ("t_rand", "u_rand", "noise0", "noise1")}
    res = m(t["rb"], N_samples=m.cfg.n_samples, skts=skts_t, cyls=t["cyl"], N_importance=m.cfg.n_importance, draws=draws)
    loss_of(res, t["target"]).backward()
    out.update({f"train.{k}": res[k].detach() for k in ("rgb_map", "acc_map", "rgb0", "acc0")})
    for tag, net in (("c", m.network), ("f", m.network_fine)):
        out.update({f"train.{tag}.{k}": p.grad for k, p in net.named_parameters()})
    out["train.d_skts"] = skts_t.grad
    verts, tris = r.marching_cubes(d["grid"], 0.0, clamp=float("-inf"))
    assert verts.shape[0] > 0 and tris.shape[0] > 0
    out["mesh.verts"], out["mesh.tris"] = verts, tris
    torch.cuda.synchronize()
    return out


def _assert_same_bytes(a, b, what):
    assert a.keys() == b.keys()
    for k in a:
        x, y = a[k].detach().cpu().contiguous(), b[k].detach().cpu().contiguous()
        assert x.shape == y.shape and x.dtype == y.dtype, (what, k)
        assert x.numpy().tobytes() == y.numpy().tobytes(), f"{what}: {k} differs"


def test_module_state_is_per_handle_and_goes_with_it(inputs):
    d = inputs
    ra, ma = _handle(d["golden"])
    first = _the_set(ra, ma, d)
    ra.close()
    assert ra.handle is None
    ra.close()                                      # the second close does nothing
    assert ra.handle is None

    rb, mb = _handle(d["golden"])
    try:
        _assert_same_bytes(first, _the_set(rb, mb, d), "a fresh handle after a destroyed one")
        # another handle comes, creates state of its own and goes: nothing of it is B's
        rc, _ = _handle(d["golden"])
        try:
            _assert_same_bytes({k: v for k, v in first.items() if k.startswith(("scores.", "loss."))}, _per_handle(rc, d), "a third handle")
        finally:
            rc.close()
        again = _per_handle(rb, d)
        _assert_same_bytes({k: first[k] for k in again}, again, "handle B after handle C was destroyed")
    finally:
        rb.close()


def test_mesh_emit_without_a_count_on_a_fresh_handle(inputs):
    """pg_mesh_emit only reads the mesh state: on a handle that has none it fails as it always has, and creates none"""
    r, _ = _handle(inputs["golden"])
    try:
        g = inputs["grid"]
        with pytest.raises(_ffi.PgError, match="pg_mesh_emit: no pg_mesh_count of this grid shape, threshold and clamp precedes the call") as e:
            r._check(r.lib.pg_mesh_emit(r.handle, r._stream(), _ffi.ptr(g), *g.shape, 0.0, 0.0, None, None, 0, 0))
        assert e.value.code == _ffi.PG_ESTATE
    finally:
        r.close()
