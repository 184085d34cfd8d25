"""The trainer's losses, pose regulariser and gradient norms on the device (csrc/pg_trainloss.hip through posegen_amd/train_losses.py
and posegen_amd/trainer.py) against the float64 restatement (tests/train_loss_ref.py) on the same float32 inputs.

Bounds.  A summary value is a float64 sum of fewer than 3 10^5 terms, each rounded at 2^-53, in another order than the restatement's:
1e-10 relative.  A gradient is the float64 value rounded once to float32: within one float32 ulp of the restatement's float64
gradient.  Planted values are exact.  End to end, the maps of the two steps are identical, so the loss gradients that enter the
caster's backward differ by at most one float32 ulp (2^-23 relative per element); the backward is linear in them and sums at most
64 x 48 samples per parameter entry, so a parameter or pose gradient may move by 2^-23 of the sum of its terms' magnitudes, which
cancellation makes up to ~100 times the entry's own scale: 1e-5 of the tensor's scale max(largest entry, norm / sqrt(size)), the
scale of the fp32 rule of test_gpu_poseopt.py.  Stats within 1e-6."""
import ctypes as C
from types import SimpleNamespace

import numpy as np
import pytest
import torch

from tests import train_loss_ref as ref
from tests.helpers import cfg_from_golden, load_golden, model_for

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
PHOTO = ["mse_scalar", "l1_bgs_bce_coarse", "huber_nobg_coarse", "huber_bgs_bce", "mse_nobg_bce_coarse", "l1_scalar_coarse",
         "planted_l1_zero", "planted_huber_knee", "planted_bce"]
KP = ["kp_tol0", "kp_tol001_temp", "kp_planted"]
SIZES = [1, 63, 64, 65, 257, 4097]


@pytest.fixture(scope="module")
def renderer():
    from posegen_amd import surreal_config
    from posegen_amd.raycaster import HipRenderer
    r = HipRenderer(surreal_config(), device=DEV)
    yield r
    r.close()


@pytest.fixture(scope="module")
def golden():
    return load_golden("train_losses")


def dev(a, grad=False):
    return None if a is None else torch.tensor(np.asarray(a), device=DEV).requires_grad_(grad)


def close(got, want, what):
    got, want = float(got.detach() if torch.is_tensor(got) else got), float(want)
    if np.isnan(want):
        assert np.isnan(got), f"{what}: {got}, NaN expected"
        return
    err = abs(got - want)
    print(f"{what}: {got!r} against {want!r}, relative error {err / max(abs(want), 1e-300):.2e}")
    assert err <= 1e-10 * abs(want), what


def within_one_ulp(got, want64, what):
    got = got.detach().cpu().numpy()
    assert got.dtype == np.float32 and got.shape == want64.shape, what
    err = np.abs(got.astype(np.float64) - want64) / ref.ulp32(want64)
    print(f"{what}: largest error {err.max():.3f} float32 ulp")
    assert (err <= 1.0).all(), what


def run_photo(renderer, inputs, settings, upstream=None):
    """photometric_loss on the device: (loss_dict, stats, the four maps' gradients or None)"""
    from posegen_amd.train_losses import photometric_loss
    rgb, acc, rgb0, acc0, target, bgs, fgs = inputs
    preds = {"rgb_map": dev(rgb, True), "acc_map": dev(acc, True)}
    if rgb0 is not None:
        preds.update(rgb0=dev(rgb0, True), acc0=dev(acc0, True))
    batch = {"target_s": dev(target), "fgs": dev(fgs)[:, None]}
    if bgs is not None:
        batch["bgs"] = dev(bgs)
    loss_dict, stats = photometric_loss(preds, batch, renderer=renderer, **settings)
    (loss_dict["total_loss"] if upstream is None else loss_dict["total_loss"] * upstream).backward()
    return loss_dict, stats, {"d_" + k: v.grad for k, v in preds.items()}


def check_photo(renderer, inputs, settings, what):
    vals, grads = ref.photometric(*inputs, **settings)
    loss_dict, stats, got = run_photo(renderer, inputs, settings)
    for k, v in {**loss_dict, **stats}.items():
        assert v.dtype == torch.float64 and v.dim() == 0 and v.is_cuda
        close(v, vals[k], f"[{what}] {k}")
    assert set(loss_dict) | set(stats) == {k for k in vals if not k.startswith("n_bce")}
    assert loss_dict["total_loss"].requires_grad and not any(v.requires_grad for k, v in loss_dict.items() if k != "total_loss")
    for k, g in got.items():
        if g is None:                                        # no path: acc without a background and without a regulariser
            assert not grads[k].any(), k
        else:
            within_one_ulp(g, grads[k], f"[{what}] {k}")
    return vals, grads, got


def random_photo(n, seed, coarse=True):
    rng = np.random.RandomState(seed)
    f = lambda *s: rng.uniform(0, 1, s).astype(np.float32)
    fgs = np.where(rng.uniform(size=n) < 0.4, 1.0, rng.uniform(0, 0.9, n)).astype(np.float32)
    fgs[0] = 0.5                                             # (the BCE set is never empty)
    return (f(n, 3), f(n), f(n, 3) if coarse else None, f(n) if coarse else None, f(n, 3), f(n, 3), fgs)


SHIPPED = dict(loss_fn="L1", loss_beta=0.1, use_background=True, coarse_weight=0.5, reg_fn="BCE", reg_coef=0.1)


# ---- the photometric loss ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", PHOTO)
def test_photometric_golden_cases(renderer, golden, name):
    c = ref.golden_case(golden, name)
    check_photo(renderer, ref.photo_inputs(c), ref.photo_settings(c), name)


@pytest.mark.parametrize("n", SIZES)
@pytest.mark.parametrize("loss_fn", ["MSE", "L1", "Huber"])
def test_photometric_sizes(renderer, n, loss_fn):
    check_photo(renderer, random_photo(n, 7 * n), dict(SHIPPED, loss_fn=loss_fn), f"n={n} {loss_fn}")


def test_photometric_planted_values_are_exact(renderer, golden):
    c = ref.golden_case(golden, "planted_l1_zero")
    n = len(c["acc_map"])
    _, _, got = run_photo(renderer, ref.photo_inputs(c), ref.photo_settings(c))
    g = got["d_rgb_map"].cpu().numpy()
    zero = c["rgb_map"] == c["target"]
    assert zero.sum() >= 10 and (g[zero] == 0).all()
    assert (np.abs(g[~zero]) == np.float32(1.0 / (3 * n))).all()
    c = ref.golden_case(golden, "planted_huber_knee")
    n = len(c["acc_map"])
    _, _, got = run_photo(renderer, ref.photo_inputs(c), ref.photo_settings(c))
    for k, w in (("rgb_map", 1.0), ("rgb0", 0.5)):
        d = c[k].astype(np.float64) - c["target"]
        knee = np.abs(d) == 0.125
        assert (got["d_" + k].cpu().numpy()[knee] == (np.sign(d[knee]) * w / (3 * n)).astype(np.float32)).all()      # the linear branch
    c = ref.golden_case(golden, "planted_bce")
    kw = ref.photo_settings(c)
    ld, _, got = run_photo(renderer, ref.photo_inputs(c), kw)
    _, _, plain = run_photo(renderer, ref.photo_inputs(c), dict(kw, reg_fn=None))
    ones = c["fgs"] == 1.0
    assert torch.equal(got["d_acc_map"][torch.tensor(ones)], plain["d_acc_map"][torch.tensor(ones)])                   # y = 1.0: no BCE gradient
    assert torch.isfinite(got["d_acc_map"]).all() and torch.isfinite(ld["total_loss"])                                   # acc of exactly 0 and 1


def test_nan_in_one_ray_reaches_the_loss(renderer):
    inputs = list(random_photo(65, 3))
    inputs[0] = inputs[0].copy()
    inputs[0][17, 1] = np.nan
    for loss_fn in ("MSE", "L1", "Huber"):
        ld, stats, _ = run_photo(renderer, tuple(inputs), dict(SHIPPED, loss_fn=loss_fn))
        assert torch.isnan(ld["total_loss"]) and torch.isnan(ld["rgb_loss"]) and torch.isnan(stats["psnr"])
        assert torch.isfinite(ld["rgb_loss0"]) and torch.isfinite(ld["reg_loss"])


def test_empty_bce_set_is_nan_with_a_zero_gradient(renderer):
    inputs = list(random_photo(70, 4))
    inputs[6] = np.ones(70, dtype=np.float32)
    ld, _, got = run_photo(renderer, tuple(inputs), SHIPPED)
    _, _, plain = run_photo(renderer, tuple(inputs), dict(SHIPPED, reg_fn=None))
    assert torch.isnan(ld["reg_loss"]) and torch.isnan(ld["reg_loss0"]) and torch.isnan(ld["total_loss"]) and torch.isfinite(ld["rgb_loss"])
    for k in got:
        assert torch.equal(got[k], plain[k]), k


def test_upstream_gradient_scales_and_double_backward_raises(renderer):
    from posegen_amd.train_losses import photometric_loss
    inputs = random_photo(65, 5)
    _, _, one = run_photo(renderer, inputs, SHIPPED)
    _, _, three = run_photo(renderer, inputs, SHIPPED, upstream=3.0)
    for k in one:
        assert torch.equal(three[k], one[k] * 3.0), k
    preds = {"rgb_map": dev(inputs[0], True), "acc_map": dev(inputs[1], True)}
    batch = {"target_s": dev(inputs[4]), "fgs": dev(inputs[6])[:, None]}
    total = photometric_loss(preds, batch, renderer=renderer, **SHIPPED)[0]["total_loss"]
    w = torch.tensor(2.0, dtype=torch.float64, device=DEV, requires_grad=True)       # an upstream gradient that itself wants a gradient
    (g,) = torch.autograd.grad(total * w, preds["rgb_map"], create_graph=True)
    with pytest.raises(RuntimeError, match="once_differentiable"):
        g.sum().backward()


# ---- the pose regulariser ------------------------------------------------------------------------------------------------------------
def run_kp(renderer, args, kw):
    from posegen_amd.train_losses import pose_regulariser
    rots, kps, idx, a_rots, a_kps = args
    r, k = dev(rots, True), dev(kps, True)
    temporal = None
    if "prev" in kw:
        temporal = dict(prev_rots=dev(kw["prev"][0]), prev_kps=dev(kw["prev"][1]), next_rots=dev(kw["nxt"][0]), next_kps=dev(kw["nxt"][1]),
                        temp_val=dev(kw["temp_val"]), temp_coef=kw["temp_coef"])
    total, terms = pose_regulariser(r, k, np.asarray(idx), {"rots": dev(a_rots), "kps": dev(a_kps)}, tol=kw["tol"], coef=kw["coef"],
                                    ext_scale=kw["ext_scale"], temporal=temporal, renderer=renderer)
    total.backward()
    return total, terms, r.grad, k.grad


def check_kp(renderer, args, kw, what):
    vals, grads = ref.pose_regulariser(*args, **kw)
    total, terms, d_rots, d_kps = run_kp(renderer, args, kw)
    close(total, vals["total"], f"[{what}] total")
    for k, v in terms.items():
        close(v, vals[k], f"[{what}] {k}")
        assert not v.requires_grad
    assert set(terms) == set(vals) - {"total"}
    within_one_ulp(d_rots, grads["d_rots"], f"[{what}] d_rots")
    within_one_ulp(d_kps, grads["d_kps"], f"[{what}] d_kps")
    assert not d_rots[..., 2].any()                         # the third column of every matrix
    if "prev" not in kw:
        assert not d_rots[:, 0].any() and not d_kps.any()   # the root joint gets only the temporal term
    return grads, d_rots


def random_kp(n, seed, temporal=True, tol=0.01):
    rng = np.random.RandomState(seed)
    N = 5
    f = lambda s, *shape: rng.normal(0, s, shape).astype(np.float32)
    idx = rng.randint(0, N, n)
    a_rots, a_kps = f(0.5, N, 24, 3, 3), f(0.3, N, 24, 3)
    rots, kps = a_rots[idx] + f(0.1, n, 24, 3, 3), a_kps[idx] + f(0.02, n, 24, 3)        # squares around tol: both branches
    kw = dict(tol=tol, coef=2.0, ext_scale=0.001)
    if temporal:
        kw.update(prev=(rots + f(0.05, n, 24, 3, 3), kps + f(0.02, n, 24, 3)), nxt=(rots + f(0.05, n, 24, 3, 3), kps + f(0.02, n, 24, 3)),
                  temp_val=(rng.uniform(size=n) > 0.3).astype(np.float32), temp_coef=0.05)
    return (rots, kps, idx, a_rots, a_kps), kw


@pytest.mark.parametrize("name", KP)
def test_pose_regulariser_golden_cases(renderer, golden, name):
    c = ref.golden_case(golden, name)
    args, kw = ref.kp_inputs(c)
    grads, d_rots = check_kp(renderer, args, kw, name)
    if name == "kp_planted":                                 # x = tol exactly: excluded by the strict >
        x = ((c["anchor_rots"].astype(np.float64) - c["rots"])[c["kp_idx"]][..., :2]) ** 2
        at = x == 0.015625
        at[:, 0] = False
        assert at.sum() >= 100 and (d_rots.cpu().numpy()[..., :2][at] == 0).all()


@pytest.mark.parametrize("n", SIZES)
def test_pose_regulariser_sizes(renderer, n):
    check_kp(renderer, *random_kp(n, 11 * n, temporal=True), f"n={n} temporal")
    check_kp(renderer, *random_kp(n, 13 * n, temporal=False, tol=0.0), f"n={n} tol=0")


# ---- the gradient norms --------------------------------------------------------------------------------------------------------------
def _params(tensors):
    ps = []
    for t in tensors:
        p = torch.nn.Parameter(torch.zeros(t.shape, device=DEV))
        p.grad = t
        ps.append(p)
    return ps


def check_norms(renderer, tensors, what):
    from posegen_amd.train_losses import grad_norms
    total, avg, per = grad_norms(_params(tensors), renderer)
    want = ref.grad_norms(tensors)
    close(total, want[0], f"[{what}] total_norm")
    close(avg, want[1], f"[{what}] avg_norm")
    assert per.shape == (len(tensors),) and per.dtype == torch.float64
    for i, (a, b) in enumerate(zip(per.cpu().tolist(), want[2])):
        close(a, b, f"[{what}] tensor {i}")
    return total, avg, per


def test_gradient_norms_golden_and_skipped_parameters(renderer, golden):
    from posegen_amd.train_losses import grad_norms
    g = ref.golden_case(golden, "norms")
    tensors = [dev(g[f"g{i}"]) for i in range(5)]
    check_norms(renderer, tensors, "golden")
    m = torch.nn.Module()
    for i, p in enumerate(_params(tensors)):
        m.register_parameter(f"p{i}", p)
    m.register_parameter("no_grad", torch.nn.Parameter(torch.zeros(5, device=DEV)))          # .grad is None: skipped, not counted
    total, avg, per = grad_norms(m, renderer)
    assert per.numel() == 5
    close(avg, ref.grad_norms(tensors)[1], "avg_norm over the five tensors that have a gradient")


def test_gradient_norms_of_unaligned_views_and_every_size(renderer):
    """A gradient sliced at an odd element offset is only 4-byte aligned: every offset 0..3, lengths around the 16-byte quad, the
    1024 slots and the 16384-element segment; the norm of the same values is the same bits wherever they lie"""
    rng = np.random.RandomState(5)
    base = torch.tensor(rng.normal(0, 1, 3 * 16384 + 64).astype(np.float32), device=DEV)
    tensors = [base[o:o + L] for o, L in ((1, 1), (3, 2), (2, 3), (1, 5), (3, 255), (1, 1023), (2, 1025), (3, 4097), (1, 16384), (2, 16385),
                                          (3, 3 * 16384 + 1), (5, 40000), (0, 16383))]
    assert any(t.data_ptr() % 16 for t in tensors)
    _, _, per = check_norms(renderer, tensors, "views")
    _, _, moved = check_norms(renderer, [t.clone() for t in tensors], "the same values, aligned")
    assert torch.equal(per, moved)
    check_norms(renderer, [torch.zeros(0, device=DEV), base[1:8]], "an empty tensor")


# ---- repeatability and the ABI's refusals ----------------------------------------------------------------------------------------------
def test_two_calls_give_the_same_bytes(renderer):
    from posegen_amd.train_losses import grad_norms
    inputs = random_photo(4097, 21)
    a, b = run_photo(renderer, inputs, SHIPPED), run_photo(renderer, inputs, SHIPPED)
    for k in a[0]:
        assert torch.equal(a[0][k], b[0][k]), k
    for k in a[2]:
        assert torch.equal(a[2][k], b[2][k]), k
    args, kw = random_kp(257, 22)
    a, b = run_kp(renderer, args, kw), run_kp(renderer, args, kw)
    assert torch.equal(a[0], b[0]) and torch.equal(a[2], b[2]) and torch.equal(a[3], b[3])
    ps = _params([torch.randn(s, device=DEV) for s in (7, 40000, 256 * 7)])
    a, b = grad_norms(ps, renderer), grad_norms(ps, renderer)
    assert all(torch.equal(x, y) for x, y in zip(a, b))


def test_the_library_refuses_before_it_launches(renderer):
    from posegen_amd import _ffi
    r = renderer
    n = 8
    f = lambda *s: torch.rand(*s, device=DEV)
    rgb, acc, target, fgs = f(n, 3), f(n), f(n, 3), f(n)
    summary = torch.full((10,), 7.0, dtype=torch.float64, device=DEV)
    d_rgb = torch.full((n, 3), 7.0, device=DEV)
    p = lambda t: None if t is None else C.c_void_p(t.data_ptr())

    def loss(reg_kind=0, loss_kind=1, rgb0=None, acc0=None, beta=0.1, n=n, fgs=fgs):
        return r.lib.pg_train_loss(r.handle, r._stream(), n, p(rgb), p(acc), p(rgb0), p(acc0), p(target), None, 1.0, p(fgs), loss_kind, beta, 1,
                                   1.0, reg_kind, 0.1, p(summary), p(d_rgb), None, None, None)
    for reg in (_ffi.PG_TRAIN_REG_L1, _ffi.PG_TRAIN_REG_MSE):
        assert loss(reg_kind=reg) == _ffi.PG_EINVAL
        msg = r.lib.pg_last_error(r.handle).decode()
        assert "reduction='off'" in msg and "backward() raises" in msg
    for kw in (dict(reg_kind=9), dict(loss_kind=3), dict(rgb0=rgb), dict(acc0=acc), dict(loss_kind=2, beta=-1.0), dict(n=0), dict(reg_kind=1, fgs=None)):
        assert loss(**kw) == _ffi.PG_EINVAL, kw
    rots, kps = f(n, 24, 3, 3), f(n, 24, 3)
    a_rots, a_kps = f(3, 24, 3, 3), f(3, 24, 3)
    s4 = torch.full((4,), 7.0, dtype=torch.float64, device=DEV)

    def reg(idx, prev_rots=None, N=3):
        arr = np.ascontiguousarray(idx, dtype=np.int32)
        return r.lib.pg_pose_reg_loss(r.handle, r._stream(), n, p(rots), p(kps), N, p(a_rots), p(a_kps), arr.ctypes.data_as(C.POINTER(C.c_int32)),
                                      0.01, 2.0, 0.001, p(prev_rots), None, None, None, None, 0.0, p(s4), None, None)
    assert reg([0, 1, 2, 0, 1, 2, 3, 0]) == _ffi.PG_EINVAL and "kp_idx[6] = 3" in r.lib.pg_last_error(r.handle).decode()
    assert reg([0, -1, 2, 0, 1, 2, 0, 0]) == _ffi.PG_EINVAL
    assert reg([0] * n, prev_rots=rots) == _ffi.PG_EINVAL
    assert reg([0] * n, N=0) == _ffi.PG_EINVAL
    out = torch.full((4,), 7.0, dtype=torch.float64, device=DEV)
    ptrs, counts = (C.c_void_p * 1)(rgb.data_ptr()), (C.c_int64 * 1)(rgb.numel())
    assert r.lib.pg_grad_norms(r.handle, r._stream(), 0, ptrs, counts, p(out)) == _ffi.PG_EINVAL
    assert "divides by zero" in r.lib.pg_last_error(r.handle).decode()
    assert r.lib.pg_grad_norms(r.handle, r._stream(), 257, ptrs, counts, p(out)) == _ffi.PG_EINVAL
    torch.cuda.synchronize()
    assert (summary == 7.0).all() and (d_rgb == 7.0).all() and (s4 == 7.0).all() and (out == 7.0).all()      # nothing was written


# ---- one training step, end to end ---------------------------------------------------------------------------------------------------
def test_train_batch_against_the_same_step_with_torch_losses():
    """64 rays, N_samples = 32, N_importance = 16, the pose layer in front: one HipTrainer.train_batch against the same step written
    with the restatement's torch losses (float64, autograd) on the same TrainableRayCaster and the same pose layer."""
    from posegen_amd.batches import RayBatch
    from posegen_amd.poseopt import HipPoseOptLayer, axisang_to_rot6d
    from posegen_amd.raycaster import HipRayCaster
    from posegen_amd.render import render
    from posegen_amd.skeleton import SURREAL_REST_SCALE, smpl_rest_pose
    from posegen_amd.train import TrainableRayCaster
    from posegen_amd.trainer import HipTrainer, temporal_indices
    g = load_golden("train_grads_pose")
    cfg = cfg_from_golden(g)
    wc, wf, tv, td = model_for(cfg, int(g["seed_model"]))
    m = TrainableRayCaster(HipRayCaster.from_weights(cfg, wc, wf, float(tv), float(td), device=DEV, precision="fp32"), train_precision="fp32",
                           opt_pose=True)
    m.train()
    sel = np.concatenate([np.arange(48), np.arange(16)])                               # 64 rays of the fixture's two frames
    rb, kp_idx = g["ray_batch"][sel], g["kp_idx"][sel].astype(np.int64)
    n = len(sel)
    rng = np.random.RandomState(8)
    rest = (smpl_rest_pose * SURREAL_REST_SCALE).astype(np.float32)[None]
    sd = {"pelvis": torch.tensor(g["kps"][:, 0].copy()), "bones": torch.tensor(axisang_to_rot6d(g["bones"])), "rest_pose": torch.tensor(rest)}
    layer = HipPoseOptLayer.from_state_dict(sd, renderer=m.renderer)
    with torch.no_grad():                                                               # anchors: the initial poses; the layer has moved since
        a_kps, _, _, _, a_rots = layer(np.arange(2))
        anchors = {"rots": a_rots.clone(), "kps": a_kps.clone()}
        layer.bones.add_(torch.tensor(rng.normal(0, 0.08, (2, 24, 6)).astype(np.float32), device=DEV))
        layer.pelvis.add_(torch.tensor(rng.normal(0, 0.01, (2, 3)).astype(np.float32), device=DEV))
    batch = RayBatch(rays=dev(np.stack([rb[:, :3], rb[:, 3:6]])), target_s=dev(g["target"][sel]), cyls=dev(g["cyl"][kp_idx]),
                     fgs=dev(np.where(rng.uniform(size=n) < 0.4, 1.0, rng.uniform(0, 0.9, n)).astype(np.float32))[:, None],
                     bgs=dev(rng.uniform(0, 1, (n, 3)).astype(np.float32)), kp_idx=dev(kp_idx),
                     temp_val=dev((rng.uniform(size=n) > 0.3).astype(np.float32)))
    batch.kp_idx_host = kp_idx
    args = SimpleNamespace(loss_fn="L1", loss_beta=0.1, reg_fn="BCE", reg_coef=0.1, use_background=True, coarse_weight=0.5, opt_pose=True,
                           opt_pose_stop=None, opt_pose_step=1, opt_pose_tol=0.01, opt_pose_coef=2.0, opt_rot6d=True, opt_pose_cache=False,
                           use_temp_loss=True, temp_coef=0.05, ext_scale=0.001, opt_framecode=False, chunk=4096, lrate=5e-4, lrate_decay=500,
                           lrate_decay_rate=0.1, decay_unit=1000, finetune=False, cutoff_step=100, cutoff_rate=10.0)
    kw_train = dict(ray_caster=m, N_samples=32, N_importance=16, near=dev(rb[:, 6:7]), far=dev(rb[:, 7:8]))
    params = {k: p_ for k, p_ in m.named_parameters() if p_.requires_grad}             # (the embedders' cutoff_dist is frozen)
    pose = {"pelvis": layer.pelvis, "bones": layer.bones}

    # the same step with torch losses
    kps, bones, skts, _, rots = layer(kp_idx)
    preds = render(0, 0, 0.0, chunk=4096, kp_batch=kps, skts=skts, bones=bones, cyls=batch["cyls"], rays=batch["rays"], cams=None,
                   subject_idxs=None, **kw_train)
    d = lambda t: t.double()
    passes = [("", d(preds["rgb_map"]), d(preds["acc_map"])), ("0", d(preds["rgb0"]), d(preds["acc0"]))]
    settings = dict(loss_fn="L1", loss_beta=0.1, use_background=True, coarse_weight=0.5, reg_fn="BCE", reg_coef=0.1)
    total, vals = ref.photometric_graph(passes, d(batch["target_s"]), d(batch["bgs"]), d(batch["fgs"][:, 0]), **settings)
    prev, nxt = temporal_indices(kp_idx, 2)
    with torch.no_grad():
        pk, _, _, _, pr = layer(prev)
        nk, _, _, _, nr = layer(nxt)
    reg, kvals = ref.pose_graph(d(rots), d(kps), torch.tensor(kp_idx, device=DEV), d(anchors["rots"]), d(anchors["kps"]), tol=0.01, coef=2.0,
                                ext_scale=0.001, prev=(d(pr), d(pk)), nxt=(d(nr), d(nk)), temp_val=d(batch["temp_val"]), temp_coef=0.05)
    (total + reg).backward()
    want = {k: p_.grad.detach().clone() for k, p_ in {**params, **pose}.items()}
    want_stats = {k: float(v.detach()) for k, v in {**vals, **kvals}.items() if not k.startswith("n_bce") and k != "total"}
    want_stats["total_loss"] = float((total + reg).detach())
    norms = ref.grad_norms([p_.grad.cpu().numpy() for p_ in m.parameters() if p_.grad is not None])
    want_stats.update(total_norm=norms[0], avg_norm=norms[1])
    for p_ in list(params.values()) + list(pose.values()):
        p_.grad = None

    # the trainer's step; lr = 0 leaves the parameters where they are, hooks keep the gradients zero_grad drops
    got = {}
    hooks = [p_.register_hook(lambda gr, k=k: got.__setitem__(k, gr.detach().clone())) for k, p_ in {**params, **pose}.items()]
    opt, popt = torch.optim.SGD(list(params.values()), lr=0.0), torch.optim.SGD(list(pose.values()), lr=0.0)
    tr = HipTrainer(args, {"hwf": (0, 0, 0.0)}, opt, popt, kw_train, {}, popt_kwargs={"popt_layer": layer, "popt_anchors": anchors})
    loss_dict, stats = tr.train_batch(batch, i=0, global_step=0)
    for h in hooks:
        h.remove()
    assert set(loss_dict) == {"rgb_loss", "reg_loss", "rgb_loss0", "reg_loss0", "kp_loss", "temp_loss", "total_loss"}
    assert set(stats) == {"lrate", "cutoff", "psnr", "psnr0", "alpha", "MPJPC", "total_norm", "avg_norm"}
    for k, v in {**loss_dict, **stats}.items():
        assert isinstance(v, float)
        if k in want_stats:
            print(f"{k}: {v!r} against {want_stats[k]!r}")
            assert abs(v - want_stats[k]) <= 1e-6 * max(1.0, abs(want_stats[k])), k
    assert stats["lrate"] == 5e-4 and stats["cutoff"] == 20.0 and tr.optim_steps == 1
    assert all(p_.grad is None or not p_.grad.any() for p_ in list(params.values()) + list(pose.values()))             # zero_grad ran
    assert set(got) == set(want) and len(got) == 50
    worst = 0.0
    for k in want:
        a, b = got[k].double(), want[k].double()
        scale = max(float(b.abs().max()), float(b.norm()) / np.sqrt(b.numel()))
        assert scale > 0, k
        worst = max(worst, float((a - b).abs().max()) / scale)
    print(f"parameter and pose gradients: largest difference {worst:.2e} of the tensor's scale")
    assert worst <= 1e-5
    values, names, host = tr.train_batch(batch, i=1, global_step=1, fetch=False)                                        # the device vector
    assert values.is_cuda and values.dtype == torch.float64 and values.shape == (len(names),) and set(host) == {"lrate", "cutoff"}
    assert names[:7] == list(loss_dict) and tr.optim_steps == 2
    m.renderer.close()


def test_train_batch_without_pose_refinement():
    """The two branches that leave the poses alone: no pose layer (the batch's own kp3d / skts / bones, trainer.py:293-295), and a
    layer past `opt_pose_stop` (its outputs detached, no kp_loss, the pose optimiser not stepped).  MSE on a white background is
    tests.helpers.loss_of; Adam moves the nets and the host-side step count drives the learning rate."""
    from posegen_amd.batches import RayBatch
    from posegen_amd.poseopt import HipPoseOptLayer, axisang_to_rot6d
    from posegen_amd.raycaster import HipRayCaster
    from posegen_amd.skeleton import SURREAL_REST_SCALE, smpl_rest_pose
    from posegen_amd.train import TrainableRayCaster
    from posegen_amd.trainer import HipTrainer, decayed_lrate
    from tests.helpers import loss_of
    g = load_golden("train_grads_pose")
    cfg = cfg_from_golden(g)
    wc, wf, tv, td = model_for(cfg, int(g["seed_model"]))
    m = TrainableRayCaster(HipRayCaster.from_weights(cfg, wc, wf, float(tv), float(td), device=DEV, precision="fp32"), train_precision="fp32",
                           opt_pose=True)
    m.train()
    rb, kp_idx = g["ray_batch"], g["kp_idx"].astype(np.int64)
    batch = RayBatch(rays=dev(np.stack([rb[:, :3], rb[:, 3:6]])), target_s=dev(g["target"]), cyls=dev(g["cyl"][kp_idx]), kp_idx=dev(kp_idx),
                     kp3d=dev(g["kps"][kp_idx]), skts=dev(g["skts"][kp_idx]), bones=dev(g["bones"][kp_idx]))
    batch.kp_idx_host = kp_idx
    args = SimpleNamespace(loss_fn="MSE", loss_beta=0.1, reg_fn=None, reg_coef=0.0, use_background=True, coarse_weight=1.0, opt_pose=False,
                           opt_pose_stop=None, opt_pose_step=1, opt_pose_tol=0.01, opt_pose_coef=2.0, opt_rot6d=True, opt_pose_cache=False,
                           use_temp_loss=False, temp_coef=0.0, ext_scale=0.001, opt_framecode=False, chunk=4096, lrate=1e-3, lrate_decay=2,
                           lrate_decay_rate=0.1, decay_unit=1, finetune=True)
    kw_train = dict(ray_caster=m, N_samples=32, N_importance=16, near=dev(rb[:, 6:7]), far=dev(rb[:, 7:8]))
    nets = [p_ for p_ in m.parameters() if p_.requires_grad]
    with torch.no_grad():
        want = float(loss_of(m(dev(rb), N_samples=32, skts=batch["skts"], cyls=batch["cyls"], N_importance=16), batch["target_s"]))
    before = [p_.detach().clone() for p_ in nets]
    opt = torch.optim.Adam(nets, lr=1e-3)
    tr = HipTrainer(args, {"hwf": (0, 0, 0.0)}, opt, None, kw_train, {})
    loss_dict, stats = tr.train_batch(batch, i=0, global_step=0)
    assert set(loss_dict) == {"rgb_loss", "rgb_loss0", "total_loss"} and "MPJPC" not in stats
    assert abs(loss_dict["total_loss"] - want) <= 1e-6 * max(1.0, want)                 # (the eval-mode maps: fp32 kernels of the same nets)
    assert sum(int(not torch.equal(a, b.detach())) for a, b in zip(before, nets)) == len(nets)
    assert stats["total_norm"] > 0 and tr.optim_steps == 1
    assert stats["lrate"] == decayed_lrate(1e-3, 2, 0.1, 1, 1) == opt.param_groups[0]["lr"]

    rest = (smpl_rest_pose * SURREAL_REST_SCALE).astype(np.float32)[None]
    sd = {"pelvis": torch.tensor(g["kps"][:, 0].copy()), "bones": torch.tensor(axisang_to_rot6d(g["bones"])), "rest_pose": torch.tensor(rest)}
    layer = HipPoseOptLayer.from_state_dict(sd, renderer=m.renderer)
    pose_before = [p_.detach().clone() for p_ in layer.parameters()]
    popt = torch.optim.Adam(list(layer.parameters()), lr=1e-2)
    args.opt_pose, args.opt_pose_stop = True, 0                                          # i = 0 is already past the stop
    anchors = {"rots": torch.zeros(2, 24, 3, 3, device=DEV), "kps": torch.zeros(2, 24, 3, device=DEV)}
    tr = HipTrainer(args, {"hwf": (0, 0, 0.0)}, opt, popt, kw_train, {}, popt_kwargs={"popt_layer": layer, "popt_anchors": anchors})
    assert tr.optim_steps == 1                                                           # read from the optimiser's state
    loss_dict, stats = tr.train_batch(batch, i=0, global_step=0)
    assert set(loss_dict) == {"rgb_loss", "rgb_loss0", "total_loss"} and "MPJPC" not in stats and tr.optim_steps == 2
    assert all(p_.grad is None for p_ in layer.parameters())
    assert all(torch.equal(a, b.detach()) for a, b in zip(pose_before, layer.parameters()))
    m.renderer.close()
