"""Pose refinement on the HIP path: `TrainableRayCaster(opt_pose=True)`, whose backward (pg_train_backward_pose) also gives
dL/dskts -- the reference's opt_pose training (core/trainer.py:286-313, 453-485), where the poses come out of PoseOptLayer with
autograd history.  Checked against the reference's own autograd (tests/golden/train_grads_pose*.npz) and against the float64
oracle across shapes in both training precisions, with the bounds and the ill-conditioned-sum rule of test_gpu_train_shapes.py
(fp32: every entry within 1e-4 of the tensor's scale max(largest entry, norm / sqrt(size)), the norm within 1e-4; bf16: 0.1 and
1e-2; a case outside its bound gets max(bound, 4 x the fp32 oracle's own deviation from float64), printed, never a looser
constant).  Also: the parameter gradients do not move, the pose gradient is bitwise repeatable, a 20-step pose-only Adam loop
follows the oracle's, and the contract of the keyword and of the ABI entry."""
import ctypes as C

import numpy as np
import pytest
import torch

from tests.helpers import cfg_from_golden, default_dtype, golden_draws, load_golden, loss_of, model_for, oracle_cfg
from tests.test_pose_grad_host import scale_of

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
BOUNDS = {"fp32": dict(entry=1e-4, norm=1e-4), "bf16": dict(entry=0.1, norm=1e-2)}


def _caster(cfg, weights, train_precision="fp32", opt_pose=True):
    from posegen_amd.raycaster import HipRayCaster
    from posegen_amd.train import TrainableRayCaster
    wc, wf, tv, td = weights
    c = HipRayCaster.from_weights(cfg, wc, wf, float(tv), float(td), device=DEV, precision="fp32")
    m = TrainableRayCaster(c, train_precision=train_precision, opt_pose=opt_pose)
    m.train()
    return m


def _deviation(got, ref):
    """(largest entry deviation / scale, norm deviation / norm)"""
    got, ref = np.asarray(got, dtype=np.float64), np.asarray(ref, dtype=np.float64)
    rn = float(np.linalg.norm(ref))
    return float(np.abs(got - ref).max()) / scale_of(ref), abs(float(np.linalg.norm(got)) - rn) / max(rn, 1e-30)


# ---- the reference's own step ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["train_grads_pose", "train_grads_pose_h36m"])
def test_pose_gradient_matches_the_reference_autograd(name):
    """The reference's training step with per-ray poses that require a gradient (two frames by kp_idx; h36m: frame codes,
    64 + 16): dL/dskts of every ray within 1e-4 of its scale, its norm within 1e-4, fp32 mode."""
    g = load_golden(name)
    cfg = cfg_from_golden(g)
    m = _caster(cfg, model_for(cfg, int(g["seed_model"])))
    kp_idx = g["kp_idx"]
    sk = torch.tensor(g["skts"][kp_idx]).requires_grad_(True)
    cams = torch.tensor(g["cams"]) if "cams" in g else None
    out = m(torch.tensor(g["ray_batch"]), N_samples=cfg.n_samples, skts=sk, cyls=torch.tensor(g["cyl"][kp_idx]), cams=cams,
            N_importance=cfg.n_importance, draws=golden_draws(g))
    loss = loss_of(out, torch.tensor(g["target"], device=DEV))
    assert abs(float(loss.detach()) - float(g["loss"])) <= 1e-5 * max(1.0, abs(float(g["loss"])))
    loss.backward()
    assert sk.grad is not None and sk.grad.shape == sk.shape and sk.grad.device == sk.device
    ent, nrm = _deviation(sk.grad.numpy(), g["dskts"])
    print(f"{name}: dL/dskts entries within {ent:.2e} of the scale, norm within {nrm:.2e}")
    assert ent <= 1e-4 and nrm <= 1e-4
    assert bool((sk.grad[..., 3, :] == 0).all())
    m.renderer.close()


# ---- the float64 oracle across shapes ----------------------------------------------------------------------------------
POSE_CASES = {
    # pose layouts: "shared" [1,24,4,4], "per_ray" [n,24,4,4] of their own, "expand" one [1,24,4,4] leaf expanded to n
    "shared": dict(n=13, S=33, N=7, pose="shared"),
    "per_ray": dict(n=21, S=32, N=8, per_ray=True, pose="per_ray"),
    "expand": dict(n=13, S=33, N=7, pose="expand"),
    "coarse_only": dict(n=7, S=40, N=0, per_ray=True, pose="per_ray"),
    "ray_noise": dict(n=13, S=33, N=7, ray_noise_std=1.0, per_ray=True, pose="per_ray"),
    "softplus": dict(n=13, S=33, N=7, fixture="train_grads_softplus", pose="shared"),
    "framecodes": dict(n=37, S=64, N=16, fixture="train_grads_h36m", per_ray=True, pose="per_ray"),
    "miss": dict(n=40, S=32, N=8, miss=True, pose="shared"),
    "p32": dict(n=1, S=32, N=0, first=1, pose="shared"),
    "p48_64": dict(n=1, S=48, N=16, per_ray=True, pose="per_ray"),
}
_ORACLE = {}


def _pose_case(key):
    from tests import test_gpu_train_shapes as ts
    opts = dict(POSE_CASES[key])
    pose = opts.pop("pose")
    ts.CASES[f"pose_{key}"] = opts
    c = ts._case(f"pose_{key}")
    c["pose"] = pose
    if pose == "shared" or pose == "expand":
        c["skts"] = c["skts"][:1]
    return c


def _leaf_and_input(skts, pose, n, dtype=torch.float32):
    """(the leaf that receives the gradient, the tensor handed to the caster)"""
    leaf = torch.tensor(np.asarray(skts), dtype=dtype).requires_grad_(True)
    return leaf, (leaf.expand(n, -1, -1, -1) if pose == "expand" else leaf)


def _oracle_pose(key, c, dtype=torch.float64):
    """the oracle's step under autograd in `dtype` with the poses requiring a gradient: (loss, dL/d(leaf))"""
    if (key, dtype) not in _ORACLE:
        from oracle import anerf_oracle as orc
        wc, wf, tv, td = c["weights"]
        n = c["rb"].shape[0]
        cast = lambda x: None if x is None else torch.as_tensor(np.asarray(x)).to(dtype)
        with default_dtype(dtype):
            nets = [{k: cast(v) for k, v in w.items()} for w in (wc, wf)]
            leaf, sk = _leaf_and_input(c["skts"], c["pose"], n, dtype)
            dr = {k: cast(v) for k, v in c["draws"].items()}
            out = orc.render_rays(cast(c["rb"]), sk, cast(c["cyls"]), oracle_cfg(c["cfg"], tv, td), nets[0], nets[1], c["S"], c["N"],
                                  cams=cast(c["cams"]), lindisp=c["lindisp"], draws=dr)
            loss = loss_of(out, cast(c["target"]))
            loss.backward()
        _ORACLE[(key, dtype)] = (float(loss.detach()), leaf.grad.double().numpy())
    return _ORACLE[(key, dtype)]


def _hip_pose(c, train_precision, opt_pose=True, skts_grad=True, m=None):
    """one HIP step: (loss, dL/d(leaf) or None, {(tag, name): parameter gradient}, caster)"""
    wc, wf, tv, td = c["weights"]
    m = m or _caster(c["cfg"], c["weights"], train_precision, opt_pose)
    for p in m.parameters():
        p.grad = None
    n = c["rb"].shape[0]
    leaf, sk = _leaf_and_input(c["skts"], c["pose"], n)
    if not skts_grad:
        leaf.requires_grad_(False)
        sk = sk.detach()
    cams = None if c["cams"] is None else torch.tensor(c["cams"])
    out = m(torch.tensor(c["rb"]), N_samples=c["S"], skts=sk, cyls=torch.tensor(c["cyls"]), cams=cams, N_importance=c["N"],
            lindisp=c["lindisp"], draws={k: v.to(DEV) for k, v in c["draws"].items()})
    loss = loss_of(out, torch.tensor(c["target"], device=DEV))
    loss.backward()
    grads = {(tag, k): p.grad.detach().clone() for tag, net in (("coarse", m.network), ("fine", m.network_fine))
             for k, p in net.named_parameters() if p.grad is not None}
    return float(loss.detach()), (leaf.grad.numpy().copy() if skts_grad else None), grads, m


def _check_pose(key, c, tp, got):
    """compare dL/dskts with the float64 oracle under the bounds of `tp` (+ the ill-conditioned-sum rule); returns the bounds"""
    _, ref = _oracle_pose(key, c)
    assert got.shape == ref.shape and np.isfinite(got).all()
    assert float(np.abs(ref).max()) > 0, "a case whose pose gradient is all zeros"
    b = BOUNDS[tp]
    te, tn = b["entry"], b["norm"]
    ent, nrm = _deviation(got, ref)
    if ent > te or nrm > tn:
        e32, n32 = _deviation(_oracle_pose(key, c, torch.float32)[1], ref)
        te, tn = max(te, 4.0 * e32), max(tn, 4.0 * n32)
        print(f"[{key}] {tp}: dL/dskts deviates {ent:.2e} / {nrm:.2e} (entries / norm); the fp32 oracle's own deviation "
              f"{e32:.2e} / {n32:.2e}: bounds {te:.2e} / {tn:.2e}")
    print(f"[{key}] {tp}: {c['rb'].shape[0]} rays x {c['S']} + {c['N']}, poses {c['pose']}: dL/dskts within {ent:.2e} / {nrm:.2e}")
    assert ent <= te and nrm <= tn, (key, tp, ent, nrm, te, tn)
    return te, tn


@pytest.mark.parametrize("key,train_precision", [(k, tp) for k in POSE_CASES for tp in ("fp32", "bf16")
                                                 if not (k == "softplus" and tp == "bf16")])
def test_pose_gradient_matches_the_float64_oracle(key, train_precision):
    """One case of the shape / option matrix in one training precision (softplus: fp32 only, as in test_gpu_train_shapes.py:
    its rays are all opaque and the gradients behind them hang on fp32 rounding).  Negative control (per_ray, fp32): the same
    comparison rejects a copy of the HIP gradient with its largest entry scaled by 1 + 1e-3."""
    c = _pose_case(key)
    _, got, _, m = _hip_pose(c, train_precision)
    te, tn = _check_pose(key, c, train_precision, got)
    if key == "per_ray" and train_precision == "fp32":
        assert te == 1e-4 and tn == 1e-4
        ref = _oracle_pose(key, c)[1]
        wrong = got.copy()
        wrong[np.unravel_index(int(np.argmax(np.abs(ref))), ref.shape)] *= 1 + 1e-3
        assert _deviation(wrong, ref)[0] > te, "the comparison must reject a pose gradient entry off by 1e-3"
    m.renderer.close()


def test_pose_gradient_at_bench_shape_matches_the_float64_oracle():
    """The timed step's shape (4096 rays x (64 + 16)) with per-ray poses, fp32 and bf16, against one float64 oracle run.  (Some
    of its rays are opaque: the per-ray gradients behind them hang on fp32 rounding, and the fp32 oracle itself lies ~1e-3 of
    the scale from float64 there -- the ill-conditioned-sum rule sets that bound; the norm stays within 1e-4.)"""
    POSE_CASES["bench"] = dict(n=4096, S=64, N=16, per_ray=True, pose="per_ray")
    c = _pose_case("bench")
    for tp in ("fp32", "bf16"):
        _, got, _, m = _hip_pose(c, tp)
        te, tn = _check_pose("bench", c, tp, got)
        if tp == "fp32":
            assert tn == 1e-4
        m.renderer.close()
    _ORACLE.pop(("bench", torch.float64), None)
    _ORACLE.pop(("bench", torch.float32), None)


# ---- no side effects ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("train_precision", ["fp32", "bf16"])
def test_pose_gradient_leaves_the_parameter_gradients_bitwise_and_is_repeatable(train_precision):
    """The parameter gradients of a step with opt_pose and skts requiring a gradient are bitwise those of the same step with a
    detached skts; two identical pose steps give bitwise equal dL/dskts."""
    c = _pose_case("framecodes")
    _, g1, p1, m = _hip_pose(c, train_precision)
    _, g2, p2, _ = _hip_pose(c, train_precision, m=m)
    _, none, p0, _ = _hip_pose(c, train_precision, skts_grad=False, m=m)
    assert none is None
    assert np.array_equal(g1, g2), "dL/dskts is not bitwise repeatable"
    assert set(p0) == set(p1) and len(p0) == 50
    for k in p0:
        assert torch.equal(p0[k], p1[k]), k
        assert torch.equal(p1[k], p2[k]), k
    m.renderer.close()


# ---- a pose-only optimisation loop -------------------------------------------------------------------------------------
def _rodrigues(w):
    """axis-angle [F,3] -> rotation [F,3,3], differentiable (at 0 too)"""
    th2 = (w * w).sum(-1, keepdim=True)[..., None]
    K = torch.zeros(w.shape[0], 3, 3, dtype=w.dtype)
    K[:, 0, 1], K[:, 0, 2], K[:, 1, 0] = -w[:, 2], w[:, 1], w[:, 2]
    K[:, 1, 2], K[:, 2, 0], K[:, 2, 1] = -w[:, 0], -w[:, 1], w[:, 0]
    big = th2 > 1e-12
    th2s = torch.where(big, th2, torch.ones_like(th2))        # (no 0 / 0 in the branch torch.where does not take: its gradient)
    th = torch.sqrt(th2s)
    a = torch.where(big, torch.sin(th) / th, 1 - th2 / 6)
    b = torch.where(big, (1 - torch.cos(th)) / th2s, 0.5 - th2 / 24)
    return torch.eye(3, dtype=w.dtype) + a * K + b * (K @ K)


def _posed(skts0, w, t):
    """skts0 [F,24,4,4] after a rigid motion of every frame's body (rotation w, translation t of the world points):
    skt' = skt [R t; 0 1]"""
    F_ = skts0.shape[0]
    M = torch.zeros(F_, 4, 4, dtype=w.dtype)
    M[:, :3, :3] = _rodrigues(w)
    M[:, :3, 3] = t
    M[:, 3, 3] = 1
    return skts0 @ M[:, None]


def test_pose_only_adam_loop_follows_the_oracle():
    """20 Adam steps on a per-frame root rotation + translation over the fixed poses of train_grads_pose (two frames, per-ray
    poses by kp_idx), the nets' parameters outside the optimiser; the targets are rendered (float64 oracle, eval mode) from a
    displaced pose.  The HIP loop's loss follows the float64 oracle's loop within the fp32 bounds (1e-5 of the loss) at every
    step, and its last loss is below its first."""
    from oracle import anerf_oracle as orc
    g = load_golden("train_grads_pose")
    cfg = cfg_from_golden(g)
    weights = model_for(cfg, int(g["seed_model"]))
    wc, wf, tv, td = weights
    kp_idx = torch.tensor(g["kp_idx"])
    rb, cy = g["ray_batch"], g["cyl"][g["kp_idx"]]
    S, N = cfg.n_samples, cfg.n_importance
    w_true = torch.tensor([[0.04, -0.03, 0.02], [-0.02, 0.05, 0.03]], dtype=torch.float64)
    t_true = torch.tensor([[0.02, -0.01, 0.015], [-0.015, 0.02, 0.01]], dtype=torch.float64)
    ocfg = oracle_cfg(cfg, tv, td)
    with default_dtype(torch.float64):
        nets64 = [{k: torch.tensor(v, dtype=torch.float64) for k, v in w.items()} for w in (wc, wf)]
        sk_t = _posed(torch.tensor(g["skts"], dtype=torch.float64), w_true, t_true)[kp_idx]
        target = orc.render_rays(torch.tensor(rb, dtype=torch.float64), sk_t, torch.tensor(cy, dtype=torch.float64), ocfg,
                                 nets64[0], nets64[1], S, N)
        target = (target["rgb_map"] + (1 - target["acc_map"])[..., None]).detach()

    def loop(step, dtype):
        w = torch.zeros(2, 3, dtype=dtype, requires_grad=True)
        t = torch.zeros(2, 3, dtype=dtype, requires_grad=True)
        opt = torch.optim.Adam([w, t], lr=5e-3)
        skts0 = torch.tensor(g["skts"], dtype=dtype)
        losses = []
        for _ in range(20):
            opt.zero_grad()
            loss = step(_posed(skts0, w, t)[kp_idx], target.to(dtype))
            loss.backward()
            opt.step()
            losses.append(float(loss.detach()))
        return np.array(losses)

    m = _caster(cfg, weights, "fp32", opt_pose=True)
    hip_step = lambda sk, tg: loss_of(m(torch.tensor(rb), N_samples=S, skts=sk, cyls=torch.tensor(cy), N_importance=N), tg.to(DEV)).cpu()
    hip = loop(hip_step, torch.float32)

    def oracle_step(dtype):
        def step(sk, tg):
            with default_dtype(dtype):
                nets = [{k: torch.tensor(v, dtype=dtype) for k, v in w.items()} for w in (wc, wf)]
                out = orc.render_rays(torch.tensor(rb, dtype=dtype), sk, torch.tensor(cy, dtype=dtype), ocfg, nets[0], nets[1], S, N)
                return loss_of(out, tg)
        return step
    ref = loop(oracle_step(torch.float64), torch.float64)
    dev = np.abs(hip - ref) / np.maximum(1.0, np.abs(ref))
    tol = np.full(20, 1e-5)
    if (dev > tol).any():
        own = np.abs(loop(oracle_step(torch.float32), torch.float32) - ref) / np.maximum(1.0, np.abs(ref))
        tol = np.maximum(tol, 4.0 * own)
        print(f"pose loop: the fp32 oracle's own deviation per step, largest {own.max():.2e}")
    print("pose loop losses (HIP):", " ".join(f"{v:.6f}" for v in hip))
    print(f"pose loop: largest deviation from the float64 oracle's loop {dev.max():.2e}")
    assert (dev <= tol).all(), (dev, tol)
    assert hip[-1] < hip[0] and ref[-1] < ref[0]
    m.renderer.close()


# ---- the contract ------------------------------------------------------------------------------------------------------
def test_opt_pose_contract():
    """opt_pose=True: kp_batch / bones that require a gradient are accepted and get none (the shipped encoders do not read
    them); ray_batch / cyls that require one are refused; skts [24,4,4] gets the sum in its own shape.  The ABI refuses a
    d_pose_stride other than 0 / 384, a null d_skts and a stale tape."""
    from posegen_amd import _ffi
    g = load_golden("train_grads_pose_h36m")
    cfg = cfg_from_golden(g)
    m = _caster(cfg, model_for(cfg, int(g["seed_model"])))
    rb, cy = torch.tensor(g["ray_batch"]), torch.tensor(g["cyl"][0])
    cams = torch.tensor(g["cams"])
    kp = torch.tensor(g["kps"][0]).expand(rb.shape[0], -1, -1).clone().requires_grad_(True)
    bones = torch.tensor(g["bones"][0]).expand(rb.shape[0], -1, -1).clone().requires_grad_(True)
    sk = torch.tensor(g["skts"][0]).requires_grad_(True)            # [24,4,4]: the sum over the rays
    call = dict(N_samples=cfg.n_samples, N_importance=cfg.n_importance, cams=cams, draws=golden_draws(g))
    out = m(rb, kp_batch=kp, skts=sk, cyls=cy, bones=bones, **call)
    loss_of(out, torch.tensor(g["target"], device=DEV)).backward()
    assert kp.grad is None and bones.grad is None
    assert sk.grad is not None and sk.grad.shape == (24, 4, 4)
    np.testing.assert_allclose(sk.grad.numpy(), g["dskts"].sum(0), rtol=0, atol=1e-4 * scale_of(g["dskts"].sum(0)))
    with pytest.raises(NotImplementedError, match="ray_batch requires a gradient"):
        m(rb.clone().requires_grad_(True), skts=sk, cyls=cy, **call)
    with pytest.raises(NotImplementedError, match="cyls requires a gradient"):
        m(rb, skts=sk, cyls=cy.clone().requires_grad_(True), **call)
    r = m.renderer
    gr = _ffi.PgNetGrads()
    buf = torch.zeros(24, 4, 4, device=DEV)
    with pytest.raises(_ffi.PgError) as e:
        r._check(r.lib.pg_train_backward_pose(r.handle, None, 1, None, None, None, None, C.byref(gr), C.byref(gr), buf.data_ptr(), 7))
    assert e.value.code == _ffi.PG_EINVAL
    with pytest.raises(_ffi.PgError) as e:
        r._check(r.lib.pg_train_backward_pose(r.handle, None, 1, None, None, None, None, C.byref(gr), C.byref(gr), None, 0))
    assert e.value.code == _ffi.PG_EINVAL
    with pytest.raises(_ffi.PgError) as e:        # the tape holds a later forward pass than id -5
        r._check(r.lib.pg_train_backward_pose(r.handle, None, -5, None, None, None, None, C.byref(gr), C.byref(gr), buf.data_ptr(), 0))
    assert e.value.code == _ffi.PG_ESTATE
    r.close()
