"""The pose layer on the device: `HipPoseOptLayer` over pg_poseopt_forward / pg_poseopt_backward (csrc/pg_poseopt.hip), the
reference's PoseOptLayer (core/pose_opt.py:240-445) with use_rot6d.  Checked against the reference's own values and autograd
(tests/golden/poseopt.npz) and against the float64 restatement (tests/poseopt_ref.py) with the fp32 rule of test_gpu_pose_grad.py /
test_gpu_train_shapes.py: every entry within 1e-4 of the tensor's scale max(largest entry, norm / sqrt(size)), the norm within 1e-4;
a case outside gets max(bound, 4 x the fp32 reference's own deviation from float64), printed, never a looser constant.  Also: the
gradients are bitwise repeatable, the refusals of the ABI, the layer in front of TrainableRayCaster(opt_pose=True), and a pose-only
Adam loop."""
import ctypes as C

import numpy as np
import pytest
import torch

from tests import poseopt_ref as ref
from tests.helpers import cfg_from_golden, default_dtype, load_golden, loss_of, model_for, oracle_cfg
from tests.test_poseopt_host import OUTS, random_case

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
_I32P = C.POINTER(C.c_int32)


@pytest.fixture(scope="module")
def renderer():
    from posegen_amd import surreal_config
    from posegen_amd.raycaster import HipRenderer
    r = HipRenderer(surreal_config(), device=DEV)
    yield r
    r.close()


def _layer(renderer, pelvis, bones, rest, rest_pose_idxs=None):
    from posegen_amd.poseopt import HipPoseOptLayer
    sd = {"pelvis": torch.tensor(pelvis), "bones": torch.tensor(bones), "rest_pose": torch.tensor(rest)}
    return HipPoseOptLayer.from_state_dict(sd, renderer=renderer, rest_pose_idxs=rest_pose_idxs)


def _step(layer, idxs, cot, only=OUTS):
    """forward(idxs), the loss sum(output * cotangent) over the outputs `only`, backward: (outputs as numpy, bones.grad, pelvis.grad)"""
    layer.zero_grad(set_to_none=True)
    kps, bones, skts, l2ws, rots = layer(idxs)
    outs = dict(kps=kps, skts=skts, l2ws=l2ws, rots=rots)
    dev = kps.device
    sum((outs[k] * torch.tensor(cot[k], dtype=kps.dtype, device=dev)).sum() for k in only).backward()
    res = {k: v.detach().cpu().numpy() for k, v in outs.items()}
    res["bones"] = bones.detach().cpu().numpy()
    grad = lambda p_: (torch.zeros_like(p_) if p_.grad is None else p_.grad).cpu().numpy().copy()      # (autograd: None = no path)
    return res, grad(layer.bones), grad(layer.pelvis)


def _restated(pelvis, bones, rest, idxs, cot, only=OUTS, rest_pose_idxs=None):
    """the float64 restatement of the same step: (outputs, bones.grad, pelvis.grad) with zeros at the poses no ray reads"""
    from posegen_amd.poseopt import ray_segments
    seg = ray_segments(idxs)
    rest = np.asarray(rest)
    if rest.shape[0] > 1:
        rest = rest[(np.arange(len(pelvis)) if rest_pose_idxs is None else np.asarray(rest_pose_idxs))[seg.unique]]
    b, p = np.asarray(bones)[seg.unique], np.asarray(pelvis)[seg.unique]
    outs = dict(zip(OUTS, ref.forward(b, p, rest, seg.inverse)))
    db, dp = ref.backward(b, p, rest, seg.inverse, **{f"d_{k}": cot[k] for k in only})
    full_b, full_p = np.zeros(np.asarray(bones).shape), np.zeros(np.asarray(pelvis).shape)
    full_b[seg.unique], full_p[seg.unique] = db, dp
    return outs, full_b, full_p


def _torch32(pelvis, bones, rest, idxs, cot, only=OUTS, rest_pose_idxs=None):
    """the same step of the torch restatement layer in fp32 on the CPU (the fp32 reference of the rule)"""
    ridx = np.arange(len(pelvis)) if rest_pose_idxs is None and np.asarray(rest).shape[0] > 1 else rest_pose_idxs
    return _step(ref.TorchPoseOptLayer(pelvis, bones, rest, rest_pose_idxs=ridx), idxs, cot, only)


# ---- the reference's own values ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("sfx", ["", "_pp"])
def test_layer_matches_the_reference_and_the_restatement(renderer, sfx):
    """poseopt.npz, shared and per-pose rest poses: the four outputs, pelvis.grad and bones.grad at the fp32 rule against the
    reference's values and against the float64 restatement; `bones` is bone[inverse_idxs] bitwise."""
    g = load_golden("poseopt")
    pelvis, bones, rest = g[f"pelvis{sfx}"], g[f"bones_param{sfx}"], g[f"rest_pose{sfx}"]
    ridx = g["rest_pose_idxs_pp"] if sfx else None
    cot = {k: g[f"d_{k}"] for k in OUTS}
    layer = _layer(renderer, pelvis, bones, rest, ridx)
    got, gb, gp = _step(layer, g["idxs"], cot)
    want, wb, wp = _restated(pelvis, bones, rest, g["idxs"], cot, rest_pose_idxs=ridx)
    for k in OUTS:
        assert got[k].dtype == np.float32
        ref.check_rule(got[k], g[f"{k}{sfx}"], f"{k}{sfx} against the reference")
        ref.check_rule(got[k], want[k], f"{k}{sfx} against the float64 restatement", own32=lambda k=k: g[f"{k}{sfx}"])
    assert np.array_equal(got["bones"], bones[np.unique(g["idxs"], return_inverse=True)[0]][np.unique(g["idxs"], return_inverse=True)[1]])
    assert np.array_equal(got["bones"], g[f"bones{sfx}"])
    for what, a, r32, r64 in (("bones.grad", gb, g[f"bones_grad{sfx}"], wb), ("pelvis.grad", gp, g[f"pelvis_grad{sfx}"], wp)):
        ref.check_rule(a, r32, f"{what}{sfx} against the reference's autograd")
        ref.check_rule(a, r64, f"{what}{sfx} against the float64 restatement", own32=lambda r32=r32: r32)
    # the skts / l2ws rows the kernels do not compute
    assert (got["skts"][..., 3, :] == np.array([0, 0, 0, 1], dtype=np.float32)).all()
    assert (got["l2ws"][..., 3, :] == np.array([0, 0, 0, 1], dtype=np.float32)).all()


# ---- shapes where the kernels can go wrong --------------------------------------------------------------------------------------
SHAPES = {
    "one": dict(U=1, idxs=[0]),
    "unsorted": dict(U=3, idxs=[2, 0, 2, 1, 0, 2, 1, 2]),
    "long_segment": dict(U=2, idxs=[0] * 130 + [1] + [0] * 126),                   # n = 257: a segment longer than a workgroup
    "reverse65": dict(U=65, idxs=list(range(64, -1, -1))),                          # more poses than a wave, no ray on its own pose
    "per_pose_rest": dict(U=5, idxs=[4, 1, 4, 0, 3, 3, 1], pp=True),
    "sparse": dict(U=9, idxs=[8, 2, 8, 5]),                                         # poses of the layer that no ray reads
}


@pytest.mark.parametrize("key", list(SHAPES))
def test_shapes_against_the_restatement(renderer, key):
    s = SHAPES[key]
    c = random_case(s["U"], s["idxs"], s.get("pp", False), seed=11)
    layer = _layer(renderer, c["pelvis"], c["bones"], c["rest"], np.arange(s["U"]) if s.get("pp") else None)
    got, gb, gp = _step(layer, c["idxs"], c["cot"])
    want, wb, wp = _restated(c["pelvis"], c["bones"], c["rest"], c["idxs"], c["cot"])
    own = {}

    def own32(k):
        if not own:
            o, b, p = _torch32(c["pelvis"], c["bones"], c["rest"], c["idxs"], c["cot"])
            own.update(o, bones_grad=b, pelvis_grad=p)
        return own[k]
    for k in OUTS:
        ref.check_rule(got[k], want[k], f"[{key}] {k}", own32=lambda k=k: own32(k))
    ref.check_rule(gb, wb, f"[{key}] bones.grad", own32=lambda: own32("bones_grad"))
    ref.check_rule(gp, wp, f"[{key}] pelvis.grad", own32=lambda: own32("pelvis_grad"))
    assert np.abs(wb).max() > 0 and np.abs(wp).max() > 0


@pytest.mark.parametrize("only", OUTS)
def test_each_cotangent_alone(renderer, only):
    """One output in the loss: the other three cotangents reach the library as NULL."""
    s = SHAPES["unsorted"]
    c = random_case(s["U"], s["idxs"], seed=12)
    layer = _layer(renderer, c["pelvis"], c["bones"], c["rest"])
    _, gb, gp = _step(layer, c["idxs"], c["cot"], only=(only,))
    _, wb, wp = _restated(c["pelvis"], c["bones"], c["rest"], c["idxs"], c["cot"], only=(only,))
    t32 = lambda i: _torch32(c["pelvis"], c["bones"], c["rest"], c["idxs"], c["cot"], only=(only,))[i]
    ref.check_rule(gb, wb, f"[{only} alone] bones.grad", own32=lambda: t32(1))
    if only == "rots":                                     # (the rotations do not read the pelvis)
        assert (gp == 0).all() and (wp == 0).all()
    else:
        ref.check_rule(gp, wp, f"[{only} alone] pelvis.grad", own32=lambda: t32(2))


def _abi_args(renderer, c, dev=DEV):
    """device tensors and host index arrays of a direct ABI call on the case c"""
    from posegen_amd.poseopt import ray_segments
    seg = ray_segments(c["idxs"])
    t = lambda a: torch.tensor(np.ascontiguousarray(a), device=dev)
    d = dict(bones=t(c["bones"][seg.unique]), pelvis=t(c["pelvis"][seg.unique]), rest=t(c["rest"]), seg=seg,
             parents=np.ascontiguousarray(ref.PARENTS, dtype=np.int32), U=len(seg.unique), n=len(seg.inverse))
    d["cot"] = {k: t(v) for k, v in c["cot"].items()}
    return d


def _backward_call(renderer, a, cot=(None, None, None, None), rot_dim=6, rest_stride=0, parents=None, seg_start=None, seg_rays=None,
                   fill=float("nan")):
    r = renderer
    p = lambda x: None if x is None else C.c_void_p(x.data_ptr())
    i = lambda x: x.ctypes.data_as(_I32P)
    db = torch.full((a["U"], 24, 6), fill, device=DEV)
    dp = torch.full((a["U"], 3), fill, device=DEV)
    keep = [np.ascontiguousarray(x, dtype=np.int32) for x in (a["parents"] if parents is None else parents,
                                                              a["seg"].seg_start if seg_start is None else seg_start,
                                                              a["seg"].seg_rays if seg_rays is None else seg_rays)]
    rc = r.lib.pg_poseopt_backward(r.handle, r._stream(), a["U"], rot_dim, p(a["bones"]), p(a["pelvis"]), p(a["rest"]), rest_stride,
                                   i(keep[0]), a["n"], i(keep[1]), i(keep[2]), *[p(x) for x in cot], p(db), p(dp))
    torch.cuda.synchronize()
    return rc, db.cpu().numpy(), dp.cpu().numpy()


def test_no_cotangent_gives_zero_gradients(renderer):
    s = SHAPES["unsorted"]
    a = _abi_args(renderer, random_case(s["U"], s["idxs"], seed=13))
    rc, db, dp = _backward_call(renderer, a)
    assert rc == 0 and (db == 0).all() and (dp == 0).all()


# ---- repeatable, and the order of the rays matters by rounding only ----------------------------------------------------------------
def test_backward_is_bitwise_repeatable_and_ray_order_is_rounding(renderer):
    """Two backward calls give the same bytes.  The batch in another order (every pose keeps its multiset of rays, the cotangents
    move with their rays) changes the sums' order only: the gradients move by rounding, far inside the rule."""
    U, n = 7, 300
    rng = np.random.RandomState(5)
    idxs = rng.randint(0, U, n)
    c = random_case(U, idxs, seed=14)
    layer = _layer(renderer, c["pelvis"], c["bones"], c["rest"])
    _, b1, p1 = _step(layer, idxs, c["cot"])
    _, b2, p2 = _step(layer, idxs, c["cot"])
    assert b1.tobytes() == b2.tobytes() and p1.tobytes() == p2.tobytes()
    perm = rng.permutation(n)
    _, b3, p3 = _step(layer, idxs[perm], {k: v[perm] for k, v in c["cot"].items()})
    eb, _ = ref.check_rule(b3, b1, "bones.grad after permuting the batch")
    ep, _ = ref.check_rule(p3, p1, "pelvis.grad after permuting the batch")
    assert eb <= 1e-6 and ep <= 1e-6, "float64 sums rounded once: a permutation moves the last float32 bit at the most"


# ---- the refusals of the ABI ------------------------------------------------------------------------------------------------------
def test_abi_refusals_launch_nothing(renderer):
    """Every PG_EINVAL of the header comes back as PgError and leaves the outputs as they were."""
    from posegen_amd import _ffi
    s = SHAPES["unsorted"]
    a = _abi_args(renderer, random_case(s["U"], s["idxs"], seed=15))
    U, n, seg = a["U"], a["n"], a["seg"]
    r = renderer
    p = lambda x: None if x is None else C.c_void_p(x.data_ptr())
    i = lambda x: None if x is None else x.ctypes.data_as(_I32P)

    def fwd(rot_dim=6, rest_stride=0, parents=a["parents"], ray_pose=seg.inverse, n_rays=n):
        out = torch.full((n, 24, 4, 4), 7.0, device=DEV)
        parents = np.ascontiguousarray(parents, dtype=np.int32)
        ray_pose = None if ray_pose is None else np.ascontiguousarray(ray_pose, dtype=np.int32)
        rc = r.lib.pg_poseopt_forward(r.handle, r._stream(), U, rot_dim, p(a["bones"]), p(a["pelvis"]), p(a["rest"]), rest_stride,
                                      i(parents), n_rays, i(ray_pose), None, None, p(out), None)
        torch.cuda.synchronize()
        return rc, out.cpu().numpy()

    def refused(rc, *outs):
        with pytest.raises(_ffi.PgError) as e:
            r._check(rc)
        assert e.value.code == _ffi.PG_EINVAL
        for o in outs:
            assert (o == 7.0).all(), "a refused call wrote its outputs"

    rc, out = fwd()
    assert rc == 0 and not (out == 7.0).any()
    bad_parent = a["parents"].copy(); bad_parent[5] = 5
    late_parent = a["parents"].copy(); late_parent[3] = 9
    for kw in (dict(rot_dim=3), dict(rest_stride=24), dict(parents=bad_parent), dict(parents=late_parent),
               dict(ray_pose=np.where(np.arange(n) == 2, U, seg.inverse)), dict(ray_pose=np.where(np.arange(n) == 4, -1, seg.inverse)),
               dict(ray_pose=None)):
        refused(*fwd(**kw))
    cot = tuple(a["cot"][k] for k in ("rots", "l2ws", "skts", "kps"))
    rc, db, dp = _backward_call(r, a, cot, fill=7.0)
    assert rc == 0 and not (db == 7.0).any()
    ss, sr = seg.seg_start, seg.seg_rays
    not_from_0 = ss.copy(); not_from_0[0] = 1
    not_to_n = ss.copy(); not_to_n[-1] = n - 1
    not_monotone = ss.copy(); not_monotone[1], not_monotone[2] = ss[2], ss[1]
    past_n = ss.copy(); past_n[1] = n + 3
    twice = sr.copy(); twice[1] = twice[0]
    outside = sr.copy(); outside[3] = n
    descending = sr.copy(); descending[[0, 1]] = descending[[1, 0]]
    assert ss[1] - ss[0] >= 2
    for kw in (dict(rot_dim=3), dict(rest_stride=5), dict(parents=bad_parent), dict(seg_start=not_from_0), dict(seg_start=not_to_n),
               dict(seg_start=not_monotone), dict(seg_start=past_n), dict(seg_rays=twice), dict(seg_rays=outside), dict(seg_rays=descending)):
        rc, db, dp = _backward_call(r, a, cot, fill=7.0, **kw)
        refused(rc, db, dp)


# ---- in front of the training step ------------------------------------------------------------------------------------------------
def _train_caster(cfg, weights):
    from posegen_amd.raycaster import HipRayCaster
    from posegen_amd.train import TrainableRayCaster
    wc, wf, tv, td = weights
    m = TrainableRayCaster(HipRayCaster.from_weights(cfg, wc, wf, float(tv), float(td), device=DEV, precision="fp32"),
                           train_precision="fp32", opt_pose=True)
    m.train()
    return m


def _pose_params(g):
    """parameters of a pose layer whose poses are the fixture's two frames (SURREAL rest pose, pelvis = the root key point)"""
    from posegen_amd.poseopt import axisang_to_rot6d
    from posegen_amd.skeleton import SURREAL_REST_SCALE, smpl_rest_pose
    rest = (smpl_rest_pose * SURREAL_REST_SCALE).astype(np.float32)[None]
    return g["kps"][:, 0].copy(), axisang_to_rot6d(g["bones"]), rest


def test_layer_in_front_of_the_training_step():
    """train_grads_pose (two frames by kp_idx): HipPoseOptLayer -> TrainableRayCaster(opt_pose=True) -> loss_of -> backward against the
    same step with the torch fp32 restatement layer on the device: pelvis.grad / bones.grad within the rule.  The layer does not
    disturb the network gradients: they are bitwise those of the step that reads the layer's skts VALUES from a plain leaf tensor.
    (Bitwise equality with the torch layer's step itself cannot hold and is not asserted: the two layers' skts differ in the last
    float32 bit -- float64 rounded once here, a float32 chain and LU inverse there -- and the step's gradients follow their
    inputs.  Measured on MI355X: 0 of 48 tensors bitwise equal, every one within 5.2e-6 of its scale; that comparison is held to
    the fp32 rule instead and the count is printed.)"""
    from tests.helpers import golden_draws
    g = load_golden("train_grads_pose")
    cfg = cfg_from_golden(g)
    m = _train_caster(cfg, model_for(cfg, int(g["seed_model"])))
    pelvis, bones, rest = _pose_params(g)
    kp_idx = g["kp_idx"]
    rb, cy, target = torch.tensor(g["ray_batch"]), torch.tensor(g["cyl"][kp_idx]), torch.tensor(g["target"], device=DEV)

    def step(skts, layer=None):
        for p_ in m.parameters():
            p_.grad = None
        out = m(rb, N_samples=cfg.n_samples, skts=skts, cyls=cy, N_importance=cfg.n_importance, draws=golden_draws(g))
        loss = loss_of(out, target)
        loss.backward()
        nets = {(tag, k): p_.grad.detach().clone() for tag, net in (("coarse", m.network), ("fine", m.network_fine))
                for k, p_ in net.named_parameters()}
        return float(loss.detach()), nets

    hip = _layer(m.renderer, pelvis, bones, rest)
    skts_hip = hip(kp_idx)[2]
    np.testing.assert_allclose(skts_hip.detach().cpu().numpy(), g["skts"][kp_idx], atol=2e-6)      # the fixture's poses
    loss_h, nets_h = step(skts_hip)
    tl = ref.TorchPoseOptLayer(pelvis, bones, rest, device=DEV)
    loss_t, nets_t = step(tl(kp_idx)[2])
    assert abs(loss_h - loss_t) <= 1e-5 * max(1.0, abs(loss_t))
    for what, a, b in (("pelvis.grad", hip.pelvis.grad, tl.pelvis.grad), ("bones.grad", hip.bones.grad, tl.bones.grad)):
        assert float(b.abs().max()) > 0
        ref.check_rule(a.cpu().numpy(), b.cpu().numpy(), f"{what} against the torch fp32 layer's step")
    same = sum(int(torch.equal(nets_h[k], nets_t[k])) for k in nets_h)
    print(f"network gradients bitwise equal to the torch layer's step: {same} of {len(nets_h)} tensors")
    for k in nets_h:
        ref.check_rule(nets_h[k].cpu().numpy(), nets_t[k].cpu().numpy(), f"{k} against the torch layer's step")
    _, nets_leaf = step(skts_hip.detach().clone().requires_grad_(True))
    assert len(nets_leaf) == 48
    for k in nets_h:
        assert torch.equal(nets_h[k], nets_leaf[k]), k
    m.renderer.close()


def test_pose_layer_adam_loop_follows_the_restatement():
    """10 Adam steps on the layer's pelvis and bones (the nets outside the optimiser) over train_grads_pose's rays, the targets rendered
    by the float64 oracle from displaced parameters: the HIP loop's loss stays within 1e-6 (relative to max(1, loss)) of the loop of
    the float64 restatement layer in front of the float64 oracle at every step, and falls."""
    from oracle import anerf_oracle as orc
    g = load_golden("train_grads_pose")
    cfg = cfg_from_golden(g)
    weights = model_for(cfg, int(g["seed_model"]))
    wc, wf, tv, td = weights
    pelvis, bones, rest = _pose_params(g)
    kp_idx = g["kp_idx"]
    rb, cy = g["ray_batch"], g["cyl"][kp_idx]
    S, N = cfg.n_samples, cfg.n_importance
    ocfg = oracle_cfg(cfg, tv, td)
    rng = np.random.RandomState(3)
    pelvis_true = pelvis + rng.normal(0, 0.02, pelvis.shape).astype(np.float32)
    bones_true = bones + rng.normal(0, 0.03, bones.shape).astype(np.float32)

    def oracle_step(dtype):
        def step(sk, tg):
            with default_dtype(dtype):
                nets = [{k: torch.tensor(v, dtype=dtype) for k, v in w.items()} for w in (wc, wf)]
                out = orc.render_rays(torch.tensor(rb, dtype=dtype), sk, torch.tensor(cy, dtype=dtype), ocfg, nets[0], nets[1], S, N)
                return loss_of(out, tg)
        return step

    with default_dtype(torch.float64), torch.no_grad():
        sk_t = ref.TorchPoseOptLayer(pelvis_true, bones_true, rest, dtype=torch.float64)(kp_idx)[2]
        nets64 = [{k: torch.tensor(v, dtype=torch.float64) for k, v in w.items()} for w in (wc, wf)]
        t = orc.render_rays(torch.tensor(rb, dtype=torch.float64), sk_t, torch.tensor(cy, dtype=torch.float64), ocfg, nets64[0], nets64[1], S, N)
        target = (t["rgb_map"] + (1 - t["acc_map"])[..., None]).detach()

    def loop(layer, step, dtype):
        opt = torch.optim.Adam([layer.pelvis, layer.bones], lr=2e-3)
        losses = []
        for _ in range(10):
            opt.zero_grad()
            loss = step(layer(kp_idx)[2], target.to(dtype))
            loss.backward()
            opt.step()
            losses.append(float(loss.detach()))
        return np.array(losses)

    m = _train_caster(cfg, weights)
    hip_step = lambda sk, tg: loss_of(m(torch.tensor(rb), N_samples=S, skts=sk, cyls=torch.tensor(cy), N_importance=N), tg.to(DEV))
    hip = loop(_layer(m.renderer, pelvis, bones, rest), hip_step, torch.float32)
    want = loop(ref.TorchPoseOptLayer(pelvis, bones, rest, dtype=torch.float64), oracle_step(torch.float64), torch.float64)
    dev = np.abs(hip - want) / np.maximum(1.0, np.abs(want))
    tol = np.full(10, 1e-6)
    if (dev > tol).any():
        own = np.abs(loop(ref.TorchPoseOptLayer(pelvis, bones, rest), oracle_step(torch.float32), torch.float32) - want) / np.maximum(1.0, np.abs(want))
        tol = np.maximum(tol, 4.0 * own)
        print(f"pose layer loop: the fp32 restatement's own deviation per step, largest {own.max():.2e}")
    print("pose layer loop losses (HIP):", " ".join(f"{v:.7f}" for v in hip))
    print(f"pose layer loop: largest deviation from the float64 loop {dev.max():.2e}")
    assert (dev <= tol).all(), (dev, tol)
    assert hip[-1] < hip[0] and want[-1] < want[0]
    m.renderer.close()
