"""pg_smpl_forward, pg_vertex_errors and pg_pose_kinematics_rot on the GPU, through the C ABI and through posegen_amd.smpl /
pose_eval / ganloop, against the float64 restatement (tests/smpl_ref.py) and the reference's own values (tests/golden/smpl_body.npz).

Bounds: those of tests/test_smpl_ref.py (u = 2^-24, mag from the restatement).  Vertices n u mag with n = (1 + NB + 207) + 24 + 4 + 8;
regressed joints (n + ceil(V / 4)) u mag -- built: float32 within one MFMA (4 vertices), double across; posed joints and key points
one float32 ulp + 9 u mag; pg_vertex_errors and what comes out of PoseScorer 1e-10 max(1, |value|), the scores as functions of
the float32 key points and vertices the device produced.

Largest observed error / bound on the MI355X (this module's printed ratios; nothing is set from them): vertices 0.050 (V = 6890),
posed joints 0.089, regressed joints 0.012, key points of pg_pose_kinematics_rot 0.087."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

from posegen_amd import _ffi, ganloop, pose_eval as pe, smpl, synthetic
from tests import pose_scores_ref as psr
from tests import smpl_ref as ref
from tests.frame_metrics_gpu import DEV, renderer  # noqa: F401 (renderer: a fixture)

pytestmark = pytest.mark.gpu
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = np.load(os.path.join(REPO, "tests", "golden", "smpl_body.npz"))
EINVAL = -1
SENTINEL = -7.0
_models, _bodies = {}, {}


def model_of(V, NB, K, seed=3):
    key = (V, NB, K, seed)
    if key not in _models:
        _models[key] = synthetic.make_body_model(V, NB=NB, seed=seed, regress_rows=(K,) if K else ())
    return _models[key]


def body_of(renderer, V, NB, K, seed=3):
    key = (V, NB, K, seed)
    if key not in _bodies:
        _bodies[key] = smpl.BodyModel.from_arrays(renderer, model_of(V, NB, K, seed))
    return _bodies[key]


def make_inputs(B, NB, seed):
    """betas in [-3, 3], poses with angles up to 1.5 about random axes (pose 0 at rest), and the matrices of those poses"""
    rng = np.random.RandomState(seed)
    betas = rng.uniform(-3.0, 3.0, size=(B, NB)).astype(np.float32)
    axes = rng.randn(B, 24, 3)
    axes /= np.linalg.norm(axes, axis=-1, keepdims=True)
    pose = (axes * rng.uniform(0.2, 1.5, size=(B, 24, 1))).astype(np.float32)
    pose[0] = 0.0
    return betas, pose, ref.rodrigues(pose.reshape(-1, 3)).reshape(B, 24, 3, 3).astype(np.float32)


def abi(r, body, betas, pose, rotmat=False, K=None, B=None, stride=None, null=(), struct=None, regress="own"):
    """pg_smpl_forward through the C ABI -> (return code, dict of numpy outputs).  Every output starts filled with SENTINEL and has
    one guard element behind it; `null`: names passed as NULL; `struct`: a pg_body_model to pass instead of the body's."""
    Bv, V = pose.shape[0], body.V
    reg = next(iter(body.regressors.values())) if body.regressors else None
    Kv = (0 if reg is None else reg.shape[0]) if K is None else K
    Kout = max(min(Kv, 64), 1)
    new = lambda n: torch.full((n + 1,), SENTINEL, dtype=torch.float32, device=DEV)
    out = {"verts": new(Bv * V * 3), "joints": new(Bv * 72), "regressed": new(Bv * Kout * 3)}
    d_betas, d_pose = torch.from_numpy(betas).to(DEV), torch.from_numpy(pose).to(DEV)
    ptr = lambda name, t: None if (name in null or t is None) else C.c_void_p(t.data_ptr())
    rc = r.lib.pg_smpl_forward(r.handle, r._stream(), None if "model" in null else C.byref(body._model if struct is None else struct),
                               Bv if B is None else B, ptr("betas", d_betas), (body.NB if betas.shape[0] == Bv else 0) if stride is None else stride,
                               ptr("pose", d_pose), int(rotmat), ptr("regress", reg if regress == "own" else regress), Kv,
                               ptr("verts", out["verts"]), ptr("joints", out["joints"]), ptr("regressed", out["regressed"]))
    torch.cuda.synchronize()
    host = {k: v.cpu().numpy() for k, v in out.items()}
    for k, v in host.items():
        assert v[-1] == SENTINEL, f"{k}: the element behind the output was written"
        if rc != 0 or k in null:
            assert (v == SENTINEL).all(), f"{k}: written though refused or not asked for"
    if rc == 0:
        host = {"verts": host["verts"][:-1].reshape(Bv, V, 3), "joints": host["joints"][:-1].reshape(Bv, 24, 3),
                "regressed": host["regressed"][:-1].reshape(Bv, Kout, 3)}
    return rc, host


def check(got, want, NB, V, what, null=()):
    """every output that was asked for against the restatement `want`, within the bounds; returns the error / bound ratios"""
    ratios = {}
    if "verts" not in null:
        ratios["verts"] = np.max(np.abs(got["verts"] - want["verts"]) / ref.bound_verts(want, NB))
    if "joints" not in null:
        ratios["joints"] = np.max(np.abs(got["joints"] - want["joints"]) / ref.bound_chain(want["joints"], want["mag_joints"]))
    if "regressed" not in null and "regressed" in want:
        ratios["regressed"] = np.max(np.abs(got["regressed"] - want["regressed"]) / ref.bound_regressed(want, NB, V))
    print(what, "error / bound:", {k: round(float(v), 4) for k, v in ratios.items()})
    assert all(v <= 1 for v in ratios.values()), (what, ratios)
    return ratios


# ---- the fixture's model ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("K", [17, 9])
@pytest.mark.parametrize("form", ["axis", "rotmat"])
def test_fixture_model_against_restatement_and_reference(renderer, form, K):
    V, NB, seed = int(GOLD["V"]), int(GOLD["NB"]), int(GOLD["seed"])
    model = synthetic.make_body_model(V, NB=NB, seed=seed, regress_rows=(17, 9))
    body = smpl.BodyModel(renderer, *(model[k] for k in smpl.MODEL_KEYS), regressors={"k": model[f"regressor_{K}"]})
    pose, sfx = (GOLD["pose"], "") if form == "axis" else (GOLD["rotmat"], "_rotmat")
    want = ref.lbs(model, GOLD["betas"], pose, pose2rot=form == "axis", regress=model[f"regressor_{K}"])
    rc, got = abi(renderer, body, GOLD["betas"], pose, rotmat=form == "rotmat")
    assert rc == 0
    check(got, want, NB, V, f"fixture {form} K={K}")
    # the reference's own float32 values, within the same bounds
    assert np.all(np.abs(got["verts"] - ref.f64(GOLD["verts" + sfx])) <= ref.bound_verts(want, NB))
    assert np.all(np.abs(got["regressed"] - ref.f64(GOLD[f"regressed_{K}{sfx}"])) <= ref.bound_regressed(want, NB, V))
    # through posegen_amd.smpl: the same bytes
    out = body.forward(GOLD["betas"], pose, pose2rot=form == "axis", regressor="k", want_vertices=True)
    assert np.array_equal(out.vertices.cpu().numpy(), got["verts"]) and np.array_equal(out.joints.cpu().numpy(), got["joints"])
    assert np.array_equal(out.regressed.cpu().numpy(), got["regressed"])
    if form == "axis":
        go = body.forward(GOLD["betas"], global_orient=GOLD["pose"][:, :1].reshape(-1, 3), body_pose=GOLD["pose"][:, 1:].reshape(-1, 69))
        assert go.vertices is None and go.regressed is None and np.array_equal(go.joints.cpu().numpy(), got["joints"])


# ---- tails in every direction -----------------------------------------------------------------------------------------------------------
TAILS = [(1, 1, 0, 1), (1, 5, 1, 10), (1, 67, 64, 16), (7, 1, 64, 10), (7, 5, 17, 10), (7, 67, 9, 16), (431, 1, 1, 16), (431, 5, 0, 10),
         (431, 67, 64, 1), (431, 67, 17, 10)]


@pytest.mark.parametrize("V,B,K,NB", TAILS)
def test_tails(renderer, V, B, K, NB):
    model, body = model_of(V, NB, K), body_of(renderer, V, NB, K)
    betas, pose, rot = make_inputs(B, NB, 10 * V + B)
    null = ("regressed",) if K == 0 else ()
    for form, p in (("axis", pose), ("rotmat", rot)):
        want = ref.lbs(model, betas, p, pose2rot=form == "axis", regress=model[f"regressor_{K}"] if K else None)
        rc, got = abi(renderer, body, betas, p, rotmat=form == "rotmat", null=null)
        assert rc == 0
        check(got, want, NB, V, f"V={V} B={B} K={K} NB={NB} {form}", null=null)


@pytest.mark.parametrize("skip", ["verts", "joints", "regressed"])
def test_each_output_null_in_turn(renderer, skip):
    V, B, K, NB = 431, 5, 9, 10
    model, body = model_of(V, NB, K), body_of(renderer, V, NB, K)
    betas, pose, _ = make_inputs(B, NB, 77)
    want = ref.lbs(model, betas, pose, regress=model[f"regressor_{K}"])
    rc, full = abi(renderer, body, betas, pose)
    rc2, got = abi(renderer, body, betas, pose, null=(skip,), K=0 if skip == "regressed" else None)
    assert rc == 0 and rc2 == 0
    check(got, want, NB, V, f"without {skip}", null=(skip,))
    for k in ("verts", "joints", "regressed"):
        if k != skip:
            assert np.array_equal(got[k], full[k]), k          # what is written does not depend on what else is


# ---- at size --------------------------------------------------------------------------------------------------------------------------------
def test_at_size(renderer):
    V, B, K, NB = 6890, 33, 17, 10
    model, body = model_of(V, NB, K, seed=0), body_of(renderer, V, NB, K, seed=0)
    betas, pose, _ = make_inputs(B, NB, 5)
    want = ref.lbs(model, betas, pose, regress=model[f"regressor_{K}"])
    rc, got = abi(renderer, body, betas, pose)
    assert rc == 0
    check(got, want, NB, V, "V=6890 with verts")
    rc, lean = abi(renderer, body, betas, pose, null=("verts",))
    assert rc == 0
    check(lean, want, NB, V, "V=6890 without verts", null=("verts",))
    assert np.array_equal(lean["regressed"], got["regressed"]) and np.array_equal(lean["joints"], got["joints"])


# ---- invariants -----------------------------------------------------------------------------------------------------------------------------
def test_bitwise_invariants(renderer):
    V, B, K, NB = 431, 67, 17, 10
    body = body_of(renderer, V, NB, K)
    betas, pose, _ = make_inputs(B, NB, 9)
    rc, a = abi(renderer, body, betas, pose)
    rc2, b = abi(renderer, body, betas, pose)
    assert rc == 0 and rc2 == 0
    for k in a:
        assert np.array_equal(a[k], b[k]), f"{k}: two calls differ"
    for at in (0, 31, 66):                                       # a pose alone = the pose in its batch
        rc, one = abi(renderer, body, betas[at:at + 1], pose[at:at + 1], stride=NB)
        assert rc == 0
        for k in a:
            assert np.array_equal(one[k][0], a[k][at]), f"{k}: pose {at} alone differs from pose {at} of {B}"
    same = np.repeat(betas[3:4], B, axis=0)
    rc, wide = abi(renderer, body, same, pose)
    rc2, one_row = abi(renderer, body, same[:1], pose, stride=0)
    assert rc == 0 and rc2 == 0
    for k in a:
        assert np.array_equal(wide[k], one_row[k]), f"{k}: betas_stride = 0 differs from the expanded betas"
    out = body.forward(same[:1], pose, regressor=str(K), want_vertices=True)           # one row broadcasts in Python too
    assert np.array_equal(out.vertices.cpu().numpy(), wide["verts"])


@pytest.mark.parametrize("where", ["pose", "betas"])
def test_nan_stays_in_its_pose(renderer, where):
    V, B, K, NB = 431, 67, 17, 10
    body = body_of(renderer, V, NB, K)
    betas, pose, _ = make_inputs(B, NB, 9)
    rc, clean = abi(renderer, body, betas, pose)
    bad_b, bad_p = betas.copy(), pose.copy()
    if where == "pose":
        bad_p[40, 7, 1] = np.nan
    else:
        bad_b[40, 2] = np.nan
    rc2, got = abi(renderer, body, bad_b, bad_p)
    assert rc == 0 and rc2 == 0
    keep = np.arange(B) != 40
    for k in clean:
        assert np.array_equal(got[k][keep], clean[k][keep]), f"{k}: a NaN in pose 40 changed another pose"
        assert not np.isfinite(got[k][40]).all(), k
    assert np.isnan(got["verts"][40]).all() and np.isnan(got["regressed"][40]).all()


# ---- refusals -------------------------------------------------------------------------------------------------------------------------------
def test_einval_writes_nothing(renderer):
    V, B, K, NB = 7, 5, 9, 10
    body = body_of(renderer, V, NB, K)
    betas, pose, _ = make_inputs(B, NB, 1)

    def struct(**changed):
        m = body._model
        s = _ffi.PgBodyModel(V=m.V, NB=m.NB, blend=m.blend, skin=m.skin, rest_joints=m.rest_joints, parents=(C.c_int32 * 24)(*m.parents))
        for k, v in changed.items():
            if k == "parents":
                s.parents = (C.c_int32 * 24)(*v)
            else:
                setattr(s, k, v)
        return s

    par = list(body._model.parents)
    cases = {
        "model NULL": dict(null=("model",)), "betas NULL": dict(null=("betas",)), "pose NULL": dict(null=("pose",)),
        "all outputs NULL": dict(null=("verts", "joints", "regressed")), "B = 0": dict(B=0), "B < 0": dict(B=-3),
        "NB = 0": dict(struct=struct(NB=0)), "NB = 17": dict(struct=struct(NB=17)), "V = 0": dict(struct=struct(V=0)),
        "V too large": dict(struct=struct(V=(2 ** 31) // ((1 + NB + 207) * 3) + 1)), "K = -1": dict(K=-1), "K = 65": dict(K=65),
        "K > 0, regress NULL": dict(null=("regress",)), "regressed with K = 0": dict(K=0),
        "parents[0] = 0": dict(struct=struct(parents=[0] + par[1:])),
        "a child before its parent": dict(struct=struct(parents=par[:5] + [7] + par[6:])),
        "a negative parent": dict(struct=struct(parents=par[:9] + [-1] + par[10:])),
    }
    for name, kw in cases.items():
        rc, _ = abi(renderer, body, betas, pose, **kw)            # (abi asserts that every sentinel is intact)
        assert rc == EINVAL, name
    rc, _ = abi(renderer, body, betas, pose)                      # and the handle still works
    assert rc == 0


# ---- mesh errors ----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("B,V", [(1, 1), (5, 7), (67, 431), (300, 65)])
def test_vertex_errors(renderer, B, V):
    rng = np.random.RandomState(B + V)
    a, b = rng.randn(B, V, 3).astype(np.float32), rng.randn(B, V, 3).astype(np.float32)
    da, db = torch.from_numpy(a).to(DEV), torch.from_numpy(b).to(DEV)
    per_pose = torch.full((B + 1,), SENTINEL, dtype=torch.float64, device=DEV)
    summary = torch.full((3,), SENTINEL, dtype=torch.float64, device=DEV)
    rc = renderer.lib.pg_vertex_errors(renderer.handle, renderer._stream(), B, V, C.c_void_p(da.data_ptr()), C.c_void_p(db.data_ptr()),
                                       C.c_void_p(per_pose.data_ptr()), C.c_void_p(summary.data_ptr()))
    torch.cuda.synchronize()
    want_pp, want_mean = ref.vertex_errors(a, b)
    pp, s = per_pose.cpu().numpy(), summary.cpu().numpy()
    assert rc == 0 and pp[-1] == SENTINEL and s[-1] == SENTINEL and s[0] == B
    assert np.all(np.abs(pp[:-1] - want_pp) <= 1e-10 * np.maximum(1, np.abs(want_pp))) and abs(s[1] - want_mean) <= 1e-10 * max(1, abs(want_mean))
    got_pp, got_mean = smpl.vertex_errors(renderer, da, db)
    assert np.array_equal(got_pp.cpu().numpy(), pp[:-1]) and float(got_mean) == s[1]
    if B > 1:                                                      # a NaN stays in its pose; the mean propagates it
        a[1, V // 2, 0] = np.nan
        got_pp, got_mean = smpl.vertex_errors(renderer, a, b)
        got_pp = got_pp.cpu().numpy()
        assert np.isnan(got_pp[1]) and np.isnan(float(got_mean)) and np.array_equal(np.delete(got_pp, 1), np.delete(pp[:-1], 1))
    for kw in (dict(B=0), dict(V=0)):
        args = dict(B=B, V=V)
        args.update(kw)
        assert renderer.lib.pg_vertex_errors(renderer.handle, renderer._stream(), args["B"], args["V"], C.c_void_p(da.data_ptr()),
                                             C.c_void_p(db.data_ptr()), C.c_void_p(per_pose.data_ptr()), None) == EINVAL
    assert renderer.lib.pg_vertex_errors(renderer.handle, renderer._stream(), B, V, None, C.c_void_p(db.data_ptr()),
                                         C.c_void_p(per_pose.data_ptr()), None) == EINVAL


# ---- kinematics from rotation matrices ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("F", [1, 5, 67])
def test_pose_kinematics_rot(renderer, F):
    from posegen_amd.skeleton import smpl_rest_pose
    bones = synthetic.make_bones(F, seed=F, sigma=0.5)
    rot = ref.axisang_to_rot(bones)
    rest = smpl_rest_pose.astype(np.float32)
    l2ws_w, kps_w, mag = ref.rot_chain(rot, rest, scale=0.4)
    kps, skts, l2ws = renderer.pose_kinematics_rot(torch.from_numpy(rot), rest, scale=0.4, want_l2ws=True)
    kps, skts, l2ws = kps.cpu().numpy(), skts.cpu().numpy(), l2ws.cpu().numpy()
    bound = ref.bound_chain(kps_w, mag)
    print("key points error / bound", float(np.max(np.abs(kps - kps_w) / bound)))
    assert np.all(np.abs(kps - kps_w) <= bound)
    assert np.abs(l2ws - l2ws_w).max() <= 1e-12
    inv = np.zeros_like(l2ws_w)                                    # skt = [R^T | -R^T t], the rigid inverse as pg_pose_kinematics forms it
    inv[..., :3, :3] = np.swapaxes(l2ws_w[..., :3, :3], -1, -2)
    inv[..., :3, 3] = -np.einsum("fjcr,fjc->fjr", l2ws_w[..., :3, :3], l2ws_w[..., :3, 3])
    inv[..., 3, 3] = 1.0
    assert np.all(np.abs(skts - inv) <= np.spacing(np.abs(inv).astype(np.float32)) + 1e-12)
    # pg_pose_kinematics fed the axis-angle vectors the matrices came from: its own float32 rounding on top of the chain bound
    rest_scaled = rest * np.float32(0.4)
    kps_aa = renderer.pose_kinematics(torch.from_numpy(bones), rest_scaled)[0].cpu().numpy()
    assert np.all(np.abs(kps - kps_aa) <= bound + np.spacing(np.abs(kps_aa)))
    # the GAN loop's feedback (run_gan.py:2081-2091): key points of the regressor's matrices into 1 - mpjpe
    gt = synthetic.make_pose(F, seed=F + 1)[1] * np.float32(0.4 / 0.714)
    pred = ganloop.regressor_keypoints(renderer, torch.from_numpy(rot).to(DEV))
    assert np.array_equal(pred.cpu().numpy(), kps)
    loss = float(ganloop.regressor_feedback(pred, torch.from_numpy(gt).to(DEV), scorer=pe.PoseScorer(renderer)))
    want = 1.0 - psr.per_pose(kps, gt, joints=psr.GAN_JOINTS, root=0, align=psr.ALIGN_NONE)["raw"].mean()
    assert abs(loss - want) <= 1e-10 * max(1.0, abs(want))
    want_own = 1.0 - psr.per_pose(kps_w, gt, joints=psr.GAN_JOINTS, root=0, align=psr.ALIGN_NONE)["raw"].mean()
    assert abs(loss - want_own) <= 4 * np.sqrt(3) * bound.max()


# ---- the two evaluation functions -----------------------------------------------------------------------------------------------------------
def test_evaluate_smpl_predictions(renderer):
    V, B, K, NB = 431, 40, 17, 10
    models = [model_of(V, NB, K, seed=s) for s in (3, 4, 5)]
    bodies = [body_of(renderer, V, NB, K, seed=s) for s in (3, 4, 5)]
    pred_betas, pose_p, pred_rot = make_inputs(B, NB, 21)
    gt_betas, gt_pose, _ = make_inputs(B, NB, 22)
    gt_pose = (pose_p + np.random.RandomState(2).normal(0, 0.05, pose_p.shape)).astype(np.float32).reshape(B, 72)
    gender = np.random.RandomState(3).randint(0, 2, B)
    assert 0 < gender.sum() < B
    sc = pe.PoseScorer(renderer)
    got = pe.evaluate_smpl_predictions(*bodies, pred_rot, pred_betas, gt_pose, gt_betas, gender, h36m=str(K), scorer=sc)
    own = ref.evaluate_test(*models, f"regressor_{K}", pred_rot, pred_betas, gt_pose, gt_betas, gender)
    # the device's key points and vertices against the restatement's: the body's bounds (joint 0 is subtracted: twice the largest)
    fem = torch.from_numpy(gender == 1).to(DEV).view(B, 1, 1)
    eye = np.broadcast_to(np.eye(3, dtype=np.float32), (B, 24, 3, 3)).copy()
    p = bodies[0].forward(pred_betas, pred_rot, pose2rot=False, regressor=str(K), want_vertices=True)
    gm = bodies[1].forward(gt_betas, gt_pose.reshape(B, 24, 3), regressor=str(K), want_vertices=True)
    gf = bodies[2].forward(gt_betas, gt_pose.reshape(B, 24, 3), regressor=str(K), want_vertices=True)
    un = [b.forward(bt, eye, pose2rot=False, want_vertices=True).vertices for b, bt in zip(bodies, (pred_betas, gt_betas, gt_betas))]
    dev_kps = (pe._pelvis_j14(p.regressed).cpu().numpy(), pe._pelvis_j14(torch.where(fem, gf.regressed, gm.regressed)).cpu().numpy())
    dev_verts = tuple(t.cpu().numpy() for t in (torch.where(fem, un[2], un[1]), un[0], torch.where(fem, gf.vertices, gm.vertices), p.vertices))
    restated = [ref.lbs(models[0], pred_betas, pred_rot, pose2rot=False, regress=models[0][f"regressor_{K}"])]
    restated += [ref.lbs(m, gt_betas, gt_pose.reshape(B, 24, 3), regress=m[f"regressor_{K}"]) for m in models[1:]]
    b_kps = 2 * max(ref.bound_regressed(o, NB, V).max() for o in restated)          # joint 0 is subtracted: two regressed joints
    b_verts = max(ref.bound_verts(o, NB).max() for o in restated)
    for d, w in zip(dev_kps, own["_kps"]):
        assert np.abs(d - w).max() <= b_kps
    for d, w in zip(dev_verts[2:], own["_verts"][2:]):
        assert np.abs(d - w).max() <= b_verts
    # the scores as functions of exactly what the device produced
    want = ref.evaluate_test(*models, f"regressor_{K}", pred_rot, pred_betas, gt_pose, gt_betas, gender, given=dev_kps + dev_verts)
    for k in ("mpjpe", "pa-mpjpe", "ume", "pme"):
        assert got[k].shape == (B,) and np.all(np.abs(got[k] - want[k]) <= 1e-10 * np.maximum(1, np.abs(want[k]))), k
    # and against the restatement's own bodies: a distance moves by no more than its two points do (a wrong body moves it by far more)
    assert np.abs(got["mpjpe"] - own["mpjpe"]).max() <= 2 * np.sqrt(3) * b_kps
    assert np.abs(got["pme"] - own["pme"]).max() <= 2 * np.sqrt(3) * b_verts and np.abs(got["ume"] - own["ume"]).max() <= 2 * np.sqrt(3) * b_verts
    print("mean pck", got["pck"].mean(), "mean mpjpe", got["mpjpe"].mean())
    assert np.abs(got["pck"] - want["pck"]).max() <= 1e-10


def test_pampjpe_from_smpl_params(renderer):
    V, B, K, NB = 431, 40, 17, 10
    model, body = model_of(V, NB, K), body_of(renderer, V, NB, K)
    betas, bones, _ = make_inputs(B, NB, 31)
    own_kps = ref.pampjpe_from_smpl_params(model, f"regressor_{K}", np.zeros((B, 17, 3)), betas[:1], bones)["pred_kps"]
    rng = np.random.RandomState(7)
    gt_kps = ((own_kps + rng.normal(0, 0.03, own_kps.shape)) * 1000.0).astype(np.float32)       # millimetres
    sc = pe.PoseScorer(renderer)
    for normalize in (False, True):
        got = pe.pampjpe_from_smpl_params(body, gt_kps, betas[:1], bones, regressor=str(K), use_normalize=normalize, scorer=sc)
        dev_kps = got["pred_kps"].cpu().numpy()
        bound = ref.bound_regressed(ref.lbs(model, betas[:1], ref.axisang_to_rot(bones), pose2rot=False, regress=model[f"regressor_{K}"]), NB, V)
        assert np.all(np.abs(dev_kps - own_kps) <= bound[:, ref.SPIN_TO_CANON])
        want = ref.pampjpe_from_smpl_params(model, f"regressor_{K}", gt_kps, betas[:1], bones, use_normalize=normalize, pred_kps=dev_kps)
        for k in ("pampjpe", "mpjpe", "pck", "auc"):
            assert abs(got[k] - want[k]) <= 1e-10 * max(1.0, abs(want[k])), (k, got[k], want[k])
        assert 0 < got["auc"] < 1 and 20 < got["pampjpe"] < 80
