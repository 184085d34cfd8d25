"""pg_smpl_backward on the GPU, through the C ABI and through BodyModel.differentiable / ganloop.regressor_body_loss, against the
hand-written float64 backward (tests/smpl_grad_ref.py) and the reference's own float64 autograd (tests/golden/smpl_body_grad.npz).

Bound (derived in tests/smpl_grad_ref.py): n u mag with u = 2^-24, n = (1 + NB + 207) + K + 70, mag the restatement's backward in
absolute values.  An entry whose mag is zero must be exactly zero.  Every case prints its error / bound; nothing is set from them.

Largest observed error / bound on the MI355X (this module's printed ratios): d_betas 0.0006, d_pose 0.0112 (V = 7, B = 67, rotation
matrices); at V = 6890, B = 33: 0.0002 and 0.0002; regressor_body_loss 0.0008 and 0.0043."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

from posegen_amd import _ffi, ganloop, smpl, synthetic
from tests import keypoint_grad_ref as kref
from tests import smpl_grad_ref as gref
from tests import smpl_ref as ref
from tests.frame_metrics_gpu import DEV, renderer  # noqa: F401 (renderer: a fixture)

pytestmark = pytest.mark.gpu
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BODY = np.load(os.path.join(REPO, "tests", "golden", "smpl_body.npz"))
GOLD = np.load(os.path.join(REPO, "tests", "golden", "smpl_body_grad.npz"))
EINVAL = -1
SENTINEL = -7.0
COTS = ("verts", "joints", "regressed")
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


def make_inputs(B, NB, V, K, seed):
    """betas in [-3, 3], poses with angles up to 1.5 about random axes (pose 0 at rest), their matrices, and cotangents at the
    fixture's scales"""
    rng = np.random.RandomState(seed)
    betas = rng.uniform(-3.0, 3.0, size=(B, NB)).astype(np.float32)
    axes = rng.randn(B, 24, 3)
    axes /= np.linalg.norm(axes, axis=-1, keepdims=True)
    pose = (axes * rng.uniform(0.2, 1.5, size=(B, 24, 1))).astype(np.float32)
    pose[0] = 0.0
    rot = ref.rodrigues(pose.reshape(-1, 3)).reshape(B, 24, 3, 3).astype(np.float32)
    cot = {"verts": (rng.randn(B, V, 3) / 16.0).astype(np.float32), "joints": rng.randn(B, 24, 3).astype(np.float32),
           "regressed": rng.randn(B, K, 3).astype(np.float32) if K else None}
    return betas, pose, rot, cot


def abi(r, body, betas, pose, cot, rotmat=False, K=None, B=None, stride=None, null=(), struct=None, blend_t=True):
    """pg_smpl_backward through the C ABI -> (return code, {"d_betas", "d_pose"} numpy).  Both outputs start filled with SENTINEL and
    have one guard element behind them; `null`: argument names passed as NULL; `cot`: {"verts", "joints", "regressed"} (None = NULL)."""
    Bv = pose.shape[0]
    reg = next(iter(body.regressors.values())) if body.regressors else None
    Kv = (0 if reg is None else reg.shape[0]) if K is None else K
    new = lambda n: torch.full((n + 1,), SENTINEL, dtype=torch.float32, device=DEV)
    out = {"d_betas": new(Bv * body.NB), "d_pose": new(pose.size)}
    dev = {k: None if cot.get(k) is None else torch.from_numpy(np.ascontiguousarray(cot[k], dtype=np.float32)).to(DEV) for k in COTS}
    d_betas_in, d_pose_in = torch.from_numpy(betas).to(DEV), torch.from_numpy(pose).to(DEV)
    ptr = lambda name, t: None if (name in null or t is None) else C.c_void_p(t.data_ptr())
    rc = r.lib.pg_smpl_backward(r.handle, r._stream(), None if "model" in null else C.byref(body._model if struct is None else struct),
                                Bv if B is None else B, ptr("betas", d_betas_in), (body.NB if betas.shape[0] == Bv else 0) if stride is None else stride,
                                ptr("pose", d_pose_in), int(rotmat), ptr("regress", reg), Kv, ptr("blend_t", body._blend_transposed() if blend_t else None),
                                ptr("verts", dev["verts"]), ptr("joints", dev["joints"]), ptr("regressed", dev["regressed"]),
                                ptr("d_betas", out["d_betas"]), ptr("d_pose", out["d_pose"]))
    torch.cuda.synchronize()
    host = {k: v.cpu().numpy() for k, v in out.items()}
    for k, v in host.items():
        assert v[-1] == SENTINEL, f"{k}: the element behind the output was written"
        if rc != 0 or k in null:
            assert (v == SENTINEL).all(), f"{k}: written though refused or not asked for"
    if rc == 0:
        host = {"d_betas": host["d_betas"][:-1].reshape(Bv, body.NB), "d_pose": host["d_pose"][:-1].reshape(pose.shape)}
    return rc, host


def restate(model, betas, pose, cot, rotmat, K):
    return gref.lbs_backward(model, betas, pose, pose2rot=not rotmat, regress=model[f"regressor_{K}"] if K else None,
                             d_verts=cot.get("verts"), d_joints=cot.get("joints"), d_regressed=cot.get("regressed"))


def ratio(got, want, bound):
    err = np.abs(ref.f64(got) - want)
    assert np.all(err[bound == 0] == 0), "an entry whose bound is zero differs"
    return float(np.max(err[bound > 0] / bound[bound > 0])) if np.any(bound > 0) else 0.0


def check(got, want, NB, K, what, null=()):
    ratios = {}
    for k, bound in zip(("d_betas", "d_pose"), gref.bounds(want, NB, K)):
        if k not in null:
            ratios[k] = ratio(got[k], want[k], bound)
    print(what, "error / bound:", {k: round(v, 4) for k, v in ratios.items()})
    assert all(v <= 1 for v in ratios.values()), (what, ratios)
    return ratios


# ---- the fixture's model ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("K", [17, 9])
@pytest.mark.parametrize("form", ["axis", "rotmat"])
def test_fixture_model_against_restatement_and_reference(renderer, form, K):
    V, NB, seed = int(GOLD["V"]), int(GOLD["NB"]), int(GOLD["seed"])
    model = synthetic.make_body_model(V, NB=NB, seed=seed, regress_rows=(17, 9))
    body = smpl.BodyModel(renderer, *(model[k] for k in smpl.MODEL_KEYS), regressors={"k": model[f"regressor_{K}"]})
    rotmat = form == "rotmat"
    pose = BODY["rotmat"] if rotmat else BODY["pose"]
    full = {"verts": GOLD["cot_verts"], "joints": GOLD["cot_joints"], "regressed": GOLD[f"cot_reg{K}"]}
    for case, keep in (("verts", ("verts",)), ("joints", ("joints",)), (f"reg{K}", ("regressed",)), (f"all{K}", COTS)):
        cot = {k: full[k] for k in keep}
        want = gref.lbs_backward(model, BODY["betas"], pose, pose2rot=not rotmat, regress=model[f"regressor_{K}"], d_verts=cot.get("verts"),
                                 d_joints=cot.get("joints"), d_regressed=cot.get("regressed"))
        rc, got = abi(renderer, body, BODY["betas"], pose, cot, rotmat=rotmat)
        assert rc == 0
        check(got, want, NB, K, f"fixture {form} {case}")
        assert np.isfinite(got["d_betas"]).all() and np.isfinite(got["d_pose"]).all()       # pose 0 is at rest, pose 1 near pi
        for name, bound in zip(("betas", "pose"), gref.bounds(want, NB, K)):                  # the reference's own float64 autograd
            r64 = ratio(got[f"d_{name}"], ref.f64(GOLD[f"d_{name}_{case}_{form}_f64"]), bound + 1e-12)
            assert r64 <= 1, (case, name, r64)


# ---- tails in every direction -----------------------------------------------------------------------------------------------------------
TAILS = [(1, 1, 0, 1), (1, 5, 1, 10), (1, 67, 64, 16), (7, 1, 64, 10), (7, 33, 17, 10), (7, 67, 0, 16), (65, 5, 17, 1), (65, 33, 1, 16),
         (65, 67, 64, 10), (431, 1, 1, 16), (431, 5, 0, 10), (431, 67, 64, 1), (431, 33, 17, 10)]


@pytest.mark.parametrize("V,B,K,NB", TAILS)
def test_tails(renderer, V, B, K, NB):
    model, body = model_of(V, NB, K), body_of(renderer, V, NB, K)
    betas, pose, rot, cot = make_inputs(B, NB, V, K, 10 * V + B)
    for form, p in (("axis", pose), ("rotmat", rot)):
        want = restate(model, betas, p, cot, form == "rotmat", K)
        rc, got = abi(renderer, body, betas, p, cot, rotmat=form == "rotmat")
        assert rc == 0
        check(got, want, NB, K, f"V={V} B={B} K={K} NB={NB} {form}")


@pytest.mark.parametrize("skip", COTS)
def test_each_cotangent_null_in_turn(renderer, skip):
    V, B, K, NB = 431, 5, 9, 10
    model, body = model_of(V, NB, K), body_of(renderer, V, NB, K)
    betas, pose, _, cot = make_inputs(B, NB, V, K, 77)
    part = {k: v for k, v in cot.items() if k != skip}
    rc, got = abi(renderer, body, betas, pose, part)
    assert rc == 0
    check(got, restate(model, betas, pose, part, False, K), NB, K, f"without d_{skip}")
    zero = dict(part)
    zero[skip] = np.zeros_like(cot[skip])                        # NULL is a zero cotangent
    rc, same = abi(renderer, body, betas, pose, zero)
    assert rc == 0
    check(same, restate(model, betas, pose, part, False, K), NB, K, f"a zero d_{skip}")
    only = {skip: cot[skip]}                                     # and each one alone
    rc, got = abi(renderer, body, betas, pose, only)
    assert rc == 0
    check(got, restate(model, betas, pose, only, False, K), NB, K, f"d_{skip} alone")


@pytest.mark.parametrize("skip", ["d_betas", "d_pose"])
def test_each_output_null_in_turn(renderer, skip):
    V, B, K, NB = 431, 5, 9, 10
    body = body_of(renderer, V, NB, K)
    betas, pose, rot, cot = make_inputs(B, NB, V, K, 78)
    for rotmat, p in ((False, pose), (True, rot)):
        rc, full = abi(renderer, body, betas, p, cot, rotmat=rotmat)
        rc2, got = abi(renderer, body, betas, p, cot, rotmat=rotmat, null=(skip,))
        assert rc == 0 and rc2 == 0
        keep = "d_pose" if skip == "d_betas" else "d_betas"
        assert np.array_equal(got[keep], full[keep])             # what is written does not depend on what else is


def test_without_blend_t(renderer):
    V, B, K, NB = 431, 33, 17, 10
    model, body = model_of(V, NB, K), body_of(renderer, V, NB, K)
    betas, pose, _, cot = make_inputs(B, NB, V, K, 79)
    rc, fast = abi(renderer, body, betas, pose, cot)
    rc2, slow = abi(renderer, body, betas, pose, cot, blend_t=False)
    assert rc == 0 and rc2 == 0
    check(slow, restate(model, betas, pose, cot, False, K), NB, K, "blend read strided")
    for k in fast:
        assert np.array_equal(fast[k], slow[k]), k               # the same operands in the same order


# ---- at size --------------------------------------------------------------------------------------------------------------------------------
def test_at_size(renderer):
    V, B, K, NB = 6890, 33, 17, 10
    model, body = model_of(V, NB, K, seed=0), body_of(renderer, V, NB, K, seed=0)
    betas, pose, _, cot = make_inputs(B, NB, V, K, 5)
    rc, got = abi(renderer, body, betas, pose, cot)
    assert rc == 0
    check(got, restate(model, betas, pose, cot, False, K), NB, K, "V=6890 B=33 K=17")


# ---- invariants -----------------------------------------------------------------------------------------------------------------------------
def test_bitwise_invariants(renderer):
    V, B, K, NB = 431, 67, 17, 10
    body = body_of(renderer, V, NB, K)
    betas, pose, _, cot = make_inputs(B, NB, V, K, 9)
    rc, a = abi(renderer, body, betas, pose, cot)
    rc2, b = abi(renderer, body, betas, pose, cot)
    assert rc == 0 and rc2 == 0
    for k in a:
        assert np.array_equal(a[k], b[k]), f"{k}: two calls differ"
    for at in (0, 31, 66):                                       # a pose alone = the pose in its batch
        rc, one = abi(renderer, body, betas[at:at + 1], pose[at:at + 1], {k: v[at:at + 1] for k, v in cot.items()}, stride=NB)
        assert rc == 0
        for k in a:
            assert np.array_equal(one[k][0], a[k][at]), f"{k}: pose {at} alone differs from pose {at} of {B}"
    roll = lambda x: np.ascontiguousarray(np.roll(x, 5, axis=0))  # and at another position in the batch
    rc, moved = abi(renderer, body, roll(betas), roll(pose), {k: roll(v) for k, v in cot.items()})
    assert rc == 0
    for k in a:
        assert np.array_equal(moved[k], roll(a[k])), f"{k}: a pose's bytes depend on where it sits"
    rc, rows = abi(renderer, body, betas[3:4], pose, cot, stride=0)      # one betas row: still a row per pose
    rc2, wide = abi(renderer, body, np.repeat(betas[3:4], B, axis=0), pose, cot)
    assert rc == 0 and rc2 == 0
    for k in a:
        assert np.array_equal(rows[k], wide[k]), f"{k}: betas_stride = 0 differs from the expanded betas"


@pytest.mark.parametrize("where", ["pose", "betas", "d_verts", "d_joints", "d_regressed"])
def test_nan_stays_in_its_pose(renderer, where):
    V, B, K, NB = 431, 67, 17, 10
    body = body_of(renderer, V, NB, K)
    betas, pose, _, cot = make_inputs(B, NB, V, K, 9)
    rc, clean = abi(renderer, body, betas, pose, cot)
    bad_b, bad_p, bad_c = betas.copy(), pose.copy(), {k: v.copy() for k, v in cot.items()}
    if where == "pose":
        bad_p[40, 7, 1] = np.nan
    elif where == "betas":
        bad_b[40, 2] = np.nan
    else:
        bad_c[where[2:]][40, 3, 1] = np.nan
    rc2, got = abi(renderer, body, bad_b, bad_p, bad_c)
    assert rc == 0 and rc2 == 0
    keep = np.arange(B) != 40
    for k in clean:
        assert np.array_equal(got[k][keep], clean[k][keep]), f"{k}: a NaN in pose 40 changed another pose"
        if (where, k) != ("betas", "d_betas"):                   # (the body is linear in betas: d_betas does not read them)
            assert not np.isfinite(got[k][40]).all(), k


# ---- refusals -------------------------------------------------------------------------------------------------------------------------------
def test_einval_writes_nothing(renderer):
    V, B, K, NB = 7, 5, 9, 10
    body = body_of(renderer, V, NB, K)
    betas, pose, _, cot = make_inputs(B, NB, V, K, 1)

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
        "all cotangents NULL": dict(null=COTS), "both outputs NULL": dict(null=("d_betas", "d_pose")), "B = 0": dict(B=0), "B < 0": dict(B=-3),
        "NB = 0": dict(struct=struct(NB=0)), "NB = 17": dict(struct=struct(NB=17)), "V = 0": dict(struct=struct(V=0)),
        "V too large": dict(struct=struct(V=(2 ** 31) // ((1 + NB + 207) * 3) + 1)), "K = -1": dict(K=-1), "K = 65": dict(K=65),
        "K > 0, regress NULL": dict(null=("regress",)), "d_regressed with K = 0": dict(K=0), "betas_stride = 3": dict(stride=3),
        "a NULL model array": dict(struct=struct(skin=None)),
        "parents[0] = 0": dict(struct=struct(parents=[0] + par[1:])),
        "a child before its parent": dict(struct=struct(parents=par[:5] + [7] + par[6:])),
        "a negative parent": dict(struct=struct(parents=par[:9] + [-1] + par[10:])),
    }
    for name, kw in cases.items():
        rc, _ = abi(renderer, body, betas, pose, cot, **kw)       # (abi asserts that every sentinel is intact)
        assert rc == EINVAL, name
    rc, _ = abi(renderer, body, betas, pose, cot)                 # and the handle still works
    assert rc == 0


# ---- through Python -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("form", ["axis", "rotmat"])
def test_differentiable_is_forward_and_its_backward_is_the_abi(renderer, form):
    V, B, K, NB = 431, 33, 17, 10
    body = body_of(renderer, V, NB, K)
    betas, pose, rot, cot = make_inputs(B, NB, V, K, 41)
    p = rot if form == "rotmat" else pose
    tb = torch.from_numpy(betas).to(DEV).requires_grad_(True)
    tp = torch.from_numpy(p).to(DEV).requires_grad_(True)
    kw = dict(pose2rot=form == "axis", regressor=str(K), want_vertices=True)
    out = body.differentiable(tb, tp, **kw)
    plain = body.forward(betas, p, **kw)
    for a, b in zip(out, plain):
        assert a.dtype == torch.float32 and torch.equal(a.detach(), b)
    dev = {k: torch.from_numpy(v).to(DEV) for k, v in cot.items()}
    (out.vertices * dev["verts"]).sum().add((out.joints * dev["joints"]).sum()).add((out.regressed * dev["regressed"]).sum()).backward()
    rc, want = abi(renderer, body, betas, p, cot, rotmat=form == "rotmat")
    assert rc == 0
    assert np.array_equal(tb.grad.cpu().numpy(), want["d_betas"]) and np.array_equal(tp.grad.cpu().numpy(), want["d_pose"])
    # an output without a cotangent is passed as NULL: the regressed joints alone
    tb.grad, tp.grad = None, None
    out = body.differentiable(tb, tp, **kw)
    (out.regressed * dev["regressed"]).sum().backward()
    rc, want = abi(renderer, body, betas, p, {"regressed": cot["regressed"]}, rotmat=form == "rotmat")
    assert np.array_equal(tb.grad.cpu().numpy(), want["d_betas"]) and np.array_equal(tp.grad.cpu().numpy(), want["d_pose"])
    # one betas row for all poses: the rows in pose order, in float64, rounded once; [B,72] and global_orient + body_pose too
    if form == "axis":
        one = torch.from_numpy(betas[:1]).to(DEV).requires_grad_(True)
        flat = torch.from_numpy(pose.reshape(B, 72)).to(DEV).requires_grad_(True)
        out = body.differentiable(one, global_orient=flat[:, :3], body_pose=flat[:, 3:], regressor=str(K))
        (out.joints * dev["joints"]).sum().add((out.regressed * dev["regressed"]).sum()).backward()
        rc, rows = abi(renderer, body, betas[:1], pose, {"joints": cot["joints"], "regressed": cot["regressed"]}, stride=0)
        assert rc == 0 and one.grad.shape == (1, NB) and flat.grad.shape == (B, 72)
        assert np.array_equal(one.grad.cpu().numpy(), gref.shared_betas_row(rows["d_betas"]).astype(np.float32))
        assert np.array_equal(flat.grad.cpu().numpy().reshape(B, 24, 3), rows["d_pose"])
        with pytest.raises(RuntimeError):                         # once differentiable
            out = body.differentiable(one, flat, regressor=str(K))
            g, = torch.autograd.grad(out.joints.sum(), flat, create_graph=True)
            g.sum().backward()


@pytest.mark.parametrize("kind", ["mpjpe", "norm_matched"])
def test_regressor_body_loss_trains_pose_and_shape(renderer, kind):
    V, B, K, NB = 431, 33, 17, 10
    model, body = model_of(V, NB, K), body_of(renderer, V, NB, K)
    betas, pose, rot, _ = make_inputs(B, NB, V, K, 51)
    gt_betas, _, gt_rot, _ = make_inputs(B, NB, V, K, 52)
    gt_kps = body.forward(gt_betas, gt_rot, pose2rot=False, regressor=str(K), joints=False).regressed
    tb = torch.from_numpy(betas).to(DEV).requires_grad_(True)
    tr = torch.from_numpy(rot).to(DEV).requires_grad_(True)
    loss = ganloop.regressor_body_loss(body, tr, tb, gt_kps, str(K), kind=kind, weight=3.0)
    loss.backward()
    # float64: pose_loss's gradient at the key points the device produced, then the restatement's backward of that cotangent
    pred = body.forward(betas, rot, pose2rot=False, regressor=str(K), joints=False).regressed.cpu().numpy()
    p64 = torch.from_numpy(ref.f64(pred)).requires_grad_(True)
    want_loss, _, _ = kref.pose_loss(p64, torch.from_numpy(ref.f64(gt_kps.cpu().numpy())), joints=ref.H36M_TO_J14, root=0, kind=kind, weight=3.0)
    d_pred, = torch.autograd.grad(want_loss, p64)
    d_pred = d_pred.numpy()
    assert abs(float(loss.detach()) - float(want_loss.detach())) <= 1e-10 * max(1.0, abs(float(want_loss.detach())))
    want = gref.lbs_backward(model, betas, rot, pose2rot=False, regress=model[f"regressor_{K}"], d_regressed=d_pred)
    # pg_pose_loss hands d_pred over within one float32 ulp (+ 1e-10) of its float64 value; the body's backward is linear in it
    slack = gref.lbs_backward(model, betas, rot, pose2rot=False, regress=model[f"regressor_{K}"],
                              d_regressed=np.spacing(np.abs(d_pred).astype(np.float32)).astype(np.float64) + 1e-10)
    bb, bp = gref.bounds(want, NB, K)
    rb = ratio(tb.grad.cpu().numpy(), want["d_betas"], bb + slack["mag_betas"])
    rp = ratio(tr.grad.cpu().numpy(), want["d_pose"], bp + slack["mag_pose"])
    print(f"regressor_body_loss {kind}: error / bound d_betas {rb:.4f}, d_rotmat {rp:.4f}")
    assert rb <= 1 and rp <= 1 and np.abs(want["d_pose"]).max() > 0 and np.abs(want["d_betas"]).max() > 0
