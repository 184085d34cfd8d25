"""The hand-written float64 backward of the SMPL body (tests/smpl_grad_ref.py) against float64 autograd through a torch restatement of
`smpl_ref.lbs`, against the reference's own autograd (tests/golden/smpl_body_grad.npz, tools/gen_golden_smpl_grad.py), the meaning of
its bound, and the Python layer of `BodyModel.differentiable` without a GPU.

Bound (derived in tests/smpl_grad_ref.py, not tuned): n u mag, u = 2^-24, n = (1 + NB + 207) + K + 70.

Observed on the host (printed by this module; nothing is set from them): the restatement against the reference's float64 autograd
4.0e-15 of max(1, |value|); the reference's float32 autograd / bound at most 0.012 (d_pose, the posed joints' cotangent alone);
least movement of an ablation 163 bounds (d_betas without -G_R^T dA_t, the 9-row regressor)."""
import os
import re
import types

import numpy as np
import pytest
import torch

from posegen_amd import _ffi, smpl, synthetic
from tests import smpl_grad_ref as gref
from tests import smpl_ref as ref

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BODY = np.load(os.path.join(REPO, "tests", "golden", "smpl_body.npz"))
GOLD = np.load(os.path.join(REPO, "tests", "golden", "smpl_body_grad.npz"))
V, NB = int(GOLD["V"]), int(GOLD["NB"])
ROWS = tuple(int(k) for k in GOLD["regress_rows"])
CASES = {"verts": ("verts",), "joints": ("joints",), "reg17": ("reg17",), "reg9": ("reg9",), "all17": ("verts", "joints", "reg17"),
         "all9": ("verts", "joints", "reg9")}
FORMS = ("axis", "rotmat")


@pytest.fixture(scope="module")
def model():
    assert int(GOLD["seed"]) == int(BODY["seed"]) and V == int(BODY["V"]) and NB == int(BODY["NB"])
    return synthetic.make_body_model(V, NB=NB, seed=int(GOLD["seed"]), regress_rows=ROWS)


def fixture_case(model, case, form, drop=()):
    """(the restatement's gradients of a fixture case, K)"""
    K = 9 if case.endswith("9") else 17
    parts = CASES[case]
    kw = dict(d_verts=GOLD["cot_verts"] if "verts" in parts else None, d_joints=GOLD["cot_joints"] if "joints" in parts else None,
              d_regressed=GOLD[f"cot_reg{K}"] if f"reg{K}" in parts else None)
    pose = BODY["pose"] if form == "axis" else BODY["rotmat"]
    return gref.lbs_backward(model, BODY["betas"], pose, pose2rot=form == "axis", regress=model[f"regressor_{K}"], drop=drop, **kw), K


def torch_lbs(model, betas, pose, pose2rot, regress):
    """`smpl_ref.lbs` in float64 torch ops: (verts, joints, regressed)"""
    t = lambda a: torch.from_numpy(ref.f64(a))
    vt, sd, pd, jr, W = (t(model[k]) for k in ("v_template", "shapedirs", "posedirs", "J_regressor", "lbs_weights"))
    parents = [int(p) for p in model["parents"]]
    B = pose.shape[0]
    betas = betas.expand(B, -1)
    v_shaped = vt[None] + torch.einsum("bl,mkl->bmk", betas, sd)
    J = torch.einsum("jv,bvc->bjc", jr, v_shaped)
    if pose2rot:
        r = pose.reshape(-1, 3)
        angle = ((r + 1e-8) ** 2).sum(1, keepdim=True).sqrt()
        d = r / angle
        z = torch.zeros_like(d[:, 0])
        Km = torch.stack([z, -d[:, 2], d[:, 1], d[:, 2], z, -d[:, 0], -d[:, 1], d[:, 0], z], 1).reshape(-1, 3, 3)
        R = (torch.eye(3, dtype=torch.float64) + torch.sin(angle)[:, :, None] * Km + (1 - torch.cos(angle))[:, :, None] * (Km @ Km))
        R = R.reshape(B, 24, 3, 3)
    else:
        R = pose.reshape(B, 24, 3, 3)
    v_posed = v_shaped + ((R[:, 1:] - torch.eye(3, dtype=torch.float64)).reshape(B, 207) @ pd).reshape(B, -1, 3)
    G_R, G_t = [R[:, 0]], [J[:, 0]]
    for i in range(1, 24):
        p = parents[i]
        G_R.append(G_R[p] @ R[:, i])
        G_t.append(G_t[p] + torch.einsum("brc,bc->br", G_R[p], J[:, i] - J[:, p]))
    G_R, joints = torch.stack(G_R, 1), torch.stack(G_t, 1)
    A = torch.cat([G_R, (joints - torch.einsum("bjrc,bjc->bjr", G_R, J))[..., None]], -1)
    T = torch.einsum("vj,bjrc->bvrc", W, A)
    verts = torch.einsum("bvrc,bvc->bvr", T[..., :3], v_posed) + T[..., 3]
    return verts, joints, None if regress is None else torch.einsum("kv,bvc->bkc", t(regress), verts)


def autograd(model, betas, pose, pose2rot, regress, d_verts, d_joints, d_regressed):
    b = torch.from_numpy(ref.f64(betas)).requires_grad_(True)
    p = torch.from_numpy(ref.f64(pose)).requires_grad_(True)
    outs = torch_lbs(model, b, p, pose2rot, regress)
    loss = sum((o * torch.from_numpy(ref.f64(c))).sum() for o, c in zip(outs, (d_verts, d_joints, d_regressed)) if c is not None)
    gb, gp = torch.autograd.grad(loss, (b, p))
    return gb.numpy(), gp.numpy()


def close(got, want, what):
    err = np.max(np.abs(got - want) / np.maximum(1.0, np.abs(want)))
    assert err <= 1e-10, (what, err)
    return err


@pytest.mark.parametrize("form", FORMS)
def test_restatement_equals_float64_autograd(model, form):
    worst = 0.0
    sets = [("fixture", model, BODY["betas"], BODY["pose"] if form == "axis" else BODY["rotmat"], 17)]
    rng = np.random.RandomState(11)
    small = synthetic.make_body_model(70, NB=4, seed=8, regress_rows=(5,))
    pose = rng.normal(0, 0.6, (3, 24, 3)).astype(np.float32)
    if form == "rotmat":                                 # any matrices: the nine entries are free
        pose = (ref.rodrigues(pose.reshape(-1, 3)).reshape(3, 24, 3, 3) + rng.normal(0, 0.05, (3, 24, 3, 3))).astype(np.float32)
    sets.append(("random", small, rng.uniform(-2, 2, (3, 4)).astype(np.float32), pose, 5))
    for name, m, betas, pose, K in sets:
        B, Vm = pose.shape[0], m["v_template"].shape[0]
        cot = dict(d_verts=rng.randn(B, Vm, 3), d_joints=rng.randn(B, 24, 3), d_regressed=rng.randn(B, K, 3))
        reg = m[f"regressor_{K}"]
        for keep in (("d_verts",), ("d_joints",), ("d_regressed",), tuple(cot)):
            kw = {k: (v if k in keep else None) for k, v in cot.items()}
            got = gref.lbs_backward(m, betas, pose, pose2rot=form == "axis", regress=reg, **kw)
            wb, wp = autograd(m, betas, pose, form == "axis", reg, **kw)
            worst = max(worst, close(got["d_betas"], wb, (name, keep, "d_betas")), close(got["d_pose"], wp.reshape(got["d_pose"].shape), (name, keep)))
            assert np.all(got["mag_betas"] >= np.abs(got["d_betas"]) * (1 - 1e-12)) and np.all(got["mag_pose"] >= np.abs(got["d_pose"]) * (1 - 1e-12))
        # one betas row for all poses: the rows added in pose order
        got = gref.lbs_backward(m, betas[:1], pose, pose2rot=form == "axis", regress=reg, **cot)
        wb, wp = autograd(m, betas[:1], pose, form == "axis", reg, **cot)
        assert got["d_betas"].shape == (B, betas.shape[1])
        worst = max(worst, close(gref.shared_betas_row(got["d_betas"]), wb, (name, "shared row")), close(got["d_pose"], wp.reshape(got["d_pose"].shape), name))
    print(f"{form}: restatement against float64 autograd, worst error / max(1, |value|) = {worst:.2e}")


@pytest.mark.parametrize("form", FORMS)
def test_restatement_equals_the_reference_float64(model, form):
    worst = 0.0
    for case in CASES:
        got, _ = fixture_case(model, case, form)
        for name in ("betas", "pose"):
            worst = max(worst, close(got[f"d_{name}"], GOLD[f"d_{name}_{case}_{form}_f64"], (case, form, name)))
    print(f"{form}: restatement against the reference's float64 autograd, worst = {worst:.2e}")


def _ratio(diff, bound):
    """max |diff| / bound; an entry with a zero bound must not differ at all"""
    diff = np.abs(diff)
    assert np.all(diff[bound == 0] == 0)
    return float(np.max(diff[bound > 0] / bound[bound > 0])) if np.any(bound > 0) else 0.0


def test_reference_float32_gradients_lie_inside_the_bound(model):
    """the condition on n: the reference's own float32 autograd, whose sums run over all V vertices in float32, is inside n u mag"""
    worst = {}
    for form in FORMS:
        for case in CASES:
            got, K = fixture_case(model, case, form)
            for name, bound in zip(("betas", "pose"), gref.bounds(got, NB, K)):
                assert np.isfinite(got[f"d_{name}"]).all() and np.isfinite(GOLD[f"d_{name}_{case}_{form}_f32"]).all()
                worst[(form, case, name)] = _ratio(ref.f64(GOLD[f"d_{name}_{case}_{form}_f32"]) - got[f"d_{name}"], bound)
    print("reference float32 / bound:", {"/".join(k): round(v, 4) for k, v in worst.items()})
    print("worst:", max(worst.values()))
    assert max(worst.values()) <= 1, worst


@pytest.mark.parametrize("term", gref.TERMS)
def test_dropping_a_term_leaves_the_bound(model, term):
    """each term of the backward, left out, moves d_betas or d_pose of the all-cotangents cases far outside the bound"""
    moved = {}
    for form in FORMS:
        for case in ("all17", "all9"):
            base, K = fixture_case(model, case, form)
            abl, _ = fixture_case(model, case, form, drop=(term,))
            bb, bp = gref.bounds(base, NB, K)
            with np.errstate(divide="ignore", invalid="ignore"):
                moved[(form, case)] = max(np.nanmax(np.abs(abl["d_betas"] - base["d_betas"]) / bb), np.nanmax(np.abs(abl["d_pose"] - base["d_pose"]) / bp))
    print(term, "moves the gradients by (bounds):", {"/".join(k): round(float(v), 1) for k, v in moved.items()})
    assert min(moved.values()) >= 10, (term, moved)


def test_n_is_a_function_of_the_sizes_only():
    assert gref.n_grad_products(10, 17) == 218 + 17 + 70 and gref.n_grad_products(16, 64) == 224 + 64 + 70
    assert gref.n_grad_products(1, 0) == 209 + 70


# ---- the Python layer without a GPU ------------------------------------------------------------------------------------------------------
def test_differentiable_refusals_come_before_the_library():
    body = object.__new__(smpl.BodyModel)                         # (a body that cannot launch anything: no renderer, no arrays)
    body.device, body.V, body.NB, body.regressors = torch.device("cuda:0"), 7, 10, {"h36m": None}
    body.renderer = types.SimpleNamespace(device="cuda:0", lib=None, handle=None)
    betas, pose = torch.zeros(2, 10, requires_grad=True), torch.zeros(2, 24, 3, requires_grad=True)
    with pytest.raises(NotImplementedError, match="transl"):
        body.differentiable(betas, pose, transl=torch.zeros(2, 3))
    with pytest.raises(NotImplementedError, match="host array"):
        body.differentiable(np.zeros((2, 10), np.float32), pose)
    with pytest.raises(NotImplementedError, match="host tensors"):
        body.differentiable(betas, pose)                          # tensors on the host, the body on a device
    with pytest.raises(NotImplementedError, match="host tensors"):
        body.differentiable(betas, global_orient=pose[:, :1], body_pose=pose[:, 1:])
    with pytest.raises(ValueError, match="global_orient and body_pose"):
        body.differentiable(betas, global_orient=pose[:, :1])
    body.device = torch.device("cpu")                             # (so that host tensors pass the device check and reach the shape checks)
    with pytest.raises(TypeError, match="floating point"):
        body.differentiable(betas, torch.zeros(2, 24, 3, dtype=torch.int32))
    with pytest.raises(ValueError, match="betas"):
        body.differentiable(torch.zeros(2, 9), pose)
    with pytest.raises(ValueError, match="rows of betas"):
        body.differentiable(torch.zeros(3, 10), pose)
    with pytest.raises(ValueError, match="rotation matrices"):
        body.differentiable(betas, pose, pose2rot=False)
    with pytest.raises(KeyError, match="no regressor"):
        body.differentiable(betas, pose, regressor="extra")
    with pytest.raises(ValueError, match="no output"):
        body.differentiable(betas, pose, joints=False)
    with pytest.raises(NotImplementedError, match="gradients"):   # forward still refuses, and names the way out
        body.forward(betas, pose)
    with pytest.raises(NotImplementedError, match="differentiable"):
        body.forward(betas, pose)


def test_header_and_binding_declare_the_backward():
    from posegen_amd import ganloop
    flat = re.sub(r"\s+", " ", open(os.path.join(REPO, "include", "posegen_hip.h")).read())
    assert ("int pg_smpl_backward(pg_handle* h, void* stream, const pg_body_model* m, int64_t B, const float* betas, int64_t betas_stride, "
            "const float* pose, int pose_is_rotmat, const float* regress, int K, const float* blend_t, const float* d_verts, "
            "const float* d_joints, const float* d_regressed, float* d_betas, float* d_pose);") in flat
    assert len(_ffi.PROTOTYPES["pg_smpl_backward"][1]) == 16 and _ffi.PG_ABI_VERSION == 11           # an added entry point does not move it
    lib = _ffi.load_library()
    assert lib.pg_smpl_backward(None, None, None, 1, None, 0, None, 0, None, 0, None, None, None, None, None, None) == _ffi.PG_EINVAL
    assert callable(smpl.BodyModel.differentiable) and callable(ganloop.regressor_body_loss)
