"""The kinematic chain the pose kernels share (csrc/pg_kin.h) on joint trees other than SMPL's: every entry point that walks the tree,
on the SMPL tree, on one chain (parent[j] = j - 1: depth 23, the most levels) and on a star (parent[j] = 0: depth 1, the root
collects 23 children, the longest collect loop), at B = 5 -- one full workgroup of four waves and a tail wave that walks the last pose
again.

Each entry point against the float64 restatement it already has, with the bound its own test uses for the SMPL tree
(tests/test_gpu_smpl.py, test_gpu_smpl_grad.py, test_gpu_keypoint_grad.py, test_gpu_poseopt.py).  One of those bounds counts the
joints along the tree's longest chain -- smpl_ref.bound_chain, 9 u mag for the float32 inputs' own rounding through SMPL's depth of 8
-- and is derived here with the depth of the tree under test (depth + 1 = 24, 9 or 2), not loosened by hand; the others do not depend
on the tree.  The restatements' gradients
are checked against float64 autograd on the two new trees first, without a GPU."""
import ctypes as C

import numpy as np
import pytest
import torch

from posegen_amd import smpl, synthetic
from posegen_amd.poseopt import ray_segments
from posegen_amd.skeleton import SMPLSkeleton
from tests import keypoint_grad_ref as kref
from tests import poseopt_ref as pref
from tests import smpl_grad_ref as gref
from tests import smpl_ref as sref
from tests.frame_metrics_gpu import DEV, renderer  # noqa: F401 (renderer: a fixture)
from tests.test_gpu_keypoint_grad import assert_f32, assert_f64, cotangent
from tests.test_gpu_poseopt import _abi_args, _backward_call
from tests.test_gpu_smpl_grad import BODY, abi as abi_smpl_backward, check as check_smpl_backward, make_inputs
from tests.test_keypoint_grad_ref import REST32, edge_bones, noisy_rotmats
from tests.test_poseopt_host import OUTS, random_case
from tests.test_smpl_grad_ref import autograd as smpl_autograd, close

B = 5
SCALE = 0.4
TREES = {"smpl": np.asarray(SMPLSkeleton.joint_trees, dtype=np.int32), "chain": np.maximum(np.arange(24, dtype=np.int32) - 1, 0),
         "star": np.zeros(24, dtype=np.int32)}
_I32P = C.POINTER(C.c_int32)
_F64P = C.POINTER(C.c_double)


def parents_of(tree, root_entry):
    """the tree's table with the root's own entry as the entry point under test wants it"""
    par = TREES[tree].copy()
    par[0] = root_entry
    return par


def depth_of(tree):
    level = np.zeros(24, dtype=int)
    for j in range(1, 24):
        level[j] = level[TREES[tree][j]] + 1
    return int(level.max())


def body_model(tree):
    """the small fixture model (tests/golden/smpl_body.npz: its V, NB and seed) on the tree"""
    m = synthetic.make_body_model(int(BODY["V"]), NB=int(BODY["NB"]), seed=int(BODY["seed"]))
    return dict(m, parents=parents_of(tree, -1))


def test_depths():
    assert [depth_of(t) for t in ("smpl", "chain", "star")] == [8, 23, 1]


@pytest.mark.parametrize("tree", ["chain", "star"])
def test_restatements_agree_with_float64_autograd(tree):
    par = parents_of(tree, 0).astype(np.int64)
    # the key points: the restatement's gradient IS torch autograd; its forward against the numpy chain of smpl_ref
    rot = noisy_rotmats(B, 31)
    kps = kref.kps_from_rotmats(rot, REST32, SCALE, parents=par).numpy()
    assert np.abs(kps - sref.rot_chain(rot, REST32, SCALE, parents=par)[1]).max() <= 1e-12
    # the body: the hand-written transpose against autograd of the same forward
    model = body_model(tree)
    NB, V = int(BODY["NB"]), int(BODY["V"])
    betas, pose, rotm, cot = make_inputs(B, NB, V, 0, 41)
    for form, p in (("axis", pose), ("rotmat", rotm)):
        kw = dict(d_verts=cot["verts"], d_joints=cot["joints"], d_regressed=None)
        got = gref.lbs_backward(model, betas, p, pose2rot=form == "axis", **kw)
        wb, wp = smpl_autograd(model, betas, p, form == "axis", None, **kw)
        close(got["d_betas"], wb, (tree, form, "d_betas"))
        close(got["d_pose"], wp.reshape(got["d_pose"].shape), (tree, form, "d_pose"))
    # the pose layer likewise
    c = random_case(3, [2, 0, 2, 1, 0, 2, 1], seed=5)
    seg = ray_segments(c["idxs"])
    db, dp = pref.backward(c["bones"], c["pelvis"], c["rest"], seg.inverse, **{f"d_{k}": c["cot"][k] for k in OUTS}, parents=par)
    t = lambda a: torch.tensor(np.asarray(a, dtype=np.float64))
    bone, pelvis = t(c["bones"]).requires_grad_(True), t(c["pelvis"]).requires_grad_(True)
    outs = pref.torch_forward(bone, pelvis, t(c["rest"]), parents=par)
    inv = torch.as_tensor(seg.inverse, dtype=torch.long)
    sum((o[inv] * t(c["cot"][k])).sum() for k, o in zip(OUTS, outs)).backward()
    for what, got, want in (("d_bones", db, bone.grad.numpy()), ("d_pelvis", dp, pelvis.grad.numpy())):
        ent, nrm = pref.deviation(got, want)
        assert ent <= 1e-10 and nrm <= 1e-10, (tree, what, ent, nrm)


@pytest.mark.gpu
@pytest.mark.parametrize("tree", list(TREES))
def test_pose_kinematics_rot(renderer, tree):
    """the bounds of tests/test_gpu_smpl.py::test_pose_kinematics_rot"""
    par = parents_of(tree, -1)
    rot = sref.axisang_to_rot(synthetic.make_bones(B, seed=B, sigma=0.5))
    l2ws_w, kps_w, mag = sref.rot_chain(rot, REST32, scale=SCALE, parents=par)
    kps, skts, l2ws = (t.cpu().numpy() for t in renderer.pose_kinematics_rot(torch.from_numpy(rot), REST32, scale=SCALE, parents=par, want_l2ws=True))
    bound = sref.bound_chain(kps_w, mag, links=depth_of(tree) + 1)
    print(f"[{tree}] key points error / bound", float(np.max(np.abs(kps - kps_w) / bound)))
    assert np.all(np.abs(kps - kps_w) <= bound)
    assert np.abs(l2ws - l2ws_w).max() <= 1e-12
    inv = np.zeros_like(l2ws_w)
    inv[..., :3, :3] = np.swapaxes(l2ws_w[..., :3, :3], -1, -2)
    inv[..., :3, 3] = -np.einsum("fjcr,fjc->fjr", l2ws_w[..., :3, :3], l2ws_w[..., :3, 3])
    inv[..., 3, 3] = 1.0
    assert np.all(np.abs(skts - inv) <= np.spacing(np.abs(inv).astype(np.float32)) + 1e-12)


@pytest.mark.gpu
@pytest.mark.parametrize("axis", [True, False])
@pytest.mark.parametrize("tree", list(TREES))
def test_kinematics_backward(renderer, tree, axis):
    """pg_pose_kinematics_bwd / pg_pose_kinematics_rot_bwd with a dense cotangent: the bounds of tests/test_gpu_keypoint_grad.py"""
    par = parents_of(tree, 0 if axis else -1)
    offs = np.ascontiguousarray(kref.bone_offsets(REST32, SCALE, parents=par)[0])
    params = edge_bones(B, 15) if axis else noisy_rotmats(B, 25)
    g = cotangent(B, "dense")
    leaf = torch.from_numpy(params.astype(np.float64)).requires_grad_(True)
    kps = (kref.kps_from_axis_angle if axis else kref.kps_from_rotmats)(leaf, REST32, SCALE, parents=par)
    want = torch.autograd.grad(kps, leaf, torch.from_numpy(g.astype(np.float64)))[0].numpy()
    p_dev, g_dev = torch.from_numpy(params).to(DEV), torch.from_numpy(g).to(DEV)
    out = torch.full((params.size + 1,), -7.0, dtype=p_dev.dtype, device=DEV)
    fn = renderer.lib.pg_pose_kinematics_bwd if axis else renderer.lib.pg_pose_kinematics_rot_bwd
    rc = fn(renderer.handle, renderer._stream(), B, C.c_void_p(p_dev.data_ptr()), offs.ctypes.data_as(_F64P), par.ctypes.data_as(_I32P),
            C.c_void_p(g_dev.data_ptr()), C.c_void_p(out.data_ptr()))
    torch.cuda.synchronize()
    host = out.cpu().numpy()
    assert rc == 0 and host[-1] == -7.0
    got = host[:-1].reshape(params.shape)
    assert np.all(np.isfinite(got))
    (assert_f64 if axis else assert_f32)(got, want, f"[{tree}] {'axis-angle' if axis else 'rotation-matrix'} backward")


@pytest.mark.gpu
@pytest.mark.parametrize("tree", list(TREES))
def test_body_joints(renderer, tree):
    """pg_smpl_forward asked for `joints` only and pg_smpl_backward given `d_joints` only (no vertex kernel runs), both pose forms:
    the bounds of tests/test_gpu_smpl.py and tests/test_gpu_smpl_grad.py"""
    model = body_model(tree)
    body = smpl.BodyModel.from_arrays(renderer, model)
    NB, V = body.NB, body.V
    betas, pose, rotm, cot = make_inputs(B, NB, V, 0, 51)
    cot = {"joints": cot["joints"]}
    for form, p in (("axis", pose), ("rotmat", rotm)):
        want = sref.lbs(model, betas, p, pose2rot=form == "axis")
        joints = body.forward(betas, p, pose2rot=form == "axis", joints=True).joints.cpu().numpy()
        bound = sref.bound_chain(want["joints"], want["mag_joints"], links=depth_of(tree) + 1)
        print(f"[{tree}] {form} joints error / bound", float(np.max(np.abs(joints - want["joints"]) / bound)))
        assert np.all(np.abs(joints - want["joints"]) <= bound)
        wantg = gref.lbs_backward(model, betas, p, pose2rot=form == "axis", d_joints=cot["joints"])
        rc, got = abi_smpl_backward(renderer, body, betas, p, cot, rotmat=form == "rotmat")
        assert rc == 0
        check_smpl_backward(got, wantg, NB, 0, f"[{tree}] {form} d_joints")
        assert np.abs(wantg["d_pose"]).max() > 0 and np.abs(wantg["d_betas"]).max() > 0


@pytest.mark.gpu
@pytest.mark.parametrize("tree", list(TREES))
def test_pose_layer(renderer, tree):
    """pg_poseopt_forward and pg_poseopt_backward through the C ABI: the fp32 rule of tests/test_gpu_poseopt.py, without its escape to
    the fp32 reference's own deviation"""
    par = parents_of(tree, 0)
    par64 = par.astype(np.int64)
    c = random_case(B, [4, 1, 4, 0, 3, 3, 1, 2], seed=13)
    a = _abi_args(renderer, c)
    n = a["n"]
    outs = dict(rots=torch.empty(n, 24, 3, 3, device=DEV), l2ws=torch.empty(n, 24, 4, 4, device=DEV), skts=torch.empty(n, 24, 4, 4, device=DEV),
                kps=torch.empty(n, 24, 3, device=DEV))
    p = lambda x: C.c_void_p(x.data_ptr())
    r = renderer
    rc = r.lib.pg_poseopt_forward(r.handle, r._stream(), a["U"], 6, p(a["bones"]), p(a["pelvis"]), p(a["rest"]), 0, par.ctypes.data_as(_I32P), n,
                                  a["seg"].inverse.ctypes.data_as(_I32P), *[p(outs[k]) for k in ("rots", "l2ws", "skts", "kps")])
    torch.cuda.synchronize()
    assert rc == 0
    u = a["seg"].unique
    want = dict(zip(OUTS, pref.forward(c["bones"][u], c["pelvis"][u], c["rest"], a["seg"].inverse, parents=par64)))
    for k in OUTS:
        pref.check_rule(outs[k].cpu().numpy(), want[k], f"[{tree}] {k}")
    rc, db, dp = _backward_call(renderer, a, cot=[a["cot"][k] for k in ("rots", "l2ws", "skts", "kps")], parents=par)
    assert rc == 0
    wb, wp = pref.backward(c["bones"][u], c["pelvis"][u], c["rest"], a["seg"].inverse, **{f"d_{k}": c["cot"][k] for k in OUTS}, parents=par64)
    pref.check_rule(db, wb, f"[{tree}] d_bones")
    pref.check_rule(dp, wp, f"[{tree}] d_pelvis")
    assert np.abs(wb).max() > 0 and np.abs(wp).max() > 0
