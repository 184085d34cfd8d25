"""The float64 restatement of the differentiable key points and pose losses (tests/keypoint_grad_ref.py) without a GPU: its key
points against the package's host kinematics and the existing restatements, its autograd against finite differences at the edge
inputs the GPU tests use, the header's closed forms of the norm-matched gradient against autograd, and the Python layer's refusals."""
import os
import re

import numpy as np
import pytest
import torch

from posegen_amd import _ffi, skeleton as sk
from tests import keypoint_grad_ref as ref, smpl_ref

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REST32 = sk.smpl_rest_pose.astype(np.float32)


def edge_bones(B, seed):
    """[B,24,3] float64: seeded N(0, 0.3^2) with joints set to the zero vector, to lengths 5e-4 and 1.5e-3 (both sides of the
    small-angle switch) and 3.1 (near pi) -- on leaf joints, inner joints and the root"""
    rng = np.random.RandomState(seed)
    b = rng.normal(0, 0.3, (B, 24, 3))
    unit = lambda: (lambda v: v / np.linalg.norm(v))(rng.normal(size=3))
    for i in range(B):
        b[i, (3 * i) % 24] = 0.0
        b[i, (3 * i + 5) % 24] = 5e-4 * unit()
        b[i, (3 * i + 9) % 24] = 1.5e-3 * unit()
        b[i, (3 * i + 14) % 24] = 3.1 * unit()
    b[0, 0] = 0.0                                            # the root at zero
    b[0, 23] = 5e-4 * unit()                                 # a leaf of the longest chain below the switch
    return b


def noisy_rotmats(B, seed, noise=0.05):
    """[B,24,3,3] float32: orthogonal matrices plus `noise`"""
    rng = np.random.RandomState(seed)
    R = ref.rotvec_to_matrix(torch.from_numpy(rng.normal(0, 0.5, (B, 24, 3)))).numpy()
    return (R + rng.normal(0, noise, R.shape)).astype(np.float32)


def loss_poses(B, J_in, seed, noise=(0.05, 0.15, 0.6)):
    """pred, gt [B,J_in,3] float32: gt the key points of seeded poses at scale 0.4 (or their first J_in joints), pred the key points
    of the same rotations disturbed by noise[b % 3] rad -- per-pose values on both sides of 0.02 at weight 0.1"""
    rng = np.random.RandomState(seed)
    bones = rng.normal(0, 0.3, (B, 24, 3))
    level = np.asarray(noise)[np.arange(B) % len(noise)][:, None, None]
    gt = ref.kps_from_axis_angle(bones, REST32, 0.4).numpy()
    pred = ref.kps_from_axis_angle(bones + level * rng.normal(size=bones.shape), REST32, 0.4).numpy()
    pred = pred + rng.normal(0, 2e-3, pred.shape)            # (no joint of pred on its gt: the pelvis would be, and a distance of zero is a kink)
    return pred[:, :J_in].astype(np.float32), gt[:, :J_in].astype(np.float32)


def test_key_points_agree_with_the_host_kinematics():
    bones = edge_bones(5, 1)
    kps = ref.kps_from_axis_angle(bones, sk.smpl_rest_pose).numpy()
    assert np.abs(kps - sk.bones_to_pose(bones, sk.smpl_rest_pose)[0]).max() <= 1e-12
    g = np.load(os.path.join(REPO, "tests", "golden", "kinematics.npz"))
    assert np.abs(ref.kps_from_axis_angle(g["bones"], g["rest_pose"]).numpy() - sk.bones_to_pose(g["bones"], g["rest_pose"])[0]).max() <= 1e-12
    rot = noisy_rotmats(4, 2)
    assert np.abs(ref.kps_from_rotmats(rot, REST32, 0.4).numpy() - smpl_ref.rot_chain(rot, REST32, 0.4)[1]).max() <= 1e-12
    # both forms on the same rotations
    R = ref.rotvec_to_matrix(torch.from_numpy(bones))
    assert np.abs(R.numpy() - sk.rotvec_to_matrix(bones)).max() <= 1e-12
    assert np.abs(ref.kps_from_rotmats(R, sk.smpl_rest_pose, 1.0).numpy() - kps).max() <= 1e-12


def test_the_series_meets_the_direct_formulas_at_the_switch():
    for th in (9.99e-4, 5e-4, 1e-5):
        t2 = th * th
        # the truncation is below 1e-22; what is left is the rounding of either side, half an ulp of 1 each
        assert abs((0.5 - t2 / 48 + t2 * t2 / 3840) - np.sin(th / 2) / th) <= 2.3e-16
        assert abs((1 - t2 / 8 + t2 * t2 / 384) - np.cos(th / 2)) <= 2.3e-16


def test_axis_angle_gradient_against_finite_differences():
    bones = torch.from_numpy(edge_bones(2, 3)).requires_grad_(True)
    f = lambda b: ref.kps_from_axis_angle(b, REST32, 0.4)
    assert torch.autograd.gradcheck(f, (bones,), eps=1e-6, atol=1e-6)
    g, = torch.autograd.grad(f(bones).sum(), bones)
    assert torch.isfinite(g).all()
    zero = torch.zeros(1, 24, 3, dtype=torch.float64, requires_grad=True)
    gz, = torch.autograd.grad((f(zero) * torch.from_numpy(np.random.RandomState(0).uniform(-1, 1, (1, 24, 3)))).sum(), zero)
    assert torch.isfinite(gz).all() and gz.abs().max() > 1e-3               # the generators' gradient, not NaN and not nothing


def test_rotation_matrix_gradient_against_finite_differences():
    rot = torch.from_numpy(noisy_rotmats(2, 4).astype(np.float64)).requires_grad_(True)
    assert torch.autograd.gradcheck(lambda m: ref.kps_from_rotmats(m, REST32, 0.4), (rot,), eps=1e-6, atol=1e-6)


@pytest.mark.parametrize("kind", ["mpjpe", "norm_matched"])
@pytest.mark.parametrize("sel", ["14 of 24, root 0", "all of 14, no root"])
def test_loss_gradients_against_finite_differences(kind, sel):
    J_in, joints, root = (24, ref.GAN_JOINTS, 0) if sel.startswith("14 of 24") else (14, None, None)
    pred, gt = loss_poses(5, J_in, 5)
    p = torch.from_numpy(pred.astype(np.float64)).requires_grad_(True)
    g = torch.from_numpy(gt.astype(np.float64)).requires_grad_(True)
    for cap in (float("inf"), 0.02):
        f = lambda a, b: ref.pose_loss(a, b, joints, root, kind, 0.1, cap)[0]
        _, per_pose, n_kept = ref.pose_loss(p, g, joints, root, kind, 0.1, cap)
        assert np.isinf(cap) or (0 < n_kept < 5 and (per_pose.detach() - cap).abs().min() > 1e-4)      # (finite differences stay on one side)
        assert torch.autograd.gradcheck(f, (p, g), eps=1e-6, atol=1e-6)


def test_norm_matched_closed_forms_against_autograd():
    pred, gt = loss_poses(6, 24, 6)
    sel = [0] + ref.GAN_JOINTS                               # the root row inside the selection: a zero distance
    P = torch.from_numpy(pred.astype(np.float64)).requires_grad_(True)
    G = torch.from_numpy(gt.astype(np.float64)).requires_grad_(True)
    loss, per_pose, _ = ref.pose_loss(P, G, sel, 0, "norm_matched", 0.1)
    dP, dG = torch.autograd.grad(loss, (P, G))
    assert torch.isfinite(dP).all() and torch.isfinite(dG).all()
    c = 0.1 / (len(sel) * 6)
    for b in range(6):
        p, g = (ref.select(x.detach(), sel, 0)[b].numpy() for x in (P, G))
        dp, dg = ref.norm_matched_closed_form(p, g, c)
        assert np.abs(dp - dP[b, sel].numpy())[1:].max() <= 1e-12 and np.abs(dg - dG[b, sel].numpy())[1:].max() <= 1e-12
        assert np.all(dp[0] == 0) and np.all(dg[0] == 0)                                   # the zero distance gives a zero gradient
        assert np.abs(dP[b, 0].numpy() + dp.sum(0)).max() <= 1e-12 and np.abs(dG[b, 0].numpy() + dg.sum(0)).max() <= 1e-12
        rest = [j for j in range(24) if j not in sel]
        assert np.all(dP[b, rest].numpy() == 0) and np.all(dG[b, rest].numpy() == 0)
    # pred == gt exactly: every distance zero, every gradient zero, in both kinds
    for kind in ("mpjpe", "norm_matched"):
        loss = ref.pose_loss(P, P.detach().clone(), sel, 0, kind)[0]
        assert float(loss.detach()) == 0.0 and np.all(torch.autograd.grad(loss, P)[0].numpy() == 0)


def test_kept_set_and_empty_mean():
    pred, gt = loss_poses(6, 24, 7)
    loss, per_pose, n_kept = ref.pose_loss(pred, gt, ref.GAN_JOINTS, 0, "norm_matched", 0.1, 0.02)
    pp = per_pose.numpy()
    assert 0 < n_kept < 6 and n_kept == int((pp < 0.02).sum()) and abs(float(loss) - pp[pp < 0.02].mean()) <= 1e-15
    loss, _, n_kept = ref.pose_loss(pred, gt, ref.GAN_JOINTS, 0, "norm_matched", 0.1, 1e-9)
    assert n_kept == 0 and np.isnan(float(loss))
    bad = pred.copy()
    bad[2] = np.nan
    loss, per_pose, n_kept = ref.pose_loss(bad, gt, ref.GAN_JOINTS, 0, "mpjpe", 1.0, 10.0)
    assert n_kept == 5 and np.isfinite(float(loss)) and np.isnan(float(per_pose[2]))
    assert np.isnan(float(ref.pose_loss(bad, gt, ref.GAN_JOINTS, 0, "mpjpe")[0]))


def test_header_binding_and_package_export_the_entry_points():
    hdr = open(os.path.join(REPO, "include", "posegen_hip.h")).read()
    flat = re.sub(r"\s+", " ", hdr)
    assert ("int pg_pose_kinematics_bwd(pg_handle* h, void* stream, int64_t n_poses, const double* bones, const double* bone_offsets, "
            "const int32_t* parents, const float* d_kps, double* d_bones);") in flat
    assert ("int pg_pose_kinematics_rot_bwd(pg_handle* h, void* stream, int64_t n_poses, const float* rotmats, const double* bone_offsets, "
            "const int32_t* parents, const float* d_kps, float* d_rotmats);") in flat
    assert ("int pg_pose_loss(pg_handle* h, void* stream, int64_t B, int J_in, const float* pred, const float* gt, const int32_t* joints, int J, "
            "int root, int kind, double weight, double cap, double* per_pose, double* summary, float* d_pred, float* d_gt);") in flat
    for name, code in (("MPJPE", 0), ("NORM_MATCHED", 1)):
        assert re.search(rf"#define\s+PG_POSE_LOSS_{name}\s+{code}\b", hdr) and getattr(_ffi, f"PG_POSE_LOSS_{name}") == code
    assert re.search(r"#define\s+PG_ABI_VERSION\s+11\b", hdr) and _ffi.PG_ABI_VERSION == 11      # added entry points do not move it
    assert [len(_ffi.PROTOTYPES[n][1]) for n in ("pg_pose_kinematics_bwd", "pg_pose_kinematics_rot_bwd", "pg_pose_loss")] == [8, 8, 16]
    lib = _ffi.load_library()
    assert lib.pg_abi_version() == 11
    # a NULL handle is refused before anything else is looked at
    assert lib.pg_pose_kinematics_bwd(None, None, 1, None, None, None, None, None) == _ffi.PG_EINVAL
    assert lib.pg_pose_kinematics_rot_bwd(None, None, 1, None, None, None, None, None) == _ffi.PG_EINVAL
    assert lib.pg_pose_loss(None, None, 1, 14, None, None, None, 14, -1, 0, 1.0, 1.0, None, None, None, None) == _ffi.PG_EINVAL
    import posegen_amd
    from posegen_amd import ganloop, pose_losses
    for name in ("keypoints_from_axis_angle", "keypoints_from_rotmats", "pose_loss"):
        assert getattr(posegen_amd, name) is getattr(pose_losses, name)
    assert callable(ganloop.generator_feedback) and callable(ganloop.regressor_loss)


def test_there_is_no_cpu_path():
    from types import SimpleNamespace

    from posegen_amd import ganloop, pose_losses
    kps = torch.zeros(2, 24, 3)
    with pytest.raises(NotImplementedError):
        pose_losses.pose_loss(kps, kps)                                             # host tensors and no renderer
    with pytest.raises(NotImplementedError):
        pose_losses.pose_loss(kps.numpy(), kps.numpy())
    cpu = SimpleNamespace(device="cpu")
    with pytest.raises(NotImplementedError):
        pose_losses.pose_loss(kps, kps, renderer=cpu)
    with pytest.raises(NotImplementedError):
        pose_losses.keypoints_from_axis_angle(cpu, torch.zeros(2, 24, 3), REST32)
    with pytest.raises(NotImplementedError):
        pose_losses.keypoints_from_rotmats(cpu, torch.zeros(2, 24, 3, 3))
    with pytest.raises(NotImplementedError):
        ganloop.generator_feedback(cpu, kps, torch.zeros(2, 24, 3, requires_grad=True))
    with pytest.raises(NotImplementedError):
        ganloop.regressor_loss(cpu, torch.zeros(2, 24, 3, 3, requires_grad=True), kps)


def test_refusals_come_before_the_library():
    from types import SimpleNamespace

    from posegen_amd import pose_losses
    gpu = SimpleNamespace(device="cuda:0")                   # nothing below reaches it
    kps = torch.zeros(2, 24, 3)
    with pytest.raises(ValueError):
        pose_losses.pose_loss(kps, kps, kind="procrustes", renderer=gpu)
    with pytest.raises(ValueError):
        pose_losses.pose_loss(kps, torch.zeros(2, 14, 3), renderer=gpu)
    with pytest.raises(ValueError):
        pose_losses.pose_loss(kps, kps, joints=[1, 2, 1], renderer=gpu)
    with pytest.raises(IndexError):
        pose_losses.pose_loss(kps, kps, joints=[1, 24], renderer=gpu)
    with pytest.raises(IndexError):
        pose_losses.pose_loss(kps, kps, root=24, renderer=gpu)
    with pytest.raises(ValueError):
        pose_losses.pose_loss(torch.zeros(2, 65, 3), torch.zeros(2, 65, 3), renderer=gpu)
    for weight, cap in ((float("nan"), 1.0), (1.0, float("nan")), (1.0, 0.0), (1.0, -1.0)):
        with pytest.raises(ValueError):
            pose_losses.pose_loss(kps, kps, weight=weight, cap=cap, renderer=gpu)
    with pytest.raises(ValueError):
        pose_losses.keypoints_from_axis_angle(gpu, torch.zeros(2, 23, 3), REST32)
    with pytest.raises(ValueError):
        pose_losses.keypoints_from_rotmats(gpu, torch.zeros(2, 24, 3))
