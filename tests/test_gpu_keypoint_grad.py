"""pg_pose_kinematics_bwd, pg_pose_kinematics_rot_bwd and pg_pose_loss on the GPU, through the C ABI and through
posegen_amd.pose_losses / ganloop, against the float64 torch restatement and its autograd (tests/keypoint_grad_ref.py).

Bounds (as 2.10's): a few hundred float64 operations with device sin / cos / sqrt within ulps, margin >= 100 --
float64 outputs within 1e-10 max(1, |value|) of the restatement; float32 outputs within one float32 ulp of the restatement's value
rounded to float32, plus 1e-10.  n_kept exactly, on inputs whose finite per-pose values stay 1e-6 (relative) clear of the cap.
End to end the restatement rounds where the interface does: key points to float32 on their way into the loss, their cotangent to
float32 on its way back (keypoint_grad_ref.as_float32_interface).
Measured on an MI355X: worst error over bound 1.2e-5 (d_bones, B = 67, dense cotangent); every float32 output equal to the rounded
restatement."""
import ctypes as C
import math

import numpy as np
import pytest
import torch

from posegen_amd import _ffi, ganloop, pose_losses
from tests import keypoint_grad_ref as ref
from tests.frame_metrics_gpu import DEV, renderer  # noqa: F401 (renderer: a fixture)
from tests.test_keypoint_grad_ref import REST32, edge_bones, loss_poses, noisy_rotmats

pytestmark = pytest.mark.gpu
EINVAL = _ffi.PG_EINVAL
SENTINEL = -7.0
INF = float("inf")
SCALE = 0.4
BATCHES = (1, 3, 67)                                         # one wave, a partly filled block, 17 blocks (the grid is never capped)
COTANGENTS = ("dense", "leaf 22", "leaf 23", "root", "zero")


def assert_f64(got, want, what):
    err, tol = np.abs(got - want), 1e-10 * np.maximum(1.0, np.abs(want))
    print(f"{what}: worst error / bound {float((err / tol).max()):.3e}")
    assert np.all(err <= tol), (what, float((err / tol).max()))


def assert_f32(got32, want64, what):
    assert got32.dtype == np.float32
    want32 = np.asarray(want64).astype(np.float32)
    err = np.abs(got32.astype(np.float64) - want32.astype(np.float64))
    tol = np.spacing(np.abs(want32)).astype(np.float64) + 1e-10
    print(f"{what}: worst error / bound {float((err / tol).max()):.3e}")
    assert np.all(err <= tol), (what, float((err / tol).max()))


def offsets(root_parent):
    offs, par = ref.bone_offsets(REST32, SCALE)
    par = par.astype(np.int32)
    par[0] = root_parent
    return np.ascontiguousarray(offs), np.ascontiguousarray(par)


def guarded(shape, dtype):
    return torch.full((int(np.prod(shape)) + 1,), SENTINEL, dtype=dtype, device=DEV)


def abi_kin_bwd(r, params, d_kps, axis, n=None, null=(), parents=None):
    """the transpose through the C ABI -> (return code, numpy gradient of params' shape); the output starts filled with SENTINEL
    and has one guard element behind it"""
    offs, par = offsets(0 if axis else -1)
    if parents is not None:
        par = np.ascontiguousarray(parents, dtype=np.int32)
    out = guarded(params.shape, params.dtype)
    ptr = lambda name, t: None if name in null else C.c_void_p(t.data_ptr())
    fn = r.lib.pg_pose_kinematics_bwd if axis else r.lib.pg_pose_kinematics_rot_bwd
    rc = fn(r.handle, r._stream(), params.shape[0] if n is None else n, ptr("params", params),
            None if "offs" in null else offs.ctypes.data_as(C.POINTER(C.c_double)),
            None if "parents" in null else par.ctypes.data_as(C.POINTER(C.c_int32)), ptr("d_kps", d_kps), ptr("out", out))
    torch.cuda.synchronize()
    host = out.cpu().numpy()
    assert host[-1] == SENTINEL, "the element behind the output was written"
    return rc, host[:-1].reshape(tuple(params.shape))


def cotangent(B, kind, seed=0):
    rng = np.random.RandomState(seed)
    g = np.zeros((B, 24, 3), np.float32)
    if kind == "dense":
        g = rng.uniform(-1, 1, g.shape).astype(np.float32)
    elif kind.startswith("leaf"):
        g[:, int(kind.split()[1])] = rng.uniform(-1, 1, (B, 3))
    elif kind == "root":
        g[:, 0] = rng.uniform(-1, 1, (B, 3))
    return g


@pytest.fixture(scope="module")
def kin_reference():
    """per B: the parameters of both forms, and per cotangent the restatement's float64 gradients -- computed once"""
    out = {}
    for B in BATCHES:
        bones = edge_bones(B, 10 + B)
        rot = noisy_rotmats(B, 20 + B)
        b = torch.from_numpy(bones).requires_grad_(True)
        m = torch.from_numpy(rot.astype(np.float64)).requires_grad_(True)
        kb, km = ref.kps_from_axis_angle(b, REST32, SCALE), ref.kps_from_rotmats(m, REST32, SCALE)
        grads = {}
        for kind in COTANGENTS:
            g = torch.from_numpy(cotangent(B, kind).astype(np.float64))
            grads[kind] = (torch.autograd.grad(kb, b, g, retain_graph=True)[0].numpy(), torch.autograd.grad(km, m, g, retain_graph=True)[0].numpy())
        out[B] = dict(bones=bones, rot=rot, grads=grads)
    return out


@pytest.mark.parametrize("B", BATCHES)
def test_axis_angle_backward(renderer, kin_reference, B):
    c = kin_reference[B]
    bones = torch.from_numpy(c["bones"]).to(DEV)
    kps = renderer.pose_kinematics(bones, REST32 * np.float32(SCALE))[0].cpu().numpy()       # the forward the transpose belongs to
    assert_f32(kps, ref.kps_from_axis_angle(c["bones"], REST32, SCALE).numpy(), f"B={B} forward")
    for kind in COTANGENTS:
        rc, got = abi_kin_bwd(renderer, bones, torch.from_numpy(cotangent(B, kind)).to(DEV), True)
        assert rc == 0 and np.all(np.isfinite(got))
        assert_f64(got, c["grads"][kind][0], f"B={B} {kind}")
        if kind == "zero":
            assert np.all(got == 0.0)
    assert np.abs(got_at_zero_rotation(renderer)).max() > 1e-3


def got_at_zero_rotation(r):
    """the gradient at an all-zero pose: finite, and the rotation generators' (not zero)"""
    bones = torch.zeros(1, 24, 3, dtype=torch.float64, device=DEV)
    g = cotangent(1, "dense", 3)
    rc, got = abi_kin_bwd(r, bones, torch.from_numpy(g).to(DEV), True)
    b = torch.zeros(1, 24, 3, dtype=torch.float64, requires_grad=True)
    want = torch.autograd.grad(ref.kps_from_axis_angle(b, REST32, SCALE), b, torch.from_numpy(g.astype(np.float64)))[0].numpy()
    assert rc == 0 and np.all(np.isfinite(got))
    assert_f64(got, want, "zero pose")
    return got


@pytest.mark.parametrize("B", BATCHES)
def test_rotation_matrix_backward(renderer, kin_reference, B):
    c = kin_reference[B]
    rot = torch.from_numpy(c["rot"]).to(DEV)
    kps = renderer.pose_kinematics_rot(rot, REST32, scale=SCALE)[0].cpu().numpy()
    assert_f32(kps, ref.kps_from_rotmats(c["rot"], REST32, SCALE).numpy(), f"B={B} forward")
    for kind in COTANGENTS:
        rc, got = abi_kin_bwd(renderer, rot, torch.from_numpy(cotangent(B, kind)).to(DEV), False)
        assert rc == 0 and np.all(np.isfinite(got))
        assert_f32(got, c["grads"][kind][1], f"B={B} {kind}")
        if kind == "zero":
            assert np.all(got == 0.0)


@pytest.mark.parametrize("axis", [True, False])
def test_backward_keeps_a_pose_to_itself_and_repeats(renderer, kin_reference, axis):
    c = kin_reference[67]
    params = torch.from_numpy(c["bones"] if axis else c["rot"]).to(DEV)
    g = cotangent(67, "dense")
    rc, whole = abi_kin_bwd(renderer, params, torch.from_numpy(g).to(DEV), axis)
    rc2, again = abi_kin_bwd(renderer, params, torch.from_numpy(g).to(DEV), axis)
    assert rc == 0 and rc2 == 0 and whole.tobytes() == again.tobytes()                     # two calls, the same bytes
    for k in (0, 13, 66):                                                                  # a pose alone and inside the batch
        rc, alone = abi_kin_bwd(renderer, params[k:k + 1].contiguous(), torch.from_numpy(g[k:k + 1]).to(DEV), axis)
        assert rc == 0 and alone.tobytes() == whole[k:k + 1].tobytes()
    # one pose with a NaN cotangent: only its rows are non-finite, the others keep their bytes
    bad = g.copy()
    bad[13, 20, 1] = np.nan
    rc, got = abi_kin_bwd(renderer, params, torch.from_numpy(bad).to(DEV), axis)
    assert rc == 0 and not np.all(np.isfinite(got[13]))
    keep = np.arange(67) != 13
    assert got[keep].tobytes() == whole[keep].tobytes()
    # a non-finite parameter likewise
    p_bad = params.clone()
    p_bad[40, 3] = float("nan")
    rc, got = abi_kin_bwd(renderer, p_bad, torch.from_numpy(g).to(DEV), axis)
    keep = np.arange(67) != 40
    assert rc == 0 and not np.all(np.isfinite(got[40])) and got[keep].tobytes() == whole[keep].tobytes()


@pytest.mark.parametrize("axis", [True, False])
def test_backward_refusals_write_nothing(renderer, kin_reference, axis):
    c = kin_reference[3]
    params = torch.from_numpy(c["bones"] if axis else c["rot"]).to(DEV)
    g = torch.from_numpy(cotangent(3, "dense")).to(DEV)
    _, good = offsets(0)
    unordered = good.copy()
    unordered[5] = 7
    cases = [dict(null=(name,)) for name in ("params", "offs", "parents", "d_kps", "out")] + [dict(n=-1), dict(parents=unordered)]
    for kw in cases:
        rc, got = abi_kin_bwd(renderer, params, g, axis, **kw)
        assert rc == EINVAL and np.all(got == SENTINEL), kw
    who = b"pg_pose_kinematics_bwd" if axis else b"pg_pose_kinematics_rot_bwd"
    assert who in renderer.lib.pg_last_error(renderer.handle)
    rc, got = abi_kin_bwd(renderer, params, g, axis, n=0)                                  # no poses: nothing to do, nothing written
    assert rc == 0 and np.all(got == SENTINEL)


# ---- the losses -----------------------------------------------------------------------------------------------------------------------
def abi_loss(r, pred, gt, joints=None, root=-1, kind=0, weight=1.0, cap=INF, J=None, B=None, J_in=None, null=()):
    """pg_pose_loss through the C ABI on device tensors -> (return code, dict of numpy outputs), sentinels and guards as above"""
    Bv, Jin = pred.shape[:2]
    out = {"per_pose": guarded((Bv,), torch.float64), "summary": guarded((3,), torch.float64),
           "d_pred": guarded(pred.shape, torch.float32), "d_gt": guarded(pred.shape, torch.float32)}
    ptr = lambda name, t: None if name in null else C.c_void_p(t.data_ptr())
    jarr = None if joints is None else (C.c_int32 * len(joints))(*joints)
    Jv = (len(joints) if joints is not None else Jin) if J is None else J
    rc = r.lib.pg_pose_loss(r.handle, r._stream(), Bv if B is None else B, Jin if J_in is None else J_in, ptr("pred", pred), ptr("gt", gt), jarr, Jv,
                            root, kind, weight, cap, ptr("per_pose", out["per_pose"]), ptr("summary", out["summary"]),
                            ptr("d_pred", out["d_pred"]), ptr("d_gt", out["d_gt"]))
    torch.cuda.synchronize()
    host = {k: v.cpu().numpy() for k, v in out.items()}
    for k, v in host.items():
        assert v[-1] == SENTINEL, f"{k}: the element behind the output was written"
    shapes = {"per_pose": (Bv,), "summary": (3,), "d_pred": tuple(pred.shape), "d_gt": tuple(pred.shape)}
    return rc, {k: v[:-1].reshape(shapes[k]) for k, v in host.items()}


def reference_loss(pred, gt, joints, root, kind, weight, cap):
    """the restatement on float32 inputs: loss, per_pose, n_kept, d_pred, d_gt (float64 numpy); the gradients are zero where nothing
    is kept"""
    P = torch.from_numpy(pred.astype(np.float64)).requires_grad_(True)
    G = torch.from_numpy(gt.astype(np.float64)).requires_grad_(True)
    loss, per_pose, n_kept = ref.pose_loss(P, G, joints, None if root < 0 else root, kind, weight, cap)
    dP, dG = torch.autograd.grad(loss, (P, G)) if n_kept else (torch.zeros_like(P), torch.zeros_like(G))
    return float(loss.detach()), per_pose.detach().numpy(), n_kept, dP.numpy(), dG.numpy()


def clear_of(per_pose, cap):
    v = per_pose[np.isfinite(per_pose)]
    return np.isinf(cap) or np.all(np.abs(v - cap) >= 1e-6 * cap)


def check_loss(r, pred, gt, joints, root, kind, weight, cap, what, finite_poses=None):
    """one call against the restatement; finite_poses: the poses whose gradient rows are compared (None: all)"""
    rc, got = abi_loss(r, torch.from_numpy(pred).to(DEV), torch.from_numpy(gt).to(DEV), joints, root, ref.KINDS[kind], weight, cap)
    assert rc == 0, r.lib.pg_last_error(r.handle)
    loss, per_pose, n_kept, dP, dG = reference_loss(pred, gt, joints, root, kind, weight, cap)
    assert clear_of(per_pose, cap), (what, "a per-pose value sits on the cap")
    print(what, "loss", got["summary"][0], "n_kept", got["summary"][1], "of", got["summary"][2])
    assert got["summary"][1] == n_kept and got["summary"][2] == len(pred)
    fin = np.isfinite(per_pose)
    assert np.array_equal(np.isnan(got["per_pose"]), np.isnan(per_pose))
    assert_f64(got["per_pose"][fin], per_pose[fin], what + " per_pose")
    if np.isnan(loss):
        assert np.isnan(got["summary"][0])
    else:
        assert_f64(got["summary"][:1], np.array([loss]), what + " loss")
    rows = np.arange(len(pred)) if finite_poses is None else np.asarray(finite_poses)
    assert_f32(got["d_pred"][rows], dP[rows], what + " d_pred")
    assert_f32(got["d_gt"][rows], dG[rows], what + " d_gt")
    # exactly zero: the rows that are not selected (the root's aside) and the poses that are not kept
    unselected = [j for j in range(pred.shape[1]) if joints is not None and j not in joints and j != root]
    dropped = ~(per_pose < cap) if np.isfinite(cap) else np.zeros(len(pred), bool)
    for d in (got["d_pred"], got["d_gt"]):
        assert np.all(d[rows][:, unselected] == 0.0) and np.all(d[dropped] == 0.0)
    return got


SELECTIONS = {"14 of 24, root 0": (24, ref.GAN_JOINTS, 0), "all of 14, no root": (14, None, -1)}


@pytest.mark.parametrize("kind", ["mpjpe", "norm_matched"])
@pytest.mark.parametrize("sel", list(SELECTIONS))
@pytest.mark.parametrize("B", [1, 2, 5, 130])
def test_pose_loss(renderer, B, sel, kind):
    J_in, joints, root = SELECTIONS[sel]
    pred, gt = loss_poses(B, J_in, 30 + B)
    kept = {}
    for cap in (INF, 1e3, 0.02, 1e-9):                       # all (two ways), some, none
        got = check_loss(renderer, pred, gt, joints, root, kind, 0.1, cap, f"B={B} {sel} {kind} cap={cap}")
        kept[cap] = int(got["summary"][1])
    assert kept[INF] == kept[1e3] == B and kept[1e-9] == 0
    assert B < 5 or 0 < kept[0.02] < B                       # noise levels on both sides of 0.02
    rc, got = abi_loss(renderer, torch.from_numpy(pred).to(DEV), torch.from_numpy(gt).to(DEV), joints, root, ref.KINDS[kind], 0.1, 1e-9)
    assert rc == 0 and np.isnan(got["summary"][0]) and np.all(got["d_pred"] == 0.0) and np.all(got["d_gt"] == 0.0)


@pytest.mark.parametrize("kind", ["mpjpe", "norm_matched"])
def test_pose_loss_edge_poses(renderer, kind):
    pred, gt = loss_poses(5, 24, 41)
    with_root = [0] + ref.GAN_JOINTS                         # the root row selected: a zero distance, a finite zero gradient of its own
    check_loss(renderer, pred, gt, with_root, 0, kind, 0.1, INF, f"{kind} root selected")
    other = [23, 3, 9, 14, 6, 17, 20]                        # another order, the root outside it
    check_loss(renderer, pred, gt, other, 11, kind, 1.0, 0.5, f"{kind} another selection")
    same = pred.copy()
    same[1] = gt[1]                                          # pred == gt exactly
    got = check_loss(renderer, same, gt, ref.GAN_JOINTS, 0, kind, 0.1, INF, f"{kind} pred == gt")
    assert got["per_pose"][1] == 0.0 and np.all(got["d_pred"][1] == 0.0) and np.all(got["d_gt"][1] == 0.0)
    # outputs that may be NULL; two calls, the same bytes
    dev = lambda a: torch.from_numpy(a).to(DEV)
    rc, full = abi_loss(renderer, dev(pred), dev(gt), ref.GAN_JOINTS, 0, ref.KINDS[kind], 0.1, 0.02)
    rc2, again = abi_loss(renderer, dev(pred), dev(gt), ref.GAN_JOINTS, 0, ref.KINDS[kind], 0.1, 0.02)
    assert rc == 0 and rc2 == 0 and all(full[k].tobytes() == again[k].tobytes() for k in full)
    rc, part = abi_loss(renderer, dev(pred), dev(gt), ref.GAN_JOINTS, 0, ref.KINDS[kind], 0.1, 0.02, null=("per_pose", "d_gt"))
    assert rc == 0 and np.all(part["per_pose"] == SENTINEL) and np.all(part["d_gt"] == SENTINEL)
    assert part["summary"].tobytes() == full["summary"].tobytes() and part["d_pred"].tobytes() == full["d_pred"].tobytes()
    rc, none = abi_loss(renderer, dev(pred), dev(gt), ref.GAN_JOINTS, 0, ref.KINDS[kind], 0.1, 0.02, null=("d_pred", "d_gt"))
    assert rc == 0 and none["summary"].tobytes() == full["summary"].tobytes() and np.all(none["d_pred"] == SENTINEL)


def test_pose_loss_non_finite_poses(renderer):
    pred, gt = loss_poses(5, 24, 42, noise=(0.05, 0.1, 0.15))
    others = [0, 1, 3, 4]
    # |p| = 0 under norm-matching: every selected row on the root -- that pose only is NaN, and a finite cap drops it
    flat = pred.copy()
    flat[2] = flat[2, 0]
    got = check_loss(renderer, flat, gt, ref.GAN_JOINTS, 0, "norm_matched", 0.1, 0.05, "|p| = 0, finite cap", finite_poses=others)
    assert np.isnan(got["per_pose"][2]) and np.all(np.isfinite(got["per_pose"][others])) and np.isfinite(got["summary"][0]) and got["summary"][1] == 4
    got = check_loss(renderer, flat, gt, ref.GAN_JOINTS, 0, "norm_matched", 0.1, INF, "|p| = 0, cap = inf", finite_poses=others)
    assert np.isnan(got["summary"][0]) and got["summary"][1] == 5
    check_loss(renderer, flat, gt, ref.GAN_JOINTS, 0, "mpjpe", 0.1, INF, "|p| = 0, mpjpe: an ordinary pose")
    # a NaN pose: under a finite cap the loss and the other poses are what they are without it
    bad = pred.copy()
    bad[2, 7, 1] = np.nan
    for kind in ("mpjpe", "norm_matched"):
        got = check_loss(renderer, bad, gt, ref.GAN_JOINTS, 0, kind, 0.1, 0.05, f"{kind} NaN pose, finite cap", finite_poses=others)
        assert got["summary"][1] == 4 and np.isfinite(got["summary"][0])
        rc, clean = abi_loss(renderer, torch.from_numpy(pred[others]).to(DEV), torch.from_numpy(gt[others]).to(DEV), ref.GAN_JOINTS, 0, ref.KINDS[kind], 0.1, 0.05)
        assert rc == 0 and clean["d_pred"].tobytes() == got["d_pred"][others].tobytes()
        assert_f64(got["summary"][:1], clean["summary"][:1], f"{kind} the loss without the NaN pose")      # (four values summed in another order)
        got = check_loss(renderer, bad, gt, ref.GAN_JOINTS, 0, kind, 0.1, INF, f"{kind} NaN pose, cap = inf", finite_poses=others)
        assert np.isnan(got["summary"][0]) and got["summary"][1] == 5
    # a NaN in a row that is neither selected nor the root is not read
    unread = pred.copy()
    unread[2, 3, 0] = np.nan
    got = check_loss(renderer, unread, gt, ref.GAN_JOINTS, 0, "mpjpe", 0.1, INF, "NaN in an unselected row")
    assert np.isfinite(got["summary"][0])


def test_pose_loss_refusals_write_nothing(renderer):
    pred, gt = (torch.from_numpy(a).to(DEV) for a in loss_poses(3, 24, 43))
    nan = float("nan")
    cases = [dict(null=("pred",)), dict(null=("gt",)), dict(null=("summary",)), dict(B=0), dict(B=-2), dict(J_in=0),
             dict(joints=[1], J=0), dict(joints=list(range(24)) * 3, J=65), dict(joints=[1, 24]), dict(joints=[-1, 2]), dict(joints=[1, 2, 1]),
             dict(root=24), dict(root=-2), dict(kind=2), dict(kind=-1), dict(weight=nan), dict(cap=nan), dict(cap=0.0), dict(cap=-1.0),
             dict(cap=-INF)]
    for kw in cases:
        rc, got = abi_loss(renderer, pred, gt, **kw)
        assert rc == EINVAL, kw
        assert all(np.all(v == SENTINEL) for v in got.values()), kw
    assert b"pg_pose_loss" in renderer.lib.pg_last_error(renderer.handle)
    wide = torch.zeros(2, 65, 3, device=DEV)
    rc, got = abi_loss(renderer, wide, wide)                 # joints = NULL selects all 65
    assert rc == EINVAL and all(np.all(v == SENTINEL) for v in got.values())


# ---- end to end -----------------------------------------------------------------------------------------------------------------------
def graph_nodes(t):
    seen, todo = [], [t.grad_fn]
    while todo:
        f = todo.pop()
        if f is None or f in seen:
            continue
        seen.append(f)
        todo += [n for n, _ in f.next_functions]
    return [type(f).__name__ for f in seen]


def test_generator_feedback_trains_the_generator(renderer):
    B = 9
    bones_np = edge_bones(B, 50).astype(np.float32)
    pred_np = loss_poses(B, 24, 51)[0]
    bones = torch.from_numpy(bones_np).to(DEV).requires_grad_(True)
    pred = torch.from_numpy(pred_np).to(DEV)
    out = ganloop.generator_feedback(renderer, pred, bones)
    assert out.dtype == torch.float64 and out.dim() == 0 and out.is_cuda
    # two library calls in backward, not torch's chain: nothing between the loss and the leaf but the two functions
    names = graph_nodes(out)
    assert names.count("_PoseLossFnBackward") == 1 and names.count("_AxisAngleFnBackward") == 1 and "AccumulateGrad" in names and len(names) <= 5, names
    out.backward()
    assert bones.grad.dtype == torch.float32 and bones.grad.device == bones.device
    b = torch.from_numpy(bones_np.astype(np.float64)).requires_grad_(True)
    want = ref.generator_feedback(pred_np, b)
    assert_f64(np.array([float(out.detach().cpu())]), np.array([float(want.detach())]), "generator feedback")
    want.backward()
    assert_f32(bones.grad.cpu().numpy(), b.grad.numpy(), "d generator_feedback / d bones")
    assert float(bones.grad.abs().max()) > 0 and bool(torch.isfinite(bones.grad).all())    # (zero vectors among the bones: finite there)
    # the existing number is the same number
    assert_f64(np.array([float(ganloop.regressor_feedback(pred, ref.kps_from_axis_angle(bones_np, REST32, SCALE).to(torch.float32).to(DEV)).cpu())]),
               np.array([float(want.detach())]), "regressor_feedback")
    with pytest.raises(RuntimeError):                        # differentiable once
        b2 = torch.from_numpy(bones_np).to(DEV).requires_grad_(True)
        g, = torch.autograd.grad(ganloop.generator_feedback(renderer, pred, b2), b2, create_graph=True)
        g.sum().backward()


@pytest.mark.parametrize("gt_form", ["key points", "axis-angle"])
def test_regressor_loss_trains_the_regressor(renderer, gt_form):
    B = 12
    rng = np.random.RandomState(60)
    bones_gt = rng.normal(0, 0.3, (B, 24, 3)).astype(np.float32)
    level = np.asarray((0.05, 0.15, 0.6))[np.arange(B) % 3][:, None, None]
    rot_np = ref.rotvec_to_matrix(torch.from_numpy(bones_gt.astype(np.float64) + level * rng.normal(size=bones_gt.shape))).numpy()
    rot_np = (rot_np + rng.normal(0, 0.01, rot_np.shape)).astype(np.float32)                # a regressor's output is not quite orthogonal
    if gt_form == "key points":
        gt_np, kw = ref.kps_from_axis_angle(bones_gt, REST32, SCALE).numpy().astype(np.float32), dict()
    else:
        gt_np, kw = bones_gt, dict(gt_is_axis_angle=True, cap=math.inf)
    rot = torch.from_numpy(rot_np).to(DEV).requires_grad_(True)
    loss = ganloop.regressor_loss(renderer, rot, torch.from_numpy(gt_np).to(DEV), **kw)
    names = graph_nodes(loss)
    assert names.count("_PoseLossFnBackward") == 1 and names.count("_RotmatFnBackward") == 1 and len(names) <= 4, names
    m = torch.from_numpy(rot_np.astype(np.float64)).requires_grad_(True)
    want = ref.regressor_loss(m, gt_np, **kw)
    _, per_pose, n_kept = ref.pose_loss(ref.kps_from_rotmats(rot_np, REST32, SCALE).to(torch.float32), ref.kps_from_axis_angle(bones_gt, REST32, SCALE).to(torch.float32),
                                        ref.GAN_JOINTS, 0, "norm_matched", 0.1, kw.get("cap", 0.02))
    assert clear_of(per_pose.numpy(), kw.get("cap", 0.02)) and (gt_form == "axis-angle" or 0 < n_kept < B)
    assert_f64(np.array([float(loss.detach().cpu())]), np.array([float(want.detach())]), "regressor loss")
    loss.backward()
    want.backward()
    assert rot.grad.dtype == torch.float32 and rot.grad.shape == rot.shape
    assert_f32(rot.grad.cpu().numpy(), m.grad.numpy(), "d regressor_loss / d pred_rotmat")
    if gt_form != "key points":
        return
    # an upstream factor scales the gradients.  The key points' float32 cotangent d is rounded again after the factor:
    # |round(0.1 d) - 0.1 d| <= 2^-24 |0.1 d| on each of 72 entries, through lever arms below 2 (the scaled skeleton's longest
    # chain), on top of the two results' own float32 roundings
    g1 = rot.grad.cpu().numpy().astype(np.float64)
    rot.grad = None
    (0.1 * ganloop.regressor_loss(renderer, rot, torch.from_numpy(gt_np).to(DEV), **kw)).backward()
    kps = pose_losses.keypoints_from_rotmats(renderer, rot.detach().requires_grad_(True))
    kps.retain_grad()
    pose_losses.pose_loss(kps, torch.from_numpy(gt_np).to(DEV), joints=ref.GAN_JOINTS, root=0, kind="norm_matched", weight=0.1, cap=0.02,
                          renderer=renderer).backward()
    d_max = float(kps.grad.abs().max().cpu())
    err = np.abs(rot.grad.cpu().numpy().astype(np.float64) - 0.1 * g1)
    tol = 1.1 * np.spacing(np.abs(g1).astype(np.float32)).astype(np.float64) + 1e-10 + 72 * 2.0 * 2.0 ** -24 * 0.1 * d_max
    print("scaled: worst error / bound", float((err / tol).max()))
    assert d_max > 0 and np.all(err <= tol), float((err / tol).max())


def test_pose_loss_function(renderer):
    pred_np, gt_np = loss_poses(6, 24, 70)
    pred = torch.from_numpy(pred_np).to(DEV).requires_grad_(True)
    gt = torch.from_numpy(gt_np).to(DEV).requires_grad_(True)
    loss, per_pose, n_kept = pose_losses.pose_loss(pred, gt, joints=ref.GAN_JOINTS, root=0, kind="norm_matched", weight=0.1, cap=0.02,
                                                   renderer=renderer, return_stats=True)
    want, pp, nk, dP, dG = reference_loss(pred_np, gt_np, ref.GAN_JOINTS, 0, "norm_matched", 0.1, 0.02)
    assert not per_pose.requires_grad and not n_kept.requires_grad and float(n_kept.cpu()) == nk
    assert_f64(per_pose.cpu().numpy(), pp, "per_pose")
    loss.backward(retain_graph=True)
    assert_f32(pred.grad.cpu().numpy(), dP, "d_pred")
    assert_f32(gt.grad.cpu().numpy(), dG, "d_gt")
    one = pred.grad.clone()
    pred.grad = None
    (0.1 * loss).backward()                                  # Python applies grad_output: the stored gradient times it, rounded once
    assert torch.equal(pred.grad, (one.to(torch.float64) * 0.1).to(torch.float32))
    # only the side that asks: a constant prediction, host arrays with a renderer, no renderer with device tensors
    g2 = torch.from_numpy(gt_np).requires_grad_(True)        # a host leaf: its gradient comes back to the host
    pose_losses.pose_loss(pred_np, g2, joints=ref.GAN_JOINTS, root=0, renderer=renderer).backward()
    assert g2.grad.device.type == "cpu" and g2.grad.dtype == torch.float32
    assert_f32(g2.grad.numpy(), reference_loss(pred_np, gt_np, ref.GAN_JOINTS, 0, "mpjpe", 1.0, INF)[4], "d_gt on the host")
    own = pose_losses.pose_loss(pred.detach(), gt.detach(), joints=ref.GAN_JOINTS, root=0)
    assert not own.requires_grad
    assert_f64(np.array([float(own.cpu())]), np.array([reference_loss(pred_np, gt_np, ref.GAN_JOINTS, 0, "mpjpe", 1.0, INF)[0]]), "the module's own renderer")
