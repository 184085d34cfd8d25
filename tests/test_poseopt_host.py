"""The pose layer's host side (posegen_amd/poseopt.py, the two pg_poseopt_* entry points of include/posegen_hip.h) and its float64
restatement (tests/poseopt_ref.py), without a GPU: the restatement's analytic backward against autograd, the restatement against
the reference's own values (tests/golden/poseopt.npz, tools/gen_golden_poseopt.py), the ray-segment builder, the state dict, the
refusals and the ABI."""
import os
import re
import types

import numpy as np
import pytest
import torch

from posegen_amd import _ffi
from posegen_amd.poseopt import HipPoseOptLayer, axisang_to_rot6d, ray_segments
from posegen_amd.skeleton import SMPLSkeleton, rotvec_to_matrix, smpl_rest_pose
from tests import poseopt_ref as ref
from tests.helpers import load_golden

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OUTS = ("kps", "skts", "l2ws", "rots")


def random_case(U, idxs, per_pose_rest=False, seed=0):
    """parameters of U poses with 6-D values away from the normalisations' eps, and cotangents for the rays `idxs`"""
    rng = np.random.RandomState(seed)
    x = rng.normal(0, 1, (U, 24, 3, 2))
    x[..., 0] += 1.5 * np.sign(x[..., 0])                        # |a1| >= 1.5 in every component ...
    x[..., 1] = x[..., 1] + np.roll(x[..., 0], 1, axis=-1) * np.array([1.0, -1.0, 0.5])     # ... and a2 off a1's line
    rest = smpl_rest_pose[None].astype(np.float64)
    if per_pose_rest:
        rest = rest * rng.uniform(0.8, 1.2, (U, 1, 1)) + rng.normal(0, 0.02, (U, 24, 3))
    n = len(idxs)
    cot = {"kps": rng.normal(0, 1, (n, 24, 3)), "skts": rng.normal(0, 1, (n, 24, 4, 4)), "l2ws": rng.normal(0, 1, (n, 24, 4, 4)),
           "rots": rng.normal(0, 1, (n, 24, 3, 3))}
    return dict(bones=x.reshape(U, 24, 6).astype(np.float32), pelvis=rng.normal(0, 0.5, (U, 3)).astype(np.float32),
                rest=rest.astype(np.float32), idxs=np.asarray(idxs), cot={k: v.astype(np.float32) for k, v in cot.items()})


def autograd64(c, inverse):
    """torch float64 autograd of the restated forward: (d_bones, d_pelvis)"""
    t = lambda a: torch.tensor(np.asarray(a, dtype=np.float64))
    bone, pelvis = t(c["bones"]).requires_grad_(True), t(c["pelvis"]).requires_grad_(True)
    inv = torch.as_tensor(inverse, dtype=torch.long)
    outs = ref.torch_forward(bone, pelvis, t(c["rest"]))
    sum((o[inv] * t(c["cot"][k])).sum() for k, o in zip(OUTS, outs)).backward()
    return bone.grad.numpy(), pelvis.grad.numpy()


@pytest.mark.parametrize("name,U,idxs,pp", [("unsorted", 3, [2, 0, 2, 1, 0, 2, 1, 2], False), ("one_ray", 1, [0], False),
                                            ("per_pose_rest", 4, [3, 1, 0, 2, 1], True)])
def test_analytic_backward_matches_float64_autograd(name, U, idxs, pp):
    """The restatement's analytic backward (the kernel's formulas) against torch float64 autograd of the restated forward:
    within 1e-10 of each gradient's scale."""
    c = random_case(U, idxs, pp, seed=3)
    seg = ray_segments(idxs)
    db, dp = ref.backward(c["bones"], c["pelvis"], c["rest"], seg.inverse, d_kps=c["cot"]["kps"], d_skts=c["cot"]["skts"],
                          d_l2ws=c["cot"]["l2ws"], d_rots=c["cot"]["rots"])
    gb, gp = autograd64(c, seg.inverse)
    for what, got, want in (("d_bones", db, gb), ("d_pelvis", dp, gp)):
        ent, nrm = ref.deviation(got, want)
        print(f"{name} {what}: {ent:.2e} / {nrm:.2e}")
        assert ent <= 1e-10 and nrm <= 1e-10
    # the forward of the two restatements agrees as well
    for k, a, b in zip(OUTS, ref.forward(c["bones"], c["pelvis"], c["rest"]),
                       ref.torch_forward(*(torch.tensor(np.asarray(c[x], dtype=np.float64)) for x in ("bones", "pelvis", "rest")))):
        assert ref.deviation(a, b.numpy())[0] <= 1e-12, k


def golden_variant(g, sfx):
    """(unique poses' bones, pelvis, rest, segments) of one variant of poseopt.npz"""
    seg = ray_segments(g["idxs"])
    rest = g[f"rest_pose{sfx}"]
    if rest.shape[0] > 1:
        rest = rest[g["rest_pose_idxs_pp"][seg.unique]]
    return g[f"bones_param{sfx}"][seg.unique], g[f"pelvis{sfx}"][seg.unique], rest, seg


@pytest.mark.parametrize("sfx", ["", "_pp"])
def test_restatement_matches_the_reference(sfx):
    """The float64 restatement against the reference's PoseOptLayer and its autograd (poseopt.npz; fp32): the four outputs and
    both parameter gradients at the fp32 rule.  The printed figures are the reference's own fp32 deviation from float64."""
    g = load_golden("poseopt")
    bones, pelvis, rest, seg = golden_variant(g, sfx)
    outs = ref.forward(bones, pelvis, rest, seg.inverse)
    for k, o in zip(OUTS, outs):
        ref.check_rule(g[f"{k}{sfx}"], o, f"reference fp32 {k}{sfx} against the float64 restatement")
    assert np.array_equal(g[f"bones{sfx}"], bones[seg.inverse])
    db, dp = ref.backward(bones, pelvis, rest, seg.inverse, **{f"d_{k}": g[f"d_{k}"] for k in OUTS})
    full_b, full_p = np.zeros((5, 24, 6)), np.zeros((5, 3))
    full_b[seg.unique], full_p[seg.unique] = db, dp
    ref.check_rule(g[f"bones_grad{sfx}"], full_b, f"reference fp32 bones.grad{sfx} against the float64 restatement")
    ref.check_rule(g[f"pelvis_grad{sfx}"], full_p, f"reference fp32 pelvis.grad{sfx} against the float64 restatement")
    assert np.abs(full_b).max() > 0 and np.abs(full_p).max() > 0


def test_ray_segments():
    """Every ray once, ascending inside a segment, np.unique's poses; the same from a list, an array and a tensor."""
    idxs = [7, 2, 7, 0, 2, 7, 0, 7, 9]
    for given in (idxs, np.asarray(idxs), np.asarray(idxs, dtype=np.int32), torch.tensor(idxs)):
        s = ray_segments(given)
        u, inv = np.unique(idxs, return_inverse=True)
        assert np.array_equal(s.unique, u) and np.array_equal(s.inverse, inv)
        assert s.inverse.dtype == s.seg_start.dtype == s.seg_rays.dtype == np.int32
        assert s.seg_start[0] == 0 and s.seg_start[-1] == len(idxs) and (np.diff(s.seg_start) >= 0).all()
        assert sorted(s.seg_rays.tolist()) == list(range(len(idxs)))
        for p in range(len(u)):
            rays = s.seg_rays[s.seg_start[p]:s.seg_start[p + 1]]
            assert (np.diff(rays) > 0).all() and (s.inverse[rays] == p).all() and len(rays) == idxs.count(int(u[p]))
    assert ray_segments(3).unique.tolist() == [3]
    with pytest.raises(TypeError):
        ray_segments([0.5, 1.0])


def test_state_dict_round_trip():
    """The layer's state dict has the reference's names and shapes (those of the fixture's layer), loads from them bitwise, and
    the multi-view layout carries root_bones / kp_map / kp_uidxs; the initial axis-angle -> 6-D conversion is the float64
    rotation's first two columns."""
    g = load_golden("poseopt")
    for sfx in ("", "_pp"):
        sd = {"pelvis": torch.tensor(g[f"pelvis{sfx}"]), "bones": torch.tensor(g[f"bones_param{sfx}"]),
              "rest_pose": torch.tensor(g[f"rest_pose{sfx}"])}
        layer = HipPoseOptLayer.from_state_dict({"poseopt_layer_state_dict": sd})
        out = layer.state_dict()
        assert list(out) == ["pelvis", "bones", "rest_pose"]
        for k in sd:
            assert out[k].dtype == torch.float32 and torch.equal(out[k], sd[k]), k
        assert [n for n, _ in layer.named_parameters()] == ["pelvis", "bones"] and layer.N_kps == 5
    rng = np.random.RandomState(1)
    kps, aa = rng.normal(0, 1, (6, 24, 3)).astype(np.float32), rng.normal(0, 0.5, (6, 24, 3)).astype(np.float32)
    aa[0, 0] = 0.0                                               # (the zero rotation: the series branch)
    layer = HipPoseOptLayer(kps, aa, smpl_rest_pose[None], use_rot6d=True)
    want = rotvec_to_matrix(aa)[..., :3, :2].reshape(6, 24, 6)
    assert np.abs(layer.bones.detach().numpy() - want).max() <= 2 ** -23
    assert torch.equal(layer.pelvis.detach(), torch.tensor(kps[:, 0]))
    mv = HipPoseOptLayer(kps, aa, smpl_rest_pose[None], use_rot6d=True, kp_map=[0, 0, 1, 1, 2, 2], kp_uidxs=[0, 2, 4])
    shapes = {k: tuple(v.shape) for k, v in mv.state_dict().items()}
    assert shapes == {"kp_map": (6,), "kp_uidxs": (3,), "rest_pose": (1, 24, 3), "pelvis": (6, 3), "root_bones": (6, 6),
                      "bones": (3, 23, 6)}
    pelvis, bone = mv.idx_to_params([5, 2])
    assert tuple(bone.shape) == (2, 24, 6) and torch.equal(bone[0, 1:], mv.bones[2]) and torch.equal(bone[1, 0], mv.root_bones[2])
    again = HipPoseOptLayer.from_state_dict(mv.state_dict())
    assert all(torch.equal(v, again.state_dict()[k]) for k, v in mv.state_dict().items())
    with pytest.raises(_ffi.HipLibraryError):
        layer([0, 1])                                            # no renderer: an error, not a torch fallback


def test_refusals():
    """use_rot6d=False, use_cache=True, another skeleton, a renderer off the HIP device: NotImplementedError, nothing computed."""
    z = np.zeros((2, 24, 3), dtype=np.float32)
    with pytest.raises(NotImplementedError, match="use_rot6d"):
        HipPoseOptLayer(z, z, z[:1])
    with pytest.raises(NotImplementedError, match="use_cache"):
        HipPoseOptLayer(z, z, z[:1], use_rot6d=True, use_cache=True)
    other = types.SimpleNamespace(joint_trees=np.arange(24) - 1, root_id=0)
    with pytest.raises(NotImplementedError, match="SMPL"):
        HipPoseOptLayer(z, z, z[:1], skel_type=other, use_rot6d=True)
    cpu = types.SimpleNamespace(device=torch.device("cpu"))
    with pytest.raises(NotImplementedError, match="HIP device"):
        HipPoseOptLayer(z, z, z[:1], use_rot6d=True, renderer=cpu)
    with pytest.raises(NotImplementedError, match="axis-angle"):
        HipPoseOptLayer.from_state_dict({"pelvis": torch.zeros(2, 3), "bones": torch.zeros(2, 24, 3), "rest_pose": torch.zeros(1, 24, 3)})
    assert HipPoseOptLayer(z, z, z[:1], skel_type=SMPLSkeleton, use_rot6d=True).N_kps == 2


def test_abi_declares_and_exports_the_pose_layer():
    """include/posegen_hip.h declares pg_poseopt_forward / pg_poseopt_backward, the built library exports them with ctypes
    prototypes, and the ABI version is still 11."""
    hdr = open(os.path.join(REPO, "include", "posegen_hip.h")).read()
    lib = _ffi.load_library()
    for name in ("pg_poseopt_forward", "pg_poseopt_backward"):
        assert re.search(rf"\bint {name}\s*\(", hdr), f"{name} is not declared in the header"
        assert hasattr(lib, name) and name in _ffi.PROTOTYPES
    assert re.search(r"#define PG_ABI_VERSION 11\b", hdr)
    assert lib.pg_abi_version() == 11 == _ffi.PG_ABI_VERSION
    import posegen_amd
    assert posegen_amd.HipPoseOptLayer is HipPoseOptLayer
