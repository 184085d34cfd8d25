"""Float64 restatement of the pose layer (posegen_amd/poseopt.py, csrc/pg_poseopt.hip) for the tests: the role tests/mesh_ref.py
plays for the mesh.  NumPy: `forward` (the reference's PoseOptLayer.calculate_kinematic, core/pose_opt.py:372-445, with
rot6d_to_rotmat, core/utils/skeleton_utils.py:507-523) and `backward`, the ANALYTIC transpose the kernel implements -- not
autograd.  Torch: `torch_forward`, the same forward as a differentiable graph in any dtype on any device (what autograd checks
`backward` against, and the torch layer the device layer is compared and timed against), and `TorchPoseOptLayer` around it.
"""
import numpy as np
import torch
import torch.nn.functional as F

from posegen_amd.skeleton import SMPLSkeleton

PARENTS = np.asarray(SMPLSkeleton.joint_trees, dtype=np.int64)
EPS = 1e-12


def _normalize(v):
    n = np.linalg.norm(v, axis=-1, keepdims=True)
    return v / np.maximum(n, EPS), n


def _normalize_bwd(b, n, g):
    """transpose of v / max(|v|, eps): below eps the derivative is 1 / eps"""
    return np.where(n > EPS, (g - b * (b * g).sum(-1, keepdims=True)) / np.where(n > EPS, n, 1.0), g / EPS)


def _unique_forward(bones, pelvis, rest, parents=PARENTS):
    """per unique pose: everything `backward` needs.  bones [U,24,6], pelvis [U,3], rest [1 or U,24,3]"""
    bones, pelvis, rest = (np.asarray(a, dtype=np.float64) for a in (bones, pelvis, rest))
    U = bones.shape[0]
    x = bones.reshape(U, 24, 3, 2)
    a1, a2 = x[..., 0], x[..., 1]
    b1, n1 = _normalize(a1)
    s = (b1 * a2).sum(-1, keepdims=True)
    b2, n2 = _normalize(a2 - s * b1)
    b3 = np.cross(b1, b2)
    R = np.stack([b1, b2, b3], axis=-1)                                   # columns
    rest = np.broadcast_to(rest, (U, 24, 3))
    rel = np.zeros((U, 24, 4, 4))
    rel[..., :3, :3] = R
    rel[..., 3, 3] = 1.0
    rel[:, 0, :3, 3] = rest[:, 0]
    rel[:, 1:, :3, 3] = rest[:, 1:] - rest[:, parents[1:]]
    chain = np.zeros_like(rel)
    chain[:, 0] = rel[:, 0]
    for j in range(1, 24):
        chain[:, j] = chain[:, parents[j]] @ rel[:, j]
    l2w = chain.copy()
    l2w[..., :3, 3] += pelvis[:, None]
    skt = np.linalg.inv(l2w)
    return dict(a2=a2, b1=b1, b2=b2, b3=b3, n1=n1, n2=n2, s=s, R=R, rel=rel, chain=chain, l2w=l2w, skt=skt)


def forward(bones, pelvis, rest, inverse=None, parents=PARENTS):
    """(kps [n,24,3], skts [n,24,4,4], l2ws [n,24,4,4], rots [n,24,3,3]) in float64; inverse [n]: ray -> pose (None: identity)"""
    f = _unique_forward(bones, pelvis, rest, parents)
    inv = np.arange(f["R"].shape[0]) if inverse is None else np.asarray(inverse)
    return f["l2w"][inv][..., :3, 3], f["skt"][inv], f["l2w"][inv], f["R"][inv]


def backward(bones, pelvis, rest, inverse=None, d_kps=None, d_skts=None, d_l2ws=None, d_rots=None, parents=PARENTS):
    """(d_bones [U,24,6], d_pelvis [U,3]) from the per-ray cotangents (None: zero), by the formulas of the kernel."""
    f = _unique_forward(bones, pelvis, rest, parents)
    U = f["R"].shape[0]
    inv = np.arange(U) if inverse is None else np.asarray(inverse)

    def seg(c, shape):
        out = np.zeros((U,) + shape)
        if c is not None:
            np.add.at(out, inv, np.asarray(c, dtype=np.float64))
        return out
    dS, dL, dRr, dK = seg(d_skts, (24, 4, 4)), seg(d_l2ws, (24, 4, 4)), seg(d_rots, (24, 3, 3)), seg(d_kps, (24, 3))
    St = np.swapaxes(f["skt"], -1, -2)
    G = -St @ dS @ St + dL                                                # torch.inverse's backward, full 4 x 4
    G[..., :3, 3] += dK
    d_pelvis = G[..., :3, 3].sum(1)
    G[..., 3, :] = 0.0                                                    # row 3 of l2w is a constant
    dRel = np.zeros((U, 24, 4, 4))
    for j in range(23, 0, -1):                                            # children before parents
        p = parents[j]
        dRel[:, j] = np.swapaxes(f["chain"][:, p], -1, -2) @ G[:, j]
        G[:, p] += G[:, j] @ np.swapaxes(f["rel"][:, j], -1, -2)
        G[:, p, 3, :] = 0.0
    dRel[:, 0] = G[:, 0]
    dR = dRel[..., :3, :3] + dRr
    g1, g2, g3 = dR[..., 0].copy(), dR[..., 1].copy(), dR[..., 2]
    g1 += np.cross(f["b2"], g3)
    g2 += np.cross(g3, f["b1"])
    du2 = _normalize_bwd(f["b2"], f["n2"], g2)
    ds = -(du2 * f["b1"]).sum(-1, keepdims=True)
    da2 = du2 + ds * f["b1"]
    g1 += -f["s"] * du2 + ds * f["a2"]
    da1 = _normalize_bwd(f["b1"], f["n1"], g1)
    return np.stack([da1, da2], axis=-1).reshape(U, 24, 6), d_pelvis


def torch_forward(bone, pelvis, rest, parents=PARENTS):
    """The forward of the unique poses as a torch graph in the inputs' dtype / device, with the reference's operations (F.normalize,
    torch.cross, matmul down the tree, torch.inverse): (kps, skts, l2ws, rots), each [U,...]."""
    U = bone.shape[0]
    x = bone.reshape(-1, 3, 2)
    a1, a2 = x[:, :, 0], x[:, :, 1]
    b1 = F.normalize(a1)
    b2 = F.normalize(a2 - torch.einsum("bi,bi->b", b1, a2).unsqueeze(-1) * b1)
    b3 = torch.cross(b1, b2, dim=-1)
    rots = torch.stack((b1, b2, b3), dim=-1).reshape(U, 24, 3, 3)
    rest = rest.expand(U, 24, 3)
    par = torch.as_tensor(np.asarray(parents), device=bone.device)
    offs = torch.cat([rest[:, :1], rest[:, 1:] - rest[:, par[1:]]], dim=1)
    bottom = torch.zeros(U, 24, 1, 4, dtype=bone.dtype, device=bone.device)
    bottom[..., 3] = 1
    rel = torch.cat([torch.cat([rots, offs[..., None]], dim=-1), bottom], dim=-2)
    l2w = [rel[:, 0]]
    for j in range(1, 24):
        l2w.append(l2w[int(parents[j])] @ rel[:, j])
    l2ws = torch.stack(l2w, dim=1)
    shift = torch.zeros(U, 1, 4, 4, dtype=bone.dtype, device=bone.device)
    shift[:, 0, :3, 3] = pelvis
    l2ws = l2ws + shift
    return l2ws[..., :3, 3], torch.inverse(l2ws), l2ws, rots


class TorchPoseOptLayer(torch.nn.Module):
    """The reference layer restated in torch (single view, use_rot6d): the same parameters as HipPoseOptLayer, forward(idxs) ->
    (kps, bones, skts, l2ws, rots) per ray through `np.unique` and a gather, whose backward is autograd's."""

    def __init__(self, pelvis, bones, rest_pose, rest_pose_idxs=None, device="cpu", dtype=torch.float32):
        super().__init__()
        t = lambda a: torch.as_tensor(np.asarray(a), dtype=dtype).to(device)
        self.pelvis = torch.nn.Parameter(t(pelvis))
        self.bones = torch.nn.Parameter(t(bones))
        self.register_buffer("rest_pose", t(rest_pose))
        self.rest_pose_idxs = rest_pose_idxs

    def forward(self, idxs, rest_pose_idxs=None):
        unique, inverse = np.unique(np.asarray(idxs), return_inverse=True)
        dev = self.pelvis.device
        u, inv = torch.as_tensor(unique, device=dev), torch.as_tensor(inverse.reshape(-1), device=dev)
        rest = self.rest_pose
        if len(rest) > 1:
            ridx = np.asarray(self.rest_pose_idxs)[unique] if rest_pose_idxs is None else np.asarray(rest_pose_idxs)
            rest = rest[torch.as_tensor(ridx, device=dev)]
        bone = self.bones[u]
        kps, skts, l2ws, rots = torch_forward(bone, self.pelvis[u], rest)
        return kps[inv], bone[inv], skts[inv], l2ws[inv], rots[inv]


# ---- the comparison rule of the pose-gradient tests (tests/test_gpu_pose_grad.py, test_gpu_train_shapes.py) ---------------------
def scale_of(a):
    a = np.asarray(a, dtype=np.float64).reshape(-1)
    return max(float(np.abs(a).max()), float(np.linalg.norm(a)) / np.sqrt(a.size), 1e-30)


def deviation(got, ref):
    """(largest entry deviation / the tensor's scale, norm deviation / norm)"""
    got, ref = np.asarray(got, dtype=np.float64), np.asarray(ref, dtype=np.float64)
    rn = float(np.linalg.norm(ref))
    return float(np.abs(got - ref).max()) / scale_of(ref), abs(float(np.linalg.norm(got)) - rn) / max(rn, 1e-30)


def check_rule(got, ref, what, own32=None, entry=1e-4, norm=1e-4):
    """fp32 rule: every entry within 1e-4 of the tensor's scale, the norm within 1e-4.  A case outside gets max(bound, 4 x the
    fp32 reference's own deviation from `ref`) -- own32() returns that fp32 reference's values -- printed, never a looser constant."""
    got, ref = np.asarray(got), np.asarray(ref)
    assert got.shape == ref.shape, (what, got.shape, ref.shape)
    assert np.isfinite(got).all(), what
    ent, nrm = deviation(got, ref)
    te, tn = entry, norm
    if (ent > te or nrm > tn) and own32 is not None:
        e32, n32 = deviation(own32(), ref)
        te, tn = max(te, 4.0 * e32), max(tn, 4.0 * n32)
        print(f"{what}: deviates {ent:.2e} / {nrm:.2e}; the fp32 reference's own deviation {e32:.2e} / {n32:.2e}: bounds {te:.2e} / {tn:.2e}")
    print(f"{what}: entries within {ent:.2e} of the scale, norm within {nrm:.2e}")
    assert ent <= te and nrm <= tn, (what, ent, nrm, te, tn)
    return ent, nrm
