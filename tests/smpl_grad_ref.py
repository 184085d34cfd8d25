"""float64 numpy restatement of pg_smpl_backward (include/posegen_hip.h): the transpose of `smpl_ref.lbs` followed
by `vertices2joints`, written out by hand -- no autograd -- for the cotangents of the vertices, the posed joints and the regressed
joints, into `d_betas` [B,NB] (one row per pose) and `d_pose` ([B,24,3] through `batch_rodrigues` exactly as written, angle =
|r + 1e-8|, or [B,24,3,3] with the nine entries of every matrix free).

Beside every gradient entry comes its `mag`: the same backward with every factor replaced by its absolute value and every difference
by a sum; the two forward quantities the device forms again in float32, v_posed and T = sum_j skin A_j, enter with their own sums of
absolute products (`mag_vp`, `mag_T` of the forward restatement), the rest joints as |rest_0| + sum_l |beta_l| |rest_l| and the
chain's offsets J_j - J_parent as the sum of those two.  `bound = n u mag`, u = 2^-24, n = `n_grad_products(NB, K)`.

The derivation of n (the device's accumulation scheme, csrc/pg_smpl.hip).  Everything outside the vertex-tile kernel is float64 and
contributes nothing at this scale; a gradient entry is a float64 sum of contributions that reach it through dA (skinning) or through
d feat (blend), so its error is at most the larger of the two paths' counts times u times the sum of the contributions' mags.
  dv      = d_verts + regress^T d_regressed: K float32 products added inside the MFMAs, one addition                    K + 1
  v_posed : the forward's blend GEMM again, rows = 1 + NB + 207 products, the once-rounded feature row                  rows + 2
  T       : 24 skin products, the once-rounded A                                                                        24 + 1
  dA path : a tile adds 64 vertices of skin (dv vp1) in float32 (two roundings per term), tiles are added in float64:
            64 + 2 + (K + 1) + (rows + 2)                                                                              = rows + K + 69
  d feat  : a tile adds 192 columns of blend dvp in float32, dvp = T_R^T dv is 3 products on T and dv:
            192 + 1 + 3 + (24 + 1) + (K + 1)                                                                           = K + 222
  the result is rounded to float32 once                                                                                 + 1
n = max(rows + K + 69, K + 222) + 1 = rows + K + 70 with rows = 1 + NB + 207 (rows >= 209 > 153).  It does not depend on V: above one
tile every sum is float64."""
import numpy as np

from tests import smpl_ref as ref

U = ref.U
f64 = ref.f64
TERMS = ("dJ_from_dAt", "pose_feature", "rest_joints", "regressor", "dAt_outer_J")


def n_grad_products(NB, K):
    """see the module docstring: rows + K + 70"""
    return (1 + NB + 207) + K + 70


def _rodrigues_parts(r):
    """batch_rodrigues' intermediates for [N,3] vectors"""
    e = r + 1e-8
    th = np.sqrt((e * e).sum(1))
    d = r / th[:, None]
    K = np.zeros((len(r), 3, 3))
    K[:, 0, 1], K[:, 0, 2], K[:, 1, 0], K[:, 1, 2], K[:, 2, 0], K[:, 2, 1] = -d[:, 2], d[:, 1], d[:, 2], -d[:, 0], -d[:, 1], d[:, 0]
    return dict(r=r, e=e, th=th, K=K, sn=np.sin(th), cs=np.cos(th), oc=1.0 - np.cos(th))


def _rodrigues_bwd(p, D, sub):
    """the cotangent D [N,3,3] of R = I + sin K + (1 - cos) K K through K = skew(r / angle), angle = |r + 1e-8| -> [N,3]"""
    K, th = p["K"], p["th"]
    Kt = np.swapaxes(K, 1, 2)
    dK = p["sn"][:, None, None] * D + p["oc"][:, None, None] * (D @ Kt + Kt @ D)
    dth = p["cs"] * (D * K).sum((1, 2)) + p["sn"] * (D * (K @ K)).sum((1, 2))
    if sub > 0:                                          # mag: the differences below are sums
        dd = np.stack([dK[:, 2, 1] + dK[:, 1, 2], dK[:, 0, 2] + dK[:, 2, 0], dK[:, 1, 0] + dK[:, 0, 1]], 1)
    else:
        dd = np.stack([dK[:, 2, 1] - dK[:, 1, 2], dK[:, 0, 2] - dK[:, 2, 0], dK[:, 1, 0] - dK[:, 0, 1]], 1)
    dth = dth + sub * (dd * p["r"]).sum(1) / (th * th)
    return dd / th[:, None] + dth[:, None] * p["e"] / th[:, None]


def _transpose(q, sub, pose2rot, drop):
    """the backward on the quantities `q`; sub = -1 for the values, +1 (with every entry of q an absolute value) for mag"""
    W, parents = q["W"], q["parents"]
    B = q["vp"].shape[0]
    dv = q["d_verts"].copy()
    if q["regress"] is not None and "regressor" not in drop:
        dv = dv + np.einsum("kv,bkc->bvc", q["regress"], q["d_regressed"])
    dvp = np.einsum("bvrc,bvr->bvc", q["T"][..., :3], dv)
    vp1 = np.concatenate([q["vp"], np.ones_like(q["vp"][..., :1])], -1)
    dA = np.einsum("vj,bvr,bvc->bjrc", W, dv, vp1)
    dfeat_pose = dvp.reshape(B, -1) @ q["pd"].T                                      # [B,207]
    dfeat_beta = np.einsum("vcl,bvc->bl", q["sd"], dvp)
    dAt = dA[..., 3]
    dG = dA.copy()
    if "dAt_outer_J" not in drop:
        dG[..., :3] += sub * dAt[..., None] * q["J"][:, :, None, :]
    dG[..., 3] += q["d_joints"]
    dJ = np.zeros_like(q["J"])
    if "dJ_from_dAt" not in drop:
        dJ += sub * np.einsum("bjrc,bjr->bjc", q["G_R"], dAt)
    M = q["M"]                                                                       # [B,24,3,4] = [R_j | J_j - J_parent]
    for i in range(23, 0, -1):                                                       # children before parents
        p = int(parents[i])
        dG[:, p, :, :3] += np.einsum("brc,bkc->brk", dG[:, i], M[:, i])
        dG[:, p, :, 3] += dG[:, i, :, 3]
    dM = dG.copy()
    for i in range(1, 24):
        dM[:, i] = np.einsum("bkr,bkc->brc", q["G_R"][:, int(parents[i])], dG[:, i])
    dR, drel = dM[..., :3].copy(), dM[..., 3]
    dJ += drel
    for i in range(1, 24):
        dJ[:, int(parents[i])] += sub * drel[:, i]
    d_betas = dfeat_beta.copy()
    if "rest_joints" not in drop:
        d_betas += np.einsum("ljc,bjc->bl", q["rest"], dJ)
    if "pose_feature" not in drop:
        dR[:, 1:] += dfeat_pose.reshape(B, 23, 3, 3)
    if not pose2rot:
        return d_betas, dR
    return d_betas, _rodrigues_bwd(q["rod"], dR.reshape(-1, 3, 3), sub).reshape(B, 24, 3)


def lbs_backward(model, betas, pose, pose2rot=True, regress=None, d_verts=None, d_joints=None, d_regressed=None, drop=()):
    """dict d_betas [B,NB], d_pose, mag_betas, mag_pose for the given cotangents (None = zero).  `drop`: names of TERMS to leave out
    (the ablations of tests/test_smpl_grad_ref.py).  A shared betas row ([1,NB]) still gets one row per pose: `shared_betas_row`."""
    pose = f64(pose)
    B = pose.shape[0]
    fw = ref.lbs(model, betas, pose, pose2rot=pose2rot, regress=regress)
    vt, sd, pd = f64(model["v_template"]), f64(model["shapedirs"]), f64(model["posedirs"])
    jr, W = f64(model["J_regressor"]), f64(model["lbs_weights"])
    parents = np.asarray(model["parents"]).astype(np.int64)
    V = vt.shape[0]
    R = fw["rot"]
    J = np.einsum("jv,bvc->bjc", jr, fw["v_shaped"])
    rel = J.copy()
    rel[:, 1:] -= J[:, parents[1:]]
    _, A, _ = ref.rigid_transform(R, J, parents)
    A = A[:, :, :3, :]
    M = np.concatenate([R, rel[..., None]], -1)
    rest = np.einsum("jv,vcl->ljc", jr, sd)
    zero = lambda *s: np.zeros(s)
    K = 0 if regress is None else np.shape(regress)[0]
    cot = dict(d_verts=zero(B, V, 3) if d_verts is None else f64(d_verts), d_joints=zero(B, 24, 3) if d_joints is None else f64(d_joints),
               d_regressed=zero(B, K, 3) if d_regressed is None else f64(d_regressed))
    q = dict(W=W, parents=parents, regress=None if regress is None else f64(regress), T=np.einsum("vj,bjrc->bvrc", W, A), vp=fw["v_posed"],
             pd=pd, sd=sd, J=J, G_R=A[..., :3], M=M, rest=rest, **cot)
    absq = {k: (v if k == "parents" or v is None else np.abs(v)) for k, v in q.items()}
    absq["T"] = np.einsum("vj,bjrc->bvrc", np.abs(W), np.abs(A))
    betas_b = np.broadcast_to(f64(betas), (B, sd.shape[2]))
    absq["vp"] = np.abs(vt)[None] + np.einsum("bl,mkl->bmk", np.abs(betas_b), np.abs(sd)) \
        + (np.abs((R[:, 1:] - np.eye(3)).reshape(B, 207)) @ np.abs(pd)).reshape(B, V, 3)
    # the rest joints are sums of products (rest_0 + sum_l beta_l rest_l) and the chain's offsets differences of two of them
    rest0 = np.einsum("jv,vc->jc", jr, vt)
    absq["J"] = np.abs(rest0)[None] + np.einsum("bl,ljc->bjc", np.abs(betas_b), np.abs(rest))
    mag_rel = absq["J"].copy()
    mag_rel[:, 1:] += absq["J"][:, parents[1:]]
    absq["M"] = np.concatenate([np.abs(R), mag_rel[..., None]], -1)
    if pose2rot:
        q["rod"] = _rodrigues_parts(pose.reshape(-1, 3))
        absq["rod"] = {k: np.abs(v) for k, v in q["rod"].items()}
    d_betas, d_pose = _transpose(q, -1.0, pose2rot, drop)
    mag_betas, mag_pose = _transpose(absq, 1.0, pose2rot, ())
    return dict(d_betas=d_betas, d_pose=d_pose, mag_betas=mag_betas, mag_pose=mag_pose)


def shared_betas_row(d_betas):
    """one betas row for all poses: the poses' rows added in float64 in pose order"""
    s = np.zeros(d_betas.shape[1])
    for row in f64(d_betas):
        s = s + row
    return s[None]


def bounds(g, NB, K):
    n = n_grad_products(NB, K)
    return n * U * g["mag_betas"], n * U * g["mag_pose"]
