"""float64 numpy restatement of pg_smpl_forward, pg_vertex_errors and pg_pose_kinematics_rot (include/posegen_hip.h)
and of the two evaluation functions in front of the pose scores.  The formulas are the reference's -- `lbs`, `vertices2joints`,
`blend_shapes`, `batch_rodrigues`, `batch_rigid_transform` (smplx/smplx/lbs.py:152-401), `evaluate.test` (run_gan.py:1584-1634),
`evaluate_pampjpe_from_smpl_params` (core/utils/evaluation_helpers.py:542-603), `get_smpl_l2ws_torch(axis_to_matrix=False)`
(core/utils/skeleton_utils.py:379-463) -- in double on the float32 inputs.

Beside every output comes `mag`: the sum of the absolute values of the products accumulated into it, carried through the stages
(blend rows; then sum_j |w_j| |A_j| applied to [mag of v_posed; 1]; then |regress| times the vertices' mag).  A float32 evaluation
of a sum of n products, in any order, is within n u mag of the exact value to first order (u = 2^-24): `bound`."""
import numpy as np

from tests import pose_scores_ref as psr

U = 2.0 ** -24
H36M_TO_J14 = [6, 5, 4, 1, 2, 3, 16, 15, 14, 11, 12, 13, 8, 10]
SPIN_TO_CANON = [10, 8, 14, 15, 16, 11, 12, 13, 4, 5, 6, 1, 2, 3, 0, 7, 9]


def f64(x):
    return np.asarray(x, dtype=np.float64)


def rodrigues(r):
    """batch_rodrigues (lbs.py:295-329) as written: [N,3] -> [N,3,3]"""
    r = f64(r)
    angle = np.sqrt(((r + 1e-8) ** 2).sum(1, keepdims=True))
    d = r / angle
    K = np.zeros((len(r), 3, 3))
    K[:, 0, 1], K[:, 0, 2], K[:, 1, 0], K[:, 1, 2], K[:, 2, 0], K[:, 2, 1] = -d[:, 2], d[:, 1], d[:, 2], -d[:, 0], -d[:, 1], d[:, 0]
    return np.eye(3) + np.sin(angle)[:, :, None] * K + (1 - np.cos(angle))[:, :, None] * (K @ K)


def axisang_to_rot(bones):
    """axisang_to_rot (skeleton_utils.py:498: axis-angle -> quaternion -> matrix) in float64, rounded to float32: [..., 3] -> [..., 3, 3]"""
    b = f64(bones)
    ang = np.sqrt((b * b).sum(-1, keepdims=True))
    small = np.abs(ang) < 1e-6
    k = np.where(small, 0.5 - ang * ang / 48.0, np.sin(0.5 * ang) / np.where(small, 1.0, ang))
    q = np.concatenate([np.cos(0.5 * ang), b * k], -1)
    r, i, j, k_ = (q[..., n] for n in range(4))
    s = 2.0 / (q * q).sum(-1)
    m = np.stack([1 - s * (j * j + k_ * k_), s * (i * j - k_ * r), s * (i * k_ + j * r), s * (i * j + k_ * r), 1 - s * (i * i + k_ * k_),
                  s * (j * k_ - i * r), s * (i * k_ - j * r), s * (j * k_ + i * r), 1 - s * (i * i + j * j)], -1)
    return m.reshape(*b.shape[:-1], 3, 3).astype(np.float32)


def rigid_transform(R, J, parents):
    """batch_rigid_transform (lbs.py:345-401): (posed joints [B,24,3], A [B,24,4,4], mag of the posed joints)"""
    B, n = R.shape[:2]
    rel = J.copy()
    rel[:, 1:] -= J[:, parents[1:]]
    M = np.zeros((B, n, 4, 4))
    M[:, :, :3, :3], M[:, :, :3, 3], M[:, :, 3, 3] = R, rel, 1.0
    G, mag = [M[:, 0]], [np.abs(rel[:, 0])]
    for i in range(1, n):
        p = int(parents[i])
        G.append(G[p] @ M[:, i])
        mag.append(mag[p] + np.einsum("brc,bc->br", np.abs(G[p][:, :3, :3]), np.abs(rel[:, i])))
    G = np.stack(G, 1)
    A = G.copy()
    A[:, :, :3, 3] -= np.einsum("bjrc,bjc->bjr", G[:, :, :3, :3], J)
    return G[:, :, :3, 3].copy(), A, np.stack(mag, 1)


def lbs(model, betas, pose, pose2rot=True, regress=None):
    """dict: verts [B,V,3], joints [B,24,3], regressed [B,K,3] (with `regress` [K,V]), v_shaped, v_posed, and mag_verts, mag_joints,
    mag_regressed.  `model`: smplx-layout arrays (synthetic.make_body_model); betas [B,NB] or [1,NB]."""
    vt, sd, pd = f64(model["v_template"]), f64(model["shapedirs"]), f64(model["posedirs"])
    jr, W = f64(model["J_regressor"]), f64(model["lbs_weights"])
    parents = np.asarray(model["parents"]).astype(np.int64)
    pose, betas = f64(pose), f64(betas)
    B = pose.shape[0]
    betas = np.broadcast_to(betas, (B, betas.shape[1]))
    V = vt.shape[0]
    v_shaped = vt[None] + np.einsum("bl,mkl->bmk", betas, sd)
    J = np.einsum("jv,bvc->bjc", jr, v_shaped)
    R = rodrigues(pose.reshape(-1, 3)).reshape(B, 24, 3, 3) if pose2rot else pose.reshape(B, 24, 3, 3)
    feat = (R[:, 1:] - np.eye(3)).reshape(B, 207)
    v_posed = v_shaped + (feat @ pd).reshape(B, V, 3)
    mag_vp = np.abs(vt)[None] + np.einsum("bl,mkl->bmk", np.abs(betas), np.abs(sd)) + (np.abs(feat) @ np.abs(pd)).reshape(B, V, 3)
    joints, A, mag_joints = rigid_transform(R, J, parents)
    T = np.einsum("vj,bjrc->bvrc", W, A[:, :, :3, :])
    mag_T = np.einsum("vj,bjrc->bvrc", np.abs(W), np.abs(A[:, :, :3, :]))
    verts = np.einsum("bvrc,bvc->bvr", T[..., :3], v_posed) + T[..., 3]
    mag_verts = np.einsum("bvrc,bvc->bvr", mag_T[..., :3], mag_vp) + mag_T[..., 3]
    out = dict(verts=verts, joints=joints, v_shaped=v_shaped, v_posed=v_posed, mag_verts=mag_verts, mag_joints=mag_joints, rot=R)
    if regress is not None:
        out["regressed"] = np.einsum("kv,bvc->bkc", f64(regress), verts)
        out["mag_regressed"] = np.einsum("kv,bvc->bkc", np.abs(f64(regress)), mag_verts)
    return out


def n_vertex_products(NB):
    """the products and roundings behind one vertex coordinate: blend rows, 24 skin weights, the 4 of T [v; 1], 8 for the
    once-rounded features and transforms"""
    return (1 + NB + 207) + 24 + 4 + 8


def bound_verts(ref_out, NB):
    return n_vertex_products(NB) * U * ref_out["mag_verts"]


def bound_regressed(ref_out, NB, V):
    """the regression adds 4 vertices in float32 (one MFMA) and everything above that in double: the tiles are ceil(V / 4)"""
    return (n_vertex_products(NB) + (V + 3) // 4) * U * ref_out["mag_regressed"]


def bound_chain(value64, mag, links=9):
    """posed joints and key points: one float32 ulp of the restatement's rounded value plus `links` u mag for the float32 inputs' own
    rounding through a chain of that many joints (root to leaf: the SMPL tree's longest has 9, its depth + 1)"""
    return np.spacing(np.abs(f64(value64).astype(np.float32))).astype(np.float64) + links * U * mag


def rot_chain(rotmats, rest_pose, scale=1.0, parents=None):
    """get_smpl_l2ws_torch(axis_to_matrix=False): (l2ws float64 [F,24,4,4], key points [F,24,3], their mag).  rest_pose * scale in
    rest_pose's own dtype, as the reference forms it."""
    from posegen_amd.skeleton import SMPLSkeleton
    par = np.asarray(SMPLSkeleton.joint_trees if parents is None else parents).astype(np.int64)
    rp = np.asarray(rest_pose).reshape(24, 3)
    rp = rp * np.asarray(scale, dtype=rp.dtype)
    offs = rp.copy()
    offs[1:] = rp[1:] - rp[par[1:]]
    offs = f64(offs)
    R = f64(rotmats)
    F = R.shape[0]
    M = np.zeros((F, 24, 4, 4))
    M[:, :, :3, :3], M[:, :, :3, 3], M[:, :, 3, 3] = R, offs[None], 1.0
    G, mag = [M[:, 0]], [np.broadcast_to(np.abs(offs[0]), (F, 3)).copy()]
    for i in range(1, 24):
        p = int(par[i])
        G.append(G[p] @ M[:, i])
        mag.append(mag[p] + np.abs(G[p][:, :3, :3]) @ np.abs(offs[i]))
    G = np.stack(G, 1)
    return G, G[:, :, :3, 3].copy(), np.stack(mag, 1)


def vertex_errors(a, b):
    """(per pose mean_v |a_v - b_v|, their mean): run_gan.py:1630-1631"""
    with np.errstate(invalid="ignore"):
        pp = np.sqrt(((f64(a) - f64(b)) ** 2).sum(-1)).mean(-1)
    return pp, pp.mean()


def pelvis_j14(regressed):
    r = f64(regressed)
    return r[:, H36M_TO_J14] - r[:, :1]


def evaluate_test(neutral, male, female, regress_key, pred_rotmat, pred_betas, gt_pose, gt_betas, gender, alpha=0.15, given=None):
    """evaluate.test behind the regressor (run_gan.py:1596-1634): dict of [B] arrays mpjpe, pa-mpjpe, pck, ume, pme.  `given`:
    float32 (pred_kps, gt_kps, un_gt, un_pred, gt_verts, pred_verts) to score instead of the restatement's own (what a device
    produced: the scores are then a function of exactly those values)."""
    B = len(pred_rotmat)
    fem = (np.asarray(gender).reshape(-1) == 1)[:, None, None]
    if given is None:
        pred = lbs(neutral, pred_betas, pred_rotmat, pose2rot=False, regress=neutral[regress_key])
        gm = lbs(male, gt_betas, np.reshape(gt_pose, (B, 24, 3)), regress=male[regress_key])
        gf = lbs(female, gt_betas, np.reshape(gt_pose, (B, 24, 3)), regress=female[regress_key])
        eye = np.broadcast_to(np.eye(3), (B, 24, 3, 3))
        un_pred = lbs(neutral, pred_betas, eye, pose2rot=False)["verts"]
        un_gt = np.where(fem, lbs(female, gt_betas, eye, pose2rot=False)["verts"], lbs(male, gt_betas, eye, pose2rot=False)["verts"])
        gt_verts, pred_verts = np.where(fem, gf["verts"], gm["verts"]), pred["verts"]
        pred_kps, gt_kps = pelvis_j14(pred["regressed"]), pelvis_j14(np.where(fem, gf["regressed"], gm["regressed"]))
    else:
        pred_kps, gt_kps, un_gt, un_pred, gt_verts, pred_verts = given
    pp = psr.per_pose(pred_kps, gt_kps, align=psr.ALIGN_ROTATION)
    dist32 = pp["dist_raw"].astype(np.float32)                          # the share is taken of the float32 distances
    return {"mpjpe": pp["raw"], "pa-mpjpe": pp["aligned"], "pck": (dist32 < np.float32(alpha)).mean(1),
            "ume": vertex_errors(un_gt, un_pred)[0], "pme": vertex_errors(gt_verts, pred_verts)[0],
            "_kps": (pred_kps, gt_kps), "_verts": (un_gt, un_pred, gt_verts, pred_verts)}


def pampjpe_from_smpl_params(model, regress_key, gt_kps, betas, bones, pck_threshold=150.0, use_normalize=False, pred_kps=None):
    """evaluate_pampjpe_from_smpl_params(ret_kp=True, ret_pck=True) (evaluation_helpers.py:542-603) with the shares taken over
    the joints' aligned distances: dict pampjpe, mpjpe, pck, auc, pred_kps.  `pred_kps`: float32 key points to score instead."""
    B = len(bones)
    if pred_kps is None:
        rots = axisang_to_rot(np.reshape(bones, (B, 24, 3)))
        pred_kps = lbs(model, betas, rots, pose2rot=False, regress=model[regress_key])["regressed"][:, SPIN_TO_CANON]
    gt = f64(np.asarray(gt_kps, dtype=np.float32))
    th = np.concatenate([[pck_threshold], np.linspace(0, 150, 31)])
    pa = psr.per_pose(pred_kps, gt, align=psr.ALIGN_BEST)
    s = psr.summary(pa, th)
    gt_m = f64((gt / 1000.0).astype(np.float32))                     # metres, rounded to float32 once
    mp = psr.per_pose(pred_kps, gt_m, root=14, align=psr.ALIGN_SCALE if use_normalize else psr.ALIGN_NONE)
    T = len(th)
    return {"pampjpe": s[2], "mpjpe": (mp["aligned"] if use_normalize else mp["raw"]).mean() * 1000.0, "pck": s[4 + T],
            "auc": s[4 + T + 1:4 + 2 * T].mean(), "pred_kps": pred_kps}
