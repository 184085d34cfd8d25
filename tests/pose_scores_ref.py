"""float64 numpy restatement of pg_pose_scores (include/posegen_hip.h): the four alignment modes per pose and the
summary over a batch.  The formulas are the reference's -- `procrustes(scaling=True, reflection='best')`
(core/utils/evaluation_helpers.py:387-467), `compute_similarity_transform` (run_gan.py:1380-1428),
`Criterion3DPose_leastQuaresScaled` (evaluation_helpers.py:506-522), `Criterion_MPJPE` (:469-483) -- in double on the float32
inputs, with numpy's LAPACK SVD where the kernel runs a Jacobi iteration."""
import numpy as np

ALIGN_NONE, ALIGN_SCALE, ALIGN_BEST, ALIGN_ROTATION = 0, 1, 2, 3
MODES = {"none": ALIGN_NONE, "scale": ALIGN_SCALE, "best": ALIGN_BEST, "rotation": ALIGN_ROTATION}
GAN_JOINTS = [1, 2, 4, 5, 7, 8, 12, 15, 16, 17, 18, 19, 20, 21]            # run_gan.py:2087


def select(pred, gt, joints=None, root=None):
    """p, g float64 [B,J,3]: the rows `joints` of both sets after both were centred on their row `root`"""
    p, g = np.asarray(pred, dtype=np.float64), np.asarray(gt, dtype=np.float64)
    if root is not None and root >= 0:
        p, g = p - p[:, root:root + 1], g - g[:, root:root + 1]
    if joints is not None:
        p, g = p[:, list(joints)], g[:, list(joints)]
    return p, g


def cross_covariance(p, g):
    """(A [B,3,3] = X0^T Y0 of the unit-norm centred sets, muX, normX, normY, Y0) with X = g the target and Y = p"""
    with np.errstate(divide="ignore", invalid="ignore"):
        muX, muY = g.mean(1, keepdims=True), p.mean(1, keepdims=True)
        X0, Y0 = g - muX, p - muY
        normX, normY = np.sqrt((X0 ** 2).sum((1, 2))), np.sqrt((Y0 ** 2).sum((1, 2)))
        X0, Y0 = X0 / normX[:, None, None], Y0 / normY[:, None, None]
        return np.einsum("nja,njb->nab", X0, Y0), muX, normX, normY, Y0


def polar(A, rotation_only):
    """(T [B,3,3] = V U^T, the sum of singular values that goes with it, the singular values) of A = U diag(s) V^T; a matrix
    with a non-finite entry gives NaN"""
    A = np.asarray(A, dtype=np.float64).reshape(-1, 3, 3)
    ok = np.isfinite(A).all((1, 2))
    U, s, Vt = np.linalg.svd(np.where(ok[:, None, None], A, np.eye(3)))
    V = np.swapaxes(Vt, 1, 2).copy()
    s = s.copy()
    if rotation_only:
        neg = np.linalg.det(V @ np.swapaxes(U, 1, 2)) < 0
        V[neg, :, 2] *= -1
        s[neg, 2] *= -1
    T = V @ np.swapaxes(U, 1, 2)
    T[~ok], s[~ok] = np.nan, np.nan
    return T, s.sum(1), s


def per_pose(pred, gt, joints=None, root=None, align=ALIGN_BEST):
    """dict: raw, aligned, d, scale float64 [B]; Z float64 [B,J,3]; dist_raw, dist_aligned float64 [B,J]; sv [B,3] (modes 2, 3).
    A pose with a non-finite coordinate among its selected joints is NaN throughout."""
    p, g = select(pred, gt, joints, root)
    B = p.shape[0]
    with np.errstate(divide="ignore", invalid="ignore"):
        A, muX, normX, normY, Y0 = cross_covariance(p, g)
        sv = np.full((B, 3), np.nan)
        if align == ALIGN_NONE:
            Z, scale = p.copy(), np.ones(B)
        elif align == ALIGN_SCALE:
            scale = (p * g).sum((1, 2)) / (p * p).sum((1, 2))
            Z = scale[:, None, None] * p
        elif align in (ALIGN_BEST, ALIGN_ROTATION):
            T, tr, sv = polar(A, align == ALIGN_ROTATION)
            Z = (normX * tr)[:, None, None] * (Y0 @ T) + muX
            scale = tr * normX / normY
        else:
            raise ValueError(f"align = {align}")
        dist_raw = np.sqrt(((p - g) ** 2).sum(-1))
        dist_al = np.sqrt(((Z - g) ** 2).sum(-1))
        d = ((Z - g) ** 2).sum((1, 2)) / normX ** 2
        out = dict(raw=dist_raw.mean(1), aligned=dist_al.mean(1), d=d, scale=np.asarray(scale, dtype=np.float64), Z=Z, dist_raw=dist_raw,
                   dist_aligned=dist_al, sv=sv)
    bad = ~(np.isfinite(p).all((1, 2)) & np.isfinite(g).all((1, 2)))
    for k in ("raw", "aligned", "d", "scale", "Z", "dist_raw", "dist_aligned"):
        out[k] = np.array(out[k], dtype=np.float64)
        out[k][bad] = np.nan
    return out


def summary(pp, thresholds=()):
    """float64 [4 + 2 T]: B, mean raw, mean aligned, mean d, then the share of the B J joint distances strictly below each
    threshold, raw and aligned"""
    th = np.asarray(thresholds, dtype=np.float64).reshape(-1)
    B = len(pp["raw"])
    with np.errstate(invalid="ignore"):
        pck_raw = [(pp["dist_raw"] < t).mean() for t in th]
        pck_al = [(pp["dist_aligned"] < t).mean() for t in th]
    return np.array([B, pp["raw"].mean(), pp["aligned"].mean(), pp["d"].mean()] + pck_raw + pck_al, dtype=np.float64)


def conditioning(pred, gt, joints=None, root=None):
    """(s3 / s1, (s2 - s3) / s1) of every pose's normalised cross-covariance: what the comparison bounds are conditioned on"""
    p, g = select(pred, gt, joints, root)
    A = cross_covariance(p, g)[0]
    ok = np.isfinite(A).all((1, 2))
    s = np.linalg.svd(np.where(ok[:, None, None], A, 0.0), compute_uv=False)
    with np.errstate(divide="ignore", invalid="ignore"):
        r3, gap = s[:, 2] / s[:, 0], (s[:, 1] - s[:, 2]) / s[:, 0]
    r3[~ok], gap[~ok] = 0.0, 0.0
    return np.nan_to_num(r3), np.nan_to_num(gap)
