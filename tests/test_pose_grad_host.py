"""The pose gradient's spec on the host (no GPU): the per-(point, joint) Jacobian that embed_bwd_kernel (pg_train.hip) implements,
restated in float64 NumPy and checked against torch autograd of the oracle's embedding, and the oracle's float64 dL/dskts pinned
to the reference's own (tests/golden/train_grads_pose*.npz, tools/gen_golden.py: gen_train_grads_pose).

The embedding of point p under bone j (skt = [R t; 0 1]): q = R p + t, v = |q|, r = q / max(v, eps), l = R d,
e = l / max(|l|, eps), eps = 1e-12; the cutoff weights w(v) = 1 - sigmoid(tau (v - c)) and w' = -tau s (1 - s); channels
v part row * 24 + j (rows v, sin 2^k v, cos 2^k v, times w_v), direction part 360 + 3 j + c (r), view part
432 + row * 72 + 3 j + c (rows e_c, sin 2^k e_c, cos 2^k e_c, times w_d).  Given dX, the gradient of one (point, joint):
  dv = sum_rows dXv (w_v f'(v) + w_v' f(v)) + sum_rows,c dXd w_d' g(e_c),   de_c = sum_rows dXd w_d g'(e_c),
  dq = r dv + (I - r r^T) / v dr,   dl = (I - e e^T) / |l| de,   dR += dq (x) p + dl (x) d,   dt += dq,
and at v or |l| below eps torch's subgradients: torch.norm gives 0, F.normalize 1 / eps."""
import math

import numpy as np
import pytest
import torch

from oracle import anerf_oracle as orc
from tests.helpers import cfg_from_golden, default_dtype, load_golden, loss_of, model_for, oracle_cfg

EPS = 1e-12
J, CH_V, CH_X = 24, 360, 432


def pose_grad_ref(pts, rays_d, skts, dX, cutoff, tau_v, tau_d, multires=7, multires_views=4):
    """float64 dL/dskts [n,24,4,4] of L = sum(X * dX), X = embed_points(pts, rays_d, skts) without the frame-code column.
    pts [n,s,3], rays_d [n,3], skts [n|1,24,4,4], dX [n,s,1080], cutoff [48] (v cutoffs, then view cutoffs) or a scalar."""
    pts, rays_d, skts, dX = (np.asarray(a, dtype=np.float64) for a in (pts, rays_d, skts, dX))
    n, s = pts.shape[:2]
    skts = np.broadcast_to(skts, (n,) + skts.shape[1:])
    cut = np.broadcast_to(np.asarray(cutoff, dtype=np.float64), (2 * J,)) if np.ndim(cutoff) else np.full(2 * J, float(cutoff))
    out = np.zeros((n, J, 4, 4))
    for ray in range(n):
        d = rays_d[ray]
        for j in range(J):
            R, t = skts[ray, j, :3, :3], skts[ray, j, :3, 3]
            l = R @ d
            ln = math.sqrt(l @ l)
            e = l / max(ln, EPS)
            gR, gt, gde = np.zeros((3, 3)), np.zeros(3), np.zeros(3)
            for i in range(s):
                p = pts[ray, i]
                q = R @ p + t
                v = math.sqrt(q @ q)
                x = dX[ray, i]
                sv = _sigmoid(tau_v * (v - cut[j]))
                wv, dwv = 1.0 - sv, -tau_v * sv * (1.0 - sv)
                dv = x[j] * (wv + dwv * v)
                for k in range(multires):
                    f = 2.0 ** k
                    sn, cs = math.sin(f * v), math.cos(f * v)
                    dv += x[(1 + 2 * k) * J + j] * (wv * f * cs + dwv * sn) + x[(2 + 2 * k) * J + j] * (-wv * f * sn + dwv * cs)
                sd = _sigmoid(tau_d * (v - cut[J + j]))
                wd, dwd = 1.0 - sd, -tau_d * sd * (1.0 - sd)
                for c in range(3):
                    g = x[CH_X + 3 * j + c]
                    de, gw = g * wd, g * e[c]
                    for k in range(multires_views):
                        f = 2.0 ** k
                        sn, cs = math.sin(f * e[c]), math.cos(f * e[c])
                        gs, gc = x[CH_X + (1 + 2 * k) * 3 * J + 3 * j + c], x[CH_X + (2 + 2 * k) * 3 * J + 3 * j + c]
                        de += wd * f * (gs * cs - gc * sn)
                        gw += gs * sn + gc * cs
                    gde[c] += de
                    dv += dwd * gw
                dr = x[CH_V + 3 * j: CH_V + 3 * j + 3]
                if v >= EPS:
                    r = q / v
                    dq = r * dv + (dr - r * (r @ dr)) / v
                else:
                    dq = (q / v * dv if v > 0 else 0.0) + dr / EPS
                gR += np.outer(dq, p)
                gt += dq
            dl = (gde - e * (e @ gde)) / ln if ln >= EPS else gde / EPS
            gR += np.outer(dl, d)
            out[ray, j, :3, :3], out[ray, j, :3, 3] = gR, gt
    return out


def _sigmoid(x):
    return 1.0 / (1.0 + math.exp(-x)) if x >= 0 else math.exp(x) / (1.0 + math.exp(x))


def _random_pose(rng, n):
    """[n,24,4,4]: rotations times a scale near 1, translations of a body's size"""
    A = rng.randn(n, J, 3, 3)
    Q, _ = np.linalg.qr(A)
    sk = np.zeros((n, J, 4, 4))
    sk[..., :3, :3] = Q * rng.uniform(0.8, 1.2, size=(n, J, 1, 1))
    sk[..., :3, 3] = 0.3 * rng.randn(n, J, 3)
    sk[..., 3, 3] = 1.0
    return sk


def _autograd(pts, d, skts, dX, cfg):
    with default_dtype(torch.float64):
        sk = torch.tensor(skts, requires_grad=True)
        x = orc.embed_points(torch.tensor(pts), torch.tensor(d), sk, cfg)
        (x * torch.tensor(dX)).sum().backward()
    return sk.grad.numpy()


@pytest.mark.parametrize("tau", [20.0, 200.0, 2000.0])
def test_pose_jacobian_matches_torch_autograd_of_the_oracle_embedding(tau):
    """Random points, poses and upstream gradients; points near and far beyond the cutoff (tau up to 2000, where the cutoff
    is a step), and a point exactly at a joint (v = 0: torch's subgradients)."""
    rng = np.random.RandomState(int(tau))
    n, s = 3, 6
    cutoff = 0.5
    skts = _random_pose(rng, n)
    pts = 0.5 * rng.randn(n, s, 3)
    # on the cutoff sphere of joint 2 (within 1 / tau of it: the weight's slope is largest there), far beyond it, near it
    R, t = skts[0, 2, :3, :3], skts[0, 2, :3, 3]
    for i, rad in ((0, cutoff + 0.3 / tau), (1, 6.0 * cutoff), (2, cutoff - 0.5 / tau)):
        u = rng.randn(3)
        pts[0, i] = np.linalg.solve(R, rad * u / np.linalg.norm(u) - t)
    # a point at joint 5 of ray 1: t = 0 and p = 0 make q = 0 exactly
    skts[1, 5, :3, 3] = 0.0
    pts[1, 0] = 0.0
    d = rng.randn(n, 3)
    dX = rng.randn(n, s, 1080)
    cfg = orc.OracleConfig(tau_v=tau, tau_d=tau, cutoff_dist=cutoff)
    got = pose_grad_ref(pts, d, skts, dX, cutoff, tau, tau)
    want = _autograd(pts, d, skts, dX, cfg)
    assert np.all(got[..., 3, :] == 0) and np.all(want[..., 3, :] == 0)
    # the point at the joint: F.normalize's 1 / eps reaches the pose (as under torch) -- compare that bone on its own scale
    at = np.zeros(got.shape, dtype=bool)
    at[1, 5] = True
    assert np.abs(want[1, 5]).max() > 1e9
    np.testing.assert_allclose(got[at], want[at], rtol=1e-9, atol=0)
    scale = np.abs(want[~at]).max()
    err = np.abs(got[~at] - want[~at]).max() / scale
    print(f"tau {tau}: largest deviation {err:.2e} of the largest entry {scale:.3e}")
    assert err < 1e-10


def test_pose_jacobian_at_zero_direction():
    """|l| = 0 (a degenerate bone transform that maps the ray direction to 0): F.normalize's subgradient 1 / eps"""
    rng = np.random.RandomState(3)
    skts = _random_pose(rng, 1)
    d = np.array([[0.0, 0.0, 1.0]])
    skts[0, 7, :3, 2] = 0.0                   # R d = 0 for joint 7
    pts = 0.4 * rng.randn(1, 4, 3)
    dX = rng.randn(1, 4, 1080)
    cfg = orc.OracleConfig(tau_v=20.0, tau_d=20.0, cutoff_dist=0.5)
    got = pose_grad_ref(pts, d, skts, dX, 0.5, 20.0, 20.0)
    want = _autograd(pts, d, skts, dX, cfg)
    np.testing.assert_allclose(got, want, rtol=1e-9, atol=1e-9 * np.abs(want).max())


def _oracle_pose_step(g, dtype=torch.float64):
    """the oracle's training step on a train_grads_pose fixture with the per-ray poses requiring a gradient: (loss, dL/dskts)"""
    cfg = cfg_from_golden(g)
    wc, wf, tv, td = model_for(cfg, int(g["seed_model"]))
    kp_idx = g["kp_idx"]
    with default_dtype(dtype):
        cast = lambda a: torch.tensor(np.asarray(a), dtype=dtype)
        nets = [{k: cast(v) for k, v in w.items()} for w in (wc, wf)]
        sk = cast(g["skts"][kp_idx]).requires_grad_(True)
        draws = {k: cast(g[k]) for k in ("t_rand", "u_rand", "noise0", "noise1", "ray_noise") if k in g}
        cams = cast(g["cams"]) if "cams" in g else None
        out = orc.render_rays(cast(g["ray_batch"]), sk, cast(g["cyl"][kp_idx]), oracle_cfg(cfg, g["tau_v"], g["tau_d"]), nets[0], nets[1],
                              cfg.n_samples, cfg.n_importance, cams=cams, draws=draws)
        loss = loss_of(out, cast(g["target"]))
        loss.backward()
    return float(loss.detach()), sk.grad.double().numpy()


def scale_of(a):
    """the comparison scale of a gradient tensor: max(largest entry, norm / sqrt(size)) (test_gpu_train.py)"""
    a = np.asarray(a, dtype=np.float64).reshape(-1)
    return max(float(np.abs(a).max()), float(np.linalg.norm(a)) / math.sqrt(a.size), 1e-30)


@pytest.mark.parametrize("name", ["train_grads_pose", "train_grads_pose_h36m"])
def test_oracle_pose_gradient_matches_the_reference(name):
    """The oracle's float64 dL/dskts against the reference's own fp32 autograd: every entry within 1e-4 of the tensor's scale,
    the norm within 1e-4 (test_oracle_float64.py's pinning of the parameter gradients)."""
    g = load_golden(name)
    assert g["dskts"].shape == (g["ray_batch"].shape[0], 24, 4, 4)
    loss, got = _oracle_pose_step(g)
    ref = g["dskts"].astype(np.float64)
    assert abs(loss - float(g["loss"])) <= 1e-5 * max(1.0, abs(float(g["loss"])))
    sc = scale_of(ref)
    ent = float(np.abs(got - ref).max()) / sc
    nrm = abs(float(np.linalg.norm(got)) - float(np.linalg.norm(ref))) / float(np.linalg.norm(ref))
    print(f"{name}: dL/dskts scale {sc:.3e}, entries within {ent:.2e}, norm within {nrm:.2e}")
    assert np.all(ref[..., 3, :] == 0) and np.all(got[..., 3, :] == 0)
    assert ent <= 1e-4 and nrm <= 1e-4
    assert len(np.unique(g["kp_idx"])) == g["skts"].shape[0]
