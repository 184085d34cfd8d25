"""A float64 restatement of the fused embed + MLP stage, per point: the bone-local transform (encoders.py:8-37), the RelDist and
VecNorm encoders with the ray direction in bone space (encoders.py:101-122, 172-193), the cutoff embedding
(cutoff_embedder.py:111-174) and the NeRF MLP (nerf.py:94-148).  Plain torch on the CPU; nothing here masks, skips or factorises.

Beyond oracle.embed_points / mlp_forward it takes the two embedders' `cutoff_dist` as 24-vectors, poses shared or per ray, a
frame-code index per ray (-1: the mean row, embedding.py:25-26) and rays with depths or explicit points.  tests/test_eval_ref_host.py
pins it to the oracle, to the reference's own raw vectors and to the per-joint-cutoff fixture eval_edges.npz.

`quant` applies a precision's operand rounding to every linear layer (oracle._linear: operands rounded, products exact, fp32
accumulate) on the float64 embedding rounded to fp32 -- used only to measure how far operand rounding alone moves raw.

`mut` = a deliberate error, for the host checks that the edge cases can tell it from rounding (never set by a GPU test).
"""
import numpy as np
import torch

from oracle import anerf_oracle as orc

J = 24
F64 = torch.float64
MUTATIONS = ("neighbour_pose", "neighbour_code", "cutoff_slot_order", "cutoff_swapped", "limb_dropped", "top_octave_sign",
             "z_shifted")
# a permutation of the joints that is not the identity on any limb group: stands for "cutoffs read in slot order"
SLOT_ORDER = np.roll(np.arange(J), 1)


def t64(a):
    return torch.as_tensor(np.asarray(a, dtype=np.float64) if not torch.is_tensor(a) else a).to(F64)


def bone_local(pts, skts):
    """pts [n,S,3], skts [n|1,J,4,4] -> q [n,S,J,3] = R_j p + t_j of the point's own ray's pose."""
    pts, skts = t64(pts), t64(skts)
    if skts.shape[0] == 1:
        skts = skts.expand(pts.shape[0], -1, -1, -1)
    return torch.einsum("njab,nsb->nsja", skts[..., :3, :3], pts) + skts[:, None, :, :3, 3]


def ray_local(rays_d, skts, n):
    """rays_d [n,3] -> R_j d [n,J,3]"""
    rays_d, skts = t64(rays_d), t64(skts)
    if skts.shape[0] == 1:
        skts = skts.expand(n, -1, -1, -1)
    return torch.einsum("njab,nb->nja", skts[..., :3, :3], rays_d)


def _unit(x):
    """F.normalize: x / max(|x|, 1e-12)"""
    return x / torch.linalg.norm(x, dim=-1, keepdim=True).clamp_min(1e-12)


def cutoff_weight(v, tau, cutoff):
    """1 - sigmoid(tau (v - cutoff)), cutoff [J]"""
    return torch.sigmoid(-float(tau) * (v - t64(cutoff)))


def _bands(x, w, n_freq, top_sign=1.0):
    """x, w [..., C] -> rows (x, sin 2^0 x, cos 2^0 x, ..., cos 2^(L-1) x) each times w, flattened row-major [..., (1+2L) C]"""
    rows = [x]
    for k in range(n_freq):
        s = top_sign if k == n_freq - 1 else 1.0
        rows += [s * torch.sin(2.0 ** k * x), s * torch.cos(2.0 ** k * x)]
    return (torch.stack(rows, dim=-2) * w[..., None, :]).flatten(start_dim=-2)


def embed(q, dl, cutoff_v, cutoff_d, tau_v, tau_d, multires=7, multires_views=4, mut=None):
    """q [n,S,J,3], dl [n,J,3] -> (x_in [n,S,J(1+2L)+3J], x_view [n,S,3J(1+2Lv)])"""
    n, S = q.shape[:2]
    cv, cd = t64(cutoff_v), t64(cutoff_d)
    if mut == "cutoff_slot_order":
        cv, cd = cv[SLOT_ORDER], cd[SLOT_ORDER]
    if mut == "cutoff_swapped":
        cv, cd = cd, cv
    v = torch.linalg.norm(q, dim=-1)                                    # [n,S,J]
    r = _unit(q).flatten(start_dim=-2)                                  # [n,S,3J]
    e = _unit(dl).flatten(start_dim=-2)[:, None, :].expand(n, S, -1)    # [n,S,3J]
    wv, wd = cutoff_weight(v, tau_v, cv), cutoff_weight(v, tau_d, cd)
    if mut == "limb_dropped":                   # the in-range joint that carries most weight, per point, is left out
        drop = torch.nn.functional.one_hot(wv.argmax(-1), J).to(F64)
        wv, wd = wv * (1 - drop), wd * (1 - drop)
    sgn = -1.0 if mut == "top_octave_sign" else 1.0
    xv = _bands(v, wv, multires, sgn)
    xd = _bands(e, wd.repeat_interleave(3, dim=-1), multires_views, sgn)
    return torch.cat([xv, r], -1), xd


def _lin(x, w, b, quant):
    if quant is None:
        return x @ t64(w).T + (0 if b is None else t64(b))
    return orc._linear(x.float(), torch.as_tensor(w).float(), None if b is None else torch.as_tensor(b).float(), quant).to(F64)


def mlp(x_in, x_view, code, weights, net_depth=8, skips=(4,), quant=None):
    """x_in [P,432], x_view [P,648], code [P,16] or None -> (raw [P,4] = (rgb_raw, sigma_raw), layer-0 pre-activation [P,256])"""
    if quant is not None:                       # the kernels' inputs are fp32 values
        x_in, x_view = x_in.float().to(F64), x_view.float().to(F64)
    W = lambda k: weights[k]
    h, pre0 = x_in, None
    for i in range(net_depth):
        pre = _lin(h, W(f"pts_linears.{i}.weight"), W(f"pts_linears.{i}.bias"), quant)
        pre0 = pre if i == 0 else pre0
        h = torch.relu(pre)
        if i in skips:
            h = torch.cat([x_in, h], -1)
    sigma = _lin(h, W("alpha_linear.weight"), W("alpha_linear.bias"), quant)
    feat = _lin(h, W("feature_linear.weight"), W("feature_linear.bias"), quant)
    xv = [feat, x_view] + ([] if code is None else [code])
    g = torch.relu(_lin(torch.cat(xv, -1), W("views_linears.0.weight"), W("views_linears.0.bias"), quant))
    rgb = _lin(g, W("rgb_linear.weight"), W("rgb_linear.bias"), quant)
    return torch.cat([rgb, sigma], -1), pre0


def _codes(weights, cams, n):
    """the frame code of every ray [n,16]: cams None / one element / [n]; index < 0 = the mean row"""
    if "framecodes.codes.weight" not in weights:
        return None
    tab = t64(weights["framecodes.codes.weight"])
    tab = torch.cat([tab, tab.mean(0, keepdim=True)], 0)
    idx = torch.full((n,), -1.0) if cams is None else torch.as_tensor(cams).reshape(-1).float()
    if idx.shape[0] == 1:
        idx = idx.expand(n)
    idx = idx.long()
    assert int(idx.max()) < tab.shape[0] - 1, "frame-code index out of range (the reference raises)"
    return tab[torch.where(idx < 0, torch.full_like(idx, tab.shape[0] - 1), idx)]


def _shift_rows(t, by=1):
    """row i takes row i + by (the last rows wrap): 'the neighbour ray's' value"""
    return torch.roll(t, -by, 0)


def eval_rays(weights, ray_batch, z, skts, cutoff_v, cutoff_d, tau_v, tau_d, cams=None, quant=None, mut=None,
              multires=7, multires_views=4, net_depth=8, skips=(4,)):
    """Rays (o, d) = ray_batch[:, 0:6] at depths z [n,S] -> dict raw [n,S,4], pre0 [n,S,256] (float64)."""
    rb, z, skts = t64(ray_batch), t64(z), t64(skts)
    n, S = z.shape
    o, d = rb[:, 0:3], rb[:, 3:6]
    if mut == "z_shifted":
        z = torch.roll(z, -1, 1)
    if mut == "neighbour_pose":
        skts = _shift_rows(skts.expand(n, -1, -1, -1) if skts.shape[0] == 1 else skts, 2)   # (poses come in blocks of 2 rays)
    pts = o[:, None, :] + d[:, None, :] * z[..., None]
    q = bone_local(pts, skts)
    dl = ray_local(d, skts, n)
    x_in, x_view = embed(q, dl, cutoff_v, cutoff_d, tau_v, tau_d, multires, multires_views, mut)
    code = _codes(weights, cams, n)
    if code is not None:
        if mut == "neighbour_code":
            code = _shift_rows(code)
        code = code[:, None, :].expand(n, S, -1).reshape(n * S, -1)
    raw, pre0 = mlp(x_in.reshape(n * S, -1), x_view.reshape(n * S, -1), code, weights, net_depth, skips, quant)
    return {"raw": raw.reshape(n, S, 4), "pre0": pre0.reshape(n, S, -1)}


def eval_points(weights, pts, skts, cutoff_v, cutoff_d, tau_v, tau_d, quant=None, mut=None, multires=7, multires_views=4,
                net_depth=8, skips=(4,)):
    """Explicit points [P,3] of one pose, zero view direction, the mean frame code (render_pts_density, raycasters.py:598-646)
    -> dict raw [P,4] (only raw[:, 3] means anything), pre0 [P,256]."""
    pts = t64(pts).reshape(-1, 1, 3)
    P = pts.shape[0]
    q = bone_local(pts, t64(skts).reshape(-1, J, 4, 4)[:1])
    dl = torch.zeros(P, J, 3, dtype=F64)
    x_in, x_view = embed(q, dl, cutoff_v, cutoff_d, tau_v, tau_d, multires, multires_views, mut)
    code = _codes(weights, None, P)
    raw, pre0 = mlp(x_in.reshape(P, -1), x_view.reshape(P, -1), code, weights, net_depth, skips, quant)
    return {"raw": raw, "pre0": pre0}
