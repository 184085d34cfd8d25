"""A float64 torch restatement of what an A-NeRF training step optimises (core/trainer.py:193-205, 321-443): the photometric loss of
both passes with the masked BCE regulariser, the 6-D pose regulariser with its temporal term, and the gradient norms.  Every input is
taken as the float32 it is and widened; everything after that is float64 with autograd.  tests/test_train_loss_ref.py holds it
against the reference's own float32 values (tests/golden/train_losses.npz); the device path (csrc/pg_trainloss.hip) is held against it."""
import math

import numpy as np
import torch

BCE_EPS = 1e-8

SUMMARY_KEYS = ("total_loss", "rgb_loss", "rgb_loss0", "reg_loss", "reg_loss0", "psnr", "psnr0", "alpha")


def _f64(x, grad=False):
    if x is None:
        return None
    t = torch.as_tensor(np.asarray(x.detach().cpu() if torch.is_tensor(x) else x, dtype=np.float32)).to(torch.float64)
    return t.requires_grad_(True) if grad else t


def _elem(loss_fn, beta, d):
    if loss_fn == "MSE":
        return d * d
    if loss_fn == "L1" or beta == 0.0:
        return d.abs()
    if loss_fn != "Huber":
        raise NotImplementedError(loss_fn)
    ad = d.abs()
    return torch.where(ad < beta, 0.5 * d * d / beta, ad - 0.5 * beta)


def photometric_graph(passes, tg, bg, y, *, loss_fn, loss_beta=0.1, use_background=True, coarse_weight=1.0, reg_fn=None, reg_coef=0.0,
                      base_bg=1.0):
    """The formulas on float64 tensors (any device), autograd intact: `passes` = [("", rgb, acc), ("0", rgb0, acc0)]; returns
    (total_loss, vals) with vals the tensors under the reference's keys plus the BCE ray counts n_bce / n_bce0."""
    if reg_fn not in (None, "BCE"):
        raise ValueError("reg_fn L1 / MSE: the reference's total_loss has shape [n] there and its backward() raises")
    vals, total = {}, 0.0
    for tag, rgb, acc in passes:
        pred = rgb + (1.0 - acc)[..., None] * (bg if bg is not None else base_bg) if use_background else rgb
        loss = _elem(loss_fn, float(loss_beta), pred - tg).mean()
        if tag:
            loss = loss * coarse_weight
        vals["psnr" + tag] = (-10.0 * torch.log(((pred.detach() - tg) ** 2).mean()) / math.log(10.0))
        vals["rgb_loss" + tag] = loss
        total = total + loss
        if reg_fn == "BCE":
            bce = -(y * torch.log(acc + BCE_EPS) + (1.0 - y) * torch.log(1.0 - acc + BCE_EPS))
            keep = y < 1.0
            reg = bce[keep].mean() * reg_coef
            vals["reg_loss" + tag] = reg
            vals["n_bce" + tag] = keep.sum().double()
            total = total + reg
    vals["alpha"] = passes[0][2].detach().mean()
    vals["total_loss"] = total
    return total, vals


def photometric(rgb_map, acc_map, rgb0, acc0, target, bgs, fgs, **settings):
    """(values, grads) on float32 host arrays: values float64 python floats under SUMMARY_KEYS plus `n_bce`, `n_bce0` (absent passes and
    terms left out); grads float64 numpy arrays d_rgb_map, d_acc_map, d_rgb0, d_acc0 of total_loss (zeros where no path exists)."""
    passes = [("", _f64(rgb_map, True), _f64(acc_map, True))]
    if rgb0 is not None:
        passes.append(("0", _f64(rgb0, True), _f64(acc0, True)))
    total, vals = photometric_graph(passes, _f64(target), _f64(bgs), _f64(fgs), **settings)
    leaves = [t for _, rgb, acc in passes for t in (rgb, acc)]
    got = torch.autograd.grad(total, leaves, allow_unused=True)
    names = ("d_rgb_map", "d_acc_map", "d_rgb0", "d_acc0")
    grads = {k: (torch.zeros_like(t) if g is None else g).numpy() for k, t, g in zip(names, leaves, got)}
    return {k: float(v.detach()) for k, v in vals.items()}, grads


def bone6(rots):
    return rots[..., :3, :2].flatten(start_dim=-2)


def pose_graph(r, k, idx, a_rots, a_kps, *, tol, coef, ext_scale, prev=None, nxt=None, temp_val=None, temp_coef=0.0):
    """The pose regulariser on float64 tensors (any device), autograd intact: (total, vals).  `tol` is rounded to float32 first: the
    value the reference's float32 comparison and subtraction see."""
    tol = float(np.float32(tol))
    bones, reg = bone6(r), bone6(a_rots[idx])
    x = ((reg - bones) ** 2)[:, 1:]
    kp_loss = torch.where((x > tol) | torch.isnan(x), x - tol, torch.zeros_like(x)).sum(-1).mean() * coef       # (a NaN stays, as through lerp)
    vals, total = {"kp_loss": kp_loss}, kp_loss
    if prev is not None:
        pb, pk, nb, nk = bone6(prev[0]), prev[1], bone6(nxt[0]), nxt[1]
        ang = (((bones - pb) - (nb - bones)) ** 2).sum(-1)
        joint = (((k - pk) - (nk - k)) ** 2).sum(-1)
        temp = ((ang + joint) * temp_val[..., None]).mean() * temp_coef
        vals["temp_loss"] = temp
        total = total + temp
    vals["MPJPC"] = ((a_kps[idx] - k.detach()) ** 2).sum(-1).sqrt().mean() / ext_scale
    vals["total"] = total
    return total, vals


def pose_regulariser(rots, kps, kp_idx, anchor_rots, anchor_kps, *, tol, coef, ext_scale, prev=None, nxt=None, temp_val=None, temp_coef=0.0):
    """(values, grads) on float32 host arrays: kp_loss, temp_loss (with prev = (rots, kps) and nxt), MPJPC, total; d_rots [n,24,3,3],
    d_kps [n,24,3] of total."""
    r, k = _f64(rots, True), _f64(kps, True)
    idx = torch.as_tensor(np.asarray(kp_idx), dtype=torch.long)
    pair = lambda p: None if p is None else (_f64(p[0]), _f64(p[1]))
    total, vals = pose_graph(r, k, idx, _f64(anchor_rots), _f64(anchor_kps), tol=tol, coef=coef, ext_scale=ext_scale, prev=pair(prev),
                             nxt=pair(nxt), temp_val=_f64(temp_val), temp_coef=temp_coef)
    got = torch.autograd.grad(total, [r, k], allow_unused=True)
    grads = {n: (torch.zeros_like(t) if g is None else g).numpy() for n, t, g in zip(("d_rots", "d_kps"), (r, k), got)}
    return {n: float(v.detach()) for n, v in vals.items()}, grads


def grad_norms(tensors):
    """(total_norm, avg_norm, per-tensor norms) of get_gradnorm in float64, nothing rounded in between"""
    sq = [float((_f64(t) ** 2).sum()) for t in tensors]
    total = math.fsum(sq)
    return math.sqrt(total), math.sqrt(total / len(sq)), np.sqrt(np.array(sq))


def ulp32(x):
    """the spacing of float32 at |x| (float64 array), the smallest normal's below it"""
    a = np.maximum(np.abs(np.asarray(x, dtype=np.float64)), 2.0 ** -126)
    return 2.0 ** (np.floor(np.log2(a)) - 23)


# ---- the cases of tests/golden/train_losses.npz -----------------------------------------------------------------------------------------
def golden_case(g, name):
    """the arrays of one case of the fixture, without the `<case>/` prefix"""
    return {k[len(name) + 1:]: v for k, v in g.items() if k.startswith(name + "/")}


def photo_settings(c):
    reg = str(c["reg_fn"])
    return dict(loss_fn=str(c["loss_fn"]), loss_beta=float(c["loss_beta"]), use_background=bool(int(c["use_background"])),
                coarse_weight=float(c["coarse_weight"]), reg_fn=None if reg == "None" else reg, reg_coef=float(c["reg_coef"]))


def photo_inputs(c):
    """(rgb_map, acc_map, rgb0, acc0, target, bgs, fgs) of a photometric case; rgb0 / acc0 / bgs None where the case has none"""
    return (c["rgb_map"], c["acc_map"], c.get("rgb0"), c.get("acc0"), c["target"], c.get("bgs"), c["fgs"])


def kp_inputs(c):
    """a kp case as the per-ray arrays the trainer sees: rots, kps = the table's rows (popt_layer(kp_idx)), and with the temporal term
    prev / next = the rows at kp_idx - 1 (numpy: -1 is the last pose) and (kp_idx + 1) % N"""
    idx = c["kp_idx"].astype(np.int64)
    N = len(c["rots"])
    kw = dict(tol=float(c["tol"]), coef=float(c["coef"]), ext_scale=float(c["ext_scale"]))
    if int(c["temporal"]):
        kw.update(prev=(c["rots"][idx - 1], c["kps"][idx - 1]), nxt=(c["rots"][(idx + 1) % N], c["kps"][(idx + 1) % N]),
                  temp_val=c["temp_val"], temp_coef=float(c["temp_coef"]))
    return (c["rots"][idx], c["kps"][idx], idx, c["anchor_rots"], c["anchor_kps"]), kw
