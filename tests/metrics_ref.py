"""float64 numpy restatement of pg_frame_metrics (include/posegen_hip.h) at the kernel's own inputs: the bank's
bytes, the float32 frame and the float32 Gaussian taps widened to double.  Plays the role tests/composite_ref.py plays for the
compositing kernels: the kernel is held to it within reordering error, and it is held to the reference's own float32 values
(tests/golden/frame_metrics.npz) within their measured deviation.

Below it the restatement of pg_frame_metrics_val: the bilinear upsampling `up` of a low-resolution float32 frame
to the bank's size -- F.interpolate(mode='bilinear', align_corners=False) with the index arithmetic in double, every product and
sum rounded on its own, one rounding to float32 -- and the twelve sums: `frame_sums` of the upsampled frame, then (n_valid,
se_valid, n_valid_map, ssim_valid) over a second rectangle."""
import os
import re

import numpy as np

WIN = 11
C1, C2 = 1e-4, 9e-4
SUMS = ("n", "se", "n_fg", "se_fg", "n_map", "ssim", "n_fg_map", "ssim_fg")
SUMS_VAL = SUMS + ("n_valid", "se_valid", "n_valid_map", "ssim_valid")
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def header_taps() -> np.ndarray:
    """The float32 taps compiled into the library: the hex literals of TAPS in csrc/pg_metrics_plan.h"""
    src = open(os.path.join(REPO, "posegen_amd", "csrc", "pg_metrics_plan.h")).read()
    body = re.search(r"TAPS\[WIN\]\s*=\s*\{([^}]*)\}", src).group(1)
    vals = [float.fromhex(v.strip().rstrip("f")) for v in body.split(",")]
    taps = np.asarray(vals, dtype=np.float32)
    assert len(vals) == WIN and all(float(t) == v for t, v in zip(taps, vals))        # every literal is a float32
    return taps


def ground_truth(img, mask, bkgd, use_bg) -> np.ndarray:
    """float32 [H,W,3]: bytes / 255 as run_render.py:912, 944 forms them (a float64 quotient, `.astype(np.float32)`); with `use_bg`
    the background's byte where the mask byte is 0 (:935-937 with a binary mask)"""
    src = img
    if use_bg:
        src = np.where((mask > 0)[..., None], img, bkgd)
    return (src / 255.).astype(np.float32)


def _valid_conv(a, g):
    """separable valid 11 x 11 convolution of a [h,w,c] float64 with the 1-D taps g (float64)"""
    h, w = a.shape[:2]
    rows = sum(g[t] * a[:, t:t + w - WIN + 1] for t in range(WIN))
    return sum(g[t] * rows[t:t + h - WIN + 1] for t in range(WIN))


def ssim_map(x, y, taps) -> np.ndarray:
    """ssim_map of pytorch_msssim.ssim (L = 1) of float64 [h,w,c] crops, [(h-10),(w-10),c]"""
    g = np.asarray(taps, dtype=np.float32).astype(np.float64)
    mu1, mu2 = _valid_conv(x, g), _valid_conv(y, g)
    mu1_sq, mu2_sq, mu1_mu2 = mu1 * mu1, mu2 * mu2, mu1 * mu2
    sigma1_sq = _valid_conv(x * x, g) - mu1_sq
    sigma2_sq = _valid_conv(y * y, g) - mu2_sq
    sigma12 = _valid_conv(x * y, g) - mu1_mu2
    v1 = 2.0 * sigma12 + C2
    v2 = sigma1_sq + sigma2_sq + C2
    return ((2.0 * mu1_mu2 + C1) * v1) / ((mu1_sq + mu2_sq + C1) * v2)


def frame_sums(img, mask, bkgd, rgb, box, taps, use_bg=False) -> np.ndarray:
    """(n, se, n_fg, se_fg, n_map, ssim, n_fg_map, ssim_fg) float64 [8].  img uint8 [H,W,3], mask uint8 [H,W] or None (no
    foreground), bkgd uint8 [H,W,3] or None, rgb float32 [H,W,3], box (x0, y0, x1, y1)."""
    assert rgb.dtype == np.float32 and img.dtype == np.uint8
    x0, y0, x1, y1 = (int(v) for v in box)
    h, w = y1 - y0, x1 - x0
    gt = ground_truth(img, mask, bkgd, use_bg)
    y = gt[y0:y1, x0:x1].astype(np.float64)
    x = rgb[y0:y1, x0:x1].astype(np.float64)
    m = np.zeros((h, w)) if mask is None else (mask[y0:y1, x0:x1] > 0).astype(np.float64)
    sq = (y - x) ** 2
    out = np.zeros(8)
    out[0], out[1] = 3.0 * h * w, sq.sum()
    out[2], out[3] = 3.0 * m.sum(), (sq * m[..., None]).sum()
    if h >= WIN and w >= WIN:
        smap = ssim_map(x, y, taps)
        mc = m[WIN // 2:h - WIN // 2, WIN // 2:w - WIN // 2]
        out[4], out[5] = 3.0 * (h - WIN + 1) * (w - WIN + 1), smap.sum()
        out[6], out[7] = 3.0 * mc.sum(), (smap * mc[..., None]).sum()
    return out


def axis_taps(n_in: int, n_out: int):
    """(i0, i1, l1) of every output pixel of one axis: int64 [n_out], int64 [n_out], float64 [n_out]"""
    assert 1 <= n_in <= n_out
    d = np.arange(n_out, dtype=np.float64)
    src = np.maximum((np.float64(n_in) / np.float64(n_out)) * (d + 0.5) - 0.5, 0.0)
    i0 = np.minimum(src.astype(np.int64), n_in - 1)
    i1 = i0 + (i0 < n_in - 1)
    return i0, i1, src - i0


def up(lo: np.ndarray, H: int, W: int) -> np.ndarray:
    """float32 [H,W,3] from float32 lo [h,w,3], h <= H, w <= W"""
    assert lo.dtype == np.float32 and lo.ndim == 3
    y0, y1, ly1 = axis_taps(lo.shape[0], H)
    x0, x1, lx1 = axis_taps(lo.shape[1], W)
    t = lo.astype(np.float64)
    lx1, ly1 = lx1[None, :, None], ly1[:, None, None]
    lx0, ly0 = 1.0 - lx1, 1.0 - ly1
    a, b = t[y0][:, x0], t[y0][:, x1]
    c, d = t[y1][:, x0], t[y1][:, x1]
    top = lx0 * a + lx1 * b
    bot = lx0 * c + lx1 * d
    return np.ascontiguousarray((ly0 * top + ly1 * bot).astype(np.float32))        # (fancy indexing leaves its own memory order)


def frame_sums_val(img, mask, bkgd, lo, box, taps, use_bg=False, valid=None, HW=None) -> np.ndarray:
    """float64 [12]: frame_sums of up(lo) inside `box`, then the four valid sums (0 without `valid`).  `valid` = (vx0, vy0,
    vx1, vy1) in frame pixels; it may reach outside the box or miss it."""
    H, W = img.shape[:2] if HW is None else HW
    U = up(lo, H, W)
    out = np.zeros(12)
    out[:8] = frame_sums(img, mask, bkgd, U, box, taps, use_bg)
    if valid is None:
        return out
    x0, y0, x1, y1 = (int(v) for v in box)
    vx0, vy0, vx1, vy1 = (int(v) for v in valid)
    h, w = y1 - y0, x1 - x0
    yy, xx = np.mgrid[y0:y1, x0:x1]
    inside = ((xx >= vx0) & (xx < vx1) & (yy >= vy0) & (yy < vy1)).astype(np.float64)
    gt = ground_truth(img, mask, bkgd, use_bg)
    y = gt[y0:y1, x0:x1].astype(np.float64)
    x = U[y0:y1, x0:x1].astype(np.float64)
    out[8], out[9] = 3.0 * inside.sum(), (((y - x) ** 2) * inside[..., None]).sum()
    if h >= WIN and w >= WIN:
        vc = inside[WIN // 2:h - WIN // 2, WIN // 2:w - WIN // 2]
        out[10], out[11] = 3.0 * vc.sum(), (ssim_map(x, y, taps) * vc[..., None]).sum()
    return out


def area_average(hi: np.ndarray, rf: int) -> np.ndarray:
    """float32 [H//rf, W//rf, 3]: the mean of every rf x rf block of float32 hi (trailing rows / columns that fill no block are
    dropped), in float64, rounded once"""
    h, w = hi.shape[0] // rf, hi.shape[1] // rf
    t = hi[:h * rf, :w * rf].astype(np.float64).reshape(h, rf, w, rf, -1)
    return np.ascontiguousarray(t.mean(axis=(1, 3)).astype(np.float32))
