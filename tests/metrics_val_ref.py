"""float64 numpy restatement of pg_frame_metrics_val (include/posegen_hip.h): the bilinear upsampling `up` of a
low-resolution float32 frame to the bank's size -- F.interpolate(mode='bilinear', align_corners=False) with the index arithmetic in
double, every product and sum rounded on its own, one rounding to float32 -- and the twelve sums: the eight of
tests/metrics_ref.py on the upsampled frame, then (n_valid, se_valid, n_valid_map, ssim_valid) over a second rectangle."""
import numpy as np

from tests import metrics_ref as ref

WIN = ref.WIN
SUMS = ref.SUMS + ("n_valid", "se_valid", "n_valid_map", "ssim_valid")


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
    """float64 [12]: ref.frame_sums of up(lo) inside `box`, then the four valid sums (0 without `valid`).  `valid` = (vx0, vy0,
    vx1, vy1) in frame pixels; it may reach outside the box or miss it."""
    H, W = img.shape[:2] if HW is None else HW
    U = up(lo, H, W)
    out = np.zeros(12)
    out[:8] = ref.frame_sums(img, mask, bkgd, U, box, taps, use_bg)
    if valid is None:
        return out
    x0, y0, x1, y1 = (int(v) for v in box)
    vx0, vy0, vx1, vy1 = (int(v) for v in valid)
    h, w = y1 - y0, x1 - x0
    yy, xx = np.mgrid[y0:y1, x0:x1]
    inside = ((xx >= vx0) & (xx < vx1) & (yy >= vy0) & (yy < vy1)).astype(np.float64)
    gt = ref.ground_truth(img, mask, bkgd, use_bg)
    y = gt[y0:y1, x0:x1].astype(np.float64)
    x = U[y0:y1, x0:x1].astype(np.float64)
    out[8], out[9] = 3.0 * inside.sum(), (((y - x) ** 2) * inside[..., None]).sum()
    if h >= WIN and w >= WIN:
        vc = inside[WIN // 2:h - WIN // 2, WIN // 2:w - WIN // 2]
        out[10], out[11] = 3.0 * vc.sum(), (ref.ssim_map(x, y, taps) * vc[..., None]).sum()
    return out


def area_average(hi: np.ndarray, rf: int) -> np.ndarray:
    """float32 [H//rf, W//rf, 3]: the mean of every rf x rf block of float32 hi (trailing rows / columns that fill no block are
    dropped), in float64, rounded once"""
    h, w = hi.shape[0] // rf, hi.shape[1] // rf
    t = hi[:h * rf, :w * rf].astype(np.float64).reshape(h, rf, w, rf, -1)
    return np.ascontiguousarray(t.mean(axis=(1, 3)).astype(np.float32))
