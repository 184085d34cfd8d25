"""float64 numpy restatement of the regressor's input (posegen_amd/regressor_batches.py, csrc/pg_regressor.hip), written from the
formulas at pg_regressor_input's declaration (include/posegen_hip.h): crop, divide by 255, normalise, and per axis a mirrored
Gaussian followed by order-1 interpolation at pixel centres, each as a dense [n,n] / [R,n] operator.  tests/test_regressor_ref.py
holds it to scipy.ndimage.gaussian_filter + scipy.ndimage.zoom (the two calls skimage's resize makes); the GPU tests compare the
kernel with it alone.  No scipy here: the GPU tests run where it may be missing."""
import numpy as np

U = 2.0 ** -24                                     # float32 unit roundoff


def mirror(i, n):
    """reflection about the centres of the first and the last of n pixels"""
    if n == 1:
        return 0
    p = 2 * (n - 1)
    j = i % p
    return j if j < n else p - j


def radius(n, R):
    """(sigma, r) of an axis n -> R"""
    s = n / R
    sigma = max(0.0, (s - 1.0) / 2.0)
    return sigma, int(4.0 * sigma + 0.5)


def gaussian_operator(n, R):
    """[n,n]: g = G v"""
    sigma, r = radius(n, R)
    G = np.zeros((n, n))
    if r == 0:
        return np.eye(n)
    t = np.arange(-r, r + 1)
    k = np.exp(-(t * t) / (2.0 * sigma * sigma))
    k = k / k.sum()
    for i in range(n):
        for tt, kk in zip(t, k):
            G[i, mirror(i + int(tt), n)] += kk
    return G


def sample_operator(n, R):
    """[R,n]: out = L g"""
    L = np.zeros((R, n))
    for o in range(R):
        x = (o + 0.5) * n / R - 0.5
        i0 = int(np.floor(x))
        t = x - i0
        L[o, mirror(i0, n)] += 1.0 - t
        L[o, mirror(i0 + 1, n)] += t
    return L


def normalise(u8, mean, std):
    """uint8 [h,w,3] -> float64 [3,h,w]"""
    v = u8.astype(np.float64) / 255.0
    return ((v - np.asarray(mean, np.float64)) / np.asarray(std, np.float64)).transpose(2, 0, 1)


def resize(v, out_hw):
    """float64 [3,h,w] -> [3,Ry,Rx]"""
    _, h, w = v.shape
    Ry, Rx = out_hw
    g = gaussian_operator(h, Ry) @ v @ gaussian_operator(w, Rx).T
    return sample_operator(h, Ry) @ g @ sample_operator(w, Rx).T


def regressor_input(image, box, R, mean, std):
    """one item: uint8 [H,W,3], box (x0, y0, x1, y1) -> float64 [3,R,R]"""
    x0, y0, x1, y1 = (int(v) for v in box)
    return resize(normalise(image[y0:y1, x0:x1], mean, std), (R, R))


def bound(h, w, R, mean, std):
    """N u M of DESIGN.md 2.14: N = (2 r_y + 1) + (2 r_x + 1) + 24, M the largest normalised magnitude"""
    m, s = np.asarray(mean, np.float64), np.asarray(std, np.float64)
    M = float((np.maximum(m, 1.0 - m) / s).max())
    N = (2 * radius(h, R)[1] + 1) + (2 * radius(w, R)[1] + 1) + 24
    return N * U * M
