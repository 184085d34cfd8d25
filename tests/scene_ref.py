"""The yardstick of the scene compositor (scene_composite_kernel, pg_scene.hip): P people's depth-sorted sample
lists of a pixel merged by depth and composited, restated in float64 / float32 (tests/test_scene_host.py pins it on the CPU,
tests/test_gpu_scene_stages.py and tests/test_gpu_scene.py measure the kernel and the scene frames by it).

Per list, alpha is the oracle's (oracle.anerf_oracle.composite, as tests/composite_ref.reference calls it: the deltas of the
person's OWN list, the last one 1e10, times |d|) and the colour its one line.  The samples of a pixel are then put in the order
(z, person, index) by a stable lexicographic sort, the transmittance is a sequential cumprod of 1 - alpha + 1e-10 over that order,
and the sums are raw2outputs' (nerf.py:150-205) plus one sum per person.  With one person this is composite_ref.reference.

Inputs are generated, rounded to float32 and only then handed to both sides (composite_ref's rule): both precisions see the same
depths, so the same order, and no case needs to be excluded.  Bounds: composite_ref.bound / deviation, unchanged.

A scene for these functions is a dict: S, density (or an OracleConfig under "cfg"), dirs [n_pix,3], z / raw = lists of P arrays
[n_p,S] / [n_p,S,4], rows [P,n_pix] int32 (the row of pixel i in list p, negative or >= n_p: person p does not cover it).
"""
import numpy as np
import torch

from oracle import anerf_oracle as orc
from tests import composite_ref as cr
from tests.helpers import default_dtype

N_PIX = 70                  # 35 workgroups of two waves
PEOPLE = (1, 2, 3, 8)
SAMPLES = (2, 33, 64, 65, 129, 256)

f32 = cr.f32


def _present(scene, p):
    rows = np.asarray(scene["rows"][p], dtype=np.int64)
    return rows, (rows >= 0) & (rows < scene["z"][p].shape[0])


def reference(scene, dtype=torch.float64):
    """rgb_map [n_pix,3], disp_map, acc_map, wsum [n_pix], person_acc [P,n_pix] as numpy arrays, computed in `dtype`"""
    P, S = len(scene["z"]), scene["S"]
    n = scene["dirs"].shape[0]
    cfg = scene.get("cfg") or cr.oracle_config(scene["density"])
    with default_dtype(dtype):
        dirs = torch.tensor(np.asarray(scene["dirs"]), dtype=dtype)
        zkey = torch.full((n, P, S), float("inf"), dtype=dtype)        # absent samples sort last, with alpha 0
        zval = torch.zeros((n, P, S), dtype=dtype)
        alpha = torch.zeros((n, P, S), dtype=dtype)
        rgb = torch.zeros((n, P, S, 3), dtype=dtype)
        for p in range(P):
            rows, here = _present(scene, p)
            if not here.any():
                continue
            idx = torch.tensor(np.nonzero(here)[0])
            z = torch.tensor(np.asarray(scene["z"][p]), dtype=dtype)[rows[here]]
            raw = torch.tensor(np.asarray(scene["raw"][p]), dtype=dtype)[rows[here]]
            alpha[idx, p] = orc.composite(raw, z, dirs[idx], cfg)["alpha"]
            rgb[idx, p] = torch.sigmoid(raw[..., :3]) * (1 + 2 * cfg.rgb_eps) - cfg.rgb_eps
            zkey[idx, p] = z
            zval[idx, p] = z
        person = torch.arange(P)[None, :, None].expand(n, P, S).reshape(n, P * S)
        index = torch.arange(S)[None, None, :].expand(n, P, S).reshape(n, P * S)
        # stable lexicographic order on (z, person, index): lexsort's LAST key is the primary one
        order = torch.tensor(np.lexsort((index.numpy(), person.numpy(), zkey.reshape(n, P * S).numpy()), axis=-1))
        take = lambda x: torch.gather(x.reshape(n, P * S), 1, order)
        a, z, who = take(alpha), take(zval), take(person)
        c = torch.gather(rgb.reshape(n, P * S, 3), 1, order[..., None].expand(-1, -1, 3))
        trans = torch.cumprod(torch.cat([torch.ones(n, 1), 1. - a + 1e-10], -1), -1)[:, :-1]
        w = a * trans
        rgb_map = torch.sum(w[..., None] * c, -2)
        depth = torch.sum(w * z, -1)
        wsum = torch.sum(w, -1)
        disp = 1. / torch.max(1e-10 * torch.ones_like(depth), depth / (wsum + 1e-10))
        disp = disp * (~torch.isclose(wsum, torch.tensor(0.))).to(dtype)
        acc = torch.minimum(wsum, torch.tensor(1.))
        pacc = torch.stack([torch.minimum(torch.sum(w * (who == p).to(dtype), -1), torch.tensor(1.)) for p in range(P)])
    return {"rgb_map": rgb_map.numpy(), "disp_map": disp.numpy(), "acc_map": acc.numpy(), "wsum": wsum.numpy(),
            "person_acc": pacc.numpy()}


# ---- generators ---------------------------------------------------------------------------------------------------------------
def presence(rng, P, n, kind):
    """[P,n] bool.  "all": everybody everywhere; "mixed": every person covers a random ~60 % of the pixels, pixels 3 and 40 are
    covered by nobody and pixel 5 by everybody"""
    if kind == "all":
        return np.ones((P, n), dtype=bool)
    m = rng.random((P, n)) < 0.6
    m[:, [3, 40]] = False
    m[:, 5] = True
    return m


def make_scene(P, S, density, kind="mixed", n=N_PIX, overlap=True):
    """P lists over n pixels: class A's depths and colours (composite_ref.jittered_depths: strictly increasing, uneven), person p's
    depth range shifted by 0.35 p of the range so that the lists of a pixel interleave (overlap=False: one behind the other), a
    density that leaves the front lists translucent; list p holds its present pixels' rows in a shuffled order, plus two rows no
    pixel refers to."""
    rng = cr._rng(11, P, S, cr.DENSITIES.index(density), kind == "all", overlap, n)
    rays = cr.make_rays(rng, n)
    here = presence(rng, P, n, kind)
    z, raw, rows = [], [], np.full((P, n), -1, dtype=np.int32)
    for p in range(P):
        m = int(here[p].sum()) + 2
        rb = rays.copy()
        span = (rays[:, 7] - rays[:, 6]).astype(np.float64)
        shift = (0.35 if overlap else 1.25) * p * span
        rb[:, 6] = f32(rays[:, 6] + shift)
        rb[:, 7] = f32(rays[:, 7] + shift)
        zp = cr.jittered_depths(rng, rb, S)
        rw = np.empty((n, S, 4))
        rw[..., :3] = rng.normal(0.0, 2.0, (n, S, 3))
        # total optical depth of a list ~ 0.2 .. 1.5 whatever S is (the last sample, delta 1e10, is opaque unless it is dead)
        pre = rng.uniform(0.05, 0.4, (n, S)) * (8.0 / S)
        if density == "softplus":
            pre = pre + cr.SOFTPLUS_SHIFT - 3.0          # softplus(pre - shift) ~ exp(-3 + small): thin
            hot = rng.integers(0, S, n)
            pre[np.arange(n), hot] = cr.SOFTPLUS_SHIFT + 20.0 + rng.uniform(0.1, 1.0, n)      # the linear branch of torch's softplus
        else:
            pre[:, -1] = np.where(rng.random(n) < 0.5, -0.1, pre[:, -1])                     # half the lists end dead: sum w < 1
        rw[..., 3] = pre * cr.DENSITY_SCALE
        slot = rng.permutation(m)[:m - 2]
        zl, rl = np.zeros((m, S), dtype=np.float32), np.zeros((m, S, 4), dtype=np.float32)
        pix = np.nonzero(here[p])[0]
        zl[slot], rl[slot] = zp[pix], f32(rw)[pix]
        rows[p, pix] = slot
        z.append(zl)
        raw.append(rl)
    return {"S": S, "density": density, "dirs": np.ascontiguousarray(rays[:, 3:6]), "z": z, "raw": raw, "rows": rows, "rays": rays}


def single(case):
    """a composite_ref case as a one-person scene: pixel i = ray i"""
    n = case["rays"].shape[0]
    return {"S": case["S"], "density": case["density"], "dirs": np.ascontiguousarray(case["rays"][:, 3:6]), "z": [case["z"]],
            "raw": [case["raw"]], "rows": np.arange(n, dtype=np.int32)[None]}


def permuted(scene, perm):
    """the same scene with person k = the old person perm[k]"""
    return {**scene, "z": [scene["z"][k] for k in perm], "raw": [scene["raw"][k] for k in perm],
            "rows": np.ascontiguousarray(scene["rows"][list(perm)])}


def cross_list_ties(scene):
    """True if two different people's samples of one pixel share a depth"""
    P = len(scene["z"])
    for i in range(scene["dirs"].shape[0]):
        zs = [scene["z"][p][_present(scene, p)[0][i]] for p in range(P) if _present(scene, p)[1][i]]
        for a in range(len(zs)):
            for b in range(a + 1, len(zs)):
                if np.intersect1d(zs[a], zs[b]).size:
                    return True
    return False
