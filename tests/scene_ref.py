"""The yardstick of the scene compositor (scene_composite_kernel, pg_scene.hip): P people's depth-sorted sample
lists of a pixel merged by depth and composited, restated in float64 / float32 (tests/test_scene_host.py pins it on the CPU,
tests/test_gpu_scene_stages.py, tests/test_gpu_scene_edges.py and tests/test_gpu_scene.py measure the kernel and the scene frames
by it).

Per list, alpha is the oracle's (oracle.anerf_oracle.composite, as tests/composite_ref.reference calls it: the deltas of the
person's OWN list, the last one 1e10, times |d|) and the colour its one line.  The samples of a pixel are then put in the order
(z, person, index) by a stable lexicographic sort, the transmittance is a sequential cumprod of 1 - alpha + 1e-10 over that order,
and the sums are raw2outputs' (nerf.py:150-205) plus one sum per person.  With one person this is composite_ref.reference.

Inputs are generated, rounded to float32 and only then handed to both sides (composite_ref's rule): both precisions see the same
depths, so the same order, and no case needs to be excluded -- not even one whose people share depths (make_scene_ties): equal
float32 depths are equal in float64, and the order of equal depths is (person, index) on both sides.  Bounds: composite_ref.bound /
deviation, unchanged.

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
    covered by nobody and pixel 5 by everybody ("many": more of both, all along the pixels)"""
    if kind == "all":
        return np.ones((P, n), dtype=bool)
    m = rng.random((P, n)) < 0.6
    if kind == "many":              # for tens of thousands of pixels: nobody on every 17th, everybody on every 19th from pixel 5 on
        m[:, ::17] = False
        m[:, 5::19] = True
    m[:, [3, 40]] = False
    m[:, 5] = True
    return m


def _raws(rng, n, S, density):
    """[n,S,4] float32: class A's colours; a density that leaves a list translucent: total optical depth ~ 0.2 .. 1.5 whatever S is
    (the last sample, delta 1e10, is opaque unless it is dead)"""
    rw = np.empty((n, S, 4))
    rw[..., :3] = rng.normal(0.0, 2.0, (n, S, 3))
    pre = rng.uniform(0.05, 0.4, (n, S)) * (8.0 / S)
    if density == "softplus":
        pre = pre + cr.SOFTPLUS_SHIFT - 3.0          # softplus(pre - shift) ~ exp(-3 + small): thin
        hot = rng.integers(0, S, n)
        pre[np.arange(n), hot] = cr.SOFTPLUS_SHIFT + 20.0 + rng.uniform(0.1, 1.0, n)      # the linear branch of torch's softplus
    else:
        pre[:, -1] = np.where(rng.random(n) < 0.5, -0.1, pre[:, -1])                     # half the lists end dead: sum w < 1
    rw[..., 3] = pre * cr.DENSITY_SCALE
    return f32(rw)


def _pack(rng, here_p, zp, rw):
    """list p of a scene: the present pixels' rows of zp [n,S] / rw [n,S,4] in a shuffled order, plus two rows no pixel refers to;
    -> z [m,S], raw [m,S,4], rows [n] (-1: absent)"""
    n, S = zp.shape
    m = int(here_p.sum()) + 2
    slot = rng.permutation(m)[:m - 2]
    zl, rl = np.zeros((m, S), dtype=np.float32), np.zeros((m, S, 4), dtype=np.float32)
    pix = np.nonzero(here_p)[0]
    zl[slot], rl[slot] = zp[pix], rw[pix]
    rows = np.full(n, -1, dtype=np.int32)
    rows[pix] = slot
    return zl, rl, rows


def _shifted(rays, by):
    """rays with near and far moved back by `by` [n] (rounded to float32)"""
    rb = rays.copy()
    rb[:, 6] = f32(rays[:, 6] + by)
    rb[:, 7] = f32(rays[:, 7] + by)
    return rb


def _scene(S, density, rays, lists):
    z, raw, rows = (list(x) for x in zip(*lists))
    return {"S": S, "density": density, "dirs": np.ascontiguousarray(rays[:, 3:6]), "z": z, "raw": raw,
            "rows": np.ascontiguousarray(np.stack(rows)), "rays": rays}


def make_scene(P, S, density, kind="mixed", n=N_PIX, overlap=True):
    """P lists over n pixels: class A's depths and colours (composite_ref.jittered_depths: strictly increasing, uneven), person p's
    depth range shifted by 0.35 p of the range so that the lists of a pixel interleave (overlap=False: one behind the other), a
    density that leaves the front lists translucent; list p holds its present pixels' rows in a shuffled order, plus two rows no
    pixel refers to."""
    rng = cr._rng(11, P, S, cr.DENSITIES.index(density), kind == "all", overlap, n)
    rays = cr.make_rays(rng, n)
    here = presence(rng, P, n, kind)
    span = (rays[:, 7] - rays[:, 6]).astype(np.float64)
    lists = []
    for p in range(P):
        zp = cr.jittered_depths(rng, _shifted(rays, (0.35 if overlap else 1.25) * p * span), S)
        lists.append(_pack(rng, here[p], zp, _raws(rng, n, S, density)))
    return _scene(S, density, rays, lists)


TIE_KINDS = ("same", "half", "runs", "flat")
# (P, S, density, kind) of the tie scenes the device is measured on: both ends of each instantiation (2 / 4 / 8 lists), E = 1 .. 4
TIE_CASES = [(P, S, den, kind) for (P, S, den) in [(2, 5, "relu"), (2, 65, "relu"), (2, 65, "softplus"), (3, 64, "relu"), (4, 33, "relu"),
                                                   (5, 33, "relu"), (8, 256, "relu")] for kind in TIE_KINDS]


def _pairs(z):
    """depths repeating in pairs (composite_ref.make_case_ties "pairs"): z_1 = z_0, z_3 = z_2, ..."""
    z = z.copy()
    z[:, 1::2] = z[:, 0:2 * (z.shape[1] // 2):2]
    return z


def _mix(rng, own, front):
    """`own` [n,S] with about half of its entries replaced by entries of `front` [n,S] at random indices, sorted again"""
    n, S = own.shape
    take = np.argsort(rng.random((n, S)), -1)[:, :S // 2]           # S / 2 different indices of `front` per pixel
    put = np.argsort(rng.random((n, S)), -1)[:, :S // 2]
    out = own.copy()
    np.put_along_axis(out, put, np.take_along_axis(front, take, -1), -1)
    return np.sort(out, -1)


def make_scene_ties(P, S, density, kind, n=N_PIX):
    """make_scene (mixed presence, shuffled rows, two unused rows per list, every person its own colours and densities) with depths
    that different people of a pixel share -- the order of equal depths is (person, index):
      "same"  every person's depths of a pixel are person 0's: the merged order is (0,0), (1,0), ..., (0,1), (1,1), ...;
      "half"  person p > 0 holds S / 2 of person 0's depths, taken at random indices, among S - S / 2 of its own (0.35 p of the range
              further back), sorted;
      "runs"  the depths repeat in pairs within a list; person 1 has person 0's runs, person p > 1 half of them among its own;
      "flat"  make_scene's depths (no tie), but on about a fifth of the pixels (pixel 5, which everybody covers, among them)
              near = far for everybody: all depths of the pixel are equal, every delta but each list's last is 0."""
    assert kind in TIE_KINDS
    rng = cr._rng(12, P, S, cr.DENSITIES.index(density), TIE_KINDS.index(kind), n)
    rays = cr.make_rays(rng, n)
    here = presence(rng, P, n, "mixed")
    span = (rays[:, 7] - rays[:, 6]).astype(np.float64)
    flat = rng.random(n) < 0.2
    flat[5] = True
    z0 = cr.jittered_depths(rng, rays, S)
    if kind == "runs":
        z0 = _pairs(z0)
    lists = []
    for p in range(P):
        own = cr.jittered_depths(rng, _shifted(rays, 0.35 * p * span), S)
        if p == 0 or kind == "same":
            zp = z0
        elif kind == "half":
            zp = _mix(rng, own, z0)
        elif kind == "runs":
            # whole runs move: the pair (2 j, 2 j + 1) of `own` becomes a pair of z0 or stays
            zp = z0 if p == 1 else np.sort(np.where(np.repeat(rng.random((n, (S + 1) // 2)) < 0.5, 2, -1)[:, :S], z0, _pairs(own)), -1)
        else:
            zp = np.where(flat[:, None], rays[:, 6:7], own)
        if kind == "flat" and p == 0:
            zp = np.where(flat[:, None], rays[:, 6:7], z0)
        rw = _raws(rng, n, S, density)
        if kind == "flat":      # the one live sample of a flat pixel's list is live indeed: no list ends dead there
            rw[flat, -1, 3] = np.abs(rw[flat, -1, 3])
        lists.append(_pack(rng, here[p], f32(zp), rw))
    return _scene(S, density, rays, lists)


def make_scene_many(P, n):
    """n pixels of S = 3 samples, relu, "many" presence: cheap enough for more pixels than the kernel's grid holds waves"""
    rng = cr._rng(13, P, n)
    rays = cr.make_rays(rng, n)
    here = presence(rng, P, n, "many")
    span = (rays[:, 7] - rays[:, 6]).astype(np.float64)
    return _scene(3, "relu", rays, [_pack(rng, here[p], cr.jittered_depths(rng, _shifted(rays, 0.35 * p * span), 3), _raws(rng, n, 3, "relu"))
                                    for p in range(P)])


DISP_S = 16


def make_scene_disp(n=N_PIX):
    """relu, two people everywhere, one live sample per list and pixel (index 1 + (pixel + 3 p) % (S - 2)), each with half of
    sum w = 1e-7 (even pixels) or 1e-9 (odd pixels) on the float64 restatement (composite_ref.make_case_disp with the weight split
    between two lists); "live": [2,n] the live indices"""
    S = DISP_S
    rng = cr._rng(14, n)
    rays = cr.make_rays(rng, n)
    span = (rays[:, 7] - rays[:, 6]).astype(np.float64)
    dn = np.linalg.norm(rays[:, 3:6].astype(np.float64), axis=-1)
    r = np.arange(n)
    target = np.where(r % 2 == 0, cr.DISP_TARGETS[0], cr.DISP_TARGETS[1])
    z, raw, live = [], [], []
    for p in range(2):
        zp = cr.jittered_depths(rng, _shifted(rays, 0.35 * p * span), S)
        rw = np.zeros((n, S, 4))
        rw[..., :3] = rng.normal(0.0, 2.0, (n, S, 3))
        rw[..., 3] = -rng.uniform(0.05, 0.4, (n, S)) * cr.DENSITY_SCALE
        k = 1 + (r + 3 * p) % (S - 2)
        delta = (zp[r, k + 1].astype(np.float64) - zp[r, k]) * dn
        rw[r, k, 3] = 0.5 * target / delta * cr.DENSITY_SCALE
        z.append(zp)
        raw.append(f32(rw))
        live.append(k)
    return {"S": S, "density": "relu", "dirs": np.ascontiguousarray(rays[:, 3:6]), "z": z, "raw": raw,
            "rows": np.ascontiguousarray(np.stack([r, r]).astype(np.int32)), "rays": rays, "live": np.stack(live)}


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
