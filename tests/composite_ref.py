"""Glue between the oracle and the stage tests of sampling and compositing (tests/test_composite_ref_host.py pins it on the CPU,
tests/test_gpu_composite_stages.py measures the kernels by it).

The reference is the oracle itself (oracle.anerf_oracle: near_far_in_cylinder, coarse_z, composite, importance_z) run under
default_dtype(float64); the backward is torch.autograd on that forward.  Nothing of the operation is restated here except the one
line of the is_only pdf (is_only_weights: the line of tests/test_train_single_host.single_net_render and
tests/test_single_net_host._isample_np, pinned against the latter and the rays_single fixture by the host test) and the pdf -> cdf
step that the CASE CONDITIONS, not the comparisons, are evaluated on.

Every input array is generated, rounded to float32 and only then handed to both sides: `reference(case, float64)` widens the very
float32 values the kernel reads (neighbouring float32 depths differ exactly in float32, so both see the same deltas).

Bounds (`bound`): 4 x the deviation of the float32 oracle from the float64 oracle on the same case, never below 4 float32 ulps of
the output's largest magnitude.  The float32 oracle is the reference's own arithmetic; the factor 4 is for what a kernel
legitimately does differently (wave-scan order instead of a sequential cumprod / cumsum, the device's expf / log1pf).
"""
import warnings

import numpy as np
import torch

from oracle import anerf_oracle as orc
from posegen_amd.config import RenderConfig
from tests.helpers import default_dtype, oracle_cfg

N_RAYS = 70                 # 17 full workgroups of 4 waves and a half one
DENSITY_SCALE = 2.0         # (a power of two: raw.w / scale is exact, the pre-activation ranges below hold to the last bit)
SOFTPLUS_SHIFT = 1.0
SHAPES = [(3, 2), (33, 7), (64, 16), (65, 16), (127, 64), (129, 64), (192, 64), (193, 2), (254, 2), (256, 0)]
FORMS = ("plain", "is_only")
DENSITIES = ("relu", "softplus")
BWD_SHAPES = [(33, 7), (65, 16), (129, 64), (256, 0)]
SC_CHUNKS = (64, 96, 256, 300, 4096)
SC_SAMPLES = (2, 3, 64, 65, 256)
SC_RAYS = 700

# class A conditions (on the float64 reference)
MIN_CDF_STEP = 1e-4         # ten times the `den < 1e-5` threshold
MIN_U_GAP = 1e-6
MIN_Z_GAP = 1e-6            # relative


def render_cfg(density, single_net=False) -> RenderConfig:
    return RenderConfig(density_type=density, softplus_shift=SOFTPLUS_SHIFT, density_scale=DENSITY_SCALE, single_net=single_net)


def oracle_config(density):
    return oracle_cfg(render_cfg(density), 1.0, 1.0)


def class_a_cases():
    """(S, N, form, draws, density) of class A: the cross product, draws only where there are importance samples"""
    return [(S, N, f, dr, den) for (S, N) in SHAPES for f in FORMS for dr in ((False, True) if N > 0 else (False,)) for den in DENSITIES]


def case_id(c):
    S, N, form, draws, density = c
    return f"S{S}-N{N}-{form}-{'draws' if draws else 'det'}-{density}"


def _rng(*key):
    return np.random.default_rng([0x5eed] + [int(k) for k in key])


f32 = lambda a: np.ascontiguousarray(a, dtype=np.float32)


# ---- generators ---------------------------------------------------------------------------------------------------------------
def make_rays(rng, n):
    """[n,11] float32: |d| in [0.6, 0.9] or [1.1, 1.6] (never 1), near in [2, 3], far - near in [1, 2]"""
    o = rng.normal(0.0, 1.0, (n, 3))
    d = rng.normal(0.0, 1.0, (n, 3))
    d /= np.linalg.norm(d, axis=-1, keepdims=True)
    scale = np.where(rng.random(n) < 0.5, rng.uniform(0.6, 0.9, n), rng.uniform(1.1, 1.6, n))
    near = rng.uniform(2.0, 3.0, n)
    far = near + rng.uniform(1.0, 2.0, n)
    return f32(np.concatenate([o, d * scale[:, None], near[:, None], far[:, None], d], -1))


def jittered_depths(rng, rays, S):
    """(i + jitter) / S of the way from near to far, jitter in [0.1, 0.9]: strictly increasing, uneven deltas"""
    t = (np.arange(S)[None, :] + rng.uniform(0.1, 0.9, (rays.shape[0], S))) / S
    near, far = rays[:, 6:7].astype(np.float64), rays[:, 7:8].astype(np.float64)
    return f32(near + (far - near) * t)


def _smooth_sigma(rng, n, S, density):
    """raw sigma column: pre-activation raw.w / scale in [0.05, 0.4]; softplus: one (S < 100) or two samples per ray above
    shift + 20, the linear branch of torch's softplus"""
    pre = rng.uniform(0.05, 0.4, (n, S))
    if density == "softplus":
        for r in range(n):
            idx = rng.choice(S, 1 if S < 100 else 2, replace=False)
            pre[r, idx] = SOFTPLUS_SHIFT + 20.0 + rng.uniform(0.1, 1.0, idx.size)
    return pre * DENSITY_SCALE


def make_case_a(S, N, form, draws, density, n=N_RAYS, rays=None):
    """A class A case whose every ray meets the class conditions on the float64 reference: a ray that does not has its density
    column (and its draws) drawn again.  float32 arrays `rays`, `z`, `raw`, `noise` / `u_rand` (or None)."""
    rng = _rng(1, S, N, FORMS.index(form), draws, DENSITIES.index(density), n)
    rays = make_rays(rng, n) if rays is None else rays
    raw = np.empty((n, S, 4))
    raw[..., :3] = rng.normal(0.0, 2.0, (n, S, 3))
    raw[..., 3] = _smooth_sigma(rng, n, S, density)
    case = {"S": S, "N": N, "form": form, "density": density, "rays": rays, "z": jittered_depths(rng, rays, S), "raw": f32(raw),
            "noise": f32(rng.uniform(-0.03, 0.03, (n, S))) if draws else None,
            "u_rand": f32(rng.uniform(0.0, 1.0, (n, N))) if draws and N > 0 else None}
    for _ in range(64):
        ok = class_a_ok(case, reference(case, torch.float64))
        if ok.all():
            return case
        bad = np.nonzero(~ok)[0]
        case["raw"][bad, :, 3] = f32(_smooth_sigma(rng, bad.size, S, density))
        if case["u_rand"] is not None:
            case["u_rand"][bad] = f32(rng.uniform(0.0, 1.0, (bad.size, N)))
    raise AssertionError(f"no class A case for {case_id((S, N, form, draws, density))}")


def class_a_margins(case, ref):
    """per ray, on the reference `ref` of `case`: the smallest cdf step, the smallest |u - cdf entry|, the smallest relative gap of
    two of the S + N depths.  Two (u, cdf) pairs are left out of the second: u = 0 against cdf[0] = 0, exact on both sides (every
    cdf[1] is >= MIN_CDF_STEP), and the linspace's u = 1 against the last cdf entry 1 -+ rounding, where both outcomes of the search
    give the last bin's upper edge (t = 0 from it with `den` replaced, or t = 1 - O(eps) towards it over a last step that is, like
    every step, >= MIN_CDF_STEP)."""
    n = case["rays"].shape[0]
    if case["N"] == 0:
        return {"cdf_step": np.full(n, np.inf), "u_gap": np.full(n, np.inf), "z_gap": np.full(n, np.inf)}
    cdf, u, zf = ref["cdf"], ref["u"], ref["z_fine"]
    gap = np.abs(u[:, :, None] - cdf[:, None, :])
    gap[:, :, 0] = np.where(u == 0.0, np.inf, gap[:, :, 0])
    if case["u_rand"] is None:
        gap[:, -1, -1] = np.inf
    return {"cdf_step": np.diff(cdf, axis=-1).min(-1), "u_gap": gap.reshape(n, -1).min(-1),
            "z_gap": (np.diff(zf, axis=-1) / np.abs(zf[:, 1:])).min(-1)}


def class_a_ok(case, ref):
    m = class_a_margins(case, ref)
    return (m["cdf_step"] >= MIN_CDF_STEP) & (m["u_gap"] >= MIN_U_GAP) & (m["z_gap"] >= MIN_Z_GAP)


def make_case_b(S, N, density, with_noise, ld_new=None):
    """Class B: the merged form on z_fine / order of the float64 reference of the class A is_only case (rounded to float32 / int32)
    and a raw_new [n,ld_new,4] of its own; `a`: that class A case"""
    a = make_case_a(S, N, "is_only", False, density)
    ref = reference(a, torch.float64)
    rng = _rng(2, S, N, DENSITIES.index(density), with_noise)
    n, ld = a["rays"].shape[0], N if ld_new is None else ld_new
    raw_new = np.empty((n, ld, 4))
    raw_new[..., :3] = rng.normal(0.0, 2.0, (n, ld, 3))
    raw_new[..., 3] = _smooth_sigma(rng, n, ld, "relu")
    zf = f32(ref["z_fine"])
    assert np.all(np.diff(zf, axis=-1) > 0), "rounding to float32 must keep the merged depths distinct"
    return {"S": S, "N": N, "density": density, "rays": a["rays"], "z": a["z"], "raw": a["raw"], "z_fine": zf,
            "order": np.ascontiguousarray(ref["order"], dtype=np.int32), "raw_new": f32(raw_new),
            "noise1": f32(rng.uniform(-0.03, 0.03, (n, S + N))) if with_noise else None, "noise0": None, "a": a}


def make_case_b_bwd(S, N, density):
    """Class B for merged_composite_bwd_kernel: both noises, and (relu) on every second ray the coarse samples from S / 2 on and the
    new samples behind that depth are dead, so that both composites of those rays end at sum w clearly below 1.  z_fine and order
    stay the sorted merge they are: the backward takes the depths as given (the samples carry no gradient)."""
    b = make_case_b(S, N, density, True)
    rng = _rng(8, S, N)
    n = b["rays"].shape[0]
    b["noise0"] = f32(rng.uniform(-0.03, 0.03, (n, S)))
    if density == "relu":
        even = (np.arange(n) % 2 == 0)[:, None]
        z_new = np.take_along_axis(b["z_fine"], np.argsort(b["order"], -1, kind="stable")[:, S:], -1)
        dead_c = even & (np.arange(S)[None, :] >= S // 2)
        dead_n = even & (z_new > b["z"][:, S // 2 - 1:S // 2])
        b["raw"][..., 3] = np.where(dead_c, f32(-rng.uniform(0.05, 0.4, (n, S)) * DENSITY_SCALE), b["raw"][..., 3])
        b["raw_new"][..., 3] = np.where(dead_n, f32(-rng.uniform(0.05, 0.4, (n, N)) * DENSITY_SCALE), b["raw_new"][..., 3])
    return b


def coarse_of(b):
    """the coarse composite of a class B case as a plain case without importance samples"""
    return {"S": b["S"], "N": 0, "form": "plain", "density": b["density"], "rays": b["rays"], "z": b["z"], "raw": b["raw"],
            "noise": b["noise0"], "u_rand": None}


def make_case_opaque_bwd(S=65):
    """relu, for the exact edges of the backward: every ray has a fully opaque sample (pre-activation 1e4: alpha = 1 exactly in
    float32 and float64), every fourth ray (`first`) at index 0, ray r of the others at index r % (S - 1).  Everything behind it stays
    alive, so sum w > 1 by ~1e-10 in exact arithmetic; on the `first` rays it is 1.0f on the device too (w_0 = 1.0f, the rest >= 0):
    acc = min(sum w, 1) is locally constant there and d_acc reaches nothing."""
    c = make_case_a(S, 0, "plain", False, "relu")
    r = np.arange(N_RAYS)
    c["first"] = r % 4 == 0
    c["raw"][r, np.where(c["first"], 0, r % (S - 1)), 3] = 1e4 * DENSITY_SCALE
    return c


def make_case_e(S, N, density):
    """Class E: a class A case (plain, all draws) for composite_bwd_kernel.  relu: on every second ray the samples from a random
    index on are dead (pre-activation in [-0.4, -0.05]: sum w clearly below 1, the d_acc gate open), and a tenth of all samples is dead
    too; no pre-activation + noise is within 1e-6 of 0.  The other rays end in alpha = 1 (delta 1e10): sum w = 1 to rounding."""
    c = make_case_a(S, N, "plain", N > 0, density)
    if c["noise"] is None:
        c["noise"] = f32(_rng(3, S, N).uniform(-0.03, 0.03, c["z"].shape))
    if density == "relu":
        rng = _rng(4, S, N)
        n = c["rays"].shape[0]
        dead = rng.random((n, S)) < 0.1
        tail = rng.integers(S // 2, S, n)
        dead |= (np.arange(S)[None, :] >= tail[:, None]) & (np.arange(n)[:, None] % 2 == 0)
        c["raw"][..., 3] = np.where(dead, f32(-rng.uniform(0.05, 0.4, (n, S)) * DENSITY_SCALE), c["raw"][..., 3])
    return c


def cotangents(case, which, fine=False):
    """float32 cotangents of a class E / merged backward case: `which` = a subset of ("d_rgb", "d_acc", "d_rgb0", "d_acc0")"""
    n = case["rays"].shape[0]
    rng = _rng(5, case["S"], case["N"], fine)
    full = {"d_rgb": rng.normal(0, 1, (n, 3)), "d_acc": rng.normal(0, 1, n), "d_rgb0": rng.normal(0, 1, (n, 3)), "d_acc0": rng.normal(0, 1, n)}
    return {k: f32(v) for k, v in full.items() if k in which}


def gate_acc(d_acc, wsum):
    """d_acc with the rays at sum w ~ 1 (|sum w - 1| <= 1e-4 on the float64 reference) set to 0: min(sum w, 1) has a kink there and
    float32 may stand on its other side.  Those rays stay in every comparison."""
    return f32(np.where(np.abs(wsum - 1.0) > 1e-4, d_acc, 0.0))


def make_case_d(chunk, per_ray_cyl, n=SC_RAYS):
    """Class D: rays and cylinders with hits and misses in known places.  Group 0 of `chunk` rays has no miss, group 1 no hit,
    group 2 a single hit, the others hit or miss at random (one group at chunk 4096: mixed).  A hit passes the axis at <= 0.8 radius,
    a miss at >= 1.3 radius.  Returns rays [n,11], cyls [1|n,5], hit [n] bool, t_rand [n,256]."""
    rng = _rng(6, chunk, per_ray_cyl, n)
    group = np.arange(n) // chunk
    hit = rng.random(n) < 0.6
    if n > chunk:
        hit[group == 0] = True
        hit[group == 1] = False
        g2 = np.nonzero(group == 2)[0]
        if g2.size:
            hit[g2] = False
            hit[g2[g2.size // 2]] = True
    m = n if per_ray_cyl else 1
    cyl = np.stack([rng.normal(0, 0.3, m), rng.normal(0, 0.3, m), rng.uniform(0.5, 0.9, m), np.full(m, 1.0), np.full(m, -1.0)], -1)
    c = np.broadcast_to(cyl, (n, 5))
    phi = rng.uniform(0, 2 * np.pi, n)
    o_xz = c[:, :2] + 4.0 * np.stack([np.cos(phi), np.sin(phi)], -1)
    b = np.where(hit, rng.uniform(0.0, 0.8, n), rng.uniform(1.3, 2.0, n)) * c[:, 2] * np.where(rng.random(n) < 0.5, -1.0, 1.0)
    ang = phi + np.pi + np.arcsin(b / 4.0)            # towards the axis, passing it at the signed distance b
    s = np.where(rng.random(n) < 0.5, rng.uniform(0.6, 0.9, n), rng.uniform(1.1, 1.6, n))
    d = np.stack([np.cos(ang) * s, rng.normal(0, 0.2, n), np.sin(ang) * s], -1)
    o = np.stack([o_xz[:, 0], rng.normal(0, 0.3, n), o_xz[:, 1]], -1)
    near = rng.uniform(0.3, 0.6, n)
    far = near + rng.uniform(6.0, 8.0, n)
    rays = f32(np.concatenate([o, d, near[:, None], far[:, None], d / np.linalg.norm(d, axis=-1, keepdims=True)], -1))
    return {"chunk": chunk, "rays": rays, "cyls": f32(cyl), "hit": hit, "t_rand": f32(rng.uniform(0, 1, (n, max(SC_SAMPLES))))}


# ---- class C: exact edges -------------------------------------------------------------------------------------------------------
def _bare_case(S, N, form, density, n, key, u_rand=False, noise=False):
    """class A's rays, depths and colours without its conditions (the caller sets the density column)"""
    rng = _rng(7, key, S, N, n)
    rays = make_rays(rng, n)
    raw = np.zeros((n, S, 4))
    raw[..., :3] = rng.normal(0.0, 2.0, (n, S, 3))
    return {"S": S, "N": N, "form": form, "density": density, "rays": rays, "z": jittered_depths(rng, rays, S), "raw": f32(raw),
            "noise": f32(rng.uniform(-0.03, 0.03, (n, S))) if noise else None,
            "u_rand": f32(rng.uniform(0.0, 1.0, (n, N))) if u_rand else None}, rng


def make_case_empty(S, N, form):
    """relu, every sigma <= 0 (a fifth exactly 0): all weights 0, a uniform pdf.  S - 2 and N - 1 are to be coprime, so that no
    interior u of the linspace meets a cdf entry k / (S - 2)."""
    assert np.gcd(S - 2, N - 1) == 1
    c, rng = _bare_case(S, N, form, "relu", N_RAYS, 1)
    sig = -rng.uniform(0.05, 0.4, (N_RAYS, S)) * DENSITY_SCALE
    c["raw"][..., 3] = f32(np.where(rng.random((N_RAYS, S)) < 0.2, 0.0, sig))
    return c


def make_case_opaque_last(S, N):
    """relu, sigma pre-activation 1e4 at the last interior sample S - 2, the rest dead: every empty bin lies before the opaque one, its cdf
    steps 1e-5 / (1 + (S - 2) 1e-5) stand below the 1e-5 threshold by a relative S 1e-5 (float32 rounds the cdf there, ~1e-3, at
    1e-10)"""
    c, rng = _bare_case(S, N, "plain", "relu", N_RAYS, 2)
    c["raw"][..., 3] = f32(-rng.uniform(0.05, 0.4, (N_RAYS, S)) * DENSITY_SCALE)
    c["raw"][:, S - 2, 3] = 1e4 * DENSITY_SCALE
    return c


TIE_RAYS = {"flat": slice(0, 10), "pairs": slice(10, 20), "u_repeat": slice(20, N_RAYS)}


def make_case_ties(S, N, form, sorted_u):
    """rays 0..9: near = far, all depths equal; rays 10..19: the depths repeat in pairs; every ray: u_rand with repeated values
    (each draw twice), in random order or sorted"""
    c, rng = _bare_case(S, N, form, "relu", N_RAYS, 3, u_rand=True)
    c["raw"][..., 3] = f32(_smooth_sigma(rng, N_RAYS, S, "relu"))
    c["z"][TIE_RAYS["flat"]] = c["rays"][TIE_RAYS["flat"], 6:7]
    c["rays"][TIE_RAYS["flat"], 7] = c["rays"][TIE_RAYS["flat"], 6]
    p = c["z"][TIE_RAYS["pairs"]]
    p[:, 1::2] = p[:, 0:2 * (S // 2):2]
    c["z"][TIE_RAYS["pairs"]] = p
    u = c["u_rand"]
    u[:, N // 2:2 * (N // 2)] = u[:, :N // 2]
    c["u_rand"] = f32(np.sort(u, -1)) if sorted_u else f32(rng.permuted(u, axis=-1))
    return c


def make_case_nan_ray(S, N, form, ray=35):
    """a class A case (all draws) whose ray `ray` has NaN depths; `without`: the same case without that ray"""
    c = make_case_a(S, N, form, True, "relu")
    c["z"][ray] = np.nan
    keep = np.arange(N_RAYS) != ray
    without = {k: (v[keep] if isinstance(v, np.ndarray) else v) for k, v in c.items()}
    return c, without, keep


def make_case_many_rays(n=65536 + 5, S=8, N=2):
    """more rays than 16384 workgroups x 4 waves: a wave takes several rays and reuses its LDS rows"""
    c, rng = _bare_case(S, N, "plain", "relu", n, 4)
    c["raw"][..., 3] = f32(_smooth_sigma(rng, n, S, "relu"))
    return c


DISP_TARGETS = (1e-7, 1e-9)


def make_case_disp(S=16):
    """relu, one live sample per ray (index 1 + ray % (S - 2)), its sigma set for sum w = 1e-7 (even rays) or 1e-9 (odd rays) on
    the float64 reference: one decade to either side of isclose's 1e-8"""
    c, rng = _bare_case(S, 0, "plain", "relu", N_RAYS, 5)
    c["raw"][..., 3] = f32(-rng.uniform(0.05, 0.4, (N_RAYS, S)) * DENSITY_SCALE)
    k = 1 + np.arange(N_RAYS) % (S - 2)
    r = np.arange(N_RAYS)
    dn = np.linalg.norm(c["rays"][:, 3:6].astype(np.float64), axis=-1)
    delta = (c["z"][r, k + 1].astype(np.float64) - c["z"][r, k]) * dn
    target = np.where(r % 2 == 0, DISP_TARGETS[0], DISP_TARGETS[1])
    c["raw"][r, k, 3] = f32(target / delta * DENSITY_SCALE)
    c["live"] = k
    return c


# ---- the reference --------------------------------------------------------------------------------------------------------------
def _t(a, dtype, grad=False):
    return None if a is None else torch.tensor(np.asarray(a), dtype=dtype, requires_grad=grad)


def is_only_weights(w):
    """the is_only pdf (ray_utils.py:269-276) in the shape importance_z takes its weights: entry k of [:, 1:-1] is
    0.5 (max(w_l, w_k) + max(w_k, w_u)) + 0.01"""
    pw = 0.5 * (torch.maximum(w[:, :-2], w[:, 1:-1]) + torch.maximum(w[:, 1:-1], w[:, 2:])) + 0.01
    return torch.cat([torch.zeros_like(w[:, :1]), pw, torch.zeros_like(w[:, :1])], -1)


def _cdf(weights):
    """what importance_z forms of its weights before it searches -- for the case conditions only"""
    pw = weights[:, 1:-1] + 1e-5
    pdf = pw / torch.sum(pw, -1, keepdim=True)
    return torch.cat([torch.zeros_like(pdf[:, :1]), torch.cumsum(pdf, -1)], -1)


_MAPS = ("rgb_map", "disp_map", "acc_map", "alpha", "weights")


def reference(case, dtype=torch.float64):
    """the oracle's composite (+ importance samples, plain or is_only pdf) on the case's float32 arrays, in `dtype`: numpy arrays"""
    with default_dtype(dtype):
        rays, z, raw, noise, u = (_t(case[k], dtype) for k in ("rays", "z", "raw", "noise", "u_rand"))
        out = orc.composite(raw, z, rays[:, 3:6], oracle_config(case["density"]), noise)
        res = {k: out[k] for k in _MAPS}
        res["wsum"] = out["weights"].sum(-1)
        N = case["N"]
        if N > 0:
            pw = is_only_weights(out["weights"]) if case["form"] == "is_only" else out["weights"]
            res["z_fine"], res["z_new"], res["order"] = orc.importance_z(z, pw, N, u)
            res["cdf"] = _cdf(pw)
            res["u"] = torch.linspace(0., 1., steps=N).expand(z.shape[0], N) if u is None else u
    return {k: v.numpy() for k, v in res.items()}


def gather_merged(raw, raw_new, order, N):
    """raw of the merged samples: cat([coarse, the N new]) taken by `order` (raycasters.py:466-469); torch or numpy"""
    if isinstance(raw, np.ndarray):
        return np.take_along_axis(np.concatenate([raw, raw_new[:, :N]], 1), order[..., None].astype(np.int64), 1)
    return torch.gather(torch.cat([raw, raw_new[:, :N]], 1), 1, order[..., None].expand(-1, -1, 4))


def reference_merged(case, dtype=torch.float64):
    with default_dtype(dtype):
        rays, zf, raw, raw_new, noise = (_t(case[k], dtype) for k in ("rays", "z_fine", "raw", "raw_new", "noise1"))
        raw_m = gather_merged(raw, raw_new, torch.tensor(case["order"].astype(np.int64)), case["N"])
        out = orc.composite(raw_m, zf, rays[:, 3:6], oracle_config(case["density"]), noise)
    return {**{k: out[k].numpy() for k in _MAPS}, "wsum": out["weights"].sum(-1).numpy(), "raw_out": raw_m.numpy()}


def _loss(out, cot, dtype, rgb="d_rgb", acc="d_acc"):
    zero = torch.zeros((), dtype=dtype)
    return ((out["rgb_map"] * _t(cot[rgb], dtype)).sum() if rgb in cot else zero) + ((out["acc_map"] * _t(cot[acc], dtype)).sum() if acc in cot else zero)


def reference_bwd(case, cot, dtype=torch.float64):
    """d_raw [n,S,4] of one composite: autograd of sum(d_rgb rgb_map) + sum(d_acc acc_map) through the oracle's composite"""
    with default_dtype(dtype):
        rays, z, noise = (_t(case[k], dtype) for k in ("rays", "z", "noise"))
        raw = _t(case["raw"], dtype, grad=True)
        out = orc.composite(raw, z, rays[:, 3:6], oracle_config(case["density"]), noise)
        loss = _loss(out, cot, dtype)
        if not loss.requires_grad:
            return np.zeros(case["raw"].shape)
        loss.backward()
    return raw.grad.numpy()


def merged_rows(case):
    """the single-net tape's raw [n S + n N, 4] of a class B case: the coarse rows ray-major, then every ray's N new rows"""
    N = case["N"]
    return f32(np.concatenate([case["raw"].reshape(-1, 4), case["raw_new"][:, :N].reshape(-1, 4)], 0))


def reference_merged_bwd(case, cot, dtype=torch.float64):
    """d_raw [n S + n N, 4]: autograd through both composites of the single-net pair and the gather by `order`"""
    n, S, N = case["rays"].shape[0], case["S"], case["N"]
    with default_dtype(dtype):
        rays, z, zf, n0, n1 = (_t(case[k], dtype) for k in ("rays", "z", "z_fine", "noise0", "noise1"))
        rows = _t(merged_rows(case), dtype, grad=True)
        raw_c, raw_n = rows[:n * S].view(n, S, 4), rows[n * S:].view(n, N, 4)
        cfg = oracle_config(case["density"])
        out_c = orc.composite(raw_c, z, rays[:, 3:6], cfg, n0)
        out_f = orc.composite(gather_merged(raw_c, raw_n, torch.tensor(case["order"].astype(np.int64)), N), zf, rays[:, 3:6], cfg, n1)
        loss = _loss(out_f, cot, dtype) + _loss(out_c, cot, dtype, "d_rgb0", "d_acc0")
        if not loss.requires_grad:
            return np.zeros((n * (S + N), 4))
        loss.backward()
    return rows.grad.numpy()


def reference_sample_coarse(case, S, lindisp, t_rand, dtype=torch.float64):
    """near_far [n,2] and z [n,S] of the oracle, one nanmean group per `chunk` rays (as test_stage_sample_coarse_chunk_groups
    slices it)"""
    n, chunk = case["rays"].shape[0], case["chunk"]
    with default_dtype(dtype), warnings.catch_warnings():
        warnings.simplefilter("ignore", RuntimeWarning)         # np.nanmean of a group without a hit
        rb = _t(case["rays"], dtype)
        cyl = _t(case["cyls"], dtype).expand(n, -1)
        tr = None if t_rand is None else _t(t_rand[:, :S], dtype)
        nf, zs = [], []
        for i in range(0, n, chunk):
            s = slice(i, i + chunk)
            near, far = orc.near_far_in_cylinder(rb[s, 0:3], rb[s, 3:6], cyl[s], rb[s, 6:7].clone(), rb[s, 7:8].clone())
            nf.append(torch.cat([near, far], -1))
            zs.append(orc.coarse_z(near, far, S, lindisp, None if tr is None else tr[s]))
    return torch.cat(nf).numpy(), torch.cat(zs).numpy()


# ---- bounds ---------------------------------------------------------------------------------------------------------------------
def bound(ref32, ref64):
    """4 x max |float32 oracle - float64 oracle| over the output, at least 4 float32 ulps of its largest magnitude"""
    ref64 = np.asarray(ref64, dtype=np.float64)
    dev = float(np.max(np.abs(np.asarray(ref32, dtype=np.float64) - ref64))) if ref64.size else 0.0
    top = float(np.max(np.abs(ref64))) if ref64.size else 0.0
    return max(4.0 * dev, 4.0 * float(np.spacing(np.float32(top))))


def deviation(got, ref64):
    return float(np.max(np.abs(np.asarray(got, dtype=np.float64) - np.asarray(ref64, dtype=np.float64)))) if np.size(ref64) else 0.0
