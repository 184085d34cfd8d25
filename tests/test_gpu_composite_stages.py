"""The sampling and compositing kernels of pg_kernels.hip (sample_coarse_kernel and its two-launch form, composite_kernel in its
plain, is_only and merged forms) and their transposes in pg_train.hip (composite_bwd_kernel, merged_composite_bwd_kernel) through
their stage entry points, against the oracle in float64 at the kernel's own float32 inputs (tests/composite_ref.py; the
yardstick itself is pinned by tests/test_composite_ref_host.py).

Classes: A smooth cases, every output value by value; B the merged form; C exact edges (empty and opaque rays, ties, unsorted
draws, a NaN ray, more rays than waves, the disparity switch); D coarse sampling over nanmean groups; E the two backward kernels.
Every bound of A, B, D and E is computed per case: 4 x max |float32 oracle - float64 oracle| over the output, at least 4 float32
ulps of its largest magnitude (composite_ref.bound).  Each comparison prints the device's deviation and the bound.

Worst device deviation / bound per class, measured on an MI355X (gfx950) on the kernels as they are here, all 1131 comparisons:

    class  worst ratio  output, case
    A      0.83   z_fine / z_new, S64-N16-plain-det-softplus (3.6e-06 against 4.3e-06); rgb_map 0.40, disp_map 0.40, weights 0.26,
                  alpha 0.13, acc_map 0.12 (one ulp below 1 against 4)
    B      0.28   disp_map, S33-N7-noise-relu; rgb_map 0.27, alpha 0.13, acc_map 0.12
    C      0.31   rgb_map of the 65541-ray case; z_new 0.29 (everything else of class C is exact)
    D      0.38   z, chunk300-cyl5-S2-lindisp-draws, in both launch forms; near_far 0.34
    E      0.30   d_raw, merged S65-N16-relu, all four cotangents

With the transmittance scan, the cdf scan and expf in float32, as these kernels were before this change, 20 of the 133 tests missed
their bounds, all at S >= 129 and by up to 1.9 x (acc_map 8.3e-07 against 4.8e-07 at S192-N64, d_raw 7.4e-07 against 3.9e-07 at
S129-N64): sum w strayed up to 7 ulp from 1 and the far samples' weights by ~1e-6 relative.  composite_kernel, composite_bwd_kernel
and merged_composite_bwd_kernel now carry the running transmittance, the cdf sum and sum w in double and take exp in double (alpha
and the factor 1 - alpha + 1e-10 from the one value); inputs and outputs stay float32.  Cost on the benchmark frame, alternating
runs on one MI355X: 30.352 ms against 30.171 ms per frame with the float32 arithmetic, 0.6 % slower.
"""
import ctypes as C

import numpy as np
import pytest
import torch

from posegen_amd import PREC_FP32, _ffi
from tests import composite_ref as cr

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
F64, F32 = torch.float64, torch.float32
SENTINEL = -777.0
WORST = {}


def T(a):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a))


def host(o):
    torch.cuda.synchronize()
    return {k: v.cpu().numpy() for k, v in o.items()} if isinstance(o, dict) else o.cpu().numpy()


@pytest.fixture(scope="module")
def renderers():
    """one handle per density activation; no weights are needed by any stage of this file"""
    from posegen_amd.raycaster import HipRenderer
    rs = {d: HipRenderer(cr.render_cfg(d), device=DEV, precision=PREC_FP32) for d in cr.DENSITIES}
    yield rs
    for r in rs.values():
        r.close()
    for cls in sorted(WORST):
        print(f"[class {cls}] worst device deviation / bound: {WORST[cls][0]:.3f} ({WORST[cls][1]})")


def hold(cls, label, got, r32, r64):
    """the kernel against the float64 oracle with the case's own bound: printed, then asserted"""
    dev, b = cr.deviation(got, r64), cr.bound(r32, r64)
    print(f"[{cls}] {label}: device {dev:.2e} bound {b:.2e} ratio {dev / b:.2f}")
    if dev / b > WORST.get(cls, (0.0, ""))[0]:
        WORST[cls] = (dev / b, label)
    assert np.isfinite(np.asarray(got)).all(), label
    assert dev <= b, f"{label}: device {dev:.2e} beyond 4 x the float32 oracle's own deviation, {b:.2e}"


def forward(r, c, ld_new=None, fill=None):
    return host(r.stage_composite_form(c["form"], T(c["rays"]), T(c["z"]), T(c["raw"]), c["N"], T(c["noise"]), T(c["u_rand"]),
                                       ld_new=ld_new, fill=fill))


def merged(r, b, order=None, fill=None):
    return host(r.stage_composite_merged(T(b["rays"]), T(b["z_fine"]), T(b["raw"]), T(b["raw_new"]), T(b["order"] if order is None else order),
                                         T(b["noise1"]), fill=fill))


def new_depths(o, S):
    """the new entries of z_fine in sample order: z_fine at the positions whose source index is S + k"""
    pos = np.argsort(o["order"], -1, kind="stable")[:, S:]
    return np.take_along_axis(o["z_fine"], pos, -1)


# ---- class A --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", cr.class_a_cases(), ids=cr.case_id)
def test_smooth_cases_value_by_value(renderers, case):
    """every output of a class A case value by value, order exactly; is_only also the ld_new padding"""
    S, N, form, draws, density = case
    c = cr.make_case_a(*case)
    r64, r32 = cr.reference(c, F64), cr.reference(c, F32)
    o = forward(renderers[density], c, fill=SENTINEL)
    tag = cr.case_id(case)
    for k in ("rgb_map", "disp_map", "acc_map", "alpha", "weights"):
        hold("A", f"{tag} {k}", o[k], r32[k], r64[k])
    if N == 0:
        return
    assert np.array_equal(o["order"], r64["order"]), "under the class conditions the sort order is the reference's"
    hold("A", f"{tag} z_fine", o["z_fine"], r32["z_fine"], r64["z_fine"])
    hold("A", f"{tag} z_new", new_depths(o, S), r32["z_new"], r64["z_new"])
    if form == "is_only":
        assert np.array_equal(o["z_new"], new_depths(o, S)), "z_new holds the new entries of z_fine"
        if N < 32:
            p = forward(renderers[density], c, ld_new=32, fill=SENTINEL)
            assert np.array_equal(p["z_new"][:, :N], o["z_new"]) and np.all(p["z_new"][:, N:] == p["z_new"][:, N - 1:N])
            assert all(np.array_equal(p[k], o[k]) for k in o if k != "z_new")


# ---- class B --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("density", cr.DENSITIES)
@pytest.mark.parametrize("with_noise", [False, True])
@pytest.mark.parametrize("S,N", [(33, 7), (65, 16), (129, 64), (192, 64)])
def test_merged_form(renderers, S, N, with_noise, density):
    """the merged form on the reference's z_fine / order and a raw_new of row length N + 3; then the two device stages chained,
    is_only then merged by the device's own order, bitwise the run on the reference's order"""
    r = renderers[density]
    b = cr.make_case_b(S, N, density, with_noise, ld_new=N + 3)
    r64, r32 = cr.reference_merged(b, F64), cr.reference_merged(b, F32)
    o = merged(r, b, fill=SENTINEL)
    tag = f"S{S}-N{N}-{'noise' if with_noise else 'det'}-{density}"
    for k in ("rgb_map", "disp_map", "acc_map", "alpha"):
        hold("B", f"{tag} {k}", o[k], r32[k], r64[k])
    assert np.array_equal(o["raw_out"], cr.gather_merged(b["raw"], b["raw_new"], b["order"], N))
    first = forward(r, b["a"], ld_new=N + 3)
    assert np.array_equal(first["order"], b["order"])
    chained = merged(r, b, order=first["order"])
    assert all(np.array_equal(chained[k], o[k]) for k in o)


# ---- class C --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("form", cr.FORMS)
def test_empty_rays(renderers, form):
    c = cr.make_case_empty(64, 16, form)
    o = forward(renderers["relu"], c, fill=SENTINEL)
    for k in ("rgb_map", "acc_map", "disp_map", "weights", "alpha"):
        assert np.all(o[k] == 0), k
    r64, r32 = cr.reference(c, F64), cr.reference(c, F32)
    assert np.array_equal(o["order"], r64["order"])
    hold("C", f"empty {form} z_new", new_depths(o, 64), r32["z_new"], r64["z_new"])


@pytest.mark.parametrize("S,N", [(64, 16), (129, 64)])
def test_opaque_last_interior_sample(renderers, S, N):
    c = cr.make_case_opaque_last(S, N)
    o = forward(renderers["relu"], c, fill=SENTINEL)
    r64, r32 = cr.reference(c, F64), cr.reference(c, F32)
    assert np.all(o["weights"][:, S - 2] == 1.0) and np.all(np.delete(o["weights"], S - 2, axis=1) == 0)
    assert np.all(o["acc_map"] == 1.0)
    assert np.array_equal(o["order"], r64["order"])
    hold("C", f"opaque S{S} z_new", new_depths(o, S), r32["z_new"], r64["z_new"])
    hold("C", f"opaque S{S} rgb_map", o["rgb_map"], r32["rgb_map"], r64["rgb_map"])


@pytest.mark.parametrize("form", cr.FORMS)
@pytest.mark.parametrize("S,N", [(65, 16), (129, 64)])
def test_ties_sort_stably_on_both_ranking_paths(renderers, S, N, form):
    """equal depths (near = far), depths repeating in pairs, repeated draws: z_fine is sorted, a permutation of cat(z, the device's
    own z_new), and order is the stable argsort of that concatenation -- with the draws in random order (the all-pairs count) and
    sorted (the two binary searches)"""
    for sorted_u in (False, True):
        c = cr.make_case_ties(S, N, form, sorted_u)
        o = forward(renderers["relu"], c, fill=SENTINEL)
        z_new = o["z_new"] if form == "is_only" else new_depths(o, S)
        cat = np.concatenate([c["z"], z_new], -1)
        want = np.argsort(cat, -1, kind="stable")
        assert np.array_equal(o["order"], want), sorted_u
        assert np.array_equal(o["z_fine"], np.take_along_axis(cat, want, -1))
        assert np.all(np.diff(o["z_fine"], axis=-1) >= 0)
        assert np.all(o["order"][cr.TIE_RAYS["flat"]] == np.arange(S + N)[None, :])


@pytest.mark.parametrize("form", cr.FORMS)
def test_unsorted_draws_equal_sorted_draws(renderers, form):
    c = cr.make_case_a(65, 16, form, True, "relu")
    s = dict(c, u_rand=np.sort(c["u_rand"], -1))
    a, b = forward(renderers["relu"], c), forward(renderers["relu"], s)
    assert np.any(np.diff(c["u_rand"], axis=-1) < 0)
    assert np.array_equal(a["z_fine"], b["z_fine"])
    assert all(np.array_equal(a[k], b[k]) for k in ("rgb_map", "weights"))


@pytest.mark.parametrize("form", cr.FORMS)
def test_a_nan_ray_leaves_the_others_alone(renderers, form):
    """one ray with NaN depths among 69 finite ones, outputs prefilled: the call succeeds and the finite rays are bitwise those of
    the call without it; the NaN ray's own maps are NaN where the float64 oracle's are (every one: not acc = 1, disp = 1e10 beside a
    NaN colour, which is what fminf / fmaxf make of NaN sums); then the merged form on the same rays"""
    r = renderers["relu"]
    c, without, keep = cr.make_case_nan_ray(65, 16, form)
    a, b = forward(r, c, fill=SENTINEL), forward(r, without, fill=SENTINEL)
    for k in b:
        assert np.array_equal(a[k][keep], b[k]), k
        assert not np.any(b[k] == SENTINEL), k
    nan_ray = {k: (v[~keep] if isinstance(v, np.ndarray) else v) for k, v in c.items()}
    want = cr.reference({**nan_ray, "N": 0, "u_rand": None}, F64)           # the composite alone: the maps do not depend on the new depths
    for k in ("rgb_map", "disp_map", "acc_map"):
        print(f"[C] NaN ray {form} {k}: device {a[k][~keep].reshape(-1)}, float64 oracle {want[k].reshape(-1)}")
        assert np.isnan(want[k]).all(), k
        assert np.array_equal(np.isnan(a[k][~keep]), np.isnan(want[k])), k
    raw_new = cr.f32(np.random.default_rng(9).normal(0, 1, (cr.N_RAYS, 16, 4)))
    m = {"rays": c["rays"], "z_fine": a["z_fine"], "raw": c["raw"], "raw_new": raw_new, "order": a["order"], "noise1": None}
    mw = {k: (v[keep] if v is not None else None) for k, v in m.items()}
    ma, mb = merged(r, m, fill=SENTINEL), merged(r, mw, fill=SENTINEL)
    for k in mb:
        assert np.array_equal(ma[k][keep], mb[k]), k


def test_more_rays_than_waves(renderers):
    """65536 + 5 rays: the 16384 workgroups' waves take a second ray and reuse their LDS rows; rays 65536.. are bitwise the same
    rays run as a call of 5"""
    c = cr.make_case_many_rays()
    tail = {k: (v[65536:] if isinstance(v, np.ndarray) else v) for k, v in c.items()}
    a, b = forward(renderers["relu"], c, fill=SENTINEL), forward(renderers["relu"], tail, fill=SENTINEL)
    for k in b:
        assert np.array_equal(a[k][65536:], b[k]), k
        assert not np.any(a[k] == SENTINEL), k
    r64, r32 = cr.reference(tail, F64), cr.reference(tail, F32)
    hold("C", "many rays rgb_map", b["rgb_map"], r32["rgb_map"], r64["rgb_map"])


def test_disparity_switch(renderers):
    """sum w = 1e-9: disp is exactly 0 (|sum w| <= 1e-8; float32 gives alpha = 0 outright).  sum w = 1e-7: the switch stays open and
    disp = (sum w + 1e-10) / (w z_k) lies between 1 / z_k and (1 + 1e-10 / w) / z_k for any float32 w >= 2^-24 of the one live
    sample k, i.e. within 1.7e-3 above 1 / z_k."""
    c = cr.make_case_disp()
    o = forward(renderers["relu"], c)
    r64 = cr.reference(c, F64)
    even = np.arange(cr.N_RAYS) % 2 == 0
    assert np.all(o["disp_map"][~even] == 0) and np.all(r64["disp_map"][~even] == 0)
    inv = 1.0 / c["z"][np.arange(cr.N_RAYS), c["live"]].astype(np.float64)
    d = o["disp_map"].astype(np.float64)
    print(f"[C] disp at sum w = 1e-7: device / (1 / z_k) - 1 in [{(d / inv - 1)[even].min():.2e}, {(d / inv - 1)[even].max():.2e}]")
    assert np.all(d[even] >= inv[even] * (1 - 1e-6)) and np.all(d[even] <= inv[even] * (1 + 2e-3))
    assert np.all(np.abs(r64["disp_map"][even] / inv[even] - 1) <= 2e-3)


# ---- class D --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("per_ray_cyl", [False, True])
@pytest.mark.parametrize("chunk", cr.SC_CHUNKS)
def test_coarse_sampling_over_nanmean_groups(renderers, chunk, per_ray_cyl):
    r = renderers["relu"]
    c = cr.make_case_d(chunk, per_ray_cyl)
    rays, cyls = T(c["rays"]), T(c["cyls"])
    r.set_chunk(chunk)
    try:
        for S in cr.SC_SAMPLES:
            for lindisp in (False, True):
                for t_rand in (None, c["t_rand"][:, :S].copy()):
                    tag = f"chunk{chunk}-cyl{5 if per_ray_cyl else 0}-S{S}-{'lindisp' if lindisp else 'lin'}-{'draws' if t_rand is not None else 'det'}"
                    (nf64, z64), (nf32, z32) = (cr.reference_sample_coarse(c, S, lindisp, t_rand, dt) for dt in (F64, F32))
                    nf, z = (host(t) for t in r.stage_sample_coarse_draws(rays, cyls, S, lindisp, T(t_rand)))
                    hold("D", f"{tag} near_far", nf, nf32, nf64)
                    hold("D", f"{tag} z", z, z32, z64)
                    if t_rand is None:      # the entry point without draws is the same launch
                        nf0, z0 = (host(t) for t in r.stage_sample_coarse(rays, cyls, S, lindisp))
                        assert np.array_equal(nf0, nf) and np.array_equal(z0, z)
                    if chunk > 256:         # the stage ran the two-launch form: the one-launch form on the same groups
                        nf1, z1 = (host(t) for t in r.stage_sample_coarse_draws(rays, cyls, S, lindisp, T(t_rand), one_launch=True))
                        hold("D", f"{tag} z (one launch)", z1, z32, z64)
                        hit = c["hit"]
                        assert np.array_equal(nf1[hit], nf[hit]), "rays that hit are not patched, in either form"
                        assert np.isfinite(nf1[~hit]).all() and np.isfinite(nf[~hit]).all(), "every miss is patched, in both forms"
                        own, own1 = ((a == c["rays"][:, 6:8]).all(-1) for a in (nf, nf1))     # patched with the ray's own near / far
                        group = np.arange(cr.SC_RAYS) // chunk
                        assert np.array_equal(own, own1) and np.array_equal(own, (group == 1) & (cr.SC_RAYS > chunk))
    finally:
        r.set_chunk(r.cfg.chunk)


# ---- class E --------------------------------------------------------------------------------------------------------------------
def _bwd(r, c, cot):
    return host(r.stage_composite_bwd(T(c["rays"]), T(c["z"]), T(c["raw"]), T(c["noise"]), T(cot.get("d_rgb")), T(cot.get("d_acc"))))


@pytest.mark.parametrize("density", cr.DENSITIES)
@pytest.mark.parametrize("S,N", cr.BWD_SHAPES)
def test_composite_backward(renderers, S, N, density):
    """d_raw of one composite against float64 autograd for d_rgb alone, d_acc alone and both; d_acc is 0 on the rays at sum w ~ 1
    (which stay in the comparison); no cotangent gives exactly zero; dead relu samples get d_raw.w == 0"""
    r = renderers[density]
    c = cr.make_case_e(S, N, density)
    wsum = cr.reference(c, F64)["wsum"]
    for which in (("d_rgb",), ("d_acc",), ("d_rgb", "d_acc")):
        cot = cr.cotangents(c, which)
        if "d_acc" in cot:
            cot["d_acc"] = cr.gate_acc(cot["d_acc"], wsum)
        g = _bwd(r, c, cot)
        g64, g32 = cr.reference_bwd(c, cot, F64), cr.reference_bwd(c, cot, F32)
        hold("E", f"S{S}-{density} {'+'.join(which)} d_raw", g, g32, g64)
        if density == "relu":
            dead = c["raw"][..., 3] / cr.DENSITY_SCALE + c["noise"] < 0
            assert dead.any() and np.all(g[..., 3][dead] == 0)
    assert np.all(_bwd(r, c, {}) == 0)


def test_composite_backward_at_opaque_samples(renderers):
    """a fully opaque sample (a = 1: suffix / (1 - a + 1e-10)) anywhere on the ray and the last sample (delta = 1e10): finite rows,
    within the bound of float64 autograd under d_rgb.  On the rays whose FIRST sample is the opaque one, d_acc alone gives exactly
    zero: w_0 = 1.0f and every other w >= 0, so sum w is 1 + O(1e-10) > 1 in exact arithmetic and 1.0f on the device whatever the
    order of the sum, and min(sum w, 1) is constant around the ray -- the `sum w < 1` gate, where no rounding can open it."""
    r = renderers["relu"]
    c = cr.make_case_opaque_bwd()
    cot = cr.cotangents(c, ("d_rgb",))
    g = _bwd(r, c, cot)
    assert np.isfinite(g).all()
    hold("E", "opaque d_rgb d_raw", g, cr.reference_bwd(c, cot, F32), cr.reference_bwd(c, cot, F64))
    only_acc = {"d_acc": np.ones(cr.N_RAYS, np.float32)}
    first = c["first"]
    assert first.sum() >= cr.N_RAYS // 4
    ga = _bwd(r, c, only_acc)
    assert np.isfinite(ga).all()
    assert np.all(cr.reference_bwd(c, only_acc, F64)[first] == 0)
    assert np.all(ga[first] == 0)


@pytest.mark.parametrize("density", cr.DENSITIES)
@pytest.mark.parametrize("S,N", [(33, 7), (65, 16), (129, 64)])
def test_merged_composite_backward(renderers, S, N, density):
    """d_raw of the single-net pair against float64 autograd through the gather by `order`: each of the four cotangents alone, all
    together, none (exactly zero); the call repeated gives the same bytes"""
    r = renderers[density]
    b = cr.make_case_b_bwd(S, N, density)
    wf, wc = cr.reference_merged(b, F64)["wsum"], cr.reference(cr.coarse_of(b), F64)["wsum"]
    rows = cr.merged_rows(b)
    run = lambda cot: host(r.stage_merged_composite_bwd(T(b["rays"]), T(b["z"]), T(b["z_fine"]), T(rows), T(b["order"]), T(b["noise0"]),
                                                        T(b["noise1"]), *[T(cot.get(k)) for k in ("d_rgb", "d_acc", "d_rgb0", "d_acc0")]))
    names = ("d_rgb", "d_acc", "d_rgb0", "d_acc0")
    for which in [(k,) for k in names] + [names]:
        cot = cr.cotangents(b, which, fine=True)
        if "d_acc" in cot:
            cot["d_acc"] = cr.gate_acc(cot["d_acc"], wf)
        if "d_acc0" in cot:
            cot["d_acc0"] = cr.gate_acc(cot["d_acc0"], wc)
        g = run(cot)
        hold("E", f"merged S{S}-N{N}-{density} {'+'.join(which)} d_raw", g, cr.reference_merged_bwd(b, cot, F32), cr.reference_merged_bwd(b, cot, F64))
        if len(which) == 4:
            assert np.array_equal(run(cot), g), "the fine and the coarse share are added in a fixed order"
    assert np.all(run({}) == 0)


def test_merged_backward_without_importance_samples(renderers):
    """N = 0: the one composite is passed as the coarse one"""
    r = renderers["relu"]
    c = cr.make_case_e(65, 0, "relu")
    cot = cr.cotangents(c, ("d_rgb", "d_acc"))
    cot["d_acc"] = cr.gate_acc(cot["d_acc"], cr.reference(c, F64)["wsum"])
    g = host(r.stage_merged_composite_bwd(T(c["rays"]), T(c["z"]), T(c["z"]), T(c["raw"].reshape(-1, 4)), T(np.zeros((cr.N_RAYS, 65), np.int32)),
                                          T(c["noise"]), None, None, None, T(cot["d_rgb"]), T(cot["d_acc"])))
    hold("E", "merged N=0 d_raw", g.reshape(c["raw"].shape), cr.reference_bwd(c, cot, F32), cr.reference_bwd(c, cot, F64))


# ---- refusals -------------------------------------------------------------------------------------------------------------------
def test_bad_arguments_are_refused_before_any_launch():
    """every rule of the new entry points (check_samples, S + N <= 256, S >= 3 with importance samples, ld_new >= N, non-null required
    pointers) is PG_EINVAL; the handle renders afterwards"""
    from posegen_amd.raycaster import HipRayCaster
    from tests.helpers import cfg_from_golden, load_golden, model_for
    g = load_golden("rays_surreal")
    cfg = cfg_from_golden(g)
    caster = HipRayCaster.from_weights(cfg, *model_for(cfg, int(g["seed_model"])), device=DEV, precision=PREC_FP32)
    r = caster.renderer
    lib, h, st = r.lib, r.handle, r._stream()
    n = 8
    buf = torch.zeros(n * 320 * 4 + 1, device=DEV)
    ibuf = torch.zeros(n * 320, device=DEV, dtype=torch.int32)
    p, ip = C.c_void_p(buf.data_ptr()), C.c_void_p(ibuf.data_ptr())
    odd = C.c_void_p(buf.data_ptr() + 4)

    def comp(form, S, N, z=p, raw=p, z_fine=p, order=ip, z_new=None, ld_new=0, raw_new=None, rays=p, n_=n):
        return lib.pg_stage_composite_form(h, st, form, n_, S, N, rays, z, raw, None, None, p, p, p, p, p, z_fine, order, z_new, ld_new,
                                           raw_new, None)

    def mbwd(S, N, z_fine=p, order=ip, raw=p, d_raw=p, z=p):
        return lib.pg_stage_merged_composite_bwd(h, st, n, S, N, p, z, z_fine, raw, None, None, order, p, p, p, p, d_raw)

    P, I, M = _ffi.PG_COMP_PLAIN, _ffi.PG_COMP_IS_ONLY, _ffi.PG_COMP_MERGED
    bad = [
        lib.pg_stage_sample_coarse_draws(h, st, -1, p, p, 0, 64, 0, None, p, p),
        lib.pg_stage_sample_coarse_draws(h, st, n, None, p, 0, 64, 0, None, p, p),
        lib.pg_stage_sample_coarse_draws(h, st, n, p, p, 0, 1, 0, None, p, p),
        lib.pg_stage_sample_coarse_draws(h, st, n, p, p, 3, 64, 0, None, p, p),
        lib.pg_stage_sample_coarse_draws(h, st, n, p, p, 0, 64, 0, None, p, None),
        comp(3, 64, 16), comp(-1, 64, 16), comp(P, 257, 0), comp(P, 1, 0), comp(P, 64, 1), comp(P, 64, 65), comp(P, 250, 16),
        comp(I, 2, 2), comp(P, 64, 16, z=None), comp(P, 64, 16, raw=None), comp(P, 64, 16, rays=None), comp(P, 64, 16, n_=-1),
        comp(P, 64, 16, z_fine=None), comp(I, 64, 16, z_fine=None), comp(I, 64, 16, z_new=p, ld_new=15),
        comp(M, 64, 16, raw_new=None, ld_new=16), comp(M, 64, 16, raw_new=p, ld_new=16, order=None), comp(M, 64, 16, raw_new=p, ld_new=15),
        comp(M, 64, 0, raw_new=p, ld_new=16), comp(M, 250, 16, raw_new=p, ld_new=16), comp(M, 2, 2, raw_new=p, ld_new=2),
        lib.pg_stage_composite_bwd(h, st, n, 257, p, p, p, None, p, p, p),
        lib.pg_stage_composite_bwd(h, st, n, 1, p, p, p, None, p, p, p),
        lib.pg_stage_composite_bwd(h, st, n, 64, p, p, p, None, p, p, None),
        lib.pg_stage_composite_bwd(h, st, n, 64, p, p, None, None, p, p, p),
        lib.pg_stage_composite_bwd(h, st, -1, 64, p, p, p, None, p, p, p),
        mbwd(250, 16), mbwd(64, 1), mbwd(64, 65), mbwd(2, 2), mbwd(1, 0), mbwd(64, 16, order=None), mbwd(64, 16, z_fine=None),
        mbwd(64, 16, raw=odd), mbwd(64, 16, d_raw=odd), mbwd(64, 16, d_raw=None), mbwd(64, 16, z=None),
    ]
    assert bad == [_ffi.PG_EINVAL] * len(bad), bad
    torch.cuda.synchronize()
    assert float(buf.abs().max()) == 0 and int(ibuf.abs().max()) == 0, "nothing was launched"
    rb, skts, cyl = torch.tensor(g["ray_batch"]), torch.tensor(g["skts"]), torch.tensor(g["cyl"])
    ok = r.render_rays(rb[:8], skts, cyl, n_samples=64, n_importance=16)
    assert torch.isfinite(ok["rgb_map"]).all()
    caster.renderer.close()
