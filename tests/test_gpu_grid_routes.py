"""The density grid (pg_grid_density) on both sides of every change of route, up to the production row length R = res + 1 = 256 and
the first one past it, and extract_mesh end to end at res = 255.  Fixtures, oracle and tolerances are those of tests/test_gpu_mesh.py.

A grid row runs as a ray through the form pick_form chooses for rays of R samples, if R reaches that form's minimum of samples per
ray and is at most 256; as explicit points otherwise.  ROUTES below is read off the sources; a change there must change it here.
Observed per call: the launches and points of the fused kernel (one launch per slab, R^3 points) and the launches of the per-ray
record kernel (one per slab on the record route, none elsewhere) -- the counters tests/test_gpu_eval_points.py reads.
"""
import math

import numpy as np
import pytest
import torch

from posegen_amd import PREC_BF16, PREC_FP16, PREC_FP16C, PREC_FP32, PREC_NAMES
from tests import mesh_ref as mr
from tests.test_gpu_mesh import DEV, PRECS, TOL, _lattice_points, _oracle_density, _threshold, caster, golden, renderer  # noqa: F401

pytestmark = pytest.mark.gpu

# precision -> [(first R of the route, route)], from posegen_amd/csrc:
#   rays at all       pg_api.hip:1336   ray_form = R >= FORMS[form].points_per_pass() / (MAXR - 1) && R <= 256;  MAXR = 9 (pg_layout.h:104)
#     kmajor          pg_eval32.hip:22  PTS_B = 4 x 32 = 128 points per pass -> R >= 16      (fp32; fp16c below evalc2's minimum)
#     direct16        pg_eval16_common.h:16  PTS = 8 x 32 = 256 -> R >= 32                    (the 16-bit form below FACT_MIN_S)
#     evalc2          pg_program.h:125  PTS = 128 -> 16, but pick_form takes it from pgp::T::MIN_S = 32 on (pg_program.h:128, pg_api.hip:227)
#   onchip            pg_api.hip:217    c.S >= FACT_MIN_S = 64 (pg_layout.h:119)
#   records           pg_api.hip:218    c.S <= ONCHIP_MAX_S = 112 stays on chip (pg_api.hip:209), 113 is the first with records
#   points again      pg_api.hip:1336   R <= 256
_SIXTEEN = [(1, "points"), (32, "direct16"), (64, "onchip"), (113, "records"), (257, "points")]
ROUTES = {
    PREC_FP32: [(1, "points"), (16, "kmajor"), (257, "points")],
    PREC_FP16: _SIXTEEN,
    PREC_BF16: _SIXTEEN,
    PREC_FP16C: [(1, "points"), (16, "kmajor"), (32, "evalc2"), (257, "points")],
}
RADIUS = 0.9
N_SAMPLED = 4096


def route_of(prec, R):
    return [name for first, name in ROUTES[prec] if R >= first][-1]


def slab_rows(R, slab_rays=0):
    """rows per launch as pg_grid_density sizes them (pg_api.hip:1338-1344): 256 MiB of raw by default, a multiple of
    256 / gcd(R, 256) rows so that every slab starts on a pass boundary, at most all R R rows"""
    slab = slab_rays if slab_rays > 0 else max(1, (256 << 20) // (16 * R))
    align = 256 // math.gcd(R, 256)
    return min(max(align, slab // align * align), R * R)


CASES = sorted({(prec, R) for prec in PRECS for first, _ in ROUTES[prec][1:] for R in (first - 1, first)})
ORACLE = {}         # R -> (idx [n,3], points [n,3], oracle density [n]): one CPU evaluation per row length, shared by the precisions


def _sample(golden, R):
    """4096 random lattice points, the eight corners, the first and last row of the grid and of every slab (at R = 257 the two rows
    on either side of the slab boundary)"""
    if R not in ORACLE:
        idx = [torch.randint(0, R, (N_SAMPLED, 3), generator=torch.Generator().manual_seed(3))]
        idx.append(torch.cartesian_prod(*[torch.tensor([0, R - 1])] * 3))
        slab = slab_rows(R)
        rows = {0, R * R - 1}
        for r0 in range(0, R * R, slab):
            rows |= {r0, min(r0 + slab, R * R) - 1}
        for row in sorted(rows):
            iz = torch.arange(R)
            idx.append(torch.stack([torch.full_like(iz, row // R), torch.full_like(iz, row % R), iz], -1))
        idx = torch.cat(idx)
        pts, _ = _lattice_points(golden[2], RADIUS, R - 1, idx)
        ORACLE[R] = (idx, pts, _oracle_density(golden, pts))
    return ORACLE[R]


def _counted_grid(renderer, kps, skts, R, **kw):
    renderer.profile_enable(True)
    try:
        renderer.profile_read(); renderer.profile_read_aux()
        grid = renderer.grid_density(kps, skts, radius=RADIUS, res=R - 1, **kw)
        torch.cuda.synchronize()
        launches, _, n_pts = renderer.profile_read()
        recs, _ = renderer.profile_read_aux()
    finally:
        renderer.profile_enable(False)
    return grid, launches, recs, n_pts


def test_route_table_covers_the_production_size():
    assert slab_rows(256) == 256 * 256 and slab_rows(257) == 65280 and 257 * 257 - 65280 == 769      # one slab; two, the second ragged
    assert 256 // math.gcd(256, 256) == 1 and slab_rows(113, 1) == 256 and slab_rows(65, 1000) == 768
    assert [route_of(p, 256) for p in PRECS] == ["kmajor", "records", "records", "evalc2"]
    assert {route_of(p, 257) for p in PRECS} == {"points"}
    assert len(CASES) == 4 + 8 + 8 + 6


@pytest.mark.parametrize("prec,R", CASES, ids=[f"{PREC_NAMES[p]}-R{R}" for p, R in CASES])
def test_grid_density_at_route_change(renderer, golden, prec, R):
    g, cfg, kps, skts = golden
    idx, pts, ref = _sample(golden, R)
    renderer.set_precision(prec)
    grid, launches, recs, n_pts = _counted_grid(renderer, kps, skts, R)
    route = route_of(prec, R)
    slabs = -(-R * R // slab_rows(R))
    assert grid.shape == (R, R, R) and bool(torch.isfinite(grid).all())
    assert (launches, n_pts) == (slabs, R ** 3) and recs == (slabs if route == "records" else 0), (route, launches, recs, n_pts)
    i = idx.to(DEV)
    got = grid[i[:, 0], i[:, 1], i[:, 2]]
    scale = float(np.abs(ref).max())
    bound = TOL[prec] * max(1.0, scale / 10)
    d = float(np.abs(got.cpu().numpy().astype(np.float64) - ref).max())
    print(f"[{PREC_NAMES[prec]}] R {R} ({route}, {slabs} slab(s)): maxdiff / bound at {len(idx)} points {d / bound:.3f} "
          f"({d:.3e}, |sigma_raw| max {scale:.1f}, bound {bound:.3e})")
    assert d <= bound
    if R >= 256:        # the same points as explicit points of one query: a transposed or shifted axis would show here
        q = renderer.query_density(pts, skts).reshape(-1)
        dq = float((q - got).abs().max())
        print(f"[{PREC_NAMES[prec]}] R {R}: maxdiff / bound vs query_density {dq / bound:.3f}")
        assert dq <= 2 * bound


@pytest.mark.parametrize("R", [113, 256])
@pytest.mark.parametrize("prec", [PREC_BF16, PREC_FP16C], ids=["bf16", "fp16c"])
def test_grid_density_slabs_are_bitwise_at(renderer, golden, prec, R):
    """R = 113: odd, every slab a multiple of 256 rows; R = 256: a row is a pass, slabs of any number of rows, one included"""
    g, cfg, kps, skts = golden
    renderer.set_precision(prec)
    whole = renderer.grid_density(kps, skts, radius=RADIUS, res=R - 1)
    for rays in (R * R, 1000):
        part, launches, recs, n_pts = _counted_grid(renderer, kps, skts, R, slab_rays=rays)
        assert launches == -(-R * R // slab_rows(R, rays)) and n_pts == R ** 3
        assert torch.equal(whole, part), rays
    # (slabs of one row at R = 256 are 65536 launches: not counted, the counters keep a pair of events per launch)
    assert torch.equal(whole, renderer.grid_density(kps, skts, radius=RADIUS, res=R - 1, slab_rays=1))


def test_extract_mesh_at_production_size(caster, golden):
    g, cfg, kps, skts = golden
    res = 255
    caster.renderer.set_precision(PREC_FP32)
    grid = caster.renderer.grid_density(kps, skts, radius=RADIUS, res=res)
    thr = _threshold(grid)
    v, t = caster.extract_mesh(kps, skts, None, radius=RADIUS, res=res, threshold=thr)
    v, t, grid = v.cpu().numpy(), t.cpu().numpy(), grid.cpu().numpy()
    rv, rt = mr.marching_cubes_ref(grid, thr, clamp=0.0)
    assert len(rt) > 10000 and np.array_equal(t, rt) and np.allclose(v, rv / res - .5, rtol=0, atol=1e-6)
    assert len(v) == mr.sign_change_edges(grid, thr, clamp=0.0)
    open_, uniq = mr.open_edges(t)
    assert uniq and bool((np.abs(v) == .5).any(1)[open_].all())
