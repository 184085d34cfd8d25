"""Mesh extraction on the GPU: marching cubes (pg_mesh_count / pg_mesh_emit) against the numpy restatement of tests/mesh_ref.py, the
density grid (pg_grid_density) against the oracle's embedding + trunk on the same lattice, and extract_mesh / render_mesh end to end.

Density bounds are those of test_query_density_on_explicit_points (tol * max(1, scale / 10)): fp32 2e-4, fp16 8e-3, bf16 5e-2;
fp16c is held to fp16's bound (it is at least as exact by construction) and its measured value printed."""
import ctypes as C

import numpy as np
import pytest
import torch

from oracle import anerf_oracle as orc
from posegen_amd import PREC_BF16, PREC_FP16, PREC_FP16C, PREC_FP32, PREC_NAMES, _ffi, mesh, synthetic as syn
from posegen_amd.config import RenderConfig, surreal_config
from tests import mesh_ref as mr
from tests.helpers import cfg_from_golden, load_golden, model_for, oracle_cfg, torch_weights

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
NINF = float("-inf")
TOL = {PREC_FP32: 2e-4, PREC_FP16: 8e-3, PREC_BF16: 5e-2, PREC_FP16C: 8e-3}
PRECS = [PREC_FP32, PREC_FP16, PREC_BF16, PREC_FP16C]


@pytest.fixture(scope="module")
def golden():
    g = load_golden("rays_surreal")
    cfg = cfg_from_golden(g)
    skts = torch.tensor(g["skts"])
    kps = torch.tensor(g["kps"]) if "kps" in g else torch.linalg.inv(skts.double())[..., :3, 3].float()
    return g, cfg, kps.reshape(-1, 24, 3), skts


@pytest.fixture(scope="module")
def caster(golden):
    from posegen_amd.raycaster import HipRayCaster
    g, cfg, kps, skts = golden
    c = HipRayCaster.from_weights(cfg, *model_for(cfg, int(g["seed_model"])), device=DEV, precision=PREC_FP32)
    yield c
    c.renderer.close()


@pytest.fixture(scope="module")
def renderer(caster):
    return caster.renderer


def _mc(renderer, grid, thr, clamp=NINF):
    v, t = renderer.marching_cubes(torch.tensor(grid), thr, clamp=clamp)
    return v.cpu().numpy(), t.cpu().numpy()


def _check_against_ref(renderer, grid, thr, clamp=NINF):
    rv, rt, v64 = mr.marching_cubes_ref(grid, thr, clamp=clamp, want64=True)
    v, t = _mc(renderer, grid, thr, clamp)
    assert v.dtype == np.float32 and t.dtype == np.int32
    assert v.shape == rv.shape and t.shape == rt.shape
    assert np.array_equal(t, rt)
    # the index part of a vertex (the integer coordinates, the edge's lower point) exactly, the position within the tolerance
    assert np.array_equal(np.floor(v), np.floor(rv), equal_nan=True)
    ok64 = np.isfinite(v64)
    assert (np.abs(v.astype(np.float64) - v64) <= mr.position_tolerance(v64))[ok64].all()
    # the kernel's tt and i + tt are the restatement's float32 operations: the same bits wherever the restatement has a number, and a
    # NaN (an edge with an end that is no number) in the same element -- of either sign, hosts differ in the NaN they generate
    fin = np.isfinite(rv)
    assert v[fin].tobytes() == rv[fin].tobytes()
    assert np.array_equal(v, rv, equal_nan=True)
    return v, t


# ---------------------------------------------------------------------------------------------- marching cubes
@pytest.mark.parametrize("name,fn,res,nv,nt,chi", mr.FIELDS, ids=[f[0] for f in mr.FIELDS])
def test_marching_cubes_on_closed_surfaces(renderer, name, fn, res, nv, nt, chi):
    grid = fn(res)
    v, t = _check_against_ref(renderer, grid, 0.0)
    assert v.shape == (nv, 3) and t.shape == (nt, 3)
    assert mr.is_closed_oriented_manifold(t) and mr.signed_volume6(v, t) > 0 and mr.euler_characteristic(nv, t) == chi
    v2, t2 = _mc(renderer, grid, 0.0)
    assert v.tobytes() == v2.tobytes() and t.tobytes() == t2.tobytes()


def test_marching_cubes_all_single_cell_patterns(renderer):
    for case in range(256):
        grid = np.zeros((2, 2, 2), np.float32)
        for c in range(8):
            grid[tuple(mesh.CORNER_OFFSETS[c])] = 1.0 if (case >> c) & 1 else -1.0
        v, t = _check_against_ref(renderer, grid, 0.0)
        assert len(v) == mr.sign_change_edges(grid, 0.0) and len(t) == mesh.N_TRI[case]


def test_marching_cubes_non_cubic_grid(renderer):
    rng = np.random.RandomState(5)
    x, y, z = np.meshgrid(np.linspace(0, 1, 17), np.linspace(0, 1, 9), np.linspace(0, 1, 5), indexing="ij")
    a = rng.uniform(-3, 3, size=(6, 4))
    grid = sum(np.sin(a[i, 0] * x + a[i, 1] * y + a[i, 2] * z + a[i, 3]) for i in range(6)).astype(np.float32)
    v, t = _check_against_ref(renderer, grid, 0.25)
    assert len(v) > 50 and len(t) > 50


def test_marching_cubes_several_scan_blocks(renderer):
    t_ = np.linspace(-1, 1, 70)
    x, y, z = np.meshgrid(t_, t_, t_, indexing="ij")
    grid = (0.7 - np.sqrt((x - .013) ** 2 + (y + .021) ** 2 + (z - .007) ** 2)).astype(np.float32)
    v, t = _check_against_ref(renderer, grid, 0.0)
    assert mr.is_closed_oriented_manifold(t) and mr.euler_characteristic(len(v), t) == 2 and mr.signed_volume6(v, t) > 0


@pytest.mark.parametrize("fill", [-1.0, 1.0])
def test_marching_cubes_without_a_crossing(renderer, fill):
    v, t = _mc(renderer, np.full((5, 4, 3), fill, np.float32), 0.0)
    assert v.shape == (0, 3) and t.shape == (0, 3)


def test_marching_cubes_clamp(renderer):
    grid = mr.sphere(12)            # threshold 0.1: the outside end of many crossing edges is below zero
    a = _check_against_ref(renderer, grid, 0.1, clamp=0.0)
    b = _check_against_ref(renderer, grid, 0.1, clamp=NINF)
    assert a[0].shape == b[0].shape and not np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])


def test_mesh_emit_refuses_other_counts(renderer):
    r = renderer
    g = torch.tensor(mr.sphere(8)).to(DEV)
    nv, nt = C.c_int64(), C.c_int64()
    args = (r.handle, r._stream(), C.c_void_p(g.data_ptr()), 9, 9, 9, 0.0, NINF)
    assert r.lib.pg_mesh_count(*args, C.byref(nv), C.byref(nt)) == _ffi.PG_OK and nv.value > 0
    v = torch.empty(nv.value + 1, 3, device=DEV)
    t = torch.empty(nt.value, 3, device=DEV, dtype=torch.int32)
    out = (C.c_void_p(v.data_ptr()), C.c_void_p(t.data_ptr()))
    assert r.lib.pg_mesh_emit(*args, *out, nv.value + 1, nt.value) == _ffi.PG_ESTATE
    assert r.lib.pg_mesh_emit(*args[:3], 9, 9, 8, 0.0, NINF, *out, nv.value, nt.value) == _ffi.PG_ESTATE
    assert r.lib.pg_mesh_emit(*args, *out, nv.value, nt.value) == _ffi.PG_OK
    assert r.lib.pg_mesh_count(r.handle, r._stream(), C.c_void_p(g.data_ptr()), 9, 9, 1, 0.0, NINF, C.byref(nv), C.byref(nt)) == _ffi.PG_EINVAL


# ---------------------------------------------------------------------------------------------- the density grid
def _oracle_density(golden, pts):
    g, cfg, kps, skts = golden
    ocfg = oracle_cfg(cfg, g["tau_v"], g["tau_d"])
    wf = torch_weights(model_for(cfg, int(g["seed_model"]))[1])
    x = orc.embed_points(pts[:, None, :], torch.zeros(pts.shape[0], 3) + torch.tensor([0., 0., 1.]), skts, ocfg)
    return orc.mlp_forward(x.reshape(pts.shape[0], -1), wf, ocfg)[:, 3].numpy()


def _lattice_points(kps, radius, res, idx=None):
    """root + (t[a], t[b], t[c]) in float32 at the grid indices idx [n,3] (all of them by default)"""
    t = torch.tensor(np.linspace(-radius, radius, res + 1).astype(np.float32))
    if idx is None:
        idx = torch.cartesian_prod(*[torch.arange(res + 1)] * 3)
    return torch.stack([t[idx[:, 0]], t[idx[:, 1]], t[idx[:, 2]]], -1) + kps[0, 0], idx


@pytest.fixture(scope="module")
def oracle_small(golden):
    pts, idx = _lattice_points(golden[2], 0.6, 8)
    return _oracle_density(golden, pts).reshape(9, 9, 9)


@pytest.fixture(scope="module")
def oracle_large(golden):
    idx = torch.randint(0, 65, (4096, 3), generator=torch.Generator().manual_seed(3))
    pts, idx = _lattice_points(golden[2], 0.9, 64, idx)
    return idx, _oracle_density(golden, pts)


@pytest.mark.parametrize("prec", PRECS, ids=[PREC_NAMES[p] for p in PRECS])
def test_grid_density_small_grid(renderer, golden, oracle_small, prec):
    """res = 8: rows of 9 points, below every form's minimum of samples per ray -> explicit points formed on the device"""
    g, cfg, kps, skts = golden
    renderer.set_precision(prec)
    grid = renderer.grid_density(kps, skts, radius=0.6, res=8)
    assert grid.shape == (9, 9, 9) and grid.is_cuda
    scale = float(np.abs(oracle_small).max())
    bound = TOL[prec] * max(1.0, scale / 10)
    d = float(np.abs(grid.cpu().numpy().astype(np.float64) - oracle_small).max())
    old = renderer.mesh_density(kps, skts, radius=0.6, res=8)
    d_old = float((grid - old).abs().max())
    print(f"[{PREC_NAMES[prec]}] res 8: maxdiff vs oracle {d:.3e}, vs mesh_density {d_old:.3e} (|sigma_raw| max {scale:.1f}, bound {bound:.3e})")
    assert d <= bound
    assert d_old <= 2 * bound          # a transposed axis would show here


@pytest.mark.parametrize("prec", PRECS, ids=[PREC_NAMES[p] for p in PRECS])
def test_grid_density_ray_form(renderer, golden, oracle_large, prec):
    """res = 64: rows of 65 samples, the first size on the 16x16x32 / evalc2 forms; 4225 rays"""
    g, cfg, kps, skts = golden
    idx, ref = oracle_large
    renderer.set_precision(prec)
    grid = renderer.grid_density(kps, skts, radius=0.9, res=64)
    assert grid.shape == (65, 65, 65) and bool(torch.isfinite(grid).all())
    got = grid.cpu().numpy()[idx[:, 0], idx[:, 1], idx[:, 2]]
    scale = float(np.abs(ref).max())
    bound = TOL[prec] * max(1.0, scale / 10)
    d = float(np.abs(got.astype(np.float64) - ref).max())
    print(f"[{PREC_NAMES[prec]}] res 64: maxdiff vs oracle at 4096 points {d:.3e} (|sigma_raw| max {scale:.1f}, bound {bound:.3e})")
    assert d <= bound


@pytest.mark.parametrize("prec", [PREC_BF16, PREC_FP16C], ids=["bf16", "fp16c"])
def test_grid_density_slabs_are_bitwise(renderer, golden, prec):
    g, cfg, kps, skts = golden
    renderer.set_precision(prec)
    one = renderer.grid_density(kps, skts, radius=0.9, res=64, slab_rays=65 * 65)
    five = renderer.grid_density(kps, skts, radius=0.9, res=64, slab_rays=1000)       # several slabs (the library rounds 1000 down to 768 rows: pass-aligned), a ragged last one
    assert torch.equal(one, five)
    assert torch.equal(one, renderer.grid_density(kps, skts, radius=0.9, res=64))


def test_grid_density_refusals(renderer, golden):
    from posegen_amd.raycaster import HipRayCaster
    g, cfg, kps, skts = golden
    for kw in (dict(res=0), dict(radius=0.0), dict(radius=float("inf")), dict(radius=float("nan")), dict(which=2)):
        with pytest.raises(_ffi.PgError) as e:
            renderer.grid_density(kps, skts, **{"radius": 0.6, "res": 8, **kw})
        assert e.value.code == _ffi.PG_EINVAL
    scfg = RenderConfig(n_samples=64, n_importance=16, single_net=True, multires_views=0)
    wc, wf, tv, td = syn.make_model(scfg, 3)
    single = HipRayCaster.from_weights(scfg, wc, None, tv, td, device=DEV, precision=PREC_FP32)
    try:
        with pytest.raises(_ffi.PgError) as e:
            single.renderer.grid_density(kps, skts, radius=0.6, res=8, which=1)
        assert e.value.code == _ffi.PG_EINVAL
        assert single.renderer.grid_density(kps, skts, radius=0.6, res=8).shape == (9, 9, 9)
    finally:
        single.renderer.close()


# ---------------------------------------------------------------------------------------------- end to end
def _threshold(grid):
    pos = grid[grid > 0]
    assert pos.numel() > 0, "the model has no positive density on this grid"
    return float(pos.median())


def test_extract_mesh(caster, golden):
    g, cfg, kps, skts = golden
    res = 32
    caster.renderer.set_precision(PREC_FP32)
    grid = caster.renderer.grid_density(kps, skts, radius=0.9, res=res)
    thr = _threshold(grid)
    v, t = caster.extract_mesh(kps, skts, None, radius=0.9, res=res, threshold=thr)
    assert v.is_cuda and t.is_cuda and v.dtype == torch.float32 and t.dtype == torch.int32
    v, t = v.cpu().numpy(), t.cpu().numpy()
    assert len(v) == mr.sign_change_edges(np.maximum(grid.cpu().numpy(), 0), thr) and len(v) > 0
    assert v.min() >= -.5 and v.max() <= .5
    open_, uniq = mr.open_edges(t)
    assert uniq
    on_boundary = (np.abs(v) == .5).any(1)
    assert on_boundary[open_].all()             # closed wherever it does not touch the grid's boundary
    rv, rt = mr.marching_cubes_ref(grid.cpu().numpy(), thr, clamp=0.0)
    assert np.array_equal(t, rt) and np.allclose(v, rv / res - .5, rtol=0, atol=1e-6)


def test_extract_mesh_selects_the_subject(golden):
    from posegen_amd.raycaster import HipRayCaster
    g, cfg, kps, skts = golden
    models = [syn.make_model(cfg, s) for s in (11, 12)]
    bank = HipRayCaster.from_subjects(cfg, models, device=DEV, precision=PREC_FP32)
    try:
        r = bank.renderer
        grids = []
        for s in (0, 1):
            with r.subject(s):
                grids.append(r.grid_density(kps, skts, radius=0.9, res=16))
        assert not torch.equal(grids[0], grids[1])
        thr = _threshold(grids[1])
        assert r.selected_subject == 0
        v1, t1 = bank.extract_mesh(kps, skts, subject_idxs=torch.tensor([1, 1]), radius=0.9, res=16, threshold=thr)
        assert r.selected_subject == 0                                       # the selection is put back
        rv, rt = mr.marching_cubes_ref(grids[1].cpu().numpy(), thr, clamp=0.0)
        assert np.array_equal(t1.cpu().numpy(), rt) and len(rt) > 0
        v0, t0 = bank.extract_mesh(kps, skts, radius=0.9, res=16, threshold=thr)
        rv0, rt0 = mr.marching_cubes_ref(grids[0].cpu().numpy(), thr, clamp=0.0)
        assert np.array_equal(t0.cpu().numpy(), rt0) and np.allclose(v0.cpu().numpy(), rv0 / 16 - .5, rtol=0, atol=1e-6)
        with pytest.raises(ValueError):
            bank.extract_mesh(kps, skts, subject_idxs=2, radius=0.9, res=16, threshold=thr)
    finally:
        r.close()


def test_render_mesh_writes_one_ply_per_pose(caster, golden, tmp_path):
    g, cfg, kps, skts = golden
    _, kps2, skts2 = syn.make_pose(2, 4)
    kp = torch.cat([kps[:1], torch.tensor(kps2[:1])])
    sk = torch.cat([skts.reshape(-1, 24, 4, 4)[:1], torch.tensor(skts2[:1])])
    caster.renderer.set_precision(PREC_FP32)
    thr = _threshold(caster.renderer.grid_density(kp[:1], sk[:1], radius=0.9, res=16))
    paths = mesh.render_mesh(str(tmp_path), {"ray_caster": caster}, {"kp": kp, "skts": sk, "bones": torch.zeros(2, 24, 3)},
                             radius=0.9, res=16, threshold=thr)
    assert [p[len(str(tmp_path)):] for p in paths] == ["/meshes/000.ply", "/meshes/001.ply"]
    for i, p in enumerate(paths):
        v, t = mesh.read_ply(p)
        ev, et = caster.extract_mesh(kp[i:i + 1], sk[i:i + 1], radius=0.9, res=16, threshold=thr)
        assert np.array_equal(v, ev.cpu().numpy()) and np.array_equal(t, et.cpu().numpy())
    assert len(mesh.read_ply(paths[0])[1]) > 0
