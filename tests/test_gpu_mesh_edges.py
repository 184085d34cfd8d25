"""Marching cubes on the GPU where the other mesh tests do not reach (tests/test_gpu_mesh.py has the fixtures and the comparison):
all 256 cases with neighbours and ambiguous faces, the grid-stride loop past its first trip up to the production 256^3, grids two
points thin, values on the threshold, values that are no numbers, a grid that changed between count and emit, and the refusals.

Every comparison goes through _check_against_ref: triangles equal, vertices bit for bit the numpy restatement's (tests/mesh_ref.py),
a NaN where it has one.  What the restatement cannot vouch for by itself -- that the table closes the surface across ambiguous
faces, whatever the axis order -- is asserted on the device's own arrays.

Pinned behaviour for degenerate values (what the interpolation tt = (thr - fa) / (fb - fa) gives, as in mcubes):
  * inside is max(g, clamp) > thr, strictly: a point ON the threshold is outside, and its edge to an inside point carries a vertex
    exactly on the grid point (tt = 0 at the lower end, 1 at the upper); several vertices may then coincide, the surface stays closed
  * a NaN point is outside; +inf is inside, -inf outside (or the clamp)
  * an edge with a non-finite LOWER end, or two non-finite ends, has a NaN coordinate; with a finite lower and an infinite upper end
    tt = 0, the vertex sits on the lower point
"""
import ctypes as C

import numpy as np
import pytest
import torch

from posegen_amd import PREC_FP32, _ffi
from tests import mesh_ref as mr
from tests.test_gpu_mesh import DEV, NINF, _check_against_ref, _mc, caster, golden, renderer  # noqa: F401  (fixtures)
from tests.test_mesh_host import check_axis_permutations

pytestmark = pytest.mark.gpu

WRAP = 16384 * 256          # pg_mesh.hip blocks_for x THREADS: the point at which a kernel's grid-stride loop starts its second trip


def _twice(renderer, grid, thr, clamp=NINF):
    """_check_against_ref, and a second run gives the same bytes (a NaN's bytes included)"""
    v, t = _check_against_ref(renderer, grid, thr, clamp)
    v2, t2 = _mc(renderer, grid, thr, clamp)
    assert v.tobytes() == v2.tobytes() and t.tobytes() == t2.tobytes()
    return v, t


# ---------------------------------------------------------------------------------------------- every case, with neighbours
def test_sign_field_and_its_axis_orders(renderer):
    g = mr.sign_field()
    assert len(np.unique(mr.cell_cases(g > 0))) == 256 and mr.ambiguous_faces(g > 0) > 1000
    v, t = _twice(renderer, g, 0.0)
    assert len(v) == mr.sign_change_edges(g, 0.0)
    assert mr.is_closed_oriented_manifold(t) and mr.signed_volume6(v, t) > 0
    check_axis_permutations(g, v, t, lambda p: _twice(renderer, p, 0.0))


def test_sign_field_without_border(renderer):
    g = mr.sign_field(border=False, shape=(24, 20, 17))
    v, t = _twice(renderer, g, 0.0)
    open_, uniq = mr.open_edges(t)
    assert uniq and len(open_) > 0 and mr.boundary_only(v, open_, g.shape)


# ---------------------------------------------------------------------------------------------- the grid-stride loop
# (shape, centre of the ball): N just above WRAP, the fastest axis no multiple of 256 so that the wrap falls inside a row; a ball of
# radius 20.45 that the last plane of axis 0 cuts.  In the first shape the wrap lies in plane 157 of 163, in the second in the last
# plane (69 of 70, row 153), where no cell has its lowest point: there the second trip holds edges and their vertices only.
STRIDE_SHAPES = [((163, 161, 165), (153.7, 80.37, 82.21)), ((70, 250, 241), (60.7, 153.37, 120.21))]


@pytest.mark.parametrize("shape,centre", STRIDE_SHAPES, ids=["163x161x165", "70x250x241"])
def test_grid_stride_second_trip(renderer, shape, centre):
    N = shape[0] * shape[1] * shape[2]
    assert WRAP < N < WRAP * 1.04 and shape[2] % 256 != 0 and WRAP % shape[2] != 0
    g = mr.ball(shape, centre, 20.45)
    inside = g > 0
    cases = mr.cell_cases(inside)
    crossed = (cases != 0) & (cases != 255)
    low = np.ravel_multi_index(np.nonzero(crossed), shape)                 # linear index of the crossed cells' lowest points
    far = low + shape[1] * shape[2] + shape[2] + 1                          # ... and of their highest corner
    straddling, beyond = int(((low < WRAP) & (far >= WRAP)).sum()), int((low >= WRAP).sum())
    edge_points = np.zeros(shape, dtype=bool)                               # points that own a vertex
    edge_points[:-1] |= inside[:-1] != inside[1:]
    edge_points[:, :-1] |= inside[:, :-1] != inside[:, 1:]
    edge_points[:, :, :-1] |= inside[:, :, :-1] != inside[:, :, 1:]
    edges_beyond = int(edge_points.reshape(-1)[WRAP:].sum())
    last_plane = int(edge_points[-1].sum())
    print(f"{shape}: {int(crossed.sum())} crossed cells, {straddling} across the wrap, {beyond} beyond it; points with a vertex beyond "
          f"the wrap {edges_beyond}, in the last plane of axis 0 {last_plane}")
    assert straddling > 0 and edges_beyond > 0 and last_plane > 0
    assert beyond > 0 or WRAP // (shape[1] * shape[2]) == shape[0] - 1     # no cell starts in the last plane
    v, t = _twice(renderer, g, 0.0)
    assert len(v) == mr.sign_change_edges(g, 0.0) and len(v) > 5000
    open_, uniq = mr.open_edges(t)
    assert uniq and len(open_) > 0 and mr.boundary_only(v, open_, shape)
    assert (v[np.unique(open_)][:, 0] == shape[0] - 1).all()                # open along the cut of the last plane of axis 0 only


def test_grid_stride_production_size(renderer):
    """256^3: four full trips, and the sentinel element i == N is the only one of a fifth"""
    g = mr.torus(255)
    assert g.size == 4 * WRAP
    v, t = _twice(renderer, g, 0.0)
    assert v.shape == (127964, 3) and t.shape == (255928, 3)
    assert mr.is_closed_oriented_manifold(t) and mr.euler_characteristic(len(v), t) == 0 and mr.signed_volume6(v, t) > 0


# ---------------------------------------------------------------------------------------------- thin grids
@pytest.mark.parametrize("shape", [(2, 9, 7), (9, 2, 7), (9, 7, 2), (2, 2, 40), (2, 2, 2 * 4096 + 3)], ids=lambda s: "x".join(map(str, s)))
def test_thin_grids(renderer, shape):
    g = mr.sign_field(shape=shape, seed=11, border=False)
    v, t = _twice(renderer, g, 0.0)
    assert len(v) == mr.sign_change_edges(g, 0.0) and len(v) > 0 and len(t) > 0
    open_, uniq = mr.open_edges(t)
    assert uniq and mr.boundary_only(v, open_, shape)


# ---------------------------------------------------------------------------------------------- values on the threshold
def _zero_length_edges(f, thr):
    """(edges with tt exactly 0, with tt exactly 1, all vertex edges) of the clamped field f"""
    thr = np.float32(thr)
    n0 = n1 = n = 0
    for a in range(3):
        m = np.moveaxis(f, a, 0)
        lo, hi = m[:-1], m[1:]
        cross = (lo > thr) != (hi > thr)
        n += int(cross.sum())
        n0 += int((cross & (lo == thr)).sum())          # the lower end on the threshold (outside), the upper inside: 0 / (fb - fa)
        n1 += int((cross & (hi == thr)).sum())          # the upper end on the threshold: (thr - fa) / (thr - fa)
    return n0, n1, n


SHARE = 0.05        # of the points of the sphere field, drawn with a fixed seed, are set exactly to the threshold


def _on_threshold_field(thr):
    g = mr.sphere(20)
    pick = np.random.RandomState(2).uniform(size=g.shape) < SHARE
    assert int(pick.sum()) == 479 and g.size == 9261         # 5.2 %
    g[pick] = np.float32(thr)
    return g, pick


@pytest.mark.parametrize("thr,clamp", [(0.1, NINF), (0.1, 0.1), (0.0, 0.0)], ids=["no-clamp", "clamp-is-threshold", "clamp-0-threshold-0"])
def test_values_on_the_threshold(renderer, thr, clamp):
    g, pick = _on_threshold_field(thr)
    assert (g < 0).any() and int((g == np.float32(thr)).sum()) == int(pick.sum())
    f = np.maximum(g, np.float32(clamp))
    n0, n1, n = _zero_length_edges(f, thr)
    print(f"thr {thr} clamp {clamp}: {n} vertex edges, tt == 0 on {n0}, tt == 1 on {n1}")
    assert n0 > 0 and n1 > 0
    if clamp == thr:
        assert n0 + n1 == n                             # every outside point is lifted onto the threshold: all vertices on grid points
    else:
        assert n - n0 - n1 > 0
    v, t = _twice(renderer, g, thr, clamp)
    assert len(v) == n == mr.sign_change_edges(g, thr, clamp)
    assert int(((v == np.floor(v)).all(1)).sum()) == n0 + n1
    assert mr.is_closed_oriented_manifold(t)
    if clamp == thr:                                    # and the ball's own points are the same inside set as without the picks' holes
        assert mr.signed_volume6(v, t) > 0


# ---------------------------------------------------------------------------------------------- values that are no numbers
def _non_finite_field():
    g = mr.sphere(12)
    s = g > 0
    up = np.argwhere(s[:-1] & ~s[1:])                  # inside, the +axis-0 neighbour outside
    down = np.argwhere(s[:, 1:] & ~s[:, :-1])          # inside, the -axis-1 neighbour outside
    a, b = tuple(up[len(up) // 2]), tuple(down[len(down) // 3] + [0, 1, 0])
    assert a != b and s[a] and not s[a[0] + 1, a[1], a[2]] and s[b] and not s[b[0], b[1] - 1, b[2]]
    g[a] = np.inf
    g[b] = np.inf
    deep = (6, 6, 6)                                    # an inside point with six inside neighbours
    assert s[5:8, 5:8, 5:8].all()
    g[deep] = np.nan
    out_next = tuple(np.argwhere(~s[:-1] & s[1:])[7])  # outside, the +axis-0 neighbour inside
    g[out_next] = -np.inf
    g[2, 9, 4] = np.nan                                 # outside points far from and next to the surface
    nan_next = tuple(np.argwhere(~s[:, :, :-1] & s[:, :, 1:])[11])
    g[nan_next] = np.nan
    g[8, 6, 6] = -np.inf                                # inside the ball: a second hole
    return g, deep


@pytest.mark.parametrize("clamp", [NINF, 0.0], ids=["no-clamp", "clamp-0"])
def test_non_finite_values(renderer, clamp):
    g, deep = _non_finite_field()
    v, t = _twice(renderer, g, 0.0, clamp)
    rv, rt = mr.marching_cubes_ref(g, 0.0, clamp=clamp)
    n_nan = int(np.isnan(rv).any(1).sum())
    print(f"clamp {clamp}: {len(rv)} vertices, {n_nan} with a NaN coordinate")
    assert n_nan > 0 and np.array_equal(np.isnan(v), np.isnan(rv)) and not np.isinf(v).any()
    assert (np.isnan(v).sum(1) <= 1).all()              # only the coordinate along the edge
    assert len(v) == mr.sign_change_edges(g, 0.0, clamp)
    # a NaN point is outside: the triangles are those of the grid with -1 in its place, and the deep one opens a hole of six edges
    h = np.where(np.isnan(g), np.float32(-1), g)
    assert np.array_equal(t, mr.marching_cubes_ref(h, 0.0, clamp=clamp)[1])
    filled = g.copy()
    filled[deep] = 1.0
    assert mr.sign_change_edges(g, 0.0, clamp) == mr.sign_change_edges(filled, 0.0, clamp) + 6
    assert mr.is_closed_oriented_manifold(t)


# ---------------------------------------------------------------------------------------------- count and emit
GUARD = 64


def _guarded(n, dtype):
    big = torch.full((GUARD + n + GUARD, 3), -7, device=DEV, dtype=dtype)
    return big, C.c_void_p(big[GUARD:].data_ptr())


def _untouched(big, n):
    return bool((big[:GUARD] == -7).all()) and bool((big[GUARD + n:] == -7).all())


def test_emit_on_a_grid_that_changed_since_the_count(renderer):
    """the slots come from the count's flags and scans: another grid of the same shape moves no store"""
    r = renderer
    a = mr.sphere(10)
    rv, rt = mr.marching_cubes_ref(a, 0.0)
    ga = torch.tensor(a).to(DEV)
    nv, nt = C.c_int64(), C.c_int64()
    shape = (11, 11, 11, 0.0, NINF)
    assert r.lib.pg_mesh_count(r.handle, r._stream(), C.c_void_p(ga.data_ptr()), *shape, C.byref(nv), C.byref(nt)) == _ffi.PG_OK
    assert (nv.value, nt.value) == (len(rv), len(rt))
    for gb in (-ga, torch.full_like(ga, 0.25)):
        bv, pv = _guarded(nv.value, torch.float32)
        bt, pt = _guarded(nt.value, torch.int32)
        assert r.lib.pg_mesh_emit(r.handle, r._stream(), C.c_void_p(gb.data_ptr()), *shape, pv, pt, nv.value, nt.value) == _ffi.PG_OK
        torch.cuda.synchronize()
        assert _untouched(bv, nv.value) and _untouched(bt, nt.value)
        t = bt[GUARD:GUARD + nt.value].cpu().numpy()
        assert t.min() >= 0 and t.max() < nv.value and np.array_equal(t, rt)


def test_mesh_refusals_write_nothing(renderer, golden):
    from posegen_amd.raycaster import HipRayCaster
    from tests.helpers import model_for
    r = renderer
    g = torch.tensor(mr.sphere(8)).to(DEV)
    gp = C.c_void_p(g.data_ptr())
    nv, nt = C.c_int64(-5), C.c_int64(-5)
    nan = float("nan")
    count = lambda h, thr, clamp: h.lib.pg_mesh_count(h.handle, h._stream(), gp, 9, 9, 9, thr, clamp, C.byref(nv), C.byref(nt))
    assert count(r, nan, NINF) == _ffi.PG_EINVAL and count(r, 0.0, nan) == _ffi.PG_EINVAL
    assert (nv.value, nt.value) == (-5, -5)
    assert count(r, 0.0, -0.0) == _ffi.PG_OK and nv.value > 0
    bv, pv = _guarded(nv.value, torch.float32)
    bt, pt = _guarded(nt.value, torch.int32)
    emit = lambda h, thr, clamp: h.lib.pg_mesh_emit(h.handle, h._stream(), gp, 9, 9, 9, thr, clamp, pv, pt, nv.value, nt.value)
    clean = lambda: bool((bv == -7).all()) and bool((bt == -7).all())
    # same_float: equal values (+0 and -0 are equal), or both NaN -- which a count never leaves, so a NaN is always another value
    for thr, clamp in ((0.5, -0.0), (0.0, NINF), (0.0, 1e-30), (nan, -0.0), (0.0, nan), (nan, nan)):
        assert emit(r, thr, clamp) == _ffi.PG_ESTATE, (thr, clamp)
    torch.cuda.synchronize()
    assert clean()
    assert emit(r, -0.0, 0.0) == _ffi.PG_OK             # the count's threshold and clamp with the other zero's sign
    torch.cuda.synchronize()
    assert not clean() and _untouched(bv, nv.value) and _untouched(bt, nt.value)
    rv, rt = mr.marching_cubes_ref(mr.sphere(8), 0.0, clamp=0.0)
    assert np.array_equal(bt[GUARD:GUARD + nt.value].cpu().numpy(), rt) and bv[GUARD:GUARD + nv.value].cpu().numpy().tobytes() == rv.tobytes()
    # a handle that never counted
    gd, cfg, kps, skts = golden
    fresh = HipRayCaster.from_weights(cfg, *model_for(cfg, int(gd["seed_model"])), device=DEV, precision=PREC_FP32)
    try:
        bv.fill_(-7); bt.fill_(-7)
        assert emit(fresh.renderer, 0.0, -0.0) == _ffi.PG_ESTATE
        torch.cuda.synchronize()
        assert clean()
    finally:
        fresh.renderer.close()
