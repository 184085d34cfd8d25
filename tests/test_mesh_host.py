"""Mesh extraction, host side: the marching-cubes case table of posegen_amd.mesh, the numpy restatement of the device algorithm
(tests/mesh_ref.py) on three closed surfaces, and the PLY writer.  No GPU.

The three fields have no value equal to the threshold and no grid face with the ambiguous diagonal sign pattern, so their vertex
counts (the sign-change edges) and positions do not depend on the table, and any hole-free table must close the surface.
What the table does on ambiguous faces BETWEEN cells is held on a random sign field (all 256 cases, thousands of ambiguous faces)
and a field of plane waves further down, together with the equality of the sparse restatement and the dense one it replaced."""
import numpy as np
import pytest

from posegen_amd import mesh
from tests import mesh_ref as mr


def test_table_uses_only_crossed_edges():
    assert mesh.TRI_TABLE.shape == (256, 3 * mesh.MAX_TRI) and mesh.N_TRI.shape == (256,)
    assert mesh.N_TRI[0] == 0 and mesh.N_TRI[255] == 0
    assert (mesh.TRI_TABLE[0] == -1).all() and (mesh.TRI_TABLE[255] == -1).all()
    for case in range(256):
        n = int(mesh.N_TRI[case])
        row = mesh.TRI_TABLE[case]
        assert (row[3 * n:] == -1).all() and (row[:3 * n] >= 0).all() and (row[:3 * n] < 12).all(), case
        inside = [(case >> c) & 1 for c in range(8)]
        crossed = {e for e in range(12) if inside[mesh.EDGE_CORNERS[e, 0]] != inside[mesh.EDGE_CORNERS[e, 1]]}
        tris = row[:3 * n].reshape(n, 3)
        for t in tris:
            assert set(t.tolist()) <= crossed, (case, t)
            assert len(set(t.tolist())) == 3, (case, t)            # no triangle repeats an edge
        # every crossed edge carries a vertex that some triangle uses
        assert set(tris.reshape(-1).tolist()) == crossed, case


def test_table_conventions():
    """corner / edge numbering as the docstring states it (the kernels and the restatement rely on it)"""
    assert mesh.CORNER_OFFSETS.tolist() == [[c & 1, c >> 1 & 1, c >> 2 & 1] for c in range(8)]
    for e in range(12):
        lo, hi = mesh.CORNER_OFFSETS[mesh.EDGE_CORNERS[e]]
        assert (lo == mesh.EDGE_LOWER[e]).all()
        assert (hi - lo).tolist() == [int(a == mesh.EDGE_AXIS[e]) for a in range(3)]


@pytest.fixture(scope="module", params=mr.FIELDS, ids=[f[0] for f in mr.FIELDS])
def field(request):
    name, fn, res, nv, nt, chi = request.param
    g = fn(res)
    v, t, v64 = mr.marching_cubes_ref(g, 0.0, want64=True)
    return g, v, t, v64, nv, nt, chi


def test_field_has_no_degenerate_input(field):
    """what makes the counts independent of the table: no value on the threshold, no ambiguous face"""
    g = field[0]
    assert not (g == 0).any()
    s = g > 0
    for a in range(3):
        m = np.moveaxis(s, a, 0)
        q = (m[:, :-1, :-1], m[:, 1:, :-1], m[:, 1:, 1:], m[:, :-1, 1:])
        assert not ((q[0] == q[2]) & (q[1] == q[3]) & (q[0] != q[1])).any()


def test_restatement_counts_and_topology(field):
    g, v, t, v64, nv, nt, chi = field
    assert v.dtype == np.float32 and t.dtype == np.int32
    assert v.shape == (nv, 3) and t.shape == (nt, 3)
    assert mr.sign_change_edges(g, 0.0) == nv
    assert t.min() == 0 and t.max() == nv - 1 and len(np.unique(t)) == nv
    assert mr.is_closed_oriented_manifold(t)
    assert mr.signed_volume6(v, t) > 0
    assert mr.euler_characteristic(nv, t) == chi


def test_restatement_vertex_positions(field):
    g, v, t, v64, nv, nt, chi = field
    assert (np.abs(v.astype(np.float64) - v64) <= mr.position_tolerance(v64)).all()
    # a vertex lies on its edge: two integer coordinates, the third inside the edge
    frac = v64 - np.floor(v64)
    assert ((frac != 0).sum(1) <= 1).all()


def test_restatement_clamp_and_empty():
    g = mr.sphere(12)               # threshold 0.1: the outside end of many crossing edges is below zero
    a = mr.marching_cubes_ref(g, 0.1, clamp=0.0)
    b = mr.marching_cubes_ref(g, 0.1, clamp=-np.inf)
    assert a[0].shape == b[0].shape and np.array_equal(a[1], b[1]) and not np.array_equal(a[0], b[0])
    for fill in (-1.0, 1.0):
        v, t = mr.marching_cubes_ref(np.full((3, 4, 5), fill, np.float32), 0.0)
        assert v.shape == (0, 3) and t.shape == (0, 3)


def test_all_single_cell_patterns_are_consistent():
    """2 x 2 x 2 grids with corner values +-1: vertex count = crossed edges, triangle count = the table's"""
    for case in range(256):
        g = np.array([1.0 if (case >> c) & 1 else -1.0 for c in range(8)], np.float32)
        grid = np.zeros((2, 2, 2), np.float32)
        for c in range(8):
            grid[tuple(mesh.CORNER_OFFSETS[c])] = g[c]
        v, t = mr.marching_cubes_ref(grid, 0.0)
        assert len(v) == mr.sign_change_edges(grid, 0.0) and len(t) == mesh.N_TRI[case]
        if len(t):
            assert mr.open_edges(t)[1]                              # no directed edge twice, even in the ambiguous cases


def test_ply_round_trip(tmp_path):
    g = mr.sphere(8)
    v, t = mr.marching_cubes_ref(g, 0.0)
    p = tmp_path / "a.ply"
    mesh.write_ply(p, v, t)
    v2, t2 = mesh.read_ply(p)
    assert v2.dtype == np.float32 and t2.dtype == np.int32
    assert np.array_equal(v, v2) and np.array_equal(t, t2)
    head = p.read_bytes()[:200]
    assert head.startswith(b"ply\nformat binary_little_endian 1.0\n") and b"property list uchar int vertex_indices" in head
    assert p.stat().st_size == head.index(b"end_header\n") + 11 + 12 * len(v) + 13 * len(t)
    e = tmp_path / "e.ply"
    mesh.write_ply(e, np.zeros((0, 3), np.float32), np.zeros((0, 3), np.int32))
    v0, t0 = mesh.read_ply(e)
    assert v0.shape == (0, 3) and t0.shape == (0, 3)


# ---- the sparse restatement against the dense one, and the table on fields with ambiguous faces ------------------------------
def _same(a, b):
    return all(x.dtype == y.dtype and x.shape == y.shape and x.tobytes() == y.tobytes() for x, y in zip(a, b)) and len(a) == len(b)


@pytest.fixture(scope="module")
def signs():
    g = mr.sign_field()
    v, t, v64 = mr.marching_cubes_ref(g, 0.0, want64=True)
    return g, v, t, v64


def test_sparse_restatement_equals_the_dense_one(signs):
    for name, fn, res, *_ in mr.FIELDS:
        g = fn(res)
        assert _same(mr.marching_cubes_ref(g, 0.0, want64=True), mr.marching_cubes_ref_dense(g, 0.0, want64=True)), name
    g = signs[0]
    assert _same(signs[1:], mr.marching_cubes_ref_dense(g, 0.0, want64=True))
    assert _same(mr.marching_cubes_ref(g, 0.3, clamp=0.0), mr.marching_cubes_ref_dense(g, 0.3, clamp=0.0))
    inner = mr.sign_field(border=False, shape=(24, 20, 17))
    assert _same(mr.marching_cubes_ref(inner, 0.0), mr.marching_cubes_ref_dense(inner, 0.0))


def test_sign_field_has_every_case_with_neighbours(signs):
    g, v, t, v64 = signs
    assert g.shape == mr.SIGN_SHAPE and (g[0] == -1).all() and (g[:, -1] == -1).all() and (g[:, :, 0] == -1).all()
    assert np.array_equal(g[1:-1, 1:-1, 1:-1], mr.sign_field(border=False, shape=(24, 20, 17)))
    assert (np.abs(g) >= np.float32(0.1)).all()
    cases = mr.cell_cases(g > 0)
    assert cases.shape == (25, 21, 18) and len(np.unique(cases)) == 256
    assert mr.ambiguous_faces(g > 0) > 1000                         # (2852: every cell has some)
    assert len(v) == mr.sign_change_edges(g, 0.0) and len(t) == int(mesh.N_TRI[cases].sum())
    assert mr.is_closed_oriented_manifold(t) and mr.signed_volume6(v, t) > 0


def _sorted_rows(v):
    return v[np.lexsort(v.T[::-1])]


def check_axis_permutations(g, v, t, run):
    """the six axis orders of grid g through run(grid) -> (vertices, triangles), against the result (v, t) of g itself"""
    import itertools
    chi = mr.euler_characteristic(len(v), t)
    for perm in itertools.permutations(range(3)):
        pv, pt = run(np.ascontiguousarray(g.transpose(perm)))
        assert _sorted_rows(pv).tobytes() == _sorted_rows(v[:, perm]).tobytes(), perm      # the same vertex set, bit for bit
        assert len(pt) == len(t) and mr.euler_characteristic(len(pv), pt) == chi, perm
        assert mr.is_closed_oriented_manifold(pt), perm
        assert mr.signed_volume6(pv, pt) > 0, perm                  # an odd permutation does not turn the surface inside out


def test_sign_field_under_axis_permutations(signs):
    g, v, t, v64 = signs
    check_axis_permutations(g, v, t, lambda p: mr.marching_cubes_ref(p, 0.0))


def test_sign_field_without_border_is_open_on_the_boundary_only():
    g = mr.sign_field(border=False, shape=(24, 20, 17))
    v, t = mr.marching_cubes_ref(g, 0.0)
    open_, uniq = mr.open_edges(t)
    assert uniq and len(open_) > 0
    assert mr.boundary_only(v, open_, g.shape)


def oriented_share(g, thr, v, t):
    """Triangle by triangle: does the normal point from the mean of the cell's inside corners to the mean of its outside ones,
    n . (outside - inside) > 0?  Held where the two means say where the sides are: cells with ONE loop of at most six edges (138
    cases).  The 24 one-loop cases with a seven-edge loop (five triangles: five corners on one side, joined across an ambiguous
    face) wind round a corner, and single triangles of them face against the cell's mean direction at any crossing positions, edge
    midpoints included; they are held to the loop's area vector (the sum of its triangles' normals, which no triangulation changes).
    Cells with several loops have a side per loop and are left to the global properties (closed, outward volume, axis orders).
    -> (share of triangles held one by one, all of them pass, share held by the loop, all of them pass)"""
    cell, case = mr.triangle_cells(g, thr)
    assert len(cell) == len(t)
    one = mr.case_loops()[case] == 1
    seven = one & (mesh.N_TRI[case] == 5)
    single = one & ~seven
    p = v[t].astype(np.float64) - cell[:, None, :]
    n = np.cross(p[:, 1] - p[:, 0], p[:, 2] - p[:, 0])
    ins = ((case[:, None] >> np.arange(8)) & 1).astype(bool)
    co = mesh.CORNER_OFFSETS.astype(np.float64)
    c_in = (ins[:, :, None] * co).sum(1) / ins.sum(1)[:, None]
    c_out = (~ins[:, :, None] * co).sum(1) / (~ins).sum(1)[:, None]
    d = np.einsum("ij,ij->i", n, c_out - c_in)
    return float(single.mean()), bool((d[single] > 0).all()), float(seven.mean()), bool((d[seven].reshape(-1, 5).sum(1) > 0).all())


def wavy_field():
    """six random plane waves on a 26 x 22 x 19 grid, threshold 0.25: smooth enough that 98 % of its triangles lie in cells with one
    loop of at most six edges, rough enough for ambiguous faces, seven-edge loops and cells with several loops"""
    rng = np.random.RandomState(5)
    x, y, z = np.meshgrid(np.linspace(0, 1, 26), np.linspace(0, 1, 22), np.linspace(0, 1, 19), indexing="ij")
    a = rng.uniform(-14, 14, size=(6, 4))
    return sum(np.sin(a[i, 0] * x + a[i, 1] * y + a[i, 2] * z + a[i, 3]) for i in range(6)).astype(np.float32)


def test_triangle_orientation_cell_by_cell(signs):
    loops = mr.case_loops()
    assert np.bincount(loops).tolist() == [2, 162, 82, 8, 2] and int(((loops == 1) & (mesh.N_TRI == 5)).sum()) == 24
    g = wavy_field()
    assert mr.ambiguous_faces(g > 0.25) > 0 and not (g == 0.25).any()
    v, t = mr.marching_cubes_ref(g, 0.25)
    share, ok, share7, ok7 = oriented_share(g, 0.25, v, t)
    print(f"wavy field: {len(t)} triangles, {share:.3f} held one by one, {share7:.3f} by their seven-edge loop")
    assert len(t) > 5000 and 0.8 <= share < 1.0 and share7 > 0
    assert ok and ok7
    # the random sign field: every one of the 138 + 24 cases, with neighbours; 0.54 of its triangles one by one, 0.13 by the loop
    g, v, t, _ = signs
    share, ok, share7, ok7 = oriented_share(g, 0.0, v, t)
    print(f"sign field: {len(t)} triangles, {share:.3f} held one by one, {share7:.3f} by their seven-edge loop")
    case = mr.triangle_cells(g, 0.0)[1]
    assert len(np.unique(case[loops[case] == 1])) == 162
    assert share > 0.5 and share7 > 0.1 and ok and ok7
    for name, fn, res, *_ in mr.FIELDS:
        f = fn(res)
        share, ok, share7, ok7 = oriented_share(f, 0.0, *mr.marching_cubes_ref(f, 0.0))
        assert share == 1.0 and ok, name
