"""Mesh extraction, host side: the marching-cubes case table of posegen_amd.mesh, the numpy restatement of the device algorithm
(tests/mesh_ref.py) on three closed surfaces, and the PLY writer.  No GPU.

The three fields have no value equal to the threshold and no grid face with the ambiguous diagonal sign pattern, so their vertex
counts (the sign-change edges) and positions do not depend on the table, and any hole-free table must close the surface."""
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
