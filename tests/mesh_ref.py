"""numpy restatement of the device marching cubes (posegen_amd/csrc/pg_mesh.hip), on the package's own case table, and the
mesh properties the tests assert.  Not a test module.

The algorithm, as the kernels implement it, on f = max(grid, clamp) in float32:
  * a point is inside when f > threshold
  * one vertex per grid edge (point i to i + 1 along axis a) whose ends differ: tt = (threshold - fa) / (fb - fa) in float32
    with fa at the lower index, coordinate i + tt on axis a (float32), the integer indices on the other two
  * vertex order: linear index of the edge's lower point (last axis fastest), then axis
  * triangles per cell in the order of the cell's lowest point, then table order; they name the edge vertices through the
    exclusive scan of the edge flags
"""
import numpy as np

from posegen_amd.mesh import CORNER_OFFSETS, EDGE_AXIS, EDGE_LOWER, MAX_TRI, N_TRI, TRI_TABLE


def cell_cases(inside):
    """the case of every cell [Nx-1,Ny-1,Nz-1] uint8: sum over the corners that are inside of 1 << c"""
    n = [k - 1 for k in inside.shape]
    case = np.zeros(n, dtype=np.uint8)
    for c, (ox, oy, oz) in enumerate(CORNER_OFFSETS.tolist()):
        case |= inside[ox:ox + n[0], oy:oy + n[1], oz:oz + n[2]].astype(np.uint8) << np.uint8(c)
    return case


def marching_cubes_ref(grid, threshold, clamp=-np.inf, want64=False):
    """-> (vertices float32 [nv,3], triangles int32 [nt,3]) (+ the vertices by the float64 formula with want64).
    The table is gathered for the cells the surface crosses only (case neither 0 nor 255), so a 256^3 grid takes about a second."""
    f = np.maximum(np.asarray(grid, dtype=np.float32), np.float32(clamp))
    thr = np.float32(threshold)
    N = f.shape
    inside = f > thr
    flags = np.zeros(N + (3,), dtype=bool)
    for a in range(3):
        lo = [slice(None)] * 3
        hi = [slice(None)] * 3
        lo[a], hi[a] = slice(0, N[a] - 1), slice(1, N[a])
        flags[tuple(lo) + (a,)] = inside[tuple(lo)] != inside[tuple(hi)]
    flat = flags.reshape(-1)
    vid = (np.cumsum(flat, dtype=np.int32) - flat).reshape(flags.shape)     # exclusive scan (32-bit, as the device's)
    idx = np.argwhere(flags)                                        # rows (ix, iy, iz, a) in exactly the vertex order
    p, a = idx[:, :3], idx[:, 3]
    q = p.copy()
    q[np.arange(len(a)), a] += 1
    fa, fb = f[tuple(p.T)], f[tuple(q.T)]
    with np.errstate(all="ignore"):
        tt = ((thr - fa) / (fb - fa)).astype(np.float32)
        verts = p.astype(np.float32)
        verts[np.arange(len(a)), a] = (p[np.arange(len(a)), a].astype(np.float32) + tt).astype(np.float32)
        v64 = p.astype(np.float64)
        v64[np.arange(len(a)), a] += (np.float64(thr) - fa.astype(np.float64)) / (fb.astype(np.float64) - fa.astype(np.float64))
    # cells, in the order of their lowest point; those of case 0 and 255 have no triangle
    cases = cell_cases(inside)
    act = np.flatnonzero((cases != 0) & (cases != 255))
    cell = np.stack(np.unravel_index(act, cases.shape), -1).reshape(-1, 3)
    case = cases.reshape(-1)[act].astype(np.int64)
    edges = TRI_TABLE[case].astype(np.int64).reshape(len(cell), MAX_TRI, 3)
    keep = np.arange(MAX_TRI)[None, :] < N_TRI[case][:, None]
    e = np.where(edges < 0, 0, edges)
    pt = cell[:, None, None, :] + EDGE_LOWER[e]
    ids = vid[pt[..., 0], pt[..., 1], pt[..., 2], EDGE_AXIS[e]]
    tris = ids[keep].astype(np.int32).reshape(-1, 3)
    return (verts, tris, v64) if want64 else (verts, tris)


def marching_cubes_ref_dense(grid, threshold, clamp=-np.inf, want64=False):
    """marching_cubes_ref as it first stood: the table gathered for every cell ([cells, 5, 3, 3] int64 arrays, some 6 GB at 256^3).
    Kept as the check of the sparse form above: the two return equal arrays (tests/test_mesh_host.py)."""
    f = np.maximum(np.asarray(grid, dtype=np.float32), np.float32(clamp))
    thr = np.float32(threshold)
    N = f.shape
    inside = f > thr
    flags = np.zeros(N + (3,), dtype=bool)
    for a in range(3):
        lo = [slice(None)] * 3
        hi = [slice(None)] * 3
        lo[a], hi[a] = slice(0, N[a] - 1), slice(1, N[a])
        flags[tuple(lo) + (a,)] = inside[tuple(lo)] != inside[tuple(hi)]
    flat = flags.reshape(-1)
    vid = (np.cumsum(flat) - flat).reshape(flags.shape)             # exclusive scan
    idx = np.argwhere(flags)                                        # rows (ix, iy, iz, a) in exactly the vertex order
    p, a = idx[:, :3], idx[:, 3]
    q = p.copy()
    q[np.arange(len(a)), a] += 1
    fa, fb = f[tuple(p.T)], f[tuple(q.T)]
    with np.errstate(all="ignore"):
        tt = ((thr - fa) / (fb - fa)).astype(np.float32)
        verts = p.astype(np.float32)
        verts[np.arange(len(a)), a] = (p[np.arange(len(a)), a].astype(np.float32) + tt).astype(np.float32)
        v64 = p.astype(np.float64)
        v64[np.arange(len(a)), a] += (np.float64(thr) - fa.astype(np.float64)) / (fb.astype(np.float64) - fa.astype(np.float64))
    # cells
    cx, cy, cz = np.meshgrid(np.arange(N[0] - 1), np.arange(N[1] - 1), np.arange(N[2] - 1), indexing="ij")
    cell = np.stack([cx, cy, cz], -1).reshape(-1, 3)                 # cell order = order of the lowest point
    case = np.zeros(len(cell), dtype=np.int64)
    for c in range(8):
        o = cell + CORNER_OFFSETS[c]
        case |= inside[tuple(o.T)].astype(np.int64) << c
    edges = TRI_TABLE[case].astype(np.int64).reshape(len(cell), MAX_TRI, 3)
    keep = np.arange(MAX_TRI)[None, :] < N_TRI[case][:, None]
    e = np.where(edges < 0, 0, edges)
    pt = cell[:, None, None, :] + EDGE_LOWER[e]
    ids = vid[pt[..., 0], pt[..., 1], pt[..., 2], EDGE_AXIS[e]]
    tris = ids[keep].astype(np.int32).reshape(-1, 3)
    return (verts, tris, v64) if want64 else (verts, tris)


def position_tolerance(v64):
    """three float32 roundings in tt and the rounding of i + tt"""
    return 2.0 ** -21 + np.spacing(np.abs(v64).astype(np.float32)).astype(np.float64)


def sign_change_edges(grid, threshold, clamp=-np.inf):
    f = np.maximum(np.asarray(grid, dtype=np.float32), np.float32(clamp)) > np.float32(threshold)
    return int((f[1:] != f[:-1]).sum() + (f[:, 1:] != f[:, :-1]).sum() + (f[:, :, 1:] != f[:, :, :-1]).sum())


def directed_edges(tris):
    t = np.asarray(tris, dtype=np.int64)
    return np.concatenate([t[:, [0, 1]], t[:, [1, 2]], t[:, [2, 0]]])


def open_edges(tris):
    """directed edges whose reverse is missing or that occur more than once -> ([k,2] array, all directed edges unique?)"""
    d = directed_edges(tris)
    key = d[:, 0] * (d.max() + 1 if len(d) else 1) + d[:, 1]
    rev = d[:, 1] * (d.max() + 1 if len(d) else 1) + d[:, 0]
    uniq = len(np.unique(key)) == len(key)
    return d[~np.isin(key, rev)], uniq


def is_closed_oriented_manifold(tris):
    """every directed edge occurs once and its reverse once"""
    missing, uniq = open_edges(tris)
    return uniq and len(missing) == 0


def euler_characteristic(n_vertices, tris):
    d = np.sort(directed_edges(tris), axis=1)
    return n_vertices - len(np.unique(d, axis=0)) + len(tris)


def signed_volume6(verts, tris):
    v = np.asarray(verts, dtype=np.float64)
    return float(np.einsum("ij,ij->i", v[tris[:, 0]], np.cross(v[tris[:, 1]], v[tris[:, 2]])).sum())


# ---- the fields of the tests ------------------------------------------------------------------------------------------------
CENTRE = (0.013, -0.021, 0.007)


def _lattice(res):
    t = np.linspace(-1, 1, res + 1)
    return np.meshgrid(t, t, t, indexing="ij")


def sphere(res, r=0.6):
    x, y, z = _lattice(res)
    cx, cy, cz = CENTRE
    return (r - np.sqrt((x - cx) ** 2 + (y - cy) ** 2 + (z - cz) ** 2)).astype(np.float32)


def torus(res):
    x, y, z = _lattice(res)
    cx, cy, cz = CENTRE
    return (0.25 - np.hypot(np.hypot(x - cx, y - cy) - 0.55, z - cz)).astype(np.float32)


def blobs(res):
    x, y, z = _lattice(res)
    g = lambda a, b, c: np.exp(-8 * ((x - a) ** 2 + (y - b) ** 2 + (z - c) ** 2))
    return (g(.3, 0, 0) + g(-.3, .05, 0) - 0.5).astype(np.float32)


# (name, field, res, vertices, triangles, Euler characteristic)
FIELDS = [("sphere", sphere, 16, 414, 824, 2), ("torus", torus, 24, 1134, 2268, 0), ("blobs", blobs, 16, 210, 416, 2)]


# ---- fields with every case, ambiguous faces and values that are no numbers ------------------------------------------------------
SIGN_SHAPE = (26, 22, 19)
SIGN_SEED = 7


def sign_field(shape=SIGN_SHAPE, seed=SIGN_SEED, border=True):
    """uniform(0.1, 1) x +-1 from a fixed seed; with `border` the outermost layer of points is -1 (outside at threshold 0), so the
    surface is closed.  sign_field(border=False) of shape n - 2 is the interior of sign_field() of shape n."""
    rng = np.random.RandomState(seed)
    inner = tuple(n - 2 for n in shape) if border else tuple(shape)
    g = (rng.uniform(0.1, 1.0, size=inner) * rng.choice([-1.0, 1.0], size=inner)).astype(np.float32)
    if not border:
        return g
    out = np.full(shape, -1.0, dtype=np.float32)
    out[1:-1, 1:-1, 1:-1] = g
    return out


def ambiguous_faces(inside):
    """grid faces whose inside corners are the two ends of one diagonal"""
    n = 0
    for a in range(3):
        m = np.moveaxis(inside, a, 0)
        q = (m[:, :-1, :-1], m[:, 1:, :-1], m[:, 1:, 1:], m[:, :-1, 1:])
        n += int(((q[0] == q[2]) & (q[1] == q[3]) & (q[0] != q[1])).sum())
    return n


def case_loops():
    """[256] the number of closed loops (connected pieces of surface) the table draws in a cell of each case"""
    out = np.zeros(256, dtype=np.int64)
    for case in range(256):
        tris = TRI_TABLE[case][:3 * N_TRI[case]].reshape(-1, 3).tolist()
        root = {e: e for t in tris for e in t}

        def find(e):
            while root[e] != e:
                e = root[e]
            return e
        for t in tris:
            root[find(t[1])] = find(t[0])
            root[find(t[2])] = find(t[0])
        out[case] = len({find(e) for e in root})
    return out


def triangle_cells(grid, threshold, clamp=-np.inf):
    """-> (cell [nt,3], case [nt]) of every triangle of marching_cubes_ref: triangles come cell by cell, N_TRI[case] each"""
    inside = np.maximum(np.asarray(grid, dtype=np.float32), np.float32(clamp)) > np.float32(threshold)
    cases = cell_cases(inside)
    n = N_TRI[cases.reshape(-1)]
    cell = np.stack(np.unravel_index(np.arange(cases.size), cases.shape), -1)
    return np.repeat(cell, n, axis=0), np.repeat(cases.reshape(-1), n)


def boundary_only(verts, open_, shape):
    """do both ends of every edge of open_ [k,2] have a coordinate equal to 0 or to n - 1?"""
    v = np.asarray(verts)
    on = ((v == 0) | (v == np.asarray(shape, dtype=v.dtype) - 1)).any(1)
    return bool(on[open_].all())


def ball(shape, centre, radius):
    """radius - |p - centre| in index coordinates on a grid of any shape (float32)"""
    x, y, z = np.meshgrid(*[np.arange(n, dtype=np.float64) for n in shape], indexing="ij", sparse=True)
    return (radius - np.sqrt((x - centre[0]) ** 2 + (y - centre[1]) ** 2 + (z - centre[2]) ** 2)).astype(np.float32)
