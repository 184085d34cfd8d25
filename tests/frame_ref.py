"""The frame front and back end restated in plain numpy (no device code): the yardstick of tests/test_gpu_frame_edges.py, pinned
without a GPU by tests/test_frame_ref_host.py.

Every function reads what the device reads: the float32 camera, the float32 intrinsics (fx, fy, cx, cy) as
raycaster._intrinsics produces them, the integer box (tl_x, tl_y, br_x, br_y; `br` row / column excluded) -- clamped to the frame
as frame_geom (pg_frames.hip) clamps it.  Boxes themselves are rays.kp_to_boxes' (float64 numpy like the reference, pinned to its
fixture): they are not restated here.

  box_rays64 / box_rays32     frame_rays_kernel's columns 0-7, float64 and float32 (rays.pixel_rays: the reference's order)
  compose64 / compose32       frame_compose_kernel's rgb, disp, acc;  rgb8_of: its uint8 frame
  CASES                       one table of frame geometries off the square, centred, in-frame case, for the host and the GPU tests
"""
import numpy as np
import torch

from posegen_amd import synthetic as syn
from posegen_amd.raycaster import _intrinsics
from posegen_amd.rays import kp_to_boxes, pixel_rays

U = 2.0 ** -24                  # unit roundoff of float32
EXT_SCALE = 0.001


def intrinsics32(H, W, focal, center=None):
    """(fx, fy, cx, cy) as the ABI takes them: _intrinsics' doubles rounded to float32"""
    return np.array(_intrinsics(H, W, focal, center), dtype=np.float32)


def flat_box(box):
    """((tl_x, tl_y), (br_x, br_y)) or a flat 4-vector -> four ints"""
    return tuple(int(v) for v in np.asarray(box).reshape(-1))


def clamp_box(H, W, box):
    """frame_geom's clamp -> (tl_x, tl_y, bw, bh): tl to >= 0, br to <= W, H; a box without pixels has bw * bh = 0"""
    tlx, tly, brx, bry = flat_box(box)
    tlx, tly = max(tlx, 0), max(tly, 0)
    brx, bry = min(brx, W), min(bry, H)
    return tlx, tly, max(brx - tlx, 0), max(bry - tly, 0)


def box_pixels(H, W, box):
    """rows, cols (int64) of the clamped box's pixels, row-major"""
    tlx, tly, bw, bh = clamp_box(H, W, box)
    rr, cc = np.arange(tly, tly + bh), np.arange(tlx, tlx + bw)
    return np.repeat(rr, bw), np.tile(cc, bh)


def box_rays64(H, W, intr, c2w, box, near, far):
    """-> (rows [n,8] float64: origin, d = dx R[:,0] + dy R[:,1] - R[:,2], near, far;  mag [n,3] = |dx R0| + |dy R1| + |R2|),
    dx = (c - cx) / fx, dy = -(r - cy) / fy, every input widened from the float32 the device holds"""
    fx, fy, cx, cy = (float(v) for v in np.asarray(intr, dtype=np.float32))
    m = np.asarray(c2w, dtype=np.float32).astype(np.float64)
    R, t = m[:3, :3], m[:3, 3]
    r, c = box_pixels(H, W, box)
    dx = ((c - cx) / fx)[:, None]
    dy = (-(r - cy) / fy)[:, None]
    d = dx * R[:, 0] + dy * R[:, 1] - R[:, 2]
    mag = np.abs(dx * R[:, 0]) + np.abs(dy * R[:, 1]) + np.abs(R[:, 2])
    n = len(r)
    rows = np.concatenate([np.broadcast_to(t, (n, 3)), d, np.full((n, 1), float(np.float32(near))), np.full((n, 1), float(np.float32(far)))], 1)
    return rows, mag


def box_rays32(H, W, intr, c2w, box, near, far):
    """rows [n,8] float32 in the reference's operation order: rays.pixel_rays (pinned to the reference's fixture) on the clamped
    box's pixels, with the float32 intrinsics"""
    fx, fy, cx, cy = (float(v) for v in np.asarray(intr, dtype=np.float32))
    r, c = box_pixels(H, W, box)
    ro, rd = pixel_rays(torch.from_numpy(r), torch.from_numpy(c), H, W, (fx, fy),
                        torch.from_numpy(np.ascontiguousarray(np.asarray(c2w, dtype=np.float32)[:3, :4])), center=(cx, cy))
    n = len(r)
    nf = np.broadcast_to(np.array([near, far], dtype=np.float32), (n, 2))
    return np.concatenate([ro.numpy().reshape(n, 3), rd.numpy().reshape(n, 3), nf], 1).astype(np.float32)


def unit64(d):
    """float64 normalisation of direction rows"""
    d = np.asarray(d, dtype=np.float64)
    return d / np.sqrt((d * d).sum(-1, keepdims=True))


def _inside(H, W, box):
    """(flat pixel ids of the clamped box in map order)"""
    r, c = box_pixels(H, W, box)
    return r * W + c


def _background(H, W, bg, base_bg, dtype):
    if bg is None:
        return np.full((H * W, 3), base_bg, dtype=np.float32).astype(dtype)
    return np.asarray(bg, dtype=np.float32).reshape(H * W, 3).astype(dtype)


def _maps(maps, n):
    rgb_map, disp_map, acc_map = maps
    if n == 0:
        return np.zeros((0, 3), np.float32), np.zeros(0, np.float32), np.zeros(0, np.float32)
    return (np.asarray(rgb_map, dtype=np.float32).reshape(n, 3), np.asarray(disp_map, dtype=np.float32).reshape(n),
            np.asarray(acc_map, dtype=np.float32).reshape(n))


def compose64(H, W, box, rgb_map, disp_map, acc_map, bg, base_bg):
    """-> rgb [H W,3], disp [H W], acc [H W] float64: rgb_map + (1 - acc) bg inside the clamped box (maps row-major with the
    clamped width), NaN disparity -> 0; outside the box the background with disp = acc = 0"""
    ids = _inside(H, W, box)
    rm, dm, am = (x.astype(np.float64) for x in _maps((rgb_map, disp_map, acc_map), len(ids)))
    rgb = _background(H, W, bg, base_bg, np.float64)
    disp, acc = np.zeros(H * W), np.zeros(H * W)
    rgb[ids] = rm + (1.0 - am)[:, None] * rgb[ids]
    disp[ids] = np.where(np.isnan(dm), 0.0, dm)
    acc[ids] = am
    return rgb, disp, acc


def compose_mag64(H, W, box, rgb_map, acc_map, bg, base_bg):
    """[H W,3]: |rgb_map| + |(1 - acc) bg| inside the box, 0 outside (the background is copied) -- what compose's bound scales with"""
    ids = _inside(H, W, box)
    rm, _, am = (x.astype(np.float64) for x in _maps((rgb_map, acc_map, acc_map), len(ids)))
    b = _background(H, W, bg, base_bg, np.float64)
    mag = np.zeros((H * W, 3))
    mag[ids] = np.abs(rm) + np.abs((1.0 - am)[:, None] * b[ids])
    return mag


def compose32(H, W, box, rgb_map, disp_map, acc_map, bg, base_bg):
    """compose64 in float32: subtraction, product and sum each rounded once"""
    ids = _inside(H, W, box)
    rm, dm, am = _maps((rgb_map, disp_map, acc_map), len(ids))
    rgb = _background(H, W, bg, base_bg, np.float32)
    disp, acc = np.zeros(H * W, np.float32), np.zeros(H * W, np.float32)
    with np.errstate(invalid="ignore", over="ignore"):
        t = (np.float32(1.0) - am).astype(np.float32)
        p = (t[:, None] * rgb[ids]).astype(np.float32)
        rgb[ids] = (rm + p).astype(np.float32)
    disp[ids] = np.where(np.isnan(dm), np.float32(0.0), dm)
    acc[ids] = am
    return rgb, disp, acc


def rgb8_of(rgb32):
    """trunc(min(max(rgb32 * 255f, 0), 255)): the product rounded once in float32, fmax / fmin semantics (a NaN colour -> 0)"""
    with np.errstate(invalid="ignore", over="ignore"):
        p = (np.asarray(rgb32, dtype=np.float32) * np.float32(255.0)).astype(np.float32)
    return np.fmin(np.fmax(p, np.float32(0.0)), np.float32(255.0)).astype(np.uint8)


def rgb8_of64(rgb32):
    """the float64 truncation of the same float32 colours (the product with 255 is exact in float64)"""
    p = np.asarray(rgb32, dtype=np.float32).astype(np.float64) * 255.0
    return np.fmin(np.fmax(p, 0.0), 255.0).astype(np.uint8)


# ---- distances in units of the GPU test's bounds (a ratio <= 1 holds the bound) ---------------------------------------------------------
def ray_excess(got, H, W, intr, c2w, box, near=0., far=1.):
    """worst |direction - box_rays64| / (4u mag) of rows [n,>=8] (inf: another ray count, or origin / near / far differ)"""
    want, mag = box_rays64(H, W, intr, c2w, box, near, far)
    got = np.asarray(got, dtype=np.float64)
    if got.shape[0] != want.shape[0] or not np.array_equal(got[:, [0, 1, 2, 6, 7]], want[:, [0, 1, 2, 6, 7]]):
        return np.inf
    return float((np.abs(got[:, 3:6] - want[:, 3:6]) / (4 * U * mag)).max()) if len(want) else 0.0


def unit_excess(rows):
    """worst |columns 8-10 - float64 normalisation of columns 3-5| / (5u |v|)"""
    v = unit64(rows[:, 3:6])
    return float((np.abs(np.asarray(rows[:, 8:11], dtype=np.float64) - v) / (5 * U * np.abs(v))).max())


def compose_excess(got_rgb, H, W, box, maps, bg, base_bg):
    """worst |rgb - compose64| / (3u (|rgb_map| + |(1 - acc) bg|)) over the finite pixels (0 / 0 where the background is copied: 0)"""
    want = compose64(H, W, box, *maps, bg, base_bg)[0]
    mag = compose_mag64(H, W, box, maps[0], maps[2], bg, base_bg)
    err = np.abs(np.asarray(got_rgb, dtype=np.float64).reshape(-1, 3) - want)
    ok = np.isfinite(want)
    if not np.array_equal(np.isfinite(np.asarray(got_rgb).reshape(-1, 3)), ok):
        return np.inf
    with np.errstate(invalid="ignore", divide="ignore"):
        q = np.where(err[ok] == 0, 0.0, err[ok] / (3 * U * mag[ok]))
    return float(q.max())


# ---- the table of geometries ---------------------------------------------------------------------------------------------------
def camera(shift=(0., 0., 0.), roll=0., H=64, W=64):
    """synthetic.make_camera's extrinsic moved by `shift` along its own axes and rolled by `roll` degrees about its view axis
    -> c2w [4,4] float32"""
    c2w = syn.make_camera(1, H, W)[0][0].astype(np.float64)
    a = np.deg2rad(roll)
    rz = np.array([[np.cos(a), -np.sin(a), 0.], [np.sin(a), np.cos(a), 0.], [0., 0., 1.]])
    out = c2w.copy()
    out[:3, 3] = c2w[:3, 3] + c2w[:3, :3] @ np.asarray(shift, dtype=np.float64)
    out[:3, :3] = c2w[:3, :3] @ rz
    return out.astype(np.float32)


def _case(name, H, W, focal, center=None, shift=(0., 0., 0.), roll=0., seed=5):
    return {"name": name, "H": H, "W": W, "focal": focal, "center": center, "shift": shift, "roll": roll, "seed": seed}


F40 = 39.0625                   # make_camera's focal at 40 rows: 500 * 40 / 512
CASES = [
    _case("interior", 40, 72, F40, shift=(0., 0., 2.)),
    _case("left", 40, 72, F40, shift=(4.5, 0., 2.)),
    _case("right", 40, 72, F40, shift=(-4.5, 0., 2.)),
    _case("top", 40, 72, F40, shift=(0., -2.5, 2.)),
    _case("bottom", 40, 72, F40, shift=(0., 2.5, 2.)),
    _case("whole", 40, 72, F40, shift=(0., 0., -2.)),
    _case("tall", 72, 40, F40, shift=(0., 0., 1.)),
    _case("odd", 41, 75, (41.5, 37.25), shift=(0., 0., 1.5)),
    _case("offcentre", 40, 72, (36.5, 43.0), center=(30.7, 17.4), shift=(0., 0., 2.)),
    _case("rolled", 48, 80, (45.0, 52.5), center=(37.25, 26.6), shift=(0.3, -0.2, 1.5), roll=35.),
    _case("empty", 40, 72, F40, center=(-30., 12.)),
]
CASE_IDS = [c["name"] for c in CASES]


def case_inputs(case):
    """-> dict: c2w [4,4] f32, kps [1,24,3] f32, skts [1,24,4,4] f32, cyl [1,5] f32 tensor, box ((tl_x, tl_y), (br_x, br_y)),
    intr (fx, fy, cx, cy) f32 -- the box from rays.kp_to_boxes, never from stored numbers"""
    H, W = case["H"], case["W"]
    c2w = camera(case["shift"], case["roll"], H, W)
    _, kps, skts = syn.make_pose(1, case["seed"])
    cyls, boxes, _ = kp_to_boxes([c2w], H, W, [case["focal"]], kps=torch.tensor(kps), ext_scale=EXT_SCALE,
                                 centers=None if case["center"] is None else [case["center"]])
    tl, br = boxes[0]
    return {"c2w": c2w, "kps": kps, "skts": skts, "cyl": cyls[:1], "box": ((int(tl[0]), int(tl[1])), (int(br[0]), int(br[1]))),
            "intr": intrinsics32(H, W, case["focal"], case["center"])}


def n_rays(case, box):
    _, _, bw, bh = clamp_box(case["H"], case["W"], box)
    return bw * bh


def ring_points(cyl, c2w, focal):
    """cylinder_to_box_2d's 100 ring points in camera coordinates [100,3] and projected [100,2] (float64, its own operations), for
    the vetting of the box inputs: depth > 0, |u|, |v| < 2^30, no extreme within 1e-6 of an integer"""
    from posegen_amd.skeleton import focal_to_intrinsic_np, nerf_c2w_to_extrinsic
    cyl = np.asarray(cyl).reshape(-1)
    phi = np.linspace(0., 2 * np.pi, 50)
    ring_x = cyl[0] + np.cos(phi) * cyl[2]
    ring_z = cyl[1] + np.sin(phi) * cyl[2]
    ones = np.ones_like(ring_x)
    pts = np.concatenate([np.stack([ring_x, cyl[3] * ones, ring_z, ones], axis=-1),
                          np.stack([ring_x, cyl[4] * ones, ring_z, ones], axis=-1)], axis=0)
    cam = pts @ nerf_c2w_to_extrinsic(np.asarray(c2w)).T
    pix = cam @ focal_to_intrinsic_np(focal).T
    return cam[:, :3], pix[:, :2] / pix[:, 2:3]


def random_box_batch(n=129, seed=7, H=75, W=101, focal=(88.0, 97.5), center=(43.3, 41.8)):
    """The GPU box test's random batch: n poses, each with its own shifted, rolled camera, on a 75 x 101 frame with an off-centre
    principal point -> (kps [n,24,3] f32, c2ws [n,4,4] f32, H, W, focal, center)"""
    _, kps, _ = syn.make_pose(n, seed)
    rng = np.random.RandomState(seed)
    shifts = rng.uniform(-1.0, 1.0, size=(n, 3)) * np.array([4.0, 4.0, 2.0]) + np.array([0., 0., 1.5])
    rolls = rng.uniform(-60., 60., size=n)
    c2ws = np.stack([camera(shifts[i], rolls[i], H, W) for i in range(n)])
    return kps, c2ws, H, W, focal, center


def host_boxes(kps, c2ws, H, W, focal, center):
    """kp_to_boxes -> (cyls [n,5] f32, boxes [n,4] int: tl_x, tl_y, br_x, br_y)"""
    n = len(c2ws)
    cyls, boxes, _ = kp_to_boxes(list(c2ws), H, W, [focal] * n, kps=torch.as_tensor(kps), ext_scale=EXT_SCALE,
                                 centers=None if center is None else [center] * n)
    return cyls.numpy(), np.array([[b[0][0], b[0][1], b[1][0], b[1][1]] for b in boxes])
