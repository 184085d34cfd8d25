"""The frame front and back end's yardstick (tests/frame_ref.py), its table of geometries and the host side of pg_stage_frame_rays,
pinned without a GPU before tests/test_gpu_frame_edges.py measures the three frame kernels by them."""
import ctypes as C
import os
import re

import numpy as np
import pytest
import torch

from posegen_amd import _ffi
from tests import frame_ref as fr
from tests.helpers import load_golden

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
U = fr.U
ray_excess, unit_excess, compose_excess = fr.ray_excess, fr.unit_excess, fr.compose_excess


def _inputs():
    return [(c, fr.case_inputs(c)) for c in fr.CASES]


# ---- the restatement against the record ----------------------------------------------------------------------------------------
def test_box_rays_are_the_reference_fixtures_rays():
    g = load_golden("valid_rays")
    H, W = int(g["H"]), int(g["W"])
    worst = 0.0
    for i in range(len(g["c2ws"])):
        intr = fr.intrinsics32(H, W, g["focals"][i])
        r32 = fr.box_rays32(H, W, intr, g["c2ws"][i], g["boxes"][i], 0., 1.)
        assert len(r32) == int(g[f"n_valid_{i}"])
        assert np.array_equal(r32[:8, 0:3], g[f"rays_o_head_{i}"])
        assert np.array_equal(r32[:8, 3:6], g[f"rays_d_head_{i}"]) and np.array_equal(r32[-8:, 3:6], g[f"rays_d_tail_{i}"])
        r, c = fr.box_pixels(H, W, g["boxes"][i])
        assert np.array_equal((r * W + c)[:8], g[f"vid_head_{i}"]) and np.array_equal((r * W + c)[-8:], g[f"vid_tail_{i}"])
        worst = max(worst, ray_excess(r32, H, W, intr, g["c2ws"][i], g["boxes"][i]))
    print(f"float32 restatement vs float64 on the fixture: {4 * worst:.2f} u mag")
    assert worst <= 1.0


def test_float32_restatement_is_inside_the_bounds_on_every_case():
    worst_d = worst_v = 0.0
    for c, x in _inputs():
        if fr.n_rays(c, x["box"]) == 0:
            continue
        r32 = fr.box_rays32(c["H"], c["W"], x["intr"], x["c2w"], x["box"], 0., 1.)
        worst_d = max(worst_d, ray_excess(r32, c["H"], c["W"], x["intr"], x["c2w"], x["box"]))
        d = torch.from_numpy(r32[:, 3:6])
        vd = (d / torch.norm(d, dim=-1, keepdim=True)).numpy()          # the reference's own float32 normalisation
        worst_v = max(worst_v, unit_excess(np.concatenate([r32, vd], 1)))
    print(f"float32 restatement: direction {4 * worst_d:.2f} u mag of 4, unit direction {5 * worst_v:.2f} u |v| of 5")
    assert worst_d <= 1.0 and worst_v <= 1.0


def test_compose32_and_rgb8_are_the_scatter_and_uint8_lines_of_the_frame_test():
    """the lines of test_render_frame_equals_ray_level_path, in torch float32 on the host, on the frame64 fixture's values"""
    g = load_golden("frame64")
    H, W = int(g["H"]), int(g["W"])
    for i in range(len(g["boxes"])):
        box = g["boxes"][i]
        r, c = fr.box_pixels(H, W, box)
        vid = torch.from_numpy(r * W + c)
        assert len(vid) == int(g["n_valid"][i])
        rgb_map = torch.from_numpy(g["rgbs"][i].reshape(-1, 3))[vid] * 0.75
        acc_map = torch.from_numpy(g["accs"][i].reshape(-1))[vid]
        disp_map = torch.from_numpy(g["disps"][i].reshape(-1))[vid]
        for base in (1.0, 0.0):
            ref_rgb = torch.full((H * W, 3), base)
            ref_acc = torch.zeros(H * W)
            ref_rgb[vid] = rgb_map + (1. - acc_map[..., None]) * ref_rgb[vid]
            ref_acc[vid] = acc_map
            rgb, disp, acc = fr.compose32(H, W, box, rgb_map.numpy(), disp_map.numpy(), acc_map.numpy(), None, base)
            assert np.array_equal(rgb, ref_rgb.numpy()) and np.array_equal(acc, ref_acc.numpy())
            assert np.array_equal(disp.reshape(H, W)[r, c], disp_map.numpy()) and np.count_nonzero(disp) == np.count_nonzero(disp_map.numpy())
            q = (ref_rgb * 255.0).clamp(0, 255).to(torch.uint8)
            assert np.array_equal(fr.rgb8_of(rgb), q.numpy())
            assert compose_excess(rgb, H, W, box, (rgb_map.numpy(), disp_map.numpy(), acc_map.numpy()), None, base) <= 1.0
    assert fr.rgb8_of(np.array([np.nan, -1.0, 2.0, 1.0, 0.0], np.float32)).tolist() == [0, 0, 255, 255, 0]


# ---- the table holds what it claims --------------------------------------------------------------------------------------------
def _touches(c, box):
    (tlx, tly), (brx, bry) = box
    return {"left": tlx == 0, "top": tly == 0, "right": brx == c["W"] - 1, "bottom": bry == c["H"] - 1}


def test_the_table_holds_every_geometry_it_is_there_for():
    found = set()
    for c, x in _inputs():
        H, W, box = c["H"], c["W"], x["box"]
        n = fr.n_rays(c, box)
        t = _touches(c, box)
        if n == 0:
            found.add("empty")
            continue
        assert n >= 200, (c["name"], n)
        if not any(t.values()):
            found.add("interior")
        for edge, on in t.items():
            if on and sum(t.values()) == 1:
                found.add(edge)                         # this edge and no other
        if all(t.values()):
            found.add("whole")
        fx, fy, cx, cy = (float(v) for v in x["intr"])
        found.update(k for k, on in (("wide", W > H), ("tall", H > W), ("odd", H % 2 == 1 and W % 2 == 1 and c["center"] is None),
                                     ("fx != fy", fx != fy), ("rolled", c["roll"] != 0.)) if on)
        if c["center"] is not None and cx != int(cx) and cy != int(cy) and (cx, cy) != (W * 0.5, H * 0.5):
            found.add("off-centre")
        if H % 2 == 1 and W % 2 == 1 and c["center"] is None:
            assert cx - int(cx) == 0.5 and cy - int(cy) == 0.5, "W/2 is a half-integer while the box offset is int(W/2)"
    want = {"interior", "left", "top", "right", "bottom", "whole", "wide", "tall", "odd", "off-centre", "fx != fy", "rolled", "empty"}
    assert found == want, want - found
    # a rolled camera is rolled: its image x axis leaves the one of make_camera
    assert abs(float(fr.camera(roll=35.)[:3, 0] @ fr.camera()[:3, 0]) - np.cos(np.deg2rad(35.))) < 1e-6


def _vet(cyl, c2w, focal, what):
    cam, pix = fr.ring_points(cyl, c2w, focal)
    assert cam[:, 2].min() > 0, (what, "a ring point behind the camera")
    assert np.abs(pix).max() < 2.0 ** 30, what
    ext = np.concatenate([pix.min(0), pix.max(0)])
    assert np.abs(ext - np.round(ext)).min() > 1e-6, (what, "an extreme on a knife edge")


def test_box_inputs_allow_a_bitwise_comparison():
    """every ring point strictly in front of the camera, projected below 2^30, no extreme within 1e-6 pixel of an integer: the
    cases of the table and the GPU box test's random batch, which clips on every side and holds an empty box"""
    for c, x in _inputs():
        _vet(x["cyl"][0].numpy(), x["c2w"], c["focal"], c["name"])
    kps, c2ws, H, W, focal, center = fr.random_box_batch()
    cyls, boxes = fr.host_boxes(kps, c2ws, H, W, focal, center)
    for i in range(len(kps)):
        _vet(cyls[i], c2ws[i], focal, f"random pose {i}")
    assert len(kps) == 129
    n = (boxes[:, 2] - boxes[:, 0]).clip(0) * (boxes[:, 3] - boxes[:, 1]).clip(0)
    assert (n == 0).any() and (n > 0).sum() > 64
    live = boxes[n > 0]
    assert (live[:, 0] == 0).any() and (live[:, 1] == 0).any() and (live[:, 2] == W - 1).any() and (live[:, 3] == H - 1).any()
    assert ((live[:, 0] > 0) & (live[:, 1] > 0) & (live[:, 2] < W - 1) & (live[:, 3] < H - 1)).any()


# ---- the bounds are not vacuous ------------------------------------------------------------------------------------------------
def _synthetic_maps(n, seed=0):
    rng = np.random.RandomState(seed)
    return (rng.uniform(0, 1, (n, 3)).astype(np.float32), rng.uniform(0, 2, n).astype(np.float32), rng.uniform(0, 1, n).astype(np.float32))


def test_swapped_axes_and_a_shifted_box_leave_the_bounds():
    moved = {"cx/cy": 0, "fx/fy": 0, "H/W rays": 0, "H/W compose": 0, "box rays": 0, "box compose": 0}
    for c, x in _inputs():
        H, W, intr, c2w, box = c["H"], c["W"], x["intr"], x["c2w"], x["box"]
        if fr.n_rays(c, box) == 0:
            continue
        good = fr.box_rays32(H, W, intr, c2w, box, 0., 1.)
        assert ray_excess(good, H, W, intr, c2w, box) <= 1.0
        fb = fr.flat_box(box)
        moved["cx/cy"] += ray_excess(fr.box_rays32(H, W, intr[[0, 1, 3, 2]], c2w, box, 0., 1.), H, W, intr, c2w, box) > 1.0
        moved["fx/fy"] += ray_excess(fr.box_rays32(H, W, intr[[1, 0, 2, 3]], c2w, box, 0., 1.), H, W, intr, c2w, box) > 1.0
        # H and W swapped where the box's list is split into rows and columns: the transposed box's list read as this one's
        tb = (fb[0], fb[1], fb[0] + (fb[3] - fb[1]), fb[1] + (fb[2] - fb[0]))
        swapped = fr.box_rays32(max(H, W), max(H, W), intr, c2w, tb, 0., 1.)
        moved["H/W rays"] += ray_excess(swapped, H, W, intr, c2w, box) > 1.0
        for shift in ((1, 0, 1, 0), (0, 1, 0, 1)):
            sb = tuple(a + b for a, b in zip(fb, shift))
            if fr.clamp_box(H, W, sb)[2:] == fr.clamp_box(H, W, fb)[2:]:
                moved["box rays"] += ray_excess(fr.box_rays32(H, W, intr, c2w, sb, 0., 1.), H, W, intr, c2w, box) > 1.0
        maps = _synthetic_maps(fr.n_rays(c, box))
        bg = np.random.RandomState(1).uniform(0, 1, (H * W, 3)).astype(np.float32)
        assert compose_excess(fr.compose32(H, W, box, *maps, bg, 0.)[0], H, W, box, maps, bg, 0.) <= 1.0
        # H and W swapped in the split of a pixel id into row and column: the frame written W rows of H
        moved["H/W compose"] += compose_excess(fr.compose32(W, H, (fb[1], fb[0], fb[3], fb[2]), maps[0], maps[1], maps[2], bg, 0.)[0],
                                               H, W, box, maps, bg, 0.) > 1.0
        sb = (fb[0] - 1, fb[1], fb[2] - 1, fb[3]) if fb[0] > 0 else (fb[0] + 1, fb[1], fb[2] + 1, fb[3])
        if fr.clamp_box(H, W, sb)[2:] == fr.clamp_box(H, W, fb)[2:]:
            moved["box compose"] += compose_excess(fr.compose32(H, W, sb, *maps, bg, 0.)[0], H, W, box, maps, bg, 0.) > 1.0
    print(moved)
    assert all(v >= 1 for v in moved.values()), moved


# ---- header, prototype and the refusals of pg_stage_frame_rays -----------------------------------------------------------------
def test_stage_frame_rays_header_binding_and_refusals():
    hdr = open(os.path.join(REPO, "include", "posegen_hip.h")).read()
    assert re.search(r"\bint pg_stage_frame_rays\(pg_handle\* h, void\* stream, int H, int W, const float\* c2w, const float\* intrinsics, "
                     r"const int\* box,\s*float near, float far, float cam, int64_t ray_begin, int64_t ray_end, float\* rays /\*\[n,11\]\*/,"
                     r"\s*float\* cams /\*\[n\] or NULL\*/\);", hdr)
    assert re.search(r"#define\s+PG_ABI_VERSION\s+11\b", hdr) and _ffi.PG_ABI_VERSION == 11      # entry points are added, none moves
    assert "maps are read as those of the CLAMPED box" in hdr
    res, args = _ffi.PROTOTYPES["pg_stage_frame_rays"]
    assert res is C.c_int and args == [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.POINTER(C.c_float), C.POINTER(C.c_float),
                                       C.POINTER(C.c_int), C.c_float, C.c_float, C.c_float, C.c_int64, C.c_int64, C.c_void_p, C.c_void_p]
    from posegen_amd.raycaster import HipRenderer
    assert callable(HipRenderer.stage_frame_rays)
    integ = open(os.path.join(REPO, "INTEGRATION.md")).read()
    assert "| `pg_stage_frame_rays` (" in integ
    lib = _ffi.load_library()
    assert hasattr(lib, "pg_stage_frame_rays") and lib.pg_abi_version() == 11
    # the refusals come before anything looks for a device, in this order: null pointers, the range, the handle
    c2w = (C.c_float * 12)(1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0)
    intr = (C.c_float * 4)(10., 10., 4., 4.)
    box = (C.c_int * 4)(1, 2, 6, 20)                    # clamped to 5 x 6 = 30 rays in an 8 x 8 frame
    buf = (C.c_float * 16)()
    rays = C.cast(buf, C.c_void_p)
    call = lambda *a: lib.pg_stage_frame_rays(None, None, *a)
    err = lambda: lib.pg_last_error(None).decode()
    good = (8, 8, c2w, intr, box, 0.0, 1.0, -1.0, 0, 30, rays, None)
    assert call(*good) == _ffi.PG_EINVAL and err() == "null handle"
    for k in (2, 3, 4, 10):
        a = list(good)
        a[k] = None
        assert call(*a) == _ffi.PG_EINVAL and "null" in err() and "handle" not in err(), (k, err())
    for r0, r1 in ((0, 31), (-1, 4), (5, 4), (31, 31)):
        a = list(good)
        a[8], a[9] = r0, r1
        assert call(*a) == _ffi.PG_EINVAL and "outside the box of 30 rays" in err(), (r0, r1, err())
    for r0, r1 in ((0, 0), (30, 30), (7, 19)):          # inside the box: only the handle is missing
        a = list(good)
        a[8], a[9] = r0, r1
        assert call(*a) == _ffi.PG_EINVAL and err() == "null handle"
    a = list(good)
    a[0] = 0
    assert call(*a) == _ffi.PG_EINVAL and "non-positive" in err()


# ---- pg_plan_frames with frames that have no rays ------------------------------------------------------------------------------
def _plan(n_rays, workers, chunk):
    lib = _ffi.load_library()
    arr = (C.c_int64 * len(n_rays))(*n_rays)
    n = C.c_int()
    assert lib.pg_plan_frames(len(n_rays), arr, workers, chunk, None, 0, C.byref(n)) == 0
    out = (C.c_int32 * (5 * max(n.value, 1)))()
    assert lib.pg_plan_frames(len(n_rays), arr, workers, chunk, out, n.value, C.byref(n)) == 0
    return [tuple(out[5 * i:5 * i + 5]) for i in range(n.value)]      # (frame, r0, r1, worker, owner)


@pytest.mark.parametrize("G", [1, 2, 3])
def test_a_frame_without_rays_gets_one_whole_task(G):
    """a frame whose box is empty is still composed (it is the background): one task (f, 0, 0), worked and owned by one worker"""
    for n_rays, chunk in (([0], 256), ([0, 0, 0], 256), ([700, 0, 1300, 0], 256), ([0, 2769, 546, 0, 638], 256), ([0, 5000], 256),
                          ([700, 0, 1300, 0], 4096), ([0, 2769, 546, 0, 638], 4096)):
        tasks = _plan(n_rays, G, chunk)
        if max(n_rays) <= chunk:                    # no frame can be cut: exactly one task each
            assert sorted(t[0] for t in tasks) == list(range(len(n_rays)))
        for f, n in enumerate(n_rays):
            mine = [t for t in tasks if t[0] == f]
            assert sum(t[2] - t[1] for t in mine) == n and all(0 <= t[3] < G and 0 <= t[4] < G for t in mine)
            assert len({t[4] for t in mine}) == 1, "one owner per frame"
            if n == 0:
                assert len(mine) == 1 and mine[0][1:3] == (0, 0) and mine[0][3] == mine[0][4], (n_rays, G, mine)
            else:
                assert len(mine) >= 1 and sorted((t[1], t[2]) for t in mine)[0][0] == 0
