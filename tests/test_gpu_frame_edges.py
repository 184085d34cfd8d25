"""The frame front and back end off the square, centred, in-frame case: pose_boxes_kernel, frame_rays_kernel (pg_stage_frame_rays)
and frame_compose_kernel value by value against tests/frame_ref.py on the geometries of its table -- wide, tall and odd frames,
boxes clipped at each edge, the whole frame, an empty box, off-centre principal points, fx != fy, rolled cameras -- past the
4096 x 256 grid cap, and the chain render_frame / render_frames / render_frame_range + compose_frame / render_scene through them.
tests/test_frame_ref_host.py has pinned the yardstick and vetted the inputs.  Bounds in u = 2^-24, from the operation counts."""
import ctypes as C

import numpy as np
import pytest
import torch

from posegen_amd import _ffi, h36m_config, surreal_config, synthetic as syn
from tests import frame_ref as fr

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
CHUNK = 256                     # nanmean group: every box of the table spans several
LIVE = [c for c in fr.CASES if c["name"] != "empty"]
LIVE_IDS = [c["name"] for c in LIVE]
EMPTY = next(c for c in fr.CASES if c["name"] == "empty")
BIG = dict(H=1031, W=1021, focal=(987.5, 1011.25), center=(498.3, 521.7))         # 1 052 651 pixels > 4096 x 256


@pytest.fixture(scope="module")
def inputs():
    return {c["name"]: fr.case_inputs(c) for c in fr.CASES}


@pytest.fixture(scope="module")
def caster():
    from posegen_amd.raycaster import HipRayCaster
    cfg = surreal_config()
    c = HipRayCaster.from_weights(cfg, *syn.make_model(cfg, 0), device=DEV, precision="fp32")
    c.renderer.set_chunk(CHUNK)
    yield c
    c.renderer.close()


@pytest.fixture(scope="module")
def rend(caster):
    return caster.renderer


def _np(t):
    return t.detach().cpu().numpy()


def _same(a, b):
    """bitwise up to the payload of a NaN"""
    a, b = np.asarray(a), np.asarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and np.array_equal(a, b, equal_nan=a.dtype.kind == "f")


def _stage(rend, c, x, r0=None, r1=None, **kw):
    n = fr.n_rays(c, x["box"])
    return rend.stage_frame_rays(c["H"], c["W"], c["focal"], x["c2w"], x["box"], 0 if r0 is None else r0, n if r1 is None else r1,
                                 center=c["center"], **kw)


# ---- rays, value by value ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", LIVE, ids=LIVE_IDS)
def test_rays_of_a_box_value_by_value(rend, inputs, case):
    x = inputs[case["name"]]
    H, W = case["H"], case["W"]
    near, far = 0.25, 3.5
    rows = _np(_stage(rend, case, x, near=near, far=far))
    assert rows.shape == (fr.n_rays(case, x["box"]), 11)
    e_d = fr.ray_excess(rows, H, W, x["intr"], x["c2w"], x["box"], near, far)
    e_v = fr.unit_excess(rows)
    print(f"{case['name']}: direction {4 * e_d:.2f} u mag of 4, unit direction {5 * e_v:.2f} u |v| of 5 "
          f"(ratios {e_d:.3f}, {e_v:.3f})")
    assert np.array_equal(rows[:, :8], fr.box_rays32(H, W, x["intr"], x["c2w"], x["box"], near, far))
    assert e_d <= 1.0 and e_v <= 1.0


def test_frame_codes_ranges_and_empty_launches(rend, inputs):
    case = next(c for c in LIVE if c["name"] == "offcentre")
    x = inputs["offcentre"]
    n = fr.n_rays(case, x["box"])
    assert n > 257 + 1
    whole, cams = _stage(rend, case, x, cam=5.0, want_cams=True)
    assert cams.shape == (n,) and bool((cams == 5.0).all())
    assert bool((_stage(rend, case, x, want_cams=True)[1] == -1.0).all())          # no frame code: the mean code's index
    # cams NULL: nothing is written behind the rows (the caller's buffer holds a sentinel there)
    buf = torch.full((n * 11 + n + 64,), 7.25, device=DEV)
    c2w_h, intr, bx = rend._frame_args(case["H"], case["W"], case["focal"], x["c2w"], x["box"], case["center"])
    rend._check(rend.lib.pg_stage_frame_rays(rend.handle, rend._stream(), case["H"], case["W"], c2w_h.ctypes.data_as(C.POINTER(C.c_float)),
                                             intr, bx, 0.0, 1.0, 5.0, 0, n, C.c_void_p(buf.data_ptr()), None))
    assert torch.equal(buf[:n * 11].view(n, 11), whole) and bool((buf[n * 11:] == 7.25).all())
    # ranges: no alignment asked for
    parts = [_stage(rend, case, x, r0, r1, cam=5.0) for r0, r1 in ((0, 1), (1, 257), (257, n))]
    assert [p.shape[0] for p in parts] == [1, 256, n - 257] and torch.equal(torch.cat(parts), whole)
    # the empty range and the empty box launch nothing and return OK
    for r0 in (0, 100, n):
        rows, cm = _stage(rend, case, x, r0, r0, want_cams=True)
        assert rows.shape == (0, 11) and cm.shape == (0,)
    e = inputs["empty"]
    assert fr.n_rays(EMPTY, e["box"]) == 0 and _stage(rend, EMPTY, e).shape == (0, 11)
    for r0, r1 in ((0, n + 1), (-1, 5), (9, 8)):
        with pytest.raises(_ffi.PgError) as err:
            _stage(rend, case, x, r0, r1)
        assert err.value.code == _ffi.PG_EINVAL and "outside the box" in str(err.value)
    assert torch.equal(_stage(rend, case, x, cam=5.0), whole)                      # the handle works on


def test_rays_past_the_grid_cap(rend):
    """one whole frame of 1031 x 1021 = 1 052 651 rays: the rows the second trip of the grid-stride loop writes"""
    H, W = BIG["H"], BIG["W"]
    c2w = fr.camera((0.3, -0.2, 0.5), 20.)
    box = ((0, 0), (W, H))
    n = H * W
    assert n > 4096 * 256
    rows = _np(rend.stage_frame_rays(H, W, BIG["focal"], c2w, box, 0, n, center=BIG["center"]))
    intr = fr.intrinsics32(H, W, BIG["focal"], BIG["center"])
    want = fr.box_rays32(H, W, intr, c2w, box, 0., 1.)
    assert rows.shape == (n, 11) and np.array_equal(rows[:, :8], want)
    e_d, e_v = fr.ray_excess(rows, H, W, intr, c2w, box), fr.unit_excess(rows)
    print(f"1031 x 1021: direction {4 * e_d:.2f} u mag of 4, unit direction {5 * e_v:.2f} u |v| of 5 (ratios {e_d:.3f}, {e_v:.3f})")
    assert e_d <= 1.0 and e_v <= 1.0
    tail = _np(rend.stage_frame_rays(H, W, BIG["focal"], c2w, box, n - 5000, n, center=BIG["center"]))      # a range at the far end
    assert np.array_equal(tail, rows[n - 5000:])


# ---- compose, value by value ---------------------------------------------------------------------------------------------------
def _byte_edges():
    """float32 colours whose float32 product with 255 lands exactly on an integer k, on the nearest product below it and on the
    nearest above it (one ulp, where a colour reaches it; k = 0, 1, 37, 128, 254, 255) -- among them colours whose exact product
    lies on the other side of k"""
    out = []
    for k in (0, 1, 37, 128, 254, 255):
        cand = [np.float32(k / 255.0)]
        for _ in range(4):
            cand = [np.nextafter(cand[0], np.float32(-9.0))] + cand + [np.nextafter(cand[-1], np.float32(9.0))]
        cand = [v for v in cand if v == 0 or abs(v) >= 2.0 ** -100]                 # no denormals
        prod = np.array([np.float32(v * np.float32(255.0)) for v in cand])
        on = [v for v, p in zip(cand, prod) if p == k]
        below = [v for v, p in zip(cand, prod) if p == prod[prod < k].max()] if (prod < k).any() else []
        above = [v for v, p in zip(cand, prod) if p == prod[prod > k].min()] if (prod > k).any() else []
        assert on and (below or k == 0) and (above or k == 0), k
        for hits in (on, below, above):
            out += [hits[0], hits[-1]] if hits else []
    return np.array(out, dtype=np.float32)


def _maps(n, seed):
    """random maps of n rays with the edges planted at the front (as many as fit)"""
    rng = np.random.RandomState(seed)
    rgb = rng.uniform(-0.05, 1.05, (n, 3)).astype(np.float32)
    disp = rng.uniform(0.0, 3.0, n).astype(np.float32)
    acc = rng.uniform(0.0, 1.0, n).astype(np.float32)
    planted = np.concatenate([_byte_edges(), np.array([0.0, -0.0, 1.0, -0.25, 1.5, np.nan, 255.5 / 255.0], np.float32)])
    m = min(len(planted), n)
    rgb[:m] = np.roll(planted, seed)[:m, None] * np.ones(3, np.float32)             # acc = 1 there: the planted colour is the pixel
    acc[:m] = 1.0
    for k, a in enumerate((0.0, 1.0, 1.0 + 2.0 ** -23, 0.0, 1.0 + 2.0 ** -23)):
        if m + k < n:
            acc[m + k] = a
    disp[::7] = np.nan
    return rgb, disp, acc


def _compose_check(rend, H, W, box, seed, what):
    """every background form; -> (worst ratio to the 3u bound, bytes that differ from the float64 truncation)"""
    n = fr.clamp_box(H, W, box)[2] * fr.clamp_box(H, W, box)[3]
    maps = _maps(n, seed) if n else (None, None, None)
    t = [None if m is None else torch.from_numpy(m) for m in maps]
    worst, odd_bytes = 0.0, 0
    img = np.random.RandomState(100 + seed).uniform(-0.1, 1.1, (H * W, 3)).astype(np.float32)
    for bg, base in ((img, 0.0), (None, 0.0), (None, 1.0)):
        rgb, disp, acc, rgb8 = rend.compose_frame(H, W, box, *t, bg=None if bg is None else torch.from_numpy(bg), base_bg=base,
                                                  want_uint8=True)
        rgb, disp, acc, rgb8 = _np(rgb).reshape(-1, 3), _np(disp).reshape(-1), _np(acc).reshape(-1), _np(rgb8).reshape(-1, 3)
        w_rgb, w_disp, w_acc = fr.compose32(H, W, box, *maps, bg, base)
        assert _same(rgb, w_rgb), (what, "rgb", base)
        assert _same(disp, w_disp) and _same(acc, w_acc), (what, base)
        assert not np.isnan(disp).any()
        assert np.array_equal(rgb8, fr.rgb8_of(w_rgb)), (what, "rgb8", base)
        worst = max(worst, fr.compose_excess(rgb, H, W, box, maps, bg, base))
        odd_bytes += int((rgb8 != fr.rgb8_of64(rgb)).sum())
        inside = np.zeros(H * W, bool)
        r, c = fr.box_pixels(H, W, box)
        inside[r * W + c] = True
        assert not disp[~inside].any() and not acc[~inside].any()
        assert np.array_equal(rgb[~inside], fr._background(H, W, bg, base, np.float32)[~inside])
    print(f"compose {what}: worst {3 * worst:.2f} u of 3 (ratio {worst:.3f}); {odd_bytes} bytes differ from the float64 truncation")
    assert worst <= 1.0
    return worst, odd_bytes


@pytest.mark.parametrize("case", fr.CASES, ids=fr.CASE_IDS)
def test_compose_value_by_value(rend, inputs, case):
    """(the count of bytes that differ from the float64 truncation is printed, not asserted: fl32(k / 255) lies above k / 255 for
    every k, and the float32 colour below it multiplies to less than k - ulp / 2, so no planted colour rounds across an integer)"""
    x = inputs[case["name"]]
    _compose_check(rend, case["H"], case["W"], x["box"], fr.CASES.index(case), case["name"])


def test_compose_one_pixel_boxes_a_clamped_box_and_the_grid_stride(rend):
    H, W = 41, 75
    for k, (cx, cy) in enumerate(((0, 0), (W - 1, 0), (0, H - 1), (W - 1, H - 1))):
        _compose_check(rend, H, W, ((cx, cy), (cx + 1, cy + 1)), k, f"one pixel at ({cx}, {cy})")
    # a box that reaches outside the frame: the maps are those of the CLAMPED box, row-major with the clamped width
    for k, box in enumerate((((-3, -2), (W + 4, 17)), ((60, 30), (90, 50)), ((-5, 10), (20, H)))):
        assert fr.clamp_box(H, W, box) == ((0, 0, W, 17), (60, 30, 15, 11), (0, 10, 20, 31))[k]
        _compose_check(rend, H, W, box, 10 + k, f"clamped {box}")
    _compose_check(rend, BIG["H"], BIG["W"], ((100, 200), (900, 977)), 20, "1031 x 1021, interior box")


# ---- boxes ---------------------------------------------------------------------------------------------------------------------
def _flat(box):
    return list(fr.flat_box(box))


def test_pose_boxes_of_every_case_are_the_host_boxes(rend, inputs):
    for c in fr.CASES:
        x = inputs[c["name"]]
        cyl, box = rend.pose_boxes(torch.tensor(x["kps"]), x["c2w"][None], c["H"], c["W"], c["focal"], fr.EXT_SCALE, center=c["center"])
        assert np.array_equal(_np(cyl), x["cyl"].numpy()), c["name"]
        assert _np(box).tolist() == [_flat(x["box"])], (c["name"], _np(box), x["box"])


@pytest.mark.parametrize("n", [1, 63, 64, 65, 129])
def test_pose_boxes_random_batch(rend, n):
    """75 x 101, off-centre principal point, fx != fy, a shifted and rolled camera per pose; then one camera for all, given once
    (w2c_stride 0) and once per pose (stride 16)"""
    kps, c2ws, H, W, focal, center = fr.random_box_batch()
    kps, c2ws = kps[:n], c2ws[:n]
    h_cyl, h_box = fr.host_boxes(kps, c2ws, H, W, focal, center)
    cyl, box = rend.pose_boxes(torch.tensor(kps), c2ws, H, W, focal, fr.EXT_SCALE, center=center)
    assert np.array_equal(_np(cyl), h_cyl) and np.array_equal(_np(box), h_box)
    one = c2ws[min(2, n - 1)]
    s_cyl, s_box = fr.host_boxes(kps, np.repeat(one[None], n, 0), H, W, focal, center)
    a = rend.pose_boxes(torch.tensor(kps), one[None], H, W, focal, fr.EXT_SCALE, center=center)
    b = rend.pose_boxes(torch.tensor(kps), np.repeat(one[None], n, 0), H, W, focal, fr.EXT_SCALE, center=center)
    assert np.array_equal(_np(a[1]), s_box) and torch.equal(a[1], b[1]) and torch.equal(a[0], b[0]) and np.array_equal(_np(a[0]), s_cyl)


# ---- the chain, end to end, in fp32 --------------------------------------------------------------------------------------------
def _background(H, W, seed=0):
    return torch.rand(H * W, 3, generator=torch.Generator().manual_seed(seed))


def _ray_level_frame(rend, case, x, bg, cam=None):
    """kp_to_valid_rays on the host -> render_rays -> scatter: (rgb [H W,3], disp [H W], acc [H W]) on the device"""
    from posegen_amd.rays import kp_to_valid_rays
    H, W = case["H"], case["W"]
    rays, vids, cyls, boxes = kp_to_valid_rays([x["c2w"]], H, W, [case["focal"]], kps=torch.tensor(x["kps"]),
                                               centers=None if case["center"] is None else [case["center"]], ext_scale=fr.EXT_SCALE)
    assert _flat(boxes[0]) == _flat(x["box"])
    ro, rd = rays[0]
    n = ro.shape[0]
    vd = rd / torch.norm(rd, dim=-1, keepdim=True)
    rb = torch.cat([ro, rd, torch.zeros(n, 1), torch.ones(n, 1), vd], -1)
    ret = rend.render_rays(rb, torch.tensor(x["skts"]), cyls[:1], cams=None if cam is None else torch.full((n,), cam), want_alpha=False)
    rgb = bg.clone().to(DEV)
    disp, acc = torch.zeros(H * W, device=DEV), torch.zeros(H * W, device=DEV)
    vid = vids[0].to(DEV)
    rgb[vid] = ret["rgb_map"] + (1. - ret["acc_map"][..., None]) * rgb[vid]
    disp[vid] = torch.nan_to_num(ret["disp_map"], nan=0.0)
    acc[vid] = ret["acc_map"]
    return rgb, disp, acc


def _frame(rend, case, x, **kw):
    return rend.render_frame(case["H"], case["W"], case["focal"], x["c2w"], x["box"], torch.tensor(x["skts"]), x["cyl"],
                             center=case["center"], **kw)


@pytest.mark.parametrize("case", LIVE, ids=LIVE_IDS)
def test_render_frame_is_the_ray_level_route(rend, inputs, case):
    x = inputs[case["name"]]
    H, W = case["H"], case["W"]
    assert fr.n_rays(case, x["box"]) > CHUNK
    bg = _background(H, W)
    want = _ray_level_frame(rend, case, x, bg)
    rgb, disp, acc, rgb8 = _frame(rend, case, x, bg=bg, want_uint8=True)
    assert float(acc.max()) > 0.05, "a body was rendered"
    for k, a, b in (("rgb", rgb.view(-1, 3), want[0]), ("disp", disp.view(-1), want[1]), ("acc", acc.view(-1), want[2])):
        assert torch.equal(a, b), f"{case['name']} {k}: max diff {float((a - b).abs().max()):.2e}"
    assert np.array_equal(_np(rgb8).reshape(-1, 3), fr.rgb8_of(_np(rgb).reshape(-1, 3)))


def test_render_frame_with_a_frame_code_off_centre():
    from posegen_amd.raycaster import HipRayCaster
    cfg = h36m_config()
    c = HipRayCaster.from_weights(cfg, *syn.make_model(cfg, 2), device=DEV, precision="fp32")
    try:
        c.renderer.set_chunk(CHUNK)
        case = next(k for k in LIVE if k["name"] == "rolled")
        x = fr.case_inputs(case)
        bg = _background(case["H"], case["W"], 3)
        for cam in (3.0, None):
            want = _ray_level_frame(c.renderer, case, x, bg, cam=-1.0 if cam is None else cam)
            rgb, disp, acc = _frame(c.renderer, case, x, bg=bg, cam=cam)
            assert torch.equal(rgb.view(-1, 3), want[0]) and torch.equal(disp.view(-1), want[1]) and torch.equal(acc.view(-1), want[2])
    finally:
        c.renderer.close()


def test_render_frame_of_an_empty_box_is_the_background(rend, inputs):
    x = inputs["empty"]
    H, W = EMPTY["H"], EMPTY["W"]
    bg = _background(H, W, 1)
    for kw in ({"bg": bg}, {"base_bg": 1.0}, {"base_bg": 0.0}):
        want = bg.view(H, W, 3) if "bg" in kw else torch.full((H, W, 3), kw["base_bg"])
        for u8 in (False, True):
            out = _frame(rend, EMPTY, x, want_uint8=u8, **kw)
            assert len(out) == (4 if u8 else 3)
            assert torch.equal(out[0].cpu(), want) and not bool(out[1].any()) and not bool(out[2].any())
            if u8:
                assert np.array_equal(_np(out[3]), fr.rgb8_of(want.numpy()))


FOUR = [dict(H=40, W=72, focal=(36.5, 43.0), center=(30.7, 17.4), shift=(0., 0., 2.), roll=0., seed=5),
        dict(H=40, W=72, focal=(39.0, 39.0), center=(-30., 12.), shift=(0., 0., 0.), roll=0., seed=6),
        dict(H=40, W=72, focal=(45.0, 41.5), center=(41.2, 22.9), shift=(0.4, -0.3, 0.5), roll=25., seed=7),
        dict(H=40, W=72, focal=(33.0, 37.0), center=(36., 20.), shift=(2.0, 0., 0.), roll=-10., seed=8)]


def test_render_frames_on_two_workers_with_a_geometry_per_frame(rend):
    """four frames of different centres, focal pairs and cameras at 40 x 72, one of them empty, one cut between the workers:
    every array bitwise render_frame's, frame by frame"""
    from posegen_amd.dist import plan_tasks
    from posegen_amd.raycaster import HipRayCaster
    H, W = 40, 72
    xs = [fr.case_inputs({**c, "name": f"frame {i}"}) for i, c in enumerate(FOUR)]
    n_rays = [fr.n_rays(c, x["box"]) for c, x in zip(FOUR, xs)]
    assert n_rays[1] == 0 and min(n_rays[0], n_rays[2], n_rays[3]) > CHUNK
    tasks = plan_tasks(n_rays, 2, CHUNK)
    assert any(sum(1 for t in tasks if t[0] == f) > 1 for f in range(4)), "one frame is cut"
    assert sum(1 for t in tasks if t[0] == 1) == 1
    bg = _background(H, W, 2)
    cfg = surreal_config()
    ndev = torch.cuda.device_count()
    multi = HipRayCaster.from_weights(cfg, *syn.make_model(cfg, 0), device=DEV, precision="fp32", devices=list(range(ndev)) if ndev >= 2 else [0, 0])
    try:
        multi.renderer.set_chunk(CHUNK)
        got = multi.renderer.render_frames(H, W, [c["focal"] for c in FOUR], [x["c2w"] for x in xs], [x["box"] for x in xs],
                                           np.concatenate([x["skts"] for x in xs]), torch.cat([x["cyl"] for x in xs]),
                                           centers=[c["center"] for c in FOUR], bg=bg, want_uint8=True)
    finally:
        multi.renderer.close()
    for f, (c, x) in enumerate(zip(FOUR, xs)):
        want = _frame(rend, c, x, bg=bg, want_uint8=True)
        for k in range(4):
            assert _same(got[k][f], _np(want[k])), (f, k)
    assert float(got[2][0].max()) > 0.05 and not got[2][1].any() and np.array_equal(got[0][1].reshape(-1, 3), bg.numpy())


def test_frame_ranges_and_compose_are_render_frame_off_centre(rend, inputs):
    """the two halves at a non-square, off-centre case, and for a box given unclamped: pieces on group boundaries + compose_frame"""
    case = next(c for c in LIVE if c["name"] == "offcentre")
    x = inputs["offcentre"]
    H, W = case["H"], case["W"]
    bg = _background(H, W, 4)
    (tlx, tly), (brx, bry) = x["box"]
    for box in (x["box"], ((tlx, -3), (brx, H + 5))):
        _, _, bw, bh = fr.clamp_box(H, W, box)
        n = bw * bh
        cuts = [0, CHUNK, 2 * CHUNK, n]
        assert n > 2 * CHUNK
        args = (H, W, case["focal"], x["c2w"], box, torch.tensor(x["skts"]), x["cyl"])
        pieces = [rend.render_frame_range(*args, r0, r1, center=case["center"]).view(5, r1 - r0) for r0, r1 in zip(cuts, cuts[1:])]
        packed = torch.cat(pieces, 1)
        rgb_map = torch.cat([p[:3].reshape(-1, 3) for p in pieces])
        got = rend.compose_frame(H, W, box, rgb_map, packed[3], packed[4], bg=bg, want_uint8=True)
        want = rend.render_frame(*args, center=case["center"], bg=bg, want_uint8=True)
        for a, b in zip(got, want):
            assert torch.equal(a, b)
        assert float(want[2].max()) > 0.05


def test_a_one_person_scene_is_the_one_person_frame_off_the_square(rend, inputs):
    from posegen_amd.scene import ScenePerson, render_scene
    for name in ("rolled", "tall"):
        case = next(c for c in LIVE if c["name"] == name)
        x = inputs[name]
        bg = _background(case["H"], case["W"], 5)
        person = ScenePerson(torch.tensor(x["skts"][0]), x["cyl"][0], x["box"])
        got = render_scene(rend, case["H"], case["W"], case["focal"], x["c2w"], [person], center=case["center"], bg=bg, want_uint8=True)
        want = _frame(rend, case, x, bg=bg, want_uint8=True)
        for k, (a, b) in enumerate(zip(got, want)):
            assert torch.equal(a, b), f"{name} output {k}: max diff {float((a.float() - b.float()).abs().max()):.2e}"
        assert float(want[2].max()) > 0.05
