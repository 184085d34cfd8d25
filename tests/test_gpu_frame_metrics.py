"""pg_frame_metrics on the GPU, through the C ABI and through FrameScorer: every one of the eight sums against the float64 restatement
(tests/metrics_ref.py) -- the counts exactly, the four real sums within 1e-9 max(1, |sum|) -- and the mapped PSNR / SSIM against
the reference's values (tests/golden/frame_metrics.npz) within the bound of tests/test_frame_metrics_ref.py.

The 1e-9: kernel and restatement add at most 2e5 double terms of magnitude <= 1 in different orders (<= 2e5 x 1.1e-16 relative),
the window sums a few ulps more.  Frames are at most 320 x 200; a tile is 32 x 32 map pixels (42 x 42 box pixels)."""
import os
import types

import numpy as np
import pytest
import torch

from posegen_amd import _ffi, evaluate as ev
from tests import metrics_ref as ref
from tests.frame_metrics_gpu import DEV, abi_sums, assert_sums, make_bank, renderer, synthetic_frames  # noqa: F401 (renderer: a fixture)
from tests.test_frame_metrics_ref import F32_EPS, PSNR_ULPS, SSIM_BOUND, golden_cases

pytestmark = pytest.mark.gpu
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EINVAL = -1
TILE = 32
H, W = 200, 320


@pytest.fixture(scope="module")
def golden():
    return dict(np.load(os.path.join(REPO, "tests", "golden", "frame_metrics.npz")))


@pytest.fixture(scope="module")
def scene(renderer):
    """two 200 x 320 images with masks and a background on the device, their frames, and the taps"""
    imgs, masks, bkgds, rgbs, white = synthetic_frames(H, W, 2, 31)
    bank = make_bank(renderer, imgs, masks, bkgds)
    return types.SimpleNamespace(imgs=imgs, masks=masks, bkgds=bkgds, rgbs=rgbs, white=white, bank=bank, dev_rgbs=torch.from_numpy(rgbs).to(DEV),
                    taps=ref.header_taps())


BOXES = {
    "one window 11x11": (7, 9, 18, 20),
    "12x13": (30, 40, 42, 53),
    "below the window 10x40": (5, 5, 15, 45),
    "below the window 40x7": (50, 60, 90, 67),
    "map one pixel wider than a tile": (3, 2, 3 + TILE + 11, 2 + TILE + 10),
    "map one pixel taller than a tile": (60, 100, 60 + TILE + 10, 100 + TILE + 11),
    "map exactly a tile": (100, 50, 100 + TILE + 10, 50 + TILE + 10),
    "several ragged tiles": (11, 13, 11 + 131, 13 + 97),
    "top left corner": (0, 0, 50, 45),
    "top right corner": (270, 0, 320, 45),
    "bottom left corner": (0, 155, 50, 200),
    "bottom right corner": (270, 155, 320, 200),
    "the whole frame": (0, 0, W, H),
}


@pytest.mark.parametrize("name", list(BOXES))
@pytest.mark.parametrize("flags", [0, _ffi.PG_METRICS_BG])
def test_sums_equal_the_restatement(renderer, scene, name, flags):
    box, f = BOXES[name], 1 if "corner" in name else 0
    rc, got = abi_sums(renderer, scene.bank.struct, f, box, scene.dev_rgbs[f], flags)
    assert rc == 0, renderer.lib.pg_last_error(renderer.handle)
    want = ref.frame_sums(scene.imgs[f], scene.masks[f], scene.bkgds[0], scene.rgbs[f], box, scene.taps, bool(flags))
    assert_sums(got, want, ref.SUMS, name)
    if "below" in name:
        assert np.all(got[4:] == 0) and got[0] == 3 * (box[2] - box[0]) * (box[3] - box[1]) and got[1] > 0


def test_a_frame_with_an_odd_width(renderer, golden):
    """50 x 37: a row is 111 floats and 111 bytes, so a staging load that assumes alignment reads the neighbour row"""
    g = golden
    bank = make_bank(renderer, g["imgs_b"], g["masks_b"], g["bkgds_b"])
    rgb = torch.from_numpy(g["rgbs_b"][0]).to(DEV)
    for box in list(g["boxes_b"]) + [(0, 0, 37, 50), (36, 0, 37, 50), (0, 49, 37, 50), (13, 17, 36, 49)]:
        for flags in (0, 1):
            rc, got = abi_sums(renderer, bank.struct, 0, box, rgb, flags)
            assert rc == 0
            assert_sums(got, ref.frame_sums(g["imgs_b"][0], g["masks_b"][0], g["bkgds_b"][0], g["rgbs_b"][0], box, g["taps"], bool(flags)),
                        ref.SUMS, f"box {tuple(box)} flags {flags}")


def test_masks_empty_full_and_one_pixel_on_a_tile_seam(renderer, scene):
    """The masked SSIM weights a map value by the mask at its window's centre: one mask pixel at the centre of the last window of
    tile (0, 0) and one at the first of tile (1, 1) give exactly those six map values; a mask edge inside a neighbour's halo"""
    x0, y0 = 9, 6
    box = (x0, y0, x0 + 131, y0 + 97)
    empty = np.zeros((H, W), np.uint8)
    seam = empty.copy()
    seam[y0 + 5 + TILE - 1, x0 + 5 + TILE - 1] = 1
    seam[y0 + 5 + TILE, x0 + 5 + TILE] = 1
    stripe = empty.copy()
    stripe[:, :x0 + TILE + 4] = 1            # ends inside the halo that tile 0 stages of tile 1's pixels
    masks = np.stack([empty, np.ones_like(empty), seam, stripe])
    imgs = np.repeat(scene.imgs[:1], 4, 0)
    bank = make_bank(renderer, imgs, masks, scene.bkgds)
    for f, what in enumerate(("empty", "all ones", "seam pixels", "stripe")):
        for flags in (0, 1):
            rc, got = abi_sums(renderer, bank.struct, f, box, scene.dev_rgbs[0], flags)
            assert rc == 0
            want = ref.frame_sums(imgs[f], masks[f], scene.bkgds[0], scene.rgbs[0], box, scene.taps, bool(flags))
            assert_sums(got, want, ref.SUMS, f"{what} flags {flags}")
            if what == "empty":
                assert got[2] == 0 and got[3] == 0 and got[6] == 0 and got[7] == 0
            if what == "all ones":
                assert got[2] == got[0] and got[6] == got[4] and got[3] == got[1] and got[7] == got[5]
            if what == "seam pixels":
                assert got[2] == 6 and got[6] == 6


def test_the_ground_truth_itself_and_the_white_region(renderer, scene):
    """rgb = the ground truth: se = 0 exactly and every map value 1; a box of constant white in both: both variances cancel alike
    and the map is exactly 1"""
    for flags in (0, 1):
        same = ref.ground_truth(scene.imgs[0], scene.masks[0], scene.bkgds[0], bool(flags))
        rc, got = abi_sums(renderer, scene.bank.struct, 0, (0, 0, W, H), torch.from_numpy(same).to(DEV), flags)
        assert rc == 0 and got[1] == 0 and got[3] == 0
        assert abs(got[5] - got[4]) <= 1e-9 * got[4] and abs(got[7] - got[6]) <= 1e-9 * got[6] and got[6] > 0
    ys, xs = np.where(scene.white)
    box = (xs.min(), ys.min(), xs.max() + 1, ys.max() + 1)
    assert scene.white[box[1]:box[3], box[0]:box[2]].all() and box[2] - box[0] > TILE + 10
    rc, got = abi_sums(renderer, scene.bank.struct, 0, box, scene.dev_rgbs[0], 0)
    assert rc == 0 and got[1] == 0 and got[4] > 0 and got[5] == got[4]


def test_two_calls_give_identical_bytes_and_a_row_leaves_its_neighbour_alone(renderer, scene):
    sc = ev.FrameScorer(scene.bank, capacity=2)
    box = ((11, 13), (142, 110))
    sc.score(0, scene.dev_rgbs[0], 0, box)
    first = sc.sums().copy()
    sc.score(1, scene.dev_rgbs[1], 1, (0, 0, W, H))
    sc.score(2, scene.dev_rgbs[0], 0, box)                      # grows the tensor past its capacity of 2
    s = sc.sums()
    assert s.shape == (3, 8) and s[0].tobytes() == first[0].tobytes() == s[2].tobytes()
    assert_sums(s[1], ref.frame_sums(scene.imgs[1], scene.masks[1], scene.bkgds[0], scene.rgbs[1], (0, 0, W, H), scene.taps, True), ref.SUMS, "row 1")
    rc, again = abi_sums(renderer, scene.bank.struct, 0, (11, 13, 142, 110), scene.dev_rgbs[0], _ffi.PG_METRICS_BG)
    assert rc == 0 and again.tobytes() == first[0].tobytes()
    # without masks the kernel is told there is no foreground
    nm = ev.FrameScorer(scene.bank, use_masks=False, background=False)
    nm.score(0, scene.dev_rgbs[0], 0, box)
    want = ref.frame_sums(scene.imgs[0], None, None, scene.rgbs[0], (11, 13, 142, 110), scene.taps, False)
    assert_sums(nm.sums()[0], want, ref.SUMS, "no masks")


def test_bad_arguments_are_einval_and_leave_the_output_untouched(renderer, scene):
    r, st, rgb = renderer, scene.bank.struct, scene.dev_rgbs[0]
    bad_boxes = [(-1, 0, 20, 20), (0, -1, 20, 20), (0, 0, W + 1, 20), (0, 0, 20, H + 1), (20, 5, 20, 30), (5, 30, 20, 30), (30, 5, 20, 30)]
    for box in bad_boxes:
        rc, out = abi_sums(r, st, 0, box, rgb, 0)
        assert rc == EINVAL and np.all(out == -7.0), box
    for row in (-1, 2):
        rc, out = abi_sums(r, st, row, (0, 0, 20, 20), rgb, 0)
        assert rc == EINVAL and np.all(out == -7.0)
    rc, out = abi_sums(r, st, 0, (0, 0, 20, 20), rgb, 2)                  # an unknown flag
    assert rc == EINVAL and np.all(out == -7.0)
    nobg = _ffi.PgImageBank.from_buffer_copy(st)
    nobg.bkgds = None
    rc, out = abi_sums(r, nobg, 0, (0, 0, 20, 20), rgb, _ffi.PG_METRICS_BG)
    assert rc == EINVAL and np.all(out == -7.0) and b"PG_METRICS_BG" in r.lib.pg_last_error(r.handle)
    rc, out = abi_sums(r, nobg, 0, (0, 0, 20, 20), rgb, 0)                # ... and fine without the flag
    assert rc == 0 and out[0] == 1200
    wrong = _ffi.PgImageBank.from_buffer_copy(st)
    wrong.H = H + 1
    rc, out = abi_sums(r, wrong, 0, (0, 0, 20, 20), rgb, 0)
    assert rc == EINVAL and np.all(out == -7.0)
    with pytest.raises(ValueError, match="against a bank of 200 x 320"):
        ev.FrameScorer(scene.bank).score(0, rgb[:100], 0, (0, 0, 20, 20))
    with pytest.raises(NotImplementedError, match="no CPU path"):
        ev.FrameScorer(scene.bank).score(0, rgb.cpu(), 0, (0, 0, 20, 20))


def test_mapped_scores_equal_the_reference_values(renderer, golden):
    """FrameScorer -> box_scores on the golden frames: ssim against pytorch_msssim's float32 value within the CPU test's bound, psnr
    against the literal float32 lines of run_render.py:947-948, 958-960 within 4 float32 ulps"""
    g = golden
    banks = {t: make_bank(renderer, g[f"imgs_{t}"], g[f"masks_{t}"], g[f"bkgds_{t}"]) for t in "ab"}
    dev = {t: torch.from_numpy(g[f"rgbs_{t}"]).to(DEV) for t in "ab"}
    scorers = {(t, bg): ev.FrameScorer(banks[t], background=bool(bg)) for t in "ab" for bg in (0, 1)}
    cases = list(golden_cases(g))
    rows = []
    for tag, f, b, use_bg, *_ in cases:
        sc = scorers[(tag, use_bg)]
        rows.append((sc, sc.n_frames))
        sc.score(sc.n_frames, dev[tag][f], f, g[f"boxes_{tag}"][b])
    sums = {k: sc.sums() for k, sc in scorers.items()}
    worst = 0.0
    for (tag, f, b, use_bg, img, mask, bk, rgb, box, want), (sc, k) in zip(cases, rows):
        s = ev.box_scores(sums[(tag, use_bg)][k:k + 1])
        x0, y0, x1, y1 = box
        se = np.square(ref.ground_truth(img, mask, bk, bool(use_bg))[y0:y1, x0:x1] - rgb[y0:y1, x0:x1])
        mc = mask[y0:y1, x0:x1, None].astype(np.float32)
        psnr = float(-10. * np.log10(se.mean()))
        print(f"{tag} {f} {tuple(box)} bg {use_bg}: ssim {s['ssim'][0]:.9f} reference {want:.9f}; psnr {s['psnr'][0]:.7f} literal {psnr:.7f}")
        assert abs(s["ssim"][0] - want) <= SSIM_BOUND
        assert abs(s["psnr"][0] - psnr) <= PSNR_ULPS * F32_EPS * abs(psnr)
        if mc.sum() >= 1:
            fg = float(-10. * np.log10((se * mc).sum() / (mc.sum() * 3.)))
            assert abs(s["fg_psnr"][0] - fg) <= PSNR_ULPS * F32_EPS * abs(fg)
        worst = max(worst, abs(s["ssim"][0] - want))
    print(f"worst ssim deviation from the reference {worst:.3e}")


def test_evaluate_metric_on_whole_frames(renderer, scene):
    """evaluation_helpers.py:257-385 with box = the frame: means over the frames that have a mask pixel, denominators max(., 1)"""
    imgs = np.concatenate([scene.imgs, scene.imgs[:1]])
    masks = np.concatenate([scene.masks, np.zeros_like(scene.masks[:1])])         # the third image has no person in it
    bank = make_bank(renderer, imgs, masks)
    rgbs = np.concatenate([scene.rgbs, scene.rgbs[:1]])
    got = ev.evaluate_metric(rgbs, bank, [0, 1, 2])
    s = np.stack([ref.frame_sums(imgs[f], masks[f], None, rgbs[f], (0, 0, W, H), scene.taps) for f in range(2)])
    assert abs(got["psnr_fg"] - np.mean(-10 * np.log10(s[:, 3] / s[:, 2]))) <= 1e-9
    assert abs(got["ssim_fg"] - np.mean(s[:, 7] / s[:, 6])) <= 1e-9
    assert got["psnr"] == got["psnr_fg"] and got["ssim"] == got["ssim_fg"]
    whole = ev.evaluate_metric(torch.from_numpy(rgbs).to(DEV), bank, [0, 1, 2], use_masks=False)
    s = np.stack([ref.frame_sums(imgs[f], None, None, rgbs[f], (0, 0, W, H), scene.taps) for f in range(3)])
    assert abs(whole["psnr"] - np.mean(-10 * np.log10(s[:, 1] / s[:, 0]))) <= 1e-9 and abs(whole["ssim"] - np.mean(s[:, 5] / s[:, 4])) <= 1e-9
    assert whole["psnr_fg"] is None


def test_evaluate_frames_scores_in_the_sink_what_scoring_afterwards_gives(tmp_path):
    """Three 48 x 48 frames of the synthetic model: scored through the frame sink as they are rendered, and rendered to the device
    first and scored afterwards -- the same bytes; the score dict, its files, and the frame without a mask pixel left out"""
    from posegen_amd import PREC_BF16, surreal_config, synthetic as syn
    from posegen_amd.raycaster import HipRayCaster
    from posegen_amd.render import render_frames_device
    cfg = surreal_config(n_samples=32, n_importance=16)
    caster = HipRayCaster.from_weights(cfg, *syn.make_model(cfg, 0), device=DEV, precision=PREC_BF16)
    try:
        h = w = 48
        F = 3
        _, kps, skts = syn.make_pose(F, 3)
        c2ws, focals = syn.make_camera(F, h, w)
        imgs, masks, bkgds, _, _ = synthetic_frames(h, w, F, 5)
        masks[:] = 1
        masks[1] = 0                                                  # frame 1: no mask pixel in its box
        bank = make_bank(caster.renderer, imgs, masks, bkgds)
        kw = {"ray_caster": caster, "N_importance": cfg.n_importance, "N_samples": cfg.n_samples, "lindisp": False}
        args = (torch.tensor(c2ws), (h, w, focals), 4096, kw)
        rkw = dict(kp=torch.tensor(kps), skts=torch.tensor(skts), white_bkgd=True, ext_scale=cfg.ext_scale)
        scores = ev.evaluate_frames(*args, bank, [2, 1, 0], basedir=str(tmp_path), **rkw)
        rgbs, _, _, _, bboxes = render_frames_device(*args, **rkw)
        sc = ev.FrameScorer(bank)
        for k in range(F):
            sc.score(k, rgbs[k].contiguous(), [2, 1, 0][k], bboxes[k])
        per = ev.box_scores(sc.sums())
        keep = [0, 2]
        for key in ("psnr", "ssim", "fg_psnr", "fg_ssim"):
            assert len(scores[key]) == 2
            assert np.asarray(scores[key], np.float64).tobytes() == per[key][keep].tobytes(), key
        assert all(np.isfinite(scores["psnr"])) and all(0 < v < 60 for v in scores["psnr"])
        saved = np.load(str(tmp_path / "scores.npy"), allow_pickle=True).item()
        assert list(saved) == ["psnr", "ssim", "fg_psnr", "fg_ssim"] and saved["psnr"] == scores["psnr"]
        lines = open(str(tmp_path / "score_final.txt")).read().splitlines()
        assert [ln.split(":")[0] for ln in lines] == ["psnr", "ssim", "fg_psnr", "fg_ssim"]
        assert abs(float(lines[0].split(":")[1]) - np.mean(scores["psnr"])) < 1e-12
    finally:
        caster.renderer.close()
