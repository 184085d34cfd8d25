"""pg_frame_metrics_val on the GPU, through the C ABI and through ValidationScorer / evaluate_validation / evaluate_testset: a frame
of the bank's size gives pg_frame_metrics' bytes; a low-resolution frame gives, bit for bit, what pg_frame_metrics gives on the
restatement's upsampled frame (tests/metrics_ref.py); all twelve sums against the float64 restatement -- the counts exactly, the
real sums within 1e-9 max(1, |sum|) -- and the mapped scores against the reference's values on torch's float32 upsampling
(tests/golden/frame_metrics_val.npz) within the bounds of tests/test_frame_metrics_val_ref.py.

The 1e-9 is tests/test_gpu_frame_metrics.py's, for its reason: kernel and restatement add at most 2.3e4 double terms of magnitude
<= 1 in different orders.  The bank is two 75 x 101 images: three tiles of 32 x 32 map pixels along each axis, the last ones ragged."""
import os
import types

import numpy as np
import pytest
import torch

from posegen_amd import _ffi, evaluate as ev
from tests import metrics_ref as ref
from tests.frame_metrics_gpu import DEV, abi_sums, abi_val, assert_sums, make_bank, renderer, synthetic_frames  # noqa: F401 (renderer: a fixture)
from tests.test_frame_metrics_val_ref import F32_EPS, PSNR_ULPS, SSIM_VAL_BOUND, golden_val_cases

pytestmark = pytest.mark.gpu
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EINVAL = -1
TILE = 32
H, W = 75, 101
LO_SHAPES = [(37, 50), (25, 33), (75, 50), (1, 101), (75, 1)]        # rf 2 with both ratios non-integer, rf 3, one axis only, one row, one column

BOXES = {
    "the whole frame": (0, 0, W, H),
    "one window 11x11": (7, 9, 18, 20),
    "below the window 10x40": (5, 5, 15, 45),
    "map exactly a tile": (20, 10, 20 + TILE + 10, 10 + TILE + 10),
    "map one pixel past a tile": (3, 2, 3 + TILE + 11, 2 + TILE + 11),
    "top left corner": (0, 0, 50, 45),
    "top right corner": (51, 0, W, 45),
    "bottom left corner": (0, 30, 50, H),
    "bottom right corner": (51, 30, W, H),
}
BOX3 = (11, 13, 95, 70)              # 84 x 57: three tiles by two, not starting at 0; tile seams at x = 43, 75 and y = 45
VALIDS = {
    "inside the box": (30, 25, 60, 50),
    "straddling it": (0, 0, 50, 40),
    "equal to it": BOX3,
    "disjoint from it": (0, 0, 11, 13),
    "narrower than the window": (40, 20, 45, 60),
    "edges on tile seams": (43, 45, 75, 70),
    "edges on the seams of the map's centres": (11 + 5 + TILE, 13 + 5 + TILE, 11 + 5 + 2 * TILE, 70),
    "reaching the frame's border": (50, 30, W, H),
    "the whole frame": (0, 0, W, H),
    "empty": (20, 20, 20, 40),
}


@pytest.fixture(scope="module")
def golden():
    g = dict(np.load(os.path.join(REPO, "tests", "golden", "frame_metrics.npz")))
    g.update(np.load(os.path.join(REPO, "tests", "golden", "frame_metrics_val.npz")))
    return g


@pytest.fixture(scope="module")
def scene(renderer):
    """two 75 x 101 images with masks and a background on the device, their full-size frames, low-resolution frames of every shape
    of LO_SHAPES (the area average of frame 0 where the shape is H // rf x W // rf, seeded noise otherwise), the restatement's
    upsampling of each on the host and on the device, and the taps"""
    imgs, masks, bkgds, rgbs, _ = synthetic_frames(H, W, 2, 41)
    rng = np.random.RandomState(43)
    lo = {(37, 50): ref.area_average(rgbs[0], 2), (25, 33): ref.area_average(rgbs[0], 3)}
    for shape in LO_SHAPES:
        lo.setdefault(shape, rng.rand(*shape, 3).astype(np.float32))
    assert all(lo[s].shape == s + (3,) for s in LO_SHAPES)
    U = {s: ref.up(lo[s], H, W) for s in LO_SHAPES}
    return types.SimpleNamespace(imgs=imgs, masks=masks, bkgds=bkgds, rgbs=rgbs, bank=make_bank(renderer, imgs, masks, bkgds),
                                 dev_rgbs=torch.from_numpy(rgbs).to(DEV), lo=lo, U=U, dev_lo={s: torch.from_numpy(v).to(DEV) for s, v in lo.items()},
                                 dev_U={s: torch.from_numpy(v).to(DEV) for s, v in U.items()}, taps=ref.header_taps())


@pytest.mark.parametrize("name", list(BOXES))
@pytest.mark.parametrize("flags", [0, _ffi.PG_METRICS_BG])
def test_a_frame_of_the_banks_size_gives_the_bytes_of_pg_frame_metrics(renderer, scene, name, flags):
    box, f = BOXES[name], 1 if "corner" in name else 0
    rc0, old = abi_sums(renderer, scene.bank.struct, f, box, scene.dev_rgbs[f], flags)
    rc1, new = abi_val(renderer, scene.bank.struct, f, box, scene.dev_rgbs[f], None, flags)
    assert rc0 == 0 and rc1 == 0, renderer.lib.pg_last_error(renderer.handle)
    assert new[:8].tobytes() == old.tobytes() and np.all(new[8:] == 0), (name, old, new)
    assert old[0] == 3 * (box[2] - box[0]) * (box[3] - box[1]) and old[1] > 0
    # ... and with a valid rectangle the eight stay those bytes
    rc2, val = abi_val(renderer, scene.bank.struct, f, box, scene.dev_rgbs[f], box, flags)
    assert rc2 == 0 and val[:8].tobytes() == old.tobytes() and val[8] == old[0]


@pytest.mark.parametrize("shape", LO_SHAPES, ids=[f"{h}x{w}" for h, w in LO_SHAPES])
def test_the_fused_upsampling_equals_scoring_the_upsampled_frame_bit_for_bit(renderer, scene, shape):
    """The eight sums of pg_frame_metrics_val on the low-resolution frame against pg_frame_metrics on the restatement's U uploaded
    as a full-size frame: the kernel's staged values are U's float32 bytes and everything behind staging is the same code.  Boxes
    that do not start at 0 and tile seams, where neighbouring tiles stage the same pixels of U."""
    for name, box in list(BOXES.items()) + [("three tiles by two", BOX3)]:
        for flags in (0, _ffi.PG_METRICS_BG):
            rc0, unfused = abi_sums(renderer, scene.bank.struct, 0, box, scene.dev_U[shape], flags)
            rc1, fused = abi_val(renderer, scene.bank.struct, 0, box, scene.dev_lo[shape], None, flags)
            assert rc0 == 0 and rc1 == 0, renderer.lib.pg_last_error(renderer.handle)
            assert fused[:8].tobytes() == unfused.tobytes(), (shape, name, flags, unfused, fused)
            assert np.all(fused[8:] == 0)
            rc2, val = abi_val(renderer, scene.bank.struct, 0, box, scene.dev_lo[shape], BOX3, flags)
            assert rc2 == 0 and val[:8].tobytes() == unfused.tobytes(), (shape, name, flags)


@pytest.mark.parametrize("shape", [(37, 50), (75, 101), (25, 33)], ids=["37x50", "75x101", "25x33"])
@pytest.mark.parametrize("box", [BOX3, BOXES["the whole frame"], BOXES["below the window 10x40"]], ids=["84x57", "whole", "below the window"])
def test_all_twelve_sums_equal_the_restatement(renderer, scene, shape, box):
    lo, dev_lo = (scene.rgbs[0], scene.dev_rgbs[0]) if shape == (H, W) else (scene.lo[shape], scene.dev_lo[shape])
    for what, valid in VALIDS.items():
        for flags in (0, _ffi.PG_METRICS_BG):
            rc, got = abi_val(renderer, scene.bank.struct, 0, box, dev_lo, valid, flags)
            assert rc == 0, renderer.lib.pg_last_error(renderer.handle)
            want = ref.frame_sums_val(scene.imgs[0], scene.masks[0], scene.bkgds[0], lo, box, scene.taps, bool(flags), valid)
            assert_sums(got, want, ref.SUMS_VAL, f"{shape} box {box} valid {what} flags {flags}")
            if what in ("disjoint from it", "empty") and box == BOX3:
                assert np.all(got[8:] == 0)
            if what == "equal to it" and box == BOX3:
                assert got[8] == got[0] and got[10] == got[4] == 3 * (84 - 10) * (57 - 10)


def test_mapped_scores_equal_the_reference_values(renderer, golden):
    """ValidationScorer on the golden low-resolution frames: ssim against pytorch_msssim's float32 value on torch's float32
    upsampling within the CPU test's bound, the three PSNR values against the literal float32 lines within 4 float32 ulps; and
    evaluate_validation's means over the same frames"""
    g = golden
    banks = {t: make_bank(renderer, g[f"imgs_{t}"], g[f"masks_{t}"], g[f"bkgds_{t}"]) for t in "ab"}
    scorers = {(t, bg): ev.ValidationScorer(banks[t], background=bool(bg)) for t in "ab" for bg in (0, 1)}
    cases = list(golden_val_cases(g))
    rows = []
    for tag, rf, f, use_bg, img, mask, bk, lo, valid, want, psnr in cases:
        sc = scorers[(tag, use_bg)]
        rows.append((sc, sc.n_frames))
        sc.score(sc.n_frames, torch.from_numpy(lo).to(DEV), f, valid)
    sums = {k: sc.sums() for k, sc in scorers.items()}
    worst = 0.0
    for (tag, rf, f, use_bg, img, mask, bk, lo, valid, want, psnr), (sc, k) in zip(cases, rows):
        s = sums[(tag, use_bg)][k]
        got = [-10. * np.log10(s[1] / s[0]), -10. * np.log10(s[3] / s[2]), -10. * np.log10(s[9] / s[8])]
        print(f"{tag} rf {rf} frame {f} bg {use_bg}: ssim {s[5] / s[4]:.9f} reference {want:.9f}; psnr {got} literal {psnr}")
        assert abs(s[5] / s[4] - want) <= SSIM_VAL_BOUND
        for a, b in zip(got, psnr):
            assert abs(a - b) <= PSNR_ULPS * F32_EPS * abs(b)
        worst = max(worst, abs(s[5] / s[4] - want))
    print(f"worst ssim deviation from the reference {worst:.3e}")
    assert len(cases) == 12
    # evaluate_validation on set a at rf 2: the means of the per-frame values, the valid pair in front with eval_both
    lo, valid = g["lo_a_rf2"], [g["valid_a"]] * 2
    s = np.stack([ref.frame_sums_val(g["imgs_a"][f], g["masks_a"][f], g["bkgds_a"][0], lo[f], (0, 0, 48, 36), g["taps"], True, valid[f]) for f in range(2)])
    both = ev.evaluate_validation(lo, banks["a"], [0, 1], valid_boxes=valid, eval_both=True, background=True)
    assert abs(both["psnr"] - np.mean(-10 * np.log10(s[:, 9] / s[:, 8]))) <= 1e-9 and abs(both["ssim"] - np.mean(s[:, 11] / s[:, 10])) <= 1e-9
    assert abs(both["psnr_fg"] - np.mean(-10 * np.log10(s[:, 3] / s[:, 2]))) <= 1e-9 and abs(both["ssim_fg"] - np.mean(s[:, 7] / s[:, 6])) <= 1e-9
    assert abs(both["psnr_fg"] - np.mean(g["psnr_a_rf2"][:, 1, 1])) <= PSNR_ULPS * F32_EPS * both["psnr_fg"]
    fg = ev.evaluate_validation(torch.from_numpy(lo).to(DEV), banks["a"], [0, 1], background=True)
    assert fg["psnr"] == fg["psnr_fg"] == both["psnr_fg"] and fg["ssim"] == fg["ssim_fg"] == both["ssim_fg"]
    whole = ev.evaluate_validation(lo, banks["a"], [0, 1], use_masks=False)
    s = np.stack([ref.frame_sums_val(g["imgs_a"][f], None, None, lo[f], (0, 0, 48, 36), g["taps"]) for f in range(2)])
    assert abs(whole["psnr"] - np.mean(-10 * np.log10(s[:, 1] / s[:, 0]))) <= 1e-9 and abs(whole["ssim"] - np.mean(s[:, 5] / s[:, 4])) <= 1e-9
    assert whole["psnr_fg"] is None
    assert abs(whole["ssim"] - np.mean(g["ssim_a_rf2"][:, 0])) <= SSIM_VAL_BOUND


def test_two_calls_give_identical_bytes_and_a_row_leaves_its_neighbour_alone(renderer, scene):
    sc = ev.ValidationScorer(scene.bank, capacity=2)
    lo, valid = scene.dev_lo[(37, 50)], ((30, 25), (60, 50))
    sc.score(0, lo, 0, valid, box=BOX3)
    first = sc.sums().copy()
    sc.score(1, scene.dev_lo[(25, 33)], 1)
    sc.score(2, lo, 0, valid, box=BOX3)                         # grows the tensor past its capacity of 2
    s = sc.sums()
    assert s.shape == (3, 12) and s[0].tobytes() == first[0].tobytes() == s[2].tobytes()
    assert_sums(s[1], ref.frame_sums_val(scene.imgs[1], scene.masks[1], scene.bkgds[0], scene.lo[(25, 33)], (0, 0, W, H), scene.taps, True), ref.SUMS_VAL, "row 1")
    assert np.all(s[1, 8:] == 0)
    rc, again = abi_val(renderer, scene.bank.struct, 0, BOX3, lo, (30, 25, 60, 50), _ffi.PG_METRICS_BG)
    assert rc == 0 and again.tobytes() == first[0].tobytes()
    # without masks the kernel is told there is no foreground
    nm = ev.ValidationScorer(scene.bank, use_masks=False, background=False)
    nm.score(0, lo, 0, valid, box=BOX3)
    want = ref.frame_sums_val(scene.imgs[0], None, None, scene.lo[(37, 50)], BOX3, scene.taps, False, (30, 25, 60, 50))
    assert_sums(nm.sums()[0], want, ref.SUMS_VAL, "no masks")


def test_bad_arguments_are_einval_and_leave_the_output_untouched(renderer, scene):
    r, st, lo = renderer, scene.bank.struct, scene.dev_lo[(37, 50)]
    good = (0, 0, 20, 20)

    def refused(*args, **kw):
        rc, out = abi_val(r, *args, **kw)
        assert rc == EINVAL and np.all(out == -7.0), (args, kw, rc, out)

    for box in [(-1, 0, 20, 20), (0, -1, 20, 20), (0, 0, W + 1, 20), (0, 0, 20, H + 1), (20, 5, 20, 30), (5, 30, 20, 30), (30, 5, 20, 30)]:
        refused(st, 0, box, lo, None, 0)                                   # everything pg_frame_metrics refuses
    for row in (-1, 2):
        refused(st, row, good, lo, None, 0)
    refused(st, 0, good, lo, None, 2)                                      # an unknown flag
    nobg = _ffi.PgImageBank.from_buffer_copy(st)
    nobg.bkgds = None
    refused(nobg, 0, good, lo, None, _ffi.PG_METRICS_BG)
    assert b"PG_METRICS_BG" in r.lib.pg_last_error(r.handle)
    wrong = _ffi.PgImageBank.from_buffer_copy(st)
    wrong.H = H + 1
    refused(wrong, 0, good, lo, None, 0)
    for hw in ((0, 50), (37, 0), (-1, 50), (H + 1, 50), (37, W + 1)):       # the frame's size: never empty, never downsampled
        refused(st, 0, good, lo, None, 0, hw=hw)
    assert b"no downsampling" in r.lib.pg_last_error(r.handle)
    for valid in [(-1, 0, 20, 20), (0, -1, 20, 20), (0, 0, W + 1, 20), (0, 0, 20, H + 1), (21, 5, 20, 30), (5, 31, 20, 30)]:
        refused(st, 0, good, lo, valid, 0)                                 # a malformed valid
    assert b"valid" in r.lib.pg_last_error(r.handle)
    rc, out = abi_val(r, nobg, 0, good, lo, (5, 5, 5, 5), 0)               # ... an empty one is fine, and so is the bank without the flag
    assert rc == 0 and out[0] == 1200 and np.all(out[8:] == 0)
    with pytest.raises(ValueError, match="against a bank of 75 x 101"):
        ev.ValidationScorer(scene.bank).score(0, scene.dev_rgbs[0].repeat(2, 1, 1), 0)
    with pytest.raises(NotImplementedError, match="no CPU path"):
        ev.ValidationScorer(scene.bank).score(0, lo.cpu(), 0)
    with pytest.raises(TypeError, match="contiguous float32"):
        ev.ValidationScorer(scene.bank).score(0, scene.dev_rgbs[0][:, ::2], 0)


def test_evaluate_testset_scores_in_the_sink_what_scoring_afterwards_gives():
    """Two 64 x 64 frames of the synthetic model at render_factor = 2: scored through the sink as they are rendered at 32 x 32, and
    rendered to the device first and scored afterwards with the same boxes -- the same dict, bit for bit.  At render_factor = 0 the
    valid sums under a frame's box are the in-box sums of evaluate_frames / FrameScorer: n and se as they are, the map's pair with
    the rectangle of the box's window centres (the box shrunk by 5 pixels)."""
    from posegen_amd import PREC_BF16, surreal_config, synthetic as syn
    from posegen_amd.raycaster import HipRayCaster
    from posegen_amd.rays import frame_boxes
    from posegen_amd.render import render_frames_device
    cfg = surreal_config(n_samples=32, n_importance=16)
    caster = HipRayCaster.from_weights(cfg, *syn.make_model(cfg, 0), device=DEV, precision=PREC_BF16)
    try:
        h = w = 64
        nf = 2
        _, kps, skts = syn.make_pose(nf, 3)
        c2ws, focals = syn.make_camera(nf, h, w)
        imgs, masks, bkgds, _, _ = synthetic_frames(h, w, nf, 5)
        masks[:] = 1                                                  # every box holds mask pixels: evaluate_frames leaves no frame out
        bank = make_bank(caster.renderer, imgs, masks, bkgds)
        kw = {"ray_caster": caster, "N_importance": cfg.n_importance, "N_samples": cfg.n_samples, "lindisp": False}
        args = (torch.tensor(c2ws), (h, w, focals), 4096, kw)
        rkw = dict(kp=torch.tensor(kps), skts=torch.tensor(skts), white_bkgd=True, ext_scale=cfg.ext_scale)
        idxs = [1, 0]
        scores = ev.evaluate_testset(*args, bank, idxs, render_factor=2, **rkw)
        rgbs, _, _, _, _ = render_frames_device(*args, render_factor=2, **rkw)
        assert tuple(rgbs.shape) == (nf, h // 2, w // 2, 3)
        _, bboxes, _ = frame_boxes(caster.renderer, args[0], h, w, focals, kps=rkw["kp"], ext_scale=cfg.ext_scale)
        after = ev.evaluate_validation(rgbs, bank, idxs, valid_boxes=bboxes, eval_both=True, background=None)
        print("evaluate_testset", scores, "afterwards", after)
        assert list(scores) == ["psnr", "ssim", "psnr_fg", "ssim_fg"]
        for key in scores:
            assert np.float64(scores[key]).tobytes() == np.float64(after[key]).tobytes(), key
        assert np.isfinite(scores["psnr"]) and 0 < scores["psnr"] < 60 and 0 < scores["ssim"] <= 1 and scores["psnr"] != scores["psnr_fg"]
        fg_only = ev.evaluate_testset(*args, bank, idxs, render_factor=2, eval_both=False, **rkw)
        assert fg_only["psnr"] == fg_only["psnr_fg"] == scores["psnr_fg"] and fg_only["ssim"] == scores["ssim_fg"]
        # render_factor = 0: the valid sums under the render's own boxes against the in-box sums
        full, _, _, _, bb0 = render_frames_device(*args, **rkw)
        inbox, val = ev.FrameScorer(bank), ev.ValidationScorer(bank)
        wide = 0
        for k in range(nf):
            (x0, y0), (x1, y1) = (int(v) for v in bb0[k][0]), (int(v) for v in bb0[k][1])
            assert (x0, y0, x1, y1) == tuple(int(v) for b in bboxes[k] for v in b)           # the boxes at the bank's size, both ways
            inbox.score(k, full[k].contiguous(), idxs[k], bb0[k])
            val.score(k, full[k].contiguous(), idxs[k], bb0[k])
            val.score(nf + k, full[k].contiguous(), idxs[k], (x0 + 5, y0 + 5, max(x1 - 5, x0 + 5), max(y1 - 5, y0 + 5)))
            wide += x1 - x0 >= 11 and y1 - y0 >= 11
        a, b = inbox.sums(), val.sums()
        for k in range(nf):
            assert b[k, 8] == a[k, 0] and abs(b[k, 9] - a[k, 1]) <= 1e-9 * max(1.0, a[k, 1])
            assert b[nf + k, 10] == a[k, 4] and abs(b[nf + k, 11] - a[k, 5]) <= 1e-9 * max(1.0, abs(a[k, 5]))
        assert wide >= 1
        at0 = ev.evaluate_testset(*args, bank, idxs, render_factor=0, **rkw)
        frames = ev.evaluate_frames(*args, bank, idxs, **rkw)
        assert len(frames["psnr"]) == nf and abs(at0["psnr"] - np.mean(frames["psnr"])) <= 1e-9 * at0["psnr"]
    finally:
        caster.renderer.close()
