"""Frame scores without a GPU: the float64 restatement of pg_frame_metrics (tests/metrics_ref.py) against the reference's own values
(tests/golden/frame_metrics.npz: the vendored pytorch_msssim on cropped pairs; the literal numpy lines of run_render.py for the
PSNR), the constants compiled into the library, the host-side box and tile arithmetic under the sanitisers, and the refusals of
posegen_amd.evaluate."""
import os
import re
import subprocess
import types

import numpy as np
import pytest
import torch

from posegen_amd import _ffi, evaluate as ev
from tests import metrics_ref as ref

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# |restatement - reference float32 SSIM| over the fixture's 50 cases, measured on the CPU: worst 5.17e-6, at the single-window
# 11 x 11 box of set a (the reference's float32 E[x^2] - mu^2 over one window); the 12 x 11 box of set b 4.8e-6, every other
# box <= 3.5e-6 (the whole frames 1.8e-6 and below).
# The bound is 4 x the worst.
SSIM_WORST_MEASURED = 5.17e-6
SSIM_BOUND = 4 * SSIM_WORST_MEASURED
PSNR_ULPS = 4                       # float32 ulps of the PSNR value, relative: both sides are means of <= 3e4 squared float32 differences
F32_EPS = float(np.finfo(np.float32).eps)


@pytest.fixture(scope="module")
def golden():
    return dict(np.load(os.path.join(REPO, "tests", "golden", "frame_metrics.npz")))


def golden_cases(g):
    """(tag, frame, box index, use_bg, img, mask, bkgd, rgb, box, reference ssim) of every fixture case"""
    for tag in "ab":
        imgs, masks, bk, rgbs, boxes, vals = (g[f"{k}_{tag}"] for k in ("imgs", "masks", "bkgds", "rgbs", "boxes", "ssim"))
        for f in range(len(imgs)):
            for b, box in enumerate(boxes):
                for use_bg in (0, 1):
                    yield tag, f, b, use_bg, imgs[f], masks[f], bk[0], rgbs[f], box, float(vals[f, b, use_bg])


def test_the_taps_compiled_into_the_library_are_the_reference_gaussian_bit_for_bit(golden):
    taps = ref.header_taps()
    assert golden["taps"].dtype == np.float32 and taps.tobytes() == golden["taps"].tobytes()


def test_a_float32_division_by_255_is_the_float64_quotient_rounded_to_float32():
    """the kernel forms gt as one IEEE float32 division; run_render.py:912, 944 as a float64 quotient cast by astype: the same 256 values"""
    b = np.arange(256)
    assert np.array_equal((b / 255.).astype(np.float32), b.astype(np.float32) / np.float32(255))


def test_restatement_ssim_equals_the_reference_ssim_on_every_golden_box(golden):
    """Restatement `ssim / n_map` against `pytorch_msssim.SSIM(size_average=False)` on the cropped pair, every box with h, w >= 11,
    with and without backgrounds.  Measured worst deviation 5.17e-6 (the 11 x 11 box: one float32 window); bound 4 x that = 2.07e-5."""
    worst, n = 0.0, 0
    for tag, f, b, use_bg, img, mask, bk, rgb, box, want in golden_cases(golden):
        assert np.isfinite(want)
        s = ref.frame_sums(img, mask, bk, rgb, box, golden["taps"], bool(use_bg))
        assert s[4] == 3 * (box[2] - box[0] - 10) * (box[3] - box[1] - 10)
        dev = abs(s[5] / s[4] - want)
        print(f"{tag} frame {f} box {tuple(box)} bg {use_bg}: ssim {s[5] / s[4]:.9f} reference {want:.9f} deviation {dev:.2e}")
        assert dev <= SSIM_BOUND, (tag, f, b, use_bg, dev)
        worst, n = max(worst, dev), n + 1
    print(f"worst deviation {worst:.3e} over {n} cases")
    assert n == 50


def test_restatement_psnr_equals_the_literal_float32_lines_of_the_reference(golden):
    """run_render.py:947-948 and :958-960 evaluated as written, in float32, on the same crop"""
    for tag, f, b, use_bg, img, mask, bk, rgb, box, _ in golden_cases(golden):
        x0, y0, x1, y1 = box
        s = ref.frame_sums(img, mask, bk, rgb, box, golden["taps"], bool(use_bg))
        gt_cropped = ref.ground_truth(img, mask, bk, bool(use_bg))[y0:y1, x0:x1]
        rgb_cropped = rgb[y0:y1, x0:x1]
        mask_cropped = mask[:, :, None][y0:y1, x0:x1].astype(np.float32)
        se = np.square(gt_cropped - rgb_cropped)
        box_psnr = -10. * np.log10(se.mean())
        assert se.dtype == np.float32
        got = -10. * np.log10(s[1] / s[0])
        print(f"{tag} {f} {tuple(box)} bg {use_bg}: psnr {got:.7f} literal {float(box_psnr):.7f}")
        assert abs(got - float(box_psnr)) <= PSNR_ULPS * F32_EPS * abs(float(box_psnr))
        if mask_cropped.sum() >= 1:
            denom = (mask_cropped.sum() * 3.)
            fg_psnr = -10. * np.log10((se * mask_cropped).sum() / denom)
            assert s[2] == denom
            got = -10. * np.log10(s[3] / s[2])
            assert abs(got - float(fg_psnr)) <= PSNR_ULPS * F32_EPS * abs(float(fg_psnr))
        else:
            assert s[2] == 0 and s[3] == 0


def test_restatement_edge_cases(golden):
    g = golden
    img, mask, bk, rgb = g["imgs_a"][0], g["masks_a"][0], g["bkgds_a"][0], g["rgbs_a"][0]
    H, W = mask.shape
    # a box below the window: no map, the squared errors are there
    for box in ((2, 3, 12, 30), (5, 0, 40, 7)):
        s = ref.frame_sums(img, mask, bk, rgb, box, g["taps"])
        assert s[0] == 3 * (box[2] - box[0]) * (box[3] - box[1]) and s[1] > 0 and np.all(s[4:] == 0)
    # the frame against its own ground truth: se = 0 exactly, the map 1 everywhere
    same = ref.ground_truth(img, mask, bk, False)
    s = ref.frame_sums(img, mask, bk, same, (0, 0, W, H), g["taps"])
    assert s[1] == 0 and s[3] == 0 and abs(s[5] - s[4]) <= 1e-9 * s[4] and abs(s[7] - s[6]) <= 1e-9 * max(s[6], 1)
    # the constant white region: both variances cancel to the same number and the map is exactly 1 there
    white = (np.mgrid[0:H, 0:W][0] < H // 3) & (np.mgrid[0:H, 0:W][1] >= W - W // 3 - 13)
    ys, xs = np.where(white)
    assert (img[white] == 255).all() and (rgb[white] == 1).all()
    box = (xs.min(), ys.min(), xs.max() + 1, ys.max() + 1)
    s = ref.frame_sums(img, mask, bk, rgb, box, g["taps"])
    assert s[4] >= 3 and s[5] == s[4] and s[1] == 0
    # the masked variant weights a map value by the mask at its window's centre: one pixel set -> that pixel's three map values
    one = np.zeros_like(mask)
    one[20, 17] = 1
    s1 = ref.frame_sums(img, one, bk, rgb, (3, 4, 40, 33), g["taps"])
    x = rgb[4:33, 3:40].astype(np.float64)
    y = (img[4:33, 3:40] / 255.).astype(np.float32).astype(np.float64)
    assert s1[2] == 3 and s1[6] == 3 and abs(s1[7] - ref.ssim_map(x, y, g["taps"])[20 - 4 - 5, 17 - 3 - 5].sum()) < 1e-12


def test_scores_from_sums_follow_both_reference_functions():
    """box_scores (run_render.py:947-964) and the mapping's corner cases: a box below the window has NaN SSIM entries, a perfect
    frame's PSNR stays inf"""
    sums = np.array([[300., 3., 30., 0.6, 150., 120., 12., 9.],
                     [300., 0., 30., 0.0, 0., 0., 0., 0.],
                     [300., 3., 0., 0.0, 150., 120., 0., 0.]])
    s = ev.box_scores(sums)
    assert np.allclose(s["psnr"][0], 20.0) and np.allclose(s["ssim"][0], 0.8)
    assert np.allclose(s["fg_psnr"][0], -10 * np.log10(0.02)) and np.allclose(s["fg_ssim"][0], 0.75)
    assert s["psnr"][1] == np.inf and s["fg_psnr"][1] == np.inf and np.isnan(s["ssim"][1]) and np.isnan(s["fg_ssim"][1])
    assert np.isnan(s["fg_psnr"][2]) and np.isnan(s["fg_ssim"][2])          # (left out by evaluate_frames: no mask pixel)


def _fake_bank(device="cuda:0", HW=(36, 48), masks=True, bkgds=False):
    return types.SimpleNamespace(device=device, HW=HW, F=2, masks=object() if masks else None, bkgds=object() if bkgds else None,
                                 renderer=None, struct=None)


def test_refusals_name_their_reason_before_anything_is_launched():
    H, W = 36, 48
    with pytest.raises(NotImplementedError, match="no CPU path"):
        ev.FrameScorer(_fake_bank(device="cpu"))
    with pytest.raises(NotImplementedError, match="no CPU path"):
        ev.evaluate_metric(np.zeros((1, H, W, 3), np.float32), _fake_bank(device="cpu"), [0])
    with pytest.raises(NotImplementedError, match="no CPU path"):
        ev.evaluate_frames([None], (H, W, 50.0), 4096, {}, _fake_bank(device="cpu"), [0], kp=object())
    sc = ev.FrameScorer(_fake_bank())
    with pytest.raises(NotImplementedError, match="no CPU path"):                       # a frame that is not on the bank's device
        sc.score(0, torch.zeros(H, W, 3), 0, (0, 0, W, H))
    # a frame whose size is not the bank's (which any render_factor gives)
    with pytest.raises(ValueError, match="against a bank of 36 x 48"):
        sc.score(0, torch.zeros(H // 2, W // 2, 3), 0, (0, 0, W // 2, H // 2))
    with pytest.raises(ValueError, match="against a bank of 36 x 48"):
        ev.evaluate_metric(np.zeros((2, H, W + 1, 3), np.float32), _fake_bank(), [0, 1])
    with pytest.raises(ValueError, match="against a bank of 36 x 48"):
        ev.evaluate_frames([None], (H, W + 1, 50.0), 4096, {}, _fake_bank(), [0], kp=object())
    with pytest.raises(NotImplementedError, match="render_factor"):
        ev.evaluate_frames([None], (H, W, 50.0), 4096, {}, _fake_bank(), [0], kp=object(), render_factor=2)
    with pytest.raises(NotImplementedError, match="render_factor"):
        ev.evaluate_metric(np.zeros((1, H, W, 3), np.float32), _fake_bank(), [0], render_factor=2)
    with pytest.raises(NotImplementedError, match="eval_both"):
        ev.evaluate_metric(np.zeros((1, H, W, 3), np.float32), _fake_bank(), [0], eval_both=True)
    # PG_METRICS_BG without backgrounds, masked scores without masks
    with pytest.raises(ValueError, match="PG_METRICS_BG"):
        ev.FrameScorer(_fake_bank(), background=True)
    with pytest.raises(ValueError, match="PG_METRICS_BG"):
        ev.evaluate_frames([None], (H, W, 50.0), 4096, {}, _fake_bank(), [0], kp=object(), background=True)
    with pytest.raises(ValueError, match="without masks"):
        ev.FrameScorer(_fake_bank(masks=False))
    assert ev.FrameScorer(_fake_bank(bkgds=True)).flags == _ffi.PG_METRICS_BG and ev.FrameScorer(_fake_bank()).flags == 0
    assert ev.FrameScorer(_fake_bank(bkgds=True), background=False).flags == 0
    assert ev.FrameScorer(_fake_bank(masks=False), use_masks=False).sums().shape == (0, 8)


def test_header_binding_and_package_export_the_entry_point():
    import posegen_amd
    hdr = open(os.path.join(REPO, "include", "posegen_hip.h")).read()
    assert re.search(r"int pg_frame_metrics\(pg_handle\* h, void\* stream, const pg_image_bank\* bank, int32_t img_row, "
                     r"const int32_t box\[4\], const float\* rgb,\s+int flags, double\* sums\);", hdr)
    assert re.search(r"#define\s+PG_METRICS_BG\s+1\b", hdr) and _ffi.PG_METRICS_BG == 1
    assert re.search(r"#define\s+PG_ABI_VERSION\s+11\b", hdr)               # an added entry point does not move the version
    lib = _ffi.load_library()
    assert hasattr(lib, "pg_frame_metrics") and len(_ffi.PROTOTYPES["pg_frame_metrics"][1]) == 8
    assert posegen_amd.FrameScorer is ev.FrameScorer and posegen_amd.evaluate_frames is ev.evaluate_frames
    assert posegen_amd.evaluate_metric is ev.evaluate_metric
    # bad host arguments are refused before the handle is looked at for a device: a null handle is PG_EINVAL
    assert lib.pg_frame_metrics(None, None, None, 0, None, None, 0, None) == _ffi.PG_EINVAL


def test_box_and_tile_arithmetic_is_clean_under_address_and_ub_sanitizers(tmp_path):
    """pg_metrics_plan.h (what pg_frame_metrics decides about a box on the host and what its kernel runs per tile) as a stand-alone
    program with its own main: boxes from 1 pixel to four tiles and a halo along each axis, 1000 x 1000 and 1 x 4096.  Every box
    pixel owned by one tile, every map pixel computed once from pixels its tile stages, every slot inside the buffer and written
    once; box_ok against the frame for boxes around and beyond every edge."""
    clang = "/opt/rocm/lib/llvm/bin/clang++"
    if not os.path.exists(clang):
        pytest.skip("ROCm clang++ not found")
    exe = str(tmp_path / "metrics_plan_asan")
    csrc = os.path.join(REPO, "posegen_amd", "csrc")
    build = subprocess.run([clang, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                            "-fno-omit-frame-pointer", "-I", csrc, os.path.join(REPO, "tools", "sanitize", "metrics_plan_asan.cpp"),
                            "-o", exe], capture_output=True, text=True)
    if build.returncode != 0 and "sanitizer" in build.stderr.lower() and "cannot find" in build.stderr.lower():
        pytest.skip("sanitizer runtime not installed")
    assert build.returncode == 0, build.stderr[-2000:]
    run = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert run.returncode == 0, (run.stdout[-1500:], run.stderr[-3000:])
    assert "784 boxes clean under ASan/UBSan" in run.stdout
