"""Validation scores without a GPU: the float64 restatement of pg_frame_metrics_val (tests/metrics_ref.py) -- its upsampling
against torch's float64 F.interpolate and its own edge cases, its scores against the reference's values on torch's float32
upsampling (tests/golden/frame_metrics_val.npz) -- the mapping of evaluation_helpers.py:296-385 on hand-written sums, the refusals
of posegen_amd.evaluate's validation names, the header and the binding, and the resampling tables and 12-wide slots under the
sanitisers."""
import os
import re
import subprocess
import types

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from posegen_amd import _ffi, evaluate as ev
from tests import metrics_ref as ref

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# |restatement - reference float32 SSIM| over the fixture's 12 whole-frame cases, measured on the CPU: worst 5.294e-6 (50 x 37 from
# 16 x 12, without the background), the next 3.1e-6, every integer-ratio 36 x 48 case of frame 0 <= 2.5e-6.  The reference's side is
# float32 throughout: torch's float32 index arithmetic of the upsampling (off its own float64 result by up to 1.2e-5 at ratios that
# are not integers, and 50 / 16, 37 / 12 are the coarsest here), then float32 window sums.  The bound is 4 x the worst = 2.12e-5,
# which is 2 % above the in-box fixture's 2.07e-5 (tests/test_frame_metrics_ref.py: SSIM_BOUND) for that reason.
SSIM_VAL_WORST_MEASURED = 5.30e-6
SSIM_VAL_BOUND = 4 * SSIM_VAL_WORST_MEASURED
PSNR_ULPS = 4                       # float32 ulps of the PSNR value, relative (as tests/test_frame_metrics_ref.py)
F32_EPS = float(np.finfo(np.float32).eps)


@pytest.fixture(scope="module")
def golden():
    g = dict(np.load(os.path.join(REPO, "tests", "golden", "frame_metrics.npz")))
    g.update(np.load(os.path.join(REPO, "tests", "golden", "frame_metrics_val.npz")))
    return g


def golden_val_cases(g):
    """(tag, rf, frame, use_bg, img, mask, bkgd, lo, valid, reference ssim, reference (psnr, psnr_fg, psnr_valid))"""
    for tag in "ab":
        for rf in (2, 3):
            lo, ssim, psnr = (g[f"{k}_{tag}_rf{rf}"] for k in ("lo", "ssim", "psnr"))
            for f in range(len(lo)):
                for use_bg in (0, 1):
                    yield (tag, rf, f, use_bg, g[f"imgs_{tag}"][f], g[f"masks_{tag}"][f], g[f"bkgds_{tag}"][0], lo[f], g[f"valid_{tag}"],
                           float(ssim[f, use_bg]), psnr[f, use_bg])


def torch64(lo, H, W):
    t = torch.from_numpy(lo.astype(np.float64)).permute(2, 0, 1)[None]
    return F.interpolate(t, size=(H, W), mode="bilinear", align_corners=False)[0].permute(1, 2, 0).numpy()


def test_upsampling_to_the_same_size_is_the_frame_bit_for_bit():
    lo = np.random.RandomState(0).rand(37, 50, 3).astype(np.float32)
    lo[3, 4] = [0.0, 1.0, 1e-40]                                        # a zero, a one and a subnormal
    assert ref.up(lo, 37, 50).tobytes() == lo.tobytes()
    i0, i1, l1 = ref.axis_taps(37, 37)
    assert np.array_equal(i0, np.arange(37)) and np.all(l1 == 0)


def test_one_texel_along_an_axis_and_the_clamped_borders():
    rng = np.random.RandomState(1)
    row = rng.rand(1, 9, 3).astype(np.float32)                          # h_lo = 1: every output row is the row upsampled along x
    U = ref.up(row, 7, 20)
    assert all(U[y].tobytes() == U[0].tobytes() for y in range(7))
    col = rng.rand(9, 1, 3).astype(np.float32)                          # w_lo = 1: constant rows
    U = ref.up(col, 20, 7)
    assert all(U[:, x].tobytes() == U[:, 0].tobytes() for x in range(7))
    assert ref.up(row, 1, 9).tobytes() == row.tobytes()
    one = rng.rand(1, 1, 3).astype(np.float32)
    assert np.all(ref.up(one, 5, 6) == one[0, 0])
    # the first and last output rows / columns take the clamped texels: src < 0 -> texel 0 alone; the last texel blends with itself
    lo = rng.rand(18, 25, 3).astype(np.float32)
    U = ref.up(lo, 37, 50)
    for n_in, n_out in ((18, 37), (25, 50), (12, 37), (1, 4096), (500, 1000)):
        i0, i1, l1 = ref.axis_taps(n_in, n_out)
        assert i0[0] == 0 and l1[0] == 0 and i0[-1] == n_in - 1 and i1[-1] == n_in - 1
        assert i0.min() >= 0 and i1.max() <= n_in - 1 and np.all(np.diff(i0) >= 0) and np.all((l1 >= 0) & (l1 <= 1))
    assert U[0, 0].tobytes() == lo[0, 0].tobytes() and U[-1, -1].tobytes() == lo[-1, -1].tobytes()
    assert U[0, -1].tobytes() == lo[0, -1].tobytes() and U[-1, 0].tobytes() == lo[-1, 0].tobytes()
    assert np.array_equal(U[0], ref.up(lo[:1], 1, 50)[0]) and np.array_equal(U[:, -1:], ref.up(lo[:, -1:], 37, 1))


def test_the_restatement_is_torch_float64_interpolate_within_one_float32_rounding():
    """|up - F.interpolate(float64)| <= one float32 rounding of a value in [0, 1) -- half an ulp, 2^-25 = 2.98e-8 at most -- plus the
    double roundings of the two evaluations: each side rounds the scale, the source index, two weights, four products and three
    sums of values <= 1 -- 16 roundings of 2^-53 or less between them.  Measured worst: 2^-25 + 1.3e-15."""
    rng = np.random.RandomState(2)
    worst = 0.0
    for (h, w), (H, W) in (((18, 25), (37, 50)), ((12, 16), (37, 50)), ((18, 24), (36, 48)), ((37, 50), (75, 101)), ((25, 33), (75, 101)),
                           ((75, 50), (75, 101)), ((1, 101), (75, 101)), ((75, 1), (75, 101)), ((167, 167), (501, 501))):
        lo = rng.rand(h, w, 3).astype(np.float32)
        dev = np.abs(ref.up(lo, H, W).astype(np.float64) - torch64(lo, H, W)).max()
        print(f"{h} x {w} -> {H} x {W}: worst |up - torch float64| {dev:.3e}")
        worst = max(worst, dev)
        assert dev <= 2.0 ** -25 + 16 * 2.0 ** -53
    print(f"worst {worst:.3e}")


def test_restatement_scores_equal_the_reference_on_torch_float32_upsampling(golden):
    """`ssim / n_map` of the whole frame against `pytorch_msssim.SSIM(size_average=False)` on F.interpolate's float32 frame, and
    the three PSNR values against the literal float32 lines (evaluation_helpers.py:322-348).  Measured worst SSIM deviation
    5.294e-6, bound 4 x 5.30e-6 = 2.12e-5; PSNR 0.97 float32 ulps measured, bound 4."""
    worst, worst_ulps, n = 0.0, 0.0, 0
    for tag, rf, f, use_bg, img, mask, bk, lo, valid, want, psnr in golden_val_cases(golden):
        H, W = mask.shape
        assert lo.shape == (H // rf, W // rf, 3) and np.isfinite(want)
        s = ref.frame_sums_val(img, mask, bk, lo, (0, 0, W, H), golden["taps"], bool(use_bg), valid)
        assert s[4] == 3 * (W - 10) * (H - 10) and s[0] == 3 * H * W
        assert s[8] == 3 * (valid[2] - valid[0]) * (valid[3] - valid[1]) and s[2] == 3 * int((mask > 0).sum())
        dev = abs(s[5] / s[4] - want)
        got = [-10. * np.log10(s[1] / s[0]), -10. * np.log10(s[3] / s[2]), -10. * np.log10(s[9] / s[8])]
        ulps = max(abs(a - b) / (F32_EPS * abs(b)) for a, b in zip(got, psnr))
        print(f"{tag} rf {rf} frame {f} bg {use_bg}: ssim {s[5] / s[4]:.9f} reference {want:.9f} deviation {dev:.2e}; psnr {got[0]:.7f} "
              f"fg {got[1]:.7f} valid {got[2]:.7f} reference {psnr[0]:.7f} {psnr[1]:.7f} {psnr[2]:.7f} ({ulps:.2f} float32 ulps)")
        assert dev <= SSIM_VAL_BOUND, (tag, rf, f, use_bg, dev)
        assert ulps <= PSNR_ULPS, (tag, rf, f, use_bg, ulps)
        worst, worst_ulps, n = max(worst, dev), max(worst_ulps, ulps), n + 1
    print(f"worst ssim deviation {worst:.3e}, worst psnr deviation {worst_ulps:.2f} float32 ulps over {n} cases")
    assert n == 12
    assert {golden[f"lo_b_rf{rf}"].shape[1:3] for rf in (2, 3)} == {(25, 18), (16, 12)}           # 50 x 37: non-integer ratios


def test_valid_sums_of_the_restatement(golden):
    g = golden
    img, mask, bk, lo = g["imgs_a"][0], g["masks_a"][0], g["bkgds_a"][0], g["lo_a_rf2"][0]
    H, W = mask.shape
    box = (3, 4, 40, 33)
    s = ref.frame_sums_val(img, mask, bk, lo, box, g["taps"], False, box)           # valid = the box: the box's own sums
    assert s[8] == s[0] and s[9] == s[1]
    inner = (box[0] + 5, box[1] + 5, box[2] - 5, box[3] - 5)                          # ... and the map's pixels are its inner centres
    s = ref.frame_sums_val(img, mask, bk, lo, box, g["taps"], False, inner)
    assert s[10] == s[4] and s[11] == s[5]
    s = ref.frame_sums_val(img, mask, bk, lo, box, g["taps"], False, (41, 0, 48, 36))             # beside the box
    assert np.all(s[8:] == 0) and s[0] > 0
    s = ref.frame_sums_val(img, mask, bk, lo, box, g["taps"], False, (20, 17, 21, 18))            # one pixel: its three map values
    U = ref.up(lo, H, W)
    x = U[4:33, 3:40].astype(np.float64)
    y = ref.ground_truth(img, mask, bk, False)[4:33, 3:40].astype(np.float64)
    assert s[8] == 3 and s[10] == 3 and abs(s[11] - ref.ssim_map(x, y, g["taps"])[17 - 4 - 5, 20 - 3 - 5].sum()) < 1e-12
    assert np.all(ref.frame_sums_val(img, mask, bk, lo, box, g["taps"])[8:] == 0)                 # no valid rectangle


def test_scores_from_sums_follow_the_validation_mapping():
    """evaluation_helpers.py:296-385 on hand-written sums: eval_both on and off, a frame without mask pixels removed, inf -> 0,
    denominators max(., 1)"""
    #                 n     se  n_fg se_fg n_map ssim n_fg_map ssim_fg n_valid se_valid n_valid_map ssim_valid
    sums = np.array([[300., 3., 30., 0.6, 150., 120., 12., 9., 60., 0.6, 30., 24.],
                     [300., 6., 0., 0.0, 150., 100., 0., 0., 60., 1.2, 30., 12.],           # no mask pixel: removed
                     [300., 3., 30., 0.0, 150., 120., 0., 0., 0., 0.0, 0., 0.],             # a perfect foreground, no valid pixel
                     [300., 3., 60., 6.0, 150., 120., 24., 12., 120., 12., 60., 30.]])
    both = ev.validation_scores(sums, eval_both=True)
    fg_psnr = np.mean([-10 * np.log10(0.6 / 30), 0.0, -10 * np.log10(6.0 / 60)])          # frame 2: -10 log10(0) = inf -> 0
    fg_ssim = np.mean([9. / 12, 0. / 1, 12. / 24])                                         # frame 2: 0 / max(0, 1)
    valid_psnr = np.mean([-10 * np.log10(0.6 / 60), 0.0, -10 * np.log10(12. / 120)])       # frame 2: 0 / max(0, 1) -> inf -> 0
    valid_ssim = np.mean([24. / 30, 0.0, 30. / 60])
    assert np.isclose(both["psnr_fg"], fg_psnr, rtol=1e-14) and np.isclose(both["ssim_fg"], fg_ssim, rtol=1e-14)
    assert np.isclose(both["psnr"], valid_psnr, rtol=1e-14) and np.isclose(both["ssim"], valid_ssim, rtol=1e-14)
    fg = ev.validation_scores(sums, eval_both=False)
    assert fg["psnr"] == fg["psnr_fg"] == both["psnr_fg"] and fg["ssim"] == fg["ssim_fg"] == both["ssim_fg"]
    whole = ev.validation_scores(sums, use_masks=False)
    assert np.isclose(whole["psnr"], np.mean(-10 * np.log10(sums[:, 1] / 300)), rtol=1e-14) and np.isclose(whole["ssim"], np.mean(sums[:, 5] / 150))
    assert whole["psnr_fg"] is None and whole["ssim_fg"] is None
    perfect = sums[:1].copy()
    perfect[0, 1] = 0.0
    assert ev.validation_scores(perfect, use_masks=False)["psnr"] == 0.0                   # inf -> 0
    none = ev.validation_scores(sums[1:2], eval_both=True)                                # every frame removed
    assert none == {"psnr": None, "ssim": None, "psnr_fg": None, "ssim_fg": None}
    assert ev.validation_scores(np.zeros((0, 12)))["psnr"] is None
    with pytest.raises(ValueError, match="eval_both needs masks"):
        ev.validation_scores(sums, use_masks=False, eval_both=True)


def test_eight_sums_take_the_same_mapping_as_evaluate_metric_had():
    """`validation_scores` on FrameScorer's eight sums, which is what `evaluate_metric` returns: hand-written rows against
    evaluation_helpers.py:296-364 written out per frame here, with masks and without.  The one place where that function's own
    mapping differed -- no inf -> 0 on the unmasked SSIM mean -- cannot show: a frame below the window has n_map = ssim = 0, which
    is NaN with and without it."""
    #                 n     se  n_fg se_fg n_map ssim n_fg_map ssim_fg
    rows = {"normal": [300., 3., 30., 0.6, 150., 120., 12., 9.],
            "no mask pixel": [300., 6., 0., 0.0, 150., 100., 0., 0.],
            "perfect": [300., 0., 30., 0.0, 150., 150., 12., 12.],
            "below the window": [90., 1.8, 30., 0.9, 0., 0., 0., 0.]}
    nan, inf = float("nan"), float("inf")

    def reference(sums, masks):
        psnr = lambda mse: -10. * np.log10(mse) if mse > 0 else inf
        zero_inf = lambda v: 0. if v == inf else v
        if masks:
            kept = [r for r in sums if r[2] > 0]                                        # :296-305
            fg_psnr = [zero_inf(psnr(r[3] / max(r[2], 1.))) for r in kept]              # :325-328
            fg_ssim = [zero_inf(r[7] / max(r[6], 1.)) for r in kept]                    # :331-332, this project's masked SSIM
            fg_psnr, fg_ssim = (np.mean(v) if kept else None for v in (fg_psnr, fg_ssim))
            return {"psnr": fg_psnr, "ssim": fg_ssim, "psnr_fg": fg_psnr, "ssim_fg": fg_ssim}        # :361-364
        test_psnr = [zero_inf(psnr(r[1] / r[0])) for r in sums]                         # :348-349
        test_ssim = [r[5] / r[4] if r[4] > 0 else nan for r in sums]                    # :352-353: the mean of a map without pixels
        return {"psnr": np.mean(test_psnr) if sums else None, "ssim": np.mean(test_ssim) if sums else None, "psnr_fg": None, "ssim_fg": None}

    for names in (list(rows), ["normal", "no mask pixel", "perfect"], ["below the window"], ["no mask pixel"], []):
        sums = [rows[k] for k in names]
        for masks in (True, False):
            got = ev.validation_scores(np.asarray(sums, np.float64).reshape(-1, 8), use_masks=masks, eval_both=False)
            want = reference(sums, masks)
            print(names, "masks" if masks else "no masks", got, want)
            assert list(got) == ["psnr", "ssim", "psnr_fg", "ssim_fg"]
            for key in got:
                if want[key] is None:
                    assert got[key] is None, (names, masks, key)
                elif np.isnan(want[key]):
                    assert np.isnan(got[key]), (names, masks, key)
                else:
                    assert np.isclose(got[key], want[key], rtol=1e-14, atol=0), (names, masks, key, got[key], want[key])
    whole = ev.validation_scores(np.asarray([rows["normal"], rows["perfect"]]), use_masks=False)
    assert np.isclose(whole["psnr"], 10.0, rtol=1e-14) and np.isclose(whole["ssim"], 0.9, rtol=1e-14)       # (20 + 0) / 2, (0.8 + 1) / 2
    assert np.isnan(ev.validation_scores(np.asarray([rows["normal"], rows["below the window"]]), use_masks=False)["ssim"])
    with pytest.raises(ValueError, match="eval_both"):
        ev.validation_scores(np.asarray([rows["normal"]]), eval_both=True)
    with pytest.raises(ValueError, match="validation_scores"):
        ev.validation_scores(np.zeros((2, 9)))


def _fake_bank(device="cuda:0", HW=(36, 48), masks=True, bkgds=False):
    return types.SimpleNamespace(device=device, HW=HW, F=2, masks=object() if masks else None, bkgds=object() if bkgds else None,
                                 renderer=None, struct=None)


def test_refusals_name_their_reason_before_anything_is_launched():
    H, W = 36, 48
    lo = np.zeros((1, H // 2, W // 2, 3), np.float32)
    with pytest.raises(NotImplementedError, match="no CPU path"):
        ev.ValidationScorer(_fake_bank(device="cpu"))
    with pytest.raises(NotImplementedError, match="no CPU path"):
        ev.evaluate_validation(lo, _fake_bank(device="cpu"), [0])
    with pytest.raises(NotImplementedError, match="no CPU path"):
        ev.evaluate_testset([None], (H, W, 50.0), 4096, {}, _fake_bank(device="cpu"), [0], render_factor=2, kp=object())
    sc = ev.ValidationScorer(_fake_bank())
    with pytest.raises(NotImplementedError, match="no CPU path"):                       # a frame that is not on the bank's device
        sc.score(0, torch.zeros(H // 2, W // 2, 3), 0)
    for shape in ((H + 1, W, 3), (H, W + 1, 3), (0, W, 3), (H, W, 4), (H, W)):          # never downsampled, never empty
        with pytest.raises(ValueError, match="against a bank of 36 x 48"):
            sc.score(0, torch.zeros(shape), 0)
    with pytest.raises(ValueError, match="against a bank of 36 x 48"):
        ev.evaluate_validation(np.zeros((2, H, W + 1, 3), np.float32), _fake_bank(), [0, 1])
    with pytest.raises(ValueError, match="2 image indices for 1 frames"):
        ev.evaluate_validation(lo, _fake_bank(), [0, 1])
    with pytest.raises(ValueError, match="against a bank of 36 x 48"):
        ev.evaluate_testset([None], (H, W + 1, 50.0), 4096, {}, _fake_bank(), [0], kp=object())
    # eval_both needs the masks and the valid boxes
    with pytest.raises(ValueError, match="eval_both needs every frame's valid box"):
        ev.evaluate_validation(lo, _fake_bank(), [0], eval_both=True)
    with pytest.raises(ValueError, match="eval_both needs masks"):
        ev.evaluate_validation(lo, _fake_bank(), [0], valid_boxes=[(0, 0, 4, 4)], use_masks=False, eval_both=True)
    with pytest.raises(ValueError, match="eval_both needs masks"):
        ev.evaluate_testset([None], (H, W, 50.0), 4096, {}, _fake_bank(), [0], use_masks=False, kp=object())
    with pytest.raises(ValueError, match="is this function's own"):
        ev.evaluate_testset([None], (H, W, 50.0), 4096, {}, _fake_bank(), [0], kp=object(), boxes=object())
    # PG_METRICS_BG without backgrounds, masked scores without masks
    with pytest.raises(ValueError, match="PG_METRICS_BG"):
        ev.ValidationScorer(_fake_bank(), background=True)
    with pytest.raises(ValueError, match="PG_METRICS_BG"):
        ev.evaluate_validation(lo, _fake_bank(), [0], background=True)
    with pytest.raises(ValueError, match="PG_METRICS_BG"):
        ev.evaluate_testset([None], (H, W, 50.0), 4096, {}, _fake_bank(), [0], kp=object(), background=True)
    with pytest.raises(ValueError, match="without masks"):
        ev.ValidationScorer(_fake_bank(masks=False))
    assert ev.ValidationScorer(_fake_bank(bkgds=True)).flags == _ffi.PG_METRICS_BG and ev.ValidationScorer(_fake_bank()).flags == 0
    assert ev.ValidationScorer(_fake_bank(bkgds=True), background=False).flags == 0
    assert ev.ValidationScorer(_fake_bank(masks=False), use_masks=False).sums().shape == (0, 12)
    # the old names keep refusing what the new ones take
    with pytest.raises(NotImplementedError, match="render_factor"):
        ev.evaluate_metric(np.zeros((1, H, W, 3), np.float32), _fake_bank(), [0], render_factor=2)
    with pytest.raises(NotImplementedError, match="eval_both"):
        ev.evaluate_metric(np.zeros((1, H, W, 3), np.float32), _fake_bank(), [0], eval_both=True)


def test_header_binding_and_package_export_the_entry_point():
    import posegen_amd
    hdr = open(os.path.join(REPO, "include", "posegen_hip.h")).read()
    assert re.search(r"int pg_frame_metrics_val\(pg_handle\* h, void\* stream, const pg_image_bank\* bank, int32_t img_row, "
                     r"const int32_t box\[4\],\s+const float\* rgb, int32_t rgb_h, int32_t rgb_w, const int32_t valid\[4\] /\* or NULL \*/,\s+"
                     r"int flags, double\* sums /\* device float64 \[12\] \*/\);", hdr)
    assert re.search(r"#define\s+PG_ABI_VERSION\s+11\b", hdr) and _ffi.PG_ABI_VERSION == 11      # an added entry point does not move it
    plan = open(os.path.join(REPO, "posegen_amd", "csrc", "pg_metrics_plan.h")).read()
    assert re.search(r"constexpr int SUMS = 8;", plan) and re.search(r"constexpr int SUMS_VAL = 12;", plan)
    lib = _ffi.load_library()
    assert hasattr(lib, "pg_frame_metrics_val") and len(_ffi.PROTOTYPES["pg_frame_metrics_val"][1]) == 11
    assert len(ev.SUMS_VAL) == 12 and ev.SUMS_VAL == ref.SUMS_VAL and ev.SUMS == ref.SUMS and ev.SUMS_VAL[:8] == ev.SUMS
    assert posegen_amd.ValidationScorer is ev.ValidationScorer and posegen_amd.evaluate_validation is ev.evaluate_validation
    assert posegen_amd.evaluate_testset is ev.evaluate_testset
    # a null handle is refused before anything else
    assert lib.pg_frame_metrics_val(None, None, None, 0, None, None, 0, 0, None, 0, None) == _ffi.PG_EINVAL


def test_resampling_tables_and_wide_slots_are_clean_under_address_and_ub_sanitizers(tmp_path):
    """pg_metrics_plan.h's resample_tap / resample_blend / overlap / slot_offset at SUMS_VAL as a stand-alone program with its own main:
    every n_in <= n_out <= 130 plus 500 -> 1000 and 1 -> 4096 -- every tile's table entries name texels of the low-resolution
    axis, weights in [0, 1], i0 never runs backwards -- and every 12-wide slot inside its buffer and written once, the counts from
    the spans equal to the pixels counted one by one."""
    clang = "/opt/rocm/lib/llvm/bin/clang++"
    if not os.path.exists(clang):
        pytest.skip("ROCm clang++ not found")
    exe = str(tmp_path / "metrics_resample_asan")
    csrc = os.path.join(REPO, "posegen_amd", "csrc")
    build = subprocess.run([clang, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                            "-fno-omit-frame-pointer", "-I", csrc, os.path.join(REPO, "tools", "sanitize", "metrics_resample_asan.cpp"),
                            "-o", exe], capture_output=True, text=True)
    if build.returncode != 0 and "sanitizer" in build.stderr.lower() and "cannot find" in build.stderr.lower():
        pytest.skip("sanitizer runtime not installed")
    assert build.returncode == 0, build.stderr[-2000:]
    run = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert run.returncode == 0, (run.stdout[-1500:], run.stderr[-3000:])
    assert "8517 axis pairs and 722 boxes clean under ASan/UBSan" in run.stdout
