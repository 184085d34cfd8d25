"""CPU tests of the regressor's input batches (posegen_amd/regressor_batches.py, csrc/pg_regressor.hip): the float64 restatement the
GPU tests compare the kernel with (tests/regressor_ref.py) against the two scipy.ndimage calls skimage's
`resize(..., anti_aliasing=True)` makes, the crop boxes against the numpy slice they stand for, the C ABI's surface, and the
refusal of a renderer that is not on a HIP device."""
import os
import re
import types

import numpy as np
import pytest
import torch

from posegen_amd import _ffi, regressor_batches as rb
from tests import regressor_ref as ref

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MEAN, STD = rb.IMG_NORM_MEAN, rb.IMG_NORM_STD
# (h, w) -> (Ry, Rx)
SHAPES = [((312, 312), (224, 224)), ((272, 272), (224, 224)), ((150, 190), (224, 224)), ((700, 520), (224, 224)),
          ((224, 224), (224, 224)), ((37, 41), (224, 224)), ((2, 3), (224, 224)), ((2048, 9), (224, 224)), ((449, 447), (224, 224)),
          ((225, 223), (224, 224)), ((1, 5), (16, 16)), ((64, 48), (16, 7))]


@pytest.mark.parametrize("hw,out", SHAPES, ids=[f"{h}x{w}-{a}x{b}" for (h, w), (a, b) in SHAPES])
def test_restatement_equals_the_two_scipy_calls(hw, out):
    """Sums of at most a few hundred float64 terms of size <= 3: 1e-11 (measured 4e-13)."""
    ndi = pytest.importorskip("scipy.ndimage")
    (h, w), (Ry, Rx) = hw, out
    u8 = np.random.default_rng(h * 10007 + w).integers(0, 256, (h, w, 3), dtype=np.uint8)
    v = ref.normalise(u8, MEAN, STD)
    assert -2.2 < v.min() and v.max() < 2.8
    sig = (0.0, ref.radius(h, Ry)[0], ref.radius(w, Rx)[0])
    want = ndi.zoom(ndi.gaussian_filter(v, sig, mode="mirror"), (1, Ry / h, Rx / w), order=1, mode="mirror", grid_mode=True)
    got = ref.resize(v, (Ry, Rx))
    assert want.shape == got.shape == (3, Ry, Rx)
    err = float(np.abs(got - want).max())
    print(f"{h} x {w} -> {Ry} x {Rx}: max |restatement - scipy| = {err:.2e}")
    assert err <= 1e-11


def test_restated_parts():
    assert [ref.mirror(i, 4) for i in range(-7, 9)] == [1, 0, 1, 2, 3, 2, 1, 0, 1, 2, 3, 2, 1, 0, 1, 2]
    assert [ref.mirror(i, 1) for i in (-3, 0, 5)] == [0, 0, 0] and [ref.mirror(i, 2) for i in (-2, -1, 0, 1, 2, 3)] == [0, 1, 0, 1, 0, 1]
    assert ref.radius(64, 16) == (1.5, 6) and ref.radius(48, 16) == (1.0, 4) and ref.radius(256, 16) == (7.5, 30)
    assert ref.radius(17, 16) == (0.03125, 0) and ref.radius(16, 16)[1] == 0 and ref.radius(5, 16) == (0.0, 0)
    for n, R in ((64, 16), (5, 16), (1, 16), (20, 16)):
        assert np.allclose(ref.gaussian_operator(n, R).sum(1), 1) and np.allclose(ref.sample_operator(n, R).sum(1), 1)
    assert np.array_equal(ref.sample_operator(7, 7), np.eye(7))                # identity: every sample on a pixel centre
    assert abs(ref.bound(312, 312, 224, MEAN, STD) - 30 * 2.0 ** -24 * (1 - 0.406) / 0.225) < 1e-18


# ---- the crop boxes ----------------------------------------------------------------------------------------------------------------

def _sliced_box(center, scale, H, W):
    """The box of the reference's crop, read off the slice itself: the lines of mpii_dataset.__getitem__ on an image whose pixels are
    their own (row, column), then the extent of what came out (None: nothing did)."""
    image = np.stack(np.meshgrid(np.arange(H), np.arange(W), indexing="ij"), -1)
    side = scale * 200
    xy1 = np.array(center, dtype=np.float64) - side / 2
    xy2 = np.array(center, dtype=np.float64) + side / 2
    xy1[0], xy2[0] = np.clip(xy1[0], 0, image.shape[0]), np.clip(xy2[0], 0, image.shape[1])
    xy1[1], xy2[1] = np.clip(xy1[1], 0, image.shape[1]), np.clip(xy2[1], 0, image.shape[0])
    crop = image[int(xy1[1]):int(xy2[1]), int(xy1[0]):int(xy2[0])]
    if crop.size == 0:
        return None
    assert np.array_equal(crop, image[crop[0, 0, 0]:crop[-1, -1, 0] + 1, crop[0, 0, 1]:crop[-1, -1, 1] + 1])
    return [crop[0, 0, 1], crop[0, 0, 0], crop[-1, -1, 1] + 1, crop[-1, -1, 0] + 1]


BOX_CASES = [
    # (center (x, y), scale, (H, W))
    ((30.0, 20.0), 0.1, (40, 70)), ((20.0, 30.0), 0.1, (70, 40)), ((35.5, 20.25), 0.123, (40, 70)),        # inside
    ((3.0, 20.0), 0.1, (40, 70)), ((66.0, 20.0), 0.1, (40, 70)), ((30.0, 4.0), 0.1, (40, 70)), ((30.0, 37.0), 0.1, (40, 70)),  # each border
    ((3.0, 3.0), 0.5, (40, 70)), ((35.0, 20.0), 2.0, (40, 70)),                                                # corners, everything
    ((60.0, 20.0), 0.1, (40, 70)),          # wide image: the left edge 50 is clipped to H = 40
    ((30.0, 60.0), 0.1, (70, 40)),          # tall image: the top edge 50 is clipped to W = 40
    ((20.0, 55.0), 0.2, (70, 40)),          # tall image: the bottom edge 75 stops at H = 70, the top 35 stays
    ((55.0, 30.0), 0.2, (40, 70)),          # wide image: the left edge 35 stays below H = 40, the bottom 50 is clipped to H
]
EMPTY_CASES = [((30.5, 20.5), 0.001, (40, 70)), ((-30.0, 20.0), 0.1, (40, 70)), ((30.0, 100.0), 0.1, (40, 70)),
               ((30.0, 39.5), 0.004, (40, 70))]


def test_mpii_crop_boxes_are_the_reference_slices():
    want = [_sliced_box(c, s, H, W) for c, s, (H, W) in BOX_CASES]
    assert all(b is not None for b in want)
    got = rb.mpii_crop_boxes([c for c, _, _ in BOX_CASES], [s for _, s, _ in BOX_CASES], [hw for _, _, hw in BOX_CASES])
    assert got.dtype == np.int32 and got.shape == (len(BOX_CASES), 4)
    assert np.array_equal(got, np.array(want)), (got.tolist(), want)
    assert want[9][0] == 40 and want[10][1] == 40 and want[11][1::2] == [35, 70]       # the swapped clips were met
    # a random sweep over both orientations, empty crops included
    rng = np.random.default_rng(7)
    n_empty = 0
    for _ in range(300):
        H, W = ((40, 70), (70, 40))[int(rng.integers(2))]
        c, s = rng.uniform(-10, 80, 2), float(rng.uniform(0.01, 0.4))
        box = _sliced_box(c, s, H, W)
        if box is None:
            n_empty += 1
            with pytest.raises(ValueError, match="item 0"):
                rb.mpii_crop_boxes([c], [s], [(H, W)])
        else:
            assert rb.mpii_crop_boxes([c], [s], [(H, W)])[0].tolist() == box
    assert 10 < n_empty < 290


@pytest.mark.parametrize("case", range(len(EMPTY_CASES)))
def test_an_empty_mpii_crop_is_a_value_error_naming_the_item(case):
    c, s, hw = EMPTY_CASES[case]
    assert _sliced_box(c, s, *hw) is None
    ok = BOX_CASES[0]
    with pytest.raises(ValueError, match=r"mpii_crop_boxes: item 1: the crop .* is empty"):
        rb.mpii_crop_boxes([ok[0], c], [ok[1], s], [ok[2], hw])


def test_fixed_crop_boxes():
    b = rb.fixed_crop_boxes(3, 120, 392)
    assert b.dtype == np.int32 and b.tolist() == [[120, 120, 392, 392]] * 3
    image = np.arange(512 * 512).reshape(512, 512)
    x0, y0, x1, y1 = rb.fixed_crop_boxes(1, 100, 412)[0]
    assert np.array_equal(image[y0:y1, x0:x1], image[100:412, 100:412])
    assert rb.fixed_crop_boxes(0, 1, 2).shape == (0, 4)
    with pytest.raises(ValueError):
        rb.fixed_crop_boxes(2, 5, 5)


# ---- surface and refusals ----------------------------------------------------------------------------------------------------------

def test_the_entry_point_is_declared_exported_and_bound():
    hdr = open(os.path.join(REPO, "include", "posegen_hip.h")).read()
    assert re.search(r"\bint pg_regressor_input\(pg_handle\* h, void\* stream, const uint8_t\* pixels, int64_t n_bytes,", hdr)
    assert re.search(r"typedef struct pg_crop_item \{ int64_t offset; int32_t H, W, x0, y0, x1, y1; \} pg_crop_item;", hdr)
    assert re.search(r"#define\s+PG_ABI_VERSION\s+11\b", hdr) and _ffi.PG_ABI_VERSION == 11          # an added entry point does not move it
    res, args = _ffi.PROTOTYPES["pg_regressor_input"]
    assert res is _ffi.C.c_int and len(args) == 10
    assert _ffi.C.sizeof(_ffi.PgCropItem) == 32 and _ffi.PgCropItem.H.offset == 8 and _ffi.PgCropItem.y1.offset == 28
    assert hasattr(_ffi.load_library(), "pg_regressor_input")
    import posegen_amd
    for name in ("PixelStore", "RegressorBatchSource", "regressor_input", "fixed_crop_boxes", "mpii_crop_boxes", "REFERENCE_NORM"):
        assert getattr(posegen_amd, name) is getattr(rb, name)
    assert rb.REFERENCE_NORM == (rb.IMG_NORM_MEAN, rb.IMG_NORM_MEAN) and rb.regressor_input.__defaults__[1:3] == (MEAN, STD)
    mk = open(os.path.join(REPO, "posegen_amd", "csrc", "Makefile")).read()
    assert re.search(r"^SRCS_HIP := .*\bpg_regressor\.hip\b", mk, re.M) and "pg_regressor.s 3pgr" in mk


class _Lib:
    def __init__(self, log):
        self.log = log

    def __getattr__(self, name):
        def call(*a):
            self.log.append(name)
            return 0
        return call


class FakeRenderer:
    def __init__(self, device="cpu"):
        self.device = torch.device(device)
        self.log = []
        self.lib = _Lib(self.log)
        self.handle = None

    def _check(self, rc):
        self.log.append("check")

    def _stream(self):
        self.log.append("stream")
        return None


def test_a_renderer_off_the_device_is_refused():
    r = FakeRenderer("cpu")
    with pytest.raises(NotImplementedError, match=r"PixelStore: the renderer is on cpu, not on a HIP device \(torch 'cuda:N'\)"):
        rb.PixelStore(r, [np.zeros((4, 4, 3), np.uint8)])
    with pytest.raises(NotImplementedError, match=r"PixelStore: the renderer is on cpu"):
        rb.PixelStore(r)
    store = types.SimpleNamespace(renderer=r, device=r.device, sizes=np.full((2, 2), 8, np.int32), offsets=np.array([0, 192]))
    with pytest.raises(NotImplementedError, match=r"RegressorBatchSource: the renderer is on cpu, not on a HIP device"):
        rb.RegressorBatchSource(store, rb.fixed_crop_boxes(2, 0, 8), torch.zeros(2, 24, 3), batch_size=2)
    assert r.log == []
