"""What tests/test_gpu_frame_metrics.py and tests/test_gpu_frame_metrics_val.py share: the renderer fixture (imported by name into
both modules), banks and frames to score, both entry points through the C ABI, and the comparison of sums with the float64
restatement (tests/metrics_ref.py)."""
import ctypes as C

import numpy as np
import pytest
import torch

DEV = "cuda:0"


@pytest.fixture(scope="module")
def renderer():
    from posegen_amd import surreal_config
    from posegen_amd.raycaster import HipRenderer
    r = HipRenderer(surreal_config(), device=DEV)          # no weights loaded: the entry point needs none
    yield r
    r.close()


def make_bank(renderer, imgs, masks, bkgds=None):
    """a DeviceImageBank of imgs [F,H,W,3], masks [F,H,W] and backgrounds [n,H,W,3] (all images use background 0)"""
    from posegen_amd.batches import DeviceImageBank
    F, h, w = masks.shape
    c2ws = np.tile(np.eye(4, dtype=np.float32)[None], (F, 1, 1))
    return DeviceImageBank(renderer, imgs.reshape(F, h * w, 3), masks.reshape(F, h * w, 1), masks.reshape(F, h * w, 1), c2ws,
                           np.full(F, 100.0, np.float32), (h, w), bkgds=None if bkgds is None else bkgds.reshape(len(bkgds), h * w, 3),
                           bkgd_idxs=None if bkgds is None else np.zeros(F, np.int32))


def synthetic_frames(h, w, F, seed):
    """uint8 images, elliptic masks, one background and float32 'rendered' frames: ground truth plus noise, a region that is
    constant white in both (rows < h/3, the right third and 13 columns: windows that see nothing else)"""
    rng = np.random.RandomState(seed)
    yy, xx = np.mgrid[0:h, 0:w]
    imgs = np.empty((F, h, w, 3), np.uint8)
    masks = np.empty((F, h, w), np.uint8)
    rgbs = np.empty((F, h, w, 3), np.float32)
    white = (yy < h // 3) & (xx >= w - w // 3 - 13)
    for f in range(F):
        smooth = 127 + 90 * np.stack([np.sin(xx / (7. + c + f) + yy / 11.) * np.cos(yy / (5. + f) - c) for c in range(3)], -1)
        imgs[f] = np.clip(smooth + rng.randint(-20, 21, size=(h, w, 3)), 0, 255).astype(np.uint8)
        masks[f] = ((xx - w * (0.45 + 0.1 * f)) ** 2 / (0.3 * w) ** 2 + (yy - h * 0.55) ** 2 / (0.35 * h) ** 2 < 1).astype(np.uint8)
        imgs[f][white] = 255
        rgbs[f] = np.clip(imgs[f] / 255. + rng.normal(0, 0.06, size=(h, w, 3)), 0, 1).astype(np.float32)
        rgbs[f][white] = 1.0
    return imgs, masks, rng.randint(0, 256, size=(1, h, w, 3)).astype(np.uint8), rgbs, white


def abi_sums(r, bank_struct, img_row, box, rgb_dev, flags, out=None):
    """pg_frame_metrics through the C ABI -> (return code, float64 [8] from the device)"""
    out = torch.full((8,), -7.0, dtype=torch.float64, device=DEV) if out is None else out
    rc = r.lib.pg_frame_metrics(r.handle, r._stream(), C.byref(bank_struct), int(img_row), (C.c_int32 * 4)(*(int(v) for v in box)),
                                C.c_void_p(rgb_dev.data_ptr()), int(flags), C.c_void_p(out.data_ptr()))
    torch.cuda.synchronize()
    return rc, out.cpu().numpy()


def abi_val(r, bank_struct, img_row, box, rgb_dev, valid, flags, hw=None):
    """pg_frame_metrics_val through the C ABI -> (return code, float64 [12] from the device, with a guard entry behind them)"""
    out = torch.full((13,), -7.0, dtype=torch.float64, device=DEV)
    h, w = rgb_dev.shape[:2] if hw is None else hw
    rc = r.lib.pg_frame_metrics_val(r.handle, r._stream(), C.byref(bank_struct), int(img_row), (C.c_int32 * 4)(*(int(v) for v in box)),
                                    C.c_void_p(rgb_dev.data_ptr()), int(h), int(w),
                                    None if valid is None else (C.c_int32 * 4)(*(int(v) for v in valid)), int(flags), C.c_void_p(out.data_ptr()))
    torch.cuda.synchronize()
    out = out.cpu().numpy()
    assert out[12] == -7.0                                  # nothing behind the twelve is written
    return rc, out[:12]


def assert_sums(got, want, names, what=""):
    """every sum of `names` (ref.SUMS or ref.SUMS_VAL: a count at every even position, the real sum it counts behind it): the
    counts exactly, the real sums within 1e-9 max(1, |sum|)"""
    print(what, "got", got, "want", want)
    assert len(got) == len(want) == len(names)
    for i in range(0, len(names), 2):
        assert got[i] == want[i], (what, names[i], got[i], want[i])
    for i in range(1, len(names), 2):
        assert abs(got[i] - want[i]) <= 1e-9 * max(1.0, abs(want[i])), (what, names[i], got[i], want[i], got[i] - want[i])
