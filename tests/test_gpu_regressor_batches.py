"""The regressor's input batches on the device (posegen_amd/regressor_batches.py; pg_regressor_input, csrc/pg_regressor.hip) against
the float64 restatement tests/regressor_ref.py, which tests/test_regressor_ref.py holds to scipy.

Every output lies within N u M of the restatement: u = 2^-24, M = max_c max(mean_c, 1 - mean_c) / std_c, and
N = (2 r_y + 1) + (2 r_x + 1) + 24 -- the two dot products with once-rounded weights (taps + 1 each), the normalisation (3), the two
interpolations (7 each) and 5 of slack; the kernel's composed filters of 2 r + 2 taps stay inside that count."""
import ctypes as C

import numpy as np
import pytest
import torch

from posegen_amd import _ffi, regressor_batches as rb
from tests import regressor_ref as ref

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
MEAN, STD = rb.IMG_NORM_MEAN, rb.IMG_NORM_STD
EINVAL = -1


@pytest.fixture(scope="module")
def renderer():
    from posegen_amd import surreal_config
    from posegen_amd.raycaster import HipRenderer
    r = HipRenderer(surreal_config(), device=DEV)          # no weights loaded: the entry point needs none
    yield r
    r.close()


def _noise(rng, h, w):
    return rng.integers(0, 256, (h, w, 3), dtype=np.uint8)


@pytest.fixture(scope="module")
def ragged(renderer):
    """A store of pictures of eight sizes and the eleven items of the edge cases: (images, store, rows, boxes)."""
    rng = np.random.default_rng(20)
    inset = np.full((40, 44, 3), 255, np.uint8)
    inset[6:29, 8:28] = _noise(rng, 23, 20)                # the box's outside is white: a mirror about the image would show
    images = [_noise(rng, 64, 48), _noise(rng, 37, 41), _noise(rng, 2, 3), _noise(rng, 1, 5), _noise(rng, 17, 16), inset,
              _noise(rng, 30, 34), _noise(rng, 256, 20)]
    full = lambda i: [0, 0, images[i].shape[1], images[i].shape[0]]
    rows = np.array([0, 1, 2, 3, 4, 5, 6, 6, 6, 6, 7])
    boxes = np.array([full(0), full(1), full(2), full(3), full(4), [8, 6, 28, 29],
                      [0, 5, 20, 25], [14, 5, 34, 25], [5, 0, 25, 20], [5, 10, 25, 30], full(7)], dtype=np.int32)
    return images, rb.PixelStore(renderer, images), rows, boxes


def _check_against_restatement(images, rows, boxes, R, got):
    worst = 0.0
    for b, (row, box) in enumerate(zip(rows, boxes)):
        want = ref.regressor_input(images[row], box, R, MEAN, STD)
        bound = ref.bound(int(box[3] - box[1]), int(box[2] - box[0]), R, MEAN, STD)
        err = float(np.abs(got[b].astype(np.float64) - want).max())
        print(f"item {b}: {box[3] - box[1]} x {box[2] - box[0]} -> {R}: max err {err:.3e}, bound {bound:.3e}, share {err / bound:.3f}")
        assert err <= bound, (b, R, err, bound)
        worst = max(worst, err / bound)
    return worst


@pytest.mark.parametrize("R", [16, 7, 48])
def test_edge_items_of_one_launch_lie_within_the_bound(ragged, R):
    """R = 16: 64 x 48 (r = 6 / 4), 37 x 41 and 2 x 3 and 1 x 5 (upscaling, mirrored borders, the n = 1 axis), 17 x 16 (s just above 1
    with r = 0 beside identity), a box inset in a white image, boxes touching each border, 256 x 20 (s = 16, r = 30).  R = 7: an odd
    tile edge, without the item that is more than 16 R high.  R = 48: 37 x 41 and the small ones upscaled."""
    images, store, rows, boxes = ragged
    keep = np.nonzero((boxes[:, 3] - boxes[:, 1] <= 16 * R) & (boxes[:, 2] - boxes[:, 0] <= 16 * R))[0]
    assert len(keep) == (10 if R == 7 else 11)
    assert ref.radius(64, 16)[1] == 6 and ref.radius(48, 16)[1] == 4 and ref.radius(256, 16)[1] == 30 and ref.radius(17, 16)[1] == 0
    out = rb.regressor_input(store, rows[keep], boxes[keep], out_res=R)
    assert out.shape == (len(keep), 3, R, R) and out.dtype == torch.float32 and out.is_contiguous()
    worst = _check_against_restatement(images, rows[keep], boxes[keep], R, out.cpu().numpy())
    print(f"R = {R}: largest share of the bound {worst:.3f}")


def test_an_item_alone_and_in_a_batch_has_the_same_bytes(ragged):
    _, store, rows, boxes = ragged
    pick = np.array([10, 1, 0, 5, 3])                        # r = 30 beside upscaling beside r = 6 / 4
    batch = rb.regressor_input(store, rows[pick], boxes[pick], out_res=16)
    again = rb.regressor_input(store, rows[pick], boxes[pick], out_res=16)
    assert torch.equal(batch, again)
    for b, i in enumerate(pick):
        alone = rb.regressor_input(store, rows[i:i + 1], boxes[i:i + 1], out_res=16)
        assert torch.equal(alone[0], batch[b]), int(i)
    other = rb.regressor_input(store, rows[pick[::-1].copy()], boxes[pick[::-1].copy()], out_res=16)
    assert torch.equal(other.flip(0), batch)


def _call(r, pixels, n_bytes, items, R, out, mean=MEAN, std=STD):
    arr = (_ffi.PgCropItem * len(items))(*[_ffi.PgCropItem(*it) for it in items])
    m, s = (C.c_float * 3)(*mean), (C.c_float * 3)(*std)
    return r.lib.pg_regressor_input(r.handle, r._stream(), C.c_void_p(pixels.data_ptr()), n_bytes, arr, len(items), R, m, s,
                                    C.c_void_p(out.data_ptr()))


def test_bad_arguments_are_refused_and_nothing_is_written(renderer, ragged):
    r = renderer
    H, W = 256, 20
    pixels = torch.zeros(H * W * 3, dtype=torch.uint8, device=DEV)
    out = torch.full((2, 3, 16, 16), -7.0, device=DEV)
    good = (0, H, W, 0, 0, 20, 30)
    assert _call(r, pixels, pixels.numel(), [good, good], 16, out) == 0
    torch.cuda.synchronize()
    assert not (out == -7).any()
    cases = {
        "an empty box": ([good, (0, H, W, 5, 4, 5, 9)], 16, pixels.numel()),
        "an empty box (rows)": ([(0, H, W, 5, 9, 8, 9), good], 16, pixels.numel()),
        "a box outside its image": ([good, (0, H, W, 0, 0, 21, 30)], 16, pixels.numel()),
        "a box below its image": ([good, (0, H, W, 0, 250, 20, 257)], 16, pixels.numel()),
        "a negative corner": ([good, (0, H, W, -1, 0, 20, 30)], 16, pixels.numel()),
        "n > 16 R": ([good, (0, H, W, 0, 0, 20, 256)], 15, pixels.numel()),
        "R = 0": ([good, good], 0, pixels.numel()),
        "R = 513": ([good, good], 513, pixels.numel()),
        "an image past n_bytes": ([good, good], 16, pixels.numel() - 1),
        "an offset past n_bytes": ([good, (3, H, W, 0, 0, 20, 30)], 16, pixels.numel()),
    }
    big = torch.full((2, 3, 513, 513), -7.0, device=DEV)     # (room for what R = 513 would write)
    for name, (items, R, n_bytes) in cases.items():
        big.fill_(-7.0)
        assert _call(r, pixels, n_bytes, items, R, big) == EINVAL, name
        assert r.lib.pg_last_error(r.handle), name
        torch.cuda.synchronize()
        assert (big == -7).all(), name
    assert _call(r, pixels, pixels.numel(), [good], 16, big, std=(0.2, 0.0, 0.2)) == EINVAL
    assert r.lib.pg_regressor_input(r.handle, r._stream(), None, 8, None, 0, 16, None, None, None) == EINVAL
    torch.cuda.synchronize()
    assert (big == -7).all()
    # the Python layer refuses the same before the library is called, `out` untouched
    _, store, rows, boxes = ragged
    out = torch.full((1, 3, 16, 16), -7.0, device=DEV)
    for box, R in (([5, 4, 5, 9], 16), ([0, 0, 49, 64], 16), ([0, 0, 48, 65], 16), ([0, 0, 48, 64], 3), ([0, 0, 48, 64], 0),
                   ([0, 0, 48, 64], 513)):
        o = out if R == 16 else None
        with pytest.raises(ValueError):
            rb.regressor_input(store, [0], [box], out_res=R, out=o)
    with pytest.raises(IndexError):
        rb.regressor_input(store, [len(store)], [[0, 0, 1, 1]], out_res=16, out=out)
    torch.cuda.synchronize()
    assert (out == -7).all()


def test_pixel_store_appends_across_a_doubling_and_adopts_without_a_copy(renderer):
    rng = np.random.default_rng(3)
    frames = torch.from_numpy(rng.integers(0, 256, (4, 20, 24, 3), dtype=np.uint8)).to(DEV)
    store = rb.PixelStore(renderer)
    assert len(store) == 0 and store.nbytes == 0 and store.sizes.shape == (0, 2)
    assert store.append(frames[:2].contiguous()).tolist() == [0, 1]
    cap = store.capacity
    boxes = rb.fixed_crop_boxes(4, 1, 19)
    before = rb.regressor_input(store, [0, 1], boxes[:2], out_res=16)
    assert store.append(frames[2:3].contiguous()).tolist() == [2]
    assert store.capacity == 2 * cap and store.nbytes == 3 * 20 * 24 * 3           # grown by doubling
    assert store.append(frames[3:4].contiguous()).tolist() == [3] and store.capacity == 2 * cap   # room was left: no growth
    assert len(store) == 4 and store.sizes.tolist() == [[20, 24]] * 4 and store.offsets.tolist() == [0, 1440, 2880, 4320]
    after = rb.regressor_input(store, [0, 1, 2, 3], boxes, out_res=16)
    assert torch.equal(after[:2], before)
    adopted = rb.PixelStore(renderer, frames)
    assert adopted.pixels.data_ptr() == frames.data_ptr() and adopted.capacity == frames.numel() and len(adopted) == 4
    assert torch.equal(rb.regressor_input(adopted, [0, 1, 2, 3], boxes, out_res=16), after)
    keep = frames.clone()
    assert adopted.append(frames[:1].contiguous()).tolist() == [4] and torch.equal(frames, keep)   # the adopted tensor is left as it is
    assert torch.equal(rb.regressor_input(adopted, [4], boxes[:1], out_res=16)[0], after[0])
    images = [f.cpu().numpy() for f in frames]
    _check_against_restatement(images, range(4), boxes, 16, after.cpu().numpy())


def test_batch_source_yields_the_loaders_batches(renderer):
    rng = np.random.default_rng(4)
    frames = torch.from_numpy(rng.integers(0, 256, (11, 20, 24, 3), dtype=np.uint8)).to(DEV)
    store = rb.PixelStore(renderer, frames)
    boxes = rb.fixed_crop_boxes(11, 2, 18)
    boxes[3] = [0, 1, 24, 20]
    poses = torch.arange(11 * 72, dtype=torch.float32, device=DEV).reshape(11, 24, 3)
    want = rb.regressor_input(store, np.arange(11), boxes, out_res=16)
    src = rb.RegressorBatchSource(store, boxes, poses, batch_size=4, out_res=16)
    batches = list(src)
    assert len(src) == 3 and [len(b["image"]) for b in batches] == [4, 4, 3] and all(set(b) == {"image", "pose"} for b in batches)
    assert torch.equal(torch.cat([b["image"] for b in batches]), want) and torch.equal(torch.cat([b["pose"] for b in batches]), poses)
    order = np.arange(11)[::-1]
    rev = list(rb.RegressorBatchSource(store, boxes, poses, batch_size=4, out_res=16, order=order))
    assert [len(b["image"]) for b in rev] == [4, 4, 3]
    assert torch.equal(torch.cat([b["image"] for b in rev]), want.flip(0)) and torch.equal(torch.cat([b["pose"] for b in rev]), poses.flip(0))
    # rows: the items' pictures
    rows = np.array([10, 0, 5])
    picked = list(rb.RegressorBatchSource(store, boxes[rows], poses[:3], batch_size=2, out_res=16, rows=rows))
    assert torch.equal(torch.cat([b["image"] for b in picked]), want[torch.from_numpy(rows).to(DEV)])
    with pytest.raises(ValueError, match="permutation"):
        rb.RegressorBatchSource(store, boxes, poses, order=[0] * 11)
    with pytest.raises(ValueError, match="item 2"):
        rb.RegressorBatchSource(store, np.r_[boxes[:2], [[0, 0, 25, 20]]], poses[:3])


def test_beside_the_torch_operator_chain(renderer):
    """A smooth 512^2 frame (a gradient plus a disc), crop [100:412] -> 224: the kernel lies within N u M of the restatement; the chain
    of torch operators (ganloop.resize_antialiased) does not lie within 4 N u M -- its F.interpolate forms the sample positions in
    float32."""
    from posegen_amd.ganloop import resize_antialiased
    yy, xx = np.mgrid[0:512, 0:512].astype(np.float64)
    disc = ((yy - 250.0) ** 2 + (xx - 270.0) ** 2 < 90.0 ** 2)
    frame = np.stack([xx / 511 * 200 + disc * 55, yy / 511 * 180 + disc * 60, (xx + yy) / 1022 * 150 + disc * 90], -1)
    frame = np.round(frame).astype(np.uint8)
    box = rb.fixed_crop_boxes(1, 100, 412)
    want = ref.regressor_input(frame, box[0], 224, MEAN, STD)
    bound = ref.bound(312, 312, 224, MEAN, STD)
    dev = torch.from_numpy(frame).to(DEV)
    got = rb.regressor_input(rb.PixelStore(renderer, dev[None].contiguous()), [0], box)[0].cpu().numpy().astype(np.float64)
    err = float(np.abs(got - want).max())
    img = dev[100:412, 100:412].permute(2, 0, 1)[None].float() / 255.0
    mean, std = torch.tensor(MEAN, device=DEV).view(1, 3, 1, 1), torch.tensor(STD, device=DEV).view(1, 3, 1, 1)
    old = resize_antialiased((img - mean) / std, (224, 224))[0].cpu().numpy().astype(np.float64)
    err_old = float(np.abs(old - want).max())
    print(f"kernel {err:.3e} ({err / bound:.3f} of the bound {bound:.3e}); torch operator chain {err_old:.3e} ({err_old / bound:.1f} bounds)")
    assert err <= bound
    assert err_old > 4 * bound
