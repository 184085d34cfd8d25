"""The regressor's training batches on the device: the reference's `pose_dataset`, `mpii_dataset` and `mpii_nerf_dataset`
(run_gan.py:1636-1735) behind `DataLoader(..., batch_size=128)` in `train_spin` (:1849-1952), and the per-image lines of
`train_gan`'s inner loop (:2057-2081).

Per image the reference reads a PNG, slices a crop, applies `process_sample` (divide by 255, normalise) and calls
`skimage.transform.resize(image, (3, 224, 224), anti_aliasing=True)` on the host.  Here the pictures live on the device as the
uint8 they are rendered as (`PixelStore`, which `render_for_regressor(..., return_frames=True)` feeds), and a batch of (image, crop
box) items becomes the float32 `[B,3,R,R]` input in one launch of pg_regressor_input (csrc/pg_regressor.hip; the arithmetic is
spelled out at its declaration in include/posegen_hip.h).  `RegressorBatchSource` yields what the reference's loaders yield.  There
is no torch fallback: a renderer that is not on a HIP device is refused.
"""
from __future__ import annotations

import ctypes as C
from typing import Optional, Sequence

import numpy as np
import torch

from . import _ffi
from .ganloop import IMG_NORM_MEAN, IMG_NORM_STD

# What the reference's `process_sample` really normalises with: `Normalize(mean=IMG_NORM_MEAN, std=IMG_NORM_MEAN)`
# (run_gan.py:2347) -- the standard deviation passed there is the mean.  Not the default here; pass `*REFERENCE_NORM` as
# (mean, std) to reproduce that line.
REFERENCE_NORM = (IMG_NORM_MEAN, IMG_NORM_MEAN)
MAX_RES = 512
MAX_SCALE = 16
_ITEM = np.dtype([("offset", "<i8"), ("H", "<i4"), ("W", "<i4"), ("x0", "<i4"), ("y0", "<i4"), ("x1", "<i4"), ("y1", "<i4")])
assert _ITEM.itemsize == C.sizeof(_ffi.PgCropItem)


def _check_renderer(who: str, renderer) -> torch.device:
    device = torch.device(renderer.device)
    if device.type != "cuda":
        raise NotImplementedError(f"{who}: the renderer is on {device}, not on a HIP device (torch 'cuda:N'); "
                                  "the regressor's batches have no CPU path")
    return device


class PixelStore:
    """uint8 pictures `[H_i,W_i,3]` (RGB-interleaved) on the renderer's device in one flat buffer.

    `images`: a contiguous `torch.uint8` tensor `[F,H,W,3]` already on the renderer's device is adopted without a copy; anything else
    is taken as a sequence of host uint8 arrays `[H_i,W_i,3]` of any sizes and uploaded once; None: an empty store.
    `append(frames)` adds device frames `[F,H,W,3]` -- what `render_for_regressor(..., return_frames=True)` returns -- and returns
    their rows; the buffer's capacity doubles when it is full, so appends cost amortised constant time.
    `len(store)`: the pictures; `sizes`: host int32 `[n,2]` = (H, W); `offsets`: host int64 `[n]`, bytes into the buffer; `nbytes`:
    bytes of pictures held; `capacity`: bytes allocated."""

    def __init__(self, renderer, images=None):
        self.device = _check_renderer("PixelStore", renderer)
        self.renderer = renderer
        self._buf = torch.empty(0, dtype=torch.uint8, device=self.device)
        self._used = 0
        self._offsets, self._sizes = [], []
        if images is None:
            return
        if torch.is_tensor(images) and images.device == self.device:
            self._check_frames("PixelStore", images)
            self._buf = images.view(-1)                                    # adopted: the same storage
            self._note(images.shape)
            return
        host = [np.asarray(a.detach().cpu() if torch.is_tensor(a) else a) for a in images]
        for i, a in enumerate(host):
            if a.dtype != np.uint8 or a.ndim != 3 or a.shape[2] != 3 or a.shape[0] < 1 or a.shape[1] < 1:
                raise TypeError(f"PixelStore: image {i} has dtype {a.dtype} and shape {a.shape}; uint8 [H,W,3] expected")
        total = sum(a.size for a in host)
        stage = torch.empty(total, dtype=torch.uint8, pin_memory=True)
        view = stage.numpy()
        for a in host:
            view[self._used:self._used + a.size] = a.reshape(-1)
            self._offsets.append(self._used)
            self._sizes.append((a.shape[0], a.shape[1]))
            self._used += a.size
        with torch.cuda.device(self.device):
            self._buf = stage.to(self.device, non_blocking=True)
            torch.cuda.current_stream(self.device).synchronize()           # the staging buffer goes away with this call

    def _check_frames(self, who, frames):
        if not torch.is_tensor(frames) or frames.device != self.device or frames.dtype != torch.uint8 or not frames.is_contiguous() \
                or frames.dim() != 4 or frames.shape[3] != 3 or min(frames.shape[:3]) < 1:
            raise TypeError(f"{who}: a contiguous torch.uint8 tensor [F,H,W,3] on {self.device} expected")

    def _note(self, shape):
        F, H, W = (int(v) for v in shape[:3])
        rows = np.arange(len(self._sizes), len(self._sizes) + F)
        self._offsets.extend(self._used + i * H * W * 3 for i in range(F))
        self._sizes.extend([(H, W)] * F)
        self._used += F * H * W * 3
        return rows

    def append(self, frames: torch.Tensor) -> np.ndarray:
        self._check_frames("PixelStore.append", frames)
        need = self._used + frames.numel()
        with torch.cuda.device(self.device):
            if need > self._buf.numel():
                grown = torch.empty(max(need, 2 * self._buf.numel()), dtype=torch.uint8, device=self.device)
                grown[:self._used].copy_(self._buf[:self._used])
                self._buf = grown
            self._buf[self._used:need].copy_(frames.view(-1))
        return self._note(frames.shape)

    def __len__(self):
        return len(self._sizes)

    @property
    def pixels(self) -> torch.Tensor:
        return self._buf

    @property
    def sizes(self) -> np.ndarray:
        return np.asarray(self._sizes, dtype=np.int32).reshape(-1, 2)

    @property
    def offsets(self) -> np.ndarray:
        return np.asarray(self._offsets, dtype=np.int64)

    @property
    def nbytes(self) -> int:
        return self._used

    @property
    def capacity(self) -> int:
        return int(self._buf.numel())


def fixed_crop_boxes(n: int, lo: int, hi: int) -> np.ndarray:
    """The boxes of `image[lo:hi, lo:hi]` for n items, host int32 `[n,4]` = (x0, y0, x1, y1): `[120:392]` in the three datasets
    (run_gan.py:1647, 1700), `[100:412]` in `train_gan` (:2061)."""
    if n < 0 or not 0 <= lo < hi:
        raise ValueError(f"fixed_crop_boxes: n = {n}, [{lo}:{hi}]: n >= 0 and 0 <= lo < hi expected")
    return np.tile(np.array([lo, lo, hi, hi], dtype=np.int32), (int(n), 1))


def mpii_crop_boxes(centers, scales, sizes) -> np.ndarray:
    """The box `mpii_dataset.__getitem__` slices (run_gan.py:1722-1728; the same lines in `mpii_nerf_dataset`, :1678-1684), host int32
    `[n,4]` = (x0, y0, x1, y1) from `centers` [n,2] = (x, y), `scales` [n] and the images' `sizes` [n,2] = (H, W):
    side = 200 scale, xy1 = center - side / 2, xy2 = center + side / 2, then the clips AS THE REFERENCE WRITES THEM, with the axes
    swapped: xy1[0] to [0, H] and xy2[0] to [0, W], xy1[1] to [0, W] and xy2[1] to [0, H] (`image.shape[0]` is the height).  On a
    picture that is not square a box can therefore end before the border it should reach, or start past the picture.  Then `int()`
    truncation, and what numpy's slice does to a bound beyond the array (it stops at the array's end).  A crop that comes out empty
    is a ValueError naming the item (the reference fails inside `resize` there)."""
    c = np.asarray(centers, dtype=np.float64).reshape(-1, 2)
    side = np.asarray(scales, dtype=np.float64).reshape(-1) * 200
    hw = np.asarray(sizes).reshape(-1, 2).astype(np.int64)
    if not (len(c) == len(side) == len(hw)):
        raise ValueError(f"mpii_crop_boxes: {len(c)} centers, {len(side)} scales and {len(hw)} sizes")
    if not (np.isfinite(c).all() and np.isfinite(side).all()):
        raise ValueError("mpii_crop_boxes: a center or a scale is not finite")
    H, W = hw[:, 0], hw[:, 1]
    xy1, xy2 = c - side[:, None] / 2, c + side[:, None] / 2
    x0, x1 = np.clip(xy1[:, 0], 0, H), np.clip(xy2[:, 0], 0, W)           # (sic: H bounds the left edge)
    y0, y1 = np.clip(xy1[:, 1], 0, W), np.clip(xy2[:, 1], 0, H)           # (sic: W bounds the top edge)
    box = np.stack([np.minimum(np.trunc(x0), W), np.minimum(np.trunc(y0), H), np.minimum(np.trunc(x1), W),
                    np.minimum(np.trunc(y1), H)], axis=1).astype(np.int32)
    empty = np.nonzero((box[:, 2] <= box[:, 0]) | (box[:, 3] <= box[:, 1]))[0]
    if len(empty):
        i = int(empty[0])
        raise ValueError(f"mpii_crop_boxes: item {i}: the crop [{box[i, 1]}:{box[i, 3]}, {box[i, 0]}:{box[i, 2]}] of its "
                         f"{H[i]} x {W[i]} image is empty")
    return box


def _items(who: str, store, rows, boxes, out_res: int) -> np.ndarray:
    """The call's pg_crop_item array after the checks the library makes as well, as ValueError / IndexError naming the item."""
    R = int(out_res)
    if not 1 <= R <= MAX_RES:
        raise ValueError(f"{who}: out_res = {R} is outside [1, {MAX_RES}]")
    rows = np.asarray(rows).reshape(-1)
    boxes = np.asarray(boxes)
    if rows.size and not np.issubdtype(rows.dtype, np.integer) or boxes.size and not np.issubdtype(boxes.dtype, np.integer):
        raise TypeError(f"{who}: rows and boxes must be integers")
    boxes = boxes.reshape(-1, 4).astype(np.int64)
    if len(rows) != len(boxes):
        raise ValueError(f"{who}: {len(rows)} rows for {len(boxes)} boxes")
    if rows.size and (rows.min() < 0 or rows.max() >= len(store)):
        raise IndexError(f"{who}: an image row is outside [0, {len(store)})")
    hw = store.sizes[rows].astype(np.int64)
    x0, y0, x1, y1 = boxes.T
    bad = (x0 < 0) | (y0 < 0) | (x0 >= x1) | (y0 >= y1) | (x1 > hw[:, 1]) | (y1 > hw[:, 0])
    if bad.any():
        i = int(np.nonzero(bad)[0][0])
        raise ValueError(f"{who}: item {i}: the box {tuple(int(v) for v in boxes[i])} is empty or leaves its "
                         f"{hw[i, 0]} x {hw[i, 1]} image")
    big = (x1 - x0 > MAX_SCALE * R) | (y1 - y0 > MAX_SCALE * R)
    if big.any():
        i = int(np.nonzero(big)[0][0])
        raise ValueError(f"{who}: item {i}: a crop of {y1[i] - y0[i]} x {x1[i] - x0[i]} is more than {MAX_SCALE} times out_res = {R}")
    items = np.empty(len(rows), dtype=_ITEM)
    items["offset"] = store.offsets[rows]
    items["H"], items["W"] = hw[:, 0], hw[:, 1]
    items["x0"], items["y0"], items["x1"], items["y1"] = x0, y0, x1, y1
    return items


def _launch(store, items: np.ndarray, out_res: int, mean, std, out: Optional[torch.Tensor]) -> torch.Tensor:
    r, dev, B, R = store.renderer, store.device, len(items), int(out_res)
    if out is None:
        out = torch.empty(B, 3, R, R, dtype=torch.float32, device=dev)
    elif not torch.is_tensor(out) or out.device != dev or out.dtype != torch.float32 or not out.is_contiguous() \
            or tuple(out.shape) != (B, 3, R, R):
        raise TypeError(f"regressor_input: out must be a contiguous float32 tensor [{B},3,{R},{R}] on {dev}")
    if B == 0:
        return out
    m, s = (C.c_float * 3)(*(float(v) for v in mean)), (C.c_float * 3)(*(float(v) for v in std))
    with torch.cuda.device(dev):
        _ffi.call(r, "pg_regressor_input", store.pixels, store.capacity, items.ctypes.data_as(C.POINTER(_ffi.PgCropItem)), B, R, m, s, out)
    return out


def regressor_input(store: PixelStore, rows, boxes, out_res: int = 224, mean: Sequence[float] = IMG_NORM_MEAN,
                    std: Sequence[float] = IMG_NORM_STD, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """float32 `[B,3,R,R]` on the device from one launch: item b is picture `rows[b]` of the store cropped to `boxes[b]` =
    (x0, y0, x1, y1) (`image[y0:y1, x0:x1]`), divided by 255, normalised with `mean` / `std` (default: the ImageNet pair of
    `render_for_regressor`; `REFERENCE_NORM` is what the reference's `process_sample` passes) and resized to R x R as
    `skimage.transform.resize(..., anti_aliasing=True)` does.  Refused before anything is launched, `out` untouched: R outside
    [1, 512], a box that is empty or leaves its picture, a crop side above 16 R.  Asynchronous on the current stream."""
    if len(mean) != 3 or len(std) != 3:
        raise ValueError("regressor_input: mean and std have three entries")
    return _launch(store, _items("regressor_input", store, rows, boxes, out_res), out_res, mean, std, out)


class RegressorBatchSource:
    """Iterating yields `{'image': [B,3,R,R] float32, 'pose': poses[items]}` on the device: what
    `DataLoader(pose_dataset(...), batch_size=128)` yields, items in sequence as the reference's loaders go without shuffling, the
    last batch short.  `boxes`: host int `[N,4]` (`fixed_crop_boxes`, `mpii_crop_boxes`); `poses`: a device tensor with one leading
    entry per item -- `[N,24,3]` key points for rendered frames, `[N,24,3]` axis-angle for MPII; `rows`: the store's picture of every
    item (None: item i is picture i); `order`: a permutation of the items chosen by the caller (None: 0 .. N - 1).  Every item is
    checked when the source is built; a batch is one launch and one slice or `index_select`, with no host synchronisation."""

    def __init__(self, store, boxes, poses: torch.Tensor, batch_size: int = 128, rows=None, order=None, out_res: int = 224,
                 mean: Sequence[float] = IMG_NORM_MEAN, std: Sequence[float] = IMG_NORM_STD):
        self.device = _check_renderer("RegressorBatchSource", store.renderer)
        self.store = store
        if batch_size < 1:
            raise ValueError(f"RegressorBatchSource: batch_size = {batch_size} must be positive")
        if len(mean) != 3 or len(std) != 3:
            raise ValueError("RegressorBatchSource: mean and std have three entries")
        self.batch_size, self.out_res, self.mean, self.std = int(batch_size), int(out_res), tuple(mean), tuple(std)
        N = len(np.asarray(boxes).reshape(-1, 4))
        self.items = _items("RegressorBatchSource", store, np.arange(N) if rows is None else rows, boxes, out_res)
        if not torch.is_tensor(poses) or poses.device != self.device or poses.shape[0] != N:
            raise TypeError(f"RegressorBatchSource: poses must be a tensor on {self.device} with {N} leading entries")
        self.poses = poses
        self.order = self.order_dev = None
        if order is not None:
            self.order = np.asarray(order).reshape(-1).astype(np.int64)
            if not np.array_equal(np.sort(self.order), np.arange(N)):
                raise ValueError(f"RegressorBatchSource: order is not a permutation of the {N} items")
            self.order_dev = torch.from_numpy(self.order).to(self.device)
        self.n_items = N

    def __len__(self):
        return -(-self.n_items // self.batch_size)

    def __iter__(self):
        for i in range(0, self.n_items, self.batch_size):
            j = min(i + self.batch_size, self.n_items)
            if self.order is None:
                items, pose = self.items[i:j], self.poses[i:j]
            else:
                items, pose = self.items[self.order[i:j]], torch.index_select(self.poses, 0, self.order_dev[i:j])
            yield {"image": _launch(self.store, np.ascontiguousarray(items), self.out_res, self.mean, self.std, None), "pose": pose}
