"""Training batches on the device: the reference's `BaseH5Dataset.__getitem__` -> `RayImageSampler` ->
`DataLoader(collate_fn=ray_collate_fn)` (core/dataset.py:57-105, 277-364, 730-802; core/load_data.py:71-84).

The reference forms a batch on the host, once per image: read the image's sampling mask, `np.where`, `np.random.choice(valid, N,
replace=False)`, sort, gather the pixels and form the rays in numpy -- 128 to 256 images per step.  Here the dataset's pixels live
on the device as the uint8 they are stored as (`DeviceImageBank`), the valid pixels of every image are indexed once, and a batch is
a few small launches on the caller's stream (`RayBatchSource`): pg_batch_sample_pixels, pg_batch_gather (csrc/pg_batch.hip), then
`torch.index_select` for the per-ray pose rows.  The batch has the reference's keys, shapes, dtypes and ray order.  There is no
torch fallback: without the library the bank cannot be built.
"""
from __future__ import annotations

import ctypes as C
from typing import Dict, Optional

import numpy as np
import torch

from . import _ffi

_I32P = C.POINTER(C.c_int32)
_I64P = C.POINTER(C.c_int64)
SLAB_BYTES = 256 << 20
MAX_PIXELS_PER_IMAGE = 1024
ITEM_KEYS = ("img_row", "pose_row", "kp_idx", "cam_row", "cam_idx")
POSE_KEYS = ("kp3d", "bones", "skts", "cyls")
# numpy's message for np.random.choice(valid, k, replace=False) with k > len(valid) (dataset.py:288-290)
CHOICE_MESSAGE = "Cannot take a larger sample than population when 'replace=False'"


def _i32p(a: Optional[np.ndarray]):
    return None if a is None else a.ctypes.data_as(_I32P)


class DeviceImageBank:
    """A dataset's pixels on the renderer's device, with the index of every image's valid pixels.

    `imgs` [F,P,3], `masks` [F,P,1], `sampling_masks` [F,P] (P = H W, `HW` = (H, W)), optional `bkgds` [n_bkgd,P,3] with
    `bkgd_idxs` [F]: uint8.  A `torch.uint8` tensor already on the renderer's device is adopted without a copy; anything else
    that can be sliced along its first axis and has a `.shape` (a numpy array, an h5py dataset) is uploaded in slabs of at most
    256 MiB through pinned staging.  `c2ws` [n_cam,4,4] or [n_cam,3,4], `focals` [n_cam] or [n_cam,2] = (fx, fy), `centers`
    [n_cam,2] or None: kept as float32 (the reference casts c2w to float32, dataset.py:247).  `mask_img`: dataset.py:272-273.

    `counts` (host int64 [F]) are the images' valid pixels: one copy back, when the bank is built.  `nbytes`: device bytes held."""

    def __init__(self, renderer, imgs, masks, sampling_masks, c2ws, focals, HW, bkgds=None, bkgd_idxs=None, centers=None,
                 mask_img=False):
        self.device = self._check_renderer(renderer)
        self.renderer = renderer
        H, W = (int(v) for v in HW)
        if H <= 0 or W <= 0:
            raise ValueError(f"DeviceImageBank: HW = ({H}, {W}) must be positive")
        self.HW, self.P = (H, W), H * W
        F = int(imgs.shape[0])
        if F <= 0:
            raise ValueError("DeviceImageBank: no images")
        if (bkgds is None) != (bkgd_idxs is None):
            raise ValueError("DeviceImageBank: bkgds and bkgd_idxs come together")
        self.F, self.mask_img = F, bool(mask_img)
        self.bkgd_idxs = None
        if bkgds is not None:
            self.bkgd_idxs = np.ascontiguousarray(np.asarray(bkgd_idxs).reshape(-1), dtype=np.int32)
            n_bkgd = int(bkgds.shape[0])
            if len(self.bkgd_idxs) != F:
                raise ValueError(f"DeviceImageBank: {len(self.bkgd_idxs)} bkgd_idxs for {F} images")
            if self.bkgd_idxs.min() < 0 or self.bkgd_idxs.max() >= n_bkgd:
                raise ValueError(f"DeviceImageBank: a background index is outside [0, {n_bkgd})")
        cam = lambda a, tail: torch.as_tensor(np.asarray(a.detach().cpu() if torch.is_tensor(a) else a), dtype=torch.float32).reshape(tail)
        c2ws = cam(c2ws, (-1,) + tuple(np.shape(c2ws)[-2:]))
        if c2ws.shape[1:] not in ((4, 4), (3, 4)):
            raise ValueError("DeviceImageBank: c2ws [n_cam,4,4] or [n_cam,3,4] expected")
        n_cam = c2ws.shape[0]
        focals = cam(focals, (n_cam, -1))
        if focals.shape[1] not in (1, 2):
            raise ValueError("DeviceImageBank: focals [n_cam] or [n_cam,2] expected")
        self.n_cam = n_cam
        self.c2ws = c2ws[:, :3, :4].contiguous().to(self.device)
        self.focals = focals.expand(n_cam, 2).contiguous().to(self.device)
        self.centers = None if centers is None else cam(centers, (n_cam, 2)).contiguous().to(self.device)
        self.imgs = self._pixels("imgs", imgs, F, 3)
        self.masks = self._pixels("masks", masks, F, 1)
        self.sampling_masks = self._pixels("sampling_masks", sampling_masks, F, 1)
        self.bkgds = None if bkgds is None else self._pixels("bkgds", bkgds, int(bkgds.shape[0]), 3)
        self._build_index()
        self.struct = _ffi.PgImageBank(
            imgs=self.imgs.data_ptr(), masks=self.masks.data_ptr(), bkgds=None if self.bkgds is None else self.bkgds.data_ptr(),
            bkgd_idxs=_i32p(self.bkgd_idxs), c2ws=self.c2ws.data_ptr(), focals=self.focals.data_ptr(),
            centers=None if self.centers is None else self.centers.data_ptr(), F=F, P=self.P,
            n_bkgd=0 if self.bkgds is None else self.bkgds.shape[0], n_cam=n_cam, H=H, W=W, mask_img=int(self.mask_img))

    @staticmethod
    def _check_renderer(renderer):
        device = torch.device(renderer.device)
        if device.type != "cuda":
            raise NotImplementedError(f"DeviceImageBank: the renderer is on {device}, not on a HIP device (torch 'cuda:N'); "
                                      "the image bank has no CPU path")
        return device

    def _pixels(self, name, src, rows, ch) -> torch.Tensor:
        """`src` as a contiguous device uint8 tensor of `rows` x (P ch) bytes."""
        shape = tuple(int(v) for v in src.shape)
        row_bytes = self.P * ch
        if shape[0] != rows or int(np.prod(shape[1:], dtype=np.int64)) != row_bytes:
            raise ValueError(f"DeviceImageBank: {name} has shape {shape}; {rows} rows of {self.P} pixels x {ch} expected")
        if torch.is_tensor(src) and src.device == self.device:
            if src.dtype != torch.uint8 or not src.is_contiguous():
                raise TypeError(f"DeviceImageBank: {name} on the device must be a contiguous torch.uint8 tensor")
            return src
        dev = torch.empty((rows, row_bytes), dtype=torch.uint8, device=self.device)
        step = max(1, SLAB_BYTES // row_bytes)
        stage = torch.empty((min(step, rows), row_bytes), dtype=torch.uint8, pin_memory=True)
        for r0 in range(0, rows, step):
            r1 = min(rows, r0 + step)
            slab = src[r0:r1]
            slab = slab.detach().cpu().numpy() if torch.is_tensor(slab) else np.asarray(slab)
            if slab.dtype != np.uint8:
                raise TypeError(f"DeviceImageBank: {name} must be uint8, not {slab.dtype}")
            stage[:r1 - r0].copy_(torch.from_numpy(np.ascontiguousarray(slab).reshape(r1 - r0, row_bytes)))
            dev[r0:r1].copy_(stage[:r1 - r0], non_blocking=True)
            torch.cuda.current_stream(self.device).synchronize()          # the staging buffer is free again
        return dev

    def _build_index(self):
        r, F, P = self.renderer, self.F, self.P
        with torch.cuda.device(self.device):
            counts = torch.empty(F, dtype=torch.int64, device=self.device)
            _ffi.call(r, "pg_pixel_index_count", self.sampling_masks, F, P, counts)
            self.start = torch.zeros(F + 1, dtype=torch.int64, device=self.device)
            torch.cumsum(counts, 0, out=self.start[1:])
            self.counts = counts.cpu().numpy()                             # the one copy back
            self.total = int(self.counts.sum())
            self.ids = torch.empty(max(self.total, 1), dtype=torch.int32, device=self.device)
            _ffi.call(r, "pg_pixel_index_emit", self.sampling_masks, F, P, self.start, self.total, self.ids)

    @property
    def nbytes(self) -> int:
        ts = (self.imgs, self.masks, self.sampling_masks, self.bkgds, self.c2ws, self.focals, self.centers, self.start, self.ids)
        return int(sum(t.numel() * t.element_size() for t in ts if t is not None))


class ImageBatchSampler:
    """The reference's `RayImageSampler` over `RandIntGenerator` (dataset.py:730-793): `N_iter` batches of `N_images` item indices,
    each batch sorted.  Every pass over the items is a fresh `torch.randperm` from a CPU generator seeded with one int64 drawn from
    the global torch RNG; indices are drawn until the batch is full and the permutation restarts when it is exhausted, so a batch
    may hold an item twice.  After `torch.manual_seed(s)` the batches are the reference's."""

    def __init__(self, n_items: int, N_images: int, N_iter: Optional[int] = None):
        if n_items <= 0 or N_images <= 0:
            raise ValueError("ImageBatchSampler: n_items and N_images must be positive")
        self.n_items, self.N_images = int(n_items), int(N_images)
        self.N_iter = self.n_items if N_iter is None else int(N_iter)

    def _pass(self):
        generator = torch.Generator(device="cpu")
        generator.manual_seed(int(torch.empty((), dtype=torch.int64).random_().item()))
        yield from torch.randperm(self.n_items, generator=generator).tolist()

    def __iter__(self):
        it = self._pass()
        for _ in range(self.N_iter):
            batch = []
            while len(batch) < self.N_images:
                try:
                    idx = next(it)
                except StopIteration:
                    it = self._pass()
                    idx = next(it)
                batch.append(idx)
            yield np.sort(batch)

    def __len__(self):
        return self.N_iter


class RayBatch(dict):
    """One training batch: the tensors of `ray_collate_fn`'s dict on the device; `kp_idx_host` is `kp_idx` as a host int64 array
    (what `HipPoseOptLayer.forward` takes without a copy back)."""
    kp_idx_host: Optional[np.ndarray] = None


class RayBatchSource:
    """Iterating yields one `RayBatch` per training step, `n = N_sample_images (N_rand // N_sample_images)` rays: the images of an
    `ImageBatchSampler` batch in sorted order, `N_rand // N_sample_images` pixels of each in ascending order.

    Keys as `ray_collate_fn` leaves them after `dict_to_device` (core/trainer.py:239): rays_o, rays_d [n,3], rays [2,n,3],
    target_s [n,3], fgs [n,1], bgs [n,3] (banks with backgrounds), kp_idx, cam_idxs [n] int64, kp3d [n,24,3], bones [n,24,3],
    skts [n,24,4,4], cyls [n,5] (with `poses`), temp_val [n] (with `temp_validity`, `TemporalDatasetWrapper`, dataset.py:713-728);
    and ray_batch [n,11] (render()'s packing, trainer.py:118-137), pixel_idxs [n] int32, img_idxs [n_img] int64 (the items).

    `poses`: dict of device float32 tensors kp3d [K,24,3], bones [K,24,3], skts [K,24,4,4], cyls [K,5].  `items`: dict of integer
    arrays, one entry per queried item -- img_row, pose_row, kp_idx, cam_row, cam_idx; a missing key is the identity, as
    `get_kp_idx` / `get_cam_idx` of the base class (dataset.py:391-405); the subclasses' index maps go here.  Draws come from
    `generator` (a torch.Generator on the bank's device, or None: the device's global one).  No host synchronisation per step.

    Not built, NotImplementedError before any library call: patch_size > 1, N_nms > 0 (`_sample_in_box2d`), multiview, several
    banks in one source (`ConcatH5Dataset`)."""

    def __init__(self, bank, N_rand: int, N_sample_images: int, poses: Optional[Dict[str, torch.Tensor]] = None,
                 items: Optional[Dict[str, np.ndarray]] = None, temp_validity=None, generator: Optional[torch.Generator] = None, *,
                 patch_size: int = 1, N_nms: float = 0, multiview: bool = False, N_iter: Optional[int] = None):
        if patch_size > 1:
            raise NotImplementedError("RayBatchSource: patch_size > 1 (patches of rays) is not built on the HIP path; no shipped config sets it")
        if N_nms > 0:
            raise NotImplementedError("RayBatchSource: N_nms > 0 (out-of-mask samples inside the 2-D box, _sample_in_box2d) is not built on "
                                      "the HIP path; no shipped config sets it")
        if multiview:
            raise NotImplementedError("RayBatchSource: multiview datasets are not built on the HIP path")
        if isinstance(bank, (list, tuple)):
            if len({tuple(b.HW) for b in bank}) > 1:
                raise NotImplementedError("RayBatchSource: banks of different frame sizes in one source (ConcatH5Dataset) are not built "
                                          "on the HIP path")
            if len(bank) != 1:
                raise NotImplementedError("RayBatchSource: several banks in one source (ConcatH5Dataset) are not built on the HIP path")
            bank = bank[0]
        self.bank, self.generator = bank, generator
        self.N_rand, self.N_sample_images = int(N_rand), int(N_sample_images)
        self.k = self.N_rand // self.N_sample_images if self.N_sample_images > 0 else 0
        if not 1 <= self.k <= MAX_PIXELS_PER_IMAGE:
            raise ValueError(f"RayBatchSource: N_rand // N_sample_images = {self.k} pixels per image is outside [1, {MAX_PIXELS_PER_IMAGE}]")
        self.device = torch.device(bank.device)
        self.items = {}
        for key in ITEM_KEYS:
            if items is not None and items.get(key) is not None:
                a = np.asarray(items[key]).reshape(-1)
                if not np.issubdtype(a.dtype, np.integer):
                    raise TypeError(f"RayBatchSource: items[{key!r}] must be integers, not {a.dtype}")
                self.items[key] = a.astype(np.int64)
        lens = {len(a) for a in self.items.values()}
        if len(lens) > 1:
            raise ValueError("RayBatchSource: the arrays of `items` differ in length")
        self.n_items = lens.pop() if lens else bank.F
        for key, bound in (("img_row", bank.F), ("cam_row", bank.n_cam)):
            a = self.items.get(key)
            if (a is not None and len(a) and (a.min() < 0 or a.max() >= bound)) or (a is None and self.n_items > bound):
                raise IndexError(f"RayBatchSource: items[{key!r}] reaches outside [0, {bound})")
        self.poses = None
        if poses is not None:
            self.poses = {}
            for key in POSE_KEYS:
                t = poses[key]
                if not torch.is_tensor(t) or t.device != self.device or t.dtype != torch.float32:
                    raise TypeError(f"RayBatchSource: poses[{key!r}] must be a float32 tensor on {self.device}")
                self.poses[key] = t.contiguous()
            K = min(t.shape[0] for t in self.poses.values())
            a = self.items.get("pose_row")
            if (a is not None and len(a) and (a.min() < 0 or a.max() >= K)) or (a is None and self.n_items > K):
                raise IndexError(f"RayBatchSource: items['pose_row'] reaches outside the {K} poses")
        self.temp_val = None
        if temp_validity is not None:
            tv = np.asarray(temp_validity)
            if len(tv) < self.n_items:
                raise ValueError(f"RayBatchSource: {len(tv)} temp_validity entries for {self.n_items} items")
            pair = ((tv + np.roll(tv, -1, axis=0)) // 2).astype(np.float32)      # (tv[idx] + tv[(idx + 1) % len]) // 2
            self.temp_val = torch.from_numpy(pair).to(self.device)
        self.N_iter = N_iter

    def _rows(self, key, q):
        a = self.items.get(key)
        return q if a is None else a[q]

    def __len__(self):
        return self.n_items if self.N_iter is None else self.N_iter

    def __iter__(self):
        for q in ImageBatchSampler(self.n_items, self.N_sample_images, self.N_iter):
            yield self.sample(q)

    def sample(self, img_idxs) -> RayBatch:
        """The batch of the items `img_idxs` in the given order, `k` random pixels of each."""
        q = self._items(img_idxs)
        bank, r, k = self.bank, self.bank.renderer, self.k
        img_rows = np.ascontiguousarray(self._rows("img_row", q), dtype=np.int32)
        if (bank.counts[img_rows] < k).any():
            raise ValueError(CHOICE_MESSAGE)
        with torch.cuda.device(self.device):
            draws = torch.rand(len(q), k, dtype=torch.float64, device=self.device, generator=self.generator)
            pix = torch.empty(len(q) * k, dtype=torch.int32, device=self.device)
            _ffi.call(r, "pg_batch_sample_pixels", bank.ids, bank.start, bank.counts.ctypes.data_as(_I64P), bank.F, _i32p(img_rows), len(q), k,
                      draws, pix)
            return self._gather(q, img_rows, pix)

    def gather(self, img_idxs, pixel_idxs) -> RayBatch:
        """The same dict from pixel ids the caller chose: `pixel_idxs` [n_img,k] (or [n_img k]) flat pixel ids, host or device."""
        q = self._items(img_idxs)
        if torch.is_tensor(pixel_idxs):
            pix = pixel_idxs.to(device=self.device, dtype=torch.int32).reshape(-1).contiguous()
        else:
            a = np.asarray(pixel_idxs).reshape(-1)
            if not np.issubdtype(a.dtype, np.integer):
                raise TypeError(f"RayBatchSource.gather: pixel ids must be integers, not {a.dtype}")
            if a.size and (a.min() < 0 or a.max() >= self.bank.P):
                raise IndexError(f"RayBatchSource.gather: a pixel id is outside [0, {self.bank.P})")
            pix = torch.from_numpy(a.astype(np.int32)).to(self.device)
        if len(q) == 0 or pix.numel() % len(q) or not 1 <= pix.numel() // len(q) <= MAX_PIXELS_PER_IMAGE:
            raise ValueError(f"RayBatchSource.gather: {pix.numel()} pixel ids for {len(q)} images")
        with torch.cuda.device(self.device):
            return self._gather(q, np.ascontiguousarray(self._rows("img_row", q), dtype=np.int32), pix)

    def _items(self, img_idxs) -> np.ndarray:
        q = np.atleast_1d(np.asarray(img_idxs.cpu() if torch.is_tensor(img_idxs) else img_idxs)).reshape(-1)
        if q.size and not np.issubdtype(q.dtype, np.integer):
            raise TypeError(f"RayBatchSource: item indices must be integers, not {q.dtype}")
        q = q.astype(np.int64)
        if q.size and (q.min() < 0 or q.max() >= self.n_items):
            raise IndexError(f"RayBatchSource: item index outside [0, {self.n_items})")
        return q

    def _gather(self, q, img_rows, pix) -> RayBatch:
        bank, r = self.bank, self.bank.renderer
        n_img, n = len(q), pix.numel()
        k = n // n_img
        cam_rows = np.ascontiguousarray(self._rows("cam_row", q), dtype=np.int32)
        dev = self.device
        rays = torch.empty(2, n, 3, device=dev)
        out = RayBatch(rays=rays, rays_o=rays[0], rays_d=rays[1], target_s=torch.empty(n, 3, device=dev), fgs=torch.empty(n, 1, device=dev),
                       ray_batch=torch.empty(n, 11, device=dev), pixel_idxs=pix)
        if bank.bkgds is not None:
            out["bgs"] = torch.empty(n, 3, device=dev)
        _ffi.call(r, "pg_batch_gather", C.byref(bank.struct), _i32p(img_rows), _i32p(cam_rows), n_img, k, pix, out["target_s"], out["fgs"],
                  out.get("bgs"), out["rays_o"], out["rays_d"], out["ray_batch"])
        # the per-image integers go up in one pinned array; everything per ray is formed from it on the device
        host = torch.from_numpy(np.stack([q, self._rows("kp_idx", q), self._rows("cam_idx", q), self._rows("pose_row", q)]).astype(np.int64))
        per_img = host.pin_memory().to(dev, non_blocking=True)
        per_ray = per_img[:, :, None].expand(4, n_img, k).reshape(4, n)
        out["img_idxs"], out["kp_idx"], out["cam_idxs"] = per_img[0], per_ray[1], per_ray[2]
        out.kp_idx_host = np.repeat(np.asarray(self._rows("kp_idx", q), dtype=np.int64), k)
        if self.poses is not None:
            for key in POSE_KEYS:
                out[key] = torch.index_select(self.poses[key], 0, per_ray[3])
        if self.temp_val is not None:
            out["temp_val"] = torch.index_select(self.temp_val, 0, per_ray[0])
        return out
