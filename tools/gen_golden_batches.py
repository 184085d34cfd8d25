#!/usr/bin/env python3
"""Capture golden training batches from the REAL reference data path: `BaseH5Dataset`, `RayImageSampler` and
`DataLoader(num_workers=0, collate_fn=ray_collate_fn)` (core/dataset.py, core/load_data.py:71-84), unmodified.

Runs only where the reference checkout exists.  The reference is imported through gen_golden's shims; the stubbed `h5py`
module gets a `File` that returns an in-memory dict (with close / __enter__ / __exit__), so the dataset reads small seeded
arrays instead of an .h5 file.  The pixel ids an item drew are not part of the reference's batch: they are recorded by a
wrapper around the instance's `sample_pixels` that calls the original and keeps its result.  Only arrays are written:
tests/golden/train_batches.npz.

Usage:  python tools/gen_golden_batches.py [--ref /root/reference] [--out tests/golden]
"""
from __future__ import annotations

import argparse
import os
import sys

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.dont_write_bytecode = True

from tools.gen_golden import _install_shims  # noqa: E402

F, H, W = 6, 20, 14                 # H != W, nothing a multiple of 4
K_PIXELS, N_IMAGES, N_BATCHES = 5, 4, 3
SEED_DATA, SEED_RUN, SEED_SAMPLER, N_SAMPLER_BATCHES = 11, 5, 7, 6
VARIANTS = {"plain": dict(centers=False, mask_img=False), "centers": dict(centers=True, mask_img=False),
            "mask_img": dict(centers=False, mask_img=True)}

_FILES = {}


class _MemFile(dict):
    """What the reference needs of h5py.File: a mapping of arrays, close(), a context manager."""

    def __init__(self, path, mode="r", **kw):
        super().__init__(_FILES[path])

    def close(self):
        pass

    def __enter__(self):
        return self

    def __exit__(self, *a):
        return False


def _rotation(rng):
    q, r = np.linalg.qr(rng.standard_normal((3, 3)))
    q = q * np.sign(np.diag(r))
    if np.linalg.det(q) < 0:
        q[:, 0] = -q[:, 0]
    return q


def make_inputs():
    rng = np.random.default_rng(SEED_DATA)
    P = H * W
    c2ws = np.zeros((F, 4, 4), np.float32)
    c2ws[:, 3, 3] = 1
    for f in range(F):
        c2ws[f, :3, :3] = np.eye(3) if f == 0 else _rotation(rng)      # frame 0: the identity shortcut of get_rays
        c2ws[f, :3, 3] = rng.uniform(-2, 2, 3)
    sampling = (rng.random((F, P)) < 0.4).astype(np.uint8)
    sampling[1::2] *= 255                                              # stored values 1 and 255
    return {
        "imgs": rng.integers(0, 256, (F, P, 3), dtype=np.uint8),
        "masks": (rng.random((F, P, 1)) < 0.5).astype(np.uint8),
        "sampling_masks": sampling,
        "bkgds": rng.integers(0, 256, (2, P, 3), dtype=np.uint8),
        "bkgd_idxs": np.array([0, 1, 1, 0, 1, 0], np.int64),
        "img_shape": np.array([F, H, W, 3], np.int64),
        "c2ws": c2ws,
        "focals": rng.uniform(15, 25, F).astype(np.float32),
        "focals_xy": rng.uniform(15, 25, (F, 2)).astype(np.float32),
        "centers": (np.array([W * 0.5, H * 0.5]) + rng.uniform(-2, 2, (F, 2))).astype(np.float32),
        "kp3d": rng.standard_normal((F, 24, 3)).astype(np.float32),
        "bones": rng.standard_normal((F, 24, 3)).astype(np.float32),
        "skts": rng.standard_normal((F, 24, 4, 4)).astype(np.float32),
        "cyls": rng.standard_normal((F, 5)).astype(np.float32),
    }


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--ref", default="/root/reference")
    ap.add_argument("--out", default=os.path.join(REPO, "tests", "golden"))
    a = ap.parse_args()
    _install_shims(a.ref)
    import torch
    from torch.utils.data import DataLoader
    sys.modules["h5py"].File = _MemFile
    from core.dataset import BaseH5Dataset, RayImageSampler, ray_collate_fn

    inp = make_inputs()
    out = {f"in_{k}": v for k, v in inp.items()}
    out.update(HW=np.array([H, W]), k_pixels=np.array(K_PIXELS), n_images=np.array(N_IMAGES), seed_run=np.array(SEED_RUN),
               seed_sampler=np.array(SEED_SAMPLER), variants=np.array(sorted(VARIANTS)))
    for name, v in VARIANTS.items():
        data = {k: inp[k] for k in ("imgs", "masks", "sampling_masks", "bkgds", "bkgd_idxs", "img_shape", "c2ws", "kp3d", "bones",
                                    "skts", "cyls")}
        data["focals"] = inp["focals_xy"] if v["centers"] else inp["focals"]      # the centres variant also has (fx, fy) focals
        if v["centers"]:
            data["centers"] = inp["centers"]
        _FILES[name] = data
        ds = BaseH5Dataset(name, N_samples=K_PIXELS, mask_img=v["mask_img"])
        drawn = []
        original = ds.sample_pixels

        def recording(idx, q_idx, original=original, drawn=drawn):
            p = original(idx, q_idx)
            drawn.append((int(q_idx), p.copy()))
            return p

        ds.sample_pixels = recording
        torch.manual_seed(SEED_RUN)
        np.random.seed(SEED_RUN)
        loader = DataLoader(ds, batch_sampler=RayImageSampler(ds, N_images=N_IMAGES, N_iter=N_BATCHES), num_workers=0,
                            collate_fn=ray_collate_fn)
        for b, batch in enumerate(loader):
            for key, t in batch.items():
                out[f"{name}_b{b}_{key}"] = t.numpy()
            mine, drawn[:] = drawn[:N_IMAGES], drawn[N_IMAGES:]
            out[f"{name}_b{b}_items"] = np.array([q for q, _ in mine], np.int64)
            out[f"{name}_b{b}_pixel_idxs"] = np.stack([p for _, p in mine]).astype(np.int64)
        assert b == N_BATCHES - 1 and not drawn
    # the sampler alone, right behind torch.manual_seed
    torch.manual_seed(SEED_SAMPLER)
    out["sampler_batches"] = np.stack(list(RayImageSampler(range(F), N_images=N_IMAGES, N_iter=N_SAMPLER_BATCHES)))
    os.makedirs(a.out, exist_ok=True)
    path = os.path.join(a.out, "train_batches.npz")
    np.savez_compressed(path, **out)
    print(f"wrote {path}: {len(out)} arrays, {os.path.getsize(path)} bytes")
    for key in ("plain_b0_rays_d", "centers_b0_rays_d", "plain_b0_target_s", "plain_b0_kp_idx", "sampler_batches"):
        print(key, out[key].dtype, out[key].shape)


if __name__ == "__main__":
    main()
