"""A numpy restatement of the training-batch kernels (posegen_amd/csrc/pg_batch.hip) and of the image sampler: the pixel index,
Floyd's k-subset at given draws, the gather in float32 in the kernels' order of operations, `RayImageSampler`'s batches.  The GPU
tests compare the device outputs with these bit for bit; the host tests compare these with the golden of the reference."""
import numpy as np
import torch

F32 = np.float32


def pixel_index(sampling_masks):
    """(counts int64 [F], start int64 [F + 1], ids int32 [total]): np.where(mask > 0) of every image, back to back."""
    m = np.asarray(sampling_masks).reshape(len(sampling_masks), -1)
    per = [np.where(row > 0)[0].astype(np.int32) for row in m]
    counts = np.array([len(p) for p in per], dtype=np.int64)
    start = np.zeros(len(m) + 1, dtype=np.int64)
    np.cumsum(counts, out=start[1:])
    return counts, start, (np.concatenate(per) if per else np.zeros(0, np.int32))


def floyd_ranks(m, k, u):
    """Floyd's algorithm in the order of the draws u [k] (float64 in [0, 1)): k distinct ranks below m, ascending."""
    assert 1 <= k <= m
    chosen = set()
    for i in range(k):
        j = m - k + i
        t = min(int(np.floor(np.float64(u[i]) * np.float64(j + 1))), j)
        chosen.add(j if t in chosen else t)
    return np.array(sorted(chosen), dtype=np.int64)


def sample_pixels(counts, start, ids, img_rows, k, draws):
    """pixel ids int32 [n_img, k] of the batch images `img_rows` at `draws` [n_img, k]."""
    out = np.empty((len(img_rows), k), dtype=np.int32)
    for a, img in enumerate(img_rows):
        out[a] = ids[start[img] + floyd_ranks(int(counts[img]), k, draws[a])]
    return out


def gather(bank, img_rows, pix, cam_rows=None):
    """`bank`: dict with imgs [F,P,3], masks [F,P,1] uint8, c2ws [n_cam,>=3,4], focals [n_cam] or [n_cam,2], HW, and optionally bkgds,
    bkgd_idxs, centers [n_cam,2], mask_img.  pix [n_img,k].  float32 throughout, one rounding per operation, in the kernel's order."""
    H, W = (int(v) for v in bank["HW"])
    P = H * W
    img_rows = np.asarray(img_rows).reshape(-1)
    cam_rows = img_rows if cam_rows is None else np.asarray(cam_rows).reshape(-1)
    pix = np.asarray(pix).reshape(len(img_rows), -1).astype(np.int64)
    k = pix.shape[1]
    img = np.repeat(img_rows, k)
    cam = np.repeat(cam_rows, k)
    p = pix.reshape(-1)
    imgs = np.asarray(bank["imgs"]).reshape(-1, P, 3)
    fg = np.asarray(bank["masks"]).reshape(-1, P)[img, p].astype(F32)[:, None]
    target = imgs[img, p].astype(F32) / F32(255)
    out = {}
    if bank.get("bkgds") is not None:
        bk = np.asarray(bank["bkgd_idxs"]).reshape(-1)[img]
        bg = np.asarray(bank["bkgds"]).reshape(-1, P, 3)[bk, p].astype(F32) / F32(255)
        if bank.get("mask_img"):
            target = target * fg + (F32(1) - fg) * bg
        out["bgs"] = bg
    c2w = np.asarray(bank["c2ws"], dtype=F32)[cam]
    focal = np.asarray(bank["focals"], dtype=F32).reshape(len(bank["c2ws"]), -1)
    fx, fy = focal[cam, 0], focal[cam, -1]
    row, col = (p // W).astype(F32), (p % W).astype(F32)
    if bank.get("centers") is not None:
        c = np.asarray(bank["centers"], dtype=F32)[cam]
        x = (col - c[:, 0]) / fx
        y = (-row + c[:, 1]) / fy
    else:
        x = (col - F32(W) * F32(0.5)) / fx
        y = (-(row - F32(H) * F32(0.5))) / fy
    R = c2w[:, :3, :3]
    d = (x[:, None] * R[:, :, 0] + y[:, None] * R[:, :, 1]) + F32(-1) * R[:, :, 2]
    o = np.ascontiguousarray(c2w[:, :3, 3])
    nrm = np.sqrt((d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2])
    n = len(p)
    ray_batch = np.concatenate([o, d, np.zeros((n, 1), F32), np.ones((n, 1), F32), d / nrm[:, None]], axis=1)
    assert all(a.dtype == F32 for a in (target, fg, d, o, ray_batch))
    out.update(target_s=target, fgs=fg, rays_o=o, rays_d=d, rays=np.stack([o, d]), ray_batch=ray_batch,
               pixel_idxs=p.astype(np.int32))
    return out


def image_batches(n_items, N_images, n_batches):
    """`RayImageSampler`'s first n_batches batches (dataset.py:730-793) from the global torch RNG as it stands."""
    def one_pass():
        g = torch.Generator(device="cpu")
        g.manual_seed(int(torch.empty((), dtype=torch.int64).random_().item()))
        return iter(torch.randperm(n_items, generator=g).tolist())

    it, out = None, []
    for _ in range(n_batches):
        batch = []
        while len(batch) < N_images:
            idx = next(it, None) if it is not None else None
            if idx is None:
                it = one_pass()
                idx = next(it)
            batch.append(idx)
        out.append(np.sort(batch))
    return out
