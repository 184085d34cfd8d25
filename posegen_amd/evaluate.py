"""Scoring rendered frames on the device: the reference's two `evaluate_metric` functions -- `run_render.py --eval`
(run_render.py:888-974: every frame inside its 2-D box) and the trainer's validation render
(core/utils/evaluation_helpers.py:257-385: whole frames) -- PSNR, SSIM and their foreground-masked variants against the
ground truth of a `DeviceImageBank`.

The reference scores on the host: every frame is downloaded, and an 11 x 11 Gaussian runs over five moment images per frame on the
CPU.  Here a frame stays where `render_frames_device` left it; `pg_frame_metrics` (csrc/pg_metrics.hip) reduces it, the bank's
bytes and the box to eight float64 sums on the device, and the sums of all frames come back in one copy (`FrameScorer`).  There is
no torch fallback.

The trainer's own call -- `render_testset(..., eval_metrics=True, eval_both=True)` at `args.render_factor` (run_nerf.py:586-589)
-- has names of its own beside those: `ValidationScorer`, `evaluate_validation` and `evaluate_testset` run on
`pg_frame_metrics_val`, which takes the frame at the size it was rendered at, scores its bilinear upsampling to the bank's size
(fused into the kernel's staging) and adds the sums under each frame's 2-D box ("valid") to the foreground ones.

The unmasked numbers are the reference's.  The masked SSIM is this project's definition: the reference multiplies
the per-image mean that `pytorch_msssim.SSIM(size_average=False)` returns by a full-size mask after a `.permute(0, 2, 3, 1)` of a
1-D tensor, which cannot run; here a map value is weighted by the mask at its window's centre pixel.
"""
from __future__ import annotations

import ctypes as C
import os
from typing import Optional

import numpy as np
import torch

from . import _ffi

SUMS = ("n", "se", "n_fg", "se_fg", "n_map", "ssim", "n_fg_map", "ssim_fg")
SUMS_VAL = SUMS + ("n_valid", "se_valid", "n_valid_map", "ssim_valid")


def _ratio(num, den):
    """num / den elementwise in float64: 0 / 0 = NaN and x / 0 = inf, without numpy's warnings"""
    with np.errstate(divide="ignore", invalid="ignore"):
        return np.asarray(num, dtype=np.float64) / np.asarray(den, dtype=np.float64)


def _psnr(mse):
    with np.errstate(divide="ignore", invalid="ignore"):
        return -10.0 * np.log10(mse)


class FrameScorer:
    """The sums of `pg_frame_metrics` for a run of frames: a device float64 [capacity, 8] tensor, one row per frame, grown as
    needed; `score` enqueues a frame on the current stream and never waits for the device, `sums()` makes the one copy back.

    `use_masks`: the foreground sums are wanted (refused for a bank without masks).  `background`: the ground truth of a pixel
    outside the mask is the image's background (run_render.py:935-937, PG_METRICS_BG); None = the bank has backgrounds."""

    def __init__(self, bank, use_masks: bool = True, background: Optional[bool] = None, capacity: int = 64):
        self.device = torch.device(bank.device)
        if self.device.type != "cuda":
            raise NotImplementedError(f"FrameScorer: the bank is on {self.device}, not on a HIP device (torch 'cuda:N'); "
                                      "frames are scored by pg_frame_metrics only, there is no CPU path")
        if use_masks and getattr(bank, "masks", None) is None:
            raise ValueError("FrameScorer: masked scores asked for from a bank without masks (use_masks=False scores whole boxes only)")
        has_bg = getattr(bank, "bkgds", None) is not None
        if background and not has_bg:
            raise ValueError("FrameScorer: background=True (PG_METRICS_BG) needs a bank with backgrounds")
        if background and getattr(bank, "masks", None) is None:
            raise ValueError("FrameScorer: background=True (PG_METRICS_BG) needs a bank with masks")
        self.bank, self.use_masks = bank, bool(use_masks)
        self.flags = _ffi.PG_METRICS_BG if (has_bg if background is None else background) else 0
        self.capacity = max(int(capacity), 1)
        self._sums: Optional[torch.Tensor] = None
        self.n_frames = 0

    def _row(self, k: int) -> torch.Tensor:
        if self._sums is None or k >= self._sums.shape[0]:
            rows = max(self.capacity, k + 1, 0 if self._sums is None else 2 * self._sums.shape[0])
            grown = torch.zeros(rows, len(SUMS), dtype=torch.float64, device=self.device)
            if self._sums is not None:
                grown[:self._sums.shape[0]].copy_(self._sums)       # on the stream, behind the frames already enqueued
            self._sums = grown
        return self._sums[k]

    def score(self, k: int, rgb: torch.Tensor, img_idx: int, box):
        """Frame `rgb` (device float32 [H,W,3], H W = the bank's) against image `img_idx` of the bank inside `box` =
        ((tl_x, tl_y), (br_x, br_y)) or (x0, y0, x1, y1), into row k."""
        H, W = self.bank.HW
        if not torch.is_tensor(rgb) or tuple(rgb.shape) != (H, W, 3):
            raise ValueError(f"FrameScorer: a frame of shape {tuple(getattr(rgb, 'shape', ()))} against a bank of {H} x {W} images "
                             "(a render_factor other than 0 resamples the frame: not built)")
        if rgb.device != self.device:
            raise NotImplementedError(f"FrameScorer: the frame is on {rgb.device}, the bank on {self.device}; there is no CPU path")
        if rgb.dtype != torch.float32 or not rgb.is_contiguous():
            raise TypeError("FrameScorer: the frame must be a contiguous float32 tensor")
        if k < 0:
            raise IndexError(f"FrameScorer: row {k}")
        bx = np.asarray([np.asarray(b).reshape(-1) for b in box] if len(box) == 2 else box).reshape(-1)
        if bx.size != 4:
            raise ValueError("FrameScorer: a box is ((tl_x, tl_y), (br_x, br_y)) or (x0, y0, x1, y1)")
        r = self.bank.renderer
        with torch.cuda.device(self.device):
            row = self._row(int(k))
            r._check(r.lib.pg_frame_metrics(r.handle, r._stream(), C.byref(self._struct()), int(img_idx),
                                            (C.c_int32 * 4)(*(int(v) for v in bx)), C.c_void_p(rgb.data_ptr()), self.flags,
                                            C.c_void_p(row.data_ptr())))
        self.n_frames = max(self.n_frames, int(k) + 1)

    def _struct(self):
        if self.use_masks or self.flags:
            return self.bank.struct
        s = _ffi.PgImageBank.from_buffer_copy(self.bank.struct)          # whole boxes only: the kernel is told there is no mask
        s.masks = None
        return s

    def sink(self, img_idxs, bboxes):
        """A `frame_sink(k, rgb, disp, acc)` for `render_frames_device`: frame k is scored against image img_idxs[k] in bboxes[k]."""
        img_idxs = [int(i) for i in np.asarray(img_idxs).reshape(-1)]

        def frame_sink(k, rgb, disp, acc):
            self.score(k, rgb, img_idxs[k], bboxes[k])
        return frame_sink

    def sums(self) -> np.ndarray:
        """float64 [n_frames, 8]: (n, se, n_fg, se_fg, n_map, ssim, n_fg_map, ssim_fg) of every frame scored so far"""
        if self._sums is None:
            return np.zeros((0, len(SUMS)), dtype=np.float64)
        return self._sums[:self.n_frames].cpu().numpy()


def box_scores(sums: np.ndarray, use_masks: bool = True):
    """The reference's per-frame values (run_render.py:947-964) from the sums [F,8] -> dict of float64 [F] arrays.  Frames below the
    window have NaN SSIM entries."""
    s = {k: sums[:, i] for i, k in enumerate(SUMS)}
    out = {"psnr": _psnr(_ratio(s["se"], s["n"])), "ssim": _ratio(s["ssim"], s["n_map"])}
    if use_masks:
        out["fg_psnr"] = _psnr(_ratio(s["se_fg"], s["n_fg"]))
        out["fg_ssim"] = _ratio(s["ssim_fg"], s["n_fg_map"])
    return out


def _refuse_resampling(who, render_factor):
    if render_factor:
        raise NotImplementedError(f"{who}: render_factor = {render_factor} resamples the frames against the ground truth "
                                  "(F.interpolate in the reference): not built, render at the bank's frame size")


@torch.no_grad()
def evaluate_frames(render_poses, hwf, chunk, render_kwargs, bank, img_idxs, basedir=None, use_masks=True, background=None,
                    **kwargs):
    """`run_render.py`'s render followed by `evaluate_metric` (run_render.py:888-974): frame k of `render_frames_device(render_poses,
    hwf, chunk, render_kwargs, **kwargs)` is scored inside its 2-D box against image img_idxs[k] of `bank` as soon as its kernels
    are enqueued, and never downloaded.  Returns the reference's score dict {'psnr', 'ssim', 'fg_psnr', 'fg_ssim'} as lists over
    frames; a frame whose box holds no mask pixel is left out of all four (the reference's `continue`), a frame whose box is below
    11 pixels has NaN SSIM entries, inf stays inf.  With `basedir`, scores.npy and score_final.txt are written as the reference does.
    `use_masks=False`: no foreground lists (the reference without gt masks)."""
    from .rays import frame_boxes
    from .render import _caster_device, _scalar_hw, render_frames_device
    _refuse_resampling("evaluate_frames", kwargs.get("render_factor", 0))
    for key in ("ret_acc", "gt_imgs", "bones", "base_bg"):       # render_path's, without meaning for frames that stay on the device
        kwargs.pop(key, None)
    for key in ("frame_sink", "boxes"):
        if kwargs.get(key) is not None:
            raise ValueError(f"evaluate_frames: {key} is this function's own")
    H, W, focal = hwf
    if not _scalar_hw(H, W) or (int(H), int(W)) != tuple(bank.HW):
        raise ValueError(f"evaluate_frames: frames of {H} x {W} against a bank of {bank.HW[0]} x {bank.HW[1]} images")
    scorer = FrameScorer(bank, use_masks=use_masks, background=background)
    r, dev = _caster_device(render_kwargs["ray_caster"])
    if torch.device(dev) != scorer.device:
        raise ValueError(f"evaluate_frames: the renderer is on {dev}, the bank on {scorer.device}")
    kp, cyls = kwargs.get("kp"), kwargs.get("cyls")
    if kp is None and cyls is None:
        raise NotImplementedError("render_path needs kp or cyls (bounding-cylinder cull)")
    ids = kwargs.get("frame_ids")
    ids = list(range(len(render_poses))) if ids is None else list(ids)
    img_idxs = np.asarray(img_idxs).reshape(-1)
    if len(img_idxs) != len(ids):
        raise ValueError(f"evaluate_frames: {len(img_idxs)} image indices for {len(ids)} frames")
    if len(img_idxs) and (img_idxs.min() < 0 or img_idxs.max() >= bank.F):
        raise IndexError(f"evaluate_frames: an image index is outside [0, {bank.F})")
    # the boxes once, for the renderer and for the scorer
    cyl_t, bboxes, meta = frame_boxes(r, render_poses, int(H), int(W), focal, kps=kp, cylinder_params=cyls,
                                      ext_scale=kwargs.get("ext_scale", 0.00035), centers=kwargs.get("centers"))
    boxes = (cyl_t, bboxes, [(None, None) + tuple(m) for m in meta])
    render_frames_device(render_poses, hwf, chunk, render_kwargs, boxes=boxes, frame_sink=scorer.sink(img_idxs, [bboxes[i] for i in ids]),
                         **kwargs)
    sums = scorer.sums()
    per = box_scores(sums, use_masks)
    keep = sums[:, 2] >= 1 if use_masks else np.ones(len(sums), dtype=bool)       # mask_cropped.sum() < 1: skipped
    score_dict = {k: [v for v in per[k][keep]] for k in ("psnr", "ssim")}
    score_dict["fg_psnr"] = [v for v in per["fg_psnr"][keep]] if use_masks else []
    score_dict["fg_ssim"] = [v for v in per["fg_ssim"][keep]] if use_masks else []
    if basedir is not None:
        os.makedirs(basedir, exist_ok=True)
        np.save(os.path.join(basedir, "scores.npy"), score_dict, allow_pickle=True)
        with open(os.path.join(basedir, "score_final.txt"), "w") as f:
            for k in score_dict:
                f.write(f"{k}: {np.mean(score_dict[k]) if len(score_dict[k]) else float('nan')}\n")
    return score_dict


@torch.no_grad()
def evaluate_metric(rgbs, bank, img_idxs, use_masks=True, eval_both=False, render_factor=0):
    """The validation render's `evaluate_metric` (core/utils/evaluation_helpers.py:257-385) on whole frames, box = the frame:
    `rgbs` [F,H,W,3] (a device tensor or numpy) against images `img_idxs` of `bank`, without backgrounds (that function takes the
    ground-truth images as they are).  Returns {"psnr", "ssim", "psnr_fg", "ssim_fg"} as means over frames, with that function's
    denominators max(., 1) and inf -> 0; with masks, images without a mask pixel are removed first (:296-305) and "psnr" / "ssim"
    are the foreground values (:361-364); without, "psnr_fg" / "ssim_fg" are None.  Not built: eval_both (a whole-frame map
    weighted by a box mask) and render_factor > 0 (resampling)."""
    if eval_both:
        raise NotImplementedError("evaluate_metric: eval_both weights a whole-frame SSIM map by each frame's box mask: not built "
                                  "(evaluate_frames scores inside the box)")
    _refuse_resampling("evaluate_metric", render_factor)
    scorer = FrameScorer(bank, use_masks=use_masks, background=False)
    H, W = bank.HW
    if len(np.shape(rgbs)) != 4 or tuple(np.shape(rgbs)[1:]) != (H, W, 3):
        raise ValueError(f"evaluate_metric: frames of shape {tuple(np.shape(rgbs))} against a bank of {H} x {W} images")
    img_idxs = np.asarray(img_idxs).reshape(-1)
    if len(img_idxs) != len(rgbs):
        raise ValueError(f"evaluate_metric: {len(img_idxs)} image indices for {len(rgbs)} frames")
    if not torch.is_tensor(rgbs):
        rgbs = torch.from_numpy(np.ascontiguousarray(rgbs, dtype=np.float32))
    rgbs = rgbs.to(device=scorer.device, dtype=torch.float32).contiguous()
    for k in range(len(rgbs)):
        scorer.score(k, rgbs[k], int(img_idxs[k]), (0, 0, W, H))
    s = scorer.sums()
    if not use_masks:                                        # :346-353: averages over all pixels
        psnr = _psnr(_ratio(s[:, 1], s[:, 0]))
        psnr[psnr == np.inf] = 0.0
        return {"psnr": psnr.mean() if len(s) else None, "ssim": _ratio(s[:, 5], s[:, 4]).mean() if len(s) else None,
                "psnr_fg": None, "ssim_fg": None}
    s = s[s[:, 2] > 0]                                       # images without any person in them
    fg_psnr = _psnr(_ratio(s[:, 3], np.maximum(s[:, 2], 1.0)))
    fg_psnr[fg_psnr == np.inf] = 0.0
    fg_ssim = _ratio(s[:, 7], np.maximum(s[:, 6], 1.0))
    fg_ssim[fg_ssim == np.inf] = 0.0
    fg_psnr = fg_psnr.mean() if len(s) else None
    fg_ssim = fg_ssim.mean() if len(s) else None
    return {"psnr": fg_psnr, "ssim": fg_ssim, "psnr_fg": fg_psnr, "ssim_fg": fg_ssim}


def _box4(who, box):
    bx = np.asarray([np.asarray(b).reshape(-1) for b in box] if len(box) == 2 else box).reshape(-1)
    if bx.size != 4:
        raise ValueError(f"{who}: a box is ((tl_x, tl_y), (br_x, br_y)) or (x0, y0, x1, y1)")
    return (C.c_int32 * 4)(*(int(v) for v in bx))


class ValidationScorer:
    """The sums of `pg_frame_metrics_val` for a run of frames: `FrameScorer`'s sibling for the trainer's validation render.  A
    device float64 [capacity, 12] tensor, one row per frame, grown as needed; `score` takes the frame at the size it was rendered
    at (h <= H, w <= W: it is scored as its bilinear upsampling to the bank's H x W) and enqueues it on the current stream,
    `sums()` makes the one copy back.  `use_masks`, `background`: as `FrameScorer` (None = the bank has backgrounds; the trainer's
    ground truth is gt * mask + (1 - mask) * bg, run_nerf.py:580-583)."""

    def __init__(self, bank, use_masks: bool = True, background: Optional[bool] = None, capacity: int = 64):
        self.device = torch.device(bank.device)
        if self.device.type != "cuda":
            raise NotImplementedError(f"ValidationScorer: the bank is on {self.device}, not on a HIP device (torch 'cuda:N'); "
                                      "frames are scored by pg_frame_metrics_val only, there is no CPU path")
        if use_masks and getattr(bank, "masks", None) is None:
            raise ValueError("ValidationScorer: masked scores asked for from a bank without masks (use_masks=False scores whole boxes only)")
        has_bg = getattr(bank, "bkgds", None) is not None
        if background and not has_bg:
            raise ValueError("ValidationScorer: background=True (PG_METRICS_BG) needs a bank with backgrounds")
        if background and getattr(bank, "masks", None) is None:
            raise ValueError("ValidationScorer: background=True (PG_METRICS_BG) needs a bank with masks")
        self.bank, self.use_masks = bank, bool(use_masks)
        self.flags = _ffi.PG_METRICS_BG if (has_bg if background is None else background) else 0
        self.capacity = max(int(capacity), 1)
        self._sums: Optional[torch.Tensor] = None
        self.n_frames = 0

    def _row(self, k: int) -> torch.Tensor:
        if self._sums is None or k >= self._sums.shape[0]:
            rows = max(self.capacity, k + 1, 0 if self._sums is None else 2 * self._sums.shape[0])
            grown = torch.zeros(rows, len(SUMS_VAL), dtype=torch.float64, device=self.device)
            if self._sums is not None:
                grown[:self._sums.shape[0]].copy_(self._sums)       # on the stream, behind the frames already enqueued
            self._sums = grown
        return self._sums[k]

    def _struct(self):
        if self.use_masks or self.flags:
            return self.bank.struct
        s = _ffi.PgImageBank.from_buffer_copy(self.bank.struct)          # whole boxes only: the kernel is told there is no mask
        s.masks = None
        return s

    def score(self, k: int, rgb: torch.Tensor, img_idx: int, valid_box=None, box=None):
        """Frame `rgb` (device float32 contiguous [h,w,3], h <= H, w <= W) against image `img_idx` of the bank into row k: the
        eight sums inside `box` (None: the whole frame) and the four under `valid_box` (None: 0).  Both boxes are in the bank's
        pixels, ((tl_x, tl_y), (br_x, br_y)) or (x0, y0, x1, y1)."""
        H, W = self.bank.HW
        shape = tuple(getattr(rgb, "shape", ()))
        if not torch.is_tensor(rgb) or len(shape) != 3 or shape[2] != 3 or not (1 <= shape[0] <= H and 1 <= shape[1] <= W):
            raise ValueError(f"ValidationScorer: a frame of shape {shape} against a bank of {H} x {W} images (a frame is [h,w,3] with "
                             "1 <= h <= H and 1 <= w <= W: it is upsampled, never downsampled)")
        if rgb.device != self.device:
            raise NotImplementedError(f"ValidationScorer: the frame is on {rgb.device}, the bank on {self.device}; there is no CPU path")
        if rgb.dtype != torch.float32 or not rgb.is_contiguous():
            raise TypeError("ValidationScorer: the frame must be a contiguous float32 tensor")
        if k < 0:
            raise IndexError(f"ValidationScorer: row {k}")
        bx = _box4("ValidationScorer", (0, 0, W, H) if box is None else box)
        vb = None if valid_box is None else _box4("ValidationScorer", valid_box)
        r = self.bank.renderer
        with torch.cuda.device(self.device):
            row = self._row(int(k))
            r._check(r.lib.pg_frame_metrics_val(r.handle, r._stream(), C.byref(self._struct()), int(img_idx), bx, C.c_void_p(rgb.data_ptr()),
                                                int(shape[0]), int(shape[1]), vb, self.flags, C.c_void_p(row.data_ptr())))
        self.n_frames = max(self.n_frames, int(k) + 1)

    def sink(self, img_idxs, valid_boxes=None):
        """A `frame_sink(k, rgb, disp, acc)` for `render_frames_device`: frame k is scored whole against image img_idxs[k], with
        valid_boxes[k] as its valid rectangle."""
        img_idxs = [int(i) for i in np.asarray(img_idxs).reshape(-1)]

        def frame_sink(k, rgb, disp, acc):
            self.score(k, rgb, img_idxs[k], None if valid_boxes is None else valid_boxes[k])
        return frame_sink

    def sums(self) -> np.ndarray:
        """float64 [n_frames, 12]: FrameScorer's eight, then (n_valid, se_valid, n_valid_map, ssim_valid), of every frame scored so far"""
        if self._sums is None:
            return np.zeros((0, len(SUMS_VAL)), dtype=np.float64)
        return self._sums[:self.n_frames].cpu().numpy()


def validation_scores(sums: np.ndarray, use_masks: bool = True, eval_both: bool = False):
    """{"psnr", "ssim", "psnr_fg", "ssim_fg"} from the sums [F,12] as evaluation_helpers.py:296-385 maps them: with masks, images
    without a mask pixel are removed first (:296-305); denominators max(., 1) (:325, :336), inf -> 0, means over frames; with
    `eval_both` "psnr" / "ssim" are the valid values (:372-373), without it the foreground values (:363-364); without masks the
    averages over all pixels (:346-353) and None for the "_fg" pair.  No frame left: None."""
    s = np.asarray(sums, dtype=np.float64).reshape(-1, len(SUMS_VAL))
    if eval_both and not use_masks:
        raise ValueError("eval_both needs masks (the reference's lines raise a NameError on fg_psnr without gt_masks)")

    def mean_of(v):
        v = np.asarray(v, dtype=np.float64)
        v[v == np.inf] = 0.0
        return v.mean() if len(v) else None

    if not use_masks:                                        # :346-353
        return {"psnr": mean_of(_psnr(_ratio(s[:, 1], s[:, 0]))), "ssim": mean_of(_ratio(s[:, 5], s[:, 4])), "psnr_fg": None, "ssim_fg": None}
    s = s[s[:, 2] > 0]                                       # images without any person in them
    fg_psnr = mean_of(_psnr(_ratio(s[:, 3], np.maximum(s[:, 2], 1.0))))
    fg_ssim = mean_of(_ratio(s[:, 7], np.maximum(s[:, 6], 1.0)))
    if not eval_both:
        return {"psnr": fg_psnr, "ssim": fg_ssim, "psnr_fg": fg_psnr, "ssim_fg": fg_ssim}
    valid_psnr = mean_of(_psnr(_ratio(s[:, 9], np.maximum(s[:, 8], 1.0))))
    valid_ssim = mean_of(_ratio(s[:, 11], np.maximum(s[:, 10], 1.0)))
    return {"psnr": valid_psnr, "ssim": valid_ssim, "psnr_fg": fg_psnr, "ssim_fg": fg_ssim}


def _refuse_eval_both(who, eval_both, use_masks, valid_boxes):
    if eval_both and not use_masks:
        raise ValueError(f"{who}: eval_both needs masks (the reference's lines raise a NameError on fg_psnr without gt_masks)")
    if eval_both and valid_boxes is None:
        raise ValueError(f"{who}: eval_both needs every frame's valid box (valid_boxes; rays.frame_boxes at the bank's H, W)")


@torch.no_grad()
def evaluate_validation(rgbs, bank, img_idxs, valid_boxes=None, use_masks=True, eval_both=False, background=False):
    """The validation render's `evaluate_metric` (core/utils/evaluation_helpers.py:257-385) as the trainer calls it: `rgbs`
    [F,h,w,3] (numpy or a device tensor) at the size they were rendered at, h <= H and w <= W, are scored whole against images
    `img_idxs` of `bank` as their bilinear upsampling to H x W (:309-312); `valid_boxes[k]` is frame k's 2-D box at the bank's
    resolution (its pixels are the reference's valid_masks).  Returns `validation_scores` of the sums.  `background`: the ground
    truth outside the mask is the image's background (run_nerf.py:580-583); None = the bank has backgrounds."""
    _refuse_eval_both("evaluate_validation", eval_both, use_masks, valid_boxes)
    scorer = ValidationScorer(bank, use_masks=use_masks, background=background)
    H, W = bank.HW
    shape = tuple(np.shape(rgbs))
    if len(shape) != 4 or shape[3] != 3 or (shape[0] and not (1 <= shape[1] <= H and 1 <= shape[2] <= W)):
        raise ValueError(f"evaluate_validation: frames of shape {shape} against a bank of {H} x {W} images ([F,h,w,3], h <= H, w <= W)")
    img_idxs = np.asarray(img_idxs).reshape(-1)
    if len(img_idxs) != shape[0]:
        raise ValueError(f"evaluate_validation: {len(img_idxs)} image indices for {shape[0]} frames")
    if valid_boxes is not None and len(valid_boxes) != shape[0]:
        raise ValueError(f"evaluate_validation: {len(valid_boxes)} valid boxes for {shape[0]} frames")
    if not torch.is_tensor(rgbs):
        rgbs = torch.from_numpy(np.ascontiguousarray(rgbs, dtype=np.float32))
    rgbs = rgbs.to(device=scorer.device, dtype=torch.float32).contiguous()
    for k in range(len(rgbs)):
        scorer.score(k, rgbs[k], int(img_idxs[k]), None if valid_boxes is None else valid_boxes[k])
    return validation_scores(scorer.sums(), use_masks, eval_both)


@torch.no_grad()
def evaluate_testset(render_poses, hwf, chunk, render_kwargs, bank, img_idxs, render_factor=0, eval_both=True, use_masks=True,
                     background=None, **kwargs):
    """The scoring path of the trainer's `render_testset(..., eval_metrics=True, eval_both=True)` (run_nerf.py:586-589): frame k of
    `render_frames_device(render_poses, hwf, chunk, render_kwargs, render_factor=render_factor, **kwargs)` -- H // render_factor x
    W // render_factor pixels -- goes to a `ValidationScorer`'s sink as soon as its kernels are enqueued, is scored as its upsampling
    to the bank's H x W against image img_idxs[k], and is never downloaded.  The valid boxes are `rays.frame_boxes` at the bank's
    H, W and the unscaled focal (evaluation_helpers.py:262-266 recomputes them this way when render_factor != 0); at
    render_factor = 0 they are the render's own boxes, computed once.  Returns {"psnr", "ssim", "psnr_fg", "ssim_fg"}
    (`validation_scores`)."""
    from .rays import frame_boxes
    from .render import _caster_device, _scalar_hw, render_frames_device
    for key in ("ret_acc", "gt_imgs", "bones", "base_bg"):       # render_path's, without meaning for frames that stay on the device
        kwargs.pop(key, None)
    for key in ("frame_sink", "boxes"):
        if kwargs.get(key) is not None:
            raise ValueError(f"evaluate_testset: {key} is this function's own")
    if eval_both and not use_masks:
        raise ValueError("evaluate_testset: eval_both needs masks (the reference's lines raise a NameError on fg_psnr without gt_masks)")
    render_factor = int(render_factor)
    if render_factor < 0:
        raise ValueError(f"evaluate_testset: render_factor = {render_factor}")
    H, W, focal = hwf
    if not _scalar_hw(H, W) or (int(H), int(W)) != tuple(bank.HW):
        raise ValueError(f"evaluate_testset: frames of {H} x {W} (before render_factor) against a bank of {bank.HW[0]} x {bank.HW[1]} images")
    if render_factor and (int(H) // render_factor < 1 or int(W) // render_factor < 1):
        raise ValueError(f"evaluate_testset: render_factor = {render_factor} leaves no pixel of a {H} x {W} frame")
    scorer = ValidationScorer(bank, use_masks=use_masks, background=background)
    r, dev = _caster_device(render_kwargs["ray_caster"])
    if torch.device(dev) != scorer.device:
        raise ValueError(f"evaluate_testset: the renderer is on {dev}, the bank on {scorer.device}")
    kp, cyls = kwargs.get("kp"), kwargs.get("cyls")
    if kp is None and cyls is None:
        raise NotImplementedError("render_path needs kp or cyls (bounding-cylinder cull)")
    ids = kwargs.get("frame_ids")
    ids = list(range(len(render_poses))) if ids is None else list(ids)
    img_idxs = np.asarray(img_idxs).reshape(-1)
    if len(img_idxs) != len(ids):
        raise ValueError(f"evaluate_testset: {len(img_idxs)} image indices for {len(ids)} frames")
    if len(img_idxs) and (img_idxs.min() < 0 or img_idxs.max() >= bank.F):
        raise IndexError(f"evaluate_testset: an image index is outside [0, {bank.F})")
    # the boxes at the bank's resolution: the scorer's valid rectangles, and at render_factor = 0 the renderer's boxes as well
    cyl_t, bboxes, meta = frame_boxes(r, render_poses, int(H), int(W), focal, kps=kp, cylinder_params=cyls,
                                      ext_scale=kwargs.get("ext_scale", 0.00035), centers=kwargs.get("centers"))
    boxes = (cyl_t, bboxes, [(None, None) + tuple(m) for m in meta]) if render_factor == 0 else None
    render_frames_device(render_poses, hwf, chunk, render_kwargs, render_factor=render_factor, boxes=boxes,
                         frame_sink=scorer.sink(img_idxs, [bboxes[i] for i in ids]), **kwargs)
    return validation_scores(scorer.sums(), use_masks, eval_both)
