"""Scoring rendered frames on the device: the reference's two `evaluate_metric` functions -- `run_render.py --eval`
(run_render.py:888-974: every frame inside its 2-D box) and the trainer's validation render
(core/utils/evaluation_helpers.py:257-385: whole frames) -- PSNR, SSIM and their foreground-masked variants against the
ground truth of a `DeviceImageBank`.

The reference scores on the host: every frame is downloaded, and an 11 x 11 Gaussian runs over five moment images per frame on the
CPU.  Here a frame stays where `render_frames_device` left it; `pg_frame_metrics` (csrc/pg_metrics.hip) reduces it, the bank's
bytes and the box to eight float64 sums on the device, and the sums of all frames come back in one copy (`FrameScorer`).  There is
no torch fallback.

The trainer's own call -- `render_testset(..., eval_metrics=True, eval_both=True)` at `args.render_factor` (run_nerf.py:586-589)
-- is `ValidationScorer`, `evaluate_validation` and `evaluate_testset` on `pg_frame_metrics_val`, which takes the frame at the size
it was rendered at, scores its bilinear upsampling to the bank's size (fused into the kernel's staging) and adds
the sums under each frame's 2-D box ("valid") to the foreground ones.

Both scorers are one class, `_SumsScorer`, with two row layouts (SUMS, SUMS_VAL) and two entry points; `evaluate_frames` and
`evaluate_testset` are one driver, `_render_scored`, with the scorer and the mapping of the sums as their own; `evaluate_metric`
and `evaluate_validation` map their sums by the one `validation_scores`.

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


class _SumsScorer:
    """What `FrameScorer` and `ValidationScorer` are: the sums of one entry point for a run of frames, a device float64
    [capacity, len(COLUMNS)] tensor, one row per frame, grown as needed.  `score` enqueues a frame on the current stream and never
    waits for the device, `sums()` makes the one copy back.  A subclass names itself (NAME, in messages), its row (COLUMNS) and its
    entry point (ENTRY), and has its own `score` and `sink`.

    `use_masks`: the foreground sums are wanted (refused for a bank without masks).  `background`: the ground truth of a pixel
    outside the mask is the image's background (run_render.py:935-937, PG_METRICS_BG); None = the bank has backgrounds."""
    NAME = ENTRY = ""
    COLUMNS: tuple = ()

    def __init__(self, bank, use_masks: bool = True, background: Optional[bool] = None, capacity: int = 64):
        who = self.NAME
        self.device = torch.device(bank.device)
        if self.device.type != "cuda":
            raise NotImplementedError(f"{who}: the bank is on {self.device}, not on a HIP device (torch 'cuda:N'); "
                                      f"frames are scored by {self.ENTRY} only, there is no CPU path")
        if use_masks and getattr(bank, "masks", None) is None:
            raise ValueError(f"{who}: masked scores asked for from a bank without masks (use_masks=False scores whole boxes only)")
        has_bg = getattr(bank, "bkgds", None) is not None
        if background and not has_bg:
            raise ValueError(f"{who}: background=True (PG_METRICS_BG) needs a bank with backgrounds")
        if background and getattr(bank, "masks", None) is None:
            raise ValueError(f"{who}: background=True (PG_METRICS_BG) needs a bank with masks")
        self.bank, self.use_masks = bank, bool(use_masks)
        self.flags = _ffi.PG_METRICS_BG if (has_bg if background is None else background) else 0
        self.capacity = max(int(capacity), 1)
        self._sums: Optional[torch.Tensor] = None
        self.n_frames = 0

    def _row(self, k: int) -> torch.Tensor:
        if self._sums is None or k >= self._sums.shape[0]:
            rows = max(self.capacity, k + 1, 0 if self._sums is None else 2 * self._sums.shape[0])
            grown = torch.zeros(rows, len(self.COLUMNS), dtype=torch.float64, device=self.device)
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

    def _check_frame(self, k: int, rgb: torch.Tensor):
        """what both entry points ask of a frame whose shape has been accepted"""
        if rgb.device != self.device:
            raise NotImplementedError(f"{self.NAME}: the frame is on {rgb.device}, the bank on {self.device}; there is no CPU path")
        if rgb.dtype != torch.float32 or not rgb.is_contiguous():
            raise TypeError(f"{self.NAME}: the frame must be a contiguous float32 tensor")
        if k < 0:
            raise IndexError(f"{self.NAME}: row {k}")

    def _enqueue(self, k: int, img_idx: int, box, rgb: torch.Tensor, *resampling):
        """ENTRY(handle, stream, bank, img_idx, box, rgb, *resampling, flags, row k) on the current stream"""
        r = self.bank.renderer
        with torch.cuda.device(self.device):
            row = self._row(int(k))
            _ffi.call(r, self.ENTRY, C.byref(self._struct()), int(img_idx), box, rgb, *resampling, self.flags, row)
        self.n_frames = max(self.n_frames, int(k) + 1)

    def sums(self) -> np.ndarray:
        """float64 [n_frames, len(COLUMNS)]: the COLUMNS of every frame scored so far"""
        if self._sums is None:
            return np.zeros((0, len(self.COLUMNS)), dtype=np.float64)
        return self._sums[:self.n_frames].cpu().numpy()


def _box4(who, box):
    bx = np.asarray([np.asarray(b).reshape(-1) for b in box] if len(box) == 2 else box).reshape(-1)
    if bx.size != 4:
        raise ValueError(f"{who}: a box is ((tl_x, tl_y), (br_x, br_y)) or (x0, y0, x1, y1)")
    return (C.c_int32 * 4)(*(int(v) for v in bx))


class FrameScorer(_SumsScorer):
    """The eight sums of `pg_frame_metrics` (SUMS) for a run of frames of the bank's size, each inside a box."""
    NAME, COLUMNS, ENTRY = "FrameScorer", SUMS, "pg_frame_metrics"

    def score(self, k: int, rgb: torch.Tensor, img_idx: int, box):
        """Frame `rgb` (device float32 [H,W,3], H W = the bank's) against image `img_idx` of the bank inside `box` =
        ((tl_x, tl_y), (br_x, br_y)) or (x0, y0, x1, y1), into row k."""
        H, W = self.bank.HW
        if not torch.is_tensor(rgb) or tuple(rgb.shape) != (H, W, 3):
            raise ValueError(f"FrameScorer: a frame of shape {tuple(getattr(rgb, 'shape', ()))} against a bank of {H} x {W} images "
                             "(a render_factor other than 0 resamples the frame: not built)")
        self._check_frame(k, rgb)
        self._enqueue(k, img_idx, _box4("FrameScorer", box), rgb)

    def sink(self, img_idxs, bboxes):
        """A `frame_sink(k, rgb, disp, acc)` for `render_frames_device`: frame k is scored against image img_idxs[k] in bboxes[k]."""
        img_idxs = [int(i) for i in np.asarray(img_idxs).reshape(-1)]

        def frame_sink(k, rgb, disp, acc):
            self.score(k, rgb, img_idxs[k], bboxes[k])
        return frame_sink


class ValidationScorer(_SumsScorer):
    """The twelve sums of `pg_frame_metrics_val` (SUMS_VAL) for a run of frames of the trainer's validation render: `score` takes
    the frame at the size it was rendered at (h <= H, w <= W: it is scored as its bilinear upsampling to the bank's H x W).  The
    trainer's ground truth is gt * mask + (1 - mask) * bg (run_nerf.py:580-583): `background=None` on a bank with backgrounds."""
    NAME, COLUMNS, ENTRY = "ValidationScorer", SUMS_VAL, "pg_frame_metrics_val"

    def score(self, k: int, rgb: torch.Tensor, img_idx: int, valid_box=None, box=None):
        """Frame `rgb` (device float32 contiguous [h,w,3], h <= H, w <= W) against image `img_idx` of the bank into row k: the
        eight sums inside `box` (None: the whole frame) and the four under `valid_box` (None: 0).  Both boxes are in the bank's
        pixels, ((tl_x, tl_y), (br_x, br_y)) or (x0, y0, x1, y1)."""
        H, W = self.bank.HW
        shape = tuple(getattr(rgb, "shape", ()))
        if not torch.is_tensor(rgb) or len(shape) != 3 or shape[2] != 3 or not (1 <= shape[0] <= H and 1 <= shape[1] <= W):
            raise ValueError(f"ValidationScorer: a frame of shape {shape} against a bank of {H} x {W} images (a frame is [h,w,3] with "
                             "1 <= h <= H and 1 <= w <= W: it is upsampled, never downsampled)")
        self._check_frame(k, rgb)
        bx = _box4("ValidationScorer", (0, 0, W, H) if box is None else box)
        vb = None if valid_box is None else _box4("ValidationScorer", valid_box)
        self._enqueue(k, img_idx, bx, rgb, int(shape[0]), int(shape[1]), vb)

    def sink(self, img_idxs, valid_boxes=None):
        """A `frame_sink(k, rgb, disp, acc)` for `render_frames_device`: frame k is scored whole against image img_idxs[k], with
        valid_boxes[k] as its valid rectangle."""
        img_idxs = [int(i) for i in np.asarray(img_idxs).reshape(-1)]

        def frame_sink(k, rgb, disp, acc):
            self.score(k, rgb, img_idxs[k], None if valid_boxes is None else valid_boxes[k])
        return frame_sink


def box_scores(sums: np.ndarray, use_masks: bool = True):
    """The reference's per-frame values (run_render.py:947-964) from the sums [F,8] -> dict of float64 [F] arrays.  Frames below the
    window have NaN SSIM entries."""
    s = {k: sums[:, i] for i, k in enumerate(SUMS)}
    out = {"psnr": _psnr(_ratio(s["se"], s["n"])), "ssim": _ratio(s["ssim"], s["n_map"])}
    if use_masks:
        out["fg_psnr"] = _psnr(_ratio(s["se_fg"], s["n_fg"]))
        out["fg_ssim"] = _ratio(s["ssim_fg"], s["n_fg_map"])
    return out


def validation_scores(sums: np.ndarray, use_masks: bool = True, eval_both: bool = False):
    """{"psnr", "ssim", "psnr_fg", "ssim_fg"} from the sums [F,12] or [F,8] as evaluation_helpers.py:296-385 maps them: with masks,
    images without a mask pixel are removed first (:296-305); denominators max(., 1) (:325, :336), inf -> 0, means over frames; with
    `eval_both` (twelve sums only) "psnr" / "ssim" are the valid values (:372-373), without it the foreground values (:363-364);
    without masks the averages over all pixels (:346-353) and None for the "_fg" pair.  No frame left: None.

    inf -> 0 is applied to every value, also to the unmasked SSIM mean, which the reference takes as it is (:352).  It changes
    nothing there: ssim / n_map is inf only for n_map = 0 with ssim != 0, and the kernel writes n_map = 0 only for a box below the
    window, which has no map and the map sum 0.0 -- 0 / 0, NaN either way."""
    s = np.asarray(sums, dtype=np.float64)
    width = s.shape[-1] if s.ndim else 0
    if width not in (len(SUMS), len(SUMS_VAL)):
        raise ValueError(f"validation_scores: sums of shape {s.shape}, not [F,{len(SUMS)}] or [F,{len(SUMS_VAL)}]")
    s = s.reshape(-1, width)
    if eval_both and not use_masks:
        raise ValueError("eval_both needs masks (the reference's lines raise a NameError on fg_psnr without gt_masks)")
    if eval_both and width != len(SUMS_VAL):
        raise ValueError(f"eval_both needs the valid sums: [F,{len(SUMS_VAL)}] (ValidationScorer), not [F,{width}]")

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


def _refuse_resampling(who, render_factor):
    if render_factor:
        raise NotImplementedError(f"{who}: render_factor = {render_factor} resamples the frames against the ground truth "
                                  "(F.interpolate in the reference): not built, render at the bank's frame size")


def _device_frames(who, rgbs, img_idxs, device):
    """`rgbs` [F,...] (numpy or a tensor) as a contiguous float32 tensor on `device`, and the F image indices as an int array"""
    img_idxs = np.asarray(img_idxs).reshape(-1)
    if len(img_idxs) != len(rgbs):
        raise ValueError(f"{who}: {len(img_idxs)} image indices for {len(rgbs)} frames")
    if not torch.is_tensor(rgbs):
        rgbs = torch.from_numpy(np.ascontiguousarray(rgbs, dtype=np.float32))
    return rgbs.to(device=device, dtype=torch.float32).contiguous(), img_idxs


def _render_scored(who, scorer_cls, render_poses, hwf, chunk, render_kwargs, bank, img_idxs, use_masks, background, render_factor, kwargs):
    """What `evaluate_frames` and `evaluate_testset` share: frame k of `render_frames_device(render_poses, hwf, chunk,
    render_kwargs, render_factor=render_factor, **kwargs)` goes to the sink of a `scorer_cls` as soon as its kernels are enqueued,
    with image img_idxs[k] and the frame's 2-D box at the bank's resolution, and is never downloaded.  At render_factor = 0 those
    boxes are the renderer's as well, computed once.  Returns the scorer's sums."""
    from .rays import frame_boxes
    from .render import _caster_device, _scalar_hw, render_frames_device
    for key in ("ret_acc", "gt_imgs", "bones", "base_bg"):       # render_path's, without meaning for frames that stay on the device
        kwargs.pop(key, None)
    for key in ("frame_sink", "boxes"):
        if kwargs.get(key) is not None:
            raise ValueError(f"{who}: {key} is this function's own")
    H, W, focal = hwf
    if not _scalar_hw(H, W) or (int(H), int(W)) != tuple(bank.HW):
        raise ValueError(f"{who}: frames of {H} x {W} (hwf, before any render_factor) against a bank of {bank.HW[0]} x {bank.HW[1]} images")
    scorer = scorer_cls(bank, use_masks=use_masks, background=background)
    r, dev = _caster_device(render_kwargs["ray_caster"])
    if torch.device(dev) != scorer.device:
        raise ValueError(f"{who}: the renderer is on {dev}, the bank on {scorer.device}")
    kp, cyls = kwargs.get("kp"), kwargs.get("cyls")
    if kp is None and cyls is None:
        raise NotImplementedError("render_path needs kp or cyls (bounding-cylinder cull)")
    ids = kwargs.get("frame_ids")
    ids = list(range(len(render_poses))) if ids is None else list(ids)
    img_idxs = np.asarray(img_idxs).reshape(-1)
    if len(img_idxs) != len(ids):
        raise ValueError(f"{who}: {len(img_idxs)} image indices for {len(ids)} frames")
    if len(img_idxs) and (img_idxs.min() < 0 or img_idxs.max() >= bank.F):
        raise IndexError(f"{who}: an image index is outside [0, {bank.F})")
    cyl_t, bboxes, meta = frame_boxes(r, render_poses, int(H), int(W), focal, kps=kp, cylinder_params=cyls,
                                      ext_scale=kwargs.get("ext_scale", 0.00035), centers=kwargs.get("centers"))
    boxes = (cyl_t, bboxes, [(None, None) + tuple(m) for m in meta]) if render_factor == 0 else None
    render_frames_device(render_poses, hwf, chunk, render_kwargs, render_factor=render_factor, boxes=boxes,
                         frame_sink=scorer.sink(img_idxs, [bboxes[i] for i in ids]), **kwargs)
    return scorer.sums()


@torch.no_grad()
def evaluate_frames(render_poses, hwf, chunk, render_kwargs, bank, img_idxs, basedir=None, use_masks=True, background=None,
                    **kwargs):
    """`run_render.py`'s render followed by `evaluate_metric` (run_render.py:888-974): frame k of `render_frames_device(render_poses,
    hwf, chunk, render_kwargs, **kwargs)` is scored inside its 2-D box against image img_idxs[k] of `bank` as soon as its kernels
    are enqueued, and never downloaded.  Returns the reference's score dict {'psnr', 'ssim', 'fg_psnr', 'fg_ssim'} as lists over
    frames; a frame whose box holds no mask pixel is left out of all four (the reference's `continue`), a frame whose box is below
    11 pixels has NaN SSIM entries, inf stays inf.  With `basedir`, scores.npy and score_final.txt are written as the reference does.
    `use_masks=False`: no foreground lists (the reference without gt masks)."""
    _refuse_resampling("evaluate_frames", kwargs.pop("render_factor", 0))
    sums = _render_scored("evaluate_frames", FrameScorer, render_poses, hwf, chunk, render_kwargs, bank, img_idxs, use_masks, background,
                          0, kwargs)
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
    ground-truth images as they are).  Returns `validation_scores` of the eight sums: {"psnr", "ssim", "psnr_fg", "ssim_fg"} as
    means over frames.  Not built here: eval_both and render_factor > 0 (`evaluate_validation` takes both)."""
    if eval_both:
        raise NotImplementedError("evaluate_metric: eval_both weights a whole-frame SSIM map by each frame's box mask: not built "
                                  "(evaluate_frames scores inside the box)")
    _refuse_resampling("evaluate_metric", render_factor)
    scorer = FrameScorer(bank, use_masks=use_masks, background=False)
    H, W = bank.HW
    if len(np.shape(rgbs)) != 4 or tuple(np.shape(rgbs)[1:]) != (H, W, 3):
        raise ValueError(f"evaluate_metric: frames of shape {tuple(np.shape(rgbs))} against a bank of {H} x {W} images")
    rgbs, img_idxs = _device_frames("evaluate_metric", rgbs, img_idxs, scorer.device)
    for k in range(len(rgbs)):
        scorer.score(k, rgbs[k], int(img_idxs[k]), (0, 0, W, H))
    return validation_scores(scorer.sums(), use_masks, eval_both=False)


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
    if valid_boxes is not None and len(valid_boxes) != shape[0]:
        raise ValueError(f"evaluate_validation: {len(valid_boxes)} valid boxes for {shape[0]} frames")
    rgbs, img_idxs = _device_frames("evaluate_validation", rgbs, img_idxs, scorer.device)
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
    if eval_both and not use_masks:
        raise ValueError("evaluate_testset: eval_both needs masks (the reference's lines raise a NameError on fg_psnr without gt_masks)")
    render_factor = int(render_factor)
    if render_factor < 0:
        raise ValueError(f"evaluate_testset: render_factor = {render_factor}")
    if render_factor > min(bank.HW):
        raise ValueError(f"evaluate_testset: render_factor = {render_factor} leaves no pixel of a {bank.HW[0]} x {bank.HW[1]} frame")
    sums = _render_scored("evaluate_testset", ValidationScorer, render_poses, hwf, chunk, render_kwargs, bank, img_idxs, use_masks,
                          background, render_factor, kwargs)
    return validation_scores(sums, use_masks, eval_both)
