"""Several posed people in one frame, in front of and behind each other (pg_render_scene, include/posegen_hip.h).

The subject bank renders one character per FRAME; a scene renders P characters of the bank into the SAME frame with correct mutual
occlusion, and says how much of each of them is visible (`person_acc`).  Every person is rendered over its own 2-D box exactly as
`render_frame` renders it; the library keeps the per-ray sample lists and merges them per pixel by depth (all people share one
camera).  The reference has no counterpart: its frames hold one character.

`render_scene` is one frame on the device (also `HipRenderer.render_scene`), `render_scenes` a path of frames with `render_path`'s
conventions, `place_people` moves characters posed at the root apart.

Out of scope: casters on several devices, gradients through a scene (training mode), summed densities of overlapping fields,
shadows, more than PG_SCENE_MAX_PEOPLE people.
"""
from __future__ import annotations

import ctypes as C
from typing import NamedTuple, Optional

import numpy as np
import torch

from . import _ffi
from .raycaster import _check_subject_range, _resolve_sn, _subject_values
from .render import _caster_device, frame_background, emit_frame, frame_setup, frame_stacks, frames_to_host

MAX_PEOPLE = _ffi.PG_SCENE_MAX_PEOPLE


class ScenePerson(NamedTuple):
    """One person of a scene: skts [24,4,4], cyl [5] (tensors), box ((tl_x, tl_y), (br_x, br_y)), the subject of the bank
    (None: the selected one) and the frame-code index (None: the mean code)."""
    skts: torch.Tensor
    cyl: torch.Tensor
    box: tuple
    subject: Optional[int] = None
    cam: Optional[float] = None


def _refuse(caster, who):
    """what a scene is not built for, before any library call: a caster on several devices, training mode"""
    inner = getattr(caster, "module", caster)
    r = getattr(inner, "renderer", inner)
    if getattr(r, "n_devices", 1) > 1:
        raise NotImplementedError(f"{who}: a caster on several devices is not supported (a scene renders on one device; build a "
                                  "one-device caster for it)")
    if getattr(inner, "training", False):
        raise NotImplementedError(f"{who}: training mode is not supported (no gradient flows through a scene); call .eval() first")
    return r


def _as_person(p) -> ScenePerson:
    return p if isinstance(p, ScenePerson) else (ScenePerson(**p) if isinstance(p, dict) else ScenePerson(*p))


def render_scene(renderer, H: int, W: int, focal, c2w, people, center=None, near: float = 0., far: float = 1.,
                 n_samples: Optional[int] = None, n_importance: Optional[int] = None, lindisp: bool = False,
                 bg: Optional[torch.Tensor] = None, base_bg: float = 0., want_uint8: bool = False,
                 want_person_acc: bool = False, return_lists: bool = False):
    """One frame with `people` (ScenePerson, or dicts / tuples of its fields) entirely on the device (pg_render_scene).
    Returns device tensors (rgb [H,W,3], disp [H,W,1], acc [H,W,1]), then, as asked for and in this order: rgb8 uint8 [H,W,3],
    person_acc [P,H,W] (the visible coverage of each person; 0 outside its box), lists = [(z [n_p,S_f], raw [n_p,S_f,4]) per
    person] -- the sample lists the frame was composited from, rows = the pixels of the person's clipped box, row-major.
    `renderer`: a HipRenderer (or a caster that owns one)."""
    r = _refuse(renderer, "render_scene")
    people = [_as_person(p) for p in people]
    P = len(people)
    if not 1 <= P <= MAX_PEOPLE:
        raise ValueError(f"render_scene: {P} people (1..{MAX_PEOPLE})")
    subj = np.array([r.selected_subject if p.subject is None else int(_subject_values(p.subject, "subject")[0]) for p in people])
    _check_subject_range(subj, r.n_subjects, "subject")
    S, N = _resolve_sn(r.cfg, n_samples, n_importance)
    H, W = int(H), int(W)
    c2w_h, intr, _ = r._frame_args(H, W, focal, c2w, ((0, 0), (0, 0)), center)
    arr = (_ffi.PgScenePerson * P)()
    keep, n_rows = [], []
    for k, p in enumerate(people):
        sk, _ = r._pose_args(p.skts, 1)
        cy, _ = r._cyl_args(p.cyl, 1)
        keep.append((sk, cy))
        (tlx, tly), (brx, bry) = p.box
        bx = (int(tlx), int(tly), int(brx), int(bry))
        arr[k].subject = int(subj[k])
        arr[k].box = (C.c_int32 * 4)(*bx)
        arr[k].skts, arr[k].cyl = sk.data_ptr(), cy.data_ptr()
        arr[k].cam = -1.0 if p.cam is None else float(p.cam)
        n_rows.append(max(min(bx[2], W) - max(bx[0], 0), 0) * max(min(bx[3], H) - max(bx[1], 0), 0))
    rgb, disp, acc, rgb8, bgt = r._frame_outputs(H, W, bg, want_uint8)
    pacc = torch.empty(P, H, W, device=r.device) if want_person_acc else None
    lists, lp = None, None
    if return_lists:
        lists = [(torch.empty(n, S + N, device=r.device), torch.empty(n, S + N, 4, device=r.device)) for n in n_rows]
        lp = (C.c_void_p * (2 * P))(*[t.data_ptr() for zr in lists for t in zr])
    _ffi.call(r, "pg_render_scene", H, W, c2w_h.ctypes.data_as(C.POINTER(C.c_float)), intr, float(near), float(far), P, arr, S, N,
              _ffi.PG_FLAG_LINDISP if lindisp else 0, bgt, float(base_bg), rgb, disp, acc, rgb8, pacc, lp)
    out = (rgb, disp, acc)
    for want, x in ((want_uint8, rgb8), (want_person_acc, pacc), (return_lists, lists)):
        if want:
            out += (x,)
    return out


def stage_scene_composite(renderer, z, raw, rows, dirs, want_person_acc=True, fill=None):
    """scene_composite_kernel on the caller's lists (pg_stage_scene_composite): z / raw = P device tensors [n_p,S] / [n_p,S,4],
    rows int32 [P,n_pix] (outside [0, n_p): absent), dirs [n_pix,3].  Returns a dict of device tensors rgb_map [n_pix,3], disp_map,
    acc_map [n_pix] (, person_acc [P,n_pix]).  The density line follows the renderer's config.  `fill`: the outputs are prefilled
    with this value (a test's sentinel) instead of left uninitialised."""
    r = renderer
    dev = r.device
    P = len(z)
    z = [t.to(dev, torch.float32).contiguous() for t in z]
    raw = [t.to(dev, torch.float32).contiguous() for t in raw]
    rows = rows.to(dev, torch.int32).contiguous()
    dirs = dirs.to(dev, torch.float32).contiguous()
    n, S = int(dirs.shape[0]), int(z[0].shape[1])
    assert rows.shape == (P, n) and all(t.shape[1] == S for t in z)
    new = (lambda *shape: torch.empty(*shape, device=dev)) if fill is None else (lambda *shape: torch.full(shape, float(fill), device=dev))
    out = {"rgb_map": new(n, 3), "disp_map": new(n), "acc_map": new(n)}
    if want_person_acc:
        out["person_acc"] = new(P, n)
    vp = lambda ts: (C.c_void_p * P)(*[t.data_ptr() for t in ts])
    _ffi.call(r, "pg_stage_scene_composite", n, P, S, vp(z), vp(raw), (C.c_int64 * P)(*[int(t.shape[0]) for t in z]), rows, dirs,
              out["rgb_map"], out["disp_map"], out["acc_map"], out.get("person_acc"))
    return out


def place_people(kps, skts, offsets):
    """Characters posed at the root, moved apart: kps [P,24,3], skts [P,24,4,4] (world -> bone), offsets [P,3] (world) ->
    (kps + offset, skts @ T(-offset)), so that skt' [kp' ; 1] = skt [kp ; 1].  Tensors in, tensors out (numpy in, numpy out)."""
    as_np = not torch.is_tensor(kps)
    kp_t, sk_t = torch.as_tensor(kps), torch.as_tensor(skts)
    off = torch.as_tensor(offsets).to(kp_t.dtype).reshape(-1, 1, 3)
    if not (kp_t.shape[0] == sk_t.shape[0] == off.shape[0]):
        raise ValueError(f"place_people: {kp_t.shape[0]} kps / {sk_t.shape[0]} skts / {off.shape[0]} offsets")
    T = torch.eye(4, dtype=sk_t.dtype).repeat(off.shape[0], 1, 1, 1)
    T[:, 0, :3, 3] = -off[:, 0].to(sk_t.dtype)
    kp2, sk2 = kp_t + off, sk_t @ T
    return (kp2.numpy(), sk2.numpy()) if as_np else (kp2, sk2)


def _scene_subjects(r, subject_idxs, F, P):
    """[F,P] subjects from None | [P] | [F,P]"""
    if subject_idxs is None:
        return None
    a = np.asarray(torch.as_tensor(subject_idxs).detach().cpu())
    flat = _subject_values(a, "subject_idxs")
    _check_subject_range(flat, r.n_subjects)
    if a.shape == (P,):
        return np.broadcast_to(flat.reshape(1, P), (F, P))
    if a.shape == (F, P):
        return flat.reshape(F, P)
    raise ValueError(f"subject_idxs must be [P] = [{P}] or [F,P] = [{F},{P}], got {list(a.shape)}")


@torch.no_grad()
def render_scenes(render_poses, hwf, chunk, render_kwargs, kp=None, skts=None, subject_idxs=None, cams=None, bg_imgs=None,
                  bg_indices=None, white_bkgd=False, ret_acc=False, ret_person_acc=False, ext_scale=0.00035, render_factor=0):
    """F frames of P people each, with render_path's conventions: render_poses [F,4,4], hwf = (H, W, focal), `chunk` = the nanmean
    group size, render_kwargs holds the caster and N_samples / N_importance / lindisp; kp [F,P,24,3], skts [F,P,24,4,4];
    subject_idxs None | [P] | [F,P]; cams (frame-code indices) None | [F,P].  Returns numpy (rgbs [F,H,W,3], disps [F,H,W,1],
    accs [F,H,W,1] or [] without ret_acc, person_accs [F,P,H,W] or [] without ret_person_acc, bboxes = per frame the P (tl, br))."""
    caster = render_kwargs["ray_caster"]
    _refuse(caster, "render_scenes")
    if kp is None or skts is None:
        raise ValueError("render_scenes needs kp [F,P,24,3] and skts [F,P,24,4,4]")
    kp_t, sk_t = torch.as_tensor(kp), torch.as_tensor(skts)
    F_, P = int(kp_t.shape[0]), int(kp_t.shape[1])
    if len(render_poses) != F_ or tuple(sk_t.shape[:2]) != (F_, P):
        raise ValueError(f"render_scenes: {len(render_poses)} poses, kp {list(kp_t.shape)}, skts {list(sk_t.shape)}")
    if not 1 <= P <= MAX_PEOPLE:
        raise ValueError(f"render_scenes: {P} people per frame (1..{MAX_PEOPLE})")

    def driver(frame_sink):
        # one box per (frame, person): the frame's camera P times over, frame_boxes (in frame_setup) does the rest
        poses = [render_poses[f] for f in range(F_) for _ in range(P)]
        H, W, focal = hwf
        foc = focal if isinstance(focal, float) or np.ndim(focal) == 0 else np.repeat(np.asarray(focal), P, axis=0)
        su = frame_setup(poses, (H, W, foc), render_kwargs, None, kp_t.reshape(F_ * P, 24, 3), None, render_factor, ext_scale)
        r, dev = su.r, su.dev
        subj = _scene_subjects(r, subject_idxs, F_, P)
        cm = None if cams is None else np.asarray(torch.as_tensor(cams).detach().float().cpu()).reshape(F_, P)
        r.set_chunk(int(chunk))
        sk_d = sk_t.to(dev, dtype=torch.float32)
        cy_d = torch.as_tensor(su.cyls).to(dev, dtype=torch.float32)
        kw = render_kwargs
        frames, paccs = [], []
        for f in range(F_):
            h, w, fo, c2w_np, center = su.meta[f * P]
            people = [ScenePerson(sk_d[f, p], cy_d[f * P + p], su.bboxes[f * P + p], None if subj is None else int(subj[f, p]),
                                  None if cm is None else float(cm[f, p])) for p in range(P)]
            res = render_scene(r, h, w, fo, c2w_np, people, center=center, n_samples=kw.get("N_samples"),
                               n_importance=kw.get("N_importance"), lindisp=bool(kw.get("lindisp", False)),
                               bg=frame_background(bg_imgs, bg_indices, f, h, w, white_bkgd, dev),
                               base_bg=1.0 if white_bkgd else 0.0, want_person_acc=ret_person_acc)
            if ret_person_acc:
                paccs.append(res[3])
            emit_frame(frame_sink, frames, f, *res[:3])
        boxes = [[su.bboxes[f * P + p] for p in range(P)] for f in range(F_)]
        return frame_stacks(frame_sink, frames, su) + (paccs, boxes)

    rgbs, disps, accs, paccs, boxes = frames_to_host(driver, render_kwargs, hwf, F_, render_factor, ret_acc)
    return rgbs, disps, accs, (torch.stack(paccs).cpu().numpy() if ret_person_acc and paccs else []), boxes
