"""HIP-backed drop-in for the reference's `RayCaster` (core/raycasters.py:326-794).

`HipRenderer` is a typed wrapper around one `pg_handle` (device memory and streams
come from PyTorch-ROCm: plumbing only).  `HipRayCaster` is the duck-typed object the
reference stores under ``render_kwargs['ray_caster']`` and calls at
core/trainer.py:74: same call signature, same returned dict keys
(`_collect_outputs`, raycasters.py:711-724), same checkpoint key scheme
(`state_dict` / `load_state_dict`, raycasters.py:752-788).

Forward values only (no autograd graph): the training step with a gradient is `train.TrainableRayCaster`,
which wraps a `HipRayCaster`.  Eval mode is the measured path; the training-mode
arguments (perturb, raw_noise_std, ray_noise_std, pytest) are honoured with the random numbers
drawn on the host side of the ABI (`training_draws`, pg_train_draws).

Every ray-level call (render_rays, the training forward, stage_eval) is marshalled by `marshal_ray_call`; the
reference's keywords the kernels do not honour are refused by `refuse_reference_kwargs`, for both casters.
"""
from __future__ import annotations

import ctypes as C
from contextlib import contextmanager
from typing import Dict, NamedTuple, Optional

import numpy as np
import torch

from . import _ffi
from .config import PREC_BF16, PREC_BY_NAME, PREC_NAMES, RenderConfig
from .rays import _focal_xy

NET_TENSOR_ORDER = ([f"pts_linears.{l}.{k}" for l in range(8) for k in ("weight", "bias")]
                    + [f"{n}.{k}" for n in ("alpha_linear", "feature_linear", "views_linears.0", "rgb_linear")
                       for k in ("weight", "bias")])


def _density_act(density_type: str) -> int:
    """--density_type -> PG_ACT_* (get_density_fn, core/raycasters.py:230-238 raises on anything else)."""
    try:
        return {"relu": _ffi.PG_ACT_RELU, "softplus": _ffi.PG_ACT_SOFTPLUS}[density_type]
    except KeyError:
        raise NotImplementedError(f"density activation {density_type} is undefined") from None


def _np32(x) -> np.ndarray:
    if isinstance(x, torch.Tensor):
        x = x.detach().cpu().numpy()
    return np.ascontiguousarray(np.asarray(x), dtype=np.float32)


def _dev_f32(t: torch.Tensor, device) -> torch.Tensor:
    return t.to(device=device, dtype=torch.float32).contiguous()


def _net_key(which: int) -> str:
    """the reference checkpoint's key of net 0 (coarse) / 1 (fine)"""
    return "network_fn_state_dict" if which == 0 else "network_fine_state_dict"


def _resolve_sn(cfg: RenderConfig, n_samples, n_importance):
    """(S, N) of a call: the configuration's counts unless the caller gives its own"""
    return (cfg.n_samples if n_samples is None else int(n_samples),
            cfg.n_importance if n_importance is None else int(n_importance))


def _intrinsics(H, W, focal, center=None, f32_focal=False):
    """(fx, fy, cx, cy): one focal length serves both axes, the principal point defaults to the frame's centre.
    f32_focal: the focal lengths rounded through float32 (pose_boxes: nerf_c2w_to_extrinsic parity with the reference)."""
    fx, fy = _focal_xy(focal)
    if f32_focal:
        fx, fy = float(np.float32(fx)), float(np.float32(fy))
    cx, cy = (W * 0.5, H * 0.5) if center is None else (float(center[0]), float(center[1]))
    return fx, fy, cx, cy


def _per_ray(x: torch.Tensor, n: int, device, dims: int, stride: int, what: str):
    """[1|n, ...] (or one un-batched item of `dims` - 1 dimensions) -> (contiguous device tensor, stride in floats: 0 = one
    item for all rays).  `what`: the refusal's subject, e.g. "skts has {} poses"."""
    if x.dim() == dims - 1:
        x = x[None]
    if x.shape[0] == 1 or x.stride(0) == 0:
        return _dev_f32(x[:1], device), 0
    if x.shape[0] != n:
        raise ValueError(f"{what.format(x.shape[0])} for {n} rays")
    return _dev_f32(x, device), stride


MIXED_SUBJECTS = ("subject_idxs holds more than one subject in one ray call: per-ray mixing of subjects is not built (it would "
                  "split the call's nanmean groups); render each subject's rays in a call of their own, or render whole frames "
                  "with one subject per frame (render_path)")


def _subject_values(x, what="subject_idxs") -> np.ndarray:
    """int64 array of the subject indices in `x` (int, sequence, numpy array or tensor); anything that is not a whole number
    is a ValueError."""
    if isinstance(x, torch.Tensor):
        x = x.detach().cpu().numpy()
    if isinstance(x, (list, tuple)) and any(isinstance(v, (bool, np.bool_)) for v in x):
        raise ValueError(f"{what} must hold integer subject indices, not booleans")
    a = np.asarray(x)
    if a.dtype == np.bool_ or not (np.issubdtype(a.dtype, np.integer) or np.issubdtype(a.dtype, np.floating)):
        raise ValueError(f"{what} must hold integer subject indices, not {a.dtype}")
    if np.issubdtype(a.dtype, np.floating):
        if not np.all(np.isfinite(a)) or np.any(a != np.floor(a)):
            raise ValueError(f"{what} must hold integer subject indices, got non-integer values")
    return a.astype(np.int64).reshape(-1)


def _check_subject_range(a: np.ndarray, n_subjects: int, what="subject_idxs"):
    if a.size and (a.min() < 0 or a.max() >= n_subjects):
        bad = int(a.min()) if a.min() < 0 else int(a.max())
        raise ValueError(f"{what}: subject {bad} is outside [0, {n_subjects}) (the caster holds {n_subjects} subject"
                         f"{'s' if n_subjects != 1 else ''})")


def call_subject(subject_idxs, n_subjects: int, what="subject_idxs") -> Optional[int]:
    """The ONE subject of a ray-level call: None (the selected subject), an int, or an array / tensor whose entries are all
    equal -- what the reference's per-ray expansion of a frame's subject produces.  Mixed values are refused (MIXED_SUBJECTS),
    values outside [0, n_subjects) are a ValueError; both before anything is launched."""
    if subject_idxs is None:
        return None
    a = _subject_values(subject_idxs, what)
    if a.size == 0:
        return None
    if np.any(a != a[0]):
        raise NotImplementedError(MIXED_SUBJECTS)
    _check_subject_range(a[:1], n_subjects, what)
    return int(a[0])


def frame_subjects(subject_idxs, n_frames: int, n_subjects: int, what="subject_idxs") -> Optional[list]:
    """One subject per frame for the frame drivers: None, a scalar, [F], or [n_pose] indexed i % n_pose like every other
    per-pose argument.  Values outside [0, n_subjects) are a ValueError before anything is launched."""
    if subject_idxs is None:
        return None
    a = _subject_values(subject_idxs, what)
    if a.size == 0:
        raise ValueError(f"{what} is empty")
    _check_subject_range(a, n_subjects, what)
    return [int(a[i % a.size]) for i in range(n_frames)]


class RayCall(NamedTuple):
    """What the ABI needs for one ray-level call; the tensors live as long as this does."""
    rb: torch.Tensor                    # [n,11] ray batch (zero-padded)
    sk: torch.Tensor                    # pose(s) and their stride in floats
    ps: int
    cy: Optional[torch.Tensor]          # cylinder(s) and their stride
    cs: int
    cam: Optional[torch.Tensor]         # [n] frame-code index per ray
    S: int
    N: int
    flags: int
    draws: Optional[_ffi.PgTrainDraws]  # None: eval mode
    keep: list                          # every tensor a pointer above refers to

    @property
    def n(self) -> int:
        return self.rb.shape[0]


def marshal_ray_call(cfg: RenderConfig, device, ray_batch, skts, cyls=None, cams=None, n_samples=None, n_importance=None,
                     lindisp=False, draws=None) -> RayCall:
    """The one place where a caller's ray-level arguments become ABI arguments.  `draws`: any of t_rand [n,S],
    u_rand [n,N], noise0 [n,S], noise1 [n,S+N], ray_noise [n,S+N,3]; u_rand / noise1 are dropped when N = 0."""
    S, N = _resolve_sn(cfg, n_samples, n_importance)
    rb = _dev_f32(torch.as_tensor(ray_batch), device)
    n = rb.shape[0]
    if rb.dim() != 2 or rb.shape[1] < 8:
        raise ValueError("ray_batch must be [n, >=8] (o, d, near, far [, viewdir])")
    if rb.shape[1] != 11:
        pad = torch.zeros(n, 11, device=device)
        pad[:, :min(11, rb.shape[1])] = rb[:, :11]
        rb = pad
    skts = torch.as_tensor(skts).detach()
    sk, ps = _per_ray(skts, n, device, 4, 24 * 16, "skts has {} poses")
    cy, cs = (None, 0) if cyls is None else _per_ray(cyls, n, device, 2, 5, "cyls has {} rows")
    cam = None
    if cams is not None:
        cam = _dev_f32(torch.as_tensor(cams).reshape(-1), device)
        if cam.shape[0] == 1 and n > 1:
            cam = cam.expand(n).contiguous()
    keep = [rb, sk, cy, cam]
    pd = None
    if draws:
        shapes = {"t_rand": (n, S), "u_rand": (n, N), "noise0": (n, S), "noise1": (n, S + N), "ray_noise": (n, S + N, 3)}
        unknown = set(draws) - set(shapes)
        if unknown:
            raise ValueError(f"unknown draws {sorted(unknown)}; expected a subset of {sorted(shapes)}")
        pd = _ffi.PgTrainDraws()
        for k, shp in shapes.items():
            t = draws.get(k)
            if t is None or (N == 0 and k in ("u_rand", "noise1")):
                continue
            t = _dev_f32(t, device)
            if tuple(t.shape) != shp:
                raise ValueError(f"draws[{k!r}] must be {shp}, got {tuple(t.shape)}")
            keep.append(t)
            setattr(pd, k, t.data_ptr())
    return RayCall(rb, sk, ps, cy, cs, cam, S, N, _ffi.PG_FLAG_LINDISP if lindisp else 0, pd, keep)


def alloc_ray_outputs(n, S, N, device, want_alpha=True, extras=False):
    """The result tensors of one ray-level call -> (maps (+ alphas) dict, extras dict, PgOutputs pointing at them)."""
    new = lambda *s: torch.empty(*s, device=device, dtype=torch.float32)
    SF = S + N
    out = {"rgb_map": new(n, 3), "disp_map": new(n), "acc_map": new(n)}
    if want_alpha:
        out["alpha"] = new(n, SF)
    if N > 0:
        out.update({"rgb0": new(n, 3), "disp0": new(n), "acc0": new(n)})
        if want_alpha:
            out["alpha0"] = new(n, S)
    ex = {}
    if extras:
        ex = {"near_far": new(n, 2), "z_coarse": new(n, S), "raw_coarse": new(n, S, 4), "weights0": new(n, S)}
        if N > 0:
            ex.update({"z_fine": new(n, SF), "raw_fine": new(n, SF, 4)})
    po = _ffi.PgOutputs()
    for k in ("rgb_map", "disp_map", "acc_map", "alpha", "rgb0", "disp0", "acc0", "alpha0"):
        setattr(po, k, out[k].data_ptr() if k in out else None)
    for k in ("near_far", "z_coarse", "z_fine", "raw_coarse", "raw_fine", "weights0"):
        setattr(po, k, ex[k].data_ptr() if k in ex else None)
    return out, ex, po


@contextmanager
def one_nanmean_group(renderer, n, grouped=False):
    """One call = one nanmean group, like get_near_far_in_cylinder on the reference's ray_batch (ray_utils.py:292-344):
    only batchify_rays / render_path split a frame into `chunk` groups (`grouped`: keep theirs).  The group size is a
    property of THIS call: the renderer's own setting (what later direct render_rays / render_frame calls see) is put
    back afterwards."""
    keep = renderer._chunk
    if not grouped:
        renderer.set_chunk(max(int(n), 1))
    try:
        yield
    finally:
        renderer.set_chunk(keep)


class HipRenderer:
    """Owns a pg_handle on one HIP device."""

    def __init__(self, cfg: RenderConfig, device="cuda:0", precision=PREC_BF16, devices=None):
        """`devices`: HIP device indices for in-process multi-GPU frame rendering (render_frames /
        render_path); the first one is `device`, where every ray-level call runs.  An index may
        repeat (two workers on one GPU)."""
        if isinstance(precision, str):
            precision = PREC_BY_NAME[precision]
        self.cfg = cfg
        if devices is not None:
            devices = [int(torch.device(d).index) if not isinstance(d, int) else int(d) for d in devices]
            device = f"cuda:{devices[0]}"
        self.device = torch.device(device)
        if self.device.type != "cuda":
            raise _ffi.HipLibraryError("HipRenderer needs a HIP device (torch device 'cuda:N'); "
                                       "the render path has no CPU fallback")
        self.lib = _ffi.load_library()
        self.precision = int(precision)
        pc = _ffi.PgConfig(n_joints=cfg.n_joints, multires=cfg.multires, multires_views=cfg.multires_views,
                           multires_bones=cfg.multires_bones, net_depth=cfg.net_depth, net_width=cfg.net_width,
                           skip_layer=cfg.skips[0], view_width=cfg.net_width // 2,
                           framecode_ch=cfg.framecode_ch, n_framecodes=cfg.n_framecodes, chunk=cfg.chunk,
                           precision=self.precision, cutoff_dist=cfg.cutoff_dist,
                           density_scale=cfg.density_scale, rgb_eps=cfg.rgb_eps,
                           softplus_shift=float(cfg.softplus_shift), density_act=_density_act(cfg.density_type),
                           single_net=1 if cfg.single_net else 0)
        idx = self.device.index if self.device.index is not None else torch.cuda.current_device()
        dev_ids = [idx] if devices is None else devices
        ids = (C.c_int * len(dev_ids))(*dev_ids)
        self.devices = list(dev_ids)
        h = C.c_void_p()
        rc = self.lib.pg_create(C.byref(pc), len(dev_ids), ids, C.byref(h))
        _ffi.check(self.lib, None, rc)
        self.handle = h
        # host-side bookkeeping PER SUBJECT: the state dicts kept for checkpoints, and those to fetch from their owner on demand
        # (load_network_device).  `_state` / `_state_lazy` are the selected subject's.
        self._subjects = [{"state": {}, "lazy": {}}]
        self._subject = 0
        self._chunk = cfg.chunk
        self._wave_counts = None

    # -- lifetime ---------------------------------------------------------------------
    def close(self):
        if getattr(self, "handle", None):
            self.lib.pg_destroy(self.handle)
            self.handle = None

    def __del__(self):  # pragma: no cover
        try:
            self.close()
        except Exception:
            pass

    def _check(self, rc):
        _ffi.check(self.lib, self.handle, rc)

    # -- the subject bank (pg_set_subject_count / pg_select_subject) -----------------
    @property
    def _state(self) -> Dict[str, dict]:
        return self._subjects[self._subject]["state"]

    @property
    def _state_lazy(self) -> Dict[str, object]:
        return self._subjects[self._subject]["lazy"]

    @property
    def n_subjects(self) -> int:
        return len(self._subjects)

    @property
    def selected_subject(self) -> int:
        return self._subject

    def set_subject_count(self, n: int):
        """n >= 1 complete models behind this handle.  Growing keeps the loaded subjects, shrinking frees the dropped ones
        (the selected subject must be one that stays)."""
        n = int(n)
        if n != len(self._subjects):
            self._check(self.lib.pg_set_subject_count(self.handle, n))
            del self._subjects[n:]
            while len(self._subjects) < n:
                self._subjects.append({"state": {}, "lazy": {}})

    def select_subject(self, s: int):
        """Every later call -- loads, embedder state, renders, density queries, state_dict -- acts on subject s.  A swap of
        host pointers in the library: nothing is packed, copied or waited for."""
        s = int(s)
        if not 0 <= s < len(self._subjects):
            raise ValueError(f"subject {s} is outside [0, {len(self._subjects)})")
        if s != self._subject:
            self._check(self.lib.pg_select_subject(self.handle, s))
            self._subject = s

    @contextmanager
    def subject(self, s: Optional[int]):
        """`with r.subject(s):` selects subject s and puts the previous selection back (None: leaves it alone)."""
        prev = self._subject
        if s is not None:
            self.select_subject(s)
        try:
            yield self
        finally:
            if s is not None:
                self.select_subject(prev)

    def subject_info(self, s: Optional[int] = None):
        """pg_subject_info: which nets of subject s are loaded, the device bytes of its packed images, images built so far."""
        ln, by, bu = C.c_int32(), C.c_int64(), C.c_int64()
        self._check(self.lib.pg_subject_info(self.handle, self._subject if s is None else int(s), C.byref(ln), C.byref(by), C.byref(bu)))
        return {"loaded_nets": [w for w in (0, 1) if ln.value >> w & 1], "image_bytes": by.value, "image_builds": bu.value}

    def _stream(self):
        return C.c_void_p(torch.cuda.current_stream(self.device).cuda_stream)

    # -- state ------------------------------------------------------------------------
    def load_network(self, which: int, sd: Dict[str, np.ndarray]):
        """which 0 = coarse ('network_fn_state_dict'), 1 = fine ('network_fine_state_dict').  With multires_views = 0 the
        view weight keeps the reference's [128, 256+72(+16)] shape here and in state_dict(); the library widens its copy."""
        arrs = [_np32(sd[k]) for k in NET_TENSOR_ORDER]
        ptrs = (C.c_void_p * len(arrs))(*[a.ctypes.data for a in arrs])
        shp = (C.c_int64 * (2 * len(arrs)))()
        for i, a in enumerate(arrs):
            shp[2 * i] = a.shape[0]
            shp[2 * i + 1] = a.shape[1] if a.ndim == 2 else 1
        self._check(self.lib.pg_load_weights(self.handle, which, ptrs, shp, len(arrs)))
        if self.cfg.framecode_ch > 0:
            codes = _np32(sd["framecodes.codes.weight"])
            self._check(self.lib.pg_set_framecodes(self.handle, which, codes.ctypes.data, codes.shape[0]))
        st = {k: torch.from_numpy(_np32(v).copy()) for k, v in sd.items()}
        self._state[_net_key(which)] = st
        if self.cfg.single_net:     # network_fine is network: the reference's checkpoint holds both keys (raycasters.py:751-766)
            self._state["network_fine_state_dict"] = st

    def load_network_device(self, which: int, tensors, codes=None, state_provider=None):
        """New values of an already loaded net from DEVICE tensors (pg_load_weights_device): `tensors` = the 24 parameters in
        NET_TENSOR_ORDER (contiguous fp32 on this device), `codes` the frame codes [n,16] when the config has them.  The packed
        images of the fast paths are re-formed on the device; nothing is copied to the host.  `state_provider()` must return the
        net's state dict (CPU tensors) when somebody asks this renderer for it (state_dict / parameters): until then the host
        copy kept for checkpoints is stale."""
        ts = [t.detach() for t in tensors]
        for t in ts:
            if not (t.is_cuda and t.dtype == torch.float32 and t.is_contiguous()):
                raise ValueError("load_network_device: contiguous float32 device tensors expected")
        ptrs = (C.c_void_p * len(ts))(*[t.data_ptr() for t in ts])
        cptr, ncodes = None, 0
        if self.cfg.framecode_ch > 0:
            codes = codes.detach()
            if not (codes.is_cuda and codes.dtype == torch.float32 and codes.is_contiguous()):
                raise ValueError("load_network_device: contiguous float32 device frame codes expected")
            cptr, ncodes = codes.data_ptr(), codes.shape[0]
        _ffi.call(self, "pg_load_weights_device", which, ptrs, len(ts), cptr, ncodes)
        self._state_lazy[_net_key(which)] = state_provider

    def _refresh_state(self):
        """the host-side state dicts brought up to date after device-side weight loads"""
        for key, provider in list(self._state_lazy.items()):
            if provider is not None:
                self._state[key] = {k: v.detach().cpu().clone() for k, v in provider().items()}
                if self.cfg.single_net and key == "network_fn_state_dict":      # (one net under both keys, as load_network keeps it)
                    self._state["network_fine_state_dict"] = self._state[key]
            del self._state_lazy[key]

    def set_embedder(self, which: int, tau: float, cutoff_dist=None):
        """which 0 = embed_fn, 1 = embeddirs_fn (cutoff_embedder.py:89-94)."""
        cd = _np32(np.full(24, self.cfg.cutoff_dist) if cutoff_dist is None else cutoff_dist)
        self._check(self.lib.pg_set_embedder(self.handle, which, cd.ctypes.data, float(tau)))
        self._state["embed_state_dict" if which == 0 else "embeddirs_state_dict"] = {
            "cutoff_dist": torch.from_numpy(cd.copy()), "tau": torch.tensor(float(tau))}

    def set_precision(self, precision):
        if isinstance(precision, str):
            precision = PREC_BY_NAME[precision]
        self._check(self.lib.pg_set_precision(self.handle, int(precision)))
        self.precision = int(precision)

    def set_chunk(self, chunk: int):
        if int(chunk) != self._chunk:
            self._check(self.lib.pg_set_chunk(self.handle, int(chunk)))
            self._chunk = int(chunk)

    def set_onchip(self, mode="auto"):
        """Which form of the 16x16x32 kernel calls with >= 64 samples per ray take (pg_set_onchip): "records" (per-ray records in
        HBM), "auto" (on chip up to 112 samples per ray: the faster of the two, the default) or "always" (on chip whatever the
        sample count: no record workspace)."""
        modes = {"records": 0, "auto": 1, "always": 2, 0: 0, 1: 1, 2: 2}
        if mode not in modes:
            raise ValueError(f"set_onchip: mode must be 'records', 'auto' or 'always', not {mode!r}")
        self._check(self.lib.pg_set_onchip(self.handle, modes[mode]))

    def set_far_skip(self, on=True):
        """Test / measurement aid (pg_set_far_skip): off = the fused kernels compute every limb for every point."""
        self._check(self.lib.pg_set_far_skip(self.handle, 1 if on else 0))

    def set_empty_skip(self, on=True):
        """pg_set_empty_skip: off = the 16x16x32 kernel runs the colour branch for every wave, also for those whose points
        all have sigma <= 0 (tests, A/B; the maps are bitwise the same either way).  Default on."""
        self._check(self.lib.pg_set_empty_skip(self.handle, 1 if on else 0))

    def count_waves(self, on=True):
        """Measurement aid (pg_debug_wave_counts): while on, the render calls' own launches of the on-chip 16x16x32 form (one
        pose, no frame codes) count passes and empty / skipped waves; read_wave_counts() reads and clears."""
        self._wave_counts = torch.zeros(16, device=self.device, dtype=torch.int32) if on else None
        self._check(self.lib.pg_debug_wave_counts(self.handle, self._wave_counts.data_ptr() if on else None))

    def read_wave_counts(self):
        c = [int(v) for v in self._wave_counts.cpu()]
        self._wave_counts.zero_()
        return _wave_stats(c)

    def set_train_precision(self, precision="fp32"):
        """Arithmetic of the training step (pg_set_train_precision): "fp32" (the reference's, default) or "bf16" (bf16 tape
        and GEMM operands); independent of the rendering precision."""
        p = PREC_BY_NAME[precision] if isinstance(precision, str) else int(precision)
        self._check(self.lib.pg_set_train_precision(self.handle, p))

    def profile_enable(self, on=True):
        self._check(self.lib.pg_profile_enable(self.handle, 1 if on else 0))

    def profile_read(self):
        """(launches, summed device ms, points) of the fused embed+MLP kernel since the last read."""
        n, ms, pts = C.c_int64(), C.c_double(), C.c_int64()
        self._check(self.lib.pg_profile_read(self.handle, C.byref(n), C.byref(ms), C.byref(pts)))
        return n.value, ms.value, pts.value

    def profile_read_aux(self):
        """(launches, summed device ms) of the per-ray record kernel in front of the factorised 16-bit launches."""
        n, ms = C.c_int64(), C.c_double()
        self._check(self.lib.pg_profile_read_aux(self.handle, C.byref(n), C.byref(ms)))
        return n.value, ms.value

    def device_info(self):
        n, k = C.c_int32(), C.c_int32()
        self._check(self.lib.pg_device_info(self.handle, C.byref(n), C.byref(k)))
        return {"n_cu": n.value, "clock_khz": k.value}

    def calibrate_mfma(self, f16=False, lds_fed=False, min_ms=20.0):
        """TFLOP/s this device sustains on bare 32x32x16 MFMAs, operands in registers or (lds_fed) the A
        operand read from LDS per MFMA (pg_calibrate_mfma); synchronous."""
        tf, ms = C.c_double(), C.c_double()
        self._check(self.lib.pg_calibrate_mfma(self.handle, 1 if f16 else 0, int(lds_fed), float(min_ms),
                                               C.byref(tf), C.byref(ms)))
        return {"tflops": tf.value, "ms": ms.value}

    def query(self, precision=None):
        sb, mf = C.c_int64(), C.c_int64()
        self._check(self.lib.pg_query(self.handle, self.precision if precision is None else int(precision),
                                      C.byref(sb), C.byref(mf)))
        return {"stream_bytes": sb.value, "mfma_per_group": mf.value}

    # -- the hot path -----------------------------------------------------------------
    def _pose_args(self, skts: torch.Tensor, n: int):
        """[1|n,24,4,4] -> (contiguous device tensor, stride in floats)."""
        return _per_ray(skts, n, self.device, 4, 24 * 16, "skts has {} poses")

    def _cyl_args(self, cyls: torch.Tensor, n: int):
        return _per_ray(cyls, n, self.device, 2, 5, "cyls has {} rows")

    def render_rays(self, ray_batch: torch.Tensor, skts: torch.Tensor, cyls: torch.Tensor,
                    cams: Optional[torch.Tensor] = None, n_samples: Optional[int] = None,
                    n_importance: Optional[int] = None, lindisp: bool = False,
                    want_alpha: bool = True, extras: bool = False,
                    draws: Optional[Dict[str, torch.Tensor]] = None) -> Dict[str, torch.Tensor]:
        """One `RayCaster.render_rays` call (core/raycasters.py:361-474).  `draws` = None: eval mode.
        Otherwise the random numbers of a training-mode call (pg_train_draws, posegen_hip.h): any of
        t_rand [n,S], u_rand [n,N], noise0 [n,S], noise1 [n,S+N], ray_noise [n,S+N,3]."""
        c = marshal_ray_call(self.cfg, self.device, ray_batch, skts, cyls, cams, n_samples, n_importance, lindisp, draws)
        out, ex, po = alloc_ray_outputs(c.n, c.S, c.N, self.device, want_alpha, extras)
        args = (c.n, c.rb, c.sk, c.ps, c.cy, c.cs, c.cam, c.S, c.N, c.flags)
        if c.n > 0 and c.draws is not None:
            _ffi.call(self, "pg_render_rays_train", *args, C.byref(c.draws), C.byref(po))
        elif c.n > 0:
            _ffi.call(self, "pg_render_rays", *args, C.byref(po))
        if extras:
            out["extras"] = ex
        return out

    def render_frame(self, H: int, W: int, focal, c2w, box, skts: torch.Tensor, cyl: torch.Tensor,
                     center=None, cam: Optional[float] = None, near: float = 0., far: float = 1.,
                     n_samples: Optional[int] = None, n_importance: Optional[int] = None, lindisp: bool = False,
                     bg: Optional[torch.Tensor] = None, base_bg: float = 0., want_uint8: bool = False):
        """One frame entirely on the device (pg_render_frame): rays of the pixels in `box` =
        ((tl_x, tl_y), (br_x, br_y)), render, scatter over the background.  Returns device
        tensors rgb [H,W,3], disp [H,W,1], acc [H,W,1] (+ rgb8 uint8 [H,W,3])."""
        S, N = _resolve_sn(self.cfg, n_samples, n_importance)
        c2w_h, intr, bx = self._frame_args(H, W, focal, c2w, box, center)
        sk, _ = self._pose_args(skts, 1)
        cy_t, _ = self._cyl_args(cyl, 1)
        rgb, disp, acc, rgb8, bgt = self._frame_outputs(H, W, bg, want_uint8)
        _ffi.call(self, "pg_render_frame", int(H), int(W), c2w_h.ctypes.data_as(C.POINTER(C.c_float)), intr, bx, float(near), float(far),
                  sk, cy_t, -1.0 if cam is None else float(cam), S, N, _ffi.PG_FLAG_LINDISP if lindisp else 0, bgt, float(base_bg), rgb,
                  disp, acc, rgb8)
        return (rgb, disp, acc, rgb8) if want_uint8 else (rgb, disp, acc)

    def _frame_args(self, H, W, focal, c2w, box, center):
        """-> (camera [3,4] float32 on the host, (fx, fy, cx, cy), (tl_x, tl_y, br_x, br_y)) as the ABI takes them"""
        c2w_h = np.ascontiguousarray(np.asarray(c2w.detach().cpu() if isinstance(c2w, torch.Tensor) else c2w,
                                                dtype=np.float32)[:3, :4])
        (tlx, tly), (brx, bry) = box
        return (c2w_h, (C.c_float * 4)(*_intrinsics(H, W, focal, center)), (C.c_int * 4)(int(tlx), int(tly), int(brx), int(bry)))

    def _frame_outputs(self, H, W, bg, want_uint8):
        """The tensors of one composed frame -> (rgb [H,W,3], disp [H,W,1], acc [H,W,1], rgb8 uint8 [H,W,3] or None,
        background [H*W,3] on the device or None)."""
        dev = self.device
        rgb = torch.empty(H, W, 3, device=dev)
        disp = torch.empty(H, W, 1, device=dev)
        acc = torch.empty(H, W, 1, device=dev)
        rgb8 = torch.empty(H, W, 3, device=dev, dtype=torch.uint8) if want_uint8 else None
        return rgb, disp, acc, rgb8, None if bg is None else _dev_f32(bg.reshape(H * W, 3), dev)

    def render_frame_range(self, H: int, W: int, focal, c2w, box, skts: torch.Tensor, cyl: torch.Tensor,
                           ray_begin: int, ray_end: int, center=None, cam: Optional[float] = None, near: float = 0.,
                           far: float = 1., n_samples: Optional[int] = None, n_importance: Optional[int] = None,
                           lindisp: bool = False, out: Optional[torch.Tensor] = None) -> torch.Tensor:
        """Rays [ray_begin, ray_end) of the box's row-major ray list -> their maps, packed as one device tensor
        [5, n]: rows 0-2 hold rgb_map [n,3] (flat), row 3 disp_map, row 4 acc_map (pg_render_frame_range; the
        unit of work of the multi-process partition, dist.plan_tasks).  `ray_begin` must be 0 or a multiple
        of the nanmean group size, so the values are those of the whole frame."""
        S, N = _resolve_sn(self.cfg, n_samples, n_importance)
        n = int(ray_end) - int(ray_begin)
        buf = torch.empty(5 * n, device=self.device) if out is None else out
        if buf.numel() != 5 * n or buf.dtype != torch.float32 or not buf.is_contiguous():
            raise ValueError("render_frame_range: `out` must be a contiguous float32 tensor of 5 * n elements")
        if n > 0:
            c2w_h, intr, bx = self._frame_args(H, W, focal, c2w, box, center)
            sk, _ = self._pose_args(skts, 1)
            cy_t, _ = self._cyl_args(cyl, 1)
            flat = buf.view(-1)
            _ffi.call(self, "pg_render_frame_range", int(H), int(W), c2w_h.ctypes.data_as(C.POINTER(C.c_float)), intr, bx, float(near),
                      float(far), sk, cy_t, -1.0 if cam is None else float(cam), S, N, _ffi.PG_FLAG_LINDISP if lindisp else 0,
                      int(ray_begin), int(ray_end), flat[:3 * n], flat[3 * n:4 * n], flat[4 * n:])
        return buf

    def compose_frame(self, H: int, W: int, box, rgb_map: torch.Tensor, disp_map: torch.Tensor, acc_map: torch.Tensor,
                      bg: Optional[torch.Tensor] = None, base_bg: float = 0., want_uint8: bool = False):
        """The maps of a whole box over the background (pg_compose_frame): device tensors rgb [H,W,3],
        disp [H,W,1], acc [H,W,1] (+ rgb8).  The maps of a box without pixels may be None."""
        dev = self.device
        (tlx, tly), (brx, bry) = box
        rgb, disp, acc, rgb8, bgt = self._frame_outputs(H, W, bg, want_uint8)
        rm, dm, am = (None if m is None else _dev_f32(m, dev) for m in (rgb_map, disp_map, acc_map))
        _ffi.call(self, "pg_compose_frame", int(H), int(W), (C.c_int * 4)(int(tlx), int(tly), int(brx), int(bry)), rm, dm, am, bgt,
                  float(base_bg), rgb, disp, acc, rgb8)
        return (rgb, disp, acc, rgb8) if want_uint8 else (rgb, disp, acc)

    def render_scene(self, H: int, W: int, focal, c2w, people, **kw):
        """Several people of the bank in ONE frame with mutual occlusion (pg_render_scene): posegen_amd.scene.render_scene."""
        from .scene import render_scene
        return render_scene(self, H, W, focal, c2w, people, **kw)

    @property
    def n_devices(self) -> int:
        return len(self.devices)

    def render_frames(self, H: int, W: int, focals, c2ws, boxes, skts, cyls, centers=None, cams=None,
                      near: float = 0., far: float = 1., n_samples: Optional[int] = None,
                      n_importance: Optional[int] = None, lindisp: bool = False, bg=None, base_bg: float = 0.,
                      want_uint8: bool = False, subjects=None):
        """Frames on ALL devices of the handle (pg_render_frames), host in / host out: numpy arrays
        rgbs [F,H,W,3], disps [F,H,W,1], accs [F,H,W,1] (+ rgb8 uint8 [F,H,W,3]).  `boxes` = list of
        ((tl_x, tl_y), (br_x, br_y)); skts [F,24,4,4], cyls [F,5] (one pose per frame); `subjects`: one subject per frame
        (pg_render_frames_subjects; None: the selected subject for all)."""
        S, N = _resolve_sn(self.cfg, n_samples, n_importance)
        F = len(boxes)
        subj = frame_subjects(subjects, F, self.n_subjects, "subjects")
        sj = None if subj is None else np.ascontiguousarray(np.asarray(subj, dtype=np.int32))
        c2w_h = np.ascontiguousarray(np.stack([np.asarray(torch.as_tensor(c).detach().cpu(), dtype=np.float32)[:3, :4]
                                               for c in c2ws]))
        intr = np.zeros((F, 4), dtype=np.float32)
        for i in range(F):
            intr[i] = _intrinsics(H, W, focals[i] if np.ndim(focals) > 0 else focals, None if centers is None else centers[i])
        bx = np.ascontiguousarray(np.array([[b[0][0], b[0][1], b[1][0], b[1][1]] for b in boxes], dtype=np.int32))
        sk = _np32(skts).reshape(-1, 24, 4, 4)
        cy = _np32(cyls).reshape(-1, 5)
        if sk.shape[0] == 1 and F > 1:
            sk = np.ascontiguousarray(np.repeat(sk, F, 0))
        if cy.shape[0] == 1 and F > 1:
            cy = np.ascontiguousarray(np.repeat(cy, F, 0))
        if sk.shape[0] != F or cy.shape[0] != F:
            raise ValueError(f"need one pose per frame: {sk.shape[0]} skts / {cy.shape[0]} cyls for {F} frames")
        cm = None if cams is None else _np32(cams).reshape(-1)
        bgh = None if bg is None else _np32(bg).reshape(H * W, 3)
        # results in page-locked memory when they are small enough to pin as a whole: the library then copies every
        # frame straight into them on a copy stream while the next one renders; pageable arrays (long paths) are
        # filled through the library's own pinned staging
        pin = F * H * W * (23 if want_uint8 else 20) <= (256 << 20) and torch.cuda.is_available()
        new = lambda c, dt: torch.empty((F, H, W, c), dtype=dt, pin_memory=pin).numpy()
        rgbs, disps, accs = new(3, torch.float32), new(1, torch.float32), new(1, torch.float32)
        rgb8 = new(3, torch.uint8) if want_uint8 else None
        hp = lambda a: None if a is None else C.c_void_p(a.ctypes.data)
        args = (self.handle, F, int(H), int(W), hp(c2w_h), hp(intr), hp(bx), float(near), float(far), hp(sk), hp(cy), hp(cm),
                S, N, _ffi.PG_FLAG_LINDISP if lindisp else 0, hp(bgh), float(base_bg), hp(rgbs), hp(disps), hp(accs), hp(rgb8))
        if sj is None:
            self._check(self.lib.pg_render_frames(*args))
        else:
            self._check(self.lib.pg_render_frames_subjects(*args, hp(sj)))
        return (rgbs, disps, accs, rgb8) if want_uint8 else (rgbs, disps, accs)

    def query_density(self, pts: torch.Tensor, skts: torch.Tensor, which: Optional[int] = None) -> torch.Tensor:
        """Raw density (alpha_linear output, no activation) of net `which` (default: the fine net if
        loaded, like the reference; net 0 with single_net) at explicit points [...,3] for one pose: render_pts_density
        (core/raycasters.py:598-646).  Returns a device tensor [..., 1]."""
        if which is None:
            which = 1 if "network_fine_state_dict" in self._state and not self.cfg.single_net else 0
        p = _dev_f32(torch.as_tensor(pts).reshape(-1, 3), self.device)
        n = p.shape[0]
        sk, _ = self._pose_args(skts, 1)
        raw = torch.empty(n, 4, device=self.device)
        if n > 0:
            _ffi.call(self, "pg_query_density", int(which), n, p, sk, raw)
        return raw[:, 3:4].reshape(*torch.as_tensor(pts).shape[:-1], 1)

    def mesh_density(self, kps: torch.Tensor, skts: torch.Tensor, radius: float = 1.0, res: int = 64,
                     which: Optional[int] = None) -> torch.Tensor:
        """Raw density on the (res+1)^3 grid of half-width `radius` around the root joint, laid out
        like RayCaster.render_mesh_density (core/raycasters.py:579-596)."""
        t = np.linspace(-radius, radius, res + 1)
        grid = np.stack(np.meshgrid(t, t, t), axis=-1).astype(np.float32)
        sh = grid.shape
        pts = torch.tensor(grid.reshape(-1, 3)) + torch.as_tensor(kps, dtype=torch.float32).reshape(-1, 24, 3)[0, 0]
        d = self.query_density(pts, skts, which)
        return d.reshape(*sh[:-1]).transpose(1, 0)

    def _density_net(self, which: Optional[int]) -> int:
        """the net a density query means: the fine net if loaded, like the reference; net 0 with single_net"""
        if which is None:
            which = 1 if "network_fine_state_dict" in self._state and not self.cfg.single_net else 0
        return int(which)

    def grid_density(self, kps: torch.Tensor, skts: torch.Tensor, radius: float = 1.8, res: int = 255,
                     which: Optional[int] = None, slab_rays: int = 0) -> torch.Tensor:
        """mesh_density's grid, formed and evaluated on the device (pg_grid_density): raw density at root + (t[a], t[b], t[c]),
        t = linspace(-radius, radius, res + 1), as a device tensor [R,R,R].  A grid row runs as a ray, through the kernel forms
        of a render call; nothing but the root joint and the pose crosses the bus.  `slab_rays`: rows per launch (0: the
        library sizes the slabs); the values do not depend on it."""
        R = int(res) + 1
        root = _np32(torch.as_tensor(kps).reshape(-1, 24, 3)[0, 0])
        sk, _ = self._pose_args(torch.as_tensor(skts).detach(), 1)
        sigma = torch.empty(R, R, R, device=self.device) if res >= 1 else None
        _ffi.call(self, "pg_grid_density", self._density_net(which), int(res), float(radius), root.ctypes.data_as(C.POINTER(C.c_float)), sk,
                  int(slab_rays), sigma)
        return sigma

    def marching_cubes(self, grid: torch.Tensor, threshold: float, clamp: float = 0.0):
        """Marching cubes on a device grid [Nx,Ny,Nz] (pg_mesh_count + pg_mesh_emit): inside is max(grid, clamp) > threshold
        (clamp = 0: the reference's np.maximum(raw, 0); -inf: the grid as it is).  Returns device tensors (vertices float32
        [nv,3] in index coordinates, triangles int32 [nt,3]); shared vertices, normals away from the inside."""
        g = _dev_f32(torch.as_tensor(grid), self.device)
        if g.dim() != 3:
            raise ValueError(f"marching_cubes: a 3-D grid expected, got {tuple(g.shape)}")
        nv, nt = C.c_int64(), C.c_int64()
        args = (g, *(int(n) for n in g.shape), float(threshold), float(clamp))
        _ffi.call(self, "pg_mesh_count", *args, C.byref(nv), C.byref(nt))
        verts = torch.empty(nv.value, 3, device=self.device)
        tris = torch.empty(nt.value, 3, device=self.device, dtype=torch.int32)
        _ffi.call(self, "pg_mesh_emit", *args, verts if nv.value else None, tris if nt.value else None, nv.value, nt.value)
        return verts, tris

    def pose_kinematics(self, bones: torch.Tensor, rest_pose, parents=None, want_l2ws: bool = False):
        """bones [F,24,3] axis-angle (any device/dtype) -> device kps [F,24,3] f32, skts [F,24,4,4] f32
        (+ l2ws f64), computed on the device in float64 (pg_pose_kinematics; the host equivalent is
        skeleton.bones_to_pose)."""
        from .skeleton import SMPLSkeleton
        b = torch.as_tensor(bones).to(device=self.device, dtype=torch.float64).contiguous()
        F = b.shape[0]
        par = np.ascontiguousarray(np.asarray(SMPLSkeleton.joint_trees if parents is None else parents, dtype=np.int32))
        rp = np.asarray(rest_pose).reshape(24, 3)             # offsets in the rest pose's own dtype, like
        offs = rp.copy()                                      # get_smpl_l2ws (float32 for smpl_rest_pose)
        offs[1:] = rp[1:] - rp[par[1:]]
        rest = np.ascontiguousarray(offs.astype(np.float64))
        kps = torch.empty(F, 24, 3, device=self.device)
        skts = torch.empty(F, 24, 4, 4, device=self.device)
        l2ws = torch.empty(F, 24, 4, 4, device=self.device, dtype=torch.float64) if want_l2ws else None
        _ffi.call(self, "pg_pose_kinematics", F, b, rest.ctypes.data_as(C.POINTER(C.c_double)), par.ctypes.data_as(C.POINTER(C.c_int32)),
                  kps, skts, l2ws)
        return (kps, skts, l2ws) if want_l2ws else (kps, skts)

    def pose_kinematics_rot(self, rotmats: torch.Tensor, rest_pose, scale: float = 1.0, parents=None, want_l2ws: bool = False):
        """`pose_kinematics` with the rotations given: rotmats [F,24,3,3] (any device/dtype; float32 on the device) -> device kps
        [F,24,3] f32, skts [F,24,4,4] f32 (+ l2ws f64), get_smpl_l2ws_torch(pose, rest_pose, scale, axis_to_matrix=False)
        (core/utils/skeleton_utils.py:379-463; pg_pose_kinematics_rot).  `scale` multiplies the rest pose in its own dtype, as
        the reference's `rest_pose * scale` does."""
        from .skeleton import SMPLSkeleton
        shape = tuple(np.shape(rotmats))
        if len(shape) != 4 or shape[1:] != (24, 3, 3):
            raise ValueError(f"pose_kinematics_rot: rotmats {shape}; [F,24,3,3] expected")
        par = np.asarray(SMPLSkeleton.joint_trees if parents is None else parents)
        if par.dtype.kind not in "iu" or par.shape != (24,):
            raise ValueError("pose_kinematics_rot: parents must be 24 integers")
        par = np.ascontiguousarray(par.astype(np.int32))
        par[0] = -1
        if any(not 0 <= par[j] < j for j in range(1, 24)):
            raise ValueError("pose_kinematics_rot: every joint must come after its parent")
        rp = np.asarray(rest_pose).reshape(24, 3)
        rp = rp * np.asarray(scale, dtype=rp.dtype)
        offs = rp.copy()
        offs[1:] = rp[1:] - rp[par[1:]]
        rest = np.ascontiguousarray(offs.astype(np.float64))
        m = _dev_f32(torch.as_tensor(rotmats), self.device)
        F = m.shape[0]
        kps = torch.empty(F, 24, 3, device=self.device)
        skts = torch.empty(F, 24, 4, 4, device=self.device)
        l2ws = torch.empty(F, 24, 4, 4, device=self.device, dtype=torch.float64) if want_l2ws else None
        _ffi.call(self, "pg_pose_kinematics_rot", F, m, rest.ctypes.data_as(C.POINTER(C.c_double)),
                  par.ctypes.data_as(C.POINTER(C.c_int32)), kps, skts, l2ws)
        return (kps, skts, l2ws) if want_l2ws else (kps, skts)

    def pose_boxes(self, kps: torch.Tensor, c2ws, H: int, W: int, focal, ext_scale: float, center=None,
                   extend_mm: float = 250., top_expand_ratio: float = 1.60, bot_expand_ratio: float = 1.10):
        """Device bounding cylinders [F,5] f32 and integer boxes [F,4] i32 (tl_x, tl_y, br_x, br_y) of device
        key points [F,24,3] (pg_pose_boxes: kp_to_valid_rays' cull without the host round trip).  `c2ws`:
        one camera [4,4] or one per pose [F,4,4] (host); the extrinsic is inverted on the host in float32
        exactly as the reference does (nerf_c2w_to_extrinsic)."""
        from .skeleton import nerf_c2w_to_extrinsic
        kp = _dev_f32(kps.reshape(-1, 24, 3), self.device)
        F = kp.shape[0]
        c2w = np.asarray(torch.as_tensor(c2ws).detach().cpu(), dtype=np.float32).reshape(-1, 4, 4)
        w2c = np.stack([nerf_c2w_to_extrinsic(c) for c in c2w]).astype(np.float64)      # float32 inverse, widened
        if w2c.shape[0] not in (1, F):
            raise ValueError(f"{w2c.shape[0]} cameras for {F} poses")
        phi = np.linspace(0., 2 * np.pi, 50)
        ring = np.ascontiguousarray(np.stack([np.cos(phi), np.sin(phi)], -1))
        fx, fy, cx, cy = _intrinsics(H, W, focal, center, f32_focal=True)
        offx, offy = int(cx), int(cy)                   # (the reference's integer principal point)
        ext = extend_mm * ext_scale
        d_w2c = torch.tensor(w2c, dtype=torch.float64, device=self.device)
        d_ring = torch.tensor(ring, dtype=torch.float64, device=self.device)
        cyls = torch.empty(F, 5, device=self.device)
        boxes = torch.empty(F, 4, device=self.device, dtype=torch.int32)
        _ffi.call(self, "pg_pose_boxes", F, kp, d_w2c, 16 if w2c.shape[0] > 1 else 0, d_ring, float(ext), float(ext * top_expand_ratio),
                  float(ext * bot_expand_ratio), fx, fy, int(H), int(W), offx, offy, cyls, boxes)
        return cyls, boxes

    # -- stage entry points (tests / profiling) ---------------------------------------
    def stage_frame_rays(self, H, W, focal, c2w, box, r0, r1, center=None, cam=None, near=0., far=1., want_cams=False):
        """Rays [r0, r1) of the box's row-major ray list as the frame front end writes them (pg_stage_frame_rays) ->
        ray_batch rows [r1 - r0, 11] (+ their frame codes [r1 - r0] with want_cams); nothing is rendered."""
        n = max(int(r1) - int(r0), 0)
        rays = torch.empty(max(n, 1), 11, device=self.device)              # (an empty range still hands a buffer over)
        cams = torch.empty(max(n, 1), device=self.device) if want_cams else None
        c2w_h, intr, bx = self._frame_args(H, W, focal, c2w, box, center)
        _ffi.call(self, "pg_stage_frame_rays", int(H), int(W), c2w_h.ctypes.data_as(C.POINTER(C.c_float)), intr, bx, float(near),
                  float(far), -1.0 if cam is None else float(cam), int(r0), int(r1), rays, cams)
        return (rays[:n], cams[:n]) if want_cams else rays[:n]

    def stage_sample_coarse(self, ray_batch, cyls, n_samples, lindisp=False):
        rb = _dev_f32(ray_batch, self.device)
        n = rb.shape[0]
        cy, cs = self._cyl_args(cyls, n)
        nf = torch.empty(n, 2, device=self.device)
        z = torch.empty(n, n_samples, device=self.device)
        _ffi.call(self, "pg_stage_sample_coarse", n, rb, cy, cs, int(n_samples), _ffi.PG_FLAG_LINDISP if lindisp else 0, nf, z)
        return nf, z

    def stage_eval(self, which, ray_batch, z, skts, cams=None, want_dbg=False, dbg_stage=0, dbg=None):
        """Net `which` at the depths z [n,S] (pg_stage_eval) -> raw [n,S,4] (+ the activations of `dbg_stage` with want_dbg).
        `dbg`: the caller's own buffer for a dbg_stage that writes something else (97: counters)."""
        zz = _dev_f32(z, self.device)
        n, S = zz.shape
        c = marshal_ray_call(self.cfg, self.device, ray_batch, skts, None, cams, n_samples=S, n_importance=0)
        raw = torch.empty(n, S, 4, device=self.device)
        if want_dbg:
            dbg = torch.zeros(n * S, 256, device=self.device)
        _ffi.call(self, "pg_stage_eval", int(which), n, S, c.rb, zz, c.sk, c.ps, c.cam, raw, dbg, int(dbg_stage))
        return (raw, dbg) if want_dbg else raw

    def limb_skip_stats(self, which, ray_batch, z, skts, cams=None):
        """Measurement aid (pg_stage_eval, dbg_stage 97): what the limb masks of the fused kernel leave out on this launch --
        the kernel itself counts.  Returns the fraction of (pass, limb) pairs left out of whole passes and the fraction of
        (wave or column tile, limb) pairs left out at the finer level (which includes the former)."""
        cnt = torch.zeros(64, device=self.device, dtype=torch.int32)
        self.stage_eval(which, ray_batch, z, skts, cams, dbg_stage=97, dbg=cnt)
        return _wave_stats([int(v) for v in cnt[:5].cpu()])

    def stage_composite(self, ray_batch, z, raw, n_importance=0):
        rb = _dev_f32(ray_batch, self.device)
        zz = _dev_f32(z, self.device)
        rw = _dev_f32(raw, self.device)
        n, S = zz.shape
        new = lambda *s: torch.empty(*s, device=self.device, dtype=torch.float32)
        o = {"rgb_map": new(n, 3), "disp_map": new(n), "acc_map": new(n), "alpha": new(n, S),
             "weights": new(n, S)}
        zf = new(n, S + n_importance) if n_importance > 0 else None
        _ffi.call(self, "pg_stage_composite", n, S, rb, zz, rw, o["rgb_map"], o["disp_map"], o["acc_map"], o["alpha"], o["weights"],
                  int(n_importance), zf)
        if zf is not None:
            o["z_fine"] = zf
        return o

    def stage_sample_coarse_draws(self, ray_batch, cyls, n_samples, lindisp=False, t_rand=None, one_launch=False):
        """stage_sample_coarse with the stratified draws t_rand [n,S] (pg_stage_sample_coarse_draws); `one_launch`: the one-launch
        form of the kernel also for chunks of more than 256 rays."""
        rb = _dev_f32(ray_batch, self.device)
        n = rb.shape[0]
        cy, cs = self._cyl_args(cyls, n)
        tr = None if t_rand is None else _dev_f32(t_rand, self.device)
        nf = torch.empty(n, 2, device=self.device)
        z = torch.empty(n, n_samples, device=self.device)
        _ffi.call(self, "pg_stage_sample_coarse_draws", n, rb, cy, cs, int(n_samples),
                  (_ffi.PG_FLAG_LINDISP if lindisp else 0) | (_ffi.PG_FLAG_STAGE_ONE_LAUNCH if one_launch else 0), tr, nf, z)
        return nf, z

    def stage_composite_form(self, form, ray_batch, z, raw, n_importance=0, noise=None, u_rand=None, ld_new=None, fill=None):
        """One composite launch in the named form, "plain" or "is_only" (pg_stage_composite_form): the maps, alpha, weights and, with
        n_importance > 0, z_fine, order and (is_only) z_new [n,ld_new].  `fill`: the outputs start as this value, not uninitialised."""
        rb, zz, rw = (_dev_f32(t, self.device) for t in (ray_batch, z, raw))
        n, S = zz.shape
        N = int(n_importance)
        nz = None if noise is None else _dev_f32(noise, self.device)
        ur = None if u_rand is None else _dev_f32(u_rand, self.device)
        new = lambda *s, dtype=torch.float32: (torch.empty(*s, device=self.device, dtype=dtype) if fill is None
                                               else torch.full(s, fill, device=self.device, dtype=dtype))
        o = {"rgb_map": new(n, 3), "disp_map": new(n), "acc_map": new(n), "alpha": new(n, S), "weights": new(n, S)}
        iso = {"plain": False, "is_only": True}[form]
        ld = N if ld_new is None else int(ld_new)
        if N > 0:
            o["z_fine"], o["order"] = new(n, S + N), new(n, S + N, dtype=torch.int32)
            if iso:
                o["z_new"] = new(n, ld)
        _ffi.call(self, "pg_stage_composite_form", _ffi.PG_COMP_IS_ONLY if iso else _ffi.PG_COMP_PLAIN, n, S, N, rb, zz, rw, nz, ur,
                  o["rgb_map"], o["disp_map"], o["acc_map"], o["alpha"], o["weights"], o.get("z_fine"), o.get("order"), o.get("z_new"), ld,
                  None, None)
        return o

    def stage_composite_merged(self, ray_batch, z_fine, raw, raw_new, order, noise=None, fill=None):
        """The fine pass of the single-net pair (pg_stage_composite_form, merged): z_fine [n,S+N], coarse raw [n,S,4], raw_new
        [n,ld_new,4], order [n,S+N] int32 -> the maps, alpha and raw_out [n,S+N,4]."""
        rb, zf, rw, rn = (_dev_f32(t, self.device) for t in (ray_batch, z_fine, raw, raw_new))
        od = order.to(device=self.device, dtype=torch.int32).contiguous()
        n, S, ld = rw.shape[0], rw.shape[1], rn.shape[1]
        N = zf.shape[1] - S
        nz = None if noise is None else _dev_f32(noise, self.device)
        new = lambda *s: (torch.empty(*s, device=self.device) if fill is None else torch.full(s, fill, device=self.device))
        o = {"rgb_map": new(n, 3), "disp_map": new(n), "acc_map": new(n), "alpha": new(n, S + N), "raw_out": new(n, S + N, 4)}
        _ffi.call(self, "pg_stage_composite_form", _ffi.PG_COMP_MERGED, n, S, N, rb, zf, rw, nz, None, o["rgb_map"], o["disp_map"],
                  o["acc_map"], o["alpha"], None, None, od, None, ld, rn, o["raw_out"])
        return o

    def stage_composite_bwd(self, ray_batch, z, raw, noise=None, d_rgb=None, d_acc=None):
        """d_raw [n,S,4] of one composite from the cotangents of its rgb and acc maps (pg_stage_composite_bwd)."""
        opt = lambda t: None if t is None else _dev_f32(t, self.device)
        rb, zz, rw = (_dev_f32(t, self.device) for t in (ray_batch, z, raw))
        nz, gr, ga = opt(noise), opt(d_rgb), opt(d_acc)
        n, S = zz.shape
        d_raw = torch.empty(n, S, 4, device=self.device)
        _ffi.call(self, "pg_stage_composite_bwd", n, S, rb, zz, rw, nz, gr, ga, d_raw)
        return d_raw

    def stage_merged_composite_bwd(self, ray_batch, z, z_fine, raw, order, noise0=None, noise1=None, d_rgb=None, d_acc=None,
                                   d_rgb0=None, d_acc0=None):
        """d_raw [n S + n N, 4] of the single-net pair (pg_stage_merged_composite_bwd): raw holds the coarse rows [n S, 4], then the
        new points' [n N, 4]."""
        opt = lambda t: None if t is None else _dev_f32(t, self.device)
        rb, zz, zf, rw = (_dev_f32(t, self.device) for t in (ray_batch, z, z_fine, raw))
        od = order.to(device=self.device, dtype=torch.int32).contiguous()
        n, S = zz.shape
        N = zf.shape[1] - S
        keep = [opt(t) for t in (noise0, noise1, d_rgb, d_acc, d_rgb0, d_acc0)]
        d_raw = torch.empty(n * (S + N), 4, device=self.device)
        _ffi.call(self, "pg_stage_merged_composite_bwd", n, S, N, rb, zz, zf, rw, keep[0], keep[1], od, *keep[2:], d_raw)
        return d_raw


def _wave_stats(c):
    """the counters of pg_stage_eval's dbg_stage 97 as fractions; the empty-wave counts come from pg_eval16r.hip only"""
    passes, per_pass, fine, empty, skipped = c[:5]
    per_fine = 48                                   # 8 waves / column tiles x 6 limbs per pass in both kernels
    return {"passes": passes, "limbs_left_out_of_whole_passes_frac": per_pass / max(6 * passes, 1),
            "limbs_left_out_frac": fine / max(per_fine * passes, 1),
            "empty_waves_frac": empty / max(8 * passes, 1), "skipped_waves_frac": skipped / max(8 * passes, 1)}


def check_single_net_states(coarse, fine):
    """A single-net caster has one net, which the reference saves under both keys (raycasters.py:751-766): a fine state
    dict, where there is one, must hold the coarse one's keys and bitwise its values.  Anything else is not the reference's
    checkpoint, and nobody guesses which of the two to render."""
    if coarse is None or fine is None:
        return
    if set(coarse) != set(fine) or not all(np.array_equal(_np32(coarse[k]), _np32(fine[k])) for k in coarse):
        raise ValueError("single_net: network_fine_state_dict differs from network_fn_state_dict "
                         "(a single-net caster has one net; not guessing which one to render)")


def refuse_reference_kwargs(who, check_preproc, skts, cyls, kw, own_fine=None):
    """Refuse, don't render differently: a caller configured for anything the fused kernels do not compute.  `kw`: the
    reference's keywords beyond the ones the casters act on, as `who`.forward got them; `own_fine`: the one `network_fine`
    argument that is no request for another net (TrainableRayCaster's own).  retraw / verbose / ext_scale change nothing
    the reference returns for these calls and are ignored."""
    kw = dict(kw)
    fwd_type = kw.pop("fwd_type", "")
    if fwd_type:
        raise NotImplementedError(f"fwd_type={fwd_type!r} is not on the HIP path of forward (HipRayCaster's call dispatches "
                                  "'density' and 'mesh')")
    if kw.pop("subject_idxs", None) is not None:       # (HipRayCaster resolves its own before it comes here: call_subject)
        raise NotImplementedError(f"{who}: subject_idxs in training mode is not built (training a subject bank is out of scope; "
                                  "eval-mode calls render the subject through the HipRayCaster)")
    if skts is None or cyls is None:
        raise ValueError("skts and cyls are required (A-NeRF bone-relative rendering)")
    nerf_type = kw.pop("nerf_type", "nerf")
    if nerf_type != "nerf":
        raise NotImplementedError(f"nerf_type={nerf_type!r}: only 'nerf' is on the HIP path")
    if not kw.pop("use_viewdirs", True):
        raise NotImplementedError("use_viewdirs=False: the HIP kernels always evaluate the view branch (nerf.py:112-121)")
    fine = kw.pop("network_fine", None)
    if fine is not None and fine is not own_fine:
        raise NotImplementedError("network_fine: the caster renders with the nets it was loaded with (load_state_dict)")
    check_preproc(kw.pop("preproc_kwargs", None))
    for k in ("retraw", "verbose", "ext_scale"):
        kw.pop(k, None)
    if kw:
        raise TypeError(f"{who}.forward: unexpected keyword arguments {sorted(kw)}")


class HipRayCaster:
    """Call-compatible stand-in for `RayCaster` / `nn.DataParallel(RayCaster)`.

    Reference call site: ``ray_caster(rays_flat[i:i+chunk].to('cuda'), **batch_kwargs)``
    (core/trainer.py:74) with the kwargs of `render_kwargs_test`
    (core/raycasters.py:156-178) plus the per-ray pose tensors.
    """

    def __init__(self, cfg: RenderConfig, device="cuda:0", precision=PREC_BF16, devices=None):
        """`devices=[0, 1, ...]`: all GPUs of this process behind one caster, the replacement of
        `nn.DataParallel(RayCaster)` (core/raycasters.py:157): `render_path` then spreads the frames
        (or, with fewer frames than GPUs, the frames' ray chunks) over them inside one call."""
        self.cfg = cfg
        self.renderer = HipRenderer(cfg, device, precision, devices=devices)
        self.training = False

    # ---- construction helpers -------------------------------------------------------
    @classmethod
    def from_weights(cls, cfg, w_coarse, w_fine, tau_v, tau_d, device="cuda:0", precision=PREC_BF16, devices=None):
        """`w_fine` may be None (coarse-only renders, or single_net: network_fine is network)."""
        if cfg.single_net:
            check_single_net_states(w_coarse, w_fine)
        rc = cls(cfg, device, precision, devices=devices)
        rc.renderer.load_network(0, w_coarse)
        if w_fine is not None and not cfg.single_net:
            rc.renderer.load_network(1, w_fine)
        rc.renderer.set_embedder(0, tau_v)
        rc.renderer.set_embedder(1, tau_d)
        return rc

    @classmethod
    def from_subjects(cls, cfg, models, device="cuda:0", precision=PREC_BF16, devices=None):
        """A bank of len(models) subjects of one architecture: `models` = [(w_coarse, w_fine, tau_v, tau_d), ...], each as
        from_weights takes them.  Subject 0 is selected."""
        models = list(models)
        if not models:
            raise ValueError("from_subjects: at least one (w_coarse, w_fine, tau_v, tau_d)")
        if cfg.single_net:
            for wc, wf, _, _ in models:
                check_single_net_states(wc, wf)
        rc = cls(cfg, device, precision, devices=devices)
        r = rc.renderer
        r.set_subject_count(len(models))
        for s, (wc, wf, tau_v, tau_d) in enumerate(models):
            with r.subject(s):
                r.load_network(0, wc)
                if wf is not None and not cfg.single_net:
                    r.load_network(1, wf)
                r.set_embedder(0, tau_v)
                r.set_embedder(1, tau_d)
        return rc

    # ---- the subject bank -------------------------------------------------------------
    @property
    def n_subjects(self) -> int:
        return self.renderer.n_subjects

    def set_subject_count(self, n: int):
        self.renderer.set_subject_count(n)

    def select_subject(self, s: int):
        self.renderer.select_subject(s)

    def subject(self, s):
        """context manager: subject s selected inside, the previous selection restored afterwards"""
        return self.renderer.subject(s)

    def load_subject(self, s: int, ckpt, strict=True):
        """load_state_dict (the reference's checkpoint layout) applied to subject s; the selection is left as it was"""
        with self.renderer.subject(int(s)):
            self.load_state_dict(ckpt, strict=strict)

    def _call_subject(self, subject_idxs) -> Optional[int]:
        return call_subject(subject_idxs, self.renderer.n_subjects)

    # ---- density queries (core/raycasters.py:579-646) ----------------------------------------
    def render_pts_density(self, pts, kps, skts, bones=None, render_kwargs=None, subject_idxs=None,
                           netchunk=1024 * 64, network=None, color=False, v=None):
        """Raw density [..., 1] at points `pts` [n,1,3] (or [n,3]) for one pose; fine net unless
        `network` is 0/1.  `kps`, `bones`, `netchunk` are accepted for call compatibility."""
        if color or v is not None:
            raise NotImplementedError("render_pts_density: color / precomputed v are not supported")
        which = network if network in (0, 1) else None
        with self.renderer.subject(self._call_subject(subject_idxs)):
            return self.renderer.query_density(torch.as_tensor(pts), skts, which)

    def render_mesh_density(self, kps, skts, bones=None, subject_idxs=None, radius=1.0, res=64,
                            render_kwargs=None, netchunk=1024 * 64, v=None):
        """Raw density on the (res+1)^3 grid around the root joint, as the reference lays it out."""
        if v is not None:
            raise NotImplementedError("render_mesh_density: precomputed v is not supported")
        with self.renderer.subject(self._call_subject(subject_idxs)):
            return self.renderer.mesh_density(kps, skts, radius=radius, res=res)

    def extract_mesh(self, kps, skts, bones=None, subject_idxs=None, radius=1.8, res=255, threshold=10., which=None):
        """The mesh of one pose as the reference's render_mesh builds it (run_render.py:976-991), on the device: density grid,
        relu, marching cubes at `threshold`.  Returns device tensors (vertices / res - .5 float32 [nv,3], triangles int32
        [nt,3]).  `bones` is accepted for call compatibility."""
        with self.renderer.subject(self._call_subject(subject_idxs)):
            grid = self.renderer.grid_density(kps, skts, radius=radius, res=res, which=which)
            verts, tris = self.renderer.marching_cubes(grid, threshold, clamp=0.0)
        return verts / res - .5, tris

    # ---- nn.Module-like surface the reference touches -------------------------------
    @property
    def module(self):            # trainer.py:267,272,506 reach through DataParallel
        return self

    def to(self, *a, **k):       # trainer.py:73 `ray_caster.to('cuda')`
        return self

    def eval(self):
        self.training = False
        return self

    def train(self, mode: bool = True):
        self.training = bool(mode)
        return self

    def parameters(self):
        self.renderer._refresh_state()
        seen = set()
        for sd in self.renderer._state.values():
            for v in sd.values():
                if id(v) not in seen:       # (single_net: both net keys hold the same tensors)
                    seen.add(id(v))
                    yield v

    def state_dict(self):
        self.renderer._refresh_state()
        sd = {k: dict(v) for k, v in self.renderer._state.items()}
        sd.setdefault("embedbones_state_dict", {})
        return sd

    def load_state_dict(self, ckpt, strict=True):
        r = self.renderer
        fine = ckpt.get("network_fine_state_dict")
        if self.cfg.single_net:
            check_single_net_states(ckpt.get("network_fn_state_dict"), fine)
        if "network_fn_state_dict" in ckpt:
            r.load_network(0, ckpt["network_fn_state_dict"])
        elif strict:
            raise KeyError("network_fn_state_dict")
        if fine is not None and not self.cfg.single_net:
            r.load_network(1, fine)
        for which, key in ((0, "embed_state_dict"), (1, "embeddirs_state_dict")):
            e = ckpt.get(key)
            if e is not None and "tau" in e:
                r.set_embedder(which, float(e["tau"]), e.get("cutoff_dist"))
            elif strict:
                raise KeyError(key)

    # ---- the call -------------------------------------------------------------------
    def __call__(self, *args, fwd_type="", **kwargs):
        # the reference dispatches on fwd_type before anything else (core/raycasters.py:349-359)
        if fwd_type == "density":
            return self.render_pts_density(*args, **kwargs)
        if fwd_type == "mesh":
            return self.render_mesh_density(*args, **kwargs)
        return self.forward(*args, fwd_type=fwd_type, **kwargs)

    def forward(self, ray_batch, N_samples=None, kp_batch=None, skts=None, cyls=None, bones=None,
                cams=None, subject_idxs=None, retraw=False, lindisp=False, perturb=0., N_importance=0,
                network_fine=None, raw_noise_std=0., ray_noise_std=0., verbose=False, ext_scale=0.001,
                pytest=False, preproc_kwargs=None, nerf_type="nerf", fwd_type="", use_viewdirs=True,
                want_alpha=True, extras=False, draws=None, **unused):
        """`RayCaster.forward` (core/raycasters.py:349-474), forward values only (no autograd graph: the training
        step is train.TrainableRayCaster).  perturb / raw_noise_std /
        ray_noise_std behave as in render_kwargs_train (raycasters.py:156-165): the random numbers
        come from torch's generator on the caster's device, from numpy after np.random.seed(0) when
        pytest=True (the reference's deterministic test mode; it has no override for the position
        noise, which stays a torch draw), or from `draws` when the caller supplies them."""
        refuse_reference_kwargs("HipRayCaster", self._check_preproc_kwargs, skts, cyls,
                                dict(unused, fwd_type=fwd_type, nerf_type=nerf_type,
                                     use_viewdirs=use_viewdirs, network_fine=network_fine, preproc_kwargs=preproc_kwargs))
        # one subject per ray call (an int, or the reference's per-ray expansion of it); checked before anything is launched
        with self.renderer.subject(self._call_subject(subject_idxs)), one_nanmean_group(self.renderer, ray_batch.shape[0], grouped=getattr(self, "_grouped_call", False)):
            if draws is None and (perturb or raw_noise_std or ray_noise_std):
                S, _ = _resolve_sn(self.cfg, N_samples, None)
                draws = self.training_draws(int(ray_batch.shape[0]), S, int(N_importance or 0), perturb, raw_noise_std,
                                            ray_noise_std, pytest=pytest)
            return self.renderer.render_rays(ray_batch, skts, cyls, cams=cams, n_samples=N_samples,
                                             n_importance=N_importance, lindisp=bool(lindisp),
                                             want_alpha=want_alpha, extras=extras, draws=draws)

    # the reference's preproc_kwargs (core/raycasters.py:140-152): the encoder objects and the density function
    # `create_raycaster` picked.  The kernels implement exactly one choice of each.
    _ENCODERS = {"pts_tr_fn": "WorldToLocalEncoder", "kp_input_fn": "RelDistEncoder",
                 "view_input_fn": "VecNormEncoder", "bone_input_fn": "VecNormEncoder"}

    def _check_preproc_kwargs(self, pk):
        if not pk:
            return
        cfg = self.cfg
        unknown = set(pk) - set(self._ENCODERS) - {"density_scale", "density_fn"}
        if unknown:
            raise NotImplementedError(f"preproc_kwargs {sorted(unknown)} are not supported by the HIP renderer")
        for key, want in self._ENCODERS.items():
            fn = pk.get(key)
            if fn is not None and type(fn).__name__ != want:
                raise NotImplementedError(f"preproc_kwargs[{key!r}] is a {type(fn).__name__}; the HIP kernels compute {want} only")
        ds = pk.get("density_scale")
        if ds is not None and float(ds) != float(cfg.density_scale):
            raise ValueError(f"preproc_kwargs['density_scale']={float(ds)} but the caster was created with "
                             f"density_scale={cfg.density_scale} (RenderConfig)")
        dfn = pk.get("density_fn")
        if dfn is not None:
            # any callable may arrive here (get_density_fn returns F.relu or a lambda): compare it with the
            # configured activation on probe values instead of guessing from its identity
            x = torch.tensor([-30., -2., -0.25, 0., 0.5, 1., 3., 25.])
            want = torch.relu(x) if cfg.density_type == "relu" else torch.nn.functional.softplus(x - cfg.softplus_shift, beta=1)
            got = torch.as_tensor(dfn(x)).detach().float().cpu()
            if got.shape != want.shape or not torch.allclose(got, want, rtol=1e-6, atol=1e-7):
                raise NotImplementedError(
                    f"preproc_kwargs['density_fn'] is not the configured density activation (density_type={cfg.density_type!r}"
                    + (f", softplus_shift={cfg.softplus_shift}" if cfg.density_type != "relu" else "")
                    + "): create the caster with the matching RenderConfig")

    def training_draws(self, n, S, N, perturb=0., raw_noise_std=0., ray_noise_std=0., pytest=False):
        return make_training_draws(n, S, N, perturb, raw_noise_std, ray_noise_std, pytest=pytest,
                                   density_scale=self.cfg.density_scale, device=self.renderer.device)


def make_training_draws(n, S, N, perturb=0., raw_noise_std=0., ray_noise_std=0., pytest=False,
                        density_scale=1., device="cpu"):
    """The random numbers one training-mode render_rays call consumes, in the reference's
    places: t_rand (ray_utils.py:238-244), u_rand (ray_utils.py:166-180), the density noise
    randn * raw_noise_std * B of both passes (nerf.py:174-182; pytest: rand * raw_noise_std,
    numpy, no B) and the position noise randn * ray_noise_std (raycasters.py:660-661, 673-674)."""
    dev = device
    d = {}
    f32 = lambda a: torch.Tensor(a).to(dev)
    if perturb and perturb > 0.:
        if pytest:
            np.random.seed(0); d["t_rand"] = f32(np.random.rand(n, S))
            if N > 0:
                np.random.seed(0); d["u_rand"] = f32(np.random.rand(n, N))
        else:
            d["t_rand"] = torch.rand(n, S, device=dev)
            if N > 0:
                d["u_rand"] = torch.rand(n, N, device=dev)
    if raw_noise_std and raw_noise_std > 0.:
        B = float(density_scale)
        for key, m in (("noise0", S),) + ((("noise1", S + N),) if N > 0 else ()):
            if pytest:
                np.random.seed(0); d[key] = f32(np.random.rand(n, m) * raw_noise_std)
            else:
                d[key] = torch.randn(n, m, device=dev) * (raw_noise_std * B)
    if ray_noise_std and ray_noise_std > 0.:
        d["ray_noise"] = torch.randn(n, S + N, 3, device=dev) * ray_noise_std
    return d


def create_raycaster(cfg: RenderConfig, ckpt=None, device="cuda:0", precision=PREC_BF16, devices=None):
    """Counterpart of `create_raycaster` (core/raycasters.py:17-184) for rendering:
    returns `render_kwargs_test` with the HIP caster under 'ray_caster'.  `devices` = the GPUs the
    reference would hand to nn.DataParallel (raycasters.py:157).  `ckpt`: one checkpoint, or a list of them: a bank with
    one subject per checkpoint (render_path's subject_idxs picks per frame)."""
    caster = HipRayCaster(cfg, device, precision, devices=devices)
    if isinstance(ckpt, (list, tuple)):
        caster.set_subject_count(len(ckpt))
        for s, c in enumerate(ckpt):
            caster.load_subject(s, c)
    elif ckpt is not None:
        caster.load_state_dict(ckpt)
    caster.eval()
    return {"ray_caster": caster, "perturb": False, "N_importance": cfg.n_importance,
            "N_samples": cfg.n_samples, "use_viewdirs": True, "raw_noise_std": 0., "ray_noise_std": 0.,
            "ext_scale": cfg.ext_scale, "preproc_kwargs": {"density_scale": cfg.density_scale}, "lindisp": cfg.lindisp,
            "nerf_type": "nerf"}


def find_checkpoint(basedir: str, expname: str, ft_path: Optional[str] = None, no_reload: bool = False) -> Optional[str]:
    """The checkpoint `create_raycaster` would reload (core/raycasters.py:124-141): `ft_path` if given (and not
    the string 'None'), otherwise the LAST entry, in sorted name order, of basedir/expname whose name contains
    'tar' and not 'pose'; None when there is none or `no_reload` is set."""
    import os
    if ft_path is not None and ft_path != "None":
        ckpts = [ft_path]
    else:
        d = os.path.join(basedir, expname)
        ckpts = [os.path.join(d, f) for f in sorted(os.listdir(d)) if "tar" in f and "pose" not in f]
    return ckpts[-1] if ckpts and not no_reload else None


_RAYCASTER_CACHE: Dict[tuple, dict] = {}


def load_raycaster(ckpt_path, cfg: RenderConfig, device="cuda:0", precision=PREC_BF16, devices=None):
    """`create_raycaster` on an A-NeRF checkpoint file (`.tar`, the reference's five state dicts,
    core/raycasters.py:752-766), memoised on (path, mtime, size, config, device, precision).  A list of paths gives ONE
    memoised bank with a subject per file, in the list's order.

    The reference's `run_render` reloads and re-wraps the checkpoint on every call of the GAN
    loop (run_gan.py:135-165, 2290-2330); here a repeated call returns the caster whose packed
    weights are already resident on the device."""
    import os
    if isinstance(precision, str):
        precision = PREC_BY_NAME[precision]
    many = isinstance(ckpt_path, (list, tuple))
    paths = [os.fspath(p) for p in ckpt_path] if many else [ckpt_path]
    stamp = lambda p, st: (os.path.abspath(p), st.st_mtime_ns, st.st_size)
    files = tuple(stamp(p, os.stat(p)) for p in paths)
    key = (files if many else files[0]) + (repr(cfg), str(device), int(precision), None if devices is None else tuple(devices))
    kw = _RAYCASTER_CACHE.get(key)
    if kw is None:
        ckpts = [torch.load(p, map_location="cpu", weights_only=False) for p in paths]
        kw = create_raycaster(cfg, ckpts if many else ckpts[0], device=device, precision=precision, devices=devices)
        _RAYCASTER_CACHE[key] = kw
    return dict(kw)
