"""The A-NeRF training step on the HIP path: `render` in training mode with a gradient.

In the reference, `Trainer.train_batch` (core/trainer.py:232-275) renders a ray batch through
`render_kwargs_train['ray_caster']`, forms the loss from rgb_map / acc_map / rgb0 / acc0 (trainer.py:321-383) and calls
`loss.backward()` (trainer.py:463): autograd walks back through compositing, both MLPs and the embedding's inputs.
`TrainableRayCaster` gives the HIP caster the same property: its parameters are ordinary torch Parameters on the
device (an optimiser owns them), its call returns tensors that carry a grad_fn, and backward runs in the library
(`pg_train_forward` / `pg_train_backward`, csrc/pg_train.hip) -- exact fp32, activations kept on a tape inside the
handle.  disp_map and the alpha tensors are returned without a gradient (the reference's losses do not read them).
"""
from __future__ import annotations

import ctypes as C
from typing import Dict, Optional

import torch

from . import _ffi
from .raycaster import (NET_TENSOR_ORDER, HipRayCaster, _dev_f32, _resolve_sn, alloc_ray_outputs,
                        check_single_net_states, make_training_draws, marshal_ray_call, one_nanmean_group,
                        refuse_reference_kwargs)


class _RenderRaysFn(torch.autograd.Function):
    """outputs (rgb_map, acc_map, rgb0, acc0, disp_map, disp0, alpha, alpha0) of one training-mode render_rays call (the alphas
    only for a single-net caster, empty otherwise); differentiable
    with respect to the 24 (+ frame codes) tensors of each net and, with opt_pose, to `skts` (the caller's tensor as passed:
    [n,24,4,4] gets one gradient per ray -- an expanded single pose included, autograd's ExpandBackward sums them --,
    [1,24,4,4] / [24,4,4] the sum over the rays)."""

    @staticmethod
    def forward(ctx, caster, call, skts, *params):
        r = caster.renderer
        dev = r.device
        n, S, N = call.n, call.S, call.N                 # (`call`: the RayCall of raycaster.marshal_ray_call)
        ctx.skts_shape, ctx.skts_dtype, ctx.skts_device = tuple(skts.shape), skts.dtype, skts.device
        nper = 24 + (1 if caster.cfg.framecode_ch > 0 else 0)
        single = bool(caster.cfg.single_net)             # one parameter set: network_fine is network
        nets = [params[:nper], params[nper:2 * nper]] if N > 0 and not single else [params[:nper]]
        keep = list(call.keep)
        structs = []
        for tens in nets:
            st = _ffi.PgNetParams()
            for i in range(24):
                t = tens[i].detach()
                if not (t.is_contiguous() and t.dtype == torch.float32 and t.device == dev):
                    raise ValueError("training parameters must be contiguous float32 tensors on the caster's device")
                st.w[i] = t.data_ptr()
            if nper == 25:
                codes = tens[24].detach()
                ext = torch.cat([codes, codes.mean(0, keepdim=True)], 0).contiguous()      # embedding.py:25-26
                keep.append(ext)
                st.codes, st.n_codes = ext.data_ptr(), codes.shape[0]
            structs.append(st)
        # the maps always; the alphas for a single-net caster, whose call in the reference returns them besides the maps
        out, _, po = alloc_ray_outputs(n, S, N, dev, want_alpha=single)
        tape = C.c_int64(0)
        _ffi.call(r, "pg_train_forward", n, call.rb, call.sk, call.ps, call.cy, call.cs, call.cam, S, N, call.flags,
                  None if call.draws is None else C.byref(call.draws), C.byref(structs[0]),
                  C.byref(structs[1]) if len(structs) > 1 else None, C.byref(po), C.byref(tape))
        ctx.caster, ctx.n_nets, ctx.nper, ctx.keep, ctx.tape_id = caster, len(nets), nper, keep, tape.value
        ctx.shapes = [tuple(p.shape) for p in params]
        zero = lambda k: out[k] if k in out else torch.zeros(0, device=dev)
        outs = (out["rgb_map"], out["acc_map"], zero("rgb0"), zero("acc0"), out["disp_map"], zero("disp0"), zero("alpha"), zero("alpha0"))
        ctx.mark_non_differentiable(*outs[4:])
        return outs

    @staticmethod
    def backward(ctx, g_rgb, g_acc, g_rgb0, g_acc0, _g_disp, _g_disp0, _g_alpha=None, _g_alpha0=None):
        caster = ctx.caster
        r = caster.renderer
        dev = r.device
        grads = [torch.empty(s, device=dev, dtype=torch.float32) for s in ctx.shapes]
        structs = []
        for k in range(ctx.n_nets):
            st = _ffi.PgNetGrads()
            for i in range(24):
                st.w[i] = grads[k * ctx.nper + i].data_ptr()
            if ctx.nper == 25:
                st.codes = grads[k * ctx.nper + 24].data_ptr()
            structs.append(st)
        for g in grads[ctx.n_nets * ctx.nper:]:         # (parameters of a fine net that this call did not use)
            g.zero_()
        gp = lambda g: None if g is None or g.numel() == 0 else _dev_f32(g, dev)
        a, b, c, d = gp(g_rgb), gp(g_acc), gp(g_rgb0), gp(g_acc0)
        # (a forward pass in between has overwritten the handle's one tape: the library refuses the stale id)
        nets = (C.byref(structs[0]), C.byref(structs[1]) if ctx.n_nets > 1 else None)
        d_skts = None
        if ctx.needs_input_grad[2]:                     # pose refinement: dL/dskts with the parameter gradients, in one pass
            shape = ctx.skts_shape
            per_ray = len(shape) == 4 and shape[0] > 1
            d_skts = torch.empty((shape[0] if per_ray else 1, 24, 4, 4), device=dev, dtype=torch.float32)
            _ffi.call(r, "pg_train_backward_pose", ctx.tape_id, a, b, c, d, *nets, d_skts, 384 if per_ray else 0)
            d_skts = d_skts.reshape(shape).to(device=ctx.skts_device, dtype=ctx.skts_dtype)
        else:
            _ffi.call(r, "pg_train_backward", ctx.tape_id, a, b, c, d, *nets)
        caster._stale = True                            # (an optimiser step follows: the inference kernels' packed weights lag from here)
        return (None, None, d_skts) + tuple(grads)


class _NetParams(torch.nn.Module):
    """The parameters of one NeRF net under the reference's names (core/networks/nerf.py:57-88): pts_linears.{0..7},
    alpha_linear, feature_linear, views_linears.0, rgb_linear (+ framecodes.codes, core/networks/embedding.py).  The
    nn.Linear / nn.Embedding modules are containers only -- the arithmetic runs in the library -- but they make
    `state_dict()` the reference checkpoint's `network_fn_state_dict`, `named_parameters()` its parameter list, and
    `pts_linears[i].parameters()` what get_grad_vars' freeze_weights walks (raycasters.py:194-203)."""

    def __init__(self, sd: Dict[str, torch.Tensor], framecodes: bool, device):
        super().__init__()
        lin = lambda name: self._linear(sd[f"{name}.weight"], sd[f"{name}.bias"], device)
        self.pts_linears = torch.nn.ModuleList([lin(f"pts_linears.{i}") for i in range(8)])
        self.alpha_linear = lin("alpha_linear")
        self.feature_linear = lin("feature_linear")
        self.views_linears = torch.nn.ModuleList([lin("views_linears.0")])
        self.rgb_linear = lin("rgb_linear")
        if framecodes:
            codes = sd["framecodes.codes.weight"]
            self.framecodes = torch.nn.Module()
            self.framecodes.codes = torch.nn.Embedding(codes.shape[0], codes.shape[1], device=device)
            with torch.no_grad():
                self.framecodes.codes.weight.copy_(codes)

    @staticmethod
    def _linear(w, b, device):
        m = torch.nn.Linear(w.shape[1], w.shape[0], device=device)
        with torch.no_grad():
            m.weight.copy_(w)
            m.bias.copy_(b)
        return m

    def tensors(self, names):
        p = dict(self.named_parameters())
        return [p[k] for k in names]


class _EmbedState(torch.nn.Module):
    """State of one CutoffEmbedder as the reference checkpoints it (core/cutoff_embedder.py:89-94): `cutoff_dist`
    Parameter[24] (requires_grad=False, opt_cutoff off) and the `tau` buffer, with the tau schedule of
    update_threshold (cutoff_embedder.py:176-183; the frequency schedule is off in every shipped config)."""

    def __init__(self, renderer, which: int, sd: Dict[str, torch.Tensor]):
        super().__init__()
        self._renderer, self._which = [renderer], which          # (a list: not a sub-module)
        self.cutoff_dist = torch.nn.Parameter(sd["cutoff_dist"].clone().float(), requires_grad=False)
        self.register_buffer("tau", sd["tau"].clone().float().reshape(()))
        self.init_tau = 20.0                                      # CutoffEmbedder(init_tau=20): cutoff_embedder.py:66

    def get_tau(self):
        return float(self.tau)

    def set(self, tau, cutoff_dist=None):
        if cutoff_dist is not None:
            with torch.no_grad():
                self.cutoff_dist.copy_(torch.as_tensor(cutoff_dist).float())
        self.tau.fill_(float(tau))
        self._renderer[0].set_embedder(self._which, float(tau), self.cutoff_dist.detach().cpu().numpy())

    def update_threshold(self, global_step, tau_step, tau_rate, alpha_step=None, alpha_target=None):
        self.set(min(self.init_tau * tau_rate ** (global_step / float(tau_step * 1000)), 2000.))


class TrainableRayCaster(torch.nn.Module):
    """`HipRayCaster` with a gradient: the object to put under `render_kwargs_train['ray_caster']`
    (core/raycasters.py:156-165).  It has the surface the reference's trainer touches: `get_networks()` /
    `get_embed_fns()` (so `get_grad_vars` + Adam, raycasters.py:186-228, work unchanged), `update_embed_fns`
    (trainer.py:265-266), `.module`, and `state_dict()` / `load_state_dict()` in the reference checkpoint layout
    (raycasters.py:752-788: `network_fn_state_dict` with `pts_linears.0.weight`, ..., `embed_state_dict`, ...), which
    `HipRayCaster.load_state_dict`, `load_raycaster` and the reference itself read back.
    `sync_inference_weights()` hands the current values to the fused inference kernels (validation renders); a render
    in eval mode does it by itself when a backward pass or a checkpoint load has changed the parameters since.

    `train_precision`: "fp32" (default: the reference trains in fp32, trainer.py:232-275; gradients within 1e-4 of its
    autograd) or "bf16" (opt-in: the tape and the large GEMMs' operands in bf16, fp32 accumulate).  It is the TRAINING
    step's arithmetic only and independent of the caster's rendering precision (`set_precision`).

    `opt_pose` (the reference's flag, set in its h36m / mixamo / perfcap configs): `skts` may require a gradient -- the
    output of PoseOptLayer (core/pose_opt.py:240-447, core/trainer.py:286-313) -- and `loss.backward()` reaches it through
    the bone-relative transform and the embedding (pg_train_backward_pose).  `kp_batch` / `bones` may require one too and
    receive none, as in the reference (the shipped encoders do not read them).  Rays and cylinders get no gradient."""

    def __init__(self, caster: HipRayCaster, train_precision: str = "fp32", opt_pose: bool = False):
        super().__init__()
        if train_precision not in ("fp32", "bf16"):
            raise ValueError(f"train_precision must be 'fp32' or 'bf16', not {train_precision!r}")
        self._check_model(caster.cfg)
        if getattr(caster, "n_subjects", 1) > 1:
            raise NotImplementedError(f"{type(self).__name__}: training a subject bank is not built (the caster holds "
                                      f"{caster.n_subjects} subjects; train each subject's model in a caster of its own)")
        self.caster = caster
        self.train_precision = train_precision
        self.opt_pose = bool(opt_pose)
        caster.renderer.set_train_precision(train_precision)
        self._stale = False                              # the inference kernels' packed weights lag the parameters
        self.cfg = caster.cfg
        dev = caster.renderer.device
        caster.renderer._refresh_state()                 # (a device-side weight load leaves the host copies to be fetched on demand)
        st = caster.renderer._state
        fc = self.cfg.framecode_ch > 0
        self._names = list(NET_TENSOR_ORDER) + (["framecodes.codes.weight"] if fc else [])
        self.network = _NetParams(st["network_fn_state_dict"], fc, dev)
        if self.cfg.single_net:                         # ONE parameter set under both names (core/raycasters.py:99-104)
            self.network_fine = self.network
        else:
            self.network_fine = _NetParams(st["network_fine_state_dict"], fc, dev) if "network_fine_state_dict" in st else None
        self.embed_fn = _EmbedState(caster.renderer, 0, st["embed_state_dict"])
        self.embedbones_fn = None                       # multires_bones = 0: a parameter-free identity Embedder
        self.embeddirs_fn = _EmbedState(caster.renderer, 1, st["embeddirs_state_dict"])

    @staticmethod
    def _check_model(cfg):
        """This class is the two-net step with the 4-band view embedding; it refuses everything else rather than train the
        wrong thing.  Single-net models train through SingleNetTrainableRayCaster (`make_trainable` picks the class)."""
        if cfg.single_net:
            raise NotImplementedError("TrainableRayCaster is the two-net training step: a single_net model trains through "
                                      "SingleNetTrainableRayCaster (posegen_amd.make_trainable picks the class)")
        if cfg.multires_views != 4:
            raise NotImplementedError("TrainableRayCaster: two nets with multires_views != 4 are not trained on the HIP path (no "
                                      "shipped config; such models render through HipRayCaster)")

    @property
    def module(self):
        return self

    @property
    def renderer(self):
        return self.caster.renderer

    # ---- the reference RayCaster's accessors (core/raycasters.py:726-794) -----------------------------------------
    def get_networks(self):
        return self.network, self.network_fine

    def get_embed_fns(self):
        return self.embed_fn, self.embedbones_fn, self.embeddirs_fn

    def update_embed_fns(self, global_step, args):
        for fn in (self.embed_fn, self.embeddirs_fn):
            fn.update_threshold(global_step, args.cutoff_step, args.cutoff_rate, getattr(args, "freq_schedule_step", None),
                                self.cfg.multires - 1)

    def state_dict(self, *args, **kwargs):
        """The reference's checkpoint entries (raycasters.py:752-766): one state dict per sub-module."""
        cpu = lambda m: {k: v.detach().cpu().clone() for k, v in m.state_dict().items()}
        sd = {"network_fn_state_dict": cpu(self.network), "embed_state_dict": cpu(self.embed_fn),
              "embedbones_state_dict": {}, "embeddirs_state_dict": cpu(self.embeddirs_fn)}
        if self.network_fine is not None:
            sd["network_fine_state_dict"] = cpu(self.network_fine)
        return sd

    def load_state_dict(self, ckpt, strict=True):
        """Resume from a checkpoint in that layout (written by this class, by HipRayCaster.state_dict or by the
        reference's trainer, trainer.py:496-507): parameters, embedder state and the inference kernels' weights."""
        self.network.load_state_dict(ckpt["network_fn_state_dict"], strict=strict)
        if self.network_fine is not None and ckpt.get("network_fine_state_dict") is not None:
            self.network_fine.load_state_dict(ckpt["network_fine_state_dict"], strict=strict)
        for fn, key in ((self.embed_fn, "embed_state_dict"), (self.embeddirs_fn, "embeddirs_state_dict")):
            e = ckpt.get(key)
            if e is not None and "tau" in e:
                fn.set(float(e["tau"]), e.get("cutoff_dist"))
            elif strict:
                raise KeyError(key)
        self.sync_inference_weights()

    def _flat(self):
        out = self.network.tensors(self._names)
        if self.network_fine is not None and self.network_fine is not self.network:
            out += self.network_fine.tensors(self._names)
        return out

    def net_state_dict(self, which: int) -> Dict[str, torch.Tensor]:
        net = self.network if which == 0 else self.network_fine
        return {k: v.detach().cpu() for k, v in net.state_dict().items()}

    def _state_provider(self, net):
        """What the inner caster's state_dict() / parameters() fetch after a device-side sync: the net's tensors -- after another
        sync if the parameters have moved since, so that the state handed out is the state the kernels render with."""
        def provide():
            if self._stale:
                self.sync_inference_weights()
            return net.state_dict()
        return provide

    def sync_inference_weights(self, on_device: Optional[bool] = None):
        """Hand the current parameter values to the fused inference kernels (after optimiser steps).  on_device (default:
        whenever the renderer has one device): the packed weight images are re-formed on the GPU from the parameter tensors
        themselves (pg_load_weights_device: no host copy, bitwise the host packing); False: through the host (pg_load_weights)."""
        r = self.caster.renderer
        if on_device is None:
            on_device = len(getattr(r, "devices", [0])) <= 1
        nets = [(0, self.network)]
        if self.network_fine is not None and self.network_fine is not self.network:      # (a single-net handle has net 0 only)
            nets.append((1, self.network_fine))
        for which, net in nets:
            if on_device:
                p = dict(net.named_parameters())
                codes = p["framecodes.codes.weight"] if self.cfg.framecode_ch > 0 else None
                r.load_network_device(which, [p[k] for k in NET_TENSOR_ORDER], codes, state_provider=self._state_provider(net))
            else:
                r.load_network(which, self.net_state_dict(which))
        self._stale = False

    def forward(self, ray_batch, N_samples=None, kp_batch=None, skts=None, cyls=None, bones=None, cams=None,
                subject_idxs=None, lindisp=False, perturb=0., N_importance=0, raw_noise_std=0., ray_noise_std=0.,
                pytest=False, draws: Optional[Dict[str, torch.Tensor]] = None, **unused):
        # the reference's keywords the kernels do not honour are refused, in training and in eval mode alike; subject_idxs in
        # training mode only (an eval-mode call hands it to the caster, which checks it against its one subject)
        training = self.training and torch.is_grad_enabled()
        refuse_reference_kwargs("TrainableRayCaster", self.caster._check_preproc_kwargs, skts, cyls,
                                dict(unused, subject_idxs=subject_idxs if training else None), own_fine=self.network_fine)
        if not training:
            if self._stale:                              # a backward pass has run since the last packing: render what was trained
                self.sync_inference_weights()
            return self.caster(ray_batch, N_samples=N_samples, kp_batch=kp_batch, skts=skts, cyls=cyls, bones=bones, cams=cams,
                               subject_idxs=subject_idxs, lindisp=lindisp, perturb=perturb, N_importance=N_importance,
                               raw_noise_std=raw_noise_std, ray_noise_std=ray_noise_std, pytest=pytest, draws=draws)
        # Without opt_pose the backward pass differentiates with respect to the networks' tensors only: a pose that wants a
        # gradient is refused rather than left without one.  With opt_pose (the reference's pose refinement, popt_layer,
        # trainer.py:286-313, 453-485) skts gets dL/dskts; kp_batch / bones are accepted and get none, as in the reference,
        # whose shipped encoders read only skts.  Rays and cylinders are refused either way.
        wanted = ("ray_batch", "cyls") if self.opt_pose else ("ray_batch", "skts", "kp_batch", "cyls", "bones")
        for name, t in (("ray_batch", ray_batch), ("skts", skts), ("kp_batch", kp_batch), ("cyls", cyls), ("bones", bones)):
            if name in wanted and torch.is_tensor(t) and t.requires_grad:
                why = "rays and cylinders get no gradient" if self.opt_pose else \
                    "the HIP training step has no gradient for poses / rays without opt_pose=True"
                raise NotImplementedError(f"{name} requires a gradient: {why}; pass a detached tensor")
        r = self.caster.renderer
        cfg = self.cfg
        S, N = _resolve_sn(cfg, N_samples, int(N_importance or 0))
        if N > 0 and self.network_fine is None:
            raise ValueError("N_importance > 0 needs the fine network")
        n = ray_batch.shape[0]
        if draws is None and (perturb or raw_noise_std or ray_noise_std):
            draws = make_training_draws(n, S, N, perturb, raw_noise_std, ray_noise_std, pytest=pytest,
                                        density_scale=cfg.density_scale, device=r.device)
        skts = torch.as_tensor(skts)
        call = marshal_ray_call(cfg, r.device, ray_batch, skts, cyls, cams, S, N, lindisp, draws)
        with one_nanmean_group(r, n):
            rgb, acc, rgb0, acc0, disp, disp0, alpha, alpha0 = _RenderRaysFn.apply(self, call, skts, *self._flat())
        out = {"rgb_map": rgb, "disp_map": disp, "acc_map": acc}
        if N > 0:
            out.update({"rgb0": rgb0, "disp0": disp0, "acc0": acc0})
        if cfg.single_net:
            out["alpha"] = alpha
            if N > 0:
                out["alpha0"] = alpha0
        return out


class SingleNetTrainableRayCaster(TrainableRayCaster):
    """The training step of a single-net caster (`single_net = True`, configs/surreal/surreal_single.txt; the reference's
    core/raycasters.py:99-104, 446-469): ONE parameter set -- `network_fine is network`, so `parameters()` yields each tensor
    once and `get_grad_vars` builds the optimiser it builds for the reference's own single-net caster -- evaluated at a ray's S
    coarse points and at its N importance points only (S + N rows per ray on the tape instead of 2 S + N).  The loss reads the
    coarse maps and the fine maps, which composite the coarse and the new raw merged by depth; the one set of gradients sums
    the three paths (pg_train.hip: merged_composite_bwd_kernel, one backward of the net over all rows).

    `multires_views = 0`: `views_linears.0.weight` and its gradient have the reference's [128, 256 + 72 (+16)] shape.  The
    library widens a copy to the 4-band layout every step (the sin / cos columns exact zeros) and narrows the gradient back:
    those columns are never parameters.  `state_dict()` holds the one net under both `network_fn_state_dict` and
    `network_fine_state_dict`, as the reference saves it.  A training-mode call also returns `alpha` / `alpha0` (no gradient).
    Everything else -- `train_precision`, `opt_pose`, the refused keywords, the re-sync before an eval-mode render, one
    outstanding tape -- is TrainableRayCaster's."""

    @staticmethod
    def _check_model(cfg):
        if not cfg.single_net:
            raise ValueError("SingleNetTrainableRayCaster needs a single_net caster (two-net models: TrainableRayCaster)")

    def load_state_dict(self, ckpt, strict=True):
        check_single_net_states(ckpt.get("network_fn_state_dict"), ckpt.get("network_fine_state_dict"))
        super().load_state_dict(ckpt, strict=strict)


def make_trainable(caster: HipRayCaster, **kw) -> TrainableRayCaster:
    """The trainable wrapper of `caster`: SingleNetTrainableRayCaster for a single-net caster, TrainableRayCaster otherwise
    (keywords: `train_precision`, `opt_pose`)."""
    cls = SingleNetTrainableRayCaster if caster.cfg.single_net else TrainableRayCaster
    return cls(caster, **kw)
