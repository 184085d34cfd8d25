"""GPU tests of the single-net training step (`SingleNetTrainableRayCaster`; pg_train.hip: one net on one tape pass of
S + N rows per ray, merged_composite_bwd_kernel, one backward): against the reference's own autograd (fixtures
train_grads_single, train_grads_single_v4, train_grads_single_pose) and against a restatement of the step from the oracle's
pieces (tests/test_train_single_host.py, pinned there to the same fixtures)."""
import numpy as np
import pytest
import torch

from posegen_amd import synthetic as syn
from posegen_amd.config import surreal_config, surreal_single_config
from tests.helpers import golden_draws, load_golden, loss_of
from tests.test_pose_grad_host import scale_of
from tests.test_train_single_host import single_cfg, single_model, single_net_grads
from tools.gen_golden import grad_sample_index

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def _wrap(cfg, w, tv, td, train_precision="fp32", precision="fp32", opt_pose=False):
    from posegen_amd.raycaster import HipRayCaster
    from posegen_amd.train import make_trainable
    c = HipRayCaster.from_weights(cfg, w, None, float(tv), float(td), device=DEV, precision=precision)
    m = make_trainable(c, train_precision=train_precision, opt_pose=opt_pose)
    m.train()
    return m


def _trainable(g, **kw):
    cfg = single_cfg(g)
    w, tv, td = single_model(cfg, g)
    return cfg, _wrap(cfg, w, float(g["tau_v"]) if "tau_v" in g else tv, float(g["tau_d"]) if "tau_d" in g else td, **kw)


def _step(m, cfg, g, sk=None, cy=None, loss_fn=loss_of):
    m.zero_grad()
    out = m(torch.tensor(g["ray_batch"]), N_samples=cfg.n_samples, skts=torch.tensor(g["skts"]) if sk is None else sk,
            cyls=torch.tensor(g["cyl"]) if cy is None else cy, N_importance=cfg.n_importance, draws=golden_draws(g))
    loss = loss_fn(out, torch.tensor(g["target"], device=DEV))
    loss.backward()
    return out, float(loss.detach()), {k: p.grad.clone() for k, p in m.network.named_parameters()}


def _grad_devs(grads, g):
    """per tensor (entry deviation / scale, norm deviation / norm) against the fixture's sampled gradients"""
    devs = {}
    for k, gr in grads.items():
        ref_vals, ref_norm = g[f"gval_coarse_{k}"], float(g[f"gnorm_coarse_{k}"])
        got = gr.detach().cpu().numpy().reshape(-1)
        scale = max(float(np.abs(ref_vals).max()), ref_norm / np.sqrt(got.size), 1e-12)
        devs[k] = (float(np.abs(got[grad_sample_index(got.size)] - ref_vals).max()) / scale,
                   abs(float(np.linalg.norm(got.astype(np.float64))) - ref_norm) / max(ref_norm, 1e-12))
    return devs


@pytest.mark.parametrize("name", ["train_grads_single", "train_grads_single_v4"])
def test_single_net_gradients_match_the_reference_autograd(name):
    """fp32 mode: the four maps within 2e-5, the loss within 1e-5, every parameter tensor of the ONE net (24, each once) within
    1e-4 of its scale and of its norm -- the bounds of tests/test_gpu_train.py for the two-net step."""
    g = load_golden(name)
    cfg, m = _trainable(g)
    out, loss, grads = _step(m, cfg, g)
    for k in ("rgb_map", "acc_map", "rgb0", "acc0"):
        assert float(np.abs(out[k].detach().cpu().numpy() - g[k]).max()) <= 2e-5, k
    assert abs(loss - float(g["loss"])) <= 1e-5 * max(1.0, abs(float(g["loss"])))
    devs = _grad_devs(grads, g)
    print(f"[{name}] fixture grad_sensitivity {float(g['grad_sensitivity']):.2e}; worst entry deviation "
          f"{max(d[0] for d in devs.values()):.2e}, worst norm deviation {max(d[1] for d in devs.values()):.2e}")
    assert len(devs) == 24
    for k, (e, nrm) in devs.items():
        assert e <= 1e-4 and nrm <= 1e-4, (k, e, nrm)
    assert tuple(grads["views_linears.0.weight"].shape) == (128, 256 + (72 if cfg.multires_views == 0 else 648))
    m.renderer.close()


def test_single_net_pose_gradient_matches_the_reference_autograd():
    """train_grads_single_pose: dL/dskts of every ray (S coarse + N new points each) within 1e-4 of its scale and norm, and
    the parameter gradients of the same backward within 1e-4 (the bounds of tests/test_gpu_pose_grad.py)."""
    g = load_golden("train_grads_single_pose")
    cfg, m = _trainable(g, opt_pose=True)
    idx = g["kp_idx"]
    sk = torch.tensor(g["skts"][idx]).requires_grad_(True)
    out, loss, grads = _step(m, cfg, g, sk=sk, cy=torch.tensor(g["cyl"][idx]))
    assert abs(loss - float(g["loss"])) <= 1e-5 * max(1.0, abs(float(g["loss"])))
    got, ref = sk.grad.numpy().astype(np.float64), g["dskts"].astype(np.float64)
    ent = float(np.abs(got - ref).max()) / scale_of(ref)
    nrm = abs(float(np.linalg.norm(got)) - float(np.linalg.norm(ref))) / float(np.linalg.norm(ref))
    devs = _grad_devs(grads, g)
    print(f"[train_grads_single_pose] grad_sensitivity {float(g['grad_sensitivity']):.2e}; dL/dskts within {ent:.2e} / {nrm:.2e}; "
          f"parameters within {max(max(d) for d in devs.values()):.2e}")
    assert ent <= 1e-4 and nrm <= 1e-4
    assert all(e <= 1e-4 and n_ <= 1e-4 for e, n_ in devs.values())
    assert bool((sk.grad[..., 3, :] == 0).all())
    # bitwise repeatable, pose gradient included
    g1 = sk.grad.clone()
    sk.grad = None
    _, _, grads2 = _step(m, cfg, g, sk=sk, cy=torch.tensor(g["cyl"][idx]))
    assert torch.equal(g1, sk.grad) and all(torch.equal(grads[k], grads2[k]) for k in grads)
    m.renderer.close()


@pytest.mark.parametrize("name", ["train_grads_single", "train_grads_single_v4"])
def test_single_net_bf16_mode_is_close_and_repeatable(name):
    """The bf16 tape on the same fixtures at the mode's asserted bounds: loss 2e-3, gradient norms 1e-2, single
    entries 1e-1 of the tensor's largest; bitwise the same on a second run."""
    g = load_golden(name)
    cfg, m = _trainable(g, train_precision="bf16")
    out, loss, grads = _step(m, cfg, g)
    devs = _grad_devs(grads, g)
    print(f"[{name}] bf16 tape: loss deviation {abs(loss - float(g['loss'])):.2e}, worst entry {max(d[0] for d in devs.values()):.2e}, "
          f"worst norm {max(d[1] for d in devs.values()):.2e}")
    assert abs(loss - float(g["loss"])) <= 2e-3 * max(1.0, abs(float(g["loss"])))
    for k, (e, nrm) in devs.items():
        assert torch.isfinite(grads[k]).all() and nrm <= 1e-2 and e <= 1e-1, (k, e, nrm)
    _, loss2, grads2 = _step(m, cfg, g)
    assert loss2 == loss and all(torch.equal(grads[k], grads2[k]) for k in grads)
    m.renderer.close()


def test_training_mode_forward_is_the_renderers():
    """rays_single_train (perturb, raw noise, ray noise) through the wrapper in training mode: the fp32 bounds
    tests/test_gpu_single_net.py holds the renderer to on the same fixture (maps 1e-4, alpha 2e-4 at its 99th percentile)."""
    g = load_golden("rays_single_train")
    cfg, m = _trainable(g)
    rb = torch.tensor(g["ray_batch"])
    n = rb.shape[0]
    out = m(rb, N_samples=cfg.n_samples, kp_batch=torch.tensor(g["kps"]).expand(n, -1, -1), skts=torch.tensor(g["skts"]).expand(n, -1, -1, -1),
            cyls=torch.tensor(g["cyl"]).expand(n, -1), bones=torch.tensor(g["bones"]).expand(n, -1, -1), N_importance=cfg.n_importance,
            perturb=float(g["perturb"]), raw_noise_std=float(g["raw_noise_std"]), ray_noise_std=float(g["ray_noise_std"]), pytest=True,
            draws=golden_draws(g))
    assert out["rgb_map"].grad_fn is not None and not out["alpha"].requires_grad
    assert out["alpha"].shape == (n, cfg.n_samples + cfg.n_importance) and out["alpha0"].shape == (n, cfg.n_samples)
    errs = {k: float(np.nanmax(np.abs(out[k].detach().cpu().numpy().astype(np.float64) - g[k]))) for k in ("rgb_map", "acc_map", "rgb0", "acc0", "disp_map")}
    for a in ("alpha", "alpha0"):
        errs[a] = float(np.quantile(np.abs(out[a].cpu().numpy().astype(np.float64) - g[a]), 0.99))
    print("[rays_single_train, training-mode wrapper] " + " ".join(f"{k}={v:.2e}" for k, v in errs.items()))
    for k in ("rgb_map", "acc_map", "rgb0", "acc0", "disp_map"):
        assert errs[k] <= 1e-4, (k, errs[k])
    assert errs["alpha"] <= 2e-4 and errs["alpha0"] <= 2e-4
    m.renderer.close()


def _restated(cfg, w, tv, td, rb, sk, cy, target, draws, dtype, loss_fn=loss_of):
    return single_net_grads(cfg, w, tv, td, rb, sk, cy, target, cfg.n_samples, cfg.n_importance, draws, dtype=dtype, loss_fn=loss_fn)


@pytest.mark.parametrize("train_precision", ["fp32", "bf16"])
def test_odd_batch_against_the_restated_step(train_precision):
    """25 rays x 33 + 7 of the shipped single-net model (multires_views = 0): 825 coarse and 175 new rows end inside a tile of
    every GEMM, and the new rows start at an odd offset of the pass.  Reference: the restatement in float64.  fp32 mode: every
    tensor within 1e-4 of its scale, or within 4 x the float32 restatement's own deviation from float64 where the batch (it is
    not conditioning-filtered like the fixtures) makes that larger; bf16: the odd-batch bounds of tests/test_gpu_train.py
    (norms 2e-2, entries 1e-1)."""
    from posegen_amd.raycaster import make_training_draws
    g = load_golden("train_grads_single")
    cfg = surreal_single_config(n_samples=33, n_importance=7)
    w, _, tv, td = syn.make_model(cfg, 4)
    n = 25
    rb, sk, cy, target = g["ray_batch"][:n], g["skts"], g["cyl"], g["target"][:n]
    draws = make_training_draws(n, 33, 7, perturb=1., raw_noise_std=1., pytest=True)
    _, _, ref, _ = _restated(cfg, w, tv, td, rb, sk, cy, target, draws, torch.float64)
    _, _, own, _ = _restated(cfg, w, tv, td, rb, sk, cy, target, draws, torch.float32)
    m = _wrap(cfg, w, tv, td, train_precision=train_precision)
    out = m(torch.tensor(rb), N_samples=33, skts=torch.tensor(sk), cyls=torch.tensor(cy), N_importance=7, draws={k: v.to(DEV) for k, v in draws.items()})
    loss_of(out, torch.tensor(target, device=DEV)).backward()
    worst = 0.0
    for k, p in m.network.named_parameters():
        r, got = ref[k].reshape(-1), p.grad.detach().cpu().numpy().reshape(-1).astype(np.float64)
        scale = max(float(np.abs(r).max()), float(np.linalg.norm(r)) / np.sqrt(r.size), 1e-12)
        e = float(np.abs(got - r).max()) / scale
        rn = float(np.linalg.norm(r))
        nerr = abs(float(np.linalg.norm(got)) - rn) / max(rn, 1e-12)
        worst = max(worst, e, nerr)
        if train_precision == "fp32":
            o = float(np.abs(own[k].reshape(-1) - r).max()) / scale
            assert e <= max(1e-4, 4.0 * o), (k, e, o)
        else:
            assert np.isfinite(got).all() and nerr <= 2e-2 and e <= 1e-1, (k, e, nerr)
    print(f"odd single-net batch, {train_precision}: worst relative gradient deviation {worst:.2e}")
    m.renderer.close()


def test_loss_curves_follow_the_restated_step():
    """30 Adam steps (lrate 5e-4) on one batch with fixed draws, multires_views = 0, 32 + 8: the restatement in float64 (the
    reference curve) and in float32 (the arithmetic's own sensitivity), the HIP step in fp32 and on the bf16 tape.  fp32 within
    1e-4 relative at every step -- or 4 x the float32 restatement's deviation from float64 where that is larger (both printed) --,
    bf16 within 5e-2; all fall.  Measured: the float32 restatement itself leaves the float64 curve by 3.78e-4 (30 Adam steps
    amplify fp32 rounding: the bound in force is 4 x that = 1.5e-3), the HIP fp32 step by 3.44e-4, the bf16 tape by 4.4e-3."""
    from posegen_amd.raycaster import make_training_draws
    g = load_golden("train_grads_single")
    cfg = surreal_single_config(n_samples=32, n_importance=8)
    w, _, tv, td = syn.make_model(cfg, 4)
    n, steps = 48, 30
    rb, sk, cy, target = g["ray_batch"][:n], g["skts"], g["cyl"], g["target"][:n]
    draws = make_training_draws(n, 32, 8, perturb=1., raw_noise_std=1., pytest=True)
    from tests.helpers import default_dtype, oracle_cfg
    from tests.test_train_single_host import single_net_render
    curves = {}
    for dtype in (torch.float64, torch.float32):
        with default_dtype(dtype):
            cast = lambda x: torch.as_tensor(x).to(dtype)
            tw = {k: torch.tensor(np.asarray(v), dtype=dtype, requires_grad=True) for k, v in w.items()}
            opt = torch.optim.Adam(list(tw.values()), lr=5e-4, betas=(0.9, 0.999))
            cur = []
            for it in range(steps):
                opt.zero_grad()
                loss = loss_of(single_net_render(cast(rb), cast(sk), cast(cy), oracle_cfg(cfg, tv, td), tw, 32, 8,
                                                 {k: cast(v) for k, v in draws.items()}), cast(target))
                loss.backward()
                opt.step()
                cur.append(float(loss.detach()))
        curves[dtype] = cur
    ref = curves[torch.float64]
    rel = lambda a: max(abs(x - y) / max(abs(y), 1e-12) for x, y in zip(a, ref))
    own = rel(curves[torch.float32])
    hip = {}
    for tp in ("fp32", "bf16"):
        m = _wrap(cfg, w, tv, td, train_precision=tp, precision="bf16")
        o = torch.optim.Adam(m.parameters(), lr=5e-4, betas=(0.9, 0.999))
        assert len(o.param_groups[0]["params"]) == 24 + 2          # the net's tensors once + the two cutoff_dist (no gradient)
        cur = []
        for it in range(steps):
            o.zero_grad()
            out = m(torch.tensor(rb), N_samples=32, skts=torch.tensor(sk), cyls=torch.tensor(cy), N_importance=8,
                    draws={k: v.to(DEV) for k, v in draws.items()})
            loss = loss_of(out, torch.tensor(target, device=DEV))
            loss.backward()
            o.step()
            cur.append(float(loss.detach()))
        hip[tp] = cur
        m.renderer.close()
    d32, d16 = rel(hip["fp32"]), rel(hip["bf16"])
    print(f"single-net loss {ref[0]:.5f} -> {ref[-1]:.5f} (float64 restatement); curve deviation: float32 restatement {own:.2e}, "
          f"HIP fp32 {d32:.2e}, HIP bf16 {d16:.2e}")
    assert ref[-1] < ref[0] and hip["fp32"][-1] < hip["fp32"][0] and hip["bf16"][-1] < hip["bf16"][0]
    assert d32 <= max(1e-4, 4.0 * own), (d32, own)
    assert d16 <= 5e-2, d16


def test_shared_parameters_are_shared():
    """The one parameter set collects three paths.  Loss on the fine maps only / on the coarse maps only: both non-zero and
    different; with the coarse-only loss the new rows contribute nothing (equal to the restatement's gradient, whose new
    points are then off the graph); the two partial gradients add up to the full one within 1e-6 of the tensor's largest."""
    g = load_golden("train_grads_single")
    cfg, m = _trainable(g)
    fine_only = lambda out, t: torch.mean((out["rgb_map"] + (1. - out["acc_map"])[..., None] - t) ** 2)
    coarse_only = lambda out, t: torch.mean((out["rgb0"] + (1. - out["acc0"])[..., None] - t) ** 2)
    _, _, full = _step(m, cfg, g)
    _, _, gf = _step(m, cfg, g, loss_fn=fine_only)
    _, _, gc = _step(m, cfg, g, loss_fn=coarse_only)
    w, tv, td = single_model(cfg, g)
    _, _, ref_c, _ = single_net_grads(cfg, w, float(g["tau_v"]), float(g["tau_d"]), g["ray_batch"], g["skts"], g["cyl"], g["target"],
                                      cfg.n_samples, cfg.n_importance, golden_draws(g), dtype=torch.float64, loss_fn=coarse_only)
    for k in full:
        big = float(full[k].abs().max())
        assert float(gf[k].abs().max()) > 0 and float(gc[k].abs().max()) > 0, k
        assert float((full[k] - gf[k]).abs().max()) > 1e-3 * big, k                 # the coarse source is present
        assert float((gf[k] + gc[k] - full[k]).abs().max()) <= 1e-6 * big, k
        r = ref_c[k]
        scale = max(float(np.abs(r).max()), 1e-12)
        assert float(np.abs(gc[k].cpu().numpy().astype(np.float64) - r).max()) <= 1e-4 * scale, k
    m.renderer.close()


@pytest.mark.parametrize("precision", ["fp32", "bf16"])
def test_widened_columns_stay_dead_and_the_device_sync_is_the_host_packing(precision):
    """5 Adam steps on the multires_views = 0 model, then: the wrapper's eval render (device-side sync) is BITWISE the render of
    a fresh HipRayCaster loaded from its state_dict() -- whose loader widens the [128, 328] view weight with exact zeros, so any
    non-zero sin / cos column in the trained images would show -- and the checkpoint has the reference's single-net layout."""
    from posegen_amd.raycaster import HipRayCaster
    g = load_golden("train_grads_single")
    cfg, m = _trainable(g, precision=precision)
    opt = torch.optim.Adam(m.parameters(), lr=5e-3)
    for it in range(5):
        _step(m, cfg, g)
        opt.step()
    assert m._stale
    rb, sk, cy = torch.tensor(g["ray_batch"]), torch.tensor(g["skts"]), torch.tensor(g["cyl"])
    m.eval()
    with torch.no_grad():
        want = m(rb, N_samples=cfg.n_samples, skts=sk, cyls=cy, N_importance=cfg.n_importance)
    assert not m._stale
    sd = m.state_dict()
    assert tuple(sd["network_fn_state_dict"]["views_linears.0.weight"].shape) == (128, 328)
    assert set(sd) == {"network_fn_state_dict", "network_fine_state_dict", "embed_state_dict", "embedbones_state_dict", "embeddirs_state_dict"}
    assert all(torch.equal(sd["network_fn_state_dict"][k], sd["network_fine_state_dict"][k]) for k in sd["network_fn_state_dict"])
    w0, _, _ = single_model(cfg, g)
    assert not torch.equal(sd["network_fn_state_dict"]["views_linears.0.weight"], torch.tensor(w0["views_linears.0.weight"]))
    fresh = HipRayCaster(cfg, device=DEV, precision=precision)
    fresh.load_state_dict(sd)
    got = fresh(rb, N_samples=cfg.n_samples, skts=sk, cyls=cy, N_importance=cfg.n_importance)
    for k in ("rgb_map", "acc_map", "disp_map", "rgb0", "acc0"):
        assert torch.equal(got[k], want[k]), k
    # the inner caster's own state follows the parameters (both keys)
    inner = m.caster.state_dict()
    for key in ("network_fn_state_dict", "network_fine_state_dict"):
        assert all(torch.equal(inner[key][k], sd["network_fn_state_dict"][k]) for k in sd["network_fn_state_dict"]), key
    fresh.renderer.close()
    m.renderer.close()


def test_repeatability_and_the_one_tape():
    from posegen_amd._ffi import PG_ESTATE, PgError
    g = load_golden("train_grads_single_v4")
    cfg, m = _trainable(g)
    _, l1, g1 = _step(m, cfg, g)
    _, l2, g2 = _step(m, cfg, g)
    assert l1 == l2 and all(torch.equal(g1[k], g2[k]) for k in g1)
    rb, sk, cy = torch.tensor(g["ray_batch"]), torch.tensor(g["skts"]), torch.tensor(g["cyl"])
    target = torch.tensor(g["target"], device=DEV)
    call = lambda rays: m(rays, N_samples=cfg.n_samples, skts=sk, cyls=cy, N_importance=cfg.n_importance)
    first = loss_of(call(rb[:24]), target[:24])
    second = loss_of(call(rb[8:40]), target[8:40])
    with pytest.raises(PgError) as ei:
        first.backward()
    assert ei.value.code == PG_ESTATE and "overwritten" in str(ei.value)
    second.backward()
    with pytest.raises(TypeError):
        m(rb, N_samples=cfg.n_samples, skts=sk, cyls=cy, N_importance=cfg.n_importance, no_such_argument=1)
    with pytest.raises(NotImplementedError, match="skts requires a gradient"):
        m(rb, N_samples=cfg.n_samples, skts=sk.clone().requires_grad_(True), cyls=cy, N_importance=cfg.n_importance)
    m.renderer.close()


def test_the_seam():
    from posegen_amd import make_trainable
    from posegen_amd.raycaster import NET_TENSOR_ORDER, HipRayCaster
    from posegen_amd.train import SingleNetTrainableRayCaster, TrainableRayCaster
    two_cfg, one_cfg = surreal_config(), surreal_single_config()
    two = HipRayCaster.from_weights(two_cfg, *syn.make_model(two_cfg, 0), device=DEV, precision="fp32")
    one = HipRayCaster.from_weights(one_cfg, syn.make_weights(one_cfg, 0), None, 79.6, 79.6, device=DEV, precision="fp32")
    try:
        a, b = make_trainable(two), make_trainable(one, train_precision="bf16")
        assert type(a) is TrainableRayCaster and type(b) is SingleNetTrainableRayCaster and b.train_precision == "bf16"
        with pytest.raises(ValueError):
            SingleNetTrainableRayCaster(two)
        with pytest.raises(NotImplementedError):
            TrainableRayCaster(one)
        assert b.network_fine is b.network and b.get_networks() == (b.network, b.network)
        trainable = [p for p in b.parameters() if p.requires_grad]
        assert len(trainable) == len(NET_TENSOR_ORDER) == 24 and len(list(b.parameters())) == 26
        assert len([p for p in a.parameters() if p.requires_grad]) == 48
        assert b.module is b and b.get_embed_fns()[1] is None
        assert tuple(dict(b.network.named_parameters())["views_linears.0.weight"].shape) == (128, 328)
    finally:
        two.renderer.close()
        one.renderer.close()
