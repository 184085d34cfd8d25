"""Empty waves of the fused 16x16x32 kernel (pg_eval16r.hip): a wave whose 32 points all have
sigma <= 0 leaves the colour branch out and writes rgb_raw = 0.  Under the ReLU density such a point composites with
weight exactly +0, so every map must be BITWISE what the kernel renders with the skip switched off
(HipRenderer.set_empty_skip) -- in both forms of the kernel, on a ragged call (97 rays: the last pass is partial, and with
80 samples per ray waves straddle two rays) -- and the skip must not happen where somebody could tell: a raw output
(extras=True), density noise in the call's draws, the softplus density.

What skipped is read from the kernel's own counters on the render call's launches (HipRenderer.count_waves): they exist in
the on-chip form with one pose per call.  The other cases of the matrix -- the record form, a pose per ray, S = 32 (the
direct kernel pg_eval16.hip runs those rays) and fp16c (pg_evalc2.hip: the skip is not ported to it) -- compare the maps,
and their counters read zero passes or zero skipped waves; that the RAYS of the test have empty and non-empty 32-sample
groups side by side is checked on the CPU with the oracle."""
import numpy as np
import pytest
import torch

from bench import full_frame_rays
from oracle import anerf_oracle as orc
from posegen_amd import surreal_config, synthetic as syn
from tests.helpers import oracle_cfg, torch_weights

N_RAYS = 97
MAPS = ("rgb_map", "disp_map", "acc_map", "rgb0", "disp0", "acc0")
SEED = 0


def _rays(device):
    """97 consecutive rays through the body of the 64 x 64 all-hit frame (cylinder radius 2.5 around the pose)."""
    rb, skts, cyl, *_ = full_frame_rays(64, 64, device)
    first = (64 * 64 - N_RAYS) // 2
    return rb[first:first + N_RAYS].contiguous(), skts, cyl


def test_rays_have_empty_and_live_groups_on_the_oracle():
    """fp32 oracle: of the groups of 32 consecutive samples of the test's rays some are all sigma <= 0 and some are not, in
    the coarse and in the fine launch -- so both branches of the kernel run in one launch."""
    cfg = surreal_config()
    wc, wf, tv, td = syn.make_model(cfg, SEED)
    rb, skts, cyl = _rays("cpu")
    with torch.no_grad():
        out = orc.render_rays(rb, skts, cyl, oracle_cfg(cfg, tv, td), torch_weights(wc), torch_weights(wf), 64, 16,
                              return_extras=True)
    for k in ("raw_coarse", "raw_fine"):
        sg = out["extras"][k][..., 3].reshape(-1)
        groups = sg[:sg.numel() // 32 * 32].reshape(-1, 32) <= 0
        share = float(groups.all(1).float().mean())
        assert 0.05 < share < 0.95, (k, share)


@pytest.fixture(scope="module")
def caster():
    from posegen_amd.raycaster import HipRayCaster
    cfg = surreal_config()
    c = HipRayCaster.from_weights(cfg, *syn.make_model(cfg, SEED), device="cuda:0", precision="bf16")
    yield c
    c.renderer.close()


def _on_off(r, call):
    """(result with the skip on, its counters, result with the skip off, its counters) of the same call"""
    r.count_waves(True)
    try:
        r.set_empty_skip(True)
        on = call()
        torch.cuda.synchronize()
        cnt_on = r.read_wave_counts()
        r.set_empty_skip(False)
        off = call()
        torch.cuda.synchronize()
        cnt_off = r.read_wave_counts()
    finally:
        r.set_empty_skip(True)
        r.count_waves(False)
    return on, cnt_on, off, cnt_off


def _same_maps(on, off, what):
    for k in MAPS:
        if k in off:
            assert torch.equal(on[k], off[k]), f"{what}: {k} differs between skip on and skip off"
    assert bool(torch.isfinite(off["rgb_map"]).all()), what


CASES = [(prec, form, S, N, "one") for prec in ("bf16", "fp16", "fp16c") for form in ("records", "always") for S, N in ((64, 16), (32, 0))]
CASES.append(("bf16", "always", 64, 16, "per_ray"))


@pytest.mark.gpu
@pytest.mark.parametrize("prec,form,S,N,pose", CASES, ids=[f"{p}-{'onchip' if f == 'always' else f}-{S}+{N}-{po}" for p, f, S, N, po in CASES])
def test_maps_are_bitwise_those_without_the_skip(caster, prec, form, S, N, pose):
    r = caster.renderer
    rb, skts, cyl = _rays(r.device)
    if pose == "per_ray":
        skts = skts.reshape(1, 24, 4, 4).repeat(N_RAYS, 1, 1, 1).contiguous()
    r.set_precision(prec)
    r.set_onchip(form)
    try:
        on, cnt_on, off, cnt_off = _on_off(r, lambda: r.render_rays(rb, skts, cyl, n_samples=S, n_importance=N, want_alpha=False))
    finally:
        r.set_onchip("auto")
        r.set_precision("bf16")
    what = f"{prec} {form} {S}+{N} {pose}"
    _same_maps(on, off, what)
    assert float(off["acc_map"].max()) > 0.5, what           # the rays do cross the body
    counted = prec in ("bf16", "fp16") and form == "always" and S >= 64 and pose == "one"
    if counted:
        assert cnt_on["passes"] == cnt_off["passes"] == -(-N_RAYS * S // 256) + (-(-N_RAYS * (S + N) // 256) if N else 0), (what, cnt_on)
        # the call really skips, and not everything: both branches ran in these launches
        assert 0.0 < cnt_on["skipped_waves_frac"] < 1.0, (what, cnt_on)
        assert cnt_on["skipped_waves_frac"] == cnt_on["empty_waves_frac"] == cnt_off["empty_waves_frac"], (what, cnt_on, cnt_off)
        assert cnt_off["skipped_waves_frac"] == 0.0, (what, cnt_off)
    else:
        # not a launch the counters cover (record form, pose per ray, the direct kernel below 64 samples), or a kernel
        # without the skip (fp16c: pg_evalc2.hip)
        assert cnt_on["skipped_waves_frac"] == 0.0 and cnt_off["skipped_waves_frac"] == 0.0, (what, cnt_on, cnt_off)


@pytest.mark.gpu
@pytest.mark.parametrize("prec", ["bf16", "fp16"])
def test_raw_outputs_refuse_the_skip(caster, prec):
    """extras=True hands raw_coarse / raw_fine out: every wave computes its colours, the raw is bitwise the switch-off call's."""
    r = caster.renderer
    rb, skts, cyl = _rays(r.device)
    r.set_precision(prec)
    r.set_onchip("always")
    try:
        on, cnt_on, off, cnt_off = _on_off(r, lambda: r.render_rays(rb, skts, cyl, n_samples=64, n_importance=16, want_alpha=False, extras=True))
    finally:
        r.set_onchip("auto")
        r.set_precision("bf16")
    for k in ("raw_coarse", "raw_fine"):
        assert torch.equal(on["extras"][k], off["extras"][k]), k
    _same_maps(on, off, "extras")
    assert cnt_on["passes"] > 0 and cnt_on["empty_waves_frac"] > 0.0, cnt_on          # empty waves there were ...
    assert cnt_on["skipped_waves_frac"] == 0.0 and cnt_off["skipped_waves_frac"] == 0.0, (cnt_on, cnt_off)      # ... none skipped
    # their colours are the network's, not the zeros a skipping wave writes
    sg = on["extras"]["raw_coarse"][..., 3]
    assert bool((on["extras"]["raw_coarse"][..., :3][sg <= 0] != 0).any())


@pytest.mark.gpu
def test_density_noise_refuses_the_skip(caster):
    """noise0 / noise1 in the call's draws: relu(sigma + noise) can be positive where sigma <= 0."""
    r = caster.renderer
    rb, skts, cyl = _rays(r.device)
    g = torch.Generator().manual_seed(3)
    draws = {"noise0": torch.randn(N_RAYS, 64, generator=g), "noise1": torch.randn(N_RAYS, 80, generator=g)}
    r.set_onchip("always")
    try:
        on, cnt_on, off, cnt_off = _on_off(r, lambda: r.render_rays(rb, skts, cyl, n_samples=64, n_importance=16, want_alpha=False, draws=draws))
        # one of the two alone refuses its own launch only
        half, cnt_half, _, _ = _on_off(r, lambda: r.render_rays(rb, skts, cyl, n_samples=64, n_importance=16, want_alpha=False,
                                                                 draws={"noise0": draws["noise0"]}))
    finally:
        r.set_onchip("auto")
    _same_maps(on, off, "noise")
    assert cnt_on["passes"] > 0 and cnt_on["empty_waves_frac"] > 0.0 and cnt_on["skipped_waves_frac"] == 0.0, cnt_on
    assert 0.0 < cnt_half["skipped_waves_frac"] < cnt_half["empty_waves_frac"], cnt_half


@pytest.mark.gpu
def test_softplus_density_refuses_the_skip():
    """softplus(sigma - shift) is positive everywhere: no point is empty (the config of the rays_softplus fixture)."""
    from posegen_amd.raycaster import HipRayCaster
    cfg = surreal_config(density_type="softplus", softplus_shift=1.0)
    c = HipRayCaster.from_weights(cfg, *syn.make_model(cfg, SEED), device="cuda:0", precision="bf16")
    r = c.renderer
    try:
        rb, skts, cyl = _rays(r.device)
        r.set_onchip("always")
        on, cnt_on, off, cnt_off = _on_off(r, lambda: r.render_rays(rb, skts, cyl, n_samples=64, n_importance=16, want_alpha=False, extras=True))
        _, cnt_plain, _, _ = _on_off(r, lambda: r.render_rays(rb, skts, cyl, n_samples=64, n_importance=16, want_alpha=False))
        stage = r.limb_skip_stats(0, rb, on["extras"]["z_coarse"], skts)
    finally:
        r.close()
    _same_maps(on, off, "softplus")
    for cnt in (cnt_on, cnt_plain, stage):
        assert cnt["passes"] > 0 and cnt["empty_waves_frac"] > 0.0 and cnt["skipped_waves_frac"] == 0.0, cnt


@pytest.mark.gpu
@pytest.mark.parametrize("form", ["records", "always"])
def test_all_empty_call(form):
    """alpha_linear = 0 x h - 1 in both nets: sigma = -1 at every point, every wave skips, acc_map is exactly 0."""
    from posegen_amd.raycaster import HipRayCaster
    cfg = surreal_config()
    wc, wf, tv, td = syn.make_model(cfg, SEED)
    for w in (wc, wf):
        w["alpha_linear.weight"] = np.zeros_like(w["alpha_linear.weight"])
        w["alpha_linear.bias"] = np.full_like(w["alpha_linear.bias"], -1.0)
    c = HipRayCaster.from_weights(cfg, wc, wf, tv, td, device="cuda:0", precision="bf16")
    r = c.renderer
    try:
        rb, skts, cyl = _rays(r.device)
        r.set_onchip(form)
        on, cnt_on, off, cnt_off = _on_off(r, lambda: r.render_rays(rb, skts, cyl, n_samples=64, n_importance=16, want_alpha=False))
    finally:
        r.close()
    _same_maps(on, off, "all empty")
    for k in ("acc_map", "acc0", "rgb_map", "rgb0"):
        assert bool((on[k] == 0).all()), k
    if form == "always":
        assert cnt_on["passes"] > 0 and cnt_on["skipped_waves_frac"] == 1.0 and cnt_off["skipped_waves_frac"] == 0.0, (cnt_on, cnt_off)
