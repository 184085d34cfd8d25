"""The HMR regression head on the device at the specs that include/posegen_regressor.h allows and the toy and the shipped spec do
not reach (`hmr_ref.edge_specs`): empty decoders, every K one short of, at, one past and at twice the 64-column step, the limits and
the minimum; mask bytes other than 0 and 1, a weight-gradient fold of 65 chunks, the backward's workspace across sizes and specs on
one handle, a NaN cotangent row, and the module's plumbing (empty Linears, unused outputs, frozen parameters, foreign dtypes and
layouts of xf and the masks, n_iter by argument, a partly given init, no_grad, p = 0).

The comparisons are those of tests/test_gpu_hmr.py (tests/hmr_checks.py: each product against float64 on the device's own operands
under (K + 2) u (|h| |W|^T + |b|), the chain of the backward under the bounds carried to first order), which tests/test_hmr_ref.py
confronts with honest float32 and with planted errors on the CPU at the same specs.  Plumbing is compared by bytes."""
import functools

import numpy as np
import pytest
import torch

from posegen_amd import _ffi
from tests import hmr_checks as chk
from tests import hmr_ref as ref
from tests.frame_metrics_gpu import DEV, renderer  # noqa: F401 (renderer: a fixture)
from tests.test_gpu_hmr import (EVERY, GRADS, SENT, Head, _all_results, _cotangents, _end_to_end, _inputs, _module, _one_row_products, _same,
                                _weight_gradients_on_own_operands)

pytestmark = pytest.mark.gpu
SPECS = ref.edge_specs()
OUTS = ("rotmat", "shape", "cam")


def _same_results(a, b, keys=None):
    """two result dicts byte for byte (an output without elements is None in both)"""
    assert set(a) == set(b)
    for k in (a if keys is None else keys):
        assert (a[k] is None and b[k] is None) or _same(a[k], b[k]), k


# ---- layer-local checks -------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=2)
def _state_dict(name, seed=51):
    return ref.make_state_dict(SPECS[name], seed)


@pytest.mark.parametrize("mode", ("train", "eval"))
@pytest.mark.parametrize("name,B", [(name, B) for name in SPECS for B in ((17,) if name == "limits" else (1, 17, 65))])
def test_layer_local_checks_on_every_named_spec(renderer, name, B, mode):
    """training mode with masks and the shared init; eval mode with an init per row"""
    spec = SPECS[name]
    sd = _state_dict(name)
    xf, masks, _ = _inputs(spec, B, 52)
    if mode == "train":
        cpu = ref.forward(ref.params_of(sd), xf, ref.init_of(sd), spec, masks)
        assert np.mean(chk.well_conditioned(spec, cpu["s"][-1])) >= 0.9       # on the CPU restatement, before the device is looked at
        run = Head(renderer, spec, sd, xf, masks, offset=B % 4)
    else:
        run = Head(renderer, spec, sd, xf, None, init=_inputs(spec, B, 55, per_row=True)[2], offset=B % 4)
    run.forward()
    _, well = chk.check_forward(run, f"{name} {mode}")
    assert np.mean(well) >= 0.9
    assert (run.out["shape"] is None) == (spec.n_shape == 0) and (run.out["cam"] is None) == (spec.n_cam == 0)
    got = chk.check_backward(run, _cotangents(spec, B, 54 if mode == "train" else 56), f"{name} {mode}")
    assert set(got) == {k for k in EVERY if k not in GRADS or run.P[k].size}


@pytest.mark.parametrize("name", ("minimum", "step64", "step65"))
def test_every_backward_product_on_the_devices_own_operands_at_one_row_and_one_round(renderer, name):
    spec = SPECS[name].with_iter(1)
    # a seed whose masks keep at least one column of each Dropout (at H = 1 that is: both elements), so that no product is all zeros
    seed = next(s for s in range(720, 800) if ref.make_masks(spec, 1, s + 1).any(axis=(2, 3)).all())
    assert seed == 720 or name == "minimum"
    _one_row_products(renderer, spec, f"one row {name}", seed)


@pytest.mark.parametrize("name", ("minimum", "step64", "step65"))
def test_weight_gradients_on_the_devices_own_operands_at_one_round(renderer, name):
    _weight_gradients_on_own_operands(renderer, SPECS[name].with_iter(1), 70)


# ---- empty decoders through the raw API ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ("no_shape", "no_cam", "pose_only"))
def test_an_absent_decoders_pointers_may_be_null_or_anything(renderer, name):
    """NULL, or pointers at sentinels (parameters, outputs, cotangents and gradients of the absent decoders): the same bytes, and the
    sentinels intact (`Head` asserts that after each call)"""
    spec, B = SPECS[name], 17
    sd = ref.make_state_dict(spec, 51)
    xf, masks, _ = _inputs(spec, B, 52)
    cots = _cotangents(spec, B, 54)
    null = _all_results(Head(renderer, spec, sd, xf, masks), cots)
    run = Head(renderer, spec, sd, xf, masks, dummies=True)
    assert sum(getattr(run.tab, k) == run.dummy for k in GRADS) == 2 * ((spec.n_shape == 0) + (spec.n_cam == 0))
    _same_results(null, _all_results(run, cots))
    assert null["tape"].size and len(null) == 4 + sum(1 for k in EVERY if k not in GRADS or run.P[k].size)


def test_a_cotangent_of_an_absent_output_alone_is_no_cotangent(renderer):
    spec, B = SPECS["pose_only"], 5
    sd = ref.make_state_dict(spec, 51)
    xf, masks, _ = _inputs(spec, B, 52)
    run = Head(renderer, spec, sd, xf, masks, dummies=True)
    run.forward()
    d_rotmat, d_shape, d_cam = _cotangents(spec, B, 54)
    assert d_shape.shape == (B, 0) and d_cam.shape == (B, 0)
    for cots in ((None, d_shape, None), (None, None, d_cam), (None, d_shape, d_cam)):
        with pytest.raises(_ffi.PgError) as info:                              # (non-null pointers, at the sentinels)
            run.backward(*cots)
        assert info.value.code == _ffi.PG_EINVAL and "no cotangent at all" in str(info.value)
        torch.cuda.synchronize()
        assert len(run.held) == len(EVERY) - 4 and all(bool((full == SENT).all()) for full, _ in run.held.values())
    alone = run.backward(d_rotmat, None, None)
    _same_results(alone, run.backward(d_rotmat, d_shape, d_cam))
    assert np.any(alone["d_xf"] != 0.0)


def test_the_cotangent_pointer_of_an_absent_output_is_not_read(renderer):
    spec, B = SPECS["no_shape"], 17
    sd = ref.make_state_dict(spec, 51)
    xf, masks, _ = _inputs(spec, B, 52)
    d_rotmat, d_shape, d_cam = _cotangents(spec, B, 54)
    run = Head(renderer, spec, sd, xf, masks, dummies=True)
    run.forward()
    _same_results(run.backward(d_rotmat, None, d_cam), run.backward(d_rotmat, d_shape, d_cam))
    _same_results(run.backward(None, None, d_cam), run.backward(None, d_shape, d_cam))


# ---- mask bytes ---------------------------------------------------------------------------------------------------------------------------------
def test_any_non_zero_mask_byte_keeps(renderer):
    spec, B = ref.toy_spec(), 17
    sd = ref.make_state_dict(spec, 81)
    xf, masks, _ = _inputs(spec, B, 1000)
    cots = _cotangents(spec, B, 1001)
    other = np.where(masks != 0, np.random.RandomState(1002).choice(np.array([2, 128, 255], np.uint8), size=masks.shape), 0).astype(np.uint8)
    assert set(np.unique(other)) == {0, 2, 128, 255} and np.array_equal(other != 0, masks != 0)
    _same_results(_all_results(Head(renderer, spec, sd, xf, masks, offset=1), cots), _all_results(Head(renderer, spec, sd, xf, other, offset=1), cots))


# ---- a longer fold ------------------------------------------------------------------------------------------------------------------------------
def test_weight_gradients_over_65_chunks_of_rows(renderer):
    """B = 4099 at one round: 64 whole chunks of 64 rows and three rows.  (R + 2) u |A|^T |B|, the bound for any order, is 4101 u here
    and would not notice the last three rows missing; the documented order -- chunks of 64, partials added in chunk order -- gives
    (64 + 2 + 65) u (hmr_ref.chunk_fold_terms), and that is what the weight products are held to.  A bias gradient is a double sum of
    R = 4099 terms, which in any order loses at most R 2^-53 of the magnitudes before its one rounding (hmr_ref.double_sum_term): 16
    times the constant that the short sums are held to."""
    spec, B = ref.toy_spec(1), 4099
    sd = ref.make_state_dict(spec, 82)
    xf, masks, _ = _inputs(spec, B, 1010)
    run = Head(renderer, spec, sd, xf, masks, offset=3)
    run.forward()
    assert ref.double_sum_term(B) > ref.DOUBLE_SUM
    assert ref.chunk_fold_terms(1, B) == 64 + 2 + 65
    got = chk.check_backward(run, _cotangents(spec, B, 1011), "toy 65 chunks", want=GRADS, double_sum=ref.double_sum_term(B),
                             row_terms=lambda rounds: ref.chunk_fold_terms(rounds, B))
    assert set(got) == set(GRADS)


# ---- the workspace ------------------------------------------------------------------------------------------------------------------------------
def test_the_workspace_across_sizes_and_specs_on_one_handle():
    """a handle of its own, so that the workspace starts empty: toy B = 5, then (nothing waited for in between) shipped B = 17, which
    grows it, toy B = 5 again and minimum B = 1 in the larger buffer; each equals the same call made alone after a synchronise"""
    from posegen_amd import surreal_config
    from posegen_amd.raycaster import HipRenderer
    r = HipRenderer(surreal_config(), device=DEV)
    try:
        runs, cots = [], []
        for i, (spec, B) in enumerate(((ref.toy_spec(), 5), (ref.shipped_spec(), 17), (SPECS["minimum"], 1))):
            xf, masks, _ = _inputs(spec, B, 1020 + 2 * i)
            runs.append(Head(r, spec, ref.make_state_dict(spec, 83 + i), xf, masks))
            runs[-1].forward()
            cots.append(_cotangents(spec, B, 1030 + i))
        toy, shipped, minimum = runs
        first = toy.backward(*cots[0])
        chain = [(shipped, cots[1]), (toy, cots[0]), (minimum, cots[2])]
        launched = [run.launch_backward(*c) for run, c in chain]
        torch.cuda.synchronize()
        chained = [run.collect_backward(l) for (run, _), l in zip(chain, launched)]
        for (run, c), got in zip(chain, chained):
            _same_results(run.backward(*c), got)
        _same_results(first, chained[1])
        assert len(chained[0]) == len(EVERY) and len(chained[2]) == len(EVERY) - 4
    finally:
        r.close()


# ---- a NaN cotangent ----------------------------------------------------------------------------------------------------------------------------
def test_a_nan_cotangent_row_stays_in_its_row(renderer):
    spec, B = ref.toy_spec(), 37
    sd = ref.make_state_dict(spec, 86)
    xf, masks, _ = _inputs(spec, B, 1040)
    cots = _cotangents(spec, B, 1041)
    run = Head(renderer, spec, sd, xf, masks)
    run.forward()
    clean = run.backward(*cots, want=("d_xf", "d_init"))
    bad = cots[0].copy()
    bad[20, 1, 2, 0] = np.nan
    dirty = run.backward(bad, cots[1], cots[2], want=("d_xf", "d_init"))
    keep = np.arange(B) != 20
    for k in ("d_xf", "d_init"):
        assert _same(clean[k][keep], dirty[k][keep]) and np.all(np.isnan(dirty[k][20])) and not np.isnan(clean[k]).any(), k


# ---- the module ---------------------------------------------------------------------------------------------------------------------------------
class _Case:
    """one toy setting and what the raw calls give for it"""

    def __init__(self, renderer, spec=None, B=17, seed=1100, sd_seed=87):
        self.r, self.spec, self.B = renderer, ref.toy_spec() if spec is None else spec, B
        self.sd = ref.make_state_dict(self.spec, sd_seed)
        self.xf, self.masks, _ = _inputs(self.spec, B, seed)
        self.cots = _cotangents(self.spec, B, seed + 2)
        self.raw = _all_results(Head(renderer, self.spec, self.sd, self.xf, self.masks), self.cots)

    def module(self):
        return _module(self.spec, self.sd, self.r, DEV).train()

    def run(self, head, xf=None, masks="given", cots="given", **kw):
        """forward and backward through the module -> results under the raw names (a gradient that autograd left out is absent)"""
        xt = torch.tensor(self.xf, device=DEV, requires_grad=True) if xf is None else xf
        if isinstance(masks, str):
            masks = torch.from_numpy(self.masks)
        outs = head(xt, masks=masks, **kw)
        torch.autograd.backward(outs, [torch.tensor(c, device=DEV) for c in (self.cots if isinstance(cots, str) else cots)])
        return self.results(head, outs, xt)

    def results(self, head, outs, xt=None):
        res = {k: (o.detach().cpu().numpy() if o.numel() else None) for k, o in zip(OUTS, outs)}
        if xt is not None and xt.is_leaf and xt.grad is not None:
            res["d_xf"] = xt.grad.cpu().numpy()
        for lin in ref.LINEARS:
            for leaf, g in (("w", getattr(head, lin).weight.grad), ("b", getattr(head, lin).bias.grad)):
                if g is not None and g.numel():
                    res[f"{lin}_{leaf}"] = g.cpu().numpy()
        return res

    def equals_raw(self, res, raw=None, without=()):
        raw = self.raw if raw is None else raw
        want = {k for k in raw if k not in ("tape", "d_init") and k not in without}
        assert set(res) == want, sorted(set(res) ^ want)
        for k in want:
            assert (res[k] is None and raw[k] is None) or _same(res[k], raw[k]), k


@pytest.fixture(scope="module")
def toy(renderer):
    return _Case(renderer)


@pytest.mark.parametrize("name", ("pose_only", "no_shape"))
def test_a_module_with_empty_decoders(renderer, name):
    case = _Case(renderer, SPECS[name], seed=1110)                             # (`_module` loads the state dict with strict=True)
    head = case.module()
    assert tuple(head.decshape.weight.shape) == (0, case.spec.n_hidden) and set(head.state_dict()) == set(case.sd)
    xt = torch.tensor(case.xf, device=DEV, requires_grad=True)
    outs = head(xt, masks=torch.from_numpy(case.masks))
    assert tuple(outs[1].shape) == (case.B, 0) and tuple(outs[2].shape) == (case.B, case.spec.n_cam) and outs[1].dtype == torch.float32
    torch.autograd.backward(outs, [torch.tensor(c, device=DEV) for c in case.cots])
    case.equals_raw(case.results(head, outs, xt))
    empty = [head.decshape] + ([head.deccam] if case.spec.n_cam == 0 else [])
    for lin in empty:
        assert lin.weight.grad is not None and tuple(lin.weight.grad.shape) == (0, case.spec.n_hidden) and tuple(lin.bias.grad.shape) == (0,)
    torch.optim.Adam(head.parameters(), lr=1e-3).step()


def test_a_loss_on_one_output_alone(toy):
    head = toy.module()
    xt = torch.tensor(toy.xf, device=DEV, requires_grad=True)
    outs = head(xt, masks=torch.from_numpy(toy.masks))
    w = torch.tensor(toy.cots[2], device=DEV)
    (outs[2] * w).sum().backward()
    run = Head(toy.r, toy.spec, toy.sd, toy.xf, toy.masks)
    run.forward()
    toy.equals_raw(toy.results(head, outs, xt), dict(toy.raw, **run.backward(None, None, toy.cots[2])))
    # pred_rotmat.sum(): the cotangent is one scalar expanded, with strides of zero
    head = toy.module()
    xt = torch.tensor(toy.xf, device=DEV, requires_grad=True)
    outs = head(xt, masks=torch.from_numpy(toy.masks))
    outs[0].sum().backward()
    ones = np.ones((toy.B, toy.spec.n_joints, 3, 3), np.float32)
    toy.equals_raw(toy.results(head, outs, xt), dict(toy.raw, **run.backward(ones, None, None)))


def test_frozen_parameters_get_no_gradient_and_change_no_other(toy):
    head = toy.module()
    for lin in (head.fc1, head.decshape):
        lin.requires_grad_(False)
    res = toy.run(head)
    frozen = ("fc1_w", "fc1_b", "decshape_w", "decshape_b")
    toy.equals_raw(res, without=frozen)
    assert all(p.grad is None for lin in (head.fc1, head.decshape) for p in lin.parameters())
    # and xf without a gradient
    res = toy.run(toy.module(), xf=torch.tensor(toy.xf, device=DEV))
    toy.equals_raw(res, without=("d_xf",))


def test_xf_in_float64_and_as_a_strided_slice(toy):
    x64 = torch.tensor(toy.xf.astype(np.float64), device=DEV, requires_grad=True)
    res = toy.run(toy.module(), xf=x64)
    assert x64.grad.dtype == torch.float64 and _same(res.pop("d_xf").astype(np.float32), toy.raw["d_xf"])
    toy.equals_raw(res, without=("d_xf",))
    wide = np.zeros((toy.B, 2 * toy.spec.n_feat), np.float32)
    wide[:, ::2], wide[:, 1::2] = toy.xf, 7.0
    big = torch.tensor(wide, device=DEV, requires_grad=True)
    view = big[:, ::2]
    assert not view.is_contiguous()
    res = toy.run(toy.module(), xf=view)
    assert "d_xf" not in res and tuple(big.grad.shape) == tuple(big.shape) and big.grad.dtype == torch.float32
    g = big.grad.cpu().numpy()
    assert _same(g[:, ::2], toy.raw["d_xf"]) and np.all(g[:, 1::2] == 0.0)
    toy.equals_raw(res, without=("d_xf",))


@pytest.mark.parametrize("kind", ("bool", "float32", "cpu", "numpy"))
def test_masks_of_any_dtype_and_on_the_host(toy, kind):
    m = torch.from_numpy(toy.masks)
    masks = {"bool": m.to(DEV).bool(), "float32": m.to(DEV).float() * 0.25, "cpu": m.clone(), "numpy": toy.masks}[kind]
    toy.equals_raw(toy.run(toy.module(), masks=masks))


def test_explicit_masks_are_applied_in_eval_mode(toy):
    head = toy.module().eval()
    toy.equals_raw(toy.run(head))
    none = toy.run(toy.module().eval(), masks=None)
    assert not _same(none["rotmat"], toy.raw["rotmat"])


@pytest.mark.parametrize("n_iter", (1, 8))
def test_n_iter_through_the_call(toy, n_iter):
    spec = toy.spec.with_iter(n_iter)
    masks = ref.make_masks(spec, toy.B, 1120 + n_iter)
    raw = _all_results(Head(toy.r, spec, toy.sd, toy.xf, masks), toy.cots)
    toy.equals_raw(toy.run(toy.module(), masks=torch.from_numpy(masks), n_iter=n_iter), raw)
    assert not _same(raw["rotmat"], toy.raw["rotmat"])


def test_an_init_given_for_the_camera_alone(toy):
    a, b = toy.spec.n_pose, toy.spec.n_pose + toy.spec.n_shape
    cam = np.random.RandomState(1130).standard_normal((toy.B, toy.spec.n_cam)).astype(np.float32)
    init = np.tile(ref.init_of(toy.sd)[None], (toy.B, 1)).astype(np.float32)
    init[:, b:] = cam
    raw = _all_results(Head(toy.r, toy.spec, toy.sd, toy.xf, toy.masks, init=init), toy.cots)
    ic = torch.tensor(cam, device=DEV, requires_grad=True)
    toy.equals_raw(toy.run(toy.module(), init_cam=ic), raw)
    assert _same(ic.grad.cpu().numpy(), raw["d_init"][:, b:]) and not _same(raw["rotmat"], toy.raw["rotmat"])


def test_no_grad_and_eval_mode(toy):
    ev = Head(toy.r, toy.spec, toy.sd, toy.xf)
    ev.forward()
    head = toy.module().eval()
    with torch.no_grad():
        outs = head(torch.tensor(toy.xf, device=DEV, requires_grad=True))
    assert not any(o.requires_grad for o in outs)
    for k, o in zip(OUTS, outs):
        assert _same(o.cpu().numpy(), ev.out[k]), k
    with torch.no_grad():                                                      # training mode under no_grad: the given masks still apply
        outs = toy.module()(torch.tensor(toy.xf, device=DEV), masks=torch.from_numpy(toy.masks))
    for k, o in zip(OUTS, outs):
        assert _same(o.cpu().numpy(), toy.raw[k]) and not o.requires_grad, k


def test_p_zero_in_training_mode_is_eval_mode(toy):
    results = []
    for training in (True, False):
        head = toy.module().train(training)
        head.drop1.p = 0.0
        results.append(toy.run(head, masks=None))
    _same_results(*results)
    assert not _same(results[0]["rotmat"], toy.raw["rotmat"])


# ---- end to end ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,at_least", [("step64", 5), ("step65", 5), ("limits", 9)])
def test_the_module_against_stock_forward_in_float32_on_the_cpu_at_the_new_widths(renderer, name, at_least):
    _end_to_end(renderer, SPECS[name], name, 17, False, at_least)
