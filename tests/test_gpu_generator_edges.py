"""The pose generator's backward layer by layer, at the documented limits and on degenerate columns (include/posegen_generator.h,
posegen_amd/csrc/pg_gen.hip, posegen_amd/generators.py).

Every gradient tensor -- each layer's dW, db, d_gamma, d_beta, and the head's d_w2, d_b2, d_h -- is compared with the float64 backward
from the device's own tape and masks under the elementwise bound that tests/generator_ref.py carries down the chain
(trunk_backward_with_bound, ba_head_backward_with_bound: the recurrences are in their docstrings; tests/test_generator_ref.py shows on
the CPU that honest float32 stays inside the bound and that planted errors leave it).  |dev - f64| <= bound is compared, never
divided; the worst ratios are printed (DESIGN.md 2.17 records them).  There is no size cut-off.  The cases are built by
generator_ref.edge_case, so that the CPU file judges the bound on the very inputs that run here.

The carried bound loosens with depth, so the nine-layer spec also meets tests/test_gpu_generator.py's end-to-end criterion (<= 4 x
torch float32 on the CPU per tensor of 256 elements and more) at B >= 17, the batches that criterion is defined for.

Row limit: B = PG_GEN_MAX_ROWS = 2^20 on one three-wide stem with a head of one joint, everything a few MB."""
import numpy as np
import pytest
import torch

from posegen_amd import _ffi
from tests import generator_ref as ref
from tests.frame_metrics_gpu import DEV, renderer  # noqa: F401 (renderer: a fixture)
from tests.test_gpu_generator import Trunks, _check_head, _check_layers, _end_to_end, _modules, _noise, _note, _rt_check, _same, _ulp32

pytestmark = pytest.mark.gpu
KEYS = ("w", "b", "gamma", "beta")


def _inside(tag, got, want, bound, where):
    """|got - want| <= bound on every entry; where the reference is NaN the device must be, and nowhere else"""
    got = np.asarray(got, np.float64).reshape(want.shape)
    nan = np.isnan(want)
    assert np.array_equal(np.isnan(got), nan), (tag, where, "the NaN pattern")
    err, bound = np.abs(got - want)[~nan], bound[~nan]
    if err.size:
        _note(tag, err, bound)
    assert np.all(err <= bound), (tag, where, float(np.max(err - bound)))


def _device_tape(run, t, noise_t):
    """(tape, masks) of trunk t as the device has them: its Z, mean, var, scale, shift read back, fmaf(Z, scale, shift) > 0"""
    tape = ref.rebuilt_tape(noise_t, [run.layer(t, l) for l in range(run.spec.layers(t))], ref.held(run.spec)[0])
    return tape, [tp["y"] > 0 for tp in tape]


def _bounded_backward(run, params, noise, cots, tag):
    """a trunk backward at the cotangents `cots` (arrays), every gradient of every layer against the carried bound
    -> the device's gradients, per trunk (tape, masks, float64 gradients, bounds)"""
    slope, eps = ref.held(run.spec)
    got = run.backward(cots)
    per_trunk = []
    for t, layers in enumerate(params):
        if cots[t] is None:
            per_trunk.append(None)
            continue
        tape, masks = _device_tape(run, t, noise[t])
        g64, bound = ref.trunk_backward_with_bound(layers, tape, masks, cots[t], slope, eps)
        for l in range(len(layers)):
            for i, k in enumerate(KEYS):
                _inside(f"{tag} d_{k}", got[(t, l, k)], g64[l][i], bound[l][i], (run.B, t, l, k))
        per_trunk.append((tape, masks, g64, bound))
    return got, per_trunk


def _bounded_head_backward(run, t, w2, y, seed, tag):
    d_pose = np.random.RandomState(seed).standard_normal((run.B, run.J, 3)).astype(np.float32)
    got = run.head_backward(t, d_pose)
    g64, bound = ref.ba_head_backward_with_bound(run.h(t, run.spec.layers(t) - 1), w2, y, d_pose)
    for k, a, b, e in zip(("d_w2", "d_b2", "d_h"), got, g64, bound):
        _inside(f"{tag} {k}", a, b, e, (run.B, run.J, k))
    return got


# ---- (a) the backward, layer by layer ----------------------------------------------------------------------------------------------------
HEAD_OF = {"toy": (0, 5), "deep": (3, 5), "flat": (2, 5), "wide": (0, 64)}             # the forward's head check: (trunk, J)


@pytest.mark.parametrize("name,B", [(name, B) for name, batches in ref.EDGE_BATCHES.items() for B in batches])
def test_every_gradient_of_every_layer_is_inside_the_carried_bound(renderer, name, B):
    spec, params, noise, cots = ref.edge_case(name, B)
    run = Trunks(renderer, spec, params, noise, B)
    _check_layers(run, params, noise, f"{name} train")
    _check_head(run, *HEAD_OF[name], 810, name)
    _bounded_backward(run, params, noise, cots, name)


@pytest.mark.parametrize("name,B,J", ref.HEAD_CASES)
def test_the_heads_gradients_are_inside_their_bound(renderer, name, B, J):
    spec, params, noise, _ = ref.edge_case(name, B)
    run = Trunks(renderer, spec, params, [noise[0]] + [None] * (len(noise) - 1), B)
    w2, _, y, _ = _check_head(run, 0, J, 820 + J, f"{name} J={J}")
    _bounded_head_backward(run, 0, w2, y, 830 + J, f"{name} head")


@pytest.mark.parametrize("B", (17, 65, 257))
def test_the_nine_layer_spec_end_to_end_against_torch_float32(renderer, B):
    spec = ref.deep_spec()
    for t, J in ((0, 64), (1, 5), (2, 24), (3, 5)):                            # (width 1: the head's d_w2 alone has 256 entries)
        _end_to_end(renderer, spec, t, B, J, 840 + 3 * t, "deep")


# ---- (b) the row limit ---------------------------------------------------------------------------------------------------------------------
def test_the_row_limit(renderer):
    B = _ffi.PG_GEN_MAX_ROWS
    spec, params, noise, cots = ref.edge_case("rows")
    assert noise[0].shape == (B, 2)
    run = Trunks(renderer, spec, params, noise, B)
    _check_layers(run, params, noise, "rows train")
    w2, _, y, _ = _check_head(run, 0, 1, 850, "rows")
    _bounded_head_backward(run, 0, w2, y, 851, "rows head")
    _bounded_backward(run, params, noise, cots, "rows")


# ---- (c) degenerate columns ----------------------------------------------------------------------------------------------------------------
def _degenerate(renderer, name):
    spec, params, noise, cots = ref.edge_case(name)
    run = Trunks(renderer, spec, params, noise, noise[0].shape[0])
    _check_layers(run, params, noise, name)
    got, per_trunk = _bounded_backward(run, params, noise, cots, name)
    assert all(np.all(np.isfinite(g)) for g in got.values())
    return spec, params, run, got, per_trunk


@pytest.mark.parametrize("l", (0, 1))
def test_a_zeroed_weight_row_gives_a_zero_variance_column(renderer, l):
    spec, params, run, got, per_trunk = _degenerate(renderer, "zero row stem" if l == 0 else "zero row middle")
    m, eps = float(np.float32(spec.momentum)), ref.held(spec)[1]
    for t, (_, width, _) in enumerate(spec.trunks):
        col, layer, d = ref.zero_row_column(width, l), params[t][l], run.layer(t, l)
        assert d["var"][col] == 0.0 and d["mean"][col] == np.float64(layer["b"][col])
        scale64 = np.float64(layer["gamma"][col]) / np.sqrt(eps)
        assert abs(d["scale"][col] - scale64) <= 2 * _ulp32(scale64)
        rv64 = (1 - m) * np.float64(layer["rv"][col])
        assert abs(np.float64(run.running(t, l)[1][col]) - rv64) <= 2 * _ulp32(rv64)
        _, _, g64, bound = per_trunk[t]
        assert got[(t, l, "gamma")][col] == 0.0 and g64[l][2][col] == 0.0 and bound[l][2][col] == 0.0


def test_gamma_zero_columns_with_beta_at_and_off_zero(renderer):
    spec, params, run, got, per_trunk = _degenerate(renderer, "gamma 0")
    slope = np.float32(spec.slope)
    betas = np.asarray(ref.GAMMA0_BETAS, np.float32)
    want = np.where(betas > 0, betas, betas * slope)                           # lrelu in float32, as the kernels form it
    for t, (_, width, _) in enumerate(spec.trunks):
        cols, top = list(ref.gamma0_columns(width)), spec.layers(t) - 1
        d = run.layer(t, top)
        assert np.all(d["scale"][cols] == 0.0) and np.all(d["shift"][cols] == betas.astype(np.float64))
        # the activation itself: a head whose four rows each select one of the columns reads it out exactly (1 h + zeros)
        w2 = np.zeros((4, width), np.float32)
        w2[np.arange(4), cols] = 1.0
        y, _ = run.head(t, 1, w2, np.zeros(4, np.float32))
        assert np.all(y == want[None, :]), t
        assert np.all(got[(t, top, "w")][cols] == 0.0) and np.all(got[(t, top, "b")][cols] == 0.0)
        _, masks, _, _ = per_trunk[t]
        assert not masks[top][:, cols[:2]].any() and not masks[top][:, cols[3]].any() and masks[top][:, cols[2]].all()


def test_two_identical_rows_have_no_variance_anywhere(renderer):
    spec, params, run, got, _ = _degenerate(renderer, "twin rows")
    for t in range(len(spec.trunks)):
        assert np.all(run.layer(t, 0)["var"] == 0.0)
    assert np.all(np.isfinite(run.host[0])) and np.all(np.isfinite(run.host[1]))


@pytest.mark.parametrize("name", [n for n in ref.DEGENERATE if n.startswith("slope")])
def test_slope_and_eps_at_their_ends(renderer, name):
    _degenerate(renderer, name)


@pytest.mark.parametrize("momentum", (0.0, 1.0))
def test_momentum_at_its_ends(renderer, momentum):
    spec, params, noise, _ = ref.edge_case("toy", 65)
    spec = ref.respec(spec, momentum=momentum)
    run = Trunks(renderer, spec, params, noise, 65)
    _check_layers(run, params, noise, f"momentum {momentum}")
    for t, layers in enumerate(params):
        for l, layer in enumerate(layers):
            rm, rv = run.running(t, l)
            if momentum == 0.0:
                assert _same(rm, layer["rm"]) and _same(rv, layer["rv"]), (t, l)
            else:
                d = run.layer(t, l)
                rv64 = d["var"] * 65 / 64.0
                assert np.all(np.abs(rm - d["mean"]) <= _ulp32(d["mean"])) and np.all(np.abs(rv - rv64) <= _ulp32(rv64)), (t, l)


def test_a_joint_with_a_zero_axis_is_nan_and_the_others_are_not(renderer):
    spec, params, noise, _ = ref.edge_case("toy", 65)
    run = Trunks(renderer, spec, params, noise, 65)
    J, dead = 5, 2
    w2, b2 = ref.make_head(4 * J, spec.trunks[0][1], np.random.RandomState(860))
    w2[4 * dead:4 * dead + 3], b2[4 * dead:4 * dead + 3] = 0.0, 0.0
    _, _, y, _ = _check_head(run, 0, J, 860, "zero axis", head=(w2, b2), nan_joints=(dead,))
    assert np.all(y[:, 4 * dead:4 * dead + 3] == 0.0)
    d_w2, d_b2, d_h = _bounded_head_backward(run, 0, w2, y, 861, "zero axis head")     # (the NaN pattern is the float64 reference's)
    rows = np.arange(4 * dead, 4 * dead + 4)
    others = np.setdiff1d(np.arange(4 * J), rows)
    assert np.all(np.isnan(d_w2.reshape(4 * J, -1)[rows])) and np.all(np.isnan(d_b2[rows])) and np.all(np.isnan(d_h))
    assert np.all(np.isfinite(d_w2.reshape(4 * J, -1)[others])) and np.all(np.isfinite(d_b2[others]))


@pytest.mark.parametrize("angle", (0.0, 1e-7, 3.5, -2.0))
def test_the_rotation_head_on_an_exact_axis_at_zero_small_and_large_angles(renderer, angle):
    """r = lrelu(beta) exactly on the R trunk's first seven columns: the axis (0.3, -0.5 slope, 0.8) without spread, the angle
    lrelu(`angle`): 0 (R = I exactly), 1e-7 (the small-angle series), 3.5, and -2 through the slope"""
    spec, params, noise, _ = ref.edge_case("toy", 65)
    params = ref.last_layer_output(params, 2, (0.3, -0.5, 0.8, 0.0, 0.0, 0.0, angle))
    run = Trunks(renderer, spec, params, noise, 65)
    r = run.h(2, spec.layers(2) - 1)[:, :7]
    want = np.asarray((0.3, -0.5, 0.8, 0.0, 0.0, 0.0, angle), np.float32)
    assert np.all(r == np.where(want > 0, want, want.astype(np.float64) * np.float64(np.float32(spec.slope)))[None, :])
    R, _, _ = _rt_check(run, 2, 0, 7, 870)
    if angle == 0.0:
        assert np.all(R == np.eye(3, dtype=np.float32)[None])


def test_the_rotation_head_with_a_zero_axis_row_and_on_the_narrowest_trunks(renderer):
    spec, params, noise, _ = ref.edge_case("toy", 65)
    params = ref.last_layer_output(params, 2, (0.0, 0.0, 0.0, 1.0, 1.0, 1.0, 0.7))      # axis = eps itself

    def edit(eps):
        eps[5] = 0.0
    _rt_check(Trunks(renderer, spec, params, noise, 65), 2, 0, 7, 871, eps_edit=edit, nan_rows=(5,))
    spec, params, noise, _ = ref.edge_case("flat", 65)
    _rt_check(Trunks(renderer, spec, params, noise, 65), 0, 1, 64, 872)                  # R trunk 7 wide, T trunk 3 wide, J = 64


# ---- (d) the modules ------------------------------------------------------------------------------------------------------------------------
B_MOD = 33


def _module_grads(renderer, seed, noise, x, cot, frozen=lambda k: False, backward=None):
    """a fresh HipPoseGenerator from `seed` (the same running statistics every time), one forward, one backward (`backward(pose)`, or
    the loss sum(pose cot)) -> {name: grad bytes or None}"""
    m, _, _ = _modules(renderer, seed, ())
    for k, p in m.named_parameters():
        p.requires_grad_(not frozen(k))
    pose = m(x, noise=noise)["pose_ba"]
    if backward is None:
        (pose * cot).sum().backward()
    else:
        backward(pose)
    return {k: None if p.grad is None else p.grad.cpu().numpy() for k, p in m.named_parameters()}


@pytest.fixture(scope="module")
def module_case(renderer):
    rng = np.random.RandomState(880)
    x = torch.tensor(rng.standard_normal((B_MOD, 24, 3)).astype(np.float32), device=DEV)
    cot = torch.tensor(rng.standard_normal((B_MOD, 24, 3)).astype(np.float32), device=DEV)
    noise = _noise(B_MOD, 881)
    return x, cot, noise, _module_grads(renderer, 882, noise, x, cot)


@pytest.mark.parametrize("case", ["w2 frozen", "every trunk parameter frozen", "one batch norm weight trainable"])
def test_frozen_parameters_keep_no_gradient_and_the_rest_keep_their_bytes(renderer, module_case, case):
    x, cot, noise, full = module_case
    one = "BAprocess.linear_stages.0.batch_norm2.weight"
    frozen = {"w2 frozen": lambda k: k.startswith("BAprocess.w2."), "every trunk parameter frozen": lambda k: not k.startswith("BAprocess.w2."),
              "one batch norm weight trainable": lambda k: k != one}[case]
    part = _module_grads(renderer, 882, noise, x, cot, frozen)
    assert full[one] is not None and full["BAprocess.w2.bias"] is not None and full["BAprocess.w1.weight"] is not None
    for k, g in part.items():
        if frozen(k) or k.startswith("RTprocess."):
            assert g is None, k
        else:
            assert g is not None and _same(g, full[k]), k


def test_a_float64_and_a_non_contiguous_cotangent_give_the_plain_bytes(renderer, module_case):
    """the same values handed back as float64, and through pose_ba.permute(1, 0, 2): the cotangent that reaches the function is then
    the [B,J,3] view of a contiguous [J,B,3] tensor"""
    x, cot, noise, full = module_case

    def as_double(pose):
        pose.backward(gradient=cot.double())

    def permuted(pose):
        (pose.permute(1, 0, 2) * cot.permute(1, 0, 2).contiguous()).sum().backward()
    for backward in (as_double, permuted):
        got = _module_grads(renderer, 882, noise, x, cot, backward=backward)
        for k, g in full.items():
            assert (g is None) == (got[k] is None) and (g is None or _same(g, got[k])), (backward.__name__, k)


def test_two_forwards_before_either_backward_keep_their_own_tapes(renderer, module_case):
    x, cot, noise_a, _ = module_case
    noise_b = _noise(B_MOD, 883)
    m, _, _ = _modules(renderer, 882, ())
    names = [k for k, p in m.named_parameters() if not k.startswith("RTprocess.")]
    ps = [dict(m.named_parameters())[k] for k in names]
    alone = []
    for noise in (noise_a, noise_b):
        one, _, _ = _modules(renderer, 882, ())
        pose = one(x, noise=noise)["pose_ba"]
        alone.append(torch.autograd.grad((pose * cot).sum(), [dict(one.named_parameters())[k] for k in names]))
    pose_a, pose_b = m(x, noise=noise_a)["pose_ba"], m(x, noise=noise_b)["pose_ba"]
    g_b = torch.autograd.grad((pose_b * cot).sum(), ps)
    g_a = torch.autograd.grad((pose_a * cot).sum(), ps)
    assert not torch.equal(pose_a, pose_b)
    for k, a, b, a1, b1 in zip(names, g_a, g_b, alone[0], alone[1]):
        assert torch.equal(a, a1) and torch.equal(b, b1), k


def test_a_ragged_module_against_float64_at_the_devices_tape(renderer):
    """HipBAGenerator(noise 5, width 40, one stage): every parameter gradient of the module, whatever its size, against the float64
    chain at the device's own tape and masks under the carried bound.  The module keeps its tape to itself; the same parameters and
    draws through the raw entry points give the same bytes (tests/test_gpu_generator.py's exactness tests), and that run is read."""
    B, J = 65, 24
    m, sd, spec, layers, noise, d_pose = ref.ragged_module_case(renderer)
    m.load_state_dict({k: torch.as_tensor(v) for k, v in sd.items()}, strict=True)
    m = m.to(DEV).train()
    pose = m(torch.zeros(B, J, 3, device=DEV), noise=noise)
    (pose * torch.tensor(d_pose, device=DEV)).sum().backward()
    run = Trunks(renderer, spec, [layers], [noise], B)
    w2, b2 = sd["w2.weight"], sd["w2.bias"]
    y, pose_raw = run.head(0, J, w2, b2)
    assert _same(pose_raw, pose.detach().cpu().numpy())
    slope, eps = ref.held(spec)
    d_h = run.head_backward(0, d_pose)[2].reshape(B, 40)
    g64, bound = ref.ba_head_backward_with_bound(run.h(0, 2), w2, y, d_pose)
    named = {k: p.grad.cpu().numpy() for k, p in m.named_parameters()}
    _inside("ragged module d_w2", named["w2.weight"], g64[0], bound[0], "w2.weight")
    _inside("ragged module d_b2", named["w2.bias"], g64[1], bound[1], "w2.bias")
    _inside("ragged module d_h", d_h, g64[2], bound[2], "d_h")
    tape, masks = _device_tape(run, 0, noise)
    t64, tbound = ref.trunk_backward_with_bound(layers, tape, masks, d_h, slope, eps)
    for l, layer in enumerate(layers):
        lin, bn = layer["names"]
        for i, key in enumerate((lin + ".weight", lin + ".bias", bn + ".weight", bn + ".bias")):
            _inside(f"ragged module d_{KEYS[i]}", named[key], t64[l][i], tbound[l][i], key)
    assert len(named) == 4 * 3 + 2
