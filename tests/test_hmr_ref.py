"""The HMR regression head without a GPU: the float64 restatement (tests/hmr_ref.py) against the reference's own numbers
(tests/golden/hmr_head.npz, written by tools/gen_golden_hmr.py from run_gan.py's classes) in both modes, outputs and gradients; its
hand-written backward against float64 autograd of `regressors.stock_forward`, at the toy and the shipped spec and at the nine of
`hmr_ref.edge_specs`; rot6d_to_rotmat at its degenerate inputs; the module's state-dict keys and shapes; the C ABI of
include/posegen_regressor.h as the library exports it; and the bounds the device is held to (tests/hmr_checks.py) confronted with a
float32 emulation of the head: honest rounding stays inside them at every spec, planted errors leave them."""
import ctypes as C
import os
import re

import numpy as np
import pytest
import torch

from posegen_amd import _ffi, regressors as reg
from tests import hmr_checks as chk
from tests import hmr_ref as ref
from tests import stream_harness as sh

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = np.load(os.path.join(REPO, "tests", "golden", "hmr_head.npz"))
HEADER = os.path.join(REPO, "include", "posegen_regressor.h")
COMPUTE = ("pg_hmr_head_forward", "pg_hmr_head_backward")
OUTS = ("pred_rotmat", "pred_shape", "pred_cam")
EDGE_SMALL = ("minimum", "no_shape", "no_cam", "pose_only", "step64")        # (eval mode with a per-row init as well)


def _rel(a, b):
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    return float(np.max(np.abs(a - b)) / max(1.0, float(np.max(np.abs(b)))))


@pytest.fixture(scope="module")
def golden():
    spec = ref.shipped_spec()
    sd = ref.make_state_dict(spec, int(GOLDEN["weight_seed"]))
    masks = ref.unpack_masks(GOLDEN["masks_packed"], tuple(GOLDEN["masks_shape"]))
    P = ref.params_of(sd)
    return spec, sd, P, masks, ref.forward(P, GOLDEN["xf"], ref.init_of(sd), spec, None), ref.forward(P, GOLDEN["xf"], ref.init_of(sd), spec, masks)


def test_the_stored_masks_and_mean_parameters_come_from_the_stored_seeds(golden):
    spec, sd, _, masks, _, _ = golden
    assert np.array_equal(masks, ref.make_masks(spec, 5, int(GOLDEN["mask_seed"]))) and float(GOLDEN["p_drop"]) == spec.p_drop == 0.5
    for k in ("pose", "shape", "cam"):
        assert np.array_equal(GOLDEN[f"mean_{k}"], sd[f"init_{k}"].reshape(-1))
    assert GOLDEN["xf"].shape == (5, 2048) and GOLDEN["xf"].dtype == np.float64
    assert os.path.getsize(os.path.join(REPO, "tests", "golden", "hmr_head.npz")) < max(
        os.path.getsize(os.path.join(REPO, "tests", "golden", f)) for f in os.listdir(os.path.join(REPO, "tests", "golden")) if f != "hmr_head.npz")


@pytest.mark.parametrize("mode", ["eval", "train"])
def test_the_restatement_equals_the_reference_forward(golden, mode):
    out = golden[4] if mode == "eval" else golden[5]
    for k, mine in zip(OUTS, (out["rotmat"], out["shape"], out["cam"])):
        assert mine.shape == GOLDEN[f"{mode}_{k}"].shape and _rel(mine, GOLDEN[f"{mode}_{k}"]) <= 1e-12, k
    assert _rel(golden[4]["rotmat"], golden[5]["rotmat"]) > 1e-3                # (the masks do something)


def test_the_restatement_equals_the_reference_backward(golden):
    spec, sd, P, masks, _, out = golden
    cot, loss = [], 0.0
    for k, mine in zip(OUTS, (out["rotmat"], out["shape"], out["cam"])):
        diff = mine - GOLDEN[f"target_{k}"]
        loss += 0.5 * np.mean(diff * diff)
        cot.append(diff / diff.size)
    assert abs(loss - float(GOLDEN["loss"])) <= 1e-12 * max(1.0, float(GOLDEN["loss"]))
    g = ref.backward(P, GOLDEN["xf"], spec, masks, out, *cot)
    assert _rel(g["d_xf"], GOLDEN["d_xf"]) <= 1e-12
    at = 0
    for i, key in enumerate(str(k) for k in GOLDEN["param_keys"]):
        lin, leaf = key.split(".")
        mine = g[f"{lin}_{'w' if leaf == 'weight' else 'b'}"]
        assert mine.shape == sd[key].shape
        idx = ref.grad_sample_index(mine.size)
        scale = max(1.0, float(GOLDEN["grad_abs_sum"][i]))
        assert abs(mine.sum() - GOLDEN["grad_sum"][i]) <= 1e-12 * scale and abs(np.abs(mine).sum() - GOLDEN["grad_abs_sum"][i]) <= 1e-12 * scale, key
        assert _rel(mine.reshape(-1)[idx], GOLDEN["grad_samples"][at:at + len(idx)]) <= 1e-12, key
        at += len(idx)
    assert at == GOLDEN["grad_samples"].size


def _module(spec, sd, dtype=torch.float64):
    head = reg.HipHMRHead(spec.n_feat, spec.n_hidden, spec.n_joints, spec.n_shape, spec.n_cam, spec.p_drop)
    head.load_state_dict({k: torch.as_tensor(v) for k, v in sd.items()}, strict=True)
    return head.to(dtype)


def _spec(which, n_iter=None):
    if which in ("toy", "shipped"):
        return (ref.toy_spec if which == "toy" else ref.shipped_spec)(*(() if n_iter is None else (n_iter,)))
    spec = ref.edge_specs()[which]
    return spec if n_iter is None else spec.with_iter(n_iter)


def _grad_equals(mine, theirs, shape):
    """1e-12 on a gradient; one without elements (an empty decoder's, which autograd may leave None) has only its shape to compare"""
    assert mine.shape == tuple(shape)
    if not mine.size:
        return theirs is None or tuple(theirs.shape) == tuple(shape)
    return _rel(mine, theirs.numpy()) <= 1e-12


@pytest.mark.parametrize("which,n_iter,with_masks,per_row", [("toy", 3, True, False), ("toy", 1, False, True), ("toy", 8, True, True),
                                                            ("shipped", 3, True, False)]
                         + [(name, None, True, False) for name in ref.edge_specs()] + [(name, None, False, True) for name in EDGE_SMALL])
def test_the_hand_written_backward_equals_float64_autograd_of_stock_forward(which, n_iter, with_masks, per_row):
    spec = _spec(which, n_iter)
    n_iter = spec.n_iter
    B = 6
    sd = ref.make_state_dict(spec, 51)
    rng = np.random.RandomState(52)
    xf = rng.standard_normal((B, spec.n_feat))
    masks = ref.make_masks(spec, B, 53) if with_masks else None
    init = rng.standard_normal((B, spec.n_state)) if per_row else ref.init_of(sd)
    head = _module(spec, sd)
    xt = torch.tensor(xf, requires_grad=True)
    kw = {}
    if per_row:
        it = torch.tensor(init, requires_grad=True)
        a, b = spec.n_pose, spec.n_pose + spec.n_shape
        kw = {"init_pose": it[:, :a], "init_shape": it[:, a:b], "init_cam": it[:, b:]}
    outs = reg.stock_forward(head.eval(), xt, n_iter=n_iter, masks=masks, **kw)
    cot = [rng.standard_normal(tuple(o.shape)) for o in outs]
    torch.autograd.backward(outs, [torch.tensor(c) for c in cot])
    P = ref.params_of(sd)
    mine = ref.forward(P, xf, init, spec, masks)
    for o, m, cols in zip(outs, (mine["rotmat"], mine["shape"], mine["cam"]), (None, spec.n_shape, spec.n_cam)):
        assert m.shape == tuple(o.shape) and (cols is None or m.shape == (B, cols))
        assert (m.size == 0 and cols == 0) or _rel(m, o.detach().numpy()) <= 1e-12
    g = ref.backward(P, xf, spec, masks, mine, *cot)
    assert _rel(g["d_xf"], xt.grad.numpy()) <= 1e-12
    if per_row:
        assert _rel(g["d_init"], it.grad.numpy()) <= 1e-12
    for lin in ref.LINEARS:
        assert _grad_equals(g[f"{lin}_w"], getattr(head, lin).weight.grad, spec.shapes()[f"{lin}_w"]), lin
        assert _grad_equals(g[f"{lin}_b"], getattr(head, lin).bias.grad, spec.shapes()[f"{lin}_b"]), lin
    assert sum(g[f"{lin}_w"].size == 0 for lin in ref.LINEARS) == (spec.n_shape == 0) + (spec.n_cam == 0)


def test_rot6d_at_a_zero_first_axis_at_parallel_axes_and_through_the_clamp():
    x = np.zeros((4, 6))
    x[0, 1::2] = [0.0, 2.0, 0.0]                                               # a1 = 0: the reference's zeros in b1 and b3, b2 = a2 / |a2|
    x[1, 0::2], x[1, 1::2] = [1.0, 2.0, 2.0], [2.0, 4.0, 4.0]                  # a2 parallel to a1: a2 - (b1 . a2) b1 = 0 exactly
    x[2, 0::2], x[2, 1::2] = [3e-13, 0.0, 0.0], [0.0, 5e-13, 0.0]              # both norms below the clamp
    x[3] = [0.3, -1.2, 2.0, 0.5, -0.7, 0.1]
    R = ref.rot6d(x)
    assert np.array_equal(R[0], np.array([[0.0, 0.0, 0.0], [0.0, 1.0, 0.0], [0.0, 0.0, 0.0]])) and not np.isnan(R).any()
    assert np.allclose(R[1][:, 0], np.array([1.0, 2.0, 2.0]) / 3.0) and np.array_equal(R[1][:, 1:], np.zeros((3, 2)))
    assert np.allclose(R[2][:, 0], [0.3, 0.0, 0.0]) and np.allclose(R[2][:, 1], [0.0, 0.5, 0.0])
    assert np.allclose(R[3].T @ R[3], np.eye(3), atol=1e-14) and np.isclose(np.linalg.det(R[3]), 1.0)
    xt = torch.tensor(x, requires_grad=True)
    Rt = reg.rot6d_to_rotmat(xt)
    assert _rel(R, Rt.detach().numpy()) <= 1e-12
    G = np.random.RandomState(3).standard_normal(R.shape)
    Rt.backward(torch.tensor(G))
    mine, theirs = ref.rot6d_backward(x, G), xt.grad.numpy()
    for row in (0, 2, 3):                                                      # the clamp's own gradient: g / 1e-12 below it
        assert np.max(np.abs(mine[row] - theirs[row])) <= 1e-12 * max(1.0, float(np.max(np.abs(theirs[row])))), row
    assert np.max(np.abs(mine[2])) > 1e11
    # (row 1: a2 - (b1 . a2) b1 is zero only up to rounding, and the clamp's 1e12 multiplies the difference between two evaluations)
    ratios = ref.rot6d_conditioning(x)
    assert ratios[0][0] == 0.0 and ratios[1][1] < 1e-15 and min(ratios[0][3], ratios[1][3]) > 1e-3


def test_the_module_carries_the_references_state_dict(golden):
    spec, sd, _, _, _, _ = golden
    head = reg.HipHMRHead()
    state = head.state_dict()
    keys = [str(k) for k in GOLDEN["keys"]]
    assert sorted(state.keys()) == sorted(keys) and list(state.keys())[:3] == list(ref.INIT_KEYS)
    assert {k: ",".join(str(n) for n in state[k].shape) for k in keys} == dict(zip(keys, (str(s) for s in GOLDEN["shapes"])))
    assert float(head.decpose.weight.detach().abs().max()) <= 0.01 * np.sqrt(6.0 / (1024 + 144)) + 1e-9      # xavier_uniform_, gain 0.01
    head.load_state_dict({k: torch.as_tensor(v) for k, v in sd.items()}, strict=True)
    assert np.array_equal(head.deccam.weight.detach().numpy(), sd["deccam.weight"]) and np.array_equal(head.init_pose.numpy(), sd["init_pose"])
    with pytest.raises(RuntimeError):
        head.load_state_dict({k: torch.as_tensor(v) for k, v in sd.items() if k != "fc2.bias"}, strict=True)
    torch.optim.Adam(head.parameters(), lr=1e-4)
    assert head.train().training and not head.eval().training
    import posegen_amd
    assert posegen_amd.HipHMRHead is reg.HipHMRHead and posegen_amd.HipHMR is reg.HipHMR


def test_adopt_shares_the_instances_parameters():
    class Stand(torch.nn.Module):
        def __init__(self):
            super().__init__()
            self.conv1 = torch.nn.Conv2d(3, 8, 3)
            self.bn1, self.relu, self.maxpool = torch.nn.BatchNorm2d(8), torch.nn.ReLU(), torch.nn.Identity()
            self.layer1 = self.layer2 = self.layer3 = self.layer4 = torch.nn.Identity()
            self.avgpool = torch.nn.AdaptiveAvgPool2d(1)
            self.fc1, self.drop1 = torch.nn.Linear(8 + 26, 12), torch.nn.Dropout(0.25)
            self.fc2, self.drop2 = torch.nn.Linear(12, 12), torch.nn.Dropout(0.25)
            self.decpose, self.decshape, self.deccam = torch.nn.Linear(12, 18), torch.nn.Linear(12, 5), torch.nn.Linear(12, 3)
            for k, n in (("init_pose", 18), ("init_shape", 5), ("init_cam", 3)):
                self.register_buffer(k, torch.ones(1, n))
    model = Stand()
    hmr = reg.HipHMR.adopt(model)
    assert hmr.head.spec.n_feat == 8 and hmr.head.spec.n_joints == 3 and hmr.head.drop1.p == 0.25
    for lin in ref.LINEARS:
        assert getattr(hmr.head, lin).weight is getattr(model, lin).weight and getattr(hmr.head, lin).bias is getattr(model, lin).bias
    assert hmr.head.init_pose is model.init_pose and hmr.trunk.conv1 is model.conv1
    assert {id(p) for p in hmr.parameters()} == {id(p) for p in model.parameters()}
    assert hmr.trunk(torch.zeros(2, 3, 9, 9)).shape == (2, 8)


def test_host_inputs_are_refused_in_the_modules_words():
    with pytest.raises(NotImplementedError, match="there is no CPU path"):
        reg.HipHMRHead(37, 50, 3, 5, 3)(torch.zeros(4, 37))
    with pytest.raises(ValueError, match="p_drop"):
        reg.HmrSpec(p_drop=1.0)
    with pytest.raises(ValueError, match="n_iter"):
        reg.HmrSpec(n_iter=9)


def test_the_fourth_header_declares_its_three_functions_and_the_library_exports_them():
    with open(HEADER) as f:
        text = f.read()
    code = re.sub(r"/\*.*?\*/", " ", text, flags=re.S)
    decls = {m.group(1): m.group(2) for m in re.finditer(r"\bint\s+(pg_\w+)\s*\(([^;]*?)\)\s*;", code, flags=re.S)}
    assert set(decls) == set(COMPUTE) | {"pg_hmr_tape_size"}
    assert sh.stream_entry_points(text) == list(COMPUTE)
    for name in COMPUTE:
        args = [a.strip() for a in decls[name].split(",")]
        assert re.fullmatch(r"pg_handle\s*\*\s*h", args[0]) and re.fullmatch(r"void\s*\*\s*stream", args[1]), name
        body = text[:text.index(f"int {name}(")]
        assert "Asynchronous on `stream`" in re.sub(r"\s*\n\s*\*?\s*", " ", body[body.rindex("/*"):]), name
    assert "PG_ABI_VERSION" not in code and '#include "posegen_hip.h"' in code
    lib = _ffi.load_library()
    assert set(_ffi.REGRESSOR_PROTOTYPES) == set(decls)
    assert not set(_ffi.REGRESSOR_PROTOTYPES) & (set(_ffi.PROTOTYPES) | set(_ffi.GAN_PROTOTYPES) | set(_ffi.GENERATOR_PROTOTYPES))
    for name, (res, args) in _ffi.REGRESSOR_PROTOTYPES.items():
        assert hasattr(lib, name), f"{name} is declared in include/posegen_regressor.h but not exported"
        fn = getattr(lib, name)
        assert res is C.c_int and fn.restype is C.c_int and list(fn.argtypes) == args
        assert len(args) == len(decls[name].split(",")), name
    assert lib.pg_abi_version() == _ffi.PG_ABI_VERSION == 11
    assert C.sizeof(_ffi.PgHmrSpec) == 7 * 4 and C.sizeof(_ffi.PgHmrParams) == C.sizeof(_ffi.PgHmrGrads) == 10 * 8
    members = re.findall(r"(?:const\s+)?float\s*\*\s*(\w+);", code[code.index("typedef struct pg_hmr_params"):code.index("} pg_hmr_params;")])
    assert tuple(members) == _ffi.HMR_TENSORS
    for name in ("PG_HMR_MAX_FEAT", "PG_HMR_MAX_HIDDEN", "PG_HMR_MAX_JOINTS", "PG_HMR_MAX_SHAPE", "PG_HMR_MAX_CAM", "PG_HMR_MAX_ITER", "PG_HMR_MAX_ROWS"):
        assert int(re.search(rf"#define {name} (\d+)", code).group(1)) == getattr(_ffi, name), name
    with open(os.path.join(REPO, "posegen_amd", "csrc", "Makefile")) as f:
        mk = f.read()
    assert re.search(r"^SRCS_HIP := .*\bpg_hmr\.hip\b", mk, re.M) and re.search(r"^HDRS := .*posegen_regressor\.h\b", mk, re.M)
    assert "pg_hmr.s 4pghm" in mk and "audit_asm_hazards.py $(AUDITDIR)/pg_hmr.s" in mk


def test_the_tape_size_and_the_host_side_refusals():
    lib = _ffi.load_library()
    n = C.c_int64(-1)
    for spec, B in ((ref.toy_spec(), 17), (ref.shipped_spec(), 128), (ref.toy_spec(8), 1)):
        cs = spec.c_spec()
        assert lib.pg_hmr_tape_size(C.byref(cs), B, C.byref(n)) == 0 and n.value == spec.tape_layout(B)[1]
    cs = ref.toy_spec().c_spec()
    assert lib.pg_hmr_tape_size(C.byref(cs), 0, C.byref(n)) == _ffi.PG_EINVAL
    assert lib.pg_hmr_tape_size(C.byref(cs), _ffi.PG_HMR_MAX_ROWS + 1, C.byref(n)) == _ffi.PG_EINVAL
    assert lib.pg_hmr_tape_size(C.byref(cs), 4, None) == _ffi.PG_EINVAL and lib.pg_hmr_tape_size(None, 4, C.byref(n)) == _ffi.PG_EINVAL
    cs.n_iter = 9
    assert lib.pg_hmr_tape_size(C.byref(cs), 4, C.byref(n)) == _ffi.PG_EINVAL


# ---- honest float32 against the bounds, and planted errors -----------------------------------------------------------------------------------
# The bounds of hmr_ref.*_with_bound are what the device tests hold pg_hmr.hip to.  Here the same checks (tests/hmr_checks.py) judge
# a float32 emulation of the head in numpy: honest rounding in another order of summation must stay inside every bound at every spec,
# and each planted error must leave them at the spec named for it.
ALL_SPECS = ("toy", "shipped") + tuple(ref.edge_specs())
_JUDGED = {}


def _judged(which, training=True, mutant=None, B=17):
    """the shared checks on one emulated run -> [(check, context, offending indices)]; the honest runs are kept"""
    key = (which, training, mutant, B)
    if key in _JUDGED:
        return _JUDGED[key]
    spec = _spec(which)
    sd = ref.make_state_dict(spec, 51)
    rng = np.random.RandomState(52)
    xf = rng.standard_normal((B, spec.n_feat)).astype(np.float32)
    masks = ref.make_masks(spec, B, 53) if training else None
    init = None if training else rng.standard_normal((B, spec.n_state)).astype(np.float32)
    rng = np.random.RandomState(54)
    cots = [rng.standard_normal(shape).astype(np.float32) for shape in ((B, spec.n_joints, 3, 3), (B, spec.n_shape), (B, spec.n_cam))]
    run = chk.Emulated(spec, sd, xf, masks, init, mutant)
    run.forward()
    tag = f"emulated {which} {'train' if training else 'eval'}" + (f" [{mutant}]" if mutant else "")
    with chk.collecting() as failed:
        _, well = chk.check_forward(run, tag)
        chk.check_backward(run, cots, tag)
    assert np.mean(well) >= 0.9
    names = sorted({name[len(tag) + 1:] for name, _, _ in failed})
    print(f"FAILED {tag}: {names}")
    _JUDGED[key] = failed
    return failed


def _names(failed):
    return {name.split(" ")[-1] for name, _, _ in failed}


FORWARD_NAMES = {"P", "h1", "h2", "s", "rotmat"}


@pytest.mark.parametrize("which", ALL_SPECS)
def test_honest_float32_stays_inside_every_bound(which):
    assert _judged(which) == []


def test_honest_float32_stays_inside_every_bound_in_eval_mode_with_a_per_row_init():
    assert _judged("step65", training=False) == []


def test_a_product_that_drops_the_tail_of_k_past_a_multiple_of_16_is_caught_at_step63_and_step65_and_not_at_step64():
    for which in ("step63", "step65"):
        assert {"P", "h1", "h2", "s"} <= _names(_judged(which, mutant="tail16")), which
    assert _judged("step64", mutant="tail16") == []                            # F = H = S = 64: there is no tail, so only the spec shows it


def test_a_segment_compare_off_by_one_is_caught_on_toy_and_differently_on_no_shape():
    def state_columns(which):
        failed = _judged(which, mutant="segment")
        assert "s" in _names(failed)
        return sorted({int(c) for name, _, where in failed if name.endswith(" s") for c in where[:, 1]})
    assert state_columns("toy") == [18, 23]                                    # the first shape column and the first cam column
    assert state_columns("no_shape") == [18]                                   # n1 == n2: the first cam column alone, taken for pose
    assert _judged("pose_only", mutant="segment") == []                       # (one segment: nothing to confuse)


def test_drop1s_mask_in_drop2s_place_in_the_backward_is_caught_on_toy():
    names = _names(_judged("toy", mutant="mask_swap"))
    assert not names & FORWARD_NAMES and {"fc1_w", "fc2_w", "fc1_b", "fc2_b", "d_xf", "d_init"} <= names


def test_d_without_the_last_round_is_caught_in_d_xf_and_the_feature_columns_of_d_fc1_w_alone():
    failed = _judged("toy", mutant="d_short")
    assert _names(failed) == {"d_xf", "fc1_w"}
    cols = {int(c) for name, _, where in failed if name.endswith(" fc1_w") for c in where[:, 1]}
    assert cols and max(cols) < _spec("toy").n_feat


def test_d_init_without_the_residual_is_caught_in_d_init_alone():
    assert _names(_judged("toy", mutant="init_no_residual")) == {"d_init"}


def test_bias_gradients_over_round_0_only_are_invisible_at_minimum_and_caught_on_no_cam():
    assert _judged("minimum", mutant="bias_round0") == []                      # one round: the planted error changes nothing
    assert _names(_judged("no_cam", mutant="bias_round0")) == {"fc1_b", "fc2_b", "decpose_b", "decshape_b"}


def test_every_planted_error_has_its_test():
    tested = {"tail16", "segment", "mask_swap", "d_short", "init_no_residual", "bias_round0"}
    assert set(ref.MUTANTS) == tested
