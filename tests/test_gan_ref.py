"""The adversarial game without a GPU: the float64 restatement (tests/gan_ref.py) against the reference's own numbers
(tests/golden/pose_discriminators.npz, written by tools/gen_golden.py from run_gan.py's classes), its hand-written backward against
float64 autograd, its carried backward bound against torch's float32 arithmetic on the ragged spec, the refusal of a negative or
non-finite slope, the pool (out-of-range slots included) and the host draw order against the reference's trace, the modules' state-dict keys, and the C ABI of
include/posegen_gan.h as the library exports it."""
import os
import re

import numpy as np
import pytest
import torch

from posegen_amd import _ffi, discriminators as disc
from tests import gan_ref
from tests import stream_harness as sh

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = np.load(os.path.join(REPO, "tests", "golden", "pose_discriminators.npz"))
GAN_HEADER = os.path.join(REPO, "include", "posegen_gan.h")
COMPUTE = ("pg_disc_forward", "pg_disc_backward", "pg_disc_loss", "pg_pool_exchange")


def _rel(a, b):
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    return float(np.max(np.abs(a - b)) / max(1.0, float(np.max(np.abs(b)))))


@pytest.fixture(scope="module")
def golden3d():
    spec = disc.pos3d_spec()
    params = gan_ref.make_params(spec, int(GOLDEN["weight_seed"]))
    x = gan_ref.make_inputs(spec, 5, int(GOLDEN["input_seed"]))
    pred, tapes = gan_ref.forward(spec, params, x)
    return spec, params, x, pred, tapes


def test_the_restatement_equals_the_reference_forward(golden3d):
    spec, params, x, pred, _ = golden3d
    assert np.array_equal(x, GOLDEN["x_3d"]) and pred.shape == (5, 7)
    assert _rel(pred, GOLDEN["pred_3d"]) <= 1e-12
    spec2 = disc.pos2d_spec()
    x2 = gan_ref.make_inputs(spec2, 5, int(GOLDEN["input_seed"]))
    pred2, _ = gan_ref.forward(spec2, gan_ref.make_params(spec2, int(GOLDEN["weight_seed"])), x2)
    assert np.array_equal(x2, GOLDEN["x_2d"]) and _rel(pred2, GOLDEN["pred_2d"]) <= 1e-12


def test_the_restatement_equals_the_reference_backward(golden3d):
    spec, params, x, pred, tapes = golden3d
    loss, d_pred = gan_ref.adversarial_loss(pred.numpy().astype(np.float32))
    # the loss on the float64 predictions, as the reference computed it
    d64 = pred.numpy() - 1.0
    assert abs(0.5 * np.mean(d64 * d64) - float(GOLDEN["loss_3d"])) <= 1e-12 * max(1.0, float(GOLDEN["loss_3d"]))
    assert abs(loss - float(GOLDEN["loss_3d"])) <= 1e-6                       # (pg_disc_loss takes float32 predictions)
    d_x, grads = gan_ref.backward(spec, params, x, tapes, gan_ref.masks_of(tapes), 0.5 * 2.0 * d64 / d64.size)
    assert _rel(d_x, GOLDEN["d_x_3d"]) <= 1e-12
    keys = [str(k) for k in GOLDEN["keys_3d"]]
    by_key = {}
    for p, (name, _, _, _) in enumerate(spec.paths):
        for lname, (dw, db) in zip(disc.LAYER_NAMES, grads[p]):
            by_key[f"{name}.{lname}.weight"], by_key[f"{name}.{lname}.bias"] = dw, db
    samples, at = GOLDEN["grad_samples_3d"], 0
    for i, k in enumerate(keys):
        g = by_key[k].reshape(-1)
        idx = gan_ref.grad_sample_index(g.numel())
        scale = max(1.0, float(GOLDEN["grad_abs_sum_3d"][i]))
        assert abs(float(g.sum()) - float(GOLDEN["grad_sum_3d"][i])) <= 1e-12 * scale, k
        assert abs(float(g.abs().sum()) - float(GOLDEN["grad_abs_sum_3d"][i])) <= 1e-12 * scale, k
        assert _rel(g[idx], samples[at:at + len(idx)]) <= 1e-12, k
        at += len(idx)
    assert at == len(samples)


@pytest.mark.parametrize("make_spec", [gan_ref.toy_spec, gan_ref.toy_spec_sparse, disc.pos2d_spec], ids=["toy", "toy_sparse", "pos2d"])
def test_the_hand_written_backward_equals_float64_autograd(make_spec):
    spec = make_spec()
    params = gan_ref.make_params(spec, 3)
    x = gan_ref.make_inputs(spec, 9, 4)
    leaves = [[(gan_ref.t64(w).requires_grad_(True), gan_ref.t64(b).requires_grad_(True)) for w, b in layers] for layers in params]
    xt = gan_ref.t64(x).requires_grad_(True)
    preds = []
    for p, layers in enumerate(leaves):
        h = gan_ref.path_input(spec, p, xt)
        for l, (w, b) in enumerate(layers):
            h = torch.nn.functional.linear(h, w, b)
            if l < 4:
                h = torch.nn.functional.leaky_relu(h, spec.slope)
        preds.append(h)
    pred = torch.cat(preds, 1)
    d_pred = torch.as_tensor(np.random.RandomState(5).standard_normal(tuple(pred.shape)))
    pred.backward(d_pred)
    ref_pred, tapes = gan_ref.forward(spec, params, x)
    assert _rel(ref_pred, pred.detach()) <= 1e-12
    d_x, grads = gan_ref.backward(spec, params, x, tapes, gan_ref.masks_of(tapes), d_pred)
    assert _rel(d_x, xt.grad) <= 1e-12
    for p, layers in enumerate(leaves):
        for l, (w, b) in enumerate(layers):
            assert _rel(grads[p][l][0], w.grad) <= 1e-12 and _rel(grads[p][l][1], b.grad) <= 1e-12, (p, l)
    if make_spec is gan_ref.toy_spec_sparse:
        unselected = [j for j in range(24) if j not in (0, 5, 7, 23)]
        assert not d_x[:, unselected].any() and d_x[:, [0, 5, 7, 23]].abs().min() > 0


def test_the_ragged_specs_hit_the_shapes_they_are_for():
    s3, s2 = gan_ref.ragged3_spec(), gan_ref.ragged2_spec()
    assert [(len(sel) * 3, w, m) for _, sel, w, m in s3.paths] == [(3, 1, 1), (9, 67, 130), (15, 64, 16), (6, 129, 65), (3, 17, 80),
                                                                  (6, 80, 63), (9, 16, 64), (6, 33, 5)]
    assert s3.n_points == 5 and s3.point_dim == 3 and s3.slope == 0.01 and len(s3.paths) == _ffi.PG_DISC_MAX_PATHS
    assert [(len(sel) * 2, w, m) for _, sel, w, m in s2.paths] == [(48, 65, 3), (2, 3, 67)] and s2.n_points == 24 and s2.point_dim == 2
    # rows 0, 1 and 3 are selected at most once within a path; 2 and 4 are repeated in one
    assert all(sel.count(j) <= 1 for _, sel, _, _ in s3.paths for j in (0, 1, 3)) and s3.paths[1][1].count(4) == 2 and s3.paths[7][1].count(2) == 2
    one = gan_ref.one_path_spec(s3, 3)
    assert one.paths == [s3.paths[3]] and one.n_points == 5 and one.layer_shapes(0) == s3.layer_shapes(3)


@pytest.mark.parametrize("B", [1, 63, 65, 129])
def test_the_backward_bound_holds_torch_float32_on_the_ragged_spec(B):
    """torch's own float32 arithmetic on the CPU stands in for the device: its tape and masks go in as the layer inputs, its dW and
    d_x must lie within the carried bound.  Its db need not (torch sums the bias gradient in float32; the bound describes a double
    sum rounded once), so db is checked on that: the float32 chain's own dZ summed in double and rounded once."""
    spec = gan_ref.ragged3_spec()
    params = gan_ref.make_params(spec, 18)
    x = gan_ref.make_inputs(spec, B, 100 + B)
    d_pred = np.random.RandomState(3).standard_normal((B, 8)).astype(np.float32)
    _, tapes32 = gan_ref.forward(spec, params, x, torch.float32)
    tapes32 = [[h.numpy() for h in tape] for tape in tapes32]
    masks = gan_ref.masks_of(tapes32)
    d_x, grads, e_dx, bounds = gan_ref.backward_with_bound(spec, params, x, tapes32, masks, d_pred)
    plain_dx, plain = gan_ref.backward(spec, params, x, tapes32, masks, d_pred)
    assert torch.equal(plain_dx, d_x) and all(torch.equal(a, b) for g, h in zip(grads, plain) for wb, vc in zip(g, h) for a, b in zip(wb, vc))
    dzs = []
    dx32, g32 = gan_ref.backward(spec, params, x, tapes32, masks, d_pred, torch.float32, dz_out=dzs)
    err = (dx32.to(gan_ref.F64) - d_x).abs()
    assert bool((err <= e_dx).all())
    worst_w = 0.0
    for p in range(8):
        for l in range(5):
            dw_err = (g32[p][l][0].to(gan_ref.F64) - grads[p][l][0]).abs()
            assert bool((dw_err <= bounds[p][l][0]).all()), (p, l)
            worst_w = max(worst_w, float((dw_err / bounds[p][l][0]).max()))
            db_once = dzs[p][l].to(gan_ref.F64).sum(0).to(torch.float32).to(gan_ref.F64)
            assert bool(((db_once - grads[p][l][1]).abs() <= bounds[p][l][1]).all()), (p, l)
            assert bounds[p][l][0].shape == grads[p][l][0].shape and bounds[p][l][1].shape == grads[p][l][1].shape
    assert 0.0 < worst_w <= 1.0 and 0.0 < float((err / e_dx).max()) <= 1.0


def test_the_bound_is_zero_on_rows_that_no_path_selects():
    spec = gan_ref.toy_spec_sparse()
    params = gan_ref.make_params(spec, 3)
    x = gan_ref.make_inputs(spec, 4, 4)
    _, tapes = gan_ref.forward(spec, params, x)
    d_x, _, e_dx, _ = gan_ref.backward_with_bound(spec, params, x, tapes, gan_ref.masks_of(tapes), np.ones((4, 2)))
    unselected = [j for j in range(24) if j not in (0, 5, 7, 23)]
    assert not e_dx[:, unselected].any() and not d_x[:, unselected].any() and e_dx[:, [0, 5, 7, 23]].min() > 0


def test_a_slot_outside_the_pool_passes_through():
    rng = np.random.RandomState(6)
    pool0 = rng.standard_normal((4, 3)).astype(np.float32)
    items = rng.standard_normal((6, 3)).astype(np.float32)
    swap, slot = np.uint8([1, 1, 1, 1, 0, 1]), np.int32([-1, 4, 2, 2 ** 31 - 1, 1, 2])
    out, pool, cur = gan_ref.pool_exchange(pool0, 4, items, swap, slot)
    assert cur == 4 and np.array_equal(out[[0, 1, 3, 4]], items[[0, 1, 3, 4]])
    assert np.array_equal(out[2], pool0[2]) and np.array_equal(out[5], items[2]) and np.array_equal(pool[2], items[5])
    assert np.array_equal(pool[[0, 1, 3]], pool0[[0, 1, 3]])
    # while the pool fills nothing is read from `slot`
    out, pool, cur = gan_ref.pool_exchange(np.zeros((8, 3), np.float32), 3, items, np.ones(6, np.uint8), np.int32([-5] * 5 + [8]))
    assert cur == 8 and np.array_equal(out, items) and np.array_equal(pool[3:8], items[:5])


@pytest.mark.parametrize("slope", [-0.01, float("inf"), float("-inf"), float("nan")])
def test_a_negative_or_non_finite_slope_is_refused(slope):
    """the backward reads LeakyReLU's mask off the tape's sign, which only a slope >= 0 preserves"""
    with pytest.raises(ValueError, match="slope"):
        disc.PartSpec(5, 3, [("p", [0, 1], 20, 8)], slope=slope)
    cs = disc.PartSpec(5, 3, [("p", [0, 1], 20, 8)]).c_spec()
    n = _ffi.C.c_int64(-1)
    lib = _ffi.load_library()
    assert lib.pg_disc_tape_floats(_ffi.C.byref(cs), 4, _ffi.C.byref(n)) == _ffi.PG_OK and n.value == 4 * 68
    cs.slope, n.value = slope, -1
    assert lib.pg_disc_tape_floats(_ffi.C.byref(cs), 4, _ffi.C.byref(n)) == _ffi.PG_EINVAL and n.value == -1
    for ok in (0.0, 1.0, 0.2):
        cs.slope = ok
        assert lib.pg_disc_tape_floats(_ffi.C.byref(cs), 4, _ffi.C.byref(n)) == _ffi.PG_OK
        assert disc.PartSpec(5, 3, [("p", [0, 1], 20, 8)], slope=ok).slope == ok


def test_the_accuracy_compares_in_float32_like_the_reference():
    p = GOLDEN["acc_pred"]
    _, c1, n, _ = gan_ref.lsgan(p, 1.0)
    _, c0, _, _ = gan_ref.lsgan(p, 0.0)
    assert c1 / n == float(GOLDEN["acc_real"]) and c0 / n == float(GOLDEN["acc_fake"])
    # exactly label +- 0.5 counts as correct; the next float32 beyond does not
    assert gan_ref.lsgan(np.float32([0.5, 1.5, np.nextafter(np.float32(1.5), np.float32(2)), np.nan]), 1.0)[1] == 2


def test_the_pool_and_the_host_draw_order_reproduce_the_reference_trace():
    items, swap, slot = GOLDEN["pool_items"], GOLDEN["pool_swap"], GOLDEN["pool_slot"]
    assert swap[0].sum() == 0 and swap[1:].sum() >= 3                          # a filling call, the call that crosses full, a full pool
    pool, cur = np.zeros((6, 4), np.float32), 0
    np.random.seed(int(GOLDEN["pool_seed"]))
    for c in range(3):
        sw, sl = disc.pool_draws(6, cur, 5)                                     # the global np.random, as the reference
        assert np.array_equal(sw, swap[c]) and np.array_equal(sl, slot[c]), c
        out, pool, cur = gan_ref.pool_exchange(pool, cur, items[c], sw, sl)
        assert out.tobytes() == GOLDEN["pool_returned"][c].tobytes(), c
    assert cur == 6 and pool.tobytes() == GOLDEN["pool_final"].tobytes()
    # a generator of one's own gives the same draws as the global one at the same seed
    rng = np.random.RandomState(int(GOLDEN["pool_seed"]))
    sw, sl = disc.pool_draws(6, 5, 5, rng)
    assert np.array_equal(sw, swap[1]) and np.array_equal(sl, slot[1])


def test_the_modules_keep_the_reference_state_dict_keys_in_order():
    m3, m2 = disc.HipPos3dDiscriminator(), disc.HipPos2dDiscriminator()
    assert list(m3.state_dict().keys()) == [str(k) for k in GOLDEN["keys_3d"]]
    assert list(m2.state_dict().keys()) == [str(k) for k in GOLDEN["keys_2d"]]
    assert [n for n, _ in m3.named_parameters()] == [str(k) for k in GOLDEN["keys_3d"]]
    # the output columns follow forward's order, not __init__'s
    assert [p[0] for p in m3.spec.paths][4:6] == ["layer_torso", "layer_head"] and m3.spec.module_order[4:6] == ["layer_head", "layer_torso"]
    # init_weights, Adam and the restatement's loader all see plain nn.Linears
    m3.apply(lambda m: torch.nn.init.kaiming_normal_(m.weight) if isinstance(m, torch.nn.Linear) else None)
    torch.optim.Adam(m3.parameters())
    params = gan_ref.make_params(m3.spec, 1)
    gan_ref.load_params(m3, params)
    assert np.array_equal(m3.layer_torso.layer_last.weight.detach().numpy(), params[4][3][0])


def test_host_inputs_are_refused_in_the_modules_words():
    for call in (lambda: disc.HipPos3dDiscriminator()(torch.zeros(2, 24, 3)), lambda: disc.lsgan_loss(torch.zeros(4), 1.0),
                 lambda: disc.FakePool(8).exchange(torch.zeros(2, 4), [0, 0], [0, 0])):
        with pytest.raises(NotImplementedError, match="there is no CPU path"):
            call()


def test_the_second_header_declares_the_five_functions_and_the_library_exports_them():
    """include/posegen_gan.h declares exactly the five functions, each compute one with `pg_handle*` first and `void* stream` second;
    the built library exports them and _ffi binds them with as many arguments; include/posegen_hip.h still yields its 45 stream-taking
    entry points and ABI version 11.  The ctypes table of the new header is `_ffi.GAN_PROTOTYPES`: `_ffi.PROTOTYPES` stays the table
    of posegen_hip.h alone, which tests/test_single_net_host.py compares with that header symbol for symbol."""
    with open(GAN_HEADER) as f:
        text = f.read()
    code = re.sub(r"/\*.*?\*/", " ", text, flags=re.S)
    decls = {m.group(1): m.group(2) for m in re.finditer(r"\bint\s+(pg_\w+)\s*\(([^;]*?)\)\s*;", code, flags=re.S)}
    assert set(decls) == set(COMPUTE) | {"pg_disc_tape_floats"}
    assert sh.stream_entry_points(text) == list(COMPUTE)
    for name in COMPUTE:
        args = [a.strip() for a in decls[name].split(",")]
        assert re.fullmatch(r"pg_handle\s*\*\s*h", args[0]) and re.fullmatch(r"void\s*\*\s*stream", args[1]), name
    assert "stream" not in decls["pg_disc_tape_floats"]
    assert "PG_ABI_VERSION" not in code and '#include "posegen_hip.h"' in code
    lib = _ffi.load_library()
    assert set(_ffi.GAN_PROTOTYPES) == set(decls) and not set(_ffi.GAN_PROTOTYPES) & set(_ffi.PROTOTYPES)
    for name, (res, args) in _ffi.GAN_PROTOTYPES.items():
        assert hasattr(lib, name), f"{name} is declared in include/posegen_gan.h but not exported"
        fn = getattr(lib, name)
        assert res is _ffi.C.c_int and fn.restype is _ffi.C.c_int and list(fn.argtypes) == args
        assert len(args) == len(decls[name].split(",")), name
    assert len(sh.stream_entry_points()) == 45 and lib.pg_abi_version() == _ffi.PG_ABI_VERSION == 11
    # the structs as the header lays them out
    assert _ffi.C.sizeof(_ffi.PgDiscPath) == 27 * 4 and _ffi.C.sizeof(_ffi.PgDiscSpec) == 3 * 4 + 8 * 27 * 4 + 4
    assert _ffi.C.sizeof(_ffi.PgDiscParams) == 2 * 8 * 5 * 8
    # and the build wiring
    with open(os.path.join(REPO, "posegen_amd", "csrc", "Makefile")) as f:
        mk = f.read()
    assert re.search(r"^SRCS_HIP := .*\bpg_disc\.hip\b", mk, re.M) and "pg_disc.s 4pgdc" in mk and "audit_asm_hazards.py $(AUDITDIR)/pg_disc.s" in mk


def test_tape_floats_and_argument_checks_on_the_host():
    lib = _ffi.load_library()
    spec = disc.pos3d_spec()
    n = _ffi.C.c_int64(0)
    cs = spec.c_spec()
    assert lib.pg_disc_tape_floats(_ffi.C.byref(cs), 1024, _ffi.C.byref(n)) == _ffi.PG_OK
    assert n.value == 1024 * 7 * 2500 == 1024 * sum(c for layers in spec.tape_layout(1)[-1:] for _, c in layers) * 7
    last_off, last_cols = spec.tape_layout(1024)[-1][-1]
    assert last_off + 1024 * last_cols == n.value
    assert lib.pg_disc_tape_floats(_ffi.C.byref(cs), 0, _ffi.C.byref(n)) == _ffi.PG_EINVAL
    cs.point_dim = 4
    assert lib.pg_disc_tape_floats(_ffi.C.byref(cs), 8, _ffi.C.byref(n)) == _ffi.PG_EINVAL
    cs = spec.c_spec()
    cs.path[2].sel[1] = 24
    assert lib.pg_disc_tape_floats(_ffi.C.byref(cs), 8, _ffi.C.byref(n)) == _ffi.PG_EINVAL
    # compute entry points refuse a null handle before anything else
    assert lib.pg_disc_loss(None, None, None, 4, 1.0, 1.0, None, None) == _ffi.PG_EINVAL
    assert lib.pg_pool_exchange(None, None, None, 4, 4, 0, None, 1, None, None, None) == _ffi.PG_EINVAL
