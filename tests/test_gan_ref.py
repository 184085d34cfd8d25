"""The adversarial game without a GPU: the float64 restatement (tests/gan_ref.py) against the reference's own numbers
(tests/golden/pose_discriminators.npz, written by tools/gen_golden.py from run_gan.py's classes), its hand-written backward against
float64 autograd, the pool and the host draw order against the reference's trace, the modules' state-dict keys, and the C ABI of
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
