"""pg_disc_forward / pg_disc_backward / pg_disc_loss / pg_pool_exchange on the GPU, through the C ABI and through
posegen_amd.discriminators / ganloop, against the float64 restatement (tests/gan_ref.py).

Weights are kaiming_normal_ as init_weights makes them, biases uniform within 1 / sqrt(fan_in), inputs N(0, 0.6^2)
(gan_ref.make_params / make_inputs).  Three kinds of check:

  layer-local (derived, factor 1)   every tape layer and pred against the float64 layer applied to the DEVICE's own previous layer:
      |dev - f64| <= (K + 2) 2^-24 (|h_in| |W|^T + |b|) + 2^-24 |h|  elementwise -- K products and K additions of a float32 dot
      product in any order, the bias addition, the LeakyReLU multiplication.  (LeakyReLU is 1-Lipschitz, so a pre-activation whose
      sign differs from float64's stays within the bound.)
  end to end, measured against torch float32 on the CPU   max |dev - f64| <= 4 max |cpu32 - f64| on the same inputs, for pred and --
      with the DEVICE's masks (the tape's signs) fed to both reference backwards -- for d_x and every parameter gradient, each tensor
      on its own.  4 = the 1.5 - 2.1 that the MFMA's sequential chain costs over torch's blocked sums at these shapes, times 2 for the
      row chunks and for a maximum over few values.  The bias gradients are summed in double on the device (rounded once), so a
      one-element tensor cannot lose to a lucky float32 sum.
  exact   batch independence, repeatability, d_x with and without grads, unselected rows, NaN containment, the loss's count, the pool.

The ratios measured on an MI355X are in DESIGN.md 2.16 and profiles/pose_discriminators.json."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

from posegen_amd import _ffi, discriminators as disc, ganloop
from tests import gan_ref
from tests.frame_metrics_gpu import DEV, renderer  # noqa: F401 (renderer: a fixture)

pytestmark = pytest.mark.gpu
U = 2.0 ** -24
F32 = torch.float32

SPECS = {"pos3d": disc.pos3d_spec, "pos2d": disc.pos2d_spec, "toy": gan_ref.toy_spec, "toy_sparse": gan_ref.toy_spec_sparse}
# the 3-D spec alone in a tile, with a partly filled tile, and with three row tiles; the 2-D spec (K = 48, mid = 100) and the toy
# spec (width 20, mid 36: one partly filled column tile) at a partly filled row tile
LAYER_CASES = [("pos3d", 1), ("pos3d", 17), ("pos3d", 130), ("pos2d", 33), ("toy", 33)]
E2E_CASES = [("pos3d", 130), ("pos2d", 33), ("toy", 33)]

_cache = {}


def flat_dev(params):
    return [torch.tensor(a, device=DEV) for layers in params for wb in layers for a in wb]


def case(name, B):
    """(spec, params, x) of a case with its device copies, made once"""
    key = (name, B)
    if key not in _cache:
        spec = SPECS[name]()
        params = gan_ref.make_params(spec, 11 + len(name))
        x = gan_ref.make_inputs(spec, B, 100 + B)
        _cache[key] = (spec, params, x, flat_dev(params), torch.tensor(x, device=DEV))
    return _cache[key]


def dev_forward(r, spec, pdev, x, want_tape=True):
    B = x.shape[0]
    cs, tab = spec.c_spec(), disc._pointer_table(spec, pdev)
    n = C.c_int64(0)
    r._check(r.lib.pg_disc_tape_floats(C.byref(cs), B, C.byref(n)))
    pred = torch.full((B, len(spec.paths)), -7.0, device=DEV)
    tape = torch.full((n.value,), -7.0, device=DEV) if want_tape else None
    _ffi.call(r, "pg_disc_forward", C.byref(cs), C.byref(tab), x, B, pred, tape)
    torch.cuda.synchronize()
    return pred, tape


def dev_backward(r, spec, pdev, x, tape, d_pred, want_dx=True, want_grads=True):
    B = x.shape[0]
    cs, tab = spec.c_spec(), disc._pointer_table(spec, pdev)
    d_x = torch.full_like(x, -7.0) if want_dx else None
    grads = [torch.full_like(p, -7.0) for p in pdev] if want_grads else None
    gtab = disc._pointer_table(spec, grads) if want_grads else None
    _ffi.call(r, "pg_disc_backward", C.byref(cs), C.byref(tab), x, B, tape, d_pred, d_x, None if gtab is None else C.byref(gtab))
    torch.cuda.synchronize()
    return d_x, grads


def tape_views(spec, B, tape):
    """per path the four tape layers as host float32 arrays [B,n]"""
    host = tape.cpu().numpy()
    return [[host[off:off + B * n].reshape(B, n) for off, n in layers] for layers in spec.tape_layout(B)]


def cotangent(B, n_paths, seed=3):
    return np.random.RandomState(seed).standard_normal((B, n_paths)).astype(np.float32)


def same_bytes(a, b):
    return a.shape == b.shape and torch.equal(a.contiguous().view(torch.uint8), b.contiguous().view(torch.uint8))


# ---- layer-local ---------------------------------------------------------------------------------------------------------------------------
def assert_layer_local(tag, spec, params, x, views, pred):
    """the layer-local criterion of the docstring on a forward's tape `views` and host `pred`; -> the worst error / bound.  Where
    the bound is 0 (a zero row of W with a zero bias) the error must be 0 as well."""
    worst = 0.0
    for p, layers in enumerate(params):
        h_in = gan_ref.path_input(spec, p, gan_ref.t64(x))
        for l, (w, b) in enumerate(layers):
            w64, b64 = gan_ref.t64(w), gan_ref.t64(b)
            want = gan_ref.layer(h_in, w64, b64, spec.slope, act=l < 4)
            got = gan_ref.t64(views[p][l] if l < 4 else pred[:, p:p + 1])
            K = w.shape[1]
            bound = (K + 2) * U * (h_in.abs() @ w64.abs().T + b64.abs()) + U * want.abs()
            err = (got - want).abs()
            ratio = float(torch.where(bound > 0, err / bound, torch.where(err > 0, float("inf"), 0.0).to(gan_ref.F64)).max())
            worst = max(worst, ratio)
            assert ratio <= 1.0, (tag, p, l, ratio)
            h_in = got                                                       # the next layer starts from the device's own values
    return worst


@pytest.mark.parametrize("name,B", LAYER_CASES)
def test_every_layer_is_within_the_float32_dot_product_bound_of_the_float64_layer(renderer, name, B):
    spec, params, x, pdev, xdev = case(name, B)
    pred, tape = dev_forward(renderer, spec, pdev, xdev)
    worst = assert_layer_local((name, B), spec, params, x, tape_views(spec, B, tape), pred.cpu().numpy())
    print(f"layer-local {name} B={B}: worst error / bound {worst:.3f}")


# ---- end to end ------------------------------------------------------------------------------------------------------------------------------
def references(spec, params, x, masks, cot):
    """(pred, d_x, grads) in float64 and in torch float32 on the CPU; `cot(pred)` -> d_pred in that arithmetic; `masks`: the device's"""
    out = []
    for dtype in (gan_ref.F64, F32):
        pred, tapes = gan_ref.forward(spec, params, x, dtype)
        d_x, grads = gan_ref.backward(spec, params, x, tapes, masks, cot(pred), dtype)
        out.append((pred, d_x, [g for layer_grads in grads for wb in layer_grads for g in wb]))
    return out


def assert_end_to_end(what, dev, f64, cpu32, report, floor=0.0):
    """`floor`: what the yardstick is at least (see test_discriminator_loss_backward_matches_the_restatement)"""
    err_dev = float((gan_ref.t64(dev.detach().cpu().numpy()) - f64).abs().max())
    err_cpu = max(float((cpu32.to(gan_ref.F64) - f64).abs().max()), floor)
    report[what] = (err_dev, err_cpu)
    assert err_dev <= 4.0 * err_cpu, f"{what}: max |dev - f64| = {err_dev:.3e}, max |cpu32 - f64| = {err_cpu:.3e}, ratio {err_dev / max(err_cpu, 1e-300):.2f}"


def print_report(tag, report):
    worst = max(report.items(), key=lambda kv: kv[1][0] / max(kv[1][1], 1e-300))
    print(f"end to end {tag}: " + ", ".join(f"{k} {d / max(c, 1e-300):.2f}" for k, (d, c) in report.items() if k in ("pred", "d_x"))
          + f"; worst gradient ratio {worst[1][0] / max(worst[1][1], 1e-300):.2f} ({worst[0]})")


@pytest.mark.parametrize("name,B", E2E_CASES)
def test_end_to_end_error_against_float64_is_within_4x_of_torch_float32_on_the_cpu(renderer, name, B):
    spec, params, x, pdev, xdev = case(name, B)
    pred, tape = dev_forward(renderer, spec, pdev, xdev)
    d_pred = cotangent(B, len(spec.paths))
    d_x, grads = dev_backward(renderer, spec, pdev, xdev, tape, torch.tensor(d_pred, device=DEV))
    masks = gan_ref.masks_of(tape_views(spec, B, tape))
    (p64, dx64, g64), (p32, dx32, g32) = references(spec, params, x, masks, lambda pred_: d_pred)
    report = {}
    assert_end_to_end("pred", pred, p64, p32, report)
    assert_end_to_end("d_x", d_x, dx64, dx32, report)
    for i, g in enumerate(grads):
        assert_end_to_end(f"path {i // 10} layer {i % 10 // 2} {'b' if i % 2 else 'W'}", g, g64[i], g32[i], report)
    print_report(f"{name} B={B}", report)


# ---- exact properties ----------------------------------------------------------------------------------------------------------------------
def test_a_row_does_not_depend_on_its_batch_or_position(renderer):
    spec, params, x, pdev, xdev = case("pos3d", 130)
    d_pred = torch.tensor(cotangent(130, 7), device=DEV)
    pred, tape = dev_forward(renderer, spec, pdev, xdev)
    d_x, _ = dev_backward(renderer, spec, pdev, xdev, tape, d_pred, want_grads=False)
    views = tape_views(spec, 130, tape)
    perm = torch.tensor(np.random.RandomState(1).permutation(130), device=DEV)
    pred_p, tape_p = dev_forward(renderer, spec, pdev, xdev[perm].contiguous())
    d_x_p, _ = dev_backward(renderer, spec, pdev, xdev[perm].contiguous(), tape_p, d_pred[perm].contiguous(), want_grads=False)
    assert same_bytes(pred_p, pred[perm]) and same_bytes(d_x_p, d_x[perm])
    views_p, hp = tape_views(spec, 130, tape_p), perm.cpu().numpy()
    for p in range(7):
        for l in range(4):
            assert views_p[p][l].tobytes() == views[p][l][hp].tobytes(), (p, l)
    for row in (0, 63, 64, 129):                                             # first and last of a tile, the last row of the batch
        pred_1, tape_1 = dev_forward(renderer, spec, pdev, xdev[row:row + 1].contiguous())
        d_x_1, _ = dev_backward(renderer, spec, pdev, xdev[row:row + 1].contiguous(), tape_1, d_pred[row:row + 1].contiguous(), want_grads=False)
        assert same_bytes(pred_1, pred[row:row + 1]) and same_bytes(d_x_1, d_x[row:row + 1]), row
        views_1 = tape_views(spec, 1, tape_1)
        for p in range(7):
            for l in range(4):
                assert views_1[p][l].tobytes() == views[p][l][row:row + 1].tobytes(), (row, p, l)


def test_two_runs_give_the_same_bytes_and_d_x_does_not_depend_on_grads(renderer):
    spec, params, x, pdev, xdev = case("pos3d", 130)
    d_pred = torch.tensor(cotangent(130, 7), device=DEV)
    runs = []
    for _ in range(2):
        pred, tape = dev_forward(renderer, spec, pdev, xdev)
        d_x, grads = dev_backward(renderer, spec, pdev, xdev, tape, d_pred)
        runs.append([pred, tape, d_x] + grads)
    for a, b in zip(*runs):
        assert same_bytes(a, b)
    assert not any(bool((g == -7.0).all()) for g in runs[0][3:])            # every gradient was written
    d_x_alone, none = dev_backward(renderer, spec, pdev, xdev, runs[0][1], d_pred, want_grads=False)
    assert none is None and same_bytes(d_x_alone, runs[0][2])
    # a forward without a tape gives the same predictions
    pred_only, _ = dev_forward(renderer, spec, pdev, xdev, want_tape=False)
    assert same_bytes(pred_only, runs[0][0])
    # gradients alone (d_x not wanted) are the same gradients
    _, grads_alone = dev_backward(renderer, spec, pdev, xdev, runs[0][1], d_pred, want_dx=False)
    for a, b in zip(grads_alone, runs[0][3:]):
        assert same_bytes(a, b)


def test_a_row_no_path_selects_gets_a_zero_gradient(renderer):
    spec, params, x, pdev, xdev = case("toy_sparse", 33)
    pred, tape = dev_forward(renderer, spec, pdev, xdev)
    d_x, _ = dev_backward(renderer, spec, pdev, xdev, tape, torch.tensor(cotangent(33, 2), device=DEV), want_grads=False)
    d_x = d_x.cpu().numpy()
    unselected = [j for j in range(24) if j not in (0, 5, 7, 23)]
    assert not d_x[:, unselected].any() and np.all(d_x[:, [0, 5, 7, 23]] != 0)
    assert d_x[:, unselected].tobytes() == np.zeros((33, 20, 3), np.float32).tobytes()        # +0, not -0


def test_a_nan_row_stays_in_its_row(renderer):
    """pred and d_x of the other rows are the clean run's bytes.  The NaN does reach dW and db: they are sums over the rows."""
    spec, params, x, pdev, xdev = case("pos3d", 17)
    d_pred = torch.tensor(cotangent(17, 7), device=DEV)
    pred, tape = dev_forward(renderer, spec, pdev, xdev)
    d_x, _ = dev_backward(renderer, spec, pdev, xdev, tape, d_pred, want_grads=False)
    bad = xdev.clone()
    bad[5, 9, 1] = float("nan")                                              # joint 9: four paths and the full body
    pred_b, tape_b = dev_forward(renderer, spec, pdev, bad)
    d_x_b, grads_b = dev_backward(renderer, spec, pdev, bad, tape_b, d_pred)
    keep = [i for i in range(17) if i != 5]
    assert same_bytes(pred_b[keep], pred[keep]) and same_bytes(d_x_b[keep], d_x[keep])
    assert bool(torch.isnan(pred_b[5, [2, 3, 4, 5, 6]]).all()) and not bool(torch.isnan(pred_b[5, [0, 1]]).any())
    # (the NaN row's own d_x is finite: a NaN activation takes the slope, as in torch, and no product of the backward meets x)
    assert all(bool(torch.isnan(g).any()) for g in grads_b[60::2])          # every dW of the full-body path carries it


# ---- the loss --------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,label", [(7, 1.0), (256, 0.0), (257, 1.0), (7168, 0.0), (7168, 1.0)])
def test_the_loss_and_its_count_equal_the_restatement(renderer, n, label):
    rng = np.random.RandomState(n)
    pred = (label + rng.standard_normal(n) * 0.6).astype(np.float32)
    edge = np.float32([label + 0.5, label - 0.5, np.nextafter(np.float32(label + 0.5), np.float32(9)),
                       np.nextafter(np.float32(label - 0.5), np.float32(-9)), np.nextafter(np.float32(label + 0.5), np.float32(-9))])
    pred[:5] = edge[:min(5, n)]
    out = torch.full((4,), -7.0, dtype=torch.float64, device=DEV)
    d_pred = torch.full((n + 1,), -7.0, device=DEV)
    _ffi.call(renderer, "pg_disc_loss", torch.tensor(pred, device=DEV), n, label, 0.5, out, d_pred)
    torch.cuda.synchronize()
    loss, count, n_ref, d_ref = gan_ref.lsgan(pred, label, 0.5)
    out, d_pred = out.cpu().numpy(), d_pred.cpu().numpy()
    assert abs(out[0] - loss) <= 1e-12 * abs(loss) and out[1] == count and out[2] == n == n_ref and out[3] == -7.0
    assert d_pred[-1] == -7.0 and d_pred[:-1].tobytes() == d_ref.astype(np.float32).tobytes()
    # without a gradient the numbers are the same
    out2 = torch.empty(3, dtype=torch.float64, device=DEV)
    _ffi.call(renderer, "pg_disc_loss", torch.tensor(pred, device=DEV), n, label, 0.5, out2, None)
    assert out2.cpu().numpy().tobytes() == out[:3].tobytes()


# ---- the pool --------------------------------------------------------------------------------------------------------------------------------
def run_pool_trace(renderer, cap, row, calls, start=None):
    """`calls`: (items, swap, slot) in turn through pg_pool_exchange (FakePool.exchange) and through the restatement, bitwise.
    `start`: a full pool [cap,row] to begin from (cur = cap from the first call); None = an empty one"""
    pool = disc.FakePool(cap, renderer)
    ref_pool, cur = np.zeros((cap, row), np.float32), 0
    if start is not None:
        ref_pool, cur = np.array(start, dtype=np.float32).reshape(cap, row), cap
        pool.pool, pool.cur = torch.tensor(ref_pool, device=DEV), cap
    for c, (items, swap, slot) in enumerate(calls):
        got = pool.exchange(torch.tensor(items, device=DEV), swap, slot)
        want, ref_pool, cur = gan_ref.pool_exchange(ref_pool, cur, items, swap, slot)
        torch.cuda.synchronize()
        assert got.cpu().numpy().tobytes() == want.tobytes(), f"call {c}: returned rows"
        assert pool.pool.cpu().numpy().tobytes() == ref_pool.tobytes(), f"call {c}: the pool"
        assert pool.cur == cur


def test_the_small_pool_fills_crosses_full_and_takes_repeated_slots(renderer):
    rng = np.random.RandomState(2)
    items = rng.standard_normal((4, 5, 4)).astype(np.float32)
    calls = [(items[0], np.zeros(5, np.uint8), np.zeros(5, np.int32)),                        # filling
             (items[1], np.uint8([1, 1, 1, 0, 1]), np.int32([3, 5, 5, 2, 5])),                # crosses full: item 0 fills row 5, then 5 is hit twice
             (items[2], np.uint8([1, 1, 0, 1, 1]), np.int32([2, 2, 2, 2, 0])),                # full: slot 2 three times
             (items[3], np.uint8([1, 0, 1, 1, 1]), np.int32([0, 1, 0, 4, 0]))]
    run_pool_trace(renderer, 6, 4, calls)


def test_the_loop_sized_pool_equals_the_restatement(renderer):
    rng = np.random.RandomState(3)
    calls = []
    for c in range(6):                                                       # 4096 / 1024: four filling calls, then two on a full pool
        items = rng.standard_normal((1024, 72)).astype(np.float32)
        swap = (rng.uniform(size=1024) > 0.5).astype(np.uint8)
        slot = rng.randint(0, 64 if c == 5 else 4096, size=1024).astype(np.int32)           # the last call: every slot hit many times
        calls.append((items, swap, slot))
    run_pool_trace(renderer, 4096, 72, calls)
    # a pool that crosses full in the middle of a call, slots among the rows that call appended
    calls = [(rng.standard_normal((1024, 8)).astype(np.float32), (rng.uniform(size=1024) > 0.3).astype(np.uint8),
              rng.randint(0, 1536, size=1024).astype(np.int32)) for _ in range(3)]
    run_pool_trace(renderer, 1536, 8, calls)


def test_fake_pool_draws_like_the_reference(renderer):
    g = np.load(os.path.join(os.path.dirname(os.path.abspath(gan_ref.__file__)), "golden", "pose_discriminators.npz"))
    pool = disc.FakePool(6, renderer)
    np.random.seed(int(g["pool_seed"]))
    for c in range(3):
        got = pool(torch.tensor(g["pool_items"][c], device=DEV))
        assert got.cpu().numpy().tobytes() == g["pool_returned"][c].tobytes(), c
    assert pool.pool.cpu().numpy().tobytes() == g["pool_final"].tobytes()


# ---- the modules ---------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def model3d(renderer):
    m = disc.HipPos3dDiscriminator(renderer).to(DEV)
    spec, params, x, pdev, xdev = case("pos3d", 17)
    gan_ref.load_params(m, params)
    return m


def module_grads(m):
    return [None if t.grad is None else t.grad for p in range(len(m.spec.paths)) for lin in m.path_linears(p) for t in (lin.weight, lin.bias)]


def test_discriminator_loss_backward_matches_the_restatement(renderer, model3d):
    """Every parameter gradient under the end-to-end criterion, each tensor on its own.  One tensor per path has a single element:
    the gradient of layer_pred.bias = sum_b d_pred[b,p] = (sum over the real rows of (pred - 1)) / n_real + (sum over the fake rows
    of pred) / n_fake with n = rows x 7, i.e. an average of the prediction errors, at most 2 / 7 of their maximum.  A ratio of two
    single rounding errors says nothing (the float32 sum on the CPU may land next to the float64 value by luck), so for these seven
    numbers the yardstick is at least that propagated share of the CPU's own prediction error -- the error the criterion allows
    `pred` itself, carried through the linear map."""
    spec, params, x, pdev, xdev = case("pos3d", 17)
    real, fake = xdev[:9], xdev[9:]
    model3d.zero_grad()
    for t in model3d.parameters():
        t.requires_grad_(True)
    loss, real_acc, fake_acc = disc.discriminator_loss(model3d, real, fake)
    loss.backward()
    _, tape = dev_forward(renderer, spec, pdev, xdev)
    masks = gan_ref.masks_of(tape_views(spec, 17, tape))

    def cot(pred):                                                           # d loss / d pred in the arithmetic of `pred`
        d = torch.empty_like(pred)
        d[:9] = 0.5 * 2.0 * (pred[:9] - 1.0) / (9 * 7)
        d[9:] = 0.5 * 2.0 * pred[9:] / (8 * 7)
        return d
    (p64, _, g64), (p32, _, g32) = references(spec, params, x, masks, cot)
    want_loss, want_real, want_fake, _, _ = gan_ref.discriminator_loss(model3d(real).detach().cpu().numpy(), model3d(fake).detach().cpu().numpy())
    assert abs(float(loss.detach()) - want_loss) <= 1e-12 * want_loss and float(real_acc) == want_real and float(fake_acc) == want_fake
    assert loss.dtype == torch.float64 and loss.is_cuda and real_acc.is_cuda and fake_acc.is_cuda
    report = {}
    pred_share = 2.0 / 7.0 * float((p32.to(gan_ref.F64) - p64).abs().max())
    for i, g in enumerate(module_grads(model3d)):
        assert_end_to_end(f"path {i // 10} layer {i % 10 // 2} {'b' if i % 2 else 'W'}", g, g64[i], g32[i], report,
                          floor=pred_share if g.numel() == 1 else 0.0)
    print_report("discriminator_loss", report)


def test_adversarial_loss_reaches_the_input_and_skips_the_weight_gradients(renderer, model3d, monkeypatch):
    spec, params, x, pdev, xdev = case("pos3d", 17)
    model3d.zero_grad()
    for t in model3d.parameters():                                          # set_grad([model_d3d], False) of the generator step
        t.requires_grad_(False)
    seen = []
    real_call = _ffi.call

    def spy(r, name, *args):
        seen.append((name, args))
        return real_call(r, name, *args)
    monkeypatch.setattr(_ffi, "call", spy)
    fake = xdev.clone().requires_grad_(True)
    loss, real_acc, fake_acc = ganloop.generator_adversarial_loss(model3d, None, fake)
    assert real_acc is None and fake_acc is None
    assert [n for n, _ in seen] == ["pg_disc_forward", "pg_disc_loss"]      # no real pass unless the accuracies are asked for
    loss.backward()
    bwd = [a for n, a in seen if n == "pg_disc_backward"]
    assert len(bwd) == 1 and bwd[0][-1] is None and bwd[0][-2] is not None  # grads null, d_x wanted
    assert all(t.grad is None for t in model3d.parameters())
    monkeypatch.undo()
    _, tape = dev_forward(renderer, spec, pdev, xdev)
    masks = gan_ref.masks_of(tape_views(spec, 17, tape))
    (p64, dx64, _), (p32, dx32, _) = references(spec, params, x, masks, lambda pred: 0.5 * 2.0 * (pred - 1.0) / pred.numel())
    report = {}
    assert_end_to_end("d_x", fake.grad, dx64, dx32, report)
    want = gan_ref.adversarial_loss(model3d(xdev).detach().cpu().numpy())[0]
    assert abs(float(loss.detach()) - want) <= 1e-12 * want
    # with the accuracies the real pass runs, under no_grad
    loss2, real_acc, fake_acc = disc.adversarial_loss(model3d, xdev[:9], xdev[9:], accuracies=True)
    pr, pf = model3d(xdev[:9]).cpu().numpy(), model3d(xdev[9:]).cpu().numpy()
    assert float(real_acc) == gan_ref.lsgan(pr, 1.0)[1] / pr.size and float(fake_acc) == gan_ref.lsgan(pf, 0.0)[1] / pf.size
    print_report("adversarial_loss", report)


def test_discriminator_step_runs_the_loop_call_site(renderer):
    """zero_grad, pool, loss, backward, clip, Adam: the parameters move, the clipped norm is at most 1, the pool has taken the batch"""
    spec, params, x, pdev, xdev = case("toy", 33)
    m = disc.PartDiscriminator(gan_ref.toy_spec(), renderer).to(DEV)
    gan_ref.load_params(m, params)
    opt = torch.optim.Adam(m.parameters(), lr=1e-3)
    pool = disc.FakePool(30, renderer)
    before = [t.detach().clone() for t in m.parameters()]
    rng = np.random.RandomState(4)
    for _ in range(2):                                                       # the second call crosses full
        real_acc, fake_acc, loss = ganloop.discriminator_step(m, opt, xdev[:16], xdev[16:] + 0.1, pool, rng)
    assert pool.cur == 30 and 0.0 <= float(real_acc) <= 1.0 and 0.0 <= float(fake_acc) <= 1.0 and np.isfinite(float(loss))
    norm = torch.sqrt(sum((t.grad.double() ** 2).sum() for t in m.parameters()))
    assert float(norm) <= 1.0 + 1e-5
    assert all(not torch.equal(a, b) for a, b in zip(before, m.parameters()))
