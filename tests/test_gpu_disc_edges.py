"""pg_disc.hip off the shapes of the shipped specs: ragged widths, mixed paths in one launch, partial gradients, views off 16-byte
alignment, LeakyReLU's kink, refusals, and the pool and the loss on edge inputs.  tests/test_gpu_discriminators.py has the shipped
specs (widths 500 / 1000 / 20, every path of a spec alike); here one launch holds eight paths of different (width, mid)
(gan_ref.ragged3_spec / ragged2_spec), at batch sizes round the 64-row chunk of the weight gradients.

  accuracy (derived, factor 1)   forward: the layer-local criterion of tests/test_gpu_discriminators.py, unchanged.  Backward:
      gan_ref.backward_with_bound -- the float64 backward from the DEVICE's own tape and masks with an elementwise bound carried down
      the chain (its docstring has the recurrences); |dev - f64| <= bound is compared, not divided: a row of d_x that no path selects
      has a bound of 0 and must be exactly 0.  That bound is loose on d_x (five layers of absolute values), so pred and d_x also meet
      the end-to-end criterion of that file, max |dev - f64| <= 4 max |cpu32 - f64|, on tensors of 256 elements and more.
  exact   a path alone gives the bytes it gives among seven others; a row does not depend on its batch; requested gradients do not
      depend on which others are requested; views 1, 2, 3 floats off 16-byte alignment give the aligned run's bytes; the weight
      gradients are the float32 sum, in chunk order, of the gradients of the 64-row chunks; workspaces that grew do not change a
      result.
  guards  every output of every call of this file lies between sentinel elements, which must stay untouched.

The ratios measured on an MI355X are in DESIGN.md 2.16 and profiles/pose_discriminators.json."""
import ctypes as C
from types import SimpleNamespace

import numpy as np
import pytest
import torch

from posegen_amd import _ffi, discriminators as disc
from tests import gan_ref
from tests.frame_metrics_gpu import DEV, renderer  # noqa: F401 (renderer: a fixture)
from tests.test_gpu_discriminators import (assert_end_to_end, assert_layer_local, cotangent, dev_backward, dev_forward, references,
                                           run_pool_trace, same_bytes, tape_views)

pytestmark = pytest.mark.gpu
GUARD = -7.0
PAD = 4                                        # guard floats on either side (16 bytes: offset 0 stays 16-byte aligned)
SPECS = {"ragged3": gan_ref.ragged3_spec, "ragged2": gan_ref.ragged2_spec}
CASES = [("ragged3", 1), ("ragged3", 63), ("ragged3", 64), ("ragged3", 65), ("ragged3", 129), ("ragged2", 65)]
INT32_MAX = 2 ** 31 - 1


# ---- guarded calls ---------------------------------------------------------------------------------------------------------------------------
class Guards:
    """output arrays with PAD sentinel elements before and after the region that is passed; `off`: floats past 16-byte alignment"""

    def __init__(self):
        self.bufs = []

    def out(self, shape, off=0, dtype=torch.float32):
        n = int(np.prod(shape))
        buf = torch.full((n + 2 * PAD,), GUARD, dtype=dtype, device=DEV)
        self.bufs.append((buf, PAD + off, n))
        return buf[PAD + off:PAD + off + n].view(*shape)

    def check(self):
        edges = torch.cat([part for buf, at, n in self.bufs for part in (buf[:at], buf[at + n:])])
        assert bool((edges == GUARD).all()), "a sentinel beside an output was overwritten"


def placed(a, off=0):
    """a float32 input on the device as a view `off` floats past 16-byte alignment"""
    a = torch.as_tensor(np.ascontiguousarray(a, dtype=np.float32))
    buf = torch.zeros(a.numel() + 2 * PAD, device=DEV)
    v = buf[PAD + off:PAD + off + a.numel()]
    v.copy_(a.reshape(-1))
    return v.view(a.shape)


def flat(params):
    return [a for layers in params for wb in layers for a in wb]


def run(r, spec, pdev, xdev, d_pred=None, want=None, off=0, want_tape=True):
    """pg_disc_forward and, with `d_pred`, pg_disc_backward, every output between guards and written in full.  `want`: per tensor
    of `pdev` whether its gradient is asked for (the others go as NULL); None = all.  -> pred, tape, d_x, grads"""
    B, n_paths = xdev.shape[0], len(spec.paths)
    cs, tab = spec.c_spec(), disc._pointer_table(spec, pdev)
    n = C.c_int64(0)
    r._check(r.lib.pg_disc_tape_floats(C.byref(cs), B, C.byref(n)))
    g = Guards()
    o = SimpleNamespace(pred=g.out((B, n_paths), off), tape=g.out((n.value,), off) if want_tape else None, d_x=None, grads=None)
    _ffi.call(r, "pg_disc_forward", C.byref(cs), C.byref(tab), xdev, B, o.pred, o.tape)
    if d_pred is not None:
        want = [True] * len(pdev) if want is None else list(want)
        o.d_x = g.out(tuple(xdev.shape), off)
        o.grads = [g.out(tuple(p.shape), off) if w else None for p, w in zip(pdev, want)]
        gtab = disc._pointer_table(spec, o.grads)
        _ffi.call(r, "pg_disc_backward", C.byref(cs), C.byref(tab), xdev, B, o.tape, d_pred, o.d_x, C.byref(gtab))
    torch.cuda.synchronize()
    g.check()
    written = [o.pred, o.tape, o.d_x] + (o.grads or [])
    assert not any(bool((t == GUARD).any()) for t in written if t is not None), "an output element was not written"
    return o


_cases = {}


def case(r, name, B):
    """a case's inputs, its run with every gradient, the tape as host arrays and the masks it implies; made once"""
    key = (name, B)
    if key not in _cases:
        spec = SPECS[name]()
        params = gan_ref.make_params(spec, 18)
        x = gan_ref.make_inputs(spec, B, 100 + B)
        d_pred = cotangent(B, len(spec.paths))
        c = SimpleNamespace(spec=spec, params=params, x=x, d_pred=d_pred, pdev=[placed(a) for a in flat(params)], xdev=placed(x),
                            d_pred_dev=placed(d_pred))
        c.out = run(r, spec, c.pdev, c.xdev, c.d_pred_dev)
        c.views = tape_views(spec, B, c.out.tape)
        c.masks = gan_ref.masks_of(c.views)
        _cases[key] = c
    return _cases[key]


def same_run(a, b, what=""):
    """two runs' outputs byte for byte (gradients that either run did not ask for are left out)"""
    assert same_bytes(a.pred, b.pred), f"{what}: pred"
    if a.tape is not None and b.tape is not None:
        assert same_bytes(a.tape, b.tape), f"{what}: tape"
    if a.d_x is not None and b.d_x is not None:
        assert same_bytes(a.d_x, b.d_x), f"{what}: d_x"
        for i, (ga, gb) in enumerate(zip(a.grads, b.grads)):
            if ga is not None and gb is not None:
                assert same_bytes(ga, gb), f"{what}: gradient {i} (path {i // 10}, layer {i % 10 // 2}, {'b' if i % 2 else 'W'})"


def host64(t):
    return gan_ref.t64(t.detach().cpu().numpy())


def ratio_to_bound(err, bound):
    """max err / bound where the bound is positive; the comparison itself is `err <= bound`"""
    return float(torch.where(bound > 0, err / bound, torch.zeros_like(err)).max())


def assert_backward_bound(tag, spec, params, x, views, masks, d_pred, out):
    """|dev - f64| <= the carried bound, elementwise, for d_x and every gradient; -> worst ratios (d_x, dW, db)"""
    d_x, grads, e_dx, bounds = gan_ref.backward_with_bound(spec, params, x, views, masks, d_pred)
    err = (host64(out.d_x) - d_x).abs()
    assert bool((err <= e_dx).all()), f"{tag}: d_x, worst error / bound {ratio_to_bound(err, e_dx):.3f}, or a nonzero where the bound is 0"
    worst = [ratio_to_bound(err, e_dx), 0.0, 0.0]
    for p in range(len(spec.paths)):
        for l in range(5):
            for k in range(2):
                dev = out.grads[(p * 5 + l) * 2 + k]
                if dev is None:
                    continue
                err = (host64(dev) - grads[p][l][k]).abs()
                assert err.shape == bounds[p][l][k].shape
                r = ratio_to_bound(err, bounds[p][l][k])
                assert bool((err <= bounds[p][l][k]).all()), f"{tag}: path {p} layer {l} {'db' if k else 'dW'}, worst error / bound {r:.3f}"
                worst[1 + k] = max(worst[1 + k], r)
    return worst


# ---- 1. accuracy against float64 -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,B", CASES)
def test_ragged_layers_are_within_the_float32_dot_product_bound_of_the_float64_layer(renderer, name, B):
    c = case(renderer, name, B)
    worst = assert_layer_local((name, B), c.spec, c.params, c.x, c.views, c.out.pred.cpu().numpy())
    print(f"layer-local {name} B={B}: worst error / bound {worst:.3f}")


@pytest.mark.parametrize("name,B", CASES)
def test_ragged_backward_is_within_the_bound_carried_down_the_chain(renderer, name, B):
    c = case(renderer, name, B)
    dx, dw, db = assert_backward_bound((name, B), c.spec, c.params, c.x, c.views, c.masks, c.d_pred, c.out)
    print(f"backward bound {name} B={B}: worst error / bound d_x {dx:.4f}, dW {dw:.3f}, db {db:.3f}")


@pytest.mark.parametrize("name,B", [cb for cb in CASES if cb[1] > 1])
def test_ragged_pred_and_d_x_are_within_4x_of_torch_float32_on_the_cpu(renderer, name, B):
    """the end-to-end criterion of tests/test_gpu_discriminators.py with its factor, on the tensors of 256 elements and more (a
    maximum over few values says little, as that file's docstring has it): at B = 1 neither tensor is, so B = 1 is not run"""
    c = case(renderer, name, B)
    (p64, dx64, _), (p32, dx32, _) = references(c.spec, c.params, c.x, c.masks, lambda pred_: c.d_pred)
    report = {}
    for what, dev, f64, cpu32 in (("pred", c.out.pred, p64, p32), ("d_x", c.out.d_x, dx64, dx32)):
        if dev.numel() >= 256:
            assert_end_to_end(what, dev, f64, cpu32, report)
    assert report
    print(f"end to end {name} B={B}: " + ", ".join(f"{k} {d / max(e, 1e-300):.2f}" for k, (d, e) in report.items()))


# ---- 2. exact properties -------------------------------------------------------------------------------------------------------------------
def test_a_path_alone_gives_the_bytes_it_gives_among_seven_others(renderer):
    """Reduction order depends on the reduction's length alone: neither the launch's grid (sized by the widest path) nor the
    offsets into the shared workspaces may change a bit.  d_x of rows 0, 1 and 3 (selected at most once within a path) is the
    float32 sum, in path order from +0, of the one-path d_x values."""
    c = case(renderer, "ragged3", 65)
    dx_sum = np.zeros((65, 5, 3), np.float32)
    for p in range(8):
        one = gan_ref.one_path_spec(c.spec, p)
        o = run(renderer, one, c.pdev[10 * p:10 * p + 10], c.xdev, placed(c.d_pred[:, p:p + 1]))
        assert same_bytes(o.pred[:, 0], c.out.pred[:, p]), p
        for l, (mine, theirs) in enumerate(zip(tape_views(one, 65, o.tape)[0], c.views[p])):
            assert mine.tobytes() == theirs.tobytes(), (p, l)
        for i in range(10):
            assert same_bytes(o.grads[i], c.out.grads[10 * p + i]), (p, i)
        dx_sum = dx_sum + o.d_x.cpu().numpy()
        assert dx_sum.dtype == np.float32
    got = c.out.d_x.cpu().numpy()
    assert got[:, [0, 1, 3]].tobytes() == dx_sum[:, [0, 1, 3]].tobytes()


def test_a_ragged_row_does_not_depend_on_its_batch_or_position(renderer):
    c = case(renderer, "ragged3", 129)
    again = run(renderer, c.spec, c.pdev, c.xdev, c.d_pred_dev)
    same_run(again, c.out, "a second run")
    perm = np.random.RandomState(1).permutation(129)
    o = run(renderer, c.spec, c.pdev, placed(c.x[perm]), placed(c.d_pred[perm]))
    hp = torch.tensor(perm, device=DEV)
    assert same_bytes(o.pred, c.out.pred[hp]) and same_bytes(o.d_x, c.out.d_x[hp])
    for p, layers in enumerate(tape_views(c.spec, 129, o.tape)):
        for l, h in enumerate(layers):
            assert h.tobytes() == c.views[p][l][perm].tobytes(), (p, l)
    for row in (0, 63, 64, 65, 128):
        o = run(renderer, c.spec, c.pdev, placed(c.x[row:row + 1]), placed(c.d_pred[row:row + 1]))
        assert same_bytes(o.pred, c.out.pred[row:row + 1]) and same_bytes(o.d_x, c.out.d_x[row:row + 1]), row
        for p, layers in enumerate(tape_views(c.spec, 1, o.tape)):
            for l, h in enumerate(layers):
                assert h.tobytes() == c.views[p][l][row:row + 1].tobytes(), (row, p, l)


def test_weight_gradients_are_the_float32_sum_of_their_64_row_chunks_in_order(renderer):
    """include/posegen_gan.h: the rows are reduced in chunks of 64, each from a zero accumulator, the partials added in chunk
    order.  So dW over 129 rows is (dW(rows 0 .. 63) + dW(rows 64 .. 127)) + dW(row 128) in float32, bit for bit (a row's tape does
    not depend on its batch); db is a double sum and only has to stay within its bound."""
    c = case(renderer, "ragged3", 129)
    parts = [run(renderer, c.spec, c.pdev, placed(c.x[a:b]), placed(c.d_pred[a:b])) for a, b in ((0, 64), (64, 128), (128, 129))]
    for i in range(0, 80, 2):
        a, b, d = (o.grads[i].cpu().numpy() for o in parts)
        want = (a + b) + d
        assert want.dtype == np.float32 and c.out.grads[i].cpu().numpy().tobytes() == want.tobytes(), (i // 10, i % 10 // 2)


PARTIAL = {"only dW": lambda i: i % 2 == 0, "only db": lambda i: i % 2 == 1, "only path d": lambda i: i // 10 == 3,
           "only layer 1 of every path": lambda i: i % 10 < 2, "only b1 of path a": lambda i: i == 1}


@pytest.mark.parametrize("which", list(PARTIAL))
def test_requested_gradients_do_not_depend_on_the_others_being_requested(renderer, which):
    c = case(renderer, "ragged3", 65)
    want = [PARTIAL[which](i) for i in range(80)]
    o = run(renderer, c.spec, c.pdev, c.xdev, c.d_pred_dev, want=want)
    assert [g is not None for g in o.grads] == want and any(want) and not all(want)
    same_run(o, c.out, which)


def test_views_off_16_byte_alignment_give_the_aligned_bytes(renderer):
    """x, every parameter, pred, tape, d_pred, d_x and every gradient start 1, 2 and 3 floats into 16-byte-aligned buffers: every
    row then takes the scalar loads.  Paths c (width 64) and f (width 80), so that the aligned run does take the 16-byte loads."""
    full = gan_ref.ragged3_spec()
    spec = disc.PartSpec(5, 3, [full.paths[2], full.paths[5]])
    params = gan_ref.make_params(spec, 18)
    x, d_pred = gan_ref.make_inputs(spec, 65, 165), cotangent(65, 2)
    runs = []
    for off in range(4):
        pdev, xdev, dp = [placed(a, off) for a in flat(params)], placed(x, off), placed(d_pred, off)
        assert all(t.data_ptr() % 16 == 4 * off for t in pdev + [xdev, dp])
        runs.append(run(renderer, spec, pdev, xdev, dp, off=off))
        assert all(t.data_ptr() % 16 == 4 * off for t in [runs[-1].pred, runs[-1].tape, runs[-1].d_x] + runs[-1].grads)
    views = tape_views(spec, 65, runs[0].tape)
    assert_layer_local("aligned", spec, params, x, views, runs[0].pred.cpu().numpy())
    for off in (1, 2, 3):
        same_run(runs[off], runs[0], f"{off} floats off alignment")


def test_workspaces_that_grew_do_not_change_a_result(renderer):
    """B = 1, then 129, then 1 again, the forward without a tape (its activations in the handle's workspace) and the backward in the
    handle's layer-gradient buffers: the first and the third results are the same bytes"""
    seen = []
    for B in (1, 129, 1):
        c = case(renderer, "ragged3", B)
        no_tape = run(renderer, c.spec, c.pdev, c.xdev, want_tape=False)
        both = run(renderer, c.spec, c.pdev, c.xdev, c.d_pred_dev)
        assert same_bytes(no_tape.pred, both.pred), B
        same_run(both, c.out, f"B = {B}")
        seen.append((no_tape, both))
    assert same_bytes(seen[0][0].pred, seen[2][0].pred)
    same_run(seen[0][1], seen[2][1], "before and after the workspaces grew")


# ---- 3. the kink and the slope -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("slope", [0.01, 0.2, 1.0, 0.0])
def test_a_pre_activation_of_exactly_zero_takes_the_slope(renderer, slope):
    """Rows 3 and 7 of W1 and those two biases are zero, so columns 3 and 7 of h1 are +0 for every row of the batch; the backward
    takes the slope there, as torch (the reference's mask is tape > 0)."""
    spec = disc.PartSpec(5, 3, [("kink", [0, 1], 20, 8)], slope=slope)
    params = gan_ref.make_params(spec, 18)
    params[0][0][0][[3, 7], :] = 0.0
    params[0][0][1][[3, 7]] = 0.0
    x, d_pred = gan_ref.make_inputs(spec, 33, 133), cotangent(33, 1)
    o = run(renderer, spec, [placed(a) for a in flat(params)], placed(x), placed(d_pred))
    views = tape_views(spec, 33, o.tape)
    assert views[0][0][:, [3, 7]].tobytes() == np.zeros((33, 2), np.float32).tobytes()          # +0 bits
    masks = gan_ref.masks_of(views)
    assert not masks[0][0][:, [3, 7]].any()
    worst = assert_backward_bound(("kink", slope), spec, params, x, views, masks, d_pred, o)
    dw1 = o.grads[0].cpu().numpy()
    if slope != 0.0:
        assert np.all(dw1[3] != 0) and np.all(dw1[7] != 0)
    else:
        assert not dw1[3].any() and not dw1[7].any()
    assert_layer_local(("kink", slope), spec, params, x, views, o.pred.cpu().numpy())
    if slope == 1.0:                                                         # LeakyReLU(1) is the identity: a plain linear chain
        h_in, pred = gan_ref.path_input(spec, 0, gan_ref.t64(x)), o.pred.cpu().numpy()
        for l, (w, b) in enumerate(params[0]):
            w64, b64 = gan_ref.t64(w), gan_ref.t64(b)
            want = h_in @ w64.T + b64
            got = gan_ref.t64(views[0][l] if l < 4 else pred)
            bound = (w.shape[1] + 2) * gan_ref.U32 * (h_in.abs() @ w64.abs().T + b64.abs()) + gan_ref.U32 * want.abs()
            assert bool(((got - want).abs() <= bound).all()), l
            h_in = got
    print(f"kink slope={slope}: worst error / bound d_x {worst[0]:.4f}, dW {worst[1]:.3f}, db {worst[2]:.3f}")


# ---- 4. refusals write nothing -------------------------------------------------------------------------------------------------------------
def _path(cs, **fields):
    for k, v in fields.items():
        setattr(cs.path[1], k, v)


def _sel(cs, v):
    cs.path[1].sel[0] = v


def _set(**fields):
    def edit(cs):
        for k, v in fields.items():
            setattr(cs, k, v)
    return edit


# what every case is checked against in check_call / spec_fault and the entry points of pg_disc.hip: all of it precedes the first
# launch and the first allocation
REFUSED_BOTH = {
    "spec NULL": dict(null="spec"), "params NULL": dict(null="params"), "x NULL": dict(null="x"),
    "n_paths 0": dict(spec=_set(n_paths=0)), "n_paths 9": dict(spec=_set(n_paths=9)),
    "n_points 0": dict(spec=_set(n_points=0)), "n_points 25": dict(spec=_set(n_points=25)),
    "point_dim 1": dict(spec=_set(point_dim=1)), "point_dim 4": dict(spec=_set(point_dim=4)),
    "n_sel 0": dict(spec=lambda cs: _path(cs, n_sel=0)), "n_sel n_points + 1": dict(spec=lambda cs: _path(cs, n_sel=6)),
    "sel -1": dict(spec=lambda cs: _sel(cs, -1)), "sel n_points": dict(spec=lambda cs: _sel(cs, 5)),
    "width 0": dict(spec=lambda cs: _path(cs, width=0)), "width 2^20 + 1": dict(spec=lambda cs: _path(cs, width=2 ** 20 + 1)),
    "mid 0": dict(spec=lambda cs: _path(cs, mid=0)), "mid 2^20 + 1": dict(spec=lambda cs: _path(cs, mid=2 ** 20 + 1)),
    "slope NaN": dict(spec=_set(slope=float("nan"))), "slope -0.01": dict(spec=_set(slope=-0.01)), "slope +inf": dict(spec=_set(slope=float("inf"))),
    "B 0": dict(B=0), "B -1": dict(B=-1), "B 64 * 65535 + 1": dict(B=64 * 65535 + 1),
    "a weight NULL": dict(param=("w", 1, 2, None)), "a bias NULL": dict(param=("b", 0, 4, None)),
    "x odd": dict(odd="x"), "a parameter odd": dict(param=("w", 1, 0, 1)),
}
REFUSED_FORWARD = dict(REFUSED_BOTH, **{"pred NULL": dict(null="pred"), "pred odd": dict(odd="pred"), "tape odd": dict(odd="tape")})
REFUSED_BACKWARD = dict(REFUSED_BOTH, **{"tape NULL": dict(null="tape"), "d_pred NULL": dict(null="d_pred"), "tape odd": dict(odd="tape"),
                                         "d_pred odd": dict(odd="d_pred"), "d_x odd": dict(odd="d_x"), "a gradient odd": dict(grad=("b", 1, 3, 1))})


def refused_disc_call(r, fn, spec=None, B=3, null=None, odd=None, param=None, grad=None):
    """`fn` on a small two-path spec with one argument spoilt; -> (rc, the outputs, all prefilled with the sentinel)"""
    ps = disc.PartSpec(5, 3, [("p", [0, 1], 20, 8), ("q", [2], 4, 4)])
    cs = ps.c_spec()
    if spec is not None:
        spec(cs)
    params = [placed(a) for a in flat(gan_ref.make_params(ps, 1))]
    tab = disc._pointer_table(ps, params)
    outs = {"pred": torch.full((3, 2), GUARD, device=DEV), "tape": torch.full((3 * (68 + 16),), GUARD, device=DEV)}
    if fn == "pg_disc_backward":
        outs = {"d_x": torch.full((3, 5, 3), GUARD, device=DEV), "grads": [torch.full_like(p, GUARD) for p in params]}
    ins = {"x": placed(gan_ref.make_inputs(ps, 3, 1)), "tape": placed(np.ones(3 * (68 + 16))), "d_pred": placed(np.ones((3, 2)))}
    gtab = disc._pointer_table(ps, outs["grads"]) if "grads" in outs else None
    for table, edit in ((tab, param), (gtab, grad)):
        if edit is not None:
            which, p, l, delta = edit
            field = getattr(table, which)
            field[p][l] = None if delta is None else field[p][l] + delta
    arg = {"spec": C.byref(cs), "params": C.byref(tab)}
    for k in ("x", "pred", "tape", "d_pred", "d_x"):
        t = outs.get(k, ins.get(k))
        arg[k] = None if t is None else C.c_void_p(t.data_ptr() + (1 if odd == k else 0))
    if null is not None:
        arg[null] = None
    if fn == "pg_disc_forward":
        rc = r.lib.pg_disc_forward(r.handle, r._stream(), arg["spec"], arg["params"], arg["x"], B, arg["pred"], arg["tape"])
    else:
        rc = r.lib.pg_disc_backward(r.handle, r._stream(), arg["spec"], arg["params"], arg["x"], B, arg["tape"], arg["d_pred"], arg["d_x"],
                                    C.byref(gtab))
    torch.cuda.synchronize()
    return rc, [t for v in outs.values() for t in (v if isinstance(v, list) else [v])]


def assert_refused(r, fn, rc, outs, what):
    assert rc == _ffi.PG_EINVAL, what
    assert all(bool((t == GUARD).all()) for t in outs), what
    assert fn.encode() in r.lib.pg_last_error(r.handle), what


@pytest.mark.parametrize("what", list(REFUSED_FORWARD))
def test_forward_refusals_write_nothing(renderer, what):
    rc, outs = refused_disc_call(renderer, "pg_disc_forward", **REFUSED_FORWARD[what])
    assert_refused(renderer, "pg_disc_forward", rc, outs, what)


@pytest.mark.parametrize("what", list(REFUSED_BACKWARD))
def test_backward_refusals_write_nothing(renderer, what):
    rc, outs = refused_disc_call(renderer, "pg_disc_backward", **REFUSED_BACKWARD[what])
    assert_refused(renderer, "pg_disc_backward", rc, outs, what)


REFUSED_LOSS = {"pred NULL": dict(null="pred"), "out NULL": dict(null="out"), "n 0": dict(n=0), "label NaN": dict(label=float("nan")),
                "weight NaN": dict(weight=float("nan")), "out off 8-byte alignment": dict(odd=("out", 4))}


@pytest.mark.parametrize("what", list(REFUSED_LOSS))
def test_loss_refusals_write_nothing(renderer, what):
    m = REFUSED_LOSS[what]
    pred, out, d_pred = placed(np.ones(8)), torch.full((4,), GUARD, dtype=torch.float64, device=DEV), torch.full((8,), GUARD, device=DEV)
    arg = {"pred": pred.data_ptr(), "out": out.data_ptr(), "d_pred": d_pred.data_ptr()}
    if "odd" in m:
        arg[m["odd"][0]] += m["odd"][1]
    if "null" in m:
        arg[m["null"]] = None
    rc = renderer.lib.pg_disc_loss(renderer.handle, renderer._stream(), arg["pred"], m.get("n", 8), m.get("label", 1.0), m.get("weight", 0.5),
                                   arg["out"], arg["d_pred"])
    torch.cuda.synchronize()
    assert_refused(renderer, "pg_disc_loss", rc, [out, d_pred], what)


REFUSED_POOL = dict({f"{k} NULL": dict(null=k) for k in ("pool", "items", "swap", "slot", "out")},
                    **{"cap 0": dict(cap=0), "cap 2^31": dict(cap=2 ** 31), "row_floats 0": dict(row=0), "cur -1": dict(cur=-1),
                       "cur cap + 1": dict(cur=7), "n 0": dict(n=0), "n 8193": dict(n=8193)},
                    **{f"{k} misaligned": dict(odd=k) for k in ("pool", "items", "out", "slot")})


@pytest.mark.parametrize("what", list(REFUSED_POOL))
def test_pool_refusals_write_nothing(renderer, what):
    m = REFUSED_POOL[what]
    pool, out = torch.full((6, 4), GUARD, device=DEV), torch.full((5, 4), GUARD, device=DEV)
    ins = {"items": placed(np.ones((5, 4))), "swap": torch.ones(8, dtype=torch.uint8, device=DEV), "slot": torch.zeros(8, dtype=torch.int32, device=DEV)}
    arg = {k: t.data_ptr() for k, t in dict(ins, pool=pool, out=out).items()}
    if "odd" in m:
        arg[m["odd"]] += 2
    if "null" in m:
        arg[m["null"]] = None
    rc = renderer.lib.pg_pool_exchange(renderer.handle, renderer._stream(), arg["pool"], m.get("cap", 6), m.get("row", 4), m.get("cur", 6),
                                       arg["items"], m.get("n", 5), arg["swap"], arg["slot"], arg["out"])
    torch.cuda.synchronize()
    assert_refused(renderer, "pg_pool_exchange", rc, [pool, out], what)


def test_fake_pool_refuses_more_items_than_a_call_takes(renderer):
    items = torch.zeros(8193, 2, device=DEV)
    fresh = disc.FakePool(4, renderer)
    with pytest.raises((ValueError, _ffi.PgError)):
        fresh.exchange(items, np.zeros(8193, np.uint8), np.zeros(8193, np.int32))
    assert fresh.cur == 0 and fresh.pool is None
    used = disc.FakePool(4, renderer)
    used.exchange(torch.ones(3, 2, device=DEV), np.zeros(3, np.uint8), np.zeros(3, np.int32))
    before, kept = used.pool.clone(), used.pool
    with pytest.raises((ValueError, _ffi.PgError)):
        used.exchange(items, np.ones(8193, np.uint8), np.zeros(8193, np.int32))
    torch.cuda.synchronize()
    assert used.cur == 3 and used.pool is kept and torch.equal(used.pool, before)
    # the largest call passes
    assert used.exchange(items[:8192], np.zeros(8192, np.uint8), np.zeros(8192, np.int32)).shape == (8192, 2) and used.cur == 4


# ---- 5. the pool and the loss on edge inputs -----------------------------------------------------------------------------------------------
def _items(rng, n, row):
    return rng.standard_normal((n, row)).astype(np.float32)


def test_slots_outside_the_pool_are_no_swap(renderer):
    rng = np.random.RandomState(7)
    calls = [(_items(rng, 8, 4), np.uint8([1, 1, 1, 1, 1, 0, 1, 1]), np.int32([-1, 6, INT32_MAX, 2, 2, -1, 6, 5])),
             (_items(rng, 3, 4), np.uint8([1, 1, 1]), np.int32([-2 ** 31, 7, 0]))]
    run_pool_trace(renderer, 6, 4, calls, start=_items(rng, 6, 4))
    # crossing full within the call: items 0 and 1 are appended whatever their slots say
    calls = [(_items(rng, 4, 4), np.zeros(4, np.uint8), np.zeros(4, np.int32)),
             (_items(rng, 6, 4), np.ones(6, np.uint8), np.int32([-1, 6, 6, 5, INT32_MAX, 5]))]
    run_pool_trace(renderer, 6, 4, calls)


def test_the_pool_takes_one_item_and_rows_of_one_and_of_257_floats(renderer):
    rng = np.random.RandomState(8)
    one = [(_items(rng, 1, 5), np.uint8([s]), np.int32([k])) for s, k in ((0, 0), (1, 2), (1, 1), (1, 1), (0, 1), (1, 3), (1, 0), (1, 1))]
    run_pool_trace(renderer, 3, 5, one)
    for row in (1, 257):
        calls = [(_items(rng, 4, row), (rng.uniform(size=4) > 0.3).astype(np.uint8), rng.randint(0, 5, size=4).astype(np.int32)) for _ in range(4)]
        run_pool_trace(renderer, 5, row, calls)


def test_300_items_on_one_slot_and_300_items_among_rows_the_call_appended(renderer):
    rng = np.random.RandomState(9)
    run_pool_trace(renderer, 4, 3, [(_items(rng, 300, 3), np.ones(300, np.uint8), np.zeros(300, np.int32))], start=_items(rng, 4, 3))
    # cur = 0, cap = 10: items 10 .. 299 swap among the rows that items 0 .. 9 of the same call filled
    calls = [(_items(rng, 300, 3), np.ones(300, np.uint8), rng.randint(0, 10, size=300).astype(np.int32)),
             (_items(rng, 300, 3), (rng.uniform(size=300) > 0.5).astype(np.uint8), rng.randint(0, 10, size=300).astype(np.int32))]
    run_pool_trace(renderer, 10, 3, calls)
    run_pool_trace(renderer, 10, 3, calls[1:], start=_items(rng, 10, 3))      # cur == cap from the first call


def test_the_largest_pool_call_equals_the_restatement(renderer):
    rng = np.random.RandomState(10)
    calls = [(_items(rng, 8192, 3), (rng.uniform(size=8192) > 0.4).astype(np.uint8), rng.randint(-1, 66, size=8192).astype(np.int32)) for _ in range(2)]
    run_pool_trace(renderer, 64, 3, calls)


def _class(v):
    v = np.asarray(v, dtype=np.float64)
    return np.where(np.isnan(v), 3, np.where(np.isposinf(v), 2, np.where(np.isneginf(v), 1, 0)))


LOSS_EXTRAS = {"nan inf -inf 1e20": [np.nan, np.inf, -np.inf, 1e20], "1e20": [1e20, -1e20], "inf 1e20": [np.inf, 1e20], "-inf": [-np.inf], "none": []}


@pytest.mark.parametrize("weight", [0.5, 0.0, -1.0])
@pytest.mark.parametrize("extras", list(LOSS_EXTRAS))
@pytest.mark.parametrize("n", [1, 255, 256, 257, 513])
def test_the_loss_on_non_finite_predictions_and_weights_of_zero_and_below(renderer, n, extras, weight):
    """gan_ref.lsgan is the reference: the count is exact (a NaN and an infinity count as wrong), out[0] has the restatement's
    NaN / +inf / -inf class or is within 1e-12 relative, d_pred is bitwise the restatement's where that is finite and of its class
    elsewhere.  1e20 squares beyond float32 and not beyond double."""
    label = 1.0
    pred = (label + np.random.RandomState(n).standard_normal(n) * 0.6).astype(np.float32)
    extra = np.float32(LOSS_EXTRAS[extras])[:n]
    pred[n - len(extra):] = extra                                            # (n = 1: the first of the extras alone)
    out = torch.full((4,), GUARD, dtype=torch.float64, device=DEV)
    d_pred = torch.full((n + 1,), GUARD, device=DEV)
    _ffi.call(renderer, "pg_disc_loss", torch.tensor(pred, device=DEV), n, label, weight, out, d_pred)
    torch.cuda.synchronize()
    with np.errstate(all="ignore"):
        loss, count, n_ref, d_ref = gan_ref.lsgan(pred, label, weight)
        d_ref32 = d_ref.astype(np.float32)
    out, d_pred = out.cpu().numpy(), d_pred.cpu().numpy()
    assert out[1] == count and out[2] == n == n_ref and out[3] == GUARD and d_pred[-1] == GUARD
    assert count == int(np.sum(np.abs(pred[np.isfinite(pred)] - np.float32(label)) <= np.float32(0.5)))
    if np.isfinite(loss):
        assert np.isfinite(out[0]) and abs(out[0] - loss) <= 1e-12 * abs(loss)
    else:
        assert _class(out[0]) == _class(loss)
    finite = np.isfinite(d_ref)
    assert d_pred[:-1][finite].tobytes() == d_ref32[finite].tobytes()
    assert np.array_equal(_class(d_pred[:-1][~finite]), _class(d_ref[~finite]))


# ---- 6. through the module -----------------------------------------------------------------------------------------------------------------
def test_frozen_parameters_get_no_gradient_and_the_rest_get_the_same_bytes(renderer):
    """requires_grad off on all of path b and on every bias of path d: _DiscFn.backward passes those as NULL"""
    c = case(renderer, "ragged3", 65)
    m = disc.PartDiscriminator(gan_ref.ragged3_spec(), renderer).to(DEV)
    gan_ref.load_params(m, c.params)
    tensors = m._flat_params()
    frozen = [i // 10 == 1 or (i // 10 == 3 and i % 2 == 1) for i in range(80)]
    for t, f in zip(tensors, frozen):
        t.requires_grad_(not f)
    x = torch.tensor(c.x, device=DEV, requires_grad=True)
    pred = m(x)
    pred.backward(torch.tensor(c.d_pred, device=DEV))
    torch.cuda.synchronize()
    # the ABI on plain torch allocations gives the guarded run's bytes, and the module gives them too
    pdev = [torch.tensor(a, device=DEV) for a in flat(c.params)]
    pred_abi, tape = dev_forward(renderer, c.spec, pdev, x.detach())
    d_x, grads = dev_backward(renderer, c.spec, pdev, x.detach(), tape, torch.tensor(c.d_pred, device=DEV))
    assert same_bytes(pred_abi, c.out.pred) and same_bytes(d_x, c.out.d_x) and all(same_bytes(a, b) for a, b in zip(grads, c.out.grads))
    assert same_bytes(pred.detach(), c.out.pred) and same_bytes(x.grad, c.out.d_x)
    for i, (t, f) in enumerate(zip(tensors, frozen)):
        if f:
            assert t.grad is None, i
        else:
            assert same_bytes(t.grad, c.out.grads[i]), i
