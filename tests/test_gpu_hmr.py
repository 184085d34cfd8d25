"""The HMR regression head on the device (include/posegen_regressor.h, posegen_amd/regressors.py) against the float64 restatement
(tests/hmr_ref.py).

Layer-local checks, forward and backward, at every B: each product against the float64 product of the device's own operands, rebuilt
from its tape, under  |dev - f64| <= (K + 2) u (|h| |W|^T + |b|),  u = 2^-24, K the reduction length, plus one rounding for each
residual add and one for the dropout scale (hmr_ref.*_with_bound).  The backward's intermediate gradients stay inside the library, so
its chain is checked in two ways: at one row and one round every intermediate is an output (a bias gradient is the column sum of one
row), and each product is checked on the device's own operands; at every other size the float64 chain from the device's tape and
cotangents is compared under the same bounds carried down the chain to first order.  The error is compared with the bound, never
divided by it for the assertion; the worst ratios are printed (DESIGN.md 2.18 records them).

The rotation epilogue: every entry within u |R_ij| + 2^-40 of the float64 restatement at the device's own final state, on the joints
whose |a1| and |a2 perpendicular| are both >= 1e-3 |a|; degenerate joints are tested for the reference's exact zeros.

End to end, per output and gradient tensor of 256 elements and more:  max|dev - f64| / max|cpu32 - f64| <= 4, cpu32 being
`regressors.stock_forward` in float32 on the CPU under the same masks -- the yardstick of tests/test_gpu_discriminators.py."""
import copy
import ctypes as C
import math

import numpy as np
import pytest
import torch

from posegen_amd import _ffi, ganloop, regressors as reg
from tests import hmr_checks as chk
from tests import hmr_ref as ref
from tests.frame_metrics_gpu import DEV, renderer  # noqa: F401 (renderer: a fixture)

pytestmark = pytest.mark.gpu
SENT, PAD = 12345.0, 64
BATCHES = (1, 2, 15, 16, 17, 63, 64, 65, 130)
# the comparisons themselves live in tests/hmr_checks.py, where the float32 emulation on the CPU is judged by the same code
U, TINY, GRADS, EVERY, WORST = chk.U, chk.TINY, chk.GRADS, chk.EVERY, chk.WORST
_note, _within, _same, _well_conditioned, _check_forward, _check_backward = (chk.note, chk.within, chk.same, chk.well_conditioned, chk.check_forward,
                                                                             chk.check_backward)


def _guarded(n, offset=0):
    """a device array of n floats between sentinels, `offset` floats off the allocation's alignment -> (all of it, the view)"""
    full = torch.full((n + 2 * PAD + offset,), SENT, dtype=torch.float32, device=DEV)
    return full, full[PAD + offset:PAD + offset + n]


def _intact(full, n, offset=0):
    h = full.cpu().numpy()
    return bool(np.all(h[:PAD + offset] == SENT) and np.all(h[PAD + offset + n:] == SENT))


def _off(a, offset=0):
    """the array on the device, `offset` floats off 16-byte alignment"""
    a = np.ascontiguousarray(a, dtype=np.float32)
    full = torch.empty(a.size + 4 + offset, dtype=torch.float32, device=DEV)
    base = (-(full.data_ptr() // 4)) % 4
    v = full[base + offset:base + offset + a.size].view(a.shape)
    v.copy_(torch.from_numpy(a))
    return v


class Head:
    """one raw-API setting: the parameters on the device (each tensor its own allocation), xf, init and masks; every output between
    sentinels, `offset` floats off 16-byte alignment (the masks one byte off).  Whatever has no elements (the tensors, outputs,
    cotangents and gradients of a decoder without columns) goes as a null pointer, or with `dummies` as a pointer into a block of
    sentinels that must stay intact"""

    def __init__(self, renderer, spec, sd, xf, masks=None, init=None, offset=0, dummies=False):
        self.r, self.spec, self.sd, self.B, self.offset = renderer, spec, sd, int(xf.shape[0]), offset
        self.P = ref.params_of(sd)
        self.dev = {k: _off(v, offset) for k, v in self.P.items()}
        self.xf_np, self.xf = np.asarray(xf, np.float32), _off(xf, offset)
        self.init_np = np.asarray(ref.init_of(sd) if init is None else init, np.float32)
        self.init = _off(self.init_np, offset)
        self.masks_np = masks
        self.masks = None
        if masks is not None:
            full = torch.empty(masks.size + 1, dtype=torch.uint8, device=DEV)
            self.masks = full[1 if offset else 0:][:masks.size].view(masks.shape)
            self.masks.copy_(torch.from_numpy(masks))
        self.cs = spec.c_spec()
        self.tab = reg.pointer_table(_ffi.PgHmrParams(), [self.dev[k] for k in GRADS])
        self.dummy_full, self.dummy = None, None
        if dummies:
            self.dummy_full = torch.full((2 * PAD,), SENT, dtype=torch.float32, device=DEV)
            self.dummy = self.dummy_full.data_ptr() + 4 * PAD
            for k in GRADS:
                if not self.P[k].size:
                    setattr(self.tab, k, self.dummy)
        self.n_f = spec.tape_layout(self.B)[1]
        self.sizes = {"rotmat": self.B * spec.n_joints * 9, "shape": self.B * spec.n_shape, "cam": self.B * spec.n_cam}

    def forward(self, want=("rotmat", "shape", "cam")):
        s, B = self.spec, self.B
        self.tape_full, self.tape = _guarded(self.n_f, self.offset)
        bufs = {k: _guarded(n, self.offset) if (k in want and n) else (None, None) for k, n in self.sizes.items()}
        ptrs = {k: self._empty() if (k in want and not self.sizes[k]) else v for k, (_, v) in bufs.items()}
        _ffi.call(self.r, "pg_hmr_head_forward", C.byref(self.cs), C.byref(self.tab), self.xf, self.init, int(self.init_np.ndim == 2), self.masks, B,
                  self.tape, ptrs["rotmat"], ptrs["shape"], ptrs["cam"])
        torch.cuda.synchronize()
        assert _intact(self.tape_full, self.n_f, self.offset) and self._dummy_intact()
        for k, (full, _) in bufs.items():
            assert full is None or _intact(full, self.sizes[k], self.offset), k
        out = {k: None if v is None else v.cpu().numpy() for k, (_, v) in bufs.items()}
        shapes = {"rotmat": (B, s.n_joints, 3, 3), "shape": (B, s.n_shape), "cam": (B, s.n_cam)}
        out = {k: None if v is None else v.reshape(shapes[k]) for k, v in out.items()}
        out["tape"] = self.tape.cpu().numpy()
        self.out = out
        return out

    def _empty(self):
        """what stands for an array without elements: NULL, or the block of sentinels"""
        return None if self.dummy is None else C.c_void_p(self.dummy)

    def _dummy_intact(self):
        return self.dummy_full is None or bool((self.dummy_full == SENT).all())

    def arrays(self):
        """the device's tape as float64 arrays (the float32 values, exactly)"""
        t = ref.tape_arrays(self.spec, self.B, self.out["tape"])
        return {k: (v.astype(np.float64) if k == "P" else [a.astype(np.float64) for a in v]) for k, v in t.items()}

    def launch_backward(self, d_rotmat=None, d_shape=None, d_cam=None, want=EVERY):
        """the backward enqueued, nothing waited for -> what `collect_backward` reads after a synchronise (it keeps the operands alive)"""
        s, B = self.spec, self.B
        shapes = dict(s.shapes(), d_xf=(B, s.n_feat), d_init=(B, s.n_state))
        held = {k: _guarded(int(np.prod(shapes[k])), self.offset) for k in want if int(np.prod(shapes[k]))}
        self.held = held
        gtab = reg.pointer_table(_ffi.PgHmrGrads(), [held[k][1] if k in held else None for k in GRADS])
        if self.dummy is not None:
            for k in GRADS:
                if k in want and not int(np.prod(shapes[k])):
                    setattr(gtab, k, self.dummy)
        cots = [None if c is None else (_off(c, self.offset) if np.asarray(c).size else self._empty()) for c in (d_rotmat, d_shape, d_cam)]
        _ffi.call(self.r, "pg_hmr_head_backward", C.byref(self.cs), C.byref(self.tab), self.xf, self.masks, B, self.tape, cots[0], cots[1], cots[2],
                  C.byref(gtab) if any(k in held for k in GRADS) else None, held["d_xf"][1] if "d_xf" in held else None,
                  held["d_init"][1] if "d_init" in held else None)
        return held, shapes, cots

    def collect_backward(self, launched):
        held, shapes, _ = launched
        assert self._dummy_intact()
        out = {}
        for k, (full, view) in held.items():
            assert _intact(full, view.numel(), self.offset), k
            out[k] = view.cpu().numpy().reshape(shapes[k])
        return out

    def backward(self, d_rotmat=None, d_shape=None, d_cam=None, want=EVERY):
        """cotangents: arrays or None (a null pointer) -> {name: gradient} for the names in `want`"""
        launched = self.launch_backward(d_rotmat, d_shape, d_cam, want)
        torch.cuda.synchronize()
        return self.collect_backward(launched)


def _inputs(spec, B, seed, training=True, per_row=False):
    rng = np.random.RandomState(seed)
    xf = rng.standard_normal((B, spec.n_feat)).astype(np.float32)
    masks = ref.make_masks(spec, B, seed + 1) if training else None
    init = rng.standard_normal((B, spec.n_state)).astype(np.float32) if per_row else None
    return xf, masks, init


def _cotangents(spec, B, seed):
    rng = np.random.RandomState(seed)
    return (rng.standard_normal((B, spec.n_joints, 3, 3)).astype(np.float32), rng.standard_normal((B, spec.n_shape)).astype(np.float32),
            rng.standard_normal((B, spec.n_cam)).astype(np.float32))


@pytest.mark.parametrize("B", BATCHES)
def test_layer_local_checks_on_the_ragged_toy_spec(renderer, B):
    spec = ref.toy_spec()
    sd = ref.make_state_dict(spec, 61)
    xf, masks, _ = _inputs(spec, B, 100 + B)
    # on the CPU restatement at least 90 % of the joints are well conditioned (here: all but a few in a thousand)
    cpu = ref.forward(ref.params_of(sd), xf, ref.init_of(sd), spec, masks)
    assert np.mean(_well_conditioned(spec, cpu["s"][-1])) >= 0.9
    run = Head(renderer, spec, sd, xf, masks, offset=B % 4)
    run.forward()
    _, well = _check_forward(run, "toy train")
    assert np.mean(well) >= 0.9
    _check_backward(run, _cotangents(spec, B, 200 + B), "toy train")
    ev = Head(renderer, spec, sd, xf, None, init=_inputs(spec, B, 300 + B, per_row=True)[2])
    ev.forward()
    _check_forward(ev, "toy eval")
    _check_backward(ev, _cotangents(spec, B, 400 + B), "toy eval")


@pytest.mark.parametrize("B", (17, 130))
def test_layer_local_checks_on_the_shipped_spec(renderer, B):
    spec = ref.shipped_spec()
    sd = ref.make_state_dict(spec, 62)
    xf, masks, _ = _inputs(spec, B, 500 + B)
    run = Head(renderer, spec, sd, xf, masks)
    run.forward()
    _, well = _check_forward(run, "shipped train")
    assert np.mean(well) >= 0.9
    _check_backward(run, _cotangents(spec, B, 600 + B), "shipped train")


@pytest.mark.parametrize("n_iter", (1, 8))
def test_one_round_and_eight_rounds(renderer, n_iter):
    spec = ref.toy_spec(n_iter, p_drop=0.25)
    sd = ref.make_state_dict(spec, 63)
    xf, masks, init = _inputs(spec, 17, 700 + n_iter, per_row=True)
    run = Head(renderer, spec, sd, xf, masks, init=init, offset=3)
    run.forward()
    _check_forward(run, f"toy {n_iter} rounds")
    _check_backward(run, _cotangents(spec, 17, 710 + n_iter), f"toy {n_iter} rounds")


def test_every_backward_product_on_the_devices_own_operands_at_one_row_and_one_round(renderer):
    _one_row_products(renderer, ref.toy_spec(1), "one row")


def _bias_row(spec, g):
    """the decoders' bias gradients side by side [1,S] (an empty decoder has none)"""
    return np.concatenate([g[k] if k in g else np.zeros(0) for k in ("decpose_b", "decshape_b", "deccam_b")])[None]


def _one_row_products(renderer, spec, tag, seed=720):
    """B = 1 and n_iter = 1: the decoders' bias gradients are d_s_1, fc2's is dz2, fc1's is dz1 -- column sums of one row in double,
    rounded once, are that row -- so every product of the chain is checked against float64 on the device's own operands."""
    assert spec.n_iter == 1
    sd = ref.make_state_dict(spec, 64)
    xf, masks, init = _inputs(spec, 1, seed, per_row=True)
    run = Head(renderer, spec, sd, xf, masks, init=init)
    run.forward()
    t = run.arrays()
    cots = _cotangents(spec, 1, seed + 1)
    g = {k: v.astype(np.float64) for k, v in run.backward(*cots).items()}
    P, F_ = run.P, spec.n_feat
    scale = ref.drop_scale(spec.p_drop)
    Wd, _ = ref.decoder_matrix(P)
    W1, W2 = np.asarray(P["fc1_w"], np.float64), np.asarray(P["fc2_w"], np.float64)
    ds1 = _bias_row(spec, g)
    want = ref.final_cotangent(spec, t["s"][1], *[np.asarray(c, np.float64) for c in cots])
    bound = U * np.abs(want) + 2.0 ** -40 * np.max(np.abs(want))
    bound[:, spec.n_pose:] = 0.0
    _within(f"{tag} d_s (rot6d backward)", ds1, want, bound)
    dz2, dz1 = g["fc2_b"][None], g["fc1_b"][None]
    v, e = ref.data_step_with_bound(ds1, None, Wd, scale, masks[0, 1])
    _within(f"{tag} dz2", dz2, v, e)
    v, e = ref.data_step_with_bound(dz2, None, W2, scale, masks[0, 0])
    _within(f"{tag} dz1", dz1, v, e)
    v, e = ref.data_step_with_bound(dz1, None, W1[:, F_:], scale, None, add=ds1)
    _within(f"{tag} d_init", g["d_init"], v, e)
    v, e = ref.data_step_with_bound(dz1, None, W1[:, :F_], scale, None)
    _within(f"{tag} d_xf", g["d_xf"], v, e)
    # the weight gradients of one row are outer products: one rounding each (held to the general (R + 2) u with R = 1)
    for name, a, b in (("fc2_w", dz2, t["h1"][0]), ("fc1_w", dz1, np.concatenate([run.xf_np.astype(np.float64), t["s"][0]], 1)),
                       ("decpose_w", ds1[:, :spec.n_pose], t["h2"][0]), ("decshape_w", ds1[:, spec.n_pose:spec.n_pose + spec.n_shape], t["h2"][0]),
                       ("deccam_w", ds1[:, spec.n_pose + spec.n_shape:], t["h2"][0])):
        if name in g:                                                          # (an empty decoder has no gradient)
            _within(f"{tag} {name}", g[name], a.T @ b, 3 * U * np.abs(a.T @ b))
    assert set(g) == {k for k, shape in dict(spec.shapes(), d_xf=(1,), d_init=(1,)).items() if int(np.prod(shape))}


def test_weight_gradients_on_the_devices_own_operands_at_one_round(renderer):
    _weight_gradients_on_own_operands(renderer, ref.toy_spec(1), 70)


def _weight_gradients_on_own_operands(renderer, spec, B):
    """n_iter = 1, B = 70 (a full chunk of 64 rows and six more): every row run alone gives that row's d_s_1, dz2 and dz1 as its bias
    gradients, and its d_xf, d_init and tape are the bytes the row has inside the batch; the batch's weight gradients are then
    checked against float64 products of those operands over K = B rows."""
    assert spec.n_iter == 1
    sd = ref.make_state_dict(spec, 77)
    xf, masks, init = _inputs(spec, B, 740, per_row=True)
    cots = _cotangents(spec, B, 741)
    whole = Head(renderer, spec, sd, xf, masks, init=init)
    whole.forward()
    t = whole.arrays()
    g = whole.backward(*cots)
    rows = {k: [] for k in ("ds1", "dz2", "dz1")}
    for b in range(B):
        one = Head(renderer, spec, sd, xf[b:b + 1], masks[:, :, b:b + 1], init=init[b:b + 1])
        one.forward()
        t1 = one.arrays()
        assert _same(t1["P"][0], t["P"][b]) and all(_same(t1[k][i][0], t[k][i][b]) for k in ("s", "h1", "h2") for i in range(len(t[k]))), b
        g1 = one.backward(*[c[b:b + 1] for c in cots])
        assert _same(g1["d_xf"][0], g["d_xf"][b]) and _same(g1["d_init"][0], g["d_init"][b]), b
        rows["ds1"].append(_bias_row(spec, g1)[0])
        rows["dz2"].append(g1["fc2_b"])
        rows["dz1"].append(g1["fc1_b"])
    ds1, dz2, dz1 = (np.stack(rows[k]).astype(np.float64) for k in ("ds1", "dz2", "dz1"))
    a, b_ = spec.n_pose, spec.n_pose + spec.n_shape

    def product(name, A, Bm):
        assert (name in g) == bool(A.shape[1])                                 # (an empty decoder has no gradient)
        if name in g:
            _within(f"own operands {name}", g[name], A.T @ Bm, (B + 2) * U * (np.abs(A).T @ np.abs(Bm)))

    def column_sums(name, A):
        assert (name in g) == bool(A.shape[1])
        if name in g:
            _within(f"own operands {name}", g[name], A.sum(0), U * np.abs(A.sum(0)) + ref.DOUBLE_SUM * np.abs(A).sum(0))
    product("fc2_w", dz2, t["h1"][0])
    product("fc1_w", dz1, np.concatenate([xf.astype(np.float64), t["s"][0]], 1))
    product("decpose_w", ds1[:, :a], t["h2"][0])
    product("decshape_w", ds1[:, a:b_], t["h2"][0])
    product("deccam_w", ds1[:, b_:], t["h2"][0])
    column_sums("fc2_b", dz2)
    column_sums("fc1_b", dz1)
    column_sums("decpose_b", ds1[:, :a])
    column_sums("decshape_b", ds1[:, a:b_])
    column_sums("deccam_b", ds1[:, b_:])


def test_degenerate_joints_give_the_references_zeros(renderer):
    """decoders that are zero leave the state at its per-row init bit for bit, so the epilogue sees exactly these six numbers"""
    spec = ref.toy_spec(1)
    sd = ref.make_state_dict(spec, 65)
    for k in ("decpose", "decshape", "deccam"):
        sd[f"{k}.weight"][:] = 0.0
        sd[f"{k}.bias"][:] = 0.0
    x = np.zeros((4, spec.n_state), np.float32)
    x[:, :] = np.random.RandomState(66).standard_normal(x.shape)
    x[0, 0:6] = [0.0, 0.0, 0.0, 2.0, 0.0, 0.0]                                 # joint 0 of row 0: a1 = 0
    x[1, 6:12] = [1.0, 2.0, 2.0, 4.0, 2.0, 4.0]                                # joint 1 of row 1: a2 = 2 a1 exactly
    x[2, 12:18] = 0.0                                                          # joint 2 of row 2: all six zero
    run = Head(renderer, spec, sd, _inputs(spec, 4, 730)[0], None, init=x)
    out = run.forward()
    assert _same(run.arrays()["s"][1].astype(np.float32), x)
    R, R64 = out["rotmat"], ref.rot6d(x[:, :spec.n_pose].astype(np.float64).reshape(4, 3, 6))
    assert not np.isnan(R).any()
    assert _same(R[0, 0], np.array([[0.0, 0.0, 0.0], [0.0, 1.0, 0.0], [0.0, 0.0, 0.0]], np.float32))
    # a2 parallel to a1: a2 - (b1 . a2) b1 is zero up to double rounding (a few 2^-53 |a2| < 4e-15), which the clamp divides by 1e-12
    assert np.all(np.abs(R[1, 1][:, 1:]) <= 4e-3) and np.allclose(R[1, 1][:, 0], np.array([1.0, 2.0, 2.0]) / 3.0, rtol=2 * U)
    assert np.all(R[2, 2] == 0.0)
    well = _well_conditioned(spec, x)
    assert not well[0, 0] and not well[1, 1] and not well[2, 2] and well.sum() == 9
    _within("degenerate rows' other joints", R[well], R64[well], U * np.abs(R64[well]) + 2.0 ** -40)
    # and the backward there is finite where the reference's is: a1 = 0 passes g / 1e-12
    g = run.backward(*_cotangents(spec, 4, 731), want=("d_init",))["d_init"]
    want = ref.final_cotangent(spec, x, *[np.asarray(c, np.float64) for c in _cotangents(spec, 4, 731)])
    assert np.all(np.isfinite(g[0, :6][np.abs(want[0, :6]) < 1e30]))
    assert np.allclose(g[0, 0:6:2], want[0, 0:6:2].astype(np.float32), rtol=1e-5)


# ---- end to end -------------------------------------------------------------------------------------------------------------------------------
def _module(spec, sd, renderer=None, device="cpu", dtype=torch.float32):
    head = reg.HipHMRHead(spec.n_feat, spec.n_hidden, spec.n_joints, spec.n_shape, spec.n_cam, spec.p_drop, renderer=renderer)
    head.load_state_dict({k: torch.as_tensor(v) for k, v in sd.items()}, strict=True)
    return head.to(device=device, dtype=dtype)


def _ratio_rule(name, dev, f64, cpu32, slack=4.0):
    num, den = float(np.max(np.abs(np.asarray(dev, np.float64) - f64))), float(np.max(np.abs(np.asarray(cpu32, np.float64) - f64)))
    print(f"RATIO end to end {name}: {num:.3e} / {den:.3e} = {num / den if den else math.inf:.3f}")
    assert num <= slack * den, name


@pytest.mark.parametrize("which,B,per_row", [("toy", 65, True), ("toy", 130, False), ("shipped", 17, False)])
def test_the_module_against_stock_forward_in_float32_on_the_cpu(renderer, which, B, per_row):
    _end_to_end(renderer, ref.toy_spec() if which == "toy" else ref.shipped_spec(), which, B, per_row, 7)


def _end_to_end(renderer, spec, which, B, per_row, at_least):
    """the module and `stock_forward` in float32 on the CPU against the float64 restatement, per tensor of 256 elements and more (at
    least `at_least` of them)"""
    sd = ref.make_state_dict(spec, 67)
    xf, masks, init = _inputs(spec, B, 800 + B, per_row=per_row)
    cots = _cotangents(spec, B, 801 + B)
    a, b = spec.n_pose, spec.n_pose + spec.n_shape
    results = []
    for device, fn in ((DEV, None), ("cpu", reg.stock_forward)):
        head = _module(spec, sd, renderer, device).train()
        xt = torch.tensor(xf, device=device, requires_grad=True)
        kw, it = {}, None
        if per_row:
            it = torch.tensor(init, device=device, requires_grad=True)
            kw = {"init_pose": it[:, :a], "init_shape": it[:, a:b], "init_cam": it[:, b:]}
        kw["n_iter"] = spec.n_iter
        outs = head(xt, masks=torch.from_numpy(masks), **kw) if fn is None else fn(head, xt, masks=masks, **kw)
        torch.autograd.backward(outs, [torch.tensor(c, device=device) for c in cots])
        res = {"rotmat": outs[0], "shape": outs[1], "cam": outs[2], "d_xf": xt.grad}
        if per_row:
            res["d_init"] = it.grad
        for lin in ref.LINEARS:
            res[f"{lin}_w"], res[f"{lin}_b"] = getattr(head, lin).weight.grad, getattr(head, lin).bias.grad
        results.append({k: v.detach().cpu().numpy() for k, v in res.items()})
    dev, cpu32 = results
    P = ref.params_of(sd)
    f64 = ref.forward(P, xf, ref.init_of(sd) if init is None else init, spec, masks)
    g64 = ref.backward(P, xf, spec, masks, f64, *[np.asarray(c, np.float64) for c in cots])
    f64.update(g64)
    checked = 0
    for k in dev:
        assert dev[k].shape == cpu32[k].shape == f64[k].shape and dev[k].dtype == np.float32, k
        if dev[k].size >= 256:
            _ratio_rule(f"{which} B={B} {k}", dev[k], f64[k], cpu32[k])
            checked += 1
    assert checked >= at_least


# ---- exactness --------------------------------------------------------------------------------------------------------------------------------
def _all_results(run, cots):
    out = dict(run.forward())
    out.update(run.backward(*cots))
    return out


def test_two_calls_give_the_same_bytes(renderer):
    spec = ref.toy_spec()
    sd = ref.make_state_dict(spec, 68)
    xf, masks, _ = _inputs(spec, 130, 900)
    cots = _cotangents(spec, 130, 901)
    run = Head(renderer, spec, sd, xf, masks)
    first, second = _all_results(run, cots), _all_results(run, cots)
    for k in first:
        assert _same(first[k], second[k]), k


def test_an_eval_row_does_not_depend_on_the_batch_or_its_position(renderer):
    spec = ref.toy_spec()
    sd = ref.make_state_dict(spec, 69)
    xf, _, _ = _inputs(spec, 130, 910, training=False)
    whole = Head(renderer, spec, sd, xf)
    whole.forward()
    tw = ref.tape_arrays(spec, 130, whole.out["tape"])
    for row in (0, 15, 77, 129):
        one = Head(renderer, spec, sd, xf[row:row + 1])
        one.forward()
        t1 = ref.tape_arrays(spec, 1, one.out["tape"])
        assert _same(t1["P"][0], tw["P"][row])
        for k in ("s", "h1", "h2"):
            for a, b in zip(t1[k], tw[k]):
                assert _same(a[0], b[row]), (k, row)
        for k in ("rotmat", "shape", "cam"):
            assert _same(one.out[k][0], whole.out[k][row]), (k, row)


def test_a_nan_row_stays_in_its_row(renderer):
    spec = ref.toy_spec()
    sd = ref.make_state_dict(spec, 70)
    xf, masks, _ = _inputs(spec, 37, 920)
    clean = Head(renderer, spec, sd, xf, masks)
    clean.forward()
    bad = xf.copy()
    bad[20, 3] = np.nan
    dirty = Head(renderer, spec, sd, bad, masks)
    dirty.forward()
    keep = np.arange(37) != 20
    tc, td = ref.tape_arrays(spec, 37, clean.out["tape"]), ref.tape_arrays(spec, 37, dirty.out["tape"])
    assert _same(tc["P"][keep], td["P"][keep]) and np.all(np.isnan(td["P"][20]))
    for k in ("s", "h1", "h2"):
        for a, b in zip(tc[k], td[k]):
            assert _same(a[keep], b[keep]), k
    for k in ("rotmat", "shape", "cam"):
        assert _same(clean.out[k][keep], dirty.out[k][keep]), k
    assert np.all(np.isnan(dirty.out["shape"][20])) and np.all(np.isnan(dirty.out["rotmat"][20]))


def test_no_dropout_with_all_ones_masks_is_eval_mode(renderer):
    spec = ref.toy_spec(p_drop=0.0)
    sd = ref.make_state_dict(spec, 71)
    xf, _, _ = _inputs(spec, 17, 930, training=False)
    cots = _cotangents(spec, 17, 931)
    ev = _all_results(Head(renderer, spec, sd, xf), cots)
    ones = _all_results(Head(renderer, spec, sd, xf, np.ones((spec.n_iter, 2, 17, spec.n_hidden), np.uint8)), cots)
    for k in ev:
        assert _same(ev[k], ones[k]), k


def test_a_round_whose_masks_are_all_zero_adds_the_decoders_biases(renderer):
    spec = ref.toy_spec()
    sd = ref.make_state_dict(spec, 72)
    xf, masks, _ = _inputs(spec, 17, 940)
    masks[1] = 0
    run = Head(renderer, spec, sd, xf, masks)
    run.forward()
    t = ref.tape_arrays(spec, 17, run.out["tape"])
    _, bd = ref.decoder_matrix(run.P)
    assert _same(t["s"][2], t["s"][1] + bd.astype(np.float32)[None])             # one float32 add per element
    assert np.all(t["h1"][1] == 0.0) and np.all(t["h2"][1] == 0.0) and not np.any(np.signbit(t["h2"][1]))
    g = run.backward(*_cotangents(spec, 17, 941))
    assert np.all(np.isfinite(g["fc1_w"]))


def test_a_shared_init_and_the_same_values_per_row_give_the_same_bytes(renderer):
    spec = ref.toy_spec()
    sd = ref.make_state_dict(spec, 73)
    xf, masks, _ = _inputs(spec, 33, 950)
    cots = _cotangents(spec, 33, 951)
    shared = _all_results(Head(renderer, spec, sd, xf, masks), cots)
    rows = _all_results(Head(renderer, spec, sd, xf, masks, init=np.tile(ref.init_of(sd)[None], (33, 1))), cots)
    for k in shared:
        assert _same(shared[k], rows[k]), k


# ---- null pointers ------------------------------------------------------------------------------------------------------------------------------
def test_every_single_null_leaves_the_other_results_unchanged(renderer):
    spec = ref.toy_spec()
    sd = ref.make_state_dict(spec, 74)
    B = 17
    xf, masks, init = _inputs(spec, B, 960, per_row=True)
    cots = _cotangents(spec, B, 961)
    base_run = Head(renderer, spec, sd, xf, masks, init=init)
    base = _all_results(base_run, cots)
    n = 0
    for i, out in enumerate(("rotmat", "shape", "cam")):
        run = Head(renderer, spec, sd, xf, masks, init=init, offset=1 + i % 3)
        got = run.forward(want=tuple(k for k in ("rotmat", "shape", "cam") if k != out))
        assert got[out] is None
        for k in ("tape", "rotmat", "shape", "cam"):
            assert k == out or _same(got[k], base[k]), (out, k)
        n += 1
    for i, name in enumerate(EVERY):
        run = Head(renderer, spec, sd, xf, masks, init=init, offset=1 + i % 3)
        run.forward()
        got = run.backward(*cots, want=tuple(k for k in EVERY if k != name))
        assert name not in got and len(got) == len(EVERY) - 1
        for k, v in got.items():
            assert _same(v, base[k]), (name, k)
        n += 1
    # a null cotangent is a zero cotangent
    for i in range(3):
        run = Head(renderer, spec, sd, xf, masks, init=init, offset=1 + i % 3)
        run.forward()
        with_null = run.backward(*[None if j == i else c for j, c in enumerate(cots)])
        with_zero = run.backward(*[np.zeros_like(c) if j == i else c for j, c in enumerate(cots)])
        for k in with_zero:
            assert _same(with_null[k], with_zero[k]), (i, k)
        n += 1
    # grads = NULL altogether
    base_run.forward()
    got = base_run.backward(*cots, want=("d_xf", "d_init"))
    assert _same(got["d_xf"], base["d_xf"]) and _same(got["d_init"], base["d_init"])
    assert n == 3 + len(EVERY) + 3


# ---- refusals ---------------------------------------------------------------------------------------------------------------------------------
def _p(t, byte_offset=0):
    return None if t is None else C.c_void_p(t.data_ptr() + byte_offset)


def test_every_refusal_leaves_the_outputs_untouched(renderer):
    spec = ref.toy_spec()
    sd = ref.make_state_dict(spec, 75)
    B = 5
    xf, masks, _ = _inputs(spec, B, 970)
    run = Head(renderer, spec, sd, xf, masks)
    run.forward()
    good_tape = run.tape
    lib, h, st = renderer.lib, renderer.handle, renderer._stream()
    outs = {k: torch.full((n,), SENT, device=DEV) for k, n in (("tape", run.n_f), ("rotmat", B * 27), ("shape", B * 5), ("cam", B * 3), ("d_xf", B * 37),
                                                              ("d_init", B * 26), ("g", 50 * 63))}
    cots = [_off(c) for c in _cotangents(spec, B, 971)]

    def fwd(**kw):
        a = dict(h=h, spec=run.cs, tab=run.tab, xf=_p(run.xf), init=_p(run.init), per_row=0, masks=_p(run.masks), B=B, tape=_p(outs["tape"]),
                 rotmat=_p(outs["rotmat"]), shape=_p(outs["shape"]), cam=_p(outs["cam"]))
        a.update(kw)
        return lib.pg_hmr_head_forward(a["h"], st, None if a["spec"] is None else C.byref(a["spec"]), None if a["tab"] is None else C.byref(a["tab"]),
                                       a["xf"], a["init"], a["per_row"], a["masks"], a["B"], a["tape"], a["rotmat"], a["shape"], a["cam"])

    def bwd(**kw):
        gt = _ffi.PgHmrGrads()
        gt.fc1_w = outs["g"].data_ptr()
        a = dict(h=h, spec=run.cs, tab=run.tab, xf=_p(run.xf), masks=_p(run.masks), B=B, tape=_p(good_tape), d_rotmat=_p(cots[0]), d_shape=_p(cots[1]),
                 d_cam=_p(cots[2]), grads=gt, d_xf=_p(outs["d_xf"]), d_init=_p(outs["d_init"]))
        a.update(kw)
        return lib.pg_hmr_head_backward(a["h"], st, None if a["spec"] is None else C.byref(a["spec"]), None if a["tab"] is None else C.byref(a["tab"]),
                                        a["xf"], a["masks"], a["B"], a["tape"], a["d_rotmat"], a["d_shape"], a["d_cam"],
                                        None if a["grads"] is None else C.byref(a["grads"]), a["d_xf"], a["d_init"])

    def respec(**kw):
        s = spec.c_spec()
        for k, v in kw.items():
            setattr(s, k, v)
        return s

    def retab(**kw):
        t = reg.pointer_table(_ffi.PgHmrParams(), [run.dev[k] for k in GRADS])
        for k, v in kw.items():
            setattr(t, k, v)
        return t
    bad_specs = [respec(**{k: v}) for k, vs in (("n_feat", (0, 4097)), ("n_hidden", (0, 2049)), ("n_joints", (0, 65)), ("n_shape", (-1, 65)),
                                               ("n_cam", (-1, 17)), ("n_iter", (0, 9)), ("p_drop", (float("nan"), float("inf"), 1.0, -0.125)))
                 for v in vs]
    assert len(bad_specs) == 16
    both = [dict(spec=None), dict(tab=None), dict(xf=None), dict(tape=None), dict(B=0), dict(B=-3), dict(B=_ffi.PG_HMR_MAX_ROWS + 1), dict(h=None),
            dict(xf=_p(run.xf, 2)), dict(tab=retab(fc2_w=None)), dict(tab=retab(deccam_b=None)), dict(tab=retab(fc1_w=run.dev["fc1_w"].data_ptr() + 1))]
    both += [dict(spec=s) for s in bad_specs]
    fwd_only = [dict(init=None), dict(init=_p(run.init, 2)), dict(tape=_p(outs["tape"], 2)), dict(rotmat=_p(outs["rotmat"], 1)),
                dict(shape=_p(outs["shape"], 2)), dict(cam=_p(outs["cam"], 3))]
    bad_g = _ffi.PgHmrGrads()
    bad_g.fc2_b = outs["g"].data_ptr() + 2
    bwd_only = [dict(d_rotmat=None, d_shape=None, d_cam=None), dict(tape=_p(good_tape, 2)), dict(d_rotmat=_p(cots[0], 2)), dict(d_xf=_p(outs["d_xf"], 2)),
                dict(d_init=_p(outs["d_init"], 1)), dict(grads=bad_g)]
    assert fwd() == 0 and bwd() == 0                                            # the table's own arguments are good ones
    torch.cuda.synchronize()
    for o in outs.values():
        o.fill_(SENT)
    torch.cuda.synchronize()
    for case in both + fwd_only:
        assert fwd(**case) == _ffi.PG_EINVAL, ("forward", case)
    for case in both + bwd_only:
        assert bwd(**case) == _ffi.PG_EINVAL, ("backward", case)
    torch.cuda.synchronize()
    for k, o in outs.items():
        assert bool((o == SENT).all()), k
    msg = lib.pg_last_error(h).decode()
    assert "pg_hmr_head_backward" in msg


# ---- the modules --------------------------------------------------------------------------------------------------------------------------------
def test_the_module_loads_a_state_dict_and_equals_the_raw_calls(renderer):
    spec = ref.toy_spec()
    sd = ref.make_state_dict(spec, 76)
    B = 17
    xf, masks, _ = _inputs(spec, B, 980)
    cots = _cotangents(spec, B, 981)
    raw = _all_results(Head(renderer, spec, sd, xf, masks), cots)
    head = _module(spec, sd, renderer, DEV).train()
    again = _module(spec, ref.make_state_dict(spec, 99), renderer, DEV)
    again.load_state_dict(head.state_dict(), strict=True)
    for k, v in head.state_dict().items():
        assert _same(v.cpu().numpy(), again.state_dict()[k].cpu().numpy()) and _same(v.cpu().numpy(), sd[k]), k
    xt = torch.tensor(xf, device=DEV, requires_grad=True)
    outs = again.train()(xt, masks=torch.from_numpy(masks))
    torch.autograd.backward(outs, [torch.tensor(c, device=DEV) for c in cots])
    for k, o in zip(("rotmat", "shape", "cam"), outs):
        assert _same(o.detach().cpu().numpy(), raw[k]), k
    assert _same(xt.grad.cpu().numpy(), raw["d_xf"])
    for lin in ref.LINEARS:
        assert _same(getattr(again, lin).weight.grad.cpu().numpy(), raw[f"{lin}_w"]) and _same(getattr(again, lin).bias.grad.cpu().numpy(), raw[f"{lin}_b"])
    # without masks= a training-mode call draws its own and an eval-mode call has none
    a, b = again(xt.detach())[1], again(xt.detach())[1]
    assert not torch.equal(a, b)
    again.eval()
    a, b = again(xt.detach())[1], again(xt.detach())[1]
    ev = Head(renderer, spec, sd, xf)
    assert torch.equal(a, b) and _same(a.detach().cpu().numpy(), ev.forward()["shape"])
    with pytest.raises(ValueError, match="masks"):
        again(xt.detach(), masks=torch.ones(3, 2, B + 1, spec.n_hidden))


class _StandIn(torch.nn.Module):
    """the attribute names of the reference's HMR around a one-conv trunk; the head is the shipped one's shape in small"""

    def __init__(self, n_feat=16, n_hidden=40):
        super().__init__()
        self.conv1 = torch.nn.Conv2d(3, n_feat, 3, stride=2)
        self.bn1, self.relu, self.maxpool = torch.nn.Identity(), torch.nn.ReLU(), torch.nn.Identity()
        self.layer1, self.layer2, self.layer3, self.layer4 = (torch.nn.Identity() for _ in range(4))
        self.avgpool = torch.nn.AdaptiveAvgPool2d(1)
        self.fc1, self.drop1 = torch.nn.Linear(n_feat + 157, n_hidden), torch.nn.Dropout()
        self.fc2, self.drop2 = torch.nn.Linear(n_hidden, n_hidden), torch.nn.Dropout()
        self.decpose, self.decshape, self.deccam = torch.nn.Linear(n_hidden, 144), torch.nn.Linear(n_hidden, 10), torch.nn.Linear(n_hidden, 3)
        g = torch.Generator().manual_seed(5)
        for k, n in (("init_pose", 144), ("init_shape", 10), ("init_cam", 3)):
            self.register_buffer(k, torch.randn(1, n, generator=g))


def test_adopt_and_one_regressor_step(renderer):
    torch.manual_seed(7)
    B = 12
    model = _StandIn().to(DEV).train()
    twins = {"f32": copy.deepcopy(model), "f64": copy.deepcopy(model)}
    for lin in ref.LINEARS:                                                    # (the head alone in float64: the trunk is torch's on every route)
        getattr(twins["f64"], lin).double()
    for k in ref.INIT_KEYS:
        twins["f64"]._buffers[k] = twins["f64"]._buffers[k].double()
    hmr = reg.HipHMR.adopt(model, renderer=renderer)
    for lin in ref.LINEARS:
        assert getattr(hmr.head, lin).weight is getattr(model, lin).weight
    assert {id(p) for p in hmr.parameters()} == {id(p) for p in model.parameters()} and hmr.head.training
    rng = np.random.RandomState(990)
    images = torch.tensor(rng.standard_normal((B, 3, 17, 17)).astype(np.float32), device=DEV)
    gt = torch.tensor(rng.normal(0, 0.3, (B, 24, 3)).astype(np.float32), device=DEV)
    masks = torch.from_numpy(ref.make_masks(hmr.head.spec, B, 991)).to(DEV)
    before = {k: v.detach().clone() for k, v in model.named_parameters()}
    opt = torch.optim.SGD(model.parameters(), lr=0.5)                           # (built on the adopted instance: its Parameters are the head's)
    loss = ganloop.regressor_step(hmr, opt, images, gt, renderer, gt_is_axis_angle=True, cap=math.inf, max_norm=1e9, masks=masks)
    assert loss.dtype == torch.float64 and bool(torch.isfinite(loss))
    moved = {k: (v.detach() - before[k]).cpu().numpy().astype(np.float64) for k, v in model.named_parameters()}
    assert all(np.any(m != 0.0) for m in moved.values()), [k for k, m in moved.items() if not np.any(m != 0.0)]
    # the same step with stock operators, the head in float32 and in float64 on the same device: the loss's own kernels take float32
    steps = {}
    for name, twin in twins.items():
        o = torch.optim.SGD(twin.parameters(), lr=0.5)
        o.zero_grad()
        trunk = reg._Trunk(twin)
        pred = reg.stock_forward(twin, trunk(images), masks=masks)[0]
        l2 = ganloop.regressor_loss(renderer, pred.float(), gt, gt_is_axis_angle=True, cap=math.inf)
        l2.backward()
        o.step()
        steps[name] = {k: v.detach().double().cpu().numpy() - before[k].double().cpu().numpy() for k, v in twin.named_parameters()}
    checked = 0
    for k, m in moved.items():
        if m.size >= 256:
            _ratio_rule(f"regressor_step {k}", m, steps["f64"][k], steps["f32"][k])
            checked += 1
    assert checked >= 5
