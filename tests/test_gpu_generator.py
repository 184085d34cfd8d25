"""The pose generator on the device (include/posegen_generator.h, posegen_amd/generators.py) against the float64 restatement
(tests/generator_ref.py).

Layer-local checks at every B: each layer's Z against the float64 layer applied to the device's own previous layer (rebuilt in
float64 from the device's Z, scale and shift), under a bound derived from float32 and carried down: with u = 2^-24, K the layer's
input width and h the rebuilt input,  |Z_dev - Z_64| <= (K + 2) u (|h| |W|^T + |b|) + dh |W|^T,  dh = 2 u |h| (the device forms h
with one fused multiply-add and one product by the slope).  The error is compared with the bound, never divided by it for the
assertion; the worst ratios are printed (DESIGN.md 2.17 records them).

End-to-end checks at B in {17, 65, 130} (and once at 1024): max|dev - f64| / max|cpu32 - f64| <= 4 per tensor of 256 elements and
more, the yardstick of tests/test_gpu_discriminators.py -- measured against torch float32 on the CPU, with the device's masks fed to
both backwards, on the pre-head y and every parameter gradient; the backward starts at the cotangent of y (the epilogue's own
derivative at the device's y: its 1 / |a| is ill-conditioned and is covered layer-locally).  The Linear biases in front of a BatchNorm have a zero gradient in
exact arithmetic and are held to an absolute bound instead: the device's db is the column sum of dZ = fl32(k (B dY - d_beta - x^
d_gamma)), whose unrounded terms sum to -d_gamma sum(x^) k = 0 up to double rounding whatever dY was, so what is left is the float32
rounding of each dZ:  |db| <= u sum_b |dZ[b]|, taken with a factor 2 on the float64 dZ (the device's differs from it by parts in
10^5) plus the double sum's own 2^-40 sum_b |dZ[b]|."""
import ctypes as C

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from posegen_amd import _ffi, ganloop, generators as gen, discriminators as disc
from tests import generator_ref as ref
from tests.frame_metrics_gpu import DEV, renderer  # noqa: F401 (renderer: a fixture)

pytestmark = pytest.mark.gpu
U = 2.0 ** -24
SENT, PAD = 12345.0, 64
BATCHES = (2, 3, 15, 16, 17, 63, 64, 65, 130)
WORST = {}


def _note(name, err, bound):
    """the worst error-to-bound ratio of a check, for the record (printed; the assertion itself compares err with bound)"""
    with np.errstate(invalid="ignore", divide="ignore"):
        r = np.where(bound > 0, err / np.where(bound > 0, bound, 1.0), np.where(err > 0, np.inf, 0.0))
    WORST[name] = max(WORST.get(name, 0.0), float(np.max(r)))
    print(f"RATIO {name}: {float(np.max(r)):.3f} (worst so far {WORST[name]:.3f})")


def _guarded(n, dtype=torch.float32, offset=0):
    """a device array of n elements between sentinels, `offset` elements off the allocation's alignment -> (all of it, the view)"""
    full = torch.full((n + 2 * PAD + offset,), SENT, dtype=dtype, device=DEV)
    return full, full[PAD + offset:PAD + offset + n]


def _intact(full, n, offset=0):
    h = full.cpu().numpy()
    return bool(np.all(h[:PAD + offset] == SENT) and np.all(h[PAD + offset + n:] == SENT))


def _off(a, offset=0):
    """the array on the device, `offset` floats off 16-byte alignment"""
    a = np.ascontiguousarray(a)
    full = torch.empty(a.size + 4 + offset, dtype=torch.float32, device=DEV)
    base = (-(full.data_ptr() // 4)) % 4                                       # to a 16-byte boundary, then `offset` floats past it
    v = full[base + offset:base + offset + a.size].view(a.shape)
    v.copy_(torch.from_numpy(a))
    return v


class Trunks:
    """one raw-API run: the parameters on the device (each tensor its own allocation), the tape between sentinels"""

    def __init__(self, renderer, spec, params, noise, B, training=True, offset=0, run=True):
        self.r, self.spec, self.B, self.training, self.offset = renderer, spec, B, training, offset
        self.dev = [[{k: _off(v, offset) for k, v in layer.items() if k != "names"} for layer in layers] for layers in params]
        self.noise = [None if n is None else _off(n, offset) for n in noise]
        self.layout, self.n_f, self.n_d = spec.tape_layout(B)
        self.tape_full, self.tape = _guarded(self.n_f, offset=offset)
        self.stats_full, self.stats = _guarded(self.n_d, torch.float64)
        self.cs = spec.c_spec()
        self.tab = gen.pointer_table(_ffi.PgGenParams(), spec, {f: [[layer[k] for layer in layers] for layers in self.dev] for f, k in
                                                                (("w", "w"), ("b", "b"), ("gamma", "gamma"), ("beta", "beta"),
                                                                 ("running_mean", "rm"), ("running_var", "rv"))})
        if run:
            self.forward()

    def forward(self):
        _ffi.call(self.r, "pg_gen_trunk_forward", C.byref(self.cs), C.byref(self.tab), gen.pointer_array(self.noise), self.B, int(self.training),
                  self.tape, self.stats)
        torch.cuda.synchronize()
        assert _intact(self.tape_full, self.n_f, self.offset) and _intact(self.stats_full, self.n_d)
        self.host = (self.tape.cpu().numpy(), self.stats.cpu().numpy())
        return self

    def layer(self, t, l):
        """the device's tape of layer l of trunk t as float64 arrays (the float32 values, exactly)"""
        at, W = self.layout[t][l], self.spec.trunks[t][1]
        tape, stats = self.host
        return {"z": tape[at["z"]:at["z"] + self.B * W].reshape(self.B, W).astype(np.float64), "scale": tape[at["scale"]:at["scale"] + W].astype(np.float64),
                "shift": tape[at["shift"]:at["shift"] + W].astype(np.float64), "mean": stats[at["mean"]:at["mean"] + W], "var": stats[at["var"]:at["var"] + W]}

    def pre(self, t, l):
        d = self.layer(t, l)
        return d["z"] * d["scale"] + d["shift"]                                # (the product is exact in double: the fused value's sign)

    def h(self, t, l):
        """layer l's activation rebuilt in float64 from the device's Z, scale and shift"""
        return ref.leaky(self.pre(t, l), float(np.float32(self.spec.slope)))   # (the slope as the kernels hold it)

    def running(self, t, l):
        return self.dev[t][l]["rm"].cpu().numpy(), self.dev[t][l]["rv"].cpu().numpy()

    def head(self, t, J, w2, b2):
        self.J, self.w2, self.b2 = J, _off(w2, self.offset), _off(b2, self.offset)
        self.y_full, self.y = _guarded(self.B * 4 * J, offset=self.offset)
        self.pose_full, self.pose = _guarded(self.B * J * 3, offset=self.offset)
        _ffi.call(self.r, "pg_gen_ba_head_forward", C.byref(self.cs), t, self.tape, self.B, J, self.w2, self.b2, self.y, self.pose)
        torch.cuda.synchronize()
        assert _intact(self.y_full, self.B * 4 * J, self.offset) and _intact(self.pose_full, self.B * J * 3, self.offset)
        return self.y.cpu().numpy().reshape(self.B, 4 * J), self.pose.cpu().numpy().reshape(self.B, J, 3)

    def head_backward(self, t, d_pose, want=(True, True, True)):
        W, J = self.spec.trunks[t][1], self.J
        sizes = (4 * J * W, 4 * J, self.B * W)
        bufs = [_guarded(n, offset=self.offset) if w else (None, None) for n, w in zip(sizes, want)]
        self.d_pose = _off(d_pose, self.offset)
        _ffi.call(self.r, "pg_gen_ba_head_backward", C.byref(self.cs), t, self.tape, self.B, J, self.w2, self.y, self.d_pose, *[b[1] for b in bufs])
        torch.cuda.synchronize()
        for (full, _), n, w in zip(bufs, sizes, want):
            assert not w or _intact(full, n, self.offset)
        self.d_h = bufs[2][1]
        return [None if v is None else v.cpu().numpy() for _, v in bufs]

    def backward(self, d_out, want=lambda t, l, k: True):
        """d_out: per trunk a device tensor, an array or None -> {(t, l, k): gradient}"""
        d_out = [None if d is None else (d if torch.is_tensor(d) else _off(d, self.offset)) for d in d_out]
        fields = {k: [[None] * self.spec.layers(t) for t in range(len(self.spec.trunks))] for k in ("w", "b", "gamma", "beta")}
        held = {}
        for t, layers in enumerate(self.dev):
            for l, layer in enumerate(layers):
                for k in fields:
                    if want(t, l, k):
                        n = layer[k].numel()
                        held[(t, l, k)] = _guarded(n, offset=self.offset) + (n, tuple(layer[k].shape))
                        fields[k][t][l] = held[(t, l, k)][1]
        gtab = gen.pointer_table(_ffi.PgGenGrads(), self.spec, fields)
        _ffi.call(self.r, "pg_gen_trunk_backward", C.byref(self.cs), C.byref(self.tab), gen.pointer_array(self.noise), self.B, int(self.training), self.tape, self.stats,
                  gen.pointer_array(d_out), C.byref(gtab) if held else None)
        torch.cuda.synchronize()
        out = {}
        for key, (full, view, n, shape) in held.items():
            assert _intact(full, n, self.offset), key
            out[key] = view.cpu().numpy().reshape(shape)
        return out


def _ulp32(v):
    return np.spacing(np.abs(np.asarray(v, np.float64)).astype(np.float32)).astype(np.float64)


def _layer_bound(h, dh, w, b):
    w, b = np.abs(np.asarray(w, np.float64)), np.abs(np.asarray(b, np.float64))
    return (w.shape[1] + 2) * U * (np.abs(h) @ w.T + b) + dh @ w.T + 2.0 ** -149


def _check_layers(run, params, noise, tag, before=None):
    """every layer-local property of one forward run"""
    spec, B = run.spec, run.B
    for t, layers in enumerate(params):
        if noise[t] is None:
            continue
        for l, layer in enumerate(layers):
            d = run.layer(t, l)
            h = np.asarray(noise[t], np.float64) if l == 0 else run.h(t, l - 1)
            dh = np.zeros_like(h) if l == 0 else 2 * U * np.abs(h)
            z64 = h @ np.asarray(layer["w"], np.float64).T + np.asarray(layer["b"], np.float64)
            err, bound = np.abs(d["z"] - z64), _layer_bound(h, dh, layer["w"], layer["b"])
            _note(f"{tag} Z", err, bound)
            assert np.all(err <= bound), (tag, B, t, l, float(np.max(err / bound)))
            rm0, rv0 = (np.asarray(layer["rm"], np.float64), np.asarray(layer["rv"], np.float64)) if before is None else before[t][l]
            if run.training:
                zl = d["z"].astype(np.longdouble)
                mean, var = (zl.sum(0) / B).astype(np.float64), (((zl - zl.sum(0) / B) ** 2).sum(0) / B).astype(np.float64)
                e_mean, b_mean = np.abs(d["mean"] - mean), B * 2.0 ** -53 * np.abs(d["z"]).sum(0) / B
                e_var, b_var = np.abs(d["var"] - var), B * 2.0 ** -53 * (d["z"] ** 2).sum(0) / B
                _note(f"{tag} mean", e_mean, b_mean)
                _note(f"{tag} var", e_var, b_var)
                assert np.all(e_mean <= b_mean) and np.all(e_var <= b_var), (tag, B, t, l)
                m = float(np.float32(spec.momentum))                           # (the momentum as the kernels hold it)
                rm64, rv64 = (1 - m) * rm0 + m * d["mean"], (1 - m) * rv0 + m * d["var"] * B / (B - 1.0)
                rm, rv = run.running(t, l)
                assert np.all(np.abs(rm - rm64) <= 2 * _ulp32(rm64)) and np.all(np.abs(rv - rv64) <= 2 * _ulp32(rv64)), (tag, B, t, l)
            else:
                assert np.array_equal(d["mean"], rm0) and np.array_equal(d["var"], rv0)
                rm, rv = run.running(t, l)
                assert np.array_equal(rm, np.asarray(layer["rm"])) and np.array_equal(rv, np.asarray(layer["rv"]))   # untouched
            scale64 = np.asarray(layer["gamma"], np.float64) / np.sqrt(d["var"] + float(np.float32(spec.eps)))
            shift64 = np.asarray(layer["beta"], np.float64) - d["mean"] * scale64
            assert np.all(np.abs(d["scale"] - scale64) <= 2 * _ulp32(scale64)) and np.all(np.abs(d["shift"] - shift64) <= 2 * _ulp32(shift64)), (tag, B, t, l)


def _check_head(run, t, J, seed, tag, head=None, nan_joints=()):
    """the head's y against the float64 layer on the device's own last layer; pose against float64 from the device's own y: the
    epilogue is nine float32 operations in a row on a value (three squares and two sums, a root, a quotient, one or two products),
    each within u: 8 u |pose| covers them (the root halves the error of the sum of squares).  `head`: (w2, b2) in place of the
    seed's; `nan_joints`: the joints whose axis the caller made exactly zero -- their pose must be NaN on every row."""
    spec = run.spec
    W = spec.trunks[t][1]
    w2, b2 = ref.make_head(4 * J, W, np.random.RandomState(seed)) if head is None else head
    y, pose = run.head(t, J, w2, b2)
    h = run.h(t, spec.layers(t) - 1)
    y64 = h @ w2.astype(np.float64).T + b2.astype(np.float64)
    err, bound = np.abs(y - y64), _layer_bound(h, 2 * U * np.abs(h), w2, b2)
    _note(f"{tag} y", err, bound)
    assert np.all(err <= bound)
    pose64 = ref.ba_pose(y.astype(np.float64))
    err, bound = np.abs(pose - pose64), 8 * U * np.abs(pose64) + 2.0 ** -149
    if len(nan_joints):
        assert np.all(np.isnan(pose[:, list(nan_joints)])) and np.all(np.isnan(pose64[:, list(nan_joints)]))
        err, bound = np.delete(err, list(nan_joints), axis=1), np.delete(bound, list(nan_joints), axis=1)
    _note(f"{tag} pose", err, bound)
    assert np.all(err <= bound)
    return w2, b2, y, pose


@pytest.mark.parametrize("B", BATCHES)
def test_layer_local_checks_on_the_ragged_toy_spec(renderer, B):
    spec = ref.toy_spec()
    params, noise = ref.make_params(spec, 41), ref.make_noise(spec, B, 42 + B)
    run = Trunks(renderer, spec, params, noise, B, training=True)
    _check_layers(run, params, noise, "toy train")
    _check_head(run, 0, 5, 43, "toy")                                          # 20 columns: one full tile and a quarter
    ev = Trunks(renderer, spec, params, noise, B, training=False)
    _check_layers(ev, params, noise, "toy eval")


def _rt_check(run, tr, tt, J, seed, eps_edit=None, nan_rows=()):
    """R, T and pose_rt against float64 from the device's own trunk outputs.  The device rounds r to float32 (dr = 2 u |r|), works in
    double from there and rounds R once: with the rotation 2-Lipschitz in its vector,  E_R = u + 2 (2 |r6| d_axis / |axis| + 2 u |r6|),
    d_axis = 2 u (|r_mean| + 2 r_std^2 |eps|) summed over the axis.  T is a float32 dot product over the width in wave order:
    the layer bound, its third entry squared.  pose_rt adds three products and three sums in float32.
    `eps_edit`: a function that edits the drawn eps in place; `nan_rows`: the rows whose axis the caller made exactly zero -- their
    R and pose_rt must be NaN and their T finite, and the bounds hold on the other rows.  -> (R, T, pose_rt) as read back"""
    spec, B = run.spec, run.B
    rng = np.random.RandomState(seed)
    WT = spec.trunks[tt][1]
    w2, b2 = ref.make_head(3, WT, rng)
    eps, x = rng.standard_normal((B, 3)).astype(np.float32), rng.standard_normal((B, J, 3)).astype(np.float32)
    if eps_edit is not None:
        eps_edit(eps)
    outs = [_guarded(n) for n in (B * 9, B * 3, B * J * 3)]
    _ffi.call(run.r, "pg_gen_rt_head", C.byref(run.cs), tr, tt, run.tape, B, J, _off(w2), _off(b2), _off(eps), _off(x), *[o[1] for o in outs])
    torch.cuda.synchronize()
    assert all(_intact(o[0], n) for o, n in zip(outs, (B * 9, B * 3, B * J * 3)))
    R, T, pose = outs[0][1].cpu().numpy().reshape(B, 3, 3), outs[1][1].cpu().numpy().reshape(B, 3), outs[2][1].cpu().numpy().reshape(B, J, 3)
    read_back = (R, T, pose)
    r, ht = run.h(tr, spec.layers(tr) - 1), run.h(tt, spec.layers(tt) - 1)
    if len(nan_rows):
        bad = list(nan_rows)
        assert np.all(np.isnan(R[bad])) and np.all(np.isnan(pose[bad])) and np.all(np.isfinite(T[bad]))
        keep = np.setdiff1d(np.arange(B), bad)
        R, T, pose, r, ht, eps, x = R[keep], T[keep], pose[keep], r[keep], ht[keep], eps[keep], x[keep]
    R64, T64, pose64 = ref.rt_head(r, ht, w2, b2, eps, x)
    d_axis = 2 * U * (np.abs(r[:, :3]) + 2 * r[:, 3:6] ** 2 * np.abs(eps)).sum(-1)
    axis = np.linalg.norm(r[:, :3] + r[:, 3:6] ** 2 * eps, axis=-1)
    e_R = (U + 2 * (2 * np.abs(r[:, 6]) * d_axis / axis + 2 * U * np.abs(r[:, 6])))[:, None, None]
    err = np.abs(R - R64)
    _note("rt R", err, np.broadcast_to(e_R, err.shape))
    assert np.all(err <= e_R)
    t_lin = ht @ w2.astype(np.float64).T + b2.astype(np.float64)
    e_t = _layer_bound(ht, 2 * U * np.abs(ht), w2, b2)
    e_t[:, 2] = 2 * np.abs(t_lin[:, 2]) * e_t[:, 2] + e_t[:, 2] ** 2 + U * T64[:, 2]
    err = np.abs(T - T64)
    _note("rt T", err, e_t)
    assert np.all(err <= e_t)
    xc = np.abs(x.astype(np.float64) - x[:, :1].astype(np.float64))
    mag = np.einsum("bcd,bjd->bjc", np.abs(R64) + e_R, xc)
    e_p = np.einsum("bcd,bjd->bjc", np.broadcast_to(e_R, R64.shape), xc) + 6 * U * (mag + np.abs(T64)[:, None, :]) + e_t[:, None, :]
    err = np.abs(pose - pose64)
    _note("rt pose_rt", err, e_p)
    assert np.all(err <= e_p)
    return read_back


def test_the_rotation_translation_head_on_the_toy_and_the_shipped_spec(renderer):
    spec = ref.toy_spec()
    params, noise = ref.make_params(spec, 51), ref.make_noise(spec, 70, 52)
    _rt_check(Trunks(renderer, spec, params, noise, 70), 2, 0, 7, 53)
    spec = ref.shipped_spec()
    params, noise = ref.make_params(spec, 54), ref.make_noise(spec, 130, 55)
    _rt_check(Trunks(renderer, spec, params, noise, 130), 1, 2, 24, 56)


def _twin(layers, noise, w2, b2, d_y, masks, dtype, spec):
    """torch on the CPU in `dtype` through its own linear and batch_norm, the given masks in LeakyReLU's place, backward from the
    cotangent d_y of the pre-head y -> (y, gradients)"""
    P = [{k: torch.tensor(np.asarray(layer[k]), dtype=dtype, requires_grad=True) for k in ("w", "b", "gamma", "beta")} for layer in layers]
    tw, tb = torch.tensor(w2, dtype=dtype, requires_grad=True), torch.tensor(b2, dtype=dtype, requires_grad=True)
    h = torch.tensor(noise, dtype=dtype)
    for p, m in zip(P, masks):
        y = F.batch_norm(F.linear(h, p["w"], p["b"]), None, None, p["gamma"], p["beta"], True, spec.momentum, spec.eps)
        h = y * torch.where(torch.tensor(m), torch.tensor(1.0, dtype=dtype), torch.tensor(spec.slope, dtype=dtype))
    y = F.linear(h, tw, tb)
    y.backward(torch.tensor(d_y, dtype=dtype))
    grads = {(l, k): p[k].grad.double().numpy() for l, p in enumerate(P) for k in p}
    grads["w2"], grads["b2"] = tw.grad.double().numpy(), tb.grad.double().numpy()
    return y.detach().double().numpy(), grads


def _end_to_end(renderer, spec, t, B, J, seed, tag):
    params, noise = ref.make_params(spec, seed), ref.make_noise(spec, B, seed + 1)
    only = [n if i == t else None for i, n in enumerate(noise)]
    run = Trunks(renderer, spec, params, only, B)
    rng = np.random.RandomState(seed + 2)
    w2, b2 = ref.make_head(4 * J, spec.trunks[t][1], rng)
    y, _ = run.head(t, J, w2, b2)
    d_pose = rng.standard_normal((B, J, 3)).astype(np.float32)
    d_w2, d_b2, _ = run.head_backward(t, d_pose)
    got = run.backward([run.d_h if i == t else None for i in range(len(spec.trunks))])
    masks = [run.pre(t, l) > 0 for l in range(spec.layers(t))]
    # the head's epilogue divides by |a| and is ill-conditioned: like the masks, its cotangent is taken at the device's own y for
    # both twins (the device forms it in double and rounds once; the epilogue itself is checked layer-locally)
    d_y = ref.ba_head_dy(y.astype(np.float64), d_pose)
    y64, g64 = _twin(params[t], noise[t], w2, b2, d_y, masks, torch.float64, spec)
    y32, g32 = _twin(params[t], noise[t], w2, b2, d_y, masks, torch.float32, spec)
    dev = {(l, k): got[(t, l, k)] for l in range(spec.layers(t)) for k in ("w", "b", "gamma", "beta")}
    dev["w2"], dev["b2"], dev["y"] = d_w2.reshape(w2.shape), d_b2, y
    g64["y"], g32["y"] = y64, y32
    # the float64 dZ of every layer, for the bias bound
    _, tape = ref.trunk_forward(params[t], noise[t], spec.slope, spec.eps, spec.momentum)
    dh = d_y @ w2.astype(np.float64)
    for l in range(spec.layers(t) - 1, -1, -1):
        tp = tape[l]
        dy = dh * np.where(masks[l], 1.0, spec.slope)
        xh = (tp["z"] - tp["mean"]) / np.sqrt(tp["var"] + spec.eps)
        dz = tp["scale"] / B * (B * dy - dy.sum(0) - xh * (dy * xh).sum(0))
        bound = (2 * U + 2.0 ** -40) * np.abs(dz).sum(0) + 2.0 ** -149
        err = np.abs(dev[(l, "b")])
        _note(f"{tag} db", err, bound)
        assert np.all(err <= bound), (tag, B, l)
        dh = dz @ np.asarray(params[t][l]["w"], np.float64)
    for key, d in dev.items():
        if (isinstance(key, tuple) and key[1] == "b") or d.size < 256:
            continue
        e_dev, e_cpu = float(np.max(np.abs(d - g64[key]))), float(np.max(np.abs(g32[key] - g64[key])))
        print(f"E2E {tag} B={B} {key}: dev {e_dev:.3e} cpu32 {e_cpu:.3e} ratio {e_dev / e_cpu:.3f}")
        WORST[f"{tag} e2e"] = max(WORST.get(f"{tag} e2e", 0.0), e_dev / e_cpu)
        assert e_dev <= 4 * e_cpu, (tag, B, key, e_dev, e_cpu)


@pytest.mark.parametrize("B", (17, 65, 130))
def test_end_to_end_against_torch_float32_on_the_toy_spec(renderer, B):
    spec = ref.toy_spec()
    for t, J in ((0, 5), (1, 3), (2, 24)):
        _end_to_end(renderer, spec, t, B, J, 60 + 3 * t, "toy")


@pytest.mark.parametrize("B", (130, 1024))
def test_the_shipped_spec_layer_local_and_end_to_end(renderer, B):
    spec = ref.shipped_spec()
    params, noise = ref.make_params(spec, 71), ref.make_noise(spec, B, 72)
    run = Trunks(renderer, spec, params, noise, B)
    _check_layers(run, params, noise, "shipped train")
    _check_head(run, 0, 24, 73, "shipped")
    _end_to_end(renderer, spec, 0, B, 24, 74, "shipped")
    print("WORST", {k: round(v, 3) for k, v in WORST.items()})


# ---- exactness ---------------------------------------------------------------------------------------------------------------------------
def _full_run(renderer, spec, params, noise, B, offset=0, want=lambda t, l, k: True, cot=(True, True, True), J=5, seed=80):
    """forward, head on trunk 0, head backward, trunk backward with random cotangents on the other trunks -> every byte that came out"""
    run = Trunks(renderer, spec, params, noise, B, offset=offset)
    rng = np.random.RandomState(seed)
    w2, b2 = ref.make_head(4 * J, spec.trunks[0][1], rng)
    d_pose = rng.standard_normal((B, J, 3)).astype(np.float32)
    cots = [rng.standard_normal((B, w)).astype(np.float32) for _, w, _ in spec.trunks]
    out = {"tape": run.tape.cpu().numpy().copy(), "stats": run.stats.cpu().numpy().copy()}
    out["y"], out["pose"] = run.head(0, J, w2, b2)
    out["d_w2"], out["d_b2"], out["d_h"] = run.head_backward(0, d_pose)
    d_out = [(run.d_h if t == 0 else cots[t]) if (cot[t] and noise[t] is not None) else None for t in range(len(spec.trunks))]
    out.update(run.backward(d_out, want))
    for t, layers in enumerate(params):
        for l in range(len(layers)):
            out[(t, l, "rm")], out[(t, l, "rv")] = run.running(t, l)
    return out, run


def _same(a, b):
    return a.shape == b.shape and a.tobytes() == b.tobytes()


@pytest.fixture(scope="module")
def toy130(renderer):
    spec = ref.toy_spec()
    params, noise = ref.make_params(spec, 81), ref.make_noise(spec, 130, 82)
    return spec, params, noise, _full_run(renderer, spec, params, noise, 130)[0]


def test_two_runs_give_the_same_bytes_and_so_do_misaligned_views(renderer, toy130):
    spec, params, noise, first = toy130
    for offset in (0, 1, 2, 3):
        again, _ = _full_run(renderer, spec, params, noise, 130, offset=offset)
        assert set(again) == set(first)
        for k in first:
            assert _same(first[k], again[k]), (offset, k)


def test_a_trunk_alone_gives_the_bytes_it_gives_grouped(renderer, toy130):
    spec, params, noise, first = toy130
    layout, _, _ = spec.tape_layout(130)
    for t in range(3):
        only = [n if i == t else None for i, n in enumerate(noise)]
        run = Trunks(renderer, spec, params, only, 130)
        tape = run.tape.cpu().numpy()
        lo, hi = layout[t][0]["z"], layout[t][-1]["shift"] + spec.trunks[t][1]
        assert _same(tape[lo:hi], first["tape"][lo:hi])
        assert np.all(tape[:lo] == SENT) and np.all(tape[hi:] == SENT)          # the other trunks' tape is not written
        for u in range(3):
            for l in range(spec.layers(u)):
                rm, rv = run.running(u, l)
                if u == t:
                    assert _same(rm, first[(u, l, "rm")]) and _same(rv, first[(u, l, "rv")])
                else:
                    assert _same(rm, np.asarray(params[u][l]["rm"])) and _same(rv, np.asarray(params[u][l]["rv"]))
        cot = np.random.RandomState(83).standard_normal((130, spec.trunks[t][1])).astype(np.float32)
        alone = run.backward([cot if i == t else None for i in range(3)])
        both = Trunks(renderer, spec, params, noise, 130).backward([cot if i == t else np.ones((130, spec.trunks[i][1]), np.float32) for i in range(3)])
        for key, g in alone.items():
            if key[0] == t:
                assert _same(g, both[key]), key
            else:
                assert np.all(g == SENT), key                                  # a trunk with a NULL cotangent writes nothing


def test_the_stems_rows_do_not_depend_on_the_batch(renderer, toy130):
    spec, params, noise, first = toy130
    layout, _, _ = spec.tape_layout(130)
    small = Trunks(renderer, spec, params, [n[:17] for n in noise], 17)
    for t in range(3):
        W = spec.trunks[t][1]
        z17 = small.tape.cpu().numpy()[small.layout[t][0]["z"]:][:17 * W]
        assert _same(z17, first["tape"][layout[t][0]["z"]:][:17 * W])


def test_eval_mode_rows_are_independent_of_the_batch(renderer):
    spec = ref.toy_spec()
    params, noise = ref.make_params(spec, 84), ref.make_noise(spec, 130, 85)
    J = 5
    w2, b2 = ref.make_head(4 * J, 40, np.random.RandomState(86))

    def rows(ns, B):
        run = Trunks(renderer, spec, params, ns, B, training=False)
        y, pose = run.head(0, J, w2, b2)
        zs = [run.layer(t, l)["z"] for t in range(3) for l in range(spec.layers(t))]
        return zs, y, pose
    zs, y, pose = rows(noise, 130)
    perm = np.random.RandomState(87).permutation(130)
    zp, yp, posep = rows([n[perm] for n in noise], 130)
    assert all(_same(a[perm], b) for a, b in zip(zs, zp)) and _same(y[perm], yp) and _same(pose[perm], posep)
    for row in (0, 77, 129):
        z1, y1, pose1 = rows([n[row:row + 1] for n in noise], 1)
        assert all(_same(a[row:row + 1], b) for a, b in zip(zs, z1)) and _same(y[row:row + 1], y1) and _same(pose[row:row + 1], pose1)


@pytest.mark.parametrize("subset", ["one trunk", "one layer", "one tensor", "none but the head"])
def test_any_subset_of_gradient_pointers_gives_the_all_gradients_bytes(renderer, toy130, subset):
    spec, params, noise, first = toy130
    want = {"one trunk": lambda t, l, k: t == 1, "one layer": lambda t, l, k: l == 2, "one tensor": lambda t, l, k: (t, l, k) == (2, 3, "gamma"),
            "none but the head": lambda t, l, k: False}[subset]
    part, run = _full_run(renderer, spec, params, noise, 130, want=want)
    assert any(isinstance(k, tuple) and k[2] in ("w", "b", "gamma", "beta") for k in part) == (subset != "none but the head")
    for k, v in part.items():
        assert _same(v, first[k]), k
    # the head's three results one at a time
    for i in range(3):
        got = run.head_backward(0, run.d_pose.cpu().numpy(), want=tuple(j == i for j in range(3)))
        assert _same(got[i], first[("d_w2", "d_b2", "d_h")[i]]) and all(g is None for j, g in enumerate(got) if j != i)


def test_results_are_the_same_before_and_after_the_workspaces_grew(toy130):
    """On a handle of its own, so that what the workspaces hold is this test's doing: the first run allocates dZ (130 rows of the
    toy spec's 525 columns = 68 250 floats) and dy (130 x 20); the shipped spec at B = 300 with three cotangents and J = 24 then asks
    for 3 x 5 x 300 x 256 = 1 152 000 and 300 x 96 floats, so both buffers are freed and allocated again; the third run works in
    the grown buffers.  All three toy results are the bytes of the module's handle."""
    from posegen_amd import surreal_config
    from posegen_amd.raycaster import HipRenderer
    spec, params, noise, first = toy130
    big = ref.shipped_spec()
    assert 3 * 5 * 300 * 256 > 130 * sum(spec.layers(t) * w for t, (_, w, _) in enumerate(spec.trunks)) and 300 * 96 > 130 * 20
    own = HipRenderer(surreal_config(), device=DEV)
    try:
        before, _ = _full_run(own, spec, params, noise, 130)
        _full_run(own, big, ref.make_params(big, 88), ref.make_noise(big, 300, 89), 300, J=24)
        after, _ = _full_run(own, spec, params, noise, 130)
    finally:
        own.close()
    for k in first:
        assert _same(first[k], before[k]) and _same(first[k], after[k]), k


def test_a_nan_noise_row_fills_its_trunk_and_leaves_the_others(renderer, toy130):
    spec, params, noise, first = toy130
    layout, _, _ = spec.tape_layout(130)
    bad = [n.copy() for n in noise]
    bad[1][7, 3] = np.nan
    run = Trunks(renderer, spec, params, bad, 130)
    tape = run.tape.cpu().numpy()
    last = run.layer(1, spec.layers(1) - 1)
    assert np.all(np.isnan(last["z"])) and np.all(np.isnan(last["scale"])) and np.all(np.isnan(run.running(1, 0)[0]))
    for t in (0, 2):
        lo, hi = layout[t][0]["z"], layout[t][-1]["shift"] + spec.trunks[t][1]
        assert _same(tape[lo:hi], first["tape"][lo:hi])


def test_a_backward_of_an_eval_mode_tape_is_refused(renderer):
    spec = ref.toy_spec()
    params, noise = ref.make_params(spec, 90), ref.make_noise(spec, 20, 91)
    run = Trunks(renderer, spec, params, noise, 20, training=False)
    cots = [np.ones((20, w), np.float32) for _, w, _ in spec.trunks]
    with pytest.raises(_ffi.PgError, match="eval mode"):
        run.backward(cots)
    run.training = True
    run.forward()                                                              # the same tape written again in training mode
    assert len(run.backward(cots)) == 4 * 13


# ---- the modules ---------------------------------------------------------------------------------------------------------------------------
def _modules(renderer, seed, dtype_list=(torch.float64, torch.float32)):
    m = gen.HipPoseGenerator(renderer=renderer)
    sd_np = ref.make_state_dict(m, seed)
    sd = {k: torch.as_tensor(v) for k, v in sd_np.items()}
    m.load_state_dict(sd, strict=True)
    twins = []
    for dt in dtype_list:
        tw = gen.HipPoseGenerator()
        tw.load_state_dict(sd, strict=True)
        twins.append(tw.to(dt).train())
    return m.to(DEV).train(), twins, sd_np


def _noise(B, seed):
    rng = np.random.RandomState(seed)
    return {"ba": rng.standard_normal((B, 32)).astype(np.float32), "r": rng.standard_normal((B, 72)).astype(np.float32),
            "eps": rng.standard_normal((B, 3)).astype(np.float32), "t": rng.standard_normal((B, 72)).astype(np.float32)}


def _device_masks(renderer, sd_np, noise, B):
    """the LeakyReLU masks of the BA trunk as the device has them: the module keeps no tape to read, but the same parameters and draws
    through the raw entry point give the same bytes (the exactness tests above)"""
    run = Trunks(renderer, ref.shipped_spec(), ref.pose_generator_trunks(sd_np), [noise["ba"], noise["r"], noise["t"]], B)
    return [torch.tensor(run.pre(0, l) > 0) for l in range(5)]


def _disc_masks(renderer, d, pose):
    """the discriminator's LeakyReLU masks on `pose` as the device has them (the sign of pg_disc_forward's tape).  The discriminator is
    piecewise linear: a perturbation of its input of float32's size flips a few of its ~10^6 masks, and one flip moves the gradient of
    the input by parts in 10^2 (measured on the CPU in float64: inputs 1e-6 apart gave gradients 4e-7 .. 8e-7 of 5e-5 apart in four
    of five trials).  So, like the generator's own masks, they are fed to both twins: the ratio then measures arithmetic."""
    spec, n_rows = d.spec, pose.shape[0]
    cs, tab, n = spec.c_spec(), disc._pointer_table(spec, d._flat_params()), C.c_int64(0)
    renderer._check(renderer.lib.pg_disc_tape_floats(C.byref(cs), n_rows, C.byref(n)))
    pred, tape = torch.empty(n_rows, len(spec.paths), device=DEV), torch.empty(n.value, device=DEV)
    _ffi.call(renderer, "pg_disc_forward", C.byref(cs), C.byref(tab), pose.detach().contiguous(), n_rows, pred, tape)
    tape = tape.cpu()
    return [[tape[off:off + n_rows * cols].reshape(n_rows, cols) > 0 for off, cols in layers] for layers in spec.tape_layout(n_rows)]


def _adversarial_loss_cpu(d, pose, dtype, masks):
    """0.5 mse(D(pose), 1) with the discriminator's Linears as torch operators on the CPU in `dtype`, the given masks in LeakyReLU's place"""
    preds = []
    one, slope = torch.ones((), dtype=dtype), torch.full((), d.spec.slope, dtype=dtype)
    for p, (_, sel, _, _) in enumerate(d.spec.paths):
        h = pose[:, sel, :].reshape(pose.shape[0], -1)
        for i, lin in enumerate(d.path_linears(p)):
            h = F.linear(h, lin.weight.detach().cpu().to(dtype), lin.bias.detach().cpu().to(dtype))
            h = h * torch.where(masks[p][i], one, slope) if i < 4 else h
        preds.append(h)
    return 0.5 * ((torch.cat(preds, 1) - 1.0) ** 2).mean()


@pytest.fixture(scope="module")
def frozen_disc(renderer):
    torch.manual_seed(3)
    d = disc.HipPos3dDiscriminator(renderer).to(DEV)
    for p in d.parameters():
        p.requires_grad_(False)
    return d


def test_the_module_against_its_cpu_twins(renderer, frozen_disc):
    B = 65
    m, (t64, t32), sd_np = _modules(renderer, 101)
    noise, x = _noise(B, 102), np.random.RandomState(103).standard_normal((B, 24, 3)).astype(np.float32)
    masks = _device_masks(renderer, sd_np, noise, B)
    real = torch.tensor(x, device=DEV)
    out = m(real, noise=noise)
    assert set(out) == {"pose_ba", "ba_diff", "pose_bl", "blr", "pose_rt", "R", "T"} and out["ba_diff"] is None and out["blr"] is None
    assert out["pose_ba"].requires_grad and not out["R"].requires_grad and not out["T"].requires_grad and not out["pose_rt"].requires_grad
    ganloop.generator_adversarial_loss(frozen_disc, real, out["pose_ba"])[0].backward()
    d_masks = _disc_masks(renderer, frozen_disc, out["pose_ba"])
    res = []
    for tw, dt in ((t64, torch.float64), (t32, torch.float32)):
        o = gen.stock_forward(tw, torch.tensor(x), noise, masks=masks)
        _adversarial_loss_cpu(frozen_disc, o["pose_ba"], dt, d_masks).backward()
        res.append(o)
    for k in ("R", "T", "pose_rt"):
        # (pose_ba itself goes through 1 / |a|, which is ill-conditioned: it is covered layer-locally above; here its gradients are)
        d, a, b = out[k].detach().cpu().double().numpy(), res[0][k].detach().double().numpy(), res[1][k].detach().double().numpy()
        e_dev, e_cpu = np.max(np.abs(d - a)), np.max(np.abs(b - a))
        print(f"MODULE {k}: dev {e_dev:.3e} cpu32 {e_cpu:.3e}")
        assert e_dev <= 4 * e_cpu, k
    assert np.allclose(out["pose_ba"].detach().cpu().numpy(), res[0]["pose_ba"].detach().numpy(), rtol=1e-3, atol=1e-4)
    named, n64, n32 = dict(m.named_parameters()), dict(t64.named_parameters()), dict(t32.named_parameters())
    for k, p in named.items():
        assert (p.grad is None) == (n64[k].grad is None) == k.startswith("RTprocess."), k
        if p.grad is None or p.numel() < 256 or (k.endswith(".bias") and "batch_norm" not in k and not k.endswith("BAprocess.w2.bias")):
            continue                                                           # (the Linear biases in front of a BatchNorm: zero in exact arithmetic)
        a = n64[k].grad.numpy()
        e_dev, e_cpu = np.max(np.abs(p.grad.cpu().double().numpy() - a)), np.max(np.abs(n32[k].grad.double().numpy() - a))
        print(f"MODULE grad {k}: dev {e_dev:.3e} cpu32 {e_cpu:.3e}")
        assert e_dev <= 4 * e_cpu, k
    for (k, b), (_, b64) in zip(m.named_buffers(), t64.named_buffers()):
        if k.endswith("num_batches_tracked"):
            assert int(b) == int(b64) == 4, k
        else:
            assert np.all(np.abs(b.cpu().numpy() - b64.numpy()) <= 1e-5 * (1.0 + np.abs(b64.numpy()))), k


def test_the_default_draws_follow_the_references_order(renderer):
    B = 20
    m, _, _ = _modules(renderer, 105, ())
    x = torch.zeros(B, 24, 3, device=DEV)
    torch.manual_seed(7)
    a = m(x)
    torch.manual_seed(7)
    manual = {"ba": torch.randn(B, 32, device=DEV), "r": torch.randn(B, 72, device=DEV), "eps": torch.randn(B, 3, device=DEV),
              "t": torch.randn(B, 72, device=DEV)}
    m2, _, _ = _modules(renderer, 105, ())
    b = m2(x, noise=manual)
    for k in ("pose_ba", "R", "T", "pose_rt"):
        assert torch.equal(a[k], b[k]), k


def test_a_gradient_asked_in_eval_mode_raises_and_eval_runs_without_one(renderer):
    m, _, _ = _modules(renderer, 106, ())
    m.eval()
    x = torch.zeros(4, 24, 3, device=DEV)
    with torch.no_grad():
        out = m(x, noise=_noise(4, 107))
    assert torch.isfinite(out["pose_ba"]).all() and int(m.BAprocess.batch_norm1.num_batches_tracked) == 3
    out = m(x, noise=_noise(4, 107))
    with pytest.raises(RuntimeError, match="training mode only"):
        out["pose_ba"].sum().backward()


def test_one_generator_step_with_adam_moves_the_parameters_as_the_twin_does(renderer, frozen_disc):
    B = 64
    m, (t64,), sd_np = _modules(renderer, 108, (torch.float64,))
    real = torch.tensor(np.random.RandomState(110).standard_normal((B, 24, 3)).astype(np.float32), device=DEV)
    torch.manual_seed(11)
    noise = {k: v.cpu().numpy() for k, v in gen.draw_noise(B, real.device).items()}     # what generator_step draws after the same seed
    masks = _device_masks(renderer, sd_np, noise, B)
    before = {k: p.detach().clone() for k, p in m.named_parameters()}
    opt = torch.optim.Adam(m.parameters(), lr=1e-3)
    torch.manual_seed(11)
    pose, loss = ganloop.generator_step(m, frozen_disc, opt, real)             # (its own draws: the ones made above after the same seed)
    assert pose.shape == (B, 24, 3) and not pose.requires_grad and loss.ndim == 0 and loss.is_cuda and torch.isfinite(loss)
    # the twin: the same step in float64 on the CPU
    opt64 = torch.optim.Adam(t64.parameters(), lr=1e-3)
    opt64.zero_grad()
    loss64 = _adversarial_loss_cpu(frozen_disc, gen.stock_forward(t64, real.cpu(), noise, masks=masks)["pose_ba"], torch.float64,
                                   _disc_masks(renderer, frozen_disc, pose))
    loss64.backward()
    torch.nn.utils.clip_grad_norm_(t64.parameters(), max_norm=1.0)
    opt64.step()
    assert abs(float(loss) - float(loss64.detach())) <= 1e-4 * max(1.0, abs(float(loss64.detach())))
    moved = 0
    for (k, p), (_, q) in zip(m.named_parameters(), t64.named_parameters()):
        if k.startswith("RTprocess."):
            assert torch.equal(p.detach(), before[k]), k                       # no gradient: Adam leaves it
            continue
        # Adam's first step is lr g / (|g| + 1e-8): entries whose clipped gradient is well away from zero moved by lr sign(g) to 1 %
        step, step64 = (p.detach() - before[k]).cpu().double(), q.detach() - before[k].cpu().double()
        firm = q.grad.abs() > 1e-6
        assert torch.allclose(step[firm], step64[firm], atol=2e-5), k
        moved += int(firm.sum())
    assert moved > 1000


def test_the_two_generators_alone_give_the_pose_generators_bytes(renderer):
    """`HipBAGenerator` and `HipRTGenerator` called on their own (one trunk, two trunks) against `HipPoseGenerator` on the same tensors
    and draws: a trunk's bytes do not depend on what it is grouped with, and the RT generator alone builds no graph"""
    B = 33
    m, _, _ = _modules(renderer, 111, ())
    noise, x = _noise(B, 112), torch.tensor(np.random.RandomState(113).standard_normal((B, 24, 3)).astype(np.float32), device=DEV)
    whole = m(x, noise=noise)
    stats = {k: b.clone() for k, b in m.named_buffers()}
    m2, _, _ = _modules(renderer, 111, ())
    pose_ba = m2.BAprocess.train()(x, noise=noise["ba"])
    R, T, pose_rt = m2.RTprocess.train()(x, noise={k: noise[k] for k in ("r", "eps", "t")})
    assert torch.equal(pose_ba, whole["pose_ba"]) and torch.equal(R, whole["R"]) and torch.equal(T, whole["T"]) and torch.equal(pose_rt, whole["pose_rt"])
    assert pose_ba.requires_grad and not R.requires_grad and not pose_rt.requires_grad
    for k, b in m2.named_buffers():
        assert torch.equal(b, stats[k]), k
    pose_ba.sum().backward()
    whole["pose_ba"].sum().backward()
    for (k, p), (_, q) in zip(m.named_parameters(), m2.named_parameters()):
        assert (p.grad is None) == (q.grad is None) and (p.grad is None or torch.equal(p.grad, q.grad)), k
