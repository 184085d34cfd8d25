"""Float64 restatement of the pose generator (posegen_amd/generators.py, include/posegen_generator.h) in numpy on the CPU: the trunks
(Linear -> BatchNorm1d -> LeakyReLU per layer, training and eval mode, torch's running-statistics rule), the bone-angle head and
the rotation / translation head, each forward and -- where the library has one -- a hand-written backward.  It is tested against
the reference's own numbers (tests/golden/pose_generator.npz, written by tools/gen_golden_generator.py from run_gan.py's classes)
and against float64 autograd (tests/test_generator_ref.py), and is what the device tests compare with."""
import numpy as np

from posegen_amd import generators as gen

F64 = np.float64
U32 = 2.0 ** -24
JOINT0_SCALE = 3.14 * 2                         # the reference's literal (the device multiplies by 6.28f, within half an ulp of it)


def toy_spec():
    """three ragged trunks in one launch: K below, at and past a chunk of 16, widths off a 16-column tile"""
    return gen.GenSpec([(5, 40, 1), (16, 17, 2), (33, 64, 2)])


def shipped_spec():
    """PoseGenerator: BAprocess (noise of 32), RTprocess's R and T trunks (72), width 256, two stages"""
    return gen.GenSpec([(32, 256, 2), (72, 256, 2), (72, 256, 2)])


def deep_spec():
    """four trunks of nine layers: 36 groups, the grouped weight-gradient launch's whole table; width 1, nz 1, K at and one past a
    64-wide step of the product"""
    return gen.GenSpec([(3, 1, 4), (1, 17, 4), (64, 16, 4), (65, 48, 4)])


def wide_spec():
    """nz and width at PG_GEN_MAX_DIM: the largest weight slab in LDS, 32 column tiles, 8 x 8 weight-gradient tiles"""
    return gen.GenSpec([(512, 512, 1)])


def flat_spec():
    """no stages: the stem alone; an R trunk exactly 7 wide, a T trunk narrower than a wave, one ragged trunk for a head"""
    return gen.GenSpec([(4, 7, 0), (2, 3, 0), (5, 40, 0)])


def respec(spec, **kw):
    """the same trunks with another slope, eps or momentum"""
    args = {"slope": spec.slope, "eps": spec.eps, "momentum": spec.momentum}
    args.update(kw)
    return gen.GenSpec(spec.trunks, **args)


def make_trunk(nz, width, n_stages, rng, dtype=np.float32):
    """the layers of one trunk: w, b, gamma, beta and running statistics that are not the initial ones"""
    layers = []
    for l in range(1 + 2 * n_stages):
        k = nz if l == 0 else width
        layers.append({"w": (rng.standard_normal((width, k)) / np.sqrt(k)).astype(dtype), "b": (0.1 * rng.standard_normal(width)).astype(dtype),
                       "gamma": (1.0 + 0.2 * rng.standard_normal(width)).astype(dtype), "beta": (0.1 * rng.standard_normal(width)).astype(dtype),
                       "rm": (0.1 * rng.standard_normal(width)).astype(dtype), "rv": (0.5 + rng.uniform(size=width)).astype(dtype)})
    return layers


def make_params(spec, seed, dtype=np.float32):
    rng = np.random.RandomState(seed)
    return [make_trunk(nz, width, n, rng, dtype) for nz, width, n in spec.trunks]


def make_head(n_out, width, rng, dtype=np.float32):
    return (rng.standard_normal((n_out, width)) / np.sqrt(width)).astype(dtype), (0.1 * rng.standard_normal(n_out)).astype(dtype)


def make_noise(spec, B, seed):
    rng = np.random.RandomState(seed)
    return [rng.standard_normal((B, nz)).astype(np.float32) for nz, _, _ in spec.trunks]


def make_state_dict(module, seed):
    """a state dict for `module` (a generators.HipPoseGenerator and the like) from a seed, key by key in the module's order: Linear
    weights N(0, 1/in), biases and beta 0.1 N, gamma 1 + 0.2 N, running_mean 0.1 N, running_var 0.5 + U, num_batches_tracked 3"""
    rng = np.random.RandomState(seed)
    sd = {}
    for key, t in module.state_dict().items():
        shape = tuple(t.shape)
        if key.endswith("num_batches_tracked"):
            sd[key] = np.int64(3)
        elif key.endswith("running_var"):
            sd[key] = (0.5 + rng.uniform(size=shape)).astype(np.float32)
        elif key.endswith("running_mean"):
            sd[key] = (0.1 * rng.standard_normal(shape)).astype(np.float32)
        elif len(shape) == 2:
            sd[key] = (rng.standard_normal(shape) / np.sqrt(shape[1])).astype(np.float32)
        elif "batch_norm" in key and key.endswith("weight"):
            sd[key] = (1.0 + 0.2 * rng.standard_normal(shape)).astype(np.float32)
        else:
            sd[key] = (0.1 * rng.standard_normal(shape)).astype(np.float32)
    return sd


def trunk_of_state(sd, prefix, stem, stem_bn, stages, n_stages=2):
    """the layers of one trunk out of a state dict under the reference's names"""
    names = [(stem, stem_bn)]
    for i in range(n_stages):
        names += [(f"{stages}.{i}.w1", f"{stages}.{i}.batch_norm1"), (f"{stages}.{i}.w2", f"{stages}.{i}.batch_norm2")]
    return [{"w": np.asarray(sd[f"{prefix}{lin}.weight"]), "b": np.asarray(sd[f"{prefix}{lin}.bias"]), "gamma": np.asarray(sd[f"{prefix}{bn}.weight"]),
             "beta": np.asarray(sd[f"{prefix}{bn}.bias"]), "rm": np.asarray(sd[f"{prefix}{bn}.running_mean"]),
             "rv": np.asarray(sd[f"{prefix}{bn}.running_var"]), "names": (f"{prefix}{lin}", f"{prefix}{bn}")} for lin, bn in names]


def pose_generator_trunks(sd):
    """(BA, R, T) trunks of a PoseGenerator state dict"""
    return [trunk_of_state(sd, "BAprocess.", "w1", "batch_norm1", "linear_stages"),
            trunk_of_state(sd, "RTprocess.", "w1_R", "batch_norm_R", "linear_stages_R"),
            trunk_of_state(sd, "RTprocess.", "w1_T", "batch_norm_T", "linear_stages_T")]


def leaky(y, slope):
    return np.where(y > 0, y, y * slope)


def bn_statistics(z, layer, eps, training):
    """(mean, biased var, scale, shift) of one layer in float64"""
    if training:
        mean, var = z.mean(0), z.var(0)
    else:
        mean, var = np.asarray(layer["rm"], F64), np.asarray(layer["rv"], F64)
    scale = np.asarray(layer["gamma"], F64) / np.sqrt(var + eps)
    return mean, var, scale, np.asarray(layer["beta"], F64) - mean * scale


def running_update(layer, mean, var, B, momentum):
    """torch's rule: (1 - m) old + m new, the unbiased variance for running_var"""
    return ((1.0 - momentum) * np.asarray(layer["rm"], F64) + momentum * mean,
            (1.0 - momentum) * np.asarray(layer["rv"], F64) + momentum * var * (B / (B - 1.0)))


def trunk_forward(layers, noise, slope=0.01, eps=1e-5, momentum=0.1, training=True):
    """-> (h [B,width] the trunk's output, tape: per layer z, mean, var, scale, shift, h_in, and the running statistics after)"""
    h = np.asarray(noise, F64)
    B = h.shape[0]
    tape = []
    for layer in layers:
        z = h @ np.asarray(layer["w"], F64).T + np.asarray(layer["b"], F64)
        mean, var, scale, shift = bn_statistics(z, layer, eps, training)
        rm, rv = running_update(layer, mean, var, B, momentum) if training else (np.asarray(layer["rm"], F64), np.asarray(layer["rv"], F64))
        y = z * scale + shift
        tape.append({"h_in": h, "z": z, "mean": mean, "var": var, "scale": scale, "shift": shift, "y": y, "rm": rm, "rv": rv})
        h = leaky(y, slope)
    return h, tape


def masks_of(tape):
    return [t["y"] > 0 for t in tape]


def trunk_backward(layers, tape, d_out, slope=0.01, eps=1e-5, masks=None):
    """the backward of a training-mode trunk_forward at the cotangent d_out of its output; `masks`: per layer where the
    pre-activation counts as positive (None: the tape's own) -> per layer (dw, db, dgamma, dbeta)"""
    masks = masks_of(tape) if masks is None else masks
    dh = np.asarray(d_out, F64)
    B = dh.shape[0]
    grads = [None] * len(layers)
    for l in range(len(layers) - 1, -1, -1):
        t = tape[l]
        dy = dh * np.where(masks[l], 1.0, slope)
        xh = (t["z"] - t["mean"]) / np.sqrt(t["var"] + eps)
        dbeta, dgamma = dy.sum(0), (dy * xh).sum(0)
        dz = t["scale"] / B * (B * dy - dbeta - xh * dgamma)
        grads[l] = (dz.T @ t["h_in"], dz.sum(0), dgamma, dbeta)
        dh = dz @ np.asarray(layers[l]["w"], F64)
    return grads


def ba_head(h, w2, b2):
    """-> (y [B,4J], pose [B,J,3])"""
    y = np.asarray(h, F64) @ np.asarray(w2, F64).T + np.asarray(b2, F64)
    return y, ba_pose(y)


def ba_pose(y):
    y4 = np.asarray(y, F64).reshape(y.shape[0], -1, 4)
    with np.errstate(invalid="ignore", divide="ignore"):
        pose = y4[:, :, :3] / np.linalg.norm(y4[:, :, :3], axis=-1, keepdims=True) * y4[:, :, 3:4]
    pose[:, 0] *= JOINT0_SCALE
    return pose


def ba_head_dy(y, d_pose):
    """d y of the head's epilogue: d a = s theta (g - a^ (a^ . g)) / |a|, d theta = s a^ . g"""
    y4, g = np.asarray(y, F64).reshape(y.shape[0], -1, 4), np.asarray(d_pose, F64)
    s = np.ones((1, y4.shape[1], 1))
    s[0, 0, 0] = JOINT0_SCALE
    nrm = np.linalg.norm(y4[:, :, :3], axis=-1, keepdims=True)
    u = y4[:, :, :3] / nrm
    ug = (u * g).sum(-1, keepdims=True)
    return np.concatenate([s * y4[:, :, 3:4] * (g - u * ug) / nrm, s * ug], -1).reshape(y.shape[0], -1)


def ba_head_backward(h, w2, y, d_pose):
    """-> (d_w2, d_b2, d_h)"""
    dy = ba_head_dy(y, d_pose)
    return dy.T @ np.asarray(h, F64), dy.sum(0), dy @ np.asarray(w2, F64)


def axis_angle_to_matrix(rv):
    """pytorch3d.transforms.axis_angle_to_matrix in float64, restated: rotation vector -> quaternion (w, x, y, z) with
    sin(angle / 2) / angle (below 1e-6: 1/2 - angle^2 / 48) -> matrix with two_s = 2 / |q|^2"""
    rv = np.asarray(rv, F64)
    ang = np.linalg.norm(rv, axis=-1, keepdims=True)
    half = 0.5 * ang
    small = np.abs(ang) < 1e-6
    with np.errstate(invalid="ignore", divide="ignore"):
        k = np.where(small, 0.5 - ang * ang / 48.0, np.sin(half) / np.where(small, 1.0, ang))
    q = np.concatenate([np.cos(half), rv * k], -1)
    r, i, j, kk = q[..., 0], q[..., 1], q[..., 2], q[..., 3]
    two_s = 2.0 / (q * q).sum(-1)
    o = np.stack([1 - two_s * (j * j + kk * kk), two_s * (i * j - kk * r), two_s * (i * kk + j * r),
                  two_s * (i * j + kk * r), 1 - two_s * (i * i + kk * kk), two_s * (j * kk - i * r),
                  two_s * (i * kk - j * r), two_s * (j * kk + i * r), 1 - two_s * (i * i + j * j)], -1)
    return o.reshape(rv.shape[:-1] + (3, 3))


def rt_head(r, h_t, w2_t, b2_t, eps, x):
    """RTGenerator's tail: r [B,>=7] the R trunk's output, h_t the T trunk's -> (R [B,3,3], T [B,3], pose_rt [B,J,3])"""
    r, x = np.asarray(r, F64), np.asarray(x, F64)
    axis = r[:, 0:3] + r[:, 3:6] * r[:, 3:6] * np.asarray(eps, F64)
    axis = axis / np.linalg.norm(axis, axis=-1, keepdims=True) * r[:, 6:7]
    R = axis_angle_to_matrix(axis)
    t = np.asarray(h_t, F64) @ np.asarray(w2_t, F64).T + np.asarray(b2_t, F64)
    t[:, 2] = t[:, 2] * t[:, 2]
    xc = x - x[:, :1]
    return R, t, np.einsum("bcd,bjd->bjc", R, xc) + t[:, None, :]


def pose_generator(sd, x, noise, training=True, slope=0.01, eps=1e-5, momentum=0.1):
    """PoseGenerator.forward on a state dict (numpy arrays) at the draws `noise` (ba, r, eps, t)
    -> (outputs dict, the three trunks' tapes, the three trunks' layers)"""
    trunks = pose_generator_trunks(sd)
    outs, tapes = zip(*[trunk_forward(layers, noise[k], slope, eps, momentum, training) for layers, k in zip(trunks, ("ba", "r", "t"))])
    y, pose_ba = ba_head(outs[0], sd["BAprocess.w2.weight"], sd["BAprocess.w2.bias"])
    R, T, pose_rt = rt_head(outs[1], outs[2], sd["RTprocess.w2_T.weight"], sd["RTprocess.w2_T.bias"], noise["eps"], x)
    return {"pose_ba": pose_ba, "y": y, "R": R, "T": T, "pose_rt": pose_rt, "h": outs}, tapes, trunks


def pose_generator_backward(sd, out, tapes, trunks, d_pose, slope=0.01, eps=1e-5, masks=None):
    """the gradients of every parameter that has one, by state-dict key (the RT parameters and w2_R have none)"""
    d_w2, d_b2, d_h = ba_head_backward(out["h"][0], sd["BAprocess.w2.weight"], out["y"], d_pose)
    grads = {"BAprocess.w2.weight": d_w2, "BAprocess.w2.bias": d_b2}
    for layer, (dw, db, dgamma, dbeta) in zip(trunks[0], trunk_backward(trunks[0], tapes[0], d_h, slope, eps, masks)):
        lin, bn = layer["names"]
        grads[lin + ".weight"], grads[lin + ".bias"], grads[bn + ".weight"], grads[bn + ".bias"] = dw, db, dgamma, dbeta
    return grads


def grad_sample_index(numel, k=8):
    """the k flat entries of a parameter gradient the fixture keeps"""
    return np.unique(np.linspace(0, numel - 1, k).astype(np.int64))


# ---- parameter edits: the degenerate columns of training ---------------------------------------------------------------------------------
def _copied(params):
    return [[{k: (np.array(v, copy=True) if isinstance(v, np.ndarray) else v) for k, v in layer.items()} for layer in layers] for layers in params]


def zero_weight_row(params, t, l, col):
    """a copy of `params` with row `col` of layer l of trunk t's weight zeroed: that column's Z is the bias on every row, its variance 0"""
    out = _copied(params)
    out[t][l]["w"][col, :] = 0.0
    return out


def dead_gamma(params, t, l, cols, betas):
    """a copy with gamma = 0 and beta = `betas` on the columns `cols` of layer l of trunk t: the pre-activation is exactly beta"""
    out = _copied(params)
    out[t][l]["gamma"][list(cols)] = 0.0
    out[t][l]["beta"][list(cols)] = np.asarray(betas, out[t][l]["beta"].dtype)
    return out


def last_layer_output(params, t, pre):
    """a copy whose trunk t puts out exactly lrelu(pre) on its first len(pre) columns: gamma = 0, beta = pre on the last layer"""
    return dead_gamma(params, t, len(params[t]) - 1, range(len(pre)), pre)


# On the top layer of each trunk: below a BatchNorm the column sums of dZ are 0, so the d_beta of a column whose mask is the same on
# every row is 0 whatever the mask says; only the top layer's d_beta = s sum(cot) shows which way an exactly-zero pre-activation went.
GAMMA0_BETAS = (0.0, -0.0, 0.3, -0.3)


def gamma0_columns(width):
    """the four columns the gamma = 0 cases use: the first tile's ends and the last two of the trunk (a ragged tile's where there is one)"""
    return (0, min(3, width - 3), width - 2, width - 1)


# ---- the backward with a carried bound -----------------------------------------------------------------------------------------------------
D53 = 2.0 ** -53


def rebuilt_tape(noise, records, slope):
    """A tape for the backward from per-layer records {z, mean, var, scale, shift} (the device's own, read back, or
    emulate32_forward's): h_in of layer l is lrelu(z scale + shift) of layer l - 1 in float64 -- the product of two float32 values
    is exact in double, so this is the device's fmaf up to its one rounding -- and y the layer's own pre-activation."""
    tape, h = [], np.asarray(noise, F64)
    for r in records:
        z, sc, sh = (np.asarray(r[k], F64) for k in ("z", "scale", "shift"))
        y = z * sc + sh
        tape.append({"h_in": h, "z": z, "mean": np.asarray(r["mean"], F64), "var": np.asarray(r["var"], F64), "scale": sc, "shift": sh, "y": y})
        h = leaky(y, slope)
    return tape


def trunk_backward_with_bound(layers, tape, masks, d_out, slope, eps):
    """The float64 backward of one trunk from a GIVEN tape (rebuilt_tape of the device's Z, mean, var, scale, shift: the forward's
    error does not enter) and GIVEN masks (the device's fmaf(Z, scale, shift) > 0), at the cotangent d_out [B,width], with an
    elementwise bound on what pg_gen.hip's float32 backward of the same chain may differ by, carried down the chain.
    slope, eps: as the kernels hold them (float32 values).  u = 2^-24; E_X bounds the device's X; a float32 reduction of length n
    is bounded by (n + 2) u sum |a| |b| (tests/test_gpu_generator.py's _layer_bound); sums run over the B rows of a column.
        top layer      dY = fl32(cot s), s = 1 or the slope per the mask                E_Y = u |dY|
        below it       dH_l = dZ_{l+1} W_{l+1}  (N = width products, float32)           E_H = E_Z |W| + (N + 2) u (|dZ| + E_Z) |W|
                       dY = fl32(dH s)                                                   E_Y = E_H |s| + u |dY|
        d_beta         = sum dY in double, rounded once                                  E_beta  = sum E_Y + u (|d_beta| + sum E_Y) + B 2^-53 sum |dY|
        d_gamma        = sum dY x^ in double, x^ = (Z - mean) / sqrt(var + eps)          E_gamma = sum E_Y |x^| + u (|d_gamma| + sum E_Y |x^|)
                         from the tape's doubles, rounded once                                     + B 2^-53 sum |dY| |x^|
        dZ             = fl32(k (B dY - d_beta - x^ d_gamma)), k = gamma / sqrt(var + eps) / B, in double from the unrounded sums
                                                                                         E_Z = |k| (B E_Y + sum E_Y + |x^| sum E_Y |x^|) + u |dZ|
                                                                                               + (B + 8) 2^-53 |k| (B |dY| + sum |dY| + |x^| sum |dY| |x^|)
        dW_l           = dZ_l^T H_{l-1}, H recomputed on load (one fused multiply-add and one product: dH = 2 u |H|; the stem's
                         H is the noise itself, dH = 0), B products in float32       E_W = E_Z^T |H| + (|dZ| + E_Z)^T dH + (B + 2) u (|dZ| + E_Z)^T |H|
        db_l           = colsum(dZ) in double, rounded once.  The exact value is 0 whatever dY was (the unrounded terms of a column
                         of dZ sum to -d_gamma k sum x^ = 0), so what the device has is the float32 rounding of each dZ:
                                                                                         E_b = (2 u + 2^-40) sum |dZ| + 2^-149   (absolute)
    A column whose variance is 0 has x^ = 0 exactly: its d_gamma is 0 with a bound of 0.  A column with gamma = 0 has k = 0: dZ,
    its dW row and db are 0 with a bound of 0 (db: 2^-149).
    -> grads: per layer (dw, db, dgamma, dbeta); bounds: the same shapes"""
    dh = np.asarray(d_out, F64)
    B = dh.shape[0]
    e_h = np.zeros_like(dh)
    grads, bounds = [None] * len(layers), [None] * len(layers)
    for l in range(len(layers) - 1, -1, -1):
        t = tape[l]
        s = np.where(masks[l], 1.0, slope)
        dy = dh * s
        e_y = e_h * np.abs(s) + U32 * np.abs(dy)
        invstd = 1.0 / np.sqrt(t["var"] + eps)
        xh = (t["z"] - t["mean"]) * invstd
        axh, ady = np.abs(xh), np.abs(dy)
        dbeta, dgamma = dy.sum(0), (dy * xh).sum(0)
        se, sex, sa, sax = e_y.sum(0), (e_y * axh).sum(0), ady.sum(0), (ady * axh).sum(0)
        e_beta = se + U32 * (np.abs(dbeta) + se) + B * D53 * sa
        e_gamma = sex + U32 * (np.abs(dgamma) + sex) + B * D53 * sax
        k = np.asarray(layers[l]["gamma"], F64) * invstd / B
        dz = k * (B * dy - dbeta - xh * dgamma)
        e_z = np.abs(k) * (B * e_y + se + axh * sex) + U32 * np.abs(dz) + (B + 8) * D53 * np.abs(k) * (B * ady + sa + axh * sax)
        h = np.asarray(t["h_in"], F64)
        ah, mag = np.abs(h), np.abs(dz) + e_z
        d_h = 2 * U32 * ah if l else np.zeros_like(ah)
        w = np.asarray(layers[l]["w"], F64)
        grads[l] = (dz.T @ h, dz.sum(0), dgamma, dbeta)
        bounds[l] = (e_z.T @ ah + mag.T @ d_h + (B + 2) * U32 * (mag.T @ ah), (2 * U32 + 2.0 ** -40) * np.abs(dz).sum(0) + 2.0 ** -149, e_gamma, e_beta)
        dh = dz @ w
        e_h = e_z @ np.abs(w) + (w.shape[0] + 2) * U32 * (mag @ np.abs(w))
    return grads, bounds


def ba_head_backward_with_bound(h, w2, y, d_pose):
    """The float64 backward of the bone-angle head from the device's own y [B,4J] and the trunk's output h rebuilt from the device's
    tape, with the bound on pg_gen.hip's float32 results:
        dy     formed in double from y and d_pose, rounded once          E_dy = u |dy| + 16 2^-53 |f| (|g| + |a^| sum |a^| |g|)   (f = s theta / |a|; the
                                                                                angle's entry: 16 2^-53 s sum |a^| |g|)
        d_b2   = colsum(dy) in double, rounded once                       E = sum E_dy + u (|d_b2| + sum E_dy) + B 2^-53 sum |dy|
        d_w2   = dy^T H, H recomputed on load (dH = 2 u |H|)              E = E_dy^T |H| + (|dy| + E_dy)^T dH + (B + 2) u (|dy| + E_dy)^T |H|
        d_h    = dy w2, a float32 reduction of length 4J                  E = E_dy |w2| + (4J + 2) u (|dy| + E_dy) |w2|
    A joint with |a| = 0 has a NaN dy: its entries of d_w2 and d_b2 and every d_h of the row are NaN in value and in bound.
    -> (d_w2, d_b2, d_h), (their bounds)"""
    h, w2, y = np.asarray(h, F64), np.asarray(w2, F64), np.asarray(y, F64)
    B = h.shape[0]
    y4, g = y.reshape(B, -1, 4), np.asarray(d_pose, F64)
    with np.errstate(invalid="ignore", divide="ignore"):
        dy = ba_head_dy(y, d_pose)
        s = np.ones((1, y4.shape[1], 1))
        s[0, 0, 0] = JOINT0_SCALE
        nrm = np.linalg.norm(y4[:, :, :3], axis=-1, keepdims=True)
        ua = np.abs(y4[:, :, :3] / nrm)
        uag = (ua * np.abs(g)).sum(-1, keepdims=True)
        dbl = np.concatenate([np.abs(s * y4[:, :, 3:4] / nrm) * (np.abs(g) + ua * uag), s * uag], -1).reshape(B, -1)
        e_dy = U32 * np.abs(dy) + 16 * D53 * dbl
        ah, mag = np.abs(h), np.abs(dy) + e_dy
        d_b2 = dy.sum(0)
        se = e_dy.sum(0)
        grads = (dy.T @ h, d_b2, dy @ w2)
        bounds = (e_dy.T @ ah + mag.T @ (2 * U32 * ah) + (B + 2) * U32 * (mag.T @ ah), se + U32 * (np.abs(d_b2) + se) + B * D53 * np.abs(dy).sum(0),
                  e_dy @ np.abs(w2) + (w2.shape[0] + 2) * U32 * (mag @ np.abs(w2)))
    return grads, bounds


# ---- the same chain in float32 on the CPU: what honest float32 does inside the bound, and what planted errors do outside it ---------------
F32 = np.float32
MUTANTS = ("unbiased x^", "scale32 k", "no x^ d_gamma", "short last column")


def _act32(z, scale, shift, slope):
    """lrelu(fmaf(z, scale, shift)) as the kernels form it: the fused value rounded once (the product is exact in double), then
    one float32 product by the slope"""
    y = (np.asarray(z, F64) * np.asarray(scale, F64) + np.asarray(shift, F64)).astype(F32)
    return np.where(y > 0, y, y * F32(slope))


def emulate32_forward(layers, noise, slope, eps):
    """the training-mode forward of a trunk the way the device runs it, in numpy: Z in float32 (plain `@`), mean and the biased
    variance of that Z in double, scale and shift formed in double and rounded once -> per layer {z, mean, var, scale, shift}"""
    h, out = np.asarray(noise, F32), []
    for layer in layers:
        z = h @ np.asarray(layer["w"], F32).T + np.asarray(layer["b"], F32)
        z64 = z.astype(F64)
        mean = z64.mean(0)
        var = ((z64 - mean) ** 2).mean(0)
        sc = np.asarray(layer["gamma"], F64) / np.sqrt(var + eps)
        out.append({"z": z, "mean": mean, "var": var, "scale": sc.astype(F32), "shift": (np.asarray(layer["beta"], F64) - mean * sc).astype(F32)})
        h = _act32(z, out[-1]["scale"], out[-1]["shift"], slope)
    return out


def emulate32_backward(layers, tape, masks, d_out, slope, eps, mutant=None):
    """trunk_backward_with_bound's chain as pg_gen.hip runs it, in numpy float32 with the double sums kept in float64; plain `@` for
    the products, not the device's order.  It exists so that the bound can be judged without a device: honest float32 must stay
    inside it, and each planted error (`mutant`, one of MUTANTS) must leave it:
        "unbiased x^"         x^ from the unbiased variance
        "scale32 k"           k from the tape's rounded float32 scale in place of gamma / sqrt(var + eps)
        "no x^ d_gamma"       dZ without its third term
        "short last column"   the last live column of a ragged 16-column tile summed over B - 1 rows
    -> per layer (dw, db, dgamma, dbeta) as float32"""
    assert mutant is None or mutant in MUTANTS
    dh = np.asarray(d_out, F32)
    B = dh.shape[0]
    grads = [None] * len(layers)
    for l in range(len(layers) - 1, -1, -1):
        t = tape[l]
        dy = dh * np.where(masks[l], F32(1.0), F32(slope))
        invstd = 1.0 / np.sqrt(t["var"] + eps)
        xh = (t["z"] - t["mean"]) * (1.0 / np.sqrt(t["var"] * (B / (B - 1.0)) + eps) if mutant == "unbiased x^" else invstd)
        dy64 = dy.astype(F64)
        dbeta, dgamma = dy64.sum(0), (dy64 * xh).sum(0)
        if mutant == "short last column" and dy.shape[1] % 16:
            dbeta[-1] = dy64[:-1, -1].sum()
        k = (np.asarray(t["scale"], F64) if mutant == "scale32 k" else np.asarray(layers[l]["gamma"], F64) * invstd) / B
        dz = (k * (B * dy64 - dbeta - (0.0 if mutant == "no x^ d_gamma" else xh * dgamma))).astype(F32)
        h = np.asarray(t["h_in"], F32) if l == 0 else _act32(tape[l - 1]["z"], tape[l - 1]["scale"], tape[l - 1]["shift"], slope)
        grads[l] = (dz.T @ h, dz.astype(F64).sum(0).astype(F32), dgamma.astype(F32), dbeta.astype(F32))
        dh = dz @ np.asarray(layers[l]["w"], F32)
    return grads


def emulate32_head_backward(tape_last, w2, y, d_pose, slope):
    """ba_head_backward_with_bound's chain in float32: dy in double rounded once, H recomputed from the last layer's tape -> (d_w2, d_b2, d_h)"""
    with np.errstate(invalid="ignore", divide="ignore"):
        dy = ba_head_dy(np.asarray(y, F64), d_pose).astype(F32)
        h = _act32(tape_last["z"], tape_last["scale"], tape_last["shift"], slope)
        return dy.T @ h, dy.astype(F64).sum(0).astype(F32), dy @ np.asarray(w2, F32)


# ---- the cases of tests/test_gpu_generator_edges.py, judged on the CPU by tests/test_generator_ref.py ---------------------------------------
EDGE_SPECS = {"toy": toy_spec, "deep": deep_spec, "flat": flat_spec, "wide": wide_spec}
EDGE_BATCHES = {"toy": (2, 17, 65, 257), "deep": (2, 17, 65, 257), "flat": (2, 17, 65, 257), "wide": (2, 18)}
EDGE_SEEDS = {"toy": 200, "deep": 300, "flat": 400, "wide": 500}
ROW_LIMIT_SPEC = [(2, 3, 0)]
DEGENERATE = ("zero row stem", "zero row middle", "gamma 0", "twin rows") + tuple(f"slope {s} eps {e}" for s in (0.0, 1.0, 0.2) for e in (1e-12, 1.0))
HEAD_CASES = (("toy", 65, 1), ("toy", 65, 5), ("toy", 65, 64), ("wide", 18, 64), ("wide", 18, 1))     # (spec, B, J), the head on trunk 0


def zero_row_column(width, l):
    """the column whose weight row the zero-row cases clear: column 1 in the stem, the last column (a ragged tile's) in layer 1"""
    return 1 if l == 0 else width - 1


def edge_case(name, B=None):
    """-> (spec, params, noise, cots): one case of the edge tests by name -- a key of EDGE_SPECS at a batch of EDGE_BATCHES, "rows"
    (the row limit; B may shorten it), or one of DEGENERATE (the toy spec at B = 65, edited)"""
    if name in EDGE_SPECS:
        spec, seed = EDGE_SPECS[name](), EDGE_SEEDS[name] + B
        params = make_params(spec, EDGE_SEEDS[name])
    elif name == "rows":
        spec, B = gen.GenSpec(ROW_LIMIT_SPEC), (1 << 20) if B is None else B
        params, seed = make_params(spec, 600), 601
    else:
        spec, B, seed = toy_spec(), 2 if name == "twin rows" else 65, 700 + DEGENERATE.index(name)
        params = make_params(spec, 700)
        if name.startswith("zero row"):
            l = 0 if name.endswith("stem") else 1
            for t, (_, width, _) in enumerate(spec.trunks):
                params = zero_weight_row(params, t, l, zero_row_column(width, l))
        elif name == "gamma 0":
            for t, (_, width, _) in enumerate(spec.trunks):
                params = dead_gamma(params, t, spec.layers(t) - 1, gamma0_columns(width), GAMMA0_BETAS)   # (the top layer: see GAMMA0_BETAS)
        elif name.startswith("slope"):
            spec = respec(spec, slope=float(name.split()[1]), eps=float(name.split()[3]))
    noise = make_noise(spec, B, seed)
    if name == "twin rows":
        noise = [np.repeat(n[:1], 2, axis=0) for n in noise]
    rng = np.random.RandomState(seed + 1)
    return spec, params, noise, [rng.standard_normal((B, width)).astype(np.float32) for _, width, _ in spec.trunks]


def held(spec):
    """slope and eps as the kernels hold them: the float32 values, as doubles"""
    return float(np.float32(spec.slope)), float(np.float32(spec.eps))


def ragged_module_case(renderer=None):
    """HipBAGenerator(noise 5, width 40, one stage) with a seeded state dict, its draws and the cotangent of its pose at B = 65
    -> (module on the CPU, state dict, spec, the trunk's layers, noise [65,5], d_pose [65,24,3])"""
    m = gen.HipBAGenerator(noise_channle=5, linear_size=40, num_stage=1, renderer=renderer)
    sd = make_state_dict(m, 890)
    rng = np.random.RandomState(891)
    noise, d_pose = rng.standard_normal((65, 5)).astype(np.float32), rng.standard_normal((65, 24, 3)).astype(np.float32)
    return m, sd, gen.GenSpec([(5, 40, 1)]), trunk_of_state(sd, "", "w1", "batch_norm1", "linear_stages", n_stages=1), noise, d_pose
