"""Float64 restatement of the adversarial game (posegen_amd/discriminators.py, include/posegen_gan.h), in torch on the CPU: the
part-path discriminators forward, a hand-written backward that takes the activation masks as an argument (and the same with an
elementwise float32 error bound carried down the chain), the two losses with the discriminator accuracy, and the pool at given
draws.  A plain helper module; tests/test_gan_ref.py checks it against the reference's
own numbers (tests/golden/pose_discriminators.npz) and against float64 autograd.

Parameters are a list per path of five (W [out,in], b [out]) pairs; a spec is a `posegen_amd.discriminators.PartSpec`."""
import math

import numpy as np
import torch

F64 = torch.float64


def toy_spec():
    """two narrow paths over [0,5,23] and all 24 rows: rows 1-4, 6-22 of d_x meet the second path only, and a spec that leaves rows
    unselected is `toy_spec_sparse`"""
    from posegen_amd.discriminators import PartSpec
    return PartSpec(24, 3, [("part", [0, 5, 23], 20, 36), ("all", list(range(24)), 20, 36)])


def toy_spec_sparse():
    """two paths that leave most rows unselected: [0,5,23] and [5,7]"""
    from posegen_amd.discriminators import PartSpec
    return PartSpec(24, 3, [("part", [0, 5, 23], 20, 36), ("pair", [5, 7], 20, 36)])


def ragged3_spec():
    """eight paths of different (width, mid) over five 3-D rows, in one launch: K = 3, 9, 15, 6, 3, 6, 9, 6 into layer 1, widths
    below, at and one past a chunk of 16, a round of 64 and a tile of 64, odd widths, repeated rows"""
    from posegen_amd.discriminators import PartSpec
    return PartSpec(5, 3, [("a", [0], 1, 1),                      # K = 3, N = 1 everywhere
                           ("b", [4, 4, 2], 67, 130),             # odd width; two rounds (64 + 3); a repeated row; three column tiles
                           ("c", [0, 1, 2, 3, 4], 64, 16),        # K = 15; exactly one tile
                           ("d", [1, 3], 129, 65),                # three rounds (64 + 64 + 1); one column past a tile
                           ("e", [2], 17, 80),                    # one column past a chunk
                           ("f", [3, 0], 80, 63),                 # five chunks, the fifth in accumulator 0 again
                           ("g", [4, 1, 0], 16, 64),              # exactly one chunk
                           ("h", [2, 2], 33, 5)])                 # a repeated row only


def ragged2_spec():
    """two 2-D paths: all 24 rows (K = 48) into width 65, and one row (K = 2) into width 3"""
    from posegen_amd.discriminators import PartSpec
    return PartSpec(24, 2, [("wide", list(range(24)), 65, 3), ("last", [23], 3, 67)])


def one_path_spec(spec, p):
    """path p of `spec` as a spec of its own"""
    from posegen_amd.discriminators import PartSpec
    return PartSpec(spec.n_points, spec.point_dim, [spec.paths[p]], slope=spec.slope)


def make_params(spec, seed, dtype=np.float32):
    """Weights as `init_weights` makes them (kaiming_normal_: N(0, 2 / fan_in)), biases as nn.Linear leaves them (uniform within
    1 / sqrt(fan_in)), from the project's own generator np.random.RandomState(seed); float32 values"""
    rng = np.random.RandomState(seed)
    params = []
    for p in range(len(spec.paths)):
        layers = []
        for n_out, n_in in spec.layer_shapes(p):
            w = (rng.standard_normal((n_out, n_in)) * math.sqrt(2.0 / n_in)).astype(dtype)
            b = rng.uniform(-1.0 / math.sqrt(n_in), 1.0 / math.sqrt(n_in), n_out).astype(dtype)
            layers.append((w, b))
        params.append(layers)
    return params


def make_inputs(spec, B, seed):
    """poses N(0, 0.6^2) as float32 [B,n_points,point_dim]"""
    return (np.random.RandomState(seed).standard_normal((B, spec.n_points, spec.point_dim)) * 0.6).astype(np.float32)


def load_params(module, params):
    """the restatement's parameters into a `PartDiscriminator` (or anything with its `path_linears`)"""
    with torch.no_grad():
        for p, layers in enumerate(params):
            for lin, (w, b) in zip(module.path_linears(p), layers):
                lin.weight.copy_(torch.as_tensor(w))
                lin.bias.copy_(torch.as_tensor(b))


def t64(a, dtype=F64):
    return torch.as_tensor(np.asarray(a)).to(dtype)


def leaky(z, slope):
    return torch.where(z > 0, z, z * slope)


def path_input(spec, p, x):
    """the rows path p gathers, flattened: [B, n_sel point_dim]"""
    return x[:, spec.paths[p][1], :].reshape(x.shape[0], -1)


def layer(h_in, w, b, slope, act=True):
    z = h_in @ w.T + b
    return leaky(z, slope) if act else z


def forward(spec, params, x, dtype=F64):
    """-> pred [B,n_paths], tapes: per path the four post-activation layers.  Everything in `dtype`: float64, or float32 for torch's
    own float32 arithmetic on the CPU as the yardstick of an end-to-end error."""
    x = t64(x, dtype)
    preds, tapes = [], []
    for p, layers in enumerate(params):
        h, tape = path_input(spec, p, x), []
        for w, b in layers[:4]:
            h = layer(h, t64(w, dtype), t64(b, dtype), spec.slope)
            tape.append(h)
        preds.append(layer(h, t64(layers[4][0], dtype), t64(layers[4][1], dtype), spec.slope, act=False))
        tapes.append(tape)
    return torch.cat(preds, 1), tapes


def masks_of(tapes):
    """the activation masks a tape implies: > 0 (at exactly 0 the slope applies, as torch)"""
    return [[torch.as_tensor(np.asarray(h)) > 0 for h in tape] for tape in tapes]


def backward(spec, params, x, tapes, masks, d_pred, dtype=F64, dz_out=None):
    """The backward by hand at the cotangent d_pred [B,n_paths]: dZ = dH (mask ? 1 : slope) with the masks GIVEN (so that the device's
    own decisions at LeakyReLU's kink can be fed in), tapes = the layer inputs.  -> d_x [B,n_points,point_dim], grads: per path five
    (dW, db).  `dz_out`: a list that receives, per path, the five layers' dZ."""
    x, d_pred = t64(x, dtype), t64(d_pred, dtype)
    d_x = torch.zeros_like(x)
    grads = []
    for p, layers in enumerate(params):
        ins = [path_input(spec, p, x)] + [t64(h, dtype) for h in tapes[p]]
        dz = d_pred[:, p:p + 1]
        g, dzs = [None] * 5, [None] * 5
        for l in range(4, -1, -1):
            g[l], dzs[l] = (dz.T @ ins[l], dz.sum(0)), dz
            dh = dz @ t64(layers[l][0], dtype)
            if l:
                m = torch.as_tensor(np.asarray(masks[p][l - 1]))
                dz = dh * torch.where(m, torch.ones((), dtype=dtype), torch.full((), spec.slope, dtype=dtype))
        sel = spec.paths[p][1]
        dh = dh.reshape(x.shape[0], len(sel), spec.point_dim)
        for i, j in enumerate(sel):
            d_x[:, j, :] += dh[:, i, :]
        grads.append(g)
        if dz_out is not None:
            dz_out.append(dzs)
    return d_x, grads


U32 = 2.0 ** -24


def gamma(n):
    """n u / (1 - n u) at float32's unit roundoff: what n roundings in a row can lose, relatively"""
    return n * U32 / (1.0 - n * U32)


def backward_with_bound(spec, params, x, tapes, masks, d_pred):
    """The float64 backward from GIVEN tapes (the layer inputs: the device's own, so that its forward error does not enter) and
    masks, with an elementwise bound on what a float32 backward of the same chain may differ by, carried down the chain.
    With E_l the bound on the float32 dZ_l (E = 0 at the head: the cotangent is given), N_l outputs and layer input H_{l-1}:
        E(dW_l)     = E_l^T |H_{l-1}| + gamma(B + 1) (|dZ_l| + E_l)^T |H_{l-1}|      B products and B additions in any order
        E(db_l)     = colsum(E_l) + u (|db_l| + colsum(E_l))                          a double sum, rounded once
        E(dH_{l-1}) = E_l |W_l| + gamma(N_l + 1) (|dZ_l| + E_l) |W_l|
        E_{l-1}     = E(dH_{l-1}) |s| + u |dZ_{l-1}|                                  s = 1 or the slope per the mask; one product
        E(d_x)      = scatter(E(dH_0)) + gamma(c) scatter(|dH_0| + E(dH_0))           c contributions to the row, added in float32
    -> d_x, grads (as `backward`), E_dx, E_grads (the same shapes).  A row that no path selects has a bound of 0."""
    x, d_pred = t64(x), t64(d_pred)
    B = x.shape[0]
    d_x, e_dx, mag, count = torch.zeros_like(x), torch.zeros_like(x), torch.zeros_like(x), torch.zeros(spec.n_points, dtype=F64)
    grads, bounds = [], []
    for p, layers in enumerate(params):
        ins = [path_input(spec, p, x)] + [t64(h) for h in tapes[p]]
        dz, e = d_pred[:, p:p + 1], torch.zeros(B, 1, dtype=F64)
        g, eg = [None] * 5, [None] * 5
        for l in range(4, -1, -1):
            w, h = t64(layers[l][0]), ins[l].abs()
            db = dz.sum(0)
            g[l] = (dz.T @ ins[l], db)
            eg[l] = (e.T @ h + gamma(B + 1) * ((dz.abs() + e).T @ h), e.sum(0) + U32 * (db.abs() + e.sum(0)))
            dh = dz @ w
            e_dh = e @ w.abs() + gamma(w.shape[0] + 1) * ((dz.abs() + e) @ w.abs())
            if l:
                s = torch.where(torch.as_tensor(np.asarray(masks[p][l - 1])), torch.ones((), dtype=F64), torch.full((), spec.slope, dtype=F64))
                dz = dh * s
                e = e_dh * s.abs() + U32 * dz.abs()
        sel = spec.paths[p][1]
        dh, e_dh = dh.reshape(B, len(sel), spec.point_dim), e_dh.reshape(B, len(sel), spec.point_dim)
        for i, j in enumerate(sel):
            d_x[:, j, :] += dh[:, i, :]
            e_dx[:, j, :] += e_dh[:, i, :]
            mag[:, j, :] += dh[:, i, :].abs() + e_dh[:, i, :]
            count[j] += 1
        grads.append(g)
        bounds.append(eg)
    return d_x, grads, e_dx + gamma(count)[None, :, None] * mag, bounds


def lsgan(pred, label, weight=1.0):
    """(weight mean((pred - label)^2) in float64, the count of |pred - label| <= 0.5 compared in float32 as numpy does in
    get_discriminator_accuracy, n, d_pred = weight 2 (pred - label) / n).  A NaN counts as wrong (pg_disc_loss's `<=`); the
    reference's `np.where(rlt > 0.5, 0, 1)` would count it as right -- the only value on which the two differ."""
    p32 = np.asarray(pred, dtype=np.float32).reshape(-1)
    n = p32.size
    d = p32.astype(np.float64) - np.float64(np.float32(label))
    count = int(np.sum(np.abs(p32 - np.float32(label)) <= np.float32(0.5)))
    return float(weight * np.mean(d * d)), count, n, (weight * 2.0 * d / n).reshape(np.shape(pred))


def adversarial_loss(pred_fake):
    """get_adv_loss: 0.5 mse(D(fake), 1) -> (loss, d_pred)"""
    loss, _, _, d = lsgan(pred_fake, 1.0, 0.5)
    return loss, d


def discriminator_loss(pred_real, pred_fake):
    """train_dis: 0.5 (mse(D(real), 1) + mse(D(fake), 0)) -> (loss, real_acc, fake_acc, d_pred_real, d_pred_fake)"""
    lr, cr, nr, dr = lsgan(pred_real, 1.0, 0.5)
    lf, cf, nf, df = lsgan(pred_fake, 0.0, 0.5)
    return lr + lf, cr / nr, cf / nf, dr, df


def pool_exchange(pool, cur, items, swap, slot):
    """Sample_from_Pool.__call__ at given draws, item by item: pool [cap,row] (a copy is updated), cur rows filled.  An item whose
    slot lies outside [0, cap) passes through whatever its `swap` says, as the header has it.
    -> (returned [n,row], pool, cur)"""
    pool, items = np.array(pool, copy=True), np.asarray(items)
    cap = pool.shape[0]
    out = np.empty_like(items)
    for i in range(items.shape[0]):
        if cur < cap:
            pool[cur] = items[i]
            cur += 1
            out[i] = items[i]
        elif swap[i] and 0 <= slot[i] < cap:                                    # (a slot outside [0, cap) is no swap: pg_pool_exchange)
            out[i] = pool[slot[i]]
            pool[slot[i]] = items[i]
        else:
            out[i] = items[i]
    return out, pool, cur


def grad_sample_index(numel, k=8):
    """the k flat entries of a parameter gradient the fixture keeps"""
    return np.unique(np.linspace(0, numel - 1, k).astype(np.int64))
