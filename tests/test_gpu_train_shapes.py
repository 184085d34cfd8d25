"""The training step (`TrainableRayCaster`: pg_train_forward / pg_train_backward) across shapes and options, in both training
precisions, against the oracle under torch autograd in float64 (tests/helpers.py: oracle_grads, pinned to the reference's
gradients by tests/test_oracle_float64.py).  The batches are the train_grads fixture's rays, repeated and jittered; the
draws are make_training_draws(..., pytest=True).  Every case compares the loss, the maps the loss reads and the gradient of
every parameter tensor of both nets (and the frame codes) -- every entry, not a sample of them.

Bounds.  fp32: every entry within 1e-4 of the tensor's scale (max(largest entry, norm / sqrt(size)), as in
test_gpu_train.py), every norm within 1e-4 relative, the loss within 1e-5, the maps within 2e-5.  bf16: the mode's bounds
(norms 1e-2, entries 0.1, loss 2e-3; maps 1e-2).  A tensor or map a case cannot hold to its bound -- an ill-conditioned sum,
where the reference's own fp32 arithmetic lies as far from float64 -- gets max(bound, 4 x the fp32 oracle's deviation from
float64 on it), computed in the test and printed; never a looser constant.  The bf16 entry bound applies, as in
test_gpu_train.py, at the entries the fixtures sample; the largest deviation of any entry is printed.

Shapes: point counts below 64 and at the last row tile of every persistent layer GEMM variant (64-row tiles of the 256-wide
layers, 32-row tiles of layer 0 and of the skip layer), coarse-only, lindisp / ray noise / softplus, per-ray poses and
cylinders, frame codes, rays that miss the cylinder, the longest rows the composite takes, and the step at size: enough rows
that every persistent variant's ring wraps and the weight gradients reduce dozens of split-K slices."""
import math
import os

import numpy as np
import pytest
import torch

from tests.helpers import cfg_from_golden, load_golden, loss_of, model_for, oracle_grads

pytestmark = pytest.mark.gpu
DEV = "cuda:0"

# persistent layer GEMM variants (pg_train.hip: LG256 / LG432 / LGSKIP): rows per tile, ring depth
LG_VARIANTS = {"lgemm256": (64, 4), "lgemm432": (32, 4), "lgemm_skip": (32, 3)}
PART_FLOATS = 20 << 20          # pg_train.hip: the split-K scratch


def _batch(n, seed=0, name="train_grads", first=0):
    """n rays of the fixture, repeated, the repeats' directions jittered (view directions re-derived), targets along.  The
    half-opaque rays come first, then the opaque ones, the empty ones last: about half of the fixture's rays see nothing (acc
    0, no gradient at all), and behind a ray that is opaque (transmittance within fp32 rounding of 0) the gradients hang on
    that rounding -- a small batch of either would compare little or nothing."""
    g = load_golden(name)
    m = g["ray_batch"].shape[0]
    acc = g["acc_map"].astype(np.float64)
    idx = np.lexsort((np.abs(acc - 0.5), acc >= 0.99, acc <= 0.01))[(np.arange(n) + first) % m]
    rb = g["ray_batch"][idx].copy()
    rng = np.random.RandomState(seed)
    rep = np.arange(n) >= m
    d = rb[:, 3:6]
    d[rep] += 0.02 * np.linalg.norm(d[rep], axis=1, keepdims=True) * rng.randn(int(rep.sum()), 3).astype(np.float32)
    rb[:, 8:11] = d / np.linalg.norm(d, axis=1, keepdims=True)
    return g, rb, g["target"][idx].copy()


def _misses(rb, cyl):
    """rays whose line misses the cylinder in the x-z plane (the oracle's NaN of near_far_in_cylinder)"""
    o, d = rb[:, [0, 2]], rb[:, [3, 5]]
    c = np.broadcast_to(cyl[..., :2], o.shape)
    cross = (c - o)[:, 0] * d[:, 1] - (c - o)[:, 1] * d[:, 0]
    return np.abs(cross) / np.linalg.norm(d, axis=1) > np.broadcast_to(cyl[..., 2], o.shape[:1])


def _case(key):
    """inputs of a case: dict(cfg, weights, rays, skts, cyls, cams, target, S, N, draws, lindisp)"""
    from posegen_amd import surreal_config
    from posegen_amd.raycaster import make_training_draws
    opts = dict(CASES[key])
    n, S, N = opts.pop("n"), opts.pop("S"), opts.pop("N")
    fixture = opts.pop("fixture", "train_grads")
    g, rb, target = _batch(n, seed=n * 1000 + S, name=fixture, first=opts.pop("first", 0))
    cfg = cfg_from_golden(g) if fixture != "train_grads" else surreal_config(n_samples=S, n_importance=N)
    cfg.n_samples, cfg.n_importance = S, N
    weights = model_for(cfg, int(g["seed_model"]) if fixture != "train_grads" else 4)
    skts, cyls, cams = g["skts"].copy(), g["cyl"].copy(), None
    rng = np.random.RandomState(7)
    if opts.get("per_ray"):         # a pose and a cylinder of its own for every ray (pose_stride 384, cyl_stride 5)
        skts = np.repeat(skts, n, 0)
        skts[:, :, :3, 3] += 0.01 * rng.randn(n, skts.shape[1], 3).astype(np.float32)
        cyls = np.repeat(cyls, n, 0)
        cyls[:, :2] += 0.005 * rng.randn(n, 2).astype(np.float32)
    # (the fixture's own batch has 2 rays in 48 that miss the cylinder, the jittered repeats a few more: the nanmean patch of
    # near / far is in most cases; "miss" moves every tenth ray sideways by 4 radii on top)
    if opts.get("miss"):
        sel = np.arange(n) % 10 == 3
        d = rb[sel][:, [3, 5]]
        perp = np.stack([-d[:, 1], d[:, 0]], 1) / np.linalg.norm(d, axis=1, keepdims=True)
        rb[np.ix_(sel, [0, 2])] += 4.0 * float(cyls[0, 2]) * perp
        miss = _misses(rb, cyls)
        assert miss[sel].all() and miss.mean() >= 0.1, "the moved rays miss"
    if cfg.framecode_ch:            # code 0, the last code, repeats
        cams = (np.arange(n) * 29 % cfg.n_framecodes).astype(np.float32)
        cams[:3] = [0, cfg.n_framecodes - 1, 0]
        cams[-1] = cfg.n_framecodes - 1
    torch.manual_seed(n + S)
    draws = make_training_draws(n, S, N, perturb=1., raw_noise_std=1., ray_noise_std=opts.get("ray_noise_std", 0.), pytest=True)
    return dict(cfg=cfg, weights=weights, rb=rb, skts=skts, cyls=cyls, cams=cams, target=target, S=S, N=N, draws=draws,
                lindisp=bool(opts.get("lindisp")))


def _composite_max():
    from posegen_amd import _ffi
    lib = _ffi.load_library()
    return int(lib.pg_composite_max_samples()), int(lib.pg_composite_max_importance())


CASES = {
    # P < 64 and P = 64 (the 16-bit mode's persistent kernel and 128-tile kernels want 64 rows)
    # (p32 takes the second ray of the ordering: 32 points of the first one put a views-layer bias entry on a ReLU kink that the
    # bf16 forward flips -- that entry moves by 27 % of the tensor's scale, the fp32 step stays within 4e-6)
    "p32": dict(n=1, S=32, N=0, first=1),
    "p62": dict(n=2, S=31, N=0),
    "p48_64": dict(n=1, S=48, N=16),
    # the last row tile of every persistent variant: 64 k - 1, 64 k, 64 k + 1 and 32 k - 1, 32 k + 1 rows (k odd)
    "p511": dict(n=7, S=73, N=0),
    "p512": dict(n=8, S=64, N=0),
    "p513": dict(n=27, S=19, N=0),
    "p287": dict(n=7, S=41, N=0),
    "p289": dict(n=17, S=17, N=0),
    "coarse_only": dict(n=7, S=40, N=0),
    "lindisp": dict(n=13, S=33, N=7, lindisp=True),
    "ray_noise": dict(n=13, S=33, N=7, ray_noise_std=1.0),
    "softplus": dict(n=13, S=33, N=7, fixture="train_grads_softplus"),   # (every ray opaque: see _batch)
    "per_ray": dict(n=21, S=32, N=8, per_ray=True),
    "framecodes": dict(n=37, S=64, N=16, fixture="train_grads_h36m"),
    "miss": dict(n=40, S=32, N=8, miss=True),
    "max_samples": dict(n=3, S=None, N=None),       # S + N = pg_composite_max_samples(), N = pg_composite_max_importance()
}
_ORACLE = {}


def _oracle(key, c, dtype=torch.float64):
    if (key, dtype) not in _ORACLE:
        wc, wf, tv, td = c["weights"]
        _ORACLE[(key, dtype)] = oracle_grads(c["cfg"], wc, wf, float(tv), float(td), c["rb"], c["skts"], c["cyls"], c["target"], c["S"],
                                             c["N"], cams=c["cams"], draws=c["draws"], lindisp=c["lindisp"], dtype=dtype)
    return _ORACLE[(key, dtype)]


def _hip_step(c, train_precision):
    """one training step on the HIP path: (loss, maps, grads {(tag, name): float64 array}, the trainable caster)"""
    from posegen_amd.raycaster import HipRayCaster
    from posegen_amd.train import TrainableRayCaster
    wc, wf, tv, td = c["weights"]
    caster = HipRayCaster.from_weights(c["cfg"], wc, wf, float(tv), float(td), device=DEV, precision="fp32")
    m = TrainableRayCaster(caster, train_precision=train_precision)
    m.train()
    cams = None if c["cams"] is None else torch.tensor(c["cams"])
    out = m(torch.tensor(c["rb"]), N_samples=c["S"], skts=torch.tensor(c["skts"]), cyls=torch.tensor(c["cyls"]), cams=cams,
            N_importance=c["N"], lindisp=c["lindisp"], draws={k: v.to(DEV) for k, v in c["draws"].items()})
    loss = loss_of(out, torch.tensor(c["target"], device=DEV))
    loss.backward()
    maps = {k: out[k].detach().double().cpu().numpy() for k in ("rgb_map", "acc_map", "rgb0", "acc0") if k in out}
    grads = {}
    for tag, net in (("coarse", m.network), ("fine", m.network_fine)):
        for k, p in net.named_parameters():
            if tag == "fine" and c["N"] == 0:           # no fine pass: the fine net is not on the tape
                assert p.grad is None or not bool(p.grad.any()), k
                continue
            assert p.grad is not None, (tag, k)
            grads[(tag, k)] = p.grad.detach().double().cpu().numpy()
    return float(loss.detach()), maps, grads, m


def _deviations(got, ref, sampled=False):
    """per tensor: (largest entry deviation / scale, norm deviation / norm, scale, norm); sampled: the entries at the positions
    the train_grads fixtures store (grad_sample_index), else every entry"""
    from tools.gen_golden import grad_sample_index
    dev = {}
    for key, r in ref.items():
        a, r = got[key].reshape(-1), r.reshape(-1)
        rn = float(np.linalg.norm(r))
        scale = max(float(np.abs(r).max()), rn / math.sqrt(r.size), 1e-12)
        at = grad_sample_index(r.size) if sampled else slice(None)
        dev[key] = (float(np.abs(a[at] - r[at]).max()) / scale, abs(float(np.linalg.norm(a)) - rn) / max(rn, 1e-12), scale, rn)
    return dev


def _violations(got, ref, tol_entry, tol_norm, sampled=False):
    """tensors outside the bounds (floats, or dicts of per-tensor bounds)"""
    assert set(got) == set(ref), sorted(set(got) ^ set(ref))
    bad = []
    for key, (ve, vn, scale, rn) in _deviations(got, ref, sampled).items():
        te = tol_entry[key] if isinstance(tol_entry, dict) else tol_entry
        tn = tol_norm[key] if isinstance(tol_norm, dict) else tol_norm
        if ve * scale > te * scale + 1e-9 or vn * max(rn, 1e-12) > tn * rn + 1e-9 or not np.isfinite(got[key]).all():
            bad.append((key, ve, vn))
    return bad


# bf16: the training mode's bounds (test_bf16_training_mode_gradients_are_close_and_repeatable: loss 2e-3, norms 1e-2, the
# fixture's sampled entries 0.1) and the 16-bit rendering modes' bound on the maps (test_gpu_parity.py: 4e-2)
BOUNDS = {"fp32": dict(loss=1e-5, maps=2e-5, entry=1e-4, norm=1e-4), "bf16": dict(loss=2e-3, maps=4e-2, entry=0.1, norm=1e-2)}


def _check_step(key, c, tp, hip=None):
    """run the HIP step (or take `hip`), compare with the float64 oracle.  A quantity outside its bound is measured against
    the case's own sensitivity: the bound becomes max(bound, 4 x the fp32 oracle's deviation from float64 on that tensor /
    map), computed here and printed.  Returns (the per-tensor entry bounds, the worst deviation, hip)."""
    ref_loss, ref_maps, ref_grads = _oracle(key, c)
    hip = hip or _hip_step(c, tp)
    loss, maps, grads, m = hip
    b = BOUNDS[tp]
    n_nets = 2 if c["N"] > 0 else 1
    assert len(ref_grads) == n_nets * (25 if c["cfg"].framecode_ch else 24)
    assert all(float(np.abs(r).max()) > 0 for r in ref_grads.values()), "a case with a gradient tensor that is all zeros"
    assert abs(loss - ref_loss) <= b["loss"] * max(1.0, abs(ref_loss)), (loss, ref_loss)
    own = lambda: _oracle(key, c, torch.float32)
    for k, v in ref_maps.items():
        err = float(np.abs(maps[k] - v).max())
        if err > b["maps"]:
            sens = float(np.abs(own()[1][k] - v).max())
            print(f"[{key}] {tp}: {k} off by {err:.2e} > {b['maps']:.0e}; the fp32 oracle's own deviation {sens:.2e}")
            assert err <= max(b["maps"], 4.0 * sens), (k, err, sens)
    sampled = tp == "bf16"
    dev = _deviations(grads, ref_grads, sampled)
    worst = max(max(ve, vn) for ve, vn, _, _ in dev.values())
    if sampled:
        every = max(ve for ve, _, _, _ in _deviations(grads, ref_grads).values())
        print(f"[{key}] bf16: largest deviation of any entry {every:.2e} of its tensor's scale (bounded at the sampled entries)")
    tol_e = {k: b["entry"] for k in ref_grads}
    tol_n = {k: b["norm"] for k in ref_grads}
    bad = _violations(grads, ref_grads, tol_e, tol_n, sampled)
    if bad:
        d32 = _deviations(own()[2], ref_grads, sampled)
        for k, _, _ in bad:
            tol_e[k] = max(b["entry"], 4.0 * d32[k][0])
            tol_n[k] = max(b["norm"], 4.0 * d32[k][1])
            print(f"[{key}] {tp}: {k} deviates {dev[k][0]:.2e} / {dev[k][1]:.2e} (entries / norm); the fp32 oracle's own deviation "
                  f"{d32[k][0]:.2e} / {d32[k][1]:.2e}: bounds {tol_e[k]:.2e} / {tol_n[k]:.2e}")
        bad = _violations(grads, ref_grads, tol_e, tol_n, sampled)
    assert not bad, bad[:6]
    return tol_e, worst, hip


# softplus: fp32 only.  Every ray of the softplus model is opaque, and behind an opaque ray the gradients hang on fp32 rounding
# (the fp32 oracle itself lies up to 20x the tensor's scale from float64 on the trunk's biases): the case checks that the HIP
# step reproduces the reference's fp32 arithmetic there; a bf16 tape against float64 would compare noise with noise.
@pytest.mark.parametrize("key,train_precision", [(k, tp) for k in CASES for tp in ("fp32", "bf16") if not (k == "softplus" and tp == "bf16")])
def test_training_step_gradients_match_the_float64_oracle(key, train_precision):
    """One case of the shape / option matrix (CASES) in one training precision.  The 16-bit cases below 64 points take the
    plain GEMMs (two GEMMs for the skip and view layers, alpha's share of dH7 through an fp32 array) -- the persistent and
    128-tile kernels want 64 rows -- and before that fallback existed were refused ("two-segment GEMM outside the 128-tile
    bf16 kernel", "a rank-1 term outside the persistent layer kernel")."""
    if key == "max_samples":
        smax, nmax = _composite_max()
        CASES[key].update(S=smax - nmax, N=nmax)
    c = _case(key)
    tol, worst, hip = _check_step(key, c, train_precision)
    print(f"[{key}] {train_precision}: {c['rb'].shape[0]} rays x {c['S']} + {c['N']}: worst relative gradient deviation {worst:.2e}")
    hip[3].renderer.close()


def _at_size_rays(n_cu, S, N):
    """the first ray count whose fine pass makes every persistent variant's ring wrap (tiles >= (NBUF + 1) x n_cu), with
    tiles not a multiple of n_cu (the last round partial) and P not a multiple of 64 (the last tile partial)"""
    n = math.ceil(max((nb + 1) * n_cu * rows for rows, nb in LG_VARIANTS.values()) / (S + N))
    while not all(_ring_predicate(n * (S + N), n_cu, rows, nb) for rows, nb in LG_VARIANTS.values()):
        n += 1
    return n


def _ring_predicate(P, n_cu, rows, nbuf):
    tiles = -(-P // rows)
    return tiles >= (nbuf + 1) * n_cu and tiles % n_cu != 0 and P % 64 != 0


def _ksplit(P, out, inp):
    """linear_bwd_w's split-K slice count (pg_train.hip; POSEGEN_DW_WGS unset)"""
    tb = 128 if out >= 64 and inp >= 64 else 64
    tiles = -(-out // tb) * -(-inp // tb)
    k = max(2, max(1, min(512 // tiles, -(-P // 1024))))
    return min(k, PART_FLOATS // (out * inp))


@pytest.mark.parametrize("train_precision", ["fp32", "bf16"])
def test_training_step_at_size_matches_the_float64_oracle(train_precision):
    """The step at size: n rays x (64 + 16), n derived from the device's CU count so that in the fine pass every persistent
    variant has tiles >= (NBUF + 1) x n_cu (each workgroup walks its ring around more than once), tiles not a multiple of
    n_cu (the last round is partial) and P not a multiple of 64 (the last tile is partial, its prefetch clamped); the weight
    gradients reduce ~64-81 split-K slices.  Negative control: the same comparison rejects a copy of the fp32 gradients with
    one dW scaled by 1 + 1e-3 (the bf16 bounds cannot see 1e-3 by design)."""
    from posegen_amd import surreal_config
    from posegen_amd.raycaster import HipRenderer
    S, N = 64, 16
    r = HipRenderer(surreal_config(), DEV)
    n_cu = r.device_info()["n_cu"]
    r.close()
    n = _at_size_rays(n_cu, S, N)
    P = n * (S + N)
    for name, (rows, nb) in LG_VARIANTS.items():
        assert _ring_predicate(P, n_cu, rows, nb), name
        tiles = -(-P // rows)
        print(f"at size {n} x ({S} + {N}), {n_cu} CUs: {name} fine pass {tiles} tiles of {rows} rows, {min(tiles, n_cu)} workgroups, "
              f"{-(-tiles // min(tiles, n_cu))} tiles per workgroup (ring of {nb})")
    ks = {f"{o}x{i}": _ksplit(P, o, i) for o, i in ((256, 432), (256, 256), (128, 256))}
    print(f"at size: split-K slices of the fine pass's weight gradients {ks}")
    assert max(ks.values()) >= 64
    key = f"at_size_{n}"
    CASES[key] = dict(n=n, S=S, N=N)
    c = _case(key)
    tol, worst, hip = _check_step(key, c, train_precision)
    print(f"at size {n} x ({S} + {N}), {train_precision}: worst relative gradient deviation {worst:.2e}")
    if train_precision == "fp32":
        ref_grads = _oracle(key, c)[2]
        wrong = dict(hip[2])
        k = ("fine", "pts_linears.3.weight")
        wrong[k] = wrong[k] * (1 + 1e-3)
        assert tol[k] == 1e-4, tol[k]
        assert _violations(wrong, ref_grads, tol, tol), "the comparison must reject a dW off by 1e-3"
    hip[3].renderer.close()


def test_training_step_at_bench_shape_matches_the_float64_oracle():
    """The timed step's own shape (bench.py train_step_rate: 4096 rays x (64 + 16), P = 327 680 in the fine pass), fp32 and
    bf16, against one float64 oracle run (about 24 GB of host memory, 20 s on 8 threads)."""
    key = "bench"
    CASES[key] = dict(n=4096, S=64, N=16)
    c = _case(key)
    for tp in ("fp32", "bf16"):
        tol, worst, hip = _check_step(key, c, tp)
        print(f"bench shape 4096 x (64 + 16), {tp}: worst relative gradient deviation {worst:.2e}")
        hip[3].renderer.close()
    _ORACLE.pop((key, torch.float64), None)


def test_persistent_layer_kernel_is_bitwise_the_tile_kernel_at_size(tmp_path):
    """test_persistent_layer_kernel_is_bitwise_the_tile_kernel again at the at-size shape (rings that wrap, a partial last
    round, a partial last tile): child processes with POSEGEN_LGEMM=1 / 0 (read once per process).  The heads' gradients
    (alpha, feature, view and rgb layers: 8 tensors per net) are bitwise equal; the trunk's, behind dH7, within 1e-6 of the
    tensor's largest entry -- at this size the rank-1 fusion's single rounding flips some bf16 entries of dH7, and every
    trunk layer below sees it."""
    import subprocess
    import sys
    from posegen_amd import surreal_config
    from posegen_amd.raycaster import HipRenderer
    r = HipRenderer(surreal_config(), DEV)
    n_cu = r.device_info()["n_cu"]
    r.close()
    n = _at_size_rays(n_cu, 64, 16)
    repo = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    grads = {}
    for v in ("1", "0"):
        out = str(tmp_path / f"g{v}.pt")
        run = subprocess.run([sys.executable, os.path.join(repo, "tests", "diag", "odd_batch_grads.py"), out, str(n), "64", "16"],
                             capture_output=True, text=True, timeout=300, env=dict(os.environ, POSEGEN_LGEMM=v), cwd=repo)
        assert run.returncode == 0, run.stderr[-2000:]
        grads[v] = torch.load(out)
    same = differ = 0
    for k, a in grads["1"].items():
        b = grads["0"][k]
        if torch.equal(a, b):
            same += 1
        else:
            differ += 1
            assert float((a - b).abs().max()) <= 1e-6 * float(b.abs().max()), k
            assert "pts_linears" in k, k
    print(f"at size {n} x (64 + 16): persistent vs tile GEMM: {same} gradient tensors bitwise equal, {differ} within 1e-6")
    assert same + differ == 48 and same >= 16
