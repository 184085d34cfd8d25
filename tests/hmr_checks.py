"""The layer-local checks of the HMR regression head, shared by the device tests (tests/test_gpu_hmr.py, tests/test_gpu_hmr_specs.py)
and by the float32 emulation on the CPU (tests/test_hmr_ref.py): what judges `hmr_ref.emulate_forward` / `emulate_backward` is the
code that judges pg_hmr.hip.  A run is anything with `spec`, `B`, `P`, `xf_np`, `init_np`, `masks_np`, `out` (rotmat, shape, cam; None
where not produced), `arrays()` (the tape as float64 arrays) and `backward(*cotangents, want=)`: `Head` of tests/test_gpu_hmr.py on
the device, `Emulated` here.

Every comparison is  |got - f64| <= bound  elementwise, the error never divided by the bound for the verdict; the worst ratios are
printed and kept in WORST for the record.  Inside `collecting()` a failed comparison is recorded in place of raised, so that a test of
a planted error can say which quantities left their bounds and where."""
import contextlib

import numpy as np

from posegen_amd import _ffi
from tests import hmr_ref as ref

U = 2.0 ** -24
TINY = 2.0 ** -149
GRADS = _ffi.HMR_TENSORS
EVERY = GRADS + ("d_xf", "d_init")
WORST = {}
_FAILED = None


@contextlib.contextmanager
def collecting():
    """-> a list that receives (name, context, indices of the offending elements or None) of every check that fails inside"""
    global _FAILED
    before, _FAILED = _FAILED, []
    try:
        yield _FAILED
    finally:
        _FAILED = before


def require(cond, name, ctx=(), where=None):
    if _FAILED is not None:
        if not cond:
            _FAILED.append((name, tuple(ctx), where))
        return
    assert cond, (name,) + tuple(ctx)


def note(name, err, bound):
    """the worst error-to-bound ratio of a check, for the record (printed; the assertion itself compares err with bound)"""
    err, bound = np.broadcast_arrays(np.asarray(err, np.float64), np.asarray(bound, np.float64))
    if not err.size:
        return
    with np.errstate(invalid="ignore", divide="ignore"):
        r = np.where(bound > 0, err / np.where(bound > 0, bound, 1.0), np.where(err > 0, np.inf, 0.0))
    WORST[name] = max(WORST.get(name, 0.0), float(np.max(r)))
    print(f"RATIO {name}: {float(np.max(r)):.3f} (worst so far {WORST[name]:.3f})")


def within(name, dev, want, bound, ctx=()):
    err = np.abs(np.asarray(dev, np.float64) - want)
    note(name, err, bound + TINY)
    ok = err <= bound + TINY                                                 # (a NaN error is not within)
    require(bool(np.all(ok)), name, ctx, None if np.all(ok) else np.argwhere(~np.broadcast_to(ok, err.shape)))


def same(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


def well_conditioned(spec, s_final):
    c1, c2 = ref.rot6d_conditioning(np.asarray(s_final, np.float64)[:, :spec.n_pose].reshape(-1, spec.n_joints, 6))
    return (c1 >= 1e-3) & (c2 >= 1e-3)


def check_forward(run, tag):
    """every layer-local property of one forward run"""
    spec, B, P, out = run.spec, run.B, run.P, run.out
    t = run.arrays()
    ctx = (tag, B)
    require(same(t["s"][0].astype(np.float32), np.broadcast_to(run.init_np, (B, spec.n_state))), f"{tag} s_0 is the init", ctx)
    v, e = ref.p_with_bound(P, run.xf_np, spec)
    within(f"{tag} P", t["P"], v, e, ctx)
    for i in range(spec.n_iter):
        m1, m2 = (None, None) if run.masks_np is None else (run.masks_np[i, 0], run.masks_np[i, 1])
        v, e = ref.h1_with_bound(P, t["P"], t["s"][i], spec, m1)
        within(f"{tag} h1", t["h1"][i], v, e, ctx + (i,))
        v, e = ref.h2_with_bound(P, t["h1"][i], spec, m2)
        within(f"{tag} h2", t["h2"][i], v, e, ctx + (i,))
        v, e = ref.state_with_bound(P, t["s"][i], t["h2"][i])
        within(f"{tag} s", t["s"][i + 1], v, e, ctx + (i,))
        if m1 is not None:                                                     # a dropped element is +0
            for h, m in ((t["h1"][i], m1), (t["h2"][i], m2)):
                require(bool(np.all(h[m == 0] == 0.0) and not np.any(np.signbit(h[m == 0]))), f"{tag} a dropped element is +0", ctx + (i,))
    s_final = t["s"][-1]
    a, b = spec.n_pose, spec.n_pose + spec.n_shape
    for k, cols in (("shape", s_final[:, a:b]), ("cam", s_final[:, b:])):      # (an empty output has no buffer: nothing to compare)
        if cols.shape[1] or out[k] is not None:
            require(out[k] is not None and same(out[k], cols.astype(np.float32)), f"{tag} {k} is the final state's columns", ctx)
    R64 = ref.rot6d(s_final[:, :a].reshape(B, spec.n_joints, 6))
    well = well_conditioned(spec, s_final)
    within(f"{tag} rotmat", out["rotmat"][well], R64[well], U * np.abs(R64[well]) + 2.0 ** -40, ctx)
    return t, well


def check_backward(run, cots, tag, want=EVERY, **bound_kw):
    """the float64 chain from the run's own tape and cotangents against its gradients, under the bounds carried down the chain
    (`bound_kw`: `double_sum` and `row_terms` of hmr_ref.backward_with_bound, for sums longer than the defaults are worded for)"""
    spec, B = run.spec, run.B
    t = run.arrays()
    assert np.all(well_conditioned(spec, t["s"][-1])) or cots[0] is None, "the seed gives an ill-conditioned joint: choose another"
    c64 = [None if c is None else np.asarray(c, np.float64) for c in cots]
    ds = ref.final_cotangent(spec, t["s"][-1], *c64)
    e_final = U * np.abs(ds) + 2.0 ** -40 * np.max(np.abs(ds), axis=1, keepdims=True)
    e_final[:, spec.n_pose:] = 0.0                                            # (the shape and cam cotangents are copied)
    val, bnd = ref.backward_with_bound(run.P, run.xf_np, spec, run.masks_np, t, ds, e_final, **bound_kw)
    got = run.backward(*cots, want=want)
    for k, g in got.items():
        within(f"{tag} {k}", g, val[k], bnd[k], (tag, B))
    return got


class Emulated:
    """`hmr_ref.emulate_forward` / `emulate_backward` behind the interface of a device run; `mutant`: one of hmr_ref.MUTANTS or None"""

    def __init__(self, spec, sd, xf, masks=None, init=None, mutant=None):
        self.spec, self.sd, self.B, self.mutant = spec, sd, int(xf.shape[0]), mutant
        self.P = ref.params_of(sd)
        self.xf_np = np.asarray(xf, np.float32)
        self.init_np = np.asarray(ref.init_of(sd) if init is None else init, np.float32)
        self.masks_np = masks

    def forward(self):
        tape, rotmat, shape, cam = ref.emulate_forward(self.P, self.xf_np, self.init_np, self.spec, self.masks_np, self.mutant)
        self.out = {"tape": tape, "rotmat": rotmat, "shape": shape if self.spec.n_shape else None, "cam": cam if self.spec.n_cam else None}
        return self.out

    def arrays(self):
        t = ref.tape_arrays(self.spec, self.B, self.out["tape"])
        return {k: (v.astype(np.float64) if k == "P" else [a.astype(np.float64) for a in v]) for k, v in t.items()}

    def backward(self, d_rotmat=None, d_shape=None, d_cam=None, want=EVERY):
        g = ref.emulate_backward(self.P, self.xf_np, self.spec, self.masks_np, self.out["tape"], d_rotmat, d_shape, d_cam, self.mutant)
        return {k: g[k] for k in want if g[k].size}
