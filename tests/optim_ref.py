"""The float64 restatement of pg_adam_step (include/posegen_optim.h) in numpy, the bound the device is held to, and
the case tables the host and the GPU tests share.

One call on tensors i with float32 inputs p, g, m, v, group hyperparameters (lr, b1, b2, eps, wd) and step t:
    norm = sqrt(sum g^2) over all tensors;  coef = min(max_norm / (norm + 1e-6), 1), NaN staying NaN; 1 without clipping
    gc = coef g;  g' = gc + wd p  (wd == 0: g' = gc)
    m' = m + (g' - m)(1 - b1);  v' = b2 v + (1 - b2) g'^2
    D = sqrt(v') / sqrt(1 - b2^t) + eps;  T = (lr / (1 - b1^t)) (m' / D);  p' = p - T
all in float64; the device rounds p', m', v' (and gc with write_grads) to float32 once.

The bound, per element:  |device - f64| <= 0.5 ulp32(f64) + k 2^-53 mag.  u = 2^-53 is the largest relative error of one double
operation.  The table constants (1 - b1, 1 - b2, lr / (1 - b1^t), sqrt(1 - b2^t)) are formed by the same double operations of the
same libm on both sides and count as exact, and so does coef: the GPU tests hand the device's own coefficient to the restatement
(after holding it to 1e-14 of the restatement's), because two orders of a sum of N squares may differ by log2(N) u, which is not an
error of the update.  Roundings, in units of u:
    gc: 1 (product).  g': wd p (1), the sum (1) -> 3 on mag_g = |gc| + |wd p|.
    m': g' (3, scaled by 1 - b1 <= 1), g' - m (1), the product (1), the sum (1) -> k_m = 6 on mag_m = |m| + (mag_g + |m|)(1 - b1).
    v': b2 v (1); g'^2 (2 x 3 + 1 = 7), times 1 - b2 (1) = 8; the sum (1) -> k_v = 9 on mag_v = b2 |v| + (1 - b2) mag_g^2.
    p': with a_m = mag_m / |m'| and a_v = mag_v / v' (>= 1: how much cancellation enlarged the relative errors of m', v'):
        sqrt(v') 4.5 a_v + 1, / bc2 1, + eps 1, m' / D 6 a_m + 1, times the step size 1: T carries 6 a_m + 4.5 a_v + 5; p - T 1 on
        |p| + |T|.  With mag_p = |p| + |T| (a_m + a_v), k_p = 9 covers it: 9 (a_m + a_v) >= 6 a_m + 4.5 a_v + 6 for a_m, a_v >= 1.
So k = (9, 6, 9) for (p, m, v) and 1 for the clipped gradient: all below 16.  Derived, not tuned.
"""
import numpy as np

U = 2.0 ** -53
K_P, K_M, K_V, K_G = 9, 6, 9, 1
SEG = 16384
NO_CLIP = None

MUTANTS = ("coef32", "t_minus_1", "eps_in_sqrt", "swap_betas", "wd_scaled")


def total_norm(tensors):
    """(sum of g^2 over every tensor)^(1/2) in float64"""
    return float(np.sqrt(sum(float(np.sum(np.asarray(t["g"], np.float64) ** 2)) for t in tensors)))


def clip_coef(norm, max_norm):
    if max_norm is None:
        return 1.0
    with np.errstate(all="ignore"):
        c = np.float64(max_norm) / (np.float64(norm) + 1e-6)
    return float(c if not c > 1.0 else 1.0)              # (NaN stays NaN, as torch.clamp(max=1))


def adam_step(tensors, groups, max_norm=None, coef=None, mutant=None, alt=False):
    """tensors: [{p, g, m, v: arrays, group: int, step: int}], groups: [{lr, betas, eps, weight_decay}].  `coef`: use this
    coefficient in place of the restatement's own (the device's, see the module docstring).  `mutant`: one of MUTANTS, a planted
    formula error; `alt`: the same formula in another association of its double operations, as a compiler's contraction or
    another reading of it might give (both for the emulation in tests/test_optim_ref.py, never for a reference).
    -> {norm, coef, tensors: [{p, m, v, gc, mag_p, mag_m, mag_v, mag_g}]} in float64."""
    norm = total_norm(tensors)
    own = clip_coef(norm, max_norm)
    c = own if coef is None else float(coef)
    if mutant == "coef32":
        c = float(np.float32(c))
    out = []
    with np.errstate(all="ignore"):
        for t in tensors:
            q = groups[t["group"]]
            b1, b2 = q["betas"]
            if mutant == "swap_betas":
                b1, b2 = b2, b1
            lr, eps, wd, step = float(q["lr"]), float(q["eps"]), float(q["weight_decay"]), int(t["step"])
            e = step - 1 if mutant == "t_minus_1" else step
            step_size = np.float64(lr) / np.float64(1.0 - b1 ** e)
            bc2 = np.sqrt(np.float64(1.0 - b2 ** e))
            p, g, m, v = (np.asarray(t[k], np.float64) for k in "pgmv")
            gc = c * g
            if wd != 0.0:
                gp = c * (g + wd * p) if mutant == "wd_scaled" else gc + wd * p
                mag_g = np.abs(gc) + np.abs(wd * p)
            else:
                gp, mag_g = gc, np.abs(gc)
            if alt:
                m1 = b1 * m + (1.0 - b1) * gp
                v1 = v + (gp * gp - v) * (1.0 - b2)
            else:
                m1 = m + (gp - m) * (1.0 - b1)
                v1 = b2 * v + (1.0 - b2) * (gp * gp)
            D = np.sqrt(v1 + eps) / bc2 if mutant == "eps_in_sqrt" else np.sqrt(v1) / bc2 + eps
            T = (step_size * m1) / D if alt else step_size * (m1 / D)
            p1 = p - T
            mag_m = np.abs(m) + (mag_g + np.abs(m)) * (1.0 - b1)
            mag_v = b2 * np.abs(v) + (1.0 - b2) * mag_g * mag_g
            a_v = np.where(v1 > 0, mag_v / np.where(v1 > 0, v1, 1.0), 1.0)
            mag_p = np.abs(p) + np.abs(step_size / D) * mag_m + np.abs(T) * a_v
            out.append({"p": p1, "m": m1, "v": v1, "gc": gc, "mag_p": mag_p, "mag_m": mag_m, "mag_v": mag_v, "mag_g": np.abs(gc)})
    return {"norm": norm, "coef": own, "tensors": out}


def excess(dev32, ref64, mag, k):
    """How far each element of the float32 `dev32` is outside the bound around `ref64`, as a share of the bound (<= 1: inside).
    Where the float64 value is not finite, or rounds to a float32 infinity, the device must give exactly its float32."""
    dev32 = np.asarray(dev32, np.float32)
    ref64, mag = np.asarray(ref64, np.float64), np.asarray(mag, np.float64)
    with np.errstate(all="ignore"):
        r32 = ref64.astype(np.float32)
        exact = ~np.isfinite(r32) | ~np.isfinite(mag)
        same = (np.isnan(r32) & np.isnan(dev32)) | (r32 == dev32)
        ulp = np.spacing(np.abs(np.where(exact, 1.0, r32)).astype(np.float32)).astype(np.float64)
        bound = 0.5 * ulp + k * U * np.where(exact, 0.0, mag)
        share = np.abs(dev32.astype(np.float64) - ref64) / bound
        return np.where(exact, np.where(same, 0.0, np.inf), np.where(np.isfinite(dev32), share, np.inf))


def judge(dev, ref, write_grads=False):
    """dev: [{p, m, v[, g]} float32 arrays] of the device (or an emulation), ref: adam_step(...)["tensors"] ->
    (the largest share of the bound, the share of elements bitwise equal to float32(f64), [(tensor, name, index, share)] outside)"""
    worst, n, n_eq, bad = 0.0, 0, 0, []
    for i, (d, r) in enumerate(zip(dev, ref)):
        names = (("p", "p", "mag_p", K_P), ("m", "m", "mag_m", K_M), ("v", "v", "mag_v", K_V)) + ((("g", "gc", "mag_g", K_G),) if write_grads else ())
        for dk, rk, mk, k in names:
            x = np.asarray(d[dk], np.float32).reshape(-1)
            if x.size == 0:
                continue
            s = excess(x, r[rk].reshape(-1), r[mk].reshape(-1), k)
            worst = max(worst, float(s.max()))
            with np.errstate(all="ignore"):
                r32 = r[rk].reshape(-1).astype(np.float32)
            n += x.size
            n_eq += int(np.sum(x.view(np.uint32) == r32.view(np.uint32)))
            for j in np.nonzero(~(s <= 1.0))[0][:3]:
                bad.append((i, dk, int(j), float(s[j])))
    return worst, (n_eq / n if n else 1.0), bad


def emulate(tensors, groups, max_norm=None, mutant=None):
    """what the device does: the formula in double from float32 inputs (in another association than the restatement's), one
    rounding per output"""
    r = adam_step(tensors, groups, max_norm, mutant=mutant, alt=True)
    with np.errstate(all="ignore"):
        return [{"p": t["p"].astype(np.float32), "m": t["m"].astype(np.float32), "v": t["v"].astype(np.float32), "g": t["gc"].astype(np.float32)}
                for t in r["tensors"]]


# ---- cases ------------------------------------------------------------------------------------------------------------------------------
GROUPS = [{"lr": 1e-3, "betas": (0.9, 0.999), "eps": 1e-8, "weight_decay": 0.0},
          {"lr": 3e-2, "betas": (0.5, 0.9), "eps": 1e-5, "weight_decay": 1e-2}]
COUNTS = (0, 1, 3, 4, 5, 63, 64, 65, 255, 1023, 1025, SEG - 1, SEG, SEG + 1, 2 * SEG + 7)
TENSOR_COUNTS = (1, 2, 255, 256, 257, 4096)
STEPS = (1, 2, 1000, 10 ** 6)


def make_tensor(rng, count, group=0, step=3, groups=GROUPS, p_scale=1.0):
    """float32 p, g and the m, v a previous float64 step from zero state leaves (non-trivial, v >= 0)"""
    p = (rng.standard_normal(count) * p_scale).astype(np.float32)
    g0 = rng.standard_normal(count) * 0.3
    b1, b2 = groups[group]["betas"]
    m = ((1.0 - b1) * g0).astype(np.float32)
    v = ((1.0 - b2) * g0 * g0).astype(np.float32)
    g = (rng.standard_normal(count) * 0.3).astype(np.float32)
    return {"p": p, "g": g, "m": m, "v": v, "group": group, "step": step}


def table_cases():
    """name -> (tensors, groups, max_norm): the cases of the GPU table that do not depend on memory layout"""
    cases = {}
    rng = np.random.RandomState(5)
    cases["counts"] = ([make_tensor(rng, c, group=i % 2) for i, c in enumerate(COUNTS)], GROUPS, 1.0)
    cases["counts_noclip"] = ([make_tensor(rng, c, group=i % 2) for i, c in enumerate(COUNTS)], GROUPS, None)
    for n in TENSOR_COUNTS:
        cases[f"tensors_{n}"] = ([make_tensor(rng, 1 + (i * 7) % 9, group=i % 2, step=1 + i % 5) for i in range(n)], GROUPS, 0.5)
    cases["steps"] = ([make_tensor(rng, 130, group=i % 2, step=s) for i, s in enumerate(STEPS + STEPS)], GROUPS, None)
    cases["below"] = ([make_tensor(rng, 300, group=i % 2) for i in range(3)], GROUPS, 1e4)
    cases["above"] = ([make_tensor(rng, 300, group=i % 2) for i in range(3)], GROUPS, 0.01)
    cases["zero_norm"] = ([make_tensor(rng, 300, group=i % 2) for i in range(3)], GROUPS, 0.0)
    cases["tiny_p"] = ([make_tensor(rng, 4000, group=0, p_scale=1e-6), make_tensor(rng, 100, group=0)], GROUPS, 0.37)
    return cases
