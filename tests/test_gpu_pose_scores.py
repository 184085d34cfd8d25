"""pg_pose_scores on the GPU, through the C ABI and through posegen_amd.pose_eval, against the float64 restatement
(tests/pose_scores_ref.py).

Bounds.  per_pose and the summary's means: 1e-10 max(1, |value|) on conditioned poses (s3 / s1 >= 1e-2 of the normalised
cross-covariance; where the rotation mode flips, (s2 - s3) / s1 >= 1e-2 too) -- a double Jacobi backward error of a few 1e-16 times
the polar factor's sensitivity <= 2 / (s2 + s3) <= 2e2, with a margin of 100.  Z: one float32 ulp of the restatement's rounded Z
(assert_f32_neighbours: plus the doubles' own 1e-10 where a coordinate cancels to less than that).
Threshold shares: equal, with no restatement distance within 1e-9 of a threshold.  Degenerate poses (two joints, three joints:
rank <= 2) are compared in raw and d only, and d is reproduced from the Z the kernel wrote.  The reference's own float32 values
(tests/golden/pose_scores.npz) within the bounds of tests/test_pose_scores_ref.py."""
import ctypes as C
import os
import types

import numpy as np
import pytest
import torch

from posegen_amd import _ffi, pose_eval as pe
from tests import pose_scores_ref as ref
from tests.frame_metrics_gpu import DEV, renderer  # noqa: F401 (renderer: a fixture)
from tests.test_pose_scores_ref import BOUND, MIN_RATIO, TAGS, golden_differences

pytestmark = pytest.mark.gpu
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EINVAL = -1
MODES = [ref.ALIGN_NONE, ref.ALIGN_SCALE, ref.ALIGN_BEST, ref.ALIGN_ROTATION]
MODE_NAMES = {v: k for k, v in ref.MODES.items()}
THRESHOLDS = [0.0, 1e-3, 0.02, 0.05, 0.1, 0.3, 1.0, 3.0, 1e6]
F32_EPS = float(np.finfo(np.float32).eps)
SENTINEL = -7.0


def abi(r, pred, gt, joints=None, root=-1, align=ref.ALIGN_BEST, thresholds=(), J=None, B=None, J_in=None, T=None, null=(), out=None):
    """pg_pose_scores through the C ABI on device tensors -> (return code, dict of numpy outputs).  Every output starts filled with
    SENTINEL and has one guard element behind it; `null`: names passed as NULL."""
    Bv, Jin = pred.shape[:2]
    Jv = (len(joints) if joints is not None else Jin) if J is None else J
    Tn = len(thresholds) if T is None else T
    Jout = max(min(Jv, 64), 1)
    if out is None:
        new = lambda n, dt: torch.full((n + 1,), SENTINEL, dtype=dt, device=DEV)
        out = {"per_pose": new(Bv * 4, torch.float64), "aligned": new(Bv * Jout * 3, torch.float32), "joint_err": new(Bv * Jout, torch.float32),
               "summary": new(4 + 2 * max(min(Tn, 64), 0), torch.float64)}
    ptr = lambda name, t: None if name in null else C.c_void_p(t.data_ptr())
    jarr = None if joints is None else (C.c_int32 * len(joints))(*joints)
    tarr = (C.c_double * max(len(thresholds), 1))(*thresholds)
    rc = r.lib.pg_pose_scores(r.handle, r._stream(), Bv if B is None else B, Jin if J_in is None else J_in, ptr("pred", pred), ptr("gt", gt),
                              jarr, Jv, root, align, tarr, Tn, ptr("per_pose", out["per_pose"]), ptr("aligned", out["aligned"]),
                              ptr("joint_err", out["joint_err"]), ptr("summary", out["summary"]))
    torch.cuda.synchronize()
    host = {k: v.cpu().numpy() for k, v in out.items()}
    for k, v in host.items():
        assert v[-1] == SENTINEL, f"{k}: the element behind the output was written"
    if rc == 0:
        host = {"per_pose": host["per_pose"][:-1].reshape(Bv, 4), "aligned": host["aligned"][:-1].reshape(Bv, Jout, 3),
                "joint_err": host["joint_err"][:-1].reshape(Bv, Jout), "summary": host["summary"][:-1]}
    return rc, host


def body_poses(n, joints, seed, noise=0.03, sel=None, root=None, mirror=False):
    """n body-like poses of this project's kinematics: gt [n,J,3] and its prediction -- gt plus joint noise under a random similarity
    transform (mirror: and a reflection) -- in float32.  As in the fixture's generator, a pose whose normalised cross-covariance (of
    the joints `sel` after centring on `root`) misses s3 / s1 >= 1e-2 (mirror: or (s2 - s3) / s1 >= 1e-2) is drawn again."""
    from posegen_amd import synthetic as syn
    rng = np.random.RandomState(seed)
    pool = syn.make_pose(8 * n + 32, seed=seed, sigma=0.35)[1].astype(np.float64)
    if joints <= 24:
        pool = pool[:, :joints]
    else:                                                             # more joints than the skeleton has: a cloud around it
        pool = np.concatenate([pool, pool[:, rng.randint(0, 24, joints - 24)] + rng.normal(0, 0.1, (len(pool), joints - 24, 3))], 1)
    preds, gts = [], []
    for kp in pool:
        q, _ = np.linalg.qr(rng.normal(size=(3, 3)))
        q *= np.sign(np.linalg.det(q))
        if mirror:
            q = q @ np.diag([-1.0, 1.0, 1.0])
        pred = (rng.uniform(0.7, 1.4) * (kp + rng.normal(0, noise, kp.shape)) @ q.T + rng.uniform(-1, 1, 3)).astype(np.float32)
        gt = kp.astype(np.float32)
        r3, gap = ref.conditioning(pred[None], gt[None], sel, root)
        if joints > 3 and (r3[0] < 1.2 * MIN_RATIO or (mirror and gap[0] < 1.2 * MIN_RATIO)):
            continue
        preds.append(pred)
        gts.append(gt)
        if len(preds) == n:
            return np.stack(preds), np.stack(gts)
    raise AssertionError(f"body_poses: {len(preds)} of {n} conditioned poses in a pool of {len(pool)}")


def make_cases():
    cases = {}
    for B, J in ((1, 14), (4, 14), (5, 17), (37, 24), (3, 33), (2, 64), (6, 2)):
        pred, gt = body_poses(B, J, 100 + B + J)
        cases[f"{B}x{J}"] = dict(pred=pred, gt=gt)
    rng = np.random.RandomState(5)
    planar_gt = rng.normal(size=(6, 3, 3)).astype(np.float32)
    cases["6x3 planar"] = dict(pred=(1.3 * planar_gt[:, ::-1] + rng.normal(0, 0.05, (6, 3, 3))).astype(np.float32), gt=planar_gt)
    pred, gt = body_poses(5, 24, 7, sel=ref.GAN_JOINTS, root=0)
    cases["a subset with a root"] = dict(pred=pred, gt=gt, joints=ref.GAN_JOINTS, root=0)
    other = [23, 3, 9, 0, 14, 6, 6, 17, 20]
    pred, gt = body_poses(5, 24, 6, sel=other, root=11)
    cases["a subset in another order, root outside it"] = dict(pred=pred, gt=gt, joints=other, root=11)
    pred, gt = body_poses(4, 14, 8)
    pred, gt = pred + np.float32(1000.0), gt + np.float32(1000.0)
    assert ref.conditioning(pred, gt)[0].min() >= MIN_RATIO            # (still, after the rounding at 1e3)
    cases["offset by 1e3"] = dict(pred=pred, gt=gt)
    pred, gt = body_poses(4, 17, 9, noise=0.0)
    cases["an exact similarity copy"] = dict(pred=pred, gt=gt)
    pred, gt = body_poses(4, 17, 10, noise=0.0, mirror=True)
    cases["a mirrored copy"] = dict(pred=pred, gt=gt)
    return cases


CASES = make_cases()
DEGENERATE = ("6x2", "6x3 planar")


@pytest.fixture(scope="module")
def on_device():
    return {name: (torch.from_numpy(c["pred"]).to(DEV), torch.from_numpy(c["gt"]).to(DEV)) for name, c in CASES.items()}


_restated = {}


def restated(name, mode):
    """the restatement of case `name` in `mode`, computed once: (per-pose dict, summary, conditioned [B])"""
    if (name, mode) not in _restated:
        c = CASES[name]
        pp = ref.per_pose(c["pred"], c["gt"], c.get("joints"), c.get("root"), mode)
        r3, gap = ref.conditioning(c["pred"], c["gt"], c.get("joints"), c.get("root"))
        ok = np.ones(len(r3), bool)
        if mode in (ref.ALIGN_BEST, ref.ALIGN_ROTATION):
            ok = r3 >= MIN_RATIO
        if mode == ref.ALIGN_ROTATION:
            T = ref.polar(ref.cross_covariance(*ref.select(c["pred"], c["gt"], c.get("joints"), c.get("root")))[0], False)[0]
            with np.errstate(invalid="ignore"):
                ok &= (np.linalg.det(np.nan_to_num(T)) > 0) | (gap >= MIN_RATIO)
        _restated[(name, mode)] = (pp, ref.summary(pp, THRESHOLDS), ok)
    return _restated[(name, mode)]


def close(got, want, what):
    got, want = np.asarray(got, dtype=np.float64), np.asarray(want, dtype=np.float64)
    assert np.array_equal(np.isnan(got), np.isnan(want)), (what, got, want)
    with np.errstate(invalid="ignore"):
        err = np.abs(got - want) / np.maximum(1.0, np.abs(want))
    err = np.where(np.isnan(want) | (got == want), 0.0, err)                # (inf == inf)
    assert err.max(initial=0.0) <= 1e-10, (what, float(err.max()), got, want)


def assert_f32_neighbours(got32, want64, what):
    """`got32` is the float32 rounding of a double within 1e-10 max(1, |value|) of `want64` (the bound of the doubles above): it is
    within one float32 ulp of the rounded `want64`, plus that 1e-10 -- which only matters where the ulp is smaller than it: a
    coordinate that cancels to 1e-10 (a pelvis at the origin) has an ulp of 1e-17, below the rounding error of the double sums of
    numbers near 1 that form it on either side."""
    want32 = np.asarray(want64).astype(np.float32)
    err = np.abs(got32.astype(np.float64) - want32.astype(np.float64))
    tol = np.spacing(np.abs(want32)).astype(np.float64) + 1e-10 * np.maximum(1.0, np.abs(want64))
    assert np.all(err <= tol), (what, float((err - tol).max()))
    assert np.mean(err <= np.spacing(np.abs(want32))) > 0.95, what               # (and nearly all of them within the ulp alone)


def thresholds_are_clear_of(dist):
    th = np.asarray(THRESHOLDS[1:])                                          # (nothing is below 0, whatever its distance from it)
    d = dist[np.isfinite(dist)]
    return np.abs(d[:, None] - th[None]).min() > 1e-9


@pytest.mark.parametrize("mode", MODES, ids=[MODE_NAMES[m] for m in MODES])
@pytest.mark.parametrize("name", list(CASES))
def test_every_output_against_the_restatement(renderer, on_device, name, mode):
    c = CASES[name]
    pred, gt = on_device[name]
    pp, want_summary, ok = restated(name, mode)
    rc, got = abi(renderer, pred, gt, c.get("joints"), c.get("root", -1), mode, THRESHOLDS)
    assert rc == 0
    B, J = pp["dist_raw"].shape
    T = len(THRESHOLDS)
    print(name, MODE_NAMES[mode], "per_pose[0]", got["per_pose"][0], "want", [pp[k][0] for k in ("raw", "aligned", "d", "scale")], "conditioned", int(ok.sum()), "of", B)
    degenerate = name in DEGENERATE and mode in (ref.ALIGN_BEST, ref.ALIGN_ROTATION)
    assert degenerate or ok.all(), "a case that is meant to be conditioned is not"
    close(got["per_pose"][:, 0], pp["raw"], "raw")
    close(got["per_pose"][:, 2], pp["d"], "d")
    assert got["summary"][0] == B
    close(got["summary"][1], want_summary[1], "mean raw")
    close(got["summary"][3], want_summary[3], "mean d")
    assert thresholds_are_clear_of(pp["dist_raw"])
    assert np.array_equal(got["summary"][4:4 + T], want_summary[4:4 + T]), "raw shares"
    g = ref.select(c["pred"], c["gt"], c.get("joints"), c.get("root"))[1]
    if degenerate:
        # d from the Z that was written: Z is float32, |dZ_j| <= sqrt(3) eps/2 max|Z| = e moves sum |Z - g|^2 by <= 2 sqrt(sum) sqrt(J) e + J e^2
        Z = got["aligned"].astype(np.float64)
        ssx = ((g - g.mean(1, keepdims=True)) ** 2).sum((1, 2))
        e = np.sqrt(3.0) * 0.5 * F32_EPS * np.abs(Z).max((1, 2))
        d = got["per_pose"][:, 2]
        bound = (2 * np.sqrt(d * ssx) * np.sqrt(J) * e + J * e * e) / ssx + 1e-12
        again = ((Z - g) ** 2).sum((1, 2)) / ssx
        print("d from Z", again, "d", d, "bound", bound)
        assert np.all(np.abs(again - d) <= bound)
        return
    close(got["per_pose"][:, 1], pp["aligned"], "aligned")
    close(got["per_pose"][:, 3], pp["scale"], "scale")
    close(got["summary"][2], want_summary[2], "mean aligned")
    assert_f32_neighbours(got["aligned"], pp["Z"], "Z")
    assert_f32_neighbours(got["joint_err"], pp["dist_aligned"], "joint_err")
    assert thresholds_are_clear_of(pp["dist_aligned"])
    assert np.array_equal(got["summary"][4 + T:], want_summary[4 + T:]), "aligned shares"
    if name == "an exact similarity copy" and mode in (ref.ALIGN_BEST, ref.ALIGN_ROTATION):
        assert got["per_pose"][:, 1].max() < 1e-6 and got["per_pose"][:, 2].max() < 1e-10        # (the copy is exact up to float32 rounding)
    if name == "a mirrored copy":
        if mode == ref.ALIGN_BEST:
            assert got["per_pose"][:, 2].max() < 1e-10
        if mode == ref.ALIGN_ROTATION:
            assert got["per_pose"][:, 2].min() > 0.01


@pytest.mark.parametrize("mode", ["none", "scale", "best", "rotation"])
def test_pose_scorer_returns_the_restatements_numbers_in_the_asked_unit(renderer, on_device, mode):
    name = "a subset with a root"
    c = CASES[name]
    sc = pe.PoseScorer(renderer)
    unit, pck, auc = 1000.0, 150.0, np.linspace(0, 150, 31)
    pp = ref.per_pose(c["pred"], c["gt"], c["joints"], c["root"], ref.MODES[mode])
    want = ref.summary(pp, np.concatenate([[pck], auc]) / unit)
    both, th = np.concatenate([pp["dist_raw"].ravel(), pp["dist_aligned"].ravel()]), (np.concatenate([[pck], auc]) / unit)
    assert np.abs(both[:, None] - th[None][:, th > 0]).min() > 1e-9
    for inputs in (on_device[name], (c["pred"], c["gt"])):                # device tensors, and host arrays that are copied over
        got = sc.score(*inputs, joints=c["joints"], root=c["root"], align=mode, unit=unit, pck_threshold=pck, auc_thresholds=auc,
                       ret_aligned=True, ret_joint_err=True, ret_per_pose=True)
        print(mode, {k: v for k, v in got.items() if not torch.is_tensor(v)})
        assert got["n"] == 5 and all(isinstance(got[k], float) for k in ("mpjpe", "aligned", "d", "pck", "auc", "pck_raw", "auc_raw"))
        close(got["mpjpe"] / unit, want[1], "mpjpe")
        close(got["aligned"] / unit, want[2], "aligned")
        close(got["d"], want[3], "d")
        assert got["pck_raw"] == want[4] and got["pck"] == want[4 + 32]
        close(got["auc_raw"], want[5:4 + 32].mean(), "auc_raw")
        close(got["auc"], want[4 + 33:].mean(), "auc")
        assert got["aligned_kps"].device.type == "cuda" and tuple(got["aligned_kps"].shape) == (5, 14, 3)
        assert tuple(got["joint_err"].shape) == (5, 14) and tuple(got["per_pose"].shape) == (5, 4)
        close(got["per_pose"].cpu().numpy()[:, 1], pp["aligned"], "per_pose aligned")
    none = sc.score(*on_device[name], pck_threshold=None, auc_thresholds=None)
    assert none["pck"] is None and none["auc"] is None and none["pck_raw"] is None and none["auc_raw"] is None


@pytest.mark.parametrize("T", [0, 1, 64])
def test_threshold_counts_with_no_one_and_64_thresholds(renderer, on_device, T):
    name = "37x24"
    pp = restated(name, ref.ALIGN_BEST)[0]
    th = list(np.linspace(0.011, 2.9, T)) if T > 1 else [0.0437][:T]
    both = np.concatenate([pp["dist_raw"].ravel(), pp["dist_aligned"].ravel()])
    assert T == 0 or np.abs(both[:, None] - np.asarray(th)[None]).min() > 1e-9
    rc, got = abi(renderer, *on_device[name], align=ref.ALIGN_BEST, thresholds=th)
    assert rc == 0 and got["summary"].shape == (4 + 2 * T,)
    want = ref.summary(pp, th)
    assert np.array_equal(got["summary"][4:], want[4:])
    close(got["summary"][1:4], want[1:4], "means")
    if T == 64:
        assert 0 < want[4 + 5] < 1 and 0 < want[4 + T] < 1 and want[4 + 2 * T - 1] == 1.0        # (the thresholds do separate the distances)


def test_nan_and_zero_spread_poses_stay_alone(renderer):
    pred, gt = body_poses(9, 14, 21)
    clean = abi(renderer, torch.from_numpy(pred).to(DEV), torch.from_numpy(gt).to(DEV), align=ref.ALIGN_BEST, thresholds=[0.05, 1.0])[1]
    bad_pred, bad_gt = pred.copy(), gt.copy()
    bad_pred[2, 5, 1] = np.nan
    bad_gt[5, 0, 0] = np.inf
    bad_pred[7] = bad_pred[7, 3]                                     # no spread: every joint the same point
    bad_gt[8] = 0.0                                                  # no spread in the target
    bad = [2, 5, 7, 8]
    good = [0, 1, 3, 4, 6]
    for mode in (ref.ALIGN_BEST, ref.ALIGN_ROTATION):
        rc, got = abi(renderer, torch.from_numpy(bad_pred).to(DEV), torch.from_numpy(bad_gt).to(DEV), align=mode, thresholds=[0.05, 1.0])
        assert rc == 0                                               # (and the call has returned)
        pp = ref.per_pose(bad_pred, bad_gt, align=mode)
        want = ref.summary(pp, [0.05, 1.0])
        print("per_pose", got["per_pose"], "summary", got["summary"], "want", want)
        assert np.isnan(got["per_pose"][[2, 5]]).all() and np.isnan(got["aligned"][[2, 5]]).all() and np.isnan(got["joint_err"][[2, 5]]).all()
        assert np.isfinite(got["per_pose"][[7, 8], 0]).all() and np.isnan(got["per_pose"][[7, 8], 1:]).all()
        close(got["per_pose"][:, 0], pp["raw"], "raw")
        assert np.array_equal(np.isnan(got["summary"]), np.isnan(want)) and np.isnan(got["summary"][1:4]).all()
        assert np.array_equal(got["summary"][4:], want[4:])                           # a NaN distance is below nothing
        if mode == ref.ALIGN_BEST:
            for k in ("per_pose", "aligned", "joint_err"):
                assert got[k][good].tobytes() == clean[k][good].tobytes(), k
    for mode in (ref.ALIGN_NONE, ref.ALIGN_SCALE):
        rc, got = abi(renderer, torch.from_numpy(bad_pred).to(DEV), torch.from_numpy(bad_gt).to(DEV), align=mode)
        pp = ref.per_pose(bad_pred, bad_gt, align=mode)
        assert rc == 0 and np.isnan(got["per_pose"][[2, 5]]).all()
        for col, k in enumerate(("raw", "aligned", "d", "scale")):
            close(got["per_pose"][:, col], pp[k], k)


def test_two_calls_give_the_same_bytes_and_a_pose_does_not_see_its_batch(renderer, on_device):
    name = "37x24"
    pred, gt = on_device[name]
    for mode in MODES:
        a = abi(renderer, pred, gt, align=mode, thresholds=THRESHOLDS)[1]
        b = abi(renderer, pred, gt, align=mode, thresholds=THRESHOLDS)[1]
        for k in a:
            assert a[k].tobytes() == b[k].tobytes(), (mode, k)
        for i in (0, 3, 4, 17, 36):
            one = abi(renderer, pred[i:i + 1].contiguous(), gt[i:i + 1].contiguous(), align=mode, thresholds=THRESHOLDS)[1]
            for k in ("per_pose", "aligned", "joint_err"):
                assert one[k][0].tobytes() == a[k][i].tobytes(), (mode, k, i)


def test_golden_fixture_through_the_kernel(renderer):
    g = dict(np.load(os.path.join(REPO, "tests", "golden", "pose_scores.npz")))
    worst = {k: 0.0 for k in BOUND}
    for tag in TAGS:
        pred, gt = torch.from_numpy(g[f"pred_{tag}"]).to(DEV), torch.from_numpy(g[f"gt_{tag}"]).to(DEV)

        def scores(mode):
            rc, got = abi(renderer, pred, gt, align=mode)
            assert rc == 0
            return dict(raw=got["per_pose"][:, 0], aligned=got["per_pose"][:, 1], d=got["per_pose"][:, 2], scale=got["per_pose"][:, 3],
                        Z=got["aligned"].astype(np.float64), dist_aligned=got["joint_err"].astype(np.float64))
        for k, v in golden_differences(g, tag, scores).items():
            worst[k] = max(worst[k], float(np.max(v)))
    print({k: f"{v:.3e}" for k, v in worst.items()})
    for k, v in worst.items():
        assert v <= BOUND[k], (k, v, BOUND[k])


# ---- the wrappers ---------------------------------------------------------------------------------------------------------------------------
def f32_mean_bound(n):
    """relative error of a float32 mean of n float32-rounded non-negative numbers, worst case: (n + 1) eps"""
    return (n + 1) * F32_EPS


def test_wrappers_with_the_references_call_shapes(renderer):
    from posegen_amd import ganloop
    sc = pe.PoseScorer(renderer)
    pred, gt = body_poses(6, 24, 33)
    dp, dg = torch.from_numpy(pred).to(DEV), torch.from_numpy(gt).to(DEV)
    # the GAN loop's number: a float64 device scalar
    fb = ganloop.regressor_feedback(dp, dg, scorer=sc)
    assert torch.is_tensor(fb) and fb.device.type == "cuda" and fb.dim() == 0 and fb.dtype == torch.float64
    want = 1.0 - ref.per_pose(pred, gt, ref.GAN_JOINTS, 0, ref.ALIGN_NONE)["raw"].mean()
    close(float(fb), want, "regressor_feedback")
    close(float(ganloop.regressor_feedback(dp, dg)), want, "regressor_feedback on the module's own scorer")
    n = pred.shape[0] * pred.shape[1]
    for fn, mode in ((pe.pa_mpjpe, ref.ALIGN_BEST), (pe.n_mpjpe, ref.ALIGN_SCALE)):
        pp = ref.per_pose(pred, gt, align=mode)
        metric, kps = fn(dp, dg, scorer=sc)
        assert metric.device.type == "cuda" and kps.device.type == "cuda" and tuple(kps.shape) == pred.shape
        assert abs(float(metric) - pp["dist_aligned"].mean()) <= f32_mean_bound(n) * pp["dist_aligned"].mean()
        assert abs(float(fn(dp, dg, "sum", scorer=sc)[0]) - pp["dist_aligned"].sum()) <= f32_mean_bound(n) * pp["dist_aligned"].sum()
        per_joint = fn(dp, dg, None, scorer=sc)[0].cpu().numpy()
        assert_f32_neighbours(per_joint, pp["dist_aligned"], "the wrapper's distances")
        assert_f32_neighbours(kps.cpu().numpy(), pp["Z"], "the wrapper's key points")
    pp = ref.per_pose(pred, gt, align=ref.ALIGN_ROTATION)
    close(reconstruction_error_np(pe.reconstruction_error(dp, dg, reduction=None, scorer=sc)), pp["aligned"], "reconstruction_error")
    close(float(pe.reconstruction_error(dp, dg, scorer=sc)), pp["aligned"].mean(), "reconstruction_error mean")
    close(float(pe.reconstruction_error(dp, dg, reduction="sum", scorer=sc)), pp["aligned"].sum(), "reconstruction_error sum")
    alpha = 1.9
    raw32 = pp["dist_raw"].astype(np.float32)
    assert np.abs(raw32 - np.float32(alpha)).min() > 1e-5                      # no distance near alpha: float32 rounding cannot move a count
    re, pck, s1_hat = pe.reconstruction_error(dp, dg, reduction="mean", needpck=True, alpha=alpha, scorer=sc)
    want_pck = (pp["dist_raw"] < alpha).mean(1)
    # (torch forms the mean of a pose's 24 flags as sum x 1/24, numpy as sum / 24: the counts are compared exactly, the shares to rounding)
    assert 0 < want_pck.mean() < 1 and np.array_equal(np.rint(pck.cpu().numpy() * pred.shape[1]), (pp["dist_raw"] < alpha).sum(1))
    close(pck.cpu().numpy(), want_pck, "error_pck")
    assert_f32_neighbours(s1_hat.cpu().numpy(), pp["Z"], "S1_hat")


def reconstruction_error_np(t):
    assert t.device.type == "cuda" and t.dtype == torch.float64
    return t.cpu().numpy()


def test_refinement_scores_of_a_small_pose_layer(renderer):
    from posegen_amd import synthetic as syn
    from posegen_amd.poseopt import HipPoseOptLayer
    from posegen_amd.skeleton import SURREAL_REST_SCALE, smpl_rest_pose
    bones, kps, _ = syn.make_pose(4, seed=12)
    rest = (smpl_rest_pose * SURREAL_REST_SCALE).astype(np.float32)[None]
    layer = HipPoseOptLayer(kps, bones, rest, use_rot6d=True, renderer=renderer)
    with torch.no_grad():                                            # a refinement step's worth of change
        layer.pelvis.add_(0.01)
        layer.bones.add_(0.02 * torch.randn(layer.bones.shape, generator=torch.Generator().manual_seed(1)).to(DEV))
    idx = [2, 0, 3]
    now = layer(np.asarray(idx))[0].detach().cpu().numpy()
    ext = 0.001
    gt = body_poses(4, 24, 44)[1]
    got = pe.refinement_scores(layer, idx, kps, gt_kps=gt, ext_scale=ext)
    print(got)
    close(got["MPJPC"] * ext, ref.per_pose(now, kps[idx], align=ref.ALIGN_NONE)["raw"].mean(), "MPJPC")
    best = ref.per_pose(now, gt[idx], align=ref.ALIGN_BEST)
    close(got["PA-MPJPE"] * ext, best["aligned"].mean(), "PA-MPJPE")
    close(got["MPJPE"] * ext, best["raw"].mean(), "MPJPE")
    close(got["d"], best["d"].mean(), "d")
    assert got["MPJPC"] > 1.0 and set(pe.refinement_scores(layer, idx, torch.from_numpy(kps).to(DEV))) == {"MPJPC"}


REFUSED = {
    "pred NULL": dict(null=("pred",)), "gt NULL": dict(null=("gt",)), "summary NULL": dict(null=("summary",)),
    "B = 0": dict(B=0), "B = -1": dict(B=-1), "J = 0 with joints": dict(joints=[], J=0), "J = 65 with joints": dict(joints=[0] * 65),
    "a joint index = J_in": dict(joints=[0, 1, 14]), "a joint index = -1": dict(joints=[3, -1]), "root = J_in": dict(root=14),
    "root = -2": dict(root=-2), "mode 4": dict(align=4), "mode -1": dict(align=-1), "T = 65": dict(thresholds=[0.1] * 65),
    "T = -1": dict(T=-1), "J_in = 0": dict(J_in=0),
}


@pytest.mark.parametrize("what", list(REFUSED))
def test_refusals_write_nothing(renderer, on_device, what):
    pred, gt = on_device["4x14"]
    rc, got = abi(renderer, pred, gt, **REFUSED[what])
    assert rc == EINVAL, what
    for k, v in got.items():
        assert np.all(v == SENTINEL), (what, k)
    assert b"pg_pose_scores" in renderer.lib.pg_last_error(renderer.handle)


def test_65_joints_without_a_selection_are_refused(renderer):
    x = torch.zeros(2, 65, 3, device=DEV)
    rc, got = abi(renderer, x, x)
    assert rc == EINVAL and all(np.all(v == SENTINEL) for v in got.values())
    rc, got = abi(renderer, x, x, joints=list(range(1, 65)), root=0, align=ref.ALIGN_NONE)       # 64 of the 65 are fine
    assert rc == 0 and np.all(got["per_pose"][:, 0] == 0)
