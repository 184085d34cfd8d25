"""Pose scores without a GPU: the float64 restatement of pg_pose_scores (tests/pose_scores_ref.py) against the reference's five
functions on the float32 poses of tests/golden/pose_scores.npz; pg_pose_align.h compiled stand-alone with g++ against the
restatement on seeded, rank-deficient, zero, NaN and mirrored poses; the same program under the sanitisers; the refusals of
posegen_amd.pose_eval; the header and the binding."""
import os
import re
import shutil
import subprocess
import types

import numpy as np
import pytest
import torch

from posegen_amd import _ffi, pose_eval as pe
from tests import pose_scores_ref as ref

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(REPO, "posegen_amd", "csrc")
PROGRAM = os.path.join(REPO, "tools", "sanitize", "pose_align_asan.cpp")
TAGS = ("j14", "j17", "j24", "mirror")
MIN_RATIO = 1e-2                    # the fixture's condition: s3 / s1 of every pose, (s2 - s3) / s1 of the mirrored ones

# |restatement - reference| / max(the reference's error, 1e-3 m), the worst over the fixture's 104 poses, measured on the CPU.  The
# reference's side is float32 throughout (numpy's float32 LAPACK SVD, torch float32 norms) on poses up to 2.8 m across that lie up
# to 2 m from the origin: an absolute error of a few 1e-8 m per coordinate against the 1e-3 m floor, and for `d` = 1 - trace^2 of
# a value near 1e-3 a cancellation of float32 numbers near 1.  The bound is 4 x the measured value (the last-bit spread of float32
# LAPACK between builds); tests/test_gpu_pose_scores.py holds the kernel to the same bounds.
MEASURED = {
    "mpjpe_dist": 1.26e-7,     # Criterion_MPJPE(reduction=None)
    "mpjpe_mean": 1.26e-7,     # Criterion_MPJPE(reduction="mean")
    "pa_dist": 3.84e-5,        # Criterion3DPose_ProcrustesCorrected: the distances
    "pa_kps": 6.31e-5,         #   procrustes' Z
    "pa_d": 1.39e-4,           #   procrustes' d (relative to max(|d|, 1e-3))
    "pa_scale": 2.10e-7,       #   procrustes' scale
    "n_dist": 2.80e-7,         # Criterion3DPose_leastQuaresScaled: the distances
    "n_kps": 3.97e-7,          #   s_opt * pred
    "cst_kps": 3.65e-5,        # compute_similarity_transform
    "re": 7.49e-7,             # reconstruction_error(reduction=None)
}
BOUND = {k: 4 * v for k, v in MEASURED.items()}


@pytest.fixture(scope="module")
def golden():
    return dict(np.load(os.path.join(REPO, "tests", "golden", "pose_scores.npz")))


def golden_differences(g, tag, scores):
    """{name: |scores' value - the reference's| / max(the reference's error, 1e-3)} for the poses `tag` of the fixture;
    `scores(mode)` = the per-pose dict of tests/pose_scores_ref.per_pose for that alignment mode, from whatever computes it"""
    gt = g[f"gt_{tag}"].astype(np.float64)
    rel = lambda got, want, floor_of=None: np.abs(got - want) / np.maximum(np.abs(want if floor_of is None else floor_of), 1e-3)
    joint_rel = lambda Z, want: np.sqrt(((Z - want) ** 2).sum(-1)) / np.maximum(np.sqrt(((want - gt) ** 2).sum(-1)), 1e-3)
    f64 = lambda k: g[f"{k}_{tag}"].astype(np.float64)
    none, scale, best, rot = (scores(m) for m in (ref.ALIGN_NONE, ref.ALIGN_SCALE, ref.ALIGN_BEST, ref.ALIGN_ROTATION))
    return {"mpjpe_dist": rel(none["dist_aligned"], f64("mpjpe_dist")),
            "mpjpe_mean": rel(none["raw"].mean(), f64("mpjpe_mean")),
            "pa_dist": rel(best["dist_aligned"], f64("pa_dist")), "pa_kps": joint_rel(best["Z"], f64("pa_kps")),
            "pa_d": rel(best["d"], f64("pa_d")), "pa_scale": rel(best["scale"], f64("pa_scale")),
            "n_dist": rel(scale["dist_aligned"], f64("n_dist")), "n_kps": joint_rel(scale["Z"], f64("n_kps")),
            "cst_kps": joint_rel(rot["Z"], f64("cst_kps")), "re": rel(rot["aligned"], f64("re"))}


def test_fixture_holds_its_condition_and_takes_the_reflection_branch(golden):
    assert os.path.getsize(os.path.join(REPO, "tests", "golden", "pose_scores.npz")) < 200 * 1024
    for tag in TAGS:
        pred, gt = golden[f"pred_{tag}"], golden[f"gt_{tag}"]
        assert pred.dtype == gt.dtype == np.float32 and pred.shape == gt.shape == ((8 if tag == "mirror" else 32), int(tag[1:]) if tag != "mirror" else 14, 3)
        r3, gap = ref.conditioning(pred, gt)
        assert r3.min() >= MIN_RATIO, (tag, r3.min())
        if tag == "mirror":
            assert gap.min() >= MIN_RATIO and np.all(golden[f"pa_det_{tag}"] < 0)
        else:
            assert np.all(golden[f"pa_det_{tag}"] > 0)


def test_restatement_against_the_references_five_functions(golden):
    """Measured on the CPU (numpy 2 / OpenBLAS float32 on the reference's side), worst relative difference over all 104 poses:
    Criterion_MPJPE 1.26e-7, Criterion3DPose_ProcrustesCorrected 3.84e-5 (Z 6.31e-5, d 1.39e-4, scale 2.10e-7),
    Criterion3DPose_leastQuaresScaled 2.80e-7 (s_opt pred 3.97e-7), compute_similarity_transform 3.65e-5, reconstruction_error
    7.49e-7.  Each bound is 4 x its measured value (MEASURED / BOUND above)."""
    worst = {k: 0.0 for k in BOUND}
    for tag in TAGS:
        diffs = golden_differences(golden, tag, lambda mode: ref.per_pose(golden[f"pred_{tag}"], golden[f"gt_{tag}"], align=mode))
        for k, v in diffs.items():
            worst[k] = max(worst[k], float(np.max(v)))
    print({k: f"{v:.3e}" for k, v in worst.items()})
    for k, v in worst.items():
        assert v <= BOUND[k], (k, v, BOUND[k])
    # the mirrored poses: the two modes differ there, and only there
    for tag in TAGS:
        b = ref.per_pose(golden[f"pred_{tag}"], golden[f"gt_{tag}"], align=ref.ALIGN_BEST)
        r = ref.per_pose(golden[f"pred_{tag}"], golden[f"gt_{tag}"], align=ref.ALIGN_ROTATION)
        if tag == "mirror":
            assert np.all(r["d"] > b["d"] + 0.01)
        else:
            assert np.allclose(r["Z"], b["Z"], rtol=0, atol=1e-12)


def test_summary_counts_strictly_and_propagates_nan():
    rng = np.random.RandomState(3)
    gt = rng.randint(-8, 9, size=(5, 4, 3)).astype(np.float32)            # (integers: + 0.5 below is exact)
    pred = gt.copy()
    pred[:, :, 0] += np.float32(0.5)                                     # every raw distance is exactly 0.5
    pp = ref.per_pose(pred, gt, align=ref.ALIGN_NONE)
    s = ref.summary(pp, [0.5, 0.5000001, 0.0])
    assert s[0] == 5 and s[1] == 0.5 and list(s[4:7]) == [0.0, 1.0, 0.0] and list(s[7:10]) == [0.0, 1.0, 0.0]
    pred[2, 1, 1] = np.nan
    pp = ref.per_pose(pred, gt, align=ref.ALIGN_BEST)
    s = ref.summary(pp, [10.0])
    assert np.isnan(pp["raw"][2]) and np.isnan(pp["Z"][2]).all() and np.isfinite(pp["raw"][[0, 1, 3, 4]]).all()
    assert np.isnan(s[1:4]).all() and s[4] == 0.8                          # a NaN distance is below nothing
    one = ref.per_pose(pred[:1, :1], gt[:1, :1], align=ref.ALIGN_BEST)     # J = 1: no spread
    assert np.isfinite(one["raw"][0]) and np.isnan([one["aligned"][0], one["d"][0], one["scale"][0]]).all()


# ---- pg_pose_align.h stand-alone -----------------------------------------------------------------------------------------------------
def header_cases():
    """(poses, names): 2000 seeded poses of 2 .. 64 joints, a third of them mirrored, then the edge cases"""
    rng = np.random.RandomState(11)
    poses, names = [], []
    for i in range(2000):
        J = int(rng.randint(4, 65)) if i % 10 else int(rng.randint(2, 4))
        gt = rng.normal(size=(J, 3)) * rng.uniform(0.3, 1.0, 3) + rng.normal(0, 3, 3)
        q, _ = np.linalg.qr(rng.normal(size=(3, 3)))
        if i % 3 == 0:
            q = q @ np.diag([1.0, -1.0, 1.0])
        pred = rng.uniform(0.2, 5) * (gt + rng.normal(0, rng.choice([1e-3, 0.05, 0.5]), gt.shape)) @ q.T + rng.normal(0, 3, 3)
        poses.append((pred.astype(np.float32), gt.astype(np.float32)))
        names.append(f"seeded {i}")
    line = np.outer(np.linspace(-1, 2, 5), [1.0, 2.0, -0.5])
    generic = rng.normal(size=(5, 3))
    plane = rng.normal(size=(10, 3)) * [1.0, 1.0, 0.0]
    cross = np.array([[2, 0, 0], [-2, 0, 0], [0, 1, 0], [0, -1, 0], [0, 0, 1], [0, 0, -1]], dtype=np.float64)
    rot, _ = np.linalg.qr(rng.normal(size=(3, 3)))
    nan = rng.normal(size=(6, 3))
    nan[3, 1] = np.nan
    inf = rng.normal(size=(6, 3))
    inf[0, 0] = np.inf
    for name, pred, gt in (("rank 1: both collinear", 2 * line + 1, line), ("rank 1: the target collinear", generic, line),
                           ("rank 1: the prediction collinear", line, generic), ("rank 1: two joints", generic[:2], generic[2:4]),
                           ("rank 2: three joints", generic[:3], generic[2:5] * 2), ("rank 2: the target planar", rng.normal(size=(10, 3)), plane),
                           ("rank 2: both planar", plane @ rot.T, plane + 1), ("zero: the prediction", np.zeros((6, 3)), cross),
                           ("zero: both one point", np.ones((6, 3)), np.full((6, 3), 2.0)), ("zero: one joint", generic[:1], generic[1:2]),
                           ("nan in the prediction", nan, cross), ("nan in the target", cross, nan), ("inf in the prediction", inf, cross),
                           ("mirrored, s2 = s3 exactly", cross * [-1, 1, 1], cross), ("mirrored, s2 = s3, rotated", (cross * [-1, 1, 1]) @ rot.T, cross),
                           ("s1 = s2 = s3, a rotated cube", (np.array([[x, y, z] for x in (-1, 1) for y in (-1, 1) for z in (-1, 1)]) @ rot.T), np.array([[x, y, z] for x in (-1, 1) for y in (-1, 1) for z in (-1, 1)]))):
        poses.append((np.asarray(pred, dtype=np.float32), np.asarray(gt, dtype=np.float32)))
        names.append(name)
    return poses, names


def program_input(poses):
    fmt = lambda a: " ".join(repr(float(v)) for v in np.asarray(a, dtype=np.float64).reshape(-1))
    return f"{len(poses)}\n" + "".join(f"{len(p)}\n{fmt(p)}\n{fmt(g)}\n" for p, g in poses)


def run_program(exe, poses, timeout=120):
    run = subprocess.run([exe], input=program_input(poses), capture_output=True, text=True, timeout=timeout)
    assert run.returncode == 0, (run.stdout[-1500:], run.stderr[-3000:])
    lines = run.stdout.strip().split("\n")
    assert lines[-1] == f"{len(poses)} poses done" and len(lines) == 2 * len(poses) + 1
    return np.array([[float(w) for w in ln.split()] for ln in lines[:-1]]).reshape(len(poses), 2, 17)


def test_pose_align_header_with_plain_gxx_against_the_restatement(tmp_path):
    """T and the sum of singular values within 1e-10 wherever the fixture's conditions hold (s3 / s1 >= 1e-2; where the rotation
    mode flips, (s2 - s3) / s1 >= 1e-2 as well); d within 1e-10 max(1, d) for every pose, NaN where the restatement's is; and the
    program returns on every pose -- the sweep count is fixed."""
    gxx = shutil.which("g++")
    if gxx is None:
        pytest.skip("g++ not found")
    exe = str(tmp_path / "pose_align")
    build = subprocess.run([gxx, "-std=c++17", "-O2", "-I", CSRC, PROGRAM, "-o", exe], capture_output=True, text=True)
    assert build.returncode == 0, build.stderr[-2000:]
    poses, names = header_cases()
    got = run_program(exe, poses)
    n_T = [0, 0]
    worst_T = worst_d = 0.0
    for i, (pred, gt) in enumerate(poses):
        r3, gap = (float(v[0]) for v in ref.conditioning(pred[None], gt[None]))
        A = ref.cross_covariance(*ref.select(pred[None], gt[None]))[0]
        for m, mode in enumerate((ref.ALIGN_BEST, ref.ALIGN_ROTATION)):
            want = ref.per_pose(pred[None], gt[None], align=mode)
            T, tr, _ = ref.polar(A, mode == ref.ALIGN_ROTATION)
            flipped = mode == ref.ALIGN_ROTATION and got[i, m, 13] < 0
            if r3 >= MIN_RATIO and (not flipped or gap >= MIN_RATIO):
                n_T[m] += 1
                err = max(np.abs(got[i, m, :9].reshape(3, 3) - T[0]).max(), abs(got[i, m, 9] - tr[0]))
                worst_T = max(worst_T, err)
                assert err <= 1e-10, (names[i], mode, err)
                assert abs(got[i, m, 15] - want["scale"][0]) <= 1e-10 * max(1.0, abs(want["scale"][0])), (names[i], mode)
                assert abs(got[i, m, 16] - want["aligned"][0]) <= 1e-10 * max(1.0, abs(want["aligned"][0])), (names[i], mode)
            d = want["d"][0]
            if np.isnan(d):
                assert np.isnan(got[i, m, 14]), (names[i], mode, got[i, m, 14])
            else:
                worst_d = max(worst_d, abs(got[i, m, 14] - d))
                assert abs(got[i, m, 14] - d) <= 1e-10 * max(1.0, abs(d)), (names[i], mode, got[i, m, 14], d)
    print(f"T compared on {n_T} of {len(poses)} poses, worst |T - T_ref| {worst_T:.2e}, worst |d - d_ref| {worst_d:.2e}")
    assert min(n_T) > 1700                                                  # (200 of the seeded poses have 2 or 3 joints: rank <= 2)
    flips = [i for i in range(len(poses)) if got[i, 1, 13] < 0]
    assert len(flips) > 400 and all(got[i, 0, 9] >= got[i, 1, 9] for i in flips)


def test_pose_align_program_is_clean_under_address_and_ub_sanitizers(tmp_path):
    """tools/sanitize/pose_align_asan.cpp under ASan + UBSan on every edge case and 200 seeded poses."""
    clang = "/opt/rocm/lib/llvm/bin/clang++"
    if not os.path.exists(clang):
        pytest.skip("ROCm clang++ not found")
    exe = str(tmp_path / "pose_align_asan")
    build = subprocess.run([clang, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                            "-fno-omit-frame-pointer", "-I", CSRC, PROGRAM, "-o", exe], capture_output=True, text=True)
    if build.returncode != 0 and "sanitizer" in build.stderr.lower() and "cannot find" in build.stderr.lower():
        pytest.skip("sanitizer runtime not installed")
    assert build.returncode == 0, build.stderr[-2000:]
    poses, _ = header_cases()
    poses = poses[:200] + poses[2000:]
    got = run_program(exe, poses)
    assert got.shape == (len(poses), 2, 17)


# ---- the Python layer without a GPU ------------------------------------------------------------------------------------------------------
def _fake_renderer(device="cuda:0"):
    return types.SimpleNamespace(device=device, lib=None, handle=None)


def test_there_is_no_cpu_path():
    with pytest.raises(NotImplementedError, match="no CPU path"):
        pe.PoseScorer(_fake_renderer("cpu"))
    with pytest.raises(NotImplementedError, match="no CPU path"):
        pe.default_scorer("cpu")
    x = np.zeros((2, 14, 3), np.float32)
    for fn in (pe.pa_mpjpe, pe.n_mpjpe, pe.reconstruction_error):
        with pytest.raises(NotImplementedError, match="no CPU path"):
            fn(x, x)
        with pytest.raises(NotImplementedError, match="no CPU path"):
            fn(torch.zeros(2, 14, 3), torch.zeros(2, 14, 3))
    from posegen_amd import ganloop
    with pytest.raises(NotImplementedError, match="no CPU path"):
        ganloop.regressor_feedback(torch.zeros(2, 24, 3), torch.zeros(2, 24, 3))
    with pytest.raises(_ffi.HipLibraryError, match="no renderer"):
        pe.refinement_scores(types.SimpleNamespace(_renderer=[None]), [0], np.zeros((1, 24, 3)))


def test_argument_refusals_come_before_the_device():
    sc = pe.PoseScorer(_fake_renderer())                         # (a renderer that cannot launch anything: lib = None)
    x = np.zeros((2, 14, 3), np.float32)
    with pytest.raises(ValueError, match=r"\[B,J,3\]"):
        sc.score(np.zeros((2, 14, 2)), np.zeros((2, 14, 2)))
    with pytest.raises(ValueError, match=r"\[B,J,3\]"):
        sc.score(x, x[:1])
    with pytest.raises(ValueError, match="no poses"):
        sc.score(x[:0], x[:0])
    with pytest.raises(ValueError, match="at most 64"):
        sc.score(np.zeros((1, 65, 3)), np.zeros((1, 65, 3)))
    with pytest.raises(IndexError, match="joint index"):
        sc.score(x, x, joints=[0, 14])
    with pytest.raises(IndexError, match="joint index"):
        sc.score(x, x, joints=[-1])
    with pytest.raises(ValueError, match="empty joint selection"):
        sc.score(x, x, joints=[])
    with pytest.raises(IndexError, match="root"):
        sc.score(x, x, root=14)
    with pytest.raises(ValueError, match="align"):
        sc.score(x, x, align="similarity")
    with pytest.raises(ValueError, match="align"):
        sc.score(x, x, align=4)
    with pytest.raises(NotImplementedError, match="scaling=False"):
        sc.score(x, x, align=False)
    with pytest.raises(ValueError, match="unit"):
        sc.score(x, x, unit=0.0)
    with pytest.raises(ValueError, match="at most 64"):
        sc.score(x, x, auc_thresholds=np.linspace(0, 150, 64))   # 64 and the PCK threshold
    with pytest.raises(ValueError, match="not finite"):
        sc.score(x, x, pck_threshold=float("nan"))
    for fn in (pe.pa_mpjpe, pe.n_mpjpe, pe.reconstruction_error):
        with pytest.raises(ValueError, match="reduction"):
            fn(x, x, reduction="median", scorer=sc)
    with pytest.raises(ValueError, match="ext_scale"):
        pe.refinement_scores(None, [0], x, ext_scale=0.0)
    # 65 joints of which 64 are selected are accepted up to the launch, which this renderer does not have
    assert pe.PoseScorer._check_selection(65, list(range(64)), 64) == (list(range(64)), 64, 64)
    assert pe.PoseScorer._check_thresholds(1000.0, 150.0, np.linspace(0, 150, 31))[1].shape == (32,)
    assert pe.GAN_LOOP_JOINTS == tuple(ref.GAN_JOINTS) and pe.ALIGN_MODES == ref.MODES


def test_header_binding_and_package_export_the_entry_point():
    import posegen_amd
    hdr = open(os.path.join(REPO, "include", "posegen_hip.h")).read()
    assert re.search(r"int pg_pose_scores\(pg_handle\* h, void\* stream, int64_t B, int J_in, const float\* pred, const float\* gt, "
                     r"const int32_t\* joints, int J,\s+int root, int align, const double\* thresholds, int T, double\* per_pose, "
                     r"float\* aligned, float\* joint_err,\s+double\* summary\);", hdr)
    for code, name in enumerate(("NONE", "SCALE", "BEST", "ROTATION")):
        assert re.search(rf"#define\s+PG_POSE_ALIGN_{name}\s+{code}\b", hdr) and getattr(_ffi, f"PG_POSE_ALIGN_{name}") == code
    assert re.search(r"#define\s+PG_ABI_VERSION\s+11\b", hdr) and _ffi.PG_ABI_VERSION == 11      # an added entry point does not move it
    lib = _ffi.load_library()
    assert hasattr(lib, "pg_pose_scores") and len(_ffi.PROTOTYPES["pg_pose_scores"][1]) == 16
    for name in ("PoseScorer", "pa_mpjpe", "n_mpjpe", "reconstruction_error", "refinement_scores"):
        assert getattr(posegen_amd, name) is getattr(pe, name)
    # a null handle is PG_EINVAL before anything looks for a device
    assert lib.pg_pose_scores(None, None, 1, 14, None, None, None, 14, -1, 2, None, 0, None, None, None, None) == _ffi.PG_EINVAL
