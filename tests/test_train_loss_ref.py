"""The float64 restatement of the trainer's losses (tests/train_loss_ref.py) against the reference Trainer's own float32 values and
autograd gradients (tests/golden/train_losses.npz, tools/gen_golden_train_losses.py).

No tolerance is chosen here.  A loss or stat the reference reports is a float32 mean of N non-negative terms, so it may differ from the
float64 value by the float32 bound of its own arithmetic: (log2 N + 4) 2^-24 relative (pairwise summation log2 N roundings, four more
for forming a term), N = 3n for a photometric loss, the BCE ray count for reg_loss, n 23 6 / n 24 for the pose terms.  PSNR =
-10 log(mse) / log(10): that relative bound of mse is (10 / ln 10) (log2 N + 4) 2^-24 dB, plus 4 2^-24 |psnr| for the float32 log, the
product, the quotient and float32 log(10).  total_loss: the sum of its terms' bounds plus one rounding per addition.  A gradient
element is at most four float32 operations deep, each rounding relative to the largest term that enters it: 8 2^-24 of
max(|element|, the tensor's scale), the scale being the largest photometric term 3 max|d_rgb| max(1, |bg|) for the maps and the
largest element for the pose gradients.

Measured (error / bound, the largest over all cases): losses 0.40, PSNR 0.21, alpha 0.23, map gradients 0.35, pose losses 0.05,
MPJPC 0.11, pose gradients 0.20, gradient norms 0.04."""
import math

import numpy as np
import pytest

from tests import train_loss_ref as ref
from tests.helpers import load_golden

U = 2.0 ** -24


@pytest.fixture(scope="module")
def golden():
    return load_golden("train_losses")


def mean_bound(N):
    return (math.log2(max(N, 1)) + 4.0) * U


def _ratio(got, want, bound):
    return abs(got - want) / bound


def test_fixture_holds_the_cases_the_generator_lists(golden):
    assert len(golden["photo_cases"]) == 9 and len(golden["kp_cases"]) == 3
    ns = [len(golden[f"{c}/acc_map"]) for c in golden["photo_cases"]] + [len(golden[f"{c}/kp_idx"]) for c in golden["kp_cases"]]
    assert min(ns) == 37 and max(ns) == 200


@pytest.mark.parametrize("name", ["mse_scalar", "l1_bgs_bce_coarse", "huber_nobg_coarse", "huber_bgs_bce", "mse_nobg_bce_coarse",
                                  "l1_scalar_coarse", "planted_l1_zero", "planted_huber_knee", "planted_bce"])
def test_photometric_restatement_against_the_reference(golden, name):
    c = ref.golden_case(golden, name)
    kw = ref.photo_settings(c)
    vals, grads = ref.photometric(*ref.photo_inputs(c), **kw)
    n = len(c["acc_map"])
    worst = {"loss": 0.0, "psnr": 0.0, "alpha": 0.0, "grad": 0.0}
    total_bound = 0.0
    for tag in ("", "0"):
        if "rgb_loss" + tag not in vals:
            assert "ref_rgb_loss" + tag not in c
            continue
        b = mean_bound(3 * n) * abs(vals["rgb_loss" + tag])
        total_bound += b
        worst["loss"] = max(worst["loss"], _ratio(float(c["ref_rgb_loss" + tag]), vals["rgb_loss" + tag], b))
        pb = 10.0 / math.log(10.0) * mean_bound(3 * n) + 4.0 * U * abs(vals["psnr" + tag])
        worst["psnr"] = max(worst["psnr"], _ratio(float(c["ref_psnr" + tag]), vals["psnr" + tag], pb))
        if kw["reg_fn"]:
            b = mean_bound(vals["n_bce" + tag]) * abs(vals["reg_loss" + tag])
            total_bound += b
            worst["loss"] = max(worst["loss"], _ratio(float(c["ref_reg_loss" + tag]), vals["reg_loss" + tag], b))
    total_bound += 4.0 * U * abs(vals["total_loss"])
    worst["loss"] = max(worst["loss"], _ratio(float(c["ref_total_loss"]), vals["total_loss"], total_bound))
    worst["alpha"] = _ratio(float(c["ref_alpha"]), vals["alpha"], mean_bound(n) * abs(vals["alpha"]))
    bgmax = max(1.0, float(np.abs(c["bgs"]).max())) if "bgs" in c and kw["use_background"] else 1.0
    for k, g64 in grads.items():
        if k not in c:
            continue
        scale = 3.0 * np.abs(grads["d_rgb0" if k.endswith("0") else "d_rgb_map"]).max() * bgmax
        bound = 8.0 * U * np.maximum(np.abs(g64), scale)
        worst["grad"] = max(worst["grad"], float((np.abs(c[k].astype(np.float64) - g64) / bound).max()))
    print(f"[{name}] error / bound: " + ", ".join(f"{k} {v:.3f}" for k, v in worst.items()))
    assert all(v <= 1.0 for v in worst.values()), worst


def test_planted_values_take_the_branch_the_reference_takes(golden):
    """The exact cases: the L1 derivative at a zero difference is 0; at |d| = beta the Huber derivative is the linear branch's
    sign(d) w / 3n; a ray with y = 1.0 gets no BCE gradient -- in the reference's gradients and in the restatement's, bit for bit
    where the value is exactly representable."""
    c = ref.golden_case(golden, "planted_l1_zero")
    _, g = ref.photometric(*ref.photo_inputs(c), **ref.photo_settings(c))
    zero = c["rgb_map"] == c["target"]
    assert zero.sum() >= 10 and (g["d_rgb_map"][zero] == 0).all() and (c["d_rgb_map"][zero] == 0).all()
    assert (np.abs(g["d_rgb_map"][~zero]) == 1.0 / (3 * len(c["acc_map"]))).all()
    c = ref.golden_case(golden, "planted_huber_knee")
    _, g = ref.photometric(*ref.photo_inputs(c), **ref.photo_settings(c))
    n = len(c["acc_map"])
    for k, w in (("rgb_map", 1.0), ("rgb0", 0.5)):
        d = c[k].astype(np.float64) - c["target"]
        knee = np.abs(d) == 0.125
        assert knee.sum() >= 10
        assert (g["d_" + k][knee] == np.sign(d[knee]) * w / (3 * n)).all()
        assert (c["d_" + k][knee] == (np.sign(d[knee]) * w / (3 * n)).astype(np.float32)).all()
    c = ref.golden_case(golden, "planted_bce")
    kw = ref.photo_settings(c)
    vals, g = ref.photometric(*ref.photo_inputs(c), **kw)
    ones = c["fgs"] == 1.0
    assert ones.sum() >= 4 and vals["n_bce"] == (~ones).sum()
    photo = ref.photometric(*ref.photo_inputs(c), **dict(kw, reg_fn=None))[1]
    assert (g["d_acc_map"][ones] == photo["d_acc_map"][ones]).all() and np.isfinite(g["d_acc_map"]).all()
    assert (g["d_acc_map"][~ones] != photo["d_acc_map"][~ones]).sum() >= (~ones).sum() - 3      # (y = x = 0.5: the BCE derivative is 0)


@pytest.mark.parametrize("name", ["kp_tol0", "kp_tol001_temp", "kp_planted"])
def test_pose_regulariser_restatement_against_the_reference(golden, name):
    c = ref.golden_case(golden, name)
    args, kw = ref.kp_inputs(c)
    vals, grads = ref.pose_regulariser(*args, **kw)
    n = len(c["kp_idx"])
    worst = {"loss": _ratio(float(c["ref_kp_loss"]), vals["kp_loss"], mean_bound(n * 23 * 6) * abs(vals["kp_loss"])),
             "MPJPC": _ratio(float(c["ref_MPJPC"]), vals["MPJPC"], mean_bound(n * 24) * abs(vals["MPJPC"])), "grad": 0.0}
    if int(c["temporal"]):
        worst["loss"] = max(worst["loss"], _ratio(float(c["ref_temp_loss"]), vals["temp_loss"], mean_bound(n * 24 * 9) * abs(vals["temp_loss"])))
    else:
        assert "temp_loss" not in vals and "ref_temp_loss" not in c and "d_kps" not in c and not grads["d_kps"].any()
    assert not grads["d_rots"][..., 2].any()
    for got, want in ((c["d_rots01"], grads["d_rots"][..., :2]), (c.get("d_kps"), grads["d_kps"])):
        if got is not None:
            bound = 8.0 * U * np.maximum(np.abs(want), np.abs(want).max())
            worst["grad"] = max(worst["grad"], float((np.abs(got.astype(np.float64) - want) / bound).max()))
            assert ((got == 0) == (want == 0)).all()                        # the same elements masked out
    if not int(c["temporal"]):
        assert not grads["d_rots"][:, 0].any()                               # the root joint gets only the temporal term
    print(f"[{name}] error / bound: " + ", ".join(f"{k} {v:.3f}" for k, v in worst.items()))
    assert all(v <= 1.0 for v in worst.values()), worst


def test_planted_threshold_is_excluded(golden):
    """x = tol = 0.015625 exactly: the strict > leaves the element out, in the reference's gradient and in the restatement's"""
    c = ref.golden_case(golden, "kp_planted")
    args, kw = ref.kp_inputs(c)
    _, grads = ref.pose_regulariser(*args, **kw)
    idx = c["kp_idx"].astype(np.int64)
    x = ((c["anchor_rots"].astype(np.float64) - c["rots"])[idx][..., :2]) ** 2
    at = x == 0.015625
    at[:, 0] = False
    assert at.sum() >= 100
    assert (grads["d_rots"][..., :2][at] == 0).all() and (c["d_rots01"][at] == 0).all()
    above = x > 0.015625
    above[:, 0] = False
    assert (grads["d_rots"][..., :2][above] != 0).all()


def test_gradient_norms_restatement_against_the_reference(golden):
    g = ref.golden_case(golden, "norms")
    tensors = [g[f"g{i}"] for i in range(5)]
    assert [t.size for t in tensors] == [1, 3, 128, 257, 256 * 7]
    total, avg, per = ref.grad_norms(tensors)
    b = mean_bound(sum(t.size for t in tensors))
    worst = max(_ratio(float(g["ref_total_norm"]), total, b * total), _ratio(float(g["ref_avg_norm"]), avg, b * avg))
    print(f"[norms] error / bound: {worst:.3f}")
    assert worst <= 1.0
    assert avg == math.sqrt(total * total / 5) or abs(avg - total / math.sqrt(5)) <= 1e-15 * avg
    np.testing.assert_allclose(per, [np.sqrt((t.astype(np.float64) ** 2).sum()) for t in tensors], rtol=1e-15)
