"""The direction operands of a pass of the 16x16x32 kernel (pg_eval16r.hip dir_operands16): a pass forms
the bone-local position of the lane's 12 (joint slot, point) pairs once, in front of layer 0, and from it the wave's limb mask
and the B fragments that both x phases -- layer 0 and the skip layer, a whole trunk apart -- take ready.  What is carried
through a pass must not depend on which pass a workgroup ran before, nor on how many passes it runs:

  walk      the default grid (every workgroup runs one pass of these small calls), POSEGEN_MAX_WG=1 (one workgroup walks every
            pass) and POSEGEN_MAX_WG=2 render the same bytes: raw_coarse, raw_fine and the maps of 1 x 64, 4 x 64, 5 x 64, 13 x 80,
            7 x 113 (records) and 3 x 171 (records: the last pass is ONE point) rays x samples, bf16 and fp16, both forms, one pose,
            a pose per ray, frame codes; and pg_stage_eval of the edge inputs below;
  float64   under POSEGEN_MAX_WG=1, pg_stage_eval against tests/eval_ref.py with the bounds of tests/eval_cases.py (bound_16bit,
            2 x the RMS yardstick) on seams (1 x 64, 5 x 64, 13 x 80, 7 x 113, 3 x 171), all_far, on_joint and cutoffs at tau_d = -4 (no
            masks at all) and at (400, 4);
  masks     the 13 x 80 call with the limb masks off against the default, one workgroup, within the per-ray bound of
            test_limb_skipping_changes_nothing_beyond_rounding (1e-3 bf16, 1e-4 fp16); and the kernel's own count of limbs left out
            per wave (limb_skip_stats, the CNT instantiation) equals the formula restated on the host.

The switch is read once per process: three child processes (tests/diag/x_operands_cases.py), one per grid, started once for
the module.  Worst measured / bound of the float64 part on an MI355X (max-abs or RMS, whichever is closer): bf16 0.58, fp16 0.58."""
import json
import os
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MASK_TOL = {"bf16": 1e-3, "fp16": 1e-4}         # tests/test_gpu_frames.py test_limb_skipping_changes_nothing_beyond_rounding
ARRAYS = ("raw_coarse", "raw_fine", "rgb_map", "disp_map", "acc_map")


def _child(env, *args):
    e = {k: v for k, v in os.environ.items() if k not in ("POSEGEN_PASS_WALK", "POSEGEN_MAX_WG", "POSEGEN_ONCHIP")}
    e.update(env)
    run = subprocess.run([sys.executable, os.path.join(REPO, "tests", "diag", "x_operands_cases.py"), *args],
                         capture_output=True, text=True, timeout=300, env=e, cwd=REPO)
    assert run.returncode == 0, (env, run.stderr[-2000:])
    line = [l for l in run.stdout.splitlines() if l.startswith("X_OPERANDS ")][-1]
    return json.loads(line[len("X_OPERANDS "):])


@pytest.fixture(scope="module")
def grids():
    return {"default": _child({}), "one": _child({"POSEGEN_MAX_WG": "1"}, "ref"), "two": _child({"POSEGEN_MAX_WG": "2"})}


def test_calls_cover_the_shapes(grids):
    keys = set(grids["default"])
    assert keys == set(grids["one"]) - {"masks:bf16", "masks:fp16"} == set(grids["two"])
    walk = [k for k in keys if k.startswith("walk:")]
    # 3 models x (4 shapes x 2 forms + 2 record-only shapes) x 2 precisions
    assert len(walk) == 3 * (4 * 2 + 2) * 2
    assert any(k.endswith(":3x171:bf16:records") for k in walk) and any(":7x113:" in k for k in walk)
    assert len([k for k in keys if k.startswith("stage:")]) == 11 * 2 * 2 * 2


def test_walk_independence(grids):
    """default grid: operands of every pass from that workgroup's first (only) pass; one workgroup: every pass but the first
    behind another pass of the same workgroup.  Byte for byte the same."""
    ref = grids["default"]
    for key, want in ref.items():
        if not key.startswith("walk:"):
            continue
        assert want["finite"], key
        for label in ("one", "two"):
            got = grids[label][key]
            assert got["finite"], (label, key)
            for k in ARRAYS:
                assert got[k] == want[k], f"{key}: {k} with POSEGEN_MAX_WG={1 if label == 'one' else 2} differs from the default grid's"


def test_stage_eval_is_grid_independent(grids):
    for key, want in grids["default"].items():
        if key.startswith("stage:"):
            for label in ("one", "two"):
                assert grids[label][key]["raw"] == want["raw"], (label, key)


def test_against_float64_with_one_workgroup(grids):
    worst = {}
    bad = []
    for key, d in grids["one"].items():
        if not key.startswith("stage:"):
            continue
        prec = key.split(":")[-2]
        print(f"[{key}] raw max {d['emax']:.3e} <= {d['bmax']:.3e}; rms {d['erms']:.3e} <= {d['brms']:.3e}")
        worst[prec] = max(worst.get(prec, 0.0), d["emax"] / d["bmax"], d["erms"] / d["brms"])
        if not (d["finite"] and d["emax"] <= d["bmax"] and d["erms"] <= d["brms"]):
            bad.append(key)
    print("worst measured / bound:", worst)
    assert not bad, bad


def test_last_pass_of_one_point(grids):
    """3 x 171 = 2 x 256 + 1 points: the last pass holds one point, every other lane repeats it"""
    keys = [k for k in grids["one"] if ":3x171:" in k or "seams[3x171]" in k]
    assert len(keys) == 3 * 2 + 2 * 2 * 2
    for k in keys:
        assert grids["one"][k]["finite"] and grids["default"][k]["finite"], k


@pytest.mark.parametrize("prec", ["bf16", "fp16"])
def test_limb_masks(grids, prec):
    d = grids["one"][f"masks:{prec}"]
    print(prec, d)
    assert d["finite"]
    for k in ("rgb_map", "acc_map", "rgb0", "acc0"):
        assert d[k] <= MASK_TOL[prec], (prec, k, d[k])
    for which in (0, 1):
        c = d[f"count{which}"]
        # (the host restates the formula in float64: only meaningful when no point sits at a radius to within fp32 rounding)
        assert c["margin"] > 1e-5, c
        assert 0 < c["host_left_out"] < 48 * c["host_passes"], c           # (the call has limbs in range and limbs out of it)
        assert c["passes"] == c["host_passes"] and c["left_out"] == c["host_left_out"], (prec, which, c)
