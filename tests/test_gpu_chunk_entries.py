"""The A pipe of the 16x16x32 kernel across chunk entries (pg_eval16r.hip hidden layers).

The last units of a chunk of a hidden layer issue the ring reads of the next chunk's first units ahead of that chunk's barrier, and
the entry in front has waited for the next chunk's refill as well.  An LDS-DMA that lands behind such a read returns the bytes the
slot held before, silently: what shows it is a byte that changes from one run of a call to the next, or with the grid (one workgroup
walks every pass of a call, so the weight stream wraps in every pass and every mask hands over; many workgroups run one pass each).
tests/diag/chunk_entries_cases.py renders the cases in a child process per grid -- the default, POSEGEN_MAX_WG=1 and =2 -- three
times each, bf16 and fp16, on-chip and record form, and reports digests of raw_coarse / raw_fine and the maps.

Bounds are the project's own: limb masks on / off as test_limb_skipping_changes_nothing_beyond_rounding (tests/test_gpu_frames.py)
holds them; raw against the float64 restatement as tests/eval_cases.py bounds every 16-bit form (D of the case + EMUL_TOL, RMS <=
2 D_rms).  The edge inputs of tests/golden/eval_edges.npz have 33 depths per ray, below the kernel's 64: the child runs them with the
midpoints between the fixture's depths as well, 66 per ray.  The 1 ray x 32 samples call of the list is likewise below 64: it runs the
direct kernel (pg_eval16.hip) and exercises nothing of this change; 1 x 64 stands beside it."""
import json
import os
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GRIDS = {"default": {}, "max_wg_1": {"POSEGEN_MAX_WG": "1"}, "max_wg_2": {"POSEGEN_MAX_WG": "2"}}
MASK_TOL = {"bf16": 1e-3, "fp16": 1e-4}         # test_limb_skipping_changes_nothing_beyond_rounding
_RUNS = {}


def run(grid):
    """the child's report for a grid, computed once per session (the default grid's with the float64 comparisons)"""
    if grid not in _RUNS:
        e = {k: v for k, v in os.environ.items() if k not in ("POSEGEN_PASS_WALK", "POSEGEN_MAX_WG", "POSEGEN_ONCHIP")}
        e.update(GRIDS[grid])
        # (the float64 comparisons where one workgroup walks every pass, and on the default grid)
        args = ["ref"] if grid in ("default", "max_wg_1") else []
        res = subprocess.run([sys.executable, os.path.join(REPO, "tests", "diag", "chunk_entries_cases.py")] + args,
                             capture_output=True, text=True, timeout=300, env=e, cwd=REPO)
        assert res.returncode == 0, (grid, res.stderr[-2000:])
        line = [l for l in res.stdout.splitlines() if l.startswith("CHUNK_ENTRIES ")][-1]
        _RUNS[grid] = json.loads(line[len("CHUNK_ENTRIES "):])
    return _RUNS[grid]


def digests(rep):
    return {k: v for k, v in rep.items() if isinstance(v, str)}


@pytest.mark.parametrize("grid", list(GRIDS))
def test_three_runs_of_a_call_give_the_same_bytes(grid):
    out = run(grid)
    calls = [k for k in out if k.startswith(("walk:", "stage:"))]
    assert len(calls) == 6 * 4 + 3 * 2 * 4
    for key in calls:
        reps = out[key]
        assert len(reps) == 3 and all(r["finite"] for r in reps), key
        for r in reps[1:]:
            assert digests(r) == digests(reps[0]), f"{grid} {key}: a run differs from the first"


@pytest.mark.parametrize("grid", ["max_wg_1", "max_wg_2"])
def test_the_grid_does_not_show_in_a_byte(grid):
    ref, out = run("default"), run(grid)
    for key, reps in ref.items():
        if key.startswith(("walk:", "stage:")):
            assert digests(out[key][0]) == digests(reps[0]), f"{key}: {grid} differs from the default grid"


def test_raw_coarse_and_raw_fine_are_compared():
    """every two-stage call reports both raws, and the two forms of the kernel were both asked for"""
    out = run("default")
    for key, reps in out.items():
        if key.startswith("walk:"):
            assert "raw_coarse" in reps[0] and (("raw_fine" in reps[0]) == (not key.split(":")[3].endswith("+0"))), key
    assert {k.split(":")[-1] for k in out if k.startswith("walk:")} == {"always", "records"}
    assert {k.split(":")[-2] for k in out if k.startswith("walk:")} == {"bf16", "fp16"}


@pytest.mark.parametrize("grid", ["default", "max_wg_1"])
def test_edge_inputs_within_the_float64_bounds(grid):
    """no limb in range of any pass, tau_d <= 0 (nothing masked), and the eval_edges.npz inputs (per-joint cutoffs, tau_v != tau_d):
    per-point raw of both nets, both precisions, both forms, within the bounds of tests/eval_cases.py -- also where one workgroup
    walks every pass"""
    out = run(grid)
    keys = [k for k in out if k.startswith("stage:")]
    assert {k.split(":")[1] for k in keys} >= {"eval_edges_66"} and len(keys) == 24
    for key in keys:
        d = out[key][-1]
        print(f"[{grid} {key}] raw max {d['emax']:.3e} <= {d['bmax']:.3e}; rms {d['erms']:.3e} <= {d['brms']:.3e}")
        assert d["emax"] <= d["bmax"] and d["erms"] <= d["brms"], (grid, key, d)


@pytest.mark.parametrize("grid", ["default", "max_wg_1"])
def test_limb_masks_and_empty_waves_change_nothing_beyond_rounding(grid):
    out = run(grid)
    keys = [k for k in out if k.startswith("masks:")]
    assert len(keys) == 4
    for key in keys:
        d, prec = out[key], key.split(":")[1]
        assert d["finite"] and d["acc_max"] > 0.5, (key, d)
        for k in ("rgb_map", "acc_map", "rgb0", "acc0"):
            print(f"[{grid} {key}] {k}: masks on - off max {d[k]['max']:.3e} mean {d[k]['mean']:.3e} rays {d[k]['frac']:.4f}")
            assert d[k]["max"] <= MASK_TOL[prec] and d[k]["mean"] <= 1e-8 and d[k]["frac"] <= 0.03, (grid, key, k, d[k])
        assert all(d["empty_skip_same"].values()), (grid, key, d["empty_skip_same"])
