"""The on-chip form's Y segment (pg_eval16r.hip y_segment16) against the record form: the same calls
rendered with set_onchip("always") and set_onchip("records").  Y -- the view layer's direction part -- reaches the colour
only, so acc_map and disp_map of the two forms are equal bit for bit, and rgb_map agrees within the forms' own rounding
(bf16 1e-3, fp16 2e-4).

The calls (tests/diag/y_segment_cases.py) are chosen for what a change of y_segment16 can break: 1, 3, 37 and 1024 rays of
the 32 x 32 all-hit frame at pose spreads 0.2 and 0.6; 64 + 16 and 96 + 16 samples, i.e. passes of 4, 3.2, 2.67 and 2.3 rays,
so that a pass has 1 .. 5 rays (nrm1 = 0 .. 4) and the last pass is ragged; bf16 and fp16; one pose, a pose per ray, frame
codes; the default grid and POSEGEN_MAX_WG=1, where one workgroup walks every pass and each pass finds the limbs of all
earlier passes still in the Y image.  That the rays put some limbs in range of a pass and leave others out, and that the
body is there, is checked on the CPU with the oracle."""
import json
import os
import subprocess
import sys

import pytest
import torch

from oracle import anerf_oracle as orc
from posegen_amd import surreal_config, synthetic as syn
from tests.diag import y_segment_cases as cases
from tests.helpers import oracle_cfg, torch_weights
from tools.diag_empty_waves import limbs_in_range, pass_figures

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RGB_BOUND = {"bf16": 1e-3, "fp16": 2e-4}            # form to form


@pytest.mark.parametrize("rays", list(cases.RAY_SETS))
def test_rays_put_limbs_in_and_out_of_range_on_the_oracle(rays):
    """fp32 oracle, coarse launch at 64 samples: some pass of the call has limbs in range and limbs out of range (by point:
    within the distance beyond which the cutoff weight is below 2^-24), and at least a tenth of the rays have a live point
    (sigma > 0) -- with the frame's pose and, for the per-ray-pose calls, with the alternating second pose."""
    cfg = surreal_config()
    wc, wf, tv, td = syn.make_model(cfg, 0)
    rb, skts, cyl = cases.rays_of(rays, "cpu")
    n = rb.shape[0]
    for sk in (skts[None], cases.per_ray_poses(skts, n, "cpu")):
        with torch.no_grad():
            ex = orc.render_rays(rb, sk, cyl, oracle_cfg(cfg, tv, td), torch_weights(wc), torch_weights(wf), 64, 0,
                                 return_extras=True)["extras"]
        sigma = ex["raw_coarse"][..., 3]
        fig = pass_figures(sigma, limbs_in_range(rb, ex["z_coarse"], sk, cfg, tv, td))
        live_rays = float((sigma > 0).any(1).float().mean())
        print(rays, fig, "live rays", live_rays)
        assert fig["passes_with_limbs_in_and_out"] >= 1, (rays, fig)
        assert live_rays >= 0.1, (rays, live_rays)


@pytest.fixture(scope="module")
def default_grid():
    return cases.run_cases("cuda:0")


@pytest.fixture(scope="module")
def one_workgroup():
    env = {k: v for k, v in os.environ.items() if k not in ("POSEGEN_MAX_WG", "POSEGEN_ONCHIP", "POSEGEN_PASS_WALK")}
    env["POSEGEN_MAX_WG"] = "1"
    run = subprocess.run([sys.executable, os.path.join(REPO, "tests", "diag", "y_segment_cases.py")], capture_output=True, text=True,
                         timeout=600, env=env, cwd=REPO)
    assert run.returncode == 0, run.stderr[-2000:]
    return json.loads([l for l in run.stdout.splitlines() if l.startswith("Y_SEGMENT ")][-1][len("Y_SEGMENT "):])


def _check(d, case):
    print(case, d)
    prec = case.split("-")[0]
    assert d["finite"], (case, d)
    assert d["acc_map_equal"] and d["disp_map_equal"], (case, d)
    assert d["rgb_map"] <= RGB_BOUND[prec], (case, d)
    if case.split("-")[2].startswith("1024"):
        assert d["acc_max"] > 0.5, (case, d)            # the rays do cross the body


@pytest.mark.gpu
@pytest.mark.parametrize("case", cases.CASE_IDS)
def test_on_chip_form_against_record_form(default_grid, case):
    _check(default_grid[case], case)


@pytest.mark.gpu
@pytest.mark.parametrize("case", cases.CASE_IDS)
def test_on_chip_form_against_record_form_one_workgroup(one_workgroup, case):
    _check(one_workgroup[case], case)
