"""The pass walk of the fused kernels with limb masks (pg_device.h PassWalk).

Which workgroup runs a pass must not show in any output byte: the rotated walk (the default) and the static walk
(POSEGEN_PASS_WALK=0) render bitwise equal raw, rgb_map, disp_map and acc_map, in every kernel that uses the walk
(pg_eval16r.hip record and on-chip forms, with frame codes and with a pose per ray; pg_evalc2.hip) -- a child
process per (case, walk), since the switches are read once per process (tests/diag/pass_walk_cases.py).  And every pass runs
exactly once: the kernels' own pass counters on the GPU, and the walk itself on the host (pg_debug_pass_walk: the two-step
update of (first point, ray, sample) against the integer division, for every pass of a 2^19-ray call).

The dynamic claim of the issue (an atomic counter and a host-made reciprocal of S) is not built -- the rotated walk left no
spread for it to remove (profiles/pass_walk_imbalance.txt) -- so there is no reciprocal to test; the host test covers the
division-free update that is there instead."""
import ctypes as C
import json
import os
import subprocess
import sys

import pytest

from posegen_amd import _ffi

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIG = (1 << 19) + 1000          # more rays than one launch takes (pg_api.hip launch_eval: 2^19 per launch)

# id -> (case of tests/diag/pass_walk_cases.py, environment of both children)
CASES = {
    # 4099 rays: no sample count makes that a whole number of passes; 1025 to 4612 passes = 5 to 37 rounds of the grid
    "bf16": ("surreal:bf16:one:4099:64,80,128,144", {}),
    "fp16": ("surreal:fp16:one:4099:64,80,128,144", {}),
    "fp16c": ("surreal:fp16c:one:4099:64,80,128,144", {}),
    # fewer passes than workgroups (10 to 21 passes of 256 points)
    "few_passes_bf16": ("surreal:bf16:one:37:64,80,128,144", {}),
    "few_passes_fp16c": ("surreal:fp16c:one:37:64,80,128,144", {}),
    "max_wg_1_bf16": ("surreal:bf16:one:301:64,128", {"POSEGEN_MAX_WG": "1"}),
    "max_wg_7_bf16": ("surreal:bf16:one:301:64,128", {"POSEGEN_MAX_WG": "7"}),
    "max_wg_1_fp16c": ("surreal:fp16c:one:301:64,128", {"POSEGEN_MAX_WG": "1"}),
    "max_wg_7_fp16c": ("surreal:fp16c:one:301:64,128", {"POSEGEN_MAX_WG": "7"}),
    "pose_per_ray_bf16": ("surreal:bf16:per_ray:1501:64,128", {}),
    "pose_per_ray_fp16c": ("surreal:fp16c:per_ray:1501:64,128", {}),
    "framecodes_bf16": ("h36m:bf16:one:4099:64,128", {}),
    "framecodes_fp16c": ("h36m:fp16c:one:4099:64,128", {}),
    "above_one_launch_bf16": (f"surreal:bf16:one:{BIG}:64", {}),
    # the other form that walks: the 16x16x32 kernel with per-ray records
    "records_bf16": ("surreal:bf16:one:4099:64,144", {"POSEGEN_ONCHIP": "0"}),
}
TWICE = ("bf16", "fp16c", "framecodes_bf16")        # the default walk twice: the same bytes


def _child(case, env):
    e = {k: v for k, v in os.environ.items() if k not in ("POSEGEN_PASS_WALK", "POSEGEN_MAX_WG", "POSEGEN_ONCHIP")}
    e.update(env)
    run = subprocess.run([sys.executable, os.path.join(REPO, "tests", "diag", "pass_walk_cases.py"), case],
                         capture_output=True, text=True, timeout=300, env=e, cwd=REPO)
    assert run.returncode == 0, (case, env, run.stderr[-2000:])
    line = [l for l in run.stdout.splitlines() if l.startswith("PASS_WALK ")][-1]
    return json.loads(line[len("PASS_WALK "):])


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(CASES))
def test_rotated_walk_is_bitwise_the_static_walk(name):
    case, env = CASES[name]
    static = _child(case, dict(env, POSEGEN_PASS_WALK="0"))
    rotated = _child(case, env)
    runs = [("static", static), ("rotated", rotated)]
    if name in TWICE:
        runs.append(("rotated again", _child(case, env)))
    for S, ref in static.items():
        assert ref["finite"], (name, S, ref)
        for label, res in runs:
            for k in ("raw", "rgb_map", "disp_map", "acc_map"):
                assert res[S][k] == ref[k], f"{name}: S={S} {k} of the {label} walk differs from the static walk's"
            if "passes" in ref:
                assert res[S]["passes_counted"] == res[S]["passes"], (name, S, label, res[S])


def test_host_walk_takes_every_pass_once_without_a_division():
    """pg_debug_pass_walk (pg_api.hip): every workgroup of the grid walks its passes on the host through the same PassWalk the
    kernels use; counts passes whose (first point, ray, sample) differ from the integer division of the pass index, passes out
    of round order, and passes taken twice or never.  Every S in 32 .. 160 on a 2^19-ray call, both pass sizes, the full grid
    with the default rotation and with none, and grids the rotation does not fit in."""
    lib = _ffi.load_library()
    fn = lib.pg_debug_pass_walk
    fn.restype = C.c_longlong
    fn.argtypes = [C.c_longlong, C.c_int, C.c_int, C.c_int, C.c_int]
    for S in range(32, 161):
        for pts in (128, 256):
            for G, rho in ((256, 99), (256, 0), (7, 99 % 7)):
                assert fn(1 << 19, S, pts, G, rho) == 0, (S, pts, G, rho)
    for G in (1, 2, 3, 64, 99, 100, 255, 512):
        for n in (1, 37, 4099):
            assert fn(n, 64, 256, G, 99 % G) == 0 and fn(n, 81, 128, G, 99 % G) == 0, (G, n)
    assert fn(4099, 64, 256, 7, 7) == -1         # a rotation must be below the grid size
