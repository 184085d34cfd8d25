"""scene_composite_kernel (pg_scene.hip) through pg_stage_scene_composite against the float64 restatement at the kernel's own
float32 inputs (tests/scene_ref.py; pinned by tests/test_scene_host.py): 70 pixels, P in {1, 2, 3, 8} people, S in {2, 33, 64, 65,
129, 256} samples per list -- the lane-packing and wave edges --, both density activations, everybody everywhere or mixed presence
maps with pixels nobody covers.  Every output, person_acc included, is held to composite_ref.bound: 4 x the float32 restatement's
deviation from the float64 one, at least 4 float32 ulps.  Each comparison prints the device's deviation and the bound."""
import numpy as np
import pytest
import torch

from posegen_amd import PREC_FP32
from posegen_amd.scene import stage_scene_composite
from tests import composite_ref as cr
from tests import scene_ref as sr

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
F64, F32 = torch.float64, torch.float32
OUTPUTS = ("rgb_map", "disp_map", "acc_map", "person_acc")
WORST = [0.0, ""]


@pytest.fixture(scope="module")
def renderers():
    """one handle per density activation; the stage needs no weights"""
    from posegen_amd.raycaster import HipRenderer
    rs = {d: HipRenderer(cr.render_cfg(d), device=DEV, precision=PREC_FP32) for d in cr.DENSITIES}
    yield rs
    for r in rs.values():
        r.close()
    print(f"worst device deviation / bound: {WORST[0]:.3f} ({WORST[1]})")


def run(r, s):
    T = lambda a: torch.from_numpy(np.ascontiguousarray(a))
    o = stage_scene_composite(r, [T(z) for z in s["z"]], [T(w) for w in s["raw"]], T(s["rows"]), T(s["dirs"]))
    torch.cuda.synchronize()
    return {k: v.cpu().numpy() for k, v in o.items()}


def hold(label, got, r32, r64):
    dev, b = cr.deviation(got, r64), cr.bound(r32, r64)
    print(f"{label}: device {dev:.2e} bound {b:.2e} ratio {dev / b:.2f}")
    if dev / b > WORST[0]:
        WORST[:] = [dev / b, label]
    assert np.isfinite(np.asarray(got)).all(), label
    assert dev <= b, f"{label}: device {dev:.2e} beyond 4 x the float32 restatement's own deviation, {b:.2e}"


@pytest.mark.parametrize("kind", ["all", "mixed"])
@pytest.mark.parametrize("density", cr.DENSITIES)
@pytest.mark.parametrize("S", sr.SAMPLES)
@pytest.mark.parametrize("P", sr.PEOPLE)
def test_merged_composite_value_by_value(renderers, P, S, density, kind):
    s = sr.make_scene(P, S, density, kind)
    r64, r32 = sr.reference(s, F64), sr.reference(s, F32)
    o = run(renderers[density], s)
    for k in OUTPUTS:
        hold(f"P{P}-S{S}-{density}-{kind} {k}", o[k], r32[k], r64[k])
    # exact: a pixel nobody covers is all zero, and so is person_acc wherever the person is absent
    here = np.stack([sr._present(s, p)[1] for p in range(P)])
    nobody = ~here.any(0)
    assert nobody[[3, 40]].all() if kind == "mixed" else not nobody.any()
    for k in ("rgb_map", "disp_map", "acc_map"):
        assert not o[k][nobody].any(), k
    assert not o["person_acc"][~here].any()
    assert np.all(o["acc_map"][~nobody] > 0)
    # exact: no atomics, a fixed reduction order -- a second run gives the same bits
    again = run(renderers[density], s)
    for k in OUTPUTS:
        assert np.array_equal(o[k], again[k]), k


@pytest.mark.parametrize("S", [2, 65, 256])
def test_one_empty_list_gives_acc_0_and_disp_0(renderers, S):
    """P = 1, relu, every sigma <= 0 (a fifth exactly 0): every weight is 0"""
    s = sr.single(cr.make_case_empty(S, 2 if S % 2 == 0 else 3, "plain") if S > 2 else _empty2())
    o = run(renderers["relu"], s)
    for k in OUTPUTS:
        assert not o[k].any(), k


def _empty2():
    c, _ = cr._bare_case(2, 0, "plain", "relu", cr.N_RAYS, 9)
    c["raw"][..., 3] = np.float32(-0.25)
    return c


def test_bad_arguments_are_refused_before_any_launch(renderers):
    r = renderers["relu"]
    s = sr.make_scene(2, 33, "relu", "all")
    T = lambda a: torch.from_numpy(np.ascontiguousarray(a))
    from posegen_amd._ffi import PgError
    with pytest.raises(PgError):        # nine lists
        stage_scene_composite(r, [T(s["z"][0])] * 9, [T(s["raw"][0])] * 9, T(np.zeros((9, sr.N_PIX), np.int32)), T(s["dirs"]))
    with pytest.raises(PgError):        # 257 samples
        stage_scene_composite(r, [torch.zeros(4, 257)], [torch.zeros(4, 257, 4)], T(np.zeros((1, sr.N_PIX), np.int32)), T(s["dirs"]))
    # rows outside a list are absent, not read: the whole map of person 1 points past its list
    rows = s["rows"].copy()
    rows[1] = s["z"][1].shape[0] + 5
    o = run(r, {**s, "rows": rows})
    alone = run(r, {**s, "z": s["z"][:1], "raw": s["raw"][:1], "rows": s["rows"][:1]})
    assert np.array_equal(o["rgb_map"], alone["rgb_map"]) and not o["person_acc"][1].any()
