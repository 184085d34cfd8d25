"""The scene compositor's yardstick (tests/scene_ref.py) and the host side of scenes (posegen_amd/scene.py, the two entry points of
include/posegen_hip.h), pinned without a GPU before tests/test_gpu_scene_stages.py and tests/test_gpu_scene.py measure anything by
them."""
import ctypes as C
import os
import re
import types

import numpy as np
import pytest
import torch

from posegen_amd import _ffi, scene, synthetic as syn
from tests import composite_ref as cr
from tests import scene_ref as sr

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F64 = torch.float64
MAPS = ("rgb_map", "disp_map", "acc_map", "wsum")


@pytest.mark.parametrize("case", [(33, 7, "plain", False, "relu"), (65, 16, "plain", False, "softplus"), (256, 0, "plain", False, "relu")],
                         ids=cr.case_id)
def test_one_person_is_the_composite_oracle(case):
    """P = 1: the merged order is the list's own, and every map is composite_ref.reference's to 1e-13"""
    c = cr.make_case_a(*case)
    want, got = cr.reference(c, F64), sr.reference(sr.single(c), F64)
    for k in MAPS:
        assert cr.deviation(got[k], want[k]) <= 1e-13, k
    assert cr.deviation(got["person_acc"][0], want["acc_map"]) <= 1e-13


def test_permuting_people_permutes_person_acc_and_nothing_else():
    s = sr.make_scene(3, 33, "relu", "mixed")
    assert not sr.cross_list_ties(s)
    perm = (2, 0, 1)
    a, b = sr.reference(s, F64), sr.reference(sr.permuted(s, perm), F64)
    for k in MAPS:
        assert cr.deviation(b[k], a[k]) <= 1e-13, k
    assert cr.deviation(b["person_acc"], a["person_acc"][list(perm)]) <= 1e-13
    # the scene is one where the order matters: person 0 alone is not the scene
    alone = sr.reference({**s, "z": s["z"][:1], "raw": s["raw"][:1], "rows": s["rows"][:1]}, F64)
    assert cr.deviation(alone["rgb_map"], a["rgb_map"]) > 1e-2


def test_two_identical_lists_follow_the_tie_rule():
    """the same depths twice: (0,0), (1,0), (0,1), (1,1), ... -- person 0's sample k stands in front of person 1's sample k"""
    S, n = 5, 4
    c = cr.make_case_a(S, 0, "plain", False, "relu", n=n)
    rng = np.random.default_rng(3)
    raw1 = c["raw"].copy()
    raw1[..., :3] = rng.normal(0, 2, (n, S, 3)).astype(np.float32)
    raw1[..., 3] = (c["raw"][..., 3] * 1.5).astype(np.float32)
    s = {"S": S, "density": "relu", "dirs": np.ascontiguousarray(c["rays"][:, 3:6]), "z": [c["z"], c["z"].copy()], "raw": [c["raw"], raw1],
         "rows": np.stack([np.arange(n), np.arange(n)]).astype(np.int32)}
    got = sr.reference(s, F64)
    each = [cr.reference({**c, "raw": r}, F64) for r in (c["raw"], raw1)]       # per-list alpha, on the list's own deltas
    eps = cr.oracle_config("relu").rgb_eps
    for i in range(n):
        T, rgb, pacc = 1.0, np.zeros(3), [0.0, 0.0]
        for k in range(S):
            for p in (0, 1):
                a = each[p]["alpha"][i, k]
                col = 1.0 / (1.0 + np.exp(-s["raw"][p][i, k, :3].astype(np.float64))) * (1 + 2 * eps) - eps
                rgb += a * T * col
                pacc[p] += a * T
                T *= 1.0 - a + 1e-10
        assert np.abs(got["rgb_map"][i] - rgb).max() <= 1e-13
        assert np.abs(got["person_acc"][:, i] - np.minimum(pacc, 1.0)).max() <= 1e-13
    swapped = sr.reference(sr.permuted(s, (1, 0)), F64)
    assert cr.deviation(swapped["rgb_map"], got["rgb_map"]) > 1e-3, "with ties, who comes first is visible"


@pytest.mark.parametrize("case", sr.TIE_CASES, ids=lambda c: "P%d-S%d-%s-%s" % c)
def test_tie_scenes_have_ties_whose_order_is_visible(case):
    """every tie scene the device is measured on (tests/test_gpu_scene_edges.py): people share depths, the reversed people give
    another picture, and -- by construction of the bound; asserted so that no generator change can hide a case -- the float32
    restatement is within composite_ref.bound of the float64 one"""
    P, S, density, kind = case
    s = sr.make_scene_ties(*case)
    assert sr.cross_list_ties(s)
    assert all(z.dtype == np.float32 and np.all(np.diff(z, axis=-1) >= 0) for z in s["z"]), "every list is non-decreasing"
    here = np.stack([sr._present(s, p)[1] for p in range(P)])
    assert all(z.shape[0] == h.sum() + 2 for z, h in zip(s["z"], here)), "two rows no pixel refers to"
    assert not here[:, [3, 40]].any() and here[:, 5].all() and (here.sum(0) >= 2).sum() > 10
    r64, r32 = sr.reference(s, F64), sr.reference(s, torch.float32)
    back = sr.reference(sr.permuted(s, tuple(reversed(range(P)))), F64)
    assert cr.deviation(back["rgb_map"], r64["rgb_map"]) > 1e-3, "with ties, who comes first is visible"
    for k in MAPS + ("person_acc",):
        assert np.isfinite(r64[k]).all() and cr.deviation(r32[k], r64[k]) <= cr.bound(r32[k], r64[k]), k
    if kind == "flat":
        i = 5                   # everybody covers it, all depths are equal: only each list's last sample has a delta
        zs = np.stack([s["z"][p][s["rows"][p, i]] for p in range(P)])
        assert np.all(zs == zs[0, 0])
    if kind == "runs":
        z0 = s["z"][0][s["rows"][0, 5]]
        assert np.all(z0[1:2 * (S // 2):2] == z0[0:2 * (S // 2):2]) and np.array_equal(s["z"][1][s["rows"][1, 5]], z0)


def test_the_many_pixel_scene_and_the_disparity_scene_are_what_they_say():
    n = 1000
    s = sr.make_scene_many(5, n)
    here = np.stack([sr._present(s, p)[1] for p in range(5)])
    assert s["S"] == 3 and s["dirs"].shape == (n, 3) and not sr.cross_list_ties({**s, "dirs": s["dirs"][:70]})
    assert (~here.any(0))[600:].sum() > 10 and here.all(0)[600:].sum() > 10 and 0.4 < here.mean() < 0.7
    d = sr.make_scene_disp()
    w = sr.reference(d, F64)
    even = np.arange(sr.N_PIX) % 2 == 0
    assert np.abs(w["wsum"][even] / cr.DISP_TARGETS[0] - 1).max() <= 1e-3 and np.abs(w["wsum"][~even] / cr.DISP_TARGETS[1] - 1).max() <= 1e-3
    assert np.abs(w["person_acc"] / (0.5 * w["wsum"]) - 1).max() <= 1e-3, "the weight is split between the two people"
    assert np.all(w["disp_map"][~even] == 0) and np.all(w["disp_map"][even] > 0)


def test_an_opaque_front_sample_hides_the_person_behind():
    s = sr.make_scene(2, 33, "relu", "all", overlap=False)
    assert np.all(s["z"][0].max(-1)[s["rows"][0]] < s["z"][1].min(-1)[s["rows"][1]]), "person 1 stands behind person 0"
    visible = sr.reference(s, F64)["person_acc"][1]
    assert visible.max() > 0.05
    s["raw"][0][:, 0, 3] = 1e4 * cr.DENSITY_SCALE
    got = sr.reference(s, F64)
    assert got["person_acc"][1].max() <= 1e-9
    assert np.abs(got["person_acc"][0] - 1.0).max() <= 1e-9 and np.abs(got["acc_map"] - 1.0).max() <= 1e-9


def test_place_people_keeps_bone_coordinates():
    place_people = scene.place_people
    _, kps, skts = syn.make_pose(3, 5)
    off = np.array([[0.5, 0.0, -0.25], [-1.0, 0.125, 2.0], [0.0, 0.0, 0.0]], dtype=np.float32)
    kp2, sk2 = place_people(kps.astype(np.float64), skts.astype(np.float64), off)
    assert kp2.shape == kps.shape and sk2.shape == skts.shape
    assert np.array_equal(kp2, kps.astype(np.float64) + off[:, None].astype(np.float64))
    hom = lambda k: np.concatenate([k, np.ones_like(k[..., :1])], -1)
    # every joint seen from every bone: skt'_b [kp'_j ; 1] = skt_b [kp_j ; 1]
    before = np.einsum("pbrc,pjc->pbjr", skts.astype(np.float64), hom(kps.astype(np.float64)))
    after = np.einsum("pbrc,pjc->pbjr", sk2, hom(kp2))
    assert np.abs(after - before).max() <= 1e-12
    kt, st = place_people(torch.tensor(kps), torch.tensor(skts), torch.tensor(off))
    assert torch.is_tensor(kt) and kt.dtype == torch.float32 and st.dtype == torch.float32 and tuple(st.shape) == skts.shape
    with pytest.raises(ValueError):
        place_people(kps, skts, off[:2])


def test_header_binding_and_library_export_both_entry_points():
    import posegen_amd
    hdr = open(os.path.join(REPO, "include", "posegen_hip.h")).read()
    assert re.search(r"\bint pg_render_scene\(pg_handle\* h, void\* stream, int H, int W,", hdr)
    assert re.search(r"\bint pg_stage_scene_composite\(pg_handle\* h, void\* stream, int64_t n_pix, int n_people,", hdr)
    assert re.search(r"#define\s+PG_SCENE_MAX_PEOPLE\s+8\b", hdr) and _ffi.PG_SCENE_MAX_PEOPLE == 8
    assert re.search(r"typedef struct pg_scene_person \{\s*int32_t subject;[^}]*int32_t box\[4\];[^}]*const float\* skts;[^}]*"
                     r"const float\* cyl;[^}]*float cam;[^}]*\} pg_scene_person;", hdr)
    assert re.search(r"#define\s+PG_ABI_VERSION\s+11\b", hdr) and _ffi.PG_ABI_VERSION == 11      # entry points are added, none moves
    assert [f[0] for f in _ffi.PgScenePerson._fields_] == ["subject", "box", "skts", "cyl", "cam"] and C.sizeof(_ffi.PgScenePerson) == 48
    assert len(_ffi.PROTOTYPES["pg_render_scene"][1]) == 21 and len(_ffi.PROTOTYPES["pg_stage_scene_composite"][1]) == 14
    lib = _ffi.load_library()
    assert hasattr(lib, "pg_render_scene") and hasattr(lib, "pg_stage_scene_composite") and lib.pg_abi_version() == 11
    for name in ("render_scene", "render_scenes", "place_people", "ScenePerson"):
        assert getattr(posegen_amd, name) is getattr(scene, name)
    # a null handle is PG_EINVAL before anything else is looked at
    assert lib.pg_render_scene(None, None, 8, 8, None, None, 0.0, 1.0, 1, None, 32, 0, 0, None, 0.0, None, None, None, None, None, None) == _ffi.PG_EINVAL
    assert lib.pg_stage_scene_composite(None, None, 0, 1, 2, None, None, None, None, None, None, None, None, None) == _ffi.PG_EINVAL


class _Untouchable:
    """stands where the library and the handle stand: any use is a failure"""
    def __getattr__(self, name):
        raise AssertionError(f"the library was touched ({name})")


def _fake_caster(n_devices=1, training=False):
    r = types.SimpleNamespace(n_devices=n_devices, lib=_Untouchable(), handle=_Untouchable(), device=torch.device("cpu"))
    return types.SimpleNamespace(renderer=r, training=training)


def test_scenes_refuse_several_devices_and_training_mode_before_any_library_call():
    ScenePerson, render_scene, render_scenes = scene.ScenePerson, scene.render_scene, scene.render_scenes
    person = ScenePerson(torch.zeros(24, 4, 4), torch.zeros(5), ((0, 0), (4, 4)))
    kp, skts = torch.zeros(1, 1, 24, 3), torch.zeros(1, 1, 24, 4, 4)
    for caster, word in ((_fake_caster(n_devices=2), "several devices"), (_fake_caster(training=True), "training mode")):
        with pytest.raises(NotImplementedError, match=word):
            render_scene(caster, 8, 8, 10.0, np.eye(4), [person])
        with pytest.raises(NotImplementedError, match=word):
            render_scene(caster.renderer if word == "several devices" else caster, 8, 8, 10.0, np.eye(4), [person])
        with pytest.raises(NotImplementedError, match=word):
            render_scenes(np.eye(4)[None], (8, 8, 10.0), 64, {"ray_caster": caster}, kp=kp, skts=skts)
