"""The float64 restatement of the SMPL body (tests/smpl_ref.py) against the reference's own float32 `lbs` (tests/golden/smpl_body.npz,
tools/gen_golden_smpl.py), the meaning of the bounds, and the Python layer of posegen_amd.smpl without a GPU.

Bounds (derived, not tuned; u = 2^-24, `mag` = the restatement's sum of absolute products behind an element): a float32 evaluation
of a sum of n products in any order is within n u mag to first order.  Vertices: n = (1 + NB + 207) + 24 + 4 + 8.  Regressed
joints: that n plus ceil(V / 4) -- the device adds 4 vertices in float32 per MFMA and everything above in double; the reference's
float32 einsum is held to n + V.  Posed joints, key points: one float32 ulp of the rounded value + 9 u mag.

Largest observed error / bound.  Host, the reference's float32 values against the restatement: vertices 0.016, posed joints 0.054
(their bound widened by the reference's float32 rest joints and chain, (V + 36) u mag), regressed 0.0035.  Device
(tests/test_gpu_smpl.py, MI355X): vertices 0.050, posed joints 0.089, regressed 0.012, key points 0.087.  Least movement of an
ablation: 103.7 bounds (a column of the 9-row regressor).  Nothing is set from these."""
import os
import re
import types

import numpy as np
import pytest
import torch

from posegen_amd import _ffi, smpl, synthetic
from tests import smpl_ref as ref

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = np.load(os.path.join(REPO, "tests", "golden", "smpl_body.npz"))
V, NB = int(GOLD["V"]), int(GOLD["NB"])
ROWS = tuple(int(k) for k in GOLD["regress_rows"])


@pytest.fixture(scope="module")
def model():
    return synthetic.make_body_model(V, NB=NB, seed=int(GOLD["seed"]), regress_rows=ROWS)


def restated(model, form, m=None):
    """the restatement of the fixture's poses in one of its two forms, both regressors: {K: lbs dict}"""
    m = model if m is None else m
    pose, p2r = (GOLD["pose"], True) if form == "axis" else (GOLD["rotmat"], False)
    return {K: ref.lbs(m, GOLD["betas"], pose, pose2rot=p2r, regress=m[f"regressor_{K}"]) for K in ROWS}


def ratio(got, want, bound):
    return float(np.max(np.abs(ref.f64(got) - want) / bound))


@pytest.mark.parametrize("form", ["axis", "rotmat"])
def test_restatement_matches_the_reference_lbs(model, form):
    sfx = "" if form == "axis" else "_rotmat"
    out = restated(model, form)
    o = out[ROWS[0]]
    r_v = ratio(GOLD["verts" + sfx], o["verts"], ref.bound_verts(o, NB))
    # the reference's rest joints are a float32 sum of V products and its chain float32 products of depth <= 9 with 4 terms each
    r_j = ratio(GOLD["joints" + sfx], o["joints"], ref.bound_chain(o["joints"], o["mag_joints"]) + (V + 36) * ref.U * o["mag_joints"])
    r_k = max(ratio(GOLD[f"regressed_{K}{sfx}"], out[K]["regressed"],
                    (ref.n_vertex_products(NB) + V) * ref.U * out[K]["mag_regressed"]) for K in ROWS)
    print(f"{form}: error / bound: verts {r_v:.4f}, joints {r_j:.4f}, regressed {r_k:.4f}")
    assert r_v <= 1 and r_j <= 1 and r_k <= 1
    if form == "axis":          # the two forms of the fixture are the same poses (a dozen float32 roundings of numbers up to 2)
        assert np.abs(ref.rodrigues(GOLD["pose"].reshape(-1, 3)).reshape(-1, 24, 3, 3) - GOLD["rotmat"]).max() < 16 * ref.U


def test_rest_pose_is_the_shaped_template(model):
    assert not GOLD["pose"][0].any()
    o = ref.lbs(model, GOLD["betas"][:1], GOLD["pose"][:1])
    shaped = ref.f64(model["v_template"]) + np.einsum("l,mkl->mk", ref.f64(GOLD["betas"][0]), ref.f64(model["shapedirs"]))
    assert np.abs(o["v_posed"][0] - shaped).max() == 0
    # the skin rows are float32 numbers that sum to 1 within rounding, not exactly: verts = (sum_j w_j) v_shaped
    rowsum = ref.f64(model["lbs_weights"]).sum(1, keepdims=True)
    assert np.abs(o["verts"][0] - rowsum * shaped).max() < 1e-14
    assert np.abs(o["verts"][0] - shaped).max() < 4 * ref.U * np.abs(shaped).max()
    assert np.abs(o["joints"][0] - ref.f64(model["J_regressor"]) @ shaped).max() < 1e-14


def _moved(base, abl):
    """the largest |change| / bound over the vertices and both regressors"""
    worst = 0.0
    for K in ROWS:
        b, a = base[K], abl[K]
        worst = max(worst, ratio(a["verts"], b["verts"], ref.bound_verts(b, NB)),
                    ratio(a["regressed"], b["regressed"], ref.bound_regressed(b, NB, V)))
    return worst


def test_the_bounds_are_tight_against_mistakes(model):
    """leaving out any single blend row, skin weight column or regressor column, or shifting a vertex index by one, moves some
    output by at least 100 times its bound"""
    base = restated(model, "axis")
    least = {}

    def ablate(kind, **changed):
        m = dict(model)
        m.update(changed)
        moved = _moved(base, restated(model, "axis", m))
        least[kind] = min(least.get(kind, np.inf), moved)

    z = lambda a, idx: (lambda c: (c.__setitem__(idx, 0), c)[1])(a.copy())
    ablate("template row", v_template=np.zeros_like(model["v_template"]))
    for l in range(NB):
        ablate("shape row", shapedirs=z(model["shapedirs"], (slice(None), slice(None), l)))
    for r in range(207):
        ablate("pose row", posedirs=z(model["posedirs"], r))
    for j in range(24):
        ablate("skin column", lbs_weights=z(model["lbs_weights"], (slice(None), j)))
    for K in ROWS:                      # a regressor column: the change is that column's own products
        b = base[K]
        delta = np.abs(ref.f64(model[f"regressor_{K}"])[None, :, :, None] * b["verts"][:, None, :, :])          # [B,K,V,3]
        moved = (delta / ref.bound_regressed(b, NB, V)[:, :, None, :]).max(axis=(0, 1, 3))                      # per column
        least[f"regressor_{K} column"] = float(moved.min())
    ablate("skin rows shifted by one vertex", lbs_weights=np.roll(model["lbs_weights"], 1, axis=0))
    ablate("blend columns shifted by one vertex", posedirs=np.roll(model["posedirs"], 3, axis=1),
           shapedirs=np.roll(model["shapedirs"], 1, axis=0), v_template=np.roll(model["v_template"], 1, axis=0))
    ablate("regressor columns shifted by one vertex", **{f"regressor_{K}": np.roll(model[f"regressor_{K}"], 1, axis=1) for K in ROWS})
    print({k: round(v, 1) for k, v in least.items()})
    assert min(least.values()) >= 100, least


def test_rotation_chain_reproduces_the_kinematics_fixture():
    """rotation matrices formed in float64 from the fixture's bones and rounded to float32 give its key points: the float32
    inputs' own rounding through a chain of depth <= 9"""
    g = np.load(os.path.join(REPO, "tests", "golden", "kinematics.npz"))
    rot = ref.axisang_to_rot(g["bones"])
    l2ws, kps, mag = ref.rot_chain(rot, g["rest_pose"])
    r = ratio(kps, g["kps"], ref.bound_chain(g["kps"], mag))
    print(f"key points: error / bound {r:.4f}")
    assert r <= 1
    assert np.abs(l2ws[:, :, :3, :3] - g["l2ws"][:, :, :3, :3]).max() < 40 * ref.U


def test_layout_helper_against_the_restatement(model):
    blend, rest = smpl.pack_model(model["v_template"], model["shapedirs"], model["posedirs"], model["J_regressor"])
    assert blend.dtype == np.float32 and blend.shape == (1 + NB + 207, 3 * V) and rest.dtype == np.float64 and rest.shape == (1 + NB, 24, 3)
    o = ref.lbs(model, GOLD["betas"], GOLD["pose"])
    feat = np.concatenate([np.ones((len(GOLD["betas"]), 1)), ref.f64(GOLD["betas"]), (o["rot"][:, 1:] - np.eye(3)).reshape(-1, 207)], 1)
    assert np.abs((feat @ ref.f64(blend)).reshape(-1, V, 3) - o["v_posed"]).max() < 1e-13
    J = np.einsum("bl,ljc->bjc", feat[:, :1 + NB], rest)
    assert np.abs(J - np.einsum("jv,bvc->bjc", ref.f64(model["J_regressor"]), o["v_shaped"])).max() < 1e-13
    assert np.array_equal(blend[0], model["v_template"].reshape(-1)) and np.array_equal(blend[1 + NB:], model["posedirs"])
    assert np.array_equal(blend[3].reshape(V, 3), model["shapedirs"][:, :, 2])


# ---- the Python layer without a GPU ------------------------------------------------------------------------------------------------------
def _fake_renderer(device="cuda:0"):
    return types.SimpleNamespace(device=device, lib=None, handle=None)


def _args(model, **changed):
    m = dict(model)
    m.update(changed)
    return [m[k] for k in smpl.MODEL_KEYS]


def test_there_is_no_cpu_path(model):
    with pytest.raises(NotImplementedError, match="no CPU path"):
        smpl.BodyModel(_fake_renderer("cpu"), *_args(model))
    with pytest.raises(NotImplementedError, match="no CPU path"):
        smpl.vertex_errors(_fake_renderer("cpu"), np.zeros((1, 2, 3)), np.zeros((1, 2, 3)))


def test_model_refusals_come_before_the_library(model):
    r = _fake_renderer()
    bad = lambda **c: smpl.pack_model(*_args(model, **c)[:4])
    with pytest.raises(ValueError, match="shape coefficients"):
        bad(shapedirs=np.zeros((V, 3, 0), np.float32))
    with pytest.raises(ValueError, match="shape coefficients"):
        bad(shapedirs=np.zeros((V, 3, 17), np.float32))
    with pytest.raises(ValueError, match="shapedirs"):
        bad(shapedirs=np.zeros((V + 1, 3, NB), np.float32))
    with pytest.raises(ValueError, match="posedirs"):
        bad(posedirs=np.zeros((207, 3 * V + 3), np.float32))
    with pytest.raises(ValueError, match="posedirs"):
        bad(posedirs=np.zeros((459, 3 * V), np.float32))                      # SMPL-X's pose rows
    with pytest.raises(ValueError, match="J_regressor"):
        bad(J_regressor=np.zeros((55, V), np.float32))
    with pytest.raises(ValueError, match="v_template"):
        bad(v_template=np.zeros((V, 2), np.float32))
    with pytest.raises(TypeError, match="integers"):
        smpl.check_parents(np.arange(24, dtype=np.float32) - 1)
    with pytest.raises(ValueError, match="after its parent"):
        smpl.check_parents(np.array([-1, 0, 3] + list(range(2, 23)), dtype=np.int64))
    with pytest.raises(ValueError, match=r"\[24\]"):
        smpl.check_parents(np.arange(55) - 1)
    assert smpl.check_parents(np.array([2 ** 32 - 1] + list(range(23)), dtype=np.int64))[0] == -1     # smplx's wrapped root
    # the checks above run in the constructor before a tensor is made; a fake renderer gets as far as torch's device
    for changed, match in ((dict(lbs_weights=np.zeros((V, 23), np.float32)), "lbs_weights"),):
        with pytest.raises(ValueError, match=match):
            smpl.BodyModel(r, *_args(model, **changed))
    with pytest.raises(ValueError, match="K in 1..64"):
        smpl.BodyModel(r, *_args(model), regressors={"big": np.zeros((65, V), np.float32)})
    with pytest.raises(ValueError, match="K in 1..64"):
        smpl.BodyModel(r, *_args(model), regressors={"other": np.zeros((17, V + 1), np.float32)})
    with pytest.raises(KeyError, match="lbs_weights"):
        smpl.BodyModel.from_arrays(r, {k: v for k, v in model.items() if k != "lbs_weights"})


def test_forward_refusals_come_before_the_library():
    body = object.__new__(smpl.BodyModel)                         # (a body that cannot launch anything: no renderer, no arrays)
    body.device, body.V, body.NB, body.regressors, body.renderer = torch.device("cuda:0"), 7, 10, {"h36m": None}, _fake_renderer()
    betas, pose = np.zeros((2, 10), np.float32), np.zeros((2, 24, 3), np.float32)
    with pytest.raises(ValueError, match="betas"):
        body.forward(np.zeros((2, 9), np.float32), pose)
    with pytest.raises(ValueError, match="rows of betas"):
        body.forward(np.zeros((3, 10), np.float32), pose)
    with pytest.raises(ValueError, match="axis-angle"):
        body.forward(betas, np.zeros((2, 23, 3), np.float32))
    with pytest.raises(ValueError, match="rotation matrices"):
        body.forward(betas, pose, pose2rot=False)
    with pytest.raises(ValueError, match="axis-angle"):
        body.forward(betas, np.zeros((2, 24, 3, 3), np.float32))
    with pytest.raises(ValueError, match="no poses"):
        body.forward(betas[:0], pose[:0])
    with pytest.raises(KeyError, match="no regressor"):
        body.forward(betas, pose, regressor="extra")
    with pytest.raises(ValueError, match="no output"):
        body.forward(betas, pose, joints=False)
    with pytest.raises(NotImplementedError, match="transl"):
        body.forward(betas, pose, transl=np.zeros((2, 3)))
    with pytest.raises(TypeError, match="floating point"):
        body.forward(betas, np.zeros((2, 24, 3), np.int32))
    with pytest.raises(NotImplementedError, match="gradients"):
        body.forward(torch.zeros(2, 10, requires_grad=True), pose)
    with pytest.raises(ValueError, match="global_orient and body_pose"):
        body.forward(betas, global_orient=pose[:, :1])
    with pytest.raises(ValueError, match=r"\[B,V,3\]"):
        smpl.vertex_errors(_fake_renderer(), np.zeros((2, 5, 3)), np.zeros((2, 4, 3)))
    from posegen_amd.raycaster import HipRenderer
    kin = types.SimpleNamespace(device="cuda:0")
    with pytest.raises(ValueError, match=r"\[F,24,3,3\]"):
        HipRenderer.pose_kinematics_rot(kin, np.zeros((2, 24, 3)), np.zeros((24, 3)))
    with pytest.raises(ValueError, match="after its parent"):
        HipRenderer.pose_kinematics_rot(kin, np.zeros((2, 24, 3, 3)), np.zeros((24, 3)), parents=[0, 0, 5] + list(range(2, 23)))
    with pytest.raises(ValueError, match="24 integers"):
        HipRenderer.pose_kinematics_rot(kin, np.zeros((2, 24, 3, 3)), np.zeros((24, 3)), parents=np.zeros(24))


def test_header_binding_and_package_export_the_entry_points():
    import posegen_amd
    from posegen_amd import pose_eval
    hdr = open(os.path.join(REPO, "include", "posegen_hip.h")).read()
    flat = re.sub(r"\s+", " ", hdr)
    assert ("int pg_smpl_forward(pg_handle* h, void* stream, const pg_body_model* m, int64_t B, const float* betas, int64_t betas_stride, "
            "const float* pose, int pose_is_rotmat, const float* regress, int K, float* verts, float* joints, float* regressed);") in flat
    assert "int pg_vertex_errors(pg_handle* h, void* stream, int64_t B, int V, const float* a, const float* b, double* per_pose, double* summary);" in flat
    assert ("int pg_pose_kinematics_rot(pg_handle* h, void* stream, int64_t n_poses, const float* rotmats, const double* bone_offsets, "
            "const int32_t* parents, float* kps, float* skts, double* l2ws);") in flat
    assert re.search(r"typedef struct pg_body_model \{ int32_t V, NB;.*const float\* blend;.*const float\* skin;.*const double\* rest_joints;"
                     r".*int32_t parents\[24\];.*\} pg_body_model;", flat)
    assert re.search(r"#define\s+PG_ABI_VERSION\s+11\b", hdr) and _ffi.PG_ABI_VERSION == 11      # added entry points do not move it
    assert [len(_ffi.PROTOTYPES[n][1]) for n in ("pg_smpl_forward", "pg_vertex_errors", "pg_pose_kinematics_rot")] == [13, 8, 9]
    assert [f[0] for f in _ffi.PgBodyModel._fields_] == ["V", "NB", "blend", "skin", "rest_joints", "parents"]
    lib = _ffi.load_library()
    assert lib.pg_abi_version() == 11
    # a null handle is PG_EINVAL before anything looks for a device
    assert lib.pg_smpl_forward(None, None, None, 1, None, 0, None, 0, None, 0, None, None, None) == _ffi.PG_EINVAL
    assert lib.pg_vertex_errors(None, None, 1, 1, None, None, None, None) == _ffi.PG_EINVAL
    assert lib.pg_pose_kinematics_rot(None, None, 1, None, None, None, None, None, None) == _ffi.PG_EINVAL
    assert posegen_amd.BodyModel is smpl.BodyModel and posegen_amd.vertex_errors is smpl.vertex_errors
    assert posegen_amd.evaluate_smpl_predictions is pose_eval.evaluate_smpl_predictions
    assert tuple(ref.H36M_TO_J14) == pose_eval.H36M_TO_J14 and tuple(ref.SPIN_TO_CANON) == pose_eval.SPIN_TO_CANON
    rot = smpl.bones_to_rotmats(torch.from_numpy(GOLD["pose"])).numpy()
    assert np.abs(rot.astype(np.float64) - ref.axisang_to_rot(GOLD["pose"])).max() <= 2 * ref.U
