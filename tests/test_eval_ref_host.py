"""CPU pins of the float64 restatement of the embed + MLP stage (tests/eval_ref.py), and the conditions on the edge cases of
tests/eval_cases.py: each is built as its docstring says, is well conditioned, and moves raw under every deliberate error it is
there to catch by more than the bound tests/test_gpu_eval_points.py holds a kernel to."""
import numpy as np
import pytest
import torch

from oracle import anerf_oracle as orc
from tests import eval_cases as ec
from tests import eval_ref as er
from tests.helpers import cfg_from_golden, default_dtype, load_golden, model_for, oracle_cfg, torch_weights, weights_digest

# the bound tests/test_oracle_golden.py holds the oracle's raw to against the reference's own vectors
RAW_TOL = {"coarse": dict(rtol=1e-4, atol=2e-4), "fine": dict(rtol=1e-3, atol=2e-3)}


def _golden_stage(name):
    g = load_golden(name)
    cfg = cfg_from_golden(g)
    wc, wf, _, _ = model_for(cfg, int(g["seed_model"]))
    assert weights_digest(wc) == str(g["digest_coarse"])
    return g, cfg, wc, wf


@pytest.mark.parametrize("name", ["rays_surreal", "rays_h36m"])
def test_restatement_matches_the_oracle_in_float64_and_the_reference_vectors(name):
    """Uniform cutoffs: orc.embed_points + orc.mlp_forward run in float64 agree with the restatement to 1e-12 relative, and the
    restatement cast to fp32 matches raw_coarse / raw_fine of the fixture -- the reference's own vectors -- at the oracle's bound."""
    g, cfg, wc, wf = _golden_stage(name)
    rb, skts = g["ray_batch"], g["skts"]
    cams = g["cams"] if "cams" in g else None
    cut = np.full(24, cfg.cutoff_dist)
    for tag, w, z in (("coarse", wc, g["z_coarse"]), ("fine", wf, g["z_fine"])):
        n, S = z.shape
        ref = er.eval_rays(w, rb, z, skts, cut, cut, g["tau_v"], g["tau_d"], cams=cams)["raw"]
        with default_dtype(torch.float64):
            c64 = lambda a: torch.tensor(np.asarray(a), dtype=torch.float64)
            o, d = c64(rb[:, 0:3]), c64(rb[:, 3:6])
            x = orc.embed_points(o[:, None, :] + d[:, None, :] * c64(z)[..., None], d, c64(skts), oracle_cfg(cfg, g["tau_v"], g["tau_d"]),
                                 None if cams is None else c64(cams))
            w64 = {k: c64(v) for k, v in w.items()}
            o64 = orc.mlp_forward(x.reshape(n * S, -1), w64, oracle_cfg(cfg, g["tau_v"], g["tau_d"])).reshape(n, S, 4)
        rel = float((ref - o64).abs().max() / o64.abs().max())
        print(f"[{name} {tag}] restatement vs float64 oracle: {rel:.2e} relative")
        assert rel <= 1e-12
        np.testing.assert_allclose(ref.float().numpy(), g[f"raw_{tag}"], **RAW_TOL[tag])


def test_restatement_matches_the_reference_with_per_joint_cutoffs():
    """eval_edges.npz: the reference's own embedders and nets with non-uniform cutoff_dist, different for embed_fn and
    embeddirs_fn, and tau_v != tau_d.  The restatement and the oracle's array-valued cutoffs both match it; exchanging the two
    cutoff vectors, or reading them in another joint order, does not."""
    g, cfg, wc, wf = _golden_stage("eval_edges")
    assert np.ptp(g["cutoff_v"]) > 0.2 and np.abs(g["cutoff_v"] - g["cutoff_d"]).max() > 0.2 and float(g["tau_v"]) != float(g["tau_d"])
    assert g["raw_coarse"].size // 4 <= 600
    args = (g["ray_batch"], g["z"], g["skts"], g["cutoff_v"], g["cutoff_d"], float(g["tau_v"]), float(g["tau_d"]))
    n, S = g["z"].shape
    ocfg = oracle_cfg(cfg, g["tau_v"], g["tau_d"])
    ocfg.cutoff_v, ocfg.cutoff_d = g["cutoff_v"], g["cutoff_d"]
    rb = torch.tensor(g["ray_batch"])
    x = orc.embed_points(rb[:, None, 0:3] + rb[:, None, 3:6] * torch.tensor(g["z"])[..., None], rb[:, 3:6], torch.tensor(g["skts"]), ocfg)
    for tag, w in (("coarse", wc), ("fine", wf)):
        ref = er.eval_rays(w, *args)["raw"].float().numpy()
        np.testing.assert_allclose(ref, g[f"raw_{tag}"], **RAW_TOL["coarse"])
        o32 = orc.mlp_forward(x.reshape(n * S, -1), torch_weights(w), ocfg).reshape(n, S, 4).numpy()
        np.testing.assert_allclose(o32, g[f"raw_{tag}"], **RAW_TOL["coarse"])
        for mut in ("cutoff_swapped", "cutoff_slot_order"):
            bad = er.eval_rays(w, *args, mut=mut)["raw"].float().numpy()
            assert np.abs(bad - g[f"raw_{tag}"]).max() > 0.1, (tag, mut)


def test_oracle_array_cutoff_of_equal_values_is_bitwise_the_scalar():
    """the array-valued cutoff of the oracle: an array of equal values gives bitwise the scalar's embedding (the scalar path
    itself is untouched: tests/test_oracle_golden.py pins it to the reference)"""
    g, cfg, wc, wf = _golden_stage("rays_surreal")
    rb = torch.tensor(g["ray_batch"][:16])
    pts = rb[:, None, 0:3] + rb[:, None, 3:6] * torch.tensor(g["z_coarse"][:16])[..., None]
    ocfg = oracle_cfg(cfg, g["tau_v"], g["tau_d"])
    a = orc.embed_points(pts, rb[:, 3:6], torch.tensor(g["skts"]), ocfg)
    ocfg.cutoff_v = ocfg.cutoff_d = np.full(24, cfg.cutoff_dist, np.float32)
    b = orc.embed_points(pts, rb[:, 3:6], torch.tensor(g["skts"]), ocfg)
    assert torch.equal(a, b)


# ---------------------------------------------------------------------------------------------- the cases as built
def test_seams_shapes():
    for n in ec.SEAM_N:
        for S in ec.SEAM_S:
            c = ec.seams(n, S)
            assert c.z.shape == (n, S) and c.n_points % 128 != 0 and c.skts.shape[0] == n and len(np.unique(c.cams)) == n
            assert (np.diff(c.z, axis=1) > 0).all()
            pid = c.note["pose_of_ray"]
            assert len(set(pid)) == 3 and all(pid[i] == pid[i + 1] for i in range(0, n - 1, 2))
    # 13 x 65: four 256-point passes (the last ragged), and a pass whose points belong to 5 rays
    big = ec.seams(13, 65)
    ray_of_point = np.repeat(np.arange(13), 65)
    per_pass = [len(set(ray_of_point[p:p + 256])) for p in range(0, big.n_points, 256)]
    assert len(per_pass) >= 3 and max(per_pass) == 5 and big.n_points % 256 != 0


def test_cutoffs_case_spans_every_radius_and_sits_on_the_threshold():
    seen = set()
    for tv, td in ec.CUTOFF_TAUS:
        c = ec.cutoffs(tv, td)
        assert tv != td and np.abs(c.cutoff_v - c.cutoff_d).max() > 0.1
        assert c.cutoff_v.min() >= 0.3 and c.cutoff_v.max() <= 0.7 and c.cutoff_d.min() >= 0.3 and c.cutoff_d.max() <= 0.7
        seen |= {tv, td}
        dist = ec.min_joint_distance(c)                  # [n,S,24]
        rad = c.far_radius()
        if "threshold_rays" in c.note:
            inside = (dist < rad).reshape(-1, 24)
            assert inside.any(0).all() and (~inside).any(0).all(), "every joint has points inside and outside its far-skip radius"
            lo, hi = c.note["threshold_rays"]
            m_lo, m_hi = dist[lo, :, 21].min() / rad[21], dist[hi, :, 21].min() / rad[21]
            print(f"[{c.name}] closest approach / radius of joint 21: {m_lo - 1:+.2e}, {m_hi - 1:+.2e}")
            assert 1 - 2.0 ** -17 < m_lo < 1 - 2.0 ** -19 and 1 + 2.0 ** -19 < m_hi < 1 + 2.0 ** -17
    assert {4.0, ec.TAU_MODEL, 400.0} <= seen and any("threshold_rays" in ec.cutoffs(*t).note for t in ec.CUTOFF_TAUS)


@pytest.mark.parametrize("S", [32, 64])
def test_on_joint_is_exactly_zero_in_fp32_and_well_conditioned(S):
    c = ec.on_joint(S)
    r, k, j = c.note["ray"], c.note["sample"], c.note["joint"]
    o, d, z = c.ray_batch[r, 0:3], c.ray_batch[r, 3:6], c.z[r]
    R, t = c.skts[0, j, :3, :3], c.skts[0, j, :3, 3]
    f32 = np.float32
    a, b = (R @ o + t).astype(f32), (R @ d).astype(f32)
    assert np.all((a + z[k] * b).astype(f32) == 0) and np.all((R @ (o + z[k] * d).astype(f32) + t).astype(f32) == 0)
    dist = ec.min_joint_distance(c)[r, :, j] / np.linalg.norm(d.astype(np.float64))
    near = np.sort(dist)[:15]
    want = np.sort(np.concatenate([[0.0], np.repeat(2.0 ** -np.arange(4, 11), 2)]))
    np.testing.assert_allclose(near, want, rtol=1e-6, atol=0)
    assert (np.diff(c.z, axis=1) > 0).all()
    # well conditioned: the fp32 oracle and the float64 restatement agree on the ray, at the oracle's own bound
    cfg, wc, wf = ec.model(c.model)
    rb = torch.tensor(c.ray_batch)
    ocfg = oracle_cfg(cfg, c.tau_v, c.tau_d)
    x = orc.embed_points(rb[:, None, 0:3] + rb[:, None, 3:6] * torch.tensor(c.z)[..., None], rb[:, 3:6], torch.tensor(c.skts), ocfg)
    for which, w in ((0, wc), (1, wf)):
        o32 = orc.mlp_forward(x.reshape(-1, x.shape[-1]), torch_weights(w), ocfg).reshape(*c.z.shape, 4).numpy()
        ref = c.reference(which)["raw"].numpy()
        err = np.abs(o32 - ref).max(-1)
        print(f"[{c.name} net {which}] fp32 oracle vs float64: {err.max():.2e} over the case, {err[r].max():.2e} on the joint's ray")
        np.testing.assert_allclose(o32[r], ref[r], **RAW_TOL["coarse"])
        np.testing.assert_allclose(o32, ref, **RAW_TOL["coarse"])


def test_all_far_rays_miss_every_radius_and_give_the_empty_space_output():
    for layout in ("all", "first", "last"):
        c = ec.all_far(layout)
        far = c.note["far_rays"]
        dist = ec.min_joint_distance(c).min(-1)          # [n,S]
        assert dist[far].min() > 2.0 and dist[~far].min() < 0.3 if (~far).any() else dist.min() > 2.0
        assert c.far_radius().max() < 1.0
        p0 = np.repeat(far, c.S)                          # per point
        if layout == "first":
            assert p0[:256].all() and not p0[256:].any() and c.n_points > 512
        if layout == "last":
            assert not p0[:256].any() and p0[256:].all() and 0 < c.n_points - 256 < 256
        # empty space: every cutoff weight is 0, the density input is the 72 directions alone
        raw = c.reference(0)["raw"].numpy()
        cfg, wc, _ = ec.model(c.model)
        sig = raw[far][..., 3]
        assert sig.max() < 0, "the synthetic model's empty space has negative density"
        rb64, z64 = c.ray_batch[far].astype(np.float64), c.z[far].astype(np.float64)
        q = er.bone_local(rb64[:, None, 0:3] + rb64[:, None, 3:6] * z64[..., None], c.skts)
        x_in = torch.cat([torch.zeros(*q.shape[:2], cfg.ch_v, dtype=torch.float64), er._unit(q).flatten(start_dim=-2)], -1)
        empty, _ = er.mlp(x_in.reshape(-1, x_in.shape[-1]), torch.zeros(x_in.shape[0] * x_in.shape[1], cfg.ch_d, dtype=torch.float64), None, wc)
        assert np.abs(empty.numpy().reshape(*sig.shape, 4) - raw[far]).max() < 1e-9


def test_codes_ties_and_points_as_described():
    last = ec.config_of("h36m").n_framecodes - 1
    assert set(ec.codes(False).cams) == {-1.0, 0.0, float(last)} and ec.codes(True).cams.shape == (1,)
    a, b = ec.codes(False).reference(1)["raw"], ec.codes(True).reference(1)["raw"]
    same = torch.tensor(ec.codes(False).cams == last)
    assert torch.equal(a[same], b[same]) and (a[~same] - b[~same]).abs().max() > 1e-2
    t = ec.ties()
    assert (t.z[3] == t.z[3, 0]).all() and ((np.diff(t.z, axis=1) == 0).sum(1) >= 10).all()
    for count in (1, 129, 257):
        p = ec.points(count)
        dist = ec.min_joint_distance(p)[:, 0, :]
        assert p.pts.shape == (count, 3) and dist[0, 17] == 0.0
        if count > 1:
            rad = p.far_radius()[21]
            assert 1 - 2.0 ** -17 < dist[1, 21] / rad < 1 - 2.0 ** -19 and 1 + 2.0 ** -19 < dist[2, 21] / rad < 1 + 2.0 ** -17
            assert dist[3].min() > 3.0


# ---------------------------------------------------------------------------------------------- every error shows
def _mutation_cases():
    seam, codes = ec.seams(13, 65), ec.codes(False)
    cut = [ec.cutoffs(*t) for t in ec.CUTOFF_TAUS]
    return ([("neighbour_pose", seam), ("neighbour_code", seam), ("neighbour_code", codes), ("z_shifted", seam), ("z_shifted", ec.ties()),
             ("top_octave_sign", seam), ("top_octave_sign", ec.on_joint(64)), ("limb_dropped", seam)]
            + [(m, c) for c in cut for m in ("cutoff_slot_order", "cutoff_swapped", "limb_dropped", "top_octave_sign")])


@pytest.mark.parametrize("mut,case", _mutation_cases(), ids=lambda v: v if isinstance(v, str) else v.name)
def test_every_deliberate_error_moves_raw_by_more_than_the_bounds(mut, case):
    """A condition on the INPUTS (seeds, weight scale): each error moves raw at one point or more by more than the fp16 bound of
    the GPU test -- the loosest bound among the precisions that have to catch it: the exact modes' bounds (fp32 4e-5, bf16x3 3e-4,
    fp16c 9e-4, times max(1, |raw|max / 10)) are all below it, and every form runs in fp16 or in an exact mode."""
    for which in (0, 1):
        ref = ec.reference(case, which)["raw"]
        bad = case.reference(which, mut=mut)["raw"]
        y = ec.yardstick(case, which, "fp16")
        b16 = ec.bound_16bit("fp16", y)
        move = float((bad - ref).abs().max())
        print(f"[{case.name} net {which}] {mut}: raw moves by {move:.3e}; fp16 bound {b16:.3e} (|raw| max {y['scale']:.1f})")
        assert move > b16 and b16 > max(ec.bound_exact(p, y["scale"]) for p in ec.EXACT_TOL)
