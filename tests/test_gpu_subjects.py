"""The subject bank on the GPU: one caster holding several A-NeRF models renders each frame (ray call, density query)
with the model it names, bitwise as a caster that holds that model alone would -- same kernels, same packed images, same
launch shapes, so the bar is equality, not a tolerance."""
import dataclasses

import numpy as np
import pytest
import torch

from oracle import anerf_oracle as orc
from posegen_amd import h36m_config, surreal_config, surreal_single_config, synthetic as syn
from posegen_amd.raycaster import HipRayCaster
from posegen_amd.render import render_path
from tests.helpers import cfg_from_golden, load_golden

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
SEEDS = (0, 1, 2)


def same(a, b):
    a, b = (x.detach().cpu().numpy() if torch.is_tensor(x) else np.asarray(x) for x in (a, b))
    return a.shape == b.shape and np.array_equal(a, b, equal_nan=True)


def same_maps(a, b):
    assert set(a) == set(b)
    return all(same(a[k], b[k]) for k in a)


@pytest.fixture(scope="module")
def casters():
    """one-subject casters and banks, made once per (config, seeds, devices) and closed at the end of the module"""
    made = {}

    def get(cfg, seeds, devices=None, models=None):
        key = (repr(cfg), tuple(seeds), None if devices is None else tuple(devices))
        if key not in made:
            ms = models if models is not None else [syn.make_model(cfg, s) for s in seeds]
            made[key] = (HipRayCaster.from_subjects(cfg, ms, device=DEV, precision="bf16", devices=devices) if len(ms) > 1
                         else HipRayCaster.from_weights(cfg, *ms[0], device=DEV, precision="bf16", devices=devices))
        return made[key]
    yield get
    for c in made.values():
        c.renderer.close()


def frame_rays(H, W, seed=1, n_rays=None):
    """the rays of one synthetic frame's box: (ray_batch [n,11], skts [1,24,4,4], cyls [1,5]) on the device"""
    _, kps, skts = syn.make_pose(1, seed)
    c2ws, focals = syn.make_camera(1, H, W)
    rays, _, cyls, _ = orc.valid_rays(torch.tensor(c2ws), H, W, focals, torch.tensor(kps), 0.001)
    ro, rd = rays[0]
    n = ro.shape[0]
    vd = rd / torch.norm(rd, dim=-1, keepdim=True)
    rb = torch.cat([ro, rd, torch.zeros(n, 1), torch.ones(n, 1), vd], -1)
    if n_rays is not None:
        assert n >= n_rays, n
        rb = rb[torch.linspace(0, n - 1, n_rays).long()]
    return rb.to(DEV), torch.tensor(skts).to(DEV), torch.as_tensor(cyls).float().to(DEV)


def path_inputs(F, H, W, seed=3):
    _, kps, skts = syn.make_pose(F, seed)
    c2ws, focals = syn.make_camera(F, H, W)
    return torch.tensor(c2ws), focals, dict(kp=torch.tensor(kps), skts=torch.tensor(skts), white_bkgd=True, ret_acc=True, ext_scale=0.001)


@pytest.mark.parametrize("prec", ["bf16", "fp16c"])
def test_bank_equals_separate_casters_bitwise(casters, prec):
    """Six 48 x 48 frames at 64 + 16 through render_path with subject_idxs = [0, 1, 2, 2, 0, 1] on a three-subject bank
    against three one-subject casters.  (Before the bank, render_path dropped subject_idxs: every frame was subject 0's.)"""
    cfg = surreal_config()
    subj = [0, 1, 2, 2, 0, 1]
    H = W = 48
    c2ws, focals, kw = path_inputs(len(subj), H, W)
    bank = casters(cfg, SEEDS)
    assert bank.n_subjects == 3
    bank.renderer.set_precision(prec)
    rk = lambda c: {"ray_caster": c, "N_samples": 64, "N_importance": 16}
    got = render_path(c2ws, (H, W, focals), 1024, rk(bank), subject_idxs=subj, **kw)
    assert bank.renderer.selected_subject == 0
    alone = []
    for s in SEEDS:
        c = casters(cfg, (s,))
        c.renderer.set_precision(prec)
        alone.append(render_path(c2ws, (H, W, focals), 1024, rk(c), **kw))
    for f, s in enumerate(subj):
        for k in range(3):                                    # rgbs, disps, accs
            assert same(got[k][f], alone[s][k][f]), (f, s, k)
    assert same(np.array(got[4]), np.array(alone[0][4]))      # the boxes
    # the test can see a wrong selection: the subjects' frames differ
    for a in range(3):
        for b in range(a + 1, 3):
            assert np.abs(alone[a][0][0] - alone[b][0][0]).max() > 1e-2, (a, b)
    # [n_pose] subjects are indexed i % n_pose, a scalar names one subject for all frames
    two = render_path(c2ws, (H, W, focals), 1024, rk(bank), subject_idxs=[1, 2], **kw)
    for f in range(len(subj)):
        assert same(two[0][f], alone[1 + f % 2][0][f])
    one = render_path(c2ws[:2], (H, W, focals[:2]), 1024, rk(bank), subject_idxs=2,
                      **dict(kw, kp=kw["kp"][:2], skts=kw["skts"][:2]))
    assert same(one[0], alone[2][0][:2])


def _h36m_models():
    cfg = h36m_config()
    return cfg, [syn.make_model(cfg, 0), syn.make_model(dataclasses.replace(cfg, n_framecodes=40), 1)]


@pytest.mark.parametrize("kind,S,N", [("h36m", 128, 16), ("h36m", 64, 16), ("single", 96, 48)])
def test_every_kernel_form_follows_the_selection(casters, kind, S, N):
    """forward(subject_idxs=...) on a two-subject bank, bitwise the one-subject caster's, in bf16 / fp16c / fp32: h36m (frame
    codes, K = 920, subjects with 64 and 40 codes) at 128 + 16 (the record form, above 112 samples) and at 64 + 16 (on chip
    with frame codes), and the single-net surreal config at 96 + 48."""
    if kind == "h36m":
        cfg, models = _h36m_models()
    else:
        cfg = surreal_single_config()
        models = [(wc, None, tv, td) for wc, _, tv, td in (syn.make_model(cfg, s) for s in SEEDS[:2])]     # one net per subject
    bank = casters(cfg, ("bank", kind), models=models)
    alone = [casters(cfg, ("alone", kind, s), models=[m]) for s, m in enumerate(models)]
    rb, skts, cyls = frame_rays(32, 32)
    n = rb.shape[0]
    cams = (torch.arange(n, device=DEV) % 40).float() if cfg.framecode_ch else None
    cams = None if cams is None else torch.where(torch.arange(n, device=DEV) % 7 == 0, -torch.ones_like(cams), cams)   # (some mean codes)
    call = lambda c, **kw: c(rb, N_samples=S, skts=skts, cyls=cyls, cams=cams, N_importance=N, **kw)
    outs = {}
    for prec in ("bf16", "fp16c", "fp32"):
        bank.renderer.set_precision(prec)
        for s in (1, 0):
            alone[s].renderer.set_precision(prec)
            want = call(alone[s])
            assert same_maps(call(bank, subject_idxs=torch.full((n, 1), s, device=DEV)), want), (prec, s, "per-ray tensor")
            assert same_maps(call(bank, subject_idxs=s), want), (prec, s, "int")
            outs[prec, s] = want
        assert (outs[prec, 0]["rgb_map"] - outs[prec, 1]["rgb_map"]).abs().max() > 1e-2
    assert bank.renderer.selected_subject == 0


def test_selection_between_enqueued_launches(casters):
    """Subject 0, 1, 0 enqueued on one stream with no host synchronisation in between (256 rays each at 64 + 16), per-subject
    tau and cutoff_dist: a cutoff buffer or workspace shared between subjects and rewritten under a launch in flight shows."""
    cfg = surreal_config()
    models = [syn.make_model(cfg, s) for s in SEEDS[:2]]
    emb = [((31.5, np.linspace(0.35, 0.6, 24)), (47.0, np.linspace(0.6, 0.4, 24))),
           ((90.0, np.linspace(0.55, 0.3, 24)), (64.0, np.full(24, 0.45)))]
    bank = casters(cfg, ("enqueue", "bank"), models=models)
    alone = [casters(cfg, ("enqueue", s), models=[m]) for s, m in enumerate(models)]
    for s in (0, 1):
        for c, ctx in ((alone[s], alone[s].subject(None)), (bank, bank.subject(s))):
            with ctx:
                c.renderer.set_precision("bf16")
                for which in (0, 1):
                    c.renderer.set_embedder(which, emb[s][which][0], emb[s][which][1])
    rb, skts, cyls = frame_rays(48, 48, n_rays=256)
    r = bank.renderer
    r.set_chunk(256)
    render = lambda rr: rr.render_rays(rb, skts, cyls, n_samples=64, n_importance=16)
    render(r)                                   # (sizes the workspaces once, so that nothing below has a reason to wait)
    torch.cuda.synchronize()
    got = []
    for s in (0, 1, 0):
        r.select_subject(s)
        got.append(render(r))                   # asynchronous: inputs and outputs live on the device
    torch.cuda.synchronize()
    r.select_subject(0)
    want = []
    for c in alone:
        c.renderer.set_chunk(256)
        want.append(render(c.renderer))
    torch.cuda.synchronize()
    for g, s in zip(got, (0, 1, 0)):
        assert same_maps(g, want[s]), s
    assert (want[0]["acc_map"] - want[1]["acc_map"]).abs().max() > 1e-2


def test_no_packing_in_steady_state(casters):
    """Once every subject has rendered in a precision, alternating between them builds no image (pg_subject_info)."""
    cfg = surreal_config()
    bank = casters(cfg, SEEDS)
    H = W = 48
    c2ws, focals, kw = path_inputs(10, H, W)
    rk = {"ray_caster": bank, "N_samples": 64, "N_importance": 16}
    r = bank.renderer
    for prec in ("bf16", "fp16c"):
        r.set_precision(prec)
        first = dict(kw, kp=kw["kp"][:3], skts=kw["skts"][:3])
        render_path(c2ws[:3], (H, W, focals[:3]), 1024, rk, subject_idxs=[0, 1, 2], **first)
        before = [r.subject_info(s) for s in range(3)]
        render_path(c2ws, (H, W, focals), 1024, rk, subject_idxs=[0, 1, 2], **kw)       # ten frames, round robin
        after = [r.subject_info(s) for s in range(3)]
        assert after == before, (prec, before, after)
        assert all(i["loaded_nets"] == [0, 1] and i["image_builds"] > 0 for i in after)
        assert len({i["image_bytes"] for i in after}) == 1 and after[0]["image_bytes"] > 1 << 20


def test_loads_hit_the_selected_subject_only(casters):
    cfg = surreal_config()
    m0, m1, m2 = (syn.make_model(cfg, s) for s in SEEDS)
    bank = HipRayCaster.from_subjects(cfg, [m0, m1], device=DEV, precision="bf16")
    fresh = casters(cfg, (2,))
    fresh.renderer.set_precision("bf16")
    rb, skts, cyls = frame_rays(32, 32)
    call = lambda c, **kw: c(rb, N_samples=64, skts=skts, cyls=cyls, N_importance=16, **kw)
    sd_eq = lambda a, b: set(a) == set(b) and all(set(a[k]) == set(b[k]) and all(same(a[k][n], b[k][n]) for n in a[k]) for k in a)
    r0, sd0 = call(bank, subject_idxs=0), bank.state_dict()
    other = fresh.state_dict()
    # 1. load_subject
    bank.load_subject(1, other)
    assert bank.renderer.selected_subject == 0
    assert same_maps(call(bank), r0) and sd_eq(bank.state_dict(), sd0)
    assert same_maps(call(bank, subject_idxs=1), call(fresh))
    with bank.subject(1):
        assert sd_eq(bank.state_dict(), other)
    # 2. select + load_state_dict
    one = casters(cfg, (1,))
    one.renderer.set_precision("bf16")
    bank.select_subject(1)
    bank.load_state_dict(one.state_dict())
    assert sd_eq(bank.state_dict(), one.state_dict()) and same_maps(call(bank), call(one))
    bank.select_subject(0)
    assert same_maps(call(bank), r0) and sd_eq(bank.state_dict(), sd0)
    # 3. the device route: subject 1 takes model 2's tensors from device memory
    from posegen_amd.raycaster import NET_TENSOR_ORDER
    with bank.subject(1):
        for which, w in ((0, m2[0]), (1, m2[1])):
            ts = [torch.tensor(w[k], device=DEV).reshape(w[k].shape[0], -1).contiguous() for k in NET_TENSOR_ORDER]
            bank.renderer.load_network_device(which, ts, state_provider=lambda w=w: {k: torch.tensor(v) for k, v in w.items()})
        assert same_maps(call(bank), call(fresh))
        assert same(bank.state_dict()["network_fine_state_dict"]["rgb_linear.weight"], m2[1]["rgb_linear.weight"])
    assert same_maps(call(bank), r0) and sd_eq(bank.state_dict(), sd0)
    # the bank's size: growing keeps what is loaded, shrinking keeps the rest; a dropped or unknown subject is refused
    bank.set_subject_count(4)
    assert same_maps(call(bank, subject_idxs=0), r0) and same_maps(call(bank, subject_idxs=1), call(fresh))
    assert bank.renderer.subject_info(3) == {"loaded_nets": [], "image_bytes": 0, "image_builds": 0}
    bank.set_subject_count(2)
    assert same_maps(call(bank, subject_idxs=1), call(fresh))
    bank.set_subject_count(1)
    assert same_maps(call(bank), r0)
    with pytest.raises(ValueError):
        call(bank, subject_idxs=1)
    bank.renderer.close()


def test_density_queries_follow_the_subject(casters):
    g = load_golden("rays_surreal")
    cfg = cfg_from_golden(g)
    bank = casters(cfg, SEEDS[:2])
    one = casters(cfg, (1,))
    rb, skts = torch.tensor(g["ray_batch"]), torch.tensor(g["skts"])
    z = torch.tensor(g["z_coarse"])
    n = 77                                        # 77 * 64 points: not a multiple of a pass
    pts = (rb[:n, None, 0:3] + rb[:n, None, 3:6] * z[:n, :, None]).reshape(-1, 3)
    kps = torch.tensor(g["kps"]) if "kps" in g else pts[:24][None]
    for prec in ("bf16", "fp32"):
        bank.renderer.set_precision(prec)
        one.renderer.set_precision(prec)
        want = one(pts[:, None, :], None, skts, None, fwd_type="density")
        assert same(bank(pts[:, None, :], None, skts, None, subject_idxs=1, fwd_type="density"), want)
        assert not same(bank(pts[:, None, :], None, skts, None, fwd_type="density"), want)
        assert same(bank(kps, skts, None, subject_idxs=torch.tensor([1]), radius=0.6, res=8, fwd_type="mesh"),
                    one(kps, skts, None, radius=0.6, res=8, fwd_type="mesh"))
    assert bank.renderer.selected_subject == 0


def test_multi_device_frames_keep_their_subject(casters):
    """HipRayCaster(devices=[0, 0]) (the real devices when there are two) with three subjects: five frames with small boxes
    and one with a box large enough to be cut across the two workers, all on one 96 x 96 canvas (a multi-device render_path
    has one frame size).  pg_render_frames_subjects must give bitwise the single-device bank's frames, and pg_render_frames
    (no subjects) the frames of a caster that holds the selected model alone."""
    from posegen_amd.dist import plan_tasks
    cfg = surreal_config()
    ndev = torch.cuda.device_count()
    devices = list(range(ndev)) if ndev >= 2 else [0, 0]
    subj = [0, 1, 2, 2, 0, 1]
    H = W = 96
    c2ws, focals, kw = path_inputs(len(subj), H, W, seed=5)
    focals = focals * np.array([0.4] * 5 + [1.0], dtype=np.float32)      # five small boxes, one large (frame 5)
    chunk = 256
    rk = lambda c: {"ray_caster": c, "N_samples": 64, "N_importance": 16}
    bank1 = casters(cfg, SEEDS)
    bank1.renderer.set_precision("bf16")
    want = render_path(c2ws, (H, W, focals), chunk, rk(bank1), subject_idxs=subj, **kw)
    tasks = plan_tasks([len(v) for v in want[3]], 2, chunk)
    assert any(t.r0 > 0 and t.frame == 5 for t in tasks), "the large frame is cut across the two workers"
    bank2 = casters(cfg, SEEDS, devices=devices)
    bank2.renderer.set_precision("bf16")
    got = render_path(c2ws, (H, W, focals), chunk, rk(bank2), subject_idxs=subj, **kw)
    for a, b in zip(want[:3], got[:3]):
        assert same(a, b)
    assert bank2.renderer.selected_subject == 0
    assert np.abs(want[0][5] - render_path(c2ws, (H, W, focals), chunk, rk(bank1), subject_idxs=0, **kw)[0][5]).max() > 1e-2
    # null subjects: today's pg_render_frames, with the selected subject
    alone = casters(cfg, (0,))
    alone.renderer.set_precision("bf16")
    today = render_path(c2ws, (H, W, focals), chunk, rk(alone), **kw)
    plain = render_path(c2ws, (H, W, focals), chunk, rk(bank2), **kw)
    for a, b in zip(today[:3], plain[:3]):
        assert same(a, b)
    with pytest.raises(ValueError):
        render_path(c2ws, (H, W, focals), chunk, rk(bank2), subject_idxs=[0, 3], **kw)


def test_gan_loop_takes_one_subject_per_pose(casters):
    from posegen_amd.ganloop import render_for_regressor
    from posegen_amd.skeleton import SURREAL_REST_SCALE, smpl_rest_pose
    cfg = surreal_config()
    bank = casters(cfg, SEEDS[:2])
    subj = [0, 1, 1, 0]
    H = W = 128
    rest = smpl_rest_pose * SURREAL_REST_SCALE
    c2ws, focals = syn.make_camera(1, H, W)
    bones = torch.tensor(syn.make_bones(4, 7), device=DEV)
    args = (bones, rest, c2ws[0], H, W, float(focals[0]))
    kw = dict(ext_scale=cfg.ext_scale, crop=(16, 112), out_res=56, return_frames=True)
    bank.renderer.set_precision("bf16")
    img, frames = render_for_regressor(bank, *args, subject_idxs=subj, **kw)
    assert img.shape == (4, 3, 56, 56) and bank.renderer.selected_subject == 0
    per = []
    for s in (0, 1):
        c = casters(cfg, (s,))
        c.renderer.set_precision("bf16")
        per.append(render_for_regressor(c, *args, **kw))
    for i, s in enumerate(subj):
        assert same(img[i], per[s][0][i]) and same(frames[i], per[s][1][i]), i
    assert (frames[1].float() - per[0][1][1].float()).abs().max() > 2
