"""CPU tests of the subject bank (several A-NeRF models behind one caster): the C ABI's surface, the Python layer's
argument validation on a stub renderer (no library call may happen before a refusal), the per-frame subject in the
frame drivers and in the process-per-GPU plan (gloo, world size 2), and the bank's swap logic under ASan + UBSan."""
import os
import re
import subprocess
import types

import numpy as np
import pytest
import torch

from posegen_amd import _ffi, surreal_config, synthetic as syn
from posegen_amd.raycaster import MIXED_SUBJECTS, HipRayCaster, HipRenderer, call_subject, frame_subjects
from tests.test_host_logic import _run_world2

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ("pg_set_subject_count", "pg_select_subject", "pg_subject_info", "pg_render_frames_subjects")


def test_header_declares_the_bank_and_the_abi_version_stays():
    hdr = open(os.path.join(REPO, "include", "posegen_hip.h")).read()
    declared = set(re.findall(r"\b(pg_[a-z0-9_]+)\s*\(", hdr))
    for name in NEW_SYMBOLS:
        assert name in declared, f"{name} is not declared in include/posegen_hip.h"
        assert name in _ffi.PROTOTYPES, f"{name} has no ctypes prototype"
        assert _ffi.PROTOTYPES[name][0] is _ffi.C.c_int
    # pg_render_frames_subjects = pg_render_frames' arguments + the subjects
    assert _ffi.PROTOTYPES["pg_render_frames_subjects"][1][:-1] == _ffi.PROTOTYPES["pg_render_frames"][1]
    assert re.search(r"#define\s+PG_ABI_VERSION\s+11\b", hdr) and _ffi.PG_ABI_VERSION == 11
    assert re.search(r"#define\s+PG_MAX_SUBJECTS\s+64\b", hdr)
    lib = _ffi.load_library()
    for name in NEW_SYMBOLS:
        assert hasattr(lib, name)
    assert lib.pg_abi_version() == 11


# ---- a HipRenderer without a library: the real bookkeeping (subject / select_subject / _state), recorded calls ----------
class _Lib:
    def __init__(self, log):
        self.log = log

    def __getattr__(self, name):
        def call(*a):
            self.log.append((name,) + tuple(x for x in a[1:] if isinstance(x, int)))
            return 0
        return call


class StubRenderer(HipRenderer):
    def __init__(self, n_subjects=1, cfg=None):         # (no pg_create: no GPU)
        self.cfg = cfg or surreal_config()
        self.device = torch.device("cpu")
        self.devices = [0]
        self.log = []
        self.lib = _Lib(self.log)
        self.handle = None
        self._subjects = [{"state": {}, "lazy": {}}]
        self._subject = 0
        self._chunk = self.cfg.chunk
        self.set_subject_count(n_subjects)
        self.log.clear()

    @property
    def pose_boxes(self):                               # (no device: the frame drivers take the host route to the boxes)
        raise AttributeError("pose_boxes")

    def render_rays(self, ray_batch, skts, cyls, **kw):
        self.log.append(("render_rays", self._subject, int(ray_batch.shape[0])))
        return {"rgb_map": torch.zeros(ray_batch.shape[0], 3)}

    def query_density(self, pts, skts, which=None):
        self.log.append(("query_density", self._subject))
        return torch.zeros(pts.shape[0], 1)

    def render_frame(self, H, W, focal, c2w, box, skts, cyl, **kw):
        self.log.append(("render_frame", self._subject))
        return torch.full((H, W, 3), float(self._subject)), torch.zeros(H, W, 1), torch.zeros(H, W, 1)


def stub_caster(n_subjects):
    c = object.__new__(HipRayCaster)
    c.cfg = surreal_config()
    c.renderer = StubRenderer(n_subjects, c.cfg)
    c.training = False
    return c


def _call(c, subject_idxs, n=8):
    return c(torch.zeros(n, 11), N_samples=64, skts=torch.zeros(1, 24, 4, 4), cyls=torch.zeros(1, 5), N_importance=16,
             subject_idxs=subject_idxs)


def test_a_ray_call_renders_the_one_subject_it_names_and_restores_the_selection():
    c = stub_caster(3)
    c.select_subject(1)
    c.renderer.log.clear()
    for given in (2, np.int64(2), torch.tensor(2), torch.full((8, 1), 2), torch.full((8,), 2.0), [2] * 8):
        _call(c, given)
    renders = [e for e in c.renderer.log if e[0] == "render_rays"]
    assert renders == [("render_rays", 2, 8)] * 6
    assert c.renderer.selected_subject == 1
    selects = [e for e in c.renderer.log if e[0] == "pg_select_subject"]
    assert selects == [("pg_select_subject", 2), ("pg_select_subject", 1)] * 6
    c.renderer.log.clear()
    _call(c, None)                                       # no subject: the selected one, and no selection call at all
    _call(c, 1)                                          # the selected one by name: nothing to select either
    assert c.renderer.log == [("pg_set_chunk", 8), ("render_rays", 1, 8), ("pg_set_chunk", c.cfg.chunk)] * 2


def test_mixed_subjects_in_one_ray_call_are_refused_with_the_documented_message():
    c = stub_caster(3)
    mixed = torch.tensor([0, 0, 1, 1, 0, 0, 0, 0])
    for call in (lambda: _call(c, mixed), lambda: _call(c, mixed[:, None]),
                 lambda: c(torch.zeros(4, 1, 3), None, torch.zeros(1, 24, 4, 4), None, subject_idxs=[0, 1], fwd_type="density"),
                 lambda: c(torch.zeros(1, 24, 3), torch.zeros(1, 24, 4, 4), subject_idxs=torch.tensor([2, 1]), res=2, fwd_type="mesh")):
        with pytest.raises(NotImplementedError) as e:
            call()
        assert str(e.value) == MIXED_SUBJECTS
    assert "per-ray mixing of subjects is not built" in MIXED_SUBJECTS
    assert c.renderer.log == [], "refused before any library call"


@pytest.mark.parametrize("bad", [3, -1, 1.5, torch.tensor([2.5] * 8), torch.full((8,), 7), float("nan"), True, "1",
                                 torch.tensor([-2] * 8)])
def test_bad_subject_indices_raise_before_any_library_call(bad):
    c = stub_caster(3)
    for call in (lambda: _call(c, bad),
                 lambda: c.render_pts_density(torch.zeros(4, 3), None, torch.zeros(1, 24, 4, 4), subject_idxs=bad),
                 lambda: c.render_mesh_density(torch.zeros(1, 24, 3), torch.zeros(1, 24, 4, 4), subject_idxs=bad, res=2)):
        with pytest.raises(ValueError):
            call()
    with pytest.raises(ValueError):
        frame_subjects([0, bad] if not isinstance(bad, torch.Tensor) else bad, 4, 3)
    with pytest.raises(ValueError):
        c.select_subject(3)
    assert c.renderer.log == [], "refused before any library call"


def test_a_one_subject_caster_accepts_only_subject_zero():
    c = stub_caster(1)
    _call(c, 0)
    _call(c, torch.zeros(8, 1, dtype=torch.long))
    assert [e for e in c.renderer.log if e[0] == "render_rays"] == [("render_rays", 0, 8)] * 2
    assert not [e for e in c.renderer.log if e[0] == "pg_select_subject"]
    with pytest.raises(ValueError, match=r"outside \[0, 1\)"):
        _call(c, 1)
    assert call_subject(None, 1) is None and frame_subjects(None, 5, 1) is None


def test_per_frame_subjects_broadcast_like_every_per_pose_argument():
    assert frame_subjects([0, 1, 2], 7, 3) == [0, 1, 2, 0, 1, 2, 0]
    assert frame_subjects(torch.tensor([2, 0]), 5, 3) == [2, 0, 2, 0, 2]
    assert frame_subjects(1, 3, 2) == [1, 1, 1]
    assert frame_subjects(np.array([[0], [1]]), 2, 2) == [0, 1]
    with pytest.raises(ValueError):
        frame_subjects([], 2, 2)
    with pytest.raises(ValueError):
        frame_subjects([0, 2], 2, 2)


def test_the_frame_loop_selects_each_frames_subject_and_puts_the_selection_back():
    from posegen_amd.render import render_frames_device, render_path
    c = stub_caster(3)
    c.select_subject(2)
    H = W = 32
    F = 5
    _, kps, skts = syn.make_pose(F, 3)
    c2ws, focals = syn.make_camera(F, H, W)
    rk = {"ray_caster": c, "N_samples": 64, "N_importance": 16}
    kw = dict(kp=torch.tensor(kps), skts=torch.tensor(skts), white_bkgd=True, ext_scale=0.001)
    for given, want in (([0, 1], [0, 1, 0, 1, 0]), (torch.tensor([2, 1, 0, 0, 1]), [2, 1, 0, 0, 1]), (1, [1] * 5), (None, [2] * 5)):
        c.renderer.log.clear()
        rgbs = render_frames_device(torch.tensor(c2ws), (H, W, focals), 256, rk, subject_idxs=given, **kw)[0]
        assert [e[1] for e in c.renderer.log if e[0] == "render_frame"] == want
        assert [float(x) for x in rgbs[:, 0, 0, 0]] == [float(s) for s in want]
        assert c.renderer.selected_subject == 2
        if given is None:
            assert not [e for e in c.renderer.log if e[0] == "pg_select_subject"]
    # render_path hands them on (it dropped them before); a subset of frames keeps each frame's own subject
    c.renderer.log.clear()
    out = render_path(torch.tensor(c2ws), (H, W, focals), 256, rk, subject_idxs=[0, 1, 2, 1, 0], frame_ids=[3, 2], **kw)
    assert [e[1] for e in c.renderer.log if e[0] == "render_frame"] == [1, 2]
    assert [float(x) for x in out[0][:, 0, 0, 0]] == [1.0, 2.0]
    c.renderer.log.clear()
    with pytest.raises(ValueError):
        render_path(torch.tensor(c2ws), (H, W, focals), 256, rk, subject_idxs=[0, 3], **kw)
    assert not [e for e in c.renderer.log if e[0] in ("render_frame", "pg_select_subject")]


def test_state_bookkeeping_is_per_subject():
    """subject 1's load must not overwrite subject 0's host state (state_dict / parameters act on the selected subject)"""
    c = stub_caster(2)
    cfg = c.cfg
    m0, m1 = syn.make_model(cfg, 0), syn.make_model(cfg, 1)
    for s, (wc, wf, tv, td) in enumerate((m0, m1)):
        with c.subject(s):
            c.renderer.load_network(0, wc)
            c.renderer.load_network(1, wf)
            c.renderer.set_embedder(0, tv)
            c.renderer.set_embedder(1, td + s)
    assert c.renderer.selected_subject == 0
    sd0 = c.state_dict()
    with c.subject(1):
        sd1 = c.state_dict()
        n1 = len(list(c.parameters()))
    k = "pts_linears.3.weight"
    assert np.array_equal(sd0["network_fn_state_dict"][k].numpy(), m0[0][k])
    assert np.array_equal(sd1["network_fn_state_dict"][k].numpy(), m1[0][k])
    assert np.array_equal(sd1["network_fine_state_dict"][k].numpy(), m1[1][k])
    f32 = lambda v: float(np.float32(v))
    assert float(sd0["embeddirs_state_dict"]["tau"]) == f32(m0[3]) and float(sd1["embeddirs_state_dict"]["tau"]) == f32(m1[3] + 1)
    assert n1 == len(list(c.parameters()))
    # load_subject: the checkpoint layout of load_state_dict applied to subject 1, subject 0 untouched, selection kept
    c.load_subject(1, sd0)
    with c.subject(1):
        assert np.array_equal(c.state_dict()["network_fn_state_dict"][k].numpy(), m0[0][k])
    assert c.renderer.selected_subject == 0
    assert np.array_equal(c.state_dict()["network_fn_state_dict"][k].numpy(), m0[0][k])
    # shrinking drops the dropped subjects' bookkeeping
    c.set_subject_count(1)
    assert c.n_subjects == 1 and ("pg_set_subject_count", 1) in c.renderer.log


def test_trainable_raycaster_refuses_a_bank_and_subjects_in_training_mode():
    from posegen_amd.train import TrainableRayCaster
    bank = types.SimpleNamespace(cfg=surreal_config(), n_subjects=2)
    with pytest.raises(NotImplementedError, match="training a subject bank is not built"):
        TrainableRayCaster(bank)
    # training mode keeps refusing subject_idxs, by name, before anything else happens
    t = object.__new__(TrainableRayCaster)
    torch.nn.Module.__init__(t)
    t.caster = stub_caster(1)
    t.network_fine = None
    t.train()
    with pytest.raises(NotImplementedError, match="subject_idxs in training mode is not built"):
        t.forward(torch.zeros(4, 11), skts=torch.zeros(1, 24, 4, 4), cyls=torch.zeros(1, 5), subject_idxs=0)
    assert t.caster.renderer.log == []


_GLOO_SUBJECT_WORKER = r"""
import os, sys, numpy as np, torch, torch.distributed as dist
sys.path.insert(0, sys.argv[1])
from posegen_amd import synthetic as syn
from posegen_amd.dist import plan_tasks, render_path_distributed
from posegen_amd.render import render_path

class StubRenderer:                       # a ray's maps = f(subject, box, pose, camera, ray index); records (frame, subject)
    device = torch.device("cpu")
    n_subjects = 3
    selected_subject = 0
    seen = []
    pose_sums = []
    def set_chunk(self, c): self.chunk = c
    def select_subject(self, s):
        assert 0 <= s < self.n_subjects
        StubRenderer.selected_subject = s
    def render_frame_range(self, H, W, focal, c2w, box, skts, cyl, r0, r1, center=None, cam=None, **kw):
        assert r0 == 0 or r0 % self.chunk == 0, "a run starts on a nanmean group boundary"
        ps = float(torch.as_tensor(skts).sum())
        frame = min(range(len(self.pose_sums)), key=lambda i: abs(self.pose_sums[i] - ps))
        StubRenderer.seen.append((frame, self.selected_subject))
        v = (ps + float(np.asarray(c2w).sum())) % 1.0
        i = torch.arange(r0, r1, dtype=torch.float32)
        rgb = torch.stack([v + 0 * i, (i % 7) / 7, 0.125 * self.selected_subject + 0 * i], -1)
        disp = torch.full((r1 - r0,), float("nan"))
        acc = 0.5 + 0.25 * torch.sin(i)
        return torch.cat([rgb.reshape(-1), disp, acc])
    def compose_frame(self, H, W, box, rgb_map, disp_map, acc_map, bg=None, base_bg=0., **kw):
        (tlx, tly), (brx, bry) = box
        rgb = torch.full((H, W, 3), float(base_bg)); disp = torch.zeros(H, W, 1); acc = torch.zeros(H, W, 1)
        bh, bw = bry - tly, brx - tlx
        rgb[tly:bry, tlx:brx] = rgb_map.view(bh, bw, 3) + (1 - acc_map.view(bh, bw, 1)) * base_bg
        disp[tly:bry, tlx:brx] = torch.nan_to_num(disp_map.view(bh, bw, 1), nan=0.0)
        acc[tly:bry, tlx:brx] = acc_map.view(bh, bw, 1)
        return rgb, disp, acc
    def render_frame(self, H, W, focal, c2w, box, skts, cyl, **kw):
        (tlx, tly), (brx, bry) = box
        n = (bry - tly) * (brx - tlx)
        p = self.render_frame_range(H, W, focal, c2w, box, skts, cyl, 0, n)
        return self.compose_frame(H, W, box, p[:3 * n].view(n, 3), p[3 * n:4 * n], p[4 * n:], base_bg=kw.get("base_bg", 0.))
class StubCaster:
    renderer = StubRenderer()
    module = property(lambda self: self)

dist.init_process_group("gloo")
rank, world = dist.get_rank(), dist.get_world_size()
H = W = 64
for F, subj, want_subj in ((3, [2, 0, 1], [2, 0, 1]), (1, 1, [1]), (5, [1, 2], [1, 2, 1, 2, 1])):     # F odd: a frame is cut between the ranks
    _, kps, skts = syn.make_pose(F, 3)
    c2ws, focals = syn.make_camera(F, H, W)
    StubRenderer.pose_sums = [float(torch.tensor(skts[i]).sum()) for i in range(F)]
    kw = dict(kp=torch.tensor(kps), skts=torch.tensor(skts), white_bkgd=True, ext_scale=0.001, ret_acc=True, subject_idxs=subj)
    rk = {"ray_caster": StubCaster(), "N_samples": 64, "N_importance": 16}
    StubRenderer.selected_subject = 0
    want = render_path(torch.tensor(c2ws), (H, W, focals), 256, rk, **kw)
    assert StubRenderer.selected_subject == 0
    StubRenderer.seen = []
    got = render_path_distributed(torch.tensor(c2ws), (H, W, focals), 256, rk, **kw)
    assert StubRenderer.selected_subject == 0, "the selection is put back"
    for a, b in zip(want[:3], got[:3]):
        assert a.shape == b.shape and np.array_equal(a, b), (rank, F)
    # the plan carried every frame's subject to the rank that rendered it, the runs of a cut frame included
    mine = [t for t in plan_tasks([len(v) for v in want[3]], world, 256) if t.worker == rank and t.r1 > t.r0]
    assert StubRenderer.seen == [(t.frame, want_subj[t.frame]) for t in mine], (rank, StubRenderer.seen)
    cut = {t.frame for t in plan_tasks([len(v) for v in want[3]], world, 256) if t.r0 > 0}
    assert cut or F != 3, "the three-frame case cuts a frame between the ranks"
    # without subjects nothing is selected and every frame is the selected subject's
    StubRenderer.seen = []
    kw["subject_idxs"] = None
    render_path_distributed(torch.tensor(c2ws), (H, W, focals), 256, rk, **kw)
    assert all(s == 0 for _, s in StubRenderer.seen)
bad = dict(kw, subject_idxs=[0, 3])
try:
    render_path_distributed(torch.tensor(c2ws), (H, W, focals), 256, rk, **bad)
    raise SystemExit("an out-of-range subject was accepted")
except ValueError:
    pass
dist.barrier()
dist.destroy_process_group()
open(os.path.join(os.path.dirname(os.path.abspath(__file__)), f"ok_{rank}"), "w").write("ok")
"""


def test_render_path_distributed_gloo_world2_carries_each_frames_subject(tmp_path):
    """dist.py's plan carries each frame's subject to the rank that renders it: a stub caster records (frame, subject) on
    both ranks, cut frames included, and the assembled frames are those of the single-process render."""
    _run_world2(tmp_path, _GLOO_SUBJECT_WORKER)


def test_subject_bank_swap_logic_is_clean_under_address_and_ub_sanitizers(tmp_path):
    """pg_bank.h (what pg_set_subject_count / pg_select_subject run) as a stand-alone program with its own main: grow, shrink,
    select; no leak of host vectors or of the subjects' "device" memory, no use after a shrink."""
    clang = "/opt/rocm/lib/llvm/bin/clang++"
    if not os.path.exists(clang):
        pytest.skip("ROCm clang++ not found")
    exe = str(tmp_path / "subject_bank_asan")
    csrc = os.path.join(REPO, "posegen_amd", "csrc")
    build = subprocess.run([clang, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                            "-fno-omit-frame-pointer", "-I", csrc, os.path.join(REPO, "tools", "sanitize", "subject_bank_asan.cpp"),
                            "-o", exe], capture_output=True, text=True)
    if build.returncode != 0 and "sanitizer" in build.stderr.lower() and "cannot find" in build.stderr.lower():
        pytest.skip("sanitizer runtime not installed")
    assert build.returncode == 0, build.stderr[-2000:]
    run = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert run.returncode == 0, (run.stdout[-1500:], run.stderr[-3000:])
    assert "subject bank clean under ASan/UBSan" in run.stdout
