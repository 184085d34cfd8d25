"""CPU tests of the training batches (posegen_amd/batches.py, csrc/pg_batch.hip): the numpy restatement the GPU tests compare the
kernels with (tests/batches_ref.py) against batches of the real reference data path (tests/golden/train_batches.npz, written by
tools/gen_golden_batches.py), the properties of the Floyd sampler, the C ABI's surface, and the Python layer's refusals on a logging
fake renderer (no library call may happen before a refusal)."""
import itertools
import os
import re
import types

import numpy as np
import pytest
import torch

from posegen_amd import _ffi, batches
from posegen_amd import DeviceImageBank, ImageBatchSampler, RayBatchSource
from tests import batches_ref as ref

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ("pg_pixel_index_count", "pg_pixel_index_emit", "pg_batch_sample_pixels", "pg_batch_gather")
VARIANTS = ("plain", "centers", "mask_img")


@pytest.fixture(scope="module")
def golden():
    return dict(np.load(os.path.join(REPO, "tests", "golden", "train_batches.npz")))


def golden_bank(g, variant):
    """The inputs of one variant of the golden as tests/batches_ref.gather (and DeviceImageBank) take them."""
    bank = {k: g[f"in_{k}"] for k in ("imgs", "masks", "sampling_masks", "bkgds", "bkgd_idxs", "c2ws")}
    bank["HW"] = tuple(int(v) for v in g["HW"])
    bank["focals"] = g["in_focals_xy"] if variant == "centers" else g["in_focals"]
    bank["centers"] = g["in_centers"] if variant == "centers" else None
    bank["mask_img"] = variant == "mask_img"
    return bank


# ---- the restatement against the reference's batches ------------------------------------------------------------------------

@pytest.mark.parametrize("variant", VARIANTS)
def test_restated_gather_equals_the_reference_batches(golden, variant):
    g = golden
    assert sorted(g["variants"]) == sorted(VARIANTS)
    bank = golden_bank(g, variant)
    H, W = bank["HW"]
    k = int(g["k_pixels"])
    for b in range(3):
        key = lambda name: g[f"{variant}_b{b}_{name}"]
        items, pix = key("items"), key("pixel_idxs")
        assert np.array_equal(items, np.sort(items)) and pix.shape == (len(items), k)
        out = ref.gather(bank, items, pix)
        for name in ("target_s", "fgs", "bgs", "rays_o"):
            assert out[name].dtype == key(name).dtype == np.float32
            assert np.array_equal(out[name], key(name)), (variant, b, name)
        per_ray = np.repeat(items, k)
        assert key("kp_idx").dtype == key("cam_idxs").dtype == np.int64
        assert np.array_equal(key("kp_idx"), per_ray) and np.array_equal(key("cam_idxs"), per_ray)
        for name in ("kp3d", "bones", "skts", "cyls"):
            assert np.array_equal(key(name), g[f"in_{name}"][per_ray])
        # rays_d: one rounding each for the division, the three products and the two sums of
        # (x R[c,0] + y R[c,1]) + z R[c,2] -> 6 2^-24 sum_c |dirs_c R[r,c]| per component of the (float64) golden
        p = pix.reshape(-1)
        row, col = (p // W).astype(np.float64), (p % W).astype(np.float64)
        focal = np.asarray(bank["focals"], np.float64).reshape(len(bank["c2ws"]), -1)[per_ray]
        if bank["centers"] is not None:
            c = bank["centers"].astype(np.float64)[per_ray]
            x, y = (col - c[:, 0]) / focal[:, 0], (-row + c[:, 1]) / focal[:, -1]
        else:
            x, y = (col - W * 0.5) / focal[:, 0], (-(row - H * 0.5)) / focal[:, -1]
        dirs = np.stack([x, y, -np.ones_like(x)], -1)
        R = bank["c2ws"].astype(np.float64)[per_ray][:, :3, :3]
        bound = 6 * 2.0 ** -24 * np.abs(dirs[:, None, :] * R).sum(-1)
        err = np.abs(out["rays_d"].astype(np.float64) - key("rays_d").astype(np.float64))
        assert (err <= bound).all(), (variant, b, float((err / bound).max()))
        assert np.array_equal(key("rays")[0], key("rays_o")) and key("rays").shape == (2, len(p), 3)
        # the packing of render() (trainer.py:118-137)
        rb = out["ray_batch"]
        assert np.array_equal(rb[:, :3], out["rays_o"]) and np.array_equal(rb[:, 3:6], out["rays_d"])
        assert (rb[:, 6] == 0).all() and (rb[:, 7] == 1).all()
        d64 = out["rays_d"].astype(np.float64)
        assert np.abs(rb[:, 8:] - d64 / np.linalg.norm(d64, axis=-1, keepdims=True)).max() <= 4 * 2.0 ** -24


def test_image_batch_sampler_reproduces_the_reference_batches(golden):
    want = golden["sampler_batches"]
    n_items, n_images = len(golden["in_imgs"]), int(golden["n_images"])
    torch.manual_seed(int(golden["seed_sampler"]))
    got = list(ImageBatchSampler(n_items, n_images, N_iter=len(want)))
    assert np.array_equal(np.stack(got), want)
    torch.manual_seed(int(golden["seed_sampler"]))
    assert np.array_equal(np.stack(ref.image_batches(n_items, n_images, len(want))), want)
    # 6 items in batches of 4: the permutation restarts inside a batch
    assert len(ImageBatchSampler(n_items, n_images)) == n_items
    assert all(np.array_equal(b, np.sort(b)) for b in got)


def test_restated_pixel_index_is_np_where_of_every_image(golden):
    masks = golden["in_sampling_masks"]
    counts, start, ids = ref.pixel_index(masks)
    assert set(np.unique(masks)) == {0, 1, 255}
    for f in range(len(masks)):
        assert np.array_equal(ids[start[f]:start[f + 1]], np.where(masks[f] > 0)[0])
    assert start[-1] == counts.sum() == len(ids)
    # the pixels every golden item drew are valid pixels of its image
    for variant in VARIANTS:
        for b in range(3):
            for img, pix in zip(golden[f"{variant}_b{b}_items"], golden[f"{variant}_b{b}_pixel_idxs"]):
                assert np.isin(pix, ids[start[img]:start[img + 1]]).all() and (np.diff(pix) > 0).all()


# ---- the sampler restatement ---------------------------------------------------------------------------------------------------

def test_floyd_sample_is_sorted_distinct_and_inside_the_mask():
    rng = np.random.default_rng(3)
    masks = (rng.random((4, 300)) < 0.3).astype(np.uint8) * 255
    counts, start, ids = ref.pixel_index(masks)
    k = 17
    rows = np.array([2, 0, 3, 2])
    pix = ref.sample_pixels(counts, start, ids, rows, k, rng.random((len(rows), k)))
    for a, img in enumerate(rows):
        assert (np.diff(pix[a]) > 0).all() and (masks[img, pix[a]] > 0).all()
    assert not np.array_equal(pix[0], pix[3])                  # the same image twice: two independent rows of draws


@pytest.mark.parametrize("u", [0.0, 1.0 - 2.0 ** -53, 0.5])
@pytest.mark.parametrize("m,k", [(1, 1), (7, 3), (64, 64), (1 << 20, 5), (65, 64)])
def test_floyd_at_degenerate_draws(m, k, u):
    r = ref.floyd_ranks(m, k, np.full(k, u))
    assert len(r) == k and (np.diff(r) > 0).all() and r[0] >= 0 and r[-1] < m
    if m == k:
        assert np.array_equal(r, np.arange(m))                 # count == k: every valid pixel
    if u == 0.0:
        assert np.array_equal(r, np.r_[0, np.arange(m - k + 1, m)])
    if u == 1.0 - 2.0 ** -53:
        assert np.array_equal(r, np.arange(m - k, m))          # floor(u (j + 1)) = j: always the new top rank


def test_floyd_count_equal_k_returns_every_valid_pixel():
    rng = np.random.default_rng(5)
    for m in (1, 2, 12, 100):
        assert np.array_equal(ref.floyd_ranks(m, m, rng.random(m)), np.arange(m))


def test_floyd_is_uniform_over_the_subsets():
    m, k, trials = 7, 3, 35000
    draws = np.random.default_rng(2024).random((trials, k))
    seen = {}
    for u in draws:
        key = tuple(ref.floyd_ranks(m, k, u))
        seen[key] = seen.get(key, 0) + 1
    subsets = list(itertools.combinations(range(m), k))
    assert len(subsets) == 35 and set(seen) == set(subsets)
    sigma = np.sqrt(trials * (1 / 35) * (34 / 35))             # ~ 31.2
    assert 31 < sigma < 32
    worst = max(abs(seen[s] - trials / 35) for s in subsets)
    assert worst <= 5 * sigma, worst


# ---- header and export -----------------------------------------------------------------------------------------------------------

def test_the_four_entry_points_are_declared_exported_and_bound():
    hdr = open(os.path.join(REPO, "include", "posegen_hip.h")).read()
    declared = set(re.findall(r"\b(pg_[a-z0-9_]+)\s*\(", hdr))
    lib = _ffi.load_library()
    for name in NEW_SYMBOLS:
        assert name in declared, f"{name} is not declared in include/posegen_hip.h"
        assert name in _ffi.PROTOTYPES and _ffi.PROTOTYPES[name][0] is _ffi.C.c_int
        assert hasattr(lib, name)
    assert re.search(r"#define\s+PG_ABI_VERSION\s+11\b", hdr) and _ffi.PG_ABI_VERSION == 11 and lib.pg_abi_version() == 11
    # pg_image_bank as the header lays it out: 7 pointers, 4 int64, 3 int32 (+ padding)
    assert re.search(r"typedef struct pg_image_bank \{", hdr)
    assert _ffi.PgImageBank.F.offset == 56 and _ffi.PgImageBank.H.offset == 88 and _ffi.C.sizeof(_ffi.PgImageBank) == 104
    import posegen_amd
    for name in ("DeviceImageBank", "ImageBatchSampler", "RayBatchSource"):
        assert getattr(posegen_amd, name) is getattr(batches, name)


# ---- refusals, before any library call --------------------------------------------------------------------------------------------

class _Lib:
    def __init__(self, log):
        self.log = log

    def __getattr__(self, name):
        def call(*a):
            self.log.append(name)
            return 0
        return call


class FakeRenderer:
    def __init__(self, device="cpu"):
        self.device = torch.device(device)
        self.log = []
        self.lib = _Lib(self.log)
        self.handle = None

    def _check(self, rc):
        self.log.append("check")

    def _stream(self):
        self.log.append("stream")
        return None


def fake_bank(HW=(20, 14), F=6, counts=None):
    r = FakeRenderer()
    return types.SimpleNamespace(renderer=r, device=r.device, HW=HW, P=HW[0] * HW[1], F=F, n_cam=F, bkgds=None,
                                 counts=np.full(F, 50, np.int64) if counts is None else np.asarray(counts, np.int64))


def test_a_renderer_off_the_device_is_refused_in_the_pose_layers_words():
    r = FakeRenderer("cpu")
    z = np.zeros((2, 4, 3), np.uint8)
    with pytest.raises(NotImplementedError, match=r"the renderer is on cpu, not on a HIP device \(torch 'cuda:N'\)"):
        DeviceImageBank(r, z, z[..., :1], z[..., 0], np.zeros((2, 4, 4)), np.ones(2), (2, 2))
    assert r.log == []


@pytest.mark.parametrize("kw,match", [(dict(patch_size=2), "patch_size"), (dict(N_nms=1), "N_nms"), (dict(N_nms=0.5), "N_nms"),
                                      (dict(multiview=True), "multiview")])
def test_unbuilt_options_are_refused_before_any_library_call(kw, match):
    bank = fake_bank()
    with pytest.raises(NotImplementedError, match=match):
        RayBatchSource(bank, 24, 4, **kw)
    assert bank.renderer.log == []


def test_banks_of_different_frame_sizes_are_refused():
    a, b = fake_bank((20, 14)), fake_bank((16, 16))
    with pytest.raises(NotImplementedError, match="different frame sizes"):
        RayBatchSource([a, b], 24, 4)
    with pytest.raises(NotImplementedError, match="ConcatH5Dataset"):
        RayBatchSource([a, fake_bank((20, 14))], 24, 4)
    assert a.renderer.log == [] and b.renderer.log == []


def test_more_pixels_than_an_image_has_is_numpys_value_error():
    with pytest.raises(ValueError) as numpys:
        np.random.choice(np.arange(3), 5, replace=False)
    assert str(numpys.value) == batches.CHOICE_MESSAGE
    bank = fake_bank(counts=[50, 50, 5, 50, 50, 50])
    src = RayBatchSource(bank, 24, 4)                          # 6 pixels per image
    with pytest.raises(ValueError) as mine:
        src.sample([0, 2, 3, 3])
    assert str(mine.value) == str(numpys.value)
    assert bank.renderer.log == []


def test_bad_source_arguments_are_refused():
    bank = fake_bank()
    with pytest.raises(ValueError, match="pixels per image"):
        RayBatchSource(bank, 3, 4)                             # 0 pixels per image
    with pytest.raises(ValueError, match="pixels per image"):
        RayBatchSource(bank, 4 * 1025, 4)
    with pytest.raises(IndexError):
        RayBatchSource(bank, 24, 4, items={"img_row": np.array([0, 6])})
    with pytest.raises(IndexError):
        RayBatchSource(bank, 24, 4).sample([0, 1, 2, 6])
    with pytest.raises(TypeError):
        RayBatchSource(bank, 24, 4, items={"img_row": np.array([0.0, 1.0])})
    assert bank.renderer.log == []
