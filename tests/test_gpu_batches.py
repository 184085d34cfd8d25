"""Training batches on the device (posegen_amd/batches.py; pg_pixel_index_count / pg_pixel_index_emit / pg_batch_sample_pixels /
pg_batch_gather, csrc/pg_batch.hip) against the numpy restatement tests/batches_ref.py, which tests/test_batches_host.py holds to
batches of the real reference data path (tests/golden/train_batches.npz).

Device outputs equal the restatement BIT FOR BIT -- integer outputs, and float32 outputs formed by the same IEEE operations in the
same order -- except ray_batch[:, 8:11] (the view directions, carried but unused by the nets that ship): within 4 float32 ulps of
the normalisation in float64.  (Its float32 error: the squares and the two sums under the square root are three roundings of 2^-24
relative, halved by the root, plus the root's and the division's own: 3.5 x 2^-24 relative, which is below 3.5 ulps.)"""
import ctypes as C
import os

import numpy as np
import pytest
import torch

from tests import batches_ref as ref
from tests.test_batches_host import VARIANTS, golden_bank

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ONE_BELOW = 1.0 - 2.0 ** -53
EINVAL, ESTATE = -1, -4


@pytest.fixture(scope="module")
def renderer():
    from posegen_amd import surreal_config
    from posegen_amd.raycaster import HipRenderer
    r = HipRenderer(surreal_config(), device=DEV)          # no weights loaded: the batch entry points need none
    yield r
    r.close()


@pytest.fixture(scope="module")
def golden():
    return dict(np.load(os.path.join(REPO, "tests", "golden", "train_batches.npz")))


def _p(t):
    return None if t is None else C.c_void_p(t.data_ptr())


def _i32(a):
    return a.ctypes.data_as(C.POINTER(C.c_int32))


def device_index(r, masks: torch.Tensor):
    """(counts host int64 [F], start device [F + 1], ids device) of device masks [F,P] through the two index entry points."""
    F, P = masks.shape
    counts = torch.full((F,), -7, dtype=torch.int64, device=DEV)
    r._check(r.lib.pg_pixel_index_count(r.handle, r._stream(), _p(masks), F, P, _p(counts)))
    start = torch.zeros(F + 1, dtype=torch.int64, device=DEV)
    torch.cumsum(counts, 0, out=start[1:])
    host = counts.cpu().numpy()
    total = int(host.sum())
    ids = torch.full((total + 8,), -7, dtype=torch.int32, device=DEV)
    r._check(r.lib.pg_pixel_index_emit(r.handle, r._stream(), _p(masks), F, P, _p(start), total, _p(ids)))
    assert (ids[total:] == -7).all()                       # nothing past the total
    return host, start, ids[:total]


def device_sample(r, counts, start, ids, rows, k, draws):
    rows = np.ascontiguousarray(rows, dtype=np.int32)
    d = torch.from_numpy(np.ascontiguousarray(draws, dtype=np.float64)).to(DEV)
    pix = torch.full((len(rows) * k + 8,), -7, dtype=torch.int32, device=DEV)
    r._check(r.lib.pg_batch_sample_pixels(r.handle, r._stream(), _p(ids), _p(start), counts.ctypes.data_as(C.POINTER(C.c_int64)),
                                          len(counts), _i32(rows), len(rows), k, _p(d), _p(pix)))
    out = pix.cpu().numpy()
    assert (out[len(rows) * k:] == -7).all()
    return out[:len(rows) * k].reshape(len(rows), k)


def assert_batch_equals_restatement(batch, want):
    for name in ("target_s", "fgs", "rays_o", "rays_d", "rays", "pixel_idxs"):
        got = batch[name].cpu().numpy()
        assert got.dtype == want[name].dtype and got.shape == want[name].shape, name
        assert np.array_equal(got, want[name]), name
    assert ("bgs" in batch) == ("bgs" in want)
    if "bgs" in want:
        assert np.array_equal(batch["bgs"].cpu().numpy(), want["bgs"])
    rb = batch["ray_batch"].cpu().numpy()
    assert rb.dtype == np.float32 and np.array_equal(rb[:, :8], want["ray_batch"][:, :8])
    d = want["rays_d"].astype(np.float64)
    unit = d / np.linalg.norm(d, axis=-1, keepdims=True)
    ulps = np.abs(rb[:, 8:].astype(np.float64) - unit) / np.spacing(np.abs(unit).astype(np.float32)).astype(np.float64)
    print(f"view directions: {ulps.max():.2f} ulps from the float64 normalisation")
    assert ulps.max() <= 4


# ---- the pixel index -------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("P", [1, 63, 64, 65, 257, 4097])
def test_pixel_index_is_np_where_of_every_image(renderer, P):
    rng = np.random.default_rng(P)
    masks = np.zeros((3, P), np.uint8)
    masks[0] = np.where(rng.random(P) < 0.5, rng.choice([1, 255], P), 0)     # bytes 1 and 255; the middle image empty; one full
    masks[0, -1] = 255
    masks[2] = 1
    want_counts, want_start, want_ids = ref.pixel_index(masks)
    counts, start, ids = device_index(renderer, torch.from_numpy(masks).to(DEV))
    assert counts.dtype == np.int64 and np.array_equal(counts, want_counts) and counts[1] == 0 and counts[2] == P
    assert np.array_equal(start.cpu().numpy(), want_start)
    assert np.array_equal(ids.cpu().numpy(), want_ids)


def test_pixel_index_over_many_tiles_and_images(renderer):
    rng = np.random.default_rng(0)
    masks = (rng.random((37, 3 * 4096 + 5)) < 0.3).astype(np.uint8)          # several tiles per image, the last one partial
    masks[5] = 0
    want_counts, want_start, want_ids = ref.pixel_index(masks)
    m = torch.from_numpy(masks).to(DEV)
    counts, start, ids = device_index(renderer, m)
    assert np.array_equal(counts, want_counts) and np.array_equal(ids.cpu().numpy(), want_ids)
    again = device_index(renderer, m)[2]
    assert torch.equal(ids, again)


# ---- the sampler -----------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("k", [1, 2, 63, 64, 65, 1024])
def test_sampler_equals_floyd_at_the_draws(renderer, k):
    """images with k, k + 1 and 2^20 valid pixels; random draws, one image twice, and the draws all 0 and all 1 - 2^-53"""
    P = 1 << 20
    rng = np.random.default_rng(k)
    masks = np.zeros((3, P), np.uint8)
    masks[0, rng.choice(P, k, replace=False)] = 255
    masks[1, rng.choice(P, k + 1, replace=False)] = 1
    masks[2] = 1
    counts, start, ids = device_index(renderer, torch.from_numpy(masks).to(DEV))
    assert list(counts) == [k, k + 1, P]
    rows = np.array([0, 1, 2, 2, 0, 1, 2, 0, 1, 2])
    draws = rng.random((len(rows), k))
    draws[4:7], draws[7:10] = 0.0, ONE_BELOW
    got = device_sample(renderer, counts, start, ids, rows, k, draws)
    want = ref.sample_pixels(counts, *ref.pixel_index(masks)[1:], rows, k, draws)
    assert np.array_equal(got, want)
    assert np.array_equal(got[0], np.where(masks[0])[0])                     # count == k: every valid pixel
    assert (np.diff(got, axis=1) > 0).all() if k > 1 else True
    assert k == 1 or not np.array_equal(got[2], got[3])                     # one image twice: independent rows
    for a, img in enumerate(rows):
        assert (masks[img, got[a]] > 0).all()


@pytest.mark.parametrize("n_img", [1, 300])
def test_sampler_over_more_workgroups_than_compute_units(renderer, n_img):
    rng = np.random.default_rng(n_img)
    masks = (rng.random((5, 1000)) < 0.2).astype(np.uint8)
    counts, start, ids = device_index(renderer, torch.from_numpy(masks).to(DEV))
    rows, k = rng.integers(0, 5, n_img), 12
    draws = rng.random((n_img, k))
    got = device_sample(renderer, counts, start, ids, rows, k, draws)
    assert np.array_equal(got, ref.sample_pixels(counts, start.cpu().numpy(), ids.cpu().numpy(), rows, k, draws))
    assert np.array_equal(got, device_sample(renderer, counts, start, ids, rows, k, draws))


# ---- the gather ------------------------------------------------------------------------------------------------------------------

def _poses(g):
    return {k: torch.from_numpy(g[f"in_{k}"]).to(DEV) for k in ("kp3d", "bones", "skts", "cyls")}


def _device_bank(renderer, bank, **over):
    from posegen_amd import DeviceImageBank
    b = dict(bank, **over)
    return DeviceImageBank(renderer, b["imgs"], b["masks"], b["sampling_masks"], b["c2ws"], b["focals"], b["HW"], bkgds=b.get("bkgds"),
                           bkgd_idxs=b.get("bkgd_idxs") if b.get("bkgds") is not None else None, centers=b.get("centers"),
                           mask_img=b.get("mask_img", False))


@pytest.mark.parametrize("variant", VARIANTS)
def test_gather_of_the_golden_batches(renderer, golden, variant):
    """plain: scalar focals, no centres; centers: (fx, fy) focals and per-image centres; mask_img"""
    from posegen_amd import RayBatchSource
    g = golden
    bank = golden_bank(g, variant)
    dbank = _device_bank(renderer, bank)
    counts, start, ids = ref.pixel_index(bank["sampling_masks"])
    assert np.array_equal(dbank.counts, counts) and np.array_equal(dbank.ids.cpu().numpy()[:dbank.total], ids)
    assert dbank.nbytes > bank["imgs"].nbytes
    k = int(g["k_pixels"])
    src = RayBatchSource(dbank, k * int(g["n_images"]), int(g["n_images"]), poses=_poses(g))
    for b in range(3):
        key = lambda name: g[f"{variant}_b{b}_{name}"]
        items, pix = key("items"), key("pixel_idxs")
        batch = src.gather(items, pix)
        assert_batch_equals_restatement(batch, ref.gather(bank, items, pix))
        # and the reference's batch itself: keys, shapes, dtypes, values (rays_d / rays: float64 there, bounded on the host side)
        for name in ("target_s", "fgs", "bgs", "rays_o", "kp_idx", "cam_idxs", "kp3d", "bones", "skts", "cyls"):
            got = batch[name].cpu().numpy()
            assert got.dtype == key(name).dtype and got.shape == key(name).shape, name
            assert np.array_equal(got, key(name)), name
        assert batch["rays"].shape == key("rays").shape and batch["rays_d"].shape == key("rays_d").shape
        prefix = f"{variant}_b{b}_"
        theirs = {name[len(prefix):] for name in g if name.startswith(prefix)} - {"items", "pixel_idxs"}     # (those two: the tool's)
        assert set(batch) == theirs | {"ray_batch", "pixel_idxs", "img_idxs"}
        assert np.array_equal(batch.kp_idx_host, key("kp_idx")) and batch.kp_idx_host.dtype == np.int64
        assert np.array_equal(batch["img_idxs"].cpu().numpy(), items)
        assert all(t.device == torch.device(DEV) for t in batch.values())


def test_gather_without_backgrounds_at_the_frame_corners_and_through_item_maps(renderer, golden):
    from posegen_amd import RayBatchSource
    bank = golden_bank(golden, "centers")
    H, W = bank["HW"]
    nobg = dict(bank, bkgds=None, bkgd_idxs=None, mask_img=True)            # mask_img without backgrounds changes nothing
    src = RayBatchSource(_device_bank(renderer, nobg), 8, 4)
    items = np.array([0, 3, 3, 5])
    pix = np.array([[0, H * W - 1], [W - 1, W], [0, 1], [H * W - 2, H * W - 1]])     # first and last pixel of a frame
    batch = src.gather(items, pix)
    assert "bgs" not in batch and "kp3d" not in batch
    assert_batch_equals_restatement(batch, ref.gather(nobg, items, pix))
    # items: image, camera, pose rows and the two indices each from a map of its own
    maps = {"img_row": np.array([5, 4, 0]), "cam_row": np.array([1, 1, 2]), "pose_row": np.array([2, 0, 0]),
            "kp_idx": np.array([10, 11, 12]), "cam_idx": np.array([7, 7, 9])}
    tv = np.array([1, 1, 0])
    src = RayBatchSource(_device_bank(renderer, bank), 9, 3, poses=_poses(golden), items=maps, temp_validity=tv)
    q = np.array([2, 0, 1])
    pix = np.array([[3, 4, 200], [0, 7, 8], [1, 2, 279]])
    batch = src.gather(q, torch.from_numpy(pix).to(DEV))
    assert_batch_equals_restatement(batch, ref.gather(bank, maps["img_row"][q], pix, cam_rows=maps["cam_row"][q]))
    per_ray = np.repeat(q, 3)
    assert np.array_equal(batch["kp_idx"].cpu().numpy(), maps["kp_idx"][per_ray])
    assert np.array_equal(batch["cam_idxs"].cpu().numpy(), maps["cam_idx"][per_ray])
    assert np.array_equal(batch["skts"].cpu().numpy(), golden["in_skts"][maps["pose_row"][per_ray]])
    want_tv = ((tv + np.roll(tv, -1)) // 2).astype(np.float32)[per_ray]
    assert batch["temp_val"].dtype == torch.float32 and np.array_equal(batch["temp_val"].cpu().numpy(), want_tv)


def test_the_row_ring_wraps_and_regrows_under_consecutive_gathers(golden):
    """Ten pg_batch_gather calls in a row on a fresh renderer, nothing waited for in between: more than the ring's 8 slots, so
    calls 8 and 9 reuse the slots of calls 0 and 1.  n_img = 40 first meets an empty slot (call 2), then the slot call 0 sized
    for n_img = 2 (call 8: 120 words against the 73 it holds), which is freed and allocated again."""
    from posegen_amd import RayBatchSource, surreal_config
    from posegen_amd.raycaster import HipRenderer
    bank = golden_bank(golden, "centers")
    F, P = bank["imgs"].shape[0], bank["imgs"].shape[1]
    r = HipRenderer(surreal_config(), device=DEV)
    try:
        src = RayBatchSource(_device_bank(r, bank), 5, 1)
        rng = np.random.default_rng(8)
        calls = []
        for n_img in (2, 2, 40, 2, 2, 2, 2, 2, 40, 2):
            items, pix = rng.integers(0, F, n_img), rng.integers(0, P, (n_img, 5))
            calls.append((items, pix, src.gather(items, pix)))
        assert len(calls) > 8
        for items, pix, batch in calls:
            assert_batch_equals_restatement(batch, ref.gather(bank, items, pix))
    finally:
        r.close()


def test_sampled_batches_equal_the_restatement_at_the_same_draws(renderer, golden):
    from posegen_amd import RayBatchSource
    bank = golden_bank(golden, "plain")
    dbank = _device_bank(renderer, bank)
    k = 6
    src = RayBatchSource(dbank, 4 * k, 4, poses=_poses(golden), generator=torch.Generator(device=DEV).manual_seed(3))
    twin = torch.Generator(device=DEV).manual_seed(3)
    counts, start, ids = ref.pixel_index(bank["sampling_masks"])
    torch.manual_seed(11)
    want_items = ref.image_batches(6, 4, 3)
    torch.manual_seed(11)
    for step, batch in zip(range(3), src):
        draws = torch.rand(4, k, dtype=torch.float64, device=DEV, generator=twin).cpu().numpy()
        items = batch["img_idxs"].cpu().numpy()
        assert np.array_equal(items, want_items[step])
        pix = ref.sample_pixels(counts, start, ids, items, k, draws)
        assert_batch_equals_restatement(batch, ref.gather(bank, items, pix))


# ---- 64-bit addressing -----------------------------------------------------------------------------------------------------------

def test_the_last_image_of_a_bank_beyond_4_gb(renderer):
    from posegen_amd import DeviceImageBank, RayBatchSource
    F, H, W = 1400, 1024, 1024
    P = H * W
    rng = np.random.default_rng(64)
    last = {"imgs": rng.integers(0, 256, (1, P, 3), dtype=np.uint8), "masks": rng.integers(0, 2, (1, P, 1), dtype=np.uint8),
            "sampling_masks": (rng.random((1, P)) < 0.25).astype(np.uint8), "HW": (H, W),
            "c2ws": golden_c2w(), "focals": np.array([900.0], np.float32)}
    imgs = torch.empty((F, P, 3), dtype=torch.uint8, device=DEV)             # 4.4 GB: row F - 1 starts past 2^32 bytes
    masks = torch.empty((F, P, 1), dtype=torch.uint8, device=DEV)
    sampling = torch.zeros((F, P), dtype=torch.uint8, device=DEV)
    imgs[-1], masks[-1], sampling[-1] = (torch.from_numpy(last[n][0]).to(DEV) for n in ("imgs", "masks", "sampling_masks"))
    assert (F - 1) * P * 3 > 2 ** 32
    bank = DeviceImageBank(renderer, imgs, masks, sampling, last["c2ws"], last["focals"], (H, W))
    assert bank.imgs.data_ptr() == imgs.data_ptr() and bank.sampling_masks.data_ptr() == sampling.data_ptr()      # adopted
    counts, start, ids = ref.pixel_index(last["sampling_masks"])
    assert bank.counts[-1] == counts[0] and bank.total == counts[0] and not bank.counts[:-1].any()
    k = 16
    src = RayBatchSource(bank, k, 1, items={"img_row": np.array([F - 1]), "cam_row": np.array([0])},
                         generator=torch.Generator(device=DEV).manual_seed(9))
    batch = src.sample([0])
    draws = torch.rand(1, k, dtype=torch.float64, device=DEV, generator=torch.Generator(device=DEV).manual_seed(9)).cpu().numpy()
    pix = ref.sample_pixels(counts, start, ids, [0], k, draws)
    assert_batch_equals_restatement(batch, ref.gather(last, [0], pix))
    del bank, src, batch, imgs, masks, sampling
    torch.cuda.empty_cache()


def golden_c2w():
    c2w = np.eye(4, dtype=np.float32)[None].copy()
    c, s = np.float32(np.cos(0.3)), np.float32(np.sin(0.3))
    c2w[0, :3, :3] = [[c, 0, s], [0, 1, 0], [-s, 0, c]]
    c2w[0, :3, 3] = [0.1, -0.2, 2.5]
    return c2w


# ---- refusals --------------------------------------------------------------------------------------------------------------------

def test_bad_arguments_are_einval_and_leave_the_outputs_untouched(renderer):
    from posegen_amd import _ffi
    r, lib = renderer, renderer.lib
    F, H, W = 3, 5, 4
    P = H * W
    masks = torch.ones((F, P), dtype=torch.uint8, device=DEV)
    counts, start, ids = device_index(r, masks)
    sentinel_i = lambda n: torch.full((n,), -7, dtype=torch.int32, device=DEV)
    sentinel_f = lambda *s: torch.full(s, -7.0, device=DEV)
    cnt = torch.full((F,), -7, dtype=torch.int64, device=DEV)
    st = r._stream
    # the index
    assert lib.pg_pixel_index_count(r.handle, st(), None, F, P, _p(cnt)) == EINVAL
    assert lib.pg_pixel_index_count(r.handle, st(), _p(masks), 0, P, _p(cnt)) == EINVAL
    assert lib.pg_pixel_index_count(r.handle, st(), _p(masks), F, 0, _p(cnt)) == EINVAL
    assert lib.pg_pixel_index_count(r.handle, st(), _p(masks), F, P, None) == EINVAL
    out_ids = sentinel_i(F * P)
    assert lib.pg_pixel_index_emit(r.handle, st(), _p(masks), F, P, None, F * P, _p(out_ids)) == EINVAL
    assert lib.pg_pixel_index_emit(r.handle, st(), _p(masks), F, -1, _p(start), F * P, _p(out_ids)) == EINVAL
    assert lib.pg_pixel_index_emit(r.handle, st(), _p(masks), F - 1, P, _p(start), F * P, _p(out_ids)) == ESTATE   # not the count's F
    # the sampler
    k = 4
    draws = torch.rand(2, 1024, dtype=torch.float64, device=DEV)
    pix = sentinel_i(2 * 1025)
    c64 = lambda a: a.ctypes.data_as(C.POINTER(C.c_int64))
    rows = lambda *a: _i32(np.array(a, np.int32))
    sample = lambda ids_=ids, start_=start, counts_=counts, F_=F, rows_=rows(0, 2), n=2, k_=k, draws_=draws, pix_=pix: \
        lib.pg_batch_sample_pixels(r.handle, st(), _p(ids_), _p(start_), None if counts_ is None else c64(counts_), F_, rows_, n, k_,
                                   _p(draws_), _p(pix_))
    assert sample(k_=0) == EINVAL and sample(k_=1025) == EINVAL and sample(k_=-3) == EINVAL
    assert sample(rows_=rows(0, F)) == EINVAL and sample(rows_=rows(-1, 0)) == EINVAL
    assert sample(draws_=None) == EINVAL and sample(ids_=None) == EINVAL and sample(counts_=None) == EINVAL and sample(rows_=None) == EINVAL
    assert sample(pix_=None) == EINVAL and sample(F_=0) == EINVAL
    assert sample(k_=P + 1) == EINVAL                                        # more than the image has
    few = counts.copy()
    few[2] = k - 1
    assert sample(counts_=few) == EINVAL
    assert b"valid pixels" in lib.pg_last_error(r.handle)
    # the gather
    n = 2 * k
    outs = dict(target=sentinel_f(n, 3), fgs=sentinel_f(n, 1), bgs=sentinel_f(n, 3), o=sentinel_f(n, 3), d=sentinel_f(n, 3), rb=sentinel_f(n, 11))
    imgs = torch.zeros((F, P, 3), dtype=torch.uint8, device=DEV)
    bk = torch.zeros((2, P, 3), dtype=torch.uint8, device=DEV)
    c2ws, focals = torch.zeros(F, 3, 4, device=DEV), torch.ones(F, 2, device=DEV)
    bkgd_idxs = np.array([0, 1, 1], np.int32)
    gpix = torch.zeros(n, dtype=torch.int32, device=DEV)

    def struct(**over):
        f = dict(imgs=imgs.data_ptr(), masks=masks.data_ptr(), bkgds=bk.data_ptr(), bkgd_idxs=_i32(bkgd_idxs), c2ws=c2ws.data_ptr(),
                 focals=focals.data_ptr(), centers=None, F=F, P=P, n_bkgd=2, n_cam=F, H=H, W=W, mask_img=0)
        f.update(over)
        return _ffi.PgImageBank(**f)

    def gather(bank=None, rows_=rows(0, 2), cams=None, n_img=2, k_=k, pix_=gpix, **over):
        o = dict({name: _p(t) for name, t in outs.items()}, **over)
        b = struct() if bank is None else bank
        return lib.pg_batch_gather(r.handle, st(), C.byref(b), rows_, cams, n_img, k_, _p(pix_), o["target"], o["fgs"], o["bgs"], o["o"],
                                   o["d"], o["rb"])

    assert gather(k_=0) == EINVAL and gather(k_=1025) == EINVAL
    assert gather(rows_=rows(0, F)) == EINVAL and gather(rows_=rows(-1, 1)) == EINVAL and gather(cams=rows(0, F)) == EINVAL
    assert gather(rows_=None) == EINVAL and gather(pix_=None) == EINVAL and gather(target=None) == EINVAL and gather(rb=None) == EINVAL
    assert gather(bank=struct(imgs=None)) == EINVAL and gather(bank=struct(focals=None)) == EINVAL
    assert gather(bank=struct(P=0)) == EINVAL and gather(bank=struct(F=0)) == EINVAL and gather(bank=struct(H=H + 1)) == EINVAL
    bad = np.array([0, 1, 2], np.int32)                                      # image 2's background is outside the bank of 2
    assert gather(bank=struct(bkgd_idxs=_i32(bad))) == EINVAL
    assert b"bkgd_idxs" in lib.pg_last_error(r.handle)
    assert gather(bank=struct(bkgd_idxs=_i32(np.array([0, 1, -1], np.int32)))) == EINVAL
    assert gather(bank=struct(bkgds=None)) == EINVAL                         # bgs asked for from a bank without backgrounds
    torch.cuda.synchronize()
    assert (cnt == -7).all() and (out_ids == -7).all() and (pix == -7).all()
    for t in outs.values():
        assert (t == -7).all()
    # and the calls are fine once the arguments are
    assert sample() == 0 and gather() == 0
    torch.cuda.synchronize()
    assert (pix[:2 * k] >= 0).all() and (pix[2 * k:] == -7).all() and not (outs["rb"] == -7).any()


# ---- repeatability and the training step ------------------------------------------------------------------------------------------

def test_two_sources_with_equal_seeds_give_equal_bytes(renderer, golden):
    from posegen_amd import RayBatchSource
    bank = golden_bank(golden, "mask_img")
    dbank = _device_bank(renderer, bank)
    runs = []
    for _ in range(2):
        torch.manual_seed(21)
        src = RayBatchSource(dbank, 24, 4, poses=_poses(golden), generator=torch.Generator(device=DEV).manual_seed(5))
        runs.append([{k: v.cpu().numpy().tobytes() for k, v in batch.items()} for _, batch in zip(range(5), src)])
    assert len(runs[0]) == 5 and runs[0] == runs[1]
    assert len({b["pixel_idxs"] for b in runs[0]}) == 5                      # and the steps differ from each other


def test_a_training_step_on_a_batch_of_the_source(renderer):
    """4 images, 8 pixels each: the gradients of one step on the source's tensors are bitwise those of the same step on clones"""
    from oracle import anerf_oracle as orc
    from posegen_amd import DeviceImageBank, RayBatchSource, surreal_config, synthetic as syn
    from posegen_amd.raycaster import HipRayCaster, make_training_draws
    from posegen_amd.train import TrainableRayCaster
    from tests.helpers import loss_of, model_for
    cfg = surreal_config(n_samples=32, n_importance=16)
    wc, wf, tv, td = model_for(cfg, 4)
    H = W = 32
    F = 4
    _, kps, skts = syn.make_pose(1, 1)
    c2ws, focals = syn.make_camera(1, H, W)
    _, _, cyls, _ = orc.valid_rays(torch.tensor(c2ws), H, W, focals, torch.tensor(kps), cfg.ext_scale)
    rng = np.random.default_rng(1)
    caster = HipRayCaster.from_weights(cfg, wc, wf, float(tv), float(td), device=DEV, precision="fp32")
    bank = DeviceImageBank(caster.renderer, rng.integers(0, 256, (F, H * W, 3), dtype=np.uint8), np.ones((F, H * W, 1), np.uint8),
                           np.ones((F, H * W), np.uint8), np.repeat(np.asarray(c2ws, np.float32)[:1], F, 0),
                           np.repeat(np.asarray(focals, np.float32).reshape(1, -1), F, 0), (H, W))
    rep = lambda a, tail: torch.tensor(np.asarray(a, np.float32)).reshape((1,) + tail).repeat(F, *([1] * len(tail))).to(DEV)
    poses = {"kp3d": rep(kps, (24, 3)), "bones": torch.zeros(F, 24, 3, device=DEV), "skts": rep(skts, (24, 4, 4)),
             "cyls": rep(np.asarray(cyls), (5,))}
    src = RayBatchSource(bank, 32, F, poses=poses, generator=torch.Generator(device=DEV).manual_seed(2))
    torch.manual_seed(0)
    batch = next(iter(src))
    n = batch["ray_batch"].shape[0]
    assert n == 32
    draws = {k: v.to(DEV) for k, v in make_training_draws(n, 32, 16, perturb=1., raw_noise_std=1., ray_noise_std=0., pytest=True).items()}
    m = TrainableRayCaster(caster, train_precision="fp32")
    m.train()

    def step(rb, skts_, cyls_, cams, target):
        m.zero_grad(set_to_none=True)
        out = m(rb, N_samples=32, skts=skts_, cyls=cyls_, cams=cams, N_importance=16, draws=draws)
        loss_of(out, target).backward()
        return {f"{tag}.{k}": p.grad.clone() for tag, net in (("coarse", m.network), ("fine", m.network_fine))
                for k, p in net.named_parameters() if p.grad is not None}

    cams = batch["cam_idxs"].float()
    mine = step(batch["ray_batch"], batch["skts"], batch["cyls"], cams, batch["target_s"])
    outside = [t.detach().cpu().clone().to(DEV) for t in (batch["ray_batch"], batch["skts"], batch["cyls"], cams, batch["target_s"])]
    theirs = step(*outside)
    assert mine.keys() == theirs.keys() and len(mine) >= 24
    assert any(bool(g.any()) for g in mine.values()), "the step has gradients"
    for k in mine:
        assert torch.equal(mine[k], theirs[k]), k
    caster.renderer.close()
