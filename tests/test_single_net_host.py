"""Single-net A-NeRF models (single_net, multires_views = 0) on the host side: configuration, the widening of the
0-band view weight where weights enter the library, the C ABI, and the importance-sampling rule the composite kernel
implements (is_only, core/utils/ray_utils.py:255-289), pinned on the reference's own fixtures.  No GPU needed."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from posegen_amd import _ffi, synthetic as syn
from posegen_amd.config import (PREC_BF16, PREC_BF16X3, PREC_FP16, PREC_FP16C, PREC_FP32, RenderConfig,
                                surreal_config, surreal_single_config)
from posegen_amd.raycaster import NET_TENSOR_ORDER

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(REPO, "tests", "golden")
NEW_FIXTURES = ("rays_single", "rays_single_v4", "rays_views0", "rays_single_train")


def _lib():
    try:
        return _ffi.load_library()
    except _ffi.HipLibraryError as e:
        pytest.fail(f"library missing: {e} (run __graft_entry__.build())")


def _golden(name):
    return dict(np.load(os.path.join(GOLDEN, f"{name}.npz"), allow_pickle=False))


# ---- configuration ----------------------------------------------------------------------------------------------------

def test_render_config_defaults_are_the_two_net_model():
    c = RenderConfig()
    assert c.single_net is False and c.multires_views == 4
    assert (c.n_samples, c.n_importance) == (64, 16)
    assert c.evals_per_ray() == 64 + 80
    assert RenderConfig(n_importance=0).evals_per_ray() == 64


def test_surreal_single_config_is_surreal_single_txt():
    # configs/surreal/surreal_single.txt: single_net = True, multires_views = 0, multires = 7, netwidth 256,
    # N_samples = 96, N_importance = 48, chunk = 4096, ext_scale = 0.001
    c = surreal_single_config()
    assert c.single_net is True
    assert (c.multires, c.multires_views, c.multires_bones) == (7, 0, 0)
    assert (c.net_depth, c.net_width, c.framecode_ch) == (8, 256, 0)
    assert (c.n_samples, c.n_importance, c.chunk) == (96, 48, 4096)
    assert c.ext_scale == 0.001 and c.cutoff_mm == 500.0
    assert c.ch_d == 72 and c.ch_view_in == 256 + 72
    assert c.evals_per_ray() == 96 + 48          # the fine pass evaluates only the new points
    assert surreal_config(single_net=True).evals_per_ray() == 64 + 16


# ---- the widening of the multires_views = 0 view weight -----------------------------------------------------------------

def _widen_np(vw, fc):
    out = np.zeros((128, 256 + 648 + fc), np.float32)
    out[:, :256 + 72] = vw[:, :256 + 72]
    out[:, 256 + 648:] = vw[:, 256 + 72:]
    return out


def _arrays(w):
    arrs = [np.ascontiguousarray(w[k], dtype=np.float32) for k in NET_TENSOR_ORDER]
    ptrs = (C.c_void_p * 24)(*[a.ctypes.data for a in arrs])
    shp = (C.c_int64 * 48)()
    for i, a in enumerate(arrs):
        shp[2 * i], shp[2 * i + 1] = a.shape[0], (a.shape[1] if a.ndim == 2 else 1)
    return arrs, ptrs, shp


def _pack(lib, w, fc, prec, fact):
    keep, ptrs, shp = _arrays(w)
    size, chunk = C.c_int64(), C.c_int32()
    assert lib.pg_debug_pack(ptrs, shp, 24, fc, prec, fact, None, 0, C.byref(size), None, C.byref(chunk)) == 0, lib.pg_last_error(None)
    buf = np.zeros(size.value, np.uint8)
    bias = np.zeros(82 * 32 * 4, np.float32)
    assert lib.pg_debug_pack(ptrs, shp, 24, fc, prec, fact, buf.ctypes.data, size.value, C.byref(size), bias.ctypes.data,
                             C.byref(chunk)) == 0, lib.pg_last_error(None)
    return buf, bias


def _pack_map(lib, w, fc, form):
    keep, ptrs, shp = _arrays(w)
    mn, sn = C.c_int64(), C.c_int64()
    assert lib.pg_debug_pack_map(ptrs, shp, 24, fc, form, None, 0, C.byref(mn), None, 0, C.byref(sn)) == 0, lib.pg_last_error(None)
    m = np.zeros(mn.value, np.int32)
    src = np.zeros(sn.value, np.float32)
    assert lib.pg_debug_pack_map(ptrs, shp, 24, fc, form, m.ctypes.data, mn.value, C.byref(mn), src.ctypes.data, sn.value,
                                 C.byref(sn)) == 0, lib.pg_last_error(None)
    return m, src


def _pack_vy(lib, w, fc, prec):
    keep, ptrs, shp = _arrays(w)
    n = C.c_int64()
    assert lib.pg_debug_pack_vy(ptrs, shp, 24, fc, prec, None, 0, C.byref(n)) == 0, lib.pg_last_error(None)
    vy = np.zeros(n.value, np.uint8)
    assert lib.pg_debug_pack_vy(ptrs, shp, 24, fc, prec, vy.ctypes.data, n.value, C.byref(n)) == 0, lib.pg_last_error(None)
    return vy


def _views0_weights(fc):
    cfg = surreal_single_config(framecode_ch=fc, n_framecodes=8 if fc else 0)
    w = syn.make_weights(cfg, 3)
    assert w["views_linears.0.weight"].shape == (128, 256 + 72 + fc)
    wide = dict(w)
    wide["views_linears.0.weight"] = _widen_np(w["views_linears.0.weight"], fc)
    return w, wide


@pytest.mark.parametrize("fc", [0, 16])
def test_widen_entry_point_is_the_hand_widened_matrix(fc):
    lib = _lib()
    w, wide = _views0_weights(fc)
    vw = np.ascontiguousarray(w["views_linears.0.weight"])
    n = C.c_int64()
    assert lib.pg_debug_widen_views(vw.ctypes.data, 128, vw.shape[1], fc, None, 0, C.byref(n)) == 0
    assert n.value == 128 * (256 + 648 + fc)
    out = np.full(n.value, np.nan, np.float32)
    assert lib.pg_debug_widen_views(vw.ctypes.data, 128, vw.shape[1], fc, out.ctypes.data, n.value, C.byref(n)) == 0
    assert out.reshape(128, -1).tobytes() == wide["views_linears.0.weight"].tobytes()
    # a 4-band matrix is not a 0-band one
    wv = np.zeros((128, 256 + 648 + fc), np.float32)
    assert lib.pg_debug_widen_views(wv.ctypes.data, 128, wv.shape[1], fc, out.ctypes.data, n.value, C.byref(n)) == _ffi.PG_EINVAL


@pytest.mark.parametrize("fc", [0, 16])
@pytest.mark.parametrize("prec,fact", [(PREC_FP32, 0), (PREC_BF16X3, 0), (PREC_BF16, 0), (PREC_BF16, 1), (PREC_BF16, 3),
                                       (PREC_FP16, 1), (PREC_FP16C, 0), (PREC_FP16C, 4)])
def test_views0_pack_is_byte_identical_to_the_widened_pack(fc, prec, fact):
    """The packed streams and bias tables of a multires_views = 0 net are those of the 4-band net whose view weight is
    the hand-widened matrix: what the kernels see is exactly the 4-band layout with zero sin/cos weights."""
    lib = _lib()
    w, wide = _views0_weights(fc)
    b0, bias0 = _pack(lib, w, fc, prec, fact)
    b1, bias1 = _pack(lib, wide, fc, prec, fact)
    assert b0.size == b1.size and b0.tobytes() == b1.tobytes()
    assert bias0.tobytes() == bias1.tobytes()
    if fact == 1:
        assert _pack_vy(lib, w, fc, prec).tobytes() == _pack_vy(lib, wide, fc, prec).tobytes()


@pytest.mark.parametrize("fc", [0, 16])
@pytest.mark.parametrize("form", [0, 1, 2])
def test_views0_source_maps_are_those_of_the_widened_net(fc, form):
    """pg_load_weights_device re-forms the images from these maps and the flat source vector: both are the 4-band ones."""
    lib = _lib()
    w, wide = _views0_weights(fc)
    m0, s0 = _pack_map(lib, w, fc, form)
    m1, s1 = _pack_map(lib, wide, fc, form)
    assert m0.tobytes() == m1.tobytes()
    assert s0.tobytes() == s1.tobytes()


# ---- the C ABI --------------------------------------------------------------------------------------------------------

def test_abi_version_11_and_the_single_net_field():
    lib = _lib()
    hdr = open(os.path.join(REPO, "include", "posegen_hip.h")).read()
    assert re.search(r"#define PG_ABI_VERSION 11\b", hdr)
    assert _ffi.PG_ABI_VERSION == 11 and lib.pg_abi_version() == 11
    assert re.search(r"int32_t single_net;", hdr) and "reserved0" not in hdr
    # the field took reserved0's place: the layout is unchanged
    assert C.sizeof(_ffi.PgConfig) == 18 * 4
    assert _ffi.PgConfig.single_net.offset == 17 * 4
    assert "pg_debug_widen_views" in _ffi.PROTOTYPES and re.search(r"\bpg_debug_widen_views\s*\(", hdr)
    declared = set(re.findall(r"\b(pg_[a-z0-9_]+)\s*\(", hdr)) - {"pg_handle"}
    assert declared == set(_ffi.PROTOTYPES)
    for name in declared:
        assert hasattr(lib, name), name


# ---- the fixtures and the importance-sampling rule --------------------------------------------------------------------

@pytest.mark.parametrize("name", NEW_FIXTURES)
def test_new_fixtures_carry_their_keys(name):
    g = _golden(name)
    want = {"rays_single": (1, 0, 96, 48), "rays_single_v4": (1, 4, 64, 16), "rays_views0": (0, 0, 64, 16),
            "rays_single_train": (1, 0, 96, 48)}[name]
    assert (int(g["single_net"]), int(g["multires_views"]), int(g["n_samples"]), int(g["n_importance"])) == want
    n, S, N = int(g["n_rays"]), want[2], want[3]
    assert 48 <= n <= 96
    for k, shp in (("rgb_map", (n, 3)), ("acc_map", (n,)), ("rgb0", (n, 3)), ("acc0", (n,)), ("alpha", (n, S + N)),
                   ("alpha0", (n, S))):
        assert g[k].shape == shp, k
    if name == "rays_single_train":
        for k, shp in (("t_rand", (n, S)), ("u_rand", (n, N)), ("noise0", (n, S)), ("noise1", (n, S + N)),
                       ("ray_noise", (n, S + N, 3))):
            assert g[k].shape == shp, k
    else:
        for k, shp in (("z_coarse", (n, S)), ("weights0", (n, S)), ("z_fine", (n, S + N)), ("raw_coarse", (n, S, 4)),
                       ("raw_fine", (n, S + N, 4)), ("z_new", (n, N)), ("order", (n, S + N))):
            assert g[k].shape == shp, k
    assert os.path.getsize(os.path.join(GOLDEN, f"{name}.npz")) < 1 << 20


def _isample_np(z, w, N, is_only):
    """isample_from_lineseg + sample_pdf(det=True) restated in float32 numpy (ray_utils.py:157-201, 255-289)."""
    f = np.float32
    mids = f(0.5) * (z[:, 1:] + z[:, :-1])
    if is_only:
        wl, wk, wu = w[:, :-2], w[:, 1:-1], w[:, 2:]
        pw = f(0.5) * (np.maximum(wl, wk) + np.maximum(wk, wu)) + f(0.01)
    else:
        pw = w[:, 1:-1]
    pw = pw + f(1e-5)
    pdf = pw / pw.sum(-1, keepdims=True, dtype=np.float32)
    cdf = np.concatenate([np.zeros_like(pdf[:, :1]), np.cumsum(pdf, -1, dtype=np.float32)], -1)
    u = np.linspace(0., 1., N).astype(np.float32)
    out = np.empty((z.shape[0], N), np.float32)
    tol = np.empty((z.shape[0], N), np.float32)
    for r in range(z.shape[0]):
        inds = np.searchsorted(cdf[r], u, side="right")
        below = np.maximum(inds - 1, 0)
        above = np.minimum(inds, cdf.shape[1] - 1)
        c0, c1 = cdf[r, below], cdf[r, above]
        b0, b1 = mids[r, below], mids[r, above]
        den = c1 - c0
        small = den < 1e-5
        den = np.where(small, np.float32(1), den)
        out[r] = b0 + (u - c0) / den * (b1 - b0)
        # the documented tolerance rule: where the denominator is below (or within rounding of) the 1e-5 switch, or u lies
        # within rounding of a cdf value (u = 1 against a last cdf entry of 1 -+ an ulp: torch's and numpy's cumsum round
        # differently), the sample may take the other branch or the neighbouring bin: it is held to two bin widths there
        near = np.abs((c1 - c0) - 1e-5) < 1e-6
        on_step = np.abs(cdf[r][None, :] - u[:, None]).min(-1) < 1e-6
        bin_w = float(np.abs(np.diff(mids[r])).max())
        tol[r] = np.where(near | small | on_step, 2 * bin_w + 1e-6, 2e-5)
    return out, tol


@pytest.mark.parametrize("name", ["rays_single", "rays_single_v4", "rays_views0"])
def test_numpy_is_only_rule_reproduces_the_fixture_z_fine(name):
    """The spec of the composite kernel's importance samples, pinned on the reference's recorded z_fine."""
    g = _golden(name)
    S, N = int(g["n_samples"]), int(g["n_importance"])
    z, w = g["z_coarse"].astype(np.float32), g["weights0"].astype(np.float32)
    z_new, tol = _isample_np(z, w, N, bool(int(g["single_net"])))
    assert np.all(np.abs(z_new - g["z_new"]) <= tol), float(np.abs(z_new - g["z_new"]).max())
    merged = np.sort(np.concatenate([z, g["z_new"]], -1), -1, kind="stable")
    assert np.array_equal(merged, g["z_fine"])
    # the other rule does not reproduce it (the fixtures tell the two algorithms apart)
    other, _ = _isample_np(z, w, N, not bool(int(g["single_net"])))
    assert np.abs(other - g["z_new"]).max() > 1e-3
