"""The pose generator without a GPU: the float64 restatement (tests/generator_ref.py) against the reference's own numbers
(tests/golden/pose_generator.npz, written by tools/gen_golden_generator.py from run_gan.py's classes), its hand-written backward
against float64 autograd on the shipped spec and on the ragged toy spec, the modules' state-dict keys and shapes, the C ABI of
include/posegen_generator.h as the library exports it, and every refusal the header documents (the arguments are checked before the
handle is, so they are refused on a machine without a device too)."""
import ctypes as C
import os
import re

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from posegen_amd import _ffi, generators as gen
from tests import generator_ref as ref
from tests import stream_harness as sh

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = np.load(os.path.join(REPO, "tests", "golden", "pose_generator.npz"))
HEADER = os.path.join(REPO, "include", "posegen_generator.h")
COMPUTE = ("pg_gen_trunk_forward", "pg_gen_trunk_backward", "pg_gen_ba_head_forward", "pg_gen_ba_head_backward", "pg_gen_rt_head")


def _rel(a, b):
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    return float(np.max(np.abs(a - b)) / max(1.0, float(np.max(np.abs(b)))))


@pytest.fixture(scope="module")
def golden():
    module = gen.HipPoseGenerator()
    sd = ref.make_state_dict(module, int(GOLDEN["weight_seed"]))
    noise = {"ba": GOLDEN["noise_ba"], "r": GOLDEN["noise_r"], "eps": GOLDEN["eps"], "t": GOLDEN["noise_t"]}
    out, tapes, trunks = ref.pose_generator(sd, GOLDEN["x"], noise)
    return module, sd, noise, out, tapes, trunks


def test_the_stored_draws_come_from_the_stored_seed_in_the_references_order(golden):
    rng = np.random.RandomState(int(GOLDEN["noise_seed"]))
    assert [str(k) for k in GOLDEN["draw_order"]] == ["noise_ba", "noise_r", "eps", "noise_t"]
    for k, cols in (("noise_ba", 32), ("noise_r", 72), ("eps", 3), ("noise_t", 72)):
        assert np.array_equal(GOLDEN[k], rng.standard_normal((5, cols)).astype(np.float32))
    assert [str(k) for k in GOLDEN["restated"]] == ["pytorch3d.transforms.axis_angle_to_matrix"]


def test_the_restatement_equals_the_reference_forward(golden):
    _, sd, _, out, tapes, trunks = golden
    for k in ("pose_ba", "R", "T", "pose_rt"):
        assert out[k].shape == GOLDEN[k].shape and _rel(out[k], GOLDEN[k]) <= 1e-12, k
    after = {}
    for layers, tape in zip(trunks, tapes):
        for layer, t in zip(layers, tape):
            after[layer["names"][1] + ".running_mean"], after[layer["names"][1] + ".running_var"] = t["rm"], t["rv"]
    got = np.concatenate([after[str(k)] for k in GOLDEN["stat_keys"]])
    assert _rel(got, GOLDEN["stats_after"]) <= 1e-12
    assert np.all(GOLDEN["batches_tracked_after"] == 4)                       # 3 in the state dict, one training call


def test_the_restatement_equals_the_reference_backward(golden):
    _, sd, _, out, tapes, trunks = golden
    d = out["pose_ba"] - GOLDEN["target"].astype(np.float64)
    assert abs(0.5 * np.mean(d * d) - float(GOLDEN["loss"])) <= 1e-12 * max(1.0, float(GOLDEN["loss"]))
    grads = ref.pose_generator_backward(sd, out, tapes, trunks, d / d.size)
    pkeys = [str(k) for k in GOLDEN["param_keys"]]
    none = {k for k, n in zip(pkeys, GOLDEN["grad_none"]) if n}
    assert none == set(pkeys) - set(grads) and none == {k for k in pkeys if k.startswith("RTprocess.")}
    at = 0
    for i, k in enumerate(pkeys):
        idx = ref.grad_sample_index(int(np.prod(sd[k].shape)))
        if k in grads:
            g = grads[k]
            scale = max(1.0, float(GOLDEN["grad_abs_sum"][i]))
            assert abs(g.sum() - GOLDEN["grad_sum"][i]) <= 1e-12 * scale and abs(np.abs(g).sum() - GOLDEN["grad_abs_sum"][i]) <= 1e-12 * scale, k
            assert _rel(g.reshape(-1)[idx], GOLDEN["grad_samples"][at:at + len(idx)]) <= 1e-12, k
        else:
            assert np.all(np.isnan(GOLDEN["grad_samples"][at:at + len(idx)]))
        at += len(idx)
    assert at == GOLDEN["grad_samples"].size


def _autograd_trunk(layers, noise, d_out, slope, eps):
    """float64 autograd through torch's own batch_norm and leaky_relu"""
    params = [{k: torch.tensor(np.asarray(layer[k], np.float64), requires_grad=True) for k in ("w", "b", "gamma", "beta")} for layer in layers]
    h = torch.tensor(np.asarray(noise, np.float64))
    for p in params:
        h = F.leaky_relu(F.batch_norm(F.linear(h, p["w"], p["b"]), None, None, p["gamma"], p["beta"], True, 0.1, eps), slope)
    h.backward(torch.tensor(d_out))
    return h.detach().numpy(), [tuple(p[k].grad.numpy() for k in ("w", "b", "gamma", "beta")) for p in params]


@pytest.mark.parametrize("which", ["shipped", "toy"])
def test_the_hand_written_trunk_backward_equals_float64_autograd(which):
    spec = ref.shipped_spec() if which == "shipped" else ref.toy_spec()
    B = 5
    params, noise = ref.make_params(spec, 21), ref.make_noise(spec, B, 22)
    rng = np.random.RandomState(23)
    for t, layers in enumerate(params):
        d_out = rng.standard_normal((B, spec.trunks[t][1]))
        h, tape = ref.trunk_forward(layers, noise[t], spec.slope, spec.eps, spec.momentum)
        h_t, grads_t = _autograd_trunk(layers, noise[t], d_out, spec.slope, spec.eps)
        assert _rel(h, h_t) <= 1e-12
        for l, (mine, theirs) in enumerate(zip(ref.trunk_backward(layers, tape, d_out, spec.slope, spec.eps), grads_t)):
            for name, m, g in zip(("dw", "db", "dgamma", "dbeta"), mine, theirs):
                scale = max(1.0, float(np.max(np.abs(g))))
                if name == "db":
                    # (zero in exact arithmetic: held to the scale of the sums it is the difference of)
                    scale = max(scale, float(np.abs(tape[l]["scale"]).max() * np.abs(d_out).sum()))
                assert np.max(np.abs(m - g)) <= 1e-12 * scale, (t, l, name)


def test_the_hand_written_head_backward_equals_float64_autograd():
    rng = np.random.RandomState(31)
    B, J, W = 5, 24, 40
    h, (w2, b2), g = rng.standard_normal((B, W)), ref.make_head(4 * J, W, rng), rng.standard_normal((B, J, 3))
    ht, wt, bt = (torch.tensor(np.asarray(a, np.float64), requires_grad=True) for a in (h, w2, b2))
    y = F.linear(ht, wt, bt).view(B, -1, 4)
    out = y[:, :, :3] / torch.linalg.norm(y[:, :, :3], dim=-1, keepdim=True) * y[:, :, 3:4]
    out[:, 0] *= ref.JOINT0_SCALE
    out.backward(torch.tensor(g))
    y_ref, pose = ref.ba_head(h, w2, b2)
    assert _rel(pose, out.detach().numpy()) <= 1e-12
    for mine, theirs in zip(ref.ba_head_backward(h, w2, y_ref, g), (wt.grad, bt.grad, ht.grad)):
        assert _rel(mine, theirs.numpy()) <= 1e-12


def test_the_rotation_head_is_orthonormal_and_small_angles_are_finite():
    rv = np.array([[0.0, 0.0, 0.0], [1e-9, 0.0, 0.0], [0.3, -1.2, 2.0], [np.pi, 0.0, 0.0]])
    R = ref.axis_angle_to_matrix(rv)
    assert np.allclose(R @ np.swapaxes(R, -1, -2), np.eye(3), atol=1e-14) and np.allclose(np.linalg.det(R), 1.0)
    assert np.allclose(R[0], np.eye(3)) and np.allclose(R[3], np.diag([1.0, -1.0, -1.0]), atol=1e-15)


def test_the_modules_carry_the_references_state_dict(golden):
    module, sd, _, _, _, _ = golden
    keys = list(module.state_dict().keys())
    assert keys == [str(k) for k in GOLDEN["keys"]]
    assert [",".join(str(n) for n in module.state_dict()[k].shape) for k in keys] == [str(s) for s in GOLDEN["shapes"]]
    module.load_state_dict({k: torch.as_tensor(v) for k, v in sd.items()}, strict=True)
    assert np.array_equal(module.RTprocess.linear_stages_T[1].w2.weight.detach().numpy(), sd["RTprocess.linear_stages_T.1.w2.weight"])
    assert int(module.BAprocess.batch_norm1.num_batches_tracked) == 3
    # what the loop does with the module works as on any nn.Module
    module.apply(lambda m: torch.nn.init.kaiming_normal_(m.weight) if isinstance(m, torch.nn.Linear) else None)
    torch.optim.Adam(module.parameters(), lr=1e-4)
    assert module.train().training and not module.eval().BAprocess.training
    import posegen_amd
    assert posegen_amd.HipPoseGenerator is gen.HipPoseGenerator and posegen_amd.HipBAGenerator is gen.HipBAGenerator


def test_host_inputs_are_refused_in_the_modules_words():
    with pytest.raises(NotImplementedError, match="there is no CPU path"):
        gen.HipPoseGenerator()(torch.zeros(4, 24, 3))
    with pytest.raises(ValueError, match="slope"):
        gen.GenSpec([(5, 40, 1)], slope=-0.01)


def test_the_third_header_declares_its_six_functions_and_the_library_exports_them():
    with open(HEADER) as f:
        text = f.read()
    code = re.sub(r"/\*.*?\*/", " ", text, flags=re.S)
    decls = {m.group(1): m.group(2) for m in re.finditer(r"\bint\s+(pg_\w+)\s*\(([^;]*?)\)\s*;", code, flags=re.S)}
    assert set(decls) == set(COMPUTE) | {"pg_gen_tape_size"}
    assert sh.stream_entry_points(text) == list(COMPUTE)
    for name in COMPUTE:
        args = [a.strip() for a in decls[name].split(",")]
        assert re.fullmatch(r"pg_handle\s*\*\s*h", args[0]) and re.fullmatch(r"void\s*\*\s*stream", args[1]), name
        body = text[:text.index(f"int {name}(")]
        assert "Asynchronous on `stream`" in re.sub(r"\s*\n\s*\*?\s*", " ", body[body.rindex("/*"):]), name
    assert "stream" not in decls["pg_gen_tape_size"]
    assert "PG_ABI_VERSION" not in code and '#include "posegen_hip.h"' in code
    lib = _ffi.load_library()
    assert set(_ffi.GENERATOR_PROTOTYPES) == set(decls)
    assert not set(_ffi.GENERATOR_PROTOTYPES) & (set(_ffi.PROTOTYPES) | set(_ffi.GAN_PROTOTYPES))
    for name, (res, args) in _ffi.GENERATOR_PROTOTYPES.items():
        assert hasattr(lib, name), f"{name} is declared in include/posegen_generator.h but not exported"
        fn = getattr(lib, name)
        assert res is C.c_int and fn.restype is C.c_int and list(fn.argtypes) == args
        assert len(args) == len(decls[name].split(",")), name
    assert len(sh.stream_entry_points()) == 45 and lib.pg_abi_version() == _ffi.PG_ABI_VERSION == 11
    # the structs and limits as the header lays them out
    assert C.sizeof(_ffi.PgGenTrunk) == 12 and C.sizeof(_ffi.PgGenSpec) == 4 + 4 * 12 + 3 * 4
    assert C.sizeof(_ffi.PgGenParams) == 6 * 4 * 9 * 8 and C.sizeof(_ffi.PgGenGrads) == 4 * 4 * 9 * 8
    for name in ("PG_GEN_MAX_TRUNKS", "PG_GEN_MAX_STAGES", "PG_GEN_MAX_LAYERS", "PG_GEN_MAX_DIM", "PG_GEN_MAX_ROWS", "PG_GEN_MAX_JOINTS"):
        assert int(re.search(rf"#define {name} (\d+)", code).group(1)) == getattr(_ffi, name), name
    # and the build wiring
    with open(os.path.join(REPO, "posegen_amd", "csrc", "Makefile")) as f:
        mk = f.read()
    assert re.search(r"^SRCS_HIP := .*\bpg_gen\.hip\b", mk, re.M) and re.search(r"^HDRS := .*posegen_generator\.h\b", mk, re.M)
    assert "pg_gen.s 4pggn" in mk and "audit_asm_hazards.py $(AUDITDIR)/pg_gen.s" in mk
    with open(os.path.join(REPO, "posegen_amd", "csrc", "pg_modules.h")) as f:
        assert re.search(r"MOD_GEN,\s*MOD_COUNT", f.read())


def _tables(spec, ptr=0x1000):
    """a parameter table whose pointers are plausible device addresses (never dereferenced by a refused call)"""
    fields = {k: [[None] * spec.layers(t) for t in range(len(spec.trunks))] for k in ("w", "b", "gamma", "beta", "running_mean", "running_var")}
    tab = gen.pointer_table(_ffi.PgGenParams(), spec, fields)
    for k in fields:
        for t in range(len(spec.trunks)):
            for l in range(spec.layers(t)):
                getattr(tab, k)[t][l] = ptr
    return tab


def _refused(rc, lib, words):
    msg = (lib.pg_last_error(None) or b"").decode()
    assert rc == _ffi.PG_EINVAL and words in msg, (rc, msg, words)


def test_tape_size_and_its_refusals():
    lib = _ffi.load_library()
    spec = ref.toy_spec()
    cs, nf, nd = spec.c_spec(), C.c_int64(0), C.c_int64(0)
    assert lib.pg_gen_tape_size(C.byref(cs), 70, C.byref(nf), C.byref(nd)) == _ffi.PG_OK
    per_row = 3 * 40 + 5 * 17 + 5 * 64
    assert nf.value == (70 + 2) * per_row and nd.value == 2 * per_row
    layout, n_f, n_d = spec.tape_layout(70)
    assert (n_f, n_d) == (nf.value, nd.value) and layout[2][4]["shift"] + 64 == n_f and layout[2][4]["var"] + 64 == n_d
    _refused(lib.pg_gen_tape_size(None, 8, C.byref(nf), C.byref(nd)), lib, "null spec")
    _refused(lib.pg_gen_tape_size(C.byref(cs), 0, C.byref(nf), C.byref(nd)), lib, "outside [1, 1048576]")
    _refused(lib.pg_gen_tape_size(C.byref(cs), _ffi.PG_GEN_MAX_ROWS + 1, C.byref(nf), C.byref(nd)), lib, "outside [1, 1048576]")
    _refused(lib.pg_gen_tape_size(C.byref(cs), 8, None, C.byref(nd)), lib, "no place")
    for field, value, words in (("n_trunks", 0, "n_trunks"), ("n_trunks", 5, "n_trunks"), ("slope", -0.01, "slope"), ("slope", float("inf"), "slope"),
                                ("slope", float("nan"), "slope"), ("eps", 0.0, "eps"), ("eps", float("nan"), "eps"), ("momentum", 1.5, "momentum"),
                                ("momentum", float("nan"), "momentum")):
        bad = spec.c_spec()
        setattr(bad, field, value)
        _refused(lib.pg_gen_tape_size(C.byref(bad), 8, C.byref(nf), C.byref(nd)), lib, words)
    for field, value in (("nz", 0), ("nz", 513), ("width", 0), ("width", 513), ("n_stages", -1), ("n_stages", 5)):
        bad = spec.c_spec()
        setattr(bad.trunk[1], field, value)
        _refused(lib.pg_gen_tape_size(C.byref(bad), 8, C.byref(nf), C.byref(nd)), lib, "trunk's")


def test_every_documented_refusal_of_the_compute_entry_points():
    lib = _ffi.load_library()
    spec = ref.toy_spec()
    cs, tab = spec.c_spec(), _tables(spec)
    P = 0x2000                                                                # an aligned address that no refused call reads
    noise, none = _ffi._GEN_PTRS(P, P, P), _ffi._GEN_PTRS(None, None, None)
    fwd, bwd = lib.pg_gen_trunk_forward, lib.pg_gen_trunk_backward
    # the trunk forward
    _refused(fwd(None, None, None, C.byref(tab), noise, 8, 1, P, P), lib, "null spec")
    _refused(fwd(None, None, C.byref(cs), None, noise, 8, 1, P, P), lib, "are required")
    _refused(fwd(None, None, C.byref(cs), C.byref(tab), None, 8, 1, P, P), lib, "are required")
    _refused(fwd(None, None, C.byref(cs), C.byref(tab), noise, 8, 1, None, P), lib, "are required")
    _refused(fwd(None, None, C.byref(cs), C.byref(tab), noise, 8, 1, P, None), lib, "are required")
    _refused(fwd(None, None, C.byref(cs), C.byref(tab), none, 8, 1, P, P), lib, "no trunk to run")
    _refused(fwd(None, None, C.byref(cs), C.byref(tab), noise, 1, 1, P, P), lib, "B >= 2")
    _refused(fwd(None, None, C.byref(cs), C.byref(tab), noise, 0, 0, P, P), lib, "outside [1, 1048576]")
    _refused(fwd(None, None, C.byref(cs), C.byref(tab), noise, _ffi.PG_GEN_MAX_ROWS + 1, 1, P, P), lib, "outside [1, 1048576]")
    _refused(fwd(None, None, C.byref(cs), C.byref(tab), noise, 8, 1, P + 2, P), lib, "not aligned")
    _refused(fwd(None, None, C.byref(cs), C.byref(tab), noise, 8, 1, P, P + 4), lib, "not aligned")
    _refused(fwd(None, None, C.byref(cs), C.byref(tab), _ffi._GEN_PTRS(P, P + 1, P), 8, 1, P, P), lib, "not aligned")
    bad = spec.c_spec()
    bad.slope = -0.5
    _refused(fwd(None, None, C.byref(bad), C.byref(tab), noise, 8, 1, P, P), lib, "slope")
    hole = _tables(spec)
    hole.running_var[2][3] = None
    _refused(fwd(None, None, C.byref(cs), C.byref(hole), noise, 8, 1, P, P), lib, "trunk 2, layer 3")
    hole = _tables(spec)
    hole.gamma[0][1] = 0x1002
    _refused(fwd(None, None, C.byref(cs), C.byref(hole), noise, 8, 1, P, P), lib, "trunk 0, layer 1")
    _refused(fwd(None, None, C.byref(cs), C.byref(tab), noise, 8, 1, P, P), lib, "null handle")     # all else in order: the handle is checked last
    _refused(fwd(None, None, C.byref(cs), C.byref(tab), noise, 1, 0, P, P), lib, "null handle")     # eval mode takes one row
    # the trunk backward
    _refused(bwd(None, None, C.byref(cs), C.byref(tab), noise, 8, 0, P, P, noise, None), lib, "eval mode")      # a tape of an eval-mode forward
    _refused(bwd(None, None, C.byref(cs), C.byref(tab), noise, 8, 1, P, P, None, None), lib, "d_out is required")
    _refused(bwd(None, None, C.byref(cs), C.byref(tab), noise, 8, 1, P, P, none, None), lib, "no trunk to run")
    _refused(bwd(None, None, C.byref(cs), C.byref(tab), _ffi._GEN_PTRS(None, P, P), 8, 1, P, P, _ffi._GEN_PTRS(P, None, None), None), lib, "has no noise")
    _refused(bwd(None, None, C.byref(cs), C.byref(tab), noise, 1, 1, P, P, noise, None), lib, "B >= 2")
    _refused(bwd(None, None, C.byref(cs), C.byref(tab), noise, 8, 1, None, P, noise, None), lib, "are required")
    g = _ffi.PgGenGrads()
    g.beta[1][2] = 0x3001
    _refused(bwd(None, None, C.byref(cs), C.byref(tab), noise, 8, 1, P, P, noise, C.byref(g)), lib, "gradient pointer is misaligned")
    _refused(bwd(None, None, C.byref(cs), C.byref(tab), noise, 8, 1, P, P, noise, None), lib, "null handle")
    # the heads
    hf, hb, rt = lib.pg_gen_ba_head_forward, lib.pg_gen_ba_head_backward, lib.pg_gen_rt_head
    _refused(hf(None, None, C.byref(cs), 3, P, 8, 24, P, P, P, P), lib, "trunk 3 is outside")
    _refused(hf(None, None, C.byref(cs), -1, P, 8, 24, P, P, P, P), lib, "trunk -1 is outside")
    _refused(hf(None, None, C.byref(cs), 0, P, 8, 0, P, P, P, P), lib, "J = 0")
    _refused(hf(None, None, C.byref(cs), 0, P, 8, 65, P, P, P, P), lib, "J = 65")
    _refused(hf(None, None, C.byref(cs), 0, P, 0, 24, P, P, P, P), lib, "outside [1, 1048576]")
    _refused(hf(None, None, C.byref(cs), 0, P, 8, 24, P, P, None, P), lib, "are required")
    _refused(hf(None, None, C.byref(cs), 0, P, 8, 24, P, P, P, P + 1), lib, "not aligned")
    _refused(hf(None, None, C.byref(cs), 0, P, 8, 24, P, P, P, P), lib, "null handle")
    _refused(hb(None, None, C.byref(cs), 0, P, 8, 24, P, None, P, P, P, P), lib, "are required")
    _refused(hb(None, None, C.byref(cs), 0, P, 8, 24, P, P, P, P, P + 3, P), lib, "not aligned")
    _refused(hb(None, None, C.byref(bad), 0, P, 8, 24, P, P, P, None, None, None), lib, "slope")
    _refused(hb(None, None, C.byref(cs), 0, P, 8, 24, P, P, P, None, None, None), lib, "null handle")
    _refused(rt(None, None, C.byref(cs), 1, 3, P, 8, 24, P, P, P, P, P, P, P), lib, "trunk 3 is outside")
    _refused(rt(None, None, C.byref(cs), 1, 2, P, 8, 24, P, P, None, P, P, P, P), lib, "are required")
    _refused(rt(None, None, C.byref(cs), 1, 2, P, 8, 24, P, P, P, P, P, P + 2, P), lib, "not aligned")
    narrow = gen.GenSpec([(5, 6, 1), (5, 40, 1)]).c_spec()
    _refused(rt(None, None, C.byref(narrow), 0, 1, P, 8, 24, P, P, P, P, P, P, P), lib, "narrower than 7")
    _refused(rt(None, None, C.byref(cs), 1, 2, P, 8, 24, P, P, P, P, P, P, P), lib, "null handle")


# ---- the backward's carried bound, judged without a device ---------------------------------------------------------------------------------
EDGE_CASES = [(name, B) for name, batches in ref.EDGE_BATCHES.items() for B in batches] + [("rows", None)] + [(name, None) for name in ref.DEGENERATE]
NAMES = ("dw", "db", "dgamma", "dbeta")
U = 2.0 ** -24
WORST32 = {}


def _ratio(err, bound):
    with np.errstate(invalid="ignore", divide="ignore"):
        r = np.where(bound > 0, err / np.where(bound > 0, bound, 1.0), np.where(err > 0, np.inf, 0.0))
    return float(np.max(r)) if r.size else 0.0


def _emulated(name, B):
    """one case as the device would run it, in float32 on the CPU -> spec, params, per trunk (tape, masks), cots"""
    spec, params, noise, cots = ref.edge_case(name, B)
    slope, eps = ref.held(spec)
    runs = []
    for layers, n in zip(params, noise):
        tape = ref.rebuilt_tape(n, ref.emulate32_forward(layers, n, slope, eps), slope)
        runs.append((tape, [t["y"] > 0 for t in tape]))
    return spec, params, runs, cots


@pytest.mark.parametrize("name,B", EDGE_CASES)
def test_the_bounded_backward_equals_the_hand_written_one_and_float64_autograd(name, B):
    """on a float64 tape of its own the three agree to float64's rounding, on every spec and parameter edit of the edge tests (the row
    limit at 4096 rows: autograd's time).  Two identical noise rows are compared with the hand-written backward alone: there every
    variance is 0 and x^ = (z - mean) / sqrt(eps) turns the last bit of a forward's own z into 1e-14, which the k = gamma / sqrt(eps) / 2
    of each layer below multiplies by 10^2 again, so autograd's gradients are its own forward's rounding noise (1e-7 of d_gamma on one
    machine, 0 on another); the backward from a given tape has no such freedom, and that is what the device is compared with."""
    spec, params, noise, cots = ref.edge_case(name, 4096 if name == "rows" else B)
    for t, layers in enumerate(params):
        _, tape = ref.trunk_forward(layers, noise[t], spec.slope, spec.eps, spec.momentum)
        masks = ref.masks_of(tape)
        mine, bound = ref.trunk_backward_with_bound(layers, tape, masks, cots[t], spec.slope, spec.eps)
        old = ref.trunk_backward(layers, tape, cots[t], spec.slope, spec.eps)
        _, auto = _autograd_trunk(layers, noise[t], cots[t].astype(np.float64), spec.slope, spec.eps)
        for l in range(len(layers)):
            for k, m, o, a, e in zip(NAMES, mine[l], old[l], auto[l], bound[l]):
                # float64's rounding is relative to the sum of the magnitudes that an entry adds up, not to the entry (two identical
                # rows: every dW is 0 exactly, the sum of two opposite products); the bound carries that sum at u = 2^-24, so 2^-20
                # of the bound is 2^-44 of it
                tol = 1e-12 * max(1.0, float(np.max(np.abs(o)))) + 2.0 ** -20 * e
                assert np.all(np.abs(m - o) <= tol) and (name == "twin rows" or np.all(np.abs(m - a) <= 100 * tol)), (t, l, k)


@pytest.mark.parametrize("name,B", EDGE_CASES)
def test_honest_float32_stays_inside_the_backwards_bound(name, B):
    spec, params, runs, cots = _emulated(name, B)
    slope, eps = ref.held(spec)
    worst = {}
    for t, (layers, (tape, masks)) in enumerate(zip(params, runs)):
        g64, bound = ref.trunk_backward_with_bound(layers, tape, masks, cots[t], slope, eps)
        g32 = ref.emulate32_backward(layers, tape, masks, cots[t], slope, eps)
        for l in range(len(layers)):
            for k, a, b, e in zip(NAMES, g32[l], g64[l], bound[l]):
                err = np.abs(a.astype(np.float64) - b)
                worst[k] = max(worst.get(k, 0.0), _ratio(err, e))
                assert np.all(np.isfinite(b)) and np.all(err <= e), (name, B, t, l, k, _ratio(err, e))
    for k, v in worst.items():
        WORST32[k] = max(WORST32.get(k, 0.0), v)
    print(f"EMULATE32 {name} B={B}: " + ", ".join(f"{k} {v:.3f}" for k, v in worst.items()) + " | worst so far " + ", ".join(f"{k} {v:.3f}" for k, v in WORST32.items()))


@pytest.mark.parametrize("name,B,J", ref.HEAD_CASES + (("rows", None, 1),))
def test_honest_float32_stays_inside_the_heads_bound(name, B, J):
    spec, params, runs, _ = _emulated(name, B)
    slope, _ = ref.held(spec)
    tape, rng = runs[0][0], np.random.RandomState(800 + J)
    Bn, W = tape[-1]["z"].shape
    w2, b2 = ref.make_head(4 * J, W, rng)
    d_pose = rng.standard_normal((Bn, J, 3)).astype(np.float32)
    h = ref.leaky(tape[-1]["y"], slope)
    y = (ref._act32(tape[-1]["z"], tape[-1]["scale"], tape[-1]["shift"], slope) @ w2.T + b2).astype(np.float32)
    g64, bound = ref.ba_head_backward_with_bound(h, w2, y, d_pose)
    g32 = ref.emulate32_head_backward(tape[-1], w2, y, d_pose, slope)
    old = ref.ba_head_backward(h, w2, y, d_pose)
    for k, a, b, e, o in zip(("d_w2", "d_b2", "d_h"), g32, g64, bound, old):
        err = np.abs(a.astype(np.float64) - b)
        print(f"EMULATE32 head {name} J={J} {k}: {_ratio(err, e):.3f}")
        assert np.array_equal(b, o) and np.all(err <= e), (k, _ratio(err, e))


def test_honest_float32_stays_inside_the_bound_on_the_ragged_modules_parameters():
    """the head of 24 joints and the three layers of HipBAGenerator(noise 5, width 40, one stage), as the device test chains them"""
    _, sd, spec, layers, noise, d_pose = ref.ragged_module_case()
    slope, eps = ref.held(spec)
    tape = ref.rebuilt_tape(noise, ref.emulate32_forward(layers, noise, slope, eps), slope)
    masks = [t["y"] > 0 for t in tape]
    w2, b2 = sd["w2.weight"], sd["w2.bias"]
    y = (ref._act32(tape[-1]["z"], tape[-1]["scale"], tape[-1]["shift"], slope) @ w2.T + b2).astype(np.float32)
    g64, bound = ref.ba_head_backward_with_bound(ref.leaky(tape[-1]["y"], slope), w2, y, d_pose)
    g32 = ref.emulate32_head_backward(tape[-1], w2, y, d_pose, slope)
    worst = max(_ratio(np.abs(a.astype(np.float64) - b), e) for a, b, e in zip(g32, g64, bound))
    assert all(np.all(np.abs(a.astype(np.float64) - b) <= e) for a, b, e in zip(g32, g64, bound))
    t64, tbound = ref.trunk_backward_with_bound(layers, tape, masks, g32[2], slope, eps)
    t32 = ref.emulate32_backward(layers, tape, masks, g32[2], slope, eps)
    for l in range(3):
        for k, a, b, e in zip(NAMES, t32[l], t64[l], tbound[l]):
            err = np.abs(a.astype(np.float64) - b)
            worst = max(worst, _ratio(err, e))
            assert np.all(err <= e), (l, k)
    print(f"EMULATE32 ragged module: {worst:.3f}")


def _broken(name, B, mutant=None, masks_edit=None):
    """per tensor name, the (trunk, layer) pairs where a planted error leaves the bound"""
    spec, params, runs, cots = _emulated(name, B)
    slope, eps = ref.held(spec)
    out = {k: set() for k in NAMES}
    for t, (layers, (tape, masks)) in enumerate(zip(params, runs)):
        g64, bound = ref.trunk_backward_with_bound(layers, tape, masks, cots[t], slope, eps)
        wrong = masks if masks_edit is None else masks_edit(tape, masks)
        g32 = ref.emulate32_backward(layers, tape, wrong, cots[t], slope, eps, mutant)
        for l in range(len(layers)):
            for k, a, b, e in zip(NAMES, g32[l], g64[l], bound[l]):
                if not np.all(np.abs(a.astype(np.float64) - b) <= e):
                    out[k].add((t, l))
    return spec, out


MUTANT_CASES = [(name, B) for name, batches in ref.EDGE_BATCHES.items() for B in batches] + [(name, None) for name in ref.DEGENERATE if name != "twin rows"]


@pytest.mark.parametrize("name,B", MUTANT_CASES)
def test_the_bound_sees_x_hat_from_the_unbiased_variance(name, B):
    """d_gamma and dW of every trunk's top layer leave the bound (slope 0 aside, where a dW can be all zero past the top layer only)"""
    spec, out = _broken(name, B, "unbiased x^")
    for t in range(len(spec.trunks)):
        top = spec.layers(t) - 1
        assert (t, top) in out["dgamma"] and (t, top) in out["dw"], (t, out)


@pytest.mark.parametrize("name,B", MUTANT_CASES)
def test_the_bound_sees_a_dropped_x_hat_d_gamma_term(name, B):
    spec, out = _broken(name, B, "no x^ d_gamma")
    for t in range(len(spec.trunks)):
        assert (t, spec.layers(t) - 1) in out["dw"], (t, out)


@pytest.mark.parametrize("name,B", [(n, B) for n, B in MUTANT_CASES if n in ("toy", "deep")])
def test_the_bound_sees_a_ragged_tiles_last_column_summed_one_row_short(name, B):
    """d_beta at width 17 (trunk 1 of the toy and of the deep spec), top layer"""
    spec, out = _broken(name, B, "short last column")
    assert spec.trunks[1][1] == 17 and (1, spec.layers(1) - 1) in out["dbeta"], out


def test_the_bound_sees_an_exactly_zero_pre_activation_taken_as_positive():
    """d_beta of the gamma = 0, beta = +-0 columns (the top layer of every trunk; the slope is 0.01)"""
    def edit(tape, masks):
        return [m | (t["y"] == 0) for t, m in zip(tape, masks)]
    spec, params, runs, cots = _emulated("gamma 0", None)
    slope, eps = ref.held(spec)
    for t, (layers, (tape, masks)) in enumerate(zip(params, runs)):
        cols = list(ref.gamma0_columns(spec.trunks[t][1])[:2])
        assert np.all(tape[-1]["y"][:, cols] == 0) and not masks[-1][:, cols].any()
        g64, bound = ref.trunk_backward_with_bound(layers, tape, masks, cots[t], slope, eps)
        g32 = ref.emulate32_backward(layers, tape, edit(tape, masks), cots[t], slope, eps)
        err = np.abs(g32[-1][3].astype(np.float64) - g64[-1][3])
        assert np.all(err[cols] > bound[-1][3][cols]), t
        others = np.setdiff1d(np.arange(err.size), cols)
        assert np.all(err[others] <= bound[-1][3][others]), t


@pytest.mark.parametrize("name,B", MUTANT_CASES)
def test_k_from_the_rounded_scale_is_one_rounding_and_cannot_be_seen(name, B):
    """The mutant the bound does not see, and why: a float32 scale is gamma / sqrt(var + eps) to within u / (1 + u) of it -- rounding
    to nearest has no column that `rounds badly` -- so k from it moves dZ by less than the u |dZ| that dZ's own rounding is
    allowed, and every dW by less than u |dW|: inside (B + 2) u |dZ|^T |H| by construction.  Asserted on every fixture: no column's
    scale is further off than that, and the mutant stays inside the bound everywhere.  The mutant is dropped."""
    spec, params, runs, _ = _emulated(name, B)
    _, eps = ref.held(spec)
    for layers, (tape, _) in zip(params, runs):
        for layer, t in zip(layers, tape):
            exact = np.asarray(layer["gamma"], np.float64) / np.sqrt(t["var"] + eps)
            assert np.all(np.abs(t["scale"] - exact) <= U / (1 + U) * np.abs(exact) * (1 + 2.0 ** -50))
    _, out = _broken(name, B, "scale32 k")
    assert not any(out.values()), out
