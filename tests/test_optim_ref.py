"""Host checks of the optimiser step (include/posegen_optim.h, posegen_amd/optim.py): the float64 restatement
(tests/optim_ref.py) against torch.optim.Adam in float64, a float32 emulation of the device and five planted errors against the bound
the device is held to, the header against its ctypes mirror, the refusals through the built library, `HipAdam` on host parameters,
and the planning code under the sanitisers.  No GPU."""
import ctypes as C
import math
import os
import re
import subprocess

import numpy as np
import pytest
import torch

from posegen_amd import _ffi, optim
from tests import optim_ref as ref
from tests import stream_harness as sh

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(REPO, "include", "posegen_optim.h")


# ---- the restatement against torch in float64 ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("weight_decay", [0.0, 0.05])
def test_the_restatement_is_torch_adam_in_float64_over_five_steps(weight_decay):
    rng = np.random.RandomState(3)
    shapes = [(7,), (3, 5), (1,), (40,)]
    groups = [{"lr": 2e-3, "betas": (0.9, 0.999), "eps": 1e-8, "weight_decay": weight_decay},
              {"lr": 1e-2, "betas": (0.8, 0.95), "eps": 1e-6, "weight_decay": weight_decay}]
    params = [torch.nn.Parameter(torch.tensor(rng.standard_normal(s), dtype=torch.float64)) for s in shapes]
    opt = torch.optim.Adam([dict(params=params[:2], **groups[0]), dict(params=params[2:], **groups[1])], foreach=False)
    mine = [{"p": p.detach().numpy().copy().reshape(-1), "m": np.zeros(p.numel()), "v": np.zeros(p.numel()), "group": 0 if i < 2 else 1}
            for i, p in enumerate(params)]
    for step in range(1, 6):
        grads = [rng.standard_normal(s) * (3.0 if step % 2 else 0.01) for s in shapes]        # above and below the clipping norm
        for p, g in zip(params, grads):
            p.grad = torch.tensor(g)
        norm = torch.nn.utils.clip_grad_norm_(params, 1.0)
        opt.step()
        for t, g in zip(mine, grads):
            t["g"], t["step"] = g.reshape(-1), step
        r = ref.adam_step(mine, groups, max_norm=1.0)
        assert abs(r["norm"] - float(norm)) <= 1e-13 * float(norm)
        for t, o, p in zip(mine, r["tensors"], params):
            t["p"], t["m"], t["v"] = o["p"], o["m"], o["v"]
            st = opt.state[p]
            # (relative to the terms the value is the sum of: m + (g' - m)(1 - b1) cancels where the gradient turns)
            for mine_x, mag, torch_x in ((o["p"], o["mag_p"], p), (o["m"], o["mag_m"], st["exp_avg"]), (o["v"], o["mag_v"], st["exp_avg_sq"])):
                want = torch_x.detach().numpy().reshape(-1)
                assert np.all(np.abs(mine_x - want) <= 1e-13 * mag), step


# ---- the bound: an honest float32 emulation inside it, planted errors outside ----------------------------------------------------------------
CASES = ref.table_cases()


@pytest.mark.parametrize("name", sorted(CASES))
def test_the_float32_emulation_is_inside_the_bound_at_every_table_case(name):
    tensors, groups, max_norm = CASES[name]
    r = ref.adam_step(tensors, groups, max_norm)
    worst, equal, bad = ref.judge(ref.emulate(tensors, groups, max_norm), r["tensors"], write_grads=True)
    print(f"{name}: emulation at {worst:.3f} of the bound, {equal:.4f} bitwise float32(f64)")
    assert not bad and worst <= 1.0, bad[:5]


MUTANT_CASES = {"coef32": "tiny_p", "t_minus_1": "steps", "eps_in_sqrt": "counts", "swap_betas": "counts", "wd_scaled": "above"}


@pytest.mark.parametrize("mutant", ref.MUTANTS)
def test_each_planted_error_leaves_the_bound(mutant):
    name = MUTANT_CASES[mutant]
    tensors, groups, max_norm = CASES[name]
    if mutant == "coef32":
        assert float(np.abs(tensors[0]["p"]).max()) < 1e-5       # the case whose parameters are around 1e-6
    r = ref.adam_step(tensors, groups, max_norm)
    worst, _, bad = ref.judge(ref.emulate(tensors, groups, max_norm, mutant=mutant), r["tensors"], write_grads=True)
    print(f"{mutant} on {name}: {worst:.3g} of the bound, {len(bad)} elements reported")
    assert bad and worst > 1.0


def test_torchs_own_float32_adam_is_outside_the_ulp_term_by_design():
    """torch's float32 CPU Adam rounds after every operator (lerp, mul, addcmul, sqrt, div, add, addcdiv), so it sits outside one
    rounding of the float64 value: reported in the bound's units, which is why the device is held to float64 and not to it."""
    tensors, groups, max_norm = CASES["below"]                    # (coefficient 1: the gradients go in as they are)
    r = ref.adam_step(tensors, groups, None)
    dev = []
    for t in tensors:
        q = groups[t["group"]]
        p = torch.nn.Parameter(torch.tensor(t["p"]))
        p.grad = torch.tensor(t["g"])
        o = torch.optim.Adam([p], lr=q["lr"], betas=q["betas"], eps=q["eps"], weight_decay=q["weight_decay"], foreach=False)
        o.state[p] = {"step": torch.tensor(float(t["step"] - 1)), "exp_avg": torch.tensor(t["m"]), "exp_avg_sq": torch.tensor(t["v"])}
        o.step()
        dev.append({"p": p.detach().numpy(), "m": o.state[p]["exp_avg"].numpy(), "v": o.state[p]["exp_avg_sq"].numpy()})
    worst, equal, bad = ref.judge(dev, r["tensors"])
    print(f"torch float32 CPU Adam: {worst:.2f} of the bound, {equal:.4f} bitwise float32(f64)")
    assert worst > 1.0                                            # outside one rounding (far outside where m + (g' - m)(1 - b1) cancels)
    tol = max(float(np.max(np.abs(d["p"].astype(np.float64) - t["p"]) / (np.abs(t["p"]) + 1e-3))) for d, t in zip(dev, r["tensors"]))
    assert tol < 1e-5                                             # yet the same formula


# ---- the header, its mirror and the wiring ---------------------------------------------------------------------------------------------------
def test_the_fifth_header_declares_one_function_and_the_library_exports_it():
    with open(HEADER) as f:
        text = f.read()
    code = re.sub(r"/\*.*?\*/", " ", text, flags=re.S)
    decls = {m.group(1): m.group(2) for m in re.finditer(r"\bint\s+(pg_\w+)\s*\(([^;]*?)\)\s*;", code, flags=re.S)}
    assert set(decls) == {"pg_adam_step"} and sh.stream_entry_points(text) == ["pg_adam_step"]
    args = [a.strip() for a in decls["pg_adam_step"].split(",")]
    assert re.fullmatch(r"pg_handle\s*\*\s*h", args[0]) and re.fullmatch(r"void\s*\*\s*stream", args[1])
    body = text[:text.index("int pg_adam_step(")]
    assert "Asynchronous on `stream`" in re.sub(r"\s*\n\s*\*?\s*", " ", body[body.rindex("/*"):])
    assert "PG_ABI_VERSION" not in code and '#include "posegen_hip.h"' in code
    lib = _ffi.load_library()
    assert set(_ffi.OPTIM_PROTOTYPES) == set(decls)
    others = set(_ffi.PROTOTYPES) | set(_ffi.GAN_PROTOTYPES) | set(_ffi.GENERATOR_PROTOTYPES) | set(_ffi.REGRESSOR_PROTOTYPES)
    assert not set(_ffi.OPTIM_PROTOTYPES) & others
    res, argtypes = _ffi.OPTIM_PROTOTYPES["pg_adam_step"]
    fn = lib.pg_adam_step
    assert res is C.c_int and fn.restype is C.c_int and list(fn.argtypes) == argtypes and len(argtypes) == len(args) == 9
    # the structs and the #defines against their mirrors
    assert C.sizeof(_ffi.PgAdamGroup) == 5 * 8 and C.sizeof(_ffi.PgAdamTensor) == 4 * 8 + 8 + 4 + 4
    group = code[code.index("typedef struct pg_adam_group"):code.index("} pg_adam_group;")]
    assert [n.strip() for n in re.search(r"double\s+([^;]+);", group).group(1).split(",")] == [n for n, _ in _ffi.PgAdamGroup._fields_]
    tensor = code[code.index("typedef struct pg_adam_tensor"):code.index("} pg_adam_tensor;")]
    assert re.findall(r"(\w+)\s*;", tensor) == [n for n, _ in _ffi.PgAdamTensor._fields_]
    assert re.findall(r"(float\s*\*|int64_t|int32_t)\s*\w+\s*;", tensor) == ["float*"] * 4 + ["int64_t", "int32_t", "int32_t"]
    for name in ("PG_ADAM_MAX_TENSORS", "PG_ADAM_MAX_GROUPS", "PG_ADAM_SEGMENT"):
        assert int(re.search(rf"#define {name} (\d+)", code).group(1)) == getattr(_ffi, name), name
    assert float(re.search(r"#define PG_ADAM_NO_CLIP \((-?[\d.]+)\)", code).group(1)) == _ffi.PG_ADAM_NO_CLIP == -1.0
    assert ref.SEG == _ffi.PG_ADAM_SEGMENT
    # what the other headers' tests pin still holds
    main = sh.header_text()
    assert re.search(r"#define\s+PG_ABI_VERSION\s+11\b", main) and lib.pg_abi_version() == _ffi.PG_ABI_VERSION == 11
    assert len(sh.stream_entry_points(main)) == 45 and "pg_adam_step" not in main
    with open(os.path.join(REPO, "posegen_amd", "csrc", "Makefile")) as f:
        mk = f.read()
    assert re.search(r"^SRCS_HIP := .*\bpg_optim\.hip\b", mk, re.M) and re.search(r"^HDRS := .*\bpg_optim_plan\.h\b.*posegen_optim\.h\b", mk, re.M)
    assert "pg_optim.s 4pgop" in mk and re.search(r"^audit:.*\$\(AUDITDIR\)/pg_optim\.s\b", mk, re.M)
    with open(os.path.join(REPO, "posegen_amd", "csrc", "pg_modules.h")) as f:
        assert re.search(r"MOD_OPTIM,\s*MOD_GEN,\s*MOD_COUNT", f.read())
    import posegen_amd
    assert posegen_amd.HipAdam is optim.HipAdam


def _tables(n=1, count=8, **over):
    tab = (_ffi.PgAdamTensor * max(n, 1))()
    for e in tab:
        e.param = e.grad = e.exp_avg = e.exp_avg_sq = 4096
        e.count, e.group, e.step = count, 0, 1
    g = (_ffi.PgAdamGroup * 2)()
    for q in g:
        q.lr, q.beta1, q.beta2, q.eps, q.weight_decay = 1e-3, 0.9, 0.999, 1e-8, 0.0
    return tab, g


def test_the_refusals_come_before_the_handle_is_looked_at():
    """every refusal of the header through the built library with a NULL handle: PG_EINVAL with the refusal's own message (a legal
    call with a NULL handle is refused as well, with "null handle": that is the control)"""
    lib = _ffi.load_library()

    def call(tab, groups, n=1, n_groups=2, max_norm=1.0, out=None):
        rc = lib.pg_adam_step(None, None, n, tab, n_groups, groups, max_norm, 0, out)
        return rc, (lib.pg_last_error(None) or b"").decode()
    tab, g = _tables()
    rc, msg = call(tab, g)
    assert rc == _ffi.PG_EINVAL and "null handle" in msg
    rc, msg = call(tab, g, max_norm=_ffi.PG_ADAM_NO_CLIP)
    assert rc == _ffi.PG_EINVAL and "null handle" in msg

    def refused(words, **kw):
        t, q = kw.pop("tab", tab), kw.pop("groups", g)
        rc, msg = call(t, q, **kw)
        assert rc == _ffi.PG_EINVAL and "null handle" not in msg and words in msg, (words, msg)
    refused("n_tensors", n=0)
    refused("n_tensors", n=_ffi.PG_ADAM_MAX_TENSORS + 1)
    refused("n_groups", n_groups=0)
    refused("n_groups", n_groups=_ffi.PG_ADAM_MAX_GROUPS + 1)
    refused("required", tab=None)
    refused("required", groups=None)
    refused("max_norm", max_norm=float("nan"))
    refused("max_norm", max_norm=-0.5)
    refused("out is not aligned", out=C.c_void_p(4100))
    for field, value, words in (("group", 2, "group"), ("group", -1, "group"), ("step", 0, "step"), ("count", -1, "elements"),
                                ("grad", None, "NULL pointer"), ("param", None, "NULL pointer"), ("exp_avg", 4098, "not aligned"),
                                ("exp_avg_sq", 4097, "not aligned"), ("count", 2 ** 62, "segments")):
        t, _ = _tables()
        setattr(t[0], field, value)
        refused(words, tab=t)
    t, _ = _tables(n=2, count=(2 ** 31 - 1) * _ffi.PG_ADAM_SEGMENT)
    t[1].count = 1
    refused("segments", tab=t, n=2)
    for field, value in (("lr", -1e-3), ("eps", -1e-8), ("beta1", 1.0), ("beta1", -0.1), ("beta2", 1.0), ("weight_decay", -0.1), ("lr", float("nan"))):
        _, q = _tables()
        setattr(q[1], field, value)
        refused("group 1", groups=q)
    # count == 0 is legal with NULL pointers: the call gets as far as the handle
    t, _ = _tables(count=0)
    t[0].param = t[0].grad = t[0].exp_avg = t[0].exp_avg_sq = None
    rc, msg = call(t, g)
    assert rc == _ffi.PG_EINVAL and "null handle" in msg


# ---- HipAdam on host parameters --------------------------------------------------------------------------------------------------------------
def _params():
    g = torch.Generator().manual_seed(4)
    return [torch.nn.Parameter(torch.randn(3, 4, generator=g)), torch.nn.Parameter(torch.randn(5, generator=g))]


def test_hipadam_keeps_torch_adams_layout_and_refuses_what_is_not_built():
    params = _params()
    opt = optim.HipAdam([{"params": params[:1]}, {"params": params[1:], "lr": 5e-2, "betas": (0.5, 0.9)}], lr=2e-3, weight_decay=0.01)
    twin = torch.optim.Adam([{"params": params[:1]}, {"params": params[1:], "lr": 5e-2, "betas": (0.5, 0.9)}], lr=2e-3, weight_decay=0.01)
    assert isinstance(opt, torch.optim.Optimizer)
    for a, b in zip(opt.param_groups, twin.param_groups):
        assert set(a) == set(b) and all(a[k] == b[k] for k in a if k != "params")
    # hand-filled state through both load_state_dict directions
    for i, p in enumerate(params):
        twin.state[p] = {"step": torch.tensor(float(3 + i)), "exp_avg": torch.full_like(p, 0.25 * (i + 1)), "exp_avg_sq": torch.full_like(p, 0.5 * (i + 1))}
    opt.load_state_dict(twin.state_dict())
    for i, p in enumerate(params):
        st = opt.state[p]
        assert set(st) == {"step", "exp_avg", "exp_avg_sq"}
        assert st["step"].device.type == "cpu" and st["step"].dtype == torch.float32 and st["step"].dim() == 0 and int(st["step"]) == 3 + i
        assert torch.equal(st["exp_avg"], torch.full_like(p, 0.25 * (i + 1))) and torch.equal(st["exp_avg_sq"], torch.full_like(p, 0.5 * (i + 1)))
    back = torch.optim.Adam([{"params": params[:1]}, {"params": params[1:]}])
    back.load_state_dict(opt.state_dict())
    assert back.param_groups[1]["lr"] == 5e-2 and back.param_groups[1]["betas"] == (0.5, 0.9) and back.param_groups[0]["weight_decay"] == 0.01
    sd_a, sd_b = twin.state_dict(), back.state_dict()
    assert sd_a["param_groups"] == sd_b["param_groups"]
    for k in sd_a["state"]:
        for leaf in ("step", "exp_avg", "exp_avg_sq"):
            assert torch.equal(sd_a["state"][k][leaf], sd_b["state"][k][leaf])
    # an integer step of an old checkpoint becomes the tensor torch keeps now
    sd = twin.state_dict()
    sd["state"][0]["step"] = 7
    opt.load_state_dict(sd)
    assert isinstance(opt.state[params[0]]["step"], torch.Tensor) and int(opt.state[params[0]]["step"]) == 7
    # foreach / fused are accepted and ignored; the rest is refused by name
    optim.HipAdam(_params(), foreach=True, fused=True)
    for k in ("amsgrad", "maximize", "capturable", "differentiable"):
        with pytest.raises(NotImplementedError, match=k):
            optim.HipAdam(_params(), **{k: True})
    with pytest.raises(ValueError):
        optim.HipAdam(_params(), lr=-1.0)                      # torch's own checks
    with pytest.raises(TypeError, match="momentum"):
        optim.HipAdam(_params(), momentum=0.9)
    opt.param_groups[0]["amsgrad"] = True
    params[0].grad = torch.zeros_like(params[0])
    with pytest.raises(NotImplementedError, match="amsgrad"):
        opt.step()


def test_hipadam_adopts_an_adam_and_has_no_cpu_path():
    params = _params()
    adam = torch.optim.Adam(params, lr=3e-3, betas=(0.8, 0.9), eps=1e-6)
    for p in params:
        p.grad = torch.ones_like(p)
    adam.step()
    opt = optim.HipAdam.adopt(adam)
    assert opt.param_groups[0] is adam.param_groups[0] and opt.param_groups[0]["lr"] == 3e-3 and opt.param_groups[0]["betas"] == (0.8, 0.9)
    for p in params:
        assert opt.state[p]["exp_avg"] is adam.state[p]["exp_avg"] and opt.state[p]["exp_avg_sq"] is adam.state[p]["exp_avg_sq"]
        assert int(opt.state[p]["step"]) == 1
    with pytest.raises(NotImplementedError, match="there is no CPU path"):
        opt.step()
    with pytest.raises(NotImplementedError, match="there is no CPU path"):
        opt.step(max_norm=1.0)
    assert all(int(opt.state[p]["step"]) == 1 for p in params)   # a refused step moves nothing
    with pytest.raises(NotImplementedError, match="SGD"):
        optim.HipAdam.adopt(torch.optim.SGD(_params(), lr=0.1))
    with pytest.raises(NotImplementedError, match="AdamW"):
        optim.HipAdam.adopt(torch.optim.AdamW(_params()))
    # without a gradient nothing is stepped and nothing is refused
    fresh = optim.HipAdam(_params())
    assert fresh.step() is None and len(fresh.state) == 0
    # the refusals of a tensor's kind name it (before the device is looked at only the CPU refusal can come first: a meta check)
    for make, words in ((lambda p: p.double(), "float64"), (lambda p: p.t(), "non-contiguous")):
        p = torch.nn.Parameter(torch.zeros(3, 4))
        with pytest.raises(NotImplementedError, match=words):
            optim.HipAdam([p])._check(make(p.detach()), make(torch.zeros(3, 4)))
    with pytest.raises(NotImplementedError, match="sparse"):
        optim.HipAdam([torch.nn.Parameter(torch.zeros(3, 4))])._check(torch.zeros(3, 4), torch.zeros(3, 4).to_sparse())


# ---- the planning code under the sanitisers --------------------------------------------------------------------------------------------------
def test_the_planning_code_is_clean_under_address_and_ub_sanitizers(tmp_path):
    """pg_optim_plan.h (what pg_adam_step checks and plans on the host, and the block lookup its kernels run) as a stand-alone program
    with its own main: empty and one-element tensors, counts at SEG - 1 / SEG / SEG + 1, 4096 tensors, the block at every segment
    boundary, every refusal."""
    clang = "/opt/rocm/lib/llvm/bin/clang++"
    if not os.path.exists(clang):
        pytest.skip("ROCm clang++ not found")
    exe = str(tmp_path / "optim_plan_asan")
    csrc = os.path.join(REPO, "posegen_amd", "csrc")
    build = subprocess.run([clang, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                            "-fno-omit-frame-pointer", "-I", csrc, os.path.join(REPO, "tools", "sanitize", "optim_plan_asan.cpp"),
                            "-o", exe], capture_output=True, text=True)
    if build.returncode != 0 and "sanitizer" in build.stderr.lower() and "cannot find" in build.stderr.lower():
        pytest.skip("sanitizer runtime not installed")
    assert build.returncode == 0, build.stderr[-2000:]
    run = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert run.returncode == 0, (run.stdout[-1500:], run.stderr[-3000:])
    assert re.search(r"\d+ block lookups clean under ASan/UBSan", run.stdout)
