"""The five compute entry points of include/posegen_generator.h and `HipPoseGenerator` on a busy, non-blocking side stream
(tests/stream_harness.run_decoy, the pattern of tests/test_gpu_disc_streams.py): decoy inputs, the real ones copied in behind a
>= 50 ms delay, two calls back to back with different inputs; both results must be the default-stream bytes, and the delay must
still be pending when the calls have returned -- the header documents all five as asynchronous.  The parameters travel with the
inputs: a training-mode forward rewrites the running statistics, so every run starts from its own copy."""
import ctypes as C
import re

import numpy as np
import pytest
import torch

from posegen_amd import _ffi, generators as gen
from tests import generator_ref as ref
from tests import stream_harness as sh
from tests.frame_metrics_gpu import DEV, renderer  # noqa: F401 (renderer: a fixture)

pytestmark = pytest.mark.gpu
SEEDS = {"A": 1, "A2": 2, "B": 3}
B, J = 70, 5
FIELDS = (("w", "w"), ("b", "b"), ("gamma", "gamma"), ("beta", "beta"), ("running_mean", "rm"), ("running_var", "rv"))


@pytest.fixture(scope="module")
def env():
    dev = torch.device(DEV)
    side = torch.cuda.Stream(dev)
    return dev, side, sh.Delay(side, dev)


def test_the_header_documents_the_compute_entry_points_as_asynchronous():
    with open(sh.HEADER.replace("posegen_hip.h", "posegen_generator.h")) as f:
        text = f.read()
    names = sh.stream_entry_points(text)
    assert len(names) == 5
    for name in names:
        body = text[:text.index(f"int {name}(")]
        prose = re.sub(r"\s*\n\s*\*?\s*", " ", body[body.rindex("/*"):])          # (line breaks of the comment become one space)
        assert "Asynchronous on `stream`" in prose, name


def test_every_entry_point_on_a_busy_side_stream(renderer, env):
    dev, side, delay = env
    spec = ref.toy_spec()
    cs = spec.c_spec()
    layout, n_f, n_d = spec.tape_layout(B)

    def make(v):
        rng = np.random.RandomState(SEEDS[v])
        d = {}
        for t, layers in enumerate(ref.make_params(spec, 20 + SEEDS[v])):
            for l, layer in enumerate(layers):
                for k, a in layer.items():
                    d[f"p{t}.{l}.{k}"] = torch.tensor(a)
        for t, n in enumerate(ref.make_noise(spec, B, 30 + SEEDS[v])):
            d[f"noise{t}"] = torch.tensor(n)
        w2, b2 = ref.make_head(4 * J, 40, rng)
        w2t, b2t = ref.make_head(3, 17, rng)
        d.update({"w2": torch.tensor(w2), "b2": torch.tensor(b2), "w2t": torch.tensor(w2t), "b2t": torch.tensor(b2t),
                  "eps": torch.tensor(rng.standard_normal((B, 3)).astype(np.float32)), "x": torch.tensor(rng.standard_normal((B, J, 3)).astype(np.float32)),
                  "d_pose": torch.tensor(rng.standard_normal((B, J, 3)).astype(np.float32)),
                  "cot1": torch.tensor(rng.standard_normal((B, 17)).astype(np.float32))})
        return d, None

    def run(d, _host):
        tab = gen.pointer_table(_ffi.PgGenParams(), spec, {f: [[d[f"p{t}.{l}.{k}"] for l in range(spec.layers(t))] for t in range(3)] for f, k in FIELDS})
        noise = gen.pointer_array([d[f"noise{t}"] for t in range(3)])
        tape, stats = torch.empty(n_f, device=dev), torch.empty(n_d, dtype=torch.float64, device=dev)
        y, pose = torch.empty(B, 4 * J, device=dev), torch.empty(B, J, 3, device=dev)
        R, T, pose_rt = torch.empty(B, 3, 3, device=dev), torch.empty(B, 3, device=dev), torch.empty(B, J, 3, device=dev)
        d_w2, d_b2, d_h = torch.empty(4 * J, 40, device=dev), torch.empty(4 * J, device=dev), torch.empty(B, 40, device=dev)
        grads = {k: [[torch.empty_like(d[f"p{t}.{l}.{k}"]) for l in range(spec.layers(t))] for t in range(3)] for k in ("w", "b", "gamma", "beta")}
        gtab = gen.pointer_table(_ffi.PgGenGrads(), spec, grads)
        _ffi.call(renderer, "pg_gen_trunk_forward", C.byref(cs), C.byref(tab), noise, B, 1, tape, stats)
        _ffi.call(renderer, "pg_gen_ba_head_forward", C.byref(cs), 0, tape, B, J, d["w2"], d["b2"], y, pose)
        _ffi.call(renderer, "pg_gen_rt_head", C.byref(cs), 2, 1, tape, B, J, d["w2t"], d["b2t"], d["eps"], d["x"], R, T, pose_rt)
        _ffi.call(renderer, "pg_gen_ba_head_backward", C.byref(cs), 0, tape, B, J, d["w2"], y, d["d_pose"], d_w2, d_b2, d_h)
        _ffi.call(renderer, "pg_gen_trunk_backward", C.byref(cs), C.byref(tab), noise, B, 1, tape, stats, gen.pointer_array([d_h, d["cot1"], None]),
                  C.byref(gtab))
        # an eval-mode forward in the same queue, on a tape of its own
        tape_e, stats_e = torch.empty(n_f, device=dev), torch.empty(n_d, dtype=torch.float64, device=dev)
        _ffi.call(renderer, "pg_gen_trunk_forward", C.byref(cs), C.byref(tab), noise, B, 0, tape_e, stats_e)
        out = {"tape": tape, "stats": stats, "y": y, "pose": pose, "R": R, "T": T, "pose_rt": pose_rt, "d_w2": d_w2, "d_b2": d_b2, "d_h": d_h,
               "tape_e": tape_e, "stats_e": stats_e}
        for t in range(2):                                                     # (trunk 2 has no cotangent: its gradients are not written)
            for l in range(spec.layers(t)):
                out.update({f"g{t}.{l}.{k}": grads[k][t][l] for k in grads})
        for t in range(3):
            for l in range(spec.layers(t)):
                out[f"rm{t}.{l}"], out[f"rv{t}.{l}"] = d[f"p{t}.{l}.rm"], d[f"p{t}.{l}.rv"]
        return out
    rep = sh.run_decoy("generator_entry_points", make, run, side, delay, dev, pend=True)
    assert rep["pending"]


def test_the_module_on_a_busy_side_stream(renderer, env):
    dev, side, delay = env
    module = gen.HipPoseGenerator(renderer=renderer)
    names = list(module.state_dict().keys())

    def make(v):
        sd = ref.make_state_dict(module, 40 + SEEDS[v])
        rng = np.random.RandomState(50 + SEEDS[v])
        d = {f"sd.{k}": torch.as_tensor(sd[k]) for k in names}
        d.update({"ba": torch.tensor(rng.standard_normal((B, 32)).astype(np.float32)), "r": torch.tensor(rng.standard_normal((B, 72)).astype(np.float32)),
                  "eps": torch.tensor(rng.standard_normal((B, 3)).astype(np.float32)), "t": torch.tensor(rng.standard_normal((B, 72)).astype(np.float32)),
                  "x": torch.tensor(rng.standard_normal((B, 24, 3)).astype(np.float32))})
        return d, None

    def run(d, _host):
        m = module
        # the module's tensors ARE the case's inputs (no copy: the real values arrive behind the delay)
        for k in names:
            owner, leaf = m, k.split(".")
            for part in leaf[:-1]:
                owner = getattr(owner, part)
            if leaf[-1] in owner._parameters:
                owner._parameters[leaf[-1]] = torch.nn.Parameter(d[f"sd.{k}"])
            else:
                owner._buffers[leaf[-1]] = d[f"sd.{k}"]
        m.train()
        out = m(d["x"], noise={k: d[k] for k in ("ba", "r", "eps", "t")})
        out["pose_ba"].backward(d["x"])                                        # (any cotangent that differs between the variants)
        res = {k: out[k] for k in ("pose_ba", "R", "T", "pose_rt")}
        res.update({f"grad.{k}": p.grad for k, p in m.named_parameters() if p.grad is not None})
        res.update({f"buf.{k}": b for k, b in m.named_buffers()})
        return res
    rep = sh.run_decoy("generator_module", make, run, side, delay, dev, pend=True)
    assert rep["pending"]
