"""The two compute entry points of include/posegen_regressor.h and `HipHMRHead` on a busy, non-blocking side stream
(tests/stream_harness.run_decoy, the pattern of tests/test_gpu_generator_streams.py): decoy inputs, the real ones copied in behind a
>= 50 ms delay, two calls back to back with different inputs; both results must be the default-stream bytes, and the delay must
still be pending when the calls have returned -- the header documents both as asynchronous.  The parameters travel with the inputs."""
import ctypes as C
import re

import numpy as np
import pytest
import torch

from posegen_amd import _ffi, regressors as reg
from tests import hmr_ref as ref
from tests import stream_harness as sh
from tests.frame_metrics_gpu import DEV, renderer  # noqa: F401 (renderer: a fixture)

pytestmark = pytest.mark.gpu
SEEDS = {"A": 1, "A2": 2, "B": 3}
B = 70


@pytest.fixture(scope="module")
def env():
    dev = torch.device(DEV)
    side = torch.cuda.Stream(dev)
    return dev, side, sh.Delay(side, dev)


def test_the_header_documents_the_compute_entry_points_as_asynchronous():
    with open(sh.HEADER.replace("posegen_hip.h", "posegen_regressor.h")) as f:
        text = f.read()
    names = sh.stream_entry_points(text)
    assert names == ["pg_hmr_head_forward", "pg_hmr_head_backward"]
    for name in names:
        body = text[:text.index(f"int {name}(")]
        prose = re.sub(r"\s*\n\s*\*?\s*", " ", body[body.rindex("/*"):])          # (line breaks of the comment become one space)
        assert "Asynchronous on `stream`" in prose, name


def _make(spec, v):
    rng = np.random.RandomState(60 + SEEDS[v])
    sd = ref.make_state_dict(spec, 20 + SEEDS[v])
    d = {f"sd.{k}": torch.tensor(a) for k, a in sd.items()}
    d.update({"xf": torch.tensor(rng.standard_normal((B, spec.n_feat)).astype(np.float32)),
              "init": torch.tensor(rng.standard_normal((B, spec.n_state)).astype(np.float32)),
              "masks": torch.tensor(ref.make_masks(spec, B, 30 + SEEDS[v])),
              "d_rotmat": torch.tensor(rng.standard_normal((B, spec.n_joints, 3, 3)).astype(np.float32)),
              "d_shape": torch.tensor(rng.standard_normal((B, spec.n_shape)).astype(np.float32)),
              "d_cam": torch.tensor(rng.standard_normal((B, spec.n_cam)).astype(np.float32))})
    return d, None


def test_both_entry_points_on_a_busy_side_stream(renderer, env):
    dev, side, delay = env
    spec = ref.toy_spec()
    cs = spec.c_spec()
    n_f = spec.tape_layout(B)[1]
    names = [f"sd.{lin}.{leaf}" for lin in ref.LINEARS for leaf in ("weight", "bias")]

    def run(d, _host):
        tab = reg.pointer_table(_ffi.PgHmrParams(), [d[k] for k in names])
        tape = torch.empty(n_f, device=dev)
        rotmat, shape, cam = torch.empty(B, spec.n_joints, 3, 3, device=dev), torch.empty(B, spec.n_shape, device=dev), torch.empty(B, spec.n_cam, device=dev)
        grads = [torch.empty_like(d[k]) for k in names]
        gtab = reg.pointer_table(_ffi.PgHmrGrads(), grads)
        d_xf, d_init = torch.empty(B, spec.n_feat, device=dev), torch.empty(B, spec.n_state, device=dev)
        _ffi.call(renderer, "pg_hmr_head_forward", C.byref(cs), C.byref(tab), d["xf"], d["init"], 1, d["masks"], B, tape, rotmat, shape, cam)
        _ffi.call(renderer, "pg_hmr_head_backward", C.byref(cs), C.byref(tab), d["xf"], d["masks"], B, tape, d["d_rotmat"], d["d_shape"], d["d_cam"],
                  C.byref(gtab), d_xf, d_init)
        # an eval-mode forward in the same queue, on a tape of its own, from the shared init
        tape_e, rot_e = torch.empty(n_f, device=dev), torch.empty(B, spec.n_joints, 3, 3, device=dev)
        _ffi.call(renderer, "pg_hmr_head_forward", C.byref(cs), C.byref(tab), d["xf"], d["init"], 0, None, B, tape_e, rot_e, None, None)
        out = {"tape": tape, "rotmat": rotmat, "shape": shape, "cam": cam, "d_xf": d_xf, "d_init": d_init, "tape_e": tape_e, "rot_e": rot_e}
        out.update({f"g.{k}": g for k, g in zip(names, grads)})
        return out
    rep = sh.run_decoy("hmr_entry_points", lambda v: _make(spec, v), run, side, delay, dev, pend=True)
    assert rep["pending"]


def test_the_module_on_a_busy_side_stream(renderer, env):
    dev, side, delay = env
    spec = ref.toy_spec()
    module = reg.HipHMRHead(spec.n_feat, spec.n_hidden, spec.n_joints, spec.n_shape, spec.n_cam, spec.p_drop, renderer=renderer).to(dev)
    keys = list(module.state_dict().keys())

    def run(d, _host):
        m = module
        # the module's tensors ARE the case's inputs (no copy: the real values arrive behind the delay)
        for k in keys:
            owner, leaf = m, k.split(".")
            for part in leaf[:-1]:
                owner = getattr(owner, part)
            if leaf[-1] in owner._parameters:
                owner._parameters[leaf[-1]] = torch.nn.Parameter(d[f"sd.{k}"])
            else:
                owner._buffers[leaf[-1]] = d[f"sd.{k}"]
        m.train()
        xf = d["xf"].detach().requires_grad_(True)
        outs = m(xf, masks=d["masks"])
        torch.autograd.backward(outs, [d["d_rotmat"], d["d_shape"], d["d_cam"]])
        res = {"rotmat": outs[0], "shape": outs[1], "cam": outs[2], "d_xf": xf.grad}
        res.update({f"grad.{k}": p.grad for k, p in m.named_parameters()})
        return res
    rep = sh.run_decoy("hmr_module", lambda v: _make(spec, v), run, side, delay, dev, pend=True)
    assert rep["pending"]
