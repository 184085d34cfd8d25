"""The four compute entry points of include/posegen_gan.h and `FakePool` on a busy, non-blocking side stream
(tests/stream_harness.run_decoy, as tests/test_gpu_streams.py runs the entry points of posegen_hip.h): decoy inputs, the real ones
copied in behind a >= 50 ms delay, two calls back to back with different host arrays; both results must be the default-stream
bytes, and the delay must still be pending when the calls have returned -- the header documents all four as asynchronous."""
import ctypes as C
import re

import numpy as np
import pytest
import torch

from posegen_amd import _ffi, discriminators as disc
from tests import gan_ref
from tests import stream_harness as sh
from tests.frame_metrics_gpu import DEV, renderer  # noqa: F401 (renderer: a fixture)

pytestmark = pytest.mark.gpu
SEEDS = {"A": 1, "A2": 2, "B": 3}


@pytest.fixture(scope="module")
def env():
    dev = torch.device(DEV)
    side = torch.cuda.Stream(dev)
    return dev, side, sh.Delay(side, dev)


def test_the_header_documents_the_compute_entry_points_as_asynchronous():
    with open(sh.HEADER.replace("posegen_hip.h", "posegen_gan.h")) as f:
        text = f.read()
    for name in sh.stream_entry_points(text):
        body = text[:text.index(f"int {name}(")]
        prose = re.sub(r"\s*\n\s*\*?\s*", " ", body[body.rindex("/*"):])          # (line breaks of the comment become one space)
        assert "Asynchronous on `stream`" in prose, name


def test_forward_and_backward_on_a_busy_side_stream(renderer, env):
    dev, side, delay = env
    spec = gan_ref.toy_spec()
    params = [torch.tensor(a, device=dev) for layers in gan_ref.make_params(spec, 5) for wb in layers for a in wb]
    B = 70                                                                  # two row tiles
    cs, tab = spec.c_spec(), disc._pointer_table(spec, params)
    n = C.c_int64(0)
    renderer._check(renderer.lib.pg_disc_tape_floats(C.byref(cs), B, C.byref(n)))

    def make(v):
        rng = np.random.RandomState(SEEDS[v])
        return {"x": torch.tensor(gan_ref.make_inputs(spec, B, SEEDS[v])), "d_pred": torch.tensor(rng.standard_normal((B, 2)).astype(np.float32))}, None

    def run(d, _host):
        pred, tape = torch.empty(B, 2, device=dev), torch.empty(n.value, device=dev)
        d_x, grads = torch.empty_like(d["x"]), [torch.empty_like(p) for p in params]
        gtab = disc._pointer_table(spec, grads)
        _ffi.call(renderer, "pg_disc_forward", C.byref(cs), C.byref(tab), d["x"], B, pred, tape)
        _ffi.call(renderer, "pg_disc_backward", C.byref(cs), C.byref(tab), d["x"], B, tape, d["d_pred"], d_x, C.byref(gtab))
        # a forward without a tape of its own (the handle's workspace) and a backward without gradients, in the same queue
        pred_ws = torch.empty(B, 2, device=dev)
        _ffi.call(renderer, "pg_disc_forward", C.byref(cs), C.byref(tab), d["x"], B, pred_ws, None)
        d_x_only = torch.empty_like(d["x"])
        _ffi.call(renderer, "pg_disc_backward", C.byref(cs), C.byref(tab), d["x"], B, tape, d["d_pred"], d_x_only, None)
        out = {"pred": pred, "tape": tape, "d_x": d_x, "pred_ws": pred_ws, "d_x_only": d_x_only}
        out.update({f"g{i}": g for i, g in enumerate(grads)})
        return out
    rep = sh.run_decoy("disc_forward_backward", make, run, side, delay, dev, pend=True)
    assert rep["pending"]


def test_the_loss_on_a_busy_side_stream(renderer, env):
    dev, side, delay = env

    def make(v):
        return {"pred": torch.tensor(np.random.RandomState(SEEDS[v]).standard_normal(7 * 130).astype(np.float32))}, float(SEEDS[v] % 2)

    def run(d, label):
        out, d_pred = torch.empty(3, dtype=torch.float64, device=dev), torch.empty_like(d["pred"])
        _ffi.call(renderer, "pg_disc_loss", d["pred"], d["pred"].numel(), label, 0.5, out, d_pred)
        return {"out": out, "d_pred": d_pred}
    assert sh.run_decoy("disc_loss", make, run, side, delay, dev, pend=True)["pending"]


def _pool_inputs(v, cap, n, row):
    rng = np.random.RandomState(10 + SEEDS[v])
    dev_in = {"pool": torch.tensor(rng.standard_normal((cap, row)).astype(np.float32)), "items": torch.tensor(rng.standard_normal((n, row)).astype(np.float32))}
    return dev_in, ((rng.uniform(size=n) > 0.4).astype(np.uint8), rng.randint(0, cap, size=n).astype(np.int32))


def test_the_pool_exchange_on_a_busy_side_stream(renderer, env):
    dev, side, delay = env
    cap, n, row = 16, 24, 8                                                  # more items than slots: every slot hit more than once

    def make(v):
        dev_in, (swap, slot) = _pool_inputs(v, cap, n, row)
        dev_in["swap"], dev_in["slot"] = torch.tensor(swap), torch.tensor(slot)
        return dev_in, None

    def run(d, _host):
        pool, out = d["pool"].clone(), torch.empty_like(d["items"])
        _ffi.call(renderer, "pg_pool_exchange", pool, cap, row, cap - 5, d["items"], n, d["swap"], d["slot"], out)
        return {"out": out, "pool": pool}
    assert sh.run_decoy("pool_exchange", make, run, side, delay, dev, pend=True)["pending"]


def test_fake_pool_uploads_its_draws_without_waiting(renderer, env):
    """`FakePool.exchange` with host draws: the second call's draws must not reach the first call (the staging array is per call),
    and neither call may wait for the stream"""
    dev, side, delay = env
    cap, n, row = 16, 24, 8

    def make(v):
        return _pool_inputs(v, cap, n, row)

    def run(d, host):
        pool = disc.FakePool(cap, renderer)
        pool.pool, pool.cur = d["pool"].clone(), cap
        out = pool.exchange(d["items"], host[0], host[1])
        return {"out": out, "pool": pool.pool}
    assert sh.run_decoy("fake_pool", make, run, side, delay, dev, pend=True)["pending"]
