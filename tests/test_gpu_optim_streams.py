"""pg_adam_step (include/posegen_optim.h) and `HipAdam.step` on a busy, non-blocking side stream (tests/stream_harness.run_decoy, the
pattern of tests/test_gpu_hmr_streams.py): decoy inputs, the real ones copied in behind a >= 50 ms delay, two calls back to back with
different tables and different groups, with clipping and `out`; the updated p, m, v and `out` of both must be the default-stream
bytes, and the delay must still be pending when the calls have returned -- the header documents the call as asynchronous.  This is
what catches a host table that the second call overwrites under the first one's upload, or a kernel on stream 0."""
import re

import numpy as np
import pytest
import torch

from posegen_amd import _ffi, optim
from tests import optim_gpu as og
from tests import optim_ref as ref
from tests import stream_harness as sh
from tests.frame_metrics_gpu import DEV, renderer  # noqa: F401 (renderer: a fixture)

pytestmark = pytest.mark.gpu
SEG = ref.SEG
FLAT = 2 * SEG + 4096
# the two back-to-back calls differ in their tables (counts, order, groups, steps) and in their groups' numbers
SPECS = {"A": ((300, SEG + 5, 77), (0, 1, 0), 3, 1.0), "A2": ((SEG + 5, 77, 300, 9), (1, 1, 0, 0), 5, 0.4), "B": ((300, SEG + 5, 77), (0, 1, 0), 3, 1.0)}
SEEDS = {"A": 1, "A2": 2, "B": 3}


@pytest.fixture(scope="module")
def env():
    dev = torch.device(DEV)
    side = torch.cuda.Stream(dev)
    return dev, side, sh.Delay(side, dev)


def test_the_header_documents_the_call_as_asynchronous():
    with open(sh.HEADER.replace("posegen_hip.h", "posegen_optim.h")) as f:
        text = f.read()
    assert sh.stream_entry_points(text) == ["pg_adam_step"]
    body = text[:text.index("int pg_adam_step(")]
    assert "Asynchronous on `stream`" in re.sub(r"\s*\n\s*\*?\s*", " ", body[body.rindex("/*"):])


def _make(v):
    counts, group_of, step, max_norm = SPECS[v]
    rng = np.random.RandomState(70 + SEEDS[v])
    tensors = [ref.make_tensor(rng, c, group=g, step=step + i) for i, (c, g) in enumerate(zip(counts, group_of))]
    lay = og.Layout(tensors)
    assert all(lay.size[k] <= FLAT for k in og.KINDS)
    dev = {}
    for k in og.KINDS:
        a = np.full(FLAT, og.SENT, np.float32)
        a[:lay.size[k]] = lay.flat(tensors, k)
        dev[k] = torch.tensor(a)
    groups = [dict(q, lr=q["lr"] * (1 + SEEDS[v])) for q in ref.GROUPS]
    return dev, (tensors, lay, groups, max_norm)


def test_two_calls_back_to_back_on_a_busy_side_stream(renderer, env):
    dev, side, delay = env

    def run(d, host):
        tensors, lay, groups, max_norm = host
        out = torch.empty(2, dtype=torch.float64, device=dev)
        og.enqueue(renderer, og.tensor_table(tensors, lay, d), og.groups_table(groups), max_norm, True, out)
        return {"p": d["p"], "g": d["g"], "m": d["m"], "v": d["v"], "out": out}
    rep = sh.run_decoy("adam_step", _make, run, side, delay, dev, pend=True)
    assert rep["pending"]


def test_hipadam_step_on_a_busy_side_stream(renderer, env):
    dev, side, delay = env

    def run(d, host):
        tensors, lay, groups, max_norm = host
        params = []
        for i, (t, c) in enumerate(zip(tensors, lay.counts)):
            view = {k: d[k][lay.off[k][i]:lay.off[k][i] + c] for k in og.KINDS}
            p = torch.nn.Parameter(view["p"])                      # the case's buffers ARE the parameters: the real values arrive behind the delay
            p.grad = view["g"]
            params.append((p, view, t))
        opt = optim.HipAdam([{"params": [p for p, _, t in params if t["group"] == g], **groups[g]} for g in range(len(groups))], renderer=renderer)
        for p, view, t in params:
            opt.state[p] = {"step": torch.tensor(float(t["step"] - 1)), "exp_avg": view["m"], "exp_avg_sq": view["v"]}
        norm = opt.step(max_norm=max_norm)
        assert norm.is_cuda and norm.dtype == torch.float64
        return {"p": d["p"], "g": d["g"], "m": d["m"], "v": d["v"], "out": opt.last_norm_coef, "norm": norm.reshape(1)}
    rep = sh.run_decoy("hipadam_step", _make, run, side, delay, dev, pend=True)
    assert rep["pending"]
