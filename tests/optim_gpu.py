"""What tests/test_gpu_optim.py and tests/test_gpu_optim_streams.py share: pg_adam_step through the C ABI on tensors laid out as
views into flat device buffers (one buffer per kind: p, g, m, v) at chosen 4-byte phases with eight guard elements on each side of
every view, and the comparison with the float64 restatement (tests/optim_ref.py)."""
import numpy as np
import torch

from posegen_amd import _ffi
from tests import optim_ref as ref
from tests.frame_metrics_gpu import DEV

KINDS = ("p", "g", "m", "v")
GUARD = 8
SENT = np.float32(-7777.25)


class Layout:
    """Element offsets of every tensor's four views.  phases: per tensor a 4-tuple of element phases (0..3, times 4 bytes) for p, g,
    m, v (None: all four on phase i mod 4, so that the 16-byte path runs behind a scalar head)."""

    def __init__(self, tensors, phases=None):
        self.counts = [len(t["p"]) for t in tensors]
        self.off = {k: [] for k in KINDS}
        cursor = {k: 0 for k in KINDS}
        for i, c in enumerate(self.counts):
            ph = phases[i] if phases is not None else (i % 4,) * 4
            for k, f in zip(KINDS, ph):
                start = (cursor[k] + 3) // 4 * 4 + GUARD + f         # (GUARD is a multiple of four elements: the phase is f)
                self.off[k].append(start)
                cursor[k] = start + c + GUARD
        self.size = {k: cursor[k] + 4 for k in KINDS}

    def flat(self, tensors, k):
        a = np.full(self.size[k], SENT, np.float32)
        for t, o, c in zip(tensors, self.off[k], self.counts):
            a[o:o + c] = t[k]
        return a

    def mask(self, k):
        m = np.zeros(self.size[k], bool)
        for o, c in zip(self.off[k], self.counts):
            m[o:o + c] = True
        return m


def groups_table(groups):
    g = (_ffi.PgAdamGroup * len(groups))()
    for q, d in zip(g, groups):
        q.lr, (q.beta1, q.beta2), q.eps, q.weight_decay = d["lr"], d["betas"], d["eps"], d["weight_decay"]
    return g


def tensor_table(tensors, layout, bufs):
    tab = (_ffi.PgAdamTensor * len(tensors))()
    for i, (e, t) in enumerate(zip(tab, tensors)):
        for k, field in zip(KINDS, ("param", "grad", "exp_avg", "exp_avg_sq")):
            setattr(e, field, bufs[k].data_ptr() + 4 * layout.off[k][i])
        e.count, e.group, e.step = layout.counts[i], t["group"], t["step"]
    return tab


def enqueue(renderer, tab, groups, max_norm, write_grads, out):
    """one pg_adam_step on the current stream"""
    _ffi.call(renderer, "pg_adam_step", len(tab), tab, len(groups), groups, _ffi.PG_ADAM_NO_CLIP if max_norm is None else float(max_norm),
              int(write_grads), out)


def device_step(renderer, tensors, groups, max_norm=None, write_grads=False, want_out=True, phases=None):
    """pg_adam_step on `tensors` -> {flat: {kind: float32 array}, tensors: [{p, g, m, v}], norm, coef}; asserts that every byte outside
    the views is untouched (and, without write_grads, every gradient byte)."""
    lay = Layout(tensors, phases)
    host = {k: lay.flat(tensors, k) for k in KINDS}
    bufs = {k: torch.tensor(host[k], device=DEV) for k in KINDS}
    assert all(bufs[k].data_ptr() % 16 == 0 for k in KINDS)
    out = torch.full((2,), -3.0, dtype=torch.float64, device=DEV) if want_out else None
    enqueue(renderer, tensor_table(tensors, lay, bufs), groups_table(groups), max_norm, write_grads, out)
    torch.cuda.synchronize()
    flat = {k: bufs[k].cpu().numpy() for k in KINDS}
    for k in KINDS:
        outside = ~lay.mask(k)
        assert np.array_equal(flat[k][outside].view(np.uint32), host[k][outside].view(np.uint32)), f"bytes outside the views of {k} were written"
    if not write_grads:
        assert np.array_equal(flat["g"].view(np.uint32), host["g"].view(np.uint32)), "the gradients were written without write_grads"
    res = [{k: flat[k][lay.off[k][i]:lay.off[k][i] + c] for k in KINDS} for i, c in enumerate(lay.counts)]
    norm, coef = (float(x) for x in out.cpu().numpy()) if want_out else (None, None)
    return {"flat": flat, "tensors": res, "norm": norm, "coef": coef}


def same_bytes(a, b):
    return a.shape == b.shape and np.array_equal(np.ascontiguousarray(a).view(np.uint32), np.ascontiguousarray(b).view(np.uint32))


def hold_to_bound(name, dev, tensors, groups, max_norm, write_grads, record):
    """the device's out against the restatement's to 1e-14, then every element against the restatement that uses the device's own
    coefficient, under the bound.  record[name] = (share of the bound, share of bitwise-equal elements)."""
    r0 = ref.adam_step(tensors, groups, max_norm)
    if dev["norm"] is not None:
        if np.isfinite(r0["norm"]):
            assert abs(dev["norm"] - r0["norm"]) <= 1e-14 * r0["norm"], (name, dev["norm"], r0["norm"])
            assert abs(dev["coef"] - r0["coef"]) <= 1e-14 * r0["coef"], (name, dev["coef"], r0["coef"])
        else:
            assert (np.isnan(dev["norm"]) and np.isnan(r0["norm"])) or dev["norm"] == r0["norm"], (name, dev["norm"], r0["norm"])
            assert (np.isnan(dev["coef"]) and np.isnan(r0["coef"])) or dev["coef"] == r0["coef"], (name, dev["coef"], r0["coef"])
    coef = dev["coef"] if (dev["coef"] is not None and max_norm is not None) else None
    r = ref.adam_step(tensors, groups, max_norm, coef=coef)
    devs = [dict(t) for t in dev["tensors"]]
    worst, equal, bad = ref.judge(devs, r["tensors"], write_grads=write_grads)
    record[name] = (worst, equal)
    print(f"BOUND {name}: {worst:.3f} of the bound, {equal:.5f} of the elements bitwise float32(f64)")
    assert not bad and worst <= 1.0, (name, bad[:6])
    return r
