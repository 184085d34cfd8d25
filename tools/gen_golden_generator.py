#!/usr/bin/env python3
"""tests/golden/pose_generator.npz: the reference's pose generator on recorded draws.

`Linear`, `BAGenerator`, `RTGenerator` and `PoseGenerator` are lifted out of the reference's run_gan.py (:767-980) by
tools/gen_golden._reference_definitions and run in float64 on the CPU, in training mode, on weights made from a seed
(tests/generator_ref.make_state_dict: gamma, beta and the running statistics are not the initial ones), B = 5 poses.  The classes draw
their noise with torch.randn and torch.normal; here those two names hand out draws that were made beforehand from a stored seed, and
the draws themselves are stored (not a torch seed).  pytorch3d is not installed: `axis_angle_to_matrix` is the one function of the
run that is restated (tests/generator_ref.axis_angle_to_matrix, the quaternion route in float64); the fixture says so.

Stored: the seeds, the input poses, the draws (`noise_ba`, `noise_r`, `eps`, `noise_t`), `pose_ba`, `R`, `T`, `pose_rt`, the running
statistics and num_batches_tracked after the call, and for the loss 0.5 mean((pose_ba - c)^2) every parameter gradient as sum,
absolute sum and eight samples (NaN where the reference leaves `grad None`), the state-dict keys and shapes.

    python tools/gen_golden_generator.py [--ref REFERENCE_ROOT] [--out tests/golden]
"""
import argparse
import os
import sys

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

WEIGHT_SEED, NOISE_SEED, INPUT_SEED, TARGET_SEED, BATCH = 11, 12, 13, 14, 5


class _RecordedTorch:
    """`torch` for the lifted classes: everything is torch's own, except that randn and normal hand out the prepared draws in order"""

    def __init__(self, torch, draws):
        self._torch, self._draws, self.used = torch, list(draws), []

    def __getattr__(self, name):
        return getattr(self._torch, name)

    def _next(self, shape):
        name, a = self._draws.pop(0)
        assert tuple(a.shape) == tuple(shape), (name, a.shape, shape)
        self.used.append(name)
        return self._torch.tensor(a, dtype=self._torch.float64)

    def randn(self, *shape, device=None):
        return self._next(shape)

    def normal(self, mean, std):
        return mean + std * self._next(mean.shape)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--ref", default=os.environ.get("POSEGEN_REFERENCE", ""))
    ap.add_argument("--out", default=os.path.join(REPO, "tests", "golden"))
    a = ap.parse_args()
    if not a.ref:
        sys.exit("gen_golden_generator: --ref (or POSEGEN_REFERENCE) names the reference's root")
    import types
    import torch
    import torch.nn as nn
    from posegen_amd import generators
    from tests import generator_ref as ref
    from tools.gen_golden import _reference_definitions

    rng = np.random.RandomState(NOISE_SEED)
    draws = [("noise_ba", rng.standard_normal((BATCH, 32)).astype(np.float32)), ("noise_r", rng.standard_normal((BATCH, 72)).astype(np.float32)),
             ("eps", rng.standard_normal((BATCH, 3)).astype(np.float32)), ("noise_t", rng.standard_normal((BATCH, 72)).astype(np.float32))]
    rec = _RecordedTorch(torch, draws)
    torch3d = types.SimpleNamespace(axis_angle_to_matrix=lambda v: torch.tensor(ref.axis_angle_to_matrix(v.detach().numpy())))
    rg = _reference_definitions(os.path.join(a.ref, "run_gan.py"), ["Linear", "BAGenerator", "RTGenerator", "PoseGenerator"],
                                extra={"nn": nn, "torch": rec, "torch3d": torch3d})
    model = rg["PoseGenerator"](None).double()
    model.train()
    keys = list(model.state_dict().keys())
    ours = generators.HipPoseGenerator()
    sd = ref.make_state_dict(ours, WEIGHT_SEED)
    model.load_state_dict({k: torch.tensor(v).double() if k.endswith(("weight", "bias", "running_mean", "running_var")) else torch.tensor(v)
                           for k, v in sd.items()}, strict=True)
    x = np.random.RandomState(INPUT_SEED).standard_normal((BATCH, 24, 3)).astype(np.float32)
    target = np.random.RandomState(TARGET_SEED).standard_normal((BATCH, 24, 3)).astype(np.float32)
    out = model(torch.tensor(x).double())
    assert rec.used == [n for n, _ in draws] and not rec._draws, rec.used          # the reference's draw order
    loss = 0.5 * ((out["pose_ba"] - torch.tensor(target).double()) ** 2).mean()
    loss.backward()
    d = {"weight_seed": np.int64(WEIGHT_SEED), "noise_seed": np.int64(NOISE_SEED), "input_seed": np.int64(INPUT_SEED),
         "target_seed": np.int64(TARGET_SEED), "x": x, "target": target, "restated": np.asarray(["pytorch3d.transforms.axis_angle_to_matrix"]),
         "draw_order": np.asarray(rec.used), "loss": np.float64(loss.item())}
    d.update(dict(draws))
    for k in ("pose_ba", "R", "T", "pose_rt"):
        d[k] = out[k].detach().numpy()
    after = model.state_dict()
    d["keys"] = np.asarray(keys)
    d["shapes"] = np.asarray([",".join(str(n) for n in after[k].shape) for k in keys])
    stat_keys = [k for k in keys if k.endswith(("running_mean", "running_var"))]
    d["stat_keys"] = np.asarray(stat_keys)
    d["stats_after"] = np.concatenate([after[k].numpy().reshape(-1) for k in stat_keys])
    d["batches_tracked_after"] = np.asarray([int(after[k]) for k in keys if k.endswith("num_batches_tracked")], dtype=np.int64)
    named = dict(model.named_parameters())
    pkeys = list(named)
    d["param_keys"] = np.asarray(pkeys)
    d["grad_none"] = np.asarray([named[k].grad is None for k in pkeys])
    nan = float("nan")
    d["grad_sum"] = np.asarray([nan if named[k].grad is None else named[k].grad.sum().item() for k in pkeys])
    d["grad_abs_sum"] = np.asarray([nan if named[k].grad is None else named[k].grad.abs().sum().item() for k in pkeys])
    d["grad_samples"] = np.concatenate([np.full(len(ref.grad_sample_index(named[k].numel())), nan) if named[k].grad is None else
                                        named[k].grad.reshape(-1)[ref.grad_sample_index(named[k].numel())].numpy() for k in pkeys])
    path = os.path.join(a.out, "pose_generator.npz")
    np.savez_compressed(path, **d)
    print(f"[pose_generator] {os.path.getsize(path)} bytes; {int(d['grad_none'].sum())} of {len(pkeys)} parameters without a gradient")


if __name__ == "__main__":
    main()
