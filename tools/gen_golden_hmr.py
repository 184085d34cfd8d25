#!/usr/bin/env python3
"""tests/golden/hmr_head.npz: the reference's HMR regressor on recorded dropout masks.

`rot6d_to_rotmat`, `Bottleneck` and `HMR` are lifted out of the reference's run_gan.py (:1188-1358) by
tools/gen_golden._reference_definitions and run in float64 on the CPU as HMR(Bottleneck, [1, 1, 1, 1], <mean parameters made from a
seed>) on B = 5 images of 224 x 224, once in eval mode and once in training mode.  The head's weights come from a seed
(tests/hmr_ref.make_state_dict; the 9 MB fc1.weight is never stored), the trunk's from the class's own initialisation: what the trunk
hands to the head, `xf`, is captured with a hook on `avgpool` and stored.  The classes build their Dropouts with nn.Dropout; here that
one name gives modules that apply masks recorded beforehand from a stored seed, in the order the reference calls them (round 0 drop1,
round 0 drop2, round 1, ...), and the masks themselves are stored (bit-packed).

Stored: the seeds, `xf`, the masks, the mean parameters, `pred_rotmat` / `pred_shape` / `pred_cam` of both runs, and for the
training-mode run the loss 0.5 (mean (pred_rotmat - T_r)^2 + mean (pred_shape - T_s)^2 + mean (pred_cam - T_c)^2), `d_xf` in full and
every head parameter's gradient as sum, absolute sum and eight samples; the head's state-dict keys and shapes.

    python tools/gen_golden_hmr.py [--ref REFERENCE_ROOT] [--out tests/golden]
"""
import argparse
import math
import os
import sys
import tempfile

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

WEIGHT_SEED, MASK_SEED, IMAGE_SEED, TARGET_SEED, TRUNK_SEED, BATCH = 41, 42, 43, 44, 45, 5


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--ref", default=os.environ.get("POSEGEN_REFERENCE", ""))
    ap.add_argument("--out", default=os.path.join(REPO, "tests", "golden"))
    a = ap.parse_args()
    if not a.ref:
        sys.exit("gen_golden_hmr: --ref (or POSEGEN_REFERENCE) names the reference's root")
    import torch
    import torch.nn as nn
    import torch.nn.functional as F
    from tests import hmr_ref as ref
    from tools.gen_golden import _reference_definitions

    spec = ref.shipped_spec()
    masks = ref.make_masks(spec, BATCH, MASK_SEED)
    feed = []

    class RecordedDropout(nn.Module):
        """nn.Dropout for the lifted HMR: in training mode the next recorded mask, a kept element times 1 / (1 - p)"""

        def __init__(self, p=0.5):
            super().__init__()
            self.p = p

        def forward(self, x):
            if not self.training:
                return x
            return torch.where(feed.pop(0), x * (1.0 / (1.0 - self.p)), torch.zeros((), dtype=x.dtype))

    class RecordedNN:
        """`nn` for the lifted classes: torch.nn's own names, except Dropout"""
        Dropout = RecordedDropout

        def __getattr__(self, name):
            return getattr(nn, name)

    rg = _reference_definitions(os.path.join(a.ref, "run_gan.py"), ["rot6d_to_rotmat", "Bottleneck", "HMR"],
                                extra={"nn": RecordedNN(), "F": F, "math": math})
    sd = ref.make_state_dict(spec, WEIGHT_SEED)
    mean = {"pose": sd["init_pose"].reshape(-1), "shape": sd["init_shape"].reshape(-1), "cam": sd["init_cam"].reshape(-1)}
    torch.manual_seed(TRUNK_SEED)
    with tempfile.TemporaryDirectory() as tmp:
        path = os.path.join(tmp, "smpl_mean_params.npz")
        np.savez(path, **mean)
        model = rg["HMR"](rg["Bottleneck"], [1, 1, 1, 1], path).double()
    missing, unexpected = model.load_state_dict({k: torch.tensor(sd[k]).double() for k in ref.HEAD_KEYS}, strict=False)
    assert not unexpected and not [k for k in missing if k.split(".")[0] in ref.LINEARS], (missing, unexpected)
    head_keys = [k for k in model.state_dict() if k.split(".")[0] in ref.LINEARS + ref.INIT_KEYS]
    caught = {}
    model.avgpool.register_forward_hook(lambda m, i, o: (o.retain_grad() if o.requires_grad else None, caught.__setitem__("xf", o))[-1])
    images = np.random.RandomState(IMAGE_SEED).standard_normal((BATCH, 3, 224, 224)).astype(np.float32)
    x = torch.tensor(images).double()
    d = {"weight_seed": np.int64(WEIGHT_SEED), "mask_seed": np.int64(MASK_SEED), "image_seed": np.int64(IMAGE_SEED),
         "target_seed": np.int64(TARGET_SEED), "trunk_seed": np.int64(TRUNK_SEED), "p_drop": np.float64(model.drop1.p),
         "masks_packed": ref.pack_masks(masks), "masks_shape": np.asarray(masks.shape, np.int64),
         "mean_pose": mean["pose"], "mean_shape": mean["shape"], "mean_cam": mean["cam"]}
    model.eval()
    with torch.no_grad():
        out = model(x)
    d["xf"] = caught["xf"].detach().reshape(BATCH, -1).numpy()
    for k, o in zip(("pred_rotmat", "pred_shape", "pred_cam"), out):
        d[f"eval_{k}"] = o.numpy()
    model.train()
    for m in model.modules():                                                 # train_spin freezes the BatchNorm statistics; the stored xf is the eval run's
        if isinstance(m, nn.BatchNorm2d):
            m.eval()
    feed.extend(torch.tensor(masks[i, w] != 0) for i in range(spec.n_iter) for w in range(2))
    out = model(x)
    assert not feed
    assert np.array_equal(caught["xf"].detach().reshape(BATCH, -1).numpy(), d["xf"])
    rng = np.random.RandomState(TARGET_SEED)
    targets = [rng.standard_normal(tuple(o.shape)) for o in out]
    loss = sum(0.5 * ((o - torch.tensor(t)) ** 2).mean() for o, t in zip(out, targets))
    loss.backward()
    for k, o, t in zip(("pred_rotmat", "pred_shape", "pred_cam"), out, targets):
        d[f"train_{k}"] = o.detach().numpy()
        d[f"target_{k}"] = t
    d["loss"] = np.float64(loss.item())
    d["d_xf"] = caught["xf"].grad.reshape(BATCH, -1).numpy()
    after = model.state_dict()
    d["keys"] = np.asarray(head_keys)
    d["shapes"] = np.asarray([",".join(str(n) for n in after[k].shape) for k in head_keys])
    named = dict(model.named_parameters())
    d["param_keys"] = np.asarray(ref.HEAD_KEYS)
    d["grad_sum"] = np.asarray([named[k].grad.sum().item() for k in ref.HEAD_KEYS])
    d["grad_abs_sum"] = np.asarray([named[k].grad.abs().sum().item() for k in ref.HEAD_KEYS])
    d["grad_samples"] = np.concatenate([named[k].grad.reshape(-1)[ref.grad_sample_index(named[k].numel())].numpy() for k in ref.HEAD_KEYS])
    path = os.path.join(a.out, "hmr_head.npz")
    np.savez_compressed(path, **d)
    print(f"[hmr_head] {os.path.getsize(path)} bytes")


if __name__ == "__main__":
    main()
