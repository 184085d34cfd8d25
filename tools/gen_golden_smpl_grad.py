#!/usr/bin/env python3
"""tests/golden/smpl_body_grad.npz from the REAL reference's `lbs` and `vertices2joints` (smplx/smplx/lbs.py:152-268) under torch
autograd, on the host, on the model seed and the inputs of tests/golden/smpl_body.npz (tools/gen_golden_smpl.py).

Runs only where the reference checkout exists: its vendored `smplx` package goes on sys.path and `smplx.lbs` is imported.  Stored:
seeded float32 cotangents for the vertices, the posed joints and both regressors' joints (17 and 9 rows), and, for each cotangent
alone (`verts`, `joints`, `reg17`, `reg9`) and for vertices + joints + one regressor together (`all17`, `all9`), the reference's
`d_betas` [B,NB] and `d_pose` in axis-angle ([B,24,3]) and in rotation-matrix form ([B,24,3,3], the nine entries free), once with
the reference run in float32 (`_f32`) and once in float64 on the same float32 numbers (`_f64`).  Arrays only.

The cotangent scales (SCALE) put the three cotangents' contributions to a gradient entry at the same order of magnitude, so that
leaving out any one term of the backward moves the gradients far outside the bounds (tests/test_smpl_grad_ref.py prints by how much).

Usage:  python tools/gen_golden_smpl_grad.py --ref REFERENCE_CHECKOUT [--out tests/golden]
"""
from __future__ import annotations

import argparse
import os
import sys

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.dont_write_bytecode = True

from tools.gen_golden_smpl import B, NB, REGRESS_ROWS, SEED, V, make_inputs  # noqa: E402

SCALE = {"verts": 1.0 / 16.0, "joints": 1.0, "reg": 1.0}
CASES = {"verts": ("verts",), "joints": ("joints",), "reg17": ("reg17",), "reg9": ("reg9",), "all17": ("verts", "joints", "reg17"),
         "all9": ("verts", "joints", "reg9")}


def make_cotangents():
    rng = np.random.RandomState(SEED + 2)
    cot = {"verts": rng.randn(B, V, 3) * SCALE["verts"], "joints": rng.randn(B, 24, 3) * SCALE["joints"]}
    for K in REGRESS_ROWS:
        cot[f"reg{K}"] = rng.randn(B, K, 3) * SCALE["reg"]
    return {k: v.astype(np.float32) for k, v in cot.items()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--ref", required=True, help="the reference checkout (its smplx/ is imported)")
    ap.add_argument("--out", default=os.path.join(REPO, "tests", "golden"))
    args = ap.parse_args()
    path = os.path.join(args.ref, "smplx", "smplx", "lbs.py")
    if not os.path.exists(path):
        sys.exit(f"gen_golden_smpl_grad: {path} not found -- the fixture is made from the reference's own lbs; pass --ref")
    import torch
    sys.path.insert(0, os.path.join(args.ref, "smplx"))
    from smplx import lbs as ref_lbs

    from posegen_amd.synthetic import make_body_model
    model = make_body_model(V, NB=NB, seed=SEED, regress_rows=REGRESS_ROWS)
    betas, pose = make_inputs()
    with torch.no_grad():
        rotmat = ref_lbs.batch_rodrigues(torch.from_numpy(pose).view(-1, 3)).view(B, 24, 3, 3).numpy()
    cot = make_cotangents()
    out = dict(seed=np.int64(SEED), V=np.int64(V), NB=np.int64(NB), regress_rows=np.asarray(REGRESS_ROWS, dtype=np.int64))
    out.update({f"cot_{k}": v for k, v in cot.items()})
    for prec, dt in (("f32", torch.float32), ("f64", torch.float64)):
        t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dt)
        parents = torch.from_numpy(model["parents"].astype(np.int64))
        common = (t(model["v_template"]), t(model["shapedirs"]), t(model["posedirs"]), t(model["J_regressor"]), parents, t(model["lbs_weights"]))
        for form in ("axis", "rotmat"):
            for case, parts in CASES.items():
                b = t(betas).requires_grad_(True)
                p = (t(pose).view(B, 72) if form == "axis" else t(rotmat)).requires_grad_(True)
                verts, joints = ref_lbs.lbs(b, p, *common, pose2rot=form == "axis")
                outs = {"verts": verts, "joints": joints}
                for K in REGRESS_ROWS:
                    outs[f"reg{K}"] = ref_lbs.vertices2joints(t(model[f"regressor_{K}"]), verts)
                loss = sum((outs[k] * t(cot[k])).sum() for k in parts)
                gb, gp = torch.autograd.grad(loss, (b, p))
                out[f"d_betas_{case}_{form}_{prec}"] = gb.numpy()
                out[f"d_pose_{case}_{form}_{prec}"] = gp.numpy().reshape((B, 24, 3) if form == "axis" else (B, 24, 3, 3))
    dst = os.path.join(args.out, "smpl_body_grad.npz")
    np.savez_compressed(dst, **out)
    print(f"wrote {dst}: {os.path.getsize(dst)} bytes")


if __name__ == "__main__":
    main()
