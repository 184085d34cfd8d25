#!/usr/bin/env python3
"""tests/golden/smpl_body.npz from the REAL reference's `lbs` and `vertices2joints` (smplx/smplx/lbs.py:152-268), in float32 on
the host, on the seeded synthetic body of posegen_amd.synthetic.make_body_model (no licensed model file is needed or read).

Runs only where the reference checkout exists: its vendored `smplx` package goes on sys.path and `smplx.lbs` is imported.  Stored: the model's seed and sizes, not its arrays; the inputs --
6 poses at V = 431, NB = 10 in axis-angle and as the rotation matrices `batch_rodrigues` makes of them, pose 0 all zero, pose 1
with angles near pi, betas up to +-3 --; the reference's float32 `verts` and `J_transformed` of both pose forms and
`vertices2joints` of the 17-row and the 9-row regressor.

Usage:  python tools/gen_golden_smpl.py [--ref /root/reference] [--out tests/golden]
"""
from __future__ import annotations

import argparse
import os
import sys

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.dont_write_bytecode = True

V, NB, SEED, B = 431, 10, 3, 6
REGRESS_ROWS = (17, 9)


def make_inputs():
    """(betas [B,NB], pose [B,24,3]) float32: pose 0 at rest, pose 1 with every angle within 0.02 of pi, the others with angles
    up to 1.5 about random axes; betas uniform in [-3, 3]"""
    rng = np.random.RandomState(SEED + 1)
    betas = rng.uniform(-3.0, 3.0, size=(B, NB)).astype(np.float32)
    axes = rng.randn(B, 24, 3)
    axes /= np.linalg.norm(axes, axis=-1, keepdims=True)
    angles = rng.uniform(0.2, 1.5, size=(B, 24, 1))
    angles[1] = np.pi - rng.uniform(0.0, 0.02, size=(24, 1))
    pose = axes * angles
    pose[0] = 0.0
    return betas, pose.astype(np.float32)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--ref", default="/root/reference")
    ap.add_argument("--out", default=os.path.join(REPO, "tests", "golden"))
    args = ap.parse_args()
    path = os.path.join(args.ref, "smplx", "smplx", "lbs.py")
    if not os.path.exists(path):
        sys.exit(f"gen_golden_smpl: {path} not found -- the fixture is made from the reference's own lbs; pass --ref")
    import torch
    sys.path.insert(0, os.path.join(args.ref, "smplx"))
    from smplx import lbs as ref_lbs

    from posegen_amd.synthetic import make_body_model
    model = make_body_model(V, NB=NB, seed=SEED, regress_rows=REGRESS_ROWS)
    betas, pose = make_inputs()
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a))
    parents = t(model["parents"].astype(np.int64))
    common = (t(model["v_template"]), t(model["shapedirs"]), t(model["posedirs"]), t(model["J_regressor"]), parents, t(model["lbs_weights"]))
    with torch.no_grad():
        rotmat = ref_lbs.batch_rodrigues(t(pose).view(-1, 3)).view(B, 24, 3, 3)
        verts, joints = ref_lbs.lbs(t(betas), t(pose).view(B, 72), *common, pose2rot=True)
        verts_rm, joints_rm = ref_lbs.lbs(t(betas), rotmat, *common, pose2rot=False)
        out = dict(seed=np.int64(SEED), V=np.int64(V), NB=np.int64(NB), regress_rows=np.asarray(REGRESS_ROWS, dtype=np.int64),
                   betas=betas, pose=pose, rotmat=rotmat.numpy(), verts=verts.numpy(), joints=joints.numpy(),
                   verts_rotmat=verts_rm.numpy(), joints_rotmat=joints_rm.numpy())
        for K in REGRESS_ROWS:
            out[f"regressed_{K}"] = ref_lbs.vertices2joints(t(model[f"regressor_{K}"]), verts).numpy()
            out[f"regressed_{K}_rotmat"] = ref_lbs.vertices2joints(t(model[f"regressor_{K}"]), verts_rm).numpy()
    dst = os.path.join(args.out, "smpl_body.npz")
    np.savez_compressed(dst, **out)
    print(f"wrote {dst}: {os.path.getsize(dst)} bytes")


if __name__ == "__main__":
    main()
