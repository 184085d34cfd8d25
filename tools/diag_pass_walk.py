"""How evenly the pass walk spreads a frame's work over the persistent workgroups (the numbers of
profiles/pass_walk_imbalance.txt).  Needs a library whose pg_eval16r.hip is built with -DPG_WALK_STAMPS:

    FILE=pg_eval16r.hip tools/build_variant.sh walk_stamps -DPG_WALK_STAMPS
    POSEGEN_HIP_LIB=build_ab/lib_walk_stamps.so [POSEGEN_PASS_WALK=0] python tools/diag_pass_walk.py [bf16|fp16] [RES]

In that build the limb-mask counter instantiation of the on-chip kernel (pg_stage_eval, dbg_stage 97) also records, per workgroup,
its clock at entry and exit (s_memtime; the XCDs' clocks have different origins, so only the difference of a workgroup's own
two stamps means something), its passes and its limbs in range summed over them.  Runs the coarse (64 samples) and the
fine (64 + 16) launch of the benchmark frame and prints min / median / mean / max over the workgroups."""
import os, sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np, torch
from posegen_amd import surreal_config, synthetic as syn
from posegen_amd.raycaster import HipRayCaster
from bench import full_frame_rays

prec = sys.argv[1] if len(sys.argv) > 1 else "bf16"
res = int(sys.argv[2]) if len(sys.argv) > 2 else 512
dev = torch.device("cuda:0")
cfg = surreal_config()
c = HipRayCaster.from_weights(cfg, *syn.make_model(cfg, 0), device=dev, precision=prec)
rb, skts, cyl, *_ = full_frame_rays(res, res, dev)
r = c.renderer
nf, z = r.stage_sample_coarse(rb, cyl, cfg.n_samples)
raw = r.stage_eval(0, rb, z, skts)
z_fine = r.stage_composite(rb, z, raw, n_importance=cfg.n_importance)["z_fine"]
MAXWG = 1024


def stamps(which, zz):
    S = zz.shape[1]
    for _ in range(2):          # (the second launch: clocks settled, weights in L2)
        dbg = torch.zeros(16 + 8 * MAXWG, device=dev, dtype=torch.int32)
        r.stage_eval(which, rb, zz, skts, dbg_stage=97, dbg=dbg)
        torch.cuda.synchronize()
    d = dbg.cpu().numpy().view(np.uint32)
    rec = d[16:].reshape(MAXWG, 8)
    rec = rec[rec[:, 4] > 0]
    if not len(rec):
        sys.exit("no per-workgroup records: is POSEGEN_HIP_LIB a -DPG_WALK_STAMPS build?")
    t0 = rec[:, 0].astype(np.uint64) | (rec[:, 1].astype(np.uint64) << np.uint64(32))
    t1 = rec[:, 2].astype(np.uint64) | (rec[:, 3].astype(np.uint64) << np.uint64(32))
    busy = (t1 - t0).astype(np.float64)
    limbs = rec[:, 5] / rec[:, 4]
    line = lambda name, v, f: print(f"  {name:34s} min {v.min():{f}}  median {np.median(v):{f}}  mean {v.mean():{f}}  max {v.max():{f}}"
                                    f"  (max - mean) / mean {100 * (v.max() - v.mean()) / v.mean():.2f} %")
    print(f"{['coarse', 'fine'][which]} launch, S = {S}: {int(d[0])} passes on {len(rec)} workgroups, {int(rec[:, 4].min())}..{int(rec[:, 4].max())} each")
    line("busy ticks per workgroup (s_memtime)", busy, ".0f")
    line("limbs in range per pass", limbs, ".3f")


print(f"{prec} {res} x {res}, POSEGEN_PASS_WALK={os.environ.get('POSEGEN_PASS_WALK', 'default')}")
stamps(0, z)
stamps(1, z_fine)
