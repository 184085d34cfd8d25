"""The float64 oracle gradient (tests/helpers.py: oracle_grads) pinned to the reference's own autograd on the training
fixtures, without a GPU: the yardstick of tests/test_gpu_train_shapes.py is checked before any kernel is measured by it."""
import numpy as np
import pytest
import torch

from tests.helpers import cfg_from_golden, golden_draws, load_golden, model_for, oracle_grads
from tools.gen_golden import grad_sample_index


@pytest.mark.parametrize("name", ["train_grads", "train_grads_h36m"])
def test_float64_oracle_gradients_match_the_reference_autograd(name):
    """render_rays + loss + backward() of the oracle in float64 (every input, weight, draw and constant) against the
    fixture's reference gradients, with the bounds the fp32 HIP step meets (test_gpu_train.py): every sampled entry within
    1e-4 of its tensor's scale, every norm within 1e-4 relative, the loss within 1e-5, the maps within 2e-5."""
    g = load_golden(name)
    cfg = cfg_from_golden(g)
    wc, wf, tv, td = model_for(cfg, int(g["seed_model"]))
    prev = torch.get_default_dtype()
    loss, maps, grads = oracle_grads(cfg, wc, wf, float(g["tau_v"]), float(g["tau_d"]), g["ray_batch"], g["skts"], g["cyl"],
                                     g["target"], cfg.n_samples, cfg.n_importance, cams=g.get("cams"), draws=golden_draws(g))
    assert torch.get_default_dtype() == prev, "the default dtype is restored"
    assert abs(loss - float(g["loss"])) <= 1e-5 * max(1.0, abs(float(g["loss"])))
    for k in ("rgb_map", "acc_map", "rgb0", "acc0"):
        assert float(np.abs(maps[k] - g[k]).max()) <= 2e-5, k
    n_checked, worst = 0, 0.0
    for (tag, k), gr in grads.items():
        ref_vals, ref_norm = g[f"gval_{tag}_{k}"], float(g[f"gnorm_{tag}_{k}"])
        got = gr.reshape(-1)
        scale = max(float(np.abs(ref_vals).max()), ref_norm / np.sqrt(got.size), 1e-12)
        err = float(np.abs(got[grad_sample_index(got.size)] - ref_vals).max())
        nerr = abs(float(np.linalg.norm(got)) - ref_norm)
        worst = max(worst, err / scale, nerr / max(ref_norm, 1e-12))
        assert err <= 1e-4 * scale + 1e-9, (tag, k, err, scale)
        assert nerr <= 1e-4 * ref_norm + 1e-9, (tag, k, nerr, ref_norm)
        n_checked += 1
    assert n_checked == (50 if cfg.framecode_ch else 48)
    print(f"[{name}] float64 oracle vs the reference's autograd: worst relative gradient deviation {worst:.2e}")


def test_float64_oracle_is_the_fp32_oracle_in_fp32():
    """dtype=float32 is the oracle the existing tests run (same loss and gradients bitwise): the helper changes the
    precision, nothing else."""
    from oracle import anerf_oracle as orc
    from tests.helpers import loss_of, oracle_cfg
    g = load_golden("train_grads")
    cfg = cfg_from_golden(g)
    wc, wf, tv, td = model_for(cfg, int(g["seed_model"]))
    loss, _, grads = oracle_grads(cfg, wc, wf, float(g["tau_v"]), float(g["tau_d"]), g["ray_batch"], g["skts"], g["cyl"],
                                  g["target"], cfg.n_samples, cfg.n_importance, draws=golden_draws(g), dtype=torch.float32)
    tw = lambda w: {k: torch.tensor(v, requires_grad=True) for k, v in w.items()}
    twc, twf = tw(wc), tw(wf)
    ref = orc.render_rays(torch.tensor(g["ray_batch"]), torch.tensor(g["skts"]), torch.tensor(g["cyl"]), oracle_cfg(cfg, tv, td),
                          twc, twf, cfg.n_samples, cfg.n_importance, draws=golden_draws(g))
    ref_loss = loss_of(ref, torch.tensor(g["target"]))
    ref_loss.backward()
    assert loss == float(ref_loss.detach())
    for tag, w in (("coarse", twc), ("fine", twf)):
        for k, p in w.items():
            assert np.array_equal(grads[(tag, k)], p.grad.double().numpy()), (tag, k)
