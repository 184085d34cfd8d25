"""Host side of the training step (posegen_amd/trainer.py, posegen_amd/train_losses.py): what is decided before any kernel runs -- the
refusals, the learning-rate schedule, the temporal term's pose indices, the once-differentiable guard.  No GPU."""
from types import SimpleNamespace

import numpy as np
import pytest
import torch


def _args(**kw):
    base = dict(loss_fn="L1", loss_beta=0.1, reg_fn=None, reg_coef=0.1, use_background=True, coarse_weight=1.0, opt_pose=True, opt_pose_stop=None,
                opt_pose_step=1, opt_pose_tol=0.01, opt_pose_coef=2.0, opt_rot6d=True, opt_pose_cache=False, use_temp_loss=False, temp_coef=0.05,
                ext_scale=0.001, opt_framecode=False, chunk=4096, lrate=5e-4, lrate_decay=500, lrate_decay_rate=0.1, decay_unit=1000,
                finetune=False)
    base.update(kw)
    return SimpleNamespace(**base)


def _trainer(args, optimizer=None, popt_kwargs=None):
    from posegen_amd.trainer import HipTrainer
    return HipTrainer(args, {"hwf": (8, 8, 10.0)}, optimizer, None, {}, {}, popt_kwargs=popt_kwargs)


def test_the_new_modules_import_and_are_exported():
    import posegen_amd
    from posegen_amd import _ffi, train_losses, trainer
    assert posegen_amd.HipTrainer is trainer.HipTrainer
    for name in ("photometric_loss", "pose_regulariser", "grad_norms"):
        assert getattr(posegen_amd, name) is getattr(train_losses, name)
    for name in ("pg_train_loss", "pg_pose_reg_loss", "pg_grad_norms"):
        assert name in _ffi.PROTOTYPES
    assert train_losses.LOSS_KINDS == {"MSE": 0, "L1": 1, "Huber": 2}


@pytest.mark.parametrize("reg_fn", ["L1", "MSE"])
def test_reg_fn_l1_and_mse_are_refused_with_the_reason(reg_fn):
    """In the reference reduction='off' falls through to the unreduced tensor, total_loss has shape [n] and backward() raises"""
    from posegen_amd import train_losses
    with pytest.raises(ValueError, match=r"reduction='off'.*shape \[n\].*backward\(\) raises"):
        train_losses.check_loss_settings("L1", reg_fn)
    preds = {"rgb_map": torch.zeros(4, 3), "acc_map": torch.zeros(4)}
    batch = {"target_s": torch.zeros(4, 3), "fgs": torch.zeros(4, 1)}
    with pytest.raises(ValueError, match="refused"):
        train_losses.photometric_loss(preds, batch, loss_fn="MSE", reg_fn=reg_fn, renderer=None)
    with pytest.raises(ValueError, match="refused"):
        _trainer(_args(reg_fn=reg_fn))
    assert train_losses.check_loss_settings("Huber", "BCE", 0.0) == (2, 1)
    with pytest.raises(NotImplementedError):
        train_losses.check_loss_settings("L2", None)
    with pytest.raises(ValueError):
        train_losses.check_loss_settings("Huber", None, -1.0)


def test_opt_pose_cache_and_axis_angle_poses_are_refused():
    with pytest.raises(NotImplementedError, match="opt_pose_cache"):
        _trainer(_args(opt_pose_cache=True))
    with pytest.raises(NotImplementedError, match="opt_rot6d"):
        _trainer(_args(opt_rot6d=False), popt_kwargs={"popt_layer": object(), "popt_anchors": {}})
    _trainer(_args(opt_rot6d=False))                         # (no pose layer: nothing to regularise)


def test_a_bad_kp_idx_is_refused_before_anything_runs():
    from posegen_amd import train_losses
    assert train_losses.check_kp_idx(np.array([0, 4, 2]), 3, 5).dtype == np.int32
    for bad in ([0, 5, 2], [0, -1, 2]):
        with pytest.raises(IndexError, match=r"kp_idx\[1\]"):
            train_losses.check_kp_idx(np.array(bad), 3, 5)
    with pytest.raises(ValueError):
        train_losses.check_kp_idx(np.array([0, 1]), 3, 5)
    with pytest.raises(TypeError):
        train_losses.check_kp_idx(np.array([0.0, 1.0, 2.0]), 3, 5)
    rots, kps = torch.zeros(3, 24, 3, 3), torch.zeros(3, 24, 3)
    anchors = {"rots": torch.zeros(5, 24, 3, 3), "kps": torch.zeros(5, 24, 3)}
    with pytest.raises(IndexError):                          # (before the device check: the renderer is never asked)
        train_losses.pose_regulariser(rots, kps, np.array([0, 5, 2]), anchors, tol=0.01, coef=2.0, ext_scale=0.001, renderer=None)


def test_no_cpu_path():
    from posegen_amd import train_losses
    cpu = SimpleNamespace(device="cpu")
    preds = {"rgb_map": torch.zeros(4, 3), "acc_map": torch.zeros(4)}
    batch = {"target_s": torch.zeros(4, 3), "fgs": torch.zeros(4, 1)}
    with pytest.raises(NotImplementedError, match="no CPU path"):
        train_losses.photometric_loss(preds, batch, loss_fn="MSE", renderer=cpu)
    anchors = {"rots": torch.zeros(5, 24, 3, 3), "kps": torch.zeros(5, 24, 3)}
    with pytest.raises(NotImplementedError, match="no CPU path"):
        train_losses.pose_regulariser(torch.zeros(3, 24, 3, 3), torch.zeros(3, 24, 3), np.array([0, 1, 2]), anchors, tol=0.01, coef=2.0,
                                      ext_scale=0.001, renderer=cpu)
    p = torch.nn.Parameter(torch.zeros(3))
    p.grad = torch.ones(3)
    with pytest.raises(NotImplementedError, match="no CPU path"):
        train_losses.grad_norms([p], cpu)
    with pytest.raises(ValueError, match="divides by zero"):
        train_losses.grad_norms([torch.nn.Parameter(torch.zeros(3))], cpu)
    gpu = SimpleNamespace(device="cuda:0")                   # inputs on another device than the renderer's
    with pytest.raises(NotImplementedError, match="is on cpu"):
        train_losses.photometric_loss(preds, batch, loss_fn="MSE", renderer=gpu)


def test_learning_rate_schedule_follows_the_reference_formula():
    """decay_optimizer_lrate (core/trainer.py:175-185): lrate * decay_rate ** ((step // decay_unit) / lrate_decay) with the optimiser's
    own step count; the trainer's host-side count starts from the optimiser's state and follows its steps"""
    from posegen_amd.trainer import decayed_lrate
    p = torch.nn.Parameter(torch.zeros(2))
    opt = torch.optim.Adam([p], lr=5e-4)
    args = _args(lrate=5e-4, lrate_decay=3, lrate_decay_rate=0.1, decay_unit=2)
    for _ in range(3):                                       # a resumed optimiser: three steps before the trainer exists
        p.grad = torch.ones(2)
        opt.step()
    tr = _trainer(args, optimizer=opt)
    assert tr.optim_steps == 3
    for _ in range(6):
        p.grad = torch.ones(2)
        opt.step()
        tr.optim_steps += 1
        step = int(opt.state[opt.param_groups[0]["params"][0]]["step"])
        want = args.lrate * (args.lrate_decay_rate ** ((step // args.decay_unit) / args.lrate_decay))
        assert tr.optim_steps == step
        assert tr.decay_optimizer_lrate() == want and opt.param_groups[0]["lr"] == want
    assert decayed_lrate(5e-4, 500, 0.1, 0) == 5e-4 and decayed_lrate(5e-4, 500, 0.1, 999) == 5e-4
    assert decayed_lrate(5e-4, 500, 0.1, 500000) == 5e-4 * 0.1 ** 1.0
    assert _trainer(args, optimizer=torch.optim.Adam([torch.nn.Parameter(torch.zeros(1))])).optim_steps == 0


def test_temporal_indices_wrap_as_numpy_indexing_does():
    from posegen_amd.trainer import temporal_indices
    table = np.arange(7) * 10
    idx = np.array([0, 6, 3, 0, 1])
    prev, nxt = temporal_indices(idx, 7)
    assert prev.tolist() == [6, 5, 2, 6, 0] and nxt.tolist() == [1, 0, 4, 1, 2]
    assert (table[prev] == table[idx - 1]).all()             # -1 -> the last pose, what the reference's popt_layer(kp_idx - 1) reads
    assert (table[nxt] == table[(idx + 1) % 7]).all()
    assert prev.min() >= 0


def test_the_loss_functions_are_differentiable_once():
    """backward scales the stored gradients by the upstream gradient; differentiating that again raises"""
    from posegen_amd import train_losses
    for fn, n_in in ((train_losses._PhotometricFn, 10), (train_losses._PoseRegFn, 8)):
        assert hasattr(fn.backward, "__wrapped__")
        stored = torch.arange(6, dtype=torch.float32).reshape(2, 3)
        ctx = SimpleNamespace(grads=[stored, None] + ([None, None] if n_in == 10 else []),
                              meta=[((2, 3), torch.float32), None] + ([None, None] if n_in == 10 else []))
        g = torch.tensor(2.0, dtype=torch.float64, requires_grad=True)
        out = fn.backward(ctx, g)
        assert len(out) == n_in and out[0] is None and out[2] is None
        assert torch.equal(out[1].detach(), stored * 2)
        with pytest.raises(RuntimeError, match="once_differentiable"):
            out[1].sum().backward()


def test_train_batch_index_bookkeeping_without_a_pose_layer():
    """get_kp_args / get_fwd_args read the batch's own poses when there is no pose layer (trainer.py:293-295)"""
    tr = _trainer(_args(opt_framecode=True))
    batch = {"kp3d": 1, "skts": 2, "bones": 3, "cyls": 4, "rays": 5, "cam_idxs": 6}
    kp_args, extras = tr.get_kp_args(batch)
    assert kp_args == {"kp_batch": 1, "skts": 2, "bones": 3, "cyls": 4} and extras == {}
    assert tr.get_fwd_args(batch) == {"rays": 5, "cams": 6, "subject_idxs": None}
