"""posegen_amd -- MI355X-native A-NeRF renderer for the PoseGen loop.

Drop-in for the reference's volumetric rendering hot path
(`render_path` -> `render` -> `RayCaster.render_rays`): Python host code on
PyTorch-ROCm calls hand-written HIP kernels for gfx950 through a C-ABI shared
library (`include/posegen_hip.h`).  There is no CPU fallback: every compute
entry point raises if the HIP library is missing.
"""
from .config import (RenderConfig, surreal_config, surreal_single_config, h36m_config, PREC_FP32, PREC_BF16,
                     PREC_BF16X3, PREC_FP16, PREC_FP16X3, PREC_FP16C, PREC_FP16M, PREC_NAMES, PREC_BY_NAME)

__all__ = ["RenderConfig", "surreal_config", "surreal_single_config", "h36m_config", "PREC_FP32", "PREC_BF16",
           "PREC_BF16X3", "PREC_FP16", "PREC_FP16X3", "PREC_FP16C", "PREC_FP16M", "PREC_NAMES", "PREC_BY_NAME"]
__version__ = "0.1.0"

_TRAIN_NAMES = ("make_trainable", "TrainableRayCaster", "SingleNetTrainableRayCaster")
_POSEOPT_NAMES = ("HipPoseOptLayer",)
_BATCH_NAMES = ("DeviceImageBank", "ImageBatchSampler", "RayBatchSource")
_EVALUATE_NAMES = ("FrameScorer", "evaluate_frames", "evaluate_metric", "ValidationScorer", "evaluate_validation", "evaluate_testset",
                   "validation_scores")
_POSE_EVAL_NAMES = ("PoseScorer", "pa_mpjpe", "n_mpjpe", "reconstruction_error", "refinement_scores", "evaluate_smpl_predictions",
                    "pampjpe_from_smpl_params")
_SMPL_NAMES = ("BodyModel", "vertex_errors")
_POSE_LOSS_NAMES = ("keypoints_from_axis_angle", "keypoints_from_rotmats", "pose_loss")
_TRAIN_LOSS_NAMES = ("photometric_loss", "pose_regulariser", "grad_norms")
_TRAINER_NAMES = ("HipTrainer",)
_REGRESSOR_BATCH_NAMES = ("PixelStore", "RegressorBatchSource", "regressor_input", "fixed_crop_boxes", "mpii_crop_boxes", "REFERENCE_NORM")
_SCENE_NAMES = ("ScenePerson", "render_scene", "render_scenes", "place_people")
_GENERATOR_NAMES = ("HipBAGenerator", "HipRTGenerator", "HipPoseGenerator")
_REGRESSOR_NAMES = ("HipHMRHead", "HipHMR")
_OPTIM_NAMES = ("HipAdam",)


def __getattr__(name):
    # the training wrappers live in posegen_amd.train (imports torch): resolved on first use
    if name in _TRAIN_NAMES:
        from . import train
        return getattr(train, name)
    if name in _POSEOPT_NAMES:                 # the pose layer of pose refinement (imports torch as well)
        from . import poseopt
        return getattr(poseopt, name)
    if name in _BATCH_NAMES:                   # training batches on the device (imports torch as well)
        from . import batches
        return getattr(batches, name)
    if name in _EVALUATE_NAMES:                # frame scores on the device (imports torch as well)
        from . import evaluate
        return getattr(evaluate, name)
    if name in _POSE_EVAL_NAMES:               # pose scores on the device (imports torch as well)
        from . import pose_eval
        return getattr(pose_eval, name)
    if name in _SMPL_NAMES:                    # the SMPL body on the device (imports torch as well)
        from . import smpl
        return getattr(smpl, name)
    if name in _POSE_LOSS_NAMES:               # differentiable key points and pose losses (imports torch as well)
        from . import pose_losses
        return getattr(pose_losses, name)
    if name in _TRAIN_LOSS_NAMES:              # the trainer's losses, pose regulariser and gradient norms (imports torch as well)
        from . import train_losses
        return getattr(train_losses, name)
    if name in _TRAINER_NAMES:                 # the training step: the reference's Trainer (imports torch as well)
        from . import trainer
        return getattr(trainer, name)
    if name in _REGRESSOR_BATCH_NAMES:         # the regressor's input batches on the device (imports torch as well)
        from . import regressor_batches
        return getattr(regressor_batches, name)
    if name in _SCENE_NAMES:                  # several people in one frame (imports torch as well)
        from . import scene
        return getattr(scene, name)
    if name in _GENERATOR_NAMES:              # the pose generator of the GAN loop (imports torch as well)
        from . import generators
        return getattr(generators, name)
    if name in _REGRESSOR_NAMES:              # the regressor's head (imports torch as well)
        from . import regressors
        return getattr(regressors, name)
    if name in _OPTIM_NAMES:                  # the optimiser step on the device (imports torch as well)
        from . import optim
        return getattr(optim, name)
    raise AttributeError(f"module {__name__!r} has no attribute {name!r}")
