"""HPARAM presets restricted to the fields the hot path reads ("Config / flags").
Mirrors the attribute names and values of F/config.py:11-160 (DEFAULT_POSE_HPARAM, MASK_TRAINING,
HEAD_TRAINING, EVALUATING, INFERENCE) and the CAMERA constants of F/tools/project.py:78-88 so the
benchmarks and tests can build a model without the reference's `tools` package."""
import argparse

import numpy as np

CAMERA_INTRINSICS = np.array([[577.5, 0, 319.5], [0., 577.5, 239.5], [0., 0., 1.]])
CAMERA_CLASSES = ['bg', 'bottle', 'bowl', 'camera', 'can', 'laptop', 'mug']


class DEFAULT_POSE_HPARAM(argparse.Namespace):
    RUNTIME_TIMING = False
    MODEL = 'PoseRegressor'
    DATASET_NAME = 'CAMERA'
    SELECTED_CLASSES = CAMERA_CLASSES
    NUMPY_INTRINSICS = CAMERA_INTRINSICS
    BATCH_SIZE = 3

    FREEZE_ENCODER = False
    FREEZE_MASK_TRAINING = False
    FREEZE_ROTATION_TRAINING = False
    FREEZE_TRANSLATION_TRAINING = False
    FREEZE_SCALES_TRAINING = False

    PERFORM_AGGREGATION = True
    PERFORM_HOUGH_VOTING = True
    PERFORM_RT_CALCULATION = True
    PERFORM_MATCHING = True

    BACKBONE_ARCH = 'FPN'
    ENCODER = 'resnet18'
    ENCODER_WEIGHTS = 'imagenet'

    HV_NUM_OF_HYPOTHESES = 128

    # Not in the reference: which matrix products the native backbone engine's plans may use.
    # The fp16-piece forms take activations as they come: full accuracy while the values a 3x3 site reads lie in about
    # 2^-2 .. 2^14 (3 * 2^-23 relative; 2^-24 ABSOLUTE below, saturation from 1.3e5); the bf16 x 3 and f32 forms have no such range.
    ENGINE_SPLIT_PRECISION = True     # False: f32 matrix products only
    ENGINE_SPLIT_F16 = True           # False: split-precision sites on three bf16 pieces only (no operand range)
    ENGINE_SPLIT_F16_3P = True        # False: the fp16-piece forms keep all four piece products
    # The guard of that range ("The activation-range guard"): off by default.  On: the first real forward of a plan
    # surveys what every convolution site reads and moves the fp16-piece sites whose input lies outside LO .. HI (on max |x|; or is
    # not finite) to their range-free plans, for good, with one warning; the frame is then run again on the guarded plans.
    ENGINE_RANGE_GUARD = False
    ENGINE_RANGE_GUARD_EVERY = 0      # N > 0: every N-th forward of a plan surveys again (demotions are never undone)
    ENGINE_RANGE_LO = 2.0 ** -2       # a site whose input has 0 < max |x| < LO is demoted (conservative: the bound is on the maximum)
    ENGINE_RANGE_HI = 2.0 ** 14       # ... or max |x| >= HI (x 4 by the Winograd input transform stays below 2^16)


class MASK_TRAINING(DEFAULT_POSE_HPARAM):
    FREEZE_ROTATION_TRAINING = True
    FREEZE_TRANSLATION_TRAINING = True
    FREEZE_SCALES_TRAINING = True
    PERFORM_AGGREGATION = False
    PERFORM_HOUGH_VOTING = False
    PERFORM_RT_CALCULATION = False
    PERFORM_MATCHING = False


class HEAD_TRAINING(DEFAULT_POSE_HPARAM):
    pass


class EVALUATING(DEFAULT_POSE_HPARAM):
    HV_NUM_OF_HYPOTHESES = 1000


class INFERENCE(DEFAULT_POSE_HPARAM):
    HV_NUM_OF_HYPOTHESES = 1000
    BATCH_SIZE = 1
    RUNTIME_TIMING = True
