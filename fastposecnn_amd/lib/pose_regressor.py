"""Drop-in for the model half of F/lib/pose_regressor.py (:443-777): the `Model` mixin
(class_compression, aggregate, hough_voting, perform_RT_calculation,
agg_hough_and_generate_RT, load_from_ckpt, construct_model, report_runtime), `PoseRegressor`
and `MODELS`.  The Lightning training task of the reference file (:70-438) is harness code
outside the hot path and is not provided; it keeps working against this model because the
constructor signature, `forward` output schema and state-dict names are the same.

forward(x[B,3,H,W]) -> {'logits': {...}, 'categorical': {...}, 'aggregated': AggData | None}
"""
import logging
import warnings
from typing import Optional, OrderedDict, Union

import numpy as np
import torch
import torch.nn as nn

from fastposecnn_amd.tools import timer as tm

import initialization as init
import gpu_tensor_funcs as gtf
import aggregation_layer as al
import hough_voting as hv
import backbone as bb

LOGGER = logging.getLogger('fastposecnn')

# same six stage names as the reference (pose_regressor.py:43-48)
FORWARD_TIMER = tm.TimerDecorator('forward')
MODEL_TIMER = tm.TimerDecorator('model')
AGG_TIMER = tm.TimerDecorator('Aggregation')
HV_TIMER = tm.TimerDecorator('Hough Voting')
RT_CAL_TIMER = tm.TimerDecorator('RT Calculation')
CLASS_COMPRESS_TIMER = tm.TimerDecorator('Class Compression')


class Model(object):

    @CLASS_COMPRESS_TIMER
    def class_compression(self, logits):
        # the engine's last kernel already produced the categorical data of ITS logits
        fused = getattr(self, '_fused', None)
        if fused is not None and fused[0] is logits:
            self._fused = None
            return fused[1]
        # arg-max of log-softmax + class compression + normalisation in one kernel
        return gtf.class_compression_fused(self.classes, logits)

    @AGG_TIMER
    def aggregate(self, data):
        return self.aggregation_layer.forward(data)

    @HV_TIMER
    def hough_voting(self, agg_data):
        return self.hough_voting_layer(agg_data)

    def _inv_k(self, dev):
        """Inverse intrinsics resident on `dev` (moved once, as forward() does at :749-751)."""
        if self.intrinsics.device != dev:
            self.intrinsics = self.intrinsics.to(dev)
            self.inv_intrinsics = torch.inverse(self.intrinsics)
        return self.inv_intrinsics

    @RT_CAL_TIMER
    def perform_RT_calculation(self, agg_data):
        return gtf.samplewise_get_RT(agg_data, self._inv_k(agg_data['quaternion'].device))

    def agg_hough_and_generate_RT(self, categorical_data) -> Union[None, dict]:
        if not self.HPARAM.PERFORM_AGGREGATION:
            return None
        if categorical_data['mask'].is_cuda and self.HPARAM.PERFORM_HOUGH_VOTING and not self.HPARAM.RUNTIME_TIMING:
            return self._post_network_deferred(categorical_data)
        agg_data = self.aggregate(categorical_data)
        if self.HPARAM.PERFORM_HOUGH_VOTING:
            agg_data = self.hough_voting(agg_data)
            if self.HPARAM.PERFORM_RT_CALCULATION:
                agg_data = self.perform_RT_calculation(agg_data)
        return agg_data

    def _post_network_deferred(self, categorical_data):
        """aggregate -> hough voting -> RT enqueued back to back on capacity-sized buffers, the instance
        count staying on the device (the reference synchronises >= 3 + rounds times PER INSTANCE,
        RV/ransac_voting_gpu.py:532-581); ONE host read at the end trims every tensor to [:n].
        Same dict as the stage-by-stage path."""
        return self.post_network_finish(self.post_network_enqueue(categorical_data))

    def post_network_enqueue(self, categorical_data, capacity=None, seed=None):
        """Enqueues aggregate -> hough voting -> RT on the CURRENT stream without any host read and
        returns a ticket for `post_network_finish`.  A caller that streams frames can enqueue the next
        frame's network before finishing this one (bench.py runs the two on separate HIP streams)."""
        B = categorical_data['mask'].shape[0]
        cap = int(capacity) if capacity else int(getattr(self.HPARAM, 'MAX_INSTANCES', 32)) * B
        if seed is None:
            seed = int(torch.randint(0, 2 ** 62, (1,)).item())      # one draw, also if the stages are re-run
        agg, n_dev = self.aggregation_layer.forward_deferred(categorical_data, cap)
        rt = self.HPARAM.PERFORM_RT_CALCULATION
        agg = self.hough_voting_layer(agg, n_dev=n_dev, seed=seed,
                                      inv_intrinsics=self._inv_k(agg['quaternion'].device) if rt else None)
        if rt and 'RT' not in agg:      # (an empty frame: the vote has nothing to append to)
            agg = gtf.samplewise_get_RT(agg, self._inv_k(agg['quaternion'].device))
        # asynchronous read-back of the instance count into pinned memory + an event to wait on
        pool = self.__dict__.setdefault('_pinned_counts', [])
        if len(pool) < 8:
            pool.append(torch.empty(1, dtype=torch.int32).pin_memory())
        slot = self.__dict__['_pinned_next'] = (self.__dict__.get('_pinned_next', -1) + 1) % len(pool)
        n_host = pool[slot]
        n_host.copy_(n_dev, non_blocking=True)
        event = torch.cuda.Event()
        event.record()
        return {'agg': agg, 'n_host': n_host, 'event': event, 'cat': categorical_data, 'cap': cap, 'seed': seed}

    def post_network_finish(self, ticket):
        """Waits for the ticket's work (only), trims every tensor to the n instances found."""
        ticket['event'].synchronize()
        n = int(ticket['n_host'][0])
        if n > ticket['cap']:       # more instances than the capacity: run again at the exact size
            return self.post_network_finish(self.post_network_enqueue(ticket['cat'], capacity=n, seed=ticket['seed']))
        agg = ticket['agg']
        if n == 0:
            agg['class_ids'] = agg['class_ids'].float()      # reference: float class ids when empty (:116)
        return {k: v[:n] for k, v in agg.items()}

    @classmethod
    def load_from_ckpt(self, ckpt_path, HPARAM):
        if ckpt_path is not None:
            checkpoint = torch.load(ckpt_path, map_location='cpu', weights_only=False)
            OLD_HPARAM = checkpoint['hyper_parameters']
            for attr in OLD_HPARAM.keys():
                if attr in ['MODEL', 'BACKBONE_ARCH', 'ENCODER', 'ENCODER_WEIGHTS', 'SELECTED_CLASSES']:
                    setattr(HPARAM, attr, OLD_HPARAM[attr])
            model = self.construct_model(HPARAM)
            # strip the 'model.' prefix PyTorch-Lightning adds (reference :528-531)
            striped_state_dict = OrderedDict([(k.replace('model.', ''), v)
                                              for (k, v) in checkpoint['state_dict'].items()])
            model.load_state_dict(striped_state_dict)
        else:
            model = self.construct_model(HPARAM)
        return model

    @classmethod
    def construct_model(self, HPARAM):
        model = self(
            HPARAM=HPARAM,
            architecture=HPARAM.BACKBONE_ARCH,
            encoder_name=HPARAM.ENCODER,
            encoder_weights=HPARAM.ENCODER_WEIGHTS,
            classes=len(HPARAM.SELECTED_CLASSES),
        )
        model.TIMERS = [MODEL_TIMER, AGG_TIMER, HV_TIMER, RT_CAL_TIMER, CLASS_COMPRESS_TIMER, FORWARD_TIMER]
        # the timers are module-level objects (as in the reference): set them from THIS model's flag so that a
        # model built with RUNTIME_TIMING=False is not timed because an earlier one asked for it
        for timer in model.TIMERS:
            timer.enabled = bool(HPARAM.RUNTIME_TIMING)
        return model

    def report_runtime(self):
        if self.HPARAM.RUNTIME_TIMING:
            for timer in self.TIMERS:
                print(f"{timer.name}: {timer.average:.3f} ms - {timer.fps} fps")
        else:
            print("Incapable of Runtime calculation: Set RUNTIME_TIMING = True next time.")


class PoseRegressor(Model, torch.nn.Module):

    def __init__(
        self,
        HPARAM,
        architecture: str = 'FPN',
        encoder_name: str = "resnet34",
        encoder_depth: int = 5,
        encoder_weights: Optional[str] = "imagenet",
        decoder_pyramid_channels: int = 256,
        decoder_segmentation_channels: int = 128,
        decoder_merge_policy: str = "add",
        decoder_dropout: float = 0.2,
        in_channels: int = 3,
        classes: int = 2,
        activation: Optional[str] = None,
        upsampling: int = 4,
    ):
        torch.nn.Module.__init__(self)
        self._engines = {}
        self._fused = None
        self._weights_gen = [0]         # shared (by reference) with copy.copy()'d instances: see note_unversioned_write
        self.HPARAM = HPARAM
        self.classes = classes  # includes background
        self.intrinsics = torch.from_numpy(np.asarray(HPARAM.NUMPY_INTRINSICS)).float()
        self.inv_intrinsics = torch.inverse(self.intrinsics)

        self.encoder = bb.get_encoder(encoder_name, in_channels=in_channels, depth=encoder_depth,
                                      weights=encoder_weights)
        if architecture != 'FPN':
            raise ValueError("only BACKBONE_ARCH='FPN' is built by the reference (pose_regressor.py:616)")
        param_dict = {
            'encoder_channels': self.encoder.out_channels,
            'encoder_depth': encoder_depth,
            'pyramid_channels': decoder_pyramid_channels,
            'segmentation_channels': decoder_segmentation_channels,
            'dropout': decoder_dropout,
            'merge_policy': decoder_merge_policy,
        }
        self.mask_decoder = bb.FPNDecoder(**param_dict)
        self.rotation_decoder = bb.FPNDecoder(**param_dict)
        self.translation_decoder = bb.FPNDecoder(**param_dict)
        self.scales_decoder = bb.FPNDecoder(**param_dict)

        head = dict(activation=activation, kernel_size=1, upsampling=upsampling)
        self.segmentation_head = bb.SegmentationHead(self.mask_decoder.out_channels, classes, **head)
        self.rotation_head = bb.SegmentationHead(self.rotation_decoder.out_channels, 4 * (classes - 1), **head)
        self.translation_head = bb.SegmentationHead(self.translation_decoder.out_channels, 3 * (classes - 1), **head)
        self.scales_head = bb.SegmentationHead(self.scales_decoder.out_channels, 3 * (classes - 1), **head)

        self.aggregation_layer = al.AggregationLayer(self.HPARAM, self.classes)
        self.hough_voting_layer = hv.HoughVotingLayer(self.HPARAM)

        for dec, hd in ((self.mask_decoder, self.segmentation_head), (self.rotation_decoder, self.rotation_head),
                        (self.translation_decoder, self.translation_head), (self.scales_decoder, self.scales_head)):
            init.initialize_decoder(dec)
            init.initialize_head(hd)

        if getattr(HPARAM, 'FREEZE_ENCODER', False):
            gtf.freeze(self.encoder)
        if getattr(HPARAM, 'FREEZE_MASK_TRAINING', False):
            gtf.freeze(self.mask_decoder); gtf.freeze(self.segmentation_head)
        if getattr(HPARAM, 'FREEZE_ROTATION_TRAINING', False):
            gtf.freeze(self.rotation_decoder); gtf.freeze(self.rotation_head)
        if getattr(HPARAM, 'FREEZE_TRANSLATION_TRAINING', False):
            gtf.freeze(self.translation_decoder); gtf.freeze(self.translation_head)
        if getattr(HPARAM, 'FREEZE_SCALES_TRAINING', False):
            gtf.freeze(self.scales_decoder); gtf.freeze(self.scales_head)

        # channel split of the translation head: per class (x, y, z) -> xy (2 ch) and z (1 ch)
        n_xyz = 3 * (classes - 1)
        self._xy_index = [i for i in range(n_xyz) if i % 3 != 2]
        self._z_index = [i for i in range(n_xyz) if i % 3 == 2]

    # ---- native engine (inference) -------------------------------------------------------
    def _engine_for(self, x):
        """The native plan for this input, or None when the torch modules must run: training /
        autograd (the engine has no backward), CPU tensors (config 1 plumbing), odd sizes.  The engine plans 2 to 32
        classes (background included), the bound of the class compression and the metrics; a model of more raises here."""
        if (self.training or torch.is_grad_enabled() or not x.is_cuda or x.dim() != 4 or x.shape[1] != 3
                or x.shape[2] % 32 or x.shape[3] % 32 or not getattr(self.HPARAM, 'USE_NATIVE_ENGINE', True)):
            return None
        key = (x.shape[0], x.shape[2], x.shape[3], x.device)
        eng = self._engines.get(key)
        if eng is None:
            from fastposecnn_amd.engine import NetEngine
            # ENGINE_AUTOTUNE=False keeps the static planner's tilings: results are then reproducible run to
            # run (tuned plans may differ in split-K, i.e. in f32 summation order)
            eng = NetEngine(self, key[0], key[1], key[2], x.device,
                            autotune=getattr(self.HPARAM, 'ENGINE_AUTOTUNE', True),
                            tune_mode=int(getattr(self.HPARAM, 'ENGINE_TUNE_MODE', 0)),
                            graph=bool(getattr(self.HPARAM, 'ENGINE_GRAPH', True)),
                            # 0: f32 matrix products only; 1: + the bf16 x 3 forms; 2: + the fp16 x 2 Winograd form (range-limited
                            # operands, csrc/wino_h2.hip) — HPARAM.ENGINE_SPLIT_PRECISION / ENGINE_SPLIT_F16
                            split_precision=(0 if not getattr(self.HPARAM, 'ENGINE_SPLIT_PRECISION', True)
                                             else (1 if not getattr(self.HPARAM, 'ENGINE_SPLIT_F16', True)
                                                   else (3 if getattr(self.HPARAM, 'ENGINE_SPLIT_F16_3P', True) else 2))))
            eng.generation = self._weights_gen[0]
            self._engines[key] = eng
        elif eng.stale() or eng.generation != self._weights_gen[0]:
            # a parameter changed since the plan packed it (load_state_dict on the model or a sub-module, an optimizer
            # or EMA step, p.copy_()): repack; the tuned tilings and the workspace stay.  Checked per forward, by every
            # FrameStreamer copy for its own plans; train()/eval() alone no longer costs a re-tune.
            eng.bind(self)
            eng.generation = self._weights_gen[0]
        return eng

    def _drop_engines(self):
        self._engines = {}
        self._fused = None

    def note_unversioned_write(self):
        """Something rewrote parameters or buffers without PyTorch's version counters seeing it (BatchNorm's running
        statistics in a training-mode forward, a kernel writing through raw pointers): every native plan bound to these
        tensors - this module's and its FrameStreamer copies', which share the counter - repacks at its next forward
        (bind() keeps the tuned tilings and the workspace: no re-tune).  The encoder's native BatchNorm (csrc/batchnorm.hip) is
        such a kernel: it writes running_mean / running_var through their data pointers, inside the training-mode forward that
        calls this first."""
        self._weights_gen[0] += 1

    def _apply(self, fn, *args, **kwargs):
        # .to() / .cuda() / .float(): the parameters become new tensors, possibly on another device
        self._drop_engines()
        return super()._apply(fn, *args, **kwargs)

    def _guarded_forward(self, eng, x):
        """HPARAM.ENGINE_RANGE_GUARD: the first real forward of a plan (the autotuning pass on zeros is none), and every
        ENGINE_RANGE_GUARD_EVERY-th after it, surveys the activations every convolution site reads; a site on an fp16-piece form
        whose input lies outside ENGINE_RANGE_LO .. ENGINE_RANGE_HI is demoted to its range-free plan, for good, and the frame runs
        again so that what is returned already comes from the guarded plans.  One warning per surveyed frame that demoted names
        the sites."""
        k = eng.guard_forwards
        eng.guard_forwards += 1
        every = int(getattr(self.HPARAM, 'ENGINE_RANGE_GUARD_EVERY', 0))
        if k != 0 and not (every > 0 and k % every == 0):
            return eng.forward(x)
        lo = float(getattr(self.HPARAM, 'ENGINE_RANGE_LO', 2.0 ** -2))
        hi = float(getattr(self.HPARAM, 'ENGINE_RANGE_HI', 2.0 ** 14))
        before, moved = eng.conv_plans(), []
        while True:
            # a site behind a saturating one was surveyed on ITS wrong output: after a demotion the frame is run again as a survey,
            # until a pass demotes nothing (every pass but the last demotes a site for good, so there are at most sites + 1)
            logits, cat, records = eng.survey(x)
            demoted = eng.guard_ranges(records, lo, hi)
            if not demoted:
                break
            mx = eng.record_max(records)
            for i in demoted:
                j = i
                # the folded s2.0 has a second operand, p3, surveyed into the record of the p2 lateral (reported 5000 while folded
                # away): name the record that is outside the bounds
                own_ok = not records[i, 1].item() and (mx[i].item() == 0 or lo <= mx[i].item() < hi)
                if own_ok and before[i][2] == -9:
                    j = next((k for k, p in enumerate(before) if p[2] == 5000), i)
                moved.append((i, mx[j].item(), int(records[j, 1].item()), " (its p3 operand)" if j != i else ""))
        if moved:
            after = eng.conv_plans()
            warnings.warn("fastposecnn_amd: activation-range guard (%g <= max|x| < %g) moved %d convolution site(s) of the %dx%dx%d "
                          "plan off the fp16-piece forms: %s" % (lo, hi, len(moved), eng.B, eng.H, eng.W, ", ".join(
                              "site %d max|x| %.4g%s%s plan %d -> %d" % (i, m, what, " (%d non-finite)" % bad if bad else "", before[i][2], after[i][2])
                              for i, m, bad, what in moved)), RuntimeWarning, stacklevel=3)
        return logits, cat

    @MODEL_TIMER
    def pure_model_forward(self, x: torch.Tensor):
        eng = self._engine_for(x)
        if eng is not None:
            if getattr(self.HPARAM, 'ENGINE_RANGE_GUARD', False):
                logits, cat = self._guarded_forward(eng, x)
            else:
                logits, cat = eng.forward(x)
            self._fused = (logits, cat)
            return logits
        if self.training:
            self.note_unversioned_write()   # BatchNorm moves its running statistics in place, unversioned
        features = self.encoder(x)
        mask_logits = self.segmentation_head(self.mask_decoder(*features))
        quat_logits = self.rotation_head(self.rotation_decoder(*features))
        xyz_logits = self.translation_head(self.translation_decoder(*features))
        scales_logits = self.scales_head(self.scales_decoder(*features))
        # reference :729-732 — channels 3k,3k+1 are xy of class k+1, channel 3k+2 is its z
        xy_logits = xyz_logits[:, self._xy_index, :, :]
        z_logits = xyz_logits[:, self._z_index, :, :]
        return {'mask': mask_logits, 'quaternion': quat_logits, 'scales': scales_logits,
                'xy': xy_logits, 'z': z_logits}

    @FORWARD_TIMER
    def forward(self, x: torch.Tensor):
        self._inv_k(x.device)
        logits = self.pure_model_forward(x)
        if x.is_cuda and torch.is_grad_enabled() and any(v.requires_grad for v in logits.values()):
            return self._forward_train(logits)
        categorical_data = self.class_compression(logits)
        agg_pred = self.agg_hough_and_generate_RT(categorical_data)
        return {'logits': logits, 'categorical': categorical_data, 'aggregated': agg_pred}

    def _forward_train(self, logits):
        """The post-network stages of a training step: the inference kernels forward, csrc/train.hip backward
        (lib/train_functions.py).  Same dict as the inference path; quaternion / scales / xy / z (+ R, T, RT) of
        'aggregated' and the four regression planes of 'categorical' carry autograd edges to the logits."""
        import train_functions as tf
        categorical_data = tf.class_compression_train(self.classes, logits)
        agg_pred = None
        if self.HPARAM.PERFORM_AGGREGATION:
            if not self.HPARAM.PERFORM_HOUGH_VOTING:
                raise NotImplementedError("training with PERFORM_AGGREGATION but without PERFORM_HOUGH_VOTING: no reference "
                                          "preset does (F/config.py:95-133)")
            agg_pred = tf.post_network_train(self, categorical_data)
        return {'logits': logits, 'categorical': categorical_data, 'aggregated': agg_pred}


MODELS = {
    'PoseRegressor': PoseRegressor
}
