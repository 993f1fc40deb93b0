"""Drop-in for `fcn8s_tensorflow.FCN8s` (reference: fcn8s_tensorflow.py:17-952).

Same constructor, `train / evaluate / predict / predict_and_save / save /
load_variables / close` signatures, keyword names, defaults, validation
messages and bookkeeping attributes.  The TensorFlow session behind them is
replaced by `engine.Engine` (ctypes -> libfcn8s_hip.so, hand-written gfx950
kernels).  Host-side control flow below restates the reference's loops; the
three `sess.run` sites (:554-572, :685-689, :764-770) become
`Engine.train_step / eval_step / predict`.

Differences a maintainer must know (also listed in INTEGRATION.md):
  * Variables stored by TensorFlow (the VGG-16 SavedModel for `vgg16_dir`,
    FCN-8s SavedModels / Saver checkpoints for `model_load_dir`,
    `variables_load_dir`, `load_variables`) are READ through `tf_bundle.py`
    (tensor-bundle format, no TensorFlow needed; graph files are ignored).
    `save()` keeps the reference's directory naming scheme (:904-920) but
    stores `variables.npz` + `fcn8s_meta.json`; `export_tf_variables()` writes
    a TF-restorable bundle.  `vgg16_dir` may also hold `vgg16_weights.npz` or
    be the string 'synthetic[:seed]'.
  * Labels may also be passed as uint8 class-id maps (N,H,W); one-hot
    (N,H,W,C) input as in the reference is reduced to ids on the GPU.
  * Data-parallel training: launch one process per GPU with torch.distributed
    initialised (RCCL); every rank feeds its own shard of the minibatch.
"""
from __future__ import annotations

import contextlib
import json
import os
import shutil
import sys
import time
import warnings
from collections import deque
from glob import glob

import numpy as np

try:
    from tqdm import trange
except Exception:  # pragma: no cover
    def trange(n, **kw):
        class _R:
            def __init__(self, n): self.n = n
            def __iter__(self): return iter(range(self.n))
            def set_description(self, *a, **k): pass
            def set_postfix(self, *a, **k): pass
        return _R(n)

from . import _lib as L
from . import crf as crf_mod
from . import temperature as ts_mod
from . import pseudo_label as pl_mod
from . import class_mix as cm_mod
from . import strong_augment as sa_mod
from . import fda as fda_mod
from . import regions as regions_mod
from . import sweeps
from . import loss as loss_mod
from . import optim as optim_mod
from . import tf_bundle
from .engine import Engine, padded_classes

_SAVERS = {'saved_model', 'train_saver'}


def _check_metric_names(metrics):
    for metric in metrics:
        if metric not in ('loss', 'mean_iou', 'accuracy'):
            raise ValueError("{} is not a valid metric. Valid metrics are ['loss', mean_iou', 'accuracy']".format(metric))


class FCN8s:

    def __init__(self, model_load_dir=None, tags=None, vgg16_dir=None, num_classes=None, variables_load_dir=None,
                 device_id=None, seed=0, widths=None, fc6_ksize=7):
        '''
        Arguments (first five: fcn8s_tensorflow.py:19-35; the rest are additions):
            model_load_dir (string, optional): directory written by `save(saver='saved_model')`, or a TensorFlow
                SavedModel directory written by the reference (its variables bundle is read).
            tags (list, optional): kept for signature parity; checked against the saved tags if given.
            vgg16_dir (string, optional): the VGG-16 SavedModel directory (variables bundle), a directory with
                `vgg16_weights.npz`, or 'synthetic[:seed]'.
            num_classes (int, optional): number of segmentation classes (any count up to 64; counts that are not a multiple of 4
                are padded inside the engine with classes of probability 0).
            variables_load_dir (string, optional): path prefix written by `save(saver='train_saver')`.
            device_id (int, optional): HIP device; defaults to LOCAL_RANK or 0.
            seed (int): dropout seed (rank is added in data-parallel runs).
        '''
        if (model_load_dir is None) and (vgg16_dir is None or num_classes is None):
            raise ValueError("You must provide either both `model_load_dir` and `tags` or both `vgg16_dir` and `num_classes`.")

        self.variables_load_dir = variables_load_dir
        self.model_load_dir = model_load_dir
        self.tags = tags
        self.vgg16_dir = vgg16_dir
        self.vgg16_tag = 'vgg16'
        self.num_classes = num_classes

        self.variables_updated = False
        self.eval_dataset = None
        # False: mean IoU over the classes that occur (tf.metrics.mean_iou of later TF 1.x); True: over all classes, absent ones
        # counting 0 -- the TF 1.3.0 the tutorial ran on (fcn8s_tutorial.ipynb:311).  Not a reference argument; set it on the instance.
        self.mean_iou_over_all_classes = False

        self.metric_names = []
        self.metric_values = []
        self.best_metric_values = []
        self.metric_value_tensors = []   # kept for attribute parity; hold metric names here
        self.metric_update_ops = []

        self.training_loss = None
        self.best_training_loss = 99999999.9
        self.g_step = None
        self.temperature = None          # set by fit_temperature (or restored from a saved model); `predict(temperature=...)` takes it
        self.pseudo_label_thresholds = None   # set by fit_pseudo_label_thresholds; they belong to a dataset and are not saved with the model

        if device_id is None:
            device_id = int(os.environ.get("LOCAL_RANK", "0"))
        rank = int(os.environ.get("RANK", "0"))

        fp8_calibration = None
        tf_prefix = tf_bundle.find_bundle_prefix(model_load_dir) if model_load_dir is not None else None
        if model_load_dir is not None and tf_prefix is not None and not os.path.isfile(os.path.join(model_load_dir, 'fcn8s_meta.json')):
            # a TensorFlow SavedModel / Saver checkpoint written by the reference (:922-934): variables, Adam slots, global_step
            tensors = tf_bundle.read_bundle(tf_prefix)
            if 'fc7_1x1/bias' not in tensors:
                raise ValueError("'{}' does not hold an FCN-8s checkpoint (no variable 'fc7_1x1/bias').".format(model_load_dir))
            self.num_classes = int(tensors['fc7_1x1/bias'].shape[0])
            w = tuple(int(tensors[k].shape[-1]) for k in ('conv1_2/filter', 'conv2_2/filter', 'conv3_3/filter', 'conv4_3/filter', 'conv5_3/filter', 'fc6/weights', 'fc7/weights'))
            self.engine = Engine(padded_classes(self.num_classes), widths=w, fc6_ksize=int(tensors['fc6/weights'].shape[0]), device_id=device_id, seed=seed + rank,
                                 logical_classes=self.num_classes)
            _load_tf_tensors(self.engine, tensors, with_state=True)
        elif model_load_dir is not None:
            meta = _read_meta(model_load_dir)
            if tags is not None and meta.get("tags") is not None and not set(tags) <= set(meta["tags"]):
                raise RuntimeError("MetaGraphDef associated with tags {} could not be found in SavedModel (available: {}).".format(tags, meta["tags"]))
            self.num_classes = int(meta["num_classes"])
            self.engine = Engine(padded_classes(self.num_classes), widths=meta.get("widths"), fc6_ksize=meta.get("fc6_ksize", 7),
                                 device_id=device_id, seed=seed + rank, logical_classes=self.num_classes)
            _load_checkpoint(self.engine, os.path.join(model_load_dir, "variables", "variables.npz"), with_state=True)
            fp8_calibration = meta.get("fp8_calibration")
            self.temperature = meta.get("temperature")
            if meta.get("ema_decay"):         # behind the checkpoint: a restored shadow is kept, not set to the parameters
                self.engine.set_ema(meta["ema_decay"], meta.get("ema_warmup", True))
        else:
            self.engine = Engine(padded_classes(num_classes), widths=widths, fc6_ksize=fc6_ksize, device_id=device_id, seed=seed + rank,
                                 logical_classes=num_classes)
            self._load_vgg16()
            if variables_load_dir is not None:
                self.load_variables(variables_load_dir)
        self.engine.broadcast_params(0)
        if fp8_calibration is not None:      # after the parameters: writing them clears a calibration
            self.engine.set_fp8_calibration(fp8_calibration)
        self.engine.metrics_reset()

    # fcn8s_tensorflow.py:127-152 -- the encoder weights enter here
    def _load_vgg16(self):
        d = str(self.vgg16_dir)
        if d.startswith('synthetic'):
            s = int(d.split(':', 1)[1]) if ':' in d else 0
            self.engine.init_params(seed=s)
            return
        prefix = tf_bundle.find_bundle_prefix(d)
        if prefix is not None:                       # the reference's VGG-16 SavedModel (README.md:42): variables bundle
            self.engine.init_params(seed=0)          # decoder: truncated normal (:159-160); encoder overwritten below
            tensors = tf_bundle.read_bundle(prefix)
            params = {k: v for k, v in tensors.items() if k in self.engine.specs and (k.startswith('conv') or k.startswith('fc6/') or k.startswith('fc7/'))}
            missing = [k for k in self.engine.specs if (k.startswith('conv') or k.startswith('fc6/') or k.startswith('fc7/')) and k not in params]
            if missing:
                raise ValueError("the VGG-16 checkpoint lacks variables: {}".format(missing[:5]))
            self.engine.set_params(params)
            return
        npz = os.path.join(d, 'vgg16_weights.npz')
        if os.path.isfile(npz):
            self.engine.init_params(seed=0)          # decoder: truncated normal (:159-160); encoder overwritten below
            data = np.load(npz)
            params = {k: data[k] for k in data.files if k in self.engine.specs}
            missing = [k for k in self.engine.specs if ('conv' in k.split('/')[0] and 'trans' not in k or k.startswith('fc6/') or k.startswith('fc7/')) and k not in params]
            if missing:
                raise ValueError("vgg16_weights.npz lacks variables: {}".format(missing[:5]))
            self.engine.set_params(params)
            return
        raise ValueError("`vgg16_dir` must contain a TensorFlow SavedModel (variables/variables.index), vgg16_weights.npz, or be 'synthetic[:seed]', got '{}'.".format(d))

    def _initialize_metrics(self, metrics):
        '''fcn8s_tensorflow.py:371-397'''
        table = (('loss', 99999999.9, 'mean_loss'), ('mean_iou', 0.0, 'mean_iou'), ('accuracy', 0.0, 'acc'))
        chosen = [row for row in table if row[0] in metrics]
        self.metric_names = [name for name, _, _ in chosen]
        self.best_metric_values = [worst for _, worst, _ in chosen]
        self.metric_update_ops = [stem + '_update_op' for _, _, stem in chosen]      # names only: there is no graph
        self.metric_value_tensors = [stem + '_value' for _, _, stem in chosen]

    def train(self,
              train_generator,
              epochs,
              steps_per_epoch,
              learning_rate_schedule,
              keep_prob=0.5,
              l2_regularization=0.0,
              eval_dataset='train',
              eval_frequency=5,
              val_generator=None,
              val_steps=None,
              metrics={},
              save_during_training=False,
              save_dir=None,
              save_best_only=True,
              save_tags=['default'],
              save_name='',
              save_frequency=5,
              saver='saved_model',
              monitor='loss',
              record_summaries=True,
              summaries_frequency=10,
              summaries_dir=None,
              summaries_name=None,
              training_loss_display_averaging=3,
              class_weights=None,
              ohem_thresh=None,
              ohem_min_kept=100000,
              lovasz_weight=0.0,
              lovasz_per_image=False,
              lovasz_classes='present',
              ce_weight=1.0,
              boundary_weight=None,
              boundary_sigma=None,
              boundary_radius=None,
              boundary_ignore_band=None,
              accumulation_steps=1,
              clip_global_norm=None,
              ema_decay=None,
              ema_warmup=True,
              ema_evaluate=True,
              teacher=None,
              distill_weight=1.0,
              distill_temperature=1.0,
              distill_pixels='valid',
              teacher_predict=None,
              unlabeled_generator=None,
              unlabeled_labeler='self',
              unlabeled_thresholds=None,
              unlabeled_predict=None,
              unlabeled_mix=True,
              unlabeled_seed=0,
              unlabeled_augment=None,
              entropy_weight=0.0,
              entropy_pixels='unlabeled',
              entropy_images='all',
              focal_gamma=0.0,
              fda_beta=None):
        '''Trains the model; arguments as fcn8s_tensorflow.py:424-503.  Summaries are written as TensorBoard
        event files (`<summaries_dir>/<summaries_name>[_eval]/events.out.tfevents.*`: total_loss, learning_rate and
        mean / stddev / max / min / histogram of the ten watched weight-bias pairs, :331-366) and, for reading
        without TensorBoard, as JSON lines (`scalars.jsonl`) next to them; if `summaries_dir` is None nothing is recorded.
        `class_weights` (one per class), `ohem_thresh` (a probability in (0, 1]) and `ohem_min_kept` set the training loss for the duration
        of the call (Engine.set_loss, loss.py: class-weighted and / or hard-pixel-mined cross-entropy); the evaluations keep reporting the
        reference's loss, and the previous loss configuration is restored when train() returns or raises.
        `lovasz_weight`, `lovasz_per_image`, `lovasz_classes` ('present', 'all' or a list of class ids) and `ce_weight` add the
        Lovász-softmax term for the duration of the call (Engine.set_lovasz, loss.py: ce_weight * cross-entropy + lovasz_weight * Lovász);
        the evaluations keep reporting the reference's loss, and the previous configuration is restored when train() returns or raises.
        `boundary_weight` + `boundary_sigma` (U-Net's weight map 1 + weight * exp(-d^2 / 2 sigma^2) around the ground-truth boundaries, out to
        `boundary_radius` pixels, default min(15, ceil(3 sigma))) and / or `boundary_ignore_band` = k (weight 0 within k pixels of a boundary)
        weight the cross-entropy's pixels by their distance to the nearest boundary of the step's own labels for the duration of the call
        (loss.resolve_boundary, Engine.set_boundary_loss); the evaluations keep reporting the reference's loss, and the previous
        configuration is restored when train() returns or raises.  Data-parallel runs need nothing: each rank weights its own labels.
        `accumulation_steps` = A >= 1: an update consumes A batches from the generator (Engine.accumulate_step for the first A - 1,
        Engine.train_step for the last; optim.py), its gradient is their mean and its reported loss the mean of their losses;
        `steps_per_epoch`, the global step, the learning-rate schedule, `summaries_frequency` and the saves all count updates.
        `clip_global_norm` (positive; inf = skip non-finite updates only) clips every update's gradient by its global norm for the duration
        of the call (Engine.set_grad_clip); `grad_norm` and `clip_coef` then join the recorded scalars, on the steps that are recorded.
        `ema_decay` in (0, 1) keeps an exponential moving average of the parameters for the duration of the call (Engine.set_ema, optim.py;
        `ema_warmup`: TensorFlow's num_updates rule); the engine's previous setting is restored when train() returns or raises, the shadow
        stays.  With `ema_evaluate` the in-training evaluations and the `save_during_training` saves run on the averaged weights
        (Engine.averaged_weights); the live weights are the raw ones again when train() returns or raises.  Use
        `with model.averaged_weights():` around evaluate / predict / save afterwards.
        `teacher` adds the soft-target term distill_weight * T^2 / P * sum_p KL(teacher_p || student_p) at T = `distill_temperature` for the
        duration of the call (Engine.set_soft_targets, loss.py; `distill_pixels` = 'valid': the pixels with a label, 'all': every pixel, so that
        unlabelled frames train too): another FCN8s on the same device with the same number of classes (any widths or precision), or a
        callable mapping the batch's device images (a cuda tensor [N, H, W, 3]) to a cuda float32 softmax [N, H, W, num_classes].  Per batch,
        each accumulated micro-batch included, the images are uploaded once, the teacher runs device in / device out, its result is bound
        (Engine.bind_soft_targets) and the step runs on the same device images.  `teacher_predict`: keywords of the teacher's `predict`
        (`scales`, `flip`, `crf`, `temperature`), or `samples` / `keep_prob` for the Monte-Carlo mean of `predict_uncertainty`.  A teacher
        model is frozen for the duration of the call and its frozen state restored afterwards; the student's previous soft-target setting is
        restored when train() returns or raises.  While a teacher is set the batches are fed unstaged (no copy of batch k + 1 behind step
        k).  `distill_loss` (the unscaled term) joins the recorded scalars on the steps that are recorded.
        `unlabeled_generator` adds online self-training with class mixing (ClassMix, Olsson et al. 2021; DACS, Tranheden et al. 2021;
        class_mix.py): per update, and per micro-batch under `accumulation_steps`, a batch of M >= 2 unlabelled uint8 images of the labelled
        batch's height and width is drawn from it (of a tuple the first element is taken), uploaded once and labelled on the device:
        `unlabeled_labeler` = 'self' predicts with the student as it is (dropout off), 'ema' with its averaged weights (a mean teacher: the
        prediction runs inside `averaged_weights()`, the raw weights are back before the step; needs `ema_decay` or an existing average),
        another FCN8s on the same device with the same number of classes predicts with that model, frozen for the call as a `teacher` is.
        `unlabeled_predict`: keywords of that prediction (`scales`, `flip`, `crf`, `temperature`, or `samples` / `keep_prob` / `mi_max`, as in
        `fit_pseudo_label_thresholds`).  The softmax becomes hard labels by `Engine.pseudo_label` with `unlabeled_thresholds` (a float, one
        value per class, or None: `self.pseudo_label_thresholds`, and ValueError if there are none) and the ignore id 255; with
        `unlabeled_mix`, `Engine.class_mix` then pastes half of the classes of image (n + 1) mod M onto image n, pixels and labels alike,
        with seed `unlabeled_seed` + rank and draw (global step) * accumulation_steps + micro-batch index, so that a resumed run mixes as the
        uninterrupted one would.  The labelled batch's labels are brought to uint8 ids on the device, both batches are joined into one of
        N + M images and the ordinary step runs on it: the loss ignores ids >= num_classes and its mean runs over all (N + M) H W pixels, so
        the unlabelled term's weight is its pixel share.  The batches are fed unstaged, as under a teacher.  `pseudo_kept`, the share of the
        unlabelled pixels that kept a label (the last micro-batch's), joins the recorded scalars on the steps that are recorded.  Together
        with `teacher` it raises.  With 'self' and 'ema' the student's engine sees batches of M and of N + M in turn and re-allocates its
        workspace at every change of shape, which can cost far more than the prediction (README: timing); a labeler model of its own keeps
        both engines on one shape.
        `unlabeled_augment` adds DACS's strong augmentation of the student's view (strong_augment.py): after the mixing -- and with
        `unlabeled_mix=False` too -- `Engine.strong_augment` recolours and blurs the unlabelled images with the mixing's seed and draw; the
        labeler has already seen the clean images and the labels do not change.  None: off (nothing new is launched or allocated); True:
        `strong_augment.DEFAULTS` (colour jitter with probability 0.8 and strength 0.25 on brightness, contrast and saturation, hue within a
        quarter of +-90 units, Gaussian blur with probability 0.5, sigma in [0.15, 1.15] in 16 levels, radius 4 -- DACS's settings as
        recalled, not checked against its code); a dict overrides fields of those.  Without `unlabeled_generator` it raises.
        `entropy_weight` adds the entropy of the student's own prediction to the loss for the duration of the call (Engine.set_entropy_term,
        loss.py): entropy_weight / (P log K) * sum_{p in U} h_p over the K classes, P all pixels of the step's batch.  A positive weight is
        entropy minimisation (Grandvalet & Bengio 2005; MinEnt of ADVENT, Vu et al. 2019, which uses 0.001 -- that paper's value as recalled,
        not checked against its code), the one term that trains on a pixel without a label and needs no labeler, threshold or second model; a
        negative weight is the confidence penalty on labelled pixels (Pereyra et al. 2017); 0, the default, is off: nothing is launched or
        allocated and the step is bit for bit what it was.  `entropy_pixels`: 'unlabeled' (the pixels whose label id is >= num_classes: void
        pixels, and under `unlabeled_generator` the pixels below their class threshold), 'valid' (the pixels with a label) or 'all'.
        `entropy_images`: 'all' takes every image of the batch; 'unlabeled' needs `unlabeled_generator` (it raises otherwise) and restricts the
        term to the M unlabelled images of the joined batch, so that the void pixels of the labelled images stay out.  It combines with
        `teacher` and with every `unlabeled_*` keyword.  The engine's previous setting is restored when train() returns or raises.
        `entropy_loss` (the unscaled term, the last micro-batch's) joins the recorded scalars on the steps that are recorded.
        `focal_gamma` in (0, 8] turns the cross-entropy into the focal loss (Lin et al. 2017) for the duration of the call (Engine.set_focal,
        loss.py): every pixel's l_p is scaled by (1 - p_y)^gamma, so that the many easy pixels and confident pseudo-labels stop dominating the
        gradient; the denominator stays P.  2 is the paper's default, not a value tuned here.  `class_weights` act as its alpha, the boundary
        table acts on it, the Lovász, soft-target and entropy terms add behind it; together with `ohem_thresh` (or an OHEM configuration the
        engine already has) it raises, because both address the same thing.  0, the default, is off: nothing new is launched or allocated and
        the step is bit for bit what it was.  The evaluations keep reporting the reference's loss, and the engine's previous setting is
        restored when train() returns or raises.
        `fda_beta` adds Fourier domain adaptation of the labelled batch (FDA, Yang & Soatto 2020; fda.py): a float in (0, 0.09] needs
        `unlabeled_generator` (it raises otherwise); per batch, and per micro-batch under `accumulation_steps`, the labelled uint8 images x
        become `Engine.fda_transfer(x, u, beta=fda_beta, pair=(n + draw) mod M)` -- the amplitudes of the (2 b + 1)^2 lowest frequencies,
        b = floor(min(H, W) fda_beta), of labelled image n are replaced by those of the CLEAN unlabelled image (n + draw) mod M, the phases
        stay -- as soon as the unlabelled batch u is on the device and before anything changes it.  `draw` is the mixing's, so a resumed run
        pairs as the uninterrupted one would.  The labels do not change, the labeler still sees the clean u, and everything downstream is
        as it is without the keyword; it works with every `unlabeled_labeler`, with `unlabeled_mix=False` and under `accumulation_steps`.
        0.01 is the paper's smallest band, not a value tuned here.  A b above 96 (a short side of 1078 or more at 0.09) raises when the first
        batch of that size is joined, before anything of that batch is launched; an update that it cuts short is discarded.  None, the default, is off: nothing new is launched or allocated.
        Not done here: the paper's multi-band ensemble of three models, a style source other than the unlabelled batch, FDA of the unlabelled
        images, float training images, a separate weight on the unlabelled term (change M), a per-class or per-pixel weight or a threshold on the entropy,
        ADVENT's adversarial branch, CutMix boxes, geometric strong augmentation, augmenting or
        mixing the labelled images, and any change to `BatchGenerator`.'''
        if self.engine.precision == 'fp8_infer':
            raise ValueError("The 'fp8_infer' precision is inference only; switch the engine to another precision "
                             "(e.g. model.engine.set_precision('bf16_train')) before training.")
        _check_metric_names(metrics)
        custom_loss = class_weights is not None or bool(ohem_thresh)
        if custom_loss:
            loss_mod.validate(class_weights, ohem_thresh, ohem_min_kept, self.engine.logical_classes)
        custom_lovasz = lovasz_weight != 0 or ce_weight != 1.0
        if custom_lovasz:
            loss_mod.validate_lovasz(lovasz_weight, ce_weight, lovasz_per_image, lovasz_classes, self.engine.logical_classes)
        boundary_table, boundary_R = loss_mod.resolve_boundary(boundary_weight, boundary_sigma, boundary_radius, boundary_ignore_band)
        custom_boundary = boundary_table is not None
        accumulation_steps, max_norm = optim_mod.validate(accumulation_steps, clip_global_norm)
        ema_d, ema_w = optim_mod.validate_ema(ema_decay, ema_warmup)
        teacher_fn = self._resolve_teacher(teacher, teacher_predict, distill_weight, distill_temperature, distill_pixels)
        unlabeled = self._resolve_unlabeled(unlabeled_generator, unlabeled_labeler, unlabeled_thresholds, unlabeled_predict, unlabeled_mix,
                                            unlabeled_seed, teacher, bool(ema_d), unlabeled_augment, fda_beta)
        entropy = self._resolve_entropy(entropy_weight, entropy_pixels, entropy_images, unlabeled_generator)
        focal = loss_mod.validate_focal(focal_gamma, ohem_thresh if custom_loss else (self.engine.loss_config or {}).get('ohem_thresh'))
        if not focal and self.engine.focal_config is not None:
            loss_mod.validate_focal(self.engine.focal_config['gamma'], ohem_thresh)     # the engine's own focal setting meets this call's OHEM
        if eval_dataset not in ('train', 'val'):
            raise ValueError("`eval_dataset` must be one of 'train' or 'val', but is '{}'.".format(eval_dataset))
        if eval_dataset == 'val' and (val_generator is None or val_steps is None):
            raise ValueError("When eval_dataset == 'val', a `val_generator` and `val_steps` must be passed.")
        if monitor != 'loss' and monitor not in metrics:
            raise ValueError('You are trying to monitor {}, but it is not in `metrics` and is therefore not being computed.'.format(monitor))

        self.eval_dataset = eval_dataset
        self._initialize_metrics(metrics)
        self.g_step = self.engine.global_step
        self._lr = learning_rate_schedule(self.g_step)       # the schedule is called once here and once after every step (:527, :583)

        train_log = eval_log = None
        if record_summaries and summaries_dir is not None and self.engine.rank == 0:
            run = summaries_name or 'training'
            train_log = _ScalarLog(os.path.join(summaries_dir, run), engine=self.engine)
            if metrics:
                eval_log = _ScalarLog(os.path.join(summaries_dir, run + '_eval'))

        eval_source = {'train': (train_generator, steps_per_epoch, 'Evaluation on training dataset'),
                       'val': (val_generator, val_steps, 'Evaluation on validation dataset')}[eval_dataset]

        prev_loss = self.engine.loss_config
        prev_lovasz = self.engine.lovasz_config
        prev_boundary = self.engine.boundary_config
        prev_clip = self.engine.grad_clip
        prev_ema = self.engine.ema_config
        prev_soft = self.engine.soft_target_config
        prev_entropy = self.engine.entropy_config
        prev_focal = self.engine.focal_config
        teacher_engine = teacher.engine if (teacher_fn is not None and isinstance(teacher, FCN8s)) else None
        teacher_was_frozen = bool(teacher_engine.get_option("frozen")) if teacher_engine is not None else False
        labeler_engine = unlabeled.labeler_engine if unlabeled is not None else None
        labeler_was_frozen = bool(labeler_engine.get_option("frozen")) if labeler_engine is not None else False
        try:
            if labeler_engine is not None:
                labeler_engine.freeze(True)
            if teacher_fn is not None:
                self.engine.set_soft_targets(distill_weight, distill_temperature, distill_pixels)
                if teacher_engine is not None:
                    teacher_engine.freeze(True)
            if ema_d:
                self.engine.set_ema(ema_d, ema_w)
            averaged = self.engine.averaged_weights if (ema_evaluate and self.engine.ema_config) else contextlib.nullcontext
            if max_norm:
                self.engine.set_grad_clip(max_norm)
            if custom_loss:
                self.engine.set_loss(class_weights, ohem_thresh, ohem_min_kept)
            if custom_lovasz:
                self.engine.set_lovasz(lovasz_weight, ce_weight, lovasz_per_image, lovasz_classes)
            if custom_boundary:
                self.engine.set_boundary_loss(boundary_table, boundary_R)
            if focal:
                self.engine.set_focal(focal)
            if entropy is not None and not entropy['per_batch']:
                self.engine.set_entropy_term(entropy['weight'], entropy['pixels'])
            if unlabeled is not None:
                unlabeled.entropy = entropy if (entropy is not None and entropy['per_batch']) else None
            for epoch in range(1, epochs + 1):
                self._run_epoch(train_generator, steps_per_epoch, learning_rate_schedule, keep_prob, l2_regularization,
                                'Epoch {}/{}'.format(epoch, epochs), training_loss_display_averaging,
                                train_log, summaries_frequency, accumulation_steps, teacher_fn, unlabeled, entropy is not None)
                eval_epoch = epoch % eval_frequency == 0

                if metrics and eval_epoch:
                    generator, num_batches, description = eval_source
                    with averaged():
                        self._evaluate(generator, metrics, num_batches, l2_regularization, description)
                    if eval_log is not None:
                        eval_log.add(self.g_step, **{('mean_loss' if n == 'loss' else n): v for n, v in zip(self.metric_names, self.metric_values)})    # tags of :360-362

                if save_during_training and epoch % save_frequency == 0 and self._wants_save(save_best_only, monitor):
                    with averaged():
                        self.save(model_save_dir=save_dir, saver=saver, tags=save_tags, name=save_name,
                                  include_global_step=True, include_last_training_loss=True,
                                  include_metrics=bool(self.metric_names))

                # Bests are updated after the save decision (fcn8s_tensorflow.py:648-658).
                self.best_training_loss = min(self.best_training_loss, self.training_loss)
                if eval_epoch:
                    for i, name in enumerate(self.metric_names):
                        if self._improved(name, i):
                            self.best_metric_values[i] = self.metric_values[i]
        finally:
            if self.engine.pending_micro_batches:      # an update that an exception cut short: its micro-batches must not leak into the next one
                self.engine.discard_accumulated()
            if max_norm:
                self.engine.set_grad_clip(prev_clip)
            if ema_d:
                self.engine.set_ema(**(prev_ema or dict(decay=None)))
            if focal:                                   # (in front of the loss: a previous OHEM configuration comes back only with the focal loss off)
                self.engine.set_focal(**(prev_focal or {}))
            if custom_loss:
                self.engine.set_loss(**(prev_loss or {}))
            if custom_lovasz:
                self.engine.set_lovasz(**(prev_lovasz or dict(lovasz_weight=0.0)))
            if custom_boundary:
                self.engine.set_boundary_loss(**(prev_boundary or {}))
            if entropy is not None:
                self.engine.set_entropy_term(**(prev_entropy or {}))
            if teacher_fn is not None:
                self.engine.set_soft_targets(**(prev_soft or {}))
                if teacher_engine is not None:
                    teacher_engine.freeze(teacher_was_frozen)
            if labeler_engine is not None:
                labeler_engine.freeze(labeler_was_frozen)
            for log in (train_log, eval_log):          # the event files are complete and closed when train() returns or raises
                if log is not None:
                    log.close()

    def fda_transfer(self, images, targets, beta=0.01, pair=None):
        '''Fourier domain adaptation (FDA, Yang & Soatto 2020; fda.py, `Engine.fda_transfer`) of uint8 `images` [N,H,W,3] towards uint8
        `targets` [M,H,W,3] of the same height and width: the amplitudes of the (2 b + 1)^2 lowest frequencies, b = floor(min(H, W) beta),
        of image n become those of target pair[n] (None: n mod M), the phases stay.  NumPy arrays or device tensors; returns the same kind
        (uint8, clamp(rint(y), 0, 255)).'''
        torch = self.engine.torch
        on_device = isinstance(images, torch.Tensor) and images.is_cuda
        x, t = (a if isinstance(a, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(a)) for a in (images, targets))
        if x.dtype != torch.uint8 or t.dtype != torch.uint8 or x.dim() != 4 or t.dim() != 4:
            raise ValueError("`images` and `targets` must be uint8 [N, H, W, 3].")
        out = self.engine.fda_transfer(x.to(self.engine.device).contiguous(), t.to(self.engine.device).contiguous(), beta=beta, pair=pair)
        return out if on_device else out.cpu().numpy()

    def _resolve_teacher(self, teacher, teacher_predict, weight, temperature, pixels):
        '''train()'s teacher arguments -> None (no teacher, or weight 0) or a function: device images -> device softmax.'''
        if teacher is None:
            if teacher_predict is not None:
                raise ValueError("`teacher_predict` needs a `teacher`.")
            return None
        w, _, _ = loss_mod.validate_soft_targets(weight, temperature, pixels)
        kw = dict(teacher_predict or {})
        if not isinstance(teacher, FCN8s):
            if not callable(teacher):
                raise ValueError("`teacher` must be an FCN8s or a callable mapping device images to a device softmax, got {!r}.".format(teacher))
            if kw:
                raise ValueError("`teacher_predict` goes with an FCN8s teacher; a callable teacher takes the images alone.")
            return teacher if w else None
        if teacher is self or teacher.engine is self.engine:
            raise ValueError("`teacher` must be another model: training changes the student's weights under a frozen teacher.")
        if teacher.engine.device != self.engine.device:
            raise ValueError("`teacher` must live on the student's device ({}), but is on {}.".format(self.engine.device, teacher.engine.device))
        if teacher.engine.logical_classes != self.engine.logical_classes:
            raise ValueError("`teacher` has {} classes, the student {}.".format(teacher.engine.logical_classes, self.engine.logical_classes))
        monte_carlo = 'samples' in kw or 'keep_prob' in kw
        allowed = {'samples', 'keep_prob'} if monte_carlo else {'scales', 'flip', 'crf', 'temperature'}
        if set(kw) - allowed:
            raise ValueError("`teacher_predict` takes `scales`, `flip`, `crf`, `temperature`, or `samples` / `keep_prob` for the Monte-Carlo "
                             "mean; got {}.".format(sorted(kw)))
        if not w:
            return None
        if monte_carlo:
            return lambda images: teacher.predict_uncertainty(images, argmax=False, **kw)[0]
        return lambda images: teacher.predict(images, argmax=False, **kw)

    def _resolve_entropy(self, weight, pixels, images, unlabeled_generator):
        '''train()'s entropy arguments -> None (weight 0: off) or dict(weight, pixels, per_batch): with `per_batch` (entropy_images =
        'unlabeled') the term is set for every joined batch with first_image = the labelled batch's size.'''
        w, _, _ = loss_mod.validate_entropy_term(weight, pixels, 0)
        if images not in ('all', 'unlabeled'):
            raise ValueError("`entropy_images` must be 'all' or 'unlabeled', got {!r}.".format(images))
        if images == 'unlabeled' and unlabeled_generator is None:
            raise ValueError("entropy_images='unlabeled' needs an `unlabeled_generator`: without one the batch has no unlabelled images.")
        if not w:
            return None
        return dict(weight=w, pixels=pixels, per_batch=images == 'unlabeled')

    def _bind_teacher(self, teacher_fn, images):
        '''One batch under a teacher: the images on the device (uploaded once), the teacher's softmax of them bound as the next training
        loss's targets.  Returns the device images for the step.'''
        dev = self.engine._images(images, force_device=True)[0]
        self.engine.bind_soft_targets(teacher_fn(dev))
        return dev

    def _resolve_unlabeled(self, generator, labeler, thresholds, predict, mix, seed, teacher, ema_requested, augment=None, fda_beta=None):
        '''train()'s unlabelled-batch arguments -> None (no generator) or the state of the route: the generator, `label` (device images ->
        (device softmax, score map | None)), the thresholds on the device, the tables `Engine.pseudo_label` counts into, and the mixing's
        settings.'''
        if generator is None:
            if labeler != 'self' or thresholds is not None or predict is not None:
                raise ValueError("`unlabeled_labeler`, `unlabeled_thresholds` and `unlabeled_predict` need an `unlabeled_generator`.")
            sa_mod.validate(augment, has_generator=False)
            fda_mod.validate(fda_beta, has_generator=False)
            return None
        augment = sa_mod.validate(augment)
        fda_beta = fda_mod.validate(fda_beta)
        has_average = ema_requested or self.engine.ema_info()['has_shadow']
        v = cm_mod.validate(self.num_classes, labeler=labeler, thresholds=thresholds, predict=predict, mix=mix, seed=seed, teacher=teacher,
                            has_average=has_average, model_thresholds=self.pseudo_label_thresholds, student=self)
        model = self if isinstance(labeler, str) else labeler
        kw = v['predict']
        route = sweeps.resolve_route(model, kw.get('scales'), kw.get('flip', False), kw.get('crf'), kw.get('temperature'), kw.get('samples'),
                                     kw.get('keep_prob', 0.5), mi_max=kw.get('mi_max'))
        routed = lambda images: route.softmax(images, mutual_information=kw.get('mi_max') is not None)[::2]
        predict_fn = routed if kw else (lambda images: (model.predict(images, argmax=False), None))
        if labeler == 'ema':
            def label(images):
                with self.engine.averaged_weights():
                    return predict_fn(images)
        else:
            label = predict_fn
        torch = self.engine.torch
        dev = self.engine.device
        Cn = self.num_classes
        flat = torch.zeros(2 * Cn + 3, dtype=torch.int64, device=dev)
        return _Unlabeled(generator=generator, label=label, thresholds=torch.from_numpy(v['thresholds']).to(dev), mi_max=kw.get('mi_max'),
                          mix=v['mix'], seed=v['seed'] + self.engine.rank, flat=flat, augment=augment, fda_beta=fda_beta,
                          tables=dict(hist=None, counts=flat[:2 * Cn].view(Cn, 2), misc=flat[2 * Cn:]),
                          labeler_engine=None if isinstance(labeler, str) else labeler.engine)

    def _join_unlabeled(self, unl, images, labels, draw):
        '''One batch of the self-training route: the labelled batch on the device with uint8 ids, an unlabelled batch drawn, labelled,
        thresholded, (with `mix`) class-mixed and (with `augment`) recoloured and blurred on the device, both joined; with `fda_beta` the labelled images are first
        adapted to the clean unlabelled ones.  Returns the device images and labels for the step.'''
        torch = self.engine.torch
        dev = self.engine.device
        x = self.engine._images(images, force_device=True)[0]
        if x.dtype != torch.uint8:
            raise ValueError("`unlabeled_generator` needs uint8 images from `train_generator` (the joined batch is one uint8 tensor).")
        nhw = tuple(int(d) for d in x.shape[:3])
        fda_b = None
        if unl.fda_beta is not None:                                # refused here: nothing of this batch has been launched, no unlabelled batch drawn
            fda_b = fda_mod.check_half_width(nhw[1], nhw[2], fda_mod.half_width(nhw[1], nhw[2], unl.fda_beta))
        lab_rank = labels.dim() if isinstance(labels, torch.Tensor) else np.ndim(labels)
        if lab_rank == 4:
            t = labels if isinstance(labels, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(labels))
            ids = self.engine._onehot_to_ids(t, nhw)
        elif lab_rank == 3:
            ids = (labels if isinstance(labels, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(labels, dtype=np.uint8)))
            ids = ids.to(torch.uint8).to(dev).contiguous()
            if tuple(ids.shape) != nhw:
                raise ValueError("labels shape %s does not match images %s" % (tuple(ids.shape), nhw))
        else:
            raise ValueError("labels must be one-hot (batch, height, width, num_classes) or class ids (batch, height, width)")
        batch = next(unl.generator)
        if isinstance(batch, tuple):
            batch = batch[0]
        u = self.engine._images(batch, force_device=True)[0]
        if u.dtype != torch.uint8 or u.shape[0] < 2 or tuple(u.shape[1:3]) != nhw[1:]:
            raise ValueError("`unlabeled_generator` must yield at least 2 uint8 images of the labelled batch's size {}x{}, got {} of dtype {}."
                             .format(nhw[1], nhw[2], tuple(u.shape), u.dtype))
        if unl.fda_beta is not None:                                # the labelled images take the clean unlabelled images' low-frequency amplitudes
            if unl.fda_base is None or unl.fda_base.numel() != nhw[0]:          # 0 .. N - 1 on the device, made once: the pairing uploads nothing
                unl.fda_base = torch.arange(nhw[0], dtype=torch.int32, device=dev)
            pair = torch.remainder(unl.fda_base + int(draw) % int(u.shape[0]), int(u.shape[0]))
            x = self.engine.fda_transfer(x, u, b=fda_b, pair=pair)
        prob, score = unl.label(u)
        unl.flat.zero_()
        pseudo, _ = self.engine.pseudo_label(prob, thresholds=unl.thresholds, ignore_id=255, score=score,
                                             score_max=unl.mi_max if score is not None else None, labels=True, tables=unl.tables)
        unl.pixels = int(pseudo.numel())
        if unl.mix:
            u, pseudo = self.engine.class_mix(u, pseudo, seed=unl.seed, draw=draw)
        if unl.augment is not None:                                 # the student's view only: the labeler has seen the clean images
            u = self.engine.strong_augment(u, seed=unl.seed, draw=draw, jitter=unl.augment['jitter'], blur=unl.augment['blur'])
        if unl.entropy is not None:                                 # the term on the M unlabelled images only (host state: nothing is launched)
            self.engine.set_entropy_term(unl.entropy['weight'], unl.entropy['pixels'], first_image=nhw[0])
        return torch.cat([x, u]), torch.cat([ids, pseudo])

    def _run_epoch(self, generator, steps, schedule, keep_prob, l2_rate, title, window, log, log_every, accumulation_steps=1, teacher_fn=None,
                   unlabeled=None, entropy=False):
        '''One epoch of train steps (fcn8s_tensorflow.py:542-590): a step runs with the schedule's value
        at the global step before it; `training_loss` is the mean over the last `window` steps.  With `accumulation_steps` = A > 1 a
        step is one update over A batches: A - 1 accumulated micro-batches, then the train step; its loss is the mean of the A losses.'''
        recent = deque(maxlen=window)
        bar = trange(steps, file=sys.stdout, disable=self.engine.rank != 0)
        bar.set_description(title)
        # batch k+1 is decoded / staged / copied while step k runs (under a teacher: decoded only -- the teacher reads the images as a tensor)
        feed = _Feeder(self.engine, generator, steps * accumulation_steps, stage=teacher_fn is None and unlabeled is None)
        try:
            for _ in bar:
                lr = self._lr
                micro = []
                for _k in range(accumulation_steps - 1):
                    images, labels = feed.next()
                    if teacher_fn is not None:
                        images = self._bind_teacher(teacher_fn, images)
                    if unlabeled is not None:
                        images, labels = self._join_unlabeled(unlabeled, images, labels, self.g_step * accumulation_steps + _k)
                    micro.append(self.engine.accumulate_step(images, labels, keep_prob=keep_prob, l2_rate=l2_rate))
                images, labels = feed.next()
                if teacher_fn is not None:
                    images = self._bind_teacher(teacher_fn, images)
                if unlabeled is not None:
                    images, labels = self._join_unlabeled(unlabeled, images, labels, self.g_step * accumulation_steps + accumulation_steps - 1)
                loss, self.g_step = self.engine.train_step(images, labels, learning_rate=lr, keep_prob=keep_prob, l2_rate=l2_rate)
                if micro:
                    loss = float(np.mean(micro + [loss]))
                self.variables_updated = True
                if log is not None and (self.g_step - 1) % log_every == 0:
                    extra = {}
                    if self.engine.grad_clip is not None:      # (reading them synchronises: only on the steps that are recorded)
                        st = self.engine.update_stats()
                        extra.update(grad_norm=st['norm'], clip_coef=st['clip_coef'])
                    if teacher_fn is not None:                 # (the last micro-batch's term)
                        extra.update(distill_loss=self.engine.soft_target_term())
                    if entropy:                                # (the last micro-batch's term)
                        extra.update(entropy_loss=self.engine.entropy_term())
                    if unlabeled is not None:                  # (the last micro-batch's share; the download synchronises)
                        extra.update(pseudo_kept=float(unlabeled.tables['counts'][:, 0].sum().item()) / unlabeled.pixels)
                    log.add(self.g_step, total_loss=loss, learning_rate=lr, **extra)
                recent.append(loss)
                self.training_loss = float(np.mean(recent))
                bar.set_postfix(ordered_dict={'loss': self.training_loss, 'learning rate': lr})
                self._lr = schedule(self.g_step)
        finally:
            feed.close()

    def _improved(self, name, i):
        '''Whether metric `i` beat its best.  The reference compares the name against
        ['accuracry', 'mean_iou'] (fcn8s_tensorflow.py:626,:656), so 'accuracy' never counts as an
        improvement there; kept, because `best_metric_values` and save decisions depend on it.'''
        if name == 'loss':
            return self.metric_values[i] < self.best_metric_values[i]
        if name == 'mean_iou':
            return self.metric_values[i] > self.best_metric_values[i]
        return False

    def _wants_save(self, best_only, monitor):
        '''Save decision of fcn8s_tensorflow.py:612-634.'''
        if not best_only:
            return True
        if monitor == 'loss' and 'loss' not in self.metric_names:
            better = self.training_loss < self.best_training_loss
        else:
            better = self._improved(monitor, self.metric_names.index(monitor))
        if better:
            print('New best {} value, saving model.'.format(monitor))
        else:
            print('No improvement over previous best {} value, not saving model.'.format(monitor))
        return better

    def _evaluate(self, data_generator, metrics, num_batches, l2_regularization, description='Running evaluation'):
        '''fcn8s_tensorflow.py:660-697'''
        self.engine.metrics_reset()

        tr = trange(num_batches, file=sys.stdout, disable=self.engine.rank != 0)
        tr.set_description(description)

        self.engine.freeze(True)            # no training inside an evaluation loop: transformed filters are built once
        feed = _Feeder(self.engine, data_generator, num_batches)
        try:
            for step in tr:
                batch_images, batch_labels = feed.next()
                self.engine.eval_step(batch_images, batch_labels, l2_rate=l2_regularization)
        finally:
            feed.close()
            self.engine.freeze(False)

        self.engine.metrics_allreduce()
        values = dict(zip(('loss', 'mean_iou', 'accuracy'), self.engine.metrics_get(all_classes=self.mean_iou_over_all_classes)))
        self.metric_values = [values[n] for n in self.metric_names]

        if self.engine.rank == 0:
            print(''.join('{}: {:.4f}  '.format(n, v) for n, v in zip(self.metric_names, self.metric_values)))

    def averaged_weights(self):
        '''Not in the reference: `with model.averaged_weights():` makes the exponential moving average of the parameters that
        `train(..., ema_decay=...)` kept the live weights for the block -- `evaluate`, `predict*`, `evaluate_cityscapes`, `calibrate_fp8`
        and `save` inside it work on the average -- and puts the raw weights back behind it, whatever the block raises.  Training inside
        the block raises.  Without an average the block runs on the weights as they are.'''
        return self.engine.averaged_weights()

    def calibrate_fp8(self, data_generator, num_batches):
        '''Not in the reference: switch the engine to the inference-only 'fp8_infer' precision and calibrate its static per-layer activation
        scales over `num_batches` batches of `data_generator` (the images of each batch; the first batch starts a new calibration).  After it,
        `predict`, `predict_and_save`, `predict_and_export_label_ids`, `evaluate` and the multi-scale / flip keywords run in FP8; `save`
        stores the calibration.  Returns it (float32[14], the max |input| of conv1_2 .. conv5_3, fc6, fc7).'''
        if num_batches < 1:
            raise ValueError("`num_batches` must be at least 1.")
        self.engine.set_precision('fp8_infer')
        cal = None
        for i in range(num_batches):
            batch = next(data_generator)
            cal = self.engine.calibrate_fp8(batch[0], reset=(i == 0))
        return cal

    def evaluate(self, data_generator, num_batches, metrics={'loss', 'mean_iou', 'accuracy'}, l2_regularization=0.0, dataset='val'):
        '''fcn8s_tensorflow.py:699-741'''
        _check_metric_names(metrics)
        if dataset not in ('train', 'val'):
            raise ValueError("`dataset` must be either 'train' or 'val'.")
        self._initialize_metrics(metrics)
        self._evaluate(data_generator, metrics, num_batches, l2_regularization, description='Running evaluation')
        self.eval_dataset = dataset

    def predict(self, images, argmax=True, scales=None, flip=False, crf=None, temperature=None, min_region=None, region_connectivity=4,
                region_rounds=1):
        '''fcn8s_tensorflow.py:743-770.  `images`: array-like of rank 4 (a list of HWC arrays works).
        Returns int64 class ids (N,H,W) or the float32 softmax (N,H,W,C).
        Not in the reference: `scales` (1 to 8 factors in (0, 4]) and / or `flip` average the softmax over resized and mirrored passes
        (multi-scale / flip test-time augmentation, see tta.py) and take images of any size; `scales=(1.0,)` alone predicts an image of
        any size at its own resolution.  Without them, height and width must be multiples of 32, as in the reference.
        `crf` (also not in the reference): refine the (mean) softmax by a mean-field CRF over a local window whose pairwise term reads
        the colours of the uint8 input (crf.py; fcn8s_predict_crf) -- True for the default parameters, a dict of fields or a crf.Params to
        override them, None / False for no CRF.  Images of any size, as with `scales=(1.0,)`.
        `temperature` (also not in the reference): with `argmax=False`, the returned distribution calibrated at that temperature
        (temperature.py; one `fcn8s_op_temperature_apply` on the result, whichever route made it) -- `fit_temperature` finds the value and
        keeps it in `self.temperature`.  None or 1.0, or `argmax=True` (the map cannot change an argmax): nothing is launched.
        `min_region` (also not in the reference): connected-region cleanup of the argmax map (regions.py; `fcn8s_op_regions_clean`) --
        every connected component (`region_connectivity` 4 or 8) of fewer pixels than the threshold takes the class of its largest
        4-adjacent neighbour that is not small itself, `region_rounds` (1..8) times.  An int, a sequence of one int per class or a dict
        {class: area} (0 = that class is never merged away); None / 0 / False: nothing is launched.  On every route the cleanup acts on
        the argmax where it lies on the device, before any download (host images are uploaded once for that).  Needs `argmax=True`.'''
        if isinstance(images, (list, tuple)):
            images = np.asarray(images)
        if temperature is not None:
            temperature = ts_mod.validate_temperature(temperature)
        table = regions_mod.resolve(min_region, self.num_classes)
        if table is not None:
            if not argmax:
                raise ValueError("`min_region` cleans the argmax map; a cleaned softmax is not defined: needs argmax=True.")
            regions_mod._check(region_connectivity, region_rounds)
            torch = self.engine.torch
            on_host = not (isinstance(images, torch.Tensor) and images.is_cuda)
            if on_host:
                images = self.engine._images(images, force_device=True)[0]
            out = self.predict(images, argmax=True, scales=scales, flip=flip, crf=crf)
            self.engine.regions_clean(out, table, connectivity=region_connectivity, rounds=region_rounds)
            return out.cpu().numpy() if on_host else out
        params = crf_mod.resolve(crf)
        if params is not None:
            out = self.engine.predict_crf(images, params, scales=(1.0,) if scales is None else scales, flip=flip, argmax=argmax)
        elif scales is None and not flip:
            out = self.engine.predict(images, argmax=argmax)
        else:
            out = self.engine.predict_tta(images, scales=(1.0,) if scales is None else scales, flip=flip, argmax=argmax)
        if argmax or temperature is None or temperature == 1.0:
            return out
        return self.engine.temperature_apply(out, temperature, out=out)[0]

    def predict_uncertainty(self, images, samples=20, keep_prob=0.5, argmax=True, sample_offset=0):
        '''Not in the reference: Monte-Carlo dropout inference (mc_dropout.py; fcn8s_predict_mc).  Dropout stays on behind fc6 and fc7,
        `samples` stochastic passes are drawn -- the VGG trunk runs once, fc6 -> fc7 -> decoder once per sample -- and their softmaxes are
        averaged.  Returns (prediction, entropy, mutual_information): int64 class ids (N,H,W) of the mean softmax or (argmax=False) the
        mean softmax (N,H,W,C); the predictive entropy of the mean and the mutual information between prediction and weights, float32
        (N,H,W), in nats.  `sample_offset` moves the call to other masks (sample s uses the streams of index sample_offset + s); two
        identical calls return identical bits.  Images of any size.  Works inside `averaged_weights()`.'''
        if isinstance(images, (list, tuple)):
            images = np.asarray(images)
        return self.engine.predict_mc(images, samples=samples, keep_prob=keep_prob, sample_offset=sample_offset, argmax=argmax,
                                      entropy=True, mutual_information=True)

    def predict_and_save(self,
                         results_dir,
                         images_dir,
                         color_map,
                         resize=False,
                         image_file_extension='png',
                         include_unprocessed_image=False,
                         arrangement='vertical',
                         overwrite_existing=True,
                         scales=None,
                         flip=False,
                         crf=None,
                         min_region=None,
                         region_connectivity=4,
                         region_rounds=1):
        '''fcn8s_tensorflow.py:772-855 (PIL instead of scipy.misc / helpers.visualization_utils).  `scales` / `flip` / `crf`: as in `predict`
        (images of any size; `resize` is then optional).  `min_region` / `region_connectivity` / `region_rounds`: as in `predict`; the
        overlay then shows the cleaned argmax map.'''
        regions = None
        if regions_mod.resolve(min_region, self.num_classes) is not None:
            regions = dict(min_region=min_region, region_connectivity=region_connectivity, region_rounds=region_rounds)

        if overwrite_existing and os.path.exists(results_dir):
            shutil.rmtree(results_dir)
        os.makedirs(results_dir)

        image_paths = glob(os.path.join(images_dir, '*.' + image_file_extension))
        num_images = len(image_paths)

        print('The segmented images will be saved to "{}"'.format(results_dir))

        tr = trange(num_images, file=sys.stdout)
        tr.set_description('Processing images')

        with sweeps.frozen(self.engine):
            for i in tr:
                self._segment_file(image_paths[i], results_dir, color_map, resize, include_unprocessed_image, arrangement, scales, flip, crf, regions)

    def predict_and_export_label_ids(self, results_dir, images_dir, resize=False, image_file_extension='png', overwrite_existing=True,
                                     scales=None, flip=False, crf=None, min_region=None, region_connectivity=4, region_rounds=1):
        '''Not in the reference: runs every `*.png` below `images_dir` (sub-directories = cities, as in leftImg8bit/val) through the
        model and writes the argmax as single-channel label-id PNGs under the same file names into `results_dir` -- the input of the
        official scorer (cityscapesscripts/evaluation/evalPixelLevelSemanticLabeling.py:72-106, 553-555; cityscapes_eval.evaluate_directory
        here).  Predictions are train ids 0..19 (0 = void) mapped through labels.py:188-192; `resize=(h, w)` feeds the network a
        resized image and writes the prediction back at the file's own size (nearest neighbour).  `scales` / `flip` / `crf`: as in `predict`
        (multi-scale / flip averaging on images of any size; `resize` is then optional).  `min_region` / `region_connectivity` /
        `region_rounds`: as in `predict` -- the train-id map is cleaned on the device before it is downloaded and mapped.'''
        from PIL import Image
        from . import cityscapes_eval as ce
        if self.num_classes != 20:
            raise ValueError("label-id export uses the 20 Cityscapes train ids; this model has {} classes.".format(self.num_classes))
        if overwrite_existing and os.path.exists(results_dir):
            shutil.rmtree(results_dir)
        os.makedirs(results_dir, exist_ok=True)
        paths = sweeps.image_files(images_dir, image_file_extension, allow_none=True)
        tr = trange(len(paths), file=sys.stdout)
        tr.set_description('Exporting label ids')
        with sweeps.frozen(self.engine):
            for i in tr:
                image, size = sweeps.load_image(paths[i], resize, 'cpu')        # a host image: the call uploads it and downloads the ids
                pred = np.asarray(self.predict(image, argmax=True, scales=scales, flip=flip, crf=crf, min_region=min_region,
                                               region_connectivity=region_connectivity, region_rounds=region_rounds))[0]
                ids = Image.fromarray(ce.TRAINIDS_TO_IDS_ARRAY[pred])
                if ids.size != size:
                    ids = ids.resize(size, Image.NEAREST)
                ids.save(os.path.join(results_dir, os.path.basename(paths[i])))
        return len(paths)

    def evaluate_cityscapes(self, images_dir, ground_truth_search, resize=False, image_file_extension='png', scales=None, flip=False, crf=None,
                            instance_level=True, json_path=None, boundary_radius=None, min_region=None, region_connectivity=4, region_rounds=1,
                            panoptic=None):
        '''Not in the reference: the official Cityscapes pixel-level table (IoU and iIoU, for classes and for categories) of this model in
        one call, scored where the predictions already are.  Every ground-truth file of the glob `ground_truth_search` (the official one is
        `<cityscapes>/gtFine/val/*/*_gtFine_labelIds.png`) is paired with its image `<city>_<seq>_<frame>*.<ext>` below `images_dir`; per
        image: decode, one upload, `predict` with `scales` / `flip` / `crf` on the device, upload of the label-id (and, with
        `instance_level`, the `*_instanceIds.png`) map, one `fcn8s_op_cityscapes_pair` call that consumes the int64 argmax as it is.  The
        prediction never visits the host and no file is written -- except with `resize=(h, w)`, where it comes back to the file's own size by
        PIL's nearest neighbour exactly as `predict_and_export_label_ids` writes it.  Returns the dict of
        `cityscapes_eval.evaluate_directory(..., instance_level=...)` -- which it equals exactly when that is run on the export of
        `predict_and_export_label_ids` with the same arguments; `json_path`: also write it in the evaluator's result-file layout
        (instance-level only).  `boundary_radius=R` (1..16): one more call per image, `fcn8s_op_boundary_pair`, on the prediction and the
        label map that are already on the device, and the trimap IoU for the band widths 1..R around the ground-truth boundaries and the
        boundary F-score for the tolerances 0..R in the result (`cityscapes_eval.trimap_scores`, `boundary_f_scores`): what `scales`,
        `flip` or `crf` change at the contours.  With None nothing more is launched and the dict is the one described above.
        `min_region` / `region_connectivity` / `region_rounds`: as in `predict` -- the argmax is cleaned on the device
        (`fcn8s_op_regions_clean`) before the counting calls see it: every speck it removes is a closed contour without a match in the
        ground truth.  With None nothing more is launched and the dict is the same, key for key.
        `panoptic=4` or `8` (needs `instance_level`): panoptic quality as well (panoptic.py; PQ = SQ x RQ, Kirillov et al., CVPR 2019) -- per
        image one `fcn8s_op_regions_label` and one `fcn8s_op_panoptic_pair` call on the argmax (after any `min_region` cleanup) and the
        instance map that are already on the device; the `panoptic*` keys of the result.  The predicted things are split into connected
        components of that connectivity, the naive way to turn a semantic map into instances: touching cars are one segment, so PQ of the
        things measures the semantic model plus that rule; PQ of the stuff classes and the fp counts -- the specks -- are the figures this
        is for.  With None nothing more is launched or allocated and the dict is the same, key for key.'''
        from PIL import Image
        import torch
        from . import cityscapes_eval as ce
        if self.num_classes != 20:
            raise ValueError("the Cityscapes evaluation uses the 20 Cityscapes train ids; this model has {} classes.".format(self.num_classes))
        if json_path is not None and not instance_level:
            raise ValueError("`json_path` writes the evaluator's result file, which holds the instance-level scores: needs instance_level=True.")
        gts, paths = sweeps.paired_files(images_dir, ground_truth_search, image_file_extension)
        dev = self.engine.device
        ev = ce.PixelLevelEvaluator(instance_level=instance_level, boundary_radius=boundary_radius, panoptic=panoptic)
        pixels = 0
        tr = trange(len(gts), file=sys.stdout)
        tr.set_description('Evaluating')
        with sweeps.frozen(self.engine):
            for i in tr:
                image, size = sweeps.load_image(paths[i], resize, dev)
                pred = self.predict(image, argmax=True, scales=scales, flip=flip, crf=crf, min_region=min_region,
                                    region_connectivity=region_connectivity, region_rounds=region_rounds)[0]       # int64 train ids, on the device
                train_ids = True
                if (pred.shape[1], pred.shape[0]) != size:
                    ids = Image.fromarray(ce.TRAINIDS_TO_IDS_ARRAY[pred.cpu().numpy()]).resize(size, Image.NEAREST)
                    pred = torch.from_numpy(np.array(ids)).to(dev); train_ids = False
                gt = np.array(Image.open(gts[i]))
                sweeps.check_label_map(gt, pred.shape, paths[i], gts[i])
                inst = None
                if instance_level:
                    inf = ce.instance_file_of(gts[i])
                    if inf == gts[i] or not os.path.isfile(inf):
                        raise ValueError("Unable to load " + inf)
                    inst = np.array(Image.open(inf))
                    if inst.shape != gt.shape:
                        raise ValueError("Image sizes of " + inf + " and " + gts[i] + " are not equal.")
                    inst = ce.instance_map_tensor(inst, dev)
                ev.add(pred, torch.from_numpy(gt.astype(np.uint8)).to(dev), inst, pred_is_train_ids=train_ids)
                pixels += gt.size
                if int(ev.conf.sum()) != pixels:
                    raise ValueError("Number of analyzed pixels and entries in confusion matrix disagree: contMatrix {}, pixels {}".format(int(ev.conf.sum()), pixels))
        res = ev.results()
        res["confMatrix"] = ev.conf
        res["nbPixels"] = pixels
        if json_path is not None:
            ce.write_result_json(res, json_path)
        return res

    def evaluate_reliability(self, images_dir, ground_truth_search, samples=None, keep_prob=0.5, sample_offset=0, scales=None, flip=False,
                             crf=None, bins=15, score_max=None, image_file_extension='png', json_path=None, temperature=None):
        '''Not in the reference: what this model's softmax and uncertainty maps are worth on a Cityscapes-style directory -- calibration
        (ECE, MCE, the reliability diagram, NLL, Brier score) and error detection (AUROC, AUPR, risk-coverage, AURC and E-AURC of
        "uncertainty predicts a wrong pixel") -- scored where the predictions already are (reliability.py; `fcn8s_op_reliability_pair`).
        Files are paired as in `evaluate_cityscapes`; per image: decode, one upload, the prediction on the device with `argmax=False`,
        upload of the label-id map, one op call.  The softmax never visits the host; the tables stay on the device and are downloaded
        once at the end.  Pixels whose label has train id 0 (void) are ignored, as in the official evaluation.  Routes:
        `samples=S`: `predict_uncertainty` (Monte-Carlo dropout at `keep_prob`, `sample_offset`); scores 'maxProb', 'entropy' and
        'mutualInformation'.  `samples=None` without `scales` / `flip` / `crf`: the same route with one sample and no dropout -- `predict`
        bit for bit, with the entropy map; scores 'maxProb' and 'entropy'.  With `scales` / `flip` / `crf`: `predict(argmax=False, ...)`,
        'maxProb' only; `samples` together with them raises ValueError (the Monte-Carlo route has no such passes).  `bins`: confidence
        bins of the calibration (1..64); `score_max`: the uncertainty that lands in the last of the 1024 histogram bins, default
        ln(num_classes).  Returns `reliability.Evaluator.results()` plus 'nbPixels' and 'route'; `json_path`: also write it
        (`reliability.write_result_json`).  Works inside `averaged_weights()`.
        `temperature=T`: score the distribution calibrated at T (`fit_temperature`) -- one `fcn8s_op_temperature_apply` per image, in place;
        on the single-pass route the 'entropy' score is the calibrated distribution's, from the same launch.  None or 1.0: nothing is
        launched.  Together with `samples=S` it raises ValueError: calibrating Monte-Carlo samples needs the temperature inside each
        sample's softmax, which `fcn8s_predict_mc` does not take.'''
        from PIL import Image
        import torch
        from . import reliability as rel
        route = sweeps.resolve_route(self, scales, flip, crf, temperature, samples, keep_prob, sample_offset, verb='score')
        if self.num_classes != 20:
            raise ValueError("the Cityscapes evaluation uses the 20 Cityscapes train ids; this model has {} classes.".format(self.num_classes))
        names = {'mc': ('entropy', 'mutualInformation'), 'single': ('entropy',), 'passes': ()}[route.name]
        ev = rel.Evaluator(bins=bins, num_classes=self.num_classes, lut=rel.cityscapes_lut(), score_names=names, score_max=score_max)
        gts, paths = sweeps.paired_files(images_dir, ground_truth_search, image_file_extension)
        dev = self.engine.device
        pixels = 0
        tr = trange(len(gts), file=sys.stdout)
        tr.set_description('Evaluating')
        with sweeps.frozen(self.engine):
            for i in tr:
                prob, *maps = route.softmax(sweeps.load_image(paths[i], False, dev)[0], entropy=True, mutual_information=True)
                gt = np.array(Image.open(gts[i]))
                sweeps.check_label_map(gt, prob.shape[1:3], paths[i], gts[i])
                ev.add(prob, torch.from_numpy(gt.astype(np.uint8)[None]).to(dev), tuple(maps[:len(names)]))
                pixels += gt.size
        res = ev.results()
        bad = res["tables"]["bad"]
        if bad.any():
            raise ValueError("{} pixels hold a train id outside 0..19 and {} a confidence or uncertainty that is not finite".format(int(bad[0]), int(bad[1])))
        res["nbPixels"] = pixels
        res["route"] = route.name
        if json_path is not None:
            rel.write_result_json(res, json_path)
        return res

    def fit_temperature(self, images_dir, ground_truth_search, scales=None, flip=False, crf=None, passes=2, candidates=32, t_min=0.125, t_max=8.0,
                        image_file_extension='png', json_path=None):
        '''Not in the reference: temperature scaling (Guo et al., ICML 2017; temperature.py), the remedy for what `evaluate_reliability`
        measures.  Fits the one scalar T that minimises the NLL of the calibrated distribution on a Cityscapes-style directory and keeps
        it in `self.temperature` (`save` stores it; `predict(..., temperature=model.temperature)` and
        `evaluate_reliability(..., temperature=...)` apply it).  Files are paired, the weights frozen and every image predicted on the
        device exactly as `evaluate_reliability` does on its single-pass route (no `scales` / `flip` / `crf`) or its passes route; per image
        one `fcn8s_op_temperature_nll` call evaluates all `candidates` (3..32) temperatures of the sweep's grid on the softmax where it is.
        `passes` sweeps over the files: the first grid is log-spaced over [t_min, t_max] and contains T = 1, each later one spans the two
        neighbours of the minimum (the NLL is convex in 1 / T).  K + 3 integers come back to the host per sweep.  Pixels whose label has
        train id 0 (void) are ignored.  Returns 'temperature', 'atBound' (the minimum is t_min or t_max: widen the range), 'nllBefore'
        (T = 1) and 'nllAfter' (means per counted pixel), 'candidates' (per sweep the list of (T, mean NLL)), 'pixels', 'nbPixels' and
        'route'; `json_path`: also write it.  Works inside `averaged_weights()`.'''
        from PIL import Image
        import torch
        from . import reliability as rel
        if self.num_classes != 20:
            raise ValueError("the Cityscapes evaluation uses the 20 Cityscapes train ids; this model has {} classes.".format(self.num_classes))
        ts_mod.validate_fit(passes, candidates, t_min, t_max)
        route = sweeps.resolve_route(self, scales, flip, crf)
        gts, paths = sweeps.paired_files(images_dir, ground_truth_search, image_file_extension)
        dev = self.engine.device
        lut = rel.cityscapes_lut()
        nb = [0]

        def sweep(betas):
            fitter = ts_mod.Fitter(betas, lut, num_classes=self.num_classes)
            nb[0] = 0
            tr = trange(len(gts), file=sys.stdout)
            tr.set_description('Fitting temperature')
            for i in tr:
                prob = route.softmax(sweeps.load_image(paths[i], False, dev)[0])[0]
                gt = np.array(Image.open(gts[i]))
                sweeps.check_label_map(gt, prob.shape[1:3], paths[i], gts[i])
                fitter.add(prob, torch.from_numpy(gt.astype(np.uint8)[None]).to(dev))
                nb[0] += gt.size
            return fitter.result()

        with sweeps.frozen(self.engine):
            res = ts_mod.fit(sweep, passes=passes, candidates=candidates, t_min=t_min, t_max=t_max)
        res["nbPixels"] = nb[0]
        res["route"] = route.name
        self.temperature = res["temperature"]
        if json_path is not None:
            ts_mod.write_result_json(res, json_path)
        return res

    def fit_pseudo_label_thresholds(self, images_dir, portion=0.2, t_min=0.0, t_max=None, scales=None, flip=False, crf=None, temperature=None,
                                    samples=None, keep_prob=0.5, mi_max=None, resize=False, image_file_extension='png', json_path=None):
        '''Not in the reference: the first sweep of class-balanced self-training (CBST, Zou et al., ECCV 2018; pseudo_label.py) -- one
        confidence threshold per class for pseudo-labelling the unlabelled (or coarsely labelled) images below `images_dir`, set where
        `portion` (a value in (0, 1], or one per class) of the pixels predicted as that class lies above it.  One global threshold gives
        every kept pixel to road, sky and building; a threshold per class keeps the same share of pole, rider and bicycle.
        Walks every `*.<ext>` below `images_dir` as `predict_and_export_label_ids` does; per image: decode, one upload, the prediction on the
        device with `argmax=False`, one `fcn8s_op_pseudo_label` call without labels that adds the maximum softmax probability of every pixel
        to its predicted class's histogram of 1024 bins.  The softmax never visits the host; the tables are downloaded once at the end.
        Routes and refusals as in `evaluate_reliability`: `samples=S` is the Monte-Carlo dropout mean at `keep_prob`, and `mi_max` then
        keeps out of the histograms the pixels whose mutual information exceeds it; otherwise `scales` / `flip` / `crf` / `temperature` as
        in `predict`.  `temperature` or `scales` / `flip` / `crf` together with `samples` raise ValueError.  `resize=(h, w)` feeds the
        network resized images.  Thresholds are bin edges j / 1024 clamped to [t_min, t_max] (`pseudo_label.thresholds_from_hist`), so that
        the export sweep keeps exactly the histogram's tail.  Returns dict(thresholds float32[C], bins int64[C], hist, counts, misc, summary,
        nbImages, route) and keeps the thresholds in `self.pseudo_label_thresholds`; they belong to this directory, not to the model:
        `save` does not store them.  `json_path`: also write the result.  Works inside `averaged_weights()`.'''
        pl_mod.validate(self.num_classes, portion=portion, t_min=t_min, t_max=t_max)
        route = sweeps.resolve_route(self, scales, flip, crf, temperature, samples, keep_prob, mi_max=mi_max)
        paths = sweeps.image_files(images_dir, image_file_extension)
        dev = self.engine.device
        tables = None
        tr = trange(len(paths), file=sys.stdout)
        tr.set_description('Fitting pseudo-label thresholds')
        with sweeps.frozen(self.engine):
            for i in tr:
                prob, _, score = route.softmax(sweeps.load_image(paths[i], resize, dev)[0], mutual_information=mi_max is not None)
                _, tables = self.engine.pseudo_label(prob, score=score, score_max=mi_max, labels=False, tables=tables)
        host = pl_mod.tables_to_host(tables, self.num_classes)
        thr, bins = pl_mod.thresholds_from_hist(host["hist"], portion, t_min=t_min, t_max=t_max)
        kept = pl_mod.tail_sums(host["hist"], bins)                     # what the export sweep keeps at these thresholds
        expected = np.stack([kept, host["counts"].sum(1) - kept], 1)
        res = dict(thresholds=thr, bins=bins, hist=host["hist"], counts=host["counts"], misc=host["misc"],
                   summary=pl_mod.summary(host["hist"], expected, host["misc"], thr), nbImages=len(paths), route=route.name)
        self.pseudo_label_thresholds = thr
        if json_path is not None:
            pl_mod.write_result_json(res, json_path)
        return res

    def predict_and_export_pseudo_labels(self, results_dir, images_dir, thresholds=None, ignore_id=255, id_space='train', base_search=None,
                                         base_fill=None, scales=None, flip=False, crf=None, temperature=None, samples=None, keep_prob=0.5,
                                         mi_max=None, resize=False, image_file_extension='png', overwrite_existing=True, json_path=None):
        '''Not in the reference: the second sweep of class-balanced self-training -- pseudo-label maps for every `*.<ext>` below `images_dir`,
        written as single-channel PNGs under the images' basenames into `results_dir`: the predicted class where its maximum softmax
        probability clears the class's threshold, `ignore_id` elsewhere.  A later `train()` reads them through the ordinary `BatchGenerator`;
        the loss ignores label ids >= num_classes, so no teacher is on the device and nothing changes in the step.
        `thresholds`: one per class; None takes `self.pseudo_label_thresholds` (`fit_pseudo_label_thresholds`) and raises when there are
        none.  `id_space='train'` writes train ids; 'label' writes Cityscapes label ids through `cityscapes_eval.TRAINIDS_TO_IDS_ARRAY`
        (20-class models only) -- `ignore_id` must then be an id that the `convert_ids_to_ids` table given to the `BatchGenerator` sends to a
        value >= num_classes, as it is written as it is.  `base_search` / `base_fill`: a glob of existing label maps (a coarse annotation)
        to complete; a map belongs to the image of the same `<city>_<seq>_<frame>` -- `evaluate_cityscapes`' naming rule in the other
        direction, its basename is `<city>_<seq>_<frame>_*` -- and a missing or a second partner raises ValueError.  Each map is uploaded;
        its pixels that differ from `base_fill` are written as they are, and only the others are predicted.  It has to have the size of the
        prediction, so `resize` with it raises.  Routes as in `fit_pseudo_label_thresholds`; with `samples` and `mi_max`, pixels whose mutual
        information exceeds `mi_max` are ignored.  Per image: decode, one upload, the prediction with `argmax=False` on the device, one
        `fcn8s_op_pseudo_label` call, and the download of the label map -- 1 byte per pixel, not the 4 C of the softmax.  `resize=(h, w)`
        behaves as in `predict_and_export_label_ids`: the labels come back to the file's size by PIL's nearest neighbour.  Returns
        `pseudo_label.summary` of the whole sweep plus 'thresholds', 'images' (per file: kept, dropped, badRows, passedThrough,
        droppedByScore), 'nbImages' and 'route'; `json_path`: also write it.
        Not done here: filling labels on the fly inside `train(teacher=...)`, iterating rounds with a growing portion (the caller loops over
        fit, export and train), spatial priors (CBST-SP), and any change to `BatchGenerator`.'''
        from PIL import Image
        import torch
        from . import cityscapes_eval as ce
        if thresholds is None:
            thresholds = self.pseudo_label_thresholds
            if thresholds is None:
                raise ValueError("no thresholds: pass `thresholds` or run `fit_pseudo_label_thresholds` first.")
        v = pl_mod.validate(self.num_classes, thresholds=thresholds, ignore_id=ignore_id, id_space=id_space, base_search=base_search, base_fill=base_fill,
                            resize=resize)
        route = sweeps.resolve_route(self, scales, flip, crf, temperature, samples, keep_prob, mi_max=mi_max)
        paths = sweeps.image_files(images_dir, image_file_extension)
        bases = None
        if base_search is not None:
            found = sorted(glob(base_search))
            bases = [pl_mod.find_base(p, found) for p in paths]
        if overwrite_existing and os.path.exists(results_dir):
            shutil.rmtree(results_dir)
        os.makedirs(results_dir, exist_ok=True)
        dev = self.engine.device
        Cn = self.num_classes
        thr = torch.from_numpy(v["thresholds"]).to(dev)
        oid = torch.from_numpy(ce.TRAINIDS_TO_IDS_ARRAY.astype(np.uint8)).to(dev) if id_space == 'label' else None
        flat = torch.zeros(2 * Cn + 3, dtype=torch.int64, device=dev)           # counts and misc in one piece: one small download per image
        tables = dict(hist=None, counts=flat[:2 * Cn].view(Cn, 2), misc=flat[2 * Cn:])
        seen = np.zeros(2 * Cn + 3, np.int64)
        images = []
        tr = trange(len(paths), file=sys.stdout)
        tr.set_description('Exporting pseudo-labels')
        with sweeps.frozen(self.engine):
            for i in tr:
                image, size = sweeps.load_image(paths[i], resize, dev)
                prob, _, score = route.softmax(image, mutual_information=mi_max is not None)
                base = None
                if bases is not None:
                    bm = np.array(Image.open(bases[i]))
                    if bm.ndim != 2 or bm.dtype != np.uint8:
                        raise ValueError("The base label map " + bases[i] + " is not a single-channel 8-bit image.")
                    if bm.shape != tuple(prob.shape[1:3]):
                        raise ValueError("Image sizes of " + paths[i] + " and " + bases[i] + " are not equal.")
                    base = torch.from_numpy(bm[None]).to(dev)
                labels, _ = self.engine.pseudo_label(prob, thresholds=thr, out_ids=oid, ignore_id=v["ignore_id"], base=base, base_fill=v["base_fill"],
                                                     score=score, score_max=mi_max, labels=True, tables=tables)
                out = Image.fromarray(labels[0].cpu().numpy())
                now = flat.cpu().numpy()
                d, seen = now - seen, now
                images.append(dict(file=os.path.basename(paths[i]), kept=int(d[0:2 * Cn:2].sum()), dropped=int(d[1:2 * Cn:2].sum()),
                                   badRows=int(d[2 * Cn]), passedThrough=int(d[2 * Cn + 1]), droppedByScore=int(d[2 * Cn + 2])))
                if out.size != size:
                    out = out.resize(size, Image.NEAREST)
                out.save(os.path.join(results_dir, os.path.basename(paths[i])))
        res = pl_mod.summary(None, seen[:2 * Cn].reshape(Cn, 2), seen[2 * Cn:], v["thresholds"])
        res.update(thresholds=v["thresholds"], images=images, nbImages=len(paths), route=route.name)
        if json_path is not None:
            pl_mod.write_result_json(res, json_path)
        return res

    def _instance_table(self, connectivity, min_instance_pixels, samples, keep_prob, scales, flip, crf, temperature, min_region, region_connectivity,
                        region_rounds):
        '''The arguments and the device path of the two instance-level sweeps: (route, table) where `table(image, inst, path)` takes a uint8
        device tensor (1,H,W,3) and the image's instance map (NumPy, or None) and returns (int32 components on the device, rows).'''
        if self.num_classes != 20:
            raise ValueError("the Cityscapes evaluation uses the 20 Cityscapes train ids; this model has {} classes.".format(self.num_classes))
        regions_mod._check(connectivity)
        if isinstance(min_instance_pixels, bool) or not isinstance(min_instance_pixels, (int, np.integer)) or min_instance_pixels < 0:
            raise ValueError("`min_instance_pixels` is a non-negative integer, not {!r}".format(min_instance_pixels))
        clean = regions_mod.resolve(min_region, self.num_classes)
        if clean is not None:
            regions_mod._check(region_connectivity, region_rounds)
        route = sweeps.resolve_route(self, scales, flip, crf, temperature, samples, keep_prob)

        def table(image, inst, path):
            prob = route.softmax(image)[0]
            labels, _t = self.engine.pseudo_label(prob, labels=True)            # zero thresholds, the identity table: the argmax as uint8
            if clean is not None:
                self.engine.regions_clean(labels, clean, connectivity=region_connectivity, rounds=region_rounds)
            comp, _area = self.engine.regions_label(labels, connectivity=connectivity, area=False)
            rows, bad = self.engine.instance_pair(prob, labels, comp, inst)
            if bad.any():
                raise ValueError("{}: {} pixels hold a label outside 0..19 and {} a probability outside [0, 1]".format(path, int(bad[0, 0]), int(bad[0, 1])))
            return comp, rows
        return route.name, table

    def evaluate_cityscapes_instances(self, images_dir, ground_truth_search, connectivity=4, min_instance_pixels=0, samples=None, keep_prob=0.5,
                                      scales=None, flip=False, crf=None, temperature=None, min_region=None, region_connectivity=4, region_rounds=1,
                                      image_file_extension='png', json_path=None):
        '''Not in the reference's model code: the official Cityscapes instance-level table (AP over the overlaps 0.5 .. 0.95 and AP50%, per
        thing class and on average; instances.py has the definition) of this model in one call, scored where the predictions already are.
        The predicted instances are the connected components (`connectivity` 4 or 8) of the thing classes of the argmax, and the confidence
        of an instance is the mean probability of the assigned class over its pixels -- so a calibrated `temperature`, the Monte-Carlo mean
        (`samples`, `keep_prob`), `scales` / `flip` averaging and the `crf`, which IoU and PQ cannot see where they do not move the argmax,
        show up here as a ranking of segments, and `min_region` cleanup as fewer of them.
        Every ground-truth file of the glob `ground_truth_search` (the official one is `<cityscapes>/gtFine/val/*/*_gtFine_instanceIds.png`)
        is paired with its image `<city>_<seq>_<frame>*.<ext>` below `images_dir` as in `evaluate_cityscapes`; per image: decode, one upload,
        the softmax on the device through `evaluate_reliability`'s routes (and its refusals), one `fcn8s_op_pseudo_label` call for the uint8
        argmax, an optional `fcn8s_op_regions_clean`, one `fcn8s_op_regions_label` and one `fcn8s_op_instance_pair` call against the uploaded
        instance map.  The softmax never visits the host; a few hundred table rows per image do.  `min_instance_pixels`: predicted instances
        of fewer pixels are dropped on the host before the matching.  Returns `instances.results(...)` plus 'nbPixels', 'route' and
        'connectivity'; `json_path`: also write it in the layout of resultInstanceLevelSemanticLabeling.json.  Works inside
        `averaged_weights()`.
        Caveat: connected components merge touching cars, so this AP measures the semantic model plus that rule -- a baseline and a speck
        detector, not an instance-segmentation method.'''
        from PIL import Image
        from . import instances as ins
        route, table = self._instance_table(connectivity, min_instance_pixels, samples, keep_prob, scales, flip, crf, temperature, min_region,
                                            region_connectivity, region_rounds)
        gts, paths = sweeps.paired_files(images_dir, ground_truth_search, image_file_extension)
        stats = ins.new_stats()
        pixels = 0
        tr = trange(len(gts), file=sys.stdout)
        tr.set_description('Evaluating')
        with sweeps.frozen(self.engine):
            for i in tr:
                image = sweeps.load_image(paths[i], False, self.engine.device)[0]
                inst = np.array(Image.open(gts[i]))
                if inst.ndim != 2 or inst.shape != tuple(image.shape[1:3]):
                    raise ValueError("Image sizes of " + paths[i] + " and " + gts[i] + " are not equal.")
                _comp, rows = table(image, inst[None], paths[i])
                ins.stats_add(stats, rows[0], min_instance_pixels)
                pixels += inst.size
        res = ins.results(stats)
        res["nbPixels"] = pixels
        res["route"] = route
        res["connectivity"] = int(connectivity)
        if json_path is not None:
            ins.write_result_json(res, json_path)
        return res

    def predict_and_export_instances(self, results_dir, images_dir, connectivity=4, min_instance_pixels=0, samples=None, keep_prob=0.5, scales=None,
                                     flip=False, crf=None, temperature=None, min_region=None, region_connectivity=4, region_rounds=1,
                                     image_file_extension='png', overwrite_existing=True):
        '''Not in the reference's model code: the predictions of `evaluate_cityscapes_instances` for every `*.<ext>` below `images_dir`,
        written into `results_dir` in the official instance-level result format (`instances.write_export`): per image `<basename>.txt` with
        one line `<relative mask path> <label id> <confidence>` per instance and one binary mask PNG per instance.  The same device path
        without ground truth; the component map (4 bytes per pixel) and the table rows are downloaded, the softmax is not.
        `instances.evaluate_directory` on this export gives the dict of `evaluate_cityscapes_instances` with the same arguments.  Returns
        dict(files = the text files in image order, nbImages, nbInstances, route).'''
        from . import instances as ins
        route, table = self._instance_table(connectivity, min_instance_pixels, samples, keep_prob, scales, flip, crf, temperature, min_region,
                                            region_connectivity, region_rounds)
        paths = sweeps.image_files(images_dir, image_file_extension)
        if overwrite_existing and os.path.exists(results_dir):
            shutil.rmtree(results_dir)
        os.makedirs(results_dir, exist_ok=True)
        files, count = [], 0
        tr = trange(len(paths), file=sys.stdout)
        tr.set_description('Exporting instances')
        with sweeps.frozen(self.engine):
            for i in tr:
                comp, rows = table(sweeps.load_image(paths[i], False, self.engine.device)[0], None, paths[i])
                files.append(ins.write_export(results_dir, os.path.splitext(os.path.basename(paths[i]))[0], comp[0].cpu().numpy(), rows[0], min_instance_pixels))
                with open(files[-1]) as f:
                    count += sum(1 for _line in f)
        return dict(files=files, nbImages=len(paths), nbInstances=count, route=route)

    def _segment_file(self, filepath, results_dir, color_map, resize, include_unprocessed_image, arrangement, scales=None, flip=False, crf=None,
                      regions=None):
        '''Loop body of predict_and_save (fcn8s_tensorflow.py:829-855).'''
        from PIL import Image
        image = sweeps.load_image(filepath, resize, 'cpu')[0][0].numpy()
        img_height, img_width, img_ch = image.shape

        if regions is None:
            prediction = self.predict([image], argmax=False, scales=scales, flip=flip, crf=crf)
        else:                                   # the cleaned argmax map, one-hot: the overlay takes its argmax
            prediction = np.eye(self.num_classes, dtype=np.float32)[self.predict([image], argmax=True, scales=scales, flip=flip, crf=crf, **regions)]
        processed = print_segmentation_onto_image(image=image, prediction=prediction, color_map=color_map)

        if include_unprocessed_image:
            pil = Image.fromarray(image)
            if arrangement == 'vertical':
                canvas = Image.new('RGB', (img_width, 2 * img_height))
                canvas.paste(processed, (0, 0)); canvas.paste(pil, (0, img_height))
            else:
                canvas = Image.new('RGB', (2 * img_width, img_height))
                canvas.paste(processed, (0, 0)); canvas.paste(pil, (img_width, 0))
            processed = canvas

        processed.save(os.path.join(results_dir, os.path.basename(filepath)))

    def save(self,
             model_save_dir,
             saver,
             tags=['default'],
             name=None,
             include_global_step=True,
             include_last_training_loss=True,
             include_metrics=True,
             force_save=False):
        '''fcn8s_tensorflow.py:857-936: same guard, same validation, same directory name.'''
        if (not self.variables_updated) and (not force_save):
            print("Abort: Nothing to save, no training has been performed since the model was last saved.")
            return

        if not saver in _SAVERS:
            raise ValueError("Unexpected value for `saver`: Can be either 'saved_model' or 'train_saver', but received '{}'.".format(saver))

        if self.training_loss is None:
            include_last_training_loss = False

        model_name = 'saved_model'
        if not name is None:
            model_name += '_' + name
        if include_global_step:
            self.g_step = self.engine.global_step
            model_name += '_(globalstep-{})'.format(self.g_step)
        if include_last_training_loss:
            model_name += '_(trainloss-{:.4f})'.format(self.training_loss)
        if include_metrics:
            if self.eval_dataset == 'val':
                model_name += '_(eval_on_val_dataset)'
            else:
                model_name += '_(eval_on_train_dataset)'
            for i in range(len(self.metric_names)):
                model_name += '_({}-{:.4f})'.format(self.metric_names[i], self.metric_values[i])
        if not (include_global_step or include_last_training_loss or include_metrics) and (name is None):
            model_name += '_{}'.format(time.time())

        if self.engine.rank == 0:
            target = os.path.join(model_save_dir, model_name)
            if saver == 'saved_model':
                if os.path.exists(target):
                    raise AssertionError("Export directory already exists. Please specify a different export directory: {}".format(target))
                os.makedirs(os.path.join(target, 'variables'))
                _save_checkpoint(self.engine, os.path.join(target, 'variables', 'variables.npz'))
                _write_meta(target, self.engine, tags, self.temperature)
            else:
                os.makedirs(target, exist_ok=True)
                _save_checkpoint(self.engine, os.path.join(target, 'variables.npz'))
                _write_meta(target, self.engine, tags, self.temperature)      # (the reference builds a fresh Saver per save() call, :927-934, so its
                                                            #  max_to_keep=5 never deletes an earlier checkpoint: nothing is pruned here either)
        self.last_saved_model_name = model_name

        self.variables_updated = False

    def load_variables(self, path):
        '''fcn8s_tensorflow.py:938-944.  `path` is the prefix `<dir>/<model_name>/variables`
        (as passed to tf.train.Saver.restore) or the `.npz` file itself.'''
        if os.path.isfile(path + '.index'):          # a tf.train.Saver checkpoint written by the reference
            _load_tf_tensors(self.engine, tf_bundle.read_bundle(path), with_state=True)
            return
        f = path if path.endswith('.npz') else path + '.npz'
        if not os.path.isfile(f):
            raise ValueError("The passed save_path is not a valid checkpoint: {}".format(path))
        _load_checkpoint(self.engine, f, with_state=True)

    def export_tf_variables(self, prefix, include_optimizer_state=True):
        '''Not in the reference: writes all variables (and the Adam slots / global_step under the names
        tf.train.AdamOptimizer(name='adam_optimizer') gives them) as a TensorFlow tensor bundle
        `<prefix>.index` + `<prefix>.data-00000-of-00001`, restorable with tf.train.Saver.  A parameter average (train's `ema_decay`)
        is written as `<variable>/ExponentialMovingAverage`, the shadow variables of tf.train.ExponentialMovingAverage.'''
        tensors = dict(self.engine.get_params())
        if include_optimizer_state:
            m, v = self.engine.get_opt_state()
            for k, (shape, off) in self.engine.specs.items():
                n = int(np.prod(shape))
                tensors[k + tf_bundle.ADAM_M_SUFFIX] = self.engine.unpad(k, m[off:off + n].reshape(shape))
                tensors[k + tf_bundle.ADAM_V_SUFFIX] = self.engine.unpad(k, v[off:off + n].reshape(shape))
            step = self.engine.global_step
            tensors['optimizer/global_step'] = np.asarray(step, dtype=np.int32)
            # AdamOptimizer's non-slot variables (initialised to beta, multiplied by beta in every apply): a Saver over all
            # saveable variables (load_variables, :943) would not restore without them
            tensors['optimizer/beta1_power'] = np.asarray(0.9 ** (step + 1), dtype=np.float32)
            tensors['optimizer/beta2_power'] = np.asarray(0.999 ** (step + 1), dtype=np.float32)
        info = self.engine.ema_info()
        if info['has_shadow'] and not info['swapped']:      # the names tf.train.ExponentialMovingAverage.average_name gives its shadow variables
            sh = self.engine.get_ema()
            for k, (shape, off) in self.engine.specs.items():
                tensors[k + tf_bundle.EMA_SUFFIX] = self.engine.unpad(k, sh[off:off + int(np.prod(shape))].reshape(shape))
        tf_bundle.write_bundle(prefix, tensors)

    def close(self):
        '''fcn8s_tensorflow.py:946-952'''
        self.engine.close()
        print("The session has been closed.")


# ---------------------------------------------------------------------------------------------
# checkpoint format: variables by reference name + Adam slots + global_step
# ---------------------------------------------------------------------------------------------
def _save_checkpoint(engine, path):
    arrays = dict(engine.get_params())
    m, v = engine.get_opt_state()
    arrays['__adam_m__'] = m
    arrays['__adam_v__'] = v
    arrays['optimizer/global_step'] = np.asarray(engine.global_step, dtype=np.int64)
    info = engine.ema_info()
    if info['has_shadow'] and not info['swapped']:      # (inside averaged_weights() the variables ARE the average: a checkpoint to serve, without a shadow)
        arrays['__ema__'] = engine.get_ema()
    tmp = path + '.tmp.npz'
    np.savez(tmp, **arrays)
    os.replace(tmp, path)


def _load_checkpoint(engine, path, with_state=True):
    data = np.load(path)
    engine.set_params({k: data[k] for k in data.files if k in engine.specs})
    if with_state:
        if '__adam_m__' in data.files:
            engine.set_opt_state(data['__adam_m__'], data['__adam_v__'])
        if 'optimizer/global_step' in data.files:
            engine.global_step = int(data['optimizer/global_step'])
        if '__ema__' in data.files:
            engine.set_ema_state(data['__ema__'])


def _load_tf_tensors(engine, tensors, with_state=True):
    engine.set_params({k: v for k, v in tensors.items() if k in engine.specs})
    if not with_state:
        return
    n = engine.flat_params.numel()
    m = np.zeros(n, np.float32); v = np.zeros(n, np.float32); found = False
    for k, (shape, off) in engine.specs.items():
        cnt = int(np.prod(shape))
        if k + tf_bundle.ADAM_M_SUFFIX in tensors and k + tf_bundle.ADAM_V_SUFFIX in tensors:
            m[off:off + cnt] = engine.pad(k, tensors[k + tf_bundle.ADAM_M_SUFFIX], slot=True).reshape(-1)
            v[off:off + cnt] = engine.pad(k, tensors[k + tf_bundle.ADAM_V_SUFFIX], slot=True).reshape(-1)
            found = True
    if found:
        engine.set_opt_state(m, v)
    if any(k + tf_bundle.EMA_SUFFIX in tensors for k in engine.specs):      # tf.train.ExponentialMovingAverage's shadow variables
        s = engine.flat_params.detach().cpu().numpy().copy()                # (a variable without one keeps s = theta)
        for k, (shape, off) in engine.specs.items():
            if k + tf_bundle.EMA_SUFFIX in tensors:
                s[off:off + int(np.prod(shape))] = engine.pad(k, tensors[k + tf_bundle.EMA_SUFFIX]).reshape(-1)
        engine.set_ema_state(s)
    for key in ('optimizer/global_step', 'global_step'):
        if key in tensors:
            engine.global_step = int(np.asarray(tensors[key]).reshape(-1)[0])
            break


def _write_meta(target, engine, tags, temperature=None):
    meta = {'format': 'fcn8s_tensorflow_amd/1', 'num_classes': engine.logical_classes, 'widths': list(engine.widths),
            'fc6_ksize': engine.specs['fc6/weights'][0][0], 'tags': list(tags) if tags else None,
            'global_step': engine.global_step}
    info = engine.ema_info()
    if info['decay'] > 0:                 # the parameter average's setting (the shadow itself: '__ema__' of the checkpoint)
        meta['ema_decay'] = info['decay']
        meta['ema_warmup'] = info['warmup']
    cal = engine.fp8_calibration()
    if cal is not None:                   # the 'fp8_infer' calibration (float32 values, stored exactly as Python floats)
        meta['fp8_calibration'] = [float(v) for v in cal]
    if temperature is not None:           # the fitted temperature of fit_temperature
        meta['temperature'] = float(temperature)
    with open(os.path.join(target, 'fcn8s_meta.json'), 'w') as f:
        json.dump(meta, f)


def _read_meta(model_dir):
    f = os.path.join(model_dir, 'fcn8s_meta.json')
    if not os.path.isfile(f):
        if os.path.isfile(os.path.join(model_dir, 'saved_model.pb')):
            raise NotImplementedError("'{}' is a TensorFlow SavedModel; it cannot be loaded without TensorFlow.".format(model_dir))
        raise IOError("SavedModel file does not exist at: {}".format(model_dir))
    with open(f) as fh:
        return json.load(fh)


class _Unlabeled:
    """The state of train()'s self-training route for one call (FCN8s._resolve_unlabeled)."""

    def __init__(self, **kw):
        self.pixels = 0
        self.entropy = None          # train(entropy_images='unlabeled'): the term's weight and pixel set, set per joined batch
        self.fda_base = None         # train(fda_beta=...): int32 0 .. N - 1 on the device, made at the first joined batch
        self.__dict__.update(kw)


class _Feeder:
    """Pulls exactly `count` batches from a generator on a helper thread, one batch ahead of the consumer, and -- when the batch is
    (uint8 images, uint8 class ids) -- already starts its host-to-device copy through a staging slot (Engine.stage), so that PNG
    decoding, the pinned-memory copy and the DMA of batch k+1 overlap the GPU work of step k.  The reference pulls and feeds
    serially inside the step loop (fcn8s_tensorflow.py:551-572).  Generators made by this package's BatchGenerator offer
    `next_ids()` (the same batch with class ids instead of the 20x larger one-hot rows); any other generator is consumed through
    next() and its arrays are fed as they are.  Exactly `count` batches are consumed, as in the reference's loops."""

    def __init__(self, engine, generator, count, stage=True):
        import queue
        import threading
        self.q = queue.Queue(maxsize=1)
        self.err = None
        self.stop = threading.Event()

        def put(item):
            while not self.stop.is_set():
                try:
                    self.q.put(item, timeout=0.05)
                    return True
                except queue.Full:
                    pass
            return False

        def work():
            try:
                pull = getattr(generator, 'next_ids', None)
                for i in range(count):
                    if self.stop.is_set():
                        return
                    images, labels = pull() if pull is not None else next(generator)
                    if (stage and isinstance(images, np.ndarray) and images.dtype == np.uint8 and isinstance(labels, np.ndarray)
                            and labels.dtype == np.uint8 and labels.ndim == 3 and images.ndim == 4):
                        item = (engine.stage(images, labels, slot=i % L.NUM_STAGE_SLOTS), None)
                    else:
                        item = (images, labels)
                    if not put(item):
                        return
            except BaseException as e:          # surfaces in the consumer
                self.err = e
                put(None)

        self.t = threading.Thread(target=work, daemon=True)
        self.t.start()

    def next(self):
        item = self.q.get()
        if item is None:
            raise self.err
        return item

    def close(self):
        """Stops the helper thread and waits for it: after a step raised (or Ctrl-C) it must not keep pulling batches from the
        user's generator, nor sit inside fcn8s_stage_inputs while the model is being closed."""
        import queue
        self.stop.set()
        try:
            while True:
                self.q.get_nowait()
        except queue.Empty:
            pass
        self.t.join()


class _ScalarLog:
    """One of the reference's two tf.summary.FileWriters (fcn8s_tensorflow.py:531-535): a TensorBoard event file
    (`events.out.tfevents.*`, tf_events.py) in `logdir`, plus the same scalars as JSON lines (`scalars.jsonl`) for reading without
    TensorBoard.  With an engine, every record also carries what `_build_summary_ops` (:331-350) attaches to the ten watched
    weight / bias pairs: mean, stddev, max, min and a histogram (helpers/tf_variable_summaries.py:3-20), computed on the GPU."""

    def __init__(self, logdir, engine=None):
        from .tf_events import EventFileWriter
        os.makedirs(logdir, exist_ok=True)
        self.path = os.path.join(logdir, 'scalars.jsonl')
        self.events = EventFileWriter(logdir)
        self.engine = engine

    def add(self, step, **scalars):
        from . import tf_events
        with open(self.path, 'a') as f:
            f.write(json.dumps(dict(step=int(step), **{k: float(v) for k, v in scalars.items()})) + '\n')
        summary = b''
        if self.engine is not None:
            for name, scope in tf_events.WATCHED_VARIABLES:
                if name in self.engine.specs:
                    summary += tf_events.add_variable_summaries(self.engine.logical_param_view(name), scope)
        summary += b''.join(tf_events.scalar_value(k, v) for k, v in scalars.items())
        self.events.add_summary(summary, int(step))

    def close(self):
        self.events.close()


def create_video_from_images(video_output_name, image_input_dir, frame_rate=30.0, image_file_extension='png'):
    '''helpers/visualization_utils.py:102-120: a video from the images of a directory (sorted by name).  The reference encodes
    MP4 through moviepy (ffmpeg); when moviepy is importable that is what happens here, otherwise -- this image has neither moviepy
    nor ffmpeg -- the frames are written as Motion-JPEG into an AVI container (`<video_output_name>.avi`, plays everywhere, no
    dependencies beyond Pillow).  Returns the path written.'''
    image_paths = sorted(glob(os.path.join(image_input_dir, '*.' + image_file_extension)))
    if not image_paths:
        raise ValueError("no '*.{}' images in {}".format(image_file_extension, image_input_dir))
    try:
        from moviepy.editor import ImageSequenceClip
    except ImportError:
        ImageSequenceClip = None
    if ImageSequenceClip is not None:
        out = "{}.mp4".format(video_output_name)
        ImageSequenceClip(image_paths, fps=frame_rate).write_videofile(out)
        return out
    return _write_mjpeg_avi("{}.avi".format(video_output_name), image_paths, frame_rate)


def _write_mjpeg_avi(path, image_paths, frame_rate, quality=90):
    '''RIFF/AVI 1.0 with one MJPG video stream: hdrl (avih + strl(strh, strf)), movi (one '00dc' chunk per JPEG frame), idx1.'''
    import io
    import struct
    from PIL import Image
    frames, size = [], None
    for p in image_paths:
        im = Image.open(p).convert('RGB')
        if size is None:
            size = im.size
        elif im.size != size:
            im = im.resize(size)
        buf = io.BytesIO()
        im.save(buf, format='JPEG', quality=quality)
        frames.append(buf.getvalue())
    w, h = size
    n = len(frames)
    usec = int(round(1e6 / float(frame_rate)))
    rate, scale = int(round(float(frame_rate) * 1000)), 1000
    maxb = max(len(f) for f in frames)

    def chunk(fourcc, data):
        return fourcc + struct.pack('<I', len(data)) + data + (b'\x00' if len(data) & 1 else b'')

    def lst(kind, data):
        return b'LIST' + struct.pack('<I', 4 + len(data)) + kind + data

    avih = struct.pack('<14I', usec, maxb * rate // scale, 0, 0x10, n, 0, 1, maxb, w, h, 0, 0, 0, 0)           # 0x10 = AVIF_HASINDEX
    strh = b'vids' + b'MJPG' + struct.pack('<IHHIIIIIIII', 0, 0, 0, 0, scale, rate, 0, n, maxb, 0xFFFFFFFF, 0) + struct.pack('<4H', 0, 0, w, h)
    strf = struct.pack('<IiiHH4sIiiII', 40, w, h, 1, 24, b'MJPG', w * h * 3, 0, 0, 0, 0)
    hdrl = lst(b'hdrl', chunk(b'avih', avih) + lst(b'strl', chunk(b'strh', strh) + chunk(b'strf', strf)))
    movi_data, index, off = b'', b'', 4
    for f in frames:
        c = chunk(b'00dc', f)
        index += b'00dc' + struct.pack('<III', 0x10, off, len(f))           # 0x10 = AVIIF_KEYFRAME; offset relative to 'movi'
        movi_data += c
        off += len(c)
    body = b'AVI ' + hdrl + lst(b'movi', movi_data) + chunk(b'idx1', index)
    with open(path, 'wb') as fh:
        fh.write(b'RIFF' + struct.pack('<I', len(body)) + body)
    return path


def print_segmentation_onto_image(image, prediction, color_map):
    '''helpers/visualization_utils.py:7-52: RGBA overlay of the argmax map (returns a PIL image).'''
    from PIL import Image
    if (image.shape[0] != prediction.shape[1]) or (image.shape[1] != prediction.shape[2]):
        raise ValueError("'image' and 'prediction' must have the same height and width, but image has spatial dimensions ({}, {}) and prediction has spatial dimensions ({}, {}).".format(image.shape[0], image.shape[1], prediction.shape[1], prediction.shape[2]))
    mask = np.zeros(shape=(image.shape[0], image.shape[1], 4), dtype=np.uint8)
    segmentation_map = np.squeeze(np.argmax(prediction, axis=-1))
    for segmentation_class, color_value in color_map.items():
        mask[segmentation_map == segmentation_class] = color_value
    mask = Image.fromarray(mask, mode='RGBA')
    out = Image.fromarray(np.asarray(image, dtype=np.uint8)).convert('RGB')
    out.paste(mask, box=None, mask=mask)
    return out
