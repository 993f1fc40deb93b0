"""What every directory sweep of `FCN8s` shares (`predict_and_save` .. `predict_and_export_instances`): the prediction route of an image and
the combinations it refuses, the file walkers with the decode, and the frozen state of the weights for the length of the sweep.  A sweep method
itself is its argument checks, its per-image consumer and its result dict."""
from __future__ import annotations

import contextlib
import math
import os
from glob import glob

import numpy as np

from . import crf as crf_mod
from . import temperature as ts_mod


def check_route(passes, samples=None, temperature=None, mi_max=None, verb='use'):
    """The refusals of the routes: `samples` (the Monte-Carlo route) with `scales` / `flip` / `crf` passes or with a `temperature`, `mi_max`
    without `samples`.  `verb`: what the caller does with a route ('use', 'score').  Returns `mi_max` as a float, or None."""
    if samples is not None and passes:
        raise ValueError("`samples` runs the Monte-Carlo dropout route, which has no `scales` / `flip` / `crf` passes; use one or the other.")
    if samples is not None and temperature is not None:
        raise ValueError("`temperature` with `samples`: calibrating Monte-Carlo samples needs the temperature inside each sample's softmax; "
                         "{} the single-pass, `scales` / `flip` or `crf` route instead.".format(verb))
    if mi_max is not None:
        if samples is None:
            raise ValueError("`mi_max` gates on the mutual information of the Monte-Carlo route: it needs `samples`")
        if not math.isfinite(float(mi_max)):
            raise ValueError("`mi_max` must be finite, got {!r}".format(mi_max))
        mi_max = float(mi_max)
    return mi_max


class Route:
    """How a sweep predicts one image, a uint8 tensor (1,H,W,3).  `name`: 'single' (one `predict_mc` sample without dropout: `predict` bit for
    bit, on images of any size, with the entropy map), 'passes' (`predict` with `scales` / `flip` / `crf`) or 'mc' (`predict_mc`)."""

    def __init__(self, model, name, passes, mc, temperature):
        self.model, self.name, self.passes, self.mc, self.temperature = model, name, passes, mc, temperature

    def softmax(self, image, entropy=False, mutual_information=False):
        """(softmax, entropy | None, mutual information | None): the maps that were asked for and that the route has -- 'passes' has none,
        'single' no mutual information.  A temperature is applied in place by one launch, which on 'single' also gives the entropy of the
        calibrated distribution."""
        if self.name == 'passes':
            return self.model.predict(image, argmax=False, temperature=self.temperature, **self.passes), None, None
        engine = self.model.engine
        prob, ent, mi = engine.predict_mc(image, argmax=False, entropy=entropy, mutual_information=mutual_information and self.name == 'mc',
                                          **self.mc)
        if self.temperature is not None:
            ent = engine.temperature_apply(prob, self.temperature, entropy=entropy, out=prob)[1]
        return prob, ent, mi


def resolve_route(model, scales, flip, crf, temperature=None, samples=None, keep_prob=0.5, sample_offset=0, mi_max=None, verb='use'):
    """The route of a sweep with these arguments, or the ValueError of what it refuses (`check_route`, `temperature.validate_temperature`).
    A temperature of 1.0 launches nothing."""
    if temperature is not None:
        temperature = ts_mod.validate_temperature(temperature)
    passes = scales is not None or bool(flip) or crf_mod.resolve(crf) is not None
    check_route(passes, samples, temperature, mi_max, verb)
    if temperature == 1.0:
        temperature = None
    mc = dict(samples=1, keep_prob=1.0, sample_offset=0)
    if samples is not None:
        mc = dict(samples=samples, keep_prob=keep_prob, sample_offset=sample_offset)
    name = 'mc' if samples is not None else 'passes' if passes else 'single'
    return Route(model, name, dict(scales=scales, flip=flip, crf=crf), mc, temperature)


@contextlib.contextmanager
def frozen(engine):
    """Constant weights for the block -- the transformed filter banks are built once -- and the frozen state it found behind it, whatever the
    block raises."""
    was_frozen = bool(engine.get_option("frozen"))
    engine.freeze(True)
    try:
        yield
    finally:
        engine.freeze(was_frozen)


def image_files(images_dir, ext, allow_none=False):
    """Every `*.<ext>` below `images_dir` (sub-directories = cities, as in leftImg8bit/val), sorted."""
    paths = sorted(glob(os.path.join(images_dir, '**', '*.' + ext), recursive=True))
    if not paths and not allow_none:
        raise ValueError("Cannot find any images below: {}".format(images_dir))
    return paths


def paired_files(images_dir, ground_truth_search, ext):
    """(ground-truth files of the glob, sorted; the image `<city>_<seq>_<frame>*.<ext>` below `images_dir` of each)."""
    from . import cityscapes_eval as ce
    gts = sorted(glob(ground_truth_search))
    if not gts:
        raise ValueError("Cannot find any ground truth images to use for evaluation. Searched for: {}".format(ground_truth_search))
    walk = ce.walk_predictions(images_dir)
    return gts, [ce.find_prediction(images_dir, g, walk, extension=ext) for g in gts]


def load_image(path, resize, device):
    """Decode, `resize=(h, w)` bilinearly unless the file has that size, one upload: (uint8 tensor (1,H,W,3) on `device`, the file's own PIL
    size (w, h))."""
    from PIL import Image
    import torch
    pil = Image.open(path).convert('RGB')
    size = pil.size
    if resize and not np.array_equal((pil.height, pil.width), resize):
        pil = pil.resize((resize[1], resize[0]), Image.BILINEAR)
    return torch.from_numpy(np.array(pil)[None]).to(device), size


def check_label_map(gt, shape, image_path, gt_path):
    """A decoded label-id map against the (height, width) of its image's prediction."""
    from . import cityscapes_eval as ce
    if shape[1] != gt.shape[1]:
        raise ValueError("Image widths of " + image_path + " and " + gt_path + " are not equal.")
    if shape[0] != gt.shape[0]:
        raise ValueError("Image heights of " + image_path + " and " + gt_path + " are not equal.")
    if gt.ndim != 2 or gt.max() >= ce.NUM_IDS:
        raise ValueError("Unknown label with id {:}".format(int(gt.max())))
