#!/usr/bin/env python
"""Digests of what a build of libfcn8s_hip.so computes and launches, one JSON line per case: for comparing two BUILDS of the library that
are meant to be the same program (a host-side refactor of csrc/model.hip).  Not a test: it needs the other build.

    python tools/pass_digest.py OUT.jsonl [--full]

A case is one fresh engine: two training steps (SGD, keep_prob 0.5, l2 1e-3), one eval_step, one predict(argmax=False).  Its line holds
SHA-256 digests of the two losses, the logits of the second forward pass, every gradient of step 2, the flat parameters after step 2 and the
predict output ("values", from an engine with option deterministic = 1), and the profile tables of step 2 and of the predict -- group ->
[launches, flops, bytes], no times -- from a second engine with default options ("launches").  fp8_infer runs the eval and predict parts on a
calibration made the way tests/test_state_coherence_gpu.py makes it.  The file keeps one SHA-256 per case over each of the two parts (a few
hundred bytes per case: small enough to commit); --full writes the parts themselves, to find WHICH tensor or profile group moved.

Run it with one build in place, then with the other (copy the .so into place as tools/ab_libs.sh does), and diff the two files.  Before it
writes anything the tool checks that it could tell two builds apart: the launch tables of fuse_out_in 0 / 2, of fc6_fft 0 / 1 and (on
fc6's 4x4 map) of winograd_fc6 1 / 0 differ, and the value digests of two parameter seeds differ."""
import hashlib
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from fcn8s_tensorflow_amd import _lib as L  # noqa: E402
from fcn8s_tensorflow_amd.engine import Engine  # noqa: E402
from oracle import fcn8s_oracle as orc  # noqa: E402  (the initializer only)

CLASSES = 20
WIDTHS = (64, 64, 128, 128, 128, 128, 128)            # the coherence tests' widths: every precision takes them
DEFAULT_WIDTHS = (64, 128, 256, 512, 512, 4096, 4096)
ODD_WIDTHS = (64, 192, 192, 64, 64, 128, 192)         # 192: bt_gemm_ok refuses, the adjoint gradients take their second bank
TRAINING = ('fp32', 'f32x3', 'f32x2', 'bf16_fc', 'bf16_fwd', 'bf16_fwd_x2', 'bf16_train')
SHAPES = ((2, 64, 96), (1, 96, 160), (1, 192, 192))
VARIANT_SHAPE = (1, 96, 160)
VARIANTS = (("fuse_out_in", 0), ("fuse_out_in", 2), ("fuse_dgrad_dout", 0), ("conv1_in_transform", 0), ("winograd_tile", 4), ("fc6_fft_wgrad", 2),
            ("fc6_fft", 0), ("bf16_acts", 0), ("bf16_fuse_pool", 0), ("keep_output_gradients", 1), ("gemm_out_fused64", 0))
# the options that decide something in bf16_fwd (its conv1 / conv2 blocks and all of its backward pass run through Winograd)
BF16_FWD_VARIANTS = ("fuse_out_in", "fuse_dgrad_dout", "conv1_in_transform", "winograd_tile", "keep_output_gradients")
# the options that move a layer from one route to another (csrc/conv_route.h), fp32 and bf16_fwd.  winograd_min_cin = 128 with WIDTHS: direct blocks
# 1-2 and a direct conv3_1 in front of a Winograd conv3_2 -- a "wv:" / "rb:" slot exists for one neighbour only
ROUTE_VARIANTS = ({"winograd_min_cin": 128}, {"winograd_min_cin": 0}, {"winograd_tile": 2}, {"winograd_tile_hires": 4, "winograd_hires_pixels": 8000})
# the false sides of bf16_train's keep-or-skip rules (csrc/conv_route.h, Bf16Opts): no copies in the evaluation / prediction passes, conv1_1 on the
# plain kernel, every fp32 tensor kept.  CONV1_128_WIDTHS: conv1_1 is not the 64-wide gather kernel and conv1_2 converts its own input
BF16_RULE_VARIANTS = ({"bf16_infer_copies": 0}, {"conv1_tiled": 0}, {"bf16_acts": 0, "bf16_fuse_pool": 0})
CONV1_128_WIDTHS = (128,) + WIDTHS[1:]
# fc6's own backward routes (conv_wgrad / conv_dgrad): SHAPES give it maps of 2x3, 3x5 and 6x6, none of which has an F(4x4,4x4) tile.  128x128: a 4x4 map,
# the DFT tiles are not cheaper (292 planes against 196 positions) -- F(4x4,4x4) forward, the Winograd-domain weight gradient, the adjoint data gradient
# (winograd_fc6 = 0: the direct taps and the lazy flipped kernel).  128x256, two images: a 4x8 map, the DFT forward is cheaper (292 against 392) -- the
# weight gradient in F(4x4,4x4) under a held fft6_ready or (fc6_fft_wgrad = 2) in the DFT domain, the data gradient in the DFT domain.
# ODD_WIDTHS: fc6 is 64 -> 128, the adjoint route's transposed-bank GEMM takes it
FC6_ROUTE_CASES = (('fp32', (1, 128, 128), WIDTHS, {}), ('fp32', (1, 128, 128), WIDTHS, {"winograd_fc6": 0}),
                   ('fp32', (2, 128, 256), WIDTHS, {}), ('fp32', (2, 128, 256), WIDTHS, {"fc6_fft": 0}), ('fp32', (2, 128, 256), WIDTHS, {"fc6_fft_wgrad": 2}),
                   ('bf16_fwd', (1, 128, 128), WIDTHS, {}), ('fp32', (1, 128, 128), ODD_WIDTHS, {}))


def sha(a):
    return hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()


def table(prof):
    return {k: [int(v["launches"]), float(v["flops"]), float(v["bytes"])] for k, v in sorted(prof.items()) if int(v["launches"])}


def weighted_layers(shape, widths):
    """(layer, shape of its output gradient) for every layer whose weight gradient knows its own name."""
    n, h, w = shape
    out = []
    for b, nconv in enumerate((2, 2, 3, 3, 3), start=1):
        out += [("conv%d_%d" % (b, i), (n, h, w, widths[b - 1])) for i in range(1, nconv + 1)]
        h //= 2; w //= 2
    return out + [("fc6", (n, h, w, widths[5])), ("fc7", (n, h, w, widths[6]))]


def inputs(shape, seed):
    rng = np.random.default_rng(1000 + seed)
    return rng.integers(0, 256, shape + (3,), dtype=np.uint8), rng.integers(0, CLASSES, shape, dtype=np.uint8)


_params = {}


def load(e, widths, seed):
    if widths == DEFAULT_WIDTHS:          # (0.5 GB of parameters: the library's own initializer, on the device)
        e.init_params(seed)
        return
    if (widths, seed) not in _params:
        _params[(widths, seed)] = orc.init_params(CLASSES, widths, seed=seed, decoder_std_scale=6.0, bias_std=0.05)
    e.set_params(_params[(widths, seed)])


_cal = {}


def calibration(seed):
    if seed not in _cal:
        e = Engine(CLASSES, widths=WIDTHS, precision='fp8_infer'); load(e, WIDTHS, seed)
        _cal[seed] = e.calibrate_fp8(inputs((1, 128, 160), 2)[0], reset=True).copy()
        e.close()
    return _cal[seed]


def run(precision, shape, widths, options, seed, values):
    """One engine through the sequence.  values: the digests (deterministic = 1); else the launch tables (default options)."""
    opts = dict(options)
    if values:
        opts["deterministic"] = 1
    e = Engine(CLASSES, widths=widths, precision=precision, options=opts)
    load(e, widths, seed)
    img, lab = inputs(shape, seed)
    out = {}
    if precision == 'fp8_infer':
        e.set_fp8_calibration(calibration(seed))
    else:
        loss1, _ = e.train_step(img, lab, 1e-3, keep_prob=0.5, l2_rate=1e-3, optimizer=L.OPT_SGD_MOMENTUM)
        if not values:
            e.profile(2); e.profile_reset()
        loss2, _ = e.train_step(img, lab, 1e-3, keep_prob=0.5, l2_rate=1e-3, optimizer=L.OPT_SGD_MOMENTUM)
        if values:
            out["loss"] = [sha(np.float32(loss1)), sha(np.float32(loss2))]
            out["logits"] = sha(e.activation("logits", shape + (CLASSES,)))
            out["grads"] = {k: sha(g) for k, g in e.get_grads().items()}
            out["params"] = sha(e.flat_params.detach().cpu().numpy())
            if opts.get("keep_output_gradients"):
                dy = {}
                for name, shp in weighted_layers(shape, widths):
                    try:
                        a = e.activation("dy:" + name, shp, missing_ok=True)
                    except L.Fcn8sError:          # (handed on as routing bytes, a Winograd-domain image or a bf16 copy: no fp32 tensor)
                        a = None
                    dy[name] = None if a is None else sha(a)
                out["dy"] = dy
        else:
            out["step2"] = table(e.profile_results())
            e.profile(0)
    e.eval_step(img, lab, l2_rate=1e-3)
    if not values:
        e.profile(2); e.profile_reset()
    pred = e.predict(img, argmax=False)
    if values:
        cm, loss_sum, _ = e.metrics_raw()
        out["eval_metrics"] = [sha(cm), sha(np.float64(loss_sum))]
        out["predict"] = sha(pred)
    else:
        out["predict"] = table(e.profile_results())
    e.close()
    return out


def cases():
    for p in TRAINING + ('fp8_infer',):
        for s in SHAPES:
            yield p, s, WIDTHS, {}
    yield 'fp32', VARIANT_SHAPE, DEFAULT_WIDTHS, {}
    yield 'fp32', VARIANT_SHAPE, ODD_WIDTHS, {}
    yield 'fp32', VARIANT_SHAPE, ODD_WIDTHS, {"fuse_dgrad_dout": 0}
    for k, v in VARIANTS:
        for p in ('fp32', 'bf16_train') + (('bf16_fwd',) if k in BF16_FWD_VARIANTS else ()):
            yield p, VARIANT_SHAPE, WIDTHS, {k: v}
    for options in ROUTE_VARIANTS:
        for p in ('fp32', 'bf16_fwd'):
            yield p, VARIANT_SHAPE, WIDTHS, dict(options)
    for options in BF16_RULE_VARIANTS:
        yield 'bf16_train', VARIANT_SHAPE, WIDTHS, dict(options)
    yield 'bf16_train', VARIANT_SHAPE, CONV1_128_WIDTHS, {}
    for p, s, widths, options in FC6_ROUTE_CASES:
        yield p, s, widths, dict(options)


def name_of(p, s, widths, options):
    w = "" if widths == WIDTHS else "/w" + "-".join(str(x) for x in widths)
    return "%s/%dx%dx%d%s%s" % (p, s[0], s[1], s[2], w, "".join("/%s=%d" % kv for kv in sorted(options.items())))


def compact(line):
    return {"case": line["case"], **{k: hashlib.sha256(json.dumps(line[k], sort_keys=True).encode()).hexdigest() for k in ("values", "launches")}}


def main(path, full=False):
    lines = {}
    for p, s, widths, options in cases():
        name = name_of(p, s, widths, options)
        lines[name] = {"case": name, "values": run(p, s, widths, options, 1, True), "launches": run(p, s, widths, options, 1, False)}
        print(name, flush=True)
    # the tool has force: what it digests moves when the program does
    base = "fp32/1x96x160"
    for a, b in (("fp32/1x96x160/fuse_out_in=0", "fp32/1x96x160/fuse_out_in=2"), (base, "fp32/1x96x160/fc6_fft=0"),
                 ("fp32/1x128x128", "fp32/1x128x128/winograd_fc6=0")):
        assert lines[a]["launches"]["step2"] != lines[b]["launches"]["step2"], ("the launch tables do not tell these apart", a, b)
    other = run('fp32', VARIANT_SHAPE, WIDTHS, {}, 2, True)
    for k in ("loss", "logits", "params", "predict"):
        assert other[k] != lines[base]["values"][k], ("another seed, the same digest", k)
    with open(path, "w") as f:
        for name in sorted(lines):
            f.write(json.dumps(lines[name] if full else compact(lines[name]), sort_keys=True) + "\n")
    print("%d cases -> %s" % (len(lines), path))


if __name__ == "__main__":
    main(sys.argv[1], "--full" in sys.argv[2:])
