#!/usr/bin/env python3
"""The strong-augmentation op (fcn8s_op_strong_augment) against a copy of its bytes, and what `unlabeled_augment=True` adds to a self-training
step of FCN8s.train(unlabeled_generator=...).

Op leg, per shape (16 x 1024x512, 1 x 2048x1024) and mode, every gate open: `colour` (saturation, brightness and hue: the HSV step alone),
`blur` (R = 4, the upper half of the 16 default levels, so that every level has taps beside the centre), `both`, and `both_contrast` (the same with
a contrast strength: the clear and the grey-sum kernels run first).  Its algorithmic bytes are 6 per pixel (3 read, 3 written) and 9 with the
grey-sum pass (3 more read), next to a same-process device-to-device copy of as many bytes (half of them read, half written).  Inputs rotate
through more sets than 2 x the 256 MiB Infinity Cache holds.  Alternating blocks, device events around --kreps launches.  Every record holds
ratio_to_copy against the 1.25 x the project's streaming kernels aim at (reported, not asserted).

Step leg, the full-width fp32 model, 1024x512, a second, frozen model as the labeler ('self' has the known workspace stall): the self-training
step of 8 labelled + 8 unlabelled images through the facade's own join, without and with `unlabeled_augment=True`, alternating in one process
with the op alone on the 8 images at the same settings.  Condition row: t(with) <= t(without) + t(op alone) + the spread of the blocks of the
step without; printed true or false, a record, not a gate.
Prints one JSON line per record and writes them to --out if given."""
import argparse
import ctypes as C
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from cityscapes_eval_bench import CACHE_BYTES, PEAK_HBM, SHAPES, timed  # noqa: E402

NC = 20
BAR = 1.25
ONE = 65536
MODES = {"colour": ([ONE, 0, 16384, 16384, 22], False, 6), "blur": (None, True, 6), "both": ([ONE, 0, 16384, 16384, 22], True, 6),
         "both_contrast": ([ONE, 16384, 16384, 16384, 22], True, 9)}


def op_leg(shapes, warmup, reps, blocks):
    import torch
    from fcn8s_tensorflow_amd import _lib as L, strong_augment as SA
    lib = L.lib
    ptr = lambda t: C.c_void_p(t.data_ptr()) if t is not None else None
    taps = SA.taps_table(0.15, 1.15, 16, 4)[8:]
    blur_h = (C.c_int32 * 3)(ONE, taps.shape[0], taps.shape[1] - 1)
    taps_h = (C.c_uint16 * taps.size)(*[int(v) for v in taps.reshape(-1)])
    out = []
    for name, n, h, w in shapes:
        npix = n * h * w
        nsets = max(2, -(-2 * CACHE_BYTES // (3 * npix)) + 1)
        assert nsets * 3 * npix > 2 * CACHE_BYTES
        work = torch.empty(SA.work_bytes(n), dtype=torch.uint8, device="cuda")
        oi = torch.empty((n, h, w, 3), dtype=torch.uint8, device="cuda")
        par = torch.empty((n, 8), dtype=torch.int32, device="cuda")
        images = [torch.randint(0, 256, (n, h, w, 3), dtype=torch.uint8, device="cuda") for _ in range(nsets)]
        for mode, (jitter, blurred, per_px) in MODES.items():
            by = per_px * npix
            half = by // 2 // 16 * 16
            csrc = [torch.empty(half, dtype=torch.uint8, device="cuda") for _ in range(max(2, -(-2 * CACHE_BYTES // half) + 1))]
            cdst = torch.empty(half, dtype=torch.uint8, device="cuda")
            jit_h = (C.c_int32 * 5)(*jitter) if jitter is not None else None
            args = [(None, ptr(im), n, h, w, 3, s, jit_h, blur_h if blurred else None, taps_h if blurred else None, ptr(work), ptr(oi), ptr(par))
                    for s, im in enumerate(images)]
            rcs = []

            def kern(k):
                rcs.append(lib.fcn8s_op_strong_augment(*args[k % nsets]))

            def copy(k):
                cdst.copy_(csrc[k % len(csrc)])

            tk, tc = [], []
            for _ in range(blocks):
                tk.append(timed(kern, 1 << 30, warmup, reps)); tc.append(timed(copy, 1 << 30, warmup, reps))
            torch.cuda.synchronize()
            assert not any(rcs), L.lib.fcn8s_last_error(None)
            p = par.cpu().numpy()
            assert p[:, 0].all() == (jitter is not None) and p[:, 6].all() == blurred
            k_us, c_us = float(np.median(tk)), float(np.median(tc))
            rec = dict(leg="op", op="strong_augment", mode=mode, shape=name, radius=4 if blurred else 0, input_sets=nsets, reps=reps, blocks=blocks,
                       bytes_per_pixel=per_px, bytes_needed=by, op_us=round(k_us, 2), op_us_min_max=[round(min(tk), 2), round(max(tk), 2)],
                       copy_us=round(c_us, 2), copy_us_min_max=[round(min(tc), 2), round(max(tc), 2)], copy_bytes=2 * half,
                       copy_TBps=round(2 * half / c_us * 1e-6, 3), ratio_to_copy=round(k_us / c_us, 3), within_bar=bool(k_us / c_us <= BAR), bar=BAR,
                       op_TBps=round(by / k_us * 1e-6, 3), fraction_of_hbm_8TBps=round(by / (k_us * 1e-6) / PEAK_HBM, 4))
            print(json.dumps(rec), flush=True)
            out.append(rec)
            del csrc, cdst
        del images, oi
        torch.cuda.empty_cache()
    return out


def step_leg(warmup, reps, blocks):
    import torch
    from fcn8s_tensorflow_amd.fcn8s import FCN8s
    H, W, NL, NU = 512, 1024, 8, 8
    m = FCN8s(vgg16_dir='synthetic:0', num_classes=NC)
    e = m.engine
    g = torch.Generator(device="cuda"); g.manual_seed(0)
    img8 = torch.randint(0, 256, (NL, H, W, 3), dtype=torch.uint8, device="cuda", generator=g)
    unl8 = torch.randint(0, 256, (NU, H, W, 3), dtype=torch.uint8, device="cuda", generator=g)
    lab8 = torch.randint(0, NC, (NL, H, W), dtype=torch.uint8, device="cuda", generator=g)
    thr = np.zeros(NC, np.float32)                                             # an untrained model: every pixel keeps its label

    def forever():
        while True:
            yield unl8
    other = FCN8s(vgg16_dir='synthetic:1', num_classes=NC)
    other.engine.freeze(True)
    plain = m._resolve_unlabeled(forever(), other, thr, None, True, 0, None, False)
    strong = m._resolve_unlabeled(forever(), other, thr, None, True, 0, None, False, True)
    lr = 1e-6
    draw = [0]

    def step(u):
        x, y = m._join_unlabeled(u, img8, lab8, draw[0]); draw[0] += 1
        e.train_step(x, y, lr)

    states = [("self_training_step_8_8", lambda: step(plain)),
              ("self_training_step_8_8_augmented", lambda: step(strong)),
              ("strong_augment_op_8", lambda: e.strong_augment(unl8, draw=1, jitter=strong.augment['jitter'], blur=strong.augment['blur']))]

    def wall(fn):
        fn()                                                                   # discarded: the first call after another state
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(reps):
            fn()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3 / reps

    for _ in range(max(1, warmup)):
        for _, fn in states:
            fn()
    ts = {name: [] for name, _ in states}
    for _ in range(blocks):
        for name, fn in states:
            ts[name].append(wall(fn))
    m.close(); other.close()
    med = {k: float(np.median(v)) for k, v in ts.items()}
    spread = max(ts["self_training_step_8_8"]) - min(ts["self_training_step_8_8"])
    common = dict(leg="step", shape="1024x512", precision="fp32", labelled=NL, unlabelled=NU, labeler="model", reps=reps, blocks=blocks)
    recs = [dict(common, state=k, ms=round(med[k], 3), block_spread_ms=round(max(ts[k]) - min(ts[k]), 3)) for k in ts]
    bound = med["self_training_step_8_8"] + med["strong_augment_op_8"] + spread
    key = "self_training_step_8_8_augmented"
    recs.append(dict(leg="step_condition", shape="1024x512", precision="fp32", labeler="model", augmented_step_ms=round(med[key], 3),
                     augmented_step_ms_min_max=[round(min(ts[key]), 3), round(max(ts[key]), 3)], step_plus_op_plus_spread_ms=round(bound, 3),
                     spread_ms=round(spread, 3), step_within_parts_plus_spread=bool(med[key] <= bound)))
    for r in recs:
        print(json.dumps(r), flush=True)
    return recs


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--kreps", type=int, default=10, help="launches per block of the op leg")
    ap.add_argument("--kblocks", type=int, default=10, help="alternating blocks of the op leg")
    ap.add_argument("--reps", type=int, default=2, help="calls per block of the step leg")
    ap.add_argument("--blocks", type=int, default=5, help="alternating blocks of the step leg")
    ap.add_argument("--legs", default="op,step")
    ap.add_argument("--out")
    a = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("strong_augment_bench.py measures on an MI355X; no GPU here")
    recs = []
    legs = a.legs.split(",")
    if "op" in legs:
        recs += op_leg([SHAPES[0], SHAPES[2]], a.warmup, a.kreps, a.kblocks)
        torch.cuda.empty_cache()
    if "step" in legs:
        recs += step_leg(a.warmup, a.reps, a.blocks)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            for r in recs:
                f.write(json.dumps(r) + "\n")


if __name__ == "__main__":
    main()
