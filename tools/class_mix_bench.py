#!/usr/bin/env python3
"""The ClassMix op (fcn8s_op_class_mix) against a copy of its bytes, and what a self-training step of FCN8s.train(unlabeled_generator=...)
costs next to its parts.

Op leg, per shape (16 x 1024x512, 1 x 2048x1024), 20 classes, src = (n + 1) mod N, and two label maps: cityscapes_like (blocks of 64 x 64
pixels of seven classes, 2 % of the pixels salted with other ids and with the ignore id 255) and constant (one class everywhere: every pixel
is pasted).  One call = clear + presence + selection + mix; its algorithmic bytes are 13 per pixel (the presence pass reads 1, the mix reads 4
from each of two images and their labels and writes 4), next to a same-process device-to-device copy of 13 bytes per pixel (half of them
read, half written).  Inputs rotate through more sets than 2 x the 256 MiB Infinity Cache holds.  Alternating blocks, device events around
--kreps launches.  Every record holds ratio_to_copy against the 1.25 x the project's streaming kernels aim at (reported, not asserted).

Step leg, the full-width fp32 model, 1024x512: a self-training step (8 labelled + 8 unlabelled images, through the facade's own join) with the
'self' labeler and with a second, frozen model as the labeler, alternating in one process with the plain train_step on 16 labelled images, the
unfrozen `predict` of 8, the pseudo_label op and the class_mix op on the 8.  Condition rows, one per labeler: t(self-training step) <= t(plain
step of 16) + t(predict of 8) + t(pseudo_label) + t(class_mix) + the plain state's spread; printed true or false, a record, not a gate.  With
'self' (and 'ema') the student's engine sees batches of 8 and of 16 in turn and re-allocates its workspace at every change of shape; a labeler
model of its own keeps both engines on one shape.
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
PER_PX = 13


def label_maps(kind, n, h, w, seed):
    import torch
    g = torch.Generator(device="cuda"); g.manual_seed(seed)
    if kind == "constant":
        return torch.full((n, h * w), seed % NC, dtype=torch.uint8, device="cuda")
    pool = torch.tensor([0, 1, 2, 8, 10, 11, 13], dtype=torch.uint8, device="cuda")
    low = pool[torch.randint(0, len(pool), (n, h // 64, w // 64), device="cuda", generator=g)]
    lab = low.repeat_interleave(64, 1).repeat_interleave(64, 2).contiguous()
    salt = torch.rand((n, h, w), device="cuda", generator=g) < 0.02
    other = torch.randint(0, NC + 1, (n, h, w), device="cuda", generator=g).to(torch.uint8)
    other[other == NC] = 255
    return torch.where(salt, other, lab).reshape(n, h * w).contiguous()


def op_leg(shapes, warmup, reps, blocks):
    import torch
    from fcn8s_tensorflow_amd import _lib as L, class_mix as CM
    lib = L.lib
    ptr = lambda t: C.c_void_p(t.data_ptr()) if t is not None else None
    out = []
    for name, n, h, w in shapes:
        npix = n * h * w
        nsets = max(2, -(-2 * CACHE_BYTES // (4 * npix)) + 1)
        assert nsets * 4 * npix > 2 * CACHE_BYTES
        src = ((torch.arange(n, dtype=torch.int32, device="cuda") + 1) % n).contiguous()
        work = torch.empty(CM.work_bytes(n), dtype=torch.uint8, device="cuda")
        oi = torch.empty((npix, 3), dtype=torch.uint8, device="cuda"); ol = torch.empty(npix, dtype=torch.uint8, device="cuda")
        sel = torch.empty((n, 256), dtype=torch.uint8, device="cuda")
        images = [torch.randint(0, 256, (npix, 3), dtype=torch.uint8, device="cuda") for _ in range(nsets)]
        by = PER_PX * npix
        half = by // 2 // 16 * 16
        csrc = [torch.empty(half, dtype=torch.uint8, device="cuda") for _ in range(max(2, -(-2 * CACHE_BYTES // half) + 1))]
        cdst = torch.empty(half, dtype=torch.uint8, device="cuda")
        for kind in ("cityscapes_like", "constant"):
            labels = [label_maps(kind, n, h, w, 7 + s) for s in range(nsets)]
            args = [(None, ptr(im), ptr(lb), ptr(src), n, h * w, NC, 3, s, ptr(work), ptr(oi), ptr(ol), ptr(sel)) for s, (im, lb) in enumerate(zip(images, labels))]
            rcs = []

            def kern(k):
                rcs.append(lib.fcn8s_op_class_mix(*args[k % nsets]))

            def copy(k):
                cdst.copy_(csrc[k % len(csrc)])

            tk, tc = [], []
            for _ in range(blocks):
                tk.append(timed(kern, 1 << 30, warmup, reps)); tc.append(timed(copy, 1 << 30, warmup, reps))
            torch.cuda.synchronize()
            assert not any(rcs), L.lib.fcn8s_last_error(None)
            pasted = float((ol != labels[(warmup + reps - 1) % nsets].reshape(-1)).float().mean()) if kind != "constant" else None
            k_us, c_us = float(np.median(tk)), float(np.median(tc))
            rec = dict(leg="op", op="class_mix", input=kind, shape=name, classes=NC, input_sets=nsets, reps=reps, blocks=blocks, bytes_per_pixel=PER_PX,
                       bytes_needed=by, op_us=round(k_us, 2), op_us_min_max=[round(min(tk), 2), round(max(tk), 2)], copy_us=round(c_us, 2),
                       copy_us_min_max=[round(min(tc), 2), round(max(tc), 2)], copy_bytes=2 * half, copy_TBps=round(2 * half / c_us * 1e-6, 3),
                       ratio_to_copy=round(k_us / c_us, 3), within_bar=bool(k_us / c_us <= BAR), bar=BAR, op_TBps=round(by / k_us * 1e-6, 3),
                       fraction_of_hbm_8TBps=round(by / (k_us * 1e-6) / PEAK_HBM, 4), selected_classes=int(sel[0].sum()), labels_changed_share=pasted)
            print(json.dumps(rec), flush=True)
            out.append(rec)
            del labels
        del images, csrc, cdst, oi, ol
        torch.cuda.empty_cache()
    return out


def step_leg(warmup, reps, blocks):
    import torch
    from fcn8s_tensorflow_amd.fcn8s import FCN8s
    H, W, NL, NU = 512, 1024, 8, 8
    m = FCN8s(vgg16_dir='synthetic:0', num_classes=NC)
    e = m.engine
    g = torch.Generator(device="cuda"); g.manual_seed(0)
    img16 = torch.randint(0, 256, (NL + NU, H, W, 3), dtype=torch.uint8, device="cuda", generator=g)
    lab16 = label_maps("cityscapes_like", NL + NU, H, W, 1).reshape(NL + NU, H, W)
    img8, lab8, unl8 = img16[:NL].contiguous(), lab16[:NL].contiguous(), img16[NL:].contiguous()
    thr = np.zeros(NC, np.float32)                                             # an untrained model: every pixel keeps its label, the mix does all its work

    def forever():
        while True:
            yield unl8
    unl = m._resolve_unlabeled(forever(), 'self', thr, None, True, 0, None, False)
    other = FCN8s(vgg16_dir='synthetic:1', num_classes=NC)
    other.engine.freeze(True)
    unl_other = m._resolve_unlabeled(forever(), other, thr, None, True, 0, None, False)
    prob = m.predict(unl8, argmax=False)
    pseudo, tables = e.pseudo_label(prob, thresholds=thr, ignore_id=255, tables=unl.tables)
    lr = 1e-6
    draw = [0]

    def self_step(u=unl):
        x, y = m._join_unlabeled(u, img8, lab8, draw[0]); draw[0] += 1
        e.train_step(x, y, lr)

    states = [("plain_step_16", lambda: e.train_step(img16, lab16, lr)),
              ("self_training_step_8_8", self_step),
              ("self_training_step_8_8_labeler_model", lambda: self_step(unl_other)),
              ("predict_8_unfrozen", lambda: m.predict(unl8, argmax=False)),
              ("pseudo_label_op_8", lambda: e.pseudo_label(prob, thresholds=unl.thresholds, ignore_id=255, tables=unl.tables)),
              ("class_mix_op_8", lambda: e.class_mix(unl8, pseudo, draw=1))]

    def wall(fn):
        fn()                                                                   # discarded: the first call after another state (a change of the engine's batch shape) is not this state's cost
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
    spread = max(ts["plain_step_16"]) - min(ts["plain_step_16"])
    common = dict(leg="step", shape="1024x512", precision="fp32", labelled=NL, unlabelled=NU, reps=reps, blocks=blocks)
    recs = [dict(common, state=k, ms=round(med[k], 3), block_spread_ms=round(max(ts[k]) - min(ts[k]), 3)) for k in ts]
    bound = med["plain_step_16"] + med["predict_8_unfrozen"] + med["pseudo_label_op_8"] + med["class_mix_op_8"] + spread
    for labeler, key in (("self", "self_training_step_8_8"), ("model", "self_training_step_8_8_labeler_model")):
        recs.append(dict(leg="step_condition", shape="1024x512", precision="fp32", labeler=labeler, self_training_step_ms=round(med[key], 3),
                         self_training_step_ms_min_max=[round(min(ts[key]), 3), round(max(ts[key]), 3)], sum_of_parts_plus_spread_ms=round(bound, 3),
                         spread_plain_ms=round(spread, 3), step_within_parts_plus_spread=bool(med[key] <= bound)))
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
        raise SystemExit("class_mix_bench.py measures on an MI355X; no GPU here")
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
