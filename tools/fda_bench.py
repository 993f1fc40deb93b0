#!/usr/bin/env python3
"""The Fourier-domain-adaptation op (fcn8s_op_fda_transfer) against a copy of its bytes, and what `fda_beta` adds to a self-training step of
FCN8s.train(unlabeled_generator=...).

Op leg, per shape (16 + 16 x 1024x512, 1 + 1 x 2048x1024) and half-width (b = 5: beta = 0.01 at a short side of 512; b = 46: beta = 0.09), the
uint8 output alone.  Its algorithmic bytes are 9 per pixel (3 read of the source, 3 of the target, 3 written), next to a same-process
device-to-device copy of as many bytes (half of them read, half written).  Inputs rotate through more sets than 2 x the 256 MiB Infinity Cache
holds.  Alternating blocks, device events around --kreps launches.  Every record holds ratio_to_copy against the 1.25 x the project's streaming
kernels aim at (reported, not asserted), and the issue-time estimate of the op's floating-point work at the fp32 matrix rate: the two MFMA GEMMs
(2 flops per pixel, channel and real column, over N + M images in the analysis and N in the synthesis) plus the two column stages (8 flops per
complex multiply-add), divided by 157.3 TFLOP/s, the MI355X's published fp32 matrix peak.

Step leg, the full-width fp32 model, 1024x512, a second, frozen model as the labeler ('self' has the known workspace stall): the self-training
step of 8 labelled + 8 unlabelled images through the facade's own join, without and with `fda_beta`, alternating in one process with the op
alone on the 8 + 8 images.  Condition row: t(with) <= t(without) + t(op alone) + the spread of the blocks of the step without; printed true or
false, a record, not a gate.
Prints one JSON line per record and writes them to --out if given.  --shapes and --half-widths narrow the op leg to one configuration, so that a
kernel trace of the run (rocprofv3 --kernel-trace --stats -- python tools/fda_bench.py --legs op --shapes 0 --half-widths 5) splits its time by kernel."""
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
PER_PX = 9
FP32_MATRIX = 157.3e12
HALF_WIDTHS = (5, 46)


def flops(n, m, h, w, b):
    cp, B, q = 2 * (b + 1), 2 * b + 1, 3 * (b + 1)
    gemm = 2.0 * h * w * 3 * cp * ((n + m) + n)
    columns = 8.0 * B * h * q * ((n + m) + n)
    return gemm, columns


def op_leg(shapes, warmup, reps, blocks, half_widths=HALF_WIDTHS):
    import torch
    from fcn8s_tensorflow_amd import _lib as L, fda as FDA
    lib = L.lib
    ptr = lambda t: C.c_void_p(t.data_ptr()) if t is not None else None
    out = []
    for name, n, h, w in shapes:
        npix = n * h * w
        nsets = max(2, -(-2 * CACHE_BYTES // (6 * npix)) + 1)
        assert nsets * 6 * npix > 2 * CACHE_BYTES
        oi = torch.empty((n, h, w, 3), dtype=torch.uint8, device="cuda")
        images = [torch.randint(0, 256, (n, h, w, 3), dtype=torch.uint8, device="cuda") for _ in range(nsets)]
        targets = [torch.randint(0, 256, (n, h, w, 3), dtype=torch.uint8, device="cuda") for _ in range(nsets)]
        by = PER_PX * npix
        half = by // 2 // 16 * 16
        csrc = [torch.empty(half, dtype=torch.uint8, device="cuda") for _ in range(max(2, -(-2 * CACHE_BYTES // half) + 1))]
        cdst = torch.empty(half, dtype=torch.uint8, device="cuda")
        for b in half_widths:
            work = torch.empty(FDA.work_bytes(n, n, h, w, b), dtype=torch.uint8, device="cuda")
            args = [(None, ptr(im), n, ptr(tg), n, h, w, b, None, ptr(work), ptr(oi), None) for im, tg in zip(images, targets)]
            rcs = []

            def kern(k):
                rcs.append(lib.fcn8s_op_fda_transfer(*args[k % nsets]))

            def copy(k):
                cdst.copy_(csrc[k % len(csrc)])

            tk, tc = [], []
            for _ in range(blocks):
                tk.append(timed(kern, 1 << 30, warmup, reps)); tc.append(timed(copy, 1 << 30, warmup, reps))
            torch.cuda.synchronize()
            assert not any(rcs), L.lib.fcn8s_last_error(None)
            k_us, c_us = float(np.median(tk)), float(np.median(tc))
            gemm, columns = flops(n, n, h, w, b)
            est_us = (gemm + columns) / FP32_MATRIX * 1e6
            rec = dict(leg="op", op="fda_transfer", shape="%d+%s" % (n, name), b=b, input_sets=nsets, reps=reps, blocks=blocks, bytes_per_pixel=PER_PX,
                       bytes_needed=by, work_bytes=int(work.numel()), op_us=round(k_us, 2), op_us_min_max=[round(min(tk), 2), round(max(tk), 2)],
                       copy_us=round(c_us, 2), copy_us_min_max=[round(min(tc), 2), round(max(tc), 2)], copy_bytes=2 * half,
                       copy_TBps=round(2 * half / c_us * 1e-6, 3), ratio_to_copy=round(k_us / c_us, 3), within_bar=bool(k_us / c_us <= BAR), bar=BAR,
                       op_TBps=round(by / k_us * 1e-6, 3), fraction_of_hbm_8TBps=round(by / (k_us * 1e-6) / PEAK_HBM, 4),
                       gemm_gflop=round(gemm * 1e-9, 3), column_stage_gflop=round(columns * 1e-9, 3), fp32_matrix_TFLOPs=FP32_MATRIX * 1e-12,
                       flops_at_matrix_rate_us=round(est_us, 2), ratio_to_flop_estimate=round(k_us / est_us, 2),
                       reached_TFLOPs=round((gemm + columns) / k_us * 1e-6, 2))
            print(json.dumps(rec), flush=True)
            out.append(rec)
            del work
        del images, targets, oi, csrc, cdst
        torch.cuda.empty_cache()
    return out


def step_leg(warmup, reps, blocks, beta):
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
    adapted = m._resolve_unlabeled(forever(), other, thr, None, True, 0, None, False, None, beta)
    lr = 1e-6
    draw = [0]

    def step(u):
        x, y = m._join_unlabeled(u, img8, lab8, draw[0]); draw[0] += 1
        e.train_step(x, y, lr)

    states = [("self_training_step_8_8", lambda: step(plain)),
              ("self_training_step_8_8_fda", lambda: step(adapted)),
              ("fda_op_8_8", lambda: e.fda_transfer(img8, unl8, beta=beta, pair=[(n + 1) % NU for n in range(NL)]))]

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
    common = dict(leg="step", shape="1024x512", precision="fp32", labelled=NL, unlabelled=NU, labeler="model", fda_beta=beta, reps=reps, blocks=blocks)
    recs = [dict(common, state=k, ms=round(med[k], 3), block_spread_ms=round(max(ts[k]) - min(ts[k]), 3)) for k in ts]
    bound = med["self_training_step_8_8"] + med["fda_op_8_8"] + spread
    key = "self_training_step_8_8_fda"
    recs.append(dict(leg="step_condition", shape="1024x512", precision="fp32", labeler="model", fda_beta=beta, fda_step_ms=round(med[key], 3),
                     fda_step_ms_min_max=[round(min(ts[key]), 3), round(max(ts[key]), 3)], step_plus_op_plus_spread_ms=round(bound, 3),
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
    ap.add_argument("--beta", type=float, default=0.01, help="fda_beta of the step leg")
    ap.add_argument("--legs", default="op,step")
    ap.add_argument("--half-widths", default="5,46", help="half-widths of the op leg")
    ap.add_argument("--shapes", default="0,2", help="indices into the shape list of the op leg (0: 16 x 1024x512, 2: 1 x 2048x1024)")
    ap.add_argument("--out")
    a = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("fda_bench.py measures on an MI355X; no GPU here")
    recs = []
    legs = a.legs.split(",")
    if "op" in legs:
        recs += op_leg([SHAPES[int(i)] for i in a.shapes.split(",")], a.warmup, a.kreps, a.kblocks, tuple(int(b) for b in a.half_widths.split(",")))
        torch.cuda.empty_cache()
    if "step" in legs:
        recs += step_leg(a.warmup, a.reps, a.blocks, a.beta)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            for r in recs:
                f.write(json.dumps(r) + "\n")


if __name__ == "__main__":
    main()
