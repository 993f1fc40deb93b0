#!/usr/bin/env python3
"""Monte-Carlo dropout inference: what running the trunk once buys, and the accumulate kernel against a copy.

Model leg, per shape (16 x 1024x512, 1 x 2048x1024) and precision (fp32, bf16_train), the full-width model, frozen, device tensors in
and out: Engine.predict (softmax out) and Engine.predict_mc at S = 1 / 4 / 8 / 16 (mean softmax, entropy and mutual information out,
keep_prob 0.5), each call between two device events, the five states alternating in blocks of --reps calls in one process.  Per state:
the median over its calls and the spread (max - min) of its block medians.  Next to predict_mc(S) stands S x t(predict): what S
back-to-back dropout-enabled predict calls would cost (a lower bound: they would also need an accumulation pass each).
Condition row per shape and precision: t(predict_mc, S = 8) + the spread of the predict blocks < 8 t(predict); nothing is tuned to make it true.
Kernel leg, 16 x 1024x512 x 20 classes, plain layout: fcn8s_op_mc_accumulate as a middle sample (logits in, both accumulators read and
written: the bytes of most launches of a call), as a first sample (accumulators written only) and as a last sample (accumulators read,
all four outputs written), each next to a same-process device-to-device copy of the same algorithmic bytes (half of them read, half
written).  Inputs rotate through more sets than 2 x the 256 MiB Infinity Cache holds.  Alternating blocks, device events around --kreps
launches.  Records ratio_to_copy; no figure is fixed in advance.
Prints one JSON line per record and writes them to --out if given."""
import argparse
import ctypes as C
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from cityscapes_eval_bench import CACHE_BYTES, PEAK_HBM, SHAPES, timed  # noqa: E402

SAMPLES = (1, 4, 8, 16)


def model_leg(shapes, precisions, warmup, reps, blocks):
    import torch
    from fcn8s_tensorflow_amd.engine import Engine
    out = []
    for name, n, h, w in shapes:
        g = torch.Generator(device="cuda").manual_seed(0)
        img = torch.randint(0, 256, (n, h, w, 3), dtype=torch.uint8, device="cuda", generator=g)
        for prec in precisions:
            e = Engine(20, device_id=0, seed=0, precision=prec)
            e.freeze()
            states = [("predict", lambda: e.predict(img, argmax=False))]
            for S in SAMPLES:
                states.append(("predict_mc_S%d" % S, (lambda S_: lambda: e.predict_mc(img, samples=S_, keep_prob=0.5, argmax=False))(S)))

            def run(fn, k):
                ev = []
                for _ in range(k):
                    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    a.record(); fn(); b.record()
                    ev.append((a, b))
                torch.cuda.synchronize()
                return [a.elapsed_time(b) for a, b in ev]

            for _, fn in states:                                       # every state's buffers and banks exist before anything is timed
                run(fn, max(2, warmup))
            allocs = e.get_option("workspace_allocations")
            calls = {st: [] for st, _ in states}
            meds = {st: [] for st, _ in states}
            for _ in range(blocks):                                    # alternating blocks: all states see the same clocks and neighbours
                for st, fn in states:
                    t = run(fn, reps + 1)[1:]                          # (the first call behind a switch is not counted)
                    calls[st] += t; meds[st].append(float(np.median(t)))
            assert e.get_option("workspace_allocations") == allocs
            e.close()
            torch.cuda.empty_cache()
            med = {st: float(np.median(calls[st])) for st in calls}
            spread = {st: max(meds[st]) - min(meds[st]) for st in calls}
            tp = med["predict"]
            out.append(dict(leg="model", state="predict", shape=name, precision=prec, calls_per_block=reps, blocks=blocks, ms=round(tp, 4),
                            block_median_spread_ms=round(spread["predict"], 4)))
            for S in SAMPLES:
                st = "predict_mc_S%d" % S
                out.append(dict(leg="model", state="predict_mc", samples=S, shape=name, precision=prec, keep_prob=0.5, calls_per_block=reps, blocks=blocks,
                                ms=round(med[st], 4), block_median_spread_ms=round(spread[st], 4), s_predict_calls_ms=round(S * tp, 4),
                                ratio_to_s_predict_calls=round(med[st] / (S * tp), 4), ms_per_sample_beyond_first=round((med[st] - med["predict_mc_S1"]) / max(1, S - 1), 4) if S > 1 else None))
            t8 = med["predict_mc_S8"]
            out.append(dict(leg="model_condition", shape=name, precision=prec, predict_mc_S8_ms=round(t8, 4), spread_predict_ms=round(spread["predict"], 4),
                            eight_predict_ms=round(8 * tp, 4), mc8_plus_spread_below_8_predict=bool(t8 + spread["predict"] < 8 * tp)))
            for r in out[-(len(SAMPLES) + 2):]:
                print(json.dumps(r), flush=True)
    return out


def kernel_leg(warmup, reps, blocks):
    import torch
    from fcn8s_tensorflow_amd import _lib as L
    lib = L.lib
    ptr = lambda t: C.c_void_p(t.data_ptr()) if t is not None else None
    name, n, h, w = SHAPES[0]
    NC = 20
    npix = n * h * w
    lb = npix * NC * 4                                                 # one logits tensor: 671 MB, already more than 2 x the cache
    nsets = max(2, -(-2 * CACHE_BYTES // lb) + 1)
    assert nsets * lb > 2 * CACHE_BYTES
    g = torch.Generator(device="cuda").manual_seed(0)
    logits = [torch.randn((n, h, w, NC), device="cuda", generator=g) * 3 for _ in range(nsets)]
    acc = [torch.zeros((n, h, w, NC), device="cuda") for _ in range(nsets)]
    eacc = [torch.zeros((n, h, w), device="cuda") for _ in range(nsets)]
    sm = torch.empty((n, h, w, NC), device="cuda"); am = torch.empty((n, h, w), dtype=torch.int64, device="cuda")
    ent = torch.empty((n, h, w), device="cuda"); mi = torch.empty((n, h, w), device="cuda")
    roles = {
        # role: (first, last, outputs, algorithmic bytes)
        "middle": (0, 0, (None, None, None, None), lb + 2 * (lb + 4 * npix)),
        "first": (1, 0, (None, None, None, None), lb + (lb + 4 * npix)),
        "last": (0, 1, (sm, am, ent, mi), lb + (lb + 4 * npix) + lb + 8 * npix + 8 * npix),
    }
    out = []
    for role, (first, last, outs, by) in roles.items():
        half = by // 2 // 16 * 16
        src = [torch.empty(half, dtype=torch.uint8, device="cuda") for _ in range(max(2, -(-2 * CACHE_BYTES // half) + 1))]
        dst = torch.empty(half, dtype=torch.uint8, device="cuda")

        def kern(k):
            L.check(lib.fcn8s_op_mc_accumulate(None, ptr(logits[k % nsets]), n, h, w, NC, ptr(acc[k % nsets]), ptr(eacc[k % nsets]), first, last, 8,
                                               *[ptr(t) for t in outs]))

        def copy(k):
            dst.copy_(src[k % len(src)])

        tk, tc = [], []
        for _ in range(blocks):
            tk.append(timed(kern, 1 << 30, warmup, reps)); tc.append(timed(copy, 1 << 30, warmup, reps))
        torch.cuda.synchronize()
        k_us, c_us = float(np.median(tk)), float(np.median(tc))
        rec = dict(leg="kernel", role=role, shape=name, classes=NC, layout="plain", logits_sets=nsets, reps=reps, blocks=blocks, bytes_needed=by,
                   accumulate_us=round(k_us, 2), accumulate_us_min_max=[round(min(tk), 2), round(max(tk), 2)],
                   copy_us=round(c_us, 2), copy_us_min_max=[round(min(tc), 2), round(max(tc), 2)], copy_bytes=2 * half,
                   ratio_to_copy=round(k_us / c_us, 3), accumulate_TBps=round(by / k_us * 1e-6, 3), copy_TBps=round(2 * half / c_us * 1e-6, 3),
                   fraction_of_hbm_8TBps=round(by / (k_us * 1e-6) / PEAK_HBM, 4))
        print(json.dumps(rec), flush=True)
        out.append(rec)
        del src, dst
        torch.cuda.empty_cache()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--reps", type=int, default=4, help="timed calls per block of the model leg")
    ap.add_argument("--blocks", type=int, default=5, help="alternating blocks per state of the model leg")
    ap.add_argument("--kreps", type=int, default=10, help="launches per block of the kernel leg")
    ap.add_argument("--kblocks", type=int, default=10, help="alternating blocks of the kernel leg")
    ap.add_argument("--precisions", default="fp32,bf16_train")
    ap.add_argument("--legs", default="kernel,model")
    ap.add_argument("--out")
    a = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("mc_dropout_bench.py measures on an MI355X; no GPU here")
    recs = []
    legs = a.legs.split(",")
    if "kernel" in legs:
        recs += kernel_leg(a.warmup, a.kreps, a.kblocks)
        torch.cuda.empty_cache()
    if "model" in legs:
        recs += model_leg([SHAPES[0], SHAPES[2]], a.precisions.split(","), a.warmup, a.reps, a.blocks)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            for r in recs:
                f.write(json.dumps(r) + "\n")


if __name__ == "__main__":
    main()
