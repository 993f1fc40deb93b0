#!/usr/bin/env python3
"""The soft-target term (fcn8s_set_soft_targets): its kernel against a copy of its bytes, what it adds to the training step, and the teacher's own time.

The kernel has no op-level entry point, so it is timed where it runs: inside fcn8s_forward_loss of the full-width fp32 model, by the device events of
its profile group ("soft_targets": the kernel and its one-block reduction).

Kernel leg, per shape (16 x 1024x512 x 20, 1 x 2048x1024 x 20) and per logits layout (tconv_gemm 0 = plain, 1 = blocked): --reps training losses per
block with the term on, each with its own binding; kernel_us = the group's time / its launches.  Alternating with it in the same process: a
device-to-device copy of the kernel's algorithmic bytes (321 B per pixel at C = K = 20: logits 4 C, targets 4 K, the label byte, dlogits read and
written 8 C), half of them read and half written, source buffers rotated through more than 2 x the 256 MiB Infinity Cache.  The kernel's own inputs
need no rotation: the forward pass that runs between two launches streams several GB through the cache; the targets rotate through --target-sets
tensors all the same.  ratio_to_copy against the 1.25 x the project's streaming kernels aim at is reported, not asserted.
Step leg, 16 x 1024x512, full-width fp32: Engine.train_step on device tensors with the term off (the parent commit's step: nothing of the term is
launched) and on, the two states alternating in blocks of --step-reps steps, every step between two device events.  Per state the median over its
steps and the spread (max - min) of its block medians.  The condition row: added = on - off against the kernel's time at this shape and layout (kernel
leg, same run) plus the off state's spread -- added_within_kernel_plus_noise; nothing is tuned to make it true.
Teacher leg: a second full-width fp32 model's predict(argmax=False) on the same device images, device in and device out -- reported separately, it is
no part of the condition.
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

from cityscapes_eval_bench import CACHE_BYTES, PEAK_HBM, timed  # noqa: E402

SHAPES = [("16x1024x512", 16, 512, 1024), ("1x2048x1024", 1, 1024, 2048)]
NC, BAR = 20, 1.25
WEIGHT, TEMP = 1.0, 2.0


def batch(n, h, w, seed=0):
    import torch
    g = torch.Generator(device="cuda").manual_seed(seed)
    img = torch.randint(0, 256, (n, h, w, 3), dtype=torch.uint8, device="cuda", generator=g)
    lab = torch.randint(0, NC, (n, h, w), dtype=torch.uint8, device="cuda", generator=g)
    lab[torch.rand((n, h, w), device="cuda", generator=g) < 0.05] = 255
    return img, lab


def target_sets(n, h, w, count):
    """`count` tensors of spatially varying, sharpened rows"""
    import torch
    g = torch.Generator(device="cuda").manual_seed(1)
    out = []
    for _ in range(count):
        t = torch.randn((n, h, w, NC), device="cuda", generator=g)
        out.append(torch.softmax(t.mul_(3.0), -1))
        del t
    return out


def kernel_leg(warmup, reps, blocks, nsets):
    import torch
    from fcn8s_tensorflow_amd import _lib as L
    from fcn8s_tensorflow_amd.engine import Engine
    out = []
    for name, n, h, w in SHAPES:
        npix = n * h * w
        by = npix * (4 * NC + 4 * NC + 1 + 8 * NC)
        half = by // 2 // 16 * 16
        ncopy = max(2, -(-2 * CACHE_BYTES // half) + 1)
        src = [torch.empty(half, dtype=torch.uint8, device="cuda").random_() for _ in range(ncopy)]
        dst = torch.empty(half, dtype=torch.uint8, device="cuda")
        copy = lambda k: dst.copy_(src[k % ncopy])
        img, lab = batch(n, h, w)
        tg = target_sets(n, h, w, nsets)
        for gemm in (0, 1):
            e = Engine(NC, device_id=0, seed=0, options=dict(tconv_gemm=gemm))
            e.set_soft_targets(WEIGHT, TEMP, 'valid')
            pi, pl = C.c_void_p(img.data_ptr()), C.c_void_p(lab.data_ptr())
            turn = [0]

            def losses(k):
                for _ in range(k):
                    e.bind_soft_targets(tg[turn[0] % nsets]); turn[0] += 1
                    L.check(L.lib.fcn8s_forward_loss(e.h, pi, L.IMG_U8, pl, n, h, w, 0.5, 0.0, L.DEVICE), e.h)
                    e._soft_targets = None
            losses(max(2, warmup))
            torch.cuda.synchronize()
            e.profile(True)
            tk, tc = [], []
            for _ in range(blocks):                                    # alternating blocks: both see the same clocks and neighbours
                e.profile_reset()
                losses(reps)
                torch.cuda.synchronize()
                grp = e.profile_results()["soft_targets"]
                assert grp["launches"] == reps
                tk.append(grp["ms"] * 1e3 / reps)
                tc.append(timed(copy, 1 << 30, warmup, reps))
            term = e.soft_target_term()
            e.close()
            k_us, c_us = float(np.median(tk)), float(np.median(tc))
            rec = dict(leg="kernel", shape=name, classes=NC, ncols=NC, layout="blocked" if gemm else "plain", temperature=TEMP, pixels="valid",
                       reps=reps, blocks=blocks, target_sets=nsets, copy_sets=ncopy, bytes_needed=by, bytes_per_pixel=by / npix,
                       kernel_us=round(k_us, 2), kernel_us_min_max=[round(min(tk), 2), round(max(tk), 2)],
                       copy_us=round(c_us, 2), copy_us_min_max=[round(min(tc), 2), round(max(tc), 2)], copy_bytes=2 * half,
                       ratio_to_copy=round(k_us / c_us, 3), within_bar=bool(k_us / c_us <= BAR), bar=BAR,
                       kernel_TBps=round(by / k_us * 1e-6, 3), fraction_of_hbm_8TBps=round(by / (k_us * 1e-6) / PEAK_HBM, 4), term=term)
            print(json.dumps(rec), flush=True)
            out.append(rec)
        del src, dst, tg
        torch.cuda.empty_cache()
    return out


def step_leg(kernel_recs, warmup, reps, blocks):
    import torch
    from fcn8s_tensorflow_amd.engine import Engine
    name, n, h, w = SHAPES[0]
    img, lab = batch(n, h, w)
    tg = target_sets(n, h, w, 1)[0]
    e = Engine(NC, device_id=0, seed=0)
    layout = "blocked" if e.get_option("tconv_gemm") else "plain"
    states = (("off", lambda: e.set_soft_targets()), ("on", lambda: e.set_soft_targets(WEIGHT, TEMP, 'valid')))

    def run(k, on):
        """k steps queued back to back, each between two device events of its own -> ms per step"""
        ev = []
        for _ in range(k):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            if on:
                e.bind_soft_targets(tg)
            e.train_step(img, lab, 1e-6, keep_prob=0.5, fetch_loss=False)
            b.record()
            ev.append((a, b))
        torch.cuda.synchronize()
        return [a.elapsed_time(b) for a, b in ev]

    for st, switch in states:                                          # both states' buffers exist before anything is timed
        switch()
        run(max(2, warmup), st == "on")
    allocs = e.get_option("workspace_allocations")
    steps = {"off": [], "on": []}
    meds = {"off": [], "on": []}
    for _ in range(blocks):                                            # alternating blocks: both states see the same clocks and neighbours
        for st, switch in states:
            switch()
            t = run(reps + 1, st == "on")[1:]                          # (the first step behind a switch is not counted)
            steps[st] += t; meds[st].append(float(np.median(t)))
    assert e.get_option("workspace_allocations") == allocs
    e.close()
    out, stat = [], {}
    for st in ("off", "on"):
        stat[st] = (float(np.median(steps[st])), max(meds[st]) - min(meds[st]))
        out.append(dict(leg="step", state=st, shape=name, precision="fp32", layout=layout, weight=WEIGHT if st == "on" else 0.0,
                        temperature=TEMP if st == "on" else None, steps_per_block=reps, blocks=blocks, step_ms=round(stat[st][0], 4),
                        block_median_ms_min=round(min(meds[st]), 4), block_median_ms_max=round(max(meds[st]), 4),
                        block_median_spread_ms=round(stat[st][1], 4)))
    k_us = next(r["kernel_us"] for r in kernel_recs if r["shape"] == name and r["layout"] == layout)
    added = stat["on"][0] - stat["off"][0]
    bound = k_us * 1e-3 + stat["off"][1]
    out.append(dict(leg="step_condition", shape=name, layout=layout, added_ms=round(added, 4), added_fraction_of_step=round(added / stat["off"][0], 5),
                    t_kernel_ms=round(k_us * 1e-3, 4), spread_off_ms=round(stat["off"][1], 4), bound_ms=round(bound, 4),
                    added_within_kernel_plus_noise=bool(added <= bound)))
    for r in out:
        print(json.dumps(r), flush=True)
    return out


def teacher_leg(warmup, reps):
    import torch
    from fcn8s_tensorflow_amd.engine import Engine
    name, n, h, w = SHAPES[0]
    img, _ = batch(n, h, w)
    t = Engine(NC, device_id=0, seed=1)
    t.freeze(True)
    for _ in range(max(2, warmup)):
        t.predict(img, argmax=False)
    torch.cuda.synchronize()
    ms = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record(); t.predict(img, argmax=False); b.record()
        torch.cuda.synchronize()
        ms.append(a.elapsed_time(b))
    t.close()
    rec = dict(leg="teacher", shape=name, precision="fp32", widths="full", call="predict(argmax=False), device in / device out, frozen",
               reps=reps, predict_ms=round(float(np.median(ms)), 4), predict_ms_min_max=[round(min(ms), 4), round(max(ms), 4)])
    print(json.dumps(rec), flush=True)
    return [rec]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--reps", type=int, default=6, help="training losses (and copies) per block of the kernel leg")
    ap.add_argument("--blocks", type=int, default=6, help="alternating blocks of the kernel leg")
    ap.add_argument("--target-sets", type=int, default=2)
    ap.add_argument("--step-reps", type=int, default=8, help="timed training steps per block of the step leg")
    ap.add_argument("--step-blocks", type=int, default=8, help="alternating blocks per state of the step leg")
    ap.add_argument("--skip-step", action="store_true")
    ap.add_argument("--out")
    a = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("soft_targets_bench.py measures on an MI355X; no GPU here")
    recs = kernel_leg(a.warmup, a.reps, a.blocks, a.target_sets)
    torch.cuda.empty_cache()
    if not a.skip_step:
        recs += step_leg(recs, a.warmup, a.step_reps, a.step_blocks)
        torch.cuda.empty_cache()
        recs += teacher_leg(a.warmup, max(5, a.step_reps))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            for r in recs:
                f.write(json.dumps(r) + "\n")


if __name__ == "__main__":
    main()
