#!/usr/bin/env python3
"""Multi-scale / flip prediction (fcn8s_predict_tta) against the forwards it is made of.

Per case (one 2048x1024 image, four 1024x512 images; scales 0.75 / 1.0 / 1.25 with flip = 6 passes) and precision (fp32, bf16_train),
on a frozen full-width model:
  * the call time (device input and output, synchronised, median of --calls calls after --warmup) against the sum of frozen
    fcn8s_predict times at the same padded pass shapes, measured in the same process (TTA overhead = call / sum - 1);
  * the tta_input and tta_accumulate profile groups (ms per call, algorithmic bytes, fraction of 8 TB/s);
  * workspace_allocations before and after the timed calls, for the frozen model and again after `freeze(False)` (an unfrozen model keeps
    its banks' storage between calls and rebuilds their contents in every call: call_ms_unfrozen).
Prints one JSON line per (case, precision) and writes them to --out if given."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

PEAK_BPS = 8e12
SCALES = (0.75, 1.0, 1.25)
CASES = [("1x2048x1024", 1, 1024, 2048), ("4x1024x512", 4, 512, 1024)]


def timed(fn, calls, warmup):
    import torch
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(calls):
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        ts.append(time.perf_counter() - t0)
    return float(np.median(ts)) * 1e3, float(np.min(ts)) * 1e3


def run(precision, name, N, H, W, calls, warmup):
    import torch
    from fcn8s_tensorflow_amd import tta
    from fcn8s_tensorflow_amd.engine import Engine
    e = Engine(20, device_id=0, precision=precision, seed=0)
    e.freeze(True)
    img = torch.randint(0, 256, (N, H, W, 3), dtype=torch.uint8, device="cuda")
    # the forwards: frozen fcn8s_predict at each padded pass shape (each shape runs once unflipped and once mirrored)
    fwd = {}
    for s, f, Hs, Ws, Hp, Wp in tta.passes(H, W, SCALES, True):
        if (Hp, Wp) not in fwd:
            x = torch.randint(0, 256, (N, Hp, Wp, 3), dtype=torch.uint8, device="cuda")
            fwd[(Hp, Wp)] = timed(lambda: e.predict(x, argmax=True), calls, warmup)[0]
    fwd_sum = sum(fwd[(p[4], p[5])] for p in tta.passes(H, W, SCALES, True))
    call = lambda: e.predict_tta(img, scales=SCALES, flip=True, argmax=True)
    call()
    torch.cuda.synchronize()
    a0 = e.get_option("workspace_allocations")
    t_med, t_min = timed(call, calls, warmup)
    a1 = e.get_option("workspace_allocations")
    # profile groups of the TTA kernels (a separate, profiled run: the events cost a little)
    e.profile(True); e.profile_reset()
    for _ in range(3):
        call()
    torch.cuda.synchronize()
    prof = e.profile_results()
    e.profile(False)
    e.freeze(False)
    call()
    torch.cuda.synchronize()
    u0 = e.get_option("workspace_allocations")
    tu_med, _ = timed(call, calls, warmup)
    u1 = e.get_option("workspace_allocations")
    groups = {}
    for g in ("tta_input", "tta_accumulate"):
        r = prof.get(g, dict(ms=0.0, launches=0, bytes=0.0))
        ms = r["ms"] / 3
        by = r["bytes"] / 3
        groups[g] = dict(ms_per_call=round(ms, 4), launches_per_call=r["launches"] // 3, bytes_per_call=by,
                         tb_s=round(by / (ms * 1e-3) / 1e12, 3) if ms else None, frac_of_8tbs=round(by / (ms * 1e-3) / PEAK_BPS, 3) if ms else None)
    e.close()
    return dict(case=name, precision=precision, passes=6, scales=list(SCALES), flip=True, call_ms_median=round(t_med, 3), call_ms_min=round(t_min, 3),
                forward_ms_by_shape={"%dx%d" % k: round(v, 3) for k, v in fwd.items()}, sum_of_forwards_ms=round(fwd_sum, 3),
                tta_overhead=round(t_med / fwd_sum - 1, 4), workspace_allocations_before=a0, workspace_allocations_after=a1,
                call_ms_unfrozen=round(tu_med, 3), workspace_allocations_unfrozen_before=u0, workspace_allocations_unfrozen_after=u1, groups=groups)


def main():
    ap = argparse.ArgumentParser(description=__doc__)
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--precisions", default="fp32,bf16_train")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    lines = []
    for prec in a.precisions.split(","):
        for name, N, H, W in CASES:
            r = run(prec, name, N, H, W, a.calls, a.warmup)
            print(json.dumps(r), flush=True)
            lines.append(r)
    if a.out:
        with open(a.out, "w") as f:
            for r in lines:
                f.write(json.dumps(r) + "\n")


if __name__ == "__main__":
    main()
