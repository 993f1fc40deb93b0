#!/usr/bin/env python3
"""fp8_infer against bf16_train predictions on one frozen full-width model (two engines with the same parameters in one process).

Per case (16 x 1024x512, 1 x 1024x512, 4 x 2048x1024; device uint8 input, device argmax output) the two modes are timed in alternating
rounds (median of --calls synchronised calls per round after --warmup), then one profiled call per mode gives the per-layer groups
(ms, launches, TFLOP/s of the algorithmic direct-convolution flops, fraction of the mode's dense peak: 2.5 PFLOP/s bf16, 5 PFLOP/s MX fp8).
The fp8 engine's calibration is one batch of the case's images; its time is reported too, with the pixel agreement of the two modes'
argmax.  Prints one JSON line per case and appends them to --out if given."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

PEAK = {'bf16_train': 2.5e15, 'fp8_infer': 5.0e15}
CASES = [("16x1024x512", 16, 512, 1024), ("1x1024x512", 1, 512, 1024), ("4x2048x1024", 4, 1024, 2048)]


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
    return float(np.median(ts)) * 1e3


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--cases", default=",".join(c[0] for c in CASES))
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import torch
    assert torch.cuda.is_available(), "fp8_bench needs an MI355X"
    from fcn8s_tensorflow_amd.engine import Engine
    eng = {}
    for mode in ('bf16_train', 'fp8_infer'):
        e = Engine(20, device_id=0)
        e.init_params(seed=0)
        e.set_precision(mode)
        eng[mode] = e
    eng['fp8_infer'].set_params(eng['bf16_train'].get_params())
    lines = []
    for name, N, H, W in CASES:
        if name not in a.cases.split(","):
            continue
        img = torch.from_numpy(np.random.default_rng(0).integers(0, 256, (N, H, W, 3), dtype=np.uint8)).cuda()
        e8 = eng['fp8_infer']
        e8.freeze(False)
        torch.cuda.synchronize(); t0 = time.perf_counter()
        e8.calibrate_fp8(img, reset=True)
        torch.cuda.synchronize(); cal_ms = (time.perf_counter() - t0) * 1e3
        for e in eng.values():
            e.freeze(True)
            e.predict(img)
        ms = {m: [] for m in eng}
        for _ in range(a.rounds):
            for m, e in eng.items():
                ms[m].append(timed(lambda: e.predict(img), a.calls, a.warmup))
        preds = {m: e.predict(img).cpu().numpy() for m, e in eng.items()}
        rec = dict(case=name, N=N, H=H, W=W, calibrate_ms=round(cal_ms, 3),
                   argmax_agreement=float((preds['bf16_train'] == preds['fp8_infer']).mean()))
        for m, e in eng.items():
            med = float(np.median(ms[m]))
            rec[m] = dict(ms=round(med, 4), ms_rounds=[round(x, 4) for x in ms[m]], images_per_s=round(N / med * 1e3, 1))
            e.profile(2); e.profile_reset()
            e.predict(img)
            torch.cuda.synchronize()
            groups = {}
            for g, r in e.profile_results().items():
                if r['ms'] <= 0:
                    continue
                d = dict(ms=round(r['ms'], 4), launches=r['launches'])
                if r['flops'] > 0:
                    d['tflops'] = round(r['flops'] / (r['ms'] * 1e-3) / 1e12, 1)
                    d['of_peak'] = round(r['flops'] / (r['ms'] * 1e-3) / PEAK[m], 3)
                groups[g] = d
            rec[m]['groups'] = groups
            e.profile(False)
        rec['speedup'] = round(rec['bf16_train']['ms'] / rec['fp8_infer']['ms'], 3)
        line = json.dumps(rec)
        print(line, flush=True)
        lines.append(line)
    if a.out:
        with open(a.out, "a") as f:
            for line in lines:
                f.write(line + "\n")
    for e in eng.values():
        e.close()


if __name__ == "__main__":
    main()
