#!/usr/bin/env python3
"""Mean-field CRF refinement (fcn8s_predict_crf) next to the prediction it refines.

Per case (one 2048x1024 image, four 1024x512 images) and (radius, dilation) in (3, 1), (3, 2), (5, 1), fp32, 5 iterations, on a frozen
full-width model and structured inputs (crf.synthetic_scene):
  * the median call time of predict_crf next to predict_tta with the same scales=(1.0,), measured in the same process, alternating
    (device input and output, synchronised, --calls calls each after --warmup);
  * the crf_meanfield profile group: ms per iteration, and per iteration from the shapes the algorithmic HBM bytes (read Q, read P,
    write Q, read the image), LDS bytes (taps x C floats per pixel) and lane-operations (taps x (14 for the weights + 2 C FMAs) per pixel),
    each divided by its peak (8 TB/s; 150 TB/s of ds_read_b128; 78.6 T lane-operations/s = the 157.3 TFLOP/s fp32 vector peak), and the
    share of the largest of the three floors in the measured time;
  * workspace_allocations before and after the timed calls.
With --distances: max |device - float64 restatement| of fcn8s_op_crf_meanfield on structured scenes (cases of tests/test_crf_gpu.py), next to d32 =
max |float32 restatement - float64 restatement| and the tests' gate 8 max(d32, 2^-23).
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

PEAK_HBM, PEAK_LDS, PEAK_LANE_OPS = 8e12, 150e12, 78.6e12
CASES = [("1x2048x1024", 1, 1024, 2048), ("4x1024x512", 4, 512, 1024)]
WINDOWS = [(3, 1), (3, 2), (5, 1)]
ITERATIONS = 5
DISTANCE_CASES = [   # H, W, C, r, d, T, w_appearance, w_smooth
    (96, 128, 20, 3, 1, 5, 4.0, 2.0), (61, 83, 20, 2, 3, 10, 4.0, 2.0), (64, 64, 4, 5, 1, 5, 10.0, 3.0), (96, 128, 20, 3, 2, 10, 10.0, 3.0),
    (45, 51, 12, 1, 4, 1, 4.0, 2.0), (50, 67, 20, 7, 1, 5, 4.0, 2.0), (70, 91, 20, 3, 8, 5, 4.0, 2.0), (512, 1024, 20, 3, 1, 5, 4.0, 2.0)]


def floors(npix, C_, r):
    taps = (2 * r + 1) ** 2 - 1
    hbm, lds, ops = npix * (12.0 * C_ + 3), npix * taps * 4.0 * C_, npix * taps * (14.0 + 2 * C_)
    return dict(hbm_bytes=hbm, lds_bytes=lds, lane_ops=ops, hbm_floor_us=hbm / PEAK_HBM * 1e6, lds_floor_us=lds / PEAK_LDS * 1e6,
                valu_floor_us=ops / PEAK_LANE_OPS * 1e6)


def run(name, N, H, W, calls, warmup):
    import torch
    from fcn8s_tensorflow_amd import crf
    from fcn8s_tensorflow_amd.engine import Engine
    e = Engine(20, device_id=0, precision="fp32", seed=0)
    e.freeze(True)
    img = torch.as_tensor(np.stack([crf.synthetic_scene(H, W, 20, seed=n)[1] for n in range(N)])).cuda()
    out = []
    for r, d in WINDOWS:
        p = crf.Params(iterations=ITERATIONS, radius=r, dilation=d)
        plain = lambda: e.predict_tta(img, scales=(1.0,), argmax=True)
        refined = lambda: e.predict_crf(img, p, scales=(1.0,), argmax=True)
        for _ in range(warmup):
            plain(); refined()
        torch.cuda.synchronize()
        a0 = e.get_option("workspace_allocations")
        tp, tc = [], []
        for _ in range(calls):                     # alternating: both see the same clocks and the same neighbours on the machine
            for fn, ts in ((plain, tp), (refined, tc)):
                t0 = time.perf_counter()
                fn()
                torch.cuda.synchronize()
                ts.append(time.perf_counter() - t0)
        a1 = e.get_option("workspace_allocations")
        e.profile(True); e.profile_reset()
        for _ in range(3):
            refined()
        torch.cuda.synchronize()
        g = e.profile_results().get("crf_meanfield", dict(ms=0.0, launches=0, bytes=0.0))
        e.profile(False)
        ms_it = g["ms"] / max(g["launches"], 1)
        fl = floors(N * H * W, 20, r)
        top = max(fl["hbm_floor_us"], fl["lds_floor_us"], fl["valu_floor_us"])
        rec = dict(case=name, precision="fp32", iterations=ITERATIONS, radius=r, dilation=d,
                   predict_tta_ms_median=round(float(np.median(tp)) * 1e3, 3), predict_crf_ms_median=round(float(np.median(tc)) * 1e3, 3),
                   crf_added_ms=round(float(np.median(tc) - np.median(tp)) * 1e3, 3), crf_meanfield_ms_per_iteration=round(ms_it, 4),
                   launches_per_call=g["launches"] // 3, profiled_bytes_per_iteration=g["bytes"] / max(g["launches"], 1),
                   largest_floor_us=round(top, 2), share_of_largest_floor=round(top / (ms_it * 1e3), 3) if ms_it else None,
                   workspace_allocations_before=a0, workspace_allocations_after=a1)
        rec.update({k: (round(v, 2) if k.endswith("_us") else v) for k, v in fl.items()})
        print(json.dumps(rec), flush=True)
        out.append(rec)
    e.close()
    return out


def distances():
    import torch
    from fcn8s_tensorflow_amd import _lib as L, crf
    out = []
    for H, W, C_, r, d, T, wa, ws in DISTANCE_CASES:
        prob, img, _ = crf.synthetic_scene(H, W, C_, seed=H + W)
        p = crf.validate(crf.Params(iterations=T, radius=r, dilation=d, w_appearance=wa, w_smooth=ws))
        cp = L.CrfParams(**p.as_dict())
        dp, di = torch.as_tensor(prob[None]).cuda(), torch.as_tensor(img[None]).cuda()
        work = torch.empty(int(L.lib.fcn8s_op_crf_work_floats(1, H, W, C_, C.byref(cp))), dtype=torch.float32, device="cuda")
        q = torch.empty_like(dp)
        L.check(L.lib.fcn8s_op_crf_meanfield(None, C.c_void_p(dp.data_ptr()), C.c_void_p(di.data_ptr()), 1, H, W, C_, C.byref(cp),
                                             C.c_void_p(work.data_ptr()), C.c_void_p(q.data_ptr()), None))
        torch.cuda.synchronize()
        ref = crf.meanfield(prob, img, p, np.float64)
        d32 = float(np.abs(crf.meanfield(prob, img, p, np.float32) - ref).max())
        dist = float(np.abs(q.cpu().numpy()[0] - ref).max())
        rec = dict(record="device_distance", H=H, W=W, C=C_, radius=r, dilation=d, iterations=T, w_appearance=wa, w_smooth=ws,
                   device_distance=dist, d32=d32, gate=8 * max(d32, 2.0 ** -23), distance_over_d32=round(dist / max(d32, 2.0 ** -23), 3),
                   argmax_changed_by_crf=round(float((ref.argmax(-1) != prob.argmax(-1)).mean()), 4))
        print(json.dumps(rec), flush=True)
        out.append(rec)
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__)
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--distances", action="store_true")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    lines = []
    for name, N, H, W in CASES:
        lines += run(name, N, H, W, a.calls, a.warmup)
    if a.distances:
        lines += distances()
    if a.out:
        with open(a.out, "w") as f:
            for r in lines:
                f.write(json.dumps(r) + "\n")


if __name__ == "__main__":
    main()
