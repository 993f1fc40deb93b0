#!/usr/bin/env python3
"""The pseudo-label kernel (fcn8s_op_pseudo_label) against a copy of its bytes, and what the two sweeps of class-balanced pseudo-labelling cost
next to evaluate_reliability.

Op leg, per shape (16 x 1024x512, 1 x 2048x1024), 20 classes, and two inputs (tools/reliability_bench.py's): uniform (confidences uniform in
[1/C, 1): every block meets far more (class, bin) keys than its 2048 LDS slots hold) and trained (confidences concentrated above 0.95), in
three modes:
  fit          tables only, with the histogram, no labels       reads 4 C bytes per pixel                       (80)
  export       labels, no histogram                             reads 4 C, writes 1                             (81)
  export_full  labels, no histogram, base map and score gate    reads 4 C + 1 + 4, writes 1                     (86)
each next to a same-process device-to-device copy of its algorithmic bytes (half of them read, half written).  Inputs rotate through more sets
than 2 x the 256 MiB Infinity Cache holds.  Alternating blocks, device events around --kreps launches.  Every record holds ratio_to_copy
against the 1.25 x the project's streaming kernels aim at and the copy's own rate (reported, not asserted).

End-to-end leg, the full-width fp32 model, frozen, over --images synthetic 2048x1024 PNGs (and label maps for evaluate_reliability) in a
temporary directory: FCN8s.fit_pseudo_label_thresholds and FCN8s.predict_and_export_pseudo_labels next to FCN8s.evaluate_reliability on the
same single-pass route and files, alternating blocks, wall clock per image.  Condition row: one fit sweep costs no more per image than
evaluate_reliability plus the spread of its blocks (the op replaces reliability_pair and no ground truth is uploaded); printed true or false.
Prints one JSON line per record and writes them to --out if given."""
import argparse
import contextlib
import ctypes as C
import io
import json
import os
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from cityscapes_eval_bench import CACHE_BYTES, PEAK_HBM, SHAPES, timed  # noqa: E402
from reliability_bench import make_inputs  # noqa: E402

NC = 20
BAR = 1.25
MODES = (("fit", 4 * NC), ("export", 4 * NC + 1), ("export_full", 4 * NC + 6))


def op_leg(shapes, warmup, reps, blocks, modes):
    import torch
    from fcn8s_tensorflow_amd import _lib as L, pseudo_label as PL
    lib = L.lib
    ptr = lambda t: C.c_void_p(t.data_ptr()) if t is not None else None
    out = []
    for name, n, h, w in shapes:
        npix = n * h * w
        nsets = max(2, -(-2 * CACHE_BYTES // (4 * NC * npix)) + 1)
        assert nsets * 4 * NC * npix > 2 * CACHE_BYTES
        for kind in ("uniform", "trained"):
            sets = []
            for s in range(nsets):
                prob, gt, scores = make_inputs(kind, npix, 1, 100 * s)
                base = torch.where(torch.rand(npix, device="cuda") < 0.5, torch.full_like(gt, 255), gt % NC)      # about half the pixels to fill
                sets.append((prob, base, scores[0]))
            score_max = float(torch.median(sets[0][2]))                    # the gate drops about half of the examined pixels
            thr = torch.full((NC,), 0.5 if kind == "uniform" else 0.97, dtype=torch.float32, device="cuda")
            labels = torch.empty(npix, dtype=torch.uint8, device="cuda")
            tabs = PL.new_tables_device(NC, "cuda")
            for mode, per_px in MODES:
                if mode not in modes:
                    continue
                by = per_px * npix
                hist = tabs["hist"] if mode == "fit" else None
                lab = None if mode == "fit" else labels
                full = mode == "export_full"
                args = [(None, ptr(p), n, h * w, NC, ptr(thr), None, 255, ptr(b) if full else None, 255, ptr(sc) if full else None,
                         score_max if full else 0.0, ptr(lab), ptr(hist), ptr(tabs["counts"]), ptr(tabs["misc"])) for p, b, sc in sets]
                half = by // 2 // 16 * 16
                src = [torch.empty(half, dtype=torch.uint8, device="cuda") for _ in range(max(2, -(-2 * CACHE_BYTES // half) + 1))]
                dst = torch.empty(half, dtype=torch.uint8, device="cuda")
                rcs = []

                def kern(k):
                    rcs.append(lib.fcn8s_op_pseudo_label(*args[k % nsets]))

                def copy(k):
                    dst.copy_(src[k % len(src)])

                tk, tc = [], []
                for _ in range(blocks):
                    tk.append(timed(kern, 1 << 30, warmup, reps)); tc.append(timed(copy, 1 << 30, warmup, reps))
                torch.cuda.synchronize()
                assert not any(rcs), L.lib.fcn8s_last_error(None)
                k_us, c_us = float(np.median(tk)), float(np.median(tc))
                rec = dict(leg="op", op="pseudo_label", mode=mode, input=kind, shape=name, classes=NC, input_sets=nsets, reps=reps, blocks=blocks,
                           bytes_per_pixel=per_px, bytes_needed=by, op_us=round(k_us, 2), op_us_min_max=[round(min(tk), 2), round(max(tk), 2)],
                           copy_us=round(c_us, 2), copy_us_min_max=[round(min(tc), 2), round(max(tc), 2)], copy_bytes=2 * half,
                           copy_TBps=round(2 * half / c_us * 1e-6, 3), ratio_to_copy=round(k_us / c_us, 3), within_bar=bool(k_us / c_us <= BAR), bar=BAR,
                           op_TBps=round(by / k_us * 1e-6, 3), fraction_of_hbm_8TBps=round(by / (k_us * 1e-6) / PEAK_HBM, 4))
                print(json.dumps(rec), flush=True)
                out.append(rec)
                del src, dst
                torch.cuda.empty_cache()
            assert int(tabs["counts"].sum()) > 0
            del sets, tabs, labels
            torch.cuda.empty_cache()
    return out


def e2e_leg(nimages, warmup, blocks):
    import torch
    from PIL import Image
    from fcn8s_tensorflow_amd.fcn8s import FCN8s
    H, W = 1024, 2048
    rng = np.random.default_rng(0)
    with tempfile.TemporaryDirectory() as root:
        img_dir, gt_dir = os.path.join(root, "leftImg8bit", "val", "city"), os.path.join(root, "gtFine", "val", "city")
        os.makedirs(img_dir); os.makedirs(gt_dir)
        for i in range(nimages):                                           # blocky images and label maps: PNGs of a realistic size
            img = np.kron(rng.integers(0, 256, (H // 32, W // 32, 3), dtype=np.uint8), np.ones((32, 32, 1), np.uint8))
            img = (img.astype(np.int16) + rng.integers(-8, 9, img.shape)).clip(0, 255).astype(np.uint8)
            gt = np.kron(rng.integers(0, 34, (H // 64, W // 64), dtype=np.uint8), np.ones((64, 64), np.uint8))
            Image.fromarray(img).save(os.path.join(img_dir, "city_%06d_000019_leftImg8bit.png" % i))
            Image.fromarray(gt).save(os.path.join(gt_dir, "city_%06d_000019_gtFine_labelIds.png" % i))
        search = os.path.join(root, "gtFine", "val", "*", "*_gtFine_labelIds.png")
        images_dir = os.path.join(root, "leftImg8bit", "val")
        results_dir = os.path.join(root, "pseudo")
        m = FCN8s(vgg16_dir='synthetic:0', num_classes=NC)

        def wall(fn):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            with contextlib.redirect_stdout(io.StringIO()):
                fn()
            torch.cuda.synchronize()
            return (time.perf_counter() - t0) * 1e3 / nimages

        evaluate = lambda: m.evaluate_reliability(images_dir, search)
        fit = lambda: m.fit_pseudo_label_thresholds(images_dir, portion=0.2)
        export = lambda: m.predict_and_export_pseudo_labels(results_dir, images_dir)
        for _ in range(max(1, warmup)):
            wall(evaluate); wall(fit); wall(export)
        ta, tb, tc = [], [], []
        for _ in range(blocks):
            ta.append(wall(evaluate)); tb.append(wall(fit)); tc.append(wall(export))
        m.close()
    a_ms, b_ms, c_ms = float(np.median(ta)), float(np.median(tb)), float(np.median(tc))
    spread = max(ta) - min(ta)
    common = dict(leg="e2e", route="single", shape="1x2048x1024", precision="fp32", images=nimages, blocks=blocks)
    recs = [dict(common, state="evaluate_reliability", ms_per_image=round(a_ms, 3), block_spread_ms=round(spread, 3)),
            dict(common, state="fit_pseudo_label_thresholds", ms_per_image=round(b_ms, 3), block_spread_ms=round(max(tb) - min(tb), 3)),
            dict(common, state="predict_and_export_pseudo_labels", ms_per_image=round(c_ms, 3), block_spread_ms=round(max(tc) - min(tc), 3)),
            dict(leg="e2e_condition", shape="1x2048x1024", precision="fp32", fit_ms_per_image=round(b_ms, 3), evaluate_ms_per_image=round(a_ms, 3),
                 spread_evaluate_ms=round(spread, 3), fit_within_evaluate_plus_spread=bool(b_ms <= a_ms + spread))]
    for r in recs:
        print(json.dumps(r), flush=True)
    return recs


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--kreps", type=int, default=10, help="launches per block of the op leg")
    ap.add_argument("--kblocks", type=int, default=10, help="alternating blocks of the op leg")
    ap.add_argument("--images", type=int, default=4, help="PNGs of the end-to-end leg")
    ap.add_argument("--blocks", type=int, default=5, help="alternating blocks of the end-to-end leg")
    ap.add_argument("--legs", default="op,e2e")
    ap.add_argument("--modes", default="fit,export,export_full", help="modes of the op leg")
    ap.add_argument("--out")
    a = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("pseudo_label_bench.py measures on an MI355X; no GPU here")
    recs = []
    legs = a.legs.split(",")
    if "op" in legs:
        recs += op_leg([SHAPES[0], SHAPES[2]], a.warmup, a.kreps, a.kblocks, a.modes.split(","))
        torch.cuda.empty_cache()
    if "e2e" in legs:
        recs += e2e_leg(a.images, a.warmup, a.blocks)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            for r in recs:
                f.write(json.dumps(r) + "\n")


if __name__ == "__main__":
    main()
