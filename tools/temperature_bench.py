#!/usr/bin/env python3
"""The temperature-scaling kernels (fcn8s_op_temperature_nll, fcn8s_op_temperature_apply) against a copy of their bytes and against
fcn8s_op_reliability_pair, and what one fit_temperature sweep costs next to evaluate_reliability.

Op leg, per shape (16 x 1024x512, 1 x 2048x1024), 20 classes, and two inputs (tools/reliability_bench.py's): uniform (confidences uniform in
[1/C, 1)) and trained (confidences concentrated above 0.95):
  temperature_nll at K = 1, 8, 32          reads (4 C + 1) bytes per pixel
  temperature_apply in place, without and with the entropy map   reads 4 C, writes 4 C (+ 4) bytes per pixel
  reliability_pair with no uncertainty map (J = 0)               reads (4 C + 1) bytes per pixel
each next to a same-process device-to-device copy of its algorithmic bytes (half of them read, half written).  Inputs rotate through more sets
than 2 x the 256 MiB Infinity Cache holds.  Alternating blocks, device events around --kreps launches.  K = 1 and the two apply forms record
ratio_to_copy against the 1.25 x the project's streaming kernels aim at (reported, not asserted); K = 32 records the time per (pixel x
candidate) and its ratio to the issue-count estimate: per 64 pixels and candidate C x (4 + 8 + 4) cycles of one SIMD, 1024 SIMDs at 2.4 GHz.

End-to-end leg, the full-width fp32 model, frozen, over --images synthetic 2048x1024 PNG pairs in a temporary directory: one sweep of
FCN8s.fit_temperature (passes=1, 32 candidates) next to FCN8s.evaluate_reliability on the same single-pass route and files, alternating blocks,
wall clock per image.  Condition row: the difference is no larger than t(temperature_nll, K = 32) - t(reliability_pair, J = 0) at this shape on
the route's own softmax, plus the spread of the evaluate_reliability blocks; printed true or false.
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
EST_CYCLES = NC * (4 + 8 + 4)            # per 64 pixels and candidate on one SIMD: multiply, v_exp_f32, add per class
SIMDS, CLOCK = 1024, 2.4e9


def grid_betas(K):
    from fcn8s_tensorflow_amd import temperature as ts
    return np.array([1.0], np.float32) if K == 1 else ts.betas_of(ts.candidate_grid(0.125, 8.0, K))


def op_leg(shapes, warmup, reps, blocks):
    import torch
    from fcn8s_tensorflow_amd import _lib as L, reliability as rel
    lib = L.lib
    ptr = lambda t: C.c_void_p(t.data_ptr())
    lut = torch.from_numpy(rel.identity_lut()).cuda()
    out = []
    for name, n, h, w in shapes:
        npix = n * h * w
        by_read = (4 * NC + 1) * npix
        nsets = max(2, -(-2 * CACHE_BYTES // by_read) + 1)
        assert nsets * by_read > 2 * CACHE_BYTES
        for kind in ("uniform", "trained"):
            sets = [make_inputs(kind, npix, 0, 100 * s)[:2] for s in range(nsets)]
            rtab = rel.new_tables_device(15, 0, "cuda")
            kernels = []                                                  # (record fields, bytes, launch(k))
            for K in (1, 8, 32):
                b = grid_betas(K)
                tab = torch.zeros(K + 3, dtype=torch.int64, device="cuda")
                args = [(None, ptr(p), ptr(g), ptr(lut), n, h * w, NC, b.ctypes.data_as(L._fp), K, C.c_void_p(tab.data_ptr()),
                         C.c_void_p(tab.data_ptr() + 8 * K), C.c_void_p(tab.data_ptr() + 8 * K + 8)) for p, g in sets]
                kernels.append((dict(op="temperature_nll", candidates=K), by_read, lib.fcn8s_op_temperature_nll, args, (b, tab)))
            args = [(None, ptr(p), ptr(g), ptr(lut), n, h * w, NC, None, None, 0, 15) + tuple(ptr(t) for t in rtab) for p, g in sets]
            kernels.append((dict(op="reliability_pair", scores=0), by_read, lib.fcn8s_op_reliability_pair, args, None))
            ent = torch.empty(npix, dtype=torch.float32, device="cuda")
            for with_ent in (False, True):                                # in place: after the first launch the inputs are calibrated rows, still rows
                args = [(None, ptr(p), n, h * w, NC, 0.8, ptr(p), ptr(ent) if with_ent else None) for p, _ in sets]
                kernels.append((dict(op="temperature_apply", in_place=True, entropy=with_ent), (8 * NC + (4 if with_ent else 0)) * npix,
                                lib.fcn8s_op_temperature_apply, args, None))
            for fields, by, fn, args, keep in kernels:
                half = by // 2 // 16 * 16
                src = [torch.empty(half, dtype=torch.uint8, device="cuda") for _ in range(max(2, -(-2 * CACHE_BYTES // half) + 1))]
                dst = torch.empty(half, dtype=torch.uint8, device="cuda")
                rcs = []

                def kern(k):
                    rcs.append(fn(*args[k % nsets]))

                def copy(k):
                    dst.copy_(src[k % len(src)])

                tk, tc = [], []
                for _ in range(blocks):
                    tk.append(timed(kern, 1 << 30, warmup, reps)); tc.append(timed(copy, 1 << 30, warmup, reps))
                torch.cuda.synchronize()
                assert not any(rcs), L.lib.fcn8s_last_error(None)
                k_us, c_us = float(np.median(tk)), float(np.median(tc))
                rec = dict(leg="op", input=kind, shape=name, classes=NC, **fields, input_sets=nsets, reps=reps, blocks=blocks, bytes_needed=by,
                           op_us=round(k_us, 2), op_us_min_max=[round(min(tk), 2), round(max(tk), 2)],
                           copy_us=round(c_us, 2), copy_us_min_max=[round(min(tc), 2), round(max(tc), 2)], copy_bytes=2 * half,
                           ratio_to_copy=round(k_us / c_us, 3), within_bar=bool(k_us / c_us <= BAR), bar=BAR,
                           op_TBps=round(by / k_us * 1e-6, 3), fraction_of_hbm_8TBps=round(by / (k_us * 1e-6) / PEAK_HBM, 4))
                if fields["op"] == "temperature_nll":
                    K = fields["candidates"]
                    est_us = npix * K / 64.0 * EST_CYCLES / SIMDS / CLOCK * 1e6
                    rec.update(ps_per_pixel_candidate=round(k_us * 1e6 / (npix * K), 3), issue_estimate_us=round(est_us, 2),
                               ratio_to_issue_estimate=round(k_us / est_us, 3))
                    assert int(keep[1][K]) > 0 and not bool(keep[1][K + 1:].any())
                print(json.dumps(rec), flush=True)
                out.append(rec)
                del src, dst
                torch.cuda.empty_cache()
            del sets, kernels, rtab
            torch.cuda.empty_cache()
    return out


def e2e_leg(nimages, warmup, blocks):
    import torch
    from PIL import Image
    from fcn8s_tensorflow_amd import reliability as rel, temperature as ts
    from fcn8s_tensorflow_amd.fcn8s import FCN8s
    H, W = 1024, 2048
    rng = np.random.default_rng(0)
    with tempfile.TemporaryDirectory() as root:
        img_dir, gt_dir = os.path.join(root, "leftImg8bit", "val", "city"), os.path.join(root, "gtFine", "val", "city")
        os.makedirs(img_dir); os.makedirs(gt_dir)
        imgs, gts = [], []
        for i in range(nimages):                                           # blocky images and label maps: PNGs of a realistic size
            img = np.kron(rng.integers(0, 256, (H // 32, W // 32, 3), dtype=np.uint8), np.ones((32, 32, 1), np.uint8))
            img = (img.astype(np.int16) + rng.integers(-8, 9, img.shape)).clip(0, 255).astype(np.uint8)
            gt = np.kron(rng.integers(0, 34, (H // 64, W // 64), dtype=np.uint8), np.ones((64, 64), np.uint8))
            imgs.append(os.path.join(img_dir, "city_%06d_000019_leftImg8bit.png" % i)); gts.append(os.path.join(gt_dir, "city_%06d_000019_gtFine_labelIds.png" % i))
            Image.fromarray(img).save(imgs[-1]); Image.fromarray(gt).save(gts[-1])
        search = os.path.join(root, "gtFine", "val", "*", "*_gtFine_labelIds.png")
        images_dir = os.path.join(root, "leftImg8bit", "val")
        m = FCN8s(vgg16_dir='synthetic:0', num_classes=NC)
        e = m.engine
        dev = e.device

        def wall(fn):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            with contextlib.redirect_stdout(io.StringIO()):
                fn()
            torch.cuda.synchronize()
            return (time.perf_counter() - t0) * 1e3 / nimages

        evaluate = lambda: m.evaluate_reliability(images_dir, search)
        fit = lambda: m.fit_temperature(images_dir, search, passes=1, candidates=32)
        for _ in range(max(1, warmup)):
            wall(evaluate); wall(fit)
        ta, tb = [], []
        for _ in range(blocks):
            ta.append(wall(evaluate)); tb.append(wall(fit))
        # the parts: both ops at this shape on the route's own softmax
        image = torch.from_numpy(np.array(Image.open(imgs[0]).convert('RGB'))[None]).to(dev)
        prob, ent, _ = e.predict_mc(image, samples=1, keep_prob=1.0, argmax=False, mutual_information=False)
        gt_dev = torch.from_numpy(np.array(Image.open(gts[0])).astype(np.uint8)[None]).to(dev)
        lut = torch.from_numpy(rel.cityscapes_lut()).to(dev)
        rtab = rel.new_tables_device(15, 0, dev)
        betas = grid_betas(32)
        ttab = ts.new_tables_device(32, dev)
        rel_us = float(np.median([timed(lambda k: rel.counts_device(prob, gt_dev, lut, (), (), 15, rtab), 1, 2, 10) for _ in range(5)]))
        nll_us = float(np.median([timed(lambda k: ts.nll_device(prob, gt_dev, lut, betas, ttab), 1, 2, 10) for _ in range(5)]))
        m.close()
    a_ms, b_ms = float(np.median(ta)), float(np.median(tb))
    spread = max(ta) - min(ta)
    added = b_ms - a_ms
    allowed = (nll_us - rel_us) * 1e-3 + spread
    recs = [dict(leg="e2e", state="evaluate_reliability", route="single", shape="1x2048x1024", precision="fp32", images=nimages, blocks=blocks,
                 ms_per_image=round(a_ms, 3), block_spread_ms=round(spread, 3)),
            dict(leg="e2e", state="fit_temperature_one_sweep", route="single", candidates=32, shape="1x2048x1024", precision="fp32", images=nimages, blocks=blocks,
                 ms_per_image=round(b_ms, 3), block_spread_ms=round(max(tb) - min(tb), 3)),
            dict(leg="e2e_condition", shape="1x2048x1024", precision="fp32", added_ms_per_image=round(added, 3), temperature_nll_k32_ms=round(nll_us * 1e-3, 4),
                 reliability_pair_j0_ms=round(rel_us * 1e-3, 4), spread_evaluate_ms=round(spread, 3), allowed_ms=round(allowed, 3),
                 added_within_op_difference_plus_spread=bool(added <= allowed))]
    for r in recs:
        print(json.dumps(r), flush=True)
    return recs


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--kreps", type=int, default=10, help="launches per block of the op leg")
    ap.add_argument("--kblocks", type=int, default=10, help="alternating blocks of the op leg")
    ap.add_argument("--images", type=int, default=4, help="PNG pairs of the end-to-end leg")
    ap.add_argument("--blocks", type=int, default=5, help="alternating blocks of the end-to-end leg")
    ap.add_argument("--legs", default="op,e2e")
    ap.add_argument("--out")
    a = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("temperature_bench.py measures on an MI355X; no GPU here")
    recs = []
    legs = a.legs.split(",")
    if "op" in legs:
        recs += op_leg([SHAPES[0], SHAPES[2]], a.warmup, a.kreps, a.kblocks)
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
