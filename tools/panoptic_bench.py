#!/usr/bin/env python3
"""The segment pair table of panoptic quality (fcn8s_op_panoptic_pair) against a copy of its algorithmic bytes and against
fcn8s_op_cityscapes_pair in the same process, and what `evaluate_cityscapes(panoptic=4)` costs next to `evaluate_cityscapes`.

Op leg, per shape (16 x 1024x512, 1 x 2048x1024) and input, int64 predictions as `predict` writes them, components from
fcn8s_op_regions_label (connectivity 4) computed outside the timed region:
  cityscapes_like   the label / instance maps of tools/cityscapes_eval_bench.py (blocks of 64 with 40 rectangles), its damaged train ids
  salted            the same with 5 % of the pixels set to a random class: thousands of one-pixel thing segments per image
  constant          one class, one instance value: every pixel goes to one pair
14 bytes per pixel are read (2 instance map, 8 prediction, 4 components).  Next to it: a same-process device-to-device copy of those bytes
(half read, half written), fcn8s_op_cityscapes_pair on the same label / instance / prediction maps (11 bytes per pixel), and
fcn8s_op_regions_label alone.  Inputs rotate through more sets than 2 x the 256 MiB Infinity Cache holds.  Alternating blocks; per block
the median over --reps calls, each between its own pair of device events.  No bar is set: a hash insert is not a streaming kernel; the
ratios are recorded.

End-to-end leg, the full-width fp32 model, frozen, --images synthetic 2048x1024 PNG triples: `evaluate_cityscapes(panoptic=4)` next to
`evaluate_cityscapes`, alternating blocks, wall clock per image.  Condition row: t(with panoptic) <= t(without) + t(label) + t(pair op)
+ the spread of the "without" blocks, label and pair op timed alone on one of the run's own argmax maps; printed true or false.
Prints one JSON line per record and writes them to --out if given."""
import argparse
import ctypes as C
import json
import os
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from cityscapes_eval_bench import CACHE_BYTES, PEAK_HBM, SHAPES, make_maps  # noqa: E402
from regions_bench import per_call_us  # noqa: E402


def make_input(kind, N, H, W):
    """(gt uint8, inst uint16, train int64), each [N, H, W]"""
    gt, inst, train = (a.reshape(N, H, W) for a in make_maps(N, H, W, "cityscapes_like", seed=N + H))
    if kind == "salted":
        rng = np.random.default_rng(H)
        m = rng.random(train.shape) < 0.05
        train = train.copy(); train[m] = rng.integers(0, 20, int(m.sum()))
    elif kind == "constant":
        gt = np.full_like(gt, 26); inst = np.full_like(inst, 26001); train = np.full_like(train, 14)
    return gt, inst, train


def op_leg(shapes, warmup, reps, blocks):
    import torch
    from fcn8s_tensorflow_amd import _lib as L, panoptic as PQ, regions as R
    lib = L.lib
    ptr = lambda t: C.c_void_p(t.data_ptr())
    out = []
    for name, N, H, W in shapes:
        npix, P = N * H * W, H * W
        by = 14 * npix
        nsets = max(2, -(-2 * CACHE_BYTES // by) + 1)
        assert nsets * by > 2 * CACHE_BYTES
        rwork = torch.empty(256, dtype=torch.uint8, device="cuda")
        for kind in ("cityscapes_like", "salted", "constant"):
            gt, inst, train = make_input(kind, N, H, W)
            sets = []
            for s in range(nsets):                                     # rolled copies: the same statistics in distinct memory
                sh = (37 * s, 91 * s)
                g = torch.from_numpy(np.roll(gt, sh, (1, 2))).cuda(); i = torch.from_numpy(np.roll(inst, sh, (1, 2)).view(np.int16)).cuda()
                p = torch.from_numpy(np.roll(train, sh, (1, 2))).cuda()
                comp, _a, rwork = R.label_device(p, connectivity=4, area=False, work=rwork)
                sets.append((g, i, p, comp))
            # room found by the route callers take: pair_rows_device's retries on the first set
            rows0, _bad, w = PQ.pair_rows_device(sets[0][2], sets[0][1], connectivity=4)
            found = max(len(r) for r in rows0)
            slots = w["slots"]
            max_rows = max(PQ.DEFAULT_MAX_ROWS, 2 * found)
            table = torch.empty(lib.fcn8s_op_panoptic_work_bytes(N, slots), dtype=torch.uint8, device="cuda")
            rows = torch.empty((N, max_rows, 3), dtype=torch.int64, device="cuda")
            counts = torch.empty((N, 4), dtype=torch.int64, device="cuda")
            comp_out = torch.empty((N, H, W), dtype=torch.int32, device="cuda")
            conf = torch.zeros(34 * 34, dtype=torch.int64, device="cuda"); ccounts = torch.zeros((N, 3), dtype=torch.int64, device="cuda")
            cwork = torch.empty(lib.fcn8s_op_cityscapes_work_bytes(N), dtype=torch.uint8, device="cuda")
            entries = torch.empty((N, 2048, 4), dtype=torch.int32, device="cuda")
            half = by // 2
            src = [torch.empty(half, dtype=torch.uint8, device="cuda") for _ in range(max(2, -(-2 * CACHE_BYTES // half) + 1))]
            dst = torch.empty(half, dtype=torch.uint8, device="cuda")
            rcs = []
            fns = dict(
                pair=lambda k: rcs.append(lib.fcn8s_op_panoptic_pair(None, ptr(sets[k][1]), ptr(sets[k][2]), 0, ptr(sets[k][3]), N, H, W, ptr(table), slots,
                                                                     ptr(rows), max_rows, ptr(counts))),
                copy=lambda k: dst.copy_(src[k % len(src)]),
                cityscapes_pair=lambda k: rcs.append(lib.fcn8s_op_cityscapes_pair(None, ptr(sets[k][0]), ptr(sets[k][1]), ptr(sets[k][2]), 0, N, P, ptr(conf),
                                                                                  ptr(cwork), ptr(entries), 2048, ptr(ccounts))),
                label=lambda k: rcs.append(lib.fcn8s_op_regions_label(None, ptr(sets[k][2]), 0, N, H, W, 4, ptr(comp_out), None, ptr(rwork))))
            t = {k: [] for k in fns}
            for _ in range(blocks):
                for k, fn in fns.items():
                    t[k].append(per_call_us(fn, lambda _k: None, nsets, warmup, reps))
            torch.cuda.synchronize()
            assert not any(rcs), lib.fcn8s_last_error(None)
            cnt = counts.cpu().numpy()
            assert not cnt[:, 2].any() and (cnt[:, 1] + cnt[:, 3] == P).all() and int(cnt[:, 0].max()) <= max_rows, cnt.tolist()
            med = {k: float(np.median(v)) for k, v in t.items()}
            rec = dict(leg="op", input=kind, shape=name, input_sets=nsets, reps=reps, blocks=blocks, bytes_read=by, slots_per_image=slots,
                       table_bytes=int(table.numel()), rows_per_image_max=int(cnt[:, 0].max()),
                       pair_us=round(med["pair"], 2), pair_us_min_max=[round(min(t["pair"]), 2), round(max(t["pair"]), 2)],
                       copy_us=round(med["copy"], 2), copy_us_min_max=[round(min(t["copy"]), 2), round(max(t["copy"]), 2)], copy_bytes=2 * half,
                       cityscapes_pair_us=round(med["cityscapes_pair"], 2), regions_label_us=round(med["label"], 2),
                       ratio_to_copy=round(med["pair"] / med["copy"], 3), ratio_to_cityscapes_pair=round(med["pair"] / med["cityscapes_pair"], 3),
                       ns_per_pixel=round(med["pair"] * 1e3 / npix, 4), fraction_of_hbm_8TBps=round(by / (med["pair"] * 1e-6) / PEAK_HBM, 4))
            print(json.dumps(rec), flush=True)
            out.append(rec)
            del sets, src, dst, table, rows
            torch.cuda.empty_cache()
    return out


def e2e_leg(nimg, reps, blocks):
    import torch
    from PIL import Image
    from fcn8s_tensorflow_amd import panoptic as PQ, regions as R
    from fcn8s_tensorflow_amd.cityscapes_eval import instance_map_tensor
    from fcn8s_tensorflow_amd.fcn8s import FCN8s
    H, W = 1024, 2048
    m = FCN8s(vgg16_dir='synthetic:0', num_classes=20)
    rng = np.random.default_rng(0)
    with tempfile.TemporaryDirectory() as d:
        gt, inst, _ = make_maps(nimg, H, W, "cityscapes_like", seed=1)
        for n in range(nimg):
            os.makedirs(os.path.join(d, "leftImg8bit", "city"), exist_ok=True); os.makedirs(os.path.join(d, "gtFine", "city"), exist_ok=True)
            img = (np.kron(rng.integers(0, 256, (H // 16, W // 16, 3)), np.ones((16, 16, 1), np.int64)) // 2 + rng.integers(0, 32, (H, W, 3))).astype(np.uint8)
            stem = "city_%06d_000019" % n
            Image.fromarray(img).save(os.path.join(d, "leftImg8bit", "city", stem + "_leftImg8bit.png"))
            Image.fromarray(gt[n].reshape(H, W)).save(os.path.join(d, "gtFine", "city", stem + "_gtFine_labelIds.png"))
            Image.fromarray(inst[n].reshape(H, W)).save(os.path.join(d, "gtFine", "city", stem + "_gtFine_instanceIds.png"))
        search, images = os.path.join(d, "gtFine", "*", "*_gtFine_labelIds.png"), os.path.join(d, "leftImg8bit")

        def wall(**kw):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(reps):
                res = m.evaluate_cityscapes(images, search, **kw)
            torch.cuda.synchronize()
            return (time.perf_counter() - t0) * 1e3 / (reps * nimg), res
        wall(); wall(panoptic=4)                                       # warm-up: workspaces, code objects
        ta, tb = [], []
        for _ in range(blocks):
            ta.append(wall()[0]); t, res = wall(panoptic=4); tb.append(t)
        pred = m.predict(torch.from_numpy(img[None]).to(m.engine.device))
        it = instance_map_tensor(inst[nimg - 1].reshape(1, H, W), pred.device)
        comp, _a, rwork = R.label_device(pred, connectivity=4, area=False)
        rows, _bad, w = PQ.pair_rows_device(pred, it, connectivity=4)
        slots = w["slots"]
        # what the condition's right-hand side leaves out: the host's half (download and sort of the rows, the float64 scores)
        torch.cuda.synchronize(); t0 = time.perf_counter()
        for _ in range(3):
            rows, _bad, w = PQ.pair_rows_device(pred, it, connectivity=4, work=w)
        host_rows_ms = (time.perf_counter() - t0) * 1e3 / 3
        t0 = time.perf_counter()
        for _ in range(3):
            PQ.stats_add(PQ.new_stats(), rows[0])
        host_scores_ms = (time.perf_counter() - t0) * 1e3 / 3
        label_us = float(np.median([per_call_us(lambda k: R.label_device(pred, connectivity=4, area=False, work=rwork), lambda k: None, 1, 2, 10) for _ in range(5)]))
        pair_us = float(np.median([per_call_us(lambda k: PQ.raw_pair_device(pred, it, comp, slots, w["max_rows"], table=w["table"], rows=w["rows"]),
                                               lambda k: None, 1, 2, 10) for _ in range(5)]))
    m.close()
    a_ms, b_ms = float(np.median(ta)), float(np.median(tb))
    spread = max(ta) - min(ta)
    allowed = a_ms + (label_us + pair_us) * 1e-3 + spread
    recs = [dict(leg="e2e", state="evaluate_cityscapes", images=nimg, shape="2048x1024", precision="fp32", reps=reps, blocks=blocks,
                 ms_per_image=round(a_ms, 3), block_spread_ms=round(spread, 3)),
            dict(leg="e2e", state="evaluate_cityscapes_panoptic_4", images=nimg, shape="2048x1024", precision="fp32", reps=reps, blocks=blocks,
                 ms_per_image=round(b_ms, 3), block_spread_ms=round(max(tb) - min(tb), 3), rows_last_image=len(rows[0]),
                 panoptic_quality=res["panopticQuality"], fp_total=int(res["panopticFp"].sum())),
            dict(leg="e2e_condition", shape="2048x1024", precision="fp32", without_ms=round(a_ms, 3), with_panoptic_ms=round(b_ms, 3),
                 label_alone_ms=round(label_us * 1e-3, 4), pair_alone_ms=round(pair_us * 1e-3, 4), spread_without_ms=round(spread, 3),
                 allowed_ms=round(allowed, 3), with_panoptic_within_without_plus_label_plus_pair_plus_spread=bool(b_ms <= allowed),
                 rows_last_image=len(rows[0]), pair_rows_device_whole_call_ms=round(host_rows_ms, 3), stats_add_ms=round(host_scores_ms, 3))]
    for r in recs:
        print(json.dumps(r), flush=True)
    return recs


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--reps", type=int, default=10, help="calls per block")
    ap.add_argument("--blocks", type=int, default=5, help="alternating blocks")
    ap.add_argument("--images", type=int, default=4, help="PNG triples of the end-to-end leg")
    ap.add_argument("--e2e-reps", type=int, default=2, help="directory evaluations per block of the end-to-end leg")
    ap.add_argument("--legs", default="op,e2e")
    ap.add_argument("--out")
    a = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("panoptic_bench.py measures on an MI355X; no GPU here")
    recs = []
    legs = a.legs.split(",")
    if "op" in legs:
        recs += op_leg([SHAPES[0], SHAPES[2]], a.warmup, a.reps, a.blocks)
        torch.cuda.empty_cache()
    if "e2e" in legs:
        recs += e2e_leg(a.images, a.e2e_reps, a.blocks)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            for r in recs:
                f.write(json.dumps(r) + "\n")


if __name__ == "__main__":
    main()
