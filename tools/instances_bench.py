#!/usr/bin/env python3
"""The instance pair table of instance-level AP (fcn8s_op_instance_pair) against a copy of its algorithmic bytes and against
fcn8s_op_panoptic_pair in the same process, and what `evaluate_cityscapes_instances` costs next to `evaluate_reliability`.

Op leg, per shape (16 x 1024x512, 1 x 2048x1024) and input; uint8 train ids, components from fcn8s_op_regions_label (connectivity 4)
computed outside the timed region, a softmax of 20 classes made on the device in which the label's column is the maximum:
  cityscapes_like   the label / instance maps of tools/cityscapes_eval_bench.py (blocks of 64 with 40 rectangles), its damaged train ids
  salted            the same with 5 % of the pixels set to a random class: thousands of one-pixel instances per image
  constant          one class, one instance value: every pixel goes to one pair
87 bytes per pixel are read (80 softmax, 1 label, 4 components, 2 instance map).  Next to it: a same-process device-to-device copy of those
bytes (half read, half written) and fcn8s_op_panoptic_pair on the same maps (int64 predictions, 14 bytes per pixel).  Inputs rotate
through more sets than 2 x the 256 MiB Infinity Cache holds.  Alternating blocks; per block the median over --reps calls, each between
its own pair of device events.  The aim on the Cityscapes-like maps at the batch shape is the 1.25 x copy the other streaming kernels are
held to; it is an aim, not a condition (a hash insert sits inside the kernel): the ratios are recorded.

End-to-end leg, the full-width fp32 model, frozen, --images synthetic 2048x1024 images with instance maps: `evaluate_cityscapes_instances`
next to `evaluate_reliability` (the same single-pass route), alternating blocks, wall clock per image; the device calls that the former
adds (pseudo_label, regions_label, instance_pair) and the host half (download and sort of the rows; matching) timed alone on the last
image.  On an untrained model the row count dominates the host half.
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
from panoptic_bench import make_input  # noqa: E402
from regions_bench import per_call_us  # noqa: E402

CLASSES = 20
BYTES_PER_PIXEL = 4 * CLASSES + 1 + 4 + 2


def device_softmax(labels, seed):
    """float32 [N, H, W, 20] on the device: small random columns, the label's column (labels < 20) the maximum, each in [0, 1]"""
    import torch
    g = torch.Generator(device="cuda"); g.manual_seed(seed)
    prob = torch.rand(tuple(labels.shape) + (CLASSES,), generator=g, device="cuda") * 0.02
    top = 0.55 + 0.4 * torch.rand(tuple(labels.shape) + (1,), generator=g, device="cuda")
    prob.scatter_(-1, labels.long().unsqueeze(-1), top)
    return prob


def op_leg(shapes, warmup, reps, blocks):
    import torch
    from fcn8s_tensorflow_amd import _lib as L, instances as INS, panoptic as PQ, regions as R
    lib = L.lib
    ptr = lambda t: C.c_void_p(t.data_ptr())
    out = []
    for name, N, H, W in shapes:
        npix = N * H * W
        by = BYTES_PER_PIXEL * npix
        nsets = max(2, -(-2 * CACHE_BYTES // by) + 1)
        assert nsets * by > 2 * CACHE_BYTES
        rwork = torch.empty(256, dtype=torch.uint8, device="cuda")
        for kind in ("cityscapes_like", "salted", "constant"):
            _gt, inst, train = make_input(kind, N, H, W)
            sets = []
            for s in range(nsets):                                     # rolled copies: the same statistics in distinct memory
                sh = (37 * s, 91 * s)
                i = torch.from_numpy(np.roll(inst, sh, (1, 2)).view(np.int16)).cuda()
                p64 = torch.from_numpy(np.roll(train, sh, (1, 2))).cuda()
                lab = p64.to(torch.uint8)
                comp, _a, rwork = R.label_device(lab, connectivity=4, area=False, work=rwork)
                sets.append((device_softmax(lab, s), lab, comp, i, p64))
            w, found = None, 0
            for st in sets:                                            # room found by the route callers take: its retries, carried from set to set
                rows0, _bad, w = INS.pair_rows_device(*st[:4], work=w)
                found = max(found, max(len(r) for r in rows0))
            slots = w["slots"]
            max_rows = max(INS.DEFAULT_MAX_ROWS, 2 * found)
            table = torch.empty(lib.fcn8s_op_instance_work_bytes(N, slots), dtype=torch.uint8, device="cuda")
            rows = torch.empty((N, max_rows, 4), dtype=torch.int64, device="cuda")
            counts = torch.empty((N, 5), dtype=torch.int64, device="cuda")
            _r, _b, pw = PQ.pair_rows_device(sets[0][4], sets[0][3], connectivity=4)
            pslots, pmax = pw["slots"], max(PQ.DEFAULT_MAX_ROWS, 2 * max(len(r) for r in _r))
            ptable = torch.empty(lib.fcn8s_op_panoptic_work_bytes(N, pslots), dtype=torch.uint8, device="cuda")
            prows = torch.empty((N, pmax, 3), dtype=torch.int64, device="cuda")
            pcounts = torch.empty((N, 4), dtype=torch.int64, device="cuda")
            del w, pw
            half = by // 2
            src = [torch.empty(half, dtype=torch.uint8, device="cuda") for _ in range(max(2, -(-2 * CACHE_BYTES // half) + 1))]
            dst = torch.empty(half, dtype=torch.uint8, device="cuda")
            rcs = []
            fns = dict(
                pair=lambda k: rcs.append(lib.fcn8s_op_instance_pair(None, ptr(sets[k][0]), CLASSES, ptr(sets[k][1]), ptr(sets[k][2]), ptr(sets[k][3]), N, H, W,
                                                                     ptr(table), slots, ptr(rows), max_rows, ptr(counts))),
                copy=lambda k: dst.copy_(src[k % len(src)]),
                panoptic_pair=lambda k: rcs.append(lib.fcn8s_op_panoptic_pair(None, ptr(sets[k][3]), ptr(sets[k][4]), 0, ptr(sets[k][2]), N, H, W, ptr(ptable),
                                                                              pslots, ptr(prows), pmax, ptr(pcounts))))
            t = {k: [] for k in fns}
            for _ in range(blocks):
                for k, fn in fns.items():
                    t[k].append(per_call_us(fn, lambda _k: None, nsets, warmup, reps))
            torch.cuda.synchronize()
            assert not any(rcs), lib.fcn8s_last_error(None)
            cnt = counts.cpu().numpy()
            assert not cnt[:, 2].any() and (cnt[:, 3] == H * W).all() and not cnt[:, [1, 4]].any() and int(cnt[:, 0].max()) <= max_rows, cnt.tolist()
            med = {k: float(np.median(v)) for k, v in t.items()}
            rec = dict(leg="op", input=kind, shape=name, classes=CLASSES, input_sets=nsets, reps=reps, blocks=blocks, bytes_read=by, slots_per_image=slots,
                       table_bytes=int(table.numel()), rows_per_image_max=int(cnt[:, 0].max()),
                       pair_us=round(med["pair"], 2), pair_us_min_max=[round(min(t["pair"]), 2), round(max(t["pair"]), 2)],
                       copy_us=round(med["copy"], 2), copy_us_min_max=[round(min(t["copy"]), 2), round(max(t["copy"]), 2)], copy_bytes=2 * half,
                       panoptic_pair_us=round(med["panoptic_pair"], 2),
                       ratio_to_copy=round(med["pair"] / med["copy"], 3), ratio_to_panoptic_pair=round(med["pair"] / med["panoptic_pair"], 3),
                       aim_ratio_to_copy=1.25, ns_per_pixel=round(med["pair"] * 1e3 / npix, 4),
                       fraction_of_hbm_8TBps=round(by / (med["pair"] * 1e-6) / PEAK_HBM, 4))
            print(json.dumps(rec), flush=True)
            out.append(rec)
            del sets, src, dst, table, rows, ptable, prows
            torch.cuda.empty_cache()
    return out


def e2e_leg(nimg, reps, blocks):
    import torch
    from PIL import Image
    from fcn8s_tensorflow_amd import instances as INS
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
        images = os.path.join(d, "leftImg8bit")
        lab_search, inst_search = os.path.join(d, "gtFine", "*", "*_gtFine_labelIds.png"), os.path.join(d, "gtFine", "*", "*_gtFine_instanceIds.png")

        def wall(fn):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(reps):
                res = fn()
            torch.cuda.synchronize()
            return (time.perf_counter() - t0) * 1e3 / (reps * nimg), res
        rel = lambda: m.evaluate_reliability(images, lab_search)
        ap = lambda: m.evaluate_cityscapes_instances(images, inst_search)
        wall(rel); wall(ap)                                            # warm-up: workspaces, code objects
        ta, tb = [], []
        for _ in range(blocks):
            ta.append(wall(rel)[0]); t, res = wall(ap); tb.append(t)
        # the calls the instance route adds, alone, on the last image
        e = m.engine
        e.freeze(True)
        prob = e.predict_mc(torch.from_numpy(img[None]).to(e.device), samples=1, keep_prob=1.0, sample_offset=0, argmax=False, entropy=False, mutual_information=False)[0]
        e.freeze(False)
        labels, _t = e.pseudo_label(prob, labels=True)
        comp, _a = e.regions_label(labels, connectivity=4, area=False)
        it = inst[nimg - 1].reshape(1, H, W)
        rows, _bad = e.instance_pair(prob, labels, comp, it)
        w = e._instance_work
        from fcn8s_tensorflow_amd.cityscapes_eval import instance_map_tensor
        itd = instance_map_tensor(it, e.device)
        med = lambda fn: float(np.median([per_call_us(fn, lambda k: None, 1, 2, 10) for _ in range(5)]))
        label_us = med(lambda k: e.pseudo_label(prob, labels=True))
        comp_us = med(lambda k: e.regions_label(labels, connectivity=4, area=False))
        pair_us = med(lambda k: INS.raw_pair_device(prob, labels, comp, itd, w["slots"], w["max_rows"], table=w["table"], rows=w["rows"]))
        torch.cuda.synchronize(); t0 = time.perf_counter()
        for _ in range(3):
            rows, _bad = e.instance_pair(prob, labels, comp, itd)
        host_rows_ms = (time.perf_counter() - t0) * 1e3 / 3
        t0 = time.perf_counter()
        st = INS.new_stats()
        INS.stats_add(st, rows[0])
        host_match_ms = (time.perf_counter() - t0) * 1e3
        t0 = time.perf_counter()
        INS.results(st)
        host_results_ms = (time.perf_counter() - t0) * 1e3
    m.close()
    a_ms, b_ms = float(np.median(ta)), float(np.median(tb))
    recs = [dict(leg="e2e", state="evaluate_reliability", images=nimg, shape="2048x1024", precision="fp32", reps=reps, blocks=blocks,
                 ms_per_image=round(a_ms, 3), block_spread_ms=round(max(ta) - min(ta), 3)),
            dict(leg="e2e", state="evaluate_cityscapes_instances", images=nimg, shape="2048x1024", precision="fp32", reps=reps, blocks=blocks,
                 ms_per_image=round(b_ms, 3), block_spread_ms=round(max(tb) - min(tb), 3), rows_last_image=len(rows[0]),
                 predictions=int(res["nbPredictions"].sum()), all_ap=res["averages"]["allAp"]),
            dict(leg="e2e_parts", shape="2048x1024", precision="fp32", rows_last_image=len(rows[0]),
                 device_pseudo_label_ms=round(label_us * 1e-3, 4), device_regions_label_ms=round(comp_us * 1e-3, 4), device_instance_pair_ms=round(pair_us * 1e-3, 4),
                 host_pair_rows_device_whole_call_ms=round(host_rows_ms, 3), host_image_instances_ms=round(host_match_ms, 3),
                 host_results_one_image_ms=round(host_results_ms, 3))]
    for r in recs:
        print(json.dumps(r), flush=True)
    return recs


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--reps", type=int, default=10, help="calls per block")
    ap.add_argument("--blocks", type=int, default=5, help="alternating blocks")
    ap.add_argument("--images", type=int, default=2, help="images of the end-to-end leg")
    ap.add_argument("--e2e-reps", type=int, default=1, help="directory evaluations per block of the end-to-end leg")
    ap.add_argument("--legs", default="op,e2e")
    ap.add_argument("--out")
    a = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("instances_bench.py measures on an MI355X; no GPU here")
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
