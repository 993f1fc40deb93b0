#!/usr/bin/env python3
"""The reliability counting pass (fcn8s_op_reliability_pair) against a copy of its bytes, and what evaluate_reliability adds to predict_mc.

Op leg, per shape (16 x 1024x512, 1 x 2048x1024), 20 classes, J = 0 and J = 2 uncertainty maps, B = 15, and three inputs:
  uniform   confidences uniform in [1/C, 1), scores uniform in [0, score_max): every table entry is hit, no entry often
  trained   confidences 1 - 0.05 u^4 (concentrated above 0.95), entropy of that row and 0.3 x it: a wave's pixels share a few entries
  constant  every pixel the same row, label and scores: one entry per table takes every add
the op next to a same-process device-to-device copy of its algorithmic bytes, (4 C + 1 + 4 J) per pixel (half of them read, half written).
Inputs rotate through more sets than 2 x the 256 MiB Infinity Cache holds.  Alternating blocks, device events around --kreps launches.
Records ratio_to_copy and whether it is within the 1.25 x bar of the project's streaming kernels; nothing fails on it.

End-to-end leg, the full-width fp32 model, frozen, over --images synthetic 2048x1024 PNG pairs in a temporary directory:
  mc_alone   per image: decode the PNG, one upload, Engine.predict_mc(samples=8, argmax=False), synchronise
  evaluate   FCN8s.evaluate_reliability(samples=8) over the directory, per image
alternating blocks in one process, wall clock (the decode is host work); beside them the op at this shape and the label map's upload
alone (and its PNG decode, which evaluate pays and mc_alone does not).  Condition row: added time <= t(op) + t(label upload) + the spread of
the mc_alone blocks, printed true or false.
Prints one JSON line per record and writes them to --out if given."""
import argparse
import ctypes as C
import json
import math
import os
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from cityscapes_eval_bench import CACHE_BYTES, PEAK_HBM, SHAPES, timed  # noqa: E402

NC = 20
BAR = 1.25


def make_inputs(kind, npix, J, seed):
    """(prob [npix, NC], gt [npix] uint8, scores) on the device."""
    import torch
    g = torch.Generator(device="cuda").manual_seed(seed)
    u = torch.rand(npix, device="cuda", generator=g)
    if kind == "constant":
        conf = torch.full((npix,), 0.9, device="cuda")
        k = torch.full((npix,), 7, dtype=torch.int64, device="cuda")
    else:
        conf = 1.0 / NC + (1.0 - 1.0 / NC) * u if kind == "uniform" else 1.0 - 0.05 * u ** 4
        k = torch.randint(0, NC, (npix,), device="cuda", generator=g)
    prob = ((1.0 - conf) / (NC - 1))[:, None].repeat(1, NC)
    prob.scatter_(1, k[:, None], conf[:, None])
    if kind == "constant":
        gt = k.to(torch.uint8)
    else:                                                                  # 80 % correct, 15 % another class, 5 % ignored
        r = torch.rand(npix, device="cuda", generator=g)
        gt = torch.where(r < 0.8, k, torch.randint(0, NC, (npix,), device="cuda", generator=g)).to(torch.uint8)
        gt[r > 0.95] = 255
    scores = []
    if J:
        if kind == "uniform":
            scores = [torch.rand(npix, device="cuda", generator=g) * math.log(NC) for _ in range(J)]
        else:
            ent = -(prob * torch.log(prob.clamp_min(1e-38))).sum(1)
            scores = [ent * (0.3 ** j) for j in range(J)]
    del u, conf, k
    return prob.contiguous(), gt.contiguous(), [s.contiguous() for s in scores]


def op_leg(shapes, warmup, reps, blocks):
    import torch
    from fcn8s_tensorflow_amd import _lib as L, reliability as rel
    lib = L.lib
    ptr = lambda t: C.c_void_p(t.data_ptr())
    lut = torch.from_numpy(rel.identity_lut()).cuda()
    out = []
    for name, n, h, w in shapes:
        npix = n * h * w
        for J in (0, 2):
            by = (4 * NC + 1 + 4 * J) * npix
            nsets = max(2, -(-2 * CACHE_BYTES // by) + 1)
            assert nsets * by > 2 * CACHE_BYTES
            half = by // 2 // 16 * 16
            src = [torch.empty(half, dtype=torch.uint8, device="cuda") for _ in range(max(2, -(-2 * CACHE_BYTES // half) + 1))]
            dst = torch.empty(half, dtype=torch.uint8, device="cuda")
            for kind in ("uniform", "trained", "constant"):
                sets = [make_inputs(kind, npix, J, 100 * s + J) for s in range(nsets)]
                tables = rel.new_tables_device(15, J, "cuda")
                scl = (C.c_float * max(J, 1))(*[float(np.float32(rel.SCORE_BINS) / np.float32(math.log(NC)))] * J)
                ptrs = [(C.c_void_p * max(J, 1))(*[s.data_ptr() for s in sc]) for _, _, sc in sets]
                # every argument is built once: at these sizes a launch takes less time than marshalling fifteen arguments does
                args = [(None, ptr(p), ptr(g), ptr(lut), n, h * w, NC, ptrs[i], scl, J, 15) + tuple(ptr(t) for t in tables) for i, (p, g, _) in enumerate(sets)]
                fn = lib.fcn8s_op_reliability_pair
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
                counted = int(tables[1][0])
                assert counted > 0 and not bool(tables[3].any())
                k_us, c_us = float(np.median(tk)), float(np.median(tc))
                rec = dict(leg="op", input=kind, shape=name, classes=NC, scores=J, bins=15, input_sets=nsets, reps=reps, blocks=blocks, bytes_needed=by,
                           op_us=round(k_us, 2), op_us_min_max=[round(min(tk), 2), round(max(tk), 2)],
                           copy_us=round(c_us, 2), copy_us_min_max=[round(min(tc), 2), round(max(tc), 2)], copy_bytes=2 * half,
                           ratio_to_copy=round(k_us / c_us, 3), within_bar=bool(k_us / c_us <= BAR), bar=BAR,
                           op_TBps=round(by / k_us * 1e-6, 3), copy_TBps=round(2 * half / c_us * 1e-6, 3),
                           fraction_of_hbm_8TBps=round(by / (k_us * 1e-6) / PEAK_HBM, 4))
                print(json.dumps(rec), flush=True)
                out.append(rec)
                del sets, tables, ptrs
                torch.cuda.empty_cache()
            del src, dst
            torch.cuda.empty_cache()
    return out


def e2e_leg(nimages, warmup, blocks, samples=8):
    import torch
    from PIL import Image
    from fcn8s_tensorflow_amd import reliability as rel
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
        m = FCN8s(vgg16_dir='synthetic:0', num_classes=NC)
        e = m.engine
        e.freeze()
        dev = e.device

        def mc_alone():
            for p in imgs:
                image = torch.from_numpy(np.array(Image.open(p).convert('RGB'))[None]).to(dev)
                e.predict_mc(image, samples=samples, keep_prob=0.5, argmax=False)
            torch.cuda.synchronize()

        def evaluate():
            m.evaluate_reliability(os.path.join(root, "leftImg8bit", "val"), search, samples=samples)
            torch.cuda.synchronize()

        def wall(fn):
            torch.cuda.synchronize()
            t0 = time.perf_counter(); fn()
            return (time.perf_counter() - t0) * 1e3 / nimages

        import contextlib
        import io
        for _ in range(max(1, warmup)):
            mc_alone()
            with contextlib.redirect_stdout(io.StringIO()):
                evaluate()
        ta, tb = [], []
        for _ in range(blocks):
            ta.append(wall(mc_alone))
            with contextlib.redirect_stdout(io.StringIO()):
                tb.append(wall(evaluate))
        # the parts: the op at this shape on the route's own outputs, the label map's upload, its decode
        image = torch.from_numpy(np.array(Image.open(imgs[0]).convert('RGB'))[None]).to(dev)
        prob, ent, mi = e.predict_mc(image, samples=samples, keep_prob=0.5, argmax=False)
        gt_host = np.array(Image.open(gts[0])).astype(np.uint8)[None]
        gt_dev = torch.from_numpy(gt_host).to(dev)
        lut = torch.from_numpy(rel.cityscapes_lut()).to(dev)
        tables = rel.new_tables_device(15, 2, dev)
        scales = [np.float32(rel.SCORE_BINS) / np.float32(math.log(NC))] * 2
        op_us = float(np.median([timed(lambda k: rel.counts_device(prob, gt_dev, lut, [ent, mi], scales, 15, tables), 1, 2, 10) for _ in range(5)]))
        up, dec = [], []
        for _ in range(10):
            t0 = time.perf_counter(); a = np.array(Image.open(gts[0])); t1 = time.perf_counter()
            torch.from_numpy(a.astype(np.uint8)[None]).to(dev); torch.cuda.synchronize(); t2 = time.perf_counter()
            dec.append((t1 - t0) * 1e3); up.append((t2 - t1) * 1e3)
        m.close()
    a_ms, b_ms = float(np.median(ta)), float(np.median(tb))
    spread = max(ta) - min(ta)
    added = b_ms - a_ms
    allowed = op_us * 1e-3 + float(np.median(up)) + spread
    recs = [dict(leg="e2e", state="mc_alone", shape="1x2048x1024", precision="fp32", samples=samples, images=nimages, blocks=blocks, ms_per_image=round(a_ms, 3),
                 block_spread_ms=round(spread, 3)),
            dict(leg="e2e", state="evaluate_reliability", shape="1x2048x1024", precision="fp32", samples=samples, images=nimages, blocks=blocks,
                 ms_per_image=round(b_ms, 3), block_spread_ms=round(max(tb) - min(tb), 3)),
            dict(leg="e2e_condition", shape="1x2048x1024", precision="fp32", samples=samples, added_ms_per_image=round(added, 3), op_ms=round(op_us * 1e-3, 4),
                 label_upload_ms=round(float(np.median(up)), 3), label_png_decode_ms=round(float(np.median(dec)), 3), spread_mc_alone_ms=round(spread, 3),
                 allowed_ms=round(allowed, 3), added_within_op_plus_upload_plus_spread=bool(added <= allowed),
                 added_minus_label_decode_ms=round(added - float(np.median(dec)), 3))]
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
        raise SystemExit("reliability_bench.py measures on an MI355X; no GPU here")
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
