#!/usr/bin/env python3
"""The fused Cityscapes counting pass (fcn8s_op_cityscapes_pair) next to the confusion kernel it extends, and the one-call evaluation
next to the export + file route.

Kernel legs, per shape (16 x 1024x512, 4 x 2048x1024, 1 x 2048x1024) and per kind of instance map -- `cityscapes_like` (a few dozen large
instances per image: long runs) and `adversarial` (the maps of tests/test_cityscapes_instances_gpu.py: hundreds of instances, one-pixel-wide
interleaved columns, a row in which every pixel is its own instance, 2 % speckle in the prediction):
  * fused_us: device events around --reps launches on resident inputs after --warmup discarded ones; the launches walk over enough
    distinct input sets (rolled copies of one map, > 2 x the 256 MiB Infinity Cache in total) that no set is served from the cache;
  * bytes read (11 per pixel for int64 predictions) / time, and that as a fraction of the 8 TB/s HBM rate of the project's roofline;
  * confusion_us: fcn8s_op_confusion (the parent's kernel, untouched: 9 bytes per pixel, one counter) on the same pixels, same method,
    same process, alternating blocks; ratio = fused / confusion;
  * copy_TBps: a device-to-device copy of 1 GiB in the same process (read + written bytes / time), and inst_read_us = the instance map's
    bytes at that rate: fused_us against confusion_us + inst_read_us is the question the README answers.
End-to-end leg (--e2e N): a frozen full-width fp32 model over N synthetic 2048x1024 PNG triples: evaluate_cityscapes against
predict_and_export_label_ids + evaluate_directory(instance_level=True) (the host route), per image, with the PNG decode time of the
triple listed separately (both routes pay it; the host route also encodes and decodes the prediction).
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

PEAK_HBM = 8e12
CACHE_BYTES = 256 << 20
SHAPES = [("16x1024x512", 16, 512, 1024), ("4x2048x1024", 4, 1024, 2048), ("1x2048x1024", 1, 1024, 2048)]


def make_maps(N, H, W, kind, seed):
    """(gt uint8, inst uint16, train int64), each [N, H*W]"""
    from fcn8s_tensorflow_amd import cityscapes_eval as ce
    rng = np.random.default_rng(seed)
    things = np.array(ce.HAS_INSTANCES_IDS)
    blk = 64 if kind == "cityscapes_like" else 32
    gt = np.kron(rng.choice([0, 4, 7, 8, 11, 21, 23], (N, H // blk, W // blk)), np.ones((blk, blk), np.int64)).astype(np.uint8)
    inst = gt.astype(np.uint16)
    for n in range(N):
        if kind == "cityscapes_like":
            for k in range(40):
                lab = int(things[rng.integers(0, len(things))])
                h, w = int(rng.integers(20, H // 4)), int(rng.integers(20, W // 6))
                y, x = int(rng.integers(0, H - h)), int(rng.integers(0, W - w))
                gt[n, y:y + h, x:x + w] = lab
                inst[n, y:y + h, x:x + w] = lab if k % 5 == 0 else lab * 1000 + k
        else:
            for k in range(300):
                lab = int(things[rng.integers(0, len(things))])
                h, w = (int(rng.integers(1, 120)), int(rng.integers(1, 200))) if k % 3 else (int(rng.integers(1, 4)), int(rng.integers(1, 4)))
                y, x = int(rng.integers(0, H - h)), int(rng.integers(0, W - w))
                gt[n, y:y + h, x:x + w] = lab
                inst[n, y:y + h, x:x + w] = lab if rng.random() < 0.2 else lab * 1000 + int(rng.integers(0, 1000))
            y, x = int(rng.integers(0, H // 2)), int(rng.integers(0, W // 2))
            gt[n, y:y + H // 2, x:x + W // 2] = 26; inst[n, y:y + H // 2, x:x + W // 2] = 26999
            y, x = int(rng.integers(0, H - 64)), int(rng.integers(0, W - 64))
            cols = np.arange(64)
            gt[n, y:y + 64, x:x + 64] = np.where(cols % 2, 24, 25)[None, :]
            inst[n, y:y + 64, x:x + 64] = np.where(cols % 2, 24000, 25998)[None, :]
            y2 = int(rng.integers(0, H - 8))
            gt[n, y2, :] = 33; inst[n, y2, :] = 33000 + (np.arange(W) % 1000)
    train = ce.IDS_TO_TRAINIDS_ARRAY[gt].astype(np.int64)
    b = 16 if kind == "cityscapes_like" else 8
    damaged = np.kron(rng.random((N, H // b, W // b)) < (0.1 if kind == "cityscapes_like" else 0.3), np.ones((b, b), bool))
    train[damaged] = np.kron(rng.integers(0, 20, (N, H // b, W // b)), np.ones((b, b), np.int64))[damaged]
    if kind == "adversarial":
        speck = rng.random(train.shape) < 0.02
        train[speck] = rng.integers(0, 20, int(speck.sum()))
    return gt.reshape(N, -1), inst.reshape(N, -1), train.reshape(N, -1)


def timed(fn, nsets, warmup, reps):
    """mean microseconds per call of fn(set index) by device events around `reps` back-to-back launches"""
    import torch
    for r in range(warmup):
        fn(r % nsets)
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for r in range(reps):
        fn(r % nsets)
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) * 1e3 / reps


def copy_rate():
    import torch
    x = torch.empty(1 << 30, dtype=torch.uint8, device="cuda"); y = torch.empty_like(x)
    us = timed(lambda _i: y.copy_(x), 1, 3, 20)
    return 2.0 * x.numel() / (us * 1e-6)


def kernel_legs(warmup, reps, blocks):
    import torch
    from fcn8s_tensorflow_amd import _lib as L
    from fcn8s_tensorflow_amd import cityscapes_eval as ce
    lib = L.lib
    ptr = lambda t: C.c_void_p(t.data_ptr())
    rate = copy_rate()
    lut = torch.as_tensor(ce.TRAINIDS_TO_IDS_ARRAY.astype(np.int64)).cuda()
    out = []
    for name, N, H, W in SHAPES:
        for kind in ("cityscapes_like", "adversarial"):
            gt, inst, train = make_maps(N, H, W, kind, seed=N + H)
            P = H * W
            set_bytes = N * P * 11
            nsets = max(2, -(-2 * CACHE_BYTES // set_bytes) + 1)
            g0, i0, p0 = torch.from_numpy(gt).cuda(), torch.from_numpy(inst.view(np.int16)).cuda(), torch.from_numpy(train).cuda()
            sets = []
            for s in range(nsets):                                     # rolled copies: the same statistics in distinct memory
                sh = s * 4099 * 16
                g, i, p = torch.roll(g0, sh, 1).contiguous(), torch.roll(i0, sh, 1).contiguous(), torch.roll(p0, sh, 1).contiguous()
                sets.append((g, i, p, lut[p]))
            conf = torch.zeros(34 * 34, dtype=torch.int64, device="cuda")
            counts = torch.zeros((N, 3), dtype=torch.int64, device="cuda")
            work = torch.empty(lib.fcn8s_op_cityscapes_work_bytes(N), dtype=torch.uint8, device="cuda")
            entries = torch.empty((N, 2048, 4), dtype=torch.int32, device="cuda")

            def fused(s):
                g, i, p, _ = sets[s]
                L.check(lib.fcn8s_op_cityscapes_pair(None, ptr(g), ptr(i), ptr(p), 0, N, P, ptr(conf), ptr(work), ptr(entries), 2048, ptr(counts)))

            def old(s):
                g, _, _, q = sets[s]
                L.check(lib.fcn8s_op_confusion(None, ptr(g), ptr(q), N * P, ptr(conf), 34))

            tf, to = [], []
            for _ in range(blocks):                                    # alternating blocks: both see the same clocks and neighbours
                tf.append(timed(fused, nsets, warmup, reps)); to.append(timed(old, nsets, warmup, reps))
            torch.cuda.synchronize()
            found = int(counts[:, 0].max())
            fused_us, old_us = float(np.median(tf)), float(np.median(to))
            inst_read_us = N * P * 2 / rate * 1e6
            rec = dict(leg="kernel", shape=name, maps=kind, input_sets=nsets, reps=reps, blocks=blocks, entries_per_image_max=found,
                       fused_us=round(fused_us, 2), fused_us_min=round(min(tf), 2), fused_us_max=round(max(tf), 2),
                       bytes_read=set_bytes, fused_TBps=round(set_bytes / fused_us * 1e-6, 3), fraction_of_hbm_8TBps=round(set_bytes / (fused_us * 1e-6) / PEAK_HBM, 3),
                       confusion_us=round(old_us, 2), confusion_TBps=round(N * P * 9 / old_us * 1e-6, 3), ratio_fused_over_confusion=round(fused_us / old_us, 3),
                       copy_TBps=round(rate * 1e-12, 3), inst_read_us=round(inst_read_us, 2),
                       fused_minus_confusion_plus_inst_read_us=round(fused_us - (old_us + inst_read_us), 2))
            print(json.dumps(rec), flush=True)
            out.append(rec)
            del sets
            torch.cuda.empty_cache()
    return out


def e2e_leg(nimg):
    import torch
    from PIL import Image
    from fcn8s_tensorflow_amd import cityscapes_eval as ce
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
        search = os.path.join(d, "gtFine", "*", "*_gtFine_labelIds.png")
        images = os.path.join(d, "leftImg8bit")
        t0 = time.perf_counter()
        for root, _, files in os.walk(d):
            for f in files:
                np.array(Image.open(os.path.join(root, f)))
        decode = time.perf_counter() - t0
        m.evaluate_cityscapes(images, search)                         # warm-up: workspaces, code objects
        torch.cuda.synchronize()
        one, host = [], []
        for _ in range(3):
            t0 = time.perf_counter(); a = m.evaluate_cityscapes(images, search); torch.cuda.synchronize(); one.append(time.perf_counter() - t0)
            t0 = time.perf_counter()
            m.predict_and_export_label_ids(os.path.join(d, "results"), images)
            b = ce.evaluate_directory(search, os.path.join(d, "results"), instance_level=True)
            host.append(time.perf_counter() - t0)
        assert (a["confMatrix"] == b["confMatrix"]).all() and a["instStats"] == b["instStats"]
    m.close()
    rec = dict(leg="e2e", images=nimg, shape="2048x1024", precision="fp32", model="full width, synthetic weights, frozen",
               evaluate_cityscapes_ms_per_image=round(float(np.median(one)) / nimg * 1e3, 2),
               export_plus_evaluate_directory_ms_per_image=round(float(np.median(host)) / nimg * 1e3, 2),
               png_decode_of_the_triple_ms_per_image=round(decode / nimg * 1e3, 2), results_equal=True)
    print(json.dumps(rec), flush=True)
    return [rec]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--reps", type=int, default=200)
    ap.add_argument("--blocks", type=int, default=5)
    ap.add_argument("--e2e", type=int, default=4, help="images of the end-to-end leg (0: skip it)")
    ap.add_argument("--no-kernel", action="store_true")
    ap.add_argument("--out")
    a = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("cityscapes_eval_bench.py measures on an MI355X; no GPU here")
    recs = []
    if not a.no_kernel:
        recs += kernel_legs(a.warmup, a.reps, a.blocks)
    if a.e2e > 0:
        recs += e2e_leg(a.e2e)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            for r in recs:
                f.write(json.dumps(r) + "\n")


if __name__ == "__main__":
    main()
