#!/usr/bin/env python3
"""The boundary counting pass (fcn8s_op_boundary_pair: trimap rings and boundary precision / recall tables) next to
fcn8s_op_cityscapes_pair without an instance map on the same pixels, and evaluate_cityscapes with and without boundary_radius=8.

Kernel legs, per shape (16 x 1024x512, 4 x 2048x1024, 1 x 2048x1024), per R in {3, 8, 16} and per kind of map -- `cityscapes_like` (the
label maps of tools/cityscapes_eval_bench.py: 64-pixel blocks and a few dozen large rectangles per image, the prediction damaged in 10 %
of its 16-pixel blocks) and `noise` (every pixel an independent label in both maps: every pixel is a contour pixel):
  * boundary_us: device events around --reps launches on resident inputs after --warmup discarded ones; the launches walk over enough
    distinct input sets (rolled copies of one map, > 2 x the 256 MiB Infinity Cache in total) that no set is served from the cache;
  * pair_us: fcn8s_op_cityscapes_pair with a NULL instance map (the parent's kernel: the same 9 bytes per pixel, one 34 x 34 table) on the
    same pixels, same method, same process, alternating blocks; ratio = boundary / pair;
  * bytes the algorithm needs (9 per pixel: uint8 ground truth + int64 prediction, each once) / time, and that as a fraction of the
    8 TB/s HBM rate of the project's roofline.  The kernel itself re-reads the halo of every tile (from the L2, mostly).
End-to-end leg (--e2e N): a frozen full-width fp32 model over N synthetic 2048x1024 PNG triples: evaluate_cityscapes with
boundary_radius=8 against the same call without a radius, per image, alternating.
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

from cityscapes_eval_bench import CACHE_BYTES, PEAK_HBM, SHAPES, make_maps, timed  # noqa: E402

RADII = (3, 8, 16)


def noise_maps(N, H, W, seed):
    rng = np.random.default_rng(seed)
    return rng.integers(0, 34, (N, H * W)).astype(np.uint8), rng.integers(0, 20, (N, H * W)).astype(np.int64)


def kernel_legs(warmup, reps, blocks):
    import torch
    from fcn8s_tensorflow_amd import _lib as L
    lib = L.lib
    ptr = lambda t: C.c_void_p(t.data_ptr())
    out = []
    for name, N, H, W in SHAPES:
        for kind in ("cityscapes_like", "noise"):
            if kind == "noise":
                gt, train = noise_maps(N, H, W, seed=N + H)
            else:
                gt, _, train = make_maps(N, H, W, kind, seed=N + H)
            P = H * W
            set_bytes = N * P * 9
            nsets = max(2, -(-2 * CACHE_BYTES // set_bytes) + 1)
            g0, p0 = torch.from_numpy(gt).cuda().view(N, H, W), torch.from_numpy(train).cuda().view(N, H, W)
            # rolled copies (rows and columns): the same statistics in distinct memory
            sets = [(torch.roll(g0, (s * 37, s * 4099), (1, 2)).contiguous(), torch.roll(p0, (s * 37, s * 4099), (1, 2)).contiguous()) for s in range(nsets)]
            conf = torch.zeros(34 * 34, dtype=torch.int64, device="cuda")
            counts = torch.zeros((N, 3), dtype=torch.int64, device="cuda")

            def pair(s):
                g, p = sets[s]
                L.check(lib.fcn8s_op_cityscapes_pair(None, ptr(g), None, ptr(p), 0, N, P, ptr(conf), None, None, 0, ptr(counts)))

            for R in RADII:
                rings = torch.zeros((R + 1) * 34 * 34, dtype=torch.int64, device="cuda")
                bprec = torch.zeros((R + 2) * 34, dtype=torch.int64, device="cuda"); brec = torch.zeros_like(bprec)
                bad = torch.zeros(1, dtype=torch.int64, device="cuda")

                def boundary(s):
                    g, p = sets[s]
                    L.check(lib.fcn8s_op_boundary_pair(None, ptr(g), ptr(p), 0, N, H, W, R, ptr(rings), ptr(bprec), ptr(brec), ptr(bad)))

                tb, tp = [], []
                for _ in range(blocks):                                # alternating blocks: both see the same clocks and neighbours
                    tb.append(timed(boundary, nsets, warmup, reps)); tp.append(timed(pair, nsets, warmup, reps))
                torch.cuda.synchronize()
                calls = blocks * (warmup + reps)
                near = int(rings[:R * 34 * 34].sum()) / float(calls * N * P)
                contour = int(bprec.sum() + brec.sum()) / float(2 * calls * N * P)
                b_us, p_us = float(np.median(tb)), float(np.median(tp))
                rec = dict(leg="kernel", shape=name, maps=kind, R=R, input_sets=nsets, reps=reps, blocks=blocks,
                           pixels_within_R_of_a_gt_boundary=round(near, 4), contour_pixels_per_pixel=round(contour, 4),
                           boundary_us=round(b_us, 2), boundary_us_min=round(min(tb), 2), boundary_us_max=round(max(tb), 2),
                           pair_us=round(p_us, 2), pair_us_min=round(min(tp), 2), pair_us_max=round(max(tp), 2),
                           ratio_boundary_over_pair=round(b_us / p_us, 2), bytes_needed=set_bytes,
                           boundary_TBps=round(set_bytes / b_us * 1e-6, 3), fraction_of_hbm_8TBps=round(set_bytes / (b_us * 1e-6) / PEAK_HBM, 4),
                           pair_TBps=round(set_bytes / p_us * 1e-6, 3))
                print(json.dumps(rec), flush=True)
                out.append(rec)
            del sets
            torch.cuda.empty_cache()
    return out


def e2e_leg(nimg, radius=8):
    import torch
    from PIL import Image
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
        m.evaluate_cityscapes(images, search, boundary_radius=radius)     # warm-up: workspaces, code objects
        torch.cuda.synchronize()
        plain, withr = [], []
        for _ in range(5):                                                # alternating
            t0 = time.perf_counter(); a = m.evaluate_cityscapes(images, search); torch.cuda.synchronize(); plain.append(time.perf_counter() - t0)
            t0 = time.perf_counter(); b = m.evaluate_cityscapes(images, search, boundary_radius=radius); torch.cuda.synchronize(); withr.append(time.perf_counter() - t0)
        assert (a["confMatrix"] == b["confMatrix"]).all() and (b["trimapRings"].sum(0) == a["confMatrix"]).all()
    m.close()
    p, w = float(np.median(plain)) / nimg * 1e3, float(np.median(withr)) / nimg * 1e3
    rec = dict(leg="e2e", images=nimg, shape="2048x1024", precision="fp32", model="full width, synthetic weights, frozen", boundary_radius=radius,
               evaluate_cityscapes_ms_per_image=round(p, 2), evaluate_cityscapes_ms_per_image_min_max=[round(min(plain) / nimg * 1e3, 2), round(max(plain) / nimg * 1e3, 2)],
               with_boundary_radius_ms_per_image=round(w, 2), with_boundary_radius_ms_per_image_min_max=[round(min(withr) / nimg * 1e3, 2), round(max(withr) / nimg * 1e3, 2)],
               added_ms_per_image=round(w - p, 2))
    print(json.dumps(rec), flush=True)
    return [rec]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--reps", type=int, default=100)
    ap.add_argument("--blocks", type=int, default=3)
    ap.add_argument("--e2e", type=int, default=4, help="images of the end-to-end leg (0: skip it)")
    ap.add_argument("--no-kernel", action="store_true")
    ap.add_argument("--out")
    a = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("trimap_bench.py measures on an MI355X; no GPU here")
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
