#!/usr/bin/env python3
"""The connected-region kernels (fcn8s_op_regions_label, fcn8s_op_regions_clean at rounds = 1) against a copy of their algorithmic bytes, and
what `predict(min_region=16)` costs next to `predict`.

Op leg, per shape (16 x 1024x512, 1 x 2048x1024), connectivity (4, 8) and input, int64 maps as `predict` writes them:
  cityscapes_like   the label maps of tools/cityscapes_eval_bench.py (blocks of 64 with 40 rectangles), as train ids
  salted            the same with 5 % of the pixels set to a random class
  spiral            a one-pixel-wide spiral through the whole image: two components, the worst case for the depth of the merges
  label             8 bytes in + 4 (comp) + 4 (area) out per pixel
  clean, 1 round    16 bytes per pixel (8 in, and 8 for the map written back at worst)
each next to a same-process device-to-device copy of those bytes (half read, half written).  Inputs rotate through more sets than 2 x the 256 MiB
Infinity Cache holds; the cleanup works in place, so every timed call is preceded, outside its pair of device events, by a copy of the
pristine map over the one it is about to clean.  Alternating blocks; per block the median over --reps calls, each between its own pair of device
events.  No bar is set: a union-find is not a streaming kernel; ratio_to_copy is recorded.

End-to-end leg, the full-width fp32 model, frozen, one 2048x1024 image on the device: `predict(min_region=16)` next to `predict`, alternating
blocks, wall clock.  Condition row: t(predict with cleanup) <= t(predict) + t(clean alone, on the route's own argmax) + the spread of the
`predict` blocks; printed true or false.
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
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from cityscapes_eval_bench import CACHE_BYTES, PEAK_HBM, SHAPES, make_maps  # noqa: E402


def spiral(H, W, a, b):
    """A one-pixel-wide rectangular spiral of class a in b: the arm advances until the cell two steps ahead is already spiral."""
    L = np.full((H, W), b, np.int64)
    y, x, d, turns = 0, 0, 0, 0
    dirs = [(0, 1), (1, 0), (0, -1), (-1, 0)]
    L[0, 0] = a
    while turns < 2:
        dy, dx = dirs[d]
        ny, nx, ay, ax = y + dy, x + dx, y + 2 * dy, x + 2 * dx
        if not (0 <= ny < H and 0 <= nx < W) or (0 <= ay < H and 0 <= ax < W and L[ay, ax] == a):
            d = (d + 1) % 4; turns += 1
            continue
        y, x, turns = ny, nx, 0
        L[y, x] = a
    return L


def make_input(kind, N, H, W):
    from fcn8s_tensorflow_amd import cityscapes_eval as ce
    if kind == "spiral":
        return np.broadcast_to(spiral(H, W, 13, 1), (N, H, W)).copy()
    gt = make_maps(N, H, W, "cityscapes_like", seed=N + H)[0].reshape(N, H, W)
    L = ce.IDS_TO_TRAINIDS_ARRAY[gt].astype(np.int64)
    L[(L < 0) | (L > 19)] = 0
    if kind == "salted":
        rng = np.random.default_rng(H)
        m = rng.random(L.shape) < 0.05
        L[m] = rng.integers(0, 20, int(m.sum()))
    return L


def per_call_us(fn, before, nsets, warmup, reps):
    """median microseconds of fn(set index), each call between its own pair of device events; before(set index) runs outside them"""
    import torch
    for r in range(warmup):
        before(r % nsets); fn(r % nsets)
    ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(reps)]
    for r in range(reps):
        before(r % nsets)
        ev[r][0].record(); fn(r % nsets); ev[r][1].record()
    torch.cuda.synchronize()
    return float(np.median([a.elapsed_time(b) for a, b in ev])) * 1e3


def op_leg(shapes, warmup, reps, blocks):
    import torch
    from fcn8s_tensorflow_amd import _lib as L, regions as R
    lib = L.lib
    ptr = lambda t: C.c_void_p(t.data_ptr())
    out = []
    table = torch.full((256,), 16, dtype=torch.int32, device="cuda")
    for name, N, H, W in shapes:
        npix = N * H * W
        nsets = max(2, -(-2 * CACHE_BYTES // (8 * npix)) + 1)
        assert nsets * 8 * npix > 2 * CACHE_BYTES
        work = torch.empty(R.work_bytes(N, H, W), dtype=torch.uint8, device="cuda")
        comp = torch.empty((N, H, W), dtype=torch.int32, device="cuda"); area = torch.empty_like(comp)
        stats = torch.empty((1, 4), dtype=torch.int64, device="cuda")
        for kind in ("cityscapes_like", "salted", "spiral"):
            base = make_input(kind, N, H, W)
            pristine = [torch.from_numpy(np.roll(base, (37 * s, 91 * s), (1, 2)) if kind != "spiral" else base).cuda() for s in range(nsets)]
            maps = [p.clone() for p in pristine]
            for conn in (4, 8):
                rcs = []
                ops = (("label", 16 * npix, lambda k: rcs.append(lib.fcn8s_op_regions_label(None, ptr(pristine[k]), 0, N, H, W, conn, ptr(comp), ptr(area), ptr(work))),
                        lambda k: None),
                       ("clean", 16 * npix, lambda k: rcs.append(lib.fcn8s_op_regions_clean(None, ptr(maps[k]), 0, N, H, W, conn, ptr(table), 1, ptr(work), ptr(stats))),
                        lambda k: maps[k].copy_(pristine[k])))
                for op, by, fn, before in ops:
                    half = by // 2
                    src = [torch.empty(half, dtype=torch.uint8, device="cuda") for _ in range(max(2, -(-2 * CACHE_BYTES // half) + 1))]
                    dst = torch.empty(half, dtype=torch.uint8, device="cuda")
                    tk, tc = [], []
                    for _ in range(blocks):
                        tk.append(per_call_us(fn, before, nsets, warmup, reps))
                        tc.append(per_call_us(lambda k: dst.copy_(src[k % len(src)]), lambda k: None, nsets, warmup, reps))
                    torch.cuda.synchronize()
                    assert not any(rcs), lib.fcn8s_last_error(None)
                    assert R.status_device(work)[0] == 0
                    k_us, c_us = float(np.median(tk)), float(np.median(tc))
                    rec = dict(leg="op", op=op, input=kind, shape=name, connectivity=conn, input_sets=nsets, reps=reps, blocks=blocks, bytes_needed=by,
                               op_us=round(k_us, 2), op_us_min_max=[round(min(tk), 2), round(max(tk), 2)],
                               copy_us=round(c_us, 2), copy_us_min_max=[round(min(tc), 2), round(max(tc), 2)], copy_bytes=2 * half,
                               ratio_to_copy=round(k_us / c_us, 3), ns_per_pixel=round(k_us * 1e3 / npix, 4),
                               fraction_of_hbm_8TBps=round(by / (k_us * 1e-6) / PEAK_HBM, 4))
                    if op == "clean":
                        rec.update(stats_last_call=[int(v) for v in stats[0].cpu()])
                    else:
                        rec.update(components_first_image=int((comp[0].view(-1) == torch.arange(H * W, device="cuda", dtype=torch.int32)).sum()))
                    print(json.dumps(rec), flush=True)
                    out.append(rec)
                    del src, dst
                    torch.cuda.empty_cache()
            del pristine, maps
            torch.cuda.empty_cache()
        del work, comp, area
        torch.cuda.empty_cache()
    return out


def e2e_leg(warmup, reps, blocks):
    import torch
    from fcn8s_tensorflow_amd.fcn8s import FCN8s
    H, W = 1024, 2048
    rng = np.random.default_rng(0)
    img = (np.kron(rng.integers(0, 256, (H // 16, W // 16, 3)), np.ones((16, 16, 1), np.int64)) // 2 + rng.integers(0, 32, (H, W, 3))).astype(np.uint8)
    m = FCN8s(vgg16_dir='synthetic:0', num_classes=20)
    m.engine.freeze(True)
    image = torch.from_numpy(img[None]).to(m.engine.device)

    def wall(fn):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(reps):
            fn()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3 / reps

    plain = lambda: m.predict(image)
    clean = lambda: m.predict(image, min_region=16)
    for _ in range(max(1, warmup)):
        wall(plain); wall(clean)
    ta, tb = [], []
    for _ in range(blocks):
        ta.append(wall(plain)); tb.append(wall(clean))
    pred = m.predict(image)
    scratch = pred.clone()
    alone_us = float(np.median([per_call_us(lambda k: m.engine.regions_clean(scratch, 16), lambda k: scratch.copy_(pred), 1, 2, 10) for _ in range(5)]))
    st = m.engine.regions_clean(pred.clone(), 16, stats=True).cpu().numpy().tolist()
    m.engine.freeze(False)
    m.close()
    a_ms, b_ms = float(np.median(ta)), float(np.median(tb))
    spread = max(ta) - min(ta)
    allowed = a_ms + alone_us * 1e-3 + spread
    recs = [dict(leg="e2e", state="predict", shape="1x2048x1024", precision="fp32", reps=reps, blocks=blocks, ms=round(a_ms, 3), block_spread_ms=round(spread, 3)),
            dict(leg="e2e", state="predict_min_region_16", shape="1x2048x1024", precision="fp32", reps=reps, blocks=blocks, ms=round(b_ms, 3),
                 block_spread_ms=round(max(tb) - min(tb), 3), stats=st),
            dict(leg="e2e_condition", shape="1x2048x1024", precision="fp32", predict_ms=round(a_ms, 3), with_cleanup_ms=round(b_ms, 3),
                 clean_alone_ms=round(alone_us * 1e-3, 4), spread_predict_ms=round(spread, 3), allowed_ms=round(allowed, 3),
                 with_cleanup_within_predict_plus_clean_plus_spread=bool(b_ms <= allowed))]
    for r in recs:
        print(json.dumps(r), flush=True)
    return recs


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--reps", type=int, default=10, help="calls per block")
    ap.add_argument("--blocks", type=int, default=5, help="alternating blocks")
    ap.add_argument("--legs", default="op,e2e")
    ap.add_argument("--out")
    a = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("regions_bench.py measures on an MI355X; no GPU here")
    recs = []
    legs = a.legs.split(",")
    if "op" in legs:
        recs += op_leg([SHAPES[0], SHAPES[2]], a.warmup, a.reps, a.blocks)
        torch.cuda.empty_cache()
    if "e2e" in legs:
        recs += e2e_leg(a.warmup, a.reps, a.blocks)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            for r in recs:
                f.write(json.dumps(r) + "\n")


if __name__ == "__main__":
    main()
