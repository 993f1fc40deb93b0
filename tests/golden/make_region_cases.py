#!/usr/bin/env python
"""Generates tests/golden/region_cases.npz: small label maps with the components, areas and cleaned maps of the regions definition
(include/fcn8s_hip.h at fcn8s_op_regions_label), computed by a route that shares nothing with fcn8s_tensorflow_amd/regions.py or the kernels:
`scipy.ndimage.label` per class and `ndimage.minimum` for the ids; the cleanup walks the small components one at a time and looks at the
ring a cross-shaped dilation adds to each.  Needs SciPy; the tests only read the file.

    python tests/golden/make_region_cases.py

Layout of the file: `index` is a JSON list of cases {name, batch, configs: [{tag, rounds}]}; arrays `<name>.L` (uint8 [H, W], or [N, H, W]
for a batch), `<name>.T.<tag>` (the int32 [256] thresholds), and for c in (4, 8): `<name>.c<c>.comp`, `<name>.c<c>.area` (int32, L's
shape), `<name>.c<c>.<tag>.r<rounds>.out` (uint8, L's shape) and `.stats` (int64 [rounds, 4], summed over a batch).
"""
import json
import os

import numpy as np
from scipy import ndimage

HERE = os.path.dirname(os.path.abspath(__file__))
CROSS = np.array([[0, 1, 0], [1, 1, 1], [0, 1, 0]], bool)
FULL = np.ones((3, 3), bool)


def components(L, conn):
    H, W = L.shape
    index = np.arange(H * W).reshape(H, W)
    comp = np.zeros((H, W), np.int64)
    for c in np.unique(L):
        lbl, n = ndimage.label(L == c, structure=CROSS if conn == 4 else FULL)
        ids = np.asarray(ndimage.minimum(index, lbl, np.arange(1, n + 1))).astype(np.int64)
        m = lbl > 0
        comp[m] = ids[lbl[m] - 1]
    area = np.bincount(comp.ravel(), minlength=H * W)[comp]
    return comp, area


def clean_round(L, table, conn):
    H, W = L.shape
    comp, area = components(L, conn)
    thr = table[L]
    small = (thr > 0) & (area < thr)
    ids, inv = np.unique(comp, return_inverse=True)
    lab = inv.reshape(H, W) + 1
    out = L.copy()
    nsmall = nrel = nchanged = 0
    for k, sl in enumerate(ndimage.find_objects(lab), start=1):
        y, x = sl
        if not small.flat[ids[k - 1]]:                      # the component's id is its smallest pixel index
            continue
        nsmall += 1
        box = (slice(max(y.start - 1, 0), min(y.stop + 1, H)), slice(max(x.start - 1, 0), min(x.stop + 1, W)))
        sub = lab[box] == k
        ring = ndimage.binary_dilation(sub, structure=CROSS) & ~sub & ~small[box]
        if not ring.any():
            continue
        a, i = area[box][ring], comp[box][ring]
        best = np.lexsort((i, -a))[0]
        out[box][sub] = L.flat[i[best]]
        nrel += 1
        nchanged += int(sub.sum())
    return out, [len(ids), nsmall, nrel, nchanged]


def clean(L, table, conn, rounds):
    stats = []
    for _ in range(rounds):
        L, st = clean_round(L, table, conn)
        stats.append(st)
    return L, np.asarray(stats, np.int64)


def voronoi(rng, H, W, cells, classes, salt):
    py, px = rng.integers(0, H, cells), rng.integers(0, W, cells)
    cl = rng.integers(0, classes, cells)
    yy, xx = np.mgrid[0:H, 0:W]
    d = (yy[..., None] - py) ** 2 + (xx[..., None] - px) ** 2
    L = cl[np.argmin(d, -1)]
    m = rng.random((H, W)) < salt
    L[m] = rng.integers(0, classes, int(m.sum()))
    return L.astype(np.uint8)


def spiral(H, W, a, b):
    """A one-pixel-wide rectangular spiral walked turn by turn: the arm advances until the cell two steps ahead is already spiral."""
    L = np.full((H, W), b, np.uint8)
    y, x, d = 0, 0, 0
    dirs = [(0, 1), (1, 0), (0, -1), (-1, 0)]
    L[y, x] = a
    turns = 0
    while turns < 2:
        dy, dx = dirs[d]
        ny, nx, ay, ax = y + dy, x + dx, y + 2 * dy, x + 2 * dx
        blocked = not (0 <= ny < H and 0 <= nx < W) or (0 <= ay < H and 0 <= ax < W and L[ay, ax] == a)
        if blocked:
            d = (d + 1) % 4
            turns += 1
            continue
        y, x = ny, nx
        L[y, x] = a
        turns = 0
    return L


def comb(H, W, a, b):
    L = np.full((H, W), b, np.uint8)
    L[:, ::2] = a                # teeth
    L[H - 1, :] = a              # joined along the bottom row only
    return L


def tile_multiples(H, W):
    L = np.zeros((H, W), np.uint8)
    yy, xx = np.mgrid[0:H, 0:W]
    L[:] = 1 + (yy // 16 + 2 * (xx // 32)) % 3 + 3 * ((yy // 64 + xx // 64) % 2)
    d = np.arange(min(H, W))
    L[d, d] = 9                  # a diagonal one-pixel line through the tile corners
    return L


def hand_rules():
    L = np.full((14, 24), 1, np.uint8)
    L[3:6, 3:6] = 2; L[4, 4] = 3            # a small pixel inside a small ring: round 1 moves the ring, round 2 the pixel
    L[9, 12] = 5                            # a hole inside one big region
    L[0, 22:] = 7; L[1, 23] = 7             # a small region at the image's corner
    L[10:, 0:2] = 4                         # a region of 8 at the edge
    L[7:9, 18:21] = 6                       # a region of 6
    return L


def hand_tie():
    L = np.zeros((5, 9), np.uint8)
    L[:, :4] = 1; L[:, 4] = 2; L[:, 5:] = 3  # a small strip between two regions of equal area: the smaller id (the left one) wins
    return L


def main():
    rng = np.random.default_rng(20240611)
    cases = []

    def table_of(v):
        t = np.zeros(256, np.int32)
        if isinstance(v, dict):
            for c, a in v.items():
                t[c] = a
        else:
            t[:] = v
        return t

    def add(name, L, configs):
        cases.append((name, np.asarray(L, np.uint8), [(tag, table_of(v), rounds) for tag, v, rounds in configs]))

    vor = [("m8", 8, 1), ("m16", 16, 1), ("m32", 32, 1), ("m8", 8, 4), ("m16", 16, 4), ("m32", 32, 4)]
    add("voronoi_37x53_s05", voronoi(rng, 37, 53, 12, 20, 0.05), vor)
    add("voronoi_61x95_s10", voronoi(rng, 61, 95, 20, 20, 0.10), vor)
    add("voronoi_70x131_s30", voronoi(rng, 70, 131, 30, 20, 0.30), vor)
    add("spiral_97x101", spiral(97, 101, 3, 11), [("m16", 16, 1)])
    add("comb_67x130", comb(67, 130, 2, 5), [("m16", 16, 1), ("m200", 200, 2)])
    yy, xx = np.mgrid[0:33, 0:47]
    add("checker_33x47", ((yy + xx) % 2).astype(np.uint8) + 4, [("m8", 8, 1)])
    add("constant_19x70", np.full((19, 70), 13, np.uint8), [("m5000", 5000, 1), ("m5000", 5000, 3)])
    add("noise_33x47", rng.integers(0, 20, (33, 47)), [("m8", 8, 1), ("m8", 8, 4)])
    add("column_50x1", rng.integers(0, 3, (50, 1)), [("m4", 4, 2)])
    add("row_1x77", rng.integers(0, 3, (1, 77)), [("m4", 4, 2)])
    add("single_1x1", np.full((1, 1), 7), [("m4", 4, 1)])
    add("tiles_64x128", tile_multiples(64, 128), [("m100", 100, 1), ("m600", 600, 2)])
    add("tiles_128x256", tile_multiples(128, 256), [("m100", 100, 1), ("m600", 600, 2)])
    add("hand_rules", hand_rules(), [("m16", 16, 1), ("m16", 16, 2), ("perclass", {2: 16, 3: 0, 5: 2, 7: 4, 4: 8, 6: 6}, 2)])
    add("hand_tie", hand_tie(), [("m8", 8, 1)])
    b0 = voronoi(rng, 45, 70, 10, 20, 0.10)
    add("batch2_45x70", np.stack([b0, np.roll(b0, (3, 5), (0, 1))]), [("m16", 16, 1), ("m16", 16, 3)])

    arrays, index = {}, []
    for name, L, configs in cases:
        maps = L if L.ndim == 3 else L[None]
        arrays[name + ".L"] = L
        for tag, t, _ in configs:
            arrays["%s.T.%s" % (name, tag)] = t
        for conn in (4, 8):
            ca = [components(m, conn) for m in maps]
            comp = np.stack([c for c, _ in ca]).astype(np.int32).reshape(L.shape)
            area = np.stack([a for _, a in ca]).astype(np.int32).reshape(L.shape)
            arrays["%s.c%d.comp" % (name, conn)] = comp
            arrays["%s.c%d.area" % (name, conn)] = area
            for tag, t, rounds in configs:
                res = [clean(m, t.astype(np.int64), conn, rounds) for m in maps]
                arrays["%s.c%d.%s.r%d.out" % (name, conn, tag, rounds)] = np.stack([o for o, _ in res]).astype(np.uint8).reshape(L.shape)
                arrays["%s.c%d.%s.r%d.stats" % (name, conn, tag, rounds)] = sum(s for _, s in res)
        index.append(dict(name=name, batch=L.ndim == 3, configs=[dict(tag=tag, rounds=rounds) for tag, _, rounds in configs]))
        print(name, L.shape)
    arrays["index"] = np.frombuffer(json.dumps(index).encode(), np.uint8)
    path = os.path.join(HERE, "region_cases.npz")
    np.savez_compressed(path, **arrays)
    print(path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
