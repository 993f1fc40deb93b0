#!/usr/bin/env python
"""Generates tests/golden/trimap_cases.npz: small label maps and the three tables of fcn8s_op_boundary_pair's definition (include/fcn8s_hip.h)
computed by an INDEPENDENT route -- SciPy's exact Euclidean distance transform, not the package's NumPy route and not the HIP kernel:

    python tests/golden/make_trimap_cases.py        # needs SciPy

  rings:  per ground-truth label l, distance_transform_edt of the mask G == l gives every pixel of l its distance to the nearest pixel of
          another label; squared and rounded it is the integer d2 of the definition.
  bprec:  per class c, distance_transform_edt of the complement of {q in B(G): G[q] == c} gives every pixel its distance to the nearest true
          contour pixel of c; read at the predicted contour pixels of c.  brec: the same with the maps exchanged.

Cases: Voronoi cells with a shifted and salted prediction, thin one-pixel structures, a constant map, pure noise, a label that touches all
four image edges; sizes that are multiples of nothing; R in {1, 3, 8, 16}.  tests/test_trimap_host.py holds the NumPy route against these
tables, tests/test_trimap_gpu.py the kernel.
"""
import os

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
L = 34


def ring_of(d2, R):
    k = np.full(d2.shape, R + 1, np.int64)
    for r in range(R, -1, -1):
        k[d2 <= r * r] = r
    return k


def bset(M):
    b = np.zeros(M.shape, bool)
    b[:-1] |= M[:-1] != M[1:]; b[1:] |= M[1:] != M[:-1]
    b[:, :-1] |= M[:, :-1] != M[:, 1:]; b[:, 1:] |= M[:, 1:] != M[:, :-1]
    return b


def tables_scipy(G, P, R):
    from scipy import ndimage as ndi
    G = G.astype(np.int64); P = P.astype(np.int64)
    H, W = G.shape
    d2 = np.zeros((H, W), np.int64)
    for l in np.unique(G):
        m = G == l
        if m.all():
            d2[m] = 1 << 30
            continue
        d2[m] = np.rint(ndi.distance_transform_edt(m)[m] ** 2).astype(np.int64)
    k = ring_of(d2, R)
    rings = np.zeros((R + 1, L, L), np.int64)
    np.add.at(rings, (k - 1, G, P), 1)

    def match(S, T):
        BS, BT = bset(S), bset(T)
        kk = np.full((H, W), R + 1, np.int64)
        for c in np.unique(S[BS]):
            t = BT & (T == c)
            if not t.any():
                continue
            dd = np.rint(ndi.distance_transform_edt(~t) ** 2).astype(np.int64)
            sel = BS & (S == c)
            kk[sel] = ring_of(dd, R)[sel]
        out = np.zeros((R + 2, L), np.int64)
        np.add.at(out, (kk[BS], S[BS]), 1)
        return out
    return rings, match(P, G), match(G, P)


def voronoi(rng, H, W, n, labels):
    ys, xs = np.mgrid[:H, :W]
    py, px = rng.integers(0, H, n), rng.integers(0, W, n)
    lab = rng.choice(labels, n)
    return lab[np.argmin((ys[..., None] - py) ** 2 + (xs[..., None] - px) ** 2, -1)].astype(np.uint8)


def shifted_salted(rng, G, shift, salt):
    P = np.roll(G, shift, (0, 1)).copy()
    n = rng.random(G.shape) < salt
    P[n] = rng.integers(0, L, int(n.sum()))
    return P


def make_cases():
    rng = np.random.default_rng(20131)
    all_ids = np.arange(L)
    cases = []
    for H, W, R, cells in ((37, 53, 3, 9), (61, 95, 8, 14), (45, 131, 16, 10), (23, 29, 1, 6)):
        G = voronoi(rng, H, W, cells, all_ids)
        cases.append((G, shifted_salted(rng, G, (int(rng.integers(-3, 4)), int(rng.integers(-3, 4))), 0.02), R))
    # thin structures: one-pixel lines and isolated pixels on a background, the prediction one pixel off and partly missing
    G = np.full((41, 67), 7, np.uint8); G[10, 3:60] = 17; G[5:38, 30] = 19; G[20, 50] = 24; G[0, 0] = 26; G[40, 66] = 33; G[25:27, 5:20] = 20
    P = np.full_like(G, 7); P[11, 3:50] = 17; P[5:38, 31] = 19; P[22, 52] = 24; P[25:27, 6:21] = 20
    cases.append((G, P, 3)); cases.append((G, P, 8))
    # a constant map, predicted exactly
    cases.append((np.full((19, 70), 23, np.uint8), np.full((19, 70), 23, np.uint8), 16))
    # pure noise: every pixel a contour pixel
    cases.append((rng.integers(0, L, (33, 47)).astype(np.uint8), rng.integers(0, L, (33, 47)).astype(np.uint8), 8))
    cases.append((rng.integers(0, 3, (29, 31)).astype(np.uint8) + 7, rng.integers(0, 3, (29, 31)).astype(np.uint8) + 7, 16))
    # a label that touches all four image edges (a frame) around a blob, the prediction's blob larger
    G = np.full((50, 77), 11, np.uint8); G[6:44, 9:70] = 21; G[20:30, 30:50] = 26
    P = np.full_like(G, 11); P[4:46, 6:72] = 21; P[18:33, 28:49] = 26
    cases.append((G, P, 8)); cases.append((G, P, 16))
    return cases


def main():
    out = {}
    cases = make_cases()
    for i, (G, P, R) in enumerate(cases):
        rings, bprec, brec = tables_scipy(G, P, R)
        assert rings.sum() == G.size
        out["G%d" % i] = G; out["P%d" % i] = P; out["R%d" % i] = np.int64(R)
        out["rings%d" % i] = rings; out["bprec%d" % i] = bprec; out["brec%d" % i] = brec
    out["n"] = np.int64(len(cases))
    path = os.path.join(HERE, "trimap_cases.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), "bytes,", len(cases), "cases")


if __name__ == "__main__":
    main()
