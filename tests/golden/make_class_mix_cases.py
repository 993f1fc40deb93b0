"""Writes tests/golden/class_mix_cases.npz: inputs and expected outputs of `fcn8s_op_class_mix` (the definition is in include/fcn8s_hip.h).

Everything here is plain Python: loops over pixels, and a Philox-4x32 on Python ints masked to 32 bits.  It shares nothing with
fcn8s_tensorflow_amd/class_mix.py or the kernel, so that agreement of the three means something.  NumPy only draws the inputs and holds the
arrays.  Run from the repository root:  python tests/golden/make_class_mix_cases.py"""
import os

import numpy as np

M32 = 0xFFFFFFFF
STREAM = 0x434D4958


def philox_first_word(idx, seed, stream):
    c = [idx & M32, (idx >> 32) & M32, stream & M32, 0x9E3779B9]
    k = [seed & M32, (seed >> 32) & M32]
    for _ in range(10):
        p0 = 0xD2511F53 * c[0]
        p1 = 0xCD9E8D57 * c[2]
        c = [((p1 >> 32) ^ c[1] ^ k[0]) & M32, p1 & M32, ((p0 >> 32) ^ c[3] ^ k[1]) & M32, p0 & M32]
        k = [(k[0] + 0x9E3779B9) & M32, (k[1] + 0xBB67AE85) & M32]
    return c[0]


def expected(images, labels, src, C, seed, draw):
    N, P = len(labels), len(labels[0])
    out_i = [[list(px) for px in img] for img in images]
    out_l = [list(row) for row in labels]
    selected = [[0] * 256 for _ in range(N)]
    for n in range(N):
        s = src[n] if 0 <= src[n] < N else n
        present = []
        for c in range(C):
            found = False
            for p in range(P):
                if labels[s][p] == c:
                    found = True
                    break
            if found:
                present.append(c)
        keyed = sorted((philox_first_word((draw << 16) + (n << 8) + c, seed, STREAM), c) for c in present)
        m = (len(present) + 1) // 2
        for _, c in keyed[:m]:
            selected[n][c] = 1
        for p in range(P):
            v = labels[s][p]
            if v < C and selected[n][v]:
                out_i[n][p] = list(images[s][p])
                out_l[n][p] = v
    return out_i, out_l, selected


def case(rng, N, P, C, src, seed, draw, labels=None, note=""):
    images = rng.integers(0, 256, (N, P, 3), dtype=np.uint8)
    if labels is None:
        # a few classes per image, with the ids C and 255 (both "ignore") among them
        labels = np.empty((N, P), np.uint8)
        for n in range(N):
            pool = list(rng.choice(C, size=min(C, int(rng.integers(1, 8))), replace=False)) + [C, 255]
            labels[n] = rng.choice(np.array(pool, np.uint8), size=P)
    labels = np.asarray(labels, np.uint8).reshape(N, P)
    oi, ol, sel = expected(images.tolist(), labels.tolist(), list(src), C, seed, draw)
    return dict(N=N, P=P, C=C, src=np.asarray(src, np.int32), seed=np.uint64(seed), draw=np.uint64(draw), images=images, labels=labels,
                out_images=np.asarray(oi, np.uint8), out_labels=np.asarray(ol, np.uint8), selected=np.asarray(sel, np.uint8), note=note)


def k_of(c, n):
    s = int(c["src"][n])
    return len(set(int(v) for v in c["labels"][s] if v < c["C"]))


def main():
    rng = np.random.default_rng(20211)
    cases = []
    classes = [2, 19, 20, 21, 64, 255]
    for i, P in enumerate([1, 15, 16, 17, 255, 256, 257, 1023, 1025]):
        cases.append(case(rng, 2, P, classes[i % len(classes)], [1, 0], seed=11 + i, draw=i, note="P"))
    for C in classes:
        cases.append(case(rng, 2, 257, C, [1, 0], seed=3, draw=5, note="C"))
    cases.append(case(rng, 3, 300, 20, [1, 2, 0], seed=7, draw=0, note="batch, src a rotation"))
    cases.append(case(rng, 3, 300, 20, [0, 1, 2], seed=7, draw=1, note="src[n] = n"))
    cases.append(case(rng, 3, 300, 20, [2, 2, 0], seed=7, draw=2, note="a repeated source"))
    one = np.full((2, 64), 255, np.uint8); one[0, ::3] = 4; one[1, 5:40] = 7; one[1, 50] = 20
    cases.append(case(rng, 2, 64, 20, [1, 0], seed=1, draw=3, labels=one, note="one present class"))
    ign = rng.integers(0, 20, (2, 64)).astype(np.uint8); ign[1] = 255; ign[1, ::2] = 20
    cases.append(case(rng, 2, 64, 20, [1, 0], seed=1, draw=4, labels=ign, note="a source with only ignore labels"))
    full = np.stack([np.arange(300) % 255, rng.permutation(300) % 255]).astype(np.uint8)
    cases.append(case(rng, 2, 300, 255, [1, 0], seed=9, draw=6, labels=full, note="all 255 classes present"))
    for k in (5, 6):
        lab = np.stack([rng.permutation(120) % k, (rng.permutation(120) % k) * 3]).astype(np.uint8)
        cases.append(case(rng, 2, 120, 20, [1, 0], seed=2, draw=7, labels=lab, note="k = %d" % k))
    same = rng.integers(0, 12, (2, 200)).astype(np.uint8)
    pair = []
    for draw in (0, 1, (1 << 48) - 1):
        r2 = np.random.default_rng(5)                        # the same images for the three draws
        pair.append(case(r2, 2, 200, 20, [1, 0], seed=4, draw=draw, labels=same, note="draw = %d on the same input" % draw))
    assert (pair[0]["images"] == pair[1]["images"]).all()
    assert (pair[0]["selected"] != pair[1]["selected"]).any(), "the two draws select the same sets: choose another seed"
    cases += pair

    # what the fixture promises, checked while it is written
    ks = set()
    for c in cases:
        for n in range(c["N"]):
            k = k_of(c, n)
            ks.add(k)
            assert int(c["selected"][n].sum()) == (k + 1) // 2 and not c["selected"][n][c["C"]:].any()
    assert {0, 1, 5, 6, 255} <= ks, ks
    assert any((c["labels"] == c["C"]).any() for c in cases) and any((c["labels"] == 255).any() for c in cases)

    out = {"count": np.int64(len(cases))}
    for i, c in enumerate(cases):
        for name, v in c.items():
            out["c%02d_%s" % (i, name)] = np.asarray(v)
    path = os.path.join(os.path.dirname(os.path.abspath(__file__)), "class_mix_cases.npz")
    np.savez_compressed(path, **out)
    print("%d cases, %d bytes -> %s" % (len(cases), os.path.getsize(path), path))


if __name__ == "__main__":
    main()
