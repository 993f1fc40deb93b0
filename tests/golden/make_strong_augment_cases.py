"""Writes tests/golden/strong_augment_cases.npz: inputs and expected outputs of `fcn8s_op_strong_augment` (the definition is in include/fcn8s_hip.h).

Everything here is plain Python: loops over pixels, a Philox-4x32 on Python ints masked to 32 bits, and the float32 steps of OpenCV's 8-bit
HSV -> RGB rounded through `struct` after every operation (the product, sum or difference of two float32 values is exact in a double, so one
rounding to float32 gives the float32 operation's result).  It shares nothing with fcn8s_tensorflow_amd/strong_augment.py, cv2_compat.py or the
kernel, so that agreement of the three means something.  NumPy only draws the inputs and holds the arrays.  Run from the repository root:
python tests/golden/make_strong_augment_cases.py  (a few seconds, most of them the search for the two seeds whose contrast factor is exactly 0 and
exactly 2)"""
import math
import os
import struct

import numpy as np

M32 = 0xFFFFFFFF
STREAM = 0x53415547
ONE = 65536


def philox_first_word(idx, seed, stream):
    c = [idx & M32, (idx >> 32) & M32, stream & M32, 0x9E3779B9]
    k = [seed & M32, (seed >> 32) & M32]
    for _ in range(10):
        p0 = 0xD2511F53 * c[0]
        p1 = 0xCD9E8D57 * c[2]
        c = [((p1 >> 32) ^ c[1] ^ k[0]) & M32, p1 & M32, ((p0 >> 32) ^ c[3] ^ k[1]) & M32, p0 & M32]
        k = [(k[0] + 0x9E3779B9) & M32, (k[1] + 0xBB67AE85) & M32]
    return c[0]


def word(seed, draw, n, j):
    return philox_first_word((draw << 16) + (n << 8) + j, seed, STREAM)


def uniform(u, S):
    return -S + ((u * (2 * S + 1)) >> 32)


def f32(x):
    return struct.unpack('f', struct.pack('f', x))[0]


def cv_round(x):
    return int(round(x))                                     # half to even, as cvRound


SDIV = [0] + [cv_round((255 << 12) / v) for v in range(1, 256)]
HDIV = [0] + [cv_round((180 << 12) / (6.0 * d)) for d in range(1, 256)]


def rgb2hsv(r, g, b):
    v = max(r, g, b)
    diff = v - min(r, g, b)
    s = (diff * SDIV[v] + (1 << 11)) >> 12
    if v == r:
        h = g - b
    elif v == g:
        h = b - r + 2 * diff
    else:
        h = r - g + 4 * diff
    h = (h * HDIV[diff] + (1 << 11)) >> 12                  # (>> of a negative Python int is arithmetic)
    if h < 0:
        h += 180
    return h, s, v


SECTOR = [(1, 3, 0), (1, 0, 2), (3, 0, 1), (0, 2, 1), (0, 1, 3), (2, 1, 0)]      # tab index of (b, g, r)


def hsv2rgb(H, S, V):
    s = f32(S * f32(1.0 / 255.0))
    v = f32(V * f32(1.0 / 255.0))
    if s == 0.0:
        fb = fg = fr = v
    else:
        h = f32(H * f32(6.0 / 180.0))
        if h >= 6.0:
            h = f32(h - 6.0)
        sector = int(math.floor(h))
        h = f32(h - sector)
        if not 0 <= sector < 6:
            sector, h = 0, 0.0
        one = 1.0
        tab = [v, f32(v * f32(one - s)), f32(v * f32(one - f32(s * h))), f32(v * f32(one - f32(s * f32(one - h))))]
        fb, fg, fr = (tab[i] for i in SECTOR[sector])
    return tuple(min(255, max(0, cv_round(f32(x * 255.0)))) for x in (fr, fg, fb))


def taps_row(sigma, R):
    g = [math.exp(-(i * i) / (2.0 * sigma * sigma)) for i in range(-R, R + 1)]
    total = sum(g)
    w = [cv_round(2048 * g[R + i] / total) for i in range(1, R + 1)]
    row = [2048 - 2 * sum(w)] + w
    assert all(row[i] <= row[i - 1] for i in range(1, R + 1)) and row[0] + 2 * sum(row[1:]) == 2048, row
    return row


def taps(lo, hi, Q, R):
    return [taps_row(lo if Q == 1 else lo + (hi - lo) * q / (Q - 1), R) for q in range(Q)]


def reflect(i, n):
    if i < 0:
        return -i
    if i >= n:
        return 2 * (n - 1) - i
    return i


def expected(images, seed, draw, jitter, blur, seen):
    """images: nested lists [N][H][W][3]; jitter: None or [gate, Cs, Ss, Bs, Hs]; blur: None or (gate, table).  -> (out, params).  `seen`
    collects what happened on the way (hue wraps, clamps), for the promises checked in main()."""
    N, H, W = len(images), len(images[0]), len(images[0][0])
    out, params = [], []
    for n in range(N):
        img = [[list(px) for px in row] for row in images[n]]
        p = [0] * 8
        if jitter is not None and (word(seed, draw, n, 0) >> 16) < jitter[0]:
            p[0] = 1
            contrast = jitter[1] != 0
            hsv = (jitter[2] | jitter[3] | jitter[4]) != 0
            if contrast:
                p[1] = ONE + uniform(word(seed, draw, n, 1), jitter[1])
                total = 0
                for row in img:
                    for r, g, b in row:
                        total += (4899 * r + 9617 * g + 1868 * b + 8192) >> 14
                p[5] = (2 * total + H * W) // (2 * H * W)
            if hsv:
                p[2] = ONE + uniform(word(seed, draw, n, 2), jitter[2])
                p[3] = ONE + uniform(word(seed, draw, n, 3), jitter[3])
                p[4] = uniform(word(seed, draw, n, 4), jitter[4])
            for row in img:
                for px in row:
                    if contrast:
                        for k in range(3):
                            t = (px[k] * p[1] + p[5] * (ONE - p[1]) + 32768) >> 16
                            if t < 0 or t > 255:
                                seen.add("clamp")
                            px[k] = min(255, max(0, t))
                    if hsv:
                        h, s, v = rgb2hsv(*px)
                        if h + p[4] < 0:
                            seen.add("hue wraps below 0")
                        if h + p[4] >= 180:
                            seen.add("hue wraps above 179")
                        h = (h + 180 + p[4]) % 180
                        s = min(255, (s * p[2] + 32768) >> 16)
                        v = min(255, (v * p[3] + 32768) >> 16)
                        px[0], px[1], px[2] = hsv2rgb(h, s, v)
        if blur is not None and (word(seed, draw, n, 5) >> 16) < blur[0]:
            table = blur[1]
            p[6] = 1
            p[7] = (word(seed, draw, n, 6) * len(table)) >> 32
            w = table[p[7]]
            R = len(w) - 1
            a = [[[sum(w[abs(i)] * img[y][reflect(x + i, W)][k] for i in range(-R, R + 1)) for k in range(3)] for x in range(W)] for y in range(H)]
            img = [[[(sum(w[abs(i)] * a[reflect(y + i, H)][x][k] for i in range(-R, R + 1)) + (1 << 21)) >> 22 for k in range(3)] for x in range(W)]
                   for y in range(H)]
        out.append(img)
        params.append(p)
    return out, params


SEEN = set()


def case(images, seed, draw, jitter, blur, note):
    images = np.asarray(images, np.uint8)
    out, params = expected(images.tolist(), seed, draw, jitter, blur, SEEN)
    none_i = np.zeros(0, np.int32)
    return dict(N=images.shape[0], H=images.shape[1], W=images.shape[2], seed=np.uint64(seed), draw=np.uint64(draw),
                jitter=np.asarray(jitter, np.int32) if jitter is not None else none_i,
                blur_gate=np.int32(blur[0] if blur is not None else -1),
                taps=np.asarray(blur[1], np.uint16) if blur is not None else np.zeros((0, 0), np.uint16),
                images=images, out_images=np.asarray(out, np.uint8), params=np.asarray(params, np.int32), note=note)


def find_seed(pred, start=0):
    seed = start
    while not pred(seed):
        seed += 1
    return seed


def main():
    rng = np.random.default_rng(20212)
    img = lambda N, H, W: rng.integers(0, 256, (N, H, W, 3), dtype=np.uint8)
    T = {1: taps(0.3, 0.6, 3, 1), 4: taps(0.15, 1.15, 16, 4), 7: taps(0.5, 2.0, 16, 7)}
    FULL = [ONE, 16384, 16384, 16384, 23]
    cases = []
    # shapes: around a 16-byte line, around the tile of 32 x 64, and H = R + 1, W = R + 1 for R = 1, 4, 7
    for i, (H, W, R) in enumerate([(2, 2, 1), (5, 5, 4), (8, 8, 7), (15, 31, 4), (16, 32, 4), (17, 33, 7), (33, 63, 4), (2, 64, 1), (5, 65, 4), (8, 129, 7),
                                   (33, 2, 1), (17, 5, 4), (16, 8, 7)]):
        cases.append(case(img(2, H, W), 11 + i, i, FULL, (ONE, T[R]), "shape R%d" % R))
    # a batch whose images draw different gates
    gates = lambda s: ([(word(s, 3, n, 0) >> 16) < 52429 for n in range(3)], [(word(s, 3, n, 5) >> 16) < 32768 for n in range(3)])
    seed = find_seed(lambda s: all(len(set(g)) == 2 for g in gates(s)))
    cases.append(case(img(3, 48, 80), seed, 3, [52429, 16384, 16384, 16384, 23], (32768, T[4]), "batch, images draw different gates"))
    # each stage alone, the gates' ends, the identities
    base = img(2, 15, 31)
    cases.append(case(base, 1, 0, [ONE, 16384, 0, 0, 0], None, "contrast alone"))
    cases.append(case(base, 1, 1, [ONE, 0, 16384, 0, 0], None, "saturation alone"))
    cases.append(case(base, 1, 2, [ONE, 0, 0, 16384, 0], None, "brightness alone"))
    cases.append(case(base, 1, 3, [ONE, 0, 0, 0, 45], None, "hue alone"))
    cases.append(case(base, 1, 4, None, (ONE, T[4]), "blur alone"))
    cases.append(case(base, 1, 5, FULL, None, "jitter alone"))
    cases.append(case(base, 1, 6, [0] + FULL[1:], (0, T[4]), "gates 0: a copy"))
    cases.append(case(base, 1, 7, None, None, "no stage: a copy"))
    cases.append(case(base, 1, 8, [ONE, 0, 0, 0, 0], None, "strengths 0: the input"))
    cases.append(case(base, 1, 9, [ONE, ONE, ONE, ONE, 90], (ONE, T[4]), "full strengths"))
    # c16 at its ends: U(u_1, 65536) = -65536 iff u_1 (2^17 + 1) < 2^32, = +65536 iff u_1 (2^17 + 1) >= 2^17 * 2^32
    lo = find_seed(lambda s: word(s, 0, 0, 1) * 131073 < 1 << 32)
    hi = find_seed(lambda s: word(s, 0, 0, 1) * 131073 >= 131072 << 32)
    cases.append(case(base[:1], lo, 0, [ONE, ONE, 0, 0, 0], None, "c16 = 0: flat at m"))
    cases.append(case(base[:1], hi, 0, [ONE, ONE, 0, 0, 0], None, "c16 = 131072: clamping"))
    # grey, black, white and saturated pixels; hues next to 0 and to 179 under shifts of either sign
    special = np.zeros((1, 8, 16, 3), np.uint8)
    special[0, 0] = np.arange(16)[:, None] * 17                                              # greys, black and white among them
    prim = [(255, 0, 0), (0, 255, 0), (0, 0, 255), (255, 255, 0), (0, 255, 255), (255, 0, 255), (255, 255, 255), (0, 0, 0)]
    special[0, 1] = np.array(prim + prim[::-1], np.uint8)
    special[0, 2] = [(255, 0, k) for k in range(0, 32, 2)]                                   # hues just below 180
    special[0, 3] = [(255, k, 0) for k in range(0, 32, 2)]                                   # hues just above 0
    special[0, 4] = [(k, k, k + 1) for k in range(0, 64, 4)]                                 # nearly grey, dark
    special[0, 5:] = rng.integers(0, 256, (3, 16, 3))
    up = find_seed(lambda s: uniform(word(s, 0, 0, 4), 90) > 30)
    down = find_seed(lambda s: uniform(word(s, 0, 0, 4), 90) < -30)
    cases.append(case(special, up, 0, [ONE, 0, 20000, 20000, 90], None, "special pixels, hue up"))
    cases.append(case(special, down, 0, [ONE, 0, 20000, 20000, 90], None, "special pixels, hue down"))
    cases.append(case(special, 5, 1, FULL, (ONE, T[4]), "special pixels, every stage"))
    # the blur's own shapes: a constant image stays, an impulse gives the outer product of the taps, a ramp shows the reflection
    three = np.zeros((3, 17, 33, 3), np.uint8)
    three[0] = (201, 7, 255)
    three[1, 8, 16] = 255; three[1, 0, 0] = (255, 128, 1); three[1, 16, 32] = 77
    three[2] = (np.arange(33)[None, :, None] * 7 + np.arange(17)[:, None, None] * 2 + np.arange(3)[None, None, :]).astype(np.uint8)
    one_level = [taps_row(1.0, 4)]
    cases.append(case(three, 2, 0, None, (ONE, one_level), "blur Q1: constant, impulse, ramp"))
    cases.append(case(three, 2, 1, None, (ONE, T[7]), "blur Q16 R7: constant, impulse, ramp"))
    cases.append(case(img(2, 16, 32), 9, (1 << 48) - 1, FULL, (ONE, T[4]), "draw = 2^48 - 1"))

    # what the fixture promises, checked while it is written
    assert {"clamp", "hue wraps below 0", "hue wraps above 179"} <= SEEN, SEEN
    by = {c["note"]: c for c in cases}
    for note in ("gates 0: a copy", "no stage: a copy", "strengths 0: the input"):
        assert (by[note]["out_images"] == by[note]["images"]).all(), note
    assert by["strengths 0: the input"]["params"][:, 0].all()
    c = by["c16 = 0: flat at m"]
    assert c["params"][0, 1] == 0 and (c["out_images"] == c["params"][0, 5]).all()
    c = by["c16 = 131072: clamping"]
    assert c["params"][0, 1] == 131072 and (c["out_images"] == 0).any() and (c["out_images"] == 255).any()
    c = by["batch, images draw different gates"]
    assert len(set(c["params"][:, 0])) == 2 and len(set(c["params"][:, 6])) == 2
    c = by["blur Q1: constant, impulse, ramp"]
    assert (c["out_images"][0] == c["images"][0]).all()
    w = one_level[0]
    full = [w[abs(i)] for i in range(-4, 5)]
    for dy in range(-4, 5):
        for dx in range(-4, 5):
            assert c["out_images"][1, 8 + dy, 16 + dx, 0] == (255 * full[dy + 4] * full[dx + 4] + (1 << 21)) >> 22
    assert len({int(q) for cc in cases for q in cc["params"][:, 7]}) > 4
    assert any(cc["taps"].shape[0] == 1 for cc in cases) and any(cc["taps"].shape[0] == 16 for cc in cases)

    out = {"count": np.int64(len(cases))}
    for i, c in enumerate(cases):
        for name, v in c.items():
            out["c%02d_%s" % (i, name)] = np.asarray(v)
    path = os.path.join(os.path.dirname(os.path.abspath(__file__)), "strong_augment_cases.npz")
    np.savez_compressed(path, **out)
    print("%d cases, %d bytes -> %s" % (len(cases), os.path.getsize(path), path))


if __name__ == "__main__":
    main()
