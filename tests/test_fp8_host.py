"""The host restatement of the 'fp8_infer' arithmetic (fcn8s_tensorflow_amd/fp8.py): q(v) and E(a), checked against an independent
round-to-nearest-even over the table of e4m3 values.  No GPU."""
import math

import numpy as np
import torch

from fcn8s_tensorflow_amd import fp8


def e4m3_table():
    """(finite non-negative e4m3 values ascending, their codes), decoded by hand from the OCP E4M3FN bit layout."""
    vals, codes = [], []
    for c in range(128):
        e, m = (c >> 3) & 15, c & 7
        if e == 15 and m == 7:
            continue                                             # NaN
        vals.append(math.ldexp(1 + m / 8, e - 7) if e else math.ldexp(m, -9))
        codes.append(c)
    return np.array(vals), np.array(codes)


def ref_code(v):
    """clamp to [-448, 448], round to nearest e4m3, ties to the even code -- from the table, not from torch."""
    vals, codes = e4m3_table()
    s = 128 if (v < 0 or (v == 0 and math.copysign(1.0, v) < 0)) else 0
    a = min(abs(float(v)), 448.0)
    i = int(np.searchsorted(vals, a))
    if i < len(vals) and vals[i] == a:
        return s | int(codes[i])
    lo, hi = i - 1, i
    dl, dh = a - vals[lo], vals[hi] - a
    pick = lo if dl < dh else hi if dh < dl else (lo if codes[lo] % 2 == 0 else hi)
    return s | int(codes[pick])


def sweep():
    vals, _ = e4m3_table()
    v32 = vals.astype(np.float32)
    mids = ((vals[:-1] + vals[1:]) / 2).astype(np.float32)           # exact in fp32: five significant bits
    pts = [v32, mids,
           np.nextafter(v32, np.float32(np.inf)), np.nextafter(v32, np.float32(-np.inf)),
           np.nextafter(mids, np.float32(np.inf)), np.nextafter(mids, np.float32(-np.inf)),
           np.array([448, 449, 464, 465, 500, 1e6, 3.0e38, 2.0 ** -10, 2.0 ** -11, 3 * 2.0 ** -11, 1e-30, 1e-45], np.float32)]
    p = np.concatenate(pts)
    p = p[np.isfinite(p) & (p >= 0)]
    return np.concatenate([p, -p, np.array([0.0, -0.0], np.float32)]).astype(np.float32)


def test_q_is_clamp_then_round_to_nearest_even():
    x = sweep()
    got = fp8.codes(torch.from_numpy(x)).numpy()
    want = np.array([ref_code(v) for v in x], np.uint8)
    bad = np.nonzero(got != want)[0]
    assert bad.size == 0, [(float(x[i]), int(got[i]), int(want[i])) for i in bad[:10]]
    # values: q(v) is the decoded code, and the explicit clamp keeps everything finite (torch alone turns 500.0 into NaN)
    qv = fp8.q(x)
    assert np.isfinite(qv).all() and np.abs(qv).max() == 448.0
    assert np.isnan(torch.tensor([500.0]).to(torch.float8_e4m3fn).float().item())


def test_q_ties_go_to_the_even_code():
    # 1 + 1/16 lies halfway between 1 (code 0x38) and 1.125 (0x39): even wins; 1 + 3/16 between 0x39 and 0x3a: 0x3a
    assert fp8.codes(torch.tensor([1.0625, 1.1875, 2 ** -10, 3 * 2 ** -10])).tolist() == [0x38, 0x3a, 0x00, 0x02]


def test_exponent_at_and_around_the_boundaries():
    for e in range(-20, 21):
        a = np.float32(math.ldexp(448.0, e))
        assert fp8.exponent(a) == e
        assert fp8.exponent(np.nextafter(a, np.float32(np.inf))) == e + 1
        assert fp8.exponent(np.nextafter(a, np.float32(0))) == e
    assert fp8.exponent(0.0) == 0
    sub = np.float32(1e-40)                                          # an fp32 subnormal
    e = fp8.exponent(sub)
    assert sub <= math.ldexp(448.0, e) and sub > math.ldexp(448.0, e - 1)
    assert fp8.exponent(np.float32(2.0 ** -149)) == -157             # 448 2^-157 = 1.75 2^-149 >= 2^-149 > 448 2^-158


def test_weight_quantization_is_exact_per_column():
    rng = np.random.default_rng(0)
    w = (rng.standard_normal((3, 3, 64, 8)) * np.logspace(-3, 2, 8)).astype(np.float32)
    wq, ew = fp8.quantize_weights(w)
    wq = wq.numpy()
    for co in range(8):
        a = np.abs(w[..., co]).max()
        assert ew[co] == fp8.exponent(a)
        col = w[..., co] * np.float32(2.0 ** -ew[co])
        assert np.abs(col).max() <= 448.0
        np.testing.assert_array_equal(wq[..., co], fp8.q(col))
