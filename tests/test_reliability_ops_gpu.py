"""`fcn8s_op_reliability_pair` (csrc/reliability.hip) against `reliability.counts_numpy` on the same arrays.

calib, sums[0], sums[1], sums[3], hist and bad are compared with ==: the argmax, the bins, q_conf and the Brier fold are IEEE-exact in both
routes.  sums[2] (q_nll) may differ by at most the number of counted pixels: the device logf and NumPy's agree to 2 ulp, which moves one
pixel's rounded term by at most 1 at the scale 2^16 (a NumPy check over 2 M values, perturbing by +-1 and +2 ulp, gave max |delta| = 1).

Shapes are the smallest at which each path of the kernel can go wrong: pixel counts around the wave (64) and the tile (256), several tiles,
C = 20 (16-byte path with the next tile's loads in registers), C = 4, 8, 16, 60 (16-byte path at run-time C; 8 and 16 pad the row stride,
60 takes more than 64 KB of LDS), C = 19, 2 (generic path, rows that are not 16-byte aligned), C = 64, 67, 68 (rows too long for the LDS
image: read from global memory), a `prob` pointer off by one float, `gt` off by 1, 2, 3 bytes, and one pixel count past a full grid of the
kernel's block cap, where the grid-stride loop runs twice."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from fcn8s_tensorflow_amd import _lib as L, reliability as rel  # noqa: E402
from tests.test_reliability_host import edge_case  # noqa: E402

M = rel.SCORE_BINS
f32 = np.float32
NAMES = ("calib", "sums", "hist", "bad")


def dev_at(a, off=0):
    """A device copy of `a` (flat) whose first element lies `off` elements behind an allocation's (256-byte aligned) start."""
    flat = torch.from_numpy(np.array(a).reshape(-1))                      # a writable copy: the shared cases are read-only
    buf = torch.zeros(flat.numel() + off, dtype=flat.dtype, device="cuda")
    buf[off:].copy_(flat)
    return buf[off:]


def ptr(t):
    return C.c_void_p(t.data_ptr()) if t is not None else None


def call(prob, gt, lut, scores, scales, N, P, Cn, B, tables, J=None, stream=None):
    J = len(scores) if J is None else J
    ptrs = (C.c_void_p * max(len(scores), 1))(*[None if s is None else s.data_ptr() for s in scores])
    scl = (C.c_float * max(len(scales), 1))(*[float(s) for s in scales])
    return L.lib.fcn8s_op_reliability_pair(stream, ptr(prob), ptr(gt), ptr(lut), N, P, Cn, ptrs, scl, J, B, *[ptr(t) for t in tables])


def run(prob, gt, lut, scores, scales, B, prob_off=0, gt_off=0, tables=None):
    """prob [N,P,C], gt [N,P], scores [N,P] (NumPy) through the op; returns the tables as NumPy (and leaves `tables` on the device)."""
    N, P, Cn = prob.shape
    if tables is None:
        tables = rel.new_tables_device(B, len(scores), "cuda")
    keep = [dev_at(prob, prob_off), dev_at(gt, gt_off), dev_at(lut)] + [dev_at(s) for s in scores]
    L.check(call(keep[0], keep[1], keep[2], keep[3:], scales, N, P, Cn, B, tables))
    torch.cuda.synchronize()
    return tuple(t.cpu().numpy() for t in tables)


def softmax32(x):
    e = np.exp(x - x.max(-1, keepdims=True))
    return (e / e.sum(-1, keepdims=True)).astype(f32)


@functools.lru_cache(maxsize=None)
def case(N, P, Cn, J, B, seed=0):
    """Random softmaxes at mixed temperatures (confidences from 1 / C to 1.0), labels that are mostly valid classes with some ignored (255)
    and some >= C, scores with zeros, negatives and values past the last bin; and its reference, computed once."""
    rng = np.random.default_rng([seed, N, P, Cn, J])
    temp = rng.choice(np.array([0.3, 1.0, 4.0, 40.0], f32), (N, P, 1))
    prob = softmax32(rng.normal(0, 1, (N, P, Cn)).astype(f32) * temp)
    gt = rng.integers(0, Cn, (N, P)).astype(np.uint8)
    r = rng.random((N, P))
    gt[r < 0.10] = 255
    gt[(r >= 0.10) & (r < 0.13)] = Cn + 1 if Cn + 1 < 255 else Cn
    lut = rel.identity_lut()
    scores = []
    for j in range(J):
        s = (rng.random((N, P)) * 3.4).astype(f32)                       # score_max 3: some land past the last bin
        s[rng.random((N, P)) < 0.05] = 0.0
        s[rng.random((N, P)) < 0.05] = -0.5
        scores.append(s)
    scales = [f32(M) / f32(3.0 + j) for j in range(J)]
    ref = rel.counts_numpy(prob, gt, lut, scores, scales, B)
    for a in (prob, gt, lut, *scores, *ref):
        a.setflags(write=False)
    return prob, gt, lut, tuple(scores), tuple(scales), ref


def check(got, want, tag=""):
    counted = int(want[1][0])
    for g, w, name in zip(got, want, NAMES):
        if name == "sums":
            d = abs(int(g[2]) - int(w[2]))
            print("%s: %d counted pixels, q_nll device %d numpy %d (|difference| %d, allowed %d)" % (tag, counted, g[2], w[2], d, counted))
            assert (g[[0, 1, 3]] == w[[0, 1, 3]]).all(), (tag, name, g, w)
            assert d <= counted, (tag, "q_nll", d, counted)
        else:
            assert (g == w).all(), (tag, name, np.argwhere(g != w)[:8])
    # the three views of the same pixels agree
    assert got[0][:, 0].sum() == got[1][0] and all(got[2][j].sum() == got[1][0] for j in range(got[2].shape[0])), tag
    assert got[0][:, 1].sum() == got[1][1] and all(got[2][j, :, 0].sum() == got[1][1] for j in range(got[2].shape[0])), tag


@pytest.mark.parametrize("N", [1, 3])
@pytest.mark.parametrize("P", [1, 63, 64, 65, 255, 256, 257, 4099])
def test_pixel_counts_around_the_wave_and_the_tile(P, N):
    prob, gt, lut, scores, scales, ref = case(N, P, 20, 1, 15)
    check(run(prob, gt, lut, scores, scales, 15), ref, "N %d P %d" % (N, P))


@pytest.mark.parametrize("J", [0, 1, 3])
@pytest.mark.parametrize("Cn", [20, 19, 4, 2, 8, 16, 60, 64, 67, 68])
def test_class_counts_of_every_path(Cn, J):
    P = 4099 if Cn <= 20 else 517
    prob, gt, lut, scores, scales, ref = case(3, P, Cn, J, 15)
    check(run(prob, gt, lut, scores, scales, 15), ref, "C %d J %d" % (Cn, J))


@pytest.mark.parametrize("B", [1, 15, 64])
def test_confidence_bin_counts(B):
    prob, gt, lut, scores, scales, ref = case(3, 257, 20, 1, B)
    got = run(prob, gt, lut, scores, scales, B)
    check(got, ref, "B %d" % B)
    assert got[0].shape == (B, 3)


@pytest.mark.parametrize("prob_off,gt_off", [(1, 0), (0, 1), (0, 2), (0, 3), (1, 3), (2, 1), (3, 2)])
def test_any_alignment_of_prob_and_gt(prob_off, gt_off):
    for Cn in (20, 19):
        prob, gt, lut, scores, scales, ref = case(3, 257, Cn, 1, 15)
        check(run(prob, gt, lut, scores, scales, 15, prob_off=prob_off, gt_off=gt_off), ref, "C %d prob + %d floats, gt + %d bytes" % (Cn, prob_off, gt_off))


@pytest.mark.parametrize("Cn,J", [(20, 1), (19, 0), (4, 0)])
def test_one_partial_block_past_a_full_grid(Cn, J):
    """TILE_PIXELS * MAX_BLOCKS pixels fill every block of the kernel's largest grid once; 100 more give block 0 a second, partial trip."""
    P = rel.TILE_PIXELS * rel.MAX_BLOCKS + 100
    prob, gt, lut, scores, scales, ref = case(1, P, Cn, J, 15)
    check(run(prob, gt, lut, scores, scales, 15), ref, "C %d, %d pixels" % (Cn, P))


@pytest.mark.parametrize("Cn", [20, 19])
def test_identical_pixels_put_all_the_contention_on_one_bin(Cn):
    N, P = 2, 4099
    row = softmax32(np.linspace(-3, 3, Cn, dtype=f32)[None] * f32(2.0))[0]
    prob = np.broadcast_to(row, (N, P, Cn)).copy()
    gt = np.full((N, P), Cn - 1, np.uint8)
    s = [np.full((N, P), 0.0125, f32), np.full((N, P), 2.5, f32)]
    scales = [f32(M) / f32(3.0)] * 2
    ref = rel.counts_numpy(prob, gt, rel.identity_lut(), s, scales, 15)
    got = run(prob, gt, rel.identity_lut(), s, scales, 15)
    check(got, ref, "identical pixels, C %d" % Cn)
    assert (got[0][:, 0] != 0).sum() == 1 and all((got[2][j] != 0).sum() == 1 for j in range(3)) and got[1][0] == got[1][1] == N * P
    # ... and with every second pixel wrong, two entries per table
    gt[:, ::2] = 0
    check(run(prob, gt, rel.identity_lut(), s, scales, 15), rel.counts_numpy(prob, gt, rel.identity_lut(), s, scales, 15), "alternating, C %d" % Cn)


def test_ignored_pixels_leave_the_tables_untouched_and_out_of_range_ones_count_in_bad0_only():
    prob, gt, lut, scores, scales, _ = case(3, 257, 20, 1, 15)
    sentinel = lambda: tuple(torch.full(t.shape, 7, dtype=torch.int64, device="cuda") for t in rel.new_tables(15, 1))
    got = run(prob, np.full_like(gt, 255), lut, scores, scales, 15, tables=sentinel())
    assert all((g == 7).all() for g in got)
    ignore_all = np.full(256, 255, np.uint8)
    got = run(prob, gt, ignore_all, scores, scales, 15, tables=sentinel())
    assert all((g == 7).all() for g in got)
    got = run(prob, np.full_like(gt, 20), lut, scores, scales, 15, tables=sentinel())
    assert all((g == 7).all() for g in got[:3]) and got[3].tolist() == [7 + 3 * 257, 7]
    high = np.full(256, 254, np.uint8)                                   # the look-up table decides, not the label byte
    got = run(prob, gt, high, scores, scales, 15, tables=sentinel())
    assert all((g == 7).all() for g in got[:3]) and got[3].tolist() == [7 + 3 * 257, 7]


def test_the_edge_values_of_the_host_test():
    prob, gt, lut, scores, scales, B, _ = edge_case()
    ref = rel.counts_numpy(prob, gt, lut, scores, scales, B)
    got = run(prob[None], gt[None], lut, [scores[0][None]], scales, B)
    check(got, ref, "edge values")
    assert got[3].tolist() == [1, 3] and got[1][0] == 6 and got[0][15, 0] == 2 and got[0][8, 0] == 1 and got[2][1, 1023].sum() == 2


def test_two_calls_accumulate_and_two_runs_give_the_same_bits():
    a = case(3, 4099, 20, 1, 15, seed=0)
    b = case(3, 4099, 20, 1, 15, seed=1)
    one = run(*a[:5], 15)
    two = run(*b[:5], 15)
    tables = rel.new_tables_device(15, 1, "cuda")
    run(*a[:5], 15, tables=tables)
    both = run(*b[:5], 15, tables=tables)
    assert all((s == x + y).all() for s, x, y in zip(both, one, two))
    again = run(*a[:5], 15)
    assert all((x == y).all() for x, y in zip(one, again))


def test_engine_free_wrapper_takes_nhwc_tensors_and_the_current_stream():
    prob, gt, lut, scores, scales, ref = case(3, 4099, 20, 1, 15)
    t = lambda a, shape: torch.from_numpy(np.array(a)).cuda().reshape(shape)
    tables = rel.counts_device(t(prob, (3, 4099, 1, 20)), t(gt, (3, 4099, 1)), lut, [t(scores[0], (3, 4099, 1))], scales, 15)
    torch.cuda.synchronize()
    check(tuple(x.cpu().numpy() for x in tables), ref, "counts_device")
    ev = rel.Evaluator(bins=15, num_classes=20, score_names=("s",), score_max=3.0)
    for n in range(3):
        ev.add(t(prob[n], (1, 4099, 20)), t(gt[n], (1, 4099)), [t(scores[0][n], (1, 4099))])
    check(ev.tables(), ref, "Evaluator on the device")


def test_bad_arguments_return_their_code_and_touch_nothing():
    prob, gt, lut, scores, scales, _ = case(1, 65, 20, 1, 15)
    p, g, l, s = dev_at(prob), dev_at(gt), dev_at(lut), dev_at(scores[0])
    tables = tuple(torch.full(t.shape, 7, dtype=torch.int64, device="cuda") for t in rel.new_tables(64, 3))
    sc = float(scales[0])
    ok = dict(prob=p, gt=g, lut=l, scores=[s], scales=[sc], N=1, P=65, Cn=20, B=15, tables=tables)
    bad_arg = [dict(prob=None), dict(gt=None), dict(lut=None), dict(N=0), dict(N=-1), dict(P=0), dict(P=-5), dict(Cn=1), dict(Cn=0), dict(B=0),
               dict(B=65), dict(J=-1), dict(J=4), dict(scores=[None]), dict(scores=[s, None], scales=[sc, sc]),
               dict(scales=[0.0]), dict(scales=[-1.0]), dict(scales=[float('nan')]), dict(scales=[float('inf')])]
    bad_arg += [dict(tables=tables[:i] + (None,) + tables[i + 1:]) for i in range(4)]
    for kw in bad_arg:
        assert call(**{**ok, **kw}) == L.ERR_BAD_ARG, kw
    assert L.lib.fcn8s_op_reliability_pair(None, ptr(p), ptr(g), ptr(l), 1, 65, 20, None, None, 1, 15, *[ptr(t) for t in tables]) == L.ERR_BAD_ARG
    assert call(**{**ok, "P": 1 << 31}) == L.ERR_SHAPE
    torch.cuda.synchronize()
    assert all(bool((t == 7).all()) for t in tables)
    assert call(**ok) == L.OK                                            # the same arguments, unspoilt, are taken
    assert L.lib.fcn8s_op_reliability_pair(None, ptr(p), ptr(g), ptr(l), 1, 65, 20, None, None, 0, 15, *[ptr(t) for t in tables]) == L.OK
    torch.cuda.synchronize()
    assert int(tables[1][0]) > 7
