"""`fcn8s_op_temperature_nll` and `fcn8s_op_temperature_apply` (csrc/temperature.hip) against the float64 restatement in temperature.py.

The bar of temperature_nll.  The reference is `nll_numpy(..., float64)`; E is the largest per-pixel |float32 restatement - float64| * 2^16 on
the case's own inputs (tests/test_temperature_host.py: `e_units`); a counted pixel may differ from the reference by 8 E + 0.5 units -- the factor
8 is what the CRF and Monte-Carlo dropout tests allow a kernel that restates a definition in fp32, the 0.5 is the rintf -- and a table entry by
count times that.  count and bad are compared with ==.  Every case prints the multiple of E it needed.

Measured on the MI355X (the worst case of each test): a single pixel is off by at most 0.5 + 1.5 E units (E = 1.6 on that case, whose clamped
true classes carry terms of 87 beta); every table entry is off by less than the 0.5 of the rintf per counted pixel (0.43 at one pixel, at most
0.16 from 49 pixels on: the per-pixel differences cancel), so the tables need 0 E; temperature_apply needs 1.22 x its own float32-to-float64
distance for q and 1.5 x for the entropy; reliability_pair on the applied distribution differs from temperature_nll by 0.04 units per pixel.

Shapes are the smallest at which each path of the kernels can go wrong: pixel counts around the wave (64) and the tile (256), several tiles,
C = 20 (16-byte path, next tile's loads in registers), C = 4, 8, 16, 60 (16-byte path at run-time C), C = 19, 2 (generic path), C = 64, 67 (rows
read from global memory), `prob` off by one float, `gt` off by 1-3 bytes, one pixel count past a full grid, K = 1, 2, 31, 32 (every KB the
launcher instantiates is reached by K = 1, 2, 3, 8, 16, 31, 32)."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from fcn8s_tensorflow_amd import _lib as L, reliability as rel, temperature as ts  # noqa: E402
from tests.test_temperature_host import IDENTITY, case, e_units, grid_betas  # noqa: E402

f32 = np.float32
Q = ts.Q_NLL


def dev_at(a, off=0):
    """A device copy of `a` (flat) whose first element lies `off` elements behind an allocation's (256-byte aligned) start."""
    flat = torch.from_numpy(np.array(a).reshape(-1))                      # a writable copy: the shared cases are read-only
    buf = torch.zeros(flat.numel() + off, dtype=flat.dtype, device="cuda")
    buf[off:].copy_(flat)
    return buf[off:]


def ptr(t, byte_off=0):
    return C.c_void_p(t.data_ptr() + byte_off) if t is not None else None


def call_nll(prob, gt, lut, N, P, Cn, betas, tables, K=None, row=0, stream=None):
    """The raw op; tables: int64 [rows, K + 3] on the device, `row` is written."""
    b = np.asarray(betas, f32)
    K = b.size if K is None else K
    base = row * (b.size + 3) * 8
    has = tables is not None
    return L.lib.fcn8s_op_temperature_nll(stream, ptr(prob), ptr(gt), ptr(lut), N, P, Cn, b.ctypes.data_as(L._fp) if b.size else None, K,
                                          ptr(tables, base) if has else None, ptr(tables, base + 8 * b.size) if has else None,
                                          ptr(tables, base + 8 * (b.size + 1)) if has else None)


def run_nll(prob, gt, lut, betas, prob_off=0, gt_off=0, tables=None):
    """prob [N,P,C], gt [N,P] (NumPy) through the op; returns (nll [K], count, bad [2]) as NumPy."""
    N, P, Cn = prob.shape
    K = len(betas)
    if tables is None:
        tables = torch.zeros((1, K + 3), dtype=torch.int64, device="cuda")
    keep = [dev_at(prob, prob_off), dev_at(gt, gt_off), dev_at(lut)]
    L.check(call_nll(keep[0], keep[1], keep[2], N, P, Cn, betas, tables))
    torch.cuda.synchronize()
    t = tables.cpu().numpy()[0]
    return t[:K], int(t[K]), t[K + 1:]


@functools.lru_cache(maxsize=None)
def reference(N, P, Cn, K, seed=0, wrong_hot=False):
    """The case, its candidates, E and the float64 reference, computed once and shared."""
    prob, gt = case(N, P, Cn, seed=seed, wrong_hot=wrong_hot)
    betas = grid_betas(K)
    E, r32, r64 = e_units(prob, gt, IDENTITY, betas)
    return prob, gt, betas, E, r64


def check_nll(got, ref, tag):
    prob, gt, betas, E, (terms, _, count, bad) = ref
    nll, n, b = got
    assert n == count and (b == bad).all(), (tag, n, count, b, bad)
    want = terms.sum(0) * Q
    d = np.abs(nll.astype(np.float64) - want)
    allowed = count * (8 * E + 0.5)
    per = d.max() / max(count, 1)
    print("%s: %d counted pixels, bad %s, E = %.3f units, worst table entry off by %.3f units per pixel = 0.5 + %.3f E (allowed 0.5 + 8 E)"
          % (tag, count, bad.tolist(), E, per, max(per - 0.5, 0.0) / max(E, 1e-30)))
    assert (d <= allowed).all(), (tag, d.max(), allowed)


def test_single_pixel_calls_hold_every_pixel_to_the_bar_and_any_partition_gives_the_same_tables():
    prob, gt, betas, E, (terms, _, count, bad) = reference(1, 300, 20, 8, wrong_hot=True)
    K = betas.size
    p, g, l = dev_at(prob), dev_at(gt), dev_at(IDENTITY)
    rows = torch.zeros((300, K + 3), dtype=torch.int64, device="cuda")
    for i in range(300):
        L.check(L.lib.fcn8s_op_temperature_nll(None, ptr(p, i * 80), ptr(g, i), ptr(l), 1, 1, 20, betas.ctypes.data_as(L._fp), K,
                                               ptr(rows, i * (K + 3) * 8), ptr(rows, (i * (K + 3) + K) * 8), ptr(rows, (i * (K + 3) + K + 1) * 8)))
    torch.cuda.synchronize()
    r = rows.cpu().numpy()
    counted = r[:, K] == 1
    assert counted.sum() == count and (r[:, K + 1:].sum(0) == bad).all() and bad.min() > 0 and (r[~counted, :K] == 0).all()
    d = np.abs(r[counted, :K].astype(np.float64) - terms * Q)
    print("single pixels: E = %.3f units, the worst pixel is off by %.3f units = 0.5 + %.3f E (allowed 0.5 + 8 E)" % (E, d.max(), max(d.max() - 0.5, 0) / E))
    assert (d <= 8 * E + 0.5).all()
    assert (r[counted, :K] >= 0).all()
    whole = run_nll(prob, gt, IDENTITY, betas)
    assert (whole[0] == r[:, :K].sum(0)).all() and whole[1] == count and (whole[2] == bad).all()
    halves = torch.zeros((1, K + 3), dtype=torch.int64, device="cuda")
    run_nll(prob[:, :137], gt[:, :137], IDENTITY, betas, tables=halves)
    both = run_nll(prob[:, 137:], gt[:, 137:], IDENTITY, betas, tables=halves)
    assert (both[0] == whole[0]).all() and both[1] == whole[1] and (both[2] == whole[2]).all()


@pytest.mark.parametrize("N", [1, 3])
@pytest.mark.parametrize("P", [1, 63, 64, 65, 255, 256, 257, 4099])
def test_pixel_counts_around_the_wave_and_the_tile(P, N):
    ref = reference(N, P, 20, 8)
    check_nll(run_nll(ref[0], ref[1], IDENTITY, ref[2]), ref, "N %d P %d" % (N, P))


@pytest.mark.parametrize("Cn", [4, 8, 16, 60, 19, 2, 64, 67])
def test_class_counts_of_every_path(Cn):
    ref = reference(3, 4099 if Cn <= 20 else 517, Cn, 3)
    check_nll(run_nll(ref[0], ref[1], IDENTITY, ref[2]), ref, "C %d" % Cn)


@pytest.mark.parametrize("prob_off,gt_off", [(1, 0), (0, 1), (0, 2), (0, 3), (1, 3), (2, 1), (3, 2)])
def test_any_alignment_of_prob_and_gt(prob_off, gt_off):
    for Cn in (20, 19):
        ref = reference(3, 257, Cn, 3)
        check_nll(run_nll(ref[0], ref[1], IDENTITY, ref[2], prob_off=prob_off, gt_off=gt_off), ref, "C %d prob + %d floats, gt + %d bytes" % (Cn, prob_off, gt_off))


@pytest.mark.parametrize("Cn", [20, 19])
def test_one_partial_block_past_a_full_grid(Cn):
    """TILE_PIXELS * MAX_BLOCKS pixels fill every block of the kernel's largest grid once; 100 more give block 0 a second, partial trip."""
    ref = reference(1, ts.TILE_PIXELS * ts.MAX_BLOCKS + 100, Cn, 2)
    check_nll(run_nll(ref[0], ref[1], IDENTITY, ref[2]), ref, "C %d, %d pixels" % (Cn, ref[0].shape[1]))


@pytest.mark.parametrize("K", [1, 2, 16, 31, 32])
def test_candidate_counts(K):
    for Cn in (20, 19):
        ref = reference(3, 257, Cn, K)
        got = run_nll(ref[0], ref[1], IDENTITY, ref[2])
        check_nll(got, ref, "K %d C %d" % (K, Cn))
        assert got[0].shape == (K,) and (got[0] > 0).all()


def test_the_clamp_on_the_true_class_and_the_ends_of_the_beta_range():
    prob, gt = case(3, 257, 20, wrong_hot=True)
    betas = np.array([2.0 ** -6, 0.25, 1.0, 4.0, 2.0 ** 6], f32)
    E, _, r64 = e_units(prob, gt, IDENTITY, betas)
    check_nll(run_nll(prob, gt, IDENTITY, betas), (prob, gt, betas, E, r64), "beta 2^-6 .. 2^6, clamped true classes")


def test_ignored_pixels_leave_the_tables_untouched_and_out_of_range_ones_count_in_bad0_only():
    prob, gt, betas, _, _ = reference(3, 257, 20, 3)
    sentinel = lambda: torch.full((1, 6), 7, dtype=torch.int64, device="cuda")
    got = run_nll(prob, np.full_like(gt, 255), IDENTITY, betas, tables=sentinel())
    assert (got[0] == 7).all() and got[1] == 7 and (got[2] == 7).all()
    got = run_nll(prob, gt, np.full(256, 255, np.uint8), betas, tables=sentinel())
    assert (got[0] == 7).all() and got[1] == 7 and (got[2] == 7).all()
    got = run_nll(prob, gt, np.full(256, 254, np.uint8), betas, tables=sentinel())      # the look-up table decides, not the label byte
    assert (got[0] == 7).all() and got[1] == 7 and got[2].tolist() == [7 + 3 * 257, 7]


def test_two_calls_accumulate_and_two_runs_give_the_same_bits():
    a = reference(3, 4099, 20, 8, seed=0)
    b = reference(3, 4099, 20, 8, seed=1)
    one = run_nll(a[0], a[1], IDENTITY, a[2])
    two = run_nll(b[0], b[1], IDENTITY, b[2])
    tables = torch.zeros((1, 11), dtype=torch.int64, device="cuda")
    run_nll(a[0], a[1], IDENTITY, a[2], tables=tables)
    both = run_nll(b[0], b[1], IDENTITY, b[2], tables=tables)
    assert (both[0] == one[0] + two[0]).all() and both[1] == one[1] + two[1] and (both[2] == one[2] + two[2]).all()
    again = run_nll(a[0], a[1], IDENTITY, a[2])
    assert (again[0] == one[0]).all() and again[1] == one[1] and (again[2] == one[2]).all()
    run_nll(a[0], a[1], IDENTITY, a[2], tables=tables.zero_())
    twice = run_nll(a[0], a[1], IDENTITY, a[2], tables=tables)
    assert (twice[0] == 2 * one[0]).all() and twice[1] == 2 * one[1] and (twice[2] == 2 * one[2]).all()


def test_engine_free_wrapper_and_fitter_take_nhwc_tensors():
    ref = reference(3, 4099, 20, 8)
    prob, gt, betas = ref[:3]
    t = lambda a, shape: torch.from_numpy(np.array(a)).cuda().reshape(shape)
    tables = ts.nll_device(t(prob, (3, 4099, 1, 20)), t(gt, (3, 4099, 1)), IDENTITY, betas)
    torch.cuda.synchronize()
    got = tables.cpu().numpy()
    check_nll((got[:8], int(got[8]), got[9:]), ref, "nll_device")
    fitter = ts.Fitter(betas, IDENTITY, num_classes=20)
    for n in range(3):
        fitter.add(t(prob[n], (1, 4099, 20)), t(gt[n], (1, 4099)))
    nll, count, bad = fitter.result()
    assert (nll == got[:8]).all() and count == got[8] and (bad == got[9:]).all()
    with pytest.raises(ValueError):
        ts.nll_device(t(prob, (3, 4099, 20)), t(gt, (3, 4099)), IDENTITY, [100.0])
    with pytest.raises(ValueError):
        ts.nll_device(t(prob, (3, 4099, 20)), t(gt, (3, 4099)), IDENTITY, betas, tables=torch.zeros(5, dtype=torch.int64, device="cuda"))


def test_bad_arguments_return_their_code_and_touch_nothing():
    prob, gt, betas, _, _ = reference(1, 65, 20, 3)
    p, g, l = dev_at(prob), dev_at(gt), dev_at(IDENTITY)
    tables = torch.full((1, 6), 7, dtype=torch.int64, device="cuda")
    ok = dict(prob=p, gt=g, lut=l, N=1, P=65, Cn=20, betas=betas, tables=tables)
    bad_arg = [dict(prob=None), dict(gt=None), dict(lut=None), dict(tables=None), dict(N=0), dict(N=-1), dict(P=0), dict(P=-5), dict(Cn=1), dict(Cn=0),
               dict(K=0), dict(K=-1), dict(K=33), dict(betas=[1.0, 0.0, 2.0]), dict(betas=[-1.0]), dict(betas=[float('nan')]), dict(betas=[float('inf')]),
               dict(betas=[2.0 ** -7]), dict(betas=[64.5])]
    for kw in bad_arg:
        assert call_nll(**{**ok, **kw}) == L.ERR_BAD_ARG, kw
    for i in range(3):                                                   # each table pointer NULL in turn, and a NULL betas array
        tp = [ptr(tables), ptr(tables, 24), ptr(tables, 32)]
        tp[i] = None
        assert L.lib.fcn8s_op_temperature_nll(None, ptr(p), ptr(g), ptr(l), 1, 65, 20, betas.ctypes.data_as(L._fp), 3, *tp) == L.ERR_BAD_ARG
    assert L.lib.fcn8s_op_temperature_nll(None, ptr(p), ptr(g), ptr(l), 1, 65, 20, None, 3, ptr(tables), ptr(tables, 24), ptr(tables, 32)) == L.ERR_BAD_ARG
    assert call_nll(**{**ok, "P": 1 << 31}) == L.ERR_SHAPE
    out = torch.full((65 * 20,), 7.0, dtype=torch.float32, device="cuda")
    ent = torch.full((65,), 7.0, dtype=torch.float32, device="cuda")
    apply = lambda **kw: L.lib.fcn8s_op_temperature_apply(None, *[{**dict(prob=ptr(p), N=1, P=65, Cn=20, beta=0.5, out=ptr(out), ent=ptr(ent)), **kw}[k]
                                                                 for k in ("prob", "N", "P", "Cn", "beta", "out", "ent")])
    for kw in (dict(prob=None), dict(out=None, ent=None), dict(N=0), dict(P=0), dict(P=-1), dict(Cn=1), dict(beta=0.0), dict(beta=-1.0),
               dict(beta=float('nan')), dict(beta=float('inf')), dict(beta=100.0), dict(beta=0.001)):
        assert apply(**kw) == L.ERR_BAD_ARG, kw
    assert apply(P=1 << 31) == L.ERR_SHAPE
    torch.cuda.synchronize()
    assert bool((tables == 7).all()) and bool((out == 7).all()) and bool((ent == 7).all())
    assert call_nll(**ok) == L.OK and apply() == L.OK                    # the same arguments, unspoilt, are taken
    torch.cuda.synchronize()
    assert int(tables[0, 3]) > 7 and not bool((out == 7).any()) and not bool((ent == 7).any())


# ---- temperature_apply ----------------------------------------------------------------------------------------------------------------------
def run_apply(prob, beta, want_out=True, want_ent=True, in_place=False, prob_off=0):
    N, P, Cn = prob.shape
    p = dev_at(prob, prob_off)
    out = p if in_place else (torch.full((N * P * Cn + prob_off,), -7.0, dtype=torch.float32, device="cuda")[prob_off:] if want_out else None)
    ent = torch.full((N * P,), -7.0, dtype=torch.float32, device="cuda") if want_ent else None
    L.check(L.lib.fcn8s_op_temperature_apply(None, ptr(p), N, P, Cn, float(beta), ptr(out), ptr(ent)))
    torch.cuda.synchronize()
    return (out.cpu().numpy().reshape(N, P, Cn) if out is not None else None), (ent.cpu().numpy().reshape(N, P) if ent is not None else None)


def check_apply(q, h, prob, beta, tag):
    """q and h within 8 x the float32-to-float64 distance of apply_numpy on the case; sum_c q_c within C / 2 ulp of 1; rows with a non-finite
    entry NaN; the argmax kept wherever the float64 top-2 margin exceeds the bar."""
    q64, h64 = ts.apply_numpy(prob, beta, np.float64)
    q32, h32 = ts.apply_numpy(prob, beta, np.float32)
    fin = np.isfinite(prob).all(-1)
    Dq = np.abs(q32[fin].astype(np.float64) - q64[fin]).max()
    Dh = np.abs(h32[fin].astype(np.float64) - h64[fin]).max()
    Cn = prob.shape[-1]
    if q is not None:
        assert np.isnan(q[~fin]).all() and np.isfinite(q[fin]).all(), tag
        dq = np.abs(q[fin].astype(np.float64) - q64[fin]).max()
        print("%s: q off by %.3g = %.2f x the float32-to-float64 distance %.3g (allowed 8)" % (tag, dq, dq / Dq, Dq))
        assert dq <= 8 * Dq, (tag, dq, Dq)
        assert np.abs(q[fin].astype(np.float64).sum(-1) - 1).max() <= Cn / 2 * 2.0 ** -23, tag
        top = np.sort(q64[fin], -1)
        decidable = top[:, -1] - top[:, -2] > 16 * Dq                    # both candidates may move by the bar
        assert decidable.mean() >= 0.99, (tag, decidable.mean())
        assert (q[fin].argmax(-1)[decidable] == q64[fin].argmax(-1)[decidable]).all(), tag
        assert (q64[fin].argmax(-1)[decidable] == np.where(np.isfinite(prob), prob, -1)[fin].argmax(-1)[decidable]).all(), tag
    if h is not None:
        assert np.isnan(h[~fin]).all() and np.isfinite(h[fin]).all(), tag
        dh = np.abs(h[fin].astype(np.float64) - h64[fin]).max()
        print("%s: entropy off by %.3g = %.2f x the float32-to-float64 distance %.3g (allowed 8)" % (tag, dh, dh / Dh, Dh))
        assert dh <= 8 * Dh, (tag, dh, Dh)


@functools.lru_cache(maxsize=None)
def apply_case(N, P, Cn):
    """Softmaxes at mixed sharpness whose top two entries are apart (the argmax is then decidable at the bar), with spoilt rows."""
    rng = np.random.default_rng([7, N, P, Cn])
    z = rng.normal(0, 1, (N, P, Cn)) * rng.choice([0.3, 1.0, 4.0, 12.0], (N, P, 1))
    z[np.arange(N)[:, None], np.arange(P)[None, :], rng.integers(0, Cn, (N, P))] += 0.05 + np.abs(z).max(-1)
    e = np.exp(z - z.max(-1, keepdims=True))
    prob = (e / e.sum(-1, keepdims=True)).astype(f32)
    r = rng.random((N, P))
    prob[r < 0.01, 0] = np.nan
    prob[(r >= 0.01) & (r < 0.02), Cn - 1] = np.inf
    prob[(r >= 0.02) & (r < 0.03), 1] = -np.inf
    prob[(r >= 0.03) & (r < 0.05), Cn // 2] = 0.0
    prob.setflags(write=False)
    return prob


@pytest.mark.parametrize("beta", [0.4, 2.5])
@pytest.mark.parametrize("N,P,Cn", [(1, 1, 20), (1, 65, 20), (3, 257, 20), (3, 4099, 20), (3, 4099, 19), (3, 517, 8), (3, 517, 60), (3, 517, 2), (3, 517, 67)])
def test_apply_against_float64_in_place_and_each_output_alone(N, P, Cn, beta):
    prob = apply_case(N, P, Cn)
    tag = "N %d P %d C %d beta %.1f" % (N, P, Cn, beta)
    q, h = run_apply(prob, beta)
    check_apply(q, h, prob, beta, tag)
    qi, hi = run_apply(prob, beta, in_place=True)
    assert (qi.view(np.uint32) == q.view(np.uint32)).all() and (hi.view(np.uint32) == h.view(np.uint32)).all(), tag
    q1, none = run_apply(prob, beta, want_ent=False)
    assert none is None and (q1.view(np.uint32) == q.view(np.uint32)).all(), tag
    none, h1 = run_apply(prob, beta, want_out=False)
    assert none is None and (h1.view(np.uint32) == h.view(np.uint32)).all(), tag


def test_apply_one_partial_block_past_a_full_grid_and_an_unaligned_pointer():
    prob = apply_case(1, ts.TILE_PIXELS * ts.MAX_BLOCKS + 100, 20)
    q, h = run_apply(prob, 0.7, in_place=True)
    check_apply(q, h, prob, 0.7, "one pixel count past a full grid")
    prob = apply_case(3, 257, 20)
    q, h = run_apply(prob, 0.7)
    qo, ho = run_apply(prob, 0.7, prob_off=1)                          # the generic path computes the same row arithmetic
    assert (qo.view(np.uint32) == q.view(np.uint32)).all() and (ho.view(np.uint32) == h.view(np.uint32)).all()


def test_apply_device_wrapper_and_identity_at_temperature_one():
    prob = apply_case(3, 257, 20)
    dev = torch.from_numpy(np.array(prob)).cuda().reshape(3, 257, 1, 20)
    q, h = ts.apply_device(dev, 2.0, entropy=True)
    assert q.shape == dev.shape and h.shape == (3, 257, 1) and q.data_ptr() != dev.data_ptr()
    check_apply(q.cpu().numpy().reshape(3, 257, 20), h.cpu().numpy().reshape(3, 257), prob, 0.5, "apply_device, T = 2")
    same, none = ts.apply_device(dev, 2.0, out=dev)
    assert none is None and same.data_ptr() == dev.data_ptr() and (same.cpu().numpy().view(np.uint32) == q.cpu().numpy().view(np.uint32)).all()
    none, h2 = ts.apply_device(torch.from_numpy(np.array(prob)).cuda(), 2.0, entropy=True, out=False)
    assert none is None and (h2.cpu().numpy().view(np.uint32) == h.cpu().numpy().reshape(3, 257).view(np.uint32)).all()
    with pytest.raises(ValueError):
        ts.apply_device(dev, 2.0, out=False)
    with pytest.raises(ValueError):
        ts.apply_device(dev, 1000.0)


def test_reliability_pair_on_the_applied_distribution_reports_the_nll_that_temperature_nll_summed():
    """beta <= 1 keeps q_t of this case's sharpest rows a normal float (at beta > 1 it can underflow, where reliability_pair's own clamp at
    FLT_MIN caps its term at 87.3 and temperature_nll's 87.3 beta is the exact one)."""
    prob, gt = case(3, 4099, 20)
    betas = np.array([0.5, 0.7, 1.0], f32)
    E, _, r64 = e_units(prob, gt, IDENTITY, betas)
    nll, count, bad = run_nll(prob, gt, IDENTITY, betas)
    assert count == r64[2] and bad[1] > 0
    for k, beta in enumerate(betas):
        q, _ = run_apply(prob, beta, want_ent=False)
        tables = rel.counts_device(torch.from_numpy(q).cuda(), torch.from_numpy(np.array(gt)).cuda(), IDENTITY, bins=15)
        torch.cuda.synchronize()
        sums, rbad = tables[1].cpu().numpy(), tables[3].cpu().numpy()
        assert sums[0] == count and (rbad == bad).all()                  # the NaN rows of apply are reliability_pair's bad[1]
        d = abs(int(sums[2]) - int(nll[k]))
        print("beta %.2f: q_nll of reliability_pair %d, temperature_nll %d: %.3f units per pixel (allowed 8 E + 1 = %.3f)" % (beta, sums[2], nll[k], d / count, 8 * E + 1))
        assert d <= count * (8 * E + 1)
