"""conv1_2's fused forward kernel (csrc/wino_fused64.hip: wino_gemm_out64_kernel -- the 64 position GEMMs of F(6x6,3x3), output transform, bias,
ReLU and the 2x2/2 max-pool with its argmax bytes) at op level, against float64 torch on the same fp32 inputs.

fcn8s_op_conv3x3_winograd_pool runs the model's own conv_fwd on a bare model; the op context "op_gemm_out_fused64" (0 = position GEMM + output
transform, 1 = ask for the fused kernel, 2 = the same with its non-temporal-store instantiation) picks the route, and the entry reports whether the
kernel was launched.  Channels are 64 -> 64 and the tile is 6 throughout (the only shape class the kernel takes).  Every scratch buffer of the entry is
NaN before the call, and every tensor the entry sees is tests/hostile.py's: x, k, b fenced by NaN bands and checked intact, `pool` / `pidx` all 0xFF
bytes inside their bands until written.

Shapes (N, H, W) and the tile count T = N ceil(H / 6) ceil(W / 6); one block of the kernel owns 16 tiles:
  (1, 2, 2)     T = 1    one partial tile, one window: fifteen of the block's sixteen rows are clamped to tile T - 1
  (1, 12, 12)   T = 4    no partial tiles
  (1, 24, 24)   T = 16   exactly one full block
  (1, 6, 102)   T = 17   a second block that owns one tile
  (5, 6, 6)     T = 5    every tile is its own image
  (2, 34, 22)   T = 48   exactly three blocks, the image boundary in mid-block (the existing op shape of test_ops_gpu.py, twice)
  (3, H, W) for H in (12, 14, 16), W in (18, 20, 22): T = 18 .. 36, all nine (H % 6, W % 6) combinations, blocks straddle images

Bounds: 1e-4 of the largest reference value for fp32 F(6x6,3x3) against float64 (test_ops_gpu.py, header of winograd.hip); 2e-5 max(1, max |pool|)
between the two routes (test_gemm_out_fused64_gpu.py: they differ in the summation order of a 64-term chain alone); the argmax bytes are held to a
rule evaluated on the float64 pre-activation, outside windows the REFERENCE alone calls ambiguous at 1e-4 max(1, max |z|).

Measured on the MI355X: LABNOTES.md, section 0c."""
import contextlib
import ctypes as C
import functools

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from oracle import fcn8s_oracle as orc  # noqa: E402  (checker only)
from tests import hostile  # noqa: E402
from tests.hostile import inp, out  # noqa: E402
from tests.test_ops_gpu import check_conv3x3_winograd_backward, rel_err  # noqa: E402

CH = 64
TILE = 6
UNWRITTEN = 0xFF                                                                           # a byte of `pidx` no kernel stored
EDGE_SHAPES = tuple((3, h, w) for h in (12, 14, 16) for w in (18, 20, 22))
SHAPES = ((1, 2, 2), (1, 12, 12), (1, 24, 24), (1, 6, 102), (5, 6, 6), (2, 34, 22)) + EDGE_SHAPES
BWD_CASES = (((1, 34, 22), 2), ((3, 14, 20), 1), ((1, 12, 12), 0), ((1, 6, 102), 1))     # (shape, mask_mode)
BANK_PAIRS = ((0, 0), (3, 17), (21, 5), (38, 63), (63, 42), (16, 16))                      # (ci, co) over the index fields of the MFMA-ordered bank
OPTION = b"op_gemm_out_fused64"


def lib():
    from fcn8s_tensorflow_amd import _lib
    return _lib


@pytest.fixture(autouse=True)
def hostile_memory():
    """tests/hostile.py's memory for every test (check_conv3x3_winograd_backward draws on it too): NaN scratch pools, verify() at the end"""
    with hostile.session(lib()) as arena:
        yield arena


def ptr(t):
    return C.c_void_p(t.data_ptr()) if t is not None else None


def tiles(n, h, w):
    return n * ((h + 5) // 6) * ((w + 5) // 6)


@contextlib.contextmanager
def op_context(**options):
    """Set op-context options of this thread; every one of them is put back on the way out."""
    L = lib()
    saved = {}
    try:
        for k, v in options.items():
            cur = C.c_int64(-1)
            L.check(L.lib.fcn8s_get_option(None, k.encode(), C.byref(cur)))
            saved[k] = cur.value
            L.check(L.lib.fcn8s_set_option(None, k.encode(), v))
        yield
    finally:
        for k, v in saved.items():
            L.lib.fcn8s_set_option(None, k.encode(), v)


@functools.lru_cache(maxsize=None)
def inputs(n, h, w):
    rng = np.random.default_rng(41)
    x = rng.standard_normal((n, h, w, CH)).astype(np.float32)
    k = (rng.standard_normal((3, 3, CH, CH)) / np.sqrt(576)).astype(np.float32)
    b = (0.3 * rng.standard_normal(CH)).astype(np.float32)
    for a in (x, k, b):
        a.setflags(write=False)
    return x, k, b


def windows(z):
    """[n, h, w, c] -> [n, h/2, w/2, c, 4], the last axis in the order (0,0), (0,1), (1,0), (1,1): index 2 dy + dx."""
    n, h, w, c = z.shape
    return z.reshape(n, h // 2, 2, w // 2, 2, c).transpose(0, 1, 3, 5, 2, 4).reshape(n, h // 2, w // 2, c, 4)


def reference_of(x, k, b):
    """float64: the pre-activation z (NHWC), the pool of its ReLU, the bytes of the rule, and the windows round-off may decide.
      byte       2 dy + dx of the FIRST maximum of the ReLU'd window; 4 where that maximum is not > 0
      ambiguous  the two largest ReLU'd entries closer than tol while the largest is > 0, or |max| below tol; tol = 1e-4 max(1, max |z|)"""
    z = orc.conv2d_same_t(torch.tensor(x).permute(0, 3, 1, 2).double(), torch.tensor(k).double(), torch.tensor(b).double())
    z = z.permute(0, 2, 3, 1).contiguous().numpy()
    win = windows(z)
    r = np.maximum(win, 0.0)
    pool = r.max(-1)
    byte = np.where(pool > 0, r.argmax(-1), 4).astype(np.uint8)         # (argmax: the first of equal maxima)
    tol = 1e-4 * max(1.0, float(np.abs(z).max()))
    srt = np.sort(r, -1)
    amb = ((srt[..., 3] - srt[..., 2] < tol) & (srt[..., 3] > 0)) | (np.abs(win.max(-1)) < tol)
    return dict(z=z, pool=pool, byte=byte, amb=amb)


@functools.lru_cache(maxsize=None)
def reference(n, h, w):
    return reference_of(*inputs(n, h, w))


def call(x, k, b, option, train, f32x3=0):
    """One fcn8s_op_conv3x3_winograd_pool call under the given op context, on the current test's arena: pool and pidx all 0xFF bytes (NaN /
    UNWRITTEN) inside their bands; an inference pass must leave pidx alone.  Returns the pool, the bytes, the entry's `fused` report and
    whether the arena verifies (bands and fences whole, inputs intact, every pool element written) -- the fixture verifies again at the end."""
    L = lib()
    n, h, w, _ = x.shape
    shape = (n, h // 2, w // 2, CH)
    xd, kd, bd = inp(x, "x"), inp(k, "k"), inp(b, "b")
    pool, pidx = out(shape, name="pool"), out(shape, torch.uint8, name="pidx", untouched=not train)
    fused = C.c_int(-1)
    torch.cuda.synchronize()
    with op_context(op_gemm_out_fused64=option, op_f32x3=f32x3):
        L.check(L.lib.fcn8s_op_conv3x3_winograd_pool(None, ptr(xd), ptr(kd), ptr(bd), ptr(pool), ptr(pidx), n, h, w, CH, CH, TILE, train, C.byref(fused)))
    torch.cuda.synchronize()
    try:
        hostile.current().verify()
        bands = True
    except hostile.HostileMemoryError as e:
        print(e)
        bands = False
    return dict(pool=pool.cpu().numpy(), byte=pidx.cpu().numpy(), fused=fused.value, bands=bands)


@functools.lru_cache(maxsize=None)
def run(n, h, w, option, train):
    """The seeded case of a shape (shared by the tests, never modified)."""
    return call(*inputs(n, h, w), option, train)


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def relu_bias(b, shape):
    """What a convolution of nothing leaves behind: max(b, 0) in every pooled element, the bytes 0 where b > 0 and 4 elsewhere."""
    return np.broadcast_to(np.maximum(b, np.float32(0)), shape), np.broadcast_to(np.where(b > 0, 0, 4).astype(np.uint8), shape)


def assert_relu_bias(got, b, what):
    pool, byte = relu_bias(b, got["pool"].shape)
    assert np.array_equal(bits(got["pool"]), bits(pool)), what
    assert np.array_equal(got["byte"], byte), what


# ---- 1. values --------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,h,w", SHAPES)
def test_pool_against_float64_on_both_routes(n, h, w):
    ref = reference(n, h, w)["pool"]
    f1, f0, u1, u0 = run(n, h, w, 1, 1), run(n, h, w, 1, 0), run(n, h, w, 0, 1), run(n, h, w, 0, 0)
    assert (f1["fused"], f0["fused"], u1["fused"], u0["fused"]) == (1, 1, 0, 0)
    ef, eu = rel_err(f1["pool"], ref), rel_err(u1["pool"], ref)
    d = float(np.abs(f1["pool"].astype(np.float64) - u1["pool"]).max())
    tol = 2e-5 * max(1.0, float(np.abs(u1["pool"]).max()))
    print("%d x %dx%d (T = %d): against float64 fused %.3g, two kernels %.3g (of max |ref| = %.3g); fused - two kernels %.3g (tolerance %.3g)"
          % (n, h, w, tiles(n, h, w), ef, eu, float(np.abs(ref).max()), d, tol))
    assert ef < 1e-4 and eu < 1e-4
    assert d <= tol
    # an inference pass (V in the shared scratch, no bytes) computes the training pass's bits
    assert np.array_equal(bits(f0["pool"]), bits(f1["pool"]))
    assert np.array_equal(bits(u0["pool"]), bits(u1["pool"]))


def test_fused_error_is_at_most_twice_the_two_kernel_error_over_all_shapes():
    """Both routes are 64-term fp32 chains with one worst-case bound.  Over all shapes together: one case of 64 windows is too small a sample."""
    ef = max(float(np.abs(run(*s, 1, 1)["pool"] - reference(*s)["pool"]).max()) for s in SHAPES)
    eu = max(float(np.abs(run(*s, 0, 1)["pool"] - reference(*s)["pool"]).max()) for s in SHAPES)
    print("largest |pool - float64| over %d shapes: fused %.3g, two kernels %.3g" % (len(SHAPES), ef, eu))
    assert ef <= 2.0 * eu


# ---- 2. bytes ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,h,w", SHAPES)
def test_the_reference_leaves_few_windows_to_round_off(n, h, w):
    """The reference alone.  Measured with this recipe on the CPU: 0 to 0.091 % of a shape's windows are ambiguous (11 of 12096 at 3 x 14x18);
    0.2 % is a cap on what the byte comparisons may exclude, not a tolerance."""
    amb = reference(n, h, w)["amb"]
    print("%d x %dx%d: %d of %d windows ambiguous" % (n, h, w, int(amb.sum()), amb.size))
    assert amb.mean() <= 2e-3


@pytest.mark.parametrize("n,h,w", SHAPES)
def test_dead_windows_are_well_represented(n, h, w):
    """The reference alone.  Byte 4 (a maximum that is not > 0): about 8 to 9 % of the windows, at least 5 % of every shape's."""
    dead = reference(n, h, w)["byte"] == 4
    print("%d x %dx%d: %d of %d windows dead" % (n, h, w, int(dead.sum()), dead.size))
    assert dead.mean() >= 0.05


@pytest.mark.parametrize("n,h,w", SHAPES)
def test_bytes_against_the_rule(n, h, w):
    ref = reference(n, h, w)
    f, u = run(n, h, w, 1, 1), run(n, h, w, 0, 1)
    off_rule, off_route = f["byte"] != ref["byte"], f["byte"] != u["byte"]
    print("%d x %dx%d: %d of %d fused bytes off the rule, %d differ between the routes, %d windows ambiguous, %d dead"
          % (n, h, w, int(off_rule.sum()), off_rule.size, int(off_route.sum()), int(ref["amb"].sum()), int((f["byte"] == 4).sum())))
    assert f["byte"].max() <= 4
    assert not (off_rule & ~ref["amb"]).any()
    assert not ((u["byte"] != ref["byte"]) & ~ref["amb"]).any()
    assert not (off_route & ~ref["amb"]).any()
    # the kernel's own consistency: byte 4 exactly where the pooled value is not > 0
    assert np.array_equal(f["byte"] == 4, ~(f["pool"] > 0))


# ---- 3. nothing stray -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,h,w", SHAPES)
def test_nothing_stray_is_written_or_read(n, h, w):
    """The bands around pool and pidx are untouched, every element inside is written, and no NaN of the scratch (V rows beyond T, M, the bank
    behind its last float) reaches the pool."""
    for option in (1, 2, 0):
        for train in (1, 0):
            r = run(n, h, w, option, train) if option != 2 else call(*inputs(n, h, w), 2, train)
            what = (option, train)
            assert r["fused"] == (option != 0), what
            assert r["bands"], what
            assert np.isfinite(r["pool"]).all(), what
            if train:
                assert not (r["byte"] == UNWRITTEN).any() and r["byte"].max() <= 4, what
            else:
                assert (r["byte"] == UNWRITTEN).all(), what                 # an inference pass writes no bytes


# ---- 4. exact cases ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,h,w", SHAPES)
def test_zero_filter_gives_the_relu_of_the_bias_bit_for_bit(n, h, w):
    x, k, b = inputs(n, h, w)
    r = call(x, np.zeros_like(k), b, 1, 1)
    assert r["fused"] == 1
    assert_relu_bias(r, b, (n, h, w))


@pytest.mark.parametrize("n,h,w,live", [(3, 14, 20, 0), (3, 14, 20, 1), (3, 14, 20, 2), (5, 6, 6, 2)])
def test_an_empty_image_gives_the_relu_of_the_bias_bit_for_bit(n, h, w, live):
    """x is non-zero in one image only: every other image's tiles multiply zeros, whichever block and rows they sit in.  The tile-to-image
    bookkeeping (n, ty, tx from a flat tile index), pinned exactly, not to round-off."""
    x, k, b = inputs(n, h, w)
    x1 = np.zeros_like(x); x1[live] = x[live]
    r = call(x1, k, b, 1, 1)
    assert r["fused"] == 1
    for i in range(n):
        one = dict(pool=r["pool"][i], byte=r["byte"][i])
        if i != live:
            assert_relu_bias(one, b, (n, h, w, live, i))
    full = run(n, h, w, 1, 1)                                            # the live image: its bits in the full batch
    assert np.array_equal(bits(r["pool"][live]), bits(full["pool"][live]))
    assert np.array_equal(r["byte"][live], full["byte"][live])
    assert not np.array_equal(bits(r["pool"][live]), bits(relu_bias(b, r["pool"][live].shape)[0]))


# ---- 5. placement invariance ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("h,w", [(14, 20), (16, 22)])
def test_an_image_does_not_depend_on_its_batch(h, w):
    x, k, b = inputs(3, h, w)
    three = run(3, h, w, 1, 1)
    for i in range(3):
        one = call(x[i:i + 1], k, b, 1, 1)
        assert one["fused"] == 1
        assert np.array_equal(bits(one["pool"][0]), bits(three["pool"][i])), i
        assert np.array_equal(one["byte"][0], three["byte"][i]), i


@pytest.mark.parametrize("n,h,w", [(3, 14, 20), (1, 2, 2)])
def test_non_temporal_stores_change_no_bit(n, h, w):
    a, nt = run(n, h, w, 1, 1), call(*inputs(n, h, w), 2, 1)
    assert nt["fused"] == 1
    assert np.array_equal(bits(a["pool"]), bits(nt["pool"]))
    assert np.array_equal(a["byte"], nt["byte"])


@pytest.mark.parametrize("n,h,w", [(2, 34, 22), (1, 6, 102)])
def test_two_identical_calls_give_identical_bits(n, h, w):
    a, b = run(n, h, w, 1, 1), call(*inputs(n, h, w), 1, 1)
    assert np.array_equal(bits(a["pool"]), bits(b["pool"]))
    assert np.array_equal(a["byte"], b["byte"])


# ---- 6. the MFMA-ordered second filter bank ---------------------------------------------------------------------------------------------
def swap_low_fields(c):
    """Bits 0-1 and 2-3 of a channel index exchanged."""
    return (c & 0x30) | ((c & 3) << 2) | ((c >> 2) & 3)


@pytest.mark.parametrize("ci,co", BANK_PAIRS)
def test_second_filter_bank_places_every_channel_pair(ci, co):
    """u_mfma64[pos][kc][nb][lane][s] = U[pos][16 kc + 4 (lane / 16) + s][16 nb + lane % 16], written by wino_filter_kernel: one live input channel
    against a filter with one live (ci, co) pair.  Matched, only output channel co moves off max(b, 0); unmatched, nothing does -- exactly."""
    n, h, w = 1, 14, 20
    x, k, b = inputs(n, h, w)
    k1 = np.zeros_like(k); k1[:, :, ci, co] = 8.0 * k[:, :, ci, co]          # (8 = sqrt(64): one channel carries a whole layer's signal)

    def one_channel(c):
        x1 = np.zeros_like(x); x1[..., c] = x[..., c]
        return x1
    r = call(one_channel(ci), k1, b, 1, 1)
    assert r["fused"] == 1
    ref = reference_of(one_channel(ci), k1, b)
    others = np.arange(CH) != co
    rest = dict(pool=r["pool"][..., others], byte=r["byte"][..., others])
    assert_relu_bias(rest, b[others], (ci, co))
    e = rel_err(r["pool"], ref["pool"])
    print("(ci, co) = (%d, %d): against float64 %.3g" % (ci, co, e))
    assert e < 1e-4
    floor = max(float(b[co]), 0.0)
    above = ref["pool"][..., co] > floor + 1e-4 * np.abs(ref["pool"]).max()      # where float64 says so beyond the bound
    assert above.mean() > 0.25 and (r["pool"][..., co][above] > floor).all()
    for c in sorted({ci ^ 1, ci ^ 4, ci ^ 16, swap_low_fields(ci)} - {ci}):
        m = call(one_channel(c), k1, b, 1, 1)
        assert m["fused"] == 1
        assert_relu_bias(m, b, (ci, co, c))


# ---- 7. the backward pass on this forward -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape,mask_mode", BWD_CASES)
def test_backward_reads_the_fused_forward(shape, mask_mode):
    """fcn8s_op_conv3x3_winograd_fwd_bwd (y = NULL, pooled) with the op context on: test_conv3x3_winograd_backward's checker, near-tie zeroing of dy
    and 1e-4 bounds on dx, dw, db -- the gradients routed by the bytes wino_gemm_out64_kernel wrote.  That the route ran there: the pool it
    returns is the fused pool of fcn8s_op_conv3x3_winograd_pool for the same inputs, bit for bit."""
    n, h, w = shape
    with op_context(op_gemm_out_fused64=1):
        pool = check_conv3x3_winograd_backward(n, h, w, CH, CH, TILE, 1, mask_mode, inputs=tuple(np.array(a) for a in inputs(n, h, w)))
    f, u = run(n, h, w, 1, 1), run(n, h, w, 0, 1)
    assert f["fused"] == 1 and u["fused"] == 0
    assert np.array_equal(bits(pool), bits(f["pool"]))
    if pool.size >= 1000:
        assert not np.array_equal(bits(pool), bits(u["pool"]))           # (the two routes do differ in their last bits: the equality above says something)


# ---- 8. declining -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,h,w", [(3, 14, 20), (1, 2, 2)])
def test_the_split_bf16_arithmetic_declines_and_returns_the_two_kernel_bits(n, h, w):
    x, k, b = inputs(n, h, w)
    for train in (1, 0):
        asked, plain = call(x, k, b, 1, train, f32x3=1), call(x, k, b, 0, train, f32x3=1)
        assert asked["fused"] == 0 and plain["fused"] == 0
        assert np.array_equal(bits(asked["pool"]), bits(plain["pool"]))
        assert np.array_equal(asked["byte"], plain["byte"])
        assert asked["bands"] and np.isfinite(asked["pool"]).all()
        assert rel_err(asked["pool"], reference(n, h, w)["pool"]) < 1e-4


def test_option_values_outside_0_1_2_are_refused():
    L = lib()
    cur = C.c_int64(-1)
    with op_context(op_gemm_out_fused64=2):
        for bad in (3, -1):
            with pytest.raises(ValueError):
                L.check(L.lib.fcn8s_set_option(None, OPTION, bad))
            L.check(L.lib.fcn8s_get_option(None, OPTION, C.byref(cur)))
            assert cur.value == 2
    L.check(L.lib.fcn8s_get_option(None, OPTION, C.byref(cur)))
    assert cur.value == 0                                                # the default, restored
