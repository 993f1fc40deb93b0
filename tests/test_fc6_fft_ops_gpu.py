"""fc6's fp32 training path at op level: one 7x7 SAME convolution, forward + weight gradient + data gradient, through the model's own launch
sequences (fcn8s_op_conv7x7_fc6_fwd_bwd) against float64 torch on the same fp32 inputs -- on the 14x14 real-DFT tiles (csrc/fft_fc6.hip + the
292-plane batched GEMMs), on F(4x4,4x4) and on the direct kernels, at the shapes where tiles are partial, patches overlap, a plane has more
than one 128-row GEMM tile, and the three products do not all run in the same domain.  The op fills its scratch with NaNs first, so a kernel
that lets a slab's skew, a row beyond T or a stale plane reach a result fails here.

The bar for y, dx, dw and db on every path is 2e-5 of the reference tensor's largest magnitude, the fp32 op bar of test_conv2d_fwd_bwd: fp32
summation order alone stays at or below 1.6e-6 on shapes of this class (float32 NumPy DFT forward, float32 direct dx / dw against float64).

Measured on an MI355X (worst over the cases, error / max |reference|, y / dx / dw / db): path 2 4.2e-6 / 3.8e-6 / 2.7e-6 / 1.3e-7, path 1
4.2e-6 / 3.8e-6 / 9.9e-6 / 2.3e-7, path 0 8.3e-6 / 5.5e-6 / 9.9e-6 / 2.3e-7; the products that ran in the DFT domain 2.7e-7 / 4.3e-7 / 4.2e-7
(the DFT weight gradient at T = 135: 3.6e-7), the rest is F(4x4,4x4) and the direct kernels.  Every test prints its figures."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

from tests import hostile  # noqa: E402
from tests.hostile import inp, out  # noqa: E402
from tests.test_ops_gpu import _lib, ptr, rel_err  # noqa: E402


@pytest.fixture(autouse=True)
def hostile_memory():
    """tests/hostile.py's memory for every test: fenced inputs checked intact, outputs NaN until written, NaN scratch pools, verify() at the end"""
    with hostile.session(_lib()) as arena:
        yield arena


BAR = 2e-5

# N, H, W, Cin, Cout, the products that run in the DFT domain on path 2 (bit 0 forward, bit 1 weight gradient, bit 2 data gradient)
CASES = [
    (1, 3, 3, 64, 128, 7),        # T = 1: the smallest map the rule sends to the DFT tiles, the patch mostly padding, a reduction over one tile
    (1, 8, 8, 64, 128, 7),        # T = 1: one whole tile
    (2, 5, 9, 64, 128, 7),        # T = 4: the map shorter than a tile, the second tile column one pixel wide
    (1, 7, 15, 64, 384, 7),       # T = 2: Cout = 3 x 128, one row and one column short of whole tiles
    (1, 16, 17, 128, 128, 7),     # T = 6: whole tiles plus a one-pixel edge column, overlap rows between tile rows
    (2, 10, 13, 128, 256, 7),     # T = 8: the shape class of the model-level fc6 tests
    (2, 64, 64, 64, 128, 7),      # T = 128: exactly one full GEMM row tile per plane, the training shape's class
    (3, 40, 72, 64, 128, 7),      # T = 135: a partial second row tile, the weight gradient reduces over 135 rows
    (2, 10, 13, 32, 128, 3),      # mixed: the transposed-B GEMM does not take Cin = 32, the data gradient leaves the DFT domain
    (1, 8, 16, 48, 128, 3),       # mixed, Cin no multiple of 32
    (1, 24, 8, 16, 128, 3),       # mixed, the smallest Cin
    (1, 4, 4, 64, 128, 0),        # the rule refuses (292 plane products against F(4x4,4x4)'s 196): nothing runs in the DFT domain, the result is still right
    (1, 8, 16, 256, 128, 7),      # T = 2, Cin > Cout: Xf / dXf (Cin channels) are the wider tensors, V must be planned for them
]
BIG = (3, 40, 72, 64, 128)
DROP = (2, 10, 13, 128, 256)


def expected_bits(bits2, path):
    """Path 1 differs from path 2 in the weight-gradient product only; path 0 never enters the DFT domain."""
    return {2: bits2, 1: bits2 & 5, 0: 0}[path]


@functools.lru_cache(maxsize=None)
def case(N, H, W, Cin, Cout):
    """Inputs (x post-ReLU like pool5) and the float64 reference, computed once per shape and shared read-only."""
    rng = np.random.default_rng(1000 * H + 10 * W + N + Cin)
    x = np.maximum(rng.standard_normal((N, H, W, Cin)), 0).astype(np.float32)
    w = (rng.standard_normal((7, 7, Cin, Cout)) / np.sqrt(49 * Cin)).astype(np.float32)
    b = rng.standard_normal(Cout).astype(np.float32)
    dy = rng.standard_normal((N, H, W, Cout)).astype(np.float32)
    xt = torch.tensor(x).permute(0, 3, 1, 2).double()
    wt = torch.tensor(w).permute(3, 2, 0, 1).double().contiguous()
    dyt = torch.tensor(dy).permute(0, 3, 1, 2).double().contiguous()
    conv = F.conv2d(xt, wt, None, padding=3).permute(0, 2, 3, 1).numpy()
    c = dict(x=x, w=w, b=b, dy=dy, conv=conv, y=np.maximum(conv + b.astype(np.float64), 0),
             dx=torch.nn.grad.conv2d_input(xt.shape, wt, dyt, padding=3).permute(0, 2, 3, 1).numpy(),
             dw=torch.nn.grad.conv2d_weight(xt, wt.shape, dyt, padding=3).permute(2, 3, 1, 0).numpy(),
             db=dy.astype(np.float64).sum((0, 1, 2)))
    for v in c.values():
        v.setflags(write=False)
    return c


def run(shape, path, images=None, bias=True, keep=1.0, seed=0):
    """One call of the op on `shape` (optionally on its first `images` images only); the outputs are the arena's: everything is assigned."""
    L = _lib()
    N, H, W, Cin, Cout = shape
    c = case(*shape)
    n = images or N
    xd, wd, dyd = inp(c["x"][:n]), inp(c["w"]), inp(c["dy"][:n])
    bd = inp(c["b"]) if bias else None
    y, dx = out((n, H, W, Cout)), out((n, H, W, Cin))
    dw = out((7, 7, Cin, Cout))
    db = out((Cout,)) if bias else None
    bits = C.c_int(-1)
    L.check(L.lib.fcn8s_op_conv7x7_fc6_fwd_bwd(None, ptr(xd), ptr(wd), ptr(bd), ptr(dyd), ptr(y), ptr(dx), ptr(dw), ptr(db),
                                                n, H, W, Cin, Cout, path, keep, seed, C.byref(bits)))
    torch.cuda.synchronize()
    return dict(y=y.cpu().numpy(), dx=dx.cpu().numpy(), dw=dw.cpu().numpy(), db=db.cpu().numpy() if bias else None, bits=bits.value)


def check_parity(shape, path, got, what=("y", "dx", "dw", "db")):
    c = case(*shape)
    err = {k: rel_err(got[k], c[k]) for k in what}
    print("fc6 op %s path %d, DFT products %d: error / max |ref| " % (shape, path, got["bits"]) + ", ".join("%s %.2e" % kv for kv in err.items()))
    for k in what:
        assert err[k] < BAR, (shape, path, k, err[k])


@pytest.mark.parametrize("path", [2, 1, 0])
@pytest.mark.parametrize("N,H,W,Cin,Cout,bits2", CASES)
def test_fc6_fwd_bwd_against_float64(N, H, W, Cin, Cout, bits2, path):
    """y = relu(conv + b), dx, dw, db of every case on every path within 2e-5 of float64, and the products that ran in the DFT domain are the
    ones the model's rules (fft6_cheaper, fft6_shape_ok, bt_gemm_ok) give for the shape.  Path 1 is the only place where the DFT data gradient
    builds dYf itself and where F(4x4,4x4)'s weight gradient runs beside a DFT forward; path 0 is the F(4x4,4x4) / direct backward."""
    shape = (N, H, W, Cin, Cout)
    got = run(shape, path)
    assert got["bits"] == expected_bits(bits2, path)
    check_parity(shape, path, got)


def test_fc6_without_a_bias():
    shape = (2, 5, 9, 64, 128)
    got = run(shape, 2, bias=False)
    assert got["bits"] == 7
    c = case(*shape)
    err = {"y": rel_err(got["y"], np.maximum(c["conv"], 0)), "dx": rel_err(got["dx"], c["dx"]), "dw": rel_err(got["dw"], c["dw"])}
    print("fc6 op %s without a bias: " % (shape,) + ", ".join("%s %.2e" % kv for kv in err.items()))
    assert max(err.values()) < BAR, err


def test_fc6_dft_path_is_batch_independent_across_gemm_row_tiles():
    """135 tiles fill one 128-row GEMM tile per plane and part of a second; the first image alone has 45.  What the DFT path computes for an
    image must not depend on the images that share its batch (a data-parallel shard computes the big batch's bits): y[0] and dx[0] bit for bit."""
    full, one = run(BIG, 2), run(BIG, 2, images=1)
    assert full["bits"] == one["bits"] == 7
    assert np.array_equal(full["y"][0], one["y"][0])
    assert np.array_equal(full["dx"][0], one["dx"][0])


def test_fc6_dft_path_is_reproducible():
    """The DFT-domain weight gradient has one writer per element and plain stores: two calls give the same bits in all four tensors."""
    a, b = run(BIG, 2), run(BIG, 2)
    for k in ("y", "dx", "dw", "db"):
        assert np.array_equal(a[k], b[k]), k


def test_fc6_dropout_on_partial_tiles():
    """keep_prob = 0.5 on a 10x13 map (partial edge tiles in both directions): the DFT output transform and the direct 7x7 kernel drop the same
    elements (the Philox index is the NHWC element index, whatever the tile), survivors are scaled by 1 / keep, and about half are dropped."""
    keep, seed = 0.5, 20240607
    c = case(*DROP)
    dft, direct = run(DROP, 2, keep=keep, seed=seed), run(DROP, 0, keep=keep, seed=seed)
    assert dft["bits"] == 7 and direct["bits"] == 0
    assert np.array_equal(dft["y"] == 0, direct["y"] == 0)
    ref = c["y"] / keep
    on = c["y"] > BAR * np.abs(c["y"]).max()             # elements that are not zero for the ReLU's sake
    bar = BAR * np.abs(ref).max()
    n = int(on.sum())
    for name, got in (("DFT", dft["y"]), ("direct", direct["y"])):
        dropped = got[on] == 0
        err = np.abs(got[on] - ref[on])[~dropped].max()
        share = dropped.mean()
        print("fc6 op %s dropout, %s: %d elements, dropped share %.4f, survivors' error / max |ref| %.2e" % (DROP, name, n, share, err / np.abs(ref).max()))
        assert err < bar, (name, err, bar)
        assert abs(share - (1 - keep)) < 5 * np.sqrt(keep * (1 - keep) / n), (name, share, n)


def test_fc6_op_argument_checks():
    L = _lib()
    N, H, W, Cin, Cout = 1, 8, 8, 64, 128
    t = {k: (out((n,)) if k in ("y", "dx", "dw") else inp(np.zeros(n, np.float32))) for k, n in (("x", N * H * W * Cin), ("w", 49 * Cin * Cout), ("dy", N * H * W * Cout), ("y", N * H * W * Cout),
                                               ("dx", N * H * W * Cin), ("dw", 49 * Cin * Cout))}

    def call(cin=Cin, cout=Cout, path=2, keep=1.0, null=None):
        a = {k: (None if k == null else ptr(v)) for k, v in t.items()}
        return L.lib.fcn8s_op_conv7x7_fc6_fwd_bwd(None, a["x"], a["w"], None, a["dy"], a["y"], a["dx"], a["dw"], None, N, H, W, cin, cout, path, keep, 0, None)

    L.check(call())
    bad = [dict(cin=24), dict(cin=8), dict(cout=64), dict(cout=192), dict(path=-1), dict(path=3), dict(keep=0.0), dict(keep=-0.5), dict(keep=1.5),
           dict(keep=float("nan"))] + [dict(null=k) for k in t]
    for kw in bad:
        with pytest.raises(ValueError):
            L.check(call(**kw))


def test_fc6_dft_path_steps_aside_in_split_bf16_mode():
    """Under op_split_pieces = 3 every GEMM of the op runs the split-bf16 arithmetic; the DFT plane GEMMs are fp32 only, so nothing may run in the
    DFT domain -- and the path that runs instead holds the fp32 bar."""
    L = _lib()
    prev = C.c_int64()
    L.check(L.lib.fcn8s_get_option(None, b"op_split_pieces", C.byref(prev)))
    try:
        L.check(L.lib.fcn8s_set_option(None, b"op_split_pieces", 3))
        got = run(DROP, 2)
    finally:
        L.check(L.lib.fcn8s_set_option(None, b"op_split_pieces", int(prev.value)))
    assert got["bits"] == 0
    check_parity(DROP, 2, got)
