"""Every entry point on a non-default stream.

The one rule this module checks: on any stream a library call gives the result it gives on the default stream, and needs no ordering but
that of the stream it was given; a model keeps that property when the caller moves it to another stream between calls.

The rest of the suite passes None as the op-level stream and drives every Engine with torch's default stream current -- the legacy NULL
stream, which orders all of its own work: a launch, clear or copy that goes to the NULL stream instead of the caller's is still ordered
there.  A torch.cuda.Stream() is non-blocking; the same mistake there reads inputs that are not written yet or clears an output after it
was produced, and the numbers look plausible.

The harness forces each such race to resolve the harmful way.  Every case -- each row of the op table, each model sequence, the wrappers,
the model that moves between streams and the two interleaved engines -- runs on a side stream S under two skews:
  side late   a delay kernel is queued on S; behind it, still on S, the inputs are copied from clean staging tensors into the buffers the
              call reads (poison until then); then the call is made with stream S.  Whatever the library sends to the NULL stream runs
              before the delay ends, on poison or on the warm-up's stale scratch.
  NULL late   the delay is queued on the NULL stream, the inputs are ready, the call is made with stream S.  Whatever goes to the NULL
              stream runs after the call's real work: a stray clear wipes a finished result, a stray producer delivers too late.
Values only: float poison is NaN; index-like buffers (labels, predictions, instance ids, codes, look-up tables, per-image parameters) are
poisoned with other in-range values; every buffer is allocated at full size before the delay starts and none is freed during a case.  Each
case is warmed up on S first with inputs of another seed, so the (device, S) scratch exists and holds wrong data, not last call's answer.
A canary in torch ops alone (a chain on S with one link issued on the NULL stream) runs with the same streams and delay before and after
the case table: if S and the NULL stream shared a hardware queue the skew would vanish, and the canary is what says so.

Results on S are held to (1) the float64 reference of the entry's own test at that test's tolerance and (2) the same call on the default
stream -- bit for bit with op_deterministic = 1 or where the entry has no float atomics; the split-K / atomic routes run with the switch
off against (1) alone.  Outputs are pre-filled with garbage, so an output that was never written fails too.

The delay: torch.cuda._sleep, calibrated once per session with events.  It is DELAY_MULTIPLE = 4 times a host time measured on the default
stream, and at least DELAY_FLOOR_MS.  For a row of the op table and for a wrapper that time is the row's own: the whole call, warm, with its
synchronisations, which is no less than its enqueue.  For the canary it is one fcn8s_op_conv2d_bwd enqueue, for the model cases one
train_step(fetch_loss=False) at 2 x 64 x 96, measured in the same setup step.  The asynchronous model calls assert that the delay's end
event has not fired when they return.  The figures of a run are printed by the first and the last test (pytest -s).
Measured on the MI355X: 2.40e6 sleep cycles per ms; enqueue of the conv backward 0.14 - 0.15 ms, of the training step 0.54 - 1.17 ms; the
longest call of a row or wrapper 0.79 ms (host time, synchronisations included); 4 x those is 0.6 ms, 2.1 - 4.7 ms and 3.2 ms, so every
delay sits at the 5 ms floor.  The whole module (114 tests) takes 7.9 s, 4.2 s of it behind the harness set-up.
"""
import ctypes as C
import functools
import time

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from oracle import fcn8s_oracle as orc  # noqa: E402  (checker only)
from fcn8s_tensorflow_amd import crf, cv2_compat, fp8, optim, tta  # noqa: E402
from fcn8s_tensorflow_amd import cityscapes_eval as cs, loss as LM, mc_dropout as mc, regions as RG, reliability as rel, temperature as ts  # noqa: E402
from tests.test_ops_gpu import rel_err  # noqa: E402
from tests import test_fc6_fft_ops_gpu as fc6t, test_fp8_gpu as fp8t, test_loss_gpu as losst, test_boundary_loss_ops_gpu as pxt  # noqa: E402
from tests import test_reliability_ops_gpu as relt, test_temperature_ops_gpu as tst, test_mc_dropout_ops_gpu as mct, test_crf_gpu as crft  # noqa: E402
from tests import test_predict_tta_gpu as ttat  # noqa: E402
from tests import test_gemm_out_fused64_ops_gpu as f64t  # noqa: E402

DELAY_MULTIPLE = 4
DELAY_FLOOR_MS = 5.0
SKEWS = ("side_late", "null_late")
f32 = np.float32


def lib():
    from fcn8s_tensorflow_amd import _lib
    return _lib


def ptr(t, byte_off=0):
    return C.c_void_p(t.data_ptr() + byte_off) if t is not None else None


def sptr(stream):
    return C.c_void_p(stream.cuda_stream) if stream is not None else None


def set_det(v):
    """op_deterministic is thread-local and a model call resets it: set it immediately before each op call."""
    L = lib()
    L.check(L.lib.fcn8s_set_option(None, b"op_deterministic", int(v)))


# ---- the harness ---------------------------------------------------------------------------------------------------------------------
class Harness:
    """The two side streams and the calibrated delay (made once per session)."""

    def __init__(self):
        assert torch.cuda.is_available()
        self.S, self.S2 = torch.cuda.Stream(), torch.cuda.Stream()
        assert self.S.cuda_stream != 0 and self.S2.cuda_stream != 0 and self.S.cuda_stream != self.S2.cuda_stream
        assert torch.cuda.current_stream().cuda_stream == 0, "the suite's default stream is the NULL stream"
        torch.cuda._sleep(1000); torch.cuda.synchronize()
        cycles, ms = 1_000_000, 0.0
        for _ in range(8):                                     # bounded: grow until the delay is long enough to time
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record(); torch.cuda._sleep(cycles); b.record(); torch.cuda.synchronize()
            ms = a.elapsed_time(b)
            if ms >= 2.0:
                break
            cycles *= 4
        assert ms >= 0.5, "torch.cuda._sleep could not be calibrated (%d cycles took %.3f ms)" % (cycles, ms)
        self.cycles_per_ms = cycles / ms
        self.enqueue_ms = {}
        self.delay_ms = {}

    def set_delay(self, kind, enqueue_ms):
        self.enqueue_ms[kind] = enqueue_ms
        self.delay_ms[kind] = max(DELAY_FLOOR_MS, DELAY_MULTIPLE * enqueue_ms)

    def delay(self, kind, host_ms=0.0):
        """Queue the delay on the current stream: the kind's own, or DELAY_MULTIPLE x host_ms (the measured host time of the call that
        follows) if that is longer; returns the event behind it."""
        ms = max(self.delay_ms[kind], DELAY_MULTIPLE * host_ms)
        self.longest_ms = max(self.longest_ms, ms)
        torch.cuda._sleep(int(ms * self.cycles_per_ms))
        ev = torch.cuda.Event()
        ev.record()
        return ev


@pytest.fixture(scope="module")
def H():
    h = Harness()
    h.longest_ms, h.longest_host_ms = 0.0, 0.0
    L = lib()
    # the canary's delay: one conv backward's enqueue on the default stream, warm (every row of the table measures its own call besides)
    c = conv_case(1, 8, 8, 128, 256, 3, 1)
    t = {k: torch.tensor(c[k]).cuda() for k in ("x", "w", "dy")}
    o = [torch.empty(s).cuda() for s in (c["x"].shape, c["w"].shape, (256,))]
    call = lambda: L.check(L.lib.fcn8s_op_conv2d_bwd(None, ptr(t["x"]), ptr(t["w"]), ptr(t["dy"]), ptr(o[0]), ptr(o[1]), ptr(o[2]), 1, 8, 8, 128, 256, 3))
    call(); torch.cuda.synchronize()
    t0 = time.perf_counter(); call(); dt = time.perf_counter() - t0
    torch.cuda.synchronize()
    h.set_delay("op", dt * 1e3)
    # the model cases' longest enqueue: one training step that does not fetch the loss
    e = fresh("fp32")
    img, lab = dev_batch(SHAPE_A, 50)
    for _ in range(2):
        e.train_step(img, lab, 1e-4, keep_prob=1.0, fetch_loss=False)
    torch.cuda.synchronize()
    t0 = time.perf_counter(); e.train_step(img, lab, 1e-4, keep_prob=1.0, fetch_loss=False); dt = time.perf_counter() - t0
    torch.cuda.synchronize()
    e.close()
    h.set_delay("model", dt * 1e3)
    h.t_start = time.perf_counter()
    print("\nstream harness: %.0f sleep cycles per ms; enqueue op %.3f ms -> delay %.1f ms; enqueue train_step %.3f ms -> delay %.1f ms (x%d, floor %.0f ms)"
          % (h.cycles_per_ms, h.enqueue_ms["op"], h.delay_ms["op"], h.enqueue_ms["model"], h.delay_ms["model"], DELAY_MULTIPLE, DELAY_FLOOR_MS))
    return h


def poison_of(a):
    """Float: NaN.  Integer: other values of the same buffer, so index-like data stays in range."""
    a = np.asarray(a)
    if a.dtype.kind == "f":
        return np.full(a.shape, np.nan, a.dtype)
    if a.dtype == np.bool_:
        return ~a
    lo, hi = a.min(), a.max()
    if lo == hi:                                               # (a constant buffer: rows give such a one an explicit poison)
        return a.copy()
    return np.where(a == hi, lo, hi).astype(a.dtype)


def garbage(shape, dtype):
    dtype = np.dtype(dtype)
    if dtype.kind == "f":
        return np.full(shape, np.nan, dtype)
    return np.full(shape, 0x5A, dtype)


def to_dev(a):
    a = np.ascontiguousarray(a)
    if a.dtype == np.uint16:
        return torch.from_numpy(a.view(np.int16)).cuda()
    return torch.from_numpy(a.copy()).cuda()


def to_host(t, dtype):
    a = t.cpu().numpy()
    return a.view(np.uint16) if np.dtype(dtype) == np.uint16 else a


class Case:
    """One call's data: inp name -> array (inputs and in-out buffers), out name -> (shape, dtype), fetch = the names read back,
    poison = explicit poison for inputs whose values are sizes or offsets, aux = whatever call / check need on the host."""

    def __init__(self, inp, out=None, fetch=None, poison=None, **aux):
        self.inp, self.out, self.poison, self.aux = inp, out or {}, poison or {}, aux
        self.fetch = list(fetch) if fetch is not None else list(self.out)


class Row:
    def __init__(self, name, entries, make, call, check, bitwise=True, det=1):
        self.name, self.entries, self.make, self.call, self.check, self.bitwise, self.det = name, tuple(entries), make, call, check, bitwise, det
        self.host_ms = 0.0                                     # the call's measured host time on the default stream (default_result)

    def __repr__(self):
        return self.name


def execute(row, case, H, stream, skew):
    """One call of the row on `stream` (None: the default stream, no skew) -> {name: array} of case.fetch plus what call() returns."""
    L = lib()
    stage = {k: to_dev(v) for k, v in case.inp.items()}
    if stream is None:
        bufs = dict(stage)
    else:
        bufs = {k: to_dev(case.poison.get(k, poison_of(v))) for k, v in case.inp.items()}
    for k, (shape, dtype) in case.out.items():
        bufs[k] = to_dev(garbage(shape, dtype))
    torch.cuda.synchronize()
    if stream is None:
        set_det(row.det)
        t0 = time.perf_counter()
        extra = row.call(L, None, bufs, case)
        row.host_ms = (time.perf_counter() - t0) * 1e3         # the whole call on the host, its synchronisations included: no less than its enqueue
    elif skew == "side_late":
        with torch.cuda.stream(stream):
            H.delay("op", row.host_ms)
            for k in stage:
                bufs[k].copy_(stage[k])
            set_det(row.det)
            extra = row.call(L, sptr(stream), bufs, case)
    else:
        with torch.cuda.stream(stream):
            for k in stage:
                bufs[k].copy_(stage[k])
        stream.synchronize()
        H.delay("op", row.host_ms)                             # on the NULL stream
        set_det(row.det)
        extra = row.call(L, sptr(stream), bufs, case)
    torch.cuda.synchronize()
    set_det(0)
    got = {k: to_host(bufs[k], (case.inp[k].dtype if k in case.inp else case.out[k][1])) for k in case.fetch}
    got.update(extra or {})
    return got


def same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


# ---- the canary ----------------------------------------------------------------------------------------------------------------------
def canary(H, stray, skew):
    """y = ((x + 1) * 3) - 2 on S in three kernels, with one link on the NULL stream: stray 'zero' = a zero_() of the output,
    stray 'producer' = the middle link.  Returns (result, the all-on-S result)."""
    S = H.S
    n = 1 << 16
    xs = torch.arange(n, dtype=torch.float32, device="cuda")
    outs = []
    for strayed in (True, False):
        x = torch.full((n,), float("nan"), device="cuda"); a = torch.full((n,), float("nan"), device="cuda")
        b = torch.full((n,), float("nan"), device="cuda"); y = torch.full((n,), float("nan"), device="cuda")
        torch.cuda.synchronize()
        null = torch.cuda.default_stream()
        if skew == "side_late":
            with torch.cuda.stream(S):
                H.delay("op")
                x.copy_(xs)
                torch.add(x, 1.0, out=a)
                with torch.cuda.stream(null if (strayed and stray == "producer") else S):
                    torch.mul(a, 3.0, out=b)
                if strayed and stray == "zero":
                    with torch.cuda.stream(null):
                        y.zero_()
                torch.sub(b, 2.0, out=y)
        else:
            with torch.cuda.stream(S):
                x.copy_(xs)
            S.synchronize()
            H.delay("op")
            with torch.cuda.stream(S):
                torch.add(x, 1.0, out=a)
                with torch.cuda.stream(null if (strayed and stray == "producer") else S):
                    torch.mul(a, 3.0, out=b)
                torch.sub(b, 2.0, out=y)
                if strayed and stray == "zero":
                    with torch.cuda.stream(null):
                        y.zero_()
        torch.cuda.synchronize()
        outs.append(y.cpu().numpy())
    return outs


def run_canary(H):
    want = (np.arange(1 << 16, dtype=np.float32) + 1) * 3 - 2
    for stray, skew in (("zero", "null_late"), ("producer", "side_late"), ("producer", "null_late")):
        got, clean = canary(H, stray, skew)
        assert np.array_equal(clean, want), "the all-on-S chain is wrong under %s: the harness itself is broken" % skew
        if same_bits(got, clean):
            pytest.fail("the canary detected nothing: a stray %s on the NULL stream under the %s skew left the result of the chain on S unchanged -- "
                        "S and the NULL stream are ordered against each other here (a shared hardware queue?), so no case of this module can see a "
                        "misdirected launch" % (stray, skew))


def test_canary_detects_both_kinds_of_stray_launch_before_the_case_table(H):
    run_canary(H)


# ---- op level: shared references -----------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def conv_case(N, Hh, W, Cin, Cout, K, seed):
    """test_conv2d_fwd_bwd's inputs and float64 autograd reference."""
    rng = np.random.default_rng(seed)
    x = rng.standard_normal((N, Hh, W, Cin)).astype(f32)
    w = (rng.standard_normal((K, K, Cin, Cout)) / np.sqrt(K * K * Cin)).astype(f32)
    b = rng.standard_normal(Cout).astype(f32)
    dy = rng.standard_normal((N, Hh, W, Cout)).astype(f32)
    xt = torch.tensor(x).permute(0, 3, 1, 2).double().requires_grad_(True)
    wt = torch.tensor(w).double().requires_grad_(True)
    bt = torch.tensor(b).double().requires_grad_(True)
    yt = orc.conv2d_same_t(xt, wt, bt, relu=False)
    yt.backward(torch.tensor(dy).permute(0, 3, 1, 2).double())
    return dict(x=x, w=w, b=b, dy=dy, y=yt.detach().permute(0, 2, 3, 1).numpy(), dx=xt.grad.permute(0, 2, 3, 1).numpy(),
                dw=wt.grad.numpy(), db=bt.grad.numpy())


def F(*shape):
    return (tuple(shape), f32)


def expect(got, ref, tol, keys):
    for k in keys:
        e = rel_err(got[k], ref[k])
        assert e < tol, (k, e, tol)


ROWS = []


def row(name, entries, bitwise=True, det=1):
    def deco(cls):
        ROWS.append(Row(name, entries, cls.make, cls.call, cls.check, bitwise, det))
        return cls
    return deco


def conv_rows(shape, tag, det=1, bitwise=True):
    N, Hh, W, Cin, Cout, K = shape

    @row("conv2d+bwd %s %s" % (tag, "det" if det else "atomics"), ("fcn8s_op_conv2d", "fcn8s_op_conv2d_bwd"), bitwise, det)
    class _:
        @staticmethod
        def make(seed):
            c = conv_case(N, Hh, W, Cin, Cout, K, seed)
            return Case({k: c[k] for k in ("x", "w", "b", "dy")}, dict(y=F(N, Hh, W, Cout), dx=F(N, Hh, W, Cin), dw=F(K, K, Cin, Cout), db=F(Cout)), ref=c)

        @staticmethod
        def call(L, s, b, case):
            L.check(L.lib.fcn8s_op_conv2d(s, ptr(b["x"]), ptr(b["w"]), ptr(b["b"]), ptr(b["y"]), N, Hh, W, Cin, Cout, K, 0))
            L.check(L.lib.fcn8s_op_conv2d_bwd(s, ptr(b["x"]), ptr(b["w"]), ptr(b["dy"]), ptr(b["dx"]), ptr(b["dw"]), ptr(b["db"]), N, Hh, W, Cin, Cout, K))

        @staticmethod
        def check(case, got):
            expect(got, case.aux["ref"], 2e-5, ("y", "dx", "dw", "db"))                    # test_conv2d_fwd_bwd's bar


conv_rows((2, 8, 16, 4, 64, 3), "conv1 kernels")
conv_rows((1, 8, 8, 128, 256, 3), "implicit GEMM")
conv_rows((1, 8, 8, 128, 256, 3), "implicit GEMM", det=0, bitwise=False)                  # split K: the zeroing memset and the atomics
conv_rows((3, 11, 3, 512, 20, 1), "skinny heads")
conv_rows((3, 11, 3, 512, 20, 1), "skinny heads", det=0, bitwise=False)
conv_rows((2, 4, 16, 64, 128, 7), "row-per-block 7x7 wgrad")
conv_rows((2, 4, 16, 64, 128, 7), "row-per-block 7x7 wgrad", det=0, bitwise=False)


@functools.lru_cache(maxsize=None)
def wino_case(N, Hh, W, Cin, Cout, tile, pooled, mask_mode, seed):
    """test_conv3x3_winograd_backward's inputs and float64 reference (near-tie pool windows get no upstream gradient, as there)."""
    rng = np.random.default_rng(seed)
    x = rng.standard_normal((N, Hh, W, Cin)).astype(f32)
    w = (rng.standard_normal((3, 3, Cin, Cout)) / np.sqrt(9 * Cin)).astype(f32)
    b = (0.3 * rng.standard_normal(Cout)).astype(f32)
    skip = rng.standard_normal((N, Hh, W, Cin)).astype(f32)
    xt = torch.tensor(x).permute(0, 3, 1, 2).double().requires_grad_(True)
    wt = torch.tensor(w).double().requires_grad_(True)
    bt = torch.tensor(b).double().requires_grad_(True)
    z = orc.conv2d_same_t(xt, wt, bt, relu=False)
    yt = torch.relu(z)
    if pooled:
        out = orc.maxpool2x2_t(yt)
        dy = rng.standard_normal((N, Hh // 2, W // 2, Cout)).astype(f32)
        ynp = yt.detach().permute(0, 2, 3, 1).numpy()
        srt = np.sort(ynp.reshape(N, Hh // 2, 2, W // 2, 2, Cout).transpose(0, 1, 3, 5, 2, 4).reshape(N, Hh // 2, W // 2, Cout, 4), -1)
        near_tie = (srt[..., 3] > 0) & (srt[..., 3] - srt[..., 2] < 1e-4 * np.abs(ynp).max())
        assert near_tie.mean() < 0.01
        dy[near_tie] = 0.0
        out.backward(torch.tensor(dy).permute(0, 3, 1, 2).double())
        fwd = out.detach().permute(0, 2, 3, 1).numpy()
    else:
        dy = rng.standard_normal((N, Hh, W, Cout)).astype(f32)
        z.backward(torch.tensor(dy).permute(0, 3, 1, 2).double())
        fwd = yt.detach().permute(0, 2, 3, 1).numpy()
    dx = xt.grad.permute(0, 2, 3, 1).numpy() + skip
    if mask_mode:
        dx = dx * (x > 0)
    return dict(x=x, w=w, b=b, dy=dy, skip=skip, fwd=fwd, dx=dx, dw=wt.grad.numpy(), db=bt.grad.numpy())


def wino_rows(shape):
    N, Hh, W, Cin, Cout, tile, pooled, mask_mode = shape

    @row("conv3x3_winograd_fwd_bwd %s" % (shape,), ("fcn8s_op_conv3x3_winograd_fwd_bwd",))
    class _:
        @staticmethod
        def make(seed):
            c = wino_case(*shape, seed)
            fshape = (N, Hh // 2, W // 2, Cout) if pooled else (N, Hh, W, Cout)
            return Case({k: c[k] for k in ("x", "w", "b", "dy", "skip")}, dict(fwd=F(*fshape), dx=F(N, Hh, W, Cin), dw=F(3, 3, Cin, Cout), db=F(Cout)), ref=c)

        @staticmethod
        def call(L, s, b, case):
            y, pool = (None, b["fwd"]) if pooled else (b["fwd"], None)
            L.check(L.lib.fcn8s_op_conv3x3_winograd_fwd_bwd(s, ptr(b["x"]), ptr(b["w"]), ptr(b["b"]), ptr(b["dy"]), ptr(b["skip"]), ptr(y), ptr(pool),
                                                            ptr(b["dx"]), ptr(b["dw"]), ptr(b["db"]), N, Hh, W, Cin, Cout, tile, pooled, mask_mode))

        @staticmethod
        def check(case, got):
            expect(got, case.aux["ref"], 2e-5 if tile == 2 else 1e-4, ("fwd", "dx", "dw", "db"))    # test_conv3x3_winograd_backward's bars
            if mask_mode:
                assert (got["dx"][case.aux["ref"]["x"] <= 0] == 0).all()


for _s in ((1, 34, 22, 64, 64, 6, 1, 2), (2, 12, 18, 192, 192, 6, 0, 1), (1, 16, 32, 64, 64, 4, 1, 1), (1, 8, 12, 64, 128, 2, 0, 1)):
    wino_rows(_s)


def winograd_fwd_rows(shape):
    N, Hh, W, Cin, Cout, tile, K = shape

    @row("conv2d_winograd %s" % (shape,), ("fcn8s_op_conv2d_winograd",))
    class _:
        @staticmethod
        def make(seed):
            c = conv_case(N, Hh, W, Cin, Cout, K, seed)
            return Case({k: c[k] for k in ("x", "w", "b")}, dict(y=F(N, Hh, W, Cout)), ref=np.maximum(c["y"], 0))

        @staticmethod
        def call(L, s, b, case):
            L.check(L.lib.fcn8s_op_conv2d_winograd(s, ptr(b["x"]), ptr(b["w"]), ptr(b["b"]), ptr(b["y"]), N, Hh, W, Cin, Cout, K, 1, tile))

        @staticmethod
        def check(case, got):
            assert rel_err(got["y"], case.aux["ref"]) < (1e-5 if tile == 2 else 1e-4)             # test_conv3x3_winograd's bars


winograd_fwd_rows((3, 2, 4, 32, 64, 6, 3))
winograd_fwd_rows((1, 4, 4, 16, 32, 4, 7))

def winograd_pool_rows(shape, option):
    N, Hh, W = shape

    @row("conv3x3_winograd_pool %s op_gemm_out_fused64 %d" % (shape, option), ("fcn8s_op_conv3x3_winograd_pool",))
    class _:
        @staticmethod
        def make(seed):
            x, k, b = f64t.inputs(N, Hh, W)
            if seed != 1:                                        # the warm-up's other data
                x, k, b = (np.roll(a, 1) for a in (x, k, b))
            pshape = (N, Hh // 2, W // 2, f64t.CH)
            return Case(dict(x=np.array(x), w=np.array(k), b=np.array(b)), dict(pool=F(*pshape), byte=(pshape, np.uint8)),
                        ref=f64t.reference(N, Hh, W) if seed == 1 else None)

        @staticmethod
        def call(L, s, b, case):
            fused = C.c_int(-1)
            with f64t.op_context(op_gemm_out_fused64=option):
                L.check(L.lib.fcn8s_op_conv3x3_winograd_pool(s, ptr(b["x"]), ptr(b["w"]), ptr(b["b"]), ptr(b["pool"]), ptr(b["byte"]), N, Hh, W, f64t.CH, f64t.CH,
                                                             f64t.TILE, 1, C.byref(fused)))
            return dict(fused=np.array(fused.value))

        @staticmethod
        def check(case, got):
            ref = case.aux["ref"]
            assert int(got["fused"]) == (option != 0)
            assert rel_err(got["pool"], ref["pool"]) < 1e-4                                       # test_gemm_out_fused64_ops_gpu's bars
            assert not ((got["byte"] != ref["byte"]) & ~ref["amb"]).any()


winograd_pool_rows((3, 14, 20), 1)
winograd_pool_rows((1, 6, 102), 2)

FC6_SHAPE = min(fc6t.CASES, key=lambda c: c[0] * c[1] * c[2] * c[3] * c[4])[:5]


def fc6_rows(path):
    N, Hh, W, Cin, Cout = FC6_SHAPE

    @row("conv7x7_fc6_fwd_bwd %s path %d" % (FC6_SHAPE, path), ("fcn8s_op_conv7x7_fc6_fwd_bwd",))
    class _:
        @staticmethod
        def make(seed):
            if seed == 1:
                c = fc6t.case(*FC6_SHAPE)
            else:                                                # the warm-up's other data
                c = {k: np.roll(v, 1) for k, v in fc6t.case(*FC6_SHAPE).items()}
            return Case({k: np.array(c[k]) for k in ("x", "w", "b", "dy")}, dict(y=F(N, Hh, W, Cout), dx=F(N, Hh, W, Cin), dw=F(7, 7, Cin, Cout), db=F(Cout)), ref=c)

        @staticmethod
        def call(L, s, b, case):
            bits = C.c_int(-1)
            L.check(L.lib.fcn8s_op_conv7x7_fc6_fwd_bwd(s, ptr(b["x"]), ptr(b["w"]), ptr(b["b"]), ptr(b["dy"]), ptr(b["y"]), ptr(b["dx"]), ptr(b["dw"]), ptr(b["db"]),
                                                       N, Hh, W, Cin, Cout, path, 1.0, 0, C.byref(bits)))
            return dict(bits=np.array(bits.value))

        @staticmethod
        def check(case, got):
            expect(got, case.aux["ref"], fc6t.BAR, ("y", "dx", "dw", "db"))
            bits2 = [c[5] for c in fc6t.CASES if c[:5] == FC6_SHAPE][0]
            assert int(got["bits"]) == fc6t.expected_bits(bits2, path)


for _p in (2, 1, 0):
    fc6_rows(_p)


@row("conv2d_bf16 (2,3,3,32,128,3)", ("fcn8s_op_conv2d_bf16",))
class _:
    SH = (2, 3, 3, 32, 128, 3)

    @staticmethod
    def make(seed):
        N, Hh, W, Cin, Cout, K = (2, 3, 3, 32, 128, 3)
        c = conv_case(N, Hh, W, Cin, Cout, K, seed)
        xr = torch.tensor(c["x"]).to(torch.bfloat16).double().permute(0, 3, 1, 2)
        wr = torch.tensor(c["w"]).to(torch.bfloat16).double()
        ref = orc.conv2d_same_t(xr, wr, torch.tensor(c["b"]).double(), relu=True).permute(0, 2, 3, 1).numpy()
        return Case({k: c[k] for k in ("x", "w", "b")}, dict(y=F(N, Hh, W, Cout)), ref=ref)

    @staticmethod
    def call(L, s, b, case):
        L.check(L.lib.fcn8s_op_conv2d_bf16(s, ptr(b["x"]), ptr(b["w"]), ptr(b["b"]), ptr(b["y"]), 2, 3, 3, 32, 128, 3, 1))

    @staticmethod
    def check(case, got):
        assert rel_err(got["y"], case.aux["ref"]) < 1e-5                                          # test_conv_bf16_mfma's bar


@functools.lru_cache(maxsize=None)
def bf16_train_case(N, Hh, W, Cin, Cout, K, seed):
    """test_conv_bf16_train_kernels' inputs and float64 references on the bf16-rounded operands."""
    rng = np.random.default_rng(seed)
    x = rng.standard_normal((N, Hh, W, Cin)).astype(f32)
    w = (rng.standard_normal((K, K, Cin, Cout)) / np.sqrt(K * K * Cin)).astype(f32)
    b = rng.standard_normal(Cout).astype(f32)
    dy = rng.standard_normal((N, Hh, W, Cout)).astype(f32)
    mask = rng.standard_normal((N, Hh, W, Cin)).astype(f32)
    rb = lambda a: torch.tensor(a).to(torch.bfloat16).double()
    nchw = lambda t: t.permute(0, 3, 1, 2)
    nhwc = lambda t: t.permute(0, 2, 3, 1).numpy()
    pad = (K - 1) // 2
    xr, wr, dyr = nchw(rb(x)), rb(w).permute(3, 2, 0, 1), nchw(rb(dy))
    return dict(x=x, w=w, b=b, dy=dy, mask=mask,
                y=nhwc(torch.relu(torch.nn.functional.conv2d(xr, wr, torch.tensor(b).double(), padding=pad))),
                dx=nhwc(torch.nn.grad.conv2d_input(xr.shape, wr, dyr, padding=pad)) * (mask > 0),
                dw=torch.nn.grad.conv2d_weight(xr, wr.shape, dyr, padding=pad).permute(2, 3, 1, 0).numpy(),
                db=dy.astype(np.float64).sum((0, 1, 2)))


def bf16_train_rows(shape, det, bitwise):
    N, Hh, W, Cin, Cout, K = shape

    @row("conv2d_bf16_train %s %s" % (shape, "det" if det else "atomics"), ("fcn8s_op_conv2d_bf16_train",), bitwise, det)
    class _:
        @staticmethod
        def make(seed):
            c = bf16_train_case(*shape, seed)
            return Case({k: c[k] for k in ("x", "w", "b", "dy", "mask")}, dict(y=F(N, Hh, W, Cout), dx=F(N, Hh, W, Cin), dw=F(K, K, Cin, Cout), db=F(Cout)), ref=c)

        @staticmethod
        def call(L, s, b, case):
            L.check(L.lib.fcn8s_op_conv2d_bf16_train(s, ptr(b["x"]), ptr(b["w"]), ptr(b["b"]), ptr(b["y"]), 1, ptr(b["dy"]), ptr(b["mask"]), ptr(b["dx"]),
                                                     ptr(b["dw"]), ptr(b["db"]), N, Hh, W, Cin, Cout, K))

        @staticmethod
        def check(case, got):
            expect(got, case.aux["ref"], 1e-5, ("y", "dx", "dw", "db"))                          # test_conv_bf16_train_kernels' bar


for _s in ((1, 20, 24, 64, 128, 3), (1, 8, 16, 256, 512, 7)):
    bf16_train_rows(_s, 1, True)
    bf16_train_rows(_s, 0, False)

FP8_SHAPE = min(fp8t.CASES, key=lambda c: c[0] * c[1] * c[2] * c[3] * c[4] * c[5] * c[5])


@row("conv2d_fp8 %s" % (FP8_SHAPE,), ("fcn8s_op_conv2d_fp8",))
class _:
    @staticmethod
    def make(seed):
        N, Hh, W, Cin, Cout, K = FP8_SHAPE
        rng = np.random.default_rng(N * 1000 + Cin + Cout + K + seed - 1)            # seed 1: the inputs of test_op_conv2d_fp8_against_float64_...
        x = np.maximum(rng.standard_normal((N, Hh, W, Cin)), 0).astype(f32) * 3
        w = (rng.standard_normal((K, K, Cin, Cout)) * np.sqrt(2.0 / (K * K * Cin)) * np.logspace(-1, 1, Cout)).astype(f32)
        b = (rng.standard_normal(Cout) * 0.1).astype(f32)
        return Case(dict(x=x, w=w, b=b), dict(y=F(N, Hh, W, Cout)), ex=int(fp8.exponent(np.abs(x).max())))

    @staticmethod
    def call(L, s, b, case):
        N, Hh, W, Cin, Cout, K = FP8_SHAPE
        L.check(L.lib.fcn8s_op_conv2d_fp8(s, ptr(b["x"]), ptr(b["w"]), ptr(b["b"]), ptr(b["y"]), 0, case.aux["ex"], N, Hh, W, Cin, Cout, K))

    @staticmethod
    def check(case, got):
        x, w, b, ex = case.inp["x"], case.inp["w"], case.inp["b"], case.aux["ex"]
        xq = fp8.quantize_activation(x, ex).numpy().astype(np.float64)
        wq, ew = fp8.quantize_weights(w)
        wd = wq.numpy().astype(np.float64) * np.ldexp(1.0, ew)
        ref = fp8t.conv64(xq, wd) + b
        mag = fp8t.conv64(np.abs(xq), np.abs(wd)) + np.abs(b)
        assert (np.abs(got["y"] - ref) / (mag + 1e-30)).max() < fp8t.TOL


@row("maxpool2x2+bwd (1,4,6,8)", ("fcn8s_op_maxpool2x2", "fcn8s_op_maxpool2x2_bwd"))
class _:
    @staticmethod
    def make(seed):
        rng = np.random.default_rng(seed)
        x = np.maximum(rng.standard_normal((1, 4, 6, 8)), 0).astype(f32)
        dy = rng.standard_normal((1, 2, 3, 8)).astype(f32)
        return Case(dict(x=x, dy=dy), dict(y=F(1, 2, 3, 8), dx=F(1, 4, 6, 8)))

    @staticmethod
    def call(L, s, b, case):
        L.check(L.lib.fcn8s_op_maxpool2x2(s, ptr(b["x"]), ptr(b["y"]), 1, 4, 6, 8))
        L.check(L.lib.fcn8s_op_maxpool2x2_bwd(s, ptr(b["x"]), ptr(b["dy"]), ptr(b["dx"]), 1, 4, 6, 8, 1))

    @staticmethod
    def check(case, got):
        x, dy = case.inp["x"], case.inp["dy"]
        yt = orc.maxpool2x2_t(torch.tensor(x).permute(0, 3, 1, 2))
        assert np.array_equal(got["y"], yt.permute(0, 2, 3, 1).numpy())
        pre = torch.tensor(x).permute(0, 3, 1, 2).clone()
        pre[pre == 0] = -1.0
        pre.requires_grad_(True)
        orc.maxpool2x2_t(torch.relu(pre)).backward(torch.tensor(dy).permute(0, 3, 1, 2))
        assert np.array_equal(got["dx"], pre.grad.permute(0, 2, 3, 1).numpy())                    # test_maxpool: exact


def tconv_rows(shape, det, bitwise):
    N, Hi, Wi, Cc, K, S_ = shape

    @row("conv2d_transpose+bwd %s %s" % (shape, "det" if det else "atomics"), ("fcn8s_op_conv2d_transpose", "fcn8s_op_conv2d_transpose_bwd"), bitwise, det)
    class _:
        @staticmethod
        def make(seed):
            rng = np.random.default_rng(seed)
            x = rng.standard_normal((N, Hi, Wi, Cc)).astype(f32)
            w = (rng.standard_normal((K, K, Cc, Cc)) * 0.1).astype(f32)
            b = rng.standard_normal(Cc).astype(f32)
            add = rng.standard_normal((N, Hi * S_, Wi * S_, Cc)).astype(f32)
            dy = rng.standard_normal((N, Hi * S_, Wi * S_, Cc)).astype(f32)
            return Case(dict(x=x, w=w, b=b, add=add, dy=dy), dict(y=F(N, Hi * S_, Wi * S_, Cc), dx=F(N, Hi, Wi, Cc), dw=F(K, K, Cc, Cc), db=F(Cc)))

        @staticmethod
        def call(L, s, b, case):
            L.check(L.lib.fcn8s_op_conv2d_transpose(s, ptr(b["x"]), ptr(b["w"]), ptr(b["b"]), ptr(b["add"]), ptr(b["y"]), N, Hi, Wi, Cc, K, S_))
            L.check(L.lib.fcn8s_op_conv2d_transpose_bwd(s, ptr(b["x"]), ptr(b["w"]), ptr(b["dy"]), ptr(b["dx"]), ptr(b["dw"]), ptr(b["db"]), N, Hi, Wi, Cc, K, S_))

        @staticmethod
        def check(case, got):
            i = case.inp
            xt = torch.tensor(i["x"]).permute(0, 3, 1, 2).double().requires_grad_(True)
            wt = torch.tensor(i["w"]).double().requires_grad_(True)
            bt = torch.tensor(i["b"]).double().requires_grad_(True)
            yt = orc.conv2d_transpose_same_t(xt, wt, bt, S_) + torch.tensor(i["add"]).permute(0, 3, 1, 2).double()
            yt.backward(torch.tensor(i["dy"]).permute(0, 3, 1, 2).double())
            ref = dict(y=yt.detach().permute(0, 2, 3, 1).numpy(), dx=xt.grad.permute(0, 2, 3, 1).numpy(), dw=wt.grad.numpy(), db=bt.grad.numpy())
            expect(got, ref, 2e-5, ("y", "dx", "dw", "db"))                                      # test_conv2d_transpose_fwd_bwd's bar


for _s in ((2, 3, 5, 20, 4, 2), (1, 4, 4, 20, 16, 8)):
    tconv_rows(_s, 1, True)
    tconv_rows(_s, 0, False)


# ---- losses ---------------------------------------------------------------------------------------------------------------------------
@row("softmax_xent + softmax_argmax (257,12)", ("fcn8s_op_softmax_xent", "fcn8s_op_softmax_argmax"))
class _:
    @staticmethod
    def make(seed):
        rng = np.random.default_rng(3 + seed)
        logits = (rng.standard_normal((257, 12)) * 3).astype(f32)
        labels = rng.integers(0, 12, 257).astype(np.uint8)
        return Case(dict(logits=logits, labels=labels), dict(dl=F(257, 12), lo=F(1), sm=F(257, 12), am=((257,), np.int64)))

    @staticmethod
    def call(L, s, b, case):
        L.check(L.lib.fcn8s_op_softmax_xent(s, ptr(b["logits"]), ptr(b["labels"]), ptr(b["dl"]), ptr(b["lo"]), 257, 12))
        L.check(L.lib.fcn8s_op_softmax_argmax(s, ptr(b["logits"]), ptr(b["sm"]), ptr(b["am"]), 257, 12))

    @staticmethod
    def check(case, got):
        logits, labels = case.inp["logits"], case.inp["labels"]
        lt = torch.tensor(logits).double().requires_grad_(True)
        loss = torch.nn.functional.cross_entropy(lt, torch.tensor(labels.astype(np.int64)))
        loss.backward()
        assert abs(float(got["lo"][0]) - float(loss.detach())) < 1e-5 * max(1.0, abs(float(loss.detach())))
        assert np.abs(got["dl"] - lt.grad.numpy()).max() < 1e-6
        sm_ref = orc.softmax(logits)
        assert np.abs(got["sm"] - sm_ref).max() < 1e-6
        assert np.array_equal(got["am"], np.argmax(sm_ref, -1))                                   # test_softmax_xent_and_argmax's bars


def xent_ex_rows(px):
    name = "softmax_xent_px (codes, table)" if px else "softmax_xent_ex (weights, OHEM)"

    @row(name + " (257,12)", ("fcn8s_op_softmax_xent_px" if px else "fcn8s_op_softmax_xent_ex",))
    class _:
        @staticmethod
        def make(seed):
            logits, lab, codes, table = pxt.op_batch(257, 12, 40 + seed)
            w = np.random.default_rng(seed).uniform(0.5, 2.0, 12).astype(f32)
            inp = dict(logits=logits, lab=lab, w=w)
            if px:
                inp.update(codes=codes, table=table)
            return Case(inp, dict(dl=F(257, 12), lo=F(1), pl=F(257), st=((3,), np.int64)))

        @staticmethod
        def call(L, s, b, case):
            if px:
                L.check(L.lib.fcn8s_op_softmax_xent_px(s, ptr(b["logits"]), ptr(b["lab"]), ptr(b["w"]), 0.7, 10, ptr(b["codes"]), ptr(b["table"]), ptr(b["dl"]),
                                                       ptr(b["lo"]), ptr(b["pl"]), ptr(b["st"]), 257, 12))
            else:
                L.check(L.lib.fcn8s_op_softmax_xent_ex(s, ptr(b["logits"]), ptr(b["lab"]), ptr(b["w"]), 0.7, 10, ptr(b["dl"]), ptr(b["lo"]), ptr(b["pl"]),
                                                       ptr(b["st"]), 257, 12))

        @staticmethod
        def check(case, got):
            i = case.inp
            valid = i["lab"] < 12
            assert (got["pl"][~valid] == -1.0).all()
            l64 = LM.pixel_losses(i["logits"], i["lab"])
            assert np.abs(got["pl"][valid] - l64[valid]).max() <= 1e-5 * max(1.0, np.abs(l64[valid]).max())
            r = LM.restate(i["logits"], i["lab"], class_weights=i["w"], ohem_thresh=0.7, ohem_min_kept=10, pixel_loss=got["pl"],
                           pixel_weights=i["table"][i["codes"]] if px else None)
            assert np.array_equal((got["dl"] != 0).any(1), r["kept"]) or px                      # (a zero table entry may silence a kept pixel)
            assert got["st"].tolist() == [r["valid"], r["num_kept"], losst.f32_bits(r["threshold"])]
            assert abs(float(got["lo"][0]) - r["loss"]) <= 2e-6 * max(1e-30, abs(r["loss"]))
            assert np.abs(got["dl"] - r["dlogits"]).max() <= 2e-6 * np.abs(r["dlogits"]).max()   # test_op_ohem_selection_is_exact's bars


xent_ex_rows(False)
xent_ex_rows(True)


def lovasz_rows(with_grad):
    @row("lovasz_softmax (257,12) %s" % ("with a gradient" if with_grad else "loss only"), ("fcn8s_op_lovasz_softmax",))
    class _:
        @staticmethod
        def make(seed):
            rng = np.random.default_rng(40 + seed)
            z = (rng.standard_normal((257, 12)) * 3).astype(f32)
            lab = rng.integers(0, 12, 257).astype(np.uint8)
            lab[rng.random(257) < 0.1] = 255
            out = dict(lo=F(1), cl=F(12), sm=F(257, 12), am=((257,), np.int64))
            if with_grad:
                out["g"] = F(257, 12)
            return Case(dict(z=z, lab=lab), out)

        @staticmethod
        def call(L, s, b, case):
            L.check(L.lib.fcn8s_op_lovasz_softmax(s, ptr(b["z"]), 1, ptr(b["lab"]), 1, 257, 12, 0, None, ptr(b["lo"]), ptr(b.get("g")), ptr(b["cl"])))
            L.check(L.lib.fcn8s_op_softmax_argmax(s, ptr(b["z"]), ptr(b["sm"]), ptr(b["am"]), 257, 12))      # test_lovasz_gpu.dev_softmax, on this stream

        @staticmethod
        def check(case, got):
            # test_op_on_logits: the restatement on the device's own fp32 softmax (the probabilities the kernels use, bit for bit), its bars
            assert np.abs(got["sm"] - orc.softmax(case.inp["z"])).max() < 1e-6
            r = LM.lovasz_restate(got["sm"], case.inp["lab"], 1, per_image=False, x_is='probs')
            assert abs(float(got["lo"][0]) - r["loss"]) <= 2e-6 * r["loss"]
            if with_grad:
                assert np.abs(got["g"] - r["grad_logits"]).max() / max(np.abs(r["grad_logits"]).max(), 1e-30) <= 1e-6


lovasz_rows(True)
lovasz_rows(False)


# ---- integer counting kernels -----------------------------------------------------------------------------------------------------------
@row("onehot_to_ids", ("fcn8s_onehot_to_ids",))
class _:
    @staticmethod
    def make(seed):
        rng = np.random.default_rng(seed)
        ids = rng.integers(0, 20, 1031)
        oh = np.eye(20, dtype=np.uint8)[ids]
        oh[::17] = 0                                                 # all-zero rows -> 255
        return Case(dict(oh=oh, bad=np.zeros(1, np.int32)), dict(ids=((1031,), np.uint8)), fetch=("ids", "bad"), poison=dict(oh=np.roll(oh, 1, axis=1), bad=np.full(1, 77, np.int32)))

    @staticmethod
    def call(L, s, b, case):
        L.check(L.lib.fcn8s_onehot_to_ids(s, ptr(b["oh"]), 1, 1031, 20, ptr(b["ids"]), ptr(b["bad"])))

    @staticmethod
    def check(case, got):
        oh = case.inp["oh"]
        want = np.where(oh.any(1), oh.argmax(1), 255).astype(np.uint8)
        assert np.array_equal(got["ids"], want) and int(got["bad"][0]) == int((oh.sum(1) != 1).sum())


@row("confusion", ("fcn8s_op_confusion",))
class _:
    @staticmethod
    def make(seed):
        rng = np.random.default_rng(5 + seed)
        lab = rng.integers(0, 20, 4099).astype(np.uint8); pred = rng.integers(0, 20, 4099).astype(np.int64)
        return Case(dict(lab=lab, pred=pred, conf=np.zeros(400, np.int64)), fetch=("conf",), poison=dict(conf=np.full(400, 1 << 40, np.int64)))

    @staticmethod
    def call(L, s, b, case):
        L.check(L.lib.fcn8s_op_confusion(s, ptr(b["lab"]), ptr(b["pred"]), 4099, ptr(b["conf"]), 20))

    @staticmethod
    def check(case, got):
        assert np.array_equal(got["conf"].reshape(20, 20), orc.confusion_matrix(case.inp["lab"], case.inp["pred"], 20))


def cs_maps(seed, N, Hh, W):
    """Label-id maps with a few car / person instances, and a damaged train-id prediction."""
    rng = np.random.default_rng(seed)
    gt = np.full((N, Hh, W), 7, np.uint8)                            # road
    inst = np.full((N, Hh, W), 7, np.uint16)
    for n in range(N):
        for k in range(4):
            y, x = int(rng.integers(0, Hh - 8)), int(rng.integers(0, W - 8))
            lab = 26 if k % 2 else 24
            gt[n, y:y + 8, x:x + 8] = lab
            inst[n, y:y + 8, x:x + 8] = lab * 1000 + k
    pred = rng.integers(0, 19, (N, Hh, W)).astype(np.int64)
    return gt, inst, pred


@row("cityscapes_pair", ("fcn8s_op_cityscapes_pair",))
class _:
    N, HW, ME = 2, (24, 40), 16

    @staticmethod
    def make(seed):
        gt, inst, pred = cs_maps(seed, 2, 24, 40)
        L = lib()
        nwork = int(L.lib.fcn8s_op_cityscapes_work_bytes(2))
        return Case(dict(gt=gt, inst=inst, pred=pred, conf=np.zeros(34 * 34, np.int64)),
                    dict(work=((nwork,), np.uint8), entries=((2, 16, 4), np.int32), counts=((2, 3), np.int64)), fetch=("conf", "entries", "counts"),
                    poison=dict(conf=np.full(34 * 34, 1 << 40, np.int64)))

    @staticmethod
    def call(L, s, b, case):
        L.check(L.lib.fcn8s_op_cityscapes_pair(s, ptr(b["gt"]), ptr(b["inst"]), ptr(b["pred"]), 0, 2, 24 * 40, ptr(b["conf"]), ptr(b["work"]), ptr(b["entries"]),
                                               16, ptr(b["counts"])))

    @staticmethod
    def check(case, got):
        i = case.inp
        conf, entries = cs.pair_counts_numpy(i["pred"], i["gt"], i["inst"])
        assert np.array_equal(got["conf"].reshape(34, 34), conf)
        for n in range(2):
            k = int(got["counts"][n, 0])
            assert k == len(entries[n]) and k > 0 and got["counts"][n, 1] == 0 and got["counts"][n, 2] == 0
            assert np.array_equal(got["entries"][n, :k].astype(np.int64), np.asarray(entries[n], np.int64))


@row("boundary_pair + boundary_distance", ("fcn8s_op_boundary_pair", "fcn8s_op_boundary_distance"))
class _:
    @staticmethod
    def make(seed):
        gt, _, pred = cs_maps(10 + seed, 2, 24, 40)
        R = 3
        return Case(dict(gt=gt, pred=pred, rings=np.zeros((R + 1) * 34 * 34, np.int64), bprec=np.zeros((R + 2) * 34, np.int64), brec=np.zeros((R + 2) * 34, np.int64),
                         bad=np.zeros(1, np.int64)), dict(codes=((2, 24, 40), np.uint8)), fetch=("rings", "bprec", "brec", "bad", "codes"),
                    poison={k: np.full(n, 1 << 40, np.int64) for k, n in (("rings", 4 * 34 * 34), ("bprec", 5 * 34), ("brec", 5 * 34), ("bad", 1))})

    @staticmethod
    def call(L, s, b, case):
        L.check(L.lib.fcn8s_op_boundary_pair(s, ptr(b["gt"]), ptr(b["pred"]), 0, 2, 24, 40, 3, ptr(b["rings"]), ptr(b["bprec"]), ptr(b["brec"]), ptr(b["bad"])))
        L.check(L.lib.fcn8s_op_boundary_distance(s, ptr(b["gt"]), 2, 24, 40, 3, ptr(b["codes"])))

    @staticmethod
    def check(case, got):
        i = case.inp
        rings, bprec, brec = cs.boundary_counts_numpy(i["pred"], i["gt"], 3)
        assert np.array_equal(got["rings"].reshape(rings.shape), rings) and np.array_equal(got["bprec"].reshape(bprec.shape), bprec)
        assert np.array_equal(got["brec"].reshape(brec.shape), brec) and int(got["bad"][0]) == 0
        assert np.array_equal(got["codes"], LM.boundary_codes_numpy(i["gt"], 3))


@row("reliability_pair", ("fcn8s_op_reliability_pair",))
class _:
    @staticmethod
    def make(seed):
        prob, gt, lut, scores, scales, ref = relt.case(1, 257, 20, 1, 15, seed=seed)
        z = lambda *s: np.zeros(s, np.int64)
        inp = dict(prob=np.array(prob), gt=np.array(gt), lut=np.array(lut), score=np.array(scores[0]), calib=z(15, 3), sums=z(4), hist=z(2, relt.M, 2), bad=z(2))
        return Case(inp, fetch=relt.NAMES, poison={k: np.full(inp[k].shape, 1 << 40, np.int64) for k in relt.NAMES}, scales=scales, ref=ref)

    @staticmethod
    def call(L, s, b, case):
        L.check(relt.call(b["prob"], b["gt"], b["lut"], [b["score"]], case.aux["scales"], 1, 257, 20, 15, [b[k] for k in relt.NAMES], stream=s))

    @staticmethod
    def check(case, got):
        relt.check(tuple(got[k] for k in relt.NAMES), case.aux["ref"], "streams")


@row("temperature_nll + temperature_apply", ("fcn8s_op_temperature_nll", "fcn8s_op_temperature_apply"))
class _:
    @staticmethod
    def make(seed):
        prob, gt, betas, E, r64 = tst.reference(1, 300, 20, 8, seed=seed)
        return Case(dict(prob=np.array(prob), gt=np.array(gt), lut=np.array(tst.IDENTITY), tables=np.zeros((1, 11), np.int64)),
                    dict(q=F(1, 300, 20), ent=F(1, 300)), fetch=("tables", "q", "ent"), poison=dict(tables=np.full((1, 11), 1 << 40, np.int64)),
                    ref=(prob, gt, betas, E, r64))

    @staticmethod
    def call(L, s, b, case):
        L.check(tst.call_nll(b["prob"], b["gt"], b["lut"], 1, 300, 20, case.aux["ref"][2], b["tables"], stream=s))
        L.check(L.lib.fcn8s_op_temperature_apply(s, ptr(b["prob"]), 1, 300, 20, 0.4, ptr(b["q"]), ptr(b["ent"])))

    @staticmethod
    def check(case, got):
        t = got["tables"][0]
        tst.check_nll((t[:8], int(t[8]), t[9:]), case.aux["ref"], "streams")
        tst.check_apply(got["q"], got["ent"], np.array(case.aux["ref"][0]), 0.4, "streams")


def region_map(seed, N, Hh, W):
    rng = np.random.default_rng(seed)
    coarse = rng.integers(0, 4, (N, Hh // 4 + 1, W // 4 + 1))
    Lm = np.repeat(np.repeat(coarse, 4, 1), 4, 2)[:, :Hh, :W].astype(np.uint8)
    salt = rng.random((N, Hh, W)) < 0.05
    Lm[salt] = rng.integers(0, 4, int(salt.sum()))
    return Lm


@row("regions_label + regions_clean + regions_status", ("fcn8s_op_regions_label", "fcn8s_op_regions_clean", "fcn8s_op_regions_status"))
class _:
    @staticmethod
    def make(seed):
        Lm = region_map(seed, 2, 21, 37)
        table = np.zeros(256, np.int32); table[:4] = 6
        nwork = int(lib().lib.fcn8s_op_regions_work_bytes(2, 21, 37))
        return Case(dict(labels=Lm, cleaned=Lm.copy(), table=table), dict(comp=((2, 21, 37), np.int32), area=((2, 21, 37), np.int32), work=((nwork,), np.uint8),
                                                                         stats=((2, 4), np.int64)), fetch=("comp", "area", "cleaned", "stats"))

    @staticmethod
    def call(L, s, b, case):
        st = (C.c_int64 * 2)(-1, -1)
        L.check(L.lib.fcn8s_op_regions_label(s, ptr(b["labels"]), 1, 2, 21, 37, 8, ptr(b["comp"]), ptr(b["area"]), ptr(b["work"])))
        L.check(L.lib.fcn8s_op_regions_status(s, ptr(b["work"]), st))
        L.check(L.lib.fcn8s_op_regions_clean(s, ptr(b["cleaned"]), 1, 2, 21, 37, 4, ptr(b["table"]), 2, ptr(b["work"]), ptr(b["stats"])))
        st2 = (C.c_int64 * 2)(-1, -1)
        L.check(L.lib.fcn8s_op_regions_status(s, ptr(b["work"]), st2))
        return dict(status=np.array([st[0], st[1], st2[0], st2[1]]))

    @staticmethod
    def check(case, got):
        Lm = case.inp["labels"]
        comp, area = RG.components_numpy(Lm, 8)
        assert np.array_equal(got["comp"], comp) and np.array_equal(got["area"], area)
        out = RG.clean_numpy(Lm, case.inp["table"], 4, 2)
        out, stats = out if isinstance(out, tuple) else (out, None)
        assert np.array_equal(got["cleaned"], out) and (got["cleaned"] != Lm).any()
        if stats is not None:
            assert np.array_equal(got["stats"], np.asarray(stats).reshape(2, 4))
        assert got["status"].tolist() == [0, 0, 0, 0]


# ---- inference kernels -----------------------------------------------------------------------------------------------------------------
@row("preprocess + tta_input", ("fcn8s_op_preprocess", "fcn8s_op_tta_input"))
class _:
    @staticmethod
    def make(seed):
        rng = np.random.default_rng(7 + seed)
        img = rng.integers(0, 256, (2, 4, 8, 3), dtype=np.uint8)
        big = rng.integers(0, 256, (1, 41, 27, 3), dtype=np.uint8)
        # test_tta_input_is_resize_flip_preprocess_pad's reference: the host's resize and mirror through the preprocess kernel
        rs = np.ascontiguousarray(cv2_compat.resize_linear(big[0], 31, 20)[:, ::-1])
        return Case(dict(img=img, big=big, rs=rs), dict(pre=F(2, 4, 8, 4), tin=F(1, 32, 32, 4), rpre=F(31, 20, 4)))

    @staticmethod
    def call(L, s, b, case):
        L.check(L.lib.fcn8s_op_preprocess(s, ptr(b["img"]), 0, ptr(b["pre"]), 2 * 4 * 8))
        L.check(L.lib.fcn8s_op_tta_input(s, ptr(b["big"]), 1, 41, 27, 31, 20, 32, 32, 1, ptr(b["tin"])))
        L.check(L.lib.fcn8s_op_preprocess(s, ptr(b["rs"]), 0, ptr(b["rpre"]), 31 * 20))

    @staticmethod
    def check(case, got):
        ref = orc.preprocess_t(torch.tensor(case.inp["img"]).float()).numpy()
        np.testing.assert_allclose(got["pre"][..., :3], ref, rtol=0, atol=1e-5)                  # test_preprocess's bar
        assert (got["pre"][..., 3] == 0).all()
        want = np.zeros((1, 32, 32, 4), f32)
        want[0, :31, :20] = got["rpre"]
        assert same_bits(got["tin"], want)


@row("tta_accumulate", ("fcn8s_op_tta_accumulate",))
class _:
    P, SH = 2, (2, 32, 32, 17, 23, 40, 31, 4)                        # N, Hp, Wp, Hs, Ws, H, W, C: ACC_CASES' (4, (17, 23), (40, 31)) with two passes

    @staticmethod
    def make(seed):
        rng = np.random.default_rng(seed)
        lg = rng.normal(0, 4, (2, 2, 32, 32, 4)).astype(f32)
        lg[:, :, 17:] = 1e6; lg[:, :, :, 23:] = 1e6                  # padding region: never read
        return Case(dict(l0=lg[0], l1=lg[1]), dict(acc=F(2, 40, 31, 4), sm=F(2, 40, 31, 4), am=((2, 40, 31), np.int64)), fetch=("sm", "am"))

    @staticmethod
    def call(L, s, b, case):
        for k in range(2):
            L.check(L.lib.fcn8s_op_tta_accumulate(s, ptr(b["l%d" % k]), 2, 32, 32, 17, 23, k % 2, 4, 40, 31, ptr(b["acc"]), int(k == 0), int(k == 1), 2,
                                                  ptr(b["sm"]), ptr(b["am"])))

    @staticmethod
    def check(case, got):
        lgs = [case.inp["l0"][:, :17, :23], case.inp["l1"][:, :17, :23]]
        ref = ttat.torch_reference(lgs, [False, True], 40, 31)
        ttat.check_probs(got["sm"], ref, 1e-6)
        ttat.check_argmax(got["am"], ref)


@row("mc_accumulate", ("fcn8s_op_mc_accumulate",))
class _:
    @staticmethod
    def make(seed):
        x = mct.make_logits(np.random.default_rng(seed), 3, (2, 17, 33), 20, 1)
        return Case(dict(x0=x[0], x1=x[1], x2=x[2]), dict(acc=F(2, 17, 33, 20), eacc=F(2, 17, 33), sm=F(2, 17, 33, 20), am=((2, 17, 33), np.int64),
                                                         ent=F(2, 17, 33), mi=F(2, 17, 33)), fetch=("sm", "am", "ent", "mi"), x=x)

    @staticmethod
    def call(L, s, b, case):
        for k in range(3):
            L.check(L.lib.fcn8s_op_mc_accumulate(s, ptr(b["x%d" % k]), 2, 17, 33, 20, ptr(b["acc"]), ptr(b["eacc"]), int(k == 0), int(k == 2), 3,
                                                 ptr(b["sm"]), ptr(b["am"]), ptr(b["ent"]), ptr(b["mi"])))

    @staticmethod
    def check(case, got):
        ref, bar = mct.bar_of(case.aux["x"])
        mct.check_case(case.aux["x"], (got["sm"], got["am"], got["ent"], got["mi"]), ref, bar, "streams")


@row("crf_meanfield", ("fcn8s_op_crf_meanfield",))
class _:
    PAR = dict(iterations=2, radius=3, dilation=2, w_appearance=4.0, w_smooth=2.0)

    @staticmethod
    def make(seed):
        prob, img = crft.scenes(1, 5, 7, 20, seed=12 + seed)           # KERNEL_CASES' (1, 5, 7, 20, 3, 2, 2, 4.0, 2.0)
        cp = crft.struct(crf.Params(iterations=2, radius=3, dilation=2, w_appearance=4.0, w_smooth=2.0))
        nwork = max(int(lib().lib.fcn8s_op_crf_work_floats(1, 5, 7, 20, C.byref(cp))), 4)
        return Case(dict(prob=prob.astype(f32), img=img), dict(work=F(nwork), q=F(1, 5, 7, 20), am=((1, 5, 7), np.int64)), fetch=("q", "am"), cp=cp)

    @staticmethod
    def call(L, s, b, case):
        L.check(L.lib.fcn8s_op_crf_meanfield(s, ptr(b["prob"]), ptr(b["img"]), 1, 5, 7, 20, C.byref(case.aux["cp"]), ptr(b["work"]), ptr(b["q"]), ptr(b["am"])))

    @staticmethod
    def check(case, got):
        prob, img = case.inp["prob"], case.inp["img"]
        p = crf.Params(iterations=2, radius=3, dilation=2, w_appearance=4.0, w_smooth=2.0)
        ref = crf.meanfield(prob, img, p, dtype=np.float64)
        d32 = float(np.abs(crf.meanfield(prob, img, p, dtype=np.float32).astype(np.float64) - ref).max())
        assert float(np.abs(got["q"].astype(np.float64) - ref).max()) <= 8.0 * max(d32, 2.0 ** -23)      # test_kernel_matches_the_float64_restatement's gate
        assert np.array_equal(got["am"], got["q"].argmax(-1))


@row("augment_u8 + resample_u8", ("fcn8s_op_augment_u8", "fcn8s_op_resample_u8"))
class _:
    @staticmethod
    def make(seed):
        rng = np.random.default_rng(seed)
        img = rng.integers(0, 256, (2, 12, 20, 3), dtype=np.uint8)
        lab = rng.integers(0, 20, (2, 12, 20)).astype(np.uint8)
        apar = np.array([[2, 3, 1, 0], [0, 1, 0, 0]], np.int32)         # y offset, x offset, flip, brightness
        rpar = np.array([[9, 15, 1, 2], [16, 24, -2, -3]], np.int32)    # resized height, width, y offset, x offset
        zero = np.zeros((2, 4), np.int32)
        return Case(dict(img=img, lab=lab, apar=apar, rpar=rpar), dict(aimg=((2, 8, 16, 3), np.uint8), alab=((2, 8, 16), np.uint8), rimg=((2, 12, 20, 3), np.uint8),
                                                                     rlab=((2, 12, 20), np.uint8)),
                    poison=dict(apar=zero, rpar=np.array([[12, 20, 0, 0], [12, 20, 0, 0]], np.int32)))      # sizes and offsets: other VALID ones

    @staticmethod
    def call(L, s, b, case):
        L.check(L.lib.fcn8s_op_augment_u8(s, ptr(b["img"]), ptr(b["lab"]), ptr(b["aimg"]), ptr(b["alab"]), ptr(b["apar"]), None, 2, 12, 20, 8, 16, 255))
        L.check(L.lib.fcn8s_op_resample_u8(s, ptr(b["img"]), ptr(b["lab"]), ptr(b["rimg"]), ptr(b["rlab"]), ptr(b["rpar"]), 2, 12, 20, 12, 20, 255))

    @staticmethod
    def check(case, got):
        img, lab, apar, rpar = (case.inp[k] for k in ("img", "lab", "apar", "rpar"))

        def place(src, Ho, Wo, oy, ox, fill):
            out = np.full((Ho, Wo) + src.shape[2:], fill, np.uint8)
            ys, xs = max(0, oy), max(0, ox)
            ye, xe = min(Ho, oy + src.shape[0]), min(Wo, ox + src.shape[1])
            if ye > ys and xe > xs:
                out[ys:ye, xs:xe] = src[ys - oy:ye - oy, xs - ox:xe - ox]
            return out
        for n in range(2):
            oy, ox, flip, _ = (int(v) for v in apar[n])
            # out[y, x] = in[y + oy, (flip ? Wo - 1 - x : x) + ox]
            wi, wl = place(img[n], 8 + oy, 16 + ox, 0, 0, 0)[oy:, ox:], place(lab[n], 8 + oy, 16 + ox, 0, 0, 255)[oy:, ox:]
            if flip:
                wi, wl = wi[:, ::-1], wl[:, ::-1]
            assert np.array_equal(got["aimg"][n], wi) and np.array_equal(got["alab"][n], wl)
            rh, rw, oy, ox = (int(v) for v in rpar[n])
            assert np.array_equal(got["rimg"][n], place(cv2_compat.resize_linear(img[n], rh, rw), 12, 20, oy, ox, 0))
            assert np.array_equal(got["rlab"][n], place(cv2_compat.resize_nearest(lab[n], rh, rw), 12, 20, oy, ox, 255))


# ---- the update kernels at n = 100003 ---------------------------------------------------------------------------------------------------
NU = 100003
LR_A, LR_S, GS, OMEGA = 1e-3, 1e-2, 0.37, np.float32(1.0 - 0.999)


def update_inputs(seed):
    rng = np.random.default_rng(6 + seed)
    return dict(th=rng.standard_normal(NU).astype(f32), g=rng.standard_normal(NU).astype(f32), m=(rng.standard_normal(NU) * 0.1).astype(f32),
                v=(rng.standard_normal(NU) ** 2).astype(f32), sh=rng.standard_normal(NU).astype(f32))


def check_adam(i, got, s, t="th", m="m", v="v"):
    # test_optimizers' bars (2e-6 on theta, 1e-6 on the slots, absolute, for slots below 1); the slots here start from values up to 16, so
    # the slot bars are taken relative to the largest entry: 1e-6 of 16 is 8 fp32 ulps there, as 1e-6 is 8 ulps of 1
    th, mm, vv = optim.adam_step(i["th"], i["g"], i["m"], i["v"], 3, LR_A, s)
    assert np.abs(got[t] - th).max() < 2e-6 and np.abs(got[m] - mm).max() < 1e-6 * max(1.0, np.abs(mm).max())      # test_optimizers' bars
    assert np.abs(got[v] - vv).max() < 1e-6 * max(1.0, np.abs(vv).max()) and not np.array_equal(got[t], i["th"])


def check_sgd(i, got, s, t="th2", m="buf"):
    th, bb = optim.sgd_step(i["th"], i["g"], i["m"], LR_S, s)
    assert np.abs(got[t] - th).max() < 2e-6 and np.abs(got[m] - bb).max() < 2e-6 and not np.array_equal(got[t], i["th"])


def check_ema(s0, theta, got_s):
    bound = 4.0 * 2.0 ** -23 * np.maximum(np.abs(s0), np.abs(theta)).astype(np.float64)           # test_ema_update_against_float64's bound
    assert (np.abs(got_s.astype(np.float64) - optim.ema_step(s0, theta, OMEGA)) <= bound).all()
    assert not np.array_equal(got_s, s0)


@row("tf_adam + sgd_momentum", ("fcn8s_op_tf_adam", "fcn8s_op_sgd_momentum"))
class _:
    @staticmethod
    def make(seed):
        i = update_inputs(seed)
        return Case(dict(th=i["th"], g=i["g"], m=i["m"], v=i["v"], th2=i["th"].copy(), buf=i["m"].copy()), fetch=("th", "m", "v", "th2", "buf"), i=i)

    @staticmethod
    def call(L, s, b, case):
        L.check(L.lib.fcn8s_op_tf_adam(s, ptr(b["th"]), ptr(b["g"]), ptr(b["m"]), ptr(b["v"]), NU, 3, LR_A, 0.9, 0.999, 1e-8, GS))
        L.check(L.lib.fcn8s_op_sgd_momentum(s, ptr(b["th2"]), ptr(b["g"]), ptr(b["buf"]), NU, LR_S, 0.9, GS))

    @staticmethod
    def check(case, got):
        check_adam(case.aux["i"], got, GS)
        check_sgd(case.aux["i"], got, GS)


@row("grad_norm + tf_adam_dev + sgd_momentum_dev", ("fcn8s_op_grad_norm", "fcn8s_op_tf_adam_dev", "fcn8s_op_sgd_momentum_dev"))
class _:
    @staticmethod
    def make(seed):
        i = update_inputs(seed)
        return Case(dict(th=i["th"], g=i["g"], m=i["m"], v=i["v"], th2=i["th"].copy(), buf=i["m"].copy()), dict(slab=F(5)),
                    fetch=("th", "m", "v", "th2", "buf", "slab"), i=i)

    @staticmethod
    def call(L, s, b, case):
        L.check(L.lib.fcn8s_op_grad_norm(s, ptr(b["g"]), NU, 0.5, 40.0, ptr(b["slab"])))            # |g| ~ 316, scaled 158: the clip bites
        L.check(L.lib.fcn8s_op_tf_adam_dev(s, ptr(b["th"]), ptr(b["g"]), ptr(b["m"]), ptr(b["v"]), NU, 3, LR_A, 0.9, 0.999, 1e-8, ptr(b["slab"])))
        L.check(L.lib.fcn8s_op_sgd_momentum_dev(s, ptr(b["th2"]), ptr(b["g"]), ptr(b["buf"]), NU, LR_S, 0.9, ptr(b["slab"])))

    @staticmethod
    def check(case, got):
        i = case.aux["i"]
        norm, c, s, ok, zero = got["slab"]
        want = optim.global_norm(i["g"], 0.5)
        assert abs(float(norm) - float(want)) <= 4 * float(np.spacing(want)) and ok == 1.0 and zero == 0.0 and c < 1.0      # test_grad_norm_against_float64's bar
        cw, sw, _ = optim.clip_scale(norm, 0.5, 40.0)
        assert abs(float(c) - float(cw)) <= 2 * float(np.spacing(cw)) and abs(float(s) - float(sw)) <= 2 * float(np.spacing(sw))
        check_adam(i, got, float(s))
        check_sgd(i, got, float(s))


@row("tf_adam_ema + sgd_momentum_ema", ("fcn8s_op_tf_adam_ema", "fcn8s_op_sgd_momentum_ema"))
class _:
    @staticmethod
    def make(seed):
        i = update_inputs(seed)
        return Case(dict(th=i["th"], g=i["g"], m=i["m"], v=i["v"], sh=i["sh"], th2=i["th"].copy(), buf=i["m"].copy(), sh2=i["sh"].copy()),
                    fetch=("th", "m", "v", "sh", "th2", "buf", "sh2"), i=i)

    @staticmethod
    def call(L, s, b, case):
        L.check(L.lib.fcn8s_op_tf_adam_ema(s, ptr(b["th"]), ptr(b["g"]), ptr(b["m"]), ptr(b["v"]), ptr(b["sh"]), NU, 3, LR_A, 0.9, 0.999, 1e-8, GS, None, float(OMEGA)))
        L.check(L.lib.fcn8s_op_sgd_momentum_ema(s, ptr(b["th2"]), ptr(b["g"]), ptr(b["buf"]), ptr(b["sh2"]), NU, LR_S, 0.9, GS, None, float(OMEGA)))

    @staticmethod
    def check(case, got):
        i = case.aux["i"]
        check_adam(i, got, GS)
        check_sgd(i, got, GS)
        check_ema(i["sh"], got["th"], got["sh"])
        check_ema(i["sh"], got["th2"], got["sh2"])


@row("grad_accumulate + ema_update + swap", ("fcn8s_op_grad_accumulate", "fcn8s_op_ema_update", "fcn8s_op_swap"))
class _:
    @staticmethod
    def make(seed):
        i = update_inputs(seed)
        return Case(dict(dst=i["m"], src=i["g"], dst0=i["v"], sh=i["sh"], th=i["th"], a=i["th"].copy(), b=i["g"].copy()), fetch=("dst", "dst0", "sh", "a", "b"), i=i)

    @staticmethod
    def call(L, s, b, case):
        L.check(L.lib.fcn8s_op_grad_accumulate(s, ptr(b["dst"]), ptr(b["src"]), NU, 1))
        L.check(L.lib.fcn8s_op_grad_accumulate(s, ptr(b["dst0"]), ptr(b["src"]), NU, 0))
        L.check(L.lib.fcn8s_op_ema_update(s, ptr(b["sh"]), ptr(b["th"]), NU, float(OMEGA), None))
        L.check(L.lib.fcn8s_op_swap(s, ptr(b["a"]), ptr(b["b"]), NU))

    @staticmethod
    def check(case, got):
        i = case.aux["i"]
        assert np.array_equal(got["dst"], (i["m"] + i["g"]).astype(f32)) and np.array_equal(got["dst0"], i["g"])       # == NumPy float32, as the op tests ask
        check_ema(i["sh"], i["th"], got["sh"])
        assert same_bits(got["a"], i["g"]) and same_bits(got["b"], i["th"])


# ---- the case table --------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def default_result(index):
    """The row's call on the default stream with the test's own inputs, once, shared by both skews and never written.  A call on other
    data goes first, so that the second one's host time (row.host_ms, which the row's delay must outlast) is a warm call's."""
    r = ROWS[index]
    case = r.make(1)
    execute(r, r.make(2), None, None, None)
    got = execute(r, case, None, None, None)
    r.check(case, got)
    return case, got


@pytest.mark.parametrize("skew", SKEWS)
@pytest.mark.parametrize("index", range(len(ROWS)), ids=[r.name.replace(" ", "_") for r in ROWS])
def test_op_on_a_side_stream(index, skew, H):
    r = ROWS[index]
    case, want = default_result(index)
    H.longest_host_ms = max(H.longest_host_ms, r.host_ms)
    execute(r, r.make(2), H, H.S, "side_late" if skew == "null_late" else "null_late")           # warm-up on S: other data, the (device, S) scratch
    got = execute(r, case, H, H.S, skew)
    r.check(case, got)                                                                           # (1) the float64 reference at the entry's own bar
    if r.bitwise:                                                                                # (2) the default stream, bit for bit
        for k in want:
            assert same_bits(np.asarray(got[k]), np.asarray(want[k])), "%s: '%s' on the side stream differs from the default stream's" % (r.name, k)


# ---- model level -----------------------------------------------------------------------------------------------------------------------
from tests.test_state_coherence_gpu import CLASSES, SHAPE_A, SHAPE_B, WIDTHS, params  # noqa: E402


def fresh(precision, options=None, seed=1):
    """test_state_coherence_gpu.fresh with `deterministic` = 1: a model created directly in its state."""
    from tests.test_state_coherence_gpu import fresh as make
    e = make(precision, params(seed)[1], options=dict(deterministic=1, **(options or {})))
    return e


def host_batch(shape, seed):
    rng = np.random.default_rng(seed)
    return rng.integers(0, 256, shape + (3,), dtype=np.uint8), rng.integers(0, CLASSES, shape, dtype=np.uint8)


def dev_batch(shape, seed):
    img, lab = host_batch(shape, seed)
    return torch.from_numpy(img).cuda(), torch.from_numpy(lab).cuda()


class Drive:
    """Runs steps on an engine: on `stream` under `skew`, or (stream None) on the default stream with no skew.  A step is
    fn(engine, images, labels) -> result; its inputs are device tensors written on the step's stream (behind the delay under 'side late')."""

    def __init__(self, H, engine, stream=None, skew=None, first_params=None):
        self.H, self.e, self.stream, self.skew = H, engine, stream, skew
        self.first_params = first_params.cuda() if first_params is not None else None      # (made now: every step's prepare() synchronises behind it)
        self.keep = []                                               # nothing is freed during a case
        self.ready = {}

    def prepare(self, batches):
        """Make the device buffers of later steps now, so that those steps need no synchronise of their own."""
        for shape, seed in batches:
            img_h, lab_h = host_batch(shape, seed)
            self.ready[(shape, seed)] = (torch.from_numpy(img_h).cuda(), torch.from_numpy(lab_h).cuda(),
                                         torch.from_numpy(np.ascontiguousarray(img_h[:, ::-1])).cuda(),          # poison: another image,
                                         torch.from_numpy(poison_of(lab_h)).cuda())                              # other in-range labels
        torch.cuda.synchronize()

    def step(self, fn, shape, seed, asynchronous=False, stream="same", delayed=True):
        stream = self.stream if stream == "same" else stream
        flat = self.first_params
        self.first_params = None
        twin = stream is None and self.skew is None
        made = (shape, seed) in self.ready
        if not made:
            assert delayed or twin, "a step without a delay has its buffers prepared in advance"
            self.prepare([(shape, seed)])
        simg, slab, img, lab = self.ready.pop((shape, seed))
        if twin:
            if flat is not None:
                self.e.flat_params.copy_(flat)
            out = fn(self.e, simg, slab)
            torch.cuda.synchronize()
            return out
        sflat = flat
        self.keep += [simg, slab, img, lab, sflat]
        if not made:
            torch.cuda.synchronize()
        ctx = torch.cuda.stream(stream) if stream is not None else torch.cuda.stream(torch.cuda.default_stream())
        if not delayed:                                              # no delay in front of the call: it races whatever is still queued elsewhere
            ev = None
            if self.skew == "null_late" and stream is not None:      # ... and whatever it sends to the NULL stream lands late
                with torch.cuda.stream(torch.cuda.default_stream()):
                    ev = self.H.delay("model")
            with ctx:
                img.copy_(simg); lab.copy_(slab)
                out = fn(self.e, img, lab)
                if asynchronous and ev is not None:
                    assert not ev.query(), "the call returned after the delay ended: the skew did not cover its enqueue (delay %.1f ms)" % self.H.delay_ms["model"]
        elif self.skew == "side_late":
            with ctx:
                if sflat is not None:
                    self.e.flat_params.fill_(float("nan"))
                ev = self.H.delay("model")
                img.copy_(simg); lab.copy_(slab)
                if sflat is not None:
                    self.e.flat_params.copy_(sflat)
                out = fn(self.e, img, lab)
                if asynchronous:
                    assert not ev.query(), "the call returned after the delay ended: the skew did not cover its enqueue (delay %.1f ms)" % self.H.delay_ms["model"]
        else:
            with ctx:
                img.copy_(simg); lab.copy_(slab)
                if sflat is not None:
                    self.e.flat_params.copy_(sflat)
            (stream or torch.cuda.default_stream()).synchronize()
            other = torch.cuda.default_stream() if stream is not None else self.H.S2
            with torch.cuda.stream(other):
                ev = self.H.delay("model")
            with ctx:
                out = fn(self.e, img, lab)
                if asynchronous:
                    assert not ev.query(), "the call returned after the delay ended: the skew did not cover its enqueue (delay %.1f ms)" % self.H.delay_ms["model"]
        return out

    def state(self):
        """Everything a sequence leaves behind, after a full device synchronise."""
        torch.cuda.synchronize()
        ctx = torch.cuda.stream(self.stream) if self.stream is not None else torch.cuda.stream(torch.cuda.default_stream())
        with ctx:
            e = self.e
            m, v = e.get_opt_state()
            st = dict(params=e.flat_params.detach().cpu().numpy(), grads=e.flat_grads.detach().cpu().numpy(), m=m, v=v, step=e.global_step)
            if e.ema_info()["has_shadow"]:
                st["ema"] = e.get_ema()
        torch.cuda.synchronize()
        return st


def assert_same(a, b, what=""):
    """Bit for bit, through nested tuples / dicts / arrays / scalars."""
    if isinstance(a, dict):
        assert a.keys() == b.keys(), (what, a.keys(), b.keys())
        for k in a:
            assert_same(a[k], b[k], "%s.%s" % (what, k))
    elif isinstance(a, (tuple, list)):
        assert len(a) == len(b), what
        for i, (x, y) in enumerate(zip(a, b)):
            assert_same(x, y, "%s[%d]" % (what, i))
    elif a is None or b is None:
        assert a is None and b is None, what
    elif isinstance(a, torch.Tensor):
        assert_same(a.cpu().numpy(), b.cpu().numpy(), what)
    else:
        x, y = np.asarray(a), np.asarray(b)
        assert same_bits(x, y), "%s: the side stream's result differs from the default stream's (%d of %d elements)" % (
            what, int((x != y).sum()) if x.shape == y.shape else -1, x.size)


def run_both(H, precision, sequence, options=None):
    """sequence(drive) -> results; run on the twin (default stream, no skew), then on a fresh engine on S under each skew; everything
    returned and everything left behind must match bit for bit."""
    flat = params(1)[1]
    twin = fresh(precision, options)
    d = Drive(H, twin, first_params=flat)
    want = sequence(d)
    want_state = d.state()
    assert np.abs(want_state["params"] - flat.numpy()).max() > 0 or not want_state["step"], "the sequence did not move the parameters"
    twin.close()
    for skew in SKEWS:
        e = fresh(precision, options, seed=2)                        # other parameters until the first step writes the real ones on S
        with torch.cuda.stream(H.S):                                 # warm-up on S with other data: scratch, workspace, one-time allocations
            wi, wl = dev_batch(SHAPE_A, 77)
            if precision == "fp8_infer":
                e.calibrate_fp8(wi, reset=True)
            else:
                e.train_step(wi, wl, 1e-4, keep_prob=1.0)
            e.predict(wi)
            e.global_step = 0; e.flat_grads.zero_()
            e.set_opt_state(np.zeros(flat.numel(), f32), np.zeros(flat.numel(), f32))
        torch.cuda.synchronize()
        d = Drive(H, e, H.S, skew, first_params=flat)
        got = sequence(d)
        got_state = d.state()
        assert_same(got, want, "%s %s results" % (precision, skew))
        assert_same(got_state, want_state, "%s %s state" % (precision, skew))
        e.close()


TRAIN_PRECISIONS = ("fp32", "bf16_fwd", "bf16_train")


def moved_params(e, before):
    torch.cuda.synchronize()
    now = e.flat_params.detach().cpu().numpy()
    assert np.abs(now - before).max() > 0, "the step did not move the parameters: the test has no force"
    return now


@pytest.mark.parametrize("precision", TRAIN_PRECISIONS)
def test_training_on_a_side_stream_equals_the_default_stream(precision, H):
    """Two train_steps (the first without fetching the loss), forward_backward + apply_update, one accumulated micro-batch and a clipped
    train_step with the average on, ema_swap and back."""
    def sequence(d):
        out = []
        out.append(d.step(lambda e, i, l: e.train_step(i, l, 1e-3, keep_prob=0.5, fetch_loss=False), SHAPE_A, 11, asynchronous=True))
        p = moved_params(d.e, params(1)[1].numpy())
        out.append(d.step(lambda e, i, l: e.train_step(i, l, 1e-3, keep_prob=0.5), SHAPE_B, 12))
        p = moved_params(d.e, p)
        out.append(d.step(lambda e, i, l: e.forward_backward(i, l, keep_prob=1.0, l2_rate=1e-4), SHAPE_A, 13))
        out.append(d.step(lambda e, i, l: e.apply_update(1e-3), SHAPE_A, 13, asynchronous=True))
        p = moved_params(d.e, p)
        out.append(d.step(lambda e, i, l: (e.set_ema(0.9), e.set_grad_clip(0.5)), SHAPE_A, 13))
        out.append(d.step(lambda e, i, l: e.accumulate_step(i, l, keep_prob=1.0), SHAPE_A, 14))
        out.append(d.step(lambda e, i, l: (e.train_step(i, l, 1e-3, keep_prob=1.0), e.update_stats(), e.loss_terms()), SHAPE_A, 15))
        p = moved_params(d.e, p)
        out.append(d.step(lambda e, i, l: e.ema_swap(), SHAPE_A, 15, asynchronous=True))
        p = moved_params(d.e, p)
        out.append(d.step(lambda e, i, l: e.predict(i, argmax=False), SHAPE_B, 16))
        out.append(d.step(lambda e, i, l: e.ema_swap(), SHAPE_A, 15, asynchronous=True))
        moved_params(d.e, p)
        return out
    run_both(H, precision, sequence)


@pytest.mark.parametrize("loss", ("set_loss", "set_lovasz", "set_boundary_loss"))
def test_training_losses_on_a_side_stream(loss, H):
    def sequence(d):
        e = d.e
        if loss == "set_loss":
            e.set_loss(class_weights=np.linspace(0.5, 2.0, CLASSES).astype(f32), ohem_thresh=0.7, ohem_min_kept=1000)
        elif loss == "set_lovasz":
            e.set_lovasz(0.5, per_image=True)
        else:
            e.set_boundary_loss(LM.boundary_table(4.0, 3.0, 5), 5)
        out = [d.step(lambda e, i, l: (e.train_step(i, l, 1e-3, keep_prob=1.0), e.loss_terms()), SHAPE_A, 21)]
        moved_params(e, params(1)[1].numpy())
        if loss == "set_loss":
            out.append(e.loss_stats())
        return out
    run_both(H, "fp32", sequence)


def test_evaluation_and_inference_on_a_side_stream(H):
    def sequence(d):
        out = [d.step(lambda e, i, l: (e.eval_step(i, l), e.metrics_get()), SHAPE_A, 31)]
        out.append(d.step(lambda e, i, l: e.predict(i), SHAPE_B, 32))
        out.append(d.step(lambda e, i, l: e.predict_tta(i, scales=(0.75, 1.0), flip=True, argmax=False), SHAPE_A, 33))
        out.append(d.step(lambda e, i, l: e.predict_mc(i, samples=3), SHAPE_A, 34))
        out.append(d.step(lambda e, i, l: e.predict_crf(i, crf.Params(iterations=2), argmax=False), SHAPE_A, 35))
        return out
    run_both(H, "fp32", sequence)


def test_fp8_calibration_and_prediction_on_a_side_stream(H):
    def sequence(d):
        out = [d.step(lambda e, i, l: np.array(e.calibrate_fp8(i, reset=True)), SHAPE_B, 41)]
        out.append(d.step(lambda e, i, l: e.predict(i, argmax=False), SHAPE_A, 42))
        return out
    run_both(H, "fp8_infer", sequence)


def test_staged_inputs_with_the_model_on_a_side_stream(H):
    """stage() -> train_step(Staged): the copy stream's events against m->stream."""
    img, lab = host_batch(SHAPE_A, 51)

    def sequence(d):
        def fn(e, i, l):
            st = e.stage(img, lab, slot=1)
            return e.train_step(st, None, 1e-3, keep_prob=1.0)
        out = [d.step(fn, SHAPE_A, 51)]
        moved_params(d.e, params(1)[1].numpy())
        return out
    run_both(H, "fp32", sequence)


@pytest.mark.parametrize("skew", SKEWS)
def test_free_standing_wrappers_take_the_current_stream(skew, H):
    """regions.py, cityscapes_eval.py, temperature.py, reliability.py: one call each under torch.cuda.stream(S), each under the skew with a
    delay and input buffers of its own, against its default-stream result."""
    gt, inst, pred = cs_maps(3, 2, 24, 40)
    prob, rgt, lut, scores, scales, _ = relt.case(1, 257, 20, 1, 15, seed=1)
    Lm = region_map(3, 2, 21, 37)
    src = dict(Lm=to_dev(Lm), pred=to_dev(pred), gt=to_dev(gt), inst=to_dev(inst), prob=to_dev(np.array(prob).reshape(1, 257, 20)), rgt=to_dev(np.array(rgt)),
               lut=to_dev(np.array(lut)), score=to_dev(np.array(scores[0])))

    def clean(t):
        cleaned = t["Lm"].clone()
        return RG.clean_device(cleaned, 6, 4, 2, stats=True)[0], cleaned
    wrappers = [lambda t: RG.label_device(t["Lm"], 8)[:2], clean,
                lambda t: cs.pair_counts_device(t["pred"], t["gt"], t["inst"]), lambda t: cs.boundary_counts_device(t["pred"], t["gt"], 3),
                lambda t: ts.nll_device(t["prob"], t["rgt"], t["lut"], tst.grid_betas(8)), lambda t: ts.apply_device(t["prob"], 2.0, entropy=True),
                lambda t: rel.counts_device(t["prob"], t["rgt"], t["lut"], [t["score"]], scales, 15)]

    other = {k: v.flip(-1).contiguous() for k, v in src.items()}    # other data of the same value sets, for the warm-up

    def calls(src, skew=None, host_ms=None):
        """-> (results, each call's host time).  Every buffer is made before the first delay starts."""
        bufs = [{k: torch.full(v.shape, float("nan") if v.is_floating_point() else 0, dtype=v.dtype, device="cuda") if skew == "side_late" else v.clone()
                 for k, v in src.items()} for _ in wrappers]
        torch.cuda.synchronize()
        out, ms = [], []
        for i, (fn, t) in enumerate(zip(wrappers, bufs)):
            if skew == "side_late":
                H.delay("op", host_ms[i])
                for k in t:
                    t[k].copy_(src[k])
            elif skew == "null_late":
                with torch.cuda.stream(torch.cuda.default_stream()):
                    H.delay("op", host_ms[i])
            t0 = time.perf_counter()
            out.append(fn(t))
            ms.append((time.perf_counter() - t0) * 1e3)
        torch.cuda.synchronize()
        return out, ms
    torch.cuda.synchronize()
    calls(other)
    want, host_ms = calls(src)                                       # (warm: the times each call's delay must outlast)
    H.longest_host_ms = max([H.longest_host_ms] + host_ms)
    with torch.cuda.stream(H.S):
        calls(other)                                                 # warm-up on S
        got, _ = calls(src, skew, host_ms)
    assert_same(got, want, "wrappers")


@pytest.mark.parametrize("skew", SKEWS)
def test_a_model_moved_between_streams_keeps_its_state_ordered(skew, H):
    """train_step on S under the skew with no synchronise after it, predict with the default stream current, train_step on S2, eval_step on S
    again; the inputs of each call are made on that call's stream.  The twin does the same four calls on the default stream.
    side late: the delay sits in front of the first call alone, and the later calls, on other streams, start at once.  NULL late: the delay is
    queued on the NULL stream in front of every call on a side stream, so the predict on the NULL stream runs behind it, late, and the
    train_step on S2 that follows may not change the parameters before that predict has read them."""
    flat = params(1)[1]

    def four(d, streams):
        # no synchronise between the four calls; one shape throughout: another shape would make the workspace anew, and the hipFree in that
        # synchronises the device, which would order the calls whatever fcn8s_set_stream did
        d.prepare([(SHAPE_A, 61), (SHAPE_A, 62), (SHAPE_A, 63), (SHAPE_A, 64)])
        out = [d.step(lambda e, i, l: e.train_step(i, l, 1e-3, keep_prob=0.5, fetch_loss=False), SHAPE_A, 61, asynchronous=d.skew is not None, stream=streams[0])]
        # no call but the first has a delay in front of it on its own stream: each must wait, on the device, for the one before it
        out.append(d.step(lambda e, i, l: e.predict(i, argmax=False), SHAPE_A, 62, stream=streams[1], delayed=False))
        out.append(d.step(lambda e, i, l: e.train_step(i, l, 1e-3, keep_prob=0.5, fetch_loss=False), SHAPE_A, 63, asynchronous=d.skew is not None,
                          stream=streams[2], delayed=False))
        out.append(d.step(lambda e, i, l: (e.eval_step(i, l), e.metrics_get()), SHAPE_A, 64, stream=streams[3], delayed=False))
        return out
    twin = fresh("fp32")
    d = Drive(H, twin, first_params=flat)
    want = four(d, [None] * 4)
    want_state = d.state()
    assert np.abs(want_state["params"] - flat.numpy()).max() > 0
    twin.close()
    e = fresh("fp32", seed=2)
    for s in (H.S, H.S2):
        with torch.cuda.stream(s):
            wi, wl = dev_batch(SHAPE_A, 78)
            e.train_step(wi, wl, 1e-4, keep_prob=1.0); e.predict(wi)
    with torch.cuda.stream(H.S):
        e.global_step = 0; e.flat_grads.zero_()
        e.set_opt_state(np.zeros(flat.numel(), f32), np.zeros(flat.numel(), f32))
    torch.cuda.synchronize()
    d = Drive(H, e, H.S, skew, first_params=flat)
    got = four(d, [H.S, None, H.S2, H.S])
    d.stream = H.S
    got_state = d.state()
    assert_same(got, want, "moved model results")
    assert_same(got_state, want_state, "moved model state")
    e.close()


@pytest.mark.parametrize("skew", SKEWS)
def test_two_engines_on_two_streams_interleaved_from_one_thread(skew, H):
    """P on S and Q on S2, calls interleaved (train, predict, train, different images), every call under the skew: each equals its own solo
    twin.  NULL late is the skew under which a launch or clear that one engine sends to the NULL stream lands after the other engine's work."""
    flat = params(1)[1]
    plan = dict(P=(71, 72, 73), Q=(81, 82, 83))

    def calls(d, seeds, k):
        if k == 0:
            return d.step(lambda e, i, l: e.train_step(i, l, 1e-3, keep_prob=0.5, fetch_loss=False), SHAPE_A, seeds[0], asynchronous=d.skew is not None)
        if k == 1:
            return d.step(lambda e, i, l: e.predict(i, argmax=False), SHAPE_B, seeds[1])
        return d.step(lambda e, i, l: e.train_step(i, l, 1e-3, keep_prob=0.5), SHAPE_A, seeds[2])
    want = {}
    for name, seeds in plan.items():
        twin = fresh("fp32")
        d = Drive(H, twin, first_params=flat)
        want[name] = ([calls(d, seeds, k) for k in range(3)], d.state())
        twin.close()
    engines, drives = {}, {}
    for name, s in (("P", H.S), ("Q", H.S2)):
        e = fresh("fp32", seed=2)
        with torch.cuda.stream(s):
            wi, wl = dev_batch(SHAPE_A, 79)
            e.train_step(wi, wl, 1e-4, keep_prob=1.0); e.predict(wi)
            e.global_step = 0; e.flat_grads.zero_()
            e.set_opt_state(np.zeros(flat.numel(), f32), np.zeros(flat.numel(), f32))
        engines[name], drives[name] = e, Drive(H, e, s, skew, first_params=flat)
        drives[name].prepare([(SHAPE_A, plan[name][0]), (SHAPE_B, plan[name][1]), (SHAPE_A, plan[name][2])])      # no synchronise between the calls
    torch.cuda.synchronize()
    got = dict(P=[], Q=[])
    for k in range(3):
        for name in ("P", "Q"):
            got[name].append(calls(drives[name], plan[name], k))
    for name in ("P", "Q"):
        assert_same(got[name], want[name][0], "engine %s results" % name)
        assert_same(drives[name].state(), want[name][1], "engine %s state" % name)
        engines[name].close()


def scratch_bytes_live():
    L = lib()
    v = C.c_int64()
    L.check(L.lib.fcn8s_get_option(None, b"scratch_bytes_live", C.byref(v)))
    return int(v.value)


def test_a_closed_engine_gives_back_the_scratch_of_every_stream_it_ran_on(H):
    streams = [H.S, H.S2, torch.cuda.Stream()]

    def visit():
        e = fresh("fp32")
        img, lab = dev_batch(SHAPE_A, 91)
        seen = []
        for s in streams:
            with torch.cuda.stream(s):
                e.train_step(img, lab, 1e-4, keep_prob=1.0)
            seen.append(scratch_bytes_live())
        return e, seen
    L = lib()
    assert L.lib.fcn8s_set_option(None, b"scratch_bytes_live", 0) == L.ERR_BAD_ARG               # read-only, as device_bytes_live is
    e, _ = visit(); e.close()                                        # whatever earlier tests left on these streams is released with it
    before = scratch_bytes_live()
    e, seen = visit()
    assert seen[0] > before and seen[1] > seen[0] and seen[2] > seen[1], (before, seen)          # each stream grew scratch of its own
    e.close()
    assert scratch_bytes_live() == before


def test_canary_detects_both_kinds_of_stray_launch_after_the_case_table(H):
    run_canary(H)
    print("\nstream module: %.1f s since the harness was made; longest measured call of a row or wrapper %.3f ms, longest delay queued %.1f ms"
          % (time.perf_counter() - H.t_start, H.longest_host_ms, H.longest_ms))
