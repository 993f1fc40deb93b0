"""The parameter average's kernels on synthetic device buffers (csrc/optim.hip through the fcn8s_op_* entry points): the average alone,
the updates fused with it, and the swap -- at every float alignment of every pointer, with sizes that exercise the scalar head, the
float4 body and the scalar tail.

References: optim.ema_step in float64 fed the same fp32 inputs and the same fp32 weight; the library's own fcn8s_op_tf_adam /
fcn8s_op_sgd_momentum (and their _dev forms) for theta and the slots, held to tests/golden/update_bits.npz -- the bits of the kernels the
one update kernel replaced (tests/golden/make_update_bits.py); fcn8s_op_ema_update on the resulting theta for the shadow."""
import ctypes as C
import hashlib
import os

import numpy as np
import pytest

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

from fcn8s_tensorflow_amd import optim  # noqa: E402

SIZES = (1, 3, 4, 5, 255, 1023, 1025, 262147)
# 2048 * 256 * 4 + 1029: more float4 than 2048 blocks of 256 lanes hold -- a lane of a grid capped there takes a second one -- with a non-empty
# tail (n mod 4 = 1).
# The update's golden test only, at two placements.
BIG = 2098181
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "update_bits.npz")
SENTINEL = np.float32(-12345.5)
PAD = 8
OMEGAS = (np.float32(9.0 / 11.0), np.float32(1.0 - 0.999))          # warm-up's first step, and the steady state of decay 0.999


def _lib():
    from fcn8s_tensorflow_amd import _lib
    return _lib


def ptr(t, off=0):
    return C.c_void_p(t.data_ptr() + 4 * off)


def placed(a, off):
    """a on the device, `off` floats behind a 16-byte boundary, sentinels on either side -> (tensor, float offset of a[0])"""
    h = np.full(a.size + 2 * PAD + 4, SENTINEL, np.float32)
    h[PAD + off:PAD + off + a.size] = a
    t = torch.from_numpy(h).cuda()
    assert t.data_ptr() % 16 == 0
    return t, PAD + off


def taken(t, at, n):
    """the n floats at `at`, after checking that nothing outside them was written"""
    out = t.cpu().numpy()
    assert (out[:at] == SENTINEL).all() and (out[at + n:] == SENTINEL).all()
    return out[at:at + n].copy()


def slab(scale, ok):
    """what fcn8s_op_grad_norm leaves: {norm, c, s, ok, 0}"""
    return torch.tensor([1.0, 1.0, float(scale), 1.0 if ok else 0.0, 0.0], dtype=torch.float32).cuda()


def make_inputs(sizes=SIZES + (BIG,)):
    """n -> dict of float32 arrays (never written): theta and shadow spanning 1e-6 .. 1e3 in magnitude with both signs, gradient, slots.
    One seeded stream in the order of `sizes`: a new size goes to the end.  (tests/golden/make_update_bits.py feeds these to the parent's kernels.)"""
    rng = np.random.default_rng(23)
    out = {}
    for n in sizes:
        mag = lambda: (10.0 ** rng.uniform(-6, 3, n) * rng.choice([-1.0, 1.0], n)).astype(np.float32)
        d = dict(theta=mag(), shadow=mag(), g=mag(), m=(rng.standard_normal(n) * 0.1).astype(np.float32),
                 v=(rng.standard_normal(n) ** 2).astype(np.float32))
        d["shadow"][::3] = d["theta"][::3] * np.float32(1.0 + 1e-4)          # a shadow close to theta too: the subtraction cancels
        for a in d.values():
            a.setflags(write=False)
        out[n] = d
    return out


@pytest.fixture(scope="module")
def data():
    return make_inputs()


@pytest.fixture(scope="module")
def golden():
    with np.load(GOLDEN) as z:
        return {k: z[k] for k in z.files}


def assert_golden(golden, opt, n, arrays, tag):
    """arrays (theta, m, v) == the recorded bits of the replaced kernels: raw arrays at the small sizes, SHA-256 digests at the two large ones"""
    for key, a in zip(("theta", "m", "v") if opt == "adam" else ("theta", "m"), arrays):
        raw, dig = "%s_%s_%d" % (opt, key, n), "%s_%s_sha256_%d" % (opt, key, n)
        if raw in golden:
            assert a.tobytes() == golden[raw].tobytes(), (tag, key, np.flatnonzero(a.view(np.uint32) != golden[raw].view(np.uint32))[:8])
        else:
            assert hashlib.sha256(a.tobytes()).hexdigest() == str(golden[dig]), (tag, key)


@pytest.mark.parametrize("n", SIZES)
def test_ema_update_against_float64(n, data):
    """|dev - f64| <= 4 * 2^-23 * max(|s_i|, |theta_i|) elementwise: at most three fp32 roundings (the subtraction, and the product and the
    sum -- one rounding where they are fused), each at most 2^-24 of a magnitude <= 2 M, plus headroom for either form."""
    L = _lib()
    s0, th = data[n]["shadow"], data[n]["theta"]
    bound = 4.0 * 2.0 ** -23 * np.maximum(np.abs(s0), np.abs(th)).astype(np.float64)
    worst = 0.0
    for w in OMEGAS:
        want = optim.ema_step(s0, th, w)
        for so in range(4):
            for to in range(4):
                s, sa = placed(s0, so); t, ta = placed(th, to)
                L.check(L.lib.fcn8s_op_ema_update(None, ptr(s, sa), ptr(t, ta), n, float(w), None))
                torch.cuda.synchronize()
                got = taken(s, sa, n)
                assert np.array_equal(taken(t, ta, n), th)
                err = np.abs(got.astype(np.float64) - want)
                worst = max(worst, float((err / np.maximum(bound, 1e-300)).max()))
                assert (err <= bound).all(), (n, so, to, float(w), float((err / bound).max()))
    print("n=%d: worst error %.3f of the bound" % (n, worst))
    # the guard said no: no bit of s changes; it said yes: the bits of the call without a slab
    s, sa = placed(s0, 1); t, ta = placed(th, 2)
    L.check(L.lib.fcn8s_op_ema_update(None, ptr(s, sa), ptr(t, ta), n, float(OMEGAS[0]), ptr(slab(0.5, False))))
    torch.cuda.synchronize()
    assert taken(s, sa, n).tobytes() == s0.tobytes()
    L.check(L.lib.fcn8s_op_ema_update(None, ptr(s, sa), ptr(t, ta), n, float(OMEGAS[0]), ptr(slab(0.5, True))))
    r, ra = placed(s0, 0)
    L.check(L.lib.fcn8s_op_ema_update(None, ptr(r, ra), ptr(t, ta), n, float(OMEGAS[0]), None))
    torch.cuda.synchronize()
    assert taken(s, sa, n).tobytes() == taken(r, ra, n).tobytes() != s0.tobytes()


def _reference_update(L, opt, d, n, gs, use_slab):
    """theta, slots after the library's own update on aligned copies; then the shadow by fcn8s_op_ema_update of the new theta"""
    dev = lambda a: torch.from_numpy(a.copy()).cuda()
    th, g, m, v = dev(d["theta"]), dev(d["g"]), dev(d["m"]), dev(d["v"])
    sl = slab(gs, True)
    if opt == "adam":
        if use_slab:
            L.check(L.lib.fcn8s_op_tf_adam_dev(None, ptr(th), ptr(g), ptr(m), ptr(v), n, 3, 1e-3, 0.9, 0.999, 1e-8, ptr(sl)))
        else:
            L.check(L.lib.fcn8s_op_tf_adam(None, ptr(th), ptr(g), ptr(m), ptr(v), n, 3, 1e-3, 0.9, 0.999, 1e-8, gs))
    else:
        if use_slab:
            L.check(L.lib.fcn8s_op_sgd_momentum_dev(None, ptr(th), ptr(g), ptr(m), n, 1e-2, 0.9, ptr(sl)))
        else:
            L.check(L.lib.fcn8s_op_sgd_momentum(None, ptr(th), ptr(g), ptr(m), n, 1e-2, 0.9, gs))
    torch.cuda.synchronize()
    return th.cpu().numpy(), m.cpu().numpy(), v.cpu().numpy(), th


@pytest.mark.parametrize("n", SIZES + (BIG,))
@pytest.mark.parametrize("opt", ["adam", "sgd"])
def test_fused_update_equals_update_then_average(opt, n, data, golden):
    L = _lib()
    d = data[n]
    gs = 0.37
    w = OMEGAS[0]
    # every pointer at its own alignment (o = 0: all aligned, the model's case), and all at the same odd one
    placements = [tuple((o + k) % 4 for k in (0, 1, 2, 0, 3)) for o in range(4)] + [(0, 0, 0, 0, 0), (1, 1, 1, 1, 1), (3, 3, 3, 3, 3)]
    if n == BIG:
        placements = [(0, 0, 0, 0, 0), (1, 1, 1, 1, 1)]
    for use_slab in (False, True):
        th_ref, m_ref, v_ref, th_dev = _reference_update(L, opt, d, n, gs, use_slab)
        assert not np.array_equal(th_ref, d["theta"])
        assert_golden(golden, opt, n, (th_ref, m_ref, v_ref), (opt, n, use_slab))
        s_ref = torch.from_numpy(d["shadow"].copy()).cuda()
        L.check(L.lib.fcn8s_op_ema_update(None, ptr(s_ref), ptr(th_dev), n, float(w), None))
        torch.cuda.synchronize()
        s_ref = s_ref.cpu().numpy()
        for offs in placements:
            sl = slab(gs, True) if use_slab else None
            slp = ptr(sl) if use_slab else None
            gsa = 123.0 if use_slab else gs                            # (with a slab the host scale is ignored)
            for fused in (True, False):                                # with the average, and the plain / _dev form
                th, ta = placed(d["theta"], offs[0]); g, ga = placed(d["g"], offs[1]); m, ma = placed(d["m"], offs[2])
                v, va = placed(d["v"], offs[3]); s, sa = placed(d["shadow"], offs[4])
                a4 = (ptr(th, ta), ptr(g, ga), ptr(m, ma), ptr(v, va))
                if opt == "adam" and fused:
                    L.check(L.lib.fcn8s_op_tf_adam_ema(None, *a4, ptr(s, sa), n, 3, 1e-3, 0.9, 0.999, 1e-8, gsa, slp, float(w)))
                elif opt == "adam" and use_slab:
                    L.check(L.lib.fcn8s_op_tf_adam_dev(None, *a4, n, 3, 1e-3, 0.9, 0.999, 1e-8, slp))
                elif opt == "adam":
                    L.check(L.lib.fcn8s_op_tf_adam(None, *a4, n, 3, 1e-3, 0.9, 0.999, 1e-8, gs))
                elif fused:
                    L.check(L.lib.fcn8s_op_sgd_momentum_ema(None, *a4[:3], ptr(s, sa), n, 1e-2, 0.9, gsa, slp, float(w)))
                elif use_slab:
                    L.check(L.lib.fcn8s_op_sgd_momentum_dev(None, *a4[:3], n, 1e-2, 0.9, slp))
                else:
                    L.check(L.lib.fcn8s_op_sgd_momentum(None, *a4[:3], n, 1e-2, 0.9, gs))
                torch.cuda.synchronize()
                tag = (opt, n, use_slab, offs, fused)
                assert taken(th, ta, n).tobytes() == th_ref.tobytes(), tag
                assert taken(m, ma, n).tobytes() == m_ref.tobytes(), tag
                assert taken(v, va, n).tobytes() == (v_ref if opt == "adam" else d["v"]).tobytes(), tag
                assert taken(s, sa, n).tobytes() == (s_ref if fused else d["shadow"]).tobytes(), tag
                assert np.array_equal(taken(g, ga, n), d["g"])
    # ok = 0: nothing changes
    th, ta = placed(d["theta"], 1); g, ga = placed(d["g"], 2); m, ma = placed(d["m"], 3); v, va = placed(d["v"], 0); s, sa = placed(d["shadow"], 1)
    sl = slab(gs, False)
    if opt == "adam":
        L.check(L.lib.fcn8s_op_tf_adam_ema(None, ptr(th, ta), ptr(g, ga), ptr(m, ma), ptr(v, va), ptr(s, sa), n, 3, 1e-3, 0.9, 0.999, 1e-8, gs, ptr(sl), float(w)))
    else:
        L.check(L.lib.fcn8s_op_sgd_momentum_ema(None, ptr(th, ta), ptr(g, ga), ptr(m, ma), ptr(s, sa), n, 1e-2, 0.9, gs, ptr(sl), float(w)))
    torch.cuda.synchronize()
    for t, at, key in ((th, ta, "theta"), (m, ma, "m"), (v, va, "v"), (s, sa, "shadow")):
        assert taken(t, at, n).tobytes() == d[key].tobytes(), (opt, n, key)


@pytest.mark.parametrize("n", SIZES)
def test_swap_exchanges_bits_and_twice_is_identity(n, data):
    L = _lib()
    a0, b0 = data[n]["theta"], data[n]["shadow"]
    for ao in range(4):
        for bo in range(4):
            a, aa = placed(a0, ao); b, ba = placed(b0, bo)
            L.check(L.lib.fcn8s_op_swap(None, ptr(a, aa), ptr(b, ba), n))
            torch.cuda.synchronize()
            assert taken(a, aa, n).tobytes() == b0.tobytes() and taken(b, ba, n).tobytes() == a0.tobytes(), (n, ao, bo)
            L.check(L.lib.fcn8s_op_swap(None, ptr(a, aa), ptr(b, ba), n))
            torch.cuda.synchronize()
            assert taken(a, aa, n).tobytes() == a0.tobytes() and taken(b, ba, n).tobytes() == b0.tobytes(), (n, ao, bo)


def test_ops_refuse_bad_arguments():
    L = _lib()
    t = torch.zeros(8).cuda()
    assert L.lib.fcn8s_op_swap(None, None, ptr(t), 4) == L.ERR_BAD_ARG
    assert L.lib.fcn8s_op_swap(None, ptr(t), None, 4) == L.ERR_BAD_ARG
    assert L.lib.fcn8s_op_swap(None, ptr(t), ptr(t, 4), -1) == L.ERR_BAD_ARG
    assert L.lib.fcn8s_op_ema_update(None, None, ptr(t), 4, 0.1, None) == L.ERR_BAD_ARG
    assert L.lib.fcn8s_op_ema_update(None, ptr(t), ptr(t, 4), -1, 0.1, None) == L.ERR_BAD_ARG
    assert L.lib.fcn8s_op_tf_adam_ema(None, ptr(t), ptr(t), ptr(t), ptr(t), None, 4, 1, 1e-3, 0.9, 0.999, 1e-8, 1.0, None, 0.1) == L.ERR_BAD_ARG
    assert L.lib.fcn8s_op_sgd_momentum_ema(None, ptr(t), ptr(t), ptr(t), None, 4, 1e-2, 0.9, 1.0, None, 0.1) == L.ERR_BAD_ARG
    L.check(L.lib.fcn8s_op_swap(None, ptr(t), ptr(t, 4), 0))            # n = 0: nothing to do
    torch.cuda.synchronize()
    assert not t.cpu().numpy().any()
