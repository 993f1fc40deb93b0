"""The update's kernels on synthetic device buffers (csrc/optim.hip through the fcn8s_op_* entry points): fold / flush at every float
alignment, the global norm in its fixed order, and the optimizers that read their scale and the guard's verdict from the device.

Reference: NumPy float32 for the adds (one fp32 add per element), optim.py's float64 restatement for the norm and the clip, and the
library's own fcn8s_op_tf_adam / fcn8s_op_sgd_momentum for the optimizer steps (same expressions, host-given scale)."""
import ctypes as C

import numpy as np
import pytest

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

from fcn8s_tensorflow_amd import optim  # noqa: E402

SIZES = (1, 3, 4, 5, 255, 1023, 1025, 262147)
SENTINEL = np.float32(-12345.5)


def _lib():
    from fcn8s_tensorflow_amd import _lib
    return _lib


def ptr(t, off=0):
    return C.c_void_p(t.data_ptr() + 4 * off)


def ulps(a, b):
    """distance of two float32 in units in the last place of b"""
    a, b = np.float32(a), np.float32(b)
    return abs(float(a) - float(b)) / float(np.spacing(np.abs(b)))


@pytest.fixture(scope="module")
def values():
    """n -> float32 values spanning 1e-6 .. 1e3 in magnitude, both signs (made once, never written)"""
    rng = np.random.default_rng(11)
    out = {}
    for n in SIZES:
        v = (10.0 ** rng.uniform(-6, 3, n) * rng.choice([-1.0, 1.0], n)).astype(np.float32)
        v.setflags(write=False)
        out[n] = v
    return out


@pytest.mark.parametrize("n", SIZES)
def test_grad_accumulate_every_alignment_both_modes(n, values):
    """dst and src each start 0 .. 3 floats behind a 16-byte boundary (scalar head, float4 body, scalar tail; equal and unequal alignment of the two);
    == NumPy float32, and the eight floats on either side of the range keep their sentinel."""
    L = _lib()
    rng = np.random.default_rng(n)
    src = values[n]
    dst0 = rng.standard_normal(n).astype(np.float32)
    pad = 8
    for do in range(4):
        for so in range(4):
            for mode in (0, 1):
                hd = np.full(n + 2 * pad + 4, SENTINEL, np.float32); hd[pad + do:pad + do + n] = dst0
                hs = np.full(n + 2 * pad + 4, SENTINEL, np.float32); hs[pad + so:pad + so + n] = src
                d, s = torch.from_numpy(hd).cuda(), torch.from_numpy(hs).cuda()
                assert d.data_ptr() % 16 == 0 and s.data_ptr() % 16 == 0
                L.check(L.lib.fcn8s_op_grad_accumulate(None, ptr(d, pad + do), ptr(s, pad + so), n, mode))
                torch.cuda.synchronize()
                out = d.cpu().numpy()
                want = src if mode == 0 else (dst0 + src).astype(np.float32)
                assert np.array_equal(out[pad + do:pad + do + n], want), (n, do, so, mode)
                assert (out[:pad + do] == SENTINEL).all() and (out[pad + do + n:] == SENTINEL).all(), (n, do, so, mode)
                assert np.array_equal(s.cpu().numpy(), hs)


def test_grad_accumulate_refuses_bad_arguments():
    L = _lib()
    t = torch.zeros(8).cuda()
    assert L.lib.fcn8s_op_grad_accumulate(None, ptr(t), ptr(t), 4, 2) == L.ERR_BAD_ARG
    assert L.lib.fcn8s_op_grad_accumulate(None, None, ptr(t), 4, 0) == L.ERR_BAD_ARG
    assert L.lib.fcn8s_op_grad_accumulate(None, ptr(t), ptr(t), -1, 0) == L.ERR_BAD_ARG
    assert L.lib.fcn8s_op_grad_norm(None, ptr(t), 4, 1.0, -1.0, ptr(t)) == L.ERR_BAD_ARG
    assert L.lib.fcn8s_op_grad_norm(None, ptr(t), 4, 1.0, float("nan"), ptr(t)) == L.ERR_BAD_ARG


def run_norm(g_dev, n, gs, max_norm, off=0):
    L = _lib()
    out = torch.full((5,), 7.0).cuda()
    L.check(L.lib.fcn8s_op_grad_norm(None, ptr(g_dev, off), n, gs, max_norm, ptr(out)))
    torch.cuda.synchronize()
    return out.cpu().numpy()


@pytest.mark.parametrize("n", SIZES)
def test_grad_norm_against_float64_and_bit_reproducible(n, values):
    L = _lib()
    g = values[n]
    gd = torch.from_numpy(np.concatenate([np.zeros(4, np.float32), g])).cuda()           # g itself at float offsets 4 (aligned) and 1 .. 3 below
    for gs in (1.0, -0.25):
        want = optim.global_norm(g, gs)
        outs = []
        for det in (0, 1, 0):
            L.check(L.lib.fcn8s_set_option(None, b"op_deterministic", det))
            try:
                outs.append(run_norm(gd, n, gs, 0.0, off=4))
            finally:
                L.check(L.lib.fcn8s_set_option(None, b"op_deterministic", 0))
        assert outs[0].tobytes() == outs[1].tobytes() == outs[2].tobytes()                # no float atomics, whatever `deterministic` says
        norm, c, s, ok, zero = outs[0]
        print("n=%d gs=%g norm %r want %r: %.2f ulps" % (n, gs, norm, want, ulps(norm, want)))
        assert ulps(norm, want) <= 4
        assert c == 1.0 and s.tobytes() == np.float32(gs).tobytes() and ok == 1.0 and zero == 0.0        # clip off
        # the clip does not bite: s == gs bit for bit (max_norm = norm, above it, and inf)
        for mx in (float(norm), float(norm) * 2.0, float("inf")):
            o = run_norm(gd, n, gs, mx, off=4)
            assert o[0].tobytes() == norm.tobytes() and o[1] == 1.0 and o[2].tobytes() == np.float32(gs).tobytes() and o[3] == 1.0
        # it bites: c and s within 2 ulps of the float32 formula evaluated at the device's own norm
        for mx in (float(norm) * 0.5, float(norm) * 0.9999, 1e-7):
            o = run_norm(gd, n, gs, mx, off=4)
            cw, sw, okw = optim.clip_scale(o[0], gs, mx)
            assert okw and o[3] == 1.0 and o[1] < 1.0
            assert ulps(o[1], cw) <= 2 and ulps(o[2], sw) <= 2, (n, gs, mx, o, cw, sw)
    # a sub-range that starts 1 .. 3 floats behind a 16-byte boundary: the same value to the same bar
    for off in (1, 2, 3):
        sub = np.concatenate([np.zeros(4, np.float32), g])[off:off + n]
        o = run_norm(gd, n, 1.0, 0.0, off=off)
        assert ulps(o[0], optim.global_norm(sub, 1.0)) <= 4 or (o[0] == 0.0 and not sub.any())


@pytest.mark.parametrize("n", SIZES)
@pytest.mark.parametrize("bad", [float("nan"), float("inf")])
def test_grad_norm_guard_sees_one_bad_element_anywhere(n, bad, values):
    for where in sorted({0, n // 2, n - 1}):
        g = values[n].copy(); g[where] = bad
        for mx in (0.0, 1.0, float("inf")):
            o = run_norm(torch.from_numpy(g).cuda(), n, 0.5, mx)
            assert o[3] == 0.0 and not np.isfinite(o[0]), (n, bad, where, mx, o)


@pytest.mark.parametrize("n", (1025, 262147))
def test_device_scale_optimizers_equal_the_host_scale_ones(n, values):
    L = _lib()
    rng = np.random.default_rng(n + 1)
    g = values[n]
    th0 = rng.standard_normal(n).astype(np.float32)
    m0 = (rng.standard_normal(n) * 0.1).astype(np.float32)
    v0 = (rng.standard_normal(n) ** 2).astype(np.float32)
    gd = torch.from_numpy(g.copy()).cuda()
    norm = run_norm(gd, n, 0.5, 0.0)[0]
    slab = torch.full((5,), 7.0).cuda()
    L.check(L.lib.fcn8s_op_grad_norm(None, ptr(gd), n, 0.5, float(norm) * 0.37, ptr(slab)))      # a clip that bites: s is no round number
    s = float(slab.cpu().numpy()[2])
    assert slab.cpu().numpy()[3] == 1.0 and 0.0 < s < 0.5
    dev = lambda a: torch.from_numpy(a.copy()).cuda()
    # TF-Adam, step t = 3
    a = [dev(x) for x in (th0, m0, v0)]; b = [dev(x) for x in (th0, m0, v0)]
    L.check(L.lib.fcn8s_op_tf_adam_dev(None, ptr(a[0]), ptr(gd), ptr(a[1]), ptr(a[2]), n, 3, 1e-3, 0.9, 0.999, 1e-8, ptr(slab)))
    L.check(L.lib.fcn8s_op_tf_adam(None, ptr(b[0]), ptr(gd), ptr(b[1]), ptr(b[2]), n, 3, 1e-3, 0.9, 0.999, 1e-8, s))
    torch.cuda.synchronize()
    for x, y, z in zip(a, b, (th0, m0, v0)):
        assert np.array_equal(x.cpu().numpy(), y.cpu().numpy()) and not np.array_equal(x.cpu().numpy(), z)
    # SGD with momentum
    a = [dev(x) for x in (th0, m0)]; b = [dev(x) for x in (th0, m0)]
    L.check(L.lib.fcn8s_op_sgd_momentum_dev(None, ptr(a[0]), ptr(gd), ptr(a[1]), n, 1e-2, 0.9, ptr(slab)))
    L.check(L.lib.fcn8s_op_sgd_momentum(None, ptr(b[0]), ptr(gd), ptr(b[1]), n, 1e-2, 0.9, s))
    torch.cuda.synchronize()
    for x, y, z in zip(a, b, (th0, m0)):
        assert np.array_equal(x.cpu().numpy(), y.cpu().numpy()) and not np.array_equal(x.cpu().numpy(), z)
    # ok = 0: theta, m and v keep their bits
    gb = g.copy(); gb[n // 3] = np.nan
    gbd = torch.from_numpy(gb).cuda()
    L.check(L.lib.fcn8s_op_grad_norm(None, ptr(gbd), n, 0.5, 1.0, ptr(slab)))
    assert slab.cpu().numpy()[3] == 0.0
    a = [dev(x) for x in (th0, m0, v0)]
    L.check(L.lib.fcn8s_op_tf_adam_dev(None, ptr(a[0]), ptr(gbd), ptr(a[1]), ptr(a[2]), n, 3, 1e-3, 0.9, 0.999, 1e-8, ptr(slab)))
    L.check(L.lib.fcn8s_op_sgd_momentum_dev(None, ptr(a[0]), ptr(gbd), ptr(a[1]), n, 1e-2, 0.9, ptr(slab)))
    torch.cuda.synchronize()
    for x, z in zip(a, (th0, m0, v0)):
        assert x.cpu().numpy().tobytes() == z.tobytes()
