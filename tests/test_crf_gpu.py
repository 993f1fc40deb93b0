"""Mean-field CRF refinement on the GPU (fcn8s_op_crf_meanfield, fcn8s_predict_crf, Engine.predict_crf, FCN8s.predict(crf=)): the kernel
against the float64 restatement of the definition (crf.meanfield) with a tolerance taken from the restatement's own float32 rounding, the
argmax output, iterations = 0 / NULL parameters against fcn8s_predict_tta bit for bit, the composition with fcn8s_predict_tta bit for bit,
determinism, allocations, errors, the facade."""
import ctypes as C

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from oracle import fcn8s_oracle as orc  # noqa: E402  (checker only)
from fcn8s_tensorflow_amd import _lib as L, crf  # noqa: E402

SMALL = (8, 16, 32, 64, 64, 128, 128)
SMALL64 = (64, 64, 64, 64, 64, 128, 128)        # bf16_train: every width a multiple of 64


def dev(a):
    return torch.as_tensor(np.ascontiguousarray(a)).cuda()


def ptr(t):
    return C.c_void_p(t.data_ptr()) if t is not None else None


def engine(widths=SMALL, precision="fp32", seed=1):
    from fcn8s_tensorflow_amd.engine import Engine
    e = Engine(20, widths=widths, device_id=0, precision=precision)
    e.set_params(orc.init_params(20, widths, seed=seed, decoder_std_scale=30.0, bias_std=0.05))
    return e


def scenes(N, H, W, C_, seed=0):
    ps, imgs = zip(*[crf.synthetic_scene(H, W, C_, seed=seed + 101 * n)[:2] for n in range(N)])
    return np.stack(ps), np.stack(imgs)


def images(N, H, W, seed=0):
    return scenes(N, H, W, 20, seed)[1]


def struct(p):
    return L.CrfParams(**crf.validate(p).as_dict())


def op_meanfield(prob, img, params, want_q=True, want_am=True):
    """fcn8s_op_crf_meanfield on device copies of prob / img -> (Q^T or None, argmax or None) as NumPy arrays"""
    N, H, W, C_ = prob.shape
    cp = struct(params)
    dp, di = dev(prob), dev(img)
    nwork = L.lib.fcn8s_op_crf_work_floats(N, H, W, C_, C.byref(cp))
    assert nwork > 0 or cp.iterations == 0
    work = torch.empty(max(int(nwork), 4), dtype=torch.float32, device="cuda")
    q = torch.full((N, H, W, C_), -7.0, dtype=torch.float32, device="cuda") if want_q else None
    am = torch.full((N, H, W), -7, dtype=torch.int64, device="cuda") if want_am else None
    L.check(L.lib.fcn8s_op_crf_meanfield(None, ptr(dp), ptr(di), N, H, W, C_, C.byref(cp), ptr(work), ptr(q), ptr(am)))
    torch.cuda.synchronize()
    assert np.array_equal(dp.cpu().numpy().view(np.uint32), prob.view(np.uint32)), "prob was written"
    return (q.cpu().numpy() if want_q else None), (am.cpu().numpy() if want_am else None)


# ---- 1. the kernel against the float64 restatement ---------------------------------------------------------------------------------
KERNEL_CASES = [
    # N, H, W, C, r, d, T, w_appearance, w_smooth
    (1, 96, 128, 20, 3, 1, 5, 4.0, 2.0),
    (1, 61, 83, 20, 2, 3, 10, 4.0, 2.0),
    (1, 64, 64, 4, 5, 1, 5, 10.0, 3.0),
    (1, 96, 128, 20, 3, 2, 10, 10.0, 3.0),
    (2, 45, 51, 12, 1, 4, 1, 4.0, 2.0),           # the any-C form, N = 2, odd H and W
    (2, 37, 53, 20, 3, 1, 1, 4.0, 2.0),
    (2, 33, 47, 4, 3, 2, 5, 4.0, 2.0),
    (1, 70, 91, 20, 3, 8, 5, 4.0, 2.0),           # dilation 8
    (1, 75, 66, 12, 5, 3, 5, 6.0, 1.0),
    (1, 50, 67, 20, 7, 1, 5, 4.0, 2.0),           # radius 7: the largest LDS tile
    (1, 49, 40, 4, 7, 2, 10, 4.0, 2.0),
    (1, 40, 44, 12, 7, 4, 1, 4.0, 2.0),
    (1, 5, 7, 4, 3, 2, 2, 4.0, 2.0),              # smaller than the window
    (1, 5, 7, 20, 3, 2, 2, 4.0, 2.0),
    (1, 1, 1, 4, 1, 1, 3, 4.0, 2.0),              # no neighbour at all
    (2, 1, 9, 20, 1, 8, 3, 4.0, 2.0),             # only the two end pixels see each other
    (1, 512, 1024, 20, 3, 1, 5, 4.0, 2.0),        # a size a user would run, the defaults
]


@pytest.mark.parametrize("N,H,W,C_,r,d,T,wa,ws", KERNEL_CASES)
def test_kernel_matches_the_float64_restatement(N, H, W, C_, r, d, T, wa, ws):
    """Gate: max |device - float64| <= 8 * max(d32, 2^-23), d32 = max |meanfield(float32) - meanfield(float64)| on the same inputs (the
    rounding of the definition itself in the device's number format; 8x for another summation order over up to 224 taps, fused
    multiply-adds and the device's exp).  The argmax output equals the float64 argmax wherever the float64 top-2 margin exceeds 1e-4
    (at most 1 % of the pixels may fall below that margin)."""
    prob, img = scenes(N, H, W, C_, seed=H + W)
    p = crf.Params(iterations=T, radius=r, dilation=d, w_appearance=wa, w_smooth=ws)
    q, am = op_meanfield(prob, img, p)
    ref = crf.meanfield(prob, img, p, dtype=np.float64)
    d32 = float(np.abs(crf.meanfield(prob, img, p, dtype=np.float32).astype(np.float64) - ref).max())
    gate = 8.0 * max(d32, 2.0 ** -23)
    dist = float(np.abs(q.astype(np.float64) - ref).max())
    srt = np.sort(ref, -1)
    safe = (srt[..., -1] - srt[..., -2]) > 1e-4
    changed = float((ref.argmax(-1) != prob.argmax(-1)).mean())
    print("crf case N=%d %dx%dx%d r=%d d=%d T=%d: device distance %.3e, d32 %.3e, gate %.3e, low-margin share %.5f, argmax changed by the CRF %.3f"
          % (N, H, W, C_, r, d, T, dist, d32, gate, 1 - safe.mean(), changed))
    assert dist <= gate, (dist, d32, gate)
    assert 1 - safe.mean() <= 0.01
    assert (am[safe] == ref.argmax(-1)[safe]).all()
    assert np.array_equal(am, q.argmax(-1))                         # the argmax output is the argmax of the Q^T that was written
    if min(H, W) >= 32:
        assert changed > 0.05                                        # (a kernel that does nothing cannot pass)


def test_outputs_are_optional_and_runs_are_identical():
    prob, img = scenes(2, 41, 59, 20, seed=3)
    p = crf.Params(iterations=4, dilation=2)
    q, am = op_meanfield(prob, img, p)
    q2, _ = op_meanfield(prob, img, p, want_am=False)
    _, am2 = op_meanfield(prob, img, p, want_q=False)
    assert np.array_equal(q.view(np.uint32), q2.view(np.uint32)) and np.array_equal(am, am2)
    # iterations = 0: P untouched, bit for bit, and its own argmax
    q0, am0 = op_meanfield(prob, img, crf.Params(iterations=0))
    assert np.array_equal(q0.view(np.uint32), prob.view(np.uint32)) and np.array_equal(am0, prob.argmax(-1))


# ---- 2. fcn8s_predict_crf ------------------------------------------------------------------------------------------------------------
def raw_predict(e, fn, img, scales, flip, argmax, cp=None, where=L.HOST):
    N, H, W = img.shape[:3]
    arr = (C.c_float * len(scales))(*scales)
    shape, dt = ((N, H, W), torch.int64) if argmax else ((N, H, W, 20), torch.float32)
    extra = (C.byref(cp) if cp is not None else None,) if fn == "crf" else ()
    f = L.lib.fcn8s_predict_crf if fn == "crf" else L.lib.fcn8s_predict_tta
    if where == L.HOST:
        out = np.empty(shape, np.int64 if argmax else np.float32)
        src = np.ascontiguousarray(img)
        L.check(f(e.h, src.ctypes.data_as(C.c_void_p), L.IMG_U8, N, H, W, arr, len(scales), int(flip), *extra, int(argmax),
                  out.ctypes.data_as(C.c_void_p), where), e.h)
        return out
    out = torch.empty(shape, dtype=dt, device="cuda")
    src = dev(img)
    L.check(f(e.h, ptr(src), L.IMG_U8, N, H, W, arr, len(scales), int(flip), *extra, int(argmax), ptr(out), where), e.h)
    torch.cuda.synchronize()
    return out.cpu().numpy()


@pytest.mark.parametrize("scales,flip", [((1.0,), False), ((0.75, 1.25), True)])
def test_zero_iterations_and_null_params_are_predict_tta_bit_for_bit(scales, flip):
    e = engine()
    img = images(2, 50, 70, seed=5)
    for argmax in (False, True):
        want = raw_predict(e, "tta", img, scales, flip, argmax)
        for cp in (None, struct(crf.Params(iterations=0))):
            got = raw_predict(e, "crf", img, scales, flip, argmax, cp)
            assert np.array_equal(got.view(np.uint32 if not argmax else np.int64), want.view(np.uint32 if not argmax else np.int64))
    # the identity case that fcn8s_predict_tta hands to fcn8s_predict
    img = images(1, 64, 96, seed=6)
    assert np.array_equal(raw_predict(e, "crf", img, (1.0,), False, True, None), e.predict(img))
    e.close()


@pytest.mark.parametrize("where", [L.HOST, L.DEVICE])
@pytest.mark.parametrize("widths,precision", [(SMALL, "fp32"), (SMALL64, "bf16_train")])
def test_predict_crf_is_meanfield_of_predict_tta_bit_for_bit(widths, precision, where):
    e = engine(widths, precision)
    p = crf.Params(iterations=3, radius=2, dilation=2, w_appearance=6.0)
    for (N, H, W, scales, flip) in [(2, 50, 70, (0.75, 1.25), True), (1, 45, 67, (1.0,), False), (1, 64, 96, (1.0,), False)]:
        img = images(N, H, W, seed=H)
        sm = raw_predict(e, "tta", img, scales, flip, False, where=where)
        want_q, want_am = op_meanfield(sm, img, p)
        got_q = raw_predict(e, "crf", img, scales, flip, False, struct(p), where=where)
        got_am = raw_predict(e, "crf", img, scales, flip, True, struct(p), where=where)
        assert np.array_equal(got_q.view(np.uint32), want_q.view(np.uint32))
        assert np.array_equal(got_am, want_am)
    e.close()


def test_repeat_call_is_identical_and_allocates_nothing():
    e = engine()
    img = images(2, 50, 70, seed=11)
    p = dict(iterations=4, radius=3)
    for kw in (dict(scales=(0.75, 1.0), flip=True), dict(scales=(1.0,), flip=False)):
        for argmax in (False, True):
            a = e.predict_crf(img, p, argmax=argmax, **kw)
            n1 = e.get_option("workspace_allocations")
            b = e.predict_crf(img, p, argmax=argmax, **kw)
            assert e.get_option("workspace_allocations") == n1
            assert np.array_equal(a, b) and a.tobytes() == b.tobytes()
    d = e.predict_crf(dev(img), p, scales=(1.0,), argmax=False)
    assert d.is_cuda and np.array_equal(d.cpu().numpy(), e.predict_crf(img, p, scales=(1.0,), argmax=False))
    e.close()


def test_profile_group():
    e = engine()
    img = images(1, 48, 64, seed=2)
    e.profile(True); e.profile_reset()
    e.predict_crf(img, dict(iterations=3))
    prof = e.profile_results()
    e.profile(False)
    g = prof["crf_meanfield"]
    assert g["launches"] == 3
    assert g["bytes"] == 3 * 48 * 64 * (12 * 20 + 3) + 8 * 48 * 64          # read Q, read P, write Q, read I; the argmax with the last update
    e.close()


# ---- 3. errors --------------------------------------------------------------------------------------------------------------------------
BAD = [("iterations", -1), ("iterations", 33), ("radius", 0), ("radius", 8), ("dilation", 0), ("dilation", 9),
       ("w_appearance", -0.5), ("w_appearance", float("nan")), ("w_appearance", float("inf")),
       ("w_smooth", -0.5), ("w_smooth", float("nan")), ("w_smooth", float("inf")),
       ("theta_alpha", 0.0), ("theta_alpha", float("nan")), ("theta_alpha", float("inf")),
       ("theta_beta", 0.0), ("theta_beta", -3.0), ("theta_beta", float("nan")), ("theta_beta", float("inf")),
       ("theta_gamma", 0.0), ("theta_gamma", float("nan")), ("theta_gamma", float("inf"))]


def test_bad_arguments():
    e = engine()
    img = images(1, 48, 64)
    prob, _ = scenes(1, 48, 64, 20)
    dp, di = dev(prob), dev(img)
    work = torch.empty(2 * prob.size, dtype=torch.float32, device="cuda")
    q = torch.zeros(prob.shape, dtype=torch.float32, device="cuda")
    arr = (C.c_float * 1)(1.0)
    out = np.full((1, 48, 64), -1, np.int64)
    for field, value in BAD:
        cp = L.CrfParams(**crf.Params().as_dict())
        setattr(cp, field, value)
        rc = L.lib.fcn8s_predict_crf(e.h, img.ctypes.data_as(C.c_void_p), L.IMG_U8, 1, 48, 64, arr, 1, 0, C.byref(cp), 1, out.ctypes.data_as(C.c_void_p), L.HOST)
        assert rc == L.ERR_BAD_ARG and field.encode() in L.lib.fcn8s_last_error(e.h), (field, value)
        rc = L.lib.fcn8s_op_crf_meanfield(None, ptr(dp), ptr(di), 1, 48, 64, 20, C.byref(cp), ptr(work), ptr(q), None)
        assert rc == L.ERR_BAD_ARG and field.encode() in L.lib.fcn8s_last_error(None), (field, value)
        assert L.lib.fcn8s_op_crf_work_floats(1, 48, 64, 20, C.byref(cp)) == 0
        for call in (lambda: e.predict_crf(img, {field: value}), lambda: e.predict_crf(img, crf.Params(**{field: value}))):
            with pytest.raises(ValueError, match=field):
                call()
    torch.cuda.synchronize()
    assert (out == -1).all() and float(q.abs().max()) == 0.0                 # nothing was launched
    # float32 images: refused with iterations > 0, taken (as fcn8s_predict_tta takes them) with iterations = 0
    f32 = np.ascontiguousarray(img, np.float32)
    cp = struct(crf.Params())
    rc = L.lib.fcn8s_predict_crf(e.h, f32.ctypes.data_as(C.c_void_p), L.IMG_F32, 1, 48, 64, arr, 1, 0, C.byref(cp), 1, out.ctypes.data_as(C.c_void_p), L.HOST)
    assert rc == L.ERR_BAD_ARG and b"float32" in L.lib.fcn8s_last_error(e.h)
    with pytest.raises(ValueError, match="float32"):
        e.predict_crf(f32, True)
    assert np.array_equal(e.predict_crf(f32, dict(iterations=0), flip=True), e.predict_tta(f32, flip=True))
    # whatever fcn8s_predict_tta refuses
    with pytest.raises(ValueError):
        e.predict_crf(img, True, scales=(0.0,))
    with pytest.raises(ValueError):
        e.predict_crf(img, 3)
    e.close()


# ---- 4. the facade ----------------------------------------------------------------------------------------------------------------------
def _facade():
    from fcn8s_tensorflow_amd.fcn8s import FCN8s
    return FCN8s(vgg16_dir='synthetic:3', num_classes=20, widths=SMALL)


def test_facade(tmp_path):
    from PIL import Image
    from fcn8s_tensorflow_amd import cityscapes_eval as ce
    m = _facade()
    img = images(2, 64, 96, seed=17)
    # crf=None / False: today's predict, bit for bit
    for argmax in (True, False):
        want = m.engine.predict(img, argmax=argmax)
        assert np.array_equal(m.predict(img, argmax=argmax, crf=None), want) and np.array_equal(m.predict(img, argmax=argmax, crf=False), want)
        assert np.array_equal(m.predict(img, argmax=argmax, crf=True), m.engine.predict_crf(img, crf.Params(), argmax=argmax))
    assert np.array_equal(m.predict(img, crf=dict(radius=5, dilation=2)), m.engine.predict_crf(img, crf.Params(radius=5, dilation=2)))
    odd = images(1, 45, 77, seed=18)
    assert np.array_equal(m.predict(odd, scales=(0.75, 1.0), flip=True, crf=True),
                          m.engine.predict_crf(odd, True, scales=(0.75, 1.0), flip=True))
    assert m.predict(odd, crf=True).shape == (1, 45, 77)          # any size, as with scales=(1.0,)
    with pytest.raises(ValueError, match="radius"):
        m.predict(img, crf=dict(radius=9))
    with pytest.raises(ValueError, match="theta_beta"):
        m.predict(img, crf=dict(theta_beta=float("nan")))
    src = tmp_path / "leftImg8bit" / "city"
    src.mkdir(parents=True)
    files = {"a_leftImg8bit.png": images(1, 45, 77, seed=1)[0], "b_leftImg8bit.png": images(1, 64, 50, seed=2)[0]}
    for name, a in files.items():
        Image.fromarray(a).save(str(src / name))
    n = m.predict_and_export_label_ids(str(tmp_path / "results"), str(tmp_path / "leftImg8bit"), crf=True)
    assert n == 2
    for name, a in files.items():
        got = np.asarray(Image.open(str(tmp_path / "results" / name)))
        want = ce.TRAINIDS_TO_IDS_ARRAY[m.engine.predict_crf(a[None], crf.Params(), argmax=True)[0]]
        assert np.array_equal(got, want)
    m.predict_and_save(str(tmp_path / "out"), str(src), {c: (0, 255, 0, 127) for c in range(20)}, crf=dict(iterations=2))
    assert sorted(p.name for p in (tmp_path / "out").iterdir()) == sorted(files)
