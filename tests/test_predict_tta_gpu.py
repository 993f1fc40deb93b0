"""Multi-scale / flip prediction on images of any size (fcn8s_predict_tta, Engine.predict_tta, FCN8s.predict(scales=, flip=)):
the two kernels against their host restatements, the identity case bit for bit against predict, arbitrary sizes against predict on the
mean-padded image, the full composition against per-pass predict + host interpolation, determinism, allocations, the facade."""
import ctypes as C

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from oracle import fcn8s_oracle as orc  # noqa: E402  (checker only)
from fcn8s_tensorflow_amd import _lib as L, cv2_compat, tta  # noqa: E402

SMALL = (8, 16, 32, 64, 64, 128, 128)
SMALL64 = (64, 64, 64, 64, 64, 128, 128)        # bf16_train: every width a multiple of 64
MEAN_RGB = (123.68, 116.779, 103.939)


def dev(a):
    return torch.as_tensor(np.ascontiguousarray(a)).cuda()


def ptr(t):
    return C.c_void_p(t.data_ptr()) if t is not None else None


def engine(widths=SMALL, precision="fp32", seed=1):
    from fcn8s_tensorflow_amd.engine import Engine
    e = Engine(20, widths=widths, device_id=0, precision=precision)
    e.set_params(orc.init_params(20, widths, seed=seed, decoder_std_scale=30.0, bias_std=0.05))
    return e


def images(n, h, w, seed=0):
    return np.random.default_rng(seed).integers(0, 256, (n, h, w, 3), dtype=np.uint8)


def check_probs(got, ref, atol, margin=1e-5):
    """probabilities within atol; argmax of the mean equal wherever the reference's top-2 margin exceeds `margin`"""
    got = np.asarray(got, np.float64); ref = np.asarray(ref, np.float64)
    assert got.shape == ref.shape
    err = np.abs(got - ref).max()
    assert err <= atol, err
    srt = np.sort(ref, -1)
    safe = (srt[..., -1] - srt[..., -2]) > margin
    assert (np.argmax(got, -1)[safe] == np.argmax(ref, -1)[safe]).all()
    return safe


def check_argmax(am, ref, margin=1e-5):
    srt = np.sort(ref, -1)
    safe = (srt[..., -1] - srt[..., -2]) > margin
    assert (np.asarray(am)[safe] == np.argmax(ref, -1)[safe]).all()


# ---- 1. tta_input ------------------------------------------------------------------------------------------------------------
INPUT_CASES = [
    # N, H, W, Hs, Ws, flip
    (1, 37, 53, 20, 29, 0),          # shrink
    (2, 37, 53, 60, 81, 1),          # enlarge, N = 2
    (1, 64, 96, 32, 48, 1),          # the exact 2x shrink (box mean)
    (2, 33, 45, 33, 45, 0),          # identity, odd H and W
    (1, 50, 70, 50, 70, 1),          # identity + mirror
    (1, 41, 27, 31, 20, 0),
]


@pytest.mark.parametrize("N,H,W,Hs,Ws,flip", INPUT_CASES)
def test_tta_input_is_resize_flip_preprocess_pad(N, H, W, Hs, Ws, flip):
    img = images(N, H, W, seed=H * W)
    Hp, Wp = -(-Hs // 32) * 32, -(-Ws // 32) * 32
    out = torch.full((N, Hp, Wp, 4), 7.0, dtype=torch.float32, device="cuda")
    L.check(L.lib.fcn8s_op_tta_input(None, ptr(dev(img)), N, H, W, Hs, Ws, Hp, Wp, flip, ptr(out)))
    torch.cuda.synchronize()
    ref = np.zeros((N, Hp, Wp, 4), np.float32)
    for n in range(N):
        r = cv2_compat.resize_linear(img[n], Hs, Ws)
        if flip:
            r = r[:, ::-1]
        r = dev(np.ascontiguousarray(r))
        pre = torch.empty((Hs, Ws, 4), dtype=torch.float32, device="cuda")
        L.check(L.lib.fcn8s_op_preprocess(None, ptr(r), L.IMG_U8, ptr(pre), Hs * Ws))
        torch.cuda.synchronize()
        ref[n, :Hs, :Ws] = pre.cpu().numpy()
    got = out.cpu().numpy()
    assert np.array_equal(got.view(np.uint32), ref.view(np.uint32))


# ---- 2. tta_accumulate -------------------------------------------------------------------------------------------------------
def torch_reference(pass_logits, flips, H, W):
    acc = None
    for lg, f in zip(pass_logits, flips):
        t = torch.from_numpy(np.asarray(lg, np.float64)).permute(0, 3, 1, 2)
        if f:
            t = torch.flip(t, dims=[3])
        p = torch.softmax(torch.nn.functional.interpolate(t, size=(H, W), mode="bilinear", align_corners=False), dim=1)
        acc = p if acc is None else acc + p
    return (acc / len(pass_logits)).permute(0, 2, 3, 1).numpy()


ACC_CASES = [
    # C, (Hs, Ws), (H, W), P
    (20, (24, 40), (37, 61), 6),       # upsampling
    (20, (40, 64), (25, 33), 2),       # downsampling
    (20, (30, 50), (30, 50), 1),       # identity
    (4, (17, 23), (40, 31), 6),
    (4, (32, 32), (32, 32), 2),
    (12, (19, 29), (27, 21), 6),
    (12, (9, 13), (9, 13), 1),
]


@pytest.mark.parametrize("C_,hw_s,hw,P", ACC_CASES)
def test_tta_accumulate_matches_interpolate_softmax_mean(C_, hw_s, hw, P):
    rng = np.random.default_rng(C_ * 100 + P)
    N, (Hs, Ws), (H, W) = 2, hw_s, hw
    Hp, Wp = -(-Hs // 32) * 32, -(-Ws // 32) * 32
    acc = torch.empty((N, H, W, C_), dtype=torch.float32, device="cuda")
    sm = torch.empty((N, H, W, C_), dtype=torch.float32, device="cuda")
    am = torch.empty((N, H, W), dtype=torch.int64, device="cuda")
    lgs, flips = [], []
    for k in range(P):
        full = rng.normal(0, 4, (N, Hp, Wp, C_)).astype(np.float32)
        full[:, Hs:] = 1e6; full[:, :, Ws:] = 1e6                  # padding region: never read
        f = k % 2
        d = dev(full)
        L.check(L.lib.fcn8s_op_tta_accumulate(None, ptr(d), N, Hp, Wp, Hs, Ws, f, C_, H, W, ptr(acc), int(k == 0), int(k == P - 1), P,
                                              ptr(sm), ptr(am)))
        torch.cuda.synchronize()
        lgs.append(full[:, :Hs, :Ws]); flips.append(bool(f))
    ref = torch_reference(lgs, flips, H, W)
    check_probs(sm.cpu().numpy(), ref, 1e-6)
    check_argmax(am.cpu().numpy(), ref)
    np.testing.assert_allclose(tta.compose(lgs, flips, H, W), ref, rtol=0, atol=1e-12)


# ---- 3. identity case: bit for bit fcn8s_predict --------------------------------------------------------------------------------
@pytest.mark.parametrize("N,H,W", [(2, 64, 96), (1, 512, 1024)])
def test_identity_case_is_predict_bit_for_bit(N, H, W):
    e = engine()
    img = images(N, H, W, seed=3)
    for argmax in (True, False):
        a = e.predict(img, argmax=argmax)
        b = e.predict_tta(img, scales=(1.0,), argmax=argmax)
        assert a.dtype == b.dtype and a.shape == b.shape
        assert np.array_equal(np.asarray(a).view(np.uint8), np.asarray(b).view(np.uint8))
    e.close()


# ---- 4. arbitrary sizes ------------------------------------------------------------------------------------------------------
def mean_padded(img, Hp, Wp):
    out = np.empty((img.shape[0], Hp, Wp, 3), np.float32)
    out[:] = np.asarray(MEAN_RGB, np.float32)
    out[:, : img.shape[1], : img.shape[2]] = img
    return out


@pytest.mark.parametrize("N,H,W", [(2, 50, 70), (1, 375, 1242)])
def test_any_size_equals_crop_of_mean_padded_predict(N, H, W):
    e = engine()
    img = images(N, H, W, seed=5)
    _, _, Hp, Wp = tta.pass_shape(H, W, 1.0)
    ref = e.predict(mean_padded(img, Hp, Wp), argmax=False)[:, :H, :W]
    sm = e.predict_tta(img, scales=(1.0,), argmax=False)
    am = e.predict_tta(img, scales=(1.0,), argmax=True)
    assert sm.shape == (N, H, W, 20) and am.shape == (N, H, W)
    check_probs(sm, ref, 1e-6)
    check_argmax(am, ref)
    e.close()


# ---- 5. the full composition -----------------------------------------------------------------------------------------------
def host_composition(e, img, scales, flip):
    N, H, W = img.shape[:3]
    lgs, flips = [], []
    for s, f, Hs, Ws, Hp, Wp in tta.passes(H, W, tta.validate(scales), flip):
        x = np.stack([cv2_compat.resize_linear(img[n], Hs, Ws) for n in range(N)])
        if f:
            x = x[:, :, ::-1]
        e.predict(mean_padded(x, Hp, Wp), argmax=False)
        lgs.append(e.activation("logits", (N, Hp, Wp, 20))[:, :Hs, :Ws])
        flips.append(f)
    return tta.compose(lgs, flips, H, W)


@pytest.mark.parametrize("widths,precision,N,H,W,scales", [
    (SMALL, "fp32", 2, 96, 160, (0.5, 1.0, 1.5)),
    (SMALL64, "bf16_train", 2, 96, 160, (0.5, 1.0, 1.5)),
    (SMALL, "fp32", 1, 1024, 512, (0.75, 1.0, 1.25)),
])
def test_composition_of_six_passes(widths, precision, N, H, W, scales):
    e = engine(widths, precision)
    img = images(N, H, W, seed=7)
    sm = e.predict_tta(img, scales=scales, flip=True, argmax=False)
    am = e.predict_tta(img, scales=scales, flip=True, argmax=True)
    ref = host_composition(e, img, scales, True)
    check_probs(sm, ref, 1e-5)
    check_argmax(am, ref)
    e.close()


def test_device_inputs_and_outputs():
    e = engine()
    img = images(2, 45, 67, seed=9)
    host = e.predict_tta(img, scales=(0.75, 1.25), flip=True, argmax=False)
    devo = e.predict_tta(dev(img), scales=(0.75, 1.25), flip=True, argmax=False)
    assert devo.is_cuda
    assert np.array_equal(devo.cpu().numpy(), host)
    e.close()


# ---- 6. determinism, allocations, frozen state -------------------------------------------------------------------------------
@pytest.mark.parametrize("frozen", [False, True])
def test_repeat_call_is_identical_and_allocates_nothing(frozen):
    e = engine()
    if frozen:
        e.freeze(True)
    img = images(2, 50, 70, seed=11)
    before = e.get_option("frozen")
    a = e.predict_tta(img, scales=(0.75, 1.0, 1.25), flip=True, argmax=False)
    n1 = e.get_option("workspace_allocations")
    b = e.predict_tta(img, scales=(0.75, 1.0, 1.25), flip=True, argmax=False)
    assert e.get_option("workspace_allocations") == n1
    assert np.array_equal(a.view(np.uint32), b.view(np.uint32))
    assert e.get_option("frozen") == before == int(frozen)
    with pytest.raises(ValueError):
        e.set_option("workspace_allocations", 0)
    e.close()


def test_bf16_train_repeat_call_allocates_nothing():
    e = engine(SMALL64, "bf16_train")
    img = images(1, 70, 90, seed=12)
    a = e.predict_tta(img, scales=(1.25, 0.5), flip=True)
    n1 = e.get_option("workspace_allocations")
    b = e.predict_tta(img, scales=(1.25, 0.5), flip=True)
    assert e.get_option("workspace_allocations") == n1
    assert np.array_equal(a, b)
    e.close()


@pytest.mark.parametrize("widths,precision", [(SMALL, "fp32"), (SMALL64, "bf16_train")])
def test_unfrozen_banks_are_rebuilt_after_a_parameter_change(widths, precision):
    """an unfrozen model keeps its banks' storage between calls, not their contents: new parameters give a fresh model's result"""
    e = engine(widths, precision, seed=1)
    img = images(1, 50, 70, seed=14)
    e.predict_tta(img, scales=(0.75, 1.0), flip=True, argmax=False)
    P2 = orc.init_params(20, widths, seed=2, decoder_std_scale=30.0, bias_std=0.05)
    e.set_params(P2)
    n1 = e.get_option("workspace_allocations")
    a = e.predict_tta(img, scales=(0.75, 1.0), flip=True, argmax=False)
    assert e.get_option("workspace_allocations") == n1
    f = engine(widths, precision, seed=2)
    b = f.predict_tta(img, scales=(0.75, 1.0), flip=True, argmax=False)
    assert np.array_equal(a.view(np.uint32), b.view(np.uint32))
    e.close(); f.close()


@pytest.mark.parametrize("widths,precision", [(SMALL, "fp32"), (SMALL64, "bf16_train")])
def test_predict_and_training_after_tta_match_a_fresh_model(widths, precision):
    """the re-carved workspace (and, in bf16_train, the kept padded bf16 copies, re-zeroed for each new shape) leaves nothing behind that a
    later predict at another shape, a predict at the last pass's shape or a training pass at that shape would see"""
    e, f = engine(widths, precision), engine(widths, precision)
    e.predict_tta(images(1, 70, 90), scales=(1.25, 0.5), flip=True)
    _, _, Hp, Wp = tta.pass_shape(70, 90, 0.5)                         # the last pass ran at Hp x Wp
    for (h, w) in [(96, 128), (Hp, Wp)]:
        img = images(1, h, w, seed=h)
        assert np.array_equal(e.predict(img, argmax=False), f.predict(img, argmax=False))
    img = images(1, Hp, Wp, seed=15)
    lab = np.random.default_rng(15).integers(0, 20, (1, Hp, Wp), dtype=np.uint8)
    le, lf = e.forward_backward(img, lab, keep_prob=1.0), f.forward_backward(img, lab, keep_prob=1.0)
    assert abs(le - lf) <= 1e-6 * max(1.0, abs(lf)), (le, lf)
    ge, gf = e.get_grads(), f.get_grads()
    for k in gf:
        err = np.abs(ge[k] - gf[k]).max() / (np.abs(gf[k]).max() + 1e-30)
        assert err < 1e-4, (k, err)
    e.close(); f.close()


# ---- 7. errors and the facade ----------------------------------------------------------------------------------------------
def test_bad_arguments_raise():
    e = engine()
    img = images(1, 48, 64)
    for bad in [(), (1.0,) * 9, (0.0,), (-0.5,), (4.5,), (float("nan"),), (float("inf"),)]:
        with pytest.raises(ValueError):
            e.predict_tta(img, scales=bad)
    with pytest.raises(ValueError):
        e.predict_tta(img.astype(np.float32), scales=(0.5,))
    e.predict_tta(img.astype(np.float32), scales=(1.0,), flip=True)            # float32 without resizing is taken
    arr = (C.c_float * 1)(0.5)
    out = np.empty((1, 48, 64), np.int64)
    f32 = np.ascontiguousarray(img, np.float32)
    rc = L.lib.fcn8s_predict_tta(e.h, f32.ctypes.data_as(C.c_void_p), L.IMG_F32, 1, 48, 64, arr, 1, 0, 1, out.ctypes.data_as(C.c_void_p), L.HOST)
    assert rc == L.ERR_BAD_ARG
    e.close()


def _facade():
    from fcn8s_tensorflow_amd.fcn8s import FCN8s
    return FCN8s(vgg16_dir='synthetic:3', num_classes=20, widths=SMALL)


def test_facade_predict_any_size(tmp_path):
    from PIL import Image
    from fcn8s_tensorflow_amd import cityscapes_eval as ce
    m = _facade()
    img = images(2, 48, 64, seed=17)
    with pytest.raises(ValueError):
        m.predict(img)                                           # the reference's rule stands without TTA
    assert m.predict(img, scales=(1.0,)).shape == (2, 48, 64)
    for bad in [(), (0.0,), (5.0,)]:
        with pytest.raises(ValueError):
            m.predict(img, scales=bad)
    src = tmp_path / "leftImg8bit" / "city"
    src.mkdir(parents=True)
    files = {"a_leftImg8bit.png": images(1, 45, 77, seed=1)[0], "b_leftImg8bit.png": images(1, 64, 50, seed=2)[0]}
    for name, a in files.items():
        Image.fromarray(a).save(str(src / name))
    n = m.predict_and_export_label_ids(str(tmp_path / "results"), str(tmp_path / "leftImg8bit"), scales=(0.75, 1.0), flip=True)
    assert n == 2
    for name, a in files.items():
        got = np.asarray(Image.open(str(tmp_path / "results" / name)))
        want = ce.TRAINIDS_TO_IDS_ARRAY[m.predict([a], scales=(0.75, 1.0), flip=True)[0]]
        assert np.array_equal(got, want)
    m.predict_and_save(str(tmp_path / "out"), str(src), {c: (0, 255, 0, 127) for c in range(20)}, scales=(1.0,), flip=True)
    assert sorted(p.name for p in (tmp_path / "out").iterdir()) == sorted(files)
