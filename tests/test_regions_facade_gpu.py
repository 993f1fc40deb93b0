"""The `min_region` argument of FCN8s.predict, predict_and_export_label_ids, predict_and_save and evaluate_cityscapes on the small synthetic
model with livelier decoder weights (as test_temperature_facade_gpu.py makes it: the default synthetic softmax is uniform).  The cleanup is
all integers: every comparison is `==` against regions.py's NumPy route on the prediction without cleanup."""
import math
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from fcn8s_tensorflow_amd import cityscapes_eval as ce, regions as R  # noqa: E402

SMALL = (8, 16, 32, 64, 64, 128, 128)
DECODER_SCALE = 12.0
K = 24                                                         # the threshold of the tests


def make_model():
    """The synthetic model of test_temperature_facade_gpu.py, with the last upsampling (16 x 16, stride 8) set to the bilinear kernel an FCN-8s
    is initialised with.  With random weights there, the argmax is noise from pixel to pixel (5500 components on 6144 pixels, measured): almost
    nothing has a neighbour that is not small, and the cleanup changes nothing.  With the bilinear kernel the map has regions of 100 to 200
    pixels with specks between them: about 180 components per 64 x 96 image, and K = 24 moves 11 to 13 % of the pixels (the oracle's forward
    pass on the CPU)."""
    from fcn8s_tensorflow_amd.fcn8s import FCN8s
    from oracle import fcn8s_oracle as orc
    m = FCN8s(vgg16_dir='synthetic:3', num_classes=20, widths=SMALL)
    m.engine.set_option("deterministic", 1)
    P = orc.init_params(20, SMALL, seed=3, decoder_std_scale=DECODER_SCALE, bias_std=0.05)
    g = 1.0 - np.abs(np.arange(16) - 7.5) / 8.0
    up = np.zeros((16, 16, 20, 20), np.float32)
    up[:, :, np.arange(20), np.arange(20)] = np.outer(g, g).astype(np.float32)[:, :, None]
    assert P["fc7_pool4_pool3_conv2d_trans/kernel"].shape == up.shape
    P["fc7_pool4_pool3_conv2d_trans/kernel"] = up
    m.engine.set_params(P)
    return m


def make_image(rng, h=64, w=96):
    """Blocks of 8 x 8 with a little noise: an argmax map of regions with specks on them."""
    img = np.kron(rng.integers(0, 256, (h // 8, w // 8, 3)), np.ones((8, 8, 1), np.int64)).astype(np.uint8)
    return img // 2 + rng.integers(0, 128, (h, w, 3), dtype=np.uint8)


@pytest.fixture(scope="module")
def model():
    m = make_model()
    yield m
    m.close()


@pytest.fixture(scope="module")
def images():
    rng = np.random.default_rng(41)
    return np.stack([make_image(rng), make_image(rng)])


ROUTES = (dict(), dict(scales=(0.75, 1.0), flip=True), dict(crf=True))


def test_predict_with_cleanup_equals_the_numpy_route_on_the_plain_prediction(model, images):
    changed = []
    for kw in ROUTES:
        plain = model.predict(images, **kw)
        assert isinstance(plain, np.ndarray) and plain.dtype == np.int64
        for conn, rounds in ((4, 1), (8, 3)):
            want, stats = R.clean_numpy(plain, K, conn, rounds)
            got = model.predict(images, min_region=K, region_connectivity=conn, region_rounds=rounds, **kw)
            assert isinstance(got, np.ndarray) and got.dtype == np.int64 and np.array_equal(got, want), (kw, conn, rounds)
            dgot = model.predict(torch.from_numpy(images).cuda(), min_region=K, region_connectivity=conn, region_rounds=rounds, **kw)
            assert isinstance(dgot, torch.Tensor) and dgot.is_cuda and dgot.dtype == torch.int64
            assert np.array_equal(dgot.cpu().numpy(), want), (kw, conn, rounds, "device input")
            changed.append(max(float((w != p).mean()) for w, p in zip(want, plain)))
        # the other forms of the argument
        per_class = {c: K for c in range(20)}
        assert np.array_equal(model.predict(images, min_region=per_class, **kw), R.clean_numpy(plain, K, 4, 1)[0])
        table = [K if c % 2 else 0 for c in range(20)]
        full = np.zeros(256, np.int32); full[:20] = table
        assert np.array_equal(model.predict(images, min_region=table, **kw), R.clean_numpy(plain, full, 4, 1)[0])
    print("largest share of pixels changed on an image, per route and setting:", ["%.4f" % c for c in changed])
    assert min(changed) >= 0.01                                # not vacuous: the cleanup changes at least 1 % of the pixels of an image


def test_off_means_the_same_bits_and_nothing_launched(model, images):
    for kw in ROUTES:
        plain = model.predict(images, **kw)
        for off in (None, 0, False, [0] * 20, {}):
            assert np.array_equal(model.predict(images, min_region=off, **kw), plain)
        soft = model.predict(images, argmax=False, **kw)
        assert np.array_equal(model.predict(images, argmax=False, min_region=None, **kw), soft)
    fresh = make_model()
    fresh.predict(images, min_region=None); fresh.predict(images, min_region=0)
    assert not hasattr(fresh.engine, "_regions_work")          # off: no scratch was ever made
    fresh.predict(images, min_region=K)
    assert fresh.engine._regions_work.numel() >= 16 * images.shape[0] * 64 * 96
    fresh.close()


def test_refusals(model, images):
    with pytest.raises(ValueError, match="argmax"):
        model.predict(images, argmax=False, min_region=K)
    for bad in (-1, 2.5, [K] * 19, {20: 4}, True):
        with pytest.raises(ValueError):
            model.predict(images, min_region=bad)
    with pytest.raises(ValueError):
        model.predict(images, min_region=K, region_connectivity=6)
    with pytest.raises(ValueError):
        model.predict(images, min_region=K, region_rounds=0)


def _same(a, b, where=""):
    if isinstance(a, dict):
        assert isinstance(b, dict) and list(a) == list(b), where
        for k in a:
            _same(a[k], b[k], "%s/%s" % (where, k))
    elif isinstance(a, (list, tuple)):
        assert len(a) == len(b), where
        for i, (x, y) in enumerate(zip(a, b)):
            _same(x, y, "%s[%d]" % (where, i))
    elif isinstance(a, np.ndarray) or isinstance(b, np.ndarray):
        np.testing.assert_array_equal(np.asarray(a), np.asarray(b), err_msg=where)
    elif isinstance(a, float) and math.isnan(a):
        assert isinstance(b, float) and math.isnan(b), where
    else:
        assert a == b, where


def test_evaluate_cityscapes_equals_export_plus_directory_evaluation(model, tmp_path):
    from PIL import Image
    m = model
    rng = np.random.default_rng(8)
    names = ["aachen_000000_000019", "aachen_000001_000019", "bonn_000002_000019"]
    things = np.array(ce.HAS_INSTANCES_IDS)
    for nm in names:
        city = nm.split("_")[0]
        (tmp_path / "leftImg8bit" / city).mkdir(parents=True, exist_ok=True); (tmp_path / "gtFine" / city).mkdir(parents=True, exist_ok=True)
        img = make_image(rng)
        gt = np.kron(rng.integers(0, 34, (8, 12)), np.ones((8, 8), np.int64)).astype(np.uint8)
        inst = gt.astype(np.uint16)
        for k in range(10):
            lab = int(things[rng.integers(0, len(things))])
            y, x, h, w = int(rng.integers(0, 50)), int(rng.integers(0, 80)), int(rng.integers(1, 14)), int(rng.integers(1, 16))
            gt[y:y + h, x:x + w] = lab; inst[y:y + h, x:x + w] = lab * 1000 + k if k % 4 else lab
        Image.fromarray(img).save(tmp_path / "leftImg8bit" / city / (nm + "_leftImg8bit.png"))
        Image.fromarray(gt).save(tmp_path / "gtFine" / city / (nm + "_gtFine_labelIds.png"))
        Image.fromarray(inst).save(tmp_path / "gtFine" / city / (nm + "_gtFine_instanceIds.png"))
    images_dir, search = str(tmp_path / "leftImg8bit"), str(tmp_path / "gtFine" / "*" / "*_gtFine_labelIds.png")

    # off: the dict of the call without the keywords, key for key, and of the export route
    off = m.evaluate_cityscapes(images_dir, search, scales=(1.0,), boundary_radius=3)
    _same(m.evaluate_cityscapes(images_dir, search, scales=(1.0,), boundary_radius=3, min_region=None), off)
    out0 = str(tmp_path / "results_off")
    assert m.predict_and_export_label_ids(out0, images_dir, scales=(1.0,)) == 3
    _same(off, ce.evaluate_directory(search, out0, instance_level=True, boundary_radius=3))

    share = []
    for run, kw in enumerate((dict(scales=(1.0,)), dict(scales=(0.75, 1.0), flip=True, crf=True, region_connectivity=8, region_rounds=2))):
        res = m.evaluate_cityscapes(images_dir, search, boundary_radius=3, min_region=K, **kw)
        out = str(tmp_path / ("results%d" % run))
        assert m.predict_and_export_label_ids(out, images_dir, min_region=K, **kw) == 3
        _same(res, ce.evaluate_directory(search, out, instance_level=True, boundary_radius=3))
        assert list(res) == list(off) and res["nbPixels"] == 3 * 64 * 96
        # the export is the cleaned prediction, and the cleanup did something
        plain_kw = {k: v for k, v in kw.items() if not k.startswith("region_")}
        for nm in names:
            city = nm.split("_")[0]
            img = np.array(Image.open(tmp_path / "leftImg8bit" / city / (nm + "_leftImg8bit.png")).convert("RGB"))
            plain = m.predict(img[None], **plain_kw)
            want = R.clean_numpy(plain, K, kw.get("region_connectivity", 4), kw.get("region_rounds", 1))[0]
            assert np.array_equal(np.array(Image.open(os.path.join(out, nm + "_leftImg8bit.png"))), ce.TRAINIDS_TO_IDS_ARRAY[want[0]])
            share.append(float((want != plain).mean()))
        if run == 0:                                           # the route of `off`: the cleanup shows in the counts
            assert not np.array_equal(res["confMatrix"], off["confMatrix"])
    print("share of pixels changed per exported file:", ["%.4f" % s for s in share])
    assert max(share[:3]) >= 0.01 and max(share[3:]) >= 0.01


def test_predict_and_save_shows_the_cleaned_map(model, tmp_path):
    from PIL import Image
    rng = np.random.default_rng(3)
    src = tmp_path / "in"; src.mkdir()
    img = make_image(rng)
    Image.fromarray(img).save(src / "a.png")
    colors = {c: (int(rng.integers(0, 256)), int(rng.integers(0, 256)), int(rng.integers(0, 256)), 255) for c in range(20)}
    model.predict_and_save(str(tmp_path / "plain"), str(src), colors)
    model.predict_and_save(str(tmp_path / "clean"), str(src), colors, min_region=K)
    want = R.clean_numpy(model.predict(img[None]), K, 4, 1)[0][0]
    shown = np.array(Image.open(tmp_path / "clean" / "a.png").convert("RGB"))
    expect = np.array([colors[c][:3] for c in range(20)], np.uint8)[want]
    assert np.array_equal(shown, expect)
    assert not np.array_equal(shown, np.array(Image.open(tmp_path / "plain" / "a.png").convert("RGB")))
