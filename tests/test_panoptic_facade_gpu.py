"""The `panoptic` argument of FCN8s.evaluate_cityscapes and cityscapes_eval.evaluate_directory on the small synthetic model of
test_regions_facade_gpu.py and synthetic PNG triples.  The table is all integers and the scores are one float64 route on the host: every
comparison is exact, against panoptic.py's NumPy route on what `predict` returns."""
import math
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from fcn8s_tensorflow_amd import cityscapes_eval as ce, panoptic as PQ  # noqa: E402

SMALL = (8, 16, 32, 64, 64, 128, 128)
K = 16                                                         # min_region of the second route


def make_model():
    """As test_regions_facade_gpu.py makes it: livelier decoder weights and a bilinear last upsampling, so that the argmax map has regions
    with specks between them."""
    from fcn8s_tensorflow_amd.fcn8s import FCN8s
    from oracle import fcn8s_oracle as orc
    m = FCN8s(vgg16_dir='synthetic:3', num_classes=20, widths=SMALL)
    m.engine.set_option("deterministic", 1)
    P = orc.init_params(20, SMALL, seed=3, decoder_std_scale=12.0, bias_std=0.05)
    g = 1.0 - np.abs(np.arange(16) - 7.5) / 8.0
    up = np.zeros((16, 16, 20, 20), np.float32)
    up[:, :, np.arange(20), np.arange(20)] = np.outer(g, g).astype(np.float32)[:, :, None]
    P["fc7_pool4_pool3_conv2d_trans/kernel"] = up
    m.engine.set_params(P)
    return m


def make_image(rng, h=64, w=96):
    img = np.kron(rng.integers(0, 256, (h // 8, w // 8, 3)), np.ones((8, 8, 1), np.int64)).astype(np.uint8)
    return img // 2 + rng.integers(0, 128, (h, w, 3), dtype=np.uint8)


@pytest.fixture(scope="module")
def model():
    m = make_model()
    yield m
    m.close()


NAMES = ["aachen_000000_000019", "aachen_000001_000019", "bonn_000002_000019"]


@pytest.fixture(scope="module")
def triples(tmp_path_factory):
    """Three images with label-id and instance-id maps: blocks of labels, boxes of instances (every fourth a crowd region)."""
    from PIL import Image
    root = tmp_path_factory.mktemp("panoptic_triples")
    rng = np.random.default_rng(8)
    things = np.array(ce.HAS_INSTANCES_IDS)
    insts = {}
    for nm in NAMES:
        city = nm.split("_")[0]
        (root / "leftImg8bit" / city).mkdir(parents=True, exist_ok=True); (root / "gtFine" / city).mkdir(parents=True, exist_ok=True)
        gt = np.kron(rng.integers(0, 34, (8, 12)), np.ones((8, 8), np.int64)).astype(np.uint8)
        inst = gt.astype(np.uint16)
        for k in range(10):
            lab = int(things[rng.integers(0, len(things))])
            y, x, h, w = int(rng.integers(0, 50)), int(rng.integers(0, 80)), int(rng.integers(1, 14)), int(rng.integers(1, 16))
            gt[y:y + h, x:x + w] = lab; inst[y:y + h, x:x + w] = lab * 1000 + k if k % 4 else lab
        Image.fromarray(make_image(rng)).save(root / "leftImg8bit" / city / (nm + "_leftImg8bit.png"))
        Image.fromarray(gt).save(root / "gtFine" / city / (nm + "_gtFine_labelIds.png"))
        Image.fromarray(inst).save(root / "gtFine" / city / (nm + "_gtFine_instanceIds.png"))
        insts[nm] = inst
    return root, str(root / "leftImg8bit"), str(root / "gtFine" / "*" / "*_gtFine_labelIds.png"), insts


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


def _numpy_results(model, root, insts, conn, **kw):
    """panoptic.results over pair_rows_numpy(predict(...)) per file, in file order."""
    from PIL import Image
    stats = PQ.new_stats()
    for nm in sorted(NAMES):
        img = np.array(Image.open(root / "leftImg8bit" / nm.split("_")[0] / (nm + "_leftImg8bit.png")).convert("RGB"))
        rows, bad = PQ.pair_rows_numpy(model.predict(img[None], **kw)[0], insts[nm], conn)
        assert bad == 0
        PQ.stats_add(stats, rows)
    return PQ.results(stats)


def test_evaluate_cityscapes_equals_the_numpy_route_on_predict(model, triples, tmp_path):
    root, images_dir, search, insts = triples
    off = model.evaluate_cityscapes(images_dir, search)
    fps = {}
    for tag, kw in (("plain", dict()), ("clean", dict(min_region=K))):
        for conn in (4, 8):
            res = model.evaluate_cityscapes(images_dir, search, panoptic=conn, **kw)
            want = _numpy_results(model, root, insts, conn, **kw)
            assert res["panopticConnectivity"] == conn
            for k in want:
                _same(res[k], want[k], "%s/c%d/%s" % (tag, conn, k))
            assert set(res) - set(off) == set(ce.PANOPTIC_RESULT_KEYS) and [k for k in res if k not in ce.PANOPTIC_RESULT_KEYS] == list(off)
            if not kw:
                _same({k: res[k] for k in off}, off, "the parent's entries beside the panoptic ones")
            # the export route: label-id PNGs through evaluate_directory, on the GPU and in NumPy
            out = str(tmp_path / ("export_%s" % tag))
            assert model.predict_and_export_label_ids(out, images_dir, **kw) == 3
            for device in (torch.device("cuda"), None):
                exp = ce.evaluate_directory(search, out, device=device, instance_level=True, panoptic=conn)
                for k in ce.PANOPTIC_RESULT_KEYS:
                    _same(exp[k], res[k], "%s/c%d/export/%s/%s" % (tag, conn, device, k))
        fps[tag] = int(res["panopticFp"].sum())
        assert int(res["panopticTp"].sum()) + int(res["panopticFn"].sum()) > 0 and res["panopticQuality"]["All"]["n"] > 0
    print("unmatched predicted segments (fp), plain and with min_region=%d:" % K, fps)
    assert fps["clean"] != fps["plain"]                         # the cleanup shows in the segment counts


def test_off_is_the_parents_dict_and_nothing_is_allocated(model, triples):
    root, images_dir, search, insts = triples
    off = model.evaluate_cityscapes(images_dir, search, boundary_radius=2)
    _same(model.evaluate_cityscapes(images_dir, search, boundary_radius=2, panoptic=None), off)
    assert not any(k.startswith("panoptic") for k in off)
    ev = ce.PixelLevelEvaluator(instance_level=True, panoptic=None)
    assert not hasattr(ev, "_panoptic_work") and not hasattr(ev, "panoptic_stats")
    fresh = make_model()
    fresh.evaluate_cityscapes(images_dir, search)
    assert not hasattr(fresh.engine, "_panoptic_work") and not hasattr(fresh.engine, "_regions_work")
    # the engine's own entry point keeps its scratch
    pred = fresh.predict(torch.zeros((1, 64, 96, 3), dtype=torch.uint8, device="cuda"))
    rows, bad = fresh.engine.panoptic_pair(pred, insts[NAMES[0]][None], connectivity=4)
    want, wbad = PQ.pair_rows_numpy(pred.cpu().numpy(), insts[NAMES[0]][None], 4)
    assert np.array_equal(rows[0], want[0]) and bad.tolist() == wbad
    table = fresh.engine._panoptic_work["table"].data_ptr()
    fresh.engine.panoptic_pair(pred, insts[NAMES[0]][None], connectivity=8)
    assert fresh.engine._panoptic_work["table"].data_ptr() == table
    fresh.close()


def test_refusals(model, triples, tmp_path):
    root, images_dir, search, insts = triples
    with pytest.raises(ValueError, match="instance_level"):
        model.evaluate_cityscapes(images_dir, search, instance_level=False, panoptic=4)
    for wrong in (6, True, "8"):
        with pytest.raises(ValueError):
            model.evaluate_cityscapes(images_dir, search, panoptic=wrong)
    with pytest.raises(ValueError, match="instance_level"):
        ce.evaluate_file_pairs([], [], instance_level=False, panoptic=4)


def test_json_carries_the_keys(model, triples, tmp_path):
    import json
    root, images_dir, search, insts = triples
    path = str(tmp_path / "result.json")
    res = model.evaluate_cityscapes(images_dir, search, panoptic=4, json_path=path)
    with open(path) as f:
        d = json.load(f)
    assert d["panopticConnectivity"] == 4 and d["panopticFp"] == res["panopticFp"].tolist()
    assert d["panopticQuality"]["Stuff"]["n"] == res["panopticQuality"]["Stuff"]["n"]
