"""FCN8s.evaluate_cityscapes_instances and FCN8s.predict_and_export_instances on the small synthetic model of test_regions_facade_gpu.py
and three synthetic images with instance maps.  The table is all integers and the scores are one float64 route on the host: every
comparison is exact, against instances.py's NumPy route on the softmax that the route itself returns."""
import math
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from fcn8s_tensorflow_amd import instances as INS, regions as RG  # noqa: E402
from tests.test_panoptic_facade_gpu import make_image, make_model  # noqa: E402

K = 16                                                         # min_region of the cleanup route
SIZES = {"aachen_000000_000019": (64, 96), "aachen_000001_000019": (80, 64), "bonn_000002_000019": (96, 128)}
NAMES = sorted(SIZES)
THINGS = np.array(INS.INST_LABEL_IDS + [29, 30])


@pytest.fixture(scope="module")
def model():
    m = make_model()
    yield m
    m.close()


@pytest.fixture(scope="module")
def scenes(tmp_path_factory):
    """Three images of three sizes with instance-id maps: blocks of labels, boxes of instances (every fourth a group region)."""
    from PIL import Image
    root = tmp_path_factory.mktemp("instance_scenes")
    rng = np.random.default_rng(9)
    insts = {}
    for nm in NAMES:
        h, w = SIZES[nm]
        city = nm.split("_")[0]
        (root / "leftImg8bit" / city).mkdir(parents=True, exist_ok=True); (root / "gtFine" / city).mkdir(parents=True, exist_ok=True)
        inst = np.kron(rng.integers(0, 24, (h // 8, w // 8)), np.ones((8, 8), np.int64)).astype(np.uint16)
        for k in range(12):
            lab = int(THINGS[rng.integers(0, len(THINGS))])
            y, x, bh, bw = int(rng.integers(0, h - 20)), int(rng.integers(0, w - 24)), int(rng.integers(4, 20)), int(rng.integers(4, 24))
            inst[y:y + bh, x:x + bw] = lab * 1000 + k if k % 4 else lab
        Image.fromarray(make_image(rng, h, w)).save(root / "leftImg8bit" / city / (nm + "_leftImg8bit.png"))
        Image.fromarray(inst).save(root / "gtFine" / city / (nm + "_gtFine_instanceIds.png"))
        insts[nm] = inst
    return root, str(root / "leftImg8bit"), str(root / "gtFine" / "*" / "*_gtFine_instanceIds.png"), insts


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


def _image(root, nm):
    from PIL import Image
    img = np.array(Image.open(root / "leftImg8bit" / nm.split("_")[0] / (nm + "_leftImg8bit.png")).convert("RGB"))
    return torch.from_numpy(img[None]).cuda()


def _softmax(model, image, route):
    """The softmax of a route through the model's public entry points, on the host."""
    e = model.engine
    if route.get("samples") is not None:
        prob = e.predict_mc(image, samples=route["samples"], keep_prob=0.5, sample_offset=0, argmax=False, entropy=False, mutual_information=False)[0]
    elif "scales" in route or "flip" in route:
        prob = model.predict(image, argmax=False, scales=route.get("scales"), flip=route.get("flip", False))
    else:
        prob = e.predict_mc(image, samples=1, keep_prob=1.0, sample_offset=0, argmax=False, entropy=False, mutual_information=False)[0]
    if route.get("temperature") is not None:
        e.temperature_apply(prob, route["temperature"], out=prob)
    return prob.cpu().numpy()[0]


def _numpy_results(model, root, insts, conn, route, min_instance_pixels=0):
    """instances.results over pair_rows_numpy of the route's own softmax per file, in file order; also the label maps and the instance counts."""
    stats, labels_of = INS.new_stats(), {}
    model.engine.freeze(True)
    try:
        for nm in NAMES:
            prob = _softmax(model, _image(root, nm), route)
            labels = np.argmax(prob, -1).astype(np.uint8)
            if route.get("min_region"):
                labels = RG.clean_numpy(labels, route["min_region"], connectivity=4, rounds=1)[0].astype(np.uint8)
            rows, bad = INS.pair_rows_numpy(prob, labels, insts[nm], conn)
            assert not bad.any()
            INS.stats_add(stats, rows, min_instance_pixels)
            labels_of[nm] = labels
    finally:
        model.engine.freeze(False)
    return INS.results(stats), labels_of


ROUTES = [("plain", dict()), ("temperature", dict(temperature=2.5)), ("mc", dict(samples=4)), ("tta", dict(scales=(0.75, 1.0), flip=True)),
          ("clean", dict(min_region=K))]


def test_evaluate_equals_the_numpy_route_on_the_routes_own_softmax(model, scenes, tmp_path):
    root, images_dir, search, insts = scenes
    counts = {}
    for tag, route in ROUTES:
        conn = 8 if tag == "tta" else 4
        res = model.evaluate_cityscapes_instances(images_dir, search, connectivity=conn, **route)
        want, _labels = _numpy_results(model, root, insts, conn, route)
        for k in want:
            _same(res[k], want[k], "%s/%s" % (tag, k))
        assert res["connectivity"] == conn and res["nbPixels"] == sum(h * w for h, w in SIZES.values())
        assert res["route"] == {"plain": "single", "temperature": "single", "mc": "mc", "tta": "passes", "clean": "single"}[tag]
        counts[tag] = int(res["nbPredictions"].sum())
        assert counts[tag] > 0 and int(res["nbGroundTruth"].sum()) > 0
    print("predicted instances per route:", counts)
    assert counts["clean"] != counts["plain"]                  # the cleanup changes the number of predicted instances
    small = model.evaluate_cityscapes_instances(images_dir, search, min_instance_pixels=K)
    want, _l = _numpy_results(model, root, insts, 4, dict(), min_instance_pixels=K)
    _same(small["ap"], want["ap"], "min_instance_pixels")
    assert int(small["nbPredictions"].sum()) < counts["plain"]


def test_export_read_back_gives_the_same_dict(model, scenes, tmp_path):
    import json
    root, images_dir, search, insts = scenes
    from glob import glob
    gts = sorted(glob(search))
    for tag, route in (ROUTES[0], ROUTES[4]):
        res = model.evaluate_cityscapes_instances(images_dir, search, json_path=str(tmp_path / (tag + ".json")), **route)
        out = model.predict_and_export_instances(str(tmp_path / ("export_" + tag)), images_dir, **route)
        assert out["nbImages"] == 3 and out["nbInstances"] == int(res["nbPredictions"].sum()) and [os.path.basename(f) for f in out["files"]] == [nm + "_leftImg8bit.txt" for nm in NAMES]
        back = INS.evaluate_directory(out["files"], gts)
        for k in back:
            _same(back[k], res[k], "%s/export/%s" % (tag, k))
        with open(tmp_path / (tag + ".json")) as f:
            d = json.load(f)
        assert sorted(d) == ["averages", "instLabels", "minRegionSizes", "overlaps", "resultApMatrix"]
        # masks of one image are disjoint and cover exactly the thing pixels of the label map
        _want, labels_of = _numpy_results(model, root, insts, 4, route)
        for f, nm in zip(out["files"], NAMES):
            masks = [m for m, _l, _c in INS.read_export(f)]
            cover = np.sum(masks, axis=0) if masks else np.zeros(SIZES[nm], np.int64)
            things = (labels_of[nm] >= 12) & (labels_of[nm] < 20)
            assert np.array_equal(cover, things.astype(cover.dtype)), (tag, nm)


def test_the_frozen_state_is_restored_also_after_an_exception(model, scenes, tmp_path):
    from PIL import Image
    root, images_dir, search, insts = scenes
    bad_root = tmp_path / "bad"
    (bad_root / "gtFine" / "aachen").mkdir(parents=True)
    Image.fromarray(np.zeros((32, 32), np.uint16)).save(bad_root / "gtFine" / "aachen" / (NAMES[0] + "_gtFine_instanceIds.png"))     # the wrong size
    bad_search = str(bad_root / "gtFine" / "*" / "*_gtFine_instanceIds.png")
    for frozen in (False, True):
        model.engine.freeze(frozen)
        model.evaluate_cityscapes_instances(images_dir, search)
        assert bool(model.engine.get_option("frozen")) == frozen
        with pytest.raises(ValueError, match="not equal"):
            model.evaluate_cityscapes_instances(images_dir, bad_search)
        assert bool(model.engine.get_option("frozen")) == frozen
        with pytest.raises(ValueError):
            model.predict_and_export_instances(str(tmp_path / "never"), str(tmp_path / "no_images_here"))
        assert bool(model.engine.get_option("frozen")) == frozen
    model.engine.freeze(False)


def test_refusals(model, scenes, tmp_path):
    root, images_dir, search, insts = scenes
    with pytest.raises(ValueError):
        model.evaluate_cityscapes_instances(images_dir, search, connectivity=6)
    with pytest.raises(ValueError):
        model.evaluate_cityscapes_instances(images_dir, search, min_instance_pixels=-1)
    with pytest.raises(ValueError):
        model.evaluate_cityscapes_instances(images_dir, search, samples=4, temperature=2.0)            # evaluate_reliability's refusals
    with pytest.raises(ValueError):
        model.evaluate_cityscapes_instances(images_dir, search, samples=4, flip=True)
    with pytest.raises(ValueError, match="Cannot find"):
        model.evaluate_cityscapes_instances(images_dir, str(tmp_path / "*.png"))
