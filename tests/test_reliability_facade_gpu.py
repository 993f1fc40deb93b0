"""FCN8s.evaluate_reliability on a small synthetic model and three PNG pairs of different sizes: the device route (softmax and tables stay on
the GPU) against `reliability.Evaluator` fed the host arrays of the same predictions, the three routes, the errors, repeatability, the JSON
file and averaged_weights()."""
import json
import math
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

from fcn8s_tensorflow_amd import reliability as rel  # noqa: E402
from tests.test_reliability_host import nan_equal  # noqa: E402

SMALL = (8, 16, 32, 64, 64, 128, 128)
SIZES = [(64, 96), (40, 72), (32, 32)]
NAMES = ("calib", "sums", "hist", "bad")


def make_model(num_classes=20):
    from fcn8s_tensorflow_amd.fcn8s import FCN8s
    m = FCN8s(vgg16_dir='synthetic:3', num_classes=num_classes, widths=SMALL)
    m.engine.set_option("deterministic", 1)
    return m


@pytest.fixture(scope="module")
def setup(tmp_path_factory):
    from PIL import Image
    root = tmp_path_factory.mktemp("reliability")
    img_dir, gt_dir = root / "leftImg8bit" / "val" / "aachen", root / "gtFine" / "val" / "aachen"
    os.makedirs(img_dir); os.makedirs(gt_dir)
    rng = np.random.default_rng(17)
    pairs = []
    for i, (h, w) in enumerate(SIZES):
        img = rng.integers(0, 256, (h, w, 3), dtype=np.uint8)
        gt = rng.integers(0, 34, (h, w), dtype=np.uint8)
        stem = "aachen_%06d_000019" % i
        Image.fromarray(img).save(str(img_dir / (stem + "_leftImg8bit.png")))
        Image.fromarray(gt).save(str(gt_dir / (stem + "_gtFine_labelIds.png")))
        pairs.append((img, gt))
    m = make_model()
    yield m, str(root / "leftImg8bit" / "val"), str(root / "gtFine" / "val" / "*" / "*_gtFine_labelIds.png"), pairs
    m.close()


def tables_match(got, want, tag):
    """== everywhere but q_nll (sums[2]), which may differ by the number of counted pixels (the two logf's last bits).  True if that too is equal."""
    for name in NAMES:
        g, w = got[name] if isinstance(got, dict) else got[NAMES.index(name)], want[NAMES.index(name)]
        if name == "sums":
            d = abs(int(g[2]) - int(w[2]))
            print("%s: %d counted pixels, q_nll |device - numpy| = %d" % (tag, int(w[0]), d))
            assert (g[[0, 1, 3]] == w[[0, 1, 3]]).all() and d <= int(w[0]), (tag, g, w)
        else:
            assert (np.asarray(g) == w).all(), (tag, name)
    return int(got["sums"][2] if isinstance(got, dict) else got[1][2]) == int(want[1][2])


def strip(res):
    return {k: v for k, v in rel.result_dict(res).items() if k not in ("nbPixels", "route")}


def test_monte_carlo_route_against_the_host_evaluator(setup):
    m, img_dir, gt_glob, pairs = setup
    res = m.evaluate_reliability(img_dir, gt_glob, samples=4)
    assert res["route"] == "mc" and list(res["scores"]) == ["maxProb", "entropy", "mutualInformation"]
    assert res["nbPixels"] == sum(h * w for h, w in SIZES) and res["bins"] == 15 and res["scoreMax"]["entropy"] == math.log(20)
    ev = rel.Evaluator(bins=15, num_classes=20, lut=rel.cityscapes_lut(), score_names=("entropy", "mutualInformation"))
    for img, gt in pairs:
        sm, ent, mi = m.predict_uncertainty(img[None], argmax=False, samples=4)
        assert isinstance(sm, np.ndarray)
        ev.add(sm, gt[None], [ent, mi])
    same = tables_match(res["tables"], ev.tables(), "samples=4")
    assert res["pixels"] == int((rel.cityscapes_lut()[np.concatenate([g.reshape(-1) for _, g in pairs])] != 255).sum()) and not res["tables"]["bad"].any()
    # every derived measure is a function of the tables alone ...
    own = rel.measures(*[res["tables"][k] for k in NAMES], score_names=("entropy", "mutualInformation"))
    assert nan_equal(rel.result_dict(own), {k: v for k, v in strip(res).items() if k not in ("bins", "scoreMax")})
    # ... so with equal tables the host evaluator reports the same numbers
    if same:
        assert nan_equal(rel.result_dict(ev.results()), strip(res))
    assert 0 <= res["ece"] <= 1 and 0 < res["nll"] and 0 <= res["scores"]["entropy"]["auroc"] <= 1
    # a second identical call returns identical tables
    again = m.evaluate_reliability(img_dir, gt_glob, samples=4)
    assert all((again["tables"][k] == res["tables"][k]).all() for k in NAMES) and nan_equal(strip(again), strip(res))
    # other masks, other tables
    other = m.evaluate_reliability(img_dir, gt_glob, samples=4, sample_offset=4)
    assert not (other["tables"]["hist"] == res["tables"]["hist"]).all()


def test_single_pass_route_is_predict_with_the_entropy_map(setup):
    import torch
    m, img_dir, gt_glob, pairs = setup
    res = m.evaluate_reliability(img_dir, gt_glob)
    assert res["route"] == "single" and list(res["scores"]) == ["maxProb", "entropy"] and "mutualInformation" not in res["scores"]
    one = m.evaluate_reliability(img_dir, gt_glob, samples=1, keep_prob=1.0)
    assert list(one["scores"]) == ["maxProb", "entropy", "mutualInformation"]
    for k in ("calib", "sums", "bad"):
        assert (res["tables"][k] == one["tables"][k]).all(), k
    assert (res["tables"]["hist"] == one["tables"]["hist"][:2]).all()
    assert one["tables"]["hist"][2, 1:].sum() == 0                     # no dropout: the mutual information is 0.0 everywhere
    for k in ("ece", "mce", "nll", "brier", "accuracy"):
        assert res[k] == one[k]
    assert nan_equal(rel.result_dict(res["scores"]["entropy"]), rel.result_dict(one["scores"]["entropy"]))
    # the route's probabilities are `predict`'s: the same argmax (sizes `predict` takes), hence the same count of correct pixels
    lut = rel.cityscapes_lut()
    for img, gt in pairs:
        if img.shape[0] % 32 or img.shape[1] % 32:
            continue
        sm, _, _ = m.engine.predict_mc(torch.from_numpy(img[None]).cuda(), samples=1, keep_prob=1.0, argmax=False, mutual_information=False)
        pred = m.predict(img[None])
        assert (sm.argmax(-1).cpu().numpy() == pred).all()
        assert (sm.cpu().numpy() == m.predict(img[None], argmax=False)).all()


def test_passes_route_has_the_max_prob_score_only(setup):
    m, img_dir, gt_glob, pairs = setup
    res = m.evaluate_reliability(img_dir, gt_glob, scales=(1.0,), flip=True, bins=10)
    assert res["route"] == "passes" and list(res["scores"]) == ["maxProb"] and res["tables"]["hist"].shape == (1, rel.SCORE_BINS, 2)
    ev = rel.Evaluator(bins=10, num_classes=20, lut=rel.cityscapes_lut())
    for img, gt in pairs:
        ev.add(m.predict(img[None], argmax=False, scales=(1.0,), flip=True), gt[None])
    tables_match(res["tables"], ev.tables(), "scales=(1.0,), flip=True")
    assert res["tables"]["calib"].shape == (10, 3)


def test_refusals(setup):
    m, img_dir, gt_glob, _ = setup
    with pytest.raises(ValueError):
        m.evaluate_reliability(img_dir, gt_glob, samples=4, flip=True)
    with pytest.raises(ValueError):
        m.evaluate_reliability(img_dir, gt_glob, samples=4, scales=(1.0,))
    with pytest.raises(ValueError):
        m.evaluate_reliability(img_dir, gt_glob, samples=4, crf=True)
    with pytest.raises(ValueError):
        m.evaluate_reliability(img_dir, gt_glob, bins=0)
    with pytest.raises(ValueError):
        m.evaluate_reliability(img_dir, os.path.join(img_dir, "nothing", "*.png"))
    m19 = make_model(19)
    with pytest.raises(ValueError):
        m19.evaluate_reliability(img_dir, gt_glob)
    m19.close()


def test_json_file_holds_the_same_numbers(setup, tmp_path):
    m, img_dir, gt_glob, _ = setup
    path = str(tmp_path / "out" / "reliability.json")
    res = m.evaluate_reliability(img_dir, gt_glob, samples=2, json_path=path)
    back = json.load(open(path))
    assert nan_equal(json.loads(json.dumps(rel.result_dict(res))), back)
    assert back["tables"]["hist"] == res["tables"]["hist"].tolist() and back["ece"] == res["ece"] and back["route"] == "mc"


def test_unchanged_inside_and_after_averaged_weights_on_an_untrained_average(setup):
    m, img_dir, gt_glob, _ = setup
    before = m.evaluate_reliability(img_dir, gt_glob, samples=2)
    m.engine.set_ema(0.9, warmup=False)                                # no step taken: the shadow is the parameters
    try:
        with m.averaged_weights():
            inside = m.evaluate_reliability(img_dir, gt_glob, samples=2)
        after = m.evaluate_reliability(img_dir, gt_glob, samples=2)
    finally:
        m.engine.set_ema(None)
    for r in (inside, after):
        assert all((r["tables"][k] == before["tables"][k]).all() for k in NAMES) and nan_equal(strip(r), strip(before))
