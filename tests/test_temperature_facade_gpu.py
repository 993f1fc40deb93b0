"""FCN8s.fit_temperature, and the `temperature` argument of predict and evaluate_reliability, on the small synthetic model and three PNG pairs of
test_reliability_facade_gpu.py's shapes.  The ground truth is the model's own argmax on a fraction of the pixels and random elsewhere: at
FRACTION the float64 optimum on the downloaded softmaxes is interior to [0.125, 8] (asserted), so the fit has something to find.  The bar is
the one of test_temperature_ops_gpu.py: per counted pixel 8 E + 0.5 units of 2^-16, E from the float32 and float64 restatements on the same
softmaxes."""
import json
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

from fcn8s_tensorflow_amd import reliability as rel, temperature as ts  # noqa: E402
from tests.test_temperature_host import e_units, exact_nll, golden_section_temperature  # noqa: E402

SMALL = (8, 16, 32, 64, 64, 128, 128)
SIZES = [(64, 96), (40, 72), (32, 32)]
FRACTION = 0.7
NAMES = ("calib", "sums", "hist", "bad")


DECODER_SCALE = 12.0


def make_model(num_classes=20):
    """The synthetic model with livelier decoder weights (the oracle's `decoder_std_scale`, as smoke() uses it): with the reference's
    initialisation the softmax is uniform to four digits, and at smoke()'s 30 it is one-hot: the optimum then lies outside the ops' range
    of temperatures either way.  At 12 the median confidence is 0.72.  Measured on the MI355X, the float64 optimum at FRACTION = 0.1 / 0.3 /
    0.5 / 0.7 / 0.9: T = 18.2 / 6.6 / 4.0 / 2.5 / 1.2 -- 0.7 is an overconfident model whose optimum is well inside [0.125, 8]."""
    from fcn8s_tensorflow_amd.fcn8s import FCN8s
    from oracle import fcn8s_oracle as orc
    m = FCN8s(vgg16_dir='synthetic:3', num_classes=num_classes, widths=SMALL)
    m.engine.set_option("deterministic", 1)
    m.engine.set_params(orc.init_params(num_classes, SMALL, seed=3, decoder_std_scale=DECODER_SCALE, bias_std=0.05))
    return m


@pytest.fixture(scope="module")
def setup(tmp_path_factory):
    from PIL import Image
    from fcn8s_tensorflow_amd import cityscapes_eval as ce
    root = tmp_path_factory.mktemp("temperature")
    img_dir, gt_dir = root / "leftImg8bit" / "val" / "aachen", root / "gtFine" / "val" / "aachen"
    os.makedirs(img_dir); os.makedirs(gt_dir)
    rng = np.random.default_rng(23)
    m = make_model()
    pairs = []
    for i, (h, w) in enumerate(SIZES):
        img = rng.integers(0, 256, (h, w, 3), dtype=np.uint8)
        sm = m.engine.predict_mc(img[None], samples=1, keep_prob=1.0, argmax=False, entropy=False, mutual_information=False)[0]
        own = ce.TRAINIDS_TO_IDS_ARRAY[sm[0].argmax(-1)]               # label ids of the model's own argmax (train id 0 -> label 0: ignored)
        gt = np.where(rng.random((h, w)) < FRACTION, own, rng.integers(0, 34, (h, w))).astype(np.uint8)
        stem = "aachen_%06d_000019" % i
        Image.fromarray(img).save(str(img_dir / (stem + "_leftImg8bit.png")))
        Image.fromarray(gt).save(str(gt_dir / (stem + "_gtFine_labelIds.png")))
        pairs.append((img, gt, sm[0]))
    # the host's view of the same validation set: counted pixels only
    lut = rel.cityscapes_lut()
    t = np.concatenate([lut[g.reshape(-1)] for _, g, _ in pairs]).astype(np.int64)
    p = np.concatenate([s.reshape(-1, 20) for _, _, s in pairs])
    keep = t != 255
    host = dict(prob=p[keep], t=t[keep], best=golden_section_temperature(p[keep], t[keep]))
    yield m, str(root / "leftImg8bit" / "val"), str(root / "gtFine" / "val" / "*" / "*_gtFine_labelIds.png"), pairs, host
    m.close()


def bar(host, temperatures):
    """(8 E + 0.5) / 2^16 per counted pixel for these temperatures on the host's softmaxes, and E."""
    gt = host["t"].astype(np.uint8)[None]
    E, _, _ = e_units(host["prob"][None], gt, rel.identity_lut(), ts.betas_of(temperatures))
    return (8 * E + 0.5) / ts.Q_NLL, E


def test_the_fit_matches_the_host_and_a_second_call_returns_the_same_integers(setup):
    m, img_dir, gt_glob, pairs, host = setup
    assert 0.125 * 1.2 < host["best"] < 8.0 / 1.2, host["best"]        # interior: FRACTION was chosen for that
    res = m.fit_temperature(img_dir, gt_glob)
    assert res["route"] == "single" and res["nbPixels"] == sum(h * w for h, w in SIZES) and res["pixels"] == len(host["t"])
    assert m.temperature == res["temperature"] and not res["atBound"]
    assert len(res["candidates"]) == 2 and all(len(c) == 32 for c in res["candidates"]) and any(T == 1.0 for T, _ in res["candidates"][0])
    last = [T for T, _ in res["candidates"][-1]]
    step = last[1] / last[0]
    ratio = max(res["temperature"] / host["best"], host["best"] / res["temperature"])
    print("fit %.4f, host golden section %.4f: ratio %.5f, the last grid's step ratio %.5f" % (res["temperature"], host["best"], ratio, step))
    assert ratio <= step
    tol, E = bar(host, [1.0, res["temperature"]])
    before = exact_nll(host["prob"], host["t"], 1.0)
    after = exact_nll(host["prob"], host["t"], float(ts.betas_of([res["temperature"]])[0]))
    print("nll before %.6f (host %.6f), after %.6f (host %.6f), allowed %.2g (E = %.3f units)" % (res["nllBefore"], before, res["nllAfter"], after, tol, E))
    assert abs(res["nllBefore"] - before) <= tol and abs(res["nllAfter"] - after) <= tol and res["nllAfter"] < res["nllBefore"]
    again = m.fit_temperature(img_dir, gt_glob)
    assert again == res


def test_calibration_lowers_the_nll_that_evaluate_reliability_reports(setup):
    m, img_dir, gt_glob, pairs, host = setup
    res = m.fit_temperature(img_dir, gt_glob)
    T = res["temperature"]
    plain = m.evaluate_reliability(img_dir, gt_glob)
    cal = m.evaluate_reliability(img_dir, gt_glob, temperature=T)
    tol, E = bar(host, [T])
    print("nll %.6f -> %.6f (fit: %.6f -> %.6f), allowed %.2g" % (plain["nll"], cal["nll"], res["nllBefore"], res["nllAfter"], tol + 0.5 / ts.Q_NLL))
    assert cal["nll"] < plain["nll"] and cal["pixels"] == plain["pixels"] == res["pixels"]
    assert abs(cal["nll"] - res["nllAfter"]) <= tol + 0.5 / ts.Q_NLL     # (8 E + 1) units: both quantise
    assert abs(plain["nll"] - res["nllBefore"]) <= tol + 0.5 / ts.Q_NLL
    assert cal["route"] == "single" and list(cal["scores"]) == ["maxProb", "entropy"]
    assert cal["accuracy"] == plain["accuracy"]                          # the argmax does not move
    assert not (cal["tables"]["hist"][1] == plain["tables"]["hist"][1]).all()      # the entropy score is the calibrated distribution's


def test_temperature_none_and_one_change_nothing(setup):
    import torch
    m, img_dir, gt_glob, pairs, _ = setup
    base = m.evaluate_reliability(img_dir, gt_glob)
    for T in (None, 1.0, 1):
        r = m.evaluate_reliability(img_dir, gt_glob, temperature=T)
        assert all((r["tables"][k] == base["tables"][k]).all() for k in NAMES)
    img = pairs[0][0][None]
    sm = m.predict(img, argmax=False)
    am = m.predict(img)
    for T in (None, 1.0):
        assert (m.predict(img, argmax=False, temperature=T).view(np.uint32) == sm.view(np.uint32)).all()
    # argmax output: the same ids, and the model's profile shows the same launches as a call without the argument
    m.engine.profile(True)
    try:
        m.engine.profile_reset()
        assert (m.predict(img) == am).all()
        want = {k: v["launches"] for k, v in m.engine.profile_results().items()}
        m.engine.profile_reset()
        assert (m.predict(img, temperature=2.0) == am).all()
        got = {k: v["launches"] for k, v in m.engine.profile_results().items()}
    finally:
        m.engine.profile(False)
    assert got == want and not any("temperature" in k for k in got)
    # with the softmax asked for, host and device inputs are calibrated alike, in place on the device, and the argmax stays
    q = m.predict(img, argmax=False, temperature=2.0)
    qd = m.predict(torch.from_numpy(img).cuda(), argmax=False, temperature=2.0)
    assert isinstance(q, np.ndarray) and (qd.cpu().numpy().view(np.uint32) == q.view(np.uint32)).all()
    q64, _ = ts.apply_numpy(sm, 0.5, np.float64)
    q32, _ = ts.apply_numpy(sm, 0.5, np.float32)
    assert np.abs(q - q64).max() <= 8 * np.abs(q32 - q64).max()
    top = np.sort(q64, -1)
    sure = top[..., -1] - top[..., -2] > 1e-5
    assert (q.argmax(-1)[sure] == am[sure]).all()


def test_refusals(setup):
    m, img_dir, gt_glob, _, _ = setup
    with pytest.raises(ValueError):
        m.evaluate_reliability(img_dir, gt_glob, samples=4, temperature=2.0)
    with pytest.raises(ValueError):
        m.evaluate_reliability(img_dir, gt_glob, temperature=0.0)
    with pytest.raises(ValueError):
        m.predict(np.zeros((1, 32, 32, 3), np.uint8), argmax=False, temperature=1000.0)
    with pytest.raises(ValueError):
        m.fit_temperature(img_dir, gt_glob, candidates=33)
    with pytest.raises(ValueError):
        m.fit_temperature(img_dir, gt_glob, passes=0)
    with pytest.raises(ValueError):
        m.fit_temperature(img_dir, gt_glob, t_min=2.0, t_max=1.0)
    with pytest.raises(ValueError):
        m.fit_temperature(img_dir, os.path.join(img_dir, "nothing", "*.png"))


def test_routes_and_averaged_weights(setup):
    m, img_dir, gt_glob, pairs, _ = setup
    lut = rel.cityscapes_lut()
    for kw in (dict(scales=(1.0,), flip=True), dict(crf=True)):
        res = m.fit_temperature(img_dir, gt_glob, passes=2, candidates=8, **kw)
        assert res["route"] == "passes" and 0.125 <= res["temperature"] <= 8.0 and res["nllAfter"] <= res["nllBefore"]
        # the first sweep's table entry at T = 1 is the NLL of the route's own softmax
        p = np.concatenate([m.predict(img[None], argmax=False, **kw).reshape(-1, 20) for img, _, _ in pairs])
        t = np.concatenate([lut[g.reshape(-1)] for _, g, _ in pairs]).astype(np.int64)
        host = dict(prob=p[t != 255], t=t[t != 255])
        tol, _ = bar(host, [1.0])
        assert abs(res["nllBefore"] - exact_nll(host["prob"], host["t"], 1.0)) <= tol
        cal = m.evaluate_reliability(img_dir, gt_glob, temperature=res["temperature"], **kw)
        assert cal["route"] == "passes" and list(cal["scores"]) == ["maxProb"]
        tol, _ = bar(host, [res["temperature"]])
        assert abs(cal["nll"] - res["nllAfter"]) <= tol + 0.5 / ts.Q_NLL
    before = m.fit_temperature(img_dir, gt_glob, candidates=8)
    m.engine.set_ema(0.9, warmup=False)                                # no step taken: the shadow is the parameters
    try:
        with m.averaged_weights():
            inside = m.fit_temperature(img_dir, gt_glob, candidates=8)
        after = m.fit_temperature(img_dir, gt_glob, candidates=8)
    finally:
        m.engine.set_ema(None)
    assert inside == before and after == before


def test_save_and_load_round_trip_the_temperature(setup, tmp_path):
    from fcn8s_tensorflow_amd.fcn8s import FCN8s
    m, img_dir, gt_glob, _, _ = setup
    m.temperature = None
    m.save(str(tmp_path / "plain"), 'saved_model', tags=['default'], force_save=True)
    d = [x for x in (tmp_path / "plain").iterdir() if x.is_dir()][0]
    meta = json.load(open(str(d / "fcn8s_meta.json")))
    assert sorted(meta) == ['fc6_ksize', 'format', 'global_step', 'num_classes', 'tags', 'widths']      # the parent's file, key for key
    T = m.fit_temperature(img_dir, gt_glob, candidates=8)["temperature"]
    m.save(str(tmp_path / "fitted"), 'saved_model', tags=['default'], force_save=True)
    d2 = [x for x in (tmp_path / "fitted").iterdir() if x.is_dir()][0]
    meta2 = json.load(open(str(d2 / "fcn8s_meta.json")))
    assert meta2.pop("temperature") == T and meta2 == meta
    m2 = FCN8s(model_load_dir=str(d2), tags=['default'])
    m1 = FCN8s(model_load_dir=str(d), tags=['default'])
    try:
        assert m2.temperature == T and m1.temperature is None
    finally:
        m1.close(); m2.close()


def test_json_file_holds_the_same_numbers(setup, tmp_path):
    m, img_dir, gt_glob, _, _ = setup
    path = str(tmp_path / "out" / "temperature.json")
    res = m.fit_temperature(img_dir, gt_glob, candidates=8, json_path=path)
    back = json.load(open(path))
    assert back == json.loads(json.dumps(res)) and back["temperature"] == res["temperature"] and back["route"] == "single"
    assert [tuple(c) for c in back["candidates"][0]] == res["candidates"][0]
