"""FCN8s.fit_pseudo_label_thresholds and FCN8s.predict_and_export_pseudo_labels on the small synthetic model of test_temperature_facade_gpu.py
and three synthetic images of 64 x 96, 80 x 64 and 96 x 128 in a temporary city directory (80 is no multiple of 32: the single-pass route
takes images of any size, as `evaluate_reliability`'s does).  Everything is compared with `==`: the exported PNGs against
`pseudo_label.tables_numpy` on the softmax the same route returns, and the export's kept counts against the tail sums of the fit's
histograms -- the exact identity of the definition, which also shows that the two sweeps predict the same bits."""
import json
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from fcn8s_tensorflow_amd import cityscapes_eval as ce, pseudo_label as PL  # noqa: E402
from tests.test_temperature_facade_gpu import make_model  # noqa: E402

SIZES = [(64, 96), (80, 64), (96, 128)]
M = PL.BINS


def stem(i):
    return "aachen_%06d_000019" % i


@pytest.fixture(scope="module")
def setup(tmp_path_factory):
    from PIL import Image
    root = tmp_path_factory.mktemp("pseudo_label")
    img_dir = root / "leftImg8bit" / "train_extra" / "aachen"
    os.makedirs(img_dir)
    rng = np.random.default_rng(29)
    imgs = []
    for i, (h, w) in enumerate(SIZES):
        img = rng.integers(0, 256, (h, w, 3), dtype=np.uint8)
        Image.fromarray(img).save(str(img_dir / (stem(i) + "_leftImg8bit.png")))
        imgs.append(img)
    m = make_model()
    yield m, root, str(root / "leftImg8bit" / "train_extra"), imgs
    m.close()


def dev(img):
    return torch.from_numpy(np.array(img)[None]).cuda()


def single_softmax(m, img):
    """The single-pass route's softmax [H,W,C] as NumPy: one sample without dropout, which is `predict(argmax=False)` bit for bit where that
    takes the size."""
    sm = m.engine.predict_mc(dev(img), samples=1, keep_prob=1.0, argmax=False, entropy=False, mutual_information=False)[0][0].cpu().numpy()
    if img.shape[0] % 32 == 0 and img.shape[1] % 32 == 0:
        assert (m.predict(dev(img), argmax=False)[0].cpu().numpy().view(np.uint32) == sm.view(np.uint32)).all()
    return sm


def read(results_dir, i):
    from PIL import Image
    a = np.array(Image.open(os.path.join(str(results_dir), stem(i) + "_leftImg8bit.png")))
    assert a.dtype == np.uint8 and a.shape == SIZES[i]
    return a


def kept_of(res):
    return np.array([r["kept"] for r in res["classes"]], np.int64)


def test_fit_then_export_on_the_single_pass_route(setup, tmp_path):
    m, root, img_dir, imgs = setup
    sms = [single_softmax(m, img) for img in imgs]
    fit = m.fit_pseudo_label_thresholds(img_dir, portion=0.3, json_path=str(tmp_path / "fit.json"))
    assert fit["route"] == "single" and fit["nbImages"] == 3
    host = [PL.tables_numpy(s) for s in sms]
    assert (fit["hist"] == sum(h[1] for h in host)).all() and (fit["counts"] == sum(h[2] for h in host)).all() and (fit["misc"] == 0).all()
    assert fit["hist"].sum() == sum(h * w for h, w in SIZES) and (fit["hist"].sum(1) > 0).sum() >= 3, "the model predicts too few classes for this test"
    thr, bins = PL.thresholds_from_hist(fit["hist"], 0.3)
    assert (fit["thresholds"] == thr).all() and (fit["bins"] == bins).all() and (m.pseudo_label_thresholds == thr).all()
    assert json.load(open(str(tmp_path / "fit.json")))["bins"] == bins.tolist()
    out = tmp_path / "pl"
    res = m.predict_and_export_pseudo_labels(str(out), img_dir, json_path=str(tmp_path / "export.json"))
    assert res["route"] == "single" and res["nbImages"] == 3 and sorted(os.listdir(str(out))) == [stem(i) + "_leftImg8bit.png" for i in range(3)]
    for i, s in enumerate(sms):
        lab, _, counts, misc = PL.tables_numpy(s, thresholds=thr)
        png = read(out, i)
        assert (png == lab).all(), i
        per = res["images"][i]
        assert per["file"] == stem(i) + "_leftImg8bit.png" and per["kept"] == counts[:, 0].sum() and per["dropped"] == counts[:, 1].sum()
        assert (png == 255).sum() == per["dropped"] + per["badRows"] and per["passedThrough"] == 0      # ignore_id exactly where a pixel was dropped
    # the second sweep keeps exactly the tail of the first one's histograms
    assert (kept_of(res) == PL.tail_sums(fit["hist"], bins)).all()
    assert [r["kept"] for r in fit["summary"]["classes"]] == kept_of(res).tolist()
    assert 0 < res["totals"]["kept"] < res["totals"]["predicted"] == sum(h * w for h, w in SIZES)
    assert json.load(open(str(tmp_path / "export.json")))["totals"] == json.loads(json.dumps(res["totals"]))
    # explicit thresholds, another ignore id, and no overwrite of the directory's other files
    open(str(out / "keep.txt"), "w").write("x")
    res2 = m.predict_and_export_pseudo_labels(str(out), img_dir, thresholds=np.full(20, 0.5, np.float32), ignore_id=77, overwrite_existing=False)
    assert os.path.isfile(str(out / "keep.txt"))
    for i, s in enumerate(sms):
        assert (read(out, i) == PL.tables_numpy(s, thresholds=np.full(20, 0.5, np.float32), ignore_id=77)[0]).all()
    assert (res2["thresholds"] == 0.5).all()


def test_the_scales_and_flip_route_and_the_temperature(setup, tmp_path):
    m, root, img_dir, imgs = setup
    kw = dict(scales=(1.0, 0.75), flip=True)
    fit = m.fit_pseudo_label_thresholds(img_dir, portion=0.5, t_min=0.3, **kw)
    assert fit["route"] == "passes" and (fit["bins"] >= 308).all()
    res = m.predict_and_export_pseudo_labels(str(tmp_path / "pl"), img_dir, **kw)
    for i, img in enumerate(imgs):
        sm = m.predict(dev(img), argmax=False, **kw)[0].cpu().numpy()
        assert (read(tmp_path / "pl", i) == PL.tables_numpy(sm, thresholds=fit["thresholds"])[0]).all()
    free = PL.thresholds_from_hist(fit["hist"], 0.5)[1]
    bites = fit["bins"] != free
    assert (kept_of(res)[~bites] == PL.tail_sums(fit["hist"], free)[~bites]).all() and (kept_of(res) <= PL.tail_sums(fit["hist"], free)).all()
    assert (kept_of(res) == PL.tail_sums(fit["hist"], fit["bins"])).all()
    cal = m.fit_pseudo_label_thresholds(img_dir, portion=0.5, temperature=2.0)
    assert cal["route"] == "single" and not (cal["hist"] == m.fit_pseudo_label_thresholds(img_dir, portion=0.5)["hist"]).all()
    res = m.predict_and_export_pseudo_labels(str(tmp_path / "cal"), img_dir, thresholds=cal["thresholds"], temperature=2.0)
    assert (kept_of(res) == PL.tail_sums(cal["hist"], cal["bins"])).all()


def test_the_monte_carlo_route_gates_on_the_mutual_information(setup, tmp_path):
    m, root, img_dir, imgs = setup
    mc = lambda img: m.engine.predict_mc(dev(img), samples=4, keep_prob=0.5, sample_offset=0, argmax=False, entropy=False, mutual_information=True)
    mi_max = float(np.median(mc(imgs[0])[2].cpu().numpy()))
    fit = m.fit_pseudo_label_thresholds(img_dir, portion=0.4, samples=4, mi_max=mi_max)
    assert fit["route"] == "mc" and 0 < fit["misc"][2] < sum(h * w for h, w in SIZES) and fit["hist"].sum() + fit["misc"][2] == sum(h * w for h, w in SIZES)
    res = m.predict_and_export_pseudo_labels(str(tmp_path / "pl"), img_dir, samples=4, mi_max=mi_max)
    for i, img in enumerate(imgs):
        prob, _, mi = mc(img)
        lab, _, counts, misc = PL.tables_numpy(prob[0].cpu().numpy(), thresholds=fit["thresholds"], score=mi[0].cpu().numpy(), score_max=mi_max)
        assert (read(tmp_path / "pl", i) == lab).all() and res["images"][i]["droppedByScore"] == misc[2] > 0
    assert (kept_of(res) == PL.tail_sums(fit["hist"], fit["bins"])).all() and res["totals"]["droppedByScore"] == fit["misc"][2]
    free = m.predict_and_export_pseudo_labels(str(tmp_path / "free"), img_dir, samples=4)                 # no gate: nothing is dropped by score
    assert free["totals"]["droppedByScore"] == 0 and free["totals"]["kept"] >= res["totals"]["kept"]


def test_base_maps_are_completed_and_label_ids_are_written(setup, tmp_path):
    from PIL import Image
    m, root, img_dir, imgs = setup
    thr = m.fit_pseudo_label_thresholds(img_dir, portion=0.5)["thresholds"]
    rng = np.random.default_rng(31)
    coarse = tmp_path / "gtCoarse" / "aachen"
    os.makedirs(str(coarse))
    bases = []
    for i, (h, w) in enumerate(SIZES):
        b = ce.TRAINIDS_TO_IDS_ARRAY[rng.integers(0, 20, (h, w))]
        b[rng.random((h, w)) < 0.5] = 255
        b[0, :4] = 254                                                   # the ignore id of the call, already in the base: passed through like any label
        Image.fromarray(b).save(str(coarse / (stem(i) + "_gtCoarse_labelIds.png")))
        bases.append(b)
    glob_ = str(tmp_path / "gtCoarse" / "*" / "*_gtCoarse_labelIds.png")
    res = m.predict_and_export_pseudo_labels(str(tmp_path / "pl"), img_dir, id_space='label', ignore_id=254, base_search=glob_, base_fill=255)
    for i, img in enumerate(imgs):
        png, b = read(tmp_path / "pl", i), bases[i]
        assert (png[b != 255] == b[b != 255]).all()                      # the labelled pixels are the base's, byte for byte
        lab, _, counts, misc = PL.tables_numpy(single_softmax(m, img), thresholds=thr, out_ids=ce.TRAINIDS_TO_IDS_ARRAY, ignore_id=254, base=b, base_fill=255)
        assert (png == lab).all() and res["images"][i]["passedThrough"] == (b != 255).sum() == misc[1]
        fill = b == 255
        assert ((png[fill] == 254) | np.isin(png[fill], ce.TRAINIDS_TO_IDS_ARRAY)).all() and (png[fill] == 254).sum() == res["images"][i]["dropped"]
    # id_space='label' alone: the train-id export mapped through the table
    m.predict_and_export_pseudo_labels(str(tmp_path / "ids"), img_dir, id_space='label')
    m.predict_and_export_pseudo_labels(str(tmp_path / "train"), img_dir)
    for i in range(3):
        t = read(tmp_path / "train", i)
        assert (read(tmp_path / "ids", i) == np.where(t == 255, 255, ce.TRAINIDS_TO_IDS_ARRAY[np.minimum(t, 19)])).all()
    os.remove(str(coarse / (stem(1) + "_gtCoarse_labelIds.png")))
    with pytest.raises(ValueError, match="no base label map"):
        m.predict_and_export_pseudo_labels(str(tmp_path / "pl2"), img_dir, base_search=glob_, base_fill=255)


def test_resize_brings_the_labels_back_to_the_files_size(setup, tmp_path):
    from PIL import Image
    m, root, img_dir, imgs = setup
    thr = np.full(20, 0.4, np.float32)
    m.predict_and_export_pseudo_labels(str(tmp_path / "pl"), img_dir, thresholds=thr, resize=(64, 64))
    for i, img in enumerate(imgs):
        small = np.asarray(Image.fromarray(img).resize((64, 64), Image.BILINEAR))
        lab = PL.tables_numpy(single_softmax(m, small), thresholds=thr)[0]
        assert (read(tmp_path / "pl", i) == np.asarray(Image.fromarray(lab).resize((SIZES[i][1], SIZES[i][0]), Image.NEAREST))).all()


def test_refusals_and_the_frozen_state_after_an_exception(setup, tmp_path):
    from PIL import Image
    m, root, img_dir, imgs = setup
    saved, m.pseudo_label_thresholds = m.pseudo_label_thresholds, None
    with pytest.raises(ValueError, match="no thresholds"):
        m.predict_and_export_pseudo_labels(str(tmp_path / "x"), img_dir)
    m.pseudo_label_thresholds = saved
    thr = np.full(20, 0.5, np.float32)
    for kw in (dict(samples=4, temperature=2.0), dict(samples=4, flip=True), dict(mi_max=0.1), dict(samples=4, mi_max=float('nan')), dict(temperature=0.0)):
        with pytest.raises(ValueError):
            m.fit_pseudo_label_thresholds(img_dir, **kw)
        with pytest.raises(ValueError):
            m.predict_and_export_pseudo_labels(str(tmp_path / "x"), img_dir, thresholds=thr, **kw)
    for kw in (dict(portion=0.0), dict(portion=1.1), dict(t_min=0.9, t_max=0.1)):
        with pytest.raises(ValueError):
            m.fit_pseudo_label_thresholds(img_dir, **kw)
    for kw in (dict(ignore_id=256), dict(id_space='ids'), dict(base_fill=255), dict(base_search="x"), dict(thresholds=np.zeros(19, np.float32)),
               dict(base_search=str(tmp_path / "*"), base_fill=255, resize=(64, 64))):
        with pytest.raises(ValueError):
            m.predict_and_export_pseudo_labels(str(tmp_path / "x"), img_dir, **{**dict(thresholds=thr), **kw})
    with pytest.raises(ValueError):
        m.fit_pseudo_label_thresholds(str(tmp_path / "nothing"))
    # a file that breaks inside the loop: the frozen state is the caller's again, whichever it was
    broken = tmp_path / "broken" / "aachen"
    os.makedirs(str(broken))
    Image.fromarray(imgs[0]).save(str(broken / "aachen_000000_000019_leftImg8bit.png"))
    open(str(broken / "aachen_000001_000019_leftImg8bit.png"), "w").write("no image")
    for frozen in (False, True):
        m.engine.freeze(frozen)
        with pytest.raises(Exception):
            m.fit_pseudo_label_thresholds(str(tmp_path / "broken"))
        assert bool(m.engine.get_option("frozen")) == frozen
        with pytest.raises(Exception):
            m.predict_and_export_pseudo_labels(str(tmp_path / "y"), str(tmp_path / "broken"), thresholds=thr)
        assert bool(m.engine.get_option("frozen")) == frozen
        m.fit_pseudo_label_thresholds(img_dir)
        assert bool(m.engine.get_option("frozen")) == frozen
    m.engine.freeze(False)


def test_a_later_train_reads_the_exported_maps_through_the_ordinary_batch_generator(setup, tmp_path):
    from fcn8s_tensorflow_amd.batch_generator import BatchGenerator
    _, root, img_dir, imgs = setup
    m = make_model()
    try:
        m.fit_pseudo_label_thresholds(img_dir, portion=0.5)
        res = m.predict_and_export_pseudo_labels(str(tmp_path / "pl" / "aachen"), img_dir)
        assert 0 < res["totals"]["dropped"] and 0 < res["totals"]["kept"]
        gen = BatchGenerator(image_dirs=[img_dir], image_file_extension="png", ground_truth_dirs=[str(tmp_path / "pl")],
                             image_name_split_separator=".png", ground_truth_suffix="", check_existence=True, num_classes=20)
        assert gen.get_num_files() == 3
        g = gen.generate(batch_size=2, convert_to_one_hot=False, resize=(64, 96), shuffle=False)
        ids = g.next_ids()[1]
        assert ids.shape == (2, 64, 96) and (ids == 255).any() and (ids[ids != 255] < 20).all()
        m.train(g, epochs=1, steps_per_epoch=2, learning_rate_schedule=lambda s: 1e-4, keep_prob=1.0, record_summaries=False)
        assert m.g_step == 2 and np.isfinite(m.training_loss)
    finally:
        m.close()
