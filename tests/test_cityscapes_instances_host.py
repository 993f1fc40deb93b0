"""The instance-level half of the official Cityscapes scoring (iIoU; cityscapes_eval.py) against what the reference evaluator
itself computed with evalInstLevelScore on (tests/golden/make_cityscapes_instances.py -> cityscapes_instances.npz).  CPU only: the
NumPy route.  Integers and float64 sums are the evaluator's own operations in its own order, so every comparison is an equality."""
import json
import math
import os

import numpy as np
import pytest

from fcn8s_tensorflow_amd import cityscapes_eval as ce

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
FIELDS = ["tp", "fn", "tpWeighted", "fnWeighted"]


@pytest.fixture(scope="module")
def gold():
    return np.load(os.path.join(GOLD, "cityscapes_instances.npz"))


def same_float(a, b):
    return (math.isnan(a) and math.isnan(b)) or a == b


def check_against_fixture(res, d, conf):
    np.testing.assert_array_equal(conf, d["conf"])
    assert list(d["stat_fields"]) == FIELDS
    st = res["instStats"]
    assert list(st["classes"]) == list(d["inst_class_names"]) and list(st["categories"]) == list(d["inst_cat_names"])
    np.testing.assert_array_equal(np.array([[st["classes"][c][f] for f in FIELDS] for c in d["inst_class_names"]], np.float64), d["inst_class_stats"])
    np.testing.assert_array_equal(np.array([[st["categories"][c][f] for f in FIELDS] for c in d["inst_cat_names"]], np.float64), d["inst_cat_stats"])
    assert list(res["classScores"]) == list(d["class_names"]) == list(res["classInstScores"])
    assert list(res["categoryScores"]) == list(d["cat_names"]) == list(res["categoryInstScores"])
    for key, names, want in (("classScores", "class_names", "class_scores"), ("classInstScores", "class_names", "class_inst_scores"),
                             ("categoryScores", "cat_names", "cat_scores"), ("categoryInstScores", "cat_names", "cat_inst_scores")):
        for n, w in zip(d[names], d[want]):
            assert same_float(res[key][n], float(w)), (key, n, res[key][n], float(w))
    for k, w in zip(("averageScoreClasses", "averageScoreInstClasses", "averageScoreCategories", "averageScoreInstCategories"), d["averages"]):
        assert same_float(res[k], float(w)), (k, res[k], float(w))
    assert sum(not math.isnan(v) for v in res["classInstScores"].values()) == 8
    assert sum(not math.isnan(v) for v in res["categoryInstScores"].values()) == 2


def write_triples(d, root, swap_instances=None):
    from PIL import Image
    gts = []
    os.makedirs(os.path.join(root, "results", "sub"), exist_ok=True)
    for n, nm in enumerate(d["names"]):
        city = str(nm).split("_")[0]
        os.makedirs(os.path.join(root, "gtFine", "val", city), exist_ok=True)
        gf = os.path.join(root, "gtFine", "val", city, str(nm) + "_gtFine_labelIds.png")
        Image.fromarray(d["gts"][n]).save(gf)
        inst = d["insts"][n] if swap_instances is None else swap_instances(n, d["insts"][n])
        if inst is not None:
            Image.fromarray(inst).save(ce.instance_file_of(gf))
        Image.fromarray(d["preds"][n]).save(os.path.join(root, "results", "sub", str(nm) + "_leftImg8bit.png"))
        gts.append(gf)
    return gts


def test_tables_match_reference(gold):
    assert dict(zip((str(k) for k in gold["avg_class_size_names"]), (float(v) for v in gold["avg_class_size"]))) == ce.AVG_CLASS_SIZE
    assert list(ce.new_instance_stats()["classes"]) == list(gold["inst_class_names"])
    assert [",".join(str(i) for i in ids) for ids in ce.INSTANCE_CATEGORY_TO_IDS.values()] == list(gold["inst_cat_label_ids"])
    assert list(ce.INSTANCE_CATEGORY_TO_IDS) == list(gold["inst_cat_names"])


def test_numpy_path_equals_reference_evaluator(gold):
    d = gold
    ev = ce.PixelLevelEvaluator(instance_level=True)
    for n in range(len(d["names"])):                                     # label-id predictions, image by image as the evaluator walks them
        ev.add(d["preds"][n], d["gts"][n], d["insts"][n], pred_is_train_ids=False)
    check_against_fixture(ev.results(), d, ev.conf)
    # the same through train ids (what `predict` returns): the fixture's predictions only hold label 0 and evaluated labels
    ev2 = ce.PixelLevelEvaluator(instance_level=True)
    for n in range(len(d["names"])):
        tid = ce.IDS_TO_TRAINIDS_ARRAY[d["preds"][n]].astype(np.int64)
        np.testing.assert_array_equal(ce.TRAINIDS_TO_IDS_ARRAY[tid], d["preds"][n])
        ev2.add(tid, d["gts"][n], d["insts"][n])
    check_against_fixture(ev2.results(), d, ev2.conf)
    # a stack in one call = the images one by one
    ev3 = ce.PixelLevelEvaluator(instance_level=True)
    ev3.add(d["preds"], d["gts"], d["insts"], pred_is_train_ids=False)
    check_against_fixture(ev3.results(), d, ev3.conf)


def test_entry_tables_cover_the_cases(gold):
    d = gold
    tabs = [ce.instance_entries_numpy(d["preds"][n], d["insts"][n]) for n in range(len(d["names"]))]
    assert tabs[0].shape == (0, 4)                                                        # an image without any instance
    for t in tabs:
        assert (np.diff(t[:, 0]) > 0).all() and (t[:, 1] > 0).all() and (t[:, 2] <= t[:, 3]).all() and (t[:, 3] <= t[:, 1]).all()
        assert not np.isin(t[:, 0] // 1000, [29, 30]).any()                               # caravan / trailer instances are skipped
    assert 24000 in tabs[1][:, 0] and {26001, 26002} <= set(tabs[1][:, 0]) and 26001 in tabs[2][:, 0]
    row = tabs[4][tabs[4][:, 0] == 28007][0]
    assert row[2] == 0 and row[3] == 0                                                    # tp = 0
    row = tabs[5][tabs[5][:, 0] == 27999][0]
    assert 0 < row[2] < row[3] == row[1]                                                  # predicted as another vehicle
    assert (d["insts"][3] == 29000).any() and (d["preds"] == 0).any()


def test_file_pairs_and_directory(gold, tmp_path):
    d = gold
    gts = write_triples(d, str(tmp_path))
    preds = [ce.find_prediction(os.path.join(str(tmp_path), "results"), g) for g in gts]
    res = ce.evaluate_file_pairs(preds, gts, instance_level=True)
    check_against_fixture(res, d, res["confMatrix"])
    assert res["nbPixels"] == d["gts"].size
    res = ce.evaluate_directory(os.path.join(str(tmp_path), "gtFine", "val", "*", "*_gtFine_labelIds.png"), os.path.join(str(tmp_path), "results"),
                                instance_level=True)
    check_against_fixture(res, d, res["confMatrix"])


def test_instance_level_off_is_todays_result(gold, tmp_path):
    d = gold
    gts = write_triples(d, str(tmp_path), swap_instances=lambda n, a: None)               # no instance files at all: not needed
    search = os.path.join(str(tmp_path), "gtFine", "val", "*", "*_gtFine_labelIds.png")
    res = ce.evaluate_directory(search, os.path.join(str(tmp_path), "results"))
    assert sorted(res) == ["averageScoreCategories", "averageScoreClasses", "categoryScores", "classScores", "confMatrix", "nbPixels"]
    np.testing.assert_array_equal(res["confMatrix"], d["conf"])
    for n, w in zip(d["class_names"], d["class_scores"]):
        assert same_float(res["classScores"][n], float(w))
    for n, w in zip(d["cat_names"], d["cat_scores"]):
        assert same_float(res["categoryScores"][n], float(w))
    assert res["averageScoreClasses"] == float(d["averages"][0]) and res["averageScoreCategories"] == float(d["averages"][2])
    ev = ce.PixelLevelEvaluator()
    ev.add(ce.IDS_TO_TRAINIDS_ARRAY[d["preds"]].astype(np.int64), d["gts"])
    assert sorted(ev.results()) == ["averageScoreCategories", "averageScoreClasses", "categoryScores", "classScores"]
    np.testing.assert_array_equal(ev.conf, d["conf"])
    # ... and with instance_level the missing file is an error that names it
    with pytest.raises(ValueError, match="instanceIds"):
        ce.evaluate_directory(search, os.path.join(str(tmp_path), "results"), instance_level=True)


def test_errors(gold, tmp_path):
    d = gold
    bad = d["insts"][1].copy(); bad[0, :3] = 7005                                         # road has no instances: the evaluator's KeyError
    with pytest.raises(ValueError, match="7005"):
        ce.instance_entries_numpy(d["preds"][1], bad)
    bad = d["insts"][1].copy(); bad[5, 5] = 34001                                         # no such label
    with pytest.raises(ValueError, match="34001"):
        ce.PixelLevelEvaluator(instance_level=True).add(d["preds"][1], d["gts"][1], bad, pred_is_train_ids=False)
    ok = d["insts"][1].copy(); ok[0, :3] = 1000; ok[1, :3] = 1001; ok[2, :3] = 9004; ok[3, :3] = 18000   # not > 1000 / ignored labels: skipped
    np.testing.assert_array_equal(ce.instance_entries_numpy(d["preds"][1], ok)[:, 0],
                                  np.unique(ok[(ok > 1000) & np.isin(ok // 1000, ce.INSTANCE_LABEL_IDS)]))
    with pytest.raises(ValueError):
        ce.PixelLevelEvaluator(instance_level=True).add(d["preds"][1], d["gts"][1], pred_is_train_ids=False)   # no instance map
    with pytest.raises(ValueError):
        ce.PixelLevelEvaluator(instance_level=True).add(d["preds"][1], d["gts"][1], d["insts"][1][:, :-1], pred_is_train_ids=False)
    with pytest.raises(ValueError, match="Unknown label"):
        g = d["gts"][1].copy(); g[0, 0] = 34
        ce.PixelLevelEvaluator(instance_level=True).add(d["preds"][1], g, d["insts"][1], pred_is_train_ids=False)
    # files: an instance map of another size, a bad value
    gts = write_triples(d, str(tmp_path / "a"), swap_instances=lambda n, a: a[:, :-2] if n == 2 else a)
    preds = [ce.find_prediction(os.path.join(str(tmp_path / "a"), "results"), g) for g in gts]
    with pytest.raises(ValueError, match="not equal"):
        ce.evaluate_file_pairs(preds, gts, instance_level=True)

    def spoil(n, a):
        a = a.copy()
        if n == 4:
            a[0, 0] = 23001
        return a
    gts = write_triples(d, str(tmp_path / "b"), swap_instances=spoil)
    preds = [ce.find_prediction(os.path.join(str(tmp_path / "b"), "results"), g) for g in gts]
    with pytest.raises(ValueError, match="23001"):
        ce.evaluate_file_pairs(preds, gts, instance_level=True)


def test_result_json_round_trip(gold, tmp_path):
    d = gold
    gts = write_triples(d, str(tmp_path))
    res = ce.evaluate_directory(os.path.join(str(tmp_path), "gtFine", "val", "*", "*_gtFine_labelIds.png"), os.path.join(str(tmp_path), "results"),
                                instance_level=True)
    path = os.path.join(str(tmp_path), "out", "resultPixelLevelSemanticLabeling.json")
    ce.write_result_json(res, path)
    back = json.load(open(path))
    assert sorted(back) == list(d["json_keys"])                                           # createResultDict's keys (no perImageScores: evalPixelAccuracy is off)
    np.testing.assert_array_equal(np.array(back["confMatrix"], np.int64), d["conf"])
    assert list(back["labels"]) == sorted(str(n) for n in d["label_names"])               # sort_keys, as writeDict2JSON
    assert {k: back["labels"][k] for k in back["labels"]} == dict(zip((str(n) for n in d["label_names"]), (int(i) for i in d["label_ids"])))
    for n, w in zip(d["prior_names"], d["priors"]):
        assert same_float(back["priors"][str(n)], float(w))
    for key, names, want in (("classScores", "class_names", "class_scores"), ("classInstScores", "class_names", "class_inst_scores"),
                             ("categoryScores", "cat_names", "cat_scores"), ("categoryInstScores", "cat_names", "cat_inst_scores")):
        assert sorted(back[key]) == sorted(str(n) for n in d[names])
        for n, w in zip(d[names], d[want]):
            assert same_float(back[key][str(n)], float(w)), (key, n)
    for k, w in zip(("averageScoreClasses", "averageScoreInstClasses", "averageScoreCategories", "averageScoreInstCategories"), d["averages"]):
        assert same_float(back[k], float(w))
    with pytest.raises(ValueError):
        ce.result_dict(ce.PixelLevelEvaluator().results())
