"""Instance-level AP on the host (fcn8s_tensorflow_amd/instances.py) against tests/golden/instance_ap_cases.npz, which
tests/golden/make_instance_ap_cases.py records by running the reference's instance-level evaluator on inputs made without this package.
No GPU."""
import os

import numpy as np
import pytest

from fcn8s_tensorflow_amd import instances as ins

GOLD = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "instance_ap_cases.npz"))
CASES = [str(c) for c in GOLD["case_names"]]


def case(name):
    return (int(GOLD[name + "_connectivity"]), GOLD[name + "_labels"], GOLD[name + "_prob"], GOLD[name + "_inst"])


def flatten(images):
    """The fixture's flattening of the match lists (make_instance_ap_cases.py: flatten), from `image_instances`' two lists."""
    ints, confs = [], []
    for preds, gts in images:
        ints.append(len(preds))
        for p in preds:
            ints += [p["labelID"], p["pixelCount"], p["voidIntersection"], len(p["matchedGt"])]
            for v, gpix, inter in p["matchedGt"]:
                ints += [v, gpix, inter]
            confs.append(p["confidence"])
        mine = [g for g in gts if g["labelID"] in ins.INST_LABEL_IDS]
        ints.append(len(mine))
        for g in mine:
            ints += [g["instID"], g["labelID"], g["pixelCount"], len(g["matchedPred"])]
            for pi, inter in g["matchedPred"]:
                ints += [pi, inter]
    return np.array(ints, np.int64), np.array(confs, np.float64)


def same(a, b):
    """== with NaN equal to NaN."""
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return a.shape == b.shape and bool(((a == b) | (np.isnan(a) & np.isnan(b))).all())


def stats_of(name):
    conn, labels, prob, inst = case(name)
    rows, bad = ins.pair_rows_numpy(prob, labels, inst, connectivity=conn)
    st = ins.new_stats()
    for r in rows:
        ins.stats_add(st, r)
    return st, rows, bad


def test_the_label_tables():
    assert ins.INST_LABEL_IDS == [24, 25, 26, 27, 28, 31, 32, 33]
    assert ins.INST_LABEL_NAMES == [str(n) for n in GOLD["inst_label_names"]]
    assert ins.VOID_IDS.tolist() == [0, 1, 2, 3, 4, 5, 6, 9, 10, 14, 15, 16, 18, 29, 30]
    assert ins.OVERLAPS.shape == (10,) and ins.OVERLAPS[0] == 0.5


@pytest.mark.parametrize("name", CASES)
def test_rows_equal_the_recorded_rows(name):
    conn, labels, prob, inst = case(name)
    rows, bad = ins.pair_rows_numpy(prob, labels, inst, connectivity=conn)
    for n, r in enumerate(rows):
        assert r.dtype == np.int64 and np.array_equal(r, GOLD["%s_rows%d" % (name, n)])
        assert r[:, 2].sum() == labels[n].size
        one, bad1 = ins.pair_rows_numpy(prob[n], labels[n], inst[n], connectivity=conn)           # one image: the same rows
        assert np.array_equal(one, r) and np.array_equal(bad1, bad[n])
    if name.startswith("scene"):
        assert bad[0].tolist() == [21, 4] and bad[1].tolist() == [0, 0]                            # 21 labels >= 20; NaN, -0.25, 1.5 and inf
        free, _ = ins.pair_rows_numpy(prob[0], labels[0], None, connectivity=conn)                # without ground truth: v = 0, the same instances
        assert (free[:, 1] == 0).all() and np.array_equal(np.unique(free[:, 0]), np.unique(rows[0][:, 0]))
        assert free[:, 3].sum() == rows[0][:, 3].sum()


@pytest.mark.parametrize("name", CASES)
def test_image_instances_equal_the_reference_match_lists(name):
    _st, rows, _bad = stats_of(name)
    ints, confs = flatten([ins.image_instances(r) for r in rows])
    assert np.array_equal(ints, GOLD[name + "_matches"])
    assert np.array_equal(confs, GOLD[name + "_confidences"])                                     # ==: one correctly rounded division of exact integers


@pytest.mark.parametrize("name", CASES)
def test_results_equal_the_reference_ap(name):
    """== holds, NaN for NaN: every count is an integer, precision and recall are single divisions, the step widths are exact halves of
    differences, and the final dot product and the means are NumPy's own, taken over the same values in the same order."""
    st, _rows, _bad = stats_of(name)
    res = ins.results(st)
    assert res["ap"].shape == (8, 10)
    assert same(res["ap"], GOLD[name + "_ap"])
    av = res["averages"]
    got = [av["allAp"], av["allAp50%"]] + [av["classes"][k][f] for k in ins.INST_LABEL_NAMES for f in ("ap", "ap50%")]
    assert same(got, GOLD[name + "_averages"])
    assert res["resultApMatrix"][0][2][0] == res["ap"][2, 0] or np.isnan(res["ap"][2, 0])
    assert res["instLabels"] == ins.INST_LABEL_NAMES and res["minRegionSizes"] == [100] and res["overlaps"] == ins.OVERLAPS.tolist()


def test_nan_averages_are_skipped_like_nanmean():
    st, _rows, _bad = stats_of("scene_c4")
    res = ins.results(st)
    ap = res["ap"]
    assert np.isnan(ap).any() and not np.isnan(ap).all()
    assert res["averages"]["allAp"] == np.nanmean(ap) and np.isfinite(res["averages"]["allAp"])
    assert res["averages"]["allAp50%"] == np.nanmean(ap[:, 0])
    assert np.isnan(res["averages"]["classes"]["train"]["ap"])
    empty = ins.results(ins.new_stats())                                                          # nothing at all: every mean is NaN, no exception
    assert np.isnan(empty["ap"]).all() and np.isnan(empty["averages"]["allAp"])


def test_min_instance_pixels_drops_predictions_not_ground_truth():
    _st, rows, _bad = stats_of("scene_c4")
    all_p, all_g = ins.image_instances(rows[1])
    big_p, big_g = ins.image_instances(rows[1], min_instance_pixels=2)
    assert len(all_p) > len(big_p) == sum(1 for p in all_p if p["pixelCount"] >= 2)
    assert [g["pixelCount"] for g in all_g] == [g["pixelCount"] for g in big_g]
    st_all, st_big = ins.new_stats(), ins.new_stats()
    for r in rows:
        ins.stats_add(st_all, r); ins.stats_add(st_big, r, min_instance_pixels=2)
    assert ins.results(st_big)["ap"][0, 0] > ins.results(st_all)["ap"][0, 0]                      # the one-pixel persons were false positives


@pytest.mark.parametrize("name", ["scene_c4", "scene_c8", "no_things"])
def test_export_read_back_equals_the_in_memory_route(name, tmp_path):
    from PIL import Image
    from fcn8s_tensorflow_amd import regions
    conn, labels, prob, inst = case(name)
    st, rows, _bad = stats_of(name)
    txts, gts = [], []
    for n in range(labels.shape[0]):
        comp, _area = regions.components_numpy(labels[n], conn)
        free, _ = ins.pair_rows_numpy(prob[n], labels[n], None, connectivity=conn)                # the export route has no ground truth
        stem = "aachen_%06d_000019" % n
        txts.append(ins.write_export(str(tmp_path / "results"), stem + "_leftImg8bit", comp, free))
        gt = tmp_path / "gt" / (stem + "_gtFine_instanceIds.png")
        os.makedirs(gt.parent, exist_ok=True)
        Image.fromarray(inst[n]).save(gt)
        gts.append(str(gt))
        back = ins.read_export(txts[-1])
        preds, _g = ins.image_instances(rows[n])
        assert [(lab, conf) for _m, lab, conf in back] == [(p["labelID"], p["confidence"]) for p in preds]      # repr reads back exactly
        if back:
            cover = np.sum([m for m, _l, _c in back], axis=0)
            assert np.array_equal(cover, ((labels[n] >= 12) & (labels[n] < 20)).astype(cover.dtype))             # disjoint, and exactly the thing pixels
    res_file, res_mem = ins.evaluate_directory(txts, gts), ins.results(st)
    assert same(res_file["ap"], res_mem["ap"]) and same(res_file["ap"], GOLD[name + "_ap"])
    assert str(res_file["averages"]) == str(res_mem["averages"])
    ins.write_result_json(res_file, str(tmp_path / "out" / "resultInstanceLevelSemanticLabeling.json"))
    import json
    written = json.load(open(tmp_path / "out" / "resultInstanceLevelSemanticLabeling.json"))
    assert sorted(written) == ["averages", "instLabels", "minRegionSizes", "overlaps", "resultApMatrix"]
    assert sorted(written["averages"]) == ["allAp", "allAp50%", "classes"] and sorted(written["averages"]["classes"]["car"]) == ["ap", "ap50%"]


def test_refusals():
    conn, labels, prob, inst = case("no_things")
    with pytest.raises(ValueError):
        ins.pair_rows_numpy(prob[0][:, :, :19], labels[0], inst[0])                               # fewer than 20 classes
    with pytest.raises(ValueError):
        ins.pair_rows_numpy(prob[0], labels[0], inst[0], connectivity=6)
    with pytest.raises(ValueError):
        ins.pair_rows_numpy(prob[0].astype(np.float64), labels[0], inst[0])
    bad = inst[0].copy(); bad[0, 0] = 34001
    rows, _ = ins.pair_rows_numpy(prob[0], labels[0], bad)
    with pytest.raises(ValueError, match="Unknown label"):
        ins.image_instances(rows)                                                                 # v // 1000 > 33 is refused for the image
    with pytest.raises(ValueError, match="ascending"):
        ins.image_instances(rows[::-1])
