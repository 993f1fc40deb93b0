"""The NumPy route and the host half of panoptic quality (fcn8s_tensorflow_amd/panoptic.py; include/fcn8s_hip.h at fcn8s_op_panoptic_pair)
against tests/golden/panoptic_cases.npz, which a SciPy / dict-counting route of its own wrote (tests/golden/make_panoptic_cases.py): the
tables and the integer counts with ==, the float64 sums within 1e-10.  No GPU."""
import json
import os

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
# 1e-10 absolute, the bound set for these sums: iou_sum adds terms <= 1 in float64, and a sum of k such terms, in any order, is off by at
# most (k - 1) * k * 2^-53 -- a fixture case has under 100 matches per class, so under 1.1e-12; PQ / SQ / RQ are quotients of it by numbers
# >= 1/2, then means over at most 19 classes.
TOL = 1e-10


def _module():
    from fcn8s_tensorflow_amd import panoptic
    return panoptic


@pytest.fixture(scope="module")
def golden():
    z = np.load(os.path.join(HERE, "golden", "panoptic_cases.npz"))
    return z, json.loads(bytes(z["index"]).decode())


def _images(z, name):
    pred, inst = z[name + ".pred"], z[name + ".inst"]
    return (pred, inst) if pred.ndim == 3 else (pred[None], inst[None])


def test_fixture_holds_the_cases(golden):
    z, index = golden
    names = [c["name"] for c in index]
    for want in ("hand_iou_half", "hand_void_inside", "hand_crowd_fp", "hand_crowd_fn", "hand_class_mismatch", "hand_pred_void", "hand_touching",
                 "single_1x1", "scene_1x17", "scene_3x5", "scene_33x65", "scene_64x128", "batch2_48x80"):
        assert want in names
    car, truck, road = 14, 15, 1
    g = lambda name, what: z["%s.c4.%s" % (name, what)]
    # what the hand-made cases were made for, one rule each
    assert g("hand_iou_half", "tp")[car] == 0 and g("hand_iou_half", "fp")[car] == 1 and g("hand_iou_half", "fn")[car] == 1      # 0.5 is no match
    assert g("hand_void_inside", "tp")[car] == 1 and g("hand_void_inside", "iou_sum")[car] == 1.0                               # void lifts 4 / 8 to 4 / 4
    assert g("hand_crowd_fp", "fp")[car] == 0 and g("hand_crowd_fp", "tp")[car] == 0 and g("hand_crowd_fp", "fn")[car] == 0
    assert g("hand_crowd_fn", "fn").sum() == 0 and g("hand_crowd_fn", "tp")[road] == 1
    assert g("hand_class_mismatch", "tp")[[car, truck]].sum() == 0 and g("hand_class_mismatch", "fp")[truck] == 1 and g("hand_class_mismatch", "fn")[car] == 1
    assert g("hand_pred_void", "rows0").tolist() == [[0, 1, 2], [1, 1, 8]]
    assert g("hand_touching", "tp")[car] == 1 and g("hand_touching", "fn")[car] == 1 and g("hand_touching", "fp")[car] == 0
    assert g("hand_touching", "iou_sum")[car] == 0.75
    assert g("scene_33x65", "bad")[0] == 3 and g("scene_64x128", "bad")[0] == 3
    rows = g("scene_64x128", "rows0")
    assert ((rows[:, 1] >> 30) == 1).any() and (rows[:, 1] == 0).any() and (rows[:, 0] == 0).any() and ((rows[:, 0] >> 31) == 1).sum() > 20
    assert g("scene_64x128", "tp")[12:].sum() > 0 and g("scene_64x128", "fp")[12:].sum() > 20
    assert not np.array_equal(z["scene_64x128.c4.rows0"], z["scene_64x128.c8.rows0"])
    assert index[names.index("batch2_48x80")]["images"] == 2
    assert os.path.getsize(os.path.join(HERE, "golden", "panoptic_cases.npz")) < 200 * 1024


def test_numpy_route_equals_the_fixture(golden):
    P = _module()
    z, index = golden
    for case in index:
        name = case["name"]
        pred, inst = z[name + ".pred"], z[name + ".inst"]
        for conn in (4, 8):
            rows, bad = P.pair_rows_numpy(pred, inst, conn)
            if pred.ndim == 2:
                rows, bad = [rows], [bad]
            assert len(rows) == case["images"]
            for k, r in enumerate(rows):
                want = z["%s.c%d.rows%d" % (name, conn, k)]
                assert r.dtype == np.int64 and r.shape == want.shape and np.array_equal(r, want), (name, conn, k)
                assert int(r[:, 2].sum()) == pred.size // case["images"] - bad[k]                     # the counts sum to the pixels minus bad
            assert list(bad) == z["%s.c%d.bad" % (name, conn)].tolist(), (name, conn)
            # the other spellings of the same maps
            r2, b2 = P.pair_rows_numpy(pred.astype(np.int64), inst.view(np.int16), conn)
            r2 = [r2] if pred.ndim == 2 else r2
            assert all(np.array_equal(a, b) for a, b in zip(rows, r2))


def test_label_id_predictions(golden):
    from fcn8s_tensorflow_amd import cityscapes_eval as ce
    P = _module()
    z, _ = golden
    for name in ("scene_33x65", "hand_touching", "batch2_48x80"):
        pred, inst = z[name + ".pred"], z[name + ".inst"]
        ids = ce.TRAINIDS_TO_IDS_ARRAY[pred]
        a, ba = P.pair_rows_numpy(pred, inst, 8)
        b, bb = P.pair_rows_numpy(ids, inst, 8, pred_is_train_ids=False)
        if pred.ndim == 2:
            a, b = [a], [b]
        assert all(np.array_equal(x, y) for x, y in zip(a, b)) and np.array_equal(ba, bb)
    # a label id beyond 33 and a train id beyond 19 are bad pixels; ignored label ids are void
    inst = np.full((2, 3), 7, np.uint16)
    rows, bad = P.pair_rows_numpy(np.array([[7, 7, 34], [9, 29, 7]], np.uint8), inst, 4, pred_is_train_ids=False)
    assert bad == 1 and rows.tolist() == [[0, 1, 2], [1, 1, 3]]
    rows, bad = P.pair_rows_numpy(np.array([[1, 1, 20], [0, -1, 1]], np.int64), inst, 4)
    assert bad == 2 and rows.tolist() == [[0, 1, 1], [1, 1, 3]]


def test_scores_equal_the_fixture(golden):
    P = _module()
    z, index = golden
    for case in index:
        name = case["name"]
        for conn in (4, 8):
            key = "%s.c%d." % (name, conn)
            stats = P.new_stats()
            for k in range(case["images"]):
                P.stats_add(stats, z[key + "rows%d" % k])
            for what in ("tp", "fp", "fn"):
                assert stats[what].dtype == np.int64 and np.array_equal(stats[what], z[key + what]), (key, what)
            assert np.abs(stats["iou_sum"] - z[key + "iou_sum"]).max() <= TOL, key
            res = P.results(stats)
            for g, group in enumerate(("All", "Things", "Stuff")):
                got = res["panopticQuality"][group]
                assert got["n"] == int(z[key + "pqn"][g]), (key, group)
                for j, what in enumerate(("pq", "sq", "rq")):
                    want = float(z[key + "pq"][g, j])
                    assert (np.isnan(want) and np.isnan(got[what])) or abs(got[what] - want) <= TOL, (key, group, what, got[what], want)
            assert np.array_equal(res["panopticTp"], stats["tp"]) and np.array_equal(res["panopticFp"], stats["fp"]) and np.array_equal(res["panopticFn"], stats["fn"])
            per = res["panopticClassScores"]
            assert list(per)[0] == "road" and list(per)[-1] == "bicycle" and len(per) == 19
            for c, (cname, s) in enumerate(per.items(), start=1):
                assert (s["tp"], s["fp"], s["fn"]) == (int(stats["tp"][c]), int(stats["fp"][c]), int(stats["fn"][c]))
                if s["tp"] + s["fp"] + s["fn"]:
                    assert abs(s["pq"] - s["sq"] * s["rq"]) <= TOL                                      # PQ = SQ x RQ


def test_keys():
    P = _module()
    assert P.pred_keys([0, 5, 11, 12, 19, 20, -1], [9, 9, 9, 9, 3, 9, 9]).tolist() == [0, 5, 11, (1 << 31) | 9 << 5 | 12, (1 << 31) | 3 << 5 | 19, -1, -1]
    assert P.gt_keys([0, 7, 26, 26001, 26999, 33000, 29001, 4, 34, 999, 34000, 65535]).tolist() == \
        [0, 1, (1 << 30) | 14, (1 << 31) | 1 << 5 | 14, (1 << 31) | 999 << 5 | 14, (1 << 31) | 19, 0, 0, -1, -1, -1, -1]
    assert P.key_class([(1 << 31) | 999 << 5 | 14, (1 << 30) | 14, 11, 0]).tolist() == [14, 14, 11, 0]
    assert P.key_is_crowd([(1 << 30) | 14, (1 << 31) | (1 << 25) << 5 | 14, 14]).tolist() == [True, False, False]
    assert P.crowd_key(14) == (1 << 30) | 14
    assert P.default_slots(1, 1) == 256 and P.default_slots(1024, 2048) == 1 << 18 and P._pow2_at_least(3) == 4 and P._pow2_at_least(1) == 1


def test_numpy_route_refuses():
    P = _module()
    pred, inst = np.zeros((4, 4), np.uint8), np.zeros((4, 4), np.uint16)
    for conn in (0, 6, "4"):
        with pytest.raises(ValueError):
            P.pair_rows_numpy(pred, inst, conn)
    with pytest.raises(ValueError):
        P.pair_rows_numpy(pred, inst[:3], 4)
    with pytest.raises(ValueError):
        P.pair_rows_numpy(pred.astype(np.float32), inst, 4)
    with pytest.raises(ValueError):
        P.pair_rows_numpy(pred[0], inst[0], 4)


def _maps(golden, name):
    from fcn8s_tensorflow_amd import cityscapes_eval as ce
    z, _ = golden
    pred, inst = z[name + ".pred"], z[name + ".inst"].copy()
    inst[inst == 40005] = 7                                          # the evaluator refuses a label beyond 33
    lab = np.where(inst < 1000, inst, inst // 1000).astype(np.uint8)
    return ce, pred, lab, inst


def test_evaluator_numpy_route(golden):
    P = _module()
    ce, pred, gt, inst = _maps(golden, "scene_33x65")
    base = ce.PixelLevelEvaluator(instance_level=True)
    base.add(pred, gt, inst)
    parent = base.results()
    none = ce.PixelLevelEvaluator(instance_level=True, panoptic=None)
    none.add(pred, gt, inst)
    assert list(none.results()) == list(parent) and not any(k.startswith("panoptic") for k in parent)     # the parent's keys, in its order
    for conn in (4, 8):
        ev = ce.PixelLevelEvaluator(instance_level=True, panoptic=conn)
        ev.add(pred, gt, inst)
        ev.add(ce.TRAINIDS_TO_IDS_ARRAY[pred], gt, inst, pred_is_train_ids=False)
        res = ev.results()
        assert list(res)[:len(parent)] == list(parent) and set(res) - set(parent) == set(ce.PANOPTIC_RESULT_KEYS)
        stats = P.new_stats()
        rows, bad = P.pair_rows_numpy(pred, inst, conn)
        assert bad == 0
        P.stats_add(stats, rows); P.stats_add(stats, rows)
        want = P.results(stats)
        same = lambda a, b: json.dumps(a) == json.dumps(b)                                            # (NaN == NaN; bit for bit otherwise)
        assert res["panopticConnectivity"] == conn and same(res["panopticQuality"], want["panopticQuality"])
        assert same(res["panopticClassScores"], want["panopticClassScores"]) and np.array_equal(res["panopticFp"], want["panopticFp"])
    # a label beyond 33 in the instance map is refused, as the other measures refuse what they cannot score
    z, _ = golden
    ev = ce.PixelLevelEvaluator(instance_level=True, panoptic=4)
    bad_inst = inst.copy(); bad_inst[0, 0] = 500
    with pytest.raises(ValueError):
        ev.add(pred, gt, bad_inst)
    for wrong in (True, 6, "4", 0):
        with pytest.raises(ValueError):
            ce.PixelLevelEvaluator(instance_level=True, panoptic=wrong)
    with pytest.raises(ValueError):
        ce.PixelLevelEvaluator(instance_level=False, panoptic=4)


def test_result_json_carries_the_keys_only_when_they_exist(golden, tmp_path):
    ce, pred, gt, inst = _maps(golden, "scene_33x65")
    out = {}
    for tag, conn in (("off", None), ("on", 8)):
        ev = ce.PixelLevelEvaluator(instance_level=True, panoptic=conn)
        ev.add(pred, gt, inst)
        res = ev.results(); res["confMatrix"] = ev.conf
        path = str(tmp_path / (tag + ".json"))
        ce.write_result_json(res, path)
        with open(path) as f:
            out[tag] = json.load(f)
    assert set(out["on"]) - set(out["off"]) == set(ce.PANOPTIC_RESULT_KEYS)
    assert all(json.dumps(out["on"][k], sort_keys=True) == json.dumps(out["off"][k], sort_keys=True) for k in out["off"])
    assert out["on"]["panopticConnectivity"] == 8
    assert out["on"]["panopticQuality"]["Stuff"]["n"] >= 1 and len(out["on"]["panopticFp"]) == 20
