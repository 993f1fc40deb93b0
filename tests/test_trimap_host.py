"""The boundary measures of cityscapes_eval.py (trimap IoU, boundary F-score) on the CPU: the NumPy route of fcn8s_op_boundary_pair's
definition (include/fcn8s_hip.h) against tables that SciPy's exact distance transform produced (tests/golden/make_trimap_cases.py ->
trimap_cases.npz), against hand-counted cases, and the scores built from the tables.  Every comparison of counts is an equality."""
import math
import os

import numpy as np
import pytest

from fcn8s_tensorflow_amd import cityscapes_eval as ce

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def fixture_cases():
    d = np.load(os.path.join(GOLD, "trimap_cases.npz"))
    return [(d["G%d" % i], d["P%d" % i], int(d["R%d" % i]), d["rings%d" % i], d["bprec%d" % i], d["brec%d" % i]) for i in range(int(d["n"]))]


def hand_cases():
    """(G, P, R, {(ring index, gt, pred): count} of rings, {(ring, class): count} of bprec, the same of brec); everything else is 0."""
    out = []
    # a 4 x 4 square of label 8 predicted inside a constant ground truth 7: no true boundary anywhere, so every pixel is in ring R + 1, the
    # square's 12 contour pixels and the 16 pixels of 7 that touch it are unmatched predicted contour pixels, and there is nothing to recall
    R = 4
    G = np.full((20, 20), 7, np.uint8); P = G.copy(); P[5:9, 5:9] = 8
    out.append((G, P, R, {(R, 7, 7): 384, (R, 7, 8): 16}, {(R + 1, 8): 12, (R + 1, 7): 16}, {}))
    # a vertical edge between 7 (columns 0..9) and 8 (10..19), six rows, predicted two columns too far right; R = 3
    G = np.full((6, 20), 7, np.uint8); G[:, 10:] = 8
    P = np.full((6, 20), 7, np.uint8); P[:, 12:] = 8
    out.append((G, P, 3,
                {(0, 7, 7): 6, (0, 8, 7): 6, (1, 7, 7): 6, (1, 8, 7): 6, (2, 7, 7): 6, (2, 8, 8): 6, (3, 7, 7): 42, (3, 8, 8): 42},
                {(2, 7): 6, (2, 8): 6}, {(2, 7): 6, (2, 8): 6}))
    # one pixel of person (24) in the middle of a 5 x 5 road, missed by the prediction; R = 2: the pixel and its 4 neighbours (d2 = 1) are in
    # ring 1, the 4 diagonal (d2 = 2) and the 4 straight (d2 = 4) ones in ring 2, the 8 + 4 at d2 = 5 and 8 beyond
    G = np.full((5, 5), 7, np.uint8); G[2, 2] = 24
    P = np.full((5, 5), 7, np.uint8)
    out.append((G, P, 2, {(0, 24, 7): 1, (0, 7, 7): 4, (1, 7, 7): 8, (2, 7, 7): 12}, {}, {(3, 24): 1, (3, 7): 4}))
    return out


def dense(shape, entries):
    a = np.zeros(shape, np.int64)
    for k, v in entries.items():
        a[k] = v
    return a


def voronoi_pair(rng, H, W, cells=10, salt=0.02):
    ys, xs = np.mgrid[:H, :W]
    py, px = rng.integers(0, H, cells), rng.integers(0, W, cells)
    lab = rng.integers(0, 34, cells)
    G = lab[np.argmin((ys[..., None] - py) ** 2 + (xs[..., None] - px) ** 2, -1)].astype(np.uint8)
    P = np.roll(G, (int(rng.integers(-3, 4)), int(rng.integers(-3, 4))), (0, 1)).copy()
    n = rng.random((H, W)) < salt
    P[n] = rng.integers(0, 34, int(n.sum()))
    return G, P


def test_numpy_route_equals_scipy_fixture():
    cases = fixture_cases()
    assert len(cases) >= 8 and {c[2] for c in cases} == {1, 3, 8, 16}
    for G, P, R, rings, bprec, brec in cases:
        r, bp, br = ce.boundary_counts_numpy(P, G, R, pred_is_train_ids=False)
        assert r.dtype == np.int64 and r.shape == (R + 1, 34, 34) and bp.shape == (R + 2, 34) and br.shape == (R + 2, 34)
        np.testing.assert_array_equal(r, rings); np.testing.assert_array_equal(bp, bprec); np.testing.assert_array_equal(br, brec)


def test_hand_counted_cases():
    for G, P, R, rings, bprec, brec in hand_cases():
        r, bp, br = ce.boundary_counts_numpy(P, G, R, pred_is_train_ids=False)
        np.testing.assert_array_equal(r, dense((R + 1, 34, 34), rings))
        np.testing.assert_array_equal(bp, dense((R + 2, 34), bprec))
        np.testing.assert_array_equal(br, dense((R + 2, 34), brec))


def test_numpy_route_equals_fresh_scipy_computation():
    pytest.importorskip("scipy.ndimage")
    import importlib.util
    spec = importlib.util.spec_from_file_location("make_trimap_cases", os.path.join(GOLD, "make_trimap_cases.py"))
    mk = importlib.util.module_from_spec(spec); spec.loader.exec_module(mk)
    rng = np.random.default_rng(77)
    for H, W, R in ((31, 44, 2), (57, 39, 5), (40, 83, 11), (18, 18, 16)):
        G, P = voronoi_pair(rng, H, W)
        for a, b in zip(ce.boundary_counts_numpy(P, G, R, pred_is_train_ids=False), mk.tables_scipy(G, P, R)):
            np.testing.assert_array_equal(a, b)


def test_rings_sum_to_the_confusion_matrix_and_train_ids_map_back():
    rng = np.random.default_rng(3)
    G, _ = voronoi_pair(rng, 48, 65)
    train = rng.integers(0, 20, (48, 65))
    train[10:30, 5:40] = ce.IDS_TO_TRAINIDS_ARRAY[G[10:30, 5:40]]
    rings, bprec, brec = ce.boundary_counts_numpy(train, G, 5)
    ids = ce.TRAINIDS_TO_IDS_ARRAY[train]
    np.testing.assert_array_equal(rings.sum(0), ce.confusion_add(np.zeros((34, 34), np.int64), G, ids))
    for a, b in zip((rings, bprec, brec), ce.boundary_counts_numpy(ids, G, 5, pred_is_train_ids=False)):
        np.testing.assert_array_equal(a, b)
    assert bprec.sum() == ce.boundary_set(ids).sum() and brec.sum() == ce.boundary_set(G).sum()
    # a stack is the sum of its images
    G2, P2 = voronoi_pair(rng, 48, 65)
    both = ce.boundary_counts_numpy(np.stack([ids, P2]), np.stack([G, G2]), 5, pred_is_train_ids=False)
    for a, b, c in zip(both, (rings, bprec, brec), ce.boundary_counts_numpy(P2, G2, 5, pred_is_train_ids=False)):
        np.testing.assert_array_equal(a, b + c)


def test_prefix_property():
    """The band of width r from a call with radius R is the band from a call with radius r; the same for the tolerances of bprec / brec."""
    rng = np.random.default_rng(4)
    G, P = voronoi_pair(rng, 52, 71, cells=7)
    R = 16
    big = ce.boundary_counts_numpy(P, G, R, pred_is_train_ids=False)
    for r in (1, 2, 3, 7, 12):
        small = ce.boundary_counts_numpy(P, G, r, pred_is_train_ids=False)
        np.testing.assert_array_equal(small[0][:r], big[0][:r])
        np.testing.assert_array_equal(small[0][r], big[0][r:].sum(0))
        for a, b in zip(small[1:], big[1:]):
            np.testing.assert_array_equal(a[:r + 1], b[:r + 1])
            np.testing.assert_array_equal(a[r + 1], b[r + 1:].sum(0))


def _eq(a, b):
    return (math.isnan(a) and math.isnan(b)) or a == b


def test_trimap_scores_are_the_evaluators_scores_on_the_bands():
    rng = np.random.default_rng(5)
    G, P = voronoi_pair(rng, 60, 90, cells=20, salt=0.1)
    R = 6
    rings, _, _ = ce.boundary_counts_numpy(P, G, R, pred_is_train_ids=False)
    s = ce.trimap_scores(rings)
    assert len(s["trimapScoreClasses"]) == R + 1 and len(s["trimapScoreCategories"]) == R + 1
    conf = ce.confusion_add(np.zeros((34, 34), np.int64), G, P)
    full = {ce.ID_TO_NAME[l]: ce.iou_for_label(l, conf) for l in range(34)}
    assert list(s["trimapClassScores"]) == list(full)
    for name, v in full.items():
        assert _eq(s["trimapClassScores"][name][R], v)
    assert _eq(s["trimapScoreClasses"][R], ce.score_average(full))
    assert _eq(s["trimapScoreCategories"][R], ce.score_average({c: ce.iou_for_category(c, conf) for c in ce.CATEGORY_TO_IDS}))
    for r in (1, 3):
        band = rings[:r].sum(0)
        assert _eq(s["trimapScoreClasses"][r - 1], ce.score_average({l: ce.iou_for_label(l, band) for l in range(34)}))
        assert _eq(s["trimapClassScores"]["road"][r - 1], ce.iou_for_label(7, band))
    assert not math.isnan(s["trimapScoreClasses"][0])
    with pytest.raises(ValueError):
        ce.trimap_scores(np.zeros((3, 34, 33)))


def test_boundary_f_scores_on_hand_tables():
    R = 2
    bprec = np.zeros((R + 2, 34), np.int64); brec = np.zeros((R + 2, 34), np.int64)
    bprec[:, 7] = (1, 2, 1, 4); brec[:, 7] = (2, 0, 2, 0)            # road: P = 1/8, 3/8, 4/8; R = 2/4, 2/4, 4/4
    bprec[:, 8] = (0, 0, 0, 5); brec[:, 8] = (0, 0, 0, 3)            # sidewalk: nothing matched: P = R = 0, F undefined
    bprec[:, 26] = (3, 0, 0, 0)                                      # car: predicted contours, no true ones: recall undefined
    brec[:, 24] = (0, 1, 0, 0)                                       # person: the other way round
    bprec[:, 0] = (9, 0, 0, 0); brec[:, 0] = (9, 0, 0, 0)            # unlabeled is not evaluated
    s = ce.boundary_f_scores(bprec, brec)
    road = s["boundaryClassScores"]["road"]
    assert road["precision"] == [1 / 8, 3 / 8, 4 / 8] and road["recall"] == [2 / 4, 2 / 4, 4 / 4]
    assert road["f"] == [2 * (1 / 8) * (2 / 4) / (1 / 8 + 2 / 4), 2 * (3 / 8) * (2 / 4) / (3 / 8 + 2 / 4), 2 * (4 / 8) * 1.0 / (4 / 8 + 1.0)]
    side = s["boundaryClassScores"]["sidewalk"]
    assert side["precision"] == [0.0] * 3 and side["recall"] == [0.0] * 3 and all(math.isnan(f) for f in side["f"])
    car = s["boundaryClassScores"]["car"]
    assert car["precision"] == [1.0] * 3 and all(math.isnan(x) for x in car["recall"] + car["f"])
    person = s["boundaryClassScores"]["person"]
    assert person["recall"] == [0.0, 1.0, 1.0] and all(math.isnan(x) for x in person["precision"] + person["f"])
    assert all(math.isnan(x) for k in ("precision", "recall", "f") for x in s["boundaryClassScores"]["unlabeled"][k])
    assert all(math.isnan(x) for x in s["boundaryClassScores"]["sky"]["f"])
    assert s["boundaryFScoreClasses"] == road["f"]                   # the only label with a defined F
    assert list(s["boundaryClassScores"]) == [ce.ID_TO_NAME[l] for l in range(34)]
    empty = ce.boundary_f_scores(np.zeros((3, 34), np.int64), np.zeros((3, 34), np.int64))
    assert all(math.isnan(x) for x in empty["boundaryFScoreClasses"])
    with pytest.raises(ValueError):
        ce.boundary_f_scores(bprec, brec[:3])


def test_bad_arguments_and_ids_are_refused():
    G = np.full((4, 4), 7, np.uint8)
    for R in (0, 17, 2.5):
        with pytest.raises(ValueError, match="boundary_radius"):
            ce.boundary_counts_numpy(G, G, R, pred_is_train_ids=False)
    with pytest.raises(ValueError, match="train ids"):
        ce.boundary_counts_numpy(np.full((4, 4), 20), G, 2)
    with pytest.raises(ValueError, match="label ids"):
        ce.boundary_counts_numpy(np.full((4, 4), 34), G, 2, pred_is_train_ids=False)
    with pytest.raises(ValueError, match="Unknown label"):
        ce.boundary_counts_numpy(G, np.full((4, 4), 40, np.uint8), 2, pred_is_train_ids=False)
    with pytest.raises(ValueError):
        ce.boundary_counts_numpy(G, G[:3], 2, pred_is_train_ids=False)
    # the definition's fourth clause, which the device tests lean on: an id out of range is a boundary and is counted in `bad` only
    Gb = np.full((3, 5), 7, np.uint8); Gb[1, 2] = ce.BAD_ID
    rings, bprec, brec, bad = ce.boundary_tables_numpy(Gb, np.full((3, 5), 7, np.uint8), 1)
    assert bad == 1 and rings.sum() == 14 and rings[0, 7, 7] == 4 and rings[1, 7, 7] == 10
    assert bprec.sum() == 0 and brec.sum() == 4 and brec[2, 7] == 4


def test_evaluator_without_a_radius_is_todays():
    rng = np.random.default_rng(6)
    G, _ = voronoi_pair(rng, 30, 40)
    train = rng.integers(0, 20, (30, 40))
    ev = ce.PixelLevelEvaluator(); ev.add(train, G)
    assert sorted(ev.results()) == ["averageScoreCategories", "averageScoreClasses", "categoryScores", "classScores"]
    evb = ce.PixelLevelEvaluator(boundary_radius=3); evb.add(train, G); evb.add(train[::-1], G[::-1])
    res = evb.results()
    assert sorted(set(res) - set(ev.results())) == sorted(ce.BOUNDARY_RESULT_KEYS)
    assert res["boundaryRadius"] == 3 and len(res["trimapScoreClasses"]) == 3 and len(res["trimapScoreCategories"]) == 3
    assert len(res["boundaryFScoreClasses"]) == 4 and all(len(v) == 3 for v in res["trimapClassScores"].values())
    one = ce.boundary_counts_numpy(train, G, 3)
    two = ce.boundary_counts_numpy(train[::-1], G[::-1], 3)
    for k, a, b in zip(("trimapRings", "boundaryPrecisionCounts", "boundaryRecallCounts"), one, two):
        np.testing.assert_array_equal(res[k], a + b)
    np.testing.assert_array_equal(res["trimapRings"].sum(0), evb.conf)
    for k in ("classScores", "categoryScores"):
        assert all(_eq(res[k][n], ce.PixelLevelEvaluator.results(evb)[k][n]) for n in res[k])
    with pytest.raises(ValueError, match="boundary_radius"):
        ce.PixelLevelEvaluator(boundary_radius=0)


def test_evaluate_directory_with_a_radius_equals_the_tables_summed_by_hand(tmp_path):
    from PIL import Image
    rng = np.random.default_rng(9)
    names = ["aachen_000000_000019", "aachen_000001_000019", "bonn_000002_000019"]
    R = 4
    sums = None
    for nm in names:
        city = nm.split("_")[0]
        (tmp_path / "gtFine" / city).mkdir(parents=True, exist_ok=True); (tmp_path / "results").mkdir(exist_ok=True)
        G, P = voronoi_pair(rng, 33, 58)
        Image.fromarray(G).save(tmp_path / "gtFine" / city / (nm + "_gtFine_labelIds.png"))
        Image.fromarray(G.astype(np.uint16)).save(tmp_path / "gtFine" / city / (nm + "_gtFine_instanceIds.png"))
        Image.fromarray(P).save(tmp_path / "results" / (nm + "_leftImg8bit.png"))
        t = ce.boundary_counts_numpy(P, G, R, pred_is_train_ids=False)
        sums = t if sums is None else tuple(a + b for a, b in zip(sums, t))
    search = str(tmp_path / "gtFine" / "*" / "*_gtFine_labelIds.png")
    plain = ce.evaluate_directory(search, str(tmp_path / "results"))
    assert not set(plain) & set(ce.BOUNDARY_RESULT_KEYS)
    for inst_level in (False, True):
        res = ce.evaluate_directory(search, str(tmp_path / "results"), instance_level=inst_level, boundary_radius=R)
        for k, a in zip(("trimapRings", "boundaryPrecisionCounts", "boundaryRecallCounts"), sums):
            np.testing.assert_array_equal(res[k], a)
        np.testing.assert_array_equal(res["trimapRings"].sum(0), res["confMatrix"])
        np.testing.assert_array_equal(res["confMatrix"], plain["confMatrix"])
        assert res["trimapScoreClasses"] == [x for x in ce.trimap_scores(sums[0])["trimapScoreClasses"][:R]] or \
            all(_eq(a, b) for a, b in zip(res["trimapScoreClasses"], ce.trimap_scores(sums[0])["trimapScoreClasses"][:R]))
        f = ce.boundary_f_scores(sums[1], sums[2])["boundaryFScoreClasses"]
        assert all(_eq(a, b) for a, b in zip(res["boundaryFScoreClasses"], f)) and len(f) == R + 1
    # the result file keeps the evaluator's layout and carries the new keys only when they exist
    import json
    ce.write_result_json(res, str(tmp_path / "with.json"))
    ce.write_result_json(ce.evaluate_directory(search, str(tmp_path / "results"), instance_level=True), str(tmp_path / "without.json"))
    w = json.load(open(tmp_path / "with.json")); wo = json.load(open(tmp_path / "without.json"))
    assert sorted(set(w) - set(wo)) == sorted(ce.BOUNDARY_RESULT_KEYS) and not set(wo) - set(w)
    assert w["trimapRings"] == sums[0].tolist() and w["boundaryRadius"] == R
