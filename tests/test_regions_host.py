"""The NumPy route of the regions definition (fcn8s_tensorflow_amd/regions.py; include/fcn8s_hip.h at fcn8s_op_regions_label) against
tests/golden/region_cases.npz, which a SciPy route of its own wrote (tests/golden/make_region_cases.py): every table with ==.  No GPU."""
import json
import os

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))


def _module():
    from fcn8s_tensorflow_amd import regions
    return regions


@pytest.fixture(scope="module")
def golden():
    z = np.load(os.path.join(HERE, "golden", "region_cases.npz"))
    return z, json.loads(bytes(z["index"]).decode())


def test_fixture_holds_the_cases(golden):
    z, index = golden
    names = [c["name"] for c in index]
    for want in ("voronoi_37x53_s05", "voronoi_61x95_s10", "voronoi_70x131_s30", "spiral_97x101", "comb_67x130", "checker_33x47",
                 "constant_19x70", "noise_33x47", "column_50x1", "row_1x77", "single_1x1", "tiles_64x128", "tiles_128x256", "hand_rules",
                 "hand_tie", "batch2_45x70"):
        assert want in names
    # what the cases were made for
    assert len(np.unique(z["spiral_97x101.c4.comp"])) == 2
    assert len(np.unique(z["comb_67x130.c4.comp"])) == 1 + 65 and z["comb_67x130.c4.comp"][66, 129] == 0
    assert len(np.unique(z["checker_33x47.c4.comp"])) == 33 * 47 and len(np.unique(z["checker_33x47.c8.comp"])) == 2
    assert np.array_equal(z["constant_19x70.c4.m5000.r1.out"], z["constant_19x70.L"]) and z["constant_19x70.c4.m5000.r1.stats"].tolist() == [[1, 1, 0, 0]]
    L, out = z["hand_tie.L"], z["hand_tie.c4.m8.r1.out"]
    assert (out[:, 4] == 1).all() and (out[L != 2] == L[L != 2]).all()                       # equal areas: the smaller id
    L, r1, r2 = z["hand_rules.L"], z["hand_rules.c4.m16.r1.out"], z["hand_rules.c4.m16.r2.out"]
    assert r1[4, 4] == 3 and r1[3, 3] == 1 and r2[4, 4] == 1                                 # small inside small: a round later
    assert r1[9, 12] == 1 and r1[0, 23] == 1 and r1[12, 0] == 1
    pc = z["hand_rules.c4.perclass.r2.out"]
    assert pc[4, 4] == 3 and pc[3, 3] == 1 and pc[9, 12] == 1 and pc[12, 0] == 4 and pc[7, 18] == 6      # 0 = never small; area == threshold is not small
    b = z["batch2_45x70.c4.comp"]
    assert b[1].max() < 45 * 70 and b[1][0, 0] == 0                                          # the second image's ids are its own
    assert os.path.getsize(os.path.join(HERE, "golden", "region_cases.npz")) < 200 * 1024


def test_numpy_route_equals_the_fixture(golden):
    R = _module()
    z, index = golden
    for case in index:
        name, L = case["name"], z[case["name"] + ".L"]
        for conn in (4, 8):
            comp, area = R.components_numpy(L, conn)
            assert comp.dtype == np.int32 and area.dtype == np.int32 and comp.shape == L.shape
            assert np.array_equal(comp, z["%s.c%d.comp" % (name, conn)]), (name, conn)
            assert np.array_equal(area, z["%s.c%d.area" % (name, conn)]), (name, conn)
            for cfg in case["configs"]:
                key = "%s.c%d.%s.r%d" % (name, conn, cfg["tag"], cfg["rounds"])
                out, stats = R.clean_numpy(L, z["%s.T.%s" % (name, cfg["tag"])], conn, cfg["rounds"])
                assert out.dtype == L.dtype and np.array_equal(out, z[key + ".out"]), key
                assert stats.dtype == np.int64 and np.array_equal(stats, z[key + ".stats"]), key


def test_invariants(golden):
    R = _module()
    z, index = golden
    for case in index:
        L = z[case["name"] + ".L"]
        maps = L if L.ndim == 3 else L[None]
        for conn in (4, 8):
            comp, area = R.components_numpy(L, conn)
            comp, area = comp.reshape(maps.shape), area.reshape(maps.shape)
            for m, c, a in zip(maps, comp, area):
                H, W = m.shape
                roots = c.ravel() == np.arange(H * W)
                assert a.ravel()[roots].sum() == H * W                                       # the areas sum to H * W
                assert np.array_equal(c.ravel()[c.ravel()], c.ravel())                       # comp[comp] == comp
                assert np.array_equal(m.ravel()[c.ravel()], m.ravel())                       # L[comp] == L
                assert (c.ravel() <= np.arange(H * W)).all()


def test_int_threshold_and_int64_maps(golden):
    R = _module()
    z, _ = golden
    L = z["voronoi_37x53_s05.L"]
    a, sa = R.clean_numpy(L.astype(np.int64), 16, 4, 4)
    assert a.dtype == np.int64 and np.array_equal(a, z["voronoi_37x53_s05.c4.m16.r4.out"]) and np.array_equal(sa, z["voronoi_37x53_s05.c4.m16.r4.stats"])
    # a label outside 0..255 is a component of its own that is never small, no candidate, and never written
    M = np.full((6, 6), 1, np.int64); M[2, 2] = 300; M[2, 3] = 300; M[4, 4] = 2; M[0, 0] = 9; M[0, 1] = 300
    comp, area = R.components_numpy(M, 8)
    assert comp[2, 2] == 14 and comp[2, 3] == 15 and area[2, 2] == 1 and area[2, 3] == 1
    out, st = R.clean_numpy(M, 4, 4, 1)
    assert out[2, 2] == 300 and out[2, 3] == 300 and out[4, 4] == 1 and out[0, 0] == 1 and st.tolist() == [[6, 2, 2, 2]]


def test_resolve():
    R = _module()
    for off in (None, 0, False, [0] * 20, {}, {3: 0}):
        assert R.resolve(off, 20) is None
    t = R.resolve(16, 20)
    assert t.dtype == np.int32 and t.shape == (256,) and (t[:20] == 16).all() and (t[20:] == 0).all()
    t = R.resolve(np.int64(5), 20)
    assert (t[:20] == 5).all()
    t = R.resolve(list(range(20)), 20)
    assert t[:20].tolist() == list(range(20)) and (t[20:] == 0).all()
    t = R.resolve(tuple(np.arange(20)), 20)
    assert t[:20].tolist() == list(range(20))
    t = R.resolve({13: 64, 14: 100}, 20)
    assert t[13] == 64 and t[14] == 100 and t.sum() == 164
    for bad in (-1, 2.0, 16.5, True, "16", [1] * 19, [1] * 21, [1.5] * 20, [-1] + [0] * 19, {20: 4}, {-1: 4}, {3: -2}, {3: 1.5}, {"car": 4}, 2 ** 31):
        with pytest.raises(ValueError):
            R.resolve(bad, 20)


def test_numpy_route_refuses():
    R = _module()
    L = np.zeros((4, 4), np.uint8)
    for conn in (0, 6, "4"):
        with pytest.raises(ValueError):
            R.components_numpy(L, conn)
    for rounds in (0, 9, 1.5, True):
        with pytest.raises(ValueError):
            R.clean_numpy(L, 4, 4, rounds)
    with pytest.raises(ValueError):
        R.components_numpy(np.zeros((4, 4), np.float32), 4)
    with pytest.raises(ValueError):
        R.clean_numpy(L, np.zeros(20, np.int32), 4, 1)
