"""The host half of class-balanced pseudo-labelling (fcn8s_tensorflow_amd/pseudo_label.py) against tests/golden/pseudo_label_cases.npz, whose
expected values were written by plain Python loops and `sorted()` (tests/golden/make_pseudo_label_cases.py shares no code with the module).
Everything that decides anything is an integer: every comparison is `==`."""
import functools
import json
import os
from fractions import Fraction

import numpy as np
import pytest

from fcn8s_tensorflow_amd import pseudo_label as PL

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "pseudo_label_cases.npz")
M = PL.BINS


@functools.lru_cache(maxsize=None)
def golden():
    z = np.load(GOLDEN)
    meta = json.loads(bytes(z["meta"]).decode())
    cases = []
    for i, (N, P, Cn) in enumerate(meta["cases"]):
        d = {k[len("%d_" % i):]: z[k] for k in z.files if k.startswith("%d_" % i)}
        for a in d.values():
            a.setflags(write=False)
        d.update(N=N, P=P, C=Cn, base_fill=int(d["base_fill"]), score_max=float(d["score_max"]))
        cases.append(d)
    return meta, cases


def case_ids():
    return ["N%d-P%d-C%d" % tuple(c) for c in golden()[0]["cases"]]


def full_args(c):
    """The arguments of variant A: everything given."""
    return dict(thresholds=c["thr"], out_ids=c["out_ids"], ignore_id=250, base=c["base"], base_fill=c["base_fill"], score=c["score"],
                score_max=c["score_max"])


def same(got, c, variant, names=("labels", "hist", "counts", "misc")):
    for g, name in zip(got, ("labels", "hist", "counts", "misc")):
        if name in names:
            w = c["%s_%s" % (variant, name)]
            assert g.dtype == w.dtype and g.shape == w.shape and (g == w).all(), (variant, name, np.argwhere(g != w)[:8])


def test_the_fixture_holds_the_cases_the_kernel_can_go_wrong_at():
    meta, cases = golden()
    assert meta["bins"] == M and {c["P"] * c["N"] for c in cases} >= {1, 15, 255, 256, 257, 513, 600} and {c["C"] for c in cases} == {2, 19, 20, 21, 64}
    assert os.path.getsize(GOLDEN) < 512 * 1024
    from fcn8s_tensorflow_amd import cityscapes_eval as ce
    c20 = [c for c in cases if c["C"] == 20][0]
    assert (c20["out_ids"] == ce.TRAINIDS_TO_IDS_ARRAY).all()
    for c in cases:
        assert 0.3 < ((c["base"] == c["base_fill"]).mean() if c["P"] > 15 else 0.5) < 0.7
        e = c["C"] - 1
        frac = c["thr"].astype(np.float64) * M % 1
        assert frac[e] == 0 and (np.delete(frac, e) != 0).all()          # thresholds off the bin edges, but for the edge rows' class


@pytest.mark.parametrize("i", range(len(golden()[0]["cases"])), ids=case_ids())
def test_tables_numpy_equals_the_fixture(i):
    c = golden()[1][i]
    same(PL.tables_numpy(c["prob"], **full_args(c)), c, "A")
    same(PL.tables_numpy(c["prob"]), c, "B")
    thr = (c["fit_bins"].astype(np.float64) / M).astype(np.float32)
    same(PL.tables_numpy(c["prob"], thresholds=thr), c, "C", ("labels", "counts"))


def test_the_hand_made_rows_land_where_the_definition_puts_them():
    meta, cases = golden()
    hand = {n: j for j, n in enumerate(meta["hand"])}
    j = meta["edge_bin"]
    for c in cases:
        if c["P"] < 15:
            continue
        Cn, e = c["C"], c["C"] - 1
        p = c["prob"][0]
        lab, hist, counts, misc = PL.tables_numpy(p[:len(hand)], **{k: (v[0, :len(hand)] if k in ("base", "score") else v) for k, v in full_args(c).items()})
        oid = c["out_ids"]
        thr = c["thr"]
        assert lab[hand["tie_0"]] == (oid[0] if np.float32(0.4) >= thr[0] else 250) and hist[0, int(np.float32(0.4) * np.float32(M))] == 1      # k = 0
        assert lab[hand["tie_high"]] == (oid[1] if np.float32(0.45) >= thr[1] else 250) and hist[1, int(np.float32(0.45) * np.float32(M))] == 1
        assert lab[hand["on_edge"]] == oid[e] and hist[e, j] == 1
        assert lab[hand["below_edge"]] == 250 and hist[e, j - 1] == 1
        assert lab[hand["one"]] == oid[0] and hist[0, M - 1] == 1
        assert lab[hand["zeros"]] == 250 and lab[hand["negative_max"]] == 250 and hist[0, 0] == 1 and hist[1, 0] == 1
        assert lab[hand["nan_0"]] == 250 and lab[hand["inf"]] == 250 and misc[0] == 2
        assert hist[2 if Cn >= 3 else 0, int(np.float32(0.8) * np.float32(M))] == 1           # the NaN below the maximum changed nothing
        assert lab[hand["score_on"]] == oid[0] and lab[hand["score_above"]] == 250 and lab[hand["score_nan"]] == 250 and misc[2] == 2
        assert lab[hand["plain"]] == oid[0] and hist[0, int(np.float32(0.97) * np.float32(M))] == 2      # score_on and plain; the gated two are not in hist
        assert misc[1] == 0 and counts.sum() == len(hand) - 2 and hist.sum() == len(hand) - 4
        # with nothing given the row of zeros is kept (0 >= 0) and the negative maximum is not
        lab = PL.tables_numpy(p[:len(hand)])[0]
        assert lab[hand["zeros"]] == 0 and lab[hand["negative_max"]] == 255 and lab[hand["nan_0"]] == 255
        if Cn >= 5:
            assert c["B_hist"][Cn // 2].sum() == 0 and c["fit_bins"][Cn // 2] == M              # a class that is never predicted


@pytest.mark.parametrize("i", range(len(golden()[0]["cases"])), ids=case_ids())
def test_thresholds_from_hist_equals_the_sorted_portion_rule(i):
    c = golden()[1][i]
    thr, bins = PL.thresholds_from_hist(c["B_hist"], 0.2)
    assert bins.dtype == np.int64 and (bins == c["fit_bins"]).all()
    assert thr.dtype == np.float32 and (thr == (c["fit_bins"] / M).astype(np.float32)).all()
    pc = [float(Fraction(int(n), int(d))) for n, d in c["portions_pc"]]
    assert (PL.thresholds_from_hist(c["B_hist"], pc)[1] == c["fit_bins_pc"]).all()


def kept_under(c, bins):
    thr = (np.asarray(bins, np.float64) / M).astype(np.float32)
    return PL.tables_numpy(c["prob"], thresholds=thr)[2][:, 0]


@pytest.mark.parametrize("i", range(len(golden()[0]["cases"])), ids=case_ids())
def test_kept_counts_under_fitted_thresholds_are_the_tail_sums_of_the_histogram(i):
    """The exact identity of the definition.  It holds for conf in [0, 1): a negative maximum sits in bin 0 without clearing the threshold 0,
    and conf = 1.0 clears the threshold 1024 / 1024 from bin 1023, so the classes of those two hand-made rows are compared only where their
    threshold lies strictly between."""
    c = golden()[1][i]
    hist = c["B_hist"]
    for portion in (0.2, 0.05, 0.9):
        thr, bins = PL.thresholds_from_hist(hist, portion)
        ok = (bins > 0) & (bins < M)
        assert (kept_under(c, bins)[ok] == PL.tail_sums(hist, bins)[ok]).all()
        assert (c["C_counts"][:, 0][ok] == PL.tail_sums(hist, c["fit_bins"])[ok]).all() if portion == 0.2 else True
        # a clamp that does not bite changes nothing
        lo, hi = int(bins[ok].min()) if ok.any() else 1, int(bins[ok].max()) if ok.any() else M - 1
        _, b2 = PL.thresholds_from_hist(hist, portion, t_min=lo / M, t_max=hi / M)
        assert (b2[ok] == bins[ok]).all()
        # a biting t_min raises thresholds: kept <= the unclamped tail; a biting t_max lowers them: kept >= it
        mid = (lo + hi + 1) // 2
        _, up = PL.thresholds_from_hist(hist, portion, t_min=mid / M)
        assert (up == np.maximum(bins, mid)).all() and (kept_under(c, up)[ok] <= PL.tail_sums(hist, bins)[ok]).all()
        assert (kept_under(c, up)[ok & (up < M)] == PL.tail_sums(hist, up)[ok & (up < M)]).all()
        _, down = PL.thresholds_from_hist(hist, portion, t_max=mid / M)
        assert (down == np.minimum(bins, mid)).all() and (kept_under(c, down)[ok] >= PL.tail_sums(hist, bins)[ok]).all()


def test_thresholds_fall_as_the_portion_grows_and_portion_one_keeps_every_eligible_pixel():
    for c in golden()[1]:
        hist = c["B_hist"]
        prev = None
        for portion in (0.01, 0.1, 0.2, 0.5, 0.75, 1.0):
            thr, bins = PL.thresholds_from_hist(hist, portion)
            assert prev is None or ((bins <= prev).all() and (thr <= prev_thr).all())
            prev, prev_thr = bins, thr
        n = hist.sum(1)
        assert (PL.tail_sums(hist, bins) == n).all()                      # portion = 1: the whole histogram lies above the threshold
        assert (bins[n == 0] == M).all()
        ok = bins > 0                                                     # (a class whose smallest confidence is <= 0 has bin 0: see the identity's note)
        assert (kept_under(c, bins)[ok] == n[ok]).all()


def test_the_portion_is_an_exact_rational():
    hist = np.zeros((2, M), np.int64)
    hist[0, 10] = 7; hist[0, 500] = 3                                     # n = 10: portion 0.3 takes exactly the 3 at bin 500
    hist[1, 1023] = 1
    assert PL.thresholds_from_hist(hist, 0.3)[1].tolist() == [500, 1023]
    assert PL.thresholds_from_hist(hist, 0.30001)[1].tolist() == [10, 1023]
    assert PL.thresholds_from_hist(hist, [0.1, 1.0])[1].tolist() == [500, 1023]
    assert PL.thresholds_from_hist(hist, 1.0, t_min=0.5, t_max=0.75)[1].tolist() == [512, 768]
    assert PL.thresholds_from_hist(hist, 1.0, t_min=0.5001)[1].tolist() == [513, 1023]           # ceil(t_min M)
    assert PL.thresholds_from_hist(hist, 1.0, t_max=0.9999)[1].tolist() == [10, 1023]            # floor(t_max M)
    assert PL.portions_of(0.2, 3) == [Fraction(1, 5)] * 3


def test_summary_is_plain_and_adds_up():
    c = [c for c in golden()[1] if c["P"] == 513 and c["C"] == 20][0]
    lab, hist, counts, misc = PL.tables_numpy(c["prob"], **full_args(c))
    s = PL.summary(hist, counts, misc, c["thr"])
    s2 = json.loads(json.dumps(s))
    assert s2["totals"]["pixels"] == 513 and s2["totals"]["kept"] == int(counts[:, 0].sum()) == int((lab != 250).sum()) - int(misc[1])
    assert [r["predicted"] for r in s2["classes"]] == counts.sum(1).tolist() and s2["classes"][3]["threshold"] == float(c["thr"][3])
    assert s2["totals"]["passedThrough"] == int(misc[1]) and s2["totals"]["droppedByScore"] == int(misc[2]) and s2["totals"]["badRows"] == int(misc[0])
    assert PL.summary(None, counts, misc)["classes"][0]["threshold"] is None


def test_validate_refuses_what_the_facade_refuses():
    ok = PL.validate(20, portion=0.2, t_min=0.1, t_max=0.9, ignore_id=255, id_space='label', base_search="x/*.png", base_fill=0, samples=4, mi_max=0.1)
    assert ok["bins_range"] == (103, 921) and ok["ignore_id"] == 255 and ok["base_fill"] == 0 and ok["mi_max"] == 0.1 and ok["thresholds"] is None
    bad = [dict(portion=0.0), dict(portion=1.5), dict(portion=-0.1), dict(portion=float('nan')), dict(portion=[0.2] * 19), dict(t_min=-0.1), dict(t_min=1.1),
           dict(t_min=0.8, t_max=0.5), dict(t_max=1.5), dict(t_min=0.30001, t_max=0.30002), dict(ignore_id=256), dict(ignore_id=-1), dict(ignore_id=2.5),
           dict(ignore_id=True), dict(id_space='ids'), dict(base_search="x/*.png"), dict(base_fill=255), dict(base_search="x", base_fill=256),
           dict(base_search="x", base_fill=0, resize=(64, 64)), dict(samples=4, passes=True), dict(samples=4, temperature=1.5), dict(mi_max=0.1),
           dict(samples=4, mi_max=float('inf')), dict(thresholds=[0.5] * 19), dict(thresholds=[float('nan')] * 20)]
    for kw in bad:
        with pytest.raises(ValueError):
            PL.validate(20, **kw)
    for n in (1, 256):
        with pytest.raises(ValueError):
            PL.validate(n)
    with pytest.raises(ValueError):
        PL.validate(19, id_space='label')
    PL.validate(19, id_space='train')
    with pytest.raises(ValueError):
        PL.tables_numpy(np.zeros((4, 20), np.float32), score=np.zeros(4, np.float32))            # a score map without score_max
    with pytest.raises(ValueError):
        PL.tables_numpy(np.zeros((4, 20), np.float32), base=np.zeros(4, np.uint8))               # a base map without base_fill
    with pytest.raises(ValueError):
        PL.tables_numpy(np.zeros((4, 20), np.float64))


def test_find_base_pairs_by_city_sequence_and_frame():
    files = ["/b/aachen_000000_000019_gtCoarse_labelTrainIds.png", "/b/aachen_000001_000019_gtCoarse_labelTrainIds.png"]
    assert PL.find_base("/i/aachen/aachen_000001_000019_leftImg8bit.png", files) == files[1]
    with pytest.raises(ValueError):
        PL.find_base("/i/aachen/aachen_000002_000019_leftImg8bit.png", files)
    with pytest.raises(ValueError):
        PL.find_base("/i/aachen/aachen_000000_000019_leftImg8bit.png", files + ["/c/aachen_000000_000019_gtFine_labelIds.png"])
