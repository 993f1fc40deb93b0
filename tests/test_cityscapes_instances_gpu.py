"""`fcn8s_op_cityscapes_pair` (csrc/cityscapes.hip) and the routes built on it, on the GPU.  The integer kernels are exactly comparable
with the reference evaluator, so the reference-derived fixture (tests/golden/cityscapes_instances.npz) reaches the HIP kernel directly
and every comparison in this file is an equality."""
import ctypes as C
import math
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from fcn8s_tensorflow_amd import cityscapes_eval as ce  # noqa: E402
from tests.test_cityscapes_instances_host import check_against_fixture, write_triples  # noqa: E402

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
SMALL = (8, 16, 32, 64, 64, 128, 128)


def L():
    from fcn8s_tensorflow_amd import _lib
    return _lib


def ptr(t):
    return C.c_void_p(t.data_ptr()) if t is not None else None


def dev(a):
    a = np.ascontiguousarray(a)
    if a.dtype == np.uint16:
        a = a.view(np.int16)
    return torch.from_numpy(a).cuda()


def run_op(gt, inst, pred, kind, max_entries=1024, conf=None, guard=0):
    """One raw call.  gt / inst / pred: device tensors [N, P] (inst may be None).  Returns (conf, entries [N, max_entries + guard, 4], counts, rc);
    the guard rows behind each image's entries are pre-filled with -7 and must come back untouched."""
    lib = L().lib
    N, P = gt.shape
    conf = torch.zeros(34 * 34, dtype=torch.int64, device="cuda") if conf is None else conf
    counts = torch.full((N, 3), -1, dtype=torch.int64, device="cuda")
    work = torch.empty(lib.fcn8s_op_cityscapes_work_bytes(N), dtype=torch.uint8, device="cuda") if inst is not None else None
    entries = torch.full((N * max_entries + guard, 4), -7, dtype=torch.int32, device="cuda") if inst is not None else None
    rc = lib.fcn8s_op_cityscapes_pair(None, ptr(gt), ptr(inst), ptr(pred), kind, N, P, ptr(conf), ptr(work), ptr(entries), max_entries, ptr(counts))
    torch.cuda.synchronize()
    return conf, entries, counts, rc


def numpy_truth(gt, inst, pred_ids):
    """conf and per-image entry tables by NumPy bincounts.  [N, P] arrays; pred_ids: label ids."""
    conf = np.bincount(gt.astype(np.int64).ravel() * 34 + pred_ids.astype(np.int64).ravel(), minlength=34 * 34).reshape(34, 34)
    tabs = []
    for n in range(gt.shape[0]):
        v = inst[n].astype(np.int64); p = pred_ids[n].astype(np.int64)
        lab = v // 1000
        counted = (v > 1000) & np.isin(lab, ce.INSTANCE_LABEL_IDS)
        size = np.bincount(v[counted], minlength=34000)
        tp = np.bincount(v[counted & (p == lab)], minlength=34000)
        incat = ((lab <= 25) & ((p == 24) | (p == 25))) | ((lab >= 26) & (p >= 26) & (p <= 33))
        cattp = np.bincount(v[counted & incat], minlength=34000)
        vals = np.flatnonzero(size)
        tabs.append(np.stack([vals, size[vals], tp[vals], cattp[vals]], 1))
    return conf, tabs


def check_entries(entries, counts, tabs, max_entries):
    e = entries.cpu().numpy(); c = counts.cpu().numpy()
    for n, t in enumerate(tabs):
        assert c[n, 0] == len(t) and c[n, 1] == 0 and c[n, 2] == 0
        k = min(len(t), max_entries)
        np.testing.assert_array_equal(e[n * max_entries:n * max_entries + k], t[:k])
        assert (e[n * max_entries + k:(n + 1) * max_entries] == -7).all()            # nothing written past them
    assert (e[len(tabs) * max_entries:] == -7).all()


def synthetic(N, H, W, seed, thin=True):
    """Label / instance / prediction maps with a few hundred instances per image, from one pixel to a quarter of the image, ids up to 999;
    `thin`: also one-pixel-wide columns and rows of alternating instances (every pixel a run of its own) and single pixels."""
    rng = np.random.default_rng(seed)
    things = np.array(ce.HAS_INSTANCES_IDS)
    gt = np.kron(rng.choice([0, 4, 7, 8, 11, 21, 23], (N, (H + 31) // 32, (W + 31) // 32)), np.ones((32, 32), np.int64))[:, :H, :W].astype(np.uint8)
    inst = gt.astype(np.uint16)
    for n in range(N):
        for k in range(300):
            lab = int(things[rng.integers(0, len(things))])
            h, w = (int(rng.integers(1, 120)), int(rng.integers(1, 200))) if k % 3 else (int(rng.integers(1, 4)), int(rng.integers(1, 4)))
            y, x = int(rng.integers(0, H - min(h, H - 1))), int(rng.integers(0, W - min(w, W - 1)))
            gt[n, y:y + h, x:x + w] = lab
            inst[n, y:y + h, x:x + w] = lab if rng.random() < 0.2 else lab * 1000 + int(rng.integers(0, 1000))
        y, x = int(rng.integers(0, H // 2)), int(rng.integers(0, W // 2))
        gt[n, y:y + H // 2, x:x + W // 2] = 26; inst[n, y:y + H // 2, x:x + W // 2] = 26999        # a quarter of the image, k = 999
        if thin:
            y, x = int(rng.integers(0, H - 64)), int(rng.integers(0, W - 64))
            cols = np.arange(64)
            gt[n, y:y + 64, x:x + 64] = np.where(cols % 2, 24, 25)[None, :]                         # interleaved one-pixel columns of two instances
            inst[n, y:y + 64, x:x + 64] = np.where(cols % 2, 24000, 25998)[None, :]
            y2 = int(rng.integers(0, H - 8))
            gt[n, y2, :] = 33; inst[n, y2, :] = 33000 + (np.arange(W) % 1000)                       # a row in which every pixel is its own instance
            gt[n, y2 + 2, : W // 2] = 31; inst[n, y2 + 2, : W // 2] = 31500                         # a one-pixel-high instance
    train = ce.IDS_TO_TRAINIDS_ARRAY[gt].astype(np.int64)
    damaged = np.kron(rng.random((N, (H + 7) // 8, (W + 7) // 8)) < 0.3, np.ones((8, 8), bool))[:, :H, :W]
    train[damaged] = rng.integers(0, 20, int(damaged.sum()))
    speck = rng.random(train.shape) < 0.02
    train[speck] = rng.integers(0, 20, int(speck.sum()))
    return gt.reshape(N, -1), inst.reshape(N, -1), train.reshape(N, -1)


def test_fixture_through_the_kernel_both_pred_kinds():
    d = np.load(os.path.join(GOLD, "cityscapes_instances.npz"))
    N = len(d["names"])
    gt, inst, pred = d["gts"].reshape(N, -1), d["insts"].reshape(N, -1), d["preds"].reshape(N, -1)
    truth_conf, truth_tabs = ce.pair_counts_numpy(d["preds"], d["gts"], d["insts"], pred_is_train_ids=False)
    for kind in (0, 1):
        p = dev(ce.IDS_TO_TRAINIDS_ARRAY[pred].astype(np.int64)) if kind == 0 else dev(pred)
        conf, entries, counts, rc = run_op(dev(gt), dev(inst), p, kind, max_entries=64, guard=3)
        assert rc == 0
        np.testing.assert_array_equal(conf.cpu().numpy().reshape(34, 34), truth_conf)
        np.testing.assert_array_equal(truth_conf, d["conf"])
        check_entries(entries, counts, truth_tabs, 64)
        # scores: the host half on the kernel's entries == the reference evaluator's
        ev = ce.PixelLevelEvaluator(instance_level=True)
        if kind == 0:
            ev.add(p.view(d["preds"].shape), dev(d["gts"]), dev(d["insts"]))
        else:
            ev.add(p.view(d["preds"].shape), dev(d["gts"]), dev(d["insts"]), pred_is_train_ids=False)
        check_against_fixture(ev.results(), d, ev.conf)
    # image by image, and the file route with device=
    ev = ce.PixelLevelEvaluator(instance_level=True)
    for n in range(N):
        ev.add(dev(ce.IDS_TO_TRAINIDS_ARRAY[d["preds"][n]].astype(np.int64)), d["gts"][n], d["insts"][n])
    check_against_fixture(ev.results(), d, ev.conf)


def test_file_route_on_the_device(tmp_path):
    d = np.load(os.path.join(GOLD, "cityscapes_instances.npz"))
    write_triples(d, str(tmp_path))
    res = ce.evaluate_directory(os.path.join(str(tmp_path), "gtFine", "val", "*", "*_gtFine_labelIds.png"), os.path.join(str(tmp_path), "results"),
                                device=torch.device("cuda", 0), instance_level=True)
    check_against_fixture(res, d, res["confMatrix"])


@pytest.mark.parametrize("N,H,W", [(4, 1024, 2048), (16, 512, 1024), (3, 301, 517), (1, 7, 5)])
def test_full_size_against_bincounts(N, H, W):
    """Exact against NumPy at the sizes a user runs, adversarial maps included; 301 x 517: P not a multiple of 16, so the second and third
    image start off the 16-byte grid (odd W: every row start misaligned as well); 7 x 5: less than one lane's 16 pixels."""
    if H >= 64:
        gt, inst, train = synthetic(N, H, W, seed=H + N)
    else:
        rng = np.random.default_rng(3)
        gt = rng.integers(0, 34, (N, H * W)).astype(np.uint8); train = rng.integers(0, 20, (N, H * W))
        inst = np.where(rng.random((N, H * W)) < 0.5, gt.astype(np.uint16) * 1000 + 7, gt.astype(np.uint16))
        inst[(inst > 1000) & ~np.isin(inst // 1000, ce.HAS_INSTANCES_IDS + list(ce.IGNORED_IDS))] = 5
    ids = ce.TRAINIDS_TO_IDS_ARRAY[train]
    truth_conf, truth_tabs = numpy_truth(gt, inst, ids)
    if H >= 512:
        assert min(len(t) for t in truth_tabs) >= 200 and min(t[:, 1].max() for t in truth_tabs) >= H * W // 5 and min(t[:, 1].min() for t in truth_tabs) == 1
        assert any((t[:, 0] % 1000 == 999).any() for t in truth_tabs)
    g, i = dev(gt), dev(inst)
    for kind, p in ((0, dev(train)), (1, dev(ids))):
        conf, entries, counts, rc = run_op(g, i, p, kind, max_entries=1536, guard=2)
        assert rc == 0
        np.testing.assert_array_equal(conf.cpu().numpy().reshape(34, 34), truth_conf)
        check_entries(entries, counts, truth_tabs, 1536)
    # buffers that do not start on a 16-byte boundary: the same answer
    if H == 301:
        g1 = torch.empty(gt.size + 1, dtype=torch.uint8, device="cuda"); g1[1:] = g.view(-1)
        conf, entries, counts, rc = run_op(g1[1:].view(N, -1), i, dev(train), 0, max_entries=1536)
        assert rc == 0
        np.testing.assert_array_equal(conf.cpu().numpy().reshape(34, 34), truth_conf)
        check_entries(entries, counts, truth_tabs, 1536)


def test_without_instances_is_the_confusion_kernel_and_conf_accumulates():
    gt, inst, train = synthetic(2, 256, 512, seed=11)
    lib = L().lib
    g, p = dev(gt), dev(train)
    ids = dev(ce.TRAINIDS_TO_IDS_ARRAY[train].astype(np.int64))
    old = torch.zeros(34 * 34, dtype=torch.int64, device="cuda")
    assert lib.fcn8s_op_confusion(None, ptr(g), ptr(ids), gt.size, ptr(old), 34) == 0
    conf, entries, counts, rc = run_op(g, None, p, 0)
    assert rc == 0 and entries is None
    assert torch.equal(conf, old)
    assert counts.cpu().numpy().tolist() == [[0, 0, 0], [0, 0, 0]]
    conf2, _, _, rc = run_op(g, dev(inst), p, 0, conf=conf)                                     # a second call adds to the same matrix
    assert rc == 0 and conf2 is conf and torch.equal(conf, 2 * old)


def test_more_entries_than_room_and_the_retry():
    gt, inst, train = synthetic(2, 256, 512, seed=5)
    ids = ce.TRAINIDS_TO_IDS_ARRAY[train]
    truth_conf, truth_tabs = numpy_truth(gt, inst, ids)
    assert min(len(t) for t in truth_tabs) > 40
    for room in (40, 1, 0):
        conf, entries, counts, rc = run_op(dev(gt), dev(inst), dev(train), 0, max_entries=room, guard=5)
        assert rc == 0
        check_entries(entries, counts, truth_tabs, room)                                       # the count is reported, the first `room` entries are right
        np.testing.assert_array_equal(conf.cpu().numpy().reshape(34, 34), truth_conf)
    ev = ce.PixelLevelEvaluator(instance_level=True)                                            # the Python layer repeats the call with the reported count
    ev.add(dev(train).view(2, 256, 512), dev(gt).view(2, 256, 512), dev(inst).view(2, 256, 512), max_entries=40)
    ref = ce.PixelLevelEvaluator(instance_level=True)
    ref.add(train.reshape(2, 256, 512), gt.reshape(2, 256, 512), inst.reshape(2, 256, 512))
    np.testing.assert_array_equal(ev.conf, ref.conf)                                            # ... and counts the matrix once
    assert ev.results()["instStats"] == ref.results()["instStats"]
    a, b = ev.results(), ref.results()
    for k in ("classInstScores", "categoryInstScores"):
        for name in a[k]:
            assert (math.isnan(a[k][name]) and math.isnan(b[k][name])) or a[k][name] == b[k][name]


def test_out_of_range_ids_are_counted_and_nowhere_else():
    gt, inst, train = synthetic(2, 128, 256, seed=9, thin=False)
    ids = ce.TRAINIDS_TO_IDS_ARRAY[train]
    gt_bad = gt.copy(); train_bad = train.copy(); inst_bad = inst.copy()
    gt_bad[0, 5:9] = 34; gt_bad[1, 100] = 255                                                   # 5 pixels of an unknown label
    train_bad[1, 7000:7003] = 20; train_bad[0, 11] = -1; train_bad[0, 12] = 1 << 40             # 5 predictions outside 0..19
    inst_bad[0, 300:310] = 7005; inst_bad[1, 400:403] = 34001; inst_bad[1, 500] = 65535         # 14 pixels of a value the evaluator dies on
    bad = (gt_bad >= 34) | (train_bad < 0) | (train_bad >= 20)
    keep_gt = np.where(bad, 0, gt_bad); keep_ids = np.where(bad, 0, ce.TRAINIDS_TO_IDS_ARRAY[np.where(bad, 0, train_bad)])
    keep_inst = np.where(bad | (inst_bad == 7005) | (inst_bad == 34001) | (inst_bad == 65535), 0, inst_bad)
    truth_conf, truth_tabs = numpy_truth(keep_gt, keep_inst, keep_ids)
    truth_conf[0, 0] -= int(bad.sum())
    conf, entries, counts, rc = run_op(dev(gt_bad), dev(inst_bad), dev(train_bad), 0)
    assert rc == 0
    c = counts.cpu().numpy()
    assert c[:, 1].tolist() == [int(bad[0].sum()), int(bad[1].sum())] and c[:, 1].sum() == 10
    badv = (~bad) & np.isin(inst_bad, [7005, 34001, 65535])
    assert c[:, 2].tolist() == [int(badv[0].sum()), int(badv[1].sum())]
    np.testing.assert_array_equal(conf.cpu().numpy().reshape(34, 34), truth_conf)
    assert int(conf.sum()) == gt.size - int(bad.sum())
    e = entries.cpu().numpy()
    for n, t in enumerate(truth_tabs):
        assert c[n, 0] == len(t)
        np.testing.assert_array_equal(e[n * 1024:n * 1024 + len(t)], t)
    # the Python layer turns each of them into the evaluator's error
    shape = (2, 128, 256)
    with pytest.raises(ValueError, match="Unknown label with id 255"):
        ce.PixelLevelEvaluator(instance_level=True).add(dev(train).view(shape), dev(gt_bad).view(shape), dev(inst).view(shape))
    with pytest.raises(ValueError, match="train ids"):
        ce.PixelLevelEvaluator(instance_level=True).add(dev(train_bad).view(shape), dev(gt).view(shape), dev(inst).view(shape))
    with pytest.raises(ValueError, match="7005"):
        ce.PixelLevelEvaluator(instance_level=True).add(dev(train).view(shape), dev(gt).view(shape), dev(inst_bad).view(shape))


def test_argument_errors_launch_nothing():
    _lib = L(); lib = _lib.lib
    gt, inst, train = synthetic(1, 64, 128, seed=2, thin=False)
    g, i, p = dev(gt), dev(inst), dev(train)
    conf = torch.zeros(34 * 34, dtype=torch.int64, device="cuda")
    counts = torch.full((1, 3), -1, dtype=torch.int64, device="cuda")
    work = torch.full((lib.fcn8s_op_cityscapes_work_bytes(1),), 0x5A, dtype=torch.uint8, device="cuda")
    entries = torch.full((16, 4), -7, dtype=torch.int32, device="cuda")
    call = lambda gi, kind, N, P, me, ent: lib.fcn8s_op_cityscapes_pair(None, ptr(g), ptr(gi), ptr(p), kind, N, P, ptr(conf), ptr(work), ptr(ent), me, ptr(counts))
    assert call(i, 2, 1, gt.size, 16, entries) == _lib.ERR_BAD_ARG
    assert call(i, -1, 1, gt.size, 16, entries) == _lib.ERR_BAD_ARG
    assert call(i, 0, 0, gt.size, 16, entries) == _lib.ERR_BAD_ARG
    assert call(i, 0, 1, 0, 16, entries) == _lib.ERR_BAD_ARG
    assert call(i, 0, 1, gt.size, -1, entries) == _lib.ERR_BAD_ARG
    assert call(i, 0, 1, gt.size, 16, None) == _lib.ERR_BAD_ARG
    assert call(i, 0, 1, 1 << 31, 16, entries) == _lib.ERR_SHAPE
    assert b"2^31" in lib.fcn8s_last_error(None)
    torch.cuda.synchronize()
    assert int(conf.abs().sum()) == 0 and (counts == -1).all() and (entries == -7).all() and (work == 0x5A).all()
    assert lib.fcn8s_op_cityscapes_work_bytes(0) == 0 and lib.fcn8s_op_cityscapes_work_bytes(-2) == 0 and lib.fcn8s_op_cityscapes_work_bytes(3) == 3 * lib.fcn8s_op_cityscapes_work_bytes(1)


def test_two_runs_give_identical_bits():
    gt, inst, train = synthetic(4, 512, 1024, seed=21)
    g, i, p = dev(gt), dev(inst), dev(train)
    a = run_op(g, i, p, 0, max_entries=1536)
    b = run_op(g, i, p, 0, max_entries=1536)
    assert a[3] == 0 and b[3] == 0
    for x, y in zip(a[:3], b[:3]):
        assert torch.equal(x, y)


def _same(a, b):
    assert sorted(a) == sorted(b)
    np.testing.assert_array_equal(a["confMatrix"], b["confMatrix"])
    assert a["nbPixels"] == b["nbPixels"]
    if "instStats" in a:
        assert a["instStats"] == b["instStats"]
    for k in a:
        if k.startswith("average"):
            assert (math.isnan(a[k]) and math.isnan(b[k])) or a[k] == b[k], k
        elif k.endswith("Scores"):
            assert list(a[k]) == list(b[k])
            for name in a[k]:
                assert (math.isnan(a[k][name]) and math.isnan(b[k][name])) or a[k][name] == b[k][name], (k, name)


def test_facade_equals_export_plus_directory_evaluation(tmp_path):
    """evaluate_cityscapes == predict_and_export_label_ids + evaluate_directory on the same files and arguments, exactly; nothing is written
    into the images directory.  64 x 96 is not a multiple of 32: `scales=(1.0,)` in the plain run."""
    from PIL import Image
    from fcn8s_tensorflow_amd.fcn8s import FCN8s
    m = FCN8s(vgg16_dir='synthetic:3', num_classes=20, widths=SMALL)
    rng = np.random.default_rng(8)
    names = ["aachen_000000_000019", "aachen_000001_000019", "bonn_000002_000019"]
    things = np.array(ce.HAS_INSTANCES_IDS)
    for nm in names:
        city = nm.split("_")[0]
        (tmp_path / "leftImg8bit" / city).mkdir(parents=True, exist_ok=True); (tmp_path / "gtFine" / city).mkdir(parents=True, exist_ok=True)
        img = np.kron(rng.integers(0, 256, (8, 12, 3)), np.ones((8, 8, 1), np.int64)).astype(np.uint8) + rng.integers(0, 8, (64, 96, 3), dtype=np.uint8) // 2
        gt = np.kron(rng.integers(0, 34, (8, 12)), np.ones((8, 8), np.int64)).astype(np.uint8)
        inst = gt.astype(np.uint16)
        for k in range(10):
            lab = int(things[rng.integers(0, len(things))])
            y, x, h, w = int(rng.integers(0, 50)), int(rng.integers(0, 80)), int(rng.integers(1, 14)), int(rng.integers(1, 16))
            gt[y:y + h, x:x + w] = lab; inst[y:y + h, x:x + w] = lab * 1000 + k if k % 4 else lab
        Image.fromarray(img).save(tmp_path / "leftImg8bit" / city / (nm + "_leftImg8bit.png"))
        Image.fromarray(gt).save(tmp_path / "gtFine" / city / (nm + "_gtFine_labelIds.png"))
        Image.fromarray(inst).save(tmp_path / "gtFine" / city / (nm + "_gtFine_instanceIds.png"))
    before = sorted(os.path.join(r, f) for r, _, fs in os.walk(tmp_path / "leftImg8bit") for f in fs)
    search = str(tmp_path / "gtFine" / "*" / "*_gtFine_labelIds.png")
    for run, kw in enumerate((dict(scales=(1.0,)), dict(scales=(0.75, 1.0), flip=True, crf=True))):
        res = m.evaluate_cityscapes(str(tmp_path / "leftImg8bit"), search, json_path=str(tmp_path / ("r%d" % run) / "result.json"), **kw)
        assert sorted(os.path.join(r, f) for r, _, fs in os.walk(tmp_path / "leftImg8bit") for f in fs) == before
        out = str(tmp_path / ("results%d" % run))
        assert m.predict_and_export_label_ids(out, str(tmp_path / "leftImg8bit"), **kw) == 3
        _same(res, ce.evaluate_directory(search, out, instance_level=True))
        assert res["nbPixels"] == 3 * 64 * 96 and "classInstScores" in res
        assert os.path.isfile(tmp_path / ("r%d" % run) / "result.json")
    # pixel-level only, and through a resize (the prediction comes back to the file's size as the export writes it)
    res = m.evaluate_cityscapes(str(tmp_path / "leftImg8bit"), search, resize=(32, 64), instance_level=False)
    out = str(tmp_path / "results_resized")
    m.predict_and_export_label_ids(out, str(tmp_path / "leftImg8bit"), resize=(32, 64))
    _same(res, ce.evaluate_directory(search, out))
    res = m.evaluate_cityscapes(str(tmp_path / "leftImg8bit"), search, resize=(32, 64))
    _same(res, ce.evaluate_directory(search, out, instance_level=True))
    with pytest.raises(ValueError, match="Cannot find any ground truth"):
        m.evaluate_cityscapes(str(tmp_path / "leftImg8bit"), str(tmp_path / "nothing" / "*.png"))
    m.close()
