"""`fcn8s_op_boundary_pair` (csrc/boundary.hip) and the routes built on it, on the GPU.  The kernel counts integers, so the SciPy-derived
fixture (tests/golden/trimap_cases.npz), the hand-counted cases and the package's NumPy route of the same definition are all compared
with `==`."""
import ctypes as C
import math
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from fcn8s_tensorflow_amd import cityscapes_eval as ce  # noqa: E402
from tests.test_trimap_host import dense, fixture_cases, hand_cases, voronoi_pair  # noqa: E402

SMALL = (8, 16, 32, 64, 64, 128, 128)
GUARD = 5                                                      # words behind each output that must come back untouched
MAGIC = -0x5A5A5A5A5A5A5A5B


def L():
    from fcn8s_tensorflow_amd import _lib
    return _lib


def ptr(t, offset=0):
    return C.c_void_p(t.data_ptr() + offset) if t is not None else None


class Out:
    """rings / bprec / brec / bad on the device, each followed by GUARD words of MAGIC."""

    def __init__(self, R):
        self.R = R
        self.sizes = ((R + 1) * 34 * 34, (R + 2) * 34, (R + 2) * 34, 1)
        self.bufs = [torch.full((n + GUARD,), MAGIC, dtype=torch.int64, device="cuda") for n in self.sizes]
        for b, n in zip(self.bufs, self.sizes):
            b[:n] = 0

    def tables(self):
        torch.cuda.synchronize()
        for b, n in zip(self.bufs, self.sizes):
            assert (b[n:] == MAGIC).all(), "guard words overwritten"
        R = self.R
        r, bp, br, bad = (b[:n].cpu().numpy() for b, n in zip(self.bufs, self.sizes))
        return r.reshape(R + 1, 34, 34), bp.reshape(R + 2, 34), br.reshape(R + 2, 34), int(bad[0])


def run_op(gt, pred, kind, R, out=None, N=None, H=None, W=None):
    """One raw call on device tensors [N, H, W] (or [H, W])."""
    shape = tuple(gt.shape)
    N = (1 if len(shape) == 2 else shape[0]) if N is None else N
    H = shape[-2] if H is None else H
    W = shape[-1] if W is None else W
    out = Out(R) if out is None else out
    rc = L().lib.fcn8s_op_boundary_pair(None, ptr(gt), ptr(pred), kind, N, H, W, R, *(ptr(b) for b in out.bufs))
    return out, rc


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def to_train(ids, rng):
    """int64 train ids whose label ids are `ids` where that is possible (an evaluated label or 0); elsewhere a random train id."""
    ids = np.asarray(ids)
    t = ce.IDS_TO_TRAINIDS_ARRAY[ids].astype(np.int64)
    back = ce.TRAINIDS_TO_IDS_ARRAY[t]
    other = back != ids
    t[other] = rng.integers(0, 20, int(other.sum()))
    return t


def check(G, P_ids, R, train=None):
    """Both pred_kinds against the NumPy route; G, P_ids [H, W] or [N, H, W] uint8, train: int64 train ids for pred_kind 0."""
    want = ce.boundary_counts_numpy(P_ids, G, R, pred_is_train_ids=False)
    out, rc = run_op(dev(G), dev(P_ids), 1, R)
    assert rc == 0
    got = out.tables()
    for a, b in zip(got[:3], want):
        np.testing.assert_array_equal(a, b)
    assert got[3] == 0
    if train is not None:
        want = ce.boundary_counts_numpy(train, G, R)
        out, rc = run_op(dev(G), dev(train), 0, R)
        assert rc == 0
        got = out.tables()
        for a, b in zip(got[:3], want):
            np.testing.assert_array_equal(a, b)
        assert got[3] == 0
    return want


def cityscapes_like(rng, N, H, W, blk=64):
    """Large rectangles of constant label (long runs, few contours), the prediction shifted by a few pixels with some damaged blocks."""
    G = np.kron(rng.integers(0, 34, (N, (H + blk - 1) // blk, (W + blk - 1) // blk)), np.ones((blk, blk), np.int64))[:, :H, :W].astype(np.uint8)
    for n in range(N):
        for _ in range(12):
            y, x, h, w = (int(rng.integers(0, max(H - 8, 1))), int(rng.integers(0, max(W - 8, 1))), int(rng.integers(1, max(H // 6, 2))),
                          int(rng.integers(1, max(W // 10, 2))))
            G[n, y:y + h, x:x + w] = rng.integers(24, 34)
    P = np.roll(G, (2, -3), (1, 2)).copy()
    damaged = np.kron(rng.random((N, (H + 15) // 16, (W + 15) // 16)) < 0.05, np.ones((16, 16), bool))[:, :H, :W]
    P[damaged] = rng.integers(0, 34, int(damaged.sum()))
    return G, P


def test_kernel_equals_scipy_fixture():
    for G, P, R, rings, bprec, brec in fixture_cases():
        out, rc = run_op(dev(G), dev(P), 1, R)
        assert rc == 0
        r, bp, br, bad = out.tables()
        np.testing.assert_array_equal(r, rings); np.testing.assert_array_equal(bp, bprec); np.testing.assert_array_equal(br, brec)
        assert bad == 0


def test_kernel_equals_hand_counted_cases():
    for G, P, R, rings, bprec, brec in hand_cases():
        out, rc = run_op(dev(G), dev(P), 1, R)
        assert rc == 0
        r, bp, br, bad = out.tables()
        np.testing.assert_array_equal(r, dense((R + 1, 34, 34), rings))
        np.testing.assert_array_equal(bp, dense((R + 2, 34), bprec))
        np.testing.assert_array_equal(br, dense((R + 2, 34), brec))
        assert bad == 0


@pytest.mark.parametrize("H,W", [(1, 1), (1, 70), (70, 1), (37, 53), (257, 511)])
@pytest.mark.parametrize("R", [1, 2, 5, 16])
def test_kernel_equals_numpy_route(H, W, R):
    rng = np.random.default_rng(1000 * H + 10 * W + R)
    for N in (1, 3):
        pairs = [voronoi_pair(rng, H, W, cells=max(2, min(40, H * W // 300))) for _ in range(N)]
        G = np.stack([p[0] for p in pairs]); P = np.stack([p[1] for p in pairs])
        if N == 1:
            G, P = G[0], P[0]
        train = to_train(P, rng)
        check(G, P, R, train if R == 5 or H * W < 4000 else None)


def test_full_size_cityscapes_like_map():
    """One 1024 x 2048 map at R = 8 (the NumPy route takes about a second for it)."""
    rng = np.random.default_rng(12)
    G, P = cityscapes_like(rng, 1, 1024, 2048)
    want = check(G[0], P[0], 8)
    assert want[0][8].sum() > want[0][:8].sum() > 0 and want[1].sum() > 0


def test_noise_and_constant_maps():
    rng = np.random.default_rng(13)
    for R in (3, 16):
        # every pixel a contour pixel: the worst case for the searches and for the atomics
        G = rng.integers(0, 34, (2, 150, 203)).astype(np.uint8); P = rng.integers(0, 34, (2, 150, 203)).astype(np.uint8)
        check(G, P, R, to_train(P, rng) if R == 3 else None)
        G = rng.integers(7, 9, (97, 130)).astype(np.uint8); P = rng.integers(7, 9, (97, 130)).astype(np.uint8)
        check(G, P, R)
        # no boundary at all (the fast path), and a single differing pixel in a corner tile
        G = np.full((200, 300), 23, np.uint8)
        want = check(G, G.copy(), R, np.full((200, 300), 11, np.int64))
        assert want[0][R, 23, 23] == 200 * 300 and want[0].sum() == 200 * 300 and want[1].sum() == 0 and want[2].sum() == 0
        P = G.copy(); P[199, 299] = 7
        check(G, P, R)
        G2 = G.copy(); G2[0, 0] = 7
        check(G2, G, R)


def test_unaligned_buffers():
    rng = np.random.default_rng(14)
    G, P = voronoi_pair(rng, 75, 131, cells=15)
    train = to_train(P, rng)
    want = ce.boundary_counts_numpy(P, G, 5, pred_is_train_ids=False)
    gbuf = torch.zeros(G.size + 16, dtype=torch.uint8, device="cuda"); pbuf = torch.zeros(P.size + 16, dtype=torch.uint8, device="cuda")
    for off in (1, 3):
        gbuf[off:off + G.size] = dev(G).view(-1); pbuf[off:off + P.size] = dev(P).view(-1)
        out = Out(5)
        rc = L().lib.fcn8s_op_boundary_pair(None, ptr(gbuf, off), ptr(pbuf, off), 1, 1, 75, 131, 5, *(ptr(b) for b in out.bufs))
        assert rc == 0
        for a, b in zip(out.tables()[:3], want):
            np.testing.assert_array_equal(a, b)
    # int64 train ids behind a one-byte-off ground truth
    want = ce.boundary_counts_numpy(train, G, 5)
    gbuf[1:1 + G.size] = dev(G).view(-1)
    out = Out(5)
    rc = L().lib.fcn8s_op_boundary_pair(None, ptr(gbuf, 1), ptr(dev(train)), 0, 1, 75, 131, 5, *(ptr(b) for b in out.bufs))
    assert rc == 0
    for a, b in zip(out.tables()[:3], want):
        np.testing.assert_array_equal(a, b)


def test_accumulation_over_calls_and_identical_runs():
    rng = np.random.default_rng(15)
    G1, P1 = cityscapes_like(rng, 2, 300, 420, blk=32)
    G2, P2 = voronoi_pair(rng, 300, 420, cells=30)
    t2 = to_train(P2, rng)
    R = 7
    out, rc = run_op(dev(G1), dev(P1), 1, R)
    assert rc == 0
    _, rc = run_op(dev(G2), dev(t2), 0, R, out=out)
    assert rc == 0
    a = ce.boundary_counts_numpy(P1, G1, R, pred_is_train_ids=False)
    b = ce.boundary_counts_numpy(t2, G2, R)
    for x, y, z in zip(out.tables()[:3], a, b):
        np.testing.assert_array_equal(x, y + z)
    # two runs: the same bits
    g, p = dev(G1), dev(P1)
    o1, _ = run_op(g, p, 1, R); o2, _ = run_op(g, p, 1, R)
    torch.cuda.synchronize()
    for x, y in zip(o1.bufs, o2.bufs):
        assert torch.equal(x, y)


def test_rings_sum_to_the_confusion_matrix_of_cityscapes_pair():
    rng = np.random.default_rng(16)
    G, P = cityscapes_like(rng, 3, 260, 517, blk=32)
    train = to_train(P, rng)
    g, p = dev(G), dev(train)
    out, rc = run_op(g, p, 0, 6)
    assert rc == 0
    conf = torch.zeros(34 * 34, dtype=torch.int64, device="cuda"); counts = torch.zeros((3, 3), dtype=torch.int64, device="cuda")
    assert L().lib.fcn8s_op_cityscapes_pair(None, ptr(g), None, ptr(p), 0, 3, 260 * 517, ptr(conf), None, None, 0, ptr(counts)) == 0
    rings = out.tables()[0]
    np.testing.assert_array_equal(rings.sum(0), conf.cpu().numpy().reshape(34, 34))
    assert rings.sum() == 3 * 260 * 517


def test_out_of_range_ids_land_in_bad_only():
    rng = np.random.default_rng(17)
    G, P = voronoi_pair(rng, 90, 140, cells=12)
    train = to_train(P, rng)
    Gb = G.copy(); Gb[rng.random(G.shape) < 0.01] = 200; Gb[40:44, 60:70] = 34
    tb = train.copy(); tb[rng.random(G.shape) < 0.01] = 20; tb[5, 5] = -1; tb[6, 6] = 1 << 40; tb[70:72, 10:30] = 25
    Pb = P.copy(); Pb[rng.random(G.shape) < 0.01] = 34; Pb[80, 100:120] = 255
    R = 4
    for kind, pred, ids in ((0, tb, np.where((tb >= 0) & (tb < 20), ce.TRAINIDS_TO_IDS_ARRAY[np.clip(tb, 0, 19)], ce.BAD_ID)),
                            (1, Pb, np.where(Pb < 34, Pb, ce.BAD_ID))):
        want = ce.boundary_tables_numpy(np.where(Gb < 34, Gb, ce.BAD_ID).astype(np.uint8), ids.astype(np.uint8), R)
        out, rc = run_op(dev(Gb), dev(pred), kind, R)
        assert rc == 0
        got = out.tables()
        for a, b in zip(got[:3], want[:3]):
            np.testing.assert_array_equal(a, b)
        assert got[3] == want[3] > 0 and got[0].sum() + got[3] == G.size
    # the Python layer refuses such an image on either route
    with pytest.raises(ValueError, match="Unknown label"):
        ce.boundary_counts_device(dev(P), dev(Gb), R)
    with pytest.raises(ValueError, match="train ids"):
        ce.boundary_counts_device(dev(tb), dev(G), R)
    with pytest.raises(ValueError, match="label ids"):
        ce.boundary_counts_device(dev(Pb), dev(G), R)


def test_argument_errors_launch_nothing():
    _lib = L(); lib = _lib.lib
    rng = np.random.default_rng(18)
    G, P = voronoi_pair(rng, 40, 50)
    g, p = dev(G), dev(P)
    out = Out(4)
    for b, n in zip(out.bufs, out.sizes):
        b[:n] = MAGIC
    o = [ptr(b) for b in out.bufs]
    call = lambda gg, pp, kind, N, H, W, R, oo: lib.fcn8s_op_boundary_pair(None, gg, pp, kind, N, H, W, R, *oo)
    assert call(None, ptr(p), 1, 1, 40, 50, 4, o) == _lib.ERR_BAD_ARG
    assert call(ptr(g), None, 1, 1, 40, 50, 4, o) == _lib.ERR_BAD_ARG
    for k in range(4):
        assert call(ptr(g), ptr(p), 1, 1, 40, 50, 4, o[:k] + [None] + o[k + 1:]) == _lib.ERR_BAD_ARG
    assert call(ptr(g), ptr(p), 2, 1, 40, 50, 4, o) == _lib.ERR_BAD_ARG
    assert call(ptr(g), ptr(p), -1, 1, 40, 50, 4, o) == _lib.ERR_BAD_ARG
    assert call(ptr(g), ptr(p), 1, 0, 40, 50, 4, o) == _lib.ERR_BAD_ARG
    assert call(ptr(g), ptr(p), 1, 1, 0, 50, 4, o) == _lib.ERR_BAD_ARG
    assert call(ptr(g), ptr(p), 1, 1, 40, -3, 4, o) == _lib.ERR_BAD_ARG
    assert call(ptr(g), ptr(p), 1, 1, 40, 50, 0, o) == _lib.ERR_BAD_ARG
    assert call(ptr(g), ptr(p), 1, 1, 40, 50, 17, o) == _lib.ERR_BAD_ARG
    assert call(ptr(g), ptr(p), 1, 1, 1 << 16, 1 << 15, 4, o) == _lib.ERR_SHAPE
    assert b"2^31" in lib.fcn8s_last_error(None)
    torch.cuda.synchronize()
    for b in out.bufs:
        assert (b == MAGIC).all()


def test_python_routes_on_device_tensors():
    rng = np.random.default_rng(19)
    G, P = cityscapes_like(rng, 2, 120, 200, blk=32)
    train = to_train(P, rng)
    for a, b in zip(ce.boundary_counts_device(dev(train), dev(G), 6), ce.boundary_counts_numpy(train, G, 6)):
        assert a.dtype == np.int64
        np.testing.assert_array_equal(a, b)
    for a, b in zip(ce.boundary_counts_device(dev(P[0]), dev(G[0]), 6), ce.boundary_counts_numpy(P[0], G[0], 6, pred_is_train_ids=False)):
        np.testing.assert_array_equal(a, b)
    with pytest.raises(ValueError, match="boundary_radius"):
        ce.boundary_counts_device(dev(P), dev(G), 17)
    with pytest.raises(ValueError):
        ce.boundary_counts_device(dev(P).int(), dev(G), 3)
    # the evaluator: the device route and the NumPy route accumulate the same tables and report the same scores
    d = ce.PixelLevelEvaluator(boundary_radius=6); h = ce.PixelLevelEvaluator(boundary_radius=6)
    d.add(dev(train), dev(G)); h.add(train, G)
    d.add(dev(P[1]), dev(G[1]), pred_is_train_ids=False); h.add(P[1], G[1], pred_is_train_ids=False)
    _same(d.results(), h.results())


def _feq(a, b):
    if isinstance(a, (list, tuple)):
        return len(a) == len(b) and all(_feq(x, y) for x, y in zip(a, b))
    if isinstance(a, dict):
        return list(a) == list(b) and all(_feq(a[k], b[k]) for k in a)
    if isinstance(a, np.ndarray):
        return np.array_equal(a, b)
    if isinstance(a, float) and math.isnan(a):
        return isinstance(b, float) and math.isnan(b)
    return a == b


def _same(a, b):
    assert sorted(a) == sorted(b)
    for k in a:
        assert _feq(a[k], b[k]), k


def test_facade_with_and_without_a_radius(tmp_path):
    """evaluate_cityscapes(boundary_radius=4) == predict_and_export_label_ids + evaluate_directory(boundary_radius=4), key by key; with
    None exactly the keys and values of evaluate_directory without a radius."""
    from PIL import Image
    from fcn8s_tensorflow_amd.fcn8s import FCN8s
    m = FCN8s(vgg16_dir='synthetic:3', num_classes=20, widths=SMALL)
    rng = np.random.default_rng(8)
    names = ["aachen_000000_000019", "aachen_000001_000019", "bonn_000002_000019"]
    for nm in names:
        city = nm.split("_")[0]
        (tmp_path / "leftImg8bit" / city).mkdir(parents=True, exist_ok=True); (tmp_path / "gtFine" / city).mkdir(parents=True, exist_ok=True)
        img = np.kron(rng.integers(0, 256, (8, 12, 3)), np.ones((8, 8, 1), np.int64)).astype(np.uint8) + rng.integers(0, 8, (64, 96, 3), dtype=np.uint8) // 2
        gt = np.kron(rng.integers(0, 34, (8, 12)), np.ones((8, 8), np.int64)).astype(np.uint8)
        Image.fromarray(img).save(tmp_path / "leftImg8bit" / city / (nm + "_leftImg8bit.png"))
        Image.fromarray(gt).save(tmp_path / "gtFine" / city / (nm + "_gtFine_labelIds.png"))
        Image.fromarray(gt.astype(np.uint16)).save(tmp_path / "gtFine" / city / (nm + "_gtFine_instanceIds.png"))
    search = str(tmp_path / "gtFine" / "*" / "*_gtFine_labelIds.png")
    images = str(tmp_path / "leftImg8bit")
    out = str(tmp_path / "results")
    assert m.predict_and_export_label_ids(out, images, scales=(1.0,)) == 3
    for inst_level in (True, False):
        res = m.evaluate_cityscapes(images, search, scales=(1.0,), instance_level=inst_level, boundary_radius=4)
        _same(res, ce.evaluate_directory(search, out, instance_level=inst_level, boundary_radius=4))
        _same(res, ce.evaluate_directory(search, out, device="cuda", instance_level=inst_level, boundary_radius=4))
        assert res["boundaryRadius"] == 4 and res["trimapRings"].sum() == 3 * 64 * 96 and res["boundaryRecallCounts"].sum() > 0
        plain = m.evaluate_cityscapes(images, search, scales=(1.0,), instance_level=inst_level)
        want = ce.evaluate_directory(search, out, instance_level=inst_level)
        _same(plain, want)
        assert not set(plain) & set(ce.BOUNDARY_RESULT_KEYS)
        assert sorted(set(res) - set(plain)) == sorted(ce.BOUNDARY_RESULT_KEYS)
    # through a resize the boundary tables are taken on the resized-back label ids, as the IoU is
    res = m.evaluate_cityscapes(images, search, resize=(32, 64), instance_level=False, boundary_radius=4)
    out2 = str(tmp_path / "results_resized")
    m.predict_and_export_label_ids(out2, images, resize=(32, 64))
    _same(res, ce.evaluate_directory(search, out2, boundary_radius=4))
    res = m.evaluate_cityscapes(images, search, scales=(1.0,), boundary_radius=4, json_path=str(tmp_path / "r" / "result.json"))
    import json
    w = json.load(open(tmp_path / "r" / "result.json"))
    assert w["trimapRings"] == res["trimapRings"].tolist() and w["boundaryRadius"] == 4
    with pytest.raises(ValueError, match="boundary_radius"):
        m.evaluate_cityscapes(images, search, boundary_radius=40)
    m.close()
