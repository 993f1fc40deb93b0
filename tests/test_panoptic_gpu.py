"""`fcn8s_op_panoptic_pair` (csrc/panoptic.hip) on the GPU.  Everything is an integer, so the SciPy / dict-counting fixture
(tests/golden/panoptic_cases.npz) and the package's NumPy route of the same definition are compared with `==` after sorting the rows."""
import ctypes as C
import json
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from fcn8s_tensorflow_amd import cityscapes_eval as ce, panoptic as PQ, regions as R  # noqa: E402

HERE = os.path.dirname(os.path.abspath(__file__))
GUARD = 9                                                      # int64 elements behind rows / counts that must come back untouched
SENTINEL = -0x5A5A5A5A5A5A5A5B


def lib():
    from fcn8s_tensorflow_amd import _lib
    return _lib


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def inst_dev(a):
    return dev(np.ascontiguousarray(a).view(np.int16))


def shifted(a, off):
    """A device copy of `a` that starts `off` elements behind a 256-byte boundary."""
    flat = torch.empty(a.numel() + off, dtype=a.dtype, device="cuda")
    flat[off:] = a.reshape(-1)
    return flat[off:].view(a.shape)


@pytest.fixture(scope="module")
def golden():
    z = np.load(os.path.join(HERE, "golden", "panoptic_cases.npz"))
    return z, json.loads(bytes(z["index"]).decode())


def run_op(pred, inst, comp, slots, max_rows, fill=0xFF, stream=None, table=None):
    """One raw call with guards: (rows per image as the op wrote them (at most max_rows each), counts [N, 4])."""
    kind, N, H, W = R._kind(pred)
    nbytes = lib().lib.fcn8s_op_panoptic_work_bytes(N, slots)
    assert nbytes == 16 * N * slots
    if table is None:
        table = torch.full((nbytes + 16 * GUARD,), fill, dtype=torch.uint8, device="cuda")
    tail = table[nbytes:].clone()
    rbuf = torch.full((N * max_rows * 3 + GUARD,), SENTINEL, dtype=torch.int64, device="cuda")
    cbuf = torch.full((N * 4 + GUARD,), SENTINEL, dtype=torch.int64, device="cuda")
    p = lambda t: C.c_void_p(t.data_ptr())
    if stream is not None:
        torch.cuda.synchronize()                                # the buffers above were filled on the current stream
    rc = lib().lib.fcn8s_op_panoptic_pair(C.c_void_p(stream.cuda_stream) if stream is not None else None, p(inst), p(pred), kind, p(comp), N, H, W,
                                          p(table), slots, p(rbuf), max_rows, p(cbuf))
    assert rc == 0, lib().lib.fcn8s_last_error(None)
    (stream.synchronize() if stream is not None else torch.cuda.synchronize())
    assert bool((rbuf[N * max_rows * 3:] == SENTINEL).all()) and bool((cbuf[N * 4:] == SENTINEL).all()) and torch.equal(table[nbytes:], tail)
    counts = cbuf[:N * 4].view(N, 4).cpu().numpy()
    rows = rbuf[:N * max_rows * 3].view(N, max_rows, 3).cpu().numpy()
    written = [rows[n, :min(int(counts[n, 0]), max_rows)] for n in range(N)]
    for n in range(N):                                          # what lies behind the rows written is untouched too
        assert (rows[n, len(written[n]):] == SENTINEL).all()
    return written, counts


def want_of(z, name, conn, images):
    return [z["%s.c%d.rows%d" % (name, conn, k)] for k in range(images)], z["%s.c%d.bad" % (name, conn)]


def check(written, counts, want_rows, want_bad, pixels, where):
    for n, (got, want) in enumerate(zip(written, want_rows)):
        assert counts[n].tolist() == [len(want), int(want_bad[n]), 0, pixels - int(want_bad[n])], (where, n, counts[n])
        assert np.array_equal(PQ.sort_rows(got), want), (where, n)


def test_op_equals_the_fixture(golden):
    """Every case, both connectivities, int64 train ids and uint8 label ids, scratch prefilled with 0xFF and 0x00, guards behind everything."""
    z, index = golden
    for case in index:
        name, pred, inst = case["name"], z[case["name"] + ".pred"], z[case["name"] + ".inst"]
        pixels = pred.size // case["images"]
        for conn in (4, 8):
            want_rows, want_bad = want_of(z, name, conn, case["images"])
            for fill, t in ((0xFF, dev(pred.astype(np.int64))), (0x00, dev(ce.TRAINIDS_TO_IDS_ARRAY[pred]))):
                comp, _a, _w = R.label_device(t, connectivity=conn, area=False)
                written, counts = run_op(t, inst_dev(inst), comp, 4096, 2048, fill=fill)
                check(written, counts, want_rows, want_bad, pixels, (name, conn, str(t.dtype)))


def test_every_pointer_offset(golden):
    """Each input 0..7 elements off a 16-byte boundary, one at a time and all three at odds with each other: wide and scalar loads of every array."""
    z, _ = golden
    name = "batch2_48x80"                                        # 3840 pixels per image: a body of full groups, a head and a tail
    pred, inst = z[name + ".pred"], z[name + ".inst"]
    want_rows, want_bad = want_of(z, name, 4, 2)
    for kind_pred in (pred.astype(np.int64), ce.TRAINIDS_TO_IDS_ARRAY[pred]):
        base = dev(kind_pred)
        comp0, _a, _w = R.label_device(base, connectivity=4, area=False)
        i0 = inst_dev(inst)
        offsets = [(o, 0, 0) for o in range(8)] + [(0, o, 0) for o in range(1, 8)] + [(0, 0, o) for o in range(1, 8)] + [(1, 3, 5), (7, 2, 1), (4, 4, 4)]
        for oi, op, oc in offsets:
            written, counts = run_op(shifted(base, op), shifted(i0, oi), shifted(comp0, oc), 1024, 512)
            check(written, counts, want_rows, want_bad, 48 * 80, (str(base.dtype), oi, op, oc))
    # images of 2145 pixels: the second and third start off every boundary, so each has a head of scalar loads in front of its body
    one_p, one_i = z["scene_33x65.pred"], z["scene_33x65.inst"]
    pred = np.stack([one_p, np.roll(one_p, 7, 1), one_p.T.reshape(33, 65)]); inst = np.stack([one_i, one_i, np.roll(one_i, 3, 0)])
    want_rows, want_bad = PQ.pair_rows_numpy(pred, inst, 8)
    assert np.array_equal(want_rows[0], z["scene_33x65.c8.rows0"])
    for base in (dev(pred.astype(np.int64)), dev(ce.TRAINIDS_TO_IDS_ARRAY[pred])):
        comp0, _a, _w = R.label_device(base, connectivity=8, area=False)
        for oi, op, oc in ((0, 0, 0), (3, 1, 2)):
            written, counts = run_op(shifted(base, op), shifted(inst_dev(inst), oi), shifted(comp0, oc), 1024, 512)
            check(written, counts, want_rows, want_bad, 33 * 65, ("odd images", str(base.dtype), oi, op, oc))


def _every_pixel_its_own_pair(H, W):
    yy, xx = np.mgrid[0:H, 0:W]
    pred = np.where((yy + xx) % 2 == 0, 14, 15).astype(np.int64)          # a checkerboard of cars and trucks: every pixel a component (4-connectivity)
    inst = (26000 + (yy * W + xx) % 1000).astype(np.uint16)               # and per-pixel instance values
    return pred, inst


def test_block_exceeds_its_lds_table_and_constant_map():
    H, W = 64, 128                                              # 8192 pairs on two blocks of 4096 pixels: twice the 2048 LDS entries each
    pred, inst = _every_pixel_its_own_pair(H, W)
    want, bad = PQ.pair_rows_numpy(pred, inst, 4)
    assert len(want) == H * W and bad == 0 and (want[:, 2] == 1).all()
    t = dev(pred)
    comp, _a, _w = R.label_device(t, connectivity=4, area=False)
    written, counts = run_op(t, inst_dev(inst), comp, 1 << 14, H * W)
    check(written, counts, [want], [0], H * W, "every pixel its own pair")
    # a constant map: one row
    for value, v in ((14, 26001), (1, 7), (0, 0)):
        t = dev(np.full((H, W), value, np.int64))
        comp, _a, _w = R.label_device(t, connectivity=4, area=False)
        written, counts = run_op(t, inst_dev(np.full((H, W), v, np.uint16)), comp, 256, 4)
        kp = int(PQ.pred_keys([value], [0])[0]); kg = int(PQ.gt_keys([v])[0])
        assert counts.tolist() == [[1, 0, 0, H * W]] and written[0].tolist() == [[kp, kg, H * W]]


def test_table_or_rows_too_small_are_reported_and_recovered(golden):
    z, _ = golden
    name = "scene_64x128"
    pred, inst = z[name + ".pred"], z[name + ".inst"]
    want_rows, want_bad = want_of(z, name, 4, 1)
    K = len(want_rows[0])
    assert K > 64
    t, i = dev(pred.astype(np.int64)), inst_dev(inst)
    comp, _a, _w = R.label_device(t, connectivity=4, area=False)
    # max_rows too small: the count is exact, max_rows rows were written (run_op checks that nothing lies behind them), each of them a true row
    written, counts = run_op(t, i, comp, 1024, 16)
    assert counts[0].tolist() == [K, int(want_bad[0]), 0, pred.size - int(want_bad[0])] and len(written[0]) == 16
    true_rows = set(map(tuple, want_rows[0].tolist()))
    assert all(tuple(r) in true_rows for r in written[0].tolist()) and len(set(map(tuple, written[0].tolist()))) == 16
    # slots too small: the flag is up, the pixels counted are fewer than the image, nothing is written out of bounds
    for slots in (1, 16, 64):
        written, counts = run_op(t, i, comp, slots, 512)
        assert counts[0, 2] == 1 and counts[0, 0] <= slots and counts[0, 1] == want_bad[0] and counts[0, 3] < pred.size - want_bad[0], (slots, counts)
    # pair_rows_device recovers the exact rows from either start, and from both
    for kw in (dict(slots_per_image=16), dict(max_rows=3), dict(slots_per_image=1, max_rows=1)):
        rows, bad, work = PQ.pair_rows_device(t, i, connectivity=4, **kw)
        assert np.array_equal(rows[0], want_rows[0]) and bad.tolist() == want_bad.tolist(), kw
    # a table of 2 H W slots is probed in full: every pixel its own pair at load 1 / 2
    p2, i2 = _every_pixel_its_own_pair(16, 32)
    t2 = dev(p2)
    comp2, _a, _w = R.label_device(t2, connectivity=4, area=False)
    written, counts = run_op(t2, inst_dev(i2), comp2, 2 * 16 * 32, 16 * 32)
    check(written, counts, [PQ.pair_rows_numpy(p2, i2, 4)[0]], [0], 16 * 32, "full table")


def test_two_runs_and_a_side_stream_give_the_same_bits(golden):
    z, _ = golden
    name = "batch2_48x80"
    pred, inst = z[name + ".pred"], z[name + ".inst"]
    want_rows, want_bad = want_of(z, name, 8, 2)
    t, i = dev(pred.astype(np.int64)), inst_dev(inst)
    comp, _a, _w = R.label_device(t, connectivity=8, area=False)
    a, ca = run_op(t, i, comp, 2048, 512)
    b, cb = run_op(t, i, comp, 2048, 512, fill=0x00)
    assert np.array_equal(ca, cb) and all(np.array_equal(PQ.sort_rows(x), PQ.sort_rows(y)) for x, y in zip(a, b))
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    written, counts = run_op(t, i, comp, 2048, 512, stream=side)
    check(written, counts, want_rows, want_bad, 48 * 80, "side stream")
    with torch.cuda.stream(side):                               # the Python route on the current stream
        rows, bad, _w = PQ.pair_rows_device(t, i, connectivity=8)
    assert all(np.array_equal(x, y) for x, y in zip(rows, want_rows)) and bad.tolist() == want_bad.tolist()


def test_large_salted_maps_equal_the_numpy_route():
    rng = np.random.default_rng(5)
    N, H, W = 2, 512, 1024
    yy, xx = np.mgrid[0:H, 0:W]
    cells = 40
    py, px = rng.integers(0, H, cells), rng.integers(0, W, cells)
    val = rng.choice([7, 8, 11, 21, 23, 26001, 26002, 24001, 25001, 28001, 26, 4, 0], cells)
    one = val[np.argmin((yy[..., None] - py) ** 2 + (xx[..., None] - px) ** 2, -1)]
    inst = np.stack([one, np.roll(one, (100, 300), (0, 1))]).astype(np.uint16)
    lab = np.where(inst < 1000, inst, inst // 1000)
    pred = ce.IDS_TO_TRAINIDS_ARRAY[lab].astype(np.int64)
    salt = rng.random((N, H, W)) < 0.05
    pred[salt] = rng.integers(0, 20, int(salt.sum()))
    want, wbad = PQ.pair_rows_numpy(pred, inst, 4)
    assert min(len(w) for w in want) > 5000                     # thousands of speck segments per image: more rows than the default max_rows
    rows, bad, work = PQ.pair_rows_device(dev(pred), inst_dev(inst), connectivity=4)
    assert all(np.array_equal(a, b) for a, b in zip(rows, want)) and bad.tolist() == list(wbad)
    assert work["max_rows"] >= max(len(w) for w in want) and work["slots"] >= PQ.default_slots(H, W)      # where the next call on this work starts
    # the engine-style reuse of the scratch: a second call on the same work gives the same rows
    rows2, _b, work2 = PQ.pair_rows_device(dev(pred), inst_dev(inst), connectivity=4, work=work)
    assert all(np.array_equal(a, b) for a, b in zip(rows2, want)) and work2["table"].data_ptr() == work["table"].data_ptr()


def test_refusals():
    L = lib()
    t = torch.zeros((4, 8), dtype=torch.int64, device="cuda"); i = torch.zeros((4, 8), dtype=torch.int16, device="cuda")
    comp = torch.zeros((4, 8), dtype=torch.int32, device="cuda")
    table = torch.zeros(16 * 64 + 16, dtype=torch.uint8, device="cuda"); rows = torch.zeros(3 * 8, dtype=torch.int64, device="cuda")
    counts = torch.full((4,), 77, dtype=torch.int64, device="cuda")
    p = lambda x, off=0: C.c_void_p(x.data_ptr() + off) if x is not None else None
    call = lambda inst=i, pred=t, kind=0, cp=comp, N=1, H=4, W=8, work=p(table), slots=64, r=rows, mr=8, c=counts: \
        L.lib.fcn8s_op_panoptic_pair(None, p(inst), p(pred), kind, p(cp), N, H, W, work, slots, p(r), mr, p(c))
    assert call() == L.OK
    for kw in (dict(inst=None), dict(pred=None), dict(cp=None), dict(work=None), dict(r=None), dict(c=None), dict(kind=2), dict(N=0), dict(H=0), dict(W=-1),
               dict(mr=0), dict(slots=0), dict(slots=48), dict(slots=-64), dict(slots=1 << 29), dict(work=p(table, 8))):
        counts.fill_(77)
        assert call(**kw) == L.ERR_BAD_ARG, kw
        torch.cuda.synchronize()
        assert kw.get("c", counts) is None or (counts == 77).all()        # nothing was launched
    assert call(H=8192, W=8193) == L.ERR_SHAPE and call(N=65536) == L.ERR_SHAPE
    assert L.lib.fcn8s_op_panoptic_work_bytes(2, 1024) == 2 * 1024 * 16
    for bad in ((0, 64), (1, 0), (1, 48), (1, 1 << 29)):
        assert L.lib.fcn8s_op_panoptic_work_bytes(*bad) == 0
    with pytest.raises(ValueError):
        PQ.pair_rows_device(t.to(torch.int32), i)
    with pytest.raises(ValueError):
        PQ.pair_rows_device(t, i, connectivity=6)
    with pytest.raises(ValueError):
        PQ.pair_rows_device(t, i, slots_per_image=48)
    with pytest.raises(ValueError):
        PQ.pair_rows_device(t, i[:2])
