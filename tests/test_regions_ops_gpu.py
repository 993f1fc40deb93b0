"""`fcn8s_op_regions_label` and `fcn8s_op_regions_clean` (csrc/regions.hip) on the GPU.  Everything is an integer, so the SciPy-derived fixture
(tests/golden/region_cases.npz) and the package's NumPy route of the same definition are compared with `==`."""
import ctypes as C
import json
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from fcn8s_tensorflow_amd import regions as R  # noqa: E402

HERE = os.path.dirname(os.path.abspath(__file__))
GUARD = 7                                                      # elements behind each output that must come back untouched
SENTINEL = -0x5A5A5A5B


def lib():
    from fcn8s_tensorflow_amd import _lib
    return _lib


def ptr(t, offset=0):
    return C.c_void_p(t.data_ptr() + offset) if t is not None else None


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


@pytest.fixture(scope="module")
def golden():
    z = np.load(os.path.join(HERE, "golden", "region_cases.npz"))
    return z, json.loads(bytes(z["index"]).decode())


def nhw(L):
    return ((1,) + tuple(L.shape)) if L.ndim == 2 else tuple(L.shape)


def make_work(N, H, W, fill):
    n = lib().lib.fcn8s_op_regions_work_bytes(N, H, W)
    assert n >= 16 * N * H * W and n <= 16 * N * H * W + 8192          # 16 bytes per pixel and a header
    return torch.full((n,), fill, dtype=torch.uint8, device="cuda")


def guarded(shape, dtype):
    """An output of `shape` followed by GUARD sentinels, all sentinel to begin with."""
    n = int(np.prod(shape))
    buf = torch.full((n + GUARD,), SENTINEL if dtype != torch.uint8 else 0xA5, dtype=dtype, device="cuda")
    return buf, buf[:n].view(shape)


def guard_ok(buf, n):
    return bool((buf[n:] == (SENTINEL if buf.dtype != torch.uint8 else 0xA5)).all())


def run_label(labels, conn, work, area=True):
    N, H, W = nhw(labels)
    kind = 0 if labels.dtype == torch.int64 else 1
    cbuf, comp = guarded(labels.shape, torch.int32)
    abuf, ar = guarded(labels.shape, torch.int32) if area else (None, None)
    rc = lib().lib.fcn8s_op_regions_label(None, ptr(labels), kind, N, H, W, conn, ptr(comp), ptr(ar), ptr(work))
    assert rc == 0, lib().lib.fcn8s_last_error(None)
    torch.cuda.synchronize()
    assert guard_ok(cbuf, comp.numel()) and (abuf is None or guard_ok(abuf, ar.numel()))
    assert R.status_device(work) == (0, 0)
    return comp.cpu().numpy(), (ar.cpu().numpy() if area else None)


def run_clean(labels, table, conn, rounds, work, stats=True):
    """In place on `labels` (a device tensor); returns the stats."""
    N, H, W = nhw(labels)
    kind = 0 if labels.dtype == torch.int64 else 1
    sbuf, st = guarded((rounds, 4), torch.int64) if stats else (None, None)
    rc = lib().lib.fcn8s_op_regions_clean(None, ptr(labels), kind, N, H, W, conn, ptr(table), rounds, ptr(work), ptr(st))
    assert rc == 0, lib().lib.fcn8s_last_error(None)
    torch.cuda.synchronize()
    assert sbuf is None or guard_ok(sbuf, st.numel())
    assert R.status_device(work) == (0, 0)
    return st.cpu().numpy() if stats else None


def test_label_equals_the_fixture(golden):
    """int64 and uint8 maps, area_out NULL and not, the scratch prefilled with 0xFF and with zeros, one work buffer for every shape."""
    z, index = golden
    biggest = max(int(np.prod(nhw(z[c["name"] + ".L"]))) for c in index)
    for fill in (0xFF, 0x00):
        work = make_work(1, 1, biggest, fill)                          # reused across all shapes
        for case in index:
            name, L = case["name"], z[case["name"] + ".L"]
            for conn in (4, 8):
                want_c, want_a = z["%s.c%d.comp" % (name, conn)], z["%s.c%d.area" % (name, conn)]
                for t in (dev(L.astype(np.int64)), dev(L)):
                    comp, area = run_label(t, conn, work)
                    assert np.array_equal(comp, want_c), (name, conn, t.dtype)
                    assert np.array_equal(area, want_a), (name, conn, t.dtype)
                comp, area = run_label(dev(L), conn, work, area=False)
                assert area is None and np.array_equal(comp, want_c), (name, conn, "no area")


def test_clean_equals_the_fixture(golden):
    """int64 and uint8 maps, stats NULL and not, both scratch prefills, one work buffer for every shape, two runs bit-identical."""
    z, index = golden
    shapes = [nhw(z[c["name"] + ".L"]) for c in index]
    work_bytes = max(lib().lib.fcn8s_op_regions_work_bytes(*s) for s in shapes)
    for fill in (0xFF, 0x00):
        work = torch.full((work_bytes,), fill, dtype=torch.uint8, device="cuda")
        for case in index:
            name, L = case["name"], z[case["name"] + ".L"]
            for conn in (4, 8):
                for cfg in case["configs"]:
                    key = "%s.c%d.%s.r%d" % (name, conn, cfg["tag"], cfg["rounds"])
                    table = dev(z["%s.T.%s" % (name, cfg["tag"])])
                    outs = []
                    for t in (dev(L.astype(np.int64)), dev(L), dev(L)):
                        st = run_clean(t, table, conn, cfg["rounds"], work)
                        assert np.array_equal(t.cpu().numpy().astype(np.uint8), z[key + ".out"]), (key, t.dtype)
                        assert np.array_equal(st, z[key + ".stats"]), (key, t.dtype)
                        outs.append(t)
                    assert torch.equal(outs[1], outs[2])                # two runs: the same bits
                    if fill == 0xFF:
                        t = dev(L)
                        assert run_clean(t, table, conn, cfg["rounds"], work, stats=False) is None
                        assert np.array_equal(t.cpu().numpy(), z[key + ".out"]), (key, "no stats")


def test_uint8_maps_at_every_pointer_offset(golden):
    z, _ = golden
    name = "voronoi_70x131_s30"                                        # W = 131: no row but the first starts on a multiple of 4
    L = z[name + ".L"]
    H, W = L.shape
    work = make_work(1, H, W, 0xFF)
    table = dev(z[name + ".T.m16"])
    for off in range(4):
        buf = torch.full((H * W + 8,), 0xA5, dtype=torch.uint8, device="cuda")
        view = buf[off:off + H * W].view(H, W)
        for conn in (4, 8):
            view.copy_(dev(L))
            comp, area = run_label(view, conn, work)
            assert np.array_equal(comp, z["%s.c%d.comp" % (name, conn)]) and np.array_equal(area, z["%s.c%d.area" % (name, conn)]), (off, conn)
            st = run_clean(view, table, conn, 4, work)
            assert np.array_equal(view.cpu().numpy(), z["%s.c%d.m16.r4.out" % (name, conn)]), (off, conn)
            assert np.array_equal(st, z["%s.c%d.m16.r4.stats" % (name, conn)]), (off, conn)
            assert (buf[:off] == 0xA5).all() and (buf[off + H * W:] == 0xA5).all()
    # an int64 map on an address that is 8 but not 16 modulo 16: the paired loads fall back to single ones
    buf = torch.zeros(H * W + 1, dtype=torch.int64, device="cuda")
    view = buf[1:].view(H, W)
    view.copy_(dev(L.astype(np.int64)))
    assert view.data_ptr() % 16 == 8
    comp, area = run_label(view, 8, work)
    assert np.array_equal(comp, z[name + ".c8.comp"]) and np.array_equal(area, z[name + ".c8.area"])
    run_clean(view, table, 8, 4, work)
    assert np.array_equal(view.cpu().numpy(), z[name + ".c8.m16.r4.out"])


def _voronoi(rng, H, W, cells, salt):
    py, px, cl = rng.integers(0, H, cells), rng.integers(0, W, cells), rng.integers(0, 20, cells)
    yy, xx = np.mgrid[0:H, 0:W]
    best = np.full((H, W), np.iinfo(np.int64).max)
    L = np.zeros((H, W), np.int64)
    for k in range(cells):
        d = (yy - py[k]) ** 2 + (xx - px[k]) ** 2
        m = d < best
        best[m] = d[m]; L[m] = cl[k]
    m = rng.random((H, W)) < salt
    L[m] = rng.integers(0, 20, int(m.sum()))
    return L


def test_a_large_salted_voronoi_batch_against_the_numpy_route():
    """512 x 1024, N = 2: 16 x 16 tiles per image.  Against regions.py with ==, and the cheap invariants on the device."""
    rng = np.random.default_rng(77)
    H, W = 512, 1024
    L = np.stack([_voronoi(rng, H, W, 60, 0.05), _voronoi(rng, H, W, 200, 0.10)])
    t = dev(L)
    work = make_work(2, H, W, 0xFF)
    idx = torch.arange(H * W, device="cuda", dtype=torch.int32).view(1, H, W)
    for conn in (4, 8):
        want_c, want_a = R.components_numpy(L, conn)
        cbuf, comp = guarded(t.shape, torch.int32)
        abuf, area = guarded(t.shape, torch.int32)
        assert lib().lib.fcn8s_op_regions_label(None, ptr(t), 0, 2, H, W, conn, ptr(comp), ptr(area), ptr(work)) == 0
        torch.cuda.synchronize()
        assert guard_ok(cbuf, comp.numel()) and guard_ok(abuf, area.numel()) and R.status_device(work) == (0, 0)
        # invariants, on the device: an id is at most the pixel's index; equal-class neighbours share it
        assert bool((comp <= idx).all()) and bool((comp >= 0).all())
        same = t[:, :, 1:] == t[:, :, :-1]
        assert bool((comp[:, :, 1:][same] == comp[:, :, :-1][same]).all())
        same = t[:, 1:, :] == t[:, :-1, :]
        assert bool((comp[:, 1:, :][same] == comp[:, :-1, :][same]).all())
        for a, b in (((slice(1, None), slice(1, None)), (slice(0, -1), slice(0, -1))), ((slice(1, None), slice(0, -1)), (slice(0, -1), slice(1, None)))):
            same = t[:, a[0], a[1]] == t[:, b[0], b[1]]
            if conn == 8:
                assert bool((comp[:, a[0], a[1]][same] == comp[:, b[0], b[1]][same]).all())
        assert np.array_equal(comp.cpu().numpy(), want_c) and np.array_equal(area.cpu().numpy(), want_a)
        want, want_st = R.clean_numpy(L, 16, conn, 2)
        u = t.clone()
        st = run_clean(u, dev(np.full(256, 16, np.int32)), conn, 2, work)
        assert np.array_equal(u.cpu().numpy(), want) and np.array_equal(st, want_st)
        assert want_st[0, 3] > 0.03 * L.size                           # the salt is what goes


def test_labels_out_of_range_in_an_int64_map():
    M = np.full((40, 70), 1, np.int64)
    M[2, 2] = 300; M[2, 3] = 300; M[4, 4] = 2; M[0, 0] = 9; M[0, 1] = -1; M[35, 66] = 1 << 40; M[35, 65] = 3
    work = make_work(1, 40, 70, 0xFF)
    for conn in (4, 8):
        want_c, want_a = R.components_numpy(M, conn)
        N, H, W = 1, 40, 70
        comp = torch.empty((H, W), dtype=torch.int32, device="cuda"); area = torch.empty_like(comp)
        assert lib().lib.fcn8s_op_regions_label(None, ptr(dev(M)), 0, N, H, W, conn, ptr(comp), ptr(area), ptr(work)) == 0
        assert R.status_device(work) == (0, 4)                         # four such pixels, counted
        assert np.array_equal(comp.cpu().numpy(), want_c) and np.array_equal(area.cpu().numpy(), want_a)
        want, want_st = R.clean_numpy(M, 4, conn, 2)
        t = dev(M)
        st = torch.empty((2, 4), dtype=torch.int64, device="cuda")
        assert lib().lib.fcn8s_op_regions_clean(None, ptr(t), 0, N, H, W, conn, ptr(dev(np.full(256, 4, np.int32))), 2, ptr(work), ptr(st)) == 0
        assert R.status_device(work) == (0, 4)
        assert np.array_equal(t.cpu().numpy(), want) and np.array_equal(st.cpu().numpy(), want_st)
        assert want[2, 2] == 300 and want[35, 66] == 1 << 40 and want[0, 0] == 1 and want[35, 65] == 1


def test_refusals_launch_nothing():
    _lib = lib()
    H, W = 40, 70
    L = dev(np.random.default_rng(5).integers(0, 20, (H, W)).astype(np.int64))
    before = L.clone()
    comp = torch.full((H, W), SENTINEL, dtype=torch.int32, device="cuda"); area = comp.clone()
    st = torch.full((8, 4), SENTINEL, dtype=torch.int64, device="cuda")
    work = make_work(1, H, W, 0x5A)
    table = dev(np.full(256, 16, np.int32))
    BAD, SHAPE = _lib.ERR_BAD_ARG, _lib.ERR_SHAPE
    label = lambda labels=L, kind=0, N=1, H=H, W=W, conn=4, c=comp, a=area, w=work, off=0: \
        _lib.lib.fcn8s_op_regions_label(None, ptr(labels), kind, N, H, W, conn, ptr(c), ptr(a), ptr(w, off) if w is not None else None)
    clean = lambda labels=L, kind=0, N=1, H=H, W=W, conn=4, t=table, rounds=1, w=work, s=st, off=0: \
        _lib.lib.fcn8s_op_regions_clean(None, ptr(labels), kind, N, H, W, conn, ptr(t), rounds, ptr(w, off) if w is not None else None, ptr(s))
    assert label(labels=None) == BAD and label(c=None) == BAD and label(w=None) == BAD and label(off=8) == BAD
    assert label(kind=2) == BAD and label(kind=-1) == BAD and label(conn=6) == BAD and label(conn=0) == BAD
    assert label(N=0) == BAD and label(H=0) == BAD and label(W=-3) == BAD
    assert label(H=1 << 16, W=1 << 15) == SHAPE and label(N=65536) == SHAPE
    assert clean(labels=None) == BAD and clean(t=None) == BAD and clean(w=None) == BAD and clean(off=8) == BAD
    assert clean(kind=2) == BAD and clean(conn=5) == BAD and clean(rounds=0) == BAD and clean(rounds=9) == BAD
    assert clean(N=0) == BAD and clean(H=-1) == BAD and clean(W=0) == BAD
    assert clean(H=1 << 16, W=1 << 15) == SHAPE and clean(N=65536) == SHAPE
    assert b"regions" in _lib.lib.fcn8s_last_error(None)
    torch.cuda.synchronize()
    assert bool((comp == SENTINEL).all()) and bool((area == SENTINEL).all()) and bool((st == SENTINEL).all())
    assert bool((work == 0x5A).all()) and torch.equal(L, before)
    assert _lib.lib.fcn8s_op_regions_work_bytes(0, 4, 4) == 0 and _lib.lib.fcn8s_op_regions_work_bytes(1, -4, 4) == 0
    assert _lib.lib.fcn8s_op_regions_work_bytes(1, 1 << 16, 1 << 15) == 0


def test_engine_methods_keep_one_work_buffer():
    from fcn8s_tensorflow_amd.engine import Engine
    e = Engine(20, widths=(8, 16, 32, 64, 64, 128, 128), device_id=0)
    z = np.load(os.path.join(HERE, "golden", "region_cases.npz"))
    L = z["batch2_45x70.L"]
    t = dev(L.astype(np.int64))
    st = e.regions_clean(t, 16, connectivity=8, rounds=3, stats=True)
    assert np.array_equal(t.cpu().numpy(), z["batch2_45x70.c8.m16.r3.out"]) and np.array_equal(st.cpu().numpy(), z["batch2_45x70.c8.m16.r3.stats"])
    w = e._regions_work
    comp, area = e.regions_label(dev(L), connectivity=4)
    assert comp.dtype == torch.int32 and np.array_equal(comp.cpu().numpy(), z["batch2_45x70.c4.comp"]) and np.array_equal(area.cpu().numpy(), z["batch2_45x70.c4.area"])
    comp, area = e.regions_label(dev(L[0]), connectivity=8, area=False)
    assert area is None and np.array_equal(comp.cpu().numpy(), z["batch2_45x70.c8.comp"][0])
    assert e.regions_clean(dev(L[0]), 4) is None and e._regions_work is w          # a smaller call: the same buffer
    big = dev(np.zeros((3, 64, 128), np.uint8))
    e.regions_clean(big, 4)
    assert e._regions_work is not w and e._regions_work.numel() >= 16 * big.numel()
    for bad in (t.float(), t.cpu(), t[:, :, ::2]):
        with pytest.raises(ValueError):
            e.regions_clean(bad, 4)
    with pytest.raises(ValueError):
        e.regions_clean(t, 4, connectivity=6)
    with pytest.raises(ValueError):
        e.regions_clean(t, 4, rounds=9)
    e.close()
