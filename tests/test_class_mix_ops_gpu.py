"""`fcn8s_op_class_mix` (csrc/class_mix.hip) against tests/golden/class_mix_cases.npz and `class_mix.mix_numpy` with `==` in the mixed images,
the mixed labels and the table of selected classes: nothing but integers decides anything.

Shapes are the smallest at which each path of the kernels can go wrong: the fixture's pixel counts around a 16-byte line and around the mix
kernel's tile of 1024 pixels (1, 15, 16, 17, 255 .. 257, 1023, 1025, a batch of 3 x 300, whose images start at every alignment), C = 2 .. 255
(classes from 64 on take the presence kernel's LDS path), every byte offset of the four pixel streams within a line (offsets that are multiples
of 4 keep the mix kernel on its dword path, the others put it on the byte path), guard bytes around every output, and one 2 x 512 x 1024 batch
(several trips per block)."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from fcn8s_tensorflow_amd import _lib as L, class_mix as CM  # noqa: E402
from tests.test_class_mix_host import golden, case_ids, pick  # noqa: E402
from tests.test_pseudo_label_ops_gpu import dev_at, ptr  # noqa: E402

GUARD = 0xA5
PAD = 64


def guarded(nbytes, off=0, fill=GUARD):
    """(buffer, view): `nbytes` bytes at byte offset `off` behind PAD guard bytes, PAD more behind them."""
    buf = torch.full((PAD + off + nbytes + PAD,), GUARD, dtype=torch.uint8, device="cuda")
    view = buf[PAD + off: PAD + off + nbytes]
    if fill != GUARD:
        view.fill_(fill)
    return buf, view


def guards_hold(buf, off, nbytes):
    b = buf.cpu().numpy()
    return (b[:PAD + off] == GUARD).all() and (b[PAD + off + nbytes:] == GUARD).all()


class Call:
    """The device buffers of one call: inputs at their offsets, outputs, work and selected_out between guard bytes."""

    def __init__(self, images, labels, src, img_off=0, lab_off=0, oimg_off=0, olab_off=0, work_off=0, work_fill=0xFF, selected=True):
        self.N, self.P = labels.shape[0], int(np.prod(labels.shape[1:]))
        T = self.N * self.P
        self.images, self.labels = dev_at(images, img_off), dev_at(labels, lab_off)
        self.src = dev_at(np.asarray(src, np.int32))
        self.offs = (oimg_off, olab_off, work_off)
        self.oi_buf, self.oi = guarded(3 * T, oimg_off)
        self.ol_buf, self.ol = guarded(T, olab_off)
        self.wbytes = CM.work_bytes(self.N)
        self.w_buf, self.w = guarded(self.wbytes, work_off, work_fill)
        self.sel_buf, self.sel = guarded(self.N * 256) if selected else (None, None)

    def run(self, Cn, seed_, draw_, stream=None, **over):
        a = dict(images=self.images, labels=self.labels, src=self.src, N=self.N, P=self.P, C=Cn, seed=seed_, draw=draw_, work=self.w, oi=self.oi,
                 ol=self.ol, sel=self.sel)
        a.update(over)
        return L.lib.fcn8s_op_class_mix(stream, ptr(a["images"]), ptr(a["labels"]), ptr(a["src"]), a["N"], a["P"], a["C"], a["seed"], a["draw"],
                                        ptr(a["work"]), ptr(a["oi"]), ptr(a["ol"]), ptr(a["sel"]))

    def fetch(self):
        """(out_images [N,P,3], out_labels [N,P], selected [N,256] | None, flag) after checking every guard."""
        torch.cuda.synchronize()
        T = self.N * self.P
        assert guards_hold(self.oi_buf, self.offs[0], 3 * T), "a byte outside out_images was written"
        assert guards_hold(self.ol_buf, self.offs[1], T), "a byte outside out_labels was written"
        assert guards_hold(self.w_buf, self.offs[2], self.wbytes), "a byte outside work was written"
        sel = None
        if self.sel is not None:
            assert guards_hold(self.sel_buf, 0, self.N * 256), "a byte outside selected_out was written"
            sel = self.sel.cpu().numpy().reshape(self.N, 256)
        return (self.oi.cpu().numpy().reshape(self.N, self.P, 3), self.ol.cpu().numpy().reshape(self.N, self.P), sel, CM.flag_of(self.w, self.N))


def run(c, src=None, **kw):
    call = Call(c["images"], c["labels"], c["src"] if src is None else src, **kw)
    L.check(call.run(c["C"], c["seed"], c["draw"]))
    return call.fetch()


def same(got, c, tag=""):
    for g, name in zip(got[:3], ("out_images", "out_labels", "selected")):
        if g is not None:
            assert g.shape == c[name].shape and (g == c[name]).all(), (tag, name, np.argwhere(g != c[name])[:8])


@pytest.mark.parametrize("i", range(len(golden())), ids=case_ids())
def test_the_op_equals_the_fixture(i):
    c = golden()[i]
    got = run(c)
    same(got, c)
    assert got[3] == 0


@pytest.mark.parametrize("off", range(16))
def test_every_byte_offset_of_every_pixel_stream(off):
    for c in (pick(1025, 20), pick(300, 20, 3), pick(17, 21)):
        for which in ("img_off", "lab_off", "oimg_off", "olab_off"):
            same(run(c, **{which: off}), c, "%s = %d" % (which, off))
        same(run(c, img_off=off, lab_off=(5 * off + 3) % 16, oimg_off=(7 * off + 1) % 16, olab_off=(3 * off + 2) % 16, work_off=off), c, "all, %d" % off)


@pytest.mark.parametrize("fill", [0xFF, 0x00])
def test_the_prior_content_of_work_does_not_matter(fill):
    for c in (pick(257, 255), pick(300, 20, 3)):
        same(run(c, work_fill=fill), c, "work prefilled with %#x" % fill)


def test_selected_out_may_be_null():
    c = pick(300, 20, 3)
    got = run(c, selected=False)
    assert got[2] is None
    same(got, c)


def test_two_runs_give_the_same_bits():
    c = pick(1025, 20)
    one, two = run(c), run(c)
    assert all(x.tobytes() == y.tobytes() for x, y in zip(one[:3], two[:3]))


def test_bad_arguments_return_their_code_and_leave_the_outputs_untouched():
    c = pick(257, 20)
    call = Call(c["images"], c["labels"], c["src"])
    T = 2 * 257
    bad = [dict(images=None), dict(labels=None), dict(src=None), dict(work=None), dict(oi=None), dict(ol=None), dict(N=0), dict(N=-1), dict(P=0),
           dict(P=-5), dict(C=1), dict(C=0), dict(C=256), dict(draw=1 << 48), dict(draw=(1 << 64) - 1),
           dict(oi=call.images), dict(ol=call.labels), dict(oi=call.labels), dict(ol=call.images[3 * T - 1:]), dict(oi=call.images[5:]),
           dict(ol=call.src.view(torch.uint8)[4:])]
    for kw in bad:
        assert call.run(20, 1, 2, **kw) == L.ERR_BAD_ARG, kw
    assert call.run(20, 1, 2, N=257) == L.ERR_SHAPE
    assert call.run(20, 1, 2, P=1 << 31) == L.ERR_SHAPE
    oi, ol, sel, _ = call.fetch()
    assert (oi == GUARD).all() and (ol == GUARD).all() and (sel == GUARD).all()
    assert (call.images.cpu().numpy() == c["images"].reshape(-1)).all() and (call.labels.cpu().numpy() == c["labels"].reshape(-1)).all()
    assert call.run(c["C"], c["seed"], c["draw"]) == L.OK                                       # the same buffers, unspoilt arguments
    same(call.fetch(), c)


def test_a_source_out_of_range_counts_as_the_image_itself_and_sets_the_flag():
    c = pick(300, 20, 3)
    for bad in (-1, 3, 2 ** 31 - 1, -2 ** 31):
        src = c["src"].copy(); src[1] = bad
        got = run(c, src=src)
        want = CM.mix_numpy(c["images"], c["labels"], src, 20, c["seed"], c["draw"])
        assert all((g == w).all() for g, w in zip(got[:3], want)) and got[3] == 1
        assert (got[0][1] == c["images"][1]).all() and (got[1][1] == c["labels"][1]).all()
    call = Call(c["images"], c["labels"], [7, 0, 1])                                             # the flag does not outlive the call that set it
    L.check(call.run(20, 1, 2)); assert call.fetch()[3] == 1
    L.check(call.run(20, 1, 2, src=dev_at(c["src"]))); assert call.fetch()[3] == 0


def voronoi(rng, H, W, sites, Cn):
    """A salted Voronoi label map: the class of the nearest of `sites` random points, 1 % of the pixels replaced by a random id (Cn and 255,
    the ignore ids, among them)."""
    ys, xs = rng.integers(0, H, sites), rng.integers(0, W, sites)
    cls = rng.integers(0, Cn, sites).astype(np.uint8)
    yy, xx = np.mgrid[0:H, 0:W].astype(np.int32)
    ys, xs = ys.astype(np.int32), xs.astype(np.int32)
    d = (yy[None] - ys[:, None, None]) ** 2 + (xx[None] - xs[:, None, None]) ** 2
    lab = cls[np.argmin(d, 0)]
    salt = rng.random((H, W)) < 0.01
    lab[salt] = rng.choice(np.array(list(range(Cn)) + [Cn, 255], np.uint8), int(salt.sum()))
    return lab


def test_a_batch_of_two_512_by_1024_images():
    rng = np.random.default_rng(3)
    H, W, Cn = 512, 1024, 20
    labels = np.stack([voronoi(rng, H, W, 24, Cn), voronoi(rng, H, W, 24, 12)]).reshape(2, H * W)
    images = rng.integers(0, 256, (2, H * W, 3), dtype=np.uint8)
    want = CM.mix_numpy(images, labels, [1, 0], Cn, 17, 4)
    call = Call(images, labels, [1, 0], oimg_off=4)
    L.check(call.run(Cn, 17, 4))
    got = call.fetch()
    assert all((g == w).all() for g, w in zip(got[:3], want)) and got[3] == 0
    assert 0 < (got[1] != labels).sum() < labels.size                                           # something was pasted, and not everything


def test_the_engine_wrapper_returns_new_tensors_the_table_and_the_flag():
    from fcn8s_tensorflow_amd.engine import Engine
    c = pick(300, 20, 3)
    e = Engine(20, widths=(8, 16, 32, 64, 64, 128, 128), device_id=0)
    try:
        img = torch.from_numpy(c["images"].reshape(3, 15, 20, 3)).cuda(); lab = torch.from_numpy(c["labels"].reshape(3, 15, 20)).cuda()
        oi, ol, sel, flag = e.class_mix(img, lab, seed=c["seed"], draw=c["draw"], selected=True, status=True)        # src None: (n + 1) mod N
        assert flag == 0 and (sel.cpu().numpy() == c["selected"]).all()
        assert (oi.cpu().numpy().reshape(3, 300, 3) == c["out_images"]).all() and (ol.cpu().numpy().reshape(3, 300) == c["out_labels"]).all()
        assert (img.cpu().numpy().reshape(3, 300, 3) == c["images"]).all()                        # the inputs are not written
        work = e._class_mix_work
        oi2, ol2, flag = e.class_mix(img, lab, src=[0, 9, 2], seed=c["seed"], draw=c["draw"], status=True)
        assert flag == 1 and e._class_mix_work is work                                            # the scratch is kept
        want = CM.mix_numpy(c["images"], c["labels"], [0, 9, 2], 20, c["seed"], c["draw"])
        assert (oi2.cpu().numpy().reshape(3, 300, 3) == want[0]).all() and (ol2.cpu().numpy().reshape(3, 300) == want[1]).all()
        for kw in (dict(draw=1 << 48), dict(num_classes=256), dict(src=[0, 1])):
            with pytest.raises(ValueError):
                e.class_mix(img, lab, **kw)
        with pytest.raises(ValueError):
            e.class_mix(img.float(), lab)
    finally:
        e.close()
