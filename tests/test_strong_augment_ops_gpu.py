"""`fcn8s_op_strong_augment` (csrc/strong_augment.hip) against tests/golden/strong_augment_cases.npz and `strong_augment.augment_numpy` with `==`
in the augmented images and in `params_out`: integers and the float32 steps of HSV -> RGB decide everything.

Shapes are the smallest at which each path of the kernels can go wrong: the fixture's heights and widths around a 16-byte line and around the
augment kernel's tile of 32 x 64 pixels (H = R + 1 and W = R + 1 among them, where every neighbour is a reflection), a batch of 3 x 48 x 80 whose
images draw different gates (the block-uniform branches), every byte offset of the input and the output within a line (the grey kernel's three
pixel phases, the ragged lines of staging and store), guard bytes around every output, and one 2 x 512 x 1024 batch (several blocks per image in
both kernels, many chunks per thread of the grey sum)."""
import ctypes as C

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from fcn8s_tensorflow_amd import _lib as L, strong_augment as SA  # noqa: E402
from tests.test_strong_augment_host import golden, case_ids, pick, ONE  # noqa: E402
from tests.test_class_mix_ops_gpu import GUARD, guarded, guards_hold  # noqa: E402
from tests.test_pseudo_label_ops_gpu import dev_at, ptr  # noqa: E402


class Call:
    """The device buffers of one call: the input at its offset; output, work and params_out between guard bytes."""

    def __init__(self, images, img_off=0, out_off=0, work_off=0, work_fill=0xFF, params=True):
        self.N, self.H, self.W = images.shape[:3]
        self.T = int(images.size)
        self.images = dev_at(images, img_off)
        self.offs = (out_off, work_off)
        self.o_buf, self.o = guarded(self.T, out_off)
        self.wbytes = SA.work_bytes(self.N)
        self.w_buf, self.w = guarded(self.wbytes, work_off, work_fill)
        self.p_buf, self.p = guarded(self.N * 32) if params else (None, None)

    def run(self, seed, draw, jitter, blur, stream=None, **over):
        a = dict(images=self.images, N=self.N, H=self.H, W=self.W, seed=seed, draw=draw, work=self.w, out=self.o, par=self.p)
        a.update(over)
        jit_h = (C.c_int32 * 5)(*[int(v) for v in jitter]) if jitter is not None else None
        blur_h = taps_h = None
        if blur is not None:                                     # (gate, taps [Q, R + 1]) or, for the refusals, (gate, Q, R, flat taps | None)
            if len(blur) == 2:
                blur = (blur[0], blur[1].shape[0], blur[1].shape[1] - 1, np.asarray(blur[1]).reshape(-1))
            blur_h = (C.c_int32 * 3)(*[int(v) for v in blur[:3]])
            taps_h = (C.c_uint16 * len(blur[3]))(*[int(v) for v in blur[3]]) if blur[3] is not None else None
        return L.lib.fcn8s_op_strong_augment(stream, ptr(a["images"]), a["N"], a["H"], a["W"], a["seed"], a["draw"], jit_h, blur_h, taps_h,
                                             ptr(a["work"]), ptr(a["out"]), ptr(a["par"]))

    def fetch(self):
        """(out_images [N,H,W,3], params [N,8] | None) after checking every guard."""
        torch.cuda.synchronize()
        assert guards_hold(self.o_buf, self.offs[0], self.T), "a byte outside out_images was written"
        assert guards_hold(self.w_buf, self.offs[1], self.wbytes), "a byte outside work was written"
        par = None
        if self.p is not None:
            assert guards_hold(self.p_buf, 0, self.N * 32), "a byte outside params_out was written"
            par = self.p.cpu().numpy().view(np.int32).reshape(self.N, 8)
        return self.o.cpu().numpy().reshape(self.N, self.H, self.W, 3), par


def run(c, jitter="case", blur="case", **kw):
    call = Call(c["images"], **kw)
    L.check(call.run(c["seed"], c["draw"], c["jitter"] if isinstance(jitter, str) else jitter, c["blur"] if isinstance(blur, str) else blur))
    return call.fetch()


def same(got, c, tag=""):
    out, par = got
    assert out.shape == c["out_images"].shape and (out == c["out_images"]).all(), (tag, "out_images", np.argwhere(out != c["out_images"])[:8])
    if par is not None:
        assert (par == c["params"]).all(), (tag, par.tolist(), c["params"].tolist())


@pytest.mark.parametrize("i", range(len(golden())), ids=case_ids())
def test_the_op_equals_the_fixture(i):
    c = golden()[i]
    same(run(c), c)


@pytest.mark.parametrize("off", range(16))
def test_every_byte_offset_of_the_input_and_of_the_output(off):
    for c in (pick("batch"), pick("shape R7"), [k for k in golden() if (k["H"], k["W"]) == (33, 63)][0], pick("contrast alone")):
        same(run(c, img_off=off), c, "img_off = %d" % off)
        same(run(c, out_off=off), c, "out_off = %d" % off)
        same(run(c, img_off=off, out_off=(7 * off + 1) % 16, work_off=off), c, "all, %d" % off)


@pytest.mark.parametrize("fill", [0xFF, 0x00])
def test_the_prior_content_of_work_does_not_matter(fill):
    for c in (pick("batch"), pick("contrast alone"), pick("full strengths")):
        same(run(c, work_fill=fill), c, "work prefilled with %#x" % fill)


def test_params_out_may_be_null():
    c = pick("batch")
    got = run(c, params=False)
    assert got[1] is None
    same(got, c)


def test_a_null_jitter_a_null_blur_and_both():
    c = pick("batch")
    for jitter, blur in ((None, "case"), ("case", None), (None, None)):
        j = c["jitter"] if jitter == "case" else None
        b = c["blur"] if blur == "case" else None
        want = SA.augment_numpy(c["images"], c["seed"], c["draw"], j, b)
        out, par = run(c, jitter=j, blur=b)
        assert (out == want[0]).all() and (par == want[1]).all()
        if j is None and b is None:
            assert (out == c["images"]).all() and not par.any()                                  # a copy


def test_two_runs_give_the_same_bits():
    for c in (pick("batch"), pick("full strengths")):
        one, two = run(c), run(c)
        assert all(x.tobytes() == y.tobytes() for x, y in zip(one, two))


def test_bad_arguments_return_their_code_and_leave_the_outputs_untouched():
    c = pick("batch")
    call = Call(c["images"])
    jit, (gate, taps) = c["jitter"], c["blur"]
    Q, R = taps.shape[0], taps.shape[1] - 1
    flat = taps.reshape(-1).astype(np.int64)
    up = taps.astype(np.int64); d = up[-1, 0] - up[-1, 1]; up[-1, 0] -= 2 * d; up[-1, 1] += d   # the same sum, but w[1] > w[0]
    assert up[-1, 0] >= 0 and up[-1, 1] > up[-1, 0] and up[-1, 0] + 2 * up[-1, 1:].sum() == 2048
    off = flat.copy(); off[-(R + 1)] += 2                                                        # the last row sums to 2050
    j = lambda k, v: [v if i == k else int(x) for i, x in enumerate(jit)]
    bad = [dict(images=None), dict(work=None), dict(out=None), dict(N=0), dict(N=-1), dict(H=0), dict(H=-3), dict(W=0), dict(W=-1),
           dict(draw=1 << 48), dict(draw=(1 << 64) - 1),
           dict(jitter=j(0, ONE + 1)), dict(jitter=j(0, -1)), dict(jitter=j(1, ONE + 1)), dict(jitter=j(1, -1)), dict(jitter=j(2, ONE + 1)),
           dict(jitter=j(2, -1)), dict(jitter=j(3, ONE + 1)), dict(jitter=j(3, -1)), dict(jitter=j(4, 91)), dict(jitter=j(4, -1)),
           dict(blur=(ONE + 1, Q, R, flat)), dict(blur=(-1, Q, R, flat)), dict(blur=(gate, 0, R, flat)), dict(blur=(gate, 17, R, np.tile(flat, 2))),
           dict(blur=(gate, Q, 0, flat)), dict(blur=(gate, 4, 8, np.tile(flat, 2))), dict(blur=(gate, Q, R, None)),
           dict(blur=(gate, Q, R, up.reshape(-1))), dict(blur=(gate, Q, R, off)),
           dict(out=call.images), dict(out=call.images[5:]), dict(out=call.images[call.T - 1:])]
    for kw in bad:
        over = dict(kw)
        assert call.run(1, over.pop("draw", 2), over.pop("jitter", jit), over.pop("blur", (gate, taps)), **over) == L.ERR_BAD_ARG, kw
    assert call.run(1, 2, jit, (gate, taps), N=257) == L.ERR_SHAPE
    assert call.run(1, 2, jit, (gate, taps), H=1 << 16, W=1 << 15) == L.ERR_SHAPE
    assert call.run(1, 2, jit, (gate, taps), H=R) == L.ERR_SHAPE
    assert call.run(1, 2, jit, (gate, taps), W=R) == L.ERR_SHAPE
    out, par = call.fetch()
    assert (out == GUARD).all() and (par.view(np.uint8) == GUARD).all() and (call.w.cpu().numpy() == 0xFF).all()
    assert (call.images.cpu().numpy() == c["images"].reshape(-1)).all()
    assert call.run(c["seed"], c["draw"], jit, (gate, taps)) == L.OK                              # the same buffers, unspoilt arguments
    same(call.fetch(), c)
    assert call.run(c["seed"], c["draw"], jit, None, H=R, W=c["H"] * c["W"] // R) == L.OK         # without a blur a narrow image is fine


def test_a_batch_of_two_512_by_1024_images():
    rng = np.random.default_rng(4)
    images = rng.integers(0, 256, (2, 512, 1024, 3), dtype=np.uint8)
    images[1, :, :512] //= 3                                                                     # two different mean greys
    jitter, blur = [ONE, 16384, 16384, 16384, 23], (ONE, SA.taps_table(0.15, 1.15, 16, 4)[8:])
    want = SA.augment_numpy(images, 17, 4, jitter, blur)
    call = Call(images, out_off=4)
    L.check(call.run(17, 4, jitter, blur))
    out, par = call.fetch()
    assert (par == want[1]).all() and par[0, 5] != par[1, 5] and par[:, 0].all() and par[:, 6].all()
    assert (out == want[0]).all(), np.argwhere(out != want[0])[:8]


def test_the_engine_wrapper_returns_a_new_tensor_the_params_and_keeps_its_scratch():
    from fcn8s_tensorflow_amd.engine import Engine
    c = pick("batch")
    e = Engine(20, widths=(8, 16, 32, 64, 64, 128, 128), device_id=0)
    try:
        img = torch.from_numpy(c["images"]).cuda()
        out, par = e.strong_augment(img, seed=c["seed"], draw=c["draw"], jitter=c["jitter"], blur=c["blur"], params=True)
        assert (out.cpu().numpy() == c["out_images"]).all() and (par.cpu().numpy() == c["params"]).all()
        assert (img.cpu().numpy() == c["images"]).all()                                           # the input is not written
        work = e._strong_augment_work
        out2 = e.strong_augment(img, seed=c["seed"], draw=c["draw"], jitter=c["jitter"])
        assert isinstance(out2, torch.Tensor) and e._strong_augment_work is work                  # the scratch is kept
        assert (out2.cpu().numpy() == SA.augment_numpy(c["images"], c["seed"], c["draw"], c["jitter"], None)[0]).all()
        for kw in (dict(draw=1 << 48), dict(jitter=[ONE + 1, 0, 0, 0, 0]), dict(blur=(ONE, c["taps"][:, :1]))):
            with pytest.raises(ValueError):
                e.strong_augment(img, **kw)
        with pytest.raises(ValueError):
            e.strong_augment(img.float())
    finally:
        e.close()
