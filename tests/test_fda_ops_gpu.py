"""`fcn8s_op_fda_transfer` (csrc/fda.hip) against tests/golden/fda_cases.npz -- float64 results of the published fft2 route -- and against
`fda.transfer_numpy(float64)`, which tests/test_fda_host.py ties to that fixture.

Tolerance.  Per case E = max |transfer_numpy(float32) - reference|, the float32 restatement's own rounding; the bar is 8 max(E, spacing(256f)): the
factor 8 is what every float test of this library allows over the restatement's rounding, the floor is one rounding of the final add.  out_f32 lies
within the bar of the reference and EVERY byte of out_u8 within 0.5 + bar of clamp(reference, 0, 255); no share of pixels is excluded.  Each test
prints the device's distance and E.

Everything else holds with ==: the equal-bytes identity, two runs, the prior content of work, an image alone against the same image at each place
in a batch, pair NULL against n mod M, either output NULL, every byte offset of images, targets and out_u8, every refusal, the flag.

Every buffer the op sees is carved from tests/hostile.py's arena: 0xFF all over (a NaN as float32), a band of 1 MiB on either side that must come
back whole, inputs that must come back unchanged, and a float output of which every element must have been written.

Shapes: the fixture's (2 x 2 to 33 x 129; one batch 3 + 2 with a rotated pair and a repeated target); 130 x 257 at b = 12 -- five row tiles of 32,
the last of 2 rows, five chunks of 64 pixels in the analysis and three tiles of 128 pixels in the synthesis, the last of one pixel --; 200 x 193 at
b = 96, the largest half-width (seven column tiles of 32, window = width; (c, v) in five blocks of 64); and one 1 x 512 x 1024 call at b = 46."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from fcn8s_tensorflow_amd import _lib as L, fda as FDA  # noqa: E402
from tests import hostile  # noqa: E402
from tests.test_fda_host import golden, case_ids, pick, restated32  # noqa: E402

FLOOR = float(np.spacing(np.float32(256)))


def bar_of(E):
    return 8.0 * max(E, FLOOR)


@pytest.fixture(autouse=True)
def _hostile():
    with hostile.session(L) as arena:
        yield arena


def ptr(t):
    return C.c_void_p(t.data_ptr()) if t is not None else None


def inp_at(a, off):
    """The bytes of `a` on the device, `off` bytes behind a 256-byte boundary."""
    flat = np.ascontiguousarray(a).reshape(-1).view(np.uint8)
    return hostile.inp(np.concatenate([np.full(off, 0xFF, np.uint8), flat]))[off:]


class Call:
    """The device buffers of one call, all from the arena: inputs at their byte offsets, out_u8 at its offset inside 16 spare bytes, out_f32, work."""

    def __init__(self, images, targets, b, pair=None, img_off=0, trg_off=0, out_off=0, work_off=0, work_fill=0xFF, u8=True, f32=True):
        self.N, self.H, self.W = images.shape[:3]
        self.M, self.b = targets.shape[0], b
        self.T = int(images.size)
        self.images, self.targets = inp_at(images, img_off), inp_at(targets, trg_off)
        self.pair = hostile.inp(np.asarray(pair, np.int32)) if pair is not None else None
        self.out_off = out_off
        self.u8_buf = hostile.out((self.T + 16,), torch.uint8) if u8 else None
        self.u8 = self.u8_buf[out_off:out_off + self.T] if u8 else None
        self.f32 = hostile.out(images.shape, torch.float32) if f32 else None
        self.wbytes = FDA.work_bytes(self.N, self.M, self.H, self.W, b)
        self.w_buf = hostile.inout(np.full(self.wbytes + 16, work_fill, np.uint8))
        self.w = self.w_buf[work_off:work_off + self.wbytes]

    def run(self, stream=None, **over):
        a = dict(images=self.images, N=self.N, targets=self.targets, M=self.M, H=self.H, W=self.W, b=self.b, pair=self.pair, work=self.w, u8=self.u8,
                 f32=self.f32)
        a.update(over)
        return L.lib.fcn8s_op_fda_transfer(stream, ptr(a["images"]), a["N"], ptr(a["targets"]), a["M"], a["H"], a["W"], a["b"], ptr(a["pair"]),
                                           ptr(a["work"]), ptr(a["u8"]), ptr(a["f32"]))

    def fetch(self):
        """(out_u8 | None, out_f32 | None, flag) after checking the spare bytes around out_u8; the bands are the arena's to check."""
        torch.cuda.synchronize()
        u8 = f32 = None
        if self.u8 is not None:
            raw = self.u8_buf.cpu().numpy()
            assert (raw[:self.out_off] == 0xFF).all() and (raw[self.out_off + self.T:] == 0xFF).all(), "a byte outside out_u8 was written"
            u8 = raw[self.out_off:self.out_off + self.T].reshape(self.N, self.H, self.W, 3).copy()
        if self.f32 is not None:
            f32 = self.f32.cpu().numpy()
        return u8, f32, FDA.flag_of(self.w)


def run(images, targets, b, pair=None, **kw):
    call = Call(images, targets, b, pair, **kw)
    L.check(call.run())
    return call.fetch()


def run_case(c, **kw):
    return run(c["images"], c["targets"], c["b"], c["pair"], **kw)


def bits(got):
    return tuple(None if x is None else x.tobytes() for x in got[:2])


def within(got, ref64, E, tag):
    """out_f32 within the bar of the reference, every byte of out_u8 within 0.5 + bar of its clamp; prints the figures."""
    u8, f32, _ = got
    bar = bar_of(E)
    d32 = float(np.abs(f32.astype(np.float64) - ref64).max())
    d8 = float(np.abs(u8.astype(np.float64) - np.clip(ref64, 0, 255)).max())
    print("fda %s: device %.3e, E %.3e, device / max(E, floor) %.2f, bar %.3e, bytes %.4f" % (tag, d32, E, d32 / max(E, FLOOR), bar, d8))
    assert np.isfinite(f32).all() and d32 <= bar, (tag, d32, bar)
    assert d8 <= 0.5 + bar, (tag, d8, 0.5 + bar)
    assert (u8 == np.clip(np.rint(f32), 0, 255).astype(np.uint8)).all(), (tag, "out_u8 is not the rounded out_f32")


@functools.lru_cache(maxsize=None)
def synthetic(N, M, H, W, b, seed):
    """(images, targets, reference float64, E) of a shape the fixture does not hold: noise sources, smooth-plus-noise targets."""
    rng = np.random.default_rng(seed)
    images = rng.integers(0, 256, (N, H, W, 3), dtype=np.uint8)
    y, x = np.mgrid[0:H, 0:W]
    wave = lambda m: (np.sin(2.1 * y / H + m) * np.cos(1.3 * x / W))[..., None] * np.array([1.0, 0.8, 0.6])
    targets = np.stack([np.clip(np.rint(120 + 70 * wave(m) + rng.normal(0, 10, (H, W, 3))), 0, 255).astype(np.uint8) for m in range(M)])
    ref = FDA.transfer_numpy(images, targets, b)
    E = float(np.abs(FDA.transfer_numpy(images, targets, b, dtype=np.float32).astype(np.float64) - ref).max())
    return images, targets, ref, E


@pytest.mark.parametrize("i", range(len(golden())), ids=case_ids())
def test_the_op_lies_within_the_bar_of_the_fixture(i):
    c = golden()[i]
    within(run_case(c), c["y"], restated32(i)[1], c["name"])


@pytest.mark.parametrize("shape", [(2, 2, 130, 257, 12), (1, 1, 200, 193, 96), (1, 2, 257, 130, 5)], ids=lambda s: "%d+%d_%dx%d_b%d" % s)
def test_more_than_one_tile_each_way_and_the_largest_half_width(shape):
    images, targets, ref, E = synthetic(*shape, seed=7)
    within(run(images, targets, shape[4]), ref, E, "%d+%d %dx%d b=%d" % shape)


def test_one_full_size_call():
    images, targets, ref, E = synthetic(1, 1, 512, 1024, 46, seed=11)
    within(run(images, targets, 46), ref, E, "1+1 512x1024 b=46")


def test_a_source_whose_target_holds_the_same_bytes_comes_back_exactly():
    for c in (pick("batch"), pick("33x129 b=16")):
        u8, f32, _ = run(c["images"], c["images"].copy(), c["b"])                 # (another buffer: inp_at copies)
        assert (u8 == c["images"]).all() and (f32 == c["images"].astype(np.float32)).all(), c["name"]
    images, _, _, _ = synthetic(2, 2, 130, 257, 12, seed=7)
    u8, f32, _ = run(images, images[::-1].copy(), 12, pair=[1, 0])
    assert (u8 == images).all() and (f32 == images.astype(np.float32)).all()
    c = pick("batch")                                                             # one source of three has its own bytes as target
    trg = np.stack([c["targets"][0], c["images"][1]])
    u8, f32, _ = run(c["images"], trg, c["b"], pair=[0, 1, 0])
    assert (u8[1] == c["images"][1]).all() and (f32[1] == c["images"][1].astype(np.float32)).all() and (u8[0] != c["images"][0]).any()


def test_two_runs_and_either_content_of_work_give_the_same_bits():
    for c in (pick("batch"), pick("33x129 b=16")):
        one = bits(run_case(c))
        assert bits(run_case(c)) == one
        assert bits(run_case(c, work_fill=0x00)) == one and bits(run_case(c, work_fill=0xFF, work_off=9)) == one


def test_an_image_alone_equals_the_same_pair_at_each_place_in_a_batch():
    c = pick("batch")
    N, M = c["N"], c["M"]
    alone = [bits(run(c["images"][n:n + 1], c["targets"][c["pair"][n]:c["pair"][n] + 1], c["b"])) for n in range(N)]
    for k in range(N):                                                            # the batch rolled by k: image n sits at place (n + k) mod N
        order = [(j - k) % N for j in range(N)]
        u8, f32, _ = run(c["images"][order], c["targets"], c["b"], pair=[int(c["pair"][n]) for n in order])
        for j, n in enumerate(order):
            assert (u8[j].tobytes(), f32[j].tobytes()) == alone[n], (k, j, n)
    u8, f32, _ = run(c["images"], c["targets"][::-1].copy(), c["b"], pair=[1 - int(p) for p in c["pair"]])     # the targets' places swapped
    assert all((u8[n].tobytes(), f32[n].tobytes()) == alone[n] for n in range(N))
    big = np.concatenate([c["targets"], c["targets"][:1], c["images"][:2]])       # M = 5, two of them referenced
    u8, f32, _ = run(c["images"], big, c["b"], pair=[1, 2, 1])
    assert all((u8[n].tobytes(), f32[n].tobytes()) == alone[n] for n in range(N))


def test_a_null_pair_is_n_mod_m_and_either_output_may_be_null():
    c = pick("batch")
    both = bits(run(c["images"], c["targets"], c["b"], pair=[0, 1, 0]))
    assert bits(run(c["images"], c["targets"], c["b"], pair=None)) == both
    assert bits(run(c["images"], c["targets"], c["b"], u8=False)) == (None, both[1])
    assert bits(run(c["images"], c["targets"], c["b"], f32=False)) == (both[0], None)


@pytest.mark.parametrize("off", range(16))
def test_every_byte_offset_of_the_inputs_and_of_out_u8(off):
    for c in (pick("batch"), pick("8x63 b=3")):
        want = bits(run_case(c))
        assert bits(run_case(c, img_off=off)) == want, ("images", off)
        assert bits(run_case(c, trg_off=off)) == want, ("targets", off)
        assert bits(run_case(c, out_off=off)) == want, ("out_u8", off)
        assert bits(run_case(c, img_off=off, trg_off=(5 * off + 3) % 16, out_off=(7 * off + 1) % 16, work_off=off)) == want, ("all", off)


def test_a_pair_out_of_range_counts_as_n_mod_m_and_sets_the_flag():
    c = pick("batch")
    want = run(c["images"], c["targets"], c["b"], pair=[1, 1, 0])
    assert want[2] == 0
    for pair in ([1, 5, -1], [1, 2, 1 << 30], [1, -(1 << 31), 0]):
        got = run(c["images"], c["targets"], c["b"], pair=pair)
        assert bits(got) == bits(want) and got[2] == 1, pair


def test_bad_arguments_return_their_code_and_leave_the_outputs_untouched():
    c = pick("batch")
    call = Call(c["images"], c["targets"], c["b"], c["pair"])
    H, W = c["H"], c["W"]
    bad = [dict(images=None), dict(targets=None), dict(work=None), dict(u8=None, f32=None), dict(N=0), dict(N=-1), dict(M=0), dict(M=-2), dict(H=0),
           dict(H=-1), dict(W=0), dict(W=-1), dict(b=-1), dict(b=97), dict(b=8), dict(b=12, H=25, W=24), dict(b=96, H=192, W=400),
           dict(u8=call.images), dict(u8=call.images[7:]), dict(u8=call.targets[call.targets.numel() - 1:]), dict(u8=call.w[16:]),
           dict(f32=call.images), dict(f32=call.targets[4:]), dict(f32=call.pair), dict(f32=call.w[32:]), dict(u8=call.f32.view(torch.uint8).reshape(-1)[8:]),
           dict(f32=call.f32.view(torch.uint8).reshape(-1)[1:])]
    for kw in bad:
        assert call.run(**kw) == L.ERR_BAD_ARG, kw
    assert call.run(N=257) == L.ERR_SHAPE and call.run(M=257) == L.ERR_SHAPE
    assert call.run(H=1 << 16, W=1 << 15) == L.ERR_SHAPE and call.run(H=1 << 15, W=1 << 16, b=0) == L.ERR_SHAPE
    torch.cuda.synchronize()
    assert (call.u8_buf == 0xFF).all() and (call.f32.view(torch.int32) == -1).all() and (call.w_buf == 0xFF).all()
    assert call.run() == L.OK                                                     # the same buffers, unspoilt arguments
    within(call.fetch(), c["y"], restated32(len(golden()) - 1)[1], "after the refusals")
    assert np.isfinite(run(c["images"], c["targets"], 7)[1]).all()                # 2 b + 1 = 15 <= 16: the largest that fits


def test_the_engine_wrapper_returns_a_new_tensor_and_keeps_its_scratch():
    from fcn8s_tensorflow_amd.engine import Engine
    c = pick("batch")
    e = Engine(20, widths=(8, 16, 32, 64, 64, 128, 128), device_id=0)
    try:
        img, trg = torch.from_numpy(c["images"]).cuda(), torch.from_numpy(c["targets"]).cuda()
        want = run_case(c)
        out, flag = e.fda_transfer(img, trg, b=c["b"], pair=c["pair"].tolist(), status=True)
        assert out.dtype == torch.uint8 and out.data_ptr() != img.data_ptr() and flag == 0 and (out.cpu().numpy() == want[0]).all()
        assert (img.cpu().numpy() == c["images"]).all() and (trg.cpu().numpy() == c["targets"]).all()
        work = e._fda_work
        y = e.fda_transfer(img, trg, b=c["b"], pair=torch.tensor([1, 0, 1], dtype=torch.int32, device="cuda"), out_float=True)
        assert y.dtype == torch.float32 and (y.cpu().numpy() == want[1]).all() and e._fda_work is work       # the scratch is kept
        assert FDA.half_width(c["H"], c["W"], 0.13) == c["b"]
        assert (e.fda_transfer(img, trg, beta=0.13, pair=[1, 0, 1]).cpu().numpy() == want[0]).all()          # b = floor(16 * 0.13) = 2
        _, flag = e.fda_transfer(img, trg, b=c["b"], pair=torch.tensor([1, 7, 1], dtype=torch.int32, device="cuda"), status=True)
        assert flag == 1
        for kw in (dict(b=8), dict(b=-1), dict(b=1.5), dict(beta=-0.1), dict(beta="x"), dict(b=2, pair=[0, 1]), dict(b=2, pair=[0, 2, 0]),
                   dict(b=2, pair=torch.tensor([1, 0, 1], device="cuda"))):
            with pytest.raises(ValueError):
                e.fda_transfer(img, trg, **kw)
        for a, t in ((img.float(), trg), (img, trg[:, :8]), (img.cpu(), trg), (img[:, :, ::2], trg[:, :, ::2])):
            with pytest.raises(ValueError):
                e.fda_transfer(a, t, b=1)
    finally:
        e.close()
