"""`fcn8s_op_entropy_term` on the GPU (the definition is in include/fcn8s_hip.h, restated in fcn8s_tensorflow_amd/loss.py): the kernel and its
reduction off the model, at the smallest shapes at which the tiling can go wrong -- P = 1, 15, 255, 256, 257, 513 pixels as one image and 2 x 300
with first_image = 1, times (C, K) = (4, 2), (20, 19), (20, 20), (21, 21), (64, 64): the 16-byte and the 4-byte path, even and odd C / 4, rows
beyond the C = 20 specialisation.

Bars (the project's): 1e-5 relative for the term, 1e-5 of the largest sum of |column| for bias_out, 2e-6 of the largest entry for dlogits, against
the float64 golden fixture (plain Python doubles) and against the float64 restatement.  Each case prints the device's distance next to the float32
restatement's own distance E to float64; where 8 E exceeds a bar, 8 E is the bar.

Exact, without a tolerance: columns >= K and rows outside U keep their bits, a prefilled dlogits comes back as pattern + contribution to one
rounding of the add, two runs give the same bits, weight -w is the exact negation of weight w.

Rows of equal logits give gradient rows of exact zeros for every K: the kernel takes ls_c + h_p as b_c - sum s b (the header's definition), which is
0 - 0 there.  Taken as written, with the two logf(S) left to cancel in fp32, the same rows came out at 2.9e-11 .. 4.6e-11 on the device for
K = 19, 20, 21, 64 (P = 257, weight 1) and only K = 2 gave zeros."""
import ctypes as C

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from fcn8s_tensorflow_amd import loss as LM  # noqa: E402
from tests import test_streams_gpu as ST  # noqa: E402
from tests.test_entropy_term_host import golden  # noqa: E402

CK = ((4, 2), (20, 19), (20, 20), (21, 21), (64, 64))
SHAPES = ((1, 1, 0), (1, 15, 0), (1, 255, 0), (1, 256, 0), (1, 257, 0), (1, 513, 0), (2, 300, 1))      # (N, HW, first_image)
GUARD = 64
PAT = np.float32(-7.25)


def _lib():
    from fcn8s_tensorflow_amd import _lib
    return _lib


def make_case(N, HW, Cn, K, seed, unlabeled=0.4):
    rng = np.random.default_rng(seed)
    P = N * HW
    z = (3.0 * rng.standard_normal((P, Cn))).astype(np.float32)
    z[::7, rng.integers(0, K)] += 40.0                                        # confident rows
    z[3::11] = z[3::11, :1]                                                   # flat rows
    if K < Cn:
        z[:, K:] = -1e30
    lab = rng.integers(0, Cn, P).astype(np.uint8)
    lab[rng.random(P) < unlabeled] = 255
    return z, lab


def run_op(z, lab, N, K, pixels='all', first=0, weight=1.0, d0=None, want_d=True, want_bias=True, zoff=0, doff=0, laboff=0, work_fill=0xFF,
           work_cut=0, stream=None, raw=None):
    """One raw call on padded buffers.  z (P, C) float32, lab (P,) uint8; d0: the prefill of dlogits (None: zeros).  The float buffers start
    `zoff` / `doff` floats and the labels `laboff` bytes behind a 16-byte boundary; guard words lie around dlogits and behind work, term_out and
    bias_out and must come back untouched.  Returns dict(rc, term, d, bias) as numpy (d / bias None when not asked for)."""
    L = _lib()
    P, Cn = z.shape
    HW = P // N
    ps = LM.ENTROPY_PIXEL_SETS.index(pixels)
    n = P * Cn
    zb = torch.full((n + 8,), float("nan"), device="cuda"); zv = zb[zoff:zoff + n]; zv.copy_(torch.from_numpy(z.reshape(-1)))
    db = torch.full((n + 2 * GUARD + 8,), float(PAT), device="cuda"); dv = db[GUARD + doff:GUARD + doff + n]
    dv.copy_(torch.from_numpy(np.zeros(n, np.float32) if d0 is None else np.ascontiguousarray(d0, np.float32).reshape(-1)))
    lb = torch.full((P + 32,), 7, dtype=torch.uint8, device="cuda"); lv = lb[laboff:laboff + P]; lv.copy_(torch.from_numpy(lab))
    assert zb.data_ptr() % 16 == 0 and db.data_ptr() % 16 == 0 and lb.data_ptr() % 16 == 0
    nwork = int(L.lib.fcn8s_op_entropy_term_work_bytes()) - work_cut
    wb = torch.full((nwork + GUARD,), work_fill, dtype=torch.uint8, device="cuda")
    wb[nwork:] = 0x5A
    tb = torch.full((1 + GUARD,), float(PAT), device="cuda")
    bb = torch.full((Cn + GUARD,), float(PAT), device="cuda")
    p = lambda t: C.c_void_p(t.data_ptr())
    args = dict(N=N, HW=HW, C=Cn, K=K, ps=ps, first=first, weight=weight, z=p(zv), d=p(dv) if want_d else None, lab=p(lv), work=p(wb), nwork=nwork,
                term=p(tb), bias=p(bb) if want_bias else None)
    args.update(raw or {})
    s = C.c_void_p(stream.cuda_stream) if stream is not None else None
    rc = L.lib.fcn8s_op_entropy_term(s, args["z"], args["d"], args["lab"], args["N"], args["HW"], args["C"], args["K"], args["ps"], args["first"],
                                     args["weight"], args["work"], args["nwork"], args["term"], args["bias"])
    torch.cuda.synchronize()
    dall, tall, ball = db.cpu().numpy(), tb.cpu().numpy(), bb.cpu().numpy()
    assert (dall[:GUARD + doff] == PAT).all() and (dall[GUARD + doff + n:] == PAT).all(), "a guard word around dlogits was written"
    assert (tall[1:] == PAT).all() and (ball[Cn:] == PAT).all(), "a guard word behind term_out or bias_out was written"
    assert (wb[nwork:].cpu().numpy() == 0x5A).all(), "a guard byte behind work was written"
    assert (lb.cpu().numpy()[laboff + P:] == 7).all()
    if rc != L.OK or not want_bias:
        assert (ball == PAT).all(), "bias_out was written by a call that must leave it alone"
    if rc != L.OK:
        assert tall[0] == PAT, "a refused call wrote term_out"
        assert np.array_equal(dall[GUARD + doff:GUARD + doff + n], np.zeros(n, np.float32) if d0 is None else np.asarray(d0, np.float32).reshape(-1))
    return dict(rc=rc, term=tall[0], d=dall[GUARD + doff:GUARD + doff + n].reshape(P, Cn).copy(), bias=ball[:Cn].copy() if want_bias else None)


def distances(got, ref, r32, what):
    """The device's distances to the float64 reference `ref` (dict term, dlogits, bias) and the float32 restatement's own (E); asserts the bars."""
    dmax, col = np.abs(ref["dlogits"]).max(), np.abs(ref["dlogits"]).sum(0).max()
    if dmax == 0.0:                                                           # an empty U, or rows that all have a zero gradient
        assert got["term"] == np.float32(ref["term"]) and not got["d"].any() and not got["bias"].any(), what
        return
    rel = lambda a, b, s: float(np.abs(np.asarray(a, np.float64) - b).max() / s)
    dev = dict(term=rel(got["term"], ref["term"], abs(ref["term"])), d=rel(got["d"], ref["dlogits"], dmax), bias=rel(got["bias"], ref["bias"], col))
    E = dict(term=rel(r32["term"], ref["term"], abs(ref["term"])), d=rel(r32["dlogits"], ref["dlogits"], dmax), bias=rel(r32["bias"], ref["bias"], col))
    print("%s: device %s; float32 restatement E %s" % (what, {k: "%.2e" % v for k, v in dev.items()}, {k: "%.2e" % v for k, v in E.items()}))
    assert dev["term"] <= max(1e-5, 8 * E["term"]), (what, got["term"], ref["term"])
    assert dev["bias"] <= max(1e-5, 8 * E["bias"]), what
    assert dev["d"] <= max(2e-6, 8 * E["d"]), what


GOLDEN = golden()


@pytest.mark.parametrize("i", range(len(GOLDEN)), ids=["%dx%d_C%d_K%d_%s" % (c["N"], c["HW"], c["C"], c["K"], c["pixels"]) for c in GOLDEN])
def test_op_matches_the_golden_fixture(i):
    c = GOLDEN[i]
    kw = dict(weight=c["weight"], pixels=c["pixels"], ncols=c["K"], first_image=c["first_image"], pixels_per_image=c["HW"])
    got = run_op(c["logits"], c["labels"], c["N"], c["K"], c["pixels"], c["first_image"], c["weight"])
    assert got["rc"] == 0
    r32 = LM.entropy_restate(c["logits"], c["labels"], dtype=np.float32, **kw)
    distances(got, c, r32, "fixture %d x %d C=%d K=%d %s first=%d" % (c["N"], c["HW"], c["C"], c["K"], c["pixels"], c["first_image"]))
    r = LM.entropy_restate(c["logits"], c["labels"], **kw)
    distances(got, r, r32, "  (restatement)")
    assert not got["d"][:, c["K"]:].any() and not got["d"][~r["used"]].any()                # columns >= K and rows outside U: exactly 0
    assert not c["dlogits"][~r["used"]].any() and np.array_equal(c["h"] != 0, r["used"])    # ... and the fixture has the same U


@pytest.mark.parametrize("Cn,K", CK)
@pytest.mark.parametrize("N,HW,first", SHAPES)
def test_op_matches_the_restatement(N, HW, first, Cn, K):
    """The full cross product of the shapes and (C, K), every pixel set."""
    z, lab = make_case(N, HW, Cn, K, 100 * HW + Cn + K)
    for j, pixels in enumerate(LM.ENTROPY_PIXEL_SETS):
        w = (1.0, -0.5, 0.25)[j]
        kw = dict(weight=w, pixels=pixels, ncols=K, first_image=first, pixels_per_image=HW)
        got = run_op(z, lab, N, K, pixels, first, w)
        assert got["rc"] == 0
        distances(got, LM.entropy_restate(z, lab, **kw), LM.entropy_restate(z, lab, dtype=np.float32, **kw),
                  "%d x %d C=%d K=%d %s first=%d" % (N, HW, Cn, K, pixels, first))


def ulp_of(x):
    x = np.abs(np.asarray(x, np.float32))
    return np.spacing(np.maximum(x, np.finfo(np.float32).tiny)).astype(np.float64)


@pytest.mark.parametrize("Cn,K", [(20, 19), (21, 21), (4, 2)])
@pytest.mark.parametrize("pixels", LM.ENTROPY_PIXEL_SETS)
@pytest.mark.parametrize("first", [0, 1, 2])
def test_exactness_that_needs_no_tolerance(Cn, K, pixels, first):
    N, HW = 2, 300
    z, lab = make_case(N, HW, Cn, K, 7 + Cn)
    P = N * HW
    rng = np.random.default_rng(5)
    pattern = (rng.standard_normal((P, Cn)) * 1e-3).astype(np.float32)
    pattern[::5] = 0.0
    pattern[1::5, 0] = -0.0                                                   # a negative zero must come back as one
    used = LM.entropy_restate(z, lab, 1.0, pixels, K, first, HW)["used"]
    assert used.any() == (first < N)
    zero = run_op(z, lab, N, K, pixels, first, 0.75)
    pre = run_op(z, lab, N, K, pixels, first, 0.75, d0=pattern)
    again = run_op(z, lab, N, K, pixels, first, 0.75, d0=pattern)
    neg = run_op(z, lab, N, K, pixels, first, -0.75)
    assert zero["rc"] == pre["rc"] == again["rc"] == neg["rc"] == 0
    bits = lambda a: np.ascontiguousarray(a, np.float32).view(np.uint32)
    # columns >= K and rows outside U: bit for bit what they were
    assert np.array_equal(bits(pre["d"][:, K:]), bits(pattern[:, K:]))
    assert np.array_equal(bits(pre["d"][~used]), bits(pattern[~used]))
    assert not zero["d"][:, K:].any() and not zero["d"][~used].any()
    assert zero["d"][used][:, :K].any() or first >= N
    # pattern + contribution, to one rounding of the add
    diff = pre["d"].astype(np.float64) - pattern
    assert (np.abs(diff - zero["d"]) <= np.maximum(ulp_of(pattern), ulp_of(zero["d"]))).all()
    # two runs, identical bits
    for k in ("d", "bias"):
        assert np.array_equal(bits(pre[k]), bits(again[k])), k
    assert bits(pre["term"]) == bits(again["term"]) == bits(zero["term"]) == bits(neg["term"])
    # weight -w: the exact negation
    assert np.array_equal(neg["d"], -zero["d"]) and np.array_equal(neg["bias"], -zero["bias"])


@pytest.mark.parametrize("Cn,K", CK)
def test_equal_logit_rows_give_exact_zero_gradient_rows(Cn, K):
    """Every K, not only the powers of two: b = 0, sum s b = 0, and coef (-(s (0 - 0))) is a zero."""
    z, lab = make_case(1, 257, Cn, K, 3)
    flat = np.zeros(257, bool)
    flat[3::11] = True
    assert (z[flat][:, :K] == z[flat][:, :1]).all()
    got = run_op(z, lab, 1, K, 'all', 0, 1.0)
    r32 = LM.entropy_restate(z, lab, 1.0, 'all', K, dtype=np.float32)
    print("C=%d K=%d: largest gradient entry of an equal-logit row: device %.3e, float32 restatement %.3e"
          % (Cn, K, np.abs(got["d"][flat]).max(), np.abs(r32["dlogits"][flat]).max()))
    assert got["rc"] == 0 and got["d"][~flat].any()
    assert not got["d"][flat].any()


@pytest.mark.parametrize("Cn,K", [(20, 20), (20, 19), (21, 21), (64, 64)])
def test_every_alignment_of_the_pointers(Cn, K):
    z, lab = make_case(1, 257, Cn, K, 11)
    kw = dict(weight=1.0, pixels='unlabeled', ncols=K)
    r, r32 = LM.entropy_restate(z, lab, **kw), LM.entropy_restate(z, lab, dtype=np.float32, **kw)
    rng = np.random.default_rng(2)
    pattern = (rng.standard_normal(z.shape) * 1e-3).astype(np.float32)
    for zoff in range(4):
        for doff in range(4):
            got = run_op(z, lab, 1, K, 'unlabeled', 0, 1.0, d0=pattern, zoff=zoff, doff=doff, laboff=(5 * zoff + 3 * doff) % 16)
            assert got["rc"] == 0
            got["d"] = got["d"] - pattern                                     # (the contribution, to one rounding of the add)
            distances(got, r, r32, "C=%d K=%d logits + %d floats, dlogits + %d floats" % (Cn, K, zoff, doff))
    base = run_op(z, lab, 1, K, 'unlabeled', 0, 1.0)
    for laboff in range(16):
        got = run_op(z, lab, 1, K, 'unlabeled', 0, 1.0, laboff=laboff)
        assert got["rc"] == 0 and np.array_equal(got["d"], base["d"]) and got["term"] == base["term"] and np.array_equal(got["bias"], base["bias"]), laboff


@pytest.mark.parametrize("Cn,K", [(20, 20), (21, 21)])
def test_work_prefill_and_null_outputs(Cn, K):
    z, lab = make_case(2, 300, Cn, K, 13)
    a = run_op(z, lab, 2, K, 'valid', 1, 0.5, work_fill=0xFF)
    b = run_op(z, lab, 2, K, 'valid', 1, 0.5, work_fill=0)
    assert a["rc"] == b["rc"] == 0 and a["term"] == b["term"] and np.array_equal(a["d"], b["d"]) and np.array_equal(a["bias"], b["bias"])
    n = run_op(z, lab, 2, K, 'valid', 1, 0.5, want_d=False)                   # the term and the column sums only: dlogits keeps its zeros
    assert n["rc"] == 0 and n["term"] == a["term"] and not n["d"].any() and np.array_equal(n["bias"], a["bias"])
    n = run_op(z, lab, 2, K, 'valid', 1, 0.5, want_bias=False)
    assert n["rc"] == 0 and n["term"] == a["term"] and np.array_equal(n["d"], a["d"])
    n = run_op(z, lab, 2, K, 'valid', 1, 0.5, want_d=False, want_bias=False)
    assert n["rc"] == 0 and n["term"] == a["term"] and not n["d"].any()
    e = run_op(z, lab, 2, K, 'valid', 2, 0.5)                                 # first_image = N: U is empty
    assert e["rc"] == 0 and e["term"] == 0.0 and not e["d"].any() and not e["bias"].any()


def test_refusals_leave_every_output_untouched():
    L = _lib()
    z, lab = make_case(2, 40, 20, 20, 17)
    pattern = np.full(z.shape, 3.5, np.float32)
    ok = run_op(z, lab, 2, 20, d0=pattern)
    assert ok["rc"] == 0
    bad = (dict(z=None), dict(lab=None), dict(work=None), dict(term=None), dict(weight=float("nan")), dict(weight=float("inf")), dict(ps=-1), dict(ps=3),
           dict(K=1), dict(K=21), dict(C=1), dict(C=65, K=65), dict(first=-1), dict(nwork=0))
    for raw in bad:
        assert run_op(z, lab, 2, 20, d0=pattern, raw=raw)["rc"] == L.ERR_BAD_ARG, raw
    for raw in (dict(N=0), dict(HW=0), dict(N=-1), dict(HW=-5)):
        assert run_op(z, lab, 2, 20, d0=pattern, raw=raw)["rc"] == L.ERR_SHAPE, raw
    assert run_op(z, lab, 2, 20, d0=pattern, work_cut=1)["rc"] == L.ERR_BAD_ARG          # a work one byte too small
    # misaligned float pointers
    zt = torch.zeros(z.size + 4, device="cuda")
    for k in ("z", "d", "term", "bias"):
        assert run_op(z, lab, 2, 20, d0=pattern, raw={k: C.c_void_p(zt.data_ptr() + 2)})["rc"] == L.ERR_BAD_ARG, k
    with pytest.raises(ValueError):
        L.check(L.lib.fcn8s_op_entropy_term(None, None, None, None, 2, 40, 20, 20, 2, 0, 1.0, None, 0, None, None))


def test_engine_wrapper():
    from tests.test_lovasz_gpu import SMALL, engine
    e = engine(SMALL)
    z, lab = make_case(2, 300, 20, 20, 19)
    zt = torch.from_numpy(z.reshape(2, 20, 15, 20)).cuda(); lt = torch.from_numpy(lab.reshape(2, 20, 15)).cuda()
    d = torch.zeros_like(zt)
    term, bias = e.entropy_term_op(zt, lt, 0.5, 'unlabeled', first_image=1, dlogits=d, bias=True)
    r = LM.entropy_restate(z, lab, 0.5, 'unlabeled', None, 1, 300)
    r32 = LM.entropy_restate(z, lab, 0.5, 'unlabeled', None, 1, 300, dtype=np.float32)
    distances(dict(term=term.cpu().numpy()[0], d=d.cpu().numpy().reshape(-1, 20), bias=bias.cpu().numpy()), r, r32, "Engine.entropy_term_op")
    t2, b2 = e.entropy_term_op(zt, lt, 0.5, 'unlabeled', first_image=1)
    assert b2 is None and t2.cpu().numpy()[0] == term.cpu().numpy()[0]
    for bad in (dict(logits=zt.cpu()), dict(labels=lt.long()), dict(labels=lt[:1]), dict(dlogits=d[..., :19]), dict(pixels='x'), dict(ncols=1)):
        kw = dict(logits=zt, labels=lt)
        kw.update(bad)
        with pytest.raises(ValueError):
            e.entropy_term_op(**kw)
    e.close()


def test_every_block_trips_more_than_once():
    """2 x 512 x 1024 x 20: 4096 tiles over at most 1024 blocks."""
    N, HW, Cn = 2, 512 * 1024, 20
    gen = torch.Generator(device="cuda").manual_seed(3)
    zt = (torch.randn((N * HW, Cn), device="cuda", generator=gen) * 3).contiguous()
    lt = torch.randint(0, Cn, (N * HW,), dtype=torch.uint8, device="cuda", generator=gen)
    lt[torch.rand(N * HW, device="cuda", generator=gen) < 0.5] = 255
    d = torch.zeros_like(zt)
    L = _lib()
    work = torch.empty(int(L.lib.fcn8s_op_entropy_term_work_bytes()), dtype=torch.uint8, device="cuda")
    term = torch.zeros(1, device="cuda"); bias = torch.zeros(Cn, device="cuda")
    p = lambda t: C.c_void_p(t.data_ptr())
    L.check(L.lib.fcn8s_op_entropy_term(None, p(zt), p(d), p(lt), N, HW, Cn, Cn, 0, 1, 1.0, p(work), work.numel(), p(term), p(bias)))
    torch.cuda.synchronize()
    z, lab = zt.cpu().numpy(), lt.cpu().numpy()
    kw = dict(weight=1.0, pixels='unlabeled', first_image=1, pixels_per_image=HW)
    r, r32 = LM.entropy_restate(z, lab, **kw), LM.entropy_restate(z, lab, dtype=np.float32, **kw)
    got = dict(term=term.cpu().numpy()[0], d=d.cpu().numpy(), bias=bias.cpu().numpy())
    assert not got["d"][:HW].any() and not got["d"][HW:][lab[HW:] < Cn].any()
    distances(got, r, r32, "2 x 512 x 1024 x 20 unlabeled first=1")


# ---- a side stream: the op's row in the stream case table (tests/test_streams_host.py asks for one per entry point that takes a stream) -----------
@ST.row("entropy_term", ("fcn8s_op_entropy_term",))
class _EntropyTermRow:
    @staticmethod
    def make(seed):
        N, HW, Cn, K = (2, 300, 20, 20) if seed == 1 else (1, 513, 20, 19)
        z, lab = make_case(N, HW, Cn, K, 40 + seed)
        rng = np.random.default_rng(seed)
        d = (rng.standard_normal(z.shape) * 1e-3).astype(np.float32)
        nwork = int(_lib().lib.fcn8s_op_entropy_term_work_bytes())
        inp = dict(z=z, lab=lab, d=d)
        poison = dict(lab=np.where(lab == 255, np.uint8(0), np.uint8(255)).astype(np.uint8))    # the complementary pixel set
        out = dict(term=((1,), np.float32), bias=((Cn,), np.float32), work=((nwork,), np.uint8))
        return ST.Case(inp, out, fetch=("d", "term", "bias"), poison=poison, N=N, HW=HW, C=Cn, K=K)

    @staticmethod
    def call(L, s, b, case):
        a = case.aux
        p = ST.ptr
        L.check(L.lib.fcn8s_op_entropy_term(s, p(b["z"]), p(b["d"]), p(b["lab"]), a["N"], a["HW"], a["C"], a["K"], 0, 0, 0.5, p(b["work"]),
                                            b["work"].numel(), p(b["term"]), p(b["bias"])))

    @staticmethod
    def check(case, got):
        a, i = case.aux, case.inp
        kw = dict(weight=0.5, pixels='unlabeled', ncols=a["K"], pixels_per_image=a["HW"])
        r, r32 = LM.entropy_restate(i["z"], i["lab"], **kw), LM.entropy_restate(i["z"], i["lab"], dtype=np.float32, **kw)
        distances(dict(term=got["term"][0], d=got["d"] - i["d"], bias=got["bias"]), r, r32, "stream row %d x %d" % (a["N"], a["HW"]))


ROW = ST.ROWS[-1]
MAX_QUEUES = 4                                                   # HIP's default number of hardware queues (tests/test_strong_augment_streams_gpu.py)
CANARY_CASES = (("zero", "null_late"), ("producer", "side_late"), ("producer", "null_late"))      # run_canary's


@pytest.fixture(scope="module")
def harness():
    """As tests/test_strong_augment_streams_gpu.py: the first of up to MAX_QUEUES fresh harnesses whose side stream the canary can tell from the
    NULL stream (this file runs after several others have taken streams, and the runtime deals its hardware queues in turn)."""
    made = []                                                   # kept alive: a released stream would be handed out again
    for _ in range(MAX_QUEUES):
        h = ST.Harness()
        h.longest_ms, h.longest_host_ms = 0.0, 0.0
        h.set_delay("op", 0.0)
        made.append(h)
        if not any(ST.same_bits(*ST.canary(h, stray, skew)) for stray, skew in CANARY_CASES):
            h.others = made
            return h
    pytest.fail("none of %d fresh side streams can be told from the NULL stream by the canary: no case of this module can see a misdirected launch" % MAX_QUEUES)


def test_the_row_is_in_the_table():
    assert ROW.name == "entropy_term" and ROW.entries == ("fcn8s_op_entropy_term",) and ROW in ST.ROWS


@pytest.mark.parametrize("skew", ST.SKEWS)
def test_entropy_term_on_a_side_stream(skew, harness):
    ST.run_canary(harness)                                      # the harness sees a stray launch here and now
    case = ROW.make(1)
    ST.execute(ROW, ROW.make(2), None, None, None)              # default stream, other data: warm, and the row's host time
    want = ST.execute(ROW, case, None, None, None)
    ROW.check(case, want)
    ST.execute(ROW, ROW.make(2), harness, harness.S, "side_late" if skew == "null_late" else "null_late")
    got = ST.execute(ROW, case, harness, harness.S, skew)
    ROW.check(case, got)
    for name in ("d", "term", "bias"):
        assert ST.same_bits(got[name], want[name]), name        # the default stream's result, bit for bit
