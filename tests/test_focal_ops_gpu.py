"""`fcn8s_op_focal_xent` on the GPU (the definition is in include/fcn8s_hip.h, restated in fcn8s_tensorflow_amd/loss.py): the kernel and its
reduction off the model, at the smallest shapes at which the tiling can go wrong -- P = 1, 15, 255, 256, 257, 513 pixels and 2 x 300, times
C = 2, 4, 19, 20, 21, 64: the 16-byte and the 4-byte path, even and odd C / 4, rows beyond the C = 20 specialisation -- and gamma = 0.5, 1, 2, 5.

Bars (the project's): 1e-5 relative for the loss, 1e-5 of the largest sum of |column| for bias_out, 2e-6 of the largest entry for dlogits, against
the float64 golden fixture (plain Python doubles) and against the float64 restatement.  Each case prints the device's distance next to the float32
restatement's own distance E to float64; where 8 E exceeds a bar, 8 E is the bar.

Exact, with ==: a row with u = 0 is a row of zeros, ignored rows and padding columns are zeros, all weights x 2 doubles the loss and every entry, a
table of 1.0 equals no table, a class weight 0 equals relabelling that class to 255, two runs give the same bits."""
import ctypes as C

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from fcn8s_tensorflow_amd import loss as LM  # noqa: E402
from tests import test_streams_gpu as ST  # noqa: E402
from tests.test_focal_host import GAMMAS, case_id, golden, make_case, weights  # noqa: E402

CS = ((2, 2), (4, 4), (19, 19), (20, 19), (20, 20), (21, 21), (64, 64))      # (C, K)
PS = (1, 15, 255, 256, 257, 513, 600)
GUARD = 64
PAT = np.float32(-7.25)


def _lib():
    from fcn8s_tensorflow_amd import _lib
    return _lib


def make_px(P, seed):
    rng = np.random.default_rng(seed)
    return rng.integers(0, 256, P).astype(np.uint8), (rng.integers(0, 49, 256) / 16.0).astype(np.float32)


def run_op(z, lab, gamma, cw=None, codes=None, table=None, want_d=True, want_bias=True, zoff=0, doff=0, laboff=0, codeoff=0, cwoff=0, taboff=0,
           work_fill=0xFF, work_cut=0, stream=None, raw=None):
    """One raw call on padded buffers.  z (P, C) float32, lab (P,) uint8.  The float buffers start `zoff` / `doff` / `cwoff` / `taboff` floats and
    the labels and codes `laboff` / `codeoff` bytes behind a 16-byte boundary; dlogits is prefilled with a pattern (the op stores, so nothing of
    it may survive); guard words lie around dlogits and behind work, loss_dev and bias_out and must come back untouched.
    Returns dict(rc, loss, d, bias) as numpy."""
    L = _lib()
    P, Cn = z.shape
    n = P * Cn
    zb = torch.full((n + 8,), float("nan"), device="cuda"); zv = zb[zoff:zoff + n]; zv.copy_(torch.from_numpy(z.reshape(-1)))
    db = torch.full((n + 2 * GUARD + 8,), float(PAT), device="cuda"); dv = db[GUARD + doff:GUARD + doff + n]
    lb = torch.full((P + 32,), 7, dtype=torch.uint8, device="cuda"); lv = lb[laboff:laboff + P]; lv.copy_(torch.from_numpy(lab))
    cb = torch.full((P + 32,), 9, dtype=torch.uint8, device="cuda"); cv = cb[codeoff:codeoff + P]
    if codes is not None:
        cv.copy_(torch.from_numpy(codes))
    wt = torch.full((Cn + 8,), float("nan"), device="cuda"); wv = wt[cwoff:cwoff + Cn]
    if cw is not None:
        wv.copy_(torch.from_numpy(np.asarray(cw, np.float32)))
    tt = torch.full((256 + 8,), float("nan"), device="cuda"); tv = tt[taboff:taboff + 256]
    if table is not None:
        tv.copy_(torch.from_numpy(np.asarray(table, np.float32)))
    assert zb.data_ptr() % 16 == 0 and db.data_ptr() % 16 == 0 and lb.data_ptr() % 16 == 0 and cb.data_ptr() % 16 == 0
    nwork = int(L.lib.fcn8s_op_focal_xent_work_bytes()) - work_cut
    wb = torch.full((nwork + GUARD,), work_fill, dtype=torch.uint8, device="cuda")
    wb[nwork:] = 0x5A
    ob = torch.full((1 + GUARD,), float(PAT), device="cuda")
    bb = torch.full((Cn + GUARD,), float(PAT), device="cuda")
    p = lambda t: C.c_void_p(t.data_ptr())
    args = dict(z=p(zv), lab=p(lv), cw=p(wv) if cw is not None else None, codes=p(cv) if codes is not None else None,
                table=p(tv) if table is not None else None, gamma=gamma, d=p(dv) if want_d else None, loss=p(ob), bias=p(bb) if want_bias else None,
                npix=P, C=Cn, work=p(wb), nwork=nwork)
    args.update(raw or {})
    s = C.c_void_p(stream.cuda_stream) if stream is not None else None
    rc = L.lib.fcn8s_op_focal_xent(s, args["z"], args["lab"], args["cw"], args["codes"], args["table"], args["gamma"], args["d"], args["loss"],
                                   args["bias"], args["npix"], args["C"], args["work"], args["nwork"])
    torch.cuda.synchronize()
    dall, oall, ball = db.cpu().numpy(), ob.cpu().numpy(), bb.cpu().numpy()
    assert (dall[:GUARD + doff] == PAT).all() and (dall[GUARD + doff + n:] == PAT).all(), "a guard word around dlogits was written"
    assert (oall[1:] == PAT).all() and (ball[Cn:] == PAT).all(), "a guard word behind loss_dev or bias_out was written"
    assert (wb[nwork:].cpu().numpy() == 0x5A).all(), "a guard byte behind work was written"
    assert (lb.cpu().numpy()[laboff + P:] == 7).all()
    if rc != L.OK or not want_bias:
        assert (ball == PAT).all(), "bias_out was written by a call that must leave it alone"
    if rc != L.OK or not want_d:
        assert (dall == PAT).all(), "dlogits was written by a call that must leave it alone"
    if rc != L.OK:
        assert oall[0] == PAT, "a refused call wrote loss_dev"
        assert (wb[:nwork].cpu().numpy() == work_fill).all(), "a refused call wrote work"
    return dict(rc=rc, loss=oall[0], d=dall[GUARD + doff:GUARD + doff + n].reshape(P, Cn).copy(), bias=ball[:Cn].copy() if want_bias else None)


def distances(got, ref, r32, what):
    """The device's distances to the float64 reference `ref` (dict loss, dlogits, bias) and the float32 restatement's own (E); asserts the bars."""
    dmax, col = np.abs(ref["dlogits"]).max(), np.abs(ref["dlogits"]).sum(0).max()
    if dmax == 0.0:                                                           # no valid pixel, or rows that all have a zero gradient
        assert abs(float(got["loss"]) - ref["loss"]) <= 1e-5 * abs(ref["loss"]) and not got["d"].any() and not got["bias"].any(), what
        return
    rel = lambda a, b, s: float(np.abs(np.asarray(a, np.float64) - b).max() / s) if s else float(np.abs(np.asarray(a, np.float64) - b).max())
    if ref["loss"] == 0.0:                                                    # (one confident pixel: l is 0 in double already)
        assert got["loss"] == 0.0 and r32["loss"] == 0.0, what
    dev = dict(loss=rel(got["loss"], ref["loss"], abs(ref["loss"])), d=rel(got["d"], ref["dlogits"], dmax), bias=rel(got["bias"], ref["bias"], col))
    E = dict(loss=rel(r32["loss"], ref["loss"], abs(ref["loss"])), d=rel(r32["dlogits"], ref["dlogits"], dmax), bias=rel(r32["bias"], ref["bias"], col))
    print("%s: device %s; float32 restatement E %s" % (what, {k: "%.2e" % v for k, v in dev.items()}, {k: "%.2e" % v for k, v in E.items()}))
    assert dev["loss"] <= max(1e-5, 8 * E["loss"]), (what, got["loss"], ref["loss"])
    assert dev["bias"] <= max(1e-5, 8 * E["bias"]), what
    assert dev["d"] <= max(2e-6, 8 * E["d"]), what


def exact_zeros(got, z, lab, K, r32):
    """Ignored rows, padding columns and rows with u = 0 (the float32 restatement says which: R / S == 0 there) are zeros."""
    Cn = z.shape[1]
    assert not got["d"][lab >= Cn].any() and not got["d"][:, K:].any()
    u0 = (r32["f"] == 0) & r32["valid"]
    assert not got["d"][u0].any()
    return int(u0.sum())


GOLDEN = golden()


@pytest.mark.parametrize("i", range(len(GOLDEN)), ids=[case_id(c) for c in GOLDEN])
def test_op_matches_the_golden_fixture(i):
    c = GOLDEN[i]
    got = run_op(c["logits"], c["labels"], c["gamma"], c["cw"], c["codes"], c["table"])
    assert got["rc"] == 0
    r32 = LM.focal_restate(c["logits"], c["labels"], c["gamma"], c["cw"], c["pw"], dtype=np.float32)
    distances(got, c, r32, "fixture " + case_id(c))
    distances(got, LM.focal_restate(c["logits"], c["labels"], c["gamma"], c["cw"], c["pw"]), r32, "  (restatement)")
    exact_zeros(got, c["logits"], c["labels"], c["K"], r32)


@pytest.mark.parametrize("Cn,K", CS)
@pytest.mark.parametrize("P", PS)
def test_op_matches_the_restatement(P, Cn, K):
    """The full cross product of the shapes and C; the gammas and the weightings in turn."""
    z, lab = make_case(P, Cn, K, 100 * P + Cn + K)
    cw = weights(Cn, K, P + Cn)
    codes, table = make_px(P, P + K)
    nzero = 0
    for j, gamma in enumerate(GAMMAS + (0.25, 8.0)):
        a_cw, a_px = (None, cw, cw, None)[(j + P) % 4], (None, None, (codes, table), (codes, table))[(j + P) % 4]
        pw = table[codes] if a_px else None
        got = run_op(z, lab, gamma, a_cw, *(a_px or (None, None)))
        assert got["rc"] == 0
        r32 = LM.focal_restate(z, lab, gamma, a_cw, pw, dtype=np.float32)
        distances(got, LM.focal_restate(z, lab, gamma, a_cw, pw), r32, "P=%d C=%d K=%d gamma=%g cw=%d px=%d" % (P, Cn, K, gamma, a_cw is not None, bool(a_px)))
        nzero += exact_zeros(got, z, lab, K, r32)
    assert nzero or P < 255                                                    # the inputs do hold rows with u = 0


@pytest.mark.parametrize("Cn,K", [(20, 19), (21, 21), (4, 4), (64, 64)])
@pytest.mark.parametrize("gamma", [0.5, 2.0])
def test_exactness_that_needs_no_tolerance(Cn, K, gamma):
    P = 600
    z, lab = make_case(P, Cn, K, 7 + Cn)
    cw = weights(Cn, K, 5)
    codes, table = make_px(P, 9)
    base = run_op(z, lab, gamma, cw, codes, table)
    again = run_op(z, lab, gamma, cw, codes, table)
    assert base["rc"] == again["rc"] == 0 and base["d"].any()
    bits = lambda a: np.ascontiguousarray(a, np.float32).view(np.uint32)
    for k in ("d", "bias", "loss"):                                           # two runs, identical bits
        assert np.array_equal(bits(base[k]), bits(again[k])), k
    # all weights x 2: the loss and every entry double.  On inputs without the + 40 and + 160 rows: there u^gamma and with it c_p fall below
    # FLT_MIN, where IEEE rounding of a product no longer commutes with doubling a factor; the moderate rows keep every product normal
    # (the smallest nonzero entry is asserted to be: an entry is e_c q <= q <= c_p <= a, so everything on its way is at least as large), and then every step of the definition is a product or quotient that doubles exactly.
    zm, lm = make_case(P, Cn, K, 7 + Cn, confident=False)
    once, twice = run_op(zm, lm, gamma, cw, codes, table), run_op(zm, lm, gamma, 2 * cw, codes, table)
    assert once["rc"] == twice["rc"] == 0 and np.abs(once["d"][once["d"] != 0]).min() > 4 * np.finfo(np.float32).tiny
    assert twice["loss"] == 2 * once["loss"] and np.array_equal(twice["d"], 2 * once["d"]) and np.array_equal(twice["bias"], 2 * once["bias"])
    # a table of 1.0 = no table; unit class weights = none
    plain = run_op(z, lab, gamma, cw)
    ones = run_op(z, lab, gamma, cw, codes, np.ones(256, np.float32))
    assert plain["loss"] == ones["loss"] and np.array_equal(plain["d"], ones["d"]) and np.array_equal(plain["bias"], ones["bias"])
    unit = run_op(z, lab, gamma, np.ones(Cn, np.float32))
    none = run_op(z, lab, gamma)
    assert unit["loss"] == none["loss"] and np.array_equal(unit["d"], none["d"]) and np.array_equal(unit["bias"], none["bias"])
    # a class weight 0 = relabelling that class to 255
    zc = 1 % K
    assert cw[zc] == 0 and (lab == zc).any()
    rel = run_op(z, np.where(lab == zc, 255, lab).astype(np.uint8), gamma, cw, codes, table)
    assert rel["loss"] == base["loss"] and np.array_equal(rel["d"], base["d"]) and np.array_equal(rel["bias"], base["bias"])
    assert not base["d"][lab == zc].any()
    # ignored rows, padding columns, rows with u = 0
    r32 = LM.focal_restate(z, lab, gamma, cw, table[codes], dtype=np.float32)
    assert exact_zeros(base, z, lab, K, r32) > 0


def test_gamma_one_is_the_cross_entropy_times_u():
    """gamma = 1 gives t = 1 exactly: the loss is sum u l / P."""
    z, lab = make_case(257, 20, 20, 23)
    got = run_op(z, lab, 1.0)
    r = LM.focal_restate(z, lab, 1.0)
    pl = LM.pixel_losses(z, lab)
    valid = lab < 20
    sm = np.exp(z.astype(np.float64) - z.max(1, keepdims=True)); sm /= sm.sum(1, keepdims=True)
    sm[np.nonzero(valid)[0], lab[valid]] = 0.0
    want = float((sm.sum(1)[valid] * pl[valid]).sum() / 257)
    assert abs(r["loss"] - want) <= 1e-12 * want and abs(float(got["loss"]) - want) <= 1e-5 * want


@pytest.mark.parametrize("Cn,K", [(20, 20), (20, 19), (21, 21), (64, 64)])
def test_every_alignment_of_the_pointers(Cn, K):
    z, lab = make_case(257, Cn, K, 11)
    cw = weights(Cn, K, 3)
    codes, table = make_px(257, 5)
    r, r32 = LM.focal_restate(z, lab, 2.0, cw, table[codes]), LM.focal_restate(z, lab, 2.0, cw, table[codes], dtype=np.float32)
    for zoff in range(4):
        for doff in range(4):
            got = run_op(z, lab, 2.0, cw, codes, table, zoff=zoff, doff=doff, laboff=(5 * zoff + 3 * doff) % 16, codeoff=(7 * zoff + doff) % 16,
                         cwoff=(zoff + doff) % 4, taboff=(zoff + 2 * doff) % 4)
            assert got["rc"] == 0
            distances(got, r, r32, "C=%d K=%d logits + %d floats, dlogits + %d floats" % (Cn, K, zoff, doff))
    base = run_op(z, lab, 2.0, cw, codes, table)
    for off in range(16):
        for kw in (dict(laboff=off), dict(codeoff=off)):
            got = run_op(z, lab, 2.0, cw, codes, table, **kw)
            assert got["rc"] == 0 and np.array_equal(got["d"], base["d"]) and got["loss"] == base["loss"] and np.array_equal(got["bias"], base["bias"]), kw


@pytest.mark.parametrize("Cn,K", [(20, 20), (21, 21)])
def test_work_prefill_and_null_outputs(Cn, K):
    z, lab = make_case(600, Cn, K, 13)
    cw = weights(Cn, K, 1)
    a = run_op(z, lab, 2.0, cw, work_fill=0xFF)
    b = run_op(z, lab, 2.0, cw, work_fill=0)
    assert a["rc"] == b["rc"] == 0 and a["loss"] == b["loss"] and np.array_equal(a["d"], b["d"]) and np.array_equal(a["bias"], b["bias"])
    n = run_op(z, lab, 2.0, cw, want_d=False)                                 # the loss and the column sums only (run_op: dlogits keeps its pattern)
    assert n["rc"] == 0 and n["loss"] == a["loss"] and np.array_equal(n["bias"], a["bias"])
    n = run_op(z, lab, 2.0, cw, want_bias=False)
    assert n["rc"] == 0 and n["loss"] == a["loss"] and np.array_equal(n["d"], a["d"])
    n = run_op(z, lab, 2.0, cw, want_d=False, want_bias=False)
    assert n["rc"] == 0 and n["loss"] == a["loss"]
    e = run_op(z, np.full(600, 255, np.uint8), 2.0, cw)                       # no valid pixel
    assert e["rc"] == 0 and e["loss"] == 0.0 and not e["d"].any() and not e["bias"].any()


def test_refusals_leave_every_output_untouched():
    L = _lib()
    z, lab = make_case(80, 20, 20, 17)
    codes, table = make_px(80, 1)
    cw = weights(20, 20, 1)
    assert run_op(z, lab, 2.0, cw, codes, table)["rc"] == 0
    bad = (dict(z=None), dict(lab=None), dict(work=None), dict(loss=None), dict(gamma=0.0), dict(gamma=-1.0), dict(gamma=8.5), dict(gamma=float("nan")),
           dict(gamma=float("inf")), dict(C=1), dict(C=65), dict(codes=None), dict(table=None), dict(nwork=0))
    for raw in bad:
        assert run_op(z, lab, 2.0, cw, codes, table, raw=raw)["rc"] == L.ERR_BAD_ARG, raw
    for raw in (dict(npix=0), dict(npix=-5)):
        assert run_op(z, lab, 2.0, cw, codes, table, raw=raw)["rc"] == L.ERR_SHAPE, raw
    assert run_op(z, lab, 2.0, cw, codes, table, work_cut=1)["rc"] == L.ERR_BAD_ARG      # a work one byte too small
    zt = torch.zeros(z.size + 4, device="cuda")                               # misaligned float pointers
    for k in ("z", "d", "loss", "bias", "cw", "table"):
        assert run_op(z, lab, 2.0, cw, codes, table, raw={k: C.c_void_p(zt.data_ptr() + 2)})["rc"] == L.ERR_BAD_ARG, k
    with pytest.raises(ValueError):
        L.check(L.lib.fcn8s_op_focal_xent(None, None, None, None, None, None, 2.0, None, None, None, 80, 20, None, 0))


def test_engine_wrapper():
    from tests.test_lovasz_gpu import SMALL, engine
    e = engine(SMALL)
    z, lab = make_case(600, 20, 20, 19)
    cw = weights(20, 20, 2)
    codes, table = make_px(600, 3)
    zt = torch.from_numpy(z.reshape(2, 20, 15, 20)).cuda(); lt = torch.from_numpy(lab.reshape(2, 20, 15)).cuda()
    ct = torch.from_numpy(codes.reshape(2, 20, 15)).cuda(); tt = torch.from_numpy(table).cuda(); wt = torch.from_numpy(cw).cuda()
    d = torch.full_like(zt, 3.5)
    loss, bias = e.focal_xent_op(zt, lt, 2.0, wt, ct, tt, dlogits=d, bias=True)
    r = LM.focal_restate(z, lab, 2.0, cw, table[codes])
    r32 = LM.focal_restate(z, lab, 2.0, cw, table[codes], dtype=np.float32)
    distances(dict(loss=loss.cpu().numpy()[0], d=d.cpu().numpy().reshape(-1, 20), bias=bias.cpu().numpy()), r, r32, "Engine.focal_xent_op")
    l2, b2 = e.focal_xent_op(zt, lt, 2.0, wt, ct, tt)
    assert b2 is None and l2.cpu().numpy()[0] == loss.cpu().numpy()[0]
    for bad in (dict(logits=zt.cpu()), dict(labels=lt.long()), dict(labels=lt[:1]), dict(dlogits=d[..., :19]), dict(gamma=9.0), dict(gamma=0.0),
                dict(codes=ct), dict(table=tt), dict(class_weights=wt[:19])):
        kw = dict(logits=zt, labels=lt, gamma=2.0)
        kw.update(bad)
        with pytest.raises(ValueError):
            e.focal_xent_op(**kw)
    e.close()


def test_every_block_trips_more_than_once():
    """2 x 512 x 1024 x 20: 4096 tiles over at most 1024 blocks."""
    P, Cn = 2 * 512 * 1024, 20
    gen = torch.Generator(device="cuda").manual_seed(3)
    zt = (torch.randn((P, Cn), device="cuda", generator=gen) * 3).contiguous()
    zt[::7, 3] += 40.0
    zt[14::28, 3] += 120.0
    lt = torch.randint(0, Cn, (P,), dtype=torch.uint8, device="cuda", generator=gen)
    lt[::14] = 3
    lt[torch.rand(P, device="cuda", generator=gen) < 0.2] = 255
    d = torch.full_like(zt, 3.5)
    L = _lib()
    work = torch.empty(int(L.lib.fcn8s_op_focal_xent_work_bytes()), dtype=torch.uint8, device="cuda")
    loss = torch.zeros(1, device="cuda"); bias = torch.zeros(Cn, device="cuda")
    p = lambda t: C.c_void_p(t.data_ptr())
    L.check(L.lib.fcn8s_op_focal_xent(None, p(zt), p(lt), None, None, None, 2.0, p(d), p(loss), p(bias), P, Cn, p(work), work.numel()))
    torch.cuda.synchronize()
    z, lab = zt.cpu().numpy(), lt.cpu().numpy()
    r, r32 = LM.focal_restate(z, lab, 2.0), LM.focal_restate(z, lab, 2.0, dtype=np.float32)
    got = dict(loss=loss.cpu().numpy()[0], d=d.cpu().numpy(), bias=bias.cpu().numpy())
    assert exact_zeros(got, z, lab, Cn, r32) > 0
    distances(got, r, r32, "2 x 512 x 1024 x 20")


# ---- a side stream: the op's row in the stream case table (tests/test_streams_host.py asks for one per entry point that takes a stream) -----------
@ST.row("focal_xent", ("fcn8s_op_focal_xent",))
class _FocalRow:
    @staticmethod
    def make(seed):
        P, Cn, K = (600, 20, 20) if seed == 1 else (513, 20, 19)
        z, lab = make_case(P, Cn, K, 40 + seed)
        codes, table = make_px(P, seed)
        nwork = int(_lib().lib.fcn8s_op_focal_xent_work_bytes())
        inp = dict(z=z, lab=lab, cw=weights(Cn, K, seed), codes=codes, table=table)
        poison = dict(lab=np.where(lab == 255, np.uint8(0), np.uint8(255)).astype(np.uint8), codes=(255 - codes).astype(np.uint8))
        out = dict(d=((P, Cn), np.float32), loss=((1,), np.float32), bias=((Cn,), np.float32), work=((nwork,), np.uint8))
        return ST.Case(inp, out, fetch=("d", "loss", "bias"), poison=poison, P=P, C=Cn, K=K)

    @staticmethod
    def call(L, s, b, case):
        a = case.aux
        p = ST.ptr
        L.check(L.lib.fcn8s_op_focal_xent(s, p(b["z"]), p(b["lab"]), p(b["cw"]), p(b["codes"]), p(b["table"]), 2.0, p(b["d"]), p(b["loss"]), p(b["bias"]),
                                          a["P"], a["C"], p(b["work"]), b["work"].numel()))

    @staticmethod
    def check(case, got):
        a, i = case.aux, case.inp
        pw = i["table"][i["codes"]]
        r, r32 = LM.focal_restate(i["z"], i["lab"], 2.0, i["cw"], pw), LM.focal_restate(i["z"], i["lab"], 2.0, i["cw"], pw, dtype=np.float32)
        distances(dict(loss=got["loss"][0], d=got["d"], bias=got["bias"]), r, r32, "stream row P = %d" % a["P"])


ROW = ST.ROWS[-1]
MAX_QUEUES = 4                                                   # HIP's default number of hardware queues (tests/test_strong_augment_streams_gpu.py)
CANARY_CASES = (("zero", "null_late"), ("producer", "side_late"), ("producer", "null_late"))      # run_canary's


@pytest.fixture(scope="module")
def harness():
    """As tests/test_entropy_term_ops_gpu.py: the first of up to MAX_QUEUES fresh harnesses whose side stream the canary can tell from the NULL
    stream (this file runs after several others have taken streams, and the runtime deals its hardware queues in turn)."""
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
    assert ROW.name == "focal_xent" and ROW.entries == ("fcn8s_op_focal_xent",) and ROW in ST.ROWS


@pytest.mark.parametrize("skew", ST.SKEWS)
def test_focal_xent_on_a_side_stream(skew, harness):
    ST.run_canary(harness)                                      # the harness sees a stray launch here and now
    case = ROW.make(1)
    ST.execute(ROW, ROW.make(2), None, None, None)              # default stream, other data: warm, and the row's host time
    want = ST.execute(ROW, case, None, None, None)
    ROW.check(case, want)
    ST.execute(ROW, ROW.make(2), harness, harness.S, "side_late" if skew == "null_late" else "null_late")
    got = ST.execute(ROW, case, harness, harness.S, skew)
    ROW.check(case, got)
    for name in ("d", "loss", "bias"):
        assert ST.same_bits(got[name], want[name]), name        # the default stream's result, bit for bit
