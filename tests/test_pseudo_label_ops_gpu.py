"""`fcn8s_op_pseudo_label` (csrc/pseudo_label.hip) against tests/golden/pseudo_label_cases.npz and `pseudo_label.tables_numpy` with `==` in the
labels and in every table: nothing but integers decides anything.

Shapes are the smallest at which each path of the kernel can go wrong: the fixture's pixel counts around the tile (255, 256, 257, 513, a batch
of 2 x 300), C = 20 (16-byte path with the next tile's loads in registers), C = 64 (16-byte rows too long for the LDS image: read from global
memory), C = 2, 19, 21 (generic path), every float offset of `prob` (an offset puts C = 20 on the generic path), every byte offset of `base`
and `labels_out` within a 16-byte line (the packed label stores and their ragged ends), float offsets of `score`; one 2 x 512 x 1024 x 20
batch (eight trips per block), and one batch whose blocks each meet more distinct (class, bin) keys than their 2048 LDS slots hold, so that
counts reach the histogram through the spill to global memory."""
import ctypes as C

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from fcn8s_tensorflow_amd import _lib as L, pseudo_label as PL  # noqa: E402
from tests.test_pseudo_label_host import golden, case_ids, full_args  # noqa: E402

M = PL.BINS
GUARD = 0xA5
NAMES = ("labels", "hist", "counts", "misc")


def dev_at(a, off=0):
    """A device copy of `a` (flat) whose first element lies `off` elements behind an allocation's (256-byte aligned) start."""
    flat = torch.from_numpy(np.array(a).reshape(-1))
    buf = torch.zeros(flat.numel() + off, dtype=flat.dtype, device="cuda")
    buf[off:].copy_(flat)
    return buf[off:]


def ptr(t):
    return C.c_void_p(t.data_ptr()) if t is not None else None


def call(prob, N, P, Cn, thr=None, oid=None, ignore_id=255, base=None, base_fill=0, score=None, score_max=0.0, labels=None, hist=None, counts=None,
         misc=None, stream=None):
    return L.lib.fcn8s_op_pseudo_label(stream, ptr(prob), N, P, Cn, ptr(thr), ptr(oid), ignore_id, ptr(base), base_fill, ptr(score), score_max,
                                       ptr(labels), ptr(hist), ptr(counts), ptr(misc))


class Out:
    """labels_out with 64 guard bytes on either side at a byte offset, and the three tables in one buffer with 8 guard words behind each."""

    def __init__(self, T, Cn, lab_off=0, fill=0, labels=True, hist=True):
        self.T, self.Cn, self.fill = T, Cn, fill
        self.lab_buf = torch.full((64 + lab_off + T + 64,), GUARD, dtype=torch.uint8, device="cuda")
        self.labels = self.lab_buf[64 + lab_off: 64 + lab_off + T] if labels else None
        self.lab_off = lab_off
        sizes = (Cn * M, Cn * 2, 3)
        self.tab_buf = torch.full((sum(sizes) + 24,), -GUARD, dtype=torch.int64, device="cuda")
        self.tabs, o = [], 0
        for n in sizes:
            self.tabs.append(self.tab_buf[o:o + n]); self.tabs[-1].fill_(fill); o += n + 8
        self.hist = self.tabs[0] if hist else None
        self.counts, self.misc = self.tabs[1], self.tabs[2]

    def kw(self):
        return dict(labels=self.labels, hist=self.hist, counts=self.counts, misc=self.misc)

    def fetch(self):
        """(labels, hist, counts, misc) as NumPy, the prefill taken off the tables, after checking every guard."""
        torch.cuda.synchronize()
        lb = self.lab_buf.cpu().numpy()
        a, b = 64 + self.lab_off, 64 + self.lab_off + self.T
        assert (lb[:a] == GUARD).all() and (lb[b:] == GUARD).all(), "a byte outside labels_out was written"
        tb = self.tab_buf.cpu().numpy()
        Cn, o, out = self.Cn, 0, []
        for n, shape in ((Cn * M, (Cn, M)), (Cn * 2, (Cn, 2)), (3, (3,))):
            assert (tb[o + n:o + n + 8] == -GUARD).all(), "a word behind a table was written"
            out.append(tb[o:o + n].reshape(shape) - self.fill); o += n + 8
        return (lb[a:b].copy(),) + tuple(out)


def run(prob, thresholds=None, out_ids=None, ignore_id=255, base=None, base_fill=None, score=None, score_max=None, prob_off=0, base_off=0, score_off=0,
        lab_off=0, fill=0, labels=True, hist=True, out=None):
    """prob [N,P,C] (NumPy) and the optional inputs through the op at the given element offsets; returns (labels [N,P], hist, counts, misc)."""
    N, P, Cn = prob.shape
    out = out or Out(N * P, Cn, lab_off, fill, labels, hist)
    keep = [dev_at(prob, prob_off), None if thresholds is None else dev_at(np.asarray(thresholds, np.float32)),
            None if out_ids is None else dev_at(np.asarray(out_ids, np.uint8)), None if base is None else dev_at(base, base_off),
            None if score is None else dev_at(score, score_off)]
    L.check(call(keep[0], N, P, Cn, keep[1], keep[2], ignore_id, keep[3], base_fill or 0, keep[4], float(score_max or 0.0), **out.kw()))
    got = out.fetch()
    return (got[0].reshape(N, P) if got[0].size == N * P else got[0],) + got[1:]        # (a shared `out` holds more than this call's pixels)


def same(got, want, tag="", names=NAMES):
    for g, w, name in zip(got, want, NAMES):
        if name in names:
            assert g.shape == w.shape and (g == w).all(), (tag, name, np.argwhere(g != w)[:8])


def want_of(c, v):
    return tuple(c["%s_%s" % (v, n)] for n in NAMES)


@pytest.mark.parametrize("i", range(len(golden()[0]["cases"])), ids=case_ids())
def test_the_op_equals_the_fixture(i):
    c = golden()[1][i]
    same(run(c["prob"], **full_args(c)), want_of(c, "A"), "A")
    same(run(c["prob"]), want_of(c, "B"), "B")
    thr = (c["fit_bins"].astype(np.float64) / M).astype(np.float32)
    got = run(c["prob"], thresholds=thr)
    assert (got[0] == c["C_labels"]).all() and (got[2] == c["C_counts"]).all()
    ok = (c["fit_bins"] > 0) & (c["fit_bins"] < M)
    assert (got[2][:, 0][ok] == PL.tail_sums(c["B_hist"], c["fit_bins"])[ok]).all()       # the second sweep keeps the first one's tail


def pick(P, Cn, N=1):
    return [c for c in golden()[1] if (c["N"], c["P"], c["C"]) == (N, P, Cn)][0]


@pytest.mark.parametrize("Cn", [20, 19, 64])
@pytest.mark.parametrize("off", [0, 1, 2, 3])
def test_every_float_offset_of_prob_and_of_score(off, Cn):
    c = pick(257, Cn)
    same(run(c["prob"], prob_off=off, score_off=(off + 1) % 4, **full_args(c)), want_of(c, "A"), "prob + %d floats" % off)


@pytest.mark.parametrize("off", range(16))
def test_every_byte_offset_of_labels_out_and_base(off):
    for c in (pick(513, 20), pick(300, 19, 2), pick(15, 20)):
        same(run(c["prob"], lab_off=off, base_off=(5 * off + 3) % 16, **full_args(c)), want_of(c, "A"), "labels_out + %d bytes" % off)
        same(run(c["prob"], lab_off=off, hist=False), want_of(c, "B"), "no hist, + %d bytes" % off, ("labels", "counts", "misc"))


def test_tables_are_accumulated_into_and_a_split_of_the_pixels_gives_the_same_tables():
    c = pick(513, 20)
    a = full_args(c)
    same(run(c["prob"], fill=1 << 40, **a), want_of(c, "A"), "prefilled")
    for cut in (1, 256, 300):
        out = Out(513, 20)
        first = {k: (v[:, :cut] if k in ("base", "score") else v) for k, v in a.items()}
        rest = {k: (v[:, cut:] if k in ("base", "score") else v) for k, v in a.items()}
        out.labels = out.lab_buf[64:64 + cut]
        run(c["prob"][:, :cut], out=out, **first)
        out.labels = out.lab_buf[64 + cut:64 + 513]
        run(c["prob"][:, cut:], prob_off=cut % 4, out=out, **rest)
        out.labels = out.lab_buf[64:64 + 513]
        got = out.fetch()
        same((got[0].reshape(1, 513),) + got[1:], want_of(c, "A"), "split at %d" % cut)


def test_two_runs_give_the_same_bits():
    c = pick(300, 20, 2)
    one, two = run(c["prob"], **full_args(c)), run(c["prob"], **full_args(c))
    assert all(x.tobytes() == y.tobytes() for x, y in zip(one, two))


def test_each_optional_pointer_may_be_null():
    c = pick(513, 20)
    full = full_args(c)
    for drop in ("thresholds", "out_ids", ("base", "base_fill"), ("score", "score_max")):
        kw = {k: v for k, v in full.items() if k not in (drop if isinstance(drop, tuple) else (drop,))}
        same(run(c["prob"], **kw), PL.tables_numpy(c["prob"], **kw), "without %s" % (drop,))
    want = want_of(c, "A")
    same(run(c["prob"], hist=False, **full), want, "hist NULL", ("labels", "counts", "misc"))
    kw = {k: v for k, v in full.items() if k not in ("base", "base_fill")}                      # the fit sweep: tables only (and so no base)
    same(run(c["prob"], labels=False, **kw), PL.tables_numpy(c["prob"], **kw), "labels_out NULL", ("hist", "counts", "misc"))


def test_bad_arguments_return_their_code_and_launch_nothing():
    c = pick(257, 20)
    out = Out(257, 20, fill=7)
    p, b, s = dev_at(c["prob"]), dev_at(c["base"]), dev_at(c["score"])
    ok = dict(prob=p, N=1, P=257, Cn=20, ignore_id=255, base=b, base_fill=255, score=s, score_max=0.05, **out.kw())
    bad = [dict(prob=None), dict(counts=None), dict(misc=None), dict(labels=None, hist=None, base=None), dict(N=0), dict(N=-1), dict(P=0), dict(P=-3),
           dict(Cn=1), dict(Cn=0), dict(Cn=256), dict(ignore_id=-1), dict(ignore_id=256), dict(base_fill=-1), dict(base_fill=256),
           dict(labels=None), dict(score_max=float('nan')), dict(score_max=float('inf')), dict(score_max=float('-inf'))]
    for kw in bad:
        assert call(**{**ok, **kw}) == L.ERR_BAD_ARG, kw
    assert call(**{**ok, "P": 1 << 31}) == L.ERR_SHAPE
    got = out.fetch()
    assert (got[0] == GUARD).all() and all((t == 0).all() for t in got[1:])                      # (fetch takes the prefill off)
    assert call(**ok) == L.OK                                                                    # the same arguments, unspoilt, are taken
    got = out.fetch()
    assert got[2].sum() + got[3][0] + got[3][1] == 257 and (got[0] != GUARD).any()


def test_a_batch_of_two_512_by_1024_images():
    rng = np.random.default_rng(7)
    N, P, Cn = 2, 512 * 1024, 20
    z = rng.standard_normal((N, P, Cn), np.float32) * rng.choice(np.array([0.5, 3.0, 10.0], np.float32), (N, P, 1))
    e = np.exp(z - z.max(-1, keepdims=True))
    prob = e / e.sum(-1, keepdims=True)
    prob[0, 1000] = np.nan
    thr = np.linspace(0.3, 0.9, Cn).astype(np.float32)
    base = rng.integers(0, 34, (N, P)).astype(np.uint8); base[rng.random((N, P)) < 0.5] = 255
    score = (rng.random((N, P), np.float32) * np.float32(0.1)); score[1, 77] = np.nan
    kw = dict(thresholds=thr, out_ids=golden()[1][0]["out_ids"], ignore_id=250, base=base, base_fill=255, score=score, score_max=0.05)
    want = PL.tables_numpy(prob, **kw)
    got = run(prob, lab_off=3, **kw)
    same(got, want, "2 x 512 x 1024 x 20")
    assert got[2].sum() + got[3][0] + got[3][1] == N * P


def test_more_keys_than_a_block_has_slots_reach_the_histogram_through_global_memory():
    """4 Mi pixels on the kernel's MAX_BLOCKS = 512 blocks: a block takes the tiles b, b + 512, ... -- 8192 pixels whose confidences are spread
    evenly over [0.2, 1) in 8 classes, more than 2048 distinct (class, bin) keys (counted below for block 0), so some cannot be in its 2048
    slots."""
    rng = np.random.default_rng(11)
    T, Cn = 1 << 22, 8
    conf = (np.float32(0.2) + rng.random(T, np.float32) * np.float32(0.8)).astype(np.float32)
    k = rng.integers(0, Cn, T)
    prob = np.repeat(((1 - conf) / np.float32(Cn - 1))[:, None], Cn, 1) * np.float32(0.5)
    prob[np.arange(T), k] = conf
    tiles = np.arange(T // PL.TILE_PIXELS).reshape(-1, PL.MAX_BLOCKS)[:, 0]
    px = (tiles[:, None] * PL.TILE_PIXELS + np.arange(PL.TILE_PIXELS)).reshape(-1)
    assert len(np.unique(k[px] * M + PL.bins_of(conf[px]))) > 2048
    want = PL.tables_numpy(prob[None])
    got = run(prob[None])
    same(got, want, "spill")
    assert got[1].sum() == T
