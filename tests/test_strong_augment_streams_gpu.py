"""`fcn8s_op_strong_augment` in the stream case table of tests/test_streams_gpu.py: the op on a side stream under both skews of that module's
harness (inputs that arrive late on the side stream; a NULL stream that runs late), against the golden fixture with `==`.  The case has a
contrast strength, so all three kernels run: a grey sum or a clear of it that went to the NULL stream would move the mean grey.

As in tests/test_pseudo_label_streams_gpu.py the row is registered on import (tests/test_streams_host.py asks that every entry point taking a
stream has one) and run here by the table's own `execute`.  The harness is that module's -- the stream module's `Harness` with the op delay at
its floor -- made here with one addition: this file sorts behind tests/test_streams_gpu.py, so by the time it runs the process has handed out
several side streams, and the runtime deals its few hardware queues to new streams in turn; a side stream that lands on the NULL stream's
queue is ordered against it and the canary, rightly, sees nothing.  The fixture therefore makes up to MAX_QUEUES harnesses, keeps them all
alive, and takes the first whose side stream the canary can tell from the NULL stream; if none can, it fails as `run_canary` would."""
import ctypes as C

import numpy as np
import pytest
import torch  # noqa: F401

pytestmark = pytest.mark.gpu

from fcn8s_tensorflow_amd import strong_augment as SA  # noqa: E402
from tests import test_streams_gpu as ST  # noqa: E402
from tests.test_strong_augment_host import golden  # noqa: E402

OUTS = ("out_images", "params")


def fixture_case(seed):
    """seed 1: the batch of 3 x 48 x 80 whose images draw different gates, seed 2 (the warm-up on other data): 2 x 33 x 63, every stage."""
    want = (3, 48, 80) if seed == 1 else (2, 33, 63)
    return [c for c in golden() if (c["N"], c["H"], c["W"]) == want][0]


@ST.row("strong_augment", ("fcn8s_op_strong_augment",))
class _StrongAugmentRow:
    @staticmethod
    def make(seed):
        c = fixture_case(seed)
        N = c["N"]
        inp = dict(images=np.array(c["images"]))
        poison = dict(images=np.ascontiguousarray(c["images"][:, ::-1]))                 # another image of the same kind
        out = dict(out_images=(c["images"].shape, np.uint8), params=((N, 8), np.int32), work=((SA.work_bytes(N),), np.uint8))
        return ST.Case(inp, out, fetch=OUTS, poison=poison, c=c)

    @staticmethod
    def call(L, s, b, case):
        c = case.aux["c"]
        p = ST.ptr
        gate, taps = c["blur"]
        jit = (C.c_int32 * 5)(*[int(v) for v in c["jitter"]])
        blur = (C.c_int32 * 3)(gate, taps.shape[0], taps.shape[1] - 1)
        flat = (C.c_uint16 * taps.size)(*[int(v) for v in taps.reshape(-1)])
        L.check(L.lib.fcn8s_op_strong_augment(s, p(b["images"]), c["N"], c["H"], c["W"], c["seed"], c["draw"], jit, blur, flat, p(b["work"]),
                                              p(b["out_images"]), p(b["params"])))

    @staticmethod
    def check(case, got):
        c = case.aux["c"]
        assert np.array_equal(got["out_images"], c["out_images"]), "out_images"
        assert np.array_equal(got["params"], c["params"]), "params"


ROW = ST.ROWS[-1]
MAX_QUEUES = 4                                                   # HIP's default number of hardware queues: that many streams in a row cannot all share the NULL stream's
CANARY_CASES = (("zero", "null_late"), ("producer", "side_late"), ("producer", "null_late"))      # run_canary's


@pytest.fixture(scope="module")
def harness():
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
    assert ROW.name == "strong_augment" and ROW.entries == ("fcn8s_op_strong_augment",) and ROW in ST.ROWS
    c = fixture_case(1)
    assert c["jitter"][1] != 0 and c["params"][:, 0].any() and c["params"][:, 6].any()    # the grey sum, the colour step and the blur all run


@pytest.mark.parametrize("skew", ST.SKEWS)
def test_strong_augment_on_a_side_stream(skew, harness):
    ST.run_canary(harness)                                      # the harness sees a stray launch here and now
    case = ROW.make(1)
    ST.execute(ROW, ROW.make(2), None, None, None)              # default stream, other data: warm, and the row's host time
    want = ST.execute(ROW, case, None, None, None)
    ROW.check(case, want)
    ST.execute(ROW, ROW.make(2), harness, harness.S, "side_late" if skew == "null_late" else "null_late")
    got = ST.execute(ROW, case, harness, harness.S, skew)
    ROW.check(case, got)
    for name in OUTS:
        assert ST.same_bits(got[name], want[name]), name        # the default stream's result, bit for bit
