"""`fcn8s_op_fda_transfer` in the stream case table of tests/test_streams_gpu.py: the op on a side stream under both skews of that module's harness
(inputs that arrive late on the side stream; a NULL stream that runs late), within the fixture's bar of tests/test_fda_ops_gpu.py, and bit for bit
the default stream's result.  Six kernels pass G, F, D and S on through `work`: one of them on the NULL stream would read what the side stream has
not written yet, or write what it has already read.

As in tests/test_strong_augment_streams_gpu.py the row is registered on import (tests/test_streams_host.py asks that every entry point taking a
stream has one) and run here by the table's own `execute`, on the first of up to MAX_QUEUES fresh harnesses whose side stream the canary can tell
from the NULL stream."""
import numpy as np
import pytest
import torch  # noqa: F401

pytestmark = pytest.mark.gpu

from fcn8s_tensorflow_amd import fda as FDA  # noqa: E402
from tests import test_streams_gpu as ST  # noqa: E402
from tests.test_fda_host import golden, restated32  # noqa: E402

OUTS = ("out_u8", "out_f32")
FLOOR = float(np.spacing(np.float32(256)))


def fixture_case(seed):
    """seed 1: the batch of 3 + 2 images of 16 x 24 at b = 2 with pair = [1, 0, 1]; seed 2 (the warm-up on other data): 33 x 129 at b = 16."""
    i = [k for k, c in enumerate(golden()) if c["name"].startswith("batch" if seed == 1 else "33x129 b=16")][0]
    return i, golden()[i]


@ST.row("fda_transfer", ("fcn8s_op_fda_transfer",))
class _FdaRow:
    @staticmethod
    def make(seed):
        i, c = fixture_case(seed)
        inp = dict(images=np.array(c["images"]), targets=np.array(c["targets"]), pair=c["pair"].astype(np.int32))
        poison = dict(images=np.ascontiguousarray(c["images"][:, ::-1]), targets=np.ascontiguousarray(c["targets"][:, :, ::-1]),
                      pair=np.zeros(c["N"], np.int32))                                   # other images of the same kind, another pairing
        out = dict(out_u8=(c["images"].shape, np.uint8), out_f32=(c["images"].shape, np.float32),
                   work=((FDA.work_bytes(c["N"], c["M"], c["H"], c["W"], c["b"]),), np.uint8))
        return ST.Case(inp, out, fetch=OUTS, poison=poison, c=c, E=restated32(i)[1])

    @staticmethod
    def call(L, s, b, case):
        c = case.aux["c"]
        p = ST.ptr
        L.check(L.lib.fcn8s_op_fda_transfer(s, p(b["images"]), c["N"], p(b["targets"]), c["M"], c["H"], c["W"], c["b"], p(b["pair"]), p(b["work"]),
                                            p(b["out_u8"]), p(b["out_f32"])))

    @staticmethod
    def check(case, got):
        c, bar = case.aux["c"], 8.0 * max(case.aux["E"], FLOOR)
        assert np.abs(got["out_f32"].astype(np.float64) - c["y"]).max() <= bar, "out_f32"
        assert np.abs(got["out_u8"].astype(np.float64) - np.clip(c["y"], 0, 255)).max() <= 0.5 + bar, "out_u8"


ROW = ST.ROWS[-1]
MAX_QUEUES = 4                                                   # HIP's default number of hardware queues (tests/test_strong_augment_streams_gpu.py)
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
    assert ROW.name == "fda_transfer" and ROW.entries == ("fcn8s_op_fda_transfer",) and ROW in ST.ROWS
    _, c = fixture_case(1)
    assert c["pair"].tolist() == [1, 0, 1] and c["b"] == 2 and (np.abs(c["y"] - c["images"]) > 1).any()     # the op changes the images


@pytest.mark.parametrize("skew", ST.SKEWS)
def test_fda_transfer_on_a_side_stream(skew, harness):
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
