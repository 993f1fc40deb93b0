"""`fcn8s_op_class_mix` in the stream case table of tests/test_streams_gpu.py: the op on a side stream under both skews of that module's
harness (inputs that arrive late on the side stream; a NULL stream that runs late), against the golden fixture with `==`.

As in tests/test_pseudo_label_streams_gpu.py, whose harness fixture this file reuses, the row is registered on import (tests/test_streams_host.py
asks that every entry point taking a stream has one) and run here by the table's own `execute`."""
import numpy as np
import pytest
import torch  # noqa: F401

pytestmark = pytest.mark.gpu

from fcn8s_tensorflow_amd import class_mix as CM  # noqa: E402
from tests import test_streams_gpu as ST  # noqa: E402
from tests.test_class_mix_host import golden  # noqa: E402
from tests.test_pseudo_label_streams_gpu import harness  # noqa: E402,F401

OUTS = ("out_images", "out_labels", "selected")


def fixture_case(seed):
    """seed 1: 3 x 300 x 20 with a rotation, seed 2 (the warm-up on other data): 2 x 1025 x 20."""
    want = (3, 300, 20) if seed == 1 else (2, 1025, 20)
    return [c for c in golden() if (c["N"], c["P"], c["C"]) == want][0]


@ST.row("class_mix", ("fcn8s_op_class_mix",))
class _ClassMixRow:
    @staticmethod
    def make(seed):
        c = fixture_case(seed)
        N, P = c["N"], c["P"]
        inp = dict(images=np.array(c["images"]), labels=np.array(c["labels"]), src=np.array(c["src"]))
        poison = dict(src=np.roll(c["src"], 1))                                        # other sources, still in range
        out = dict(out_images=((N, P, 3), np.uint8), out_labels=((N, P), np.uint8), selected=((N, 256), np.uint8), work=((CM.work_bytes(N),), np.uint8))
        return ST.Case(inp, out, fetch=OUTS, poison=poison, c=c)

    @staticmethod
    def call(L, s, b, case):
        c = case.aux["c"]
        p = ST.ptr
        L.check(L.lib.fcn8s_op_class_mix(s, p(b["images"]), p(b["labels"]), p(b["src"]), c["N"], c["P"], c["C"], c["seed"], c["draw"], p(b["work"]),
                                         p(b["out_images"]), p(b["out_labels"]), p(b["selected"])))

    @staticmethod
    def check(case, got):
        c = case.aux["c"]
        for name in OUTS:
            assert np.array_equal(got[name], c[name]), name


ROW = ST.ROWS[-1]


def test_the_row_is_in_the_table():
    assert ROW.name == "class_mix" and ROW.entries == ("fcn8s_op_class_mix",) and ROW in ST.ROWS


@pytest.mark.parametrize("skew", ST.SKEWS)
def test_class_mix_on_a_side_stream(skew, harness):  # noqa: F811
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
