"""`fcn8s_op_pseudo_label` in the stream case table of tests/test_streams_gpu.py: the op on a side stream under both skews of that module's
harness (inputs that arrive late on the side stream; a NULL stream that runs late), against the golden fixture with `==`.

The row is registered from this file: importing it appends the row to `tests.test_streams_gpu.ROWS`, which is what
tests/test_streams_host.py reads when it asks that every entry point taking a stream has a row (pytest imports every test module of the
directory before it runs a test).  The table's own parametrised test was sized when that module was imported, so the row is run here, by
the same `execute`."""
import numpy as np
import pytest
import torch  # noqa: F401

pytestmark = pytest.mark.gpu

from fcn8s_tensorflow_amd import pseudo_label as PL  # noqa: E402
from tests import test_streams_gpu as ST  # noqa: E402
from tests.test_pseudo_label_host import golden  # noqa: E402

TABLES = ("hist", "counts", "misc")


def fixture_case(seed):
    """seed 1: 2 x 300 x 20, seed 2 (the warm-up on other data): 1 x 513 x 20."""
    want = (2, 300, 20) if seed == 1 else (1, 513, 20)
    return [c for c in golden()[1] if (c["N"], c["P"], c["C"]) == want][0]


@ST.row("pseudo_label", ("fcn8s_op_pseudo_label",))
class _PseudoLabelRow:
    @staticmethod
    def make(seed):
        c = fixture_case(seed)
        N, P, Cn = c["N"], c["P"], c["C"]
        z = lambda *s: np.zeros(s, np.int64)
        inp = dict(prob=np.array(c["prob"]), thr=np.array(c["thr"]), oid=np.array(c["out_ids"]), base=np.array(c["base"]), score=np.array(c["score"]),
                   hist=z(Cn, PL.BINS), counts=z(Cn, 2), misc=z(3))
        poison = {k: np.full(inp[k].shape, 1 << 40, np.int64) for k in TABLES}
        poison["base"] = np.where(c["base"] == c["base_fill"], 0, c["base_fill"]).astype(np.uint8)        # the other pixels are passed through
        return ST.Case(inp, dict(labels=((N, P), np.uint8)), fetch=("labels",) + TABLES, poison=poison, c=c)

    @staticmethod
    def call(L, s, b, case):
        c = case.aux["c"]
        p = ST.ptr
        L.check(L.lib.fcn8s_op_pseudo_label(s, p(b["prob"]), c["N"], c["P"], c["C"], p(b["thr"]), p(b["oid"]), 250, p(b["base"]), c["base_fill"],
                                            p(b["score"]), c["score_max"], p(b["labels"]), p(b["hist"]), p(b["counts"]), p(b["misc"])))

    @staticmethod
    def check(case, got):
        c = case.aux["c"]
        for name in ("labels",) + TABLES:
            assert np.array_equal(got[name], c["A_" + name]), name


ROW = ST.ROWS[-1]


@pytest.fixture(scope="module")
def harness():
    """The stream module's harness with the op delay at its floor; `execute` raises it to four times the row's own measured host time."""
    h = ST.Harness()
    h.longest_ms, h.longest_host_ms = 0.0, 0.0
    h.set_delay("op", 0.0)
    return h


def test_the_row_is_in_the_table():
    assert ROW.name == "pseudo_label" and ROW.entries == ("fcn8s_op_pseudo_label",) and ROW in ST.ROWS


@pytest.mark.parametrize("skew", ST.SKEWS)
def test_pseudo_label_on_a_side_stream(skew, harness):
    ST.run_canary(harness)                                      # the harness sees a stray launch here and now
    case = ROW.make(1)
    ST.execute(ROW, ROW.make(2), None, None, None)              # default stream, other data: warm, and the row's host time
    want = ST.execute(ROW, case, None, None, None)
    ROW.check(case, want)
    ST.execute(ROW, ROW.make(2), harness, harness.S, "side_late" if skew == "null_late" else "null_late")
    got = ST.execute(ROW, case, harness, harness.S, skew)
    ROW.check(case, got)
    for name in ("labels",) + TABLES:
        assert ST.same_bits(got[name], want[name]), name        # the default stream's result, bit for bit
