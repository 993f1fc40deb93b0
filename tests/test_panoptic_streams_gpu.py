"""`fcn8s_op_panoptic_pair` in the stream case table of tests/test_streams_gpu.py: the op on a side stream under both skews of that module's
harness (inputs that arrive late on the side stream; a NULL stream that runs late), against the NumPy route with `==`.

The row is registered from this file: importing it appends the row to `tests.test_streams_gpu.ROWS`, which is what
tests/test_streams_host.py reads when it asks that every entry point taking a stream has a row (pytest imports every test module of the
directory before it runs a test).  The table's own parametrised test was sized when that module was imported, so the row is run here, by
the same `execute`."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from fcn8s_tensorflow_amd import panoptic as PQ, regions as RG  # noqa: E402
from tests import test_streams_gpu as ST  # noqa: E402

N, HH, WW = 2, 48, 80
SLOTS, MAX_ROWS = 2048, 1024


@ST.row("panoptic_pair", ("fcn8s_op_panoptic_pair",), bitwise=False)     # (the rows' order is unspecified: check() sorts and compares with ==)
class _PanopticRow:
    @staticmethod
    def make(seed):
        rng = np.random.default_rng(seed)
        blocks = rng.choice([7, 8, 21, 23, 26001, 26002, 24001, 26, 4, 0], (N, HH // 8, WW // 8))
        inst = np.kron(blocks, np.ones((8, 8), np.int64)).astype(np.uint16)
        lab = np.where(inst < 1000, inst, inst // 1000)
        from fcn8s_tensorflow_amd import cityscapes_eval as ce
        pred = np.roll(ce.IDS_TO_TRAINIDS_ARRAY[lab].astype(np.int64), (1, 2), (1, 2))
        salt = rng.random(pred.shape) < 0.05
        pred[salt] = rng.integers(0, 20, int(salt.sum()))
        comp = RG.components_numpy(pred, 4)[0]
        want = PQ.pair_rows_numpy(pred, inst, 4)
        return ST.Case(dict(inst=inst, pred=pred, comp=comp),
                       dict(rows=((N, MAX_ROWS, 3), np.int64), counts=((N, 4), np.int64), table=((16 * N * SLOTS,), np.uint8)),
                       fetch=("rows", "counts"), want=want)

    @staticmethod
    def call(L, s, b, case):
        p = ST.ptr
        L.check(L.lib.fcn8s_op_panoptic_pair(s, p(b["inst"]), p(b["pred"]), 0, p(b["comp"]), N, HH, WW, p(b["table"]), SLOTS, p(b["rows"]), MAX_ROWS, p(b["counts"])))

    @staticmethod
    def check(case, got):
        want_rows, want_bad = case.aux["want"]
        for n in range(N):
            assert got["counts"][n].tolist() == [len(want_rows[n]), want_bad[n], 0, HH * WW - want_bad[n]], (n, got["counts"][n])
            assert np.array_equal(PQ.sort_rows(got["rows"][n, :len(want_rows[n])]), want_rows[n]), n


ROW = ST.ROWS[-1]


@pytest.fixture(scope="module")
def harness():
    """The stream module's harness with the op delay at its floor; `execute` raises it to four times the row's own measured host time."""
    h = ST.Harness()
    h.longest_ms, h.longest_host_ms = 0.0, 0.0
    h.set_delay("op", 0.0)
    return h


def test_the_row_is_in_the_table():
    assert ROW.name == "panoptic_pair" and ROW.entries == ("fcn8s_op_panoptic_pair",) and ROW in ST.ROWS


@pytest.mark.parametrize("skew", ST.SKEWS)
def test_panoptic_pair_on_a_side_stream(skew, harness):
    ST.run_canary(harness)                                      # the harness sees a stray launch here and now
    case = ROW.make(1)
    ST.execute(ROW, ROW.make(2), None, None, None)              # default stream, other data: warm, and the row's host time
    want = ST.execute(ROW, case, None, None, None)
    ROW.check(case, want)
    ST.execute(ROW, ROW.make(2), harness, harness.S, "side_late" if skew == "null_late" else "null_late")
    got = ST.execute(ROW, case, harness, harness.S, skew)
    ROW.check(case, got)
    assert np.array_equal(got["counts"], want["counts"])
    for n in range(N):
        k = int(want["counts"][n, 0])
        assert np.array_equal(PQ.sort_rows(got["rows"][n, :k]), PQ.sort_rows(want["rows"][n, :k]))           # the default stream's rows, bit for bit
