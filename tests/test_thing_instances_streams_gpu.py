"""`fcn8s_op_instance_pair` in the stream case table of tests/test_streams_gpu.py: the op on a side stream under both skews of that module's
harness (inputs that arrive late on the side stream; a NULL stream that runs late), against the NumPy route with `==`.

The row is registered from this file: importing it appends the row to `tests.test_streams_gpu.ROWS`, which is what
tests/test_streams_host.py reads when it asks that every entry point taking a stream has a row (pytest imports every test module of the
directory before it runs a test).  The table's own parametrised test was sized when that module was imported, so the row is run here, by
the same `execute`.

Like every module that runs the harness's canary, this one needs its side stream on another hardware queue than the NULL stream, and streams
take the process's hardware queues in turn.  The GPU test modules of the instance table therefore sort behind tests/test_streams_gpu.py: the
streams they take come after those of every other module that runs the canary, and leave them on the queues they had."""
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from fcn8s_tensorflow_amd import instances as INS, regions as RG  # noqa: E402
from tests import test_streams_gpu as ST  # noqa: E402

N, HH, WW = 2, 48, 80
SLOTS, MAX_ROWS = 2048, 1024
GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "instance_ap_cases.npz")


@ST.row("instance_pair", ("fcn8s_op_instance_pair",), bitwise=False)     # (the rows' order is unspecified: check() sorts and compares with ==)
class _InstanceRow:
    @staticmethod
    def make(seed):
        z = np.load(GOLD)
        shift = (3 * seed, 5 * seed)
        labels = np.roll(z["scene_c4_labels"], shift, (1, 2)); prob = np.roll(z["scene_c4_prob"], shift, (1, 2)); inst = np.roll(z["scene_c4_inst"], seed, 2)
        comp = RG.components_numpy(labels, 4)[0].astype(np.int32)
        want = INS.pair_rows_numpy(prob, labels, inst, 4, comp=comp)
        return ST.Case(dict(prob=prob, labels=labels, comp=comp, inst=inst),
                       dict(rows=((N, MAX_ROWS, 4), np.int64), counts=((N, 5), np.int64), table=((32 * N * SLOTS,), np.uint8)),
                       fetch=("rows", "counts"), want=want)

    @staticmethod
    def call(L, s, b, case):
        p = ST.ptr
        L.check(L.lib.fcn8s_op_instance_pair(s, p(b["prob"]), 20, p(b["labels"]), p(b["comp"]), p(b["inst"]), N, HH, WW, p(b["table"]), SLOTS,
                                             p(b["rows"]), MAX_ROWS, p(b["counts"])))

    @staticmethod
    def check(case, got):
        want_rows, want_bad = case.aux["want"]
        for n in range(N):
            assert got["counts"][n].tolist() == [len(want_rows[n]), want_bad[n][0], 0, HH * WW, want_bad[n][1]], (n, got["counts"][n])
            assert np.array_equal(INS.sort_rows(got["rows"][n, :len(want_rows[n])]), want_rows[n]), n


ROW = ST.ROWS[-1]


@pytest.fixture(scope="module")
def harness():
    """The stream module's harness with the op delay at its floor; `execute` raises it to four times the row's own measured host time."""
    h = ST.Harness()
    h.longest_ms, h.longest_host_ms = 0.0, 0.0
    h.set_delay("op", 0.0)
    return h


def test_the_row_is_in_the_table():
    assert ROW.name == "instance_pair" and ROW.entries == ("fcn8s_op_instance_pair",) and ROW in ST.ROWS


@pytest.mark.parametrize("skew", ST.SKEWS)
def test_instance_pair_on_a_side_stream(skew, harness):
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
        assert np.array_equal(INS.sort_rows(got["rows"][n, :k]), INS.sort_rows(want["rows"][n, :k]))           # the default stream's rows, bit for bit
