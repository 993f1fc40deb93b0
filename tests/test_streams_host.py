"""Completeness of the stream case table (tests/test_streams_gpu.py), on the CPU: every C entry point of include/fcn8s_hip.h whose first
parameter is `void* stream` is named by a row of the table, and the table names nothing else.  An op added later without a stream case
fails here."""
import os
import re

HEADER = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "fcn8s_hip.h")


def stream_entries():
    text = re.sub(r"/\*.*?\*/", " ", open(HEADER).read(), flags=re.S)
    return set(re.findall(r"\b(fcn8s_\w+)\s*\(\s*void\s*\*\s*stream\b", text))


def test_the_header_has_the_entries_this_check_is_about():
    names = stream_entries()
    assert "fcn8s_onehot_to_ids" in names and len(names) >= 45 and all(n == "fcn8s_onehot_to_ids" or n.startswith("fcn8s_op_") for n in names)


def test_every_entry_that_takes_a_stream_has_a_row_in_the_stream_case_table():
    from tests.test_streams_gpu import ROWS
    named = set()
    for r in ROWS:
        assert r.entries, r.name
        named.update(r.entries)
    want = stream_entries()
    assert not want - named, "entry points that take a stream and have no row in tests/test_streams_gpu.py: %s" % sorted(want - named)
    assert not named - want, "rows of tests/test_streams_gpu.py name what the header does not declare with a stream: %s" % sorted(named - want)
