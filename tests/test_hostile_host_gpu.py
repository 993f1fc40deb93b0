"""tests/hostile.py itself: each violation it exists to catch is caught, by the right name and side, and a clean use passes.

torch operations only, on memory the arena owns: no kernel of this project runs and nothing faults -- every access below lands inside the arena's
own allocation (the bands are part of it)."""
import numpy as np
import pytest
import torch

from tests import hostile

pytestmark = pytest.mark.gpu


def raw_of(arena, t):
    """The arena's record of tensor t."""
    return next(it for it in arena.items if it.tensor.data_ptr() == t.data_ptr())


def flat_with_neighbours(arena, t, before=0, after=0):
    """t's elements as one flat view, lengthened by `before` / `after` elements into its bands."""
    it = raw_of(arena, t)
    e = t.element_size()
    return it.raw[it.lo - before * e:it.lo + it.nbytes + after * e].view(t.dtype)


def failures_of(arena):
    with pytest.raises(hostile.HostileMemoryError) as e:
        arena.verify()
    return [(name, kind) for name, kind, _, _ in e.value.failures], e.value


def filled(arena):
    """Two inputs, two outputs and an in-place buffer, the outputs written as a correct op would."""
    rng = np.random.default_rng(0)
    x = arena.inp(rng.standard_normal((3, 5, 7)).astype(np.float32), name="x")
    lab = arena.inp(rng.integers(0, 20, 33).astype(np.uint8), name="labels")
    y = arena.out((3, 5, 7), name="y")
    am = arena.out((33,), torch.int64, name="argmax")
    th = arena.inout(rng.standard_normal(101).astype(np.float32), name="theta")
    y.copy_(2 * x)
    am.copy_(lab.long())
    th.mul_(0.5)
    return x, lab, y, am, th


def test_layout():
    a = hostile.Arena()
    x = np.arange(35, dtype=np.float32).reshape(5, 7)
    for t in (a.inp(x), a.out((3, 3)), a.out((5,), torch.int64), a.out((7,), torch.uint8), a.inout(x)):
        it = raw_of(a, t)
        assert t.data_ptr() % 256 == 0 and t.is_contiguous()
        assert it.lo >= hostile.BAND and it.raw.numel() - it.lo - it.nbytes >= hostile.BAND
    assert hostile.BAND == 1 << 20
    assert np.array_equal(a.items[0].tensor.cpu().numpy(), x)
    assert torch.isnan(a.items[1].tensor).all() and (a.items[2].tensor == -1).all() and (a.items[3].tensor == 255).all()
    assert (a.items[0].raw[:a.items[0].lo] == 255).all()


def test_a_clean_pass():
    a = hostile.Arena()
    filled(a)
    a.out((4, 4), name="not asked for", untouched=True)
    a.verify()


def test_a_store_just_before_an_output_is_caught():
    a = hostile.Arena()
    _, _, y, _, _ = filled(a)
    flat_with_neighbours(a, y, before=1)[0] = 1.0
    got, err = failures_of(a)
    assert got == [("y", "before")]
    assert err.failures[0][3] == 4 and "y: band before" in str(err)          # four bytes before the tensor: its last element's neighbour


def test_a_store_just_after_an_output_is_caught():
    a = hostile.Arena()
    _, _, _, am, _ = filled(a)
    flat_with_neighbours(a, am, after=1)[-1] = 3
    got, err = failures_of(a)
    assert got == [("argmax", "after")]
    assert err.failures[0][2] == 0 and "argmax: band after" in str(err)


def test_a_changed_input_element_is_caught():
    a = hostile.Arena()
    x, lab, _, _, _ = filled(a)
    x[1, 2, 3] += 1.0
    got, err = failures_of(a)
    assert got == [("x", "changed")]
    assert err.failures[0][2] == 4 * (1 * 35 + 2 * 7 + 3)
    lab[32] = 255                                                            # and both at once, each by its name
    assert failures_of(a)[0] == [("x", "changed"), ("labels", "changed")]


def test_an_output_element_left_unwritten_is_caught():
    a = hostile.Arena()
    x = a.inp(np.ones((6, 4), np.float32), name="x")
    y = a.out((6, 4), name="y")
    am = a.out((6,), torch.int64, name="argmax")
    y.copy_(x); am.zero_()
    a.verify()
    b = hostile.Arena()
    y = b.out((6, 4), name="y")
    am = b.out((6,), torch.int64, name="argmax")
    y.view(-1)[:23] = 1.0                                                    # the last element never written
    am[:5] = 0
    got, err = failures_of(b)
    assert got == [("y", "unwritten"), ("argmax", "unwritten")]
    assert err.failures[0][2] == 4 * 23 and err.failures[1][2] == 8 * 5


def test_an_untouched_output_that_is_written_is_caught():
    a = hostile.Arena()
    t = a.out((8,), torch.uint8, name="pidx", untouched=True)
    a.verify()
    t[3] = 2
    assert failures_of(a)[0] == [("pidx", "written")]


def test_an_inout_buffer_has_bands_and_no_intact_check():
    a = hostile.Arena()
    _, _, _, _, th = filled(a)
    a.verify()                                                               # theta was halved in place: not an offence
    flat_with_neighbours(a, th, after=1)[-1] = 0.0
    assert failures_of(a)[0] == [("theta", "after")]


def test_a_sum_that_reads_one_element_too_far_is_nan():
    """No verify() failure here: a read leaves no trace in memory.  The fence value shows in the result instead."""
    a = hostile.Arena()
    x = a.inp(np.ones(1000, np.float32), name="x")
    assert float(x.sum()) == 1000.0
    assert np.isnan(float(flat_with_neighbours(a, x, after=1).sum()))
    assert np.isnan(float(flat_with_neighbours(a, x, before=1).sum()))
    lab = a.inp(np.zeros(64, np.uint8), name="labels")
    assert int(flat_with_neighbours(a, lab, after=1)[-1]) == 255               # a label read past the end is the ignore id
    a.verify()
